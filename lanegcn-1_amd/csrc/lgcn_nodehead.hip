// Head of an Att block whose targets are the lane nodes (lgcn_node_head: A2M's first launch), weight-stationary.  One grid
// runs up to LGCN_MAX_MULTI row-chain problems, each of one of three forms over its own rows x (one LGCN_REL_IDENT
// relation):
//   head   : y = ReLU(GN1(x W^T + rank-4 update))                          (A2M.meta, reference lanegcn.py:387-395)
//            u = ReLU(GN_q(y W_q^T)) W_u^T                                 (optional: layer 0's U, lgcn.h ch_*)
//   u-chain: out = ReLU(GN1(x W^T)) W_2^T                                  (Att's U over its target rows, lanegcn.py:696-699)
//   plain  : out = x W^T                                                   (Att's V over its context rows)
// Problems over the same rows (same src, same n_rows; not the head) share their tiles -- up to two plain problems and a
// u-chain: the rows are read and split once and the weights run one after the other, the plain ones first.  That is the
// actor side of A2M's first launch (V0, V1, and M2A's U0 riding along): 34 tiles at S2 instead of 68, which with the
// head's 216 leaves every workgroup a CU of its own (250 <= 256).
//
// The generic row block (lgcn_rowmlp_bf.hip) runs these on 32-row tiles whose four MFMA waves stream every weight image
// L2 -> VGPR through a one- or two-deep fragment ring; for the head that is three dependent GEMMs of four dependent round
// trips each.  Here, as in lgcn_nodetail.hip (whose machinery this shares: lgcn_wslice.hpp), a workgroup takes a 48-row
// tile and each of its 8 waves owns the 16-channel slice `wave` of EVERY weight over the full K.  Two slices are in
// flight: a tile's first two weights are requested behind its row loads, and the head's third (W_u) goes into the slice
// of the first once that GEMM's MFMAs are issued and its accumulators are in the tile, two GEMMs before it is used.
//
// Arithmetic: the row block's, to the bit.  One fp32 accumulator per output element that starts at 0 and takes K-steps
// 0..3 in order and the plane products in Fmt<F>::PA / PB order (kstep of lgcn_mma_bf.hpp); the rank-4 update is
// rank4_update of lgcn_mma_bf.hpp on the accumulator element, as in the row block; GroupNorm goes through the fp32 LDS
// tile and row_gn of lgcn_tile.hpp on the same lanes of a row (two barriers per GEMM); every final GEMM's rows leave
// from the accumulators as 64-byte row segments.
#include "lgcn_common.hpp"
#include "lgcn_mma_bf.hpp"
#include "lgcn_wslice.hpp"

namespace lgcn {

enum { kHeadOnly = 0, kHeadChain = 1, kUChain = 2, kPlain = 3 };

// One tile range of the grid.  By kind (w[1] then w[2] are what a tile's chain runs through):
//   kHeadOnly / kHeadChain: w[0] = W, gn[0] = GN1, out[0] = y;  kHeadChain: w[1] = W_q, gn[1] = GN_q, w[2] = W_u, out[1] = u
//                           (kHeadOnly: w[1] = W, requested and not used)
//   kUChain               : w[1] = W, gn[1] = GN1, w[2] = W_2, out[1] = out, and n_plain = 0..2 plain problems in front
//   kPlain                : n_plain = 1..2 plain problems pw[i] -> pout[i]
struct HeadSlot {
    const float *src;
    int64_t n_rows;
    int kind, tiles, n_plain;
    float eps;
    const float *w[3];
    const float *gn_g[2], *gn_b[2];
    const float *w4, *x4_a, *x4_b, *x4_c;
    float *out[2];
    const float *pw[2];
    float *pout[2];
};

struct NodeHeadArgs {
    HeadSlot s[LGCN_MAX_MULTI];
    int n;
};

template <int F>
struct NodeHeadSmem {
    using TL = Tile<kNtRB, F>;
    static constexpr int A0 = 0;                           // planes of x, then of every later GEMM's operand rows
    static constexpr int T = TL::ABUF_BYTES;               // fp32 accumulator tile
    static constexpr int GN = T + TL::T_BYTES;             // gn[0] g|b, gn[1] g|b
    static constexpr int X4 = GN + 4 * kC * 4;             // the tile's rows of the rank-4 update: turn.x, turn.y, control, intersect
    static constexpr int W4 = X4 + TL::ROWS * 16;          // the weight's four columns of it, per channel
    static constexpr int BYTES = W4 + kC * 16;
};

// The tile's rows: thread -> (row = 16 it + tid / 32, 4 channels); row indices are clamped for the last tile (such rows
// are computed and never stored).
__device__ __forceinline__ void rows_request(f32x4 (&v)[kNtRB], const HeadSlot &p, int64_t row0, int tid) {
    const f32x4 *__restrict__ xa = reinterpret_cast<const f32x4 *>(p.src);
#pragma unroll
    for (int it = 0; it < kNtRB; ++it) {
        const int64_t n = row0 + 16 * it + (tid >> 5);
        v[it] = xa[(n < p.n_rows ? n : p.n_rows - 1) * (kC / 4) + (tid & 31)];
    }
}

template <int F>
__device__ __forceinline__ void rows_split(uint16_t *A0, const f32x4 (&v)[kNtRB], int tid) {
#pragma unroll
    for (int it = 0; it < kNtRB; ++it)
        split_store<F>(A0, Tile<kNtRB, F>::PLANE, 16 * it + (tid >> 5), 4 * (tid & 31), make_float4(v[it][0], v[it][1], v[it][2], v[it][3]));
}

// out = rows W^T for the operand rows in A0 (behind a barrier), stored from the accumulators
template <int F>
__device__ __forceinline__ void plain_gemm(float *__restrict__ out, const uint16_t *A0, const WSlice<F> &w, int64_t row0, int64_t n_rows,
                                           int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    f32x4 acc[kNtRB][1];
    acc_zero(acc);
    gemm_slice<F>(A0, w, lane, acc);
    __builtin_amdgcn_sched_barrier(0);                        // the rows' addresses are formed behind the MFMAs, not held through them
    acc_to_global(out, acc, row0, n_rows, lane, wave);
}

// out[1] = ReLU(GN(rows W_1^T)) W_2^T for the operand rows in A0 (behind a barrier), GN's g | b at gq: two barriers, the
// result stored from the accumulators.  Row phase: threads 0..383, eight per row.
template <int F>
__device__ __forceinline__ void chain_tail(const HeadSlot &p, uint16_t *A0, float *T, const float *gq, const WSlice<F> &w1,
                                           const WSlice<F> &w2, int64_t row0, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    f32x4 acc[kNtRB][1];
    acc_zero(acc);
    gemm_slice<F>(A0, w1, lane, acc);
    acc_to_tile(T, acc, lane, wave);                          // T's readers, if any, passed the barrier in front of this call
    lds_barrier();
    if (tid < 8 * Tile<kNtRB, F>::ROWS) {
        RowVals r = row_load(T, tid);
        row_gn<F != 1>(r, tid, gq, gq + kC, p.eps);
        row_relu(r);
        row_split_store<F>(A0, Tile<kNtRB, F>::PLANE, tid >> 3, tid, r);      // A0's readers passed the barrier above
    }
    lds_barrier();
    acc_zero(acc);
    gemm_slice<F>(A0, w2, lane, acc);
    __builtin_amdgcn_sched_barrier(0);                        // the rows' addresses are formed behind the MFMAs, not held through them
    acc_to_global(p.out[1], acc, row0, p.n_rows, lane, wave);
}

// <= 128 VGPRs: a second workgroup, or another forward's kernel, shares the CU.
template <int F>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_node_head(const NodeHeadArgs m) {
    using SM = NodeHeadSmem<F>;
    using TL = Tile<kNtRB, F>;
    constexpr int ROWS = TL::ROWS;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SM::BYTES];
    uint16_t *A0 = reinterpret_cast<uint16_t *>(smem + SM::A0);
    float *T = reinterpret_cast<float *>(smem + SM::T);
    float *gnp = reinterpret_cast<float *>(smem + SM::GN);
    float4 *x4s = reinterpret_cast<float4 *>(smem + SM::X4);
    float4 *w4s = reinterpret_cast<float4 *>(smem + SM::W4);

    // the workgroup's slot and tile: uniform over the workgroup, so all of its waves meet the same barriers
    int b = blockIdx.x, si = 0;
    while (si + 1 < m.n && b >= m.s[si].tiles) { b -= m.s[si].tiles; ++si; }
    const HeadSlot &p = m.s[si];
    const int kind = p.kind;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = xcd_chunk_remap(b, p.tiles);
    const int64_t row0 = (int64_t)tile * ROWS;

    // Every kind: one barrier behind a prologue that requests the tile's rows and, behind them, its first two weight slices.
    f32x4 v[kNtRB];
    f32x4 acc[kNtRB][1];
    WSlice<F> wa, wb;
    if (kind == kPlain) {
        const int np = p.n_plain;
        rows_request(v, p, row0, tid);
        load_slice<F>(wa, p.pw[0], wave, lane);
        load_slice<F>(wb, p.pw[np - 1], wave, lane);          // (one problem: its weight again, not used)
        rows_split<F>(A0, v, tid);
        lds_barrier();
        plain_gemm<F>(p.pout[0], A0, wa, row0, p.n_rows, tid);
        if (np == 2) plain_gemm<F>(p.pout[1], A0, wb, row0, p.n_rows, tid);
        return;
    }
    if (kind == kUChain) {
        // the weights in the order they run: the plain ones, W, W_2.  The chain takes wa then wb, so a single plain weight
        // starts in wb; a slice is refilled with the weight two GEMMs ahead once its MFMAs are issued.
        const int np = p.n_plain;
        rows_request(v, p, row0, tid);
        load_slice<F>(wa, np == 2 ? p.pw[0] : p.w[1], wave, lane);
        load_slice<F>(wb, np == 2 ? p.pw[1] : np == 1 ? p.pw[0] : p.w[2], wave, lane);
        if (tid < kC) { gnp[2 * kC + tid] = p.gn_g[1][tid]; gnp[3 * kC + tid] = p.gn_b[1][tid]; }
        rows_split<F>(A0, v, tid);
        lds_barrier();
        if (np == 2) {
            plain_gemm<F>(p.pout[0], A0, wa, row0, p.n_rows, tid);
            load_slice<F>(wa, p.w[1], wave, lane);
        }
        if (np >= 1) {
            plain_gemm<F>(p.pout[np - 1], A0, wb, row0, p.n_rows, tid);
            load_slice<F>(wb, p.w[2], wave, lane);
        }
        chain_tail<F>(p, A0, T, gnp + 2 * kC, wa, wb, row0, tid);
        return;
    }

    // ---- the head: GEMM, the rank-4 update on its accumulators, GN1, ReLU; then the chain from its rows
    const bool chain = kind == kHeadChain, r4 = p.w4 != nullptr;
    rows_request(v, p, row0, tid);
    load_slice<F>(wa, p.w[0], wave, lane);
    load_slice<F>(wb, p.w[1], wave, lane);                    // W_q (without a chain: W again, not used)
    if (tid < kC) {
        gnp[tid] = p.gn_g[0][tid]; gnp[kC + tid] = p.gn_b[0][tid];
        if (chain) { gnp[2 * kC + tid] = p.gn_g[1][tid]; gnp[3 * kC + tid] = p.gn_b[1][tid]; }
        if (r4) w4s[tid] = reinterpret_cast<const float4 *>(p.w4)[tid];
    } else if (r4 && tid < kC + ROWS) {
        const int64_t n = row0 + (tid - kC);
        const int64_t nc = n < p.n_rows ? n : p.n_rows - 1;
        const float2 tu = reinterpret_cast<const float2 *>(p.x4_a)[nc];
        x4s[tid - kC] = make_float4(tu.x, tu.y, p.x4_b[nc], p.x4_c[nc]);
    }
    rows_split<F>(A0, v, tid);
    lds_barrier();

    acc_zero(acc);
    gemm_slice<F>(A0, wa, lane, acc);
    __builtin_amdgcn_sched_barrier(0);                        // the update's rows are read behind the MFMAs, not held through them
    if (r4) {
        const float4 wc = w4s[16 * wave + (lane & 15)];
#pragma unroll
        for (int rb = 0; rb < kNtRB; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 x = x4s[16 * rb + 4 * (lane >> 4) + i];
                acc[rb][0][i] = rank4_update(acc[rb][0][i], make_float2(x.x, x.y), x.z, x.w, wc);
            }
    }
    acc_to_tile(T, acc, lane, wave);
    if (chain) load_slice<F>(wa, p.w[2], wave, lane);         // W_u into the slice this GEMM has consumed: used three barriers on
    lds_barrier();
    if (tid < 8 * ROWS) {
        const int64_t n = row0 + (tid >> 3);
        RowVals r = row_load(T, tid);
        row_gn<F != 1>(r, tid, gnp, gnp + kC, p.eps);
        row_relu(r);
        if (n < p.n_rows) row_store_global(p.out[0] + n * kC, tid, r);
        if (chain) row_split_store<F>(A0, TL::PLANE, tid >> 3, tid, r);      // A0's readers passed the barrier above
    }
    if (!chain) return;
    lds_barrier();
    chain_tail<F>(p, A0, T, gnp + 2 * kC, wb, wa, row0, tid);
}

// The form of a problem (kHeadOnly stands for both head kinds), or -1 for anything this launch does not run.
static int head_form(const lgcn_agg_mlp_t &p) {
    if (p.n_rel != 1 || p.rel[0].mode != LGCN_REL_IDENT) return -1;
    if (p.ch_wv || p.ch_v_out || p.out_pre || p.out_mid || p.out_pre2 || p.tile_rb != 0) return -1;
    if (p.flags == (LGCN_F_GN1 | LGCN_F_RELU1)) return kHeadOnly;
    if (p.w4 || p.ch_wu) return -1;
    if (p.flags == (LGCN_F_GN1 | LGCN_F_RELU1 | LGCN_F_GEMM2)) return kUChain;
    return p.flags == 0 ? kPlain : -1;
}

}  // namespace lgcn

extern "C" int lgcn_node_head(const lgcn_agg_mlp_t *const *ps, int n, void *stream) {
    using namespace lgcn;
    LGCN_CHECK_PTR(ps);
    if (n < 1 || n > LGCN_MAX_MULTI) return LGCN_EINVAL;
    for (int i = 0; i < n; ++i) LGCN_CHECK_PTR(ps[i]);
    const int mma = ps[0]->mma;
    if (mma != LGCN_MMA_F16X2 && mma != LGCN_MMA_BF16) return LGCN_ESHAPE;
    for (int i = 0; i < n; ++i) if (ps[i]->mma != mma) return LGCN_ESHAPE;
    int form[LGCN_MAX_MULTI];
    for (int i = 0; i < n; ++i) if ((form[i] = head_form(*ps[i])) < 0) return LGCN_ESHAPE;
    for (int i = 0; i < n; ++i) {
        if (ps[i]->n_rows < 0) return LGCN_EINVAL;
        if (ps[i]->n_rows > 0x7fffffff) return LGCN_ESHAPE;
    }
    // every required pointer of every non-empty problem, then their alignment
    const void *need[LGCN_MAX_MULTI * 16];
    int n_need = 0;
    for (int i = 0; i < n; ++i) {
        const lgcn_agg_mlp_t &p = *ps[i];
        if (p.n_rows == 0) continue;
        for (const void *q : {(const void *)p.rel[0].src, (const void *)p.rel[0].wp, (const void *)p.out}) need[n_need++] = q;
        if (form[i] != kPlain) { need[n_need++] = p.gn1_g; need[n_need++] = p.gn1_b; }
        if (form[i] == kUChain) need[n_need++] = p.wp2;
        if (form[i] == kHeadOnly && p.w4) need[n_need++] = p.w4;
        if (form[i] == kHeadOnly && p.ch_wu)
            for (const void *q : {(const void *)p.ch_wq, (const void *)p.ch_gq_g, (const void *)p.ch_gq_b, (const void *)p.ch_wu, (const void *)p.ch_u_out})
                need[n_need++] = q;
    }
    for (int k = 0; k < n_need; ++k) LGCN_CHECK_PTR(need[k]);
    for (int i = 0; i < n; ++i)      // the rank-4 rows: [N,2], [N], [N] fp32, read as float2 / float
        if (ps[i]->n_rows > 0 && form[i] == kHeadOnly && ps[i]->w4) {
            LGCN_CHECK_PTR(ps[i]->x4_a); LGCN_CHECK_PTR(ps[i]->x4_b); LGCN_CHECK_PTR(ps[i]->x4_c);
        }
    for (int k = 0; k < n_need; ++k) LGCN_CHECK_ALIGN16(need[k]);

    NodeHeadArgs a{};
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const lgcn_agg_mlp_t &p = *ps[i];
        if (p.n_rows == 0) continue;
        HeadSlot *s = nullptr;
        if (form[i] != kHeadOnly)      // a problem over the rows of an earlier one rides in its tiles, while that slot has room
            for (int k = 0; k < a.n && s == nullptr; ++k)
                if (a.s[k].kind >= kUChain && a.s[k].src == p.rel[0].src && a.s[k].n_rows == p.n_rows &&
                    (form[i] == kPlain ? a.s[k].n_plain < 2 : a.s[k].kind == kPlain))
                    s = &a.s[k];
        if (s == nullptr) {
            s = &a.s[a.n++];
            s->src = p.rel[0].src;
            s->n_rows = p.n_rows;
            s->tiles = (int)((p.n_rows + 16 * kNtRB - 1) / (16 * kNtRB));
            s->kind = kPlain;
            total += s->tiles;
        }
        if (form[i] == kHeadOnly) {
            s->kind = p.ch_wu ? kHeadChain : kHeadOnly;
            s->eps = p.eps;
            s->w[0] = s->w[1] = p.rel[0].wp; s->gn_g[0] = p.gn1_g; s->gn_b[0] = p.gn1_b; s->out[0] = p.out;
            s->w4 = p.w4; s->x4_a = p.x4_a; s->x4_b = p.x4_b; s->x4_c = p.x4_c;
            if (p.ch_wu) { s->w[1] = p.ch_wq; s->gn_g[1] = p.ch_gq_g; s->gn_b[1] = p.ch_gq_b; s->w[2] = p.ch_wu; s->out[1] = p.ch_u_out; }
        } else if (form[i] == kUChain) {
            s->kind = kUChain;
            s->eps = p.eps;
            s->w[1] = p.rel[0].wp; s->gn_g[1] = p.gn1_g; s->gn_b[1] = p.gn1_b; s->w[2] = p.wp2; s->out[1] = p.out;
        } else {
            s->pw[s->n_plain] = p.rel[0].wp;
            s->pout[s->n_plain++] = p.out;
        }
    }
    if (a.n == 0) return LGCN_OK;
    hipStream_t st = (hipStream_t)stream;
    if (mma == LGCN_MMA_F16X2) hipLaunchKernelGGL((k_node_head<1>), dim3((unsigned)total), dim3(512), 0, st, a);
    else hipLaunchKernelGGL((k_node_head<2>), dim3((unsigned)total), dim3(512), 0, st, a);
    return launch_status();
}
