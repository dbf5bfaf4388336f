// Node-side tail of an Att block whose targets outnumber its context rows (lgcn_node_tail: A2M, the lane nodes),
// weight-stationary:
//   S[n] = sum_{p in [rowptr[n], rowptr[n+1])} m[p]                        (pair order)
//   y    = ReLU(GN2(ReLU(GN1(a W_agt^T + S W_c1^T)) W2^T) + res)          (reference lanegcn.py:702-709)
//   u    = ReLU(GN_q(y W_q^T)) W_u^T                                       (optional: the next layer's U, lgcn.h ch_*)
//
// The generic row block (lgcn_rowmlp_bf.hip) runs this chain of three to five dependent 128 x 128 GEMMs on 32-row tiles
// whose four MFMA waves stream every weight image L2 -> VGPR through a one- or two-deep fragment ring while the other
// four waves gather or wait: a tile sits through a dozen or more dependent L2 round trips.  Here a workgroup takes a
// 48-row tile (216 workgroups over the 10,368 lane nodes of S2, one per CU), and each of its 8 waves owns the
// 16-channel slice `wave` of EVERY weight over the full K (NP x 4 fragments: 32 VGPRs in f16x2).  Two slices are in
// flight: the first two weights are requested behind the row loads at kernel start, and the slice a GEMM has consumed
// is refilled with the weight two GEMMs ahead before the next GEMM's MFMAs are issued, so no GEMM waits for a weight.
//
// Arithmetic: the row block's, to the bit.  One fp32 accumulator per output element that starts at 0 and takes
// relation 0 then relation 1, K-steps 0..3 in order and the plane products in Fmt<F>::PA / PB order (kstep of
// lgcn_mma_bf.hpp, shared); GroupNorm(1, 128) needs a row's 128 channels, which lie in all 8 waves, so the accumulators
// go through the fp32 LDS tile T and the row phase (thread -> row t >> 3, columns 4 (t & 7) + 32 j) is row_gn of
// lgcn_tile.hpp on the same lanes of a row as in the row block: the same sums in the same order.  That costs the row
// block's two barriers per GEMM; the rows go back to LDS as operand planes (split_store).
#include "lgcn_common.hpp"
#include "lgcn_mma_bf.hpp"
#include "lgcn_wslice.hpp"

namespace lgcn {

template <int F>
struct NodeTailSmem {
    using TL = Tile<kNtRB, F>;
    static constexpr int A0 = 0;                           // planes of a, then of every later GEMM's operand rows
    static constexpr int A1 = TL::ABUF_BYTES;              // planes of S
    static constexpr int T = 2 * TL::ABUF_BYTES;           // fp32 accumulator tile
    static constexpr int GN = T + TL::T_BYTES;             // gn1 g|b, gn2 g|b, chained query g|b
    static constexpr int BYTES = GN + 6 * kC * 4;
};

// <= 128 VGPRs: a second workgroup, or another forward's kernel, shares the CU.
template <int F>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_node_tail(const lgcn_agg_mlp_t p, int n_tiles) {
    using SM = NodeTailSmem<F>;
    using TL = Tile<kNtRB, F>;
    constexpr int ROWS = TL::ROWS;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SM::BYTES];
    uint16_t *A0 = reinterpret_cast<uint16_t *>(smem + SM::A0);
    uint16_t *A1 = reinterpret_cast<uint16_t *>(smem + SM::A1);
    float *T = reinterpret_cast<float *>(smem + SM::T);
    float *gnp = reinterpret_cast<float *>(smem + SM::GN);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = xcd_chunk_remap(blockIdx.x, n_tiles);
    const int64_t row0 = (int64_t)tile * ROWS;
    const bool chain = p.ch_wu != nullptr;            // uniform over the launch

    // ---- prologue, one barrier: the tile's rows of a and the bounds of their pair ranges, the first two weight slices
    // behind them, then the pair rows (whose addresses need the bounds).  thread -> (row = 16 it + tid / 32, 4 channels);
    // row indices are clamped for the last tile (such rows are computed and never stored).
    const int hr = tid >> 5, l = tid & 31;
    const f32x4 *__restrict__ xa = reinterpret_cast<const f32x4 *>(p.rel[0].src);
    const f32x4 *__restrict__ xm = reinterpret_cast<const f32x4 *>(p.rel[1].src);
    const f32x4 *arow_p = xa + l;       // a valid address for the loads of a target without pairs
    f32x4 v[kNtRB];
    int b[kNtRB], e[kNtRB];
#pragma unroll
    for (int it = 0; it < kNtRB; ++it) {
        const int64_t n = row0 + 16 * it + hr;
        v[it] = xa[(n < p.n_rows ? n : p.n_rows - 1) * (kC / 4) + l];
        b[it] = p.rowptr[n < p.n_rows ? n : p.n_rows];
        e[it] = p.rowptr[n + 1 < p.n_rows ? n + 1 : p.n_rows];
    }
    WSlice<F> w0, w1;
    load_slice<F>(w0, p.rel[0].wp, wave, lane);
    load_slice<F>(w1, p.rel[1].wp, wave, lane);
    if (tid < kC) {
        gnp[tid] = p.gn1_g[tid]; gnp[kC + tid] = p.gn1_b[tid];
        gnp[2 * kC + tid] = p.gn2_g[tid]; gnp[3 * kC + tid] = p.gn2_b[tid];
        if (chain) { gnp[4 * kC + tid] = p.ch_gq_g[tid]; gnp[5 * kC + tid] = p.ch_gq_b[tid]; }
    }
    // S in pair order, as the LGCN_REL_RANGE gather of the row block sums it: first and second pair rows of the thread's
    // three targets in one round trip (a target without one reads row 0 of a instead: a valid address, no branch),
    // the rest four loads at a time.
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    auto mrow = [&](int j) -> const f32x4 * { return xm + ((uint64_t)(unsigned)j << 5) + l; };
    f32x4 s[kNtRB], x[kNtRB];
#pragma unroll
    for (int it = 0; it < kNtRB; ++it) s[it] = *(b[it] < e[it] ? mrow(b[it]) : arow_p);
#pragma unroll
    for (int it = 0; it < kNtRB; ++it) x[it] = *(b[it] + 1 < e[it] ? mrow(b[it] + 1) : arow_p);
#pragma unroll
    for (int it = 0; it < kNtRB; ++it) split_store<F>(A0, TL::PLANE, 16 * it + hr, 4 * l, make_float4(v[it][0], v[it][1], v[it][2], v[it][3]));
    bool more = false;
#pragma unroll
    for (int it = 0; it < kNtRB; ++it) {
        s[it] = b[it] < e[it] ? s[it] : zero;
        s[it] = s[it] + (b[it] + 1 < e[it] ? x[it] : zero);
        more = more | (b[it] + 2 < e[it]);
    }
    if (__any(more)) {
#pragma unroll
        for (int it = 0; it < kNtRB; ++it) {
            int j = b[it] + 2;
            const int end = e[it];
            f32x4 a = s[it];
            for (; j + 3 < end; j += 4) {
                const f32x4 y0 = *mrow(j), y1 = *mrow(j + 1), y2 = *mrow(j + 2), y3 = *mrow(j + 3);
                a = (((a + y0) + y1) + y2) + y3;
            }
            for (; j < end; ++j) a = a + *mrow(j);
            s[it] = a;
        }
    }
#pragma unroll
    for (int it = 0; it < kNtRB; ++it) split_store<F>(A1, TL::PLANE, 16 * it + hr, 4 * l, make_float4(s[it][0], s[it][1], s[it][2], s[it][3]));
    lds_barrier();

    // ---- GEMM 1: a W_agt^T + S W_c1^T into one accumulator; each slice is refilled once its MFMAs are issued
    f32x4 acc[kNtRB][1];
    acc_zero(acc);
    gemm_slice<F>(A0, w0, lane, acc);
    load_slice<F>(w0, p.wp2, wave, lane);
    gemm_slice<F>(A1, w1, lane, acc);
    if (chain) load_slice<F>(w1, p.ch_wq, wave, lane);
    acc_to_tile(T, acc, lane, wave);
    lds_barrier();

    // ---- row phases: threads 0..383, eight per row
    const bool has_row = tid < 8 * ROWS;
    const int row = tid >> 3;
    const int64_t n = row0 + row;
    const bool live = has_row && n < p.n_rows;
    if (has_row) {
        RowVals r = row_load(T, tid);
        row_gn<F != 1>(r, tid, gnp, gnp + kC, p.eps);
        row_relu(r);
        row_split_store<F>(A0, TL::PLANE, row, tid, r);      // A0's readers passed the barrier above
    }
    lds_barrier();

    // ---- GEMM 2
    acc_zero(acc);
    gemm_slice<F>(A0, w0, lane, acc);
    RowVals resv;
    if (has_row) {
        // the residual rows, requested once the MFMAs are issued: they arrive under the barrier and GroupNorm's statistics
        const float *rp_ = p.res + (n < p.n_rows ? n : p.n_rows - 1) * kC + 4 * (tid & 7);
#pragma unroll
        for (int j = 0; j < 4; ++j) resv.v[j] = *reinterpret_cast<const float4 *>(rp_ + 32 * j);
    }
    acc_to_tile(T, acc, lane, wave);                          // T's readers passed the barrier above
    lds_barrier();
    if (has_row) {
        RowVals r = row_load(T, tid);
        row_gn<F != 1>(r, tid, gnp + 2 * kC, gnp + 3 * kC, p.eps);
        row_add(r, resv);
        row_relu(r);
        if (live) row_store_global(p.out + n * kC, tid, r);
        if (chain) row_split_store<F>(A0, TL::PLANE, row, tid, r);
    }
    if (!chain) return;
    load_slice<F>(w0, p.ch_wu, wave, lane);                   // used two barriers on
    lds_barrier();

    // ---- chained U of the next layer: ReLU(GN_q(y W_q^T)) W_u^T, stored from the accumulators (64-byte row segments)
    acc_zero(acc);
    gemm_slice<F>(A0, w1, lane, acc);
    acc_to_tile(T, acc, lane, wave);
    lds_barrier();
    if (has_row) {
        RowVals r = row_load(T, tid);
        row_gn<F != 1>(r, tid, gnp + 4 * kC, gnp + 5 * kC, p.eps);
        row_relu(r);
        row_split_store<F>(A0, TL::PLANE, row, tid, r);
    }
    lds_barrier();
    acc_zero(acc);
    gemm_slice<F>(A0, w0, lane, acc);
    acc_to_global(p.ch_u_out, acc, row0, p.n_rows, lane, wave);
}

}  // namespace lgcn

extern "C" int lgcn_node_tail(const lgcn_agg_mlp_t *ph, void *stream) {
    using namespace lgcn;
    LGCN_CHECK_PTR(ph);
    const lgcn_agg_mlp_t &p = *ph;
    if (p.mma != LGCN_MMA_F16X2 && p.mma != LGCN_MMA_BF16) return LGCN_ESHAPE;
    constexpr int kFull = LGCN_F_GN1 | LGCN_F_RELU1 | LGCN_F_GEMM2 | LGCN_F_GN2 | LGCN_F_RES | LGCN_F_RELU2;
    if (p.n_rel != 2 || p.rel[0].mode != LGCN_REL_IDENT || p.rel[1].mode != LGCN_REL_RANGE || p.flags != kFull) return LGCN_ESHAPE;
    if (p.ch_wv || p.ch_v_out || p.w4 || p.out_pre || p.out_mid || p.out_pre2 || p.tile_rb != 0) return LGCN_ESHAPE;
    if (p.n_rows < 0) return LGCN_EINVAL;
    if (p.n_rows > 0x7fffffff) return LGCN_ESHAPE;
    if (p.n_rows == 0) return LGCN_OK;
    const void *need[] = {p.rel[0].src, p.rel[0].wp, p.rel[1].src, p.rel[1].wp, p.rowptr, p.gn1_g, p.gn1_b,
                          p.wp2, p.gn2_g, p.gn2_b, p.res, p.out};
    for (const void *q : need) LGCN_CHECK_PTR(q);
    for (const void *q : need) if (q != p.rowptr) LGCN_CHECK_ALIGN16(q);
    if (p.ch_wu) {
        const void *q[] = {p.ch_wq, p.ch_gq_g, p.ch_gq_b, p.ch_wu, p.ch_u_out};
        for (const void *c : q) { LGCN_CHECK_PTR(c); LGCN_CHECK_ALIGN16(c); }
    }
    const int n_tiles = (int)((p.n_rows + 16 * kNtRB - 1) / (16 * kNtRB));
    hipStream_t st = (hipStream_t)stream;
    if (p.mma == LGCN_MMA_F16X2) hipLaunchKernelGGL((k_node_tail<1>), dim3(n_tiles), dim3(512), 0, st, p, n_tiles);
    else hipLaunchKernelGGL((k_node_tail<2>), dim3(n_tiles), dim3(512), 0, st, p, n_tiles);
    return launch_status();
}
