// Floating-point path of the LaneGCN hot path on gfx950 (MI355X):
// fused row-block kernels built from three tile primitives
//   (1) gather-sum of 128-channel rows into a 32 x 128 LDS tile,
//   (2) 32 x 128 x K tile GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 fma chain),
//   (3) per-row GroupNorm(1,128) / ReLU / residual over the LDS tile.
// Workgroup tile = 32 rows x 128 output channels; wave w of the 4 MFMA waves
// owns output channels [32w, 32w+32) and streams its own slice of the packed
// weight straight from L2 to registers (no wave shares a weight element);
// the A operand (gathered rows) is the shared, LDS-resident one.
#include "lgcn_common.hpp"
#include "lgcn_tile.hpp"

namespace lgcn {

constexpr int kTM32 = 32;                  // rows of one f32-MFMA tile (two CSR sub-tiles)
constexpr int kTileFloats = kTM32 * kLDA;  // one 32 x (128+4) LDS tile

// acc[32 x 32 block of this wave] += A[32 x 8*nq] * Wpacked
// A operand of 32x32x2: lane l holds A[l & 31][k = l >> 5]; B operand holds
// B[k = l >> 5][l & 31].  With one float4 per lane per 8 k's, step j of the
// q-th group contracts k = 8q + 4(l >> 5) + j on both operands.
__device__ __forceinline__ void tile_gemm(const float *__restrict__ A, const float4 *__restrict__ wp_wave,
                                          f32x16 &acc, int lane, int nq) {
    const float *arow = A + (lane & 31) * kLDA + 4 * (lane >> 5);
    const float4 *b = wp_wave + lane;
#pragma unroll 4
    for (int q = 0; q < nq; ++q) {
        const float4 a = *reinterpret_cast<const float4 *>(arow + 8 * q);
        const float4 w = b[q * 64];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc, 0, 0, 0);
    }
}

// C/D layout of 32x32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ void acc_to_lds(float *T, const f32x16 &acc, int lane, int wave) {
    float *p = T + 32 * wave + (lane & 31);
#pragma unroll
    for (int i = 0; i < 16; ++i) p[acc_row(i, lane) * kLDA] = acc[i];
}

// ------------------------------------------------------------ packing -----
__global__ __launch_bounds__(256) void k_pack_weight(const float *__restrict__ W, int ld, int k_real, int k_pad,
                                                     float *__restrict__ out, int transpose) {
    const int nq = k_pad >> 3;
    const int total = 4 * nq * 64 * 4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int j = i & 3, lane = (i >> 2) & 63, q = (i >> 8) % nq, w = (i >> 8) / nq;
        const int row = 32 * w + (lane & 31), k = 8 * q + 4 * (lane >> 5) + j;
        out[i] = k < k_real ? (transpose ? W[(int64_t)k * ld + row] : W[(int64_t)row * ld + k]) : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_pack_weight_batch(const lgcn_pack_job_t *__restrict__ jobs) {
    const lgcn_pack_job_t job = jobs[blockIdx.y];
    float *__restrict__ out = reinterpret_cast<float *>(job.out);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // < 128 * 128
    const int j = i & 3, lane = (i >> 2) & 63, q = (i >> 8) % (kC >> 3), w = (i >> 8) / (kC >> 3);
    const int row = 32 * w + (lane & 31), k = 8 * q + 4 * (lane >> 5) + j;
    out[i] = job.transpose ? job.W[(int64_t)k * job.ld + row] : job.W[(int64_t)row * job.ld + k];
}

// ------------------------------------------------------------ agg_mlp -----
// 8 waves: waves 0-3 run the MFMA chain of relation i while waves 4-7 gather
// relation i+1 into the other LDS buffer (one barrier per relation).
__device__ __forceinline__ void gather_rel(float *__restrict__ Abuf, const lgcn_agg_mlp_t &p, int ri, int tile,
                                           int gt /*0..255*/) {
    const float4 *__restrict__ src = reinterpret_cast<const float4 *>(p.rel[ri].src);
    const int mode = p.rel[ri].mode;
    const int hw = gt >> 5, l = gt & 31;
    int b[4], e[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + hw;
        const int64_t n = (int64_t)tile * kTM32 + row;
        b[it] = 0; e[it] = 0;
        if (n < p.n_rows) {
            if (mode == LGCN_REL_CSR) {   // 32-row tile = CSR sub-tiles 2*tile, 2*tile+1
                const int64_t k = (((int64_t)tile * 2 + (row >> 4)) * p.n_rel_csr + p.rel[ri].ridx) * 16 + (row & 15);
                b[it] = p.rowptr[k]; e[it] = p.rowptr[k + 1];
            } else if (mode == LGCN_REL_RANGE) {
                b[it] = p.rowptr[n]; e[it] = p.rowptr[n + 1];
            } else {
                b[it] = (int)n; e[it] = (int)n + 1;
            }
        }
    }
    float4 s[4];
    // first edge of each of the 4 rows: independent loads in flight together
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        s[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b[it] < e[it]) {
            const int idx = mode == LGCN_REL_CSR ? p.col[b[it]] : b[it];
            s[it] = src[(int64_t)idx * 32 + l];
        }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        int j = b[it] + 1;
        for (; j + 1 < e[it]; j += 2) {  // two loads in flight, summed in index order
            const int i0 = mode == LGCN_REL_CSR ? p.col[j] : j;
            const int i1 = mode == LGCN_REL_CSR ? p.col[j + 1] : j + 1;
            const float4 x0 = src[(int64_t)i0 * 32 + l];
            const float4 x1 = src[(int64_t)i1 * 32 + l];
            s[it] = f4add(f4add(s[it], x0), x1);
        }
        if (j < e[it]) {
            const int i0 = mode == LGCN_REL_CSR ? p.col[j] : j;
            s[it] = f4add(s[it], src[(int64_t)i0 * 32 + l]);
        }
        *reinterpret_cast<float4 *>(Abuf + (it * 8 + hw) * kLDA + 4 * l) = s[it];
    }
}

// Does relation r have an edge into 32-row tile `tile`?  (A relation with none contributes an all-zero A tile: the
// forward skips its gather and its MFMAs, the weight gradient the whole tile.)
__device__ __forceinline__ bool rel_tile_active(const lgcn_agg_mlp_t &p, int r, int64_t tile) {
    const int mode = p.rel[r].mode;
    if (mode == LGCN_REL_CSR) {
        const int64_t n_sub = (p.n_rows + 15) >> 4;
        bool on = false;
        for (int h = 0; h < 2; ++h) {
            const int64_t sub = tile * 2 + h;
            if (sub < n_sub) {
                const int64_t k0 = (sub * p.n_rel_csr + p.rel[r].ridx) * 16;
                on = on || p.rowptr[k0 + 16] > p.rowptr[k0];
            }
        }
        return on;
    }
    if (mode == LGCN_REL_RANGE) {
        const int64_t r0 = tile * kTM32, r1 = r0 + kTM32 < p.n_rows ? r0 + kTM32 : p.n_rows;
        return p.rowptr[r1] > p.rowptr[r0];
    }
    return true;
}

// KIND only names the instantiation (1 = LaneConv layer: CSR relations; 0 = every other use) so
// that profilers report the dominant kernel separately; the code is identical.
template <int KIND>
__global__ __launch_bounds__(512) void k_agg_mlp(const lgcn_agg_mlp_t p, int n_tiles) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTileFloats + 32];
    float *buf0 = smem, *buf1 = smem + kTileFloats;
    int *act = reinterpret_cast<int *>(smem + 2 * kTileFloats);  // [0..15] relation ids, [16] count

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = xcd_chunk_remap(blockIdx.x, n_tiles);
    const int64_t row0 = (int64_t)tile * kTM32;

    if (wave == 0) {     // active relations of this tile, in relation order
        const bool on = lane < p.n_rel && rel_tile_active(p, lane, tile);
        const unsigned long long m = __ballot(on);
        if (on) act[__popcll(m & ((1ull << lane) - 1ull))] = lane;
        if (lane == 0) act[16] = __popcll(m);
    }
    __syncthreads();
    const int nact = __builtin_amdgcn_readfirstlane(act[16]);

    if (wave >= 4 && nact > 0) gather_rel(buf0, p, __builtin_amdgcn_readfirstlane(act[0]), tile, tid - 256);
    __syncthreads();

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    for (int i = 0; i < nact; ++i) {
        float *cur = (i & 1) ? buf1 : buf0;
        float *nxt = (i & 1) ? buf0 : buf1;
        if (wave < 4) {
            const int ri = __builtin_amdgcn_readfirstlane(act[i]);
            tile_gemm(cur, reinterpret_cast<const float4 *>(p.rel[ri].wp) + wave * (16 * 64), acc, lane, 16);
        } else if (i + 1 < nact) {
            gather_rel(nxt, p, __builtin_amdgcn_readfirstlane(act[i + 1]), tile, tid - 256);
        }
        __syncthreads();
    }

    if (wave < 4) {
        if (p.w4 != nullptr) {
            // rank-4 update: the 4 extra input channels of A2M.meta (lanegcn.py:387-395)
            const float4 wc = *reinterpret_cast<const float4 *>(p.w4 + 4 * (32 * wave + (lane & 31)));
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t n = row0 + acc_row(i, lane);
                if (n < p.n_rows) {
                    const float2 tu = reinterpret_cast<const float2 *>(p.x4_a)[n];
                    acc[i] += tu.x * wc.x + tu.y * wc.y + p.x4_b[n] * wc.z + p.x4_c[n] * wc.w;
                }
            }
        }
        acc_to_lds(buf0, acc, lane, wave);
    }
    __syncthreads();

    const int rrow = tid >> 3;  // valid for tid < 256
    const int64_t n = row0 + rrow;
    const bool live = tid < 256 && n < p.n_rows;
    const int flags = p.flags;

    if (!(flags & LGCN_F_GEMM2)) {
        if (tid < 256) {
            RowVals r = row_load(buf0, tid);
            if (live && p.out_pre) row_store_global(p.out_pre + n * kC, tid, r);
            if (flags & LGCN_F_GN1) row_gn(r, tid, p.gn1_g, p.gn1_b, p.eps);
            if (live && (flags & LGCN_F_RES)) row_add_global(r, p.res + n * kC, tid);
            if (flags & LGCN_F_RELU1) row_relu(r);
            if (live) row_store_global(p.out + n * kC, tid, r);
        }
        return;
    }

    if (tid < 256) {
        RowVals r = row_load(buf0, tid);
        if (live && p.out_pre) row_store_global(p.out_pre + n * kC, tid, r);
        if (flags & LGCN_F_GN1) row_gn(r, tid, p.gn1_g, p.gn1_b, p.eps);
        if (flags & LGCN_F_RELU1) row_relu(r);
        if (live && p.out_mid) row_store_global(p.out_mid + n * kC, tid, r);
        row_store_lds(buf0, tid, r);
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        tile_gemm(buf0, reinterpret_cast<const float4 *>(p.wp2) + wave * (16 * 64), acc, lane, 16);
        acc_to_lds(buf1, acc, lane, wave);
    }
    __syncthreads();
    if (tid < 256) {
        RowVals r = row_load(buf1, tid);
        if (live && p.out_pre2) row_store_global(p.out_pre2 + n * kC, tid, r);
        if (flags & LGCN_F_GN2) row_gn(r, tid, p.gn2_g, p.gn2_b, p.eps);
        if (live && (flags & LGCN_F_RES)) row_add_global(r, p.res + n * kC, tid);
        if (flags & LGCN_F_RELU2) row_relu(r);
        if (live) row_store_global(p.out + n * kC, tid, r);
    }
}

// ------------------------------------------------------- mapnet input -----
// h1[row][c] = ReLU(w1[c][0] * x + w1[c][1] * y + b1[c]) for the thread's 16 columns
__device__ __forceinline__ void lin2_relu_to_lds(float *T, int t, float x, float y, const float *__restrict__ w1,
                                                 const float *__restrict__ b1) {
    float *p = T + (t >> 3) * kLDA + 4 * (t & 7);
    const int c0 = 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + 32 * j;
        const float4 wa = *reinterpret_cast<const float4 *>(w1 + 2 * c);      // (c,0) (c,1) (c+1,0) (c+1,1)
        const float4 wb = *reinterpret_cast<const float4 *>(w1 + 2 * c + 4);  // c+2, c+3
        const float4 bb = *reinterpret_cast<const float4 *>(b1 + c);
        float4 o;
        o.x = relu_nan(x * wa.x + y * wa.y + bb.x);
        o.y = relu_nan(x * wa.z + y * wa.w + bb.y);
        o.z = relu_nan(x * wb.x + y * wb.y + bb.z);
        o.w = relu_nan(x * wb.z + y * wb.w + bb.w);
        *reinterpret_cast<float4 *>(p + 32 * j) = o;
    }
}

__global__ __launch_bounds__(256) void k_mapnet_input(const InputParams p, int n_tiles) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTileFloats];
    float *T1 = smem, *T2 = smem + kTileFloats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    const int64_t n = (int64_t)tile * kTM32 + (tid >> 3);
    const bool live = n < p.n_rows;
    f32x16 acc;

    float2 c = make_float2(0.f, 0.f), f = make_float2(0.f, 0.f);
    if (live) { c = reinterpret_cast<const float2 *>(p.ctrs)[n]; f = reinterpret_cast<const float2 *>(p.feats)[n]; }

    lin2_relu_to_lds(T1, tid, c.x, c.y, p.wa1, p.ba1);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    tile_gemm(T1, reinterpret_cast<const float4 *>(p.wpa2) + wave * (16 * 64), acc, lane, 16);
    acc_to_lds(T2, acc, lane, wave);
    __syncthreads();
    RowVals ra = row_load(T2, tid);
    row_gn(ra, tid, p.ga, p.bta, p.eps);

    lin2_relu_to_lds(T1, tid, f.x, f.y, p.ws1, p.bs1);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    tile_gemm(T1, reinterpret_cast<const float4 *>(p.wps2) + wave * (16 * 64), acc, lane, 16);
    acc_to_lds(T2, acc, lane, wave);
    __syncthreads();
    RowVals rs = row_load(T2, tid);
    row_gn(rs, tid, p.gs, p.bts, p.eps);
#pragma unroll
    for (int j = 0; j < 4; ++j) rs.v[j] = f4add(rs.v[j], ra.v[j]);
    row_relu(rs);
    if (live) row_store_global(p.out + n * kC, tid, rs);
}

// ---------------------------------------------------------- att pairs -----
// ReLU masks of a pair row as bits (the training forward saves them instead of any [P,128] tensor): word j of a row's four
// holds channels 32 j .. 32 j + 31, bit b = channel 32 j + b is set where the value is > 0.  A thread owns bits
// 4 sub .. 4 sub + 3 of every word; the 8 threads of a row OR theirs together (the butterfly of sum8).
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov_u(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}

__device__ __forceinline__ uint4 row_mask_words(const RowVals &r, int t) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t b = (r.v[j].x > 0.f ? 1u : 0u) | (r.v[j].y > 0.f ? 2u : 0u) | (r.v[j].z > 0.f ? 4u : 0u) |
                     (r.v[j].w > 0.f ? 8u : 0u);
        b <<= 4 * (t & 7);
        b |= dpp_mov_u<0xB1>(b);
        b |= dpp_mov_u<0x4E>(b);
        b |= dpp_mov_u<0x141>(b);
        w[j] = b;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// g = 0 where the thread's bit of the row's mask words is clear
__device__ __forceinline__ float4 mask4(float4 g, uint32_t b) {
    return make_float4((b & 1u) ? g.x : 0.f, (b & 2u) ? g.y : 0.f, (b & 4u) ? g.z : 0.f, (b & 8u) ? g.w : 0.f);
}

// mw = the row's four words of one mask, or nullptr for a row past the count (no gradient)
__device__ __forceinline__ void row_apply_mask(RowVals &g, const uint4 *__restrict__ mw, int t) {
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
    if (mw != nullptr) { const uint4 m = *mw; w0 = m.x; w1 = m.y; w2 = m.z; w3 = m.w; }
    const int sh = 4 * (t & 7);
    g.v[0] = mask4(g.v[0], w0 >> sh); g.v[1] = mask4(g.v[1], w1 >> sh);
    g.v[2] = mask4(g.v[2], w2 >> sh); g.v[3] = mask4(g.v[3], w3 >> sh);
}

// MASKS: the training forward (lgcn_att_pairs_train).  masks[p][k] = the four words of mask k of pair p, k = 0: W_d0 d +
// b_d0 > 0, 1: e > 0, 2: m > 0; the arithmetic of m is the inference kernel's.
template <bool MASKS>
__global__ __launch_bounds__(256) void k_att_pairs(const PairParams p, uint4 *__restrict__ masks) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTileFloats];
    float *T1 = smem, *T2 = smem + kTileFloats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t P = *p.n_pairs;
    if (P < 0 || P > p.cap) P = p.cap;
    const int64_t n_tiles = (P + kTM32 - 1) / kTM32;
    f32x16 acc;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t pr = tile * kTM32 + (tid >> 3);
        const bool live = pr < P;
        int h = 0, w = 0;
        float dx = 0.f, dy = 0.f;
        if (live) {
            h = p.hi[pr]; w = p.wi[pr];
            const float2 a = reinterpret_cast<const float2 *>(p.agt_ctrs)[h];
            const float2 c = reinterpret_cast<const float2 *>(p.ctx_ctrs)[w];
            dx = a.x - c.x; dy = a.y - c.y;
        }
        lin2_relu_to_lds(T1, tid, dx, dy, p.wd0, p.bd0);
        if constexpr (MASKS) {      // ReLU(z) > 0 <=> z > 0; the thread reads back its own elements
            const uint4 mw = row_mask_words(row_load(T1, tid), tid);
            if (live && (tid & 7) == 0) masks[pr * 3] = mw;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        tile_gemm(T1, reinterpret_cast<const float4 *>(p.wpd2) + wave * (16 * 64), acc, lane, 16);
        acc_to_lds(T2, acc, lane, wave);
        __syncthreads();
        {
            RowVals r = row_load(T2, tid);
            row_gn(r, tid, p.gd, p.btd, p.eps);
            row_relu(r);
            row_store_lds(T2, tid, r);
            if constexpr (MASKS) {
                const uint4 mw = row_mask_words(r, tid);
                if (live && (tid & 7) == 0) masks[pr * 3 + 1] = mw;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        tile_gemm(T2, reinterpret_cast<const float4 *>(p.wpc0e) + wave * (16 * 64), acc, lane, 16);
        acc_to_lds(T1, acc, lane, wave);
        __syncthreads();
        {
            RowVals r = row_load(T1, tid);
            if (live) {
                row_add_global(r, p.U + (int64_t)h * kC, tid);
                row_add_global(r, p.V + (int64_t)w * kC, tid);
            }
            row_gn(r, tid, p.gc, p.btc, p.eps);
            row_relu(r);
            if (live) row_store_global(p.m + pr * kC, tid, r);
            if constexpr (MASKS) {
                const uint4 mw = row_mask_words(r, tid);
                if (live && (tid & 7) == 0) masks[pr * 3 + 2] = mw;
            }
        }
        // next iteration's first write to T1 is by the same thread that just
        // read those elements; T2 is rewritten only after the next barrier.
    }
}

// --------------------------------------------------------- pool pairs -----
// The pair stage of the fork's LanePooling (reference lanercnn.py:492-499): k_att_pairs with a 4-d relative pose in
// place of the 2-d offset, one GEMM instead of two and one hoisted row block (U, per context row) instead of two.
// h[row][c] = ReLU(w[c] . d + b[c]) for the thread's 16 columns; w: [128,4], one float4 per channel
__device__ __forceinline__ void lin4_relu_to_lds(float *T, int t, float4 d, const float *__restrict__ w,
                                                 const float *__restrict__ b) {
    float *p = T + (t >> 3) * kLDA + 4 * (t & 7);
    const int c0 = 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 *wc = reinterpret_cast<const float4 *>(w) + (c0 + 32 * j);
        const float4 bb = *reinterpret_cast<const float4 *>(b + c0 + 32 * j);
        const float4 w0 = wc[0], w1 = wc[1], w2 = wc[2], w3 = wc[3];
        float4 o;
        o.x = relu_nan(d.x * w0.x + d.y * w0.y + d.z * w0.z + d.w * w0.w + bb.x);
        o.y = relu_nan(d.x * w1.x + d.y * w1.y + d.z * w1.z + d.w * w1.w + bb.y);
        o.z = relu_nan(d.x * w2.x + d.y * w2.y + d.z * w2.z + d.w * w2.w + bb.z);
        o.w = relu_nan(d.x * w3.x + d.y * w3.y + d.z * w3.z + d.w * w3.w + bb.w);
        *reinterpret_cast<float4 *>(p + 32 * j) = o;
    }
}

// MASKS: the training forward (lgcn_pool_pairs_train).  masks[p][k] = the four words of mask k of pair p, k = 0: W_p d + b_p
// > 0, 1: m > 0 (the layout of k_att_pairs); the arithmetic of m is the inference kernel's.
template <bool MASKS>
__global__ __launch_bounds__(256) void k_pool_pairs(const PoolParams p, uint4 *__restrict__ masks) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTileFloats];
    float *T1 = smem, *T2 = smem + kTileFloats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t P = *p.n_pairs;
    if (P < 0 || P > p.cap) P = p.cap;
    const int64_t n_tiles = (P + kTM32 - 1) / kTM32;
    f32x16 acc;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t pr = tile * kTM32 + (tid >> 3);
        const bool live = pr < P;
        int c = 0;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            c = p.ci[pr];
            const float4 a = reinterpret_cast<const float4 *>(p.ctx_pose)[c];
            const float4 b = reinterpret_cast<const float4 *>(p.tgt_pose)[p.ti[pr]];
            d = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
        }
        lin4_relu_to_lds(T1, tid, d, p.wp, p.bp);
        if constexpr (MASKS) {      // ReLU(y0) > 0 <=> y0 > 0; the thread reads back its own elements
            const uint4 mw = row_mask_words(row_load(T1, tid), tid);
            if (live && (tid & 7) == 0) masks[pr * 2] = mw;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        tile_gemm(T1, reinterpret_cast<const float4 *>(p.wpc0h) + wave * (16 * 64), acc, lane, 16);
        acc_to_lds(T2, acc, lane, wave);
        __syncthreads();
        {
            RowVals r = row_load(T2, tid);
            if (live) row_add_global(r, p.U + (int64_t)c * kC, tid);
            row_gn(r, tid, p.g, p.bt, p.eps);
            row_relu(r);
            if (live) row_store_global(p.m + pr * kC, tid, r);
            if constexpr (MASKS) {
                const uint4 mw = row_mask_words(r, tid);
                if (live && (tid & 7) == 0) masks[pr * 2 + 1] = mw;
            }
        }
        // T1 is rewritten only after every wave's tile_gemm (the barrier above); T2 only after the next iteration's
        // first barrier, which every thread reaches after its row_load.
    }
}


// ------------------------------------------------------------- wgrad ------
// One 32-row tile of dW += D^T S for the 64 x 64 block (q >> 1, q & 1) of the 128 x 128 result: D (the dT rows) and S (the
// source rows) are LDS tiles, the contraction runs over their rows, two per MFMA; a?? = the block's four 32 x 32 quadrants.
__device__ __forceinline__ void wgrad_tile(const float *__restrict__ D, const float *__restrict__ S, f32x16 &a00, f32x16 &a01,
                                           f32x16 &a10, f32x16 &a11, int q, int lane) {
    const float *Dp = D + (lane >> 5) * kLDA + 64 * (q >> 1) + (lane & 31);
    const float *Sp = S + (lane >> 5) * kLDA + 64 * (q & 1) + (lane & 31);
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
        const float a0 = Dp[2 * s * kLDA], a1 = Dp[2 * s * kLDA + 32];
        const float b0 = Sp[2 * s * kLDA], b1 = Sp[2 * s * kLDA + 32];
        a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, a00, 0, 0, 0);
        a01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, a01, 0, 0, 0);
        a10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, a10, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, a11, 0, 0, 0);
    }
}

// The block's four quadrants to a row-major [128,128] image
__device__ __forceinline__ void wgrad_store(float *__restrict__ o, const f32x16 &a00, const f32x16 &a01, const f32x16 &a10,
                                            const f32x16 &a11, int q, int lane) {
    float *p = o + (64 * (q >> 1)) * kC + 64 * (q & 1) + (lane & 31);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int r = acc_row(g, lane);
        p[r * kC] = a00[g]; p[r * kC + 32] = a01[g];
        p[(32 + r) * kC] = a10[g]; p[(32 + r) * kC + 32] = a11[g];
    }
}

// dW[r] = dT^T (G_r src_r): block (chunk, r) walks the 32-row tiles chunk, chunk + n_chunks, ... that
// relation r touches; waves 4-7 stage the gathered source rows and the dT rows of the next tile in LDS
// while waves 0-3 contract the current one over its rows on v_mfma_f32_32x32x2_f32 (K-step = 2 rows;
// with lanes along the channel axis both operands are plain row reads, no transpose).  Wave w owns the
// 64 x 64 block (w >> 1, w & 1) of the 128 x 128 result; partials per chunk are summed by k_wgrad_reduce.
__global__ __launch_bounds__(512) void k_wgrad(const lgcn_agg_mlp_t p, const float *__restrict__ dT,
                                               float *__restrict__ part, int n_tiles, int n_chunks) {
    __shared__ __attribute__((aligned(16))) float smem[4 * kTileFloats];
    auto bufA = [&](int b) { return smem + b * kTileFloats; };
    auto bufD = [&](int b) { return smem + (2 + b) * kTileFloats; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.y, chunk = blockIdx.x;

    auto next_active = [&](int64_t t) -> int64_t {
        while (t < n_tiles && !rel_tile_active(p, r, t)) t += n_chunks;
        return t;
    };
    auto fill = [&](int b, int64_t t) {   // waves 4-7
        const int gt = tid - 256;
        gather_rel(bufA(b), p, r, (int)t, gt);
        const int hw = gt >> 5, l = gt & 31;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = it * 8 + hw;
            const int64_t n = t * kTM32 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < p.n_rows) v = reinterpret_cast<const float4 *>(dT)[n * 32 + l];
            *reinterpret_cast<float4 *>(bufD(b) + row * kLDA + 4 * l) = v;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    int64_t t = next_active(chunk);
    if (wave >= 4 && t < n_tiles) fill(0, t);
    __syncthreads();
    int b = 0;
    while (t < n_tiles) {
        const int64_t tn = next_active(t + n_chunks);
        if (wave < 4) {
            wgrad_tile(bufD(b), bufA(b), acc[0][0], acc[0][1], acc[1][0], acc[1][1], wave, lane);
        } else if (tn < n_tiles) {
            fill(b ^ 1, tn);
        }
        __syncthreads();
        t = tn;
        b ^= 1;
    }
    if (wave < 4)
        wgrad_store(part + ((int64_t)r * n_chunks + chunk) * (kC * kC), acc[0][0], acc[0][1], acc[1][0], acc[1][1], wave, lane);
}

__global__ __launch_bounds__(256) void k_wgrad_reduce(const float *__restrict__ part, int n_chunks, float *__restrict__ dW) {
    const int r = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;   // < 128*128
    const float *p = part + (int64_t)r * n_chunks * (kC * kC) + e;
    float s = 0.f;
    for (int c = 0; c < n_chunks; ++c) s += p[(int64_t)c * (kC * kC)];
    dW[(int64_t)r * (kC * kC) + e] = s;
}

// ------------------------------------------------------ att pairs bwd -----
// Backward of the pair stage for dS [T,128] (include/lgcn.h, lgcn_att_pairs_bwd).  Workgroup `chunk` walks the 32-pair
// tiles chunk, chunk + n_chunks, ...  Per tile, waves 0-3 recompute h1, t1, e, c and the GroupNorm statistics with the
// forward's device functions (their 256 threads are the row phase, their 4 waves the 32 x 128 x 128 tile GEMMs), apply the
// stored masks, run both GroupNorm backwards in registers and the two dx GEMMs on the transposed images.  Waves 4-7 own
// everything that is summed over pairs, in registers across the workgroup's tiles: the two 128 x 128 weight gradients
// (wave 4 + q: block q of both, A[0..7]) contracted over the tile's rows, and the seven [128] vectors as column sums of
// tiles the row phase leaves in LDS (thread (which, c) of the 2 x 128: one column of one tile), all while waves 0-3 run
// the next GEMM.  That split instead of "waves 0-3 dW_d2, waves 4-7 dW_c0e": waves 0-3 already issue four tile GEMMs
// (256 MFMAs) per tile against 128 MFMAs for both weight gradients, and 64 more accumulator registers beside the row
// phase's working set did not fit without scratch.
// LDS: H (h1), E (e), X (GEMM output), G (dc, then dt1, then dz0 * dy), XD (xhat of GN_d), P1 / P2 (g * xhat / g of a
// GroupNorm backward, then dz0 / dz0 * dx): 7 x 16.5 KiB.
constexpr int kPairRecTail = 7 * kC;
constexpr int kPairRec = 2 * kC * kC + kPairRecTail;      // floats per chunk record

__device__ __forceinline__ RowVals row_mul(const RowVals &a, const RowVals &b) {
    RowVals r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = make_float4(a.v[j].x * b.v[j].x, a.v[j].y * b.v[j].y, a.v[j].z * b.v[j].z, a.v[j].w * b.v[j].w);
    return r;
}

__device__ __forceinline__ RowVals row_scale(const RowVals &a, float s) {
    RowVals r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = make_float4(a.v[j].x * s, a.v[j].y * s, a.v[j].z * s, a.v[j].w * s);
    return r;
}

// sum over the 32 rows of column c of a tile, in row order
__device__ __forceinline__ float tile_colsum(const float *T, int c) {
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) s += T[r * kLDA + c];
    return s;
}

__global__ __launch_bounds__(512) void k_att_pairs_bwd(const PairBwdParams p) {
    __shared__ __attribute__((aligned(16))) float smem[7 * kTileFloats];
    float *H = smem, *E = smem + kTileFloats, *X = smem + 2 * kTileFloats, *G = smem + 3 * kTileFloats;
    float *XD = smem + 4 * kTileFloats, *P1 = smem + 5 * kTileFloats, *P2 = smem + 6 * kTileFloats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool rowt = tid < 256;
    const int which = (tid >> 7) & 1, col = tid & 127;       // waves 4-7: column sums
    const PairParams &f = p.f;
    int64_t P = *f.n_pairs;
    if (P < 0 || P > f.cap) P = f.cap;
    const int64_t n_tiles = (P + kTM32 - 1) / kTM32;
    const bool want_rec = p.rec != nullptr, want_d = p.want_d != 0, want_wc = p.want_wc != 0;

    f32x16 A[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) A[k][i] = 0.f;
    float s_c = 0.f, s_d = 0.f, s_0a = 0.f, s_0b = 0.f;      // which = 0: dgamma_c, dgamma_d, db_d0, dW_d0[:,0]; 1: dbeta_c, dbeta_d, dW_d0[:,1]
    bool pend = false;           // those three tiles are waiting
    f32x16 acc;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t pr = tile * kTM32 + (tid >> 3);
        const bool live = rowt && pr < P;
        const uint4 *mk = live ? p.masks + pr * 3 : nullptr;              // rows past the count: no gradient
        int h = 0, w = 0;
        float dx = 0.f, dy = 0.f;
        if (live) {
            h = f.hi[pr]; w = f.wi[pr];
            const float2 a = reinterpret_cast<const float2 *>(f.agt_ctrs)[h];
            const float2 c = reinterpret_cast<const float2 *>(f.ctx_ctrs)[w];
            dx = a.x - c.x; dy = a.y - c.y;
        }
        // ---- forward again: h1 -> H, t1 -> X, e -> E, c -> X
        if (rowt) lin2_relu_to_lds(H, tid, dx, dy, f.wd0, f.bd0);
        __syncthreads();
        if (wave < 4) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            tile_gemm(H, reinterpret_cast<const float4 *>(f.wpd2) + wave * (16 * 64), acc, lane, 16);
            acc_to_lds(X, acc, lane, wave);
        } else if (pend) {      // what the last row phase of the tile before left: P1 = dz0, P2 = dz0 * dx, G = dz0 * dy
            s_0a += tile_colsum(which ? G : P1, col);     // (they are next written three barriers from here)
            if (which == 0) s_0b += tile_colsum(P2, col);
        }
        pend = false;
        __syncthreads();
        float rstd_d = 0.f;
        if (rowt) {
            RowVals xd = row_load(X, tid);
            rstd_d = row_gn_hat(xd, f.eps);
            row_store_lds(XD, tid, xd);     // read back by this thread alone
            RowVals e = row_affine(xd, tid, f.gd, f.btd);
            row_relu(e);
            row_store_lds(E, tid, e);
        }
        __syncthreads();
        if (wave < 4) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            tile_gemm(E, reinterpret_cast<const float4 *>(f.wpc0e) + wave * (16 * 64), acc, lane, 16);
            acc_to_lds(X, acc, lane, wave);
        }
        __syncthreads();
        // ---- m = ReLU(GN_c(c)): g2 = dS[h] * mask2 (P1 = g2 * chat, P2 = g2), dc -> G and global
        if (rowt) {
            RowVals c = row_load(X, tid);
            RowVals g;
#pragma unroll
            for (int j = 0; j < 4; ++j) g.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                row_add_global(c, f.U + (int64_t)h * kC, tid);
                row_add_global(c, f.V + (int64_t)w * kC, tid);
                row_add_global(g, p.dS + (int64_t)h * kC, tid);
            }
            const float rstd_c = row_gn_hat(c, f.eps);
            row_apply_mask(g, mk ? mk + 2 : mk, tid);
            if (want_rec) { row_store_lds(P1, tid, row_mul(g, c)); row_store_lds(P2, tid, g); }
            row_gn_bwd(g, c, rstd_c, tid, f.gc);
            row_store_lds(G, tid, g);
            if (live && p.dc) row_store_global(p.dc + pr * kC, tid, g);
        }
        if (!want_rec) continue;                // uniform; X is next written two barriers from here
        __syncthreads();
        // ---- c = W_c0e e + ..: de = dc W_c0e -> X (waves 0-3); dW_c0e += dc^T e, dgamma_c, dbeta_c (waves 4-7)
        if (wave < 4) {
            if (want_d) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                tile_gemm(G, reinterpret_cast<const float4 *>(p.wptc0e) + wave * (16 * 64), acc, lane, 16);
                acc_to_lds(X, acc, lane, wave);
            }
        } else {
            if (want_wc) wgrad_tile(G, E, A[4], A[5], A[6], A[7], wave - 4, lane);
            s_c += tile_colsum(which ? P2 : P1, col);
        }
        if (!want_d) continue;                  // uniform; E, G, P1 and P2 are next written at least two barriers from here
        __syncthreads();
        // ---- e = ReLU(GN_d(t1)): g1 = de * mask1 (P1 = g1 * t1hat, P2 = g1), dt1 -> G
        if (rowt) {
            RowVals g = row_load(X, tid);
            const RowVals xd = row_load(XD, tid);
            row_apply_mask(g, mk ? mk + 1 : mk, tid);
            row_store_lds(P1, tid, row_mul(g, xd));
            row_store_lds(P2, tid, g);
            row_gn_bwd(g, xd, rstd_d, tid, f.gd);
            row_store_lds(G, tid, g);
        }
        __syncthreads();
        // ---- t1 = W_d2 h1: dh1 = dt1 W_d2 -> X (waves 0-3); dW_d2 += dt1^T h1, dgamma_d, dbeta_d (waves 4-7)
        if (wave < 4) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            tile_gemm(G, reinterpret_cast<const float4 *>(p.wptd2) + wave * (16 * 64), acc, lane, 16);
            acc_to_lds(X, acc, lane, wave);
        } else {
            wgrad_tile(G, H, A[0], A[1], A[2], A[3], wave - 4, lane);
            s_d += tile_colsum(which ? P2 : P1, col);
        }
        __syncthreads();
        // ---- h1 = ReLU(W_d0 d + b_d0): dz0 = dh1 * mask0 -> P1, dz0 * dx -> P2, dz0 * dy -> G; waves 4-7 sum them
        // behind the next barrier (the next tile's first, or the one after the loop)
        if (rowt) {
            RowVals g = row_load(X, tid);
            row_apply_mask(g, mk, tid);
            row_store_lds(P1, tid, g);
            row_store_lds(P2, tid, row_scale(g, dx));
            row_store_lds(G, tid, row_scale(g, dy));
        }
        pend = true;
    }

    if (!want_rec) return;
    if (pend) {
        __syncthreads();
        if (wave >= 4) {
            s_0a += tile_colsum(which ? G : P1, col);
            if (which == 0) s_0b += tile_colsum(P2, col);
        }
    }
    if (wave >= 4) {
        float *rec = p.rec + (int64_t)blockIdx.x * kPairRec;
        wgrad_store(rec, A[0], A[1], A[2], A[3], wave - 4, lane);
        wgrad_store(rec + kC * kC, A[4], A[5], A[6], A[7], wave - 4, lane);
        float *tail = rec + 2 * kC * kC;
        tail[which * kC + col] = s_c;
        tail[(2 + which) * kC + col] = s_d;
        tail[(which ? 6 : 4) * kC + col] = s_0a;
        if (which == 0) tail[5 * kC + col] = s_0b;
    }
}

// out = sum over the chunk records, in chunk order.  Record: dW_d2 [128,128], dW_c0e [128,128], then seven [128] vectors:
// dgamma_c, dbeta_c, dgamma_d, dbeta_d, db_d0, dW_d0[:,0], dW_d0[:,1].
__global__ __launch_bounds__(256) void k_att_pairs_bwd_reduce(const float *__restrict__ rec, int n_rec, const PairBwdOut o) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kPairRec) return;
    float *dst = nullptr;
    if (e < kC * kC) dst = o.dwd2 ? o.dwd2 + e : nullptr;
    else if (e < 2 * kC * kC) dst = o.dwc0e ? o.dwc0e + (e - kC * kC) : nullptr;
    else {
        const int v = (e - 2 * kC * kC) >> 7, c = e & 127;
        float *const vec = v == 0 ? o.dgc : v == 1 ? o.dbc : v == 2 ? o.dgd : v == 3 ? o.dbd : v == 4 ? o.dbd0 : o.dwd0;
        if (vec != nullptr) dst = v < 5 ? vec + c : vec + 2 * c + (v - 5);
    }
    if (dst == nullptr) return;
    float s = 0.f;
    for (int k = 0; k < n_rec; ++k) s += rec[(int64_t)k * kPairRec + e];
    *dst = s;
}

// --------------------------------------------------- LaneConv block bwd ----
// Backward of out = ReLU(GN2(ReLU(GN1(T)) W2^T) + X) from d_out down to dT (include/lgcn.h, lgcn_laneconv_bwd), shaped like
// k_att_pairs_bwd: workgroup `chunk` walks the 32-row tiles chunk, chunk + n_chunks, ...; waves 0-3 are the row phase (8
// threads per row) and the tile GEMMs, waves 4-7 stage the saved Y (and X) rows and own everything summed over rows, in
// registers across the workgroup's tiles: dW2 (and dW1) on wgrad_tile, wave 4 + q holding block q, and the four GroupNorm
// vectors as column sums of the tiles P1 / P2 the row phase leaves in LDS.  IDENT1 (T = X W1^T, a LinearRes) finishes the
// block: dX = dT W1 + g2 with g2 kept in the row threads' registers, dW1 += dT^T X; neither dT nor g2 reaches memory.
// LDS: YT (Y rows), D (dZ, then dT), P1 / P2 (g * xhat / g of a GroupNorm backward), G (GEMM output), and XT (X rows) for
// IDENT1: 5 or 6 x 16.5 KiB.  Four barriers per tile.
struct LcBwdParams {
    const float *d_out, *out, *Z, *Y, *T, *X;
    const float *gamma1, *gamma2, *wpt2, *wpt1;
    float *dT, *g2, *dX, *rec;
    int64_t n_rows;
    float eps;
    int want_w2, want_w1;
};

struct LcBwdOut { float *dw2, *dw1, *dg2, *db2, *dg1, *db1; };

__host__ __device__ constexpr int lc_rec_floats(bool ident1) { return (ident1 ? 2 : 1) * kC * kC + 4 * kC; }

__device__ __forceinline__ RowVals row_load_global(const float *__restrict__ rowp, int t) {
    RowVals r;
    const float *p = rowp + 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = *reinterpret_cast<const float4 *>(p + 32 * j);
    return r;
}

__device__ __forceinline__ RowVals row_zero() {
    RowVals r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    return r;
}

// g where post > 0, else 0 (the mask of k_gn_bwd)
__device__ __forceinline__ void row_mask_pos(RowVals &g, const RowVals &post) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        g.v[j].x = post.v[j].x > 0.f ? g.v[j].x : 0.f; g.v[j].y = post.v[j].y > 0.f ? g.v[j].y : 0.f;
        g.v[j].z = post.v[j].z > 0.f ? g.v[j].z : 0.f; g.v[j].w = post.v[j].w > 0.f ? g.v[j].w : 0.f;
    }
}

// rows [32 tile, 32 tile + 32) of a [n_rows,128] tensor into an LDS tile, zeros past n_rows (gt = 0..255 of waves 4-7)
__device__ __forceinline__ void stage_rows(float *__restrict__ dst, const float *__restrict__ src, int64_t tile, int64_t n_rows,
                                           int gt) {
    const int hw = gt >> 5, l = gt & 31;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + hw;
        const int64_t n = tile * kTM32 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < n_rows) v = reinterpret_cast<const float4 *>(src)[n * 32 + l];
        *reinterpret_cast<float4 *>(dst + row * kLDA + 4 * l) = v;
    }
}

template <bool IDENT1>
__global__ __launch_bounds__(512) void k_lc_bwd_rows(const LcBwdParams p) {
    __shared__ __attribute__((aligned(16))) float smem[(IDENT1 ? 6 : 5) * kTileFloats];
    float *YT = smem, *D = smem + kTileFloats, *P1 = smem + 2 * kTileFloats, *P2 = smem + 3 * kTileFloats;
    float *G = smem + 4 * kTileFloats, *XT = smem + (IDENT1 ? 5 : 0) * kTileFloats;      // XT: IDENT1 only
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool rowt = tid < 256;
    const int which = (tid >> 7) & 1, col = tid & 127;       // waves 4-7: column sums
    const int64_t n_tiles = (p.n_rows + kTM32 - 1) / kTM32;
    const bool want_rec = p.rec != nullptr, want_w2 = p.want_w2 != 0, want_w1 = IDENT1 && p.want_w1 != 0;
    const bool want_dx = IDENT1 && p.dX != nullptr;

    f32x16 A[IDENT1 ? 8 : 4];
#pragma unroll
    for (int k = 0; k < (IDENT1 ? 8 : 4); ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) A[k][i] = 0.f;
    float s2 = 0.f, s1 = 0.f;      // which = 0: dgamma2, dgamma1; 1: dbeta2, dbeta1
    f32x16 acc;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t n = tile * kTM32 + (tid >> 3);
        const bool live = rowt && n < p.n_rows;
        RowVals g2 = row_zero();
        // ---- out = ReLU(GN2(Z) + X): g2 = d_out * (out > 0) (P1 = g2 * zhat, P2 = g2), dZ -> D; waves 4-7 stage Y (and X)
        if (rowt) {
            RowVals z = row_zero();
            if (live) {
                g2 = row_load_global(p.d_out + n * kC, tid);
                row_mask_pos(g2, row_load_global(p.out + n * kC, tid));
                z = row_load_global(p.Z + n * kC, tid);
                if (!IDENT1 && p.g2) row_store_global(p.g2 + n * kC, tid, g2);
            }
            const float rstd2 = row_gn_hat(z, p.eps);
            if (want_rec) { row_store_lds(P1, tid, row_mul(g2, z)); row_store_lds(P2, tid, g2); }
            RowVals dz = g2;
            row_gn_bwd(dz, z, rstd2, tid, p.gamma2);
            row_store_lds(D, tid, dz);
        } else {
            stage_rows(YT, p.Y, tile, p.n_rows, tid - 256);
            if (want_w1) stage_rows(XT, p.X, tile, p.n_rows, tid - 256);
        }
        __syncthreads();
        // ---- Z = Y W2^T: dY = dZ W2 -> G (waves 0-3); dW2 += dZ^T Y, dgamma2, dbeta2 (waves 4-7)
        if (wave < 4) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            tile_gemm(D, reinterpret_cast<const float4 *>(p.wpt2) + wave * (16 * 64), acc, lane, 16);
            acc_to_lds(G, acc, lane, wave);
        } else if (want_rec) {
            if (want_w2) wgrad_tile(D, YT, A[0], A[1], A[2], A[3], wave - 4, lane);
            s2 += tile_colsum(which ? P2 : P1, col);
        }
        __syncthreads();
        // ---- Y = ReLU(GN1(T)): g1 = dY * (Y > 0) (P1 = g1 * that, P2 = g1), dT -> memory, or -> D for IDENT1
        if (rowt) {
            RowVals g = row_load(G, tid);
            row_mask_pos(g, row_load(YT, tid));
            RowVals t = row_zero();
            if (live) t = row_load_global(p.T + n * kC, tid);
            const float rstd1 = row_gn_hat(t, p.eps);
            if (want_rec) { row_store_lds(P1, tid, row_mul(g, t)); row_store_lds(P2, tid, g); }
            row_gn_bwd(g, t, rstd1, tid, p.gamma1);
            if (IDENT1) row_store_lds(D, tid, g);
            else if (live && p.dT) row_store_global(p.dT + n * kC, tid, g);
        }
        __syncthreads();
        // ---- T = X W1^T (IDENT1): dX = dT W1 -> G (waves 0-3); dW1 += dT^T X, and dgamma1, dbeta1 for both (waves 4-7)
        if (wave < 4) {
            if (want_dx) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                tile_gemm(D, reinterpret_cast<const float4 *>(p.wpt1) + wave * (16 * 64), acc, lane, 16);
                acc_to_lds(G, acc, lane, wave);
            }
        } else if (want_rec) {
            if constexpr (IDENT1) {
                if (want_w1) wgrad_tile(D, XT, A[4], A[5], A[6], A[7], wave - 4, lane);
            }
            s1 += tile_colsum(which ? P2 : P1, col);
        }
        __syncthreads();      // every tile is next written behind this barrier, G two barriers from here
        if (want_dx && live) {
            RowVals dx = row_load(G, tid);
            // g2 again from memory (the same bits) instead of 16 registers held across the tile's four barriers: with them the
            // row waves' GroupNorm recomputation does not fit next to the eight accumulator tiles
            RowVals gr = row_load_global(p.d_out + n * kC, tid);
            row_mask_pos(gr, row_load_global(p.out + n * kC, tid));
            row_add(dx, gr);
            row_store_global(p.dX + n * kC, tid, dx);
        }
    }

    if (!want_rec || wave < 4) return;
    float *rec = p.rec + (int64_t)blockIdx.x * lc_rec_floats(IDENT1);
    wgrad_store(rec, A[0], A[1], A[2], A[3], wave - 4, lane);
    if constexpr (IDENT1) wgrad_store(rec + kC * kC, A[4], A[5], A[6], A[7], wave - 4, lane);
    float *tail = rec + (IDENT1 ? 2 : 1) * kC * kC;
    tail[which * kC + col] = s2;
    tail[(2 + which) * kC + col] = s1;
}

// out = sum over the chunk records, in chunk order.  Record: dW2 [128,128], dW1 [128,128] (ident1 only), then four [128]
// vectors: dgamma2, dbeta2, dgamma1, dbeta1.
__global__ __launch_bounds__(256) void k_lc_bwd_reduce(const float *__restrict__ rec, int n_rec, int ident1, const LcBwdOut o) {
    const int n_w = (ident1 ? 2 : 1) * kC * kC, n_e = n_w + 4 * kC;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_e) return;
    float *dst = nullptr;
    if (e < kC * kC) dst = o.dw2 ? o.dw2 + e : nullptr;
    else if (e < n_w) dst = o.dw1 ? o.dw1 + (e - kC * kC) : nullptr;
    else {
        const int v = (e - n_w) >> 7, c = e & 127;
        float *const vec = v == 0 ? o.dg2 : v == 1 ? o.db2 : v == 2 ? o.dg1 : o.db1;
        if (vec != nullptr) dst = vec + c;
    }
    if (dst == nullptr) return;
    float s = 0.f;
    for (int k = 0; k < n_rec; ++k) s += rec[(int64_t)k * n_e + e];
    *dst = s;
}

// ----------------------------------------------------- pool pairs bwd -----
// Backward of the pair stage of LanePooling for dS [T,128] (include/lgcn.h, lgcn_pool_pairs_bwd), shaped like k_att_pairs_bwd
// with one GEMM and one GroupNorm less: workgroup `chunk` walks the 32-pair tiles chunk, chunk + n_chunks, ...  Per tile,
// waves 0-3 recompute h and z and the GroupNorm statistics with the forward's device functions, apply the stored masks, run
// the GroupNorm backward in registers (dz -> G and memory) and the dh GEMM on the transposed image.  Waves 4-7 own what is
// summed over pairs, in registers across the workgroup's tiles: dW_0h on wgrad_tile (wave 4 + q: block q, A[0..3]) and the
// seven [128] vectors as column sums over the tile's rows, in row order: dgamma / dbeta from the tiles P1 = g * zhat and
// P2 = g, and db_p and the four columns of dW_p from ONE tile, dy0, whose column c thread (which, c) sums plainly (db_p) and
// weighted with the rows' d (D4, 32 x 4 floats, broadcast reads).  Five product tiles dy0, dy0 * d.x, ... would have to sit
// in H and X as well, which the next tile's first two phases rewrite while waves 4-7 still sum them: that costs two more
// barriers per tile or two more tiles of LDS, and four more tile stores per row thread either way.
// LDS: H (h), X (GEMM output), G (dz), P1 / P2 (g * zhat / g, then dy0 in P1), D4: 5 x 16.5 KiB + 512 B.  Four barriers per
// tile.
constexpr int kPoolRecTail = 7 * kC;
constexpr int kPoolRec = kC * kC + kPoolRecTail;          // floats per chunk record

// sum over the 32 rows of T[r][c] * w[4 r], in row order (w: one of the four columns of a 32 x 4 LDS array)
__device__ __forceinline__ float tile_colsum_w(const float *T, int c, const float *w) {
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) s += T[r * kLDA + c] * w[4 * r];
    return s;
}

__global__ __launch_bounds__(512) void k_pool_pairs_bwd(const PoolBwdParams p) {
    __shared__ __attribute__((aligned(16))) float smem[5 * kTileFloats + 4 * kTM32];
    float *H = smem, *X = smem + kTileFloats, *G = smem + 2 * kTileFloats, *P1 = smem + 3 * kTileFloats;
    float *P2 = smem + 4 * kTileFloats, *D4 = smem + 5 * kTileFloats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool rowt = tid < 256;
    const int which = (tid >> 7) & 1, col = tid & 127;       // waves 4-7: column sums
    const PoolParams &f = p.f;
    int64_t P = *f.n_pairs;
    if (P < 0 || P > f.cap) P = f.cap;
    const int64_t n_tiles = (P + kTM32 - 1) / kTM32;
    const bool want_rec = p.rec != nullptr, want_p = p.want_p != 0, want_w = p.want_w != 0;

    f32x16 A[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) A[k][i] = 0.f;
    float s_g = 0.f, s_b = 0.f, s_w0 = 0.f, s_w1 = 0.f;      // which = 0: dgamma, db_p, dW_p[:,0], dW_p[:,1]; 1: dbeta, -, dW_p[:,2], dW_p[:,3]
    bool pend = false;           // dy0 (P1) and d (D4) of the tile before are waiting
    f32x16 acc;

    auto pending_sums = [&]() {      // waves 4-7
        if (which == 0) s_b += tile_colsum(P1, col);
        s_w0 += tile_colsum_w(P1, col, D4 + 2 * which);
        s_w1 += tile_colsum_w(P1, col, D4 + 2 * which + 1);
    };

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t pr = tile * kTM32 + (tid >> 3);
        const bool live = rowt && pr < P;
        const uint4 *mk = live ? p.masks + pr * 2 : nullptr;              // rows past the count: no gradient
        int t = 0, c = 0;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            t = f.ti[pr]; c = f.ci[pr];
            const float4 a = reinterpret_cast<const float4 *>(f.ctx_pose)[c];
            const float4 b = reinterpret_cast<const float4 *>(f.tgt_pose)[t];
            d = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
        }
        // ---- forward again: h -> H, W_0h h -> X
        if (rowt) lin4_relu_to_lds(H, tid, d, f.wp, f.bp);
        __syncthreads();
        if (wave < 4) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            tile_gemm(H, reinterpret_cast<const float4 *>(f.wpc0h) + wave * (16 * 64), acc, lane, 16);
            acc_to_lds(X, acc, lane, wave);
        } else if (pend) {      // what the last row phase of the tile before left (P1 is next written behind the next barrier,
            pending_sums();     // D4 three barriers from here)
        }
        pend = false;
        __syncthreads();
        // ---- m = ReLU(GN(z)): g = dS[t] * mask1 (P1 = g * zhat, P2 = g), dz -> G and global
        if (rowt) {
            RowVals z = row_load(X, tid);
            RowVals g = row_zero();
            if (live) {
                row_add_global(z, f.U + (int64_t)c * kC, tid);
                row_add_global(g, p.dS + (int64_t)t * kC, tid);
            }
            const float rstd = row_gn_hat(z, f.eps);
            row_apply_mask(g, mk ? mk + 1 : mk, tid);
            if (want_rec) { row_store_lds(P1, tid, row_mul(g, z)); row_store_lds(P2, tid, g); }
            row_gn_bwd(g, z, rstd, tid, f.g);
            row_store_lds(G, tid, g);
            if (live && p.dz) row_store_global(p.dz + pr * kC, tid, g);
        }
        if (!want_rec) continue;                // uniform; H's readers are past the barrier above, X is next written a barrier on
        __syncthreads();
        // ---- z = W_0h h + U[c]: dh = dz W_0h -> X (waves 0-3); dW_0h += dz^T h, dgamma, dbeta (waves 4-7)
        if (wave < 4) {
            if (want_p) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                tile_gemm(G, reinterpret_cast<const float4 *>(p.wptc0h) + wave * (16 * 64), acc, lane, 16);
                acc_to_lds(X, acc, lane, wave);
            }
        } else {
            if (want_w) wgrad_tile(G, H, A[0], A[1], A[2], A[3], wave - 4, lane);
            s_g += tile_colsum(which ? P2 : P1, col);
        }
        __syncthreads();                        // H, G, P1 and P2 are free behind this barrier
        if (!want_p) continue;                  // uniform
        // ---- h = ReLU(W_p d + b_p): dy0 = dh * mask0 -> P1, d -> D4; waves 4-7 sum them behind the next barrier (the next
        // tile's first, or the one after the loop)
        if (rowt) {
            RowVals g = row_load(X, tid);
            row_apply_mask(g, mk, tid);
            row_store_lds(P1, tid, g);
            if ((tid & 7) == 0) *reinterpret_cast<float4 *>(D4 + 4 * (tid >> 3)) = d;
        }
        pend = true;
    }

    if (!want_rec) return;
    if (pend) {
        __syncthreads();
        if (wave >= 4) pending_sums();
    }
    if (wave >= 4) {
        float *rec = p.rec + (int64_t)blockIdx.x * kPoolRec;
        wgrad_store(rec, A[0], A[1], A[2], A[3], wave - 4, lane);
        float *tail = rec + kC * kC;
        tail[which * kC + col] = s_g;
        if (which == 0) tail[2 * kC + col] = s_b;
        tail[(3 + 2 * which) * kC + col] = s_w0;
        tail[(4 + 2 * which) * kC + col] = s_w1;
    }
}

// out = sum over the chunk records, in chunk order.  Record: dW_0h [128,128], then seven [128] vectors: dgamma, dbeta, db_p,
// dW_p[:,0], dW_p[:,1], dW_p[:,2], dW_p[:,3].
__global__ __launch_bounds__(256) void k_pool_pairs_bwd_reduce(const float *__restrict__ rec, int n_rec, const PoolBwdOut o) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kPoolRec) return;
    float *dst = nullptr;
    if (e < kC * kC) dst = o.dw0h ? o.dw0h + e : nullptr;
    else {
        const int v = (e - kC * kC) >> 7, c = e & 127;
        float *const vec = v == 0 ? o.dg : v == 1 ? o.dbt : v == 2 ? o.dbp : o.dwp;
        if (vec != nullptr) dst = v < 3 ? vec + c : vec + 4 * c + (v - 3);
    }
    if (dst == nullptr) return;
    float s = 0.f;
    for (int k = 0; k < n_rec; ++k) s += rec[(int64_t)k * kPoolRec + e];
    *dst = s;
}

// ------------------------------------------------------ row block bwd -----
// Backward of one row block out = [ReLU]([GN](sum_r src_r W_r^T) [+ res]) with NREL = 1 or 2 IDENT relations
// (include/lgcn.h, lgcn_rowblock_bwd): the lower half of k_lc_bwd_rows<true> as a kernel of its own.  Workgroup `chunk`
// walks the 32-row tiles chunk, chunk + n_chunks, ...  Waves 0-3 are the row phase (8 threads per row: g = d_out masked by
// out > 0, d_res = g, and with GN the tiles P1 = g * xhat, P2 = g and dT = GroupNorm backward of g; without GN dT = g, so
// that a plain Linear stages d_out straight into D) and then the NREL tile GEMMs dT W_r -> G_r, which the row threads store
// behind the barrier.  Waves 4-7 stage the src_r rows and own everything summed over rows, in registers across the
// workgroup's tiles: dW_r on wgrad_tile (wave 4 + q: block q of every relation) and, with GN, dgamma / dbeta as column sums
// of P1 / P2.  LDS: D, G_r, S_r (src_r rows) and, with GN, P1 / P2: 3 + 2 (NREL - 1) + 2 GN tiles of 16.5 KiB, seven at
// the most.  Two barriers per tile.
struct RbBwdParams {
    const float *d_out, *out, *pre, *gamma;
    const float *src[2], *wpt[2];
    float *d_src[2], *d_res, *rec;
    int64_t n_rows;
    float eps;
    int want_w[2], want_gn;
};

struct RbBwdOut { float *dw[2], *dg, *db; int ld[2]; };

__host__ __device__ constexpr int rb_rec_floats(int n_rel) { return n_rel * kC * kC + 2 * kC; }

template <int NREL, bool GN>
__global__ __launch_bounds__(512) void k_rb_bwd_rows(const RbBwdParams p) {
    constexpr int kTiles = 1 + 2 * NREL + (GN ? 2 : 0);
    __shared__ __attribute__((aligned(16))) float smem[kTiles * kTileFloats];
    float *D = smem, *G = smem + kTileFloats, *S = smem + (1 + NREL) * kTileFloats;      // G, S: NREL tiles each
    float *P1 = smem + (GN ? 1 + 2 * NREL : 0) * kTileFloats, *P2 = smem + (GN ? 2 + 2 * NREL : 0) * kTileFloats;   // GN only
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool rowt = tid < 256;
    const int which = (tid >> 7) & 1, col = tid & 127;       // waves 4-7: column sums
    const int64_t n_tiles = (p.n_rows + kTM32 - 1) / kTM32;
    const bool want_rec = p.rec != nullptr, want_gn = GN && p.want_gn != 0;

    f32x16 A[4 * NREL];
#pragma unroll
    for (int k = 0; k < 4 * NREL; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) A[k][i] = 0.f;
    float s = 0.f;      // which = 0: dgamma; 1: dbeta
    f32x16 acc;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t n = tile * kTM32 + (tid >> 3);
        const bool live = rowt && n < p.n_rows;
        // ---- g = d_out * (out > 0) -> d_res; GN: P1 = g * xhat, P2 = g, dT = GN backward of g; dT -> D.  Waves 4-7 stage src_r
        if (rowt) {
            RowVals g = row_zero();
            if (live) {
                g = row_load_global(p.d_out + n * kC, tid);
                if (p.out) row_mask_pos(g, row_load_global(p.out + n * kC, tid));
                if (p.d_res) row_store_global(p.d_res + n * kC, tid, g);
            }
            if constexpr (GN) {
                RowVals x = row_zero();
                if (live) x = row_load_global(p.pre + n * kC, tid);
                const float rstd = row_gn_hat(x, p.eps);
                if (want_gn) { row_store_lds(P1, tid, row_mul(g, x)); row_store_lds(P2, tid, g); }
                row_gn_bwd(g, x, rstd, tid, p.gamma);
            }
            row_store_lds(D, tid, g);
        } else {
#pragma unroll
            for (int r = 0; r < NREL; ++r)
                if (p.want_w[r]) stage_rows(S + r * kTileFloats, p.src[r], tile, p.n_rows, tid - 256);
        }
        __syncthreads();
        // ---- d_src_r = dT W_r -> G_r (waves 0-3); dW_r += dT^T src_r, dgamma, dbeta (waves 4-7)
        if (wave < 4) {
#pragma unroll
            for (int r = 0; r < NREL; ++r) {
                if (p.d_src[r] == nullptr) continue;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                tile_gemm(D, reinterpret_cast<const float4 *>(p.wpt[r]) + wave * (16 * 64), acc, lane, 16);
                acc_to_lds(G + r * kTileFloats, acc, lane, wave);
            }
        } else if (want_rec) {
#pragma unroll
            for (int r = 0; r < NREL; ++r)
                if (p.want_w[r]) wgrad_tile(D, S + r * kTileFloats, A[4 * r], A[4 * r + 1], A[4 * r + 2], A[4 * r + 3], wave - 4, lane);
            if constexpr (GN) {
                if (want_gn) s += tile_colsum(which ? P2 : P1, col);
            }
        }
        __syncthreads();      // D, P1, P2 and S_r are next written behind this barrier, G_r behind the next one
        if (live) {
#pragma unroll
            for (int r = 0; r < NREL; ++r)
                if (p.d_src[r]) row_store_global(p.d_src[r] + n * kC, tid, row_load(G + r * kTileFloats, tid));
        }
    }

    if (!want_rec || wave < 4) return;
    float *rec = p.rec + (int64_t)blockIdx.x * rb_rec_floats(NREL);
#pragma unroll
    for (int r = 0; r < NREL; ++r)
        if (p.want_w[r]) wgrad_store(rec + r * kC * kC, A[4 * r], A[4 * r + 1], A[4 * r + 2], A[4 * r + 3], wave - 4, lane);
    if constexpr (GN) {
        if (want_gn) rec[NREL * kC * kC + which * kC + col] = s;
    }
}

// out = sum over the chunk records, in chunk order.  Record: dW_0 [128,128], dW_1 [128,128] (two relations only), then
// dgamma, dbeta [128]; dW_r goes out with row stride ld[r] (a 128-column block of a wider weight gradient).
__global__ __launch_bounds__(256) void k_rb_bwd_reduce(const float *__restrict__ rec, int n_rec, int n_rel, const RbBwdOut o) {
    const int n_w = n_rel * kC * kC, n_e = n_w + 2 * kC;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_e) return;
    float *dst = nullptr;
    if (e < n_w) {
        const int r = e >> 14, row = (e >> 7) & 127, c = e & 127;
        if (o.dw[r] != nullptr) dst = o.dw[r] + (int64_t)row * o.ld[r] + c;
    } else {
        float *const vec = (e - n_w) < kC ? o.dg : o.db;
        if (vec != nullptr) dst = vec + (e & 127);
    }
    if (dst == nullptr) return;
    float s = 0.f;
    for (int k = 0; k < n_rec; ++k) s += rec[(int64_t)k * n_e + e];
    *dst = s;
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

static bool valid_mma(int mma) { return mma >= LGCN_MMA_F32 && mma <= LGCN_MMA_F16X2; }

int64_t lgcn_packed_bytes(int k_pad, int mma) {
    if (!valid_mma(mma) || k_pad < 8 || (k_pad & 7)) return LGCN_EINVAL;
    if (mma == LGCN_MMA_F32) return (int64_t)kC * k_pad * 4;
    if (k_pad != kC) return LGCN_ESHAPE;
    return (int64_t)(mma == LGCN_MMA_BF16X3 ? 3 : mma == LGCN_MMA_F16X2 ? 2 : 1) * kC * kC * 2;
}

int lgcn_pack_weight(const float *W, int ld, int k_real, int k_pad, int mma, void *out, void *stream) {
    LGCN_CHECK_PTR(W); LGCN_CHECK_PTR(out);
    if (!valid_mma(mma) || k_real < 1 || k_pad < k_real || (k_pad & 7) || ld < k_real) return LGCN_EINVAL;
    LGCN_CHECK_ALIGN16(out);
    if (mma != LGCN_MMA_F32) {
        if (k_real != kC || k_pad != kC) return LGCN_ESHAPE;
        return pack_weight_bf(W, ld, mma, 0, out, (hipStream_t)stream);
    }
    const int total = kC * k_pad;
    hipLaunchKernelGGL(k_pack_weight, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, W, ld, k_real, k_pad,
                       reinterpret_cast<float *>(out), 0);
    return launch_status();
}

int lgcn_pack_weight_t(const float *W, int ld, int mma, void *out, void *stream) {
    LGCN_CHECK_PTR(W); LGCN_CHECK_PTR(out);
    if (!valid_mma(mma) || ld < kC) return LGCN_EINVAL;
    LGCN_CHECK_ALIGN16(out);
    if (mma != LGCN_MMA_F32) return pack_weight_bf(W, ld, mma, 1, out, (hipStream_t)stream);
    hipLaunchKernelGGL(k_pack_weight, dim3(kC * kC / 256), dim3(256), 0, (hipStream_t)stream, W, ld, kC, kC,
                       reinterpret_cast<float *>(out), 1);
    return launch_status();
}

int lgcn_pack_weight_batch(const lgcn_pack_job_t *jobs, int n_jobs, int mma, void *stream) {
    if (!valid_mma(mma) || n_jobs < 0 || n_jobs > 65535) return LGCN_EINVAL;
    if (n_jobs == 0) return LGCN_OK;
    LGCN_CHECK_PTR(jobs);
    if (mma != LGCN_MMA_F32) return pack_weight_batch_bf(jobs, n_jobs, mma, (hipStream_t)stream);
    hipLaunchKernelGGL(k_pack_weight_batch, dim3(kC * kC / 256, n_jobs), dim3(256), 0, (hipStream_t)stream, jobs);
    return launch_status();
}

static_assert(sizeof(lgcn_agg_mlp_t) == 32 + LGCN_MAX_REL * 24 + 23 * 8 && LGCN_MAX_REL == 16,
              "lgcn_agg_mlp_t layout: keep lanegcn-1_amd/_lib.py (AggMlp) and tests/test_host_cabi.py in step");

// The relation table of a launch: sources, modes and the index arrays they need.  fwd: a forward launch, which also
// reads the packed weights and, in the split-precision modes, knows RANGE16; the weight gradient (fwd = false) does neither.
static int validate_rels(const lgcn_agg_mlp_t &p, bool fwd, bool *need_col_out) {
    bool need_rowptr = false, need_col = false;
    for (int r = 0; r < p.n_rel; ++r) {
        LGCN_CHECK_PTR(p.rel[r].src);
        if (fwd) LGCN_CHECK_PTR(p.rel[r].wp);
        LGCN_CHECK_ALIGN16(p.rel[r].src);
        if (fwd) LGCN_CHECK_ALIGN16(p.rel[r].wp);
        switch (p.rel[r].mode) {
            case LGCN_REL_IDENT: break;
            case LGCN_REL_CSR:
                if (p.rel[r].ridx < 0 || p.rel[r].ridx >= p.n_rel_csr) return LGCN_EINVAL;
                need_rowptr = need_col = true; break;
            case LGCN_REL_RANGE: need_rowptr = true; break;
            case LGCN_REL_RANGE16:          // split-precision forward kernels only
                if (!fwd) return LGCN_EINVAL;
                if (p.mma == LGCN_MMA_F32) return LGCN_ESHAPE;
                need_rowptr = true; break;
            default: return LGCN_EINVAL;
        }
    }
    if (need_rowptr) LGCN_CHECK_PTR(p.rowptr);
    if (need_col) LGCN_CHECK_PTR(p.col);
    *need_col_out = need_col;
    return LGCN_OK;
}

static int validate_agg(const lgcn_agg_mlp_t &p, bool *need_col_out) {
    if (p.n_rows < 0 || p.n_rel < 1 || p.n_rel > LGCN_MAX_REL || !valid_mma(p.mma)) return LGCN_EINVAL;
    constexpr int kKnownFlags = LGCN_F_GN1 | LGCN_F_RELU1 | LGCN_F_GEMM2 | LGCN_F_GN2 | LGCN_F_RES | LGCN_F_RELU2;
    if (p.flags & ~kKnownFlags) return LGCN_EINVAL;      // unknown bits are an error, not a silent no-op
    if (p.n_rows == 0) return LGCN_OK;
    if (p.n_rows > 0x7fffffff) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(p.out); LGCN_CHECK_ALIGN16(p.out);
    bool need_col = false;
    const int rc = validate_rels(p, true, &need_col);
    if (rc != LGCN_OK) return rc;
    if (need_col) {   // one rowptr per launch: a CSR plan and a RANGE prefix cannot be mixed
        for (int r = 0; r < p.n_rel; ++r)
            if (p.rel[r].mode == LGCN_REL_RANGE || p.rel[r].mode == LGCN_REL_RANGE16) return LGCN_EINVAL;
    }
    if (p.flags & LGCN_F_GN1) { LGCN_CHECK_PTR(p.gn1_g); LGCN_CHECK_PTR(p.gn1_b); LGCN_CHECK_ALIGN16(p.gn1_g); LGCN_CHECK_ALIGN16(p.gn1_b); }
    if (p.flags & LGCN_F_GEMM2) { LGCN_CHECK_PTR(p.wp2); LGCN_CHECK_ALIGN16(p.wp2); }
    if (p.flags & LGCN_F_GN2) {
        if (!(p.flags & LGCN_F_GEMM2)) return LGCN_EINVAL;
        LGCN_CHECK_PTR(p.gn2_g); LGCN_CHECK_PTR(p.gn2_b); LGCN_CHECK_ALIGN16(p.gn2_g); LGCN_CHECK_ALIGN16(p.gn2_b);
    }
    if ((p.flags & LGCN_F_RELU2) && !(p.flags & LGCN_F_GEMM2)) return LGCN_EINVAL;
    if (p.flags & LGCN_F_RES) { LGCN_CHECK_PTR(p.res); LGCN_CHECK_ALIGN16(p.res); }
    if (p.w4) { LGCN_CHECK_PTR(p.x4_a); LGCN_CHECK_PTR(p.x4_b); LGCN_CHECK_PTR(p.x4_c); LGCN_CHECK_ALIGN16(p.w4); }
    if (p.out_pre) LGCN_CHECK_ALIGN16(p.out_pre);
    if (p.out_mid) LGCN_CHECK_ALIGN16(p.out_mid);
    if (p.out_pre2) LGCN_CHECK_ALIGN16(p.out_pre2);
    if (p.ch_wu) {
        const void *q[] = {p.ch_wq, p.ch_gq_g, p.ch_gq_b, p.ch_wu, p.ch_u_out};
        for (const void *v : q) { LGCN_CHECK_PTR(v); LGCN_CHECK_ALIGN16(v); }
    }
    if (p.ch_wv) { LGCN_CHECK_PTR(p.ch_v_out); LGCN_CHECK_ALIGN16(p.ch_wv); LGCN_CHECK_ALIGN16(p.ch_v_out); }
    if ((p.ch_wu || p.ch_wv) && need_col) return LGCN_EINVAL;      // chained outputs: row blocks without CSR relations
    *need_col_out = need_col;
    return LGCN_OK;
}

// The chained outputs of a block as launches of their own on its `out` rows (exact-f32 mode, whose kernels have no
// chained stages): the same arithmetic, lanegcn.py:696-699.
static int chain_as_launches(const lgcn_agg_mlp_t &p, void *stream) {
    lgcn_agg_mlp_t q{};
    q.n_rows = p.n_rows; q.n_rel = 1; q.eps = p.eps; q.mma = p.mma;
    q.rel[0].src = p.out; q.rel[0].mode = LGCN_REL_IDENT;
    if (p.ch_wu) {
        q.rel[0].wp = p.ch_wq; q.flags = LGCN_F_GN1 | LGCN_F_RELU1 | LGCN_F_GEMM2;
        q.gn1_g = p.ch_gq_g; q.gn1_b = p.ch_gq_b; q.wp2 = p.ch_wu; q.out = p.ch_u_out;
        const int rc = lgcn_agg_mlp(&q, stream);
        if (rc != LGCN_OK) return rc;
    }
    if (p.ch_wv) {
        q.rel[0].wp = p.ch_wv; q.flags = 0; q.gn1_g = q.gn1_b = q.wp2 = nullptr; q.out = p.ch_v_out;
        return lgcn_agg_mlp(&q, stream);
    }
    return LGCN_OK;
}

int lgcn_agg_mlp(const lgcn_agg_mlp_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_agg_mlp_t &p = *ph;
    bool need_col = false;
    const int rc = validate_agg(p, &need_col);
    if (rc != LGCN_OK || p.n_rows == 0) return rc;
    if (p.mma != LGCN_MMA_F32) return agg_mlp_bf(p, need_col, (hipStream_t)stream);
    const int n_tiles = (int)((p.n_rows + kTM32 - 1) / kTM32);
    if (need_col)
        hipLaunchKernelGGL((k_agg_mlp<1>), dim3(n_tiles), dim3(512), 0, (hipStream_t)stream, p, n_tiles);
    else
        hipLaunchKernelGGL((k_agg_mlp<0>), dim3(n_tiles), dim3(512), 0, (hipStream_t)stream, p, n_tiles);
    const int st = launch_status();
    return st != LGCN_OK || !(p.ch_wu || p.ch_wv) ? st : chain_as_launches(p, stream);
}

int lgcn_agg_mlp_multi(const lgcn_agg_mlp_t *const *ps, int n, void *stream) {
    LGCN_CHECK_PTR(ps);
    if (n < 1 || n > LGCN_MAX_MULTI) return LGCN_EINVAL;
    bool one = true;
    for (int i = 0; i < n; ++i) {
        LGCN_CHECK_PTR(ps[i]);
        bool c = false;
        const int rc = validate_agg(*ps[i], &c);
        if (rc != LGCN_OK) return rc;
        one = one && ps[i]->n_rows > 0 && ps[i]->mma == ps[0]->mma && ps[i]->mma != LGCN_MMA_F32 && !c && ps[i]->tile_rb == ps[0]->tile_rb;
    }
    if (one && n > 1) return agg_mlp_multi_bf(ps, n, (hipStream_t)stream);
    for (int i = 0; i < n; ++i) {
        const int rc = lgcn_agg_mlp(ps[i], stream);
        if (rc != LGCN_OK) return rc;
    }
    return LGCN_OK;
}

int lgcn_agg_mlp_pair(const lgcn_agg_mlp_t *a, const lgcn_agg_mlp_t *b, void *stream) {
    LGCN_CHECK_PTR(a); LGCN_CHECK_PTR(b);
    bool ca = false, cb = false;
    int rc = validate_agg(*a, &ca);
    if (rc != LGCN_OK) return rc;
    rc = validate_agg(*b, &cb);
    if (rc != LGCN_OK) return rc;
    // one launch only for two non-empty split-precision problems without CSR relations in the same mode
    if (a->n_rows > 0 && b->n_rows > 0 && a->mma == b->mma && a->mma != LGCN_MMA_F32 && !ca && !cb &&
        a->tile_rb == 0 && b->tile_rb == 0)
        return agg_mlp_pair_bf(*a, *b, (hipStream_t)stream);
    rc = lgcn_agg_mlp(a, stream);
    return rc != LGCN_OK ? rc : lgcn_agg_mlp(b, stream);
}

int lgcn_mapnet_input(const float *ctrs, const float *feats, int64_t n_rows, const float *wa1, const float *ba1,
                      const float *wpa2, const float *ga, const float *bta, const float *ws1, const float *bs1,
                      const float *wps2, const float *gs, const float *bts, float eps, int mma, float *out, void *stream) {
    if (n_rows < 0 || !valid_mma(mma)) return LGCN_EINVAL;
    if (n_rows == 0) return LGCN_OK;
    if (n_rows > 0x7fffffff) return LGCN_ESHAPE;
    const void *ptrs[] = {ctrs, feats, wa1, ba1, wpa2, ga, bta, ws1, bs1, wps2, gs, bts, out};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {wa1, ba1, wpa2, ga, bta, ws1, bs1, wps2, gs, bts, out};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    InputParams p{ctrs, feats, n_rows, wa1, ba1, wpa2, ga, bta, ws1, bs1, wps2, gs, bts, eps, out};
    if (mma != LGCN_MMA_F32) return mapnet_input_bf(p, mma, (hipStream_t)stream);
    const int n_tiles = (int)((n_rows + kTM32 - 1) / kTM32);
    hipLaunchKernelGGL(k_mapnet_input, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, p, n_tiles);
    return launch_status();
}

int lgcn_att_pairs(const float *agt_ctrs, const float *ctx_ctrs, const int32_t *hi, const int32_t *wi,
                   const int32_t *n_pairs, int64_t cap, const float *wd0, const float *bd0, const float *wpd2,
                   const float *gd, const float *btd, const float *wpc0e, const float *U, const float *V,
                   const float *gc, const float *btc, float eps, int mma, float *m, void *stream) {
    if (cap < 0 || !valid_mma(mma)) return LGCN_EINVAL;
    if (mma != LGCN_MMA_F32) return LGCN_ESHAPE;      // split-precision modes: lgcn_att_pairs_ws / lgcn_att_pairs_wi
    if (cap == 0) return LGCN_OK;
    if (cap > 0x7ffffff0) return LGCN_ESHAPE;
    const void *ptrs[] = {agt_ctrs, ctx_ctrs, hi, wi, n_pairs, wd0, bd0, wpd2, gd, btd, wpc0e, U, V, gc, btc, m};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {wd0, bd0, wpd2, gd, btd, wpc0e, U, V, gc, btc, m};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    PairParams p{agt_ctrs, ctx_ctrs, hi, wi, n_pairs, cap, wd0, bd0, wpd2, gd, btd, wpc0e, U, V, gc, btc, eps, m};
    int64_t tiles = (cap + kTM32 - 1) / kTM32;
    const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);
    hipLaunchKernelGGL(k_att_pairs<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, (uint4 *)nullptr);
    return launch_status();
}

int lgcn_att_pairs_train(const float *agt_ctrs, const float *ctx_ctrs, const int32_t *hi, const int32_t *wi,
                         const int32_t *n_pairs, int64_t cap, const float *wd0, const float *bd0, const float *wpd2,
                         const float *gd, const float *btd, const float *wpc0e, const float *U, const float *V,
                         const float *gc, const float *btc, float eps, float *m, uint32_t *masks, void *stream) {
    if (cap < 0) return LGCN_EINVAL;
    if (cap == 0) return LGCN_OK;
    if (cap > 0x7ffffff0) return LGCN_ESHAPE;
    const void *ptrs[] = {agt_ctrs, ctx_ctrs, hi, wi, n_pairs, wd0, bd0, wpd2, gd, btd, wpc0e, U, V, gc, btc, m, masks};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {wd0, bd0, wpd2, gd, btd, wpc0e, U, V, gc, btc, m, masks};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    PairParams p{agt_ctrs, ctx_ctrs, hi, wi, n_pairs, cap, wd0, bd0, wpd2, gd, btd, wpc0e, U, V, gc, btc, eps, m};
    const int64_t tiles = (cap + kTM32 - 1) / kTM32;
    const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);
    hipLaunchKernelGGL(k_att_pairs<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, reinterpret_cast<uint4 *>(masks));
    return launch_status();
}

int lgcn_pool_pairs(const float *ctx_pose, const float *tgt_pose, const int32_t *ti, const int32_t *ci,
                    const int32_t *n_pairs, int64_t cap, const float *wp, const float *bp, const float *wpc0h,
                    const float *U, const float *g, const float *bt, float eps, float *m, void *stream) {
    if (cap < 0) return LGCN_EINVAL;
    if (cap == 0) return LGCN_OK;
    if (cap > 0x7ffffff0) return LGCN_ESHAPE;
    const void *ptrs[] = {ctx_pose, tgt_pose, ti, ci, n_pairs, wp, bp, wpc0h, U, g, bt, m};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {ctx_pose, tgt_pose, wp, bp, wpc0h, U, g, bt, m};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    PoolParams p{ctx_pose, tgt_pose, ti, ci, n_pairs, cap, wp, bp, wpc0h, U, g, bt, eps, m};
    const int64_t tiles = (cap + kTM32 - 1) / kTM32;
    const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);
    hipLaunchKernelGGL(k_pool_pairs<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, (uint4 *)nullptr);
    return launch_status();
}

int lgcn_pool_pairs_train(const float *ctx_pose, const float *tgt_pose, const int32_t *ti, const int32_t *ci,
                          const int32_t *n_pairs, int64_t cap, const float *wp, const float *bp, const float *wpc0h,
                          const float *U, const float *g, const float *bt, float eps, float *m, uint32_t *masks, void *stream) {
    if (cap < 0) return LGCN_EINVAL;
    if (cap == 0) return LGCN_OK;
    if (cap > 0x7ffffff0) return LGCN_ESHAPE;
    const void *ptrs[] = {ctx_pose, tgt_pose, ti, ci, n_pairs, wp, bp, wpc0h, U, g, bt, m, masks};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {ctx_pose, tgt_pose, wp, bp, wpc0h, U, g, bt, m, masks};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    PoolParams p{ctx_pose, tgt_pose, ti, ci, n_pairs, cap, wp, bp, wpc0h, U, g, bt, eps, m};
    const int64_t tiles = (cap + kTM32 - 1) / kTM32;
    const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);
    hipLaunchKernelGGL(k_pool_pairs<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, reinterpret_cast<uint4 *>(masks));
    return launch_status();
}

static_assert(sizeof(lgcn_att_pairs_bwd_t) == 31 * 8,
              "lgcn_att_pairs_bwd_t layout: keep lanegcn-1_amd/_lib.py (AttPairsBwd) and tests/test_host_att_train_cabi.py in step");

// workgroups of a backward launch: never more than the tiles that cap allows
static int64_t pair_bwd_chunks(int64_t cap, int n_chunks) {
    const int64_t tiles = (cap + kTM32 - 1) / kTM32;
    return tiles < n_chunks ? tiles : n_chunks;
}

int64_t lgcn_att_pairs_bwd_ws_elems(int64_t cap, int n_chunks) {
    if (cap < 0 || cap > 0x7ffffff0 || n_chunks < 1 || n_chunks > 1024) return LGCN_EINVAL;
    return pair_bwd_chunks(cap, n_chunks) * kPairRec;
}

int lgcn_att_pairs_bwd(const lgcn_att_pairs_bwd_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_att_pairs_bwd_t &a = *ph;
    if (a.cap < 0 || a.n_chunks < 1 || a.n_chunks > 1024) return LGCN_EINVAL;
    if (a.cap == 0) return LGCN_OK;
    if (a.cap > 0x7ffffff0) return LGCN_ESHAPE;
    const bool want_d = a.d_wd2 || a.d_wd0 || a.d_bd0 || a.d_gd || a.d_btd;
    const bool want_rec = want_d || a.d_wc0e || a.d_gc || a.d_btc;
    const void *ptrs[] = {a.agt_ctrs, a.ctx_ctrs, a.hi, a.wi, a.n_pairs, a.wd0, a.bd0, a.wpd2, a.gd, a.btd, a.wpc0e, a.U, a.V,
                          a.gc, a.btc, a.masks, a.dS};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    if (want_d) { LGCN_CHECK_PTR(a.wptd2); LGCN_CHECK_PTR(a.wptc0e); }
    if (want_rec) LGCN_CHECK_PTR(a.ws);
    const void *al[] = {a.wd0, a.bd0, a.wpd2, a.gd, a.btd, a.wpc0e, a.U, a.V, a.gc, a.btc, a.masks, a.dS, a.wptd2, a.wptc0e,
                        a.dc, a.ws, a.d_wd2, a.d_wc0e, a.d_wd0, a.d_bd0, a.d_gd, a.d_btd, a.d_gc, a.d_btc};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);      // absent (null) ones pass
    if (!want_rec && a.dc == nullptr) return LGCN_OK;
    PairBwdParams p{};
    p.f = PairParams{a.agt_ctrs, a.ctx_ctrs, a.hi, a.wi, a.n_pairs, a.cap, a.wd0, a.bd0, a.wpd2, a.gd, a.btd, a.wpc0e, a.U, a.V,
                     a.gc, a.btc, a.eps, nullptr};
    p.wptd2 = a.wptd2; p.wptc0e = a.wptc0e;
    p.masks = reinterpret_cast<const uint4 *>(a.masks);
    p.dS = a.dS; p.dc = a.dc; p.rec = want_rec ? a.ws : nullptr;
    p.want_d = want_d; p.want_wc = a.d_wc0e != nullptr;
    const int n_rec = (int)pair_bwd_chunks(a.cap, a.n_chunks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_att_pairs_bwd, dim3(n_rec), dim3(512), 0, st, p);
    if (want_rec) {
        const PairBwdOut o{a.d_wd2, a.d_wc0e, a.d_gc, a.d_btc, a.d_gd, a.d_btd, a.d_bd0, a.d_wd0};
        hipLaunchKernelGGL(k_att_pairs_bwd_reduce, dim3((kPairRec + 255) / 256), dim3(256), 0, st, a.ws, n_rec, o);
    }
    return launch_status();
}

static_assert(sizeof(lgcn_pool_pairs_bwd_t) == 23 * 8,
              "lgcn_pool_pairs_bwd_t layout: keep lanegcn-1_amd/_lib.py (PoolPairsBwd) and tests/test_host_pool_train_cabi.py in step");

int64_t lgcn_pool_pairs_bwd_ws_elems(int64_t cap, int n_chunks) {
    if (cap < 0 || cap > 0x7ffffff0 || n_chunks < 1 || n_chunks > 1024) return LGCN_EINVAL;
    return pair_bwd_chunks(cap, n_chunks) * kPoolRec;
}

int lgcn_pool_pairs_bwd(const lgcn_pool_pairs_bwd_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_pool_pairs_bwd_t &a = *ph;
    if (a.cap < 0 || a.n_chunks < 1 || a.n_chunks > 1024) return LGCN_EINVAL;
    if (a.cap == 0) return LGCN_OK;
    if (a.cap > 0x7ffffff0) return LGCN_ESHAPE;
    const bool want_p = a.d_wp || a.d_bp;
    const bool want_rec = want_p || a.d_w0h || a.d_g || a.d_bt;
    const void *ptrs[] = {a.ctx_pose, a.tgt_pose, a.ti, a.ci, a.n_pairs, a.wp, a.bp, a.wpc0h, a.U, a.g, a.bt, a.masks, a.dS};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    if (want_p) LGCN_CHECK_PTR(a.wptc0h);
    if (want_rec) LGCN_CHECK_PTR(a.ws);
    const void *al[] = {a.ctx_pose, a.tgt_pose, a.wp, a.bp, a.wpc0h, a.U, a.g, a.bt, a.masks, a.dS, a.wptc0h, a.dz, a.ws,
                        a.d_w0h, a.d_wp, a.d_bp, a.d_g, a.d_bt};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);      // absent (null) ones pass
    if (!want_rec && a.dz == nullptr) return LGCN_OK;
    PoolBwdParams p{};
    p.f = PoolParams{a.ctx_pose, a.tgt_pose, a.ti, a.ci, a.n_pairs, a.cap, a.wp, a.bp, a.wpc0h, a.U, a.g, a.bt, a.eps, nullptr};
    p.wptc0h = a.wptc0h;
    p.masks = reinterpret_cast<const uint4 *>(a.masks);
    p.dS = a.dS; p.dz = a.dz; p.rec = want_rec ? a.ws : nullptr;
    p.want_p = want_p; p.want_w = a.d_w0h != nullptr;
    const int n_rec = (int)pair_bwd_chunks(a.cap, a.n_chunks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pool_pairs_bwd, dim3(n_rec), dim3(512), 0, st, p);
    if (want_rec) {
        const PoolBwdOut o{a.d_w0h, a.d_wp, a.d_bp, a.d_g, a.d_bt};
        hipLaunchKernelGGL(k_pool_pairs_bwd_reduce, dim3((kPoolRec + 255) / 256), dim3(256), 0, st, a.ws, n_rec, o);
    }
    return launch_status();
}

static_assert(sizeof(lgcn_laneconv_bwd_t) == 23 * 8,
              "lgcn_laneconv_bwd_t layout: keep lanegcn-1_amd/_lib.py (LaneConvBwd) and tests/test_host_laneconv_bwd_cabi.py in step");

// workgroups of a backward launch: never more than the 32-row tiles
static int64_t lc_bwd_chunks(int64_t n_rows, int n_chunks) {
    const int64_t tiles = (n_rows + kTM32 - 1) / kTM32;
    return tiles < n_chunks ? tiles : n_chunks;
}

int64_t lgcn_laneconv_bwd_ws_elems(int64_t n_rows, int n_chunks, int ident1) {
    if (n_rows < 0 || n_rows > 0x7fffffff || n_chunks < 1 || n_chunks > 1024 || (ident1 != 0 && ident1 != 1)) return LGCN_EINVAL;
    return lc_bwd_chunks(n_rows, n_chunks) * lc_rec_floats(ident1 != 0);
}

int lgcn_laneconv_bwd(const lgcn_laneconv_bwd_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_laneconv_bwd_t &a = *ph;
    if (a.n_rows < 0 || a.n_chunks < 1 || a.n_chunks > 1024 || (a.ident1 != 0 && a.ident1 != 1)) return LGCN_EINVAL;
    if (a.n_rows == 0) return LGCN_OK;
    if (a.n_rows > 0x7fffffff) return LGCN_ESHAPE;
    const bool ident1 = a.ident1 != 0;
    // outputs of the other variant are an error, not a silent no-op
    if (ident1 ? (a.dT || a.g2) : (a.dX || a.d_w1)) return LGCN_EINVAL;
    const bool want_rec = a.d_w2 || a.d_w1 || a.d_g2 || a.d_b2 || a.d_g1 || a.d_b1;
    const void *ptrs[] = {a.d_out, a.out, a.Z, a.Y, a.T, a.gamma1, a.gamma2, a.wpt2};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    if (ident1) { LGCN_CHECK_PTR(a.X); LGCN_CHECK_PTR(a.wpt1); }
    if (want_rec) LGCN_CHECK_PTR(a.ws);
    const void *al[] = {a.d_out, a.out, a.Z, a.Y, a.T, a.X, a.gamma1, a.gamma2, a.wpt2, a.wpt1, a.dT, a.g2, a.dX,
                        a.d_w2, a.d_w1, a.d_g2, a.d_b2, a.d_g1, a.d_b1, a.ws};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);      // absent (null) ones pass
    if (!want_rec && !(ident1 ? a.dX != nullptr : (a.dT || a.g2))) return LGCN_OK;
    LcBwdParams p{a.d_out, a.out, a.Z, a.Y, a.T, a.X, a.gamma1, a.gamma2, a.wpt2, a.wpt1, a.dT, a.g2, a.dX,
                  want_rec ? a.ws : nullptr, a.n_rows, a.eps, a.d_w2 != nullptr, a.d_w1 != nullptr};
    const int n_rec = (int)lc_bwd_chunks(a.n_rows, a.n_chunks);
    hipStream_t st = (hipStream_t)stream;
    if (ident1) hipLaunchKernelGGL(k_lc_bwd_rows<true>, dim3(n_rec), dim3(512), 0, st, p);
    else hipLaunchKernelGGL(k_lc_bwd_rows<false>, dim3(n_rec), dim3(512), 0, st, p);
    if (want_rec) {
        const LcBwdOut o{a.d_w2, a.d_w1, a.d_g2, a.d_b2, a.d_g1, a.d_b1};
        hipLaunchKernelGGL(k_lc_bwd_reduce, dim3((lc_rec_floats(ident1) + 255) / 256), dim3(256), 0, st, a.ws, n_rec,
                           (int)ident1, o);
    }
    return launch_status();
}

static_assert(sizeof(lgcn_rowblock_bwd_t) == 20 * 8,
              "lgcn_rowblock_bwd_t layout: keep lanegcn-1_amd/_lib.py (RowBlockBwd) and tests/test_host_rowblock_bwd_cabi.py in step");

int64_t lgcn_rowblock_bwd_ws_elems(int64_t n_rows, int n_chunks, int n_rel) {
    if (n_rows < 0 || n_rows > 0x7fffffff || n_chunks < 1 || n_chunks > 1024 || n_rel < 1 || n_rel > 2) return LGCN_EINVAL;
    return lc_bwd_chunks(n_rows, n_chunks) * rb_rec_floats(n_rel);
}

int lgcn_rowblock_bwd(const lgcn_rowblock_bwd_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_rowblock_bwd_t &a = *ph;
    if (a.n_rows < 0) return LGCN_EINVAL;
    if (a.n_rows > 0x7fffffff) return LGCN_ESHAPE;
    if (a.n_rel < 1 || a.n_rel > 2 || a.n_chunks < 1 || a.n_chunks > 1024) return LGCN_EINVAL;
    if (a.n_rows == 0) return LGCN_OK;
    const int n_rel = a.n_rel;
    const bool gn = a.pre != nullptr;
    LGCN_CHECK_PTR(a.d_out);
    if (gn != (a.gamma != nullptr)) return LGCN_EINVAL;
    if (!gn && (a.d_gamma || a.d_beta)) return LGCN_EINVAL;
    bool want_rec = a.d_gamma || a.d_beta, want_rows = a.d_res != nullptr;
    for (int r = 0; r < n_rel; ++r) {
        LGCN_CHECK_PTR(a.src[r]); LGCN_CHECK_PTR(a.wpt[r]);
        want_rec = want_rec || a.d_w[r];
        want_rows = want_rows || a.d_src[r];
    }
    if (want_rec) LGCN_CHECK_PTR(a.ws);
    for (int r = 0; r < n_rel; ++r)
        if (a.d_w[r] && (a.ld_w[r] < kC || (a.ld_w[r] & 3) != 0)) return LGCN_EINVAL;
    const void *al[] = {a.d_out, a.out, a.pre, a.gamma, a.src[0], a.src[1], a.wpt[0], a.wpt[1], a.d_src[0], a.d_src[1],
                        a.d_w[0], a.d_w[1], a.d_res, a.d_gamma, a.d_beta, a.ws};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);      // absent (null) ones pass
    if (!want_rec && !want_rows) return LGCN_OK;
    RbBwdParams p{};
    p.d_out = a.d_out; p.out = a.out; p.pre = a.pre; p.gamma = a.gamma;
    RbBwdOut o{};
    for (int r = 0; r < n_rel; ++r) {
        p.src[r] = a.src[r]; p.wpt[r] = a.wpt[r]; p.d_src[r] = a.d_src[r]; p.want_w[r] = a.d_w[r] != nullptr;
        o.dw[r] = a.d_w[r]; o.ld[r] = a.ld_w[r];
    }
    p.d_res = a.d_res; p.rec = want_rec ? a.ws : nullptr;
    p.n_rows = a.n_rows; p.eps = a.eps; p.want_gn = a.d_gamma || a.d_beta;
    o.dg = a.d_gamma; o.db = a.d_beta;
    const int n_rec = (int)lc_bwd_chunks(a.n_rows, a.n_chunks);
    hipStream_t st = (hipStream_t)stream;
    if (n_rel == 2) {
        if (gn) hipLaunchKernelGGL((k_rb_bwd_rows<2, true>), dim3(n_rec), dim3(512), 0, st, p);
        else hipLaunchKernelGGL((k_rb_bwd_rows<2, false>), dim3(n_rec), dim3(512), 0, st, p);
    } else {
        if (gn) hipLaunchKernelGGL((k_rb_bwd_rows<1, true>), dim3(n_rec), dim3(512), 0, st, p);
        else hipLaunchKernelGGL((k_rb_bwd_rows<1, false>), dim3(n_rec), dim3(512), 0, st, p);
    }
    if (want_rec)
        hipLaunchKernelGGL(k_rb_bwd_reduce, dim3((rb_rec_floats(n_rel) + 255) / 256), dim3(256), 0, st, a.ws, n_rec, n_rel, o);
    return launch_status();
}

int lgcn_wgrad(const lgcn_agg_mlp_t *ph, const float *dT, float *dW, float *part, int n_chunks, void *stream) {
    LGCN_CHECK_PTR(ph); LGCN_CHECK_PTR(dT); LGCN_CHECK_PTR(dW); LGCN_CHECK_PTR(part);
    const lgcn_agg_mlp_t &p = *ph;
    if (p.n_rows < 0 || p.n_rel < 1 || p.n_rel > LGCN_MAX_REL || n_chunks < 1 || n_chunks > 1024) return LGCN_EINVAL;
    if (p.n_rows > 0x7fffffff) return LGCN_ESHAPE;
    LGCN_CHECK_ALIGN16(dT); LGCN_CHECK_ALIGN16(dW); LGCN_CHECK_ALIGN16(part);
    bool need_col = false;
    const int rc = validate_rels(p, false, &need_col);
    if (rc != LGCN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int n_tiles = (int)((p.n_rows + kTM32 - 1) / kTM32);
    hipLaunchKernelGGL(k_wgrad, dim3(n_chunks, p.n_rel), dim3(512), 0, st, p, dT, part, n_tiles, n_chunks);
    hipLaunchKernelGGL(k_wgrad_reduce, dim3(kC * kC / 256, p.n_rel), dim3(256), 0, st, part, n_chunks, dW);
    return launch_status();
}

}  // extern "C"
