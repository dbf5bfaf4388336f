// Device helpers, parameter structs and the relation check that the forward row-block kernels (lgcn_rowmlp.hip) and their
// backward (lgcn_rowmlp_bwd.hip) share.  Only those two files include it.
#pragma once
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

// ------------------------------------------------------------ relations ---
// One relation's gathered source rows of a 32-row tile into an LDS tile (gt = 0..255 of the four gathering waves)
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

// ---------------------------------------------------------- first layers --
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

// ---------------------------------------------------------- mask words -----
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


// ------------------------------------------------------- parameter structs -
// lgcn_pool_pairs: the pair stage of the fork's LanePooling (see include/lgcn.h)
struct PoolParams {
    const float *ctx_pose, *tgt_pose;
    const int32_t *ti, *ci, *n_pairs;
    int64_t cap;
    const float *wp, *bp, *wpc0h, *U, *g, *bt;
    float eps;
    float *m;
};

// lgcn_att_pairs_bwd: the forward's inputs, what it saved and the gradient outputs (see include/lgcn.h)
struct PairBwdParams {
    PairParams f;
    const float *wptd2, *wptc0e;      // transposed images of W_d2 and W_c0[:, 0:128]
    const uint4 *masks;
    const float *dS;
    float *dc, *rec;
    int want_d, want_wc;              // anything upstream of e (the dist parameters) / dW_c0e
};

// lgcn_pool_pairs_bwd: the forward's inputs, what it saved and the gradient outputs (see include/lgcn.h)
struct PoolBwdParams {
    PoolParams f;
    const float *wptc0h;              // transposed image of W_0[:, 128:256]
    const uint4 *masks;
    const float *dS;
    float *dz, *rec;
    int want_p, want_w;               // anything upstream of h (relpose.0's parameters) / dW_0h
};

// ------------------------------------------------------------- host side ---
// lgcn_agg_mlp_t is the kernel argument of the forward launches and of k_wgrad
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

}  // namespace lgcn
