// Row-phase helpers shared by the f32 and the split-bf16 row-block kernels.
#pragma once
#include "lgcn_common.hpp"

namespace lgcn {

// Row phase: thread (row = t >> 3, sub = t & 7) of the 256 compute threads
// owns columns 4*sub + 32*j + {0..3}, j = 0..3 of its row (8 threads write
// 128 contiguous bytes per j when the row goes to global memory).
struct RowVals { float4 v[4]; };

__device__ __forceinline__ RowVals row_load(const float *T, int t) {
    RowVals r;
    const float *p = T + (t >> 3) * kLDA + 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = *reinterpret_cast<const float4 *>(p + 32 * j);
    return r;
}

__device__ __forceinline__ void row_store_lds(float *T, int t, const RowVals &r) {
    float *p = T + (t >> 3) * kLDA + 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4 *>(p + 32 * j) = r.v[j];
}

// Cross-lane move by a DPP control word (VALU speed; __shfl_xor compiles to ds_bpermute_b32, an LDS round
// trip per step).
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}

// Sum over the 8 consecutive lanes that share a row; every lane gets the same bits as the xor-1/2/4 butterfly:
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], then row_half_mirror (lane i <- lane 7 - i of its group of 8,
// which sits in the other quad and holds that quad's sum).
__device__ __forceinline__ float sum8(float x) {
    x += dpp_mov<0xB1>(x);
    x += dpp_mov<0x4E>(x);
    x += dpp_mov<0x141>(x);
    return x;
}

// 1 / sqrt(var + eps) of a row whose fp32 sum of squares overflowed (centred values beyond ~2^60: var = inf, rstd = 0,
// and the row would come out as beta): the same sum over the centred values scaled by 2^-68 (exact), rstd scaled back.
// Rare path behind one compare; a row that holds a NaN or an inf takes it too and comes out NaN as before.  The eight
// lanes of a row share var, so they take the branch together and sum8 finds its partners.
// row_gn compiles it in with WIDE (the default): the f32 kernels and the split kernels of every format with fp32's
// exponent range do -- the three-plane mode (Fmt<0>) and the single bf16 plane (Fmt<2>), whose rows reach a GroupNorm at
// 2^100 as readily as fp32's (the pair kernel of lgcn_pairs.hip restates the same path for its own layout).
// The fp16-plane kernels (Fmt<1>) pass WIDE = false: their GEMM outputs cannot pass 128 * 15 * 65520^2 < 2^50,
// whose squares fit (what else reaches a GroupNorm there -- U + V of the pair stage, the rank-4 meta update -- are such
// outputs or O(1) inputs in this network), and they keep the register budget that lets two workgroups share a CU.
// row_gn_hat, the backward's recomputation, and k_gn_bwd take the same path: with rstd ~ 2^-70 the gradients of such a row
// (dx ~ rstd dy, dW = dT^T x ~ dy) stay inside fp32, and a backward that returned rstd = 0 where the forward did not
// would hand back silent zeros.
// The squares are added one at a time (two live temporaries, not the pairwise tree of row_gn's first pass): the bf16
// LaneConv tile kernel sits at its 128-VGPR limit and takes no more without scratch.
__device__ __forceinline__ float row_rstd_wide(const RowVals &r, float mean, float eps) {
    constexpr float k = 0x1p-68f;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float t = (r.v[j].x - mean) * k; q += t * t;
        t = (r.v[j].y - mean) * k; q += t * t;
        t = (r.v[j].z - mean) * k; q += t * t;
        t = (r.v[j].w - mean) * k; q += t * t;
    }
    return k / sqrtf(sum8(q) * (1.0f / kC) + eps * (k * k));
}

// GroupNorm(1, 128): per-row mean / biased variance over the 128 channels
// (layers.py:73, gcd(1, n_out) = 1 group), two-pass in registers.
template <bool WIDE = true>
__device__ __forceinline__ void row_gn(RowVals &r, int t, const float *__restrict__ g,
                                       const float *__restrict__ b, float eps) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (r.v[j].x + r.v[j].y) + (r.v[j].z + r.v[j].w);
    const float mean = sum8(s) * (1.0f / kC);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = r.v[j].x - mean, bb = r.v[j].y - mean, c = r.v[j].z - mean, d = r.v[j].w - mean;
        q += (a * a + bb * bb) + (c * c + d * d);
    }
    const float var = sum8(q) * (1.0f / kC);
    float rstd = 1.0f / sqrtf(var + eps);
    if constexpr (WIDE)
        if (__builtin_expect(!(var <= 3.4028234e38f), 0)) rstd = row_rstd_wide(r, mean, eps);
    const int c0 = 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 gg = *reinterpret_cast<const float4 *>(g + c0 + 32 * j);
        const float4 bb = *reinterpret_cast<const float4 *>(b + c0 + 32 * j);
        r.v[j].x = (r.v[j].x - mean) * rstd * gg.x + bb.x;
        r.v[j].y = (r.v[j].y - mean) * rstd * gg.y + bb.y;
        r.v[j].z = (r.v[j].z - mean) * rstd * gg.z + bb.z;
        r.v[j].w = (r.v[j].w - mean) * rstd * gg.w + bb.w;
    }
}

// The two halves of row_gn for a backward that recomputes the forward: r becomes xhat = (x - mean) * rstd (returns rstd),
// and row_affine(xhat) = xhat * g + b restates row_gn's output.  Nothing downstream needs the two to agree to the bit (they
// do not: row_gn_hat centres twice): the backward takes its ReLU decisions from the stored masks.
__device__ __forceinline__ float row_gn_hat(RowVals &r, float eps) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (r.v[j].x + r.v[j].y) + (r.v[j].z + r.v[j].w);
    const float mean = sum8(s) * (1.0f / kC);
    // The fp32 mean of a row that sits far from zero is off by up to half an ulp of the mean (6e-5 at 2^10) however it is
    // summed, and that goes straight into xhat and from there into dgamma = sum g xhat.  x - mean is exact there (Sterbenz),
    // so the mean of the centred values is what the first mean left behind: take it out too (a corrected two-pass).
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r.v[j].x -= mean; r.v[j].y -= mean; r.v[j].z -= mean; r.v[j].w -= mean;
        e += (r.v[j].x + r.v[j].y) + (r.v[j].z + r.v[j].w);
    }
    const float rest = sum8(e) * (1.0f / kC);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r.v[j].x -= rest; r.v[j].y -= rest; r.v[j].z -= rest; r.v[j].w -= rest;
        q += (r.v[j].x * r.v[j].x + r.v[j].y * r.v[j].y) + (r.v[j].z * r.v[j].z + r.v[j].w * r.v[j].w);
    }
    const float var = sum8(q) * (1.0f / kC);
    float rstd = 1.0f / sqrtf(var + eps);
    if (__builtin_expect(!(var <= 3.4028234e38f), 0)) rstd = row_rstd_wide(r, 0.f, eps);      // r is centred already
#pragma unroll
    for (int j = 0; j < 4; ++j) { r.v[j].x *= rstd; r.v[j].y *= rstd; r.v[j].z *= rstd; r.v[j].w *= rstd; }
    return rstd;
}

__device__ __forceinline__ RowVals row_affine(const RowVals &xh, int t, const float *__restrict__ g, const float *__restrict__ b) {
    RowVals r;
    const int c0 = 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 gg = *reinterpret_cast<const float4 *>(g + c0 + 32 * j);
        const float4 bb = *reinterpret_cast<const float4 *>(b + c0 + 32 * j);
        r.v[j] = make_float4(xh.v[j].x * gg.x + bb.x, xh.v[j].y * gg.y + bb.y, xh.v[j].z * gg.z + bb.z, xh.v[j].w * gg.w + bb.w);
    }
    return r;
}

// GroupNorm backward of one row in registers (the formula of k_gn_bwd): g = dy (already masked) becomes
// dx = rstd * (g gamma - mean(g gamma) - xhat * mean(g gamma xhat)).
__device__ __forceinline__ void row_gn_bwd(RowVals &g, const RowVals &xh, float rstd, int t, const float *__restrict__ gamma) {
    const int c0 = 4 * (t & 7);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 gm = *reinterpret_cast<const float4 *>(gamma + c0 + 32 * j);
        g.v[j] = make_float4(g.v[j].x * gm.x, g.v[j].y * gm.y, g.v[j].z * gm.z, g.v[j].w * gm.w);
        m1 += (g.v[j].x + g.v[j].y) + (g.v[j].z + g.v[j].w);
        m2 += (g.v[j].x * xh.v[j].x + g.v[j].y * xh.v[j].y) + (g.v[j].z * xh.v[j].z + g.v[j].w * xh.v[j].w);
    }
    m1 = sum8(m1) * (1.0f / kC);
    m2 = sum8(m2) * (1.0f / kC);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        g.v[j].x = rstd * (g.v[j].x - m1 - xh.v[j].x * m2); g.v[j].y = rstd * (g.v[j].y - m1 - xh.v[j].y * m2);
        g.v[j].z = rstd * (g.v[j].z - m1 - xh.v[j].z * m2); g.v[j].w = rstd * (g.v[j].w - m1 - xh.v[j].w * m2);
    }
}

__device__ __forceinline__ void row_relu(RowVals &r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r.v[j].x = relu_nan(r.v[j].x); r.v[j].y = relu_nan(r.v[j].y);
        r.v[j].z = relu_nan(r.v[j].z); r.v[j].w = relu_nan(r.v[j].w);
    }
}

__device__ __forceinline__ void row_add_global(RowVals &r, const float *__restrict__ rowp, int t) {
    const float *p = rowp + 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 x = *reinterpret_cast<const float4 *>(p + 32 * j);
        r.v[j].x += x.x; r.v[j].y += x.y; r.v[j].z += x.z; r.v[j].w += x.w;
    }
}

__device__ __forceinline__ void row_add(RowVals &r, const RowVals &x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r.v[j].x += x.v[j].x; r.v[j].y += x.v[j].y; r.v[j].z += x.v[j].z; r.v[j].w += x.v[j].w;
    }
}

__device__ __forceinline__ void row_store_global(float *__restrict__ rowp, int t, const RowVals &r) {
    float *p = rowp + 4 * (t & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4 *>(p + 32 * j) = r.v[j];
}

__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }


struct InputParams {
    const float *ctrs, *feats;
    int64_t n_rows;
    const float *wa1, *ba1, *wpa2, *ga, *bta;
    const float *ws1, *bs1, *wps2, *gs, *bts;
    float eps;
    float *out;
};

struct PairParams {
    const float *agt_ctrs, *ctx_ctrs;
    const int32_t *hi, *wi, *n_pairs;
    int64_t cap;
    const float *wd0, *bd0, *wpd2, *gd, *btd;
    const float *wpc0e, *U, *V, *gc, *btc;
    float eps;
    float *m;
};

// split-bf16 implementations (lgcn_rowmlp_bf.hip)
int agg_mlp_bf(const lgcn_agg_mlp_t &p, bool lane_conv, hipStream_t st);
int agg_mlp_pair_bf(const lgcn_agg_mlp_t &a, const lgcn_agg_mlp_t &b, hipStream_t st);
int agg_mlp_multi_bf(const lgcn_agg_mlp_t *const *ps, int n, hipStream_t st);
int mapnet_input_bf(const InputParams &p, int mma, hipStream_t st);
int pack_weight_bf(const float *W, int ld, int mma, int transpose, void *out, hipStream_t st);
int pack_weight_batch_bf(const lgcn_pack_job_t *jobs, int n_jobs, int mma, hipStream_t st);

}  // namespace lgcn
