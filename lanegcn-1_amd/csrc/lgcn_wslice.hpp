// Weight-stationary 48-row tiles shared by lgcn_nodetail.hip and lgcn_nodehead.hip: each of a workgroup's 8 waves owns
// the 16-channel slice `wave` of a 128 x 128 weight over the full K (NP x 4 fragments: 32 VGPRs in f16x2), the A operand
// planes live in LDS, and the accumulators go to the fp32 LDS tile for a row phase or straight to global memory.
#pragma once
#include "lgcn_common.hpp"
#include "lgcn_mma_bf.hpp"

namespace lgcn {

constexpr int kNtRB = 3;            // 48-row tiles

// One weight's slice of a wave: K-step s -> the fragment of channels [16 wave, 16 wave + 16) (packed image of
// lgcn_pack_weight: channel quarter wave >> 1, 16-column block wave & 1).
template <int F>
struct WSlice { BFrag<F, 1> s[4]; };

template <int F>
__device__ __forceinline__ void load_slice(WSlice<F> &w, const float *__restrict__ wp, int wave, int lane) {
    const uint4 *__restrict__ Bw = reinterpret_cast<const uint4 *>(wp);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int p = 0; p < Fmt<F>::NP; ++p)
            w.s[s].v[p][0] = Bw[((((p * 4 + (wave >> 1)) * 4 + s) * 2 + (wave & 1)) << 6) + lane];
}

template <int F>
__device__ __forceinline__ void gemm_slice(const uint16_t *__restrict__ A, const WSlice<F> &w, int lane, f32x4 (&acc)[kNtRB][1]) {
    const uint16_t *arow = A + (lane & 15) * kLDB + 8 * (lane >> 4);
#pragma unroll
    for (int s = 0; s < 4; ++s) kstep<kNtRB, F>(arow, s, w.s[s], acc);
}

// C/D layout of 16x16: col = lane & 15, row = 4 (lane >> 4) + reg
__device__ __forceinline__ void acc_to_tile(float *T, const f32x4 (&acc)[kNtRB][1], int lane, int wave) {
#pragma unroll
    for (int rb = 0; rb < kNtRB; ++rb) {
        float *p = T + (16 * rb + 4 * (lane >> 4)) * kLDA + 16 * wave + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i * kLDA] = acc[rb][0][i];
    }
}

// A GEMM's output rows straight from the accumulators (64-byte row segments); rows past the end are masked
__device__ __forceinline__ void acc_to_global(float *__restrict__ out, const f32x4 (&acc)[kNtRB][1], int64_t row0, int64_t n_rows,
                                              int lane, int wave) {
#pragma unroll
    for (int rb = 0; rb < kNtRB; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t n = row0 + 16 * rb + 4 * (lane >> 4) + i;
            if (n < n_rows) out[n * kC + 16 * wave + (lane & 15)] = acc[rb][0][i];
        }
}

}  // namespace lgcn
