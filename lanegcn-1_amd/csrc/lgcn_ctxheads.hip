// Context heads of an Att block (lgcn_ctx_heads): out[j] = x W_j^T for one or two 128 x 128 weights over the same rows
// (V = ctx W_c0[:, 256:384]^T of both Att layers of M2A, lanegcn.py:696-699), weight-stationary.
//
// The generic row block (lgcn_rowmlp_bf.hip) runs such a GEMM as one problem per weight: every 32-row tile reads its
// rows once per weight and streams the whole weight image L2 -> VGPR through a two-deep fragment ring (four dependent
// round trips), with the gather waves and the MFMA waves taking turns.  Here a workgroup reads a 48-row tile ONCE, and
// wave (j, cq) of its 8 waves holds the 32-channel slice cq of W_j over the full K in registers (NP x 4 x 2 fragments,
// 64 VGPRs in f16x2), all of it requested at kernel start: one round trip, one barrier, then rows x 4 K-steps x NPROD
// MFMAs per wave from LDS A fragments, stored straight from the accumulators (64-byte row segments).
//
// Arithmetic: exactly the row block's with one LGCN_REL_IDENT relation and flags = 0 -- the rows are the A operand, the
// weights the B operand, one fp32 accumulator per output element that starts at 0 and takes K-steps 0..3 in order and,
// within a K-step, the plane products in Fmt<F>::PA / PB order (kstep of lgcn_mma_bf.hpp, shared) -- so the two agree
// bit for bit.
#include "lgcn_common.hpp"
#include "lgcn_mma_bf.hpp"

namespace lgcn {

constexpr int kChRB = 3;            // 48-row tiles: 216 workgroups over the 10,368 lane nodes of S2, one per CU

struct CtxHeadsParams {
    const float *x;
    int64_t n_rows;
    const uint4 *w[2];
    float *out[2];
    int n_w;
};

// <= 128 VGPRs: a second workgroup, or another forward's kernel, shares the CU.
template <int F>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_ctx_heads(const CtxHeadsParams p, int n_tiles) {
    using TL = Tile<kChRB, F>;
    constexpr int ROWS = TL::ROWS;
    __shared__ __attribute__((aligned(16))) uint16_t A[TL::ABUF_BYTES / 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = wave >> 2, cq = wave & 3;          // weight, channel quarter [32 cq, 32 cq + 32)
    const int tile = xcd_chunk_remap(blockIdx.x, n_tiles);
    const int64_t row0 = (int64_t)tile * ROWS;
    const bool mine = j < p.n_w;                     // wave-uniform; with one weight waves 4..7 only load rows

    // the tile's rows, once: thread -> (row = 16 it + tid / 32, 4 channels), row index clamped for the last tile
    const int hr = tid >> 5, l = tid & 31;
    float4 v[kChRB];
#pragma unroll
    for (int it = 0; it < kChRB; ++it) {
        int64_t n = row0 + 16 * it + hr;
        n = n < p.n_rows ? n : p.n_rows - 1;
        v[it] = reinterpret_cast<const float4 *>(p.x)[n * (kC / 4) + l];
    }
    // the wave's whole weight slice, requested behind the rows: it lands while they are split
    BFrag<F> b[4];
    if (mine) {
#pragma unroll
        for (int s = 0; s < 4; ++s) load_b<F>(b[s], p.w[j], cq, lane, s);
    }
#pragma unroll
    for (int it = 0; it < kChRB; ++it) split_store<F>(A, TL::PLANE, 16 * it + hr, 4 * l, v[it]);
    lds_barrier();
    if (!mine) return;

    f32x4 acc[kChRB][2];
    acc_zero<kChRB>(acc);
    const uint16_t *arow = A + (lane & 15) * kLDB + 8 * (lane >> 4);
#pragma unroll
    for (int s = 0; s < 4; ++s) kstep<kChRB, F>(arow, s, b[s], acc);

    // C/D layout of 16x16: col = lane & 15, row = 4 (lane >> 4) + reg; rows past the end are masked
    float *__restrict__ out = p.out[j];
#pragma unroll
    for (int rb = 0; rb < kChRB; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t n = row0 + 16 * rb + 4 * (lane >> 4) + i;
                if (n < p.n_rows) out[n * kC + 32 * cq + 16 * cb + (lane & 15)] = acc[rb][cb][i];
            }
}

}  // namespace lgcn

extern "C" int lgcn_ctx_heads(const float *x, int64_t n_rows, const void *const *w, int n_w, int mma, float *const *out,
                              void *stream) {
    using namespace lgcn;
    if (mma != LGCN_MMA_F16X2 && mma != LGCN_MMA_BF16) return LGCN_ESHAPE;
    if (n_rows < 0 || n_w < 1 || n_w > 2) return LGCN_EINVAL;
    if (n_rows > 0x7fffffff) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(w);
    LGCN_CHECK_PTR(out);
    if (n_rows == 0) return LGCN_OK;
    LGCN_CHECK_PTR(x);
    for (int j = 0; j < n_w; ++j) { LGCN_CHECK_PTR(w[j]); LGCN_CHECK_PTR(out[j]); }
    LGCN_CHECK_ALIGN16(x);
    for (int j = 0; j < n_w; ++j) { LGCN_CHECK_ALIGN16(w[j]); LGCN_CHECK_ALIGN16(out[j]); }
    CtxHeadsParams p{};
    p.x = x;
    p.n_rows = n_rows;
    p.n_w = n_w;
    for (int j = 0; j < n_w; ++j) { p.w[j] = reinterpret_cast<const uint4 *>(w[j]); p.out[j] = out[j]; }
    const int n_tiles = (int)((n_rows + 16 * kChRB - 1) / (16 * kChRB));
    hipStream_t st = (hipStream_t)stream;
    if (mma == LGCN_MMA_F16X2) hipLaunchKernelGGL((k_ctx_heads<1>), dim3(n_tiles), dim3(512), 0, st, p, n_tiles);
    else hipLaunchKernelGGL((k_ctx_heads<2>), dim3(n_tiles), dim3(512), 0, st, p, n_tiles);
    return launch_status();
}
