// PredNet's tail (reference lanegcn.py:575-631 PredNet.forward, 713-737 AttDest, 147-150 the world-frame transform) in
// two launches around the row-block kernels that already run its LinearRes / Linear + GroupNorm stages:
//
//   lgcn_pred_reg    reg[a, m, t, :] = W_m h_m[a] + b_m + ctr[a]          (the M heads' nn.Linear(128, 2 T), :601-612)
//                    hd[a M + m, :]  = relu(Wd (ctr[a] - reg[a, m, T - 1, :]) + bd)     (AttDest.dist[0..1], :725-729)
//   lgcn_pred_final  cls[a, :] = sort_desc(wc . f[a M + m, :] + bc),  reg_out[a, j] = reg[a, order_j] rot[a] + orig[a]
//                    (the score nn.Linear(128, 1), the sort and the gather of :614-625, matmul + orig of Net.forward)
//
// and their backward for training (PredNet.train_hip), at most four launches:
//
//   lgcn_pred_final_bwd  the scatter back through the saved order, d f = g_s wc, per-workgroup partials of d wc / d bc
//                        + one fixed-order reduction launch
//   lgcn_pred_reg_bwd    d h_m = g_reg W_m, per-chunk partials of d W_m = g_reg^T h_m, d b_m, d wd, d bd
//                        + one fixed-order reduction launch
//
// Plain fp32 FMAs (74 MFLOP for 1,600 actors): the work is launch latency, not arithmetic -- these two launches stand
// for 6 GEMM calls, a stack, an add, a slice, a subtraction, two more GEMMs, a ReLU, a sort, an arange, an indexed gather,
// an einsum and an add of the stock path.
#include "lgcn_common.hpp"

namespace lgcn {

constexpr int kPredMaxMod = 8;
constexpr int kPredActors = 32;        // actors per workgroup of k_pred_reg
constexpr int kPredLd = 132;           // LDS row stride of the actors' feature rows (floats): 16 lanes' float4 reads spread over the banks

struct PredRegParams {
    const float *h[kPredMaxMod];       // [A, 128] per mode: the heads' LinearRes outputs
    const float *w[kPredMaxMod];       // [np2, 128] per mode
    const float *b[kPredMaxMod];       // [np2] per mode
    const float *ctrs;                 // [A, 2]
    const float *wd, *bd;              // [128, 2], [128]: AttDest.dist[0]
    float *reg;                        // [A, M, np2]
    float *hd;                         // [A * M, 128]
    int n_act, n_mod, np2;
};

__global__ __launch_bounds__(256) void k_pred_reg(const PredRegParams p) {
    __shared__ __attribute__((aligned(16))) float sW[64 * 128];
    __shared__ __attribute__((aligned(16))) float sH[kPredActors * kPredLd];
    __shared__ float sD[kPredActors][2];
    const int tid = threadIdx.x, m = blockIdx.y, a0 = blockIdx.x * kPredActors;
    const float *wm = p.w[m], *hm = p.h[m];
    for (int i = tid; i < 64 * 32; i += 256) {                  // float4 index: row i >> 5, columns 4 (i & 31)
        const int o = i >> 5;
        reinterpret_cast<float4 *>(sW)[i] = o < p.np2 ? reinterpret_cast<const float4 *>(wm)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = tid; i < kPredActors * 32; i += 256) {
        const int r = i >> 5, c4 = i & 31;
        const int a = a0 + r;
        *reinterpret_cast<float4 *>(sH + r * kPredLd + 4 * c4) =
            a < p.n_act ? reinterpret_cast<const float4 *>(hm + (int64_t)a * 128)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int al = tid & 31, og = tid >> 5;                    // actor of the block, group of 8 outputs
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const float *hr = sH + al * kPredLd;
    for (int k = 0; k < 128; k += 4) {
        const float4 x = *reinterpret_cast<const float4 *>(hr + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 w = *reinterpret_cast<const float4 *>(sW + (og * 8 + j) * 128 + k);   // one address per half-wave
            acc[j] = fmaf(x.x, w.x, acc[j]);
            acc[j] = fmaf(x.y, w.y, acc[j]);
            acc[j] = fmaf(x.z, w.z, acc[j]);
            acc[j] = fmaf(x.w, w.w, acc[j]);
        }
    }
    const int a = a0 + al;
    float cx = 0.f, cy = 0.f;
    if (a < p.n_act) { cx = p.ctrs[2 * (int64_t)a]; cy = p.ctrs[2 * (int64_t)a + 1]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int o = og * 8 + j;
        if (o < p.np2) {
            const float v = (acc[j] + p.b[m][o]) + ((o & 1) ? cy : cx);
            if (a < p.n_act) p.reg[((int64_t)a * p.n_mod + m) * p.np2 + o] = v;
            if (o >= p.np2 - 2) sD[al][o & 1] = ((o & 1) ? cy : cx) - v;          // agt_ctr - dest
        }
    }
    __syncthreads();
    for (int i = tid; i < kPredActors * 32; i += 256) {
        const int r = i >> 5, c = 4 * (i & 31);
        const int ar = a0 + r;
        if (ar >= p.n_act) continue;
        const float dx = sD[r][0], dy = sD[r][1];
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float2 w = *reinterpret_cast<const float2 *>(p.wd + 2 * (c + q));
            o[q] = relu_nan(fmaf(dy, w.y, dx * w.x) + p.bd[c + q]);      // ATen's relu keeps a NaN
        }
        *reinterpret_cast<float4 *>(p.hd + ((int64_t)ar * p.n_mod + m) * 128 + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

struct PredFinalParams {
    const float *f;                    // [A * M, 128]: the score head's LinearRes output
    const float *wc, *bc;              // [128], [1]
    const float *reg;                  // [A, M, np, 2]
    const float *rot, *orig;           // [A, 2, 2], [A, 2] or null: no transform
    float *cls;                        // [A, M] descending
    float *out;                        // [A, M, np, 2] in the order of cls
    int *order;                        // [A, M] or null: the mode that took rank j (training: the backward's scatter index)
    int n_act, n_mod, np;
};

__global__ __launch_bounds__(256) void k_pred_final(const PredFinalParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = blockIdx.x * 4 + wave;                        // one wave per actor
    if (a >= p.n_act) return;
    const float w0 = p.wc[lane], w1 = p.wc[64 + lane], bc = p.bc[0];
    float c[kPredMaxMod];
#pragma unroll
    for (int m = 0; m < kPredMaxMod; ++m) {
        c[m] = 0.f;
        if (m < p.n_mod) {
            const float *fr = p.f + ((int64_t)a * p.n_mod + m) * 128;
            float s = fmaf(fr[64 + lane], w1, fr[lane] * w0);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
            c[m] = s + bc;
        }
    }
    // descending order, equal scores in mode order, NaN scores first (torch.sort treats NaN as the largest value): a
    // total order, so every rank 0 .. n_mod - 1 is taken exactly once and every slot of cls / out is written
    int order[kPredMaxMod];
#pragma unroll
    for (int m = 0; m < kPredMaxMod; ++m) order[m] = 0;
#pragma unroll
    for (int m = 0; m < kPredMaxMod; ++m) {
        if (m < p.n_mod) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < kPredMaxMod; ++j)
                if (j < p.n_mod) {
                    const bool nj = c[j] != c[j], nm = c[m] != c[m];
                    const bool before = (nj || nm) ? (nj && (!nm || j < m)) : (c[j] > c[m] || (c[j] == c[m] && j < m));
                    if (before) ++rank;
                }
#pragma unroll
            for (int r = 0; r < kPredMaxMod; ++r)
                if (r == rank) order[r] = m;
            if (lane == 0) {
                p.cls[(int64_t)a * p.n_mod + rank] = c[m];
                if (p.order != nullptr) p.order[(int64_t)a * p.n_mod + rank] = m;
            }
        }
    }
    float r00 = 1.f, r01 = 0.f, r10 = 0.f, r11 = 1.f, ox = 0.f, oy = 0.f;
    const bool xf = p.rot != nullptr;
    if (xf) {
        const float4 r = *reinterpret_cast<const float4 *>(p.rot + 4 * (int64_t)a);
        r00 = r.x; r01 = r.y; r10 = r.z; r11 = r.w;
        ox = p.orig[2 * (int64_t)a]; oy = p.orig[2 * (int64_t)a + 1];
    }
    const int total = p.n_mod * p.np;
    for (int i = lane; i < total; i += 64) {
        const int mo = i / p.np, t = i - mo * p.np;
        int src = 0;
#pragma unroll
        for (int r = 0; r < kPredMaxMod; ++r)
            if (r == mo) src = order[r];
        const float2 v = *reinterpret_cast<const float2 *>(p.reg + (((int64_t)a * p.n_mod + src) * p.np + t) * 2);
        float2 o = v;
        if (xf) {
            o.x = fmaf(v.y, r10, v.x * r00) + ox;               // reg @ rot + orig
            o.y = fmaf(v.y, r11, v.x * r01) + oy;
        }
        *reinterpret_cast<float2 *>(p.out + (((int64_t)a * p.n_mod + mo) * p.np + t) * 2) = o;
    }
}


// ---------------------------------------------------------------- backward (training)
constexpr int kFinalBwdRec = 132;      // floats of one partial record of k_pred_final_bwd: d wc [128], d bc, 3 of padding

struct PredFinalBwdParams {
    const float *g_cls;                // [A, M] or null (taken as zeros)
    const float *g_out;                // [A, M, np2] or null (taken as zeros)
    const int *order;                  // [A, M]: the forward's order
    const float *f, *wc;               // [A * M, 128], [128]
    float *g_reg;                      // [A, M, np2] or null: not computed
    float *d_f;                        // [A * M, 128] or null: not computed
    float *part;                       // [gridDim.x, kFinalBwdRec]
    int n_act, n_mod, np2, per_wave;   // per_wave: actors a wave takes one after the other
};

// One wave per actor, per_wave actors per wave.  The scatter through the order is written as a gather through its inverse:
// every element of g_reg is written exactly once whatever `order` holds.  Lane l owns channels 2 l, 2 l + 1.
__global__ __launch_bounds__(256) void k_pred_final_bwd(const PredFinalBwdParams p) {
    __shared__ float sP[4][kFinalBwdRec];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float2 w = reinterpret_cast<const float2 *>(p.wc)[lane];
    float ax = 0.f, ay = 0.f, ab = 0.f;
    const int half = p.np2 >> 1, total = p.n_mod * half;
    for (int i = 0; i < p.per_wave; ++i) {
        const int a = (blockIdx.x * p.per_wave + i) * 4 + wave;          // wave-uniform
        if (a >= p.n_act) break;
        int inv[kPredMaxMod];
        float gs[kPredMaxMod];
#pragma unroll
        for (int m = 0; m < kPredMaxMod; ++m) { inv[m] = 0; gs[m] = 0.f; }
#pragma unroll
        for (int j = 0; j < kPredMaxMod; ++j)
            if (j < p.n_mod) {
                const int o = p.order[(int64_t)a * p.n_mod + j];
                const float g = p.g_cls != nullptr ? p.g_cls[(int64_t)a * p.n_mod + j] : 0.f;
#pragma unroll
                for (int m = 0; m < kPredMaxMod; ++m)
                    if (o == m) { inv[m] = j; gs[m] = g; }
            }
#pragma unroll
        for (int m = 0; m < kPredMaxMod; ++m)
            if (m < p.n_mod) {
                const int64_t row = (int64_t)a * p.n_mod + m;
                const float2 fv = reinterpret_cast<const float2 *>(p.f + row * 128)[lane];
                if (p.d_f != nullptr) reinterpret_cast<float2 *>(p.d_f + row * 128)[lane] = make_float2(gs[m] * w.x, gs[m] * w.y);
                ax = fmaf(gs[m], fv.x, ax);
                ay = fmaf(gs[m], fv.y, ay);
                ab += gs[m];
            }
        if (p.g_reg != nullptr)
            for (int k = lane; k < total; k += 64) {
                const int m = k / half, t = k - m * half;
                int src = 0;
#pragma unroll
                for (int r = 0; r < kPredMaxMod; ++r)
                    if (r == m) src = inv[r];
                float2 v = make_float2(0.f, 0.f);
                if (p.g_out != nullptr) v = reinterpret_cast<const float2 *>(p.g_out)[((int64_t)a * p.n_mod + src) * half + t];
                reinterpret_cast<float2 *>(p.g_reg)[((int64_t)a * p.n_mod + m) * half + t] = v;
            }
    }
    sP[wave][2 * lane] = ax;
    sP[wave][2 * lane + 1] = ay;
    if (lane == 0) sP[wave][128] = ab;
    __syncthreads();
    if (threadIdx.x < 129)
        p.part[(int64_t)blockIdx.x * kFinalBwdRec + threadIdx.x] =
            ((sP[0][threadIdx.x] + sP[1][threadIdx.x]) + sP[2][threadIdx.x]) + sP[3][threadIdx.x];
}

// d wc [128], d bc [1] = the records of k_pred_final_bwd summed in record order
__global__ __launch_bounds__(256) void k_pred_final_reduce(const float *part, int n_part, float *d_wc, float *d_bc) {
    const int k = threadIdx.x;
    if (k >= 129) return;
    float s = 0.f;
    for (int i = 0; i < n_part; ++i) s += part[(int64_t)i * kFinalBwdRec + k];
    if (k < 128) d_wc[k] = s;
    else d_bc[0] = s;
}

constexpr int kRegBwdGLd = 68;         // LDS row stride of the g_reg tile (floats): float4 reads of 16 rows spread over the banks
constexpr int kRegBwdTail = 64 + 384;  // floats behind the d W block of a partial record: d b (64 slots), d wd [128, 2], d bd [128]

struct PredRegBwdParams {
    const float *h[kPredMaxMod];       // [A, 128] per mode
    const float *w[kPredMaxMod];       // [np2, 128] per mode
    float *dh[kPredMaxMod];            // [A, 128] per mode or null: not computed
    const float *g_reg;                // [A, M, np2]
    const float *g_hd;                 // [A * M, 128] or null (taken as zeros)
    const float *hd, *reg, *ctrs;      // the forward's outputs and centres
    float *part;                       // [n_chunks, M, np2 * 128 + kRegBwdTail]
    int n_act, n_mod, np2, chunk_tiles, want_w, want_d;
};

// Workgroup (chunk, mode): chunk_tiles tiles of kPredActors actors one after the other.  Per tile g_reg's [32, np2] block, the
// actors' feature rows and (once) the head's weight sit in LDS; d h leaves per tile, the sums over actors stay in registers
// until the chunk's record is written.
__global__ __launch_bounds__(256) void k_pred_reg_bwd(const PredRegBwdParams p) {
    __shared__ __attribute__((aligned(16))) float sW[64 * 128];
    __shared__ __attribute__((aligned(16))) float sH[kPredActors * kPredLd];
    __shared__ __attribute__((aligned(16))) float sG[kPredActors * kRegBwdGLd];
    __shared__ float sD[kPredActors][2];
    __shared__ float sR[2][384];
    const int tid = threadIdx.x, m = blockIdx.y;
    const float *wm = p.w[m], *hm = p.h[m];
    float *dhm = p.dh[m];
    if (dhm != nullptr)
        for (int i = tid; i < 64 * 32; i += 256) {
            const int o = i >> 5;
            reinterpret_cast<float4 *>(sW)[i] = o < p.np2 ? reinterpret_cast<const float4 *>(wm)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    const int cl = tid & 31, grp = tid >> 5;                    // 4 channels; group of 4 actors (d h) or of 8 outputs (d W)
    float accw[8][4];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) accw[j][q] = 0.f;
    float accb = 0.f, pw0 = 0.f, pw1 = 0.f, pb = 0.f;
    for (int t = 0; t < p.chunk_tiles; ++t) {
        const int a0 = (blockIdx.x * p.chunk_tiles + t) * kPredActors;
        if (a0 >= p.n_act) break;                               // uniform over the workgroup
        __syncthreads();                                        // the previous tile's readers are done
        for (int i = tid; i < kPredActors * 64; i += 256) {
            const int r = i >> 6, o = i & 63;
            const int a = a0 + r;
            sG[r * kRegBwdGLd + o] = (a < p.n_act && o < p.np2) ? p.g_reg[((int64_t)a * p.n_mod + m) * p.np2 + o] : 0.f;
        }
        if (p.want_w)
            for (int i = tid; i < kPredActors * 32; i += 256) {
                const int r = i >> 5, c4 = i & 31;
                const int a = a0 + r;
                *reinterpret_cast<float4 *>(sH + r * kPredLd + 4 * c4) =
                    a < p.n_act ? reinterpret_cast<const float4 *>(hm + (int64_t)a * 128)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        if (p.want_d && tid < 2 * kPredActors) {
            const int r = tid >> 1, k = tid & 1;
            const int a = a0 + r;
            sD[r][k] = a < p.n_act ? p.ctrs[2 * (int64_t)a + k] - p.reg[((int64_t)a * p.n_mod + m) * p.np2 + p.np2 - 2 + k] : 0.f;
        }
        __syncthreads();
        if (dhm != nullptr) {                                   // d h[a, :] = sum_o g[a, o] W[o, :]
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
            for (int o = 0; o < p.np2; o += 4) {                // rows of sW / columns of sG beyond np2 are zero
                float4 g[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) g[i] = *reinterpret_cast<const float4 *>(sG + (grp * 4 + i) * kRegBwdGLd + o);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 wv = *reinterpret_cast<const float4 *>(sW + (o + k) * 128 + 4 * cl);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float gv = k == 0 ? g[i].x : k == 1 ? g[i].y : k == 2 ? g[i].z : g[i].w;
                        acc[i][0] = fmaf(gv, wv.x, acc[i][0]);
                        acc[i][1] = fmaf(gv, wv.y, acc[i][1]);
                        acc[i][2] = fmaf(gv, wv.z, acc[i][2]);
                        acc[i][3] = fmaf(gv, wv.w, acc[i][3]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int a = a0 + grp * 4 + i;
                if (a < p.n_act)
                    *reinterpret_cast<float4 *>(dhm + (int64_t)a * 128 + 4 * cl) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
            }
        }
        if (p.want_w) {                                         // d W[o, :] += sum_a g[a, o] h[a, :],  d b[o] += sum_a g[a, o]
            for (int r = 0; r < kPredActors; ++r) {             // rows beyond n_act are zero
                const float4 hv = *reinterpret_cast<const float4 *>(sH + r * kPredLd + 4 * cl);
                const float4 g0 = *reinterpret_cast<const float4 *>(sG + r * kRegBwdGLd + grp * 8);
                const float4 g1 = *reinterpret_cast<const float4 *>(sG + r * kRegBwdGLd + grp * 8 + 4);
                const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    accw[j][0] = fmaf(gv[j], hv.x, accw[j][0]);
                    accw[j][1] = fmaf(gv[j], hv.y, accw[j][1]);
                    accw[j][2] = fmaf(gv[j], hv.z, accw[j][2]);
                    accw[j][3] = fmaf(gv[j], hv.w, accw[j][3]);
                }
            }
            if (tid < 64)
                for (int r = 0; r < kPredActors; ++r) accb += sG[r * kRegBwdGLd + tid];
        }
        if (p.want_d) {                                         // p = g_hd (hd > 0); d wd[c, :] += p d, d bd[c] += p
            const int c = tid & 127, r0 = (tid >> 7) * (kPredActors / 2);
            for (int r = r0; r < r0 + kPredActors / 2; ++r) {
                const int a = a0 + r;
                if (a >= p.n_act) break;
                const int64_t e = ((int64_t)a * p.n_mod + m) * 128 + c;
                const float pv = (p.g_hd != nullptr && p.hd[e] > 0.f) ? p.g_hd[e] : 0.f;
                pw0 = fmaf(pv, sD[r][0], pw0);
                pw1 = fmaf(pv, sD[r][1], pw1);
                pb += pv;
            }
        }
    }
    const int rec = p.np2 * 128 + kRegBwdTail;
    float *out = p.part + ((int64_t)blockIdx.x * p.n_mod + m) * rec;
    if (p.want_w) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int o = grp * 8 + j;
            if (o < p.np2)
                *reinterpret_cast<float4 *>(out + o * 128 + 4 * cl) = make_float4(accw[j][0], accw[j][1], accw[j][2], accw[j][3]);
        }
        if (tid < p.np2) out[p.np2 * 128 + tid] = accb;
    }
    if (p.want_d) {
        const int c = tid & 127, hf = tid >> 7;
        sR[hf][2 * c] = pw0;
        sR[hf][2 * c + 1] = pw1;
        sR[hf][256 + c] = pb;
        __syncthreads();
        for (int k = tid; k < 384; k += 256) out[p.np2 * 128 + 64 + k] = sR[0][k] + sR[1][k];
    }
}

struct PredRegReduceParams {
    const float *part;
    float *dw[kPredMaxMod], *db[kPredMaxMod];                   // [np2, 128], [np2] per mode, or null
    float *dwd, *dbd;                                           // [128, 2], [128], or null
    int n_chunks, n_mod, np2;
};

// The chunks' records summed in chunk order (d wd / d bd: chunk-major, then mode).  Grid (record / 256, mode).
__global__ __launch_bounds__(256) void k_pred_reg_reduce(const PredRegReduceParams p) {
    const int k = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    const int nw = p.np2 * 128, rec = nw + kRegBwdTail;
    if (k >= rec) return;
    if (k < nw + 64) {
        float *dst = k < nw ? p.dw[m] : p.db[m];
        const int e = k < nw ? k : k - nw;
        if (dst == nullptr || (k >= nw && e >= p.np2)) return;
        float s = 0.f;
        for (int c = 0; c < p.n_chunks; ++c) s += p.part[((int64_t)c * p.n_mod + m) * rec + k];
        dst[e] = s;
        return;
    }
    if (m != 0) return;
    const int e = k - nw - 64;
    float *dst = e < 256 ? p.dwd : p.dbd;
    if (dst == nullptr) return;
    float s = 0.f;
    for (int c = 0; c < p.n_chunks * p.n_mod; ++c) s += p.part[(int64_t)c * rec + k];
    dst[e < 256 ? e : e - 256] = s;
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int lgcn_pred_reg(const lgcn_pred_reg_t *q, void *stream) {
    LGCN_CHECK_PTR(q);
    if (q->n_act < 0 || q->n_mod < 1 || q->n_mod > kPredMaxMod) return LGCN_EINVAL;
    if (q->np2 < 2 || q->np2 > 64 || (q->np2 & 1)) return LGCN_ESHAPE;
    if (q->n_act > 0x7fffffff / (kPredMaxMod * 128)) return LGCN_ESHAPE;
    PredRegParams p;
    for (int m = 0; m < kPredMaxMod; ++m) {
        p.h[m] = p.w[m] = p.b[m] = nullptr;
        if (m < q->n_mod) {
            LGCN_CHECK_PTR(q->h[m]); LGCN_CHECK_PTR(q->w[m]); LGCN_CHECK_PTR(q->b[m]);
            LGCN_CHECK_ALIGN16(q->h[m]); LGCN_CHECK_ALIGN16(q->w[m]);
            p.h[m] = q->h[m]; p.w[m] = q->w[m]; p.b[m] = q->b[m];
        }
    }
    const void *ptrs[] = {q->ctrs, q->wd, q->bd, q->reg, q->hd};
    for (const void *v : ptrs) LGCN_CHECK_PTR(v);
    LGCN_CHECK_ALIGN16(q->hd);
    if (reinterpret_cast<uintptr_t>(q->wd) & 7u) return LGCN_EALIGN;
    if (q->n_act == 0) return LGCN_OK;
    p.ctrs = q->ctrs; p.wd = q->wd; p.bd = q->bd; p.reg = q->reg; p.hd = q->hd;
    p.n_act = (int)q->n_act; p.n_mod = q->n_mod; p.np2 = q->np2;
    const unsigned gx = (unsigned)((q->n_act + kPredActors - 1) / kPredActors);
    hipLaunchKernelGGL(k_pred_reg, dim3(gx, (unsigned)q->n_mod), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status();
}

static int pred_final_launch(const float *f, const float *wc, const float *bc, const float *reg, const float *rot,
                             const float *orig, int64_t n_act, int n_mod, int n_pred, float *cls, float *out, int32_t *order,
                             void *stream) {
    if (n_act < 0 || n_mod < 1 || n_mod > kPredMaxMod || n_pred < 1) return LGCN_EINVAL;
    if (n_pred > 4096 || n_act > 0x7fffffff / (kPredMaxMod * 128)) return LGCN_ESHAPE;
    const void *ptrs[] = {f, wc, bc, reg, cls, out};
    for (const void *v : ptrs) LGCN_CHECK_PTR(v);
    if ((rot == nullptr) != (orig == nullptr)) return LGCN_EINVAL;
    if (reinterpret_cast<uintptr_t>(reg) & 7u || reinterpret_cast<uintptr_t>(out) & 7u) return LGCN_EALIGN;
    if (rot != nullptr) LGCN_CHECK_ALIGN16(rot);
    if (n_act == 0) return LGCN_OK;
    PredFinalParams p;
    p.f = f; p.wc = wc; p.bc = bc; p.reg = reg; p.rot = rot; p.orig = orig; p.cls = cls; p.out = out; p.order = order;
    p.n_act = (int)n_act; p.n_mod = n_mod; p.np = n_pred;
    hipLaunchKernelGGL(k_pred_final, dim3((unsigned)((n_act + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status();
}

int lgcn_pred_final(const float *f, const float *wc, const float *bc, const float *reg, const float *rot, const float *orig,
                    int64_t n_act, int n_mod, int n_pred, float *cls, float *out, void *stream) {
    return pred_final_launch(f, wc, bc, reg, rot, orig, n_act, n_mod, n_pred, cls, out, nullptr, stream);
}

// n_mod, np2 and the n_act bound of the training entries
static int pred_train_shape(int64_t n_act, int n_mod, int np2) {
    if (n_act < 0 || n_mod < 1 || n_mod > kPredMaxMod) return LGCN_EINVAL;
    if (np2 < 2 || np2 > 64 || (np2 & 1)) return LGCN_ESHAPE;
    if (n_act > 0x7fffffff / (kPredMaxMod * 128)) return LGCN_ESHAPE;
    return LGCN_OK;
}

int lgcn_pred_final_train(const float *f, const float *wc, const float *bc, const float *reg, int64_t n_act, int n_mod,
                          int np2, float *cls, float *out, int32_t *order, void *stream) {
    const int rc = pred_train_shape(n_act, n_mod, np2);
    if (rc != LGCN_OK) return rc;
    LGCN_CHECK_PTR(order);
    return pred_final_launch(f, wc, bc, reg, nullptr, nullptr, n_act, n_mod, np2 / 2, cls, out, order, stream);
}

// actors per wave of k_pred_final_bwd: 4, more beyond 4,096 actors so that there are never more than 256 records
static int final_bwd_per_wave(int64_t n_act) {
    const int64_t need = (n_act + 1023) / 1024;
    return (int)(need > 4 ? need : 4);
}

int64_t lgcn_pred_final_bwd_ws_elems(int64_t n_act) {
    if (n_act < 0 || n_act > 0x7fffffff / (kPredMaxMod * 128)) return -1;
    const int per_wg = 4 * final_bwd_per_wave(n_act);
    return (n_act + per_wg - 1) / per_wg * kFinalBwdRec;
}

int lgcn_pred_final_bwd(const float *g_cls, const float *g_out, const int32_t *order, const float *f, const float *wc,
                        int64_t n_act, int n_mod, int np2, float *g_reg, float *d_f, float *d_wc, float *d_bc, float *part,
                        void *stream) {
    const int rc = pred_train_shape(n_act, n_mod, np2);
    if (rc != LGCN_OK) return rc;
    const void *ptrs[] = {order, f, wc, d_wc, d_bc, part};
    for (const void *v : ptrs) LGCN_CHECK_PTR(v);
    const void *al8[] = {g_out, f, wc, g_reg, d_f};             // read / written as float2 (null: absent)
    for (const void *v : al8)
        if (reinterpret_cast<uintptr_t>(v) & 7u) return LGCN_EALIGN;
    if (n_act == 0) return LGCN_OK;
    PredFinalBwdParams p;
    p.g_cls = g_cls; p.g_out = g_out; p.order = order; p.f = f; p.wc = wc; p.g_reg = g_reg; p.d_f = d_f; p.part = part;
    p.n_act = (int)n_act; p.n_mod = n_mod; p.np2 = np2; p.per_wave = final_bwd_per_wave(n_act);
    const int per_wg = 4 * p.per_wave;
    const unsigned n_wg = (unsigned)((n_act + per_wg - 1) / per_wg);
    hipLaunchKernelGGL(k_pred_final_bwd, dim3(n_wg), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(k_pred_final_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float *)part, (int)n_wg, d_wc, d_bc);
    return launch_status();
}

// tiles of kPredActors actors per workgroup of k_pred_reg_bwd: 2, more beyond 4,096 actors (never more than 64 chunks)
static int reg_bwd_chunk_tiles(int64_t n_act) {
    const int64_t n_tiles = (n_act + kPredActors - 1) / kPredActors;
    const int64_t need = (n_tiles + 63) / 64;
    return (int)(need > 2 ? need : 2);
}

static int64_t reg_bwd_chunks(int64_t n_act) {
    const int64_t per = (int64_t)reg_bwd_chunk_tiles(n_act) * kPredActors;
    return (n_act + per - 1) / per;
}

int64_t lgcn_pred_reg_bwd_ws_elems(int64_t n_act, int n_mod, int np2) {
    if (pred_train_shape(n_act, n_mod, np2) != LGCN_OK) return -1;
    return reg_bwd_chunks(n_act) * n_mod * (np2 * 128 + kRegBwdTail);
}

int lgcn_pred_reg_bwd(const lgcn_pred_reg_bwd_t *q, void *stream) {
    LGCN_CHECK_PTR(q);
    const int rc = pred_train_shape(q->n_act, q->n_mod, q->np2);
    if (rc != LGCN_OK) return rc;
    PredRegBwdParams p;
    PredRegReduceParams r;
    bool want_w = false;
    for (int m = 0; m < kPredMaxMod; ++m) {
        p.h[m] = p.w[m] = nullptr;
        p.dh[m] = r.dw[m] = r.db[m] = nullptr;
        if (m < q->n_mod) {
            LGCN_CHECK_PTR(q->h[m]); LGCN_CHECK_PTR(q->w[m]);
            LGCN_CHECK_ALIGN16(q->h[m]); LGCN_CHECK_ALIGN16(q->w[m]); LGCN_CHECK_ALIGN16(q->d_h[m]);
            p.h[m] = q->h[m]; p.w[m] = q->w[m]; p.dh[m] = q->d_h[m];
            r.dw[m] = q->d_w[m]; r.db[m] = q->d_b[m];
            want_w = want_w || q->d_w[m] != nullptr || q->d_b[m] != nullptr;
        }
    }
    const void *ptrs[] = {q->g_reg, q->hd, q->reg, q->ctrs, q->part};
    for (const void *v : ptrs) LGCN_CHECK_PTR(v);
    LGCN_CHECK_ALIGN16(q->part);
    if (q->n_act == 0) return LGCN_OK;
    p.g_reg = q->g_reg; p.g_hd = q->g_hd; p.hd = q->hd; p.reg = q->reg; p.ctrs = q->ctrs; p.part = q->part;
    p.n_act = (int)q->n_act; p.n_mod = q->n_mod; p.np2 = q->np2; p.chunk_tiles = reg_bwd_chunk_tiles(q->n_act);
    p.want_w = want_w; p.want_d = q->d_wd != nullptr || q->d_bd != nullptr;
    const unsigned n_chunks = (unsigned)reg_bwd_chunks(q->n_act);
    hipLaunchKernelGGL(k_pred_reg_bwd, dim3(n_chunks, (unsigned)q->n_mod), dim3(256), 0, (hipStream_t)stream, p);
    if (p.want_w || p.want_d) {
        r.part = q->part; r.dwd = q->d_wd; r.dbd = q->d_bd; r.n_chunks = (int)n_chunks; r.n_mod = q->n_mod; r.np2 = q->np2;
        const unsigned gx = (unsigned)((q->np2 * 128 + kRegBwdTail + 255) / 256);
        hipLaunchKernelGGL(k_pred_reg_reduce, dim3(gx, (unsigned)q->n_mod), dim3(256), 0, (hipStream_t)stream, r);
    }
    return launch_status();
}

}  // extern "C"
