// Backward of ActorNet's conv unit (lgcn_conv1d_gn; reference layers.py:40-62 Conv1d, 142-190 Res1d; lanegcn.py:212-263):
//
//   y = conv(x; W, stride, pad),   out = act( GN_{(Lout, Cout) of actor a}(y) + residual )
//
// given g = dL/dout and the training forward's y and out (lgcn_conv1d_gn_train).  Three launches, all fp32 (gradients fall
// below fp16's normal range, so no fp16 planes here), no floating-point atomics:
//
//   k_conv_gn_bwd      the 80-row workgroups of the forward (whole actors): ReLU mask from out, dres (the mask itself, or
//                      the adjoint of the x2 linear upsampling), the per-actor GroupNorm backward from y (two-pass
//                      statistics, lgcn_gn_cl_bwd's formulas) -> dy, per-workgroup dgamma / dbeta partials, and
//                      dx = the transposed convolution of dy on v_mfma_f32_16x16x4_f32 (exact fp32; stride 2 as a gather
//                      of the output rows an input row feeds), the dy tile staying in LDS.
//   k_conv_wgrad       dW[co, ci, t] = sum_{a, l} dy[a, l, co] x[a, l stride + t - pad, ci]: workgroup (chunk, t) walks
//                      the actor groups chunk, chunk + n_chunks, ... and keeps a [cout, cin] partial in registers.
//   k_conv_bwd_reduce  the chunk partials and the dgamma / dbeta partials summed in a fixed order.
#include "lgcn_conv.hpp"

namespace lgcn {

struct ConvBwdParams {
    const float *g, *y, *out;          // [A, lout, cout]: upstream gradient, pre-norm conv output, forward output (ReLU mask)
    int64_t n_act;
    int lin, cin, cout, ks, stride, lout;
    const float *wt;                   // lgcn_conv_pack_weight_t image: wt[t][ci][co], ci padded to 16 with zeros
    const float *gamma;
    float eps;
    int res_mode, relu;
    float *dx;                         // [A, lin, cin] or null
    float *dres;                       // [A, lout, cout] (res_mode 1) / [A, lout / 2, cout] (res_mode 2) or null
    float *dy;                         // [A, lout, cout]: gradient of the pre-norm output
    float *part;                       // [n_wg][2][cout]: sum g xhat, sum g over the workgroup's rows
};

// wt[t][ci][co] = W[co][ci][t] for ci < cin, 0 for cin <= ci < cin16
__global__ __launch_bounds__(256) void k_conv_pack_t(const float *__restrict__ w, int cout, int cin, int ks,
                                                     float *__restrict__ out) {
    const int cin16 = (cin + 15) & ~15;
    const int64_t total = (int64_t)ks * cin16 * cout;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int co = (int)(i % cout);
    const int64_t q = i / cout;
    const int ci = (int)(q % cin16), t = (int)(q / cin16);
    out[i] = ci < cin ? w[((int64_t)co * cin + ci) * ks + t] : 0.f;
}

__global__ __launch_bounds__(512) void k_conv_gn_bwd(const ConvBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float s_red[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int na = kConvRows / p.lout;
    const int64_t a0 = (int64_t)blockIdx.x * na;
    const int ldt = p.cout + 4;
    float *T0 = reinterpret_cast<float *>(smem), *T1 = T0 + (kConvRows + 1) * ldt;

    // ---- the forward's GroupNorm mapping and its statistics of y (the same code: conv_gn_stats)
    const ConvGnMap m(p.lout, p.cout, tid);
    const int64_t a = a0 + m.al;
    const bool live = a < p.n_act;
    float4 yv[5], gv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        yv[k] = gv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live && m.has(k)) {
            const int64_t off = (a * p.lout + m.l(k)) * p.cout + m.c;
            yv[k] = *reinterpret_cast<const float4 *>(p.y + off);
            gv[k] = *reinterpret_cast<const float4 *>(p.g + off);
            if (p.relu) {
                const float4 o = *reinterpret_cast<const float4 *>(p.out + off);
                gv[k].x = o.x > 0.f ? gv[k].x : 0.f; gv[k].y = o.y > 0.f ? gv[k].y : 0.f;
                gv[k].z = o.z > 0.f ? gv[k].z : 0.f; gv[k].w = o.w > 0.f ? gv[k].w : 0.f;
            }
            if (p.res_mode == 1 && p.dres) *reinterpret_cast<float4 *>(p.dres + off) = gv[k];
        }
    }
    float mean, rstd;
    conv_gn_stats<true>(yv, m, s_red, p.eps, mean, rstd);      // y may come from the exact units: their wide path too
    // corrected two-pass, as row_gn_hat (lgcn_tile.hpp): the mean of the centred values is what the fp32 mean left behind.
    // s_red[0] is free again: its readers passed the second barrier of conv_gn_stats.
    float rest = 0.f;
    {
        float e = 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (m.has(k)) e += ((yv[k].x - mean) + (yv[k].y - mean)) + ((yv[k].z - mean) + (yv[k].w - mean));
        e = conv_half_sum(e);
        if ((tid & 31) == 0) s_red[0][tid >> 5] = e;
        lds_barrier();
        for (int k = 0; k < m.ng; ++k) rest += s_red[0][m.g0 + k];
        rest = rest / m.per;
    }
    // GroupNorm backward: dy = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat))
    const float4 gm = *reinterpret_cast<const float4 *>(p.gamma + m.c);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        yv[k] = make_float4(((yv[k].x - mean) - rest) * rstd, ((yv[k].y - mean) - rest) * rstd, ((yv[k].z - mean) - rest) * rstd,
                            ((yv[k].w - mean) - rest) * rstd);
        const float4 gg = make_float4(gv[k].x * gm.x, gv[k].y * gm.y, gv[k].z * gm.z, gv[k].w * gm.w);
        s1 += (gg.x + gg.y) + (gg.z + gg.w);
        s2 += (gg.x * yv[k].x + gg.y * yv[k].y) + (gg.z * yv[k].z + gg.w * yv[k].w);
    }
    s1 = conv_half_sum(s1);
    s2 = conv_half_sum(s2);
    if ((tid & 31) == 0) { s_red[2][tid >> 5] = s1; s_red[3][tid >> 5] = s2; }
    lds_barrier();
    float m1 = 0.f, m2 = 0.f;
    for (int k = 0; k < m.ng; ++k) { m1 += s_red[2][m.g0 + k]; m2 += s_red[3][m.g0 + k]; }
    m1 = m1 / m.per;
    m2 = m2 / m.per;
    float4 dv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        dv[k] = make_float4(rstd * (gv[k].x * gm.x - m1 - yv[k].x * m2), rstd * (gv[k].y * gm.y - m1 - yv[k].y * m2),
                            rstd * (gv[k].z * gm.z - m1 - yv[k].z * m2), rstd * (gv[k].w * gm.w - m1 - yv[k].w * m2));
        if (m.has(k)) {
            if (!live) dv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            else *reinterpret_cast<float4 *>(p.dy + (a * p.lout + m.l(k)) * p.cout + m.c) = dv[k];
            *reinterpret_cast<float4 *>(T0 + m.row(k) * ldt + m.c) = gv[k];
            *reinterpret_cast<float4 *>(T1 + m.row(k) * ldt + m.c) =
                make_float4(gv[k].x * yv[k].x, gv[k].y * yv[k].y, gv[k].z * yv[k].z, gv[k].w * yv[k].w);
        }
    }
    lds_barrier();
    // ---- per-workgroup dgamma / dbeta partials (rows of absent actors hold zeros), fixed order
    for (int e = tid; e < 2 * p.cout; e += 512) {
        const int which = e / p.cout, cc = e - which * p.cout;
        const float *col = (which == 0 ? T1 : T0) + cc;
        float acc = 0.f;
        for (int r = 0; r < kConvRows; ++r) acc += col[r * ldt];
        p.part[((int64_t)blockIdx.x * 2 + which) * p.cout + cc] = acc;
    }
    // ---- dres of the x2-upsampled residual: res'[l] = w0(l) r[i0(l)] + w1(l) r[i1(l)]  ->  dr[h] = sum_l g[l] w(l -> h)
    if (p.res_mode == 2 && p.dres) {
        const int half = p.lout >> 1, c4 = m.c4, per_a = half * c4;
        for (int e = tid; e < na * per_a; e += 512) {
            const int ah = e / per_a, rem = e - ah * per_a, h = rem / c4, cq = 4 * (rem - (rem / c4) * c4);
            if (a0 + ah >= p.n_act) continue;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            const int l0 = 2 * h - 2 > 0 ? 2 * h - 2 : 0, l1 = 2 * h + 2 < p.lout - 1 ? 2 * h + 2 : p.lout - 1;
            for (int l = l0; l <= l1; ++l) {
                int i0, i1;
                float w1;
                up2_taps(l, half, i0, i1, w1);
                const float w = (i0 == h ? 1.0f - w1 : 0.f) + (i1 == h ? w1 : 0.f);
                if (w != 0.f) {
                    const float4 gl = *reinterpret_cast<const float4 *>(T0 + (ah * p.lout + l) * ldt + cq);
                    acc.x += w * gl.x; acc.y += w * gl.y; acc.z += w * gl.z; acc.w += w * gl.w;
                }
            }
            *reinterpret_cast<float4 *>(p.dres + ((a0 + ah) * half + h) * p.cout + cq) = acc;
        }
    }
    if (p.dx == nullptr) return;                                // block-uniform
    lds_barrier();                                              // T0 / T1 are done with: dy takes T0's place
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (m.has(k)) *reinterpret_cast<float4 *>(T0 + m.row(k) * ldt + m.c) = dv[k];
    if (tid < m.c4) *reinterpret_cast<float4 *>(T0 + kConvRows * ldt + 4 * tid) = make_float4(0.f, 0.f, 0.f, 0.f);
    lds_barrier();

    // ---- dx[r_in, ci] = sum_t sum_co dy[row(r_in, t), co] W[co, ci, t]: row(r_in, t) = the output row whose tap t reads
    // input row r_in (l stride + t - pad = li), or the zero row.  M = the na * lin input rows (16-row tiles), N = cin (16-
    // column blocks), K = ks x cout.  Wave -> one column block and every nwn-th row tile; a lane reads 4 consecutive K values
    // of its row (one ds_read_b128) and of its weight column (one 16-byte load), fed to 4 MFMAs as k-slot (lane >> 4).
    const int cin16 = (p.cin + 15) & ~15, nt = cin16 >> 4, nwn = 8 / nt;
    const int n_in = na * p.lin, mt = (n_in + 15) >> 4;
    const int nb = wave % nt, mb0 = wave / nt;
    if (mb0 >= nwn) return;                                     // wave-uniform
    const int pad = (p.ks - 1) >> 1, kq = lane >> 4;
    constexpr int kMaxT = 10;                                   // n_in <= 160
    f32x4 acc[kMaxT];
    int ar[kMaxT], li[kMaxT];
#pragma unroll
    for (int i = 0; i < kMaxT; ++i) {
        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int r = 16 * (mb0 + i * nwn) + (lane & 15);
        ar[i] = r < n_in ? r / p.lin : -1;
        li[i] = r - (r < n_in ? ar[i] : 0) * p.lin;
    }
    const float *wcol = p.wt + (int64_t)(16 * nb + (lane & 15)) * p.cout + 4 * kq;
    for (int t = 0; t < p.ks; ++t) {
        int roff[kMaxT];
#pragma unroll
        for (int i = 0; i < kMaxT; ++i) {
            const int num = li[i] + pad - t;
            const int l = num / p.stride;
            const bool ok = ar[i] >= 0 && num >= 0 && l * p.stride == num && l < p.lout;
            roff[i] = (ok ? ar[i] * p.lout + l : kConvRows) * ldt + 4 * kq;
        }
        const float *wt_t = wcol + (int64_t)t * cin16 * p.cout;
        for (int kb = 0; kb < p.cout; kb += 16) {
            const float4 b = *reinterpret_cast<const float4 *>(wt_t + kb);
#pragma unroll
            for (int i = 0; i < kMaxT; ++i) {
                if (mb0 + i * nwn < mt) {                       // wave-uniform
                    const float4 av = *reinterpret_cast<const float4 *>(T0 + roff[i] + kb);
                    f32x4 cacc = acc[i];
                    cacc = mfma4(av.x, b.x, cacc);
                    cacc = mfma4(av.y, b.y, cacc);
                    cacc = mfma4(av.z, b.z, cacc);
                    cacc = mfma4(av.w, b.w, cacc);
                    acc[i] = cacc;
                }
            }
        }
    }
    const int ci = 16 * nb + (lane & 15);
#pragma unroll
    for (int i = 0; i < kMaxT; ++i) {
        if (mb0 + i * nwn < mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * (mb0 + i * nwn) + 4 * kq + r;     // C/D: row 4 (lane >> 4) + r, column lane & 15
                if (row < n_in && ci < p.cin) {
                    const int arow = row / p.lin;
                    if (a0 + arow < p.n_act) p.dx[((a0 + arow) * p.lin + (row - arow * p.lin)) * p.cin + ci] = acc[i][r];
                }
            }
        }
    }
}

struct ConvWgradParams {
    const float *dy, *x;               // [A, lout, cout], [A, lin, cin]
    int64_t n_act;
    int lin, cin, cout, ks, stride, lout;
    int n_groups, n_chunks;
    float *part;                       // [n_chunks][ks][cout][cin16]
};

// Workgroup (chunk, t): the 80 dy rows of an actor group and the group's input rows (+ a zero row) staged in LDS, then
// partial[co, ci] += sum_rows dy[row, co] x[row shifted by tap t, ci] on v_mfma_f32_16x16x4_f32 (A = dy^T: column of dy
// along the lanes, B = the shifted x rows; K = 4 rows per instruction).  16 x 16 output tiles, tile w + 8 k to wave w.
__global__ __launch_bounds__(512) void k_conv_wgrad(const ConvWgradParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, t = blockIdx.y;
    const int na = kConvRows / p.lout, n_in = na * p.lin;
    const int cin16 = (p.cin + 15) & ~15, ldd = p.cout + 4, ldx = cin16 + 4;
    float *D = reinterpret_cast<float *>(smem), *X = D + kConvRows * ldd;
    const int pad = (p.ks - 1) >> 1, mt = p.cout >> 4, ntile = mt * (cin16 >> 4);
    constexpr int kMaxW = 8;                                    // <= 64 tiles of 16 x 16 per tap
    f32x4 acc[kMaxW];
#pragma unroll
    for (int k = 0; k < kMaxW; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kq = lane >> 4, col = lane & 15;
    for (int grp = chunk; grp < p.n_groups; grp += p.n_chunks) {
        const int64_t a0 = (int64_t)grp * na;
        const int c4 = p.cout >> 2;
        for (int e = tid; e < kConvRows * c4; e += 512) {       // dy rows a0 * lout .. + 79 are contiguous
            const int r = e / c4, cq = 4 * (e - r * c4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a0 + r / p.lout < p.n_act) v = *reinterpret_cast<const float4 *>(p.dy + (a0 * p.lout + r) * p.cout + cq);
            *reinterpret_cast<float4 *>(D + r * ldd + cq) = v;
        }
        const int q4 = cin16 >> 2;
        for (int e = tid; e < (n_in + 1) * q4; e += 512) {       // 4 channels per step (cin % 4 == 0: one 16-byte load)
            const int r = e / q4, ci = 4 * (e - r * q4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < n_in && ci < p.cin && a0 + r / p.lin < p.n_act) {
                const float *src = p.x + (a0 * p.lin + r) * p.cin + ci;
                if ((p.cin & 3) == 0) v = *reinterpret_cast<const float4 *>(src);
                else {
                    v.x = src[0];
                    if (ci + 1 < p.cin) v.y = src[1];
                    if (ci + 2 < p.cin) v.z = src[2];
                    if (ci + 3 < p.cin) v.w = src[3];
                }
            }
            *reinterpret_cast<float4 *>(X + r * ldx + ci) = v;
        }
        lds_barrier();
        for (int kb = 0; kb < kConvRows; kb += 4) {
            const int row = kb + kq, ar = row / p.lout, l = row - ar * p.lout, lx = l * p.stride + t - pad;
            const float *xr = X + ((lx >= 0 && lx < p.lin) ? ar * p.lin + lx : n_in) * ldx + col;
            const float *dr = D + row * ldd + col;
#pragma unroll
            for (int k = 0; k < kMaxW; ++k) {
                const int tile = wave + 8 * k;
                if (tile < ntile) {                             // wave-uniform
                    const int mb = tile % mt, nb = tile / mt;
                    acc[k] = mfma4(dr[16 * mb], xr[16 * nb], acc[k]);
                }
            }
        }
        lds_barrier();
    }
    float *o = p.part + ((int64_t)chunk * p.ks + t) * p.cout * cin16;
#pragma unroll
    for (int k = 0; k < kMaxW; ++k) {
        const int tile = wave + 8 * k;
        if (tile < ntile) {
            const int mb = tile % mt, nb = tile / mt;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[(int64_t)(16 * mb + 4 * kq + r) * cin16 + 16 * nb + col] = acc[k][r];
        }
    }
}

// Blocks [0, n_wblk): dW[co][ci][t] = sum over chunks (one thread per element, chunk order).  Blocks after them: one wave
// per dgamma / dbeta channel, lanes over the workgroup partials (stride 64), then a fixed butterfly.
__global__ __launch_bounds__(256) void k_conv_bwd_reduce(const float *__restrict__ wpart, int n_chunks, int ks, int cout,
                                                         int cin, int n_wblk, const float *__restrict__ gpart, int n_wg,
                                                         float *__restrict__ dw, float *__restrict__ dgamma,
                                                         float *__restrict__ dbeta) {
    const int cin16 = (cin + 15) & ~15;
    if ((int)blockIdx.x < n_wblk) {
        const int e = blockIdx.x * 256 + threadIdx.x, total = cout * cin * ks;
        if (e >= total) return;
        const int co = e / (cin * ks), rem = e - co * (cin * ks), ci = rem / ks, t = rem - ci * ks;
        const float *q = wpart + ((int64_t)t * cout + co) * cin16 + ci;
        const int64_t step = (int64_t)ks * cout * cin16;
        float s = 0.f;
        for (int ch = 0; ch < n_chunks; ++ch) s += q[ch * step];
        dw[e] = s;
        return;
    }
    const int o = (blockIdx.x - n_wblk) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= 2 * cout) return;                                  // wave-uniform
    const int which = o / cout, cc = o - which * cout;          // 0: dgamma, 1: dbeta
    float s = 0.f;
    for (int b = lane; b < n_wg; b += 64) s += gpart[((int64_t)b * 2 + which) * cout + cc];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    float *dst = which == 0 ? dgamma : dbeta;
    if (lane == 0 && dst) dst[cc] = s;
}

// workspace layout (floats): dy [A lout cout] | GroupNorm partials [n_wg][2][cout] | wgrad partials [n_chunks][ks][cout][cin16]
struct ConvBwdLayout {
    int lout, na, n_wg, n_chunks;
    int64_t dy, gpart, wpart, total;
};

static bool conv_bwd_layout(int64_t n_act, int lin, int cin, int cout, int ks, int stride, ConvBwdLayout &L) {
    const int pad = (ks - 1) / 2;
    L.lout = stride > 0 ? (lin + 2 * pad - ks) / stride + 1 : 0;
    if (n_act < 0 || !conv_shape_ok(cin, cout, ks, stride, lin, L.lout)) return false;
    if (n_act > 0x7fffffff / (kConvRows * 128)) return false;
    L.na = kConvRows / L.lout;
    L.n_wg = (int)((n_act + L.na - 1) / L.na);
    const int target = 192 / ks;                                // ~192 wgrad workgroups, partials <= 192 x cout x cin16
    L.n_chunks = L.n_wg < target ? (L.n_wg > 0 ? L.n_wg : 1) : target;
    L.dy = 0;
    L.gpart = n_act * L.lout * cout;
    L.wpart = L.gpart + (int64_t)L.n_wg * 2 * cout;
    L.total = L.wpart + (int64_t)L.n_chunks * ks * cout * ((cin + 15) & ~15);
    return true;
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int64_t lgcn_conv_packed_t_bytes(int cin, int cout, int ks) {
    if (!conv_weight_ok(cin, cout, ks)) return LGCN_EINVAL;
    return (int64_t)ks * ((cin + 15) & ~15) * cout * 4;
}

int lgcn_conv_pack_weight_t(const float *w, int cin, int cout, int ks, void *out, void *stream) {
    const int64_t nbytes = lgcn_conv_packed_t_bytes(cin, cout, ks);
    if (nbytes < 0) return LGCN_EINVAL;
    LGCN_CHECK_PTR(w); LGCN_CHECK_PTR(out); LGCN_CHECK_ALIGN16(out);
    const int64_t total = nbytes / 4;
    hipLaunchKernelGGL(k_conv_pack_t, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, cout, cin, ks,
                       reinterpret_cast<float *>(out));
    return launch_status();
}

int64_t lgcn_conv1d_gn_bwd_ws_bytes(int64_t n_act, int lin, int cin, int cout, int ks, int stride) {
    ConvBwdLayout L;
    if (!conv_bwd_layout(n_act, lin, cin, cout, ks, stride, L)) return LGCN_ESHAPE;
    return L.total * 4;
}

int lgcn_conv1d_gn_bwd(const float *g, const float *x, const float *y, const float *out, int64_t n_act, int lin, int cin,
                       const void *wt, int cout, int ks, int stride, const float *gamma, float eps, int res_mode, int relu,
                       float *dx, float *dw, float *dgamma, float *dbeta, float *dres, void *ws, void *stream) {
    if (n_act < 0 || res_mode < 0 || res_mode > 2) return LGCN_EINVAL;
    ConvBwdLayout L;
    if (!conv_bwd_layout(n_act, lin, cin, cout, ks, stride, L)) return LGCN_ESHAPE;
    if (res_mode == 2 && (L.lout & 1)) return LGCN_ESHAPE;
    if (n_act == 0) return LGCN_OK;
    const void *al[] = {g, y, wt, gamma, ws};
    for (const void *v : al) { LGCN_CHECK_PTR(v); LGCN_CHECK_ALIGN16(v); }
    if (relu) { LGCN_CHECK_PTR(out); LGCN_CHECK_ALIGN16(out); }
    if (dw) { LGCN_CHECK_PTR(x); LGCN_CHECK_ALIGN16(x); LGCN_CHECK_ALIGN16(dw); }
    if (dres) LGCN_CHECK_ALIGN16(dres);
    if (dx) LGCN_CHECK_ALIGN16(dx);
    if (dgamma) LGCN_CHECK_ALIGN16(dgamma);
    if (dbeta) LGCN_CHECK_ALIGN16(dbeta);
    float *wsf = reinterpret_cast<float *>(ws);
    hipStream_t st = (hipStream_t)stream;

    ConvBwdParams p;
    p.g = g; p.y = y; p.out = out; p.n_act = n_act;
    p.lin = lin; p.cin = cin; p.cout = cout; p.ks = ks; p.stride = stride; p.lout = L.lout;
    p.wt = reinterpret_cast<const float *>(wt); p.gamma = gamma; p.eps = eps; p.res_mode = res_mode; p.relu = relu;
    p.dx = dx; p.dres = res_mode ? dres : nullptr; p.dy = wsf + L.dy; p.part = wsf + L.gpart;
    const size_t lds_b = (size_t)2 * (kConvRows + 1) * (cout + 4) * 4;
    int rc = set_lds(reinterpret_cast<const void *>(k_conv_gn_bwd), lds_b);
    if (rc != LGCN_OK) return rc;
    hipLaunchKernelGGL(k_conv_gn_bwd, dim3((unsigned)L.n_wg), dim3(512), lds_b, st, p);

    if (dw) {
        ConvWgradParams q;
        q.dy = wsf + L.dy; q.x = x; q.n_act = n_act;
        q.lin = lin; q.cin = cin; q.cout = cout; q.ks = ks; q.stride = stride; q.lout = L.lout;
        q.n_groups = L.n_wg; q.n_chunks = L.n_chunks; q.part = wsf + L.wpart;
        const size_t lds_w = conv_lds_tile(cout) + (size_t)(L.na * lin + 1) * (((cin + 15) & ~15) + 4) * 4;
        rc = set_lds(reinterpret_cast<const void *>(k_conv_wgrad), lds_w);
        if (rc != LGCN_OK) return rc;
        hipLaunchKernelGGL(k_conv_wgrad, dim3((unsigned)L.n_chunks, (unsigned)ks), dim3(512), lds_w, st, q);
    }
    if (dw || dgamma || dbeta) {
        const int n_wblk = dw ? (cout * cin * ks + 255) / 256 : 0;
        const int n_gblk = (dgamma || dbeta) ? (2 * cout + 3) / 4 : 0;
        hipLaunchKernelGGL(k_conv_bwd_reduce, dim3((unsigned)(n_wblk + n_gblk)), dim3(256), 0, st, wsf + L.wpart, L.n_chunks,
                           ks, cout, cin, n_wblk, wsf + L.gpart, L.n_wg, dw, dgamma, dbeta);
    }
    return launch_status();
}

}  // extern "C"
