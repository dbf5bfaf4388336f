// Shape rules and building blocks shared by ActorNet's convolution kernels (lgcn_conv.hip: forward, lgcn_conv_bwd.hip:
// backward): staging of an actor group's rows in LDS, the shifted GEMM over them, the accumulator -> tile store, the
// GroupNorm thread map and its two-pass statistics, LDS sizing.  One definition each: the fused block equals its units,
// and the backward recomputes the forward's statistics, because they run the same code.
#pragma once
#include "lgcn_common.hpp"
#include "lgcn_mma_bf.hpp"

namespace lgcn {

constexpr int kConvRows = 80;          // output rows per workgroup (5 sub-blocks of 16): 80 / lout whole actors
constexpr int kConvSub = kConvRows / 16;

__host__ __device__ inline int conv_kpad(int cin) { return (cin + 31) & ~31; }

// F.interpolate(scale_factor = 2, mode = "linear", align_corners = False) of a length-n sequence at output position j:
// source coordinate (j + 0.5) / 2 - 0.5, clamped at 0; weights 0.75 / 0.25 (and 1 / 0 at the two ends).
__device__ __forceinline__ void up2_taps(int j, int n, int &i0, int &i1, float &w1) {
    float src = (j + 0.5f) * 0.5f - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + 1 < n ? i0 + 1 : n - 1;
    w1 = src - (float)i0;
}

inline bool conv_weight_ok(int cin, int cout, int ks) {
    return cin >= 1 && cin <= 128 && (cout == 32 || cout == 64 || cout == 128) && (ks == 1 || ks == 3);
}

inline bool conv_shape_ok(int cin, int cout, int ks, int stride, int lin, int lout) {
    if (!conv_weight_ok(cin, cout, ks) || (stride != 1 && stride != 2) || lin < 1) return false;
    const int pad = (ks - 1) / 2;
    if (lout != (lin + 2 * pad - ks) / stride + 1) return false;
    return lout == 5 || lout == 10 || lout == 20;             // 16 / 8 / 4 actors per workgroup: 512 / na threads each in the GroupNorm phase
}

// Dynamic LDS of the three layouts a forward workgroup's region takes: an actor group's input rows (+ a zero row) as two
// fp16 planes (fp32 rows are at most as wide), the 80 x cout fp32 tile, 80 intermediate rows (+ a zero row) as planes.
inline size_t conv_lds_in_planes(int na, int lin, int cin) { return (size_t)2 * (na * lin + 1) * (conv_kpad(cin) + 8) * 2; }
inline size_t conv_lds_tile(int cout) { return (size_t)kConvRows * (cout + 4) * 4; }
inline size_t conv_lds_mid_planes(int c) { return (size_t)2 * (kConvRows + 1) * (c + 8) * 2; }

// The kernel's static words share the 160 KB; above the default ceiling of dynamic LDS the limit is raised (a property
// set on the code object; idempotent).
inline int set_lds(const void *kern, size_t lds) {
    if (lds > 159 * 1024) return LGCN_ESHAPE;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
        if (e != hipSuccess) return (int)e;
    }
    return LGCN_OK;
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// 4 consecutive channels of a row as two fp16 planes: hi = the rounding of v, lo = the rounding of what it left
__device__ __forceinline__ void conv_split_store(uint16_t *hi, uint16_t *lo, float4 v) {
    const uint32_t h0 = Fmt<1>::pack(v.x, v.y), h1 = Fmt<1>::pack(v.z, v.w);
    const f32x2 r0 = Fmt<1>::unpack(h0), r1 = Fmt<1>::unpack(h1);
    *reinterpret_cast<uint2 *>(hi) = make_uint2(h0, h1);
    *reinterpret_cast<uint2 *>(lo) = make_uint2(Fmt<1>::pack(v.x - r0.x, v.y - r0.y), Fmt<1>::pack(v.z - r1.x, v.w - r1.y));
}

// Stage the input rows of actors a0 .. a0 + n_in / lin - 1 (and the all-zero row n_in) in LDS, ldk elements per row, cin
// padded to a multiple of 32 with zeros: two fp16 planes of (n_in + 1) * ldk elements each, or (F32) the fp32 rows as they
// are.  4 channels per thread and step, four row loads in flight.
template <bool F32>
__device__ __forceinline__ void conv_stage_rows(unsigned char *smem, const float *x, int64_t a0, int64_t n_act, int lin,
                                                int cin, int n_in, int ldk, int tid) {
    uint16_t *P0 = reinterpret_cast<uint16_t *>(smem), *P1 = P0 + (n_in + 1) * ldk;
    float *X = reinterpret_cast<float *>(smem);
    const int c4n = conv_kpad(cin) / 4, total = (n_in + 1) * c4n;
    for (int i0 = tid; i0 < total; i0 += 4 * 512) {
        float4 v[4];
        int rr[4], cc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 512;
            const int r = i / c4n, c = 4 * (i - r * c4n);
            rr[u] = r; cc[u] = c;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int ar = r / lin;
            const int64_t a = a0 + ar;
            if (i < total && r < n_in && a < n_act) {
                const float *src = x + (a * lin + (r - ar * lin)) * cin + c;
                if (c + 3 < cin && (cin & 3) == 0) v[u] = *reinterpret_cast<const float4 *>(src);
                else {
                    if (c < cin) v[u].x = src[0];
                    if (c + 1 < cin) v[u].y = src[1];
                    if (c + 2 < cin) v[u].z = src[2];
                    if (c + 3 < cin) v[u].w = src[3];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u * 512 < total) {
                const int off = rr[u] * ldk + cc[u];
                if constexpr (F32) *reinterpret_cast<float4 *>(X + off) = v[u];
                else conv_split_store(P0 + off, P1 + off, v[u]);
            }
        }
    }
}

// A wave's share of the 80 x cout output tile: one 16-channel block cb and the 16-row sub-blocks rb0, rb0 + nw, ...
struct ConvWave {
    int lane, kq, ncb, nw, cb, rb0;
    __device__ __forceinline__ ConvWave(int cout, int tid) {
        const int wave = tid >> 6;
        lane = tid & 63; kq = lane >> 4;
        ncb = cout >> 4; nw = 8 / ncb;
        cb = wave % ncb; rb0 = wave / ncb;
    }
    __device__ __forceinline__ bool has(int i) const { return rb0 + i * nw < kConvSub; }       // wave-uniform
    // packed weight fragments of K-step s = t * nkc + kc (lgcn_conv_pack_weight / _f32's image)
    __device__ __forceinline__ void wfrag(const uint4 *wp, int s, uint4 &h, uint4 &l) const {
        const int64_t wb = (((int64_t)s * ncb + cb) * 2) << 6;
        h = wp[wb + lane];
        l = wp[wb + 64 + lane];
    }
};

// A wave's accumulators: 4 consecutive channels x its row of sub-block i per lane (one f32x4 per sub-block).  A struct,
// not a bare array: hipcc turns a bare array of vectors that a not yet unrolled loop indexes into ONE 20-float vector
// right after inlining (2 - 4 x the VGPRs, scratch in the exact units); a struct is left to the scalar replacement
// behind the unroller.
struct ConvAcc { f32x4 v[kConvSub]; };

// The staged operand rows of one convolution and where this lane's output rows read them.
template <bool F32>
struct ConvRows {
    const unsigned char *p;            // fp16: plane 0, plane 1 `plane` elements behind it; F32: the fp32 rows
    int plane, ld, zero_row, lin;
    int ks;                            // taps: with the padding it fixes lpos, so it lives here; conv_taps loops over it
    int base[kConvSub], lpos[kConvSub];    // per sub-block: the actor's first staged row, the position under tap 0
    __device__ __forceinline__ ConvRows(const unsigned char *p_, int plane_, int ld_, int zero_row_, int lin_, int stride,
                                        int ks_, int lout, const ConvWave &w)
        : p(p_), plane(plane_), ld(ld_), zero_row(zero_row_), lin(lin_), ks(ks_) {
        const int pad = (ks - 1) >> 1;
#pragma unroll
        for (int i = 0; i < kConvSub; ++i) {
            const int r = 16 * (w.rb0 + i * w.nw) + (w.lane & 15);     // this lane's output row (may be >= 80: unused)
            const int a = r / lout, l = r - a * lout;
            base[i] = a * lin;
            lpos[i] = l * stride - pad;
        }
    }
    // LDS element offset of this lane's rows under tap t (rows outside the sequence read the zero row)
    __device__ __forceinline__ void tap(int t, int kq, int (&roff)[kConvSub]) const {
#pragma unroll
        for (int i = 0; i < kConvSub; ++i) {
            const int li = lpos[i] + t;
            roff[i] = ((li >= 0 && li < lin) ? base[i] + li : zero_row) * ld + (F32 ? 4 : 8) * kq;
        }
    }
};

// One K-step (32 input channels of one tap) of out^T = W x^T for the wave's sub-blocks; b0 / b1: its weight fragments.
template <bool F32>
__device__ __forceinline__ void conv_kstep(const ConvWave &w, const ConvRows<F32> &rows, const int (&roff)[kConvSub], int kc,
                                           const uint4 b0, const uint4 b1, ConvAcc &acc) {
    if constexpr (F32) {
        // b0 / b1: the weights of channels 32 kc + 4 kq + j and 32 kc + 16 + 4 kq + j.  The sub-blocks' chains are
        // independent: they are interleaved so that an MFMA does not wait for the one before it (40 cycles).
        const float *X = reinterpret_cast<const float *>(rows.p);
        const f32x4 wf[2] = {__builtin_bit_cast(f32x4, b0), __builtin_bit_cast(f32x4, b1)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ConvAcc a;                                          // the rows' 4 channels (a struct for ConvAcc's reason)
#pragma unroll
            for (int i = 0; i < kConvSub; ++i)
                if (w.has(i)) a.v[i] = *reinterpret_cast<const f32x4 *>(X + roff[i] + 32 * kc + 16 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < kConvSub; ++i)
                    if (w.has(i)) acc.v[i] = mfma4(wf[h][j], a.v[i][j], acc.v[i]);
        }
    } else {
        const uint16_t *P0 = reinterpret_cast<const uint16_t *>(rows.p), *P1 = P0 + rows.plane;
#pragma unroll
        for (int i = 0; i < kConvSub; ++i) {
            if (w.has(i)) {
                const int off = roff[i] + 32 * kc;
                const uint4 a_hi = *reinterpret_cast<const uint4 *>(P0 + off);
                const uint4 a_lo = *reinterpret_cast<const uint4 *>(P1 + off);
                f32x4 c = acc.v[i];                             // smallest terms first; weights first: D^T, 4 channels per lane
                c = Fmt<1>::mfma(b0, a_lo, c);
                c = Fmt<1>::mfma(b1, a_hi, c);
                c = Fmt<1>::mfma(b0, a_hi, c);
                acc.v[i] = c;
            }
        }
    }
}

// acc = one convolution as rows.ks x nkc K-steps (tap outer, chunk inner) over staged rows, weight fragments one K-step ahead
template <bool F32>
__device__ __forceinline__ void conv_taps(const ConvWave &w, const ConvRows<F32> &rows, int nkc, const uint4 *wp,
                                          ConvAcc &acc) {
#pragma unroll
    for (int i = 0; i < kConvSub; ++i) acc.v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nks = rows.ks * nkc;
    uint4 nb0, nb1;
    w.wfrag(wp, 0, nb0, nb1);
    for (int t = 0; t < rows.ks; ++t) {
        int roff[kConvSub];
        rows.tap(t, w.kq, roff);
        for (int kc = 0; kc < nkc; ++kc) {
            const uint4 b0 = nb0, b1 = nb1;
            const int sn = t * nkc + kc + 1;
            w.wfrag(wp, sn < nks ? sn : nks - 1, nb0, nb1);
            conv_kstep<F32>(w, rows, roff, kc, b0, b1, acc);
        }
    }
}

// The wave's accumulators to the fp32 tile T[80][ldt] (D^T: a lane holds 4 consecutive channels of its row)
__device__ __forceinline__ void conv_acc_to_tile(const ConvWave &w, float *T, int ldt, const ConvAcc &acc) {
#pragma unroll
    for (int i = 0; i < kConvSub; ++i)
        if (w.has(i))
            *reinterpret_cast<f32x4 *>(T + (16 * (w.rb0 + i * w.nw) + (w.lane & 15)) * ldt + 16 * w.cb + 4 * w.kq) = acc.v[i];
}

// GroupNorm over (lout x cout) per actor, all 512 threads: 512 / na threads per actor (128, 64 or 32), each keeps <= 5
// float4 of the actor in registers -- float4 i = j + k * tpa of the actor's n4, row i / c4, channels c .. c + 3 (the quad
// is the same for every k: threads-per-actor is a multiple of cout / 4).
struct ConvGnMap {
    int tid, lout, tpa, al, j, c4, n4, c, g0, ng;
    float per;
    __device__ __forceinline__ ConvGnMap(int lout_, int cout, int tid_) : tid(tid_), lout(lout_) {
        tpa = 512 / (kConvRows / lout); al = tid / tpa; j = tid - al * tpa;
        c4 = cout >> 2; n4 = lout * c4;                         // float4 columns per row, float4s per actor
        c = 4 * (j % c4);
        g0 = (al * tpa) >> 5; ng = tpa >> 5;                    // this actor's half-waves
        per = (float)(lout * cout);
    }
    __device__ __forceinline__ bool has(int k) const { return j + k * tpa < n4; }
    __device__ __forceinline__ int l(int k) const { return (j + k * tpa) / c4; }               // row within the actor
    __device__ __forceinline__ int row(int k) const { return al * lout + l(k); }               // row within the workgroup's 80
};

// sum over the 32 lanes of a half-wave (butterfly: every lane ends with it)
__device__ __forceinline__ float conv_half_sum(float s) {
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// The per-actor statistics of the values the actor's threads hold (absent ones are zero), two passes as ATen's GroupNorm:
// mean, then the variance about it.  They meet through 32-lane shuffles and one LDS word per half-wave, summed in
// ascending order.  Contains two barriers; s_red: 2 x 16 words.
// WIDE: the exact units (fp32 operands, fp32's exponent range) and the backward that recomputes their statistics.  Centred
// values beyond ~2^58 (lout x cout <= 2,560 squares) take the sum of squares out of fp32: var = inf, rstd = 0, and the
// actor would come out as beta.  Then the same sum is formed over the centred values scaled by 2^-70 (exact) and rstd is
// scaled back -- row_rstd_wide (lgcn_tile.hpp) for this layout.  The workgroup's actors do not share var and the second
// sum needs barriers, so every thread forms every actor's sum from s_red (the same additions in the same order as the
// owner's) and the workgroup takes the branch together; only the actors whose own sum left fp32 replace their rstd, so
// every other actor keeps its bits.  An actor that holds a NaN or an inf takes the branch too and comes out NaN as before.
// The two-plane kernels pass WIDE = false and keep their code: their convolution outputs cannot pass
// 3 * 128 * 3 * 65520^2 < 2^43, whose squares fit.
template <bool WIDE = false>
__device__ __forceinline__ void conv_gn_stats(const float4 (&v)[5], const ConvGnMap &m, float (*s_red)[16], float eps,
                                              float &mean, float &rstd) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    s = conv_half_sum(s);
    if ((m.tid & 31) == 0) s_red[0][m.tid >> 5] = s;
    lds_barrier();
    mean = 0.f;
    for (int k = 0; k < m.ng; ++k) mean += s_red[0][m.g0 + k];
    mean = mean / m.per;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        if (m.has(k)) {
            const float d0 = v[k].x - mean, d1 = v[k].y - mean, d2 = v[k].z - mean, d3 = v[k].w - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    }
    q = conv_half_sum(q);
    if ((m.tid & 31) == 0) s_red[1][m.tid >> 5] = q;
    lds_barrier();
    float var = 0.f;
    for (int k = 0; k < m.ng; ++k) var += s_red[1][m.g0 + k];
    rstd = 1.0f / sqrtf(var / m.per + eps);
    if constexpr (WIDE) {
        bool any = false;                                       // workgroup-uniform: every actor's sum, as its owner formed it
        for (int g = 0; g < 16; g += m.ng) {
            float t = 0.f;
            for (int k = 0; k < m.ng; ++k) t += s_red[1][g + k];
            any |= !(t <= 3.4028234e38f);
        }
        if (__builtin_expect(any, 0)) {
            constexpr float ks = 0x1p-70f;
            float qs = 0.f;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                if (m.has(k)) {
                    const float d0 = (v[k].x - mean) * ks, d1 = (v[k].y - mean) * ks, d2 = (v[k].z - mean) * ks,
                                d3 = (v[k].w - mean) * ks;
                    qs += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                }
            }
            qs = conv_half_sum(qs);
            lds_barrier();                                      // every thread has read the first sums
            if ((m.tid & 31) == 0) s_red[1][m.tid >> 5] = qs;
            lds_barrier();
            float vs = 0.f;
            for (int k = 0; k < m.ng; ++k) vs += s_red[1][m.g0 + k];
            if (!(var <= 3.4028234e38f)) rstd = ks / sqrtf(vs / m.per + eps * (ks * ks));
        }
    }
}

// a thread's <= 5 float4 of the fp32 tile
__device__ __forceinline__ void conv_tile_load(const float *T, int ldt, const ConvGnMap &m, float4 (&v)[5]) {
#pragma unroll
    for (int k = 0; k < 5; ++k)
        v[k] = m.has(k) ? *reinterpret_cast<const float4 *>(T + m.row(k) * ldt + m.c) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float4 conv_gn_apply(float4 v, float mean, float rstd, float4 g, float4 b) {
    return make_float4((v.x - mean) * rstd * g.x + b.x, (v.y - mean) * rstd * g.y + b.y,
                       (v.z - mean) * rstd * g.z + b.z, (v.w - mean) * rstd * g.w + b.w);
}

}  // namespace lgcn
