// ActorNet's building block (reference layers.py:40-62 Conv1d, 142-190 Res1d; lanegcn.py:212-263) in ONE launch:
//
//   out[a, l, :] = act( GN_{(C, L) of actor a}( sum_t W_t x[a, l * stride + t - pad, :] ) + residual )
//
// on channels-last tensors x [A, Lin, Cin], out [A, Lout, Cout] (Lout = (Lin + 2 pad - K) / stride + 1, pad = (K - 1) / 2,
// K = 1 or 3, stride = 1 or 2, Cin <= 128, Cout in {32, 64, 128}, GroupNorm with one group = statistics over all
// Lout x Cout values of an actor).  residual: none | a tensor of the output's shape | a tensor of half the length,
// upsampled x2 on the fly (F.interpolate(mode="linear", align_corners=False): the FPN's top-down step).
//
// A workgroup owns NA whole actors = 80 output rows (NA = 80 / Lout: 4, 8 or 16 actors at Lout = 20, 10, 5), so the
// GroupNorm statistics never leave the CU.  The actors' input rows are staged once in LDS as fp16 operand planes
// (2 planes, 3 products: the fp32-grade split of lgcn_mma_bf.hpp); the convolution is K x ceil(Cin / 32) MFMA K-steps
// whose A fragments are the staged rows shifted by the tap (rows outside the sequence read an all-zero row); a wave
// owns one 16-channel block of the output and a share of the five 16-row sub-blocks, its weight fragments come from
// the packed image (lgcn_conv_pack_weight) once per K-step.  The 80 x Cout fp32 tile then goes through LDS to the
// norm: 512 / NA threads per actor, two passes (mean, then variance about it, as ATen's GroupNorm), residual, ReLU, and
// 512-byte coalesced stores.
#include "lgcn_conv.hpp"

namespace lgcn {

struct ConvParams {
    const float *x;                    // [A, lin, cin]
    int64_t n_act;
    int lin, cin, cout, ks, stride, lout;
    const uint4 *wp;                   // packed weight image
    const float *gamma, *beta;
    float eps;
    const float *res;                  // residual source or null
    int res_mode;                      // 0 none, 1 [A, lout, cout], 2 [A, lout / 2, cout] upsampled x2
    int relu;
    float *out;                        // [A, lout, cout]
    float *y;                          // [A, lout, cout]: the pre-norm convolution output (training forward only)
};

// Packed image: for tap t, K-chunk kc (32 input channels), channel block cb (16 outputs), plane pl: 64 x uint4, lane
// (n = lane & 15, kq = lane >> 4) holds W[16 cb + n][32 kc + 8 kq + j][t], j = 0..7, as fp16 plane pl (hi, then the
// rounding of the residual).  Input channels beyond cin are zero.
__global__ __launch_bounds__(256) void k_conv_pack(const float *w, int cout, int cin, int ks, uint4 *out) {
    const int nkc = conv_kpad(cin) / 32, ncb = cout / 16;
    const int64_t total = (int64_t)ks * nkc * ncb * 64;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int lane = (int)(i & 63);
    int64_t q = i >> 6;
    const int cb = (int)(q % ncb); q /= ncb;
    const int kc = (int)(q % nkc);
    const int t = (int)(q / nkc);
    const int n = lane & 15, kq = lane >> 4;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = 32 * kc + 8 * kq + j;
        v[j] = c < cin ? w[((int64_t)(16 * cb + n) * cin + c) * ks + t] : 0.f;
    }
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hi[j] = Fmt<1>::pack(v[2 * j], v[2 * j + 1]);
        const f32x2 r = Fmt<1>::unpack(hi[j]);
        lo[j] = Fmt<1>::pack(v[2 * j] - r.x, v[2 * j + 1] - r.y);
    }
    const int64_t base = ((((int64_t)t * nkc + kc) * ncb + cb) * 2) << 6;
    out[base + lane] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    out[base + 64 + lane] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// Packed fp32 image (exact units): for tap t, K-chunk kc (32 input channels), channel block cb (16 outputs), half h:
// 64 x float4, lane (n = lane & 15, kq = lane >> 4) holds W[16 cb + n][32 kc + 16 h + 4 kq + j][t], j = 0..3.  The same
// bytes per K chunk as the two fp16 planes.  Input channels beyond cin are zero.
__global__ __launch_bounds__(256) void k_conv_pack_f32(const float *w, int cout, int cin, int ks, float4 *out) {
    const int nkc = conv_kpad(cin) / 32, ncb = cout / 16;
    const int64_t total = (int64_t)ks * nkc * ncb * 128;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int lane = (int)(i & 63), h = (int)((i >> 6) & 1);
    int64_t q = i >> 7;
    const int cb = (int)(q % ncb); q /= ncb;
    const int kc = (int)(q % nkc);
    const int t = (int)(q / nkc);
    const int n = lane & 15, kq = lane >> 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 32 * kc + 16 * h + 4 * kq + j;
        v[j] = c < cin ? w[((int64_t)(16 * cb + n) * cin + c) * ks + t] : 0.f;
    }
    out[i] = make_float4(v[0], v[1], v[2], v[3]);              // i = ((((t nkc + kc) ncb + cb) 2 + h) << 6) + lane
}

// SAVE: also store the pre-norm tile to p.y (the training forward); the arithmetic of `out` is the same either way.
//
// F32: the exact-fp32 unit.  The rows are staged as fp32 and the convolution runs on v_mfma_f32_16x16x4_f32: a lane reads
// 4 consecutive channels of its row (one ds_read_b128) and of its weight row (one 16-byte load, lgcn_conv_pack_weight_f32's
// image) and feeds them to 4 MFMAs as K slot lane >> 4, so an output is ONE fused multiply-add chain in a fixed order.
// Row stride in LDS: the 16 lanes that share an LDS cycle of a ds_read_b128 are 8 rows of one K quarter and the other 8
// rows of the next quarter (4 dwords further on).  They cover the 64 banks once when consecutive rows are 2 (mod 4)
// 16-byte slots apart -- even slots for one quarter, odd for the other: kpad + 8 floats for stride 1 (consecutive rows),
// kpad + 4 for stride 2 (every other row).
template <int KS, int NKC, bool SAVE, bool F32 = false>        // taps, 32-channel K chunks; KS == 0: both read from p (any shape)
__global__ __launch_bounds__(512) void k_conv_gn(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float s_red[2][16];
    const int tid = threadIdx.x;
    const int na = kConvRows / p.lout;                        // actors per workgroup
    const int64_t a0 = (int64_t)blockIdx.x * na;
    const int kpad = conv_kpad(p.cin);
    const int ldk = kpad + (F32 && p.stride == 2 ? 4 : 8);     // elements per staged row (fp16: + 16 B, bank spread; fp32: above)
    const int n_in = na * p.lin;                               // staged input rows; row n_in is all zero
    const int ldt = p.cout + 4;
    float *T = reinterpret_cast<float *>(smem);                // the fp32 tile takes the planes' place once the GEMM is done
    const ConvWave w(p.cout, tid);
    // An L2 round trip is several K-steps long (a K-step is <= 15 MFMAs): with the shape known the first kWd steps'
    // fragments are requested before the rows are staged and the ring is refilled kWd steps ahead.
    constexpr int NKS = KS * NKC, kWd = NKS < 6 ? (NKS ? NKS : 1) : 6;
    uint4 wh[kWd], wl[kWd];
    if constexpr (KS != 0) {
#pragma unroll
        for (int s_ = 0; s_ < kWd; ++s_) w.wfrag(p.wp, s_, wh[s_], wl[s_]);
    }

    conv_stage_rows<F32>(smem, p.x, a0, p.n_act, p.lin, p.cin, n_in, ldk, tid);
    lds_barrier();

    // ---- convolution
    const ConvRows<F32> rows(smem, (n_in + 1) * ldk, ldk, n_in, p.lin, p.stride, p.ks, p.lout, w);
    ConvAcc acc;
    if constexpr (KS != 0) {
        int roff[kConvSub];
#pragma unroll
        for (int i = 0; i < kConvSub; ++i) acc.v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s_ = 0; s_ < NKS; ++s_) {
            if (s_ % NKC == 0) rows.tap(s_ / NKC, w.kq, roff);
            const uint4 b0 = wh[s_ % kWd], b1 = wl[s_ % kWd];
            if (s_ + kWd < NKS) w.wfrag(p.wp, s_ + kWd, wh[s_ % kWd], wl[s_ % kWd]);
            conv_kstep<F32>(w, rows, roff, s_ % NKC, b0, b1, acc);
        }
    } else {
        conv_taps<F32>(w, rows, kpad >> 5, p.wp, acc);          // any shape
    }
    lds_barrier();                                              // every wave is done reading the planes
    conv_acc_to_tile(w, T, ldt, acc);
    lds_barrier();

    // ---- GroupNorm over (lout x cout) per actor, residual, ReLU
    const ConvGnMap m(p.lout, p.cout, tid);
    const int64_t a = a0 + m.al;
    const int c = m.c;
    float4 v[5];
    conv_tile_load(T, ldt, m, v);
    const float4 g = *reinterpret_cast<const float4 *>(p.gamma + c), bt = *reinterpret_cast<const float4 *>(p.beta + c);
    float mean, rstd;
    conv_gn_stats<F32>(v, m, s_red, p.eps, mean, rstd);        // the exact units: with the wide path
    if (a < p.n_act) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (m.has(k)) {
                const int l = m.l(k);
                float4 y = conv_gn_apply(v[k], mean, rstd, g, bt);
                if (p.res_mode == 1) {
                    const float4 r = *reinterpret_cast<const float4 *>(p.res + (a * p.lout + l) * p.cout + c);
                    y.x += r.x; y.y += r.y; y.z += r.z; y.w += r.w;
                } else if (p.res_mode == 2) {
                    int i0, i1;
                    float w1;
                    const int half = p.lout >> 1;
                    up2_taps(l, half, i0, i1, w1);
                    const float4 r0 = *reinterpret_cast<const float4 *>(p.res + (a * half + i0) * p.cout + c);
                    const float4 r1 = *reinterpret_cast<const float4 *>(p.res + (a * half + i1) * p.cout + c);
                    const float w0 = 1.0f - w1;
                    y.x += w0 * r0.x + w1 * r1.x; y.y += w0 * r0.y + w1 * r1.y;
                    y.z += w0 * r0.z + w1 * r1.z; y.w += w0 * r0.w + w1 * r1.w;
                }
                if (p.relu) { y.x = relu_nan(y.x); y.y = relu_nan(y.y); y.z = relu_nan(y.z); y.w = relu_nan(y.w); }
                *reinterpret_cast<float4 *>(p.out + (a * p.lout + l) * p.cout + c) = y;
                if constexpr (SAVE) *reinterpret_cast<float4 *>(p.y + (a * p.lout + l) * p.cout + c) = v[k];
            }
        }
    }
}

// ---------------------------------------------------------------- a whole Res1d block in one launch -----
// layers.Res1d (reference layers.py:142-190):  out = relu( GN2(conv2( relu(GN1(conv1(x))) )) + r ),  conv1 k = 3 stride s,
// conv2 k = 3 stride 1, r = x (cin == c, s == 1) or GN_d(conv_d(x)) with conv_d k = 1 stride s.  Same 80-row workgroups:
// the intermediate never leaves the CU -- GN1's output goes straight back into LDS as operand planes (Y), the shortcut's
// 1 x 1 convolution runs on the staged input right behind conv1 and its normalised rows wait in registers.  A second
// block with the identity shortcut can be chained behind the first (an ActorNet group): its input is the first block's
// output as planes, its shortcut the values each thread still holds.
struct Res1dParams {
    const float *x;                    // [A, lin, cin]
    int64_t n_act;
    int lin, cin, c, stride, lout;
    const uint4 *w1, *w2, *wd;         // packed images (wd: null = identity shortcut)
    const float *g1, *b1, *g2, *b2, *gd, *bd;
    const uint4 *w1b, *w2b;            // a second block with the identity shortcut chained behind the first (null: none)
    const float *g1b, *b1b, *g2b, *b2b;
    float eps;
    float *out;                        // [A, lout, c]
};

__global__ __launch_bounds__(512) void k_res1d_gn(const Res1dParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float s_red[2][16];
    const int tid = threadIdx.x;
    const int na = kConvRows / p.lout;
    const int64_t a0 = (int64_t)blockIdx.x * na;
    const int kpad = conv_kpad(p.cin), ldk = kpad + 8;
    const int n_in = na * p.lin;
    const int ldy = p.c + 8, ldt = p.c + 4;
    // ONE region of LDS serves in turn as the input planes, every fp32 tile and every set of intermediate planes (80 rows
    // + a zero row): each is dead before the next is written -- a tile is consumed into registers by tile_gn (whose two
    // barriers every thread has passed when it returns), planes are done with at the barrier behind their convolution.
    float *T = reinterpret_cast<float *>(smem);
    uint16_t *Y0 = reinterpret_cast<uint16_t *>(smem), *Y1 = Y0 + (kConvRows + 1) * ldy;
    const bool chain = p.w1b != nullptr, down = p.wd != nullptr;
    const ConvWave w(p.c, tid);

    conv_stage_rows<false>(smem, p.x, a0, p.n_act, p.lin, p.cin, n_in, ldk, tid);
    lds_barrier();

    ConvAcc acc;
    auto conv_in = [&](int ks, const uint4 *wp) {               // on the staged input, stride s
        const ConvRows<false> rows(smem, (n_in + 1) * ldk, ldk, n_in, p.lin, p.stride, ks, p.lout, w);
        conv_taps<false>(w, rows, kpad >> 5, wp, acc);
    };
    auto conv_mid = [&](const uint4 *wp) {                      // 3 taps, stride 1 on the intermediate planes
        const ConvRows<false> rows(smem, (kConvRows + 1) * ldy, ldy, kConvRows, p.lout, 1, 3, p.lout, w);
        conv_taps<false>(w, rows, p.c >> 5, wp, acc);
    };
    const ConvGnMap m(p.lout, p.c, tid);
    const int64_t a = a0 + m.al;
    auto tile_gn = [&](float4 (&v)[5], const float *gamma, const float *beta) {     // GroupNorm of the tile; contains two barriers
        const float4 g = *reinterpret_cast<const float4 *>(gamma + m.c), bt = *reinterpret_cast<const float4 *>(beta + m.c);
        conv_tile_load(T, ldt, m, v);
        float mean, rstd;
        conv_gn_stats(v, m, s_red, p.eps, mean, rstd);
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = conv_gn_apply(v[k], mean, rstd, g, bt);
    };

    // ---- conv1 (and the shortcut's 1 x 1 convolution) on the staged input
    conv_in(3, p.w1);
    const ConvAcc acc1 = acc;
    if (down) conv_in(1, p.wd);
    lds_barrier();                                              // the input planes are done with
    conv_acc_to_tile(w, T, ldt, acc1);
    lds_barrier();
    float4 v[5], res[5];
    tile_gn(v, p.g1, p.b1);
    // a thread's normalised values -> operand planes (row = al * lout + l: the output row numbering)
    auto to_planes = [&](const float4 (&y_)[5]) {
        if (tid < ldy / 4) {                                    // the zero row the padding taps read
            *reinterpret_cast<uint2 *>(Y0 + kConvRows * ldy + 4 * tid) = make_uint2(0u, 0u);
            *reinterpret_cast<uint2 *>(Y1 + kConvRows * ldy + 4 * tid) = make_uint2(0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (m.has(k)) {
                const int off = m.row(k) * ldy + m.c;
                conv_split_store(Y0 + off, Y1 + off, y_[k]);
            }
        }
    };
    auto relu5 = [&](float4 (&y_)[5]) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            y_[k] = make_float4(relu_nan(y_[k].x), relu_nan(y_[k].y), relu_nan(y_[k].z), relu_nan(y_[k].w));
    };
    relu5(v);
    // ---- the shortcut
    if (down) {
        conv_acc_to_tile(w, T, ldt, acc);                       // the conv1 tile is in registers everywhere
        lds_barrier();
        tile_gn(res, p.gd, p.bd);
    } else {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            res[k] = (a < p.n_act && m.has(k)) ? *reinterpret_cast<const float4 *>(p.x + (a * p.lout + m.l(k)) * p.c + m.c)
                                               : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    to_planes(v);                                               // relu(GN1(conv1 x))
    lds_barrier();
    // ---- conv2 on the intermediate, GN2, + shortcut, ReLU
    conv_mid(p.w2);
    lds_barrier();                                              // the planes are done with: the tile takes their place
    conv_acc_to_tile(w, T, ldt, acc);
    lds_barrier();
    tile_gn(v, p.g2, p.b2);
    auto add_res_relu = [&]() {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const bool live = m.has(k);
            v[k] = make_float4(live ? relu_nan(v[k].x + res[k].x) : 0.f, live ? relu_nan(v[k].y + res[k].y) : 0.f,
                               live ? relu_nan(v[k].z + res[k].z) : 0.f, live ? relu_nan(v[k].w + res[k].w) : 0.f);
        }
    };
    auto store_out = [&]() {
        if (a < p.n_act) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (m.has(k)) *reinterpret_cast<float4 *>(p.out + (a * p.lout + m.l(k)) * p.c + m.c) = v[k];
        }
    };
    add_res_relu();
    if (!chain) { store_out(); return; }
    // ---- the chained block (identity shortcut = the values this thread holds)
    to_planes(v);
#pragma unroll
    for (int k = 0; k < 5; ++k) res[k] = v[k];
    lds_barrier();
    conv_mid(p.w1b);
    lds_barrier();
    conv_acc_to_tile(w, T, ldt, acc);
    lds_barrier();
    tile_gn(v, p.g1b, p.b1b);
    relu5(v);
    to_planes(v);
    lds_barrier();
    conv_mid(p.w2b);
    lds_barrier();
    conv_acc_to_tile(w, T, ldt, acc);
    lds_barrier();
    tile_gn(v, p.g2b, p.b2b);
    add_res_relu();
    store_out();
}

}  // namespace lgcn

using namespace lgcn;

template <bool SAVE, bool F32 = false>
static int conv1d_gn_launch(const float *x, int64_t n_act, int lin, int cin, const void *wp, int cout, int ks, int stride,
                            const float *gamma, const float *beta, float eps, const float *res, int res_mode, int relu,
                            float *out, float *y, void *stream) {
    if (n_act < 0 || res_mode < 0 || res_mode > 2) return LGCN_EINVAL;
    const int pad = (ks - 1) / 2;
    const int lout = stride > 0 ? (lin + 2 * pad - ks) / stride + 1 : 0;
    if (!conv_shape_ok(cin, cout, ks, stride, lin, lout)) return LGCN_ESHAPE;
    if (res_mode == 2 && (lout & 1)) return LGCN_ESHAPE;
    if (n_act == 0) return LGCN_OK;
    if (n_act > 0x7fffffff / (kConvRows * 128)) return LGCN_ESHAPE;
    const void *al[] = {x, wp, gamma, beta, out};
    for (const void *v : al) { LGCN_CHECK_PTR(v); LGCN_CHECK_ALIGN16(v); }
    if (res_mode != 0) { LGCN_CHECK_PTR(res); LGCN_CHECK_ALIGN16(res); }
    if (SAVE) { LGCN_CHECK_PTR(y); LGCN_CHECK_ALIGN16(y); }
    ConvParams p;
    p.x = x; p.n_act = n_act; p.lin = lin; p.cin = cin; p.cout = cout; p.ks = ks; p.stride = stride; p.lout = lout;
    p.wp = reinterpret_cast<const uint4 *>(wp); p.gamma = gamma; p.beta = beta; p.eps = eps;
    p.res = res; p.res_mode = res_mode; p.relu = relu; p.out = out; p.y = y;
    const int na = kConvRows / lout;
    const size_t lds_planes = conv_lds_in_planes(na, lin, cin), lds_tile = conv_lds_tile(cout);
    const size_t lds = lds_planes > lds_tile ? lds_planes : lds_tile;
    void (*kern)(ConvParams) = k_conv_gn<0, 0, SAVE, F32>;
    const int nkc = conv_kpad(cin) >> 5;
    if (ks == 1) kern = nkc == 1 ? k_conv_gn<1, 1, SAVE, F32> : nkc == 2 ? k_conv_gn<1, 2, SAVE, F32> : nkc == 4 ? k_conv_gn<1, 4, SAVE, F32> : kern;
    if (ks == 3) kern = nkc == 1 ? k_conv_gn<3, 1, SAVE, F32> : nkc == 2 ? k_conv_gn<3, 2, SAVE, F32> : nkc == 4 ? k_conv_gn<3, 4, SAVE, F32> : kern;
    const int rc = set_lds(reinterpret_cast<const void *>(kern), lds);
    if (rc != LGCN_OK) return rc;
    const unsigned grid = (unsigned)((n_act + na - 1) / na);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, (hipStream_t)stream, p);
    return launch_status();
}

// bytes of a packed image, fp16 planes or fp32 halves alike: per tap, K chunk and channel block 2 x 64 x 16
static int64_t conv_packed_bytes(int cin, int cout, int ks) {
    if (!conv_weight_ok(cin, cout, ks)) return LGCN_EINVAL;
    return (int64_t)ks * (conv_kpad(cin) / 32) * (cout / 16) * 2 * 64 * 16;
}

extern "C" {

int64_t lgcn_conv_packed_bytes(int cin, int cout, int ks) { return conv_packed_bytes(cin, cout, ks); }

int lgcn_conv_pack_weight(const float *w, int cin, int cout, int ks, void *out, void *stream) {
    const int64_t nbytes = conv_packed_bytes(cin, cout, ks);
    if (nbytes < 0) return LGCN_EINVAL;
    LGCN_CHECK_PTR(w); LGCN_CHECK_PTR(out); LGCN_CHECK_ALIGN16(out);
    const int64_t total = nbytes / 32;                          // one thread per lane: a uint4 of either plane
    hipLaunchKernelGGL(k_conv_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, cout, cin, ks,
                       reinterpret_cast<uint4 *>(out));
    return launch_status();
}

int lgcn_conv1d_gn(const float *x, int64_t n_act, int lin, int cin, const void *wp, int cout, int ks, int stride,
                   const float *gamma, const float *beta, float eps, const float *res, int res_mode, int relu,
                   float *out, void *stream) {
    return conv1d_gn_launch<false>(x, n_act, lin, cin, wp, cout, ks, stride, gamma, beta, eps, res, res_mode, relu, out,
                                   nullptr, stream);
}

int lgcn_conv1d_gn_train(const float *x, int64_t n_act, int lin, int cin, const void *wp, int cout, int ks, int stride,
                         const float *gamma, const float *beta, float eps, const float *res, int res_mode, int relu,
                         float *out, float *y, void *stream) {
    return conv1d_gn_launch<true>(x, n_act, lin, cin, wp, cout, ks, stride, gamma, beta, eps, res, res_mode, relu, out, y,
                                  stream);
}

// Exact-fp32 unit (reference layers.py:40-62 Conv1d, 142-190 Res1d's two halves; lanegcn.py:212-263): lgcn_conv1d_gn's
// contract on v_mfma_f32_16x16x4_f32.
int64_t lgcn_conv_packed_f32_bytes(int cin, int cout, int ks) { return conv_packed_bytes(cin, cout, ks); }

int lgcn_conv_pack_weight_f32(const float *w, int cin, int cout, int ks, void *out, void *stream) {
    const int64_t nbytes = conv_packed_bytes(cin, cout, ks);
    if (nbytes < 0) return LGCN_EINVAL;
    LGCN_CHECK_PTR(w); LGCN_CHECK_PTR(out); LGCN_CHECK_ALIGN16(out);
    const int64_t total = nbytes / 16;                          // one thread per float4
    hipLaunchKernelGGL(k_conv_pack_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, cout, cin,
                       ks, reinterpret_cast<float4 *>(out));
    return launch_status();
}

int lgcn_conv1d_gn_f32(const float *x, int64_t n_act, int lin, int cin, const void *wp, int cout, int ks, int stride,
                       const float *gamma, const float *beta, float eps, const float *res, int res_mode, int relu,
                       float *out, float *y, void *stream) {
    if (y != nullptr)
        return conv1d_gn_launch<true, true>(x, n_act, lin, cin, wp, cout, ks, stride, gamma, beta, eps, res, res_mode, relu,
                                            out, y, stream);
    return conv1d_gn_launch<false, true>(x, n_act, lin, cin, wp, cout, ks, stride, gamma, beta, eps, res, res_mode, relu, out,
                                         nullptr, stream);
}

static int res1d_launch(const float *x, int64_t n_act, int lin, int cin, int c, int stride, const void *w1p, const float *g1,
                        const float *b1, const void *w2p, const float *g2, const float *b2, const void *wdp, const float *gd,
                        const float *bd, const void *const *second, float eps, float *out, void *stream) {
    if (n_act < 0) return LGCN_EINVAL;
    const int lout = stride > 0 ? (lin + 2 - 3) / stride + 1 : 0;
    if (!conv_shape_ok(cin, c, 3, stride, lin, lout) || (c & 31)) return LGCN_ESHAPE;
    if (wdp == nullptr && (cin != c || stride != 1)) return LGCN_ESHAPE;      // identity shortcut: same shape in and out
    if ((wdp == nullptr) != (gd == nullptr) || (wdp == nullptr) != (bd == nullptr)) return LGCN_EINVAL;
    if (n_act == 0) return LGCN_OK;
    if (n_act > 0x7fffffff / (kConvRows * 128)) return LGCN_ESHAPE;
    const void *al[] = {x, w1p, g1, b1, w2p, g2, b2, out};
    for (const void *v : al) { LGCN_CHECK_PTR(v); LGCN_CHECK_ALIGN16(v); }
    if (wdp != nullptr) { LGCN_CHECK_ALIGN16(wdp); LGCN_CHECK_ALIGN16(gd); LGCN_CHECK_ALIGN16(bd); }
    Res1dParams p;
    p.x = x; p.n_act = n_act; p.lin = lin; p.cin = cin; p.c = c; p.stride = stride; p.lout = lout;
    p.w1 = reinterpret_cast<const uint4 *>(w1p); p.w2 = reinterpret_cast<const uint4 *>(w2p); p.wd = reinterpret_cast<const uint4 *>(wdp);
    p.g1 = g1; p.b1 = b1; p.g2 = g2; p.b2 = b2; p.gd = gd; p.bd = bd; p.eps = eps; p.out = out;
    p.w1b = p.w2b = nullptr; p.g1b = p.b1b = p.g2b = p.b2b = nullptr;
    if (second != nullptr) {          // {w1p, g1, b1, w2p, g2, b2} of the chained block
        for (int i = 0; i < 6; ++i) { LGCN_CHECK_PTR(second[i]); LGCN_CHECK_ALIGN16(second[i]); }
        p.w1b = reinterpret_cast<const uint4 *>(second[0]); p.g1b = reinterpret_cast<const float *>(second[1]);
        p.b1b = reinterpret_cast<const float *>(second[2]); p.w2b = reinterpret_cast<const uint4 *>(second[3]);
        p.g2b = reinterpret_cast<const float *>(second[4]); p.b2b = reinterpret_cast<const float *>(second[5]);
    }
    const int na = kConvRows / lout;
    const size_t in_planes = conv_lds_in_planes(na, lin, cin), tile = conv_lds_tile(c), mid_planes = conv_lds_mid_planes(c);
    size_t lds = in_planes > tile ? in_planes : tile;          // one region, reused (see the kernel)
    lds = lds > mid_planes ? lds : mid_planes;
    const int rc = set_lds(reinterpret_cast<const void *>(k_res1d_gn), lds);
    if (rc != LGCN_OK) return rc;
    hipLaunchKernelGGL(k_res1d_gn, dim3((unsigned)((n_act + na - 1) / na)), dim3(512), lds, (hipStream_t)stream, p);
    return launch_status();
}

int lgcn_res1d_gn(const float *x, int64_t n_act, int lin, int cin, int c, int stride, const void *w1p, const float *g1,
                  const float *b1, const void *w2p, const float *g2, const float *b2, const void *wdp, const float *gd,
                  const float *bd, float eps, float *out, void *stream) {
    return res1d_launch(x, n_act, lin, cin, c, stride, w1p, g1, b1, w2p, g2, b2, wdp, gd, bd, nullptr, eps, out, stream);
}

int lgcn_res1d_pair_gn(const float *x, int64_t n_act, int lin, int cin, int c, int stride, const void *w1p, const float *g1,
                       const float *b1, const void *w2p, const float *g2, const float *b2, const void *wdp, const float *gd,
                       const float *bd, const void *w1q, const float *g1q, const float *b1q, const void *w2q, const float *g2q,
                       const float *b2q, float eps, float *out, void *stream) {
    const void *second[6] = {w1q, g1q, b1q, w2q, g2q, b2q};
    return res1d_launch(x, n_act, lin, cin, c, stride, w1p, g1, b1, w2p, g2, b2, wdp, gd, bd, second, eps, out, stream);
}

}  // extern "C"
