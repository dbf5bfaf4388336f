// Backward of the exact-fp32 row-block kernels of lgcn_rowmlp.hip: the weight gradient of a relation stage (k_wgrad) and
// four fused backward families -- Att pairs, LaneConv / LinearRes, LanePooling pairs, row blocks.  Each family is a
// 512-thread kernel that leaves one partial record per workgroup and one launch of k_rec_reduce, which sums the records
// in chunk order into the outputs that were asked for.
#include "lgcn_rowmlp.hpp"

namespace lgcn {

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

// ------------------------------------------------------ record reduce -----
// out = sum over the chunk records of a backward launch, in chunk order: the second launch of all four families below.
// A record is a run of 128-float rows.  Segment s of its layout covers the next nrows record rows, and element (i, c) of
// the segment goes to dst[i * ld + c * cs]; dst = nullptr: that output was not asked for, the segment is skipped.
struct RecSeg { float *dst; int nrows, ld, cs; };
constexpr int kRecSegs = 8;                               // Att: two matrices, five [128] vectors and d_wd0
struct RecLayout { float *dst[kRecSegs]; int nrows[kRecSegs], ld[kRecSegs], cs[kRecSegs]; };

inline RecSeg rec_mat(float *dw, int ld = kC) { return {dw, kC, ld, 1}; }     // 128 x 128, row stride ld
inline RecSeg rec_vec(float *v) { return {v, 1, 0, 1}; }                      // [128]
inline RecSeg rec_cols(float *w, int k) { return {w, k, 1, k}; }              // [128,k], record row j = column j

// The table of a record's segments in record order; RecSeg{} (no rows) stands for one that this launch's record lacks.
static RecLayout rec_layout(std::initializer_list<RecSeg> segs) {
    RecLayout L{};
    int s = 0;
    for (const RecSeg &g : segs) { L.dst[s] = g.dst; L.nrows[s] = g.nrows; L.ld[s] = g.ld; L.cs[s] = g.cs; ++s; }
    return L;
}

__global__ __launch_bounds__(256) void k_rec_reduce(const float *__restrict__ rec, int n_rec, int rec_floats, const RecLayout L) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    // A wave's 64 elements lie in one record row, so its segment is uniform: found by scalar compares and selects along the
    // unrolled table, never by indexing the kernel argument with a per-thread value (which would put the table in scratch).
    // Selects, not branches around the table's fields: the whole table is then fetched at once, in front of the chain.
    const int row = __builtin_amdgcn_readfirstlane(e >> 7), c = e & 127;
    float *dst = nullptr;
    int i = 0, ld = 0, cs = 0, r0 = 0;
#pragma unroll
    for (int s = 0; s < kRecSegs; ++s) {
        const int n = L.nrows[s];
        const bool hit = row >= r0 && row < r0 + n;
        dst = hit ? L.dst[s] : dst; i = hit ? row - r0 : i; ld = hit ? L.ld[s] : ld; cs = hit ? L.cs[s] : cs;
        r0 += n;
    }
    if (dst == nullptr || e >= rec_floats) return;      // a row past the last segment has no dst either
    float sum = 0.f;
    for (int k = 0; k < n_rec; ++k) sum += rec[(int64_t)k * rec_floats + e];
    dst[(int64_t)i * ld + c * cs] = sum;
}

static void launch_rec_reduce(const float *rec, int n_rec, int rec_floats, const RecLayout &L, hipStream_t st) {
    hipLaunchKernelGGL(k_rec_reduce, dim3((rec_floats + 255) / 256), dim3(256), 0, st, rec, n_rec, rec_floats, L);
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

}  // namespace lgcn

using namespace lgcn;

extern "C" {

static_assert(sizeof(lgcn_att_pairs_bwd_t) == 31 * 8,
              "lgcn_att_pairs_bwd_t layout: keep lanegcn-1_amd/_lib.py (AttPairsBwd) and tests/test_host_att_train_cabi.py in step");

// workgroups (and chunk records) of a backward launch over `rows` rows or pairs: never more than its 32-row tiles
static int64_t bwd_chunks(int64_t rows, int n_chunks) {
    const int64_t tiles = (rows + kTM32 - 1) / kTM32;
    return tiles < n_chunks ? tiles : n_chunks;
}

// The arguments every backward entry shares: LGCN_EINVAL for a negative row count or n_chunks outside 1..1024, else
// LGCN_ESHAPE for more than max_rows rows.
static int check_bwd_args(int64_t rows, int64_t max_rows, int n_chunks) {
    if (rows < 0 || n_chunks < 1 || n_chunks > 1024) return LGCN_EINVAL;
    return rows > max_rows ? LGCN_ESHAPE : LGCN_OK;
}

constexpr int64_t kMaxPairs = 0x7ffffff0, kMaxRows = 0x7fffffff;

int64_t lgcn_att_pairs_bwd_ws_elems(int64_t cap, int n_chunks) {
    if (check_bwd_args(cap, kMaxPairs, n_chunks) != LGCN_OK) return LGCN_EINVAL;
    return bwd_chunks(cap, n_chunks) * kPairRec;
}

int lgcn_att_pairs_bwd(const lgcn_att_pairs_bwd_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_att_pairs_bwd_t &a = *ph;
    const int rc = check_bwd_args(a.cap, kMaxPairs, a.n_chunks);
    if (rc != LGCN_OK || a.cap == 0) return rc;
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
    const int n_rec = (int)bwd_chunks(a.cap, a.n_chunks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_att_pairs_bwd, dim3(n_rec), dim3(512), 0, st, p);
    if (want_rec) {
        // Record: dW_d2 [128,128], dW_c0e [128,128], then seven [128] vectors: dgamma_c, dbeta_c, dgamma_d, dbeta_d, db_d0,
        // dW_d0[:,0], dW_d0[:,1].
        const RecLayout L = rec_layout({rec_mat(a.d_wd2), rec_mat(a.d_wc0e), rec_vec(a.d_gc), rec_vec(a.d_btc), rec_vec(a.d_gd),
                                        rec_vec(a.d_btd), rec_vec(a.d_bd0), rec_cols(a.d_wd0, 2)});
        launch_rec_reduce(a.ws, n_rec, kPairRec, L, st);
    }
    return launch_status();
}

static_assert(sizeof(lgcn_pool_pairs_bwd_t) == 23 * 8,
              "lgcn_pool_pairs_bwd_t layout: keep lanegcn-1_amd/_lib.py (PoolPairsBwd) and tests/test_host_pool_train_cabi.py in step");

int64_t lgcn_pool_pairs_bwd_ws_elems(int64_t cap, int n_chunks) {
    if (check_bwd_args(cap, kMaxPairs, n_chunks) != LGCN_OK) return LGCN_EINVAL;
    return bwd_chunks(cap, n_chunks) * kPoolRec;
}

int lgcn_pool_pairs_bwd(const lgcn_pool_pairs_bwd_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_pool_pairs_bwd_t &a = *ph;
    const int rc = check_bwd_args(a.cap, kMaxPairs, a.n_chunks);
    if (rc != LGCN_OK || a.cap == 0) return rc;
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
    const int n_rec = (int)bwd_chunks(a.cap, a.n_chunks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pool_pairs_bwd, dim3(n_rec), dim3(512), 0, st, p);
    if (want_rec) {
        // Record: dW_0h [128,128], then seven [128] vectors: dgamma, dbeta, db_p, dW_p[:,0], dW_p[:,1], dW_p[:,2], dW_p[:,3].
        const RecLayout L = rec_layout({rec_mat(a.d_w0h), rec_vec(a.d_g), rec_vec(a.d_bt), rec_vec(a.d_bp), rec_cols(a.d_wp, 4)});
        launch_rec_reduce(a.ws, n_rec, kPoolRec, L, st);
    }
    return launch_status();
}

static_assert(sizeof(lgcn_laneconv_bwd_t) == 23 * 8,
              "lgcn_laneconv_bwd_t layout: keep lanegcn-1_amd/_lib.py (LaneConvBwd) and tests/test_host_laneconv_bwd_cabi.py in step");

int64_t lgcn_laneconv_bwd_ws_elems(int64_t n_rows, int n_chunks, int ident1) {
    if (check_bwd_args(n_rows, kMaxRows, n_chunks) != LGCN_OK || (ident1 != 0 && ident1 != 1)) return LGCN_EINVAL;
    return bwd_chunks(n_rows, n_chunks) * lc_rec_floats(ident1 != 0);
}

int lgcn_laneconv_bwd(const lgcn_laneconv_bwd_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_laneconv_bwd_t &a = *ph;
    if (a.ident1 != 0 && a.ident1 != 1) return LGCN_EINVAL;
    const int rc = check_bwd_args(a.n_rows, kMaxRows, a.n_chunks);
    if (rc != LGCN_OK || a.n_rows == 0) return rc;
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
    const int n_rec = (int)bwd_chunks(a.n_rows, a.n_chunks);
    hipStream_t st = (hipStream_t)stream;
    if (ident1) hipLaunchKernelGGL(k_lc_bwd_rows<true>, dim3(n_rec), dim3(512), 0, st, p);
    else hipLaunchKernelGGL(k_lc_bwd_rows<false>, dim3(n_rec), dim3(512), 0, st, p);
    if (want_rec) {
        // Record: dW2 [128,128], dW1 [128,128] (ident1 only), then four [128] vectors: dgamma2, dbeta2, dgamma1, dbeta1.
        const RecLayout L = rec_layout({rec_mat(a.d_w2), ident1 ? rec_mat(a.d_w1) : RecSeg{}, rec_vec(a.d_g2), rec_vec(a.d_b2),
                                        rec_vec(a.d_g1), rec_vec(a.d_b1)});
        launch_rec_reduce(a.ws, n_rec, lc_rec_floats(ident1), L, st);
    }
    return launch_status();
}

static_assert(sizeof(lgcn_rowblock_bwd_t) == 20 * 8,
              "lgcn_rowblock_bwd_t layout: keep lanegcn-1_amd/_lib.py (RowBlockBwd) and tests/test_host_rowblock_bwd_cabi.py in step");

int64_t lgcn_rowblock_bwd_ws_elems(int64_t n_rows, int n_chunks, int n_rel) {
    if (check_bwd_args(n_rows, kMaxRows, n_chunks) != LGCN_OK || n_rel < 1 || n_rel > 2) return LGCN_EINVAL;
    return bwd_chunks(n_rows, n_chunks) * rb_rec_floats(n_rel);
}

int lgcn_rowblock_bwd(const lgcn_rowblock_bwd_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_rowblock_bwd_t &a = *ph;
    if (a.n_rows > kMaxRows) return LGCN_ESHAPE;      // this entry reports the row count before n_rel and n_chunks
    if (check_bwd_args(a.n_rows, kMaxRows, a.n_chunks) != LGCN_OK || a.n_rel < 1 || a.n_rel > 2) return LGCN_EINVAL;
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
    for (int r = 0; r < n_rel; ++r) {
        p.src[r] = a.src[r]; p.wpt[r] = a.wpt[r]; p.d_src[r] = a.d_src[r]; p.want_w[r] = a.d_w[r] != nullptr;
    }
    p.d_res = a.d_res; p.rec = want_rec ? a.ws : nullptr;
    p.n_rows = a.n_rows; p.eps = a.eps; p.want_gn = a.d_gamma || a.d_beta;
    const int n_rec = (int)bwd_chunks(a.n_rows, a.n_chunks);
    hipStream_t st = (hipStream_t)stream;
    if (n_rel == 2) {
        if (gn) hipLaunchKernelGGL((k_rb_bwd_rows<2, true>), dim3(n_rec), dim3(512), 0, st, p);
        else hipLaunchKernelGGL((k_rb_bwd_rows<2, false>), dim3(n_rec), dim3(512), 0, st, p);
    } else {
        if (gn) hipLaunchKernelGGL((k_rb_bwd_rows<1, true>), dim3(n_rec), dim3(512), 0, st, p);
        else hipLaunchKernelGGL((k_rb_bwd_rows<1, false>), dim3(n_rec), dim3(512), 0, st, p);
    }
    if (want_rec) {
        // Record: dW_0 [128,128], dW_1 [128,128] (two relations only), then dgamma, dbeta [128]; dW_r goes out with row stride
        // ld_w[r] (a 128-column block of a wider weight gradient).
        const RecLayout L = rec_layout({rec_mat(a.d_w[0], a.ld_w[0]), n_rel == 2 ? rec_mat(a.d_w[1], a.ld_w[1]) : RecSeg{},
                                        rec_vec(a.d_gamma), rec_vec(a.d_beta)});
        launch_rec_reduce(a.ws, n_rec, rb_rec_floats(n_rel), L, st);
    }
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
