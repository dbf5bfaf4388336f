// Per-row bodies of graph construction, one copy for the per-scene kernels of
// lgcn_index.hip and the batch kernels of lgcn_graphbatch.hip: a row of the boolean square, an entry of the lane mask,
// the nearest allowed centre of a node with its heading test.  Compile with -ffp-contract=off (the Makefile does).
#pragma once
#include "lgcn_common.hpp"

namespace lgcn {

// ------------------------------------------------------------ boolean square
// Row u of A * A (reference data.py:520-534, `mat * mat`): the distinct columns of the rows A[v], v in A[u], ascending.
// The entries of A[u] are col[e0 .. e1); row_of(v) is the CSR row of node v, or < 0 for an entry to be ignored.  Rows may
// be unsorted and hold duplicates.  Nothing is buffered, so no row has a capacity: each step takes the smallest candidate
// above the last one taken (candidates x result entries reads; lane graphs branch rarely: a row of A^32 has a handful).
constexpr int64_t kSqNone = INT64_MAX;

template <typename RowOf>
__device__ __forceinline__ int64_t sq_next_col(const int32_t *rowptr, const int32_t *col, int e0, int e1, RowOf row_of,
                                               int64_t after) {
    int64_t best = kSqNone;
    for (int e = e0; e < e1; ++e) {
        const int r = row_of(col[e]);
        if (r < 0) continue;
        int f = rowptr[r];
        const int f1 = rowptr[r + 1];
        for (; f + 4 <= f1; f += 4) {                           // four loads in flight: a long row is latency-bound
            const int64_t w0 = col[f], w1 = col[f + 1], w2 = col[f + 2], w3 = col[f + 3];
            if (w0 > after && w0 < best) best = w0;
            if (w1 > after && w1 < best) best = w1;
            if (w2 > after && w2 < best) best = w2;
            if (w3 > after && w3 < best) best = w3;
        }
        for (; f < f1; ++f) {
            const int64_t w = col[f];
            if (w > after && w < best) best = w;
        }
    }
    return best;
}

// Returns the length of the row; with out != nullptr the first `cap` entries are written (cap = the room the caller
// counted for this row: a write beyond it is dropped, never made).
template <typename RowOf>
__device__ __forceinline__ int sq_merge_row(const int32_t *rowptr, const int32_t *col, int e0, int e1, RowOf row_of,
                                            int32_t *out, int cap) {
    int k = 0;
    for (int64_t w = sq_next_col(rowptr, col, e0, e1, row_of, INT64_MIN); w != kSqNone;
         w = sq_next_col(rowptr, col, e0, e1, row_of, w)) {
        if (out != nullptr && k < cap) out[k] = (int32_t)w;
        ++k;
    }
    return k;
}

// ------------------------------------------------------------ left / right
// Lane-level mask (reference preprocess_data.py:318-327 / :356-360): mat = (S pre + S suc + S) > 0.5 with S, pre, suc the
// 0/1 matrices of the side pairs and the predecessor / successor lane pairs: mat[a][b] = S[a][b] or exists c: S[a][c] and
// (pre[c][b] or suc[c][b]).  Work item t of n_side * (n_pre + n_suc + 1).
__device__ __forceinline__ void lane_mask_item(const int64_t *side, int64_t n_side, const int64_t *pre, int64_t n_pre,
                                               const int64_t *suc, int64_t n_suc, int num_lanes, uint8_t *mat, int64_t t) {
    const int64_t per = n_pre + n_suc + 1;
    if (t >= n_side * per) return;
    const int64_t i = t / per, j = t % per;
    const int64_t a = side[2 * i], c = side[2 * i + 1];
    if (a < 0 || a >= num_lanes || c < 0 || c >= num_lanes) return;
    int64_t b = c;
    if (j > 0) {
        const int64_t *pp = j - 1 < n_pre ? pre + 2 * (j - 1) : suc + 2 * (j - 1 - n_pre);
        if (pp[0] != c) return;
        b = pp[1];
        if (b < 0 || b >= num_lanes) return;
    }
    mat[a * num_lanes + b] = 1;
}

// One wave per node h of a scene of n nodes (:329-347): over the nodes w whose lane is allowed for h's lane, the nearest
// centre (fp32 sub / mul / add / sqrt as ATen evaluates sqrt(((a - b) ** 2).sum(2)); the FIRST w among equals, as a CPU
// min(1) returns); kept when the distance is < cross_dist and the two segments' headings differ by < pi / 4.  Returns the
// partner w or -1, the same in every lane.
__device__ __forceinline__ int cross_partner(const float2 *ctrs, const float2 *feats, const int64_t *lane_idcs, int n,
                                             const uint8_t *mat, int num_lanes, float cross_dist, int h, int lane) {
    const float2 a = ctrs[h];
    const int64_t la = lane_idcs[h];
    const bool la_ok = la >= 0 && la < num_lanes;
    float best = 3.0e38f;
    int bw = 0x7fffffff;
    for (int w0 = 0; w0 < n; w0 += 64) {
        const int w = w0 + lane;
        if (w < n) {
            const int64_t lb = lane_idcs[w];
            const bool ok = la_ok && lb >= 0 && lb < num_lanes && mat[la * num_lanes + lb] != 0;
            float d = 1e6f;                                     // :332 masked entries
            if (ok) {
                const float2 c = ctrs[w];
                const float dx = __fsub_rn(a.x, c.x), dy = __fsub_rn(a.y, c.y);
                d = __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
            }
            if (d < best) { best = d; bw = w; }                 // ascending w per lane: the first of equals stays
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int ow = __shfl_xor(bw, off, 64);
        if (ob < best || (ob == best && ow < bw)) { best = ob; bw = ow; }
    }
    int out = -1;
    if (best < cross_dist && bw < n) {
        const float2 f1 = feats[h], f2 = feats[bw];
        const float t1 = atan2f(f1.y, f1.x), t2 = atan2f(f2.y, f2.x);
        float dt = fabsf(__fsub_rn(t1, t2));
        if (dt > 3.14159274101257324f) dt = fabsf(__fsub_rn(dt, 6.28318548202514648f));      // float32(pi), float32(2 pi)
        if (dt < 0.785398185253143311f) out = bw;                                            // float32(pi / 4)
    }
    return out;
}

}  // namespace lgcn
