// Graph construction for a BATCH of scenes: the dilated scales of pre / suc (reference data.py:520-534) and the left /
// right node adjacency (preprocess_data.py:287-392, cross_angle = None), from flat arrays plus per-scene offset tables.
// Scenes are independent graphs: the batch's adjacency is block-diagonal, so its boolean square is the blocks' squares,
// and a node looks for its partner among its own scene's nodes only.  See include/lgcn.h and DESIGN.md section 3.11.
//
// The per-row bodies are those of the per-scene kernels (lgcn_graphops.hpp), so both paths give the same integers.  Order
// comes from block scans plus per-block totals (lgcn_blockscan.hpp); this file adds no atomic (the scale-0 CSR is built by
// lgcn_csr_build, which sorts its rows).
#include "lgcn_common.hpp"
#include "lgcn_blockscan.hpp"
#include "lgcn_graphops.hpp"

namespace lgcn {

// `value` is the exclusive prefix in front of item i of the stacked space 2 x n (relation or side, then scene base +
// node): recorded in bounds [2][S + 1] for every scene that begins at i (empty scenes share a beginning) and at both ends.
__device__ __forceinline__ void gb_bounds(const int32_t *node_off, int S, int n, int i, int value, int32_t *bounds) {
    if (i < 2 * n) {
        const int r = i >= n ? 1 : 0, g = i - r * n;
        for (int s = find_seg(node_off, S, g); s >= 0 && node_off[s] == g; --s) bounds[r * (S + 1) + s] = value;
    }
    if (i == n || i == 2 * n) {
        const int r = i / n - 1;
        for (int s = S; s >= 0 && node_off[s] == n; --s) bounds[r * (S + 1) + s] = value;
    }
}

// ------------------------------------------------------------------ dilation
struct GbDilWs {
    int32_t *loc, *sums, *csr;       // [2 N + 1], [blocks], lgcn_csr_ws_elems(2 N, 1)
    int64_t *u, *v;                  // [n_pre + n_suc] re-based scale-0 edges
    int64_t total;
};
__host__ __device__ inline GbDilWs gb_dil_ws(int32_t *ws, int64_t n_nodes, int64_t n_edges, int64_t n_csr) {
    GbDilWs w;
    int64_t o = 0;
    w.loc = ws + o; o += up4(2 * n_nodes + 1);
    w.sums = ws + o; o += up4(sc_blocks(2 * n_nodes + 1));
    w.csr = ws + o; o += up4(n_csr);
    w.u = reinterpret_cast<int64_t *>(ws + o); o += up4(2 * n_edges);
    w.v = reinterpret_cast<int64_t *>(ws + o); o += up4(2 * n_edges);
    w.total = o;
    return w;
}

// One thread per scale-0 edge of either relation: row = relation * N + scene base + u, column = scene base + v; an edge
// with an end outside its scene's [0, n) becomes (-1, -1), which lgcn_csr_build drops.
__global__ __launch_bounds__(kScThreads) void k_gb_rebase(const lgcn_dilate_batch_t p, const GbDilWs w) {
    const int64_t e = (int64_t)blockIdx.x * kScThreads + threadIdx.x;
    if (e >= p.n_pre + p.n_suc) return;
    const int S = p.n_scenes, r = e >= p.n_pre ? 1 : 0;
    const int le = (int)(e - (r ? p.n_pre : 0));
    const int32_t *node_off = p.off_dev, *edge_off = p.off_dev + (1 + r) * (S + 1);
    const int s = find_seg(edge_off, S, le);
    const int lo = node_off[s], n = node_off[s + 1] - lo;
    const int64_t u = (r ? p.suc_u : p.pre_u)[le], v = (r ? p.suc_v : p.pre_v)[le];
    const bool ok = u >= 0 && u < n && v >= 0 && v < n;
    w.u[e] = ok ? r * p.n_nodes + lo + u : -1;
    w.v[e] = ok ? lo + v : -1;
}

// Row i of the stacked CSR (2 N rows): its relation's first row, its node g and its scene's node range [lo, hi).
struct GbRow {
    int rel_base, g, lo, hi;
};
__device__ __forceinline__ GbRow gb_row(const lgcn_dilate_batch_t &p, int i) {
    const int N = (int)p.n_nodes;
    GbRow q;
    q.rel_base = i >= N ? N : 0;
    q.g = i - q.rel_base;
    const int s = find_seg(p.off_dev, p.n_scenes, q.g);
    q.lo = p.off_dev[s];
    q.hi = p.off_dev[s + 1];
    return q;
}

// One thread per row (see sq_merge_row): the exact length of the row of A * A, scanned inside the block.
__global__ __launch_bounds__(kScThreads) void k_gb_sq_count(const lgcn_dilate_batch_t p, const GbDilWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int NR = 2 * (int)p.n_nodes;
    const int i = blockIdx.x * kScThreads + threadIdx.x;
    int v[1] = {0};
    if (i < NR) {
        const GbRow q = gb_row(p, i);
        const auto row_of = [q](int x) { return x >= q.lo && x < q.hi ? q.rel_base + x : -1; };
        v[0] = sq_merge_row(p.rowptr, p.col, p.rowptr[i], p.rowptr[i + 1], row_of, nullptr, 0);
    }
    int excl[1];
    sc_scan_local<1>(v, excl, w.sums, lds);
    if (i <= NR) w.loc[i] = excl[0];
}

// The new row pointer, and its value at the scene boundaries of both relations (what the host reads back).
__global__ __launch_bounds__(kScThreads) void k_gb_sq_rowptr(const lgcn_dilate_batch_t p, const GbDilWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int N = (int)p.n_nodes;
    const int i = blockIdx.x * kScThreads + threadIdx.x;
    int base[1];
    sc_block_base<1>(w.sums, base, lds);
    if (i > 2 * N) return;
    const int o = base[0] + w.loc[i];
    p.out_rowptr[i] = o;
    gb_bounds(p.off_dev, p.n_scenes, N, i, o, p.bounds);
}

// The same merge again, written straight into the row's final place; u and v leave as scene-local int64.
__global__ __launch_bounds__(kScThreads) void k_gb_sq_fill(const lgcn_dilate_batch_t p) {
    const int i = blockIdx.x * kScThreads + threadIdx.x;
    if (i >= 2 * (int)p.n_nodes) return;
    const int b = p.out_rowptr[i], cap = p.out_rowptr[i + 1] - b;
    if (b < 0 || cap <= 0 || (int64_t)b + cap > p.nnz) return;
    const GbRow q = gb_row(p, i);
    const auto row_of = [q](int x) { return x >= q.lo && x < q.hi ? q.rel_base + x : -1; };
    int k = sq_merge_row(p.rowptr, p.col, p.rowptr[i], p.rowptr[i + 1], row_of, p.out_col + b, cap);
    if (k > cap) k = cap;
    for (int j = 0; j < k; ++j) {
        p.out_u[b + j] = q.g - q.lo;
        p.out_v[b + j] = p.out_col[b + j] - q.lo;
    }
}

// ------------------------------------------------------------------ left / right
// off_*: nine tables of S + 1: node, lane, pre, suc, left, right, mask, left work, right work
struct GbCrossWs {
    int32_t *partner, *loc, *sums;   // [2 N], [2 N + 1], [blocks]
    int64_t total;
};
__host__ __device__ inline GbCrossWs gb_cross_ws(int32_t *ws, int64_t n_nodes) {
    GbCrossWs w;
    int64_t o = 0;
    w.partner = ws + o; o += up4(2 * n_nodes);
    w.loc = ws + o; o += up4(2 * n_nodes + 1);
    w.sums = ws + o; o += up4(sc_blocks(2 * n_nodes + 1));
    w.total = o;
    return w;
}

// One scene's slice of the batch for one side (blockIdx.y: 0 = left, 1 = right).
struct GbScene {
    const int64_t *side, *pre, *suc;
    int n_side, n_pre, n_suc, num_lanes, node_lo, n_nodes;
    uint8_t *mat;
};
__device__ __forceinline__ GbScene gb_scene(const lgcn_cross_batch_t &p, int s, int side) {
    const int S1 = p.n_scenes + 1;
    const int32_t *node = p.off_dev, *lane = node + S1, *pre = lane + S1, *suc = pre + S1, *sd = suc + S1 * (1 + side),
                  *mask = node + 6 * S1;
    GbScene q;
    q.side = (side ? p.right_pairs : p.left_pairs) + 2 * (int64_t)sd[s];
    q.pre = p.pre_pairs + 2 * (int64_t)pre[s];
    q.suc = p.suc_pairs + 2 * (int64_t)suc[s];
    q.n_side = sd[s + 1] - sd[s];
    q.n_pre = pre[s + 1] - pre[s];
    q.n_suc = suc[s + 1] - suc[s];
    q.num_lanes = lane[s + 1] - lane[s];
    q.node_lo = node[s];
    q.n_nodes = node[s + 1] - node[s];
    q.mat = p.mat + (int64_t)side * mask[p.n_scenes] + mask[s];
    return q;
}

// k_lane_mask per scene: a thread finds its scene in the side's work-offset table.
__global__ __launch_bounds__(kScThreads) void k_gb_lane_mask(const lgcn_cross_batch_t p) {
    const int side = blockIdx.y, S = p.n_scenes;
    const int32_t *work = p.off_dev + (7 + side) * (S + 1);
    const int64_t t = (int64_t)blockIdx.x * kScThreads + threadIdx.x;
    if (t >= work[S]) return;
    const int s = find_seg(work, S, (int)t);
    const GbScene q = gb_scene(p, s, side);
    lane_mask_item(q.side, q.n_side, q.pre, q.n_pre, q.suc, q.n_suc, q.num_lanes, q.mat, t - work[s]);
}

// k_cross_edges per scene: one wave per node of the batch, which scans its own scene's nodes only.  A scene whose side
// list is empty has no edge on that side (the reference's `len(pairs) > 0` branch).
__global__ __launch_bounds__(kScThreads) void k_gb_partner(const lgcn_cross_batch_t p, const GbCrossWs w) {
    const int side = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t h = (int64_t)blockIdx.x * (kScThreads >> 6) + (threadIdx.x >> 6);
    if (h >= p.n_nodes) return;
    const GbScene q = gb_scene(p, find_seg(p.off_dev, p.n_scenes, (int)h), side);
    int out = -1;
    if (q.n_side > 0)
        out = cross_partner(reinterpret_cast<const float2 *>(p.ctrs) + q.node_lo, reinterpret_cast<const float2 *>(p.feats) + q.node_lo,
                            p.lane_idcs + q.node_lo, q.n_nodes, q.mat, q.num_lanes, p.cross_dist, (int)h - q.node_lo, lane);
    if (lane == 0) w.partner[side * p.n_nodes + h] = out;
}

// The compaction that torch.nonzero did per scene: kept nodes in (side, scene, node) order.
__global__ __launch_bounds__(kScThreads) void k_gb_cross_flag(const lgcn_cross_batch_t p, const GbCrossWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int i = blockIdx.x * kScThreads + threadIdx.x;
    int v[1] = {i < 2 * (int)p.n_nodes && w.partner[i] >= 0 ? 1 : 0};
    int excl[1];
    sc_scan_local<1>(v, excl, w.sums, lds);
    if (i <= 2 * (int)p.n_nodes) w.loc[i] = excl[0];
}

__global__ __launch_bounds__(kScThreads) void k_gb_cross_fill(const lgcn_cross_batch_t p, const GbCrossWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int N = (int)p.n_nodes;
    const int i = blockIdx.x * kScThreads + threadIdx.x;
    int base[1];
    sc_block_base<1>(w.sums, base, lds);
    if (i > 2 * N) return;
    const int o = base[0] + w.loc[i];
    gb_bounds(p.off_dev, p.n_scenes, N, i, o, p.counts);
    if (i == 2 * N || w.partner[i] < 0 || o >= 2 * N) return;
    const int h = i >= N ? i - N : i;
    const int lo = p.off_dev[find_seg(p.off_dev, p.n_scenes, h)];
    p.out_u[o] = (int16_t)(h - lo);          // the low 16 bits, as .astype(np.int16) keeps them
    p.out_v[o] = (int16_t)w.partner[i];
}

// ------------------------------------------------------------------ host side
constexpr int64_t kGbMaxNodes = 0x3ffffff0;        // 2 N + 1 rows must fit an int
constexpr int64_t kGbMaxEdges = 0x0ffffff0;        // 4 int32 of workspace per edge

// stage 0: lgcn_dilate_batch_csr, 1: .._count, 2: .._fill
static int gb_dilate_validate(const lgcn_dilate_batch_t *p, int stage) {
    if (p == nullptr) return LGCN_EINVAL;
    if (p->n_scenes < 0 || p->n_nodes < 0 || p->n_pre < 0 || p->n_suc < 0) return LGCN_EINVAL;
    if (p->n_scenes == 0) return (p->n_nodes | p->n_pre | p->n_suc) ? LGCN_EINVAL : LGCN_OK;
    if (p->n_scenes > 0x7fffffff / 16 || p->n_nodes > kGbMaxNodes || p->n_pre > kGbMaxEdges || p->n_suc > kGbMaxEdges ||
        p->n_pre + p->n_suc > kGbMaxEdges)
        return LGCN_ESHAPE;
    LGCN_CHECK_PTR(p->off_host);
    const int S = p->n_scenes;
    if (int rc = check_table(p->off_host, S, p->n_nodes)) return rc;
    if (int rc = check_table(p->off_host + (S + 1), S, p->n_pre)) return rc;
    if (int rc = check_table(p->off_host + 2 * (S + 1), S, p->n_suc)) return rc;
    LGCN_CHECK_PTR(p->off_dev); LGCN_CHECK_PTR(p->ws); LGCN_CHECK_PTR(p->rowptr); LGCN_CHECK_PTR(p->col);
    if (stage == 0) {
        if (p->n_pre > 0) { LGCN_CHECK_PTR(p->pre_u); LGCN_CHECK_PTR(p->pre_v); }
        if (p->n_suc > 0) { LGCN_CHECK_PTR(p->suc_u); LGCN_CHECK_PTR(p->suc_v); }
    } else {
        LGCN_CHECK_PTR(p->out_rowptr); LGCN_CHECK_PTR(p->bounds);
    }
    if (stage == 2) {
        if (p->nnz < 0) return LGCN_EINVAL;
        if (p->nnz > 0x7fffffff) return LGCN_ESHAPE;
        if (p->nnz > 0) { LGCN_CHECK_PTR(p->out_col); LGCN_CHECK_PTR(p->out_u); LGCN_CHECK_PTR(p->out_v); }
    }
    LGCN_CHECK_ALIGN16(p->ws);
    const void *words[] = {p->off_dev, p->rowptr, p->col, p->out_rowptr, p->bounds, p->out_col};
    for (const void *q : words)
        if (misaligned(q, 3u)) return LGCN_EALIGN;
    const void *dwords[] = {p->pre_u, p->pre_v, p->suc_u, p->suc_v, p->out_u, p->out_v};
    for (const void *q : dwords)
        if (misaligned(q, 7u)) return LGCN_EALIGN;
    return LGCN_OK;
}

static int gb_cross_validate(const lgcn_cross_batch_t *p) {
    if (p == nullptr) return LGCN_EINVAL;
    const int64_t totals[] = {p->n_nodes, p->n_lanes, p->n_pre, p->n_suc, p->n_left, p->n_right};
    if (p->n_scenes < 0) return LGCN_EINVAL;
    for (int64_t t : totals)
        if (t < 0) return LGCN_EINVAL;
    if (!(p->cross_dist == p->cross_dist)) return LGCN_EINVAL;
    if (p->n_scenes == 0) {
        for (int64_t t : totals)
            if (t != 0) return LGCN_EINVAL;
        return LGCN_OK;
    }
    if (p->n_scenes > 0x7fffffff / 16 || p->n_nodes > kGbMaxNodes) return LGCN_ESHAPE;
    for (int64_t t : totals)
        if (t > 0x7ffffff0) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(p->off_host);
    const int S = p->n_scenes, S1 = S + 1;
    const int32_t *off = p->off_host;
    for (int k = 0; k < 6; ++k)
        if (int rc = check_table(off + k * S1, S, totals[k])) return rc;
    // the mask and work tables must be what the first six imply: a bad entry never becomes an address
    int64_t mask = 0, work[2] = {0, 0};
    for (int s = 0; s <= S; ++s) {
        if (off[6 * S1 + s] != mask || off[7 * S1 + s] != work[0] || off[8 * S1 + s] != work[1]) return LGCN_EINVAL;
        if (s == S) break;
        const int64_t L = off[S1 + s + 1] - off[S1 + s];
        const int64_t per = (int64_t)(off[2 * S1 + s + 1] - off[2 * S1 + s]) + (off[3 * S1 + s + 1] - off[3 * S1 + s]) + 1;
        mask += L * L;
        work[0] += (off[4 * S1 + s + 1] - off[4 * S1 + s]) * per;
        work[1] += (off[5 * S1 + s + 1] - off[5 * S1 + s]) * per;
        if (2 * mask > 0x7ffffff0 || work[0] > 0x7ffffff0 || work[1] > 0x7ffffff0) return LGCN_ESHAPE;
    }
    LGCN_CHECK_PTR(p->off_dev); LGCN_CHECK_PTR(p->ws); LGCN_CHECK_PTR(p->counts);
    if (p->n_nodes > 0) {
        LGCN_CHECK_PTR(p->ctrs); LGCN_CHECK_PTR(p->feats); LGCN_CHECK_PTR(p->lane_idcs); LGCN_CHECK_PTR(p->out_u);
        LGCN_CHECK_PTR(p->out_v);
    }
    if (mask > 0) LGCN_CHECK_PTR(p->mat);
    if (p->n_pre > 0) LGCN_CHECK_PTR(p->pre_pairs);
    if (p->n_suc > 0) LGCN_CHECK_PTR(p->suc_pairs);
    if (p->n_left > 0) LGCN_CHECK_PTR(p->left_pairs);
    if (p->n_right > 0) LGCN_CHECK_PTR(p->right_pairs);
    LGCN_CHECK_ALIGN16(p->ws);
    const void *dwords[] = {p->ctrs, p->feats, p->lane_idcs, p->pre_pairs, p->suc_pairs, p->left_pairs, p->right_pairs};
    for (const void *q : dwords)
        if (misaligned(q, 7u)) return LGCN_EALIGN;
    if (misaligned(p->off_dev, 3u) || misaligned(p->counts, 3u) || misaligned(p->out_u, 1u) || misaligned(p->out_v, 1u))
        return LGCN_EALIGN;
    return LGCN_OK;
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int64_t lgcn_dilate_batch_ws_elems(int64_t n_nodes, int64_t n_edges) {
    if (n_nodes < 0 || n_edges < 0) return LGCN_EINVAL;
    if (n_nodes > kGbMaxNodes || n_edges > kGbMaxEdges) return LGCN_ESHAPE;
    const int64_t n_csr = lgcn_csr_ws_elems(2 * n_nodes, 1);
    if (n_csr < 0) return n_csr;
    const int64_t n = gb_dil_ws(nullptr, n_nodes, n_edges, n_csr).total;
    return n > 0x7fffffff ? (int64_t)LGCN_ESHAPE : n;
}

int lgcn_dilate_batch_csr(const lgcn_dilate_batch_t *p, void *stream) {
    if (int rc = gb_dilate_validate(p, 0)) return rc;
    if (p->n_nodes == 0) return LGCN_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_edges = p->n_pre + p->n_suc;
    if (lgcn_dilate_batch_ws_elems(p->n_nodes, n_edges) < 0) return LGCN_ESHAPE;
    const GbDilWs w = gb_dil_ws(p->ws, p->n_nodes, n_edges, lgcn_csr_ws_elems(2 * p->n_nodes, 1));
    if (n_edges > 0)
        hipLaunchKernelGGL(k_gb_rebase, dim3((unsigned)sc_blocks(n_edges)), dim3(kScThreads), 0, st, *p, w);
    const int64_t *u = w.u, *v = w.v;
    return lgcn_csr_build(&u, &v, &n_edges, 1, 2 * p->n_nodes, p->rowptr, p->col, w.csr, stream);
}

int lgcn_dilate_batch_count(const lgcn_dilate_batch_t *p, void *stream) {
    if (int rc = gb_dilate_validate(p, 1)) return rc;
    if (p->n_scenes == 0) return LGCN_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p->n_nodes == 0) {                     // every boundary is 0
        hipError_t e = hipMemsetAsync(p->bounds, 0, sizeof(int32_t) * 2 * ((size_t)p->n_scenes + 1), st);
        return e == hipSuccess ? LGCN_OK : (int)e;
    }
    if (lgcn_dilate_batch_ws_elems(p->n_nodes, p->n_pre + p->n_suc) < 0) return LGCN_ESHAPE;
    const GbDilWs w = gb_dil_ws(p->ws, p->n_nodes, p->n_pre + p->n_suc, lgcn_csr_ws_elems(2 * p->n_nodes, 1));
    const dim3 grid((unsigned)sc_blocks(2 * p->n_nodes + 1));
    hipLaunchKernelGGL(k_gb_sq_count, grid, dim3(kScThreads), 0, st, *p, w);
    hipLaunchKernelGGL(k_gb_sq_rowptr, grid, dim3(kScThreads), 0, st, *p, w);
    return launch_status();
}

int lgcn_dilate_batch_fill(const lgcn_dilate_batch_t *p, void *stream) {
    if (int rc = gb_dilate_validate(p, 2)) return rc;
    if (p->n_nodes == 0 || p->nnz == 0) return LGCN_OK;
    hipLaunchKernelGGL(k_gb_sq_fill, dim3((unsigned)sc_blocks(2 * p->n_nodes)), dim3(kScThreads), 0,
                       static_cast<hipStream_t>(stream), *p);
    return launch_status();
}

int64_t lgcn_cross_edges_batch_ws_elems(int64_t n_nodes) {
    if (n_nodes < 0) return LGCN_EINVAL;
    if (n_nodes > kGbMaxNodes / 4) return LGCN_ESHAPE;
    return gb_cross_ws(nullptr, n_nodes).total;
}

int lgcn_cross_edges_batch(const lgcn_cross_batch_t *p, void *stream) {
    if (int rc = gb_cross_validate(p)) return rc;
    if (p->n_scenes == 0) return LGCN_OK;
    if (lgcn_cross_edges_batch_ws_elems(p->n_nodes) < 0) return LGCN_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S1 = p->n_scenes + 1;
    const GbCrossWs w = gb_cross_ws(p->ws, p->n_nodes);
    if (p->n_nodes == 0) {                     // every count is 0
        hipError_t e = hipMemsetAsync(p->counts, 0, sizeof(int32_t) * 2 * (size_t)S1, st);
        return e == hipSuccess ? LGCN_OK : (int)e;
    }
    const int64_t mask = p->off_host[6 * S1 + p->n_scenes];
    const int64_t work = p->off_host[7 * S1 + p->n_scenes] > p->off_host[8 * S1 + p->n_scenes] ? p->off_host[7 * S1 + p->n_scenes]
                                                                                                  : p->off_host[8 * S1 + p->n_scenes];
    if (mask > 0) {
        hipError_t e = hipMemsetAsync(p->mat, 0, 2 * (size_t)mask, st);
        if (e != hipSuccess) return (int)e;
    }
    if (work > 0)
        hipLaunchKernelGGL(k_gb_lane_mask, dim3((unsigned)sc_blocks(work), 2), dim3(kScThreads), 0, st, *p);
    hipLaunchKernelGGL(k_gb_partner, dim3((unsigned)((p->n_nodes + 3) / 4), 2), dim3(kScThreads), 0, st, *p, w);
    const dim3 grid((unsigned)sc_blocks(2 * p->n_nodes + 1));
    hipLaunchKernelGGL(k_gb_cross_flag, grid, dim3(kScThreads), 0, st, *p, w);
    hipLaunchKernelGGL(k_gb_cross_fill, grid, dim3(kScThreads), 0, st, *p, w);
    return launch_status();
}

}  // extern "C"
