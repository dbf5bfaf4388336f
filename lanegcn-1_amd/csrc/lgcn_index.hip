// Integer path of the LaneGCN hot path: graph_gather offsets, tile-major CSR
// plan, distance-gated pair search.  Everything here is bit-exact against the
// reference (lanegcn.py:171-209, 672-689); this file is compiled with
// -ffp-contract=off so the pair-search distance is evaluated exactly like
// ATen's sub / pow(2) / sum / sqrt / le chain (no FMA).  The scans and the
// segment search are those of lgcn_blockscan.hpp.
#include "lgcn_common.hpp"
#include "lgcn_blockscan.hpp"
#include "lgcn_graphops.hpp"

namespace lgcn {

// -------------------------------------------------------- graph_gather ----
__global__ __launch_bounds__(256) void k_graph_gather(const int64_t *in, int64_t n,
                                                      const int64_t *seg_off, const int64_t *seg_base,
                                                      int n_seg, int64_t *out64, int32_t *out32) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = in[e] + seg_base[find_seg(seg_off, n_seg, e)];
        if (out64) out64[e] = v;
        if (out32) out32[e] = (int32_t)v;
    }
}

// ----------------------------------------------------------- CSR plan -----
struct CooTable {
    const int64_t *u[LGCN_MAX_REL];
    const int64_t *v[LGCN_MAX_REL];
    int64_t start[LGCN_MAX_REL + 1];  // prefix of n_edges
    int n_rel;
    int64_t n_nodes;
};

__device__ __forceinline__ int64_t csr_key(int64_t n, int r, int n_rel) {
    return ((n >> 4) * n_rel + r) * 16 + (n & 15);
}

// pass 0: count, pass 1: fill
template <int PASS>
__global__ __launch_bounds__(256) void k_csr_edges(const CooTable t, int32_t *cnt_or_cursor,
                                                   const int32_t *rowptr, int32_t *col) {
    const int64_t total = t.start[t.n_rel];
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        int r = 0;
        while (r + 1 < t.n_rel && e >= t.start[r + 1]) ++r;
        const int64_t le = e - t.start[r];
        const int64_t u = t.u[r][le], v = t.v[r][le];
        if (u < 0 || u >= t.n_nodes || v < 0 || v >= t.n_nodes) continue;  // never index out of bounds
        const int64_t k = csr_key(u, r, t.n_rel);
        if (PASS == 0) {
            atomicAdd(&cnt_or_cursor[k], 1);
        } else {
            const int pos = rowptr[k] + atomicAdd(&cnt_or_cursor[k], 1);
            col[pos] = (int32_t)v;
        }
    }
}

// Canonical order inside each row (ascending source index) so that the
// floating-point gather-sum that consumes the plan is deterministic.
__global__ __launch_bounds__(256) void k_csr_sort_rows(const int32_t *rowptr, int32_t *col, int64_t n_keys) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_keys) return;
    const int b = rowptr[k], e = rowptr[k + 1];
    for (int i = b + 1; i < e; ++i) {
        const int x = col[i];
        int j = i - 1;
        while (j >= b && col[j] > x) { col[j + 1] = col[j]; --j; }
        col[j + 1] = x;
    }
}

// -------------------------------------------------------- pair search -----
// lanegcn.py:676-678: dist = a - c; sqrt((dist ** 2).sum(2)) <= th, fp32, no FMA.
__device__ __forceinline__ bool within(float ax, float ay, float cx, float cy, float th) {
    const float dx = __fsub_rn(ax, cx), dy = __fsub_rn(ay, cy);
    const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
    return __fsqrt_rn(d2) <= th;
}

// Workspace layout of one pair search: rowptr_true [T+1] | hi_base [B+1] | wi_base [B].  The count pass leaves the rows'
// raw counts in the caller's segment table rowptr_q [T+1] (an output that the fill pass writes in full afterwards), so
// that the scan reads counts that no workgroup of its own launch overwrites.
struct PairsJob {
    const float2 *agt; const int32_t *agt_off;
    const float2 *ctx; const int32_t *ctx_off;
    int n_scenes, n_agt, n_ctx, legacy;
    float th;
    int lanes;                  // lanes per target row in the row passes: kShortLanes or 64 (pairs_row_lanes)
    int32_t *hi, *wi;
    int64_t cap;
    int32_t *n_pairs, *rowptr_q, *ws;
    __device__ int32_t *rp() const { return ws; }
    __device__ int32_t *hi_base() const { return ws + (n_agt + 1); }
    __device__ int32_t *wi_base() const { return ws + (n_agt + 1) + n_scenes + 1; }
};
struct PairsJobs { PairsJob j[4]; };

// How many lanes a job gives each target row: kShortLanes at or below a mean context-list length (n_ctx / n_scenes) of
// kShortMeanCtx, a whole wave above it.  The rule only chooses speed; every width gives the same words for any list.
// Measured at S2 (mean list 50), count + fill launch: 64 lanes 9.3 + 9.0 us, 16 lanes 8.3 + 6.2, 8 lanes 8.4 + 6.8, 4 lanes
// 8.5 + 8.5, one lane per row 9.8 + 16.9 (the row's serial walk of its list: 50 correctly rounded square roots).
constexpr int kShortLanes = 16;
constexpr int kShortMeanCtx = 64;       // four trips of the short body
constexpr int kOffLds = 256;            // the row passes search agt_off in LDS when its n_scenes + 1 words fit
static inline int pairs_row_lanes(int64_t n_ctx, int n_scenes) {
    return n_ctx <= (int64_t)kShortMeanCtx * n_scenes ? kShortLanes : 64;
}
static inline int64_t pairs_row_blocks(int64_t n_agt, int lanes) {      // 256 / lanes rows per workgroup
    const int rows = 256 / lanes;
    return (n_agt + rows - 1) / rows;
}

// The context range of scene sc.  Offset tables are caller data: a table that does not describe this job (stale memory
// under a captured graph) must not take a load or a store out of bounds.
__device__ __forceinline__ void ctx_range(const PairsJob &j, int sc, int &c0, int &c1) {
    c0 = j.ctx_off[sc]; c1 = j.ctx_off[sc + 1];
    c0 = c0 < 0 ? 0 : c0 > j.n_ctx ? j.n_ctx : c0;
    c1 = c1 < c0 ? c0 : c1 > j.n_ctx ? j.n_ctx : c1;
}

// Fill pass, once per target row g of scene sc: the segment table of the later index_add_(0, hi, .):
// rowptr_q[h] = first p with hi[p] >= h.  hi is non-decreasing and a row g of a scene that advances the numbering owns
// h = hval(g), so rowptr_q[hval(g)] = rowptr[g]; rows of scenes that do not advance it (legacy: scenes without pairs)
// fill the tail [h_used, T), where no pair can follow: P.  rowptr_q[T] = P.
__device__ __forceinline__ void pairs_row_segment(const PairsJob &j, int sc, int g, int hval, int64_t pos) {
    const int32_t *rowptr = j.rp(), *hi_base = j.hi_base();
    const int n_agt = j.n_agt;
    const int P = rowptr[n_agt];
    int s0 = j.agt_off[sc], s1 = j.agt_off[sc + 1];
    s0 = s0 < 0 ? 0 : s0 > n_agt ? n_agt : s0;
    s1 = s1 < s0 ? s0 : s1 > n_agt ? n_agt : s1;
    const bool advances = !j.legacy || rowptr[s1] - rowptr[s0] > 0;
    const int q2 = hi_base[j.n_scenes] + g - hi_base[sc];
    // a capacity below the true pair count (n_pairs comes back negative): the segment table describes the pairs
    // that were kept, [0, cap) -- whatever walks it afterwards stays inside the caller's [cap, .] buffers
    const int Pc = (int64_t)P > j.cap ? (int)j.cap : P;
    if (advances) { if (hval >= 0 && hval <= n_agt) j.rowptr_q[hval] = pos > j.cap ? (int)j.cap : (int)pos; }
    else if (q2 >= 0 && q2 <= n_agt) j.rowptr_q[q2] = Pc;
    if (g == 0) j.rowptr_q[n_agt] = Pc;
}

// W lanes per target row, 64 / W rows per wave: the W lanes test W context rows per trip and their bits of the wave's
// ballot order the hits (ascending s).  PASS 0 counts, PASS 1 writes (hi, wi) and the row's word of the segment table.
// W = 64 is one wave per row, for long context lists (M2A: a scene's lane nodes); a short list (A2M, A2A: a scene's ~50
// actors) leaves most of such a wave idle around its private chain of dependent loads, so those jobs take fewer lanes
// per row and with them fewer waves.  The rows of a wave may lie in different scenes: a group that runs out of context
// rows leaves the loop, and the ballot shows its lanes as zeros.  s_off: kOffLds words of LDS for agt_off; every thread
// of the workgroup makes the call (it holds __syncthreads()).
template <int PASS, int W>
__device__ __forceinline__ void pairs_rows_body(const PairsJob &j, int row_block, int *s_off) {
    const bool staged = j.n_scenes + 1 <= kOffLds;          // the same in every thread
    if (staged) {
        if ((int)threadIdx.x <= j.n_scenes) s_off[threadIdx.x] = j.agt_off[threadIdx.x];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, sub = lane & (W - 1);
    const int g = row_block * (256 / W) + (int)threadIdx.x / W;
    if (g >= j.n_agt) return;
    const int sc = staged ? find_seg((const int *)s_off, j.n_scenes, g) : find_seg(j.agt_off, j.n_scenes, g);
    int c0, c1;
    ctx_range(j, sc, c0, c1);
    const float2 a = j.agt[g];
    int count = 0;
    int64_t pos = 0;
    int hval = 0, wbase = 0;
    if (PASS == 1) {
        pos = j.rp()[g];
        hval = g - (staged ? s_off[sc] : j.agt_off[sc]) + j.hi_base()[sc];
        wbase = j.wi_base()[sc] - c0;
        if (sub == 0) pairs_row_segment(j, sc, g, hval, pos);
    }
    for (int s0 = c0; s0 < c1; s0 += W) {
        const int s = s0 + sub;
        bool ok = false;
        if (s < c1) {
            const float2 c = j.ctx[s];
            ok = within(a.x, a.y, c.x, c.y, j.th);
        }
        unsigned long long m = __ballot(ok);
        if (W < 64) m = (m >> (lane - sub)) & ((1ull << (W & 63)) - 1ull);      // the row's own lanes
        if (PASS == 0) {
            count += __popcll(m);
        } else {
            if (ok) {
                const int64_t o = pos + __popcll(m & ((1ull << sub) - 1ull));
                if (o < j.cap) { j.hi[o] = hval; j.wi[o] = s + wbase; }
            }
            pos += __popcll(m);
        }
    }
    if (PASS == 0 && sub == 0) j.rowptr_q[g] = count;
}

template <int PASS>
__device__ __forceinline__ void pairs_rows_any(const PairsJob &j, int row_block, int *s_off) {
    if (j.lanes == kShortLanes) pairs_rows_body<PASS, kShortLanes>(j, row_block, s_off);
    else pairs_rows_body<PASS, 64>(j, row_block, s_off);
}

// blockIdx.y selects the job; blocks past a job's rows return at once
template <int PASS>
__global__ __launch_bounds__(256) void k_pairs_rows(const PairsJobs jobs) {
    __shared__ int s_off[kOffLds];
    pairs_rows_any<PASS>(jobs.j[blockIdx.y], (int)blockIdx.x, s_off);
}

// Row scan and per-scene bases of one pair job, in T / 4096 + 1 tile workgroups and one base workgroup (`part` past the
// tiles).  Both read the rows' RAW counts (rowptr_q) and the caller's tables only, never what another workgroup of the
// launch writes.
//   * tile workgroup: walks the 4096-row chunks (1024 threads x 4 consecutive rows: adjacent threads touch adjacent
//     words) up to its own; of those in front it only adds up the counts -- a few 10^4 ints at most, read directly, as
//     block_base does for the key tiles' totals -- its own it scans into rp[].  The last one holds rp[T] = P and
//     writes n_pairs.
//   * base workgroup: the per-scene index bases (lanegcn.py:681-687; legacy: a scene without pairs does not advance
//     the running counts) and hi_base[n_scenes] = rows numbered in all (h_used).  Whether a scene has a pair comes from
//     the raw counts: every row with a count marks its scene, found in the staged piece of agt_off, 1024 scenes per trip.
static inline int64_t pairs_scan_tiles(int64_t n_agt) { return n_agt / 4096 + 1; }

__device__ __forceinline__ void pairs_scan_bases_body(const PairsJob &j, int64_t part, int *lds, int *s_aoff, int *s_flag) {
    const int32_t *cnt = j.rowptr_q;
    const int n_agt = j.n_agt, n_scenes = j.n_scenes;
    if (part * 4096 <= n_agt) {
        int32_t *rp = j.rp();
        const int64_t t0 = part * 4096, b = t0 + 4 * (int64_t)threadIdx.x;
        int v[4] = {0, 0, 0, 0}, front = 0;
        // no branch on what is loaded: the loads of all chunks are in flight together
#pragma unroll 4
        for (int64_t c0 = 0; c0 <= n_agt; c0 += 4096) {
            if (c0 > t0) break;                                // the same in every thread
            const int64_t i = c0 + 4 * (int64_t)threadIdx.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = i + k < n_agt ? cnt[i + k] : 0;  // word T holds no count
                if (c0 == t0) v[k] = x; else front += x;
            }
        }
        int before, chunk;
        block_exclusive_scan<1024>(front, &before, lds);
        int off = block_exclusive_scan<1024>(v[0] + v[1] + v[2] + v[3], &chunk, lds) + before;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (b + k <= n_agt) rp[b + k] = off;
            off += v[k];
        }
        if (threadIdx.x == 0 && t0 + 4096 > n_agt) {           // the last tile
            const int tot = before + chunk;
            *j.n_pairs = (int64_t)tot > j.cap ? -tot : tot;
            if (n_agt == 0) j.rowptr_q[0] = 0;                 // no rows: the fill pass never runs for this job
        }
        return;
    }
    int32_t *hi_base = j.hi_base(), *wi_base = j.wi_base();
    int carry_h = 0, carry_w = 0;
    for (int c = 0; c < n_scenes; c += 1024) {
        const int i = c + threadIdx.x, nsc = n_scenes - c < 1024 ? n_scenes - c : 1024;
        for (int k = threadIdx.x; k <= nsc; k += 1024) {
            const int a = j.agt_off[c + k];
            s_aoff[k] = a < 0 ? 0 : a > n_agt ? n_agt : a;     // caller data: never index cnt[] out of bounds
        }
        if (threadIdx.x < nsc) s_flag[threadIdx.x] = 0;
        __syncthreads();
        if (j.legacy) {
            const int r0 = s_aoff[0], r1 = s_aoff[nsc];
            for (int r = r0 + 4 * (int)threadIdx.x; r < r1; r += 4096) {      // 4 consecutive rows: mostly one scene, one search
                int x[4], any = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { x[k] = r + k < r1 ? cnt[r + k] : 0; any |= x[k]; }
                if (any <= 0) continue;
                const int sc = find_seg((const int *)s_aoff, nsc, r);
                if (r + 3 < s_aoff[sc + 1]) { s_flag[sc] = 1; continue; }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x[k] > 0) s_flag[find_seg((const int *)s_aoff, nsc, r + k)] = 1;
            }
            __syncthreads();
        }
        int th = 0, tw = 0;
        if (i < n_scenes) {
            const int a0 = s_aoff[threadIdx.x], a1 = s_aoff[threadIdx.x + 1] < a0 ? a0 : s_aoff[threadIdx.x + 1];
            if (!j.legacy || s_flag[threadIdx.x]) { th = a1 - a0; tw = j.ctx_off[i + 1] - j.ctx_off[i]; }
        }
        int tot_h, tot_w;
        const int ph = block_exclusive_scan<1024>(th, &tot_h, lds);
        const int pw = block_exclusive_scan<1024>(tw, &tot_w, lds);
        if (i < n_scenes) { hi_base[i] = ph + carry_h; wi_base[i] = pw + carry_w; }
        carry_h += tot_h;
        carry_w += tot_w;
    }
    if (threadIdx.x == 0) hi_base[n_scenes] = carry_h;
}

// blockIdx.y selects the job; blockIdx.x: a tile of its row scan, the first one past its tiles its scene bases
__global__ __launch_bounds__(1024) void k_pairs_scan_bases(const PairsJobs jobs) {
    __shared__ int lds[1024 / 64 + 1], s_aoff[1024 + 1], s_flag[1024];
    const PairsJob &j = jobs.j[blockIdx.y];
    if ((int64_t)blockIdx.x <= (int64_t)j.n_agt / 4096 + 1) pairs_scan_bases_body(j, blockIdx.x, lds, s_aoff, s_flag);
}

// ------------------------------------------------- fused index pipeline -----
// lgcn_index_build: graph_gather + CSR plan + up to four pair searches in FOUR launches (count | scan | fill | sort)
// instead of twelve.  At S2 every one of those launches is a few microseconds of work behind a launch boundary
// of the same size; what the twelve cost is their number.
//   * graph_gather is folded into the edge pass: an edge thread turns its two local indices into global ones
//     (binary search of the segment table) and keeps them as an int32 pair for the fill pass.
//   * the per-key counter word serves the count pass (low half: edges of the key) AND the fill pass (high half: slots
//     handed out); the sort pass, which puts each key's entries in canonical (ascending source) order, writes it
//     back to ZERO.  The counters must be zero on entry and are zero again on completion: no zeroing launch and no
//     separate cursor array.  (Sorting a key from the thread that fills its last slot -- one launch fewer -- was
//     measured 8 x slower: the release/acquire pair it needs is a write-back + invalidate of an XCD's L2 per wave.)
//   * the count pass also adds up the keys of every 4096-key scan tile (LDS histogram per workgroup, one global
//     atomic per touched tile), so the scan is ONE launch of independent tiles: tile b adds the totals in front of it.
//   * the pair searches' count / scan / fill bodies ride in the first three launches as extra workgroups.
//   * the count pass searches the segment table in LDS when its pieces fit kIdxSegLds words (every workgroup stages
//     it once: a few coalesced loads per thread instead of two chains of log2(n_seg) dependent global loads per edge).
constexpr int kIdxScanTile = 4096;      // 1024 threads x 4 keys
constexpr int kIdxMaxTiles = 1024;      // n_keys1 <= 2^22
constexpr int kIdxSegLds = 2048;        // 16 KB of int64: S2 has 28 pieces per scene, 896

struct IndexParams {
    const int64_t *idx_local, *seg_off, *seg_base;
    int n_seg, n_rel;
    int64_t u_off[LGCN_MAX_REL], v_off[LGCN_MAX_REL];
    int64_t start[LGCN_MAX_REL + 1];          // prefix of the relations' edge counts
    int64_t n_nodes, n_keys1;                 // keys + 1
    unsigned long long *cnt;                  // [n_keys1 + kIdxMaxTiles], zero on entry and on completion:
                                              // per key (edges | slots handed out << 32), then the scan tiles' totals
    int32_t *uv;                              // [2 * total] global (u, v) of every edge; u = -1: dropped
    int32_t *rowptr, *col;
    int edge_blocks, scan_blocks, n_jobs;
    int job_blocks[5];                        // prefix of the pair jobs' row-block counts
    int job_tiles[5];                         // prefix of the pair jobs' row-scan tiles
    int32_t *clear_word;                      // optional word zeroed by the count pass
    PairsJobs jobs;
};

// as k_graph_gather; s_seg: the staged copy of seg_off (words 1 .. n_seg - 1, all that find_seg reads) or null
__device__ __forceinline__ int64_t to_global(const IndexParams &p, const int64_t *s_seg, int64_t i) {
    const int sg = s_seg ? find_seg(s_seg, p.n_seg, i) : find_seg(p.seg_off, p.n_seg, i);
    return p.idx_local[i] + p.seg_base[sg];
}

template <int PASS>     // 0: count, 1: fill
__global__ __launch_bounds__(256) void k_index_edges(const IndexParams p) {
    __shared__ int s_tile[kIdxMaxTiles];      // pair-search workgroups: the row body's offset table (kOffLds)
    __shared__ int64_t s_seg[PASS == 0 ? kIdxSegLds : 1];
    static_assert(kOffLds <= kIdxMaxTiles, "the row body's table lives in s_tile");
    const int bid = blockIdx.x;
    if (PASS == 0 && bid == 0 && threadIdx.x == 0 && p.clear_word) *p.clear_word = 0;
    if (bid >= p.edge_blocks) {               // pair-search workgroups
        const int b = bid - p.edge_blocks;
        int jn = 0;
        while (jn + 1 < p.n_jobs && b >= p.job_blocks[jn + 1]) ++jn;
        pairs_rows_any<PASS>(p.jobs.j[jn], b - p.job_blocks[jn], s_tile);
        return;
    }
    const bool seg_lds = PASS == 0 && p.n_seg <= kIdxSegLds;
    if (PASS == 0) {
        for (int i = threadIdx.x; i < p.scan_blocks; i += blockDim.x) s_tile[i] = 0;
        if (seg_lds)
            for (int i = 1 + threadIdx.x; i < p.n_seg; i += blockDim.x) s_seg[i] = p.seg_off[i];
        __syncthreads();
    }
    const int64_t total = p.start[p.n_rel];
    for (int64_t e = (int64_t)bid * blockDim.x + threadIdx.x; e < total; e += (int64_t)p.edge_blocks * blockDim.x) {
        int r = 0;
        while (r + 1 < p.n_rel && e >= p.start[r + 1]) ++r;
        if (PASS == 0) {
            const int64_t le = e - p.start[r];
            const int64_t *seg = seg_lds ? s_seg : nullptr;
            const int64_t u = to_global(p, seg, p.u_off[r] + le), v = to_global(p, seg, p.v_off[r] + le);
            const bool ok = u >= 0 && u < p.n_nodes && v >= 0 && v < p.n_nodes;     // never index out of bounds
            p.uv[2 * e] = ok ? (int32_t)u : -1;
            p.uv[2 * e + 1] = (int32_t)v;
            if (ok) {
                const int64_t k = csr_key(u, r, p.n_rel);
                atomicAdd(&p.cnt[k], 1ull);
                atomicAdd(&s_tile[k / kIdxScanTile], 1);
            }
        } else {
            const int u = p.uv[2 * e], v = p.uv[2 * e + 1];
            if (u < 0) continue;
            const int64_t k = csr_key(u, r, p.n_rel);
            const unsigned long long a = atomicAdd(&p.cnt[k], 1ull << 32);
            p.col[p.rowptr[k] + (int)(a >> 32)] = v;
        }
    }
    if (PASS == 0) {
        __syncthreads();
        for (int i = threadIdx.x; i < p.scan_blocks; i += blockDim.x)
            if (s_tile[i] != 0) atomicAdd(&p.cnt[p.n_keys1 + i], (unsigned long long)s_tile[i]);
    }
}

__global__ __launch_bounds__(1024) void k_index_scan(const IndexParams p) {
    __shared__ int lds[1024 / 64 + 1], s_aoff[1024 + 1], s_flag[1024];
    const int bid = blockIdx.x;
    if (bid >= p.scan_blocks) {               // pair searches: per job its row-scan tiles and one workgroup for the bases
        const int b = bid - p.scan_blocks;
        int jn = 0;
        while (jn + 1 < p.n_jobs && b >= p.job_tiles[jn + 1]) ++jn;
        pairs_scan_bases_body(p.jobs.j[jn], b - p.job_tiles[jn], lds, s_aoff, s_flag);
        return;
    }
    // keys in front of this tile: the totals of the tiles in front of it (<= 1024: one per thread; bid is blockIdx.x here)
    const int before = block_base<1024>(p.cnt + p.n_keys1, 1, lds);
    const int64_t b = (int64_t)bid * kIdxScanTile + 4 * (int64_t)threadIdx.x;
    int v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = b + k < p.n_keys1 ? (int)(p.cnt[b + k] & 0xffffffffull) : 0;
        sum += v[k];
    }
    int tile_total;
    int off = block_exclusive_scan<1024>(sum, &tile_total, lds) + before;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (b + k < p.n_keys1) p.rowptr[b + k] = off;
        off += v[k];
    }
}

// canonical order inside each key (as k_csr_sort_rows) + the counters back to zero
__global__ __launch_bounds__(256) void k_index_sort(const IndexParams p) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < kIdxMaxTiles) p.cnt[p.n_keys1 + k] = 0ull;
    if (k >= p.n_keys1) return;
    const unsigned long long w = p.cnt[k];
    if (w == 0ull) return;
    p.cnt[k] = 0ull;
    const int n = (int)(w & 0xffffffffull);
    int32_t *c = p.col + p.rowptr[k];
    for (int i = 1; i < n; ++i) {
        const int x = c[i];
        int q = i - 1;
        while (q >= 0 && c[q] > x) { c[q + 1] = c[q]; --q; }
        c[q + 1] = x;
    }
}

// -------------------------------------------- graph construction (row f3) -----
// dilated_nbrs (reference data.py:520-534): the scale-i relation is the boolean power A^(2^i) of the scale-0
// adjacency, formed by repeated squaring (mat = mat * mat).  One squaring of a CSR matrix with sorted or unsorted
// rows (duplicates allowed: they only repeat candidates):
//   bound  : cand_ptr[u] = exclusive scan of sum_{v in A[u]} |A[v]|
//   expand : row u's candidates {w : w in A[v], v in A[u]} -> sorted, each once (sq_merge_row), count kept
//   compact: rows packed to the scanned counts (+ the COO row index of every entry)
// One thread per row: lane graphs branch rarely, a row of A^32 has a handful of entries.
__global__ __launch_bounds__(256) void k_sq_bound(const int32_t *rowptr, const int32_t *col, int64_t n, int32_t *ub) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u > n) return;
    int s = 0;
    if (u < n)
        for (int e = rowptr[u]; e < rowptr[u + 1]; ++e) {
            const int v = col[e];
            if (v >= 0 && v < n) s += rowptr[v + 1] - rowptr[v];
        }
    ub[u] = s;        // ub[n] = 0: the scan leaves the total there
}

__global__ __launch_bounds__(256) void k_sq_expand(const int32_t *rowptr, const int32_t *col, int64_t n,
                                                   const int32_t *cand_ptr, int32_t *cand, int32_t *cnt) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u > n) return;
    if (u == n) { cnt[n] = 0; return; }
    const auto row_of = [n](int v) { return v >= 0 && v < n ? v : -1; };
    cnt[u] = sq_merge_row(rowptr, col, rowptr[u], rowptr[u + 1], row_of, cand + cand_ptr[u], cand_ptr[u + 1] - cand_ptr[u]);
}

__global__ __launch_bounds__(256) void k_sq_compact(const int32_t *cand_ptr, const int32_t *cand, const int32_t *out_rowptr,
                                                    int64_t n, int32_t *out_col, int32_t *out_row) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    const int b = out_rowptr[u], k = out_rowptr[u + 1] - b;
    const int32_t *c = cand + cand_ptr[u];
    for (int i = 0; i < k; ++i) {
        out_col[b + i] = c[i];
        if (out_row) out_row[b + i] = (int32_t)u;
    }
}

// Left / right node adjacency (reference preprocess_data.py:287-392, cross_angle = None); the bodies are in
// lgcn_graphops.hpp.
__global__ __launch_bounds__(256) void k_lane_mask(const int64_t *side, int64_t n_side, const int64_t *pre, int64_t n_pre,
                                                   const int64_t *suc, int64_t n_suc, int num_lanes, uint8_t *mat) {
    lane_mask_item(side, n_side, pre, n_pre, suc, n_suc, num_lanes, mat, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_cross_edges(const float2 *ctrs, const float2 *feats, const int64_t *lane_idcs,
                                                     int n, const uint8_t *mat, int num_lanes, float cross_dist,
                                                     int32_t *partner) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (h >= n) return;
    const int out = cross_partner(ctrs, feats, lane_idcs, n, mat, num_lanes, cross_dist, h, lane);
    if (lane == 0) partner[h] = out;
}

// rowptr and cursor of the CSR plan zeroed in one launch (two memset nodes cost a launch boundary each)
__global__ __launch_bounds__(256) void k_zero2(int32_t *a, int32_t *b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        a[i] = 0;
        b[i] = 0;
    }
}

__global__ __launch_bounds__(256) void k_widen(const int32_t *in, const int32_t *n_dev, int64_t cap, int64_t *out) {
    int64_t n = *n_dev;
    if (n < 0 || n > cap) n = cap;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = in[i];
}

static inline unsigned grid_for(int64_t n, int threads, int64_t max_blocks = 4096) {
    int64_t b = (n + threads - 1) / threads;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (unsigned)b;
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int lgcn_version(void) { return LGCN_VERSION; }

const char *lgcn_strerror(int code) {
    switch (code) {
        case LGCN_OK: return "ok";
        case LGCN_EINVAL: return "invalid argument (null pointer, negative size or bad flag)";
        case LGCN_ESHAPE: return "unsupported shape";
        case LGCN_EALIGN: return "pointer not 16-byte aligned";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown lgcn error";
    }
}

int lgcn_graph_gather(const int64_t *in, int64_t n_elem, const int64_t *seg_off, const int64_t *seg_base,
                      int n_seg, int64_t *out64, int32_t *out32, void *stream) {
    if (n_elem < 0 || n_seg < 0) return LGCN_EINVAL;
    if (n_elem == 0) return LGCN_OK;
    LGCN_CHECK_PTR(in); LGCN_CHECK_PTR(seg_off); LGCN_CHECK_PTR(seg_base);
    if (n_seg < 1 || (!out64 && !out32)) return LGCN_EINVAL;
    hipLaunchKernelGGL(k_graph_gather, dim3(grid_for(n_elem, 256)), dim3(256), 0, (hipStream_t)stream,
                       in, n_elem, seg_off, seg_base, n_seg, out64, out32);
    return launch_status();
}

int64_t lgcn_csr_rowptr_elems(int64_t n_nodes, int n_rel) {
    if (n_nodes < 0 || n_rel < 1 || n_rel > LGCN_MAX_REL) return LGCN_EINVAL;
    return ((n_nodes + 15) / 16) * n_rel * 16 + 1;
}

int64_t lgcn_csr_ws_elems(int64_t n_nodes, int n_rel) {
    const int64_t k = lgcn_csr_rowptr_elems(n_nodes, n_rel);
    if (k < 0) return k;
    return k + scan_ws_elems(k);  // cursor + scan block sums
}

int lgcn_csr_build(const int64_t *const *u_host, const int64_t *const *v_host, const int64_t *n_edges_host,
                   int n_rel, int64_t n_nodes, int32_t *rowptr, int32_t *col, int32_t *ws, void *stream) {
    if (n_rel < 1 || n_rel > LGCN_MAX_REL || n_nodes < 0) return LGCN_EINVAL;
    LGCN_CHECK_PTR(u_host); LGCN_CHECK_PTR(v_host); LGCN_CHECK_PTR(n_edges_host);
    LGCN_CHECK_PTR(rowptr); LGCN_CHECK_PTR(ws);
    hipStream_t st = (hipStream_t)stream;
    CooTable t;
    t.n_rel = n_rel;
    t.n_nodes = n_nodes;
    t.start[0] = 0;
    for (int r = 0; r < n_rel; ++r) {
        if (n_edges_host[r] < 0) return LGCN_EINVAL;
        if (n_edges_host[r] > 0 && (!u_host[r] || !v_host[r])) return LGCN_EINVAL;
        t.u[r] = u_host[r];
        t.v[r] = v_host[r];
        t.start[r + 1] = t.start[r] + n_edges_host[r];
    }
    for (int r = n_rel; r < LGCN_MAX_REL; ++r) { t.u[r] = nullptr; t.v[r] = nullptr; t.start[r + 1] = t.start[n_rel]; }
    const int64_t total = t.start[n_rel];
    if (total > 0x7fffffff || n_nodes > 0x7fffffff) return LGCN_ESHAPE;
    if (total > 0) LGCN_CHECK_PTR(col);
    const int64_t nk1 = lgcn_csr_rowptr_elems(n_nodes, n_rel);  // keys + 1
    int32_t *cursor = ws;
    int32_t *sums = ws + nk1;
    hipLaunchKernelGGL(k_zero2, dim3(grid_for(nk1, 256, 1024)), dim3(256), 0, st, rowptr, cursor, nk1);
    if (total > 0) {
        hipLaunchKernelGGL((k_csr_edges<0>), dim3(grid_for(total, 256)), dim3(256), 0, st, t, rowptr, nullptr, nullptr);
    }
    int rc = exclusive_scan(rowptr, rowptr, nk1, sums, st);
    if (rc != LGCN_OK) return rc;
    if (total > 0) {
        hipLaunchKernelGGL((k_csr_edges<1>), dim3(grid_for(total, 256)), dim3(256), 0, st, t, cursor, rowptr, col);
        hipLaunchKernelGGL(k_csr_sort_rows, dim3((unsigned)((nk1 - 1 + 255) / 256)), dim3(256), 0, st,
                           rowptr, col, nk1 - 1);
    }
    return launch_status();
}

int64_t lgcn_pairs_ws_elems(int64_t n_agt, int n_scenes) {
    if (n_agt < 0 || n_scenes < 0) return LGCN_EINVAL;
    // rowptr_true [T+1] + hi_base [B+1] + wi_base [B]
    return (n_agt + 1) + 2 * (int64_t)n_scenes + 1;
}

static int pairs_job_check(const lgcn_pairs_job_t &q) {
    if (q.n_scenes < 1 || q.n_agt < 0 || q.n_ctx < 0 || q.cap < 0) return LGCN_EINVAL;
    if (q.n_agt > 0x7ffffff0 || q.n_ctx > 0x7ffffff0 || q.cap > 0x7ffffff0) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(q.agt_off); LGCN_CHECK_PTR(q.ctx_off); LGCN_CHECK_PTR(q.n_pairs);
    LGCN_CHECK_PTR(q.rowptr); LGCN_CHECK_PTR(q.ws);
    if (q.n_agt > 0) LGCN_CHECK_PTR(q.agt_ctrs);
    if (q.n_ctx > 0) LGCN_CHECK_PTR(q.ctx_ctrs);
    if (q.cap > 0) { LGCN_CHECK_PTR(q.hi); LGCN_CHECK_PTR(q.wi); }
    return LGCN_OK;
}

static PairsJob to_device_job(const lgcn_pairs_job_t &q) {
    PairsJob d;
    d.agt = (const float2 *)q.agt_ctrs; d.agt_off = q.agt_off;
    d.ctx = (const float2 *)q.ctx_ctrs; d.ctx_off = q.ctx_off;
    d.n_scenes = q.n_scenes; d.n_agt = (int)q.n_agt; d.n_ctx = (int)q.n_ctx; d.legacy = q.legacy_offsets; d.th = q.dist_th;
    d.hi = q.hi; d.wi = q.wi; d.cap = q.cap; d.n_pairs = q.n_pairs; d.rowptr_q = q.rowptr; d.ws = q.ws;
    d.lanes = pairs_row_lanes(q.n_ctx, q.n_scenes);
    return d;
}

int lgcn_pairs_build_multi(const lgcn_pairs_job_t *jobs, int n_jobs, void *stream) {
    if (n_jobs < 1 || n_jobs > 4) return LGCN_EINVAL;
    LGCN_CHECK_PTR(jobs);
    hipStream_t st = (hipStream_t)stream;
    PairsJobs dj;
    int64_t row_blocks = 0, tiles = 0;
    for (int k = 0; k < n_jobs; ++k) {
        const lgcn_pairs_job_t &q = jobs[k];
        const int rc = pairs_job_check(q);
        if (rc != LGCN_OK) return rc;
        dj.j[k] = to_device_job(q);
        const int64_t nb = pairs_row_blocks(q.n_agt, dj.j[k].lanes), nt = pairs_scan_tiles(q.n_agt);
        if (nb > row_blocks) row_blocks = nb;
        if (nt > tiles) tiles = nt;
    }
    for (int k = n_jobs; k < 4; ++k) dj.j[k] = dj.j[0];
    // three launches for all jobs: count per target row, scan tiles + per-scene bases (one more block per job), fill
    // (+ segment table).  A job without rows still gets rowptr[0] = P = 0 from its scan tile.
    if (row_blocks > 0) hipLaunchKernelGGL((k_pairs_rows<0>), dim3((unsigned)row_blocks, n_jobs), dim3(256), 0, st, dj);
    hipLaunchKernelGGL(k_pairs_scan_bases, dim3((unsigned)(tiles + 1), n_jobs), dim3(1024), 0, st, dj);
    if (row_blocks > 0) hipLaunchKernelGGL((k_pairs_rows<1>), dim3((unsigned)row_blocks, n_jobs), dim3(256), 0, st, dj);
    return launch_status();
}

int lgcn_pairs_build(const float *agt_ctrs, const int32_t *agt_off, const float *ctx_ctrs,
                     const int32_t *ctx_off, int n_scenes, int64_t n_agt, int64_t n_ctx, float dist_th,
                     int legacy_offsets, int32_t *hi, int32_t *wi, int64_t cap, int32_t *n_pairs,
                     int32_t *rowptr, int32_t *ws, void *stream) {
    lgcn_pairs_job_t q;
    q.agt_ctrs = agt_ctrs; q.agt_off = agt_off; q.ctx_ctrs = ctx_ctrs; q.ctx_off = ctx_off;
    q.n_scenes = n_scenes; q.legacy_offsets = legacy_offsets; q.n_agt = n_agt; q.n_ctx = n_ctx;
    q.dist_th = dist_th; q.pad_ = 0; q.hi = hi; q.wi = wi; q.cap = cap; q.n_pairs = n_pairs; q.rowptr = rowptr; q.ws = ws;
    return lgcn_pairs_build_multi(&q, 1, stream);
}

int64_t lgcn_index_uv_elems(int64_t n_edges) { return n_edges < 0 ? (int64_t)LGCN_EINVAL : 2 * n_edges; }

int64_t lgcn_index_cnt_words(int64_t n_nodes, int n_rel) {
    const int64_t k = lgcn_csr_rowptr_elems(n_nodes, n_rel);
    return k < 0 ? k : k + kIdxMaxTiles;
}

int lgcn_index_build(const lgcn_index_t *ph, void *stream) {
    LGCN_CHECK_PTR(ph);
    const lgcn_index_t &q = *ph;
    if (q.n_rel < 1 || q.n_rel > LGCN_MAX_REL || q.n_nodes < 0 || q.n_seg < 1 || q.n_jobs < 0 || q.n_jobs > 4 || q.n_elem < 0)
        return LGCN_EINVAL;
    LGCN_CHECK_PTR(q.rowptr); LGCN_CHECK_PTR(q.cnt);
    if (misaligned(q.cnt, 7u)) return LGCN_EALIGN;
    if (q.n_jobs > 0) LGCN_CHECK_PTR(q.jobs);
    IndexParams p;
    p.idx_local = q.idx_local; p.seg_off = q.seg_off; p.seg_base = q.seg_base; p.n_seg = q.n_seg; p.n_rel = q.n_rel;
    p.start[0] = 0;
    for (int r = 0; r < q.n_rel; ++r) {
        if (q.n_edges[r] < 0 || q.u_off[r] < 0 || q.v_off[r] < 0 || q.u_off[r] + q.n_edges[r] > q.n_elem ||
            q.v_off[r] + q.n_edges[r] > q.n_elem)
            return LGCN_EINVAL;
        p.u_off[r] = q.u_off[r]; p.v_off[r] = q.v_off[r];
        p.start[r + 1] = p.start[r] + q.n_edges[r];
    }
    for (int r = q.n_rel; r < LGCN_MAX_REL; ++r) { p.u_off[r] = p.v_off[r] = 0; p.start[r + 1] = p.start[q.n_rel]; }
    const int64_t total = p.start[q.n_rel];
    if (total > 0x7fffffff || q.n_nodes > 0x7fffffff) return LGCN_ESHAPE;
    const int64_t nk1 = lgcn_csr_rowptr_elems(q.n_nodes, q.n_rel);
    if (nk1 > (int64_t)kIdxScanTile * kIdxMaxTiles) return LGCN_ESHAPE;      // one scan launch: <= 1024 tiles of 4096 keys
    if (total > 0) {
        LGCN_CHECK_PTR(q.idx_local); LGCN_CHECK_PTR(q.seg_off); LGCN_CHECK_PTR(q.seg_base);
        LGCN_CHECK_PTR(q.col); LGCN_CHECK_PTR(q.uv);
    }
    p.n_nodes = q.n_nodes; p.n_keys1 = nk1;
    p.cnt = reinterpret_cast<unsigned long long *>(q.cnt); p.uv = q.uv; p.rowptr = q.rowptr; p.col = q.col;
    p.n_jobs = q.n_jobs;
    p.clear_word = q.clear_word;
    p.job_blocks[0] = 0;
    p.job_tiles[0] = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < q.n_jobs) {
            const lgcn_pairs_job_t &jq = q.jobs[k];
            const int rc = pairs_job_check(jq);
            if (rc != LGCN_OK) return rc;
            p.jobs.j[k] = to_device_job(jq);
            p.job_blocks[k + 1] = p.job_blocks[k] + (int)pairs_row_blocks(jq.n_agt, p.jobs.j[k].lanes);
            p.job_tiles[k + 1] = p.job_tiles[k] + (int)pairs_scan_tiles(jq.n_agt) + 1;       // + the base workgroup
        } else {
            if (k > 0) p.jobs.j[k] = p.jobs.j[0];
            p.job_blocks[k + 1] = p.job_blocks[k];
            p.job_tiles[k + 1] = p.job_tiles[k];
        }
    }
    if (q.n_jobs == 0) {
        PairsJob z{};
        for (int k = 0; k < 4; ++k) p.jobs.j[k] = z;
    }
    p.edge_blocks = total > 0 ? (int)grid_for(total, 256, 1024) : 0;
    p.scan_blocks = (int)((nk1 + kIdxScanTile - 1) / kIdxScanTile);
    hipStream_t st = (hipStream_t)stream;
    const unsigned g13 = (unsigned)(p.edge_blocks + p.job_blocks[4]);
    if (g13 > 0) hipLaunchKernelGGL((k_index_edges<0>), dim3(g13), dim3(256), 0, st, p);
    else if (q.clear_word) { hipError_t e = hipMemsetAsync(q.clear_word, 0, 4, st); if (e != hipSuccess) return (int)e; }
    hipLaunchKernelGGL(k_index_scan, dim3((unsigned)(p.scan_blocks + p.job_tiles[4])), dim3(1024), 0, st, p);
    if (g13 > 0) hipLaunchKernelGGL((k_index_edges<1>), dim3(g13), dim3(256), 0, st, p);
    if (total > 0) hipLaunchKernelGGL(k_index_sort, dim3((unsigned)((nk1 + 255) / 256)), dim3(256), 0, st, p);
    return launch_status();
}

int lgcn_bool_square_bound(const int32_t *rowptr, const int32_t *col, int64_t n, int32_t *cand_ptr, int32_t *ws,
                            void *stream) {
    if (n < 0) return LGCN_EINVAL;
    if (n > 0x7ffffff0) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(rowptr); LGCN_CHECK_PTR(cand_ptr); LGCN_CHECK_PTR(ws);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sq_bound, dim3(grid_for(n + 1, 256, 1 << 22)), dim3(256), 0, st, rowptr, col, n, cand_ptr);
    return exclusive_scan(cand_ptr, cand_ptr, n + 1, ws, st);
}

int lgcn_bool_square(const int32_t *rowptr, const int32_t *col, int64_t n, const int32_t *cand_ptr, int32_t *cand,
                     int32_t *out_rowptr, int32_t *ws, void *stream) {
    if (n < 0) return LGCN_EINVAL;
    if (n > 0x7ffffff0) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(rowptr); LGCN_CHECK_PTR(cand_ptr); LGCN_CHECK_PTR(out_rowptr); LGCN_CHECK_PTR(ws);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sq_expand, dim3(grid_for(n + 1, 256, 1 << 22)), dim3(256), 0, st, rowptr, col, n, cand_ptr, cand,
                       out_rowptr);
    return exclusive_scan(out_rowptr, out_rowptr, n + 1, ws, st);
}

int lgcn_bool_square_compact(const int32_t *cand_ptr, const int32_t *cand, const int32_t *out_rowptr, int64_t n,
                             int32_t *out_col, int32_t *out_row, void *stream) {
    if (n < 0) return LGCN_EINVAL;
    if (n == 0) return LGCN_OK;
    LGCN_CHECK_PTR(cand_ptr); LGCN_CHECK_PTR(out_rowptr);
    hipLaunchKernelGGL(k_sq_compact, dim3(grid_for(n, 256, 1 << 22)), dim3(256), 0, (hipStream_t)stream, cand_ptr, cand,
                       out_rowptr, n, out_col, out_row);
    return launch_status();
}

int64_t lgcn_scan_ws_elems(int64_t n) { return n < 0 ? (int64_t)LGCN_EINVAL : scan_ws_elems(n); }

int lgcn_cross_edges(const float *ctrs, const float *feats, const int64_t *lane_idcs, int64_t n_nodes, int num_lanes,
                     const int64_t *side_pairs, int64_t n_side, const int64_t *pre_pairs, int64_t n_pre,
                     const int64_t *suc_pairs, int64_t n_suc, float cross_dist, uint8_t *mat, int32_t *partner,
                     void *stream) {
    if (n_nodes < 0 || num_lanes < 0 || n_side < 0 || n_pre < 0 || n_suc < 0) return LGCN_EINVAL;
    if (n_nodes > 0x7ffffff0 || (int64_t)num_lanes * num_lanes > 0x7ffffff0) return LGCN_ESHAPE;
    if (n_nodes == 0) return LGCN_OK;
    LGCN_CHECK_PTR(ctrs); LGCN_CHECK_PTR(feats); LGCN_CHECK_PTR(lane_idcs); LGCN_CHECK_PTR(partner);
    if (num_lanes > 0) LGCN_CHECK_PTR(mat);
    if (n_side > 0) LGCN_CHECK_PTR(side_pairs);
    if (n_pre > 0) LGCN_CHECK_PTR(pre_pairs);
    if (n_suc > 0) LGCN_CHECK_PTR(suc_pairs);
    hipStream_t st = (hipStream_t)stream;
    if (num_lanes > 0) {
        hipError_t e = hipMemsetAsync(mat, 0, (size_t)num_lanes * num_lanes, st);
        if (e != hipSuccess) return (int)e;
    }
    const int64_t work = n_side * (n_pre + n_suc + 1);
    if (work > 0)
        hipLaunchKernelGGL(k_lane_mask, dim3(grid_for(work, 256, 1 << 22)), dim3(256), 0, st, side_pairs, n_side, pre_pairs,
                           n_pre, suc_pairs, n_suc, num_lanes, mat);
    hipLaunchKernelGGL(k_cross_edges, dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, st, (const float2 *)ctrs,
                       (const float2 *)feats, lane_idcs, (int)n_nodes, mat, num_lanes, cross_dist, partner);
    return launch_status();
}

int lgcn_widen_i32(const int32_t *in, const int32_t *n_dev, int64_t cap, int64_t *out, void *stream) {
    if (cap < 0) return LGCN_EINVAL;
    if (cap == 0) return LGCN_OK;
    LGCN_CHECK_PTR(in); LGCN_CHECK_PTR(n_dev); LGCN_CHECK_PTR(out);
    hipLaunchKernelGGL(k_widen, dim3(grid_for(cap, 256, 1024)), dim3(256), 0, (hipStream_t)stream, in, n_dev, cap, out);
    return launch_status();
}

}  // extern "C"
