// Lane-RoI extraction of the fork model for a batch of scenes (reference data_lrcnn.py:620-844, generate_lane_roi):
// per-agent lane search, RoI nodes, the 14 induced relations.  Integer and exact-fp32 kernels; compiled with
// -ffp-contract=off so that every distance is sub / mul / add / sqrt as numpy forms it.  See include/lgcn.h.
//
// Order never comes from an atomic: atomics here only count (integers), OR bits or take a minimum, whose results do not
// depend on arrival order; the one cursor-style fill (k_roi_edge_fill_rows) is followed by a sort of every row.  The scans
// (block-wide and device-wide) and the offset-table search are those of lgcn_blockscan.hpp.
#include "lgcn_common.hpp"
#include "lgcn_blockscan.hpp"

namespace lgcn {

constexpr int kRoiMaxLanes = 4096;            // lanes per scene: the search kernel's LDS bitsets and lane list
constexpr int kRoiWords = kRoiMaxLanes / 32;
constexpr int kRoiMaxLevels = 4096;           // levels of one lane search (a cycle of zero-length lanes never ends)
constexpr int kRoiRel = 14;
constexpr int kRoiSteps = 20;
constexpr int kRoiThreads = 256;
constexpr int kStRange = 1, kStLevels = 2;
constexpr int kRoiSumBlock = 128;             // numpy's PW_BLOCKSIZE: longer sums are split in halves
constexpr int kRoiSumBuffer = 8192;           // numpy's default reduction buffer: longer sums go piece by piece
constexpr int kRoiSumDepth = 10;

// regions of the int32 workspace (each a multiple of 4 elements)
struct RoiWs {
    int32_t *cursor, *cnt, *sums, *lane_nodes, *node_rank, *col, *agent_lanes, *roi_lanes, *roi_lane_off;
    float *lane_len;
    int64_t n_keys, n_scan, total;
};

__host__ __device__ inline RoiWs roi_ws(int32_t *ws, int64_t N, int64_t L, int64_t E, int64_t slots, int64_t A) {
    RoiWs w;
    w.n_keys = kRoiRel * N;
    w.n_scan = w.n_keys + L + 1;
    int64_t o = 0;
    w.cursor = ws + o;       o += up4(w.n_keys);
    w.cnt = ws + o;          o += up4(w.n_scan);
    w.sums = ws + o;         o += up4(scan_ws_elems(w.n_scan));
    w.lane_len = reinterpret_cast<float *>(ws + o); o += up4(L);
    w.lane_nodes = ws + o;   o += up4(N);
    w.node_rank = ws + o;    o += up4(N);
    w.col = ws + o;          o += up4(E);
    w.agent_lanes = ws + o;  o += up4(A);
    w.roi_lanes = ws + o;    o += up4(slots);
    w.roi_lane_off = ws + o; o += up4(slots);
    w.total = o;
    return w;
}

struct RoiTabs {      // the offset tables inside lgcn_roi_t::off_*
    const int32_t *node, *lane, *agent, *slot, *suc, *pre, *edge;
};
__host__ __device__ inline RoiTabs roi_tabs(const int32_t *off, int S) {
    RoiTabs t;
    t.node = off;
    t.lane = off + (S + 1);
    t.agent = off + 2 * (S + 1);
    t.slot = off + 3 * (S + 1);
    t.suc = off + 4 * (S + 1);
    t.pre = off + 5 * (S + 1);
    t.edge = off + 6 * (S + 1);
    return t;
}

// ------------------------------------------------------------------ lane tables
// One thread per lane of the batch walks its scene's nodes (the loads are the same address across a scene's threads).
__global__ __launch_bounds__(kRoiThreads) void k_roi_lane_count(const lgcn_roi_t p, const RoiWs w) {
    const int gl = blockIdx.x * kRoiThreads + threadIdx.x;
    if (gl == 0) {
        p.agent_nodes[p.n_agents] = 0;           // status word
        w.cnt[w.n_keys + p.n_lanes] = 0;         // tail of the scan
    }
    if (gl >= p.n_lanes) return;
    const RoiTabs t = roi_tabs(p.off_dev, p.n_scenes);
    const int s = find_seg(t.lane, p.n_scenes, gl);
    const int l = gl - t.lane[s];
    int c = 0;
    for (int i = t.node[s]; i < t.node[s + 1]; ++i) c += p.lane_idcs[i] == l;
    w.cnt[w.n_keys + gl] = c;
}

__host__ __device__ __forceinline__ float roi_norm(const float *xy) {
    const float x = xy[0], y = xy[1];
    return sqrtf(x * x + y * y);      // correctly rounded sqrt; no contraction
}

// numpy's pairwise_sum of the norms of feats[nodes[0..n)] for n <= 128 (8 accumulators, then the remainder in order)
__host__ __device__ inline float roi_lane_block(const int32_t *nodes, int n, const float *feats) {
    if (n < 8) {
        float r = 0.f;
        for (int k = 0; k < n; ++k) r += roi_norm(feats + 2 * nodes[k]);
        return r;
    }
    float r0 = roi_norm(feats + 2 * nodes[0]), r1 = roi_norm(feats + 2 * nodes[1]), r2 = roi_norm(feats + 2 * nodes[2]),
          r3 = roi_norm(feats + 2 * nodes[3]), r4 = roi_norm(feats + 2 * nodes[4]), r5 = roi_norm(feats + 2 * nodes[5]),
          r6 = roi_norm(feats + 2 * nodes[6]), r7 = roi_norm(feats + 2 * nodes[7]);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += roi_norm(feats + 2 * nodes[i]);     r1 += roi_norm(feats + 2 * nodes[i + 1]);
        r2 += roi_norm(feats + 2 * nodes[i + 2]); r3 += roi_norm(feats + 2 * nodes[i + 3]);
        r4 += roi_norm(feats + 2 * nodes[i + 4]); r5 += roi_norm(feats + 2 * nodes[i + 5]);
        r6 += roi_norm(feats + 2 * nodes[i + 6]); r7 += roi_norm(feats + 2 * nodes[i + 7]);
    }
    float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += roi_norm(feats + 2 * nodes[i]);
    return res;
}

// numpy's pairwise_sum of up to 8192 elements: above 128 elements numpy halves the range (the left half cut down to a
// multiple of 8) and adds the two halves' sums, recursively.  The recursion is walked with a stack of frames: a range of m
// elements leaves at most m / 2 + 8 to its right half, so 8192 elements are down to 128 within 7 levels.
__host__ __device__ inline float roi_lane_piece(const int32_t *nodes, int n, const float *feats) {
    if (n <= kRoiSumBlock) return roi_lane_block(nodes, n, feats);
    int off[kRoiSumDepth], len[kRoiSumDepth], stage[kRoiSumDepth];
    float left[kRoiSumDepth];
    int sp = 0;
    off[0] = 0; len[0] = n; stage[0] = 0; left[0] = 0.f;
    float ret = 0.f;
    while (sp >= 0) {
        const int o = off[sp], m = len[sp];
        if (m <= kRoiSumBlock || sp + 1 >= kRoiSumDepth) {       // a leaf (the depth bound is never reached, see above)
            ret = roi_lane_block(nodes + o, m, feats);
            --sp;
            continue;
        }
        int half = m / 2;
        half -= half % 8;
        if (stage[sp] == 0) {
            stage[sp] = 1;
            ++sp;
            off[sp] = o; len[sp] = half; stage[sp] = 0;
        } else if (stage[sp] == 1) {
            left[sp] = ret;
            stage[sp] = 2;
            ++sp;
            off[sp] = o + half; len[sp] = m - half; stage[sp] = 0;
        } else {
            ret = left[sp] + ret;
            --sp;
        }
    }
    return ret;
}

// np.sum of the norms of feats[nodes[0..n)]: numpy reduces through its buffer, 8192 elements at a time (np.getbufsize()'s
// default), every piece by pairwise_sum, the pieces' sums added in order
__host__ __device__ inline float roi_lane_length(const int32_t *nodes, int n, const float *feats) {
    float res = roi_lane_piece(nodes, n < kRoiSumBuffer ? n : kRoiSumBuffer, feats);
    for (int i = kRoiSumBuffer; i < n; i += kRoiSumBuffer)
        res += roi_lane_piece(nodes + i, n - i < kRoiSumBuffer ? n - i : kRoiSumBuffer, feats);
    return res;
}

__global__ __launch_bounds__(kRoiThreads) void k_roi_lane_fill(const lgcn_roi_t p, const RoiWs w) {
    const int gl = blockIdx.x * kRoiThreads + threadIdx.x;
    if (gl >= p.n_lanes) return;
    const RoiTabs t = roi_tabs(p.off_dev, p.n_scenes);
    const int s = find_seg(t.lane, p.n_scenes, gl);
    const int l = gl - t.lane[s];
    const int32_t *lane_ptr = w.cnt + w.n_keys;
    const int base = lane_ptr[gl] - lane_ptr[0], end = lane_ptr[gl + 1] - lane_ptr[0];
    const int nb = t.node[s], nl = t.lane[s + 1] - t.lane[s];
    int c = base;
    bool bad = false;       // a node of no lane of its scene: no table holds it, so it is reported, not dropped in silence
    for (int i = nb; i < t.node[s + 1]; ++i) {
        const int li = p.lane_idcs[i];
        bad |= (unsigned)li >= (unsigned)nl;
        if (li == l && c < end) {
            w.lane_nodes[c] = i - nb;
            w.node_rank[i] = c - base;
            ++c;
        }
    }
    if (bad && l == 0) atomicOr(&p.agent_nodes[p.n_agents], kStRange);
    w.lane_len[gl] = roi_lane_length(w.lane_nodes + base, c - base, p.feats + 2 * (int64_t)nb);
}

// ------------------------------------------------------------------ the 14 relations as CSR rows (key = rel * N + node)
__device__ __forceinline__ bool roi_edge_key(const lgcn_roi_t &p, const RoiTabs &t, int e, int *key, int *v_local) {
    const int S = p.n_scenes;
    const int seg = find_seg(t.edge, kRoiRel * S, e);
    const int r = seg / S, s = seg - r * S;
    const int nn = t.node[s + 1] - t.node[s];
    const int u = p.edge_u[e], v = p.edge_v[e];
    if ((unsigned)u >= (unsigned)nn || (unsigned)v >= (unsigned)nn) return false;
    *key = r * p.n_nodes + t.node[s] + u;
    *v_local = v;
    return true;
}

__global__ __launch_bounds__(kRoiThreads) void k_roi_edge_rows(const lgcn_roi_t p, const RoiWs w) {
    const int e = blockIdx.x * kRoiThreads + threadIdx.x;
    if (e >= p.n_edges) return;
    const RoiTabs t = roi_tabs(p.off_dev, p.n_scenes);
    int key, v;
    if (roi_edge_key(p, t, e, &key, &v)) atomicAdd(&w.cnt[key], 1);
    else atomicOr(&p.agent_nodes[p.n_agents], kStRange);
}

__global__ __launch_bounds__(kRoiThreads) void k_roi_edge_fill_rows(const lgcn_roi_t p, const RoiWs w) {
    const int e = blockIdx.x * kRoiThreads + threadIdx.x;
    if (e >= p.n_edges) return;
    const RoiTabs t = roi_tabs(p.off_dev, p.n_scenes);
    int key, v;
    if (!roi_edge_key(p, t, e, &key, &v)) return;
    const int pos = w.cnt[key] + atomicAdd(&w.cursor[key], 1);
    if (pos < w.cnt[key + 1] && pos < p.n_edges) w.col[pos] = v;
}

__device__ __forceinline__ void roi_sort32(int32_t *a, int n) {
    for (int i = 1; i < n; ++i) {
        const int32_t x = a[i];
        int j = i - 1;
        for (; j >= 0 && a[j] > x; --j) a[j + 1] = a[j];
        a[j + 1] = x;
    }
}

__global__ __launch_bounds__(kRoiThreads) void k_roi_sort_rows(const RoiWs w) {
    const int64_t k = (int64_t)blockIdx.x * kRoiThreads + threadIdx.x;
    if (k >= w.n_keys) return;
    roi_sort32(w.col + w.cnt[k], w.cnt[k + 1] - w.cnt[k]);
}

// ------------------------------------------------------------------ stage 1: one workgroup per agent
__device__ __forceinline__ bool roi_bit(const uint32_t *set, int i) { return (set[i >> 5] >> (i & 31)) & 1u; }

// numpy's pairwise_sum over the 20 step norms: 8 accumulators over steps 0..15, then steps 16..19 in order
__device__ __forceinline__ float roi_speed(const float *steps) {
    int first = -1, last = -1;
    for (int k = 0; k < kRoiSteps; ++k)
        if (roi_norm(steps + 2 * k) > 0.f) {
            if (first < 0) first = k;
            last = k;
        }
    if (first < 0) return 0.f;
    float r0 = roi_norm(steps + 0) + roi_norm(steps + 16), r1 = roi_norm(steps + 2) + roi_norm(steps + 18),
          r2 = roi_norm(steps + 4) + roi_norm(steps + 20), r3 = roi_norm(steps + 6) + roi_norm(steps + 22),
          r4 = roi_norm(steps + 8) + roi_norm(steps + 24), r5 = roi_norm(steps + 10) + roi_norm(steps + 26),
          r6 = roi_norm(steps + 12) + roi_norm(steps + 28), r7 = roi_norm(steps + 14) + roi_norm(steps + 30);
    float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (int k = 16; k < kRoiSteps; ++k) res += roi_norm(steps + 2 * k);
    // fp32 distance over the float64 duration (steps * 0.1 s), rounded to fp32 on assignment
    return (float)((double)res / ((double)(last - first + 1) * 0.1));
}

__global__ __launch_bounds__(kRoiThreads) void k_roi_search(const lgcn_roi_t p, const RoiWs w) {
    __shared__ uint32_t s_front[kRoiWords], s_next[kRoiWords], s_seen[kRoiWords], s_all[kRoiWords], s_cur[kRoiWords];
    __shared__ int s_list[kRoiMaxLanes];
    __shared__ unsigned long long s_best[2];
    __shared__ unsigned s_minbits;
    __shared__ float s_vel, s_dist;
    __shared__ int s_any, s_n, s_add, s_cnt, s_has;

    const int a = blockIdx.x, tid = threadIdx.x;
    const RoiTabs t = roi_tabs(p.off_dev, p.n_scenes);
    const int S = p.n_scenes;
    const int s = find_seg(t.agent, S, a);
    const int nl = t.lane[s + 1] - t.lane[s], lb = t.lane[s];
    const int nb = t.node[s], nn = t.node[s + 1] - nb;
    const int W = (nl + 31) >> 5;
    int32_t *status = p.agent_nodes + p.n_agents;

    if (tid == 0) {
        s_vel = roi_speed(p.a_feats + (int64_t)a * kRoiSteps * 2);
        s_best[0] = s_best[1] = ~0ull;
        p.agent_nodes[a] = 0;
        w.agent_lanes[a] = 0;
    }
    __syncthreads();
    const float vel = s_vel;
    if (tid == 0) p.agent_vel[a] = vel;
    if (vel == 0.f || nl <= 0 || nl > kRoiMaxLanes || nn <= 0) return;

    // ---- anchor node
    {
        const float kPi = (float)3.141592653589793, kTwoPi = (float)(2 * 3.141592653589793);
        const float kQuarter = (float)(0.25 * 3.141592653589793), kHalf = (float)(0.5 * 3.141592653589793);
        const float *f19 = p.a_feats + ((int64_t)a * kRoiSteps + (kRoiSteps - 1)) * 2;
        const float t1 = atan2f(f19[1], f19[0]);
        const float ax = p.a_ctrs[2 * a], ay = p.a_ctrs[2 * a + 1];
        unsigned long long b4 = ~0ull, b2 = ~0ull;
        for (int i = tid; i < nn; i += kRoiThreads) {
            const float *f = p.feats + 2 * (int64_t)(nb + i), *c = p.ctrs + 2 * (int64_t)(nb + i);
            float dt = fabsf(t1 - atan2f(f[1], f[0]));
            if (dt > kPi) dt = fabsf(dt - kTwoPi);
            const float dx = c[0] - ax, dy = c[1] - ay;
            const float d = sqrtf(dx * dx + dy * dy);
            const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
            if (dt < kQuarter && key < b4) b4 = key;
            if (dt < kHalf && key < b2) b2 = key;
        }
        if (b4 != ~0ull) atomicMin(&s_best[0], b4);
        if (b2 != ~0ull) atomicMin(&s_best[1], b2);
    }
    __syncthreads();
    const unsigned long long best = s_best[0] != ~0ull ? s_best[0] : s_best[1];
    if (best == ~0ull) return;
    const int node_id = (int)(best & 0xffffffffu);
    const int tl = p.lane_idcs[nb + node_id];
    if ((unsigned)tl >= (unsigned)nl) {
        if (tid == 0) atomicOr(status, kStRange);
        return;
    }

    // ---- lane search: suc, then pre
    for (int i = tid; i < W; i += kRoiThreads) s_seen[i] = 0;
    __syncthreads();
    if (tid == 0) {
        s_seen[tl >> 5] = 1u << (tl & 31);
        s_list[0] = tl;
        s_n = 1;
    }
    const float len_t = w.lane_len[lb + tl];
    for (int dir = 0; dir < 2; ++dir) {
        const float thres = dir == 0 ? vel * 3.0f + p.horizon_buffer : vel * 2.0f + p.horizon_buffer;
        const int32_t *pairs = dir == 0 ? p.suc_pairs : p.pre_pairs;
        const int pb = dir == 0 ? t.suc[s] : t.pre[s], pe = dir == 0 ? t.suc[s + 1] : t.pre[s + 1];
        __syncthreads();
        for (int i = tid; i < W; i += kRoiThreads) s_front[i] = 0;
        __syncthreads();
        if (tid == 0) {
            s_front[tl >> 5] = 1u << (tl & 31);
            s_dist = len_t;
        }
        __syncthreads();
        int level = 0;
        for (; level < kRoiMaxLevels; ++level) {
            if (s_dist >= thres) break;
            for (int i = tid; i < W; i += kRoiThreads) s_next[i] = 0;
            if (tid == 0) {
                s_any = 0;
                s_minbits = 0x7f800000u;
            }
            __syncthreads();
            for (int e = pb + tid; e < pe; e += kRoiThreads) {
                const int x = pairs[2 * e], y = pairs[2 * e + 1];
                if ((unsigned)x >= (unsigned)nl || (unsigned)y >= (unsigned)nl) {
                    atomicOr(status, kStRange);
                    continue;
                }
                if (roi_bit(s_front, x)) atomicOr(&s_next[y >> 5], 1u << (y & 31));
            }
            __syncthreads();
            for (int i = tid; i < W; i += kRoiThreads) {
                uint32_t bits = s_next[i];
                if (bits) s_any = 1;
                while (bits) {
                    const int b = __ffs(bits) - 1;
                    bits &= bits - 1;
                    atomicMin(&s_minbits, __float_as_uint(w.lane_len[lb + i * 32 + b]));     // lengths are >= 0
                }
            }
            __syncthreads();
            if (!s_any) break;
            // the level's new lanes, ascending, behind the list
            for (int i = tid; i < W; i += kRoiThreads) {
                uint32_t bits = s_next[i] & ~s_seen[i];
                if (bits) {
                    int pos = s_n;
                    for (int j = 0; j < i; ++j) pos += __popc(s_next[j] & ~s_seen[j]);
                    while (bits) {
                        const int b = __ffs(bits) - 1;
                        bits &= bits - 1;
                        if (pos < kRoiMaxLanes) s_list[pos++] = i * 32 + b;
                    }
                }
            }
            if (tid == 0) {
                int add = 0;
                for (int j = 0; j < W; ++j) add += __popc(s_next[j] & ~s_seen[j]);
                s_add = add;
            }
            __syncthreads();
            for (int i = tid; i < W; i += kRoiThreads) {
                s_seen[i] |= s_next[i];
                s_front[i] = s_next[i];
            }
            if (tid == 0) {
                s_n += s_add;
                s_dist = s_dist + __uint_as_float(s_minbits);
            }
            __syncthreads();
        }
        if (level == kRoiMaxLevels) {
            if (tid == 0) atomicOr(status, kStLevels);
            return;
        }
    }
    __syncthreads();

    // ---- left / right closure over the lanes of the node-level left and right edges
    for (int i = tid; i < W; i += kRoiThreads) s_all[i] = s_cur[i] = s_seen[i];
    __syncthreads();
    bool grew = false;
    for (int it = 0; it <= nl; ++it) {
        for (int i = tid; i < W; i += kRoiThreads) s_next[i] = 0;
        if (tid == 0) s_any = 0;
        __syncthreads();
        for (int r = 12; r < 14; ++r)
            for (int e = t.edge[r * S + s] + tid; e < t.edge[r * S + s + 1]; e += kRoiThreads) {
                const int u = p.edge_u[e], v = p.edge_v[e];
                if ((unsigned)u >= (unsigned)nn || (unsigned)v >= (unsigned)nn) continue;
                const int lu = p.lane_idcs[nb + u], lv = p.lane_idcs[nb + v];
                if ((unsigned)lu >= (unsigned)nl || (unsigned)lv >= (unsigned)nl) continue;
                if (roi_bit(s_cur, lu)) atomicOr(&s_next[lv >> 5], 1u << (lv & 31));
            }
        __syncthreads();
        for (int i = tid; i < W; i += kRoiThreads)
            if (s_next[i] & ~s_all[i]) s_any = 1;
        __syncthreads();
        if (!s_any) break;
        grew = true;
        for (int i = tid; i < W; i += kRoiThreads) {
            s_all[i] |= s_next[i];
            s_cur[i] = s_next[i];
        }
        __syncthreads();
    }

    // ---- lane order, node count, pre[0] / suc[0] edge
    const int slot = t.slot[s] + (a - t.agent[s]) * nl;
    if (tid == 0) s_cnt = s_has = 0;
    if (grew) {      // ascending lane ids
        for (int i = tid; i < W; i += kRoiThreads) {
            uint32_t bits = s_all[i];
            if (bits) {
                int pos = 0;
                for (int j = 0; j < i; ++j) pos += __popc(s_all[j]);
                while (bits) {
                    const int b = __ffs(bits) - 1;
                    bits &= bits - 1;
                    if (pos < nl) w.roi_lanes[slot + pos++] = i * 32 + b;
                }
            }
        }
        if (tid == 0) {
            int n = 0;
            for (int j = 0; j < W; ++j) n += __popc(s_all[j]);
            s_n = n;
        }
    } else {         // search order
        for (int k = tid; k < s_n && k < nl; k += kRoiThreads) w.roi_lanes[slot + k] = s_list[k];
    }
    __syncthreads();
    const int n_l = s_n < nl ? s_n : nl;
    const int32_t *lane_ptr = w.cnt + w.n_keys + lb;
    for (int i = tid; i < W; i += kRoiThreads) {
        uint32_t bits = s_all[i];
        int c = 0;
        while (bits) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1;
            c += lane_ptr[i * 32 + b + 1] - lane_ptr[i * 32 + b];
        }
        if (c) atomicAdd(&s_cnt, c);
    }
    for (int r = 0; r < 12; r += 6)
        for (int e = t.edge[r * S + s] + tid; e < t.edge[r * S + s + 1]; e += kRoiThreads) {
            const int u = p.edge_u[e], v = p.edge_v[e];
            if ((unsigned)u >= (unsigned)nn || (unsigned)v >= (unsigned)nn) continue;
            const int lu = p.lane_idcs[nb + u], lv = p.lane_idcs[nb + v];
            if ((unsigned)lu >= (unsigned)nl || (unsigned)lv >= (unsigned)nl) continue;
            if (roi_bit(s_all, lu) && roi_bit(s_all, lv)) s_has = 1;
        }
    __syncthreads();
    if (tid == 0) {
        w.agent_lanes[a] = n_l;
        p.agent_nodes[a] = (s_cnt >= 6 && s_has) ? s_cnt : 0;
    }
}

// ------------------------------------------------------------------ stage 2: one workgroup per RoI
struct RoiRef {
    int a, s, nl, nb, nn, slot, base, n, n_l;
    bool ok;
};
__device__ __forceinline__ RoiRef roi_ref(const lgcn_roi_t &p, const RoiWs &w, const RoiTabs &t, int r) {
    RoiRef q;
    q.a = p.roi_agent[r];
    q.ok = (unsigned)q.a < (unsigned)p.n_agents;
    if (!q.ok) return q;
    q.s = find_seg(t.agent, p.n_scenes, q.a);
    q.nl = t.lane[q.s + 1] - t.lane[q.s];
    q.nb = t.node[q.s];
    q.nn = t.node[q.s + 1] - q.nb;
    q.slot = t.slot[q.s] + (q.a - t.agent[q.s]) * q.nl;
    q.base = p.roi_base[r];
    q.n = p.roi_base[r + 1] - q.base;
    q.n_l = w.agent_lanes[q.a];
    q.ok = q.base >= 0 && q.n >= 0 && q.base + q.n <= p.n_out_nodes && q.n_l <= q.nl;
    return q;
}

__global__ __launch_bounds__(kRoiThreads) void k_roi_nodes(const lgcn_roi_t p, const RoiWs w) {
    __shared__ int lds[kRoiThreads / 64 + 1];
    const int r = blockIdx.x, tid = threadIdx.x;
    const RoiTabs t = roi_tabs(p.off_dev, p.n_scenes);
    const RoiRef q = roi_ref(p, w, t, r);
    if (!q.ok) return;
    if (tid < 2 * kRoiSteps) {       // agent_feat: (obs x, obs y, step x, step y) per observed step
        const int k = tid >> 1, c = tid & 1;
        p.agent_feat[(int64_t)r * 80 + 4 * k + c] = p.a_obs[((int64_t)q.a * kRoiSteps + k) * 2 + c];
        p.agent_feat[(int64_t)r * 80 + 4 * k + 2 + c] = p.a_feats[((int64_t)q.a * kRoiSteps + k) * 2 + c];
    }
    for (int l = tid; l < q.nl; l += kRoiThreads) w.roi_lane_off[q.slot + l] = -1;
    __syncthreads();
    const int32_t *lane_ptr = w.cnt + w.n_keys + t.lane[q.s];
    const int ptr0 = w.cnt[w.n_keys];
    const float ax = p.a_ctrs[2 * q.a], ay = p.a_ctrs[2 * q.a + 1];
    int carry = 0;
    for (int c0 = 0; c0 < q.n_l; c0 += kRoiThreads) {
        const int k = c0 + tid;
        int l = k < q.n_l ? w.roi_lanes[q.slot + k] : -1;
        if ((unsigned)l >= (unsigned)q.nl) l = -1;
        const int cnt = l >= 0 ? lane_ptr[l + 1] - lane_ptr[l] : 0;
        int total;
        const int pre = block_exclusive_scan<kRoiThreads>(cnt, &total, lds) + carry;
        carry += total;
        if (l < 0) continue;
        w.roi_lane_off[q.slot + l] = pre;
        const int32_t *nodes = w.lane_nodes + (lane_ptr[l] - ptr0);
        for (int j = 0; j < cnt; ++j) {
            const int lo = pre + j;
            if (lo >= q.n) break;
            const int g = nodes[j];
            const int64_t gi = q.nb + g, o = q.base + lo;
            p.node_mask[o] = g;
            float *row = p.out_feats + 8 * o;
            const float cx = p.ctrs[2 * gi], cy = p.ctrs[2 * gi + 1];
            row[0] = cx;                  row[1] = cy;
            row[2] = p.feats[2 * gi];     row[3] = p.feats[2 * gi + 1];
            row[4] = p.turn[2 * gi];      row[5] = p.turn[2 * gi + 1];
            row[6] = p.control[gi];       row[7] = p.intersect[gi];
            const float dx = cx - ax, dy = cy - ay;
            p.near[o] = sqrtf(dx * dx + dy * dy) < 5.0f;
        }
    }
}

// ------------------------------------------------------------------ stage 3: one workgroup per (RoI, relation | a2m)
// local index of scene node v in the RoI, -1 outside
__device__ __forceinline__ int roi_local(const lgcn_roi_t &p, const RoiWs &w, const RoiRef &q, int v) {
    const int l = p.lane_idcs[q.nb + v];
    if ((unsigned)l >= (unsigned)q.nl) return -1;
    const int lo = w.roi_lane_off[q.slot + l];
    return lo < 0 ? -1 : lo + w.node_rank[q.nb + v];
}

// edges of local row lu in relation rel: count, and with out != nullptr the local v's, ascending
__device__ __forceinline__ int roi_row(const lgcn_roi_t &p, const RoiWs &w, const RoiRef &q, int rel, int lu, int64_t *out,
                                       int cap) {
    const int g = (int)p.node_mask[q.base + lu];
    if ((unsigned)g >= (unsigned)q.nn) return 0;
    const int64_t key = (int64_t)rel * p.n_nodes + q.nb + g;
    int c = 0, prev = -1;
    for (int e = w.cnt[key]; e < w.cnt[key + 1]; ++e) {
        const int v = w.col[e];
        if (v == prev || (unsigned)v >= (unsigned)q.nn) continue;      // a pair listed twice counts once
        prev = v;
        const int lv = roi_local(p, w, q, v);
        if (lv < 0) continue;
        if (out != nullptr && c < cap) {   // insertion into the sorted prefix
            int j = c - 1;
            for (; j >= 0 && out[j] > lv; --j) out[j + 1] = out[j];
            out[j + 1] = lv;
        }
        ++c;
    }
    return c;
}

__global__ __launch_bounds__(kRoiThreads) void k_roi_edge_count(const lgcn_roi_t p, const RoiWs w) {
    __shared__ int s_cnt;
    const int r = blockIdx.x / (kRoiRel + 1), rel = blockIdx.x % (kRoiRel + 1), tid = threadIdx.x;
    const RoiTabs t = roi_tabs(p.off_dev, p.n_scenes);
    const RoiRef q = roi_ref(p, w, t, r);
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int c = 0;
    if (q.ok)
        for (int lu = tid; lu < q.n; lu += kRoiThreads)
            c += rel == kRoiRel ? (p.near[q.base + lu] != 0) : roi_row(p, w, q, rel, lu, nullptr, 0);
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid == 0) p.edge_cnt[blockIdx.x] = s_cnt;
}

// kGraph = false: RoI-local (u, v) at the host's edge_base, a2m_v int32 (lgcn_roi_edge_fill).  kGraph = true: the indices
// of the batch's merged block-diagonal graph (lgcn_roi_edge_fill_graph): u and v shifted by the RoI's node offset,
// a2m as (RoI number, shifted node) in the int64 arrays g_u / g_v -- the same rows at the same scan positions, so where a
// row holds one edge consecutive lanes still write consecutive words of out_u / out_v.
template <bool kGraph>
__global__ __launch_bounds__(kRoiThreads) void k_roi_edge_fill(const lgcn_roi_t p, const RoiWs w, int64_t *g_u, int64_t *g_v) {
    __shared__ int lds[kRoiThreads / 64 + 1];
    const int r = blockIdx.x / (kRoiRel + 1), rel = blockIdx.x % (kRoiRel + 1), tid = threadIdx.x;
    const RoiTabs t = roi_tabs(p.off_dev, p.n_scenes);
    const RoiRef q = roi_ref(p, w, t, r);
    if (!q.ok) return;
    const int64_t limit = rel == kRoiRel ? p.n_out_a2m : p.n_out_edges;
    int carry = p.edge_base[blockIdx.x];
    if (carry < 0) return;
    for (int c0 = 0; c0 < q.n; c0 += kRoiThreads) {
        const int lu = c0 + tid;
        int c = 0;
        if (lu < q.n) c = rel == kRoiRel ? (p.near[q.base + lu] != 0) : roi_row(p, w, q, rel, lu, nullptr, 0);
        int total;
        const int pre = block_exclusive_scan<kRoiThreads>(c, &total, lds) + carry;
        carry += total;
        if (c == 0 || (int64_t)pre + c > limit) continue;
        if (rel == kRoiRel) {
            if (kGraph) {
                g_u[pre] = r;
                g_v[pre] = (int64_t)q.base + lu;
            } else {
                p.a2m_v[pre] = lu;
            }
        } else {
            roi_row(p, w, q, rel, lu, p.out_v + pre, c);
            if (kGraph) {
                for (int j = 0; j < c; ++j) {
                    p.out_v[pre + j] += q.base;
                    p.out_u[pre + j] = (int64_t)q.base + lu;
                }
            } else {
                for (int j = 0; j < c; ++j) p.out_u[pre + j] = lu;
            }
        }
    }
}

// ------------------------------------------------------------------ host side
// everything lgcn_roi_search reads; stage >= 2 adds the RoI tables, 3 the counts, 4 the edge outputs
static int roi_validate(const lgcn_roi_t *p, int stage) {
    if (p == nullptr) return LGCN_EINVAL;
    if (p->n_scenes < 0 || p->n_agents < 0 || p->n_nodes < 0 || p->n_lanes < 0 || p->n_edges < 0 || p->n_slots < 0 ||
        p->n_suc < 0 || p->n_pre < 0 || p->n_rois < 0 || p->n_out_nodes < 0 || p->n_out_edges < 0 || p->n_out_a2m < 0)
        return LGCN_EINVAL;
    if (!(p->horizon_buffer == p->horizon_buffer)) return LGCN_EINVAL;
    if (p->n_scenes == 0) return (p->n_agents | p->n_nodes | p->n_lanes | p->n_edges | p->n_rois) ? LGCN_EINVAL : LGCN_OK;
    LGCN_CHECK_PTR(p->off_host);
    const int S = p->n_scenes;
    if ((int64_t)S * (kRoiRel + 6) + 7 > 0x7fffffff) return LGCN_ESHAPE;
    const RoiTabs t = roi_tabs(p->off_host, S);
    const int64_t totals[6] = {p->n_nodes, p->n_lanes, p->n_agents, p->n_slots, p->n_suc, p->n_pre};
    const int32_t *tabs[6] = {t.node, t.lane, t.agent, t.slot, t.suc, t.pre};
    for (int i = 0; i < 6; ++i)
        if (int rc = check_table(tabs[i], S, totals[i])) return rc;
    if (int rc = check_table(t.edge, kRoiRel * S, p->n_edges)) return rc;
    for (int s = 0; s < S; ++s) {
        const int64_t nl = t.lane[s + 1] - t.lane[s], na = t.agent[s + 1] - t.agent[s];
        if (nl > kRoiMaxLanes) return LGCN_ESHAPE;
        if ((int64_t)t.slot[s + 1] - t.slot[s] != nl * na) return LGCN_EINVAL;
    }
    const int64_t ws = lgcn_roi_ws_elems(p->n_nodes, p->n_lanes, p->n_edges, p->n_slots, p->n_agents);
    if (ws < 0) return (int)ws;
    LGCN_CHECK_PTR(p->off_dev); LGCN_CHECK_PTR(p->ws); LGCN_CHECK_PTR(p->agent_nodes); LGCN_CHECK_PTR(p->agent_vel);
    if (p->n_nodes > 0) {
        LGCN_CHECK_PTR(p->ctrs); LGCN_CHECK_PTR(p->feats); LGCN_CHECK_PTR(p->turn); LGCN_CHECK_PTR(p->control);
        LGCN_CHECK_PTR(p->intersect); LGCN_CHECK_PTR(p->lane_idcs);
    }
    if (p->n_agents > 0) { LGCN_CHECK_PTR(p->a_ctrs); LGCN_CHECK_PTR(p->a_feats); LGCN_CHECK_PTR(p->a_obs); }
    if (p->n_suc > 0) LGCN_CHECK_PTR(p->suc_pairs);
    if (p->n_pre > 0) LGCN_CHECK_PTR(p->pre_pairs);
    if (p->n_edges > 0) { LGCN_CHECK_PTR(p->edge_u); LGCN_CHECK_PTR(p->edge_v); }
    if (stage >= 2 && p->n_rois > 0) {
        LGCN_CHECK_PTR(p->roi_agent); LGCN_CHECK_PTR(p->roi_base); LGCN_CHECK_PTR(p->agent_feat);
        if (p->n_out_nodes > 0) { LGCN_CHECK_PTR(p->node_mask); LGCN_CHECK_PTR(p->out_feats); LGCN_CHECK_PTR(p->near); }
        if ((int64_t)p->n_rois * (kRoiRel + 1) > 0x7fffffff) return LGCN_ESHAPE;
    }
    if (stage == 3 && p->n_rois > 0) LGCN_CHECK_PTR(p->edge_cnt);
    if (stage == 4 && p->n_rois > 0) {
        LGCN_CHECK_PTR(p->edge_base);
        if (p->n_out_edges > 0) { LGCN_CHECK_PTR(p->out_u); LGCN_CHECK_PTR(p->out_v); }
        if (p->n_out_a2m > 0) LGCN_CHECK_PTR(p->a2m_v);
    }
    LGCN_CHECK_ALIGN16(p->ws); LGCN_CHECK_ALIGN16(p->ctrs); LGCN_CHECK_ALIGN16(p->feats); LGCN_CHECK_ALIGN16(p->turn);
    LGCN_CHECK_ALIGN16(p->a_ctrs);
    const void *words[] = {p->off_dev, p->control, p->intersect, p->lane_idcs, p->a_feats, p->a_obs, p->suc_pairs, p->pre_pairs,
                           p->edge_u, p->edge_v, p->agent_nodes, p->agent_vel, p->roi_agent, p->roi_base, p->out_feats,
                           p->agent_feat, p->near, p->edge_cnt, p->edge_base, p->a2m_v};
    for (const void *q : words)
        if (misaligned(q, 3u)) return LGCN_EALIGN;
    const void *dwords[] = {p->node_mask, p->out_u, p->out_v};
    for (const void *q : dwords)
        if (misaligned(q, 7u)) return LGCN_EALIGN;
    return LGCN_OK;
}

static inline unsigned roi_blocks(int64_t n) { return (unsigned)((n + kRoiThreads - 1) / kRoiThreads); }

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int lgcn_roi_max_lanes(void) { return kRoiMaxLanes; }
int lgcn_roi_max_levels(void) { return kRoiMaxLevels; }

float lgcn_roi_lane_length_host(const float *feats, const int32_t *nodes, int n) {
    if (n < 0 || (n > 0 && (feats == nullptr || nodes == nullptr))) return __builtin_nanf("");
    return roi_lane_length(nodes, n, feats);
}

int64_t lgcn_roi_ws_elems(int64_t n_nodes, int64_t n_lanes, int64_t n_edges, int64_t n_slots, int64_t n_agents) {
    if (n_nodes < 0 || n_lanes < 0 || n_edges < 0 || n_slots < 0 || n_agents < 0) return LGCN_EINVAL;
    const int64_t lim = 0x7fffffff;
    if (n_nodes > lim / 64 || n_lanes > lim / 8 || n_edges > lim / 4 || n_slots > lim / 8 || n_agents > lim / 4) return LGCN_ESHAPE;
    const int64_t total = roi_ws(nullptr, n_nodes, n_lanes, n_edges, n_slots, n_agents).total;
    return total > lim ? (int64_t)LGCN_ESHAPE : total;
}

int lgcn_roi_search(const lgcn_roi_t *p, void *stream) {
    if (int rc = roi_validate(p, 1)) return rc;
    if (p->n_agents == 0) return LGCN_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RoiWs w = roi_ws(p->ws, p->n_nodes, p->n_lanes, p->n_edges, p->n_slots, p->n_agents);
    // cursor and the row counts are adjacent: one memset
    if (hipMemsetAsync(w.cursor, 0, sizeof(int32_t) * (size_t)(up4(w.n_keys) + w.n_keys), st) != hipSuccess)
        return launch_status();
    hipLaunchKernelGGL(k_roi_lane_count, dim3(roi_blocks(p->n_lanes + 1)), dim3(kRoiThreads), 0, st, *p, w);
    if (p->n_edges > 0)
        hipLaunchKernelGGL(k_roi_edge_rows, dim3(roi_blocks(p->n_edges)), dim3(kRoiThreads), 0, st, *p, w);
    if (int rc = exclusive_scan(w.cnt, w.cnt, w.n_scan, w.sums, st)) return rc;
    if (p->n_lanes > 0)
        hipLaunchKernelGGL(k_roi_lane_fill, dim3(roi_blocks(p->n_lanes)), dim3(kRoiThreads), 0, st, *p, w);
    if (p->n_edges > 0) {
        hipLaunchKernelGGL(k_roi_edge_fill_rows, dim3(roi_blocks(p->n_edges)), dim3(kRoiThreads), 0, st, *p, w);
        hipLaunchKernelGGL(k_roi_sort_rows, dim3(roi_blocks(w.n_keys)), dim3(kRoiThreads), 0, st, w);
    }
    hipLaunchKernelGGL(k_roi_search, dim3((unsigned)p->n_agents), dim3(kRoiThreads), 0, st, *p, w);
    return launch_status();
}

int lgcn_roi_nodes(const lgcn_roi_t *p, void *stream) {
    if (int rc = roi_validate(p, 2)) return rc;
    if (p->n_rois == 0) return LGCN_OK;
    const RoiWs w = roi_ws(p->ws, p->n_nodes, p->n_lanes, p->n_edges, p->n_slots, p->n_agents);
    hipLaunchKernelGGL(k_roi_nodes, dim3((unsigned)p->n_rois), dim3(kRoiThreads), 0, static_cast<hipStream_t>(stream), *p, w);
    return launch_status();
}

int lgcn_roi_edge_count(const lgcn_roi_t *p, void *stream) {
    if (int rc = roi_validate(p, 3)) return rc;
    if (p->n_rois == 0) return LGCN_OK;
    const RoiWs w = roi_ws(p->ws, p->n_nodes, p->n_lanes, p->n_edges, p->n_slots, p->n_agents);
    hipLaunchKernelGGL(k_roi_edge_count, dim3((unsigned)(p->n_rois * (kRoiRel + 1))), dim3(kRoiThreads), 0,
                       static_cast<hipStream_t>(stream), *p, w);
    return launch_status();
}

int lgcn_roi_edge_fill(const lgcn_roi_t *p, void *stream) {
    if (int rc = roi_validate(p, 4)) return rc;
    if (p->n_rois == 0) return LGCN_OK;
    const RoiWs w = roi_ws(p->ws, p->n_nodes, p->n_lanes, p->n_edges, p->n_slots, p->n_agents);
    hipLaunchKernelGGL(k_roi_edge_fill<false>, dim3((unsigned)(p->n_rois * (kRoiRel + 1))), dim3(kRoiThreads), 0,
                       static_cast<hipStream_t>(stream), *p, w, nullptr, nullptr);
    return launch_status();
}

// Replaces, with lane_roi_flat on the Python side, the reference's per-RoI index arrays (data_lrcnn.py:690-844) and their
// merge into one block-diagonal graph (lanercnn.py:122-231, subgraph_gather): the merged indices are written here.
int lgcn_roi_edge_fill_graph(const lgcn_roi_t *p, int64_t *a2m_u, int64_t *a2m_v, void *stream) {
    if (p == nullptr) return LGCN_EINVAL;
    lgcn_roi_t g = *p;      // stage 4 of the sibling, with the int64 a2m_v in the place of its int32 one
    g.a2m_v = reinterpret_cast<int32_t *>(a2m_v);
    if (int rc = roi_validate(&g, 4)) return rc;
    if (g.n_rois > 0 && g.n_out_a2m > 0) LGCN_CHECK_PTR(a2m_u);
    if (misaligned(a2m_u, 7u) || misaligned(a2m_v, 7u)) return LGCN_EALIGN;
    if (g.n_rois == 0) return LGCN_OK;
    const RoiWs w = roi_ws(g.ws, g.n_nodes, g.n_lanes, g.n_edges, g.n_slots, g.n_agents);
    hipLaunchKernelGGL(k_roi_edge_fill<true>, dim3((unsigned)(g.n_rois * (kRoiRel + 1))), dim3(kRoiThreads), 0,
                       static_cast<hipStream_t>(stream), g, w, a2m_u, a2m_v);
    return launch_status();
}

}  // extern "C"
