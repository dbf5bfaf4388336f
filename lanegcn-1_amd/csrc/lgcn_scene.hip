// Scene construction for a batch of raw scenes (reference data.py:148-217 get_obj_feats, :220-361 get_lane_graph at
// scale 0): tracks -> actor arrays, map lanes -> lane graph.  See include/lgcn.h and DESIGN.md section 3.11.
//
// Arithmetic: a point goes into the scene frame as d = p - (double)orig, x' = r00 * dx + r01 * dy in float64 with the two
// products and the sum rounded separately (__dmul_rn / __dadd_rn: never an FMA).  Order comes from prefix scans only
// (block scan + per-block sums, so a scene may span any number of workgroups); the one atomic is an integer maximum.
#include "lgcn_common.hpp"
#include "lgcn_blockscan.hpp"

namespace lgcn {

constexpr int kScObs = 20, kScFut = 30;

struct ScFrame {
    double ox, oy, r00, r01, r10, r11;
};
__device__ __forceinline__ ScFrame sc_frame(const float *f) {       // [orig x, y, rot 00, 01, 10, 11]
    ScFrame q;
    q.ox = (double)f[0]; q.oy = (double)f[1];
    q.r00 = (double)f[2]; q.r01 = (double)f[3]; q.r10 = (double)f[4]; q.r11 = (double)f[5];
    return q;
}
__device__ __forceinline__ void sc_xform(const ScFrame &q, const double *p, double *x, double *y) {
    const double dx = __dsub_rn(p[0], q.ox), dy = __dsub_rn(p[1], q.oy);
    *x = __dadd_rn(__dmul_rn(q.r00, dx), __dmul_rn(q.r01, dy));
    *y = __dadd_rn(__dmul_rn(q.r10, dx), __dmul_rn(q.r11, dy));
}

// ------------------------------------------------------------------ tracks
struct ScTrkWs {
    int32_t *loc, *keep, *sums;      // [T + 1], [T + 1], [blocks]
};
__host__ __device__ inline ScTrkWs sc_trk_ws(int32_t *ws, int64_t T) {
    ScTrkWs w;
    w.loc = ws;
    w.keep = ws + up4(T + 1);
    w.sums = ws + 2 * up4(T + 1);
    return w;
}

// One thread per track: which steps it holds, whether it is kept (step 19 present and inside pred_range), and the kept
// tracks in front of it in its block.  keep word: 0 = dropped, else 1 + the first step of the run that ends at 19.
__global__ __launch_bounds__(kScThreads) void k_scene_track_flag(const lgcn_scene_tracks_t p, const ScTrkWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int T = p.n_tracks, S = p.n_scenes;
    const int t = blockIdx.x * kScThreads + threadIdx.x;
    const int32_t *trk_off = p.off_dev, *row_off = p.off_dev + (S + 1);
    int v[1] = {0}, word = 0;
    if (t < T) {
        const int s = find_seg(trk_off, S, t);
        unsigned long long mask = 0;
        bool dup = false;
        int r19 = -1;
        for (int r = row_off[t]; r < row_off[t + 1]; ++r) {
            const int st = p.step[r];
            if ((unsigned)st < (unsigned)(kScObs + kScFut)) {
                const unsigned long long bit = 1ull << st;
                dup |= (mask & bit) != 0;
                mask |= bit;
                if (st == kScObs - 1) r19 = r;
            }
        }
        if (dup) atomicMax(&p.head[S + 1], T - t);        // the FIRST such track wins
        if (r19 >= 0) {
            const ScFrame q = sc_frame(p.frame + 6 * s);
            double x, y;
            sc_xform(q, p.xy + 2 * (int64_t)r19, &x, &y);
            const float fx = (float)x, fy = (float)y;
            if (!(fx < p.pred_range[0] || fx > p.pred_range[1] || fy < p.pred_range[2] || fy > p.pred_range[3])) {
                const unsigned gaps = ~(unsigned)mask & 0xfffffu;       // missing observed steps
                const int first = gaps ? 32 - __clz(gaps) : 0;         // one past the last gap
                word = 1 + first;
                v[0] = 1;
            }
        }
    }
    int excl[1];
    sc_scan_local<1>(v, excl, w.sums, lds);
    if (t <= T) {
        w.loc[t] = excl[0];
        w.keep[t] = word;
    }
}

__global__ __launch_bounds__(kScThreads) void k_scene_track_fill(const lgcn_scene_tracks_t p, const ScTrkWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int T = p.n_tracks, S = p.n_scenes;
    const int t = blockIdx.x * kScThreads + threadIdx.x;
    const int32_t *trk_off = p.off_dev, *row_off = p.off_dev + (S + 1);
    int base[1];
    sc_block_base<1>(w.sums, base, lds);
    if (t > T) return;
    const int64_t o = base[0] + w.loc[t];
    if (t == T) {
        p.head[S] = (int)o;
        return;
    }
    const int s = find_seg(trk_off, S, t);
    if (t == trk_off[s]) p.head[s] = (int)o;
    const int word = w.keep[t];
    if (word == 0 || o >= T) return;
    const int first = word - 1;
    float *obs = p.obs + o * (kScObs * 3), *feats = p.feats + o * (kScObs * 3), *gt = p.gt + o * (kScFut * 2);
    unsigned char *has = p.has + o * kScFut;
    for (int k = 0; k < kScObs * 3; ++k) obs[k] = 0.f;
    for (int k = 0; k < kScFut * 2; ++k) gt[k] = 0.f;
    for (int k = 0; k < kScFut; ++k) has[k] = 0;
    const ScFrame q = sc_frame(p.frame + 6 * s);
    for (int r = row_off[t]; r < row_off[t + 1]; ++r) {
        const int st = p.step[r];
        const double *xy = p.xy + 2 * (int64_t)r;
        if (st >= kScObs && st < kScObs + kScFut) {          // the future stays in world coordinates
            gt[2 * (st - kScObs)] = (float)xy[0];
            gt[2 * (st - kScObs) + 1] = (float)xy[1];
            has[st - kScObs] = 1;
        } else if (st >= first && st < kScObs) {
            double x, y;
            sc_xform(q, xy, &x, &y);
            obs[3 * st] = (float)x;
            obs[3 * st + 1] = (float)y;
            obs[3 * st + 2] = 1.f;
        }
    }
    p.ctrs[2 * o] = obs[3 * (kScObs - 1)];
    p.ctrs[2 * o + 1] = obs[3 * (kScObs - 1) + 1];
    for (int k = 0; k < kScObs; ++k) {                       // fp32 differences of the rounded positions
        float fx = 0.f, fy = 0.f;
        if (k > first) {
            fx = obs[3 * k] - obs[3 * (k - 1)];
            fy = obs[3 * k + 1] - obs[3 * (k - 1) + 1];
        }
        feats[3 * k] = fx;
        feats[3 * k + 1] = fy;
        feats[3 * k + 2] = k >= first ? 1.f : 0.f;
    }
}

// ------------------------------------------------------------------ lanes
struct ScTopo {      // views into one table's int32 block
    const int32_t *pt_off, *pred_off, *succ_off, *left, *right, *flags, *pred, *succ;
};
__host__ __device__ inline ScTopo sc_topo(const int32_t *t, int64_t L, int64_t n_pred) {
    ScTopo q;
    q.pt_off = t;
    q.pred_off = t + (L + 1);
    q.succ_off = t + 2 * (L + 1);
    q.left = t + 3 * (L + 1);
    q.right = q.left + L;
    q.flags = q.right + L;
    q.pred = q.flags + L;
    q.succ = q.pred + n_pred;
    return q;
}

struct ScLaneWs {
    int32_t *rank_of, *node_of;      // [n_rank] each, adjacent (one memset): global kept-lane index / first node, -1 = not kept
    int32_t *keep, *loc, *glob, *loc2, *sums, *sums2;
    int64_t total;
};
__host__ __device__ inline ScLaneWs sc_lane_ws(int32_t *ws, int64_t n_cand, int64_t n_rank) {
    ScLaneWs w;
    int64_t o = 0;
    w.rank_of = ws + o; o += up4(n_rank);
    w.node_of = ws + o; o += up4(n_rank);
    w.keep = ws + o;    o += up4(n_cand + 1);
    w.loc = ws + o;     o += 4 * up4(n_cand + 1);
    w.glob = ws + o;    o += 4 * up4(n_cand + 1);
    w.loc2 = ws + o;    o += 4 * up4(n_cand + 1);
    w.sums = ws + o;    o += 4 * up4(sc_blocks(n_cand + 1));
    w.sums2 = ws + o;   o += 4 * up4(sc_blocks(n_cand + 1));
    w.total = o;
    return w;
}

struct ScTabs {      // the tables inside lgcn_scene_lanes_t::off_*
    const int32_t *scene_tab, *cand_off, *rank_off, *cand;
};
__host__ __device__ inline ScTabs sc_tabs(const int32_t *off, int S) {
    ScTabs t;
    t.scene_tab = off;
    t.cand_off = off + S;
    t.rank_off = off + S + (S + 1);
    t.cand = off + S + 2 * (S + 1);
    return t;
}

struct ScCand {
    int s, lane, p0, p1, ro;
    ScTopo tp;
    const double *pts;
};
__device__ __forceinline__ ScCand sc_cand(const lgcn_scene_lanes_t &p, const ScTabs &t, int c) {
    ScCand q;
    q.s = find_seg(t.cand_off, p.n_scenes, c);
    const lgcn_lane_table_t *tb = p.tabs_dev + t.scene_tab[q.s];
    q.lane = p.explicit_ids ? t.cand[c] : c - t.cand_off[q.s];
    q.tp = sc_topo(tb->topo_dev, tb->n_lanes, tb->n_pred);
    q.pts = tb->pts;
    q.p0 = q.tp.pt_off[q.lane];
    q.p1 = q.tp.pt_off[q.lane + 1];
    q.ro = t.rank_off[q.s];
    return q;
}

// One thread per candidate lane: its extent in the scene frame against the pred_range rectangle (data.py:231-233), and
// the block-local scans of (kept lanes, their nodes, their predecessor and successor entries).
__global__ __launch_bounds__(kScThreads) void k_scene_lane_flag(const lgcn_scene_lanes_t p, const ScLaneWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int c = blockIdx.x * kScThreads + threadIdx.x;
    const ScTabs t = sc_tabs(p.off_dev, p.n_scenes);
    int v[4] = {0, 0, 0, 0};
    if (c < p.n_cand) {
        const ScCand q = sc_cand(p, t, c);
        const ScFrame f = sc_frame(p.frame + 6 * q.s);
        double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        for (int i = q.p0; i < q.p1; ++i) {
            double x, y;
            sc_xform(f, q.pts + 2 * (int64_t)i, &x, &y);
            if (i == q.p0) {
                x0 = x1 = x;
                y0 = y1 = y;
            } else {
                x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
                y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
            }
        }
        if (!(x1 < p.pred_range[0] || x0 > p.pred_range[1] || y1 < p.pred_range[2] || y0 > p.pred_range[3])) {
            v[0] = 1;
            v[1] = q.p1 - q.p0 - 1;
            v[2] = q.tp.pred_off[q.lane + 1] - q.tp.pred_off[q.lane];
            v[3] = q.tp.succ_off[q.lane + 1] - q.tp.succ_off[q.lane];
        }
    }
    int excl[4];
    sc_scan_local<4>(v, excl, w.sums, lds);
    if (c <= p.n_cand) {
        w.keep[c] = v[0];
#pragma unroll
        for (int k = 0; k < 4; ++k) w.loc[4 * (int64_t)c + k] = excl[k];
    }
}

// The scans made global; every kept lane's rank and first node by table row; per scene the offsets for the host.
__global__ __launch_bounds__(kScThreads) void k_scene_lane_rank(const lgcn_scene_lanes_t p, const ScLaneWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int c = blockIdx.x * kScThreads + threadIdx.x;
    const ScTabs t = sc_tabs(p.off_dev, p.n_scenes);
    int base[4];
    sc_block_base<4>(w.sums, base, lds);
    if (c > p.n_cand) return;
    int g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        g[k] = base[k] + w.loc[4 * (int64_t)c + k];
        w.glob[4 * (int64_t)c + k] = g[k];
    }
    if (c == p.n_cand) {
        for (int k = 0; k < 4; ++k) p.head[4 * p.n_scenes + k] = g[k];
        return;
    }
    const ScCand q = sc_cand(p, t, c);
    if (c == t.cand_off[q.s])
        for (int k = 0; k < 4; ++k) p.head[4 * q.s + k] = g[k];
    if (w.keep[c]) {
        w.rank_of[q.ro + q.lane] = g[0];
        w.node_of[q.ro + q.lane] = g[1];
    }
}

// kept predecessors / successors / left / right of every kept lane: a read of the rank array per neighbour
__global__ __launch_bounds__(kScThreads) void k_scene_lane_count(const lgcn_scene_lanes_t p, const ScLaneWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int c = blockIdx.x * kScThreads + threadIdx.x;
    const ScTabs t = sc_tabs(p.off_dev, p.n_scenes);
    int v[4] = {0, 0, 0, 0};
    if (c < p.n_cand && w.keep[c]) {
        const ScCand q = sc_cand(p, t, c);
        const int32_t *rank = w.rank_of + q.ro;
        for (int e = q.tp.pred_off[q.lane]; e < q.tp.pred_off[q.lane + 1]; ++e) {
            const int j = q.tp.pred[e];
            v[0] += j >= 0 && rank[j] >= 0;
        }
        for (int e = q.tp.succ_off[q.lane]; e < q.tp.succ_off[q.lane + 1]; ++e) {
            const int j = q.tp.succ[e];
            v[1] += j >= 0 && rank[j] >= 0;
        }
        const int l = q.tp.left[q.lane], r = q.tp.right[q.lane];
        v[2] = l >= 0 && rank[l] >= 0;
        v[3] = r >= 0 && rank[r] >= 0;
    }
    int excl[4];
    sc_scan_local<4>(v, excl, w.sums2, lds);
    if (c <= p.n_cand) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w.loc2[4 * (int64_t)c + k] = excl[k];
    }
}

__global__ __launch_bounds__(kScThreads) void k_scene_lane_fill(const lgcn_scene_lanes_t p, const ScLaneWs w) {
    __shared__ int lds[kScThreads / 64 + 1];
    const int c = blockIdx.x * kScThreads + threadIdx.x;
    const ScTabs t = sc_tabs(p.off_dev, p.n_scenes);
    int base[4];
    sc_block_base<4>(w.sums2, base, lds);
    if (c > p.n_cand) return;
    int g2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) g2[k] = base[k] + w.loc2[4 * (int64_t)c + k];
    if (c == p.n_cand) {
        for (int k = 0; k < 4; ++k) p.head2[4 * p.n_scenes + k] = g2[k];
        return;
    }
    const ScCand q = sc_cand(p, t, c);
    if (c == t.cand_off[q.s])
        for (int k = 0; k < 4; ++k) p.head2[4 * q.s + k] = g2[k];
    if (!w.keep[c]) return;
    const int32_t *gs = w.glob + 4 * (int64_t)t.cand_off[q.s];      // the scene's first candidate: its offsets
    const int32_t *gc = w.glob + 4 * (int64_t)c;
    const int64_t lane_g = gc[0], nb = gc[1];
    const int64_t i_loc = lane_g - gs[0], nb_loc = nb - gs[1];
    const int nseg = q.p1 - q.p0 - 1;
    const int32_t *rank = w.rank_of + q.ro, *node = w.node_of + q.ro;

    // ---- nodes (data.py:244-263): midpoints and differences of the transformed points in float64, rounded once
    const ScFrame f = sc_frame(p.frame + 6 * q.s);
    const int fl = q.tp.flags[q.lane];
    const float t_l = (fl & 0xff) == 1 ? 1.f : 0.f, t_r = (fl & 0xff) == 2 ? 1.f : 0.f;
    const float ctl = ((fl >> 8) & 0xff) ? 1.f : 0.f, isc = ((fl >> 16) & 0xff) ? 1.f : 0.f;
    double ax, ay;
    sc_xform(f, q.pts + 2 * (int64_t)q.p0, &ax, &ay);
    for (int k = 0; k < nseg; ++k) {
        double bx, by;
        sc_xform(f, q.pts + 2 * (int64_t)(q.p0 + k + 1), &bx, &by);
        const int64_t o = nb + k;
        if (o < p.n_nodes) {
            p.ctrs[2 * o] = (float)(__dadd_rn(ax, bx) / 2.0);
            p.ctrs[2 * o + 1] = (float)(__dadd_rn(ay, by) / 2.0);
            p.feats[2 * o] = (float)__dsub_rn(bx, ax);
            p.feats[2 * o + 1] = (float)__dsub_rn(by, ay);
            p.turn[2 * o] = t_l;
            p.turn[2 * o + 1] = t_r;
            p.control[o] = ctl;
            p.intersect[o] = isc;
            p.lane_idcs[o] = i_loc;
        }
        ax = bx;
        ay = by;
    }

    // ---- pre[0] / suc[0] (data.py:275-295) and the lane pairs (:302-334)
    int64_t pe = (nb - lane_g) + g2[0], se = (nb - lane_g) + g2[1];      // chain edges in front + kept neighbours in front
    int64_t pp = g2[0], sp = g2[1];
    for (int k = 0; k + 1 < nseg; ++k, ++pe, ++se) {
        if (pe < p.cap_pre) {
            p.pre_u[pe] = nb_loc + k + 1;
            p.pre_v[pe] = nb_loc + k;
        }
        if (se < p.cap_suc) {
            p.suc_u[se] = nb_loc + k;
            p.suc_v[se] = nb_loc + k + 1;
        }
    }
    for (int e = q.tp.pred_off[q.lane]; e < q.tp.pred_off[q.lane + 1]; ++e) {
        const int j = q.tp.pred[e];
        if (j < 0 || rank[j] < 0) continue;
        const int nseg_j = q.tp.pt_off[j + 1] - q.tp.pt_off[j] - 1;
        if (pe < p.cap_pre) {
            p.pre_u[pe] = nb_loc;
            p.pre_v[pe] = (int64_t)node[j] - gs[1] + nseg_j - 1;
        }
        if (pp < p.cap_pre_pairs) {
            p.pre_pairs[2 * pp] = i_loc;
            p.pre_pairs[2 * pp + 1] = (int64_t)rank[j] - gs[0];
        }
        ++pe;
        ++pp;
    }
    for (int e = q.tp.succ_off[q.lane]; e < q.tp.succ_off[q.lane + 1]; ++e) {
        const int j = q.tp.succ[e];
        if (j < 0 || rank[j] < 0) continue;
        if (se < p.cap_suc) {
            p.suc_u[se] = nb_loc + nseg - 1;
            p.suc_v[se] = (int64_t)node[j] - gs[1];
        }
        if (sp < p.cap_suc_pairs) {
            p.suc_pairs[2 * sp] = i_loc;
            p.suc_pairs[2 * sp + 1] = (int64_t)rank[j] - gs[0];
        }
        ++se;
        ++sp;
    }
    const int l = q.tp.left[q.lane], r = q.tp.right[q.lane];
    if (l >= 0 && rank[l] >= 0 && g2[2] < p.cap_left_pairs) {
        p.left_pairs[2 * (int64_t)g2[2]] = i_loc;
        p.left_pairs[2 * (int64_t)g2[2] + 1] = (int64_t)rank[l] - gs[0];
    }
    if (r >= 0 && rank[r] >= 0 && g2[3] < p.cap_right_pairs) {
        p.right_pairs[2 * (int64_t)g2[3]] = i_loc;
        p.right_pairs[2 * (int64_t)g2[3] + 1] = (int64_t)rank[r] - gs[0];
    }
}

// ------------------------------------------------------------------ host side
static int sc_tracks_validate(const lgcn_scene_tracks_t *p) {
    if (p == nullptr) return LGCN_EINVAL;
    if (p->n_scenes < 0 || p->n_tracks < 0 || p->n_rows < 0) return LGCN_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (!(p->pred_range[i] == p->pred_range[i])) return LGCN_EINVAL;
    if (p->n_scenes == 0) return (p->n_tracks | p->n_rows) ? LGCN_EINVAL : LGCN_OK;
    if (p->n_tracks > 0x7fffffff / 64 || p->n_scenes > 0x7fffffff / 16) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(p->off_host);
    const int32_t *trk_off = p->off_host, *row_off = p->off_host + (p->n_scenes + 1);
    if (int rc = check_table(trk_off, p->n_scenes, p->n_tracks)) return rc;
    if (int rc = check_table(row_off, p->n_tracks, p->n_rows)) return rc;
    for (int s = 0; s < p->n_scenes; ++s)
        if (trk_off[s + 1] == trk_off[s]) return LGCN_EINVAL;          // every scene holds its agent
    LGCN_CHECK_PTR(p->off_dev); LGCN_CHECK_PTR(p->frame); LGCN_CHECK_PTR(p->ws); LGCN_CHECK_PTR(p->head);
    LGCN_CHECK_PTR(p->feats); LGCN_CHECK_PTR(p->obs); LGCN_CHECK_PTR(p->ctrs); LGCN_CHECK_PTR(p->gt); LGCN_CHECK_PTR(p->has);
    if (p->n_rows > 0) { LGCN_CHECK_PTR(p->xy); LGCN_CHECK_PTR(p->step); }
    LGCN_CHECK_ALIGN16(p->xy); LGCN_CHECK_ALIGN16(p->ws);
    const void *words[] = {p->off_dev, p->step, p->frame, p->head, p->feats, p->obs, p->ctrs, p->gt};
    for (const void *q : words)
        if (misaligned(q, 3u)) return LGCN_EALIGN;
    return LGCN_OK;
}

static int sc_table_validate(const lgcn_lane_table_t *tb) {
    if (tb->n_lanes < 0 || tb->n_pts < 0 || tb->n_pred < 0 || tb->n_succ < 0) return LGCN_EINVAL;
    if (lgcn_scene_topo_elems(tb->n_lanes, tb->n_pred, tb->n_succ) < 0) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(tb->topo_host); LGCN_CHECK_PTR(tb->topo_dev);
    if (tb->n_pts > 0) LGCN_CHECK_PTR(tb->pts);
    LGCN_CHECK_ALIGN16(tb->pts);
    if (misaligned(tb->topo_dev, 3u) || misaligned(tb->topo_host, 3u)) return LGCN_EALIGN;
    const int L = tb->n_lanes;
    const ScTopo tp = sc_topo(tb->topo_host, L, tb->n_pred);
    if (int rc = check_table(tp.pt_off, L, tb->n_pts)) return rc;
    if (int rc = check_table(tp.pred_off, L, tb->n_pred)) return rc;
    if (int rc = check_table(tp.succ_off, L, tb->n_succ)) return rc;
    for (int l = 0; l < L; ++l) {
        if (tp.pt_off[l + 1] - tp.pt_off[l] < 2) return LGCN_EINVAL;
        if (tp.left[l] < -1 || tp.left[l] >= L || tp.right[l] < -1 || tp.right[l] >= L) return LGCN_EINVAL;
    }
    for (int e = 0; e < tb->n_pred; ++e)
        if (tp.pred[e] < -1 || tp.pred[e] >= L) return LGCN_EINVAL;
    for (int e = 0; e < tb->n_succ; ++e)
        if (tp.succ[e] < -1 || tp.succ[e] >= L) return LGCN_EINVAL;
    return LGCN_OK;
}

// stage 1: what lgcn_scene_lanes_rank reads; stage 2 adds the outputs of lgcn_scene_lanes_fill
static int sc_lanes_validate(const lgcn_scene_lanes_t *p, int stage) {
    if (p == nullptr) return LGCN_EINVAL;
    if (p->n_scenes < 0 || p->n_tables < 0 || p->n_cand < 0 || p->n_rank < 0) return LGCN_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (!(p->pred_range[i] == p->pred_range[i])) return LGCN_EINVAL;
    if (p->n_scenes == 0) return (p->n_cand | p->n_rank) ? LGCN_EINVAL : LGCN_OK;
    if (p->n_tables == 0) return LGCN_EINVAL;
    if (p->n_scenes > 0x7fffffff / 16) return LGCN_ESHAPE;
    const int64_t n_ws = lgcn_scene_lanes_ws_elems(p->n_cand, p->n_rank);
    if (n_ws < 0) return (int)n_ws;
    LGCN_CHECK_PTR(p->tabs_host); LGCN_CHECK_PTR(p->tabs_dev); LGCN_CHECK_PTR(p->off_host); LGCN_CHECK_PTR(p->off_dev);
    LGCN_CHECK_PTR(p->frame); LGCN_CHECK_PTR(p->ws); LGCN_CHECK_PTR(p->head);
    for (int i = 0; i < p->n_tables; ++i)
        if (int rc = sc_table_validate(p->tabs_host + i)) return rc;
    const int S = p->n_scenes;
    const ScTabs t = sc_tabs(p->off_host, S);
    if (int rc = check_table(t.cand_off, S, p->n_cand)) return rc;
    if (int rc = check_table(t.rank_off, S, p->n_rank)) return rc;
    int64_t most = 0;      // what the int32 scans can reach at most: every point and neighbour entry of every scene's table
    for (int s = 0; s < S; ++s) {
        if (t.scene_tab[s] < 0 || t.scene_tab[s] >= p->n_tables) return LGCN_EINVAL;
        const lgcn_lane_table_t &tb = p->tabs_host[t.scene_tab[s]];
        most += (int64_t)tb.n_pts + tb.n_pred + tb.n_succ;
        if (most > 0x7fffffff) return LGCN_ESHAPE;
        const int L = p->tabs_host[t.scene_tab[s]].n_lanes;
        if (t.rank_off[s + 1] - t.rank_off[s] != L) return LGCN_EINVAL;
        const int nc = t.cand_off[s + 1] - t.cand_off[s];
        if (nc <= 0) return LGCN_EINVAL;                               // a scene without a candidate has no graph
        if (!p->explicit_ids) {
            if (nc != L) return LGCN_EINVAL;
        } else {
            for (int c = t.cand_off[s]; c < t.cand_off[s + 1]; ++c)
                if (t.cand[c] < 0 || t.cand[c] >= L) return LGCN_EINVAL;
        }
    }
    LGCN_CHECK_ALIGN16(p->ws);
    if (misaligned(p->tabs_dev, 7u) || misaligned(p->off_dev, 3u) || misaligned(p->frame, 3u) ||
        misaligned(p->head, 3u))
        return LGCN_EALIGN;
    if (stage < 2) return LGCN_OK;
    if (p->n_nodes < 0 || p->cap_pre < 0 || p->cap_suc < 0 || p->cap_pre_pairs < 0 || p->cap_suc_pairs < 0 ||
        p->cap_left_pairs < 0 || p->cap_right_pairs < 0)
        return LGCN_EINVAL;
    LGCN_CHECK_PTR(p->head2);
    if (p->n_nodes > 0) {
        LGCN_CHECK_PTR(p->ctrs); LGCN_CHECK_PTR(p->feats); LGCN_CHECK_PTR(p->turn); LGCN_CHECK_PTR(p->control);
        LGCN_CHECK_PTR(p->intersect); LGCN_CHECK_PTR(p->lane_idcs);
    }
    if (p->cap_pre > 0) { LGCN_CHECK_PTR(p->pre_u); LGCN_CHECK_PTR(p->pre_v); }
    if (p->cap_suc > 0) { LGCN_CHECK_PTR(p->suc_u); LGCN_CHECK_PTR(p->suc_v); }
    if (p->cap_pre_pairs > 0) LGCN_CHECK_PTR(p->pre_pairs);
    if (p->cap_suc_pairs > 0) LGCN_CHECK_PTR(p->suc_pairs);
    if (p->cap_left_pairs > 0) LGCN_CHECK_PTR(p->left_pairs);
    if (p->cap_right_pairs > 0) LGCN_CHECK_PTR(p->right_pairs);
    const void *words[] = {p->head2, p->ctrs, p->feats, p->turn, p->control, p->intersect};
    for (const void *q : words)
        if (misaligned(q, 3u)) return LGCN_EALIGN;
    const void *dwords[] = {p->lane_idcs, p->pre_u, p->pre_v, p->suc_u, p->suc_v, p->pre_pairs, p->suc_pairs, p->left_pairs,
                            p->right_pairs};
    for (const void *q : dwords)
        if (misaligned(q, 7u)) return LGCN_EALIGN;
    return LGCN_OK;
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int64_t lgcn_scene_tracks_ws_elems(int64_t n_tracks) {
    if (n_tracks < 0) return LGCN_EINVAL;
    if (n_tracks > 0x7fffffff / 64) return LGCN_ESHAPE;
    return 2 * up4(n_tracks + 1) + up4(sc_blocks(n_tracks + 1));
}

int lgcn_scene_tracks(const lgcn_scene_tracks_t *p, void *stream) {
    if (int rc = sc_tracks_validate(p)) return rc;
    if (p->n_scenes == 0) return LGCN_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ScTrkWs w = sc_trk_ws(p->ws, p->n_tracks);
    const dim3 grid((unsigned)sc_blocks((int64_t)p->n_tracks + 1));
    hipLaunchKernelGGL(k_scene_track_flag, grid, dim3(kScThreads), 0, st, *p, w);
    hipLaunchKernelGGL(k_scene_track_fill, grid, dim3(kScThreads), 0, st, *p, w);
    return launch_status();
}

int64_t lgcn_scene_topo_elems(int64_t n_lanes, int64_t n_pred, int64_t n_succ) {
    if (n_lanes < 0 || n_pred < 0 || n_succ < 0) return LGCN_EINVAL;
    const int64_t lim = 0x7fffffff;
    if (n_lanes > lim / 16 || n_pred > lim / 4 || n_succ > lim / 4) return LGCN_ESHAPE;
    return 3 * (n_lanes + 1) + 3 * n_lanes + n_pred + n_succ;
}

int64_t lgcn_scene_lanes_ws_elems(int64_t n_cand, int64_t n_rank) {
    if (n_cand < 0 || n_rank < 0) return LGCN_EINVAL;
    const int64_t lim = 0x7fffffff;
    if (n_cand > lim / 32 || n_rank > lim / 8) return LGCN_ESHAPE;
    return sc_lane_ws(nullptr, n_cand, n_rank).total;
}

int lgcn_scene_lanes_rank(const lgcn_scene_lanes_t *p, void *stream) {
    if (int rc = sc_lanes_validate(p, 1)) return rc;
    if (p->n_scenes == 0) return LGCN_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ScLaneWs w = sc_lane_ws(p->ws, p->n_cand, p->n_rank);
    if (p->n_rank > 0 &&       // rank_of and node_of are adjacent: one memset to -1
        hipMemsetAsync(w.rank_of, 0xff, sizeof(int32_t) * (size_t)(2 * up4(p->n_rank)), st) != hipSuccess)
        return launch_status();
    const dim3 grid((unsigned)sc_blocks((int64_t)p->n_cand + 1));
    hipLaunchKernelGGL(k_scene_lane_flag, grid, dim3(kScThreads), 0, st, *p, w);
    hipLaunchKernelGGL(k_scene_lane_rank, grid, dim3(kScThreads), 0, st, *p, w);
    return launch_status();
}

int lgcn_scene_lanes_fill(const lgcn_scene_lanes_t *p, void *stream) {
    if (int rc = sc_lanes_validate(p, 2)) return rc;
    if (p->n_scenes == 0) return LGCN_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ScLaneWs w = sc_lane_ws(p->ws, p->n_cand, p->n_rank);
    const dim3 grid((unsigned)sc_blocks((int64_t)p->n_cand + 1));
    hipLaunchKernelGGL(k_scene_lane_count, grid, dim3(kScThreads), 0, st, *p, w);
    hipLaunchKernelGGL(k_scene_lane_fill, grid, dim3(kScThreads), 0, st, *p, w);
    return launch_status();
}

}  // extern "C"
