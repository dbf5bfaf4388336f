// Device-resident scene store (include/lgcn.h, lgcn_store_gather): one launch cuts a FlatBatch and the actor-side
// extras of any list of scenes out of the arrays of a flat store (lanegcn_amd/flatfile.py) that live in HBM.
//
// Pure data movement.  The grid is laid over OUTPUT elements, in five block ranges (one per kind of item); a thread
// finds the picked scene / index segment of its item by binary search in the per-batch table, so neither the number
// of scenes nor the number of segments is bounded by a wave or an LDS array.  Every source run is contiguous per scene
// and threads of a wave hold consecutive items: reads and writes are coalesced but for the run boundaries.
//
// lgcn_store_gather_aug is the same kernel body (k_store_gather<true>) with the reference's training rotation on the way
// through: coordinates are turned by the pick's Rm, rot comes from the per-batch table instead of the store.
//
// lgcn_store_gather_pad is its third instantiation (k_store_gather<false, true>): the table's last scene is the filler
// scene of a padded batch (negative sources), whose rows are written from constants instead of read from the store, so
// that every batch has the same sizes and the launch -- arguments and grid -- is the same for any pick.
//
// lgcn_store_pack (k_store_pack) is the write side: one launch packs index runs of int16 / int32 / int64 sources into the
// store's int32 edge arrays and cuts rot / orig out of a batch's frame rows.  Same shape of kernel: the grid lies over
// output words, a thread finds its run by binary search, the source descriptors are read from the device table.
//
// lgcn_roi_store_gather (k_roi_store_gather) is the fork's gather: the merged lane-RoI graph and the per-RoI agent rows of
// any pick out of a resident RoI store whose indices are scene-local.  Same shape of kernel, three kinds of item.
#include <cmath>

#include "lgcn_common.hpp"
#include "lgcn_blockscan.hpp"

namespace lgcn {

constexpr int kStoreThreads = 256;
constexpr int kActorRow = 60;       // floats of one actor in actor_feats [20,3] and in gt_preds [30,2]
constexpr int kHasRow = 30;         // bytes of one actor in has_preds

// the per-batch table, int64 (B picked scenes, G = 2 * n_rel * B index segments)
struct StoreTab {
    const int64_t *node_off, *actor_off;    // [B + 1] prefix sums of the OUTPUT rows
    const int64_t *node_src, *actor_src;    // [B] first row of the picked scene in the store
    const int64_t *scene;                   // [B] the picked scene (rot / orig)
    const int64_t *seg_off;                 // [G + 1] prefix sums of idx_local
    const int64_t *seg_src;                 // [G] first element of the segment in edge_u / edge_v
    int64_t total;
};

__host__ __device__ inline StoreTab store_tab(const int64_t *t, int64_t B, int64_t G) {
    StoreTab s;
    s.node_off = t;
    s.actor_off = s.node_off + B + 1;
    s.node_src = s.actor_off + B + 1;
    s.actor_src = s.node_src + B;
    s.scene = s.actor_src + B;
    s.seg_off = s.scene + B;
    s.seg_src = s.seg_off + G + 1;
    s.total = 5 * B + 2 * G + 3;
    return s;
}

// block ranges of the five kinds of item: kind k owns blocks [first[k], first[k + 1])
struct StoreGrid {
    uint32_t first[6];
};

// one picked scene's entry of the augmentation table: Rm row-major, then rot' row-major (include/lgcn.h)
struct StoreAug {
    float4 rm, rot;
};

// (x, y) Rm as the project fixes it: two fp32 products, each rounded, one fp32 add, never fused
__device__ __forceinline__ float2 store_turn(float2 p, float4 rm) {
    return make_float2(__fadd_rn(__fmul_rn(p.x, rm.x), __fmul_rn(p.y, rm.z)),
                       __fadd_rn(__fmul_rn(p.x, rm.y), __fmul_rn(p.y, rm.w)));
}

// the filler scene of a padded batch: nodes far on one side, actors far on the other and 256 m
// apart (farther than every distance threshold), all features zero
constexpr float kFillNode = 1e6f;
__device__ __forceinline__ float2 store_fill_actor(int64_t i) { return make_float2((float)(-1000000 - 256 * i), -1e6f); }

// AUG = false is lgcn_store_gather (aug is not read); AUG = true turns the picked scene j by aug[j] on the way through;
// PAD: a scene with a negative source is the filler (the last one; lgcn_store_pad_check), written without reading the store
template <bool AUG, bool PAD>
__global__ __launch_bounds__(kStoreThreads) void k_store_gather(const lgcn_store_t s, const lgcn_store_batch_t b,
                                                                const StoreGrid g, const StoreAug *__restrict__ aug) {
    const int B = b.n_scenes;
    const int64_t G = 2 * (int64_t)b.n_rel * B;
    const StoreTab t = store_tab(b.tab_dev, B, G);
    const uint32_t blk = blockIdx.x;
    int kind = 0;
    while (kind < 4 && blk >= g.first[kind + 1]) ++kind;
    const int64_t i = (int64_t)(blk - g.first[kind]) * kStoreThreads + threadIdx.x;

    if (kind == 0) {                      // one node row: ctrs, feats, turn [.,2], control, intersect
        if (i >= b.n_nodes) return;
        const int j = find_seg(t.node_off, B, i);
        const int64_t r = t.node_src[j] + (i - t.node_off[j]);
        if (PAD && t.node_src[j] < 0) {
            reinterpret_cast<float2 *>(b.node_ctrs)[i] = make_float2(kFillNode, kFillNode);
            reinterpret_cast<float2 *>(b.node_feats)[i] = make_float2(0.f, 0.f);
            reinterpret_cast<float2 *>(b.turn)[i] = make_float2(0.f, 0.f);
            b.control[i] = 0.f;
            b.intersect[i] = 0.f;
            return;
        }
        if constexpr (AUG) {
            const float4 rm = aug[j].rm;
            reinterpret_cast<float2 *>(b.node_ctrs)[i] = store_turn(reinterpret_cast<const float2 *>(s.node_ctrs)[r], rm);
            reinterpret_cast<float2 *>(b.node_feats)[i] = store_turn(reinterpret_cast<const float2 *>(s.node_feats)[r], rm);
        } else {
            reinterpret_cast<float2 *>(b.node_ctrs)[i] = reinterpret_cast<const float2 *>(s.node_ctrs)[r];
            reinterpret_cast<float2 *>(b.node_feats)[i] = reinterpret_cast<const float2 *>(s.node_feats)[r];
        }
        reinterpret_cast<float2 *>(b.turn)[i] = reinterpret_cast<const float2 *>(s.turn)[r];
        b.control[i] = s.control[r];
        b.intersect[i] = s.intersect[r];
    } else if (kind == 1) {               // one actor: ctrs, and the scene's rot / orig
        if (i >= b.n_actors) return;
        const int j = find_seg(t.actor_off, B, i);
        const int64_t r = t.actor_src[j] + (i - t.actor_off[j]);
        const int64_t sc = t.scene[j];
        if (PAD && t.actor_src[j] < 0) {
            reinterpret_cast<float2 *>(b.actor_ctrs)[i] = store_fill_actor(i - t.actor_off[j]);
            reinterpret_cast<float4 *>(b.rot)[i] = make_float4(1.f, 0.f, 0.f, 1.f);
            reinterpret_cast<float2 *>(b.orig)[i] = make_float2(0.f, 0.f);
            return;
        }
        if constexpr (AUG) {
            reinterpret_cast<float2 *>(b.actor_ctrs)[i] = store_turn(reinterpret_cast<const float2 *>(s.actor_ctrs)[r], aug[j].rm);
            reinterpret_cast<float4 *>(b.rot)[i] = aug[j].rot;
        } else {
            reinterpret_cast<float2 *>(b.actor_ctrs)[i] = reinterpret_cast<const float2 *>(s.actor_ctrs)[r];
            reinterpret_cast<float4 *>(b.rot)[i] = reinterpret_cast<const float4 *>(s.rot)[sc];
        }
        reinterpret_cast<float2 *>(b.orig)[i] = reinterpret_cast<const float2 *>(s.orig)[sc];
    } else if (kind == 2) {               // one of an actor's 60 floats: actor_feats [20,3] -> [3,20], gt_preds, has_preds
        if (i >= b.n_actors * kActorRow) return;
        const int64_t a = i / kActorRow;
        const int e = (int)(i - a * kActorRow);
        const int j = find_seg(t.actor_off, B, a);
        const int64_t r = t.actor_src[j] + (a - t.actor_off[j]);
        const int c = e / 20, step = e - c * 20;
        if (PAD && t.actor_src[j] < 0) {
            b.actor_feats[i] = 0.f;
            if (s.gt_preds != nullptr) {
                b.gt_preds[i] = 0.f;
                if (e < kHasRow) b.has_preds[a * kHasRow + e] = 0;
            }
            return;
        }
        if (AUG && c < 2) {                // channels 0 / 1 are the step's (x, y): both are read, one component is written
            const float *xy = s.actor_feats + r * kActorRow + step * 3;
            const float2 q = store_turn(make_float2(xy[0], xy[1]), aug[j].rm);
            b.actor_feats[i] = c == 0 ? q.x : q.y;
        } else {
            b.actor_feats[i] = s.actor_feats[r * kActorRow + step * 3 + c];
        }
        if (s.gt_preds != nullptr) {
            b.gt_preds[i] = s.gt_preds[r * kActorRow + e];
            if (e < kHasRow) b.has_preds[a * kHasRow + e] = s.has_preds[r * kHasRow + e];
        }
    } else if (kind == 3) {               // one element of idx_local, widened
        if (i >= b.n_elem) return;
        const int64_t k = find_seg(t.seg_off, (int)G, i);
        const int64_t r = t.seg_src[k] + (i - t.seg_off[k]);
        if (PAD && t.seg_src[k] < 0) {      // filler edge e: the self-loop of its node e mod n_f (both the u and the v segment)
            b.idx_local[i] = (i - t.seg_off[k]) % (t.node_off[B] - t.node_off[B - 1]);
            return;
        }
        const int32_t *src = ((k / B) & 1) ? s.edge_v : s.edge_u;     // segment k = (relation * 2 + u|v) * B + scene
        b.idx_local[i] = (int64_t)src[r];
    } else {                              // the offset arrays: node_off, actor_off, seg_off, seg_base
        int64_t q = i;
        if (q <= B) { b.node_off[q] = (int32_t)t.node_off[q]; return; }
        q -= B + 1;
        if (q <= B) { b.actor_off[q] = (int32_t)t.actor_off[q]; return; }
        q -= B + 1;
        if (q <= G) { b.seg_off[q] = t.seg_off[q]; return; }
        q -= G + 1;
        if (q < G) b.seg_base[q] = t.node_off[q % B];
    }
}

// ------------------------------------------------------------------ lgcn_store_pack
// the table of one pack, int64 (G runs, K sources)
struct PackTab {
    const int64_t *seg_off;     // [G + 1] prefix sums of the destination words
    const int64_t *seg_src;     // [G] the run's source
    const int64_t *seg_at;      // [G] first element of the run in its source
    const int64_t *src_ptr;     // [K] device address of the source
    const int64_t *src_kind;    // [K] bytes per element: 2, 4 or 8
    const int64_t *src_len;     // [K] elements of the source
};

__host__ __device__ inline PackTab pack_tab(const int64_t *t, int64_t G, int64_t K) {
    PackTab s;
    s.seg_off = t;
    s.seg_src = s.seg_off + G + 1;
    s.seg_at = s.seg_src + G;
    s.src_ptr = s.seg_at + G;
    s.src_kind = s.src_ptr + K;
    s.src_len = s.src_kind + K;           // 3 G + 1 + 3 K words in all (lgcn_store_pack_table_elems)
    return s;
}

// blocks [0, frame_first) own the destination words, the rest one scene's frame row each thread
__global__ __launch_bounds__(kStoreThreads) void k_store_pack(const lgcn_store_pack_t p, const uint32_t frame_first) {
    const uint32_t blk = blockIdx.x;
    if (blk < frame_first) {              // one destination word: the run's element, narrowed or sign-extended to int32
        const int64_t i = (int64_t)blk * kStoreThreads + threadIdx.x;
        if (i >= p.n_dst) return;
        const PackTab t = pack_tab(p.tab_dev, p.n_seg, p.n_src);
        const int k = find_seg(t.seg_off, (int)p.n_seg, i);
        const int64_t s = t.seg_src[k];
        const int64_t r = t.seg_at[k] + (i - t.seg_off[k]);
        const int64_t kind = t.src_kind[s];
        const uintptr_t base = (uintptr_t)t.src_ptr[s];
        int32_t v;
        if (kind == 8) v = (int32_t)reinterpret_cast<const int64_t *>(base)[r];          // the low 32 bits
        else if (kind == 4) v = reinterpret_cast<const int32_t *>(base)[r];
        else v = (int32_t)reinterpret_cast<const int16_t *>(base)[r];
        p.dst[i] = v;
    } else {                              // one scene: frame row (orig, rot row-major) -> orig [2], rot [2,2]
        const int64_t j = (int64_t)(blk - frame_first) * kStoreThreads + threadIdx.x;
        if (j >= p.n_scenes) return;
        const float2 *f = reinterpret_cast<const float2 *>(p.frame) + 3 * j;
        const float2 o = f[0], r0 = f[1], r1 = f[2];
        reinterpret_cast<float2 *>(p.orig)[j] = o;
        reinterpret_cast<float4 *>(p.rot)[j] = make_float4(r0.x, r0.y, r1.x, r1.y);
    }
}

// ------------------------------------------------------------------ host side
// prefix sums off[0..n] from 0 to total; src[i] + (off[i + 1] - off[i]) inside [0, limit].  pad_every > 0: every
// pad_every-th run is the filler's (a padded batch): a negative source and at least pad_min elements, else the pick does
// not fit the capacities; no other run may have a negative source
static int store_check_runs(const int64_t *off, const int64_t *src, int64_t n, int64_t total, int64_t limit,
                            int64_t pad_every = 0, int64_t pad_min = 0) {
    if (off[0] != 0) return LGCN_EINVAL;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = off[i + 1] - off[i];
        if (pad_every > 0 && i % pad_every == pad_every - 1) {
            if (src[i] >= 0) return LGCN_EINVAL;
            if (len < pad_min) return LGCN_ESHAPE;
            continue;
        }
        if (len < 0) return LGCN_EINVAL;
        if (src[i] < 0 || src[i] > limit || len > limit - src[i]) return LGCN_EINVAL;
    }
    return off[n] == total ? LGCN_OK : LGCN_EINVAL;
}

static inline int64_t store_blocks(int64_t n) { return (n + kStoreThreads - 1) / kStoreThreads; }

// tab: the host table to check (nullptr: none is read, lgcn_store_gather_pad); pad: the batch is a padded one, its last
// scene the filler
static int store_validate(const lgcn_store_t *s, const lgcn_store_batch_t *b, StoreGrid *grid, const int64_t *tab, bool pad,
                          bool need_tab = true) {
    if (s == nullptr || b == nullptr) return LGCN_EINVAL;
    if (s->n_scenes < 0 || s->n_nodes < 0 || s->n_actors < 0 || s->n_edges < 0) return LGCN_EINVAL;
    if (b->n_scenes < 0 || b->n_rel < 0 || b->n_nodes < 0 || b->n_actors < 0 || b->n_elem < 0) return LGCN_EINVAL;
    if (pad && (b->n_scenes < 2 || b->n_nodes == 0 || b->n_actors == 0)) return LGCN_EINVAL;
    if (b->n_scenes == 0) return (b->n_nodes | b->n_actors | b->n_elem) ? LGCN_EINVAL : LGCN_OK;
    const int64_t lim = 0x7fffffff;
    if (b->n_nodes > lim || b->n_actors > lim / kActorRow || b->n_elem > lim) return LGCN_ESHAPE;
    const int64_t B = b->n_scenes, G = 2 * (int64_t)b->n_rel * B;
    if (G > lim || lgcn_store_table_elems(B, b->n_rel) < 0) return LGCN_ESHAPE;
    if ((s->gt_preds == nullptr) != (s->has_preds == nullptr)) return LGCN_EINVAL;
    if (s->n_nodes > 0) {
        LGCN_CHECK_PTR(s->node_ctrs); LGCN_CHECK_PTR(s->node_feats); LGCN_CHECK_PTR(s->turn); LGCN_CHECK_PTR(s->control);
        LGCN_CHECK_PTR(s->intersect);
    }
    if (s->n_actors > 0) { LGCN_CHECK_PTR(s->actor_ctrs); LGCN_CHECK_PTR(s->actor_feats); }
    if (s->n_scenes > 0) { LGCN_CHECK_PTR(s->rot); LGCN_CHECK_PTR(s->orig); }
    if (s->n_edges > 0) { LGCN_CHECK_PTR(s->edge_u); LGCN_CHECK_PTR(s->edge_v); }
    if (need_tab) LGCN_CHECK_PTR(tab);
    LGCN_CHECK_PTR(b->tab_dev);
    LGCN_CHECK_PTR(b->node_off); LGCN_CHECK_PTR(b->actor_off); LGCN_CHECK_PTR(b->seg_off);
    if (G > 0) LGCN_CHECK_PTR(b->seg_base);
    if (b->n_nodes > 0) {
        LGCN_CHECK_PTR(b->node_ctrs); LGCN_CHECK_PTR(b->node_feats); LGCN_CHECK_PTR(b->turn); LGCN_CHECK_PTR(b->control);
        LGCN_CHECK_PTR(b->intersect);
    }
    if (b->n_actors > 0) {
        LGCN_CHECK_PTR(b->actor_ctrs); LGCN_CHECK_PTR(b->actor_feats); LGCN_CHECK_PTR(b->rot); LGCN_CHECK_PTR(b->orig);
        if (s->gt_preds != nullptr) { LGCN_CHECK_PTR(b->gt_preds); LGCN_CHECK_PTR(b->has_preds); }
    }
    if (b->n_elem > 0) LGCN_CHECK_PTR(b->idx_local);

    // the table, read on the host: nothing in it becomes an address before it is known to lie inside the store
    if (tab != nullptr) {
        const StoreTab t = store_tab(tab, B, G);
        const int64_t every = pad ? B : 0;
        if (int rc = store_check_runs(t.node_off, t.node_src, B, b->n_nodes, s->n_nodes, every, 1)) return rc;
        if (int rc = store_check_runs(t.actor_off, t.actor_src, B, b->n_actors, s->n_actors, every, 1)) return rc;
        if (int rc = store_check_runs(t.seg_off, t.seg_src, G, b->n_elem, s->n_edges, every, 0)) return rc;
        for (int64_t j = 0; j < B - (pad ? 1 : 0); ++j)
            if (t.scene[j] < 0 || t.scene[j] >= s->n_scenes) return LGCN_EINVAL;
        if (pad && t.scene[B - 1] >= 0) return LGCN_EINVAL;
    }

    const void *quads[] = {s->node_ctrs, s->node_feats, s->turn, s->actor_ctrs, s->rot, s->orig, b->tab_dev, b->node_ctrs,
                           b->node_feats, b->turn, b->actor_ctrs, b->rot, b->orig, b->idx_local, b->seg_off, b->seg_base};
    for (const void *q : quads) LGCN_CHECK_ALIGN16(q);
    const void *words[] = {s->control, s->intersect, s->actor_feats, s->gt_preds, s->edge_u, s->edge_v, b->control,
                           b->intersect, b->node_off, b->actor_off, b->actor_feats, b->gt_preds};
    for (const void *q : words)
        if (misaligned(q, 3u)) return LGCN_EALIGN;
    if (misaligned(tab, 7u)) return LGCN_EALIGN;

    const int64_t items[5] = {b->n_nodes, b->n_actors, b->n_actors * kActorRow, b->n_elem, 2 * (B + 1) + 2 * G + 1};
    int64_t at = 0;
    for (int k = 0; k < 5; ++k) {
        grid->first[k] = (uint32_t)at;
        at += store_blocks(items[k]);
    }
    if (at > lim) return LGCN_ESHAPE;
    grid->first[5] = (uint32_t)at;
    return LGCN_OK;
}

// everything lgcn_store_pack reads from the host table becomes an address only after it is known to lie inside a source
static int pack_validate(const lgcn_store_pack_t *p, uint32_t *frame_first, uint32_t *n_blocks) {
    if (p == nullptr) return LGCN_EINVAL;
    if (p->n_seg < 0 || p->n_src < 0 || p->n_dst < 0 || p->n_scenes < 0) return LGCN_EINVAL;
    if (p->n_seg == 0) return (p->n_dst | p->n_scenes) ? LGCN_EINVAL : LGCN_OK;
    const int64_t lim = 0x7fffffff;
    if (p->n_dst > lim || p->n_scenes > lim || lgcn_store_pack_table_elems(p->n_seg, p->n_src) < 0) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(p->tab_host); LGCN_CHECK_PTR(p->tab_dev);
    if (p->n_dst > 0) LGCN_CHECK_PTR(p->dst);
    if (p->n_scenes > 0) { LGCN_CHECK_PTR(p->frame); LGCN_CHECK_PTR(p->rot); LGCN_CHECK_PTR(p->orig); }
    if (misaligned(p->tab_host, 7u)) return LGCN_EALIGN;
    LGCN_CHECK_ALIGN16(p->tab_dev);
    LGCN_CHECK_ALIGN16(p->rot);
    if (misaligned(p->frame, 7u) || misaligned(p->orig, 7u)) return LGCN_EALIGN;
    if (misaligned(p->dst, 3u)) return LGCN_EALIGN;

    const PackTab t = pack_tab(p->tab_host, p->n_seg, p->n_src);
    for (int64_t s = 0; s < p->n_src; ++s) {
        const int64_t kind = t.src_kind[s], len = t.src_len[s];
        if ((kind != 2 && kind != 4 && kind != 8) || len < 0) return LGCN_EINVAL;
        if (len > lim) return LGCN_ESHAPE;
        if (len > 0 && t.src_ptr[s] == 0) return LGCN_EINVAL;
        if ((uint64_t)t.src_ptr[s] & (uint64_t)(kind - 1)) return LGCN_EALIGN;
    }
    if (t.seg_off[0] != 0) return LGCN_EINVAL;
    for (int64_t k = 0; k < p->n_seg; ++k) {
        if (t.seg_off[k + 1] < t.seg_off[k]) return LGCN_EINVAL;      // (so every entry is >= 0 and the difference holds)
        const int64_t len = t.seg_off[k + 1] - t.seg_off[k], s = t.seg_src[k], at = t.seg_at[k];
        if (s < 0 || s >= p->n_src) return LGCN_EINVAL;
        if (at < 0 || at > t.src_len[s] || len > t.src_len[s] - at) return LGCN_EINVAL;
    }
    if (t.seg_off[p->n_seg] != p->n_dst) return LGCN_EINVAL;
    *frame_first = (uint32_t)store_blocks(p->n_dst);
    *n_blocks = *frame_first + (uint32_t)store_blocks(p->n_scenes);
    return LGCN_OK;
}

// ------------------------------------------------------------------ lgcn_roi_store_gather
// The fork's counterpart: the lane RoIs of a split stay resident with SCENE-LOCAL int32 indices (row within the block of
// the scene's RoI nodes; for a2m_u the RoI's number within the scene), and one launch cuts the merged graph of any pick
// out of them: copy the run, add the base of the picked scene.
constexpr int kRoiRel = 14;                       // induced relations of an RoI (pre 0..5, suc 0..5, left, right)
constexpr int kRoiSegs = 2 * kRoiRel + 2;         // index runs per picked scene: u and v of each relation, a2m_u, a2m_v
constexpr int kRoiAgentQuads = 20;                // float4 of one agent_feat row [80]
constexpr int kRoiTrackQuads = 15;                // float4 of one actor_feats / obs [20,3] or gt_preds [30,2] row
constexpr int kRoiHasPairs = kHasRow / 2;         // 2-byte pieces of one has_preds row (rows start on even bytes only)
constexpr int kRoiSlots = kRoiAgentQuads + 2 * kRoiTrackQuads + 1;          // + ctrs: items of one RoI row without gt
constexpr int kRoiSlotsGt = kRoiSlots + kRoiTrackQuads + kRoiHasPairs;      // + gt_preds, has_preds

// the per-batch table, int64 (B picked scenes, G = 30 B segments ordered (run, scene): u of relation 0..13, v of
// relation 0..13, a2m_u, a2m_v)
struct RoiStoreTab {
    const int64_t *node_off, *roi_off;      // [B + 1] prefix sums of the OUTPUT node rows / RoI rows
    const int64_t *node_src, *roi_src;      // [B] first node row / first RoI of the picked scene in the store
    const int64_t *seg_off;                 // [G + 1] prefix sums of idx
    const int64_t *seg_src;                 // [G] first element of the segment in its resident array
    int64_t total;
};

__host__ __device__ inline RoiStoreTab roi_store_tab(const int64_t *t, int64_t B) {
    const int64_t G = kRoiSegs * B;
    RoiStoreTab s;
    s.node_off = t;
    s.roi_off = s.node_off + B + 1;
    s.node_src = s.roi_off + B + 1;
    s.roi_src = s.node_src + B;
    s.seg_off = s.roi_src + B;
    s.seg_src = s.seg_off + G + 1;
    s.total = 4 * B + 2 * G + 3;
    return s;
}

// block ranges of the three kinds of item: node half-rows, RoI row pieces, index elements
struct RoiStoreGrid {
    uint32_t first[4];
};

__global__ __launch_bounds__(kStoreThreads) void k_roi_store_gather(const lgcn_roi_store_t s, const lgcn_roi_store_batch_t b,
                                                                    const RoiStoreGrid g) {
    const int B = (int)b.n_scenes;
    const RoiStoreTab t = roi_store_tab(b.tab_dev, B);
    const uint32_t blk = blockIdx.x;
    int kind = 0;
    while (kind < 2 && blk >= g.first[kind + 1]) ++kind;
    const int64_t i = (int64_t)(blk - g.first[kind]) * kStoreThreads + threadIdx.x;

    if (kind == 0) {                      // half a node row: 16 of the 32 bytes of feats; the first half widens node_mask
        if (i >= 2 * b.n_nodes) return;
        const int64_t row = i >> 1;
        const int j = find_seg(t.node_off, B, row);
        const int64_t r = t.node_src[j] + (row - t.node_off[j]);
        reinterpret_cast<float4 *>(b.feats)[i] = reinterpret_cast<const float4 *>(s.feats)[2 * r + (i & 1)];
        if ((i & 1) == 0) b.node_mask[row] = (int64_t)s.node_mask[r];
    } else if (kind == 1) {               // one piece of an RoI row: a float4, the float2 of ctrs, two bytes of has_preds
        const int slots = s.gt_preds != nullptr ? kRoiSlotsGt : kRoiSlots;
        if (i >= b.n_rois * slots) return;
        const int64_t a = i / slots;
        int e = (int)(i - a * slots);
        const int j = find_seg(t.roi_off, B, a);
        const int64_t r = t.roi_src[j] + (a - t.roi_off[j]);
        if (e < kRoiAgentQuads) {
            reinterpret_cast<float4 *>(b.agent_feat)[a * kRoiAgentQuads + e] =
                reinterpret_cast<const float4 *>(s.agent_feat)[r * kRoiAgentQuads + e];
            return;
        }
        e -= kRoiAgentQuads;
        if (e < kRoiTrackQuads) {
            reinterpret_cast<float4 *>(b.actor_feats)[a * kRoiTrackQuads + e] =
                reinterpret_cast<const float4 *>(s.actor_feats)[r * kRoiTrackQuads + e];
            return;
        }
        e -= kRoiTrackQuads;
        if (e < kRoiTrackQuads) {
            reinterpret_cast<float4 *>(b.obs)[a * kRoiTrackQuads + e] = reinterpret_cast<const float4 *>(s.obs)[r * kRoiTrackQuads + e];
            return;
        }
        e -= kRoiTrackQuads;
        if (e == 0) {
            reinterpret_cast<float2 *>(b.ctrs)[a] = reinterpret_cast<const float2 *>(s.ctrs)[r];
            return;
        }
        e -= 1;
        if (e < kRoiTrackQuads) {
            reinterpret_cast<float4 *>(b.gt_preds)[a * kRoiTrackQuads + e] =
                reinterpret_cast<const float4 *>(s.gt_preds)[r * kRoiTrackQuads + e];
            return;
        }
        e -= kRoiTrackQuads;
        reinterpret_cast<uint16_t *>(b.has_preds)[a * kRoiHasPairs + e] =
            reinterpret_cast<const uint16_t *>(s.has_preds)[r * kRoiHasPairs + e];
    } else {                              // one index element: resident int32 + the base of the picked scene
        if (i >= b.n_elem) return;
        const int64_t G = (int64_t)kRoiSegs * B;
        const int64_t k = find_seg(t.seg_off, (int)G, i);
        const int64_t r = t.seg_src[k] + (i - t.seg_off[k]);
        const int run = (int)(k / B);                         // segment k = run * B + scene
        const int j = (int)(k - (int64_t)run * B);
        const int32_t *src = run < kRoiRel ? s.edge_u : run < 2 * kRoiRel ? s.edge_v : run == 2 * kRoiRel ? s.a2m_u : s.a2m_v;
        const int64_t base = run == 2 * kRoiRel ? t.roi_off[j] : t.node_off[j];
        b.idx[i] = (int64_t)src[r] + base;
    }
}

static int roi_store_validate(const lgcn_roi_store_t *s, const lgcn_roi_store_batch_t *b, RoiStoreGrid *grid) {
    if (s == nullptr || b == nullptr) return LGCN_EINVAL;
    if (s->n_scenes < 0 || s->n_nodes < 0 || s->n_rois < 0 || s->n_edges < 0 || s->n_a2m < 0) return LGCN_EINVAL;
    if (b->n_scenes < 0 || b->n_nodes < 0 || b->n_rois < 0 || b->n_elem < 0) return LGCN_EINVAL;
    if (b->n_scenes == 0) return (b->n_nodes | b->n_rois | b->n_elem) ? LGCN_EINVAL : LGCN_OK;
    const int64_t lim = 0x7fffffff;
    if (b->n_nodes > lim / 2 || b->n_rois > lim / kRoiSlotsGt || b->n_elem > lim) return LGCN_ESHAPE;
    if (lgcn_roi_store_table_elems(b->n_scenes) < 0) return LGCN_ESHAPE;       // (so G and the table fit 32 bits)
    const int64_t B = b->n_scenes, G = kRoiSegs * B;
    if ((s->gt_preds == nullptr) != (s->has_preds == nullptr)) return LGCN_EINVAL;
    if (s->n_nodes > 0) { LGCN_CHECK_PTR(s->feats); LGCN_CHECK_PTR(s->node_mask); }
    if (s->n_rois > 0) { LGCN_CHECK_PTR(s->agent_feat); LGCN_CHECK_PTR(s->ctrs); LGCN_CHECK_PTR(s->actor_feats); LGCN_CHECK_PTR(s->obs); }
    if (s->n_edges > 0) { LGCN_CHECK_PTR(s->edge_u); LGCN_CHECK_PTR(s->edge_v); }
    if (s->n_a2m > 0) { LGCN_CHECK_PTR(s->a2m_u); LGCN_CHECK_PTR(s->a2m_v); }
    LGCN_CHECK_PTR(b->tab_host); LGCN_CHECK_PTR(b->tab_dev);
    if (b->n_nodes > 0) { LGCN_CHECK_PTR(b->feats); LGCN_CHECK_PTR(b->node_mask); }
    if (b->n_rois > 0) {
        LGCN_CHECK_PTR(b->agent_feat); LGCN_CHECK_PTR(b->ctrs); LGCN_CHECK_PTR(b->actor_feats); LGCN_CHECK_PTR(b->obs);
        if (s->gt_preds != nullptr) { LGCN_CHECK_PTR(b->gt_preds); LGCN_CHECK_PTR(b->has_preds); }
    }
    if (b->n_elem > 0) LGCN_CHECK_PTR(b->idx);
    if (misaligned(b->tab_host, 7u)) return LGCN_EALIGN;

    // the table, read on the host: nothing in it becomes an address before it is known to lie inside the store
    const RoiStoreTab t = roi_store_tab(b->tab_host, B);
    if (int rc = store_check_runs(t.node_off, t.node_src, B, b->n_nodes, s->n_nodes)) return rc;
    if (int rc = store_check_runs(t.roi_off, t.roi_src, B, b->n_rois, s->n_rois)) return rc;
    if (t.seg_off[0] != 0) return LGCN_EINVAL;
    for (int64_t k = 0; k < G; ++k) {
        const int64_t len = t.seg_off[k + 1] - t.seg_off[k], at = t.seg_src[k];
        const int64_t limit = k < 2 * kRoiRel * B ? s->n_edges : s->n_a2m;
        if (len < 0 || at < 0 || at > limit || len > limit - at) return LGCN_EINVAL;
    }
    if (t.seg_off[G] != b->n_elem) return LGCN_EINVAL;

    const void *quads[] = {s->feats, s->agent_feat, s->actor_feats, s->obs, s->gt_preds, b->tab_dev, b->feats, b->agent_feat,
                           b->actor_feats, b->obs, b->gt_preds};
    for (const void *q : quads) LGCN_CHECK_ALIGN16(q);
    if (misaligned(s->ctrs, 7u) || misaligned(b->ctrs, 7u) || misaligned(b->node_mask, 7u) || misaligned(b->idx, 7u)) return LGCN_EALIGN;
    const void *words[] = {s->node_mask, s->edge_u, s->edge_v, s->a2m_u, s->a2m_v};
    for (const void *q : words)
        if (misaligned(q, 3u)) return LGCN_EALIGN;
    if (misaligned(s->has_preds, 1u) || misaligned(b->has_preds, 1u)) return LGCN_EALIGN;

    const int64_t items[3] = {2 * b->n_nodes, b->n_rois * (s->gt_preds != nullptr ? kRoiSlotsGt : kRoiSlots), b->n_elem};
    int64_t at = 0;
    for (int k = 0; k < 3; ++k) {
        grid->first[k] = (uint32_t)at;
        at += store_blocks(items[k]);
    }
    if (at > lim) return LGCN_ESHAPE;
    grid->first[3] = (uint32_t)at;
    return LGCN_OK;
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int64_t lgcn_store_table_elems(int64_t n_scenes, int64_t n_rel) {
    if (n_scenes < 0 || n_rel < 0) return LGCN_EINVAL;
    const int64_t lim = 0x7fffffff;
    if (n_scenes > lim / 8 || n_rel > lim / 8) return LGCN_ESHAPE;
    const int64_t total = store_tab(nullptr, n_scenes, 2 * n_rel * n_scenes).total;
    return total > lim ? (int64_t)LGCN_ESHAPE : total;
}

int lgcn_store_gather(const lgcn_store_t *s, const lgcn_store_batch_t *b, void *stream) {
    StoreGrid grid;
    if (int rc = store_validate(s, b, &grid, b == nullptr ? nullptr : b->tab_host, false)) return rc;
    if (b->n_scenes == 0) return LGCN_OK;
    hipLaunchKernelGGL((k_store_gather<false, false>), dim3(grid.first[5]), dim3(kStoreThreads), 0, static_cast<hipStream_t>(stream),
                       *s, *b, grid, static_cast<const StoreAug *>(nullptr));
    return launch_status();
}

int lgcn_store_gather_aug(const lgcn_store_t *s, const lgcn_store_batch_t *b, const float *aug_host, const float *aug_dev,
                          void *stream) {
    StoreGrid grid;
    if (int rc = store_validate(s, b, &grid, b == nullptr ? nullptr : b->tab_host, false)) return rc;
    if (b->n_scenes == 0) return LGCN_OK;
    LGCN_CHECK_PTR(aug_host); LGCN_CHECK_PTR(aug_dev);
    for (int64_t k = 0; k < 8 * (int64_t)b->n_scenes; ++k)
        if (!std::isfinite(aug_host[k])) return LGCN_EINVAL;
    LGCN_CHECK_ALIGN16(aug_dev);
    hipLaunchKernelGGL((k_store_gather<true, false>), dim3(grid.first[5]), dim3(kStoreThreads), 0, static_cast<hipStream_t>(stream),
                       *s, *b, grid, reinterpret_cast<const StoreAug *>(aug_dev));
    return launch_status();
}

int lgcn_store_pad_check(const lgcn_store_t *s, const lgcn_store_batch_t *b, const int64_t *tab_host) {
    StoreGrid grid;
    return store_validate(s, b, &grid, tab_host, true);
}

int lgcn_store_gather_pad(const lgcn_store_t *s, const lgcn_store_batch_t *b, void *stream) {
    StoreGrid grid;
    if (int rc = store_validate(s, b, &grid, nullptr, true, false)) return rc;
    hipLaunchKernelGGL((k_store_gather<false, true>), dim3(grid.first[5]), dim3(kStoreThreads), 0, static_cast<hipStream_t>(stream),
                       *s, *b, grid, static_cast<const StoreAug *>(nullptr));
    return launch_status();
}

int64_t lgcn_store_pack_table_elems(int64_t n_seg, int64_t n_src) {
    if (n_seg < 0 || n_src < 0) return LGCN_EINVAL;
    const int64_t lim = 0x7fffffff;
    if (n_seg > lim / 8 || n_src > lim / 8) return LGCN_ESHAPE;
    return 3 * n_seg + 1 + 3 * n_src;            // the words that pack_tab lays out
}

int lgcn_store_pack(const lgcn_store_pack_t *p, void *stream) {
    uint32_t frame_first = 0, n_blocks = 0;
    if (int rc = pack_validate(p, &frame_first, &n_blocks)) return rc;
    if (n_blocks == 0) return LGCN_OK;
    hipLaunchKernelGGL(k_store_pack, dim3(n_blocks), dim3(kStoreThreads), 0, static_cast<hipStream_t>(stream), *p, frame_first);
    return launch_status();
}

int64_t lgcn_roi_store_table_elems(int64_t n_scenes) {
    if (n_scenes < 0) return LGCN_EINVAL;
    const int64_t lim = 0x7fffffff;
    if (n_scenes > lim / 64) return LGCN_ESHAPE;
    const int64_t total = roi_store_tab(nullptr, n_scenes).total;
    return total > lim ? (int64_t)LGCN_ESHAPE : total;
}

int lgcn_roi_store_gather(const lgcn_roi_store_t *s, const lgcn_roi_store_batch_t *b, void *stream) {
    RoiStoreGrid grid;
    if (int rc = roi_store_validate(s, b, &grid)) return rc;
    if (b->n_scenes == 0 || grid.first[3] == 0) return LGCN_OK;
    hipLaunchKernelGGL(k_roi_store_gather, dim3(grid.first[3]), dim3(kStoreThreads), 0, static_cast<hipStream_t>(stream), *s, *b, grid);
    return launch_status();
}

}  // extern "C"
