// Forecasting metrics of a whole split on the device (the reference's test.py loop and Argoverse's
// get_displacement_errors_and_miss_rate): lgcn_eval_scenes writes one 32-float record per scene, one launch per batch;
// lgcn_eval_reduce sums the records of the split, one launch per summary.  lgcn_eval_actors writes the same record for every
// actor row of a batch, partial futures included (PredLoss's rule, reference lanegcn.py:740-807: the final displacement at
// the last observed step, the mean over the observed steps), into a table with one row per actor of the split;
// lgcn_eval_reduce_sel is the reduce over the records a selection keeps.  One copy of the row arithmetic (eval_row) and one
// of the reduce (k_eval_reduce<kSel>) serve both.
//
// Why records and not running sums: a running sum needs a float atomic per scene (its value then depends on the order
// the scenes arrive in) or a second launch per batch.  A record per scene costs 128 bytes, is written by exactly one wave,
// depends on nothing but that scene's rows, and the one reduce over the records runs in a fixed order: the summary of a
// split is the same bits for any batch size, batch order or number of ranks.
//
// Record of scene b (first actor row a = actor_off[b] only, as test.py:86 and PostProcess read it), at rec[slot[b]]:
//   [0] flag   0 not evaluated (no actor, or has[a, :horizon] not all set), 1 evaluated, 2 a non-finite value in
//              reg[a, :, :horizon], cls[a] or gt[a, :horizon]
//   [1] M  [2] horizon  [3] 0                                      (flag 1 only; a record of flag 0 / 2 is zero behind [0])
//   [4 + 3 (k - 1) ...] minFDE_k, minADE_k, p_k for k = 1..M over the first k modes as they come:
//       j* = the first j < k with the smallest |reg[a, j, horizon - 1] - gt[a, horizon - 1]|  (strict <)
//       minADE_k = mean_t<horizon |reg[a, j*, t] - gt[a, t]|,  p_k = softmax(cls[a, :k])[j*]  (maximum subtracted)
// Record of an actor row (lgcn_eval_actors), with O = {t < horizon : has[a, t]}, n_obs = |O|, t_last = max O: flag 0 when O is
// empty, 2 on a non-finite value in reg[a, :, :horizon], cls[a] or gt[a, t in O]; horizon - 1 -> t_last, mean over O;
//   [3] the row's index inside its scene (every flag)   [28] horizon - n_obs   [29] horizon - 1 - t_last   (flag 1)
// A fully observed first actor's record is the scene record in all 32 floats.
// Arithmetic: fp32, no FMA (-ffp-contract=off); d_t = sqrtf(dx dx + dy dy), one step per lane; the sum over t is an xor
// butterfly over the 64 lanes (lanes >= horizon hold 0), the same order for every scene; sqrtf and the division are
// correctly rounded.
//
// Drivable-area compliance (lgcn_eval_scenes_da, lgcn_eval_actors_da): eval_row<true> also looks every step of every mode up
// in the raster of the scene's city, in the launch that writes the record.  A point (x, y) is inside iff, with cx = rintf(x),
// cy = rintf(y) (half to even), u = cx m[0] + cy m[1] + m[2], v = cx m[3] + cy m[4] + m[5] in float64 (unfused, left to right),
// iu = trunc(u), iv = trunc(v): 0 < iu < W, 0 < iv < H (compared in float64, so a huge or NaN coordinate is outside) and
// raster[off + iv W + iu] != 0.  Mode j is compliant iff every step t < horizon is inside: one wave vote per mode, lanes >=
// horizon vote yes.  Record float [30] = sum_j 2^j [mode j compliant] (< 256: exact), [31] = 1 when the scene's city has a
// raster; both 0 for flag 0 / 2, a city id of -1, and through the entries without a map.  lgcn_eval_dac_reduce sums
// popcount(mask & (2^k - 1)) over the counted records as integers.
#include "lgcn_common.hpp"
#include "lgcn.h"

namespace lgcn {

constexpr int kEvalMaxMod = 8, kEvalMaxT = 64, kEvalRec = 32, kEvalWaves = 4;
constexpr int kReduceThreads = 1024, kReduceLanes = kReduceThreads / kEvalMaxMod;      // 128 slot lanes x 8 values of k
constexpr int kReduceDepth = 6;

struct EvalParams {
    const float *reg, *cls, *gt;
    const unsigned char *has;
    const int32_t *actor_off;
    const int64_t *slot;
    int n_scenes, n_mod, n_t, horizon;
    int64_t n_slots;
    float *rec, *traj, *score;
    int32_t *err;
};

// the drivable areas of a split: the cities' rasters back to back, bytes of (da_mat == 1); city [n_cities] on the device
struct DaParams {
    const unsigned char *raster;
    const lgcn_da_city_t *city;
    const int32_t *scene_city;      // [n_scenes]; -1: no map
    int n_cities;
};

// sum over the 64 lanes, every lane gets it; the order is fixed by the lane numbers alone
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, kWave);
    return v;
}

__device__ __forceinline__ bool finite32(float x) { return fabsf(x) <= 3.402823466e38f; }      // false for NaN

// The record of actor row `a` at table row `s`, by the whole wave (lane = step t).  `obs`: the observed steps t < horizon
// (wave-uniform, not empty); `local`: the row's index inside its scene.  The final displacement is taken at the last
// observed step, the mean over the observed steps (PredLoss's rule); an unobserved step's gt is never read.
// kDa: `da` (wave-uniform; nullptr: the scene has no map) is the city the row's modes are looked up in, floats [30], [31].
template <bool kDa>
__device__ __forceinline__ void eval_row(const EvalParams &p, const int64_t a, const int64_t s, const unsigned long long obs,
                                         const float local, const int lane, const unsigned char *raster = nullptr,
                                         const lgcn_da_city_t *da = nullptr) {
    const int M = p.n_mod, T = p.n_t, H = p.horizon;
    const int n_obs = __popcll(obs), t_last = 63 - __clzll(obs);
    const bool on = (obs >> lane) & 1ull;
    float *rec = p.rec + s * kEvalRec;
    float2 g = make_float2(0.f, 0.f);
    if (on) g = reinterpret_cast<const float2 *>(p.gt)[a * T + lane];
    const float c = lane < M ? p.cls[a * M + lane] : 0.f;
    bool bad = !finite32(g.x) || !finite32(g.y) || !finite32(c);
    if (p.traj != nullptr && lane < M) p.score[s * M + lane] = c;
    float v = lane == 0 ? 1.f : lane == 1 ? (float)M : lane == 2 ? (float)H : lane == 3 ? local      // this lane's float of the record
            : lane == 28 ? (float)(H - n_obs) : lane == 29 ? (float)(H - 1 - t_last) : 0.f;
    float fde_min = 0.f, ade_min = 0.f, c_max = 0.f;
    int j_min = 0;
    int mask = 0;
    int64_t da_off = 0;
    double da_w = 0., da_h = 0., m0 = 0., m1 = 0., m2 = 0., m3 = 0., m4 = 0., m5 = 0.;
    if (kDa && da != nullptr) {
        da_off = da->off; da_w = (double)da->w; da_h = (double)da->h;
        m0 = da->m[0]; m1 = da->m[1]; m2 = da->m[2]; m3 = da->m[3]; m4 = da->m[4]; m5 = da->m[5];
    }
    for (int j = 0; j < M; ++j) {
        float2 r = make_float2(0.f, 0.f);
        if (lane < T) {
            r = reinterpret_cast<const float2 *>(p.reg)[(a * M + j) * T + lane];
            if (p.traj != nullptr) reinterpret_cast<float2 *>(p.traj)[(s * M + j) * T + lane] = r;
        }
        if (lane < H) bad = bad || !finite32(r.x) || !finite32(r.y);
        if (kDa && da != nullptr) {
            bool in = true;
            if (lane < H) {
                const double cx = (double)rintf(r.x), cy = (double)rintf(r.y);
                const double iu = trunc(cx * m0 + cy * m1 + m2), iv = trunc(cx * m3 + cy * m4 + m5);
                in = iu > 0. && iu < da_w && iv > 0. && iv < da_h;      // false for NaN; inside: 1 <= iu <= W - 1, 1 <= iv <= H - 1
                if (in) in = raster[da_off + (int64_t)iv * (int64_t)da_w + (int64_t)iu] != 0;
            }
            if (__all(in)) mask |= 1 << j;
        }
        float d = 0.f;
        if (on) {
            const float dx = r.x - g.x, dy = r.y - g.y;
            d = sqrtf(dx * dx + dy * dy);
        }
        const float fde = __shfl(d, t_last, kWave);
        const float ade = wave_sum(d) / (float)n_obs;
        if (j == 0 || fde < fde_min) { fde_min = fde; ade_min = ade; j_min = j; }
        const float cj = __shfl(c, j, kWave);
        c_max = j == 0 ? cj : fmaxf(c_max, cj);
        const float e = lane <= j ? expf(c - c_max) : 0.f;
        const float prob = __shfl(e, j_min, kWave) / wave_sum(e);
        const int at = 4 + 3 * j;
        v = lane == at ? fde_min : lane == at + 1 ? ade_min : lane == at + 2 ? prob : v;
    }
    if (kDa && da != nullptr) v = lane == 30 ? (float)mask : lane == 31 ? 1.f : v;
    if (__any(bad)) v = lane == 0 ? 2.f : lane == 3 ? local : 0.f;
    if (lane < kEvalRec) rec[lane] = v;
}

// the observed steps t < horizon of row a, one bit per step (wave-uniform)
__device__ __forceinline__ unsigned long long observed(const EvalParams &p, const int64_t a, const int lane) {
    return __ballot(lane < p.horizon && p.has[a * p.n_t + lane] != 0);
}

// the city of scene b -> false when its id is not one of the table's (an argument error); *da = nullptr for id -1
__device__ __forceinline__ bool scene_city(const DaParams &d, const int b, const lgcn_da_city_t **da) {
    const int c = d.scene_city[b];
    *da = c >= 0 && c < d.n_cities ? d.city + c : nullptr;
    return c >= -1 && c < d.n_cities;
}

// one wave per scene, kEvalWaves scenes per workgroup; lane = step t
template <bool kDa>
__device__ __forceinline__ void eval_scenes_body(const EvalParams &p, const DaParams &d) {
    const int lane = threadIdx.x & (kWave - 1);
    const int b = blockIdx.x * kEvalWaves + (threadIdx.x >> 6);
    if (b >= p.n_scenes) return;
    const int64_t s = p.slot[b];
    if (s < 0 || s >= p.n_slots) {              // an argument error: flag it, write nothing
        if (lane == 0) p.err[0] = 1;
        return;
    }
    const lgcn_da_city_t *da = nullptr;
    if (kDa && !scene_city(d, b, &da) && lane == 0) p.err[0] = 1;      // flagged; the record is written without a map
    const int a0 = p.actor_off[b], a1 = p.actor_off[b + 1];
    const unsigned long long full = ~0ull >> (kWave - p.horizon);
    const unsigned long long obs = a1 > a0 ? observed(p, a0, lane) : 0ull;
    if (obs != full) {                          // the agent counts only with its whole future (test.py:86)
        if (lane < kEvalRec) p.rec[s * kEvalRec + lane] = 0.f;
        return;
    }
    eval_row<kDa>(p, a0, s, obs, 0.f, lane, d.raster, da);
}

__global__ __launch_bounds__(kEvalWaves * kWave) void k_eval_scenes(const EvalParams p) { eval_scenes_body<false>(p, DaParams{}); }
__global__ __launch_bounds__(kEvalWaves * kWave) void k_eval_scenes_da(const EvalParams p, const DaParams d) {
    eval_scenes_body<true>(p, d);
}

// one wave per actor row of the batch, kEvalWaves rows per workgroup; `slot` holds the table row of each scene's first actor
template <bool kDa>
__device__ __forceinline__ void eval_actors_body(const EvalParams &p, const int n_actors, const DaParams &d) {
    const int lane = threadIdx.x & (kWave - 1);
    const int a = blockIdx.x * kEvalWaves + (threadIdx.x >> 6);
    if (a >= n_actors) return;
    // the scene of row a: actor_off[lo] <= a < actor_off[hi] throughout, so equal entries (scenes without actors) are
    // stepped over and lo ends at the one scene that holds the row
    int lo = 0, hi = p.n_scenes;
    if (a < p.actor_off[0] || a >= p.actor_off[hi]) {      // a table that does not cover the rows: flag it, write nothing
        if (lane == 0) p.err[0] = 1;
        return;
    }
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (p.actor_off[mid] > a) hi = mid; else lo = mid;
    }
    const int i = a - p.actor_off[lo];
    const int64_t s = p.slot[lo] + i;
    if (s < 0 || s >= p.n_slots) {
        if (lane == 0) p.err[0] = 1;
        return;
    }
    const lgcn_da_city_t *da = nullptr;
    if (kDa && !scene_city(d, lo, &da) && lane == 0) p.err[0] = 1;     // flagged; the record is written without a map
    const unsigned long long obs = observed(p, a, lane);
    if (obs == 0ull) {
        if (lane < kEvalRec) p.rec[s * kEvalRec + lane] = lane == 3 ? (float)i : 0.f;
        return;
    }
    eval_row<kDa>(p, a, s, obs, (float)i, lane, d.raster, da);
}

__global__ __launch_bounds__(kEvalWaves * kWave) void k_eval_actors(const EvalParams p, const int n_actors) {
    eval_actors_body<false>(p, n_actors, DaParams{});
}
__global__ __launch_bounds__(kEvalWaves * kWave) void k_eval_actors_da(const EvalParams p, const int n_actors, const DaParams d) {
    eval_actors_body<true>(p, n_actors, d);
}

struct ReduceParams {
    const float *rec;
    int64_t n_slots;
    double miss_thr;
    double *out;          // [8, 6]
    int64_t *cnt;         // [3]; with a selection [4]
    int32_t *err;
    int who, max_missing; // the selection (kSel only): 0 all, 1 local index [3] == 0, 2 local index > 0; [28] <= max_missing
};

// One workgroup: thread = (slot lane l, k): the slots l, l + 128, ... in order, then a tree over the 128 lanes -- float64,
// the same order whatever the records hold.  out[k - 1] = sums over the flag-1 records with M >= k of
//   minADE_k, minFDE_k, [minFDE_k > miss_thr], (1 - p_k)^2 + minFDE_k, (1 - p_k)^2 + minADE_k, min(-log p_k, -log 0.05) + minADE_k
// kSel: a record the selection excludes is counted in cnt[3] and otherwise passed over, in its place in the order: the
// sums are those of the same table with the excluded rows zeroed.
template <bool kSel>
__global__ __launch_bounds__(kReduceThreads) void k_eval_reduce(const ReduceParams p) {
    constexpr int kCnt = kSel ? 4 : 3;
    __shared__ double s_sum[6][kReduceThreads];
    __shared__ int s_cnt[kCnt][kReduceLanes];
    __shared__ float s_mh[2][kReduceLanes];          // M, horizon of the lane's evaluated records; -1: none yet, -2: they differ
    const int tid = threadIdx.x, k = tid & (kEvalMaxMod - 1), l = tid >> 3;
    double acc[6] = {0., 0., 0., 0., 0., 0.};
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    float m0 = -1.f, h0 = -1.f;
    const double clip = -log(0.05);
    // kReduceDepth records per thread are requested before the first is used (the pass is bound by load latency, not by
    // bytes); they are then taken in slot order, so the order of the sums does not depend on the depth
    for (int64_t s0 = l; s0 < p.n_slots; s0 += kReduceDepth * kReduceLanes) {
        float4 head[kReduceDepth];
        float val[kReduceDepth][3], miss[kReduceDepth];
#pragma unroll
        for (int u = 0; u < kReduceDepth; ++u) {
            const int64_t s = s0 + u * kReduceLanes;
            head[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            val[u][0] = val[u][1] = val[u][2] = miss[u] = 0.f;
            if (s < p.n_slots) {
                const float *r = p.rec + s * kEvalRec;
                head[u] = *reinterpret_cast<const float4 *>(r);
                val[u][0] = r[4 + 3 * k]; val[u][1] = r[5 + 3 * k]; val[u][2] = r[6 + 3 * k];
                if (kSel) miss[u] = r[28];
            }
        }
#pragma unroll
        for (int u = 0; u < kReduceDepth; ++u) {
            if (s0 + u * kReduceLanes >= p.n_slots) continue;
            const int flag = head[u].x == 1.f ? 1 : head[u].x == 2.f ? 2 : 0;
            if (kSel) {
                const bool first = head[u].w == 0.f;
                if ((p.who == 1 && !first) || (p.who == 2 && first) || (flag == 1 && !(miss[u] <= (float)p.max_missing))) {
                    ++n3;
                    continue;
                }
            }
            n0 += flag == 0; n1 += flag == 1; n2 += flag == 2;
            if (flag != 1) continue;
            if (m0 == -1.f) { m0 = head[u].y; h0 = head[u].z; }
            else if (m0 != head[u].y || h0 != head[u].z) m0 = -2.f;
            if ((float)k < head[u].y) {
                const double fde = val[u][0], ade = val[u][1], q = 1.0 - (double)val[u][2];
                const double nl = -log((double)val[u][2]);
                acc[0] += ade;
                acc[1] += fde;
                acc[2] += fde > p.miss_thr ? 1.0 : 0.0;
                acc[3] += q * q + fde;
                acc[4] += q * q + ade;
                acc[5] += (nl < clip ? nl : clip) + ade;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) s_sum[i][tid] = acc[i];
    if (k == 0) { s_cnt[0][l] = n0; s_cnt[1][l] = n1; s_cnt[2][l] = n2; if (kSel) s_cnt[kCnt - 1][l] = n3; s_mh[0][l] = m0; s_mh[1][l] = h0; }
    __syncthreads();
    for (int w = kReduceLanes / 2; w >= 1; w >>= 1) {
        if (l < w) {
            const int o = tid + w * kEvalMaxMod;
#pragma unroll
            for (int i = 0; i < 6; ++i) s_sum[i][tid] += s_sum[i][o];
            if (k == 0) {
                for (int i = 0; i < kCnt; ++i) s_cnt[i][l] += s_cnt[i][l + w];
                const float ma = s_mh[0][l], mb = s_mh[0][l + w];
                if (ma == -1.f) { s_mh[0][l] = mb; s_mh[1][l] = s_mh[1][l + w]; }
                else if (mb != -1.f && (mb != ma || s_mh[1][l + w] != s_mh[1][l])) s_mh[0][l] = -2.f;
            }
        }
        __syncthreads();
    }
    if (l == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) p.out[k * 6 + i] = s_sum[i][tid];
    }
    if (tid < kCnt) p.cnt[tid] = s_cnt[tid][0];
    if (tid == 0) p.err[0] = s_mh[0][0] == -2.f ? 1 : 0;
}

// The compliance counts of a table: dac[k - 1] = sum over the counted records of popcount(mask & (2^k - 1)) for k <= M,
// dac[8] = n_dac, the counted records: flag 1, float [31] == 1, kept by the selection of k_eval_reduce<true> (who == 0 and
// max_missing >= the horizon keep every record).  Integers summed as integers: exact, and the same for any order.
// One workgroup; thread = slot lane (the slots tid, tid + 1024, ...); a thread sees at most 2^21 records, a wave's sum of
// the nine counts stays below 2^30, the sum over the waves is int64.
constexpr int kDacOut = kEvalMaxMod + 1;

__global__ __launch_bounds__(kReduceThreads) void k_eval_dac_reduce(const float *rec, const int64_t n_slots, const int who,
                                                                    const int max_missing, int64_t *dac) {
    __shared__ int64_t s_part[kReduceThreads / kWave][kDacOut];
    const int tid = threadIdx.x;
    int acc[kDacOut];
#pragma unroll
    for (int k = 0; k < kDacOut; ++k) acc[k] = 0;
    for (int64_t s = tid; s < n_slots; s += kReduceThreads) {
        const float *r = rec + s * kEvalRec;
        const float4 head = *reinterpret_cast<const float4 *>(r);
        const float4 tail = *reinterpret_cast<const float4 *>(r + 28);      // [28] missing steps, [30] mask, [31] has a raster
        const bool first = head.w == 0.f;
        if (head.x != 1.f || tail.w != 1.f) continue;
        if ((who == 1 && !first) || (who == 2 && first) || !(tail.x <= (float)max_missing)) continue;
        const int mask = (int)tail.z, M = (int)head.y;
        ++acc[kEvalMaxMod];
#pragma unroll
        for (int k = 1; k <= kEvalMaxMod; ++k)
            if (k <= M) acc[k - 1] += __popc(mask & ((1 << k) - 1));
    }
#pragma unroll
    for (int k = 0; k < kDacOut; ++k) {
        int v = acc[k];
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, kWave);
        if ((tid & (kWave - 1)) == 0) s_part[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < kDacOut) {
        int64_t t = 0;
        for (int w = 0; w < kReduceThreads / kWave; ++w) t += s_part[w][tid];
        dac[tid] = t;
    }
}

}  // namespace lgcn

using namespace lgcn;

// the checks of a lgcn_drivable_t, before any launch; the city table is read through its host copy
static int check_drivable(const lgcn_drivable_t *da) {
    LGCN_CHECK_PTR(da);
    if (da->n_cities < 1 || da->raster_bytes < 0) return LGCN_EINVAL;
    const void *ptrs[] = {da->raster, da->city, da->city_host, da->scene_city};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    for (int c = 0; c < da->n_cities; ++c) {
        const lgcn_da_city_t &t = da->city_host[c];
        if (t.h < 1 || t.w < 1 || t.off < 0) return LGCN_EINVAL;
        for (double m : t.m)
            if (!(fabs(m) <= 1.7976931348623157e308)) return LGCN_EINVAL;
    }
    for (int c = 0; c < da->n_cities; ++c)
        if (da->city_host[c].h > 0x7fffffff || da->city_host[c].w > 0x7fffffff) return LGCN_ESHAPE;
    for (int c = 0; c < da->n_cities; ++c) {      // a raster that ends behind the buffer: the lookup would read past it
        const lgcn_da_city_t &t = da->city_host[c];
        if (t.off > da->raster_bytes || t.h * t.w > da->raster_bytes - t.off) return LGCN_EINVAL;
    }
    LGCN_CHECK_ALIGN16(da->city);
    LGCN_CHECK_ALIGN16(da->scene_city);
    return LGCN_OK;
}

extern "C" int lgcn_eval_scenes(const float *reg, const float *cls, const float *gt, const unsigned char *has,
                                const int32_t *actor_off, const int64_t *slot, int64_t n_scenes, int n_mod, int n_t, int horizon,
                                int64_t n_slots, float *rec, float *traj, float *score, int32_t *err, void *stream) {
    if (n_scenes < 0 || n_slots < 0 || n_mod < 1 || n_t < 1 || horizon < 1 || horizon > n_t) return LGCN_EINVAL;
    if ((traj == nullptr) != (score == nullptr)) return LGCN_EINVAL;
    if (n_mod > kEvalMaxMod || n_t > kEvalMaxT || n_scenes > 0x7fffffff || n_slots > 0x7fffffff) return LGCN_ESHAPE;
    if (n_scenes == 0) return LGCN_OK;
    const void *ptrs[] = {reg, cls, gt, has, actor_off, slot, rec, err};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {reg, cls, gt, actor_off, slot, rec, traj, score, err};      // rows are read and written as float2 / float4
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    EvalParams p{reg, cls, gt, has, actor_off, slot, (int)n_scenes, n_mod, n_t, horizon, n_slots, rec, traj, score, err};
    const unsigned grid = (unsigned)((n_scenes + kEvalWaves - 1) / kEvalWaves);
    hipLaunchKernelGGL(k_eval_scenes, dim3(grid), dim3(kEvalWaves * kWave), 0, (hipStream_t)stream, p);
    return launch_status();
}

extern "C" int lgcn_eval_scenes_da(const float *reg, const float *cls, const float *gt, const unsigned char *has,
                                   const int32_t *actor_off, const int64_t *slot, int64_t n_scenes, int n_mod, int n_t, int horizon,
                                   int64_t n_slots, float *rec, float *traj, float *score, int32_t *err,
                                   const lgcn_drivable_t *da, void *stream) {
    if (n_scenes < 0 || n_slots < 0 || n_mod < 1 || n_t < 1 || horizon < 1 || horizon > n_t) return LGCN_EINVAL;
    if ((traj == nullptr) != (score == nullptr)) return LGCN_EINVAL;
    if (n_mod > kEvalMaxMod || n_t > kEvalMaxT || n_scenes > 0x7fffffff || n_slots > 0x7fffffff) return LGCN_ESHAPE;
    if (n_scenes == 0) return LGCN_OK;
    const void *ptrs[] = {reg, cls, gt, has, actor_off, slot, rec, err};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {reg, cls, gt, actor_off, slot, rec, traj, score, err};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    if (const int st = check_drivable(da)) return st;
    EvalParams p{reg, cls, gt, has, actor_off, slot, (int)n_scenes, n_mod, n_t, horizon, n_slots, rec, traj, score, err};
    DaParams d{da->raster, da->city, da->scene_city, da->n_cities};
    const unsigned grid = (unsigned)((n_scenes + kEvalWaves - 1) / kEvalWaves);
    hipLaunchKernelGGL(k_eval_scenes_da, dim3(grid), dim3(kEvalWaves * kWave), 0, (hipStream_t)stream, p, d);
    return launch_status();
}

extern "C" int lgcn_eval_reduce(const float *rec, int64_t n_slots, double miss_thr, double *out, int64_t *cnt, int32_t *err,
                                void *stream) {
    if (n_slots < 0) return LGCN_EINVAL;
    if (n_slots > 0x7fffffff) return LGCN_ESHAPE;
    if (n_slots == 0) return LGCN_OK;
    const void *ptrs[] = {rec, out, cnt, err};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    for (const void *q : ptrs) LGCN_CHECK_ALIGN16(q);
    ReduceParams p{rec, n_slots, miss_thr, out, cnt, err, 0, 0};
    hipLaunchKernelGGL(k_eval_reduce<false>, dim3(1), dim3(kReduceThreads), 0, (hipStream_t)stream, p);
    return launch_status();
}

extern "C" int lgcn_eval_actors(const float *reg, const float *cls, const float *gt, const unsigned char *has,
                                const int32_t *actor_off, const int64_t *slot_base, int64_t n_actors, int64_t n_scenes, int n_mod,
                                int n_t, int horizon, int64_t n_slots, float *rec, float *traj, float *score, int32_t *err,
                                void *stream) {
    if (n_actors < 0 || n_scenes < 0 || n_slots < 0 || n_mod < 1 || n_t < 1 || horizon < 1 || horizon > n_t) return LGCN_EINVAL;
    if ((traj == nullptr) != (score == nullptr)) return LGCN_EINVAL;
    if (n_mod > kEvalMaxMod || n_t > kEvalMaxT || n_scenes > 0x7fffffff || n_slots > 0x7fffffff) return LGCN_ESHAPE;
    if (n_actors > (1 << 24)) return LGCN_ESHAPE;          // record float [3], the local index, must hold it exactly
    if (n_actors == 0 || n_scenes == 0) return LGCN_OK;
    const void *ptrs[] = {reg, cls, gt, has, actor_off, slot_base, rec, err};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {reg, cls, gt, actor_off, slot_base, rec, traj, score, err};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    EvalParams p{reg, cls, gt, has, actor_off, slot_base, (int)n_scenes, n_mod, n_t, horizon, n_slots, rec, traj, score, err};
    const unsigned grid = (unsigned)((n_actors + kEvalWaves - 1) / kEvalWaves);
    hipLaunchKernelGGL(k_eval_actors, dim3(grid), dim3(kEvalWaves * kWave), 0, (hipStream_t)stream, p, (int)n_actors);
    return launch_status();
}

extern "C" int lgcn_eval_actors_da(const float *reg, const float *cls, const float *gt, const unsigned char *has,
                                   const int32_t *actor_off, const int64_t *slot_base, int64_t n_actors, int64_t n_scenes, int n_mod,
                                   int n_t, int horizon, int64_t n_slots, float *rec, float *traj, float *score, int32_t *err,
                                   const lgcn_drivable_t *da, void *stream) {
    if (n_actors < 0 || n_scenes < 0 || n_slots < 0 || n_mod < 1 || n_t < 1 || horizon < 1 || horizon > n_t) return LGCN_EINVAL;
    if ((traj == nullptr) != (score == nullptr)) return LGCN_EINVAL;
    if (n_mod > kEvalMaxMod || n_t > kEvalMaxT || n_scenes > 0x7fffffff || n_slots > 0x7fffffff) return LGCN_ESHAPE;
    if (n_actors > (1 << 24)) return LGCN_ESHAPE;
    if (n_actors == 0 || n_scenes == 0) return LGCN_OK;
    const void *ptrs[] = {reg, cls, gt, has, actor_off, slot_base, rec, err};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    const void *al[] = {reg, cls, gt, actor_off, slot_base, rec, traj, score, err};
    for (const void *q : al) LGCN_CHECK_ALIGN16(q);
    if (const int st = check_drivable(da)) return st;
    EvalParams p{reg, cls, gt, has, actor_off, slot_base, (int)n_scenes, n_mod, n_t, horizon, n_slots, rec, traj, score, err};
    DaParams d{da->raster, da->city, da->scene_city, da->n_cities};
    const unsigned grid = (unsigned)((n_actors + kEvalWaves - 1) / kEvalWaves);
    hipLaunchKernelGGL(k_eval_actors_da, dim3(grid), dim3(kEvalWaves * kWave), 0, (hipStream_t)stream, p, (int)n_actors, d);
    return launch_status();
}

extern "C" int lgcn_eval_dac_reduce(const float *rec, int64_t n_slots, int who, int max_missing, int64_t *dac, void *stream) {
    if (n_slots < 0 || who < 0 || who > 2 || max_missing < 0) return LGCN_EINVAL;
    if (n_slots > 0x7fffffff) return LGCN_ESHAPE;
    if (n_slots == 0) return LGCN_OK;
    LGCN_CHECK_PTR(rec);
    LGCN_CHECK_PTR(dac);
    LGCN_CHECK_ALIGN16(rec);
    LGCN_CHECK_ALIGN16(dac);
    hipLaunchKernelGGL(k_eval_dac_reduce, dim3(1), dim3(kReduceThreads), 0, (hipStream_t)stream, rec, n_slots, who, max_missing, dac);
    return launch_status();
}

extern "C" int lgcn_eval_reduce_sel(const float *rec, int64_t n_slots, double miss_thr, int who, int max_missing, double *out,
                                    int64_t *cnt, int32_t *err, void *stream) {
    if (n_slots < 0 || who < 0 || who > 2 || max_missing < 0) return LGCN_EINVAL;
    if (n_slots > 0x7fffffff) return LGCN_ESHAPE;
    if (n_slots == 0) return LGCN_OK;
    const void *ptrs[] = {rec, out, cnt, err};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    for (const void *q : ptrs) LGCN_CHECK_ALIGN16(q);
    ReduceParams p{rec, n_slots, miss_thr, out, cnt, err, who, max_missing};
    hipLaunchKernelGGL(k_eval_reduce<true>, dim3(1), dim3(kReduceThreads), 0, (hipStream_t)stream, p);
    return launch_status();
}
