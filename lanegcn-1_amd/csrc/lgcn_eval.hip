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
#include "lgcn_common.hpp"

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
__device__ __forceinline__ void eval_row(const EvalParams &p, const int64_t a, const int64_t s, const unsigned long long obs,
                                         const float local, const int lane) {
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
    for (int j = 0; j < M; ++j) {
        float2 r = make_float2(0.f, 0.f);
        if (lane < T) {
            r = reinterpret_cast<const float2 *>(p.reg)[(a * M + j) * T + lane];
            if (p.traj != nullptr) reinterpret_cast<float2 *>(p.traj)[(s * M + j) * T + lane] = r;
        }
        if (lane < H) bad = bad || !finite32(r.x) || !finite32(r.y);
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
    if (__any(bad)) v = lane == 0 ? 2.f : lane == 3 ? local : 0.f;
    if (lane < kEvalRec) rec[lane] = v;
}

// the observed steps t < horizon of row a, one bit per step (wave-uniform)
__device__ __forceinline__ unsigned long long observed(const EvalParams &p, const int64_t a, const int lane) {
    return __ballot(lane < p.horizon && p.has[a * p.n_t + lane] != 0);
}

// one wave per scene, kEvalWaves scenes per workgroup; lane = step t
__global__ __launch_bounds__(kEvalWaves * kWave) void k_eval_scenes(const EvalParams p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int b = blockIdx.x * kEvalWaves + (threadIdx.x >> 6);
    if (b >= p.n_scenes) return;
    const int64_t s = p.slot[b];
    if (s < 0 || s >= p.n_slots) {              // an argument error: flag it, write nothing
        if (lane == 0) p.err[0] = 1;
        return;
    }
    const int a0 = p.actor_off[b], a1 = p.actor_off[b + 1];
    const unsigned long long full = ~0ull >> (kWave - p.horizon);
    const unsigned long long obs = a1 > a0 ? observed(p, a0, lane) : 0ull;
    if (obs != full) {                          // the agent counts only with its whole future (test.py:86)
        if (lane < kEvalRec) p.rec[s * kEvalRec + lane] = 0.f;
        return;
    }
    eval_row(p, a0, s, obs, 0.f, lane);
}

// one wave per actor row of the batch, kEvalWaves rows per workgroup; `slot` holds the table row of each scene's first actor
__global__ __launch_bounds__(kEvalWaves * kWave) void k_eval_actors(const EvalParams p, const int n_actors) {
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
    const unsigned long long obs = observed(p, a, lane);
    if (obs == 0ull) {
        if (lane < kEvalRec) p.rec[s * kEvalRec + lane] = lane == 3 ? (float)i : 0.f;
        return;
    }
    eval_row(p, a, s, obs, (float)i, lane);
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

}  // namespace lgcn

using namespace lgcn;

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
