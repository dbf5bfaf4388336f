// Goal decoder of the fork model (reference lanercnn.py: nms_select 687-708, compute_coefficent 710-723,
// sample_trajectory / sample_d1_trajectory 728-737, Decode.forward 802-865 and 899-919).
//
// The reference selects goals in a Python loop over every node of every RoI (one host read, one vstack and one `in`
// test per node) and forms the trajectories with ~80 ATen launches; here the selection of all segments is one launch,
// the selection plus everything up to the arc-length samples of all interest agents is one launch, and the refinement
// is one launch.  All arithmetic is fp32 with every operation rounded on its own (the library is built with
// -ffp-contract=off), in the reference's order, so the comparisons that decide indices are the reference's.
//
// Greedy NMS without a sort: "take the highest-logit live node, drop every live node closer than threshold to it"
// repeated is the reference's walk over the sorted list (a node is visited after every node that outranks it, and is
// dropped iff one of the kept ones among those is closer than threshold).  lgcn_nms_select keeps the per-node state in
// the low 2 bits of the segment's own idx words and the growing list in their upper 30 bits (one writer per word: the
// thread that owns the node of that position), so there is no workspace and no cap on the segment size;
// lgcn_goal_decode keeps at most 8 nodes and re-derives liveness from that list.
#include "lgcn_common.hpp"

namespace lgcn {

constexpr int kGoalMaxMod = 8, kGoalSteps = 30;
constexpr int kGoalThreads = 256;

// rank order of torch.sort(descending=True) with the two open cases decided: NaN above every number, lower index first
// among equals (and among NaNs)
__device__ __forceinline__ bool outranks(float a, int ia, float b, int ib) {
    if (ib < 0) return ia >= 0;
    if (ia < 0) return false;
    const bool na = a != a, nb = b != b;
    if (na != nb) return na;
    if (!na && a != b) return a > b;
    return ia < ib;
}

// arg-max over the workgroup of (logit, index) candidates under outranks(); index -1 = no candidate.  Every thread
// returns the winner.  s_v / s_i: one slot per wave.
__device__ __forceinline__ int block_argmax(float v, int i, float *s_v, int *s_i) {
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(v, off, 64);
        const int oi = __shfl_down(i, off, 64);
        if (outranks(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                      // the slots of the previous call have been read
    if ((threadIdx.x & 63) == 0) { s_v[wave] = v; s_i[wave] = i; }
    __syncthreads();
    v = s_v[0]; i = s_i[0];
    for (int w = 1; w < kGoalThreads / 64; ++w)
        if (outranks(s_v[w], s_i[w], v, i)) { v = s_v[w]; i = s_i[w]; }
    return i;
}

__device__ __forceinline__ float dist2d(float ax, float ay, float bx, float by) {
    const float dx = ax - bx, dy = ay - by;
    return sqrtf(dx * dx + dy * dy);      // correctly rounded sqrt; no contraction
}

enum { ST_LIVE = 0, ST_KEPT = 1, ST_DROPPED = 2, ST_PAD = 3 };

__global__ __launch_bounds__(kGoalThreads) void k_nms_select(const float *__restrict__ xys, const float *__restrict__ logits,
                                                             const int32_t *__restrict__ seg_off, int64_t n_total, float threshold,
                                                             int min_len, int max_keep, int32_t *__restrict__ idx,
                                                             int32_t *__restrict__ count) {
    __shared__ float s_v[kGoalThreads / 64];
    __shared__ int s_i[kGoalThreads / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    int64_t lo = seg_off[s], hi = seg_off[s + 1];
    if (lo < 0 || hi < lo || hi > n_total) {         // an offset table that does not describe [0, n): touch nothing
        if (tid == 0) count[s] = 0;
        return;
    }
    const int n = (int)(hi - lo);
    const float *xy = xys + lo * 2, *lg = logits + lo;
    int32_t *w = idx + lo;
    for (int i = tid; i < n; i += kGoalThreads) w[i] = ST_LIVE;
    const int limit = max_keep > 0 && max_keep < n ? max_keep : n;
    int cnt = 0;
    // greedy survivors
    while (cnt < limit) {
        float bv = 0.f;
        int bi = -1;
        for (int i = tid; i < n; i += kGoalThreads)
            if ((w[i] & 3) == ST_LIVE && outranks(lg[i], i, bv, bi)) { bv = lg[i]; bi = i; }
        const int b = block_argmax(bv, bi, s_v, s_i);
        if (b < 0) break;
        const float bx = xy[2 * b], by = xy[2 * b + 1];
        for (int i = tid; i < n; i += kGoalThreads) {
            const int32_t old = w[i];
            int32_t st = old & 3, entry = old >> 2;
            if (i == b) st = ST_KEPT;
            else if (st == ST_LIVE && dist2d(bx, by, xy[2 * i], xy[2 * i + 1]) < threshold) st = ST_DROPPED;
            if (i == cnt) entry = b + 1;
            const int32_t now = (entry << 2) | st;
            if (now != old) w[i] = now;
        }
        ++cnt;
        __syncthreads();
    }
    // padding: the highest-logit dropped nodes, up to min_len entries
    const int want = min_len < limit ? min_len : limit;
    while (cnt < want) {
        float bv = 0.f;
        int bi = -1;
        for (int i = tid; i < n; i += kGoalThreads)
            if ((w[i] & 3) == ST_DROPPED && outranks(lg[i], i, bv, bi)) { bv = lg[i]; bi = i; }
        const int b = block_argmax(bv, bi, s_v, s_i);
        if (b < 0) break;
        for (int i = tid; i < n; i += kGoalThreads) {
            const int32_t old = w[i];
            int32_t st = old & 3, entry = old >> 2;
            if (i == b) st = ST_PAD;
            if (i == cnt) entry = b + 1;
            const int32_t now = (entry << 2) | st;
            if (now != old) w[i] = now;
        }
        ++cnt;
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < n; i += kGoalThreads) w[i] = (w[i] >> 2) - 1;
    if (tid == 0) count[s] = cnt;
}

struct GoalDecodeParams {
    const float *pred;            // [n, 5]
    const int32_t *pred_off;      // [n_agt + 1]
    const float *anc_ctrs, *anc_dirs;   // [n_anc, 2]
    const int32_t *anc_off;       // [n_agt]
    const float *agt_ctrs, *agt_dir_last, *agt_vel;
    int64_t n, n_anc;
    int n_agt, k;
    float threshold;
    int32_t *top_idx;             // [n_agt, k]
    float *goals, *logits, *coef, *s_samples;
};

__global__ __launch_bounds__(kGoalThreads) void k_goal_decode(const GoalDecodeParams p) {
    __shared__ float s_v[kGoalThreads / 64];
    __shared__ int s_i[kGoalThreads / 64];
    __shared__ float s_kx[kGoalMaxMod], s_ky[kGoalMaxMod];
    __shared__ int s_ki[kGoalMaxMod];
    const int a = blockIdx.x, tid = threadIdx.x, k = p.k;
    const int64_t lo = p.pred_off[a], hi = p.pred_off[a + 1], a0 = p.anc_off[a];
    const bool ok = lo >= 0 && hi >= lo + k && hi <= p.n && a0 >= 0 && a0 + (hi - lo) <= p.n_anc;
    if (!ok) {                            // offsets that do not describe the tensors: no read through them
        if (tid < k) p.top_idx[a * k + tid] = -1;
        return;
    }
    const int n = (int)(hi - lo);
    const float *pr = p.pred + lo * 5, *ac = p.anc_ctrs + a0 * 2, *ad = p.anc_dirs + a0 * 2;
    int cnt = 0;
    // greedy survivors: live = not listed and not closer than threshold to a listed node
    while (cnt < k) {
        float bv = 0.f;
        int bi = -1;
        for (int i = tid; i < n; i += kGoalThreads) {
            const float x = ac[2 * i] + pr[5 * i + 1], y = ac[2 * i + 1] + pr[5 * i + 2];
            bool live = true;
            for (int j = 0; j < cnt; ++j)
                if (s_ki[j] == i || dist2d(s_kx[j], s_ky[j], x, y) < p.threshold) live = false;
            if (live && outranks(pr[5 * i], i, bv, bi)) { bv = pr[5 * i]; bi = i; }
        }
        const int b = block_argmax(bv, bi, s_v, s_i);      // its barriers order the list reads above before the write below
        if (b < 0) break;
        if (tid == 0) {
            s_ki[cnt] = b;
            s_kx[cnt] = ac[2 * b] + pr[5 * b + 1];
            s_ky[cnt] = ac[2 * b + 1] + pr[5 * b + 2];
        }
        ++cnt;
        __syncthreads();
    }
    // padding: the highest-logit nodes not listed yet (n >= k: always found)
    while (cnt < k) {
        float bv = 0.f;
        int bi = -1;
        for (int i = tid; i < n; i += kGoalThreads) {
            bool free_ = true;
            for (int j = 0; j < cnt; ++j)
                if (s_ki[j] == i) free_ = false;
            if (free_ && outranks(pr[5 * i], i, bv, bi)) { bv = pr[5 * i]; bi = i; }
        }
        const int b = block_argmax(bv, bi, s_v, s_i);
        if (b < 0) break;
        if (tid == 0) {
            s_ki[cnt] = b;
            s_kx[cnt] = ac[2 * b] + pr[5 * b + 1];
            s_ky[cnt] = ac[2 * b + 1] + pr[5 * b + 2];
        }
        ++cnt;
        __syncthreads();
    }
    if (tid >= k) return;
    // one thread per mode from here on
    const int m = tid, b = s_ki[m];
    const int64_t o = (int64_t)a * k + m;
    p.top_idx[o] = b;
    const float gx = s_kx[m], gy = s_ky[m];
    p.goals[o * 2] = gx;
    p.goals[o * 2 + 1] = gy;
    p.logits[o] = pr[5 * b];
    const float theta = atan2f(ad[2 * b + 1], ad[2 * b]) + atanf(pr[5 * b + 3] / pr[5 * b + 4]);
    const float pdx = cosf(theta), pdy = sinf(theta);
    // agent direction: last observed step, normalised; below 1e-6 it is zero (:845-848)
    float dx = p.agt_dir_last[2 * a], dy = p.agt_dir_last[2 * a + 1];
    const float nrm = sqrtf(dx * dx + dy * dy);
    dx = dx / nrm;
    dy = dy / nrm;
    if (nrm < 1e-6f) { dx = 0.f; dy = 0.f; }
    const float cx = p.agt_ctrs[2 * a], cy = p.agt_ctrs[2 * a + 1];
    // :715-720
    const float a1 = (2.f * gx * dx + 2.f * cx * dx) / (2.f + dx - pdx);
    const float c0 = gx - cx - a1;
    const float b1 = (2.f * gy * dy + 2.f * cy * dy) / (2.f + dy - pdy);
    const float d0 = gy - cy - b1;
    float *cf = p.coef + o * 6;
    cf[0] = c0; cf[1] = a1; cf[2] = cx; cf[3] = d0; cf[4] = b1; cf[5] = cy;
    // length of the 31-point polyline at s = j / 30 (:851-855)
    const float inv30 = (float)(1.0 / 30);
    float px = cx, py = cy;               // s = 0: a0 * 0 + a1 * 0 + a2
    {
        const float s0 = inv30 * 0.f;
        px = c0 * (s0 * s0) + a1 * s0 + cx;
        py = d0 * (s0 * s0) + b1 * s0 + cy;
    }
    float len = 0.f;
    for (int j = 1; j <= kGoalSteps; ++j) {
        const float s = inv30 * (float)j;
        const float x = c0 * (s * s) + a1 * s + cx, y = d0 * (s * s) + b1 * s + cy;
        const float ex = x - px, ey = y - py;
        len += sqrtf(ex * ex + ey * ey);
        px = x; py = y;
    }
    // constant acceleration over 3 s that covers that length, speeds clamped at zero (:856-861)
    const float vel = p.agt_vel[a];
    const float acc = 2.f * (len - vel * 3.0f) / 9.0f;
    const float tenth = (float)0.1;
    float v0 = vel + acc * (tenth * 0.f);
    if (v0 <= 0.f) v0 = 0.f;
    float *ss = p.s_samples + o * kGoalSteps;
    for (int j = 1; j <= kGoalSteps; ++j) {
        const float t = tenth * (float)j;
        float v = vel + acc * t;
        if (v <= 0.f) v = 0.f;
        ss[j - 1] = (v0 + v) * t / 2.f;
    }
}

// one wave per (agent, mode) row: lane t < 30 owns sample t (:899-919)
__global__ __launch_bounds__(64) void k_goal_refine(const float *__restrict__ s_samples, const float *__restrict__ coef,
                                                    const float *__restrict__ delta, float *__restrict__ out) {
    const int64_t row = blockIdx.x;
    const int t = threadIdx.x;
    const bool on = t < kGoalSteps;
    float s = 0.f, dn = 0.f;
    if (on) {
        s = s_samples[row * kGoalSteps + t] + delta[(row * kGoalSteps + t) * 2];
        dn = delta[(row * kGoalSteps + t) * 2 + 1];
    }
    // maximum as torch.max forms it: a NaN wins
    float mx = on ? s : -INFINITY;
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(mx, off, 64);
        mx = (mx != mx || o != o) ? NAN : (o > mx ? o : mx);
    }
    if (!on) return;
    s = s / mx;
    if (s == 0.0f) s = 1.0f;
    const float *cf = coef + row * 6;
    const float a0 = cf[0], a1 = cf[1], a2 = cf[2], b0 = cf[3], b1 = cf[4], b2 = cf[5];
    const float x = a0 * (s * s) + a1 * s + a2, y = b0 * (s * s) + b1 * s + b2;
    const float tx = 2.f * a0 * s + a1, ty = 2.f * b0 * s + b1;
    // [[0, -1], [1, 0]] applied as the reference's matmul forms it (both products, then their sum)
    const float rx = 0.0f * tx + -1.0f * ty, ry = 1.0f * tx + 0.0f * ty;
    out[(row * kGoalSteps + t) * 2] = x + rx * dn;
    out[(row * kGoalSteps + t) * 2 + 1] = y + ry * dn;
}

}  // namespace lgcn

using namespace lgcn;

extern "C" int lgcn_nms_select(const float *xys, const float *logits, const int32_t *seg_off, int64_t n, int n_seg,
                               float threshold, int min_len, int max_keep, int32_t *idx, int32_t *count, void *stream) {
    if (n < 0 || n_seg < 0 || min_len < 0 || threshold != threshold) return LGCN_EINVAL;
    if (n > (int64_t)1 << 28) return LGCN_ESHAPE;          // list entries share a word with the 2 state bits
    LGCN_CHECK_PTR(seg_off);
    if (n_seg == 0) return LGCN_OK;
    LGCN_CHECK_PTR(count);
    if (n > 0) { LGCN_CHECK_PTR(xys); LGCN_CHECK_PTR(logits); LGCN_CHECK_PTR(idx); }
    hipLaunchKernelGGL(k_nms_select, dim3((unsigned)n_seg), dim3(kGoalThreads), 0, (hipStream_t)stream, xys, logits, seg_off, n,
                       threshold, min_len, max_keep, idx, count);
    return launch_status();
}

extern "C" int lgcn_goal_decode(const float *pred, const int32_t *pred_off, const int32_t *pred_off_host, int64_t n,
                                const float *anc_ctrs, const float *anc_dirs, int64_t n_anc, const int32_t *anc_off,
                                const int32_t *anc_off_host, const float *agt_ctrs, const float *agt_dir_last,
                                const float *agt_vel, int n_agt, int k, float threshold, int32_t *top_idx, float *goals,
                                float *logits, float *coef, float *s_samples, void *stream) {
    if (n < 0 || n_anc < 0 || n_agt < 0 || k < 1 || k > kGoalMaxMod || threshold != threshold) return LGCN_EINVAL;
    if (n > 0x7fffffff / 5 || n_anc > 0x7fffffff / 2) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(pred_off_host); LGCN_CHECK_PTR(anc_off_host);
    if (pred_off_host[0] != 0) return LGCN_EINVAL;
    for (int a = 0; a < n_agt; ++a) {
        const int64_t len = (int64_t)pred_off_host[a + 1] - pred_off_host[a];
        if (len < k || pred_off_host[a + 1] > n) return LGCN_EINVAL;              // a RoI shorter than k (the reference's cat fails)
        if (anc_off_host[a] < 0 || anc_off_host[a] + len > n_anc) return LGCN_EINVAL;
    }
    if (n_agt == 0) return LGCN_OK;
    const void *ptrs[] = {pred, pred_off, anc_ctrs, anc_dirs, anc_off, agt_ctrs, agt_dir_last, agt_vel, top_idx, goals, logits, coef,
                          s_samples};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    GoalDecodeParams p{pred, pred_off, anc_ctrs, anc_dirs, anc_off, agt_ctrs, agt_dir_last, agt_vel, n, n_anc, n_agt, k, threshold,
                       top_idx, goals, logits, coef, s_samples};
    hipLaunchKernelGGL(k_goal_decode, dim3((unsigned)n_agt), dim3(kGoalThreads), 0, (hipStream_t)stream, p);
    return launch_status();
}

extern "C" int lgcn_goal_refine(const float *s_samples, const float *coef, const float *traj_delta, int64_t n_rows,
                                float *pred_trajs, void *stream) {
    if (n_rows < 0) return LGCN_EINVAL;
    if (n_rows > 0x7fffffff / (kGoalSteps * 2)) return LGCN_ESHAPE;
    if (n_rows == 0) return LGCN_OK;
    LGCN_CHECK_PTR(s_samples); LGCN_CHECK_PTR(coef); LGCN_CHECK_PTR(traj_delta); LGCN_CHECK_PTR(pred_trajs);
    hipLaunchKernelGGL(k_goal_refine, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, s_samples, coef, traj_delta,
                       pred_trajs);
    return launch_status();
}
