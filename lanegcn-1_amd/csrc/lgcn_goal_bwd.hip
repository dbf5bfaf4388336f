// Backward of the goal decoder (csrc/lgcn_goal.hip): lgcn_goal_refine_bwd and lgcn_goal_decode_bwd, the two launches
// that replace autograd's walk over the ~80 stock ops of the training path.  Exact fp32 (no FMA: -ffp-contract=off),
// forward quantities recomputed with the forward's own operations (so the masks v_j <= 0 and s == 0 are the forward's),
// every sum in a fixed order, no atomics, nothing saved per step.
//
// What is not differentiated, as in the reference and in the stock training path: the selection top_idx; a clamped
// speed (v_j <= 0: the reference's in-place v[v <= 0] = 0); a normalised sample that was exactly 0 and was replaced
// by 1.  The division by the row maximum is differentiated as autograd does it: the first maximal element receives
// -sum_t(d u_t * s_t / max) / max in addition to its own d u_t / max.
#include "lgcn_common.hpp"

namespace lgcn {

constexpr int kGoalMaxMod = 8, kGoalSteps = 30;
constexpr int kGoalThreads = 256;

// sum over the 64 lanes in a fixed butterfly order; every lane returns the sum
__device__ __forceinline__ float wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one wave per (agent, mode) row: lane t < 30 owns sample t
__global__ __launch_bounds__(64) void k_goal_refine_bwd(const float *__restrict__ s_samples, const float *__restrict__ coef,
                                                        const float *__restrict__ delta, const float *__restrict__ d_out,
                                                        float *__restrict__ d_ss, float *__restrict__ d_coef,
                                                        float *__restrict__ d_delta) {
    const int64_t row = blockIdx.x;
    const int t = threadIdx.x;
    const bool on = t < kGoalSteps;
    float s = 0.f, dn = 0.f, gx = 0.f, gy = 0.f;
    if (on) {
        const int64_t e = (row * kGoalSteps + t) * 2;
        s = s_samples[row * kGoalSteps + t] + delta[e];
        dn = delta[e + 1];
        gx = d_out[e];
        gy = d_out[e + 1];
    }
    float mx = on ? s : -INFINITY;
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(mx, off, 64);
        mx = (mx != mx || o != o) ? NAN : (o > mx ? o : mx);
    }
    const unsigned long long at_max = __ballot(on && s == mx);
    const int first_max = at_max ? __ffsll((long long)at_max) - 1 : -1;
    const float u = s / mx;
    const bool replaced = u == 0.0f;
    const float z = replaced ? 1.0f : u;
    const float *cf = coef + row * 6;
    const float a0 = cf[0], a1 = cf[1], b0 = cf[3], b1 = cf[4];
    const float tx = 2.f * a0 * z + a1, ty = 2.f * b0 * z + b1;
    // out.x = P.x - T.y dn,  out.y = P.y + T.x dn
    const float d_dn = gy * tx - gx * ty;
    float dz = gx * tx + gy * ty + 2.f * dn * (gy * a0 - gx * b0);
    if (!on) dz = 0.f;
    const float zz = z * z, z2dn = 2.f * z * dn;
    float c[6];
    c[0] = on ? gx * zz + gy * z2dn : 0.f;       // a0: x through s^2, y through the tangent 2 a0 s dn
    c[1] = on ? gx * z + gy * dn : 0.f;          // a1
    c[2] = on ? gx : 0.f;                        // a2
    c[3] = on ? gy * zz - gx * z2dn : 0.f;       // b0
    c[4] = on ? gy * z - gx * dn : 0.f;          // b1
    c[5] = on ? gy : 0.f;                        // b2
#pragma unroll
    for (int i = 0; i < 6; ++i) c[i] = wave_sum(c[i]);
    const float du = replaced ? 0.f : dz;
    const float d_mx = -wave_sum(on ? du * u / mx : 0.f);
    float ds = du / mx;
    if (t == first_max) ds += d_mx;
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) d_coef[row * 6 + i] = c[i];
    }
    if (!on) return;
    const int64_t e = (row * kGoalSteps + t) * 2;
    d_ss[row * kGoalSteps + t] = ds;
    d_delta[e] = ds;
    d_delta[e + 1] = d_dn;
}

struct GoalDecodeBwdParams {
    const float *pred;            // [n, 5]
    const int32_t *pred_off;      // [n_agt + 1]
    const float *anc_ctrs, *anc_dirs;
    const int32_t *anc_off;
    const float *agt_ctrs, *agt_dir_last, *agt_vel;
    int64_t n, n_anc;
    int n_agt, k;
    const int32_t *top_idx;       // [n_agt, k]
    const float *d_goals, *d_logits, *d_coef, *d_ss;
    float *d_pred;                // [n, 5]
};

// one workgroup per interest agent: zero its span of d_pred, then one thread per mode fills the selected row
__global__ __launch_bounds__(kGoalThreads) void k_goal_decode_bwd(const GoalDecodeBwdParams p) {
    const int a = blockIdx.x, tid = threadIdx.x, k = p.k;
    const int64_t lo = p.pred_off[a], hi = p.pred_off[a + 1], a0 = p.anc_off[a];
    if (!(lo >= 0 && hi >= lo && hi <= p.n)) return;               // a table that does not describe pred: touch nothing
    const int64_t n5 = (hi - lo) * 5;
    float *dp = p.d_pred + lo * 5;
    for (int64_t i = tid; i < n5; i += kGoalThreads) dp[i] = 0.f;
    __syncthreads();
    if (tid >= k) return;
    if (!(a0 >= 0 && a0 + (hi - lo) <= p.n_anc)) return;
    const int n = (int)(hi - lo), m = tid;
    const int64_t o = (int64_t)a * k + m;
    const int b = p.top_idx[o];
    if (b < 0 || b >= n) return;                                     // the forward refused this agent
    const float *pr = p.pred + (lo + b) * 5, *ac = p.anc_ctrs + (a0 + b) * 2, *ad = p.anc_dirs + (a0 + b) * 2;
    // ---- the forward, as k_goal_decode forms it
    const float p3 = pr[3], p4 = pr[4];
    const float gx = ac[0] + pr[1], gy = ac[1] + pr[2];
    const float theta = atan2f(ad[1], ad[0]) + atanf(p3 / p4);
    const float pdx = cosf(theta), pdy = sinf(theta);
    float dx = p.agt_dir_last[2 * a], dy = p.agt_dir_last[2 * a + 1];
    const float nrm = sqrtf(dx * dx + dy * dy);
    dx = dx / nrm;
    dy = dy / nrm;
    if (nrm < 1e-6f) { dx = 0.f; dy = 0.f; }
    const float cx = p.agt_ctrs[2 * a], cy = p.agt_ctrs[2 * a + 1];
    const float den_x = 2.f + dx - pdx, den_y = 2.f + dy - pdy;
    const float a1 = (2.f * gx * dx + 2.f * cx * dx) / den_x;
    const float c0 = gx - cx - a1;
    const float b1 = (2.f * gy * dy + 2.f * cy * dy) / den_y;
    const float d0 = gy - cy - b1;
    const float inv30 = (float)(1.0 / 30);
    float px, py;
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
    const float vel = p.agt_vel[a];
    const float acc = 2.f * (len - vel * 3.0f) / 9.0f;
    const float tenth = (float)0.1;
    // ---- s_samples[j - 1] = (v_0 + v_j) t_j / 2, v_j = max(vel + acc t_j, 0); v_0 does not depend on acc (t_0 = 0)
    const float *gs = p.d_ss + o * kGoalSteps;
    float d_acc = 0.f;
    for (int j = 1; j <= kGoalSteps; ++j) {
        const float t = tenth * (float)j;
        const float v = vel + acc * t;
        if (!(v <= 0.f)) d_acc += gs[j - 1] * t / 2.f * t;
    }
    const float d_len = d_acc * 2.f / 9.0f;
    // ---- L = sum_j |P(s_j) - P(s_(j-1))|: e_j = c0 (s_j^2 - s_(j-1)^2) + a1 (s_j - s_(j-1)) (and the same in y)
    const float *gc = p.d_coef + o * 6;
    float d_c0 = gc[0], d_a1 = gc[1], d_d0 = gc[3], d_b1 = gc[4];
    {
        const float s0 = inv30 * 0.f;
        px = c0 * (s0 * s0) + a1 * s0 + cx;
        py = d0 * (s0 * s0) + b1 * s0 + cy;
        float sp = s0;
        for (int j = 1; j <= kGoalSteps; ++j) {
            const float s = inv30 * (float)j;
            const float x = c0 * (s * s) + a1 * s + cx, y = d0 * (s * s) + b1 * s + cy;
            const float ex = x - px, ey = y - py;
            const float l = sqrtf(ex * ex + ey * ey);
            if (l > 0.f) {                       // a segment of length 0 has no direction: no gradient through it
                const float wx = d_len * (ex / l), wy = d_len * (ey / l);
                const float q2 = s * s - sp * sp, q1 = s - sp;
                d_c0 += wx * q2; d_a1 += wx * q1;
                d_d0 += wy * q2; d_b1 += wy * q1;
            }
            px = x; py = y; sp = s;
        }
    }
    // ---- c0 = g - c - a1;  a1 = (2 g d + 2 c d) / (2 + d - p)
    const float *gg = p.d_goals + o * 2;
    const float e_a1 = d_a1 - d_c0, e_b1 = d_b1 - d_d0;
    const float d_gx = gg[0] + d_c0 + e_a1 * (2.f * dx) / den_x;
    const float d_gy = gg[1] + d_d0 + e_b1 * (2.f * dy) / den_y;
    const float d_pdx = e_a1 * a1 / den_x, d_pdy = e_b1 * b1 / den_y;
    // ---- p = (cos theta, sin theta), theta = atan2(dir) + atan(p3 / p4)
    const float d_theta = d_pdy * pdx - d_pdx * pdy;
    const float q = p3 * p3 + p4 * p4;
    float *row = dp + (int64_t)b * 5;
    row[0] = p.d_logits[o];
    row[1] = d_gx;
    row[2] = d_gy;
    row[3] = d_theta * (p4 / q);
    row[4] = -(d_theta * (p3 / q));
}

}  // namespace lgcn

using namespace lgcn;

extern "C" int lgcn_goal_refine_bwd(const float *s_samples, const float *coef, const float *traj_delta, const float *d_pred_trajs,
                                    int64_t n_rows, float *d_s_samples, float *d_coef, float *d_traj_delta, void *stream) {
    if (n_rows < 0) return LGCN_EINVAL;
    if (n_rows > 0x7fffffff / (kGoalSteps * 2)) return LGCN_ESHAPE;
    if (n_rows == 0) return LGCN_OK;
    const void *ptrs[] = {s_samples, coef, traj_delta, d_pred_trajs, d_s_samples, d_coef, d_traj_delta};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    hipLaunchKernelGGL(k_goal_refine_bwd, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, s_samples, coef, traj_delta,
                       d_pred_trajs, d_s_samples, d_coef, d_traj_delta);
    return launch_status();
}

extern "C" int lgcn_goal_decode_bwd(const float *pred, const int32_t *pred_off, const int32_t *pred_off_host, int64_t n,
                                    const float *anc_ctrs, const float *anc_dirs, int64_t n_anc, const int32_t *anc_off,
                                    const int32_t *anc_off_host, const float *agt_ctrs, const float *agt_dir_last,
                                    const float *agt_vel, int n_agt, int k, const int32_t *top_idx, const float *d_goals,
                                    const float *d_logits, const float *d_coef, const float *d_s_samples, float *d_pred,
                                    void *stream) {
    if (n < 0 || n_anc < 0 || n_agt < 0 || k < 1 || k > kGoalMaxMod) return LGCN_EINVAL;
    if (n > 0x7fffffff / 5 || n_anc > 0x7fffffff / 2) return LGCN_ESHAPE;
    LGCN_CHECK_PTR(pred_off_host); LGCN_CHECK_PTR(anc_off_host);
    if (pred_off_host[0] != 0) return LGCN_EINVAL;
    for (int a = 0; a < n_agt; ++a) {
        const int64_t len = (int64_t)pred_off_host[a + 1] - pred_off_host[a];
        if (len < k || pred_off_host[a + 1] > n) return LGCN_EINVAL;
        if (anc_off_host[a] < 0 || anc_off_host[a] + len > n_anc) return LGCN_EINVAL;
    }
    if (pred_off_host[n_agt] != n) return LGCN_EINVAL;     // the spans cover d_pred: every row is written
    if (n_agt == 0) return LGCN_OK;
    const void *ptrs[] = {pred, pred_off, anc_ctrs, anc_dirs, anc_off, agt_ctrs, agt_dir_last, agt_vel, top_idx, d_goals, d_logits,
                          d_coef, d_s_samples, d_pred};
    for (const void *q : ptrs) LGCN_CHECK_PTR(q);
    GoalDecodeBwdParams p{pred, pred_off, anc_ctrs, anc_dirs, anc_off, agt_ctrs, agt_dir_last, agt_vel, n, n_anc, n_agt, k, top_idx,
                          d_goals, d_logits, d_coef, d_s_samples, d_pred};
    hipLaunchKernelGGL(k_goal_decode_bwd, dim3((unsigned)n_agt), dim3(kGoalThreads), 0, (hipStream_t)stream, p);
    return launch_status();
}
