// Fused optimizer step (lgcn_opt_step): gradient clamp + Adam / AdamW / SGD over many fp32 tensors in ONE launch, in
// place, from a device table (include/lgcn.h; reference utils.py:98-162 Optimizer, whose update is torch.optim's).
// A streaming pass: no LDS, no atomics, no scratch; every element is touched by exactly one thread, so the result is
// bitwise repeatable.  Built with -ffp-contract=off like the rest of the library: the operations below are the
// separately rounded fp32 operations of torch.optim's single-tensor path, in its order.
#include "lgcn_common.hpp"

#include <cmath>

namespace lgcn {

constexpr int kOptChunk = 4096;        // elements of one chunk: 4 x (256 threads x 4 floats)
constexpr int kOptMaxGrid = 2048;      // memory-bound: 256 CUs x 8 workgroups, the rest grid-strides

static_assert(kOptChunk % 4 == 0, "a chunk starts on a 4-element boundary of its tensor");
static_assert(sizeof(lgcn_opt_tensor_t) == 40, "lgcn_opt_tensor_t layout: keep lanegcn-1_amd/_lib.py (OptTensor) in step");

// The table's pointers are plain device memory: say so, or every access is a flat_ instruction (the compiler cannot tell
// the address space of a pointer it loaded from memory).
using gfloat = __attribute__((address_space(1))) float;
using f32x4 = float __attribute__((ext_vector_type(4)));
using gfloat4 = __attribute__((address_space(1))) f32x4;

struct OptK {                          // the step's constants, formed on the host in double and rounded once
    float clip_low, clip_high;
    float wd;                          // coupled weight decay (Adam, SGD); 0: none
    float decay;                       // AdamW: 1 - lr * wd
    float w1, b2, w2;                  // 1 - beta1, beta2, 1 - beta2
    float neg_step;                    // Adam: -(lr / bc1); SGD: -lr
    float bc2_sqrt, eps;
    float mu;                          // SGD momentum
    int clip_on, has_wd, has_mom, first_step;
};

// One element.  g is written only by the clamp (the reference clamps p.grad in place; the weight-decay sum is a
// temporary in torch.optim too).  Comparisons, not fminf / fmaxf: a NaN gradient stays NaN, as clamp_ leaves it.
template <int KIND>
__device__ __forceinline__ void opt_elem(float &p, float &g, float &m, float &v, const OptK &k) {
    if (k.clip_on) g = g < k.clip_low ? k.clip_low : (g > k.clip_high ? k.clip_high : g);
    float ge = g;
    if (KIND == LGCN_OPT_ADAMW) {
        if (k.has_wd) p = p * k.decay;                                   // param.mul_(1 - lr * wd)
    } else if (k.has_wd) {
        ge = g + k.wd * p;                                               // grad.add(param, alpha=wd)
    }
    if (KIND == LGCN_OPT_SGD) {
        if (k.has_mom) {
            m = k.first_step ? ge : m * k.mu + ge;                       // clone(grad) | buf.mul_(mu).add_(grad)
            ge = m;
        }
        p = p + k.neg_step * ge;                                         // param.add_(grad, alpha=-lr)
    } else {
        const float d = ge - m;                                          // exp_avg.lerp_(grad, 1 - beta1)
        m = k.w1 < 0.5f ? m + k.w1 * d : ge - d * (1.f - k.w1);
        v = v * k.b2 + k.w2 * (ge * ge);                                 // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;               // (exp_avg_sq.sqrt() / bc2 ** 0.5).add_(eps)
        p = p + k.neg_step * (m / denom);                                // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_opt_step(const lgcn_opt_tensor_t *__restrict__ tensors, int n_tensors,
                                                  const int32_t *__restrict__ chunks, int n_chunks, const OptK k) {
    constexpr bool kAdam = KIND != LGCN_OPT_SGD;
    const bool use_m = kAdam || k.has_mom;
    const bool load_m = kAdam || (k.has_mom && !k.first_step);
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int32_t tid = chunks[2 * c], first = chunks[2 * c + 1];
        if (tid < 0 || tid >= n_tensors || first < 0) continue;          // a malformed table touches nothing
        const lgcn_opt_tensor_t t = tensors[tid];
        if (first >= t.n || t.p == nullptr || t.g == nullptr || (use_m && t.m == nullptr) || (kAdam && t.v == nullptr)) continue;
        const int len = (int)(t.n - first < kOptChunk ? t.n - first : kOptChunk);
        gfloat *const p = (gfloat *)(t.p + first), *const g = (gfloat *)(t.g + first);
        gfloat *const m = use_m ? (gfloat *)(t.m + first) : nullptr, *const v = kAdam ? (gfloat *)(t.v + first) : nullptr;
        const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;
        int done = 0;
        if ((bits & 15u) == 0) {                                         // 16-byte accesses on all four streams
            const int n4 = len >> 2;
            for (int i = threadIdx.x; i < n4; i += 256) {
                const f32x4 p4 = ((gfloat4 *)p)[i], g4 = ((gfloat4 *)g)[i];
                f32x4 m4 = {0.f, 0.f, 0.f, 0.f}, v4 = m4;
                if (load_m) m4 = ((gfloat4 *)m)[i];
                if (kAdam) v4 = ((gfloat4 *)v)[i];
                float pe[4], ge[4], me[4], ve[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pe[j] = p4[j]; ge[j] = g4[j]; me[j] = m4[j]; ve[j] = v4[j];
                    opt_elem<KIND>(pe[j], ge[j], me[j], ve[j], k);
                }
                ((gfloat4 *)p)[i] = f32x4{pe[0], pe[1], pe[2], pe[3]};
                if (k.clip_on) ((gfloat4 *)g)[i] = f32x4{ge[0], ge[1], ge[2], ge[3]};
                if (use_m) ((gfloat4 *)m)[i] = f32x4{me[0], me[1], me[2], me[3]};
                if (kAdam) ((gfloat4 *)v)[i] = f32x4{ve[0], ve[1], ve[2], ve[3]};
            }
            done = n4 << 2;                                              // the tail (len % 4 elements) below
        }
        for (int i = done + threadIdx.x; i < len; i += 256) {            // a pointer off 16 bytes (views of a flat gradient bucket)
            float pe = p[i], ge = g[i], me = 0.f, ve = 0.f;
            if (load_m) me = m[i];
            if (kAdam) ve = v[i];
            opt_elem<KIND>(pe, ge, me, ve, k);
            p[i] = pe;
            if (k.clip_on) g[i] = ge;
            if (use_m) m[i] = me;
            if (kAdam) v[i] = ve;
        }
    }
}

}  // namespace lgcn

using namespace lgcn;

extern "C" {

int lgcn_opt_chunk_elems(void) { return kOptChunk; }

int lgcn_opt_step(const lgcn_opt_tensor_t *tensors, int n_tensors, const int32_t *chunks, int n_chunks, int kind,
                  double lr, double beta1, double beta2, double eps, double weight_decay, double momentum, int first_step,
                  double bc1, double bc2, int clip_on, float clip_low, float clip_high, void *stream) {
    if (kind != LGCN_OPT_ADAM && kind != LGCN_OPT_ADAMW && kind != LGCN_OPT_SGD) return LGCN_EINVAL;
    if (n_chunks < 0 || n_tensors < 0) return LGCN_EINVAL;
    if (!std::isfinite(lr)) return LGCN_EINVAL;
    if (clip_on && !(clip_low <= clip_high)) return LGCN_EINVAL;
    if (kind != LGCN_OPT_SGD && !(bc1 > 0.0 && bc2 > 0.0)) return LGCN_EINVAL;    // 1 - beta^t of a step t >= 1
    if (n_chunks == 0) return LGCN_OK;
    LGCN_CHECK_PTR(tensors); LGCN_CHECK_PTR(chunks);
    if (n_tensors == 0) return LGCN_EINVAL;
    OptK k;
    k.clip_low = clip_low; k.clip_high = clip_high; k.clip_on = clip_on != 0;
    k.has_wd = weight_decay != 0.0;
    k.wd = (float)weight_decay;
    k.decay = (float)(1.0 - lr * weight_decay);
    k.w1 = (float)(1.0 - beta1); k.b2 = (float)beta2; k.w2 = (float)(1.0 - beta2);
    k.neg_step = kind == LGCN_OPT_SGD ? (float)-lr : (float)-(lr / bc1);
    k.bc2_sqrt = kind == LGCN_OPT_SGD ? 1.f : (float)std::sqrt(bc2);
    k.eps = (float)eps;
    k.mu = (float)momentum; k.has_mom = momentum != 0.0; k.first_step = first_step != 0;
    const dim3 grid(n_chunks < kOptMaxGrid ? n_chunks : kOptMaxGrid), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (kind == LGCN_OPT_ADAM) hipLaunchKernelGGL(k_opt_step<LGCN_OPT_ADAM>, grid, block, 0, s, tensors, n_tensors, chunks, n_chunks, k);
    else if (kind == LGCN_OPT_ADAMW) hipLaunchKernelGGL(k_opt_step<LGCN_OPT_ADAMW>, grid, block, 0, s, tensors, n_tensors, chunks, n_chunks, k);
    else hipLaunchKernelGGL(k_opt_step<LGCN_OPT_SGD>, grid, block, 0, s, tensors, n_tensors, chunks, n_chunks, k);
    return launch_status();
}

}  // extern "C"
