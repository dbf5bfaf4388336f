// Shape rules and helpers shared by ActorNet's convolution kernels (lgcn_conv.hip: forward, lgcn_conv_bwd.hip: backward).
#pragma once
#include "lgcn_common.hpp"

namespace lgcn {

constexpr int kConvRows = 80;          // output rows per workgroup (5 sub-blocks of 16): 80 / lout whole actors

__host__ __device__ inline int conv_kpad(int cin) { return (cin + 31) & ~31; }

// F.interpolate(scale_factor = 2, mode = "linear", align_corners = False) of a length-n sequence at output position j:
// source coordinate (j + 0.5) / 2 - 0.5, clamped at 0; weights 0.75 / 0.25 (and 1 / 0 at the two ends).
__device__ __forceinline__ void up2_taps(int j, int n, int &i0, int &i1, float &w1) {
    float src = (j + 0.5f) * 0.5f - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + 1 < n ? i0 + 1 : n - 1;
    w1 = src - (float)i0;
}

inline bool conv_shape_ok(int cin, int cout, int ks, int stride, int lin, int lout) {
    if (cin < 1 || cin > 128 || (cout != 32 && cout != 64 && cout != 128)) return false;
    if ((ks != 1 && ks != 3) || (stride != 1 && stride != 2) || lin < 1) return false;
    const int pad = (ks - 1) / 2;
    if (lout != (lin + 2 * pad - ks) / stride + 1) return false;
    return lout == 5 || lout == 10 || lout == 20;             // 16 / 8 / 4 actors per workgroup: 512 / na threads each in the GroupNorm phase
}

}  // namespace lgcn
