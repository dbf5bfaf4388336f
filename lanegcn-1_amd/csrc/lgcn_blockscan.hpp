// Block scans and offset-table helpers of the batch kernels (lgcn_scene.hip, lgcn_graphbatch.hip): order comes from a
// block-wide exclusive scan plus per-block totals, so a scene may span any number of workgroups and no atomic is needed.
#pragma once
#include "lgcn_common.hpp"

namespace lgcn {

constexpr int kScThreads = 256;

// largest s in [0, n) with tab[s] <= x (tab ascending, tab[0] = 0 <= x)
__device__ __forceinline__ int sc_find_seg(const int32_t *tab, int n, int x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int sc_wave_scan(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
// Block-wide exclusive scan of one int per thread (kScThreads threads); lds [17].
__device__ __forceinline__ int sc_block_scan(int v, int *total, int *lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = kScThreads >> 6;
    const int inc = sc_wave_scan(v, lane);
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    if (w == 0) {
        const int t = lane < nw ? lds[lane] : 0;
        const int run = sc_wave_scan(t, lane);
        if (lane < nw) lds[lane] = run - t;
        if (lane == nw - 1) lds[16] = run;
    }
    __syncthreads();
    const int base = lds[w];
    *total = lds[16];
    __syncthreads();
    return base + inc - v;
}

// K values per thread: exclusive scan inside the block, the block's totals to sums[block * K + k]
template <int K>
__device__ __forceinline__ void sc_scan_local(const int (&v)[K], int (&excl)[K], int32_t *sums, int *lds) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int total;
        excl[k] = sc_block_scan(v[k], &total, lds);
        if (threadIdx.x == 0) sums[(int64_t)blockIdx.x * K + k] = total;
    }
}
// the totals of all blocks in front of this one
template <int K>
__device__ __forceinline__ void sc_block_base(const int32_t *sums, int (&base)[K], int *lds) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int part = 0;
        for (int i = threadIdx.x; i < (int)blockIdx.x; i += kScThreads) part += sums[(int64_t)i * K + k];
        sc_block_scan(part, &base[k], lds);
    }
}

__host__ __device__ inline int64_t sc_up4(int64_t n) { return (n + 3) & ~(int64_t)3; }
__host__ __device__ inline int64_t sc_blocks(int64_t n) { return (n + kScThreads - 1) / kScThreads; }

// ------------------------------------------------------------------ host side
inline int sc_check_table(const int32_t *tab, int64_t n, int64_t total) {
    if (tab[0] != 0) return LGCN_EINVAL;
    for (int64_t i = 0; i < n; ++i)
        if (tab[i + 1] < tab[i]) return LGCN_EINVAL;
    return tab[n] == total ? LGCN_OK : LGCN_EINVAL;
}

static inline bool sc_misaligned(const void *q, unsigned mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }

}  // namespace lgcn
