// Prefix scans and offset-table helpers of the integer kernels: the one copy of each, for the CSR plan and pair search
// (lgcn_index.hip), lane-RoI extraction (lgcn_roi.hip), scene construction (lgcn_scene.hip), the batched graph ops
// (lgcn_graphbatch.hip) and the store (lgcn_store.hip).  Order comes from an exclusive scan inside the block plus per-block
// totals, so a segment may span any number of workgroups and no atomic is needed.  Everything is integer addition: a result
// does not depend on the order in which a scan adds.
#pragma once
#include "lgcn_common.hpp"

namespace lgcn {

constexpr int kScThreads = 256;

// largest s in [0, n) with tab[s] <= x, for tab ascending with tab[0] <= x (tab[0] and tab[n] are not read).  Equal
// neighbours -- empty scenes, relations or runs -- are skipped by taking the LAST such s.
template <typename T>
__device__ __forceinline__ int find_seg(const T *tab, int n, T x) {
    int lo = 0, hi = n;      // invariant: tab[lo] <= x < tab[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// Inclusive scan over the 64 lanes at VALU speed: Hillis-Steele inside every row of 16 lanes (DPP row_shr 1, 2, 4, 8: a lane
// without a source lane adds 0), then the last lane of row 0 / 2 into rows 1 / 3 (row_bcast:15) and lane 31 into rows 2
// and 3 (row_bcast:31).  (__shfl_up is ds_bpermute: an LDS round trip per step.)
// Precondition: all 64 lanes of the wave are active at the call (DPP reads an inactive source lane as 0).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add_from(int v) {
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ int wave_inclusive_scan(int v) {
    v = dpp_add_from<0x111, 0xf>(v);
    v = dpp_add_from<0x112, 0xf>(v);
    v = dpp_add_from<0x114, 0xf>(v);
    v = dpp_add_from<0x118, 0xf>(v);
    v = dpp_add_from<0x142, 0xa>(v);
    v = dpp_add_from<0x143, 0xc>(v);
    return v;
}

// Block-wide exclusive scan of one value per thread; returns the exclusive prefix, *total = block sum.  NT threads
// (multiple of 64, <= 1024), every one of which makes the call (it holds __syncthreads()); lds [NT/64 + 1], the total in
// the last slot.
template <int NT>
__device__ __forceinline__ int block_exclusive_scan(int v, int *total, int *lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = wave_inclusive_scan(v);
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    if (w == 0) {      // the wave totals are scanned by the first wave (it was a serial loop of one thread: 16 LDS round trips)
        const int t = lane < NT / 64 ? lds[lane] : 0;
        const int run = wave_inclusive_scan(t);
        if (lane < NT / 64) lds[lane] = run - t;
        if (lane == NT / 64 - 1) lds[NT / 64] = run;
    }
    __syncthreads();
    const int base = lds[w];
    *total = lds[NT / 64];
    __syncthreads();
    return base + inc - v;
}

// The totals of all blocks in front of this one: sums[i * stride] added up over i < blockIdx.x, in every thread.
template <int NT, typename T>
__device__ __forceinline__ int block_base(const T *sums, int stride, int *lds) {
    int part = 0;
    for (int i = threadIdx.x; i < (int)blockIdx.x; i += NT) part += (int)sums[(int64_t)i * stride];
    int base;
    block_exclusive_scan<NT>(part, &base, lds);
    return base;
}

// K values per thread (kScThreads threads): exclusive scan inside the block, the block's totals to sums[block * K + k]
template <int K>
__device__ __forceinline__ void sc_scan_local(const int (&v)[K], int (&excl)[K], int32_t *sums, int *lds) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int total;
        excl[k] = block_exclusive_scan<kScThreads>(v[k], &total, lds);
        if (threadIdx.x == 0) sums[(int64_t)blockIdx.x * K + k] = total;
    }
}
// the totals of all blocks in front of this one
template <int K>
__device__ __forceinline__ void sc_block_base(const int32_t *sums, int (&base)[K], int *lds) {
#pragma unroll
    for (int k = 0; k < K; ++k) base[k] = block_base<kScThreads>(sums + k, K, lds);
}

__host__ __device__ inline int64_t up4(int64_t n) { return (n + 3) & ~(int64_t)3; }
__host__ __device__ inline int64_t sc_blocks(int64_t n) { return (n + kScThreads - 1) / kScThreads; }

// ------------------------------------------------------------------ device-wide exclusive scan
// Exclusive scan of int32: per-block scan + block totals, then an add-back in which every block sums the totals
// before it (two launches; one when a single block holds everything).  Beyond 4096 blocks the totals are scanned by
// their own single-block launch first, so that no block walks more than 4096 totals: that bounds the CSR plan's scan
// and, on very large batches, lane-RoI's (rows of 14 relations per node).
// The kernels are static, as a header needs: every file that includes this one compiles its own copy of the four, and
// lgcn_index.hip and lgcn_roi.hip launch theirs.
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanThreads * kScanItems;

static __global__ __launch_bounds__(kScanThreads) void k_scan_blocks(const int32_t *in, int32_t *out, int32_t *sums,
                                                                     int64_t n) {
    __shared__ int lds[kScanThreads / 64 + 1];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int v[kScanItems];
    int s = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        v[i] = (base + i < n) ? in[base + i] : 0;
        s += v[i];
    }
    int total;
    int pre = block_exclusive_scan<kScanThreads>(s, &total, lds);
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        if (base + i < n) out[base + i] = pre;
        pre += v[i];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

static __global__ __launch_bounds__(1024) void k_scan_sums(int32_t *sums, int nb) {
    __shared__ int lds[1024 / 64 + 1];
    int carry = 0;
    for (int c = 0; c < nb; c += 1024) {      // nb is a kernel argument: the same trip count in every thread
        const int i = c + threadIdx.x;
        const int v = i < nb ? sums[i] : 0;
        int total;
        const int pre = block_exclusive_scan<1024>(v, &total, lds);
        if (i < nb) sums[i] = pre + carry;
        carry += total;
    }
}

__device__ __forceinline__ void scan_add_back(int32_t *out, int add, int64_t n) {
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i)
        if (base + i < n) out[base + i] += add;
}

// Add-back with the scan of the block totals folded in: block b sums the totals of the blocks before it (a few
// hundred at most at the plan's sizes) instead of waiting for a separate single-block scan launch.
static __global__ __launch_bounds__(kScanThreads) void k_scan_add_prefix(int32_t *out, const int32_t *sums, int64_t n) {
    __shared__ int lds[kScanThreads / 64 + 1];
    scan_add_back(out, block_base<kScanThreads>(sums, 1, lds), n);
}

// Add-back behind k_scan_sums: sums holds the scanned totals.
static __global__ __launch_bounds__(kScanThreads) void k_scan_add(int32_t *out, const int32_t *sums, int64_t n) {
    scan_add_back(out, sums[blockIdx.x], n);
}

// elements of the workspace `sums` of a scan of n
__host__ __device__ inline int64_t scan_ws_elems(int64_t n) { return (n + kScanTile - 1) / kScanTile + 1; }

// out may alias in.
static int exclusive_scan(const int32_t *in, int32_t *out, int64_t n, int32_t *sums, hipStream_t st) {
    if (n <= 0) return LGCN_OK;
    const int64_t nb = (n + kScanTile - 1) / kScanTile;
    if (nb > 0x7fffffff) return LGCN_ESHAPE;
    hipLaunchKernelGGL(k_scan_blocks, dim3((unsigned)nb), dim3(kScanThreads), 0, st, in, out, sums, n);
    if (nb > 4096) {          // very long inputs: scan the block totals in their own launch
        hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, st, sums, (int)nb);
        hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(kScanThreads), 0, st, out, sums, n);
    } else if (nb > 1) {
        hipLaunchKernelGGL(k_scan_add_prefix, dim3((unsigned)nb), dim3(kScanThreads), 0, st, out, sums, n);
    }
    return launch_status();
}

// ------------------------------------------------------------------ host side
// an offset table of n segments: starts at 0, ascends, ends at total
inline int check_table(const int32_t *tab, int64_t n, int64_t total) {
    if (tab[0] != 0) return LGCN_EINVAL;
    for (int64_t i = 0; i < n; ++i)
        if (tab[i + 1] < tab[i]) return LGCN_EINVAL;
    return tab[n] == total ? LGCN_OK : LGCN_EINVAL;
}

static inline bool misaligned(const void *q, unsigned mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }

}  // namespace lgcn
