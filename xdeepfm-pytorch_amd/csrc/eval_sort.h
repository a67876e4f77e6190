// What K14s (eval_metrics.hip) and K14w (eval_metrics_w.hip) share: the tile geometry, the order-preserving key of a score,
// the workgroup sums / scans in integers, the histogram and scan launches of a radix pass (they see keys alone, so a payload
// that travels with the keys does not concern them) and the binary search of the bounds.  The code is K14s's, moved here
// unchanged; the kernels are `static` because two translation units include this header.
#ifndef XDFM_EVAL_SORT_H
#define XDFM_EVAL_SORT_H
#include "xdfm_internal.h"

#define ES_THREADS 256
#define ES_ROWS 16                          // keys (rows) per thread and tile
#define ES_TILE (ES_THREADS * ES_ROWS)      // 4096: the tile of every kernel here
#define ES_WAVES (ES_THREADS / 64)
#define ES_WAVE_KEYS (ES_TILE / ES_WAVES)   // 1024 consecutive keys per wave in the scatter
#define ES_MAX_N (1L << 27)                 // n_pos * n_neg <= 2^52: C / 2 is exact in a double
static_assert(ES_THREADS == 256, "one thread per digit in the scan and the scatter");
static_assert(ES_WAVE_KEYS == 64 * ES_ROWS, "a wave takes its keys in ES_ROWS rounds of 64");

typedef unsigned long long u64;
typedef unsigned int u32;

__device__ __forceinline__ u32 es_key(float p) {
    u32 u = __float_as_uint(p);
    if (p == 0.0f) u = 0u;                                  // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ u64 es_block_sum_u64(u64 v, u64* __restrict__ sm) {     // sm: ES_WAVES cells; ends with the cells free
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < ES_WAVES; ++w) s += sm[w];
    return s;
}

// exclusive scan of one u32 per thread over the 256 threads; sm: ES_THREADS cells.  Returns the prefix; *total the sum.
__device__ __forceinline__ u32 es_block_exscan_u32(u32 v, u32* __restrict__ sm, u32* total) {
    const int tid = threadIdx.x;
    __syncthreads();
    sm[tid] = v;
    __syncthreads();
    u32 incl = v;
    for (int o = 1; o < ES_THREADS; o <<= 1) {
        const u32 add = tid >= o ? sm[tid - o] : 0u;
        __syncthreads();
        incl += add;
        sm[tid] = incl;
        __syncthreads();
    }
    *total = sm[ES_THREADS - 1];
    return incl - v;
}

// ---------------------------------------------------------------------------------------------- radix pass: histogram
// hist[d * nb + b] = #{keys of tile b whose digit is d}; every cell of [256][nb] is written
static __global__ __launch_bounds__(ES_THREADS) void eval_sort_hist_kernel(const u32* __restrict__ src, int N, int shift,
                                                                           u32* __restrict__ hist) {
    __shared__ u32 h[256];
    const int tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ES_ROWS; ++r) {
        const int i = blockIdx.x * ES_TILE + r * ES_THREADS + tid;
        if (i < N) atomicAdd(&h[(src[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)tid * gridDim.x + blockIdx.x] = h[tid];
}

// ---------------------------------------------------------------------------------------------- radix pass: scan
// workgroup d: hist[d][0 .. nb) becomes its exclusive prefix sum, tot[d] the digit's total.  A thread takes a run of
// ceil(nb / 256) consecutive tiles; the runs' sums are scanned across the workgroup.
static __global__ __launch_bounds__(ES_THREADS) void eval_sort_scan_kernel(u32* __restrict__ hist, int nb, u32* __restrict__ tot) {
    __shared__ u32 sm[ES_THREADS];
    const int tid = threadIdx.x;
    u32* row = hist + (size_t)blockIdx.x * nb;
    const int run = (nb + ES_THREADS - 1) / ES_THREADS;
    const int lo = tid * run < nb ? tid * run : nb, hi = lo + run < nb ? lo + run : nb;
    u32 s = 0;
    for (int k = lo; k < hi; ++k) s += row[k];
    u32 total;
    u32 pre = es_block_exscan_u32(s, sm, &total);
    for (int k = lo; k < hi; ++k) {
        const u32 c = row[k];
        row[k] = pre;
        pre += c;
    }
    if (tid == 0) tot[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------- bounds
// first index of [lo, hi) whose key is >= k (strict == false) or > k (strict == true)
__device__ __forceinline__ int es_bound(const u32* __restrict__ a, int lo, int hi, u32 k, bool strict) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const u32 v = a[mid];
        if (strict ? v <= k : v < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

#endif  // XDFM_EVAL_SORT_H
