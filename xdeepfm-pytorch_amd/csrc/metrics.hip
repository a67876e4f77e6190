// K14: the per-batch training metrics -- logloss, AUC, mse, accuracy -- of one (labels, predictions) pair.
//
// replaces the float64 ATen compositions of xdfm_amd/metrics.py (*_device) that `fit(verbose > 0)` runs behind every train
// step: a sort, two searchsorted, about a dozen elementwise / 0-d kernels and two reductions for the AUC, another dozen
// launches for the logloss -- and, for the accuracy, a device-to-host copy of both vectors with its sync.  Two launches
// here, whatever the metrics asked for: a main grid and a one-block finish.  No float atomics; the same bits on every run.
//
//   AUC       exact pair counting, no sort:  C = sum over (i positive, j not positive) of 2 [p_i > p_j] + [p_i == p_j]
//             as an unsigned 64-bit integer (fp32 compares: the same outcome as on the float64 images), then
//             AUC = (C * 0.5) / (double(n_pos) * double(n_neg)).  C / 2 is the Mann-Whitney statistic with mid-ranks, a
//             half-integer below 2^53, and the division is IEEE: the bits of metrics.roc_auc_score, ties included.
//             n_pos == 0 or n_neg == 0: 0 / 0 = NaN.  Any NaN in p: NaN.  positive: y > 0.5 (a NaN label is not).
//   logloss   -(1 / B) sum_b (y log(pc) + (1 - y) log(1 - pc)),  pc = clamp(double(p), eps, 1 - eps), eps = 2^-52; y enters
//             as a double factor (soft labels)
//   mse       (1 / B) sum_b (double(y) - double(p))^2
//   accuracy  #{b: (p_b > 0.5 ? 1 : 0) == y_b} / B: an integer count, one IEEE division
//
// Main grid (MT_I-row tiles x MT_J-column tiles; one column tile without the AUC).  A workgroup compacts the scores of its
// row tile's positives and of its column tile's non-positives into LDS (ballot + popcount, the slot base from one integer
// LDS atomic per wave: the order of the list varies, the integer count over it does not), a thread then takes one positive
// against the whole list -- work ~ n_pos * n_neg, not B^2 -- and the workgroup writes ONE u64 partial.  The workgroups of
// the first column tile also form the pointwise sums of their MT_I rows in double: a thread adds its rows in index order,
// xdfm_block_sum_f64 the threads; one partial per row tile for logloss and for mse, one packed integer for the counts.
// Finish: one workgroup adds the row tiles' partials (thread t holds tile t, then xdfm_block_sum_f64) and the pair
// partials (integers), and rounds once more per metric: the division by B, the negation being exact.
#include "xdfm_internal.h"

#define MT_THREADS 256
#define MT_I 512            // rows per row tile (2 per thread); 65536 / MT_I row tiles at most, one finish thread each
#define MT_J 512            // rows per column tile
#define MT_MAX_B 65536
#define MT_CNT_BITS 21      // three counts of at most 65536 packed into one u64: matches | positives << 21 | NaN scores << 42
static_assert(MT_MAX_B / MT_I <= MT_THREADS, "one finish thread per row tile");
static_assert(MT_I % MT_THREADS == 0 && MT_J % MT_THREADS == 0 && MT_J % 4 == 0, "tile shapes");

typedef unsigned long long u64;

// appends v to list[] for the threads with `take`; every thread of the workgroup calls it (whole waves)
__device__ __forceinline__ void mt_append(bool take, float v, float* __restrict__ list, int* __restrict__ n) {
    const u64 mask = __ballot(take);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && mask) base = atomicAdd(n, __popcll(mask));
    base = __shfl(base, 0);
    if (take) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = v;
}

__device__ __forceinline__ u64 mt_block_sum_u64(u64 v, u64* __restrict__ sm) {      // sm: MT_THREADS cells
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = MT_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    return sm[0];
}

__global__ __launch_bounds__(MT_THREADS) void batch_metrics_kernel(const float* __restrict__ y, const float* __restrict__ p, int B,
                                                                   int which, double* __restrict__ ll_part,
                                                                   double* __restrict__ mse_part, u64* __restrict__ cnt_part,
                                                                   u64* __restrict__ pair_part) {
    __shared__ __attribute__((aligned(16))) float pos_s[MT_I];
    __shared__ __attribute__((aligned(16))) float neg_s[MT_J];
    __shared__ int n_s[2];
    __shared__ double red[2][MT_THREADS / 64];
    __shared__ u64 red_u[MT_THREADS];
    const int tid = threadIdx.x;
    const bool auc = (which & XDFM_METRIC_AUC) != 0;
    const bool pointwise = blockIdx.y == 0;
    if (tid < 2) n_s[tid] = 0;
    __syncthreads();
    double ll = 0.0, se = 0.0;
    unsigned match = 0, npos = 0, nnan = 0;
#pragma unroll
    for (int r = 0; r < MT_I / MT_THREADS; ++r) {
        const int i = blockIdx.x * MT_I + r * MT_THREADS + tid;
        const bool in = i < B;
        const float yi = in ? y[i] : 0.f, pi = in ? p[i] : 0.f;
        const bool is_pos = in && yi > 0.5f;
        if (auc) mt_append(is_pos, pi, pos_s, &n_s[0]);
        if (pointwise && in) {
            const double yd = (double)yi, pd = (double)pi;
            if (which & XDFM_METRIC_LOGLOSS) {
                const double eps = 2.220446049250313e-16;            // 2^-52
                const double pc = pd < eps ? eps : (pd > 1.0 - eps ? 1.0 - eps : pd);       // a NaN stays a NaN
                ll += yd * log(pc) + (1.0 - yd) * log(1.0 - pc);
            }
            if (which & XDFM_METRIC_MSE) { const double d = yd - pd; se += d * d; }
            match += ((pi > 0.5f ? 1.f : 0.f) == yi) ? 1u : 0u;
            npos += is_pos ? 1u : 0u;
            nnan += (pi != pi) ? 1u : 0u;
        }
    }
    if (pointwise) {
        if (which & XDFM_METRIC_LOGLOSS) {
            const double s = xdfm_block_sum_f64(ll, red[0]);
            if (tid == 0) ll_part[blockIdx.x] = s;
        }
        if (which & XDFM_METRIC_MSE) {
            const double s = xdfm_block_sum_f64(se, red[1]);
            if (tid == 0) mse_part[blockIdx.x] = s;
        }
        const u64 c = mt_block_sum_u64((u64)match | ((u64)npos << MT_CNT_BITS) | ((u64)nnan << (2 * MT_CNT_BITS)), red_u);
        if (tid == 0) cnt_part[blockIdx.x] = c;
    }
    if (!auc) return;
#pragma unroll
    for (int r = 0; r < MT_J / MT_THREADS; ++r) {
        const int j = blockIdx.y * MT_J + r * MT_THREADS + tid;
        const bool in = j < B;
        const float yj = in ? y[j] : 0.f, pj = in ? p[j] : 0.f;
        mt_append(in && !(yj > 0.5f), pj, neg_s, &n_s[1]);
    }
    __syncthreads();
    const int np = n_s[0], nn = n_s[1], nn4 = (nn + 3) & ~3;
    if (tid < 4 && nn + tid < nn4) neg_s[nn + tid] = __builtin_nanf("");     // a NaN compares false both ways: the tail counts nothing
    __syncthreads();
    unsigned c = 0;                                          // at most 2 positives x 2 * MT_J per thread
    for (int k = tid; k < np; k += MT_THREADS) {
        const float pi = pos_s[k];
        for (int q = 0; q < nn4; q += 4) {
            const float4 s = *reinterpret_cast<const float4*>(neg_s + q);       // one address for the whole wave: a broadcast
            c += (unsigned)(pi > s.x) + (unsigned)(pi >= s.x);
            c += (unsigned)(pi > s.y) + (unsigned)(pi >= s.y);
            c += (unsigned)(pi > s.z) + (unsigned)(pi >= s.z);
            c += (unsigned)(pi > s.w) + (unsigned)(pi >= s.w);
        }
    }
    __syncthreads();                                         // red_u: the counts' sum above is read by then
    const u64 total = mt_block_sum_u64((u64)c, red_u);
    if (tid == 0) pair_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(MT_THREADS) void batch_metrics_finish_kernel(const double* __restrict__ ll_part,
                                                                          const double* __restrict__ mse_part,
                                                                          const u64* __restrict__ cnt_part,
                                                                          const u64* __restrict__ pair_part, int nbx, int npair, int B,
                                                                          int which, double* __restrict__ out) {
    __shared__ double red[2][MT_THREADS / 64];
    __shared__ u64 red_u[MT_THREADS];
    const int tid = threadIdx.x;
    double ll = 0.0, se = 0.0;
    if (which & XDFM_METRIC_LOGLOSS) ll = xdfm_block_sum_f64(tid < nbx ? ll_part[tid] : 0.0, red[0]);
    if (which & XDFM_METRIC_MSE) se = xdfm_block_sum_f64(tid < nbx ? mse_part[tid] : 0.0, red[1]);
    const u64 cnt = mt_block_sum_u64(tid < nbx ? cnt_part[tid] : 0ull, red_u);
    u64 pairs = 0;
    if (which & XDFM_METRIC_AUC) {
        for (int k = tid; k < npair; k += MT_THREADS) pairs += pair_part[k];
        __syncthreads();
        pairs = mt_block_sum_u64(pairs, red_u);
    }
    if (tid != 0) return;
    const u64 field = (1ull << MT_CNT_BITS) - 1ull;
    const u64 match = cnt & field, npos = (cnt >> MT_CNT_BITS) & field, nnan = cnt >> (2 * MT_CNT_BITS);
    if (which & XDFM_METRIC_LOGLOSS) out[0] = -(ll / (double)B);
    if (which & XDFM_METRIC_AUC)
        out[1] = nnan ? __builtin_nan("") : ((double)pairs * 0.5) / ((double)npos * (double)((u64)B - npos));
    if (which & XDFM_METRIC_MSE) out[2] = se / (double)B;
    if (which & XDFM_METRIC_ACC) out[3] = (double)match / (double)B;
}

static inline bool mt_ok(int B, int which) { return B >= 1 && B <= MT_MAX_B && which >= 1 && which <= 15; }

extern "C" {

size_t xdfm_batch_metrics_ws_bytes(int B, int which) {
    if (!mt_ok(B, which)) return 0;
    const size_t nbx = (size_t)ceil_div(B, MT_I), nby = (size_t)ceil_div(B, MT_J);
    return 8 * (3 * nbx + ((which & XDFM_METRIC_AUC) ? nbx * nby : 0));
}

int xdfm_batch_metrics(const float* y, const float* p, int B, int which, void* ws, double* out4, void* stream) {
    XDFM_REQUIRE(y && p && ws && out4, "batch_metrics: null pointer (y=%p p=%p ws=%p out4=%p)", (const void*)y, (const void*)p, ws,
                 (void*)out4);
    XDFM_REQUIRE(B >= 1 && B <= MT_MAX_B, "batch_metrics: B=%d outside [1, %d]", B, MT_MAX_B);
    XDFM_REQUIRE(which >= 1 && which <= 15, "batch_metrics: which=%d (bits 1 logloss, 2 auc, 4 mse, 8 accuracy)", which);
    XDFM_REQUIRE((((size_t)ws) & 7) == 0, "batch_metrics: ws=%p is not 8-byte aligned", ws);
    XDFM_REQUIRE((((size_t)out4) & 7) == 0, "batch_metrics: out4=%p is not 8-byte aligned", (void*)out4);
    hipStream_t st = (hipStream_t)stream;
    const int nbx = ceil_div(B, MT_I), nby = (which & XDFM_METRIC_AUC) ? ceil_div(B, MT_J) : 1;
    double* ll_part = (double*)ws;
    double* mse_part = ll_part + nbx;
    u64* cnt_part = (u64*)(mse_part + nbx);
    u64* pair_part = cnt_part + nbx;                 // nbx * nby cells, only with the AUC
    hipLaunchKernelGGL(batch_metrics_kernel, dim3(nbx, nby), dim3(MT_THREADS), 0, st, y, p, B, which, ll_part, mse_part, cnt_part,
                       pair_part);
    if (int rc = xdfm_check_launch("batch_metrics")) return rc;
    hipLaunchKernelGGL(batch_metrics_finish_kernel, dim3(1), dim3(MT_THREADS), 0, st, ll_part, mse_part, cnt_part, pair_part, nbx,
                       nbx * nby, B, which, out4);
    return xdfm_check_launch("batch_metrics finish");
}

}  // extern "C"
