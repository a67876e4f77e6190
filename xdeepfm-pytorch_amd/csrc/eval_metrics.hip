// K14s: logloss, AUC, mse, accuracy of one (labels, predictions) pair of ANY row count up to 2^27 -- the metrics of
// `evaluate` (validation at the end of an epoch, the trainer's --mode eval), where K14's quadratic pair count (metrics.hip,
// at most 65536 rows) does not reach.
//
// replaces the host path of BaseModel.evaluate: a device-to-host copy of all predictions, their widening to float64, and
// numpy's log_loss / roc_auc_score / mean_squared_error / accuracy on one CPU thread (a merge sort of N float64 values, a
// `repeat`, several passes over N-long arrays).
//
// The four values and `which` are K14's (include/xdfm.h): positives are y > 0.5, pc = clamp(double(p), 2^-52, 1 - 2^-52).
//
//   AUC   exact, sort-based, in integers.  C = sum over positives i of (2 #{j not positive: p_j < p_i} + #{j: p_j == p_i}),
//         auc = (C * 0.5) / (double(n_pos) * double(n_neg)): K14's finish formula, the bits of metrics.roc_auc_score.
//           keys    a score becomes an order-preserving u32 (sign flip; -0.0 takes the key of +0.0, as the float64 images the
//                   host compares are equal); a positive row's key is 0xFFFFFFFF, which no finite score has: the
//                   non-positives sort to the front of an array that keeps its length N.
//           sort    the keys alone, LSD radix, four 8-bit passes, three launches each over tiles of ES_TILE keys:
//                   histogram (one count per tile and digit, stored digit-major), scan (workgroup d turns digit d's counts
//                   into exclusive prefixes over the tiles and leaves the digit's total), scatter (a workgroup scans the 256
//                   totals itself, ranks its keys -- wave w owns keys [w * 1024, (w + 1) * 1024) of the tile and goes
//                   through them 64 at a time in index order, equal digits found by 8 ballots, so the scatter is stable --
//                   and writes every key to its place).
//           count   n_neg is where the 0xFFFFFFFF run begins in the sorted array (a binary search per workgroup: no host
//                   read, no separate launch).  Every positive row takes a lower and an upper bound of its key in
//                   [0, n_neg): lower + upper = 2 #less + #equal.  One u64 partial per workgroup, added by the finish.
//   logloss, mse     K14's arithmetic per row in double.  ORDER OF THE SUMS: a thread adds its 16 rows t, t + 256, ... of a
//         4096-row tile in index order, xdfm_block_sum_f64 adds the workgroup's 256 threads (xor tree in a wave, the 4 waves
//         in order): one partial per tile.  The finish (one workgroup) gives thread t the tiles t, t + 256, ... in index
//         order and runs xdfm_block_sum_f64 again; then one division by N (the negation is exact).
//   accuracy, n_pos, NaN scores: u64 counts per tile, added by the finish.
//
// No float atomics (integer LDS atomics in the histogram), no memset, no allocation, no synchronisation, no host read: every
// cell a kernel reads was written by an earlier launch of the same call, so the workspace may hold anything.  The launches
// and their shapes are a function of (N, which): 2 without the AUC, 15 with it.
#include "eval_sort.h"         // tile geometry, es_key, workgroup sums and scans, histogram and scan kernels, es_bound

// ---------------------------------------------------------------------------------------------- pointwise sums, counts, keys
__global__ __launch_bounds__(ES_THREADS) void eval_pointwise_kernel(const float* __restrict__ y, const float* __restrict__ p, int N,
                                                                    int which, double* __restrict__ ll_part,
                                                                    double* __restrict__ mse_part, u64* __restrict__ cnt_part,
                                                                    u32* __restrict__ keys) {
    __shared__ double red[2][ES_WAVES];
    __shared__ u64 red_u[ES_WAVES];
    const int tid = threadIdx.x;
    double ll = 0.0, se = 0.0;
    u32 match = 0, npos = 0, nnan = 0;
#pragma unroll
    for (int r = 0; r < ES_ROWS; ++r) {
        const int i = blockIdx.x * ES_TILE + r * ES_THREADS + tid;
        if (i < N) {
            const float yi = y[i], pi = p[i];
            const bool is_pos = yi > 0.5f;
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
            if (which & XDFM_METRIC_AUC) keys[i] = is_pos ? 0xFFFFFFFFu : es_key(pi);
        }
    }
    if (which & XDFM_METRIC_LOGLOSS) {
        const double s = xdfm_block_sum_f64(ll, red[0]);
        if (tid == 0) ll_part[blockIdx.x] = s;
    }
    if (which & XDFM_METRIC_MSE) {
        const double s = xdfm_block_sum_f64(se, red[1]);
        if (tid == 0) mse_part[blockIdx.x] = s;
    }
    const u64 m = es_block_sum_u64(match, red_u), np = es_block_sum_u64(npos, red_u), nn = es_block_sum_u64(nnan, red_u);
    if (tid == 0) {
        cnt_part[3 * (size_t)blockIdx.x + 0] = m;
        cnt_part[3 * (size_t)blockIdx.x + 1] = np;
        cnt_part[3 * (size_t)blockIdx.x + 2] = nn;
    }
}

// ---------------------------------------------------------------------------------------------- radix pass: scatter
__global__ __launch_bounds__(ES_THREADS) void eval_sort_scatter_kernel(const u32* __restrict__ src, u32* __restrict__ dst, int N,
                                                                       int shift, const u32* __restrict__ hist,
                                                                       const u32* __restrict__ tot) {
    __shared__ u32 sm[ES_THREADS];
    __shared__ u32 cnt[ES_WAVES][256];          // a wave's running count per digit, then its first destination per digit
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int k = 0; k < ES_WAVES; ++k) cnt[k][tid] = 0u;
    u32 unused;
    const u32 digit_base = es_block_exscan_u32(tot[tid], sm, &unused) + hist[(size_t)tid * gridDim.x + blockIdx.x];
    __syncthreads();
    volatile u32* my = cnt[w];
    const u64 below = (1ull << lane) - 1ull;
    u32 key[ES_ROWS], rank[ES_ROWS];
#pragma unroll
    for (int r = 0; r < ES_ROWS; ++r) {
        const int i = blockIdx.x * ES_TILE + w * ES_WAVE_KEYS + r * 64 + lane;
        const bool in = i < N;
        key[r] = in ? src[i] : 0u;
        const u32 d = (key[r] >> shift) & 255u;
        u64 peers = __ballot(in);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (d >> bit) & 1u;
            const u64 m = __ballot(set);
            peers &= set ? m : ~m;
        }
        // peers: the lanes of this round with my digit (myself included, if in range)
        rank[r] = my[d] + (u32)__popcll(peers & below);
        __builtin_amdgcn_wave_barrier();
        if (in && (peers & below) == 0ull) my[d] = my[d] + (u32)__popcll(peers);        // the lowest peer
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        u32 at = digit_base;                    // thread = digit: the waves' shares of the digit in index order
#pragma unroll
        for (int k = 0; k < ES_WAVES; ++k) {
            const u32 c = cnt[k][tid];
            cnt[k][tid] = at;
            at += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ES_ROWS; ++r) {
        const int i = blockIdx.x * ES_TILE + w * ES_WAVE_KEYS + r * 64 + lane;
        if (i < N) {
            const u32 at = cnt[w][(key[r] >> shift) & 255u] + rank[r];
            if (at < (u32)N) dst[at] = key[r];          // always true for a consistent histogram; never write outside
        }
    }
}

// ---------------------------------------------------------------------------------------------- bounds of the positives
__global__ __launch_bounds__(ES_THREADS) void eval_bounds_kernel(const float* __restrict__ y, const float* __restrict__ p, int N,
                                                                 const u32* __restrict__ sorted, u64* __restrict__ pair_part) {
    __shared__ int n_neg_s;
    __shared__ u64 red_u[ES_WAVES];
    const int tid = threadIdx.x;
    if (tid == 0) n_neg_s = es_bound(sorted, 0, N, 0xFFFFFFFFu, false);      // where the positives' keys begin
    __syncthreads();
    const int n_neg = n_neg_s;
    u64 c = 0;
#pragma unroll 1
    for (int r = 0; r < ES_ROWS; ++r) {
        const int i = blockIdx.x * ES_TILE + r * ES_THREADS + tid;
        if (i < N && y[i] > 0.5f) {
            const u32 k = es_key(p[i]);
            const int lb = es_bound(sorted, 0, n_neg, k, false);
            int ub = lb;
            if (lb < n_neg && sorted[lb] == k) ub = es_bound(sorted, lb + 1, n_neg, k, true);
            c += (u64)lb + (u64)ub;
        }
    }
    const u64 total = es_block_sum_u64(c, red_u);
    if (tid == 0) pair_part[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(ES_THREADS) void eval_finish_kernel(const double* __restrict__ ll_part, const double* __restrict__ mse_part,
                                                                 const u64* __restrict__ cnt_part, const u64* __restrict__ pair_part,
                                                                 int nt, int N, int which, double* __restrict__ out) {
    __shared__ double red[2][ES_WAVES];
    __shared__ u64 red_u[ES_WAVES];
    const int tid = threadIdx.x;
    double ll = 0.0, se = 0.0;
    u64 match = 0, npos = 0, nnan = 0, pairs = 0;
    for (int k = tid; k < nt; k += ES_THREADS) {
        if (which & XDFM_METRIC_LOGLOSS) ll += ll_part[k];
        if (which & XDFM_METRIC_MSE) se += mse_part[k];
        match += cnt_part[3 * (size_t)k + 0];
        npos += cnt_part[3 * (size_t)k + 1];
        nnan += cnt_part[3 * (size_t)k + 2];
        if (which & XDFM_METRIC_AUC) pairs += pair_part[k];
    }
    ll = xdfm_block_sum_f64(ll, red[0]);
    se = xdfm_block_sum_f64(se, red[1]);
    match = es_block_sum_u64(match, red_u);
    npos = es_block_sum_u64(npos, red_u);
    nnan = es_block_sum_u64(nnan, red_u);
    pairs = es_block_sum_u64(pairs, red_u);
    if (tid != 0) return;
    if (which & XDFM_METRIC_LOGLOSS) out[0] = -(ll / (double)N);
    if (which & XDFM_METRIC_AUC)
        out[1] = nnan ? __builtin_nan("") : ((double)pairs * 0.5) / ((double)npos * (double)((u64)N - npos));
    if (which & XDFM_METRIC_MSE) out[2] = se / (double)N;
    if (which & XDFM_METRIC_ACC) out[3] = (double)match / (double)N;
}

static inline bool es_ok(long N, int which) { return N >= 1 && N <= ES_MAX_N && which >= 1 && which <= 15; }

// workspace, in 8-byte cells: ll_part[nt] | mse_part[nt] | cnt_part[3 nt] | and with the AUC: pair_part[nt] | keys A [N] u32 |
// keys B [N] u32 | hist [256][nt] u32 | tot [256] u32
struct EsLayout { size_t nt, pair, keys_a, keys_b, hist, tot, cells; };
static inline EsLayout es_layout(long N, int which) {
    EsLayout l;
    l.nt = (size_t)((N + ES_TILE - 1) / ES_TILE);
    l.pair = 5 * l.nt;
    l.cells = l.pair;
    l.keys_a = l.keys_b = l.hist = l.tot = 0;
    if (which & XDFM_METRIC_AUC) {
        const size_t key_cells = ((size_t)N + 1) / 2;
        l.keys_a = l.pair + l.nt;
        l.keys_b = l.keys_a + key_cells;
        l.hist = l.keys_b + key_cells;
        l.tot = l.hist + 128 * l.nt;
        l.cells = l.tot + 128;
    }
    return l;
}

extern "C" {

size_t xdfm_eval_metrics_ws_bytes(long N, int which) {
    if (!es_ok(N, which)) return 0;
    return 8 * es_layout(N, which).cells;
}

int xdfm_eval_metrics(const float* y, const float* p, long N, int which, void* ws, double* out4, void* stream) {
    XDFM_REQUIRE(y && p && ws && out4, "eval_metrics: null pointer (y=%p p=%p ws=%p out4=%p)", (const void*)y, (const void*)p, ws,
                 (void*)out4);
    XDFM_REQUIRE(N >= 1 && N <= ES_MAX_N, "eval_metrics: N=%ld outside [1, %ld]", N, ES_MAX_N);
    XDFM_REQUIRE(which >= 1 && which <= 15, "eval_metrics: which=%d (bits 1 logloss, 2 auc, 4 mse, 8 accuracy)", which);
    XDFM_REQUIRE((((size_t)ws) & 7) == 0, "eval_metrics: ws=%p is not 8-byte aligned", ws);
    XDFM_REQUIRE((((size_t)out4) & 7) == 0, "eval_metrics: out4=%p is not 8-byte aligned", (void*)out4);
    hipStream_t st = (hipStream_t)stream;
    const EsLayout l = es_layout(N, which);
    const int nt = (int)l.nt, n = (int)N;
    u64* cells = (u64*)ws;
    double* ll_part = (double*)cells;
    double* mse_part = ll_part + l.nt;
    u64* cnt_part = cells + 2 * l.nt;
    u64* pair_part = cells + l.pair;
    u32* keys_a = (u32*)(cells + l.keys_a);
    u32* keys_b = (u32*)(cells + l.keys_b);
    u32* hist = (u32*)(cells + l.hist);
    u32* tot = (u32*)(cells + l.tot);
    hipLaunchKernelGGL(eval_pointwise_kernel, dim3(nt), dim3(ES_THREADS), 0, st, y, p, n, which, ll_part, mse_part, cnt_part, keys_a);
    if (int rc = xdfm_check_launch("eval_metrics pointwise")) return rc;
    if (which & XDFM_METRIC_AUC) {
        u32 *src = keys_a, *dst = keys_b;
        for (int shift = 0; shift < 32; shift += 8) {
            hipLaunchKernelGGL(eval_sort_hist_kernel, dim3(nt), dim3(ES_THREADS), 0, st, (const u32*)src, n, shift, hist);
            if (int rc = xdfm_check_launch("eval_metrics histogram")) return rc;
            hipLaunchKernelGGL(eval_sort_scan_kernel, dim3(256), dim3(ES_THREADS), 0, st, hist, nt, tot);
            if (int rc = xdfm_check_launch("eval_metrics scan")) return rc;
            hipLaunchKernelGGL(eval_sort_scatter_kernel, dim3(nt), dim3(ES_THREADS), 0, st, (const u32*)src, dst, n, shift,
                               (const u32*)hist, (const u32*)tot);
            if (int rc = xdfm_check_launch("eval_metrics scatter")) return rc;
            u32* t = src; src = dst; dst = t;
        }
        // four passes: the sorted keys are back in keys_a
        hipLaunchKernelGGL(eval_bounds_kernel, dim3(nt), dim3(ES_THREADS), 0, st, y, p, n, (const u32*)src, pair_part);
        if (int rc = xdfm_check_launch("eval_metrics bounds")) return rc;
    }
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(ES_THREADS), 0, st, (const double*)ll_part, (const double*)mse_part,
                       (const u64*)cnt_part, (const u64*)pair_part, nt, n, which, out4);
    return xdfm_check_launch("eval_metrics finish");
}

}  // extern "C"
