// K14w: sample-weighted logloss, AUC, mse, accuracy of one (labels, predictions, weights) triple of any row count up to 2^27
// -- the `weighted_metrics` of `evaluate` and of the per-batch log of `fit`.  K14s (eval_metrics.hip) with a weight per row.
//
// replaces the host path of the weighted metrics: a device-to-host copy of all predictions, their widening to float64 and
// xdfm_amd/metrics.py's weighted_* numpy functions on one CPU thread (a merge sort, a cumsum, two searchsorted).
//
// Definitions (xdfm_amd/metrics.py, weighted_*): positives are y > 0.5, pc = clamp(double(p), 2^-52, 1 - 2^-52), a row counts
// with wd = double(w) when w > 0 and not at all otherwise (selected, not multiplied: a NaN score on such a row is harmless; a
// negative or NaN weight, which the host never passes, is a zero too).  W = sum wd, Wpos / Wneg the same over the positives /
// the others, each its own sum.
//   logloss  -(sum wd (y log pc + (1 - y) log(1 - pc))) / W          mse  (sum wd (y - p)^2) / W
//   accuracy (sum wd [(p > 0.5 ? 1 : 0) == y]) / W
//   auc      (C * 0.5) / (Wpos * Wneg),  C = sum over positives i of wd_i (cum[lb_i] + cum[ub_i]): cum the exclusive prefix sum
//            of the non-positives' weights in ascending, stable score order, lb / ub the lower / upper bound of p_i among those
//            scores.  NaN when a row with w > 0 has a NaN score, when Wpos * Wneg == 0; W == 0 gives NaN in every slot.
//
//   pointwise  K14s's tiles and row order.  Per tile: sum wd ll, sum wd se, sum wd match, W, Wpos, Wneg (doubles) and the u64
//              count of NaN scores with w > 0; keys as K14s (positives 0xFFFFFFFF, the others es_key(p)) and the payload w.
//   sort       K14s's stable LSD radix sort; the histogram and the scan are K14s's own kernels (keys alone), the scatter
//              carries the payload: the rank found by the ballots addresses both stores.  Stability fixes the order in which
//              equal scores enter the prefix sum, and with it the bits.
//   cum        n_neg is where the 0xFFFFFFFF run begins (a binary search per workgroup).  v_k = sorted weight k for k < n_neg
//              (and w > 0), else 0.  Three launches: (1) a tile's total in the tiled order below; (2) one workgroup turns the
//              tiles' totals into exclusive prefixes, a thread taking a run of ceil(T / 256) consecutive tiles as
//              eval_sort_scan_kernel does; (3) cum[k] for every k in [0, N]: a tile goes through its 16 rows of 256
//              consecutive cells, each row scanned inside its 4 waves (Hillis-Steele over the lanes), the waves' totals
//              added in order, the rows' totals carried in order, the tile's prefix added last.  cum[N] (hence cum[n_neg]) is
//              written.  A cell passes through at most 37 + 2 ceil(T / 256) additions.
//   bounds     every positive with w > 0 takes lb / ub as in K14s and adds fma(wd, cum[lb] + cum[ub], c); one double per tile.
//   finish     thread t adds the tiles t, t + 256, ... in index order, xdfm_block_sum_f64 adds the 256 threads; then the four
//              formulas above.
// ORDER OF THE SUMS (pointwise, bounds, finish): K14s's -- a thread adds its 16 rows t, t + 256, ... of a 4096-row tile in
// index order, xdfm_block_sum_f64 adds the workgroup (xor tree in a wave, the 4 waves in order), the finish as above.
//
// UNIT WEIGHTS reproduce xdfm_eval_metrics bit for bit in all four slots: a row's logloss term is formed as K14s's compiled
// code forms it (fma(y, log pc, (1 - y) log(1 - pc))) and enters by fma(wd, term, sum), which for wd == 1 is K14s's addition;
// the squared error enters by fma(wd d, d, sum), for wd == 1 K14s's fma(d, d, sum); W == N, Wpos == n_pos, Wneg == n_neg,
// sum wd match == #match and cum[k] == k are exact integers, C is the integer K14s counts, and the divisions are the same.
//
// No float atomics (integer LDS atomics in the histogram), no memset, no allocation, no synchronisation, no host read: every
// cell a kernel reads was written by an earlier launch of the same call, so the workspace may hold anything.  Weights never
// form an address.  The launches and their shapes are a function of (N, which): 2 without the AUC, 18 with it.
#include "eval_sort.h"

// ---------------------------------------------------------------------------------------------- pointwise sums, keys, payload
// part: [6][nt] doubles, rows sum wd ll | sum wd se | sum wd match | W | Wpos | Wneg
__global__ __launch_bounds__(ES_THREADS) void evalw_pointwise_kernel(const float* __restrict__ y, const float* __restrict__ p,
                                                                     const float* __restrict__ w, int N, int which,
                                                                     double* __restrict__ part, u64* __restrict__ nan_part,
                                                                     u32* __restrict__ keys, float* __restrict__ pay) {
    __shared__ double red[6][ES_WAVES];
    __shared__ u64 red_u[ES_WAVES];
    const int tid = threadIdx.x;
    double ll = 0.0, se = 0.0, wm = 0.0, W = 0.0, Wp = 0.0, Wn = 0.0;
    u32 nnan = 0;
#pragma unroll
    for (int r = 0; r < ES_ROWS; ++r) {
        const int i = blockIdx.x * ES_TILE + r * ES_THREADS + tid;
        if (i < N) {
            const float yi = y[i], pi = p[i], wi = w[i];
            const bool is_pos = yi > 0.5f, live = wi > 0.0f;
            if (live) {
                const double yd = (double)yi, pd = (double)pi, wd = (double)wi;
                if (which & XDFM_METRIC_LOGLOSS) {
                    const double eps = 2.220446049250313e-16;            // 2^-52
                    const double pc = pd < eps ? eps : (pd > 1.0 - eps ? 1.0 - eps : pd);       // a NaN stays a NaN
                    const double term = __builtin_fma(yd, log(pc), (1.0 - yd) * log(1.0 - pc));
                    ll = __builtin_fma(wd, term, ll);
                }
                if (which & XDFM_METRIC_MSE) { const double d = yd - pd; se = __builtin_fma(wd * d, d, se); }
                wm += ((pi > 0.5f ? 1.f : 0.f) == yi) ? wd : 0.0;
                W += wd;
                Wp += is_pos ? wd : 0.0;
                Wn += is_pos ? 0.0 : wd;
                nnan += (pi != pi) ? 1u : 0u;
            }
            if (which & XDFM_METRIC_AUC) {
                keys[i] = is_pos ? 0xFFFFFFFFu : es_key(pi);
                pay[i] = wi;
            }
        }
    }
    const size_t nt = gridDim.x;
    if (which & XDFM_METRIC_LOGLOSS) {
        const double s = xdfm_block_sum_f64(ll, red[0]);
        if (tid == 0) part[0 * nt + blockIdx.x] = s;
    }
    if (which & XDFM_METRIC_MSE) {
        const double s = xdfm_block_sum_f64(se, red[1]);
        if (tid == 0) part[1 * nt + blockIdx.x] = s;
    }
    const double s2 = xdfm_block_sum_f64(wm, red[2]), s3 = xdfm_block_sum_f64(W, red[3]);
    const double s4 = xdfm_block_sum_f64(Wp, red[4]), s5 = xdfm_block_sum_f64(Wn, red[5]);
    const u64 nn = es_block_sum_u64(nnan, red_u);
    if (tid == 0) {
        part[2 * nt + blockIdx.x] = s2;
        part[3 * nt + blockIdx.x] = s3;
        part[4 * nt + blockIdx.x] = s4;
        part[5 * nt + blockIdx.x] = s5;
        nan_part[blockIdx.x] = nn;
    }
}

// ---------------------------------------------------------------------------------------------- radix pass: scatter with payload
// eval_sort_scatter_kernel (eval_metrics.hip) whose keys take their weight along: same ranks, two stores per key
__global__ __launch_bounds__(ES_THREADS) void evalw_sort_scatter_kernel(const u32* __restrict__ src, const float* __restrict__ src_pay,
                                                                        u32* __restrict__ dst, float* __restrict__ dst_pay, int N,
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
    float pay[ES_ROWS];
#pragma unroll
    for (int r = 0; r < ES_ROWS; ++r) {
        const int i = blockIdx.x * ES_TILE + w * ES_WAVE_KEYS + r * 64 + lane;
        const bool in = i < N;
        key[r] = in ? src[i] : 0u;
        pay[r] = in ? src_pay[i] : 0.f;
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
            if (at < (u32)N) {                  // always true for a consistent histogram; never write outside
                dst[at] = key[r];
                dst_pay[at] = pay[r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- cum: prefix sums of the weights
__device__ __forceinline__ int evalw_n_neg(const u32* __restrict__ sorted, int N, int* __restrict__ cell) {
    if (threadIdx.x == 0) *cell = es_bound(sorted, 0, N, 0xFFFFFFFFu, false);      // where the positives' keys begin
    __syncthreads();
    return *cell;
}

__device__ __forceinline__ double evalw_cell(const float* __restrict__ pay, int k, int n_neg) {
    if (k >= n_neg) return 0.0;
    const float v = pay[k];
    return v > 0.0f ? (double)v : 0.0;
}

// (1) ttot[b] = sum of tile b's cells, in the tiled order
__global__ __launch_bounds__(ES_THREADS) void evalw_cum_total_kernel(const u32* __restrict__ sorted, const float* __restrict__ pay,
                                                                     int N, double* __restrict__ ttot) {
    __shared__ int n_neg_s;
    __shared__ double red[ES_WAVES];
    const int n_neg = evalw_n_neg(sorted, N, &n_neg_s);
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < ES_ROWS; ++r) s += evalw_cell(pay, blockIdx.x * ES_TILE + r * ES_THREADS + (int)threadIdx.x, n_neg);
    s = xdfm_block_sum_f64(s, red);
    if (threadIdx.x == 0) ttot[blockIdx.x] = s;
}

// (2) one workgroup: ttot[0 .. nt) becomes its exclusive prefix sum.  A thread takes a run of ceil(nt / 256) consecutive tiles
// and adds them in order; the runs' sums are scanned across the workgroup (Hillis-Steele, the prefix read from the left
// neighbour: no subtraction); the thread walks its run again.
__global__ __launch_bounds__(ES_THREADS) void evalw_cum_scan_kernel(double* __restrict__ ttot, int nt) {
    __shared__ double sm[ES_THREADS];
    const int tid = threadIdx.x;
    const int run = (nt + ES_THREADS - 1) / ES_THREADS;
    const int lo = tid * run < nt ? tid * run : nt, hi = lo + run < nt ? lo + run : nt;
    double s = 0.0;
    for (int k = lo; k < hi; ++k) s += ttot[k];
    sm[tid] = s;
    __syncthreads();
    double incl = s;
    for (int o = 1; o < ES_THREADS; o <<= 1) {
        const double add = tid >= o ? sm[tid - o] : 0.0;
        __syncthreads();
        incl = add + incl;
        sm[tid] = incl;
        __syncthreads();
    }
    double pre = tid ? sm[tid - 1] : 0.0;
    for (int k = lo; k < hi; ++k) {
        const double c = ttot[k];
        ttot[k] = pre;
        pre += c;
    }
}

// (3) cum[k] = ttot[tile of k] + (carry of the tile's earlier rows + (the row's earlier waves + the wave's earlier lanes))
__global__ __launch_bounds__(ES_THREADS) void evalw_cum_store_kernel(const u32* __restrict__ sorted, const float* __restrict__ pay,
                                                                     int N, const double* __restrict__ ttot,
                                                                     double* __restrict__ cum) {
    __shared__ int n_neg_s;
    __shared__ double wtot[2][ES_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_neg = evalw_n_neg(sorted, N, &n_neg_s);
    const double base = ttot[blockIdx.x];
    double carry = 0.0;
#pragma unroll 1
    for (int r = 0; r < ES_ROWS; ++r) {
        const int k = blockIdx.x * ES_TILE + r * ES_THREADS + tid;
        const double v = evalw_cell(pay, k, n_neg);
        double incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double up = __shfl_up(incl, o);
            if (lane >= o) incl = up + incl;
        }
        const double left = __shfl_up(incl, 1);
        const double excl = lane ? left : 0.0;
        if (lane == 63) wtot[r & 1][wv] = incl;
        __syncthreads();                         // the other buffer is free again: its readers passed the previous barrier
        double wpre = 0.0, row = 0.0;
#pragma unroll
        for (int q = 0; q < ES_WAVES; ++q) {
            if (q == wv) wpre = row;
            row += wtot[r & 1][q];
        }
        const double here = carry + (wpre + excl);
        if (k < N) {
            cum[k] = base + here;
            if (k == N - 1) cum[N] = base + (here + v);
        }
        carry += row;
    }
}

// ---------------------------------------------------------------------------------------------- bounds of the positives
__global__ __launch_bounds__(ES_THREADS) void evalw_bounds_kernel(const float* __restrict__ y, const float* __restrict__ p,
                                                                  const float* __restrict__ w, int N, const u32* __restrict__ sorted,
                                                                  const double* __restrict__ cum, double* __restrict__ pair_part) {
    __shared__ int n_neg_s;
    __shared__ double red[ES_WAVES];
    const int tid = threadIdx.x;
    const int n_neg = evalw_n_neg(sorted, N, &n_neg_s);
    double c = 0.0;
#pragma unroll 1
    for (int r = 0; r < ES_ROWS; ++r) {
        const int i = blockIdx.x * ES_TILE + r * ES_THREADS + tid;
        if (i < N && y[i] > 0.5f) {
            const float wi = w[i];
            if (wi > 0.0f) {
                const u32 k = es_key(p[i]);
                const int lb = es_bound(sorted, 0, n_neg, k, false);
                int ub = lb;
                if (lb < n_neg && sorted[lb] == k) ub = es_bound(sorted, lb + 1, n_neg, k, true);
                c = __builtin_fma((double)wi, cum[lb] + cum[ub], c);
            }
        }
    }
    const double total = xdfm_block_sum_f64(c, red);
    if (tid == 0) pair_part[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(ES_THREADS) void evalw_finish_kernel(const double* __restrict__ part, const u64* __restrict__ nan_part,
                                                                  const double* __restrict__ pair_part, int nt, int which,
                                                                  double* __restrict__ out) {
    __shared__ double red[7][ES_WAVES];
    __shared__ u64 red_u[ES_WAVES];
    const int tid = threadIdx.x;
    double ll = 0.0, se = 0.0, wm = 0.0, W = 0.0, Wp = 0.0, Wn = 0.0, pairs = 0.0;
    u64 nnan = 0;
    for (int k = tid; k < nt; k += ES_THREADS) {
        if (which & XDFM_METRIC_LOGLOSS) ll += part[0 * (size_t)nt + k];
        if (which & XDFM_METRIC_MSE) se += part[1 * (size_t)nt + k];
        wm += part[2 * (size_t)nt + k];
        W += part[3 * (size_t)nt + k];
        Wp += part[4 * (size_t)nt + k];
        Wn += part[5 * (size_t)nt + k];
        nnan += nan_part[k];
        if (which & XDFM_METRIC_AUC) pairs += pair_part[k];
    }
    ll = xdfm_block_sum_f64(ll, red[0]);
    se = xdfm_block_sum_f64(se, red[1]);
    wm = xdfm_block_sum_f64(wm, red[2]);
    W = xdfm_block_sum_f64(W, red[3]);
    Wp = xdfm_block_sum_f64(Wp, red[4]);
    Wn = xdfm_block_sum_f64(Wn, red[5]);
    pairs = xdfm_block_sum_f64(pairs, red[6]);
    nnan = es_block_sum_u64(nnan, red_u);
    if (tid != 0) return;
    if (which & XDFM_METRIC_LOGLOSS) out[0] = -(ll / W);
    if (which & XDFM_METRIC_AUC) out[1] = nnan ? __builtin_nan("") : (pairs * 0.5) / (Wp * Wn);
    if (which & XDFM_METRIC_MSE) out[2] = se / W;
    if (which & XDFM_METRIC_ACC) out[3] = wm / W;
}

static inline bool ew_ok(long N, int which) { return N >= 1 && N <= ES_MAX_N && which >= 1 && which <= 15; }

// workspace, in 8-byte cells: part[6 nt] | nan_part[nt] | and with the AUC: pair_part[nt] | ttot[nt] | cum[N + 1] | keys A [N] u32 |
// keys B [N] u32 | payload A [N] f32 | payload B [N] f32 | hist [256][nt] u32 | tot [256] u32
struct EwLayout { size_t nt, pair, ttot, cum, keys_a, keys_b, pay_a, pay_b, hist, tot, cells; };
static inline EwLayout ew_layout(long N, int which) {
    EwLayout l;
    l.nt = (size_t)((N + ES_TILE - 1) / ES_TILE);
    l.pair = 7 * l.nt;
    l.cells = l.pair;
    l.ttot = l.cum = l.keys_a = l.keys_b = l.pay_a = l.pay_b = l.hist = l.tot = 0;
    if (which & XDFM_METRIC_AUC) {
        const size_t half_cells = ((size_t)N + 1) / 2;
        l.ttot = l.pair + l.nt;
        l.cum = l.ttot + l.nt;
        l.keys_a = l.cum + (size_t)N + 1;
        l.keys_b = l.keys_a + half_cells;
        l.pay_a = l.keys_b + half_cells;
        l.pay_b = l.pay_a + half_cells;
        l.hist = l.pay_b + half_cells;
        l.tot = l.hist + 128 * l.nt;
        l.cells = l.tot + 128;
    }
    return l;
}

extern "C" {

size_t xdfm_eval_metrics_w_ws_bytes(long N, int which) {
    if (!ew_ok(N, which)) return 0;
    return 8 * ew_layout(N, which).cells;
}

int xdfm_eval_metrics_w(const float* y, const float* p, const float* w, long N, int which, void* ws, double* out4, void* stream) {
    XDFM_REQUIRE(y && p && w && ws && out4, "eval_metrics_w: null pointer (y=%p p=%p w=%p ws=%p out4=%p)", (const void*)y,
                 (const void*)p, (const void*)w, ws, (void*)out4);
    XDFM_REQUIRE(N >= 1 && N <= ES_MAX_N, "eval_metrics_w: N=%ld outside [1, %ld]", N, ES_MAX_N);
    XDFM_REQUIRE(which >= 1 && which <= 15, "eval_metrics_w: which=%d (bits 1 logloss, 2 auc, 4 mse, 8 accuracy)", which);
    XDFM_REQUIRE((((size_t)ws) & 7) == 0, "eval_metrics_w: ws=%p is not 8-byte aligned", ws);
    XDFM_REQUIRE((((size_t)out4) & 7) == 0, "eval_metrics_w: out4=%p is not 8-byte aligned", (void*)out4);
    hipStream_t st = (hipStream_t)stream;
    const EwLayout l = ew_layout(N, which);
    const int nt = (int)l.nt, n = (int)N;
    u64* cells = (u64*)ws;
    double* part = (double*)cells;
    u64* nan_part = cells + 6 * l.nt;
    double* pair_part = (double*)(cells + l.pair);
    double* ttot = (double*)(cells + l.ttot);
    double* cum = (double*)(cells + l.cum);
    u32* keys_a = (u32*)(cells + l.keys_a);
    u32* keys_b = (u32*)(cells + l.keys_b);
    float* pay_a = (float*)(cells + l.pay_a);
    float* pay_b = (float*)(cells + l.pay_b);
    u32* hist = (u32*)(cells + l.hist);
    u32* tot = (u32*)(cells + l.tot);
    hipLaunchKernelGGL(evalw_pointwise_kernel, dim3(nt), dim3(ES_THREADS), 0, st, y, p, w, n, which, part, nan_part, keys_a, pay_a);
    if (int rc = xdfm_check_launch("eval_metrics_w pointwise")) return rc;
    if (which & XDFM_METRIC_AUC) {
        u32 *src = keys_a, *dst = keys_b;
        float *src_pay = pay_a, *dst_pay = pay_b;
        for (int shift = 0; shift < 32; shift += 8) {
            hipLaunchKernelGGL(eval_sort_hist_kernel, dim3(nt), dim3(ES_THREADS), 0, st, (const u32*)src, n, shift, hist);
            if (int rc = xdfm_check_launch("eval_metrics_w histogram")) return rc;
            hipLaunchKernelGGL(eval_sort_scan_kernel, dim3(256), dim3(ES_THREADS), 0, st, hist, nt, tot);
            if (int rc = xdfm_check_launch("eval_metrics_w scan")) return rc;
            hipLaunchKernelGGL(evalw_sort_scatter_kernel, dim3(nt), dim3(ES_THREADS), 0, st, (const u32*)src, (const float*)src_pay, dst,
                               dst_pay, n, shift, (const u32*)hist, (const u32*)tot);
            if (int rc = xdfm_check_launch("eval_metrics_w scatter")) return rc;
            u32* t = src; src = dst; dst = t;
            float* tp = src_pay; src_pay = dst_pay; dst_pay = tp;
        }
        // four passes: the sorted keys are back in keys_a, their weights in pay_a
        hipLaunchKernelGGL(evalw_cum_total_kernel, dim3(nt), dim3(ES_THREADS), 0, st, (const u32*)src, (const float*)src_pay, n, ttot);
        if (int rc = xdfm_check_launch("eval_metrics_w cum total")) return rc;
        hipLaunchKernelGGL(evalw_cum_scan_kernel, dim3(1), dim3(ES_THREADS), 0, st, ttot, nt);
        if (int rc = xdfm_check_launch("eval_metrics_w cum scan")) return rc;
        hipLaunchKernelGGL(evalw_cum_store_kernel, dim3(nt), dim3(ES_THREADS), 0, st, (const u32*)src, (const float*)src_pay, n,
                           (const double*)ttot, cum);
        if (int rc = xdfm_check_launch("eval_metrics_w cum store")) return rc;
        hipLaunchKernelGGL(evalw_bounds_kernel, dim3(nt), dim3(ES_THREADS), 0, st, y, p, w, n, (const u32*)src, (const double*)cum,
                           pair_part);
        if (int rc = xdfm_check_launch("eval_metrics_w bounds")) return rc;
    }
    hipLaunchKernelGGL(evalw_finish_kernel, dim3(1), dim3(ES_THREADS), 0, st, (const double*)part, (const u64*)nan_part,
                       (const double*)pair_part, nt, which, out4);
    return xdfm_check_launch("eval_metrics_w finish");
}

}  // extern "C"
