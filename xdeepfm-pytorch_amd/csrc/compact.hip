// K11: positive-row compaction of the SFG branch (deepctr/xdeepfm_pro/basemodel_sfg.py:420-476 feeds the decoder only the
// rows whose label is 1; the reference does it with a mask over the full batch, xdfm_amd/pro.py's dynamic route with
// torch.nonzero + index_select, whose output shape reaches the host).  Here every output has the capacity of the batch
// and the number of selected rows stays on the device, so the step's shapes depend on the batch shape only.
//
//   compact_scan_kernel    ONE workgroup of 16 waves walks the labels in tiles of 1024 rows: ballot + popcount of the lower
//                          lanes inside a wave, the 16 wave totals through LDS, a running base across tiles -- the slot of
//                          a selected row is the number of selected rows before it, i.e. the order torch.nonzero gives.  No
//                          atomics.  Leaves pos[b] (slot or -1), n_rows and inv_n.  With a second label vector count_y
//                          (the labels of the GLOBAL batch under row-parallel training, xdfm_compact_rows_fwd_n) the same
//                          workgroup counts its positives the same way and inv_n comes from that count: the slots stay local,
//                          the normaliser is the global one (deepctr/xdeepfm_pro/sfg_decoder.py:262-268).
//   compact_move_kernel    a bandwidth kernel over (row, 16-byte chunk): source row b goes to slot pos[b]; slot j >= n_rows
//                          is zero-filled.  The two sets of destinations are disjoint, every element of every output is
//                          written exactly once with a plain store.  The first B threads also move the per-row scalars
//                          (valid, label, the F ids as int64).
//   compact_bwd_kernel     d(dnn_in)[b] = d(d_rows)[pos[b]] or zeros: the full [B, W] gradient, plain stores.
// Rows are moved as float4 when W, both row pitches and both base addresses allow it, element by element otherwise (the
// decoder input of Criteo is 26 * D + 13 floats wide: odd).
#include "xdfm_internal.h"

#define CP_SCAN_WAVES 16
#define CP_SCAN_THREADS (64 * CP_SCAN_WAVES)
#define CP_MAX_COUNT (65536L * 1024L)                               // labels of a global batch: 65536 rows on up to 1024 ranks

__global__ __launch_bounds__(CP_SCAN_THREADS) void compact_scan_kernel(const float* __restrict__ y, int B, int positive_only,
                                                                       const float* __restrict__ count_y, long n_count,
                                                                       int* __restrict__ pos, int* __restrict__ n_rows,
                                                                       float* __restrict__ inv_n) {
    __shared__ int wave_total[CP_SCAN_WAVES];
    __shared__ int wave_count[CP_SCAN_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int base = 0;                                                  // selected rows in the tiles before this one (uniform)
    for (int t0 = 0; t0 < B; t0 += CP_SCAN_THREADS) {
        const int i = t0 + (int)threadIdx.x;
        const bool sel = i < B && (!positive_only || y[i] == 1.f);
        const unsigned long long m = __ballot(sel);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[w] = __popcll(m);
        __syncthreads();
        int wave_base = 0, tile_total = 0;
#pragma unroll
        for (int k = 0; k < CP_SCAN_WAVES; ++k) {
            const int c = wave_total[k];
            wave_base += k < w ? c : 0;
            tile_total += c;
        }
        if (i < B) pos[i] = sel ? base + wave_base + before : -1;
        base += tile_total;
        __syncthreads();                                           // wave_total is rewritten by the next tile
    }
    if (count_y == nullptr) {                                      // uniform: the step's own labels define the normaliser
        if (threadIdx.x == 0) {
            *n_rows = base;
            *inv_n = positive_only ? 1.f / ((float)base + 1e-8f) : 1.f / (float)B;
        }
        return;
    }
    int mine = 0;                                                  // positives of count_y this wave has seen (uniform in a wave)
    if (positive_only)
        for (long t0 = 0; t0 < n_count; t0 += CP_SCAN_THREADS) {   // the trip count is uniform: every lane joins every ballot
            const long i = t0 + (long)threadIdx.x;
            mine += __popcll(__ballot(i < n_count && count_y[i] == 1.f));
        }
    if (lane == 0) wave_count[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int k = 0; k < CP_SCAN_WAVES; ++k) total += wave_count[k];
        *n_rows = base;
        *inv_n = positive_only ? 1.f / ((float)total + 1e-8f) : 1.f / (float)n_count;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void compact_move_kernel(const float* __restrict__ X, long ldx, int xcols,
                                                           const float* __restrict__ dnn_in, long ldd,
                                                           const float* __restrict__ y, int B, int W,
                                                           const int* __restrict__ cols, int F, const int* __restrict__ pos,
                                                           const int* __restrict__ n_rows, float* __restrict__ valid,
                                                           float* __restrict__ d_rows, float* __restrict__ labels,
                                                           long* __restrict__ targets) {
    const int n = *n_rows;
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    for (long b = tid; b < B; b += nth) {                          // the per-row scalars
        const int p = pos[b];
        valid[b] = b < n ? 1.f : 0.f;
        if (p >= 0) labels[p] = y[b];
        if (b >= n) labels[b] = 0.f;
        for (int f = 0; f < F; ++f) {
            const int c = cols[f];
            if (p >= 0) targets[(long)f * B + p] = c >= 0 && c < xcols ? (long)X[b * ldx + c] : 0L;
            if (b >= n) targets[(long)f * B + b] = 0L;
        }
    }
    constexpr int E = VEC ? 4 : 1;
    const int wu = W / E;                                          // units per row (VEC: W % 4 == 0)
    const long units = (long)B * wu;
    for (long u = tid; u < units; u += nth) {
        const long b = u / wu;
        const int c = (int)(u - b * wu) * E;
        const int p = pos[b];
        if constexpr (VEC) {
            if (p >= 0) *reinterpret_cast<float4*>(d_rows + (long)p * W + c) = *reinterpret_cast<const float4*>(dnn_in + b * ldd + c);
            if (b >= n) *reinterpret_cast<float4*>(d_rows + b * W + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            if (p >= 0) d_rows[(long)p * W + c] = dnn_in[b * ldd + c];
            if (b >= n) d_rows[b * W + c] = 0.f;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void compact_bwd_kernel(const float* __restrict__ g, long ldg, const int* __restrict__ pos, int B, int W,
                                                          float* __restrict__ d_dnn) {
    constexpr int E = VEC ? 4 : 1;
    const int wu = W / E;
    const long units = (long)B * wu, nth = (long)gridDim.x * 256;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += nth) {
        const long b = u / wu;
        const int c = (int)(u - b * wu) * E;
        const int p = pos[b];
        if constexpr (VEC) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p >= 0) v = *reinterpret_cast<const float4*>(g + (long)p * ldg + c);
            *reinterpret_cast<float4*>(d_dnn + b * W + c) = v;
        } else {
            d_dnn[b * W + c] = p >= 0 ? g[(long)p * ldg + c] : 0.f;
        }
    }
}

static inline bool cp_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int cp_grid(long units) {                            // at most 2048 workgroups, grid-stride beyond
    long g = (units + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

static int cp_rows_fwd(const char* who, const float* X, long ldx, int xcols, const float* dnn_in, long ldd, const float* y, long B, int W,
                       const int* cols, int F, int positive_only, const float* count_y, long n_count, int* pos, int* n_rows,
                       float* inv_n, float* valid, float* d_rows, float* labels, long* targets, void* stream) {
    XDFM_REQUIRE(X && dnn_in && y && pos && n_rows && inv_n && valid && d_rows && labels, "%s: null pointer", who);
    XDFM_REQUIRE(F >= 0 && (F == 0 || (cols && targets)), "%s: F=%d needs cols and targets", who, F);
    XDFM_REQUIRE(B >= 1 && B <= 65536 && W >= 1 && xcols >= 1 && ldx >= xcols && ldd >= W,
                 "%s: bad shape B=%ld W=%d xcols=%d ldx=%ld ldd=%ld (1 <= B <= 65536)", who, B, W, xcols, ldx, ldd);
    XDFM_REQUIRE(!count_y || (n_count >= 1 && n_count <= CP_MAX_COUNT), "%s: n_count=%ld labels to count (1 <= n_count <= %ld)", who,
                 n_count, (long)CP_MAX_COUNT);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CP_SCAN_THREADS), 0, st, y, (int)B, positive_only ? 1 : 0, count_y,
                       count_y ? n_count : 0L, pos, n_rows, inv_n);
    const bool vec = W % 4 == 0 && ldd % 4 == 0 && cp_aligned16(dnn_in) && cp_aligned16(d_rows);
    if (vec)
        hipLaunchKernelGGL((compact_move_kernel<true>), dim3(cp_grid(B * (W / 4))), dim3(256), 0, st, X, ldx, xcols, dnn_in, ldd, y, (int)B, W,
                           cols, F, pos, n_rows, valid, d_rows, labels, targets);
    else
        hipLaunchKernelGGL((compact_move_kernel<false>), dim3(cp_grid(B * (long)W)), dim3(256), 0, st, X, ldx, xcols, dnn_in, ldd, y, (int)B, W,
                           cols, F, pos, n_rows, valid, d_rows, labels, targets);
    return xdfm_check_launch(who);
}

extern "C" {

int xdfm_compact_rows_fwd(const float* X, long ldx, int xcols, const float* dnn_in, long ldd, const float* y, long B, int W,
                          const int* cols, int F, int positive_only, int* pos, int* n_rows, float* inv_n, float* valid,
                          float* d_rows, float* labels, long* targets, void* stream) {
    return cp_rows_fwd("compact_rows_fwd", X, ldx, xcols, dnn_in, ldd, y, B, W, cols, F, positive_only, nullptr, 0, pos, n_rows, inv_n,
                       valid, d_rows, labels, targets, stream);
}

int xdfm_compact_rows_fwd_n(const float* X, long ldx, int xcols, const float* dnn_in, long ldd, const float* y, long B, int W,
                            const int* cols, int F, int positive_only, const float* count_y, long n_count, int* pos, int* n_rows,
                            float* inv_n, float* valid, float* d_rows, float* labels, long* targets, void* stream) {
    return cp_rows_fwd("compact_rows_fwd_n", X, ldx, xcols, dnn_in, ldd, y, B, W, cols, F, positive_only, count_y, n_count, pos, n_rows,
                       inv_n, valid, d_rows, labels, targets, stream);
}

int xdfm_compact_rows_bwd(const float* g, long ldg, const int* pos, long B, int W, float* d_dnn, void* stream) {
    XDFM_REQUIRE(g && pos && d_dnn, "compact_rows_bwd: null pointer");
    XDFM_REQUIRE(B >= 1 && B <= 65536 && W >= 1 && ldg >= W, "compact_rows_bwd: bad shape B=%ld W=%d ldg=%ld", B, W, ldg);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = W % 4 == 0 && ldg % 4 == 0 && cp_aligned16(g) && cp_aligned16(d_dnn);
    if (vec)
        hipLaunchKernelGGL((compact_bwd_kernel<true>), dim3(cp_grid(B * (W / 4))), dim3(256), 0, st, g, ldg, pos, (int)B, W, d_dnn);
    else
        hipLaunchKernelGGL((compact_bwd_kernel<false>), dim3(cp_grid(B * (long)W)), dim3(256), 0, st, g, ldg, pos, (int)B, W, d_dnn);
    return xdfm_check_launch("compact_rows_bwd");
}

}  // extern "C"
