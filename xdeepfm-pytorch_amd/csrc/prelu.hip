// K13: elementwise PReLU with one scalar slope (nn.PReLU() of deepctr/layers/core.py:104-134 with activation='prelu').
//
// replaces: aten::_prelu_kernel and, backward, _prelu_kernel_backward + the ATen `sum` that reduces the slope's gradient
// (which zeroes a semaphore buffer with a memset: the captured train step holds no memset node).  It serves the layers the
// fused dense + PReLU kernels of dnn.hip do not take: widths that are no multiple of 32, a batch norm in between, the
// library GEMM route.
//
//   u [rows][ldu] fp32, alpha a DEVICE scalar (the optimizer moves it; a replayed graph reads the new value)
//   forward    y  = u > 0 ? u : alpha * u
//   backward   du = u > 0 ? g : alpha * g  (one rounding),   dalpha = sum over the cells with u <= 0 of g * u
//
// Geometry: that of bn.hip.  A block is 4 row groups x 64 columns over 64 rows: a wave reads 64 consecutive columns of one
// row (the row pitch is arbitrary, so nothing wider than a dword is aligned), 16 rows per thread issued together.
//
// dalpha.  Every block of the backward leaves one partial -- the products g * u and their sum in double: a wave tree, then the
// waves in index order -- in the workspace; a one-block second launch adds the partials in a fixed order, in double, and
// rounds once to fp32.  No atomics, no zeroed cells, the same bits on every run.
#include "xdfm_internal.h"

#define PR_ROWBLK 64
#define PR_COLBLK 64
#define PR_THREADS 256
#define PR_RPT (PR_ROWBLK / 4)          // rows per thread

__global__ __launch_bounds__(PR_THREADS) void prelu_fwd_kernel(const float* __restrict__ u, long ldu, long rows, int cols,
                                                               const float* __restrict__ alpha_p, float* __restrict__ y, long ldy) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * PR_COLBLK + lane;
    if (c >= cols) return;
    const float alpha = *alpha_p;
    const long r0 = (long)blockIdx.x * PR_ROWBLK + rg;
    float v[PR_RPT];
#pragma unroll
    for (int t = 0; t < PR_RPT; ++t) {                         // loaded unconditionally (clamped row)
        const long r = r0 + 4 * t < rows ? r0 + 4 * t : rows - 1;
        v[t] = u[r * ldu + c];
    }
#pragma unroll
    for (int t = 0; t < PR_RPT; ++t) {
        const long r = r0 + 4 * t;
        if (r < rows) y[r * ldy + c] = v[t] > 0.f ? v[t] : alpha * v[t];
    }
}

// du and / or the block's partial of dalpha (ws[blockIdx.y * gridDim.x + blockIdx.x]); either pointer may be NULL
__global__ __launch_bounds__(PR_THREADS) void prelu_bwd_kernel(const float* __restrict__ g, long ldg, const float* __restrict__ u, long ldu,
                                                               long rows, int cols, const float* __restrict__ alpha_p,
                                                               float* __restrict__ du, long lddu, double* __restrict__ ws) {
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * PR_COLBLK + lane;
    const long r0 = (long)blockIdx.x * PR_ROWBLK + rg;
    double da = 0.0;
    if (c < cols) {
        const float alpha = *alpha_p;
        float gv[PR_RPT], uv[PR_RPT];
#pragma unroll
        for (int t = 0; t < PR_RPT; ++t) {
            const long r = r0 + 4 * t < rows ? r0 + 4 * t : rows - 1;
            gv[t] = g[r * ldg + c];
            uv[t] = u[r * ldu + c];
        }
#pragma unroll
        for (int t = 0; t < PR_RPT; ++t) {
            const long r = r0 + 4 * t;
            if (r >= rows) continue;
            if (uv[t] <= 0.f) da = fma((double)gv[t], (double)uv[t], da);
            if (du) du[r * lddu + c] = uv[t] > 0.f ? gv[t] : alpha * gv[t];
        }
    }
    if (!ws) return;                                            // uniform
    const double s = xdfm_block_sum_f64(da, sm);
    if (threadIdx.x == 0) ws[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// thread t adds the partials t, t + 256, ... in index order, then xdfm_block_sum_f64; one rounding to fp32
__global__ __launch_bounds__(PR_THREADS) void prelu_dalpha_finish_kernel(const double* __restrict__ ws, long npart, float* __restrict__ dalpha) {
    __shared__ double sm[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < npart; i += PR_THREADS) s += ws[i];
    s = xdfm_block_sum_f64(s, sm);
    if (threadIdx.x == 0) *dalpha = (float)s;
}

static int pr_shape_check(const char* what, long rows, int cols) {
    XDFM_REQUIRE(rows >= 1, "%s: rows = %ld (at least 1)", what, rows);
    XDFM_REQUIRE(rows <= ((long)1 << 36), "%s: rows = %ld (at most 2^36)", what, rows);        // 2^30 row blocks on grid.x
    XDFM_REQUIRE(cols >= 1 && cols <= PR_COLBLK * 65535, "%s: cols = %d (1 .. %d)", what, cols, PR_COLBLK * 65535);
    return XDFM_OK;
}

extern "C" {

size_t xdfm_prelu_ws_elems(long rows, int cols) {
    if (rows < 1 || cols < 1) return 0;
    return (size_t)2 * (size_t)((rows + PR_ROWBLK - 1) / PR_ROWBLK) * (size_t)((cols + PR_COLBLK - 1) / PR_COLBLK);   // one double per block
}

int xdfm_prelu_fwd(const float* u, long ldu, long rows, int cols, const float* alpha, float* y, long ldy, void* stream) {
    XDFM_REQUIRE(u && alpha && y, "prelu_fwd: null pointer");
    if (int rc = pr_shape_check("prelu_fwd", rows, cols)) return rc;
    XDFM_REQUIRE(ldu >= cols, "prelu_fwd: ldu = %ld below cols = %d", ldu, cols);
    XDFM_REQUIRE(ldy >= cols, "prelu_fwd: ldy = %ld below cols = %d", ldy, cols);
    const dim3 grid((unsigned)((rows + PR_ROWBLK - 1) / PR_ROWBLK), (unsigned)ceil_div(cols, PR_COLBLK));
    hipLaunchKernelGGL(prelu_fwd_kernel, grid, dim3(PR_THREADS), 0, (hipStream_t)stream, u, ldu, rows, cols, alpha, y, ldy);
    return xdfm_check_launch("prelu_fwd");
}

int xdfm_prelu_bwd(const float* g, long ldg, const float* u, long ldu, long rows, int cols, const float* alpha, float* du, long lddu,
                   float* dalpha, float* ws, void* stream) {
    XDFM_REQUIRE(g && u && alpha, "prelu_bwd: null pointer");
    XDFM_REQUIRE(du || dalpha, "prelu_bwd: du and dalpha are both NULL");
    if (int rc = pr_shape_check("prelu_bwd", rows, cols)) return rc;
    XDFM_REQUIRE(ldg >= cols, "prelu_bwd: ldg = %ld below cols = %d", ldg, cols);
    XDFM_REQUIRE(ldu >= cols, "prelu_bwd: ldu = %ld below cols = %d", ldu, cols);
    XDFM_REQUIRE(!du || lddu >= cols, "prelu_bwd: lddu = %ld below cols = %d", lddu, cols);
    XDFM_REQUIRE(!dalpha || ws, "prelu_bwd: workspace is NULL (xdfm_prelu_ws_elems floats; dalpha needs it)");
    XDFM_REQUIRE(!dalpha || ((size_t)ws & 7) == 0, "prelu_bwd: workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((rows + PR_ROWBLK - 1) / PR_ROWBLK), (unsigned)ceil_div(cols, PR_COLBLK));
    double* part = dalpha ? (double*)ws : nullptr;
    hipLaunchKernelGGL(prelu_bwd_kernel, grid, dim3(PR_THREADS), 0, st, g, ldg, u, ldu, rows, cols, alpha, du, lddu, part);
    if (dalpha) {
        if (int rc = xdfm_check_launch("prelu_bwd")) return rc;
        hipLaunchKernelGGL(prelu_dalpha_finish_kernel, dim3(1), dim3(PR_THREADS), 0, st, (const double*)part, (long)grid.x * grid.y, dalpha);
    }
    return xdfm_check_launch("prelu_bwd");
}

}  // extern "C"
