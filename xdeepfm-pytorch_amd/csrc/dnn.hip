// Dense layers of the DNN tower on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulators; no operand splitting).
//
// replaces, per layer of deepctr/layers/core.py:120-134: the three hipBLASLt GEMMs (forward, input gradient, weight
// gradient), the threshold_backward pass that wrote gz = (y > 0) ? g : 0, and the bias gradient's column sum with its
// finish launch.  gz is never stored: the two backward kernels form it while they stage their operand.
// (The host side runs the two backward kernels; the forward kernel does not beat the library GEMM yet and is kept,
// tested, behind ops.DNN_NATIVE_FWD.)
//
// One kernel template serves the three products C[M x N] = sum_k A[k][m] * B[k][n]:
//   forward   y  = act(x W^T + b)   M = rows, N = out, K = in     A = x  (k contiguous)   B = W  (k contiguous)
//   dX        dx = gz W             M = rows, N = in,  K = out    A = gz (k contiguous)   B = W  (n contiguous)
//   dW, db    dW = gz^T x           M = out,  N = in,  K = rows   A = gz (m contiguous)   B = x  (n contiguous)
// A workgroup of 8 waves owns a 64 x 64 tile of C: waves w and w + 4 share the 32 x 32 accumulator tile w and take half
// of every stage's contraction each (two waves per SIMD: one's MFMAs run under the other's LDS traffic); at the end the
// upper four hand their accumulators over through LDS and the lower four add them, always in that order.  The
// contraction advances 32 at a time through a double-buffered LDS image; the next stage's operands are loaded into
// registers before the current stage's MFMAs and written to the other buffer after them (one barrier per stage).  Every
// global access is a dword: the first layer's rows are 429 floats, so x, dx and W rows are only 4-byte aligned.  Rows,
// columns and contraction indices past the end are staged as zeros (the odd K = 429 included) and never stored.
//
// LDS image of an operand tile T[k][m], 32 x 64: 8 planes p = 2 * (k / 8) + (k & 1), each [m][j = (k / 2) & 3] plus 8
// floats of padding.  Lane (c = lane & 31, s = lane >> 5) of a wave reads ONE float4 per 8 contraction indices: its
// operand of the k-steps j = 0 .. 3, where MFMA step (kq, j) covers k = 8 kq + 2 j + s.  Both operands use the same
// map.  The padding puts the dword writes of the k-contiguous loader (32 lanes along k for each of two m) on 64
// different banks.
//
// dW splits the contraction over the rows across blockIdx.z; every split leaves a slab and, for the bias gradient, the
// column sums of its gz rows.  A second launch adds them over a fixed pairwise tree: no atomics, no zeroed cells, same bits
// every run.
#include "xdfm_internal.h"

#define DN_T 64                    // tile edge (rows and columns of C per workgroup)
#define DN_K 32                    // contraction indices per LDS stage
#define DN_NW 8                    // waves per workgroup
#define DN_E 4                     // elements of an operand tile per thread: DN_T * DN_K / (64 * DN_NW)
#define DN_PLANE (DN_T * 4 + 8)    // floats per plane (8 of padding)
#define DN_TILE (8 * DN_PLANE)     // floats per operand tile
#define DN_SPLIT_ROWS 256          // rows of the contraction per dW split
#define DN_MAX_SPLIT 32
#define DN_MAX_DIM (1 << 20)       // in, out

struct DnArgs {
    const float* A; const float* Ay; long lda, lday;     // Ay: the layer's output for the ReLU mask (MASK instances)
    const float* B; long ldb;
    float* C; long ldc, cslab;                           // split z writes C + z * cslab
    const float* bias; int relu;                         // forward epilogue
    float* dbpart;                                       // dW: split z leaves its column sums of gz at dbpart + z * M
    long M, N, K, kper;                                  // kper: contraction indices per split (a multiple of DN_K)
};

__device__ __forceinline__ int dn_lds(int p, int m) { return p * DN_PLANE + (m << 2); }

// One thread's share of a 32 x 64 operand tile T[k][m]: 4 elements, loaded ahead and written to LDS a stage later.
// Every load is unconditional -- an index past the end is clamped to the last valid one and the value dropped at the
// write (hipcc puts a load behind a condition into a branch of its own and waits for it there).
// KC (k contiguous in memory, src[m * ld + k]): lanes run along k, element e is row (t >> 5) + 16 e.
// otherwise (m contiguous, src[k * ld + m]):    lanes run along m, wave q stages plane q.
template <bool KC, bool MASK>
struct DnStage {
    float v[DN_E], y[DN_E];
    long off[DN_E], offy[DN_E];    // KC: row offsets of the (clamped) rows; otherwise [0]: the (clamped) column
    unsigned fixed, ok;            // bit e: element e's row / column exists; ... and its k does, in the staged step
    __device__ __forceinline__ void init(long ld, long ldy, long m0, long mdim) {
        const int t = threadIdx.x;
        fixed = 0;
        if (KC) {
#pragma unroll
            for (int e = 0; e < DN_E; ++e) {
                const long m = m0 + (t >> 5) + 2 * DN_NW * e;
                if (m < mdim) fixed |= 1u << e;
                const long mc = m < mdim ? m : mdim - 1;
                off[e] = mc * ld;
                offy[e] = mc * ldy;
            }
        } else {
            const long m = m0 + (t & 63);
            if (m < mdim) fixed = (1u << DN_E) - 1;
            off[0] = offy[0] = m < mdim ? m : mdim - 1;
        }
    }
    __device__ __forceinline__ void load(const float* __restrict__ src, const float* __restrict__ ysrc, long ld, long ldy,
                                         long k0, long kend) {
        const int t = threadIdx.x;
        if (KC) {
            const long k = k0 + (t & 31);
            const long kc = k < kend ? k : kend - 1;
            ok = k < kend ? fixed : 0u;
#pragma unroll
            for (int e = 0; e < DN_E; ++e) {
                v[e] = src[off[e] + kc];
                if (MASK) y[e] = ysrc[offy[e] + kc];
            }
        } else {
            const int q = t >> 6;
            const long kb = k0 + 8 * (q >> 1) + (q & 1);          // element e: k = kb + 2 e
            if (k0 + DN_K <= kend) {                              // uniform: all but a ragged last stage
                ok = fixed;
                const float* pv = src + kb * ld + off[0];
                const float* py = MASK ? ysrc + kb * ldy + off[0] : nullptr;
#pragma unroll
                for (int e = 0; e < DN_E; ++e) {
                    v[e] = pv[2 * e * ld];
                    if (MASK) y[e] = py[2 * e * ldy];
                }
            } else {
                ok = 0;
#pragma unroll
                for (int e = 0; e < DN_E; ++e) {
                    const long k = kb + 2 * e;
                    const long kc = k < kend ? k : kend - 1;
                    if (k < kend) ok |= 1u << e;
                    v[e] = src[kc * ld + off[0]];
                    if (MASK) y[e] = ysrc[kc * ldy + off[0]];
                }
                ok &= fixed;
            }
        }
    }
    // returns the sum of the staged values in element order (the bias gradient's share of this thread)
    __device__ __forceinline__ float store(float* __restrict__ tile) {
        const int t = threadIdx.x;
#pragma unroll
        for (int e = 0; e < DN_E; ++e) {
            const bool live = (ok >> e & 1u) && (!MASK || y[e] > 0.f);
            v[e] = live ? v[e] : 0.f;
        }
        if (KC) {
            const int k = t & 31, p = (k >> 3) * 2 + (k & 1);
#pragma unroll
            for (int e = 0; e < DN_E; ++e) tile[dn_lds(p, (t >> 5) + 2 * DN_NW * e) + ((k >> 1) & 3)] = v[e];
        } else {
            f32x4 q = {v[0], v[1], v[2], v[3]};
            *(f32x4*)(tile + dn_lds(t >> 6, t & 63)) = q;
        }
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < DN_E; ++e) s += v[e];
        return s;
    }
};

enum { DN_EPI_FWD = 0, DN_EPI_PLAIN = 1, DN_EPI_SLAB = 2 };

template <bool AKC, bool BKC, bool MASK, int EPI>
__global__ __launch_bounds__(DN_NW * 64) void dense_mfma_kernel(DnArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[4 * DN_TILE];      // [buffer][A, B]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, c = lane & 31, s = lane >> 5;
    const int wt = w & 3, kh = w >> 2;
    const int wm = (wt & 1) * 32, wn = (wt >> 1) * 32;
    const long m0 = (long)blockIdx.x * DN_T, n0 = (long)blockIdx.y * DN_T;
    const long kbeg = (long)blockIdx.z * a.kper;
    const long kend = kbeg + a.kper < a.K ? kbeg + a.kper : a.K;
    const int steps = (int)((kend - kbeg + DN_K - 1) / DN_K);

    DnStage<AKC, MASK> sa;
    DnStage<BKC, false> sb;
    sa.init(a.lda, a.lday, m0, a.M);
    sb.init(a.ldb, 0, n0, a.N);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bsum = 0.f;

    sa.load(a.A, a.Ay, a.lda, a.lday, kbeg, kend);
    sb.load(a.B, nullptr, a.ldb, 0, kbeg, kend);
    bsum += sa.store(lds);
    sb.store(lds + DN_TILE);
    __syncthreads();
    for (int it = 0; it < steps; ++it) {
        const float* As = lds + (it & 1) * 2 * DN_TILE;
        const float* Bs = As + DN_TILE;
        const bool more = it + 1 < steps;             // uniform over the workgroup
        if (more) {
            const long k0 = kbeg + (long)(it + 1) * DN_K;
            sa.load(a.A, a.Ay, a.lda, a.lday, k0, kend);
            sb.load(a.B, nullptr, a.ldb, 0, k0, kend);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int p = (2 * kh + u) * 2 + s;
            const f32x4 af = *(const f32x4*)(As + dn_lds(p, wm + c));
            const f32x4 bf = *(const f32x4*)(Bs + dn_lds(p, wn + c));
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf[j], acc, 0, 0, 0);
        }
        if (more) {
            float* nxt = lds + ((it + 1) & 1) * 2 * DN_TILE;
            bsum += sa.store(nxt);
            sb.store(nxt + DN_TILE);
        }
        __syncthreads();
    }
    // the last barrier of the loop is behind every read of the image: the upper waves' accumulators go through it
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) lds[(wt * 16 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += lds[(wt * 16 + r) * 64 + lane];
        float* C = a.C + (long)blockIdx.z * a.cslab;
        const long col = n0 + wn + c;
        float bv = 0.f;
        if (EPI == DN_EPI_FWD && a.bias && col < a.N) bv = a.bias[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = m0 + wm + frag_row(r, s);
            if (row >= a.M || col >= a.N) continue;
            float v = acc[r];
            if (EPI == DN_EPI_FWD) {
                v += bv;
                if (a.relu) v = v < 0.f ? 0.f : v;
            }
            C[row * a.ldc + col] = v;
        }
    }
    if (EPI == DN_EPI_SLAB) {
        // column sums of this split's gz rows: thread (m = t & 63, wave q) summed plane q of every stage
        if (a.dbpart && blockIdx.y == 0) {             // uniform over the workgroup
            __syncthreads();
            lds[t] = bsum;
            __syncthreads();
            if (t < DN_T && m0 + t < a.M)
                a.dbpart[(long)blockIdx.z * a.M + m0 + t] = ((lds[t] + lds[64 + t]) + (lds[128 + t] + lds[192 + t])) +
                                                            ((lds[256 + t] + lds[320 + t]) + (lds[384 + t] + lds[448 + t]));
        }
    }
}

// dW[e] = sum over the splits of slab[z][e], db[c] likewise, over a fixed pairwise tree: eight splits at a time, then the
// (at most DN_MAX_SPLIT / 8) sums of eight.  A running sum in split order rounds once per split at the magnitude of the total:
// at 29 splits the bias gradient's error was 3 ulp, three times that of a pairwise column sum of the same values.
__global__ __launch_bounds__(256) void dense_bwd_w_finish_kernel(const float* __restrict__ ws, int nsplit, long mn, long m,
                                                                 float* __restrict__ dW, float* __restrict__ db) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = mn + (db ? m : 0);
    if (e >= total) return;
    const float* p = e < mn ? ws + e : ws + (long)nsplit * mn + (e - mn);
    const long pitch = e < mn ? mn : m;
    float q[DN_MAX_SPLIT / 8];
#pragma unroll
    for (int i = 0; i < DN_MAX_SPLIT / 8; ++i) {
        const int z = 8 * i;
        q[i] = 0.f;
        if (z < nsplit) {                              // uniform; eight loads in flight, a split past the end counts as 0
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = p[(long)(z + j < nsplit ? z + j : nsplit - 1) * pitch];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = z + j < nsplit ? v[j] : 0.f;
            q[i] = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        }
    }
    static_assert(DN_MAX_SPLIT == 32, "the tree below adds four sums of eight splits");
    const float sum = (q[0] + q[1]) + (q[2] + q[3]);
    if (e < mn) dW[e] = sum;
    else db[e - mn] = sum;
}

static inline bool dn_supported(long rows, long in, long out) {
    return rows >= 1 && rows < (1L << 31) && in >= 1 && in <= DN_MAX_DIM && out >= 32 && out <= DN_MAX_DIM && out % 32 == 0;
}
// splits of the dW contraction: 256 rows each, at most 32 (longer splits beyond that)
static inline int dn_splits(long rows) {
    const long n = (rows + DN_SPLIT_ROWS - 1) / DN_SPLIT_ROWS;
    return (int)(n < 1 ? 1 : (n > DN_MAX_SPLIT ? DN_MAX_SPLIT : n));
}

#define DN_LAUNCH(AKC, BKC, MASK, EPI, grid, st, a) \
    hipLaunchKernelGGL((dense_mfma_kernel<AKC, BKC, MASK, EPI>), grid, dim3(DN_NW * 64), 0, st, a)

extern "C" {

int xdfm_dense_supported(long rows, int in, int out) { return dn_supported(rows, in, out) ? 1 : 0; }

size_t xdfm_dense_bwd_w_ws_elems(long rows, int in, int out) {
    if (!dn_supported(rows, in, out)) return 0;
    return (size_t)dn_splits(rows) * ((size_t)out * in + out);
}

int xdfm_dense_fwd(const float* x, long rows, int in, long ldx, const float* W, int out, const float* b, int act, float* y,
                   long ldy, void* stream) {
    XDFM_REQUIRE(x && W && y, "dense_fwd: null pointer");
    XDFM_REQUIRE(rows > 0, "dense_fwd: rows = %ld", rows);
    XDFM_REQUIRE(in > 0, "dense_fwd: in = %d", in);
    XDFM_REQUIRE(dn_supported(rows, in, out), "dense_fwd: unsupported shape rows = %ld, in = %d, out = %d (out must be a multiple of 32)",
                 rows, in, out);
    XDFM_REQUIRE(ldx >= in, "dense_fwd: ldx = %ld < in = %d", ldx, in);
    XDFM_REQUIRE(ldy >= out, "dense_fwd: ldy = %ld < out = %d", ldy, out);
    XDFM_REQUIRE(act == XDFM_ACT_LINEAR || act == XDFM_ACT_RELU, "dense_fwd: act = %d (0 = none, 1 = relu)", act);
    DnArgs a{};
    a.A = x; a.lda = ldx; a.B = W; a.ldb = in; a.C = y; a.ldc = ldy; a.bias = b; a.relu = act == XDFM_ACT_RELU;
    a.M = rows; a.N = out; a.K = in; a.kper = round_up(in, DN_K);
    const dim3 grid(ceil_div(rows, DN_T), ceil_div(out, DN_T), 1);
    DN_LAUNCH(true, true, false, DN_EPI_FWD, grid, (hipStream_t)stream, a);
    return xdfm_check_launch("dense_fwd");
}

int xdfm_dense_bwd_x(const float* g, long ldg, const float* y, long ldy, long rows, int out, const float* W, int in, float* dx,
                     long lddx, void* stream) {
    XDFM_REQUIRE(g && W && dx, "dense_bwd_x: null pointer");
    XDFM_REQUIRE(rows > 0, "dense_bwd_x: rows = %ld", rows);
    XDFM_REQUIRE(in > 0, "dense_bwd_x: in = %d", in);
    XDFM_REQUIRE(dn_supported(rows, in, out), "dense_bwd_x: unsupported shape rows = %ld, in = %d, out = %d (out must be a multiple of 32)",
                 rows, in, out);
    XDFM_REQUIRE(ldg >= out, "dense_bwd_x: ldg = %ld < out = %d", ldg, out);
    XDFM_REQUIRE(!y || ldy >= out, "dense_bwd_x: ldy = %ld < out = %d", ldy, out);
    XDFM_REQUIRE(lddx >= in, "dense_bwd_x: lddx = %ld < in = %d", lddx, in);
    DnArgs a{};
    a.A = g; a.Ay = y; a.lda = ldg; a.lday = ldy; a.B = W; a.ldb = in; a.C = dx; a.ldc = lddx;
    a.M = rows; a.N = in; a.K = out; a.kper = round_up(out, DN_K);
    const dim3 grid(ceil_div(rows, DN_T), ceil_div(in, DN_T), 1);
    if (y) DN_LAUNCH(true, false, true, DN_EPI_PLAIN, grid, (hipStream_t)stream, a);
    else DN_LAUNCH(true, false, false, DN_EPI_PLAIN, grid, (hipStream_t)stream, a);
    return xdfm_check_launch("dense_bwd_x");
}

int xdfm_dense_bwd_w(const float* g, long ldg, const float* y, long ldy, const float* x, long ldx, long rows, int in, int out,
                     float* ws, float* dW, float* db, void* stream) {
    XDFM_REQUIRE(g && x && dW, "dense_bwd_w: null pointer");
    XDFM_REQUIRE(rows > 0, "dense_bwd_w: rows = %ld", rows);
    XDFM_REQUIRE(in > 0, "dense_bwd_w: in = %d", in);
    XDFM_REQUIRE(dn_supported(rows, in, out), "dense_bwd_w: unsupported shape rows = %ld, in = %d, out = %d (out must be a multiple of 32)",
                 rows, in, out);
    XDFM_REQUIRE(ws, "dense_bwd_w: workspace is NULL (xdfm_dense_bwd_w_ws_elems floats)");
    XDFM_REQUIRE(ldg >= out, "dense_bwd_w: ldg = %ld < out = %d", ldg, out);
    XDFM_REQUIRE(!y || ldy >= out, "dense_bwd_w: ldy = %ld < out = %d", ldy, out);
    XDFM_REQUIRE(ldx >= in, "dense_bwd_w: ldx = %ld < in = %d", ldx, in);
    hipStream_t st = (hipStream_t)stream;
    const int want = dn_splits(rows);
    const long kper = round_up(ceil_div(rows, want), DN_K);
    const int nsplit = ceil_div(rows, kper);             // <= want: what the workspace was sized for
    const long mn = (long)out * in;
    DnArgs a{};
    a.A = g; a.Ay = y; a.lda = ldg; a.lday = ldy; a.B = x; a.ldb = ldx;
    a.M = out; a.N = in; a.K = rows; a.kper = kper; a.ldc = in;
    if (nsplit == 1) { a.C = dW; a.cslab = 0; a.dbpart = db; }
    else { a.C = ws; a.cslab = mn; a.dbpart = db ? ws + (long)nsplit * mn : nullptr; }
    const dim3 grid(ceil_div(out, DN_T), ceil_div(in, DN_T), nsplit);
    if (y) DN_LAUNCH(false, false, true, DN_EPI_SLAB, grid, st, a);
    else DN_LAUNCH(false, false, false, DN_EPI_SLAB, grid, st, a);
    if (nsplit > 1) {
        const long total = mn + (db ? out : 0);
        hipLaunchKernelGGL(dense_bwd_w_finish_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, ws, nsplit, mn, (long)out, dW, db);
    }
    return xdfm_check_launch("dense_bwd_w");
}

}  // extern "C"
