// Dense layers of the DNN tower on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulators; no operand splitting).
//
// replaces, per layer of deepctr/layers/core.py:120-134: the three hipBLASLt GEMMs (forward, input gradient, weight
// gradient), the threshold_backward pass that wrote gz = (y > 0) ? g : 0, and the bias gradient's column sum with its
// finish launch.  gz is never stored: the two backward kernels form it while they stage their operand.
// (The host side runs the two backward kernels; the forward kernel does not beat the library GEMM yet and is kept,
// tested, behind ops.DNN_NATIVE_FWD.  With dropout the host runs all three: see "Dropout" below.)
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
//
// Dropout (the _drop entry points; deepctr/layers/core.py:134 applies nn.Dropout after every activation).  The forward's
// DROP epilogue stores d = keep ? relu(z) * s : 0 with s = 1 / (1 - p) and keep a counter-based hash of (seed, layer, row,
// column): d > 0 holds exactly where the cell was kept AND z > 0, so the layer's output is its own mask.  The two backward
// kernels already select on y > 0 while they stage g; their SCALED instances multiply the selected value by the same s.
// No mask is stored or regenerated, no launch is added either way.
//
// PReLU (the _prelu entry points; nn.PReLU() behind every layer, one scalar slope alpha per layer, read from device memory by
// every kernel: the optimizer moves it and a replayed graph must see the new value).  The forward's epilogue stores
// y = z > 0 ? z : alpha * z and, for the backward, the pre-activation z itself: alpha may be 0, 1 or negative, so neither
// the sign nor the value of z can be read off y.  The two backward kernels form gz = z > 0 ? g : alpha * g while they stage
// g (one rounding, never stored).  The slope's gradient, sum of g * z over the cells with z <= 0, is a by-product of the dW
// kernel as the bias gradient is: the blocks that leave the bias partials also leave one partial per (tile of out, split),
// products and sums in double, and the finish launch adds them in a fixed order and rounds once.
#include "xdfm_internal.h"
#include "finish_batch.h"

#define DN_T 64                    // tile edge (rows and columns of C per workgroup)
#define DN_K 32                    // contraction indices per LDS stage
#define DN_NW 8                    // waves per workgroup
#define DN_E 4                     // elements of an operand tile per thread: DN_T * DN_K / (64 * DN_NW)
#define DN_PLANE (DN_T * 4 + 8)    // floats per plane (8 of padding)
#define DN_TILE (8 * DN_PLANE)     // floats per operand tile
#define DN_SPLIT_ROWS 256          // rows of the contraction per dW split
#define DN_MAX_DIM (1 << 20)       // in, out

struct DnArgs {
    const float* A; const float* Ay; long lda, lday;     // Ay: the layer's output for the ReLU mask (MASK instances)
    const float* B; long ldb;
    float* C; long ldc, cslab;                           // split z writes C + z * cslab
    const float* bias; int relu;                         // forward epilogue
    float* dbpart;                                       // dW: split z leaves its column sums of gz at dbpart + z * M
    long M, N, K, kper;                                  // kper: contraction indices per split (a multiple of DN_K)
    // dropout (behind the fields above: the plain instances read none of these)
    const unsigned long long* seed;                      // DROP epilogue: device scalar, read by the kernel
    long row0;                                           //   row r of this call is row row0 + r of the mask
    unsigned thresh; int layer;                          //   keep iff hash >= thresh
    float keep_scale;                                    // 1 / (1 - p): DROP epilogue and the SCALED stagings of g
    // PReLU (read by the PRELU instances only)
    const float* alpha;                                  // device scalar: the layer's slope
    float* Z; long ldz;                                  // forward: the pre-activation goes here too (NULL: y only)
    double* dapart;                                      // dW: block (x, y = 0, z) leaves its sum of g * z [z <= 0] at dapart[z * gridDim.x + x]
};

// Keep bit of cell (layer, row, col): three rounds of drop_mix, the shape of the attention's key (attn.hip, drop_row_key).
__device__ __forceinline__ unsigned dn_drop_layer_key(unsigned long long seed, int layer) {
    return drop_mix((unsigned)seed ^ ((unsigned)layer * 0x9E3779B1U));
}
__device__ __forceinline__ unsigned dn_drop_row_key(unsigned layer_key, unsigned long long seed, long row) {
    return drop_mix(layer_key + (unsigned)(seed >> 32) + (unsigned)row * 0x85EBCA77U);
}
__device__ __forceinline__ bool dn_drop_keep(unsigned row_key, long col, unsigned thresh) {
    return drop_mix(row_key + (unsigned)col * 0x9E3779B1U) >= thresh;
}

__device__ __forceinline__ int dn_lds(int p, int m) { return p * DN_PLANE + (m << 2); }

// One thread's share of a 32 x 64 operand tile T[k][m]: 4 elements, loaded ahead and written to LDS a stage later.
// Every load is unconditional -- an index past the end is clamped to the last valid one and the value dropped at the
// write (hipcc puts a load behind a condition into a branch of its own and waits for it there).
// KC (k contiguous in memory, src[m * ld + k]): lanes run along k, element e is row (t >> 5) + 16 e.
// otherwise (m contiguous, src[k * ld + m]):    lanes run along m, wave q stages plane q.
// SCALED (with MASK): a live value is multiplied by gscale, one rounding -- the gradient through a dropout layer whose
// kept cells are the y > 0 ones.
// PRELU (with MASK; y then holds the pre-activation z and gscale the slope): a live value with z <= 0 is multiplied by the
// slope, one rounding; PRELU == 2 also adds its g * z to *da, product and sum in double.
template <bool KC, bool MASK, bool SCALED = false, int PRELU = 0>
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
    __device__ __forceinline__ float store(float* __restrict__ tile, float gscale = 1.f, double* da = nullptr) {
        const int t = threadIdx.x;
        static_assert(!PRELU || (MASK && !SCALED), "the PReLU stagings read z where the ReLU ones read y");
#pragma unroll
        for (int e = 0; e < DN_E; ++e) {
            if constexpr (PRELU != 0) {
                const bool in = ok >> e & 1u;
                if constexpr (PRELU == 2) {
                    if (in && y[e] <= 0.f) *da = fma((double)v[e], (double)y[e], *da);
                }
                v[e] = in ? (y[e] > 0.f ? v[e] : gscale * v[e]) : 0.f;
            } else {
                const bool live = (ok >> e & 1u) && (!MASK || y[e] > 0.f);
                if (SCALED) v[e] = live ? v[e] * gscale : 0.f;
                else v[e] = live ? v[e] : 0.f;
            }
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

// 3 .. 5 are the dropout instances of the first three: the forward's DROP epilogue, dX and dW with g scaled; 6 .. 8 the PReLU
// ones: the forward's epilogue that stores y and z, dX and dW with gz formed from z and the slope (dW: the slope's gradient too)
enum { DN_EPI_FWD = 0, DN_EPI_PLAIN = 1, DN_EPI_SLAB = 2, DN_EPI_FWD_DROP = 3, DN_EPI_PLAIN_SCALED = 4, DN_EPI_SLAB_SCALED = 5,
       DN_EPI_FWD_PRELU = 6, DN_EPI_PLAIN_PRELU = 7, DN_EPI_SLAB_PRELU = 8 };

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

    constexpr bool FWD = EPI == DN_EPI_FWD || EPI == DN_EPI_FWD_DROP || EPI == DN_EPI_FWD_PRELU;
    constexpr bool SLAB = EPI == DN_EPI_SLAB || EPI == DN_EPI_SLAB_SCALED || EPI == DN_EPI_SLAB_PRELU;
    constexpr bool SCALED = EPI == DN_EPI_PLAIN_SCALED || EPI == DN_EPI_SLAB_SCALED;
    constexpr int PRELU = EPI == DN_EPI_SLAB_PRELU ? 2 : (EPI == DN_EPI_PLAIN_PRELU ? 1 : 0);      // of the staging of g
    static_assert(!SCALED || MASK, "g is scaled where the mask is open");
    float gscale = 1.f;
    if constexpr (SCALED) gscale = a.keep_scale;
    if constexpr (PRELU != 0 || EPI == DN_EPI_FWD_PRELU) gscale = *a.alpha;
    double da = 0.0;                                   // PRELU == 2: this thread's share of the slope's gradient
    DnStage<AKC, MASK, SCALED, PRELU> sa;
    DnStage<BKC, false> sb;
    sa.init(a.lda, a.lday, m0, a.M);
    sb.init(a.ldb, 0, n0, a.N);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bsum = 0.f;

    sa.load(a.A, a.Ay, a.lda, a.lday, kbeg, kend);
    sb.load(a.B, nullptr, a.ldb, 0, kbeg, kend);
    bsum += sa.store(lds, gscale, &da);
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
            bsum += sa.store(nxt, gscale, &da);
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
        if (FWD && a.bias && col < a.N) bv = a.bias[col];
        unsigned long long seed = 0;
        unsigned layer_key = 0;
        if (EPI == DN_EPI_FWD_DROP) {
            seed = *a.seed;
            layer_key = dn_drop_layer_key(seed, a.layer);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = m0 + wm + frag_row(r, s);
            if (row >= a.M || col >= a.N) continue;
            float v = acc[r];
            if (FWD) {
                v += bv;
                if (a.relu) v = v < 0.f ? 0.f : v;
            }
            if constexpr (EPI == DN_EPI_FWD_PRELU) {
                if (a.Z) a.Z[row * a.ldz + col] = v;
                v = v > 0.f ? v : gscale * v;
            }
            if (EPI == DN_EPI_FWD_DROP) {
                // this lane owns one cell of each of its 16 rows: one row key per row
                const unsigned rk = dn_drop_row_key(layer_key, seed, a.row0 + row);
                v = dn_drop_keep(rk, col, a.thresh) ? v * a.keep_scale : 0.f;
            }
            C[row * a.ldc + col] = v;
        }
    }
    if (SLAB) {
        // column sums of this split's gz rows: thread (m = t & 63, wave q) summed plane q of every stage
        if (a.dbpart && blockIdx.y == 0) {             // uniform over the workgroup
            __syncthreads();
            lds[t] = bsum;
            __syncthreads();
            if (t < DN_T && m0 + t < a.M)
                a.dbpart[(long)blockIdx.z * a.M + m0 + t] = ((lds[t] + lds[64 + t]) + (lds[128 + t] + lds[192 + t])) +
                                                            ((lds[256 + t] + lds[320 + t]) + (lds[384 + t] + lds[448 + t]));
        }
        if constexpr (EPI == DN_EPI_SLAB_PRELU) {
            // the same blocks saw every cell of g and z of their (tile of out, split) exactly once
            if (a.dapart && blockIdx.y == 0) {         // uniform over the workgroup
                __syncthreads();
                const double s = xdfm_block_sum_f64(da, (double*)lds);
                if (t == 0) a.dapart[(long)blockIdx.z * gridDim.x + blockIdx.x] = s;
            }
        }
    }
}

__global__ __launch_bounds__(256) void dense_bwd_w_finish_kernel(const float* __restrict__ ws, int nsplit, long mn, long m,
                                                                 float* __restrict__ dW, float* __restrict__ db) {
    dn_finish_elem((long)blockIdx.x * 256 + threadIdx.x, ws, nsplit, mn, m, dW, db);
}
// The PReLU layer's finish: blocks [0, eblocks) are the finish above (none with a single split, whose dW and db are final);
// one more block adds the npart partials of the slope's gradient -- thread t those of index t, t + 256, ... in order, then
// xdfm_block_sum_f64 -- in double and rounds once.
__global__ __launch_bounds__(256) void dense_prelu_bwd_w_finish_kernel(const float* __restrict__ ws, int nsplit, long mn, long m,
                                                                       float* __restrict__ dW, float* __restrict__ db, unsigned eblocks,
                                                                       const double* __restrict__ dapart, int npart,
                                                                       float* __restrict__ dalpha) {
    if (blockIdx.x < eblocks) {                        // uniform over the workgroup
        dn_finish_elem((long)blockIdx.x * 256 + threadIdx.x, ws, nsplit, mn, m, dW, db);
        return;
    }
    __shared__ double sm[4];
    dn_dalpha_finish_block(dapart, npart, dalpha, sm);
}
// the finish of a layer's dW / db (/ dalpha): a job of the open finish batch (finish_batch.h), else its own launch; eblocks = 0
// and no dalpha: nothing to do (a single split's dW and db are final)
int xdfm_dense_w_finish(const float* ws, int nsplit, long mn, long m, float* dW, float* db, bool prelu, const double* dapart, int npart,
                        float* dalpha, hipStream_t st) {
    const unsigned eblocks = nsplit > 1 ? (unsigned)ceil_div(mn + (db ? m : 0), 256) : 0u;
    if (!eblocks && !(prelu && dalpha)) return XDFM_OK;
    FinishJob j{};
    j.kind = FJ_DENSE_W; j.blocks = (int)eblocks + (prelu && dalpha ? 1 : 0);
    j.part = ws; j.i0 = nsplit; j.n0 = mn; j.n1 = m; j.out = dW; j.out2 = db; j.i1 = (int)eblocks;
    if (prelu) { j.part2 = dapart; j.i2 = npart; j.out3 = dalpha; }
    bool taken = false;
    if (int rc = xdfm_finish_defer(j, st, &taken)) return rc;
    if (taken) return XDFM_OK;
    if (prelu)
        hipLaunchKernelGGL(dense_prelu_bwd_w_finish_kernel, dim3(eblocks + (dalpha ? 1u : 0u)), dim3(256), 0, st, ws, nsplit, mn, m, dW,
                           db, eblocks, dapart, npart, dalpha);
    else
        hipLaunchKernelGGL(dense_bwd_w_finish_kernel, dim3(eblocks), dim3(256), 0, st, ws, nsplit, mn, m, dW, db);
    return XDFM_OK;
}

static inline bool dn_supported(long rows, long in, long out) {
    return rows >= 1 && rows < (1L << 31) && in >= 1 && in <= DN_MAX_DIM && out >= 32 && out <= DN_MAX_DIM && out % 32 == 0;
}
// splits of the dW contraction: 256 rows each, at most 32 (longer splits beyond that)
static inline int dn_splits(long rows) {
    const long n = (rows + DN_SPLIT_ROWS - 1) / DN_SPLIT_ROWS;
    return (int)(n < 1 ? 1 : (n > DN_MAX_SPLIT ? DN_MAX_SPLIT : n));
}

// The keep mask the DROP epilogue draws, written out: keep[row][col] (1 = kept).  Test hook, like attn_dropout_mask_kernel.
__global__ __launch_bounds__(256) void dense_dropout_mask_kernel(long rows, int out, const unsigned long long* __restrict__ seed_p,
                                                                 unsigned thresh, int layer, long row0, unsigned char* __restrict__ keep) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * out) return;
    const long row = e / out, col = e - row * out;
    const unsigned long long seed = seed_p ? *seed_p : 0ull;           // NULL only with p_drop = 0: thresh = 0 keeps every cell
    const unsigned rk = dn_drop_row_key(dn_drop_layer_key(seed, layer), seed, row0 + row);
    keep[e] = dn_drop_keep(rk, col, thresh) ? 1 : 0;
}

#define DN_LAUNCH(AKC, BKC, MASK, EPI, grid, st, a) \
    hipLaunchKernelGGL((dense_mfma_kernel<AKC, BKC, MASK, EPI>), grid, dim3(DN_NW * 64), 0, st, a)
// The instances, instantiated here so that the code object's layout does not follow the order of the launches below.
#define DN_INSTANCE(AKC, BKC, MASK, EPI) template __global__ void dense_mfma_kernel<AKC, BKC, MASK, EPI>(DnArgs)
DN_INSTANCE(true, true, false, DN_EPI_FWD_DROP);     DN_INSTANCE(true, true, false, DN_EPI_FWD);
DN_INSTANCE(true, false, true, DN_EPI_PLAIN_SCALED); DN_INSTANCE(true, false, true, DN_EPI_PLAIN);
DN_INSTANCE(true, false, false, DN_EPI_PLAIN);
DN_INSTANCE(false, false, true, DN_EPI_SLAB_SCALED); DN_INSTANCE(false, false, true, DN_EPI_SLAB);
DN_INSTANCE(false, false, false, DN_EPI_SLAB);
DN_INSTANCE(true, true, false, DN_EPI_FWD_PRELU);    DN_INSTANCE(true, false, true, DN_EPI_PLAIN_PRELU);
DN_INSTANCE(false, false, true, DN_EPI_SLAB_PRELU);

// Dropout arguments of the _drop entry points, checked: on = p_drop > 0 (p_drop = 0 runs the plain instances).
struct DnDrop {
    bool on;
    const unsigned long long* seed; unsigned thresh; float keep_scale; int layer; long row0;
};
static const DnDrop DN_NO_DROP = {false, nullptr, 0u, 1.f, 0, 0};
static int dn_drop_rate(const char* who, float p_drop, DnDrop* d) {
    *d = DN_NO_DROP;
    XDFM_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "%s: p_drop = %g outside [0, 1)", who, p_drop);
    d->on = p_drop > 0.f;
    if (d->on) { d->thresh = xdfm_drop_thresh(p_drop); d->keep_scale = xdfm_drop_keep_scale(p_drop); }
    return XDFM_OK;
}
static int dn_drop_mask_args(const char* who, float p_drop, const unsigned long long* seed, int layer, long row0, DnDrop* d) {
    if (int rc = dn_drop_rate(who, p_drop, d)) return rc;
    XDFM_REQUIRE(layer >= 0, "%s: layer = %d", who, layer);
    XDFM_REQUIRE(row0 >= 0, "%s: row0 = %ld", who, row0);
    XDFM_REQUIRE(!d->on || seed, "%s: p_drop = %g needs a device seed, seed is NULL", who, p_drop);
    d->seed = seed; d->layer = layer; d->row0 = row0;
    return XDFM_OK;
}

// What gates one layer's gradient: nothing, the ReLU mask y > 0, that mask with the kept cells scaled (dropout), or PReLU's
// z > 0 ? 1 : alpha.  `y` is the operand the backward kernels read next to g -- the layer's output, for PReLU its
// pre-activation z, which the forward writes there -- and `name` what the entry point calls it ("y" / "z", pitch "ldy" /
// "ldz") in messages.
struct DnGate {
    enum Kind { PLAIN, RELU, DROP, PRELU } kind;
    const char* name;
    const float* y; long ldy;
    DnDrop drop;                   // DROP; keep_scale = 1 for PLAIN and RELU
    const float* alpha;            // PRELU
};
// the plain and the _drop entry points: drop.on decides, then y (NULL: no mask)
static DnGate dn_gate(const float* y, long ldy, const DnDrop& drop) {
    return DnGate{drop.on ? DnGate::DROP : y ? DnGate::RELU : DnGate::PLAIN, "y", y, ldy, drop, nullptr};
}
static DnGate dn_gate_prelu(const float* z, long ldz, const float* alpha) { return DnGate{DnGate::PRELU, "z", z, ldz, DnDrop{}, alpha}; }

#define DN_REQUIRE_SHAPE(who, rows, in, out) \
    XDFM_REQUIRE(rows > 0, "%s: rows = %ld", who, rows); \
    XDFM_REQUIRE(in > 0, "%s: in = %d", who, in); \
    XDFM_REQUIRE(dn_supported(rows, in, out), "%s: unsupported shape rows = %ld, in = %d, out = %d (out must be a multiple of 32)", \
                 who, rows, in, out)
// the gating operand's pitch, and the dropped layer's need of its output (backward)
#define DN_REQUIRE_GATE(who, gate, out) \
    XDFM_REQUIRE(!gate.y || gate.ldy >= out, "%s: ld%s = %ld < out = %d", who, gate.name, gate.ldy, out); \
    XDFM_REQUIRE(gate.kind != DnGate::DROP || gate.y, "%s: p_drop > 0 needs y (the layer's dropped output is the mask), y is NULL", who)

// Forward.  The gate is PLAIN (act says whether the epilogue applies ReLU), DROP or PRELU (gate.y: where z goes, or NULL).
static int dn_fwd(const char* who, const float* x, long rows, int in, long ldx, const float* W, int out, const float* b, int act,
                  float* y, long ldy, const DnGate& gate, void* stream) {
    XDFM_REQUIRE(x && W && y, "%s: null pointer", who);
    DN_REQUIRE_SHAPE(who, rows, in, out);
    XDFM_REQUIRE(ldx >= in, "%s: ldx = %ld < in = %d", who, ldx, in);
    XDFM_REQUIRE(ldy >= out, "%s: ldy = %ld < out = %d", who, ldy, out);
    XDFM_REQUIRE(!gate.y || gate.ldy >= out, "%s: ld%s = %ld < out = %d", who, gate.name, gate.ldy, out);
    XDFM_REQUIRE(act == XDFM_ACT_LINEAR || act == XDFM_ACT_RELU, "%s: act = %d (0 = none, 1 = relu)", who, act);
    XDFM_REQUIRE(gate.kind != DnGate::DROP || act == XDFM_ACT_RELU,
                 "%s: p_drop > 0 needs act = 1 (relu), act = %d: the backward reads the mask off y > 0", who, act);
    DnArgs a{};
    a.A = x; a.lda = ldx; a.B = W; a.ldb = in; a.C = y; a.ldc = ldy; a.bias = b; a.relu = act == XDFM_ACT_RELU;
    a.M = rows; a.N = out; a.K = in; a.kper = round_up(in, DN_K);
    a.seed = gate.drop.seed; a.row0 = gate.drop.row0; a.thresh = gate.drop.thresh; a.layer = gate.drop.layer;
    a.keep_scale = gate.drop.keep_scale;
    a.alpha = gate.alpha; a.Z = const_cast<float*>(gate.y); a.ldz = gate.ldy;
    const dim3 grid(ceil_div(rows, DN_T), ceil_div(out, DN_T), 1);
    if (gate.kind == DnGate::DROP) DN_LAUNCH(true, true, false, DN_EPI_FWD_DROP, grid, (hipStream_t)stream, a);
    else if (gate.kind == DnGate::PRELU) DN_LAUNCH(true, true, false, DN_EPI_FWD_PRELU, grid, (hipStream_t)stream, a);
    else DN_LAUNCH(true, true, false, DN_EPI_FWD, grid, (hipStream_t)stream, a);
    return xdfm_check_launch(who);
}

static int dn_bwd_x(const char* who, const float* g, long ldg, long rows, int out, const float* W, int in, float* dx, long lddx,
                    const DnGate& gate, void* stream) {
    XDFM_REQUIRE(g && W && dx, "%s: null pointer", who);
    DN_REQUIRE_SHAPE(who, rows, in, out);
    XDFM_REQUIRE(ldg >= out, "%s: ldg = %ld < out = %d", who, ldg, out);
    DN_REQUIRE_GATE(who, gate, out);
    XDFM_REQUIRE(lddx >= in, "%s: lddx = %ld < in = %d", who, lddx, in);
    DnArgs a{};
    a.A = g; a.Ay = gate.y; a.lda = ldg; a.lday = gate.ldy; a.B = W; a.ldb = in; a.C = dx; a.ldc = lddx;
    a.M = rows; a.N = in; a.K = out; a.kper = round_up(out, DN_K);
    a.keep_scale = gate.drop.keep_scale; a.alpha = gate.alpha;
    const dim3 grid(ceil_div(rows, DN_T), ceil_div(in, DN_T), 1);
    if (gate.kind == DnGate::DROP) DN_LAUNCH(true, false, true, DN_EPI_PLAIN_SCALED, grid, (hipStream_t)stream, a);
    else if (gate.kind == DnGate::PRELU) DN_LAUNCH(true, false, true, DN_EPI_PLAIN_PRELU, grid, (hipStream_t)stream, a);
    else if (gate.kind == DnGate::RELU) DN_LAUNCH(true, false, true, DN_EPI_PLAIN, grid, (hipStream_t)stream, a);
    else DN_LAUNCH(true, false, false, DN_EPI_PLAIN, grid, (hipStream_t)stream, a);
    return xdfm_check_launch(who);
}

// floats of the dW workspace: per split a slab of dW and the bias partials
static inline size_t dn_ws_floats(int splits, long in, long out) { return (size_t)splits * ((size_t)out * in + out); }
// ... in front of the PReLU layer's doubles: rounded up to an even count (the base is 8-byte aligned)
static inline size_t dn_prelu_ws_floats(int splits, long in, long out) {
    const size_t n = dn_ws_floats(splits, in, out);
    return n + (n & 1);
}

// dalpha: PRELU only (NULL: no slope gradient); then ws is 8-byte aligned and holds the doubles behind its floats
static int dn_bwd_w(const char* who, const float* g, long ldg, const float* x, long ldx, long rows, int in, int out, float* ws,
                    float* dW, float* db, float* dalpha, const DnGate& gate, void* stream) {
    const bool prelu = gate.kind == DnGate::PRELU;
    XDFM_REQUIRE(g && x && dW, "%s: null pointer", who);
    DN_REQUIRE_SHAPE(who, rows, in, out);
    XDFM_REQUIRE(ws, "%s: workspace is NULL (xdfm_dense%s_bwd_w_ws_elems floats)", who, prelu ? "_prelu" : "");
    XDFM_REQUIRE(ldg >= out, "%s: ldg = %ld < out = %d", who, ldg, out);
    DN_REQUIRE_GATE(who, gate, out);
    XDFM_REQUIRE(ldx >= in, "%s: ldx = %ld < in = %d", who, ldx, in);
    hipStream_t st = (hipStream_t)stream;
    const int want = dn_splits(rows);
    const long kper = round_up(ceil_div(rows, want), DN_K);
    const int nsplit = ceil_div(rows, kper);             // <= want: what the workspace was sized for
    const long mn = (long)out * in;
    const int mtiles = ceil_div(out, DN_T);
    double* dapart = dalpha ? (double*)(ws + dn_prelu_ws_floats(nsplit, in, out)) : nullptr;
    DnArgs a{};
    a.A = g; a.Ay = gate.y; a.lda = ldg; a.lday = gate.ldy; a.B = x; a.ldb = ldx;
    a.M = out; a.N = in; a.K = rows; a.kper = kper; a.ldc = in;
    a.keep_scale = gate.drop.keep_scale; a.alpha = gate.alpha; a.dapart = dapart;
    if (nsplit == 1) { a.C = dW; a.cslab = 0; a.dbpart = db; }
    else { a.C = ws; a.cslab = mn; a.dbpart = db ? ws + (long)nsplit * mn : nullptr; }
    const dim3 grid(mtiles, ceil_div(in, DN_T), nsplit);
    if (gate.kind == DnGate::DROP) DN_LAUNCH(false, false, true, DN_EPI_SLAB_SCALED, grid, st, a);
    else if (prelu) DN_LAUNCH(false, false, true, DN_EPI_SLAB_PRELU, grid, st, a);
    else if (gate.kind == DnGate::RELU) DN_LAUNCH(false, false, true, DN_EPI_SLAB, grid, st, a);
    else DN_LAUNCH(false, false, false, DN_EPI_SLAB, grid, st, a);
    // the finish over the splits (none with a single split, whose dW and db are final); PReLU's has one more block for the slope
    if (int rc = xdfm_dense_w_finish(ws, nsplit, mn, (long)out, dW, db, prelu, dapart, nsplit * mtiles, dalpha, st)) return rc;
    return xdfm_check_launch(who);
}

extern "C" {

int xdfm_dense_supported(long rows, int in, int out) { return dn_supported(rows, in, out) ? 1 : 0; }

size_t xdfm_dense_bwd_w_ws_elems(long rows, int in, int out) {
    return dn_supported(rows, in, out) ? dn_ws_floats(dn_splits(rows), in, out) : 0;
}

size_t xdfm_dense_prelu_bwd_w_ws_elems(long rows, int in, int out) {
    if (!dn_supported(rows, in, out)) return 0;
    const int splits = dn_splits(rows);
    return dn_prelu_ws_floats(splits, in, out) + (size_t)2 * splits * ceil_div(out, DN_T);       // one double per (tile of out, split)
}

int xdfm_dense_fwd(const float* x, long rows, int in, long ldx, const float* W, int out, const float* b, int act, float* y,
                   long ldy, void* stream) {
    return dn_fwd("dense_fwd", x, rows, in, ldx, W, out, b, act, y, ldy, dn_gate(nullptr, 0, DN_NO_DROP), stream);
}

int xdfm_dense_bwd_x(const float* g, long ldg, const float* y, long ldy, long rows, int out, const float* W, int in, float* dx,
                     long lddx, void* stream) {
    return dn_bwd_x("dense_bwd_x", g, ldg, rows, out, W, in, dx, lddx, dn_gate(y, ldy, DN_NO_DROP), stream);
}

int xdfm_dense_bwd_w(const float* g, long ldg, const float* y, long ldy, const float* x, long ldx, long rows, int in, int out,
                     float* ws, float* dW, float* db, void* stream) {
    return dn_bwd_w("dense_bwd_w", g, ldg, x, ldx, rows, in, out, ws, dW, db, nullptr, dn_gate(y, ldy, DN_NO_DROP), stream);
}

int xdfm_dense_fwd_drop(const float* x, long rows, int in, long ldx, const float* W, int out, const float* b, int act, float* y,
                        long ldy, float p_drop, const unsigned long long* seed, int layer, long row0, void* stream) {
    DnDrop drop;
    if (int rc = dn_drop_mask_args("dense_fwd_drop", p_drop, seed, layer, row0, &drop)) return rc;
    return dn_fwd("dense_fwd_drop", x, rows, in, ldx, W, out, b, act, y, ldy, dn_gate(nullptr, 0, drop), stream);
}

int xdfm_dense_bwd_x_drop(const float* g, long ldg, const float* y, long ldy, long rows, int out, const float* W, int in, float* dx,
                          long lddx, float p_drop, void* stream) {
    DnDrop drop;
    if (int rc = dn_drop_rate("dense_bwd_x_drop", p_drop, &drop)) return rc;
    return dn_bwd_x("dense_bwd_x_drop", g, ldg, rows, out, W, in, dx, lddx, dn_gate(y, ldy, drop), stream);
}

int xdfm_dense_bwd_w_drop(const float* g, long ldg, const float* y, long ldy, const float* x, long ldx, long rows, int in, int out,
                          float* ws, float* dW, float* db, float p_drop, void* stream) {
    DnDrop drop;
    if (int rc = dn_drop_rate("dense_bwd_w_drop", p_drop, &drop)) return rc;
    return dn_bwd_w("dense_bwd_w_drop", g, ldg, x, ldx, rows, in, out, ws, dW, db, nullptr, dn_gate(y, ldy, drop), stream);
}

int xdfm_dense_prelu_fwd(const float* x, long rows, int in, long ldx, const float* W, int out, const float* b, const float* alpha,
                         float* y, long ldy, float* z, long ldz, void* stream) {
    XDFM_REQUIRE(alpha, "dense_prelu_fwd: null pointer");
    XDFM_REQUIRE(!y || y != z, "dense_prelu_fwd: y == z (the backward needs the pre-activation apart from the output)");
    return dn_fwd("dense_prelu_fwd", x, rows, in, ldx, W, out, b, XDFM_ACT_LINEAR, y, ldy, dn_gate_prelu(z, ldz, alpha), stream);
}

int xdfm_dense_prelu_bwd_x(const float* g, long ldg, const float* z, long ldz, const float* alpha, long rows, int out, const float* W,
                           int in, float* dx, long lddx, void* stream) {
    XDFM_REQUIRE(z && alpha, "dense_prelu_bwd_x: null pointer");
    return dn_bwd_x("dense_prelu_bwd_x", g, ldg, rows, out, W, in, dx, lddx, dn_gate_prelu(z, ldz, alpha), stream);
}

int xdfm_dense_prelu_bwd_w(const float* g, long ldg, const float* z, long ldz, const float* alpha, const float* x, long ldx, long rows,
                           int in, int out, float* ws, float* dW, float* db, float* dalpha, void* stream) {
    XDFM_REQUIRE(z && alpha, "dense_prelu_bwd_w: null pointer");
    XDFM_REQUIRE(((size_t)ws & 7) == 0, "dense_prelu_bwd_w: workspace not 8-byte aligned");
    return dn_bwd_w("dense_prelu_bwd_w", g, ldg, x, ldx, rows, in, out, ws, dW, db, dalpha, dn_gate_prelu(z, ldz, alpha), stream);
}

int xdfm_dense_dropout_mask(long rows, int out, float p_drop, const unsigned long long* seed, int layer, long row0,
                            unsigned char* keep, void* stream) {
    XDFM_REQUIRE(keep, "dense_dropout_mask: null pointer");
    XDFM_REQUIRE(rows > 0 && rows < (1L << 31), "dense_dropout_mask: rows = %ld", rows);
    XDFM_REQUIRE(out > 0 && out <= DN_MAX_DIM, "dense_dropout_mask: out = %d", out);
    DnDrop drop;
    if (int rc = dn_drop_mask_args("dense_dropout_mask", p_drop, seed, layer, row0, &drop)) return rc;
    const long blocks = (rows * out + 255) / 256;
    XDFM_REQUIRE(blocks <= 0x7fffffffL, "dense_dropout_mask: rows = %ld x out = %d cells are more than one launch covers", rows, out);
    hipLaunchKernelGGL(dense_dropout_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, out, drop.seed,
                       drop.thresh, layer, row0, keep);
    return xdfm_check_launch("dense_dropout_mask");
}

}  // extern "C"

