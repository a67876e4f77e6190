// K7w: the row-wise Adagrad step (the DLRM / TorchRec default for embedding tables, FBGEMM's "exact row-wise Adagrad") over
// 2-D tensors [rows, D]: ONE accumulator per row, the running sum over the steps of the mean over the row of g'^2.  The state is
// 1/D of Adagrad's and the sweep moves 8 + 8/D bytes per parameter (p read and written, s read and written once per row)
// instead of K7g's 16.  Unlike every other K7 kernel, which updates a 16-byte chunk on its own, this one must see a whole row,
// gradient and L2 term, before it may write any element of it.  So its loops are its own; everything around them is shared: the
// streaming accesses, the block's L2 partial (tbl_l2_slot), the call's checks and the launch composition (table_step.h:
// tbl_check_call, tbl_check_l2, tbl_launches), the block cap (option "opt_bx"), the workspace size
// (xdfm_opt_step_ws_elems) and the L2 finish (xdfm_adam_l2_finish).  The arithmetic is opt_math.h's (rw_*); D == 1 IS Adagrad
// and calls opt_one<OPT_ADAGRAD>.
//
// Per row, in fp32 unless said otherwise (l2m: the tensor's armed L2 strength):
//   g'_d = fma(2 l2m, p_d, g_d);   S = sum_d (double)g'_d (double)g'_d   (order: opt_math.h);   ms = (float)(S / (double)D)
//   s' = s + ms;   den = sqrtf(s') + eps;   p_d' = fma(-lr, g'_d / den, p_d)        (selects: ms == 0 keeps s, g'_d == 0 keeps p_d)
//
// Three paths, one summation order, the same bits:
//   lanes  D in {4, 8, 16, 32, 64}, param and grad 16-byte aligned: D / 4 neighbouring lanes hold a row's float4s in registers,
//          add their chunk sums by a butterfly (__shfl_xor) and update; coalesced, streaming accesses.  Dense gradients, and
//          marked ones of a tensor with l2m > 0 (every row is a real update; an unmarked chunk enters with the opaque zero).
//   rows   the same tensors with marks and l2m == 0: a row without a marked chunk has g' == 0 and is skipped without being
//          read.  One thread per row reads the row's D / 4 mark bytes; a marked row is updated by that one thread.
//   units  every other D and every unaligned pointer: one thread per unit of four consecutive rows -- exactly D 16-byte chunks,
//          so a unit owns its chunks whole for any D -- in scalar accesses.  The rows % 4 tail rows are one more unit, always
//          read and zeroed (the numel % 4 rule of the other kernels).
#include "xdfm_internal.h"
#include "opt_math.h"      // rw_* / opt_one, opt_bx_cap
#include "table_step.h"
#include "finish_batch.h"  // xdfm_adam_l2_finish

#define ROW_THREADS 256
#define ROW_BX 512              // most blocks one tensor gets: OPT_BX, so xdfm_opt_step_ws_elems(T) holds the partials
#define ROW_BLOCK_ELEMS 8192    // a tensor gets one block per this many elements
#define ROW_CHUNK 64            // tensors per launch: 64 descriptors of 48 bytes + first[] stay inside the 4 KB argument block
#define ROW_NF 4                // chunks per array and thread in flight on the lanes path

struct RowDev { float* param; float* grad; float* state; unsigned char* grad_marks; long numel; int dim; float l2; };
struct RowBatch { RowDev t[ROW_CHUNK]; int first[ROW_CHUNK + 1]; };
static_assert(sizeof(RowBatch) + 128 <= 4096, "the row-wise kernel's argument block");

struct RowCtx { float g2, nlr, eps, zf; };

// ---- lanes: L = D / 4 lanes per row.  MARKED: the gradient is read by its mark bytes (l2m > 0), else in full.
template <int L, bool MARKED>
__device__ __forceinline__ void rw_lanes(const RowDev& d, const RowCtx& c, long lb, long nb, float& sq) {
    constexpr int NF = ROW_NF;
    constexpr int D = 4 * L;
    float4* p4 = reinterpret_cast<float4*>(d.param);
    float4* g4 = reinterpret_cast<float4*>(d.grad);
    float* __restrict__ st = d.state;
    unsigned char* __restrict__ marks = d.grad_marks;
    const long n4 = d.numel / 4;                       // rows * L: a lane group is in range or out of it as a whole
    const long stride = nb * ROW_THREADS;
    const float4 zero4 = make_float4(c.zf, c.zf, c.zf, c.zf);
    // every lane of the wave runs every trip (the butterfly needs its partners); loads and stores are guarded
    for (long base = lb * ROW_THREADS; base < n4; base += NF * stride) {
        float4 P[NF], G[NF];
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            const long e = base + q * stride + threadIdx.x;
            const bool act = e < n4;
            P[q] = act ? tbl_ld<true>(p4 + e) : zero4;
            G[q] = zero4;
            if constexpr (MARKED) {
                if (act && marks[e]) { G[q] = g4[e]; g4[e] = zero4; marks[e] = 0; }
            } else {
                if (act) G[q] = tbl_ld<true>(g4 + e);
            }
        }
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            const long e = base + q * stride + threadIdx.x;
            const bool act = e < n4;
            float4 gp;
            double S = rw_chunk(P[q], G[q], c.g2, gp, sq);
#pragma unroll
            for (int o = 1; o < L; o <<= 1) S += __shfl_xor(S, o);      // chunk sums: neighbouring pairs first (opt_math.h)
            const long row = e / L;
            const float s1 = rw_acc(act ? st[row] : 0.f, S, D);
            if (act && (e & (L - 1)) == 0) st[row] = s1;
            rw_apply(P[q], gp, sqrtf(s1) + c.eps, c.nlr);
            if (act) tbl_st<true>(p4 + e, P[q]);
        }
    }
}

// ---- rows: marks and l2m == 0.  One thread per row; an unmarked chunk is not read, a row without a marked chunk not at all.
template <int L>
__device__ __forceinline__ void rw_rows(const RowDev& d, const RowCtx& c, long tid, long stride, float& sq) {
    constexpr int D = 4 * L;
    float4* p4 = reinterpret_cast<float4*>(d.param);
    float4* g4 = reinterpret_cast<float4*>(d.grad);
    float* __restrict__ st = d.state;
    unsigned char* __restrict__ marks = d.grad_marks;
    const long rows = d.numel / D;
    const float4 zero4 = make_float4(c.zf, c.zf, c.zf, c.zf);
    for (long r = tid; r < rows; r += stride) {
        unsigned char k[L];
        unsigned any = 0;
#pragma unroll
        for (int j = 0; j < L; ++j) { k[j] = marks[r * L + j]; any |= k[j]; }
        if (!any) continue;
        // (rows of more than four chunks read p and the marked g a second time for the update, from the cache, instead of
        // holding them: with p, g' and the chunk sums of a 64-wide row in registers this path set the whole kernel's occupancy)
        constexpr bool KEEP = L <= 4;
        float4 P[KEEP ? L : 1], GP[KEEP ? L : 1];
        double S[L];
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const long e = r * L + j;
            const float4 pa = p4[e];
            float4 gp;
            S[j] = rw_chunk(pa, k[j] ? g4[e] : zero4, c.g2, gp, sq);
            if constexpr (KEEP) { P[j] = pa; GP[j] = gp; }
        }
#pragma unroll
        for (int o = 1; o < L; o <<= 1)
#pragma unroll
            for (int j = 0; j < L; j += 2 * o) S[j] += S[j + o];
        const float s1 = rw_acc(st[r], S[0], D);
        st[r] = s1;
        const float den = sqrtf(s1) + c.eps;
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const long e = r * L + j;
            float4 pa, gp;
            if constexpr (KEEP) { pa = P[j]; gp = GP[j]; }
            else { float unused = 0.f; pa = p4[e]; rw_chunk(pa, k[j] ? g4[e] : zero4, c.g2, gp, unused); }
            if (k[j]) { g4[e] = zero4; marks[e] = 0; }
            rw_apply(pa, gp, den, c.nlr);
            p4[e] = pa;
        }
    }
}

// ---- units: any D, any alignment, scalar accesses.  A unit is four consecutive rows (D chunks); the tail rows are one more.
__device__ __forceinline__ void rw_units(const RowDev& d, const RowCtx& c, const OptHyper& hyp, long tid, long stride, float& sq) {
    float* __restrict__ p = d.param;
    float* __restrict__ g = d.grad;
    float* __restrict__ st = d.state;
    unsigned char* __restrict__ marks = d.grad_marks;
    const int D = d.dim;
    const long rows = d.numel / D;
    const long whole = rows / 4, units = whole + (rows % 4 ? 1 : 0);
    const int C = (D + 3) / 4;                         // chunk sums per row, padded with zeros to the next power of two
    int Cp = 1;
    while (Cp < C) Cp <<= 1;
    for (long u = tid; u < units; u += stride) {
        const long r0 = 4 * u;
        const int nr = u < whole ? 4 : (int)(rows - r0);
        const bool by_marks = marks && u < whole;      // the tail rows are always read
        // the gradient of element e: an unmarked chunk is not read and enters as the opaque zero
        auto grad_of = [&](long e) { return by_marks && !marks[e >> 2] ? c.zf : g[e]; };
        for (int rr = 0; rr < nr; ++rr) {
            const long r = r0 + rr, e0 = r * D;
            if (by_marks && d.l2 == 0.f) {             // no L2 term: a row none of whose chunks is marked keeps its bits
                unsigned any = 0;
                for (long k = e0 >> 2; k <= (e0 + D - 1) >> 2; ++k) any |= marks[k];
                if (!any) continue;
            }
            if (D == 1) {                              // Adagrad itself: its element update, not a second spelling
                float pa = p[e0], sa = st[r];
                opt_one<OPT_ADAGRAD>(pa, sa, grad_of(e0), c.g2, c.nlr, hyp, sq);
                p[e0] = pa; st[r] = sa;
                continue;
            }
            double stk[RW_LEVELS + 1], S = 0.0;
            for (int j = 0; j < Cp; ++j) {
                double acc = 0.0;
                if (j < C) {
                    const int hi = 4 * j + 4 < D ? 4 * j + 4 : D;
                    for (int k = 4 * j; k < hi; ++k) {
                        const float pa = p[e0 + k];
                        acc = rw_sq(acc, rw_gp(pa, grad_of(e0 + k), c.g2, sq));
                    }
                }
                // neighbouring pairs first: chunk j closes every level whose bit is set in j
#pragma unroll
                for (int lv = 0; lv <= RW_LEVELS; ++lv) {
                    if (!((j >> lv) & 1)) { stk[lv] = acc; break; }
                    acc = rw_add(stk[lv], acc);
                }
                S = acc;
            }
            const float s1 = rw_acc(st[r], S, D);
            st[r] = s1;
            const float den = sqrtf(s1) + c.eps;
            float unused = 0.f;
            for (int k = 0; k < D; ++k) {
                const float pa = p[e0 + k];
                p[e0 + k] = rw_one(pa, rw_gp(pa, grad_of(e0 + k), c.g2, unused), den, c.nlr);
            }
        }
        if (by_marks) {                                // the unit's D chunks: whole, and this thread's alone
            float4* g4 = reinterpret_cast<float4*>(g);
            const float4 zero4 = make_float4(c.zf, c.zf, c.zf, c.zf);
            for (long k = u * D; k < (u + 1) * D; ++k)
                if (marks[k]) { g4[k] = zero4; marks[k] = 0; }
        } else if (marks) {
            for (long e = r0 * D; e < d.numel; ++e) { g[e] = 0.f; marks[e >> 2] = 0; }
        }
    }
}

template <int L>
__device__ __forceinline__ void rw_hot(const RowDev& d, const RowCtx& c, long lb, long nb, float& sq) {
    if (d.grad_marks && d.l2 == 0.f) rw_rows<L>(d, c, lb * ROW_THREADS + threadIdx.x, nb * ROW_THREADS, sq);
    else if (d.grad_marks) rw_lanes<L, true>(d, c, lb, nb, sq);
    else rw_lanes<L, false>(d, c, lb, nb, sq);
}

__global__ __launch_bounds__(ROW_THREADS) void rowwise_adagrad_kernel(const RowBatch batch, int cnt, int slot0, double lr_arg,
                                                                      const double* __restrict__ lr_dev, const OptHyper hyp,
                                                                      float* __restrict__ l2_part) {
    // the learning rate as a kernel argument, or read from device memory (a captured HIP graph follows a schedule)
    const float nlr = -(float)(lr_dev ? *lr_dev : lr_arg);
    int ti = 0;                                        // wave-uniform search
    for (int k = 1; k < cnt; ++k) ti += (int)blockIdx.x >= batch.first[k] ? 1 : 0;
    const long lb = (int)blockIdx.x - batch.first[ti]; // this block among the tensor's nb blocks
    const long nb = batch.first[ti + 1] - batch.first[ti];
    const RowDev& d = batch.t[ti];
    // an opaque zero, as in K7: the gradient of an unmarked chunk enters the same instruction sequence as a loaded one
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const RowCtx c = {2.f * d.l2, nlr, hyp.eps, zf};   // d(l2m * w^2)/dw = 2 l2m w
    float sq = 0.f;
    const bool vec = ((((size_t)d.param) | ((size_t)d.grad)) & 15) == 0;
    const int D = d.dim;
    if (vec && D == 4) rw_hot<1>(d, c, lb, nb, sq);
    else if (vec && D == 8) rw_hot<2>(d, c, lb, nb, sq);
    else if (vec && D == 16) rw_hot<4>(d, c, lb, nb, sq);
    else if (vec && D == 32) rw_hot<8>(d, c, lb, nb, sq);
    else if (vec && D == 64) rw_hot<16>(d, c, lb, nb, sq);
    else rw_units(d, c, hyp, lb * ROW_THREADS + threadIdx.x, nb * ROW_THREADS, sq);
    tbl_l2_slot<ROW_THREADS>(sq, d.l2, l2_part, slot0 + (int)blockIdx.x);
}

extern "C" {

int xdfm_rowwise_adagrad_step(const xdfm_rowwise_tensor* tensors, int T, double lr, const double* lr_dev, double eps,
                              float* l2_ws, float* l2_value, void* stream) {
    const char* what = "rowwise_adagrad_step";
    if (int rc = tbl_check_call(what, tensors, T)) return rc;
    // (negated comparisons: a NaN is refused too)
    XDFM_REQUIRE(lr >= 0, "%s: bad hyper-parameters (lr %g is negative)", what, lr);
    XDFM_REQUIRE(eps > 0, "%s: bad hyper-parameters (eps %g is not above 0)", what, eps);
    if (int rc = tbl_check_l2(what, l2_ws, l2_value)) return rc;
    for (int t = 0; t < T; ++t) {
        const xdfm_rowwise_tensor& x = tensors[t];
        XDFM_REQUIRE(x.param && x.grad && x.state, "%s: tensor %d has a null pointer (%s)", what, t,
                     !x.param ? "param" : !x.grad ? "grad" : "state");
        XDFM_REQUIRE(x.rows >= 0, "%s: tensor %d has a negative row count %ld", what, t, x.rows);
        XDFM_REQUIRE(x.dim >= 1 && x.dim <= XDFM_ROWWISE_MAX_DIM, "%s: tensor %d has dim %d outside [1, %d]", what, t, x.dim,
                     XDFM_ROWWISE_MAX_DIM);
        XDFM_REQUIRE(x.l2 >= 0, "%s: tensor %d has a negative l2 %g", what, t, (double)x.l2);
        XDFM_REQUIRE(((size_t)x.state & 3) == 0, "%s: tensor %d has a misaligned state (%p: not 4-byte aligned)", what, t,
                     (void*)x.state);
        XDFM_REQUIRE(!x.grad_marks || ((((size_t)x.param) | ((size_t)x.grad)) & 15) == 0,
                     "%s: tensor %d has grad_marks but a pointer that is not 16-byte aligned (param %p, grad %p)", what, t,
                     (void*)x.param, (void*)x.grad);
    }
    hipStream_t st = (hipStream_t)stream;
    // Launch composition as K7 (table_step.h), by the tensors' element counts; option "opt_bx" caps the blocks per tensor (tests)
    std::vector<RowDev> devs(T);
    for (int t = 0; t < T; ++t) {
        const xdfm_rowwise_tensor& x = tensors[t];
        devs[t] = RowDev{x.param, x.grad, x.state, x.grad_marks, x.rows * (long)x.dim, x.dim, x.l2};
    }
    const int slots = tbl_step_launches<RowBatch>(
        devs.data(), T, [](const RowDev& d) { return d; }, ROW_BLOCK_ELEMS, opt_bx_cap(ROW_BX),
        [&](const RowBatch& batch, int cnt, int slot0, int) {
            hipLaunchKernelGGL(rowwise_adagrad_kernel, dim3(batch.first[cnt]), dim3(ROW_THREADS), 0, st, batch, cnt, slot0, lr, lr_dev,
                               opt_hyper(OPT_ADAGRAD, eps, 0.0), l2_value ? l2_ws : nullptr);
        });
    if (l2_value)
        if (int rc = xdfm_adam_l2_finish(l2_ws, slots, l2_value, st)) return rc;
    return xdfm_check_launch(what);
}

}  // extern "C"
