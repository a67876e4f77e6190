// K7f: the per-coordinate FTRL-Proximal step (McMahan et al., "Ad click prediction: a view from the trenches", 2013; lr_power
// -0.5) over all parameters -- the streaming sweep of K7s / K7g / K7r / K7m (sgd_adagrad.hip) for an optimizer with TWO state
// arrays.  It has a translation unit, a descriptor (xdfm_ftrl_tensor: z and n beside p) and a kernel of its own, so the four
// instances of opt_step_kernel stay the code they were; everything around the loops is shared: the element update
// (opt_math.h: ftrl_one, the one spelling of the arithmetic), the streaming accesses, the launch order and the grid composer
// (table_step.h), the block cap (option "opt_bx"), the workspace size (xdfm_opt_step_ws_elems) and the L2 finish
// (xdfm_adam_l2_finish: a job of the open finish batch, else its own launch).
//
// Per element, in fp32 (l2m: the tensor's armed L2 strength; l1, l2, beta: the optimizer's):
//   g' = fma(2 l2m, p, g);   g' == 0: p, z, n keep their bits
//   n' = fma(g', g', n);   sigma = g' g' / (lr (sqrt(n') + sqrt(n)));   z' = fma(-sigma, p, z + g')
//   p' = |z'| <= l1 ? 0 : (sign(z') l1 - z') / ((beta + sqrt(n')) / lr + l2)
// 24 bytes per updated parameter (p, z, n read and written) plus 4 for a gradient read in full or 1/16 for its mark byte.  The
// L2 term is proximal -- inside the closed form, not in the gradient -- so a tensor without a model L2 term costs its mark
// bytes and the batch's chunks: an unmarked chunk has g' == 0 and is skipped without being read (the zero-gradient rule makes
// that exact).  With l2m > 0 every chunk is a real update.
#include "xdfm_internal.h"
#include "opt_math.h"      // ftrl_one / ftrl_four, opt_bx_cap
#include "table_step.h"
#include "finish_batch.h"  // xdfm_adam_l2_finish

#define FTRL_THREADS 256
#define FTRL_BX 512             // most blocks one tensor gets: OPT_BX, so xdfm_opt_step_ws_elems(T) holds the partials
#define FTRL_BLOCK_ELEMS 8192   // a tensor gets one block per this many elements
#define FTRL_CHUNK 64           // tensors per launch: 64 descriptors of 56 bytes + first[] stay inside the 4 KB argument block
#define FTRL_NF 4               // chunks per array and thread in flight: twelve 16-byte loads of p, z, n (sixteen with a dense gradient)

struct FtrlDev { float* param; float* grad; float* z; float* n; unsigned char* grad_marks; long numel; float l2; };
struct FtrlBatch { FtrlDev t[FTRL_CHUNK]; int first[FTRL_CHUNK + 1]; };
static_assert(sizeof(FtrlBatch) + 128 <= 4096, "the FTRL kernel's argument block");

__global__ __launch_bounds__(FTRL_THREADS) void ftrl_step_kernel(const FtrlBatch batch, int cnt, int slot0, double lr_arg,
                                                                 const double* __restrict__ lr_dev, const FtrlHyper hyp,
                                                                 float* __restrict__ l2_part) {
    constexpr int NF = FTRL_NF;
    // the learning rate as a kernel argument, or read from device memory (a captured HIP graph follows a schedule)
    const float lr = (float)(lr_dev ? *lr_dev : lr_arg);
    int ti = 0;                                        // wave-uniform search
    for (int k = 1; k < cnt; ++k) ti += (int)blockIdx.x >= batch.first[k] ? 1 : 0;
    const int lb = (int)blockIdx.x - batch.first[ti];  // this block among the tensor's nb blocks
    const int nb = batch.first[ti + 1] - batch.first[ti];
    const FtrlDev& d = batch.t[ti];
    float* __restrict__ p = d.param;
    float* __restrict__ z = d.z;
    float* __restrict__ a = d.n;
    float* __restrict__ g = d.grad;
    unsigned char* __restrict__ marks = d.grad_marks;
    const long n = d.numel;
    const float l2c = d.l2;
    const float g2 = 2.f * l2c;                        // d(l2m * w^2)/dw = 2 l2m w
    float sq = 0.f;
    const long tid = (long)lb * FTRL_THREADS + threadIdx.x;
    const long stride = (long)nb * FTRL_THREADS;
    const bool vec = ((((size_t)p) | ((size_t)z) | ((size_t)a) | ((size_t)g)) & 15) == 0;
    const long n4 = vec ? n / 4 : 0;                   // unaligned tensors: everything goes through the scalar loop
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* z4 = reinterpret_cast<float4*>(z);
    float4* a4 = reinterpret_cast<float4*>(a);
    float4* g4 = reinterpret_cast<float4*>(g);
    // an opaque zero, as in K7: the gradient of an unmarked chunk enters the same instruction sequence as a loaded one
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const float4 zero4 = make_float4(zf, zf, zf, zf);
    const unsigned tx = threadIdx.x, tx16 = tx * 16u;
    // one chunk through the cached / the streaming accesses; a block of NF chunks per thread at a wave-uniform base
    auto one = [&](long e, const float4& ga) {
        float4 pa = tbl_ld<true>(p4 + e), za = tbl_ld<true>(z4 + e), na = tbl_ld<true>(a4 + e);
        ftrl_four(pa, za, na, ga, g2, lr, hyp, sq);
        tbl_st<true>(p4 + e, pa); tbl_st<true>(z4 + e, za); tbl_st<true>(a4 + e, na);
    };
    auto load = [&](long base, float4& P, float4& Z, float4& N) {
        P = tbl_ld<true>(at4(p4 + base, tx16)); Z = tbl_ld<true>(at4(z4 + base, tx16)); N = tbl_ld<true>(at4(a4 + base, tx16));
    };
    auto update = [&](long base, float4& P, float4& Z, float4& N, const float4& G) {
        ftrl_four(P, Z, N, G, g2, lr, hyp, sq);
        tbl_st<true>(at4(p4 + base, tx16), P); tbl_st<true>(at4(z4 + base, tx16), Z); tbl_st<true>(at4(a4 + base, tx16), N);
    };
    long i = tid;
    if (marks && l2c == 0.f) {
        // No model L2 term: an unmarked chunk has g' == 0 -- p, z and n keep their bits, so the chunk is not read at all.  The
        // scan reads the mark bytes 16 at a time (one uint4 per lane and load), two groups per thread in flight; the chunks in
        // front of the marks' first 16-byte boundary and behind the last whole group go one by one.  (K7s / K7g's scan.)
        auto process = [&](long e) {
            float4 pa = p4[e], za = z4[e], na = a4[e];
            const float4 ga = g4[e];
            g4[e] = zero4; marks[e] = 0;
            ftrl_four(pa, za, na, ga, g2, lr, hyp, sq);
            p4[e] = pa; z4[e] = za; a4[e] = na;
        };
        auto group = [&](const uint4& w4, long first) {
            if (w4.x | w4.y | w4.z | w4.w) {
                const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if ((w[b >> 2] >> ((b & 3) * 8)) & 255u) process(first + b);
            }
        };
        const long lead = (16 - (long)((size_t)marks & 15)) & 15;
        const long head = lead < n4 ? lead : n4;
        const long groups = (n4 - head) / 16;
        const uint4* __restrict__ m16 = reinterpret_cast<const uint4*>(marks + head);
        long q = tid;
        for (; q + stride < groups; q += 2 * stride) {
            const uint4 wa = m16[q], wb = m16[q + stride];
            group(wa, head + q * 16);
            group(wb, head + (q + stride) * 16);
        }
        if (q < groups) group(m16[q], head + q * 16);
        for (long e = tid; e < head; e += stride)
            if (marks[e]) process(e);
        for (long e = head + groups * 16 + tid; e < n4; e += stride)
            if (marks[e]) process(e);
        i = n4 + tid;                                   // nothing left for the dense loops below
    } else if (marks) {
        // Model L2 term: every chunk is a real update (g' = 2 l2m p where the batch left no gradient).  The mark bytes are
        // loaded first and the (rare) gradient reads sit behind one branch.
        long iu = (long)lb * FTRL_THREADS;
        for (; iu + (NF - 1) * stride + FTRL_THREADS <= n4; iu += NF * stride) {
            unsigned char k[NF];
            float4 P[NF], Z[NF], N[NF], G[NF];
            unsigned any = 0;
#pragma unroll
            for (int q = 0; q < NF; ++q) { k[q] = (marks + (iu + q * stride))[tx]; any |= k[q]; }
#pragma unroll
            for (int q = 0; q < NF; ++q) { load(iu + q * stride, P[q], Z[q], N[q]); G[q] = zero4; }
            if (any) {
#pragma unroll
                for (int q = 0; q < NF; ++q)
                    if (k[q]) {
                        G[q] = *at4(g4 + (iu + q * stride), tx16);
                        *at4(g4 + (iu + q * stride), tx16) = zero4;
                        (marks + (iu + q * stride))[tx] = 0;
                    }
            }
#pragma unroll
            for (int q = 0; q < NF; ++q) update(iu + q * stride, P[q], Z[q], N[q], G[q]);
        }
        i = iu + tx;
        for (; i < n4; i += stride) {
            float4 ga = zero4;
            if (marks[i]) { ga = g4[i]; g4[i] = zero4; marks[i] = 0; }
            one(i, ga);
        }
    }
    long iu = i - tx;                                   // dense gradient, read in full and left alone
    for (; iu + (NF - 1) * stride + FTRL_THREADS <= n4; iu += NF * stride) {
        float4 P[NF], Z[NF], N[NF], G[NF];
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            load(iu + q * stride, P[q], Z[q], N[q]);
            G[q] = tbl_ld<true>(at4(g4 + (iu + q * stride), tx16));
        }
#pragma unroll
        for (int q = 0; q < NF; ++q) update(iu + q * stride, P[q], Z[q], N[q], G[q]);
    }
    i = iu + tx;
    for (; i < n4; i += stride) one(i, tbl_ld<true>(g4 + i));
    for (long k = 4 * n4 + tid; k < n; k += stride) {  // the numel % 4 tail (always read); whole unaligned tensors
        float pa = p[k], za = z[k], na = a[k];
        ftrl_one(pa, za, na, g[k], g2, lr, hyp, sq);
        p[k] = pa; z[k] = za; a[k] = na;
        if (marks) { g[k] = 0.f; marks[k >> 2] = 0; }
    }
    if (l2_part) {                                     // fixed-order block reduction of the squares
        for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
        __shared__ float wsum[FTRL_THREADS / 64];
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sq;
        __syncthreads();
        // one slot per block of the step, in launch order: the finish adds them in that fixed order
        if (threadIdx.x == 0) l2_part[slot0 + blockIdx.x] = l2c * ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
    }
}

extern "C" {

int xdfm_ftrl_step(const xdfm_ftrl_tensor* tensors, int T, double lr, const double* lr_dev, double l1, double l2, double beta,
                   float* l2_ws, float* l2_value, void* stream) {
    const char* what = "ftrl_step";
    XDFM_REQUIRE(tensors, "%s: null pointer", what);
    XDFM_REQUIRE(T > 0 && T <= 65535, "%s: bad tensor count %d", what, T);
    // (negated comparisons: a NaN is refused too)
    XDFM_REQUIRE(lr > 0, "%s: bad hyper-parameters (lr %g is not above 0: the step divides by it)", what, lr);
    XDFM_REQUIRE(l1 >= 0, "%s: bad hyper-parameters (l1 %g is negative)", what, l1);
    XDFM_REQUIRE(l2 >= 0, "%s: bad hyper-parameters (l2 %g is negative)", what, l2);
    XDFM_REQUIRE(beta >= 0, "%s: bad hyper-parameters (beta %g is negative)", what, beta);
    XDFM_REQUIRE(!l2_value || l2_ws, "%s: l2_value needs l2_ws", what);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(tensors[t].param && tensors[t].grad && tensors[t].numel >= 0 && tensors[t].l2 >= 0,
                     "%s: tensor %d has a null pointer, a negative size or a negative l2", what, t);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(tensors[t].z && tensors[t].n, "%s: tensor %d has no state (%s)", what, t, tensors[t].z ? "n" : "z");
    for (int t = 0; t < T; ++t) {
        const size_t both = ((size_t)tensors[t].z) | ((size_t)tensors[t].n);
        XDFM_REQUIRE((both & 3) == 0, "%s: tensor %d has a misaligned state (z %p, n %p: not 4-byte aligned)", what, t,
                     (void*)tensors[t].z, (void*)tensors[t].n);
        XDFM_REQUIRE(!tensors[t].grad_marks || ((((size_t)tensors[t].param) | ((size_t)tensors[t].grad) | both) & 15) == 0,
                     "%s: tensor %d has grad_marks but a pointer that is not 16-byte aligned (param %p, grad %p, z %p, n %p)", what, t,
                     (void*)tensors[t].param, (void*)tensors[t].grad, (void*)tensors[t].z, (void*)tensors[t].n);
    }
    hipStream_t st = (hipStream_t)stream;
    // Launch composition as K7: tensors sorted by size and dealt round-robin to the launches (tbl_launch_order)
    const int nlaunch = ceil_div(T, FTRL_CHUNK);
    const std::vector<int> order = tbl_launch_order(tensors, T);
    int slot0 = 0;
    for (int l = 0; l < nlaunch; ++l) {
        FtrlBatch batch;
        int cnt = 0;
        for (int k = l; k < T; k += nlaunch) {
            const xdfm_ftrl_tensor& x = tensors[order[k]];
            batch.t[cnt++] = FtrlDev{x.param, x.grad, x.z, x.n, x.grad_marks, x.numel, x.l2};
        }
        tbl_grid(batch, cnt, FTRL_BLOCK_ELEMS, opt_bx_cap(FTRL_BX));     // option "opt_bx" caps the blocks per tensor (tests)
        hipLaunchKernelGGL(ftrl_step_kernel, dim3(batch.first[cnt]), dim3(FTRL_THREADS), 0, st, batch, cnt, slot0, lr, lr_dev,
                           ftrl_hyper(l1, l2, beta), l2_value ? l2_ws : nullptr);
        slot0 += batch.first[cnt];
    }
    if (l2_value)
        if (int rc = xdfm_adam_l2_finish(l2_ws, slot0, l2_value, st)) return rc;
    return xdfm_check_launch(what);
}

}  // extern "C"
