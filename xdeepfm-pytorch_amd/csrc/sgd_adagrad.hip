// K7s / K7g / K7r / K7m: SGD (momentum 0), Adagrad (lr_decay 0), RMSprop (momentum 0, not centered) and SGD with momentum
// (K7m: dampening 0, plain or Nesterov) steps over all
// parameters -- the streaming sweep of K7 (adam.hip) for the other optimizers the trainer offers (xdftrain.py:723
// --optimizer adam|adagrad|sgd; "rmsprop" is the fourth string of deepctr/models/basemodel.py:447-461).  One kernel
// template, four instances.
//
// replaces torch.optim.SGD.step() / torch.optim.Adagrad.step() plus the passes the stock path needs around them
// (zero fill of the dense table gradients, value and gradient of the L2 term).  Per parameter and step the sweep
// moves 8 bytes (SGD: p read + written) or 16 bytes (Adagrad: p and the accumulator), plus one mark byte per 16 bytes
// of gradient when the gradients live in a kept, marked buffer (xdfm_embed_scatter_bwd_marked) -- and NOTHING but
// the mark bytes for a tensor without an L2 term: an unmarked chunk has gradient 0, which leaves p and the
// accumulator as they are, so it is skipped without being read (an exact shortcut, not lazy arithmetic).
//
// Arithmetic in fp32, in the order of ATen's kernels (torch/optim/sgd.py, torch/optim/adagrad.py
// _single_tensor_adagrad; add_(alpha), addcmul_, sqrt().add_(eps), addcdiv_ whose a + alpha * b contracts into one fma):
//   g' = fma(2 l2, p, g)
//   SGD:      p = fma(-lr, g', p)
//   Adagrad:  s = s + g' g';   p = fma(-lr, g' / (sqrt(s) + eps), p)        IEEE sqrt and division
//   RMSprop:  v = fma(1 - alpha, g' g', alpha v);   p = fma(-lr, g' / (sqrt(v) + eps), p)   (torch/optim/rmsprop.py: mul_(alpha),
//             addcmul_(g, g, 1 - alpha), sqrt().add_(eps), addcdiv_).  v decays in EVERY step, so for RMSprop an unmarked chunk of
//             a tensor without an L2 term is no no-op: it is computed like any other (16 bytes per parameter), g' = 0 leaves p's bits.
//   SGDM:     buf = fma(mu, buf, g');   d = nesterov ? fma(mu, buf, g') : buf;   p = fma(-lr, d, p)   (torch/optim/sgd.py, dampening 0:
//             buf.mul_(mu).add_(g'), g'.add(buf, alpha=mu), p.add_(d, alpha=-lr); opt_math.h says where this follows ATen's rounding).
//             buf is signed state that moves p in EVERY step, so an unmarked chunk is never skipped, with or without an L2 term: RMSprop's
//             rule, and here g' = 0 does move p.  16 bytes per parameter.
// Descriptors by value in the kernel arguments, a 1-D grid shared out by tensor size, the learning rate as an argument
// or from one device double, per-block L2 partials summed in a fixed order by a finish kernel: all as K7.
#include "xdfm_internal.h"
#include "opt_math.h"      // opt_one / opt_four: the element update, shared with the deferred kernels
#include "table_step.h"    // the streaming accesses, the launch order and the grid composer, shared with K7

#define OPT_THREADS 256
#define OPT_BX 512              // most blocks one tensor gets (K7's ADAM_BX)
#define OPT_BLOCK_ELEMS 8192    // a tensor gets one block per this many elements
#define OPT_CHUNK 64            // tensors per launch: 64 descriptors of 48 bytes + first[] stay inside the 4 KB argument block

struct OptDev { float* param; float* grad; float* state; unsigned char* grad_marks; long numel; float l2; };
struct OptBatch { OptDev t[OPT_CHUNK]; int first[OPT_CHUNK + 1]; };
static_assert(sizeof(OptBatch) + 128 <= 4096, "the optimizer kernels' argument block");

// chunks per array and thread in flight: SGD streams one array, Adagrad two -- eight 16-byte loads per thread either way
template <int K> struct OptFlight { static constexpr int N = K != OPT_SGD ? 4 : 8; };

template <int K>
__global__ __launch_bounds__(OPT_THREADS) void opt_step_kernel(const OptBatch batch, int cnt, int slot0, double lr_arg,
                                                               const double* __restrict__ lr_dev, const OptHyper hyp,
                                                               float* __restrict__ l2_part) {
    constexpr int NF = OptFlight<K>::N;
    constexpr bool ADA = K != OPT_SGD;                 // an accumulator is streamed beside p
    // the learning rate as a kernel argument, or read from device memory (a captured HIP graph follows a schedule)
    const double lr = lr_dev ? *lr_dev : lr_arg;
    const float nlr = -(float)lr;
    int ti = 0;                                        // wave-uniform search
    for (int k = 1; k < cnt; ++k) ti += (int)blockIdx.x >= batch.first[k] ? 1 : 0;
    const int lb = (int)blockIdx.x - batch.first[ti];  // this block among the tensor's nb blocks
    const int nb = batch.first[ti + 1] - batch.first[ti];
    const OptDev& d = batch.t[ti];
    float* __restrict__ p = d.param;
    float* __restrict__ s = ADA ? d.state : d.param;   // SGD: never dereferenced
    float* __restrict__ g = d.grad;
    unsigned char* __restrict__ marks = d.grad_marks;
    const long n = d.numel;
    const float l2c = d.l2;
    const float g2 = 2.f * l2c;                        // d(l2 * w^2)/dw = 2 l2 w
    float sq = 0.f;
    const long tid = (long)lb * OPT_THREADS + threadIdx.x;
    const long stride = (long)nb * OPT_THREADS;
    const bool vec = ((((size_t)p) | ((size_t)s) | ((size_t)g)) & 15) == 0;
    const long n4 = vec ? n / 4 : 0;                   // unaligned tensors: everything goes through the scalar loop
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* s4 = reinterpret_cast<float4*>(s);
    float4* g4 = reinterpret_cast<float4*>(g);
    // an opaque zero, as in K7: the gradient of an unmarked chunk enters the same instruction sequence as a loaded one
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const float4 zero4 = make_float4(zf, zf, zf, zf);
    const unsigned tx = threadIdx.x, tx16 = tx * 16u;
    long i = tid;
    if (marks && l2c == 0.f && !OptMoves<K>::V) {
        // No L2 term: an unmarked chunk has g' == 0 -- p and the accumulator keep their bits, so the chunk is not read
        // at all.  (Not RMSprop: its accumulator decays to alpha * v whatever the gradient, so every chunk is a real update
        // and takes the branch below -- with g' == 0 that update leaves the bits of p as they are.  Not SGDM either: with
        // g' == 0 its buffer becomes mu * buf and still moves p.)  The scan reads the mark bytes 16 at a time (one uint4 per lane and load), two groups per thread in
        // flight; the chunks in front of the marks' first 16-byte boundary and behind the last whole group go one by one.
        auto process = [&](long e) {
            float4 pa = p4[e], sa = ADA ? s4[e] : zero4;
            const float4 ga = g4[e];
            g4[e] = zero4; marks[e] = 0;
            opt_four<K>(pa, sa, ga, g2, nlr, hyp, sq);
            p4[e] = pa;
            if constexpr (ADA) s4[e] = sa;
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
        // L2 term: every chunk is a real update (g' = 2 l2 p where the batch left no gradient).  The mark bytes are
        // loaded first and the (rare) gradient reads sit behind one branch; whole-block iterations address by a
        // wave-uniform base plus one 32-bit lane offset.
        long iu = (long)lb * OPT_THREADS;
        for (; iu + (NF - 1) * stride + OPT_THREADS <= n4; iu += NF * stride) {
            unsigned char k[NF];
            float4 P[NF], S[NF], G[NF];
            unsigned any = 0;
#pragma unroll
            for (int q = 0; q < NF; ++q) { k[q] = (marks + (iu + q * stride))[tx]; any |= k[q]; }
#pragma unroll
            for (int q = 0; q < NF; ++q) {
                P[q] = tbl_ld<true>(at4(p4 + (iu + q * stride), tx16));
                S[q] = ADA ? tbl_ld<true>(at4(s4 + (iu + q * stride), tx16)) : zero4;
                G[q] = zero4;
            }
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
            for (int q = 0; q < NF; ++q) {
                opt_four<K>(P[q], S[q], G[q], g2, nlr, hyp, sq);
                tbl_st<true>(at4(p4 + (iu + q * stride), tx16), P[q]);
                if constexpr (ADA) tbl_st<true>(at4(s4 + (iu + q * stride), tx16), S[q]);
            }
        }
        i = iu + tx;
        for (; i < n4; i += stride) {
            const unsigned char ka = marks[i];
            float4 pa = tbl_ld<true>(p4 + i), sa = ADA ? tbl_ld<true>(s4 + i) : zero4;
            float4 ga = zero4;
            if (ka) { ga = g4[i]; g4[i] = zero4; marks[i] = 0; }
            opt_four<K>(pa, sa, ga, g2, nlr, hyp, sq);
            tbl_st<true>(p4 + i, pa);
            if constexpr (ADA) tbl_st<true>(s4 + i, sa);
        }
    }
    long iu = i - tx;                                   // dense gradient, read in full and left alone
    for (; iu + (NF - 1) * stride + OPT_THREADS <= n4; iu += NF * stride) {
        float4 P[NF], S[NF], G[NF];
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            P[q] = tbl_ld<true>(at4(p4 + (iu + q * stride), tx16));
            G[q] = tbl_ld<true>(at4(g4 + (iu + q * stride), tx16));
            S[q] = ADA ? tbl_ld<true>(at4(s4 + (iu + q * stride), tx16)) : zero4;
        }
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            opt_four<K>(P[q], S[q], G[q], g2, nlr, hyp, sq);
            tbl_st<true>(at4(p4 + (iu + q * stride), tx16), P[q]);
            if constexpr (ADA) tbl_st<true>(at4(s4 + (iu + q * stride), tx16), S[q]);
        }
    }
    i = iu + tx;
    for (; i < n4; i += stride) {
        float4 pa = tbl_ld<true>(p4 + i), sa = ADA ? tbl_ld<true>(s4 + i) : zero4;
        const float4 ga = tbl_ld<true>(g4 + i);
        opt_four<K>(pa, sa, ga, g2, nlr, hyp, sq);
        tbl_st<true>(p4 + i, pa);
        if constexpr (ADA) tbl_st<true>(s4 + i, sa);
    }
    for (long k = 4 * n4 + tid; k < n; k += stride) {  // the numel % 4 tail (always read); whole unaligned tensors
        float pa = p[k], sa = ADA ? s[k] : zf;
        opt_one<K>(pa, sa, g[k], g2, nlr, hyp, sq);
        p[k] = pa;
        if constexpr (ADA) s[k] = sa;
        if (marks) { g[k] = 0.f; marks[k >> 2] = 0; }
    }
    if (l2_part) {                                     // fixed-order block reduction of the squares
        for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
        __shared__ float wsum[OPT_THREADS / 64];
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sq;
        __syncthreads();
        // one slot per block of the step, in launch order: the finish kernel adds them in that fixed order
        if (threadIdx.x == 0) l2_part[slot0 + blockIdx.x] = l2c * ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
    }
}

__global__ __launch_bounds__(1024) void opt_l2_finish_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ float acc[1024];
    float v = 0.f;
    for (int k = threadIdx.x; k < n; k += 1024) v += part[k];
    acc[threadIdx.x] = v;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = acc[0];
}

template <int K>
static int opt_step_impl(const char* what, const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, double eps,
                         double alpha, OptMom mom, float* l2_ws, float* l2_value, void* stream) {
    constexpr bool ADA = K != OPT_SGD;
    XDFM_REQUIRE(tensors, "%s: null pointer", what);
    XDFM_REQUIRE(T > 0 && T <= 65535, "%s: bad tensor count %d", what, T);
    XDFM_REQUIRE(lr >= 0 && (!ADA || K == OPT_SGDM || eps > 0), "%s: bad hyper-parameters", what);
    XDFM_REQUIRE(K != OPT_RMSPROP || (alpha >= 0 && alpha < 1), "%s: bad hyper-parameters (alpha %g is outside [0, 1))", what, alpha);
    XDFM_REQUIRE(K != OPT_SGDM || (mom.mu > 0 && mom.mu < 1), "%s: bad hyper-parameters (momentum %g is outside (0, 1))", what, mom.mu);
    XDFM_REQUIRE(!l2_value || l2_ws, "%s: l2_value needs l2_ws", what);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(tensors[t].param && tensors[t].grad && tensors[t].numel >= 0 && tensors[t].l2 >= 0,
                     "%s: tensor %d has a null pointer, a negative size or a negative l2", what, t);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(!ADA || tensors[t].state, "%s: tensor %d has no state (%s)", what, t, opt_state_name(K));
    for (int t = 0; t < T; ++t)       // a float pointer off a float boundary (checked for the new kind only: the others' calls stay as they were)
        XDFM_REQUIRE(K != OPT_SGDM || (((size_t)tensors[t].state) & 3) == 0, "%s: tensor %d has a misaligned state (%p is not 4-byte aligned)",
                     what, t, (void*)tensors[t].state);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(!tensors[t].grad_marks ||
                         ((((size_t)tensors[t].param) | ((size_t)tensors[t].grad) | (ADA ? (size_t)tensors[t].state : 0)) & 15) == 0,
                     "%s: tensor %d has grad_marks but a pointer that is not 16-byte aligned", what, t);
    hipStream_t st = (hipStream_t)stream;
    // Launch composition as K7: tensors sorted by size and dealt round-robin to the launches (tbl_launch_order)
    const int nlaunch = ceil_div(T, OPT_CHUNK);
    const std::vector<int> order = tbl_launch_order(tensors, T);
    int slot0 = 0;
    for (int l = 0; l < nlaunch; ++l) {
        OptBatch batch;
        int cnt = 0;
        for (int k = l; k < T; k += nlaunch) {
            const xdfm_opt_tensor& x = tensors[order[k]];
            batch.t[cnt++] = OptDev{x.param, x.grad, x.state, x.grad_marks, x.numel, x.l2};
        }
        tbl_grid(batch, cnt, OPT_BLOCK_ELEMS, opt_bx_cap(OPT_BX));      // option "opt_bx" caps the blocks per tensor (tests)
        hipLaunchKernelGGL(opt_step_kernel<K>, dim3(batch.first[cnt]), dim3(OPT_THREADS), 0, st, batch, cnt, slot0, lr, lr_dev,
                           opt_hyper(K, eps, alpha, mom), l2_value ? l2_ws : nullptr);
        slot0 += batch.first[cnt];
    }
    if (l2_value) hipLaunchKernelGGL(opt_l2_finish_kernel, dim3(1), dim3(1024), 0, st, l2_ws, slot0, l2_value);
    return xdfm_check_launch(what);
}

// the sweep over the tensors the deferred step (sgd_adagrad_deferred.hip) does not defer: the same launches as below
int xdfm_opt_step_dense(int kind, const char* what, const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, double eps,
                        double alpha, double mu, int nesterov, float* l2_ws, float* l2_value, void* stream) {
    return kind == OPT_SGDM      ? opt_step_impl<OPT_SGDM>(what, tensors, T, lr, lr_dev, 0.0, 0.0, OptMom{mu, nesterov}, l2_ws, l2_value, stream)
           : kind == OPT_RMSPROP ? opt_step_impl<OPT_RMSPROP>(what, tensors, T, lr, lr_dev, eps, alpha, OPT_NO_MOM, l2_ws, l2_value, stream)
           : kind == OPT_ADAGRAD ? opt_step_impl<OPT_ADAGRAD>(what, tensors, T, lr, lr_dev, eps, 0.0, OPT_NO_MOM, l2_ws, l2_value, stream)
                                 : opt_step_impl<OPT_SGD>(what, tensors, T, lr, lr_dev, 0.0, 0.0, OPT_NO_MOM, l2_ws, l2_value, stream);
}

extern "C" {

size_t xdfm_opt_step_ws_elems(int T) { return T > 0 ? (size_t)T * OPT_BX : 0; }

int xdfm_sgd_step(const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, float* l2_ws, float* l2_value,
                  void* stream) {
    return opt_step_impl<OPT_SGD>("sgd_step", tensors, T, lr, lr_dev, 0.0, 0.0, OPT_NO_MOM, l2_ws, l2_value, stream);
}

int xdfm_adagrad_step(const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, double eps, float* l2_ws,
                      float* l2_value, void* stream) {
    return opt_step_impl<OPT_ADAGRAD>("adagrad_step", tensors, T, lr, lr_dev, eps, 0.0, OPT_NO_MOM, l2_ws, l2_value, stream);
}

int xdfm_rmsprop_step(const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, double alpha, double eps,
                      float* l2_ws, float* l2_value, void* stream) {
    return opt_step_impl<OPT_RMSPROP>("rmsprop_step", tensors, T, lr, lr_dev, eps, alpha, OPT_NO_MOM, l2_ws, l2_value, stream);
}

int xdfm_sgdm_step(const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, double mu, int nesterov, float* l2_ws,
                   float* l2_value, void* stream) {
    return opt_step_impl<OPT_SGDM>("sgdm_step", tensors, T, lr, lr_dev, 0.0, 0.0, OptMom{mu, nesterov}, l2_ws, l2_value, stream);
}

}  // extern "C"
