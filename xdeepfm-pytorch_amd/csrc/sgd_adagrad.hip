// K7s / K7g / K7r / K7m: SGD (momentum 0), Adagrad (lr_decay 0), RMSprop (momentum 0, not centered) and SGD with momentum
// (K7m: dampening 0, plain or Nesterov) steps over all
// parameters -- the streaming sweep of K7 (adam.hip) for the other optimizers the trainer offers (xdftrain.py:723
// --optimizer adam|adagrad|sgd; "rmsprop" is the fourth string of deepctr/models/basemodel.py:447-461).  One kernel
// template, four instances; its body is the sweep of table_step.h (tbl_sweep), which K7f (ftrl.hip) runs under a rule of its
// own, and this file holds the rule (OptRule<K>: the state array, the chunks in flight, whether unmarked chunks may be
// skipped), the L2 finish and the entry points.
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
#include "table_step.h"    // the sweep, the call's checks and the launch loop

#define OPT_THREADS 256
#define OPT_BX 512              // most blocks one tensor gets (K7's ADAM_BX)
#define OPT_BLOCK_ELEMS 8192    // a tensor gets one block per this many elements
#define OPT_CHUNK 64            // tensors per launch: 64 descriptors of 48 bytes + first[] stay inside the 4 KB argument block

typedef SweepDev<1> OptDev;                 // param, grad, state, grad_marks, numel, l2
typedef SweepBatch<1, OPT_CHUNK> OptBatch;
static_assert(sizeof(OptDev) == 48 && sizeof(OptBatch) + 128 <= 4096, "the optimizer kernels' argument block");

// The sweep's rule for kind K (table_step.h: tbl_sweep).  SGD streams one array, the others two: eight 16-byte loads per thread
// in flight either way.
template <int K>
struct OptRule {
    static constexpr int NS = K != OPT_SGD ? 1 : 0;    // an accumulator (SGDM: the buffer) is streamed beside p
    static constexpr int NF = K != OPT_SGD ? 4 : 8;
    static constexpr bool SKIP = !OptMoves<K>::V;
    struct Ctx { float nlr; const OptHyper& hyp; };
    static __device__ __forceinline__ void four(float4& p, float4 (&s)[1], const float4& g, float g2, const Ctx& c, float& sq) {
        opt_four<K>(p, s[0], g, g2, c.nlr, c.hyp, sq);
    }
    static __device__ __forceinline__ void one(float& p, float (&s)[1], float g, float g2, const Ctx& c, float& sq) {
        opt_one<K>(p, s[0], g, g2, c.nlr, c.hyp, sq);
    }
};

template <int K>
__global__ __launch_bounds__(OPT_THREADS) void opt_step_kernel(const OptBatch batch, int cnt, int slot0, double lr_arg,
                                                               const double* __restrict__ lr_dev, const OptHyper hyp,
                                                               float* __restrict__ l2_part) {
    // the learning rate as a kernel argument, or read from device memory (a captured HIP graph follows a schedule)
    const double lr = lr_dev ? *lr_dev : lr_arg;
    tbl_sweep<OptRule<K>, OPT_THREADS>(batch, cnt, slot0, typename OptRule<K>::Ctx{-(float)lr, hyp}, l2_part, (int)blockIdx.x);
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
    if (int rc = tbl_check_call(what, tensors, T)) return rc;
    XDFM_REQUIRE(lr >= 0 && (!ADA || K == OPT_SGDM || eps > 0), "%s: bad hyper-parameters", what);
    XDFM_REQUIRE(K != OPT_RMSPROP || (alpha >= 0 && alpha < 1), "%s: bad hyper-parameters (alpha %g is outside [0, 1))", what, alpha);
    XDFM_REQUIRE(K != OPT_SGDM || (mom.mu > 0 && mom.mu < 1), "%s: bad hyper-parameters (momentum %g is outside (0, 1))", what, mom.mu);
    if (int rc = tbl_check_l2(what, l2_ws, l2_value)) return rc;
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
    // Launch composition as K7 (table_step.h); option "opt_bx" caps the blocks per tensor (tests)
    const int slots = tbl_step_launches<OptBatch>(
        tensors, T, [](const xdfm_opt_tensor& x) { return OptDev{x.param, x.grad, {x.state}, x.grad_marks, x.numel, x.l2}; },
        OPT_BLOCK_ELEMS, opt_bx_cap(OPT_BX), [&](const OptBatch& batch, int cnt, int slot0, int) {
            hipLaunchKernelGGL(opt_step_kernel<K>, dim3(batch.first[cnt]), dim3(OPT_THREADS), 0, st, batch, cnt, slot0, lr, lr_dev,
                               opt_hyper(K, eps, alpha, mom), l2_value ? l2_ws : nullptr);
        });
    if (l2_value) hipLaunchKernelGGL(opt_l2_finish_kernel, dim3(1), dim3(1024), 0, st, l2_ws, slots, l2_value);
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
