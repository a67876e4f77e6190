// K7f: the per-coordinate FTRL-Proximal step (McMahan et al., "Ad click prediction: a view from the trenches", 2013; lr_power
// -0.5) over all parameters -- the streaming sweep of K7s / K7g / K7r / K7m (sgd_adagrad.hip) for an optimizer with TWO state
// arrays.  It has a translation unit and a descriptor (xdfm_ftrl_tensor: z and n beside p) of its own; its kernel is the one
// sweep of table_step.h (tbl_sweep) under a rule that names the two arrays and forwards to the element update (opt_math.h:
// ftrl_one, the one spelling of the arithmetic).  Shared with the other steps as well: the launch composition (tbl_launches),
// the block cap (option "opt_bx"), the workspace size (xdfm_opt_step_ws_elems) and the L2 finish (xdfm_adam_l2_finish: a job
// of the open finish batch, else its own launch).
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

typedef SweepDev<2> FtrlDev;                // param, grad, z, n, grad_marks, numel, l2
typedef SweepBatch<2, FTRL_CHUNK> FtrlBatch;
static_assert(sizeof(FtrlDev) == 56 && sizeof(FtrlBatch) + 128 <= 4096, "the FTRL kernel's argument block");

// The sweep's rule (table_step.h: tbl_sweep): z and n beside p; an unmarked chunk of a tensor without a model L2 term has
// g' == 0 and keeps its bits (ftrl_one's zero-gradient rule), so it is skipped
struct FtrlRule {
    static constexpr int NS = 2, NF = FTRL_NF;
    static constexpr bool SKIP = true;
    struct Ctx { float lr; const FtrlHyper& hyp; };
    static __device__ __forceinline__ void four(float4& p, float4 (&s)[2], const float4& g, float g2, const Ctx& c, float& sq) {
        ftrl_four(p, s[0], s[1], g, g2, c.lr, c.hyp, sq);
    }
    static __device__ __forceinline__ void one(float& p, float (&s)[2], float g, float g2, const Ctx& c, float& sq) {
        ftrl_one(p, s[0], s[1], g, g2, c.lr, c.hyp, sq);
    }
};

__global__ __launch_bounds__(FTRL_THREADS) void ftrl_step_kernel(const FtrlBatch batch, int cnt, int slot0, double lr_arg,
                                                                 const double* __restrict__ lr_dev, const FtrlHyper hyp,
                                                                 float* __restrict__ l2_part) {
    // the learning rate as a kernel argument, or read from device memory (a captured HIP graph follows a schedule)
    const float lr = (float)(lr_dev ? *lr_dev : lr_arg);
    tbl_sweep<FtrlRule, FTRL_THREADS>(batch, cnt, slot0, FtrlRule::Ctx{lr, hyp}, l2_part, (int)blockIdx.x);
}

extern "C" {

int xdfm_ftrl_step(const xdfm_ftrl_tensor* tensors, int T, double lr, const double* lr_dev, double l1, double l2, double beta,
                   float* l2_ws, float* l2_value, void* stream) {
    const char* what = "ftrl_step";
    if (int rc = tbl_check_call(what, tensors, T)) return rc;
    // (negated comparisons: a NaN is refused too)
    XDFM_REQUIRE(lr > 0, "%s: bad hyper-parameters (lr %g is not above 0: the step divides by it)", what, lr);
    XDFM_REQUIRE(l1 >= 0, "%s: bad hyper-parameters (l1 %g is negative)", what, l1);
    XDFM_REQUIRE(l2 >= 0, "%s: bad hyper-parameters (l2 %g is negative)", what, l2);
    XDFM_REQUIRE(beta >= 0, "%s: bad hyper-parameters (beta %g is negative)", what, beta);
    if (int rc = tbl_check_l2(what, l2_ws, l2_value)) return rc;
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
    // Launch composition as K7 (table_step.h); option "opt_bx" caps the blocks per tensor (tests)
    const int slots = tbl_step_launches<FtrlBatch>(
        tensors, T, [](const xdfm_ftrl_tensor& x) { return FtrlDev{x.param, x.grad, {x.z, x.n}, x.grad_marks, x.numel, x.l2}; },
        FTRL_BLOCK_ELEMS, opt_bx_cap(FTRL_BX), [&](const FtrlBatch& batch, int cnt, int slot0, int) {
            hipLaunchKernelGGL(ftrl_step_kernel, dim3(batch.first[cnt]), dim3(FTRL_THREADS), 0, st, batch, cnt, slot0, lr, lr_dev,
                               ftrl_hyper(l1, l2, beta), l2_value ? l2_ws : nullptr);
        });
    if (l2_value)
        if (int rc = xdfm_adam_l2_finish(l2_ws, slots, l2_value, st)) return rc;
    return xdfm_check_launch(what);
}

}  // extern "C"
