// The element update of the SGD / Adagrad / RMSprop / SGD-with-momentum steps (K7s / K7g / K7r / K7m, sgd_adagrad.hip) and of
// their deferred form (K7sd / K7gd / K7rd / K7md, sgd_adagrad_deferred.hip): ONE definition, included by both translation units.  The deferred kernels replay the steps a
// chunk missed by calling this very function with g = 0 (an opaque zero, as the sweep's unmarked chunks do) and the rate
// the missed step used -- the bit identity of the two paths rests on there being nothing else that spells the arithmetic.
// Both units are compiled with the same flags: sqrtf and / expand to hipcc's correctly rounded sequences in either.
// At the end: the element update of the FTRL-Proximal step (K7f, ftrl.hip), which has two state values and no deferred form.
#pragma once
#include <hip/hip_runtime.h>
#include "xdfm_internal.h"     // xdfm_opt

// The optimizer a kernel instance is for.  SGD has no state; Adagrad's and RMSprop's `s` is the accumulator; SGDM is SGD with
// momentum (dampening 0), plain or Nesterov, and its `s` is torch's signed `momentum_buffer`.
enum OptKind { OPT_SGD = 0, OPT_ADAGRAD = 1, OPT_RMSPROP = 2, OPT_SGDM = 3 };
// `eps` and RMSprop's decay, as floats (1 - alpha is taken in double on the host, as Python takes it); SGDM's momentum as a
// float and whether the step is Nesterov's (one value per launch: a wave-uniform select in the element update)
struct OptHyper { float eps, alpha, oma, mu; int nesterov; };
// what every kind but SGDM passes for SGDM's two
struct OptMom { double mu; int nesterov; };
static const OptMom OPT_NO_MOM = {0.0, 0};
// what a kind's `state` is, for the messages (host side)
static inline const char* opt_state_name(int kind) { return kind == OPT_SGDM ? "the momentum buffer" : "the accumulator"; }
// eps, alpha and the momentum as the kernels take them (host side)
static inline OptHyper opt_hyper(int kind, double eps, double alpha, OptMom m = OPT_NO_MOM) {
    const bool acc = kind == OPT_ADAGRAD || kind == OPT_RMSPROP;
    return OptHyper{acc ? (float)eps : 0.f, kind == OPT_RMSPROP ? (float)alpha : 0.f,
                    kind == OPT_RMSPROP ? (float)(1.0 - alpha) : 0.f, kind == OPT_SGDM ? (float)m.mu : 0.f,
                    kind == OPT_SGDM && m.nesterov ? 1 : 0};
}
// kinds whose state moves in every step whatever the gradient (RMSprop's accumulator decays, SGDM's buffer decays and moves its
// weight): an unmarked chunk of a tensor without an L2 term is no no-op for them, so the sweep's exact shortcut is off
template <int K> struct OptMoves { static constexpr bool V = K == OPT_RMSPROP || K == OPT_SGDM; };

// Most blocks one tensor gets in a launch of these kernels (host side): the kernel's built-in cap, or option "opt_bx" where it
// is in (0, built-in] -- read when the call composes its launch; the grid changes, the arithmetic and the results do not.
static inline int opt_bx_cap(int builtin) {
    const int o = xdfm_opt(OPT_OPT_BX);
    return o > 0 && o < builtin ? o : builtin;
}

// One element.  The fusions are spelled out and the compiler's own contraction is off, so that the marked, the dense, the
// scalar and the replaying loops give the same bits.  `sq` collects p^2 of the weight BEFORE the update (the L2 term's value).
template <int K>
__device__ __forceinline__ void opt_one(float& p, float& s, float g, float g2, float nlr, const OptHyper& h, float& sq) {
#pragma clang fp contract(off)
    sq = fmaf(p, p, sq);
    const float gp = fmaf(g2, p, g);
    if constexpr (K == OPT_ADAGRAD) {
        s = s + gp * gp;
        p = fmaf(nlr, gp / (sqrtf(s) + h.eps), p);
    } else if constexpr (K == OPT_RMSPROP) {
        // mul_(alpha), then addcmul_(g, g, 1 - alpha) whose a + value * (b * c) contracts into one fma; addcdiv_ as Adagrad's
        s = fmaf(h.oma, gp * gp, h.alpha * s);
        p = fmaf(nlr, gp / (sqrtf(s) + h.eps), p);
    } else if constexpr (K == OPT_SGDM) {
        // torch/optim/sgd.py with dampening 0: buf.mul_(mu).add_(g'), then g'.add(buf, alpha=mu) for Nesterov, then
        // p.add_(d, alpha=-lr).  One fma per line.  Found by one bitwise comparison on an MI355X (tools/sgd_contract_probe.py;
        // the run is recorded in profiles/sgdm_probe.md) of torch.optim.SGD's step
        // (foreach on and off, 2^20 elements, plain and Nesterov) with the eight fp32 spellings of the three lines: ATen's
        // two add(alpha=) kernels contract a + alpha * b into one fma (0 mismatches for d and p as written here, 25163 and
        // 32372 without the contraction), and mul_ / add_, two kernels, round mu * buf on its own.  So the last two lines
        // MATCH torch's bits; the first does not and cannot by contraction -- it keeps the product exact, the more accurate
        // spelling, and differs from torch's buffer by at most half an ulp of mu * buf (146398 of 2^20 elements differ).
        // tests/test_sgdm_reference.py holds both spellings to half of the float64 bars.
        s = fmaf(h.mu, s, gp);
        const float d = h.nesterov ? fmaf(h.mu, s, gp) : s;
        p = fmaf(nlr, d, p);
    } else {
        p = fmaf(nlr, gp, p);
    }
}
template <int K>
__device__ __forceinline__ void opt_four(float4& p, float4& s, const float4& g, float g2, float nlr, const OptHyper& h, float& sq) {
    opt_one<K>(p.x, s.x, g.x, g2, nlr, h, sq); opt_one<K>(p.y, s.y, g.y, g2, nlr, h, sq);
    opt_one<K>(p.z, s.z, g.z, g2, nlr, h, sq); opt_one<K>(p.w, s.w, g.w, g2, nlr, h, sq);
}

// ---------------------------------------------------------------------------------------------
// FTRL-Proximal (K7f, ftrl.hip): per-coordinate, lr_power -0.5 (McMahan et al. 2013, algorithm 1 with eta = lr / (beta + sqrt(n)))
// ---------------------------------------------------------------------------------------------
// l1, the paper's lambda_2 (it enters the denominator as it is: TensorFlow's l2_regularization_strength is half of it) and beta,
// as floats
struct FtrlHyper { float l1, l2, beta; };
static inline FtrlHyper ftrl_hyper(double l1, double l2, double beta) { return FtrlHyper{(float)l1, (float)l2, (float)beta}; }

// One element: weight p, state z and n, gradient g; `lr` > 0 (the host refuses anything else: it is a divisor).
//   sigma is the paper's (sqrt(n') - sqrt(n)) / lr written as a quotient, g'^2 / (lr (sqrt(n') + sqrt(n))): the same number
//   without the cancellation of the two roots (the difference spends 6 times the z bar of the tests, the quotient 0.1 of it).
//   An element with g' == 0 keeps the bits of p, z and n -- a select, not a product with 0: at n == 0 sigma is 0 / 0, and a
//   weight that never saw a gradient must not jump from its initial value to the closed form's 0.  So an unmarked chunk of a
//   tensor without an L2 term is skipped exactly, and marks on / off give the same bits.
__device__ __forceinline__ void ftrl_one(float& p, float& z, float& n, float g, float g2, float lr, const FtrlHyper& h, float& sq) {
#pragma clang fp contract(off)
    sq = fmaf(p, p, sq);
    const float gp = fmaf(g2, p, g);
    const float n1 = fmaf(gp, gp, n);
    // n' == 0 with g' != 0: n was 0 and g'^2 underflowed (|g'| < 2.6e-23).  The root of the exact sum is |g'| then, and the
    // quotient's numerator has underflowed with its denominator: sigma = 0 instead of 0 / 0.  Everywhere else these two selects
    // pass sqrt(n') and the quotient through.
    const float r1 = n1 > 0.f ? sqrtf(n1) : fabsf(gp), r0 = sqrtf(n);
    const float ds = lr * (r1 + r0);
    const float sigma = ds > 0.f ? (gp * gp) / ds : 0.f;
    const float z1 = fmaf(-sigma, p, z + gp);
    const float den = (h.beta + r1) / lr + h.l2;
    const float p1 = fabsf(z1) <= h.l1 ? 0.f : (copysignf(h.l1, z1) - z1) / den;
    const bool live = gp != 0.f;
    p = live ? p1 : p;
    z = live ? z1 : z;
    n = live ? n1 : n;
}
__device__ __forceinline__ void ftrl_four(float4& p, float4& z, float4& n, const float4& g, float g2, float lr, const FtrlHyper& h,
                                          float& sq) {
    ftrl_one(p.x, z.x, n.x, g.x, g2, lr, h, sq); ftrl_one(p.y, z.y, n.y, g.y, g2, lr, h, sq);
    ftrl_one(p.z, z.z, n.z, g.z, g2, lr, h, sq); ftrl_one(p.w, z.w, n.w, g.w, g2, lr, h, sq);
}

// ---------------------------------------------------------------------------------------------
// Row-wise Adagrad (K7w, rowwise.hip): one accumulator per row of a [rows, D] tensor
// ---------------------------------------------------------------------------------------------
//   g'_d = fma(2 l2m, p_d, g_d);   S = sum_d (double)g'_d (double)g'_d;   ms = (float)(S / (double)D)
//   s' = s + ms;   den = sqrtf(s') + eps;   p_d' = fma(-lr, g'_d / den, p_d)
// THE ORDER OF S, the same on every path of the kernel (the products are exact in double, so only the additions round):
//   1. the row is cut into chunks of four consecutive elements (the last one has D % 4 when that is not 0); a chunk's squares
//      are added left to right, ((x0 + x1) + x2) + x3;
//   2. the C = ceil(D / 4) chunk sums are padded with zeros to the next power of two and added as a balanced tree, neighbouring
//      pairs first: t[j] = t[2j] + t[2j + 1] until one value is left.
// The zero-gradient rule is two selects, not arithmetic on zeros: ms == 0 keeps the bits of s (s + 0 would turn a -0 into +0),
// g'_d == 0 keeps the bits of p_d (fma(-lr, -0 / den, -0) is +0).  So a row without a gradient in a tensor without an L2 term is
// skipped exactly, and marks on / off give the same bits.  A row whose squares underflow even in the mean (ms == 0 with g' != 0)
// keeps s and still moves p by lr g' / (sqrt(s) + eps): nothing divides by zero because eps > 0.
#define RW_LEVELS 8            // log2 of the most chunk sums a row has: XDFM_ROWWISE_MAX_DIM / 4 = 256
static_assert((4 << RW_LEVELS) == XDFM_ROWWISE_MAX_DIM, "RW_LEVELS follows the cap on D");

// g' of one element; `sq` collects p^2 of the weight BEFORE the update
__device__ __forceinline__ float rw_gp(float p, float g, float g2, float& sq) {
#pragma clang fp contract(off)
    sq = fmaf(p, p, sq);
    return fmaf(g2, p, g);
}
// acc + g'^2 in double (the product of two floats is exact there: an fma and a multiply-add give the same bits)
__device__ __forceinline__ double rw_sq(double acc, float gp) {
#pragma clang fp contract(off)
    return acc + (double)gp * (double)gp;
}
__device__ __forceinline__ double rw_add(double a, double b) { return a + b; }
// one chunk of four: g' into `gp`, -> the chunk's sum of squares
__device__ __forceinline__ double rw_chunk(const float4& p, const float4& g, float g2, float4& gp, float& sq) {
    gp.x = rw_gp(p.x, g.x, g2, sq); gp.y = rw_gp(p.y, g.y, g2, sq);
    gp.z = rw_gp(p.z, g.z, g2, sq); gp.w = rw_gp(p.w, g.w, g2, sq);
    return rw_sq(rw_sq(rw_sq(rw_sq(0.0, gp.x), gp.y), gp.z), gp.w);
}
// the row's accumulator after the step
__device__ __forceinline__ float rw_acc(float s, double S, int D) {
#pragma clang fp contract(off)
    const float ms = (float)(S / (double)D);
    return ms > 0.f ? s + ms : s;
}
// one element of the row, den = sqrtf(s') + eps
__device__ __forceinline__ float rw_one(float p, float gp, float den, float nlr) {
#pragma clang fp contract(off)
    return gp != 0.f ? fmaf(nlr, gp / den, p) : p;
}
__device__ __forceinline__ void rw_apply(float4& p, const float4& gp, float den, float nlr) {
    p.x = rw_one(p.x, gp.x, den, nlr); p.y = rw_one(p.y, gp.y, den, nlr);
    p.z = rw_one(p.z, gp.z, den, nlr); p.w = rw_one(p.w, gp.w, den, nlr);
}
