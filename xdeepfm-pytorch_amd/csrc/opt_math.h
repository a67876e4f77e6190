// The element update of the SGD / Adagrad / RMSprop steps (K7s / K7g / K7r, sgd_adagrad.hip) and of their deferred form
// (K7sd / K7gd / K7rd, sgd_adagrad_deferred.hip): ONE definition, included by both translation units.  The deferred kernels replay the steps a
// chunk missed by calling this very function with g = 0 (an opaque zero, as the sweep's unmarked chunks do) and the rate
// the missed step used -- the bit identity of the two paths rests on there being nothing else that spells the arithmetic.
// Both units are compiled with the same flags: sqrtf and / expand to hipcc's correctly rounded sequences in either.
#pragma once
#include <hip/hip_runtime.h>
#include "xdfm_internal.h"     // xdfm_opt

// The optimizer a kernel instance is for.  SGD has no state; Adagrad's and RMSprop's `s` is the accumulator.
enum OptKind { OPT_SGD = 0, OPT_ADAGRAD = 1, OPT_RMSPROP = 2 };
// `eps` and RMSprop's decay, as floats (1 - alpha is taken in double on the host, as Python takes it)
struct OptHyper { float eps, alpha, oma; };
// eps and alpha as the kernels take them (host side)
static inline OptHyper opt_hyper(int kind, double eps, double alpha) {
    return OptHyper{kind == OPT_SGD ? 0.f : (float)eps, kind == OPT_RMSPROP ? (float)alpha : 0.f,
                    kind == OPT_RMSPROP ? (float)(1.0 - alpha) : 0.f};
}

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
    } else {
        p = fmaf(nlr, gp, p);
    }
}
template <int K>
__device__ __forceinline__ void opt_four(float4& p, float4& s, const float4& g, float g2, float nlr, const OptHyper& h, float& sq) {
    opt_one<K>(p.x, s.x, g.x, g2, nlr, h, sq); opt_one<K>(p.y, s.y, g.y, g2, nlr, h, sq);
    opt_one<K>(p.z, s.z, g.z, g2, nlr, h, sq); opt_one<K>(p.w, s.w, g.w, g2, nlr, h, sq);
}
