// Arithmetic of one Adam update (K7 / K7d), in two spellings that give THE SAME BITS:
//
//   adam_one        the reference spelling: ATen's fused-Adam sequence with IEEE sqrt and two IEEE divisions, as hipcc
//                   expands them (46 VALU instructions per element, three of them quarter-rate transcendentals).  The
//                   dense sweep is HBM-bound and uses it as it is.
//   adam_replay_pk  one step of a 16-byte chunk NO batch touched (gradient = the L2 term alone), as the deferred update
//                   replays it -- ALU-bound, 575 M elements x every step at the Criteo-card vocabulary.  It computes the
//                   same correctly rounded results with about half the issue slots: two elements per packed instruction
//                   (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32), the square root from ONE v_rsq_f32 and a coupled
//                   Newton step whose last correction rounds correctly (checked for every fp32 input, see below), the
//                   division by the step's constant sqrt(1 - beta2^t) with its exactly rounded reciprocal from the
//                   step's constant table (Markstein's correction: no transcendental, no scaling), and the general
//                   division as hipcc's own Newton chain WITHOUT v_div_scale / v_div_fmas / v_div_fixup.  Those three
//                   only act when an operand or the quotient leaves the normal range; a guard on the step's new moments
//                   (0 < v' < 2^62, 2^-50 <= |m'| < 2^30; the step's constants are range-checked by adam_tick) proves
//                   that they would not have acted, and a wave in which any lane fails the guard takes the reference
//                   spelling for that step.  So: same fused multiply-adds on the same operands -> the same bits.
//                   (adam_replay4 is the same step on a chunk held as three float4.)
//
// What a replayed step costs is what its loop issues, so the loop is kept to the arithmetic (profiles/replay_trim_probe.md:
// 95 -> 82 vector instructions per step and wave in the flush, its 14 s_nop gone): the chunk stays in six register pairs from
// step to step and both spellings end in one packed p - q, so nothing is copied; the guard compares bit patterns (3-input
// integer min / max, the four lane masks joined on the scalar unit); the two halves of the chunk run their dependent
// chains in lockstep, each the other's padding; the step's uniform constants sit in scalar registers.
//
// Verification (xdfm_adam_selftest, tests/test_gpu_host.py::test_fast_adam_replay_primitives_are_correctly_rounded; the
// flush and the catch-up against the dense sweep, bit for bit, on every path of the loop: tests/test_gpu_adam_replay_trim.py):
// the square root against sqrtf for ALL 2^32 bit patterns (through the 2^64 pre-scaling the replay uses); the division by
// a constant against IEEE division for every fp32 numerator in two binades x the constants of 300 steps; the general
// division against IEEE division on 2^32 random operand pairs inside the guard plus the guard's corners; whole replayed
// steps against adam_one on random states incl. zeros, denormals and huge values (the guard's fall-back).
#pragma once
#include <hip/hip_runtime.h>

typedef float adam_f2 __attribute__((ext_vector_type(2)));

struct AdamCoef { float w1, b2, w2, lr, eps; };

// A wave-uniform float that the compiler holds in a vector register (a kernel argument converted from double, say), moved
// to a scalar register: a packed instruction takes it as its scalar operand for both halves, where the vector copy is a
// register PAIR holding it twice -- ten registers for the five constants of a replay loop.
// (the empty assembly statement hides from the compiler that the value is uniform: it drops a readfirstlane of a value it
// knows to be uniform as a no-op and keeps the pair.  The readfirstlane itself stays the compiler's own instruction, so
// that it keeps the wait state the hardware wants between a vector write of a register and a lane read of it -- written
// inside the assembly statement it followed a v_cvt_f32_f64 of its operand directly in one kernel and read a stale value.)
__device__ __forceinline__ float adam_uniform(float x) {
    asm volatile("" : "+v"(x));
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ AdamCoef adam_uniform(const AdamCoef& c) {
    return AdamCoef{adam_uniform(c.w1), adam_uniform(c.b2), adam_uniform(c.w2), adam_uniform(c.lr), adam_uniform(c.eps)};
}

// The fusions are spelled out and the compiler's own contraction is off: left to itself it fuses differently in
// the marked and the dense loop, and the two must give the same bits.
// (in two parts: adam_one_q moves the moments and returns the amount q that leaves the weight, adam_one subtracts it --
// the replay's two spellings meet in ONE subtraction p - q, so a replay loop updates p where it stands)
__device__ __forceinline__ float adam_one_q(float g, float& m, float& v, float step_size, float bc2_sqrt, const AdamCoef& c) {
#pragma clang fp contract(off)
    m = fmaf(c.w1, g - m, m);
    v = fmaf(c.w2 * g, g, c.b2 * v);
    const float denom = sqrtf(v) / bc2_sqrt + c.eps;
    return step_size * m / denom;
}
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float step_size, float bc2_sqrt, const AdamCoef& c) {
#pragma clang fp contract(off)
    p -= adam_one_q(g, m, v, step_size, bc2_sqrt, c);
}

// One 16-byte chunk of a step with its gradient: the step's every loop, and the rows kernels, call this.  `sq` collects the
// squares of the weights BEFORE the update as (x^2 + y^2) + (z^2 + w^2) -- that association is part of the L2 value's bits --
// and g' = fma(2 l2, p, g) enters adam_one.
__device__ __forceinline__ void adam_four(float4& pa, float4& ma, float4& va, float4 ga, float g2, float step_size, float bc2_sqrt,
                                          const AdamCoef& c, float& sq) {
    sq += (pa.x * pa.x + pa.y * pa.y) + (pa.z * pa.z + pa.w * pa.w);
    ga.x = fmaf(g2, pa.x, ga.x); ga.y = fmaf(g2, pa.y, ga.y); ga.z = fmaf(g2, pa.z, ga.z); ga.w = fmaf(g2, pa.w, ga.w);
    adam_one(pa.x, ga.x, ma.x, va.x, step_size, bc2_sqrt, c); adam_one(pa.y, ga.y, ma.y, va.y, step_size, bc2_sqrt, c);
    adam_one(pa.z, ga.z, ma.z, va.z, step_size, bc2_sqrt, c); adam_one(pa.w, ga.w, ma.w, va.w, step_size, bc2_sqrt, c);
}

// Constants of one replayed step (wave-uniform; written by adam_tick_kernel into the clock's table, 4 floats per step):
//   ss   = lr / (1 - beta1^t)            bc  = sqrt(1 - beta2^t)
//   c2   = bc * 2^32                     rc2 = RN(1 / bc) * 2^-32, or 0 when the step must take the reference spelling
//                                              (a constant outside the range the guard's proof assumes)
struct AdamStepConst { float ss, bc, c2, rc2; };
#define ADAM_CONSTS_PER_STEP 4

__device__ __forceinline__ adam_f2 adam_pkfma(adam_f2 a, adam_f2 b, adam_f2 c) { return __builtin_elementwise_fma(a, b, c); }

// The short forms below come for TWO register pairs at a time -- the (x, y) and the (z, w) half of a chunk -- written in
// lockstep: a stage holds the same operation of both halves, and ADAM_LOCKSTEP() keeps the compiler's scheduler from
// moving anything across the stage's end.  Each half is one dependent chain of packed instructions, and on gfx950 a
// packed fp32 result cannot feed the very next instruction: left to itself the scheduler runs the halves one after the
// other and pads every link of the chain with an s_nop (17 of them per replayed step); in lockstep the other half's
// instruction is the padding.  The one-pair forms (the self-test calls them) are the same code on a doubled argument.
#define ADAM_LOCKSTEP() __builtin_amdgcn_sched_barrier(0)

// RN(sqrt(x)) * 2^32 for x2 = x * 2^64 (normal, > 0): one v_rsq_f32 (1 ulp), coupled Newton step on the root (s, with
// h ~ 1 / (2 s) from the same estimate), exact residual, final correction.  The correction multiplies a residual of
// about an ulp by h, so h needs a dozen good bits, not twenty-four: h0 = y / 2 serves, and its own Newton step is not
// taken.  Correct rounding checked exhaustively (xdfm_adam_selftest mode 0).
__device__ __forceinline__ void adam_sqrt_scaled2x2(adam_f2 xa, adam_f2 xb, adam_f2& oa, adam_f2& ob) {
#pragma clang fp contract(off)
    adam_f2 ya, yb;
    ya.x = __builtin_amdgcn_rsqf(xa.x);
    ya.y = __builtin_amdgcn_rsqf(xa.y);
    yb.x = __builtin_amdgcn_rsqf(xb.x);
    yb.y = __builtin_amdgcn_rsqf(xb.y);
    const adam_f2 half = {0.5f, 0.5f};
    const adam_f2 s0a = xa * ya, s0b = xb * yb, h0a = half * ya, h0b = half * yb;
    ADAM_LOCKSTEP();
    const adam_f2 ra = adam_pkfma(-s0a, h0a, half), rb = adam_pkfma(-s0b, h0b, half);
    ADAM_LOCKSTEP();
    const adam_f2 s1a = adam_pkfma(s0a, ra, s0a), s1b = adam_pkfma(s0b, rb, s0b);
    ADAM_LOCKSTEP();
    const adam_f2 dda = adam_pkfma(-s1a, s1a, xa), ddb = adam_pkfma(-s1b, s1b, xb);
    ADAM_LOCKSTEP();
    oa = adam_pkfma(dda, h0a, s1a);
    ob = adam_pkfma(ddb, h0b, s1b);
    ADAM_LOCKSTEP();
}
__device__ __forceinline__ adam_f2 adam_sqrt_scaled2(adam_f2 x2) {
    adam_f2 a, b;
    adam_sqrt_scaled2x2(x2, x2, a, b);
    return a;
}

// RN(S / bc) from s = S * 2^32, c2 = bc * 2^32, rc2 = RN(1 / bc) * 2^-32: quotient estimate and two corrections with the
// exactly rounded reciprocal (the second one is Markstein's: a faithful quotient + exact residual * RN(1/b) rounds
// correctly).  All scalings are powers of two, so every rounding is the rounding of the unscaled quantity.
__device__ __forceinline__ void adam_div_const2x2(adam_f2 sa, adam_f2 sb, float c2, float rc2, adam_f2& oa, adam_f2& ob) {
#pragma clang fp contract(off)
    const adam_f2 C = {c2, c2}, R = {rc2, rc2};
    const adam_f2 t0a = sa * R, t0b = sb * R;
    ADAM_LOCKSTEP();
    const adam_f2 r0a = adam_pkfma(-t0a, C, sa), r0b = adam_pkfma(-t0b, C, sb);
    ADAM_LOCKSTEP();
    const adam_f2 t1a = adam_pkfma(r0a, R, t0a), t1b = adam_pkfma(r0b, R, t0b);
    ADAM_LOCKSTEP();
    const adam_f2 r1a = adam_pkfma(-t1a, C, sa), r1b = adam_pkfma(-t1b, C, sb);
    ADAM_LOCKSTEP();
    oa = adam_pkfma(r1a, R, t1a);
    ob = adam_pkfma(r1b, R, t1b);
    ADAM_LOCKSTEP();
}
__device__ __forceinline__ adam_f2 adam_div_const2(adam_f2 s, float c2, float rc2) {
    adam_f2 a, b;
    adam_div_const2x2(s, s, c2, rc2, a, b);
    return b;
}

// RN(n / d): hipcc's expansion of an fp32 division on gfx950 (v_rcp_f32, one Newton step on the reciprocal, quotient, two
// residual corrections) without v_div_scale_f32 / v_div_fmas_f32 / v_div_fixup_f32 -- identical bits whenever those would
// not have rescaled: n == 0, or 2^-103 <= |n|, d and 1/d normal, n/d normal, exponent(n) - exponent(d) < 96.
__device__ __forceinline__ void adam_div2x2(adam_f2 na, adam_f2 nb, adam_f2 da, adam_f2 db, adam_f2& oa, adam_f2& ob) {
#pragma clang fp contract(off)
    adam_f2 y0a, y0b;
    y0a.x = __builtin_amdgcn_rcpf(da.x);
    y0a.y = __builtin_amdgcn_rcpf(da.y);
    y0b.x = __builtin_amdgcn_rcpf(db.x);
    y0b.y = __builtin_amdgcn_rcpf(db.y);
    const adam_f2 one = {1.f, 1.f};
    const adam_f2 ea = adam_pkfma(-da, y0a, one), eb = adam_pkfma(-db, y0b, one);
    ADAM_LOCKSTEP();
    const adam_f2 y1a = adam_pkfma(ea, y0a, y0a), y1b = adam_pkfma(eb, y0b, y0b);
    ADAM_LOCKSTEP();
    const adam_f2 q0a = na * y1a, q0b = nb * y1b;
    ADAM_LOCKSTEP();
    const adam_f2 r0a = adam_pkfma(-da, q0a, na), r0b = adam_pkfma(-db, q0b, nb);
    ADAM_LOCKSTEP();
    const adam_f2 q1a = adam_pkfma(r0a, y1a, q0a), q1b = adam_pkfma(r0b, y1b, q0b);
    ADAM_LOCKSTEP();
    const adam_f2 r1a = adam_pkfma(-da, q1a, na), r1b = adam_pkfma(-db, q1b, nb);
    ADAM_LOCKSTEP();
    oa = adam_pkfma(r1a, y1a, q1a);
    ob = adam_pkfma(r1b, y1b, q1b);
    ADAM_LOCKSTEP();
}
__device__ __forceinline__ adam_f2 adam_div2(adam_f2 n, adam_f2 d) {
    adam_f2 a, b;
    adam_div2x2(n, n, d, d, a, b);
    return a;
}

#define ADAM_V_MAX 4.611686018427388e18f      // 2^62
#define ADAM_M_MIN 8.881784197001252e-16f     // 2^-50
#define ADAM_M_MAX 1073741824.0f              // 2^30
#define ADAM_EPS_MIN 9.094947017729282e-13f   // 2^-40: the guard's proof needs d = t + eps >= 2^-40 (and eps <= 1)
// the guard's bounds as bit patterns (it compares integers, see adam_replay_pk)
#define ADAM_V_MAX_BITS 0x5e800000u           // 2^62
#define ADAM_MM_MIN_BITS 0x0d800000u          // 2^-100 = ADAM_M_MIN^2
#define ADAM_MM_MAX_BITS 0x5d800000u          // 2^60   = ADAM_M_MAX^2

// smallest / largest bit pattern of four floats, as unsigned integers (v_min3_u32 / v_max3_u32 and one more)
__device__ __forceinline__ unsigned adam_bits_min4(adam_f2 a, adam_f2 b) {
    const unsigned x = __float_as_uint(a.x), y = __float_as_uint(a.y), z = __float_as_uint(b.x), w = __float_as_uint(b.y);
    const unsigned t = x < y ? x : y, u = t < z ? t : z;
    return u < w ? u : w;
}
__device__ __forceinline__ unsigned adam_bits_max4(adam_f2 a, adam_f2 b) {
    const unsigned x = __float_as_uint(a.x), y = __float_as_uint(a.y), z = __float_as_uint(b.x), w = __float_as_uint(b.y);
    const unsigned t = x > y ? x : y, u = t > z ? t : z;
    return u > w ? u : w;
}

// One missed step of a chunk no batch touched: the gradient is the L2 term alone.  Spelled exactly like the sweep's
// update of an unmarked chunk (gradient = fmaf(2*l2, w, opaque zero)), so a replayed step gives the sweep's bits.
// The chunk travels as six register pairs -- (x, y) and (z, w) of p, m, v -- which is how the packed instructions want
// it: a replay loop keeps it in that form from step to step (adam_replay_span), and both branches below leave the new
// state in the pairs they were given, so the loop carries no copies.
// `sq2` collects the L2 VALUE of the replayed steps (x^2 + z^2, y^2 + w^2 per lane half; its total feeds a fixed-point
// accumulator that is compared at summation-noise tolerance, so its association is free).
//
// The guard (see the header comment) is  0 < v' < 2^62  and  2^-50 <= |m'| < 2^30  for all four elements, false for a NaN,
// evaluated on bit patterns: a float that is >= +0 orders like its bits, and the bits of a negative number, of -0 and of
// any NaN lie above those of every positive finite float.  So for v' the smallest pattern must be >= 1 and the largest
// below the bits of 2^62.  For m' the same is asked of the squares RN(m' m'), which carry no sign and are NaN when m' is:
// rounding is monotonic and 2^-100, 2^60 are floats, so |m'| >= 2^-50 gives RN(m'^2) >= 2^-100, and |m'| < 2^-50, i.e.
// |m'| <= 2^-50 (1 - 2^-24), gives m'^2 <= 2^-100 (1 - 2^-23 + 2^-48), which rounds to 2^-100 (1 - 2^-23); likewise at
// 2^30 / 2^60.  The predicate is the same; it costs two packed products, four 3-input min / max, and four compares whose
// lane masks meet on the scalar unit (the float min / max it replaces also let a NaN beside three good values through).
__device__ __forceinline__ void adam_replay_pk(adam_f2& pa, adam_f2& pb, adam_f2& ma, adam_f2& mb, adam_f2& va, adam_f2& vb,
                                               const AdamStepConst& k, float g2, float zf, const AdamCoef& c, adam_f2& sq2,
                                               bool eps_ok) {
#pragma clang fp contract(off)
    sq2 += adam_pkfma(pb, pb, pa * pa);
    asm volatile("" : "+v"(sq2));           // the squares are taken HERE: sunk below the update they would keep the old p alive
    const adam_f2 G2 = {g2, g2}, Z = {zf, zf}, W1 = {c.w1, c.w1}, W2 = {c.w2, c.w2}, B2 = {c.b2, c.b2};
    const adam_f2 ga = adam_pkfma(G2, pa, Z), gb = adam_pkfma(G2, pb, Z);
    const adam_f2 ma1 = adam_pkfma(W1, ga - ma, ma), mb1 = adam_pkfma(W1, gb - mb, mb);
    const adam_f2 va1 = adam_pkfma(W2 * ga, ga, B2 * va), vb1 = adam_pkfma(W2 * gb, gb, B2 * vb);
    bool fast = eps_ok && k.rc2 != 0.f;
    if (fast) {
        const adam_f2 qa = ma1 * ma1, qb = mb1 * mb1;
        const unsigned long long out = __builtin_amdgcn_ballot_w64(adam_bits_min4(va1, vb1) < 1u) |
                                       __builtin_amdgcn_ballot_w64(adam_bits_max4(va1, vb1) >= ADAM_V_MAX_BITS) |
                                       __builtin_amdgcn_ballot_w64(adam_bits_min4(qa, qb) < ADAM_MM_MIN_BITS) |
                                       __builtin_amdgcn_ballot_w64(adam_bits_max4(qa, qb) >= ADAM_MM_MAX_BITS);
        fast = out == 0;                                            // one lane outside: the whole wave takes adam_one
    }
    adam_f2 qa, qb;                                             // what leaves the weights: p' = p - q, one rounding per element
    if (fast) {
        const adam_f2 big = {18446744073709551616.f, 18446744073709551616.f};      // 2^64
        const adam_f2 E = {c.eps, c.eps}, SS = {k.ss, k.ss};
        adam_f2 sa, sb, ta, tb;
        adam_sqrt_scaled2x2(va1 * big, vb1 * big, sa, sb);
        adam_div_const2x2(sa, sb, k.c2, k.rc2, ta, tb);
        adam_div2x2(SS * ma1, SS * mb1, ta + E, tb + E, qa, qb);
        ma = ma1; mb = mb1; va = va1; vb = vb1;
    } else {
        float m0 = ma.x, m1 = ma.y, m2 = mb.x, m3 = mb.y, v0 = va.x, v1 = va.y, v2 = vb.x, v3 = vb.y;
        const float q0 = adam_one_q(ga.x, m0, v0, k.ss, k.bc, c), q1 = adam_one_q(ga.y, m1, v1, k.ss, k.bc, c);
        const float q2 = adam_one_q(gb.x, m2, v2, k.ss, k.bc, c), q3 = adam_one_q(gb.y, m3, v3, k.ss, k.bc, c);
        qa = adam_f2{q0, q1}; qb = adam_f2{q2, q3};
        ma = adam_f2{m0, m1}; mb = adam_f2{m2, m3}; va = adam_f2{v0, v1}; vb = adam_f2{v2, v3};
    }
    pa = pa - qa;
    pb = pb - qb;
}

// ... of a chunk held as three float4 (the step's mark scan replays the few steps a marked chunk misses this way)
__device__ __forceinline__ void adam_replay4(float4& p, float4& m, float4& v, const AdamStepConst& k, float g2, float zf,
                                             const AdamCoef& c, adam_f2& sq2, bool eps_ok) {
    adam_f2 pa = {p.x, p.y}, pb = {p.z, p.w}, ma = {m.x, m.y}, mb = {m.z, m.w}, va = {v.x, v.y}, vb = {v.z, v.w};
    adam_replay_pk(pa, pb, ma, mb, va, vb, k, g2, zf, c, sq2, eps_ok);
    p = make_float4(pa.x, pa.y, pb.x, pb.y);
    m = make_float4(ma.x, ma.y, mb.x, mb.y);
    v = make_float4(va.x, va.y, vb.x, vb.y);
}

__device__ __forceinline__ AdamStepConst adam_step_const(const float* __restrict__ consts, int s) {
    const float4 t = *reinterpret_cast<const float4*>(consts + ADAM_CONSTS_PER_STEP * s);
    return AdamStepConst{t.x, t.y, t.z, t.w};
}

// Steps old + 1 .. t_end of this lane's chunk; lanes with active == false take no part.  EVERY lane of the wave must reach
// the call (it starts with a wave reduction): the lanes are lined up on the step number, so that all of them replay the
// same step in the same iteration and the step's constants are four scalar registers instead of a per-lane load.
// UNIFORM_LOOP (the flush, whose every wave sits in this loop for the whole window): a wave whose active lanes all start
// from the same step -- every wave no batch touched since the last flush -- runs the steps without the per-step lane mask;
// a mixed wave masks each step by `s > old`, as every wave does without the option (the rows kernels: a second copy of
// the loop costs them registers, and their waves are mixed).
template <bool UNIFORM_LOOP = false>
__device__ __forceinline__ void adam_replay_span(float4& p, float4& m, float4& v, bool active, int old, int t_end,
                                                 const float* __restrict__ consts, float g2, float zf, const AdamCoef& c,
                                                 adam_f2& sq2, bool eps_ok) {
    int mn = active ? old : 0x7fffffff;
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(mn, o);
        mn = other < mn ? other : mn;
    }
    const int first = __builtin_amdgcn_readfirstlane(mn);
    if (first >= t_end) return;                          // also: no active lane
    adam_f2 pa = {p.x, p.y}, pb = {p.z, p.w}, ma = {m.x, m.y}, mb = {m.z, m.w}, va = {v.x, v.y}, vb = {v.z, v.w};
    if (UNIFORM_LOOP && __builtin_amdgcn_ballot_w64(active && old != first) == 0) {
        if (active)
            for (int s = first + 1; s <= t_end; ++s)
                adam_replay_pk(pa, pb, ma, mb, va, vb, adam_step_const(consts, s), g2, zf, c, sq2, eps_ok);
    } else {
        for (int s = first + 1; s <= t_end; ++s) {
            const AdamStepConst k = adam_step_const(consts, s);
            if (active && s > old) adam_replay_pk(pa, pb, ma, mb, va, vb, k, g2, zf, c, sq2, eps_ok);
        }
    }
    p = make_float4(pa.x, pa.y, pb.x, pb.y);
    m = make_float4(ma.x, ma.y, mb.x, mb.y);
    v = make_float4(va.x, va.y, vb.x, vb.y);
}

// Exactly rounded reciprocal of a normal fp32 c (host or device, one thread): the double quotient rounded to fp32 is
// RN(1/c) unless it sits within double rounding of a midpoint, so the candidate and its neighbours are compared by their
// exact residuals 1 - c*y (48-bit products: exact in double).
__host__ __device__ inline float adam_exact_rcp(float c) {
    float y = (float)(1.0 / (double)c);
    double best = fabs(1.0 - (double)c * (double)y);
    const float cand[2] = {nextafterf(y, 0.f), nextafterf(y, 3.0e38f)};
    float out = y;
    for (int k = 0; k < 2; ++k) {
        const double r = fabs(1.0 - (double)c * (double)cand[k]);
        if (r < best) { best = r; out = cand[k]; }
    }
    return out;
}
