// K7sd / K7gd / K7rd / K7md: the deferred (exact) form of the SGD, Adagrad, RMSprop and SGD-with-momentum steps for the
// embedding / linear tables (xdfm.h), K7d's scheme (adam.hip) for K7s / K7g / K7r / K7m (sgd_adagrad.hip).
//
// With an L2 term every table parameter is a real update in every step (an untouched row sees g' = 2 l2 p), so K7s / K7g
// sweep 8 / 16 bytes per table parameter and step.  An untouched chunk evolves by a recurrence in its own registers and the
// step's rate: the kernels here replay the steps a chunk missed -- opt_four with g = 0 and the rate that step used, the
// element update of the sweep itself (opt_math.h) -- when the chunk is needed:
//   opt_catchup_rows_kernel   before a batch gathers it         one thread per (example, field, chunk): latency-bound
//   opt_step_deferred_kernel  when a gradient arrives for it    a scan of the mark bytes, 16 per load: 1/16 byte per parameter
//   opt_flush_kernel          every F steps, all chunks         8 / 16 bytes per parameter, F dependent updates each: ALU-bound
// `last[chunk]` = the step (since the last flush) up to which the chunk is updated; the clock and the per-step rates live
// on the device and are advanced by the step itself, so a captured HIP graph replays all of this without the host.  The
// L2 value of the replayed steps goes to a 64-bit fixed-point cell by integer adds; there are no float atomics.
#include "xdfm_internal.h"
#include "opt_math.h"
#include "table_step.h"    // the streaming accesses and the grid composer, shared with K7 / K7d

#define OPTD_THREADS 256
#define OPTD_BX 512                 // most blocks one tensor gets in the step's scan (K7s' OPT_BX)
#define OPTD_FLUSH_BX 4096          // ... and in the flush, which wants every SIMD busy
#define OPTD_BLOCK_ELEMS 8192
#define OPTD_CHUNK 48               // tensors per launch: 48 descriptors of 56 bytes + first[] stay inside the 4 KB argument block
#define OPTD_FIX 1099511627776.0    // 2^40: fixed-point scale of the L2 cells

struct OptDefDev { float* param; float* grad; float* state; unsigned char* marks; unsigned char* last; long numel; float l2; };
struct OptDefBatch { OptDefDev t[OPTD_CHUNK]; int first[OPTD_CHUNK + 1]; };
static_assert(sizeof(OptDefBatch) + 128 <= 4096, "the deferred optimizer kernels' argument block");

__global__ void opt_tick_kernel(int* __restrict__ clock, float* __restrict__ rates, int cap, double lr_arg,
                                const double* __restrict__ lr_dev) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double lr = lr_dev ? *lr_dev : lr_arg;        // as opt_step_kernel reads it
    int t = clock[0] + 1;
    if (t >= cap) t = cap - 1;                          // the host flushes long before (defensive)
    clock[0] = t;
    rates[t] = -(float)lr;
}

__global__ void opt_clock_reset_kernel(int* __restrict__ clock) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { clock[1] += clock[0]; clock[0] = 0; }
}

// l2_value = (the sweep's value of the tensors that are not deferred, if any) + the touched chunks' share
__global__ void opt_l2_cell_finish_kernel(unsigned long long* __restrict__ cell, float* __restrict__ l2_value, int have_dense) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (l2_value) l2_value[0] = (have_dense ? l2_value[0] : 0.f) + (float)((double)(long long)cell[0] / OPTD_FIX);
        cell[0] = 0ull;
    }
}

// Block sums of two l2-weighted sums of squares in fixed point (integer adds are exact: the totals do not depend on which
// thread replayed which chunk, nor on the order of the blocks), one integer atomic per block and cell.  Every thread of
// the block calls it, once.
__device__ __forceinline__ void opt_fixed_add2(float va, unsigned long long* __restrict__ cella, float vb,
                                               unsigned long long* __restrict__ cellb) {
    long long fa = (long long)((double)va * OPTD_FIX), fb = (long long)((double)vb * OPTD_FIX);
    for (int o = 32; o > 0; o >>= 1) { fa += __shfl_xor(fa, o); fb += __shfl_xor(fb, o); }
    __shared__ long long part[2][OPTD_THREADS / 64];
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = fa; part[1][threadIdx.x >> 6] = fb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long ta = 0, tb = 0;
        for (int k = 0; k < OPTD_THREADS / 64; ++k) { ta += part[0][k]; tb += part[1][k]; }
        if (ta && cella) atomicAdd(cella, (unsigned long long)ta);
        if (tb && cellb) atomicAdd(cellb, (unsigned long long)tb);
    }
}

// smallest value of `v` over the wave, as a scalar (every lane of the wave calls it)
__device__ __forceinline__ int opt_wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o); v = w < v ? w : v; }
    return __builtin_amdgcn_readfirstlane(v);
}

// ---------------------------------------------------------------------------------------------
// the step: a scan of the mark bytes of the deferred tensors
// ---------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(OPTD_THREADS) void opt_step_deferred_kernel(const OptDefBatch batch, int cnt, const int* __restrict__ clock,
                                                                         const float* __restrict__ rates, const OptHyper hyp,
                                                                         unsigned long long* __restrict__ backlog,
                                                                         unsigned long long* __restrict__ cell) {
    constexpr bool ADA = K != OPT_SGD;                 // an accumulator goes with p
    int ti = 0;                                        // wave-uniform search
    for (int k = 1; k < cnt; ++k) ti += (int)blockIdx.x >= batch.first[k] ? 1 : 0;
    const int lb = (int)blockIdx.x - batch.first[ti];
    const int nb = batch.first[ti + 1] - batch.first[ti];
    const OptDefDev& d = batch.t[ti];
    const int t = clock[0];                            // this step (opt_tick_kernel ran in front of this launch)
    const float nlr = rates[t];
    float* __restrict__ p = d.param;
    float* __restrict__ s = ADA ? d.state : d.param;   // SGD: never dereferenced
    float* __restrict__ g = d.grad;
    unsigned char* __restrict__ marks = d.marks;
    unsigned char* __restrict__ last = d.last;
    const long n = d.numel;
    const long n4 = n / 4;
    const float l2c = d.l2;
    const float g2 = 2.f * l2c;
    float sq = 0.f, sqr = 0.f;                         // squares of this step's / of the replayed steps' weights
    const long tid = (long)lb * OPTD_THREADS + threadIdx.x;
    const long stride = (long)nb * OPTD_THREADS;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* s4 = reinterpret_cast<float4*>(s);
    float4* g4 = reinterpret_cast<float4*>(g);
    // an opaque zero, as in K7s: the gradient of a replayed step enters the same instruction sequence as a loaded one
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const float4 zero4 = make_float4(zf, zf, zf, zf);
    auto process = [&](long e) {
        float4 pa = p4[e], sa = ADA ? s4[e] : zero4;
        const float4 ga = g4[e];
        g4[e] = zero4; marks[e] = 0;
        for (int st = (int)last[e] + 1; st < t; ++st)   // steps the catch-up did not bring (rows no gather announced)
            opt_four<K>(pa, sa, zero4, g2, rates[st], hyp, sqr);
        opt_four<K>(pa, sa, ga, g2, nlr, hyp, sq);
        p4[e] = pa;
        if constexpr (ADA) s4[e] = sa;
        last[e] = (unsigned char)t;
    };
    // the marked chunks of one group of 16 mark bytes: a loop over the set bits (one copy of `process`, not sixteen)
    auto group = [&](const uint4& w4, long first) {
        const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
        unsigned set = 0;
#pragma unroll
        for (int b = 0; b < 16; ++b) set |= ((w[b >> 2] >> ((b & 3) * 8)) & 255u) ? 1u << b : 0u;
        while (set) {
            const int b = __builtin_ctz(set);
            set &= set - 1;
            process(first + b);
        }
    };
    // the mark bytes 16 at a time (one uint4 per lane and load), the next group's load in flight while this one is looked
    // at; the chunks in front of the marks' first 16-byte boundary and behind the last whole group go one by one
    const long lead = (16 - (long)((size_t)marks & 15)) & 15;
    const long head = lead < n4 ? lead : n4;
    const long groups = (n4 - head) / 16;
    const uint4* __restrict__ m16 = reinterpret_cast<const uint4*>(marks + head);
    const uint4 none = make_uint4(0u, 0u, 0u, 0u);
    uint4 cur = tid < groups ? m16[tid] : none;
    for (long q = tid; q < groups; q += stride) {
        const uint4 nxt = q + stride < groups ? m16[q + stride] : none;
        if (cur.x | cur.y | cur.z | cur.w) group(cur, head + q * 16);
        cur = nxt;
    }
    const long edge = head + (n4 - head - groups * 16);         // chunks outside the whole groups: [0, head) and the last < 16
    for (long k = tid; k < edge; k += stride) {
        const long e = k < head ? k : head + groups * 16 + (k - head);
        if (marks[e]) process(e);
    }
    for (long k = 4 * n4 + tid; k < n; k += stride) {  // the numel % 4 tail: updated densely in every step, like the sweep does
        float pa = p[k], sa = ADA ? s[k] : zf;
        opt_one<K>(pa, sa, g[k], g2, nlr, hyp, sq);
        p[k] = pa;
        if constexpr (ADA) s[k] = sa;
        g[k] = 0.f; marks[k >> 2] = 0;
    }
    opt_fixed_add2(l2c * sq, cell, l2c * sqr, backlog);
}

// ---------------------------------------------------------------------------------------------
// catch-up of the rows a batch gathers
// ---------------------------------------------------------------------------------------------
struct OptRowsDev { float* const* p; float* const* s; unsigned char* const* last; const float* l2; };

template <int K>
__global__ __launch_bounds__(OPTD_THREADS) void opt_catchup_rows_kernel(
    const float* __restrict__ X, long ldx, int B, const int* __restrict__ cols, const int* __restrict__ vocab, int m, int D,
    OptRowsDev emb, OptRowsDev lin, int has_lin, const int* __restrict__ clock, const float* __restrict__ rates, const OptHyper hyp,
    unsigned long long* __restrict__ backlog) {
    constexpr bool ADA = K != OPT_SGD;
    const int t = clock[0];
    const int QE = (D + 3) / 4 + ((D & 3) ? 1 : 0);     // chunks a row of D floats can straddle
    const int QT = QE + (has_lin ? 1 : 0);
    const long idx = (long)blockIdx.x * OPTD_THREADS + threadIdx.x;
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const float4 zero4 = make_float4(zf, zf, zf, zf);
    int old = -1;
    float4 *p4 = nullptr, *s4 = nullptr;
    float l2c = 0.f;
    if (t > 0 && idx < (long)B * m * QT) {
        const int q = (int)(idx % QT);
        const long r = idx / QT;
        const int f = (int)(r % m);
        const long b = r / m;
        const int V = vocab[f];
        long id = (long)X[b * ldx + cols[f]];           // as the gather (embed.hip): truncation, clamped
        if (id < 0 || id >= V) id = id < 0 ? 0 : V - 1;
        const bool is_lin = q >= QE;
        // picked field by field (a reference chosen at run time between two kernel-argument structs goes through scratch)
        float* const* Rp = is_lin ? lin.p : emb.p;
        float* const* Rs = is_lin ? lin.s : emb.s;
        unsigned char* const* Rl = is_lin ? lin.last : emb.last;
        const float* Rl2 = is_lin ? lin.l2 : emb.l2;
        const long w = is_lin ? 1 : D;
        const long c0 = id * w / 4, c1 = (id * w + w - 1) / 4;
        const long cc = c0 + (is_lin ? 0 : q);
        const long n4 = (long)V * w / 4;                // whole chunks; the tail elements are updated densely every step
        float* base = Rp[f];                            // a null table: not deferred
        if (cc <= c1 && cc < n4 && base != nullptr) {
            // the first thread to reach the chunk in this launch claims it: CAS on the word that holds its `last` byte;
            // duplicates of an id lose the claim and skip.  The gather runs in a later launch.  This is tbl_claim
            // (table_step.h) spelled out: through the helper, hipcc compares `ob` with `t` as unsigned in the three
            // instances of this kernel, and the kernels' code is kept as it was.
            unsigned* word = reinterpret_cast<unsigned*>(Rl[f] + (cc & ~3L));
            const int sh = (int)(cc & 3) * 8;
            unsigned seen = *word;      // a plain (cached) read: stale at worst, and then the CAS below returns the current word
            while (true) {
                const int ob = (int)((seen >> sh) & 255u);
                if (ob >= t) break;
                const unsigned want = (seen & ~(255u << sh)) | ((unsigned)t << sh);
                const unsigned got = atomicCAS(word, seen, want);
                if (got == seen) { old = ob; break; }
                seen = got;
            }
            if (old >= 0) {
                p4 = reinterpret_cast<float4*>(base) + cc;
                if constexpr (ADA) s4 = reinterpret_cast<float4*>(Rs[f]) + cc;
                l2c = Rl2[f];
            }
        }
    }
    const bool act = old >= 0;
    float4 pa = zero4, sa = zero4;
    if (act) { pa = *p4; if constexpr (ADA) sa = *s4; }
    const float g2 = 2.f * l2c;
    float sqr = 0.f;
    // the wave walks the steps together (the rate is one scalar load per step); a lane joins at its chunk's first missed one
    const int lo = opt_wave_min(act ? old : t);
    for (int st = lo + 1; st <= t; ++st) {
        const float nlr = rates[st];
        float4 pn = pa, sn = sa;
        float sqn = sqr;
        opt_four<K>(pn, sn, zero4, g2, nlr, hyp, sqn);
        if (act && st > old) { pa = pn; sa = sn; sqr = sqn; }       // a select, not a branch around the arithmetic
    }
    if (act) { *p4 = pa; if constexpr (ADA) *s4 = sa; }
    opt_fixed_add2(l2c * sqr, backlog, 0.f, nullptr);
}

// ---------------------------------------------------------------------------------------------
// flush: every chunk of the deferred tensors up to the clock; `last` back to 0
// ---------------------------------------------------------------------------------------------
// chunks per thread in flight: one chunk's replay is a dependent chain per element (Adagrad: an IEEE square root and a
// division deep), so a thread carries several chunks = 4 * N independent chains through the steps.  The step is computed
// for every chunk and taken by a select (a chunk that is ahead, or a lane behind the end, keeps its registers): a branch
// per chunk would put the chunks of a thread one after the other again.  Adagrad and RMSprop carry two chunks: their square
// root and division sequences are long enough to fill the pipeline from eight chains, and more would cost registers.  SGDM
// carries p and the buffer as they do, but its element-step is three dependent fmas, as short as SGD's one, so it takes
// SGD's four (114 VGPRs, no scratch, four waves per SIMD).  Four against two has NOT been measured for it; the measured
// flush is 7.55 ms per 574 M table parameters and 64 steps (profiles/sgdm_probe.md).
template <int K> struct OptFlushFlight { static constexpr int N = K == OPT_ADAGRAD || K == OPT_RMSPROP ? 2 : 4; };

template <int K>
__global__ __launch_bounds__(OPTD_THREADS) void opt_flush_kernel(const OptDefBatch batch, int cnt, const int* __restrict__ clock,
                                                                 const float* __restrict__ rates, const OptHyper hyp,
                                                                 unsigned long long* __restrict__ backlog) {
    constexpr int NF = OptFlushFlight<K>::N;
    constexpr bool ADA = K != OPT_SGD;
    int ti = 0;
    for (int k = 1; k < cnt; ++k) ti += (int)blockIdx.x >= batch.first[k] ? 1 : 0;
    const int lb = (int)blockIdx.x - batch.first[ti];
    const int nb = batch.first[ti + 1] - batch.first[ti];
    const OptDefDev& d = batch.t[ti];
    const int t = clock[0];
    float4* p4 = reinterpret_cast<float4*>(d.param);
    float4* s4 = reinterpret_cast<float4*>(ADA ? d.state : d.param);
    unsigned char* __restrict__ last = d.last;
    const long n4 = d.numel / 4;
    const float l2c = d.l2;
    const float g2 = 2.f * l2c;
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const float4 zero4 = make_float4(zf, zf, zf, zf);
    float sqr[NF];                                      // one chain of squares per chunk in flight
#pragma unroll
    for (int q = 0; q < NF; ++q) sqr[q] = 0.f;
    const long stride = (long)nb * OPTD_THREADS;
    // whole-wave iterations (the wave walks the steps together): the lanes behind the end are masked, not absent
    for (long base = (long)lb * OPTD_THREADS; base < n4; base += NF * stride) {
        long i[NF];
        int old[NF];
        bool in[NF], act[NF];
        float4 P[NF], S[NF];
        int lo = t;
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            i[q] = base + q * stride + threadIdx.x;
            in[q] = i[q] < n4;
            old[q] = in[q] ? (int)last[i[q]] : t;
            act[q] = in[q] && old[q] < t;
            lo = old[q] < lo ? old[q] : lo;
        }
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            P[q] = zero4; S[q] = zero4;
            if (act[q]) { P[q] = tbl_ld<true>(p4 + i[q]); if constexpr (ADA) S[q] = tbl_ld<true>(s4 + i[q]); }
        }
        lo = opt_wave_min(lo);
        for (int st = lo + 1; st <= t; ++st) {
            const float nlr = rates[st];
#pragma unroll
            for (int q = 0; q < NF; ++q) {
                float4 pn = P[q], sn = S[q];
                float sqn = sqr[q];
                opt_four<K>(pn, sn, zero4, g2, nlr, hyp, sqn);
                const bool take = act[q] && st > old[q];
                P[q].x = take ? pn.x : P[q].x; P[q].y = take ? pn.y : P[q].y; P[q].z = take ? pn.z : P[q].z; P[q].w = take ? pn.w : P[q].w;
                if constexpr (ADA) { S[q].x = take ? sn.x : S[q].x; S[q].y = take ? sn.y : S[q].y; S[q].z = take ? sn.z : S[q].z; S[q].w = take ? sn.w : S[q].w; }
                sqr[q] = take ? sqn : sqr[q];
            }
        }
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            if (act[q]) { tbl_st<true>(p4 + i[q], P[q]); if constexpr (ADA) tbl_st<true>(s4 + i[q], S[q]); }
            if (in[q] && old[q]) last[i[q]] = 0;
        }
    }
    float sqt = 0.f;
#pragma unroll
    for (int q = 0; q < NF; ++q) sqt += sqr[q];
    opt_fixed_add2(l2c * sqt, backlog, 0.f, nullptr);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int opt_clock_ok(const char* what, const xdfm_opt_clock* clk) {
    XDFM_REQUIRE(clk && clk->clock && clk->rates && clk->backlog && clk->cell, "%s: bad clock (a null pointer)", what);
    XDFM_REQUIRE(clk->cap > 2 && clk->cap <= 256, "%s: bad clock (cap %d)", what, clk->cap);     // `last`: one byte per chunk
    XDFM_REQUIRE(((((size_t)clk->backlog) | ((size_t)clk->cell)) & 7) == 0, "%s: backlog and cell must be 8-byte aligned", what);
    return XDFM_OK;
}

static OptDefDev opt_def_dev(const xdfm_opt_tensor& x, unsigned char* last) {
    return OptDefDev{x.param, x.grad, x.state, x.grad_marks, last, x.numel, x.l2};
}

template <int K>
static int opt_step_deferred_impl(const char* what, const xdfm_opt_tensor* tensors, unsigned char* const* last, int T,
                                  const xdfm_opt_clock* clk, double lr, const double* lr_dev, double eps, double alpha, OptMom mom,
                                  float* l2_ws, float* l2_value, void* stream) {
    constexpr bool ADA = K != OPT_SGD;
    if (int rc = tbl_check_call(what, tensors && last, T)) return rc;
    if (int rc = opt_clock_ok(what, clk)) return rc;
    XDFM_REQUIRE(lr >= 0 && (!ADA || K == OPT_SGDM || eps > 0), "%s: bad hyper-parameters", what);
    XDFM_REQUIRE(K != OPT_RMSPROP || (alpha >= 0 && alpha < 1), "%s: bad hyper-parameters (alpha %g is outside [0, 1))", what, alpha);
    XDFM_REQUIRE(K != OPT_SGDM || (mom.mu > 0 && mom.mu < 1), "%s: bad hyper-parameters (momentum %g is outside (0, 1))", what, mom.mu);
    if (int rc = tbl_check_l2(what, l2_ws, l2_value)) return rc;
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(tensors[t].param && tensors[t].grad && tensors[t].numel >= 0 && tensors[t].l2 >= 0,
                     "%s: tensor %d has a null pointer, a negative size or a negative l2", what, t);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(!ADA || tensors[t].state, "%s: tensor %d has no state (%s)", what, t, opt_state_name(K));
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(K != OPT_SGDM || (((size_t)tensors[t].state) & 3) == 0, "%s: tensor %d has a misaligned state (%p is not 4-byte aligned)",
                     what, t, (void*)tensors[t].state);
    for (int t = 0; t < T; ++t) {
        if (!last[t]) continue;
        XDFM_REQUIRE(tensors[t].grad_marks, "%s: tensor %d is deferred but has no grad_marks", what, t);
        XDFM_REQUIRE(tensors[t].l2 > 0, "%s: tensor %d is deferred but has no L2 term (l2 == 0 is skipped exactly by the sweep)", what, t);
        XDFM_REQUIRE(((((size_t)tensors[t].param) | ((size_t)tensors[t].grad) | (ADA ? (size_t)tensors[t].state : 0)) & 15) == 0 &&
                         (((size_t)last[t]) & 3) == 0,
                     "%s: tensor %d is deferred but a pointer is not 16-byte (last: 4-byte) aligned", what, t);
    }
    hipStream_t st = (hipStream_t)stream;
    std::vector<xdfm_opt_tensor> dense;
    std::vector<int> def;
    for (int t = 0; t < T; ++t) {
        if (last[t]) def.push_back(t); else dense.push_back(tensors[t]);
    }
    hipLaunchKernelGGL(opt_tick_kernel, dim3(1), dim3(64), 0, st, clk->clock, clk->rates, clk->cap, lr, lr_dev);
    if (!dense.empty()) {                               // stepped exactly as xdfm_sgd_step / xdfm_adagrad_step step them
        if (int rc = xdfm_opt_step_dense(K, what, dense.data(), (int)dense.size(), lr, lr_dev, eps, alpha, mom.mu, mom.nesterov, l2_ws, l2_value, stream)) return rc;
    }
    auto launch = [&](const OptDefBatch& batch, int cnt, int, int) {
        hipLaunchKernelGGL(opt_step_deferred_kernel<K>, dim3(batch.first[cnt]), dim3(OPTD_THREADS), 0, st, batch, cnt, clk->clock,
                           clk->rates, opt_hyper(K, eps, alpha, mom), clk->backlog, clk->cell);
    };
    tbl_launches<OptDefBatch>(def, false, [&](int t) { return opt_def_dev(tensors[t], last[t]); }, OPTD_BLOCK_ELEMS, opt_bx_cap(OPTD_BX),
                              launch);
    hipLaunchKernelGGL(opt_l2_cell_finish_kernel, dim3(1), dim3(64), 0, st, clk->cell, l2_value, dense.empty() ? 0 : 1);
    return xdfm_check_launch(what);
}

template <int K>
static int opt_flush_impl(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk, double eps,
                          double alpha, OptMom mom, void* stream) {
    constexpr bool ADA = K != OPT_SGD;
    if (int rc = tbl_check_call("opt_flush", tensors && last, T)) return rc;
    if (int rc = opt_clock_ok("opt_flush", clk)) return rc;
    XDFM_REQUIRE(!ADA || K == OPT_SGDM || eps > 0, "opt_flush: bad hyper-parameters");
    XDFM_REQUIRE(K != OPT_RMSPROP || (alpha >= 0 && alpha < 1), "opt_flush: bad hyper-parameters (alpha %g is outside [0, 1))", alpha);
    XDFM_REQUIRE(K != OPT_SGDM || (mom.mu > 0 && mom.mu < 1), "opt_flush: bad hyper-parameters (momentum %g is outside (0, 1))", mom.mu);
    for (int t = 0; t < T; ++t) {
        XDFM_REQUIRE(tensors[t].param && tensors[t].numel >= 0 && tensors[t].l2 >= 0,
                     "opt_flush: tensor %d has a null pointer, a negative size or a negative l2", t);
        XDFM_REQUIRE(last[t], "opt_flush: tensor %d has no last", t);
        XDFM_REQUIRE(!ADA || tensors[t].state, "opt_flush: tensor %d has no state (%s)", t, opt_state_name(K));
        XDFM_REQUIRE(((((size_t)tensors[t].param) | (ADA ? (size_t)tensors[t].state : 0)) & 15) == 0,
                     "opt_flush: tensor %d has a pointer that is not 16-byte aligned", t);
    }
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](const OptDefBatch& batch, int cnt, int, int) {
        hipLaunchKernelGGL(opt_flush_kernel<K>, dim3(batch.first[cnt]), dim3(OPTD_THREADS), 0, st, batch, cnt, clk->clock, clk->rates,
                           opt_hyper(K, eps, alpha, mom), clk->backlog);
    };
    tbl_launches<OptDefBatch>(tbl_in_order(T), false, [&](int t) { return opt_def_dev(tensors[t], last[t]); }, OPTD_BLOCK_ELEMS,
                              opt_bx_cap(OPTD_FLUSH_BX), launch);
    hipLaunchKernelGGL(opt_clock_reset_kernel, dim3(1), dim3(64), 0, st, clk->clock);
    return xdfm_check_launch("opt_flush");
}

template <int K>
static int opt_catchup_impl(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D, const xdfm_opt_rows* emb,
                            const xdfm_opt_rows* lin, const xdfm_opt_clock* clk, double eps, double alpha, OptMom mom, void* stream) {
    const OptRowsDev e = {emb->param, emb->state, emb->last, emb->l2};
    const OptRowsDev l = lin ? OptRowsDev{lin->param, lin->state, lin->last, lin->l2} : e;
    const int QT = (D + 3) / 4 + ((D & 3) ? 1 : 0) + (lin ? 1 : 0);
    const long threads = (long)B * m * QT;
    hipLaunchKernelGGL(opt_catchup_rows_kernel<K>, dim3((unsigned)ceil_div(threads, (long)OPTD_THREADS)), dim3(OPTD_THREADS), 0,
                       (hipStream_t)stream, X, ldx, B, cols, vocab, m, D, e, l, lin ? 1 : 0, clk->clock, clk->rates,
                       opt_hyper(K, eps, alpha, mom), clk->backlog);
    return xdfm_check_launch("opt_catchup_rows");
}

// what xdfm_opt_catchup_rows and xdfm_rmsprop_catchup_rows check before any device work
static int opt_catchup_ok(int kind, const float* X, int B, const int* cols, const int* vocab, int m, int D, const xdfm_opt_rows* emb,
                          const xdfm_opt_rows* lin, const xdfm_opt_clock* clk, double eps, double alpha, double mu = 0.0) {
    XDFM_REQUIRE(X && cols && vocab && emb, "opt_catchup_rows: null pointer");
    if (int rc = opt_clock_ok("opt_catchup_rows", clk)) return rc;
    XDFM_REQUIRE(B > 0 && m > 0 && D > 0, "opt_catchup_rows: bad shape B=%d m=%d D=%d", B, m, D);
    XDFM_REQUIRE(emb->param && emb->last && emb->l2 && (!lin || (lin->param && lin->last && lin->l2)),
                 "opt_catchup_rows: a row table is missing");
    XDFM_REQUIRE(kind != OPT_ADAGRAD || (eps > 0 && emb->state && (!lin || lin->state)), "opt_catchup_rows: Adagrad needs state and eps > 0");
    XDFM_REQUIRE(kind != OPT_RMSPROP || (eps > 0 && emb->state && (!lin || lin->state)), "opt_catchup_rows: RMSprop needs state and eps > 0");
    XDFM_REQUIRE(kind != OPT_RMSPROP || (alpha >= 0 && alpha < 1), "opt_catchup_rows: bad hyper-parameters (alpha %g is outside [0, 1))", alpha);
    XDFM_REQUIRE(kind != OPT_SGDM || (emb->state && (!lin || lin->state)), "opt_catchup_rows: SGD with momentum needs state (the buffers)");
    XDFM_REQUIRE(kind != OPT_SGDM || (mu > 0 && mu < 1), "opt_catchup_rows: bad hyper-parameters (momentum %g is outside (0, 1))", mu);
    return XDFM_OK;
}

extern "C" {

int xdfm_sgd_step_deferred(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                           double lr, const double* lr_dev, float* l2_ws, float* l2_value, void* stream) {
    return opt_step_deferred_impl<OPT_SGD>("sgd_step_deferred", tensors, last, T, clk, lr, lr_dev, 0.0, 0.0, OPT_NO_MOM, l2_ws, l2_value, stream);
}

int xdfm_adagrad_step_deferred(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                               double lr, const double* lr_dev, double eps, float* l2_ws, float* l2_value, void* stream) {
    return opt_step_deferred_impl<OPT_ADAGRAD>("adagrad_step_deferred", tensors, last, T, clk, lr, lr_dev, eps, 0.0, OPT_NO_MOM, l2_ws, l2_value, stream);
}

int xdfm_rmsprop_step_deferred(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                               double lr, const double* lr_dev, double alpha, double eps, float* l2_ws, float* l2_value,
                               void* stream) {
    return opt_step_deferred_impl<OPT_RMSPROP>("rmsprop_step_deferred", tensors, last, T, clk, lr, lr_dev, eps, alpha, OPT_NO_MOM, l2_ws, l2_value, stream);
}

int xdfm_sgdm_step_deferred(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                            double lr, const double* lr_dev, double mu, int nesterov, float* l2_ws, float* l2_value, void* stream) {
    return opt_step_deferred_impl<OPT_SGDM>("sgdm_step_deferred", tensors, last, T, clk, lr, lr_dev, 0.0, 0.0, OptMom{mu, nesterov}, l2_ws,
                                            l2_value, stream);
}

int xdfm_opt_catchup_rows(int adagrad, const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                          const xdfm_opt_rows* emb, const xdfm_opt_rows* lin, const xdfm_opt_clock* clk, double eps,
                          void* stream) {
    if (int rc = opt_catchup_ok(adagrad ? OPT_ADAGRAD : OPT_SGD, X, B, cols, vocab, m, D, emb, lin, clk, eps, 0.0)) return rc;
    return adagrad ? opt_catchup_impl<OPT_ADAGRAD>(X, ldx, B, cols, vocab, m, D, emb, lin, clk, eps, 0.0, OPT_NO_MOM, stream)
                   : opt_catchup_impl<OPT_SGD>(X, ldx, B, cols, vocab, m, D, emb, lin, clk, 0.0, 0.0, OPT_NO_MOM, stream);
}

int xdfm_rmsprop_catchup_rows(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                              const xdfm_opt_rows* emb, const xdfm_opt_rows* lin, const xdfm_opt_clock* clk, double alpha,
                              double eps, void* stream) {
    if (int rc = opt_catchup_ok(OPT_RMSPROP, X, B, cols, vocab, m, D, emb, lin, clk, eps, alpha)) return rc;
    return opt_catchup_impl<OPT_RMSPROP>(X, ldx, B, cols, vocab, m, D, emb, lin, clk, eps, alpha, OPT_NO_MOM, stream);
}

int xdfm_sgdm_catchup_rows(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D, const xdfm_opt_rows* emb,
                           const xdfm_opt_rows* lin, const xdfm_opt_clock* clk, double mu, int nesterov, void* stream) {
    if (int rc = opt_catchup_ok(OPT_SGDM, X, B, cols, vocab, m, D, emb, lin, clk, 0.0, 0.0, mu)) return rc;
    return opt_catchup_impl<OPT_SGDM>(X, ldx, B, cols, vocab, m, D, emb, lin, clk, 0.0, 0.0, OptMom{mu, nesterov}, stream);
}

int xdfm_opt_flush(int adagrad, const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                   double eps, void* stream) {
    return adagrad ? opt_flush_impl<OPT_ADAGRAD>(tensors, last, T, clk, eps, 0.0, OPT_NO_MOM, stream)
                   : opt_flush_impl<OPT_SGD>(tensors, last, T, clk, 0.0, 0.0, OPT_NO_MOM, stream);
}

int xdfm_rmsprop_flush(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk, double alpha,
                       double eps, void* stream) {
    return opt_flush_impl<OPT_RMSPROP>(tensors, last, T, clk, eps, alpha, OPT_NO_MOM, stream);
}

int xdfm_sgdm_flush(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk, double mu, int nesterov,
                    void* stream) {
    return opt_flush_impl<OPT_SGDM>(tensors, last, T, clk, 0.0, 0.0, OptMom{mu, nesterov}, stream);
}

}  // extern "C"
