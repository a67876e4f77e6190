// K7: Adam step over all parameters (one launch per 64 tensors, a 1-D grid shared out by tensor size; the embedding
// tables are 98 % of the bytes).
//
// replaces torch.optim.Adam.step() for the [vocab, D] / [vocab, 1] tables (deepctr/models/basemodel.py:452
// builds torch.optim.Adam over every parameter; the reference's tables carry dense gradients,
// deepctr/inputs.py:168 sparse=False, so every row is updated every step).  44 M parameters at config 2 =
// 1.2 GB of traffic per step (p, m, v read + written, g read): pure HBM streaming, 16-byte accesses, 12-16 loads
// in flight per thread.  Arithmetic follows ATen's fused kernel (fused_adam_utils.cuh), in fp32:
//   m = m + (1 - b1) (g - m);  v = b2 v + (1 - b2) g g;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// Tensor descriptors travel BY VALUE in the kernel arguments (no device-side pointer tables to build or
// refresh, nothing to upload when a gradient moves); the step counters are the device-resident fp32 scalars
// torch keeps per parameter (already incremented by the caller).
//
// Optional L2 term (deepctr/models/basemodel.py:412-428, l2 * sum(w^2) added to the loss): with l2[t] given, the
// kernel adds its gradient 2 l2[t] w to g on the fly (w is being read anyway) and returns the term's VALUE of
// the pre-update weights (per-block partials summed in a fixed order by adam_l2_finish_kernel).  That removes
// two table-sized passes per step (sum of squares; gradient initialisation) from the train step.
#include "xdfm_internal.h"
#include "finish_batch.h"
#include "adam_math.h"
#include "cin_x3_pack.h"   // the catch-up carries the |W| maxima of the CIN weight packs as a rider
#include "table_step.h"    // the streaming accesses, the chunk claim, the mark scan, the L2 partial, the launch loop

#define ADAM_THREADS 256
#define ADAM_BX 512             // most blocks one tensor gets (tools/adam_probe.py: 128 .. 4096 are within 5 % of each other, 512 best)
#define ADAM_BLOCK_ELEMS 8192   // a tensor gets one block per this many elements: 8 float4 per thread and array
#define ADAM_FLUSH_BX 4096      // ... and in the flush, which wants every SIMD busy

// Streaming accesses (table_step.h: tbl_ld / tbl_st, non-temporal, four chunks per array and thread in flight).
// tools/ubench/stream.hip is the bare read-modify-write stream of the same shape: 6.4-7.3 TB/s while the three arrays total
// 1.9 GB, 4.4-5.5 TB/s at the 7.7 GB this step sweeps -- K7 runs at 5.0-5.5 TB/s (tools/adam_probe.py), the rate the
// memory system gives this footprint.

// ADAM_FIX (2^40), the fixed-point scale of the L2 backlog (integer adds: order-independent): finish_batch.h

#define ADAM_CHUNK 64
// first[k] = first block of tensor k in the launch's 1-D grid (first[cnt] = grid size), see tbl_grid (table_step.h)
// the descriptor as the kernels see it: 72 bytes, so that ADAM_CHUNK = 64 of them (the criteo-card step holds 51 tensors
// outside the by-rows tables: one launch instead of two 35-us launches of small, latency-bound tensors) and the other
// arguments stay inside the 8 KB the static_assert below allows for a kernel's argument block
struct AdamDev {
    float* param; float* grad; float* exp_avg; float* exp_avg_sq; const float* step; unsigned char* grad_marks; unsigned char* last;
    long numel; float l2; int flags;
};
static inline AdamDev adam_dev(const xdfm_adam_tensor& t) {
    return AdamDev{t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.step, t.grad_marks, t.last, t.numel, t.l2, t.flags};
}
struct AdamBatch { AdamDev t[ADAM_CHUNK]; int first[ADAM_CHUNK + 1]; };
static_assert(sizeof(AdamBatch) + 128 <= 8192, "the Adam kernels' argument block");

// The step's body for workgroup `bid` of the launch's 1-D grid (adam_step_kernel: every workgroup; adam_step_rows_kernel: the
// workgroups in front of the rows body's).  Inlined, so that `batch` stays in the kernel's argument block.
template <bool NT>
__device__ __forceinline__ void adam_step_body(
    const AdamBatch& batch, int cnt, int slot0, double lr_arg, const double* __restrict__ lr_dev, double beta1, double beta2, double eps,
    float* __restrict__ l2_part, const int* __restrict__ clock, const float* __restrict__ consts, const int bid) {
    // the learning rate as a kernel argument, or read from device memory (a captured HIP graph then follows a
    // learning-rate schedule without being captured again)
    const double lr = lr_dev ? *lr_dev : lr_arg;
    int ti = 0;                                        // wave-uniform search over <= ADAM_CHUNK (64) entries
    for (int k = 1; k < cnt; ++k) ti += bid >= batch.first[k] ? 1 : 0;
    const int lb = bid - batch.first[ti];  // this block among the tensor's nb blocks
    const int nb = batch.first[ti + 1] - batch.first[ti];
    const AdamDev& d = batch.t[ti];
    float* __restrict__ p = d.param;
    float* __restrict__ m = d.exp_avg;
    float* __restrict__ v = d.exp_avg_sq;
    float* __restrict__ g = d.grad;
    unsigned char* __restrict__ marks = d.grad_marks;
    const long n = d.numel;
    const float* l2 = &d.l2;
    // bias corrections in double as ATen does, once per block (two double pow() per THREAD cost more than
    // the whole update of a small tensor)
    __shared__ float bcs[2];
    if (threadIdx.x == 0) {
        const double step = (double)*d.step;
        // with a clock, adam_tick has just written this step's two constants (same formula, same doubles): take them from
        // its table when the tensor's own step counter agrees with the clock -- two double pow() cost microseconds
        const int t = clock ? clock[0] : 0;
        if (clock && step == (double)(clock[1] + t)) {
            bcs[0] = consts[ADAM_CONSTS_PER_STEP * t];
            bcs[1] = consts[ADAM_CONSTS_PER_STEP * t + 1];
        } else {
            bcs[0] = (float)(lr / (1.0 - pow(beta1, step)));
            bcs[1] = (float)sqrt(1.0 - pow(beta2, step));
        }
    }
    __syncthreads();
    const float step_size = bcs[0], bc2_sqrt = bcs[1];
    const AdamCoef c = {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)lr, (float)eps};
    const float l2c = *l2;
    const float g2 = 2.f * l2c;                        // d(l2 * w^2)/dw = 2 l2 w
    float sq = 0.f;
    adam_f2 sq2 = {0.f, 0.f};                          // squares of the replayed steps (deferred tensors)
    const bool eps_ok = c.eps >= ADAM_EPS_MIN && c.eps <= 1.f;
    const long tid = (long)lb * ADAM_THREADS + threadIdx.x;
    const long stride = (long)nb * ADAM_THREADS;
    const bool vec = ((((size_t)p) | ((size_t)m) | ((size_t)v) | ((size_t)g)) & 15) == 0;
    const long n4 = vec ? n / 4 : 0;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* g4 = reinterpret_cast<float4*>(g);
    long i = tid;
    if (marks && (d.flags & XDFM_ADAM_DEFERRED) && clock) {
        // deferred (exact) update, see xdfm.h: only chunks with a gradient are touched; a chunk that still misses earlier
        // steps (its rows were not brought up to date by xdfm_adam_catchup_rows) replays them first
        const int t = clock[0];
        unsigned char* __restrict__ last = d.last;
        float zf;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
        const float4 zero4 = make_float4(zf, zf, zf, zf);
        tbl_mark_scan(marks, n4, tid, stride, [&](long e) {        // the scan of K7s / K7f's sweep (table_step.h)
            float4 pa = p4[e], ma = m4[e], va = v4[e], ga = g4[e];
            g4[e] = zero4; marks[e] = 0;
            for (int s = (int)last[e] + 1; s < t; ++s) adam_replay4(pa, ma, va, adam_step_const(consts, s), g2, zf, c, sq2, eps_ok);
            adam_four(pa, ma, va, ga, g2, step_size, bc2_sqrt, c, sq);
            p4[e] = pa; m4[e] = ma; v4[e] = va;
            last[e] = (unsigned char)t;
        });
        i = n4 + tid;                                   // nothing left for the dense loops below
    } else if (marks && (d.flags & XDFM_ADAM_LAZY)) {
        // opt-in row-sparse update: chunks the batch did not touch are skipped altogether (see xdfm.h)
        float zf;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
        const float4 zero4 = make_float4(zf, zf, zf, zf);
        for (; i + 3 * stride < n4; i += 4 * stride) {            // 4 mark bytes in flight per thread
            unsigned char k[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) k[q] = marks[i + q * stride];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (k[q]) {
                    const long e = i + q * stride;
                    float4 pa = p4[e], ma = m4[e], va = v4[e], ga = g4[e];
                    g4[e] = zero4; marks[e] = 0;
                    adam_four(pa, ma, va, ga, g2, step_size, bc2_sqrt, c, sq);
                    p4[e] = pa; m4[e] = ma; v4[e] = va;
                }
            }
        }
        for (; i < n4; i += stride) {
            if (marks[i]) {
                float4 pa = p4[i], ma = m4[i], va = v4[i], ga = g4[i];
                g4[i] = zero4; marks[i] = 0;
                adam_four(pa, ma, va, ga, g2, step_size, bc2_sqrt, c, sq);
                p4[i] = pa; m4[i] = ma; v4[i] = va;
            }
        }
    } else if (marks) {
        // sparse gradient: a chunk's mark says whether the scatter touched it; unmarked chunks are zeros by
        // construction and are not read, marked ones are read, re-zeroed and unmarked (each lane owns its chunk's
        // mark, so nothing races).  Four chunks per array and thread in flight; the mark bytes are loaded first and
        // the (rare) gradient reads sit behind one branch, so the common iteration is a straight run of 16 loads.
        // The zero is opaque to the compiler: with a literal 0 it folds fmaf(2*l2, w, 0) into a product and then
        // contracts that product into the next subtraction, which rounds differently from the dense path -- with
        // the same instruction sequence both paths give the same bits.
        float zf;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
        const float4 zero4 = make_float4(zf, zf, zf, zf);
        // whole-block iterations: the chunk index is (wave-uniform base) + threadIdx.x, so every access is a scalar
        // base plus one 32-bit lane offset (16 per-lane 64-bit addresses would not fit the register budget)
        long iu = (long)lb * ADAM_THREADS;
        const unsigned tx = threadIdx.x, tx16 = tx * 16u;
        for (; iu + 3 * stride + ADAM_THREADS <= n4; iu += 4 * stride) {
            unsigned char k[4];
            float4 P[4], M[4], V[4], G[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) k[q] = (marks + (iu + q * stride))[tx];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                P[q] = tbl_ld<NT>(at4(p4 + (iu + q * stride), tx16)); M[q] = tbl_ld<NT>(at4(m4 + (iu + q * stride), tx16));
                V[q] = tbl_ld<NT>(at4(v4 + (iu + q * stride), tx16));
                G[q] = zero4;
            }
            if (k[0] | k[1] | k[2] | k[3]) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (k[q]) { G[q] = (*at4(g4 + (iu + q * stride), tx16)); (*at4(g4 + (iu + q * stride), tx16)) = zero4; (marks + (iu + q * stride))[tx] = 0; }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 pa = P[q], ma = M[q], va = V[q], ga = G[q];
                adam_four(pa, ma, va, ga, g2, step_size, bc2_sqrt, c, sq);
                tbl_st<NT>(at4(p4 + (iu + q * stride), tx16), pa); tbl_st<NT>(at4(m4 + (iu + q * stride), tx16), ma);
                tbl_st<NT>(at4(v4 + (iu + q * stride), tx16), va);
                __builtin_amdgcn_sched_barrier(0);       // one chunk's arithmetic at a time: its temporaries die before the next
            }
        }
        i = iu + tx;
        for (; i < n4; i += stride) {
            const unsigned char ka = marks[i];
            float4 pa = tbl_ld<NT>(p4 + i), ma = tbl_ld<NT>(m4 + i), va = tbl_ld<NT>(v4 + i);
            float4 ga = zero4;
            if (ka) { ga = g4[i]; g4[i] = zero4; marks[i] = 0; }
            adam_four(pa, ma, va, ga, g2, step_size, bc2_sqrt, c, sq);
            tbl_st<NT>(p4 + i, pa); tbl_st<NT>(m4 + i, ma); tbl_st<NT>(v4 + i, va);
        }
    }
    long iu = i - threadIdx.x;                            // dense gradient: four float4 per array in flight
    const unsigned tx = threadIdx.x, tx16 = tx * 16u;
    for (; iu + 3 * stride + ADAM_THREADS <= n4; iu += 4 * stride) {
        float4 P[4], M[4], V[4], G[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            P[q] = tbl_ld<NT>(at4(p4 + (iu + q * stride), tx16)); G[q] = tbl_ld<NT>(at4(g4 + (iu + q * stride), tx16));
            M[q] = tbl_ld<NT>(at4(m4 + (iu + q * stride), tx16)); V[q] = tbl_ld<NT>(at4(v4 + (iu + q * stride), tx16));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 pa = P[q], ma = M[q], va = V[q], ga = G[q];
            adam_four(pa, ma, va, ga, g2, step_size, bc2_sqrt, c, sq);
            tbl_st<NT>(at4(p4 + (iu + q * stride), tx16), pa); tbl_st<NT>(at4(m4 + (iu + q * stride), tx16), ma);
            tbl_st<NT>(at4(v4 + (iu + q * stride), tx16), va);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    i = iu + tx;
    for (; i < n4; i += stride) {
        float4 pa = tbl_ld<NT>(p4 + i), ga = tbl_ld<NT>(g4 + i), ma = tbl_ld<NT>(m4 + i), va = tbl_ld<NT>(v4 + i);
        adam_four(pa, ma, va, ga, g2, step_size, bc2_sqrt, c, sq);
        tbl_st<NT>(p4 + i, pa); tbl_st<NT>(m4 + i, ma); tbl_st<NT>(v4 + i, va);
    }
    for (long k = 4 * n4 + tid; k < n; k += stride) {
        float pa = p[k], ma = m[k], va = v[k];
        sq = fmaf(pa, pa, sq);
        adam_one(pa, fmaf(g2, pa, g[k]), ma, va, step_size, bc2_sqrt, c);
        p[k] = pa; m[k] = ma; v[k] = va;
        if (marks) { g[k] = 0.f; marks[k >> 2] = 0; }
    }
    tbl_l2_slot<ADAM_THREADS>(sq + (sq2.x + sq2.y), l2c, l2_part, slot0 + bid);
}

template <bool NT>
__global__ __launch_bounds__(ADAM_THREADS, 3) void adam_step_kernel(
    const AdamBatch batch, int cnt, int slot0, double lr_arg, const double* __restrict__ lr_dev, double beta1, double beta2, double eps,
    float* __restrict__ l2_part, const int* __restrict__ clock, const float* __restrict__ consts) {
    adam_step_body<NT>(batch, cnt, slot0, lr_arg, lr_dev, beta1, beta2, eps, l2_part, clock, consts, (int)blockIdx.x);
}

__global__ __launch_bounds__(1024) void adam_l2_finish_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ float acc[1024];
    adam_l2_finish_block<1024>(part, n, acc);
    if (threadIdx.x == 0) out[0] = acc[0];
}
// a job of the open finish batch (finish_batch.h), else its own launch
int xdfm_adam_l2_finish(const float* part, int n, float* out, hipStream_t st) {
    FinishJob j{};
    j.kind = FJ_ADAM_L2; j.blocks = 1;
    j.part = part; j.out = out; j.i0 = n;
    bool taken = false;
    if (int rc = xdfm_finish_defer(j, st, &taken)) return rc;
    if (!taken) hipLaunchKernelGGL(adam_l2_finish_kernel, dim3(1), dim3(1024), 0, st, part, n, out);
    return XDFM_OK;
}

// ---------------------------------------------------------------------------------------------
// deferred Adam: clock, catch-up of the rows a batch gathers, flush (xdfm.h, "K7d")
// ---------------------------------------------------------------------------------------------
__global__ void adam_tick_kernel(int* __restrict__ clock, float* __restrict__ consts, int cap, double lr_arg,
                                 const double* __restrict__ lr_dev, double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double lr = lr_dev ? *lr_dev : lr_arg;
    int t = clock[0] + 1;
    if (t >= cap) t = cap - 1;                          // the host flushes long before (defensive)
    clock[0] = t;
    const double step = (double)(clock[1] + t);         // the value the per-parameter step counters hold at this step
    const float ss = (float)(lr / (1.0 - pow(beta1, step)));
    const float bc = (float)sqrt(1.0 - pow(beta2, step));
    // the replay's short forms (adam_math.h) are proven for constants in these ranges; outside them rc2 = 0 sends the
    // step through the reference spelling
    const bool ok = bc >= 0.00390625f && bc <= 1.f && ss >= 9.313225746154785e-10f && ss <= 1024.f;    // 2^-8, 2^-30, 2^10
    float* k = consts + ADAM_CONSTS_PER_STEP * t;
    k[0] = ss;
    k[1] = bc;
    k[2] = bc * 4294967296.f;                           // 2^32
    k[3] = ok ? adam_exact_rcp(bc) * 2.3283064365386963e-10f : 0.f;     // 2^-32
}

__global__ void adam_clock_reset_kernel(int* __restrict__ clock) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { clock[1] += clock[0]; clock[0] = 0; }
}

// block sum of l2-weighted squares in fixed point (integer adds are exact: the total does not depend on which thread
// replayed which chunk, nor on the order of the blocks), one atomic per block
__device__ __forceinline__ long long adam_backlog_fix(float v) { return (long long)((double)v * ADAM_FIX); }
// ... of values a thread has converted and added up itself (one per chunk of its row: the same integers as a thread per chunk)
__device__ __forceinline__ void adam_backlog_add_fix(long long f, unsigned long long* __restrict__ backlog) {
    for (int o = 32; o > 0; o >>= 1) f += __shfl_xor(f, o);
    __shared__ long long part[ADAM_THREADS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tot = 0;
        for (int k = 0; k < ADAM_THREADS / 64; ++k) tot += part[k];
        if (tot) atomicAdd(backlog, (unsigned long long)tot);
    }
}
__device__ __forceinline__ void adam_backlog_add(float v, unsigned long long* __restrict__ backlog) {
    adam_backlog_add_fix(adam_backlog_fix(v), backlog);
}

struct AdamRowsDev {
    float* const* p; float* const* m; float* const* v; unsigned char* const* last; const float* l2;
    float* const* g; unsigned char* const* marks;
};
// the embedding or the linear tables' pointer arrays, picked field by field (a reference chosen at run time between the
// two kernel-argument structs makes hipcc copy both to scratch and index them there: 120 bytes of private memory per lane)
__device__ __forceinline__ AdamRowsDev adam_rows_pick(bool is_lin, const AdamRowsDev& emb, const AdamRowsDev& lin) {
    AdamRowsDev R;
    R.p = is_lin ? lin.p : emb.p; R.m = is_lin ? lin.m : emb.m; R.v = is_lin ? lin.v : emb.v;
    R.last = is_lin ? lin.last : emb.last; R.l2 = is_lin ? lin.l2 : emb.l2;
    R.g = is_lin ? lin.g : emb.g; R.marks = is_lin ? lin.marks : emb.marks;
    return R;
}

// The chunk of thread idx -- (example, field, chunk of the row) -- and its claim: `old` >= 0 when this thread is the first
// to reach the chunk in this launch (CAS on the word that holds its `last` byte) and has to bring it from step `old` to t;
// duplicates of an id lose the claim and skip.
struct AdamClaim { int f; long cc; int old; bool is_lin; };
__device__ __forceinline__ AdamClaim adam_claim_chunk(long idx, const float* __restrict__ X, long ldx, const int* __restrict__ cols,
                                                      const int* __restrict__ vocab, int m, int D, int QE, int QT,
                                                      const AdamRowsDev& emb, const AdamRowsDev& lin, int t, bool need_table) {
    AdamClaim k;
    const int q = (int)(idx % QT);
    const long r = idx / QT;
    k.f = (int)(r % m);
    const long b = r / m;
    const int V = vocab[k.f];
    long id = (long)X[b * ldx + cols[k.f]];             // as the gather (embed.hip): truncation, clamped
    if (id < 0 || id >= V) id = id < 0 ? 0 : V - 1;
    k.is_lin = q >= QE;
    const AdamRowsDev R = adam_rows_pick(k.is_lin, emb, lin);
    const long w = k.is_lin ? 1 : D;
    const long c0 = id * w / 4, c1 = (id * w + w - 1) / 4;
    k.cc = c0 + (k.is_lin ? 0 : q);
    const long n4 = (long)V * w / 4;                    // whole chunks; the tail elements are updated densely every step
    k.old = -1;
    if (k.cc <= c1 && k.cc < n4 && (!need_table || R.p[k.f] != nullptr))       // a null table: left to the step's mark scan (small tables)
        k.old = tbl_claim(R.last[k.f], k.cc, t);
    return k;
}

// One thread per (example, field, chunk of the row): the first thread to reach a chunk replays the steps it misses.  The
// gather runs in a later launch.
__global__ __launch_bounds__(ADAM_THREADS) void adam_catchup_rows_kernel(
    const float* __restrict__ X, long ldx, int B, const int* __restrict__ cols, const int* __restrict__ vocab, int m, int D,
    AdamRowsDev emb, AdamRowsDev lin, int has_lin, const int* __restrict__ clock, const float* __restrict__ consts,
    double beta1, double beta2, double eps, unsigned long long* __restrict__ backlog, int own_blocks, const X3PackJobs riders) {
    // workgroups past the catch-up's own run a rider and return: the partial |W| maxima of the CIN weight packs (cin_x3_pack.h)
    if ((int)blockIdx.x >= own_blocks) { x3_absmax_rider(riders, (long)((int)blockIdx.x - own_blocks)); return; }
    const int t = clock[0];
    const int QE = (D + 3) / 4 + ((D & 3) ? 1 : 0);     // chunks a row of D floats can straddle
    const int QT = QE + (has_lin ? 1 : 0);
    const long idx = (long)blockIdx.x * ADAM_THREADS + threadIdx.x;
    const AdamCoef c = adam_uniform(AdamCoef{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), 0.f, (float)eps});
    const bool eps_ok = c.eps >= ADAM_EPS_MIN && c.eps <= 1.f;
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    AdamClaim k;
    k.old = -1; k.f = 0; k.cc = 0; k.is_lin = false;
    if (t > 0 && idx < (long)B * m * QT) k = adam_claim_chunk(idx, X, ldx, cols, vocab, m, D, QE, QT, emb, lin, t, false);
    const bool act = k.old >= 0;
    const AdamRowsDev R = adam_rows_pick(k.is_lin, emb, lin);
    float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), ma = pa, va = pa;
    float4 *p4 = nullptr, *m4 = nullptr, *v4 = nullptr;
    float l2c = 0.f;
    if (act) {
        p4 = reinterpret_cast<float4*>(R.p[k.f]) + k.cc;
        m4 = reinterpret_cast<float4*>(R.m[k.f]) + k.cc;
        v4 = reinterpret_cast<float4*>(R.v[k.f]) + k.cc;
        pa = *p4; ma = *m4; va = *v4;
        l2c = R.l2[k.f];
    }
    adam_f2 sq2 = {0.f, 0.f};
    adam_replay_span(pa, ma, va, act, k.old, t, consts, 2.f * l2c, zf, c, sq2, eps_ok);
    if (act) { *p4 = pa; *m4 = ma; *v4 = va; }
    adam_backlog_add(l2c * (sq2.x + sq2.y), backlog);
}

// The step's update of the deferred tables, by the batch's rows (single process: every marked chunk belongs to a row
// of X).  Threads [0, B*m*QT): one per (example, field, chunk of the row), first come first served through `last` as in
// the catch-up; then 4 * m threads per table kind for the numel % 4 tail elements, which no chunk covers.
// (the body for workgroup `bid` of the rows grid: the kernel of its own below, and the workgroups of adam_step_rows_kernel
// behind the step's; the pointer tables BY VALUE: taken by reference they go to scratch, see adam_rows_pick)
__device__ __forceinline__ void adam_apply_rows_body(
    const float* __restrict__ X, long ldx, int B, const int* __restrict__ cols, const int* __restrict__ vocab, int m, int D,
    const AdamRowsDev emb, const AdamRowsDev lin, int has_lin, const int* __restrict__ clock, const float* __restrict__ consts,
    double beta1, double beta2, double eps, unsigned long long* __restrict__ cell, const long bid) {
    const int t = clock[0];
    const int QE = (D + 3) / 4 + ((D & 3) ? 1 : 0);
    const int QT = QE + (has_lin ? 1 : 0);
    const long idx = bid * ADAM_THREADS + threadIdx.x;
    const long nrow = (long)B * m * QT;
    const float ss = consts[ADAM_CONSTS_PER_STEP * t], bc = consts[ADAM_CONSTS_PER_STEP * t + 1];
    const AdamCoef c = adam_uniform(AdamCoef{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), 0.f, (float)eps});
    const bool eps_ok = c.eps >= ADAM_EPS_MIN && c.eps <= 1.f;
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    float sqv = 0.f;
    AdamClaim k;
    k.old = -1; k.f = 0; k.cc = 0; k.is_lin = false;
    if (idx < nrow) k = adam_claim_chunk(idx, X, ldx, cols, vocab, m, D, QE, QT, emb, lin, t, true);
    const bool act = k.old >= 0;
    {
        const AdamRowsDev R = adam_rows_pick(k.is_lin, emb, lin);
        float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), ma = pa, va = pa, ga = pa;
        float4 *p4 = nullptr, *m4 = nullptr, *v4 = nullptr;
        float l2c = 0.f;
        if (act) {
            p4 = reinterpret_cast<float4*>(R.p[k.f]) + k.cc;
            m4 = reinterpret_cast<float4*>(R.m[k.f]) + k.cc;
            v4 = reinterpret_cast<float4*>(R.v[k.f]) + k.cc;
            float4* g4 = reinterpret_cast<float4*>(R.g[k.f]) + k.cc;
            pa = *p4; ma = *m4; va = *v4; ga = *g4;
            *g4 = make_float4(zf, zf, zf, zf);
            R.marks[k.f][k.cc] = 0;
            l2c = R.l2[k.f];
        }
        const float g2 = 2.f * l2c;
        adam_f2 sq2 = {0.f, 0.f};
        adam_replay_span(pa, ma, va, act, k.old, t - 1, consts, g2, zf, c, sq2, eps_ok);     // the steps the chunk still misses
        if (act) {                                                                           // then this step, with its gradient
            float sq = sq2.x + sq2.y;
            adam_four(pa, ma, va, ga, g2, ss, bc, c, sq);
            *p4 = pa; *m4 = ma; *v4 = va;
            sqv = l2c * sq;
        }
    }
    if (idx >= nrow && idx < nrow + 8L * m) {
        // tail elements: (table kind, field, element k < 4) -- updated every step, like the sweep does
        const long u = idx - nrow;
        const int kk = (int)(u & 3);
        const int f = (int)((u >> 2) % m);
        const bool is_lin = (u >> 2) >= m;
        if (!is_lin || has_lin) {
            const AdamRowsDev R = adam_rows_pick(is_lin, emb, lin);
            const long numel = (long)vocab[f] * (is_lin ? 1 : D);
            const long e = numel / 4 * 4 + kk;
            if (e < numel && R.p[f] != nullptr) {
                float* p = R.p[f]; float* mm = R.m[f]; float* vv = R.v[f]; float* g = R.g[f];
                const float l2c = R.l2[f];
                float pa = p[e], ma = mm[e], va = vv[e];
                sqv = l2c * (pa * pa);
                adam_one(pa, fmaf(2.f * l2c, pa, g[e]), ma, va, ss, bc, c);
                p[e] = pa; mm[e] = ma; vv[e] = va;
                g[e] = 0.f;
                R.marks[f][e >> 2] = 0;
            }
        }
    }
    adam_backlog_add(sqv, cell);
}
__global__ __launch_bounds__(ADAM_THREADS) void adam_apply_rows_kernel(
    const float* __restrict__ X, long ldx, int B, const int* __restrict__ cols, const int* __restrict__ vocab, int m, int D,
    AdamRowsDev emb, AdamRowsDev lin, int has_lin, const int* __restrict__ clock, const float* __restrict__ consts,
    double beta1, double beta2, double eps, unsigned long long* __restrict__ cell) {
    adam_apply_rows_body(X, ldx, B, cols, vocab, m, D, emb, lin, has_lin, clock, consts, beta1, beta2, eps, cell, (long)blockIdx.x);
}

// ---- by row (D % 4 == 0: a row is D / 4 whole chunks of its own; option "adam_rows") ----------------------------------
// Threads [0, m * B): one per (field, example), the FIELD outermost, and the whole row is the thread's: one claim per `last`
// word of the row (tbl_claim_row) instead of one per chunk -- at D = 16 a row's four bytes are one word, on which the four
// lanes of the by-chunk kernels issue four CAS in turn -- then the row's chunks in turn, each from its OWN old byte (they
// differ after a step the mark scan took).  A wave holds 64 rows of one field, so tables that are up to date (the small
// vocabularies) and tables that are not no longer share waves: the replay, which every lane of a wave sits through
// (adam_replay_span), is as long as that field needs.  Threads [m * B, 2 * m * B), with linear tables: one linear entry
// each, claimed by chunk as before (four ids share a chunk, sixteen a word).  The arithmetic per chunk is the by-chunk
// kernels', and so are the integers that go into the L2 sums (one conversion per chunk, adam_backlog_fix).
struct AdamRow { int f; long c0; int nq; bool is_lin; };      // field, first chunk, chunks that are this thread's (0: none)
__device__ __forceinline__ AdamRow adam_row_of(long idx, bool live, const float* __restrict__ X, long ldx, const int* __restrict__ cols,
                                               const int* __restrict__ vocab, int m, int B, int D, int has_lin) {
    AdamRow r;
    r.f = 0; r.c0 = 0; r.nq = 0; r.is_lin = false;
    const long nE = (long)m * B;
    if (!live || idx >= (has_lin ? 2 * nE : nE)) return r;
    r.is_lin = idx >= nE;
    const long u = r.is_lin ? idx - nE : idx;
    r.f = (int)(u / B);
    const long b = u - (long)r.f * B;
    const int V = vocab[r.f];
    long id = (long)X[b * ldx + cols[r.f]];             // as the gather (embed.hip): truncation, clamped
    if (id < 0 || id >= V) id = id < 0 ? 0 : V - 1;
    const long w = r.is_lin ? 1 : D;
    r.c0 = id * w / 4;
    const long left = (long)V * w / 4 - r.c0;           // whole chunks from c0 on; the tail elements are updated densely every step
    const long want = r.is_lin ? 1 : D / 4;
    r.nq = (int)(left < want ? (left > 0 ? left : 0) : want);
    return r;
}
// the claim of chunks q0 .. q0 + 7 of the thread's row -> their old bytes as tbl_claim_row returns them
__device__ __forceinline__ unsigned long long adam_row_claim(const AdamRow& r, unsigned char* last, int q0, int t) {
    const int gn = r.nq - q0 < 8 ? r.nq - q0 : 8;
    if (gn <= 0) return ~0ull;
    if (!r.is_lin) return tbl_claim_row(last, r.c0 + q0, gn, t);
    const int old = tbl_claim(last, r.c0, t);
    return old < 0 ? ~0ull : ((~0ull << 8) | (unsigned long long)old);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_catchup_by_row_kernel(
    const float* __restrict__ X, long ldx, int B, const int* __restrict__ cols, const int* __restrict__ vocab, int m, int D,
    AdamRowsDev emb, AdamRowsDev lin, int has_lin, const int* __restrict__ clock, const float* __restrict__ consts,
    double beta1, double beta2, double eps, unsigned long long* __restrict__ backlog, int own_blocks, const X3PackJobs riders) {
    // workgroups past the catch-up's own run a rider and return: the partial |W| maxima of the CIN weight packs (cin_x3_pack.h)
    if ((int)blockIdx.x >= own_blocks) { x3_absmax_rider(riders, (long)((int)blockIdx.x - own_blocks)); return; }
    const int t = clock[0];
    const int Q = D / 4;
    const long idx = (long)blockIdx.x * ADAM_THREADS + threadIdx.x;
    const AdamCoef c = adam_uniform(AdamCoef{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), 0.f, (float)eps});
    const bool eps_ok = c.eps >= ADAM_EPS_MIN && c.eps <= 1.f;
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const AdamRow r = adam_row_of(idx, t > 0, X, ldx, cols, vocab, m, B, D, has_lin);
    const AdamRowsDev R = adam_rows_pick(r.is_lin, emb, lin);
    float4 *p4 = nullptr, *m4 = nullptr, *v4 = nullptr;
    unsigned char* last = nullptr;
    float l2c = 0.f;
    if (r.nq > 0) {
        p4 = reinterpret_cast<float4*>(R.p[r.f]) + r.c0;
        m4 = reinterpret_cast<float4*>(R.m[r.f]) + r.c0;
        v4 = reinterpret_cast<float4*>(R.v[r.f]) + r.c0;
        last = R.last[r.f];
        l2c = R.l2[r.f];
    }
    long long fix = 0;
    for (int q0 = 0; q0 < Q; q0 += 8) {                 // wave-uniform trip counts: every lane reaches every adam_replay_span
        const unsigned long long olds = adam_row_claim(r, last, q0, t);
        const int turns = Q - q0 < 8 ? Q - q0 : 8;
        for (int j = 0; j < turns; ++j) {
            const int old = (int)((olds >> (8 * j)) & 255ull);
            const bool act = old != 255;
            float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), ma = pa, va = pa;
            if (act) { pa = p4[q0 + j]; ma = m4[q0 + j]; va = v4[q0 + j]; }
            adam_f2 sq2 = {0.f, 0.f};
            adam_replay_span(pa, ma, va, act, old, t, consts, 2.f * l2c, zf, c, sq2, eps_ok);
            if (act) {
                p4[q0 + j] = pa; m4[q0 + j] = ma; v4[q0 + j] = va;
                fix += adam_backlog_fix(l2c * (sq2.x + sq2.y));
            }
        }
    }
    adam_backlog_add_fix(fix, backlog);
}

// ... and the step's update: as adam_apply_rows_kernel, the 8 * m tail threads behind the row and linear threads
__device__ __forceinline__ void adam_apply_by_row_body(
    const float* __restrict__ X, long ldx, int B, const int* __restrict__ cols, const int* __restrict__ vocab, int m, int D,
    const AdamRowsDev emb, const AdamRowsDev lin, int has_lin, const int* __restrict__ clock, const float* __restrict__ consts,
    double beta1, double beta2, double eps, unsigned long long* __restrict__ cell, const long bid) {
    const int t = clock[0];
    const int Q = D / 4;
    const long idx = bid * ADAM_THREADS + threadIdx.x;
    const long nrow = (long)B * m * (has_lin ? 2 : 1);
    const float ss = consts[ADAM_CONSTS_PER_STEP * t], bc = consts[ADAM_CONSTS_PER_STEP * t + 1];
    const AdamCoef c = adam_uniform(AdamCoef{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), 0.f, (float)eps});
    const bool eps_ok = c.eps >= ADAM_EPS_MIN && c.eps <= 1.f;
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    long long fix = 0;
    {
        AdamRow r = adam_row_of(idx, true, X, ldx, cols, vocab, m, B, D, has_lin);
        const AdamRowsDev R = adam_rows_pick(r.is_lin, emb, lin);
        float4 *p4 = nullptr, *m4 = nullptr, *v4 = nullptr, *g4 = nullptr;
        unsigned char *last = nullptr, *marks = nullptr;
        float l2c = 0.f;
        if (r.nq > 0 && R.p[r.f] == nullptr) r.nq = 0;  // a null table: left to the step's mark scan (small tables)
        if (r.nq > 0) {
            p4 = reinterpret_cast<float4*>(R.p[r.f]) + r.c0;
            m4 = reinterpret_cast<float4*>(R.m[r.f]) + r.c0;
            v4 = reinterpret_cast<float4*>(R.v[r.f]) + r.c0;
            g4 = reinterpret_cast<float4*>(R.g[r.f]) + r.c0;
            marks = R.marks[r.f] + r.c0;
            last = R.last[r.f];
            l2c = R.l2[r.f];
        }
        const float g2 = 2.f * l2c;
        for (int q0 = 0; q0 < Q; q0 += 8) {
            const unsigned long long olds = adam_row_claim(r, last, q0, t);
            const int turns = Q - q0 < 8 ? Q - q0 : 8;
            for (int j = 0; j < turns; ++j) {
                const int old = (int)((olds >> (8 * j)) & 255ull);
                const bool act = old != 255;
                float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), ma = pa, va = pa, ga = pa;
                if (act) {
                    pa = p4[q0 + j]; ma = m4[q0 + j]; va = v4[q0 + j]; ga = g4[q0 + j];
                    g4[q0 + j] = make_float4(zf, zf, zf, zf);
                    marks[q0 + j] = 0;
                }
                adam_f2 sq2 = {0.f, 0.f};
                adam_replay_span(pa, ma, va, act, old, t - 1, consts, g2, zf, c, sq2, eps_ok);   // the steps the chunk still misses
                if (act) {                                                                       // then this step, with its gradient
                    float sq = sq2.x + sq2.y;
                    adam_four(pa, ma, va, ga, g2, ss, bc, c, sq);
                    p4[q0 + j] = pa; m4[q0 + j] = ma; v4[q0 + j] = va;
                    fix += adam_backlog_fix(l2c * sq);
                }
            }
        }
    }
    if (idx >= nrow && idx < nrow + 8L * m) {
        // tail elements: (table kind, field, element k < 4) -- updated every step, like the sweep does
        const long u = idx - nrow;
        const int kk = (int)(u & 3);
        const int f = (int)((u >> 2) % m);
        const bool is_lin = (u >> 2) >= m;
        if (!is_lin || has_lin) {
            const AdamRowsDev R = adam_rows_pick(is_lin, emb, lin);
            const long numel = (long)vocab[f] * (is_lin ? 1 : D);
            const long e = numel / 4 * 4 + kk;
            if (e < numel && R.p[f] != nullptr) {
                float* p = R.p[f]; float* mm = R.m[f]; float* vv = R.v[f]; float* g = R.g[f];
                const float l2c = R.l2[f];
                float pa = p[e], ma = mm[e], va = vv[e];
                fix += adam_backlog_fix(l2c * (pa * pa));
                adam_one(pa, fmaf(2.f * l2c, pa, g[e]), ma, va, ss, bc, c);
                p[e] = pa; mm[e] = ma; vv[e] = va;
                g[e] = 0.f;
                R.marks[f][e >> 2] = 0;
            }
        }
    }
    adam_backlog_add_fix(fix, cell);
}
__global__ __launch_bounds__(ADAM_THREADS) void adam_apply_by_row_kernel(
    const float* __restrict__ X, long ldx, int B, const int* __restrict__ cols, const int* __restrict__ vocab, int m, int D,
    AdamRowsDev emb, AdamRowsDev lin, int has_lin, const int* __restrict__ clock, const float* __restrict__ consts,
    double beta1, double beta2, double eps, unsigned long long* __restrict__ cell) {
    adam_apply_by_row_body(X, ldx, B, cols, vocab, m, D, emb, lin, has_lin, clock, consts, beta1, beta2, eps, cell, (long)blockIdx.x);
}

// The step and the rows update in ONE launch (xdfm_colaunch_adam_step, option "colaunch" bit 0).  The two touch
// different tensors -- the rows update owns the tables whose `param` its pointer arrays hold, the step everything else -- and
// both only read what adam_tick_kernel wrote, so nothing orders them; alone, either leaves most of the chip idle (the step:
// some 94 waves in long dependent chains; the rows: a claim / replay / update chain per row).  Workgroups [0, first[cnt]) run
// the step's body: its chains are the long ones, they start first, and their L2 partials keep their slots.  The workgroups
// behind them run the rows body with the block index rebased.  Same arithmetic, same sums: the bits of the two launches.
struct AdamRowsArgs {
    const float* X; long ldx; int B; const int* cols; const int* vocab; int m; int D;
    AdamRowsDev emb, lin; int has_lin; unsigned long long* cell;
};
static_assert(sizeof(AdamBatch) + sizeof(AdamRowsArgs) + 128 <= 8192, "adam_step_rows_kernel's argument block");
template <bool BY_ROW>
__global__ __launch_bounds__(ADAM_THREADS, 3) void adam_step_rows_kernel(
    const AdamBatch batch, int cnt, int slot0, double lr_arg, const double* __restrict__ lr_dev, double beta1, double beta2, double eps,
    float* __restrict__ l2_part, const int* __restrict__ clock, const float* __restrict__ consts, const AdamRowsArgs r) {
    const int own = batch.first[cnt];
    if ((int)blockIdx.x < own) {
        // NT = true always: xdfm_colaunch_adam_step leaves the cached-access experiment ("dbg" bit 17) to the two launches
        adam_step_body<true>(batch, cnt, slot0, lr_arg, lr_dev, beta1, beta2, eps, l2_part, clock, consts, (int)blockIdx.x);
        return;
    }
    const long bid = (long)blockIdx.x - own;
    if constexpr (BY_ROW)
        adam_apply_by_row_body(r.X, r.ldx, r.B, r.cols, r.vocab, r.m, r.D, r.emb, r.lin, r.has_lin, clock, consts, beta1, beta2, eps, r.cell, bid);
    else
        adam_apply_rows_body(r.X, r.ldx, r.B, r.cols, r.vocab, r.m, r.D, r.emb, r.lin, r.has_lin, clock, consts, beta1, beta2, eps, r.cell, bid);
}

__global__ void adam_rows_finish_kernel(unsigned long long* __restrict__ cell, float* __restrict__ l2_value) {
    if (threadIdx.x == 0 && blockIdx.x == 0) adam_rows_finish_one(cell, l2_value);
}
// a job of the open finish batch (finish_batch.h: behind the L2 finish that sets the same l2_value), else its own launch
int xdfm_adam_rows_finish(unsigned long long* cell, float* l2_value, hipStream_t st) {
    FinishJob j{};
    j.kind = FJ_ADAM_ROWS; j.blocks = 1;
    j.cell = cell; j.out = l2_value;
    bool taken = false;
    if (int rc = xdfm_finish_defer(j, st, &taken)) return rc;
    if (!taken) hipLaunchKernelGGL(adam_rows_finish_kernel, dim3(1), dim3(64), 0, st, cell, l2_value);
    return XDFM_OK;
}

// Every chunk of the deferred tensors up to the clock; `last` back to 0.  Same 1-D grid as the step.
__global__ __launch_bounds__(ADAM_THREADS) void adam_flush_kernel(const AdamBatch batch, int cnt, const int* __restrict__ clock,
                                                                  const float* __restrict__ consts, double beta1, double beta2,
                                                                  double eps, unsigned long long* __restrict__ backlog) {
    int ti = 0;
    for (int k = 1; k < cnt; ++k) ti += (int)blockIdx.x >= batch.first[k] ? 1 : 0;
    const int lb = (int)blockIdx.x - batch.first[ti];
    const int nb = batch.first[ti + 1] - batch.first[ti];
    const AdamDev& d = batch.t[ti];
    const int t = clock[0];
    float4* p4 = reinterpret_cast<float4*>(d.param);
    float4* m4 = reinterpret_cast<float4*>(d.exp_avg);
    float4* v4 = reinterpret_cast<float4*>(d.exp_avg_sq);
    unsigned char* __restrict__ last = d.last;
    const long n4 = d.numel / 4;
    const float l2c = d.l2;
    const float g2 = adam_uniform(2.f * l2c);
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const AdamCoef c = adam_uniform(AdamCoef{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), 0.f, (float)eps});
    adam_f2 sq2 = {0.f, 0.f};
    const bool eps_ok = c.eps >= ADAM_EPS_MIN && c.eps <= 1.f;
    const unsigned tx16 = threadIdx.x * 16u;
    // whole-wave iterations (the replay lines the lanes up on the step number): the tail lanes are masked, not absent
    for (long base = (long)lb * ADAM_THREADS; base < n4; base += (long)nb * ADAM_THREADS) {
        const long i = base + threadIdx.x;
        const bool in = i < n4;
        const int old = in ? (int)last[i] : 0;
        const bool act = in && old < t;
        float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), ma = pa, va = pa;
        // (addresses: the iteration's wave-uniform base plus one 32-bit lane offset, as in the step's loops -- three 64-bit
        // per-lane pointers would sit in registers through the whole replay)
        if (act) { pa = tbl_ld<true>(at4(p4 + base, tx16)); ma = tbl_ld<true>(at4(m4 + base, tx16)); va = tbl_ld<true>(at4(v4 + base, tx16)); }
        adam_replay_span<true>(pa, ma, va, act, old, t, consts, g2, zf, c, sq2, eps_ok);
        if (act) { tbl_st<true>(at4(p4 + base, tx16), pa); tbl_st<true>(at4(m4 + base, tx16), ma); tbl_st<true>(at4(v4 + base, tx16), va); }
        if (in && old) last[i] = 0;
    }
    adam_backlog_add(l2c * (sq2.x + sq2.y), backlog);
}

// ---------------------------------------------------------------------------------------------
// Self-test of the replay's short forms against the reference spellings (adam_math.h), on the device, for the tests.
// out[0] = cases compared, out[1] = mismatches, out[2] = an encoding of one mismatching case.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long adam_mix(unsigned long long z) {       // splitmix64
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float adam_rand_float(unsigned long long h, int emin, int emax, bool sign) {     // 2^[emin, emax) x [1, 2)
    const int e = emin + (int)((h >> 32) % (unsigned)(emax - emin));
    const unsigned bits = ((unsigned)(e + 127) << 23) | ((unsigned)h & 0x7fffffu) | ((sign && ((h >> 60) & 1)) ? 0x80000000u : 0u);
    return __uint_as_float(bits);
}
__device__ __forceinline__ AdamStepConst adam_const_for(double lr, double beta1, double beta2, double step) {
    AdamStepConst k;
    k.ss = (float)(lr / (1.0 - pow(beta1, step)));
    k.bc = (float)sqrt(1.0 - pow(beta2, step));
    k.c2 = k.bc * 4294967296.f;
    k.rc2 = adam_exact_rcp(k.bc) * 2.3283064365386963e-10f;
    return k;
}
__global__ __launch_bounds__(256) void adam_selftest_kernel(int mode, unsigned long long base, unsigned long long n,
                                                            unsigned long long seed, double lr, double beta1, double beta2, double eps,
                                                            unsigned long long* __restrict__ out) {
#pragma clang fp contract(off)
    const unsigned long long idx = base + (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long bad = 0, done = 0, what = 0;
    if (idx < n) {
        if (mode == 0) {                    // square root: every bit pattern; compared where the replay uses it (0 < x < 2^62)
            const float x = __uint_as_float((unsigned)idx);
            if (x > 0.f && x < ADAM_V_MAX) {
                const float x2 = x * 18446744073709551616.f;
                const float fast = adam_sqrt_scaled2(adam_f2{x2, x2}).x, ref = sqrtf(x) * 4294967296.f;
                done = 1; bad = __float_as_uint(fast) != __float_as_uint(ref); what = idx;
            }
        } else if (mode == 1) {             // division by the step's constant: every numerator of two binades x steps 1..
            const unsigned mant = (unsigned)(idx & 0xffffffull);
            const unsigned long long tt = (idx >> 24) + 1;
            // beyond the first 256 steps: random constants in [2^-8, 1)
            const float bc = tt <= 256 ? (float)sqrt(1.0 - pow(beta2, (double)tt)) : adam_rand_float(adam_mix(seed + tt), -8, 0, false);
            const float S = __uint_as_float(0x3f800000u + mant);
            const float s2 = S * 4294967296.f;
            const float fast = adam_div_const2(adam_f2{s2, s2}, bc * 4294967296.f, adam_exact_rcp(bc) * 2.3283064365386963e-10f).y;
            const float ref = S / bc;
            done = 1; bad = __float_as_uint(fast) != __float_as_uint(ref); what = idx;
        } else if (mode == 2) {             // general division inside the guard: d in [2^-40, 2^40), |n| in [2^-80, 2^40) or 0
            const unsigned long long h0 = adam_mix(seed + 2 * idx), h1 = adam_mix(seed + 2 * idx + 1);
            const float d = adam_rand_float(h0, -40, 40, false);
            float nn = adam_rand_float(h1, -80, 40, true);
            if ((h1 >> 40) % 1021 == 0) nn = 0.f;
            if ((h1 >> 40) % 1021 == 1) nn = __uint_as_float(((h0 >> 61) & 1) ? 0x17800000u : 0x537fffffu);    // 2^-80, just under 2^40
            const float fast = adam_div2(adam_f2{nn, nn}, adam_f2{d, d}).x, ref = nn / d;
            done = 1; bad = __float_as_uint(fast) != __float_as_uint(ref) && !(fast == 0.f && ref == 0.f);
            what = ((unsigned long long)__float_as_uint(nn) << 32) | __float_as_uint(d);
        } else {                            // whole replayed steps against adam_one, states incl. zeros / denormals / huge values
            const AdamCoef c = adam_uniform(AdamCoef{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), 0.f, (float)eps});
            const bool eps_ok = c.eps >= ADAM_EPS_MIN && c.eps <= 1.f;
            float zf;
            asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
            float pv[4], mv[4], vv[4];
            for (int e = 0; e < 4; ++e) {
                const unsigned long long h = adam_mix(seed + 16 * idx + e), h2 = adam_mix(h), h3 = adam_mix(h2);
                pv[e] = adam_rand_float(h, -30, 8, true);
                mv[e] = adam_rand_float(h2, -60, 4, true);
                vv[e] = adam_rand_float(h3, -100, 10, false);
                const unsigned sel = (unsigned)((h >> 48) % 97);
                if (sel == 0) pv[e] = 0.f;
                if (sel == 1) { mv[e] = 0.f; vv[e] = 0.f; }
                if (sel == 2) pv[e] = __uint_as_float(0x00000fffu);                   // denormal weight
                if (sel == 3) { pv[e] = 3e30f; vv[e] = 1e35f; }
                if (sel == 4) mv[e] = __uint_as_float(0x00400000u);                   // denormal first moment
                if (sel == 5) vv[e] = __uint_as_float(0x00000001u);                   // smallest second moment
            }
            const float g2 = (adam_mix(seed + idx) & 7) == 0 ? 0.f : 2e-5f;
            float4 pf = make_float4(pv[0], pv[1], pv[2], pv[3]), mf = make_float4(mv[0], mv[1], mv[2], mv[3]),
                   vf = make_float4(vv[0], vv[1], vv[2], vv[3]);
            for (int st = 1; st <= 6 && !bad; ++st) {
                const AdamStepConst k = adam_const_for(lr, beta1, beta2, (double)(st + (idx % 50) * 7));
                float4 pr = pf, mr = mf, vr = vf;
                adam_f2 sq2 = {0.f, 0.f};
                adam_replay4(pf, mf, vf, k, g2, zf, c, sq2, eps_ok);
                float* a[3] = {&pr.x, &mr.x, &vr.x};
                for (int e = 0; e < 4; ++e) adam_one(a[0][e], fmaf(g2, a[0][e], zf), a[1][e], a[2][e], k.ss, k.bc, c);
                const float* f[3] = {&pf.x, &mf.x, &vf.x};
                for (int q = 0; q < 3; ++q)
                    for (int e = 0; e < 4; ++e) {
                        const float x = f[q][e], y = a[q][e];
                        if (__float_as_uint(x) != __float_as_uint(y) && !(x != x && y != y) && !(x == 0.f && y == 0.f)) bad = 1;
                    }
                done += 1;
                what = idx * 8 + st;
            }
        }
    }
    if (done) atomicAdd(&out[0], done);
    if (bad) { atomicAdd(&out[1], 1ull); atomicMax(&out[2], what); }
}

// `last` holds the step in one byte per chunk: a table of more than 256 steps would let it wrap
static int adam_clock_ok(const char* what, const xdfm_adam_clock* clk) {
    XDFM_REQUIRE(clk && clk->clock && clk->consts && clk->cap > 2 && clk->cap <= 256, "%s: bad clock", what);
    return XDFM_OK;
}

// which kernels xdfm_adam_catchup_rows / _apply_rows launch: by row where a row is whole chunks (every other D: by chunk,
// whatever the option says); read when the launch is issued, so a captured graph keeps what it was captured with
static bool adam_by_row(int D) {
    const bool by_row = D % 4 == 0 && xdfm_opt(OPT_ADAM_ROWS) != 0;
    xdfm_opt_note(OPT_LAST_ADAM_ROWS, by_row ? 1 : 0);
    return by_row;
}

extern "C" {

size_t xdfm_adam_step_ws_elems(int T) { return T > 0 ? (size_t)T * ADAM_BX : 0; }

int xdfm_adam_step(const xdfm_adam_tensor* tensors, int T, double lr, double beta1, double beta2, double eps,
                   float* l2_ws, float* l2_value, void* stream) {
    return xdfm_adam_step_lr(tensors, T, lr, nullptr, beta1, beta2, eps, l2_ws, l2_value, stream);
}

// rows != nullptr: the rows update rides behind the first launch's workgroups (adam_step_rows_kernel)
static int adam_step_impl(const xdfm_adam_tensor* tensors, int T, const xdfm_adam_clock* clk, double lr, const double* lr_dev,
                          double beta1, double beta2, double eps, float* l2_ws, float* l2_value, void* stream,
                          const AdamRowsArgs* rows = nullptr, bool rows_by_row = false, int rows_blocks = 0);

int xdfm_adam_step_lr(const xdfm_adam_tensor* tensors, int T, double lr, const double* lr_dev, double beta1, double beta2,
                      double eps, float* l2_ws, float* l2_value, void* stream) {
    return adam_step_impl(tensors, T, nullptr, lr, lr_dev, beta1, beta2, eps, l2_ws, l2_value, stream);
}

int xdfm_adam_step_deferred(const xdfm_adam_tensor* tensors, int T, const xdfm_adam_clock* clk, double lr,
                            const double* lr_dev, double beta1, double beta2, double eps, float* l2_ws, float* l2_value,
                            void* stream) {
    // an otherwise good clock whose table is too long gets a message of its own
    XDFM_REQUIRE(!(clk && clk->clock && clk->consts && clk->cap > 256), "adam_step_deferred: bad clock (cap %d > 256)", clk->cap);
    if (int rc = adam_clock_ok("adam_step_deferred", clk)) return rc;
    return adam_step_impl(tensors, T, clk, lr, lr_dev, beta1, beta2, eps, l2_ws, l2_value, stream);
}

static int adam_step_impl(const xdfm_adam_tensor* tensors, int T, const xdfm_adam_clock* clk, double lr, const double* lr_dev,
                          double beta1, double beta2, double eps, float* l2_ws, float* l2_value, void* stream,
                          const AdamRowsArgs* rows, bool rows_by_row, int rows_blocks) {
    if (int rc = tbl_check_call("adam_step", tensors, T)) return rc;
    XDFM_REQUIRE(lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0, "adam_step: bad hyper-parameters");
    if (int rc = tbl_check_l2("adam_step", l2_ws, l2_value)) return rc;
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(tensors[t].param && tensors[t].grad && tensors[t].exp_avg && tensors[t].exp_avg_sq && tensors[t].step &&
                         tensors[t].numel >= 0, "adam_step: tensor %d has a null pointer", t);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(!(tensors[t].flags & XDFM_ADAM_LAZY) || tensors[t].grad_marks, "adam_step: tensor %d is lazy but has no grad_marks", t);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(!(tensors[t].flags & XDFM_ADAM_DEFERRED) || (clk && tensors[t].grad_marks && tensors[t].last),
                     "adam_step: tensor %d is deferred but has no clock / grad_marks / last", t);
    for (int t = 0; t < T; ++t)
        XDFM_REQUIRE(!tensors[t].grad_marks || ((((size_t)tensors[t].param) | ((size_t)tensors[t].grad) | ((size_t)tensors[t].exp_avg) |
                                                  ((size_t)tensors[t].exp_avg_sq)) & 15) == 0,
                     "adam_step: tensor %d has grad_marks but a pointer that is not 16-byte aligned", t);
    hipStream_t st = (hipStream_t)stream;
    const int* clock = clk ? clk->clock : nullptr;
    const float* consts = clk ? clk->consts : nullptr;
    if (clk) hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, st, clk->clock, clk->consts, clk->cap, lr, lr_dev, beta1, beta2);
    // Launch composition (table_step.h): tensors sorted by size and dealt round-robin to the launches, blocks per tensor by size
    // (option "adam_bx" caps them: a small footprint for experiments)
    int cap = xdfm_opt(OPT_ADAM_BX);
    if (cap <= 0 || cap > ADAM_BX) cap = ADAM_BX;
    float* part = l2_value ? l2_ws : nullptr;
    const int slots = tbl_step_launches<AdamBatch>(tensors, T, adam_dev, ADAM_BLOCK_ELEMS, cap, [&](const AdamBatch& batch, int cnt, int slot0, int l) {
        if (rows && l == 0) {                           // the step's workgroups, then the rows update's
            const dim3 grid((unsigned)(batch.first[cnt] + rows_blocks));
            if (rows_by_row)
                hipLaunchKernelGGL(adam_step_rows_kernel<true>, grid, dim3(ADAM_THREADS), 0, st, batch, cnt, slot0, lr, lr_dev, beta1,
                                   beta2, eps, part, clock, consts, *rows);
            else
                hipLaunchKernelGGL(adam_step_rows_kernel<false>, grid, dim3(ADAM_THREADS), 0, st, batch, cnt, slot0, lr, lr_dev, beta1,
                                   beta2, eps, part, clock, consts, *rows);
        } else if (xdfm_opt(OPT_DBG) & (1 << 17))       // experiment: ordinary (cached) loads and stores
            hipLaunchKernelGGL(adam_step_kernel<false>, dim3(batch.first[cnt]), dim3(ADAM_THREADS), 0, st, batch, cnt, slot0, lr,
                               lr_dev, beta1, beta2, eps, part, clock, consts);
        else
            hipLaunchKernelGGL(adam_step_kernel<true>, dim3(batch.first[cnt]), dim3(ADAM_THREADS), 0, st, batch, cnt, slot0, lr,
                               lr_dev, beta1, beta2, eps, part, clock, consts);
    });
    if (l2_value)
        if (int rc = xdfm_adam_l2_finish(l2_ws, slots, l2_value, st)) return rc;
    return xdfm_check_launch("adam_step");
}

int xdfm_adam_catchup_rows(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                           const xdfm_adam_rows* emb, const xdfm_adam_rows* lin, const xdfm_adam_clock* clk,
                           double beta1, double beta2, double eps, float* backlog, void* stream) {
    XDFM_REQUIRE(X && cols && vocab && emb && clk && backlog, "adam_catchup_rows: null pointer");
    if (int rc = adam_clock_ok("adam_catchup_rows", clk)) return rc;
    XDFM_REQUIRE(B > 0 && m > 0 && D > 0, "adam_catchup_rows: bad shape B=%d m=%d D=%d", B, m, D);
    XDFM_REQUIRE((((size_t)backlog) & 7) == 0, "adam_catchup_rows: backlog must be 8-byte aligned");
    const AdamRowsDev e = {emb->param, emb->exp_avg, emb->exp_avg_sq, emb->last, emb->l2, nullptr, nullptr};
    const AdamRowsDev l = lin ? AdamRowsDev{lin->param, lin->exp_avg, lin->exp_avg_sq, lin->last, lin->l2, nullptr, nullptr} : e;
    const bool by_row = adam_by_row(D);
    const int QT = by_row ? (lin ? 2 : 1) : (D + 3) / 4 + ((D & 3) ? 1 : 0) + (lin ? 1 : 0);      // threads per (example, field)
    const long threads = (long)B * m * QT;
    dim3 grid((unsigned)ceil_div(threads, (long)ADAM_THREADS));
    // rider: deferred |W| maxima of the CIN weight packs (xdfm_cin_pack_defer) go out as workgroups behind the catch-up's own
    const int own_blocks = (int)grid.x;
    X3PackJobs riders = {};
    grid.x += (unsigned)x3_pack_take_absmax((hipStream_t)stream, &riders);
    if (by_row)
        hipLaunchKernelGGL(adam_catchup_by_row_kernel, grid, dim3(ADAM_THREADS), 0, (hipStream_t)stream, X, ldx, B, cols, vocab, m, D,
                           e, l, lin ? 1 : 0, clk->clock, clk->consts, beta1, beta2, eps, reinterpret_cast<unsigned long long*>(backlog),
                           own_blocks, riders);
    else
        hipLaunchKernelGGL(adam_catchup_rows_kernel, grid, dim3(ADAM_THREADS), 0, (hipStream_t)stream, X, ldx, B, cols, vocab, m, D,
                           e, l, lin ? 1 : 0, clk->clock, clk->consts, beta1, beta2, eps, reinterpret_cast<unsigned long long*>(backlog),
                           own_blocks, riders);
    return xdfm_check_launch("adam_catchup_rows");
}

// the checks of xdfm_adam_apply_rows (and of the rows half of xdfm_colaunch_adam_step), before any device work
static int adam_apply_rows_check(const char* what, const float* X, const int* cols, const int* vocab, int B, int m, int D,
                                 const xdfm_adam_rows* emb, const xdfm_adam_rows* lin, const xdfm_adam_clock* clk, float* l2_cell) {
    XDFM_REQUIRE(X && cols && vocab && emb && clk && l2_cell, "%s: null pointer", what);
    if (int rc = adam_clock_ok(what, clk)) return rc;
    XDFM_REQUIRE(emb->last && (!lin || lin->last), "%s: `last` tables missing", what);
    XDFM_REQUIRE(emb->grad && emb->marks && (!lin || (lin->grad && lin->marks)), "%s: gradient / mark tables missing", what);
    XDFM_REQUIRE(B > 0 && m > 0 && D > 0, "%s: bad shape B=%d m=%d D=%d", what, B, m, D);
    XDFM_REQUIRE((((size_t)l2_cell) & 7) == 0, "%s: l2_cell must be 8-byte aligned", what);
    return XDFM_OK;
}
// ... and its kernel arguments; -> the workgroups of the rows grid
static int adam_apply_rows_args(AdamRowsArgs& a, bool by_row, const float* X, long ldx, int B, const int* cols, const int* vocab, int m,
                                int D, const xdfm_adam_rows* emb, const xdfm_adam_rows* lin, float* l2_cell) {
    const AdamRowsDev e = {emb->param, emb->exp_avg, emb->exp_avg_sq, emb->last, emb->l2, emb->grad, emb->marks};
    const AdamRowsDev l = lin ? AdamRowsDev{lin->param, lin->exp_avg, lin->exp_avg_sq, lin->last, lin->l2, lin->grad, lin->marks} : e;
    a = AdamRowsArgs{X, ldx, B, cols, vocab, m, D, e, l, lin ? 1 : 0, reinterpret_cast<unsigned long long*>(l2_cell)};
    const int QT = by_row ? (lin ? 2 : 1) : (D + 3) / 4 + ((D & 3) ? 1 : 0) + (lin ? 1 : 0);
    const long threads = (long)B * m * QT + 8L * m;
    return (int)ceil_div(threads, (long)ADAM_THREADS);
}

int xdfm_adam_apply_rows(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                         const xdfm_adam_rows* emb, const xdfm_adam_rows* lin, const xdfm_adam_clock* clk,
                         double beta1, double beta2, double eps, float* l2_cell, float* l2_value, void* stream) {
    if (int rc = adam_apply_rows_check("adam_apply_rows", X, cols, vocab, B, m, D, emb, lin, clk, l2_cell)) return rc;
    const bool by_row = adam_by_row(D);
    AdamRowsArgs a;
    const dim3 grid((unsigned)adam_apply_rows_args(a, by_row, X, ldx, B, cols, vocab, m, D, emb, lin, l2_cell));
    hipStream_t st = (hipStream_t)stream;
    if (by_row)
        hipLaunchKernelGGL(adam_apply_by_row_kernel, grid, dim3(ADAM_THREADS), 0, st, X, ldx, B, cols, vocab, m, D, a.emb, a.lin, a.has_lin,
                           clk->clock, clk->consts, beta1, beta2, eps, a.cell);
    else
        hipLaunchKernelGGL(adam_apply_rows_kernel, grid, dim3(ADAM_THREADS), 0, st, X, ldx, B, cols, vocab, m, D, a.emb, a.lin, a.has_lin,
                           clk->clock, clk->consts, beta1, beta2, eps, a.cell);
    if (int rc = xdfm_adam_rows_finish(reinterpret_cast<unsigned long long*>(l2_cell), l2_value, st)) return rc;
    return xdfm_check_launch("adam_apply_rows");
}

int xdfm_colaunch_adam_step(const xdfm_adam_tensor* tensors, int T, const xdfm_adam_clock* clk, double lr,
                            const double* lr_dev, double beta1, double beta2, double eps, float* l2_ws, float* l2_value,
                            const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                            const xdfm_adam_rows* emb, const xdfm_adam_rows* lin, float* l2_cell, void* stream) {
    // both halves' arguments are checked before either launches
    XDFM_REQUIRE(!(clk && clk->clock && clk->consts && clk->cap > 256), "colaunch_adam_step: bad clock (cap %d > 256)", clk->cap);
    if (int rc = adam_apply_rows_check("colaunch_adam_step", X, cols, vocab, B, m, D, emb, lin, clk, l2_cell)) return rc;
    // option "colaunch" bit 0 clear (or the cached-access experiment of "dbg"): the two calls, launch for launch
    const bool pair = (xdfm_opt(OPT_COLAUNCH) & 1) && !(xdfm_opt(OPT_DBG) & (1 << 17));
    xdfm_opt_note(OPT_LAST_COLAUNCH, pair ? 1 : 0);
    if (!pair) {
        if (int rc = xdfm_adam_step_deferred(tensors, T, clk, lr, lr_dev, beta1, beta2, eps, l2_ws, l2_value, stream)) return rc;
        return xdfm_adam_apply_rows(X, ldx, B, cols, vocab, m, D, emb, lin, clk, beta1, beta2, eps, l2_cell, l2_value, stream);
    }
    const bool by_row = adam_by_row(D);
    AdamRowsArgs a;
    const int rows_blocks = adam_apply_rows_args(a, by_row, X, ldx, B, cols, vocab, m, D, emb, lin, l2_cell);
    if (int rc = adam_step_impl(tensors, T, clk, lr, lr_dev, beta1, beta2, eps, l2_ws, l2_value, stream, &a, by_row, rows_blocks)) return rc;
    if (int rc = xdfm_adam_rows_finish(reinterpret_cast<unsigned long long*>(l2_cell), l2_value, (hipStream_t)stream)) return rc;
    return xdfm_check_launch("colaunch_adam_step");
}

int xdfm_adam_flush(const xdfm_adam_tensor* tensors, int T, const xdfm_adam_clock* clk, double beta1, double beta2,
                    double eps, float* backlog, void* stream) {
    XDFM_REQUIRE(tensors && clk && backlog, "adam_flush: null pointer");     // (the clock is checked in front of the count here)
    if (int rc = adam_clock_ok("adam_flush", clk)) return rc;
    XDFM_REQUIRE(T > 0 && T <= 65535, "adam_flush: bad tensor count %d", T);
    XDFM_REQUIRE((((size_t)backlog) & 7) == 0, "adam_flush: backlog must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> order;
    for (int t = 0; t < T; ++t)
        if (tensors[t].flags & XDFM_ADAM_DEFERRED) {
            XDFM_REQUIRE(tensors[t].last && tensors[t].param && tensors[t].exp_avg && tensors[t].exp_avg_sq,
                         "adam_flush: tensor %d has a null pointer", t);
            order.push_back(t);
        }
    auto launch = [&](const AdamBatch& batch, int cnt, int, int) {
        hipLaunchKernelGGL(adam_flush_kernel, dim3(batch.first[cnt]), dim3(ADAM_THREADS), 0, st, batch, cnt, clk->clock, clk->consts,
                           beta1, beta2, eps, reinterpret_cast<unsigned long long*>(backlog));
    };
    tbl_launches<AdamBatch>(order, false, [&](int t) { return adam_dev(tensors[t]); }, ADAM_BLOCK_ELEMS, ADAM_FLUSH_BX, launch);
    hipLaunchKernelGGL(adam_clock_reset_kernel, dim3(1), dim3(64), 0, st, clk->clock);
    return xdfm_check_launch("adam_flush");
}

int xdfm_adam_selftest(int mode, unsigned long long n, unsigned long long seed, double lr, double beta1, double beta2, double eps,
                       unsigned long long* out, void* stream) {
    XDFM_REQUIRE(out && mode >= 0 && mode <= 3 && n > 0 && n <= (1ull << 34), "adam_selftest: bad arguments");
    const unsigned long long per = 1ull << 30;           // a launch holds fewer than 2^32 threads
    for (unsigned long long base = 0; base < n; base += per) {
        const unsigned long long cnt = n - base < per ? n - base : per;
        hipLaunchKernelGGL(adam_selftest_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mode, base, n,
                           seed, lr, beta1, beta2, eps, out);
    }
    return xdfm_check_launch("adam_selftest");
}

}  // extern "C"
