// What the table optimizers' translation units share beside their arithmetic (adam_math.h, opt_math.h): K7 / K7d
// (adam.hip), K7s / K7g / K7r / K7m (sgd_adagrad.hip), their deferred forms (sgd_adagrad_deferred.hip), K7f (ftrl.hip) and K7w
// (rowwise.hip).
//   device: the streaming float4 accesses; the claim of a deferred chunk (or of a row's chunks) through `last`; the mark scan
//           (tbl_mark_scan); the block's L2 partial (tbl_l2_slot); and THE SWEEP (tbl_sweep): the one body of opt_step_kernel<K>
//           and ftrl_step_kernel, over a rule that names the state arrays and forwards to the element update
//   host:   the arguments every step checks (tbl_check_call, tbl_check_l2) and the composition of a step's launches (tbl_launches) -- which
//           tensors a launch takes, each tensor's share of its 1-D grid, the launch's first L2 slot
// Everything here is inlined into the kernels and launchers of those files; none of it has a symbol of its own.
#pragma once
#include "xdfm_internal.h"

#include <algorithm>
#include <vector>

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
// Streaming accesses: p and the optimizer's state are read once and written once per pass (14 GB of them per Adam step at
// Criteo-card vocabularies) -- non-temporal.  NT = false: ordinary cached accesses, for experiments.
typedef float tbl_v4f __attribute__((ext_vector_type(4)));
// wave-uniform chunk pointer + this lane's byte offset (32-bit: the access becomes scalar base + vector offset)
__device__ __forceinline__ float4* at4(float4* base, unsigned byte_off) {
    return reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + byte_off);
}
template <bool NT>
__device__ __forceinline__ float4 tbl_ld(const float4* a) {
    if constexpr (!NT) return *a;
    const tbl_v4f t = __builtin_nontemporal_load(reinterpret_cast<const tbl_v4f*>(a));
    return make_float4(t.x, t.y, t.z, t.w);
}
template <bool NT>
__device__ __forceinline__ void tbl_st(float4* a, const float4& x) {
    if constexpr (!NT) { *a = x; return; }
    const tbl_v4f t = {x.x, x.y, x.z, x.w};
    __builtin_nontemporal_store(t, reinterpret_cast<tbl_v4f*>(a));
}

// The claim of chunk `cc` of a deferred table for step `t`: the first thread to reach the chunk in a launch sets its `last`
// byte to t (CAS on the word that holds it) and gets the step the chunk was at, which it has to bring the chunk up from;
// duplicates of an id, and a chunk that is at t already, get -1.
__device__ __forceinline__ int tbl_claim(unsigned char* last, long cc, int t) {
    unsigned* word = reinterpret_cast<unsigned*>(last + (cc & ~3L));
    const int sh = (int)(cc & 3) * 8;
    unsigned seen = *word;              // a plain (cached) read: stale at worst, and then the CAS below returns the current word
    int old = -1;
    while (true) {
        const int ob = (int)((seen >> sh) & 255u);
        if (ob >= t) break;
        const unsigned want = (seen & ~(255u << sh)) | ((unsigned)t << sh);
        const unsigned got = atomicCAS(word, seen, want);
        if (got == seen) { old = ob; break; }
        seen = got;
    }
    return old;
}

// The claim of the n <= 8 consecutive chunks cc0 .. cc0 + n - 1 (a table row, or a piece of one) by ONE thread: per `last`
// word the chunks' bytes fall into, one CAS that sets every one of them that is below t to t.  The other bytes of the word
// (2 or 4 rows share a word at D = 8 / 4, and their lanes sit in the same wave) pass through as they were seen; a CAS that
// finds the word changed starts over from the word it returned, where more of the row's bytes may be at t by then.
// -> byte j = the step chunk cc0 + j was at, which the caller has to bring it up from, or 255 (never a step: t <= 255)
// for a chunk that is at t already -- someone else's, or done -- and for j >= n.
__device__ __forceinline__ unsigned long long tbl_claim_row(unsigned char* last, long cc0, int n, int t) {
    unsigned long long olds = ~0ull;
    const long end = cc0 + n;
    for (long w0 = cc0 & ~3L; w0 < end; w0 += 4) {
        unsigned* word = reinterpret_cast<unsigned*>(last + w0);
        const int lo = (int)(cc0 - w0), hi = (int)(end - w0);       // the row's bytes of this word: lo <= b < hi
        unsigned seen = *word;          // plain read, as tbl_claim's
        while (true) {
            unsigned mine = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b >= lo && b < hi && ((seen >> (8 * b)) & 255u) < (unsigned)t) mine |= 255u << (8 * b);
            if (!mine) break;
            const unsigned want = (seen & ~mine) | (((unsigned)t * 0x01010101u) & mine);
            const unsigned got = atomicCAS(word, seen, want);
            if (got == seen) {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if ((mine >> (8 * b)) & 1u) {
                        const int sh = 8 * (b - lo);                 // b - lo = the chunk's index in the run (lo < 0: later words)
                        olds = (olds & ~(255ull << sh)) | ((unsigned long long)((seen >> (8 * b)) & 255u) << sh);
                    }
                break;
            }
            seen = got;
        }
    }
    return olds;
}

// The scan of a tensor's mark bytes (one per 16-byte chunk, n4 of them) by a grid of `stride` threads: process(e) for every
// marked chunk e.  The bytes are read 16 at a time (one uint4 per lane and load: the sweep over 144 M marks at Criteo-card
// vocabularies is what a step without an L2 term costs), two groups per thread in flight; the chunks in front of the marks'
// first 16-byte boundary and behind the last whole group go one by one.
template <class Process>
__device__ __forceinline__ void tbl_mark_scan(const unsigned char* marks, long n4, long tid, long stride, Process process) {
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
    if (q < groups) group(m16[q], head + q * 16);       // this thread's last, unpaired group
    for (long e = tid; e < head; e += stride)
        if (marks[e]) process(e);
    for (long e = head + groups * 16 + tid; e < n4; e += stride)
        if (marks[e]) process(e);
}

// The block's share of a tensor's L2 term: l2c * (the block's sum of `sq`), added in a fixed order -- the wave by a butterfly,
// the four waves as (w0 + w1) + (w2 + w3) -- and written by thread 0 to l2_part[slot], one slot per block of the step in launch
// order (the finish adds the slots in that order).  Every thread of the block calls it; l2_part == nullptr: nothing is wanted.
template <int THREADS>
__device__ __forceinline__ void tbl_l2_slot(float sq, float l2c, float* __restrict__ l2_part, int slot) {
    static_assert(THREADS == 256, "four waves");
    if (!l2_part) return;
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    __shared__ float wsum[THREADS / 64];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) l2_part[slot] = l2c * ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}

// A tensor as the sweep sees it, NS state arrays beside p (SGD's one is never dereferenced), and a launch's tensors: first[k] =
// first block of tensor k in the launch's 1-D grid, first[cnt] = the grid's size (tbl_grid).  By value in the kernel arguments.
template <int NS>
struct SweepDev { float* param; float* grad; float* st[NS > 0 ? NS : 1]; unsigned char* grad_marks; long numel; float l2; };
template <int NS, int CHUNK>
struct SweepBatch { SweepDev<NS> t[CHUNK]; int first[CHUNK + 1]; };

// THE SWEEP: one step over the tensors of a launch, for workgroup `bid` of its 1-D grid.  A Rule brings
//   NS    state arrays streamed beside p (0, 1, 2)          NF    chunks per array and thread in flight
//   SKIP  an unmarked chunk of a tensor without an L2 term is an exact no-op and is not read
//   Ctx   the rate as the rule wants it, and its hyper-parameters
//   four(P, S, G, g2, ctx, sq) / one(p, s, g, g2, ctx, sq): the element update of a chunk / of one element (opt_math.h), S and s
//         arrays of max(NS, 1)
// Three ways through a tensor, the same bits on each: marks and SKIP and no L2 term -- the mark scan, which touches marked
// chunks only; marks otherwise -- every chunk is a real update, the mark bytes are loaded first and the (rare) gradient reads
// sit behind one branch; no marks -- a dense gradient, read in full and left alone.  Whole-block iterations hold NF chunks per
// array and address by a wave-uniform base plus one 32-bit lane offset.  The gradient of an unmarked chunk is an opaque zero:
// it enters the same instruction sequence as a loaded one (with a literal 0 the compiler folds fmaf(2 l2, w, 0) into a product
// and contracts it into the next operation, which rounds differently from the dense path).  A marked gradient is re-zeroed and
// unmarked as it is read (each lane owns its chunk's mark, so nothing races).
// The state loads are a loop over NS plus `if constexpr (NS == 0)` for SGD's unused array, and the whole-block loops are
// written out, not lambdas: either way round hipcc gave opt_step_kernel<0> 146 VGPRs for 139.
template <class Rule, int THREADS, class Batch>
__device__ __forceinline__ void tbl_sweep(const Batch& batch, int cnt, int slot0, const typename Rule::Ctx& ctx,
                                          float* __restrict__ l2_part, const int bid) {
    constexpr int NF = Rule::NF, NS = Rule::NS, NA = NS > 0 ? NS : 1;
    int ti = 0;                                        // wave-uniform search
    for (int k = 1; k < cnt; ++k) ti += bid >= batch.first[k] ? 1 : 0;
    const int lb = bid - batch.first[ti];              // this block among the tensor's nb blocks
    const int nb = batch.first[ti + 1] - batch.first[ti];
    const auto& d = batch.t[ti];
    float* __restrict__ p = d.param;
    float* __restrict__ g = d.grad;
    unsigned char* __restrict__ marks = d.grad_marks;
    const long n = d.numel;
    const float l2c = d.l2;
    const float g2 = 2.f * l2c;                        // d(l2 * w^2)/dw = 2 l2 w
    float sq = 0.f;
    const long tid = (long)lb * THREADS + threadIdx.x;
    const long stride = (long)nb * THREADS;
    size_t bits = ((size_t)p) | ((size_t)g);
    float* s[NA];
    float4* s4[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        s[j] = j < NS ? d.st[j] : d.param;
        s4[j] = reinterpret_cast<float4*>(s[j]);
        bits |= (size_t)s[j];
    }
    const long n4 = (bits & 15) == 0 ? n / 4 : 0;      // unaligned tensors: everything goes through the scalar loop
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float zf;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
    const float4 zero4 = make_float4(zf, zf, zf, zf);
    const unsigned tx = threadIdx.x, tx16 = tx * 16u;
    // the update of one chunk by its own index, through the streaming accesses
    auto one = [&](long e, const float4& ga, float4& pa, float4 (&sa)[NA]) {
        Rule::four(pa, sa, ga, g2, ctx, sq);
        tbl_st<true>(p4 + e, pa);
#pragma unroll
        for (int j = 0; j < NS; ++j) tbl_st<true>(s4[j] + e, sa[j]);
    };
    long i = tid;
    if (marks && l2c == 0.f && Rule::SKIP) {
        tbl_mark_scan(marks, n4, tid, stride, [&](long e) {
            float4 pa = p4[e], sa[NA];
#pragma unroll
            for (int j = 0; j < NS; ++j) sa[j] = s4[j][e];
            if constexpr (NS == 0) sa[0] = zero4;
            const float4 ga = g4[e];
            g4[e] = zero4; marks[e] = 0;
            Rule::four(pa, sa, ga, g2, ctx, sq);
            p4[e] = pa;
#pragma unroll
            for (int j = 0; j < NS; ++j) s4[j][e] = sa[j];
        });
        i = n4 + tid;                                   // nothing left for the dense loops below
    } else if (marks) {
        long iu = (long)lb * THREADS;
        for (; iu + (NF - 1) * stride + THREADS <= n4; iu += NF * stride) {
            unsigned char k[NF];
            float4 P[NF], S[NF][NA], G[NF];
            unsigned any = 0;
#pragma unroll
            for (int q = 0; q < NF; ++q) { k[q] = (marks + (iu + q * stride))[tx]; any |= k[q]; }
#pragma unroll
            for (int q = 0; q < NF; ++q) {
                P[q] = tbl_ld<true>(at4(p4 + (iu + q * stride), tx16));
#pragma unroll
                for (int j = 0; j < NS; ++j) S[q][j] = tbl_ld<true>(at4(s4[j] + (iu + q * stride), tx16));
                if constexpr (NS == 0) S[q][0] = zero4;
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
                Rule::four(P[q], S[q], G[q], g2, ctx, sq);
                tbl_st<true>(at4(p4 + (iu + q * stride), tx16), P[q]);
#pragma unroll
                for (int j = 0; j < NS; ++j) tbl_st<true>(at4(s4[j] + (iu + q * stride), tx16), S[q][j]);
            }
        }
        i = iu + tx;
        for (; i < n4; i += stride) {
            const unsigned char ka = marks[i];
            float4 pa = tbl_ld<true>(p4 + i), sa[NA];
#pragma unroll
            for (int j = 0; j < NS; ++j) sa[j] = tbl_ld<true>(s4[j] + i);
            if constexpr (NS == 0) sa[0] = zero4;
            float4 ga = zero4;
            if (ka) { ga = g4[i]; g4[i] = zero4; marks[i] = 0; }
            one(i, ga, pa, sa);
        }
    }
    long iu = i - tx;                                   // dense gradient
    for (; iu + (NF - 1) * stride + THREADS <= n4; iu += NF * stride) {
        float4 P[NF], S[NF][NA], G[NF];
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            P[q] = tbl_ld<true>(at4(p4 + (iu + q * stride), tx16));
            G[q] = tbl_ld<true>(at4(g4 + (iu + q * stride), tx16));
#pragma unroll
            for (int j = 0; j < NS; ++j) S[q][j] = tbl_ld<true>(at4(s4[j] + (iu + q * stride), tx16));
            if constexpr (NS == 0) S[q][0] = zero4;
        }
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            Rule::four(P[q], S[q], G[q], g2, ctx, sq);
            tbl_st<true>(at4(p4 + (iu + q * stride), tx16), P[q]);
#pragma unroll
            for (int j = 0; j < NS; ++j) tbl_st<true>(at4(s4[j] + (iu + q * stride), tx16), S[q][j]);
        }
    }
    i = iu + tx;
    for (; i < n4; i += stride) {
        float4 pa = tbl_ld<true>(p4 + i), sa[NA];
#pragma unroll
        for (int j = 0; j < NS; ++j) sa[j] = tbl_ld<true>(s4[j] + i);
        if constexpr (NS == 0) sa[0] = zero4;
        const float4 ga = tbl_ld<true>(g4 + i);
        one(i, ga, pa, sa);
    }
    for (long k = 4 * n4 + tid; k < n; k += stride) {  // the numel % 4 tail (always read); whole unaligned tensors
        float pa = p[k], sa[NA];
#pragma unroll
        for (int j = 0; j < NS; ++j) sa[j] = s[j][k];
        if constexpr (NS == 0) sa[0] = zf;
        Rule::one(pa, sa, g[k], g2, ctx, sq);
        p[k] = pa;
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j][k] = sa[j];
        if (marks) { g[k] = 0.f; marks[k >> 2] = 0; }
    }
    tbl_l2_slot<THREADS>(sq, l2c, l2_part, slot0 + bid);
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// What every step's entry point checks first: the tensor array (and whatever else must not be null: `pointers`) and their
// count; and, behind the entry point's own hyper-parameter checks -- a call with two mistakes reports the one it always
// reported --, that an L2 value has a workspace for its partials.
static inline int tbl_check_call(const char* what, bool pointers, int T) {
    XDFM_REQUIRE(pointers, "%s: null pointer", what);
    XDFM_REQUIRE(T > 0 && T <= 65535, "%s: bad tensor count %d", what, T);
    return XDFM_OK;
}
static inline int tbl_check_l2(const char* what, const float* l2_ws, const float* l2_value) {
    XDFM_REQUIRE(!l2_value || l2_ws, "%s: l2_value needs l2_ws", what);
    return XDFM_OK;
}

// The order in which a step's tensors are dealt to its launches: by falling size (stable, so a pure function of the
// sizes); launch l of n takes order[l], order[l + n], ...  Every launch then streams its share of the big tables and the
// small tensors' latency-bound blocks run underneath (a launch of small tensors alone took 25 us for 30 MB).
template <class Tensor>
static inline std::vector<int> tbl_launch_order(const Tensor* tensors, int T) {
    std::vector<int> order(T);
    for (int t = 0; t < T; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tensors[a].numel > tensors[b].numel; });
    return order;
}

// The 1-D grid of a launch over batch.t[0 .. cnt): first[k] = first block of tensor k, first[cnt] = the grid's size.  A
// tensor's share follows its size -- one block per `block_elems` elements, at least 1 and at most `cap` -- so a launch that
// holds four 10 M-row tables and thirty small tensors is 16 000 blocks of table sweep, not 128 per tensor.  The unused
// descriptors repeat t[0] (the kernels' search stops at cnt; nothing in the argument block is left undefined).
template <class Batch>
static inline void tbl_grid(Batch& batch, int cnt, long block_elems, int cap) {
    constexpr int N = (int)(sizeof(batch.t) / sizeof(batch.t[0]));
    for (int k = cnt; k < N; ++k) batch.t[k] = batch.t[0];
    batch.first[0] = 0;
    for (int k = 0; k < N; ++k) {
        long nb = k < cnt ? ceil_div(batch.t[k].numel, block_elems) : 0;
        if (k < cnt && nb < 1) nb = 1;
        if (nb > cap) nb = cap;
        batch.first[k + 1] = batch.first[k] + (int)nb;
    }
}

// The launches of one call over the tensors order[0 .. n): Batch holds CHUNK descriptors, so there are ceil(n / CHUNK) of them.
// deal: launch l of nl takes order[l], order[l + nl], ... (with tbl_launch_order: every launch gets its share of the big
// tables); else it takes the next CHUNK in the order given.  Per launch: the descriptors through dev_of(index), the grid
// (tbl_grid), then launch(batch, cnt, slot0, l) issues it -- slot0 = the blocks of the launches before it, which is where its L2
// partials start.  -> the blocks of all launches.
template <class Batch, class DevOf, class Launch>
static inline int tbl_launches(const std::vector<int>& order, bool deal, DevOf dev_of, long block_elems, int cap, Launch launch) {
    constexpr int CHUNK = (int)(sizeof(Batch::t) / sizeof(Batch::t[0]));
    const int n = (int)order.size(), nl = ceil_div(n, CHUNK);
    int slot0 = 0;
    for (int l = 0; l < nl; ++l) {
        Batch batch;
        int cnt = 0;
        if (deal) for (int k = l; k < n; k += nl) batch.t[cnt++] = dev_of(order[k]);
        else for (int k = l * CHUNK; k < n && cnt < CHUNK; ++k) batch.t[cnt++] = dev_of(order[k]);
        tbl_grid(batch, cnt, block_elems, cap);
        launch(batch, cnt, slot0, l);
        slot0 += batch.first[cnt];
    }
    return slot0;
}
// ... of a step over tensors[0 .. T): sorted by size and dealt
template <class Batch, class Tensor, class DevOf, class Launch>
static inline int tbl_step_launches(const Tensor* tensors, int T, DevOf dev_of, long block_elems, int cap, Launch launch) {
    return tbl_launches<Batch>(tbl_launch_order(tensors, T), true, [&](int t) { return dev_of(tensors[t]); }, block_elems, cap, launch);
}
// ... and the order 0 .. T - 1 for the calls that take their tensors as they come
static inline std::vector<int> tbl_in_order(int T) {
    std::vector<int> order(T);
    for (int t = 0; t < T; ++t) order[t] = t;
    return order;
}
