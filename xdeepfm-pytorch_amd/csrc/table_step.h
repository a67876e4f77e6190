// What the table optimizers' translation units share beside their arithmetic (adam_math.h, opt_math.h): K7 / K7d
// (adam.hip), K7s / K7g / K7r (sgd_adagrad.hip), K7sd / K7gd / K7rd (sgd_adagrad_deferred.hip) and K7f (ftrl.hip).
//   device: the streaming float4 accesses, and the claim of a deferred chunk (or of a row's chunks) through `last`
//   host:   the composition of a launch -- which tensors it takes, and each tensor's share of its 1-D grid
// Everything here is inlined into the kernels and launchers of the four files; none of it has a symbol of its own.
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

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
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
