// Riders (option "colaunch" bit 2, xdfm_rider_begin in include/xdfm.h): a small body that depends on nothing near it leaves
// inside the next suitable launch instead of alone.  The one rider body so far is the ordered sum of a CIN level's dW slabs
// (cin_x3_bww.hip): it depends on that level's dW kernel only, and nothing reads dW before the optimizer.  Between
// xdfm_rider_begin and xdfm_rider_flush it is not launched but recorded, and a host launch on the same stream takes the
// recorded jobs: a by-value table behind the host's own arguments; workgroups past the host's own grid run the rider body
// and return.  Hosts: x3_bwd_prep_kernel of the next level down (cin_x3_bww.hip) and embed_scatter_grouped_kernel
// (embed.hip), which runs behind level 0.  One thread per element, the splits in their fixed order: the same bits from any
// block size.  What nobody carried leaves in xdfm_rider_flush as one launch (x3_unpack_rider_kernel).
#pragma once
#include "xdfm_internal.h"

#define X3_RIDERS 4
struct X3UnpackJob { const float* dWt; float* dW; long slab_stride; int H, Hp, m, Hpad, IPAD, nslab, sym; };   // slab_stride = elements = threads
struct X3UnpackRiders { X3UnpackJob j[X3_RIDERS]; int n; };

// host (cin_x3_bww.hip holds the recorded jobs): the table for a host launch of `threads`-wide workgroups on `st`, taken only
// if it needs at most max_blocks workgroups -> that number (0: nothing taken, *out has n = 0)
long x3_riders_take(hipStream_t st, int threads, long max_blocks, X3UnpackRiders* out);

#ifdef __HIPCC__
// dW[h][i*m+j] = sum over n-splits of dWt[split][j][h][i], in split order (the kernel removed each split's scales)
__device__ __forceinline__ void x3_bww_unpack_one(const float* __restrict__ dWt, int H, int Hp, int m,
                                                  int Hpad, int IPAD, int nslab, long slab_stride, float* __restrict__ dW, const long idx) {
    const long total = (long)m * Hpad * IPAD;
    if (idx >= total) return;
    const int i = (int)(idx % IPAD);
    const long jh = idx / IPAD;
    const int h = (int)(jh % Hpad), j = (int)(jh / Hpad);
    if (i >= Hp || h >= H) return;
    float acc = 0.f;
    int k = 0;
    for (; k + 8 <= nslab; k += 8) {                    // 8 slab loads in flight; the sum keeps its fixed order
        float t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = dWt[(long)(k + q) * slab_stride + idx];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += t[q];
    }
    for (; k < nslab; ++k) acc += dWt[(long)k * slab_stride + idx];
    dW[(long)h * ((long)Hp * m) + (long)i * m + j] = acc;
}

// folded level 0: dW[h][i*m+j] = dW[h][j*m+i] = sum over n-splits of slab[split][t][h][r], (i, j) the pair of lane r in
// combined tile t.  One thread per slab element (coalesced reads of every split), two 4-byte stores.
__device__ __forceinline__ void x3_bww_unpack_sym_one(const float* __restrict__ dWt, int H, int m,
                                                      int Hpad, int nslab, long slab_stride, float* __restrict__ dW, const long idx) {
    if (idx >= (long)(m / 2) * Hpad * 32) return;
    const int r = (int)(idx & 31);
    const int h = (int)((idx >> 5) % Hpad), t = (int)((idx >> 5) / Hpad);
    int i, j;
    if (r <= t) { i = r; j = t; }
    else if (31 - r <= m - 1 - t) { i = 31 - r; j = m - 1 - t; }
    else return;
    if (h >= H) return;
    float acc = 0.f;
    int k = 0;
    for (; k + 8 <= nslab; k += 8) {                    // 8 slab loads in flight; the sum keeps its fixed order
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = dWt[(long)(k + q) * slab_stride + idx];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += v[q];
    }
    for (; k < nslab; ++k) acc += dWt[(long)k * slab_stride + idx];
    const float v = acc;
    float* __restrict__ row = dW + (long)h * ((long)m * m);
    row[i * m + j] = v;
    if (i != j) row[j * m + i] = v;
}

// rider workgroup `rb` of the table, in a launch of blockDim.x-wide workgroups: the job it falls into (each job takes
// ceil(elements / blockDim.x) workgroups, as x3_riders_take counted them) and its elements there
__device__ __forceinline__ void x3_unpack_rider(const X3UnpackRiders& R, long rb) {
    const long bt = (long)blockDim.x;
#pragma unroll
    for (int k = 0; k < X3_RIDERS; ++k) {
        if (k >= R.n) return;
        const X3UnpackJob& J = R.j[k];
        const long blocks = (J.slab_stride + bt - 1) / bt;
        if (rb < blocks) {
            const long idx = rb * bt + threadIdx.x;     // the bodies bound idx by the job's element count themselves
            if (J.sym) x3_bww_unpack_sym_one(J.dWt, J.H, J.m, J.Hpad, J.nslab, J.slab_stride, J.dW, idx);
            else x3_bww_unpack_one(J.dWt, J.H, J.Hp, J.m, J.Hpad, J.IPAD, J.nslab, J.slab_stride, J.dW, idx);
            return;
        }
        rb -= blocks;
    }
}
#endif
