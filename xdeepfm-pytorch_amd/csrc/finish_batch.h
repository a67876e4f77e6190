// The "finish" arithmetic of the kernels that leave per-block partials (dbias of a CIN level, the split slabs of a dense dW,
// column sums, the head's loss and parameter gradients, K7's L2 value, the deferred rows' L2 cell): one __device__ body per
// family, called by the family's own one-purpose finish kernel (cin_bwd.hip, dnn.hip, reg.hip, adam.hip) and by
// finish_multi_kernel (api.hip), which runs the finishes a batch has collected in ONE launch.  Every body adds in the order and
// over the (virtual) thread count of the kernel it came from, whatever block runs it: the bits do not depend on the route.
#pragma once
#include "xdfm_internal.h"

#define FINISH_THREADS 256         // workgroup of finish_multi_kernel
#define FINISH_MAX_JOBS 16         // jobs per launch (the table travels in the kernel arguments); more jobs: more launches

#define DN_MAX_SPLIT 32            // dense dW: most splits of the contraction (dnn.hip)
#define CS_ROWBLK 64               // column sums: row blocks = partials per column (reg.hip)
#define HEAD_BLOCKS 128            // head: workgroups = partials per sum (reg.hip)
#define ADAM_FIX 1099511627776.0   // 2^40: fixed-point scale of the L2 backlog (integer adds: order-independent) (adam.hip)
#define ADAM_L2_VTHREADS 1024      // adam_l2_finish: the (virtual) threads whose strided sums and tree fix the order

enum { FJ_CIN_DBIAS = 0, FJ_DENSE_W, FJ_COLSUM, FJ_HEAD_FWD, FJ_HEAD_BWD, FJ_ADAM_L2, FJ_ADAM_ROWS, FJ_ADD, FJ_KINDS };

// One finish.  Fields by kind:
//   FJ_CIN_DBIAS  part [H][gx] -> out[h] (+)= sum_k part[h][k];  i0 = H, i1 = gx, i2 = 1: store 0 + sum (out need not be zeroed)
//   FJ_DENSE_W    part = ws, i0 = nsplit, n0 = out * in, n1 = out, out = dW, out2 = db | NULL, i1 = element blocks;
//                 PReLU: part2 = the slope's double partials, i2 = their count, out3 = dalpha | NULL (one more block)
//   FJ_COLSUM     part [CS_ROWBLK][cols] -> out [cols];  i0 = cols
//   FJ_HEAD_FWD   part [HEAD_BLOCKS] -> out[0]
//   FJ_HEAD_BWD   part [HEAD_BLOCKS][KT] -> out [KT];  i0 = KT
//   FJ_ADAM_L2    part [n] -> out[0];  i0 = n
//   FJ_ADAM_ROWS  cell -> out[0] += cell / 2^40 (out may be NULL), cell = 0
//   FJ_ADD        add_out[0] = add_a[0] + add_b[0]
// Tails, run by the thread that wrote out[0], in this order, so that finishes that feed each other may share a launch:
// `cell` on an FJ_ADAM_L2 job = the FJ_ADAM_ROWS finish on the same out; `add_a` on either = add_out[0] = add_a[0] + out[0].
struct FinishJob {
    int kind, blocks;
    const void* part; const void* part2;
    void* out; void* out2; void* out3;
    long n0, n1;
    int i0, i1, i2;
    unsigned long long* cell;
    const float* add_a; const float* add_b; float* add_out;
};
struct FinishTable {                          // the prefix table in front: one scalar load at the head of the arguments
    int first[FINISH_MAX_JOBS + 1];          // first[k] = first workgroup of job k; the grid from first[n] on
    int n;
    FinishJob j[FINISH_MAX_JOBS];
};

// api.hip.  *taken = true: a batch is open on this device and the job now waits for
// xdfm_finish_batch_run; false: the caller launches its own finish kernel, as it always did.
int xdfm_finish_defer(const FinishJob& job, hipStream_t st, bool* taken);
// the families' finishes: deferred into the open batch, or their own launch (what the producers call after their main kernel)
int xdfm_cin_dbias_finish(const float* part, int H, int gx, float* dbias, hipStream_t st);
int xdfm_dense_w_finish(const float* ws, int nsplit, long mn, long m, float* dW, float* db, bool prelu, const double* dapart, int npart,
                        float* dalpha, hipStream_t st);
int xdfm_colsum_finish(const float* part, int cols, float* out, hipStream_t st);
int xdfm_head_fwd_finish(const float* part, float* loss, hipStream_t st);
int xdfm_head_bwd_finish(const float* part, int KT, float* out, hipStream_t st);
int xdfm_adam_l2_finish(const float* part, int n, float* out, hipStream_t st);
int xdfm_adam_rows_finish(unsigned long long* cell, float* l2_value, hipStream_t st);

#ifdef __HIPCC__
// ---- CIN dbias: thread per row, the row's slots in block order ------------------------------------------------------
__device__ __forceinline__ void cin_dbias_finish_row(int h, const float* __restrict__ part, int H, int gx, float* __restrict__ dbias,
                                                     bool set) {
    if (h >= H) return;
    // eight loads in flight, then their adds in slot order: a batch read long after its producer waits for memory once per
    // eight slots, not once per slot (a slot past the end is loaded from the last one and not added)
    const float* __restrict__ row = part + (long)h * gx;
    float s = 0.f;
    for (int k = 0; k < gx; k += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row[k + j < gx ? k + j : gx - 1];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k + j < gx) s += v[j];
    }
    if (set) dbias[h] = 0.f + s;          // what `+=` leaves in a zeroed cell (-0 becomes +0)
    else dbias[h] += s;
}

// ---- dense dW: thread per element ---------------------------------------------------------------------------------
// dW[e] = sum over the splits of slab[z][e], db[c] likewise, over a fixed pairwise tree: eight splits at a time, then the
// (at most DN_MAX_SPLIT / 8) sums of eight.  A running sum in split order rounds once per split at the magnitude of the total:
// at 29 splits the bias gradient's error was 3 ulp, three times that of a pairwise column sum of the same values.
__device__ __forceinline__ void dn_finish_elem(long e, const float* __restrict__ ws, int nsplit, long mn, long m,
                                               float* __restrict__ dW, float* __restrict__ db) {
    const long total = mn + (db ? m : 0);
    if (e >= total) return;
    const float* p = e < mn ? ws + e : ws + (long)nsplit * mn + (e - mn);
    const long pitch = e < mn ? mn : m;
    float q[DN_MAX_SPLIT / 8];
#pragma unroll
    for (int i = 0; i < DN_MAX_SPLIT / 8; ++i) {
        const int z = 8 * i;
        q[i] = 0.f;
        if (z < nsplit) {                              // uniform; eight loads in flight, a split past the end counts as 0
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = p[(long)(z + j < nsplit ? z + j : nsplit - 1) * pitch];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = z + j < nsplit ? v[j] : 0.f;
            q[i] = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        }
    }
    static_assert(DN_MAX_SPLIT == 32, "the tree below adds four sums of eight splits");
    const float sum = (q[0] + q[1]) + (q[2] + q[3]);
    if (e < mn) dW[e] = sum;
    else db[e - mn] = sum;
}
// the PReLU slope's gradient, one workgroup of 256: thread t adds the partials of index t, t + 256, ... in order, then
// xdfm_block_sum_f64 -- in double, rounded once.  sm: 4 doubles of LDS.
__device__ __forceinline__ void dn_dalpha_finish_block(const double* __restrict__ dapart, int npart, float* __restrict__ dalpha, double* sm) {
    double s = 0.0;
    for (int i = threadIdx.x; i < npart; i += 256) s += dapart[i];
    s = xdfm_block_sum_f64(s, sm);
    if (threadIdx.x == 0) *dalpha = (float)s;
}

// ---- column sums: 64 columns per workgroup of 256, the CS_ROWBLK partials of a column by 4 threads in a fixed order ----
__device__ __forceinline__ void colsum_finish_block(int blk, const float* __restrict__ part, int cols, float* __restrict__ out,
                                                    float* red /* [4][64] */) {
    const int c = blk * 64 + (threadIdx.x & 63);
    const int q = threadIdx.x >> 6;
    float s = 0.f;
    if (c < cols) {
#pragma unroll
        for (int k = 0; k < CS_ROWBLK / 4; ++k) s += part[(long)(q * (CS_ROWBLK / 4) + k) * cols + c];
    }
    red[q * 64 + (threadIdx.x & 63)] = s;
    __syncthreads();
    if (q == 0 && c < cols) out[c] = (red[threadIdx.x] + red[64 + threadIdx.x]) + (red[128 + threadIdx.x] + red[192 + threadIdx.x]);
}

// ---- head: the loss, a tree over the HEAD_BLOCKS partials (workgroup of HEAD_BLOCKS threads or more); the value is in
// red[0] for thread 0 afterwards ---------------------------------------------------------------------------------
__device__ __forceinline__ void head_fwd_finish_block(const float* __restrict__ part, float* red /* [HEAD_BLOCKS] */) {
    if (threadIdx.x < HEAD_BLOCKS) red[threadIdx.x] = part[threadIdx.x];
    __syncthreads();
    for (int o = HEAD_BLOCKS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
}
// ... and the parameter gradients: thread per sum, the blocks' partials in block order
__device__ __forceinline__ void head_bwd_finish_elem(int k, const float* __restrict__ part, int KT, float* __restrict__ out) {
    if (k >= KT) return;
    float s = 0.f;
    for (int b0 = 0; b0 < HEAD_BLOCKS; b0 += 32) {       // 32 loads in flight, then their adds in block order
        float v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = part[(long)(b0 + i) * KT + k];
#pragma unroll
        for (int i = 0; i < 32; ++i) s += v[i];
    }
    out[k] = s;
}

// ---- K7's L2 value: ADAM_L2_VTHREADS virtual threads stride over the partials, then a tree -- by a workgroup of NT real
// threads, each standing for 1024 / NT virtual ones (t, t + NT, ...): the tree's levels above NT are added in registers, in
// the tree's order (with more than 256 partials a stride of 256 would round differently).  acc: NT floats of LDS; the value
// is in acc[0] for thread 0 afterwards.
template <int NT>
__device__ __forceinline__ void adam_l2_finish_block(const float* __restrict__ part, int n, float* acc) {
    constexpr int V = ADAM_L2_VTHREADS / NT;
    static_assert(V >= 1 && V * NT == ADAM_L2_VTHREADS && (V & (V - 1)) == 0, "NT divides 1024 into a power of two");
    float vq[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
        vq[q] = 0.f;
        for (int k = threadIdx.x + q * NT; k < n; k += ADAM_L2_VTHREADS) vq[q] += part[k];
    }
#pragma unroll
    for (int w = V / 2; w >= 1; w >>= 1)
#pragma unroll
        for (int q = 0; q < w; ++q) vq[q] += vq[q + w];
    acc[threadIdx.x] = vq[0];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
        __syncthreads();
    }
}

// ---- the deferred rows' L2 cell (one thread): its value joins l2_value, the cell is ready for the next step ------------
__device__ __forceinline__ void adam_rows_finish_one(unsigned long long* __restrict__ cell, float* __restrict__ l2_value) {
    if (l2_value) l2_value[0] += (float)((double)(long long)cell[0] / ADAM_FIX);
    cell[0] = 0ull;
}
#endif
