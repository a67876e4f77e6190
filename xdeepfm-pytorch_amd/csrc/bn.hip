// K12: batch norm of a dense layer's output fused with its activation (layers.DNN with use_bn=True).
//
// replaces, per layer of deepctr/layers/core.py:120-134 with use_bn: nn.BatchNorm1d (ATen / MIOpen statistics + apply, the
// running-statistics update), the separate activation pass and, backward, threshold_backward / sigmoid_backward + the
// library's batch-norm backward -- four [rows][cols] tensors written per layer forward -- by two launches each way that
// write one tensor each (y forward, dz backward).
//
//   z [rows][ldz] fp32, statistics per column over the rows.
//   training forward   mean_c, var_c (biased) over the rows;  y = act(gamma * (z - mean) * rstd + beta),  rstd = 1 / sqrt(var + eps)
//   evaluation forward the same y from running_mean / running_var
//   backward           gm = act'(y) * g,  xhat = (z - mean) * rstd,
//                      dz = gamma * rstd * (gm - sum(gm) / n - xhat * sum(gm * xhat) / n),  dbeta = sum(gm),  dgamma = sum(gm * xhat)
//
// Statistics.  A row block (BN_ROWBLK rows) leaves the pair (mean, M2 = sum (z - mean)^2) of its rows per column; pairs are
// merged with Chan's formula.  The variance never comes from raw sums of squares: a column 1000 + N(0, 1) would lose all of
// it in fp32 that way (E[z^2] - mean^2 = 1000001 - 1000000 with 0.06 of rounding in each term).  Inside a block every
// thread holds its 16 rows in registers and makes two passes over them (mean, then squared distances).
//
// Precision.  Operands and results are fp32; the statistics, the two backward sums and the per-element arithmetic between
// a load and its store are carried in double (the workspace holds doubles).  These kernels move 8 to 16 bytes per element
// and spend a handful of fp64 operations on it, far below what the memory system leaves room for, and it makes save_mean,
// save_rstd, dgamma and dbeta correctly rounded sums.  It matters for dz over few rows, whose three terms cancel to
// rounding: what is left is then the rounding of the saved fp32 statistics alone.
//
// Geometry.  A block is 4 row groups x 64 columns: a wave reads 64 consecutive columns of one row (one 256-byte dword
// access; the row pitch is arbitrary, so nothing wider is aligned), 16 rows per thread issued together.  Row blocks on
// grid.x, column blocks on grid.y: 4096 x 256 is 64 x 4 = 256 workgroups, one per CU.
//
// Determinism.  No atomics, no zeroed cells: every partial of the workspace is written by exactly one block of launch 1 and
// read by launch 2, whose blocks all merge the same partials in the same order (4 threads per column take a quarter of the
// row blocks each, in index order, then a fixed tree over the four) -- the same bits in every block and on every run.
//
// Synchronised (row-parallel training, opt-in).  Each direction is split where the other ranks' numbers are needed:
// xdfm_bn_stats leaves this rank's merged (mean, M2) pair, the caller all-gathers (count, means, M2s) and
// xdfm_bn_fwd_apply_sync merges the ranks' triples with the same Chan formula in rank order; xdfm_bn_bwd_sums leaves this
// rank's two column sums, the caller all-gathers them and xdfm_bn_bwd_apply_sync adds them in rank order.  Every rank
// computes the global statistics from the same gathered bytes in the same order: the replicas' buffers stay bit-identical.
#include "xdfm_internal.h"

#define BN_ROWBLK 64            // rows per block of launch 1 (and per trip of launch 2)
#define BN_COLBLK 64
#define BN_THREADS 256
#define BN_RPT (BN_ROWBLK / 4)  // rows per thread
#define BN_MAX_APPLY 1024       // row blocks of launch 2's grid; beyond, its blocks walk several row blocks each

struct BnStat { double n, mean, m2; };

// Chan, Golub, LeVeque: the statistics of A followed by B
__device__ __forceinline__ BnStat bn_merge(BnStat a, BnStat b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    BnStat r;
    r.n = a.n + b.n;
    const double d = b.mean - a.mean;
    const double f = b.n / r.n;
    r.mean = fma(d, f, a.mean);
    r.m2 = (a.m2 + b.m2) + d * d * (a.n * f);
    return r;
}

__device__ __forceinline__ float bn_act_fwd(int act, float v) {
    if (act == XDFM_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == XDFM_ACT_SIGMOID) return xdfm_sigmoid(v);
    return v;
}

__device__ __forceinline__ long bn_nrb(long rows) { return (rows + BN_ROWBLK - 1) / BN_ROWBLK; }

// ---- launch 1, forward: (mean, M2) of every (row block, column) -> ws[(2 rb) * cols + c], ws[(2 rb + 1) * cols + c]
__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const float* __restrict__ z, long ldz, long rows, int cols,
                                                             double* __restrict__ ws) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    const long rb = blockIdx.x;
    const long r0 = rb * BN_ROWBLK + rg;
    BnStat s{0.0, 0.0, 0.0};
    if (c < cols) {
        float v[BN_RPT];
        int n = 0;
#pragma unroll
        for (int t = 0; t < BN_RPT; ++t) {
            const long r = r0 + 4 * t;
            const bool in = r < rows;
            v[t] = in ? z[r * ldz + c] : 0.f;
            n += in ? 1 : 0;
        }
        if (n > 0) {
            // two passes over the thread's rows in registers: distances from a pivot (its first row, always present), their
            // mean, then the squared distances from that mean
            const double pivot = (double)v[0];
            double d[BN_RPT], sum = 0.0;
#pragma unroll
            for (int t = 0; t < BN_RPT; ++t) {
                d[t] = r0 + 4 * t < rows ? (double)v[t] - pivot : 0.0;
                sum += d[t];
            }
            const double off = sum / (double)n;
            double m2 = 0.0;
#pragma unroll
            for (int t = 0; t < BN_RPT; ++t) {
                const double e = d[t] - off;
                if (r0 + 4 * t < rows) m2 = fma(e, e, m2);
            }
            s.n = (double)n; s.mean = pivot + off; s.m2 = m2;
        }
    }
    __shared__ double sn[4][64], sm[4][64], sq[4][64];
    sn[rg][lane] = s.n; sm[rg][lane] = s.mean; sq[rg][lane] = s.m2;
    __syncthreads();
    if (rg == 0 && c < cols) {
        BnStat q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { q[k].n = sn[k][lane]; q[k].mean = sm[k][lane]; q[k].m2 = sq[k][lane]; }
        const BnStat r = bn_merge(bn_merge(q[0], q[1]), bn_merge(q[2], q[3]));
        ws[(2 * rb) * cols + c] = r.mean;
        ws[(2 * rb + 1) * cols + c] = r.m2;
    }
}

// the merged statistics of column c over all row blocks, the same bits in every block: thread (rg, lane) walks row blocks
// [rg * per, (rg + 1) * per) in index order, then (0 + 1) + (2 + 3).  Called by all BN_THREADS threads.
__device__ __forceinline__ BnStat bn_merge_all(const double* __restrict__ ws, long rows, int cols, int c, int lane, int rg) {
    __shared__ double sn[4][64], sm[4][64], sq[4][64];
    const long nrb = bn_nrb(rows);
    const long per = (nrb + 3) / 4;
    BnStat s{0.0, 0.0, 0.0};
    if (c < cols) {
        const long k1 = (rg + 1) * per < nrb ? (rg + 1) * per : nrb;
        for (long k = rg * per; k < k1; ++k) {
            BnStat b;
            const long left = rows - k * BN_ROWBLK;
            b.n = (double)(left < BN_ROWBLK ? left : BN_ROWBLK);
            b.mean = ws[(2 * k) * cols + c];
            b.m2 = ws[(2 * k + 1) * cols + c];
            s = bn_merge(s, b);
        }
    }
    sn[rg][lane] = s.n; sm[rg][lane] = s.mean; sq[rg][lane] = s.m2;
    __syncthreads();
    BnStat q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k].n = sn[k][lane]; q[k].mean = sm[k][lane]; q[k].m2 = sq[k][lane]; }
    return bn_merge(bn_merge(q[0], q[1]), bn_merge(q[2], q[3]));
}

// y of the rows of row block rb, this thread's column: y = act((z - mean) * sc + beta), sc = gamma * rstd, in double per
// element with one rounding to fp32 before the activation (a few fp64 operations per 8 bytes moved: the kernel stays
// bandwidth-bound)
__device__ __forceinline__ void bn_apply_rows(const float* __restrict__ z, long ldz, long rows, long rb, int rg, int c, double mean,
                                              double sc, double be, int act, float* __restrict__ y, long ldy) {
    const long r0 = rb * BN_ROWBLK + rg;
    float v[BN_RPT];
#pragma unroll
    for (int t = 0; t < BN_RPT; ++t) {
        const long r = r0 + 4 * t;
        v[t] = r < rows ? z[r * ldz + c] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < BN_RPT; ++t) {
        const long r = r0 + 4 * t;
        if (r < rows) y[r * ldy + c] = bn_act_fwd(act, (float)fma((double)v[t] - mean, sc, be));
    }
}

// ---- launch 2, training forward
__global__ __launch_bounds__(BN_THREADS) void bn_apply_train_kernel(
    const float* __restrict__ z, long ldz, long rows, int cols, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, float momentum, int act, float* __restrict__ y, long ldy, float* __restrict__ save_mean, float* __restrict__ save_rstd,
    float* __restrict__ running_mean, float* __restrict__ running_var, const double* __restrict__ ws) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    const BnStat s = bn_merge_all(ws, rows, cols, c, lane, rg);
    if (c >= cols) return;
    const double n = (double)rows;
    const double rstd = 1.0 / sqrt(s.m2 / n + (double)eps);
    if (blockIdx.x == 0 && rg == 0) {
        const double m = (double)momentum;
        save_mean[c] = (float)s.mean;
        save_rstd[c] = (float)rstd;
        running_mean[c] = (float)fma(m, s.mean, (1.0 - m) * (double)running_mean[c]);
        running_var[c] = (float)fma(m, s.m2 / (n - 1.0), (1.0 - m) * (double)running_var[c]);
    }
    const double sc = (double)gamma[c] * rstd, be = (double)beta[c];
    const long nrb = bn_nrb(rows);
    for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) bn_apply_rows(z, ldz, rows, rb, rg, c, s.mean, sc, be, act, y, ldy);
}

// ---- evaluation forward: one launch
__global__ __launch_bounds__(BN_THREADS) void bn_apply_eval_kernel(
    const float* __restrict__ z, long ldz, long rows, int cols, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, int act, float* __restrict__ y, long ldy, const float* __restrict__ running_mean, const float* __restrict__ running_var) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    if (c >= cols) return;
    const double mean = (double)running_mean[c];
    const double sc = (double)gamma[c] / sqrt((double)running_var[c] + (double)eps), be = (double)beta[c];
    const long nrb = bn_nrb(rows);
    for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) bn_apply_rows(z, ldz, rows, rb, rg, c, mean, sc, be, act, y, ldy);
}

// ---- launch 1, backward: per (row block, column) the sums of gm and of gm * xhat -> ws, the layout of the forward's pairs.
// gm is the fp32 product the activation's backward gives; xhat and both sums are carried in double: over few rows the three
// terms of dz cancel to rounding, and what is left should be the rounding of the saved statistics, not of this arithmetic.
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_sums_kernel(
    const float* __restrict__ g, long ldg, const float* __restrict__ y, long ldy, const float* __restrict__ z, long ldz, long rows,
    int cols, const float* __restrict__ save_mean, const float* __restrict__ save_rstd, int act, double* __restrict__ ws) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    const long rb = blockIdx.x;
    const long r0 = rb * BN_ROWBLK + rg;
    double a = 0.0, b = 0.0;
    if (c < cols) {
        const double mean = (double)save_mean[c], rstd = (double)save_rstd[c];
        float gv[BN_RPT], yv[BN_RPT], zv[BN_RPT];
#pragma unroll
        for (int t = 0; t < BN_RPT; ++t) {                     // all operands loaded unconditionally (clamped row)
            const long r = r0 + 4 * t < rows ? r0 + 4 * t : rows - 1;
            gv[t] = g[r * ldg + c];
            yv[t] = act == XDFM_ACT_LINEAR ? 0.f : y[r * ldy + c];
            zv[t] = z[r * ldz + c];
        }
#pragma unroll
        for (int t = 0; t < BN_RPT; ++t) {
            if (r0 + 4 * t >= rows) continue;
            const double gm = (double)xdfm_act_bwd(act, yv[t], gv[t]);
            a += gm;
            b = fma(gm, ((double)zv[t] - mean) * rstd, b);
        }
    }
    __shared__ double sa[4][64], sb[4][64];
    sa[rg][lane] = a; sb[rg][lane] = b;
    __syncthreads();
    if (rg == 0 && c < cols) {
        ws[(2 * rb) * cols + c] = (sa[0][lane] + sa[1][lane]) + (sa[2][lane] + sa[3][lane]);
        ws[(2 * rb + 1) * cols + c] = (sb[0][lane] + sb[1][lane]) + (sb[2][lane] + sb[3][lane]);
    }
}

// ---- launch 2, backward.  FROZEN: the statistics were constants of the forward (evaluation mode): no mean terms in dz.
template <bool FROZEN>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(
    const float* __restrict__ g, long ldg, const float* __restrict__ y, long ldy, const float* __restrict__ z, long ldz, long rows,
    int cols, const float* __restrict__ gamma, const float* __restrict__ save_mean, const float* __restrict__ save_rstd, int act,
    float* __restrict__ dz, long lddz, float* __restrict__ dgamma, float* __restrict__ dbeta, const double* __restrict__ ws) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    const long nrb = bn_nrb(rows);
    __shared__ double sa[4][64], sb[4][64];
    double a = 0.0, b = 0.0;
    const bool sums = !FROZEN || (blockIdx.x == 0 && (dgamma || dbeta));       // FROZEN: only dgamma / dbeta read them
    if (sums && c < cols) {
        const long per = (nrb + 3) / 4;
        const long k1 = (rg + 1) * per < nrb ? (rg + 1) * per : nrb;
        for (long k = rg * per; k < k1; ++k) {
            a += ws[(2 * k) * cols + c];
            b += ws[(2 * k + 1) * cols + c];
        }
    }
    sa[rg][lane] = a; sb[rg][lane] = b;
    __syncthreads();
    if (c >= cols) return;
    const double s1 = (sa[0][lane] + sa[1][lane]) + (sa[2][lane] + sa[3][lane]);
    const double s2 = (sb[0][lane] + sb[1][lane]) + (sb[2][lane] + sb[3][lane]);
    if (blockIdx.x == 0 && rg == 0) {
        if (dbeta) dbeta[c] = (float)s1;
        if (dgamma) dgamma[c] = (float)s2;
    }
    if (!dz) return;
    const double mean = (double)save_mean[c], rstd = (double)save_rstd[c];
    const double k0 = (double)gamma[c] * rstd;
    const double m1 = FROZEN ? 0.0 : s1 / (double)rows, m2 = FROZEN ? 0.0 : s2 / (double)rows;
    for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const long r0 = rb * BN_ROWBLK + rg;
        float gv[BN_RPT], yv[BN_RPT], zv[BN_RPT];
#pragma unroll
        for (int t = 0; t < BN_RPT; ++t) {
            const long r = r0 + 4 * t < rows ? r0 + 4 * t : rows - 1;
            gv[t] = g[r * ldg + c];
            yv[t] = act == XDFM_ACT_LINEAR ? 0.f : y[r * ldy + c];
            zv[t] = FROZEN ? 0.f : z[r * ldz + c];
        }
#pragma unroll
        for (int t = 0; t < BN_RPT; ++t) {
            const long r = r0 + 4 * t;
            if (r >= rows) continue;
            const double gm = (double)xdfm_act_bwd(act, yv[t], gv[t]);
            if constexpr (FROZEN) dz[r * lddz + c] = (float)(k0 * gm);
            else dz[r * lddz + c] = (float)(k0 * ((gm - m1) - (((double)zv[t] - mean) * rstd) * m2));
        }
    }
}

// ---- synchronised batch norm (row-parallel training): each direction split where the other ranks' numbers are needed.
// The statistics launch and the backward's sums launch are the ones above; a one-block-row finish leaves this rank's merged
// pair / sums where the all-gather picks them up, and the apply kernels read the gathered buffer of all ranks.

// finish of xdfm_bn_stats: the Chan merge of launch 1's pairs (bn_merge_all's order) -> pair[0][c] = mean, pair[1][c] = M2
__global__ __launch_bounds__(BN_THREADS) void bn_pair_finish_kernel(const double* __restrict__ ws, long rows, int cols,
                                                                   double* __restrict__ pair) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    const BnStat s = bn_merge_all(ws, rows, cols, c, lane, rg);
    if (c >= cols || rg != 0) return;
    pair[c] = s.mean;
    pair[(long)cols + c] = s.m2;
}

// the statistics of column c over the global batch: the ranks' triples (count, mean, M2) of all [world][1 + 2 cols], merged
// in rank order; bn_merge skips a rank whose count is 0 (a stand-in row).  The same bits in every thread, block and rank.
__device__ __forceinline__ BnStat bn_merge_ranks(const double* __restrict__ all, int world, int cols, int c) {
    const long pitch = 1 + 2 * (long)cols;
    BnStat s{0.0, 0.0, 0.0};
    for (int r = 0; r < world; ++r) {
        const double* __restrict__ p = all + r * pitch;
        BnStat b;
        b.n = p[0];
        b.mean = p[1 + c];
        b.m2 = p[1 + (long)cols + c];
        s = bn_merge(s, b);
    }
    return s;
}

// ---- training forward over the global statistics: bn_apply_train_kernel with n = the sum of the ranks' counts
__global__ __launch_bounds__(BN_THREADS) void bn_apply_sync_kernel(
    const float* __restrict__ z, long ldz, long rows, int cols, const double* __restrict__ all, int world,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum, int act, float* __restrict__ y, long ldy,
    float* __restrict__ save_mean, float* __restrict__ save_rstd, float* __restrict__ running_mean, float* __restrict__ running_var) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    if (c >= cols) return;
    const BnStat s = bn_merge_ranks(all, world, cols, c);
    const double n = s.n;
    const double rstd = 1.0 / sqrt(s.m2 / n + (double)eps);
    if (blockIdx.x == 0 && rg == 0) {
        const double m = (double)momentum;
        save_mean[c] = (float)s.mean;
        save_rstd[c] = (float)rstd;
        running_mean[c] = (float)fma(m, s.mean, (1.0 - m) * (double)running_mean[c]);
        running_var[c] = (float)fma(m, s.m2 / (n - 1.0), (1.0 - m) * (double)running_var[c]);
    }
    const double sc = (double)gamma[c] * rstd, be = (double)beta[c];
    const long nrb = bn_nrb(rows);
    for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) bn_apply_rows(z, ldz, rows, rb, rg, c, s.mean, sc, be, act, y, ldy);
}

// finish of xdfm_bn_bwd_sums: launch 1's partials added in bn_bwd_apply_kernel's order -> sums[0][c], sums[1][c]
__global__ __launch_bounds__(BN_THREADS) void bn_sums_finish_kernel(const double* __restrict__ ws, long rows, int cols,
                                                                   double* __restrict__ sums) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    const long nrb = bn_nrb(rows);
    __shared__ double sa[4][64], sb[4][64];
    double a = 0.0, b = 0.0;
    if (c < cols) {
        const long per = (nrb + 3) / 4;
        const long k1 = (rg + 1) * per < nrb ? (rg + 1) * per : nrb;
        for (long k = rg * per; k < k1; ++k) {
            a += ws[(2 * k) * cols + c];
            b += ws[(2 * k + 1) * cols + c];
        }
    }
    sa[rg][lane] = a; sb[rg][lane] = b;
    __syncthreads();
    if (c >= cols || rg != 0) return;
    sums[c] = (sa[0][lane] + sa[1][lane]) + (sa[2][lane] + sa[3][lane]);
    sums[(long)cols + c] = (sb[0][lane] + sb[1][lane]) + (sb[2][lane] + sb[3][lane]);
}

// ---- backward over the global sums: all [world][2 cols] holds every rank's (sum gm, sum gm * xhat); S1, S2 are added in
// rank order, dgamma / dbeta are this rank's own row (the dense all-reduce makes them global).  COUNTED = false: the rank
// holds a stand-in row that is not part of the global batch -- its dz is exact zeros, whatever the other ranks' sums are.
template <bool COUNTED>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_sync_kernel(
    const float* __restrict__ g, long ldg, const float* __restrict__ y, long ldy, const float* __restrict__ z, long ldz, long rows,
    int cols, const double* __restrict__ all, int world, int rank, double n_total, const float* __restrict__ gamma,
    const float* __restrict__ save_mean, const float* __restrict__ save_rstd, int act, float* __restrict__ dz, long lddz,
    float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * BN_COLBLK + lane;
    if (c >= cols) return;
    const long pitch = 2 * (long)cols;
    if (blockIdx.x == 0 && rg == 0) {
        if (dbeta) dbeta[c] = (float)all[rank * pitch + c];
        if (dgamma) dgamma[c] = (float)all[rank * pitch + cols + c];
    }
    if (!dz) return;
    const long nrb = bn_nrb(rows);
    if constexpr (!COUNTED) {
        for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
            const long r0 = rb * BN_ROWBLK + rg;
#pragma unroll
            for (int t = 0; t < BN_RPT; ++t) {
                const long r = r0 + 4 * t;
                if (r < rows) dz[r * lddz + c] = 0.f;
            }
        }
    } else {
        double s1 = 0.0, s2 = 0.0;
        for (int r = 0; r < world; ++r) {
            s1 += all[r * pitch + c];
            s2 += all[r * pitch + cols + c];
        }
        const double mean = (double)save_mean[c], rstd = (double)save_rstd[c];
        const double k0 = (double)gamma[c] * rstd;
        const double m1 = s1 / n_total, m2 = s2 / n_total;
        for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
            const long r0 = rb * BN_ROWBLK + rg;
            float gv[BN_RPT], yv[BN_RPT], zv[BN_RPT];
#pragma unroll
            for (int t = 0; t < BN_RPT; ++t) {
                const long r = r0 + 4 * t < rows ? r0 + 4 * t : rows - 1;
                gv[t] = g[r * ldg + c];
                yv[t] = act == XDFM_ACT_LINEAR ? 0.f : y[r * ldy + c];
                zv[t] = z[r * ldz + c];
            }
#pragma unroll
            for (int t = 0; t < BN_RPT; ++t) {
                const long r = r0 + 4 * t;
                if (r >= rows) continue;
                const double gm = (double)xdfm_act_bwd(act, yv[t], gv[t]);
                dz[r * lddz + c] = (float)(k0 * ((gm - m1) - (((double)zv[t] - mean) * rstd) * m2));
            }
        }
    }
}

extern "C" {

int xdfm_bn_row_block(void) { return BN_ROWBLK; }

size_t xdfm_bn_ws_elems(long rows, int cols) {
    if (rows < 1 || cols < 1) return 0;
    return (size_t)4 * (size_t)ceil_div(rows, BN_ROWBLK) * (size_t)cols;        // two doubles per row block and column
}

static int bn_shape_check(const char* what, long rows, long min_rows, int cols) {
    XDFM_REQUIRE(rows >= min_rows, "%s: rows = %ld (at least %ld)", what, rows, min_rows);
    XDFM_REQUIRE(rows <= ((long)1 << 36), "%s: rows = %ld (at most 2^36)", what, rows);
    XDFM_REQUIRE(cols >= 1 && cols <= BN_COLBLK * 65535, "%s: cols = %d (1 .. %d)", what, cols, BN_COLBLK * 65535);
    return XDFM_OK;
}

static inline unsigned bn_apply_blocks(long rows) {
    const long nrb = (rows + BN_ROWBLK - 1) / BN_ROWBLK;
    return (unsigned)(nrb < BN_MAX_APPLY ? nrb : BN_MAX_APPLY);
}

int xdfm_bn_fwd_train(const float* z, long ldz, long rows, int cols, const float* gamma, const float* beta, float eps, float momentum,
                      int act, float* y, long ldy, float* save_mean, float* save_rstd, float* running_mean, float* running_var,
                      float* ws, void* stream) {
    XDFM_REQUIRE(z && gamma && beta && y && save_mean && save_rstd && running_mean && running_var, "bn_fwd_train: null pointer");
    XDFM_REQUIRE(ws, "bn_fwd_train: workspace is NULL");
    XDFM_REQUIRE(((size_t)ws & 7) == 0, "bn_fwd_train: workspace not 8-byte aligned");
    if (int rc = bn_shape_check("bn_fwd_train", rows, 2, cols)) return rc;
    XDFM_REQUIRE(ldz >= cols, "bn_fwd_train: ldz = %ld below cols = %d", ldz, cols);
    XDFM_REQUIRE(ldy >= cols, "bn_fwd_train: ldy = %ld below cols = %d", ldy, cols);
    XDFM_REQUIRE(xdfm_act_known(act), "bn_fwd_train: act = %d (0 linear, 1 relu, 2 sigmoid)", act);
    XDFM_REQUIRE(eps > 0.f, "bn_fwd_train: eps = %g (must be positive)", (double)eps);
    XDFM_REQUIRE(momentum >= 0.f && momentum <= 1.f, "bn_fwd_train: momentum = %g outside [0, 1]", (double)momentum);
    hipStream_t st = (hipStream_t)stream;
    const unsigned nrb = (unsigned)ceil_div(rows, BN_ROWBLK), cb = (unsigned)ceil_div(cols, BN_COLBLK);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(nrb, cb), dim3(BN_THREADS), 0, st, z, ldz, rows, cols, (double*)ws);
    if (int rc = xdfm_check_launch("bn_fwd_train statistics")) return rc;
    hipLaunchKernelGGL(bn_apply_train_kernel, dim3(bn_apply_blocks(rows), cb), dim3(BN_THREADS), 0, st, z, ldz, rows, cols, gamma, beta,
                       eps, momentum, act, y, ldy, save_mean, save_rstd, running_mean, running_var, (const double*)ws);
    return xdfm_check_launch("bn_fwd_train");
}

int xdfm_bn_fwd_eval(const float* z, long ldz, long rows, int cols, const float* gamma, const float* beta, float eps, int act, float* y,
                     long ldy, const float* running_mean, const float* running_var, void* stream) {
    XDFM_REQUIRE(z && gamma && beta && y && running_mean && running_var, "bn_fwd_eval: null pointer");
    if (int rc = bn_shape_check("bn_fwd_eval", rows, 1, cols)) return rc;
    XDFM_REQUIRE(ldz >= cols, "bn_fwd_eval: ldz = %ld below cols = %d", ldz, cols);
    XDFM_REQUIRE(ldy >= cols, "bn_fwd_eval: ldy = %ld below cols = %d", ldy, cols);
    XDFM_REQUIRE(xdfm_act_known(act), "bn_fwd_eval: act = %d (0 linear, 1 relu, 2 sigmoid)", act);
    XDFM_REQUIRE(eps > 0.f, "bn_fwd_eval: eps = %g (must be positive)", (double)eps);
    hipLaunchKernelGGL(bn_apply_eval_kernel, dim3(bn_apply_blocks(rows), (unsigned)ceil_div(cols, BN_COLBLK)), dim3(BN_THREADS), 0,
                       (hipStream_t)stream, z, ldz, rows, cols, gamma, beta, eps, act, y, ldy, running_mean, running_var);
    return xdfm_check_launch("bn_fwd_eval");
}

static int bn_bwd_any(const char* what, bool frozen, const float* g, long ldg, const float* y, long ldy, const float* z, long ldz,
                      long rows, int cols, const float* gamma, const float* save_mean, const float* save_rstd, int act, float* dz,
                      long lddz, float* dgamma, float* dbeta, float* ws, void* stream) {
    XDFM_REQUIRE(g && y && z && gamma && save_mean && save_rstd, "%s: null pointer", what);
    XDFM_REQUIRE(ws, "%s: workspace is NULL", what);
    XDFM_REQUIRE(((size_t)ws & 7) == 0, "%s: workspace not 8-byte aligned", what);
    if (int rc = bn_shape_check(what, rows, frozen ? 1 : 2, cols)) return rc;
    XDFM_REQUIRE(ldg >= cols, "%s: ldg = %ld below cols = %d", what, ldg, cols);
    XDFM_REQUIRE(ldy >= cols, "%s: ldy = %ld below cols = %d", what, ldy, cols);
    XDFM_REQUIRE(ldz >= cols, "%s: ldz = %ld below cols = %d", what, ldz, cols);
    XDFM_REQUIRE(!dz || lddz >= cols, "%s: lddz = %ld below cols = %d", what, lddz, cols);
    XDFM_REQUIRE(xdfm_act_known(act), "%s: act = %d (0 linear, 1 relu, 2 sigmoid)", what, act);
    if (!dz && !dgamma && !dbeta) return XDFM_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nrb = (unsigned)ceil_div(rows, BN_ROWBLK), cb = (unsigned)ceil_div(cols, BN_COLBLK);
    if (!frozen || dgamma || dbeta) {
        hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(nrb, cb), dim3(BN_THREADS), 0, st, g, ldg, y, ldy, z, ldz, rows, cols, save_mean,
                           save_rstd, act, (double*)ws);
        if (int rc = xdfm_check_launch(what)) return rc;
    }
    const dim3 grid(dz ? bn_apply_blocks(rows) : 1u, cb);
    if (frozen)
        hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid, dim3(BN_THREADS), 0, st, g, ldg, y, ldy, z, ldz, rows, cols, gamma, save_mean,
                           save_rstd, act, dz, lddz, dgamma, dbeta, (const double*)ws);
    else
        hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, dim3(BN_THREADS), 0, st, g, ldg, y, ldy, z, ldz, rows, cols, gamma, save_mean,
                           save_rstd, act, dz, lddz, dgamma, dbeta, (const double*)ws);
    return xdfm_check_launch(what);
}

int xdfm_bn_bwd(const float* g, long ldg, const float* y, long ldy, const float* z, long ldz, long rows, int cols, const float* gamma,
                const float* save_mean, const float* save_rstd, int act, float* dz, long lddz, float* dgamma, float* dbeta, float* ws,
                void* stream) {
    return bn_bwd_any("bn_bwd", false, g, ldg, y, ldy, z, ldz, rows, cols, gamma, save_mean, save_rstd, act, dz, lddz, dgamma, dbeta, ws,
                      stream);
}

int xdfm_bn_bwd_eval(const float* g, long ldg, const float* y, long ldy, const float* z, long ldz, long rows, int cols,
                     const float* gamma, const float* mean, const float* rstd, int act, float* dz, long lddz, float* dgamma, float* dbeta,
                     float* ws, void* stream) {
    return bn_bwd_any("bn_bwd_eval", true, g, ldg, y, ldy, z, ldz, rows, cols, gamma, mean, rstd, act, dz, lddz, dgamma, dbeta, ws, stream);
}

int xdfm_bn_stats(const float* z, long ldz, long rows, int cols, double* pair, float* ws, void* stream) {
    XDFM_REQUIRE(z && pair, "bn_stats: null pointer");
    XDFM_REQUIRE(ws, "bn_stats: workspace is NULL");
    XDFM_REQUIRE(((size_t)ws & 7) == 0, "bn_stats: workspace not 8-byte aligned");
    XDFM_REQUIRE(((size_t)pair & 7) == 0, "bn_stats: pair not 8-byte aligned");
    if (int rc = bn_shape_check("bn_stats", rows, 1, cols)) return rc;
    XDFM_REQUIRE(ldz >= cols, "bn_stats: ldz = %ld below cols = %d", ldz, cols);
    hipStream_t st = (hipStream_t)stream;
    const unsigned nrb = (unsigned)ceil_div(rows, BN_ROWBLK), cb = (unsigned)ceil_div(cols, BN_COLBLK);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(nrb, cb), dim3(BN_THREADS), 0, st, z, ldz, rows, cols, (double*)ws);
    if (int rc = xdfm_check_launch("bn_stats statistics")) return rc;
    hipLaunchKernelGGL(bn_pair_finish_kernel, dim3(1, cb), dim3(BN_THREADS), 0, st, (const double*)ws, rows, cols, pair);
    return xdfm_check_launch("bn_stats");
}

int xdfm_bn_fwd_apply_sync(const float* z, long ldz, long rows, int cols, const double* all, int world, const float* gamma,
                           const float* beta, float eps, float momentum, int act, float* y, long ldy, float* save_mean,
                           float* save_rstd, float* running_mean, float* running_var, void* stream) {
    XDFM_REQUIRE(z && all && gamma && beta && y && save_mean && save_rstd && running_mean && running_var,
                 "bn_fwd_apply_sync: null pointer");
    XDFM_REQUIRE(((size_t)all & 7) == 0, "bn_fwd_apply_sync: all not 8-byte aligned");
    if (int rc = bn_shape_check("bn_fwd_apply_sync", rows, 1, cols)) return rc;
    XDFM_REQUIRE(world >= 1, "bn_fwd_apply_sync: world = %d (at least 1)", world);
    XDFM_REQUIRE(ldz >= cols, "bn_fwd_apply_sync: ldz = %ld below cols = %d", ldz, cols);
    XDFM_REQUIRE(ldy >= cols, "bn_fwd_apply_sync: ldy = %ld below cols = %d", ldy, cols);
    XDFM_REQUIRE(xdfm_act_known(act), "bn_fwd_apply_sync: act = %d (0 linear, 1 relu, 2 sigmoid)", act);
    XDFM_REQUIRE(eps > 0.f, "bn_fwd_apply_sync: eps = %g (must be positive)", (double)eps);
    XDFM_REQUIRE(momentum >= 0.f && momentum <= 1.f, "bn_fwd_apply_sync: momentum = %g outside [0, 1]", (double)momentum);
    hipLaunchKernelGGL(bn_apply_sync_kernel, dim3(bn_apply_blocks(rows), (unsigned)ceil_div(cols, BN_COLBLK)), dim3(BN_THREADS), 0,
                       (hipStream_t)stream, z, ldz, rows, cols, all, world, gamma, beta, eps, momentum, act, y, ldy, save_mean, save_rstd,
                       running_mean, running_var);
    return xdfm_check_launch("bn_fwd_apply_sync");
}

int xdfm_bn_bwd_sums(const float* g, long ldg, const float* y, long ldy, const float* z, long ldz, long rows, int cols,
                     const float* save_mean, const float* save_rstd, int act, double* sums, float* ws, void* stream) {
    XDFM_REQUIRE(g && y && z && save_mean && save_rstd && sums, "bn_bwd_sums: null pointer");
    XDFM_REQUIRE(ws, "bn_bwd_sums: workspace is NULL");
    XDFM_REQUIRE(((size_t)ws & 7) == 0, "bn_bwd_sums: workspace not 8-byte aligned");
    XDFM_REQUIRE(((size_t)sums & 7) == 0, "bn_bwd_sums: sums not 8-byte aligned");
    if (int rc = bn_shape_check("bn_bwd_sums", rows, 1, cols)) return rc;
    XDFM_REQUIRE(ldg >= cols, "bn_bwd_sums: ldg = %ld below cols = %d", ldg, cols);
    XDFM_REQUIRE(ldy >= cols, "bn_bwd_sums: ldy = %ld below cols = %d", ldy, cols);
    XDFM_REQUIRE(ldz >= cols, "bn_bwd_sums: ldz = %ld below cols = %d", ldz, cols);
    XDFM_REQUIRE(xdfm_act_known(act), "bn_bwd_sums: act = %d (0 linear, 1 relu, 2 sigmoid)", act);
    hipStream_t st = (hipStream_t)stream;
    const unsigned nrb = (unsigned)ceil_div(rows, BN_ROWBLK), cb = (unsigned)ceil_div(cols, BN_COLBLK);
    hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(nrb, cb), dim3(BN_THREADS), 0, st, g, ldg, y, ldy, z, ldz, rows, cols, save_mean,
                       save_rstd, act, (double*)ws);
    if (int rc = xdfm_check_launch("bn_bwd_sums partials")) return rc;
    hipLaunchKernelGGL(bn_sums_finish_kernel, dim3(1, cb), dim3(BN_THREADS), 0, st, (const double*)ws, rows, cols, sums);
    return xdfm_check_launch("bn_bwd_sums");
}

int xdfm_bn_bwd_apply_sync(const float* g, long ldg, const float* y, long ldy, const float* z, long ldz, long rows, long rows_counted,
                           int cols, const double* all, int world, int rank, long n_total, const float* gamma, const float* save_mean,
                           const float* save_rstd, int act, float* dz, long lddz, float* dgamma, float* dbeta, void* stream) {
    XDFM_REQUIRE(g && y && z && all && gamma && save_mean && save_rstd, "bn_bwd_apply_sync: null pointer");
    XDFM_REQUIRE(((size_t)all & 7) == 0, "bn_bwd_apply_sync: all not 8-byte aligned");
    if (int rc = bn_shape_check("bn_bwd_apply_sync", rows, 1, cols)) return rc;
    XDFM_REQUIRE(rows_counted == rows || rows_counted == 0, "bn_bwd_apply_sync: rows_counted = %ld (rows = %ld, or 0 for a stand-in)",
                 rows_counted, rows);
    XDFM_REQUIRE(world >= 1, "bn_bwd_apply_sync: world = %d (at least 1)", world);
    XDFM_REQUIRE(rank >= 0 && rank < world, "bn_bwd_apply_sync: rank = %d outside [0, world = %d)", rank, world);
    XDFM_REQUIRE(n_total >= 2, "bn_bwd_apply_sync: n_total = %ld (at least 2)", n_total);
    XDFM_REQUIRE(ldg >= cols, "bn_bwd_apply_sync: ldg = %ld below cols = %d", ldg, cols);
    XDFM_REQUIRE(ldy >= cols, "bn_bwd_apply_sync: ldy = %ld below cols = %d", ldy, cols);
    XDFM_REQUIRE(ldz >= cols, "bn_bwd_apply_sync: ldz = %ld below cols = %d", ldz, cols);
    XDFM_REQUIRE(!dz || lddz >= cols, "bn_bwd_apply_sync: lddz = %ld below cols = %d", lddz, cols);
    XDFM_REQUIRE(xdfm_act_known(act), "bn_bwd_apply_sync: act = %d (0 linear, 1 relu, 2 sigmoid)", act);
    if (!dz && !dgamma && !dbeta) return XDFM_OK;
    const dim3 grid(dz ? bn_apply_blocks(rows) : 1u, (unsigned)ceil_div(cols, BN_COLBLK));
    if (rows_counted)
        hipLaunchKernelGGL(bn_bwd_apply_sync_kernel<true>, grid, dim3(BN_THREADS), 0, (hipStream_t)stream, g, ldg, y, ldy, z, ldz, rows,
                           cols, all, world, rank, (double)n_total, gamma, save_mean, save_rstd, act, dz, lddz, dgamma, dbeta);
    else
        hipLaunchKernelGGL(bn_bwd_apply_sync_kernel<false>, grid, dim3(BN_THREADS), 0, (hipStream_t)stream, g, ldg, y, ldy, z, ldz, rows,
                           cols, all, world, rank, (double)n_total, gamma, save_mean, save_rstd, act, dz, lddz, dgamma, dbeta);
    return xdfm_check_launch("bn_bwd_apply_sync");
}

}  // extern "C"
