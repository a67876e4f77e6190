// K10: AutoDis, the learned soft discretisation of the dense features of xdeepfm_pro (deepctr/xdeepfm_pro/autodis.py:20-127).
// Per (row b, field f), all in fp32:
//   h_k = W1[f][k] x[b,f] + b1[f][k];  a_k = leaky_relu(h_k, 0.2);  s_j = sum_k W2[f][j][k] a_k + b2[f][j];
//   w = softmax(s / T[f]);  out[b][f*D + d] = sum_k w_k meta[f][k][d]
// The reference runs this as a Python loop over the fields (7 launches per field + a cat; about twice that backward) on
// [B, K] tensors: ~30 MFLOP behind ~90 launches.  Here ONE launch covers all fields and rows each way, plus one
// fixed-order finish launch for the parameter gradients.
//
// Mapping: a workgroup owns one field and a block of rows, a thread owns a row.  The field's parameters (at most 12.7 KB
// at K = 32, D = 64) are staged in LDS once, zero-padded to the instance's KC in {8, 16, 32} so that the k loops are
// compile-time and a[], s[] live in registers; every LDS read of a parameter is a wave-uniform broadcast.  The run-time
// tail (K < KC) only shows in the softmax mask.
//
// Backward: only x is saved, the forward is recomputed per (row, field).  The parameter gradients are sums over the rows
// of per-row outer products (dmeta = w^T g, dW2 = ds^T a, ...).  No float atomics: the threads leave their row vectors in
// LDS, then every thread owns a few OUTPUT elements and walks the block's rows in order; the workgroup writes one partial
// per (row block, field) and autodis_finish_kernel sums the row blocks in a fixed order -- two runs give the same bits.
#include "xdfm_internal.h"

#define AD_MAXK 32
#define AD_MAXD 64
#define AD_FWD_ROWS 256
enum { AD_META = 1, AD_W1 = 2, AD_B1 = 4, AD_W2 = 8, AD_B2 = 16, AD_T = 32, AD_DX = 64, AD_PARAMS = 63 };

static inline int ad_bwd_rows(int K) { return K <= 16 ? 256 : 128; }            // rows per workgroup of the backward
__host__ __device__ static inline long ad_per_field(int K, int D) { return (long)K * D + (long)K * K + 3L * K + 1; }

// the field's parameters -> LDS, zero beyond K / D (Dp = D rounded up to 4: the meta rows are read as float4)
template <int KC, int NT>
__device__ __forceinline__ void ad_stage(const float* __restrict__ meta_f, const float* const* __restrict__ proj_f, int K, int D, int Dp,
                                         float* sW1, float* sb1, float* sW2, float* sb2, float* sM) {
    const float* W1 = proj_f[0];
    const float* b1 = proj_f[1];
    const float* W2 = proj_f[2];
    const float* b2 = proj_f[3];
    const int tid = threadIdx.x;
    for (int i = tid; i < KC; i += NT) {
        sW1[i] = i < K ? W1[i] : 0.f;
        sb1[i] = i < K ? b1[i] : 0.f;
        sb2[i] = i < K ? b2[i] : 0.f;
    }
    for (int i = tid; i < KC * KC; i += NT) {
        const int j = i / KC, k = i % KC;
        sW2[i] = (j < K && k < K) ? W2[j * K + k] : 0.f;
    }
    for (int i = tid; i < KC * Dp; i += NT) {
        const int k = i / Dp, d = i - k * Dp;
        sM[i] = (k < K && d < D) ? meta_f[k * D + d] : 0.f;
    }
}

// a, the shifted logits s_k / T - max_j s_j / T (returned in s) and the softmax weights of one row; w[k] = s[k] = 0 for k >= K
template <int KC>
__device__ __forceinline__ void ad_row_fwd(float xv, float T, int K, const float* sW1, const float* sb1, const float* sW2, const float* sb2,
                                           float (&a)[KC], float (&s)[KC], float (&w)[KC]) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const float h = fmaf(sW1[k], xv, sb1[k]);
        a[k] = h > 0.f ? h : 0.2f * h;
    }
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};         // four short chains: fewer roundings on the way than one of KC
#pragma unroll
        for (int k = 0; k < KC; ++k) acc[k & 3] = fmaf(sW2[j * KC + k], a[k], acc[k & 3]);
        s[j] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + sb2[j];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        w[k] = s[k] / T;
        if (k < K) mx = fmaxf(mx, w[k]);
    }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        s[k] = k < K ? w[k] - mx : 0.f;
        w[k] = k < K ? expf(s[k]) : 0.f;
        sum += w[k];
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) w[k] = w[k] / sum;
}

template <int KC>
__global__ __launch_bounds__(AD_FWD_ROWS) void autodis_fwd_kernel(const float* __restrict__ x, long ldx, long B, int F, int K, int D,
                                                                  const float* __restrict__ meta, const float* const* __restrict__ proj,
                                                                  const float* __restrict__ temp, float* __restrict__ out, int vec) {
    __shared__ float sW1[KC], sb1[KC], sb2[KC], sW2[KC * KC];
    __shared__ __attribute__((aligned(16))) float sM[KC * AD_MAXD];
    const int f = (int)(blockIdx.x % (unsigned)F);
    const long blk = blockIdx.x / (unsigned)F;
    const int Dp = (D + 3) & ~3;
    ad_stage<KC, AD_FWD_ROWS>(meta + (long)f * K * D, proj + 4L * f, K, D, Dp, sW1, sb1, sW2, sb2, sM);
    __syncthreads();
    const long b = blk * AD_FWD_ROWS + threadIdx.x;
    if (b >= B) return;
    float a[KC], s[KC], w[KC];
    ad_row_fwd<KC>(x[b * ldx + f], temp[f], K, sW1, sb1, sW2, sb2, a, s, w);
    float* o = out + b * ((long)F * D) + (long)f * D;
    for (int d0 = 0; d0 < Dp; d0 += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KC; ++k) acc += w[k] * *reinterpret_cast<const f32x4*>(&sM[k * Dp + d0]);
        if (vec) {
            *reinterpret_cast<f32x4*>(o + d0) = acc;
        } else {
            for (int i = 0; i < 4; ++i)
                if (d0 + i < D) o[d0 + i] = acc[i];
        }
    }
}

// part: [row block][field][K*D dmeta | K*K dW2 | K db2 | K dW1 | K db1 | 1 dT]
template <int KC, int ROWS>
__global__ __launch_bounds__(ROWS) void autodis_bwd_kernel(const float* __restrict__ x, long ldx, long B, int F, int K, int D,
                                                           const float* __restrict__ meta, const float* const* __restrict__ proj,
                                                           const float* __restrict__ temp, const float* __restrict__ g, long ldg, int gvec,
                                                           int flags, float* __restrict__ part, float* __restrict__ dx) {
    constexpr int UP = KC + 1;            // pitch of the row vectors: lane r writes bank (r * UP + k) % 32, conflict-free
    __shared__ float sW1[KC], sb1[KC], sb2[KC], sW2[KC * KC];
    __shared__ __attribute__((aligned(16))) float sM[KC * AD_MAXD];
    __shared__ float sW2T[KC * KC];      // [k][j]: da = W2^T ds reads rows too
    __shared__ float U1[ROWS * UP], U2[ROWS * UP];
    const int f = (int)(blockIdx.x % (unsigned)F);
    const long blk = blockIdx.x / (unsigned)F;
    const int Dp = (D + 3) & ~3;
    const int tid = threadIdx.x;
    ad_stage<KC, ROWS>(meta + (long)f * K * D, proj + 4L * f, K, D, Dp, sW1, sb1, sW2, sb2, sM);
    __syncthreads();
    for (int i = tid; i < KC * KC; i += ROWS) sW2T[i] = sW2[(i % KC) * KC + i / KC];
    __syncthreads();
    const long b0 = blk * ROWS;
    const int nrows = (int)(B - b0 < ROWS ? B - b0 : ROWS);
    const bool valid = tid < nrows;
    const long b = b0 + tid;
    const float T = temp[f];
    const float xv = valid ? x[b * ldx + f] : 0.f;
    const float* grow = g + (valid ? b : b0) * ldg + (long)f * D;
    // v = dL/dw = meta g, before the recompute: KC float4 reads of meta are in flight per step, next to v alone
    float v[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) v[k] = 0.f;
    for (int d0 = 0; d0 < Dp; d0 += 4) {
        f32x4 gd = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
            if (gvec) {
                gd = *reinterpret_cast<const f32x4*>(grow + d0);
            } else {
                for (int i = 0; i < 4; ++i)
                    if (d0 + i < D) gd[i] = grow[d0 + i];
            }
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const f32x4 m4 = *reinterpret_cast<const f32x4*>(&sM[k * Dp + d0]);
            v[k] = fmaf(gd[0], m4[0], fmaf(gd[1], m4[1], fmaf(gd[2], m4[2], fmaf(gd[3], m4[3], v[k]))));
        }
    }
    float a[KC], s[KC], w[KC];
    ad_row_fwd<KC>(xv, T, K, sW1, sb1, sW2, sb2, a, s, w);
    float* pb = part + (blk * F + f) * ad_per_field(K, D);
    if (flags & AD_META) {
#pragma unroll
        for (int k = 0; k < KC; ++k) U1[tid * UP + k] = w[k];
        __syncthreads();
        const float* gb = g + b0 * ldg + (long)f * D;
        for (int o = tid; o < K * D; o += ROWS) {
            const int k = o / D, d = o - k * D;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            int r = 0;
            for (; r + 4 <= nrows; r += 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(U1[(r + i) * UP + k], gb[(r + i) * ldg + d], acc[i]);
            }
            for (; r < nrows; ++r) acc[0] = fmaf(U1[r * UP + k], gb[r * ldg + d], acc[0]);
            pb[o] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        }
        __syncthreads();
    }
    // softmax and temperature: z = s / T, dz = w (v - <w, v>), ds = dz / T, dT = -<dz, s> / T^2 = -<dz, z - max z> / T: the
    // dz sum to zero, so any shift of z is allowed, and with this one a large |z_k - max z| meets a vanishing w_k
    // instead of cancelling against the other terms
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k) dot = fmaf(w[k], v[k], dot);
    float dTr = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const float dz = w[k] * (v[k] - dot);
        dTr = fmaf(dz, s[k], dTr);
        v[k] = dz / T;                                   // ds
    }
    dTr = -dTr / T;
    if (flags & (AD_W2 | AD_B2)) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            U1[tid * UP + k] = v[k];
            U2[tid * UP + k] = a[k];
        }
        __syncthreads();
        float* pW2 = pb + (long)K * D;
        for (int o = tid; o < K * K + K; o += ROWS) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            int r = 0;
            if (o < K * K) {                             // dW2[j][k] = sum_r ds[r][j] a[r][k]
                const int j = o / K, k = o - j * K;
                for (; r + 4 <= nrows; r += 4) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = fmaf(U1[(r + i) * UP + j], U2[(r + i) * UP + k], acc[i]);
                }
                for (; r < nrows; ++r) acc[0] = fmaf(U1[r * UP + j], U2[r * UP + k], acc[0]);
            } else {                                     // db2[j] = sum_r ds[r][j]
                const int j = o - K * K;
                for (; r + 4 <= nrows; r += 4) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] += U1[(r + i) * UP + j];
                }
                for (; r < nrows; ++r) acc[0] += U1[r * UP + j];
            }
            pW2[o] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        }
        __syncthreads();
    }
    if (flags & (AD_W1 | AD_B1 | AD_T | AD_DX)) {
        // da = W2^T ds, dh = leaky_relu'(h) da (h > 0 <=> a > 0), dx = <dh, W1>
        float dxv = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            float dac[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < KC; ++j) dac[j & 3] = fmaf(sW2T[k * KC + j], v[j], dac[j & 3]);
            const float da = (dac[0] + dac[1]) + (dac[2] + dac[3]);
            const float dh = a[k] > 0.f ? da : 0.2f * da;
            dxv = fmaf(dh, sW1[k], dxv);
            U1[tid * UP + k] = dh;
        }
        if ((flags & AD_DX) && valid) dx[b * F + f] = dxv;
        if (flags & (AD_W1 | AD_B1 | AD_T)) {
            U2[tid * UP + 0] = xv;
            U2[tid * UP + 1] = dTr;
            __syncthreads();
            float* pW1 = pb + (long)K * D + (long)K * K + K;
            for (int o = tid; o < 2 * K + 1; o += ROWS) {
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                int r = 0;
                if (o < K) {                             // dW1[k] = sum_r dh[r][k] x[r]
                    for (; r + 4 <= nrows; r += 4) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] = fmaf(U1[(r + i) * UP + o], U2[(r + i) * UP], acc[i]);
                    }
                    for (; r < nrows; ++r) acc[0] = fmaf(U1[r * UP + o], U2[r * UP], acc[0]);
                } else if (o < 2 * K) {                  // db1[k] = sum_r dh[r][k]
                    const int k = o - K;
                    for (; r + 4 <= nrows; r += 4) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] += U1[(r + i) * UP + k];
                    }
                    for (; r < nrows; ++r) acc[0] += U1[r * UP + k];
                } else {                                 // dT = sum_r dT[r]
                    for (; r + 4 <= nrows; r += 4) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] += U2[(r + i) * UP + 1];
                    }
                    for (; r < nrows; ++r) acc[0] += U2[r * UP + 1];
                }
                pW1[o] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            }
        }
    }
}

// grads: [F][K][D] dmeta | [F][K] dW1 | [F][K] db1 | [F][K][K] dW2 | [F][K] db2 | [F] dT  <-  sum over the row blocks, in order
__global__ __launch_bounds__(256) void autodis_finish_kernel(const float* __restrict__ part, long nblk, int F, int K, int D, int flags,
                                                             float* __restrict__ grads) {
    const long P = (long)K * D + (long)K * K + 3L * K + 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= F * P) return;
    const long f = i / P;
    const long o = i - f * P;
    const long KD = (long)K * D, KK = (long)K * K, FK = (long)F * K;
    long dst;
    int bit;
    if (o < KD) { dst = f * KD + o; bit = AD_META; }
    else if (o < KD + KK) { dst = F * KD + 2 * FK + f * KK + (o - KD); bit = AD_W2; }
    else if (o < KD + KK + K) { dst = F * KD + 2 * FK + F * KK + f * K + (o - KD - KK); bit = AD_B2; }
    else if (o < KD + KK + 2 * K) { dst = F * KD + f * K + (o - KD - KK - K); bit = AD_W1; }
    else if (o < KD + KK + 3 * K) { dst = F * KD + FK + f * K + (o - KD - KK - 2 * K); bit = AD_B1; }
    else { dst = F * KD + 3 * FK + F * KK + f; bit = AD_T; }
    if (!(flags & bit)) return;
    const float* p = part + i;
    const long step = F * P;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    long r = 0;
    for (; r + 4 <= nblk; r += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += p[(r + k) * step];
    }
    for (; r < nblk; ++r) acc[0] += p[r * step];
    grads[dst] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

static int ad_check_shape(const char* what, long B, int F, int K, int D) {
    XDFM_REQUIRE(K >= 1 && K <= AD_MAXK, "%s: K = %d buckets, supported 1..%d", what, K, AD_MAXK);
    XDFM_REQUIRE(D >= 1 && D <= AD_MAXD, "%s: D = %d, supported 1..%d", what, D, AD_MAXD);
    XDFM_REQUIRE(F >= 1, "%s: F = %d fields", what, F);
    XDFM_REQUIRE(B >= 1, "%s: B = %ld rows", what, B);
    XDFM_REQUIRE((B + 127) / 128 * (long)F <= 0x7fffffffL, "%s: B = %ld rows x F = %d fields exceed the grid", what, B, F);
    return XDFM_OK;
}

extern "C" {

int xdfm_autodis_supported(int K, int D) { return K >= 1 && K <= AD_MAXK && D >= 1 && D <= AD_MAXD ? 1 : 0; }

size_t xdfm_autodis_ws_elems(long B, int F, int K, int D) {
    if (!xdfm_autodis_supported(K, D) || F < 1 || B < 1) return 0;
    const long rows = ad_bwd_rows(K);
    return (size_t)((B + rows - 1) / rows) * (size_t)F * (size_t)ad_per_field(K, D);
}

int xdfm_autodis_fwd(const float* x, long ldx, long B, int F, int K, int D, const float* meta, const float* const* proj,
                     const float* temp, float* out, void* stream) {
    XDFM_REQUIRE(x && meta && proj && temp && out, "autodis_fwd: null pointer");
    if (int rc = ad_check_shape("autodis_fwd", B, F, K, D)) return rc;
    XDFM_REQUIRE(ldx >= F, "autodis_fwd: ldx = %ld < F = %d", ldx, F);
    hipStream_t st = (hipStream_t)stream;
    const int vec = (D % 4 == 0) && ((size_t)out % 16 == 0);
    const dim3 grid((unsigned)(((B + AD_FWD_ROWS - 1) / AD_FWD_ROWS) * F));
    if (K <= 8) autodis_fwd_kernel<8><<<grid, AD_FWD_ROWS, 0, st>>>(x, ldx, B, F, K, D, meta, proj, temp, out, vec);
    else if (K <= 16) autodis_fwd_kernel<16><<<grid, AD_FWD_ROWS, 0, st>>>(x, ldx, B, F, K, D, meta, proj, temp, out, vec);
    else autodis_fwd_kernel<32><<<grid, AD_FWD_ROWS, 0, st>>>(x, ldx, B, F, K, D, meta, proj, temp, out, vec);
    return xdfm_check_launch("autodis_fwd");
}

int xdfm_autodis_bwd(const float* x, long ldx, long B, int F, int K, int D, const float* meta, const float* const* proj,
                     const float* temp, const float* g, long ldg, int flags, float* ws, float* grads, float* dx, void* stream) {
    XDFM_REQUIRE(x && meta && proj && temp && g, "autodis_bwd: null pointer");
    if (int rc = ad_check_shape("autodis_bwd", B, F, K, D)) return rc;
    XDFM_REQUIRE(ldx >= F, "autodis_bwd: ldx = %ld < F = %d", ldx, F);
    XDFM_REQUIRE(ldg >= (long)F * D, "autodis_bwd: ldg = %ld < F * D = %ld", ldg, (long)F * D);
    XDFM_REQUIRE(flags > 0 && flags <= (AD_PARAMS | AD_DX), "autodis_bwd: flags = %d", flags);
    XDFM_REQUIRE(!(flags & AD_PARAMS) || (ws && grads), "autodis_bwd: null pointer (ws / grads with a parameter gradient asked for)");
    XDFM_REQUIRE(!(flags & AD_DX) || dx, "autodis_bwd: null pointer (dx)");
    hipStream_t st = (hipStream_t)stream;
    const int gvec = (D % 4 == 0) && (ldg % 4 == 0) && ((size_t)g % 16 == 0);
    const int rows = ad_bwd_rows(K);
    const long nblk = (B + rows - 1) / rows;
    const dim3 grid((unsigned)(nblk * F));
    if (K <= 8) autodis_bwd_kernel<8, 256><<<grid, 256, 0, st>>>(x, ldx, B, F, K, D, meta, proj, temp, g, ldg, gvec, flags, ws, dx);
    else if (K <= 16) autodis_bwd_kernel<16, 256><<<grid, 256, 0, st>>>(x, ldx, B, F, K, D, meta, proj, temp, g, ldg, gvec, flags, ws, dx);
    else autodis_bwd_kernel<32, 128><<<grid, 128, 0, st>>>(x, ldx, B, F, K, D, meta, proj, temp, g, ldg, gvec, flags, ws, dx);
    if (int rc = xdfm_check_launch("autodis_bwd")) return rc;
    if (flags & AD_PARAMS) {
        const long total = (long)F * ad_per_field(K, D);
        autodis_finish_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(ws, nblk, F, K, D, flags, grads);
        return xdfm_check_launch("autodis_finish");
    }
    return XDFM_OK;
}

}  // extern "C"
