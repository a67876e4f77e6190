// The weight packs of the f16x3 / bf16 CIN kernels (cin_x3.hip): the per-element pack bodies, the job table of
// xdfm_cin_pack_all (all levels, both directions) and the two bodies its launches run -- the partial |W| maxima and the packs
// -- shared with the launches that carry them as riders (option "colaunch" bit 1, xdfm_cin_pack_defer in include/xdfm.h):
// the maxima under deferred Adam's catch-up (adam.hip), the packs under the embedding gather (embed.hip).
#pragma once
#include "cin_x3_fwd.h"

#define X3_ABSMAX_BLOCKS 64
#define X3_HDR_PART 64

__device__ __forceinline__ float x3_weight_scale(const float* __restrict__ hdr, int nparts) {
    float mx = 0.f;
    for (int k = 0; k < nparts; ++k) mx = fmaxf(mx, hdr[X3_HDR_PART + k]);
    return x3_pow2_scale(mx, 15);
}

// pack layout (after the X3_HDR-float header: [0] = sW, [1] = 1/sW, [64..127] = partial maxima of |W|):
//   [mb][g < NS+2][mt < MT][p: 0 = hi, 1 = lo][lane][8 halves]   -- 1 KB per (mt, p) fragment
// element t of lane (r = lane & 31, hh = lane >> 5) of step g = (blk, s):
//   row = (mb*MT + mt)*32 + r,  q = 8s + t,  il = q / m,  j = q % m,  i = blk*8 + hh*RH + il
// bf16 (nt == 1): no scale (sW = 1), one fragment per (g, mt): the bf16 bit patterns of W
__device__ __forceinline__ void x3_fwd_pack_one(const float* __restrict__ W, int H, int Hp, int m, const X3Geom& G,
                                                int nparts, float* __restrict__ pack, long idx, int nt) {
    const float sW = nt == 3 ? x3_weight_scale(pack, nparts) : 1.f;
    if (idx == 0) { pack[0] = sW; pack[1] = 1.f / sW; }
    const int lane = (int)(idx & 63);
    long rest = idx >> 6;
    const int mt = (int)(rest % G.MT); rest /= G.MT;
    const int g = (int)(rest % G.NSA);
    const int mb = (int)(rest / G.NSA);
    const int r = lane & 31, hh = lane >> 5;
    const int row = (mb * G.MT + mt) * 32 + r;
    int blk, s, RH;
    if (g < G.FB * G.MP) { blk = g / G.MP; s = g - blk * G.MP; RH = 4; }
    else { blk = G.FB; s = g - G.FB * G.MP; RH = G.RH; }
    h8 hi, lo;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int q = 8 * s + t, il = q / m, j = q - il * m;
        const int i = blk * 8 + hh * RH + il;
        float v = 0.f;
        if (g < G.NS && row < H && il < RH && i < Hp) v = W[(long)row * ((long)Hp * m) + (long)i * m + j] * sW;
        if (nt == 3) {
            const _Float16 a = (_Float16)v;
            hi[t] = a;
            lo[t] = (_Float16)(v - (float)a);
        } else {
            hi[t] = __builtin_bit_cast(_Float16, (__bf16)v);
        }
    }
    if (nt == 3) {
        h8* dst = reinterpret_cast<h8*>(pack + X3_HDR) + (((long)mb * G.NSA + g) * G.MT + mt) * 128 + lane;
        dst[0] = hi;
        dst[64] = lo;
    } else {
        reinterpret_cast<h8*>(pack + X3_HDR)[(((long)mb * G.NSA + g) * G.MT + mt) * 64 + lane] = hi;
    }
}

// folded pack of level 0 (x3_sym_*), same fragment layout with the SYM geometry; its own header: the folded weights
// reach twice the maximum, so their scale is half the one of the plain pack ([0] = sW/2, [1] = 2/sW).  `hdr` = the plain
// pack's header (partial maxima of |W|).
__device__ __forceinline__ void x3_fwd_pack_sym_one(const float* __restrict__ W, int H, int m, const X3Geom& G, int nparts,
                                                    const float* __restrict__ hdr, float* __restrict__ pack, long idx, int nt) {
    const float sW = nt == 3 ? 0.5f * x3_weight_scale(hdr, nparts) : 1.f;
    if (idx == 0) { pack[0] = sW; pack[1] = 1.f / sW; }
    const int lane = (int)(idx & 63);
    long rest = idx >> 6;
    const int mt = (int)(rest % G.MT); rest /= G.MT;
    const int g = (int)(rest % G.NSA);
    const int mb = (int)(rest / G.NSA);
    const int r = lane & 31, hh = lane >> 5;
    const int row = (mb * G.MT + mt) * 32 + r;
    const float* __restrict__ Wr = W + (long)(row < H ? row : 0) * ((long)m * m);
    h8 hi, lo;
    int i = x3_sym_i(m, 8 * g), j = x3_sym_j(m, 8 * g);        // slot 8g; the next ones follow along the list's rows
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int q = 8 * g + t;
        float v = 0.f;
        if (t > 0 && ++j > m - 1 - i) { ++i; j = i; }
        if (g < G.NS && row < H && q < x3_sym_pairs(m)) {
            const int a = hh ? m - 1 - i : i, b = hh ? m - 1 - j : j;
            if (a == b) v = Wr[a * m + a];
            else if (!(hh && i + j == m - 1)) v = Wr[a * m + b] + Wr[b * m + a];
            v *= sW;
        }
        if (nt == 3) {
            const _Float16 x = (_Float16)v;
            hi[t] = x;
            lo[t] = (_Float16)(v - (float)x);
        } else {
            hi[t] = __builtin_bit_cast(_Float16, (__bf16)v);
        }
    }
    if (nt == 3) {
        h8* dst = reinterpret_cast<h8*>(pack + X3_HDR) + (((long)mb * G.NSA + g) * G.MT + mt) * 128 + lane;
        dst[0] = hi;
        dst[64] = lo;
    } else {
        reinterpret_cast<h8*>(pack + X3_HDR)[(((long)mb * G.NSA + g) * G.MT + mt) * 64 + lane] = hi;
    }
}

// pack: [tile = iblk*m + j][hb < HBT][p][lane][8 halves]; element t of lane (r, hh):
//   W[h = 16*hb + 8*hh + t][(iblk*32 + r)*m + j] * sW   (0 outside); two dummy stages appended.
__device__ __forceinline__ void x3_bwx_pack_one(const float* __restrict__ W, int H, int Hp, int m, const X3BwxGeom& G,
                                                int nparts, float* __restrict__ pack, long idx, int nt) {
    const float sW = nt == 3 ? x3_weight_scale(pack, nparts) : 1.f;
    if (idx == 0) { pack[0] = sW; pack[1] = 1.f / sW; }
    const int lane = (int)(idx & 63);
    long rest = idx >> 6;
    const int hb = (int)(rest % G.HBT);
    const long tile = rest / G.HBT;
    const int j = (int)(tile % m);
    const int iblk = (int)(tile / m);
    const int r = lane & 31, hh = lane >> 5;
    const int i = iblk * 32 + r;
    h8 hi, lo;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int h = 16 * hb + 8 * hh + t;
        float v = 0.f;
        if (tile < G.NT && h < H && i < Hp) v = W[(long)h * ((long)Hp * m) + (long)i * m + j] * sW;
        if (nt == 3) {
            const _Float16 a = (_Float16)v;
            hi[t] = a;
            lo[t] = (_Float16)(v - (float)a);
        } else {
            hi[t] = __builtin_bit_cast(_Float16, (__bf16)v);
        }
    }
    if (nt == 3) {
        h8* dst = reinterpret_cast<h8*>(pack + X3_HDR) + (tile * G.HBT + hb) * 128 + lane;
        dst[0] = hi;
        dst[64] = lo;
    } else {
        reinterpret_cast<h8*>(pack + X3_HDR)[(tile * G.HBT + hb) * 64 + lane] = hi;
    }
}

// folded pack of level 0 for the dX kernel of cin_x3_bwx_sym.hip: [tile t < m/2][hb < HBT][p][lane][8 halves]; row r of
// tile t is the pair (i = r, j = t) for r <= t, (i = 31-r, j = m-1-t) for r >= 32-m+t, nothing in between; element
// W'[h = 16*hb + 8*hh + e][(i, j)] * sW / 2 with W'(i, j) = W(i, j) + W(j, i), W(i, i) on the diagonal.  Own header as in
// the forward's folded pack; `hdr` = the plain pack's header (partial maxima of |W|).
__device__ __forceinline__ void x3_bwx_pack_sym_one(const float* __restrict__ W, int H, int m, const X3BwxGeom& G, int nparts,
                                                    const float* __restrict__ hdr, float* __restrict__ pack, long idx, int nt) {
    const float sW = nt == 3 ? 0.5f * x3_weight_scale(hdr, nparts) : 1.f;
    if (idx == 0) { pack[0] = sW; pack[1] = 1.f / sW; }
    const int lane = (int)(idx & 63);
    long rest = idx >> 6;
    const int hb = (int)(rest % G.HBT);
    const int t = (int)(rest / G.HBT);
    const int r = lane & 31, hh = lane >> 5;
    int i = -1, j = 0;
    if (t < m / 2) {
        if (r <= t) { i = r; j = t; }
        else if (31 - r <= m - 1 - t) { i = 31 - r; j = m - 1 - t; }
    }
    h8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int h = 16 * hb + 8 * hh + e;
        float v = 0.f;
        if (i >= 0 && h < H) {
            const float* __restrict__ Wr = W + (long)h * ((long)m * m);
            v = (i == j ? Wr[i * m + i] : Wr[i * m + j] + Wr[j * m + i]) * sW;
        }
        if (nt == 3) {
            const _Float16 x = (_Float16)v;
            hi[e] = x;
            lo[e] = (_Float16)(v - (float)x);
        } else {
            hi[e] = __builtin_bit_cast(_Float16, (__bf16)v);
        }
    }
    if (nt == 3) {
        h8* dst = reinterpret_cast<h8*>(pack + X3_HDR) + ((long)t * G.HBT + hb) * 128 + lane;
        dst[0] = hi;
        dst[64] = lo;
    } else {
        reinterpret_cast<h8*>(pack + X3_HDR)[((long)t * G.HBT + hb) * 64 + lane] = hi;
    }
}

// ---- all levels, both directions, in two launches (the packs depend on the weights only) ----------------------
#define X3_MAXJOBS 8
struct X3PackJobs {
    const float* W[X3_MAXJOBS];
    float* fwd[X3_MAXJOBS];
    float* bwd[X3_MAXJOBS];
    float* fsym[X3_MAXJOBS];                 // folded forward pack of a level with Hp == m (null otherwise)
    float* bsym[X3_MAXJOBS];                 // folded dX pack, likewise
    int H[X3_MAXJOBS], Hp[X3_MAXJOBS], m[X3_MAXJOBS], nparts[X3_MAXJOBS];
    long nW[X3_MAXJOBS], fthreads[X3_MAXJOBS], bthreads[X3_MAXJOBS], sthreads[X3_MAXJOBS], bsthreads[X3_MAXJOBS];
    int nt;
    int L, maxparts, gx;                     // the launches' grids: maxima (maxparts, L), packs (gx, 4 L)
    X3Geom fg[X3_MAXJOBS], sg[X3_MAXJOBS];
    X3BwxGeom bg[X3_MAXJOBS];
};
static_assert(sizeof(X3PackJobs) + 1024 <= 8192, "the argument block of a launch that carries the pack jobs");

// host (cin_x3.hip holds the deferred jobs): the table for a host launch on `st` -> the rider workgroups it needs (0: nothing
// taken).  The maxima ride on 256-thread workgroups, one per (level, part); the packs on 256-thread workgroups, gx * 4 L of
// them -- and only behind the maxima: a host that takes the packs while the maxima are still pending launches those first.
long x3_pack_take_absmax(hipStream_t st, X3PackJobs* out);
long x3_pack_take_pack(hipStream_t st, X3PackJobs* out);

#ifdef __HIPCC__
// Partial maximum `part` of level l.  Written for any workgroup width that divides 1024 (a multiple of 64): thread t takes
// the elements threads t, t + width, ... of the 1024-thread workgroup of x3_absmax_multi_kernel take, and a maximum does not
// depend on the order -- the same nparts slots with the same bits.
__device__ __forceinline__ void x3_absmax_part(const X3PackJobs& J, int l, int part) {
    if (part >= J.nparts[l]) return;
    __shared__ float red[16];
    const float* __restrict__ W = J.W[l];
    const long total = J.nW[l], nv = total >> 2;
    const long stride = (long)J.nparts[l] * 1024;
    float v = 0.f;
    const bool vec = (((size_t)W) & 15) == 0;
    for (int sub = threadIdx.x; sub < 1024; sub += blockDim.x) {
        if (vec) {
            for (long i = (long)part * 1024 + sub; i < nv; i += stride) {
                const float4 a = reinterpret_cast<const float4*>(W)[i];
                v = fmaxf(fmaxf(v, fmaxf(fabsf(a.x), fabsf(a.y))), fmaxf(fabsf(a.z), fabsf(a.w)));
            }
        }
        for (long i = (vec ? nv * 4 : 0) + (long)part * 1024 + sub; i < total; i += stride) v = fmaxf(v, fabsf(W[i]));
    }
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x < 16) {
        v = threadIdx.x < (blockDim.x >> 6) ? red[threadIdx.x] : 0.f;
        for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
        if (threadIdx.x == 0) {
            if (J.fwd[l]) J.fwd[l][X3_HDR_PART + part] = v;
            if (J.bwd[l]) J.bwd[l][X3_HDR_PART + part] = v;
        }
    }
}

// Workgroup (bx, by) of the packs' (gx, 4 L) grid: level by / 4, direction by % 4, a grid-stride walk over the pack's elements
__device__ __forceinline__ void x3_pack_block(const X3PackJobs& J, int bx, int by, int gx) {
    const int l = by >> 2, dir = by & 3;
    const long stride = (long)gx * blockDim.x;
    const long first = (long)bx * blockDim.x + threadIdx.x;
    if (dir == 3) {
        if (!J.bsym[l]) return;
        for (long idx = first; idx < J.bsthreads[l]; idx += stride)
            x3_bwx_pack_sym_one(J.W[l], J.H[l], J.m[l], J.bg[l], J.nparts[l], J.bwd[l], J.bsym[l], idx, J.nt);
    } else if (dir == 2) {
        if (!J.fsym[l]) return;
        for (long idx = first; idx < J.sthreads[l]; idx += stride)
            x3_fwd_pack_sym_one(J.W[l], J.H[l], J.m[l], J.sg[l], J.nparts[l], J.fwd[l], J.fsym[l], idx, J.nt);
    } else if (dir == 0) {
        if (!J.fwd[l]) return;
        for (long idx = first; idx < J.fthreads[l]; idx += stride)
            x3_fwd_pack_one(J.W[l], J.H[l], J.Hp[l], J.m[l], J.fg[l], J.nparts[l], J.fwd[l], idx, J.nt);
    } else {
        if (!J.bwd[l]) return;
        for (long idx = first; idx < J.bthreads[l]; idx += stride)
            x3_bwx_pack_one(J.W[l], J.H[l], J.Hp[l], J.m[l], J.bg[l], J.nparts[l], J.bwd[l], idx, J.nt);
    }
}
// rider workgroups (rider.h): the maxima's, rb < maxparts * L; the packs', rb < gx * 4 L
__device__ __forceinline__ void x3_absmax_rider(const X3PackJobs& J, long rb) {
    if (rb < (long)J.maxparts * J.L) x3_absmax_part(J, (int)(rb / J.maxparts), (int)(rb % J.maxparts));
}
__device__ __forceinline__ void x3_pack_rider(const X3PackJobs& J, long rb) {
    if (rb < (long)J.gx * 4 * J.L) x3_pack_block(J, (int)(rb % J.gx), (int)(rb / J.gx), J.gx);
}
#endif
