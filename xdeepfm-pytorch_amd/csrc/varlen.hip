// K1v / K2v: pooled variable-length fields (VarLenSparseFeat).
//
// replaces deepctr/inputs.py:213-227 (varlen_embedding_lookup: maxlen rows per example and field), :141-155
// (get_varlen_pooling_list) and deepctr/layers/sequence.py:49-77 (SequencePoolingLayer: mask, sum / mean / max), as
// input_from_feature_columns (basemodel.py:372-377) and Linear.forward (:72-77) call them, with ONE launch for all fields
// of a model; the [B, maxlen, D] rows and their masks are never written to memory.
//
// Forward: one thread per (example, column), column D being the [V, 1] linear table; the thread walks the fields and the
// positions of each.  The D + 1 threads of an example read the same ids (one cache line, broadcast) and consecutive
// floats of the same table row.  Results go straight to their three consumers: the CIN input in FM layout (field slot
// slot0 + f), the DNN input row, the linear logit (added to what K1 wrote).
// Backward: no float atomics.  An expand kernel writes one row gradient per (example, position) -- B * Tmax
// pseudo-examples per field; zeros where padded up to Tmax, where masked (sum, mean) and everywhere but the recorded position
// (max: that position gets g even when it is masked, as on an empty sequence) -- and K2's exact segmented reduce adds them up by id
// (embed.hip): a pure function of the multiset of rows per chunk, chunks in ascending order, bit-identical from run to run.
#include "xdfm_internal.h"

#define VL_THREADS 256

// valid positions of one (example, field): the length column's value, or the count of non-zero ids
__device__ __forceinline__ long vl_length(const float* __restrict__ xrow, const xdfm_varlen_field& fd) {
    if (fd.len_col >= 0) return (long)xrow[fd.len_col];               // truncation as Tensor.long() (inputs.py:151)
    long n = 0;
    for (int t = 0; t < fd.maxlen; ++t) n += ((long)xrow[fd.col + t] != 0) ? 1 : 0;
    return n;
}

// One (example, field, column): the pooled value, and for max the position of the first maximum.  The forward and the
// exchanged-rows backward (which recomputes that position instead of being handed it) share this walk, so both pick the same
// position: validity by the length column or id != 0, masked positions compete as w - 1e9, ties go to the lowest position.
__device__ __forceinline__ float vl_pool_one(const float* __restrict__ xrow, const xdfm_varlen_field& fd, const float* __restrict__ tab,
                                             int stride, int off, int* pos_out, bool* bad) {
    const long len = fd.len_col >= 0 ? (long)xrow[fd.len_col] : 0;
    float acc = 0.f, best = 0.f;
    int pos = 0;
    long cnt = 0;
    for (int t = 0; t < fd.maxlen; ++t) {
        long id = (long)xrow[fd.col + t];                          // truncation as Tensor.long() (inputs.py:225)
        const bool valid = fd.len_col >= 0 ? (long)t < len : id != 0;
        if (id < 0 || id >= fd.vocab) {                            // every position is looked up, padded ones included
            *bad = true;
            id = id < 0 ? 0 : fd.vocab - 1;
        }
        const float w = tab[id * stride + off];
        if (fd.combiner == XDFM_POOL_MAX) {
            const float v = valid ? w : w - 1e9f;                  // w - (1 - mask) * 1e9 (sequence.py:66)
            if (t == 0 || v > best) { best = v; pos = t; }         // the first maximum
        } else if (valid) {
            acc += w;
            ++cnt;
        }
    }
    *pos_out = pos;
    if (fd.combiner == XDFM_POOL_MEAN) return acc / ((float)(fd.len_col >= 0 ? len : cnt) + 1e-8f);   // sequence.py:74
    return fd.combiner == XDFM_POOL_MAX ? best : acc;
}

__global__ __launch_bounds__(VL_THREADS) void varlen_pool_fwd_kernel(
    const float* __restrict__ X, long ldx, int B, const xdfm_varlen_field* __restrict__ fields, int F, int D, int slot0,
    float* __restrict__ emb_fm, float* __restrict__ dnn_in, long ld_dnn, int dnn_off, float* __restrict__ lin_out,
    unsigned char* __restrict__ argpos, int* __restrict__ err_flag) {
    const int W = D + 1;
    const long idx = (long)blockIdx.x * VL_THREADS + threadIdx.x;
    if (idx >= (long)B * W) return;
    const int b = (int)(idx / W), d = (int)(idx - (long)b * W);
    const bool is_lin = d == D;
    if (is_lin ? lin_out == nullptr : (emb_fm == nullptr && dnn_in == nullptr)) return;
    const float* xrow = X + (long)b * ldx;
    const long N = (long)B * D;
    float lin_acc = 0.f;
    bool bad = false;
    for (int f = 0; f < F; ++f) {
        const xdfm_varlen_field fd = fields[f];
        int pos = 0;
        const float r = vl_pool_one(xrow, fd, is_lin ? fd.lin : fd.table, is_lin ? 1 : D, is_lin ? 0 : d, &pos, &bad);
        if (is_lin) {
            lin_acc += r;
        } else {
            if (emb_fm) emb_fm[(long)(slot0 + f) * N + (long)b * D + d] = r;
            if (dnn_in) dnn_in[(long)b * ld_dnn + dnn_off + (long)f * D + d] = r;
        }
        if (argpos) argpos[((long)b * F + f) * W + d] = (unsigned char)pos;
    }
    if (is_lin) lin_out[b] += lin_acc;
    if (bad && err_flag) atomicOr(err_flag, 1);
}

// Exchanged rows (row-parallel training): the positions of the maxima of R rows that this rank did not run the forward for,
// from the tables as they are before the update -- [R][F][D + 1] bytes as the forward writes them, 0 for sum and mean fields,
// whose ids are only checked against the vocabulary (by the linear column's thread).  One thread per (row, column).
__global__ __launch_bounds__(VL_THREADS) void varlen_rows_argpos_kernel(
    const float* __restrict__ X, long ldx, int R, const xdfm_varlen_field* __restrict__ fields, int F, int D, bool tabs, bool lins,
    unsigned char* __restrict__ argpos, int* __restrict__ err_flag) {
    const int W = D + 1;
    const long idx = (long)blockIdx.x * VL_THREADS + threadIdx.x;
    if (idx >= (long)R * W) return;
    const int r = (int)(idx / W), d = (int)(idx - (long)r * W);
    const bool is_lin = d == D;
    const float* xrow = X + (long)r * ldx;
    bool bad = false;
    for (int f = 0; f < F; ++f) {
        const xdfm_varlen_field fd = fields[f];
        int pos = 0;
        if (fd.combiner == XDFM_POOL_MAX) {
            if (is_lin ? lins : tabs) vl_pool_one(xrow, fd, is_lin ? fd.lin : fd.table, is_lin ? 1 : D, is_lin ? 0 : d, &pos, &bad);
        } else if (is_lin) {
            for (int t = 0; t < fd.maxlen; ++t) {
                const long id = (long)xrow[fd.col + t];
                bad = bad || id < 0 || id >= fd.vocab;
            }
        }
        argpos[((long)r * F + f) * W + d] = (unsigned char)pos;
    }
    if (bad && err_flag) atomicOr(err_flag, 1);
}

// Row gradients per position.  Pseudo-example p = b * Tmax + t; ids_out [B*Tmax][F], g_rows [F][B*Tmax][D], g_lin [F][B*Tmax].
__global__ __launch_bounds__(VL_THREADS) void varlen_pool_expand_kernel(
    const float* __restrict__ X, long ldx, int B, const xdfm_varlen_field* __restrict__ fields, int F, int D, int Tmax, int slot0,
    const float* __restrict__ d_emb_fm, const float* __restrict__ d_dnn_in, long ld_dnn, int dnn_off,
    const float* __restrict__ d_lin, long ld_lin, const unsigned char* __restrict__ argpos, float* __restrict__ ids_out,
    float* __restrict__ g_rows, float* __restrict__ g_lin) {
    const int W = D + 1;
    const long total = (long)B * F * Tmax * W;
    const long idx = (long)blockIdx.x * VL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int d = (int)(idx % W);
    long rest = idx / W;
    const int t = (int)(rest % Tmax);
    rest /= Tmax;
    const int f = (int)(rest % F);
    const int b = (int)(rest / F);
    const bool is_lin = d == D;
    const xdfm_varlen_field fd = fields[f];
    const float* xrow = X + (long)b * ldx;
    const long P = (long)B * Tmax, p = (long)b * Tmax + t;
    const bool inside = t < fd.maxlen;
    const float idv = inside ? xrow[fd.col + t] : 0.f;
    if (is_lin) ids_out[p * F + f] = idv;
    float* dst = is_lin ? (g_lin ? g_lin + (long)f * P + p : nullptr) : (g_rows ? g_rows + ((long)f * P + p) * D + d : nullptr);
    if (!dst) return;
    float val = 0.f;
    if (inside) {
        const long len = (fd.combiner != XDFM_POOL_MAX && (fd.len_col >= 0 || fd.combiner == XDFM_POOL_MEAN)) ? vl_length(xrow, fd) : 0;   // the count is the mean's divisor only
        // sum, mean: the valid positions.  max: the recorded position, valid or not -- torch.max over emb - (1 - mask) * 1e9
        // (sequence.py:65-68) sends the gradient to its first maximum, which on an all-masked sequence is a masked position
        const bool take = fd.combiner == XDFM_POOL_MAX ? (int)argpos[((long)b * F + f) * W + d] == t
                                                       : (fd.len_col >= 0 ? (long)t < len : (long)idv != 0);
        if (take) {
            float g;
            if (is_lin) {
                g = d_lin ? d_lin[(long)b * ld_lin] : 0.f;
            } else {
                const long N = (long)B * D;
                const float ge = d_emb_fm ? d_emb_fm[(long)(slot0 + f) * N + (long)b * D + d] : 0.f;
                const float gd = d_dnn_in ? d_dnn_in[(long)b * ld_dnn + dnn_off + (long)f * D + d] : 0.f;
                g = ge + gd;                       // one fp32 add, as autograd's accumulation of the two uses of the pooled row
            }
            val = fd.combiner == XDFM_POOL_MEAN ? g / ((float)len + 1e-8f) : g;
        }
    }
    *dst = val;
}

static int vl_check_fields(const char* what, const xdfm_varlen_field* fh, int F, long ldx, bool need_table, bool need_lin, int* tmax) {
    int tm = 0;
    for (int f = 0; f < F; ++f) {
        XDFM_REQUIRE(fh[f].maxlen >= 1 && fh[f].maxlen <= 255, "%s: field %d maxlen %d outside 1..255", what, f, fh[f].maxlen);
        XDFM_REQUIRE(fh[f].col >= 0 && (long)fh[f].col + fh[f].maxlen <= ldx, "%s: field %d columns %d..%d outside X (ldx=%ld)", what, f,
                     fh[f].col, fh[f].col + fh[f].maxlen - 1, ldx);
        XDFM_REQUIRE(fh[f].len_col >= -1 && fh[f].len_col < ldx, "%s: field %d length column %d outside X (ldx=%ld)", what, f, fh[f].len_col, ldx);
        XDFM_REQUIRE(fh[f].combiner >= XDFM_POOL_SUM && fh[f].combiner <= XDFM_POOL_MAX, "%s: field %d unknown combiner %d", what, f, fh[f].combiner);
        XDFM_REQUIRE(fh[f].vocab >= 1, "%s: field %d vocabulary %d", what, f, fh[f].vocab);
        XDFM_REQUIRE(!need_table || fh[f].table, "%s: field %d has no table", what, f);
        XDFM_REQUIRE(!need_lin || fh[f].lin, "%s: field %d has no linear table", what, f);
        if (fh[f].maxlen > tm) tm = fh[f].maxlen;
    }
    *tmax = tm;
    return XDFM_OK;
}

extern "C" {

int xdfm_varlen_pool_fwd(const float* X, long ldx, int B, const xdfm_varlen_field* fields, const xdfm_varlen_field* fields_host,
                         int F, int D, int slot0, float* emb_fm, float* dnn_in, long ld_dnn, int dnn_off, float* lin_out,
                         unsigned char* argpos, int* err_flag, void* stream) {
    XDFM_REQUIRE(X && fields && fields_host, "varlen_pool_fwd: null pointer");
    XDFM_REQUIRE(B > 0 && F > 0 && D > 0 && slot0 >= 0, "varlen_pool_fwd: bad shape B=%d F=%d D=%d slot0=%d", B, F, D, slot0);
    XDFM_REQUIRE(emb_fm || dnn_in || lin_out, "varlen_pool_fwd: no output");
    XDFM_REQUIRE(!dnn_in || (dnn_off >= 0 && ld_dnn >= (long)dnn_off + (long)F * D), "varlen_pool_fwd: bad dnn_in layout ld_dnn=%ld dnn_off=%d",
                 ld_dnn, dnn_off);
    int tmax = 0;
    const int rc = vl_check_fields("varlen_pool_fwd", fields_host, F, ldx, emb_fm || dnn_in, lin_out != nullptr, &tmax);
    if (rc) return rc;
    const long threads = (long)B * (D + 1);
    XDFM_REQUIRE(threads / VL_THREADS < 0x7fffffffL, "varlen_pool_fwd: batch too large");
    hipLaunchKernelGGL(varlen_pool_fwd_kernel, dim3(ceil_div(threads, VL_THREADS)), dim3(VL_THREADS), 0, (hipStream_t)stream, X, ldx, B,
                       fields, F, D, slot0, emb_fm, dnn_in, ld_dnn, dnn_off, lin_out, argpos, err_flag);
    return xdfm_check_launch("varlen_pool_fwd");
}

// ws: [g_rows F*P*D | g_lin F*P | ids P*F], P = B*Tmax; each part starts on a 16-byte boundary
static inline size_t vl_pad4(size_t n) { return (n + 3) / 4 * 4; }

size_t xdfm_varlen_pool_bwd_ws_elems(long B, int F, int D, int Tmax) {
    if (B <= 0 || F <= 0 || D <= 0 || Tmax <= 0) return 0;
    const size_t P = (size_t)B * Tmax;
    return vl_pad4(P * F * D) + vl_pad4(P * F) + vl_pad4(P * F);
}

int xdfm_varlen_pool_bwd(const float* X, long ldx, int B, const xdfm_varlen_field* fields, const xdfm_varlen_field* fields_host,
                         int F, int D, int slot0, const float* d_emb_fm, const float* d_dnn_in, long ld_dnn, int dnn_off,
                         const float* d_lin, long ld_lin, const unsigned char* argpos, const int* cols, const int* vocab,
                         float* d_flat, const long* tab_off, const long* lin_off, float* ws, void* stream) {
    XDFM_REQUIRE(X && fields && fields_host && cols && vocab && d_flat && ws, "varlen_pool_bwd: null pointer");
    XDFM_REQUIRE(B > 0 && F > 0 && D > 0 && slot0 >= 0, "varlen_pool_bwd: bad shape B=%d F=%d D=%d slot0=%d", B, F, D, slot0);
    XDFM_REQUIRE(!d_dnn_in || (dnn_off >= 0 && ld_dnn >= (long)dnn_off + (long)F * D), "varlen_pool_bwd: bad d_dnn_in layout ld_dnn=%ld dnn_off=%d",
                 ld_dnn, dnn_off);
    XDFM_REQUIRE((((size_t)ws) & 15) == 0 && (((size_t)d_flat) & 15) == 0, "varlen_pool_bwd: ws and d_flat must be 16-byte aligned");
    if (ld_lin <= 0) ld_lin = 1;
    const bool tabs = tab_off && (d_emb_fm || d_dnn_in);
    const bool lins = lin_off && d_lin;
    if (!tabs && !lins) return XDFM_OK;
    int tmax = 0;
    int rc = vl_check_fields("varlen_pool_bwd", fields_host, F, ldx, false, false, &tmax);
    if (rc) return rc;
    bool any_max = false;
    for (int f = 0; f < F; ++f) any_max = any_max || fields_host[f].combiner == XDFM_POOL_MAX;
    XDFM_REQUIRE(!any_max || argpos, "varlen_pool_bwd: a max-pooled field needs argpos of the forward");
    const long P = (long)B * tmax;
    XDFM_REQUIRE(P < 0x7fffffffL, "varlen_pool_bwd: B * Tmax = %ld too large", P);
    float* g_rows = ws;
    float* g_lin = g_rows + vl_pad4((size_t)P * F * D);
    float* ids = g_lin + vl_pad4((size_t)P * F);
    const long threads = P * F * (D + 1);
    XDFM_REQUIRE(threads / VL_THREADS < 0x7fffffffL, "varlen_pool_bwd: batch too large");
    hipLaunchKernelGGL(varlen_pool_expand_kernel, dim3(ceil_div(threads, VL_THREADS)), dim3(VL_THREADS), 0, (hipStream_t)stream, X, ldx, B,
                       fields, F, D, tmax, slot0, d_emb_fm, d_dnn_in, ld_dnn, dnn_off, d_lin, ld_lin, argpos, ids,
                       tabs ? g_rows : nullptr, lins ? g_lin : nullptr);
    rc = xdfm_check_launch("varlen_pool_bwd (expand)");
    if (rc) return rc;
    if (tabs) {
        rc = xdfm_embed_scatter_bwd_marked(ids, F, (int)P, cols, vocab, F, D, nullptr, 0, g_rows, nullptr, 0, nullptr, 0, d_flat, tab_off,
                                           nullptr, nullptr, nullptr, stream);
        if (rc) return rc;
    }
    if (lins)       // the [V, 1] tables: the same reduce with rows of one float
        rc = xdfm_embed_scatter_bwd_marked(ids, F, (int)P, cols, vocab, F, 1, nullptr, 0, g_lin, nullptr, 0, nullptr, 0, d_flat, lin_off,
                                           nullptr, nullptr, nullptr, stream);
    return rc;
}

// ws: [what xdfm_varlen_pool_bwd takes for R rows | argpos R*F*(D+1) bytes], the second part on a 16-byte boundary
size_t xdfm_varlen_pool_bwd_rows_ws_elems(long R, int F, int D, int Tmax) {
    if (R <= 0 || F <= 0 || D <= 0 || Tmax <= 0) return 0;
    return xdfm_varlen_pool_bwd_ws_elems(R, F, D, Tmax) + vl_pad4(((size_t)R * F * (D + 1) + 3) / 4);
}

int xdfm_varlen_pool_bwd_rows(const float* X, long ldx, int R, const xdfm_varlen_field* fields, const xdfm_varlen_field* fields_host,
                              int F, int D, int slot0, const float* g_rows, long ld_g, const float* d_lin, long ld_lin,
                              const int* cols, const int* vocab, float* d_flat, const long* tab_off, const long* lin_off, float* ws,
                              int* err_flag, void* stream) {
    XDFM_REQUIRE(X && fields && fields_host && cols && vocab && d_flat && ws, "varlen_pool_bwd_rows: null pointer");
    XDFM_REQUIRE(R > 0 && F > 0 && D > 0 && slot0 >= 0, "varlen_pool_bwd_rows: bad shape R=%d F=%d D=%d slot0=%d", R, F, D, slot0);
    XDFM_REQUIRE(!g_rows || ld_g >= ((long)slot0 + F) * D, "varlen_pool_bwd_rows: ld_g=%ld smaller than (slot0 + F) * D = %ld", ld_g,
                 ((long)slot0 + F) * D);
    XDFM_REQUIRE((((size_t)ws) & 15) == 0, "varlen_pool_bwd_rows: ws must be 16-byte aligned");
    const bool tabs = tab_off && g_rows;
    const bool lins = lin_off && d_lin;
    if (!tabs && !lins) return XDFM_OK;
    int tmax = 0;
    // the argmax walk reads the tables: those whose gradient is asked for must be there
    const int rc = vl_check_fields("varlen_pool_bwd_rows", fields_host, F, ldx, tabs, lins, &tmax);
    if (rc) return rc;
    XDFM_REQUIRE((long)R * tmax < 0x7fffffffL, "varlen_pool_bwd_rows: R * Tmax = %ld too large", (long)R * tmax);
    unsigned char* argpos = reinterpret_cast<unsigned char*>(ws + xdfm_varlen_pool_bwd_ws_elems(R, F, D, tmax));
    const long threads = (long)R * (D + 1);
    hipLaunchKernelGGL(varlen_rows_argpos_kernel, dim3(ceil_div(threads, VL_THREADS)), dim3(VL_THREADS), 0, (hipStream_t)stream, X, ldx, R,
                       fields, F, D, tabs, lins, argpos, err_flag);
    const int rl = xdfm_check_launch("varlen_pool_bwd_rows (argpos)");
    if (rl) return rl;
    // the exchanged row gradients have the DNN input's layout: example-major, field slot0 + f at column (slot0 + f) * D
    return xdfm_varlen_pool_bwd(X, ldx, R, fields, fields_host, F, D, slot0, nullptr, g_rows, ld_g, slot0 * D, d_lin, ld_lin, argpos, cols,
                                vocab, d_flat, tab_off, lin_off, ws, stream);
}

}  // extern "C"
