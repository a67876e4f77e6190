/*
 * xdfm.h -- C ABI of libxdfm_hip.so: the MI355X (gfx950) hot path of xDeepFM.
 *
 * The reference (Syclus123/xDeepFM-pytorch) has no FFI: its boundary for this path is a
 * Python class API made of stock ATen calls.  Every entry point below replaces one group of
 * those calls; the citation after "replaces:" is the reference file:line (relative to the
 * reference root) whose arithmetic the kernel reproduces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked [host]; buffers are caller-allocated;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and never
 *     synchronise, allocate or free (safe under hipGraph capture);
 *   - return value: 0 = ok, otherwise an XDFM_ERR_* code; xdfm_last_error() gives the text;
 *   - "FM layout" (feature-map major) of an activation with R rows for a batch of B examples
 *     and embedding width D:  T[r][n], n = b*D + d, row pitch N = B*D floats.  It is the
 *     reference's [B, R, D] tensor with the R axis outermost, so that the 64 lanes of a
 *     wavefront read consecutive n and one example's D values are contiguous.
 *   - operands, accumulators and results are IEEE fp32 ("dtype f32").  The CIN contractions run either on
 *     v_mfma_f32_32x32x2_f32 or, by default, as three v_mfma_f32_32x32x16_f16 per fp32 product on operands
 *     split into fp16 hi + lo halves with fp32 accumulation, or (opt-in) as one v_mfma_f32_32x32x16_bf16 on operands
 *     rounded to bf16 (option "cin_math", see xdfm_set_option);
 *   - nothing in the library issues a memset (hipMemsetAsync nodes inside a captured graph are not ordered
 *     reliably on ROCm 7.2 / gfx950); reductions use per-block partials and fixed-order finish kernels.
 *
 * ABI 2 (this round): + cin_math option and f16x3 pack / workspace layouts, xdfm_cin_pack_all,
 * xdfm_cin_level_bwd_x_ex, xdfm_colsum, xdfm_head_fwd/bwd (K8), xdfm_adam_step (K7), xdfm_graph_node_census.
 * ABI 3: + xdfm_embed_scatter_bwd_marked and xdfm_adam_tensor.grad_marks (gradient buffer kept across steps),
 * xdfm_relu_bwd_colsum.
 * ABI 4: K2 is a sorted, segmented, exact reduce (no atomics; same entry points), xdfm_adam_step_lr (learning rate
 * from a device scalar), read-only options "last_fwd_kernel" / "last_bwx_kernel" / "last_bww_kernel".
 * ABI 5: attention dropout in K5 (p_drop, drop_seed on xdfm_cin_attn_pool_fwd/bwd; xdfm_cin_attn_dropout_mask).
 * ABI 6: deferred (exact) Adam for the tables: xdfm_adam_tensor.last, XDFM_ADAM_DEFERRED, xdfm_adam_clock,
 * xdfm_adam_step_deferred, xdfm_adam_catchup_rows, xdfm_adam_flush.
 * ABI 7: xdfm_cin_bwd_x_is_folded (a pure query instead of the "last_sym" probe on the product path); the deferred update's
 * constant table holds 4 floats per step (xdfm_adam_clock.consts: 4 * cap) and its replayed steps run the short forms of
 * csrc/adam_math.h (same bits, about half the issue slots); xdfm_adam_selftest; xdfm_cin_bwd_prep +
 * xdfm_cin_level_bwd_w_prepared (dOut, its fp16 planes and the dW kernel's scales in one pass);
 * xdfm_cin_attn_pool_bwd_det (K5's parameter gradients without float atomics); xdfm_cin_level_fwd_ex (direct-connect sums
 * and ReLU sign bits from the forward's epilogue; the direct-connect half of a level is never stored).
 * ABI 8 additions (no existing struct or signature changed): xdfm_opt_tensor, xdfm_opt_step_ws_elems, xdfm_sgd_step,
 * xdfm_adagrad_step (K7s / K7g: the streaming sweep for the trainer's two other optimizers); xdfm_opt_clock, xdfm_opt_rows,
 * xdfm_sgd_step_deferred, xdfm_adagrad_step_deferred, xdfm_opt_catchup_rows, xdfm_opt_flush (K7sd / K7gd: their deferred form);
 * xdfm_rmsprop_step, xdfm_rmsprop_step_deferred, xdfm_rmsprop_catchup_rows, xdfm_rmsprop_flush (K7r / K7rd: RMSprop);
 * xdfm_autodis_supported, xdfm_autodis_ws_elems, xdfm_autodis_fwd, xdfm_autodis_bwd (K10: AutoDis of xdeepfm_pro).
 * Further ABI 8 additions (no existing struct or signature changed, so the version stays: a caller built against the earlier
 * ABI 8 header keeps working, and the binding checks every symbol it needs by name): xdfm_embed_gather_fwd_ld (K1 with a row pitch and a dense-column
 * offset for dnn_in), xdfm_varlen_field, xdfm_varlen_pool_fwd, xdfm_varlen_pool_bwd_ws_elems, xdfm_varlen_pool_bwd
 * (K1v / K2v: pooled variable-length fields); XDFM_LINK_*, XDFM_LOSS_*, xdfm_head_fwd_ex, xdfm_head_bwd_ex (K8 with a
 * compile-time link and loss: the regression task and the mse / mae losses); xdfm_compact_rows_fwd / _bwd (K11: positive-row
 * compaction with the count on the device) and xdfm_vocab_ce_pack_hidden_n, _fwd_n, _pack_g_n, _bwd_h_n, _bwd_w_n (K9 with a
 * device-side row count: the SFG branch of the xDeepFMPro step with batch-shaped launches, so the step can be captured);
 * xdfm_compact_rows_fwd_n (K11 whose normaliser is counted over a second label vector: the global batch of a row-parallel step).
 * xdfm_varlen_pool_bwd_rows_ws_elems, xdfm_varlen_pool_bwd_rows (K2v over the exchanged rows of a row-parallel step: the positions
 * of the maxima are recomputed, not passed) -- additions again, the version stays 8.
 * xdfm_dense_fwd_drop, xdfm_dense_bwd_x_drop, xdfm_dense_bwd_w_drop, xdfm_dense_dropout_mask (dropout of the DNN tower inside
 * the dense kernels: a hashed keep mask, read back off the stored output) -- additions, the version stays 8.
 * xdfm_bn_row_block, xdfm_bn_ws_elems, xdfm_bn_fwd_train, xdfm_bn_fwd_eval, xdfm_bn_bwd, xdfm_bn_bwd_eval (K12: batch norm of a
 * dense layer's output fused with its activation, csrc/bn.hip) -- additions, the version stays 8.
 * xdfm_dense_prelu_fwd, xdfm_dense_prelu_bwd_x, xdfm_dense_prelu_bwd_w, xdfm_dense_prelu_bwd_w_ws_elems (the dense kernels with a
 * PReLU of one scalar slope: dnn_activation='prelu') and xdfm_prelu_ws_elems, xdfm_prelu_fwd, xdfm_prelu_bwd (K13: the same
 * PReLU elementwise, csrc/prelu.hip) -- additions, the version stays 8.
 * xdfm_bn_stats, xdfm_bn_fwd_apply_sync, xdfm_bn_bwd_sums, xdfm_bn_bwd_apply_sync (K12 split around an all-gather: batch norm
 * over the global batch of a row-parallel step) -- additions, the version stays 8.
 * xdfm_head_fwd_w, xdfm_head_bwd_w (K8 with one weight per example: sample_weight / class_weight of fit()) -- additions, the
 * version stays 8.
 * xdfm_varlen_pool_bwd / _bwd_rows: an XDFM_POOL_MAX field now sends the gradient of an all-masked sequence to the recorded
 * (masked) position instead of dropping it -- a correction of the values, no struct or signature changed, the version stays 8.
 * xdfm_sgdm_step, xdfm_sgdm_step_deferred, xdfm_sgdm_catchup_rows, xdfm_sgdm_flush (K7m / K7md: SGD with momentum, plain or
 * Nesterov; xdfm_opt_tensor keeps its 48 bytes, `state` is the momentum buffer) -- additions, the version stays 8.
 * xdfm_finish_batch_begin, xdfm_finish_batch_run, xdfm_finish_batch_active, xdfm_finish and the option "finish_batch" (the
 * one-block "finish" launches of a train step collected into one launch) -- additions, the version stays 8.
 * XDFM_METRIC_*, xdfm_batch_metrics_ws_bytes, xdfm_batch_metrics (K14: the per-batch training metrics of fit() in two
 * launches) -- additions, the version stays 8.
 * ABI 9: the export that registered a device array for last-block finishes inside the producer kernels (added with ABI 7, opt-in,
 * measured slower) is removed; the finish batch saves those launches.  Nothing else changes.
 * xdfm_ftrl_tensor, xdfm_ftrl_step (K7f: per-coordinate FTRL-Proximal, a descriptor with two state arrays) -- additions, the
 * version stays 9.
 * XDFM_ROWWISE_MAX_DIM, xdfm_rowwise_tensor, xdfm_rowwise_adagrad_step (K7w: row-wise Adagrad, one accumulator per table row) --
 * additions, the version stays 9.
 * xdfm_eval_metrics_ws_bytes, xdfm_eval_metrics (K14s: the four metrics of evaluate() for up to 2^27 rows, the AUC by a radix
 * sort) -- additions, the version stays 9.
 * xdfm_eval_metrics_w_ws_bytes, xdfm_eval_metrics_w (K14w: K14s with one weight per row, the weighted_metrics of evaluate() and
 * fit()) -- additions, the version stays 9.
 */
#ifndef XDFM_H
#define XDFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XDFM_ABI_VERSION 9

enum {
    XDFM_OK = 0,
    XDFM_ERR_INVALID = 1,   /* bad shape / null pointer / unsupported option / unknown link, loss or (identity, bce) */
    XDFM_ERR_LAUNCH = 2,    /* HIP reported an error at launch */
    XDFM_ERR_NO_DEVICE = 3
};

/* `act` of the CIN entry points.  XDFM_ACT_RELU: max(v, 0); levels may keep 1 sign bit per element instead of the output
 * (the `mask` arguments).  XDFM_ACT_SIGMOID: 1 / (1 + exp(-v)) in fp32 (accurate exp, true division); its backward
 * y (1 - y) needs the stored fp32 output, so `mask` must be NULL with it.  Any other value: XDFM_ERR_INVALID. */
enum { XDFM_ACT_LINEAR = 0, XDFM_ACT_RELU = 1, XDFM_ACT_SIGMOID = 2 };

int xdfm_abi_version(void);
const char* xdfm_last_error(void);          /* [host] thread-local, never NULL */
int xdfm_device_count(void);                /* <0: HIP error code negated */
/* tuning knobs for A/B runs (e.g. "fwd_nf", "bww_nsplit"); unknown key -> XDFM_ERR_INVALID.
 * "cin_math": arithmetic of the CIN contraction (K3 / K4).  Operands, accumulators and results are fp32
 * in both modes; the packed-weight and workspace layouts (and the *_elems sizes) depend on the mode, so
 * set it before the *_pack_elems / *_ws_elems calls of a step and keep it for that step.
 *   1 (default) "f16x3": each fp32 operand is split into two fp16 halves (hi + lo, 22 mantissa bits, exact
 *      power-of-two range fitting) and each product is three v_mfma_f32_32x32x16_f16 accumulated in fp32;
 *      error against an fp64 evaluation <= that of mode 0 (tests/test_gpu_parity.py); shapes without an
 *      f16x3 kernel (odd field counts in the forward, H <= 64 in dW, ...) run mode 0 kernels;
 *   0 "f32mfma": v_mfma_f32_32x32x2_f32 on the fp32 operands;
 *   2 "bf16" (BASELINE config 5's arithmetic): operands rounded to bf16 (RNE), ONE v_mfma_f32_32x32x16_bf16 per
 *      product, fp32 accumulation, fp32 results; no range fitting (bf16 has fp32's exponent range).  Its tolerance is
 *      its own: 2e-2 (outputs) / 4e-2 (gradients) of a tensor's largest magnitude against the fp32 reference,
 *      measured 3e-3 / 8e-3 (tests/test_gpu_parity.py::test_cin_bf16_mfma_path_vs_fp32_oracle).  Kernels exist for
 *      H > 64 (forward, dW), 32 < H <= 256 per call (dX), m in {22, 26}; other shapes run mode 0. */
/* "x3_sym" (default 1): level 0 of a CIN, where x_prev IS x0 (the calls get xp == x0; interaction.py:214-224), is
 * symmetric in (i, j).  With x3_sym != 0 the f16x3 / bf16 kernels of that level contract over the pairs i <= j with the
 * folded weights W(i,j) + W(j,i) -- about half the MFMAs; fields m in {22, 26}.  The packs of every level with Hp == m
 * carry the folded layout behind the plain one (the *_pack_elems sizes include it whatever the option says), and which
 * one a launch reads is decided by xp == x0.  Results: forward and dW as before up to rounding (dW exactly symmetric);
 * dX puts the WHOLE gradient of the level into dx0 and zero-fills dxp when XDFM_BWX_SET_DXP is given (leaves it alone
 * otherwise) -- with xp == x0 only the sum dxp + dx0 was ever meaningful.  Probe "last_sym": bit 0 / 1 / 2 = the last
 * f16x3 / bf16 forward / dX / dW launch ran the folded kernel.
 * "bww_xcd" (default 1): the f16x3 / bf16 dW kernel maps its workgroups so that those of one n-split, which stream the same
 * dOut planes, run on one XCD (one L2) instead of in launch order; same results, 4.7x fewer bytes fetched at config 2. */
/* read-only probes (xdfm_get_option): "last_fwd_kernel", "last_bwx_kernel", "last_bww_kernel" = arithmetic of the kernel
 * the last xdfm_cin_level_fwd / _bwd_x / _bwd_w call launched (0 f32mfma, 1 f16x3, 2 bf16; -1 before the first call):
 * a shape without a kernel in the selected mode runs mode 0, and the tests assert which one ran.
 * "last_fwd_inst", "last_bwx_inst", "last_bww_inst" = the template instance of that launch, T * 1000 + NW * 100 + NT * 10 + S:
 * T = row tiles per wave of the forward (MT 2 / 4 / 8), h-blocks per tile of dX (HBT 2 / 4 / 8 / 16), 4 for dW; NW = waves per
 * workgroup (4 / 8); NT = MFMA terms per product (3 f16x3, 1 bf16); S = 1 for the folded level-0 kernel.  0 when the call ran
 * the mode-0 kernel, -1 before the first call.  Example: 8831 = forward, MT 8, 8 waves, f16x3, folded level 0.
 * "last_fwd_f32", "last_bwx_f32", "last_bww_f32" = the same for the mode-0 (v_mfma_f32_32x32x2_f32) kernels: the template
 * instance the last xdfm_cin_level_fwd / _bwd_x(_ex) / _bwd_w call launched, 0 when it ran an f16x3 / bf16 kernel, -1 before
 * the first call; a call that returns an error before its launch leaves them alone.
 *   last_fwd_f32 = MT * 1000 + NF * 100 + MPT: MT = row tiles of 32 per wave (1 / 2 / 4 / 8, by H), NF = column fragments of 32
 *      per wave (2 with "fwd_nf" 2 at MT 4, else 1), MPT = 13 / 11 for the straight-line kernel of m = 25, 26 / 21, 22 at
 *      MT >= 4, 0 for the generic kernel.  Example: 4213 = MT 4, two fragments, m = 26.
 *   last_bwx_f32 = HS4 * 10 + JB: HS4 = float4 groups along h (1 .. 32, the power of two >= H / 8), JB = chains a wave
 *      interleaves (2 with "dbg" bit 32, an even m and 4 <= HS4 <= 16, else 1).  Example: 161.
 *   last_bww_f32 = S * 1000 + MT * 100 + KV * 10 + slab: S = n-splits launched, MT = row tiles per wave (1 / 2 / 4, by H or
 *      "bww_mt"), KV = 1 register-staged kernel ("dbg" bit 8), 2 dword LDS-DMA, 3 dwordx4 LDS-DMA (MT 4, N % 4 == 0, 16-byte
 *      aligned operands, not "dbg" bit 16), slab = 1 per-split slabs summed in order / 0 atomic epilogue ("bww_slab").
 *      Example: 32431 = 32 n-splits, MT 4, dwordx4 LDS-DMA, slabs. */
/* "adam_rows" (default 1): xdfm_adam_catchup_rows / xdfm_adam_apply_rows with D % 4 == 0 give one thread a whole table row
 * (one claim per `last` word of the row, the row's chunks in turn) instead of one thread per 16-byte chunk; 0 = by chunk,
 * which is what every other D runs.  Same bits either way; read when the call issues its launch.  Probe "last_adam_rows":
 * 1 / 0 = the last of those two calls launched the by-row / the by-chunk kernel, -1 before the first call. */
/* "colaunch" (bit mask, default 7): bodies that do not depend on each other go out as workgroup ranges of one launch.
 * Bit 0 = xdfm_colaunch_adam_step runs the step's workgroups and the rows update's in one launch
 * (adam_step_rows_kernel); clear, it issues the launches of xdfm_adam_step_deferred followed by xdfm_adam_apply_rows.
 * Bit 1 = xdfm_cin_pack_defer records the CIN weight packs for the catch-up and the gather to carry; clear, it launches them.
 * Bit 2 = xdfm_rider_begin opens a rider scope (below); clear, it opens none.  At 0 every body
 * leaves in the launch it had before the option existed.  Same bits either way; read when a call issues its launch.  Probes:
 * "last_colaunch" 1 / 0 = the last xdfm_colaunch_adam_step issued the shared launch / the two, -1 before the first call;
 * "last_riders" = slab sums the last host launch (pre-pass or scatter) took as riders, -1 before the first. */
/* "opt_bx" (default 0), the counterpart of "adam_bx" for xdfm_sgd_step / _adagrad_step / _rmsprop_step, their _deferred forms
 * and xdfm_opt_flush / xdfm_rmsprop_flush: the most workgroups one tensor gets in a launch.  0, negative values and values
 * above the built-in caps (512 in the sweep and in the deferred step's scan, 4096 in the flush) mean those caps.  Read when
 * the call composes its launch; it changes the grid only -- same arithmetic, same bits, and xdfm_opt_step_ws_elems(T) stays
 * T * 512.  A test knob: at 1 a tensor is one workgroup, whose loops then run many times at small sizes. */
int xdfm_set_option(const char* key, int value);
int xdfm_get_option(const char* key);
/* Finish batch: the one-block "finish" launches of a train step in one launch.
 * Between xdfm_finish_batch_begin() and xdfm_finish_batch_run(stream), on
 * the current device, every entry point that would launch a finish kernel of its own (the dbias of xdfm_cin_dout_det /
 * xdfm_cin_bwd_prep, the split sums of xdfm_dense_bwd_w / _drop / xdfm_dense_prelu_bwd_w with its slope, xdfm_colsum /
 * xdfm_relu_bwd_colsum, the loss of xdfm_head_fwd* and the parameter gradients of xdfm_head_bwd*, the L2 value of
 * xdfm_adam_step* and the cell of xdfm_adam_apply_rows) records a job instead; _run issues ONE launch over all recorded jobs
 * (16 to a launch: a longer list takes more launches), whose job table travels in the kernel arguments -- no copy, no memset
 * node, capturable.  Every sum keeps its order: the results are bit-identical to the separate launches.
 *   - The deferred OUTPUTS (dbias, dW / db / dalpha of a layer with more than one split, the column sums, the loss, the head's
 *     grads, l2_value) and the `cell` are undefined until _run; the partials' workspaces must stay allocated and untouched
 *     until then.  The caller must not read a deferred output before _run, on the device or on the host.
 *   - The finish of xdfm_adam_apply_rows rides behind the L2 finish that sets the same l2_value; a job that reads what an
 *     earlier job of the batch writes, and cannot ride behind it, first sends the recorded jobs off in a launch of their own.
 *   - Inside a batch the CIN dbias is STORED (0 + sum), not accumulated: it need not be zeroed (xdfm_finish_batch_active
 *     tells a caller whether that holds for the next call).
 *   - Errors (XDFM_ERR_INVALID): _begin while a batch is open; a job or _run on another stream than the batch's first job; a
 *     job, _begin or _run on another device than the open batch's.  _run without an open batch, or with no recorded job,
 *     launches nothing and returns XDFM_OK.  A failed _run leaves the batch open.  One batch at a time per process.
 *   - Option "finish_batch" (default 1): 0 = _begin opens nothing, every finish stays its own launch (A/B runs).
 * xdfm_finish_batch_active: 1 when jobs are being recorded on the current device (a batch is open), else 0.
 * xdfm_finish: ONE finish over partials the caller supplies -- exactly what the entry points above call after their main
 * kernel: recorded in the open batch, else launched.  For tests and tools.  kind / arguments (others 0 / NULL):
 *   0 CIN dbias    part [i0 = H][i1 = partials per row] -> out [H] (+= outside a batch)
 *   1 dense dW     part = ws (xdfm_dense_bwd_w's layout: i0 = nsplit slabs [n0 = out][n1 = in], then nsplit x [out] for db),
 *                  out = dW, out2 = db or NULL; PReLU: part2 = i1 double partials, out3 = dalpha or NULL.  One split and no
 *                  dalpha: nothing to do (the main kernel's dW, db are final)
 *   2 column sums  part [64][i0 = cols] -> out [cols]
 *   3 head loss    part [128] -> out [1]
 *   4 head grads   part [128][i0 = KT] -> out [KT]
 *   5 Adam L2      part [i0 = n] -> out [1]
 *   6 rows cell    out2 = cell (8-byte aligned): out[0] += cell / 2^40 (out may be NULL), cell = 0
 *   7 add          out[0] = part[0] + part2[0] (fp32): the step's total loss; rides behind the job that writes part2 */
int xdfm_finish_batch_begin(void);
int xdfm_finish_batch_run(void* stream);
int xdfm_finish_batch_active(void);
int xdfm_finish(int kind, const void* part, const void* part2, void* out, void* out2, void* out3, long n0, long n1, int i0, int i1,
                void* stream);
/* Riders: a small body that depends on nothing near it leaves inside the next suitable launch instead of alone.
 * Between xdfm_rider_begin() and xdfm_rider_flush(stream), xdfm_cin_level_bwd_w / _prepared on the f16x3 / bf16 path do not
 * launch the ordered sum of their n-split slabs into dW but record it (up to 4; a fifth is launched as before).  A host
 * launch on the same stream takes the recorded sums as extra workgroups of its own grid (a job table in the kernel
 * arguments: no copy, capturable).  Hosts: xdfm_cin_bwd_prep where it takes the f16x3 / bf16 pre-pass, and
 * xdfm_embed_scatter_bwd / _marked (at most 512 rider workgroups: what fits beside the scatter; a longer table stays
 * recorded).  xdfm_rider_flush issues whatever nobody carried as ONE launch and closes the scope.  One thread per element,
 * the splits in their fixed order: dW is bit-identical.
 *   - dW of a recorded level and the workspace `ws` that holds its slabs are undefined / must stay allocated and untouched
 *     until the carrying launch or xdfm_rider_flush has been issued on the stream.
 *   - xdfm_rider_begin with a scope open is XDFM_ERR_INVALID; xdfm_rider_flush on another stream than the recorded jobs'
 *     drops them and returns XDFM_ERR_INVALID; without an open scope or without jobs it launches nothing.
 *   - ONE scope per process, and its state is not locked (the finish batch has the same rule): the calls between _begin
 *     and _flush must come from one backward pass at a time.  Two passes that overlap -- on two devices' autograd threads,
 *     or a backward nested in another -- would find the scope open already (XDFM_ERR_INVALID from the second _begin) or
 *     mix their jobs; the model's own train step opens one scope around its one backward.
 *   - Option "colaunch" bit 2 clear: _begin opens nothing and every sum is launched by its own call, as without a scope.
 * xdfm_rider_pending: the number of recorded sums that no launch has taken yet.  xdfm_rider_active: 1 while a scope is open
 * and records, else 0. */
int xdfm_rider_begin(void);
int xdfm_rider_flush(void* stream);
int xdfm_rider_pending(void);
int xdfm_rider_active(void);
/* [host] node types of a captured hipGraph_t (the host side replays the train step from a HIP graph):
 * memset nodes are counted separately because they are not ordered reliably against neighbouring kernel
 * nodes on ROCm 7.2 / gfx950 (tools/graph_memset_probe.py) -- a graph with n_memset > 0 must not be replayed;
 * n_unexpected counts nodes that are neither kernel, memcpy, empty nor event nodes. */
int xdfm_graph_node_census(void* graph, int* n_nodes, int* n_memset, int* n_unexpected);

/* ------------------------------------------------------------------ embedding gather (K1)
 * replaces: deepctr/models/basemodel.py:368-370 (26x slice -> .long() -> nn.Embedding),
 *           deepctr/models/basemodel.py:63-92 (Linear: 1-dim tables, sum, dense @ weight),
 *           deepctr/models/xdeepfm.py:86 + deepctr/inputs.py:126-132 (the two concatenations).
 * X        [B][ldx] fp32; ids travel as fp32 exactly as basemodel.py:242 makes them.
 * tables   device array of m table base pointers, table j is [vocab[j]][D];
 * lin_tables device array of m pointers to [vocab[j]][1] tables, or NULL (no linear part);
 * cols     device int[m]: column of X that holds field j's id;   vocab: device int[m];
 * dense_cols device int[nd] (may be NULL when nd == 0); dense_w [nd] (linear_model.weight);
 * emb_fm   out, FM layout [m][B*D]   (the CIN input, reference layout [B,m,D]);
 * dnn_in   out [B][m*D + nd] or NULL (combined_dnn_input);
 * lin_out  out [B] or NULL           (linear_logit);
 * err_flag device int[1] or NULL: bit 0 is OR-ed in when an id is outside [0, vocab) (the id is
 *          then clamped; the reference raises IndexError / device-asserts).
 */
int xdfm_embed_gather_fwd(const float* X, long ldx, int B,
                          const float* const* tables, const float* const* lin_tables,
                          const int* cols, const int* vocab, int m, int D,
                          const int* dense_cols, const float* dense_w, int nd,
                          float* emb_fm, float* dnn_in, float* lin_out,
                          int* err_flag, void* stream);

/* Same, with the layout of dnn_in given by the caller: rows of ld_dnn floats, the m*D embedding columns first, the nd dense
 * columns from column dense_off on (dense_off >= m*D, ld_dnn >= dense_off + nd).  The columns in between are left alone:
 * xdfm_varlen_pool_fwd fills them with the pooled variable-length fields, and emb_fm may then have more than m field
 * slots.  ld_dnn = m*D + nd, dense_off = m*D is xdfm_embed_gather_fwd. */
int xdfm_embed_gather_fwd_ld(const float* X, long ldx, int B,
                             const float* const* tables, const float* const* lin_tables,
                             const int* cols, const int* vocab, int m, int D,
                             const int* dense_cols, const float* dense_w, int nd,
                             float* emb_fm, float* dnn_in, long ld_dnn, int dense_off, float* lin_out,
                             int* err_flag, void* stream);

/* ------------------------------------------------------------------ pooled variable-length fields (K1v / K2v, csrc/varlen.hip)
 * replaces: varlen_embedding_lookup + get_varlen_pooling_list (deepctr/inputs.py:141-155, :213-227) with
 *           SequencePoolingLayer (deepctr/layers/sequence.py:49-77) for every VarLenSparseFeat, in input_from_feature_columns
 *           (deepctr/models/basemodel.py:372-377) and in Linear.forward (:72-77), and their autograd.
 * Field f reads maxlen ids from the columns col .. col + maxlen - 1 of X (fp32, truncated as Tensor.long()).  Position t is
 * valid when id != 0 (len_col < 0) or when t < long(X[b][len_col]).  With w_t the table row of position t:
 *   XDFM_POOL_SUM   sum of the valid w_t;
 *   XDFM_POOL_MEAN  that sum / (float(count of valid positions, or the length column's value) + 1e-8f);
 *   XDFM_POOL_MAX   max over ALL t of (valid ? w_t : w_t - 1e9f) -- an empty sequence pools to the reference's value, not to 0.
 * The [B, maxlen, D] rows exist in registers only.  Every position is looked up, padded ones too, as the reference does: an id
 * outside [0, vocab) is clamped and raises err_flag (as K1).  1 <= maxlen <= 255. */
enum { XDFM_POOL_SUM = 0, XDFM_POOL_MEAN = 1, XDFM_POOL_MAX = 2 };
typedef struct {
    const float* table;   /* [vocab][D]; may be NULL in a call without emb_fm and dnn_in */
    const float* lin;     /* [vocab][1]; may be NULL in a call without lin_out */
    int col;              /* first id column of X */
    int maxlen;
    int len_col;          /* column of X that holds the length, or -1: mask = id != 0 */
    int combiner;         /* XDFM_POOL_* */
    int vocab;
    int reserved;
} xdfm_varlen_field;
/* ONE launch for all F fields.  fields: device array; fields_host: the same F descriptors in host memory (shapes are
 * checked against ldx before anything is launched; the pointers in it are not dereferenced).
 * emb_fm  FM layout [>= slot0 + F][B*D] or NULL: field f is written to slot slot0 + f (the sparse fields of K1 come first);
 * dnn_in  [B][ld_dnn] or NULL: field f is written to columns dnn_off + f*D .. of every row;
 * lin_out [B] or NULL: the pooled [vocab][1] rows of all fields are ADDED to it (K1 has written it before);
 * argpos  [B][F][D + 1] bytes or NULL: position of the first maximum per (example, field, column), column D being the linear
 *         table's -- what xdfm_varlen_pool_bwd needs for XDFM_POOL_MAX fields (0 for the other combiners). */
int xdfm_varlen_pool_fwd(const float* X, long ldx, int B, const xdfm_varlen_field* fields,
                         const xdfm_varlen_field* fields_host, int F, int D, int slot0,
                         float* emb_fm, float* dnn_in, long ld_dnn, int dnn_off, float* lin_out,
                         unsigned char* argpos, int* err_flag, void* stream);
/* Backward: dense [vocab][D] and [vocab][1] gradients, no float atomics, bit-identical from run to run.  An expand kernel
 * writes one row gradient per position for B * Tmax pseudo-examples (Tmax = largest maxlen; g for sum, g / (len + 1e-8f) for
 * mean, both at the valid positions only; for max g at the recorded position whether or not it is valid -- an all-masked sequence
 * sends its gradient to the row its first maximum looked up, row 0 under the id != 0 mask, as autograd of the reference's
 * torch.max over w - (1 - mask) * 1e9 does; zeros everywhere else), then K2's exact segmented reduce
 * (xdfm_embed_scatter_bwd_marked) adds them to d_flat in chunks of 4096 pseudo-examples, in ascending order.
 * d_emb_fm / d_dnn_in / d_lin: the gradients of the three outputs of the forward (same layouts; each may be NULL; ld_lin = row
 * stride of d_lin, 0 = 1); the pooled row's gradient is d_emb_fm + d_dnn_in (one fp32 add).
 * d_flat: caller-initialised (zeros) gradient buffer, 16-byte aligned; table f's gradient starts at d_flat + tab_off[f], its
 * linear table's at d_flat + lin_off[f] (device long[F]; either array may be NULL: those gradients are not computed).
 * cols: device int[F] = 0 .. F-1;  vocab: device int[F];  ws: xdfm_varlen_pool_bwd_ws_elems floats. */
size_t xdfm_varlen_pool_bwd_ws_elems(long B, int F, int D, int Tmax);
int xdfm_varlen_pool_bwd(const float* X, long ldx, int B, const xdfm_varlen_field* fields,
                         const xdfm_varlen_field* fields_host, int F, int D, int slot0,
                         const float* d_emb_fm, const float* d_dnn_in, long ld_dnn, int dnn_off,
                         const float* d_lin, long ld_lin, const unsigned char* argpos,
                         const int* cols, const int* vocab, float* d_flat, const long* tab_off, const long* lin_off,
                         float* ws, void* stream);
/* The same backward over EXCHANGED rows (row-parallel training: every rank scatters all ranks' rows, and has run the forward
 * for its own only).  X [R][ldx]: the gathered rows, rank-major, zero pad rows of ragged ranks included.  g_rows [R][ld_g]:
 * per-example row gradients in the DNN input's layout, field slot0 + f of row r at g_rows[r * ld_g + (slot0 + f) * D], the two
 * uses of the pooled row already summed (ld_g >= (slot0 + F) * D).  d_lin [R] with row stride ld_lin (0 = 1).  No argpos: for
 * XDFM_POOL_MAX fields the position of the first maximum is recomputed from the tables in `fields` by the forward's own walk
 * (same validity, masked positions as w - 1e9f, ties to the lowest position) -- call it BEFORE the tables are updated.  Then
 * xdfm_varlen_pool_bwd's expand and reduce run over the R rows: same d_flat / tab_off / lin_off / cols / vocab, same bits as
 * that call on the same rows in the same order; an all-zero row with zero gradients adds nothing (a max field adds its
 * gradient, an exact zero, to row 0).  An id outside [0, vocab), at any position,
 * raises err_flag (device int[1] or NULL) and is clamped.  ws: xdfm_varlen_pool_bwd_rows_ws_elems floats, 16-byte aligned. */
size_t xdfm_varlen_pool_bwd_rows_ws_elems(long R, int F, int D, int Tmax);
int xdfm_varlen_pool_bwd_rows(const float* X, long ldx, int R, const xdfm_varlen_field* fields,
                              const xdfm_varlen_field* fields_host, int F, int D, int slot0,
                              const float* g_rows, long ld_g, const float* d_lin, long ld_lin,
                              const int* cols, const int* vocab, float* d_flat, const long* tab_off, const long* lin_off,
                              float* ws, int* err_flag, void* stream);

/* ------------------------------------------------------------------ embedding scatter (K2)
 * replaces: autograd of the above (aten::embedding_dense_backward x52, sparse=False,
 *           deepctr/inputs.py:168) and d(linear_model.weight).
 * d_emb_fm [m][B*D] or NULL, d_dnn_in [B][m*D+nd] or NULL, d_lin [B] or NULL are the incoming
 * gradients.  The dense gradient tables live in ONE caller-initialised buffer d_flat (zeros, or the
 * L2 gradient written by xdfm_l2_reg_bwd): table j starts at d_flat + tab_off[j], its linear table
 * at d_flat + lin_off[j] (device long[m], element offsets; either may be NULL); d_dense_w [nd] is added to as well.
 * No atomics on the gradients: per field the examples of a chunk of <= 4096 are grouped by id through a hash table in LDS
 * (equal ids end up adjacent, the groups in no particular order; embed_scatter_grouped_kernel), runs of equal ids
 * are summed EXACTLY (addends rounded once to a fixed-point grid 2^-13 ulp below the run's largest magnitude, added
 * as integers in doubles, rounded once to fp32) and added to d_flat by one lane per row.  The result is a function
 * of the multiset of rows: bit-identical from run to run, under any permutation of the examples of a chunk and on
 * every rank of a row-parallel run (the reference's CPU scatter, deepctr/inputs.py:168, is deterministic too; it adds
 * in example order in fp32, i.e. within a few ulp of this).  Chunks (B > 4096) are launched in ascending order.
 */
int xdfm_embed_scatter_bwd(const float* X, long ldx, int B,
                           const int* cols, const int* vocab, int m, int D,
                           const int* dense_cols, int nd,
                           const float* d_emb_fm, const float* d_dnn_in, const float* d_lin,
                           float* d_flat, const long* tab_off, const long* lin_off, float* d_dense_w,
                           void* stream);
/* Same, and marks[e >> 2] = 1 for every element offset e of d_flat (16-byte aligned) that received a gradient
 * -- one byte per 16-byte chunk; d_dense_w must then point into d_flat too.  A caller that keeps d_flat across
 * steps hands the marks to K7 (xdfm_adam_tensor.grad_marks), which reads and re-zeroes only the marked chunks:
 * the table-sized zero fill of the gradients (optim.zero_grad over dense [V, D] gradients) and
 * the table-sized gradient read of the optimizer step both shrink to the rows the batch touched.
 * marks may be NULL.  ld_dnn / ld_lin: row strides (floats) of d_dnn_in and d_lin, 0 = dense (m*D + nd and 1):
 * the row-parallel exchange hands over ONE gathered buffer whose rows hold [row gradients | X row | d_lin]. */
int xdfm_embed_scatter_bwd_marked(const float* X, long ldx, int B,
                                  const int* cols, const int* vocab, int m, int D,
                                  const int* dense_cols, int nd,
                                  const float* d_emb_fm, const float* d_dnn_in, long ld_dnn,
                                  const float* d_lin, long ld_lin,
                                  float* d_flat, const long* tab_off, const long* lin_off, float* d_dense_w,
                                  unsigned char* marks, void* stream);

/* ------------------------------------------------------------------ CIN level (K3 / K4)
 * One level of deepctr/layers/interaction.py:216-243 (same loop in
 * deepctr/layers/cin_attention.py:257-289, :417-446):
 *     Z[b,(i,j),d] = x_prev[b,i,d] * x0[b,j,d]                 (einsum, :218-222, k = i*m + j)
 *     out[b,h,d]   = act( sum_k W[h,k] * Z[b,k,d] + bias[h] )   (nn.Conv1d k=1 :224, act :226-229)
 * Z is never materialised: it is formed in registers as the B operand of the MFMA contraction.
 * W is conv1ds[i].weight [H][Hp*m] (the trailing 1 of Conv1d dropped), xp is [Hp][N], x0 [m][N],
 * out [H][N], all FM layout, N = B*D.
 */
size_t xdfm_cin_fwd_pack_elems(int H, int Hp, int m);                 /* floats in Wf */
int xdfm_cin_fwd_pack(const float* W, int H, int Hp, int m, float* Wf, void* stream);
int xdfm_cin_level_fwd(const float* xp, const float* x0, const float* Wf, const float* bias,
                       int H, int Hp, int m, long N, int act, float* out, void* stream);

/* The forward of a level with what the CIN does with its output fused into the kernel's epilogue (f16x3 / bf16 arithmetic,
 * D in {4, 8, 16, 32}: xdfm_cin_level_fwd_ex_supported): rows [0, keep_rows) are stored to out [keep_rows][N]; rows >= dir0 are
 * summed over the embedding axis into res (res[b * ldres + res_off + row - dir0], interaction.py:245-246: the
 * direct-connect half of a level in sum pooling is never written out), res == NULL: no sums; mask != NULL: bit n & 31 of
 * mask[(n >> 5) * mask_ld + row] = out[row][n] > 0 for every row (mask_ld >= H, a multiple of 4; mask 16-byte aligned: all
 * the backward needs of a ReLU level's output).
 * At BASELINE config 2 this removes 84 MB of stores, the three xdfm_cin_direct_sum launches and their 84 MB of reads, and
 * (with the mask given to xdfm_cin_bwd_prep) 134 MB of reads in the backward, per step. */
int xdfm_cin_level_fwd_ex_supported(int H, int Hp, int m, int D);
int xdfm_cin_level_fwd_ex(const float* xp, const float* x0, const float* Wf, const float* bias, int H, int Hp, int m, long N,
                          int act, float* out, int keep_rows, float* res, long ldres, int res_off, int dir0, int D,
                          unsigned* mask, long mask_ld, void* stream);

/* sum over the embedding axis of `rows` feature maps (interaction.py:245-246):
 * res[b*ldres + off + r] = sum_d A[(row0 + r)][b*D + d] */
int xdfm_cin_direct_sum(const float* A, int row0, int rows, int B, int D,
                        float* res, long ldres, int off, void* stream);

/* dOut = act'(A) * (dHid + dDirect), dbias[h] += sum_n dOut[h][n]   (autograd of :224-243).
 * A [H][N] is the saved post-activation output of the level.  Rows [hid0, hid0+hid_rows) take
 * dHid [hid_rows][N] (gradient w.r.t. next level's x_prev); rows [dir0, dir0+dir_rows) take the
 * direct-connect gradient: dir_mode 0: dDir is d(result) [B][lddir], value dDir[b*lddir+dir_off+r]
 * broadcast over d (sum pooling); dir_mode 1: dDir is FM layout [.][N], row dir_off + r
 * (attention pooling).  Either part may be absent (rows == 0 / NULL).  dbias must be zeroed by the
 * caller. */
int xdfm_cin_dout(const float* A, int H, int B, int D, int act,
                  const float* dHid, int hid0, int hid_rows,
                  const float* dDir, int dir_mode, long lddir, int dir_off, int dir0, int dir_rows,
                  float* dOut, float* dbias, void* stream);
/* Same with a workspace of xdfm_cin_dout_ws_elems(H, B, D) floats: the per-block sums of dbias are stored and added up
 * in a fixed order (a second tiny launch) instead of by one float atomic per block -- the same bits on every run. */
size_t xdfm_cin_dout_ws_elems(int H, int B, int D);
int xdfm_cin_dout_det(const float* A, int H, int B, int D, int act,
                  const float* dHid, int hid0, int hid_rows,
                  const float* dDir, int dir_mode, long lddir, int dir_off, int dir0, int dir_rows,
                  float* dOut, float* dbias, float* ws, void* stream);

/* dx_prev[i][n] += sum_j dZ[(i,j)][n] * x0[j][n];  dx0[j][n] += sum_i dZ[(i,j)][n] * x_prev[i][n]
 * with dZ = W^T dOut recomputed tile by tile.  dxp [Hp][N] and dx0 [m][N] are ACCUMULATED into
 * (caller zero-initialises); dxp and dx0 must NOT alias (for level 0, where x_prev is x0, pass a
 * scratch dxp and add it to dx0 afterwards: how the level's gradient is divided between the two is then up to the
 * kernel -- see option "x3_sym").  H <= 256 rows of the contraction per call. */
size_t xdfm_cin_bwd_pack_elems(int H, int Hp, int m);
int xdfm_cin_bwd_pack(const float* W, int H, int Hp, int m, float* Wz, void* stream);
int xdfm_cin_level_bwd_x(const float* dOut, const float* xp, const float* x0, const float* Wz,
                         int H, int Hp, int m, long N, float* dxp, float* dx0, void* stream);
/* same with flags: XDFM_BWX_SET_DXP / XDFM_BWX_SET_DX0 = store the result instead of adding it to dxp / dx0
 * (the buffer then needs no zero-fill and is not read). */
enum { XDFM_BWX_SET_DXP = 1, XDFM_BWX_SET_DX0 = 2 };
int xdfm_cin_level_bwd_x_ex(const float* dOut, const float* xp, const float* x0, const float* Wz, int H, int Hp,
                            int m, long N, float* dxp, float* dx0, int flags, void* stream);

/* 1 when xdfm_cin_level_bwd_x_ex called with these shapes and xp == x0 (xp_is_x0 != 0), dxp != dx0, under the current
 * "cin_math" / "x3_sym" options runs the folded level-0 kernel, i.e. leaves the level's WHOLE gradient in dx0 (dxp zero);
 * 0 when the caller still has to add dxp to dx0.  A pure function of its arguments and the two options: the host asks
 * it instead of reading the process-global "last_sym" probe, which another thread's launch could have rewritten. */
int xdfm_cin_bwd_x_is_folded(int H, int Hp, int m, int xp_is_x0);

/* dW[h][i*m+j] = sum_n dOut[h][n] * x_prev[i][n] * x0[j][n]   (overwrites dW [H][Hp*m]).
 * ws: workspace of xdfm_cin_bwd_w_ws_elems floats (one partial copy of dW per n-split, summed in a
 * fixed order: bitwise reproducible). */
size_t xdfm_cin_bwd_w_ws_elems(int H, int Hp, int m, long N);
int xdfm_cin_level_bwd_w(const float* dOut, const float* xp, const float* x0,
                         int H, int Hp, int m, long N, float* ws, float* dW, void* stream);

/* The level's backward up to its MFMA kernels in ONE pass over dOut (f16x3 / bf16 arithmetic): xdfm_cin_dout_det that
 * also leaves, in the dW workspace `bww_ws` (xdfm_cin_bwd_w_ws_elems floats), what xdfm_cin_level_bwd_w would otherwise
 * produce with two more passes over dOut -- its fp16 hi / lo planes and the row scales of dOut, x_prev and x0.  The
 * scales are per n-split of the dW kernel (a split's workgroups contract over the split's columns only), each block
 * finds them for its own columns, and the dW kernel removes them from its accumulators before it stores the split's
 * slab.  *prepared [host] = 1 when that happened: the caller then calls xdfm_cin_level_bwd_w_prepared with the same xp,
 * x0, shapes, workspace and options; 0 when the shape has no f16x3 / bf16 dW kernel (H <= 64, D % 4 != 0, unaligned
 * rows, cin_math 0): the call then was xdfm_cin_dout_det and xdfm_cin_level_bwd_w does its own passes.
 * dout_ws: xdfm_cin_bwd_prep_ws_elems floats (dbias partials, added up in a fixed order).  dbias is added to.
 * mask != NULL: the ReLU mask comes from the sign bits xdfm_cin_level_fwd_ex left (bit n & 31 of mask[(n >> 5) * mask_ld + h]
 * = out[h][n] > 0) and A is not read (may be NULL): the level's output then need not be kept at all beyond its hidden
 * rows, which travel as xp. */
size_t xdfm_cin_bwd_prep_ws_elems(int H, int Hp, int m, int B, int D);
/* dOut == NULL in xdfm_cin_bwd_prep (allowed when xdfm_cin_bwd_nodout_supported and a mask is given): the fp32 dOut is not
 * written at all -- the dW kernel takes the planes, and the dX kernel forms its dOut operand itself, from the very
 * sources of this pass (xdfm_cin_level_bwd_x_src: sign bits, dHid, pooled gradient).  67 MB less written and 67 MB less
 * read at level 0 of config 2.  xdfm_cin_level_bwd_x_src: one call covers rows [h0, h0 + H) of the level, H <= 256. */
int xdfm_cin_bwd_nodout_supported(int H, int Hp, int m, int B, int D);
int xdfm_cin_level_bwd_x_src(const unsigned* mask, long mask_ld, const float* dHid, int hid_rows, const float* dDir, int dir_mode,
                             long lddir, int dir_off, int dir0, int dir_rows, int D, int h0, const float* xp, const float* x0,
                             const float* Wz, int H, int Hp, int m, long N, float* dxp, float* dx0, int flags, void* stream);
int xdfm_cin_bwd_prep(const float* A, const unsigned* mask, long mask_ld, int H, int B, int D, int act, const float* dHid,
                      int hid0, int hid_rows, const float* dDir, int dir_mode, long lddir, int dir_off, int dir0, int dir_rows,
                      float* dOut, float* dbias, float* dout_ws, const float* xp, const float* x0, int Hp, int m, float* bww_ws,
                      int* prepared, void* stream);
int xdfm_cin_level_bwd_w_prepared(const float* dOut, const float* xp, const float* x0, int H, int Hp, int m, long N,
                                  float* ws, float* dW, void* stream);

/* ------------------------------------------------------------------ attention pooling (K5)
 * replaces: deepctr/layers/cin_attention.py:63-97 (MultiHeadSelfAttention), :130-144
 *           (AttentionPooling) and the tails of CINAttention.forward :302-313 /
 *           CINAttentionV2.forward :452-464: n_layers x (MHSA -> +residual -> LayerNorm) then
 *           softmax_s(w2 . tanh(W1 x_s + b1)) weighted sum.  The [B,heads,S,S] score tensor of the
 *           reference never exists; one workgroup handles one example with its S tokens on chip.
 * fm     FM layout [S][B*D]: the concatenated direct-connect feature maps (tokens x_s = fm[s][b*D..]).
 * theta  packed parameters: per layer Wq Wk Wv Wo ([D][D], nn.Linear weight layout), then gamma, beta
 *        ([D] each, only if use_ln); then W1 [D][D], b1 [D], w2 [D]  (xdfm_cin_attn_theta_elems floats).
 * nh     number of heads (must divide D; pairs (D, nh) are compiled for D in {4,8,10,16,32}).
 * out    [B][D] pooled vector.  (CINAttention's output_proj D -> featuremap_num is a plain GEMM.)
 * tok_save, o_save [n_layers][B][S][D] (each layer's output tokens / attention output before W_o),
 * ml_save [n_layers][B][S][nh][2] (base-2 log-sum-exp of the scaled scores, 1/sum): written by fwd, read by bwd.
 * bwd: dout [B][D]; dfm [S][B*D] is overwritten; dtheta (same layout as theta) is ACCUMULATED into with
 * fp32 atomics and must be zeroed by the caller.  S <= 1024.
 * p_drop, drop_seed: attention dropout (cin_attention.py:86, nn.Dropout on the softmax output, training mode
 * only).  p_drop = 0 (drop_seed may be NULL) is the reference's default and the evaluation path.  With
 * 0 < p_drop < 1 every attention weight is kept with probability 1-p_drop and scaled by 1/(1-p_drop); the keep
 * bit is a hash of (*drop_seed, example, layer, head, query, key) -- drop_seed is a DEVICE 64-bit scalar so a
 * captured graph draws a new mask per replay -- and nothing is stored: bwd must be given the same p_drop and
 * seed value as the fwd whose buffers it reads.  The stream of bits is not torch's Philox stream; like the
 * reference's CPU and CUDA generators, two back ends agree in distribution, not bit for bit.
 */
size_t xdfm_cin_attn_theta_elems(int D, int n_layers, int use_ln);
int xdfm_cin_attn_pool_fwd(const float* fm, int B, int S, int D, int nh, int n_layers, int use_ln, int use_res,
                           const float* theta, float* out, float* tok_save, float* o_save, float* ml_save,
                           float p_drop, const unsigned long long* drop_seed, void* stream);
int xdfm_cin_attn_pool_bwd(const float* fm, int B, int S, int D, int nh, int n_layers, int use_ln, int use_res,
                           const float* theta, const float* tok_save, const float* o_save, const float* ml_save,
                           const float* dout, float* dfm, float* dtheta, float p_drop,
                           const unsigned long long* drop_seed, void* stream);
/* Same without float atomics: every workgroup stores its share of the parameter gradients in `ws`
 * (xdfm_cin_attn_pool_bwd_ws_elems floats) and a second small launch adds the shares in workgroup order -- dtheta is
 * OVERWRITTEN (no zero-fill) and has the same bits on every run. */
size_t xdfm_cin_attn_pool_bwd_ws_elems(int B, int D, int n_layers, int use_ln);
int xdfm_cin_attn_pool_bwd_det(const float* fm, int B, int S, int D, int nh, int n_layers, int use_ln, int use_res,
                               const float* theta, const float* tok_save, const float* o_save, const float* ml_save,
                               const float* dout, float* dfm, float* dtheta, float* ws, float p_drop,
                               const unsigned long long* drop_seed, void* stream);
/* keep[n_layers][B][nh][S(query)][S(key)] (1 = kept): the mask the two calls above generate for this seed.
 * Test hook: lets a CPU oracle apply the same mask where the reference applies nn.Dropout. */
int xdfm_cin_attn_dropout_mask(int B, int S, int nh, int n_layers, float p_drop, const unsigned long long* drop_seed,
                               unsigned char* keep, void* stream);

/* ------------------------------------------------------------------ L2 regulariser (K6)
 * replaces: deepctr/models/basemodel.py:412-428 (per-tensor square / mul / sum / add loop over
 *           ~58 tensors, every embedding table in full) and its autograd.
 * ptrs: device array of T tensor base pointers, numel: device long[T], coeff: device float[T]
 * (the l2 strength of each tensor).  fwd: out[0] = sum_t coeff[t] * sum(w_t^2), deterministic;
 * partials: scratch of 32*T floats.  bwd: g_t = 2*coeff[t]*gscale[0]*w_t written (accumulate=0) or
 * added (accumulate=1) at gflat + goff[t] (device long[T], element offsets); gscale is a device
 * scalar.
 */
int xdfm_l2_reg_fwd(const float* const* ptrs, const long* numel, const float* coeff, int T,
                    float* partials, float* out, void* stream);
int xdfm_l2_reg_bwd(const float* const* ptrs, const long* numel, const float* coeff, int T,
                    const float* gscale, float* gflat, const long* goff, int accumulate, void* stream);

/* ------------------------------------------------------------------ all weight packs of a step
 * The packs depend on the weights only: with the f16x3 arithmetic one call prepares the forward pack and
 * the dX pack of every level in two launches (max|W| of all levels, then all packs) instead of two per pack.
 * jobs: HOST array; fwd_pack / bwd_pack sized by xdfm_cin_fwd_pack_elems / xdfm_cin_bwd_pack_elems (either may
 * be NULL); every level must satisfy xdfm_cin_pack_all_supported (f16x3 kernels both ways, H <= 256). */
typedef struct {
    const float* W;
    int H, Hp, m;
    float* fwd_pack;
    float* bwd_pack;
} xdfm_cin_pack_job;
int xdfm_cin_pack_all_supported(int H, int Hp, int m);
int xdfm_cin_pack_all(const xdfm_cin_pack_job* jobs, int L, void* stream);
/* xdfm_cin_pack_all whose launches may leave as riders (option "colaunch" bit 1; clear: exactly xdfm_cin_pack_all).  The packs
 * depend on the weights only, so a train step can announce them before its embedding gather: the call records the jobs, and
 *   - the next xdfm_adam_catchup_rows on `stream` carries the partial |W| maxima as extra workgroups of its launch (one
 *     256-thread workgroup per level and part: the same slots, and a maximum does not depend on the order);
 *   - the next xdfm_embed_gather_fwd / _ld on `stream` carries the packs (if no catch-up ran, the maxima leave in a launch
 *     of their own in front of it);
 *   - xdfm_cin_pack_flush(stream) issues what no launch carried, as xdfm_cin_pack_all's own launches; a second _defer
 *     flushes an earlier one first.  The packs are defined once the gather or the flush has been issued on the stream: call
 *     the flush before the first xdfm_cin_level_fwd that reads them.  Byte-identical packs and headers on every route.
 * The job arrays' buffers must stay allocated until then.  One set of deferred packs per process, not locked (as the
 * rider scope below).  xdfm_cin_pack_pending: 0 = nothing deferred, 1 = maxima and packs, 2 = packs.  Probe
 * "last_pack_riders" (reset by _defer): bit 0 = a catch-up carried the maxima, bit 1 = a gather carried the packs. */
int xdfm_cin_pack_defer(const xdfm_cin_pack_job* jobs, int L, void* stream);
int xdfm_cin_pack_flush(void* stream);
int xdfm_cin_pack_pending(void);

/* ------------------------------------------------------------------ dense-layer bias gradient
 * replaces: autograd of deepctr/layers/core.py:120-134 w.r.t. the bias, grad_bias[c] = sum_r g[r][c].
 * Atomics-free and without any memset (safe inside a captured HIP graph), fixed summation order.
 * g [rows][ld] fp32 (ld >= cols); ws: xdfm_colsum_ws_elems(cols) floats; out [cols]. */
size_t xdfm_colsum_ws_elems(int cols);
int xdfm_colsum(const float* g, long rows, int cols, long ld, float* ws, float* out, void* stream);
/* Backward of y = relu(x W^T + b) up to the GEMMs (deepctr/layers/core.py:120-134 with nn.ReLU, autograd's
 * threshold_backward + the bias gradient): gz [rows][cols] = (y > 0) ? g : 0 and out [cols] = column sums of gz,
 * fixed order; ws as for xdfm_colsum. */
int xdfm_relu_bwd_colsum(const float* g, const float* y, long rows, int cols, long ldg, long ldy, float* ws, float* gz,
                         float* out, void* stream);

/* ------------------------------------------------------------------ dense layer on fp32 MFMA (csrc/dnn.hip)
 * replaces: one layer of deepctr/layers/core.py:120-134 with its autograd -- y = act(x W^T + b), dx = gz W,
 * dW = gz^T x, db = column sums of gz, where gz = (y > 0) ? g : 0 for a ReLU layer (y = the layer's output) and g itself
 * with y = NULL.  gz is formed while the operands are loaded and never stored.  fp32 operands and accumulators
 * (v_mfma_f32_32x32x2_f32); every global access is a dword, so rows need no alignment beyond 4 bytes.
 * x [rows][ldx >= in], W [out][in] contiguous, b [out] or NULL, y / g [rows][ld >= out], dx [rows][lddx >= in],
 * dW [out][in], db [out] or NULL (no bias gradient wanted).
 * xdfm_dense_supported: rows >= 1, in in [1, 2^20], out a multiple of 32 in [32, 2^20]; the other entry points
 * return XDFM_ERR_INVALID outside it.  act: XDFM_ACT_LINEAR or XDFM_ACT_RELU.
 * xdfm_dense_bwd_w splits the contraction over the rows (256 rows a split, at most 32 splits), leaves one slab and
 * one bias partial per split in ws (xdfm_dense_bwd_w_ws_elems floats; nothing in it needs initialising) and adds
 * them over a fixed pairwise tree in a second launch: no atomics, the same bits on every run.  No entry point synchronises,
 * allocates or issues a memset. */
int xdfm_dense_supported(long rows, int in, int out);
size_t xdfm_dense_bwd_w_ws_elems(long rows, int in, int out);          /* 0 outside xdfm_dense_supported */
int xdfm_dense_fwd(const float* x, long rows, int in, long ldx, const float* W, int out, const float* b, int act, float* y,
                   long ldy, void* stream);
int xdfm_dense_bwd_x(const float* g, long ldg, const float* y, long ldy, long rows, int out, const float* W, int in, float* dx,
                     long lddx, void* stream);
int xdfm_dense_bwd_w(const float* g, long ldg, const float* y, long ldy, const float* x, long ldx, long rows, int in, int out,
                     float* ws, float* dW, float* db, void* stream);
/* The same layer followed by dropout (deepctr/layers/core.py:134, nn.Dropout after the activation), in the same launches.
 * Forward: y = keep ? relu(x W^T + b) * s : 0 with the fp32 s = 1.0f / (1.0f - p_drop), one rounding.  The keep bit of cell
 * (layer, row, col) is a counter-based hash -- nothing is stored, and the draw matches nn.Dropout in distribution only (it
 * is not torch's Philox stream), as the attention's does:
 *     mix(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16          (32-bit, wrapping)
 *     k    = mix((uint32)seed ^ ((uint32)layer * 0x9E3779B1))
 *     rk   = mix(k + (uint32)(seed >> 32) + (uint32)(row0 + row) * 0x85EBCA77)
 *     keep = mix(rk + (uint32)col * 0x9E3779B1) >= thresh,     thresh = min((uint32)(p_drop * 2^32), 2^32 - 1)
 * seed: a DEVICE scalar the kernel reads (a captured graph sees a new value at every replay); layer >= 0 separates the
 * layers that share one seed; row0 >= 0 is added to the row index, so a caller holding rows [row0, row0 + rows) of a batch
 * draws that batch's bits.  y > 0 then holds exactly where the cell was kept and its pre-activation was positive, so the
 * stored output is the whole mask: the backward calls take that y and compute dx, dW, db from gz = (y > 0) ? g * s : 0 with
 * the same fp32 s the forward used (recomputed from p_drop), one rounding -- what native_dropout_backward followed by
 * threshold_backward gives.  Splits, workspace (xdfm_dense_bwd_w_ws_elems) and summation order are those of
 * xdfm_dense_bwd_w.  p_drop = 0 runs the plain kernels: the bits of the entry points above, any act, seed may be NULL.
 * XDFM_ERR_INVALID: p_drop outside [0, 1); p_drop > 0 with seed = NULL, with act != XDFM_ACT_RELU (the backward reads the mask
 * off y > 0) or, in the backward calls, with y = NULL; layer < 0; row0 < 0; whatever the plain entry points refuse.
 * xdfm_dense_dropout_mask writes keep [rows][out] as bytes (1 = kept): a test hook. */
int xdfm_dense_fwd_drop(const float* x, long rows, int in, long ldx, const float* W, int out, const float* b, int act, float* y,
                        long ldy, float p_drop, const unsigned long long* seed, int layer, long row0, void* stream);
int xdfm_dense_bwd_x_drop(const float* g, long ldg, const float* y, long ldy, long rows, int out, const float* W, int in, float* dx,
                          long lddx, float p_drop, void* stream);
int xdfm_dense_bwd_w_drop(const float* g, long ldg, const float* y, long ldy, const float* x, long ldx, long rows, int in, int out,
                          float* ws, float* dW, float* db, float p_drop, void* stream);
int xdfm_dense_dropout_mask(long rows, int out, float p_drop, const unsigned long long* seed, int layer, long row0,
                            unsigned char* keep, void* stream);
/* The same layer followed by nn.PReLU() (deepctr/layers/core.py:104-134 with activation='prelu'): one scalar slope per layer,
 * torch's prelu.  With z = x W^T + b the pre-activation:
 *     y = z > 0 ? z : alpha * z,     gz = z > 0 ? g : alpha * g (one fp32 rounding),     dalpha = sum over z <= 0 of g * z;
 * a cell with z == 0 takes the alpha branch and adds 0 to dalpha.  alpha: a DEVICE scalar every kernel reads (the optimizer
 * moves it, and a replayed graph sees the new value); any finite value -- 0, 1 and negative slopes included, so neither the sign
 * nor the value of z can be read off y: the backward takes z, which the forward stores next to y.
 * xdfm_dense_prelu_fwd (one launch): y [rows][ldy >= out] and z [rows][ldz >= out]; z = NULL (evaluation) stores y only,
 * the same bits.  y == z is invalid.
 * xdfm_dense_prelu_bwd_x: dx = gz W; gz is formed while g is staged and never stored.
 * xdfm_dense_prelu_bwd_w: dW = gz^T x, db = column sums of gz (NULL: not wanted) with the splits, the slabs and the pairwise
 * finish of xdfm_dense_bwd_w -- the same bits as that call given a materialised gz.  dalpha (one float, NULL: not wanted): the
 * blocks that leave the bias partials also leave one partial per (64-wide tile of out, split), the products g * z and
 * every sum in double; the finish launch adds them in a fixed order and rounds once to fp32 (it runs for a single split too).
 * No atomics, no zeroed cells, the same bits on every run.  ws: xdfm_dense_prelu_bwd_w_ws_elems floats, 8-byte aligned (the
 * partials of dalpha are doubles); nothing in it needs initialising.
 * XDFM_ERR_INVALID, before any device call: what the plain entry points refuse, a NULL alpha or z (backward), y == z, ldz < out,
 * a NULL or misaligned workspace. */
size_t xdfm_dense_prelu_bwd_w_ws_elems(long rows, int in, int out);    /* 0 outside xdfm_dense_supported */
int xdfm_dense_prelu_fwd(const float* x, long rows, int in, long ldx, const float* W, int out, const float* b, const float* alpha,
                         float* y, long ldy, float* z, long ldz, void* stream);
int xdfm_dense_prelu_bwd_x(const float* g, long ldg, const float* z, long ldz, const float* alpha, long rows, int out, const float* W,
                           int in, float* dx, long lddx, void* stream);
int xdfm_dense_prelu_bwd_w(const float* g, long ldg, const float* z, long ldz, const float* alpha, const float* x, long ldx, long rows,
                           int in, int out, float* ws, float* dW, float* db, float* dalpha, void* stream);

/* ------------------------------------------------------------------ elementwise PReLU, one scalar slope (K13, csrc/prelu.hip)
 * replaces: aten::_prelu_kernel, _prelu_kernel_backward and the `sum` behind it (a memset inside a captured step) for the
 * layers the fused calls above do not take: widths that are no multiple of 32, a batch norm in front, the library GEMM route.
 * u, y, g, du: [rows][ld >= cols] fp32, any rows >= 1, cols >= 1 and any pitch; alpha: a device scalar, as above.
 * xdfm_prelu_fwd (one launch): y = u > 0 ? u : alpha * u.
 * xdfm_prelu_bwd (two launches at most): du = u > 0 ? g : alpha * g and dalpha = sum over u <= 0 of g * u, under the rules of
 * xdfm_dense_prelu_bwd_w: one partial per block in ws (xdfm_prelu_ws_elems floats, 8-byte aligned: doubles), products and sums
 * in double, a one-block second launch that adds them in a fixed order and rounds once.  du or dalpha may be NULL (not both):
 * the other keeps its bits; without dalpha there is one launch and ws is not read.
 * XDFM_ERR_INVALID, before any device call: a NULL operand, du and dalpha both NULL, rows < 1, cols < 1, a pitch below cols,
 * with dalpha a NULL or misaligned workspace. */
size_t xdfm_prelu_ws_elems(long rows, int cols);                       /* 0 for rows < 1 or cols < 1 */
int xdfm_prelu_fwd(const float* u, long ldu, long rows, int cols, const float* alpha, float* y, long ldy, void* stream);
int xdfm_prelu_bwd(const float* g, long ldg, const float* u, long ldu, long rows, int cols, const float* alpha, float* du, long lddu,
                   float* dalpha, float* ws, void* stream);

/* ------------------------------------------------------------------ batch norm + activation of a dense layer (K12, csrc/bn.hip)
 * replaces: nn.BatchNorm1d, the activation and their autograd in deepctr/layers/core.py:120-134 with use_bn=True.
 * z [rows][ldz >= cols] fp32 is the dense layer's output; statistics are per column, over the rows.  gamma, beta, save_mean,
 * save_rstd, running_mean, running_var, dgamma, dbeta: [cols].  y, g, dz: [rows][ld >= cols].  act: XDFM_ACT_*.
 * xdfm_bn_fwd_train (two launches): every block of xdfm_bn_row_block() rows leaves the pair (mean, M2 = sum (z - mean)^2) of
 * its rows per column in ws (xdfm_bn_ws_elems(rows, cols) floats' worth of memory, 8-byte aligned: the pairs are kept as
 * doubles; nothing in it needs initialising); the second launch merges the pairs with Chan's formula in a fixed order -- never
 * a raw sum of squares -- and writes
 *     y = act(gamma * (z - mean) * rstd + beta),   rstd = 1 / sqrt(var + eps),  var = M2 / rows (biased),
 *     save_mean = mean, save_rstd = rstd,
 *     running_mean = (1 - momentum) * running_mean + momentum * mean,
 *     running_var  = (1 - momentum) * running_var  + momentum * M2 / (rows - 1)      (unbiased, as nn.BatchNorm1d),
 * both running vectors updated in place.  rows >= 2.
 * xdfm_bn_fwd_eval (one launch): the same y with mean = running_mean, rstd = 1 / sqrt(running_var + eps).  rows >= 1.
 * xdfm_bn_bwd (two launches): with gm = act'(y) * g (relu: y > 0 ? g : 0; sigmoid: g * y * (1 - y); linear: g; never stored)
 * and xhat = (z - save_mean) * save_rstd, the per-block partial sums of gm and gm * xhat go to ws, then
 *     dz = gamma * rstd * (gm - sum(gm) / rows - xhat * sum(gm * xhat) / rows),  dbeta = sum(gm),  dgamma = sum(gm * xhat).
 * dz, dgamma and dbeta may each be NULL: only what is asked for is written, with the same bits.
 * xdfm_bn_bwd_eval: the backward of xdfm_bn_fwd_eval, whose statistics are constants: mean / rstd [cols] are the caller's
 * running_mean and 1 / sqrt(running_var + eps); dz = gamma * rstd * gm, dbeta and dgamma as above.  rows >= 1.
 * No atomics, no zeroed cells, no memset, the same bits on every run; no entry point synchronises or allocates.
 * XDFM_ERR_INVALID, before any device call: a NULL operand (ws included; or a ws off 8-byte alignment), rows < 1 (< 2 in
 * training and its backward),
 * cols < 1, a pitch below cols, an unknown act, eps <= 0, momentum outside [0, 1].
 *
 * Synchronised batch norm (row-parallel training: statistics over the global batch, as torch's SyncBatchNorm).  Each
 * direction of the training batch norm is split where the other ranks' numbers are needed; the caller runs one all-gather in
 * between.  The rules above hold for all four entry points.
 * xdfm_bn_stats (two launches): pair double[2][cols] = (mean, M2) of this rank's rows (rows >= 1), per-block pairs merged
 * with Chan's formula in the order xdfm_bn_fwd_train uses; ws as for xdfm_bn_fwd_train.
 * xdfm_bn_fwd_apply_sync (one launch): all is device memory double[world][1 + 2 * cols], per rank its count, its means, its
 * M2s (the count followed by the rank's pair: what the all-gather delivers).  The triples are merged with Chan's formula in
 * doubles in rank order 0 .. world - 1, a rank whose count is 0 (one that holds only a stand-in row) is skipped; n = the sum
 * of the counts, which the caller keeps >= 2 (the count is device data: it is not validated here).  y, save_mean, save_rstd
 * and both running vectors are as xdfm_bn_fwd_train writes them with rows = n: var = M2 / n, running_var takes M2 / (n - 1),
 * each running element updated in place by exactly one block.  The y of a stand-in row uses the global statistics.
 * xdfm_bn_bwd_sums (two launches): sums double[2][cols] = (sum gm, sum gm * xhat) over this rank's rows (rows >= 1), per-block
 * partials added in a fixed order; gm formed while g is loaded; ws as for xdfm_bn_bwd.
 * xdfm_bn_bwd_apply_sync (one launch): all is double[world][2 * cols], the ranks' sums; S1, S2 = their sums in rank order;
 *     dz = gamma * rstd * (gm - S1 / n_total - xhat * S2 / n_total),
 * dbeta, dgamma = this rank's own sums (row `rank` of all) rounded to fp32: the caller's all-reduce SUM of the dense
 * gradients makes them global.  rows_counted is rows, or 0 for a rank that holds only a stand-in row: every element of its
 * dz is an exact zero (its own sums are zero, the other ranks' are not).  dz, dgamma and dbeta may each be NULL.
 * XDFM_ERR_INVALID, before any device call, as above and: world < 1, rank outside [0, world), n_total < 2, rows_counted
 * neither rows nor 0, pair / sums / all off 8-byte alignment. */
int xdfm_bn_row_block(void);
size_t xdfm_bn_ws_elems(long rows, int cols);                          /* 0 for rows < 1 or cols < 1 */
int xdfm_bn_fwd_train(const float* z, long ldz, long rows, int cols, const float* gamma, const float* beta, float eps, float momentum,
                      int act, float* y, long ldy, float* save_mean, float* save_rstd, float* running_mean, float* running_var,
                      float* ws, void* stream);
int xdfm_bn_fwd_eval(const float* z, long ldz, long rows, int cols, const float* gamma, const float* beta, float eps, int act, float* y,
                     long ldy, const float* running_mean, const float* running_var, void* stream);
int xdfm_bn_bwd(const float* g, long ldg, const float* y, long ldy, const float* z, long ldz, long rows, int cols, const float* gamma,
                const float* save_mean, const float* save_rstd, int act, float* dz, long lddz, float* dgamma, float* dbeta, float* ws,
                void* stream);
int xdfm_bn_bwd_eval(const float* g, long ldg, const float* y, long ldy, const float* z, long ldz, long rows, int cols,
                     const float* gamma, const float* mean, const float* rstd, int act, float* dz, long lddz, float* dgamma, float* dbeta,
                     float* ws, void* stream);
int xdfm_bn_stats(const float* z, long ldz, long rows, int cols, double* pair, float* ws, void* stream);
int xdfm_bn_fwd_apply_sync(const float* z, long ldz, long rows, int cols, const double* all, int world, const float* gamma,
                           const float* beta, float eps, float momentum, int act, float* y, long ldy, float* save_mean,
                           float* save_rstd, float* running_mean, float* running_var, void* stream);
int xdfm_bn_bwd_sums(const float* g, long ldg, const float* y, long ldy, const float* z, long ldz, long rows, int cols,
                     const float* save_mean, const float* save_rstd, int act, double* sums, float* ws, void* stream);
int xdfm_bn_bwd_apply_sync(const float* g, long ldg, const float* y, long ldy, const float* z, long ldz, long rows, long rows_counted,
                           int cols, const double* all, int world, int rank, long n_total, const float* gamma, const float* save_mean,
                           const float* save_rstd, int act, float* dz, long lddz, float* dgamma, float* dbeta, void* stream);

/* ------------------------------------------------------------------ output head: link + loss (K8)
 * z_b = lin_b + <u_b, wu> + <v_b, wv> + bias,  pred = LINK(z),  loss = sum_b LOSS(pred_b, y_b).
 * replaces: cin_linear / dnn_linear (the two [B,K]x[K,1] products of deepctr/models/xdeepfm.py:95-105), the
 * logit sum, PredictionLayer (deepctr/layers/core.py:150-160) and the summed loss of the batch loop
 * (basemodel.py:254: F.binary_cross_entropy / F.mse_loss / F.l1_loss with reduction='sum') with their autograd
 * -- 2 GEMV + ~10 small launches forward, 4 skinny GEMMs + ~6 small launches backward -- by two launches each
 * way; fixed summation order.
 * lin [B] or NULL; u [B][Ku], wu [Ku] (or NULL); v [B][Kv], wv [Kv] (or NULL); bias [1] or NULL; y [B];
 * ws: xdfm_head_ws_elems(Ku, Kv) floats.  Backward: gloss [1]; dlin [B] or NULL; du [B][Ku]; dv [B][Kv];
 * grads [Ku + Kv + 1] = d wu | d wv | d bias.
 * link: XDFM_LINK_SIGMOID (task "binary", pred = 1 / (1 + exp(-z))) or XDFM_LINK_IDENTITY (task "regression",
 * pred = z).  loss: XDFM_LOSS_BCE (logs clamped at -100, as ATen), XDFM_LOSS_MSE ((pred - y)^2) or XDFM_LOSS_MAE
 * (|pred - y|, gradient sign with sgn(0) = 0, as torch.sign).  The backward reads pred and y only.  The _ex entry
 * points return XDFM_ERR_INVALID, before any device call and with both values in the message, for a link outside
 * {0, 1}, a loss outside {0, 1, 2} and for (identity, bce), which does not exist.  xdfm_head_fwd / xdfm_head_bwd
 * are the _ex calls with (XDFM_LINK_SIGMOID, XDFM_LOSS_BCE).
 *
 * Example weights (xdfm_head_fwd_w / xdfm_head_bwd_w; the `sample_weight` / `class_weight` of fit()): the _ex
 * arguments plus w [B] fp32 or NULL, in front of the stream.
 *   forward   loss = sum_b fl(w_b * LOSS(pred_b, y_b)), rows, blocks and the 128-partial tree in the order of the
 *             unweighted call; pred does not depend on w.
 *   backward  g_b = fl(w_b * g) with g the unweighted row gradient d loss / d z of the table in csrc/reg.hip; dlin,
 *             du, dv, d wu, d wv and d bias are formed from g_b as in the unweighted call.
 *   value     roundings                                                    beside the unweighted call
 *   term      fl(w_b * term): the product is never fused into the sum      + 1 per row
 *   g_b       fl(w_b * g)                                                  + 1 per row (6 / 4 / 3 / 1 for the mse,
 *                                                                            mae rows of the table; bce likewise + 1)
 * The kernel does not look at the range of w: a row with w_b = 0 and a finite pred adds an exact zero to the loss
 * and to every gradient (a NaN or infinite term times zero is NaN, as in IEEE arithmetic); a negative or non-finite
 * weight is the caller's to refuse (fit() does).  w == NULL is the _ex call, bit for bit and launch for launch: the
 * unweighted kernel instances are the ones _ex launches, the weighted ones are instances of their own.  Refused
 * with XDFM_ERR_INVALID before any device call: whatever _ex refuses, and a w that is not 4-byte aligned (the
 * message names w). */
enum { XDFM_LINK_SIGMOID = 0, XDFM_LINK_IDENTITY = 1 };
enum { XDFM_LOSS_BCE = 0, XDFM_LOSS_MSE = 1, XDFM_LOSS_MAE = 2 };
size_t xdfm_head_ws_elems(int Ku, int Kv);
int xdfm_head_fwd(const float* lin, const float* u, const float* wu, int Ku, const float* v, const float* wv, int Kv,
                  const float* bias, const float* y, int B, float* pred, float* loss, float* ws, void* stream);
int xdfm_head_bwd(const float* pred, const float* y, const float* gloss, const float* u, const float* wu, int Ku,
                  const float* v, const float* wv, int Kv, int B, float* dlin, float* du, float* dv, float* grads,
                  float* ws, void* stream);
int xdfm_head_fwd_ex(const float* lin, const float* u, const float* wu, int Ku, const float* v, const float* wv, int Kv,
                     const float* bias, const float* y, int B, float* pred, float* loss_out, float* ws, int link, int loss,
                     void* stream);
int xdfm_head_bwd_ex(const float* pred, const float* y, const float* gloss, const float* u, const float* wu, int Ku,
                     const float* v, const float* wv, int Kv, int B, float* dlin, float* du, float* dv, float* grads,
                     float* ws, int link, int loss, void* stream);
int xdfm_head_fwd_w(const float* lin, const float* u, const float* wu, int Ku, const float* v, const float* wv, int Kv,
                    const float* bias, const float* y, int B, float* pred, float* loss_out, float* ws, int link, int loss,
                    const float* w, void* stream);
int xdfm_head_bwd_w(const float* pred, const float* y, const float* gloss, const float* u, const float* wu, int Ku,
                    const float* v, const float* wv, int Kv, int B, float* dlin, float* du, float* dv, float* grads,
                    float* ws, int link, int loss, const float* w, void* stream);

/* ------------------------------------------------------------------ Adam (K7)
 * replaces: torch.optim.Adam.step() (deepctr/models/basemodel.py:452).  The embedding / linear tables carry
 * dense gradients (deepctr/inputs.py:168), so the step streams every parameter: 28 B per parameter, arithmetic
 * of ATen's fused Adam in fp32.  `tensors` is a HOST array of T descriptors (device pointers inside; they travel
 * by value in the kernel arguments, 64 per launch); `step` points to the fp32 step counter torch keeps per
 * parameter, already incremented for this step.
 * l2 > 0 in a descriptor: the kernel uses g + 2*l2*w as the gradient (the term l2 * sum(w^2) of
 * basemodel.py:412-428 with unit upstream gradient); with l2_value != NULL it also returns
 * sum_t l2_t * sum(w_t^2) of the weights BEFORE the update (l2_ws: xdfm_adam_step_ws_elems(T) floats).
 * ABI 3 added grad_marks.  Errors (NULL `tensors`, T <= 0 or T > 65535, a NULL member pointer, lr < 0, a beta outside
 * [0, 1), eps < 0, l2_value without l2_ws, XDFM_ADAM_LAZY without grad_marks, XDFM_ADAM_DEFERRED without a clock, grad_marks
 * or last, grad_marks with a pointer that is not 16-byte aligned) are reported before any device work. */
typedef struct {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    const float* step;
    long numel;
    float l2;
    /* NULL: grad is read in full and left alone.  Otherwise one byte per 16-byte chunk of grad (which must be
     * 16-byte aligned; see xdfm_embed_scatter_bwd_marked): a chunk whose mark is 0 is taken as zeros without
     * being read; a marked chunk is read, then overwritten with zeros, and its mark cleared -- after the step
     * the gradient buffer is all zeros again, ready for the next scatter.  The numel % 4 tail elements are always
     * read and zeroed. */
    unsigned char* grad_marks;
    /* XDFM_ADAM_LAZY (needs grad_marks): OPT-IN deviation from the reference.  Only marked chunks are updated at all --
     * an untouched row keeps its weight and moments (no moment decay, no L2 pull) until a batch touches it again, as
     * in "lazy" / row-sparse Adam; the step's cost then follows the rows a batch touches (plus one mark byte per 16
     * bytes of table) instead of the vocabulary.  The reference's torch.optim.Adam over dense gradients (deepctr/
     * inputs.py:168 sparse=False, basemodel.py:452) updates every row every step: 0 keeps that arithmetic. */
    int flags;
    /* XDFM_ADAM_DEFERRED (needs grad_marks): one byte per 16-byte chunk of param = the step (counted since the last
     * flush, see xdfm_adam_clock) up to which the chunk's weight and moments have been updated. */
    unsigned char* last;
} xdfm_adam_tensor;
enum { XDFM_ADAM_LAZY = 1, XDFM_ADAM_DEFERRED = 2 };
size_t xdfm_adam_step_ws_elems(int T);
int xdfm_adam_step(const xdfm_adam_tensor* tensors, int T, double lr, double beta1, double beta2, double eps,
                   float* l2_ws, float* l2_value, void* stream);
/* Same with the learning rate read from device memory when lr_dev != NULL (one double; `lr` is then ignored): a
 * captured HIP graph of the step follows a learning-rate schedule (the host rewrites the scalar between replays)
 * instead of being captured again for every value. */
int xdfm_adam_step_lr(const xdfm_adam_tensor* tensors, int T, double lr, const double* lr_dev, double beta1, double beta2,
                      double eps, float* l2_ws, float* l2_value, void* stream);

/* ------------------------------------------------------------------ SGD and Adagrad (K7s, K7g)
 * replaces: torch.optim.SGD(lr=0.01).step() and torch.optim.Adagrad().step() (deepctr/models/basemodel.py:447-461,
 * the trainer's --optimizer sgd|adagrad) with K7's streaming sweep: 8 bytes per parameter (SGD: p read + written) or
 * 16 (Adagrad: p and the accumulator `state`), in fp32 and in ATen's order:
 *   g' = fma(2 l2, p, g);   SGD: p = fma(-lr, g', p);   Adagrad: s = s + g' g', p = fma(-lr, g' / (sqrt(s) + eps), p)
 * (momentum 0, lr_decay 0, no weight decay; IEEE sqrt and division).  Descriptors, `lr` / `lr_dev`, `l2`, `l2_ws`
 * (xdfm_opt_step_ws_elems(T) floats) and `l2_value` (sum_t l2_t * sum(w_t^2) of the weights BEFORE the update) are
 * K7's; so is `grad_marks` (see xdfm_adam_tensor: unmarked chunks are zeros and not read, marked ones are read,
 * re-zeroed and unmarked, the numel % 4 tail is always read and zeroed; needs 16-byte aligned param / grad / state),
 * with one exact shortcut: an unmarked chunk of a tensor with l2 == 0 has g' == 0, which changes neither p nor s, so it
 * is skipped without reading them -- such a tensor costs one mark byte per 16 bytes of gradient.  With l2 > 0 an
 * unmarked chunk is a real update and is computed as a marked one with g = 0: marks on / off give the same bits.
 * Tensors whose pointers are not 16-byte aligned take a scalar path.  Errors (NULL `tensors`, T <= 0, Adagrad without
 * `state`, eps <= 0) are reported before any device work. */
typedef struct {
    float* param;
    float* grad;
    float* state;                   /* Adagrad: the accumulator ("sum"); RMSprop: "square_avg"; SGD with momentum: "momentum_buffer"; SGD: NULL */
    long numel;
    float l2;
    unsigned char* grad_marks;      /* NULL: grad is read in full and left alone */
} xdfm_opt_tensor;
size_t xdfm_opt_step_ws_elems(int T);
int xdfm_sgd_step(const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, float* l2_ws, float* l2_value,
                  void* stream);
int xdfm_adagrad_step(const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, double eps, float* l2_ws,
                      float* l2_value, void* stream);
/* RMSprop (K7r) -- replaces: torch.optim.RMSprop(params).step(), the fourth string of basemodel.py:447-461 -- for
 * momentum 0, not centered, no weight decay: the same sweep, descriptors (`state` is the accumulator "square_avg"), rate,
 * L2 term and marks, 16 bytes per parameter, in ATen's order (torch/optim/rmsprop.py):
 *   g' = fma(2 l2, p, g);   v = fma(1 - alpha, g' g', alpha v);   p = fma(-lr, g' / (sqrt(v) + eps), p)
 * with alpha and 1 - alpha (taken in double) rounded to float.  v decays in every step whatever the gradient, so the exact
 * shortcut of K7s / K7g does not apply: an unmarked chunk of a tensor with l2 == 0 is computed with g = 0 like any other
 * (its p keeps its bits, its v becomes alpha v).  Marks on / off give the same bits.  Errors (as above; eps <= 0, alpha
 * outside [0, 1), a tensor without `state`) are reported before any device work. */
int xdfm_rmsprop_step(const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, double alpha, double eps,
                      float* l2_ws, float* l2_value, void* stream);
/* SGD with momentum (K7m) -- replaces: torch.optim.SGD(params, momentum=mu[, nesterov=True]).step() -- for dampening 0, no
 * weight decay, not maximize: the same sweep, descriptors (`state` is torch's "momentum_buffer"), rate, L2 term and marks,
 * 16 bytes per parameter, one fma per line of torch/optim/sgd.py:
 *   g' = fma(2 l2, p, g);   buf = fma(mu, buf, g');   d = nesterov ? fma(mu, buf, g') : buf;   p = fma(-lr, d, p)
 * with mu rounded to float.  The buffer is signed and moves its weight in every step whatever the gradient, so the exact
 * shortcut of K7s / K7g does not apply, with or without an L2 term: an unmarked chunk is computed with g = 0 like any other
 * (RMSprop's rule; here p moves too).  Marks on / off give the same bits.  torch makes the buffer at the first step as
 * clone(g'); a zero buffer gives the same value (mu * 0 + g'), but for the sign of a zero.  Errors (as above; mu outside
 * (0, 1), a tensor without `state` or with one that is not 4-byte aligned -- 16-byte with grad_marks) are reported before any
 * device work, with the offending value in the message. */
int xdfm_sgdm_step(const xdfm_opt_tensor* tensors, int T, double lr, const double* lr_dev, double mu, int nesterov, float* l2_ws,
                   float* l2_value, void* stream);
/* FTRL-Proximal (K7f, csrc/ftrl.hip) -- per-coordinate, lr_power -0.5 (McMahan et al., "Ad click prediction: a view from the
 * trenches", 2013); the reference has no counterpart, the host fallback (xdfm_amd.optim.TableFTRL) spells the same formulas in
 * torch ops.  The same sweep, rate (`lr` / `lr_dev`), L2 term (`l2` of the descriptor, here l2m; `l2_ws` of
 * xdfm_opt_step_ws_elems(T) floats, `l2_value`) and marks as above, over a descriptor with TWO state arrays, z and n:
 *   g' = fma(2 l2m, p, g)
 *   g' == 0:  p, z and n keep their bits                                   (the zero-gradient rule)
 *   n' = fma(g', g', n);   r1 = sqrt(n'), r0 = sqrt(n)                     (IEEE)
 *   sigma = (g' g') / (lr (r1 + r0))          -- the paper's (r1 - r0) / lr as a quotient: no cancellation of the roots
 *   z' = fma(-sigma, p, z + g')
 *   p' = |z'| <= l1 ? 0 : (sign(z') l1 - z') / ((beta + r1) / lr + l2)
 * (one corner: n == 0 with |g'| < 2.6e-23, whose square underflows, takes r1 = |g'|, the root of the exact sum, and sigma = 0
 * where the quotient is 0 / 0 -- no NaN from finite inputs)
 * with l1, l2, beta and the rate rounded to float; the L2 term's value is taken of the weights BEFORE the update.  `l2` is the
 * paper's lambda_2 and enters the denominator as it is (TensorFlow's l2_regularization_strength is half of it).  The L1 term
 * clips a weight to exactly 0.0.  The zero-gradient rule is a select: an element without a gradient is not touched (no 0 / 0
 * at n == 0, and a weight that never saw a gradient keeps its initial value), so the exact shortcut of K7s / K7g holds -- an
 * unmarked chunk of a tensor with l2m == 0 is skipped without being read, one mark byte per 16 bytes of gradient -- and marks
 * on / off give the same bits.  24 bytes per updated parameter (p, z, n read and written), plus 4 for a gradient read in full
 * or 1/16 for its mark byte.  param, grad, z and n 16-byte aligned: the float4 path; anything else: a scalar path (z and n must
 * be 4-byte aligned; with grad_marks all four must be 16-byte aligned).  Errors (NULL `tensors`, T <= 0, lr <= 0 -- whether or
 * not lr_dev is given; the rate behind lr_dev is the caller's to keep above 0 --, l1 < 0, l2 < 0, beta < 0, a tensor without z
 * or n, a misaligned state) are reported before any device work, with the offending value in the message. */
typedef struct {
    float* param;
    float* grad;
    float* z;                       /* the adjusted gradient sum */
    float* n;                       /* the sum of squared gradients (starts at the initial accumulator value) */
    long numel;
    float l2;                       /* the model's L2 strength for the tensor (l2m), not FTRL's l2 */
    unsigned char* grad_marks;      /* NULL: grad is read in full and left alone */
} xdfm_ftrl_tensor;
int xdfm_ftrl_step(const xdfm_ftrl_tensor* tensors, int T, double lr, const double* lr_dev, double l1, double l2, double beta,
                   float* l2_ws, float* l2_value, void* stream);

/* Row-wise Adagrad (K7w, csrc/rowwise.hip) -- the rule large CTR embedding tables are usually trained with (the DLRM / TorchRec
 * default, FBGEMM's "exact row-wise Adagrad"); the reference has no counterpart, the host fallback
 * (xdfm_amd.optim.TableRowwiseAdagrad) spells the same formulas in torch ops.  A tensor is [rows, dim], row-major and dense;
 * `state` holds ONE accumulator per row ([rows] floats): 1 / dim of Adagrad's state, and 8 + 8 / dim bytes per parameter and
 * sweep where K7g moves 16.  The same rate (`lr` / `lr_dev`), L2 term (`l2` of the descriptor, here l2m; `l2_ws` of
 * xdfm_opt_step_ws_elems(T) floats; `l2_value` = sum_t l2_t * sum(w_t^2) of the weights BEFORE the update), option "opt_bx"
 * and launch composition as above.  Per row, in fp32 unless said otherwise:
 *   g'_d = fma(2 l2m, p_d, g_d)                                  d = 0 .. dim-1
 *   S    = sum_d (double)g'_d * (double)g'_d                     exact products, added in double, in THE ORDER below
 *   ms   = (float)(S / (double)dim)
 *   s'   = s + ms                                                ms == 0: s keeps its bits
 *   den  = sqrtf(s') + eps                                       IEEE sqrt; eps > 0
 *   p_d' = fma(-lr, g'_d / den, p_d)                             IEEE division; g'_d == 0: p_d keeps its bits
 * THE ORDER of S, fixed per dim and the same on every path (float4 or scalar, marks on or off, any grid), so that all paths
 * give the same bits: the row is cut into chunks of four consecutive elements (the last chunk has dim % 4 when that is not 0);
 * a chunk's squares are added left to right, ((x0 + x1) + x2) + x3; the ceil(dim / 4) chunk sums are padded with zeros to the
 * next power of two and added as a balanced tree, neighbouring pairs first (t[j] = t[2j] + t[2j + 1] until one is left).
 * The zero-gradient rule: a row whose g' is all zeros keeps the bits of s and p (two selects, see csrc/opt_math.h), so with
 * l2m == 0 a row none of whose chunks is marked is skipped without being read -- the step costs the mark bytes and the batch's
 * rows.  With l2m > 0 every row is a real update; an unmarked chunk enters with g = 0.  Marks on / off give the same bits.  A
 * row whose squares underflow even in double's mean (ms == 0 with g' != 0) keeps s and moves p by lr g' / (sqrt(s) + eps): no
 * NaN from finite inputs.  dim == 1 IS Adagrad: the call gives the bits of xdfm_adagrad_step on the same data (it runs that
 * kernel's element update).
 * Marks (`grad_marks`: one byte per 16-byte chunk of `grad`, ceil(rows dim / 4) of them; needs 16-byte aligned param and grad):
 * marked chunks are read, re-zeroed and unmarked, unmarked ones are never read.  Every chunk is read and re-zeroed by the same
 * thread: for dim in {4, 8, 16, 32, 64} a chunk lies inside one row; for every other dim the owner is a unit of four
 * consecutive rows, which is exactly dim whole chunks.  The rows % 4 tail rows of such a tensor are always read in full, zeroed
 * and unmarked (the numel % 4 rule of the other kernels): their gradient must be real.
 * Paths: dim in {4, 8, 16, 32, 64} with 16-byte aligned param and grad -- dim / 4 lanes hold a row in registers, streaming
 * float4 accesses; anything else (dim % 4 != 0, other multiples of 4, unaligned pointers) -- one thread per four rows, scalar
 * accesses, correct rather than fast.  `state` needs 4-byte alignment only.
 * Errors, reported before any device work with the offending value in the message: NULL `tensors`, T outside [1, 65535], a NULL
 * param / grad / state, rows < 0, dim outside [1, XDFM_ROWWISE_MAX_DIM], l2 < 0, lr < 0, eps <= 0, l2_value without l2_ws,
 * a state that is not 4-byte aligned, grad_marks with a param or grad that is not 16-byte aligned.
 * Not covered: a deferred form, lr_decay, weight decay, FBGEMM's weighted / counter variants. */
#define XDFM_ROWWISE_MAX_DIM 1024
typedef struct {
    float* param;                   /* [rows, dim] */
    float* grad;                    /* [rows, dim] */
    float* state;                   /* [rows]: the row's accumulator ("sum") */
    long rows;
    int dim;
    float l2;                       /* the model's L2 strength for the tensor (l2m) */
    unsigned char* grad_marks;      /* NULL: grad is read in full and left alone */
} xdfm_rowwise_tensor;
int xdfm_rowwise_adagrad_step(const xdfm_rowwise_tensor* tensors, int T, double lr, const double* lr_dev, double eps,
                              float* l2_ws, float* l2_value, void* stream);

/* ------------------------------------------------------------------ deferred Adam for the tables (K7d)
 * Same arithmetic, same results, bit for bit, as the dense sweep above -- but the sweep's 24 bytes per table parameter
 * and step are not moved every step.  The reference's torch.optim.Adam over dense table gradients (inputs.py:168,
 * basemodel.py:452) updates every row every step; a row no batch touches sees the gradient 2*l2*w only, so its
 * (w, m, v) after k untouched steps is a function of its state k steps ago and of the steps' bias corrections.  A
 * chunk is therefore updated when it is NEEDED: before a batch gathers it (xdfm_adam_catchup_rows replays its missed
 * steps, in registers), when a gradient arrives for it (XDFM_ADAM_DEFERRED in the step), and every F steps for all
 * chunks (xdfm_adam_flush) -- which bounds every replay to F steps and turns the HBM-bound sweep (2.5 ms per step at
 * 575 M parameters) into an ALU-bound one (0.63 ms per step's worth of updates, tools/ubench/replay.hip) that touches
 * memory once per F steps.  The value of the L2 term of the replayed steps (of the weights before each replayed
 * update) is accumulated into `backlog`: summed over an epoch it equals the dense path's.
 * clock: device int[2] = {steps since the last flush, steps before it}; consts: device float[4*cap] (16-byte aligned), per
 * step since the last flush the step size lr / (1 - beta1^t), c = sqrt(1 - beta2^t), c * 2^32 and RN(1/c) * 2^-32 (0 when the
 * step's constants fall outside the range the replay's short forms are proven for), written by the step itself. */
typedef struct {
    int* clock;
    float* consts;
    int cap;            /* steps the table holds, 3 .. 256 (`last` is one byte per chunk): flush before clock[0] reaches it */
} xdfm_adam_clock;
/* xdfm_adam_step_lr with a clock: advances it, records the step's constants, and treats XDFM_ADAM_DEFERRED tensors by
 * their marks only (replaying, for a marked chunk, whatever steps it still misses, then this one).  A tensor whose `step`
 * counter is not the clock's clock[0] + clock[1] takes THIS step with constants of its own counter; the steps a chunk
 * missed are always replayed with the clock's table (here, in the catch-up and in the flush), so a deferred tensor gives
 * the sweep's bits only while its counter is the clock's or none of its chunks falls behind.  Errors (those of
 * xdfm_adam_step_lr; a NULL clock or member, cap <= 2, cap > 256) are reported before any device work. */
int xdfm_adam_step_deferred(const xdfm_adam_tensor* tensors, int T, const xdfm_adam_clock* clk, double lr,
                            const double* lr_dev, double beta1, double beta2, double eps, float* l2_ws, float* l2_value,
                            void* stream);
/* Device-side tables of one gather's fields: pointers to the rows' parameter / moment / `last` arrays, L2 strengths. */
typedef struct {
    float* const* param;            /* device array [m] */
    float* const* exp_avg;
    float* const* exp_avg_sq;
    unsigned char* const* last;
    const float* l2;                /* device array [m] */
    float* const* grad;             /* xdfm_adam_apply_rows only: the tables' dense gradients and their mark bytes */
    unsigned char* const* marks;
} xdfm_adam_rows;
/* Brings the rows a batch is about to gather (X, cols, vocab as in xdfm_embed_gather_fwd; lin may be NULL) up to the
 * clock.  backlog: one 64-bit device cell (8-byte aligned, zeroed once by the caller); the L2 value of the replayed
 * steps is ADDED to it in 2^-40 fixed point (integer adds: the total does not depend on the order of the threads).
 * Errors (a NULL argument other than `lin`, a NULL clock member, cap outside 3 .. 256, B, m or D <= 0, an unaligned
 * backlog) are reported before any device work. */
int xdfm_adam_catchup_rows(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                           const xdfm_adam_rows* emb, const xdfm_adam_rows* lin, const xdfm_adam_clock* clk,
                           double beta1, double beta2, double eps, float* backlog, void* stream);
/* The step's update of the deferred tables, keyed by the batch instead of by a scan of the mark bytes: for the rows of X
 * (the batch whose gradients the scatter just wrote: single process), apply step clock[0] -- to be called after
 * xdfm_adam_step_deferred over the OTHER tensors, which advances the clock.  Reads the rows' gradient chunks, zeroes
 * them and their marks, updates the numel % 4 tail elements of every table densely.  l2_cell: 8-byte device scratch
 * (zero before the first call); l2_value[0] += the L2 value of the touched rows (may be NULL).  Errors (as the catch-up's;
 * emb or lin without grad, marks or last; an unaligned l2_cell) are reported before any device work. */
int xdfm_adam_apply_rows(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                         const xdfm_adam_rows* emb, const xdfm_adam_rows* lin, const xdfm_adam_clock* clk,
                         double beta1, double beta2, double eps, float* l2_cell, float* l2_value, void* stream);
/* xdfm_adam_step_deferred over `tensors` and xdfm_adam_apply_rows over the rows of X, as ONE call: the step and the rows
 * update touch different tensors and both only read what the clock's tick wrote, so nothing orders them.  With option
 * "colaunch" bit 0 set (the default) the tick stays a launch of its own in front, then ONE launch runs the step's
 * workgroups followed by the rows update's (with more than 64 tensors: behind those of the first of the step's launches),
 * then the two finishes as the separate calls issue them.  With the bit clear (and under "dbg" bit 17) the call IS the two
 * calls, launch for launch.  Same arithmetic, same sums, same bits either way.  Errors: those of the two calls, all
 * reported before any device work. */
int xdfm_colaunch_adam_step(const xdfm_adam_tensor* tensors, int T, const xdfm_adam_clock* clk, double lr,
                            const double* lr_dev, double beta1, double beta2, double eps, float* l2_ws, float* l2_value,
                            const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                            const xdfm_adam_rows* emb, const xdfm_adam_rows* lin, float* l2_cell, void* stream);
/* Brings every chunk of the XDFM_ADAM_DEFERRED tensors up to the clock, then resets the clock (clock[1] += clock[0],
 * clock[0] = 0, every `last` byte 0).  Errors (NULL tensors / clock / backlog, a NULL clock member, cap outside 3 .. 256,
 * T <= 0 or T > 65535, a deferred tensor with a NULL pointer, an unaligned backlog) are reported before any device work. */
int xdfm_adam_flush(const xdfm_adam_tensor* tensors, int T, const xdfm_adam_clock* clk, double beta1, double beta2,
                    double eps, float* backlog, void* stream);

/* ------------------------------------------------------------------ deferred SGD / Adagrad for the tables (K7sd, K7gd)
 * K7d's scheme for K7s / K7g, same bits as their sweep.  With l2 > 0 a row no batch touches still sees the gradient
 * 2*l2*w, so the sweep updates every table parameter every step; such a row evolves by a recurrence in its own state and
 * the step's rate only -- SGD: p = fma(-lr_t, 2 l2 p, p); Adagrad: g' = 2 l2 p, s = s + g' g', p = fma(-lr_t, g' /
 * (sqrt(s) + eps), p) -- and the kernels below replay the steps a chunk missed in registers, through the sweep's own
 * element update (csrc/opt_math.h: one definition, IEEE sqrt and division), when the chunk is needed: before a batch
 * gathers it (xdfm_opt_catchup_rows), when a gradient arrives for it (the step) and every F steps for all chunks
 * (xdfm_opt_flush).  8 / 16 bytes per table parameter move once per F steps instead of once per step.
 * clock: device int[2] = {steps since the last flush, steps before it}; rates: device float[cap], per step since the last
 * flush the -(float)lr that step used (from lr_dev when given), written by the step itself: a replayed HIP graph follows
 * a learning-rate schedule.  backlog: one 64-bit device cell, zeroed once by the caller; the L2 value of every replayed
 * step (of the weights before that update) is ADDED to it in 2^-40 fixed point (integer adds: order-independent).  cell:
 * 64-bit device scratch of the step, zero between calls.  Both 8-byte aligned. */
typedef struct {
    int* clock;
    float* rates;
    int cap;            /* steps the table holds, 3 .. 256: flush before clock[0] reaches it */
    unsigned long long* backlog;
    unsigned long long* cell;
} xdfm_opt_clock;
/* xdfm_sgd_step / xdfm_adagrad_step with a clock: advance it, record the step's rate.  last: host array [T]; last[t] ==
 * NULL: tensor t is stepped as xdfm_sgd_step / xdfm_adagrad_step step it.  Otherwise tensor t is deferred (needs l2 > 0 and
 * grad_marks; last[t]: device bytes, at least numel / 4 + 4 of them, 4-byte aligned, zero at the start and after a flush = the
 * step since the last flush up to which the chunk is updated): only its mark bytes are read, 16 per load; a marked chunk
 * replays the steps it still misses with g = 0, takes this step with its gradient, gets zeros written back to the
 * gradient, its mark cleared and last = clock[0].  The numel % 4 tail elements are updated every step.  l2_value: the
 * term's value for the chunks this step touched plus the tensors without `last`.  Errors (NULL descriptors, T <= 0, a bad
 * clock, cap <= 2 (hence cap <= 0), cap > 256 (`last` is one byte per chunk), a deferred tensor without grad_marks or with l2 == 0, Adagrad without state, eps <= 0) are reported
 * before any device work. */
int xdfm_sgd_step_deferred(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                           double lr, const double* lr_dev, float* l2_ws, float* l2_value, void* stream);
int xdfm_adagrad_step_deferred(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                               double lr, const double* lr_dev, double eps, float* l2_ws, float* l2_value, void* stream);
/* Device-side tables of one gather's fields; param[f] == NULL: field f is not deferred. */
typedef struct {
    float* const* param;            /* device array [m] */
    float* const* state;            /* Adagrad: the accumulators; SGD: NULL */
    unsigned char* const* last;
    const float* l2;                /* device array [m] */
} xdfm_opt_rows;
/* Brings the rows a batch is about to gather (X, cols, vocab as in xdfm_embed_gather_fwd; lin may be NULL) up to the
 * clock: one thread per (example, field, 16-byte chunk of the row), the first to reach a chunk claims it by an integer
 * compare-and-swap on the word of its `last` byte.  adagrad: 0 = SGD (eps unused), 1 = Adagrad. */
int xdfm_opt_catchup_rows(int adagrad, const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                          const xdfm_opt_rows* emb, const xdfm_opt_rows* lin, const xdfm_opt_clock* clk, double eps,
                          void* stream);
/* Brings every chunk of the tensors (all deferred: last[t] != NULL) up to the clock, then resets it (clock[1] += clock[0],
 * clock[0] = 0, every `last` byte 0). */
int xdfm_opt_flush(int adagrad, const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                   double eps, void* stream);
/* K7rd: the same three for RMSprop (the signatures above carry no alpha).  An untouched row with l2 > 0 evolves by
 * g' = 2 l2 p, v = fma(1 - alpha, g' g', alpha v), p = fma(-lr_t, g' / (sqrt(v) + eps), p); clock, `last` bytes, backlog and
 * cell are those of K7sd / K7gd, and so are the errors (plus alpha outside [0, 1)). */
int xdfm_rmsprop_step_deferred(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                               double lr, const double* lr_dev, double alpha, double eps, float* l2_ws, float* l2_value,
                               void* stream);
int xdfm_rmsprop_catchup_rows(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D,
                              const xdfm_opt_rows* emb, const xdfm_opt_rows* lin, const xdfm_opt_clock* clk, double alpha,
                              double eps, void* stream);
int xdfm_rmsprop_flush(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk, double alpha,
                       double eps, void* stream);
/* K7md: the same three for SGD with momentum.  An untouched row with l2 > 0 evolves by g' = 2 l2 p, buf = fma(mu, buf, g'),
 * d = nesterov ? fma(mu, buf, g') : buf, p = fma(-lr_t, d, p): buffer and weight both move in a replayed step.  Clock, `last`
 * bytes, backlog and cell are those of K7sd / K7gd, and so are the errors (plus mu outside (0, 1) and a missing or misaligned
 * state).  mu and nesterov are part of what a window of deferred steps assumes: flush before either changes.  A tensor
 * with l2 == 0 is not deferred (the sweep takes it: 16 bytes per parameter and step). */
int xdfm_sgdm_step_deferred(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk,
                            double lr, const double* lr_dev, double mu, int nesterov, float* l2_ws, float* l2_value, void* stream);
int xdfm_sgdm_catchup_rows(const float* X, long ldx, int B, const int* cols, const int* vocab, int m, int D, const xdfm_opt_rows* emb,
                           const xdfm_opt_rows* lin, const xdfm_opt_clock* clk, double mu, int nesterov, void* stream);
int xdfm_sgdm_flush(const xdfm_opt_tensor* tensors, unsigned char* const* last, int T, const xdfm_opt_clock* clk, double mu, int nesterov,
                    void* stream);

/* Test hook: compares the replay's short forms (csrc/adam_math.h) with the reference spellings ON THE DEVICE.
 * mode 0: square root, n = 2^32 bit patterns; 1: division by a step's constant, n = steps * 2^24 numerators; 2: general
 * division on n random operand pairs inside the guard; 3: whole replayed steps on n random chunks (zeros, denormals and
 * huge values included: the guard's fall-back).  out: device u64[3], zeroed by the caller = {cases compared, mismatches,
 * an encoding of one mismatching case}. */
int xdfm_adam_selftest(int mode, unsigned long long n, unsigned long long seed, double lr, double beta1, double beta2, double eps,
                       unsigned long long* out, void* stream);

/* ------------------------------------------------------------------ SFG heads of xdeepfm_pro: tiled vocabulary CE
 * replaces: the elementwise / reduction chains around the tile GEMMs of nn.Linear(K, V) + F.cross_entropy
 *           (deepctr/xdeepfm_pro/sfg_decoder.py:146-149, :277-283) when the vocabulary is walked in tiles.
 * z [rows][ld]: the logits of one vocabulary tile (T columns).  lse_update: (m[r], s[r]) <- online log-sum-exp of
 * (m[r], s[r]) and the row's T logits (m = -inf, s = 0 before the first tile).  softmax_grad: z <- exp(z - lse[r]) * g[r]
 * in place. */
int xdfm_vocab_lse_update(const float* z, long ld, int rows, int T, float* m, float* s, void* stream);
int xdfm_vocab_softmax_grad(float* z, long ld, int rows, int T, const float* lse, const float* g, void* stream);

/* The same cross-entropy without the logits in HBM (csrc/vocab_ce_x3.hip), for ALL sparse fields' heads over the same
 * hidden rows in one launch per pass: for heads of width K = 32 or 64 a 32 x 32 block of logits lives only in the
 * accumulators of one wave (f16x3 products: hi*hi + hi*lo + lo*hi on fp16 halves of power-of-two scaled operands, fp32
 * accumulation, base-2 exp / log).  Replaces, per sparse field, nn.Linear(K, V) + F.cross_entropy(reduction='none')
 * (deepctr/xdeepfm_pro/sfg_decoder.py:146-149, :277-283) and their autograd backward.  No float atomics: partial
 * results are merged in a fixed order, every row of dW / db is written once.
 *   supported       1 when K is handled and the f16x3 arithmetic is selected (option cin_math == 1), else 0: callers
 *                   then use the tiled path above.
 *   plan            host-side: fills V, vr, item0, blk0, ws_off of fields[0..F) (W, bias, dW, db are the caller's) and
 *                   the work items of the rows-stationary kernels (pass items == NULL to count); returns the number of
 *                   items, *ws_elems = floats of scratch, *n_blk = 128-row weight blocks of all fields.  The caller
 *                   copies both tables to the device.
 *   pack_hidden     hidden [R][K] fp32, contiguous -> `pack` (pack_elems(R, K) floats): MFMA fragments of H and H^T,
 *                   hi / lo halves, one power-of-two scale.  Once per step: every field's head reads the same rows.
 *   fwd             ce[f][r] = logsumexp_v(h_r.W_v + b_v) - (h_r.W_t + b_t), t = targets[f][r] (int64, clamped to
 *                   [0, V_f)); lse2 [F][rows_padded(R)] receives the base-2 log-sum-exp and
 *                   wmax [F] the bits of max|W_f|: both are inputs of the backward.
 *   pack_g          upstream gradients g [F][R] -> gpack (F * (4 + rows_padded(R)) floats): g scaled to fp16 range.
 *   bwd_h           dh[r][:] = sum_f [ sum_v g[f][r] softmax_f[r][v] W_f[v][:] - g[f][r] W_f[t][:] ]
 *   bwd_w           fields[f].dW [V_f][K], fields[f].db [V_f] = (g (softmax - onehot(target)))^T H, column sums
 *                   (either pointer may be NULL). */
typedef struct { const float* W; const float* bias; float* dW; float* db; long ws_off; int V, vr, item0, blk0; } xdfm_vce_field;
typedef struct { int field, sb0, sb1, range; } xdfm_vce_item;
int xdfm_vocab_ce_x3_supported(int K);
long xdfm_vocab_ce_pack_elems(int R, int K);
long xdfm_vocab_ce_rows_padded(int R);
long xdfm_vocab_ce_plan(int F, const int* V, int R, int K, xdfm_vce_field* fields, xdfm_vce_item* items, long max_items,
                        long* ws_elems, int* n_blk);
int xdfm_vocab_ce_pack_hidden(const float* hidden, long ldh, int R, int K, float* pack, void* stream);
int xdfm_vocab_ce_fwd(const float* pack, const float* hidden, long ldh, int R, int K, const xdfm_vce_field* fields, int F,
                      const xdfm_vce_item* items, long n_items, const long* targets, float* ws, float* ce, float* lse2,
                      unsigned* wmax, void* stream);
int xdfm_vocab_ce_pack_g(const float* g, int F, int R, float* gpack, void* stream);
int xdfm_vocab_ce_bwd_h(const float* pack, int R, int K, const xdfm_vce_field* fields, int F, const xdfm_vce_item* items, long n_items,
                        const long* targets, const float* g, const float* gpack, const float* lse2, unsigned* wmax, float* ws,
                        float* dh, long lddh, void* stream);
int xdfm_vocab_ce_bwd_w(const float* pack, int R, int K, const xdfm_vce_field* fields, int F, int n_blk, const long* targets,
                        const float* gpack, const float* lse2, const unsigned* wmax, void* stream);

/* The same five passes with the number of rows in use on the DEVICE (n_rows: one int32 in device memory, read by the
 * kernels; NULL = all R rows, which is what the entry points above pass).  R is then a capacity: the plan, pack_elems,
 * rows_padded, the workspaces and every row pitch ([F][R] targets / ce / g, [R][K] hidden / dh) come from R and never from
 * the count, so the launch sequence and every shape are the same for every count -- a captured train step replays with
 * whatever the batch holds.  Rows r >= *n_rows are absent: their hidden rows, targets and g are never read (they may hold
 * anything, NaN included), ce[f][r] = 0 and dh[r][:] = 0 exactly, and they add nothing to dW, db, lse2 or the operand
 * maxima.  A 512-row group of the rows-stationary kernels behind the count returns at once and the weights-stationary
 * kernel walks ceil(*n_rows / 32) row tiles, so absent rows cost no arithmetic.  *n_rows == 0 gives ce = 0, dh = 0, dW = 0,
 * db = 0; a count above R counts as R.  With *n_rows == R every output has the bits of the entry points above.
 * (fwd and fwd_n zero the padding of lse2 themselves: the caller need not clear it.) */
int xdfm_vocab_ce_pack_hidden_n(const float* hidden, long ldh, int R, int K, float* pack, const int* n_rows, void* stream);
int xdfm_vocab_ce_fwd_n(const float* pack, const float* hidden, long ldh, int R, int K, const xdfm_vce_field* fields, int F,
                        const xdfm_vce_item* items, long n_items, const long* targets, float* ws, float* ce, float* lse2,
                        unsigned* wmax, const int* n_rows, void* stream);
int xdfm_vocab_ce_pack_g_n(const float* g, int F, int R, float* gpack, const int* n_rows, void* stream);
int xdfm_vocab_ce_bwd_h_n(const float* pack, int R, int K, const xdfm_vce_field* fields, int F, const xdfm_vce_item* items, long n_items,
                          const long* targets, const float* g, const float* gpack, const float* lse2, unsigned* wmax, float* ws,
                          float* dh, long lddh, const int* n_rows, void* stream);
int xdfm_vocab_ce_bwd_w_n(const float* pack, int R, int K, const xdfm_vce_field* fields, int F, int n_blk, const long* targets,
                          const float* gpack, const float* lse2, const unsigned* wmax, const int* n_rows, void* stream);

/* ------------------------------------------------------------------ K11: positive-row compaction (csrc/compact.hip)
 * replaces: torch.nonzero(labels == 1) + three index_selects in front of the SFG decoder (the rows the reference's
 *           `ce_loss * positive_mask` zeroes, deepctr/xdeepfm_pro/sfg_decoder.py:262-293, left out of the decoder), whose
 *           row count reaches the host.  Every output here has the capacity B; the count stays on the device.
 *   X        [B][ldx] the model input (xcols columns in use); cols: DEVICE int32[F], the id column of each sparse field
 *   dnn_in   [B][ldd] decoder input rows, W floats each; y [B] labels (contiguous)
 *   positive_only   1: a row is selected when y[b] == 1; 0: every row is
 *   pos      [B] int32 out: the slot of row b (the number of selected rows before it: torch.nonzero's order) or -1
 *   n_rows   [1] int32 out; inv_n [1] = 1 / (n + 1e-8), or 1 / B when not positive_only
 *   valid    [B] 1 for slot < n, else 0;  d_rows [B][W] the selected rows, exact zeros behind them;  labels [B] likewise;
 *   targets  [F][B] int64: the ids (X truncated towards zero) of the selected rows, 0 behind them
 * One workgroup scans the labels (ballot + popcount + LDS, no atomics), a second launch moves the rows: every element of
 * every output is written exactly once.  bwd: d_dnn [B][W] (contiguous) = g[pos[b]][:] for a selected row, zeros otherwise
 * (plain stores; g [B][ldg] is the gradient of d_rows).  1 <= B <= 65536; 16-byte accesses when W, the row pitches and the
 * base addresses are multiples of 4 floats, single floats otherwise.  Arguments are validated before any device work. */
int xdfm_compact_rows_fwd(const float* X, long ldx, int xcols, const float* dnn_in, long ldd, const float* y, long B, int W,
                          const int* cols, int F, int positive_only, int* pos, int* n_rows, float* inv_n, float* valid,
                          float* d_rows, float* labels, long* targets, void* stream);
int xdfm_compact_rows_bwd(const float* g, long ldg, const int* pos, long B, int W, float* d_dnn, void* stream);
/* xdfm_compact_rows_fwd whose normaliser comes from a second label vector: count_y [n_count] (contiguous) are the labels of the
 * GLOBAL batch of a row-parallel step, of which y [B] is this rank's shard (the SFG loss divides by the positives of the
 * global batch, deepctr/xdeepfm_pro/sfg_decoder.py:262-268).  pos, n_rows, valid, d_rows, labels and targets come from y
 * exactly as above; inv_n [1] = 1 / (#{count_y == 1} + 1e-8), or 1 / n_count when not positive_only -- the bits
 * xdfm_compact_rows_fwd leaves when count_y are its labels.  Counted by the same one-workgroup scan (ballot + popcount, no
 * atomics, no further launch), so a captured step reads a new count from count_y at every replay.  n_count is independent of
 * B: 1 <= n_count <= 65536 * 1024.  count_y == NULL (n_count ignored): xdfm_compact_rows_fwd, bit for bit. */
int xdfm_compact_rows_fwd_n(const float* X, long ldx, int xcols, const float* dnn_in, long ldd, const float* y, long B, int W,
                            const int* cols, int F, int positive_only, const float* count_y, long n_count, int* pos, int* n_rows,
                            float* inv_n, float* valid, float* d_rows, float* labels, long* targets, void* stream);

/* ------------------------------------------------------------------ AutoDis of xdeepfm_pro (K10, csrc/autodis.hip)
 * replaces: the per-field Python loop of deepctr/xdeepfm_pro/autodis.py:99-125 (Linear(1,K), LeakyReLU(0.2), Linear(K,K),
 *           division by the field's temperature, softmax, matmul with the field's meta-embeddings, unsqueeze; then cat)
 *           and its autograd -- about 7 launches per field forward and twice that backward -- by one launch forward and
 *           one + one finish launch backward, for all F fields and B rows.  fp32 throughout, no float atomics: the
 *           parameter gradients are per-workgroup partials summed in a fixed order, so a repeated call gives the same bits.
 *   x       the dense values, x[b * ldx + f] (ldx >= F): the dense columns of a wider row-major matrix are read in place
 *   meta    [F][K][D]; temp [F]
 *   proj    DEVICE array of 4 * F device pointers, field-major: Linear(1,K).weight [K], .bias [K], Linear(K,K).weight
 *           [K][K] (stored [out][in]), .bias [K] -- the tensors stay where the state_dict keeps them
 *   out     [B][F * D], contiguous: out[b][f * D + d] = sum_k softmax(s / temp[f])_k meta[f][k][d]
 *   supported   1 for 1 <= K <= 32 and 1 <= D <= 64 (instances for K <= 8 / 16 / 32 with a run-time tail), else 0
 *   ws_elems    ceil(B / R) * F * (K * D + K * K + 3 * K + 1) floats with R = 256 rows per workgroup for K <= 16 and 128
 *               for K > 16; 0 outside the envelope
 *   bwd     g [B][ldg] (ldg >= F * D) is the gradient of out; only x is needed from the forward, which is recomputed.
 *           flags: bit 0 meta, 1 Linear(1,K).weight, 2 its bias, 3 Linear(K,K).weight, 4 its bias, 5 temp, 6 dx -- the
 *           gradients asked for.  grads (F * (K * D + K * K + 3 * K + 1) floats; needed with any of bits 0-5, as is ws)
 *           receives [F][K][D] dmeta | [F][K] dW1 | [F][K] db1 | [F][K][K] dW2 | [F][K] db2 | [F] dtemp; the parts of
 *           groups not asked for are left untouched.  dx [B][F], contiguous (needed with bit 6).
 * Any F >= 1 and B >= 1 with ceil(B / 128) * F < 2^31.  Arguments are validated before any device work. */
int xdfm_autodis_supported(int K, int D);
size_t xdfm_autodis_ws_elems(long B, int F, int K, int D);
int xdfm_autodis_fwd(const float* x, long ldx, long B, int F, int K, int D, const float* meta, const float* const* proj,
                     const float* temp, float* out, void* stream);
int xdfm_autodis_bwd(const float* x, long ldx, long B, int F, int K, int D, const float* meta, const float* const* proj,
                     const float* temp, const float* g, long ldg, int flags, float* ws, float* grads, float* dx, void* stream);

/* ------------------------------------------------------------------ K14: per-batch training metrics (csrc/metrics.hip)
 * replaces: the sklearn calls the reference's fit makes on host copies of every batch (deepctr/models/basemodel.py:264-269:
 *           log_loss, roc_auc_score, mean_squared_error, accuracy_score) -- on the device so far float64 ATen compositions
 *           (xdfm_amd/metrics.py *_device: a sort, two searchsorted and a dozen small kernels for the AUC, a dozen more
 *           for the logloss; the accuracy through a device-to-host copy and a sync) -- by two launches for any subset of
 *           the four: a main grid and a one-block finish.  No float atomics, no memset; a repeated call gives the same bits.
 *   y, p    [B] fp32 labels and predictions (contiguous); which: XDFM_METRIC_* bits, the metrics wanted
 *   out4    [4] doubles, slot order logloss | auc | mse | accuracy; a slot `which` does not name keeps its bits
 *   ws      xdfm_batch_metrics_ws_bytes(B, which) bytes, 8-byte aligned, the caller's.  Every cell the finish reads is written
 *           by the main grid first: the workspace may hold anything.  0 for a B or a `which` outside the supported range.
 * The values are those of xdfm_amd/metrics.py's numpy functions on (y, double(p)):
 *   auc       exact pair counting, no sort: C = sum over (i: y_i > 0.5, j: not) of 2 [p_i > p_j] + [p_i == p_j] in unsigned
 *             64-bit integers -- per-workgroup partials, added by the finish -- and auc = (C * 0.5) / (double(n_pos) *
 *             double(n_neg)): one IEEE division of exact operands, the bits of roc_auc_score (mid-ranks for ties).  A batch
 *             of one class gives 0 / 0 = NaN; so does any NaN in p.
 *   logloss   -(1 / B) sum (y log(pc) + (1 - y) log(1 - pc)), pc = clamp(double(p), 2^-52, 1 - 2^-52), in double, y as a
 *             double factor (soft labels allowed)
 *   mse       (1 / B) sum (double(y) - double(p))^2
 *             both sums: a thread adds its 2 rows of a 512-row tile in index order, the workgroup's threads are added by a
 *             fixed tree, the finish adds the tiles' partials by the same tree, then one division by B (the negation is
 *             exact).  Against a float64 sum in another order: |got - ref| <= (B + 4) * 2^-52 * ref.
 *   accuracy  #{(p > 0.5 ? 1 : 0) == y} / B: an integer count and one IEEE division, the bits of accuracy_score
 * 1 <= B <= 65536 (8 ranks x 8192 rows gathered).  XDFM_ERR_INVALID, before any device call: a NULL operand, B outside the
 * range, which == 0 or with bits above 15, a ws or out4 off 8-byte alignment. */
enum { XDFM_METRIC_LOGLOSS = 1, XDFM_METRIC_AUC = 2, XDFM_METRIC_MSE = 4, XDFM_METRIC_ACC = 8 };
size_t xdfm_batch_metrics_ws_bytes(int B, int which);
int xdfm_batch_metrics(const float* y, const float* p, int B, int which, void* ws, double* out4, void* stream);

/* ------------------------------------------------------------------ K14s: evaluation metrics, any row count (csrc/eval_metrics.hip)
 * replaces: the host tail of the reference's evaluate (deepctr/models/basemodel.py:311-352): all predictions copied to the
 *           host and widened to float64, then sklearn's log_loss / roc_auc_score / mean_squared_error / accuracy_score on one
 *           CPU thread -- by 2 launches without the AUC and 15 with it, for any subset of the four.  No float atomics, no
 *           memset, no allocation, no synchronisation, no host read; the launches and their shapes depend on (N, which) alone;
 *           a repeated call gives the same bits in all four slots.
 *   y, p, which, out4   as for xdfm_batch_metrics above, with the same four definitions (positives y > 0.5, the clamp of the
 *           logloss, a slot `which` does not name keeps its bits, one class or any NaN in p: auc = NaN)
 *   ws      xdfm_eval_metrics_ws_bytes(N, which) bytes, 8-byte aligned, the caller's; it may hold anything (every cell read
 *           is written first by an earlier launch of the call).  About 8 N + N / 4 bytes with the AUC, N / 100 without.
 *           0 for an N or a `which` outside the supported range.
 *   auc       exact, sort-based, in integers: scores become order-preserving u32 keys (-0.0 as +0.0), positives the key
 *             0xFFFFFFFF; an LSD radix sort of the keys alone (4 passes of 8 bits: histogram, scan, stable scatter); every
 *             positive takes a lower and an upper bound among the sorted non-positives; C = sum (lower + upper)
 *             = sum (2 #less + #equal) in unsigned 64-bit integers and auc = (C * 0.5) / (double(n_pos) * double(n_neg)):
 *             K14's formula, the bits of roc_auc_score.
 *   logloss, mse   K14's arithmetic per row.  Order of both sums: a thread adds its 16 rows t, t + 256, ... of a 4096-row tile
 *             in index order; the tile's 256 threads are added by a fixed tree (xor tree over a wave's 64 lanes, the 4 waves
 *             in order); the finish gives thread t the tiles t, t + 256, ... in index order and adds its 256 threads by the
 *             same tree; one division by N.  With T = ceil(N / 4096) tiles a term passes through at most
 *             d = 25 + ceil(T / 256) + 9 additions, so against numpy's pairwise float64 sum of the same terms
 *             (at most 27 + ceil(log2(max(N, 128) / 128)) additions deep):
 *             |got - ref| <= ((d + d_numpy) * 2^-53 + 6 * 2^-52) * ref  (tests/eval_metrics_ref.py derives it).
 *   accuracy, n_pos, NaN scores   64-bit integer counts per tile, added by the finish
 * 1 <= N <= 2^27: n_pos * n_neg <= 2^52 keeps C / 2 exact in a double.  XDFM_ERR_INVALID, before any device call: a NULL
 * operand, N outside the range, which == 0 or with bits above 15, a ws or out4 off 8-byte alignment. */
size_t xdfm_eval_metrics_ws_bytes(long N, int which);
int xdfm_eval_metrics(const float* y, const float* p, long N, int which, void* ws, double* out4, void* stream);

/* ------------------------------------------------------------------ K14w: sample-weighted evaluation metrics (csrc/eval_metrics_w.hip)
 * replaces: the host path of the weighted metrics (compile(weighted_metrics=...)): all predictions copied to the host, widened
 *           to float64, then xdfm_amd/metrics.py's weighted_log_loss / weighted_roc_auc_score / weighted_mean_squared_error /
 *           weighted_accuracy_score on one CPU thread -- by 2 launches without the AUC and 18 with it.  As K14s: no float
 *           atomics, no memset, no allocation, no synchronisation, no host read; the launches and their shapes depend on
 *           (N, which) alone; a repeated call gives the same bits in all four slots.
 *   y, p, which, out4   as for xdfm_eval_metrics
 *   w       [N] fp32 weights (contiguous), finite and >= 0 by the caller's contract (the host validates them).  A row with
 *           w == 0 is selected away, not multiplied: a NaN score on it is harmless.  Any other bit pattern (negative, NaN)
 *           counts as 0 too; weights never form an address, so the kernels write inside their arrays whatever w holds.
 *   ws      xdfm_eval_metrics_w_ws_bytes(N, which) bytes, 8-byte aligned, the caller's; it may hold anything.  In 8-byte cells,
 *           T = ceil(N / 4096): 7 T without the AUC (the documented prefix: nothing beyond it is touched then); with the AUC
 *           9 T + (N + 1) [cum, doubles] + 4 ceil(N / 2) [keys and weights, two buffers each] + 128 T + 128: about 24 N bytes.
 *           0 for an N or a `which` outside the supported range.
 * With wd = double(w) on the rows with w > 0, W = sum wd, Wpos / Wneg the same over the positives (y > 0.5) / the others (each
 * its own sum; Wneg is never W - Wpos):
 *   logloss   -(sum wd (y log(pc) + (1 - y) log(1 - pc))) / W, pc as in K14
 *   mse       (sum wd (y - p)^2) / W;      accuracy  (sum wd [(p > 0.5 ? 1 : 0) == y]) / W
 *   auc       (C * 0.5) / (Wpos * Wneg), C = sum over the positives i of wd_i (cum[lb_i] + cum[ub_i]): the keys of K14s and the
 *             weight as a payload go through K14s's stable radix sort (its histogram and scan kernels; the scatter stores key
 *             and weight at the rank the ballots give), cum[k] is the float64 exclusive prefix sum of the sorted non-positives'
 *             weights and lb / ub are K14s's bounds.  Stability fixes the order in which equal scores enter cum.  Order of cum:
 *             a tile's total in the tiled order; one workgroup scans the tiles' totals, a thread taking ceil(T / 256) consecutive
 *             tiles in order and the 256 runs by a Hillis-Steele scan; inside a tile 16 rows of 256 consecutive cells, each
 *             scanned over the lanes of its 4 waves, the waves and then the rows carried in order: at most
 *             d_cum = 37 + 2 ceil(T / 256) additions to a cell.
 *             NaN: a NaN score on a row with w > 0, Wpos * Wneg == 0.  W == 0: NaN in every slot asked for.
 *   sums      logloss, mse, accuracy, W, Wpos, Wneg and C in K14s's order (16 rows per thread, the fixed tree over the tile, the
 *             finish over the tiles: d = 25 + ceil(T / 256) + 9 additions), each term one product with wd (an fma into the
 *             sum).  tests/eval_metrics_w_ref.py derives the bounds against the float64 reference from these depths.
 * UNIT WEIGHTS (w == 1.0f everywhere) give the bits of xdfm_eval_metrics in all four slots: the terms, their order and the
 * divisions are K14s's, and W = N, Wpos, Wneg, cum[k] = k and C are then exact integers.  Weights that are multiples of 2^-k
 * with every sum below 2^53 * 2^-k make the accuracy and the AUC exact likewise.
 * 1 <= N <= 2^27.  XDFM_ERR_INVALID, before any device call: a NULL operand (w included), N outside the range, which == 0 or
 * with bits above 15, a ws or out4 off 8-byte alignment. */
size_t xdfm_eval_metrics_w_ws_bytes(long N, int which);
int xdfm_eval_metrics_w(const float* y, const float* p, const float* w, long N, int which, void* ws, double* out4, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XDFM_H */
