"""ctypes binding of libxdfm_hip.so (the C ABI declared in include/xdfm.h).

There is deliberately no fallback: if the shared library is missing or lacks a symbol the
import of any op fails with an explicit error, and every op refuses non-CUDA tensors.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p

# torch must be imported BEFORE the library is dlopen'ed: the torch wheel bundles its own
# libamdhip64 and the process must end up with ONE HIP runtime (the one that owns torch's device
# context and streams).  Loaded first, torch's copy satisfies our DT_NEEDED by soname.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XDFM_LIB", os.path.join(_HERE, "libxdfm_hip.so"))

P = c_void_p
# name -> (restype, argtypes); mirrors include/xdfm.h one to one
SIGNATURES = {
    "xdfm_abi_version": (c_int, []),
    "xdfm_last_error": (c_char_p, []),
    "xdfm_device_count": (c_int, []),
    "xdfm_set_option": (c_int, [c_char_p, c_int]),
    "xdfm_get_option": (c_int, [c_char_p]),
    "xdfm_graph_node_census": (c_int, [P, P, P, P]),
    "xdfm_finish_batch_begin": (c_int, []),
    "xdfm_finish_batch_run": (c_int, [P]),
    "xdfm_finish_batch_active": (c_int, []),
    "xdfm_rider_begin": (c_int, []),
    "xdfm_rider_flush": (c_int, [P]),
    "xdfm_rider_pending": (c_int, []),
    "xdfm_rider_active": (c_int, []),
    "xdfm_finish": (c_int, [c_int, P, P, P, P, P, c_long, c_long, c_int, c_int, P]),
    "xdfm_embed_gather_fwd": (c_int, [P, c_long, c_int, P, P, P, P, c_int, c_int, P, P, c_int, P, P, P, P, P]),
    "xdfm_embed_gather_fwd_ld": (c_int, [P, c_long, c_int, P, P, P, P, c_int, c_int, P, P, c_int, P, P, c_long, c_int, P, P, P]),
    "xdfm_varlen_pool_fwd": (c_int, [P, c_long, c_int, P, P, c_int, c_int, c_int, P, P, c_long, c_int, P, P, P, P]),
    "xdfm_varlen_pool_bwd_ws_elems": (c_size_t, [c_long, c_int, c_int, c_int]),
    "xdfm_varlen_pool_bwd": (c_int, [P, c_long, c_int, P, P, c_int, c_int, c_int, P, P, c_long, c_int, P, c_long, P, P, P, P, P, P,
                                     P, P]),
    "xdfm_varlen_pool_bwd_rows_ws_elems": (c_size_t, [c_long, c_int, c_int, c_int]),
    "xdfm_varlen_pool_bwd_rows": (c_int, [P, c_long, c_int, P, P, c_int, c_int, c_int, P, c_long, P, c_long, P, P, P, P, P, P, P, P]),
    "xdfm_embed_scatter_bwd": (c_int, [P, c_long, c_int, P, P, c_int, c_int, P, c_int, P, P, P, P, P, P, P, P]),
    "xdfm_embed_scatter_bwd_marked": (c_int, [P, c_long, c_int, P, P, c_int, c_int, P, c_int, P, P, c_long, P, c_long,
                                              P, P, P, P, P, P]),
    "xdfm_cin_fwd_pack_elems": (c_size_t, [c_int, c_int, c_int]),
    "xdfm_cin_fwd_pack": (c_int, [P, c_int, c_int, c_int, P, P]),
    "xdfm_cin_pack_all_supported": (c_int, [c_int, c_int, c_int]),
    "xdfm_cin_pack_all": (c_int, [P, c_int, P]),
    "xdfm_cin_pack_defer": (c_int, [P, c_int, P]),
    "xdfm_cin_pack_flush": (c_int, [P]),
    "xdfm_cin_pack_pending": (c_int, []),
    "xdfm_cin_level_fwd": (c_int, [P, P, P, P, c_int, c_int, c_int, c_long, c_int, P, P]),
    "xdfm_cin_direct_sum": (c_int, [P, c_int, c_int, c_int, c_int, P, c_long, c_int, P]),
    "xdfm_cin_dout": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, P, c_int, c_long, c_int, c_int,
                              c_int, P, P, P]),
    "xdfm_cin_dout_ws_elems": (c_size_t, [c_int, c_int, c_int]),
    "xdfm_cin_dout_det": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, P, c_int, c_long, c_int, c_int,
                                  c_int, P, P, P, P]),
    "xdfm_cin_bwd_prep_ws_elems": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "xdfm_cin_bwd_prep": (c_int, [P, P, c_long, c_int, c_int, c_int, c_int, P, c_int, c_int, P, c_int, c_long, c_int, c_int, c_int, P, P, P,
                                  P, P, c_int, c_int, P, P, P]),
    "xdfm_cin_level_fwd_ex_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "xdfm_cin_level_fwd_ex": (c_int, [P, P, P, P, c_int, c_int, c_int, c_long, c_int, P, c_int, P, c_long, c_int, c_int, c_int,
                                      P, c_long, P]),
    "xdfm_cin_bwd_nodout_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "xdfm_cin_level_bwd_x_src": (c_int, [P, c_long, P, c_int, P, c_int, c_long, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int, c_int,
                                         c_int, c_long, P, P, c_int, P]),
    "xdfm_cin_level_bwd_w_prepared": (c_int, [P, P, P, c_int, c_int, c_int, c_long, P, P, P]),
    "xdfm_cin_bwd_pack_elems": (c_size_t, [c_int, c_int, c_int]),
    "xdfm_cin_bwd_pack": (c_int, [P, c_int, c_int, c_int, P, P]),
    "xdfm_cin_level_bwd_x": (c_int, [P, P, P, P, c_int, c_int, c_int, c_long, P, P, P]),
    "xdfm_cin_level_bwd_x_ex": (c_int, [P, P, P, P, c_int, c_int, c_int, c_long, P, P, c_int, P]),
    "xdfm_cin_bwd_x_is_folded": (c_int, [c_int, c_int, c_int, c_int]),
    "xdfm_cin_bwd_w_ws_elems": (c_size_t, [c_int, c_int, c_int, c_long]),
    "xdfm_cin_level_bwd_w": (c_int, [P, P, P, c_int, c_int, c_int, c_long, P, P, P]),
    "xdfm_cin_attn_theta_elems": (c_size_t, [c_int, c_int, c_int]),
    "xdfm_cin_attn_pool_fwd": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, c_float, P, P]),
    "xdfm_cin_attn_pool_bwd": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, c_float,
                                       P, P]),
    "xdfm_cin_attn_pool_bwd_ws_elems": (c_size_t, [c_int, c_int, c_int, c_int]),
    "xdfm_cin_attn_pool_bwd_det": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P, c_float,
                                           P, P]),
    "xdfm_cin_attn_dropout_mask": (c_int, [c_int, c_int, c_int, c_int, c_float, P, P, P]),
    "xdfm_head_ws_elems": (c_size_t, [c_int, c_int]),
    "xdfm_head_fwd": (c_int, [P, P, P, c_int, P, P, c_int, P, P, c_int, P, P, P, P]),
    "xdfm_head_bwd": (c_int, [P, P, P, P, P, c_int, P, P, c_int, c_int, P, P, P, P, P, P]),
    "xdfm_head_fwd_ex": (c_int, [P, P, P, c_int, P, P, c_int, P, P, c_int, P, P, P, c_int, c_int, P]),
    "xdfm_head_bwd_ex": (c_int, [P, P, P, P, P, c_int, P, P, c_int, c_int, P, P, P, P, P, c_int, c_int, P]),
    "xdfm_head_fwd_w": (c_int, [P, P, P, c_int, P, P, c_int, P, P, c_int, P, P, P, c_int, c_int, P, P]),
    "xdfm_head_bwd_w": (c_int, [P, P, P, P, P, c_int, P, P, c_int, c_int, P, P, P, P, P, c_int, c_int, P, P]),
    "xdfm_adam_step_ws_elems": (c_size_t, [c_int]),
    "xdfm_adam_step": (c_int, [P, c_int, c_double, c_double, c_double, c_double, P, P, P]),
    "xdfm_adam_step_lr": (c_int, [P, c_int, c_double, P, c_double, c_double, c_double, P, P, P]),
    "xdfm_adam_step_deferred": (c_int, [P, c_int, P, c_double, P, c_double, c_double, c_double, P, P, P]),
    "xdfm_adam_catchup_rows": (c_int, [P, c_long, c_int, P, P, c_int, c_int, P, P, P, c_double, c_double, c_double, P, P]),
    "xdfm_adam_apply_rows": (c_int, [P, c_long, c_int, P, P, c_int, c_int, P, P, P, c_double, c_double, c_double, P, P, P]),
    "xdfm_colaunch_adam_step": (c_int, [P, c_int, P, c_double, P, c_double, c_double, c_double, P, P,
                                        P, c_long, c_int, P, P, c_int, c_int, P, P, P, P]),
    "xdfm_adam_flush": (c_int, [P, c_int, P, c_double, c_double, c_double, P, P]),
    "xdfm_adam_selftest": (c_int, [c_int, ctypes.c_ulonglong, ctypes.c_ulonglong, c_double, c_double, c_double, c_double, P, P]),
    "xdfm_opt_step_ws_elems": (c_size_t, [c_int]),
    "xdfm_sgd_step": (c_int, [P, c_int, c_double, P, P, P, P]),
    "xdfm_adagrad_step": (c_int, [P, c_int, c_double, P, c_double, P, P, P]),
    "xdfm_sgd_step_deferred": (c_int, [P, P, c_int, P, c_double, P, P, P, P]),
    "xdfm_adagrad_step_deferred": (c_int, [P, P, c_int, P, c_double, P, c_double, P, P, P]),
    "xdfm_opt_catchup_rows": (c_int, [c_int, P, c_long, c_int, P, P, c_int, c_int, P, P, P, c_double, P]),
    "xdfm_opt_flush": (c_int, [c_int, P, P, c_int, P, c_double, P]),
    "xdfm_rmsprop_step": (c_int, [P, c_int, c_double, P, c_double, c_double, P, P, P]),
    "xdfm_rmsprop_step_deferred": (c_int, [P, P, c_int, P, c_double, P, c_double, c_double, P, P, P]),
    "xdfm_rmsprop_catchup_rows": (c_int, [P, c_long, c_int, P, P, c_int, c_int, P, P, P, c_double, c_double, P]),
    "xdfm_rmsprop_flush": (c_int, [P, P, c_int, P, c_double, c_double, P]),
    "xdfm_sgdm_step": (c_int, [P, c_int, c_double, P, c_double, c_int, P, P, P]),
    "xdfm_sgdm_step_deferred": (c_int, [P, P, c_int, P, c_double, P, c_double, c_int, P, P, P]),
    "xdfm_sgdm_catchup_rows": (c_int, [P, c_long, c_int, P, P, c_int, c_int, P, P, P, c_double, c_int, P]),
    "xdfm_sgdm_flush": (c_int, [P, P, c_int, P, c_double, c_int, P]),
    "xdfm_ftrl_step": (c_int, [P, c_int, c_double, P, c_double, c_double, c_double, P, P, P]),
    "xdfm_rowwise_adagrad_step": (c_int, [P, c_int, c_double, P, c_double, P, P, P]),
    "xdfm_vocab_lse_update": (c_int, [P, c_long, c_int, c_int, P, P, P]),
    "xdfm_vocab_softmax_grad": (c_int, [P, c_long, c_int, c_int, P, P, P]),
    "xdfm_vocab_ce_x3_supported": (c_int, [c_int]),
    "xdfm_vocab_ce_pack_elems": (c_long, [c_int, c_int]),
    "xdfm_vocab_ce_rows_padded": (c_long, [c_int]),
    "xdfm_vocab_ce_plan": (c_long, [c_int, P, c_int, c_int, P, P, c_long, P, P]),
    "xdfm_vocab_ce_pack_hidden": (c_int, [P, c_long, c_int, c_int, P, P]),
    "xdfm_vocab_ce_fwd": (c_int, [P, P, c_long, c_int, c_int, P, c_int, P, c_long, P, P, P, P, P, P]),
    "xdfm_vocab_ce_pack_g": (c_int, [P, c_int, c_int, P, P]),
    "xdfm_vocab_ce_bwd_h": (c_int, [P, c_int, c_int, P, c_int, P, c_long, P, P, P, P, P, P, P, c_long, P]),
    "xdfm_vocab_ce_bwd_w": (c_int, [P, c_int, c_int, P, c_int, c_int, P, P, P, P, P]),
    "xdfm_vocab_ce_pack_hidden_n": (c_int, [P, c_long, c_int, c_int, P, P, P]),
    "xdfm_vocab_ce_fwd_n": (c_int, [P, P, c_long, c_int, c_int, P, c_int, P, c_long, P, P, P, P, P, P, P]),
    "xdfm_vocab_ce_pack_g_n": (c_int, [P, c_int, c_int, P, P, P]),
    "xdfm_vocab_ce_bwd_h_n": (c_int, [P, c_int, c_int, P, c_int, P, c_long, P, P, P, P, P, P, P, c_long, P, P]),
    "xdfm_vocab_ce_bwd_w_n": (c_int, [P, c_int, c_int, P, c_int, c_int, P, P, P, P, P, P]),
    "xdfm_compact_rows_fwd": (c_int, [P, c_long, c_int, P, c_long, P, c_long, c_int, P, c_int, c_int, P, P, P, P, P, P, P, P]),
    "xdfm_compact_rows_bwd": (c_int, [P, c_long, P, c_long, c_int, P, P]),
    "xdfm_compact_rows_fwd_n": (c_int, [P, c_long, c_int, P, c_long, P, c_long, c_int, P, c_int, c_int, P, c_long, P, P, P, P, P, P, P, P]),
    "xdfm_autodis_supported": (c_int, [c_int, c_int]),
    "xdfm_autodis_ws_elems": (c_size_t, [c_long, c_int, c_int, c_int]),
    "xdfm_autodis_fwd": (c_int, [P, c_long, c_long, c_int, c_int, c_int, P, P, P, P, P]),
    "xdfm_autodis_bwd": (c_int, [P, c_long, c_long, c_int, c_int, c_int, P, P, P, P, c_long, c_int, P, P, P, P]),
    "xdfm_colsum_ws_elems": (c_size_t, [c_int]),
    "xdfm_colsum": (c_int, [P, c_long, c_int, c_long, P, P, P]),
    "xdfm_relu_bwd_colsum": (c_int, [P, P, c_long, c_int, c_long, c_long, P, P, P, P]),
    "xdfm_dense_supported": (c_int, [c_long, c_int, c_int]),
    "xdfm_dense_bwd_w_ws_elems": (c_size_t, [c_long, c_int, c_int]),
    "xdfm_dense_fwd": (c_int, [P, c_long, c_int, c_long, P, c_int, P, c_int, P, c_long, P]),
    "xdfm_dense_bwd_x": (c_int, [P, c_long, P, c_long, c_long, c_int, P, c_int, P, c_long, P]),
    "xdfm_dense_bwd_w": (c_int, [P, c_long, P, c_long, P, c_long, c_long, c_int, c_int, P, P, P, P]),
    "xdfm_dense_fwd_drop": (c_int, [P, c_long, c_int, c_long, P, c_int, P, c_int, P, c_long, c_float, P, c_int, c_long, P]),
    "xdfm_dense_bwd_x_drop": (c_int, [P, c_long, P, c_long, c_long, c_int, P, c_int, P, c_long, c_float, P]),
    "xdfm_dense_bwd_w_drop": (c_int, [P, c_long, P, c_long, P, c_long, c_long, c_int, c_int, P, P, P, c_float, P]),
    "xdfm_dense_dropout_mask": (c_int, [c_long, c_int, c_float, P, c_int, c_long, P, P]),
    "xdfm_dense_prelu_bwd_w_ws_elems": (c_size_t, [c_long, c_int, c_int]),
    "xdfm_dense_prelu_fwd": (c_int, [P, c_long, c_int, c_long, P, c_int, P, P, P, c_long, P, c_long, P]),
    "xdfm_dense_prelu_bwd_x": (c_int, [P, c_long, P, c_long, P, c_long, c_int, P, c_int, P, c_long, P]),
    "xdfm_dense_prelu_bwd_w": (c_int, [P, c_long, P, c_long, P, P, c_long, c_long, c_int, c_int, P, P, P, P, P]),
    "xdfm_prelu_ws_elems": (c_size_t, [c_long, c_int]),
    "xdfm_prelu_fwd": (c_int, [P, c_long, c_long, c_int, P, P, c_long, P]),
    "xdfm_prelu_bwd": (c_int, [P, c_long, P, c_long, c_long, c_int, P, P, c_long, P, P, P]),
    "xdfm_bn_row_block": (c_int, []),
    "xdfm_bn_ws_elems": (c_size_t, [c_long, c_int]),
    "xdfm_bn_fwd_train": (c_int, [P, c_long, c_long, c_int, P, P, c_float, c_float, c_int, P, c_long, P, P, P, P, P, P]),
    "xdfm_bn_fwd_eval": (c_int, [P, c_long, c_long, c_int, P, P, c_float, c_int, P, c_long, P, P, P]),
    "xdfm_bn_bwd": (c_int, [P, c_long, P, c_long, P, c_long, c_long, c_int, P, P, P, c_int, P, c_long, P, P, P, P]),
    "xdfm_bn_bwd_eval": (c_int, [P, c_long, P, c_long, P, c_long, c_long, c_int, P, P, P, c_int, P, c_long, P, P, P, P]),
    "xdfm_bn_stats": (c_int, [P, c_long, c_long, c_int, P, P, P]),
    "xdfm_bn_fwd_apply_sync": (c_int, [P, c_long, c_long, c_int, P, c_int, P, P, c_float, c_float, c_int, P, c_long, P, P, P, P, P]),
    "xdfm_bn_bwd_sums": (c_int, [P, c_long, P, c_long, P, c_long, c_long, c_int, P, P, c_int, P, P, P]),
    "xdfm_bn_bwd_apply_sync": (c_int, [P, c_long, P, c_long, P, c_long, c_long, c_long, c_int, P, c_int, c_int, c_long, P, P, P, c_int, P,
                                       c_long, P, P, P]),
    "xdfm_l2_reg_fwd": (c_int, [P, P, P, c_int, P, P, P]),
    "xdfm_l2_reg_bwd": (c_int, [P, P, P, c_int, P, P, P, c_int, P]),
    "xdfm_batch_metrics_ws_bytes": (c_size_t, [c_int, c_int]),
    "xdfm_batch_metrics": (c_int, [P, P, c_int, c_int, P, P, P]),
    "xdfm_eval_metrics_ws_bytes": (c_size_t, [c_long, c_int]),
    "xdfm_eval_metrics": (c_int, [P, P, c_long, c_int, P, P, P]),
    "xdfm_eval_metrics_w_ws_bytes": (c_size_t, [c_long, c_int]),
    "xdfm_eval_metrics_w": (c_int, [P, P, P, c_long, c_int, P, P, P]),
}

class PackJob(ctypes.Structure):
    """xdfm_cin_pack_job of include/xdfm.h"""
    _fields_ = [("W", c_void_p), ("H", c_int), ("Hp", c_int), ("m", c_int), ("fwd_pack", c_void_p), ("bwd_pack", c_void_p)]


class VarLenField(ctypes.Structure):
    """xdfm_varlen_field of include/xdfm.h"""
    _fields_ = [("table", c_void_p), ("lin", c_void_p), ("col", c_int), ("maxlen", c_int), ("len_col", c_int), ("combiner", c_int),
                ("vocab", c_int), ("reserved", c_int)]


class AdamTensor(ctypes.Structure):
    """xdfm_adam_tensor of include/xdfm.h"""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("step", c_void_p), ("numel", c_long), ("l2", ctypes.c_float), ("grad_marks", c_void_p), ("flags", c_int),
                ("last", c_void_p)]


class OptTensor(ctypes.Structure):
    """xdfm_opt_tensor of include/xdfm.h (SGD / Adagrad / RMSprop; `state` is the accumulator of the latter two)"""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("state", c_void_p), ("numel", c_long), ("l2", ctypes.c_float),
                ("grad_marks", c_void_p)]


class FtrlTensor(ctypes.Structure):
    """xdfm_ftrl_tensor of include/xdfm.h (FTRL-Proximal: two state arrays)"""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("z", c_void_p), ("n", c_void_p), ("numel", c_long), ("l2", ctypes.c_float),
                ("grad_marks", c_void_p)]


class RowwiseTensor(ctypes.Structure):
    """xdfm_rowwise_tensor of include/xdfm.h (row-wise Adagrad: `state` is [rows])"""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("state", c_void_p), ("rows", c_long), ("dim", c_int), ("l2", ctypes.c_float),
                ("grad_marks", c_void_p)]


class OptClock(ctypes.Structure):
    """xdfm_opt_clock of include/xdfm.h (deferred SGD / Adagrad / RMSprop)"""
    _fields_ = [("clock", c_void_p), ("rates", c_void_p), ("cap", c_int), ("backlog", c_void_p), ("cell", c_void_p)]


class OptRows(ctypes.Structure):
    """xdfm_opt_rows of include/xdfm.h (device pointer tables of one gather's fields)"""
    _fields_ = [("param", c_void_p), ("state", c_void_p), ("last", c_void_p), ("l2", c_void_p)]


class AdamClock(ctypes.Structure):
    """xdfm_adam_clock of include/xdfm.h"""
    _fields_ = [("clock", c_void_p), ("consts", c_void_p), ("cap", c_int)]


class AdamRows(ctypes.Structure):
    """xdfm_adam_rows of include/xdfm.h (device pointer tables of one gather's fields)"""
    _fields_ = [("param", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("last", c_void_p), ("l2", c_void_p),
                ("grad", c_void_p), ("marks", c_void_p)]


ABI_VERSION = 9
_lib = None


class XdfmError(RuntimeError):
    pass


def load():
    """dlopen the library once, bind every symbol of include/xdfm.h, check the ABI version."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XdfmError(
            "libxdfm_hip.so not found at %s -- build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback for the xDeepFM hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise XdfmError("libxdfm_hip.so at %s does not export %s (stale build?)" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    if lib.xdfm_abi_version() != ABI_VERSION:
        raise XdfmError("libxdfm_hip.so ABI %d != binding ABI %d" % (lib.xdfm_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().xdfm_last_error().decode("utf-8", "replace")
        if rc == 1:
            raise ValueError("xdfm %s: %s" % (what, msg))
        raise XdfmError("xdfm %s failed (code %d): %s" % (what, rc, msg))


def set_option(key, value):
    check(load().xdfm_set_option(key.encode(), int(value)), "set_option")


def get_option(key):
    return load().xdfm_get_option(key.encode())
