"""Host-side checks (no GPU) of the static SFG route's plumbing: the K11 entry points and the K9 entry points with a
device-side row count are declared in include/xdfm.h, bound in `_lib.SIGNATURES` and exported by the library; the `_n`
entry points are the old ones plus one pointer; arguments are validated before any device work; the XDFM_PRO_GRAPH
switch parses; a CPU model keeps the dynamic route; a model driven by hand gives up graph replay with a warning; a batch
without a positive row gives the decoder zero gradients, not absent ones; the heads' kept state never evicts a table."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ["xdfm_compact_rows_fwd", "xdfm_compact_rows_bwd", "xdfm_vocab_ce_pack_hidden_n", "xdfm_vocab_ce_fwd_n",
       "xdfm_vocab_ce_pack_g_n", "xdfm_vocab_ce_bwd_h_n", "xdfm_vocab_ce_bwd_w_n"]


def _header():
    with open(os.path.join(ROOT, "include", "xdfm.h")) as f:
        return f.read()


def _lib():
    from xdfm_amd import _lib
    return _lib, _lib.load()


def test_new_symbols_in_header_binding_and_library():
    _l, lib = _lib()
    src = _header()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src)
        assert m, name + " is not declared in include/xdfm.h"
        assert name in _l.SIGNATURES, name
        res, args = _l.SIGNATURES[name]
        assert res is ctypes.c_int
        assert len(args) == m.group(1).count(",") + 1, "%s: %d bound arguments, header declares %d" % (
            name, len(args), m.group(1).count(",") + 1)
        assert getattr(lib, name) is not None
    assert lib.xdfm_abi_version() == _l.ABI_VERSION          # additions only: no existing signature changed


def test_counted_entry_points_are_the_old_ones_plus_one_pointer():
    _l, _ = _lib()
    for name in NEW[2:]:
        old = _l.SIGNATURES[name[:-2]][1]
        new = _l.SIGNATURES[name][1]
        assert new[:len(old) - 1] == old[:-1] and new[-2:] == [ctypes.c_void_p, ctypes.c_void_p], name
        assert len(new) == len(old) + 1


def test_compact_arguments_are_validated_before_device_work():
    _l, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(B=4, W=2, xcols=3, ldx=3, ldd=2, F=1, X=p, cols=p):
        return lib.xdfm_compact_rows_fwd(X, ldx, xcols, p, ldd, p, B, W, cols, F, 1, p, p, p, p, p, p, p, None)
    for kw in (dict(B=0), dict(B=65537), dict(W=0), dict(ldx=2), dict(ldd=1), dict(X=None), dict(cols=None), dict(F=-1)):
        assert fwd(**kw) == 1, kw
        assert b"compact_rows_fwd" in lib.xdfm_last_error()
    for args in ((None, 2, p, 4, 2, p), (p, 1, p, 4, 2, p), (p, 2, p, 0, 2, p), (p, 2, p, 65537, 2, p), (p, 2, p, 4, 2, None)):
        assert lib.xdfm_compact_rows_bwd(*args, None) == 1, args
        assert b"compact_rows_bwd" in lib.xdfm_last_error()
    with pytest.raises(ValueError):
        _l.check(fwd(B=0), "compact_rows_fwd")


@pytest.mark.parametrize("value,want", [(None, False), ("1", True), (" 1 ", True), ("0", False), (" 0 ", False), ("", False), ("2", True)])
def test_pro_graph_switch_parses(monkeypatch, value, want):
    from xdfm_amd import pro
    if value is None:
        monkeypatch.delenv("XDFM_PRO_GRAPH", raising=False)
    else:
        monkeypatch.setenv("XDFM_PRO_GRAPH", value)
    assert pro.pro_graph_enabled() is want


def test_cpu_model_keeps_the_dynamic_route(monkeypatch):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.xdeepfm_pro import xDeepFMProLight
    monkeypatch.setenv("XDFM_PRO_GRAPH", "1")
    cols = [SparseFeat("C%d" % i, 11 + i, 4) for i in range(3)] + [DenseFeat("I0", 1)]
    model = xDeepFMProLight(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(4,), sfg_hidden_units=(16, 32), device="cpu")
    model.compile("adam", "binary_crossentropy", metrics=[])
    assert not model._sfg_static() and model._optim_capturable is False
    assert model.metrics_names[:2] == ["loss", "sfg_loss"]


def test_graph_entry_keeps_the_steps_extra_and_log():
    from xdfm_amd import graphstep
    ent = graphstep._Entry(("key",))
    assert ent.extra is None and ent.log is None and ent.graph is None
    ent.extra, ent.log = torch.ones(()), ("sfg_loss", torch.zeros(()))
    assert ent.log[0] == "sfg_loss"


def _cpu_model():
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.xdeepfm_pro import xDeepFMProLight
    cols = [SparseFeat("C%d" % i, 11 + i, 4) for i in range(3)] + [DenseFeat("I0", 1)]
    model = xDeepFMProLight(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(4,), sfg_hidden_units=(16, 32), device="cpu")
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    return model


def test_hand_driven_model_gives_up_graph_replay_with_a_warning():
    """The SFG loss computed with gradients outside the model's own step: the caller's backward will bind the parameters'
    gradient accumulators to the caller's stream, so the model must not be captured afterwards.  Inside the own step, or
    without gradients, nothing changes."""
    import warnings
    model = _cpu_model()
    X, dnn_in, y = torch.zeros(5, 4), torch.randn(5, 13), torch.zeros(5, 1)      # no positive row: runs without a GPU
    model._optim_capturable = True                     # what compile() leaves on a GPU model whose heads the kernels serve
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad():
            model.compute_sfg_loss_fused(X, dnn_in, y)
        with model._own_step_scope():
            model.compute_sfg_loss_fused(X, dnn_in, y)
    assert model._optim_capturable is True and not caught
    with pytest.warns(UserWarning, match="driven by hand"):
        model.compute_sfg_loss_fused(X, dnn_in, y)
    assert model._optim_capturable is False
    with warnings.catch_warnings(record=True) as caught:      # said once: the flag is already down
        warnings.simplefilter("always")
        model.compute_sfg_loss_fused(X, dnn_in, y)
    assert not [w for w in caught if "driven by hand" in str(w.message)]
    model.compile("adam", "binary_crossentropy", metrics=[])
    assert model._optim_capturable is False            # a CPU model: compile() decides anew


def test_batch_without_positives_gives_the_decoder_zero_gradients():
    """The reference's masked loss (`ce_loss * positive_mask`) is a zero with zero-gradient TENSORS for every decoder
    parameter, so its optimizer steps them; the dynamic route must not leave them without a gradient."""
    model = _cpu_model()
    X, dnn_in, y = torch.zeros(5, 4), torch.randn(5, 13), torch.zeros(5, 1)
    total, info = model.compute_sfg_loss_fused(X, dnn_in, y)
    assert total.item() == 0.0 and info["sfg_loss"].item() == 0.0 and total.requires_grad
    total.backward()
    params = dict(model.sfg_decoder.named_parameters())
    assert params
    for k, p in params.items():
        assert p.grad is not None and p.grad.shape == p.shape and not p.grad.any(), k


def test_kept_heads_state_never_evicts(monkeypatch):
    """`ops.VocabHeadsState`: a captured step addresses the plan's items, the field table and the gradient tensors by raw
    pointer, so the state keeps every one it ever made -- also beyond any number of batch shapes, after the global plan
    cache was emptied and after the parameters moved."""
    from xdfm_amd import ops
    made = []

    def fake_plan(R, K, vocabs, dev):
        made.append(("plan", R))
        return (("fields", R), ("items", R, len(made)), 1, 1, 1)

    def fake_fields(plan, Ws, bs, dWs, dbs, dev):
        made.append(("table", plan[0][1]))
        return ("table", plan[0][1], len(made))
    monkeypatch.setattr(ops, "_vce_plan", fake_plan)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)      # no GPU here
    monkeypatch.setattr(ops, "_vce_fields", fake_fields)
    Ws, bs = [torch.zeros(7, 32), torch.zeros(9, 32)], [torch.zeros(7), torch.zeros(9)]
    state = ops.VocabHeadsState()
    dWs, dbs = state.grad_buffers(Ws, bs)
    assert state.grad_buffers(Ws, bs)[0] is dWs
    first = {}
    for R in range(1, 41):                               # 40 batch shapes
        first[R] = state.table((R, 32, (7, 9), "cpu"), Ws, bs, dWs, dbs, "cpu")
    n_made = len(made)
    for R in range(1, 41):
        plan, table = state.table((R, 32, (7, 9), "cpu"), Ws, bs, dWs, dbs, "cpu")
        assert plan is first[R][0] and table is first[R][1]
    assert len(made) == n_made and len(state.tables) == 40
    Ws2 = [torch.zeros(7, 32), torch.zeros(9, 32)]       # the parameters moved: new gradient tensors, the old ones stay owned
    dWs2, _ = state.grad_buffers(Ws2, bs)
    assert dWs2[0] is not dWs[0] and any(old[1][0] is dWs[0] for old in state.retired)
    state.table((1, 32, (7, 9), "cpu"), Ws2, bs, dWs2, dbs, "cpu")
    assert len(state.tables) == 41 and state.tables[((1, 32, (7, 9), "cpu"), state.current[(1, 32, (7, 9), "cpu")])][1] is not first[1][1]
    assert any(v[1] is first[1][1] for v in state.tables.values())
