"""CPU: the RMSprop entry points (K7r / K7rd) are declared, bound and exported and validate their arguments before any device
work; the host class keeps torch.optim.RMSprop's layout and defaults; the rms_<case> goldens exist and the oracle with
torch.optim.RMSprop at the recorded rate reproduces them (no GPU compute)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_names, load_golden

T = torch.from_numpy
NEW = ("xdfm_rmsprop_step", "xdfm_rmsprop_step_deferred", "xdfm_rmsprop_catchup_rows", "xdfm_rmsprop_flush")
CASES = ("sum_small", "sum_c1", "x3_cin")


def test_new_symbols_are_declared_bound_and_exported():
    from xdfm_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), "include/xdfm.h lacks %s" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9          # additions only
    assert ctypes.sizeof(_lib.OptTensor) == 48
    assert [f[0] for f in _lib.OptTensor._fields_] == ["param", "grad", "state", "numel", "l2", "grad_marks"]
    # the existing signatures did not change
    assert len(_lib.SIGNATURES["xdfm_adagrad_step"][1]) == 8 and len(_lib.SIGNATURES["xdfm_sgd_step"][1]) == 7
    assert len(_lib.SIGNATURES["xdfm_opt_catchup_rows"][1]) == 13 and len(_lib.SIGNATURES["xdfm_opt_flush"][1]) == 7


def test_bad_arguments_are_refused_before_any_device_work():
    from xdfm_amd import _lib
    lib = _lib.load()
    one = (_lib.OptTensor * 1)()
    arr = ctypes.cast(one, ctypes.c_void_p)
    last = (ctypes.c_void_p * 1)()
    lasts = ctypes.cast(last, ctypes.c_void_p)
    buf = (ctypes.c_float * 8)()
    host = ctypes.c_void_p(ctypes.addressof(buf))            # a host address stands in for a device one: never dereferenced
    cell = (ctypes.c_ulonglong * 2)()
    clk = _lib.OptClock(ctypes.addressof(buf), ctypes.addressof(buf), 256, ctypes.addressof(cell), ctypes.addressof(cell) + 8)
    nan = float("nan")

    def refused(rc, text):
        msg = lib.xdfm_last_error()
        assert rc == 1 and text in msg, (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc, "rmsprop")

    # the sweep
    refused(lib.xdfm_rmsprop_step(None, 1, 0.01, None, 0.99, 1e-8, None, None, None), b"null pointer")
    refused(lib.xdfm_rmsprop_step(arr, 0, 0.01, None, 0.99, 1e-8, None, None, None), b"bad tensor count")
    refused(lib.xdfm_rmsprop_step(arr, -2, 0.01, None, 0.99, 1e-8, None, None, None), b"bad tensor count")
    refused(lib.xdfm_rmsprop_step(arr, 1, 0.01, None, 0.99, 0.0, None, None, None), b"bad hyper-parameters")       # eps <= 0
    refused(lib.xdfm_rmsprop_step(arr, 1, 0.01, None, 0.99, -1e-8, None, None, None), b"bad hyper-parameters")
    for alpha in (1.0, -0.1, 1.5, nan):
        refused(lib.xdfm_rmsprop_step(arr, 1, 0.01, None, alpha, 1e-8, None, None, None), b"outside [0, 1)")
    refused(lib.xdfm_rmsprop_step(arr, 1, 0.01, None, 0.99, 1e-8, None, None, None), b"null pointer")             # param / grad NULL
    one[0].param = one[0].grad = ctypes.addressof(buf)
    one[0].numel = 8
    refused(lib.xdfm_rmsprop_step(arr, 1, 0.01, None, 0.99, 1e-8, None, None, None), b"no state")
    one[0].state = ctypes.addressof(buf)
    refused(lib.xdfm_rmsprop_step(arr, 1, 0.01, None, 0.99, 1e-8, None, host, None), b"l2_value needs l2_ws")
    one[0].state = None
    # the deferred step
    refused(lib.xdfm_rmsprop_step_deferred(None, lasts, 1, ctypes.byref(clk), 0.01, None, 0.99, 1e-8, None, None, None), b"null pointer")
    refused(lib.xdfm_rmsprop_step_deferred(arr, None, 1, ctypes.byref(clk), 0.01, None, 0.99, 1e-8, None, None, None), b"null pointer")
    refused(lib.xdfm_rmsprop_step_deferred(arr, lasts, 0, ctypes.byref(clk), 0.01, None, 0.99, 1e-8, None, None, None), b"bad tensor count")
    refused(lib.xdfm_rmsprop_step_deferred(arr, lasts, 1, None, 0.01, None, 0.99, 1e-8, None, None, None), b"bad clock")
    refused(lib.xdfm_rmsprop_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 0.99, 0.0, None, None, None), b"bad hyper-parameters")
    refused(lib.xdfm_rmsprop_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 1.0, 1e-8, None, None, None), b"outside [0, 1)")
    refused(lib.xdfm_rmsprop_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 0.99, 1e-8, None, None, None), b"no state")
    refused(lib.xdfm_rmsprop_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 0.99, 1e-8, None, host, None), b"l2_value needs l2_ws")
    # the flush
    refused(lib.xdfm_rmsprop_flush(None, lasts, 1, ctypes.byref(clk), 0.99, 1e-8, None), b"null pointer")
    refused(lib.xdfm_rmsprop_flush(arr, lasts, 70000, ctypes.byref(clk), 0.99, 1e-8, None), b"bad tensor count")
    refused(lib.xdfm_rmsprop_flush(arr, lasts, 1, ctypes.byref(clk), 0.99, 0.0, None), b"bad hyper-parameters")
    refused(lib.xdfm_rmsprop_flush(arr, lasts, 1, ctypes.byref(clk), nan, 1e-8, None), b"outside [0, 1)")
    refused(lib.xdfm_rmsprop_flush(arr, lasts, 1, ctypes.byref(clk), 0.99, 1e-8, None), b"has no last")
    last[0] = ctypes.addressof(buf)
    refused(lib.xdfm_rmsprop_flush(arr, lasts, 1, ctypes.byref(clk), 0.99, 1e-8, None), b"no state")
    # the catch-up
    rows = _lib.OptRows(ctypes.addressof(buf), None, ctypes.addressof(buf), ctypes.addressof(buf))
    full = _lib.OptRows(ctypes.addressof(buf), ctypes.addressof(buf), ctypes.addressof(buf), ctypes.addressof(buf))
    args = (host, 4, 2, host, host, 1, 4)
    refused(lib.xdfm_rmsprop_catchup_rows(None, 4, 2, host, host, 1, 4, ctypes.byref(full), None, ctypes.byref(clk), 0.99, 1e-8, None),
            b"null pointer")
    refused(lib.xdfm_rmsprop_catchup_rows(*(args + (ctypes.byref(full), None, None, 0.99, 1e-8, None))), b"bad clock")
    refused(lib.xdfm_rmsprop_catchup_rows(*(args + (ctypes.byref(rows), None, ctypes.byref(clk), 0.99, 1e-8, None))), b"RMSprop needs state")
    refused(lib.xdfm_rmsprop_catchup_rows(*(args + (ctypes.byref(full), None, ctypes.byref(clk), 0.99, 0.0, None))), b"RMSprop needs state and eps > 0")
    refused(lib.xdfm_rmsprop_catchup_rows(*(args + (ctypes.byref(full), None, ctypes.byref(clk), 1.0, 1e-8, None))), b"outside [0, 1)")


def test_table_rmsprop_keeps_the_stock_layout_and_torchs_defaults():
    from xdfm_amd.optim import TableRMSprop
    assert issubclass(TableRMSprop, torch.optim.RMSprop) and TableRMSprop._KERNEL == "rmsprop"
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(4))]
    opt = TableRMSprop(ps)
    ref = torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(1))])
    g, gr = opt.param_groups[0], ref.param_groups[0]
    assert g["lr"] == 0.01 and g["alpha"] == 0.99 and g["eps"] == 1e-8
    assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in gr.items() if k != "params"}
    assert opt.table_step and opt.generation == 0 and opt.l2_value is None and opt.owns(ps)
    assert not opt.owns([torch.nn.Parameter(torch.zeros(1))])
    assert opt._plain(g)
    for key, val in (("momentum", 0.9), ("centered", True), ("capturable", True), ("foreach", True), ("eps", 0.0), ("alpha", 1.0)):
        assert not opt._plain(dict(g, **{key: val})), key
    for key, val in (("weight_decay", 0.1), ("maximize", True), ("differentiable", True), ("lr", torch.tensor(0.01))):
        saved, g[key] = g[key], val
        assert not opt._native(), key
        g[key] = saved
    # CPU parameters: the stock update (with an armed L2 term applied by hand), bit for bit
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    mine, stock = TableRMSprop(ps), torch.optim.RMSprop(qs)
    for step in range(3):
        for p, q in zip(ps, qs):
            p.grad = torch.full_like(p, 0.5 + step)
            q.grad = p.grad.clone()
        if step == 1:
            mine.arm_l2(ps[:1], [0.25])
            want = 0.25 * float(qs[0].detach().square().sum())
            qs[0].grad.add_(qs[0].detach(), alpha=0.5)
        mine.step()
        stock.step()
        assert (mine.l2_value is None) == (step != 1)
        if step == 1:
            assert abs(float(mine.l2_value) - want) <= 1e-6 * want
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
        sa, sb = mine.state[p], stock.state[q]
        assert sorted(sa.keys()) == sorted(sb.keys()) == ["square_avg", "step"]
        assert sa["step"].dtype == sb["step"].dtype and not sa["step"].is_cuda and float(sa["step"]) == 3.0
        assert torch.equal(sa["square_avg"], sb["square_avg"])
    gen = mine.generation
    stock.load_state_dict(mine.state_dict())             # interchangeable state, both ways
    mine.load_state_dict(stock.state_dict())
    assert mine.generation > gen                         # captured graphs that baked the old state are stale
    assert float(mine.state[ps[0]]["step"]) == 3.0 and len(opt.state) == 0


def test_cpu_model_compiles_the_stock_class():
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C1", 7, 4), SparseFeat("C2", 5, 4), DenseFeat("I1", 1)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), device="cpu")
    model.compile("rmsprop", "binary_crossentropy")
    assert type(model.optim) is torch.optim.RMSprop and model.optim.param_groups[0]["lr"] == 0.01
    assert not model._optim_capturable and model._l2_fusion() is None


def test_trainer_offers_rmsprop():
    src = open(os.path.join(ROOT, "xdeepfm-pytorch_amd", "xdftrain_amd.py")).read()
    m = re.search(r'"--optimizer".*?choices=\[([^\]]*)\]', src, flags=re.S)
    assert m and sorted(re.findall(r'"(\w+)"', m.group(1))) == ["adagrad", "adam", "rmsprop", "sgd"]


def test_rmsprop_goldens_exist_and_no_other_golden_test_picks_them_up():
    assert golden_names("rms_") == sorted("rms_" + c for c in CASES)
    assert golden_names("rms64_") == sorted("rms64_" + c for c in CASES)
    for prefix in ("optim_", "model_", "cin_", "attn_", "pro_"):
        assert not [n for n in golden_names(prefix) if "rms" in n]
    for c in CASES:
        g = load_golden("rms_" + c)
        assert str(g["optim_class"]) == "RMSprop" and str(g["optimizer"]) == "rmsprop" and str(g["base"]) == "model_" + c
        assert float(g["lr0"]) == 0.01 and float(g["alpha"]) == 0.99 and float(g["eps"]) == 1e-8 and float(g["lr"]) == 1e-4
        assert 0.0 < float(g["bar_share_32_vs_64"]) < 1.0


def _spec(g):
    vocab = [int(v) for v in g["vocab"]]
    from oracle import xdeepfm_oracle as orc
    return orc.Spec(["C%d" % (i + 1) for i in range(len(vocab))], vocab, ["I%d" % (i + 1) for i in range(int(g["n_dense"]))],
                    int(g["emb_dim"]), tuple(int(v) for v in g["cin"]), True, "relu", tuple(int(v) for v in g["dnn"]),
                    "sum", 4, True, True, 1, l2_reg_dnn=1e-5)


@pytest.mark.parametrize("case", CASES)
def test_oracle_with_torch_rmsprop_reproduces_the_golden(case):
    """The oracle's forward and backward, torch.optim.RMSprop at the recorded hyper-parameters, three steps as
    BaseModel.fit does them: losses rtol 2e-5, state rtol 1e-3 / atol 2e-5 against the reference's fp32 run, every element;
    the reference's own fp64 run (the companion file) lies within the same bars of its fp32 run."""
    from oracle import xdeepfm_oracle as orc
    g = load_golden("rms_" + case)
    assert str(g["cls"]) == "xDeepFM"
    base = load_golden(str(g["base"]))
    spec, B = _spec(g), int(g["B"])
    X, y = T(base["X"]), T(base["y"])
    st = {k[3:]: T(v.copy()).requires_grad_(True) for k, v in base.items() if k.startswith("s0:")}
    opt = torch.optim.RMSprop(list(st.values()), lr=float(g["lr"]), alpha=float(g["alpha"]), eps=float(g["eps"]))
    log = []
    for s in range(3):
        tot, dl, _ = orc.total_loss(X[s * B:(s + 1) * B], y[s * B:(s + 1) * B], st, spec)
        opt.zero_grad()
        tot.backward()
        opt.step()
        log.append((float(dl.item()), float(tot.item())))
    np.testing.assert_allclose(np.array(log), g["losses3"], rtol=2e-5)
    wide = load_golden("rms64_" + case)
    worst = 0.0
    for k, v in st.items():
        want = g["s3:" + k]
        if want.size:
            worst = max(worst, float((np.abs(v.detach().numpy() - want) / (2e-5 + 1e-3 * np.abs(want))).max()))
        np.testing.assert_allclose(v.detach().numpy(), want, rtol=1e-3, atol=2e-5, err_msg=k)
        s64 = want.astype(np.float64) + wide["s3_64_minus_s3:" + k].astype(np.float64)
        np.testing.assert_allclose(want, s64, rtol=1e-3, atol=2e-5, err_msg="fp32 against fp64 reference run: " + k)
    print("%s: oracle + torch.optim.RMSprop against the golden, worst share of the bar %.4f" % (case, worst))
