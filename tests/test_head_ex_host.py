"""CPU tests of the output head's link / loss pairs: the float64 references of head_ex_ref.py against torch's float64
autograd, ops.head_mode, the xdfm_head_fwd_ex / xdfm_head_bwd_ex symbols, signatures and refusals (argument validation
returns before any device call, as test_capi.py relies on), a regression model on the CPU, and the goldens under
tests/golden/regression/ with the two conditions their generator recorded."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_ex_ref as X
from head_ex_drivers import build_golden_model
from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "xdfm.h")
GOLDENS = ["reg_xdeepfm_mse", "reg_attn_mae", "bin_xdeepfm_mse"]


@pytest.mark.parametrize("mode", X.NEW_MODES, ids=X.mode_id)
def test_references_match_float64_autograd(mode):
    dl, dg = X.autograd_check(mode)
    print("%s: loss %.3g, g %.3g" % (X.mode_id(mode), dl, dg))
    assert dl <= 1e-12 and dg <= 1e-12


def test_reference_bounds_follow_the_roundings_of_the_kernel_comment():
    assert X.HEAD_G_ROUNDINGS == {(0, 1): 5, (0, 2): 3, (1, 1): 2, (1, 2): 1}
    p = np.array([0.25, 0.5, 2.0], dtype=np.float32)
    t = np.array([0.75, 0.5, -1.0], dtype=np.float32)
    for mode in X.NEW_MODES:
        g, b = X.g_ref(p, t, 2.0, mode)
        assert g[1] == 0.0 and b[1] <= 3 * 2.0 ** -149                   # p == t: sgn(0) = 0, a zero term, no slack but the denormal one
        assert np.all(b[[0, 2]] == X.HEAD_G_ROUNDINGS[mode] * 2.0 ** -24 * np.abs(g[[0, 2]]) + X.HEAD_G_ROUNDINGS[mode] / 2.0 * 2.0 ** -149)
    assert X.g_ref(p, t, 2.0, (1, 2))[0].tolist() == [-2.0, 0.0, 2.0]
    assert X.g_ref(p, t, 2.0, (1, 1))[0].tolist() == [-2.0, 0.0, 12.0]
    assert X.loss_ref(p, t, X.LOSS_MSE)[0] == 9.25 and X.loss_ref(p, t, X.LOSS_MAE)[0] == 3.5
    assert X.loss_ref(p, p, X.LOSS_MAE)[:2] == (0.0, 0.0)


def test_ex_cases_exercise_zero_residuals():
    for link in (X.LINK_SIGMOID, X.LINK_IDENTITY):
        c = X.make_ex_case("c0010", link)
        assert c["u"] is None and c["v"] is None and c["bias"] is None
        if link == X.LINK_IDENTITY:
            assert np.array_equal(c["y"][0::3], c["lin"][0::3]) and c["B"] >= 6
            assert (c["y"][1::3] != c["lin"][1::3]).all()
        else:
            assert (c["lin"][1::3] == 0).all() and (c["y"][1::3] == 0.5).all()
    assert set(X.EX_CASES) <= set(X.R.head_case_names()) and len(X.EX_CASES) == 12
    vec = {n: X.R.head_vectorised(*[X.R.HEAD_CASES[X.R.head_case_names().index(n)][i] for i in (2, 3, 7)]) for n in X.EX_CASES}
    assert vec["k64_k60_b1"] and not vec["k3_k1_b1"] and not vec["k64_k64_u_off"] and vec["k64_k4_b65536"] and not vec["k4000_k95_b16"]
    y = X.make_ex_case("k4_k68_b2047", X.LINK_IDENTITY)["y"]
    assert y.dtype == np.float32 and y.std() > 1.0 and not np.isin(y, (0.0, 1.0)).any()


def test_head_mode_table():
    from xdfm_amd import ops
    S, I = ops.LINK_SIGMOID, ops.LINK_IDENTITY
    assert (S, I, ops.LOSS_BCE, ops.LOSS_MSE, ops.LOSS_MAE) == (0, 1, 0, 1, 2)
    assert ops.head_mode("binary", F.binary_cross_entropy) == (S, ops.LOSS_BCE)
    assert ops.head_mode("binary", F.mse_loss) == (S, ops.LOSS_MSE)
    assert ops.head_mode("binary", F.l1_loss) == (S, ops.LOSS_MAE)
    assert ops.head_mode("regression", F.mse_loss) == (I, ops.LOSS_MSE)
    assert ops.head_mode("regression", F.l1_loss) == (I, ops.LOSS_MAE)
    assert ops.head_mode("regression", F.binary_cross_entropy) is None
    for loss in (F.binary_cross_entropy, F.mse_loss, F.l1_loss):
        assert ops.head_mode("multiclass", loss) is None
        assert ops.head_mode(None, loss) is None
    assert ops.head_mode("binary", [F.mse_loss]) is None
    assert ops.head_mode("binary", [F.binary_cross_entropy, F.mse_loss]) is None
    assert ops.head_mode("binary", F.smooth_l1_loss) is None
    assert ops.head_mode("binary", lambda p, t, reduction="sum": F.mse_loss(p, t, reduction=reduction)) is None   # matched by identity
    assert ops.head_mode("binary", None) is None


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_ex_symbols_and_signatures_match_the_header():
    from xdfm_amd import _lib
    lib = _lib.load()
    src = open(HEADER).read()
    assert re.search(r"enum\s*\{\s*XDFM_LINK_SIGMOID\s*=\s*0\s*,\s*XDFM_LINK_IDENTITY\s*=\s*1\s*\}", src)
    assert re.search(r"enum\s*\{\s*XDFM_LOSS_BCE\s*=\s*0\s*,\s*XDFM_LOSS_MSE\s*=\s*1\s*,\s*XDFM_LOSS_MAE\s*=\s*2\s*\}", src)
    assert re.search(r"#define\s+XDFM_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, src) and lib.xdfm_abi_version() == _lib.ABI_VERSION
    ctype = lambda a: ctypes.c_void_p if "*" in a else {"int": ctypes.c_int}[a.split()[0]]
    for name in ("xdfm_head_fwd", "xdfm_head_bwd"):
        assert hasattr(lib, name + "_ex")
        old, new = _header_args(name), _header_args(name + "_ex")
        strip = lambda a: a.rsplit(" ", 1)[0] if "*" not in a else a.rsplit("*", 1)[0] + "*"      # the type without the name
        assert [strip(a) for a in new] == [strip(a) for a in old[:-1]] + ["int", "int", "void*"], (old, new)
        assert new[-3:] == ["int link", "int loss", "void* stream"]
        res, args = _lib.SIGNATURES[name + "_ex"]
        assert res is ctypes.c_int and args == [ctype(a) for a in new]
        assert _lib.SIGNATURES[name][1] == [ctype(a) for a in old]


def _refusals():
    return [(2, 0, "link"), (-1, 1, "link"), (0, 3, "loss"), (1, -1, "loss"), (7, 9, "link"), (1, 0, "identity")]


@pytest.mark.parametrize("link,loss,word", _refusals())
def test_ex_entry_points_refuse_unknown_modes_before_any_device_call(link, loss, word):
    """Host buffers stand in for the device pointers: a call that got past the checks would launch on them, and on a
    machine without a GPU fail with another code.  The refusal names both values."""
    from xdfm_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for which in ("fwd", "bwd"):
        if which == "fwd":
            rc = lib.xdfm_head_fwd_ex(p, p, p, 4, p, p, 4, p, p, 2, p, p, p, link, loss, None)
        else:
            rc = lib.xdfm_head_bwd_ex(p, p, p, p, p, 4, p, p, 4, 2, p, p, p, p, p, link, loss, None)
        msg = lib.xdfm_last_error().decode()
        assert rc == 1, (which, rc, msg)
        assert "head_" + which in msg and word in msg, msg
        assert ("link=%d" % link) in msg and ("loss=%d" % loss) in msg, msg
        with pytest.raises(ValueError):
            _lib.check(rc, "head_%s_ex" % which)


def test_ex_entry_points_keep_the_old_argument_checks():
    from xdfm_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for link, loss in [(0, 0)] + X.NEW_MODES:
        assert lib.xdfm_head_fwd_ex(p, p, p, 4, p, p, 4, p, None, 2, p, p, p, link, loss, None) == 1        # y
        assert b"head_fwd: bad arguments" in lib.xdfm_last_error()
        assert lib.xdfm_head_fwd_ex(p, p, p, 4, p, p, 4, p, p, 0, p, p, p, link, loss, None) == 1           # B = 0
        assert lib.xdfm_head_fwd_ex(p, p, None, 4, p, p, 4, p, p, 2, p, p, p, link, loss, None) == 1        # u without wu
        assert b"head_fwd: bad operand shapes" in lib.xdfm_last_error()
        assert lib.xdfm_head_bwd_ex(p, p, None, p, p, 4, p, p, 4, 2, p, p, p, p, p, link, loss, None) == 1  # gloss
        assert b"head_bwd: bad arguments" in lib.xdfm_last_error()
        assert lib.xdfm_head_bwd_ex(p, p, p, p, p, 4, p, p, 4, 2, p, None, p, p, p, link, loss, None) == 1  # u without du
        assert b"head_bwd: bad operand shapes" in lib.xdfm_last_error()
        assert lib.xdfm_head_bwd_ex(p, p, p, p, p, 4000, p, p, 96, 2, p, p, p, p, p, link, loss, None) == 1
        assert b"too large" in lib.xdfm_last_error()
    assert lib.xdfm_head_ws_elems(384, 256) == 128 * 641 + 128


@pytest.mark.parametrize("loss,fn", [("mse", F.mse_loss), ("mae", F.l1_loss)])
def test_regression_model_builds_and_compiles_on_the_cpu(loss, fn):
    from xdfm_amd import ops
    g = load_golden("regression/reg_xdeepfm_mse")
    model = build_golden_model(g, "cpu")
    model.compile("adam", loss, metrics=["mse"])
    assert model.out.task == "regression" and model.loss_func is fn
    assert ops.head_mode(model.out.task, model.loss_func) == (ops.LINK_IDENTITY, {"mse": 1, "mae": 2}[loss])
    x, y = torch.from_numpy(g["X"][:6]), torch.from_numpy(g["y"][:6])
    assert model._fused_head(x, y) is None                                  # CPU tensors: the stock tail
    for k, v in model.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), g["init:" + k], err_msg="init " + k)


@pytest.mark.parametrize("name", GOLDENS)
def test_regression_goldens_reload_and_meet_their_generator_conditions(name):
    g = load_golden("regression/" + name)
    path = os.path.join(ROOT, "tests", "golden", "regression", name + ".npz")
    assert os.path.getsize(path) < 100 * 1024
    cls, task, loss = {"reg_xdeepfm_mse": ("xDeepFM", "regression", "mse"), "reg_attn_mae": ("xDeepFMAttention", "regression", "mae"),
                       "bin_xdeepfm_mse": ("xDeepFM", "binary", "mse")}[name]
    assert (str(g["cls"]), str(g["task"]), str(g["loss_name"])) == (cls, task, loss)
    B = int(g["B"])
    assert B == 6 and g["X"].shape == (3 * B, 6) and g["y"].shape[0] == 3 * B and int(g["emb_dim"]) == 4
    assert len(g["vocab"]) == 4 and g["vocab"].max() < 60 and int(g["n_dense"]) == 2
    assert tuple(g["dnn"]) == (8, 4) and tuple(g["cin"]) == (6, 4)
    keys = [k[3:] for k in g if k.startswith("s0:")]
    assert keys and all("init:" + k in g and "s3:" + k in g for k in keys)
    assert sorted(k[2:] for k in g if k.startswith("g:")) == sorted(k for k in keys)
    assert g["losses3"].shape == (3, 2) and g["pred_after"].shape == (3 * B, 1) and g["y_pred"].shape[0] == B
    assert all(np.isfinite(v).all() for k, v in g.items() if v.dtype.kind == "f")
    y = g["y"].reshape(-1)
    if task == "regression":
        assert y.std() > 0.5 and abs(y.mean() - 3.0) < 1.5 and not np.isin(y, (0.0, 1.0)).any()
    else:
        assert np.isin(y, (0.0, 1.0)).all() and 0 < g["y_pred"].min() and g["y_pred"].max() < 1
    # condition 1: the reference's own fp32 / fp64 difference uses at most half of every bar
    assert 0.0 <= float(g["bar_share_32_vs_64"]) <= 0.5
    np.testing.assert_allclose(g["losses3"], g["losses3_64"], rtol=1e-5)
    # condition 2 (mae): no residual close to the kink of |.|; checked again on the recorded step-1 prediction
    if loss == "mae":
        assert float(g["min_residual_required"]) == 1e-3 and float(g["min_abs_residual"]) > 1e-3
        assert np.abs(g["y_pred"].reshape(-1) - y[:B]).min() >= float(g["min_abs_residual"])
    # the recorded loss is the summed loss of the recorded prediction
    d = g["y_pred"].reshape(-1).astype(np.float64) - y[:B]
    want = (d * d).sum() if loss == "mse" else np.abs(d).sum()
    assert abs(float(g["loss"]) - want) <= 1e-5 * want and abs(float(g["losses3"][0, 0]) - want) <= 1e-5 * want
