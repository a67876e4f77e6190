"""CPU tests of example weights: the xdfm_head_fwd_w / xdfm_head_bwd_w symbols, signatures and refusals (argument
validation returns before any device call), the float64 reference of head_w_ref.py against torch's float64 autograd and
against the unweighted head on a row-repeated batch, the weight-vector builder of fit(), the stock (CPU) tail of
train_on_batch and the trainer's --class_weight."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import head_ex_ref as X
import head_w_ref as W
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "xdfm.h")


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_w_symbols_and_signatures_match_the_header():
    from xdfm_amd import _lib
    lib = _lib.load()
    assert re.search(r"#define\s+XDFM_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, open(HEADER).read()) and lib.xdfm_abi_version() == _lib.ABI_VERSION
    ctype = lambda a: ctypes.c_void_p if "*" in a else {"int": ctypes.c_int}[a.split()[0]]
    strip = lambda a: a.rsplit(" ", 1)[0] if "*" not in a else a.rsplit("*", 1)[0] + "*"      # the type without the name
    for name in ("xdfm_head_fwd", "xdfm_head_bwd"):
        assert hasattr(lib, name + "_w")
        ex, new = _header_args(name + "_ex"), _header_args(name + "_w")
        assert [strip(a) for a in new] == [strip(a) for a in ex[:-1]] + ["const float*", "void*"], (ex, new)
        assert new[-2:] == ["const float* w", "void* stream"]
        res, args = _lib.SIGNATURES[name + "_w"]
        assert res is ctypes.c_int and args == [ctype(a) for a in new]
        assert _lib.SIGNATURES[name + "_ex"][1] == [ctype(a) for a in ex]               # untouched


def _host_ptrs():
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(p.value + 2)                 # two bytes past a float: not 4-byte aligned
    return buf, p, off


def test_w_entry_points_refuse_a_misaligned_weight_pointer_before_any_device_call():
    """Host buffers stand in for the device pointers: a call that got past the checks would launch on them, and on a
    machine without a GPU fail with another code."""
    from xdfm_amd import _lib
    lib = _lib.load()
    buf, p, off = _host_ptrs()
    for link, loss in W.ALL_MODES:
        rc = lib.xdfm_head_fwd_w(p, p, p, 4, p, p, 4, p, p, 2, p, p, p, link, loss, off, None)
        msg = lib.xdfm_last_error().decode()
        assert rc == 1 and "head_fwd_w" in msg and re.search(r"\bw=", msg) and "aligned" in msg, (rc, msg)
        rc = lib.xdfm_head_bwd_w(p, p, p, p, p, 4, p, p, 4, 2, p, p, p, p, p, link, loss, off, None)
        msg = lib.xdfm_last_error().decode()
        assert rc == 1 and "head_bwd_w" in msg and re.search(r"\bw=", msg) and "aligned" in msg, (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc, "head_bwd_w")


@pytest.mark.parametrize("with_w", [False, True], ids=["w_null", "w_given"])
def test_w_entry_points_refuse_whatever_ex_refuses(with_w):
    from xdfm_amd import _lib
    lib = _lib.load()
    buf, p, _ = _host_ptrs()
    w = p if with_w else None
    for link, loss, word in [(2, 0, "link"), (-1, 1, "link"), (0, 3, "loss"), (1, -1, "loss"), (1, 0, "identity")]:
        rc = lib.xdfm_head_fwd_w(p, p, p, 4, p, p, 4, p, p, 2, p, p, p, link, loss, w, None)
        msg = lib.xdfm_last_error().decode()
        assert rc == 1 and "head_fwd" in msg and word in msg and ("link=%d" % link) in msg and ("loss=%d" % loss) in msg, msg
        rc = lib.xdfm_head_bwd_w(p, p, p, p, p, 4, p, p, 4, 2, p, p, p, p, p, link, loss, w, None)
        msg = lib.xdfm_last_error().decode()
        assert rc == 1 and "head_bwd" in msg and word in msg and ("link=%d" % link) in msg and ("loss=%d" % loss) in msg, msg
    for link, loss in W.ALL_MODES:
        assert lib.xdfm_head_fwd_w(p, p, p, 4, p, p, 4, p, None, 2, p, p, p, link, loss, w, None) == 1        # y
        assert b"head_fwd: bad arguments" in lib.xdfm_last_error()
        assert lib.xdfm_head_fwd_w(p, p, p, 4, p, p, 4, p, p, 0, p, p, p, link, loss, w, None) == 1           # B = 0
        assert lib.xdfm_head_fwd_w(p, p, None, 4, p, p, 4, p, p, 2, p, p, p, link, loss, w, None) == 1        # u without wu
        assert b"head_fwd: bad operand shapes" in lib.xdfm_last_error()
        assert lib.xdfm_head_bwd_w(p, p, None, p, p, 4, p, p, 4, 2, p, p, p, p, p, link, loss, w, None) == 1  # gloss
        assert b"head_bwd: bad arguments" in lib.xdfm_last_error()
        assert lib.xdfm_head_bwd_w(p, p, p, p, p, 4, p, p, 4, 2, p, None, p, p, p, link, loss, w, None) == 1  # u without du
        assert b"head_bwd: bad operand shapes" in lib.xdfm_last_error()
        assert lib.xdfm_head_bwd_w(p, p, p, p, p, 4000, p, p, 96, 2, p, p, p, p, p, link, loss, w, None) == 1
        assert b"too large" in lib.xdfm_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", W.ALL_MODES, ids=W.mode_id)
def test_reference_matches_float64_autograd_of_the_weighted_sum(mode):
    errs = W.autograd_check_w(mode)
    print("%s: loss %.3g, g %.3g, dwu %.3g, dbias %.3g" % ((W.mode_id(mode),) + errs))
    assert all(e <= 1e-12 for e in errs)


@pytest.mark.parametrize("mode", W.ALL_MODES, ids=W.mode_id)
def test_integer_weights_equal_the_unweighted_reference_on_repeated_rows(mode):
    c, _ = W.make_w_case((37, 8, 32, True), mode[0])
    w = np.random.default_rng(5).integers(0, 4, 37).astype(np.float32)
    assert set(w.tolist()) == {0.0, 1.0, 2.0, 3.0}
    a = W.head_w64(c, w, mode)
    rc, idx = W.repeat_rows(c, w)
    assert rc["B"] == int(w.sum()) and rc["u"].shape == (rc["B"], 8)
    b = W.head_w64(rc, None, mode)
    rel = lambda x, y: float(np.abs(np.asarray(x) - np.asarray(y)).max()) / max(float(np.abs(np.asarray(y)).max()), 1.0)
    for k in ("loss", "dwu", "dwv", "dbias"):
        assert rel(a[k], b[k]) <= 1e-13, k
    np.testing.assert_allclose(w[idx] * b["g"], a["g"][idx], rtol=1e-14, atol=0)
    assert (a["g"][w == 0] == 0).all() and (a["du"][w == 0] == 0).all()


def test_bounds_carry_one_more_rounding_than_the_unweighted_ones():
    assert W.G_ROUNDINGS == {(0, 0): 4, (0, 1): 5, (0, 2): 3, (1, 1): 2, (1, 2): 1}
    p = np.array([0.25, 0.5, 2.0], dtype=np.float32)
    t = np.array([0.75, 0.5, -1.0], dtype=np.float32)
    w = np.array([2.0, 3.0, 0.0], dtype=np.float32)
    for mode in X.NEW_MODES:
        g, b = W.g_w_ref(p, t, w, 2.0, mode)
        g0, _ = X.g_ref(p, t, 2.0, mode)
        assert np.array_equal(g, w * g0)
        k = X.HEAD_G_ROUNDINGS[mode] + 1
        assert b[0] == k * 2.0 ** -24 * abs(g[0]) + k / 2.0 * 2.0 ** -149
        assert g[2] == 0.0 and b[2] <= 3 * 2.0 ** -149                   # w = 0: nothing but the denormal slack
    l, lb = W.loss_w_ref(p, t, w, X.LOSS_MSE)
    assert l == 2.0 * 0.25 and lb == float(X.R.gamma(3 + 3 + 1)) * 0.5 + 3 * (1.0 + 3.0) * 2.0 ** -149
    l, lb = W.loss_w_ref(p, t, w, X.LOSS_MAE)
    assert l == 1.0 and lb == float(X.R.gamma(3 + 1 + 1)) * 1.0 + 3 * 4.0 * 2.0 ** -149
    ones = np.ones(3, dtype=np.float32)
    assert W.loss_w_ref(p, t, ones, X.LOSS_MSE)[0] == X.loss_ref(p, t, X.LOSS_MSE)[0]
    assert W.loss_w_ref(p, t, ones, X.LOSS_MSE)[1] > X.loss_ref(p, t, X.LOSS_MSE)[1]
    pb = np.array([0.25, 0.5], dtype=np.float32)
    tb = np.array([1.0, 0.0], dtype=np.float32)
    l, lb = W.loss_w_ref(pb, tb, np.ones(2, dtype=np.float32), X.LOSS_BCE)
    l0, lb0, _ = X.R.head_loss_ref(pb, tb)
    assert l == l0 and lb0 < lb < 1.5 * lb0 + 1e-30


def test_cases_cover_both_row_paths_and_every_sweep_edge():
    assert len(W.W_CASES) == 30 and {c[0] for c in W.W_CASES} == {1, 5, 513, 2049, 4100}
    assert W.w_vectorised(8, 32) and not W.w_vectorised(7, 0) and not W.w_vectorised(0, 516)
    for case in [(5, 8, 32, True), (4100, 0, 516, False)]:
        for link in (0, 1):
            c, w = W.make_w_case(case, link)
            assert w.dtype == np.float32 and w.shape == (case[0],) and w.min() == 0.0 and 0 < w.max() <= 4.0
            assert (c["lin"] is not None) == case[3] and (c["bias"] is not None) == case[3]
        for loss in (X.LOSS_MSE, X.LOSS_MAE):
            c, w = W.make_w_case(case, X.LINK_IDENTITY, exact=True)
            W.assert_exact_family(c, w, loss)
            assert set(np.unique(w).tolist()) <= {0.0, 1.0, 2.0, 3.0}
    c, w = W.make_w_case((4100, 0, 516, True), X.LINK_IDENTITY, exact=True)
    c["wv"] = c["wv"] * np.float32(2.0 ** 12)
    with pytest.raises(AssertionError):
        W.assert_exact_family(c, w, X.LOSS_MSE)


# ---------------------------------------------------------------------------------------------------------------------
# the weight vector of fit()
# ---------------------------------------------------------------------------------------------------------------------
def test_example_weights_shapes_and_products():
    from xdfm_amd.models import example_weights
    y = np.array([0, 1, 1, 0, 1], dtype=np.float32)
    assert example_weights(y) is None and example_weights(y.reshape(-1, 1), None, None, "regression") is None
    sw = np.array([1, 2, 0, 0.5, 4])
    for given in (sw, sw.reshape(-1, 1), sw.astype(np.float32), sw.tolist()):
        w = example_weights(y, given)
        assert w.dtype == np.float32 and w.shape == (5,) and w.flags["C_CONTIGUOUS"] and w.tolist() == sw.tolist()
    for labels in (y, y.reshape(-1, 1), y.astype(np.int64)):
        w = example_weights(labels, None, {0: 0.25, 1: 3.0})
        assert w.dtype == np.float32 and w.tolist() == [0.25, 3.0, 3.0, 0.25, 3.0]
    w = example_weights(y, sw, {0: 0.25, 1: 3.0})
    assert w.tolist() == (sw.astype(np.float32) * np.array([0.25, 3.0, 3.0, 0.25, 3.0], dtype=np.float32)).tolist()
    assert example_weights(y * 2.5, sw, None, "regression").tolist() == sw.tolist()       # sample_weight needs no binary task


@pytest.mark.parametrize("bad", [[1, -1, 1, 1, 1], [1, float("nan"), 1, 1, 1], [1, float("inf"), 1, 1, 1], [1, 1, 1, 1],
                                 [1, 1, 1, 1, 1, 1], np.ones((5, 2)), np.ones((1, 5)), ["a"] * 5, [1e39, 1, 1, 1, 1]],
                         ids=["negative", "nan", "inf", "short", "long", "n_by_2", "row", "strings", "overflows_fp32"])
def test_example_weights_reject_bad_sample_weight(bad):
    from xdfm_amd.models import example_weights
    with pytest.raises(ValueError, match="sample_weight"):
        example_weights(np.array([0, 1, 1, 0, 1], dtype=np.float32), bad)


def test_example_weights_reject_bad_class_weight():
    from xdfm_amd.models import example_weights
    y = np.array([0, 1, 1, 0, 1], dtype=np.float32)
    cw = {0: 1.0, 1: 4.0}
    with pytest.raises(ValueError, match="class_weight"):
        example_weights(y, None, cw, "regression")
    with pytest.raises(ValueError, match="class_weight"):
        example_weights(np.array([0, 1, 0.5, 0, 1]), None, cw)                 # a soft label
    with pytest.raises(ValueError, match="class_weight"):
        example_weights(np.array([0, 1, 2, 0, 1]), None, cw)                   # a third class
    for bad in ({0: 1.0}, {0: 1.0, 1: 2.0, 2: 3.0}, {0: -1.0, 1: 1.0}, {0: 1.0, 1: float("nan")}, [1.0, 4.0]):
        with pytest.raises(ValueError, match="class_weight"):
            example_weights(y, None, bad)


def test_example_weights_stay_aligned_under_a_permutation_and_a_split():
    """fit() cuts the weights like y (validation_split) and gathers both by the same `order`: row i of every batch
    carries the weight of the example whose label it carries."""
    from xdfm_amd.models import BaseModel, example_weights
    n, split_at = 23, int(23 * (1.0 - 0.3))
    r = np.random.default_rng(3)
    y = (r.uniform(size=n) < 0.5).astype(np.float32)
    sw = (np.arange(n) + 1).astype(np.float32)                                   # the weight names the example
    w = example_weights(y, sw, {0: 1.0, 1: 100.0})
    assert w.tolist() == (sw * np.where(y == 1, 100.0, 1.0)).tolist()
    w_tr, y_tr = torch.from_numpy(w[:split_at]), torch.from_numpy(y[:split_at])
    order = torch.from_numpy(r.permutation(split_at))
    for start in range(0, split_at, 5):
        wb = BaseModel._rows(w_tr, order, start, start + 5)
        yb = BaseModel._rows(y_tr, order, start, start + 5)
        ids = order[start:start + 5].numpy()
        assert wb.tolist() == (sw[ids] * np.where(y[ids] == 1, 100.0, 1.0)).tolist() and yb.tolist() == y[ids].tolist()
        assert ids.max() < split_at


# ---------------------------------------------------------------------------------------------------------------------
# the model's step on the CPU (stock tail) and the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_model(cls_name="xDeepFM", task="binary", loss="binary_crossentropy", seed=7):
    from deepctr import models
    from deepctr.inputs import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % (i + 1), 11, 4) for i in range(3)] + [DenseFeat("I1", 1)]
    m = getattr(models, cls_name)(cols, cols, dnn_hidden_units=(8, 4), cin_layer_size=(6, 4), task=task, device="cpu", seed=seed)
    m.compile("sgd", loss)
    return m


def test_fit_checks_the_weights_once_on_the_host_before_any_device_work():
    r = np.random.default_rng(1)
    X_ = np.concatenate([r.integers(0, 11, (24, 3)), r.standard_normal((24, 1))], axis=1).astype(np.float32)
    y = (r.uniform(size=(24, 1)) < 0.5).astype(np.float32)
    x = [X_[:, i] for i in range(4)]
    c = _cpu_model()
    with pytest.raises(ValueError, match="sample_weight"):
        c.fit(x, y, batch_size=8, epochs=1, verbose=0, sample_weight=np.ones(23))
    with pytest.raises(ValueError, match="sample_weight"):
        c.fit(x, y, batch_size=8, epochs=1, verbose=0, sample_weight=-np.ones(24))
    with pytest.raises(ValueError, match="class_weight"):
        c.fit(x, y * 0.5, batch_size=8, epochs=1, verbose=0, class_weight={0: 1.0, 1: 2.0})
    with pytest.raises(ValueError, match="class_weight"):
        _cpu_model(task="regression", loss="mse").fit(x, y, batch_size=8, epochs=1, verbose=0, class_weight={0: 1.0, 1: 2.0})
    with pytest.raises(ValueError, match="sample_weight"):
        c.train_on_batch(torch.from_numpy(X_), torch.from_numpy(y), torch.ones(5))


def test_stock_tail_weights_the_unreduced_loss():
    """BaseModel._loss_forward without a native head (here: a model without `head_inputs`, on the CPU): the weighted sum
    of loss_func(..., reduction='none')."""
    import torch.nn.functional as F
    from xdfm_amd.models import BaseModel

    class Tail(BaseModel):
        def forward(self, x):
            return torch.sigmoid(x[:, :1] * 0.5)

    m = Tail.__new__(Tail)
    torch.nn.Module.__init__(m)
    m.loss_func = F.binary_cross_entropy
    x = torch.tensor([[0.5], [-1.0], [2.0], [0.0]])
    y = torch.tensor([[1.0], [0.0], [0.0], [1.0]])
    w = torch.tensor([0.0, 1.0, 2.5, 3.0])
    pred, loss = m._loss_forward(x, y, w)
    want = (w.double() * F.binary_cross_entropy(pred.double(), y.reshape(-1).double(), reduction="none")).sum()
    assert abs(loss.item() - want.item()) <= 1e-6 * want.item()
    _, plain = m._loss_forward(x, y)
    assert abs(plain.item() - F.binary_cross_entropy(pred, y.reshape(-1), reduction="sum").item()) <= 1e-6
    _, col = m._loss_forward(x, y, w.reshape(-1, 1))
    assert col.item() == loss.item()


def test_pro_models_refuse_a_weight():
    import inspect
    from xdfm_amd import pro
    assert "sample_weight" in inspect.signature(pro.BaseModelSFG.train_on_batch).parameters
    src = inspect.getsource(pro.BaseModelSFG.train_on_batch)
    assert "NotImplementedError" in src and "sample_weight" in src


def test_trainer_parses_class_weight():
    import xdftrain_amd as t
    assert t.parse_args(["--data_path", "x"]).class_weight is None
    a = t.parse_args(["--data_path", "x", "--class_weight", "1", "4"])
    assert list(a.class_weight) == [1.0, 4.0] and t._class_weight(a) == {0: 1.0, 1: 4.0}
    with pytest.raises(SystemExit):
        t.parse_args(["--data_path", "x", "--class_weight", "1"])
