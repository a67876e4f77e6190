"""CPU: the exports, the argument checks and the workspace query of K14s (xdfm_eval_metrics, include/xdfm.h) -- every refusal
happens before any device call, so it is exercised without a GPU, with made-up addresses that are never dereferenced -- and the
route `evaluate` takes on a CPU model: today's host functions, never ops.eval_metrics."""
import ctypes

import numpy as np
import pytest
import torch

import eval_metrics_ref as R

Y, P, WS, OUT = 0x10000, 0x20000, 0x30000, 0x40000         # aligned stand-in addresses


def _lib():
    from xdfm_amd import _lib
    return _lib.load()


def _call(y=Y, p=P, N=5000, which=R.ALL, ws=WS, out=OUT):
    lib = _lib()
    v = ctypes.c_void_p
    return lib.xdfm_eval_metrics(v(y) if y else None, v(p) if p else None, N, which, v(ws) if ws else None, v(out) if out else None,
                                 None), lib.xdfm_last_error().decode()


def test_both_symbols_are_exported_and_bound():
    from xdfm_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("xdfm_eval_metrics_ws_bytes", "xdfm_eval_metrics"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["xdfm_eval_metrics_ws_bytes"][1][0] is ctypes.c_long          # N is a long: 2^27 and beyond reach the check


@pytest.mark.parametrize("missing", ["y", "p", "ws", "out"])
def test_a_null_operand_is_refused(missing):
    rc, msg = _call(**{missing: 0})
    assert rc == 1 and "null pointer" in msg and "eval_metrics" in msg


@pytest.mark.parametrize("N", [0, -1, R.MAX_N + 1, 2 ** 31, 2 ** 40])
def test_n_outside_the_range_is_refused(N):
    rc, msg = _call(N=N)
    assert rc == 1 and ("N=%d" % N) in msg


@pytest.mark.parametrize("which", [0, 16, 17, 31, 256, -1])
def test_which_outside_1_to_15_is_refused(which):
    rc, msg = _call(which=which)
    assert rc == 1 and ("which=%d" % which) in msg


@pytest.mark.parametrize("off", [1, 2, 4, 7])
def test_misaligned_ws_and_out_are_refused(off):
    rc, msg = _call(ws=WS + off)
    assert rc == 1 and "ws=" in msg and ("%x" % (WS + off)) in msg and "8-byte" in msg
    rc, msg = _call(out=OUT + off)
    assert rc == 1 and "out4=" in msg and ("%x" % (OUT + off)) in msg and "8-byte" in msg


def test_refusals_raise_through_the_binding():
    from xdfm_amd import _lib
    rc, _ = _call(N=0)
    with pytest.raises(ValueError, match="N=0"):
        _lib.check(rc, "eval_metrics")


def test_ws_bytes():
    lib = _lib()
    for N in (0, -5, R.MAX_N + 1, 2 ** 33):
        assert lib.xdfm_eval_metrics_ws_bytes(N, R.ALL) == 0
    for which in (0, 16, -1):
        assert lib.xdfm_eval_metrics_ws_bytes(4096, which) == 0
    ns = R.N_EDGES + [R.N_K14_CAP_PLUS_1, R.N_MANY_TILES, R.N_SCAN_RUNS_OF_2, 1 << 22, R.MAX_N]
    for N in ns:
        sizes = {which: lib.xdfm_eval_metrics_ws_bytes(N, which) for which in range(1, 16)}
        assert all(n > 0 and n % 8 == 0 for n in sizes.values()), (N, sizes)
        # the sort's arrays come with the AUC alone: two key arrays of N u32 at least, nothing of that size without
        assert all(sizes[w] == sizes[R.AUC] >= 8 * N for w in sizes if w & R.AUC), (N, sizes)
        assert all(sizes[w] == sizes[R.ACC] < sizes[R.AUC] and sizes[w] <= 64 + N // 64 for w in sizes if not w & R.AUC), (N, sizes)
    for which in (R.ALL, R.LOGLOSS):
        sizes = [lib.xdfm_eval_metrics_ws_bytes(N, which) for N in sorted(ns)]
        assert sizes == sorted(sizes)
    assert lib.xdfm_eval_metrics_ws_bytes(R.MAX_N, R.ALL) <= 9 * R.MAX_N


def test_ops_refuses_host_tensors_and_reads_the_switch_once():
    from xdfm_amd import ops
    y, p = torch.zeros(8), torch.zeros(8)
    assert not ops.eval_metrics_supported(y, p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eval_metrics(y, p, R.ALL)
    assert isinstance(ops.EVAL_NATIVE, bool) and ops.EVAL_MAX_ROWS == R.MAX_N


# --------------------------------------------------------------------------------------------------------------- routing
def _cpu_model(monkeypatch, metrics):
    """An xDeepFM on the CPU whose forward is a stand-in (the model's kernels need a GPU): a fixed logistic function of the
    packed inputs, [B, 1] fp32 as the model's."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C%d" % (i + 1), 50, 4) for i in range(3)] + [DenseFeat("I1", 1)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), device="cpu")
    model.compile("adam", "binary_crossentropy", metrics=metrics)
    w = torch.tensor([0.03, -0.02, 0.01, 1.5])
    monkeypatch.setattr(model, "forward", lambda X: torch.sigmoid(X @ w - 0.7).reshape(-1, 1))
    return model


def test_evaluate_on_a_cpu_model_is_the_host_route(monkeypatch):
    from xdfm_amd import metrics as M
    from xdfm_amd import ops
    monkeypatch.setattr(ops, "EVAL_NATIVE", True)
    calls = []
    monkeypatch.setattr(ops, "eval_metrics", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError("native route")))
    names = ["binary_crossentropy", "auc", "mse", "acc"]
    model = _cpu_model(monkeypatch, names)
    rng = np.random.default_rng(4)
    rows = 301                                             # not a multiple of the batch size
    x = {"C%d" % (i + 1): rng.integers(0, 50, rows).astype(np.float32) for i in range(3)}
    x["I1"] = rng.random(rows).astype(np.float32)
    y = (rng.random((rows, 1)) < 0.4).astype(np.float32)
    pred = model.predict(x, 64)
    assert pred.shape == (rows, 1) and pred.dtype == np.float64
    X = np.stack([x[n] for n in model.feature_index], axis=1)
    by_hand = torch.cat([model(torch.from_numpy(X[s:s + 64])) for s in range(0, rows, 64)]).numpy().astype("float64")
    assert pred.tobytes() == by_hand.tobytes()
    got = model.evaluate(x, y, 64)
    want = {"binary_crossentropy": M.log_loss(y, pred), "auc": M.roc_auc_score(y, pred), "mse": M.mean_squared_error(y, pred),
            "acc": M.accuracy_score(y, np.where(pred > 0.5, 1, 0))}
    assert list(got) == names and all(type(v) is float for v in got.values())
    assert all(R.same_bits(got[k], want[k]) for k in names), (got, want)
    assert calls == []
    assert model.predict({k: v[:0] for k, v in x.items()}, 64).shape == (0, 1)
