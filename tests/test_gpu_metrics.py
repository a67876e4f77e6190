"""GPU tests (-m gpu) of the native batch metrics (K14) through ops.batch_metrics and the `fit` loop of models.py.

ops.batch_metrics against the float64 device compositions it replaces (xdfm_amd.metrics.*_device) on the same tensors: AUC
bit for bit, logloss / mse within metrics_ref.bar (two float64 sums of the same B terms in different orders), accuracy against
the host function bit for bit; two kernel nodes and nothing else when captured.  `fit`: the History of a small model with
ops.METRICS_NATIVE on against off from the same seed, what is and is not routed, and the cases that keep the earlier route."""
import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu
NAMES = ["binary_crossentropy", "auc", "mse", "acc"]
ROWS, BATCH, EPOCHS = 300, 64, 2                      # 5 steps per epoch, the last one of 44 rows
STEPS = (ROWS - 1) // BATCH + 1
ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


def _dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- ops
@pytest.mark.parametrize("B,sk", [(4097, "uniform"), (1000, "eight"), (44, "sigmoid")])
def test_ops_batch_metrics_against_the_device_compositions(B, sk):
    from xdfm_amd import metrics as M
    from xdfm_amd import ops
    dev = _dev()
    yn, pn = R.labels("mixed", B, 11), R.scores(sk, B, 11)
    y, p = torch.from_numpy(yn).to(dev).reshape(B, 1), torch.from_numpy(pn).to(dev)       # [B, 1] against [B]: as `fit` has them
    log = torch.full((3, 4), -1.0, dtype=torch.float64, device=dev)
    assert ops.batch_metrics_supported(y, p)
    ops.batch_metrics(y, p, R.ALL, log[1])
    torch.cuda.synchronize()
    got = log[1].tolist()
    assert bool((log[0] == -1.0).all()) and bool((log[2] == -1.0).all())
    assert R.same_bits(got[1], float(M.roc_auc_score_device(y, p)))
    assert R.ratio(got[0], float(M.log_loss_device(y, p)), B) <= 1.0
    assert R.ratio(got[2], float(M.mean_squared_error_device(y, p)), B) <= 1.0
    assert R.same_bits(got[3], M.accuracy_score(yn, np.where(pn > 0.5, 1, 0)))
    ref = R.reference(yn, pn)
    assert R.same_bits(got[1], ref[1]) and R.ratio(got[0], ref[0], B) <= 1.0 and R.ratio(got[2], ref[2], B) <= 1.0


def test_ops_batch_metrics_refuses_what_the_kernel_cannot_take():
    from xdfm_amd import ops
    dev = _dev()
    y, p = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.batch_metrics(y.cpu(), p, R.ALL, out)
    with pytest.raises(TypeError):
        ops.batch_metrics(y.double(), p, R.ALL, out)
    with pytest.raises(ValueError):
        ops.batch_metrics(y, p[:7], R.ALL, out)
    with pytest.raises(ValueError):
        ops.batch_metrics(y, p, 0, out)
    with pytest.raises(ValueError):
        ops.batch_metrics(y, p, R.ALL, out.float())
    big = torch.zeros(R.MAX_B + 1, device=dev)
    assert not ops.batch_metrics_supported(big, big) and not ops.batch_metrics_supported(y.double(), p)
    with pytest.raises(ValueError):
        ops.batch_metrics(big, big, R.ALL, out)


@pytest.mark.parametrize("which", [R.LOGLOSS | R.AUC, R.ALL, R.ACC])
def test_two_kernel_nodes_and_nothing_else(which):
    """ops.batch_metrics captured alone: 2 nodes in all, so 2 kernel nodes and neither a memset nor a memcpy node."""
    from xdfm_amd import graphstep, ops
    dev = _dev()
    B = 4096
    y, p = torch.from_numpy(R.labels("mixed", B, 12)).to(dev), torch.from_numpy(R.scores("uniform", B, 12)).to(dev)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    ops.batch_metrics(y, p, which, out)                  # the cached workspace exists before the capture
    torch.cuda.synchronize()
    eager = out.clone()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        ops.batch_metrics(y, p, which, out)
    nodes, memsets, other = graphstep.census(g)
    assert nodes == 2 and memsets == 0 and other == 0, (nodes, memsets, other)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------- fit
def _data(seed=21, one_class=False):
    rng = np.random.default_rng(seed)
    x = {"C%d" % (i + 1): rng.integers(0, 50, ROWS).astype(np.float32) for i in range(4)}
    x.update({"I%d" % (i + 1): rng.random(ROWS).astype(np.float32) for i in range(2)})
    y = np.ones((ROWS, 1), np.float32) if one_class else (rng.random((ROWS, 1)) < 0.35).astype(np.float32)
    return x, y


def _model(cls_name="xDeepFM", metrics=NAMES):
    """4 sparse fields of 50 ids, D = 4, 2 dense fields, cin (8, 8), dnn (16, 16); weights wide enough for predictions away from
    0.5.  The constructor seeds torch's generator, which draws the epochs' orders: build a model right before its fit."""
    from deepctr import models
    from deepctr.inputs import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % (i + 1), 50, 4) for i in range(4)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(2)]
    kw = dict(dnn_hidden_units=(16, 16), cin_layer_size=(8, 8), l2_reg_dnn=1e-5, device=_dev())
    if cls_name == "xDeepFMAttention":
        kw["cin_num_heads"] = 2
    model = getattr(models, cls_name)(cols, cols, **kw)
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k or k.endswith("linear.weight") or "dnn.linears" in k:
                p.copy_((0.3 * torch.randn(p.shape, generator=gen)).to(p.device))
    model.compile("adam", "binary_crossentropy", metrics=metrics)
    return model


def _fit(monkeypatch, native, cls_name="xDeepFM", metrics=NAMES, verbose=2, prepare=None, one_class=False):
    from xdfm_amd import ops
    monkeypatch.setattr(ops, "METRICS_NATIVE", native)
    x, y = _data(one_class=one_class)
    model = _model(cls_name, metrics)
    if prepare is not None:
        prepare(model)
    return model.fit(x, y, batch_size=BATCH, epochs=EPOCHS, verbose=verbose, shuffle=True).history


def _record(monkeypatch):
    """ops.batch_metrics with a list of the `which` of its calls."""
    from xdfm_amd import ops
    calls, real = [], ops.batch_metrics

    def recorded(y, p, which, out):
        calls.append((int(which), y.numel()))
        return real(y, p, which, out)
    monkeypatch.setattr(ops, "batch_metrics", recorded)
    return calls


@pytest.mark.parametrize("cls_name", ["xDeepFM", "xDeepFMAttention"])
def test_history_native_against_device_compositions(monkeypatch, cls_name):
    """2 epochs of 5 steps at verbose=2 with all four metrics, the switch on and off from the same seed.  loss, auc, acc: the same
    bits.  The logloss and mse epoch means: within the bar of a 64-row batch times the step count.  Keys in `compile` order."""
    calls = _record(monkeypatch)
    on = _fit(monkeypatch, True, cls_name)
    assert [c[0] for c in calls] == [R.ALL] * (EPOCHS * STEPS) and {c[1] for c in calls} == {BATCH, ROWS - (STEPS - 1) * BATCH}
    del calls[:]
    off = _fit(monkeypatch, False, cls_name)
    assert calls == []
    assert list(on) == list(off) == ["loss"] + NAMES
    for k in ("loss", "auc", "acc"):
        assert len(on[k]) == EPOCHS and all(R.same_bits(a, b) for a, b in zip(on[k], off[k])), (k, on[k], off[k])
    assert all(0.0 < v < 1.0 for v in on["auc"]) and on["loss"][0] != on["loss"][1]
    for k in ("binary_crossentropy", "mse"):
        for a, b in zip(on[k], off[k]):
            assert abs(a - b) <= STEPS * R.bar(BATCH, b), (k, a, b)


def test_routing(monkeypatch):
    """Switch on: neither the device compositions nor the host functions nor Tensor.cpu run per step for the routed metrics (no
    more .cpu() calls than a fit without metrics makes).  A callable the user puts into model.metrics is still called every
    step, through the host route, while the others stay native."""
    from xdfm_amd import metrics as M
    counts = {"host": 0, "device": 0, "cpu": 0, "user": 0}

    def counting(key, fn):
        def stand_in(*a, **k):
            counts[key] += 1
            return fn(*a, **k)
        return stand_in
    for name in ("log_loss", "roc_auc_score", "mean_squared_error", "accuracy_score"):
        fn = getattr(M, name)
        stand_in = counting("host", fn)
        if fn in M.DEVICE:
            monkeypatch.setitem(M.DEVICE, stand_in, counting("device", M.DEVICE[fn]))
        monkeypatch.setattr(M, name, stand_in)
    monkeypatch.setattr(torch.Tensor, "cpu", counting("cpu", torch.Tensor.cpu))
    calls = _record(monkeypatch)
    _fit(monkeypatch, True, metrics=[])
    floor = counts["cpu"]
    assert calls == [] and counts["host"] == counts["device"] == 0
    counts["cpu"] = 0
    _fit(monkeypatch, True)
    assert len(calls) == EPOCHS * STEPS
    assert counts["host"] == 0 and counts["device"] == 0 and counts["cpu"] <= floor, counts
    # the earlier route, for contrast: the device compositions per step, and two host copies per step for "acc"
    counts.update(host=0, device=0, cpu=0)
    del calls[:]
    _fit(monkeypatch, False)
    assert calls == [] and counts["device"] == 3 * EPOCHS * STEPS and counts["cpu"] >= floor + 2 * EPOCHS * STEPS, counts
    # a user's callable for "mse": called per step on host arrays; logloss | auc | acc stay in one native call
    counts.update(host=0, device=0, cpu=0)
    del calls[:]

    def user_mse(y_true, y_pred):
        assert isinstance(y_true, np.ndarray) and y_pred.dtype == np.float64
        counts["user"] += 1
        return 42.0

    h = _fit(monkeypatch, True, prepare=lambda m: m.metrics.__setitem__("mse", user_mse))
    assert counts["user"] == EPOCHS * STEPS and counts["device"] == 0
    assert [c[0] for c in calls] == [R.LOGLOSS | R.AUC | R.ACC] * (EPOCHS * STEPS)
    assert h["mse"] == [42.0] * EPOCHS and list(h) == ["loss"] + NAMES


@pytest.mark.parametrize("native", [True, False])
def test_single_class_batch_raises_the_same_error(monkeypatch, native):
    with pytest.raises(ValueError) as e:
        _fit(monkeypatch, native, one_class=True)
    assert str(e.value) == ONE_CLASS


def test_nothing_new_without_metrics_or_with_verbose_0(monkeypatch):
    calls = _record(monkeypatch)
    h = _fit(monkeypatch, True, metrics=[])
    assert list(h) == ["loss"]
    h = _fit(monkeypatch, True, verbose=0)
    assert list(h) == ["loss"]
    assert calls == []
