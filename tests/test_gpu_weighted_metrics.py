"""GPU tests (-m gpu) of compile(weighted_metrics=...) on a small model: the native route (K14w through ops.eval_metrics_w) of
`evaluate` and of the per-batch log of `fit` against the host route (ops.EVAL_W_NATIVE off: metrics.py's weighted numpy
functions) -- AUC and accuracy bit for bit under dyadic weights, logloss and mse within eval_metrics_w_ref.rel_bar --, what is
routed where, and how many native calls are made.  5000 rows: two tiles of the kernel; batches of 512, the last one of 392."""
import numpy as np
import pytest
import torch

import eval_metrics_ref as S
import eval_metrics_w_ref as R
import test_gpu_eval as TE

pytestmark = pytest.mark.gpu
NAMES = TE.NAMES
WNAMES = ["weighted_" + n for n in NAMES]
ROWS, BATCH = 5000, 512
STEPS = (ROWS - 1) // BATCH + 1


def _data(rows=ROWS, seed=31):
    x, y = TE._data(rows, seed)
    return x, y, R.weights("dyadic", rows, seed)


def _model(weighted=NAMES, metrics=NAMES):
    model = TE._model("xDeepFM", metrics)
    model.compile("adam", "binary_crossentropy", metrics=metrics, weighted_metrics=weighted)
    return model


def _spy(monkeypatch):
    """ops.eval_metrics_w, ops.eval_metrics and ops.batch_metrics with their calls recorded as (which, rows)."""
    from xdfm_amd import ops
    calls = {"w": [], "s": [], "b": []}
    real_w, real_s, real_b = ops.eval_metrics_w, ops.eval_metrics, ops.batch_metrics

    def rec_w(y, p, w, which, out=None):
        calls["w"].append((int(which), y.numel()))
        return real_w(y, p, w, which, out)

    def rec_s(y, p, which):
        calls["s"].append((int(which), y.numel()))
        return real_s(y, p, which)

    def rec_b(y, p, which, *a, **k):
        calls["b"].append((int(which), y.numel()))
        return real_b(y, p, which, *a, **k)
    monkeypatch.setattr(ops, "eval_metrics_w", rec_w)
    monkeypatch.setattr(ops, "eval_metrics", rec_s)
    monkeypatch.setattr(ops, "batch_metrics", rec_b)
    return calls


def _close(on, off, rows, what):
    """Weighted entries of the native route against the host route's: dyadic weights."""
    for n in NAMES:
        a, b = on["weighted_" + n], off["weighted_" + n]
        if n in ("auc", "acc"):
            assert S.same_bits(a, b), (what, n, a, b)
        else:
            assert abs(a - b) <= R.rel_bar(rows) * abs(b), (what, n, a, b)


def test_evaluate_native_against_host(monkeypatch):
    from xdfm_amd import metrics as M
    from xdfm_amd import ops
    model = _model()
    x, y, w = _data()
    calls = _spy(monkeypatch)
    monkeypatch.setattr(ops, "EVAL_W_NATIVE", True)
    on = model.evaluate(x, y, BATCH, sample_weight=w)
    assert calls["w"] == [(R.ALL, ROWS)] and calls["s"] == [(R.ALL, ROWS)]
    monkeypatch.setattr(ops, "EVAL_W_NATIVE", False)
    off = model.evaluate(x, y, BATCH, sample_weight=w)
    assert calls["w"] == [(R.ALL, ROWS)] and calls["s"] == [(R.ALL, ROWS)] * 2
    assert list(on) == list(off) == NAMES + WNAMES and all(type(v) is float for v in on.values())
    assert all(S.same_bits(on[n], off[n]) for n in NAMES)             # K14s serves them in both runs
    _close(on, off, ROWS, "evaluate")
    pred = model.predict(x, BATCH)
    assert S.same_bits(off["weighted_auc"], M.weighted_roc_auc_score(y, pred, w)) and on["weighted_auc"] != on["auc"]
    # the unweighted entries are those of a model compiled without weighted_metrics
    plain = TE._model().evaluate(x, y, BATCH)
    assert all(S.same_bits(on[n], plain[n]) for n in NAMES)


def test_fit_history_across_the_switch(monkeypatch):
    """2 epochs, verbose=2, sample weights and 3-item validation data: one K14w call per step and one per validation."""
    from xdfm_amd import ops
    x, y, w = _data()
    vx, vy, vw = _data(seed=32)
    calls = _spy(monkeypatch)
    hist = {}
    for native in (True, False):
        monkeypatch.setattr(ops, "EVAL_W_NATIVE", native)
        torch.manual_seed(3)
        hist[native] = _model().fit(x, y, batch_size=BATCH, epochs=2, verbose=2, shuffle=True, sample_weight=w,
                                    validation_data=(vx, vy, vw)).history
        if native:
            per_epoch = [(R.ALL, BATCH)] * (STEPS - 1) + [(R.ALL, ROWS - (STEPS - 1) * BATCH), (R.ALL, ROWS)]
            assert calls["w"] == per_epoch * 2, calls["w"]
        else:
            assert calls["w"] == []
        assert len(calls["b"]) == 2 * STEPS and calls["s"] == [(R.ALL, ROWS)] * 2       # the unweighted keys: as ever
        for v in calls.values():
            del v[:]
    on, off = hist[True], hist[False]
    assert list(on) == list(off) == ["loss"] + NAMES + WNAMES + ["val_" + n for n in NAMES + WNAMES]
    assert all(S.same_bits(a, b) for k in ["loss"] + NAMES for a, b in zip(on[k], off[k]))
    for epoch in range(2):
        _close({k: on[k][epoch] for k in WNAMES}, {k: off[k][epoch] for k in WNAMES}, BATCH, "train epoch %d" % epoch)
        _close({k: on["val_" + k][epoch] for k in WNAMES}, {k: off["val_" + k][epoch] for k in WNAMES}, ROWS, "val epoch %d" % epoch)
    assert on["weighted_auc"][0] != on["auc"][0]


def test_routing(monkeypatch):
    """No K14w call: without weights (unit weights: the unweighted values, K14s / K14), with soft labels (the host's arithmetic)
    and for a callable the user put into model.weighted_metrics (the other entries stay native)."""
    from xdfm_amd import metrics as M
    from xdfm_amd import ops
    monkeypatch.setattr(ops, "EVAL_W_NATIVE", True)
    model = _model()
    x, y, w = _data()
    calls = _spy(monkeypatch)
    unit = model.evaluate(x, y, BATCH)
    assert calls["w"] == [] and calls["s"] == [(R.ALL, ROWS)]
    assert all(S.same_bits(unit["weighted_" + n], unit[n]) for n in NAMES)
    only = _model(["auc"], metrics=[]).evaluate(x, y, BATCH)            # no unweighted entry: K14s still serves the unit case
    assert list(only) == ["weighted_auc"] and S.same_bits(only["weighted_auc"], unit["auc"]) and calls["w"] == []
    h = _model().fit(x, y, batch_size=BATCH, epochs=1, verbose=2, shuffle=False).history
    assert calls["w"] == [] and all(S.same_bits(h["weighted_" + n][0], h[n][0]) for n in NAMES)
    soft = np.where(y > 0.5, 0.9, 0.1).astype(np.float64)
    del calls["s"][:]
    got = model.evaluate(x, soft, BATCH, sample_weight=w)
    pred = model.predict(x, BATCH)
    assert calls["w"] == [] and calls["s"] == []
    assert got["weighted_binary_crossentropy"] == M.weighted_log_loss(soft, pred, w)
    seen = []
    model.weighted_metrics["weighted_mse"] = lambda yt, yp, ww: seen.append((yp.dtype, ww.dtype, ww.shape)) or 42.0
    got = model.evaluate(x, y, BATCH, sample_weight=w)
    assert calls["w"] == [(R.LOGLOSS | R.AUC | R.ACC, ROWS)] and got["weighted_mse"] == 42.0
    assert seen == [(np.dtype("float64"), np.dtype("float32"), (ROWS,))]


def test_a_model_without_weighted_metrics_launches_what_it_did(monkeypatch):
    x, y, w = _data()
    vx, vy, vw = _data(seed=32)
    calls = _spy(monkeypatch)
    model = TE._model()
    model.fit(x, y, batch_size=BATCH, epochs=1, verbose=2, shuffle=True, sample_weight=w, validation_data=(vx, vy, vw))
    assert calls["w"] == [] and calls["s"] == [(R.ALL, ROWS)] and [c[0] for c in calls["b"]] == [R.ALL] * STEPS
    with pytest.raises(ValueError, match="weighted_metrics"):
        model.evaluate(x, y, BATCH, sample_weight=w)


def test_one_class_by_weight_raises_on_both_routes(monkeypatch):
    from xdfm_amd import ops
    x, y, w = _data()
    w0 = np.where(y.reshape(-1) > 0.5, 0.0, w).astype(np.float32)
    model = _model(["auc"])
    for native in (True, False):
        monkeypatch.setattr(ops, "EVAL_W_NATIVE", native)
        with pytest.raises(ValueError) as e:
            model.evaluate(x, y, BATCH, sample_weight=w0)
        assert str(e.value) == TE.ONE_CLASS


def test_ops_eval_metrics_w():
    """NaN in the slots not asked for, `out`, the cached workspace grows, and what is refused."""
    from xdfm_amd import ops
    dev = TE._dev()
    y, p = torch.from_numpy(S.labels("mixed", 1000, 1)).to(dev), torch.from_numpy(S.scores("uniform", 1000, 1)).to(dev)
    w = torch.from_numpy(R.weights("dyadic", 1000, 1)).to(dev)
    first = ops.eval_metrics_w(y, p, w, R.AUC | R.ACC).tolist()
    assert first[0] != first[0] and first[2] != first[2] and 0.0 < first[1] < 1.0
    big = [torch.from_numpy(a).to(dev) for a in (S.labels("mixed", 70001, 2), S.scores("eight", 70001, 2), R.weights("wide", 70001, 2))]
    assert all(v == v for v in ops.eval_metrics_w(*big, R.ALL).tolist())
    row = torch.full((3, 4), 7.0, dtype=torch.float64, device=dev)
    assert ops.eval_metrics_w(y, p, w, R.AUC | R.ACC, row[1]) is not None
    assert row[1].tolist() == [7.0, first[1], 7.0, first[3]] and row[0].tolist() == [7.0] * 4 and row[2].tolist() == [7.0] * 4
    assert ops.eval_metrics_w_supported(y, p, w)
    for bad in (w[:-1], w.double(), w.cpu(), torch.stack([w, w], 1)[:, 0]):
        assert not ops.eval_metrics_w_supported(y, p, bad)
    with pytest.raises(ValueError):
        ops.eval_metrics_w(y, p, w[:-1], R.ALL)
    with pytest.raises(ValueError):
        ops.eval_metrics_w(y, p, w, 0)
