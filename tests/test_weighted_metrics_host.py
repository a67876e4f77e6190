"""CPU: compile(weighted_metrics=...) through `fit` and `evaluate` on the host route.  The model's kernels need a GPU, so the
CPU model here has a stand-in forward (a fixed logistic function of the packed inputs plus an offset) and a stand-in train step
that moves the offset: the metric plumbing of `fit` / `evaluate` -- which weights reach which entry, the History keys and
their order, early stopping on a weighted key -- is what runs."""
import numpy as np
import pytest
import torch

import eval_metrics_ref as S
from xdfm_amd import metrics as M
from xdfm_amd.callbacks import EarlyStopping

NAMES = ["binary_crossentropy", "auc", "mse", "acc"]
WNAMES = ["weighted_" + n for n in NAMES]
WFUNCS = {"weighted_binary_crossentropy": M.weighted_log_loss, "weighted_auc": M.weighted_roc_auc_score,
          "weighted_mse": M.weighted_mean_squared_error, "weighted_acc": M.weighted_accuracy_score}
ROWS, BATCH = 301, 64
CLASS_WEIGHT = {0: 1.0, 1: 4.0}


def _model(weighted="absent", metrics=NAMES, step=0.05, cls_name="xDeepFM"):
    from deepctr import models
    from deepctr.inputs import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % (i + 1), 50, 4) for i in range(3)] + [DenseFeat("I1", 1)]
    model = getattr(models, cls_name)(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), device="cpu")
    if weighted == "absent":
        model.compile("adam", "binary_crossentropy", metrics=metrics)
    else:
        model.compile("adam", "binary_crossentropy", metrics=metrics, weighted_metrics=weighted)
    coef, state = torch.tensor([0.03, -0.02, 0.01, 1.5]), {"offset": -0.7, "steps": 0}
    model.forward = lambda X: torch.sigmoid(X @ coef + state["offset"]).reshape(-1, 1)

    def train_on_batch(x, y, sample_weight=None):
        yp = model.forward(x)
        w = None if sample_weight is None else sample_weight.reshape(-1)
        loss = torch.nn.functional.binary_cross_entropy(yp.reshape(-1), y.reshape(-1), weight=w, reduction="sum")
        state["offset"] += step
        state["steps"] += 1
        return yp, loss, loss
    model.train_on_batch = train_on_batch
    model.stand_in = state
    return model


def _data(rows=ROWS, seed=4):
    rng = np.random.default_rng(seed)
    x = {"C%d" % (i + 1): rng.integers(0, 50, rows).astype(np.float32) for i in range(3)}
    x["I1"] = rng.random(rows).astype(np.float32)
    y = (rng.random((rows, 1)) < 0.4).astype(np.float32)
    w = rng.integers(0, 9, rows).astype(np.float32) / 4
    return x, y, w


def _fit(model, **kw):
    x, y, _ = _data()
    torch.manual_seed(5)
    kw.setdefault("verbose", 2)
    return model.fit(x, y, batch_size=BATCH, epochs=2, shuffle=True, **kw).history


def _same(a, b):
    return len(a) == len(b) and all(S.same_bits(float(u), float(v)) for u, v in zip(a, b))


def test_nothing_changes_without_weighted_metrics():
    """compile(weighted_metrics=None) and ([]) against compile without the keyword: the same History keys and values, the
    same evaluate dict, bit for bit, also with example weights in the fit."""
    x, y, w = _data()
    vx, vy, vw = _data(120, 9)
    runs = []
    for weighted in ("absent", None, []):
        model = _model(weighted)
        assert model.metrics_names == ["loss"] + NAMES
        h = _fit(model, sample_weight=w, class_weight=CLASS_WEIGHT, validation_data=(vx, vy, vw))
        runs.append((h, model.evaluate(x, y, BATCH)))
    for h, e in runs[1:]:
        assert list(h) == list(runs[0][0]) == ["loss"] + NAMES + ["val_" + n for n in NAMES]
        assert all(_same(h[k], runs[0][0][k]) for k in h)
        assert list(e) == NAMES and all(S.same_bits(e[k], runs[0][1][k]) for k in e)


def test_the_unweighted_entries_do_not_move():
    x, y, w = _data()
    vx, vy, vw = _data(120, 9)
    plain, both = _model(), _model(NAMES)
    assert both.metrics_names == ["loss"] + NAMES + WNAMES and list(both.weighted_metrics) == WNAMES
    kw = dict(sample_weight=w, class_weight=CLASS_WEIGHT, validation_data=(vx, vy, vw))
    hp, hb = _fit(plain, **kw), _fit(both, **kw)
    assert list(hb) == ["loss"] + NAMES + WNAMES + ["val_" + n for n in NAMES + WNAMES]
    assert all(_same(hb[k], hp[k]) for k in hp)
    ep, eb = plain.evaluate(x, y, BATCH), both.evaluate(x, y, BATCH, sample_weight=w)
    assert list(eb) == NAMES + WNAMES and all(S.same_bits(eb[k], ep[k]) for k in ep)
    pred = both.predict(x, BATCH)
    assert all(S.same_bits(eb[k], fn(y, pred, w)) for k, fn in WFUNCS.items())
    # no weights: unit weights, the values of the unweighted entries
    e1 = both.evaluate(x, y, BATCH)
    assert all(S.same_bits(e1["weighted_" + n], ep[n]) for n in NAMES)
    # an unknown name is ignored as `metrics` ignores it: a History name, no function
    odd = _model(["auc", "gauc"])
    assert list(odd.weighted_metrics) == ["weighted_auc"] and odd.metrics_names[-2:] == ["weighted_auc", "weighted_gauc"]


def test_training_values_are_the_numpy_functions_per_step(monkeypatch):
    """weighted_<name> of an epoch is the mean over its steps of the numpy function on that step's (labels, predictions,
    sample_weight * class_weight[y]); without any weights it is the unweighted key's value."""
    x, y, w = _data()
    model = _model(NAMES)
    seen, real = [], model.train_on_batch

    def spy(xb, yb, sample_weight=None):
        out = real(xb, yb, sample_weight)
        seen.append((yb.numpy().copy(), out[0].detach().numpy().astype("float64"), sample_weight.numpy().copy()))
        return out
    model.train_on_batch = spy
    h = _fit(model, sample_weight=w, class_weight=CLASS_WEIGHT)
    steps = (ROWS - 1) // BATCH + 1
    assert len(seen) == 2 * steps
    yall = np.concatenate([s[0].reshape(-1) for s in seen[:steps]])
    wall = np.concatenate([s[2].reshape(-1) for s in seen[:steps]])
    assert sorted(wall.tolist()) == sorted((w * np.where(y.reshape(-1) > 0.5, 4.0, 1.0)).tolist()) and yall.size == ROWS
    for k, fn in WFUNCS.items():
        for epoch in range(2):
            want = np.sum([fn(*s) for s in seen[epoch * steps:(epoch + 1) * steps]]) / steps
            assert S.same_bits(h[k][epoch], float(want)), (k, epoch)
    h1 = _fit(_model(NAMES))
    assert all(_same(h1["weighted_" + n], h1[n]) for n in NAMES)
    # only weighted entries compiled, no weights: the unweighted functions are computed for them
    h2 = _fit(_model(["auc", "binary_crossentropy"], metrics=[]))
    assert list(h2) == ["loss", "weighted_auc", "weighted_binary_crossentropy"]
    assert _same(h2["weighted_auc"], h1["auc"]) and _same(h2["weighted_binary_crossentropy"], h1["binary_crossentropy"])
    assert list(_fit(_model(NAMES), verbose=0)) == ["loss"]


@pytest.mark.parametrize("how", ["split", "three", "two", "two_class_weight", "three_class_weight"])
def test_validation_weights(how):
    """val_weighted_* of the last epoch equal the numpy functions on `predict`'s output for the validation rows with: the tail
    of the weight vector (validation_split), the third item times class_weight[y], class_weight[y] alone, or unit weights."""
    x, y, w = _data()
    vx, vy, vw = _data(120, 9)
    cw = CLASS_WEIGHT if "class_weight" in how else None
    model = _model(NAMES)
    if how == "split":
        h = _fit(model, sample_weight=w, class_weight=CLASS_WEIGHT, validation_split=0.25)
        at = int(ROWS * 0.75)
        vx, vy = {k: v[at:] for k, v in x.items()}, y[at:]
        want_w = (w * np.where(y.reshape(-1) > 0.5, np.float32(4.0), np.float32(1.0)))[at:]
    else:
        h = _fit(model, class_weight=cw, validation_data=(vx, vy, vw) if how.startswith("three") else (vx, vy))
        want_w = vw if how.startswith("three") else np.ones(120, np.float32)
        if cw:
            want_w = want_w * np.where(vy.reshape(-1) > 0.5, np.float32(4.0), np.float32(1.0))
    pred = model.predict(vx, BATCH)                         # the stand-in step does not run in between: the last epoch's model
    for k, fn in WFUNCS.items():
        assert S.same_bits(h["val_" + k][-1], fn(vy, pred, want_w)), (how, k)
    for n, fn in (("binary_crossentropy", M.log_loss), ("auc", M.roc_auc_score)):
        assert S.same_bits(h["val_" + n][-1], fn(vy, pred))


def test_sample_weight_without_weighted_metrics_is_refused():
    x, y, w = _data()
    with pytest.raises(ValueError, match="weighted_metrics"):
        _model().evaluate(x, y, BATCH, sample_weight=w)
    with pytest.raises(ValueError, match="sample_weight"):
        _model(NAMES).evaluate(x, y, BATCH, sample_weight=-w)
    with pytest.raises(ValueError, match="sample_weight"):
        _model(NAMES).evaluate(x, y, BATCH, sample_weight=w[:-1])


def test_one_class_by_weight_raises_the_reference_error():
    x, y, w = _data()
    w0 = np.where(y.reshape(-1) > 0.5, 0.0, 1.0).astype(np.float32)
    with pytest.raises(ValueError, match="Only one class present"):
        _model(["auc"]).evaluate(x, y, BATCH, sample_weight=w0)


def test_early_stopping_on_a_weighted_key():
    """The stand-in step raises the offset by 0.4 per step: the weighted validation logloss falls, then rises.  The series is
    computed by hand from the offsets; EarlyStopping(patience=0) must stop at its first rise."""
    x, y, w = _data()
    vx, vy, vw = _data(120, 9)
    model = _model(["binary_crossentropy"], metrics=[], step=0.4)
    steps = (ROWS - 1) // BATCH + 1
    coef = np.array([0.03, -0.02, 0.01, 1.5], np.float32)
    VX = torch.from_numpy(np.stack([vx[n] for n in model.feature_index], axis=1))
    series = []
    for epoch in range(8):
        off = -0.7 + 0.4 * steps * (epoch + 1)
        pred = torch.sigmoid(VX @ torch.from_numpy(coef) + off).numpy().astype("float64")
        series.append(M.weighted_log_loss(vy, pred, vw))
    first_rise = next(e for e in range(1, 8) if series[e] >= series[e - 1])
    assert 1 <= first_rise < 7
    stop = EarlyStopping(monitor="val_weighted_binary_crossentropy", patience=0, mode="min")
    torch.manual_seed(5)
    h = model.fit(x, y, batch_size=BATCH, epochs=8, verbose=0, validation_data=(vx, vy, vw), callbacks=[stop]).history
    assert len(h["loss"]) == first_rise + 1
    assert _same(h["val_weighted_binary_crossentropy"], series[:first_rise + 1])


def test_pro_models_refuse_weighted_metrics():
    from deepctr import xdeepfm_pro
    from deepctr.inputs import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % (i + 1), 50, 4) for i in range(3)] + [DenseFeat("I1", 1)]
    model = xdeepfm_pro.xDeepFMProLight(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), device="cpu")
    with pytest.raises(NotImplementedError, match="SFG term is normalised on its own"):
        model.compile("adam", "binary_crossentropy", metrics=["auc"], weighted_metrics=["auc"])
    model.compile("adam", "binary_crossentropy", metrics=["auc"], weighted_metrics=[])
    assert model.metrics_names[-1] == "auc"


def test_the_trainer_parses_the_flag():
    import xdftrain_amd as T
    assert T.parse_args(["--weighted_metrics", "--class_weight", "1", "4"]).weighted_metrics is True
    assert T.parse_args([]).weighted_metrics is False
