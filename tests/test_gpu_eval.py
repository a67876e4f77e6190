"""GPU tests (-m gpu) of the native route of BaseModel.evaluate (K14s through ops.eval_metrics) on a small model: the switch
ops.EVAL_NATIVE on against off -- AUC and accuracy bit for bit, logloss and mse within eval_metrics_ref.bar --, `predict`
against the batch loop written out, what is routed and what keeps the host route, and the validation of `fit`."""
import numpy as np
import pytest
import torch

import eval_metrics_ref as R

pytestmark = pytest.mark.gpu
NAMES = ["binary_crossentropy", "auc", "mse", "acc"]
ROWS, BATCH = 301, 64                                 # 5 batches, the last one of 45 rows
ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


def _dev():
    return torch.device("cuda:0")


def _data(rows=ROWS, seed=21):
    rng = np.random.default_rng(seed)
    x = {"C%d" % (i + 1): rng.integers(0, 50, rows).astype(np.float32) for i in range(4)}
    x.update({"I%d" % (i + 1): rng.random(rows).astype(np.float32) for i in range(2)})
    y = (rng.random((rows, 1)) < 0.35).astype(np.float32)
    return x, y


def _model(cls_name="xDeepFM", metrics=NAMES):
    """4 sparse fields of 50 ids, D = 4, 2 dense fields, cin (8, 8), dnn (16, 16); weights wide enough for predictions away from
    0.5."""
    from deepctr import models, xdeepfm_pro
    from deepctr.inputs import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % (i + 1), 50, 4) for i in range(4)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(2)]
    kw = dict(dnn_hidden_units=(16, 16), cin_layer_size=(8, 8), l2_reg_dnn=1e-5, device=_dev())
    model = getattr(xdeepfm_pro if "Pro" in cls_name else models, cls_name)(cols, cols, **kw)
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k or k.endswith("linear.weight") or "dnn.linears" in k:
                p.copy_((0.3 * torch.randn(p.shape, generator=gen)).to(p.device))
    model.compile("adam", "binary_crossentropy", metrics=metrics)
    return model


@pytest.fixture(scope="module")
def model():
    return _model()


def _spy(monkeypatch):
    """ops.eval_metrics and Tensor.cpu with their calls recorded: [(which, rows)] and [numel of every tensor copied]."""
    from xdfm_amd import ops
    calls, copies, real, real_cpu = [], [], ops.eval_metrics, torch.Tensor.cpu

    def recorded(y, p, which):
        calls.append((int(which), y.numel()))
        return real(y, p, which)

    def cpu(t, *a, **k):
        copies.append(t.numel())
        return real_cpu(t, *a, **k)
    monkeypatch.setattr(ops, "eval_metrics", recorded)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    return calls, copies


def _same(on, off, rows):
    assert list(on) == list(off) and all(type(v) is float for v in on.values())
    for k in on:
        if k in ("auc", "acc"):
            assert R.same_bits(on[k], off[k]), (k, on[k], off[k])
        elif k in ("binary_crossentropy", "mse"):
            assert R.ratio(on[k], off[k], rows) <= 1.0, (k, on[k], off[k])


@pytest.mark.parametrize("cls_name", ["xDeepFM", "xDeepFMProLight"])
def test_evaluate_native_against_host(monkeypatch, cls_name):
    """301 rows in batches of 64, all four metrics: the native route makes ONE ops.eval_metrics call for all four and copies no
    N-long tensor to the host; its values against the host route's.  xDeepFMProLight: BaseModelSFG inherits the route."""
    from xdfm_amd import ops
    model = _model(cls_name)
    x, y = _data()
    calls, copies = _spy(monkeypatch)
    monkeypatch.setattr(ops, "EVAL_NATIVE", True)
    on = model.evaluate(x, y, BATCH)
    assert calls == [(R.ALL, ROWS)] and all(n < ROWS for n in copies), (calls, copies)
    del calls[:], copies[:]
    monkeypatch.setattr(ops, "EVAL_NATIVE", False)
    off = model.evaluate(x, y, BATCH)
    assert calls == [] and copies.count(ROWS) == 1
    assert list(on) == NAMES and 0.0 < on["auc"] < 1.0 and on["auc"] != 0.5
    _same(on, off, ROWS)
    # labels as a bool or an int vector, or [N] instead of [N, 1]: one label per row, unchanged by float32 -- native, same values
    monkeypatch.setattr(ops, "EVAL_NATIVE", True)
    for y_alt in (y.reshape(-1), y.astype(np.int64), y.astype(bool), y.astype(np.float64)):
        del calls[:]
        alt = model.evaluate(x, y_alt, BATCH)
        assert calls == [(R.ALL, ROWS)] and all(R.same_bits(alt[k], on[k]) for k in NAMES)


def test_predict_is_the_batch_loop(model):
    x, _ = _data()
    pred = model.predict(x, BATCH)
    assert pred.shape == (ROWS, 1) and pred.dtype == np.float64
    X = torch.from_numpy(np.stack([x[n] for n in model.feature_index], axis=1)).to(_dev())
    model.eval()
    with torch.no_grad():
        by_hand = torch.cat([model(X[s:s + BATCH]) for s in range(0, ROWS, BATCH)])
    assert by_hand.dtype == torch.float32
    assert pred.tobytes() == by_hand.cpu().numpy().astype("float64").tobytes()
    assert model.predict({k: v[:0] for k, v in x.items()}, BATCH).shape == (0, 1)


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("cls", [0.0, 1.0])
def test_one_class_raises_the_same_error(monkeypatch, model, native, cls):
    from xdfm_amd import ops
    monkeypatch.setattr(ops, "EVAL_NATIVE", native)
    x, y = _data()
    with pytest.raises(ValueError) as e:
        model.evaluate(x, np.full_like(y, cls), BATCH)
    assert str(e.value) == ONE_CLASS


def test_a_user_callable_keeps_the_host_route_for_itself(monkeypatch):
    from xdfm_amd import ops
    monkeypatch.setattr(ops, "EVAL_NATIVE", True)
    model = _model()
    x, y = _data()
    want = model.evaluate(x, y, BATCH)
    seen = []

    def user_mse(y_true, y_pred):
        assert isinstance(y_true, np.ndarray) and y_pred.dtype == np.float64 and y_pred.shape == (ROWS, 1)
        seen.append(y_pred)
        return 42.0
    model.metrics["mse"] = user_mse
    calls, copies = _spy(monkeypatch)
    got = model.evaluate(x, y, BATCH)
    assert calls == [(R.LOGLOSS | R.AUC | R.ACC, ROWS)] and copies.count(ROWS) == 1 and len(seen) == 1
    assert list(got) == NAMES and got["mse"] == 42.0
    assert all(R.same_bits(got[k], want[k]) for k in NAMES if k != "mse")
    assert seen[0].tobytes() == model.predict(x, BATCH).tobytes()
    # nothing wired left: today's route entirely
    for k in NAMES:
        model.metrics[k] = user_mse
    del calls[:]
    assert model.evaluate(x, y, BATCH) == dict.fromkeys(NAMES, 42.0) and calls == []


def test_labels_that_float32_would_change_take_the_host_route(monkeypatch, model):
    from xdfm_amd import metrics as M
    from xdfm_amd import ops
    monkeypatch.setattr(ops, "EVAL_NATIVE", True)
    x, y = _data()
    soft = np.where(y > 0.5, 0.9, 0.1).astype(np.float64)             # 0.1 and 0.9 are not float32 values
    calls, _ = _spy(monkeypatch)
    got = model.evaluate(x, soft, BATCH)
    pred = model.predict(x, BATCH)
    assert calls == []
    assert got["binary_crossentropy"] == M.log_loss(soft, pred) and got["mse"] == M.mean_squared_error(soft, pred)
    # a label vector of another length is the host functions' business too
    with pytest.raises(Exception):
        model.evaluate(x, y[:-1], BATCH)
    assert calls == []


def test_fit_validation_history_is_the_same_across_the_switch(monkeypatch):
    """2 epochs with validation_data of 301 rows (not a multiple of the batch): the val_* histories of the two routes from the
    same seed, and one native call per epoch."""
    from xdfm_amd import ops
    x, y = _data()
    vx, vy = _data(seed=22)
    hist = {}
    calls, _ = _spy(monkeypatch)
    for native in (True, False):
        monkeypatch.setattr(ops, "EVAL_NATIVE", native)
        hist[native] = _model().fit(x, y, batch_size=BATCH, epochs=2, verbose=0, shuffle=True, validation_data=(vx, vy)).history
        assert calls == ([(R.ALL, ROWS)] * 2 if native else [])
        del calls[:]
    on, off = hist[True], hist[False]
    assert list(on) == list(off) and [k for k in on if k.startswith("val_")] == ["val_" + n for n in NAMES]
    assert all(R.same_bits(a, b) for a, b in zip(on["loss"], off["loss"]))
    for epoch in range(2):
        _same({n: on["val_" + n][epoch] for n in NAMES}, {n: off["val_" + n][epoch] for n in NAMES}, ROWS)
    assert on["val_auc"][0] != on["val_auc"][1]


def test_ops_eval_metrics(monkeypatch):
    """ops.eval_metrics: NaN in the slots not asked for, the cached workspace grows and is reused, and what it refuses."""
    from xdfm_amd import ops
    dev = _dev()
    small = (torch.from_numpy(R.labels("mixed", 1000, 1)).to(dev), torch.from_numpy(R.scores("uniform", 1000, 1)).to(dev))
    large = (torch.from_numpy(R.labels("mixed", 70001, 2)).to(dev), torch.from_numpy(R.scores("eight", 70001, 2)).to(dev))
    first = ops.eval_metrics(small[0], small[1], R.AUC | R.ACC).tolist()
    assert first[0] != first[0] and first[2] != first[2]
    ref = R.reference(small[0].cpu().numpy(), small[1].cpu().numpy())
    assert R.same_bits(first[1], ref[1]) and R.same_bits(first[3], ref[3])
    big = ops.eval_metrics(large[0], large[1], R.ALL).tolist()
    ws = ops._EVAL_WS[dev.index]
    assert ws.numel() * 8 >= 8 * 70001
    again = ops.eval_metrics(small[0], small[1], R.ALL).tolist()
    assert ops._EVAL_WS[dev.index] is ws and R.same_bits(again[1], first[1]) and R.same_bits(again[3], first[3])
    ref = R.reference(large[0].cpu().numpy(), large[1].cpu().numpy())
    assert R.same_bits(big[1], ref[1]) and R.same_bits(big[3], ref[3]) and R.ratio(big[0], ref[0], 70001) <= 1.0
    y, p = small
    assert ops.eval_metrics_supported(y, p)
    for bad_y, bad_p in ((y.reshape(-1, 1), p), (y, p[:-1]), (y[::2], p[::2]), (y.double(), p), (y[:0], p[:0])):
        assert not ops.eval_metrics_supported(bad_y, bad_p)
    with pytest.raises(ValueError):
        ops.eval_metrics(y, p[:-1], R.ALL)
    with pytest.raises(ValueError):
        ops.eval_metrics(y, p, 0)
    with pytest.raises(TypeError):
        ops.eval_metrics(y.double(), p, R.ALL)
