"""GPU tests of example weights through the model: train_on_batch(x, y, sample_weight), the captured weighted step, and
fit(sample_weight=, class_weight=), on the tiny model shape of test_gpu_head_ex.py (6 sparse + 3 dense columns, D = 8,
CIN (16, 8), DNN (32, 16)) at B = 64."""
import faulthandler
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
T = torch.from_numpy

STEP_LIMIT_S = 300          # a hang ends the process instead of blocking the run
VOCAB, ND, D, B = [50, 31, 77, 12, 9, 40], 3, 8, 64
CIN, DNN = (16, 8), (32, 16)
CLASSES = {"xDeepFM": "sum", "xDeepFMAttention": "attn", "xDeepFMAttentionV2": "attn_v2"}
LR = 0.01                   # of compile("sgd")


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _names():
    return ["C%d" % (i + 1) for i in range(len(VOCAB))], ["I%d" % (i + 1) for i in range(ND)]


def _model(dev, cls="xDeepFM", optimizer="adam", task="binary", loss="binary_crossentropy", graph=True, spread=0.0):
    from deepctr import models
    from deepctr.inputs import DenseFeat, SparseFeat
    from xdfm_amd import graphstep
    names, dnames = _names()
    cols = [SparseFeat(n, v, D) for n, v in zip(names, VOCAB)] + [DenseFeat(n, 1) for n in dnames]
    model = getattr(models, cls)(cols, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, l2_reg_dnn=1e-5, task=task, device=dev)
    if spread:
        g = torch.Generator().manual_seed(3)        # away from the 1e-4 initialisation: every parameter gets a gradient worth comparing
        with torch.no_grad():
            for p in model.parameters():
                p.add_((spread * torch.randn(p.shape, generator=g)).to(p.device))
    model.compile(optimizer, loss, metrics=[])
    model.train()
    step = graphstep.GraphedStep(model)
    if not graph:
        step.disabled = True                         # what XDFM_HIP_GRAPH=0 sets
    model.__dict__["_graphed_step"] = step
    return model


def _batch(s, rows=B, task="binary"):
    from oracle import xdeepfm_oracle as orc
    Xn, yn = orc.synthetic_batch(rows, VOCAB, ND, seed=100 + s)
    if task == "regression":
        yn = (3.0 + 1.5 * np.random.default_rng(500 + s).standard_normal(yn.shape)).astype(np.float32)
    return Xn.astype(np.float32), yn.astype(np.float32)


def _weights(s, rows=B):
    r = np.random.default_rng(900 + s)
    w = r.uniform(0.0, 4.0, rows).astype(np.float32)
    w[r.uniform(size=rows) < 0.2] = 0.0
    return w


def _state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _equal_states(a, b):
    sa, sb = _state(a), _state(b)
    return [k for k in sa if not torch.equal(sa[k], sb[k])]


# ---------------------------------------------------------------------------------------------------------------------
# one weighted step against a float64 replay
# ---------------------------------------------------------------------------------------------------------------------
def _replay64(state, cls, Xn, yn, w):
    """Gradients of sum_b w_b BCE(pred_b, y_b) + L2 in float64 (the oracle's forward on float64 parameters)."""
    from oracle import xdeepfm_oracle as orc
    names, dnames = _names()
    spec = orc.Spec(names, VOCAB, dnames, D, CIN, True, "relu", DNN, CLASSES[cls], l2_reg_dnn=1e-5)
    st = {k: v.double().clone().requires_grad_(v.dtype.is_floating_point) for k, v in state.items()}
    pred = orc.model_forward(T(Xn).double(), st, spec).reshape(-1)
    data = (T(np.asarray(w, dtype=np.float64)) * F.binary_cross_entropy(pred, T(yn).double().reshape(-1), reduction="none")).sum()
    (data + orc.regularization_loss(st, spec).sum()).backward()
    return data.item(), {k: v.grad.numpy() for k, v in st.items() if v.requires_grad and v.grad is not None}


def _tol(g, p):
    """The bars of test_gpu_head_ex.py's gradient comparison (2e-4 relative, 2e-5 of the tensor's largest gradient), plus
    what reading a gradient off an SGD update costs: the update p - lr g is rounded to fp32 once and the difference of
    two fp32 numbers near p is exact, so (before - after) / lr is off by at most 2^-24 max|p| / lr."""
    return 2e-4 * np.abs(g) + 2e-5 * float(np.abs(g).max()) + 1e-9 + 2.0 ** -24 * float(np.abs(p).max()) / LR


@pytest.mark.parametrize("cls", list(CLASSES))
def test_weighted_train_step_against_a_float64_replay(cls):
    Xn, yn = _batch(0)
    w = _weights(0)
    dev = _dev()
    model = _model(dev, cls, optimizer="sgd", spread=0.2)
    before = _state(model)
    # on the CPU first: the weights matter -- unweighted gradients lie more than 10 tolerances away from the weighted ones
    l64, g64 = _replay64(before, cls, Xn, yn, w)
    _, g64_plain = _replay64(before, cls, Xn, yn, np.ones(B))
    named = [k for k, _ in model.named_parameters()]
    assert sorted(g64) == sorted(named)
    for k in named:
        away = float((np.abs(g64[k] - g64_plain[k]) / _tol(g64[k], before[k].numpy())).max())
        assert away > 10.0, "%s: unweighted and weighted gradients only %.2f tolerances apart" % (k, away)
    y_pred, loss, total = model.train_on_batch(T(Xn).to(dev), T(yn).to(dev), T(w).to(dev))
    torch.cuda.synchronize()
    after = _state(model)
    assert abs(loss.item() - l64) <= 2e-5 * abs(l64), (loss.item(), l64)
    worst = {}
    for k in named:
        got = (before[k].double().numpy() - after[k].double().numpy()) / LR
        worst[k] = float((np.abs(got - g64[k]) / _tol(g64[k], before[k].numpy())).max())
    print("%s: share of the bar per parameter %s" % (cls, {k: round(v, 3) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if v > 1.0}


def test_unit_weights_give_the_bits_of_no_weights_after_three_steps():
    dev = _dev()
    a, b = _model(dev), _model(dev)
    ones = torch.ones(B, device=dev)
    for s in range(3):
        Xn, yn = _batch(s)
        oa = a.train_on_batch(T(Xn).to(dev), T(yn).to(dev))
        ob = b.train_on_batch(T(Xn).to(dev), T(yn).to(dev), ones)
        assert torch.equal(oa[1], ob[1]) and torch.equal(oa[2].reshape(-1), ob[2].reshape(-1)) and torch.equal(oa[0], ob[0])
    assert not _equal_states(a, b)


def test_regression_mse_with_weights_runs_through_the_native_head():
    dev = _dev()
    model = _model(dev, task="regression", loss="mse", spread=0.1)
    Xn, yn = _batch(1, task="regression")
    w = _weights(1)
    x, y, wd = T(Xn).to(dev), T(yn).to(dev), T(w).to(dev)
    y_pred, loss = model._loss_forward(x, y, wd)
    assert "Head" in type(loss.grad_fn).__name__ or "Head" in type(loss.grad_fn.next_functions[0][0]).__name__, loss.grad_fn
    want = float((w.astype(np.float64) * (y_pred.detach().cpu().double().numpy().reshape(-1) - yn.reshape(-1)) ** 2).sum())
    assert abs(loss.item() - want) <= 2e-5 * want
    _, plain = model._loss_forward(x, y)
    assert abs(plain.item() - loss.item()) > 1e-2 * abs(plain.item())
    out = model.train_on_batch(x, y, wd)
    assert abs(out[1].item() - want) <= 2e-5 * want and np.isfinite(out[2].item())


def test_stock_tail_on_the_gpu_takes_weights():
    """A loss callable the native head does not know: BaseModel._loss_forward weights loss_func(..., reduction='none')."""
    dev = _dev()
    custom = lambda p, t, reduction="sum": F.binary_cross_entropy(p, t, reduction=reduction)
    a, b = _model(dev, graph=False), _model(dev, graph=False)
    a.loss_func = custom
    Xn, yn = _batch(2)
    w = _weights(2)
    x, y, wd = T(Xn).to(dev), T(yn).to(dev), T(w).to(dev)
    assert a._fused_head(x, y, wd) is None
    la = a._loss_forward(x, y, wd)[1].item()
    lb = b._loss_forward(x, y, wd)[1].item()                     # the native head
    assert abs(la - lb) <= 2e-5 * abs(lb)
    oa, ob = a.train_on_batch(x, y, wd), b.train_on_batch(x, y, wd)
    assert abs(oa[2].item() - ob[2].item()) <= 2e-5 * abs(ob[2].item())


# ---------------------------------------------------------------------------------------------------------------------
# captured weighted step
# ---------------------------------------------------------------------------------------------------------------------
def test_captured_weighted_step_equals_its_eager_twin():
    from xdfm_amd import graphstep
    if os.environ.get("XDFM_HIP_GRAPH", "1") == "0":
        pytest.skip("XDFM_HIP_GRAPH=0")
    dev = _dev()
    g, e = _model(dev), _model(dev, graph=False)
    for s in range(6):
        Xn, yn = _batch(s)
        wd = T(_weights(s)).to(dev)
        og = g.train_on_batch(T(Xn).to(dev), T(yn).to(dev), wd)
        oe = e.train_on_batch(T(Xn).to(dev), T(yn).to(dev), wd)
        assert torch.equal(og[1].reshape(-1), oe[1].reshape(-1)) and torch.equal(og[2].reshape(-1), oe[2].reshape(-1)), \
            "step %d: losses (%r, %r) vs eager (%r, %r)" % (s, og[1].item(), og[2].item(), oe[1].item(), oe[2].item())
    sg, se = g.__dict__["_graphed_step"], e.__dict__["_graphed_step"]
    assert se.replays == 0 and sg.replays > 0 and not sg.disabled, (sg.replays, sg.disabled)
    diff = _equal_states(g, e)
    assert not diff, "captured and eager weighted steps differ in %s" % diff
    graphs = [ent for ent in sg.entries.values() if ent.graph is not None]
    assert len(graphs) == 1 and graphs[0].sw is not None and graphs[0].sw.shape == (B,)
    n, n_memset, n_other = graphstep.census(graphs[0].graph)
    # the unweighted capture of the same model
    u = _model(dev)
    for s in range(3):
        Xn, yn = _batch(s)
        u.train_on_batch(T(Xn).to(dev), T(yn).to(dev))
    ugraphs = [ent for ent in u.__dict__["_graphed_step"].entries.values() if ent.graph is not None]
    assert len(ugraphs) == 1 and ugraphs[0].sw is None
    n_u = graphstep.census(ugraphs[0].graph)[0]
    print("captured train step: weighted %d nodes (%d memset, %d other), unweighted %d" % (n, n_memset, n_other, n_u))
    assert n == n_u and n > 20 and n_memset == 0 and n_other == 0
    # an unweighted step on the weighted model is a graph of its own, not the weighted one with stale weights
    Xn, yn = _batch(7)
    g.train_on_batch(T(Xn).to(dev), T(yn).to(dev))
    assert len(sg.entries) == 2


# ---------------------------------------------------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------------------------------------------------
def _fit_inputs(n, seed=40):
    Xn, yn = _batch(seed, rows=n)
    names, dnames = _names()
    return Xn, yn, (lambda A: {k: A[:, i] for i, k in enumerate(names + dnames)})


def test_fit_with_weight_two_equals_fit_on_every_row_twice():
    """Every example at weight 2 and batch 32, against the data with every row repeated twice and batch 64, shuffle off:
    the same batches, the same objective.  SGD, 2 epochs of 3 steps.  The two runs differ by summation order only: a
    gradient is a sum over 32 rows of doubled terms (doubling is exact) in one run and over 64 rows in the other, so an
    element differs by a few gamma(64) = 64 * 2^-24 of the sum of its absolute row contributions; with a cancellation
    factor and a depth of layers of 25 between them that is 1e-4 of the gradient, hence of the distance a tensor has
    moved (SGD: lr times the summed gradients), plus one rounding of the parameter itself per step."""
    dev = _dev()
    n = 96
    Xn, yn, as_dict = _fit_inputs(n)
    a = _model(dev, optimizer="sgd", spread=0.2)
    b = _model(dev, optimizer="sgd", spread=0.2)
    start = _state(a)
    ha = a.fit(as_dict(Xn), yn, batch_size=32, epochs=2, verbose=0, shuffle=False, sample_weight=np.full(n, 2.0))
    idx = np.repeat(np.arange(n), 2)
    hb = b.fit(as_dict(Xn[idx]), yn[idx], batch_size=64, epochs=2, verbose=0, shuffle=False)
    sa, sb = _state(a), _state(b)
    steps = 6
    for k in sa:
        moved = float((sb[k] - start[k]).abs().max())
        tol = 1e-4 * moved + steps * 2.0 ** -24 * float(sb[k].abs().max())
        err = float((sa[k] - sb[k]).abs().max())
        assert moved > 0 and err <= tol, "%s: |weighted - repeated| %.3g, bar %.3g (moved %.3g)" % (k, err, tol, moved)
    # History: (sum of weighted data loss + L2) / sample_num -- the repeated run divides the same sums by twice the rows
    np.testing.assert_allclose(np.array(ha.history["loss"]), 2.0 * np.array(hb.history["loss"]), rtol=1e-5)


def test_class_weight_equals_the_equivalent_sample_weight_bit_for_bit():
    dev = _dev()
    n = 150                                            # 64 + 64 + 22: a ragged tail
    Xn, yn, as_dict = _fit_inputs(n, seed=41)
    assert 0 < yn.mean() < 1
    # a model is built right before its fit: the constructor seeds torch's generator, which draws the epochs' orders
    a = _model(dev)
    ha = a.fit(as_dict(Xn), yn, batch_size=64, epochs=2, verbose=0, shuffle=True, class_weight={0: 0.5, 1: 3.0})
    b = _model(dev)
    hb = b.fit(as_dict(Xn), yn, batch_size=64, epochs=2, verbose=0, shuffle=True,
               sample_weight=np.where(yn.reshape(-1) == 1, 3.0, 0.5))
    assert ha.history["loss"] == hb.history["loss"]
    assert not _equal_states(a, b)
    c = _model(dev)
    hc = c.fit(as_dict(Xn), yn, batch_size=64, epochs=2, verbose=0, shuffle=True)
    assert hc.history["loss"] != ha.history["loss"] and len(_equal_states(a, c)) > 0
    # validation_split cuts the weights like y: the first rows train, with their own weights
    split, sw = 0.2, _weights(3, n)
    split_at = int(n * (1. - split))
    assert 64 < split_at < n
    d = _model(dev)
    d.fit(as_dict(Xn), yn, batch_size=64, epochs=1, verbose=0, shuffle=True, validation_split=split, sample_weight=sw)
    e = _model(dev)
    e.fit(as_dict(Xn[:split_at]), yn[:split_at], batch_size=64, epochs=1, verbose=0, shuffle=True, sample_weight=sw[:split_at])
    assert not _equal_states(d, e)
    f = _model(dev)
    f.fit(as_dict(Xn[:split_at]), yn[:split_at], batch_size=64, epochs=1, verbose=0, shuffle=True, sample_weight=sw[n - split_at:])
    assert len(_equal_states(d, f)) > 0                # other rows' weights train another model


def test_pro_models_refuse_a_weight_and_train_without_one():
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.xdeepfm_pro import xDeepFMPro, xDeepFMProLight
    dev = _dev()
    names, dnames = _names()
    cols = [SparseFeat(n, v, D) for n, v in zip(names, VOCAB)] + [DenseFeat(n, 1) for n in dnames]
    Xn, yn = _batch(5)
    yn[0, 0] = 1.0
    x, y = T(Xn).to(dev), T(yn).to(dev)
    for cls in (xDeepFMPro, xDeepFMProLight):
        model = cls(cols, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, l2_reg_dnn=1e-5, device=dev,
                    sfg_hidden_units=(64, 32), sfg_dropout=0.0)
        model.compile("adam", "binary_crossentropy", metrics=[])
        model.train()
        before = _state(model)
        with pytest.raises(NotImplementedError, match="sample_weight"):
            model.train_on_batch(x, y, torch.ones(B, device=dev))
        with pytest.raises(NotImplementedError, match="sample_weight"):
            model.fit({k: Xn[:, i] for i, k in enumerate(names + dnames)}, yn, batch_size=B, epochs=1, verbose=0,
                      class_weight={0: 1.0, 1: 2.0})
        assert all(torch.equal(v, before[k]) for k, v in _state(model).items())        # nothing was trained
        out = model.train_on_batch(x, y)
        assert np.isfinite(out[2].item())
        assert any(not torch.equal(v, before[k]) for k, v in _state(model).items())
