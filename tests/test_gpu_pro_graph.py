"""The xDeepFMPro train step replayed from a captured graph (static SFG route: K11 + K9 by a device-side count) against
the same model on the dynamic route with eager launches (XDFM_HIP_GRAPH=0 XDFM_PRO_GRAPH=0): per-step losses, the
state_dict after 15 steps and the History of `fit`, within the tolerance tests/test_gpu_pro.py grants the product against
the reference after three steps (rtol 2e-4, atol 2e-6).  Full batches of 64 rows and a tail of 40; one batch without a
positive row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T = torch.from_numpy

VOCAB, ND, D, B, TAIL = [50, 300, 77, 120, 64, 211], 3, 8, 64, 40
FULL_STEPS, TAIL_STEPS, EMPTY_STEP = 12, 3, 6
VARIANTS = {"default": {}, "all_rows": dict(sfg_positive_only=False), "autodis": dict(use_autodis=True)}
RTOL, ATOL = 2e-4, 2e-6


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _batch(s, rows, positives=True):
    from oracle import xdeepfm_oracle as orc
    Xn, _ = orc.synthetic_batch(rows, VOCAB, ND, seed=300 + s)
    rng = np.random.default_rng(900 + s)
    yn = (rng.random((rows, 1)) < 0.3).astype(np.float32)                      # about 30 % positives
    yn[0, 0] = 1.0
    if not positives:
        yn[:] = 0.0
    return Xn.astype(np.float32), yn


def _schedule():
    return [_batch(s, B, positives=s != EMPTY_STEP) for s in range(FULL_STEPS)] + \
           [_batch(100 + s, TAIL) for s in range(TAIL_STEPS)]


def _model(dev, kw, state=None):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.xdeepfm_pro import xDeepFMProLight
    from xdfm_amd import graphstep
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(VOCAB)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(ND)]
    model = xDeepFMProLight(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev,
                            sfg_hidden_units=(64, 32), sfg_dropout=0.0, **kw)
    if state is not None:
        model.load_state_dict(state)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    step = graphstep.GraphedStep(model)           # reads XDFM_HIP_GRAPH now
    model.__dict__["_graphed_step"] = step
    return model, step


def _env(monkeypatch, graph):
    monkeypatch.setenv("XDFM_HIP_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("XDFM_PRO_GRAPH", "1" if graph else "0")


def _steps(monkeypatch, dev, kw, graph, state=None):
    _env(monkeypatch, graph)
    model, step = _model(dev, kw, state)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    log = []
    for Xn, yn in _schedule():
        _, loss, total = model.train_on_batch(T(Xn).to(dev), T(yn).to(dev))
        log.append([float(loss.reshape(-1)[0]), float(total.reshape(-1)[0]), float(model._step_log[1].reshape(-1)[0])])
    torch.cuda.synchronize()
    return model, step, np.array(log), init


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_replayed_pro_step_matches_the_eager_dynamic_route(monkeypatch, variant):
    from xdfm_amd import ops
    dev = _dev()
    kw = VARIANTS[variant]
    fused_before = ops.VocabHeadsCE.calls
    m_g, step_g, log_g, init = _steps(monkeypatch, dev, kw, True)
    assert m_g._sfg_static() and m_g._optim_capturable
    # Python ran for 2 eager steps + 1 capture per batch shape
    assert ops.VocabHeadsCE.calls - fused_before == 6
    m_e, step_e, log_e, _ = _steps(monkeypatch, dev, kw, False, state=init)
    assert not m_e._sfg_static() and not m_e._optim_capturable and step_e.replays == 0
    print("%s: replays %d, disabled %s, nodes %s" % (variant, step_g.replays, step_g.disabled,
                                                     [e.nodes for e in step_g.entries.values()]))
    print("losses (graph | eager):\n%s" % np.concatenate([log_g, log_e], axis=1))
    assert step_g.replays >= 10 and not step_g.disabled, (step_g.replays, step_g.disabled)
    graphs = [e for e in step_g.entries.values() if e.graph is not None]
    assert len(graphs) == 2 and all(e.nodes > 20 for e in graphs), [e.nodes for e in graphs]     # full batch and tail
    if variant != "all_rows":                                                   # no positive row: a replay with a count of 0
        assert log_g[EMPTY_STEP, 2] == 0.0 and log_e[EMPTY_STEP, 2] == 0.0
    assert (np.delete(log_g[:, 2], EMPTY_STEP) > 0).all()
    for k, name in enumerate(("loss", "total_loss", "sfg_loss")):
        np.testing.assert_allclose(log_g[:, k], log_e[:, k], rtol=RTOL, atol=ATOL, err_msg=name)
    sd_e = m_e.state_dict()
    for k, v in m_g.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), sd_e[k].cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg="after 15 steps " + k)


def _fit(monkeypatch, dev, kw, graph, state=None):
    _env(monkeypatch, graph)
    model, step = _model(dev, kw, state)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    parts = [_batch(40 + s, B, positives=s != 1) for s in range(3)] + [_batch(140, TAIL)]
    Xn, yn = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    names = list(model.feature_index.keys())
    hist = model.fit({n: Xn[:, i] for i, n in enumerate(names)}, yn, batch_size=B, epochs=2, verbose=0, shuffle=False)
    return model, step, hist.history, init


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_fit_history_of_the_replayed_step(monkeypatch, variant):
    """Two epochs of three full batches and a tail: the full batches of the second epoch are replays, between them the
    tail runs its eager warm-up steps.  The epoch's `sfg_loss` is read from the tensors of the graph that ran (kept per
    captured graph), not from whatever step ran Python last."""
    dev = _dev()
    kw = VARIANTS[variant]
    m_g, step_g, h_g, init = _fit(monkeypatch, dev, kw, True)
    m_e, step_e, h_e, _ = _fit(monkeypatch, dev, kw, False, state=init)
    print("%s: history graph %s | eager %s; replays %d" % (variant, h_g, h_e, step_g.replays))
    assert step_g.replays >= 4 and not step_g.disabled and step_e.replays == 0
    assert sorted(h_g.keys()) == sorted(h_e.keys()) and "sfg_loss" in h_g
    assert all(v > 0 for v in h_e["sfg_loss"])
    for k in h_g:
        np.testing.assert_allclose(h_g[k], h_e[k], rtol=RTOL, atol=ATOL, err_msg=k)


def test_many_batch_shapes_keep_their_tables(monkeypatch):
    """Ten batch shapes, three steps each (the third is captured), then one more step of each of the six shapes whose graphs
    are still held: every captured step addresses its own field table and plan items, which the model's kept state must
    still own -- the replays agree with the eager twin."""
    from xdfm_amd import graphstep
    dev = _dev()
    sizes = [64, 40, 33, 72, 96, 50, 61, 80, 45, 57]
    sched = [(s, rows) for s, rows in enumerate(sizes) for _ in range(3)] + \
            [(20 + s, rows) for s, rows in enumerate(sizes[-graphstep.MAX_GRAPHS:])]

    def run(graph, state=None):
        _env(monkeypatch, graph)
        model, step = _model(dev, {}, state)
        init = {k: v.detach().clone() for k, v in model.state_dict().items()}
        log = []
        for i, (s, rows) in enumerate(sched):
            Xn, yn = _batch(400 + 7 * s + i, rows)
            _, loss, total = model.train_on_batch(T(Xn).to(dev), T(yn).to(dev))
            log.append([float(loss.reshape(-1)[0]), float(total.reshape(-1)[0]), float(model._step_log[1].reshape(-1)[0])])
        return model, step, np.array(log), init
    m_g, step_g, log_g, init = run(True)
    m_e, step_e, log_e, _ = run(False, init)
    (_, _, state), = [m_g.__dict__["_sfg_cols"]]
    print("replays %d, tables %d, graphs held %d" % (step_g.replays, len(state.tables), len(step_g.entries)))
    assert not step_g.disabled and step_g.replays == len(sizes) + graphstep.MAX_GRAPHS and step_e.replays == 0
    assert len(state.tables) == len(sizes)                                     # one per batch shape, none dropped
    np.testing.assert_allclose(log_g, log_e, rtol=RTOL, atol=ATOL)


def test_hand_driven_model_is_not_captured(monkeypatch):
    """forward_with_sfg + the caller's own backward, the loss kept alive (what a user-driven loop does), then train_on_batch:
    the model says once that it gives up graph replay and every step launches eagerly -- no capture is attempted."""
    dev = _dev()
    _env(monkeypatch, True)
    model, step = _model(dev, {})
    assert model._optim_capturable
    Xn, yn = _batch(1, B)
    xb, yb = T(Xn).to(dev), T(yn).to(dev)
    with pytest.warns(UserWarning, match="driven by hand"):
        y_pred, info = model.forward_with_sfg(xb, yb)
    keep = torch.nn.functional.binary_cross_entropy(y_pred.squeeze(), yb.squeeze(), reduction="sum") + info["sfg_loss"]
    keep.backward()
    model.optim.zero_grad()
    assert not model._optim_capturable
    for s in range(4):
        Xn, yn = _batch(2 + s, B)
        model.train_on_batch(T(Xn).to(dev), T(yn).to(dev))
    torch.cuda.synchronize()
    assert step.replays == 0 and not step.disabled and not step.entries
    assert keep.grad_fn is not None


@pytest.mark.parametrize("dtype", [torch.float64, torch.int64])
def test_labels_of_another_dtype_select_the_same_rows(monkeypatch, dtype):
    """`labels == 1` of the dynamic route takes any dtype; the static route casts before K11 reads floats."""
    dev = _dev()
    _env(monkeypatch, True)
    model, _ = _model(dev, {})
    Xn, yn = _batch(3, B)
    xb = T(Xn).to(dev)
    with torch.no_grad():
        emb_fm, dnn_in, _ = model.fused_inputs(xb)
        want, _ = model.compute_sfg_loss_fused(xb, dnn_in, T(yn).to(dev))
        got, _ = model.compute_sfg_loss_fused(xb, dnn_in, T(yn).to(dev).to(dtype))
    assert float(want) > 0 and torch.equal(want, got)
