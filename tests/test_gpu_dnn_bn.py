"""GPU tests (-m gpu) of the native batch norm of the DNN tower through ops.BatchNormAct / ops.bn_act, layers.DNN(use_bn=True)
and a captured train step of an xDeepFM with dnn_use_bn=True.

Bar (that of tests/test_gpu_dnn.py).  For each output the native result's largest error against a float64 replay may exceed
the largest error of the STOCK route (nn.BatchNorm1d + torch.relu / torch.sigmoid, ops.DNN_BN_NATIVE off) on the same inputs
by at most a factor 2, with a floor of one fp32 ulp of the output's largest magnitude.  The float64 replay takes its ReLU
masks from the fp32 activations of the native run (a pre-activation within rounding of zero must not be open in one
precision and closed in the other: the two would differentiate different functions).

Every test sets ops.DNN_BN_NATIVE itself, so the file runs the native route whatever the switch's default is."""
import copy
import faulthandler
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy

STEP_LIMIT_S = 120
FACTOR = 2.0


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _judge(tag, native, stock, ref):
    bad = []
    for key, want in ref.items():
        want = want.detach().cpu().double()
        e_nat = float((native[key].detach().cpu().double() - want).abs().max())
        e_stock = float((stock[key].detach().cpu().double() - want).abs().max())
        floor = float(np.spacing(np.float32(want.abs().max())))
        print("%-26s %-22s native %.3e  stock %.3e  floor (1 ulp) %.3e" % (tag, key, e_nat, e_stock, floor))
        assert native[key].shape == want.shape, key
        if not e_nat <= max(FACTOR * e_stock, floor):
            bad.append((key, e_nat, e_stock, floor))
    assert not bad, (tag, bad)


def _count_native(monkeypatch, ops):
    calls = []
    real = ops._bn_act_native
    monkeypatch.setattr(ops, "_bn_act_native", lambda z, bn, code, training: (calls.append((code, training)), real(z, bn, code, training))[1])
    return calls


# ------------------------------------------------------------------------------------------ routing
@pytest.mark.parametrize("what", ["train", "eval", "sigmoid", "switch_off", "float64", "cpu", "row_parallel"])
def test_routing(monkeypatch, what):
    """A training or evaluating use_bn tower on the GPU takes the native branch of ops.bn_act once per layer; none with the
    switch off, with a float64 tower, on the CPU or while a row-parallel context is current."""
    from xdfm_amd import dist as xdist
    from xdfm_amd import layers, ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_BN_NATIVE", what != "switch_off")
    calls = _count_native(monkeypatch, ops)
    if what == "row_parallel":
        monkeypatch.setattr(xdist, "current", lambda: object())
    act = "sigmoid" if what == "sigmoid" else "relu"
    where = torch.device("cpu") if what == "cpu" else dev
    net = layers.DNN(40, (64, 40, 32), activation=act, use_bn=True, init_std=0.3, device=where)
    x = torch.randn(70, 40, generator=torch.Generator().manual_seed(2)).to(where)
    if what == "float64":
        net, x = net.double(), x.double()
    net.train(what != "eval")
    x.requires_grad_(True)
    out = net(x)
    out.sum().backward()
    native = what in ("train", "eval", "sigmoid")
    code = ops.ACT_CODES[act]
    assert calls == ([(code, what != "eval")] * 3 if native else []), (what, calls)
    assert bool(torch.isfinite(out).all()) and out.shape == (70, 32)
    for q in [x] + list(net.parameters()):
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), what
    want_tracked = 0 if what == "eval" else 1
    assert [int(b.num_batches_tracked) for b in net.bn] == [want_tracked] * 3
    assert list(net.state_dict().keys())[-5:] == ["bn.2.weight", "bn.2.bias", "bn.2.running_mean", "bn.2.running_var", "bn.2.num_batches_tracked"]


# ------------------------------------------------------------------------------------------ tower against float64
def _randomise(net, gen, dev):
    with torch.no_grad():
        for lin in net.linears:
            lin.weight.copy_((torch.randn(lin.weight.shape, generator=gen) / float(np.sqrt(lin.weight.shape[1]))).to(dev))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen).to(dev))
        for bn in net.bn:
            bn.weight.copy_((0.5 + torch.rand(bn.weight.shape, generator=gen)).to(dev))
            bn.bias.copy_((0.5 * torch.randn(bn.bias.shape, generator=gen)).to(dev))
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=gen).to(dev))
            bn.running_var.copy_((0.5 + torch.rand(bn.running_var.shape, generator=gen)).to(dev))


def _labels(net):
    out = []
    for i in range(len(net.linears)):
        out += ["dW%d" % i, "db%d" % i]
    for i in range(len(net.bn)):
        out += ["dgamma%d" % i, "dbeta%d" % i]
    return out


def _run_tower(net, xs, g0):
    """Three training calls (the first one differentiated), then one evaluation call on the first input."""
    x = xs[0].clone().requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    net.train()
    out = net(x)
    out.backward(g0)
    res = dict(out=out.detach().clone(), dx=x.grad.clone())
    for label, p in zip(_labels(net), net.parameters()):
        res[label] = p.grad.clone()
    with torch.no_grad():
        for xk in xs[1:]:
            net(xk)
    for i, bn in enumerate(net.bn):
        res["running_mean%d" % i], res["running_var%d" % i] = bn.running_mean.clone(), bn.running_var.clone()
        assert int(bn.num_batches_tracked) == len(xs)
    net.eval()
    with torch.no_grad():
        res["eval_out"] = net(xs[0]).clone()
    for i, bn in enumerate(net.bn):
        assert torch.equal(bn.running_mean, res["running_mean%d" % i]) and int(bn.num_batches_tracked) == len(xs), "evaluation touched a buffer"
    return res


def _replay64(net0, act, xs, g0, masks):
    """The same three calls and the evaluation call in float64 on the CPU; `masks` (one per layer, from the fp32 activations of
    the native run's first call) replace relu's own `> 0` in the differentiated call."""
    net = copy.deepcopy(net0).cpu().double()
    mom, eps = net.bn[0].momentum, net.bn[0].eps

    def forward(h, training, use_masks):
        for i, (lin, bn) in enumerate(zip(net.linears, net.bn)):
            v = F.batch_norm(F.linear(h, lin.weight, lin.bias), bn.running_mean, bn.running_var, bn.weight, bn.bias, training, mom, eps)
            if act == "sigmoid":
                h = torch.sigmoid(v)
            else:
                h = v * masks[i].double() if use_masks else torch.relu(v)
        return h

    x = xs[0].cpu().double().requires_grad_(True)
    out = forward(x, True, True)
    out.backward(g0.cpu().double())
    res = dict(out=out.detach(), dx=x.grad)
    for label, p in zip(_labels(net), net.parameters()):
        res[label] = p.grad
    with torch.no_grad():
        for xk in xs[1:]:
            forward(xk.cpu().double(), True, False)
        for i, bn in enumerate(net.bn):
            res["running_mean%d" % i], res["running_var%d" % i] = bn.running_mean.clone(), bn.running_var.clone()
        res["eval_out"] = forward(xs[0].cpu().double(), False, False)
    return res


@pytest.mark.parametrize("act", ["relu", "sigmoid"])
def test_tower_native_against_stock_and_a_float64_replay(monkeypatch, act):
    """layers.DNN(13, (32, 96, 40), use_bn=True) at 65 rows: outputs, every gradient, the buffers after three training calls and
    the evaluation output.  Width 40 is outside xdfm_dense_supported: that layer's dz enters the library GEMMs and xdfm_colsum,
    the other two enter the native dX / dW kernels with y = NULL."""
    from xdfm_amd import layers, ops
    dev = _dev()
    rows, k, hidden = 65, 13, (32, 96, 40)
    gen = torch.Generator().manual_seed(2718 + len(act))
    net0 = layers.DNN(k, hidden, activation=act, use_bn=True, device=dev)
    _randomise(net0, gen, dev)
    xs = [torch.randn(rows, k, generator=gen).to(dev) for _ in range(3)]
    g0 = torch.randn(rows, hidden[-1], generator=gen).to(dev)
    assert ops.DNN_NATIVE and not ops.dense_native(torch.empty(rows, 96, device=dev), net0.linears[2].weight)
    assert ops.dense_native(xs[0], net0.linears[0].weight)
    runs, acts = {}, []
    for native in (True, False):
        monkeypatch.setattr(ops, "DNN_BN_NATIVE", native)
        net = copy.deepcopy(net0)
        if native:
            real = ops._bn_act_native
            monkeypatch.setattr(ops, "_bn_act_native", lambda *a: (lambda y: (acts.append(y.detach()), y)[1])(real(*a)))
            ops.PROFILE = []
        try:
            runs[native] = _run_tower(net, xs, g0)
            names = [p[0] for p in ops.PROFILE] if native else None
        finally:
            ops.PROFILE = None
            if native:
                monkeypatch.setattr(ops, "_bn_act_native", real)
        if native:
            assert len(acts) == 3 * 3 + 3, "three layers, three training calls and the evaluation call"
            first = [n for n in names if n.startswith("bn_") or n.startswith("dense_bwd")][:10]
            assert first == ["bn_fwd_train"] * 3 + ["bn_bwd", "bn_bwd", "dense_bwd_x", "dense_bwd_w", "bn_bwd", "dense_bwd_x", "dense_bwd_w"], names
            assert names.count("bn_fwd_train") == 9 and names.count("bn_fwd_eval") == 3
    masks = [(a > 0).cpu() for a in acts[:3]]
    if act == "relu":
        for a in acts[:3]:
            assert 0 < int((a == 0).sum()) < a.numel()
    ref = _replay64(net0, act, xs, g0, masks)
    _judge("tower_r65_13_32_96_40_%s" % act, runs[True], runs[False], ref)


def test_needs_input_grad_combinations_return_the_full_calls_bits_and_launch_only_what_is_needed(monkeypatch):
    from xdfm_amd import ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_BN_NATIVE", True)
    rows, cols = 65, 40
    gen = torch.Generator().manual_seed(99)
    z0 = torch.randn(rows, cols, generator=gen).to(dev)
    g0 = torch.randn(rows, cols, generator=gen).to(dev)
    bn0 = torch.nn.BatchNorm1d(cols).to(dev)
    with torch.no_grad():
        bn0.weight.copy_((0.5 + torch.rand(cols, generator=gen)).to(dev))
        bn0.bias.copy_(torch.randn(cols, generator=gen).to(dev))

    def run(needs, training=True):
        bn = copy.deepcopy(bn0)
        bn.train(training)
        z = z0.clone().requires_grad_(needs[0])
        bn.weight.requires_grad_(needs[1])
        bn.bias.requires_grad_(needs[2])
        assert ops.bn_native(z, bn)
        ops.PROFILE = []
        try:
            y = ops.bn_act(z, bn, "relu", training)
            if any(needs):
                y.backward(g0)
            names = [p[0] for p in ops.PROFILE]
        finally:
            ops.PROFILE = None
        return (y.detach(), z.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone()), names

    for training, fwd, bwd in ((True, "bn_fwd_train", "bn_bwd"), (False, "bn_fwd_eval", "bn_bwd_eval")):
        full, names = run((True, True, True), training)
        assert names == [fwd, bwd] and all(t is not None for t in full)
        for needs in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True),
                      (False, False, False)):
            got, names = run(needs, training)
            assert names == ([fwd, bwd] if any(needs) else [fwd]), (training, needs, names)
            assert torch.equal(got[0], full[0]) and torch.equal(got[4], full[4]) and torch.equal(got[5], full[5])
            for key, t, want, w in zip(("dz", "dgamma", "dbeta"), got[1:4], full[1:4], needs):
                if w:
                    assert t is not None and torch.equal(t, want), (training, needs, key)
                else:
                    assert t is None, (training, needs, key)
    # evaluation: the statistics are constants -- against autograd of the stock sequence in evaluation mode
    bn = copy.deepcopy(bn0).eval()
    z = z0.clone().requires_grad_(True)
    torch.relu(bn(z)).backward(g0)
    full, _ = run((True, True, True), False)
    for got, want in ((full[1], z.grad), (full[2], bn.weight.grad), (full[3], bn.bias.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_one_row_raises_in_training_and_runs_in_evaluation(monkeypatch):
    from xdfm_amd import layers, ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_BN_NATIVE", True)
    calls = _count_native(monkeypatch, ops)
    net = layers.DNN(13, (32, 40), use_bn=True, init_std=0.3, device=dev)
    x = torch.randn(1, 13, generator=torch.Generator().manual_seed(3)).to(dev)
    net.train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        net(x)
    assert len(calls) == 1 and [int(b.num_batches_tracked) for b in net.bn] == [0, 0]
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        torch.nn.BatchNorm1d(32).to(dev).train()(torch.zeros(1, 32, device=dev))          # the stock module's own refusal
    net.eval()
    with torch.no_grad():
        out = net(x)
    assert out.shape == (1, 40) and bool(torch.isfinite(out).all()) and len(calls) == 3


# ------------------------------------------------------------------------------------------ captured step
def _small_xdeepfm(dev, use_graph=True):
    """The model of tests/test_gpu_dnn_dropout.py::_small_xdeepfm with dnn_use_bn=True."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    vocab, nd, Dm = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, Dm) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    torch.manual_seed(7)
    model = xDeepFM(cols, cols, dnn_hidden_units=(64, 32), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, dnn_dropout=0, dnn_use_bn=True, device=dev)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    step = graphstep.GraphedStep(model)
    step.disabled = not use_graph
    model.__dict__["_graphed_step"] = step
    return model, step, vocab, nd


def _batch(s, vocab, nd, dev, rows=128):
    from oracle import xdeepfm_oracle as orc
    X, y = orc.synthetic_batch(rows, vocab, nd, seed=500 + s)
    return T(X).to(dev), T(y).to(dev)


def _train(model, vocab, nd, dev, steps, first=0):
    losses = []
    for s in range(first, first + steps):
        out = model.train_on_batch(*_batch(s, vocab, nd, dev))
        losses.append(float(out[2].detach().reshape(-1)[0]))
    torch.cuda.synchronize()
    return losses


def _tracked(model):
    return [int(b.num_batches_tracked) for b in model.dnn.bn]


def test_five_replays_equal_five_eager_steps_bit_for_bit_and_the_graph_is_smaller(monkeypatch):
    from xdfm_amd import graphstep, ops
    monkeypatch.setenv("XDFM_HIP_GRAPH", "1")
    dev = _dev()
    models = {}
    for key, native, use_graph in (("graph", True, True), ("eager", True, False), ("stock_graph", False, True)):
        monkeypatch.setattr(ops, "DNN_BN_NATIVE", native)
        calls = _count_native(monkeypatch, ops)
        model, step, vocab, nd = _small_xdeepfm(dev, use_graph)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _train(model, vocab, nd, dev, graphstep.EAGER_STEPS_BEFORE_CAPTURE)              # the eager steps in front of the capture
            assert _tracked(model) == [graphstep.EAGER_STEPS_BEFORE_CAPTURE] * 2
            for b in model.dnn.bn:
                b.num_batches_tracked.zero_()                                                # count the next five steps alone
            losses = _train(model, vocab, nd, dev, 5, first=graphstep.EAGER_STEPS_BEFORE_CAPTURE)
        assert not [w for w in caught if "capture" in str(w.message)], [str(w.message) for w in caught]
        assert all(np.isfinite(losses)), (key, losses)
        graphs = [e for e in step.entries.values() if e.graph is not None]
        if use_graph:
            assert step.replays == 5 and not step.disabled and len(graphs) == 1, (key, step.replays, step.disabled)
            assert len(calls) == (2 * 3 if native else 0), "Python ran for two eager steps and the capture: two hidden layers each"
        else:
            assert step.replays == 0 and len(calls) == 2 * 7
        assert _tracked(model) == [5, 5], (key, _tracked(model))
        models[key] = (model, graphs[0].nodes if graphs else None, losses)
    g, e = models["graph"][0], models["eager"][0]
    assert models["graph"][2] == models["eager"][2], "the five losses"
    sd_g, sd_e = g.state_dict(), e.state_dict()
    assert list(sd_g.keys()) == list(sd_e.keys())
    for k in sd_g:
        assert torch.equal(sd_g[k], sd_e[k]), "%s differs between five replays and five eager steps" % k
    assert any("dnn.bn.0.running_var" in k for k in sd_g)
    n_native, n_stock = models["graph"][1], models["stock_graph"][1]
    print("captured train step, dnn_use_bn=True: %d nodes natively, %d with XDFM_DNN_BN_NATIVE off" % (n_native, n_stock))
    assert n_native < n_stock


def test_state_dict_round_trip_between_the_routes_and_predict_agrees(monkeypatch):
    """A checkpoint trained natively loads into a model that continues on the stock route and the other way round, keys
    identical; from one state the two routes' predictions agree within the bar the golden tests hold `predict` to (rtol 1e-4,
    atol 2e-6: evaluation mode, running statistics -- a sum-order difference only)."""
    from xdfm_amd import ops
    monkeypatch.setenv("XDFM_HIP_GRAPH", "0")
    dev = _dev()
    for first_native in (True, False):
        monkeypatch.setattr(ops, "DNN_BN_NATIVE", first_native)
        calls = _count_native(monkeypatch, ops)
        a, _, vocab, nd = _small_xdeepfm(dev, use_graph=False)
        _train(a, vocab, nd, dev, 3)
        assert (len(calls) > 0) == first_native
        sd = {k: v.clone() for k, v in a.state_dict().items()}
        monkeypatch.setattr(ops, "DNN_BN_NATIVE", not first_native)
        calls = _count_native(monkeypatch, ops)
        b, _, _, _ = _small_xdeepfm(dev, use_graph=False)
        assert list(b.state_dict().keys()) == list(sd.keys())
        assert [k for k in sd if k.startswith("dnn.bn.1.")] == ["dnn.bn.1." + n for n in ("weight", "bias", "running_mean", "running_var",
                                                                                          "num_batches_tracked")]
        b.load_state_dict(sd, strict=True)
        X, _ = _batch(50, vocab, nd, dev, rows=200)
        names = list(b.feature_index.keys())
        feed = {n: X[:, i].cpu().numpy() for i, n in enumerate(names)}
        pred_b = b.predict(feed, batch_size=64)
        monkeypatch.setattr(ops, "DNN_BN_NATIVE", first_native)
        pred_a = a.predict(feed, batch_size=64)
        monkeypatch.setattr(ops, "DNN_BN_NATIVE", not first_native)
        print("predict from one state: largest difference between the routes %.3e" % float(np.abs(pred_a - pred_b).max()))
        np.testing.assert_allclose(pred_a, pred_b, rtol=1e-4, atol=2e-6)
        b.train()                                                      # predict() left the model in evaluation mode
        losses = _train(b, vocab, nd, dev, 2, first=3)
        assert all(np.isfinite(losses)) and _tracked(b) == [5, 5]
        assert (len([c for c in calls if c[1]]) > 0) == (not first_native), "b's two training steps (a's native predict also lands here)"


# ------------------------------------------------------------------------------------------ golden of the reference
def _golden_model(g, dev):
    from deepctr import models
    from deepctr.inputs import DenseFeat, SparseFeat
    D = int(g["emb_dim"])
    cols = [SparseFeat("C%d" % (i + 1), int(v), D) for i, v in enumerate(g["vocab"])]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(int(g["n_dense"]))]
    return models.xDeepFM(cols, cols, dnn_hidden_units=tuple(int(v) for v in g["dnn"]), cin_layer_size=tuple(int(v) for v in g["cin"]),
                          l2_reg_dnn=1e-5, dnn_use_bn=True, dnn_activation=str(g["act"]), device=dev)


def _close(got, want, rtol, atol, msg):
    np.testing.assert_allclose(got.detach().cpu().numpy().reshape(np.shape(want)), want, rtol=rtol, atol=atol, err_msg=msg)


@pytest.mark.parametrize("name", ["bn_xdeepfm_relu", "bn_xdeepfm_sigmoid"])
def test_native_model_vs_reference_golden(monkeypatch, name):
    """The bars of test_gpu_parity.py::test_model_vs_reference_golden; the zero-gradient biases and running_mean as the
    generator's docstring derives (tests/golden/make_golden_bn.py)."""
    from xdfm_amd import ops
    monkeypatch.setenv("XDFM_HIP_GRAPH", "0")
    monkeypatch.setattr(ops, "DNN_BN_NATIVE", True)
    dev = _dev()
    calls = _count_native(monkeypatch, ops)
    g = load_golden("dnn_bn/" + name)
    model = _golden_model(g, dev)
    for k, v in model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), g["init:" + k], err_msg="init " + k)
    model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
    B, zero, lr = int(g["B"]), set(str(k) for k in g["zero_grad_keys"]), float(g["lr"])
    Xd, yd = T(g["X"]).to(dev), T(g["y"]).to(dev)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    model.optim.zero_grad()
    y_pred = model(Xd[:B])
    loss = F.binary_cross_entropy(y_pred.squeeze(), yd[:B].squeeze(), reduction="sum")
    reg = model.get_regularization_loss()
    (loss + reg).backward()
    assert len(calls) == 2
    _close(y_pred, g["y_pred"], 2e-5, 1e-6, "y_pred")
    assert abs(loss.item() - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    assert abs(reg.item() - float(g["reg"])) <= 1e-5 * abs(float(g["reg"]))
    for k, p in model.named_parameters():
        want = g["g:" + k]
        if k in zero:
            assert float(p.grad.abs().max()) <= float(g["zero_grad_bound"]), (k, float(p.grad.abs().max()))
            continue
        _close(p.grad, want, 2e-4, 2e-5 * float(np.abs(want).max()) + 1e-9, "grad " + k)
    for k, v in model.state_dict().items():
        if "a1:" + k in g:
            _close(v, g["a1:" + k], 1e-5, 1e-6, "after the first forward: " + k)
    model.optim.zero_grad()
    losses = []
    for s in range(3):
        out = model.train_on_batch(Xd[s * B:(s + 1) * B], yd[s * B:(s + 1) * B])
        losses.append([float(out[1].detach().reshape(-1)[0]), float(out[2].detach().reshape(-1)[0])])
    print("%s losses %s" % (name, losses))
    np.testing.assert_allclose(np.array(losses), g["losses3"], rtol=2e-5)
    for k, v in model.state_dict().items():
        if k in zero:
            assert float((v.cpu() - T(g["s0:" + k])).abs().max()) <= 3 * lr * 1.0001, k
            continue
        atol = 2e-5 + (float(g["running_mean_allowance"]) if k.endswith("running_mean") else 0.0)
        _close(v, g["s3:" + k], 1e-3, atol, "after 3 steps: " + k)
    assert int(model.dnn.bn[0].num_batches_tracked) == 4 == int(g["s3:dnn.bn.0.num_batches_tracked"])
