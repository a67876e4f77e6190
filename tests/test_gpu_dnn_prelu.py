"""GPU tests (-m gpu) of dnn_activation='prelu' through ops.DensePReLU / ops.dense_prelu, ops.PReLU / ops.prelu,
layers.DNN(activation='prelu') and captured train steps of the models.

Bar for y, dx, dW, db (that of tests/test_gpu_dnn.py).  The native result's largest error against float64 may exceed the
largest error of the STOCK composition on the same device (F.linear + F.prelu under autograd) by at most a factor 2, with a
floor of one fp32 ulp of the output's largest magnitude.  The backward of all three -- native, stock, float64 -- takes the
SAME pre-activation z (the native forward's): a z within rounding of zero must not sit on the slope's branch in one run and
on the identity's in another, the runs would differentiate different functions.
Bar for dalpha: |dalpha - exact| <= ulp32(exact) + cells * 2^-53 * sum |g z| (tests/dnn_prelu_ref.py, dalpha_bound): what the
double accumulation and the one final rounding give; stock torch is not the yardstick there.

Every test sets ops.DNN_PRELU_NATIVE (and ops.DNN_NATIVE where it matters) itself, so the file runs both routes whatever the
switch's default is."""
import copy
import faulthandler
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dnn_prelu_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy

STEP_LIMIT_S = 120
FACTOR = 2.0
_REF = {}


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _judge(tag, native, stock, ref):
    bad = []
    for key, want in ref.items():
        want = want.detach().cpu().double()
        e_nat = float((native[key].detach().cpu().double() - want).abs().max())
        e_stock = float((stock[key].detach().cpu().double() - want).abs().max())
        floor = float(np.spacing(np.float32(want.abs().max())))
        print("%-30s %-8s native %.3e  stock %.3e  floor (1 ulp) %.3e" % (tag, key, e_nat, e_stock, floor))
        assert native[key].shape == want.shape, key
        if not e_nat <= max(FACTOR * e_stock, floor):
            bad.append((key, e_nat, e_stock, floor))
    assert not bad, (tag, bad)


def _judge_dalpha(tag, got, g, z, alpha):
    gn, zn = g.detach().cpu().numpy(), z.detach().cpu().numpy()
    exact = R.prelu_bwd_ref(gn, zn, alpha)[1]
    bound = R.dalpha_bound(gn, zn, exact)
    err = abs(float(got.detach().cpu().double().reshape(-1)[0]) - exact)
    print("%-30s dalpha   native %.3e  bound %.3e  (exact %.9g)" % (tag, err, bound, exact))
    assert tuple(got.shape) == (1,) and err <= bound, (tag, err, bound)


def _count(monkeypatch, ops):
    """Calls of the three routes: the fused layer, the native elementwise op, torch's own prelu."""
    calls = dict(fused=0, elementwise=0, torch=0)
    real_f, real_e, real_t = ops._dense_prelu_fused, ops._prelu_native, F.prelu

    def fused(*a):
        calls["fused"] += 1
        return real_f(*a)

    def elementwise(*a):
        calls["elementwise"] += 1
        return real_e(*a)

    def stock(*a, **k):
        calls["torch"] += 1
        return real_t(*a, **k)

    monkeypatch.setattr(ops, "_dense_prelu_fused", fused)
    monkeypatch.setattr(ops, "_prelu_native", elementwise)
    monkeypatch.setattr(torch.nn.functional, "prelu", stock)
    return calls


def _profile(ops, fn):
    ops.PROFILE = []
    try:
        out = fn()
        names = [p[0] for p in ops.PROFILE]
    finally:
        ops.PROFILE = None
    return out, names


# ------------------------------------------------------------------------------------------ one layer against float64
LAYER_CASES = {"r520_40_64": (520, 40, 64, False), "r4099_256_256": (4099, 256, 256, False), "window_r300_45_96": (300, 45, 96, True)}


def _window(t, pad_l, pad_r):
    wide = torch.full((t.shape[0], pad_l + t.shape[1] + pad_r), 1e6, dtype=t.dtype, device=t.device)
    wide[:, pad_l:pad_l + t.shape[1]] = t
    return wide[:, pad_l:pad_l + t.shape[1]]


def _layer_inputs(name, dev):
    if name not in _REF:
        rows, k, out, _ = LAYER_CASES[name]
        gen = torch.Generator().manual_seed(rows + out)
        x = torch.randn(rows, k, generator=gen)
        W = torch.randn(out, k, generator=gen) / float(np.sqrt(k))
        _REF[name] = (x, W, torch.randn(out, generator=gen), torch.randn(rows, out, generator=gen))
    return tuple(t.to(dev) for t in _REF[name])


@pytest.mark.parametrize("alpha", [0.25, -0.3])
@pytest.mark.parametrize("name", list(LAYER_CASES))
def test_fused_layer_error_against_float64(monkeypatch, name, alpha):
    from xdfm_amd import ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", True)
    monkeypatch.setattr(ops, "DNN_NATIVE", True)
    x0, W0, b0, g0 = _layer_inputs(name, dev)
    strided = LAYER_CASES[name][3]
    leaf = lambda t: t.clone().requires_grad_(True)
    # native: its own forward; z is what it saved
    W, b, a = leaf(W0), leaf(b0), torch.tensor([alpha], device=dev, requires_grad=True)
    xin = (_window(x0, 2, 5) if strided else x0.clone()).requires_grad_(True)
    assert xin.is_contiguous() != strided
    assert ops.dense_prelu_native(xin, W, b, a)
    y = ops.dense_prelu(xin, W, b, a)
    assert isinstance(y.grad_fn, ops.DensePReLU._backward_cls)
    z = y.grad_fn.saved_tensors[2].clone()
    gin = _window(g0, 3, 1) if strided else g0
    y.backward(gin)
    native = dict(y=y.detach(), dx=xin.grad, dW=W.grad, db=b.grad)
    # stock: its own forward for y; the backward from the same z
    with torch.no_grad():
        y_s = F.prelu(F.linear(x0, W0, b0), torch.tensor([alpha], device=dev))
    zl, al = leaf(z), torch.tensor([alpha], device=dev, requires_grad=True)
    F.prelu(zl, al).backward(g0)
    gz = zl.grad
    stock = dict(y=y_s, dx=gz.mm(W0), dW=gz.t().mm(x0), db=gz.sum(0))
    # float64
    xn, Wn, bn, gn, zn = (t.detach().cpu().numpy() for t in (x0, W0, b0, g0, z))
    y_ref, _ = R.layer_ref(xn, Wn, bn, float(np.float32(alpha)))
    dx_ref, dW_ref, db_ref, _ = R.layer_bwd_ref(gn, zn, float(np.float32(alpha)), xn, Wn)
    ref = dict(y=T(y_ref), dx=T(dx_ref), dW=T(dW_ref), db=T(db_ref))
    tag = "%s_alpha%g" % (name, alpha)
    _judge(tag, native, stock, ref)
    _judge_dalpha(tag, a.grad, g0, z, alpha)
    zc = z.cpu()
    assert 0 < int((zc > 0).sum()) < zc.numel()


@pytest.mark.parametrize("alpha", [0.25, -0.3])
@pytest.mark.parametrize("shape,strided", [((520, 40), False), ((4099, 256), False), ((300, 45), True)])
def test_elementwise_error_against_float64(shape, strided, alpha):
    from xdfm_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(shape[0])
    u0, g0 = torch.randn(*shape, generator=gen).to(dev), torch.randn(*shape, generator=gen).to(dev)
    u0[0, 0] = 0.0
    u = (_window(u0, 2, 5) if strided else u0.clone()).requires_grad_(True)
    a = torch.tensor([alpha], device=dev, requires_grad=True)
    assert ops.prelu_native(u, a)
    y = ops.prelu(u, a)
    assert isinstance(y.grad_fn, ops.PReLU._backward_cls)
    y.backward(_window(g0, 1, 2) if strided else g0)
    ul, al = u0.clone().requires_grad_(True), torch.tensor([alpha], device=dev, requires_grad=True)
    ys = F.prelu(ul, al)
    ys.backward(g0)
    du_ref, _ = R.prelu_bwd_ref(g0.cpu().numpy(), u0.cpu().numpy(), float(np.float32(alpha)))
    ref = dict(y=T(R.prelu_ref(u0.cpu().numpy(), float(np.float32(alpha)))), du=T(du_ref))
    tag = "elementwise_%dx%d_alpha%g" % (shape + (alpha,))
    _judge(tag, dict(y=y.detach(), du=u.grad), dict(y=ys.detach(), du=ul.grad), ref)
    _judge_dalpha(tag, a.grad, g0, u0, alpha)


# ------------------------------------------------------------------------------------------ routing
ROUTES = {  # what: (fused, elementwise, torch) calls of a three-layer tower 40 -> 64 -> 32 -> 96 (or as noted)
    "fused": (3, 0, 0), "unfused": (0, 3, 0), "switch_off": (0, 3, 0), "width40": (2, 1, 0), "use_bn": (0, 3, 0),
    "float64": (0, 0, 3), "cpu": (0, 0, 3), "evaluation": (3, 0, 0)}


@pytest.mark.parametrize("what", list(ROUTES))
def test_routing(monkeypatch, what):
    """fused: both switches on.  unfused: XDFM_DNN_NATIVE off (the fused route needs it).  switch_off: XDFM_DNN_PRELU_NATIVE
    off.  width40: a layer outside xdfm_dense_supported.  A GPU fp32 tower never reaches torch's prelu."""
    from xdfm_amd import layers, ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", what != "switch_off")
    monkeypatch.setattr(ops, "DNN_NATIVE", what != "unfused")
    calls = _count(monkeypatch, ops)
    hidden = (64, 40, 96) if what == "width40" else (64, 32, 96)
    where = torch.device("cpu") if what == "cpu" else dev
    net = layers.DNN(40, hidden, activation="prelu", use_bn=what == "use_bn", init_std=0.3, device=where)
    with torch.no_grad():
        for m, v in zip(net.activation_layers, (0.4, -0.3, 0.0)):
            m.weight.fill_(v)
    x = torch.randn(70, 40, generator=torch.Generator().manual_seed(2)).to(where)
    if what == "float64":
        net, x = net.double(), x.double()
    if what == "evaluation":
        net.eval()
        with torch.no_grad():
            (out, names) = _profile(ops, lambda: net(x))
        assert names == ["dense_prelu_fwd"] * 3
        net.train()
        want = net(x)                                        # the same y with and without the stored pre-activation
        assert torch.equal(out, want.detach())
        calls["fused"] -= 3
    else:
        net.train()
        x.requires_grad_(True)
        out = net(x)
        out.sum().backward()
        for q in [x] + list(net.parameters()):
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), what
    assert (calls["fused"], calls["elementwise"], calls["torch"]) == ROUTES[what], (what, calls)
    assert bool(torch.isfinite(out).all()) and out.shape == (70, 96)
    assert list(net.state_dict().keys())[-3:] == ["activation_layers.%d.weight" % i for i in range(3)]


# ------------------------------------------------------------------------------------------ needs_input_grad
def test_needs_input_grad_combinations_return_the_full_calls_bits_and_launch_only_what_is_needed(monkeypatch):
    from xdfm_amd import ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", True)
    monkeypatch.setattr(ops, "DNN_NATIVE", True)
    x0, W0, b0, g0 = _layer_inputs("r520_40_64", dev)

    def run(needs):
        ts = [t.clone().requires_grad_(n) for t, n in zip((x0, W0, b0, torch.tensor([-0.3], device=dev)), needs)]

        def go():
            y = ops.dense_prelu(*ts)
            if any(needs):
                y.backward(g0)
            return y.detach()
        y, names = _profile(ops, go)
        return [y] + [t.grad for t in ts], names

    full, names = run((True,) * 4)
    assert names == ["dense_prelu_fwd", "dense_prelu_bwd_x", "dense_prelu_bwd_w"] and all(t is not None for t in full)
    for code in range(15):
        needs = tuple(bool(code >> i & 1) for i in range(4))
        got, names = run(needs)
        want_names = ["dense_prelu_fwd"] + (["dense_prelu_bwd_x"] if needs[0] else []) + (["dense_prelu_bwd_w"] if any(needs[1:]) else [])
        assert names == want_names, (needs, names)
        assert torch.equal(_bits(got[0]), _bits(full[0]))
        for key, t, want, n in zip(("dx", "dW", "db", "dalpha"), got[1:], full[1:], needs):
            assert (t is not None and torch.equal(_bits(t), _bits(want))) if n else t is None, (needs, key)

    # the elementwise op
    def run_e(needs):
        u, a = x0.clone().requires_grad_(needs[0]), torch.tensor([-0.3], device=dev, requires_grad=needs[1])

        def go():
            y = ops.prelu(u, a)
            if any(needs):
                y.backward(x0 * 0.5)
            return y.detach()
        y, names = _profile(ops, go)
        return [y, u.grad, a.grad], names

    full, names = run_e((True, True))
    assert names == ["prelu_fwd", "prelu_bwd"]
    for needs in ((True, False), (False, True), (False, False)):
        got, names = run_e(needs)
        assert names == (["prelu_fwd", "prelu_bwd"] if any(needs) else ["prelu_fwd"])
        assert torch.equal(_bits(got[0]), _bits(full[0]))
        for t, want, n in zip(got[1:], full[1:], needs):
            assert (t is not None and torch.equal(_bits(t), _bits(want))) if n else t is None, needs


# ------------------------------------------------------------------------------------------ towers against float64
def _compose(net, x, masks, training=True, keep=None):
    """The tower as stock torch ops in net's own precision and on its device, with each layer's branch taken from `masks`
    (pre-activation > 0 of the native run) instead of the layer's own sign test.  keep: a list that receives every layer's
    pre-activation, its gradient retained."""
    h = x
    for i, lin in enumerate(net.linears):
        v = F.linear(h, lin.weight, lin.bias)
        if net.use_bn:
            bn = net.bn[i]
            v = F.batch_norm(v, None, None, bn.weight, bn.bias, training, bn.momentum, bn.eps)
        if keep is not None:
            v.retain_grad()
            keep.append(v)
        h = torch.where(masks[i].to(v.device), v, net.activation_layers[i].weight * v)
    return h


def _randomise(net, gen, dev):
    with torch.no_grad():
        for lin in net.linears:
            lin.weight.copy_((torch.randn(lin.weight.shape, generator=gen) / float(np.sqrt(lin.weight.shape[1]))).to(dev))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen).to(dev))
        for bn in getattr(net, "bn", []):
            bn.weight.copy_((0.5 + torch.rand(bn.weight.shape, generator=gen)).to(dev))
            bn.bias.copy_((0.5 * torch.randn(bn.bias.shape, generator=gen)).to(dev))
        for m, v in zip(net.activation_layers, (0.4, -0.3, 0.25)):
            m.weight.fill_(v)


@pytest.mark.parametrize("use_bn", [False, True], ids=["plain", "bn"])
def test_tower_against_stock_and_a_float64_replay(monkeypatch, use_bn):
    """layers.DNN(13, (32, 96, 40), 'prelu') at 65 rows: the output and every gradient, the slopes' to their own bound.  Width
    40 is outside xdfm_dense_supported: that layer runs the library GEMMs and the elementwise kernels."""
    from xdfm_amd import layers, ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", True)
    monkeypatch.setattr(ops, "DNN_NATIVE", True)
    rows, k, hidden = 65, 13, (32, 96, 40)
    gen = torch.Generator().manual_seed(1618 + use_bn)
    net0 = layers.DNN(k, hidden, activation="prelu", use_bn=use_bn, device=dev)
    _randomise(net0, gen, dev)
    x0, g0 = torch.randn(rows, k, generator=gen).to(dev), torch.randn(rows, hidden[-1], generator=gen).to(dev)
    zs = []                                   # the native run's pre-activations, layer by layer
    real_f, real_e = ops._dense_prelu_fused, ops._prelu_native
    monkeypatch.setattr(ops, "_dense_prelu_fused", lambda *a: (lambda y: (zs.append(y.grad_fn.saved_tensors[2].detach().clone()), y)[1])(real_f(*a)))
    monkeypatch.setattr(ops, "_prelu_native", lambda u, a: (zs.append(u.detach().clone()), real_e(u, a))[1])
    calls = _count(monkeypatch, ops)

    def grads(net, x, out):
        out.backward(g0.to(out.dtype).to(out.device))
        res = dict(out=out.detach(), dx=x.grad)
        for kname, p in net.named_parameters():
            res[kname] = p.grad
        return res

    net = copy.deepcopy(net0).train()
    x = x0.clone().requires_grad_(True)
    native = grads(net, x, net(x))
    assert (calls["fused"], calls["elementwise"], calls["torch"]) == ((0, 3, 0) if use_bn else (2, 1, 0)) and len(zs) == 3
    masks = [z > 0 for z in zs]
    net_s = copy.deepcopy(net0).train()
    xs = x0.clone().requires_grad_(True)
    stock = grads(net_s, xs, _compose(net_s, xs, masks))
    net_r = copy.deepcopy(net0).cpu().double().train()
    xr = x0.cpu().double().requires_grad_(True)
    vs = []
    ref = grads(net_r, xr, _compose(net_r, xr, [m.cpu() for m in masks], keep=vs))
    slopes = [kname for kname in ref if "activation_layers" in kname]
    assert len(slopes) == 3
    skip = set(slopes) | (set(kname for kname in ref if kname.startswith("linears") and kname.endswith("bias")) if use_bn else set())
    tag = "tower_r65_13_32_96_40_%s" % ("bn" if use_bn else "plain")
    _judge(tag, native, stock, {kname: v for kname, v in ref.items() if kname not in skip})
    # The slopes.  dalpha_i = sum over z <= 0 of g z with g the layer's upstream gradient and z its pre-activation: both are
    # results of this run's fp32 contractions, so the kernel's own double accumulation is not what limits the agreement with a
    # float64 replay.  First-order forward error of fp32 contractions of total length n feeding a term is n * 2^-24 of it
    # (n: the tower's widths, through which every g and z has passed at most once each), hence
    #     |dalpha - replay| <= ulp32(replay) + n * 2^-24 * sum |g z|     with sum |g z| taken from the replay;
    # a single scalar's error against the stock run's is one noise against another, so the factor-2 rule is only the alternative.
    n_chain = k + sum(hidden)
    for i, kname in enumerate(slopes):
        exact = float(ref[kname].reshape(-1)[0])
        got = float(native[kname].double().reshape(-1)[0])
        e_stock = abs(float(stock[kname].double().reshape(-1)[0]) - exact)
        closed = ~masks[i].cpu()
        bound = R.ulp32(exact) + n_chain * 2.0 ** -24 * float((vs[i].grad * vs[i].detach()).abs()[closed].sum())
        print("%-30s %-28s native %.3e  stock %.3e  bound %.3e" % (tag, kname, abs(got - exact), e_stock, bound))
        assert abs(got - exact) <= max(FACTOR * e_stock, bound), (kname, got, exact, e_stock, bound)
    if use_bn:
        # biases in front of a batch norm, zero in exact arithmetic: the bound of tests/golden/make_golden_bn.py (rows fp32 values of
        # the size of the layer's largest weight gradient, each off by half an ulp, times 8 of margin)
        big = max(float(v.abs().max()) for kname, v in ref.items() if kname.startswith("linears") and kname.endswith("weight"))
        for kname in skip - set(slopes):
            assert float(native[kname].abs().max()) <= 8.0 * rows * 2.0 ** -24 * max(big, 1.0), kname


def test_tower_with_dropout_in_training_keeps_nn_dropout(monkeypatch):
    """dropout_rate = 0.5: nn.Dropout behind every PReLU.  Checked through the zeros pattern and the 1 / (1 - p) scale only."""
    from xdfm_amd import layers, ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", True)
    monkeypatch.setattr(ops, "DNN_NATIVE", True)
    calls = _count(monkeypatch, ops)
    torch.manual_seed(11)
    net = layers.DNN(13, (32, 96, 40), activation="prelu", dropout_rate=0.5, init_std=0.5, device=dev).train()
    seen = []
    net.dropout.register_forward_hook(lambda _m, inp, out: seen.append((inp[0].detach(), out.detach())))
    x = torch.randn(257, 13, device=dev, requires_grad=True)
    out = net(x)
    out.sum().backward()
    assert len(seen) == 3 and (calls["fused"], calls["elementwise"], calls["torch"]) == (2, 1, 0)
    assert net.last_drop_seed is None, "the hashed mask of the ReLU kernels is not drawn for prelu"
    for inp, o in seen:
        kept = o != 0
        frac = float(kept.float().mean())
        assert 0.4 < frac < 0.6, frac
        assert torch.equal(o[kept], (inp * 2.0)[kept]) and bool((inp[~kept] != 0).any())
    assert torch.equal(out.detach(), seen[-1][1]) and bool(torch.isfinite(x.grad).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    net.eval()
    with torch.no_grad():
        ev = net(x.detach())
    assert len(seen) == 6 and all(torch.equal(i, o) for i, o in seen[3:]) and bool(torch.isfinite(ev).all())


# ------------------------------------------------------------------------------------------ captured step
def _small_xdeepfm(dev, use_graph=True, use_bn=False, hidden=(64, 32)):
    """The model of tests/test_gpu_dnn_bn.py::_small_xdeepfm with dnn_activation='prelu'."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    vocab, nd, Dm = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, Dm) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    torch.manual_seed(7)
    model = xDeepFM(cols, cols, dnn_hidden_units=hidden, cin_layer_size=(16, 8), l2_reg_dnn=1e-5, dnn_dropout=0, dnn_use_bn=use_bn,
                    dnn_activation="prelu", device=dev)
    with torch.no_grad():
        for m, v in zip(model.dnn.activation_layers, (0.4, -0.3)):
            m.weight.fill_(v)
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


@pytest.mark.parametrize("route", ["fused", "switch_off", "bn"])
def test_five_replays_equal_five_eager_steps_bit_for_bit_without_a_memset_node(monkeypatch, route):
    from xdfm_amd import graphstep, ops
    monkeypatch.setenv("XDFM_HIP_GRAPH", "1")
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", route != "switch_off")
    monkeypatch.setattr(ops, "DNN_NATIVE", True)
    runs = {}
    for key, use_graph in (("graph", True), ("eager", False)):
        calls = _count(monkeypatch, ops)
        model, step, vocab, nd = _small_xdeepfm(dev, use_graph, use_bn=route == "bn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _train(model, vocab, nd, dev, graphstep.EAGER_STEPS_BEFORE_CAPTURE)
            losses = _train(model, vocab, nd, dev, 5, first=graphstep.EAGER_STEPS_BEFORE_CAPTURE)
        assert not [w for w in caught if "capture" in str(w.message)], [str(w.message) for w in caught]
        assert all(np.isfinite(losses)), (key, losses)
        assert calls["torch"] == 0 and (calls["fused"] > 0) == (route == "fused") and (calls["elementwise"] > 0) == (route != "fused")
        graphs = [e for e in step.entries.values() if e.graph is not None]
        if use_graph:
            assert step.replays == 5 and not step.disabled and len(graphs) == 1, (key, step.replays, step.disabled)
            n, n_memset, n_other = graphstep.census(graphs[0].graph)
            print("captured train step, dnn_activation='prelu', %s: %d nodes (%d memset, %d other)" % (route, n, n_memset, n_other))
            assert n > 20 and n_memset == 0 and n_other == 0
        else:
            assert step.replays == 0
        runs[key] = (model, losses)
    assert runs["graph"][1] == runs["eager"][1], "the five losses"
    sd_g, sd_e = runs["graph"][0].state_dict(), runs["eager"][0].state_dict()
    assert list(sd_g.keys()) == list(sd_e.keys())
    for k in sd_g:
        assert torch.equal(sd_g[k], sd_e[k]), "%s differs between five replays and five eager steps" % k
    for i, v in enumerate((0.4, -0.3)):                      # the replays saw the optimizer's updates: the slopes moved
        assert float(sd_g["dnn.activation_layers.%d.weight" % i]) != np.float32(v)


def test_state_dict_round_trip_between_the_switch_settings_and_to_the_cpu(monkeypatch):
    from xdfm_amd import ops
    monkeypatch.setenv("XDFM_HIP_GRAPH", "0")
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_NATIVE", True)
    for first in (True, False):
        monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", first)
        a, _, vocab, nd = _small_xdeepfm(dev, use_graph=False)
        _train(a, vocab, nd, dev, 3)
        sd = {k: v.clone() for k, v in a.state_dict().items()}
        monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", not first)
        b, _, _, _ = _small_xdeepfm(dev, use_graph=False)
        assert list(b.state_dict().keys()) == list(sd.keys())
        assert [k for k in sd if "activation_layers" in k] == ["dnn.activation_layers.0.weight", "dnn.activation_layers.1.weight"]
        b.load_state_dict(sd, strict=True)
        X, _ = _batch(50, vocab, nd, dev, rows=200)
        names = list(b.feature_index.keys())
        feed = {n: X[:, i].cpu().numpy() for i, n in enumerate(names)}
        pred_b = b.predict(feed, batch_size=64)
        monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", first)
        pred_a = a.predict(feed, batch_size=64)
        print("predict from one state: largest difference between the switch settings %.3e" % float(np.abs(pred_a - pred_b).max()))
        np.testing.assert_allclose(pred_a, pred_b, rtol=1e-4, atol=2e-6)
        # ... and to the CPU: the tower alone, stock torch there
        from xdfm_amd import layers
        cpu = layers.DNN(a.dnn.linears[0].in_features, (64, 32), activation="prelu", device="cpu")
        cpu.load_state_dict({k: v.cpu() for k, v in a.dnn.state_dict().items()}, strict=True)
        h = torch.randn(50, a.dnn.linears[0].in_features, generator=torch.Generator().manual_seed(1))
        a.eval()
        with torch.no_grad():
            np.testing.assert_allclose(a.dnn(h.to(dev)).cpu().numpy(), cpu.eval()(h).numpy(), rtol=1e-4, atol=2e-6)
        b.train()
        monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", not first)
        assert all(np.isfinite(_train(b, vocab, nd, dev, 2, first=3)))


@pytest.mark.parametrize("cls_name", ["xDeepFMAttention", "xDeepFMPro"])
def test_one_step_smoke_of_the_other_models(monkeypatch, cls_name):
    """dnn_activation passes through: one train step, finite loss, the slopes hold a gradient's worth of movement."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from xdfm_amd import ops
    monkeypatch.setenv("XDFM_HIP_GRAPH", "0")
    monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", True)
    monkeypatch.setattr(ops, "DNN_NATIVE", True)
    dev = _dev()
    calls = _count(monkeypatch, ops)
    vocab, nd, D = [50, 31, 77, 12], 2, 8
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    torch.manual_seed(3)
    if cls_name == "xDeepFMPro":
        from deepctr.xdeepfm_pro import xDeepFMPro
        model = xDeepFMPro(cols, cols, dnn_hidden_units=(32, 8), cin_layer_size=(6, 4), l2_reg_dnn=1e-5, device=dev,
                           sfg_hidden_units=(8, 6), sfg_dropout=0.0, dnn_activation="prelu")
    else:
        from deepctr import models
        model = models.xDeepFMAttention(cols, cols, dnn_hidden_units=(32, 8), cin_layer_size=(6, 4), l2_reg_dnn=1e-5, cin_num_heads=2,
                                        dnn_activation="prelu", device=dev)
    keys = [k for k in model.state_dict() if "activation_layers" in k]
    assert keys == ["dnn.activation_layers.0.weight", "dnn.activation_layers.1.weight"]
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    out = model.train_on_batch(*_batch(1, vocab, nd, dev, rows=96))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o.detach()).all()) for o in out if isinstance(o, torch.Tensor))
    assert calls["fused"] >= 1 and calls["elementwise"] >= 1 and calls["torch"] == 0
    for k in keys:
        assert float(model.state_dict()[k]) != 0.25, k


# ------------------------------------------------------------------------------------------ goldens of the reference
def _golden_model(g, dev):
    from deepctr import models
    from deepctr.inputs import DenseFeat, SparseFeat
    D = int(g["emb_dim"])
    cols = [SparseFeat("C%d" % (i + 1), int(v), D) for i, v in enumerate(g["vocab"])]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(int(g["n_dense"]))]
    return models.xDeepFM(cols, cols, dnn_hidden_units=tuple(int(v) for v in g["dnn"]), cin_layer_size=tuple(int(v) for v in g["cin"]),
                          l2_reg_dnn=1e-5, dnn_use_bn=bool(g["use_bn"]), dnn_activation="prelu", device=dev)


def _close(got, want, rtol, atol, msg):
    np.testing.assert_allclose(got.detach().cpu().numpy().reshape(np.shape(want)), want, rtol=rtol, atol=atol, err_msg=msg)


@pytest.mark.parametrize("name", ["prelu_xdeepfm", "prelu_xdeepfm_bn"])
def test_native_model_vs_reference_golden(monkeypatch, name):
    """The bars of tests/test_gpu_dnn_bn.py::test_native_model_vs_reference_golden.  The golden's layers (8 and 5 wide) are
    outside xdfm_dense_supported: they run the library GEMMs and the elementwise kernels; the slopes' gradients carry the
    reference's L2 term and the slopes move as the reference's do."""
    from xdfm_amd import ops
    monkeypatch.setenv("XDFM_HIP_GRAPH", "0")
    monkeypatch.setattr(ops, "DNN_PRELU_NATIVE", True)
    dev = _dev()
    calls = _count(monkeypatch, ops)
    g = load_golden("dnn_prelu/" + name)
    model = _golden_model(g, dev)
    for k, v in model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), g["init:" + k], err_msg="init " + k)
    assert list(model.state_dict().keys()) == [k[5:] for k in g if k.startswith("init:")]
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
    assert calls["elementwise"] == 2 and calls["torch"] == 0
    _close(y_pred, g["y_pred"], 2e-5, 1e-6, "y_pred")
    assert abs(loss.item() - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    assert abs(reg.item() - float(g["reg"])) <= 1e-5 * abs(float(g["reg"]))
    slopes = 0
    for k, p in model.named_parameters():
        want = g["g:" + k]
        if k in zero:
            assert float(p.grad.abs().max()) <= float(g["zero_grad_bound"]), (k, float(p.grad.abs().max()))
            continue
        slopes += "activation_layers" in k
        _close(p.grad, want, 2e-4, 2e-5 * float(np.abs(want).max()) + 1e-9, "grad " + k)
    assert slopes == 2
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
    for i in range(2):
        k = "dnn.activation_layers.%d.weight" % i
        assert float(model.state_dict()[k]) != float(g["s0:" + k][0])
