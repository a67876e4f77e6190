"""GPU tests (-m gpu) of the DNN tower's native dropout through ops.DenseReLUDropout, layers.DNN, SFGDecoder.hidden_native
and a captured train step, against a float64 reference computed on the CPU from the same fp32 inputs and the keep mask read
back with xdfm_dense_dropout_mask.

Bar (that of tests/test_gpu_dnn.py).  For each output the native result's largest error against float64 may exceed the
largest error of the STOCK composition -- the library GEMMs with the same mask and the same fp32 scale applied by torch ops
-- on the same inputs by at most a factor 2, with a floor of one fp32 ulp of the output's largest magnitude.  Both sum the
same fp32 products in different orders.  DESIGN.md 4.3d lists the measured pairs.

The backward's mask is the native forward's stored output (d > 0) for all three computations, as in tests/test_gpu_dnn.py:
a pre-activation within rounding of zero cannot flip a cell between them.  The gradient entering the float64 sums is
fl32(g * s): the one rounding the kernel and native_dropout_backward both make."""
import faulthandler
import warnings

import numpy as np
import pytest
import torch

import dnn_dropout_ref as D

pytestmark = pytest.mark.gpu
T = torch.from_numpy

STEP_LIMIT_S = 120
FACTOR = 2.0
#  name: (rows, in, out, strided)        the ReLU cases of tests/test_gpu_dnn.py
CASES = {
    "r33_k429_o256": (33, 429, 256, False),
    "r65_k65_o96": (65, 65, 96, False),
    "r2049_k40_o64_strided": (2049, 40, 64, True),
    "r8225_k65_o96": (8225, 65, 96, False),
}
PS = (0.1, 0.5)
_CACHE = {}


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _Ctx:
    def __init__(self, needs=(True, True, True, False, False, False)):
        self.needs_input_grad = needs
        self.saved_tensors = ()
        self.p = None

    def save_for_backward(self, *t):
        self.saved_tensors = t


def _window(t, pad_l, pad_r, fill):
    wide = torch.full((t.shape[0], pad_l + t.shape[1] + pad_r), fill, dtype=t.dtype, device=t.device)
    wide[:, pad_l:pad_l + t.shape[1]] = t
    return wide[:, pad_l:pad_l + t.shape[1]]


def _read_mask(rows, out, p, seed, layer):
    from xdfm_amd import _lib, ops
    keep = torch.empty(rows, out, dtype=torch.uint8, device=seed.device)
    _lib.check(_lib.load().xdfm_dense_dropout_mask(rows, out, float(p), ops._ptr(seed), layer, 0, ops._ptr(keep), ops._stream()),
               "dense_dropout_mask")
    return keep.bool()


def _scale(p, dev):
    return torch.tensor(D.keep_scale(p), dtype=torch.float32, device=dev)


def _judge(tag, native, stock, ref):
    """Print every (native, stock, floor) triple, then assert the bar on all of them."""
    bad = []
    for key, want in ref.items():
        e_nat = float((native[key].detach().cpu().double() - want).abs().max())
        e_lib = float((stock[key].detach().cpu().double() - want).abs().max())
        floor = float(np.spacing(np.float32(want.abs().max())))
        print("%-34s %-4s native %.3e  stock %.3e  floor (1 ulp) %.3e" % (tag, key, e_nat, e_lib, floor))
        assert native[key].shape == want.shape
        if not e_nat <= max(FACTOR * e_lib, floor):
            bad.append((key, e_nat, e_lib, floor))
    assert not bad, (tag, bad)


def _case(name, p):
    key = (name, p)
    if key in _CACHE:
        return _CACHE[key]
    from xdfm_amd import ops
    dev = _dev()
    rows, k, out, strided = CASES[name]
    gen = torch.Generator().manual_seed(1000 + len(name) + rows + k)
    x = torch.randn(rows, k, generator=gen)
    W = torch.randn(out, k, generator=gen) / float(np.sqrt(k))
    b = torch.randn(out, generator=gen)
    g = torch.randn(rows, out, generator=gen)
    xd, Wd, bd, gd = x.to(dev), W.to(dev), b.to(dev), g.to(dev)
    xn = _window(xd, 3, 2, 1e6) if strided else xd
    gn = _window(gd, 1, 4, 1e6) if strided else gd
    seed = torch.tensor([987654321012345 + rows], dtype=torch.int64, device=dev)
    layer = 2
    assert ops.dense_dropout_native(xn, Wd, bd, p), "the case must be inside the native envelope"
    ctx = _Ctx()
    d = ops.DenseReLUDropout.forward(ctx, xn, Wd, bd, p, seed, layer)
    ctx.p = float(p)
    dx, dW, db = ops.DenseReLUDropout.backward(ctx, gn)[:3]
    native = dict(d=d, dx=dx, dW=dW, db=db)
    again = dict(zip(("dx", "dW", "db"), ops.DenseReLUDropout.backward(ctx, gn)[:3]), d=ops.DenseReLUDropout.forward(_Ctx(), xn, Wd, bd, p, seed, layer))
    keep = _read_mask(rows, out, p, seed, layer)
    s = _scale(p, dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    d_lib = torch.where(keep, torch._addmm_activation(bd, xd, Wd.t(), use_gelu=False) * s, zero)
    gz = torch.where(d > 0, gd * s, zero)
    stock = dict(d=d_lib, dx=gz.mm(Wd), dW=gz.t().mm(xd), db=gz.sum(0))
    torch.cuda.synchronize()
    keep_c, d_c = keep.cpu(), d.cpu()
    z6, d6 = D.layer_ref(x, W, b, keep_c.numpy(), p)
    dx6, dW6, db6 = D.layer_bwd_ref(g, d_c, x, W, p)
    c = dict(native=native, stock=stock, again=again, ref=dict(d=d6, dx=dx6, dW=dW6, db=db6), keep=keep_c, z6=z6, x=xn, W=Wd, b=bd, g=gn,
             seed=seed, layer=layer)
    _CACHE[key] = c
    return c


# ------------------------------------------------------------------------------------------ one layer, O(1) inputs
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", list(CASES))
def test_native_error_against_float64_within_twice_the_stock_compositions(name, p):
    c = _case(name, p)
    rows, k, out, _ = CASES[name]
    d, keep = c["native"]["d"].cpu(), c["keep"]
    # the mirror on the CPU gives the bits the device wrote
    assert np.array_equal(keep.numpy(), D.keep_mask(rows, out, p, int(c["seed"].item()), c["layer"]))
    # the stored output is the mask: zero wherever dropped, positive only where kept; the fp32 and float64 signs of z agree
    # away from rounding distance of zero
    assert bool((d[~keep] == 0).all()) and bool((d >= 0).all())
    sure = c["z6"].abs() > 1e-4
    assert bool(((d > 0) == (keep & (c["z6"] > 0)))[sure].all())
    frac = float(keep.double().mean())
    assert abs(frac - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / keep.numel()), frac
    assert 0 < int((d == 0).sum()) < d.numel()
    _judge("%s_p%g" % (name, p), c["native"], c["stock"], c["ref"])


@pytest.mark.parametrize("name", list(CASES))
def test_two_calls_give_the_same_bits(name):
    c = _case(name, 0.5)
    for key, second in c["again"].items():
        assert torch.equal(c["native"][key], second), key


def test_needs_input_grad_combinations_return_the_full_calls_bits_and_launch_only_what_is_needed():
    from xdfm_amd import ops
    c = _case("r65_k65_o96", 0.5)
    saved = ops.PROFILE
    try:
        def run(needs):
            ctx = _Ctx(needs + (False, False, False))
            ops.PROFILE = []
            d = ops.DenseReLUDropout.forward(ctx, c["x"], c["W"], c["b"], 0.5, c["seed"], c["layer"])
            assert len(ctx.saved_tensors) == 3 and ctx.saved_tensors[2] is d, "saved: x, W and the dropped output only"
            got = ops.DenseReLUDropout.backward(ctx, c["g"])
            names = [q[0] for q in ops.PROFILE]
            ops.PROFILE = None
            assert len(got) == 6 and got[3:] == (None, None, None)
            return got[:3], names

        full, names = run((True, True, True))
        assert names == ["dense_fwd_drop", "dense_bwd_x_drop", "dense_bwd_w_drop"]
        for key, t in zip(("dx", "dW", "db"), full):
            assert torch.equal(t, c["native"][key]), key
        for needs, launches in (((False, True, True), ["dense_bwd_w_drop"]), ((True, False, True), ["dense_bwd_x_drop", "dense_bwd_w_drop"]),
                                ((True, True, False), ["dense_bwd_x_drop", "dense_bwd_w_drop"]), ((True, False, False), ["dense_bwd_x_drop"]),
                                ((False, False, True), ["dense_bwd_w_drop"])):
            got, names = run(needs)
            assert names == ["dense_fwd_drop"] + launches, (needs, names)
            for key, t, ref, w in zip(("dx", "dW", "db"), got, full, needs):
                if w:
                    assert t is not None and torch.equal(t, ref), (needs, key)
                else:
                    assert t is None, (needs, key)
    finally:
        ops.PROFILE = saved
    # through autograd: a frozen weight, an input without gradient
    x = c["x"].clone().requires_grad_(True)
    b = c["b"].clone().requires_grad_(True)
    d = ops.dense_relu_dropout(x, c["W"], b, 0.5, c["seed"], c["layer"])
    d.backward(c["g"])
    assert torch.equal(d.detach(), c["native"]["d"]) and torch.equal(x.grad, c["native"]["dx"]) and torch.equal(b.grad, c["native"]["db"])


# ------------------------------------------------------------------------------------------ towers
def _randomise(linears, gen, dev):
    with torch.no_grad():
        for lin in linears:
            lin.weight.copy_((torch.randn(lin.weight.shape, generator=gen) / float(np.sqrt(lin.weight.shape[1]))).to(dev))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen).to(dev))


def _tower_replay(tag, linears, p, seed, x0, g0, out_nat, grads_nat):
    """Judge a tower's output and gradients (dx, then dW, db per layer) against a float64 replay with the layers' read-back
    masks.  The fp32 activations are recomputed layer by layer with the same seed (the same bits the tower produced); the
    backward replay takes its masks and its layer inputs from them."""
    from xdfm_amd import ops
    dev = x0.device
    n = len(linears)
    s = _scale(p, dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    acts, keeps, stock_fwd = [x0], [], x0
    with torch.no_grad():
        for i, lin in enumerate(linears):
            acts.append(ops.dense_relu_dropout(acts[-1], lin.weight, lin.bias, p, seed, i))
            keeps.append(_read_mask(x0.shape[0], lin.weight.shape[0], p, seed, i))
            stock_fwd = torch.where(keeps[-1], torch._addmm_activation(lin.bias, stock_fwd, lin.weight.t(), use_gelu=False) * s, zero)
        assert torch.equal(acts[-1], out_nat), "the tower's output is the chain of dense_relu_dropout calls with its seed"
        # stock backward chain on the same activations
        g, stock = g0, {}
        for i in reversed(range(n)):
            gz = torch.where(acts[i + 1] > 0, g * s, zero)
            stock["dW%d" % i], stock["db%d" % i] = gz.t().mm(acts[i]), gz.sum(0)
            g = gz.mm(linears[i].weight)
        stock["dx"] = g
        stock["out"] = stock_fwd
    torch.cuda.synchronize()
    # float64: the forward from x0 through the masks, the backward from the fp32 activations
    h6 = x0.cpu()
    for i, lin in enumerate(linears):
        h6 = D.layer_ref(h6, lin.weight.detach().cpu(), lin.bias.detach().cpu(), keeps[i].cpu().numpy(), p)[1]
    ref = {"out": h6}
    g6 = g0.cpu().double()               # float64 all the way down the chain: g * s is not rounded to fp32 here
    for i in reversed(range(n)):
        g6, dW6, db6 = D.layer_bwd_ref(g6, acts[i + 1].cpu(), acts[i].cpu(), linears[i].weight.detach().cpu(), p)
        ref["dW%d" % i], ref["db%d" % i] = dW6, db6
    ref["dx"] = g6
    native = dict(out=out_nat, dx=grads_nat[0])
    for i in range(n):
        native["dW%d" % i], native["db%d" % i] = grads_nat[1 + 2 * i], grads_nat[2 + 2 * i]
    _judge(tag, native, stock, ref)
    return keeps, acts


@pytest.mark.parametrize("rows", [33, 520])
def test_tower_against_a_float64_replay_with_the_read_back_masks(rows):
    from xdfm_amd import layers, ops
    dev = _dev()
    k, hidden, p = 429, (256, 256, 64), 0.3
    gen = torch.Generator().manual_seed(4100 + rows)
    net = layers.DNN(k, hidden, activation="relu", dropout_rate=p, use_bn=False, device=dev)
    twin = layers.DNN(k, hidden, activation="relu", dropout_rate=0, use_bn=False, device=dev)
    _randomise(net.linears, gen, dev)
    twin.load_state_dict(net.state_dict())
    x0 = torch.randn(rows, k, generator=gen).to(dev)
    g0 = torch.randn(rows, hidden[-1], generator=gen).to(dev)
    assert ops.DNN_DROPOUT_NATIVE and ops.DNN_NATIVE
    net.train()
    x = x0.clone().requires_grad_(True)
    out = net(x)
    seed = net.last_drop_seed
    assert seed is not None and seed.dtype == torch.int64 and seed.is_cuda and seed.numel() == 1
    out.backward(g0)
    grads = [x.grad] + [q.grad for lin in net.linears for q in (lin.weight, lin.bias)]
    keeps, acts = _tower_replay("tower_r%d_k429_256_256_64_p0.3" % rows, list(net.linears), p, seed, x0, g0, out.detach(), grads)
    # three layers, three masks
    for a, b in ((keeps[0], keeps[1]), (keeps[0][:, :64], keeps[2]), (keeps[1][:, :64], keeps[2])):
        frac = float((a != b).double().mean())
        assert abs(frac - 2 * p * (1 - p)) < 0.05, frac
    for a in acts[1:]:
        assert 0 < int((a == 0).sum()) < a.numel()
    # eval(): no dropout, the bits of a dropout-free twin with the same weights
    net.eval()
    twin.eval()
    with torch.no_grad():
        assert torch.equal(net(x0), twin(x0))
    assert net.last_drop_seed is seed, "eval() draws no seed"


def test_seeds_differ_between_calls_and_follow_torch_manual_seed():
    from xdfm_amd import layers
    dev = _dev()
    net = layers.DNN(40, (64, 32), dropout_rate=0.5, init_std=0.3, device=dev)
    net.train()
    x = torch.randn(70, 40, generator=torch.Generator().manual_seed(1)).to(dev)
    torch.manual_seed(1234)
    o1, s1 = net(x).detach().clone(), int(net.last_drop_seed.item())
    o2, s2 = net(x).detach().clone(), int(net.last_drop_seed.item())
    assert s1 != s2 and not torch.equal(o1, o2)
    assert 0 <= s1 < 2 ** 62 and 0 <= s2 < 2 ** 62
    torch.manual_seed(1234)
    o3, s3 = net(x).detach().clone(), int(net.last_drop_seed.item())
    assert s3 == s1 and torch.equal(o3, o1)


@pytest.mark.parametrize("what", ["native", "out40", "sigmoid", "use_bn", "p1", "switch_off", "dnn_native_off", "eval", "p0"])
def test_routing(monkeypatch, what):
    """Only a training ReLU tower without batch norm, 0 < p < 1, native widths and both switches on takes the new op; every
    other configuration runs without one DenseReLUDropout call and still trains."""
    from xdfm_amd import layers, ops
    dev = _dev()
    calls = []
    real = ops.dense_relu_dropout

    def counted(*a, **k):
        calls.append(a[5] if len(a) > 5 else k.get("layer"))
        return real(*a, **k)

    monkeypatch.setattr(ops, "dense_relu_dropout", counted)
    kw = dict(hidden=(64, 32), activation="relu", use_bn=False, p=0.5)
    kw.update({"out40": dict(hidden=(40, 40)), "sigmoid": dict(activation="sigmoid"), "use_bn": dict(use_bn=True), "p1": dict(p=1.0),
               "p0": dict(p=0.0)}.get(what, {}))
    if what == "switch_off":
        monkeypatch.setattr(ops, "DNN_DROPOUT_NATIVE", False)
    if what == "dnn_native_off":
        monkeypatch.setattr(ops, "DNN_NATIVE", False)
    net = layers.DNN(40, kw["hidden"], activation=kw["activation"], dropout_rate=kw["p"], use_bn=kw["use_bn"], init_std=0.3, device=dev)
    net.train(what != "eval")
    x = torch.randn(70, 40, generator=torch.Generator().manual_seed(2)).to(dev).requires_grad_(True)
    out = net(x)
    out.sum().backward()
    assert calls == ([0, 1] if what == "native" else []), (what, calls)
    assert (net.last_drop_seed is not None) == (what == "native")
    assert bool(torch.isfinite(out).all()) and out.shape == (70, kw["hidden"][-1])
    for q in [x] + list(net.linears.parameters()):
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), what
    if what in ("out40", "sigmoid", "use_bn", "switch_off", "dnn_native_off"):       # nn.Dropout's own draw ran
        zeros = float((out == 0).double().mean())
        assert zeros > 0.3, (what, zeros)
    if what == "p1":
        assert float(out.detach().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ captured step
def _small_xdeepfm(dev, dnn_dropout):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    vocab, nd, Dm = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, Dm) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    torch.manual_seed(7)
    model = xDeepFM(cols, cols, dnn_hidden_units=(64, 32), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, dnn_dropout=dnn_dropout, device=dev)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    step = graphstep.GraphedStep(model)
    model.__dict__["_graphed_step"] = step
    return model, step, vocab, nd


def test_captured_step_draws_a_new_seed_at_every_replay(monkeypatch):
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import ops
    monkeypatch.setenv("XDFM_HIP_GRAPH", "1")
    dev = _dev()
    calls = []
    real = ops.dense_relu_dropout
    monkeypatch.setattr(ops, "dense_relu_dropout", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    nodes, runs = {}, {}
    for p in (0.5, 0.0):
        model, step, vocab, nd = _small_xdeepfm(dev, p)
        losses, seeds = [], []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for s in range(6):
                X, y = orc.synthetic_batch(128, vocab, nd, seed=500 + s)
                out = model.train_on_batch(T(X).to(dev), T(y).to(dev))
                losses.append(float(out[2].detach().reshape(-1)[0]))
                if p > 0:
                    seeds.append(int(model.dnn.last_drop_seed.item()))
        torch.cuda.synchronize()
        assert not [w for w in caught if "capture" in str(w.message)], [str(w.message) for w in caught]
        graphs = [e for e in step.entries.values() if e.graph is not None]
        assert step.replays > 0 and not step.disabled and len(graphs) == 1, (p, step.replays, step.disabled)
        nodes[p], runs[p] = graphs[0].nodes, (losses, seeds, step.replays)
        assert all(np.isfinite(losses)), (p, losses)
    print("captured nodes: dnn_dropout=0.5 %d, dnn_dropout=0 %d; replays %d" % (nodes[0.5], nodes[0.0], runs[0.5][2]))
    assert len(calls) == 2 * 3, "Python ran for two eager steps and the capture: two hidden layers each"
    assert nodes[0.5] <= nodes[0.0] + 2, nodes
    seeds, replays = runs[0.5][1], runs[0.5][2]
    assert replays >= 3
    assert len(set(seeds[-replays:])) == replays, "every replay reads a new seed: %r" % (seeds,)
    assert seeds[-1] != seeds[-2]


# ------------------------------------------------------------------------------------------ SFG decoder
def test_sfg_decoder_hidden_native_with_its_default_dropout(monkeypatch):
    from xdfm_amd import ops
    from xdfm_amd.pro import SFGDecoder
    dev = _dev()
    dims = {"C%d" % i: 20 + i for i in range(5)}
    dec = SFGDecoder(8, dims, ["I1", "I2", "I3"], hidden_units=(128, 64), use_label_aware_attention=False, device=dev)
    p = 0.1
    assert [m.p for m in dec.shared_layers if isinstance(m, torch.nn.Dropout)] == [p, p]
    keys_before = list(dec.state_dict().keys())
    linears = [m for m in dec.shared_layers if isinstance(m, torch.nn.Linear)]
    gen = torch.Generator().manual_seed(606)
    _randomise(linears, gen, dev)
    rows, k = 70, 5 * 8 + 3
    x0 = torch.randn(rows, k, generator=gen).to(dev)
    g0 = torch.randn(rows, 64, generator=gen).to(dev)
    calls = []
    real = ops.dense_relu_dropout
    monkeypatch.setattr(ops, "dense_relu_dropout", lambda *a, **kw: (calls.append(a[5]), real(*a, **kw))[1])
    dec.train()
    x = x0.clone().requires_grad_(True)
    out = dec.hidden_native(x, None)
    out.backward(g0)
    assert calls == [0, 1] and list(dec.state_dict().keys()) == keys_before
    grads = [x.grad] + [q.grad for lin in linears for q in (lin.weight, lin.bias)]
    monkeypatch.setattr(ops, "dense_relu_dropout", real)
    _tower_replay("sfg_r70_k43_128_64_p0.1", linears, p, dec.last_drop_seed, x0, g0, out.detach(), grads)
    # eval(): the dropout-free value, no new op
    dec.eval()
    with torch.no_grad():
        h = x0
        for lin in linears:
            h = ops.dense_relu(h, lin.weight, lin.bias)
        assert torch.equal(dec.hidden_native(x0, None), h)


def test_pro_model_with_default_sfg_dropout_trains_one_eager_step(monkeypatch):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.xdeepfm_pro import xDeepFMProLight
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import ops
    dev = _dev()
    monkeypatch.setenv("XDFM_PRO_GRAPH", "1")            # the static route: the one that runs SFGDecoder.hidden_native
    vocab, nd, Dm = [50, 300, 77, 120, 64, 211], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, Dm) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    model = xDeepFMProLight(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev,
                            sfg_hidden_units=(64, 32))
    assert [m.p for m in model.sfg_decoder.shared_layers if isinstance(m, torch.nn.Dropout)] == [0.1, 0.1]
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    calls = []
    real = ops.dense_relu_dropout
    monkeypatch.setattr(ops, "dense_relu_dropout", lambda *a, **kw: (calls.append(a[5]), real(*a, **kw))[1])
    X, _ = orc.synthetic_batch(64, vocab, nd, seed=300)
    y = (np.random.default_rng(900).random((64, 1)) < 0.3).astype(np.float32)
    y[0, 0] = 1.0
    out = model._train_step_eager(T(X.astype(np.float32)).to(dev), T(y).to(dev))
    torch.cuda.synchronize()
    assert calls == [0, 1], calls
    assert all(bool(torch.isfinite(t.detach()).all()) for t in out[1:])
    assert bool(torch.isfinite(model._step_log[1]).all())
