"""GPU tests (-m gpu) of the native AutoDis op (csrc/autodis.hip, ops.AutoDis) against a float64 composition of
deepctr/xdeepfm_pro/autodis.py:99-125 written here, and of xDeepFMPro(use_autodis=True) native against the stock loop.

Bars.  Outer: those of test_pro_model_vs_reference_golden -- output rtol 2e-5 / atol 2e-6, gradients rtol 3e-4 / atol
3e-5 * max|want| (+ 1e-9).  Relative: with every error written as a fraction of its outer bar (the worst element), the
native fraction must not exceed max(MARGIN * the stock fp32 loop's fraction on the same inputs on the same GPU, FLOOR).
Both paths are fp32 with different summation orders and the statistic is a maximum that a single near-tie of two
scores can set, so the two scatter around each other: MARGIN = 4 allows for that case by case, and FLOOR = 0.27 is the
stock composition's own worst fraction over this sweep (float32 against float64 on the CPU, fixed before the native
kernels ran) -- below it a ratio of the two says nothing.  DESIGN.md (xDeepFMPro, AutoDis) has the figures measured on
the MI355X for both paths.

Input values.  The parameters are drawn as AutoDisLayer draws them (nn.Linear's uniform ranges, 0.01 * randn
meta-embeddings).  "unit": standard normal inputs with exact zeros mixed in (both LeakyReLU branches and the kink) and
temperatures log-spaced over [0.05, 5], both ends present.  "large": the same with 2 % of the entries scaled to a magnitude
of ~1e3 and temperatures over [1, 5].  The one combination left out is inputs of ~1e3 with temperatures down to 0.05:
the scores are then ~1e3 wide and divided by 0.05, the fp32 rounding of the scores alone moves the softmax exponent by
~1e-3, and the stock fp32 composition misses the outer bars as well (float32 against float64 on the CPU, worst fraction
of the bar over SHAPES: out 1.1 and dW2 1.0 with 2 % large entries, out 5.6 and dT 6.2 with all entries large; the two
sets kept here: 0.10 and 0.27).
"""
import faulthandler

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 240          # every test here is one GPU step; a hang ends the process instead of blocking the run
MARGIN, FLOOR = 4.0, 0.27   # native fraction <= max(MARGIN * stock fraction, FLOOR), see the module docstring

#        B     F   K   D      every B, F, K, D of the sweep appears; K covers the three instances (8 / 16 / 32) and their tails
SHAPES = [(1, 1, 1, 1),
          (63, 3, 2, 4),
          (256, 13, 6, 4),
          (257, 3, 8, 10),
          (4096, 13, 16, 16),
          (4099, 1, 9, 32),
          (257, 40, 17, 64),
          (63, 13, 32, 64),
          (4099, 3, 32, 10),
          (256, 40, 16, 1),
          (4096, 1, 8, 16)]
VALUES = ["unit", "large"]
META_SCALE = 0.01           # AutoDisLayer's own initial scale of the meta-embeddings
LARGE_SHARE, LARGE_T_LO = 0.02, 1.0


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def make_case(B, F, K, D, values, seed=0, meta_scale=META_SCALE):
    """float64 CPU tensors: x [B, F], the six parameter groups, the upstream gradient gout [B, F * D].  The projectors
    are drawn as nn.Linear draws them (uniform in +-1/sqrt(fan_in)), the meta-embeddings as meta_scale * randn."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 131 * F + 17 * K + D)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = lambda bound, *s: (2.0 * torch.rand(*s, generator=g, dtype=torch.float64) - 1.0) * bound
    x = r(B, F)
    x[torch.rand(B, F, generator=g) < 0.15] = 0.0
    lo = 0.05
    if values == "large":
        x = torch.where(torch.rand(B, F, generator=g) < LARGE_SHARE, x * 1e3, x)
        lo = LARGE_T_LO
    e = torch.linspace(0.0, 1.0, F, dtype=torch.float64) if F > 1 else torch.zeros(1, dtype=torch.float64)
    T = lo * (5.0 / lo) ** e[torch.randperm(F, generator=g)]                  # log-spaced over [lo, 5], both ends present
    p = dict(meta=meta_scale * r(F, K, D), W1=u(1.0, F, K, 1), b1=u(1.0, F, K), W2=u(K ** -0.5, F, K, K), b2=u(K ** -0.5, F, K), T=T)
    # fp32-representable values, so that every path starts from the same numbers
    x = x.float().double()
    p = {k: v.float().double() for k, v in p.items()}
    gout = r(B, F * D).float().double()
    return x, p, gout


def oracle(x, p, gout, dtype=torch.float64):
    """autodis.py:99-125 on the CPU in `dtype`, with autograd: out and the gradients of sum(out * gout)."""
    x = x.to(dtype).clone().requires_grad_(True)
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    F = x.shape[1]
    embs = []
    for i in range(F):
        v = x[:, i:i + 1]
        h = torch.nn.functional.linear(v, q["W1"][i], q["b1"][i])
        a = torch.nn.functional.leaky_relu(h, 0.2)
        s = torch.nn.functional.linear(a, q["W2"][i], q["b2"][i])
        w = torch.softmax(s / q["T"][i], dim=-1)
        embs.append(torch.matmul(w, q["meta"][i]).unsqueeze(1))
    out = torch.cat(embs, dim=1).view(x.shape[0], -1)
    (out * gout.to(dtype)).sum().backward()
    res = {"out": out.detach(), "dx": x.grad}
    res.update({"d" + k: v.grad for k, v in q.items()})
    return res


def make_layer(p, dev):
    from deepctr.xdeepfm_pro.autodis import AutoDisLayer
    F, K, D = p["meta"].shape
    layer = AutoDisLayer(F, K, D, device=dev)
    with torch.no_grad():
        layer.meta_embeddings.copy_(p["meta"].float())
        layer.feature_temperatures.copy_(p["T"].float())
        for i, seq in enumerate(layer.bucket_projectors):
            seq[0].weight.copy_(p["W1"][i].float())
            seq[0].bias.copy_(p["b1"][i].float())
            seq[2].weight.copy_(p["W2"][i].float())
            seq[2].bias.copy_(p["b2"][i].float())
    return layer


def run_layer(layer, x, gout, dev, want_dx=True):
    """out and gradients of the product layer on the GPU, in the oracle's naming; the layer's .grad fields are reset."""
    xs = x.float().to(dev).requires_grad_(want_dx)
    layer.zero_grad(set_to_none=True)
    flat, lst = layer([xs[:, i:i + 1] for i in range(xs.shape[1])])
    (flat * gout.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    F = xs.shape[1]
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = {"out": flat.detach(), "dx": xs.grad,
           "dmeta": layer.meta_embeddings.grad, "dT": layer.feature_temperatures.grad,
           "dW1": torch.stack([zero(layer.bucket_projectors[i][0].weight) for i in range(F)]),
           "db1": torch.stack([zero(layer.bucket_projectors[i][0].bias) for i in range(F)]),
           "dW2": torch.stack([zero(layer.bucket_projectors[i][2].weight) for i in range(F)]),
           "db2": torch.stack([zero(layer.bucket_projectors[i][2].bias) for i in range(F)])}
    return {k: (None if v is None else v.detach().cpu()) for k, v in res.items()}, lst


def bar_fraction(name, got, want):
    """max over the elements of |got - want| / (atol + rtol * |want|) with the outer bars: <= 1 passes them."""
    want = want.double().numpy()
    got = got.double().numpy()
    if name == "out":
        tol = 2e-6 + 2e-5 * np.abs(want)
    else:
        tol = 3e-5 * float(np.abs(want).max()) + 1e-9 + 3e-4 * np.abs(want)
    return float((np.abs(got - want) / tol).max())


NAMES = ["out", "dmeta", "dW1", "db1", "dW2", "db2", "dT", "dx"]


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_F%d_K%d_D%d" % s)
def test_autodis_vs_float64(shape, values, monkeypatch):
    """Output, the six parameter gradients and dx against float64; the stock fp32 loop on the same GPU as the yardstick
    of what fp32 can do on these inputs."""
    from xdfm_amd import ops
    dev = _dev()
    B, F, K, D = shape
    x, p, gout = make_case(B, F, K, D, values)
    want = oracle(x, p, gout)
    layer = make_layer(p, dev)
    before = ops.AutoDis.calls
    monkeypatch.setenv("XDFM_AUTODIS_NATIVE", "1")
    got, lst = run_layer(layer, x, gout, dev)
    assert ops.AutoDis.calls == before + 1, "the native op did not run"
    assert len(lst) == F and all(t.shape == (B, 1, D) for t in lst)
    assert all(t.untyped_storage().data_ptr() == lst[0].untyped_storage().data_ptr() for t in lst), "list entries are views"
    monkeypatch.setenv("XDFM_AUTODIS_NATIVE", "0")
    stock, _ = run_layer(layer, x, gout, dev)
    assert ops.AutoDis.calls == before + 1
    report, bad = [], []
    for n in NAMES:
        assert got[n].shape == want[n].shape, n
        fn, fs = bar_fraction(n, got[n], want[n]), bar_fraction(n, stock[n], want[n])
        report.append("%s native %.3g stock %.3g" % (n, fn, fs))
        if not (fn <= 1.0 and fn <= max(MARGIN * fs, FLOOR)):
            bad.append(n)
    print("autodis %s %s (fractions of the outer bar): %s" % (shape, values, "; ".join(report)))
    assert not bad, "%s: %s" % (bad, "; ".join(report))


def test_autodis_deterministic():
    """Forward and backward twice on the same inputs: identical bits (no float atomics, fixed summation order)."""
    dev = _dev()
    x, p, gout = make_case(4099, 13, 16, 16, "unit", seed=3)
    layer = make_layer(p, dev)
    a, _ = run_layer(layer, x, gout, dev)
    b, _ = run_layer(layer, x, gout, dev)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n


def test_autodis_frozen_parameters():
    """requires_grad_(False) on one projector and on the temperatures: nothing raises, the frozen ones get no gradient,
    the remaining gradients still match float64."""
    dev = _dev()
    x, p, gout = make_case(257, 3, 6, 10, "unit", seed=5)
    want = oracle(x, p, gout)
    layer = make_layer(p, dev)
    layer.bucket_projectors[1].requires_grad_(False)
    layer.feature_temperatures.requires_grad_(False)
    got, _ = run_layer(layer, x, gout, dev)
    assert got["dT"] is None
    assert all(q.grad is None for q in layer.bucket_projectors[1].parameters())
    for n in ("dW1", "db1", "dW2", "db2"):
        assert float(got[n][1].abs().max()) == 0.0           # run_layer's placeholder for "no gradient"
        want[n] = want[n].clone()
        want[n][1] = 0.0
    for n in NAMES:
        if n != "dT":
            assert bar_fraction(n, got[n], want[n]) <= 1.0, n
    # every parameter frozen, input too: the forward still runs and autograd has nothing to do
    layer.requires_grad_(False)
    flat, _ = layer([x[:, i:i + 1].float().to(dev) for i in range(3)])
    assert not flat.requires_grad and bar_fraction("out", flat.cpu(), want["out"]) <= 1.0
    # only the input asks for a gradient
    xs = x.float().to(dev).requires_grad_(True)
    flat, _ = layer([xs[:, i:i + 1] for i in range(3)])
    (flat * gout.float().to(dev)).sum().backward()
    assert bar_fraction("dx", xs.grad.cpu(), want["dx"]) <= 1.0


@pytest.mark.parametrize("K,D", [(48, 8), (8, 65)])
def test_autodis_fallback_outside_envelope(K, D):
    """K > 32 or D > 64: the stock loop runs (ops.AutoDis.calls does not move) and gives the stock result."""
    from xdfm_amd import ops
    dev = _dev()
    assert not ops.autodis_supported(K, D)
    x, p, gout = make_case(63, 3, K, D, "unit", seed=7)
    want = oracle(x, p, gout)
    layer = make_layer(p, dev)
    before = ops.AutoDis.calls
    got, lst = run_layer(layer, x, gout, dev)
    assert ops.AutoDis.calls == before
    assert len(lst) == 3 and lst[0].shape == (63, 1, D)
    for n in NAMES:
        assert bar_fraction(n, got[n], want[n]) <= 1.0, n


def test_autodis_switch_off(monkeypatch):
    """XDFM_AUTODIS_NATIVE=0 keeps the stock loop inside the envelope too."""
    from xdfm_amd import ops
    dev = _dev()
    x, p, gout = make_case(63, 3, 6, 4, "unit", seed=9)
    layer = make_layer(p, dev)
    monkeypatch.setenv("XDFM_AUTODIS_NATIVE", "0")
    before = ops.AutoDis.calls
    run_layer(layer, x, gout, dev)
    assert ops.AutoDis.calls == before
    monkeypatch.setenv("XDFM_AUTODIS_NATIVE", "1")
    run_layer(layer, x, gout, dev)
    assert ops.AutoDis.calls == before + 1


def test_autodis_strided_input_in_place():
    """The dense columns of a wider matrix are read in place: same bits as from a contiguous copy."""
    dev = _dev()
    x, p, gout = make_case(257, 13, 16, 16, "unit", seed=11)
    layer = make_layer(p, dev)
    wide = torch.randn(257, 40, device=dev)
    wide[:, 27:] = x.float().to(dev)
    with torch.no_grad():
        a, _ = layer.forward_native(wide[:, 27:])
        b, _ = layer.forward_native(x.float().to(dev))
    assert torch.equal(a, b)


def test_autodis_graph_capture():
    """Forward + backward captured in a HIP graph: the replay on new input values equals the eager result bit for bit."""
    dev = _dev()
    x, p, gout = make_case(4096, 13, 16, 16, "unit", seed=13)
    x2, _, gout2 = make_case(4096, 13, 16, 16, "unit", seed=14)
    layer = make_layer(p, dev)
    params = list(layer.parameters())
    xs = x.float().to(dev)
    gs = gout.float().to(dev)

    def step():
        flat, _ = layer.forward_native(xs)
        grads = torch.autograd.grad((flat * gs).sum(), params)
        return flat, grads

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                    # warm-up off the capture: builds the pointer table, fills the allocator
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        flat_g, grads_g = step()
    xs.copy_(x2.float().to(dev))
    gs.copy_(gout2.float().to(dev))
    graph.replay()
    torch.cuda.synchronize()
    flat_r, grads_r = flat_g.clone(), [t.clone() for t in grads_g]
    flat_e, grads_e = step()
    torch.cuda.synchronize()
    assert torch.equal(flat_r, flat_e)
    for a, b in zip(grads_r, grads_e):
        assert torch.equal(a, b)
    want = oracle(x2, p, gout2)
    assert bar_fraction("out", flat_r.detach().cpu(), want["out"]) <= 1.0


def _pro_model(dev, seed):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.xdeepfm_pro import xDeepFMPro
    vocab = [30, 50, 17, 64, 40, 25]
    cols = [SparseFeat("C%d" % (i + 1), v, 16) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(13)]
    model = xDeepFMPro(cols, cols, dnn_hidden_units=(64, 32), cin_layer_size=(32, 16), l2_reg_dnn=1e-5, device=dev,
                       sfg_hidden_units=(64, 32), sfg_dropout=0.0, use_autodis=True, autodis_buckets=16, seed=seed)
    return model, vocab


def test_pro_model_native_vs_stock(monkeypatch):
    """Two xDeepFMPro(use_autodis=True) models from one state, 6 sparse + 13 dense fields, D = 16, B = 512: five train steps
    with the native op against five with the stock loop -- losses, every parameter and predict within the bars the pro_*
    golden test applies after three steps; the native model went through ops.AutoDis once per step."""
    from xdfm_amd import ops
    dev = _dev()
    B, steps = 512, 5
    native, vocab = _pro_model(dev, 1024)
    stock, _ = _pro_model(dev, 1024)
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():                       # weights large enough that AutoDis matters to the loss
        for k, q in native.named_parameters():
            if "autodis" in k and "temperatures" not in k:
                q.copy_((0.3 * torch.randn(q.shape, generator=g)).to(dev))
            elif "embedding_dict" in k or k.startswith("dnn") or k in ("linear_model.weight", "cin_linear.weight"):
                q.copy_((0.1 * torch.randn(q.shape, generator=g)).to(dev))
    stock.load_state_dict({k: v.clone() for k, v in native.state_dict().items()})
    rng = np.random.RandomState(5)
    X = np.concatenate([np.stack([rng.randint(0, v, size=B * steps) for v in vocab], axis=1).astype(np.float32),
                        rng.rand(B * steps, 13).astype(np.float32)], axis=1)
    y = (rng.rand(B * steps, 1) < 0.3).astype(np.float32)
    out = {}
    for name, model, env in (("stock", stock, "0"), ("native", native, "1")):
        monkeypatch.setenv("XDFM_AUTODIS_NATIVE", env)
        model.compile("adam", "binary_crossentropy", metrics=[])
        model.train()
        before = ops.AutoDis.calls
        losses = []
        for s in range(steps):
            xs = torch.from_numpy(X[s * B:(s + 1) * B]).to(dev)
            ys = torch.from_numpy(y[s * B:(s + 1) * B]).to(dev)
            _, l, tot = model.train_on_batch(xs, ys)
            losses.append([l.item(), tot.item()])
        calls = ops.AutoDis.calls - before
        model.eval()
        pred = model.predict([X[:, i] for i in range(X.shape[1])], batch_size=B)
        out[name] = (losses, {k: v.cpu().numpy() for k, v in model.state_dict().items()}, pred, calls)
    assert out["stock"][3] == 0
    assert out["native"][3] == steps, "one ops.AutoDis forward per train step"
    np.testing.assert_allclose(out["native"][0], out["stock"][0], rtol=2e-4)
    for k, want in out["stock"][1].items():
        np.testing.assert_allclose(out["native"][1][k], want, rtol=2e-3, atol=3e-6 + 2e-4 * float(np.abs(want).max()) * 1e-2,
                                   err_msg="after %d steps %s" % (steps, k))
    np.testing.assert_allclose(out["native"][2], out["stock"][2], rtol=2e-4, atol=2e-6)
