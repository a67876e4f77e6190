"""GPU tests (-m gpu) of the native dense layer (csrc/dnn.hip; ops.Dense / ops.DenseReLU) against a float64 reference
computed on the CPU from the same fp32 inputs.

Bar.  No fixed number: for each output (y, dx, dW, db) the native result's largest error against float64 may exceed the
largest error of the LIBRARY path (hipBLASLt GEMMs + xdfm_relu_bwd_colsum / xdfm_colsum, i.e. the code that runs with
XDFM_DNN_NATIVE=0) on the same inputs by at most a factor 2 -- both sum the same fp32 products, in different orders --
with an absolute floor of one fp32 ulp of the output's largest magnitude.  DESIGN.md (the DNN tower subsection) lists the
measured pairs.

Inputs are O(1): standard normal x and g, W ~ N(0, 1 / in), b ~ N(0, 1).  A ReLU layer's y holds exact zeros in about
half of its cells, each facing a non-zero g, so the mask's `> 0` edge decides real values.  Both backward paths and the
reference take the SAME y (the native forward's), so that a pre-activation within rounding of zero cannot flip a mask
between them.  The strided cases pass x, g and y as column windows of wider matrices (ld > columns).

Also here: the needs_input_grad combinations of both autograd functions (returned tensors against the full call's bits, the
launches that ran) and a chained layers.DNN tower with the native switch on and off against a float64 replay.  The entry
points called directly -- exact integer cases, pitches, guards -- are in tests/test_gpu_dnn_abi.py."""
import faulthandler

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
FACTOR = 2.0

#  name: (rows, in, out, relu, bias, strided)
CASES = {
    "r1_k13_o32_relu": (1, 13, 32, True, True, False),
    "r33_k429_o256_relu": (33, 429, 256, True, True, False),
    "r33_k429_o256_relu_strided": (33, 429, 256, True, True, True),
    "r257_k256_o256_none": (257, 256, 256, False, True, False),
    "r520_k40_o64_relu": (520, 40, 64, True, True, False),
    "r520_k40_o64_none_nobias": (520, 40, 64, False, False, False),
    # out a multiple of 32 but not of 64 (a half-empty last tile), one past / one short of the 64-tile, 5 / 9 / 29 splits of
    # the weight gradient (9: the last split holds one row; 29: rows beyond DN_MAX_SPLIT * 256), exactly 256 rows: one split
    "r65_k65_o96_relu": (65, 65, 96, True, True, False),
    "r63_k31_o160_none": (63, 31, 160, False, True, False),
    "r1100_k13_o32_relu": (1100, 13, 32, True, True, False),
    "r2049_k40_o64_relu_strided": (2049, 40, 64, True, True, True),
    "r8225_k65_o96_relu": (8225, 65, 96, True, True, False),
    "r256_k33_o32_relu": (256, 33, 32, True, True, False),
}
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
    """What the two autograd functions use of their ctx: lets a test call forward / backward with a y of its choice."""

    def __init__(self, needs=(True, True, True)):
        self.needs_input_grad = needs
        self.saved_tensors = ()
        self.has_bias = True

    def save_for_backward(self, *t):
        self.saved_tensors = t


def _window(t, pad_l, pad_r, fill):
    """t as a column window of a wider matrix filled with `fill` (a value that would show up in any result it leaked into)."""
    wide = torch.full((t.shape[0], pad_l + t.shape[1] + pad_r), fill, dtype=t.dtype, device=t.device)
    wide[:, pad_l:pad_l + t.shape[1]] = t
    w = wide[:, pad_l:pad_l + t.shape[1]]
    assert not w.is_contiguous() or t.shape[0] == 1
    return w


def _forward(ops, native, relu, x, W, b):
    """native: xdfm_dense_fwd itself (ops routes the forward to it only with DNN_NATIVE_FWD); otherwise the library path."""
    if native:
        return ops._dense_fwd_native(x, W, b, ops.ACT_CODES["relu" if relu else "linear"])
    ops.DNN_NATIVE = False
    return (ops.DenseReLU if relu else ops.Dense).forward(_Ctx(), x, W, b)


def _backward(ops, native, relu, x, W, b, y, g):
    ops.DNN_NATIVE = native
    ctx = _Ctx((True, True, b is not None))
    ctx.has_bias = b is not None
    ctx.saved_tensors = (x, W, y) if relu else (x, W)
    return (ops.DenseReLU if relu else ops.Dense).backward(ctx, g)


def _case(name):
    """Inputs, both paths' results and the float64 reference of one case, computed once."""
    if name in _CACHE:
        return _CACHE[name]
    from xdfm_amd import ops
    dev = _dev()
    rows, k, out, relu, bias, strided = CASES[name]
    gen = torch.Generator().manual_seed(1000 + len(name) + rows + k)
    x = torch.randn(rows, k, generator=gen)
    W = torch.randn(out, k, generator=gen) / float(np.sqrt(k))
    b = torch.randn(out, generator=gen) if bias else None
    g = torch.randn(rows, out, generator=gen)
    xd, Wd, gd = x.to(dev), W.to(dev), g.to(dev)
    bd = b.to(dev) if bias else None
    xn = _window(xd, 3, 2, 1e6) if strided else xd
    gn = _window(gd, 1, 4, 1e6) if strided else gd
    saved = ops.DNN_NATIVE
    try:
        assert ops.dense_native(xn, Wd, bd), "the case must be inside the native envelope"
        res = {"native": {}, "library": {}}
        y_nat = _forward(ops, True, relu, xn, Wd, bd)
        res["native"]["y"] = y_nat
        res["library"]["y"] = _forward(ops, False, relu, xd, Wd, bd)
        y_mask = y_nat.clone() if relu else None
        yn = _window(y_mask, 2, 5, 1e6) if (strided and relu) else y_mask
        for path, native, (xa, ga, ya) in (("native", True, (xn, gn, yn)), ("library", False, (xd, gd, y_mask))):
            dx, dW, db = _backward(ops, native, relu, xa, Wd, bd, ya, ga)
            res[path].update(dx=dx, dW=dW)
            if bias:
                res[path]["db"] = db
            else:
                assert db is None
        again = dict(zip(("dx", "dW", "db"), _backward(ops, True, relu, xn, Wd, bd, yn, gn)))
        again["y"] = _forward(ops, True, relu, xn, Wd, bd)
        torch.cuda.synchronize()
    finally:
        ops.DNN_NATIVE = saved
    # float64 on the CPU from the same fp32 inputs
    x6, W6, g6 = x.double(), W.double(), g.double()
    z6 = x6 @ W6.t() + (b.double() if bias else 0.0)
    ref = {"y": torch.relu(z6) if relu else z6}
    gz6 = torch.where(y_mask.cpu() > 0, g6, torch.zeros_like(g6)) if relu else g6
    ref.update(dx=gz6 @ W6, dW=gz6.t() @ x6)
    if bias:
        ref["db"] = gz6.sum(0)
    out_ = dict(res=res, again=again, ref=ref, zeros_in_y=int((y_mask == 0).sum()) if relu else 0, y_cells=rows * out)
    _CACHE[name] = out_
    return out_


@pytest.mark.parametrize("name", list(CASES))
def test_native_error_against_float64_within_twice_the_library_paths(name):
    c = _case(name)
    if CASES[name][3] and c["y_cells"] >= 32:
        assert 0 < c["zeros_in_y"] < c["y_cells"], "the ReLU case must hold exact zeros and live cells"
    bad = []
    for key, want in c["ref"].items():
        e_nat = float((c["res"]["native"][key].detach().cpu().double() - want).abs().max())
        e_lib = float((c["res"]["library"][key].detach().cpu().double() - want).abs().max())
        floor = float(np.spacing(np.float32(want.abs().max())))
        print("%-28s %-3s native %.3e  library %.3e  floor (1 ulp) %.3e" % (name, key, e_nat, e_lib, floor))
        assert c["res"]["native"][key].shape == want.shape
        if not e_nat <= max(FACTOR * e_lib, floor):
            bad.append((key, e_nat, e_lib, floor))
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_two_calls_give_the_same_bits(name):
    c = _case(name)
    for key, second in c["again"].items():
        if second is None:
            continue
        assert torch.equal(c["res"]["native"][key], second), key


def _train_like(ops, x, W, b):
    a = [t.clone().requires_grad_(True) for t in (x, W, b)]
    y = ops.dense_relu(*a)
    gen = torch.Generator().manual_seed(5)
    y.backward(torch.randn(y.shape, generator=gen).to(y.device))
    return [y.detach()] + [t.grad for t in a]


def _inputs(dev, rows, k, out):
    gen = torch.Generator().manual_seed(77)
    return (torch.randn(rows, k, generator=gen).to(dev), (torch.randn(out, k, generator=gen) / float(np.sqrt(k))).to(dev),
            torch.randn(out, generator=gen).to(dev))


def _stock(x, W, b):
    """The library path of ops.dense_relu spelled out in torch calls: [y, dx, dW, db] for _train_like's gradient."""
    y = torch._addmm_activation(b, x, W.t(), use_gelu=False)
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(y.shape, generator=gen).to(y.device)
    gz = torch.where(y > 0, g, torch.zeros_like(g))
    return [y, gz.mm(W), gz.t().mm(x), gz.sum(0)]


def _same_as_stock(got, x, W, b):
    want = _stock(x, W, b)
    for a_, b_, name in zip(got[:3], want[:3], ("y", "dx", "dW")):
        assert torch.equal(a_, b_), name
    # the bias gradient is xdfm_relu_bwd_colsum's fixed-order sum, ATen's is another order of the same fp32 values
    np.testing.assert_allclose(got[3].cpu().numpy(), want[3].cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_ops_dense_relu_runs_the_native_kernels_when_supported_and_the_library_otherwise():
    from xdfm_amd import ops
    dev = _dev()
    saved_native, saved_profile = ops.DNN_NATIVE, ops.PROFILE
    try:
        # supported shape, switch on: the brackets of the native operations appear (the forward's only with
        # DNN_NATIVE_FWD), the gradients are the native kernels' bits
        x, W, b = _inputs(dev, 33, 429, 256)
        ops.DNN_NATIVE, ops.PROFILE = True, []
        got = _train_like(ops, x, W, b)
        names = [p[0] for p in ops.PROFILE]
        assert names == (["dense_fwd"] if ops.DNN_NATIVE_FWD else []) + ["dense_bwd_x", "dense_bwd_w"], names
        assert all(p[1] == 0.0 for p in ops.PROFILE), "work 0: listed, never a roofline candidate"
        ops.PROFILE = None
        gen = torch.Generator().manual_seed(5)
        g = torch.randn(got[0].shape, generator=gen).to(dev)
        for a_, b_ in zip(got[1:], ops._dense_bwd_native(g, got[0], x, W, True, True, True)):
            assert torch.equal(a_, b_)
        # switch off (what XDFM_DNN_NATIVE=0 sets at import): no bracket, the library path's bits
        ops.DNN_NATIVE, ops.PROFILE = False, []
        off = _train_like(ops, x, W, b)
        assert [p[0] for p in ops.PROFILE] == []
        ops.PROFILE = None
        _same_as_stock(off, x, W, b)
        # unsupported out = 48 with the switch on: the library path's bits, no bracket
        x, W, b = _inputs(dev, 33, 429, 48)
        ops.DNN_NATIVE, ops.PROFILE = True, []
        assert not ops.dense_native(x, W, b)
        un = _train_like(ops, x, W, b)
        assert [p[0] for p in ops.PROFILE] == []
        ops.PROFILE = None
        _same_as_stock(un, x, W, b)
    finally:
        ops.DNN_NATIVE, ops.PROFILE = saved_native, saved_profile


@pytest.mark.parametrize("relu", [True, False], ids=["DenseReLU", "Dense"])
def test_needs_input_grad_combinations_return_the_full_calls_bits_and_launch_only_what_is_needed(relu):
    """(65, 65, 96): no dx, no dW but db, no db and -- Dense -- a layer without bias.  What is returned equals the full
    call's bits, the rest is None, and the ops.PROFILE brackets list the launches that ran, nothing else."""
    from xdfm_amd import ops
    dev = _dev()
    rows, k, out = 65, 65, 96
    gen = torch.Generator().manual_seed(4242)
    x = torch.randn(rows, k, generator=gen).to(dev)
    W = (torch.randn(out, k, generator=gen) / float(np.sqrt(k))).to(dev)
    b = torch.randn(out, generator=gen).to(dev)
    g = torch.randn(rows, out, generator=gen).to(dev)
    fn = ops.DenseReLU if relu else ops.Dense
    saved_native, saved_profile = ops.DNN_NATIVE, ops.PROFILE
    try:
        ops.DNN_NATIVE = True
        assert ops.dense_native(x, W, b)
        y = torch.relu(torch.addmm(b, x, W.t())) if relu else None
        if relu:
            assert 0 < int((y == 0).sum()) < y.numel()

        def run(needs, has_bias=True):
            ctx = _Ctx(needs)
            ctx.has_bias = has_bias
            ctx.saved_tensors = (x, W, y) if relu else (x, W)
            ops.PROFILE = []
            got = fn.backward(ctx, g)
            names = [p[0] for p in ops.PROFILE]
            ops.PROFILE = None
            return got, names

        full, names = run((True, True, True))
        assert names == ["dense_bwd_x", "dense_bwd_w"] and all(t is not None for t in full)
        combos = [((False, True, True), True, ["dense_bwd_w"]), ((True, False, True), True, ["dense_bwd_x", "dense_bwd_w"]),
                  ((True, True, False), True, ["dense_bwd_x", "dense_bwd_w"])]
        if not relu:
            combos.append(((True, True, True), False, ["dense_bwd_x", "dense_bwd_w"]))
        for needs, has_bias, launches in combos:
            got, names = run(needs, has_bias)
            assert names == launches, (needs, has_bias, names)
            wanted = (needs[0], needs[1], needs[2] and has_bias)
            for key, t, ref, w in zip(("dx", "dW", "db"), got, full, wanted):
                if w:
                    assert t is not None and torch.equal(t, ref), (needs, has_bias, key)
                else:
                    assert t is None, (needs, has_bias, key)
    finally:
        ops.DNN_NATIVE, ops.PROFILE = saved_native, saved_profile


def test_chained_tower_native_against_library_and_a_float64_replay():
    """layers.DNN (32, 96, 32), relu, rows 65, input width 13, with ops.DNN_NATIVE on and off.  Both runs use the library
    forward, so their outputs -- and hence their masks -- are the same bits.  Every gradient of the native run is within
    max(2 x the library run's error, 1 ulp) of a float64 replay, layer by layer, of the backward.

    The replay takes its masks (and each layer's input) from the fp32 activations of the run, not from a float64 forward:
    a pre-activation within rounding of zero would open a cell in one precision and close it in the other, and the two
    backward passes would then differentiate different functions -- a difference of the whole g in that cell, not a
    rounding error.  The kernels under test see the fp32 activations; so does the reference."""
    from xdfm_amd import layers, ops
    dev = _dev()
    rows, k, hidden = 65, 13, (32, 96, 32)
    gen = torch.Generator().manual_seed(31337)
    net = layers.DNN(k, hidden, activation="relu", dropout_rate=0, use_bn=False, device=dev)
    with torch.no_grad():
        for lin in net.linears:
            lin.weight.copy_((torch.randn(lin.weight.shape, generator=gen) / float(np.sqrt(lin.weight.shape[1]))).to(dev))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen).to(dev))
    x0 = torch.randn(rows, k, generator=gen)
    g0 = torch.randn(rows, hidden[-1], generator=gen)
    params = [p for lin in net.linears for p in (lin.weight, lin.bias)]
    saved_native, saved_profile = ops.DNN_NATIVE, ops.PROFILE
    runs = {}
    try:
        for native in (True, False):
            ops.DNN_NATIVE, ops.PROFILE = native, []
            x = x0.to(dev).requires_grad_(True)
            for p in params:
                p.grad = None
            y = net(x)
            y.backward(g0.to(dev))
            names = [p[0] for p in ops.PROFILE if p[0] != "dense_fwd"]          # the forward's only with DNN_NATIVE_FWD
            ops.PROFILE = None
            assert names == (["dense_bwd_x", "dense_bwd_w"] * 3 if native else []), names
            runs[native] = dict(y=y.detach().clone(), grads=[x.grad.clone()] + [p.grad.clone() for p in params])
        # the fp32 activations of the run: ops.dense_relu per layer, the library forward both runs used
        ops.DNN_NATIVE = False
        acts = [x0.to(dev)]
        with torch.no_grad():
            for lin in net.linears:
                acts.append(ops.dense_relu(acts[-1], lin.weight, lin.bias))
    finally:
        ops.DNN_NATIVE, ops.PROFILE = saved_native, saved_profile
    assert torch.equal(runs[True]["y"], runs[False]["y"]) and torch.equal(acts[-1], runs[True]["y"])
    acts = [a.cpu() for a in acts]
    for a in acts[1:]:
        assert 0 < int((a == 0).sum()) < a.numel()
    # float64 replay of the backward, last layer first
    g6 = g0.double()
    ref = {}
    for i in reversed(range(3)):
        W6 = net.linears[i].weight.detach().cpu().double()
        gz = torch.where(acts[i + 1] > 0, g6, torch.zeros_like(g6))
        ref[1 + 2 * i], ref[2 + 2 * i] = gz.t() @ acts[i].double(), gz.sum(0)
        g6 = gz @ W6
    ref[0] = g6
    labels = ["dx"] + ["%s%d" % (n, i) for i in range(3) for n in ("dW", "db")]
    bad = []
    for j, label in enumerate(labels):
        want = ref[j]
        e_nat = float((runs[True]["grads"][j].cpu().double() - want).abs().max())
        e_lib = float((runs[False]["grads"][j].cpu().double() - want).abs().max())
        floor = float(np.spacing(np.float32(want.abs().max())))
        print("%-28s %-3s native %.3e  library %.3e  floor (1 ulp) %.3e" % ("tower_r65_k13_32_96_32", label, e_nat, e_lib, floor))
        assert runs[True]["grads"][j].shape == want.shape
        if not e_nat <= max(FACTOR * e_lib, floor):
            bad.append((label, e_nat, e_lib, floor))
    assert not bad, bad
