"""GPU tests (-m gpu) of SGD with momentum through the model (K7m / K7md behind xdfm_amd.optim.TableSGD): the native route and
its switch, whole models against goldens produced by the reference with a torch.optim.SGD(momentum=0.9[, nesterov=True]) object,
the native step against the stock fallback, graph replay against eager launches bit for bit, the deferred update against the
sweep bit for bit, checkpoints in both directions and the fallback that remains.  Shapes are `sum_small`-sized: six fields,
vocabularies of tens of rows, B <= 64.

Tolerances: goldens as tests/test_gpu_rmsprop.py (losses rtol 2e-5, state after three steps rtol 1e-3 / atol 2e-5); native
against stock opt_ref.TOL (p 2e-6 / 1e-8, momentum buffer 2e-6 / 1e-10).

The comparisons with the stock step run every step on ONE batch: the stock step rounds mu * buf before it adds g', the kernel
does not (csrc/opt_math.h), both correct fp32 steps half an ulp of mu * buf apart -- which only stays inside the buffer's bar,
a bar relative to the result, while buf does not cancel (tests/sgdm_ref.py, "THE SIGNS").  On one batch the gradient of a step
has the sign of the step before it in all but the elements that sit at a zero of the gradient."""
import copy
import os

import numpy as np
import pytest
import torch

import opt_ref as R
from conftest import load_golden
from test_gpu_optim import _build_model, _dev, _three_steps_by_hand, cin_math, close  # noqa: F401

pytestmark = pytest.mark.gpu
T = torch.from_numpy
VOCAB, ND, D, B = [31, 17, 23, 12, 9, 40], 3, 8, 64
LR = 1e-3
NES = pytest.mark.parametrize("nesterov", [False, True], ids=["momentum", "nesterov"])


def _optim():
    from xdfm_amd import optim
    return optim


def _needs_default_env(feature):
    env = {"arena": "XDFM_GRAD_ARENA", "graph": "XDFM_HIP_GRAPH"}[feature]
    if os.environ.get(env, "1") == "0":
        pytest.skip("%s=0" % env)


def _model(dev, make_optim, use_graph=False, seed=4):
    """A small xDeepFM compiled with make_optim(params); the train step's graph switched on or off."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(VOCAB)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(ND)]
    torch.manual_seed(seed)
    model = xDeepFM(cols, cols, dnn_hidden_units=(16, 8), cin_layer_size=(8, 6), l2_reg_dnn=1e-5, device=dev)
    model.compile(make_optim(list(model.parameters())), "binary_crossentropy", metrics=[])
    model.train()
    step = graphstep.GraphedStep(model)
    step.disabled = not use_graph
    model.__dict__["_graphed_step"] = step
    return model, step


def _table(nesterov=False, **kw):
    return lambda ps: _optim().TableSGD(ps, lr=LR, momentum=0.9, nesterov=nesterov, **kw)


def _batch(dev, s):
    from oracle import xdeepfm_oracle as orc
    X, y = orc.synthetic_batch(B, VOCAB, ND, seed=300 + s)
    return T(X).to(dev), T(y).to(dev)


def _buffers(model):
    """name -> momentum buffer (the parameters that have one)"""
    return {k: model.optim.state[p]["momentum_buffer"] for k, p in model.named_parameters() if "momentum_buffer" in model.optim.state.get(p, {})}


def _snapshot(model):
    """parameters and every momentum buffer, read without the model's own flush"""
    return [p.detach().clone() for p in model.parameters()] + [b.clone() for b in _buffers(model).values()]


def _spy(monkeypatch):
    """(names of the kernels ops._run launched, calls of torch.optim.SGD.step)"""
    from xdfm_amd import ops
    names, calls = [], []
    real_run, real_step = ops._run, torch.optim.SGD.step

    def run(name, work, fn):
        names.append(name)
        return real_run(name, work, fn)

    def step(self, *a, **kw):
        calls.append(type(self).__name__)
        return real_step(self, *a, **kw)
    monkeypatch.setattr(ops, "_run", run)
    monkeypatch.setattr(torch.optim.SGD, "step", step)
    return names, calls


def _shares(a, b):
    """Largest share of the p bar and of the buffer's bar between two models (b is the reference)."""
    out = {"p": 0.0, "s": 0.0}
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        if x.is_floating_point() and x.numel():
            out["p"] = max(out["p"], R.share(x.cpu().numpy(), y.cpu().numpy(), *R.TOL["p"]))
    ba, bb = _buffers(a), _buffers(b)
    assert sorted(ba) == sorted(bb) and len(ba) > 10
    for k in ba:
        out["s"] = max(out["s"], R.share(ba[k].cpu().numpy(), bb[k].cpu().numpy(), *R.TOL["s"]))
    return out


# --------------------------------------------------------------------------------------------- 1
@NES
def test_momentum_takes_the_native_route(nesterov, monkeypatch):
    """TableSGD(momentum=0.9[, nesterov=True]) handed to compile(): every step is one sgdm_step launch, torch.optim.SGD.step is
    never called, and the state is torch's layout.  (Before K7m existed `_native()` was False here and the stock step ran.)"""
    dev = _dev()
    names, calls = _spy(monkeypatch)
    model, _ = _model(dev, _table(nesterov))
    opt = model.optim
    assert type(opt).__name__ == "TableSGD" and model._optim_capturable and model._l2_fusion() is not None
    assert opt._native() and opt._kind(opt.param_groups[0]) == "sgdm"
    for s in range(3):
        model.train_on_batch(*_batch(dev, s))
        assert opt._native()
    assert [n for n in names if n.endswith("_step[bytes]")] == ["sgdm_step[bytes]"] * 3, names
    assert calls == []
    mine = {id(p) for p in model.parameters()}
    params = list(opt.state.keys())                # (a table's .grad is a view of the kept arena: state is what shows a step)
    assert len(params) > 10 and all(id(p) in mine for p in params)
    assert all(p in opt.state for k, p in model.named_parameters() if "embedding_dict" in k or k.startswith("dnn."))
    for p in params:
        st = opt.state[p]
        assert sorted(st.keys()) == ["momentum_buffer"]
        buf = st["momentum_buffer"]
        assert buf.is_cuda and buf.dtype == torch.float32 and buf.shape == p.shape and bool(torch.isfinite(buf).all())
    assert sum(int((opt.state[p]["momentum_buffer"] != 0).sum()) for p in params) > 1000


# --------------------------------------------------------------------------------------------- 2
def test_the_switch_gives_the_stock_route_back(monkeypatch):
    dev = _dev()
    names, calls = _spy(monkeypatch)
    monkeypatch.setattr(_optim(), "SGD_MOMENTUM_NATIVE", False)
    model, _ = _model(dev, _table(True))
    assert not model.optim._native()
    for s in range(3):
        model.train_on_batch(*_batch(dev, s))
    assert calls == ["TableSGD"] * 3 and not [n for n in names if n.endswith("_step[bytes]")], (calls, names)
    # momentum 0 keeps its kernel whatever the switch says
    plain, _ = _model(dev, lambda ps: _optim().TableSGD(ps, lr=LR))
    plain.train_on_batch(*_batch(dev, 0))
    assert [n for n in names if n.endswith("_step[bytes]")] == ["sgd_step[bytes]"] and len(calls) == 3


# --------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("path", ["loop", "own_step"])
@pytest.mark.parametrize("variant", ["mom", "nes"])
def test_model_vs_reference_golden(variant, path, cin_math):
    """Three steps as BaseModel.fit does them against the reference's run with torch.optim.SGD(momentum=0.9[, nesterov=True]) at
    the recorded rate: `loop` drives autograd by hand (dense gradients, L2 term through K6), `own_step` is train_on_batch
    (marked gradients, the L2 term inside the sweep).  Parameters AND momentum buffers, every element."""
    dev = _dev()
    g = load_golden(os.path.join("sgdm", "sgdm_sum_small_" + variant))
    base = load_golden(str(g["base"]))
    model = _build_model(g, dev)
    model.load_state_dict({k[3:]: T(v) for k, v in base.items() if k.startswith("s0:")}, strict=True)
    opt = _optim().TableSGD(model.parameters(), lr=float(g["lr"]), momentum=float(g["momentum"]), nesterov=bool(g["nesterov"]))
    model.compile(opt, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    model.train()
    X, y, Bg = T(base["X"]).to(dev), T(base["y"]).to(dev), int(g["B"])
    if path == "loop":
        losses = _three_steps_by_hand(model, X, y, Bg)
    else:
        losses = []
        for s in range(3):
            _, l, tot = model.train_on_batch(X[s * Bg:(s + 1) * Bg], y[s * Bg:(s + 1) * Bg])
            losses.append([float(l.reshape(-1)[0]), float(tot.reshape(-1)[0])])
    assert model.optim is opt and opt._native()
    np.testing.assert_allclose(np.array(losses), g["losses3"], rtol=2e-5)
    worst = 0.0
    bufs = _buffers(model)
    for k, v in model.state_dict().items():
        want = g["s3:" + k]
        if want.size:
            worst = max(worst, float((np.abs(v.detach().cpu().numpy() - want) / (2e-5 + 1e-3 * np.abs(want))).max()))
    for k in [k[5:] for k in g if k.startswith("buf3:")]:
        want = g["buf3:" + k]
        worst = max(worst, float((np.abs(bufs[k].cpu().numpy() - want) / (2e-5 + 1e-3 * np.abs(want))).max()))
    print("sgdm %s %s %s: worst share of the bar %.4f" % (variant, path, "f16x3" if cin_math else "f32mfma", worst))
    for k, v in model.state_dict().items():
        close(v, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="after 3 steps: " + k)
    for k in [k[5:] for k in g if k.startswith("buf3:")]:
        close(bufs[k], g["buf3:" + k], rtol=1e-3, atol=2e-5, msg="momentum buffer after 3 steps: " + k)


# --------------------------------------------------------------------------------------------- 4
@NES
def test_native_step_against_the_stock_fallback(nesterov, monkeypatch):
    """Twin models, four steps on one batch (the module docstring says why one): the native step, then -- the switch off -- the
    stock fallback with the armed L2 term applied by hand.  Parameters and momentum buffers within opt_ref.TOL."""
    dev = _dev()
    xb, yb = _batch(dev, 0)
    native, _ = _model(dev, _table(nesterov))
    for s in range(4):
        native.train_on_batch(xb, yb)
    assert native.optim._native()
    names, calls = _spy(monkeypatch)
    monkeypatch.setattr(_optim(), "SGD_MOMENTUM_NATIVE", False)
    stock, _ = _model(dev, _table(nesterov))
    for s in range(4):
        stock.train_on_batch(xb, yb)
    assert len(calls) == 4 and not stock.optim._native()
    sh = _shares(native, stock)
    print("sgdm native against the stock fallback, nesterov=%s: share of the bar p %.3f buffer %.3f" % (nesterov, sh["p"], sh["s"]))
    assert sh["p"] <= 1.0 and sh["s"] <= 1.0, sh
    moved = max(float((a - b).abs().max()) for a, b in zip(native.state_dict().values(), _model(dev, _table(nesterov))[0].state_dict().values()))
    assert moved > 1e-4


# --------------------------------------------------------------------------------------------- 5
@NES
def test_captured_step_equals_its_eager_twin_bit_for_bit(nesterov):
    """Ten steps of train_on_batch, the steps after the warm-up replayed from ONE captured graph, against the same steps
    launched eagerly: parameters and momentum buffers bit for bit.  A StepLR scheduler halves the rate after the fifth step:
    the graph reads it from the device scalar and is not captured again."""
    _needs_default_env("graph")
    from xdfm_amd import graphstep
    dev = _dev()

    def run(use_graph):
        model, step = _model(dev, _table(nesterov), use_graph)
        sched = torch.optim.lr_scheduler.StepLR(model.optim, step_size=5, gamma=0.5)
        entries = []
        for s in range(10):
            model.train_on_batch(*_batch(dev, s))
            sched.step()
            entries.append(len([e for e in step.entries.values() if e.graph is not None]))
        assert abs(model.optim.param_groups[0]["lr"] - LR / 4) < 1e-12
        return model, step, entries

    m_g, st_g, entries = run(True)
    m_e, st_e, _ = run(False)
    assert st_g.replays >= 7 and not st_g.disabled and st_e.replays == 0, (st_g.replays, st_g.disabled)
    assert entries[4] == entries[9] == 1                          # the new rate is followed by the SAME graph
    for e in st_g.entries.values():
        if e.graph is not None:
            n, n_memset, n_other = graphstep.census(e.graph)
            assert n > 20 and n_memset == 0 and n_other == 0
    for i, (a, b) in enumerate(zip(_snapshot(m_g), _snapshot(m_e))):
        assert torch.equal(a, b), "tensor %d: %d elements differ" % (i, int((a != b).sum()))
    assert m_g.optim._native() and sorted(_buffers(m_g)) == sorted(_buffers(m_e)) and len(_buffers(m_g)) > 10


# --------------------------------------------------------------------------------------------- 6
def _run_deferral(dev, deferred, use_graph, nesterov):
    model, step = _model(dev, _table(nesterov, deferred=deferred, flush_every=4), use_graph)
    snaps, behind = [], {}
    for s in range(11):
        if s == 6:                    # eval() in the middle of a period: the model flushes
            behind[s] = model.optim._since
            model.eval()
            snaps.append(_snapshot(model))
            model.train()
        if s == 9:                    # state_dict() in the middle of the next: flushes and drops the deferred state
            behind[s] = model.optim._since
            sd = model.optim.state_dict()
            assert len(sd["state"]) > 10 and model.optim._def is None
            snaps.append(_snapshot(model))
        model.train_on_batch(*_batch(dev, s))
    model.optim.flush()
    snaps.append(_snapshot(model))
    return model, step, snaps, behind


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@NES
def test_deferred_update_is_bit_identical_to_the_sweep(nesterov, use_graph):
    """Eleven steps with flush_every = 4 (more than two periods): parameters and every momentum buffer equal the sweep's with
    torch.equal after an eval() in the middle of a period, after a state_dict() in the middle of another, and at the end."""
    _needs_default_env("arena")
    if use_graph:
        _needs_default_env("graph")
    dev = _dev()
    m_s, st_s, sn_s, _ = _run_deferral(dev, False, use_graph, nesterov)
    m_d, st_d, sn_d, behind = _run_deferral(dev, True, use_graph, nesterov)
    assert m_d.optim._def is not None and m_s.optim._def is None
    assert m_s.optim.path_counts["scan"] == 0 and m_d.optim.path_counts["scan"] >= 2
    assert m_d.optim._def["kind"] == "sgdm" and len(m_d.optim._def["tensors"]) == 12          # 6 embedding + 6 linear tables
    assert all(v >= 1 for v in behind.values()), behind
    assert len(sn_s) == len(sn_d) == 3
    for n, (a, b) in enumerate(zip(sn_s, sn_d)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), "snapshot %d tensor %d: %d elements differ" % (n, i, int((x != y).sum()))
    if use_graph:
        assert st_d.replays > 0 and not st_d.disabled and st_s.replays > 0 and not st_s.disabled


# --------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("direction", ["native_to_stock", "stock_to_native"])
def test_checkpoints_interchange_with_torch_sgd(direction):
    """Three steps by one class, its optimizer's and model's state_dict() into the other, two more steps by both (one batch
    throughout): the loaded optimizer continues as the one that wrote the checkpoint, parameters and momentum buffers within
    opt_ref.TOL.  The stock class is a torch.optim.SGD object (L2 term through K6, the stock step)."""
    dev = _dev()
    xb, yb = _batch(dev, 1)
    stock_of = lambda ps: torch.optim.SGD(ps, lr=LR, momentum=0.9, nesterov=True)
    first, second = (_table(True), stock_of) if direction == "native_to_stock" else (stock_of, _table(True))
    writer, _ = _model(dev, first)
    for s in range(3):
        writer.train_on_batch(xb, yb)
    reader, _ = _model(dev, second, seed=9)
    reader.load_state_dict(writer.state_dict())
    # a copy, as a checkpoint that went through a file is: torch's load_state_dict keeps a tensor that already has the
    # parameter's dtype and device as it is, and the two optimizers would step one buffer
    reader.optim.load_state_dict(copy.deepcopy(writer.optim.state_dict()))
    assert reader.optim.param_groups[0]["momentum"] == 0.9 and reader.optim.param_groups[0]["nesterov"] is True
    for a, b in zip(_buffers(reader).values(), _buffers(writer).values()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    for s in range(2):
        writer.train_on_batch(xb, yb)
        reader.train_on_batch(xb, yb)
    native = writer if direction == "native_to_stock" else reader
    assert type(native.optim).__name__ == "TableSGD" and native.optim._native()
    assert type((reader if native is writer else writer).optim) is torch.optim.SGD
    sh = _shares(reader, writer)
    print("sgdm checkpoint %s: share of the bar p %.3f buffer %.3f" % (direction, sh["p"], sh["s"]))
    assert sh["p"] <= 1.0 and sh["s"] <= 1.0, sh


# --------------------------------------------------------------------------------------------- 8
def test_dampening_still_falls_back_and_equals_torch(monkeypatch):
    dev = _dev()
    names, calls = _spy(monkeypatch)
    torch.manual_seed(5)
    init = [torch.randn(s, device=dev) * 0.05 for s in [(301, 16), (513,), (11,)]]
    pa = [torch.nn.Parameter(t.clone()) for t in init]
    pb = [torch.nn.Parameter(t.clone()) for t in init]
    kw = dict(lr=1e-3, momentum=0.9, dampening=0.1)
    oa, ob = _optim().TableSGD(pa, **kw), torch.optim.SGD(pb, **kw)
    for step in range(4):
        for p, q in zip(pa, pb):
            p.grad = torch.randn_like(p) * 0.1
            q.grad = p.grad.clone()
        assert not oa._native()
        if step == 2:
            oa.arm_l2(pa[:1], [0.05])
            want = 0.05 * float(pb[0].detach().double().square().sum())
            pb[0].grad.add_(pb[0].detach(), alpha=0.1)
        oa.step()
        ob.step()
        if step == 2:
            assert abs(float(oa.l2_value) - want) <= 1e-5 * want
    assert calls.count("TableSGD") == 4 and not names
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)
        assert sorted(oa.state[p].keys()) == sorted(ob.state[q].keys()) == ["momentum_buffer"]
        assert torch.equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"])
