"""GPU tests (-m gpu) of FTRL-Proximal through the model (K7f behind xdfm_amd.optim.TableFTRL): compile("ftrl") takes the
native route; train steps against ftrl_f64 applied to the gradients the step saw; graph replay against eager launches bit for
bit, a change of the rate between replays included; the kept gradient arena against fresh gradients bit for bit; the exact
zeros of the L1 term and a checkpoint that continues bit for bit.  The model is the size of `model_sum_small`: six sparse fields
with vocabularies of at most 11 rows, D = 4, B = 32, cin (8, 6), dnn (16, 8).

Bars against float64: ftrl_ref.TOL and the threshold cap, as tests/test_gpu_ftrl_abi.py.  Every step is compared on its own,
from the fp32 state it started with, so the signed sum z does not carry a rounding history (ftrl_ref.py, "THE SIGNS")."""
import copy
import os

import numpy as np
import pytest
import torch

import ftrl_ref as F
from test_gpu_optim import _dev

pytestmark = pytest.mark.gpu
T = torch.from_numpy
VOCAB, ND, D, B = [11, 7, 9, 5, 3, 10], 3, 4, 32


def _needs_default_env(feature):
    env = {"arena": "XDFM_GRAD_ARENA", "graph": "XDFM_HIP_GRAPH"}[feature]
    if os.environ.get(env, "1") == "0":
        pytest.skip("%s=0" % env)


def _model(dev, optimizer="ftrl", use_graph=False, seed=4, **model_kw):
    """A tiny xDeepFM compiled with `optimizer` (a name, or params -> an object); the train step's graph switched on or off."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(VOCAB)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(ND)]
    torch.manual_seed(seed)
    model = xDeepFM(cols, cols, dnn_hidden_units=(16, 8), cin_layer_size=(8, 6), l2_reg_dnn=1e-5, device=dev, **model_kw)
    model.compile(optimizer if isinstance(optimizer, str) else optimizer(list(model.parameters())), "binary_crossentropy", metrics=[])
    model.train()
    step = graphstep.GraphedStep(model)
    step.disabled = not use_graph
    model.__dict__["_graphed_step"] = step
    return model, step


def _ftrl(**kw):
    from xdfm_amd.optim import TableFTRL
    return lambda ps: TableFTRL(ps, **kw)


def _batch(dev, s):
    from oracle import xdeepfm_oracle as orc
    X, y = orc.synthetic_batch(B, VOCAB, ND, seed=300 + s)
    return T(X).to(dev), T(y).to(dev)


def _snapshot(model):
    """parameters, then z and n of every parameter that has state"""
    out = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        st = model.optim.state.get(p, {})
        out += [st[k].clone() for k in ("z", "n") if k in st]
    return out


def _assert_same(a, b, what):
    assert len(a) == len(b) and len(a) > 30, (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s, tensor %d: %d elements differ" % (what, i, int((x != y).sum()))


def _spy(monkeypatch):
    from xdfm_amd import ops
    names = []
    real_run = ops._run

    def run(name, work, fn):
        names.append(name)
        return real_run(name, work, fn)
    monkeypatch.setattr(ops, "_run", run)
    return names


# --------------------------------------------------------------------------------------------- 1
def test_compile_ftrl_takes_the_native_route(monkeypatch):
    """compile("ftrl"): a TableFTRL with the defaults whose every step is one ftrl_step launch -- never the torch-op step -- with
    the model's L2 term armed, the table gradients read by their marks, and z / n as state."""
    from xdfm_amd.optim import TableFTRL
    dev = _dev()
    names = _spy(monkeypatch)
    stock = []
    monkeypatch.setattr(TableFTRL, "_stock_step", lambda self, closure: stock.append(1))
    model, _ = _model(dev)
    opt = model.optim
    g = opt.param_groups[0]
    assert type(opt) is TableFTRL and model._optim_capturable and model._l2_fusion() is not None
    assert (g["lr"], g["l1"], g["l2"], g["beta"], g["initial_accumulator_value"]) == (0.05, 0.0, 0.0, 1.0, 0.1)
    for s in range(3):
        out = model.train_on_batch(*_batch(dev, s))
        assert opt._native() and opt.l2_value is not None and float(opt.l2_value) > 0
        assert bool(torch.isfinite(out[2]).all())
    assert [n for n in names if n.endswith("_step[bytes]")] == ["ftrl_step[bytes]"] * 3, names
    assert stock == [] and opt.deferred is False and opt._def is None
    if os.environ.get("XDFM_GRAD_ARENA", "1") != "0":
        assert len(opt.grad_sources) == 1 and len(model._plan.arenas()) == 1
        for a in model._plan.arenas():                     # the marked chunks were read, re-zeroed and unmarked
            assert not a.pending and float(a.flat.abs().max()) == 0.0 and int(a.marks.max()) == 0
    params = list(opt.state.keys())
    assert len(params) > 10
    for p in params:
        st = opt.state[p]
        assert sorted(st.keys()) == ["n", "z"]
        for k in "zn":
            assert st[k].is_cuda and st[k].dtype == torch.float32 and st[k].shape == p.shape and bool(torch.isfinite(st[k]).all())
        assert float(st["n"].min()) >= float(np.float32(0.1))
    assert sum(int((opt.state[p]["z"] != 0).sum()) for p in params) > 500


# --------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("hyper", [dict(), dict(lr=0.05, l1=1e-3, l2=1e-3, beta=0.5, initial_accumulator_value=0.1)], ids=["defaults", "l1_l2"])
def test_train_steps_against_float64_on_the_gradients_the_step_saw(hyper):
    """Three train_on_batch steps (eager launches).  Before each optimizer step the test keeps every parameter, its z and n, its
    gradient and its armed L2 strength; afterwards parameter, z and n lie within the bars of ftrl_f64 applied to exactly
    those, and the armed term's value within its rtol."""
    dev = _dev()
    model, _ = _model(dev, _ftrl(**hyper))
    opt = model.optim
    g = opt.param_groups[0]
    log = []
    real = opt.step

    def step(closure=None):
        armed = dict(opt._armed or {})
        rec = []
        for p in g["params"]:
            if p.grad is None:
                continue
            st = opt.state.get(p, {})
            z = st["z"].clone() if "z" in st else torch.zeros_like(p)
            n = st["n"].clone() if "n" in st else torch.full_like(p, g["initial_accumulator_value"])
            rec.append((p, p.detach().clone(), z, n, p.grad.detach().clone(), armed.get(id(p), 0.0)))
        out = real(closure)
        log.append((rec, opt.l2_value))            # (the tensor itself: its value is final once the step's finish batch has run)
        return out
    opt.step = step
    for s in range(3):
        model.train_on_batch(*_batch(dev, s))
    assert len(log) == 3 and opt._native()
    worst, left = dict.fromkeys("pzn", 0.0), 0
    for s, (rec, l2_value) in enumerate(log):
        assert len(rec) > 10 and sum(1 for r in rec if r[5] > 0) >= 12          # the tables and the DNN weights carry an L2 term
        got, want, value = [], [], 0.0
        for p, p0, z0, n0, grad, l2m in rec:
            w = F.ftrl_f64(p0.cpu().numpy().ravel(), z0.cpu().numpy().ravel(), n0.cpu().numpy().ravel(), grad.cpu().numpy().ravel(),
                           g["lr"], l2m, g["l1"], g["l2"], g["beta"])
            want.append(w[:3])
            value += w[3]
        if s < 2:                                           # the state after the step is the next record's start
            nxt = {id(r[0]): r for r in log[s + 1][0]}
            got = [tuple(nxt[id(r[0])][k].cpu().numpy().ravel() for k in (1, 2, 3)) for r in rec]
        else:
            got = [(r[0].detach().cpu().numpy().ravel(), opt.state[r[0]]["z"].cpu().numpy().ravel(), opt.state[r[0]]["n"].cpu().numpy().ravel())
                   for r in rec]
        shares, out_n, excess = F.compare(got, want, g["l1"])
        assert excess <= 0
        for k, (a, w) in enumerate(zip(got, want)):           # the element that uses most of the z bar, for the log
            r = np.abs(a[1] - w[1]) / (F.TOL["z"][1] + F.TOL["z"][0] * np.abs(w[1]))
            if r.size and float(r.max()) == shares["z"]:
                i = int(r.argmax())
                print("step %d tensor %d %r element %d: z %.9g want %.9g from p %.6g z %.6g n %.6g g %.6g l2m %g" % (
                    s + 1, k, tuple(rec[k][0].shape), i, a[1][i], w[1][i], rec[k][1].flatten()[i], rec[k][2].flatten()[i],
                    rec[k][3].flatten()[i], rec[k][4].flatten()[i], rec[k][5]))
        worst = {q: max(worst[q], shares[q]) for q in "pzn"}
        left += out_n
        assert abs(float(l2_value) - value) <= F.L2_RTOL * value, (float(l2_value), value)
    print("ftrl model %r: share of the bar %r, %d elements left out" % (hyper, worst, left))
    assert all(x <= 1.0 for x in worst.values()), worst


# --------------------------------------------------------------------------------------------- 3
def test_captured_step_equals_its_eager_twin_bit_for_bit():
    """Eight steps of train_on_batch, the steps after the warm-up replayed from ONE captured graph, against the same steps
    launched eagerly: parameters, z and n bit for bit.  param_groups[0]["lr"] changes after the fifth step: the graph reads
    the rate from the device scalar and is not captured again."""
    _needs_default_env("graph")
    dev = _dev()

    def run(use_graph):
        model, step = _model(dev, _ftrl(lr=0.05, l1=1e-3, l2=1e-3), use_graph)
        entries = []
        for s in range(8):
            if s == 5:
                model.optim.param_groups[0]["lr"] = 0.02
            model.train_on_batch(*_batch(dev, s))
            entries.append(len([e for e in step.entries.values() if e.graph is not None]))
        return model, step, entries

    m_g, st_g, entries = run(True)
    m_e, st_e, _ = run(False)
    assert st_g.replays >= 5 and not st_g.disabled and st_e.replays == 0, (st_g.replays, st_g.disabled)
    assert entries[4] == entries[7] == 1                          # the new rate is followed by the SAME graph
    _assert_same(_snapshot(m_g), _snapshot(m_e), "graph against eager")
    assert m_g.optim._native() and m_g.optim._lr_dev[0][0] == 0.02


# --------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("model_l2", [True, False], ids=["model_l2", "no_model_l2"])
def test_fresh_gradients_equal_the_kept_arena_bit_for_bit(model_l2):
    """XDFM_GRAD_ARENA=0 (a fresh, zero-filled table gradient every step, read in full) against the default (the kept arena,
    read by its marks): parameters, z and n bit for bit after four steps -- with the model's L2 term on the tables (every chunk
    is an update) and with l2_reg_embedding = l2_reg_linear = 0, FTRL's own l2 in their place (unmarked chunks are skipped)."""
    _needs_default_env("arena")
    dev = _dev()
    kw = {} if model_l2 else dict(l2_reg_embedding=0.0, l2_reg_linear=0.0)

    def run(arena):
        os.environ["XDFM_GRAD_ARENA"] = "1" if arena else "0"
        try:
            model, _ = _model(dev, _ftrl(lr=0.05, l1=1e-3, l2=1e-3), **kw)
            for s in range(4):
                model.train_on_batch(*_batch(dev, s))
            return model
        finally:
            os.environ.pop("XDFM_GRAD_ARENA", None)

    m_a, m_z = run(True), run(False)
    assert len(m_a._plan.arenas()) == 1 and len(m_z._plan.arenas()) == 0
    _assert_same(_snapshot(m_a), _snapshot(m_z), "arena against fresh gradients")
    if not model_l2:                                        # a row no batch touched is where it started, with no state moved
        fresh, _ = _model(dev, _ftrl(lr=0.05, l1=1e-3, l2=1e-3), **kw)
        still = 0
        for (k, p), (_, q) in zip(m_a.named_parameters(), fresh.named_parameters()):
            if "embedding_dict" in k:
                rows = (m_a.optim.state[p]["z"] == 0).all(dim=1)
                assert torch.equal(p[rows], q[rows]) and bool((m_a.optim.state[p]["n"][rows] == np.float32(0.1)).all())
                still += int(rows.sum())
        print("ftrl without a model L2 term: %d embedding rows no batch touched" % still)


# --------------------------------------------------------------------------------------------- 5
def test_l1_leaves_exact_zeros_and_a_checkpoint_continues_bit_for_bit():
    """l1 = 1e-2: after three steps some table elements are exactly 0.0.  The model's and the optimizer's state_dict() loaded
    into a fresh model (other initial weights): two more steps by both, parameters, z and n bit for bit."""
    dev = _dev()
    make = _ftrl(lr=0.05, l1=1e-2, l2=1e-3)
    writer, _ = _model(dev, make)
    for s in range(3):
        writer.train_on_batch(*_batch(dev, s))
    zeros = sum(int((p == 0).sum()) for k, p in writer.named_parameters() if "embedding_dict" in k)
    total = sum(p.numel() for k, p in writer.named_parameters() if "embedding_dict" in k)
    print("ftrl l1 = 1e-2: %d of %d embedding elements are exactly 0.0 after three steps" % (zeros, total))
    assert 0 < zeros
    reader, _ = _model(dev, make, seed=9)
    reader.load_state_dict(writer.state_dict())
    gen = reader.optim.generation
    reader.optim.load_state_dict(copy.deepcopy(writer.optim.state_dict()))       # a copy, as a checkpoint from a file is
    assert reader.optim.generation > gen and reader.optim.param_groups[0]["l1"] == 1e-2
    _assert_same(_snapshot(reader), _snapshot(writer), "after loading")
    for s in range(3, 5):
        writer.train_on_batch(*_batch(dev, s))
        reader.train_on_batch(*_batch(dev, s))
    _assert_same(_snapshot(reader), _snapshot(writer), "two steps after loading")
    assert reader.optim._native() and sum(int((p == 0).sum()) for k, p in reader.named_parameters() if "embedding_dict" in k) > 0
