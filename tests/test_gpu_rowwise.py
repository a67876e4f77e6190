"""GPU tests (-m gpu) of row-wise Adagrad through the model (K7w / K7g behind xdfm_amd.optim.TableRowwiseAdagrad):
compile("rowwise_adagrad") takes the native route; train steps against rw_f64 applied to the gradients the step saw; graph replay
against eager launches and the kept gradient arena against fresh gradients, bit for bit; with the tables' L2 term off, untouched
rows keep their bits; state shapes; a checkpoint that continues bit for bit.

The model: a small xDeepFM with vocabularies 50 / 7 / 1000 / 33, D = 8, two dense fields, cin (8, 6), dnn (16,), B = 64, five
steps; one variant with D = 10 (chunks straddle rows: the units path), one with a VarLenSparseFeat column, whose table gets a
dense gradient.  The bar against float64 is rowwise_ref's: C 2^-24 (|p| + |lr g' / den|), one step at a time."""
import copy
import os

import numpy as np
import pytest
import torch

import rowwise_ref as W
from test_gpu_optim import _dev
from test_rowwise_capi import record_steps, worst_ratios

pytestmark = pytest.mark.gpu
VOCAB, ND, B, STEPS = [50, 7, 1000, 33], 2, 64, 5
VARIANTS = {"D8": dict(D=8, varlen=False), "D10": dict(D=10, varlen=False), "varlen": dict(D=8, varlen=True)}
VV, MAXLEN = 9, 4


def _needs_default_env(feature):
    env = {"arena": "XDFM_GRAD_ARENA", "graph": "XDFM_HIP_GRAPH"}[feature]
    if os.environ.get(env, "1") == "0":
        pytest.skip("%s=0" % env)


def _model(dev, variant="D8", optimizer="rowwise_adagrad", use_graph=False, seed=4, **model_kw):
    from deepctr.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    v = VARIANTS[variant]
    cols = [SparseFeat("C%d" % (i + 1), n, v["D"]) for i, n in enumerate(VOCAB)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(ND)]
    if v["varlen"]:
        cols.append(VarLenSparseFeat(SparseFeat("tags", VV, v["D"]), maxlen=MAXLEN, combiner="mean"))
    torch.manual_seed(seed)
    model = xDeepFM(cols, cols, dnn_hidden_units=(16,), cin_layer_size=(8, 6), l2_reg_dnn=1e-5, device=dev, **model_kw)
    model.compile(optimizer if isinstance(optimizer, str) else optimizer(model), "binary_crossentropy", metrics=[])
    model.train()
    step = graphstep.GraphedStep(model)
    step.disabled = not use_graph
    model.__dict__["_graphed_step"] = step
    return model, step


def _batch(model, dev, s):
    """A batch laid out by the model's feature index: ids, dense values, and for the VarLenSparseFeat column 1 .. MAXLEN ids
    followed by the padding id 0."""
    rng = np.random.RandomState(300 + s)
    width = max(hi for _, hi in model.feature_index.values())
    X = np.zeros((B, width), np.float32)
    for name, (lo, hi) in model.feature_index.items():
        if name.startswith("C"):
            X[:, lo] = rng.randint(0, VOCAB[int(name[1:]) - 1], B)
        elif name.startswith("I"):
            X[:, lo:hi] = rng.rand(B, hi - lo)
        else:
            n = rng.randint(1, MAXLEN + 1, B)
            ids = rng.randint(1, VV, (B, MAXLEN))
            X[:, lo:hi] = np.where(np.arange(MAXLEN)[None, :] < n[:, None], ids, 0)
    y = (rng.rand(B, 1) < 0.4).astype(np.float32)
    return torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)


def _snapshot(model):
    out = [p.detach().clone() for p in model.parameters()]
    out += [model.optim.state[p]["sum"].clone() for p in model.parameters() if "sum" in model.optim.state.get(p, {})]
    return out


def _assert_same(a, b, what):
    assert len(a) == len(b) and len(a) > 20, (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s, tensor %d %r: %d elements differ" % (what, i, tuple(x.shape), int((x != y).sum()))


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
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_route_is_native_and_the_steps_lie_within_the_bar_of_float64(variant, monkeypatch):
    """compile("rowwise_adagrad"): the class with its two groups; every step is one rowwise_step and one adagrad_step launch,
    never the torch-op step; the tables' L2 term is armed and the marked gradients are read and re-zeroed; state shapes are
    [rows] for the tables and the parameter's shape otherwise.  Every one of the five steps, parameters and `sum`, lies within the
    bar of rw_f64 applied to the state and the gradients the step saw; the armed term's value within its rtol."""
    from xdfm_amd.optim import TableRowwiseAdagrad
    dev = _dev()
    names = _spy(monkeypatch)
    stock = []
    monkeypatch.setattr(TableRowwiseAdagrad, "_stock_step", lambda self, closure: stock.append(1))
    model, _ = _model(dev, variant)
    opt = model.optim
    assert type(opt) is TableRowwiseAdagrad and model._optim_capturable and model._l2_fusion() is not None
    assert [g["rowwise"] for g in opt.param_groups] == [True, False]
    ntab = 2 * (len(VOCAB) + (1 if VARIANTS[variant]["varlen"] else 0))
    assert len(opt.param_groups[0]["params"]) == ntab
    log = []
    record_steps(opt, log)
    for s in range(STEPS):
        out = model.train_on_batch(*_batch(model, dev, s))
        assert opt._native() and opt.l2_value is not None and float(opt.l2_value) > 0
        assert bool(torch.isfinite(out[2]).all())
    steps = [n for n in names if n.endswith("_step[bytes]")]
    assert steps == ["rowwise_step[bytes]", "adagrad_step[bytes]"] * STEPS, steps
    assert stock == [] and opt.deferred is False and opt._def is None
    if os.environ.get("XDFM_GRAD_ARENA", "1") != "0":
        assert len(opt.grad_sources) >= 1
        for a in model._plan.arenas():                     # the marked chunks were read, re-zeroed and unmarked
            assert not a.pending and float(a.flat.abs().max()) == 0.0 and int(a.marks.max()) == 0
    for p in opt.param_groups[0]["params"]:
        acc = opt.state[p]["sum"]
        assert acc.shape == (p.shape[0],) and acc.is_cuda and acc.dtype == torch.float32 and bool(torch.isfinite(acc).all())
    for p in opt.param_groups[1]["params"]:
        assert opt.state[p]["sum"].shape == p.shape
    assert len(log) == STEPS and all(len(rec) > 10 for rec, _ in log)
    assert sum(1 for r in log[0][0] if r[4] > 0) >= ntab                # the tables (and the DNN weights) carry an L2 term
    wp, ws, values = worst_ratios(opt, log)
    print("row-wise model %s: worst ratio p %.3f s %.3f (C = %g)" % (variant, wp, ws, W.C_BAR))
    assert wp <= W.C_BAR and ws <= W.C_BAR
    for (rec, l2_value), value in zip(log, values):
        assert abs(float(l2_value) - value) <= W.L2_RTOL * value, (float(l2_value), value)


# --------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_captured_step_equals_its_eager_twin_bit_for_bit(variant):
    """Eight steps of train_on_batch, the steps after the warm-up replayed from ONE captured graph, against the same steps
    launched eagerly: parameters and `sum` bit for bit.  The rate of both groups changes after the fifth step: the graph reads it
    from the device scalars and is not captured again."""
    _needs_default_env("graph")
    dev = _dev()

    def run(use_graph):
        model, step = _model(dev, variant, use_graph=use_graph)
        entries = []
        for s in range(8):
            if s == 5:
                for g in model.optim.param_groups:
                    g["lr"] = 0.02
            model.train_on_batch(*_batch(model, dev, s))
            entries.append(len([e for e in step.entries.values() if e.graph is not None]))
        return model, step, entries

    m_g, st_g, entries = run(True)
    m_e, st_e, _ = run(False)
    assert st_g.replays >= 5 and not st_g.disabled and st_e.replays == 0, (st_g.replays, st_g.disabled)
    assert entries[4] == entries[7] == 1                          # the new rate is followed by the SAME graph
    _assert_same(_snapshot(m_g), _snapshot(m_e), "graph against eager")
    assert m_g.optim._native() and m_g.optim._lr_dev[0][0] == 0.02 and m_g.optim._lr_dev[1][0] == 0.02


# --------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("model_l2", [True, False], ids=["model_l2", "no_model_l2"])
def test_fresh_gradients_equal_the_kept_arena_bit_for_bit(model_l2, variant):
    """XDFM_GRAD_ARENA=0 (a fresh, zero-filled table gradient every step, read in full) against the default (the kept arena,
    read by its marks): parameters and `sum` bit for bit after five steps -- with the model's L2 term on the tables (every row
    is an update) and with l2_reg_embedding = l2_reg_linear = 0 (rows without a marked chunk are skipped).  In the second
    configuration a row no batch touched is where it started: the bits of p, and `sum` at its initial value."""
    _needs_default_env("arena")
    dev = _dev()
    kw = {} if model_l2 else dict(l2_reg_embedding=0.0, l2_reg_linear=0.0)

    def run(arena):
        os.environ["XDFM_GRAD_ARENA"] = "1" if arena else "0"
        try:
            model, _ = _model(dev, variant, **kw)
            seen = [set() for _ in VOCAB]
            for s in range(STEPS):
                X, y = _batch(model, dev, s)
                for i in range(len(VOCAB)):
                    seen[i].update(int(v) for v in X[:, model.feature_index["C%d" % (i + 1)][0]].cpu().numpy())
                model.train_on_batch(X, y)
            return model, seen
        finally:
            os.environ.pop("XDFM_GRAD_ARENA", None)

    (m_a, seen), (m_z, _) = run(True), run(False)
    assert len(m_a._plan.arenas()) == 1 and len(m_z._plan.arenas()) == 0
    _assert_same(_snapshot(m_a), _snapshot(m_z), "arena against fresh gradients")
    if not model_l2:
        fresh, _ = _model(dev, variant, **kw)
        still = 0
        for (k, p), (_, q) in zip(m_a.named_parameters(), fresh.named_parameters()):
            if "embedding_dict.C" in k:
                i = int(k.split("embedding_dict.C")[1].split(".")[0]) - 1
                rows = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
                rows[sorted(seen[i])] = False
                acc = m_a.optim.state[p]["sum"]
                assert torch.equal(p[rows].view(torch.int32), q[rows].view(torch.int32)), k
                assert bool((acc[rows] == 0).all()) and bool((acc[~rows] > 0).all()), k
                still += int(rows.sum())
        print("row-wise without a table L2 term (%s): %d table rows no batch touched" % (variant, still))
        assert still > 1000


# --------------------------------------------------------------------------------------------- 4
def test_a_checkpoint_continues_bit_for_bit_and_adagrad_is_still_adagrad():
    """The model's and the optimizer's state_dict() loaded into a fresh model (other initial weights) and a fresh optimizer: two
    more steps by both, parameters and `sum` bit for bit.  compile("adagrad") on the same model still builds TableAdagrad, with
    per-element state."""
    from xdfm_amd.optim import TableAdagrad, TableRowwiseAdagrad
    dev = _dev()
    make = lambda m: TableRowwiseAdagrad.for_model(m, lr=0.05, eps=1e-8, initial_accumulator_value=0.1)     # noqa: E731
    writer, _ = _model(dev, "D8", make)
    for s in range(3):
        writer.train_on_batch(*_batch(writer, dev, s))
    reader, _ = _model(dev, "D8", make, seed=9)
    reader.load_state_dict(writer.state_dict())
    gen = reader.optim.generation
    reader.optim.load_state_dict(copy.deepcopy(writer.optim.state_dict()))       # a copy, as a checkpoint from a file is
    assert reader.optim.generation > gen and reader.optim.param_groups[0]["eps"] == 1e-8
    for p in reader.optim.param_groups[0]["params"]:
        assert reader.optim.state[p]["sum"].shape == (p.shape[0],) and float(reader.optim.state[p]["sum"].min()) >= float(np.float32(0.1))
    _assert_same(_snapshot(reader), _snapshot(writer), "after loading")
    for s in range(3, 5):
        writer.train_on_batch(*_batch(writer, dev, s))
        reader.train_on_batch(*_batch(reader, dev, s))
    _assert_same(_snapshot(reader), _snapshot(writer), "two steps after loading")
    assert reader.optim._native()
    writer.compile("adagrad", "binary_crossentropy", metrics=[])
    assert type(writer.optim) is TableAdagrad and len(writer.optim.param_groups) == 1
    writer.train_on_batch(*_batch(writer, dev, 7))
    assert all(writer.optim.state[p]["sum"].shape == p.shape for p in writer.parameters())
