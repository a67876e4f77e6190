"""GPU tests (-m gpu) of the deferred (exact) SGD / Adagrad table update (K7sd / K7gd, include/xdfm.h): every comparison is
against the dense sweep of the same class (`deferred=False`), which tests/test_gpu_optim.py and the goldens tie to
torch.optim -- and the comparison is bit for bit wherever the quantity is a tensor the optimizer writes."""
import io
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T = torch.from_numpy
ND, D = 3, 16
VOCAB = [5000, 31, 20003, 3, 9, 402]     # 20003 % 4 != 0: the linear table has tail rows the sweep always updates; 3 rows: a table that is all tail
KINDS = ["sgd", "adagrad"]


def _needs_default_env(feature):
    """Tests that assert a feature is ACTIVE skip when the environment switches it off (supported ways to run the product)."""
    env = {"arena": "XDFM_GRAD_ARENA", "graph": "XDFM_HIP_GRAPH"}[feature]
    if os.environ.get(env, "1") == "0":
        pytest.skip("%s=0" % env)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cls(kind):
    from xdfm_amd import optim
    return {"sgd": optim.TableSGD, "adagrad": optim.TableAdagrad, "rmsprop": optim.TableRMSprop, "adam": optim.TableAdam}[kind]


def _big_vocab_model(dev, kind, deferred, use_graph, flush_every=5, emb_dim=D, vocab=VOCAB, seed=4, metrics=(), **kw):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    cols = [SparseFeat("C%d" % (i + 1), v, emb_dim) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(ND)]
    torch.manual_seed(seed)
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev, **kw)
    with torch.no_grad():                           # weights large enough for the L2 pull to move bits every step
        for k, p in model.named_parameters():
            if "embedding_dict" in k:
                p.mul_(2000.0)
    model.compile(kind, "binary_crossentropy", metrics=list(metrics))
    assert type(model.optim) is _cls(kind)
    model.optim.deferred = deferred
    model.optim.flush_every = flush_every
    model.train()
    step = graphstep.GraphedStep(model)
    step.disabled = not use_graph
    model.__dict__["_graphed_step"] = step
    return model, step


def _opt_state(model):
    """Every Adagrad `sum` and every host `state["step"]`, in parameter order (SGD without momentum keeps no state)."""
    out = []
    for g in model.optim.param_groups:
        for p in g["params"]:
            st = model.optim.state.get(p, {})
            out.append((st["sum"].clone() if "sum" in st else None, float(st["step"]) if "step" in st else None))
    return out


def _same_state(a, b):
    assert len(a) == len(b)
    for (sa, na), (sb, nb) in zip(a, b):
        assert na == nb, (na, nb)
        assert (sa is None) == (sb is None)
        if sa is not None:
            assert torch.equal(sa, sb)


def _run23(dev, kind, deferred, use_graph, emb_dim):
    from oracle import xdeepfm_oracle as orc
    model, step = _big_vocab_model(dev, kind, deferred, use_graph, emb_dim=emb_dim)
    total, pred = 0.0, None
    for s in range(23):
        if s == 9:
            for g in model.optim.param_groups:
                g["lr"] = 3e-3
        X, y = orc.synthetic_batch(256, VOCAB, ND, seed=500 + s)
        out = model.train_on_batch(T(X).to(dev), T(y).to(dev))
        total += float(out[2])
        if s == 12:
            model.eval()
            with torch.no_grad():
                pred = model(T(X).to(dev)).clone()
            model.train()
    model.optim.flush()
    total += model.optim.take_backlog()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    return model, step, sd, _opt_state(model), total, pred


_RUNS = {}


def _runs(kind, use_graph, emb_dim):
    key = (kind, use_graph, emb_dim)
    if key not in _RUNS:
        dev = _dev()
        _RUNS[key] = (_run23(dev, kind, False, use_graph, emb_dim), _run23(dev, kind, True, use_graph, emb_dim))
    return _RUNS[key]


CASES = [(False, D), (True, D), (True, 10)]
CASE_IDS = ["eager", "graph", "graph-D10"]


@pytest.mark.parametrize("use_graph,emb_dim", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_deferred_table_update_is_bit_identical_to_the_dense_sweep(kind, use_graph, emb_dim):
    """Rows are updated when gathered / when a gradient arrives / every `flush_every` = 5 steps instead of every step.
    Parameters, every Adagrad `sum` and every `state["step"]` must equal the dense sweep's BIT FOR BIT after 23 steps with
    cold and hot rows, a learning-rate change at step 9, a prediction in the middle (flush) and flushes at steps that are
    not multiples of the period.  Eager launches, HIP-graph replay, and D = 10 (rows straddle 16-byte chunks)."""
    _needs_default_env('arena')
    if use_graph:
        _needs_default_env('graph')
    (m_d, st_d, sd_d, os_d, _, pred_d), (m_l, st_l, sd_l, os_l, _, pred_l) = _runs(kind, use_graph, emb_dim)
    assert m_l.optim._def is not None and m_d.optim._def is None
    assert m_l.optim.path_counts["scan"] >= 2 and m_d.optim.path_counts["scan"] == 0
    assert len(m_l.optim._def["tensors"]) == 12           # 6 embedding + 6 linear tables
    if use_graph:
        assert st_l.replays >= 15 and not st_l.disabled
        assert st_d.replays >= 15 and not st_d.disabled
    assert torch.equal(pred_d, pred_l)
    for k in sd_d:
        assert torch.equal(sd_d[k], sd_l[k]), k
    _same_state(os_d, os_l)
    if kind == "adagrad":
        assert all(n == 23.0 for _, n in os_l)


@pytest.mark.parametrize("use_graph,emb_dim", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_deferred_epoch_loss_with_the_backlog_matches_the_dense_sweep(kind, use_graph, emb_dim):
    """The same 23-step runs: the per-step `total_loss` summed, plus `take_backlog()` after a final flush, agrees with the
    dense run within 2e-6 relative (the bound of the Adam test for the same quantity: the two runs sum the same terms in a
    different order)."""
    _needs_default_env('arena')
    if use_graph:
        _needs_default_env('graph')
    (_, _, _, _, tot_d, _), (_, _, _, _, tot_l, _) = _runs(kind, use_graph, emb_dim)
    print("epoch loss %s graph=%s D=%d: dense %.9g deferred %.9g rel %.3g" % (kind, use_graph, emb_dim, tot_d, tot_l,
                                                                              abs(tot_d - tot_l) / abs(tot_d)))
    assert math.isfinite(tot_d) and abs(tot_d - tot_l) <= 2e-6 * abs(tot_d), (tot_d, tot_l)


@pytest.mark.parametrize("kind", KINDS)
def test_deferred_fit_history_checkpoint_and_user_driven_step(kind):
    """`fit` over 2 epochs with a validation split on the default graph path, flush_every = 7: the History equals the dense
    sweep's (rtol 2e-6 / atol 1e-9), a checkpoint (state_dict, torch.save of the model) holds current rows, and a
    user-driven step (plain backward + optim.step: dense gradients without marks) after deferred steps is taken densely on
    rows that were brought up to date first."""
    _needs_default_env('arena')
    from oracle import xdeepfm_oracle as orc
    dev = _dev()

    def run(deferred):
        model, _ = _big_vocab_model(dev, kind, deferred, True, flush_every=7, metrics=["binary_crossentropy", "auc"])
        model.__dict__.pop("_graphed_step", None)        # the default graph path of fit
        X, y = orc.synthetic_batch(3000, VOCAB, ND, seed=77)
        names = list(model.feature_index.keys())
        xd = {n: X[:, model.feature_index[n][0]] for n in names}
        hist = model.fit(xd, y, batch_size=256, epochs=2, verbose=0, validation_split=0.1, shuffle=False)
        # three more deferred steps, so that rows are behind when the checkpoints are taken
        for s in range(3):
            Xb, yb = orc.synthetic_batch(256, VOCAB, ND, seed=40 + s)
            model.train_on_batch(T(Xb).to(dev), T(yb).to(dev))
        behind = model.optim._since
        buf = io.BytesIO()
        torch.save(model, buf)                           # pickles the optimizer too: flushes
        buf.seek(0)
        twin = torch.load(buf, weights_only=False)
        saved = {k: v.clone() for k, v in twin.state_dict().items()}
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        model.train()
        model.train_on_batch(T(X[:256]).to(dev), T(y[:256]).to(dev))
        # one user-driven step: ordinary dense gradients
        model.optim.zero_grad()
        out = model(T(X[:64]).to(dev))
        torch.nn.functional.binary_cross_entropy(out.squeeze(), T(y[:64]).to(dev).squeeze(), reduction="sum").backward()
        model.optim.step()
        sd2 = {k: v.clone() for k, v in model.state_dict().items()}
        return model, hist.history, saved, sd, sd2, behind

    m_d, h_d, sv_d, sd_d, sd2_d, _ = run(False)
    m_l, h_l, sv_l, sd_l, sd2_l, behind = run(True)
    assert m_l.optim.path_counts["scan"] >= 2 and behind >= 1 and m_d.optim.path_counts["scan"] == 0
    for k in h_d:
        np.testing.assert_allclose(h_l[k], h_d[k], rtol=2e-6, atol=1e-9, err_msg=k)
    for k in sd_d:
        assert torch.equal(sv_d[k], sv_l[k]), "torch.save(model): " + k
        assert torch.equal(sd_d[k], sd_l[k]), k
        assert torch.equal(sd2_d[k], sd2_l[k]), "after a user-driven step: " + k


@pytest.mark.parametrize("kind", KINDS)
def test_auto_picks_the_update_by_table_size(kind, monkeypatch):
    """`deferred="auto"`, the default: tables of at least optim.OPT_DEFER_MIN_NUMEL parameters in total get the deferred
    update, smaller ones the dense sweep.  Same bits both ways."""
    _needs_default_env('arena')
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import optim
    dev = _dev()
    seen, sds = {}, {}
    for name, floor in (("deferred", 1000), ("sweep", 1 << 40)):
        monkeypatch.setattr(optim, "OPT_DEFER_MIN_NUMEL", floor)
        model, _ = _big_vocab_model(dev, kind, "auto", False)
        for s in range(7):
            X, y = orc.synthetic_batch(256, VOCAB, ND, seed=700 + s)
            model.train_on_batch(T(X).to(dev), T(y).to(dev))
        seen[name] = (model.optim.__dict__.get("_def") is not None, model.optim.path_counts["scan"] > 0)
        sds[name] = ({k: v.clone() for k, v in model.state_dict().items()}, _opt_state(model))
    assert seen == {"deferred": (True, True), "sweep": (False, False)}, seen
    for k in sds["sweep"][0]:
        assert torch.equal(sds["sweep"][0][k], sds["deferred"][0][k]), k
    _same_state(sds["sweep"][1], sds["deferred"][1])


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_is_deferred_without_an_l2_term(kind):
    """l2_reg_embedding = l2_reg_linear = 0: the sweep's exact shortcut already skips the untouched chunks of such tables,
    so `deferred=True` defers nothing and gives today's results."""
    _needs_default_env('arena')
    from oracle import xdeepfm_oracle as orc
    dev = _dev()

    def run(deferred):
        model, _ = _big_vocab_model(dev, kind, deferred, False, l2_reg_embedding=0.0, l2_reg_linear=0.0)
        for s in range(8):
            X, y = orc.synthetic_batch(256, VOCAB, ND, seed=600 + s)
            model.train_on_batch(T(X).to(dev), T(y).to(dev))
        return model, {k: v.clone() for k, v in model.state_dict().items()}, _opt_state(model)

    m_d, sd_d, os_d = run(False)
    m_l, sd_l, os_l = run(True)
    assert m_l.optim.path_counts["scan"] == 0 and m_l.optim._def is None
    for k in sd_d:
        assert torch.equal(sd_d[k], sd_l[k]), k
    _same_state(os_d, os_l)


@pytest.mark.parametrize("kind", KINDS)
def test_two_param_groups_stay_deferred_and_bit_identical(kind):
    """Tables in group 0, the DNN in group 1 at its own rate: the second group's step must neither flush the tables nor
    tick their clock.  Bits equal to the dense run's; at most ceil(steps / flush_every) + 1 flushes."""
    _needs_default_env('arena')
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import graphstep
    dev = _dev()
    steps, every = 13, 5

    def run(deferred):
        model, _ = _big_vocab_model(dev, kind, deferred, False)
        dnn = [p for k, p in model.named_parameters() if k.startswith("dnn.")]
        rest = [p for k, p in model.named_parameters() if not k.startswith("dnn.")]
        opt = _cls(kind)([{"params": rest}, {"params": dnn, "lr": 2e-3}], deferred=deferred, flush_every=every)
        model.compile(opt, "binary_crossentropy", metrics=[])
        model.train()
        step = graphstep.GraphedStep(model)
        step.disabled = True
        model.__dict__["_graphed_step"] = step
        flushes = [0]
        real_flush = model.optim.flush

        def counting_flush():
            if model.optim.__dict__.get("_def") is not None and model.optim._since:
                flushes[0] += 1
            return real_flush()
        model.optim.flush = counting_flush
        for s in range(steps):
            X, y = orc.synthetic_batch(256, VOCAB, ND, seed=800 + s)
            model.train_on_batch(T(X).to(dev), T(y).to(dev))
        n_flush = flushes[0]
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        return model, sd, _opt_state(model), n_flush

    m_d, sd_d, os_d, _ = run(False)
    m_l, sd_l, os_l, n_flush = run(True)
    assert len(m_l.optim.param_groups) == 2 and m_l.optim._def is not None and m_d.optim._def is None
    assert m_l.optim.path_counts["scan"] >= steps - 1
    assert n_flush <= -(-steps // every) + 1, "%d steps at flush_every=%d flushed %d times" % (steps, every, n_flush)
    for k in sd_d:
        assert torch.equal(sd_d[k], sd_l[k]), k
    _same_state(os_d, os_l)


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trip_through_the_stock_class(kind):
    """In the middle of a deferred run `optim.state_dict()` goes through torch.optim.SGD / Adagrad and back: it holds no
    trace of the deferral, the rows are current when it is taken, and the run ends with the dense run's bits."""
    _needs_default_env('arena')
    from oracle import xdeepfm_oracle as orc
    dev = _dev()

    def run(deferred):
        model, _ = _big_vocab_model(dev, kind, deferred, False)
        mid = None
        for s in range(14):
            if s == 8:
                behind = model.optim._since
                sd = model.optim.state_dict()
                mid = [p.detach().clone() for p in model.parameters()]      # read without the model's own flush
                params = [p for g in model.optim.param_groups for p in g["params"]]
                stock = torch.optim.SGD(params, lr=0.5) if kind == "sgd" else torch.optim.Adagrad(params, lr=0.5)
                stock.load_state_dict(sd)
                assert stock.param_groups[0]["lr"] == model.optim.param_groups[0]["lr"]
                model.optim.load_state_dict(stock.state_dict())
                assert model.optim._def is None and model.optim._since == 0
            X, y = orc.synthetic_batch(256, VOCAB, ND, seed=900 + s)
            model.train_on_batch(T(X).to(dev), T(y).to(dev))
        return model, mid, {k: v.clone() for k, v in model.state_dict().items()}, _opt_state(model), behind

    m_d, mid_d, sd_d, os_d, _ = run(False)
    m_l, mid_l, sd_l, os_l, behind = run(True)
    assert behind >= 1 and m_l.optim._def is not None and m_l.optim.path_counts["scan"] >= 10
    for a, b in zip(mid_d, mid_l):
        assert torch.equal(a, b)
    for k in sd_d:
        assert torch.equal(sd_d[k], sd_l[k]), k
    _same_state(os_d, os_l)


@pytest.mark.parametrize("kind", KINDS)
def test_deferred_soak_300_replayed_steps_with_the_default_period(kind):
    """300 graph-replayed steps at the default flush period (64) on tables of 100 k rows (most rows are never touched, hot
    rows every step), ragged last batches of an 'epoch' every 50 steps, then bit-equality with the dense sweep."""
    _needs_default_env('graph')
    _needs_default_env('arena')
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    vocab = [100000, 57, 100003, 1000, 9, 31337]

    def run(deferred):
        model, _ = _big_vocab_model(dev, kind, deferred, True, flush_every=64, vocab=vocab, seed=8)
        model.__dict__.pop("_graphed_step", None)
        for s in range(300):
            rows = 100 if s % 50 == 49 else 512
            X, y = orc.synthetic_batch(rows, vocab, ND, seed=9000 + s)
            model.train_on_batch(T(X).to(dev), T(y).to(dev))
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        return model, sd, _opt_state(model)

    m_d, sd_d, os_d = run(False)
    m_l, sd_l, os_l = run(True)
    assert m_l.optim._def is not None and m_l.optim.flush_every == 64
    assert m_l.__dict__["_graphed_step"].replays >= 200 and not m_l.__dict__["_graphed_step"].disabled
    for k in sd_d:
        assert torch.equal(sd_d[k], sd_l[k]), k
    _same_state(os_d, os_l)
