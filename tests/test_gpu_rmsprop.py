"""GPU tests (-m gpu) of the native RMSprop step (K7r / K7rd: csrc/sgd_adagrad.hip, csrc/sgd_adagrad_deferred.hip behind
xdfm_amd.optim.TableRMSprop): the kernel against torch.optim.RMSprop in float64, marked against dense gradients bit for bit,
whole models against goldens produced by the reference with compile("rmsprop"), graph replay, the stock path kept for stock
objects, the deferred update against the sweep bit for bit, the fallbacks and the trainer.

Tolerances are those of tests/test_gpu_optim.py: kernel test parameters rtol 2e-6 / atol 1e-8, accumulator rtol 2e-6 / atol
1e-10, L2 value 1e-5 relative; model tests losses rtol 2e-5, state after three steps rtol 1e-3 / atol 2e-5; graph against
eager losses rtol 2e-5, state rtol 2e-3 / atol 2e-6.

The rate of the kernel test's first variant is 1e-4 (the goldens' and the trainer's), with torch's alpha and eps.  At torch's
default 0.01 RMSprop moves every element by about lr / sqrt(1 - alpha) = 0.1 per step whatever the gradient's size, on weights
of 0.05: an element passes through values of 0.1 .. 0.6, whose half ulp in fp32 (up to 3e-8) is above the atol of 1e-8 that
holds for the elements that end near zero.  No fp32 implementation meets the bars there: stock torch.optim.RMSprop in fp32
against float64 on the CPU, this recipe, misses them in 3471 of 1.6 M elements by up to 43x at lr = 0.01, and uses 0.67 of
them at 1e-3, 0.13 at 1e-4 and 0.33 for the second variant (lr 2e-3, alpha 0.9, eps 1e-6)."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden
from test_gpu_optim import L2, SHAPES, _Source, _dev, _golden_model, _three_steps_by_hand, cin_math, close  # noqa: F401

pytestmark = pytest.mark.gpu
T = torch.from_numpy

VARIANTS = {
    "rmsprop": dict(lr=1e-4),
    "rmsprop_var": dict(lr=2e-3, alpha=0.9, eps=1e-6),
}


def _optim():
    from xdfm_amd import optim
    return optim


def _acc(opt, p):
    st = opt.state.get(p, {})
    return st["square_avg"] if "square_avg" in st else torch.zeros_like(p)


# --------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", sorted(VARIANTS))
def test_kernel_matches_torch_rmsprop_in_float64(kind):
    """Six steps with fresh dense gradients (views of one flat buffer at a 16-byte offset, every 7th element zero), the L2
    term armed on odd steps: parameters and `square_avg` against torch.optim.RMSprop on float64 CPU copies of the same fp32
    values with 2*l2*w added to the gradients by hand; then the state_dict goes into a stock optimizer."""
    dev = _dev()
    kw = VARIANTS[kind]
    torch.manual_seed(3)
    init = [torch.randn(s, device=dev) * 0.05 for s in SHAPES]
    pa = [torch.nn.Parameter(t.clone()) for t in init]
    pb = [torch.nn.Parameter(t.detach().cpu().double()) for t in init]
    oa, ob = _optim().TableRMSprop(pa, **kw), torch.optim.RMSprop(pb, **kw)
    assert isinstance(oa, torch.optim.RMSprop) and oa._native()
    sizes = [p.numel() for p in pa]
    for step in range(6):
        flat = torch.randn(sum(sizes) + 8, device=dev) * (0.1 if step % 2 else 1e-3)
        flat[::7] = 0.0
        host = flat.cpu().double()
        off = 4                                                               # 16-byte aligned start
        for p, q, n in zip(pa, pb, sizes):
            p.grad = flat[off:off + n].view(p.shape)
            q.grad = host[off:off + n].view(p.shape).clone()
            off += n
        if step % 2:
            oa.arm_l2(pa[:3], L2)
            want_value = sum(c * float((q.detach() ** 2).sum()) for q, c in zip(pb[:3], L2))
            for q, c in zip(pb[:3], L2):
                q.grad.add_(q.detach(), alpha=2 * c)
        oa.step()
        ob.step()
        if step % 2:
            got = float(oa.l2_value)
            print("%s step %d: l2 value rel. error %.3g" % (kind, step, abs(got - want_value) / want_value))
            assert abs(got - want_value) <= 1e-5 * want_value
        else:
            assert oa.l2_value is None
    for i, (p, q) in enumerate(zip(pa, pb)):
        want = q.detach().numpy()
        sa, sb = oa.state[p], ob.state[q]
        acc = sb["square_avg"].numpy()
        err = np.abs(p.detach().cpu().numpy().astype(np.float64) - want)
        err_acc = np.abs(sa["square_avg"].cpu().numpy().astype(np.float64) - acc)
        print("%s tensor %d: largest share of the budget: param %.3f, square_avg %.3f" % (
            kind, i, float((err / (1e-8 + 2e-6 * np.abs(want))).max()), float((err_acc / (1e-10 + 2e-6 * np.abs(acc))).max())))
        assert sorted(sa.keys()) == sorted(sb.keys()) == ["square_avg", "step"]
        assert float(sa["step"]) == float(sb["step"]) == 6.0 and sa["step"].dtype == torch.float32 and not sa["step"].is_cuda
    for i, (p, q) in enumerate(zip(pa, pb)):
        close(p, q.detach().numpy(), rtol=2e-6, atol=1e-8, msg="param %d" % i)
        close(oa.state[p]["square_avg"], ob.state[q]["square_avg"].numpy(), rtol=2e-6, atol=1e-10, msg="square_avg %d" % i)
    # state_dict round trip into a stock optimizer of fp32 GPU parameters
    oc = torch.optim.RMSprop([torch.nn.Parameter(t.clone()) for t in init], **kw)
    oc.load_state_dict(oa.state_dict())
    for p, q in zip(pa, oc.param_groups[0]["params"]):
        assert sorted(oc.state[q].keys()) == sorted(oa.state[p].keys())
        assert torch.equal(oc.state[q]["square_avg"], oa.state[p]["square_avg"]) and float(oc.state[q]["step"]) == 6.0


# --------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kind", sorted(VARIANTS))
def test_marked_gradients_give_the_bits_of_dense_gradients(kind):
    """The same steps with row-sparse gradients kept in an ops.GradArena (read by their marks) and as plain dense tensors:
    identical parameters and accumulators; the arena is all zeros and not pending after every step; in the tensor without an
    L2 term the rows without a gradient keep their parameter bits while their `square_avg` becomes alpha * v, exactly."""
    from xdfm_amd import ops
    dev = _dev()
    kw = VARIANTS[kind]
    alpha = kw.get("alpha", 0.99)
    torch.manual_seed(3)
    init = [torch.randn(s, device=dev) * 0.05 for s in SHAPES]
    pa = [torch.nn.Parameter(t.clone()) for t in init]
    pb = [torch.nn.Parameter(t.clone()) for t in init]
    oa, ob = _optim().TableRMSprop(pa, **kw), _optim().TableRMSprop(pb, **kw)
    sizes = [p.numel() for p in pa]
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4
    arena = ops.GradArena(off, dev)
    oa.grad_sources.append(_Source(arena))
    gen = torch.Generator(device="cpu").manual_seed(17)
    for step in range(6):
        dense = []
        for p in pa:
            hit = torch.rand(p.shape[0], generator=gen) < 0.03                 # the rows a batch touches
            g = torch.randn(p.shape, generator=gen) * (0.1 if step % 2 else 1e-3)
            g[~hit] = 0.0
            dense.append(g.to(dev))
        views = []
        for p, q, g, o, n in zip(pa, pb, dense, offs, sizes):
            arena.flat[o:o + n].copy_(g.reshape(-1))
            views.append(arena.flat[o:o + n].view(p.shape))
            p.grad = views[-1]
            q.grad = g.clone()
        arena.marks[:off // 4].copy_((arena.flat.view(-1, 4) != 0).any(1).to(torch.uint8))
        arena.hand_out(views)
        assert arena.pending
        before = pa[1].detach().clone()
        acc_before = _acc(oa, pa[1]).clone()
        if step % 2:
            oa.arm_l2(pa[:3], L2)
            ob.arm_l2(pb[:3], L2)
        oa.step()
        ob.step()
        assert oa._native() and ob._native()
        if step % 2:
            assert float(oa.l2_value) == float(ob.l2_value)
        assert not arena.pending and float(arena.flat.abs().max()) == 0.0 and int(arena.marks.max()) == 0
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert torch.equal(p, q), "step %d param %d: %d elements differ" % (step, i, int((p != q).sum()))
            assert torch.equal(_acc(oa, p), _acc(ob, q)), "step %d square_avg %d" % (step, i)
        # tensor 1 never has an L2 term: rows without a gradient keep p's bits; the accumulator still decays
        idle = (dense[1].reshape(-1) == 0)
        assert bool(idle.any()) and bool((~idle).any())
        assert torch.equal(pa[1].detach().reshape(-1)[idle].view(torch.int32), before.reshape(-1)[idle].view(torch.int32))
        assert bool((pa[1].detach().reshape(-1)[~idle] != before.reshape(-1)[~idle]).any())
        decayed = acc_before.reshape(-1) * alpha
        assert torch.equal(_acc(oa, pa[1]).reshape(-1)[idle], decayed[idle])
        if step > 0:
            assert bool((acc_before.reshape(-1)[idle] > 0).any())


# --------------------------------------------------------------------------------------------- 3
def _share(model, g):
    worst = 0.0
    for k, v in model.state_dict().items():
        want = g["s3:" + k]
        if want.size:
            worst = max(worst, float((np.abs(v.detach().cpu().numpy() - want) / (2e-5 + 1e-3 * np.abs(want))).max()))
    return worst


def _rms_model(name, dev, optimizer="rmsprop"):
    """_golden_model, then the recorded rate on every param group, as the generator and the trainer set it"""
    model, g, X, y, B = _golden_model(name, dev, optimizer)
    for pg in model.optim.param_groups:
        pg["lr"] = float(g["lr"])
    return model, g, X, y, B


@pytest.mark.parametrize("path", ["loop", "own_step"])
@pytest.mark.parametrize("name", golden_names("rms_"))
def test_model_vs_reference_golden_with_rmsprop(name, path, cin_math):
    """Three steps as BaseModel.fit does them against the reference's run with compile("rmsprop") and lr = 1e-4: `loop`
    drives autograd by hand (dense gradients, L2 term through K6), `own_step` is train_on_batch (marked gradients, the L2
    term inside the sweep, the third step replayed from a graph).  Every element, the bars of the model golden tests."""
    dev = _dev()
    model, g, X, y, B = _golden_model(name, dev, "rmsprop")
    assert type(model.optim).__name__ == "TableRMSprop"
    assert str(g["optim_class"]) in [c.__name__ for c in type(model.optim).__mro__]
    grp = model.optim.param_groups[0]
    assert (grp["lr"], grp["alpha"], grp["eps"]) == (float(g["lr0"]), float(g["alpha"]), float(g["eps"]))
    for pg in model.optim.param_groups:
        pg["lr"] = float(g["lr"])
    if path == "loop":
        losses = _three_steps_by_hand(model, X, y, B)
    else:
        losses = []
        for s in range(3):
            _, l, tot = model.train_on_batch(X[s * B:(s + 1) * B], y[s * B:(s + 1) * B])
            losses.append([float(l.reshape(-1)[0]), float(tot.reshape(-1)[0])])
    print("%s %s %s: worst share of the bar %.4f, losses rel. %.3g" % (
        name, path, "f16x3" if cin_math else "f32mfma", _share(model, g),
        float(np.abs(np.array(losses) / g["losses3"] - 1).max())))
    np.testing.assert_allclose(np.array(losses), g["losses3"], rtol=2e-5)
    for k, v in model.state_dict().items():
        close(v, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="after 3 steps: " + k)
    assert {float(st["step"]) for st in model.optim.state.values()} == {3.0}


# --------------------------------------------------------------------------------------------- 4
LR0 = 1e-4


def _small_model(dev, optimizer="rmsprop"):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev)
    model.compile(optimizer, "binary_crossentropy", metrics=[])
    for pg in model.optim.param_groups:
        pg["lr"] = LR0
    model.train()
    return model, vocab, nd


def test_compile_string_takes_the_native_path_and_replays_from_a_graph():
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import graphstep
    dev = _dev()
    model, vocab, nd = _small_model(dev)
    assert type(model.optim).__name__ == "TableRMSprop" and model._optim_capturable and model._l2_fusion() is not None
    if os.environ.get("XDFM_HIP_GRAPH", "1") == "0":
        pytest.skip("XDFM_HIP_GRAPH=0")

    def run(use_graph, change=True):
        model, _, _ = _small_model(dev)
        step = graphstep.GraphedStep(model)
        step.disabled = not use_graph
        model.__dict__["_graphed_step"] = step
        losses, entries = [], []
        for s in range(8):
            if s == 5 and change:
                for pg in model.optim.param_groups:
                    pg["lr"] = 3 * LR0
            X, y = orc.synthetic_batch(256, vocab, nd, seed=100 + s)
            xb, yb = T(X).to(dev), T(y).to(dev)
            out = model.train_on_batch(xb, yb) if use_graph else model._train_step_eager(xb, yb)
            losses.append(float(out[2].detach().reshape(-1)[0]))
            entries.append(len([e for e in step.entries.values() if e.graph is not None]))
        return model, step, losses, entries

    m_g, step_g, l_g, entries = run(True)
    m_e, step_e, l_e, _ = run(False)
    assert step_g.replays > 0 and not step_g.disabled and step_e.replays == 0
    assert step_g.replays >= 5, step_g.replays                    # two eager steps, then the steps come from the graph
    assert entries[4] == entries[7] == 1                          # the new rate is followed by the SAME graph
    for e in step_g.entries.values():
        if e.graph is not None:
            n, n_memset, n_other = graphstep.census(e.graph)
            assert n > 20 and n_memset == 0 and n_other == 0
    np.testing.assert_allclose(l_g, l_e, rtol=2e-5)
    for (k, a), (_, b) in zip(m_g.state_dict().items(), m_e.state_dict().items()):
        close(a, b.cpu().numpy(), rtol=2e-3, atol=2e-6, msg=k)
    # the rate change took effect: a run that keeps the old rate ends elsewhere
    m_k, _, _, _ = run(False, change=False)
    moved = max(float((a - b).abs().max()) for a, b in zip(m_g.state_dict().values(), m_k.state_dict().values()))
    assert moved > 1e-5
    for m in (m_g, m_e):
        assert type(m.optim).__name__ == "TableRMSprop" and m.optim._native()
        steps = {float(st["step"]) for st in m.optim.state.values()}
        assert steps == {8.0}, steps
        assert all(sorted(st.keys()) == ["square_avg", "step"] for st in m.optim.state.values())
    for a in m_g._plan.arenas():
        assert not a.pending and float(a.flat.abs().max()) == 0.0 and int(a.marks.max()) == 0


# --------------------------------------------------------------------------------------------- 5
def test_stock_optimizer_object_keeps_the_stock_path(cin_math):
    dev = _dev()
    name = "rms_sum_c1"
    native, g, X, y, B = _rms_model(name, dev)
    stock_model, _, _, _, _ = _golden_model(name, dev, "rmsprop")
    stock = torch.optim.RMSprop(stock_model.parameters(), lr=float(g["lr"]))
    stock_model.compile(stock, "binary_crossentropy", metrics=[])
    assert stock_model.optim is stock and not stock_model._optim_capturable and stock_model._l2_fusion() is None
    assert native._optim_capturable and type(native.optim).__name__ == "TableRMSprop"
    l_n, l_s = [], []
    for s in range(3):
        xb, yb = X[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        l_n.append(float(native.train_on_batch(xb, yb)[2].reshape(-1)[0]))
        l_s.append(float(stock_model.train_on_batch(xb, yb)[2].reshape(-1)[0]))
    assert stock_model.__dict__["_graphed_step"].replays == 0
    print("rms_sum_c1 %s: worst share of the bar: native %.4f, stock object %.4f" % (
        "f16x3" if cin_math else "f32mfma", _share(native, g), _share(stock_model, g)))
    np.testing.assert_allclose(l_n, l_s, rtol=2e-5)
    np.testing.assert_allclose(l_s, g["losses3"][:, 1], rtol=2e-5)
    for (k, a), (_, b) in zip(native.state_dict().items(), stock_model.state_dict().items()):
        close(a, b.cpu().numpy(), rtol=1e-3, atol=2e-5, msg=k)
        close(b, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="stock path, after 3 steps: " + k)


# --------------------------------------------------------------------------------------------- 6
ND, D = 3, 16
VOCAB = [5000, 31, 20003, 3, 9, 402]     # 20003 % 4 != 0: tail rows the sweep always updates; 3 rows: a table that is all tail


def _needs_default_env(feature):
    env = {"arena": "XDFM_GRAD_ARENA", "graph": "XDFM_HIP_GRAPH"}[feature]
    if os.environ.get(env, "1") == "0":
        pytest.skip("%s=0" % env)


def _big_vocab_model(dev, deferred, use_graph, flush_every=5, emb_dim=D):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    cols = [SparseFeat("C%d" % (i + 1), v, emb_dim) for i, v in enumerate(VOCAB)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(ND)]
    torch.manual_seed(4)
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev)
    with torch.no_grad():                           # weights large enough for the L2 pull to move bits every step
        for k, p in model.named_parameters():
            if "embedding_dict" in k:
                p.mul_(2000.0)
    model.compile("rmsprop", "binary_crossentropy", metrics=[])
    assert type(model.optim) is _optim().TableRMSprop
    for pg in model.optim.param_groups:
        pg["lr"] = 1e-3
    model.optim.deferred = deferred
    model.optim.flush_every = flush_every
    model.train()
    step = graphstep.GraphedStep(model)
    step.disabled = not use_graph
    model.__dict__["_graphed_step"] = step
    return model, step


def _snapshot(model):
    """parameters and every `square_avg`, read without the model's own flush"""
    out = [p.detach().clone() for p in model.parameters()]
    out += [model.optim.state[p]["square_avg"].clone() for g in model.optim.param_groups for p in g["params"]]
    return out


def _run_deferral(dev, deferred, use_graph, emb_dim):
    from oracle import xdeepfm_oracle as orc
    model, step = _big_vocab_model(dev, deferred, use_graph, emb_dim=emb_dim)
    flushes, real_flush = [], model.optim.flush

    def counting_flush():
        if model.optim.__dict__.get("_def") is not None and model.optim._since:
            flushes.append(now[0])
        return real_flush()
    model.optim.flush = counting_flush
    now, total, snaps, behind = [0], 0.0, [], {}
    for s in range(31):
        now[0] = s
        if s in (7, 13, 18):          # mid-period; behind a flush boundary (steps 5 and 10 flushed); after the rate change
            behind[s] = model.optim._since
            model.optim.flush()
            snaps.append(_snapshot(model))
        if s == 9:
            for g in model.optim.param_groups:
                g["lr"] = 3e-3
        if s == 16:                   # state_dict() / load_state_dict() through the stock class
            behind[s] = model.optim._since
            sd = model.optim.state_dict()
            snaps.append(_snapshot(model))
            params = [p for g in model.optim.param_groups for p in g["params"]]
            stock = torch.optim.RMSprop(params, lr=0.5)
            stock.load_state_dict(sd)
            assert stock.param_groups[0]["lr"] == model.optim.param_groups[0]["lr"]
            model.optim.load_state_dict(stock.state_dict())
            assert model.optim._def is None and model.optim._since == 0
        if s == 24:                   # alpha and eps change with rows behind: the owed steps are replayed with the OLD ones
            behind[s] = model.optim._since
            for g in model.optim.param_groups:
                g["alpha"], g["eps"] = 0.9, 1e-6
        X, y = orc.synthetic_batch(256, VOCAB, ND, seed=500 + s)
        out = model.train_on_batch(T(X).to(dev), T(y).to(dev))
        total += float(out[2])
        if s == 24:
            behind["after"] = model.optim._since
    model.optim.flush()
    total += model.optim.take_backlog()
    snaps.append(_snapshot(model))
    steps = {float(st["step"]) for st in model.optim.state.values()}
    return model, step, snaps, total, behind, flushes, steps


@pytest.mark.parametrize("use_graph,emb_dim", [(False, D), (True, D), (True, 10)], ids=["eager", "graph", "graph-D10"])
def test_deferred_update_is_bit_identical_to_the_sweep(use_graph, emb_dim):
    """31 steps, flush_every = 5, cold and hot rows: parameters and every `square_avg` equal the sweep's BIT FOR BIT after a
    flush in the middle of a period, behind flush boundaries, after a rate change, after a state_dict() / load_state_dict()
    round trip through torch.optim.RMSprop, and at the end, after alpha and eps changed with rows behind (which flushes
    first).  The epoch loss with the backlog agrees to 2e-6 relative.  Eager launches, graph replay, D = 10."""
    _needs_default_env("arena")
    if use_graph:
        _needs_default_env("graph")
    dev = _dev()
    m_d, st_d, sn_d, tot_d, _, fl_d, steps_d = _run_deferral(dev, False, use_graph, emb_dim)
    m_l, st_l, sn_l, tot_l, behind, fl_l, steps_l = _run_deferral(dev, True, use_graph, emb_dim)
    assert m_l.optim._def is not None and m_d.optim._def is None and not fl_d
    # path_counts counts the deferred steps whose Python ran (issued eagerly or captured); a replay runs no Python.  Every one
    # of the 31 steps is one or the other (a capturing step is both), so together they cover the run.
    scan = m_l.optim.path_counts["scan"]
    assert m_d.optim.path_counts["scan"] == 0
    assert (scan + st_l.replays >= 31 and scan >= 2) if use_graph else scan == 31, (scan, st_l.replays)
    assert len(m_l.optim._def["tensors"]) == 12           # 6 embedding + 6 linear tables
    assert all(behind[s] >= 1 for s in (7, 13, 18, 16, 24)), behind
    assert 24 in fl_l and behind["after"] == 1, (fl_l, behind)      # the change of alpha / eps flushed before that step
    if use_graph:
        assert st_l.replays >= 12 and not st_l.disabled and st_d.replays >= 12 and not st_d.disabled
    assert len(sn_d) == len(sn_l) == 5
    for n, (a, b) in enumerate(zip(sn_d, sn_l)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), "snapshot %d tensor %d: %d elements differ" % (n, i, int((x != y).sum()))
    assert steps_d == steps_l == {31.0}
    print("epoch loss rmsprop graph=%s D=%d: sweep %.9g deferred %.9g rel %.3g" % (use_graph, emb_dim, tot_d, tot_l,
                                                                                 abs(tot_d - tot_l) / abs(tot_d)))
    assert np.isfinite(tot_d) and abs(tot_d - tot_l) <= 2e-6 * abs(tot_d), (tot_d, tot_l)


def test_a_second_param_group_that_owns_the_tables_keeps_the_sweep():
    _needs_default_env("arena")
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    model, _ = _big_vocab_model(dev, True, False)
    dnn = [p for k, p in model.named_parameters() if k.startswith("dnn.")]
    rest = [p for k, p in model.named_parameters() if not k.startswith("dnn.")]
    opt = _optim().TableRMSprop([{"params": dnn}, {"params": rest, "lr": 1e-3}], lr=1e-3, deferred=True, flush_every=5)
    model.compile(opt, "binary_crossentropy", metrics=[])
    model.train()
    for s in range(6):
        X, y = orc.synthetic_batch(256, VOCAB, ND, seed=800 + s)
        model.train_on_batch(T(X).to(dev), T(y).to(dev))
    assert model.optim is opt and opt._native() and opt._def is None and opt.path_counts["scan"] == 0


# --------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("extra", [dict(momentum=0.9), dict(centered=True)], ids=["momentum", "centered"])
def test_fallbacks_run_the_stock_step(extra):
    dev = _dev()
    torch.manual_seed(5)
    init = [torch.randn(s, device=dev) * 0.05 for s in [(3001, 16), (513,), (11,)]]
    pa = [torch.nn.Parameter(t.clone()) for t in init]
    pb = [torch.nn.Parameter(t.clone()) for t in init]
    oa, ob = _optim().TableRMSprop(pa, lr=1e-3, **extra), torch.optim.RMSprop(pb, lr=1e-3, **extra)
    plain = _optim().TableRMSprop([torch.nn.Parameter(init[0].clone())], lr=1e-3)
    assert plain._native() and not oa._native()
    for step in range(4):
        for p, q in zip(pa, pb):
            p.grad = torch.randn_like(p) * 0.1
            q.grad = p.grad.clone()
        if step == 2:
            oa.arm_l2(pa[:1], [0.05])
            want = 0.05 * float(pb[0].detach().double().square().sum())
            pb[0].grad.add_(pb[0].detach(), alpha=0.1)
        oa.step()
        ob.step()
        if step == 2:
            assert abs(float(oa.l2_value) - want) <= 1e-5 * want
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)
        assert sorted(oa.state[p].keys()) == sorted(ob.state[q].keys())
        for k in ob.state[q]:
            assert torch.equal(oa.state[p][k], ob.state[q][k]), k
        assert ("momentum_buffer" in oa.state[p]) == ("momentum" in extra) and ("grad_avg" in oa.state[p]) == ("centered" in extra)


# --------------------------------------------------------------------------------------------- 8
def test_trainer_runs_end_to_end_with_rmsprop(tmp_path):
    import importlib.util
    import json
    from conftest import PKG
    _dev()
    spec = importlib.util.spec_from_file_location("xdftrain_amd", os.path.join(PKG, "xdftrain_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / "out")
    mod.main(["--model", "xdeepfm", "--mode", "final", "--cin_layer_size", "16,8", "--dnn_hidden_units", "32,16",
              "--optimizer", "rmsprop", "--synthetic", "6000", "--epochs", "3", "--batch_size", "512", "--embedding_dim", "8",
              "--out_dir", out, "--verbose", "0", "--learning_rate", "0.0001"])
    for f in ("xdeepfm_full_weights.pth", "history_full.json", "preprocess.json"):
        assert os.path.exists(os.path.join(out, f)), f
    hist = json.load(open(os.path.join(out, "history_full.json")))
    assert len(hist["loss"]) == 3 and np.all(np.isfinite(hist["loss"])) and hist["loss"][-1] < hist["loss"][0]
