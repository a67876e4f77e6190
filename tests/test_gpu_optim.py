"""GPU tests (-m gpu) of the native SGD and Adagrad steps (K7s / K7g: csrc/sgd_adagrad.hip behind
xdfm_amd.optim.TableSGD / TableAdagrad): the kernels against torch's optimizers in float64, marked against dense
gradients bit for bit, whole models against goldens produced by the reference with compile("sgd") / compile("adagrad"),
and the plumbing -- graph replay, fused L2 term, learning rate from device memory, the stock path kept for stock objects.

Tolerances: the kernel test uses those of test_table_adam_kernel_matches_torch_adam (parameters rtol 2e-6 / atol 1e-8,
accumulator rtol 2e-6 / atol 1e-10, L2 value 1e-5 relative; stock fp32 torch against float64 uses at most half of that on
these inputs); the model tests use those of test_model_vs_reference_golden (losses rtol 2e-5, state after three steps
rtol 1e-3 / atol 2e-5) and of the graph-vs-eager test (losses rtol 2e-5, state rtol 2e-3 / atol 2e-6)."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy

SHAPES = [(70001, 16), (100000, 1), (65536, 3), (300, 7), (11,)]          # three large (one odd-sized), two small
L2 = [1e-3, 0.0, 5e-2]
KINDS = {
    "sgd": (lambda ps: _optim().TableSGD(ps, lr=0.01), lambda ps: torch.optim.SGD(ps, lr=0.01)),
    "adagrad": (lambda ps: _optim().TableAdagrad(ps), lambda ps: torch.optim.Adagrad(ps)),
    "adagrad_acc": (lambda ps: _optim().TableAdagrad(ps, lr=2e-3, initial_accumulator_value=0.1),
                    lambda ps: torch.optim.Adagrad(ps, lr=2e-3, initial_accumulator_value=0.1)),
}


def _optim():
    from xdfm_amd import optim
    return optim


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close(got, want, rtol, atol, msg=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


@pytest.fixture(params=[0, 1], ids=["f32mfma", "f16x3"])
def cin_math(request):
    from xdfm_amd import _lib
    old = _lib.get_option("cin_math")
    _lib.set_option("cin_math", request.param)
    yield request.param
    _lib.set_option("cin_math", old)


# --------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_kernel_matches_torch_optimizer_in_float64(kind):
    """Six steps with fresh dense gradients (views of one flat buffer at a 16-byte offset, every 7th element zero), the
    L2 term armed on odd steps: parameters and accumulators against torch.optim.SGD / Adagrad on float64 CPU copies of
    the same fp32 values with 2*l2*w added to the gradients by hand."""
    dev = _dev()
    make, stock = KINDS[kind]
    torch.manual_seed(3)
    init = [torch.randn(s, device=dev) * 0.05 for s in SHAPES]
    pa = [torch.nn.Parameter(t.clone()) for t in init]
    pb = [torch.nn.Parameter(t.detach().cpu().double()) for t in init]
    oa, ob = make(pa), stock(pb)
    assert isinstance(oa, type(ob))
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
        err = np.abs(p.detach().cpu().numpy().astype(np.float64) - want)
        print("%s param %d: largest share of the budget %.3f" % (kind, i, float((err / (1e-8 + 2e-6 * np.abs(want))).max())))
        close(p, want, rtol=2e-6, atol=1e-8, msg="param %d" % i)
        sa, sb = oa.state[p], ob.state[q]
        assert sorted(sa.keys()) == sorted(sb.keys())
        if "sum" in sb:
            assert float(sa["step"]) == float(sb["step"]) == 6.0
            close(sa["sum"], sb["sum"].numpy(), rtol=2e-6, atol=1e-10, msg="sum %d" % i)
    # state_dict round trip into a stock optimizer of fp32 GPU parameters
    oc = stock([torch.nn.Parameter(t.clone()) for t in init])
    oc.load_state_dict(oa.state_dict())
    for p, q in zip(pa, oc.param_groups[0]["params"]):
        assert sorted(oc.state[q].keys()) == sorted(oa.state[p].keys())
        if "sum" in oc.state[q]:
            assert torch.equal(oc.state[q]["sum"], oa.state[p]["sum"]) and float(oc.state[q]["step"]) == 6.0


# --------------------------------------------------------------------------------------------- 2
class _Source(object):
    def __init__(self, arena):
        self._arena = arena

    def arenas(self):
        return [self._arena]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_marked_gradients_give_the_bits_of_dense_gradients(kind):
    """The same steps with row-sparse gradients kept in an ops.GradArena (read by their marks) and as plain dense
    tensors: identical parameters and accumulators; the arena is all zeros and not pending after every step; the unmarked
    rows of a tensor without an L2 term keep their bits."""
    from xdfm_amd import ops
    dev = _dev()
    make, _ = KINDS[kind]
    torch.manual_seed(3)
    init = [torch.randn(s, device=dev) * 0.05 for s in SHAPES]
    pa = [torch.nn.Parameter(t.clone()) for t in init]
    pb = [torch.nn.Parameter(t.clone()) for t in init]
    oa, ob = make(pa), make(pb)
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
            rows = p.shape[0]
            hit = torch.rand(rows, generator=gen) < 0.03                       # the rows a batch touches
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
        acc_before = oa.state[pa[1]]["sum"].clone() if "sum" in oa.state[pa[1]] else None
        if step % 2:
            oa.arm_l2(pa[:3], L2)
            ob.arm_l2(pb[:3], L2)
        oa.step()
        ob.step()
        if step % 2:
            assert float(oa.l2_value) == float(ob.l2_value)
        assert not arena.pending and float(arena.flat.abs().max()) == 0.0 and int(arena.marks.max()) == 0
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert torch.equal(p, q), "step %d param %d: %d elements differ" % (step, i, int((p != q).sum()))
            if "sum" in oa.state[p]:
                assert torch.equal(oa.state[p]["sum"], ob.state[q]["sum"]), "step %d sum %d" % (step, i)
        # tensor 1 never has an L2 term: rows without a gradient are not touched (nor is their accumulator)
        idle = (dense[1].reshape(-1) == 0)
        assert bool(idle.any()) and bool((~idle).any())
        assert torch.equal(pa[1].detach().reshape(-1)[idle], before.reshape(-1)[idle])
        assert bool((pa[1].detach().reshape(-1)[~idle] != before.reshape(-1)[~idle]).any())
        if acc_before is not None:
            assert torch.equal(oa.state[pa[1]]["sum"].reshape(-1)[idle], acc_before.reshape(-1)[idle])


# --------------------------------------------------------------------------------------------- 3
def _build_model(g, dev):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr import models
    vocab = [int(v) for v in g["vocab"]]
    nd, D = int(g["n_dense"]), int(g["emb_dim"])
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    kw = dict(zip([str(k) for k in g["kw_keys"]], [int(v) for v in g["kw_vals"]]))
    cls = getattr(models, str(g["cls"]))
    return cls(cols, cols, dnn_hidden_units=tuple(int(v) for v in g["dnn"]),
               cin_layer_size=tuple(int(v) for v in g["cin"]), l2_reg_dnn=1e-5, device=dev, **kw)


def _golden_model(name, dev, optimizer):
    """(model at the golden's starting weights, compiled; golden; X; y; B).  The starting weights and the batches are
    those of the model_<case> golden the optim_ golden names as its base."""
    g = load_golden(name)
    base = load_golden(str(g["base"]))
    model = _build_model(g, dev)
    model.load_state_dict({k[3:]: T(v) for k, v in base.items() if k.startswith("s0:")}, strict=True)
    model.compile(optimizer, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    model.train()
    return model, g, T(base["X"]).to(dev), T(base["y"]).to(dev), int(g["B"])


def _three_steps_by_hand(model, X, y, B):
    losses = []
    for s in range(3):
        xb, yb = X[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        yp = model(xb).squeeze()
        model.optim.zero_grad()
        l = torch.nn.functional.binary_cross_entropy(yp, yb.squeeze(), reduction="sum")
        tot = l + model.get_regularization_loss() + model.aux_loss
        losses.append([l.item(), tot.item()])
        tot.backward()
        model.optim.step()
    return losses


def test_optimizer_goldens_cover_both_optimizers_and_three_model_shapes():
    names = golden_names("optim_")
    for opt in ("sgd", "adagrad"):
        for case in ("sum_small", "sum_c1", "x3_cin"):
            assert "optim_%s_%s" % (opt, case) in names


@pytest.mark.parametrize("path", ["loop", "own_step"])
@pytest.mark.parametrize("name", golden_names("optim_"))
def test_model_vs_reference_golden_with_sgd_and_adagrad(name, path, cin_math):
    """Three steps as BaseModel.fit does them (basemodel.py:241-262) against the reference's run with the same optimizer
    string: `loop` drives autograd by hand (dense gradients, L2 term through K6), `own_step` is train_on_batch (marked
    gradients, the L2 term inside the sweep, the third step replayed from a graph)."""
    dev = _dev()
    optimizer = str(load_golden(name)["optimizer"])
    model, g, X, y, B = _golden_model(name, dev, optimizer)
    assert type(model.optim).__name__ == {"sgd": "TableSGD", "adagrad": "TableAdagrad"}[optimizer]
    assert str(g["optim_class"]) in [c.__name__ for c in type(model.optim).__mro__]
    assert model.optim.param_groups[0]["lr"] == float(g["lr"])
    if path == "loop":
        losses = _three_steps_by_hand(model, X, y, B)
    else:
        losses = []
        for s in range(3):
            _, l, tot = model.train_on_batch(X[s * B:(s + 1) * B], y[s * B:(s + 1) * B])
            losses.append([float(l.reshape(-1)[0]), float(tot.reshape(-1)[0])])
    np.testing.assert_allclose(np.array(losses), g["losses3"], rtol=2e-5)
    for k, v in model.state_dict().items():
        close(v, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="after 3 steps: " + k)


# --------------------------------------------------------------------------------------------- 4
# rates for the small model's own-step runs, set right after compile as the trainer does (xdftrain_amd.py): the loss is
# a SUM over 256 rows, so the reference's 0.01 would make SGD's trajectory diverge and the comparison ill-conditioned
LR0 = {"sgd": 1e-4, "adagrad": 1e-3}


def _small_model(dev, optimizer):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev)
    model.compile(optimizer, "binary_crossentropy", metrics=[])
    for pg in model.optim.param_groups:
        pg["lr"] = LR0[optimizer]
    model.train()
    return model, vocab, nd


@pytest.mark.parametrize("optimizer,cls_name", [("sgd", "TableSGD"), ("adagrad", "TableAdagrad")])
def test_compile_string_takes_the_native_path_and_replays_from_a_graph(optimizer, cls_name):
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import graphstep
    dev = _dev()
    model, vocab, nd = _small_model(dev, optimizer)
    assert type(model.optim).__name__ == cls_name and model._optim_capturable and model._l2_fusion() is not None
    if os.environ.get("XDFM_HIP_GRAPH", "1") == "0":
        pytest.skip("XDFM_HIP_GRAPH=0")

    def run(use_graph):
        model, _, _ = _small_model(dev, optimizer)
        step = graphstep.GraphedStep(model)
        step.disabled = not use_graph
        model.__dict__["_graphed_step"] = step
        losses, entries = [], []
        for s in range(8):
            if s == 5:
                for pg in model.optim.param_groups:
                    pg["lr"] = 3 * LR0[optimizer]
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
    moved = max(float((a - b).abs().max()) for a, b in zip(m_g.state_dict().values(), _keep_rate(dev, optimizer, vocab, nd)))
    assert moved > 1e-5
    if optimizer == "adagrad":
        for m in (m_g, m_e):
            steps = {float(st["step"]) for st in m.optim.state.values()}
            assert steps == {8.0}, steps
    for a in m_g._plan.arenas():
        assert not a.pending and float(a.flat.abs().max()) == 0.0 and int(a.marks.max()) == 0


def _keep_rate(dev, optimizer, vocab, nd):
    from oracle import xdeepfm_oracle as orc
    model, _, _ = _small_model(dev, optimizer)
    for s in range(8):
        X, y = orc.synthetic_batch(256, vocab, nd, seed=100 + s)
        model._train_step_eager(T(X).to(dev), T(y).to(dev))
    return list(model.state_dict().values())


# --------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_stock_optimizer_object_keeps_the_stock_path(optimizer, cin_math):
    dev = _dev()
    name = "optim_%s_sum_c1" % optimizer
    native, g, X, y, B = _golden_model(name, dev, optimizer)
    stock_model, _, _, _, _ = _golden_model(name, dev, optimizer)
    stock = torch.optim.SGD(stock_model.parameters(), lr=0.01) if optimizer == "sgd" else torch.optim.Adagrad(stock_model.parameters())
    stock_model.compile(stock, "binary_crossentropy", metrics=[])
    assert stock_model.optim is stock and not stock_model._optim_capturable and stock_model._l2_fusion() is None
    assert native._optim_capturable
    l_n, l_s = [], []
    for s in range(3):
        xb, yb = X[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        l_n.append(float(native.train_on_batch(xb, yb)[2].reshape(-1)[0]))
        l_s.append(float(stock_model.train_on_batch(xb, yb)[2].reshape(-1)[0]))
    assert stock_model.__dict__["_graphed_step"].replays == 0
    np.testing.assert_allclose(l_n, l_s, rtol=2e-5)
    np.testing.assert_allclose(l_s, g["losses3"][:, 1], rtol=2e-5)
    for (k, a), (_, b) in zip(native.state_dict().items(), stock_model.state_dict().items()):
        close(a, b.cpu().numpy(), rtol=1e-3, atol=2e-5, msg=k)
        close(b, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="stock path, after 3 steps: " + k)


# --------------------------------------------------------------------------------------------- 6
def test_fit_with_adagrad_returns_the_history_of_the_adam_run():
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    dev = _dev()
    g = load_golden("fit_history")
    vocab, nd, D = [int(v) for v in g["vocab"]], int(g["n_dense"]), int(g["emb_dim"])
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    X, y, Xv, yv = g["X"], g["y"], g["Xv"], g["yv"]
    hist = {}
    for optimizer in ("adam", "adagrad"):
        model = xDeepFM(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), l2_reg_dnn=1e-5, device=dev)
        model.compile(optimizer, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
        names = list(model.feature_index.keys())
        h = model.fit({n: X[:, i] for i, n in enumerate(names)}, y, batch_size=64, epochs=2, verbose=2,
                      validation_data=({n: Xv[:, i] for i, n in enumerate(names)}, yv), shuffle=False)
        hist[optimizer] = h.history
    assert type(model.optim).__name__ == "TableAdagrad"
    assert sorted(hist["adagrad"].keys()) == sorted(hist["adam"].keys()) == [str(k) for k in g["hist_keys"]]
    vals = np.array([hist["adagrad"][k] for k in sorted(hist["adagrad"])])
    assert vals.shape[1] == 2 and np.all(np.isfinite(vals))
    assert {float(st["step"]) for st in model.optim.state.values()} == {2.0 * ((X.shape[0] - 1) // 64 + 1)}


def test_trainer_runs_end_to_end_with_sgd(tmp_path):
    import importlib.util
    import json
    from conftest import PKG
    _dev()
    spec = importlib.util.spec_from_file_location("xdftrain_amd", os.path.join(PKG, "xdftrain_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / "out")
    mod.main(["--model", "xdeepfm", "--mode", "final", "--cin_layer_size", "16,8", "--dnn_hidden_units", "32,16",
              "--optimizer", "sgd", "--synthetic", "6000", "--epochs", "3", "--batch_size", "512", "--embedding_dim", "8",
              "--out_dir", out, "--verbose", "0", "--learning_rate", "0.0001"])
    for f in ("xdeepfm_full_weights.pth", "history_full.json", "preprocess.json"):
        assert os.path.exists(os.path.join(out, f)), f
    hist = json.load(open(os.path.join(out, "history_full.json")))
    assert len(hist["loss"]) == 3 and np.all(np.isfinite(hist["loss"])) and hist["loss"][-1] < hist["loss"][0]
