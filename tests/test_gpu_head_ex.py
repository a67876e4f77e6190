"""GPU tests (-m gpu) of the output head's link / loss pairs beyond (sigmoid, bce) -- the regression task and the mse / mae
losses (csrc/reg.hip; xdfm_head_fwd_ex / xdfm_head_bwd_ex; ops.Head(link, loss); BaseModel._fused_head):

  (a) every new pair against the staged float64 truth and bounds of head_ex_ref.py, through the C ABI, on the cases of
      head_ex_ref.EX_CASES (both kernel families, both B = 1 cases, a ragged stride, the LDS limit, 32 strides, the
      misaligned fall-back; c0010 with exact zeros of pred - y), guard cells around every output;
  (b) the _ex entry points with (0, 0) against the entry points without a mode, bit for bit;
  (c) (identity, mse) and (sigmoid, mae) twice in a row, bit for bit (head_ex_drivers.run_cases);
  (d) the goldens of tests/golden/regression/ (the reference run with task="regression" / "mse" / "mae"), through
      model._loss_forward and through the stock tail, in both cin_math modes, at the bars of
      test_gpu_parity.py::test_model_vs_reference_golden;
  (e) graph replay of a regression / mse train step against its eager twin, no memset node, as many nodes as the binary /
      binary_crossentropy step and fewer than with the stock tail;
  (f) a frozen cin_linear.weight with (identity, mae).
The bars of (a) are derived in head_ex_ref.py's docstring; none was fitted to what the kernels give.  Every test prints the
fraction of each bar it used before it asserts."""
import faulthandler
import gc
import os

import numpy as np
import pytest
import torch

import head_ex_drivers as DX
import head_ex_ref as X
import head_reg_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy

STEP_LIMIT_S = 300          # a hang ends the process instead of blocking the run


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(params=[0, 1], ids=["f32mfma", "f16x3"])
def cin_math(request):
    from xdfm_amd import _lib
    old = _lib.get_option("cin_math")
    _lib.set_option("cin_math", request.param)
    yield request.param
    _lib.set_option("cin_math", old)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _frac(got, ref, bound):
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    if got.size == 0:
        return 0.0
    return float((np.abs(got.reshape(ref.shape) - ref) / np.maximum(bound, 1e-300)).max())


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def close(got, want, rtol, atol, msg=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


def gclose(got, want, msg=""):
    want = np.asarray(want)
    close(got, want, rtol=2e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-9, msg=msg)


# ---------------------------------------------------------------------------------------------------------------------
# (a) kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.EX_CASES)
@pytest.mark.parametrize("mode", X.NEW_MODES, ids=X.mode_id)
def test_head_ex_against_float64(mode, name):
    dev = _dev()
    link, loss = mode
    c = X.make_ex_case(name, link)
    got = DX.run_head_ex(c, mode, dev)
    frac = {}
    p64, pb = X.pred_ref(c, link)
    frac["pred"] = _frac(got["pred"], p64, pb)
    l64, lb, terms = X.loss_ref(got["pred"], c["y"], loss)
    frac["loss"] = abs(float(got["loss"][0]) - l64) / max(lb, 1e-300)
    g64, gb = X.g_ref(got["pred"], c["y"], c["gloss"], mode)
    g32 = got["dlin"].reshape(-1)
    frac["dlin"] = _frac(g32, g64, gb)
    refs = R.head_grads_ref(g32, c["u"], c["wu"], c["v"], c["wv"])
    Ku, Kv = c["Ku"], c["Kv"]
    mine = {"du": got.get("du"), "dv": got.get("dv"), "dwu": got["grads"][:Ku], "dwv": got["grads"][Ku:Ku + Kv],
            "dbias": got["grads"][Ku + Kv]}
    assert set(refs) == {k for k, v in mine.items() if v is not None and np.size(v)}
    for k, (ref, bound) in refs.items():
        frac[k] = _frac(mine[k], ref, bound)
    vec = R.head_vectorised(Ku, Kv, c["misalign"])
    print("head_ex %-14s %-16s %s " % (X.mode_id(mode), name, "V" if vec else "S") + " ".join("%s %.3g" % kv for kv in sorted(frac.items())))
    assert got["guards"], "a guard cell around an output or a workspace was written"
    assert all(f <= 1.0 for f in frac.values()), frac
    if link == X.LINK_IDENTITY and not (Ku or Kv or c["lin"] is not None or c["bias"] is not None):
        assert (got["pred"] == 0).all()
    if name == "c0010":
        zero = slice(0, None, 3) if link == X.LINK_IDENTITY else slice(1, None, 3)
        assert (got["pred"][zero] == c["y"][zero]).all() and (terms[zero] == 0).all() and (g32[zero] == 0).all()
        assert (g32 != 0).any()
    if loss == X.LOSS_MAE and link == X.LINK_IDENTITY:
        assert set(np.unique(np.abs(g32)).tolist()) <= {0.0, abs(float(c["gloss"]))}


# ---------------------------------------------------------------------------------------------------------------------
# (b) (sigmoid, bce) through the _ex entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1111", "k3_k4_b16", "k4_k68_b2047"])
def test_head_ex_with_sigmoid_bce_equals_the_entry_points_without_a_mode(name):
    dev = _dev()
    c = R.make_head_case(name)
    a = DX.run_head_ex(c, (X.LINK_SIGMOID, X.LOSS_BCE), dev, ex=True)
    b = DX.run_head_ex(c, None, dev, ex=False)
    assert a["guards"] and b["guards"]
    assert sorted(a) == sorted(b) and {"pred", "loss", "dlin", "du", "dv", "grads"} <= set(a)
    for k in DX.OUTPUTS:
        assert _same_bits(a[k], b[k]), k
    l64, lb, _ = R.head_loss_ref(a["pred"], c["y"])
    assert abs(float(a["loss"][0]) - l64) <= lb and np.abs(a["dlin"]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# (c) twice in a row
# ---------------------------------------------------------------------------------------------------------------------
def test_head_ex_twice_in_a_row_bit_for_bit():
    """head_ex_drivers.run_cases: (identity, mse) and (sigmoid, mae) on c1111 and k4_k68_b2047, every case twice in a row:
    the same bits both times, intact guards, a finite non-zero loss and gradient."""
    out = DX.run_cases(_dev())
    keys = sorted(out)
    assert len(keys) == 4 * 2 * 7
    assert all(bool(out[k]) for k in keys if k.endswith("/guards"))
    for k in keys:
        if "/0/" in k:
            assert _same_bits(out[k], out[k.replace("/0/", "/1/")]), k
        if k.endswith(("/loss", "/grads")):
            assert np.isfinite(out[k]).all() and np.abs(out[k]).max() > 0, k


# ---------------------------------------------------------------------------------------------------------------------
# (d) goldens of the reference
# ---------------------------------------------------------------------------------------------------------------------
LOSS_FUNCS = {"mse": torch.nn.functional.mse_loss, "mae": torch.nn.functional.l1_loss}


@pytest.mark.parametrize("name", ["reg_xdeepfm_mse", "reg_attn_mae", "bin_xdeepfm_mse"])
def test_regression_model_vs_reference_golden(name, cin_math):
    dev = _dev()
    from xdfm_amd import ops
    g = load_golden("regression/" + name)
    model = DX.build_golden_model(g, dev)
    for k, v in model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), g["init:" + k], err_msg="init " + k)
    model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
    B, loss_name = int(g["B"]), str(g["loss_name"])
    fn = LOSS_FUNCS[loss_name]
    Xd, yd = T(g["X"]).to(dev), T(g["y"]).to(dev)
    model.compile("adam", loss_name, metrics=["mse"])
    model.train()
    assert ops.head_mode(model.out.task, model.loss_func) == ({"regression": 1, "binary": 0}[str(g["task"])], {"mse": 1, "mae": 2}[loss_name])

    def step1(native):
        model.optim.zero_grad()
        if native:
            y_pred, loss = model._loss_forward(Xd[:B], yd[:B])
            assert "Head" in type(loss.grad_fn).__name__ or "Head" in type(loss.grad_fn.next_functions[0][0]).__name__, loss.grad_fn
        else:
            y_pred = model(Xd[:B])
            loss = fn(y_pred.squeeze(), yd[:B].squeeze(), reduction="sum")
        reg = model.get_regularization_loss()
        fr = dict(y_pred=_frac(y_pred.detach().cpu().numpy().reshape(-1), g["y_pred"].reshape(-1),
                               1e-6 + 2e-5 * np.abs(g["y_pred"].reshape(-1))),
                  loss=abs(loss.item() - float(g["loss"])) / (2e-5 * abs(float(g["loss"]))))
        (loss + reg).backward()
        fr["grad"] = max(_frac(p.grad.cpu().numpy(), g["g:" + k], 2e-4 * np.abs(g["g:" + k]) + 2e-5 * float(np.abs(g["g:" + k]).max()) + 1e-9)
                         for k, p in model.named_parameters())
        print("%s cin_math %d %s: share of the bars %s" % (name, cin_math, "native head" if native else "stock tail", fr))
        close(y_pred.reshape(-1), g["y_pred"].reshape(-1), rtol=2e-5, atol=1e-6, msg="y_pred")
        assert abs(loss.item() - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
        assert abs(reg.item() - float(g["reg"])) <= 1e-5 * abs(float(g["reg"]))
        for k, p in model.named_parameters():
            gclose(p.grad, g["g:" + k], k)

    step1(True)
    step1(False)
    model.optim.zero_grad()
    losses = []
    for s in range(3):
        out = model.train_on_batch(Xd[s * B:(s + 1) * B], yd[s * B:(s + 1) * B])
        losses.append([float(out[1].detach().reshape(-1)[0]), float(out[2].detach().reshape(-1)[0])])
    print("%s losses %s" % (name, losses))
    np.testing.assert_allclose(np.array(losses), g["losses3"], rtol=2e-5)
    for k, v in model.state_dict().items():
        close(v, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="after 3 steps: " + k)
    names = list(model.feature_index.keys())
    pred = model.predict({n: g["X"][:, i] for i, n in enumerate(names)}, batch_size=B)
    assert pred.shape == (g["X"].shape[0], 1)
    close(pred, g["pred_after"], rtol=1e-4, atol=2e-6, msg="predict")


# ---------------------------------------------------------------------------------------------------------------------
# (e) graph replay
# ---------------------------------------------------------------------------------------------------------------------
def _graph_columns():
    from deepctr.inputs import DenseFeat, SparseFeat
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    return vocab, nd, [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]


def _graph_batch(s, task, dev):
    from oracle import xdeepfm_oracle as orc
    vocab, nd, _ = _graph_columns()
    Xn, yn = orc.synthetic_batch(256 if s != 6 else 100, vocab, nd, seed=100 + s)     # one ragged batch
    if task == "regression":
        yn = (3.0 + 1.5 * np.random.default_rng(500 + s).standard_normal(yn.shape)).astype(np.float32)
    return T(Xn).to(dev), T(yn).to(dev)


def _graph_model(task, loss, dev):
    from deepctr.models import xDeepFM
    _, _, cols = _graph_columns()
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, task=task, device=dev)
    model.compile("adam", loss, metrics=[])
    model.train()
    return model


def _run_steps(task, loss, dev, steps, use_graph):
    from xdfm_amd import graphstep
    model = _graph_model(task, loss, dev)
    step = graphstep.GraphedStep(model)
    step.disabled = not use_graph
    model.__dict__["_graphed_step"] = step
    losses = []
    for s in range(steps):
        out = model.train_on_batch(*_graph_batch(s, task, dev))
        losses.append(float(out[2].detach().reshape(-1)[0]))
    return model, step, losses


def _stock_tail_census(task, loss, dev):
    """(nodes, memset nodes, other nodes) of one captured train step of the same model with the stock tail
    (_fused_head -> None).  The graph is only counted, never replayed."""
    from xdfm_amd import graphstep
    model = _graph_model(task, loss, dev)
    model._fused_head = lambda x, y: None
    step = graphstep.GraphedStep(model)
    model.__dict__["_graphed_step"] = step
    x, y = _graph_batch(0, task, dev)
    if hasattr(model.optim, "sync_lr"):
        model.optim.sync_lr()                  # as GraphedStep.__call__: the device scalar K7 reads, set outside the capture
    for _ in range(graphstep.EAGER_STEPS_BEFORE_CAPTURE):
        step._eager_on_side_stream(x, y)
    torch.cuda.synchronize()
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        sx, sy = x.clone(), y.clone()
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, stream=step.stream):
            model._train_step_eager(sx, sy)
        return graphstep.census(graph)
    finally:
        if was:
            gc.enable()


def test_graph_replay_of_regression_train_step():
    from xdfm_amd import graphstep
    if os.environ.get("XDFM_HIP_GRAPH", "1") == "0":
        pytest.skip("XDFM_HIP_GRAPH=0")
    dev = _dev()
    m_g, step_g, l_g = _run_steps("regression", "mse", dev, 10, True)
    m_e, step_e, l_e = _run_steps("regression", "mse", dev, 10, False)
    assert step_e.replays == 0 and step_g.replays >= 5 and not step_g.disabled, (step_g.replays, step_g.disabled)
    graphs = [e for e in step_g.entries.values() if e.graph is not None]
    assert len(graphs) == 1
    n, n_memset, n_other = graphstep.census(graphs[0].graph)
    _, step_b, _ = _run_steps("binary", "binary_crossentropy", dev, 3, True)
    bin_graphs = [e for e in step_b.entries.values() if e.graph is not None]
    assert len(bin_graphs) == 1 and not step_b.disabled
    n_bin = graphstep.census(bin_graphs[0].graph)[0]
    n_stock, ms_stock, other_stock = _stock_tail_census("regression", "mse", dev)
    print("captured train step: regression / mse %d nodes (%d memset, %d other); binary / bce %d; regression / mse with the "
          "stock tail %d (%d memset, %d other)" % (n, n_memset, n_other, n_bin, n_stock, ms_stock, other_stock))
    assert n > 20 and n_memset == 0 and n_other == 0
    assert n == n_bin
    assert n < n_stock
    np.testing.assert_allclose(l_g, l_e, rtol=2e-5)
    for (k, a), (_, b) in zip(m_g.state_dict().items(), m_e.state_dict().items()):
        close(a, b.cpu().numpy(), rtol=2e-3, atol=2e-6, msg=k)


# ---------------------------------------------------------------------------------------------------------------------
# (f) a frozen head weight
# ---------------------------------------------------------------------------------------------------------------------
def test_frozen_cin_linear_weight_with_identity_mae():
    dev = _dev()
    x, y = _graph_batch(1, "regression", dev)

    def grads(freeze):
        model = _graph_model("regression", "mae", dev)
        if freeze:
            model.cin_linear.weight.requires_grad_(False)
        model.optim.zero_grad()
        y_pred, loss = model._loss_forward(x, y)
        assert "Head" in type(loss.grad_fn).__name__ or "Head" in type(loss.grad_fn.next_functions[0][0]).__name__
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), {k: (None if p.grad is None else p.grad.detach().cpu().numpy().copy()) for k, p in model.named_parameters()}

    l_a, a = grads(False)
    l_b, b = grads(True)
    assert l_a == l_b and np.isfinite(l_a)
    assert a["cin_linear.weight"] is not None and np.abs(a["cin_linear.weight"]).max() > 0
    assert b["cin_linear.weight"] is None
    for k in a:
        if k != "cin_linear.weight":
            assert (a[k] is None) == (b[k] is None), k
            assert a[k] is None or _same_bits(a[k], b[k]), k
    assert sum(v is not None for v in b.values()) >= len(b) - 1
