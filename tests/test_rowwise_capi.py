"""CPU: xdfm_rowwise_adagrad_step (K7w) is declared, bound and exported and validates its arguments before any device work, with
the offending value in the message; compile("rowwise_adagrad") on a CPU model -- the class, its two groups and state shapes;
five torch-op steps against a float64 replay; the checkpoint round trip; the trainer's --rowwise_adagrad switches (no GPU
compute)."""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

import rowwise_ref as W
from conftest import PKG, ROOT


def test_the_symbol_is_declared_bound_and_exported():
    from xdfm_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "xdfm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bxdfm_rowwise_adagrad_step\s*\(", header) and re.search(r"\}\s*xdfm_rowwise_tensor\s*;", header)
    assert "xdfm_rowwise_adagrad_step" in _lib.SIGNATURES and hasattr(lib, "xdfm_rowwise_adagrad_step")
    assert "xdfm_rowwise_tensor, xdfm_rowwise_adagrad_step" in text          # the ABI note
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9                   # additions only
    assert re.search(r"#define XDFM_ABI_VERSION 9\b", header)
    assert len(_lib.SIGNATURES["xdfm_rowwise_adagrad_step"][1]) == 8
    assert ctypes.sizeof(_lib.RowwiseTensor) == 48 and ctypes.sizeof(_lib.OptTensor) == 48 and ctypes.sizeof(_lib.FtrlTensor) == 56
    body = re.search(r"typedef struct \{([^}]*)\}\s*xdfm_rowwise_tensor", header).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in _lib.RowwiseTensor._fields_]
    assert int(re.search(r"#define XDFM_ROWWISE_MAX_DIM (\d+)", header).group(1)) == 1024
    assert "neighbouring pairs first" in text                                # the summation order is documented in the header


def test_bad_arguments_are_refused_before_any_device_work():
    from xdfm_amd import _lib
    lib = _lib.load()
    one = (_lib.RowwiseTensor * 1)()
    arr = ctypes.cast(one, ctypes.c_void_p)
    buf = (ctypes.c_float * 16)()
    base = (ctypes.addressof(buf) + 15) & ~15                # a 16-byte aligned host address: never dereferenced
    host = ctypes.c_void_p(base)
    nan = float("nan")

    def refused(rc, *texts):
        msg = lib.xdfm_last_error()
        assert rc == 1 and all(t in msg for t in texts), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc, "rowwise")

    def step(tensors=arr, T=1, lr=0.01, eps=1e-10, ws=None, val=None):
        return lib.xdfm_rowwise_adagrad_step(tensors, T, lr, None, eps, ws, val, None)

    refused(step(tensors=None), b"null pointer")
    refused(step(T=0), b"bad tensor count 0")
    refused(step(T=-2), b"bad tensor count -2")
    refused(step(T=70000), b"bad tensor count 70000")
    refused(step(lr=-0.01), b"bad hyper-parameters", b"lr -0.01 is negative")
    refused(step(lr=nan), b"bad hyper-parameters", b"nan")
    refused(lib.xdfm_rowwise_adagrad_step(arr, 1, -1.0, host, 1e-10, None, None, None), b"lr -1 ")     # with lr_dev too
    refused(step(eps=0.0), b"eps 0 is not above 0")
    refused(step(eps=-1e-3), b"eps -0.001 is not above 0")
    refused(step(eps=nan), b"eps nan")
    refused(step(val=host), b"l2_value needs l2_ws")
    refused(step(), b"tensor 0 has a null pointer (param)")
    one[0].param = base
    refused(step(), b"tensor 0 has a null pointer (grad)")
    one[0].grad = base
    refused(step(), b"tensor 0 has a null pointer (state)")
    one[0].state = base
    one[0].rows, one[0].dim = -3, 4
    refused(step(), b"negative row count -3")
    one[0].rows = 2
    for dim in (0, -1, 1025):
        one[0].dim = dim
        refused(step(), b"dim %d outside [1, 1024]" % dim)
    one[0].dim, one[0].l2 = 4, -1.0
    refused(step(), b"negative l2 -1")
    one[0].l2, one[0].state = 0.0, base + 2
    refused(step(), b"misaligned state", b"%x" % (base + 2))
    one[0].state, one[0].grad_marks, one[0].grad = base + 4, base, base + 4        # the state needs 4 bytes only ...
    refused(step(), b"grad_marks but a pointer that is not 16-byte aligned", b"%x" % (base + 4))
    one[0].grad, one[0].param = base, base + 8                                    # ... the marks 16 for param and grad
    refused(step(), b"grad_marks but a pointer that is not 16-byte aligned", b"%x" % (base + 8))


def test_the_class_refuses_bad_hyper_parameters_and_shapes_on_the_host():
    from xdfm_amd.optim import TableRowwiseAdagrad
    ps = [torch.nn.Parameter(torch.randn(5, 3))]
    for kw, shown in ((dict(lr=-1.0), "lr -1.0"), (dict(eps=0.0), "eps 0.0"), (dict(eps=-1e-3), "eps -0.001"),
                      (dict(initial_accumulator_value=-0.1), "initial_accumulator_value -0.1"), (dict(lr=float("nan")), "lr nan")):
        with pytest.raises(ValueError, match=re.escape(shown)):
            TableRowwiseAdagrad(ps, **kw)
    for bad in (torch.randn(4), torch.randn(2, 3, 4), torch.randn(())):
        with pytest.raises(ValueError, match="2-D parameters only"):
            TableRowwiseAdagrad([dict(params=[torch.nn.Parameter(bad)], rowwise=True)])
    opt = TableRowwiseAdagrad(ps)
    g = opt.param_groups[0]
    assert {k: g[k] for k in ("lr", "eps", "initial_accumulator_value", "rowwise")} == dict(
        lr=0.01, eps=1e-10, initial_accumulator_value=0.0, rowwise=False)
    assert issubclass(TableRowwiseAdagrad, torch.optim.Optimizer) and opt.table_step and opt.owns(ps) and opt.generation == 0
    assert opt.deferred is False and opt._kind(g) == "adagrad" and opt._kind(dict(g, rowwise=True)) == "rowwise" and opt._plain(g)
    opt.flush()
    assert opt.take_backlog() == 0.0                          # the no-ops of an optimizer that defers nothing
    with pytest.raises(ValueError, match="2-D parameters only"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.randn(3))], rowwise=True))
    opt.add_param_group(dict(params=[torch.nn.Parameter(torch.randn(3, 2))], rowwise=True))
    assert opt.param_groups[1]["rowwise"] is True and opt.param_groups[1]["eps"] == 1e-10


def test_xdfm_opt_deferred_is_not_read(monkeypatch):
    from xdfm_amd.optim import TableRowwiseAdagrad
    monkeypatch.setenv("XDFM_OPT_DEFERRED", "1")
    assert TableRowwiseAdagrad([torch.nn.Parameter(torch.randn(3))]).deferred is False


def _cpu_model(D=4, varlen=False):
    from deepctr.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C1", 7, D), SparseFeat("C2", 5, D), DenseFeat("I1", 1)]
    if varlen:
        cols.append(VarLenSparseFeat(SparseFeat("V1", 6, D), maxlen=3, combiner="mean"))
    torch.manual_seed(0)
    return xDeepFM(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), device="cpu")


def test_cpu_model_compiles_the_class_with_two_groups():
    from xdfm_amd.optim import TableRowwiseAdagrad
    model = _cpu_model(varlen=True)
    model.compile("rowwise_adagrad", "binary_crossentropy")
    opt = model.optim
    assert type(opt) is TableRowwiseAdagrad and not model._optim_capturable
    assert len(opt.param_groups) == 2 and [g["rowwise"] for g in opt.param_groups] == [True, False]
    for g in opt.param_groups:
        assert (g["lr"], g["eps"], g["initial_accumulator_value"]) == (0.01, 1e-10, 0.0)
    names = {id(p): k for k, p in model.named_parameters()}
    rowwise = sorted(names[id(p)] for p in opt.param_groups[0]["params"])
    assert rowwise == sorted(k for k in names.values() if "embedding_dict" in k) and len(rowwise) == 6      # 3 tables + 3 linear, V1 included
    assert all(p.dim() == 2 for p in opt.param_groups[0]["params"])
    assert sum(len(g["params"]) for g in opt.param_groups) == len(list(model.parameters()))
    assert not any("embedding_dict" in names[id(p)] for p in opt.param_groups[1]["params"])
    mine = TableRowwiseAdagrad.for_model(model, lr=0.1, eps=1e-8, initial_accumulator_value=0.5)
    model.compile(mine, "binary_crossentropy")               # an object keeps its hyper-parameters
    assert model.optim is mine and mine.param_groups[0]["eps"] == 1e-8 and mine.param_groups[1]["initial_accumulator_value"] == 0.5
    with pytest.raises(NotImplementedError):
        model.compile("rowwise", "binary_crossentropy")
    model.compile("adagrad", "binary_crossentropy")          # the other strings did not change
    assert type(model.optim) is torch.optim.Adagrad
    # a model without tables: one element-wise group
    lin = TableRowwiseAdagrad.for_model(torch.nn.Linear(3, 1))
    assert len(lin.param_groups) == 1 and lin.param_groups[0]["rowwise"] is False


def _fake_backward(model, seed):
    """The model's forward has no CPU path: gradients of the kind a batch leaves -- a few rows of every table, everything of
    the dense tensors -- are written into .grad, and the model's L2 term is armed as its train step arms it."""
    g = torch.Generator().manual_seed(seed)
    tables = []
    for k, p in model.named_parameters():
        grad = torch.randn(p.shape, generator=g) * (1e-3 if seed % 2 else 1e3)
        if "embedding_dict" in k:
            rows = torch.rand(p.shape[0], generator=g) < 0.4
            grad[~rows] = 0.0
            tables.append(p)
        p.grad = grad
    model.optim.arm_l2(tables, [1e-5] * len(tables))


def record_steps(opt, log):
    """Wrap opt.step: before every step keep (parameter, its value, its `sum`, its gradient, its armed L2 strength, its group)."""
    real = opt.step

    def step(closure=None):
        armed = dict(opt._armed or {})
        rec = []
        for g in opt.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = opt.state.get(p, {})
                shape = (p.shape[0],) if g["rowwise"] else tuple(p.shape)
                s = st["sum"].clone() if "sum" in st else torch.full(shape, float(g["initial_accumulator_value"]), device=p.device)
                rec.append((p, p.detach().clone(), s, p.grad.detach().clone(), armed.get(id(p), 0.0), g))
        out = real(closure)
        log.append((rec, opt.l2_value))
        return out
    opt.step = step


def worst_ratios(opt, log):
    """Every recorded step against rw_f64 from the fp32 state it started with -> (worst p ratio, worst s ratio, [L2 values])."""
    wp = ws = 0.0
    values = []
    for s, (rec, _) in enumerate(log):
        nxt = {id(r[0]): r for r in log[s + 1][0]} if s + 1 < len(log) else None
        value = 0.0
        for p, p0, s0, grad, l2m, g in rec:
            p1 = (nxt[id(p)][1] if nxt else p.detach()).cpu().numpy()
            s1 = (nxt[id(p)][2] if nxt else opt.state[p]["sum"]).cpu().numpy()
            a, b, c = p0.cpu().numpy(), s0.cpu().numpy(), grad.cpu().numpy()
            if not g["rowwise"]:                             # element-wise Adagrad is row-wise with D = 1
                p1, s1, a, b, c = p1.reshape(-1, 1), s1.reshape(-1), a.reshape(-1, 1), b.reshape(-1), c.reshape(-1, 1)
            rp, rs = W.ratios(p1, s1, a, b, c, g["lr"], l2m, g["eps"])
            value += W.rw_f64(a, b, c, g["lr"], l2m, g["eps"])[2]
            wp, ws = max(wp, rp), max(ws, rs)
        values.append(value)
    return wp, ws, values


@pytest.mark.parametrize("D,varlen", [(4, False), (10, True)], ids=["D4", "D10_varlen"])
def test_five_torch_op_steps_stay_within_the_bar_of_a_float64_replay(D, varlen):
    model = _cpu_model(D, varlen)
    model.compile("rowwise_adagrad", "binary_crossentropy")
    model.train()
    opt = model.optim
    log = []
    record_steps(opt, log)
    for s in range(5):
        _fake_backward(model, 50 + s)
        opt.step()
    assert len(log) == 5 and all(len(rec) > 8 for rec, _ in log)
    assert sum(1 for r in log[0][0] if r[4] > 0) >= 4                 # the tables carry an armed L2 term
    for p in opt.param_groups[0]["params"]:
        assert opt.state[p]["sum"].shape == (p.shape[0],) and opt.state[p]["sum"].dtype == torch.float32
    for p in opt.param_groups[1]["params"]:
        assert opt.state[p]["sum"].shape == p.shape
    wp, ws, values = worst_ratios(opt, log)
    print("row-wise torch-op steps D=%d: worst ratio p %.3f s %.3f (C = %g)" % (D, wp, ws, W.C_BAR))
    assert wp <= W.C_BAR and ws <= W.C_BAR
    for (rec, l2_value), value in zip(log, values):
        assert abs(float(l2_value) - value) <= 1e-5 * value, (float(l2_value), value)


def test_state_dict_round_trip_and_pickle():
    from xdfm_amd.optim import TableRowwiseAdagrad
    torch.manual_seed(0)

    def params():
        torch.manual_seed(1)
        return [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(4)), torch.nn.Parameter(torch.randn(6, 10))]

    def make(ps, **kw):
        return TableRowwiseAdagrad([dict(params=[ps[0], ps[2]], rowwise=True), dict(params=[ps[1]])], **kw)
    ps, qs = params(), params()
    kw = dict(lr=0.1, eps=1e-8, initial_accumulator_value=0.2)
    a, b = make(ps, **kw), make(qs, lr=0.7)
    grads = [[torch.randn_like(p) for p in ps] for _ in range(4)]

    def run(opt, prm, steps):
        for gs in steps:
            for p, g in zip(prm, gs):
                p.grad = g.clone()
            opt.step()
    run(a, ps, grads[:2])
    assert list(a.state[ps[0]].keys()) == ["sum"] and a.state[ps[0]]["sum"].shape == (5,) and a.state[ps[1]]["sum"].shape == (4,)
    assert a.state[ps[2]]["sum"].shape == (6,) and float(a.state[ps[2]]["sum"].min()) > 0.2
    sd = copy.deepcopy(a.state_dict())
    assert {k: v for k, v in sd["param_groups"][0].items() if k != "params"} == dict(kw, rowwise=True)
    assert sd["param_groups"][1]["rowwise"] is False and sorted(sd["state"][0].keys()) == ["sum"]
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    gen = b.generation
    b.load_state_dict(sd)
    assert b.generation > gen and b.param_groups[0]["eps"] == 1e-8 and b.param_groups[0]["lr"] == 0.1
    c = pickle.loads(pickle.dumps(a))                          # a pickled optimizer carries its parameters with it
    assert type(c) is TableRowwiseAdagrad and c.deferred is False and c.grad_sources == [] and c.generation > a.generation
    rs = [c.param_groups[0]["params"][0], c.param_groups[1]["params"][0], c.param_groups[0]["params"][1]]
    run(a, ps, grads[2:])
    run(b, qs, grads[2:])
    run(c, rs, grads[2:])
    for p, q, r in zip(ps, qs, rs):
        assert torch.equal(p, q) and torch.equal(p, r)
        assert torch.equal(a.state[p]["sum"], b.state[q]["sum"]) and torch.equal(a.state[p]["sum"], c.state[r]["sum"])


def test_torch_save_of_a_compiled_model_works(tmp_path):
    model = _cpu_model()
    model.compile("rowwise_adagrad", "binary_crossentropy")
    model.train()
    _fake_backward(model, 3)
    model.optim.step()
    path = str(tmp_path / "model.pt")
    torch.save(model, path)
    back = torch.load(path, weights_only=False)
    assert type(back.optim).__name__ == "TableRowwiseAdagrad" and [g["rowwise"] for g in back.optim.param_groups] == [True, False]
    for p, q in zip(model.parameters(), back.parameters()):
        assert torch.equal(p, q)


def _trainer():
    import importlib.util
    spec = importlib.util.spec_from_file_location("xdftrain_amd", os.path.join(PKG, "xdftrain_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_parses_the_switches_and_refuses_their_misuse(capsys):
    from xdfm_amd.optim import TableRowwiseAdagrad
    mod = _trainer()
    args = mod.parse_args([])
    assert args.rowwise_adagrad is False and (args.rowwise_eps, args.rowwise_init_acc) == (1e-10, 0.0)
    args = mod.parse_args(["--rowwise_adagrad"])
    assert args.rowwise_adagrad is True and (args.rowwise_eps, args.rowwise_init_acc) == (1e-10, 0.0)
    args = mod.parse_args(["--rowwise_adagrad", "--rowwise_eps", "1e-8", "--rowwise_init_acc", "0.1", "--learning_rate", "0.05"])
    assert (args.rowwise_eps, args.rowwise_init_acc) == (1e-8, 0.1)
    model = _cpu_model()
    opt = mod.make_optimizer(args, model)
    assert type(opt) is TableRowwiseAdagrad and [g["rowwise"] for g in opt.param_groups] == [True, False]
    for g in opt.param_groups:
        assert (g["lr"], g["eps"], g["initial_accumulator_value"]) == (0.05, 1e-8, 0.1)
    assert mod.make_optimizer(mod.parse_args(["--optimizer", "adagrad"]), model) == "adagrad"      # without the switch: as before
    assert type(mod.make_optimizer(mod.parse_args(["--ftrl"]), model)).__name__ == "TableFTRL"
    for argv, text in ((["--rowwise_adagrad", "--ftrl"], "--rowwise_adagrad does not go with --ftrl"),
                       (["--rowwise_adagrad", "--optimizer", "sgd", "--momentum", "0.9"], "--rowwise_adagrad does not go with --momentum / --nesterov"),
                       (["--rowwise_adagrad", "--nesterov"], "--rowwise_adagrad does not go with"),
                       (["--rowwise_eps", "1e-8"], "--rowwise_eps need(s) --rowwise_adagrad"),
                       (["--rowwise_init_acc", "0"], "--rowwise_init_acc need(s) --rowwise_adagrad"),
                       (["--rowwise_eps", "1e-8", "--rowwise_init_acc", "0.1"], "--rowwise_eps, --rowwise_init_acc need(s) --rowwise_adagrad"),
                       (["--ftrl", "--rowwise_eps", "1e-8"], "need(s) --rowwise_adagrad"),
                       (["--rowwise_adagrad", "--rowwise_eps", "0"], "--rowwise_eps 0 is not above 0"),
                       (["--rowwise_adagrad", "--rowwise_init_acc", "-1"], "--rowwise_init_acc -1 is negative"),
                       (["--rowwise_adagrad", "--learning_rate", "-0.1"], "--rowwise_adagrad needs --learning_rate >= 0")):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv


def test_the_optimizer_choices_did_not_change():
    src = open(os.path.join(PKG, "xdftrain_amd.py")).read()
    assert 'choices=["adam", "adagrad", "sgd", "rmsprop"]' in src
    mod = _trainer()
    with pytest.raises(SystemExit):
        mod.parse_args(["--optimizer", "rowwise_adagrad"])
