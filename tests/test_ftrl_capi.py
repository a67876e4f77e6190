"""CPU: xdfm_ftrl_step (K7f) is declared, bound and exported and validates its arguments before any device work, with the
offending value in the message; compile("ftrl") on a CPU model; TableFTRL's host-side refusals, state_dict round trip and
pickling; the trainer's --ftrl switches (no GPU compute)."""
import copy
import ctypes
import os
import pickle
import re

import pytest
import torch

from conftest import PKG, ROOT


def test_the_symbol_is_declared_bound_and_exported():
    from xdfm_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "xdfm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bxdfm_ftrl_step\s*\(", header) and re.search(r"\}\s*xdfm_ftrl_tensor\s*;", header)
    assert "xdfm_ftrl_step" in _lib.SIGNATURES and hasattr(lib, "xdfm_ftrl_step")
    assert "xdfm_ftrl_tensor, xdfm_ftrl_step" in text                # the ABI note
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9           # additions only
    assert len(_lib.SIGNATURES["xdfm_ftrl_step"][1]) == 10
    assert ctypes.sizeof(_lib.FtrlTensor) == 56 and ctypes.sizeof(_lib.OptTensor) == 48
    # the descriptor's members, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\}\s*xdfm_ftrl_tensor", header).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in _lib.FtrlTensor._fields_]


def test_bad_arguments_are_refused_before_any_device_work():
    from xdfm_amd import _lib
    lib = _lib.load()
    one = (_lib.FtrlTensor * 1)()
    arr = ctypes.cast(one, ctypes.c_void_p)
    buf = (ctypes.c_float * 16)()
    base = (ctypes.addressof(buf) + 15) & ~15                # a 16-byte aligned host address: never dereferenced
    host = ctypes.c_void_p(base)
    nan = float("nan")

    def refused(rc, *texts):
        msg = lib.xdfm_last_error()
        assert rc == 1 and all(t in msg for t in texts), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc, "ftrl")

    def step(tensors=arr, T=1, lr=0.05, l1=0.0, l2=0.0, beta=1.0, ws=None, val=None):
        return lib.xdfm_ftrl_step(tensors, T, lr, None, l1, l2, beta, ws, val, None)

    refused(step(tensors=None), b"null pointer")
    refused(step(T=0), b"bad tensor count 0")
    refused(step(T=-2), b"bad tensor count -2")
    refused(step(T=70000), b"bad tensor count 70000")
    for lr, shown in ((0.0, b"lr 0 "), (-0.01, b"lr -0.01 "), (nan, b"nan")):
        refused(step(lr=lr), b"bad hyper-parameters", shown, b"not above 0")
    refused(lib.xdfm_ftrl_step(arr, 1, 0.0, host, 0.0, 0.0, 1.0, None, None, None), b"lr 0 ")        # with lr_dev too
    refused(step(l1=-1e-3), b"l1 -0.001 is negative")
    refused(step(l2=-2.0), b"l2 -2 is negative")
    refused(step(beta=-0.5), b"beta -0.5 is negative")
    refused(step(l1=nan), b"l1 nan")
    refused(step(), b"tensor 0 has a null pointer")                                                   # param / grad NULL
    one[0].param = one[0].grad = base
    one[0].numel = 8
    refused(step(), b"tensor 0 has no state (z)")
    one[0].z = base
    refused(step(), b"tensor 0 has no state (n)")
    one[0].n = base + 2
    refused(step(), b"misaligned state", b"%x" % (base + 2))
    one[0].n, one[0].grad_marks = base + 4, base
    refused(step(), b"grad_marks but a pointer that is not 16-byte aligned", b"%x" % (base + 4))
    one[0].z, one[0].n = base + 8, base
    refused(step(), b"grad_marks but a pointer that is not 16-byte aligned", b"%x" % (base + 8))
    one[0].z, one[0].grad_marks = base, None
    refused(step(val=host), b"l2_value needs l2_ws")
    one[0].l2 = -1.0
    refused(step(), b"negative l2")
    one[0].l2, one[0].numel = 0.0, -1
    refused(step(), b"negative size")


def test_the_class_refuses_bad_hyper_parameters_on_the_host():
    from xdfm_amd.optim import TableFTRL
    ps = [torch.nn.Parameter(torch.randn(5, 3))]
    for kw, shown in ((dict(lr=0.0), "lr 0.0"), (dict(lr=-1.0), "lr -1.0"), (dict(l1=-1e-3), "l1 -0.001"), (dict(l2=-2.0), "l2 -2.0"),
                      (dict(beta=-0.5), "beta -0.5"), (dict(initial_accumulator_value=-0.1), "initial_accumulator_value -0.1"),
                      (dict(lr=float("nan")), "lr nan")):
        with pytest.raises(ValueError, match=re.escape(shown)):
            TableFTRL(ps, **kw)
    opt = TableFTRL(ps)
    g = opt.param_groups[0]
    assert {k: v for k, v in g.items() if k in ("lr", "l1", "l2", "beta", "initial_accumulator_value")} == dict(
        lr=0.05, l1=0.0, l2=0.0, beta=1.0, initial_accumulator_value=0.1)
    assert issubclass(TableFTRL, torch.optim.Optimizer) and opt.table_step and opt.owns(ps) and opt.generation == 0
    assert opt.deferred is False and opt._kind(g) == "ftrl" and opt._hyper(g) == (0.0, 0.0, 1.0) and opt._plain(g)
    opt.flush()
    assert opt.take_backlog() == 0.0                          # the no-ops of an optimizer that defers nothing
    for key, val in (("l1", -1.0), ("l2", torch.tensor(0.1)), ("beta", -1e-9)):
        assert not opt._plain(dict(g, **{key: val})), key
    # a rate <= 0 never reaches the device scalar, nor the torch-op step
    for bad in (0.0, -0.05):
        g["lr"] = bad
        with pytest.raises(ValueError, match=re.escape("lr %r" % bad)):
            opt.sync_lr()
        ps[0].grad = torch.ones_like(ps[0])
        with pytest.raises(ValueError, match=re.escape("lr %r" % bad)):
            opt.step()
    assert len(opt.state) == 0                                # refused before any state was made


def test_xdfm_opt_deferred_is_not_read(monkeypatch):
    from xdfm_amd.optim import TableFTRL
    monkeypatch.setenv("XDFM_OPT_DEFERRED", "1")
    assert TableFTRL([torch.nn.Parameter(torch.randn(3))]).deferred is False


def _cpu_model():
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C1", 7, 4), SparseFeat("C2", 5, 4), DenseFeat("I1", 1)]
    return xDeepFM(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), device="cpu")


def test_cpu_model_compiles_table_ftrl_with_the_defaults():
    from xdfm_amd.optim import TableFTRL
    model = _cpu_model()
    model.compile("ftrl", "binary_crossentropy")
    assert type(model.optim) is TableFTRL and not model._optim_capturable
    g = model.optim.param_groups[0]
    assert (g["lr"], g["l1"], g["l2"], g["beta"], g["initial_accumulator_value"]) == (0.05, 0.0, 0.0, 1.0, 0.1)
    assert len(g["params"]) == len(list(model.parameters()))
    mine = TableFTRL(model.parameters(), lr=0.1, l1=1e-2, l2=1e-3, beta=0.5, initial_accumulator_value=0.0)
    model.compile(mine, "binary_crossentropy")               # an object keeps its hyper-parameters
    assert model.optim is mine and model.optim.param_groups[0]["l1"] == 1e-2 and model.optim.param_groups[0]["beta"] == 0.5
    with pytest.raises(NotImplementedError):
        model.compile("ftrl2", "binary_crossentropy")
    model.compile("sgd", "binary_crossentropy")              # the other strings did not change
    assert type(model.optim) is torch.optim.SGD


def test_state_dict_round_trip_and_pickle():
    from xdfm_amd.optim import TableFTRL
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(4))]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    kw = dict(lr=0.1, l1=1e-2, l2=1e-3, beta=0.5, initial_accumulator_value=0.2)
    a, b = TableFTRL(ps, **kw), TableFTRL(qs, lr=0.7)
    grads = [[torch.randn_like(p) for p in ps] for _ in range(4)]

    def run(opt, params, steps):
        for gs in steps:
            for p, g in zip(params, gs):
                p.grad = g.clone()
            opt.step()
    run(a, ps, grads[:2])
    assert sorted(a.state[ps[0]].keys()) == ["n", "z"] and a.state[ps[0]]["n"].shape == ps[0].shape
    sd = copy.deepcopy(a.state_dict())
    assert {k: v for k, v in sd["param_groups"][0].items() if k != "params"} == kw
    assert sorted(sd["state"][0].keys()) == ["n", "z"]
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    gen = b.generation
    b.load_state_dict(sd)
    assert b.generation > gen and b.param_groups[0]["l1"] == 1e-2 and b.param_groups[0]["lr"] == 0.1
    c = pickle.loads(pickle.dumps(a))                          # a pickled optimizer carries its parameters with it
    assert type(c) is TableFTRL and c.deferred is False and c.grad_sources == [] and c.generation > a.generation
    rs = c.param_groups[0]["params"]
    run(a, ps, grads[2:])
    run(b, qs, grads[2:])
    run(c, rs, grads[2:])
    for p, q, r in zip(ps, qs, rs):
        assert torch.equal(p, q) and torch.equal(p, r)
        for k in "zn":
            assert torch.equal(a.state[p][k], b.state[q][k]) and torch.equal(a.state[p][k], c.state[r][k])


def _trainer():
    import importlib.util
    spec = importlib.util.spec_from_file_location("xdftrain_amd", os.path.join(PKG, "xdftrain_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_parses_the_ftrl_switches_and_refuses_their_misuse(capsys):
    from xdfm_amd.optim import TableFTRL
    mod = _trainer()
    args = mod.parse_args([])
    assert args.ftrl is False and (args.ftrl_l1, args.ftrl_l2, args.ftrl_beta, args.ftrl_init_acc) == (0.0, 0.0, 1.0, 0.1)
    args = mod.parse_args(["--ftrl"])
    assert args.ftrl is True and (args.ftrl_l1, args.ftrl_l2, args.ftrl_beta, args.ftrl_init_acc) == (0.0, 0.0, 1.0, 0.1)
    args = mod.parse_args(["--ftrl", "--ftrl_l1", "0.01", "--ftrl_l2", "0.002", "--ftrl_beta", "0.5", "--ftrl_init_acc", "0",
                           "--learning_rate", "0.05"])
    assert (args.ftrl_l1, args.ftrl_l2, args.ftrl_beta, args.ftrl_init_acc) == (0.01, 0.002, 0.5, 0.0)
    model = torch.nn.Linear(3, 1)
    opt = mod.make_optimizer(args, model)
    g = opt.param_groups[0]
    assert type(opt) is TableFTRL and (g["lr"], g["l1"], g["l2"], g["beta"], g["initial_accumulator_value"]) == (0.05, 0.01, 0.002, 0.5, 0.0)
    assert mod.make_optimizer(mod.parse_args(["--optimizer", "adagrad"]), model) == "adagrad"      # without --ftrl: as before
    for argv, text in ((["--ftrl", "--optimizer", "sgd", "--momentum", "0.9"], "--ftrl does not go with --momentum / --nesterov"),
                       (["--ftrl", "--optimizer", "sgd", "--momentum", "0.9", "--nesterov"], "--ftrl does not go with"),
                       (["--ftrl", "--nesterov"], "--ftrl does not go with"),
                       (["--ftrl_l1", "0.01"], "--ftrl_l1 need(s) --ftrl"), (["--ftrl_l2", "0"], "--ftrl_l2 need(s) --ftrl"),
                       (["--ftrl_beta", "1", "--ftrl_init_acc", "0.1"], "--ftrl_beta, --ftrl_init_acc need(s) --ftrl"),
                       (["--optimizer", "adagrad", "--ftrl_init_acc", "0.1"], "need(s) --ftrl"),
                       (["--ftrl", "--ftrl_l1", "-0.01"], "--ftrl_l1 -0.01 is negative"),
                       (["--ftrl", "--ftrl_beta", "-1"], "--ftrl_beta -1 is negative"),
                       (["--ftrl", "--learning_rate", "0"], "--ftrl needs --learning_rate > 0")):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv


def test_the_optimizer_choices_did_not_change():
    src = open(os.path.join(PKG, "xdftrain_amd.py")).read()
    assert 'choices=["adam", "adagrad", "sgd", "rmsprop"]' in src
    mod = _trainer()
    with pytest.raises(SystemExit):
        mod.parse_args(["--optimizer", "ftrl"])
