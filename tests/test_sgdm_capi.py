"""CPU: the entry points of SGD with momentum (K7m / K7md) are declared, bound and exported and validate their arguments
before any device work, with the offending value in the message; TableSGD's truth table of what its kernels take; the host
class keeps torch.optim.SGD's layout and defaults; the trainer's flags; the sgdm goldens exist, no other golden test picks them
up, and the oracle with torch.optim.SGD(momentum=...) reproduces them (no GPU compute)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT, golden_names, load_golden

T = torch.from_numpy
NEW = ("xdfm_sgdm_step", "xdfm_sgdm_step_deferred", "xdfm_sgdm_catchup_rows", "xdfm_sgdm_flush")
VARIANTS = {"mom": False, "nes": True}


def test_new_symbols_are_declared_bound_and_exported():
    from xdfm_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "xdfm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), "include/xdfm.h lacks %s" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "xdfm_sgdm_step, xdfm_sgdm_step_deferred, xdfm_sgdm_catchup_rows, xdfm_sgdm_flush" in text      # the ABI note
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9          # additions only
    assert ctypes.sizeof(_lib.OptTensor) == 48
    # the existing signatures did not change
    assert len(_lib.SIGNATURES["xdfm_sgd_step"][1]) == 7 and len(_lib.SIGNATURES["xdfm_rmsprop_step"][1]) == 9
    assert len(_lib.SIGNATURES["xdfm_sgd_step_deferred"][1]) == 9 and len(_lib.SIGNATURES["xdfm_opt_flush"][1]) == 7
    assert len(_lib.SIGNATURES["xdfm_sgdm_step"][1]) == 9 and len(_lib.SIGNATURES["xdfm_sgdm_step_deferred"][1]) == 11
    assert len(_lib.SIGNATURES["xdfm_sgdm_catchup_rows"][1]) == 13 and len(_lib.SIGNATURES["xdfm_sgdm_flush"][1]) == 7


def test_bad_arguments_are_refused_before_any_device_work():
    from xdfm_amd import _lib
    lib = _lib.load()
    one = (_lib.OptTensor * 1)()
    arr = ctypes.cast(one, ctypes.c_void_p)
    last = (ctypes.c_void_p * 1)()
    lasts = ctypes.cast(last, ctypes.c_void_p)
    buf = (ctypes.c_float * 16)()
    base = (ctypes.addressof(buf) + 15) & ~15                # a 16-byte aligned host address: never dereferenced
    host = ctypes.c_void_p(base)
    cell = (ctypes.c_ulonglong * 2)()
    clk = _lib.OptClock(base, base, 256, ctypes.addressof(cell), ctypes.addressof(cell) + 8)
    nan = float("nan")

    def refused(rc, *texts):
        msg = lib.xdfm_last_error()
        assert rc == 1 and all(t in msg for t in texts), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc, "sgdm")

    # the sweep
    refused(lib.xdfm_sgdm_step(None, 1, 0.01, None, 0.9, 0, None, None, None), b"null pointer")
    refused(lib.xdfm_sgdm_step(arr, 0, 0.01, None, 0.9, 0, None, None, None), b"bad tensor count 0")
    refused(lib.xdfm_sgdm_step(arr, -2, 0.01, None, 0.9, 1, None, None, None), b"bad tensor count -2")
    refused(lib.xdfm_sgdm_step(arr, 1, -0.01, None, 0.9, 0, None, None, None), b"bad hyper-parameters")
    for mu, shown in ((0.0, b"momentum 0 "), (1.0, b"momentum 1 "), (-0.1, b"momentum -0.1 "), (1.5, b"momentum 1.5 "), (nan, b"nan")):
        refused(lib.xdfm_sgdm_step(arr, 1, 0.01, None, mu, 0, None, None, None), b"outside (0, 1)", shown)
    refused(lib.xdfm_sgdm_step(arr, 1, 0.01, None, 0.9, 0, None, None, None), b"null pointer")             # param / grad NULL
    one[0].param = one[0].grad = base
    one[0].numel = 8
    refused(lib.xdfm_sgdm_step(arr, 1, 0.01, None, 0.9, 1, None, None, None), b"tensor 0 has no state")
    one[0].state = base + 2
    refused(lib.xdfm_sgdm_step(arr, 1, 0.01, None, 0.9, 1, None, None, None), b"misaligned state", b"%x" % (base + 2))
    one[0].state, one[0].grad_marks = base + 4, base
    refused(lib.xdfm_sgdm_step(arr, 1, 0.01, None, 0.9, 1, None, None, None), b"grad_marks but a pointer that is not 16-byte aligned")
    one[0].state, one[0].grad_marks = base, None
    refused(lib.xdfm_sgdm_step(arr, 1, 0.01, None, 0.9, 0, None, host, None), b"l2_value needs l2_ws")
    one[0].state = None
    # the deferred step
    refused(lib.xdfm_sgdm_step_deferred(None, lasts, 1, ctypes.byref(clk), 0.01, None, 0.9, 0, None, None, None), b"null pointer")
    refused(lib.xdfm_sgdm_step_deferred(arr, None, 1, ctypes.byref(clk), 0.01, None, 0.9, 0, None, None, None), b"null pointer")
    refused(lib.xdfm_sgdm_step_deferred(arr, lasts, 0, ctypes.byref(clk), 0.01, None, 0.9, 0, None, None, None), b"bad tensor count")
    refused(lib.xdfm_sgdm_step_deferred(arr, lasts, 1, None, 0.01, None, 0.9, 0, None, None, None), b"bad clock")
    refused(lib.xdfm_sgdm_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 1.0, 0, None, None, None), b"momentum 1 is outside (0, 1)")
    refused(lib.xdfm_sgdm_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 0.9, 0, None, None, None), b"no state")
    one[0].state = base + 1
    refused(lib.xdfm_sgdm_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 0.9, 0, None, None, None), b"misaligned state")
    one[0].state, last[0] = base, base
    refused(lib.xdfm_sgdm_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 0.9, 0, None, None, None), b"deferred but has no grad_marks")
    one[0].grad_marks = base
    refused(lib.xdfm_sgdm_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 0.9, 0, None, None, None), b"deferred but has no L2 term")
    one[0].grad_marks, one[0].state, last[0] = None, None, None
    refused(lib.xdfm_sgdm_step_deferred(arr, lasts, 1, ctypes.byref(clk), 0.01, None, 0.9, 0, None, host, None), b"l2_value needs l2_ws")
    # the flush
    refused(lib.xdfm_sgdm_flush(None, lasts, 1, ctypes.byref(clk), 0.9, 0, None), b"null pointer")
    refused(lib.xdfm_sgdm_flush(arr, lasts, 70000, ctypes.byref(clk), 0.9, 0, None), b"bad tensor count 70000")
    refused(lib.xdfm_sgdm_flush(arr, lasts, 1, ctypes.byref(clk), nan, 0, None), b"outside (0, 1)")
    refused(lib.xdfm_sgdm_flush(arr, lasts, 1, ctypes.byref(clk), 0.0, 1, None), b"momentum 0 is outside (0, 1)")
    refused(lib.xdfm_sgdm_flush(arr, lasts, 1, ctypes.byref(clk), 0.9, 0, None), b"has no last")
    last[0] = base
    refused(lib.xdfm_sgdm_flush(arr, lasts, 1, ctypes.byref(clk), 0.9, 0, None), b"no state")
    one[0].state = base + 4
    refused(lib.xdfm_sgdm_flush(arr, lasts, 1, ctypes.byref(clk), 0.9, 0, None), b"not 16-byte aligned")
    # the catch-up
    rows = _lib.OptRows(base, None, base, base)
    full = _lib.OptRows(base, base, base, base)
    args = (host, 4, 2, host, host, 1, 4)
    refused(lib.xdfm_sgdm_catchup_rows(None, 4, 2, host, host, 1, 4, ctypes.byref(full), None, ctypes.byref(clk), 0.9, 0, None), b"null pointer")
    refused(lib.xdfm_sgdm_catchup_rows(*(args + (ctypes.byref(full), None, None, 0.9, 0, None))), b"bad clock")
    refused(lib.xdfm_sgdm_catchup_rows(host, 4, 0, host, host, 1, 4, ctypes.byref(full), None, ctypes.byref(clk), 0.9, 0, None), b"bad shape B=0")
    refused(lib.xdfm_sgdm_catchup_rows(*(args + (ctypes.byref(rows), None, ctypes.byref(clk), 0.9, 1, None))), b"needs state")
    refused(lib.xdfm_sgdm_catchup_rows(*(args + (ctypes.byref(full), ctypes.byref(rows), ctypes.byref(clk), 0.9, 1, None))), b"needs state")
    refused(lib.xdfm_sgdm_catchup_rows(*(args + (ctypes.byref(full), None, ctypes.byref(clk), 1.0, 0, None))), b"momentum 1 is outside (0, 1)")


def test_plain_is_a_truth_table(monkeypatch):
    from xdfm_amd import optim
    ps = [torch.nn.Parameter(torch.randn(5, 3))]
    g = optim.TableSGD(ps, lr=0.01).param_groups[0]
    table = [  # momentum, dampening, nesterov -> the kernel, or None for the stock step
        (0, 0, False, "sgd"), (0.0, 0, False, "sgd"), (0, 0.1, False, None), (0, 0, True, None),
        (0.9, 0, False, "sgdm"), (0.9, 0, True, "sgdm"), (0.5, 0.0, True, "sgdm"), (1e-3, 0, False, "sgdm"),
        (0.9, 0.1, False, None), (0.9, 0.1, True, None), (1.0, 0, False, None), (1.5, 0, False, None), (-0.5, 0, False, None),
        (torch.tensor(0.9), 0, False, None),
    ]
    opt = optim.TableSGD(ps, lr=0.01)
    assert optim.SGD_MOMENTUM_NATIVE is True and opt._KERNEL == "sgd"
    for mu, damp, nes, kernel in table:
        grp = dict(g, momentum=mu, dampening=damp, nesterov=nes)
        assert bool(opt._plain(grp)) == (kernel is not None), (mu, damp, nes)
        if kernel:
            assert opt._kind(grp) == kernel
            assert opt._hyper(grp) == (None if kernel == "sgd" else (float(mu), nes))
    monkeypatch.setattr(optim, "SGD_MOMENTUM_NATIVE", False)       # the switch: momentum 0 keeps its kernel, the rest falls back
    for mu, damp, nes, kernel in table:
        assert bool(opt._plain(dict(g, momentum=mu, dampening=damp, nesterov=nes))) == (kernel == "sgd"), (mu, damp, nes)
    monkeypatch.undo()
    for key, val in (("weight_decay", 0.1), ("maximize", True), ("differentiable", True), ("lr", torch.tensor(0.01))):
        mom = optim.TableSGD(ps, lr=0.01, momentum=0.9)
        mom.param_groups[0][key] = val
        assert not mom._native(), key
    # the momentum-0 class is what it was
    assert opt._state_of(opt.param_groups[0], ps[0]) == (None, None) and opt._hyper(opt.param_groups[0]) is None


def test_the_switch_is_read_from_the_environment_at_import():
    import subprocess
    import sys
    code = "import sys; sys.path.insert(0, %r); from xdfm_amd import optim; print(optim.SGD_MOMENTUM_NATIVE)" % PKG
    for value, want in (("0", "False"), ("1", "True"), (None, "True")):
        env = {k: v for k, v in os.environ.items() if k != "XDFM_SGD_MOMENTUM_NATIVE"}
        if value is not None:
            env["XDFM_SGD_MOMENTUM_NATIVE"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)


@pytest.mark.parametrize("nesterov", [False, True])
def test_table_sgd_keeps_the_stock_layout_and_torchs_defaults(nesterov):
    from xdfm_amd.optim import TableSGD
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(4))]
    kw = dict(lr=0.01, momentum=0.9, nesterov=nesterov)
    opt = TableSGD(ps, **kw)
    ref = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], **kw)
    g, gr = opt.param_groups[0], ref.param_groups[0]
    assert issubclass(TableSGD, torch.optim.SGD)
    assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in gr.items() if k != "params"}
    assert opt.table_step and opt.generation == 0 and opt.owns(ps) and opt._plain(g) and opt._kind(g) == "sgdm"
    # CPU parameters: the stock update (with an armed L2 term applied by hand), bit for bit, and the stock state
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    mine, stock = TableSGD(ps, **kw), torch.optim.SGD(qs, **kw)
    for step in range(3):
        for p, q in zip(ps, qs):
            p.grad = torch.full_like(p, 0.5 + step)
            q.grad = p.grad.clone()
        if step == 1:
            mine.arm_l2(ps[:1], [0.25])
            want = 0.25 * float(qs[0].detach().square().sum())
            qs[0].grad.add_(qs[0].detach(), alpha=0.5)
        mine.step()
        stock.step()
        assert (mine.l2_value is None) == (step != 1)
        if step == 1:
            assert abs(float(mine.l2_value) - want) <= 1e-6 * want
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
        assert sorted(mine.state[p].keys()) == sorted(stock.state[q].keys()) == ["momentum_buffer"]
        assert torch.equal(mine.state[p]["momentum_buffer"], stock.state[q]["momentum_buffer"])
    sd_mine, sd_stock = mine.state_dict(), stock.state_dict()
    assert sd_mine["param_groups"] == sd_stock["param_groups"]
    assert sorted(sd_mine["state"].keys()) == sorted(sd_stock["state"].keys())
    gen = mine.generation
    stock.load_state_dict(sd_mine)                       # interchangeable state, both ways
    mine.load_state_dict(stock.state_dict())
    assert mine.generation > gen                         # captured graphs that baked the old state are stale
    assert torch.equal(mine.state[ps[0]]["momentum_buffer"], stock.state[qs[0]]["momentum_buffer"])
    # a torch checkpoint saved before any step has no buffers; one that says None counts as absent
    fresh = TableSGD([torch.nn.Parameter(torch.randn(3))], **kw)
    fresh.load_state_dict(torch.optim.SGD([torch.nn.Parameter(torch.randn(3))], **kw).state_dict())
    assert len(fresh.state) == 0
    fresh.state[fresh.param_groups[0]["params"][0]]["momentum_buffer"] = None
    p0 = fresh.param_groups[0]["params"][0]
    p0.grad = torch.ones_like(p0)
    fresh.step()                                         # CPU: the stock step, which also takes None as absent
    assert torch.equal(fresh.state[p0]["momentum_buffer"], torch.ones(3))


def test_cpu_model_compiles_the_stock_class():
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C1", 7, 4), SparseFeat("C2", 5, 4), DenseFeat("I1", 1)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), device="cpu")
    stock = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, nesterov=True)
    model.compile(stock, "binary_crossentropy")
    assert model.optim is stock and type(model.optim) is torch.optim.SGD
    assert not model._optim_capturable and model._l2_fusion() is None
    model.compile("sgd", "binary_crossentropy")          # the string did not change
    assert type(model.optim) is torch.optim.SGD and model.optim.param_groups[0]["momentum"] == 0


def _trainer():
    import importlib.util
    spec = importlib.util.spec_from_file_location("xdftrain_amd", os.path.join(PKG, "xdftrain_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_accepts_and_refuses_the_new_flags(capsys):
    mod = _trainer()
    args = mod.parse_args(["--optimizer", "sgd", "--momentum", "0.9", "--nesterov"])
    assert args.momentum == 0.9 and args.nesterov is True
    args = mod.parse_args(["--optimizer", "sgd"])
    assert args.momentum == 0.0 and args.nesterov is False
    assert mod.parse_args([]).momentum == 0.0
    for argv, text in ((["--momentum", "0.9"], "need --optimizer sgd"), (["--optimizer", "adagrad", "--nesterov"], "need --optimizer sgd"),
                       (["--optimizer", "rmsprop", "--momentum", "0.5"], "need --optimizer sgd"),
                       (["--optimizer", "sgd", "--momentum", "1.0"], "outside [0, 1)"), (["--optimizer", "sgd", "--momentum", "-0.1"], "outside [0, 1)"),
                       (["--optimizer", "sgd", "--nesterov"], "--nesterov needs --momentum")):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
    # what compile() is handed: the name, or on the CPU the stock object
    model = torch.nn.Linear(3, 1)
    assert mod.make_optimizer(mod.parse_args(["--optimizer", "sgd"]), model) == "sgd"
    assert mod.make_optimizer(mod.parse_args(["--optimizer", "adagrad"]), model) == "adagrad"
    opt = mod.make_optimizer(mod.parse_args(["--optimizer", "sgd", "--momentum", "0.5", "--nesterov"]), model)
    grp = opt.param_groups[0]
    assert type(opt) is torch.optim.SGD and grp["momentum"] == 0.5 and grp["nesterov"] is True and grp["dampening"] == 0


def test_sgdm_goldens_exist_and_no_other_golden_test_picks_them_up():
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "sgdm", "*")))
    assert files == ["sgdm_sum_small_%s.npz" % v for v in sorted(VARIANTS)]
    # the golden tests glob tests/golden/<prefix>*.npz: nothing of this pull request's lies there, under any prefix
    assert not [n for n in golden_names("") if "sgdm" in n]
    for prefix in ("optim_", "model_", "rms_", "rms64_", "cin_", "attn_", "pro_"):
        assert not [n for n in golden_names(prefix) if "sgdm" in n]
    for v, nesterov in VARIANTS.items():
        g = load_golden(os.path.join("sgdm", "sgdm_sum_small_" + v))
        assert str(g["optim_class"]) == "SGD" and str(g["base"]) == "model_sum_small" and str(g["cls"]) == "xDeepFM"
        assert float(g["lr"]) == 1e-4 and float(g["momentum"]) == 0.9 and bool(g["nesterov"]) == nesterov
        assert 0.0 < float(g["bar_share_32_vs_64"]) < 1.0
        assert any(k.startswith("buf3:") for k in g) and any(k.startswith("s3:") for k in g)


def _spec(g):
    vocab = [int(v) for v in g["vocab"]]
    from oracle import xdeepfm_oracle as orc
    return orc.Spec(["C%d" % (i + 1) for i in range(len(vocab))], vocab, ["I%d" % (i + 1) for i in range(int(g["n_dense"]))],
                    int(g["emb_dim"]), tuple(int(v) for v in g["cin"]), True, "relu", tuple(int(v) for v in g["dnn"]),
                    "sum", 4, True, True, 1, l2_reg_dnn=1e-5)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_oracle_with_torch_sgd_momentum_reproduces_the_golden(variant):
    """The oracle's forward and backward, torch.optim.SGD at the recorded rate, momentum and variant, three steps as
    BaseModel.fit does them: losses rtol 2e-5, parameters and momentum buffers rtol 1e-3 / atol 2e-5 against the reference's
    fp32 run, every element; the reference's own fp64 run lies within the same bars of its fp32 run."""
    from oracle import xdeepfm_oracle as orc
    g = load_golden(os.path.join("sgdm", "sgdm_sum_small_" + variant))
    base = load_golden(str(g["base"]))
    spec, B = _spec(g), int(g["B"])
    X, y = T(base["X"]), T(base["y"])
    st = {k[3:]: T(v.copy()).requires_grad_(True) for k, v in base.items() if k.startswith("s0:")}
    opt = torch.optim.SGD(list(st.values()), lr=float(g["lr"]), momentum=float(g["momentum"]), nesterov=bool(g["nesterov"]))
    log = []
    for s in range(3):
        tot, dl, _ = orc.total_loss(X[s * B:(s + 1) * B], y[s * B:(s + 1) * B], st, spec)
        opt.zero_grad()
        tot.backward()
        opt.step()
        log.append((float(dl.item()), float(tot.item())))
    np.testing.assert_allclose(np.array(log), g["losses3"], rtol=2e-5)
    worst = 0.0
    for k, v in st.items():
        for got, want, wide in ((v.detach().numpy(), g["s3:" + k], g["s3_64_minus_s3:" + k]),
                                (opt.state[v]["momentum_buffer"].numpy(), g["buf3:" + k], g["buf3_64_minus_buf3:" + k])):
            if want.size:
                worst = max(worst, float((np.abs(got - want) / (2e-5 + 1e-3 * np.abs(want))).max()))
            np.testing.assert_allclose(got, want, rtol=1e-3, atol=2e-5, err_msg=k)
            np.testing.assert_allclose(want, want.astype(np.float64) + wide.astype(np.float64), rtol=1e-3, atol=2e-5,
                                       err_msg="fp32 against fp64 reference run: " + k)
    print("sgdm %s: oracle + torch.optim.SGD against the golden, worst share of the bar %.4f" % (variant, worst))
