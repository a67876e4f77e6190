"""CPU: the SGD / Adagrad entry points (K7s / K7g) are declared, bound and exported, validate their arguments before any
device work, and the host classes keep the stock classes' layout and the reference's defaults (no compute)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("xdfm_opt_step_ws_elems", "xdfm_sgd_step", "xdfm_adagrad_step")


def test_new_symbols_are_declared_bound_and_exported():
    from xdfm_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), "include/xdfm.h lacks %s" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "xdfm_opt_tensor" in header
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9          # additions only
    # the descriptor as the header lays it out: three pointers, a long, a float (padded), a pointer
    assert ctypes.sizeof(_lib.OptTensor) == 48
    assert [f[0] for f in _lib.OptTensor._fields_] == ["param", "grad", "state", "numel", "l2", "grad_marks"]
    assert lib.xdfm_opt_step_ws_elems(0) == 0 and lib.xdfm_opt_step_ws_elems(3) >= 3


def test_option_opt_bx_round_trips_and_adds_no_symbol():
    """Option "opt_bx" (most blocks one tensor gets in the sweep, the deferred scan and the flush; a test knob): 0 by default,
    set / get round trip, out-of-range values are stored as given and mean the built-in caps when a call composes its
    launch; the workspace stays T * 512 floats and the family's entry points are the ones it had."""
    from xdfm_amd import _lib
    lib = _lib.load()
    assert _lib.get_option("opt_bx") == 0
    try:
        for v in (1, 7, 512, 100000, -3, 0):
            _lib.set_option("opt_bx", v)
            assert _lib.get_option("opt_bx") == v
            assert lib.xdfm_opt_step_ws_elems(3) == 3 * 512
    finally:
        _lib.set_option("opt_bx", 0)
    assert _lib.get_option("adam_bx") == 0 and _lib.get_option("no_such_option") == -1
    # an option is no ABI change: the version and the entry points of this family are what they were
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9
    assert sorted(k for k in _lib.SIGNATURES if k.startswith(("xdfm_opt_", "xdfm_sgd_", "xdfm_adagrad_", "xdfm_rmsprop_"))) == [
        "xdfm_adagrad_step", "xdfm_adagrad_step_deferred", "xdfm_opt_catchup_rows", "xdfm_opt_flush", "xdfm_opt_step_ws_elems",
        "xdfm_rmsprop_catchup_rows", "xdfm_rmsprop_flush", "xdfm_rmsprop_step", "xdfm_rmsprop_step_deferred", "xdfm_sgd_step",
        "xdfm_sgd_step_deferred"]


def test_bad_arguments_are_refused_before_any_device_work():
    from xdfm_amd import _lib
    lib = _lib.load()
    one = (_lib.OptTensor * 1)()
    arr = ctypes.cast(one, ctypes.c_void_p)

    def refused(rc, text):
        msg = lib.xdfm_last_error()
        assert rc == 1 and text in msg, (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc, "opt_step")

    refused(lib.xdfm_sgd_step(None, 1, 0.01, None, None, None, None), b"null pointer")
    refused(lib.xdfm_adagrad_step(None, 1, 0.01, None, 1e-10, None, None, None), b"null pointer")
    refused(lib.xdfm_sgd_step(arr, 0, 0.01, None, None, None, None), b"bad tensor count")
    refused(lib.xdfm_adagrad_step(arr, -2, 0.01, None, 1e-10, None, None, None), b"bad tensor count")
    refused(lib.xdfm_adagrad_step(arr, 1, 0.01, None, 0.0, None, None, None), b"bad hyper-parameters")      # eps <= 0
    refused(lib.xdfm_sgd_step(arr, 1, 0.01, None, None, None, None), b"null pointer")                       # param / grad NULL
    # Adagrad without the accumulator: host addresses stand in for device ones, nothing is dereferenced
    buf = (ctypes.c_float * 8)()
    one[0].param = one[0].grad = ctypes.addressof(buf)
    one[0].numel = 8
    refused(lib.xdfm_adagrad_step(arr, 1, 0.01, None, 1e-10, None, None, None), b"no state")
    refused(lib.xdfm_sgd_step(arr, 1, 0.01, None, None, ctypes.c_void_p(ctypes.addressof(buf)), None), b"l2_value needs l2_ws")


def test_table_optimizers_keep_the_stock_layout_and_the_reference_defaults():
    from xdfm_amd.optim import TableAdagrad, TableAdam, TableSGD
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(4))]
    sgd, ada = TableSGD(ps), TableAdagrad(ps)
    assert isinstance(sgd, torch.optim.SGD) and isinstance(ada, torch.optim.Adagrad)
    assert issubclass(TableSGD, torch.optim.SGD) and issubclass(TableAdagrad, torch.optim.Adagrad)
    g = sgd.param_groups[0]
    assert g["lr"] == 0.01 and g["momentum"] == 0 and g["weight_decay"] == 0 and not g["nesterov"]
    g = ada.param_groups[0]
    assert g["lr"] == 0.01 and g["eps"] == 1e-10 and g["lr_decay"] == 0 and g["initial_accumulator_value"] == 0
    for opt in (sgd, ada, TableAdam(ps)):
        assert opt.table_step and opt.generation == 0 and opt.l2_value is None and opt.owns(ps)
        assert not opt.owns([torch.nn.Parameter(torch.zeros(1))])
    assert sorted(ada.state[ps[0]].keys()) == ["step", "sum"] and not ada.state[ps[0]]["step"].is_cuda
    # CPU parameters: the stock update (with an armed L2 term applied by hand), bit for bit
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for mine, stock in ((TableSGD(ps), torch.optim.SGD(qs, lr=0.01)), (TableAdagrad(ps), torch.optim.Adagrad(qs))):
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
        gen = mine.generation
        stock.load_state_dict(mine.state_dict())             # interchangeable state
        mine.load_state_dict(stock.state_dict())
        assert mine.generation > gen                         # captured graphs that baked the old state are stale
    assert float(ada.state[ps[0]]["step"]) == 0.0 and float(mine.state[ps[0]]["step"]) == 3.0


def test_cpu_model_compiles_the_stock_classes():
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C1", 7, 4), SparseFeat("C2", 5, 4), DenseFeat("I1", 1)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), device="cpu")
    for name, cls, lr in (("sgd", torch.optim.SGD, 0.01), ("adagrad", torch.optim.Adagrad, 0.01)):
        model.compile(name, "binary_crossentropy")
        assert type(model.optim) is cls and model.optim.param_groups[0]["lr"] == lr
        assert not model._optim_capturable and model._l2_fusion() is None


def test_launch_order_and_grid_composer_under_the_host_sanitizers(tmp_path):
    """csrc/table_step.h's host side (the size-sorted round-robin launch order and the first[] grid composer that the Adam,
    SGD / Adagrad / RMSprop and deferred launchers share) in a stand-alone program, tests/table_step_host.hip, built with
    AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run on the CPU: T = 1, 63, 64, 65, 130 tensors of
    0, 1, 8191, 8192, 8193 and 10^9 elements; first[] monotone, 1 <= blocks <= cap per tensor, and everything equal to the
    loops the launchers spelled out before.  Nothing loaded into Python is sanitized."""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "table_step_host")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "table_step_host.hip"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "table_step_host ok: 270 cases" in run.stdout, (run.returncode, run.stdout, run.stderr)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
