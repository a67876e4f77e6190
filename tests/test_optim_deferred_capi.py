"""CPU: the deferred SGD / Adagrad entry points (K7sd / K7gd) are declared, bound and exported, validate their arguments
before any device work, and the host classes accept `deferred` / `flush_every` without changing anything on CPU parameters
(no compute on a device)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("xdfm_sgd_step_deferred", "xdfm_adagrad_step_deferred", "xdfm_opt_catchup_rows", "xdfm_opt_flush")


def test_new_symbols_are_declared_bound_and_exported():
    from xdfm_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), "include/xdfm.h lacks %s" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "xdfm_opt_clock" in header and "xdfm_opt_rows" in header
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9          # additions only
    assert ctypes.sizeof(_lib.OptTensor) == 48                      # `last` travels in a parallel array
    assert [f[0] for f in _lib.OptTensor._fields_] == ["param", "grad", "state", "numel", "l2", "grad_marks"]
    assert [f[0] for f in _lib.OptClock._fields_] == ["clock", "rates", "cap", "backlog", "cell"]
    assert ctypes.sizeof(_lib.OptClock) == 40 and ctypes.sizeof(_lib.OptRows) == 32


def test_bad_arguments_are_refused_before_any_device_work():
    """Host addresses stand in for device ones: nothing is dereferenced, nothing is launched."""
    from xdfm_amd import _lib
    lib = _lib.load()
    one = (_lib.OptTensor * 1)()
    arr = ctypes.cast(one, ctypes.c_void_p)
    buf = (ctypes.c_float * 64)()                       # 16-byte aligned stand-in
    addr = (ctypes.addressof(buf) + 15) & ~15
    last = (ctypes.c_void_p * 1)()
    lasts = ctypes.cast(last, ctypes.c_void_p)
    clk = _lib.OptClock(addr, addr, 256, addr, addr)
    ck = ctypes.byref(clk)

    def refused(rc, text):
        msg = lib.xdfm_last_error()
        assert rc == 1 and text in msg, (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc, "opt_deferred")

    sgd, ada, flush, rows = lib.xdfm_sgd_step_deferred, lib.xdfm_adagrad_step_deferred, lib.xdfm_opt_flush, lib.xdfm_opt_catchup_rows
    # NULL descriptors
    refused(sgd(None, lasts, 1, ck, 0.01, None, None, None, None), b"null pointer")
    refused(sgd(arr, None, 1, ck, 0.01, None, None, None, None), b"null pointer")
    refused(ada(None, lasts, 1, ck, 0.01, None, 1e-10, None, None, None), b"null pointer")
    refused(flush(0, None, lasts, 1, ck, 0.0, None), b"null pointer")
    refused(flush(1, arr, None, 1, ck, 1e-10, None), b"null pointer")
    # T <= 0
    refused(sgd(arr, lasts, 0, ck, 0.01, None, None, None, None), b"bad tensor count")
    refused(ada(arr, lasts, -3, ck, 0.01, None, 1e-10, None, None, None), b"bad tensor count")
    refused(flush(0, arr, lasts, 0, ck, 0.0, None), b"bad tensor count")
    # the clock: NULL, a NULL member, cap <= 0
    refused(sgd(arr, lasts, 1, None, 0.01, None, None, None, None), b"bad clock")
    refused(flush(0, arr, lasts, 1, None, 0.0, None), b"bad clock")
    for bad in (_lib.OptClock(None, addr, 256, addr, addr), _lib.OptClock(addr, None, 256, addr, addr),
                _lib.OptClock(addr, addr, 256, None, addr), _lib.OptClock(addr, addr, 256, addr, None),
                _lib.OptClock(addr, addr, 0, addr, addr), _lib.OptClock(addr, addr, -1, addr, addr),
                _lib.OptClock(addr, addr, 1, addr, addr), _lib.OptClock(addr, addr, 2, addr, addr)):      # the header: cap <= 2
        refused(sgd(arr, lasts, 1, ctypes.byref(bad), 0.01, None, None, None, None), b"bad clock")
        refused(flush(0, arr, lasts, 1, ctypes.byref(bad), 0.0, None), b"bad clock")
    # eps <= 0 (Adagrad)
    refused(ada(arr, lasts, 1, ck, 0.01, None, 0.0, None, None, None), b"bad hyper-parameters")
    refused(flush(1, arr, lasts, 1, ck, 0.0, None), b"bad hyper-parameters")
    # param / grad NULL
    refused(sgd(arr, lasts, 1, ck, 0.01, None, None, None, None), b"null pointer")
    one[0].param = one[0].grad = addr
    one[0].numel = 8
    # Adagrad without the accumulator
    refused(ada(arr, lasts, 1, ck, 0.01, None, 1e-10, None, None, None), b"no state")
    last[0] = addr
    refused(flush(1, arr, lasts, 1, ck, 1e-10, None), b"no state")
    # a deferred tensor (last given) without marks, then without an L2 term
    one[0].l2 = 1e-5
    refused(sgd(arr, lasts, 1, ck, 0.01, None, None, None, None), b"no grad_marks")
    one[0].grad_marks = addr
    one[0].l2 = 0.0
    refused(sgd(arr, lasts, 1, ck, 0.01, None, None, None, None), b"no L2 term")
    one[0].l2 = 1e-5
    one[0].param = addr + 4
    refused(sgd(arr, lasts, 1, ck, 0.01, None, None, None, None), b"aligned")
    one[0].param = addr
    refused(sgd(arr, lasts, 1, ck, 0.01, None, None, ctypes.c_void_p(addr), None), b"l2_value needs l2_ws")
    # the flush takes deferred tensors only
    last[0] = None
    refused(flush(0, arr, lasts, 1, ck, 0.0, None), b"no last")
    # catch-up: NULL tables, bad shapes, Adagrad without state / eps
    r = _lib.OptRows(addr, None, addr, addr)
    rb = ctypes.byref(r)
    refused(rows(0, None, 4, 2, addr, addr, 1, 4, rb, None, ck, 0.0, None), b"null pointer")
    refused(rows(0, addr, 4, 2, addr, addr, 1, 4, None, None, ck, 0.0, None), b"null pointer")
    refused(rows(0, addr, 4, 2, addr, addr, 1, 4, rb, None, None, 0.0, None), b"bad clock")
    refused(rows(0, addr, 4, 0, addr, addr, 1, 4, rb, None, ck, 0.0, None), b"bad shape")
    refused(rows(0, addr, 4, 2, addr, addr, 1, 0, rb, None, ck, 0.0, None), b"bad shape")
    refused(rows(1, addr, 4, 2, addr, addr, 1, 4, rb, None, ck, 1e-10, None), b"Adagrad needs state")
    refused(rows(1, addr, 4, 2, addr, addr, 1, 4, rb, None, ck, 0.0, None), b"Adagrad needs state")
    empty = _lib.OptRows(None, None, addr, addr)
    refused(rows(0, addr, 4, 2, addr, addr, 1, 4, ctypes.byref(empty), None, ck, 0.0, None), b"row table is missing")


def test_constructor_arguments_and_environment(monkeypatch):
    from xdfm_amd import optim
    from xdfm_amd.optim import TableAdagrad, TableSGD
    ps = [torch.nn.Parameter(torch.randn(5, 3))]
    assert optim.OPT_DEFER_MIN_NUMEL >= optim.DEFER_MIN_NUMEL >= 1 << 26       # never below Adam's floor
    for cls in (TableSGD, TableAdagrad):
        monkeypatch.delenv("XDFM_OPT_DEFERRED", raising=False)
        monkeypatch.delenv("XDFM_OPT_FLUSH_EVERY", raising=False)
        o = cls(ps)
        assert o.deferred == "auto" and o.flush_every == 64 and o.path_counts == {"scan": 0}
        assert cls(ps, deferred=True).deferred is True and cls(ps, deferred=False).deferred is False
        assert cls(ps, deferred="auto").deferred == "auto"
        assert cls(ps, flush_every=7).flush_every == 7 and cls(ps, flush_every=10 ** 6).flush_every == 248
        monkeypatch.setenv("XDFM_OPT_DEFERRED", "1")
        assert cls(ps).deferred is True and cls(ps, deferred=False).deferred is False
        monkeypatch.setenv("XDFM_OPT_DEFERRED", "0")
        assert cls(ps).deferred is False
        monkeypatch.setenv("XDFM_OPT_FLUSH_EVERY", "12")
        assert cls(ps).flush_every == 12


SHARED = ("sync_lr", "load_state_dict", "add_param_group", "_invalidate", "_last_bytes", "take_backlog", "note_replay", "owns",
          "arm_l2", "_l2_by_hand", "__getstate__", "__setstate__", "_drop_deferred", "_table_init", "flush")


def test_table_adam_host_contract_and_the_one_scaffold_of_the_four_classes(monkeypatch):
    """TableAdam's counterpart of the two tests around it, on two CPU parameters (no compute on a device): constructor
    arguments and environment, the hooks the model calls without deferred state, `generation`, the stock state layout, a
    pickle round trip, and the refusal of CPU parameters by the native step.  Then the structure: the host scaffold has one
    definition, `_TableStep`'s, for all four classes."""
    import pickle
    from xdfm_amd import optim
    from xdfm_amd.optim import TableAdagrad, TableAdam, TableRMSprop, TableSGD, _TableStep
    for env in ("XDFM_ADAM_DEFERRED", "XDFM_ADAM_FLUSH_EVERY"):
        monkeypatch.delenv(env, raising=False)
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(4))]
    o = TableAdam(ps)
    assert o.deferred == "auto" and o.flush_every == 64 and o.lazy_rows is False and o.table_step is True
    assert o.path_counts == {"rows": 0, "scan": 0} and o._def is None and o._since == 0
    assert TableAdam(ps, deferred=True).deferred is True and TableAdam(ps, deferred=False).deferred is False
    assert TableAdam(ps, flush_every=7).flush_every == 7 and TableAdam(ps, flush_every=10 ** 6).flush_every == 248
    monkeypatch.setenv("XDFM_ADAM_FLUSH_EVERY", "12")
    assert TableAdam(ps).flush_every == 12
    monkeypatch.setenv("XDFM_OPT_FLUSH_EVERY", "9")              # the other family's variable is not Adam's
    assert TableAdam(ps).flush_every == 12 and TableSGD(ps).flush_every == 9
    monkeypatch.delenv("XDFM_ADAM_FLUSH_EVERY")
    monkeypatch.setenv("XDFM_ADAM_DEFERRED", "1")
    assert TableAdam(ps).deferred is True and TableAdam(ps, deferred=False).deferred is False and TableSGD(ps).deferred == "auto"
    monkeypatch.setenv("XDFM_ADAM_DEFERRED", "0")
    assert TableAdam(ps).deferred is False
    monkeypatch.delenv("XDFM_ADAM_DEFERRED")

    mine = TableAdam(ps, lazy_rows=True, deferred=True, flush_every=3)
    assert mine.owns(ps) and not mine.owns([torch.nn.Parameter(torch.zeros(2))])
    mine.arm_l2([ps[0], ps[1], ps[0]], [0.25, 0.5, 0.125])       # a tensor named twice: its coefficients add
    assert mine._armed == {id(ps[0]): 0.375, id(ps[1]): 0.5}
    mine._armed = None
    mine.flush()                                                 # no deferred state: the model's hooks are no-ops
    assert mine.take_backlog() == 0.0
    mine.note_replay()
    assert mine._def is None and mine._since == 0 and mine.path_counts == {"rows": 0, "scan": 0}
    stock = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], fused=True, capturable=True)
    sd = mine.state_dict()
    assert sorted(sd.keys()) == sorted(stock.state_dict().keys())
    assert [sorted(g.keys()) for g in sd["param_groups"]] == [sorted(g.keys()) for g in stock.state_dict()["param_groups"]]
    gen = mine.generation
    mine.load_state_dict(sd)
    assert mine.generation > gen
    gen = mine.generation
    extra = torch.nn.Parameter(torch.randn(2, 2))
    mine.add_param_group({"params": [extra]})
    assert mine.generation > gen and mine.owns([extra]) and len(mine.param_groups) == 2
    twin = pickle.loads(pickle.dumps(mine))
    assert twin.deferred is True and twin.flush_every == 3 and twin.lazy_rows is True
    assert twin._def is None and twin._since == 0 and twin._desc == {} and twin.grad_sources == []
    for p in ps:                                                 # native-eligible hyper-parameters, CPU tensors: an error, no fall-back
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="xdfm TableAdam: parameters and gradients must be contiguous fp32 CUDA tensors"):
        mine.step()

    for cls in (TableAdam, TableSGD, TableAdagrad, TableRMSprop):
        assert cls.__mro__[1] is _TableStep
        for name in SHARED:
            assert getattr(cls, name) is getattr(_TableStep, name), "%s.%s is not _TableStep's" % (cls.__name__, name)
    assert [n for n in SHARED if n in vars(optim.TableAdam)] == []


def test_deferred_classes_take_the_stock_update_on_cpu_parameters():
    """`deferred=True` changes nothing where the native step does not run: bit for bit the stock classes, and the hooks
    the model calls (`flush`, `take_backlog`, `note_replay`) are harmless no-ops; the state layout stays the stock one."""
    import pickle
    from xdfm_amd.optim import TableAdagrad, TableSGD
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(4))]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for mine, stock in ((TableSGD(ps, deferred=True, flush_every=3), torch.optim.SGD(qs, lr=0.01)),
                        (TableAdagrad(ps, deferred=True, flush_every=3), torch.optim.Adagrad(qs))):
        for step in range(5):
            for p, q in zip(ps, qs):
                p.grad = torch.full_like(p, 0.5 + step)
                q.grad = p.grad.clone()
            if step % 2:
                mine.arm_l2(ps[:1], [0.25])
                qs[0].grad.add_(qs[0].detach(), alpha=0.5)
            mine.step()
            stock.step()
            mine.flush()
            assert mine.take_backlog() == 0.0
            mine.note_replay()
        for p, q in zip(ps, qs):
            assert torch.equal(p, q)
        assert mine._def is None and mine.path_counts == {"scan": 0}
        sd = mine.state_dict()
        assert sorted(sd.keys()) == sorted(stock.state_dict().keys())
        assert [sorted(g.keys()) for g in sd["param_groups"]] == [sorted(g.keys()) for g in stock.state_dict()["param_groups"]]
        stock.load_state_dict(sd)                            # interchangeable state: nothing of the deferral is in it
        mine.load_state_dict(stock.state_dict())
        twin = pickle.loads(pickle.dumps(mine))
        assert twin.deferred is True and twin.flush_every == 3 and twin._def is None and twin._since == 0
