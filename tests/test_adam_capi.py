"""CPU: the Adam entry points (K7 / K7d, csrc/adam.hip) are declared, bound and exported, their structs match the header,
and bad arguments are refused before any device work (host addresses stand in for device ones: nothing is dereferenced,
nothing is launched)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

ADAM = ("xdfm_adam_step_ws_elems", "xdfm_adam_step", "xdfm_adam_step_lr", "xdfm_adam_step_deferred", "xdfm_adam_catchup_rows",
        "xdfm_adam_apply_rows", "xdfm_adam_flush", "xdfm_adam_selftest")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xdfm.h")).read(), flags=re.S)


def _struct_fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    return [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


def test_adam_symbols_are_declared_bound_and_exported():
    from xdfm_amd import _lib
    lib = _lib.load()
    header = _header()
    for name in ADAM:
        assert re.search(r"\b%s\s*\(" % name, header), "include/xdfm.h lacks %s" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    exported = {n for n in _lib.SIGNATURES if n.startswith("xdfm_adam_")}
    declared = set(re.findall(r"\b(xdfm_adam_\w+)\s*\(", header))
    assert exported == declared == set(ADAM)
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9          # no signature changed


def test_adam_structs_match_the_header():
    from xdfm_amd import _lib
    header = _header()
    for cls, name, size in ((_lib.AdamTensor, "xdfm_adam_tensor", 80), (_lib.AdamClock, "xdfm_adam_clock", 24),
                            (_lib.AdamRows, "xdfm_adam_rows", 56)):
        assert [f[0] for f in cls._fields_] == _struct_fields(header, name), name
        assert ctypes.sizeof(cls) == size, name
    assert re.search(r"XDFM_ADAM_LAZY\s*=\s*1\b", header) and re.search(r"XDFM_ADAM_DEFERRED\s*=\s*2\b", header)


def test_adam_step_ws_elems():
    from xdfm_amd import _lib
    lib = _lib.load()
    assert lib.xdfm_adam_step_ws_elems(0) == 0 and lib.xdfm_adam_step_ws_elems(-5) == 0
    for T in (1, 2, 64, 65, 70, 65535):
        assert lib.xdfm_adam_step_ws_elems(T) >= T


class _Env:
    def __init__(self):
        from xdfm_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.buf = (ctypes.c_float * 64)()
        self.addr = (ctypes.addressof(self.buf) + 15) & ~15           # a 16-byte aligned stand-in for every device pointer
        self.one = (_lib.AdamTensor * 1)()
        self.arr = ctypes.cast(self.one, ctypes.c_void_p)
        self.fill()
        self.clk = _lib.AdamClock(self.addr, self.addr, 256)

    def fill(self):
        t, a = self.one[0], self.addr
        t.param = t.grad = t.exp_avg = t.exp_avg_sq = t.step = a
        t.numel, t.l2, t.grad_marks, t.flags, t.last = 8, 0.0, None, 0, None

    def refused(self, rc, text):
        msg = self.lib.xdfm_last_error()
        assert rc == 1 and text in msg, (rc, msg, text)
        with pytest.raises(ValueError):
            self._lib.check(rc, "adam")


def test_adam_step_refuses_bad_arguments_before_any_device_work():
    e = _Env()
    lib, arr, a, one, refused = e.lib, e.arr, e.addr, e.one, e.refused
    P = ctypes.c_void_p
    ok = (1e-3, None, 0.9, 0.999, 1e-8)
    step = lib.xdfm_adam_step_lr
    refused(step(None, 1, *ok, None, None, None), b"null pointer")
    refused(lib.xdfm_adam_step(None, 1, 1e-3, 0.9, 0.999, 1e-8, None, None, None), b"null pointer")
    for T in (0, -1, 65536):
        refused(step(arr, T, *ok, None, None, None), b"bad tensor count")
    for member in ("param", "grad", "exp_avg", "exp_avg_sq", "step"):
        setattr(one[0], member, None)
        refused(step(arr, 1, *ok, None, None, None), b"has a null pointer")
        e.fill()
    one[0].numel = -1
    refused(step(arr, 1, *ok, None, None, None), b"has a null pointer")
    e.fill()
    for bad in ((-1e-3, None, 0.9, 0.999, 1e-8), (1e-3, None, -0.1, 0.999, 1e-8), (1e-3, None, 1.0, 0.999, 1e-8),
                (1e-3, None, 0.9, -0.5, 1e-8), (1e-3, None, 0.9, 1.0, 1e-8), (1e-3, None, 0.9, 0.999, -1e-8)):
        refused(step(arr, 1, *bad, None, None, None), b"bad hyper-parameters")
    refused(step(arr, 1, *ok, None, P(a), None), b"l2_value needs l2_ws")
    one[0].flags = 1
    refused(step(arr, 1, *ok, None, None, None), b"lazy but has no grad_marks")
    e.fill()
    # DEFERRED: without a clock (xdfm_adam_step_lr has none), without marks, without `last`
    one[0].flags, one[0].grad_marks, one[0].last = 2, a, a
    refused(step(arr, 1, *ok, None, None, None), b"deferred but has no clock")
    ck = ctypes.byref(e.clk)
    dstep = lambda clk: lib.xdfm_adam_step_deferred(arr, 1, clk, 1e-3, None, 0.9, 0.999, 1e-8, None, None, None)
    one[0].grad_marks = None
    refused(dstep(ck), b"deferred but has no clock / grad_marks / last")
    one[0].grad_marks, one[0].last = a, None
    refused(dstep(ck), b"deferred but has no clock / grad_marks / last")
    e.fill()
    # marks with a pointer that is not 16-byte aligned
    for member in ("param", "grad", "exp_avg", "exp_avg_sq"):
        one[0].grad_marks = a
        setattr(one[0], member, a + 4)
        refused(step(arr, 1, *ok, None, None, None), b"not 16-byte aligned")
        e.fill()
    # the clock: NULL, a NULL member, cap <= 2, cap > 256 (`last` is one byte per chunk)
    refused(dstep(None), b"bad clock")
    AC = e._lib.AdamClock
    for bad in (AC(None, a, 256), AC(a, None, 256), AC(a, a, 0), AC(a, a, -7), AC(a, a, 2), AC(a, a, 257), AC(a, a, 1 << 20)):
        refused(dstep(ctypes.byref(bad)), b"bad clock")
    refused(lib.xdfm_adam_step_deferred(None, 1, ck, 1e-3, None, 0.9, 0.999, 1e-8, None, None, None), b"null pointer")
    refused(lib.xdfm_adam_step_deferred(arr, 0, ck, 1e-3, None, 0.9, 0.999, 1e-8, None, None, None), b"bad tensor count")


def test_adam_rows_and_flush_refuse_bad_arguments_before_any_device_work():
    e = _Env()
    lib, arr, a, one, refused = e.lib, e.arr, e.addr, e.one, e.refused
    P = ctypes.c_void_p
    AC, AR = e._lib.AdamClock, e._lib.AdamRows
    ck = ctypes.byref(e.clk)
    rows = AR(a, a, a, a, a, a, a)
    rb = ctypes.byref(rows)
    hp = (0.9, 0.999, 1e-8)
    catchup = lambda X=a, cols=a, vocab=a, B=4, m=1, D=4, emb=rb, lin=None, clk=ck, back=a: lib.xdfm_adam_catchup_rows(
        X, 2, B, cols, vocab, m, D, emb, lin, clk, *hp, back, None)
    apply_ = lambda X=a, cols=a, vocab=a, B=4, m=1, D=4, emb=rb, lin=None, clk=ck, cell=a, val=None: lib.xdfm_adam_apply_rows(
        X, 2, B, cols, vocab, m, D, emb, lin, clk, *hp, cell, val, None)
    for fn, name in ((catchup, b"adam_catchup_rows"), (apply_, b"adam_apply_rows")):
        for kw in (dict(X=None), dict(cols=None), dict(vocab=None), dict(emb=None), dict(clk=None)):
            refused(fn(**kw), name + b": null pointer")
        for kw in (dict(B=0), dict(m=0), dict(D=0), dict(B=-3)):
            refused(fn(**kw), name + b": bad shape")
        for bad in (AC(None, a, 256), AC(a, None, 256), AC(a, a, 2), AC(a, a, 0), AC(a, a, 257)):
            refused(fn(clk=ctypes.byref(bad)), name + b": bad clock")
    refused(catchup(back=None), b"null pointer")
    refused(apply_(cell=None), b"null pointer")
    refused(catchup(back=P(a + 4)), b"8-byte aligned")
    refused(apply_(cell=P(a + 4)), b"8-byte aligned")
    # apply: gradient / mark / last tables, of emb and of lin
    for k in (5, 6):
        vals = [a] * 7
        vals[k] = None
        bad = AR(*vals)
        refused(apply_(emb=ctypes.byref(bad)), b"gradient / mark tables missing")
        refused(apply_(lin=ctypes.byref(bad)), b"gradient / mark tables missing")
    vals = [a] * 7
    vals[3] = None
    bad = AR(*vals)
    refused(apply_(emb=ctypes.byref(bad)), b"`last` tables missing")
    refused(apply_(lin=ctypes.byref(bad)), b"`last` tables missing")
    # flush
    flush = lambda tensors=arr, T=1, clk=ck, back=a: lib.xdfm_adam_flush(tensors, T, clk, *hp, back, None)
    one[0].flags, one[0].last = 2, a
    refused(flush(tensors=None), b"null pointer")
    refused(flush(clk=None), b"null pointer")
    refused(flush(back=None), b"null pointer")
    for bad in (AC(None, a, 256), AC(a, None, 256), AC(a, a, 2), AC(a, a, 257)):
        refused(flush(clk=ctypes.byref(bad)), b"bad clock")
    for T in (0, -2, 65536):
        refused(flush(T=T), b"bad tensor count")
    refused(flush(back=P(a + 4)), b"8-byte aligned")
    for member in ("param", "exp_avg", "exp_avg_sq", "last"):
        setattr(one[0], member, None)
        refused(flush(), b"has a null pointer")
        e.fill()
        one[0].flags, one[0].last = 2, a


def test_deferred_sgd_adagrad_refuse_a_clock_of_more_than_256_steps():
    """`last` is one byte per chunk there too (csrc/sgd_adagrad_deferred.hip)."""
    from xdfm_amd import _lib
    lib = _lib.load()
    one = (_lib.OptTensor * 1)()
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15
    last = (ctypes.c_void_p * 1)()
    for cap in (257, 1 << 16):
        clk = _lib.OptClock(a, a, cap, a, a)
        rc = lib.xdfm_sgd_step_deferred(ctypes.cast(one, ctypes.c_void_p), ctypes.cast(last, ctypes.c_void_p), 1, ctypes.byref(clk),
                                        0.01, None, None, None, None)
        assert rc == 1 and b"bad clock" in lib.xdfm_last_error()
        rc = lib.xdfm_opt_flush(0, ctypes.cast(one, ctypes.c_void_p), ctypes.cast(last, ctypes.c_void_p), 1, ctypes.byref(clk), 0.0, None)
        assert rc == 1 and b"bad clock" in lib.xdfm_last_error()
