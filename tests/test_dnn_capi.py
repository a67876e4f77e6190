"""CPU: the C ABI of the native dense layer (csrc/dnn.hip) -- symbols, the supported envelope, the workspace query and
argument validation before any device work -- and the host-side routing of ops.dense / ops.dense_relu that needs no GPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "xdfm.h")
NAMES = ["xdfm_dense_supported", "xdfm_dense_bwd_w_ws_elems", "xdfm_dense_fwd", "xdfm_dense_bwd_x", "xdfm_dense_bwd_w"]
P = ctypes.c_void_p


def _lib():
    from xdfm_amd import _lib
    return _lib, _lib.load()


def test_symbols_in_header_binding_and_library():
    mod, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), "include/xdfm.h does not declare %s" % n
        assert n in mod.SIGNATURES, "xdfm_amd/_lib.py does not bind %s" % n
        assert hasattr(lib, n), "libxdfm_hip.so lacks %s" % n
    assert lib.xdfm_abi_version() == mod.ABI_VERSION == 9           # additions only


def test_supported_envelope_edges():
    _, lib = _lib()
    for rows, k, out, want in [(1, 1, 32, 1), (1, 13, 32, 1), (4096, 429, 256, 1), (4099, 256, 256, 1), (520, 40, 64, 1),
                               (7, 5, 96, 1), (100, 37, 48, 0), (100, 37, 16, 0), (100, 37, 70, 0), (100, 37, 0, 0),
                               (0, 8, 32, 0), (-3, 8, 32, 0), (8, 0, 32, 0), (8, -1, 32, 0), (8, 8, -32, 0),
                               (8, (1 << 20) + 1, 32, 0), (8, 8, (1 << 20) + 32, 0)]:
        assert lib.xdfm_dense_supported(rows, k, out) == want, (rows, k, out)


def test_workspace_is_nonzero_and_monotone():
    """splits * (out * in + out) with splits = min(32, ceil(rows / 256)): never 0 inside the envelope, never shrinking when
    rows, in or out grow; 0 outside the envelope."""
    _, lib = _lib()
    ws = lib.xdfm_dense_bwd_w_ws_elems
    assert ws(1, 1, 32) == 1 * (32 + 32)
    assert ws(4096, 429, 256) == 16 * (256 * 429 + 256)
    assert ws(257, 256, 256) == 2 * (256 * 256 + 256)
    assert ws(1 << 20, 40, 64) == 32 * (64 * 40 + 64)
    rows_seq = [1, 2, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 100000, 1 << 24]
    for k, out in [(1, 32), (429, 256), (40, 64)]:
        vals = [ws(r, k, out) for r in rows_seq]
        assert all(v > 0 for v in vals) and vals == sorted(vals), (k, out, vals)
    for rows in (1, 300, 4096):
        vals = [ws(rows, k, 64) for k in (1, 2, 63, 64, 65, 429, 430, 5000)]
        assert all(v > 0 for v in vals) and vals == sorted(vals), (rows, vals)
        vals = [ws(rows, 429, out) for out in (32, 64, 96, 256, 288, 4096)]
        assert all(v > 0 for v in vals) and vals == sorted(vals), (rows, vals)
    for bad in [(4096, 429, 48), (0, 429, 256), (4096, 0, 256), (4096, 429, 0)]:
        assert ws(*bad) == 0, bad


def test_validation_before_device_work():
    """Null pointers, rows <= 0, a pitch below the column count, a NULL workspace and an unsupported out: rc 1 and a message
    that names the argument, with no GPU in the machine."""
    mod, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)                        # a non-null host address: validation must reject before touching it

    def fwd(x=p, rows=8, k=13, ldx=13, W=p, out=32, b=p, act=1, y=p, ldy=32):
        return lib.xdfm_dense_fwd(x, rows, k, ldx, W, out, b, act, y, ldy, None)

    def bwx(g=p, ldg=32, y=p, ldy=32, rows=8, out=32, W=p, k=13, dx=p, lddx=13):
        return lib.xdfm_dense_bwd_x(g, ldg, y, ldy, rows, out, W, k, dx, lddx, None)

    def bww(g=p, ldg=32, y=p, ldy=32, x=p, ldx=13, rows=8, k=13, out=32, ws=p, dW=p, db=p):
        return lib.xdfm_dense_bwd_w(g, ldg, y, ldy, x, ldx, rows, k, out, ws, dW, db, None)

    def err():
        return lib.xdfm_last_error()

    for call, ptrs in ((fwd, ("x", "W", "y")), (bwx, ("g", "W", "dx")), (bww, ("g", "x", "dW"))):
        for arg in ptrs:
            assert call(**{arg: None}) == 1 and b"null pointer" in err(), (call.__name__, arg)
        for rows in (0, -5):
            assert call(rows=rows) == 1 and b"rows = %d" % rows in err(), (call.__name__, rows, err())
        assert call(k=0) == 1 and b"in = 0" in err(), (call.__name__, err())
        for out in (48, 16, 0, 70):
            assert call(out=out) == 1 and b"out = %d" % out in err() and b"multiple of 32" in err(), (call.__name__, out, err())
    assert bww(ws=None) == 1 and b"workspace is NULL" in err()
    for call, kw, word in [(fwd, dict(ldx=12), b"ldx = 12"), (fwd, dict(ldy=31), b"ldy = 31"), (bwx, dict(ldg=31), b"ldg = 31"),
                           (bwx, dict(ldy=31), b"ldy = 31"), (bwx, dict(lddx=12), b"lddx = 12"), (bww, dict(ldg=31), b"ldg = 31"),
                           (bww, dict(ldy=31), b"ldy = 31"), (bww, dict(ldx=12), b"ldx = 12")]:
        assert call(**kw) == 1 and word in err(), (call.__name__, kw, err())
    for act in (2, -1, 7):
        assert fwd(act=act) == 1 and b"act = %d" % act in err()
    with pytest.raises(ValueError, match="dense_fwd"):
        mod.check(fwd(out=48), "dense_fwd")


def test_switch_parsing_and_cpu_tensors_stay_on_the_stock_path():
    from xdfm_amd import ops
    assert ops._env_switch({}, "XDFM_DNN_NATIVE") is True
    assert ops._env_switch({"XDFM_DNN_NATIVE": "1"}, "XDFM_DNN_NATIVE") is True
    assert ops._env_switch({"XDFM_DNN_NATIVE": "0"}, "XDFM_DNN_NATIVE") is False
    assert ops.DNN_NATIVE is ops._env_switch(os.environ, "XDFM_DNN_NATIVE")
    torch.manual_seed(0)
    x, W, b = torch.randn(9, 13), torch.randn(32, 13), torch.randn(32)
    assert not ops.dense_native(x, W, b)
    assert not ops.dense_native(x.double(), W.double(), b.double())
    assert torch.equal(ops.dense(x, W, b), torch.nn.functional.linear(x, W, b))
    assert torch.equal(ops.dense_relu(x, W, b), torch.relu(torch.nn.functional.linear(x, W, b)))
