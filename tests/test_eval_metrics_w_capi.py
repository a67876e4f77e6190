"""CPU: the exports, the argument checks and the workspace query of K14w (xdfm_eval_metrics_w, include/xdfm.h) -- every refusal
happens before any device call, so it is exercised without a GPU, with made-up addresses that are never dereferenced -- and
what ops.eval_metrics_w refuses on the host."""
import ctypes

import pytest
import torch

import eval_metrics_w_ref as R

Y, P, W, WS, OUT = 0x10000, 0x20000, 0x50000, 0x30000, 0x40000         # aligned stand-in addresses


def _lib():
    from xdfm_amd import _lib
    return _lib.load()


def _call(y=Y, p=P, w=W, N=5000, which=R.ALL, ws=WS, out=OUT):
    lib = _lib()
    v = lambda a: ctypes.c_void_p(a) if a else None        # noqa: E731
    return lib.xdfm_eval_metrics_w(v(y), v(p), v(w), N, which, v(ws), v(out), None), lib.xdfm_last_error().decode()


def test_both_symbols_are_exported_and_bound():
    from xdfm_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("xdfm_eval_metrics_w_ws_bytes", "xdfm_eval_metrics_w"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["xdfm_eval_metrics_w_ws_bytes"][1][0] is ctypes.c_long
    assert len(_lib.SIGNATURES["xdfm_eval_metrics_w"][1]) == 8


@pytest.mark.parametrize("missing", ["y", "p", "w", "ws", "out"])
def test_a_null_operand_is_refused(missing):
    rc, msg = _call(**{missing: 0})
    assert rc == 1 and "null pointer" in msg and "eval_metrics_w" in msg


@pytest.mark.parametrize("N", [0, -1, R.MAX_N + 1, 2 ** 31, 2 ** 40])
def test_n_outside_the_range_is_refused(N):
    rc, msg = _call(N=N)
    assert rc == 1 and ("N=%d" % N) in msg


@pytest.mark.parametrize("which", [0, 16, 17, 256, -1])
def test_which_outside_1_to_15_is_refused(which):
    rc, msg = _call(which=which)
    assert rc == 1 and ("which=%d" % which) in msg


@pytest.mark.parametrize("off", [1, 2, 4, 7])
def test_misaligned_ws_and_out_are_refused(off):
    rc, msg = _call(ws=WS + off)
    assert rc == 1 and "ws=" in msg and ("%x" % (WS + off)) in msg and "8-byte" in msg
    rc, msg = _call(out=OUT + off)
    assert rc == 1 and "out4=" in msg and ("%x" % (OUT + off)) in msg and "8-byte" in msg


def test_ws_bytes():
    lib = _lib()
    for N in (0, -5, R.MAX_N + 1, 2 ** 33):
        assert lib.xdfm_eval_metrics_w_ws_bytes(N, R.ALL) == 0
    for which in (0, 16, -1):
        assert lib.xdfm_eval_metrics_w_ws_bytes(4096, which) == 0
    ns = sorted(R.N_SIZES + [65537, 1 << 22, R.MAX_N])
    for N in ns:
        tiles = (N + R.TILE - 1) // R.TILE
        sizes = {which: lib.xdfm_eval_metrics_w_ws_bytes(N, which) for which in range(1, 16)}
        # without the AUC: the 7 partial cells per tile of include/xdfm.h; with it the documented total (about 24 N bytes)
        assert all(sizes[w] == 8 * 7 * tiles for w in sizes if not w & R.AUC), (N, sizes)
        want = 8 * (9 * tiles + (N + 1) + 4 * ((N + 1) // 2) + 128 * tiles + 128)
        assert all(sizes[w] == want for w in sizes if w & R.AUC), (N, sizes, want)
        assert 24 * N <= want <= 24 * N + 8 * 137 * tiles + 1100
    for which in (R.ALL, R.LOGLOSS):
        sizes = [lib.xdfm_eval_metrics_w_ws_bytes(N, which) for N in ns]
        assert sizes == sorted(sizes)


def test_ops_refuses_host_tensors_and_reads_the_switch_once():
    from xdfm_amd import ops
    y, p, w = torch.zeros(8), torch.zeros(8), torch.ones(8)
    assert not ops.eval_metrics_w_supported(y, p, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eval_metrics_w(y, p, w, R.ALL)
    assert isinstance(ops.EVAL_W_NATIVE, bool)
