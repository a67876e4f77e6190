"""CPU: the argument checks and the workspace query of K14 (xdfm_batch_metrics, include/xdfm.h).  Every refusal happens before
any device call, so it can be exercised without a GPU -- with made-up addresses that are never dereferenced."""
import ctypes

import pytest

import metrics_ref as R

Y, P, WS, OUT = 0x10000, 0x20000, 0x30000, 0x40000         # aligned stand-in addresses


def _lib():
    from xdfm_amd import _lib
    return _lib.load()


def _call(y=Y, p=P, B=64, which=R.ALL, ws=WS, out=OUT):
    lib = _lib()
    v = ctypes.c_void_p
    return lib.xdfm_batch_metrics(v(y) if y else None, v(p) if p else None, B, which, v(ws) if ws else None, v(out) if out else None,
                                  None), lib.xdfm_last_error().decode()


@pytest.mark.parametrize("missing", ["y", "p", "ws", "out"])
def test_a_null_operand_is_refused(missing):
    rc, msg = _call(**{missing: 0})
    assert rc == 1 and "null pointer" in msg and "batch_metrics" in msg


@pytest.mark.parametrize("B", [0, -1, R.MAX_B + 1, 2 ** 31 - 1])
def test_b_outside_the_range_is_refused(B):
    rc, msg = _call(B=B)
    assert rc == 1 and ("B=%d" % B) in msg


@pytest.mark.parametrize("which", [0, 16, 17, 31, 256, -1])
def test_which_outside_1_to_15_is_refused(which):
    rc, msg = _call(which=which)
    assert rc == 1 and ("which=%d" % which) in msg


@pytest.mark.parametrize("off", [1, 2, 4, 7])
def test_misaligned_ws_and_out_are_refused(off):
    rc, msg = _call(ws=WS + off)
    assert rc == 1 and "ws=" in msg and ("%x" % (WS + off)) in msg and "8-byte" in msg
    rc, msg = _call(out=OUT + off)
    assert rc == 1 and "out4=" in msg and ("%x" % (OUT + off)) in msg and "8-byte" in msg


def test_refusals_raise_through_the_binding():
    from xdfm_amd import _lib
    rc, _ = _call(B=0)
    with pytest.raises(ValueError, match="B=0"):
        _lib.check(rc, "batch_metrics")


def test_ws_bytes():
    lib = _lib()
    for B in (0, -5, R.MAX_B + 1):
        assert lib.xdfm_batch_metrics_ws_bytes(B, R.ALL) == 0
    for which in (0, 16, -1):
        assert lib.xdfm_batch_metrics_ws_bytes(4096, which) == 0
    for B in R.B_LIST + [R.MAX_B]:
        for which in range(1, 16):
            n = lib.xdfm_batch_metrics_ws_bytes(B, which)
            assert n > 0 and n % 8 == 0, (B, which, n)
            assert lib.xdfm_batch_metrics_ws_bytes(B, which | R.AUC) >= n
    # the partials are a function of B alone apart from the pair counts: monotone in B, and the cap's size is what ops keeps
    sizes = [lib.xdfm_batch_metrics_ws_bytes(B, R.ALL) for B in R.B_LIST + [R.MAX_B]]
    assert sizes == sorted(sizes) and sizes[-1] <= 1 << 20
