"""K11 with a second label vector (xdfm_compact_rows_fwd_n, csrc/compact.hip) at the C ABI.  Under row-parallel training the
slots, the count and the moved rows come from a rank's own labels and the normaliser inv_n from the labels of the global
batch.  The reference is the old entry point itself: every output but inv_n must equal its outputs byte for byte, inv_n must
have the bits it leaves when the second vector is handed to it as its labels, and a null second vector must be the old call.
No tolerance anywhere.  One test without a GPU: the symbol is declared, bound and exported."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

W, F = 6, 2
OUTPUTS = ("pos", "n_rows", "valid", "labels", "d_rows", "targets")


def test_counted_entry_point_is_declared_bound_and_exported():
    from xdfm_amd import _lib
    with open(os.path.join(ROOT, "include", "xdfm.h")) as f:
        src = f.read()
    new, old = "xdfm_compact_rows_fwd_n", "xdfm_compact_rows_fwd"
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % new, src)
    assert m, new + " is not declared in include/xdfm.h"
    assert "count_y" in m.group(1) and "n_count" in m.group(1)
    res, args = _lib.SIGNATURES[new]
    assert res is ctypes.c_int and len(args) == m.group(1).count(",") + 1
    o = _lib.SIGNATURES[old][1]
    assert args == o[:11] + [ctypes.c_void_p, ctypes.c_long] + o[11:]           # the old call plus (count_y, n_count)
    lib = _lib.load()
    assert getattr(lib, new) is not None
    assert re.search(r"#define\s+XDFM_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, src) and lib.xdfm_abi_version() == _lib.ABI_VERSION
    # validated before any device work: a second vector needs at least one label
    p = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    assert lib.xdfm_compact_rows_fwd_n(p, 3, 3, p, 2, p, 4, 2, p, 1, 1, p, 0, p, p, p, p, p, p, p, None) == 1
    assert b"compact_rows_fwd_n" in lib.xdfm_last_error()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _labels(n, rng, positives=True):
    y = (rng.random(n) < 0.3).astype(np.float32) if positives else np.zeros(n, np.float32)
    if positives:
        y[rng.integers(0, n)] = 1.0
    y[rng.random(n) < 0.1] = 0.5                                     # neither 0 nor 1: not a positive
    return y


def _call(dev, y, positive_only, count_y="old"):
    """All outputs of one forward as bytes.  count_y "old": xdfm_compact_rows_fwd; None or an array: xdfm_compact_rows_fwd_n."""
    from xdfm_amd import _lib
    lib = _lib.load()
    B = y.size
    rng = np.random.default_rng(B)                                   # the inputs depend on B only
    Xn = np.concatenate([rng.integers(0, 1000, (B, F)).astype(np.float32), rng.random((B, 1), np.float32)], axis=1)
    X, d_in = torch.from_numpy(Xn).to(dev), torch.from_numpy(rng.standard_normal((B, W)).astype(np.float32)).to(dev)
    yt, cols = torch.from_numpy(y).to(dev), torch.arange(F, dtype=torch.int32, device=dev)
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    out = dict(pos=torch.full((B,), -7, **i32), n_rows=torch.full((1,), -7, **i32), inv_n=torch.full((1,), np.nan, **f32),
               valid=torch.full((B,), np.nan, **f32), d_rows=torch.full((B, W), np.nan, **f32),
               labels=torch.full((B,), np.nan, **f32), targets=torch.full((F, B), -7, dtype=torch.int64, device=dev))
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (P(X), X.stride(0), X.shape[1], P(d_in), W, P(yt), B, W, P(cols), F, int(positive_only))
    tail = tuple(P(out[k]) for k in ("pos", "n_rows", "inv_n", "valid", "d_rows", "labels", "targets")) + (stream,)
    if isinstance(count_y, str):
        _lib.check(lib.xdfm_compact_rows_fwd(*(head + tail)), "compact_rows_fwd")
    else:
        # five ones behind the counted labels, inside the allocation: a scan that ran past n_count would count them
        ct = None if count_y is None else torch.from_numpy(np.concatenate([count_y, np.ones(5, np.float32)])).to(dev)
        n_count = 0 if count_y is None else count_y.size
        _lib.check(lib.xdfm_compact_rows_fwd_n(*(head + (P(ct), n_count) + tail)), "compact_rows_fwd_n")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("positive_only", [True, False])
@pytest.mark.parametrize("B", [1, 1023, 1025, 4100])
def test_normaliser_from_a_second_label_vector(B, positive_only):
    """B below, at and above one tile of the scan (1024 rows) and over several; n_count = B and 3 B + 7 (another number of
    tiles than B, not a multiple of the wave); a second vector without any positive; a null one."""
    dev = _dev()
    rng = np.random.default_rng(11 * B + int(positive_only))
    y = _labels(B, rng)
    old = _call(dev, y, positive_only)
    null = _call(dev, y, positive_only, None)
    for k in OUTPUTS + ("inv_n",):
        assert null[k] == old[k], "null count_y, " + k
    for n_count, positives in ((B, True), (3 * B + 7, True), (3 * B + 7, False), (B, False)):
        count_y = _labels(n_count, rng, positives)
        new = _call(dev, y, positive_only, count_y)
        for k in OUTPUTS:
            assert new[k] == old[k], "n_count %d: %s differs from the old entry point's" % (n_count, k)
        want = _call(dev, count_y, positive_only)["inv_n"]           # the old entry point with count_y as its labels
        assert new["inv_n"] == want, (n_count, positives, np.frombuffer(new["inv_n"], np.float32), np.frombuffer(want, np.float32))
        if positive_only and not positives:
            assert np.frombuffer(new["inv_n"], np.float32)[0] == np.float32(1.0) / np.float32(1e-8)
