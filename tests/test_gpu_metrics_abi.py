"""GPU tests (-m gpu) of K14 at the C ABI (xdfm_batch_metrics, csrc/metrics.hip), the entry point called directly, against
xdfm_amd.metrics' numpy functions on (y, float64(p)) (tests/metrics_ref.py).

AUC and accuracy: bit for bit.  Logloss and mse: |got - ref| <= (B + 4) * 2^-52 * ref (metrics_ref.bar).
Every call of the driver: a guard cell behind y (0.0) and behind p (NaN) -- read, either would move every metric --, `out` as
cells 1..4 of six doubles with a sentinel in cells 0 and 5 and in every slot `which` does not name, a workspace of exactly
xdfm_batch_metrics_ws_bytes bytes filled with 0xFF (or with an earlier call's contents) with 0xFF cells behind it that must
survive, and the call made twice: the same bits.

The largest observed share of the logloss / mse bar is printed per B and recorded in the first test's docstring."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -12345.6789
TAIL = 8                              # doubles behind the workspace that no launch may touch


def _dev():
    return torch.device("cuda:0")


def _lib():
    from xdfm_amd import _lib
    return _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _workspace(B, which, dev):
    n = _lib().xdfm_batch_metrics_ws_bytes(B, which)
    assert n > 0 and n % 8 == 0
    return torch.full((n + 8 * TAIL,), 0xFF, dtype=torch.uint8, device=dev), n


def run(y, p, which, ws=None, twice=True):
    """out4 of one xdfm_batch_metrics call (a list of 4 floats, the sentinel where `which` has no bit) after the checks of the
    module docstring.  ws: (tensor, bytes) of an earlier call to reuse as it was left."""
    from xdfm_amd import _lib
    dev, B = _dev(), y.size
    lib = _lib.load()
    yb = torch.from_numpy(np.concatenate([y, np.zeros(1, np.float32)])).to(dev)
    pb = torch.from_numpy(np.concatenate([p, np.full(1, np.nan, np.float32)])).to(dev)
    buf, n = ws if ws is not None else _workspace(B, which, dev)
    assert n >= lib.xdfm_batch_metrics_ws_bytes(B, which)
    outs = []
    for _ in range(2 if twice else 1):
        out = torch.full((6,), SENTINEL, dtype=torch.float64, device=dev)
        _lib.check(lib.xdfm_batch_metrics(_p(yb), _p(pb), B, which, _p(buf), _p(out[1:]), None), "batch_metrics")
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    got = outs[0]
    assert got.tobytes() == outs[-1].tobytes(), "two calls, two results"
    assert got[0] == SENTINEL and got[5] == SENTINEL, "a cell beside out4 was written"
    for bit, slot in R.SLOT.items():
        if not which & bit:
            assert got[1 + slot] == SENTINEL, "slot %d is not in which=%d and was written" % (slot, which)
    assert bool((buf[n:] == 0xFF).all()), "cells behind the workspace were written"
    assert yb[B].item() == 0.0 and pb[B].item() != pb[B].item()
    return [float(v) for v in got[1:5]], (buf, n)


def check(got, y, p, which, what):
    """Compares the named slots with the reference; returns the largest share of the logloss / mse bar."""
    ref, B, worst = R.reference(y, p), y.size, 0.0
    if which & R.AUC:
        assert R.same_bits(got[1], ref[1]), "%s: auc %r != %r" % (what, got[1], ref[1])
    if which & R.ACC:
        assert R.same_bits(got[3], ref[3]), "%s: accuracy %r != %r" % (what, got[3], ref[3])
    for bit in (R.LOGLOSS, R.MSE):
        if which & bit:
            k = R.SLOT[bit]
            share = R.ratio(got[k], ref[k], B)
            assert share <= 1.0, "%s: slot %d got %r ref %r, %.3g of the bar" % (what, k, got[k], ref[k], share)
            worst = max(worst, share)
    return worst


@pytest.mark.parametrize("B", R.B_LIST)
def test_every_case_against_the_numpy_metrics(B):
    """All score kinds x label kinds at this B (soft labels: logloss | mse only).  Single class: AUC NaN, the other three
    correct; all-equal scores with both classes: AUC exactly 0.5.
    Largest share of the bar observed on an MI355X over all B: 0.0207 (B = 63); 0.0058 at B = 256, 3.7e-4 or less from
    B = 4095 on, 8e-6 at the cap -- the figures tests/test_metrics_reference.py gets for the same order on the CPU."""
    worst = 0.0
    for sk, lk, y, p in R.cases(B):
        which = R.which_of(lk)
        got, _ = run(y, p, which)
        worst = max(worst, check(got, y, p, which, "B=%d %s %s" % (B, sk, lk)))
        if which & R.AUC:
            pos = int((y > 0.5).sum())
            if pos in (0, B):
                assert got[1] != got[1], (B, sk, lk, got[1])
            elif sk == "equal":
                assert got[1] == 0.5, (B, lk, got[1])
    print("K14 B=%d: largest share of the logloss / mse bar %.3g" % (B, worst))


@pytest.mark.parametrize("sk", ["uniform", "eight"])
def test_the_cap(sk):
    """B = 65536, the largest supported batch (128 x 128 tiles), all four metrics."""
    B = R.MAX_B
    y, p = R.labels("mixed", B, 1), R.scores(sk, B, 1)
    got, _ = run(y, p, R.ALL)
    print("K14 B=%d %s: largest share of the bar %.3g" % (B, sk, check(got, y, p, R.ALL, "cap %s" % sk)))


@pytest.mark.parametrize("which", list(range(1, 16)))
def test_every_combination_of_which(which):
    """B = 1025 (three tiles each way): the named slots are right, the others and the cells around out4 keep the sentinel."""
    B = 1025
    y, p = R.labels("mixed", B, 3), R.scores("eight", B, 3)
    got, _ = run(y, p, which)
    check(got, y, p, which, "which=%d" % which)
    full, _ = run(y, p, R.ALL)
    for bit, slot in R.SLOT.items():
        if which & bit:
            assert R.same_bits(got[slot], full[slot]), "slot %d depends on the other bits of which" % slot


def test_a_used_workspace_does_not_matter():
    """A call at B = 4097 leaves its partials; a call at B = 257 on that workspace (more stale cells than live ones) and one
    on a 0xFF workspace give the same bits as each other, for every metric."""
    yb, pb = R.labels("mixed", 4097, 4), R.scores("uniform", 4097, 4)
    _, used = run(yb, pb, R.ALL)
    y, p = R.labels("mixed", 257, 5), R.scores("sigmoid", 257, 5)
    fresh, _ = run(y, p, R.ALL)
    again, _ = run(y, p, R.ALL, ws=used)
    assert all(R.same_bits(a, b) for a, b in zip(fresh, again)), (fresh, again)
    check(again, y, p, R.ALL, "reused workspace")


def test_nan_scores_give_a_nan_auc():
    """Documented, not compared with the host version: any NaN in p makes the AUC NaN (and the sums it enters); accuracy
    counts it as class 0."""
    B = 700
    y, p = R.labels("mixed", B, 6), R.scores("uniform", B, 6)
    p[B // 2] = np.nan
    got, _ = run(y, p, R.ALL)
    assert got[1] != got[1] and got[0] != got[0] and got[2] != got[2]
    assert R.same_bits(got[3], R.reference(y, p)[3])
