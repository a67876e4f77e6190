"""GPU tests (-m gpu) of K14s at the C ABI (xdfm_eval_metrics, csrc/eval_metrics.hip), the entry point called directly, against
xdfm_amd.metrics' numpy functions on (y, float64(p)) (tests/eval_metrics_ref.py).

AUC and accuracy: bit for bit.  Logloss and mse: within eval_metrics_ref.bar (the derived bound of the two summation orders).
Every call of the driver: a guard cell behind y (0.0) and behind p (NaN) -- read, either would move every metric --, `out` as
cells 1..4 of six doubles with a sentinel in cells 0 and 5 and in every slot `which` does not name, a workspace of exactly
xdfm_eval_metrics_ws_bytes bytes filled with 0xFF (or with an earlier call's contents) between 0xFF guard cells that must
survive, and the call made twice: the same bits.

The largest observed share of the logloss / mse bar is printed per N; on an MI355X it was 0.079 (N = 255), 0.05 or less from
N = 1024 on (0.042 at 300001 rows, 0.051 at 1048577)."""
import ctypes

import numpy as np
import pytest
import torch

import eval_metrics_ref as R
import metrics_ref as K14

pytestmark = pytest.mark.gpu
SENTINEL = -12345.6789
GUARD = 8                             # doubles in front of and behind the workspace that no launch may touch


def _dev():
    return torch.device("cuda:0")


def _lib():
    from xdfm_amd import _lib
    return _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _workspace(N, which, dev):
    n = _lib().xdfm_eval_metrics_ws_bytes(N, which)
    assert n > 0 and n % 8 == 0
    return torch.full((n + 16 * GUARD,), 0xFF, dtype=torch.uint8, device=dev), n


def run(y, p, which, ws=None, twice=True):
    """out4 of one xdfm_eval_metrics call (a list of 4 floats, the sentinel where `which` has no bit) after the checks of the
    module docstring.  ws: (tensor, bytes) of an earlier call to reuse as it was left."""
    from xdfm_amd import _lib
    dev, N = _dev(), y.size
    lib = _lib.load()
    yb = torch.from_numpy(np.concatenate([y, np.zeros(1, np.float32)])).to(dev)
    pb = torch.from_numpy(np.concatenate([p, np.full(1, np.nan, np.float32)])).to(dev)
    buf, n = ws if ws is not None else _workspace(N, which, dev)
    assert n >= lib.xdfm_eval_metrics_ws_bytes(N, which)
    body = buf[8 * GUARD:]
    outs = []
    for _ in range(2 if twice else 1):
        out = torch.full((6,), SENTINEL, dtype=torch.float64, device=dev)
        _lib.check(lib.xdfm_eval_metrics(_p(yb), _p(pb), N, which, _p(body), _p(out[1:]), None), "eval_metrics")
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    got = outs[0]
    assert got.tobytes() == outs[-1].tobytes(), "two calls, two results"
    assert got[0] == SENTINEL and got[5] == SENTINEL, "a cell beside out4 was written"
    for bit, slot in R.SLOT.items():
        if not which & bit:
            assert got[1 + slot] == SENTINEL, "slot %d is not in which=%d and was written" % (slot, which)
    assert bool((buf[:8 * GUARD] == 0xFF).all()) and bool((buf[8 * GUARD + n:] == 0xFF).all()), "cells around the workspace were written"
    assert yb[N].item() == 0.0 and pb[N].item() != pb[N].item()
    return [float(v) for v in got[1:5]], (buf, n)


def check(got, y, p, which, what, ref=None):
    """Compares the named slots with the reference; returns the largest share of the logloss / mse bar."""
    ref, N, worst = ref or R.reference(y, p), y.size, 0.0
    if which & R.AUC:
        assert R.same_bits(got[1], ref[1]), "%s: auc %r != %r" % (what, got[1], ref[1])
    if which & R.ACC:
        assert R.same_bits(got[3], ref[3]), "%s: accuracy %r != %r" % (what, got[3], ref[3])
    for bit in (R.LOGLOSS, R.MSE):
        if which & bit:
            k = R.SLOT[bit]
            share = R.ratio(got[k], ref[k], N)
            assert share <= 1.0, "%s: slot %d got %r ref %r, %.3g of the bar" % (what, k, got[k], ref[k], share)
            worst = max(worst, share)
    return worst


@pytest.mark.parametrize("N", R.N_EDGES)
def test_every_case_at_the_edges(N):
    """All score kinds x label kinds at 1, 2 and every block / tile edge +- 1.  All-equal scores with both classes: exactly 0.5;
    a single class (N = 1, or `alternating` at N = 1): NaN."""
    worst = 0.0
    for sk, lk, y, p in R.cases(N):
        got, _ = run(y, p, R.ALL, twice=(lk == "mixed"))
        worst = max(worst, check(got, y, p, R.ALL, "N=%d %s %s" % (N, sk, lk)))
        pos = int((y > 0.5).sum())
        if pos in (0, N):
            assert got[1] != got[1], (N, sk, lk, got[1])
        elif sk == "equal":
            assert got[1] == 0.5, (N, lk, got[1])
    print("K14s N=%d: largest share of the logloss / mse bar %.3g" % (N, worst))


@pytest.mark.parametrize("N,kinds", [(R.N_K14_CAP_PLUS_1, ["uniform", "eight", "byte3", "wide"]),
                                     (R.N_MANY_TILES, ["uniform", "eight", "byte0", "byte1", "byte2", "byte3"]),
                                     (R.N_SCAN_RUNS_OF_2, ["uniform"])])
def test_many_tiles(N, kinds):
    """One above K14's cap (17 tiles), 74 tiles, and the first N at which a scan thread takes two tiles (257 tiles)."""
    worst = 0.0
    for sk, lk, y, p in R.cases(N, kinds, ["mixed"]):
        got, _ = run(y, p, R.ALL, twice=(sk == "uniform"))
        worst = max(worst, check(got, y, p, R.ALL, "N=%d %s" % (N, sk)))
    print("K14s N=%d: largest share of the logloss / mse bar %.3g" % (N, worst))


@pytest.mark.parametrize("N", [1, 700, 4097])
def test_one_class_only_gives_nan(N):
    for cls in (0.0, 1.0):
        y, p = np.full(N, cls, np.float32), R.scores("uniform", N, 5)
        got, _ = run(y, p, R.ALL)
        assert got[1] != got[1]
        ref = R.reference(y, p)
        assert R.same_bits(got[3], ref[3]) and R.ratio(got[0], ref[0], N) <= 1.0 and R.ratio(got[2], ref[2], N) <= 1.0


@pytest.mark.parametrize("where", ["positive", "negative"])
def test_a_nan_score_gives_a_nan_auc(where):
    """Documented, not compared with the host version: any NaN in p makes the AUC NaN (and the sums it enters); accuracy counts
    it as class 0."""
    N = 5000
    y, p = R.labels("mixed", N, 6), R.scores("uniform", N, 6)
    rows = np.flatnonzero(y > 0.5) if where == "positive" else np.flatnonzero(y <= 0.5)
    p[rows[rows.size // 2]] = np.nan
    got, _ = run(y, p, R.ALL)
    assert got[1] != got[1] and got[0] != got[0] and got[2] != got[2]
    assert R.same_bits(got[3], R.reference(y, p)[3])


@pytest.mark.parametrize("which", list(range(1, 16)))
def test_every_combination_of_which(which):
    """N = 8193 (three tiles): the named slots are right and do not depend on the other bits, the others and the cells around
    out4 keep the sentinel."""
    N = 8193
    y, p = R.labels("mixed", N, 3), R.scores("eight", N, 3)
    got, _ = run(y, p, which)
    check(got, y, p, which, "which=%d" % which)
    full, _ = run(y, p, R.ALL, twice=False)
    for bit, slot in R.SLOT.items():
        if which & bit:
            assert R.same_bits(got[slot], full[slot]), "slot %d depends on the other bits of which" % slot


def test_a_used_workspace_does_not_matter():
    """A call at N = 65537 leaves its keys, histograms and partials; a call at N = 4097 on that workspace (more stale cells
    than live ones) and one on a 0xFF workspace give the same bits as each other, for every metric."""
    yb, pb = R.labels("mixed", 65537, 4), R.scores("uniform", 65537, 4)
    _, used = run(yb, pb, R.ALL, twice=False)
    y, p = R.labels("mixed", 4097, 5), R.scores("wide", 4097, 5)
    fresh, _ = run(y, p, R.ALL)
    again, _ = run(y, p, R.ALL, ws=used)
    assert all(R.same_bits(a, b) for a, b in zip(fresh, again)), (fresh, again)
    check(again, y, p, R.ALL, "reused workspace")


@pytest.mark.parametrize("N", [1, 257, 4097, K14.MAX_B])
def test_agreement_with_k14_below_its_cap(N):
    """xdfm_batch_metrics on the same input: AUC and accuracy in bits, logloss and mse within K14's bar AND this kernel's."""
    from xdfm_amd import _lib
    lib, dev = _lib.load(), _dev()
    for sk in ("uniform", "eight"):
        y, p = R.labels("mixed", N, 8), R.scores(sk, N, 8)
        got, _ = run(y, p, R.ALL, twice=False)
        yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
        ws = torch.empty(lib.xdfm_batch_metrics_ws_bytes(N, R.ALL) // 8, dtype=torch.float64, device=dev)
        out = torch.zeros(4, dtype=torch.float64, device=dev)
        _lib.check(lib.xdfm_batch_metrics(_p(yd), _p(pd), N, R.ALL, _p(ws), _p(out), None), "batch_metrics")
        torch.cuda.synchronize()
        k14 = out.tolist()
        assert R.same_bits(got[1], k14[1]) and R.same_bits(got[3], k14[3]), (N, sk, got, k14)
        for k in (0, 2):
            assert R.ratio(got[k], k14[k], N) <= 1.0 and K14.ratio(got[k], k14[k], N) <= 1.0, (N, sk, k, got[k], k14[k])
