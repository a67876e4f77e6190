"""GPU tests (-m gpu) of K14w at the C ABI (xdfm_eval_metrics_w, csrc/eval_metrics_w.hip), the entry point called directly,
against xdfm_amd.metrics' weighted numpy functions in float64 (tests/eval_metrics_w_ref.py, which derives the bars).

Every call of the driver: a guard cell behind y (0.0), behind p (NaN) and behind w (1.0) -- read, each would move a metric --,
`out` as cells 1..4 of six doubles with a sentinel in cells 0 and 5 and in every slot `which` does not name, a workspace of
exactly xdfm_eval_metrics_w_ws_bytes bytes filled with 0xFF (or an earlier call's contents) between 0xFF guard cells that must
survive, and the call made twice: the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import eval_metrics_ref as S
import eval_metrics_w_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -12345.6789
GUARD = 8                             # doubles in front of and behind the workspace that no launch may touch


def _dev():
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _workspace(N, which, dev, extra=0):
    from xdfm_amd import _lib
    n = _lib.load().xdfm_eval_metrics_w_ws_bytes(N, which)
    assert n > 0 and n % 8 == 0
    return torch.full((n + extra + 16 * GUARD,), 0xFF, dtype=torch.uint8, device=dev), n


def run(y, p, w, which, ws=None, twice=True):
    """out4 of one xdfm_eval_metrics_w call (4 floats, the sentinel where `which` has no bit) after the checks of the module
    docstring, and the (buffer, bytes) of its workspace."""
    from xdfm_amd import _lib
    dev, N = _dev(), y.size
    lib = _lib.load()
    yb = torch.from_numpy(np.concatenate([y, np.zeros(1, np.float32)])).to(dev)
    pb = torch.from_numpy(np.concatenate([p, np.full(1, np.nan, np.float32)])).to(dev)
    wb = torch.from_numpy(np.concatenate([w, np.ones(1, np.float32)])).to(dev)
    buf, n = ws if ws is not None else _workspace(N, which, dev)
    assert n >= lib.xdfm_eval_metrics_w_ws_bytes(N, which)
    body = buf[8 * GUARD:]
    outs = []
    for _ in range(2 if twice else 1):
        out = torch.full((6,), SENTINEL, dtype=torch.float64, device=dev)
        _lib.check(lib.xdfm_eval_metrics_w(_p(yb), _p(pb), _p(wb), N, which, _p(body), _p(out[1:]), None), "eval_metrics_w")
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    got = outs[0]
    assert got.tobytes() == outs[-1].tobytes(), "two calls, two results"
    assert got[0] == SENTINEL and got[5] == SENTINEL, "a cell beside out4 was written"
    for bit, slot in R.SLOT.items():
        if not which & bit:
            assert got[1 + slot] == SENTINEL, "slot %d is not in which=%d and was written" % (slot, which)
    assert bool((buf[:8 * GUARD] == 0xFF).all()) and bool((buf[8 * GUARD + n:] == 0xFF).all()), "cells around the workspace were written"
    assert yb[N].item() == 0.0 and pb[N].item() != pb[N].item() and wb[N].item() == 1.0
    return [float(v) for v in got[1:5]], (buf, n)


def run_unweighted(y, p, which):
    """xdfm_eval_metrics (K14s) on the same rows: 4 floats, the sentinel where `which` has no bit."""
    from xdfm_amd import _lib
    dev, lib = _dev(), _lib.load()
    yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    ws = torch.empty(lib.xdfm_eval_metrics_ws_bytes(y.size, which) // 8, dtype=torch.float64, device=dev)
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device=dev)
    _lib.check(lib.xdfm_eval_metrics(_p(yd), _p(pd), y.size, which, _p(ws), _p(out), None), "eval_metrics")
    torch.cuda.synchronize()
    return out.tolist()


def check(got, y, p, w, which, what, exact=False):
    """Every named slot within its bar; with `exact` (weights that make every sum exact) the AUC and the accuracy bit for bit.
    Returns the largest share of a bar."""
    ref, N, worst = R.reference(y, p, w), y.size, 0.0
    for bit, slot in R.SLOT.items():
        if not which & bit:
            continue
        if exact and slot in (1, 3):
            assert R.same_bits(got[slot], ref[slot]) or (got[slot] != got[slot] and ref[slot] != ref[slot]), \
                "%s: slot %d %r != %r" % (what, slot, got[slot], ref[slot])
            continue
        share = R.ratio(got[slot], ref[slot], N, slot)
        print("%s slot %d got %r ref %r share of the bar %.3g" % (what, slot, got[slot], ref[slot], share))
        assert share <= 1.0, "%s: slot %d got %r ref %r, %.3g of the bar" % (what, slot, got[slot], ref[slot], share)
        worst = max(worst, share)
    return worst


def _case(N, seed, score="uniform", label="mixed"):
    return S.labels(label, N, seed), S.scores(score, N, seed)


@pytest.mark.parametrize("N", R.N_SIZES)
def test_dyadic_weights_are_exact(N):
    """Multiples of 1/4 in [0, 4], a fifth of them zero: AUC and accuracy equal the float64 reference bit for bit (every sum
    is exact), logloss and mse lie within the derived bar.  Uniform scores and eight distinct scores (long tie runs)."""
    for sk in ("uniform", "eight"):
        y, p = _case(N, N % 977, sk)
        w = R.weights("dyadic", N, N % 977)
        got, _ = run(y, p, w, R.ALL)
        check(got, y, p, w, R.ALL, "dyadic N=%d %s" % (N, sk), exact=True)


@pytest.mark.parametrize("N", [4097, 4096 * 257 + 3])
def test_unit_weights_give_the_bits_of_k14s(N):
    """w == 1 everywhere: all four slots equal xdfm_eval_metrics' bits, for every subset `which`."""
    y, p = _case(N, 21)
    w = np.ones(N, np.float32)
    for which in range(1, 16):
        got, _ = run(y, p, w, which, twice=False)
        ref = run_unweighted(y, p, which)
        for bit, slot in R.SLOT.items():
            if which & bit:
                assert R.same_bits(got[slot], ref[slot]), "N=%d which=%d slot %d: %r != %r" % (N, which, slot, got[slot], ref[slot])


@pytest.mark.parametrize("N", R.N_SIZES)
@pytest.mark.parametrize("kind", ["uniform", "wide"])
def test_general_weights_within_the_bars(N, kind):
    y, p = _case(N, 33 + N % 89)
    w = R.weights(kind, N, N % 89)
    got, _ = run(y, p, w, R.ALL, twice=False)
    check(got, y, p, w, R.ALL, "%s N=%d" % (kind, N))


@pytest.mark.parametrize("sk", ["byte0", "byte1", "byte2", "byte3", "wide", "zeros"])
def test_scores_that_need_every_radix_pass(sk):
    """Scores that differ in one key byte only (a pass skipped, or a weight that does not follow its key, leaves the prefix
    sums wrong), negative scores with +-inf, and +-0.0 which tie.  Dyadic weights: exact."""
    N = 8193
    y, p = _case(N, 7, sk)
    w = R.weights("dyadic", N, 7)
    got, _ = run(y, p, w, R.ALL, twice=False)
    check(got, y, p, w, R.ALL, "scores %s" % sk, exact=True)


def test_a_tie_group_across_a_tile_boundary():
    """Places 4000 .. 4200 of the SORTED non-positives share one score and carry unequal weights: the group crosses the tile
    boundary at 4096, and some positives tie with it.  The weight must stay with its key through every stable pass: dyadic
    weights exact, general within the bar."""
    N = 3 * 4096 + 5
    rng = np.random.default_rng(77)
    p = np.sort(rng.random(N).astype(np.float32))
    y = (rng.random(N) < 0.1).astype(np.float32)
    neg, pos = np.flatnonzero(y == 0), np.flatnonzero(y > 0.5)    # p ascends: `neg` is the order the kernel sorts them into
    tie = p[neg[4100]]
    p[neg[4000:4201]] = tie
    p[pos[::40]] = tie
    perm = rng.permutation(N)
    for kind, exact in (("dyadic", True), ("wide", False)):
        w = R.weights(kind, N, 78)
        got, _ = run(y[perm], p[perm], w[perm], R.ALL)
        check(got, y[perm], p[perm], w[perm], R.ALL, "tie group, %s" % kind, exact=exact)


def test_one_class_and_zero_weight_give_nan():
    """All rows one class; W == 0 (NaN in every slot); Wpos == 0 by the weights alone.  Slots not asked for keep their bits
    (checked by `run`)."""
    N = 5000
    y, p = _case(N, 9)
    for cls in (0.0, 1.0):
        yy = np.full(N, cls, np.float32)
        w = R.weights("dyadic", N, 9)
        got, _ = run(yy, p, w, R.ALL)
        assert got[1] != got[1]
        check(got, yy, p, w, R.LOGLOSS | R.MSE | R.ACC, "one class", exact=True)
    got, _ = run(y, p, np.zeros(N, np.float32), R.ALL)
    assert all(v != v for v in got), got
    got, _ = run(y, p, np.zeros(N, np.float32), R.AUC | R.ACC)
    assert got[1] != got[1] and got[3] != got[3]
    w = R.weights("dyadic", N, 10)
    w[y > 0.5] = 0.0
    got, _ = run(y, p, w, R.ALL)
    assert got[1] != got[1]
    check(got, y, p, w, R.LOGLOSS | R.MSE | R.ACC, "Wpos == 0", exact=True)


@pytest.mark.parametrize("where", ["positive", "negative"])
def test_nan_scores(where):
    """A NaN score with weight 0 is ignored in every slot; with a weight > 0 the AUC is NaN."""
    N = 5000
    y, p = _case(N, 6)
    w = R.weights("dyadic", N, 6)
    rows = np.flatnonzero(y > 0.5) if where == "positive" else np.flatnonzero(y <= 0.5)
    row = rows[rows.size // 2]
    p[row] = np.nan
    w[row] = 0.0
    got, _ = run(y, p, w, R.ALL)
    assert all(v == v for v in got), got
    check(got, y, p, w, R.ALL, "NaN with weight 0", exact=True)
    w[row] = 0.75
    got, _ = run(y, p, w, R.ALL)
    assert got[1] != got[1] and got[0] != got[0] and got[2] != got[2] and got[3] == got[3]


def test_a_used_workspace_does_not_matter():
    """A call at N = 65537 leaves its keys, weights, prefix sums and partials; a call at N = 4097 on that workspace and one
    on a 0xFF workspace give the same bits."""
    yb, pb = _case(65537, 4)
    _, used = run(yb, pb, R.weights("wide", 65537, 4), R.ALL, twice=False)
    y, p = _case(4097, 5, "wide")
    w = R.weights("uniform", 4097, 5)
    fresh, _ = run(y, p, w, R.ALL)
    again, _ = run(y, p, w, R.ALL, ws=used)
    assert all(R.same_bits(a, b) for a, b in zip(fresh, again)), (fresh, again)


def test_without_the_auc_only_the_prefix_is_touched():
    """which without the AUC bit: 7 cells per tile (include/xdfm.h) -- the query says so, and a buffer with room behind them
    keeps its 0xFF there (the guard check of `run`, which takes `n` as the workspace's end)."""
    from xdfm_amd import _lib
    N = 8193
    which = R.LOGLOSS | R.MSE | R.ACC
    assert _lib.load().xdfm_eval_metrics_w_ws_bytes(N, which) == 8 * 7 * 3
    y, p = _case(N, 12)
    w = R.weights("uniform", N, 12)
    buf, n = _workspace(N, which, _dev(), extra=1 << 16)
    got, _ = run(y, p, w, which, ws=(buf, n))
    check(got, y, p, w, which, "no auc")
