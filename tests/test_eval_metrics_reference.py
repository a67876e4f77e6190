"""CPU: the arithmetic K14s (csrc/eval_metrics.hip) is built on, checked against the pinned numpy metrics without a kernel
(tests/eval_metrics_ref.py): the "sort the non-positives, two bounds per positive" count has the bits of the mid-rank form, the
key map is monotone and merges the two zeros, and the tiled summation order stays inside the derived bar."""
import numpy as np
import pytest

import eval_metrics_ref as R
from xdfm_amd import metrics as M

NS = [1, 2, 65, 257, 4097, 9001]


@pytest.mark.parametrize("N", NS)
def test_sort_and_bounds_auc_has_the_bits_of_roc_auc_score(N):
    """Every score kind (random, 8 values, all equal, one key byte varying, +-0.0 mixed, denormals, negative scores and scores
    above 1 with +-inf) x every label kind (mixed, positives first / last / alternating, one positive only, one negative
    only): bit for bit; all-equal scores give exactly 0.5; a single class gives NaN."""
    seen = 0
    for sk, lk, y, p in R.cases(N):
        got, want = R.sort_auc(y, p), R.reference(y, p)[1]
        assert R.same_bits(got, want), (N, sk, lk, got, want)
        pos = int((y > 0.5).sum())
        if pos in (0, N):
            assert got != got, (N, sk, lk)
        elif sk == "equal":
            assert got == 0.5, (N, lk, got)
        seen += 1
    assert seen == len(R.SCORES) * len(R.LABELS)


def test_the_case_generators_hold_what_they_promise():
    N = 4097
    for k in range(4):
        key = R.keys(R.scores("byte%d" % k, N, k))
        assert np.isfinite(R.scores("byte%d" % k, N, k)).all()
        varying = np.bitwise_or.reduce(key ^ key[0])
        assert varying != 0 and varying & ~np.uint32(0xFF << (8 * k)) == 0, (k, hex(int(varying)))
    z = R.scores("zeros", N, 1)
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    d = R.scores("denormal", N, 1)
    assert (np.abs(d[d != 0]) < np.finfo(np.float32).tiny).all() and (d < 0).any() and (d > 0).any()
    w = R.scores("wide", N, 1)
    assert (w < 0).any() and (w > 1).any() and np.isinf(w).sum() == 2
    assert len(np.unique(R.scores("eight", N, 1))) == 8
    for lk in R.LABELS:
        y = R.labels(lk, N, 2)
        assert 0 < (y > 0.5).sum() < N
    assert (R.labels("one_pos", N, 2) > 0.5).sum() == 1 and (R.labels("one_neg", N, 2) > 0.5).sum() == N - 1


def test_key_map_is_monotone_and_merges_the_zeros():
    """key(a) < key(b) exactly where a < b as float64, key(a) == key(b) exactly where a == b -- over every finite edge: +-0.0,
    the denormals next to them, +-FLT_MIN, +-1, +-FLT_MAX, +-inf and random bit patterns -- and no finite score has the
    positives' key."""
    rng = np.random.default_rng(7)
    edge = np.array([0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38, 1.0, -1.0, 0.5, 3.4028235e38, -3.4028235e38,
                     np.inf, -np.inf], np.float32)
    rnd = rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    a = np.concatenate([edge, rnd[~np.isnan(rnd)]])
    k = R.keys(a).astype(np.int64)
    d = a.astype(np.float64)
    assert np.array_equal(k[:, None] < k[None, :], d[:, None] < d[None, :])
    assert np.array_equal(k[:, None] == k[None, :], d[:, None] == d[None, :])
    assert R.keys(np.array([-0.0], np.float32))[0] == R.keys(np.array([0.0], np.float32))[0] == 0x80000000
    assert (k < R.POS_KEY).all()


@pytest.mark.parametrize("N", NS + [R.N_K14_CAP_PLUS_1, R.N_MANY_TILES, R.N_SCAN_RUNS_OF_2])
def test_tiled_summation_order_stays_inside_the_bar(N):
    """The kernel's order of adding the N float64 terms against numpy's mean of the same terms: within the derived bar."""
    worst = 0.0
    for sk in (["uniform", "eight", "wide"] if N < 100000 else ["uniform"]):
        for lk in ("mixed", "one_neg"):
            y, p = R.labels(lk, N, 3), R.scores(sk, N, 3)
            ref = R.reference(y, p)
            ll = R.tiled_sum(R.logloss_terms(y, p)) / N
            mse = R.tiled_sum(R.mse_terms(y, p)) / N
            worst = max(worst, R.ratio(ll, ref[0], N), R.ratio(mse, ref[2], N))
    print("N=%d: largest share of the bar %.3g" % (N, worst))
    assert worst <= 1.0


def test_the_bar_is_reachable_in_float64():
    """The bar is at least an ulp of the reference at every N -- a float64 result next to the reference passes, the bar does not
    ask for equal bits -- grows with N only through the depths, and stays below 2^-45 at the cap; the depths are those of the
    kernel's geometry."""
    assert R.depth_kernel(1) == R.depth_kernel(4096 * 256) == 35 and R.depth_kernel(4096 * 256 + 1) == 36
    assert R.depth_kernel(R.MAX_N) == 25 + 128 + 9
    assert R.depth_numpy(128) == 26 and R.depth_numpy(129) == 28 and R.depth_numpy(R.MAX_N) == 26 + 20 + 1
    last = 0.0
    for N in [1, 2, 128, 129, 4096, 4097, 1 << 18, 1 << 22, R.MAX_N]:
        rel = R.rel_bar(N)
        assert rel >= last and rel >= 6 * R.EPS
        last = rel
        for ref in (0.6931471805599453, 1e-9, 36.04):
            nxt = np.nextafter(ref, np.inf)
            assert nxt != ref and R.ratio(nxt, ref, N) <= 1.0
            assert R.ratio(ref * (1 + 2 * rel), ref, N) > 1.0
    assert R.rel_bar(R.MAX_N) < 2.0 ** -45
