"""CPU: the arithmetic K14 (csrc/metrics.hip) is built on, checked against the pinned numpy metrics without a kernel
(tests/metrics_ref.py): the pair-count form of the AUC has the bits of the mid-rank form, a blocked summation order stays
inside the logloss / mse bar, and the sklearn golden is reproduced."""
import numpy as np
import pytest

from conftest import load_golden

import metrics_ref as R
from xdfm_amd import metrics as M


@pytest.mark.parametrize("B", R.B_LIST)
def test_pair_count_auc_has_the_bits_of_roc_auc_score(B):
    """Every generated case: 2 [p_i > p_j] + [p_i == p_j] over (positive, other) pairs, halved and divided once, equals the
    mid-rank Mann-Whitney value bit for bit; all-equal scores give exactly 0.5; a single class gives NaN."""
    seen = 0
    for sk, lk, y, p in R.cases(B):
        if lk == "soft":
            continue
        got, want = R.pair_auc(y, p), R.reference(y, p)[1]
        assert R.same_bits(got, want), (B, sk, lk, got, want)
        pos = int((y > 0.5).sum())
        if pos in (0, B):
            assert got != got, (B, sk, lk)
        elif sk == "equal":
            assert got == 0.5, (B, lk, got)
        seen += 1
    assert seen == len(R.SCORES) * (len(R.LABELS) - 1)


@pytest.mark.parametrize("B", R.B_LIST + [R.MAX_B])
def test_blocked_summation_order_stays_inside_the_bar(B):
    """The kernel's order of adding the B float64 terms (tile of 512, two rows per thread, xor tree, waves in order, the same
    tree over the tiles) against numpy's mean of the same terms: within (B + 4) * 2^-52 * ref, with room to spare."""
    worst = 0.0
    for sk, lk, y, p in R.cases(B):
        ref = R.reference(y, p)
        ll = -(R.blocked_sum(R.logloss_terms(y, p)) / B)
        mse = R.blocked_sum(R.mse_terms(y, p)) / B
        worst = max(worst, R.ratio(ll, ref[0], B), R.ratio(mse, ref[2], B))
    print("B=%d: largest share of the bar %.3g" % (B, worst))
    assert worst <= 1.0


def test_sklearn_golden_is_reproduced():
    """tests/golden/metrics.npz, the (y, p, auc, logloss) test_host_logic.py pins M.* to: the pair count gives that AUC, the
    blocked sum that logloss."""
    g = load_golden("metrics")
    y, p = g["y"], g["p"]
    assert abs(R.pair_auc(y, p) - float(g["auc"])) < 1e-12
    assert R.same_bits(R.pair_auc(y, p), M.roc_auc_score(y, p))
    ll = -(R.blocked_sum(R.logloss_terms(y, np.asarray(p, np.float64))) / y.size)
    assert abs(ll - float(g["logloss"])) < 1e-12


def test_fp32_compares_equal_float64_compares():
    """The kernel compares the fp32 scores; the reference their float64 images: the conversion is exact and monotone."""
    rng = np.random.default_rng(5)
    a = rng.random(4096).astype(np.float32)
    a[::7] = a[3]
    b = np.roll(a, 11)
    assert np.array_equal(a > b, a.astype(np.float64) > b.astype(np.float64))
    assert np.array_equal(a == b, a.astype(np.float64) == b.astype(np.float64))
