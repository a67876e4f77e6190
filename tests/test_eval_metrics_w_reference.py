"""CPU: the weighted numpy metrics of xdfm_amd.metrics (the definitions K14w, csrc/eval_metrics_w.hip, is held to) without a
kernel: against an O(N^2) pair count in exact fractions, against their unweighted namesakes under unit weights, against the
rows repeated for integer weights, against sklearn's sample_weight= versions where it is installed, and the error cases."""
import numpy as np
import pytest

import eval_metrics_ref as S
import eval_metrics_w_ref as R
from xdfm_amd import metrics as M

ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


def _auc(y, p, w):
    try:
        return M.weighted_roc_auc_score(y, p, w)
    except ValueError:
        return None


@pytest.mark.parametrize("N", [1, 2, 3, 17, 64, 300])
@pytest.mark.parametrize("sk", ["uniform", "eight", "equal", "zeros", "wide"])
def test_auc_is_the_exact_pair_count(N, sk):
    """Weights that are multiples of 1/4 (a fifth of them zero): every float64 sum is exact, so the value is the rational one
    rounded once -- bit for bit.  Ties ('eight', 'equal'), +-0.0 ('zeros'), negative scores and +-inf ('wide')."""
    for lk in ("mixed", "one_pos", "one_neg"):
        y, p = S.labels(lk, N, N + 3), S.scores(sk, N, N + 3).astype(np.float64)
        w = R.weights("dyadic", N, N)
        want, got = R.pair_count_auc(y, p, w), _auc(y, p, w)
        assert (want is None and got is None) or R.same_bits(got, want), (N, sk, lk, got, want)
    w = R.weights("uniform", N, 1).astype(np.float64)          # general weights: within the derived bar of the exact value
    y, p = S.labels("mixed", N, 5), S.scores(sk, N, 5).astype(np.float64)
    want, got = R.pair_count_auc(y, p, w), _auc(y, p, w)
    assert (want is None and got is None) or abs(got - want) <= R.rel_bar_auc(N) * want


@pytest.mark.parametrize("N", [1, 2, 65, 300, 4097])
@pytest.mark.parametrize("sk", ["uniform", "eight", "zeros"])
def test_unit_weights_give_the_unweighted_bits(N, sk):
    y, p = S.labels("mixed", N, 11), S.scores(sk, N, 11).astype(np.float64)
    one = np.ones(N, np.float32)
    assert R.same_bits(M.weighted_log_loss(y, p, one), M.log_loss(y, p))
    assert R.same_bits(M.weighted_mean_squared_error(y, p, one), M.mean_squared_error(y, p))
    assert R.same_bits(M.weighted_accuracy_score(y, p, one), M.accuracy_score(y, np.where(p > 0.5, 1, 0)))
    if 0 < (y > 0.5).sum() < N:
        assert R.same_bits(M.weighted_roc_auc_score(y, p, one), M.roc_auc_score(y, p))
    else:
        assert _auc(y, p, one) is None


@pytest.mark.parametrize("N", [2, 65, 300])
def test_an_integer_weight_is_the_row_repeated(N):
    rng = np.random.default_rng(N)
    y, p = S.labels("mixed", N, 13), S.scores("eight", N, 13).astype(np.float64)
    k = rng.integers(0, 4, N)
    yr, pr = np.repeat(y, k), np.repeat(p, k)
    if 0 < (yr > 0.5).sum() < yr.size:
        assert R.same_bits(M.weighted_roc_auc_score(y, p, k), M.roc_auc_score(yr, pr))
    assert R.same_bits(M.weighted_accuracy_score(y, p, k), M.accuracy_score(yr, np.where(pr > 0.5, 1, 0)))


@pytest.mark.parametrize("N", [2, 300, 4096])
@pytest.mark.parametrize("kind", ["dyadic", "uniform", "wide"])
def test_against_sklearn(N, kind):
    sk = pytest.importorskip("sklearn.metrics")
    y, p = S.labels("mixed", N, 17), np.clip(S.scores("uniform", N, 17).astype(np.float64), 1e-6, 1 - 1e-6)
    w = R.weights(kind, N, 17).astype(np.float64)
    w[:2] = 1.0                                            # both classes keep weight at N = 2
    y[:2] = [0.0, 1.0]
    bar = (N + 8) * 2.0 ** -52
    pairs = [(M.weighted_log_loss(y, p, w), sk.log_loss(y, p, sample_weight=w)),
             (M.weighted_roc_auc_score(y, p, w), sk.roc_auc_score(y, p, sample_weight=w)),
             (M.weighted_mean_squared_error(y, p, w), sk.mean_squared_error(y, p, sample_weight=w)),
             (M.weighted_accuracy_score(y, p, w), sk.accuracy_score(y, np.where(p > 0.5, 1.0, 0.0), sample_weight=w))]
    for got, want in pairs:
        assert abs(got - want) <= bar * abs(want), (N, kind, got, want)


def test_zero_weight_rows_are_selected_away():
    y, p = S.labels("mixed", 100, 19), S.scores("uniform", 100, 19).astype(np.float64)
    w = R.weights("dyadic", 100, 19)
    w[7] = w[8] = 0.0
    want = R.reference(y, p.astype(np.float32), w)
    p2 = p.astype(np.float32).copy()
    p2[7], p2[8] = np.nan, np.inf
    got = R.reference(y, p2, w)
    assert all(R.same_bits(a, b) for a, b in zip(got, want))
    w[7] = 0.5                                             # the NaN counts now
    assert all(v != v for v in R.reference(y, p2, w)[:3])


def test_one_class_and_zero_weight():
    y, p = S.labels("mixed", 50, 23), S.scores("uniform", 50, 23).astype(np.float64)
    for w in (np.zeros(50), np.where(y > 0.5, 0.0, 1.0), np.where(y > 0.5, 1.0, 0.0)):
        with pytest.raises(ValueError) as e:
            M.weighted_roc_auc_score(y, p, w)
        assert str(e.value) == ONE_CLASS
    for cls in (0.0, 1.0):
        with pytest.raises(ValueError):
            M.weighted_roc_auc_score(np.full(50, cls), p, np.ones(50))
    zero = np.zeros(50)
    assert all(v != v for v in (M.weighted_log_loss(y, p, zero), M.weighted_mean_squared_error(y, p, zero),
                                M.weighted_accuracy_score(y, p, zero)))
    with pytest.raises(ValueError, match="weights"):
        M.weighted_log_loss(y, p, np.ones(49))


def test_the_bars_grow_with_the_depths():
    assert R.depth_cum_kernel(1) == 39 and R.depth_cum_kernel(4096 * 257 + 3) == 41
    assert R.rel_bar(1 << 20) < 2e-14 and R.rel_bar_auc(4096) < 1e-12
    assert all(R.rel_bar(a) <= R.rel_bar(b) and R.rel_bar_auc(a) < R.rel_bar_auc(b) for a, b in zip(R.N_SIZES, R.N_SIZES[1:]))
