"""Shared by the tests of K14w (csrc/eval_metrics_w.hip, the sample-weighted metrics of `evaluate` / `fit`): the float64
reference, the depths of the documented sum orders, the bounds derived from them, and seeded weight generators.

The reference everywhere is xdfm_amd.metrics' weighted_* numpy functions on (y, p.astype(float64), w.astype(float64)).  The
argument is that of tests/eval_metrics_ref.py (K14s), whose depths, cases and `same_bits` are reused, with one rounding more
per w * term product and the depth of the `cum` scan.

A sum of non-negative float64 terms formed by any tree of additions is off the exact sum by at most depth * 2^-53 of it (first
order).  With d = depth_kernel(N) (K14s's tiled order, which K14w keeps for every sum) and dn = depth_numpy(N) (numpy's
pairwise add.reduce):

LOGLOSS, MSE, ACCURACY are ratios S / W of two such sums, S = sum w * term and W = sum w:
    |got - ref| <= (2 * (d + dn) * 2^-53 + 7 * 2^-52) * |ref|
  numerator and denominator each differ by at most (d + dn) * 2^-53; what is not a sum is K14s's 6 * 2^-52 (the two logs, the
  division, the roundings of a soft label's products) and one more 2^-52 for the product with w: numpy rounds w * term, the
  kernel's fma does not, and the kernel rounds w * d in the mse.

AUC = (C * 0.5) / (Wpos * Wneg), C = sum over the positives of w_i * (cum[lb_i] + cum[ub_i]):
    |got - ref| <= (depth_cum_kernel(N) + N + 3 * (d + dn) + 8) * 2^-53 * ref
  cum[k] is a sum of at most n_neg <= N non-negative weights: the kernel's cell passes through depth_cum_kernel(N) additions
  (include/xdfm.h, K14w: 37 + 2 ceil(T / 256)), numpy's cumsum is sequential (up to N).  cum[lb] + cum[ub], the product with
  w_i, the product Wpos * Wneg and the division each round once per side (8); C, Wpos and Wneg are three sums in the two orders
  (3 * (d + dn)); C * 0.5 is exact.  numpy's sequential cumsum is what makes this bound grow with N; the kernel's share of it
  is a few dozen ulps.

EXACT CASES.  Weights that are multiples of 1/4 in [0, 4] and N <= 2^21: W, Wpos, Wneg, sum w * match are multiples of 1/4
below 2^23, every cum likewise, cum[lb] + cum[ub] < 2^24, a term below 2^26 and C a multiple of 1/16 below 2^47 (16 C < 2^51
< 2^53): every sum is exact in any order, Wpos * Wneg < 2^46 is exact, and the
accuracy and the AUC are one IEEE division of exact operands on both sides -- bit for bit.  Unit weights: the same, and the
kernel's logloss / mse are K14s's in bits as well (include/xdfm.h)."""
import numpy as np

import eval_metrics_ref as S
from xdfm_amd import metrics as M

LOGLOSS, AUC, MSE, ACC, ALL, SLOT = S.LOGLOSS, S.AUC, S.MSE, S.ACC, S.ALL, S.SLOT
same_bits = S.same_bits
MAX_N, TILE, THREADS = S.MAX_N, S.TILE, S.THREADS
# the sizes of the issue: 1, 2, a round of 64, a tile, each with a row less and more; three tiles; 258 tiles (a scan thread
# takes a run of 2 tiles in the radix scan and in the scan of the tiles' totals)
N_SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 4096 * 257 + 3]


def reference(y, p, w):
    """[logloss, auc, mse, accuracy] in float64; NaN where the host function raises (one class by weight) ."""
    y64, p64, w64 = np.asarray(y, np.float64), np.asarray(p, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    try:
        auc = M.weighted_roc_auc_score(y64, p64, w64)
    except ValueError:
        auc = float("nan")
    return [M.weighted_log_loss(y64, p64, w64), auc, M.weighted_mean_squared_error(y64, p64, w64),
            M.weighted_accuracy_score(y64, p64, w64)]


def depth_cum_kernel(N):
    tiles = (N + TILE - 1) // TILE
    return 37 + 2 * ((tiles + THREADS - 1) // THREADS)


def rel_bar(N):
    """logloss, mse, accuracy"""
    return 2 * (S.depth_kernel(N) + S.depth_numpy(N)) * 2.0 ** -53 + 7 * S.EPS


def rel_bar_auc(N):
    return (depth_cum_kernel(N) + N + 3 * (S.depth_kernel(N) + S.depth_numpy(N)) + 8) * 2.0 ** -53


def ratio(got, ref, N, slot):
    """|got - ref| as a share of the slot's bar; an exact match (NaN against NaN, inf against inf) counts 0."""
    if same_bits(got, ref) or (got != got and ref != ref):
        return 0.0
    bar = (rel_bar_auc(N) if slot == 1 else rel_bar(N)) * abs(ref)
    d = abs(got - ref)
    return d / bar if bar > 0 and d == d else float("inf")


# ------------------------------------------------------------------------------------------------------------ weights
WEIGHTS = ["dyadic", "unit", "uniform", "wide"]


def weights(kind, N, seed):
    rng = np.random.default_rng(5000 + seed)
    if kind == "unit":
        return np.ones(N, np.float32)
    if kind == "dyadic":                                   # multiples of 1/4 in [0, 4], about a fifth of them zero
        w = rng.integers(1, 17, N).astype(np.float32) / np.float32(4.0)
        w[rng.random(N) < 0.2] = 0.0
        return w
    if kind == "uniform":
        return rng.random(N).astype(np.float32)
    if kind == "wide":                                     # 2^-20 .. 2^20, a tenth of them zero
        w = np.exp2(rng.uniform(-20.0, 20.0, N)).astype(np.float32)
        w[rng.random(N) < 0.1] = 0.0
        return w
    raise KeyError(kind)


def pair_count_auc(y, p, w):
    """O(N^2) exact-fraction weighted AUC: sum over (positive i, other j) of w_i w_j ([p_i > p_j] + [p_i == p_j] / 2) over
    Wpos * Wneg, rounded once.  None when Wpos * Wneg == 0."""
    from fractions import Fraction
    y, p, w = np.asarray(y), np.asarray(p, np.float64), np.asarray(w, np.float64)
    pos = [i for i in range(y.size) if y[i] > 0.5 and w[i] > 0]
    neg = [j for j in range(y.size) if not y[j] > 0.5 and w[j] > 0]
    Wp, Wn = sum(Fraction(w[i]) for i in pos), sum(Fraction(w[j]) for j in neg)
    if Wp * Wn == 0:
        return None
    C = Fraction(0)
    for i in pos:
        inner = Fraction(0)
        for j in neg:
            if p[i] > p[j]:
                inner += Fraction(w[j])
            elif p[i] == p[j]:
                inner += Fraction(w[j]) / 2
        C += Fraction(w[i]) * inner
    return float(C / (Wp * Wn))
