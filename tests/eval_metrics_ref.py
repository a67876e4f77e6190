"""Shared by the tests of K14s (csrc/eval_metrics.hip, the metrics of `evaluate` for any row count): a numpy mirror of the
kernel's key map, of its "sort the non-positives, two bounds per positive" count and of its summation order, seeded case
generators, and the bar for logloss / mse.

The reference everywhere is xdfm_amd.metrics' numpy functions on (y, p.astype(float64)), as for K14 (tests/metrics_ref.py,
whose `reference`, `same_bits` and bit names are reused).

THE BAR for logloss and mse: |got - ref| <= ((d_kernel(N) + d_numpy(N)) * 2^-53 + 6 * 2^-52) * ref.
Both are means of N non-negative float64 terms.  A sum of non-negative terms formed by any tree of additions is off the exact
sum by at most depth * 2^-53 of it (first order: every term passes through at most `depth` roundings of relative size 2^-53,
and no partial sum exceeds the total), so the two sums differ by at most (d_kernel + d_numpy) * 2^-53 * ref.
  d_kernel  a term's way through the kernel (include/xdfm.h, K14s): 16 additions into its thread's accumulator, 6 of the xor
            tree, 3 over the waves (25 in the tile); then ceil(T / 256) additions into the finish thread's accumulator over
            T = ceil(N / 4096) tiles, 6 and 3 again.
  d_numpy   numpy's pairwise add.reduce: blocks of at most 128 terms are added by 8 accumulators (16 deep), combined (3) and
            followed by up to 7 leftover terms in sequence (26 in all); the blocks are halved recursively above that:
            ceil(log2(N / 128)) levels, and one more because the halves are rounded to multiples of 8.
  6 * 2^-52 what is not the sum.  The device's log against numpy's, each within an ulp (2^-52 relative at most): 2 * 2^-52.
            The division by N on either side: 2 * 2^-53.  With soft labels the two products and their sum round values that
            already differ: 3 roundings a side, 3 * 2^-52.  Squared terms ((d_kernel + d_numpy) * 2^-53)^2 < 2^-90 vanish in
            the slack.
The bar is a few dozen ulps at every N (42.5 * 2^-52 at N = 2^18, 110.5 * 2^-52 at the cap of 2^27): far below K14's
(B + 4) * 2^-52, which assumed nothing about the order."""
import math

import numpy as np

import metrics_ref as K14
from xdfm_amd import metrics as M

LOGLOSS, AUC, MSE, ACC, ALL, SLOT = K14.LOGLOSS, K14.AUC, K14.MSE, K14.ACC, K14.ALL, K14.SLOT
same_bits, reference = K14.same_bits, K14.reference
MAX_N = 1 << 27
TILE, THREADS = 4096, 256
EPS = 2.0 ** -52
POS_KEY = 0xFFFFFFFF

# 1 and 2; round (64), workgroup (256), a wave's keys in the scatter (1024) and the tile (4096) with one row less and one more;
# two tiles and one row; one above K14's cap; 74 tiles (many workgroups per radix pass)
N_EDGES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
N_K14_CAP_PLUS_1 = 65537
N_MANY_TILES = 300001
# the scan of a radix pass gives a thread ceil(T / 256) consecutive tiles: 257 tiles is the first N with runs of 2
N_SCAN_RUNS_OF_2 = 256 * TILE + 1


# ------------------------------------------------------------------------------------------------------------ key map
def keys(p):
    """The kernel's order-preserving u32 image of fp32 scores: the sign bit flipped for non-negative values, all bits for
    negative ones, and -0.0 taken as +0.0."""
    p = np.ascontiguousarray(p, np.float32)
    u = p.view(np.uint32).copy()
    u[p == 0.0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def sort_auc(y, p):
    """The kernel's AUC restated: positives take the key 0xFFFFFFFF, the N keys are sorted, n_neg is where that run begins,
    every positive's own key takes a lower and an upper bound in [0, n_neg): C = sum (lower + upper), then
    (C * 0.5) / (float(n_pos) * float(n_neg)).  NaN for a NaN score."""
    y = np.asarray(y).ravel()
    p = np.asarray(p, np.float32).ravel()
    pos = y > 0.5
    k = keys(p)
    s = np.sort(np.where(pos, np.uint32(POS_KEY), k), kind="stable")
    if np.isnan(p).any():
        return float("nan")
    n_neg = int(np.searchsorted(s, np.uint32(POS_KEY), side="left"))
    neg = s[:n_neg]
    kp = k[pos]
    C = int(np.searchsorted(neg, kp, side="left").astype(np.int64).sum()) + int(np.searchsorted(neg, kp, side="right").astype(np.int64).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(C * 0.5) / (np.float64(kp.size) * np.float64(n_neg)))


# ------------------------------------------------------------------------------------------------------------ sums
def _tree(acc):
    """xdfm_block_sum_f64 over rows of 256 accumulators: a xor tree inside each wave of 64, then the 4 waves in order."""
    w = np.asarray(acc, np.float64).reshape(-1, 4, 64).copy()
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ off]
    s = w[:, 0, 0]
    for k in range(1, 4):
        s = s + w[:, k, 0]
    return s


def tiled_sum(terms):
    """The order K14s adds N float64 terms in: thread t of a tile adds rows t, t + 256, ... (16 of them) in index order, _tree
    adds the tile's threads; finish thread t adds tiles t, t + 256, ... in index order, _tree adds the finish's threads."""
    t = np.asarray(terms, np.float64)
    n_tiles = (t.size + TILE - 1) // TILE
    pad = np.zeros(n_tiles * TILE, np.float64)
    pad[:t.size] = t
    rows = pad.reshape(n_tiles, TILE // THREADS, THREADS)
    acc = np.zeros((n_tiles, THREADS), np.float64)
    for r in range(TILE // THREADS):
        acc = acc + rows[:, r, :]
    parts = _tree(acc)
    rounds = (n_tiles + THREADS - 1) // THREADS
    pp = np.zeros(rounds * THREADS, np.float64)
    pp[:n_tiles] = parts
    fin = np.zeros(THREADS, np.float64)
    for r in pp.reshape(rounds, THREADS):
        fin = fin + r
    return float(_tree(fin)[0])


def depth_kernel(N):
    tiles = (N + TILE - 1) // TILE
    return 16 + 6 + 3 + (tiles + THREADS - 1) // THREADS + 6 + 3


def depth_numpy(N):
    return 26 + (math.ceil(math.log2(N / 128.0)) + 1 if N > 128 else 0)


def rel_bar(N):
    return (depth_kernel(N) + depth_numpy(N)) * 2.0 ** -53 + 6 * EPS


def bar(N, ref):
    return rel_bar(N) * abs(ref)


def ratio(got, ref, N):
    """|got - ref| as a share of the bar; an exact match counts 0 whatever the reference (a bar of 0 for ref == 0)."""
    if same_bits(got, ref):                                # also inf against inf (a score of +-inf in the mse)
        return 0.0
    d = abs(got - ref)
    return d / bar(N, ref) if ref != 0.0 else float("inf")


# ------------------------------------------------------------------------------------------------------------ cases
SCORES = ["uniform", "eight", "equal", "byte0", "byte1", "byte2", "byte3", "zeros", "denormal", "wide"]
LABELS = ["mixed", "pos_first", "pos_last", "alternating", "one_pos", "one_neg"]


def scores(kind, N, seed):
    rng = np.random.default_rng(3000 + seed)
    if kind == "uniform":
        return rng.random(N).astype(np.float32)
    if kind == "eight":                                    # 8 distinct values: long tie runs across the classes
        return (rng.integers(0, 8, N).astype(np.float32) + 0.5) / 8.0
    if kind == "equal":
        return np.full(N, 0.37, np.float32)
    if kind.startswith("byte"):                            # finite patterns that differ in ONE byte of the key only: a radix
        k = int(kind[4:])                                  # pass that is skipped or out of order leaves them unsorted
        base = 0x3F2A5C71 & ~(0xFF << (8 * k))             # 0.6655...; byte 3 takes 0x3C..0x3F (0.0104 .. 0.6655): all in (0, 1)
        digit = rng.integers(0x3C, 0x40, N) if k == 3 else rng.integers(0, 256, N)
        return (np.uint32(base) | (digit.astype(np.uint32) << np.uint32(8 * k))).astype(np.uint32).view(np.float32)
    if kind == "zeros":                                    # +0.0, -0.0 and their nearest neighbours: the two zeros tie
        return rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 0.25], np.float32), N)
    if kind == "denormal":
        return (rng.integers(-40, 41, N).astype(np.float32) * np.float32(1e-45)).astype(np.float32)
    if kind == "wide":                                     # negative scores and scores above 1, with +-inf at the ends
        p = (4.0 * rng.standard_normal(N)).astype(np.float32)
        p[0] = np.inf
        p[-1] = -np.inf
        return p
    raise KeyError(kind)


def labels(kind, N, seed):
    rng = np.random.default_rng(4000 + seed)
    if kind == "mixed":
        return K14.labels("mixed", N, seed)
    n_pos = min(max(1, int(0.3 * N)), N - 1) if N > 1 else 1
    y = np.zeros(N, np.float32)
    if kind == "pos_first":
        y[:n_pos] = 1.0
    elif kind == "pos_last":
        y[N - n_pos:] = 1.0
    elif kind == "alternating":
        y[::2] = 1.0
    elif kind == "one_pos":
        y[int(rng.integers(0, N))] = 1.0
    elif kind == "one_neg":
        y[:] = 1.0
        y[int(rng.integers(0, N))] = 0.0
    else:
        raise KeyError(kind)
    return y


def cases(N, score_kinds=SCORES, label_kinds=LABELS):
    for si, sk in enumerate(score_kinds):
        for li, lk in enumerate(label_kinds):
            seed = (N * 31 + si * 7 + li) % 100003
            yield sk, lk, labels(lk, N, seed), scores(sk, N, seed)


def logloss_terms(y, p):
    return -K14.logloss_terms(y, p)


mse_terms = K14.mse_terms
roc_auc_score = M.roc_auc_score
