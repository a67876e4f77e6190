"""Shared by the tests of K14 (csrc/metrics.hip, the per-batch training metrics): seeded case generators, the reference values,
a pair-count mirror of the kernel's AUC for small B, a mirror of its summation order, and the bar for logloss / mse.

The reference everywhere is xdfm_amd.metrics' numpy functions on (y, p.astype(float64)) -- the project's pinned definition
(tests/test_host_logic.py, tests/golden/metrics.npz).

THE BAR for logloss and mse: |got - ref| <= (B + 4) * 2^-52 * ref.  Both are means of B non-negative float64 terms.  Summing B
non-negative terms in any order costs at most (B - 1) * 2^-53 * sum relative to the exact sum, on each side (the kernel's
blocked order, numpy's pairwise one): (B - 1) * 2^-52 together.  The `+ 4` (+ 5 * 2^-52 in all) covers what is not the sum:
the device's log against numpy's (both within an ulp), the rounding of the products and of the division by B.  AUC and
accuracy have no bar: integers and one IEEE division, bit for bit."""
import numpy as np

from xdfm_amd import metrics as M

LOGLOSS, AUC, MSE, ACC = 1, 2, 4, 8
ALL = 15
SLOT = {LOGLOSS: 0, AUC: 1, MSE: 2, ACC: 3}
MAX_B = 65536
# every power-of-two tile edge from 64 to 8192 is straddled; several tiles in both grid dimensions whatever the tile
B_LIST = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 2047, 2049, 4095, 4097, 8195]
SCORES = ["uniform", "eight", "equal", "sigmoid"]
LABELS = ["mixed", "one_pos", "one_neg", "one_class", "soft"]
EPS = 2.0 ** -52


def scores(kind, B, seed):
    rng = np.random.default_rng(1000 + seed)
    if kind == "uniform":
        return rng.random(B).astype(np.float32)
    if kind == "eight":                                    # 8 distinct values: many ties, also across the classes
        return (rng.integers(0, 8, B).astype(np.float32) + 0.5) / 8.0
    if kind == "equal":
        return np.full(B, 0.37, np.float32)
    if kind == "sigmoid":                                  # wide logits: fp32 saturates, exact 0.0f and 1.0f present (the clamp)
        z = (30.0 * rng.standard_normal(B)).astype(np.float32)
        with np.errstate(over="ignore"):
            p = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
        p[0] = 0.0
        p[-1] = 1.0
        return p
    raise KeyError(kind)


def labels(kind, B, seed):
    rng = np.random.default_rng(2000 + seed)
    if kind == "mixed":                                    # about 30 % positive, both classes present from B = 2 on
        y = (rng.random(B) < 0.3).astype(np.float32)
        y[0] = 1.0
        y[-1] = 0.0 if B > 1 else y[-1]
        return y
    if kind == "one_pos":
        y = np.zeros(B, np.float32)
        y[int(rng.integers(0, B))] = 1.0
        return y
    if kind == "one_neg":
        y = np.ones(B, np.float32)
        y[int(rng.integers(0, B))] = 0.0
        return y
    if kind == "one_class":
        return np.full(B, float(seed % 2), np.float32)
    if kind == "soft":                                     # for logloss / mse only: y is a factor there, not a class
        return rng.choice(np.array([0.0, 0.3, 0.7, 1.0], np.float32), B)
    raise KeyError(kind)


def which_of(label_kind):
    return LOGLOSS | MSE if label_kind == "soft" else ALL


def cases(B):
    """(score kind, label kind, y, p) for every combination, seeded by B and the kinds."""
    for si, sk in enumerate(SCORES):
        for li, lk in enumerate(LABELS):
            seed = B * 31 + si * 7 + li
            yield sk, lk, labels(lk, B, seed), scores(sk, B, seed)


def reference(y, p):
    """[logloss, auc, mse, accuracy] of the pinned numpy functions on (y, float64(p)); auc = NaN for a single class (where
    roc_auc_score raises and the device leaves NaN)."""
    pd = p.astype(np.float64)
    pos = int((y > 0.5).sum())
    auc = M.roc_auc_score(y, pd) if 0 < pos < y.size else float("nan")
    acc = M.accuracy_score(y, np.where(p > 0.5, 1, 0))
    return [M.log_loss(y, pd), auc, M.mean_squared_error(y, pd), acc]


def bar(B, ref):
    return (B + 4) * EPS * abs(ref)


def ratio(got, ref, B):
    """|got - ref| as a share of the bar; an exact match counts 0 whatever the reference (a bar of 0 for ref == 0)."""
    d = abs(got - ref)
    if d == 0.0:
        return 0.0
    return d / bar(B, ref) if ref != 0.0 else float("inf")


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (a != a and b != b)


def pair_auc(y, p, chunk=512):
    """The kernel's AUC restated: C = sum over (i positive, j not) of 2 [p_i > p_j] + [p_i == p_j] in integers, then
    (C * 0.5) / (float(n_pos) * float(n_neg)).  O(B^2): for small B."""
    y = np.asarray(y).ravel()
    p = np.asarray(p).ravel()
    pos = y > 0.5
    P, N = p[pos], p[~pos]
    if np.isnan(p).any():
        return float("nan")
    C = 0
    for a in range(0, P.size, chunk):
        blk = P[a:a + chunk, None]
        C += 2 * int((blk > N[None, :]).sum()) + int((blk == N[None, :]).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(C * 0.5) / (np.float64(P.size) * np.float64(N.size)))


def logloss_terms(y, p):
    y = y.astype(np.float64)
    pc = np.clip(p.astype(np.float64), EPS, 1 - EPS)
    return y * np.log(pc) + (1 - y) * np.log(1 - pc)


def mse_terms(y, p):
    d = y.astype(np.float64) - p.astype(np.float64)
    return d * d


def _block_tree(v):
    """xdfm_block_sum_f64 over 256 threads: a xor tree inside each wave of 64, then the waves in index order."""
    w = np.asarray(v, np.float64).reshape(4, 64).copy()
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ off]
    s = w[0, 0]
    for k in range(1, 4):
        s = s + w[k, 0]
    return s


def blocked_sum(terms, tile=512, threads=256):
    """The order K14 adds B float64 terms in: a thread adds its rows t, t + 256 of a 512-row tile in index order, the tile's
    threads go through _block_tree, the finish gives tile k to thread k and runs _block_tree again."""
    t = np.asarray(terms, np.float64)
    n_tiles = (t.size + tile - 1) // tile
    assert n_tiles <= threads
    pad = np.zeros(n_tiles * tile, np.float64)
    pad[:t.size] = t
    parts = np.zeros(threads, np.float64)
    for k in range(n_tiles):
        rows = pad[k * tile:(k + 1) * tile].reshape(tile // threads, threads)
        acc = np.zeros(threads, np.float64)
        for r in rows:
            acc = acc + r
        parts[k] = _block_tree(acc)
    return _block_tree(parts)
