"""CPU: the row-wise Adagrad reference (tests/rowwise_ref.py) -- the fp32 mirror rw_f32 against float64 one step at a time, on
every case, with and without the L2 term; the constant C of the bar against the measured worst ratio; the zero-gradient rule;
D = 1 against the Adagrad formula; a hand-computed 2 x 2 case; the documented summation order."""
import math

import numpy as np

import opt_ref as R
import rowwise_ref as W

F32 = W.F32


def test_the_mirror_is_within_the_bar_of_float64_and_c_is_twice_its_worst_ratio():
    """Ten steps per case, the state carried by the mirror, every step also taken in float64 from the fp32 state it started
    with.  The worst ratio of |error of p| to 2^-24 (|p| + |U|) is printed and must be what rowwise_ref.py records (C is twice
    it, rounded up); nothing becomes NaN, the underflow row included."""
    worst_p = worst_s = 0.0
    for with_l2 in (False, True):
        l2m = W.L2_A if with_l2 else W.L2_0
        for st, row in enumerate(W.mirror_run(with_l2), 1):
            for t, (p0, s0, g, p1, s1, _) in enumerate(row):
                assert np.isfinite(p1).all() and np.isfinite(s1).all(), (with_l2, st, W.CASES[t])
                rp, rs = W.ratios(p1, s1, p0, s0, g, W.lr_of(st)[0], l2m[t], W.EPS)
                worst_p, worst_s = max(worst_p, rp), max(worst_s, rs)
    print("row-wise mirror against float64: worst ratio p %.4f, s %.4f; C = %g" % (worst_p, worst_s, W.C_BAR))
    assert worst_p <= W.WORST_MEASURED and worst_s <= W.WORST_MEASURED          # what C was set from still holds
    assert W.C_BAR == math.ceil(2.0 * W.WORST_MEASURED) and W.C_BAR <= 2 * 6    # (the count of roundings allows 6)
    assert worst_p > 0.5 * W.WORST_MEASURED                                     # ... and the record is not a loose one


def test_a_row_without_a_gradient_keeps_its_bits():
    rng = np.random.RandomState(0)
    p = (rng.randn(6, 8) * 0.05).astype(F32)
    p[4, 3] = F32(-0.0)
    s = np.array([0.0, 1e-4, 0.5, -0.0, 0.0, 3.0], F32)
    g = (rng.randn(6, 8)).astype(F32)
    g[[0, 3, 4]] = 0.0
    g[4, 3] = F32(-0.0)                                    # -0 gradient on a -0 weight: fma(-lr, -0 / den, -0) would be +0
    p1, s1, _ = W.rw_f32(p, s, g, 0.01, 0.0, 1e-10)
    for r in (0, 3, 4):
        assert np.array_equal(W.bits(p1[r]), W.bits(p[r])) and W.bits(s1[r:r + 1])[0] == W.bits(s[r:r + 1])[0]
    for r in (1, 2, 5):
        assert (p1[r] != p[r]).all() and s1[r] > s[r]
    # with an L2 term the row moves by 2 l2m p alone
    p2, s2, value = W.rw_f32(p, s, g, 0.01, 1e-3, 1e-10)
    assert (p2[0] != p[0]).any() and s2[0] > 0
    assert abs(value - 1e-3 * float((p.astype(np.float64) ** 2).sum())) <= 1e-6 * value
    # the underflow row: |g| = 1e-25 at s = 0 -- ms is 0 in fp32, s stays 0, p moves by lr g / eps, nothing is NaN
    g3 = np.full((1, 4), 1e-25, F32)
    p3, s3, _ = W.rw_f32(np.ones((1, 4), F32), np.zeros(1, F32), g3, 0.01, 0.0, 1e-10)
    assert s3[0] == 0 and np.isfinite(p3).all() and (p3 == 1.0).all()          # 1 - 1e-17 rounds to 1
    w3 = W.rw_f64(np.ones((1, 4)), np.zeros(1), g3, 0.01, 0.0, 1e-10)
    assert 0 < w3[1][0] < 1e-49 and np.isfinite(w3[0]).all()                   # double keeps the mean of the squares


def test_dim_one_is_the_adagrad_formula():
    rng = np.random.RandomState(1)
    p, s, g = (rng.randn(37, 1) * 0.05).astype(F32), (rng.rand(37) * 1e-3).astype(F32), rng.randn(37, 1).astype(F32)
    for l2m in (0.0, 1e-3):
        p1, s1, v1 = W.rw_f32(p, s, g, 0.01, l2m, 1e-10)
        q1, t1, w1 = R.opt_f32("adagrad", p[:, 0], s, g[:, 0], 0.01, l2m, 1e-10, 0.0)
        assert np.array_equal(W.bits(p1[:, 0]), W.bits(q1)) and np.array_equal(W.bits(s1), W.bits(t1)) and v1 == w1
        a = W.rw_f64(p, s, g, 0.01, l2m, 1e-10)
        b = R.opt_f64("adagrad", p[:, 0], s, g[:, 0], 0.01, l2m, 1e-10, 0.0)
        assert np.allclose(a[0][:, 0], b[0], rtol=1e-14, atol=0) and np.allclose(a[1], b[1], rtol=1e-14, atol=0)


def test_a_hand_computed_two_by_two_case():
    """p = [[1, 2], [3, 4]], g = [[3, 4], [0, 0]], s = [0, 1], lr = 0.5, eps -> 0, no L2 term: row 0 has ms = (9 + 16) / 2 = 12.5,
    den = sqrt(12.5), p' = p - 0.5 g / den; row 1 has no gradient and stays."""
    p = np.array([[1.0, 2.0], [3.0, 4.0]])
    g = np.array([[3.0, 4.0], [0.0, 0.0]])
    s = np.array([0.0, 1.0])
    den = math.sqrt(12.5)
    want_p = np.array([[1.0 - 1.5 / den, 2.0 - 2.0 / den], [3.0, 4.0]])
    p1, s1, value, upd = W.rw_f64(p, s, g, 0.5, 0.0, 1e-30)
    assert np.allclose(p1, want_p, rtol=1e-15) and np.allclose(s1, [12.5, 1.0]) and value == 0.0
    q1, t1, _ = W.rw_f32(p, s, g, 0.5, 0.0, 1e-30)
    assert np.allclose(q1, want_p, rtol=3e-7) and t1[0] == F32(12.5) and t1[1] == 1.0
    assert np.array_equal(q1[1], p[1].astype(F32))
    # with l2m = 0.25: g' = g + 0.5 p = [[3.5, 5], [1.5, 2]]; the value is 0.25 * 30
    p2, s2, value, _ = W.rw_f64(p, s, g, 0.5, 0.25, 1e-30)
    assert value == 7.5 and np.allclose(s2, [(3.5 ** 2 + 25.0) / 2.0, 1.0 + (2.25 + 4.0) / 2.0])
    assert np.allclose(p2[1], [3.0 - 0.5 * 1.5 / math.sqrt(s2[1]), 4.0 - 0.5 * 2.0 / math.sqrt(s2[1])])


def test_the_summation_order_is_the_documented_one():
    """Chunks of four left to right, then a balanced tree over the chunk sums padded to a power of two, neighbouring pairs
    first -- spelled out by hand for D = 10 (three chunks, the last of two elements) and D = 16."""
    rng = np.random.RandomState(2)
    x = rng.rand(1, 10) * np.array([1e16, 1.0] * 5)          # magnitudes far apart: the order shows in the last bits
    c0 = ((x[0, 0] + x[0, 1]) + x[0, 2]) + x[0, 3]
    c1 = ((x[0, 4] + x[0, 5]) + x[0, 6]) + x[0, 7]
    c2 = x[0, 8] + x[0, 9]
    assert W.tree_sum(x)[0] == (c0 + c1) + (c2 + 0.0)
    y = rng.rand(3, 16) * np.array([1e16, 1.0, 1e-8, 1e8] * 4)
    c = [((y[:, 4 * j] + y[:, 4 * j + 1]) + y[:, 4 * j + 2]) + y[:, 4 * j + 3] for j in range(4)]
    assert np.array_equal(W.tree_sum(y), (c[0] + c[1]) + (c[2] + c[3]))
    assert W.tree_sum(np.array([[5.0]]))[0] == 5.0
