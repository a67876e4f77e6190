"""What the PReLU tests (the _prelu entry points of csrc/dnn.hip, csrc/prelu.hip) share: the float64 reference of the layer
and of the elementwise op, the case tables of tests/test_gpu_dnn_prelu_abi.py and the builders of integer-valued cases whose
sums are exact in fp32 in any order.  No GPU needed; checked by tests/test_dnn_prelu_reference.py.

Semantics (torch's prelu, one scalar slope):  y = z > 0 ? z : alpha * z,  gz = z > 0 ? g : alpha * g,
dalpha = sum over z <= 0 of g * z  (a cell with z == 0 takes the alpha branch and adds 0)."""
import numpy as np

ALPHAS = (0.25, 0.0, -0.5, 2.0, 1.0)
#  (rows, in, out): the smallest shapes that reach each edge of the dense template
DENSE_CASES = {
    "min": (1, 1, 32),
    "ragged": (63, 13, 32),
    "two_row_tiles": (65, 40, 64),
    "split_edge_1": (256, 37, 96),       # one split; a half-full tile of out in dW
    "split_edge_2": (257, 37, 96),       # two
    "three_splits": (520, 40, 64),
    "tiles_3x2": (300, 65, 160),         # three tiles of out, two of in
    "long_splits": (8200, 5, 96),        # more than 32 raw splits: 288 rows each
}
ELEMENTWISE_CASES = ((1, 1), (3, 31), (64, 64), (65, 65), (257, 40), (4100, 33))
EXACT_LIMIT = 1 << 24                    # integers below it are fp32 values, and so is every partial sum
UNIT = 4                                 # the slopes are multiples of 1 / UNIT, at most 2 in magnitude


def prelu_ref(u, alpha):
    """y in float64 (+0.0 normalised: alpha * -0.0 and 0 * negative leave signed zeros behind, the sums of a kernel do too)."""
    u = np.asarray(u, dtype=np.float64)
    return np.where(u > 0, u, float(alpha) * u)


def prelu_bwd_ref(g, u, alpha):
    """(du, dalpha) in float64."""
    g, u = np.asarray(g, dtype=np.float64), np.asarray(u, dtype=np.float64)
    du = np.where(u > 0, g, float(alpha) * g)
    return du, float(np.sum(np.where(u <= 0, g * u, 0.0)))


def layer_ref(x, W, b, alpha):
    """(y, z) of y = prelu(x W^T + b, alpha) in float64."""
    z = np.asarray(x, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T
    if b is not None:
        z = z + np.asarray(b, dtype=np.float64)
    return prelu_ref(z, alpha), z


def layer_bwd_ref(g, z, alpha, x, W):
    """(dx, dW, db, dalpha) in float64 from the upstream gradient g and the pre-activation z as given."""
    gz, da = prelu_bwd_ref(g, z, alpha)
    return gz @ np.asarray(W, dtype=np.float64), gz.T @ np.asarray(x, dtype=np.float64), gz.sum(0), da


def exactness(x, W, b, g):
    """The quantities, in int64, that must stay below EXACT_LIMIT for every fp32 sum of the layer to be exact in any order,
    in units of 1 / UNIT (|gz| <= 2 |g|, so 2 * UNIT |g| quarter units): y / z, dx, dW, db and sum |g z| for dalpha."""
    xi, Wi, bi, gi = (np.abs(np.asarray(a)).astype(np.int64) for a in (x, W, b, g))
    z = np.asarray(x).astype(np.int64) @ np.asarray(W).astype(np.int64).T + np.asarray(b).astype(np.int64)
    return {"z": UNIT * int((xi @ Wi.T + bi).max()),
            "dx": 2 * UNIT * int((gi @ Wi).max()),
            "dW": 2 * UNIT * int((gi.T @ xi).max()),
            "db": 2 * UNIT * int(gi.sum(0).max()),
            "dalpha": UNIT * int((gi * np.abs(z)).sum())}


def has_all_signs(z):
    return bool((z > 0).any() and (z < 0).any() and (z == 0).any())


def int_layer_case(rows, k, out, seed=0):
    """x, W, b, g: integer-valued fp32 arrays whose layer has cells with z > 0, z < 0 and z == 0 and meets `exactness`.  The
    amplitude (values in -amp .. amp) is the largest of 3, 2, 1 that does; the seed is advanced until all three signs occur."""
    for amp in (3, 2, 1):
        for s in range(seed, seed + 64):
            rng = np.random.RandomState(1000 * amp + s)
            x, W, b, g = (rng.randint(-amp, amp + 1, size=shape).astype(np.float32)
                          for shape in ((rows, k), (out, k), (out,), (rows, out)))
            z = x.astype(np.int64) @ W.astype(np.int64).T + b.astype(np.int64)
            if has_all_signs(z) and max(exactness(x, W, b, g).values()) < EXACT_LIMIT:
                return x, W, b, g
    raise AssertionError("no exact integer case for %r" % ((rows, k, out),))


def int_elementwise_case(rows, cols, seed=0):
    """u, g: integers -3 .. 3 as fp32 with u of all three signs where there are three cells; UNIT * sum |g u| < EXACT_LIMIT."""
    for s in range(seed, seed + 64):
        rng = np.random.RandomState(77 + s)
        u = rng.randint(-3, 4, size=(rows, cols)).astype(np.float32)
        g = rng.randint(-3, 4, size=(rows, cols)).astype(np.float32)
        if (has_all_signs(u) or u.size < 3) and UNIT * int(np.abs(g.astype(np.int64) * u.astype(np.int64)).sum()) < EXACT_LIMIT:
            return u, g
    raise AssertionError("no exact integer case for %r" % ((rows, cols),))


def ulp32(v):
    """One fp32 ulp at |v| (the smallest normal's for tiny values)."""
    return float(np.spacing(np.float32(max(abs(float(v)), 1.1754944e-38))))


def dalpha_bound(g, z, exact):
    """|dalpha - exact| <= ulp32(exact) + cells * 2^-53 * sum |g z|: every product is exact in double, every one of fewer than
    `cells` double additions rounds by at most 2^-53 of a partial sum that sum |g z| bounds, and the result is rounded once."""
    gz = np.abs(np.asarray(g, dtype=np.float64) * np.asarray(z, dtype=np.float64))
    return ulp32(exact) + gz.size * 2.0 ** -53 * float(np.where(np.asarray(z) <= 0, gz, 0.0).sum())
