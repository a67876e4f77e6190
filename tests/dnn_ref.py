"""What the dense-layer tests (csrc/dnn.hip) share: a float64 reference, a mirror of the weight gradient's split plan,
the case table of tests/test_gpu_dnn_abi.py and input generators whose sums are exact in fp32.  No GPU needed; checked by
tests/test_dnn_reference.py."""
import numpy as np
import torch

DN_K, DN_SPLIT_ROWS, DN_MAX_SPLIT = 32, 256, 32         # csrc/dnn.hip

#  name: (rows, in, out)
ABI_CASES = {
    "E1": (1, 1, 32),            # pitch 1, one row, one stage
    "E2": (64, 64, 64),          # exact tiles, no ragged stage anywhere
    "E3": (65, 65, 96),          # one past in every dimension; half tiles in N (forward) and M (dW); K = 96 in dX
    "E4": (63, 31, 160),         # one short; 2.5 tiles; K = 160 in dX
    "E5a": (256, 33, 32),        # the 1-split side of the boundary
    "E5b": (257, 33, 32),        # the 2-split side of the boundary
    "E6": (1100, 13, 32),        # 5 splits: one unrolled round of the finish plus a one-term tail
    "E7": (2049, 40, 64),        # 9 splits, the last split one row
    "E8": (4096, 13, 96),        # the production batch's 16 splits: four unrolled rounds, no tail
    "E9": (8225, 65, 96),        # the cap: kper 288, 29 splits in a workspace sized for 32
    "E10": (9000, 13, 32),       # 32 splits of 288
}
#  what each case's name claims about its rows: (want, kper, nsplit, last_rows)
ABI_PLANS = {
    "E1": (1, 32, 1, 1), "E2": (1, 64, 1, 64), "E3": (1, 96, 1, 65), "E4": (1, 64, 1, 63),
    "E5a": (1, 256, 1, 256), "E5b": (2, 160, 2, 97), "E6": (5, 224, 5, 204), "E7": (9, 256, 9, 1),
    "E8": (16, 256, 16, 256), "E9": (32, 288, 29, 161), "E10": (32, 288, 32, 72),
}
#  values of y for the backward's mask: +0, -0, a negative and NaN-free positives down to the smallest normal
MASK_CLOSED = (0.0, -0.0, -1.0)
MASK_OPEN = (1.1754944e-38, 1.0)


def split_plan(rows):
    """(want, kper, nsplit, last_rows) of the weight gradient's split over the rows: a mirror of dn_splits and the three
    lines at the top of xdfm_dense_bwd_w.  `want` sizes the workspace, `nsplit` splits of `kper` rows run, the last one
    holds `last_rows`.  The mirror exists so that a test case cannot silently stop exercising what its name says (a
    one-row last split, 29 splits in a workspace for 32, ...) when the plan's constants change: the CPU test asserts the
    claims of every case, and `want` against xdfm_dense_bwd_w_ws_elems."""
    want = min(DN_MAX_SPLIT, max(1, -(-rows // DN_SPLIT_ROWS)))
    kper = -(-(-(-rows // want)) // DN_K) * DN_K
    nsplit = -(-rows // kper)
    return want, kper, nsplit, rows - (nsplit - 1) * kper


def dense_ref(x, W, b, relu):
    """y = act(x W^T + b) in float64 from fp32 (or any) inputs.  The trailing + 0.0 makes every zero a +0.0, as a sum that
    starts from +0.0 gives in round-to-nearest whatever the signs of its zero terms."""
    z = x.double() @ W.double().t()
    if b is not None:
        z = z + b.double()
    return (torch.relu(z) if relu else z) + 0.0


def dense_bwd_ref(g, y_mask, x, W):
    """(dx, dW, db) in float64 with gz = where(y_mask > 0, g, 0); y_mask None: gz = g.  -0.0, negatives and NaN close the
    mask.  Zeros are +0.0 (see dense_ref)."""
    g6 = g.double()
    gz = g6 if y_mask is None else torch.where(y_mask > 0, g6, torch.zeros_like(g6))
    return gz @ W.double() + 0.0, gz.t() @ x.double() + 0.0, gz.sum(0) + 0.0


def int_inputs(rows, k, out, seed):
    """x, W, b, g drawn from the integers -3 .. 3 as fp32.  Every product is at most 9 in magnitude and every sum of at
    most 9000 of them (plus a bias) stays below 2^24, so any order of fp32 additions is exact: an fp32 result must equal
    the float64 reference bit for bit."""
    gen = torch.Generator().manual_seed(seed)

    def draw(*shape):
        return torch.randint(-3, 4, shape, generator=gen).float()

    return draw(rows, k), draw(out, k), draw(out), draw(rows, out)


def exact_sum_bound(rows, k, out):
    """Largest magnitude any partial sum of the int_inputs products can reach in y, dx, dW or db."""
    return max(9 * k + 3, 9 * out, 9 * rows, 3 * rows)


def mask_pattern(rows, out, seed):
    """A y for the backward calls that is the test's own: every cell open or closed by a fair coin, its value drawn from
    MASK_OPEN / MASK_CLOSED."""
    gen = torch.Generator().manual_seed(seed)
    is_open = torch.randint(0, 2, (rows, out), generator=gen).bool()
    opened = torch.tensor(MASK_OPEN)[torch.randint(0, len(MASK_OPEN), (rows, out), generator=gen)]
    closed = torch.tensor(MASK_CLOSED)[torch.randint(0, len(MASK_CLOSED), (rows, out), generator=gen)]
    return torch.where(is_open, opened, closed)


def normal_inputs(rows, k, out, seed):
    """The scaling of tests/test_gpu_dnn.py: standard normal x and g, W ~ N(0, 1 / in), b ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k, generator=gen)
    W = torch.randn(out, k, generator=gen) / float(np.sqrt(k))
    return x, W, torch.randn(out, generator=gen), torch.randn(rows, out, generator=gen)


def bits(t):
    """int32 view of an fp32 tensor: equality of bits, so that NaN compares and -0.0 differs from +0.0."""
    return t.contiguous().view(torch.int32)


def first_difference(got, want, tile=64):
    """None when got and want (2-D or 1-D fp32) hold the same bits; otherwise a sentence naming the first differing
    (row, column), the 64 x 64 tile it lies in and its place inside that tile."""
    ne = bits(got) != bits(want)
    if not bool(ne.any()):
        return None
    idx = ne.nonzero()[0].tolist()
    r, c = (idx + [0])[:2] if got.dim() == 2 else (0, idx[0])
    return "%d of %d cells differ; first at (row %d, column %d): got %r, want %r; tile (%d, %d), cell (%d, %d) of it" % (
        int(ne.sum()), ne.numel(), r, c, float(got[tuple(idx)]), float(want[tuple(idx)]), r // tile, c // tile, r % tile,
        c % tile)
