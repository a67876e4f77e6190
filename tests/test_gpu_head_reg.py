"""GPU tests (-m gpu) of the kernels of csrc/reg.hip -- the fused output head, the bias-gradient column sums and the
multi-tensor L2 regulariser -- against the float64 references of tests/head_reg_ref.py, and of the families that leave
partials to a finish twice in a row, bit for bit.  The bars are derived in head_reg_ref.py's docstring; none
was fitted to what the kernels give.  Every test prints the fraction of each bar it used before it asserts.

Head cases (head_reg_ref.HEAD_CASES; fwd / bwd kernel: V = float4 kernels head_fwd_kernel<true> + head_bwd_vec_kernel,
S = scalar kernels head_fwd_kernel<false> + head_bwd_kernel; the host picks V when K % 4 == 0, K <= 512 and all operands
are 16-byte aligned):

  case               B      Ku    Kv   lin bias labels  kernel  hits
  c0000 .. c1111     17     0|64  0|60  all 16   hard/soft  V   every present / absent combination of u, v, lin, bias
                                                                (c0000: z = 0; bias-only, lin-only, ...), B = 17
  k1_b15             15     1     -    y   y    hard    S       K = 1, B = 15
  k3_k4_b16          16     3     4    y   y    soft    S       odd K = 3 next to K = 4: scalar by K % 4, B = 16
  k3_k1_b1           1      3     1    y   y    hard    S       B = 1
  k64_k60_b1         1      64    60   y   y    soft    V       B = 1, K = 60, 64
  k4_k68_b2047       2047   4     68   y   y    hard    V       K = 4, 68; one row short of a grid stride
  k512_k200_b2048    2048   512   200  y   y    sat     V       K = 512 (last float4 width), 200; one stride; saturating
  k516_k64_b2049     2049   516   64   y   y    sat     S       K = 516: scalar by size; one row past a stride; saturating
  k200_k512_b4099    4099   200   512  y   -    soft    V       ragged third stride
  k1000_b17          17     1000  -    -   y    hard    S       K = 1000: scalar by size
  k4000_k95_b16      16     4000  95   y   y    soft    S       Ku + Kv = 4095, the largest the LDS check admits
  k64_k4_b65536      65536  64    4    y   y    hard    V       B = 65536
  k5_k8_b65536       65536  5     8    y   y    soft    S       B = 65536, odd K
  k64_k64_u_off      2048   64    64   y   y    hard    S       u one float off a 16-byte boundary: scalar by alignment
  k64_k64_wv_off     17     64    64   -   -    soft    S       wv one float off: scalar by alignment

gloss cycles through 0.37, 1.0, -2.5, 1.75 by position in the list.  Every case is run twice and must give the same bits.

Column sums: head_reg_ref.COLSUM_SHAPES through the C ABI, on a column window of a wider matrix (plain: ld = cols + 5,
window from column 2; ReLU: ldg = cols + 3 from column 2, ldy = cols + 8 from column 3); 65600 columns are 1025 column
blocks.  The ReLU variant leaves out 262144 x 1000 (three 1 GB operands).
L2: head_reg_ref.L2_CASES through ops.L2Reg, accumulate = 1 through the C ABI.  t1 and t2_big hold a 2^22 + 3 element
tensor whose address and gradient slot are 16-byte aligned: 128 strides of l2_sumsq_kernel's float4 loop, 32 of
l2_grad_kernel's, and a 3-element scalar tail; t2_big's second tensor (2^21 + 1 elements) and its gradient slot are
misaligned: the scalar loops over 256 / 64 strides.  The value is held to gamma(numel) as a whole and to the bound of
the kernels' own walk (head_reg_ref.l2_value_ref), the gradient to its bits.
"""
import faulthandler

import numpy as np
import pytest
import torch

import head_reg_drivers as D
import head_reg_ref as R

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 300          # a hang ends the process instead of blocking the run


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _frac(got, ref, bound):
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    if got.size == 0:
        return 0.0
    return float((np.abs(got.reshape(ref.shape) - ref) / np.maximum(bound, 1e-300)).max())


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.head_case_names())
def test_head_against_float64(name):
    dev = _dev()
    c = R.make_head_case(name)
    B = c["B"]
    got = D.run_head(c, dev)
    again = D.run_head(c, dev)
    assert sorted(got) == sorted(again)
    present = {k for k in ("lin", "u", "wu", "v", "wv", "bias") if c[k] is not None}
    assert set(got) == {"pred", "loss"} | {"d" + k for k in present}

    frac = {}
    p64, pb = R.head_pred_ref(c["lin"], c["u"], c["wu"], c["v"], c["wv"], c["bias"], B)
    frac["pred"] = _frac(got["pred"], p64, pb)
    l64, lb, terms = R.head_loss_ref(got["pred"], c["y"])
    frac["loss"] = abs(float(got["loss"][0]) - l64) / lb
    g64 = R.head_g_ref(got["pred"], c["y"], c["gloss"])
    if "dlin" in got:
        g32 = got["dlin"].reshape(-1)
        aux_dbias = None
    else:
        g32, aux_dbias = D.head_g_aux(got["pred"], c["y"], c["gloss"], dev)
    frac["g"] = _frac(g32, g64, R.ulp_bound(g64))                       # dlin (or the kernel's g of the same pred) at 2 ulp
    refs = R.head_grads_ref(g32, c["u"], c["wu"], c["v"], c["wv"])
    for k, (ref, bound) in refs.items():
        if k in got:
            frac[k] = _frac(got[k], ref, bound)
    if aux_dbias is not None and "dbias" not in got:
        frac["dbias_aux"] = _frac(np.array(aux_dbias), *refs["dbias"])    # the bias column of the gradient row, no bias given
    vec = R.head_vectorised(c["Ku"], c["Kv"], c["misalign"])
    print("head %-16s %s " % (name, "V" if vec else "S") + " ".join("%s %.3g" % kv for kv in sorted(frac.items())))
    for k in got:
        assert _same_bits(got[k], again[k]), "%s differs between two runs" % k
    assert all(f <= 1.0 for f in frac.values()), frac
    if c["labels"] == "sat":
        p, y = got["pred"], c["y"]
        for side in (0.0, 1.0):
            for lab in (0.0, 1.0):
                assert ((p == side) & (y == lab)).any(), (side, lab)
        assert (terms == 100.0).any()
        sat = (p == 0) | (p == 1)
        assert (g32[sat] == 0).all() and (got["du"][sat] == 0).all() and (got["dv"][sat] == 0).all()
    if not present:
        assert (got["pred"] == 0.5).all()


# ---------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------
def _check_colsum(rows, cols, relu, dev):
    g, y = R.make_colsum_case(rows, cols, relu)
    gw = g[:, D.COL0_G:D.COL0_G + cols]
    yw = y[:, D.COL0_Y:D.COL0_Y + cols] if relu else None
    ref, bound, gz = R.colsum_ref(gw, yw)
    a, b = D.run_colsum(g, y, cols, dev)
    f = _frac(a["out"], ref, bound)
    print("colsum%s %7d x %5d: %.3g of the bound" % ("_relu" if relu else "", rows, cols, f))
    assert a["guards"] and b["guards"], "a guard cell around out, gz or the workspace was written"
    assert _same_bits(a["out"], b["out"])
    if relu:
        assert _same_bits(a["gz"], gz), "gz is not where(y > 0, g, 0) bit for bit"
        assert _same_bits(b["gz"], gz)
        if rows * cols >= 1000:
            zero = yw == 0
            assert (zero & np.signbit(yw)).any() and (zero & ~np.signbit(yw)).any() and (yw < 0).any()
    assert f <= 1.0, f


@pytest.mark.parametrize("rows,cols", R.COLSUM_SHAPES)
def test_colsum_against_float64(rows, cols):
    _check_colsum(rows, cols, False, _dev())


@pytest.mark.parametrize("rows,cols", [s for s in R.COLSUM_SHAPES if s != (262144, 1000)])
def test_relu_bwd_colsum_against_float64(rows, cols):
    _check_colsum(rows, cols, True, _dev())


def test_colsum_shapes_cover_the_sweep():
    assert {s[0] for s in R.COLSUM_SHAPES} == {1, 15, 16, 63, 64, 65, 1000, 4099, 262144}
    assert {s[1] for s in R.COLSUM_SHAPES} == {1, 63, 64, 65, 429, 1000, 65600}
    for cols in {s[1] for s in R.COLSUM_SHAPES}:
        ld, ldg, ldy = R.colsum_pitches(cols)
        assert ld >= D.COL0_G + cols and ldg >= D.COL0_G + cols and ldy >= D.COL0_Y + cols and ldg != ldy


# ---------------------------------------------------------------------------------------------------------------------
# L2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.L2_CASES])
def test_l2_against_float64(name):
    dev = _dev()
    c = R.l2_case(name)
    val, grads = D.run_l2(c, dev)
    val2, grads2 = D.run_l2(c, dev)
    v64, bound, walk = R.l2_value_ref(c["ws"], c["coeffs"])
    f, fw = abs(float(val) - v64) / bound, abs(float(val) - v64) / walk
    print("l2 %-6s value %.9g (float64 %.9g): %.3g of the bound, %.3g of the walk bound" % (name, val, v64, f, fw))
    assert np.float32(val).tobytes() == np.float32(val2).tobytes()
    bad = []
    for t, (w, k, g, g2) in enumerate(zip(c["ws"], c["coeffs"], grads, grads2)):
        want, _ = R.l2_grad_ref(w, k, c["gs"])
        if not (_same_bits(g.reshape(-1), want) and _same_bits(g2.reshape(-1), want)):
            bad.append(t)
    assert not bad, "gradient of tensors %s is not fl(fl(fl(2 c) gs) w)" % bad[:10]
    assert f <= 1.0, f
    assert fw <= 1.0, fw


@pytest.mark.parametrize("name", ["t1", "t2", "t2_big", "t257"])
def test_l2_accumulate_against_float64(name):
    dev = _dev()
    c = R.l2_case(name)
    n = sum(c["sizes"])
    g0 = np.random.default_rng(n).standard_normal(n, dtype=np.float32) * np.float32(1e-3)
    got, guards = D.run_l2_accumulate(c, g0, dev)
    got2, _ = D.run_l2_accumulate(c, g0, dev)
    assert guards, "a guard cell around the flat gradient was written"
    assert _same_bits(got, got2)
    off, worst = 0, 0.0
    for w, k in zip(c["ws"], c["coeffs"]):
        ref, bound = R.l2_grad_acc_ref(w, k, c["gs"], g0[off:off + w.size])
        worst = max(worst, _frac(got[off:off + w.size], ref, bound))
        off += w.size
    print("l2 accumulate %-5s: %.3g of 1 ulp" % (name, worst))
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# the families with a finish, twice in a row
# ---------------------------------------------------------------------------------------------------------------------
def test_finish_cases_repeat_bit_for_bit():
    """tests/head_reg_cases.py runs a fixed list of cases -- the 70-tensor Adam step with its L2 value, head forward and
    backward on both kernels, both column sums (the 65600-column shape among them) -- every family twice in a row, then a
    small xDeepFM train step with both L2 terms, eager and graph-replayed.  The second run in a row must give the first
    one's bits (partials or a cell left behind by the first would not), no guard cell may be written, and the train steps
    must have been replayed from the graph with finite results."""
    dev = _dev()
    import head_reg_cases
    out = head_reg_cases.run_cases(dev)
    assert int(out["meta/replays"]) >= 3
    keys = sorted(k for k in out if not k.startswith("meta/"))
    assert len(keys) > 40
    adam = [k for k in keys if k.startswith("adam70/")]
    assert len(adam) == 10 and all(np.isfinite(out[k]).all() for k in adam)       # 2 runs x (2 L2 values + p, m, v)
    assert all(float(np.abs(out[k]).max()) > 0 for k in adam)
    first = [k for k in keys if "/0/" in k]
    for fam, n in (("adam70/", 5), ("head/", len(head_reg_cases.HEAD)), ("colsum/", len(head_reg_cases.COLSUM)),
                   ("colsum_relu/", len(head_reg_cases.COLSUM))):
        assert sum(k.startswith(fam) for k in first) >= n, fam
    diff = []
    for k in first:
        a, b = out[k], out[k.replace("/0/", "/1/")]
        if not (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()):
            diff.append(k)
    assert not diff, "the second run in a row differs from the first in %s" % diff[:12]
    guards = [k for k in keys if k.endswith("/guards")]
    assert len(guards) == 4 * len(head_reg_cases.COLSUM) and all(int(out[k]) == 1 for k in guards)
    steps = [k for k in keys if k.startswith("train/step")]
    assert len(steps) == 3 * head_reg_cases.TRAIN_STEPS and head_reg_cases.TRAIN_STEPS == 6
    assert all(np.isfinite(out[k]).all() for k in keys if k.startswith("train/"))
