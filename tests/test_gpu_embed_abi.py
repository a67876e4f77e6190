"""GPU tests (-m gpu) of K1 and K2 (csrc/embed.hip) at the C ABI: xdfm_embed_gather_fwd[_ld], xdfm_embed_scatter_bwd and
xdfm_embed_scatter_bwd_marked called through ctypes (tests/embed_ref.py `drive_gather` / `drive_scatter`) with guarded
buffers of the test's own.

Gather (embed_ref.GATHER_CASES; the facts each case claims are asserted on the CPU by tests/test_embed_reference.py):
  G1  m = 33: the id pass with a division per lane, a partial last block       G6  m*D = 8316: one example per block, DV = 63
  G2  m = 40, D = 12: float4 chunks with DV = 3, no dense part, no linear part  G7  D = 6: float2 chunks, DV = 3
  G3  m = 32 exactly (lane & 31)                                               G8  m = 1, D = 1
  G4  640 staged dense values per block: the tail loop past 512                G9  _ld: two empty field slots before the dense columns
  G5  nd = 300: the weight loop past 256; ldx = m + nd + 3; shuffled columns   G10 ids -3, -0.5, 0.9, V-0.25, V, V+7, 2.7 (G10b: the
                                                                                   four that stay inside [0, V): no flag)
emb_fm and dnn_in are copies (bits); lin_out is within (m + nd + 1) * 2^-24 * sum |terms| of the float64 sum (one rounding
per add, the products' roundings together one more); err_flag; guard bands; gap columns; every optional pointer as NULL.

Scatter (embed_ref.SCATTER_CASES): d_flat and the marks are held to the BITS of embed_ref.scatter_model -- the kernel's
documented arithmetic in integers -- and to the float64 sum within the bound of tests/test_gpu_parity.py; a second run and a
permutation of the examples (one chunk) give the same bits; what the batch does not touch keeps its bits; the unmarked
entry point gives the same buffer.
  S1-c*  every id exactly c times, c = 1 .. 25: every run alignment mod 8, runs ending on a window edge, owner + left piece,
         windows inside a run, such a window followed by a one-element piece
  S2     4096 examples on 1, 2 (4095 + 1) and 3 (8, 4080, 8) rows: chains of 510 and 512 windows
  S3-B*  chunks of 1, 5, 7, 8, 9 examples                  S4-B*  a second chunk of 1 and of 8 examples
  S5     a prefilled d_flat (old + sum, += in owners)     S6     table offsets 1, 2, 3 (mod 4): vector loads, scalar writes
  S7-*   d_emb_fm / d_flat one float off 16 bytes with D % 4 == 0: the <1> instance
  S8-D*  D = 6 (half-live last slice), D = 20 (five slices)
  S9     ld_dnn, ld_lin, ldx beyond dense, permuted columns        S10    G10's ids        S11-*  source subsets"""
import faulthandler

import numpy as np
import pytest
import torch

import embed_ref as ER

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
XDFM_OK, XDFM_ERR_INVALID = 0, 1


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from xdfm_amd import _lib
    return _lib.load()


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(ER.bits(got).reshape(-1) != ER.bits(want).reshape(-1))
    print("%s: %d of %d elements differ in their bits" % (what, bad.size, got.size))
    assert bad.size == 0, "%s: %d elements differ, first at %d: got %r, want %r" % (
        what, bad.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


# ------------------------------------------------------------------------------------------------------- K1: gather
def _check_gather(tag, inp, run, with_lin=True):
    B, m, D, nd = inp["B"], inp["m"], inp["D"], inp["nd"]
    emb, dnn, lin64, lin_abs, flag = ER.gather_expected(inp, with_lin)
    assert run["rc"] == XDFM_OK, _lib().xdfm_last_error()
    assert run["untouched"], "%s: a guard band was written" % tag
    _same_bits(run["emb"], emb, "%s emb_fm" % tag)
    if run["dnn_wide"] is not None:
        off, wide = run["layout"]["dense_off"], run["dnn_wide"]
        _same_bits(wide[:, :m * D], dnn[:, :m * D], "%s dnn_in, embedding columns" % tag)
        _same_bits(wide[:, off:off + nd], dnn[:, m * D:], "%s dnn_in, dense columns" % tag)
        gap = np.concatenate([wide[:, m * D:off], wide[:, off + nd:]], axis=1)
        _same_bits(gap, np.full_like(gap, ER.SENTINEL), "%s dnn_in, columns that are not the call's" % tag)
    if run["lin"] is not None:
        err = np.abs(run["lin"].astype(np.float64) - lin64)
        tol = (m + nd + 1) * 2.0 ** -24 * lin_abs
        print("%s lin_out: worst error %.3e, its bound %.3e" % (tag, float(err.max()), float(tol[err.argmax()])))
        assert (err <= tol).all(), "%s lin_out: %d rows off, worst %g" % (tag, int((err > tol).sum()), float(err.max()))
    if run["flag"] is not None:
        assert run["flag"] == flag, "%s err_flag %d" % (tag, run["flag"])


@pytest.mark.parametrize("name", list(ER.GATHER_CASES))
def test_gather_case_against_the_reference(name):
    dev, lib = _dev(), _lib()
    inp = ER.gather_inputs(name)
    full = ER.drive_gather(lib, dev, inp)
    _check_gather(name, inp, full)
    assert full["dnn_wide"] is not None and full["lin"] is not None and full["flag"] is not None
    for null in ("dnn_in", "lin_out", "err_flag") + (("lin_tables",) if inp["lins"] is not None else ()):
        part = ER.drive_gather(lib, dev, inp, null=(null,))
        tag = "%s with %s = NULL" % (name, null)
        _check_gather(tag, inp, part, with_lin=null != "lin_tables")
        assert (part["dnn_wide"] is None) == (null == "dnn_in") and (part["lin"] is None) == (null == "lin_out") and \
            (part["flag"] is None) == (null == "err_flag")
        _same_bits(part["emb"], full["emb"], tag + ": emb_fm against the full call")
        if part["dnn_wide"] is not None:
            _same_bits(part["dnn_wide"], full["dnn_wide"], tag + ": dnn_in against the full call")
        if part["lin"] is not None and null != "lin_tables":
            _same_bits(part["lin"], full["lin"], tag + ": lin_out against the full call")


def test_gather_clamped_ids_read_the_clamped_rows():
    """G10 with tables whose rows name themselves: the rows in emb_fm are rows 0 / V - 1 for the far-out ids and the
    truncated id for the fractional ones."""
    dev, lib = _dev(), _lib()
    inp = ER.gather_inputs("G10")
    inp["tables"] = [np.repeat(np.arange(V, dtype=np.float32)[:, None], inp["D"], 1) + 100 * j for j, V in enumerate(inp["vocab"])]
    run = ER.drive_gather(lib, dev, inp)
    _check_gather("G10, self-naming rows", inp, run)
    for j, V in enumerate(inp["vocab"]):
        x = inp["X"][:, inp["cols"][j]]
        want = np.clip(np.trunc(x.astype(np.float64)), 0, V - 1) + 100 * j
        assert (run["emb"][:, j, :] == want[:, None]).all()
    assert run["flag"] == 1


def test_gather_argument_checks_launch_nothing():
    dev, lib = _dev(), _lib()
    inp = ER.gather_inputs("G7")
    calls = [("m*D = 41000", dict(override=dict(m=41, D=1000, ldx=64)), b"LDS"),
             ("B = 0", dict(override=dict(B=0)), b"bad shape"),
             ("ldx < m + nd", dict(override=dict(ldx=inp["m"] + inp["nd"] - 1)), b"bad shape"),
             ("nd > 0 without dense_cols", dict(null=("dense_cols",)), b"dense_cols"),
             ("lin_out with nd > 0 without dense_w", dict(null=("dense_w",)), b"dense_w")]
    for what, kw, word in calls:
        run = ER.drive_gather(lib, dev, inp, **kw)
        assert run["rc"] == XDFM_ERR_INVALID and word in lib.xdfm_last_error(), "%s: rc %d, %r" % (what, run["rc"], lib.xdfm_last_error())
        assert run["untouched"] and run["flag"] == 0
        for key in ("emb", "dnn_wide", "lin"):
            _same_bits(run[key], np.full_like(run[key], ER.SENTINEL), "%s: %s after a refused call" % (what, key))


# ------------------------------------------------------------------------------------------------------ K2: scatter
def _check_scatter(tag, case, run, want_flat, want_marks):
    assert run["rc"] == XDFM_OK, _lib().xdfm_last_error()
    assert run["untouched"], "%s: a guard band was written" % tag
    exact, tol = ER.scatter_bound(case)
    err = np.abs(run["flat"].astype(np.float64) - exact)
    t = ER.touched(case)
    print("%s: %d elements, %d touched; worst error / bound against float64 %.3f" % (
        tag, t.size, int(t.sum()), float((err[t] / tol[t]).max()) if t.any() else 0.0))
    _same_bits(run["flat"][~t], case["prefill"][~t], "%s d_flat, elements the batch does not touch" % tag)
    _same_bits(run["flat"], want_flat, "%s d_flat against the integer model" % tag)
    assert not (err > tol).any(), "%s: %d elements outside the float64 bound, worst %g" % (tag, int((err > tol).sum()), float(err.max()))
    if run["marks"] is not None:
        np.testing.assert_array_equal(run["marks"], want_marks, err_msg="%s marks" % tag)


@pytest.mark.parametrize("name", list(ER.SCATTER_CASES))
def test_scatter_case_to_the_bits_of_the_model(name):
    dev, lib = _dev(), _lib()
    case = ER.scatter_inputs(name)
    want_flat, want_marks = ER.scatter_model(case)
    run = ER.drive_scatter(lib, dev, case)
    assert (run["marks"] is not None) == case["marks"]
    _check_scatter(name, case, run, want_flat, want_marks)
    again = ER.drive_scatter(lib, dev, case)
    _same_bits(again["flat"], run["flat"], "%s: a second run" % name)
    if case["B"] <= ER.SC_ROWS:
        p = np.random.default_rng(17).permutation(case["B"])
        shuffled = ER.drive_scatter(lib, dev, ER.permuted(case, p))
        _same_bits(shuffled["flat"], run["flat"], "%s: examples permuted" % name)
        if case["marks"]:
            np.testing.assert_array_equal(shuffled["marks"], run["marks"])
    if case["dense_pitches"]:
        plain = ER.drive_scatter(lib, dev, case, marked=False)
        assert plain["rc"] == XDFM_OK and plain["untouched"] and plain["marks"] is None
        _same_bits(plain["flat"], run["flat"], "%s: xdfm_embed_scatter_bwd" % name)


def test_scatter_argument_checks_launch_nothing():
    dev, lib = _dev(), _lib()
    case, off = ER.scatter_inputs("S5"), ER.scatter_inputs("S7-flat")
    calls = [("marks with a d_flat off 16 bytes", off, dict(force_marks=True), b"marks need"),
             ("offsets without d_flat", off, dict(null=("d_flat",)), b"offsets without"),
             ("ld_dnn < m*D", case, dict(ld_dnn=case["m"] * case["D"] - 1), b"ld_dnn"),
             ("tab_off without a row gradient", case, dict(null=("d_emb", "d_dnn")), b"without row gradients")]
    for what, c, kw, word in calls:
        run = ER.drive_scatter(lib, dev, c, **kw)
        assert run["rc"] == XDFM_ERR_INVALID and word in lib.xdfm_last_error(), "%s: rc %d, %r" % (what, run["rc"], lib.xdfm_last_error())
        assert run["untouched"]
        _same_bits(run["flat"], c["prefill"], "%s: d_flat after a refused call" % what)
        assert run["marks"] is None or not run["marks"].any()
