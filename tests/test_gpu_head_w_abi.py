"""GPU tests of the output head with one weight per example, at the C ABI (xdfm_head_fwd_w / xdfm_head_bwd_w, csrc/reg.hip),
on the cases of head_w_ref.py: B in {1, 5, 513, 2049, 4100} (the vectorised kernels stride 2048 rows per sweep, the scalar
ones 512) x (Ku, Kv) in {(8, 32) vectorised, (7, 0) and (0, 516) scalar} x lin / bias present or absent.
  (a) the exact family (identity link, integer operands, w in {0, 1, 2, 3}): bit for bit the float64 result and the
      unweighted call on the batch with every row repeated w_b times;
  (b) all five (link, loss) pairs on random operands, w in [0, 4] with exact zeros, within the bounds head_w_ref.py derives;
      rows with w = 0 give exact zeros in dlin / du / dv;
  (c) w = NULL and w = ones are xdfm_head_fwd_ex / xdfm_head_bwd_ex bit for bit;
  (d) guard cells around every output and workspace stay untouched and a NaN-filled workspace does no harm (every call of
      this file runs that way, head_w_drivers.run_head_w);
  (e) three pairs twice in a row, bit for bit (head_w_drivers.run_cases)."""
import faulthandler

import numpy as np
import pytest
import torch

import head_ex_ref as X
import head_reg_ref as R
import head_w_drivers as DW
import head_w_ref as W

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 300          # a hang ends the process instead of blocking the run
EXACT_MODES = [(X.LINK_IDENTITY, X.LOSS_MSE), (X.LINK_IDENTITY, X.LOSS_MAE)]


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
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_values(a, b):
    """Equal as numbers (a zero's sign does not count: 0 * g and a sum of such zeros may be -0)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((a == b).all())


def _split(got, c):
    Ku, Kv = c["Ku"], c["Kv"]
    return {"du": got.get("du"), "dv": got.get("dv"), "dwu": got["grads"][:Ku], "dwv": got["grads"][Ku:Ku + Kv],
            "dbias": got["grads"][Ku + Kv]}


# ---------------------------------------------------------------------------------------------------------------------
# (a) exact family
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.W_CASES, ids=W.w_case_id)
def test_exact_family_equals_float64_and_the_row_repeated_batch_bit_for_bit(case):
    dev = _dev()
    for mode in EXACT_MODES:
        c, w = W.make_w_case(case, mode[0], exact=True)
        W.assert_exact_family(c, w, mode[1])
        got = DW.run_head_w(c, mode, dev, w)
        assert got["guards"], "a guard cell around an output or a workspace was written"
        ref = W.head_w64(c, w, mode)
        f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)
        assert _same_values(got["pred"], f32(ref["pred"])), "pred"
        assert np.array_equal(ref["pred"], f32(ref["pred"]))                  # the reference itself is an fp32 number everywhere
        assert float(got["loss"][0]) == ref["loss"], (W.mode_id(mode), float(got["loss"][0]), ref["loss"])
        assert _same_values(got["dlin"], f32(ref["g"])) and np.array_equal(ref["g"], f32(ref["g"])), "dlin"
        mine = _split(got, c)
        for k in ("du", "dv", "dwu", "dwv", "dbias"):
            if k in ref:
                assert _same_values(np.asarray(mine[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)), k
        # the unweighted entry points on the batch with row b repeated w_b times (rows of weight 0 dropped)
        rc, idx = W.repeat_rows(c, w)
        W.assert_exact_family(rc, np.ones(rc["B"], dtype=np.float32), mode[1])
        rep = DW.run_head_w(rc, mode, dev, None, entry="ex")
        assert rep["guards"]
        assert float(rep["loss"][0]) == float(got["loss"][0]), "loss vs repeated batch"
        assert _same_values(rep["grads"], got["grads"]), "grads vs repeated batch"
        # a repeated row carries the unweighted row gradient: w_b times it is the weighted one (exact here)
        assert _same_values(w[idx] * rep["dlin"], got["dlin"][idx]), "dlin vs repeated batch"
        for k in ("du", "dv"):
            if k in got:
                assert _same_values(w[idx][:, None] * rep[k], got[k][idx]), k + " vs repeated batch"
        zero = w == 0
        assert (got["dlin"][zero] == 0).all()
        assert np.abs(got["grads"]).max() > 0 or c["B"] <= 5


# ---------------------------------------------------------------------------------------------------------------------
# (b) all five pairs against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.W_CASES, ids=W.w_case_id)
@pytest.mark.parametrize("mode", W.ALL_MODES, ids=W.mode_id)
def test_weighted_head_against_float64(mode, case):
    dev = _dev()
    link, loss = mode
    c, w = W.make_w_case(case, link)
    assert w.min() >= 0 and w.max() <= 4 and (c["B"] < 5 or (w == 0).any())
    got = DW.run_head_w(c, mode, dev, w)
    frac = {}
    p64, pb = X.pred_ref(c, link)
    frac["pred"] = _frac(got["pred"], p64, pb)
    l64, lb = W.loss_w_ref(got["pred"], c["y"], w, loss)
    frac["loss"] = abs(float(got["loss"][0]) - l64) / max(lb, 1e-300)
    g64, gb = W.g_w_ref(got["pred"], c["y"], w, c["gloss"], mode)
    g32 = got["dlin"].reshape(-1)
    frac["dlin"] = _frac(g32, g64, gb)
    refs = R.head_grads_ref(g32, c["u"], c["wu"], c["v"], c["wv"])
    mine = _split(got, c)
    assert set(refs) == {k for k, v in mine.items() if v is not None and np.size(v)}
    for k, (ref, bound) in refs.items():
        frac[k] = _frac(mine[k], ref, bound)
    vec = W.w_vectorised(c["Ku"], c["Kv"])
    print("head_w %-14s %-22s %s " % (W.mode_id(mode), c["name"], "V" if vec else "S") + " ".join("%s %.3g" % kv for kv in sorted(frac.items())))
    assert got["guards"], "a guard cell around an output or a workspace was written"
    assert all(f <= 1.0 for f in frac.values()), frac
    zero = w == 0
    assert (g32[zero] == 0).all()
    for k in ("du", "dv"):
        if k in got:
            assert (got[k][zero] == 0).all(), k
    if (w > 0).any() and loss != X.LOSS_MAE:
        assert (g32[~zero] != 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# (c) w = NULL and w = ones
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(5, 8, 32, True), (2049, 8, 32, False), (513, 7, 0, True), (4100, 0, 516, True)], ids=W.w_case_id)
@pytest.mark.parametrize("mode", W.ALL_MODES, ids=W.mode_id)
def test_null_weights_and_unit_weights_are_the_ex_call_bit_for_bit(mode, case):
    dev = _dev()
    c, _ = W.make_w_case(case, mode[0])
    ex = DW.run_head_w(c, mode, dev, None, entry="ex")
    null = DW.run_head_w(c, mode, dev, None, entry="w")
    ones = DW.run_head_w(c, mode, dev, np.ones(c["B"], dtype=np.float32), entry="w")
    assert ex["guards"] and null["guards"] and ones["guards"]
    for k in DW.OUTPUTS:
        if k in ex:
            assert _same_bits(ex[k], null[k]), "w = NULL: " + k
            assert _same_bits(ex[k], ones[k]), "w = ones: " + k
    assert np.isfinite(ex["loss"]).all() and np.abs(ex["grads"]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# (e) twice in a row
# ---------------------------------------------------------------------------------------------------------------------
def test_head_w_twice_in_a_row_bit_for_bit():
    """head_w_drivers.run_cases: three pairs on a vectorised and a scalar case, every case twice in a row: the same bits
    both times, intact guards, a finite non-zero loss and gradient."""
    out = DW.run_cases(_dev())
    keys = sorted(out)
    assert len(keys) >= len(DW.REPEAT_MODES) * len(DW.REPEAT_CASES) * 2 * 6
    assert all(bool(out[k]) for k in keys if k.endswith("/guards"))
    for k in keys:
        if "/0/" in k:
            assert _same_bits(out[k], out[k.replace("/0/", "/1/")]), k
        if k.endswith(("/loss", "/grads")):
            assert np.isfinite(out[k]).all() and np.abs(out[k]).max() > 0, k
