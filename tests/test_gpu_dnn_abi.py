"""GPU tests (-m gpu) of the three dense-layer entry points of csrc/dnn.hip called directly (xdfm_dense_fwd,
xdfm_dense_bwd_x, xdfm_dense_bwd_w), so that pitches, output buffers and the workspace are the test's own.

Cases: tests/dnn_ref.py ABI_CASES (E1 .. E10): tile edges (exact multiples, one past, one short, out a multiple of 32 but
not of 64, in = 1), the 256 / 257 row step from one split to two, 5, 9, 16, 29-of-32 and 32 splits of the weight gradient.

a. Integer inputs (-3 .. 3): every sum is exact in fp32 whatever its order, so y, dx, dW and db must equal the float64
   reference bit for bit.  The backward's mask is a pattern of the test's own (+0, -0, -1, the smallest normal, 1).
b. Pitched operands cut out of NaN-filled wider matrices, outputs written into sentinel-filled wider matrices and
   between sentinel guards, a NaN-poisoned workspace of exactly the queried size: same bits as the contiguous call, every
   pad and guard cell untouched.  Runs on EVERY case.
c. +-Inf and NaN in g behind a closed mask stay out of dx, dW and db (the mask is a select, not a product).
d. Standard-normal inputs, pitched: error against float64 at most max(2 x the library path's, 1 ulp) -- the bar of
   tests/test_gpu_dnn.py, the library path being torch's fp32 mm / addmm and gz.sum(0) on the device.
e. Two calls give the same bits, the second on the first one's uncleared workspace.

What runs where (the cases' split plans are asserted on the CPU, tests/test_dnn_reference.py):
  finish kernel with 4 or more splits, ragged and full groups .. test_backward_equals_float64_bit_for_bit[E6, E7, E8, E10]
  the split cap, 29 splits in a workspace for 32 ................ ...[E9];  a one-row last split: [E7];  256 | 257 rows: [E5a], [E5b]
  out = 96 / 160, rows and in at, one past and one short of 64 .. test_forward_... and test_backward_...[E2, E3, E4];  in = 1: [E1]
  ldy > out, lddx > in, pads, guards, poisoned workspace ........ test_pitched_operands_same_bits_and_nothing_written_outside
  y = NULL instances with pitched inputs; db = NULL, nsplit > 1 . the same test (masked False; with_db False on every case)
  the mask as a select; y = -0.0 and y < 0 ...................... test_non_finite_g_behind_a_closed_mask_stays_out; the pattern
  needs_input_grad combinations, the chained tower .............. tests/test_gpu_dnn.py"""
import faulthandler

import numpy as np
import pytest
import torch

import dnn_ref as R

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
FACTOR = 2.0
GUARD = 256                      # sentinel floats before and after dW, db and the workspace
SENTINEL = -24681.357            # never a result of the integer or the normal inputs
#  (left pad, right pad) of each operand's window: all different, odd ones leave rows 4-byte aligned only
PADS = {"x": (3, 2), "g": (1, 4), "y_mask": (2, 5), "y": (5, 1), "dx": (1, 3)}
_CACHE = {}


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    from xdfm_amd import _lib, ops
    return _lib, _lib.load(), ops


class _Win:
    """A [rows][cols] column window of a wider matrix filled with `fill`: .t is the window (pitch .ld), .wide the matrix."""

    def __init__(self, rows, cols, pads, fill, dev, src=None):
        self.l, self.cols = pads[0], cols
        self.wide = torch.full((rows, pads[0] + cols + pads[1]), fill, dtype=torch.float32, device=dev)
        self.t = self.wide[:, self.l:self.l + cols]
        self.ld = self.wide.shape[1]
        assert self.ld > cols
        if src is not None:
            self.t.copy_(src)
        self.before = self.wide.clone()

    def pads_untouched(self):
        ne = R.bits(self.wide) != R.bits(self.before)
        ne[:, self.l:self.l + self.cols] = False
        return not bool(ne.any())


class _Guarded:
    """n floats between two runs of GUARD sentinels; the payload starts as `fill`."""

    def __init__(self, n, fill, dev):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)

    def guards_untouched(self):
        want = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device=self.buf.device)
        return bool((R.bits(self.buf[:GUARD]) == R.bits(want)).all()) and bool((R.bits(self.buf[GUARD + self.n:]) == R.bits(want)).all())


def _ld(t):
    return max(int(t.stride(0)), int(t.shape[1]))


def _fwd(x, W, b, relu, y=None):
    """xdfm_dense_fwd; x and y may be windows (their pitch is their stride)."""
    mod, lib, ops = _api()
    rows, k = x.shape
    out = W.shape[0]
    if y is None:
        y = torch.empty(rows, out, dtype=torch.float32, device=x.device)
    mod.check(lib.xdfm_dense_fwd(ops._ptr(x), rows, k, _ld(x), ops._ptr(W), out, ops._ptr(b), 1 if relu else 0, ops._ptr(y),
                                 _ld(y), ops._stream()), "dense_fwd")
    return y


def _bwd_x(g, y, W, dx=None):
    mod, lib, ops = _api()
    rows, out = g.shape
    k = W.shape[1]
    if dx is None:
        dx = torch.empty(rows, k, dtype=torch.float32, device=g.device)
    mod.check(lib.xdfm_dense_bwd_x(ops._ptr(g), _ld(g), ops._ptr(y), _ld(y) if y is not None else 0, rows, out, ops._ptr(W), k,
                                   ops._ptr(dx), _ld(dx), ops._stream()), "dense_bwd_x")
    return dx


def _bwd_w(g, y, x, with_db=True, ws=None, dW=None, db=None):
    """xdfm_dense_bwd_w -> (dW [out][in], db or None, ws).  ws, dW, db: flat tensors of the test's own, or fresh ones."""
    mod, lib, ops = _api()
    rows, out = g.shape
    k = x.shape[1]
    n_ws = lib.xdfm_dense_bwd_w_ws_elems(rows, k, out)
    if ws is None:
        ws = torch.empty(n_ws, dtype=torch.float32, device=g.device)
    assert ws.numel() == n_ws
    if dW is None:
        dW = torch.empty(out * k, dtype=torch.float32, device=g.device)
    if db is None and with_db:
        db = torch.empty(out, dtype=torch.float32, device=g.device)
    assert dW.numel() == out * k and (db is None or db.numel() == out)
    mod.check(lib.xdfm_dense_bwd_w(ops._ptr(g), _ld(g), ops._ptr(y), _ld(y) if y is not None else 0, ops._ptr(x), _ld(x), rows, k,
                                   out, ops._ptr(ws), ops._ptr(dW), ops._ptr(db) if with_db else None, ops._stream()), "dense_bwd_w")
    return dW.view(out, k), (db if with_db else None), ws


def _same(got, want, what):
    msg = R.first_difference(got.detach().cpu(), want.detach().cpu())
    assert msg is None, "%s: %s" % (what, msg)


def _which_split(name, ws, g, y_mask, x):
    """For a dW that differs: the first split whose slab in the workspace is not the float64 product of its own rows."""
    rows, k, out = R.ABI_CASES[name]
    _, kper, nsplit, _ = R.split_plan(rows)
    if nsplit == 1:
        return "one split (no slab): stage %d rows each" % R.DN_K
    slabs = ws.cpu()[:nsplit * out * k].view(nsplit, out, k)
    for z in range(nsplit):
        sl = slice(z * kper, min(rows, (z + 1) * kper))
        want = R.dense_bwd_ref(g[sl], None if y_mask is None else y_mask[sl], x[sl], torch.zeros(out, k))[1].float()
        msg = R.first_difference(slabs[z], want)
        if msg is not None:
            return "split %d of %d (rows %d .. %d) is wrong: %s" % (z, nsplit, sl.start, sl.stop - 1, msg)
    return "every slab is right: the finish kernel's sum over %d splits is wrong" % nsplit


def _exact(name):
    """Integer inputs of a case on the host and the device, the mask pattern and the float64 references, once."""
    if name in _CACHE:
        return _CACHE[name]
    dev = _dev()
    rows, k, out = R.ABI_CASES[name]
    x, W, b, g = R.int_inputs(rows, k, out, seed=100 + rows + k + out)
    y_mask = R.mask_pattern(rows, out, seed=rows + out)
    c = dict(x=x, W=W, b=b, g=g, y_mask=y_mask, dev={n: t.to(dev) for n, t in dict(x=x, W=W, b=b, g=g, y_mask=y_mask).items()})
    c["ref_y"] = {(relu, bias): R.dense_ref(x, W, b if bias else None, relu).float() for relu in (True, False) for bias in (True, False)}
    c["ref_bwd"] = {masked: [t.float() for t in R.dense_bwd_ref(g, y_mask if masked else None, x, W)] for masked in (True, False)}
    _CACHE[name] = c
    return c


def _contiguous(name):
    """The contiguous calls of a case (fresh torch.empty outputs): what the pitched calls must reproduce bit for bit."""
    c = _exact(name)
    if "plain" in c:
        return c["plain"]
    d = c["dev"]
    res = {}
    for relu in (True, False):
        for bias in (True, False):
            res["y", relu, bias] = _fwd(d["x"], d["W"], d["b"] if bias else None, relu)
    for masked in (True, False):
        ym = d["y_mask"] if masked else None
        res["dx", masked] = _bwd_x(d["g"], ym, d["W"])
        res["dW", masked], res["db", masked], res["ws", masked] = _bwd_w(d["g"], ym, d["x"])
    torch.cuda.synchronize()
    c["plain"] = res
    return res


# ------------------------------------------------------------------------------------------------ a. exact equality
@pytest.mark.parametrize("name", list(R.ABI_CASES))
def test_forward_equals_float64_bit_for_bit(name):
    """relu and linear, with b and with b = NULL (on every case, E1 and E3 among them)."""
    c, res = _exact(name), _contiguous(name)
    for relu in (True, False):
        for bias in (True, False):
            _same(res["y", relu, bias], c["ref_y"][relu, bias], "%s y relu=%s bias=%s" % (name, relu, bias))
    if R.ABI_CASES[name][0] * R.ABI_CASES[name][2] >= 64:
        assert bool((c["ref_y"][True, True] == 0).any()) and bool((c["ref_y"][True, True] > 0).any())


@pytest.mark.parametrize("name", list(R.ABI_CASES))
def test_backward_equals_float64_bit_for_bit(name):
    """y given (the MASK instances) and y = NULL; dW with db, and db = NULL on E3, E6 and E9 (a null dbpart on the slab path
    where nsplit > 1), which must leave dW as it was."""
    c, res = _exact(name), _contiguous(name)
    rows, k, out = R.ABI_CASES[name]
    if rows * out >= 64:
        is_open = c["y_mask"] > 0
        for dim in (0, 1):
            assert bool(is_open.any(dim).all()) and bool((~is_open).any(dim).all()), "every row and column: open and closed cells"
    for masked in (True, False):
        dx6, dW6, db6 = c["ref_bwd"][masked]
        tag = "%s %s" % (name, "masked" if masked else "y=NULL")
        _same(res["dx", masked], dx6, tag + " dx (contraction over out = %d: %d stages)" % (out, out // R.DN_K))
        ym = c["y_mask"] if masked else None
        msg = R.first_difference(res["dW", masked].cpu(), dW6)
        assert msg is None, "%s dW (row = out index, column = in index): %s; %s" % (
            tag, msg, _which_split(name, res["ws", masked], c["g"], ym, c["x"]))
        _same(res["db", masked], db6, tag + " db")
        if name in ("E3", "E6", "E9"):
            d = c["dev"]
            dW_nodb, none, _ = _bwd_w(d["g"], d["y_mask"] if masked else None, d["x"], with_db=False)
            assert none is None
            _same(dW_nodb, dW6, tag + " dW with db = NULL")


# ------------------------------------------------------------------------------ b. pitches, padding and guards
@pytest.mark.parametrize("name", list(R.ABI_CASES))
def test_pitched_operands_same_bits_and_nothing_written_outside(name):
    c, res = _exact(name), _contiguous(name)
    dev = _dev()
    rows, k, out = R.ABI_CASES[name]
    d = c["dev"]
    nan = float("nan")
    xw = _Win(rows, k, PADS["x"], nan, dev, d["x"])
    gw = _Win(rows, out, PADS["g"], nan, dev, d["g"])
    mw = _Win(rows, out, PADS["y_mask"], nan, dev, d["y_mask"])
    assert {xw.ld - k, gw.ld - out, mw.ld - out} == {5, 7} and (xw.l, gw.l, mw.l) == (3, 1, 2)
    for relu, bias in ((True, True), (False, True), (True, False), (False, False)):
        yw = _Win(rows, out, PADS["y"], SENTINEL, dev)
        _fwd(xw.t, d["W"], d["b"] if bias else None, relu, y=yw.t)
        tag = "%s relu=%s bias=%s" % (name, relu, bias)
        _same(yw.t, res["y", relu, bias], tag + " y, ldy = %d" % yw.ld)
        assert yw.pads_untouched(), tag + ": y's padding was written"
    n_ws = _api()[1].xdfm_dense_bwd_w_ws_elems(rows, k, out)
    for masked in (True, False):
        ym = mw.t if masked else None
        tag = "%s %s" % (name, "masked" if masked else "y=NULL")
        dxw = _Win(rows, k, PADS["dx"], SENTINEL, dev)
        _bwd_x(gw.t, ym, d["W"], dx=dxw.t)
        _same(dxw.t, res["dx", masked], tag + " dx, lddx = %d" % dxw.ld)
        assert dxw.pads_untouched(), tag + ": dx's padding was written"
        for with_db in (True, False):
            got = {}
            for fill in (nan, 0.0):
                ws, dW, db = _Guarded(n_ws, fill, dev), _Guarded(out * k, SENTINEL, dev), _Guarded(out, SENTINEL, dev)
                got[fill == 0.0] = _bwd_w(gw.t, ym, xw.t, with_db=with_db, ws=ws.t, dW=dW.t, db=db.t)
                for buf, what in ((ws, "ws"), (dW, "dW"), (db, "db")):
                    assert buf.guards_untouched(), "%s db=%s: a guard of %s was written" % (tag, with_db, what)
                if not with_db:
                    want = torch.full((out,), SENTINEL, dtype=torch.float32, device=dev)
                    assert bool((R.bits(db.t) == R.bits(want)).all()), tag + ": db = NULL, yet the buffer was written"
            (dW_nan, db_nan, _), (dW_zero, db_zero, _) = got[False], got[True]
            _same(dW_nan, res["dW", masked], tag + " dW db=%s, NaN-poisoned workspace, pitched g, y, x" % with_db)
            _same(dW_zero, dW_nan, tag + " dW: zero-filled against NaN-poisoned workspace")
            if with_db:
                _same(db_nan, res["db", masked], tag + " db, NaN-poisoned workspace")
                _same(db_zero, db_nan, tag + " db: zero-filled against NaN-poisoned workspace")
    for w, what in ((xw, "x"), (gw, "g"), (mw, "y")):
        assert bool((R.bits(w.wide) == R.bits(w.before)).all()), "%s: input %s was written" % (name, what)


# ------------------------------------------------------------------------------------- c. the mask is a select
@pytest.mark.parametrize("name", ["E3", "E7", "E9"])
def test_non_finite_g_behind_a_closed_mask_stays_out(name):
    c, res = _exact(name), _contiguous(name)
    rows, k, out = R.ABI_CASES[name]
    closed = ~(c["y_mask"] > 0)
    _, kper, nsplit, last = R.split_plan(rows)
    assert bool(closed[-1].any()) and bool(closed[:, -1].any()) and bool(closed[(nsplit - 1) * kper:].any())
    if name == "E7":
        assert last == 1                                  # the last row IS the one-row last split
    poison = torch.tensor([float("inf"), float("-inf"), float("nan")])[torch.arange(rows * out).view(rows, out) % 3]
    g_bad = torch.where(closed, poison, c["g"])
    g_zero = torch.where(closed, torch.zeros_like(c["g"]), c["g"])
    assert not bool(torch.isfinite(g_bad[-1]).all()) and not bool(torch.isfinite(g_bad[:, -1]).all())
    assert {float("inf"), float("-inf")} <= set(g_bad[closed].tolist()) and bool(torch.isnan(g_bad[closed]).any())
    d = c["dev"]
    outs = {}
    for key, g_ in (("bad", g_bad.to(d["x"].device)), ("zero", g_zero.to(d["x"].device))):
        dW, db, _ = _bwd_w(g_, d["y_mask"], d["x"])
        outs[key] = dict(dx=_bwd_x(g_, d["y_mask"], d["W"]), dW=dW, db=db)
    for key in ("dx", "dW", "db"):
        assert bool(torch.isfinite(outs["bad"][key]).all()), "%s %s holds a non-finite value" % (name, key)
        _same(outs["bad"][key], outs["zero"][key], "%s %s: non-finite against zero g behind the closed mask" % (name, key))
        _same(outs["zero"][key], c["ref_bwd"][True][("dx", "dW", "db").index(key)], "%s %s" % (name, key))
        _same(outs["zero"][key], res[key, True], "%s %s against the plain call" % (name, key))


# ---------------------------------------------------------------------------------- d. standard-normal inputs
@pytest.mark.parametrize("name", ["E3", "E6", "E7", "E9"])
def test_normal_inputs_error_within_twice_the_library_paths(name):
    dev = _dev()
    rows, k, out = R.ABI_CASES[name]
    x, W, b, g = R.normal_inputs(rows, k, out, seed=2000 + rows + k)
    y_mask = R.mask_pattern(rows, out, seed=rows + out)                  # given, shared by all three computations
    xd, Wd, bd, gd, md = (t.to(dev) for t in (x, W, b, g, y_mask))
    nan = float("nan")
    xw, gw, mw = _Win(rows, k, PADS["x"], nan, dev, xd), _Win(rows, out, PADS["g"], nan, dev, gd), _Win(rows, out, PADS["y_mask"], nan, dev, md)
    yw, dxw = _Win(rows, out, PADS["y"], SENTINEL, dev), _Win(rows, k, PADS["dx"], SENTINEL, dev)
    _fwd(xw.t, Wd, bd, True, y=yw.t)
    _bwd_x(gw.t, mw.t, Wd, dx=dxw.t)
    dW, db, _ = _bwd_w(gw.t, mw.t, xw.t)
    native = dict(y=yw.t, dx=dxw.t, dW=dW, db=db)
    gz = torch.where(md > 0, gd, torch.zeros_like(gd))
    library = dict(y=torch.relu(torch.addmm(bd, xd, Wd.t())), dx=gz.mm(Wd), dW=gz.t().mm(xd), db=gz.sum(0))
    ref = dict(zip(("dx", "dW", "db"), R.dense_bwd_ref(g, y_mask, x, W)), y=R.dense_ref(x, W, b, True))
    bad = []
    for key in ("y", "dx", "dW", "db"):
        want = ref[key]
        e_nat = float((native[key].cpu().double() - want).abs().max())
        e_lib = float((library[key].cpu().double() - want).abs().max())
        floor = float(np.spacing(np.float32(want.abs().max())))
        print("%-28s %-3s native %.3e  library %.3e  floor (1 ulp) %.3e" % ("abi_%s_r%d_k%d_o%d" % (name, rows, k, out), key, e_nat, e_lib, floor))
        assert native[key].shape == want.shape
        if not e_nat <= max(FACTOR * e_lib, floor):
            bad.append((key, e_nat, e_lib, floor))
    assert yw.pads_untouched() and dxw.pads_untouched()
    assert not bad, bad


# ------------------------------------------------------------------------------------------- e. determinism
@pytest.mark.parametrize("name", ["E6", "E9"])
def test_two_calls_same_bits_on_an_uncleared_workspace(name):
    c, res = _exact(name), _contiguous(name)
    d = c["dev"]
    for masked in (True, False):
        ym = d["y_mask"] if masked else None
        dW1, db1, ws = _bwd_w(d["g"], ym, d["x"])
        dW1, db1 = dW1.clone(), db1.clone()
        dW2, db2, ws2 = _bwd_w(d["g"], ym, d["x"], ws=ws)             # the first call's workspace, as it left it
        assert ws2.data_ptr() == ws.data_ptr()
        _same(dW2, dW1, "%s dW, second call" % name)
        _same(db2, db1, "%s db, second call" % name)
        _same(dW1, res["dW", masked], "%s dW against the first call of the session" % name)
        _same(_bwd_x(d["g"], ym, d["W"]), res["dx", masked], "%s dx, second call" % name)
    _same(_fwd(d["x"], d["W"], d["b"], True), res["y", True, True], "%s y, second call" % name)
