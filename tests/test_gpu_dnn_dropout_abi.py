"""GPU tests (-m gpu) of the dropout entry points of csrc/dnn.hip called directly (xdfm_dense_fwd_drop,
xdfm_dense_bwd_x_drop, xdfm_dense_bwd_w_drop, xdfm_dense_dropout_mask).

Inputs are small integers and p is 0.5 or 0.75, so the scale is exactly 2 or 4 and every sum is exact in fp32 whatever
its order (|x|, |W|, |b|, |g| <= 3: a product with the scale is at most 36, a sum of 8225 of them stays below 2^24): y, dx,
dW and db must equal the float64 reference bit for bit, given the mask -- which must equal the numpy mirror of the hash
(tests/dnn_dropout_ref.py) bit for bit.

Cases (rows, in, out): one row; the flagship's first layer at 33 rows; one past a tile in every dimension; 256 rows (one
split); 2049 rows, pitched between guard bands (9 splits, the last one row); 8225 rows (29 splits in a workspace for 32)."""
import faulthandler

import numpy as np
import pytest
import torch

import dnn_dropout_ref as D
import dnn_ref as R

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
CASES = {
    "r1_k13_o32": (1, 13, 32),
    "r33_k429_o256": (33, 429, 256),
    "r65_k65_o96": (65, 65, 96),
    "r256_k33_o32": (256, 33, 32),
    "r2049_k40_o64": (2049, 40, 64),          # pitched, between guard bands
    "r8225_k65_o96": (8225, 65, 96),          # 29 splits
}
PITCHED = "r2049_k40_o64"
PS = (0.5, 0.75)
SEED, LAYER, ROW0 = 1234567891011, 1, 0
GUARD = 256
SENTINEL = -24681.357
PADS = {"x": (3, 2), "g": (1, 4), "y": (5, 1), "dx": (1, 3)}
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


def _ld(t):
    return max(int(t.stride(0)), int(t.shape[1]))


def _seed(dev, value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _mask(rows, out, p, seed, layer=LAYER, row0=ROW0):
    mod, lib, ops = _api()
    keep = torch.full((rows, out), 7, dtype=torch.uint8, device=seed.device)
    mod.check(lib.xdfm_dense_dropout_mask(rows, out, p, ops._ptr(seed), layer, row0, ops._ptr(keep), ops._stream()), "dense_dropout_mask")
    return keep


def _fwd(x, W, b, p, seed, layer=LAYER, row0=ROW0, y=None, act=1):
    mod, lib, ops = _api()
    rows, k = x.shape
    out = W.shape[0]
    if y is None:
        y = torch.empty(rows, out, dtype=torch.float32, device=x.device)
    mod.check(lib.xdfm_dense_fwd_drop(ops._ptr(x), rows, k, _ld(x), ops._ptr(W), out, ops._ptr(b), act, ops._ptr(y), _ld(y), p,
                                      ops._ptr(seed), layer, row0, ops._stream()), "dense_fwd_drop")
    return y


def _bwd_x(g, y, W, p, dx=None):
    mod, lib, ops = _api()
    rows, out = g.shape
    k = W.shape[1]
    if dx is None:
        dx = torch.empty(rows, k, dtype=torch.float32, device=g.device)
    mod.check(lib.xdfm_dense_bwd_x_drop(ops._ptr(g), _ld(g), ops._ptr(y), _ld(y) if y is not None else 0, rows, out, ops._ptr(W), k,
                                        ops._ptr(dx), _ld(dx), p, ops._stream()), "dense_bwd_x_drop")
    return dx


def _bwd_w(g, y, x, p, ws=None, dW=None, db=None):
    mod, lib, ops = _api()
    rows, out = g.shape
    k = x.shape[1]
    n_ws = lib.xdfm_dense_bwd_w_ws_elems(rows, k, out)
    if ws is None:
        ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=g.device)     # poisoned: nothing in it is read unwritten
    assert ws.numel() == n_ws
    if dW is None:
        dW = torch.empty(out * k, dtype=torch.float32, device=g.device)
    if db is None:
        db = torch.empty(out, dtype=torch.float32, device=g.device)
    mod.check(lib.xdfm_dense_bwd_w_drop(ops._ptr(g), _ld(g), ops._ptr(y), _ld(y) if y is not None else 0, ops._ptr(x), _ld(x), rows, k,
                                        out, ops._ptr(ws), ops._ptr(dW), ops._ptr(db), p, ops._stream()), "dense_bwd_w_drop")
    return dW.view(out, k), db


def _same(got, want, what):
    msg = R.first_difference(got.detach().cpu(), want.detach().cpu())
    assert msg is None, "%s: %s" % (what, msg)


class _Win:
    """A [rows][cols] column window of a wider matrix filled with `fill`, itself between two guard bands of GUARD sentinel
    rows' worth of floats: .t is the window (pitch .ld)."""

    def __init__(self, rows, cols, pads, fill, dev, src=None):
        self.l, self.cols, self.rows = pads[0], cols, rows
        self.ld = pads[0] + cols + pads[1]
        self.buf = torch.full((GUARD + rows * self.ld + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.wide = self.buf[GUARD:GUARD + rows * self.ld].view(rows, self.ld)
        self.wide.fill_(fill)
        self.t = self.wide[:, self.l:self.l + cols]
        if src is not None:
            self.t.copy_(src)
        self.before = self.buf.clone()

    def outside_untouched(self):
        ne = (R.bits(self.buf) != R.bits(self.before))
        ne[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, self.l:self.l + self.cols] = False
        return not bool(ne.any())


class _Guarded:
    def __init__(self, n, fill, dev):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)

    def guards_untouched(self):
        want = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device=self.buf.device)
        return bool((R.bits(self.buf[:GUARD]) == R.bits(want)).all()) and bool((R.bits(self.buf[GUARD + self.n:]) == R.bits(want)).all())


def _case(name, p):
    """Integer inputs of a case, the mirror's mask, the float64 references and the device results, once."""
    key = (name, p)
    if key in _CACHE:
        return _CACHE[key]
    dev = _dev()
    rows, k, out = CASES[name]
    x, W, b, g = R.int_inputs(rows, k, out, seed=300 + rows + k + out)
    keep = D.keep_mask(rows, out, p, SEED, LAYER, ROW0)
    z, d6 = D.layer_ref(x, W, b, keep, p)
    dx6, dW6, db6 = D.layer_bwd_ref(g, d6, x, W, p)
    c = dict(x=x, W=W, b=b, g=g, keep=keep, z=z, d=d6.float(), dx=dx6.float(), dW=dW6.float(), db=db6.float(),
             dev={n: t.to(dev) for n, t in dict(x=x, W=W, b=b, g=g).items()}, seed=_seed(dev))
    assert float(d6.abs().max()) < 2 ** 24 and max(float(t.abs().max()) for t in (dx6, dW6, db6)) < 2 ** 24
    dv = c["dev"]
    c["got_keep"] = _mask(rows, out, p, c["seed"])
    c["got_d"] = _fwd(dv["x"], dv["W"], dv["b"], p, c["seed"])
    c["got_dx"] = _bwd_x(dv["g"], c["got_d"], dv["W"], p)
    c["got_dW"], c["got_db"] = _bwd_w(dv["g"], c["got_d"], dv["x"], p)
    torch.cuda.synchronize()
    _CACHE[key] = c
    return c


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", list(CASES))
def test_mask_equals_the_numpy_mirror_bit_for_bit(name, p):
    c = _case(name, p)
    got = c["got_keep"].cpu().numpy()
    assert set(np.unique(got).tolist()) <= {0, 1}
    ne = got.astype(bool) != c["keep"]
    assert not ne.any(), "%s p=%g: %d of %d keep bits differ, first at %r" % (name, p, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_equal_float64_bit_for_bit(name, p):
    c = _case(name, p)
    rows, k, out = CASES[name]
    _same(c["got_d"], c["d"], "%s p=%g y" % (name, p))
    # the stored output is the mask: positive exactly where kept and z > 0
    want_open = torch.as_tensor(c["keep"]) & (c["z"] > 0)
    assert bool(((c["got_d"].cpu() > 0) == want_open).all())
    _same(c["got_dx"], c["dx"], "%s p=%g dx" % (name, p))
    _same(c["got_dW"], c["dW"], "%s p=%g dW (row = out index, column = in index)" % (name, p))
    _same(c["got_db"], c["db"], "%s p=%g db" % (name, p))
    # kept fraction of the positive pre-activations within 5 sigma of 1 - p
    pos = c["z"] > 0
    n = int(pos.sum())
    if n >= 64:
        frac = float((c["got_d"].cpu() > 0)[pos].double().mean())
        sd = float(np.sqrt(p * (1 - p) / n))
        print("%s p=%g: kept %.4f of %d positive pre-activations (%.2f sigma)" % (name, p, frac, n, abs(frac - (1 - p)) / sd))
        assert abs(frac - (1 - p)) <= 5 * sd


@pytest.mark.parametrize("name", ["r65_k65_o96", "r2049_k40_o64"])
def test_layer_row0_and_seed_change_the_mask_and_the_same_seed_repeats_it(name):
    p = 0.5
    c = _case(name, p)
    rows, k, out = CASES[name]
    dev, dv = _dev(), c["dev"]
    base = c["got_keep"]
    assert torch.equal(_mask(rows, out, p, c["seed"]), base)
    _same(_fwd(dv["x"], dv["W"], dv["b"], p, c["seed"]), c["got_d"], name + " y, second call with the same seed")
    for what, kw, mirror in (("layer", dict(layer=LAYER + 1), dict(layer=LAYER + 1, row0=ROW0, seed=SEED)),
                             ("row0", dict(row0=5), dict(layer=LAYER, row0=5, seed=SEED)),
                             ("seed", dict(), dict(layer=LAYER, row0=ROW0, seed=SEED + 1))):
        seed = _seed(dev, mirror["seed"])
        got = _mask(rows, out, p, seed, **kw)
        frac = float((got != base).float().mean())
        assert 0.4 < frac < 0.6, (what, frac)
        want = D.keep_mask(rows, out, p, mirror["seed"], mirror["layer"], mirror["row0"])
        assert np.array_equal(got.cpu().numpy().astype(bool), want), what
        y = _fwd(dv["x"], dv["W"], dv["b"], p, seed, **kw)
        _same(y, D.layer_ref(c["x"], c["W"], c["b"], want, p)[1].float(), "%s y with another %s" % (name, what))
    if rows > 5:                                   # row0 = 5: rows 5 .. of the row0 = 0 mask
        assert torch.equal(_mask(rows - 5, out, p, c["seed"], row0=5), base[5:])
    # the seed is read on the device at run time: same launch arguments, new value in the same cell
    cell = _seed(dev)
    first = _mask(rows, out, p, cell)
    cell.fill_(SEED + 1)
    assert not torch.equal(_mask(rows, out, p, cell), first)


@pytest.mark.parametrize("p", PS)
def test_pitched_operands_guards_and_poisoned_workspace(p):
    name = PITCHED
    c = _case(name, p)
    dev, dv = _dev(), c["dev"]
    rows, k, out = CASES[name]
    nan = float("nan")
    xw = _Win(rows, k, PADS["x"], nan, dev, dv["x"])
    gw = _Win(rows, out, PADS["g"], nan, dev, dv["g"])
    yw = _Win(rows, out, PADS["y"], SENTINEL, dev)
    dxw = _Win(rows, k, PADS["dx"], SENTINEL, dev)
    _fwd(xw.t, dv["W"], dv["b"], p, c["seed"], y=yw.t)
    _same(yw.t, c["d"], "%s p=%g pitched y" % (name, p))
    assert yw.outside_untouched(), "y: padding or guard written"
    yw.before = yw.buf.clone()
    _bwd_x(gw.t, yw.t, dv["W"], p, dx=dxw.t)
    _same(dxw.t, c["dx"], "%s p=%g pitched dx" % (name, p))
    assert dxw.outside_untouched(), "dx: padding or guard written"
    n_ws = _api()[1].xdfm_dense_bwd_w_ws_elems(rows, k, out)
    ws, dW, db = _Guarded(n_ws, nan, dev), _Guarded(out * k, SENTINEL, dev), _Guarded(out, SENTINEL, dev)
    got_dW, got_db = _bwd_w(gw.t, yw.t, xw.t, p, ws=ws.t, dW=dW.t, db=db.t)
    _same(got_dW, c["dW"], "%s p=%g dW, NaN-poisoned workspace, pitched g, y, x" % (name, p))
    _same(got_db, c["db"], "%s p=%g db, NaN-poisoned workspace" % (name, p))
    for buf, what in ((ws, "ws"), (dW, "dW"), (db, "db")):
        assert buf.guards_untouched(), "a guard of %s was written" % what
    for w, what in ((xw, "x"), (gw, "g"), (yw, "y")):
        assert bool((R.bits(w.buf) == R.bits(w.before)).all()), "input %s was written" % what


@pytest.mark.parametrize("name", ["r65_k65_o96", "r2049_k40_o64", "r8225_k65_o96"])
def test_non_finite_g_behind_dropped_and_relu_closed_cells_stays_out(name):
    p = 0.5
    c = _case(name, p)
    dv = c["dev"]
    keep = torch.as_tensor(c["keep"])
    dropped = ~keep & (c["z"] > 0)                # z > 0, d == 0
    closed = ~(c["z"] > 0)                        # the ReLU's own zeros, kept or not
    assert bool(dropped.any()) and bool(closed.any()) and bool((closed & keep).any())
    assert bool(dropped[-1].any() or closed[-1].any())
    rows, out = c["g"].shape
    poison = torch.tensor([float("inf"), float("-inf"), float("nan")])[torch.arange(rows * out).view(rows, out) % 3]
    g_bad = torch.where(dropped | closed, poison, c["g"])
    assert bool(torch.isnan(g_bad[dropped]).any()) and bool(torch.isinf(g_bad[closed]).any())
    g_bad = g_bad.to(dv["x"].device)
    dx = _bwd_x(g_bad, c["got_d"], dv["W"], p)
    dW, db = _bwd_w(g_bad, c["got_d"], dv["x"], p)
    for got, key in ((dx, "dx"), (dW, "dW"), (db, "db")):
        assert bool(torch.isfinite(got).all()), "%s %s holds a non-finite value" % (name, key)
        _same(got, c[key], "%s %s with non-finite g behind the closed cells" % (name, key))


@pytest.mark.parametrize("name", ["r33_k429_o256", "r65_k65_o96", "r8225_k65_o96"])
def test_p_zero_is_the_plain_entry_points_bit_for_bit(name):
    """Standard-normal inputs (so that the order of the sums shows): p_drop = 0 through the _drop entry points, seed NULL or
    not, relu and linear, y given and y = NULL."""
    mod, lib, ops = _api()
    dev = _dev()
    rows, k, out = CASES[name]
    x, W, b, g = (t.to(dev) for t in R.normal_inputs(rows, k, out, seed=77 + rows))
    seed = _seed(dev)

    def plain_fwd(act):
        y = torch.empty(rows, out, dtype=torch.float32, device=dev)
        mod.check(lib.xdfm_dense_fwd(ops._ptr(x), rows, k, k, ops._ptr(W), out, ops._ptr(b), act, ops._ptr(y), out, ops._stream()), "dense_fwd")
        return y

    for act in (0, 1):
        want = plain_fwd(act)
        assert torch.equal(_fwd(x, W, b, 0.0, None, act=act), want)
        assert torch.equal(_fwd(x, W, b, 0.0, seed, layer=3, row0=9, act=act), want)
    y = plain_fwd(1)
    for ym in (y, None):
        dx = torch.empty(rows, k, dtype=torch.float32, device=dev)
        mod.check(lib.xdfm_dense_bwd_x(ops._ptr(g), out, ops._ptr(ym), out if ym is not None else 0, rows, out, ops._ptr(W), k, ops._ptr(dx), k,
                                       ops._stream()), "dense_bwd_x")
        assert torch.equal(_bwd_x(g, ym, W, 0.0), dx)
        ws = torch.empty(lib.xdfm_dense_bwd_w_ws_elems(rows, k, out), dtype=torch.float32, device=dev)
        dW, db = torch.empty(out, k, dtype=torch.float32, device=dev), torch.empty(out, dtype=torch.float32, device=dev)
        mod.check(lib.xdfm_dense_bwd_w(ops._ptr(g), out, ops._ptr(ym), out if ym is not None else 0, ops._ptr(x), k, rows, k, out, ops._ptr(ws),
                                       ops._ptr(dW), ops._ptr(db), ops._stream()), "dense_bwd_w")
        got_dW, got_db = _bwd_w(g, ym, x, 0.0)
        assert torch.equal(got_dW, dW) and torch.equal(got_db, db)
    assert torch.equal(_mask(rows, out, 0.0, seed), torch.ones(rows, out, dtype=torch.uint8, device=dev))
