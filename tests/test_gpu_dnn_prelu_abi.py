"""GPU tests (-m gpu) of the PReLU entry points called directly: xdfm_dense_prelu_fwd / _bwd_x / _bwd_w (csrc/dnn.hip) and
xdfm_prelu_fwd / _bwd (csrc/prelu.hip) against the float64 reference of tests/dnn_prelu_ref.py.

Exactness.  x, W, b and g are integer-valued and the slope is one of 0.25, 0, -0.5, 2, 1, with magnitudes chosen (and asserted
here in int64) so that every sum of the layer is exact in fp32 in any order: y, z, dx, dW, db and dalpha must equal float64
bit for bit (a zero of either sign counts as zero: alpha * -0.0 and 0 * negative leave signed zeros behind).  Every case holds
cells with z > 0, z < 0 and z == 0.  The dense shapes are the smallest that reach each edge of the template (ragged tiles, the
split edge, three splits, several tiles of out and in, splits longer than 256 rows); the elementwise ones straddle its 64 x 64
block.  Operands are column windows between NaN guard bands that must come back untouched, every output and the workspace
hold NaN before the call."""
import faulthandler

import numpy as np
import pytest
import torch

import dnn_prelu_ref as R

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
GUARD = 256
PAD_L, PAD_R = 1, 2                           # pitch = cols + 3
NAN = float("nan")
_CASES = {}


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


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Win:
    """A [rows][cols] window (pitch cols + 3) of a matrix of NaN between two NaN guard bands; src fills the window."""

    def __init__(self, rows, cols, dev, src=None):
        self.rows, self.cols, self.ld = rows, cols, PAD_L + cols + PAD_R
        self.buf = torch.full((GUARD + rows * self.ld + GUARD,), NAN, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + rows * self.ld].view(rows, self.ld)[:, PAD_L:PAD_L + cols]
        if src is not None:
            self.t.copy_(torch.as_tensor(src))
        self.before = self.buf.clone()

    def outside_untouched(self):
        ne = _bits(self.buf) != _bits(self.before)
        ne[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, PAD_L:PAD_L + self.cols] = False
        return not bool(ne.any())

    def unchanged(self):
        return bool((_bits(self.buf) == _bits(self.before)).all())

    def get(self):
        return self.t.cpu().numpy().astype(np.float64)


class _Vec:
    """n floats (NaN, or src) between two NaN guard bands."""

    def __init__(self, n, dev, src=None):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), NAN, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        if src is not None:
            self.t.copy_(torch.as_tensor(src).reshape(-1))
        self.before = self.buf.clone()

    def guards_untouched(self):
        ne = _bits(self.buf) != _bits(self.before)
        ne[GUARD:GUARD + self.n] = False
        return not bool(ne.any())

    def unchanged(self):
        return bool((_bits(self.buf) == _bits(self.before)).all())

    def get(self):
        return self.t.cpu().numpy().astype(np.float64)


def _same(got, want, what):
    """Equal as numbers, exactly (+0.0 == -0.0), no NaN left."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64).reshape(np.shape(got))
    assert not np.isnan(got).any(), "%s: NaN left in the output" % what
    ne = got != want
    assert not ne.any(), "%s: %d of %d cells differ; first at %r: got %r, want %r" % (
        what, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]), got[ne][0], want[ne][0])


def _case(name):
    if name not in _CASES:
        rows, k, out = R.DENSE_CASES[name]
        x, W, b, g = R.int_layer_case(rows, k, out)
        ex = R.exactness(x, W, b, g)
        assert max(ex.values()) < R.EXACT_LIMIT, (name, ex)          # int64: every fp32 sum of this case is exact in any order
        z = x.astype(np.int64) @ W.astype(np.int64).T + b.astype(np.int64)
        assert R.has_all_signs(z), name
        _CASES[name] = (x, W, b, g)
    return _CASES[name]


class _Layer:
    """One dense + PReLU layer's operands on the device and the three calls."""

    def __init__(self, name, alpha, dev):
        self.mod, self.lib, self.ops = _api()
        self.rows, self.k, self.out = R.DENSE_CASES[name]
        self.x_h, self.W_h, self.b_h, self.g_h = _case(name)
        self.alpha_h, self.dev = alpha, dev
        r, k, out = self.rows, self.k, self.out
        self.x, self.g = _Win(r, k, dev, self.x_h), _Win(r, out, dev, self.g_h)
        self.W, self.b = _Vec(out * k, dev, self.W_h), _Vec(out, dev, self.b_h)
        self.alpha = _Vec(1, dev, np.float32([alpha]))
        self.n_ws = self.lib.xdfm_dense_prelu_bwd_w_ws_elems(r, k, out)
        assert self.n_ws > 0

    def inputs_unchanged(self):
        return all(o.unchanged() for o in (self.x, self.g, self.W, self.b, self.alpha))

    def fwd(self, y, z):
        p = self.ops._ptr
        self.mod.check(self.lib.xdfm_dense_prelu_fwd(p(self.x.t), self.rows, self.k, self.x.ld, p(self.W.t), self.out, p(self.b.t), p(self.alpha.t),
                                                     p(y.t), y.ld, p(z.t) if z is not None else None, z.ld if z is not None else 0,
                                                     self.ops._stream()), "dense_prelu_fwd")

    def bwd_x(self, z, dx):
        p = self.ops._ptr
        self.mod.check(self.lib.xdfm_dense_prelu_bwd_x(p(self.g.t), self.g.ld, p(z.t), z.ld, p(self.alpha.t), self.rows, self.out, p(self.W.t),
                                                       self.k, p(dx.t), dx.ld, self.ops._stream()), "dense_prelu_bwd_x")

    def bwd_w(self, z, ws, dW, db, da):
        p = self.ops._ptr
        opt = lambda v: p(v.t) if v is not None else None
        assert ws.t.data_ptr() % 8 == 0
        self.mod.check(self.lib.xdfm_dense_prelu_bwd_w(p(self.g.t), self.g.ld, p(z.t), z.ld, p(self.alpha.t), p(self.x.t), self.x.ld, self.rows,
                                                       self.k, self.out, p(ws.t), p(dW.t), opt(db), opt(da), self.ops._stream()),
                       "dense_prelu_bwd_w")


@pytest.mark.parametrize("alpha", R.ALPHAS, ids=lambda a: "alpha%g" % a)
@pytest.mark.parametrize("name", list(R.DENSE_CASES))
def test_dense_prelu_layer_equals_float64_bit_for_bit(name, alpha):
    dev = _dev()
    L = _Layer(name, alpha, dev)
    rows, k, out = L.rows, L.k, L.out
    y_ref, z_ref = R.layer_ref(L.x_h, L.W_h, L.b_h, alpha)
    dx_ref, dW_ref, db_ref, da_ref = R.layer_bwd_ref(L.g_h, z_ref, alpha, L.x_h, L.W_h)
    # forward: y and z; z = NULL gives the same y
    y, z, y2 = _Win(rows, out, dev), _Win(rows, out, dev), _Win(rows, out, dev)
    L.fwd(y, z)
    L.fwd(y2, None)
    torch.cuda.synchronize()
    _same(y.get(), y_ref, "y")
    _same(z.get(), z_ref, "z")
    assert bool((_bits(y.t) == _bits(y2.t)).all()), "z = NULL changed y"
    assert y.outside_untouched() and z.outside_untouched() and y2.outside_untouched() and L.inputs_unchanged()
    # backward, from the z the forward stored
    zin = _Win(rows, out, dev, z.t)
    dx = _Win(rows, k, dev)
    L.bwd_x(zin, dx)
    ws, dW, db, da = _Vec(L.n_ws, dev), _Vec(out * k, dev), _Vec(out, dev), _Vec(1, dev)
    L.bwd_w(zin, ws, dW, db, da)
    torch.cuda.synchronize()
    _same(dx.get(), dx_ref, "dx")
    _same(dW.get().reshape(out, k), dW_ref, "dW")
    _same(db.get(), db_ref, "db")
    _same(da.get(), [da_ref], "dalpha")
    assert dx.outside_untouched() and zin.unchanged() and L.inputs_unchanged()
    assert all(v.guards_untouched() for v in (ws, dW, db, da))
    # db / dalpha NULL leave the other outputs' bits; a second full call gives the same bits
    for with_db, with_da in ((False, True), (True, False), (False, False), (True, True)):
        ws2, dW2 = _Vec(L.n_ws, dev), _Vec(out * k, dev)
        db2, da2 = (_Vec(out, dev) if with_db else None), (_Vec(1, dev) if with_da else None)
        L.bwd_w(zin, ws2, dW2, db2, da2)
        torch.cuda.synchronize()
        assert bool((_bits(dW2.t) == _bits(dW.t)).all()), (with_db, with_da)
        assert db2 is None or bool((_bits(db2.t) == _bits(db.t)).all())
        assert da2 is None or bool((_bits(da2.t) == _bits(da.t)).all())
        assert ws2.guards_untouched() and dW2.guards_untouched()
    dx2 = _Win(rows, k, dev)
    L.bwd_x(zin, dx2)
    torch.cuda.synchronize()
    assert bool((_bits(dx2.t) == _bits(dx.t)).all())


def test_dense_prelu_random_inputs_same_bits_on_every_run_and_dw_equals_the_plain_call_on_gz():
    """Random (inexact) inputs at the three-split shape: two calls give the same bits, and dW / db equal xdfm_dense_bwd_w's on a
    materialised gz bit for bit (the same splits and finish)."""
    dev = _dev()
    mod, lib, ops = _api()
    rows, k, out = 520, 40, 64
    gen = torch.Generator().manual_seed(5)
    x, W, b = torch.randn(rows, k, generator=gen).to(dev), (torch.randn(out, k, generator=gen) / 6).to(dev), torch.randn(out, generator=gen).to(dev)
    g = torch.randn(rows, out, generator=gen).to(dev)
    alpha = torch.tensor([-0.3], device=dev)
    p, st = ops._ptr, ops._stream
    y, z = torch.empty(rows, out, device=dev), torch.empty(rows, out, device=dev)
    mod.check(lib.xdfm_dense_prelu_fwd(p(x), rows, k, k, p(W), out, p(b), p(alpha), p(y), out, p(z), out, st()), "fwd")
    outs = []
    for _ in range(2):
        ws = torch.full((lib.xdfm_dense_prelu_bwd_w_ws_elems(rows, k, out),), NAN, device=dev)
        dW, db, da, dx = torch.empty(out, k, device=dev), torch.empty(out, device=dev), torch.empty(1, device=dev), torch.empty(rows, k, device=dev)
        mod.check(lib.xdfm_dense_prelu_bwd_w(p(g), out, p(z), out, p(alpha), p(x), k, rows, k, out, p(ws), p(dW), p(db), p(da), st()), "bwd_w")
        mod.check(lib.xdfm_dense_prelu_bwd_x(p(g), out, p(z), out, p(alpha), rows, out, p(W), k, p(dx), k, st()), "bwd_x")
        outs.append((dW, db, da, dx))
    torch.cuda.synchronize()
    for a, c in zip(*outs):
        assert bool((_bits(a) == _bits(c)).all()) and bool(torch.isfinite(a).all())
    gz = torch.where(z > 0, g, alpha * g)
    ws = torch.empty(lib.xdfm_dense_bwd_w_ws_elems(rows, k, out), device=dev)
    dW0, db0, dx0 = torch.empty(out, k, device=dev), torch.empty(out, device=dev), torch.empty(rows, k, device=dev)
    mod.check(lib.xdfm_dense_bwd_w(p(gz), out, None, 0, p(x), k, rows, k, out, p(ws), p(dW0), p(db0), st()), "plain bwd_w")
    mod.check(lib.xdfm_dense_bwd_x(p(gz), out, None, 0, rows, out, p(W), k, p(dx0), k, st()), "plain bwd_x")
    torch.cuda.synchronize()
    assert bool((_bits(dW0) == _bits(outs[0][0])).all()) and bool((_bits(db0) == _bits(outs[0][1])).all())
    assert bool((_bits(dx0) == _bits(outs[0][3])).all())
    exact = R.prelu_bwd_ref(g.cpu().numpy(), z.cpu().numpy(), -0.3)[1]
    assert abs(float(outs[0][2]) - exact) <= R.dalpha_bound(g.cpu().numpy(), z.cpu().numpy(), exact)


@pytest.mark.parametrize("alpha", R.ALPHAS, ids=lambda a: "alpha%g" % a)
@pytest.mark.parametrize("shape", R.ELEMENTWISE_CASES, ids=lambda s: "%dx%d" % s)
def test_elementwise_prelu_equals_float64_bit_for_bit(shape, alpha):
    dev = _dev()
    mod, lib, ops = _api()
    rows, cols = shape
    u_h, g_h = R.int_elementwise_case(rows, cols)
    assert R.UNIT * int(np.abs(g_h.astype(np.int64) * u_h.astype(np.int64)).sum()) < R.EXACT_LIMIT
    p, st = ops._ptr, ops._stream
    u, g, a = _Win(rows, cols, dev, u_h), _Win(rows, cols, dev, g_h), _Vec(1, dev, np.float32([alpha]))
    y = _Win(rows, cols, dev)
    mod.check(lib.xdfm_prelu_fwd(p(u.t), u.ld, rows, cols, p(a.t), p(y.t), y.ld, st()), "prelu_fwd")
    n_ws = lib.xdfm_prelu_ws_elems(rows, cols)

    def bwd(with_du, with_da):
        du, da, ws = (_Win(rows, cols, dev) if with_du else None), (_Vec(1, dev) if with_da else None), _Vec(n_ws, dev)
        assert ws.t.data_ptr() % 8 == 0
        mod.check(lib.xdfm_prelu_bwd(p(g.t), g.ld, p(u.t), u.ld, rows, cols, p(a.t), p(du.t) if du else None, du.ld if du else 0,
                                     p(da.t) if da else None, p(ws.t), st()), "prelu_bwd")
        torch.cuda.synchronize()
        assert ws.guards_untouched() and (du is None or du.outside_untouched()) and (da is None or da.guards_untouched())
        if not with_da:
            assert ws.unchanged(), "the workspace is not touched without dalpha"
        return du, da

    du, da = bwd(True, True)
    du_ref, da_ref = R.prelu_bwd_ref(g_h, u_h, alpha)
    _same(y.get(), R.prelu_ref(u_h, alpha), "y")
    _same(du.get(), du_ref, "du")
    _same(da.get(), [da_ref], "dalpha")
    assert y.outside_untouched() and u.unchanged() and g.unchanged() and a.unchanged()
    du2, _ = bwd(True, False)
    _, da2 = bwd(False, True)
    du3, da3 = bwd(True, True)
    assert bool((_bits(du2.t) == _bits(du.t)).all()) and bool((_bits(du3.t) == _bits(du.t)).all())
    assert bool((_bits(da2.t) == _bits(da.t)).all()) and bool((_bits(da3.t) == _bits(da.t)).all())
