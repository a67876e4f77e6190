"""GPU tests (-m gpu) of the batch-norm entry points of csrc/bn.hip called directly (xdfm_bn_fwd_train, xdfm_bn_fwd_eval,
xdfm_bn_bwd, xdfm_bn_bwd_eval) against the float64 reference of tests/dnn_bn_ref.py on the same fp32 inputs.

Shapes.  R = xdfm_bn_row_block(): rows in {2, 3, R-1, R, R+1, 3R+5} x cols in {1, 31, 32, 33, 40, 264} x the three
activations.  z, y, g and dz are column windows (pitch cols + 3) between guard bands that must come back untouched; the
workspace and every output hold NaN before the call.

Bar (that of tests/test_gpu_dnn.py).  For each output the native result's largest error against float64 may exceed the
largest error of the STOCK torch sequence on the GPU -- F.batch_norm + activation, autograd for the backward -- by at most a
factor 2, with a floor of one fp32 ulp of the output's largest magnitude: both are fp32 accumulations of the same length
that differ in order.

Each entry point is measured against float64 on its own inputs.  The forward's are z, gamma, beta and the running
statistics.  The backward's are g, z, gamma and what the forward stored: y, save_mean, save_rstd.  Its reference therefore
takes those three as the kernel reads them -- fp32 values -- and not a float64 forward's: the ReLU mask of a cell within
rounding of zero must be the same for everyone (as in tests/test_gpu_dnn.py), and over two rows dz is eps / (var + eps) of
its terms, 1e-5 of them, so that the last bit of the stored rstd decides half of its digits: against a float64 forward
both implementations would show the rounding of their stored statistics, 1e5 times amplified, and the comparison would be
one of two noises (measured at 2 x 1, relu: native 9.9e-10, stock 3.4e-10 on a dz of 2.2e-7).  The composite, z to dz, is
measured against a float64 replay at 65 rows in tests/test_gpu_dnn_bn.py.

Exactness.  Integer-valued z with a power-of-two row count: save_mean equals the float64 mean bit for bit.  Integer-valued g
with relu or linear: dbeta equals the float64 sum bit for bit.  Both catch a dropped or doubled row at a block edge."""
import faulthandler

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dnn_bn_ref as B

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
FACTOR = 2.0
EPS, MOM = 1e-5, 0.1
GUARD = 256
SENTINEL = -24681.357
PAD_L, PAD_R = 1, 2                           # pitch = cols + 3
COLS = (1, 31, 32, 33, 40, 264)
ACT_CODE = {"linear": 0, "relu": 1, "sigmoid": 2}
T_ACT = {"linear": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid}
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


def _row_block():
    from xdfm_amd import _lib
    return int(_lib.load().xdfm_bn_row_block())


def _rows_list():
    R = _row_block()
    return [2, 3, R - 1, R, R + 1, 3 * R + 5]


ROW_IDS = ["2", "3", "R-1", "R", "R+1", "3R+5"]


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Win:
    """A [rows][cols] window (pitch cols + 3) of a matrix whose padding holds SENTINEL, between two guard bands."""

    def __init__(self, rows, cols, fill, dev, src=None):
        self.rows, self.cols, self.ld = rows, cols, PAD_L + cols + PAD_R
        self.buf = torch.full((GUARD + rows * self.ld + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        wide = self.buf[GUARD:GUARD + rows * self.ld].view(rows, self.ld)
        self.t = wide[:, PAD_L:PAD_L + cols]
        self.t.fill_(fill)
        if src is not None:
            self.t.copy_(src)
        self.before = self.buf.clone()

    def outside_untouched(self):
        ne = _bits(self.buf) != _bits(self.before)
        ne[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, PAD_L:PAD_L + self.cols] = False
        return not bool(ne.any())

    def unchanged(self):
        return bool((_bits(self.buf) == _bits(self.before)).all())


class _Vec:
    """n floats holding `fill` between two guard bands."""

    def __init__(self, n, fill, dev, src=None):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)
        if src is not None:
            self.t.copy_(src)

    def guards_untouched(self):
        want = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device=self.buf.device)
        return bool((_bits(self.buf[:GUARD]) == _bits(want)).all()) and bool((_bits(self.buf[GUARD + self.n:]) == _bits(want)).all())


def _ld(t):
    return max(int(t.stride(0)), int(t.shape[1]))


def _fwd_train(z, gamma, beta, act, y, mean, rstd, rm, rv, ws):
    mod, lib, ops = _api()
    rows, cols = z.shape
    assert ws.numel() == lib.xdfm_bn_ws_elems(rows, cols)
    mod.check(lib.xdfm_bn_fwd_train(ops._ptr(z), _ld(z), rows, cols, ops._ptr(gamma), ops._ptr(beta), EPS, MOM, ACT_CODE[act], ops._ptr(y),
                                    _ld(y), ops._ptr(mean), ops._ptr(rstd), ops._ptr(rm), ops._ptr(rv), ops._ptr(ws), ops._stream()), "bn_fwd_train")


def _fwd_eval(z, gamma, beta, act, y, rm, rv):
    mod, lib, ops = _api()
    rows, cols = z.shape
    mod.check(lib.xdfm_bn_fwd_eval(ops._ptr(z), _ld(z), rows, cols, ops._ptr(gamma), ops._ptr(beta), EPS, ACT_CODE[act], ops._ptr(y), _ld(y),
                                   ops._ptr(rm), ops._ptr(rv), ops._stream()), "bn_fwd_eval")


def _bwd(g, y, z, gamma, mean, rstd, act, dz, dgamma, dbeta, ws, frozen=False):
    mod, lib, ops = _api()
    rows, cols = z.shape
    fn = lib.xdfm_bn_bwd_eval if frozen else lib.xdfm_bn_bwd
    mod.check(fn(ops._ptr(g), _ld(g), ops._ptr(y), _ld(y), ops._ptr(z), _ld(z), rows, cols, ops._ptr(gamma), ops._ptr(mean), ops._ptr(rstd),
                 ACT_CODE[act], ops._ptr(dz), _ld(dz) if dz is not None else 0, ops._ptr(dgamma), ops._ptr(dbeta), ops._ptr(ws), ops._stream()),
              "bn_bwd")


def _draw(rows, cols, seed, shifted=False, integer=False):
    gen = torch.Generator().manual_seed(seed)
    if integer:
        z = torch.randint(-8, 9, (rows, cols), generator=gen).float()
        g = torch.randint(-3, 4, (rows, cols), generator=gen).float()
    else:
        z = torch.randn(rows, cols, generator=gen) * (0.5 + 2.5 * torch.rand(cols, generator=gen)) + 2.0 * torch.randn(cols, generator=gen)
        g = torch.randn(rows, cols, generator=gen)
    if shifted:
        z[:, 0] = 1000.0 + torch.randn(rows, generator=gen)
    gamma = 0.5 + torch.rand(cols, generator=gen)
    beta = 0.5 * torch.randn(cols, generator=gen)
    rm = torch.randn(cols, generator=gen)
    rv = 0.5 + 1.5 * torch.rand(cols, generator=gen)
    return dict(z=z, g=g, gamma=gamma, beta=beta, rm=rm, rv=rv)


def _case(rows, cols, act, shifted=False, integer=False):
    """Inputs, the native results (pitched, guarded, NaN-poisoned), the stock sequence's and the float64 reference, once."""
    key = (rows, cols, act, shifted, integer)
    if key in _CACHE:
        return _CACHE[key]
    mod, lib, ops = _api()
    dev = _dev()
    nan = float("nan")
    h = _draw(rows, cols, 7000 + 131 * rows + 7 * cols + ACT_CODE[act], shifted, integer)
    d = {k: v.to(dev) for k, v in h.items()}
    zw, gw = _Win(rows, cols, nan, dev, d["z"]), _Win(rows, cols, nan, dev, d["g"])
    yw, dzw = _Win(rows, cols, nan, dev), _Win(rows, cols, nan, dev)
    n_ws = lib.xdfm_bn_ws_elems(rows, cols)
    vec = {k: _Vec(cols, nan, dev) for k in ("mean", "rstd", "dgamma", "dbeta")}
    vec["rm"], vec["rv"] = _Vec(cols, nan, dev, d["rm"]), _Vec(cols, nan, dev, d["rv"])
    ws_f, ws_b = _Vec(n_ws, nan, dev), _Vec(n_ws, nan, dev)
    _fwd_train(zw.t, d["gamma"], d["beta"], act, yw.t, vec["mean"].t, vec["rstd"].t, vec["rm"].t, vec["rv"].t, ws_f.t)
    _bwd(gw.t, yw.t, zw.t, d["gamma"], vec["mean"].t, vec["rstd"].t, act, dzw.t, vec["dgamma"].t, vec["dbeta"].t, ws_b.t)
    torch.cuda.synchronize()
    native = dict(y=yw.t.clone(), save_mean=vec["mean"].t.clone(), save_rstd=vec["rstd"].t.clone(), running_mean=vec["rm"].t.clone(),
                  running_var=vec["rv"].t.clone(), dz=dzw.t.clone(), dgamma=vec["dgamma"].t.clone(), dbeta=vec["dbeta"].t.clone())
    guards = dict(z=zw.unchanged(), g=gw.unchanged(), y=yw.outside_untouched(), dz=dzw.outside_untouched(), ws_f=ws_f.guards_untouched(),
                  ws_b=ws_b.guards_untouched(), **{k: v.guards_untouched() for k, v in vec.items()})
    # the stock sequence on the GPU: F.batch_norm + activation, autograd; the ReLU mask is the native output's
    zs, gs, bs = (d[k].clone().requires_grad_(True) for k in ("z", "gamma", "beta"))
    rm_s, rv_s = d["rm"].clone(), d["rv"].clone()
    xbn = F.batch_norm(zs, rm_s, rv_s, gs, bs, True, MOM, EPS)
    y_s = T_ACT[act](xbn)
    if act == "relu":
        xbn.backward(torch.where(native["y"] > 0, d["g"], torch.zeros_like(d["g"])))
    else:
        y_s.backward(d["g"])
    # the statistics F.batch_norm keeps to itself, from the operator underneath it
    _, mean_s, rstd_s = torch.native_batch_norm(d["z"], d["gamma"], d["beta"], d["rm"].clone(), d["rv"].clone(), True, MOM, EPS)
    stock = dict(y=y_s.detach(), save_mean=mean_s, save_rstd=rstd_s, running_mean=rm_s, running_var=rv_s,
                 dz=zs.grad, dgamma=gs.grad, dbeta=bs.grad)
    torch.cuda.synchronize()
    r = B.fwd_train(h["z"].numpy(), h["gamma"].numpy(), h["beta"].numpy(), EPS, MOM, act, h["rm"].numpy(), h["rv"].numpy())
    # the backward entry point in float64 on ITS inputs: g, z, gamma and the y, save_mean, save_rstd the forward stored
    dz6, dg6, db6 = B.bwd(h["g"].numpy(), native["y"].cpu().numpy(), h["z"].numpy(), h["gamma"].numpy(), native["save_mean"].cpu().numpy(),
                          native["save_rstd"].cpu().numpy(), act)
    ref = dict(y=r["y"], save_mean=r["mean"], save_rstd=r["rstd"], running_mean=r["running_mean"], running_var=r["running_var"], dz=dz6,
               dgamma=dg6, dbeta=db6)
    c = dict(host=h, dev=d, native=native, stock=stock, ref=ref, guards=guards, wins=dict(z=zw, g=gw, y=yw), vec=vec)
    _CACHE[key] = c
    return c


def _judge(tag, native, stock, ref):
    """Print every (native, stock, floor) triple, then assert the bar on all of them."""
    bad = []
    for key, want in ref.items():
        want = np.asarray(want, np.float64)
        got = native[key].detach().cpu().double().numpy()
        assert got.shape == want.shape, (key, got.shape, want.shape)
        assert np.isfinite(got).all(), "%s %s holds a non-finite value" % (tag, key)
        e_nat = float(np.abs(got - want).max())
        e_stock = float(np.abs(stock[key].detach().cpu().double().numpy() - want).max())
        floor = float(np.spacing(np.float32(np.abs(want).max())))
        print("%-30s %-12s native %.3e  stock %.3e  floor (1 ulp) %.3e" % (tag, key, e_nat, e_stock, floor))
        if not e_nat <= max(FACTOR * e_stock, floor):
            bad.append((key, e_nat, e_stock, floor))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("ri", range(6), ids=ROW_IDS)
def test_training_forward_and_backward_within_twice_the_stock_sequences_error(ri, cols, act):
    rows = _rows_list()[ri]
    c = _case(rows, cols, act)
    assert all(c["guards"].values()), "written outside its operand: %r" % ([k for k, ok in c["guards"].items() if not ok],)
    if act == "relu" and rows * cols >= 64:
        zeros = int((c["native"]["y"] == 0).sum())
        assert 0 < zeros < rows * cols, "the ReLU case must hold exact zeros and live cells"
    _judge("r%d_c%d_%s" % (rows, cols, act), c["native"], c["stock"], c["ref"])


@pytest.mark.parametrize("act", B.ACTS)
def test_a_column_with_mean_1000_keeps_its_variance(act):
    """z[:, 0] = 1000 + N(0, 1) beside ordinary columns: E[z^2] - mean^2 in fp32 would miss that column's variance by several
    per cent (the squares are 1e6 with an ulp of 0.06); the (mean, M2) pairs keep it to rounding."""
    R = _row_block()
    rows, cols = 3 * R + 5, 40
    c = _case(rows, cols, act, shifted=True)
    assert all(c["guards"].values())
    rstd, want = float(c["native"]["save_rstd"][0]), float(c["ref"]["save_rstd"][0])
    print("column 0: save_rstd native %.7f, float64 %.7f (relative error %.2e)" % (rstd, want, abs(rstd - want) / want))
    assert abs(rstd - want) <= 1e-5 * want
    _judge("shifted_r%d_c%d_%s" % (rows, cols, act), c["native"], c["stock"], c["ref"])


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("ri", range(6), ids=ROW_IDS)
def test_integer_inputs_give_exact_mean_and_exact_dbeta(ri, cols):
    rows = _rows_list()[ri]
    for act in ("relu", "linear"):
        c = _case(rows, cols, act, integer=True)
        assert all(c["guards"].values())
        h, nat = c["host"], c["native"]
        if rows & (rows - 1) == 0:                 # a power of two: the mean of small integers is an fp32 number
            want = h["z"].double().mean(0).float()
            assert bool((_bits(nat["save_mean"].cpu()) == _bits(want)).all()), (rows, cols, act, "save_mean")
        gm = B.act_bwd(nat["y"].cpu().numpy(), h["g"].double().numpy(), act)
        want = torch.from_numpy(gm.sum(0) + 0.0).float()
        got = nat["dbeta"].cpu() + 0.0
        assert bool((_bits(got) == _bits(want)).all()), (rows, cols, act, "dbeta", got, want)


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("ri,cols", [(1, 33), (4, 40), (5, 264)], ids=["3x33", "R+1x40", "3R+5x264"])
def test_two_calls_give_the_same_bits_and_null_outputs_leave_the_others_alone(ri, cols, act):
    mod, lib, ops = _api()
    dev = _dev()
    rows = _rows_list()[ri]
    c = _case(rows, cols, act)
    d, nat, w = c["dev"], c["native"], c["wins"]
    nan = float("nan")
    n_ws = lib.xdfm_bn_ws_elems(rows, cols)

    def buf(*shape):
        return torch.full(shape, nan, dtype=torch.float32, device=dev)

    y2, mean2, rstd2, rm2, rv2 = buf(rows, cols), buf(cols), buf(cols), d["rm"].clone(), d["rv"].clone()
    _fwd_train(d["z"], d["gamma"], d["beta"], act, y2, mean2, rstd2, rm2, rv2, buf(n_ws))       # contiguous this time: same bits
    for got, key in ((y2, "y"), (mean2, "save_mean"), (rstd2, "save_rstd"), (rm2, "running_mean"), (rv2, "running_var")):
        assert bool((_bits(got) == _bits(nat[key])).all()), key
    for drop in (None, "dz", "dgamma", "dbeta", "dz+dgamma", "dgamma+dbeta"):
        outs = dict(dz=buf(rows, cols), dgamma=buf(cols), dbeta=buf(cols))
        for k in (drop.split("+") if drop else ()):
            outs[k] = None
        _bwd(w["g"].t, w["y"].t, w["z"].t, d["gamma"], nat["save_mean"], nat["save_rstd"], act, outs["dz"], outs["dgamma"], outs["dbeta"], buf(n_ws))
        for k, t in outs.items():
            if t is not None:
                assert bool((_bits(t) == _bits(nat[k])).all()), "%s with %s = NULL" % (k, drop)
    torch.cuda.synchronize()


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("ri,cols", [(0, 1), (1, 33), (3, 32), (4, 40), (5, 264)], ids=["2x1", "3x33", "Rx32", "R+1x40", "3R+5x264"])
def test_evaluation_forward_and_its_backward_against_float64(ri, cols, act):
    dev = _dev()
    rows = _rows_list()[ri]
    if (ri, cols) == (0, 1):
        rows = 1                                    # evaluation takes a single row
    nan = float("nan")
    h = _draw(rows, cols, 9000 + 131 * rows + 7 * cols + ACT_CODE[act])
    d = {k: v.to(dev) for k, v in h.items()}
    zw, gw, yw, dzw = _Win(rows, cols, nan, dev, d["z"]), _Win(rows, cols, nan, dev, d["g"]), _Win(rows, cols, nan, dev), _Win(rows, cols, nan, dev)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    _fwd_eval(zw.t, d["gamma"], d["beta"], act, yw.t, rm, rv)
    assert torch.equal(rm, d["rm"]) and torch.equal(rv, d["rv"]), "evaluation must not touch the running statistics"
    rstd = torch.rsqrt(d["rv"] + EPS)
    _, lib, _ = _api()
    dg, db, ws = (_Vec(n, nan, dev) for n in (cols, cols, lib.xdfm_bn_ws_elems(rows, cols)))
    _bwd(gw.t, yw.t, zw.t, d["gamma"], d["rm"], rstd, act, dzw.t, dg.t, db.t, ws.t, frozen=True)
    torch.cuda.synchronize()
    assert zw.unchanged() and gw.unchanged() and yw.outside_untouched() and dzw.outside_untouched()
    assert dg.guards_untouched() and db.guards_untouched() and ws.guards_untouched()
    native = dict(y=yw.t.clone(), dz=dzw.t.clone(), dgamma=dg.t.clone(), dbeta=db.t.clone())
    zs, gs, bs = (d[k].clone().requires_grad_(True) for k in ("z", "gamma", "beta"))
    xbn = F.batch_norm(zs, d["rm"].clone(), d["rv"].clone(), gs, bs, False, MOM, EPS)
    y_s = T_ACT[act](xbn)
    if act == "relu":
        xbn.backward(torch.where(native["y"] > 0, d["g"], torch.zeros_like(d["g"])))
    else:
        y_s.backward(d["g"])
    stock = dict(y=y_s.detach(), dz=zs.grad, dgamma=gs.grad, dbeta=bs.grad)
    y6 = B.fwd_eval(h["z"].numpy(), h["gamma"].numpy(), h["beta"].numpy(), EPS, act, h["rm"].numpy(), h["rv"].numpy())
    dz6, dg6, db6 = B.bwd(h["g"].numpy(), native["y"].cpu().numpy(), h["z"].numpy(), h["gamma"].numpy(), h["rm"].numpy(), rstd.cpu().numpy(),
                          act, frozen=True)
    _judge("eval_r%d_c%d_%s" % (rows, cols, act), native, stock, dict(y=y6, dz=dz6, dgamma=dg6, dbeta=db6))
