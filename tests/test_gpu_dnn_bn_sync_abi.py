"""GPU tests (-m gpu) of the synchronised batch-norm entry points of csrc/bn.hip called directly (xdfm_bn_stats,
xdfm_bn_fwd_apply_sync, xdfm_bn_bwd_sums, xdfm_bn_bwd_apply_sync), the ranks of a row-parallel step emulated in one process:
the rows are split into shards, xdfm_bn_stats runs per shard, the triples are concatenated as the all-gather would deliver
them, the apply kernel runs per shard; the same for the backward.

Shapes.  R = xdfm_bn_row_block(): shards (R + 3, 1, a stand-in, 2R - 1) -- more than one row block, a one-row shard, a rank
that only holds row 0 of the global batch with count 0, a ragged last block -- and the single shard (70,), world 1; cols 40
and 96 (below and above one column block of 64), pitches cols + 3; relu, sigmoid, linear.  Column 0 is 1000 + N(0, 1), as in
tests/test_gpu_dnn_bn_abi.py: raw sums of squares would lose its variance.  z, y, g and dz are column windows between guard
bands that must come back untouched; the workspaces and every output hold NaN before the call.

Bar (that of tests/test_gpu_dnn_bn_abi.py).  The reference is float64 of the GLOBAL batch (tests/dnn_bn_ref.py), the
yardstick the stock torch sequence on the same device over the concatenated rows -- F.batch_norm + activation, autograd.
For each output the native result's largest error may exceed the yardstick's by at most a factor 2, with a floor of one fp32
ulp of the output's largest magnitude.  As there, the backward is measured on ITS inputs: the float64 backward takes the y,
save_mean and save_rstd the forward stored.  dgamma and dbeta are judged as the sum over the shards of what each wrote."""
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
COLS = (40, 96)
SPLIT_IDS = ("four_ranks", "one_rank")
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


def _counts(split):
    """Rows of the global batch per rank; 0 is a rank that holds only a stand-in row."""
    from xdfm_amd import _lib
    R = int(_lib.load().xdfm_bn_row_block())
    return (R + 3, 1, 0, 2 * R - 1) if split == "four_ranks" else (70,)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


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
    """n numbers holding `fill` between two guard bands."""

    def __init__(self, n, fill, dev, src=None, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)
        if src is not None:
            self.t.copy_(src)

    def guards_untouched(self):
        want = torch.full((GUARD,), SENTINEL, dtype=self.buf.dtype, device=self.buf.device)
        return bool((_bits(self.buf[:GUARD]) == _bits(want)).all()) and bool((_bits(self.buf[GUARD + self.n:]) == _bits(want)).all())


def _ld(t):
    return max(int(t.stride(0)), int(t.shape[1]))


def _stats(z, pair, ws):
    mod, lib, ops = _api()
    rows, cols = z.shape
    assert ws.numel() == lib.xdfm_bn_ws_elems(rows, cols) and pair.numel() == 2 * cols and pair.dtype == torch.float64
    mod.check(lib.xdfm_bn_stats(ops._ptr(z), _ld(z), rows, cols, ops._ptr(pair), ops._ptr(ws), ops._stream()), "bn_stats")


def _fwd_apply(z, gathered, world, gamma, beta, act, y, mean, rstd, rm, rv):
    mod, lib, ops = _api()
    rows, cols = z.shape
    assert gathered.numel() == world * (1 + 2 * cols) and gathered.dtype == torch.float64 and gathered.is_contiguous()
    mod.check(lib.xdfm_bn_fwd_apply_sync(ops._ptr(z), _ld(z), rows, cols, ops._ptr(gathered), world, ops._ptr(gamma), ops._ptr(beta), EPS,
                                         MOM, ACT_CODE[act], ops._ptr(y), _ld(y), ops._ptr(mean), ops._ptr(rstd), ops._ptr(rm), ops._ptr(rv),
                                         ops._stream()), "bn_fwd_apply_sync")


def _bwd_sums(g, y, z, mean, rstd, act, sums, ws):
    mod, lib, ops = _api()
    rows, cols = z.shape
    assert ws.numel() == lib.xdfm_bn_ws_elems(rows, cols) and sums.numel() == 2 * cols and sums.dtype == torch.float64
    mod.check(lib.xdfm_bn_bwd_sums(ops._ptr(g), _ld(g), ops._ptr(y), _ld(y), ops._ptr(z), _ld(z), rows, cols, ops._ptr(mean), ops._ptr(rstd),
                                   ACT_CODE[act], ops._ptr(sums), ops._ptr(ws), ops._stream()), "bn_bwd_sums")


def _bwd_apply(g, y, z, counted, gathered, world, rank, n_total, gamma, mean, rstd, act, dz, dgamma, dbeta):
    mod, lib, ops = _api()
    rows, cols = z.shape
    assert gathered.numel() == world * 2 * cols and gathered.dtype == torch.float64 and gathered.is_contiguous()
    mod.check(lib.xdfm_bn_bwd_apply_sync(ops._ptr(g), _ld(g), ops._ptr(y), _ld(y), ops._ptr(z), _ld(z), rows, rows if counted else 0, cols,
                                         ops._ptr(gathered), world, rank, n_total, ops._ptr(gamma), ops._ptr(mean), ops._ptr(rstd),
                                         ACT_CODE[act], ops._ptr(dz), _ld(dz) if dz is not None else 0, ops._ptr(dgamma), ops._ptr(dbeta),
                                         ops._stream()), "bn_bwd_apply_sync")


def _draw(rows, cols, seed):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, cols, generator=gen) * (0.5 + 2.5 * torch.rand(cols, generator=gen)) + 2.0 * torch.randn(cols, generator=gen)
    # the shards' statistics differ: the rows drift with their index
    z = z + torch.linspace(0.0, 3.0, rows)[:, None]
    z[:, 0] = 1000.0 + torch.randn(rows, generator=gen)
    g = torch.randn(rows, cols, generator=gen)
    gamma = 0.5 + torch.rand(cols, generator=gen)
    beta = 0.5 * torch.randn(cols, generator=gen)
    rm = torch.randn(cols, generator=gen)
    rv = 0.5 + 1.5 * torch.rand(cols, generator=gen)
    return dict(z=z, g=g, gamma=gamma, beta=beta, rm=rm, rv=rv)


def _shards(t, counts):
    out, lo = [], 0
    for c in counts:
        out.append(t[lo:lo + c] if c > 0 else t[0:1])
        lo += c
    return out


def _run_ranks(d, counts, cols, act, dev, pitched, drop=()):
    """The emulated step: per rank its outputs and guard verdicts.  `pitched`: operands as guarded column windows with NaN in
    every output; otherwise plain contiguous tensors.  `drop`: outputs of the backward passed as NULL."""
    _, lib, _ = _api()
    nan = float("nan")
    world, n_total = len(counts), sum(counts)
    zs, gs = _shards(d["z"], counts), _shards(d["g"], counts)
    gs = [g if c > 0 else torch.zeros_like(g) for g, c in zip(gs, counts)]       # a stand-in's root gradient is zero
    ranks, guards = [], {}

    def win(rows, src=None):
        if pitched:
            return _Win(rows, cols, nan, dev, src)
        w = type("Plain", (), {})()
        w.t = torch.full((rows, cols), nan, dtype=torch.float32, device=dev) if src is None else src.clone()
        w.unchanged = w.outside_untouched = lambda: True
        return w

    # forward, first half: every rank's pair, then the "all-gather"
    f_all = _Vec(world * (1 + 2 * cols), nan, dev, dtype=torch.float64)
    for r, (z, c) in enumerate(zip(zs, counts)):
        k = dict(rows=z.shape[0], count=c, z=win(z.shape[0], z), g=win(z.shape[0], gs[r]), y=win(z.shape[0]), dz=win(z.shape[0]))
        k["ws_f"] = _Vec(lib.xdfm_bn_ws_elems(z.shape[0], cols), nan, dev)
        k["ws_b"] = _Vec(lib.xdfm_bn_ws_elems(z.shape[0], cols), nan, dev)
        row = f_all.t[r * (1 + 2 * cols):(r + 1) * (1 + 2 * cols)]
        row[0] = float(c)
        _stats(k["z"].t, row[1:], k["ws_f"].t)
        ranks.append(k)
    # forward, second half: every rank applies the merged statistics and updates ITS replica of the running vectors
    for r, k in enumerate(ranks):
        k["vec"] = {n: _Vec(cols, nan, dev) for n in ("mean", "rstd", "dgamma", "dbeta")}
        k["vec"]["rm"], k["vec"]["rv"] = _Vec(cols, nan, dev, d["rm"]), _Vec(cols, nan, dev, d["rv"])
        v = k["vec"]
        _fwd_apply(k["z"].t, f_all.t, world, d["gamma"], d["beta"], act, k["y"].t, v["mean"].t, v["rstd"].t, v["rm"].t, v["rv"].t)
    # backward, first half
    b_all = _Vec(world * 2 * cols, nan, dev, dtype=torch.float64)
    for r, k in enumerate(ranks):
        v = k["vec"]
        _bwd_sums(k["g"].t, k["y"].t, k["z"].t, v["mean"].t, v["rstd"].t, act, b_all.t[r * 2 * cols:(r + 1) * 2 * cols], k["ws_b"].t)
    for r, k in enumerate(ranks):
        v = k["vec"]
        _bwd_apply(k["g"].t, k["y"].t, k["z"].t, k["count"] > 0, b_all.t, world, r, n_total, d["gamma"], v["mean"].t, v["rstd"].t, act,
                   None if "dz" in drop else k["dz"].t, None if "dgamma" in drop else v["dgamma"].t,
                   None if "dbeta" in drop else v["dbeta"].t)
    torch.cuda.synchronize()
    guards["gathered"] = f_all.guards_untouched() and b_all.guards_untouched()
    for r, k in enumerate(ranks):
        guards["r%d" % r] = (k["z"].unchanged() and k["g"].unchanged() and k["y"].outside_untouched() and k["dz"].outside_untouched()
                             and k["ws_f"].guards_untouched() and k["ws_b"].guards_untouched()
                             and all(v.guards_untouched() for v in k["vec"].values()))
    return ranks, guards, f_all.t.clone(), b_all.t.clone()


def _case(split, cols, act):
    """Inputs, the native results (pitched, guarded, NaN-poisoned), the stock sequence's and the float64 reference, once."""
    key = (split, cols, act)
    if key in _CACHE:
        return _CACHE[key]
    dev = _dev()
    counts = _counts(split)
    n = sum(counts)
    h = _draw(n, cols, 8000 + 131 * n + 7 * cols + ACT_CODE[act])
    d = {k: v.to(dev) for k, v in h.items()}
    ranks, guards, f_all, b_all = _run_ranks(d, counts, cols, act, dev, pitched=True)
    counted = [k for k in ranks if k["count"] > 0]
    native = dict(y=torch.cat([k["y"].t for k in counted]), dz=torch.cat([k["dz"].t for k in counted]),
                  dgamma=torch.stack([k["vec"]["dgamma"].t.double() for k in ranks]).sum(0),
                  dbeta=torch.stack([k["vec"]["dbeta"].t.double() for k in ranks]).sum(0),
                  save_mean=ranks[0]["vec"]["mean"].t.clone(), save_rstd=ranks[0]["vec"]["rstd"].t.clone(),
                  running_mean=ranks[0]["vec"]["rm"].t.clone(), running_var=ranks[0]["vec"]["rv"].t.clone())
    # the stock sequence on the GPU over the concatenated rows; the ReLU mask is the native output's
    zs, gs, bs = (d[k].clone().requires_grad_(True) for k in ("z", "gamma", "beta"))
    rm_s, rv_s = d["rm"].clone(), d["rv"].clone()
    xbn = F.batch_norm(zs, rm_s, rv_s, gs, bs, True, MOM, EPS)
    y_s = T_ACT[act](xbn)
    if act == "relu":
        xbn.backward(torch.where(native["y"] > 0, d["g"], torch.zeros_like(d["g"])))
    else:
        y_s.backward(d["g"])
    _, mean_s, rstd_s = torch.native_batch_norm(d["z"], d["gamma"], d["beta"], d["rm"].clone(), d["rv"].clone(), True, MOM, EPS)
    stock = dict(y=y_s.detach(), save_mean=mean_s, save_rstd=rstd_s, running_mean=rm_s, running_var=rv_s, dz=zs.grad, dgamma=gs.grad,
                 dbeta=bs.grad)
    torch.cuda.synchronize()
    r = B.fwd_train(h["z"].numpy(), h["gamma"].numpy(), h["beta"].numpy(), EPS, MOM, act, h["rm"].numpy(), h["rv"].numpy())
    dz6, dg6, db6 = B.bwd(h["g"].numpy(), native["y"].cpu().numpy(), h["z"].numpy(), h["gamma"].numpy(), native["save_mean"].cpu().numpy(),
                          native["save_rstd"].cpu().numpy(), act)
    ref = dict(y=r["y"], save_mean=r["mean"], save_rstd=r["rstd"], running_mean=r["running_mean"], running_var=r["running_var"], dz=dz6,
               dgamma=dg6, dbeta=db6)
    c = dict(host=h, dev=d, counts=counts, ranks=ranks, native=native, stock=stock, ref=ref, guards=guards, f_all=f_all, b_all=b_all)
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
@pytest.mark.parametrize("split", SPLIT_IDS)
def test_every_output_within_twice_the_stock_sequences_error(split, cols, act):
    c = _case(split, cols, act)
    assert all(c["guards"].values()), "written outside its operand: %r" % ([k for k, ok in c["guards"].items() if not ok],)
    if act == "relu":
        zeros = int((c["native"]["y"] == 0).sum())
        assert 0 < zeros < c["native"]["y"].numel(), "the ReLU case must hold exact zeros and live cells"
    _judge("%s_c%d_%s" % (split, cols, act), c["native"], c["stock"], c["ref"])
    # column 0 is 1000 + N(0, 1): the merged pairs keep its variance
    rstd, want = float(c["native"]["save_rstd"][0]), float(c["ref"]["save_rstd"][0])
    print("column 0: save_rstd native %.7f, float64 %.7f (relative error %.2e)" % (rstd, want, abs(rstd - want) / want))
    assert abs(rstd - want) <= 1e-5 * want


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("cols", COLS)
def test_replicas_agree_and_the_stand_in_gets_exact_zeros(cols, act):
    c = _case("four_ranks", cols, act)
    ranks, counts = c["ranks"], c["counts"]
    # every rank merged the same gathered bytes in the same order: statistics and running vectors are the same bits
    for k in ranks[1:]:
        for name in ("mean", "rstd", "rm", "rv"):
            assert bool((_bits(k["vec"][name].t) == _bits(ranks[0]["vec"][name].t)).all()), name
    stand_in = ranks[counts.index(0)]
    assert stand_in["rows"] == 1
    assert bool((_bits(stand_in["dz"].t) == 0).all()), "the stand-in's dz must be exact (+0) zeros"
    assert bool((stand_in["vec"]["dgamma"].t == 0).all()) and bool((stand_in["vec"]["dbeta"].t == 0).all())
    # the other ranks' sums are not zero: without the flag the stand-in's dz would not be
    assert float(c["b_all"].abs().max()) > 0
    # its y is row 0 of the global batch under the global statistics: the bits rank 0 wrote for that row
    assert bool((_bits(stand_in["y"].t[0]) == _bits(ranks[0]["y"].t[0])).all())
    # the gathered counts and the count-0 rank's pair (its own row: M2 = 0)
    f_all = c["f_all"].view(len(counts), 1 + 2 * cols)
    assert f_all[:, 0].tolist() == [float(x) for x in counts]
    assert bool((f_all[counts.index(0), 1 + cols:] == 0).all())


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("split,cols", [("four_ranks", 40), ("one_rank", 96)])
def test_two_runs_give_the_same_bits_and_null_outputs_leave_the_others_alone(split, cols, act):
    dev = _dev()
    c = _case(split, cols, act)
    first = c["ranks"]
    for drop in ((), ("dz",), ("dgamma",), ("dbeta",), ("dz", "dgamma"), ("dgamma", "dbeta")):
        again, _, f_all, b_all = _run_ranks(c["dev"], c["counts"], cols, act, dev, pitched=False, drop=drop)   # contiguous this time
        assert bool((_bits(f_all) == _bits(c["f_all"])).all()) and bool((_bits(b_all) == _bits(c["b_all"])).all())
        for a, b in zip(first, again):
            assert bool((_bits(a["y"].t) == _bits(b["y"].t)).all()), "y"
            for name in ("mean", "rstd", "rm", "rv"):
                assert bool((_bits(a["vec"][name].t) == _bits(b["vec"][name].t)).all()), name
            for name, x, y in (("dz", a["dz"].t, b["dz"].t), ("dgamma", a["vec"]["dgamma"].t, b["vec"]["dgamma"].t),
                               ("dbeta", a["vec"]["dbeta"].t, b["vec"]["dbeta"].t)):
                if name in drop:
                    assert bool(torch.isnan(y).all()), "%s was passed as NULL and must not be written" % name
                else:
                    assert bool((_bits(x) == _bits(y)).all()), "%s with %r = NULL" % (name, drop)
