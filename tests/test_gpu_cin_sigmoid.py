"""GPU tests (-m gpu) of the sigmoid CIN activation (XDFM_ACT_SIGMOID = 2).

Per kernel, through the C ABI, against float64
  forward   xdfm_cin_level_fwd with act = 2 on one row per kernel family (shapes of tests/test_gpu_cin_instances.py, the
            instance probe asserted as there).  Gaussian inputs; the test first asserts ON THE REFERENCE that at least 90 %
            of the float64 pre-activations z have |z| < 8 (a condition on the inputs).  Per element
                |got - sigmoid64(z64)| <= 1/4 K mag + E |ref| + 2^-24 |ref|
            K and mag as in test_gpu_cin_instances.py (2^-18 for f16x3 and fp32-MFMA, 2^-6 for bf16; mag = the contraction
            on absolute values), 1/4 = the Lipschitz constant of the sigmoid, E = 4 x the worst relative error of the CPU's
            float32 torch.sigmoid against float64 on 6 000 001 points of [-30, 30] (floor 4 * 2^-24), computed when the
            test runs.  E = 5.89e-7 (9.9 * 2^-24) where this file was written; the test prints its own.
  backward  xdfm_cin_dout_det and the fused xdfm_cin_bwd_prep with act = 2 on a given fp32 output A in [0, 1] (exact 0.0
            and 1.0, the fp32 neighbours of both within 2^-24), dHid / dDirect of both signs with exact zeros, split and
            no-split layouts, pooled and feature-map dDirect (tests/cin_sigmoid_cases.py).  The kernels compute
                s = dHid + dDirect;  d = fma(-A, A, A);  dOut = s * d
            n = 3 roundings, so |dOut - dOut64| <= 3 * 2^-24 (|dHid| + |dDirect|) A (1 - A), the float64 truth formed from
            the same stored fp32 A.  dbias against the float64 row sums of the fp32 dOut at gamma(N) * sum |dOut| (the
            column-sum bar of tests/head_reg_ref.py), the same bits from two calls; dW of xdfm_cin_level_bwd_w_prepared on
            the fused pass's planes against float64 dOut @ Z^T at K mag + 2^-24 |ref|.
  refusal   act = 3 returns 1 from the five entry points that take `act`, with "unsupported activation".

Layer and model: ops.cin_stack against the two reference goldens and the oracle in the three cin_math settings, on the
full-output path only (which entry points ran is watched directly: the instance probes do not encode where dX takes dOut
from); xDeepFM against sigmoid/model_sigmoid_small.npz at model_sum_small's bars; xDeepFMAttention against the oracle; the
graph-replayed train step against its eager twin; a relu model after a sigmoid one.
"""
import ctypes
import faulthandler
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy
F, B16 = 1, 2
K = {0: 2.0 ** -18, F: 2.0 ** -18, B16: 2.0 ** -6}
SIGMOID = 2
STEP_LIMIT_S = 240
MODEL_GOLDEN = "sigmoid/model_sigmoid_small"


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


class _Options:
    """library options for one block; every one is restored afterwards"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from xdfm_amd import _lib
        self.old = {k: _lib.get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        from xdfm_amd import _lib
        for k, v in self.old.items():
            _lib.set_option(k, v)


# ---------------------------------------------------------------------------------------------------------------------
# forward kernels
# ---------------------------------------------------------------------------------------------------------------------
_E = []


def sigmoid_E():
    if not _E:
        z = torch.linspace(-30, 30, 6_000_001, dtype=torch.float64).float()
        ref = torch.sigmoid(z.double())
        worst = float(((torch.sigmoid(z).double() - ref).abs() / ref).max())
        _E.append(max(4.0 * worst, 4.0 * 2.0 ** -24))
        print("E = %.4g (worst relative error of the CPU's float32 sigmoid %.4g)" % (_E[0], worst))
    return _E[0]


#   m, H, Hp, N, cin_math, level 0 (x_prev is x0), forward instance the host must pick (0 = fp32-MFMA)
FWD_ROWS = [
    (5, 7, 3, 1000, F, 0, 0),          # fp32-MFMA, cin_fwd_kernel: odd m, one partial row tile
    (13, 130, 11, 3000, F, 0, 0),      # fp32-MFMA, cin_fwd_kernel<8>: odd m, H > 128
    (25, 100, 7, 3000, F, 0, 0),       # fp32-MFMA, cin_fwd_mp_kernel<4, 1, 13>: 13 j-pairs per i
    (8, 33, 17, 1000, F, 0, 2430),     # f16x3 `ma`
    (22, 129, 9, 2000, F, 0, 4430),    # f16x3 `mb`
    (22, 48, 22, 3000, F, 1, 2431),    # f16x3 folded level 0
    (8, 65, 21, 3000, B16, 0, 4410),   # bf16
    (26, 256, 26, 2052, F, 1, 8431),   # f16x3 folded level 0 with 8 row tiles per wave (the bench's level 0 instance family)
]


@pytest.mark.parametrize("row", FWD_ROWS, ids=["m%d-H%d-Hp%d-N%d-math%d-l0%d" % r[:6] for r in FWD_ROWS])
def test_forward_kernel_vs_float64(row):
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    m, H, Hp, N, math, fold, want_inst = row
    g = torch.Generator(device=dev).manual_seed(((m * 1009 + H) * 1009 + Hp) * 31 + math)
    W = torch.randn((H, Hp * m), generator=g, device=dev) * 0.1
    bias = torch.randn((H,), generator=g, device=dev) * 0.1
    x0 = torch.randn((m, N), generator=g, device=dev)
    xp = x0 if fold else torch.randn((Hp, N), generator=g, device=dev)
    Z = (xp.double()[:, None, :] * x0.double()[None, :, :]).reshape(Hp * m, N)
    z64 = W.double() @ Z + bias.double()[:, None]
    mag = W.double().abs() @ Z.abs() + bias.double().abs()[:, None]
    inside = float((z64.abs() < 8).double().mean())
    assert inside >= 0.9, "inputs: only %.3f of |z| < 8" % inside
    ref = torch.sigmoid(z64)
    E = sigmoid_E()
    with _Options(cin_math=math, last_fwd_inst=-1):
        pack = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_cin_fwd_pack(_p(W), H, Hp, m, _p(pack), st), "cin_fwd_pack")
        out = torch.full((H, N), 7.0, device=dev)
        _lib.check(lib.xdfm_cin_level_fwd(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, SIGMOID, _p(out), st), "cin_level_fwd")
        torch.cuda.synchronize()
        assert (_lib.get_option("last_fwd_inst"), _lib.get_option("last_fwd_kernel")) == (want_inst, math if want_inst else 0)
    got = out.double()
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    bound = 0.25 * K[math] * mag + E * ref + 2.0 ** -24 * ref
    print("forward %s: %.3f of |z| < 8, worst err / bound %.3g, worst err %.3g" % (row, inside, float((err / bound).max()), float(err.max())))
    over = err > bound
    assert not bool(over.any()), "%d elements over the bar, worst err / bound %.3g" % (int(over.sum()), float((err / bound).max()))
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


def test_forward_ex_epilogue_with_sigmoid():
    """xdfm_cin_level_fwd_ex accepts act = 2 without a mask: kept rows and direct-connect sums of the same outputs that
    xdfm_cin_level_fwd gives (its sums against float64 sums of those fp32 outputs at gamma(D)); a mask is refused."""
    import head_reg_ref as R
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    m, H, Hp, Bn, D = 8, 100, 13, 128, 16
    N, hid = Bn * D, 50
    g = torch.Generator(device=dev).manual_seed(5)
    W = torch.randn((H, Hp * m), generator=g, device=dev) * 0.1
    bias, x0, xp = torch.randn((H,), generator=g, device=dev) * 0.1, torch.randn((m, N), generator=g, device=dev), torch.randn((Hp, N), generator=g, device=dev)
    with _Options(cin_math=F):
        pack = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_cin_fwd_pack(_p(W), H, Hp, m, _p(pack), st), "cin_fwd_pack")
        full = torch.empty((H, N), device=dev)
        _lib.check(lib.xdfm_cin_level_fwd(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, SIGMOID, _p(full), st), "cin_level_fwd")
        kept = torch.full((hid, N), 7.0, device=dev)
        res = torch.full((Bn, H - hid + 4), 7.0, device=dev)
        _lib.check(lib.xdfm_cin_level_fwd_ex(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, SIGMOID, _p(kept), hid, _p(res), res.shape[1], 4,
                                             hid, D, None, 0, st), "cin_level_fwd_ex")
        mk = torch.zeros(((N + 31) // 32, H), dtype=torch.int32, device=dev)
        rc = lib.xdfm_cin_level_fwd_ex(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, SIGMOID, _p(kept), hid, _p(res), res.shape[1], 4,
                                       hid, D, _p(mk), H, st)
        assert rc == 1 and "mask must be NULL" in lib.xdfm_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(kept, full[:hid])
    assert bool((res[:, :4] == 7.0).all())
    want = full[hid:].double().reshape(H - hid, Bn, D)
    err = (res[:, 4:].double() - want.sum(-1).t()).abs()
    assert bool((err <= float(R.gamma(D)) * want.abs().sum(-1).t()).all())


# ---------------------------------------------------------------------------------------------------------------------
# backward kernels
# ---------------------------------------------------------------------------------------------------------------------
N_ROUNDINGS = 3          # s = dHid + dDirect; d = fma(-A, A, A); dOut = s * d
_PLAIN = {}


def _plain_run(dev):
    import cin_sigmoid_cases as C
    if not _PLAIN:
        _PLAIN.update(C.run_cases(dev))
    return _PLAIN


def _check_backward(out, tag):
    import cin_sigmoid_cases as C
    import head_reg_ref as R
    for name in C.CASES:
        c = C.make_case(name)
        gh, gd = C.sources64(c)
        y = c["A"].astype(np.float64)
        slope = y * (1.0 - y)
        want = (gh + gd) * slope
        bound = N_ROUNDINGS * 2.0 ** -24 * (np.abs(gh) + np.abs(gd)) * slope
        d0, d1 = out[name + "/0/dOut"], out[name + "/1/dOut"]
        assert d0.dtype == np.float32 and np.isfinite(d0).all()
        err = np.abs(d0.astype(np.float64) - want)
        frac = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max())
        print("%s %-26s dOut: %.3g of the %d-rounding bar" % (tag, name, frac, N_ROUNDINGS))
        assert (err <= bound).all(), "%s: %d elements of dOut over the bar (worst %.3g of it)" % (name, int((err > bound).sum()), frac)
        assert not d0[(c["A"] == 0.0) | (c["A"] == 1.0)].any(), "dOut must be exactly 0 where the output is exactly 0 or 1"
        assert d0.tobytes() == d1.tobytes(), name + ": dOut of a second call has other bits"
        b0, b1 = out[name + "/0/dbias"], out[name + "/1/dbias"]
        assert b0.tobytes() == b1.tobytes(), name + ": dbias of a second call has other bits"
        sums, a = d0.sum(axis=1, dtype=np.float64), np.abs(d0).sum(axis=1, dtype=np.float64)
        bbound = R.gamma(c["N"]) * a
        bfrac = float((np.abs(b0 - sums) / bbound).max())
        print("%s %-26s dbias: %.3g of the bound" % (tag, name, bfrac))
        assert (np.abs(b0 - sums) <= bbound).all(), (name, bfrac)
        if c["Hp"]:
            Z = (c["xp"].astype(np.float64)[:, None, :] * c["x0"].astype(np.float64)[None, :, :]).reshape(c["Hp"] * c["m"], c["N"])
            dW64, mag = want @ Z.T, np.abs(want) @ np.abs(Z).T
            w0, w1 = out[name + "/0/dW"], out[name + "/1/dW"]
            assert w0.tobytes() == w1.tobytes(), name + ": dW of a second call has other bits"
            assert int(out[name + "/0/bww_inst"]) == {1: 4830, 2: 4810}[c["math"]]       # as the rows of test_gpu_cin_instances.py
            excess = np.abs(w0 - dW64) - 2.0 ** -24 * np.abs(dW64)
            wfrac = float((excess / (K[c["math"]] * mag)).max())
            print("%s %-26s dW: %.3g of K mag" % (tag, name, wfrac))
            assert (excess <= K[c["math"]] * mag + 1e-30).all(), (name, wfrac)


def test_backward_kernels_vs_float64_two_launch_finish():
    _check_backward(_plain_run(_dev()), "two-launch")


def test_unknown_activation_is_refused_by_all_five_entry_points():
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    m, H, Hp, Bn, D = 8, 100, 13, 128, 4
    N = Bn * D
    t = lambda *s: torch.zeros(s, device=dev)
    W, bias, x0, xp, out, dh, dd, dbias = t(H, Hp * m), t(H), t(m, N), t(Hp, N), t(H, N), t(H, N), t(Bn, H), t(H)
    with _Options(cin_math=F):
        pack = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.xdfm_cin_bwd_prep_ws_elems(H, Hp, m, Bn, D), dtype=torch.float32, device=dev)
        bws = torch.empty(lib.xdfm_cin_bwd_w_ws_elems(H, Hp, m, N), dtype=torch.float32, device=dev)
        flag = ctypes.c_int(0)
        for act in (3, -1, 258):
            calls = {
                "cin_level_fwd": lambda: lib.xdfm_cin_level_fwd(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, act, _p(out), st),
                "cin_level_fwd_ex": lambda: lib.xdfm_cin_level_fwd_ex(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, act, _p(out), H, None, 0, 0,
                                                                     H, D, None, 0, st),
                "cin_dout": lambda: lib.xdfm_cin_dout(_p(out), H, Bn, D, act, _p(dh), 0, H, _p(dd), 0, H, 0, 0, H, _p(out), _p(dbias), st),
                "cin_dout_det": lambda: lib.xdfm_cin_dout_det(_p(out), H, Bn, D, act, _p(dh), 0, H, _p(dd), 0, H, 0, 0, H, _p(out), _p(dbias),
                                                             _p(ws), st),
                "cin_bwd_prep": lambda: lib.xdfm_cin_bwd_prep(_p(out), None, 0, H, Bn, D, act, _p(dh), 0, H, _p(dd), 0, H, 0, 0, H, _p(dh), _p(dbias),
                                                             _p(ws), _p(xp), _p(x0), Hp, m, _p(bws), ctypes.byref(flag), st),
            }
            for name, call in calls.items():
                assert call() == 1, (name, act)
                msg = lib.xdfm_last_error().decode()
                assert "unsupported activation" in msg, (name, msg)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# layer
# ---------------------------------------------------------------------------------------------------------------------
def close(got, want, rtol=2e-5, atol=2e-6, msg=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


def gclose(got, want, msg=""):
    want = np.asarray(want)
    close(got, want, rtol=2e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-9, msg=msg)


class _Watch:
    """counts the calls of the lean-path entry points and records the `mask` argument of xdfm_cin_bwd_prep"""

    def __init__(self, monkeypatch):
        from xdfm_amd import _lib
        lib = _lib.load()
        self.calls = {"xdfm_cin_level_fwd_ex": 0, "xdfm_cin_level_bwd_x_src": 0, "xdfm_cin_level_fwd": 0, "xdfm_cin_level_bwd_x_ex": 0}
        self.prep_masks = []
        for name in self.calls:
            monkeypatch.setattr(lib, name, self._counted(name, getattr(lib, name)), raising=True)
        prep = lib.xdfm_cin_bwd_prep

        def watched_prep(A, mask, *rest):
            self.prep_masks.append((A, mask))
            return prep(A, mask, *rest)
        monkeypatch.setattr(lib, "xdfm_cin_bwd_prep", watched_prep, raising=True)

    def _counted(self, name, fn):
        def call(*a):
            self.calls[name] += 1
            return fn(*a)
        return call

    def full_output_path_only(self, levels):
        assert self.calls["xdfm_cin_level_fwd_ex"] == 0 and self.calls["xdfm_cin_level_bwd_x_src"] == 0, self.calls
        assert self.calls["xdfm_cin_level_fwd"] == levels and self.calls["xdfm_cin_level_bwd_x_ex"] >= levels, self.calls
        assert len(self.prep_masks) == levels and all(A and mask is None for A, mask in self.prep_masks)


def _stack(g_or_none, x, W, Bs, ls, split, dev):
    """ops.cin_stack (sum pooling) on device copies; returns (out, x leaf, weight leaves, bias leaves)"""
    from xdfm_amd import ops
    Bn, m, D = x.shape
    xg = x.detach().to(dev).requires_grad_(True)
    Wg = [w.detach().to(dev).requires_grad_(True) for w in W]
    Bg = [b.detach().to(dev).requires_grad_(True) for b in Bs]
    out = ops.cin_stack(ops.to_fm_layout(xg), Bn, D, ls, split, "sigmoid", "sum", Wg, Bg)
    return out, xg, Wg, Bg


def _stack_fn(out):
    fn = out.grad_fn
    while fn is not None and not hasattr(fn, "lean"):
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert fn is not None, "no CINStack node behind the output"
    return fn


@pytest.mark.parametrize("math", [0, F, B16], ids=["f32mfma", "f16x3", "bf16"])
@pytest.mark.parametrize("name", ["cin_sigmoid_split", "cin_sigmoid_nosplit"])
def test_cin_stack_vs_reference_golden(name, math, monkeypatch):
    """the bars of tests/test_gpu_parity.py::test_cin_layer_vs_reference_golden (m = 4: every level runs the fp32-MFMA kernels
    in all three settings)"""
    dev = _dev()
    g = load_golden(name)
    ls, split = tuple(int(v) for v in g["layer_size"]), bool(g["split_half"])
    L = len(ls)
    x = T(g["x"])
    Bn, m, D = x.shape
    watch = _Watch(monkeypatch)
    with _Options(cin_math=math):
        out, xg, Wg, Bg = _stack(g, x, [T(g["w%d" % i]) for i in range(L)], [T(g["b%d" % i]) for i in range(L)], ls, split, dev)
        fn = _stack_fn(out)
        assert fn.lean is False
        saved = fn.saved_tensors
        assert [tuple(t.shape) for t in saved[1:1 + L]] == [(H, Bn * D) for H in ls] and len(saved) == 1 + 3 * L
        close(out, g["out"], msg="out")
        (out * T(g["gout"]).to(dev)).sum().backward()
    watch.full_output_path_only(L)
    gclose(xg.grad, g["dx"], "dx")
    for i in range(L):
        gclose(Wg[i].grad, g["dw%d" % i], "dw%d" % i)
        gclose(Bg[i].grad, g["db%d" % i], "db%d" % i)


_RANDOM = {}


def _random_case():
    """m = 8, D = 16, B = 64, (34, 18): level 0 has f16x3 forward and dX kernels, level 1 (H = 18) an f16x3 / bf16 dX kernel"""
    if not _RANDOM:
        from deepctr.layers import CIN
        from oracle import xdeepfm_oracle as orc
        torch.manual_seed(64 * 7 + 8)
        layer = CIN(8, (34, 18), "sigmoid", True, 0.0, 1024, device="cpu")
        x = (torch.randn(64, 8, 16) * 0.6).requires_grad_(True)
        W = [c.weight.detach().clone().requires_grad_(True) for c in layer.conv1ds]
        Bs = [c.bias.detach().clone().requires_grad_(True) for c in layer.conv1ds]
        want = orc.cin_forward(x, W, Bs, True, "sigmoid")
        gout = torch.randn(want.shape)
        (want * gout).sum().backward()
        _RANDOM.update(x=x, W=W, Bs=Bs, want=want.detach(), gout=gout)
    return _RANDOM


@pytest.mark.parametrize("math", [0, F, B16], ids=["f32mfma", "f16x3", "bf16"])
def test_cin_stack_vs_oracle_random(math, monkeypatch):
    """fp32-MFMA and f16x3: the bars of tests/test_gpu_parity.py::test_cin_vs_oracle_random (no column is excluded: a sigmoid
    has no switch); bf16: those of test_cin_bf16_mfma_path_vs_fp32_oracle, element-wise as for its linear cases.  Then
    XDFM_CIN_LEAN=1 set explicitly: not one bit of the outputs or gradients changes."""
    from xdfm_amd import _lib
    dev = _dev()
    r = _random_case()
    ls = (34, 18)

    def run():
        out, xg, Wg, Bg = _stack(None, r["x"], r["W"], r["Bs"], ls, True, dev)
        fn = _stack_fn(out)
        assert fn.lean is False and [tuple(t.shape) for t in fn.saved_tensors[1:3]] == [(34, 1024), (18, 1024)]
        (out * r["gout"].to(dev)).sum().backward()
        return [out.detach(), xg.grad] + [w.grad for w in Wg] + [b.grad for b in Bg]

    watch = _Watch(monkeypatch)
    with _Options(cin_math=math, last_fwd_inst=-1, last_bwx_inst=-1, last_bww_inst=-1):
        got = run()
        # the last forward launch is level 1 (H = 18: fp32-MFMA), the last dX launch level 0 (H = 34), dW has H <= 64
        assert _lib.get_option("last_fwd_kernel") == 0 and _lib.get_option("last_bww_kernel") == 0
        assert _lib.get_option("last_bwx_kernel") == math and (_lib.get_option("last_bwx_inst") > 0) == (math != 0)
        watch.full_output_path_only(2)
        old = os.environ.get("XDFM_CIN_LEAN")
        os.environ["XDFM_CIN_LEAN"] = "1"
        try:
            again = run()
        finally:
            if old is None:
                del os.environ["XDFM_CIN_LEAN"]
            else:
                os.environ["XDFM_CIN_LEAN"] = old
        watch.full_output_path_only(4)
    for a, b in zip(got, again):
        assert torch.equal(a, b), "XDFM_CIN_LEAN=1 changed a sigmoid stack's result"
    want = [r["want"], r["x"].grad] + [w.grad for w in r["W"]] + [b.grad for b in r["Bs"]]
    names = ["out", "dx", "dw0", "dw1", "db0", "db1"]
    if math != B16:
        close(got[0], want[0].numpy(), msg="out")
        for n, a, w in zip(names[1:], got[1:], want[1:]):
            gclose(a, w.numpy(), n)
        return

    def rel(a, w):
        return float((a.cpu() - w).abs().max() / w.abs().max())

    def cos(a, w):
        a, w = a.cpu().double().flatten(), w.double().flatten()
        return float(a @ w / torch.sqrt((a @ a) * (w @ w)))

    assert rel(got[0], want[0]) < 2e-2
    for n, a, w in zip(names[1:], got[1:], want[1:]):
        assert cos(a, w) > 0.998 and rel(a, w) < 4e-2, (n, cos(a, w), rel(a, w))


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def _columns(vocab, nd, D):
    from deepctr.inputs import DenseFeat, SparseFeat
    return [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]


def _golden_model(g, dev, activation="sigmoid"):
    from deepctr.models import xDeepFM
    cols = _columns([int(v) for v in g["vocab"]], int(g["n_dense"]), int(g["emb_dim"]))
    return xDeepFM(cols, cols, dnn_hidden_units=tuple(int(v) for v in g["dnn"]), cin_layer_size=tuple(int(v) for v in g["cin"]),
                   l2_reg_dnn=1e-5, cin_activation=activation, device=dev)


@pytest.mark.parametrize("math", [0, F], ids=["f32mfma", "f16x3"])
def test_model_vs_reference_golden(math):
    """tests/test_gpu_parity.py::test_model_vs_reference_golden on the sigmoid golden, at its bars"""
    dev = _dev()
    g = load_golden(MODEL_GOLDEN)
    with _Options(cin_math=math):
        model = _golden_model(g, dev)
        for k, v in model.state_dict().items():
            np.testing.assert_array_equal(v.cpu().numpy(), g["init:" + k], err_msg="init " + k)
        model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
        B = int(g["B"])
        X, y = T(g["X"]).to(dev), T(g["y"]).to(dev)
        model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
        model.train()
        y_pred = model(X[:B])
        close(y_pred, g["y_pred"], rtol=2e-5, atol=1e-6, msg="y_pred")
        loss = torch.nn.functional.binary_cross_entropy(y_pred.squeeze(), y[:B].squeeze(), reduction="sum")
        reg = model.get_regularization_loss()
        assert abs(loss.item() - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
        assert abs(reg.item() - float(g["reg"])) <= 1e-5 * abs(float(g["reg"]))
        model.optim.zero_grad()
        (loss + reg).backward()
        for k, p in model.named_parameters():
            gclose(p.grad, g["g:" + k], k)
        model.optim.zero_grad()
        losses = []
        for s in range(3):
            xb, yb = X[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
            yp = model(xb).squeeze()
            model.optim.zero_grad()
            l = torch.nn.functional.binary_cross_entropy(yp, yb.squeeze(), reduction="sum")
            tot = l + model.get_regularization_loss() + model.aux_loss
            losses.append([l.item(), tot.item()])
            tot.backward()
            model.optim.step()
        np.testing.assert_allclose(np.array(losses), g["losses3"], rtol=2e-5)
        for k, v in model.state_dict().items():
            close(v, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="after 3 steps: " + k)
        names = list(model.feature_index.keys())
        Xn = g["X"]
        pred = model.predict({n: Xn[:, i] for i, n in enumerate(names)}, batch_size=B)
    assert pred.dtype == np.float64 and pred.shape == (Xn.shape[0], 1)
    from xdfm_amd import metrics as M
    assert abs(M.log_loss(g["y"], pred) - M.log_loss(g["y"], g["pred_after"])) < 1e-5
    assert abs(M.roc_auc_score(g["y"], pred) - M.roc_auc_score(g["y"], g["pred_after"])) < 1e-5


def test_attention_model_with_sigmoid_vs_oracle():
    """xDeepFMAttention at model_attn_small's size: the CIN feeds the attention block its feature maps (pool "fm").  Bars of
    the model goldens; the attention block's own parameters at the bar test_gpu_parity.py gives them (their gradients pass
    through softmax / LayerNorm cancellations)."""
    from deepctr.models import xDeepFMAttention
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    vocab, nd, D, cin, dnn, B = [7, 5, 11, 3, 9, 4], 3, 8, (8, 6), (16, 8), 16
    cols = _columns(vocab, nd, D)
    model = xDeepFMAttention(cols, cols, dnn_hidden_units=dnn, cin_layer_size=cin, l2_reg_dnn=1e-5, cin_num_heads=4,
                             cin_activation="sigmoid", device=dev)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k or k == "linear_model.weight" or "dnn" in k or k == "cin_linear.weight":
                p.copy_((0.3 * torch.randn(p.shape, generator=gen)).to(dev))
    state = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    X, y = orc.synthetic_batch(B, vocab, nd, seed=2025)
    spec = orc.Spec(["C%d" % (i + 1) for i in range(len(vocab))], vocab, ["I%d" % (i + 1) for i in range(nd)], D, cin, True, "sigmoid",
                    dnn, "attn", 4, True, True, 1, l2_reg_dnn=1e-5)
    tot, dl, yp = orc.total_loss(T(X), T(y), state, spec)
    tot.backward()
    model.train()
    y_pred = model(T(X).to(dev))
    close(y_pred.squeeze(), yp.detach().numpy().squeeze(), rtol=2e-5, atol=1e-6, msg="y_pred")
    loss = torch.nn.functional.binary_cross_entropy(y_pred.squeeze(), T(y).to(dev).squeeze(), reduction="sum")
    assert abs(loss.item() - dl.item()) <= 2e-5 * abs(dl.item())
    (loss + model.get_regularization_loss()).backward()
    for k, p in model.named_parameters():
        want = state[k].grad.numpy()
        if k.startswith("cin.") and "conv1ds" not in k:
            close(p.grad, want, rtol=2e-3, atol=1e-2 * float(np.abs(want).max()) + 1e-9, msg=k)
        else:
            gclose(p.grad, want, k)


def test_train_step_replayed_from_the_graph_equals_the_eager_twin():
    from xdfm_amd import graphstep
    if os.environ.get("XDFM_HIP_GRAPH", "1") == "0":
        pytest.skip("XDFM_HIP_GRAPH=0")
    dev = _dev()
    g = load_golden(MODEL_GOLDEN)
    X, y = T(g["X"]).to(dev), T(g["y"]).to(dev)
    B = int(g["B"])

    def run(use_graph):
        model = _golden_model(g, dev)
        model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
        model.compile("adam", "binary_crossentropy", metrics=[])
        model.train()
        step = graphstep.GraphedStep(model)
        step.disabled = not use_graph
        model.__dict__["_graphed_step"] = step
        for s in range(5):
            k = s % 3
            model.train_on_batch(X[k * B:(k + 1) * B], y[k * B:(k + 1) * B])
        torch.cuda.synchronize()
        return model, step

    m_g, st_g = run(True)
    m_e, st_e = run(False)
    assert st_g.replays == 3 and not st_g.disabled and st_e.replays == 0
    for (k, a), (_, b) in zip(m_g.state_dict().items(), m_e.state_dict().items()):
        assert torch.equal(a, b), k
    assert not torch.equal(m_g.state_dict()["cin.conv1ds.0.weight"].cpu(), T(g["s0:cin.conv1ds.0.weight"]))


def test_relu_model_after_a_sigmoid_one_still_runs_the_lean_kernels(monkeypatch):
    """no state leaks from a sigmoid stack: a relu CIN of the bench's field count built afterwards takes the lean forward and the
    dX kernel that forms dOut from the sign bits, with the f16x3 kernels in all three directions"""
    from deepctr.layers import CIN
    from xdfm_amd import _lib
    dev = _dev()
    torch.manual_seed(3)
    x = torch.randn(8, 26, 16, device=dev) * 0.5
    with _Options(cin_math=F, last_fwd_inst=-1, last_bwx_inst=-1, last_bww_inst=-1):
        probes = {}
        for act in ("sigmoid", "relu"):
            watch = _Watch(monkeypatch)
            layer = CIN(26, (96, 72), act, True, 0.0, 1024, device=dev)
            xg = x.clone().requires_grad_(True)
            out = layer(xg)
            fn = _stack_fn(out)
            out.sum().backward()
            probes[act] = (fn.lean, dict(watch.calls), [mask is not None for _, mask in watch.prep_masks],
                           tuple(_lib.get_option(k) for k in ("last_fwd_kernel", "last_bwx_kernel", "last_bww_kernel")))
            monkeypatch.undo()
    assert probes["sigmoid"][0] is False and probes["sigmoid"][2] == [False, False]
    assert probes["sigmoid"][1]["xdfm_cin_level_fwd_ex"] == 0 and probes["sigmoid"][1]["xdfm_cin_level_bwd_x_src"] == 0
    lean, calls, masks, kernels = probes["relu"]
    assert lean is True and masks == [True, True] and kernels == (1, 1, 1)
    assert calls["xdfm_cin_level_fwd_ex"] == 2 and calls["xdfm_cin_level_fwd"] == 0
    assert calls["xdfm_cin_level_bwd_x_src"] == 2 and calls["xdfm_cin_level_bwd_x_ex"] == 0
