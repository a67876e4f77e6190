"""CPU: the float64 references of tests/head_reg_ref.py against torch's float64 autograd, the stock fp32 composition
against the bars the GPU suite (test_gpu_head_reg.py) holds the kernels to, and the argument checks of the head, column
sum and L2 entry points that return before any launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_reg_ref as R


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# references against float64 autograd (non-saturating inputs: the staged definition and the plain one coincide)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1111", "c0110", "c1001", "k3_k4_b16", "k4_k68_b2047", "k200_k512_b4099"])
def test_head_reference_matches_float64_autograd(name):
    c = R.make_head_case(name)
    B = c["B"]
    td = lambda a: None if a is None else torch.from_numpy(a).double().requires_grad_(True)
    lin, u, wu, v, wv, bias = (td(c[k]) for k in ("lin", "u", "wu", "v", "wv", "bias"))
    y = torch.from_numpy(c["y"]).double()
    z = torch.zeros(B, dtype=torch.float64)
    if lin is not None:
        z = z + lin
    if u is not None:
        z = z + F.linear(u, wu).reshape(-1)
    if v is not None:
        z = z + F.linear(v, wv).reshape(-1)
    if bias is not None:
        z = z + bias
    pred = torch.sigmoid(z)
    loss = F.binary_cross_entropy(pred, y, reduction="sum")
    gl = float(c["gloss"])
    (gl * loss).backward()

    p64, _ = R.head_pred_ref(c["lin"], c["u"], c["wu"], c["v"], c["wv"], c["bias"], B)
    assert _rel(p64, pred.detach().numpy()) <= 1e-12
    # the second stage is defined on an fp32 pred; fed the float64 one it must be the plain BCE (float64 passes through f64())
    l64, _, _ = R.head_loss_ref(pred.detach().numpy(), c["y"])
    assert abs(l64 - loss.item()) <= 1e-12 * abs(loss.item())
    g = R.head_g_ref(pred.detach().numpy(), c["y"], c["gloss"])
    grads = R.head_grads_ref(g, c["u"], c["wu"], c["v"], c["wv"])
    want = {}
    if bias is not None:
        want["dbias"] = bias.grad.numpy().reshape(())
    if lin is not None:
        assert _rel(g, lin.grad.numpy()) <= 1e-12
        want.setdefault("dbias", lin.grad.numpy().sum())        # no bias: the bias column of the gradient row is sum_b g_b
    if u is not None:
        want["du"], want["dwu"] = u.grad.numpy(), wu.grad.numpy().reshape(-1)
    if v is not None:
        want["dv"], want["dwv"] = v.grad.numpy(), wv.grad.numpy().reshape(-1)
    for k, w in want.items():
        assert _rel(grads[k][0], w) <= 1e-12, k


@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (1000, 429)])
def test_colsum_references_match_float64_autograd(rows, cols):
    g32, y32 = R.make_colsum_case(rows, cols, relu=True)
    g32, y32 = np.ascontiguousarray(g32[:, :cols]), np.ascontiguousarray(y32[:, :cols])
    # plain: d/dx of sum(x * g) summed over rows is g.sum(0)
    s, _, _ = R.colsum_ref(g32)
    assert _rel(s, torch.from_numpy(g32).double().sum(0).numpy()) <= 1e-12
    # ReLU variant: the gradient torch.relu passes back, and its column sum (the bias gradient of relu(x + b))
    x = torch.from_numpy(y32).double().requires_grad_(True)
    b = torch.zeros(cols, dtype=torch.float64, requires_grad=True)
    out = torch.relu(x + b)
    out.backward(torch.from_numpy(g32).double())
    s, _, gz = R.colsum_ref(g32, out.detach().numpy())
    assert np.array_equal(gz.astype(np.float64), x.grad.numpy())
    if rows * cols >= 1000:      # the drawn y really carries the three kinds of non-positive entries
        assert (y32 == 0).any() and np.signbit(y32[y32 == 0]).any() and (~np.signbit(y32[y32 == 0])).any() and (y32 < 0).any()
    assert _rel(s, b.grad.numpy()) <= 1e-12


def test_l2_reference_matches_float64_autograd():
    c = R.l2_case("t257")
    ws = [torch.from_numpy(w).double().requires_grad_(True) for w in c["ws"]]
    val = sum(float(k) * (w * w).sum() for k, w in zip(c["coeffs"], ws))
    (float(c["gs"]) * val).backward()
    v64, bound, walk = R.l2_value_ref(c["ws"], c["coeffs"])
    assert abs(v64 - val.item()) <= 1e-12 * abs(val.item()) and 0 < walk < bound
    for w32, k, w in zip(c["ws"], c["coeffs"], ws):
        g32, _ = R.l2_grad_ref(w32, k, c["gs"])
        # the fp32 spelling has two roundings: within 1 ulp of the float64 gradient
        assert (np.abs(g32.astype(np.float64) - w.grad.numpy()) <= R.ulp_bound(w.grad.numpy(), 1.0)).all()
    assert c["coeffs"][-1] == 0 and c["coeffs"][0] != 0 and not c["ws"][c["T"] // 2].any()
    for name in [k[0] for k in R.L2_CASES]:
        cc = R.l2_case(name)
        assert len(cc["ws"]) == cc["T"] and set(cc["offs"]) <= {0, 1, 2, 3}
        assert cc["coeffs"][0] != 0 and cc["ws"][0].any()
    # what the list is there for: T, the sizes around the stride, every base offset, and float4 walks (tensor and gradient
    # slot both 16-byte aligned) of many strides with a scalar tail in l2_sumsq_kernel and l2_grad_kernel
    cases = [R.l2_case(k[0]) for k in R.L2_CASES]
    assert {cc["T"] for cc in cases} == {1, 2, 256, 257, 1000}
    assert {n for cc in cases for n in cc["sizes"]} >= {1, 3, 4, 5, R.L2_STRIDE - 1, R.L2_STRIDE + 1, 2 ** 22 + 3}
    assert {o for cc in cases for o in cc["offs"]} == {0, 1, 2, 3}
    vec_strides, scalar_big = 0, 0
    for cc in cases:
        goff = np.concatenate([[0], np.cumsum(cc["sizes"])[:-1]])
        for n, o, go in zip(cc["sizes"], cc["offs"], goff):
            if o == 0 and go % 4 == 0 and n % 4:
                vec_strides = max(vec_strides, (n // 4) // (R.L2_GRAD_STRIDE // 4))
            if o != 0 and go % 4 != 0:
                scalar_big = max(scalar_big, n)
    assert vec_strides >= 32 and scalar_big >= 2 ** 21


# ---------------------------------------------------------------------------------------------------------------------
# the stock fp32 composition against the GPU suite's bars
# ---------------------------------------------------------------------------------------------------------------------
def _stock_fp32(c):
    """F.linear + sigmoid + F.binary_cross_entropy(reduction='sum') in float32 on the CPU, with autograd."""
    B = c["B"]
    tf = lambda a: None if a is None else torch.from_numpy(a).clone().requires_grad_(True)
    lin, u, wu, v, wv, bias = (tf(c[k]) for k in ("lin", "u", "wu", "v", "wv", "bias"))
    z = torch.zeros(B, dtype=torch.float32)
    if lin is not None:
        z = z + lin
    if u is not None:
        z = z + F.linear(u, wu).reshape(-1)
    if v is not None:
        z = z + F.linear(v, wv).reshape(-1)
    if bias is not None:
        z = z + bias
    z = z.clone().requires_grad_(True) if not z.requires_grad else z
    z.retain_grad()
    pred = torch.sigmoid(z)
    loss = F.binary_cross_entropy(pred, torch.from_numpy(c["y"]), reduction="sum")
    (torch.tensor(float(c["gloss"])) * loss).backward()
    g = lambda t: None if t is None else t.grad.numpy()
    return dict(pred=pred.detach().numpy(), loss=float(loss.detach()), g=z.grad.numpy(), du=g(u), dv=g(v), dwu=g(wu), dwv=g(wv),
                dbias=g(bias))


WORST = {}


@pytest.mark.parametrize("name", R.head_case_names())
def test_stock_fp32_head_stays_inside_the_gpu_bars(name):
    c = R.make_head_case(name)
    s = _stock_fp32(c)
    p64, pb = R.head_pred_ref(c["lin"], c["u"], c["wu"], c["v"], c["wv"], c["bias"], c["B"])
    frac = {"pred": float((np.abs(s["pred"] - p64) / pb).max())}
    l64, lb, terms = R.head_loss_ref(s["pred"], c["y"])
    frac["loss"] = abs(s["loss"] - l64) / lb
    grads = R.head_grads_ref(s["g"], c["u"], c["wu"], c["v"], c["wv"])
    for k, (ref, bound) in grads.items():
        if s.get(k) is None:
            continue
        got = s[k].reshape(np.shape(ref)).astype(np.float64)
        frac[k] = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    for k, f in frac.items():
        WORST[k] = max(WORST.get(k, 0.0), f)
    print("stock fp32 %-18s " % name + " ".join("%s %.3g" % kv for kv in sorted(frac.items())))
    assert all(f <= 1.0 for f in frac.values()), frac
    if c["labels"] == "sat":
        # the case is what it claims: rows saturated on either side, for either label
        p, y = s["pred"], c["y"]
        for side in (0.0, 1.0):
            for lab in (0.0, 1.0):
                assert ((p == side) & (y == lab)).any(), (side, lab)
        assert (terms == 100.0).any()                          # p == 0 under label 1, or p == 1 under label 0
        assert (R.head_g_ref(p, y, c["gloss"])[(p == 0) | (p == 1)] == 0).all()
        z64 = R.head_logits(c["lin"], c["u"], c["wu"], c["v"], c["wv"], c["bias"])[0]
        assert (z64 < -20).sum() > 8 and (z64 > 20).sum() > 8


def test_head_case_list_covers_what_the_docstring_table_says():
    names = R.head_case_names()
    assert len(set(names)) == len(names)
    cases = {c[0]: c for c in R.HEAD_CASES}
    combos = {(c[2] > 0, c[3] > 0, c[4], c[5]) for c in R.HEAD_CASES}
    assert len(combos) == 16
    ks = {k for c in R.HEAD_CASES for k in (c[2], c[3]) if k}
    assert {1, 3, 4, 60, 64, 68, 200, 512, 516, 1000} <= ks
    assert {c[1] for c in R.HEAD_CASES} >= {1, 15, 16, 17, 2047, 2048, 2049, 4099, 65536}
    assert any(c[2] + c[3] == 4095 for c in R.HEAD_CASES)
    assert {c[6] for c in R.HEAD_CASES} == {"hard", "soft", "sat"}
    vec = {R.head_vectorised(c[2], c[3], c[7]) for c in R.HEAD_CASES}
    assert vec == {True, False}
    for lab in ("sat",):
        assert {R.head_vectorised(c[2], c[3], c[7]) for c in R.HEAD_CASES if c[6] == lab} == {True, False}
    assert not R.head_vectorised(*[cases["k64_k64_u_off"][i] for i in (2, 3, 7)])
    assert {c[1] for c in R.HEAD_CASES if R.head_vectorised(c[2], c[3], c[7])} >= {1, 2047, 2048, 4099, 65536}
    assert sum(1 for i in range(len(names)) if R.HEAD_GLOSS[i % 4] != 1.0) > len(names) // 2


# ---------------------------------------------------------------------------------------------------------------------
# argument checks that return before any launch (no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    from xdfm_amd import _lib
    return _lib.load()


def _bad(rc, lib, text):
    assert rc == 1 and text in lib.xdfm_last_error(), (rc, lib.xdfm_last_error())


def test_head_argument_checks():
    lib = _lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)          # a host address: never dereferenced, the checks return first
    # forward: lin, u, wu, Ku, v, wv, Kv, bias, y, B, pred, loss, ws, stream
    _bad(lib.xdfm_head_fwd(None, None, None, 0, None, None, 0, None, None, 4, p, p, p, None), lib, b"head_fwd: bad arguments")
    _bad(lib.xdfm_head_fwd(None, None, None, 0, None, None, 0, None, p, 4, None, p, p, None), lib, b"head_fwd: bad arguments")
    _bad(lib.xdfm_head_fwd(None, None, None, 0, None, None, 0, None, p, 4, p, None, p, None), lib, b"head_fwd: bad arguments")
    _bad(lib.xdfm_head_fwd(None, None, None, 0, None, None, 0, None, p, 4, p, p, None, None), lib, b"head_fwd: bad arguments")
    _bad(lib.xdfm_head_fwd(None, None, None, 0, None, None, 0, None, p, 0, p, p, p, None), lib, b"head_fwd: bad arguments")
    _bad(lib.xdfm_head_fwd(None, None, None, 0, None, None, 0, None, p, -3, p, p, p, None), lib, b"head_fwd: bad arguments")
    _bad(lib.xdfm_head_fwd(None, p, None, 4, None, None, 0, None, p, 4, p, p, p, None), lib, b"head_fwd: bad operand shapes")    # u without wu
    _bad(lib.xdfm_head_fwd(None, p, p, 0, None, None, 0, None, p, 4, p, p, p, None), lib, b"head_fwd: bad operand shapes")       # u with Ku = 0
    _bad(lib.xdfm_head_fwd(None, None, None, 0, p, None, 4, None, p, 4, p, p, p, None), lib, b"head_fwd: bad operand shapes")    # v without wv
    _bad(lib.xdfm_head_fwd(None, None, None, -1, None, None, 0, None, p, 4, p, p, p, None), lib, b"head_fwd: bad operand shapes")
    # backward: pred, y, gloss, u, wu, Ku, v, wv, Kv, B, dlin, du, dv, grads, ws, stream
    ok = [p, p, p, None, None, 0, None, None, 0, 4, None, None, None, p, p, None]
    for i in (0, 1, 2, 13, 14):
        a = list(ok)
        a[i] = None
        _bad(lib.xdfm_head_bwd(*a), lib, b"head_bwd: bad arguments")
    for B in (0, -1):
        a = list(ok)
        a[9] = B
        _bad(lib.xdfm_head_bwd(*a), lib, b"head_bwd: bad arguments")
    _bad(lib.xdfm_head_bwd(p, p, p, p, p, 4, None, None, 0, 4, None, None, None, p, p, None), lib, b"head_bwd: bad operand shapes")   # u without du
    _bad(lib.xdfm_head_bwd(p, p, p, None, None, 0, p, None, 4, 4, None, None, p, p, p, None), lib, b"head_bwd: bad operand shapes")   # v without wv
    # 4 waves * (Ku + Kv + 1) floats of LDS: 4095 is the last sum that fits 64 KiB, 4096 must be refused before the launch
    _bad(lib.xdfm_head_bwd(p, p, p, p, p, 4000, p, p, 96, 4, None, p, p, p, p, None), lib, b"too large")
    _bad(lib.xdfm_head_bwd(p, p, p, p, p, 4096, None, None, 0, 4, None, p, None, p, p, None), lib, b"too large")
    for Ku, Kv in ((0, 0), (1, 0), (64, 60), (4000, 95)):
        assert lib.xdfm_head_ws_elems(Ku, Kv) == 128 * (Ku + Kv + 1) + 128         # HEAD_BLOCKS rows of partials + the loss partials


def test_l2_argument_checks():
    lib = _lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # forward: ptrs, numel, coeff, T, partials, out, stream
    ok = [p, p, p, 3, p, p, None]
    for i in (0, 1, 2, 4, 5):
        a = list(ok)
        a[i] = None
        _bad(lib.xdfm_l2_reg_fwd(*a), lib, b"l2_reg_fwd: null pointer")
    for T in (0, -1, 65536, 1 << 20):
        a = list(ok)
        a[3] = T
        _bad(lib.xdfm_l2_reg_fwd(*a), lib, b"l2_reg_fwd: T=")
    # backward: ptrs, numel, coeff, T, gscale, gflat, goff, accumulate, stream
    ok = [p, p, p, 3, p, p, p, 0, None]
    for i in (0, 1, 2, 4, 5, 6):
        a = list(ok)
        a[i] = None
        _bad(lib.xdfm_l2_reg_bwd(*a), lib, b"l2_reg_bwd: null pointer")
    for T in (0, -1, 65536):
        a = list(ok)
        a[3] = T
        _bad(lib.xdfm_l2_reg_bwd(*a), lib, b"l2_reg_bwd: T=")


def test_colsum_argument_checks():
    lib = _lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # g, rows, cols, ld, ws, out, stream
    ok = [p, 4, 4, 4, p, p, None]
    for i in (0, 4, 5):
        a = list(ok)
        a[i] = None
        _bad(lib.xdfm_colsum(*a), lib, b"colsum: null pointer")
    for i, val in ((1, 0), (1, -5), (2, 0), (2, -1), (3, 3), (3, 0)):       # rows <= 0, cols <= 0, ld < cols
        a = list(ok)
        a[i] = val
        _bad(lib.xdfm_colsum(*a), lib, b"colsum: bad shape")
    # g, y, rows, cols, ldg, ldy, ws, gz, out, stream
    ok = [p, p, 4, 4, 4, 4, p, p, p, None]
    for i in (0, 1, 6, 7, 8):
        a = list(ok)
        a[i] = None
        _bad(lib.xdfm_relu_bwd_colsum(*a), lib, b"relu_bwd_colsum: null pointer")
    for i, val in ((2, 0), (2, -1), (3, 0), (4, 3), (5, 3)):                # rows <= 0, cols <= 0, ldg < cols, ldy < cols
        a = list(ok)
        a[i] = val
        _bad(lib.xdfm_relu_bwd_colsum(*a), lib, b"relu_bwd_colsum: bad shape")
    for cols, want in ((-1, 0), (0, 0), (1, 64), (63, 64 * 63), (429, 64 * 429), (65600, 64 * 65600)):
        assert lib.xdfm_colsum_ws_elems(cols) == want                       # CS_ROWBLK partial rows of `cols` floats
