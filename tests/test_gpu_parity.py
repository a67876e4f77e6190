"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against
(a) the golden vectors produced by the real reference and (b) the CPU oracle on seeded inputs.

Tolerances (fp32 everywhere): forward values rtol 2e-5 / atol 2e-6 -- the MFMA contraction sums
K = Hp*m products in a different order than ATen; gradients rtol 2e-4 with an absolute floor of
2e-5 x max|expected| (dW sums B*D = thousands of terms in a different order than ATen).
"""
import os

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy



def _needs_default_env(feature):
    """Tests that assert a feature is ACTIVE skip when the environment switches it off (XDFM_GRAD_ARENA=0 / XDFM_HIP_GRAPH=0 /
    XDFM_ADAM_DEFERRED=0 are supported ways to run the product; the rest of the suite passes under them)."""
    import os
    env = {"arena": "XDFM_GRAD_ARENA", "graph": "XDFM_HIP_GRAPH", "deferred": "XDFM_ADAM_DEFERRED"}[feature]
    if os.environ.get(env, "1") == "0":
        pytest.skip("%s=0" % env)

def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close(got, want, rtol=2e-5, atol=2e-6, msg=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


def gclose(got, want, msg=""):
    want = np.asarray(want)
    close(got, want, rtol=2e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-9, msg=msg)


def _f16x3_kernels_for(m, ls, B, D):
    """Which arithmetic each CIN kernel of a (m, layer sizes) stack must have run in cin_math 1: the f16x3 forward exists
    for every even m in 8..40 (instances per field count) and H > 32, dX for 16 < H <= 256 (per call), dW for H > 64 with 16-byte rows (N % 4 == 0);
    everything else falls back to the fp32-MFMA kernels -- by design, and the tests say which (no test
    asserted which kernel ran).  Returns the expected probe values of the LAST level for (fwd, bwx of level 0, bww of level 0)."""
    H_last, H0 = ls[-1], ls[0]
    N = B * D
    fwd = 1 if (m % 2 == 0 and 8 <= m <= 40 and H_last > 32) else 0
    last_call = H0 if H0 <= 256 else (H0 % 256 or 256)     # dX walks H in calls of <= 256 rows; the probe sees the last one
    bwx = 1 if last_call > 16 else 0
    bww = 1 if (H0 > 64 and N % 4 == 0 and N >= 32) else 0
    return fwd, bwx, bww


@pytest.fixture(params=[0, 1], ids=["f32mfma", "f16x3"])
def cin_math(request):
    """Both arithmetic modes of the CIN contraction: v_mfma_f32_32x32x2_f32 on fp32 operands, and the
    f16x3 split (fp32 = hi + lo fp16, three v_mfma_f32_32x32x16_f16 per product, fp32 accumulate)."""
    from xdfm_amd import _lib
    old = _lib.get_option("cin_math")
    _lib.set_option("cin_math", request.param)
    yield request.param
    _lib.set_option("cin_math", old)


# --------------------------------------------------------------------------------------------- #
def test_native_library_is_loaded():
    from xdfm_amd import _lib
    lib = _lib.load()
    assert lib.xdfm_abi_version() == _lib.ABI_VERSION == 9
    assert lib.xdfm_device_count() >= 1
    with open("/proc/self/maps") as f:
        assert "libxdfm_hip.so" in f.read()


@pytest.mark.parametrize("name", golden_names("cin_"))
def test_cin_layer_vs_reference_golden(name, cin_math):
    from deepctr.layers import CIN
    dev = _dev()
    g = load_golden(name)
    ls = tuple(int(v) for v in g["layer_size"])
    B, m, D = g["x"].shape
    layer = CIN(m, ls, str(g["activation"]), bool(g["split_half"]), 0.0, 1024, device=dev)
    with torch.no_grad():
        for i, c in enumerate(layer.conv1ds):
            c.weight.copy_(T(g["w%d" % i]))
            c.bias.copy_(T(g["b%d" % i]))
    x = T(g["x"]).to(dev).requires_grad_(True)
    import warnings
    from xdfm_amd import _lib, ops
    ops._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = layer(x)
        close(out, g["out"], msg="out")
        (out * T(g["gout"]).to(dev)).sum().backward()
    gclose(x.grad, g["dx"], "dx")
    for i, c in enumerate(layer.conv1ds):
        gclose(c.weight.grad, g["dw%d" % i], "dw%d" % i)
        gclose(c.bias.grad, g["db%d" % i], "db%d" % i)
    if name.startswith("cin_x3_") and cin_math == 1:
        # these goldens exist to pin the DEFAULT arithmetic's own kernels to the reference: no level may have fallen back
        assert not [w for w in caught if "fp32-MFMA arithmetic" in str(w.message)], [str(w.message) for w in caught]
        assert _lib.get_option("last_fwd_kernel") == _lib.get_option("last_bwx_kernel") == _lib.get_option("last_bww_kernel") == 1
        assert _lib.get_option("last_sym") & 6 == 6      # level 0 (the last dX and dW launches) ran the folded kernels


@pytest.mark.parametrize("B,m,D,ls", [(130, 26, 16, (64, 32, 32)), (37, 7, 10, (40, 24)), (257, 26, 8, (128, 128)),
                                       (70, 5, 32, (24, 10, 6)), (33, 26, 16, (256,)), (45, 22, 32, (136, 96)),
                                       (19, 25, 4, (200, 66)),
                                       (1, 26, 16, (256, 128, 128)),             # one example (last batch of an epoch)
                                       (6, 22, 32, (512, 256, 256, 128)),        # BASELINE config-5 layer sizes (H > 256)
                                       (3, 3, 4, (300, 4)),
                                       (5, 26, 10, (64, 32)),                    # f16x3 forward with N = 50: one partial wave
                                       (2, 22, 6, (40,)),                        # N = 12 < 32, odd number of column quads
                                       (9, 26, 12, (96, 34, 20)),                # Hp = 48, 17: ragged 8-row blocks
                                       # field counts other than BASELINE's 22 / 26: every even m <= 40 has f16x3 forward instances
                                       (64, 10, 16, (64, 48)), (50, 40, 8, (72, 40)), (33, 12, 16, (128, 64)), (13, 8, 16, (128, 64)),
                                       (12, 32, 8, (256, 40)), (17, 18, 12, (260, 48)), (21, 14, 8, (80, 36)),
                                       (11, 42, 8, (48, 40))])                   # m = 42 > 40: fp32 forward (and a warning)
def test_cin_vs_oracle_random(B, m, D, ls, cin_math):
    from deepctr.layers import CIN
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    torch.manual_seed(B * 7 + m)
    layer = CIN(m, ls, "relu", True, 0.0, 1024, device="cpu")
    x = (torch.randn(B, m, D) * 0.6).requires_grad_(True)
    W = [c.weight.detach().clone().requires_grad_(True) for c in layer.conv1ds]
    Bs = [c.bias.detach().clone().requires_grad_(True) for c in layer.conv1ds]
    want = orc.cin_forward(x, W, Bs, True, "relu")
    gout = torch.randn(want.shape)
    (want * gout).sum().backward()
    layer = layer.to(dev)
    xg = x.detach().to(dev).requires_grad_(True)
    import warnings
    from xdfm_amd import _lib, ops
    ops._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = layer(xg)
    # a level without an f16x3 forward kernel is announced (once per shape), never silent
    fell_back = [w for w in caught if "fp32-MFMA arithmetic" in str(w.message)]
    expect_fallback = cin_math == 1 and any(
        not (m % 2 == 0 and 8 <= m <= 40 and H > 32) for H in ls)
    assert bool(fell_back) == expect_fallback, [str(w.message) for w in caught]
    close(out, want.detach().numpy(), msg="out")
    (out * gout.to(dev)).sum().backward()
    if cin_math == 1:              # which kernels ran: the last forward launch is the last level, the last backward launches level 0
        fwd, bwx, bww = _f16x3_kernels_for(m, ls, B, D)
        assert (_lib.get_option("last_fwd_kernel"), _lib.get_option("last_bwx_kernel"), _lib.get_option("last_bww_kernel")) == \
            (fwd, bwx, bww), "unexpected kernel arithmetic for m=%d layers=%s" % (m, ls)
    else:
        assert _lib.get_option("last_fwd_kernel") == _lib.get_option("last_bwx_kernel") == _lib.get_option("last_bww_kernel") == 0
    # A ReLU whose pre-activation is within rounding of zero can switch on one side only; its whole
    # (example, d) column of dx then differs legitimately.  Such columns are excluded (and must be rare).
    risky = _near_zero_preactivation_columns(x.detach(), [w.detach() for w in W], [b.detach() for b in Bs], 4e-6)
    keep = ~risky                                                  # [B, D]
    assert risky.float().mean() < 0.1
    got_dx, want_dx = xg.grad.cpu(), x.grad
    sel = keep[:, None, :].expand_as(want_dx)
    gclose(got_dx[sel], want_dx[sel].numpy(), "dx")
    if not bool(risky.any()):
        for i, c in enumerate(layer.conv1ds):
            gclose(c.weight.grad, W[i].grad.numpy(), "dw%d" % i)
            gclose(c.bias.grad, Bs[i].grad.numpy(), "db%d" % i)


@pytest.mark.parametrize("math", [1, 2])
@pytest.mark.parametrize("H,m,N", [(256, 26, 4096 + 48), (200, 22, 1000), (40, 26, 260)])
def test_cin_level0_folded_contraction_matches_full_grid(H, m, N, math):
    """Level 0 of the CIN multiplies x0 with itself (deepctr/layers/interaction.py:218-224 with hidden_nn_layers[-1] is
    x0), so Z[(i, j)] == Z[(j, i)] and the f16x3 / bf16 kernels contract over the pairs i <= j with the folded weights
    W(i, j) + W(j, i) (option x3_sym, default on; field counts 22 and 26).  Through the C ABI, against the fp64
    contraction: forward, dX (set and accumulate), dW; the folded kernels must have run (probe last_sym), must be at
    least as close to fp64 as the full-grid kernels within a factor 1.5, and dW must be exactly symmetric."""
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(H + m)
    W = torch.randn(H, m * m, device=dev) * 0.05
    x0 = torch.randn(m, N, device=dev)
    bias = torch.randn(H, device=dev) * 0.1
    dOut = torch.randn(H, N, device=dev)
    xd = x0.double().requires_grad_(True)
    Z = (xd[:, None, :] * xd[None, :, :]).reshape(m * m, N)
    pre = W.double() @ Z + bias.double()[:, None]
    (pre * dOut.double()).sum().backward()
    want_out, want_g, want_w = torch.relu(pre.detach()), xd.grad, dOut.double() @ Z.detach().t()
    old_math, old_sym = _lib.get_option("cin_math"), _lib.get_option("x3_sym")
    errs = {}
    try:
        _lib.set_option("cin_math", math)
        for sym in (0, 1):
            _lib.set_option("x3_sym", sym)
            _lib.set_option("last_sym", 0)
            pack = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, m, m), dtype=torch.float32, device=dev)
            _lib.check(lib.xdfm_cin_fwd_pack(W.data_ptr(), H, m, m, pack.data_ptr(), st), "pack")
            out = torch.zeros(H, N, device=dev)
            _lib.check(lib.xdfm_cin_level_fwd(x0.data_ptr(), x0.data_ptr(), pack.data_ptr(), bias.data_ptr(), H, m, m, N, 1,
                                              out.data_ptr(), st), "fwd")
            used = _lib.get_option("last_fwd_kernel") == math
            wz = torch.empty(lib.xdfm_cin_bwd_pack_elems(H, m, m), dtype=torch.float32, device=dev)
            _lib.check(lib.xdfm_cin_bwd_pack(W.data_ptr(), H, m, m, wz.data_ptr(), st), "bwd pack")
            dxp, dx0 = torch.full((m, N), 3.0, device=dev), torch.full((m, N), 5.0, device=dev)
            _lib.check(lib.xdfm_cin_level_bwd_x_ex(dOut.data_ptr(), x0.data_ptr(), x0.data_ptr(), wz.data_ptr(), H, m, m, N,
                                                   dxp.data_ptr(), dx0.data_ptr(), 3, st), "bwd_x")
            g1 = (dxp + dx0).double()
            _lib.check(lib.xdfm_cin_level_bwd_x_ex(dOut.data_ptr(), x0.data_ptr(), x0.data_ptr(), wz.data_ptr(), H, m, m, N,
                                                   dxp.data_ptr(), dx0.data_ptr(), 0, st), "bwd_x")
            g2 = (dxp + dx0).double()
            ws = torch.empty(lib.xdfm_cin_bwd_w_ws_elems(H, m, m, N), dtype=torch.float32, device=dev)
            dW = torch.full((H, m * m), 7.0, device=dev)
            _lib.check(lib.xdfm_cin_level_bwd_w(dOut.data_ptr(), x0.data_ptr(), x0.data_ptr(), H, m, m, N, ws.data_ptr(),
                                                dW.data_ptr(), st), "bwd_w")
            if _lib.get_option("last_fwd_kernel") != math or _lib.get_option("last_bwx_kernel") != math:
                pytest.skip("no f16x3 / bf16 kernel for this shape")          # (bf16 needs H > 64)
            x3_dw = _lib.get_option("last_bww_kernel") == math
            assert used
            assert _lib.get_option("last_sym") == ((3 | (4 if x3_dw else 0)) if sym else 0)

            def rel(got, want):
                return float((got.double() - want).abs().max() / want.abs().max())
            errs[sym] = (rel(out, want_out), rel(g1, want_g), rel(g2, 2 * want_g), rel(dW, want_w))
            if sym and x3_dw:
                d3 = dW.view(H, m, m)
                assert torch.equal(d3, d3.transpose(1, 2))
    finally:
        _lib.set_option("cin_math", old_math)
        _lib.set_option("x3_sym", old_sym)
    tol = 2e-6 if math == 1 else 1e-2
    for a, b in zip(errs[1], errs[0]):
        assert a < tol and a < 1.5 * b + 1e-7, (errs[1], errs[0])


@pytest.mark.parametrize("B,m,D,ls,act", [
    (96, 22, 32, (512, 256, 256, 128), "linear"),      # BASELINE config 5 layer sizes (Avazu shape), gradients checked
    (96, 22, 32, (512, 256, 256, 128), "relu"),
    (130, 26, 16, (256, 128, 128), "linear"),          # config 2 layer sizes
    (64, 26, 16, (256, 128, 128), "relu"),
])
def test_cin_bf16_mfma_path_vs_fp32_oracle(B, m, D, ls, act):
    """cin_math = 2 (BASELINE config 5, "bf16 MFMA path"): operands rounded to bf16 (RNE), ONE v_mfma_f32_32x32x16_bf16
    per product, fp32 accumulation, fp32 results; no range fitting (bf16 has fp32's exponent).  Tolerance of this
    arithmetic, stated here: every product carries two 2^-9 roundings, so outputs and gradients are compared with the
    fp32 oracle (deepctr/layers/interaction.py:218-246 on the CPU) to 2e-2 / 4e-2 of the tensor's largest magnitude
    (measured: 3e-3 / 8e-3), three orders looser than the 1e-5-grade fp32 modes -- SURVEY 7-3 expects 7e-4..3e-3 on the
    CIN output.  With ReLU a pre-activation within that error of zero may switch on one side only, so the gradients
    of the ReLU cases are compared by direction (cosine > 0.998; measured 0.9989 .. 0.9998, the low end on the four-level
    stack, whichever way level 0 is contracted: tools/level0_sym.py math=2 gives the same 2.3e-3 rms output error for the
    folded and the full contraction) and the element-wise check uses the linear cases."""
    from deepctr.layers import CIN
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import _lib
    dev = _dev()
    old = _lib.get_option("cin_math")
    _lib.set_option("cin_math", 2)
    try:
        torch.manual_seed(B + m)
        layer = CIN(m, ls, act, True, 0.0, 1024, device="cpu")
        x = (torch.randn(B, m, D) * 0.5).requires_grad_(True)
        W = [c.weight.detach().clone().requires_grad_(True) for c in layer.conv1ds]
        Bs = [c.bias.detach().clone().requires_grad_(True) for c in layer.conv1ds]
        want = orc.cin_forward(x, W, Bs, True, act)
        gout = torch.randn(want.shape)
        (want * gout).sum().backward()
        layer = layer.to(dev)
        xg = x.detach().to(dev).requires_grad_(True)
        out = layer(xg)
        assert _lib.get_option("last_fwd_kernel") == 2          # the bf16 kernel ran, not a fallback
        (out * gout.to(dev)).sum().backward()
        assert _lib.get_option("last_bwx_kernel") == 2 and _lib.get_option("last_bww_kernel") == 2

        def rel(got, w):
            w = w.detach().numpy()
            return float(np.abs(got.detach().cpu().numpy() - w).max() / np.abs(w).max())

        def cos(got, w):
            a, b = got.detach().cpu().numpy().ravel().astype(np.float64), w.detach().numpy().ravel().astype(np.float64)
            return float(a @ b / np.sqrt((a @ a) * (b @ b)))

        assert rel(out, want) < 2e-2, rel(out, want)
        pairs = [(xg.grad, x.grad)] + [(c.weight.grad, W[i].grad) for i, c in enumerate(layer.conv1ds)] + \
            [(c.bias.grad, Bs[i].grad) for i, c in enumerate(layer.conv1ds)]
        for got, w in pairs:
            assert cos(got, w) > 0.998, cos(got, w)
            if act == "linear":
                assert rel(got, w) < 4e-2, rel(got, w)
    finally:
        _lib.set_option("cin_math", old)


@pytest.mark.parametrize("B", [512, 4096])          # 4096 = BASELINE config 5's per-GPU batch
def test_model_in_bf16_cin_arithmetic_tracks_the_fp32_modes(B):
    """Whole model, config-5 shape (22 sparse fields, D = 32, cin (512,256,256,128)), 6 Adam steps in cin_math 2 and in
    cin_math 1 from the same initial weights on the same batches: losses within 2e-3 relative, predictions within 5e-3
    absolute, logloss / AUC of the final predictions within 2e-3 -- the bf16 tolerance of SURVEY 8(d)."""
    from deepctr.inputs import SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import _lib, metrics as M
    dev = _dev()
    vocab, D = [500] * 22, 32
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)]
    old = _lib.get_option("cin_math")

    def run(mode):
        _lib.set_option("cin_math", mode)
        model = xDeepFM(cols, cols, cin_layer_size=(512, 256, 256, 128), dnn_hidden_units=(256, 256), init_std=0.05, device=dev)
        model.compile("adam", "binary_crossentropy", metrics=[])
        model.train()
        losses = []
        for s in range(6):
            X, y = orc.synthetic_batch(B, vocab, 0, seed=40 + s)
            losses.append(float(model.train_on_batch(T(X).to(dev), T(y).to(dev))[1]))
        X, y = orc.synthetic_batch(2048, vocab, 0, seed=99)
        names = list(model.feature_index.keys())
        return losses, model.predict({n: X[:, i] for i, n in enumerate(names)}, 512), y

    try:
        l2, p2, y = run(2)
        l1, p1, _ = run(1)
    finally:
        _lib.set_option("cin_math", old)
    np.testing.assert_allclose(l2, l1, rtol=2e-3)
    assert np.abs(p2 - p1).max() < 5e-3
    assert abs(M.log_loss(y, p2) - M.log_loss(y, p1)) < 2e-3 and abs(M.roc_auc_score(y, p2) - M.roc_auc_score(y, p1)) < 2e-3


def _near_zero_preactivation_columns(x0, W, Bs, eps):
    """[B, D] mask of the (example, d) columns in which some CIN pre-activation has |z| < eps
    (level loop of deepctr/layers/interaction.py:216-243, split_half=True, relu)."""
    B, m, D = x0.shape
    hidden, risky = x0.double(), torch.zeros(B, D, dtype=torch.bool)
    for i, (w, b) in enumerate(zip(W, Bs)):
        z = torch.einsum("bhd,bmd->bhmd", hidden, x0.double()).reshape(B, hidden.shape[1] * m, D)
        z = torch.nn.functional.conv1d(z, w.double(), b.double())
        risky |= (z.abs() < eps).any(dim=1)
        cur = torch.relu(z)
        hidden = cur[:, : w.shape[0] // 2] if i != len(W) - 1 else None
    return risky


def _cin_fp64(x, Ws, Bs):
    """CIN forward in fp64 torch ops (deepctr/layers/interaction.py:207-248, split_half, relu)."""
    B, m, D = x.shape
    hidden, finals = x, []
    for i, (w, b) in enumerate(zip(Ws, Bs)):
        z = torch.einsum("bhd,bmd->bhmd", hidden, x).reshape(B, hidden.shape[1] * m, D)
        cur = torch.relu(torch.nn.functional.conv1d(z, w, b))
        if i != len(Ws) - 1:
            hidden, direct = cur[:, : w.shape[0] // 2], cur[:, w.shape[0] // 2:]
        else:
            direct = cur
        finals.append(direct)
    return torch.cat(finals, 1).sum(-1)


@pytest.mark.parametrize("B,m,D,ls,spread", [(512, 26, 16, (256, 128, 128), False), (512, 26, 16, (256, 128, 128), True),
                                              (96, 22, 32, (512, 256, 256, 128), False), (300, 26, 8, (128, 128), True)])
def test_cin_f16x3_is_as_accurate_as_fp32_mfma(B, m, D, ls, spread):
    """The claim that makes f16x3 an fp32 path: against an fp64 evaluation of the same CIN its error is
    not larger than that of the fp32-MFMA kernels (both are dominated by the fp32 accumulation).  With
    `spread` the examples' magnitudes cover 8 decades (per-column range fitting of the fp16 halves)."""
    from deepctr.layers import CIN
    from xdfm_amd import _lib
    dev = _dev()
    torch.manual_seed(B + m)
    layer = CIN(m, ls, "relu", True, 0.0, 1024, device="cpu").to(dev)
    x = torch.randn(B, m, D, device=dev) * 0.5
    if spread:
        x = x * torch.pow(10.0, torch.rand(B, 1, 1, device=dev) * 8 - 6)
    W64 = [c.weight.detach().double().requires_grad_(True) for c in layer.conv1ds]
    B64 = [c.bias.detach().double().requires_grad_(True) for c in layer.conv1ds]
    # A ReLU whose pre-activation is within rounding of zero may switch on in one arithmetic and not in the
    # other, which changes gradients legitimately: drop the examples that hold such a pre-activation
    # (|z| < 1e-5 x the largest |z| of the same example, level and d) before comparing anything.
    with torch.no_grad():
        hid, safe = x.double(), torch.ones(B, dtype=torch.bool, device=dev)
        for i, (w, b) in enumerate(zip(W64, B64)):
            z = torch.nn.functional.conv1d(torch.einsum("bhd,bmd->bhmd", hid, x.double()).reshape(B, -1, D), w, b)
            safe &= ~(z.abs() < 1e-5 * z.abs().amax(dim=1, keepdim=True)).flatten(1).any(dim=1)
            hid = torch.relu(z)[:, : w.shape[0] // 2]
    assert float(safe.float().mean()) > 0.3
    x = x[safe].contiguous()
    x64 = x.double().requires_grad_(True)
    want = _cin_fp64(x64, W64, B64)
    gout = torch.randn(want.shape, device=dev)
    (want * gout.double()).sum().backward()
    den = want.detach().abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
    err = {}
    old = _lib.get_option("cin_math")
    try:
        for mode in (0, 1):
            _lib.set_option("cin_math", mode)
            for c in layer.conv1ds:
                c.weight.grad = c.bias.grad = None
            xg = x.clone().requires_grad_(True)
            out = layer(xg)
            (out * gout).sum().backward()
            e = ((out.detach().double() - want.detach()) / den)
            # per example: a small-magnitude example must be as accurate as a large one
            gx = ((xg.grad.double() - x64.grad).abs().flatten(1).amax(dim=1) /
                  x64.grad.abs().flatten(1).amax(dim=1).clamp_min(1e-300)).max().item()
            err[mode] = dict(fwd_rms=e.pow(2).mean().sqrt().item(), fwd_max=e.abs().max().item(), dx=gx,
                             dw=[((c.weight.grad.double() - w.grad).abs().amax() / w.grad.abs().amax()).item()
                                 for c, w in zip(layer.conv1ds, W64)])
    finally:
        _lib.set_option("cin_math", old)
    assert err[1]["fwd_rms"] <= 1.25 * err[0]["fwd_rms"] + 1e-9, err
    assert err[1]["fwd_max"] <= 2.0 * err[0]["fwd_max"] + 1e-8, err
    assert err[1]["fwd_max"] < 5e-6 and err[1]["dx"] < 5e-6, err
    assert err[1]["dx"] <= 2.0 * err[0]["dx"] + 2e-7, err
    for a, b in zip(err[1]["dw"], err[0]["dw"]):
        assert a <= 2.0 * b + 2e-7 and a < 5e-6, err


@pytest.mark.parametrize("case", ["fields", "weight_row", "dout_rows"])
def test_cin_f16x3_range_fitting_corners(case):
    """The fp16 halves of the f16x3 arithmetic are range-fitted per scale GROUP (forward / dX: one scale per column n
    for x0[:, n], x_prev[:, n], dOut[:, n], one per level for W; dW: one per row).  VERDICT r1 asked for wide dynamic
    range INSIDE one group, against the fp64 CIN, measured on the small entries:
      fields      the 26 fields of every x0 column span 1e-6 .. 1 (field j scaled by 10^(-6 j / 25));
      weight_row  one weight row of every level is 1e6 x the others (one scale per level);
      dout_rows   the upstream gradient spans 8 decades over the examples, i.e. inside every row of dOut (dW scales rows).
    Bound asserted: 1e-5 of the magnitude of the entry's own group (example row / field / weight row) for outputs,
    dx and dW -- elements further than 2^18 below their group's maximum keep an ABSOLUTE error of 2^-40 of that
    maximum (include/xdfm.h), which these cases show is enough.  The kernels that ran are asserted (no silent fallback)."""
    from deepctr.layers import CIN
    from xdfm_amd import _lib
    dev = _dev()
    B, m, D, ls = 384, 26, 16, (256, 128, 128)
    torch.manual_seed(7)
    layer = CIN(m, ls, "relu", True, 0.0, 1024, device="cpu").to(dev)
    x = torch.randn(B, m, D, device=dev) * 0.5
    fscale = torch.ones(m, device=dev)
    if case == "fields":
        fscale = torch.pow(10.0, -6.0 * torch.arange(m, device=dev) / (m - 1))
        x = x * fscale[None, :, None]
    big_rows = []
    if case == "weight_row":
        with torch.no_grad():
            for c in layer.conv1ds:             # the LAST row: a direct-connect map, so the next level's inputs stay ordinary
                c.weight[-1] *= 1e6
                c.bias[-1] *= 1e6
            big_rows = [-1]
    gscale = torch.ones(B, 1, device=dev)
    if case == "dout_rows":
        gscale = torch.pow(10.0, torch.rand(B, 1, device=dev) * 8 - 8)
    W64 = [c.weight.detach().double().requires_grad_(True) for c in layer.conv1ds]
    B64 = [c.bias.detach().double().requires_grad_(True) for c in layer.conv1ds]
    with torch.no_grad():                      # drop examples with a pre-activation within rounding of the ReLU kink
        hid, safe = x.double(), torch.ones(B, dtype=torch.bool, device=dev)
        for i, (w, b) in enumerate(zip(W64, B64)):
            z = torch.nn.functional.conv1d(torch.einsum("bhd,bmd->bhmd", hid, x.double()).reshape(B, -1, D), w, b)
            ref = z.abs().amax(dim=1, keepdim=True)
            if big_rows:                        # the kink test is per row group: the huge row must not hide the others
                small = torch.ones(z.shape[1], dtype=torch.bool, device=dev)
                small[big_rows] = False
                ref = z[:, small].abs().amax(dim=1, keepdim=True)
                safe &= ~(z[:, small].abs() < 1e-5 * ref).flatten(1).any(dim=1)
            else:
                safe &= ~(z.abs() < 1e-5 * ref).flatten(1).any(dim=1)
            hid = torch.relu(z)[:, : w.shape[0] // 2]
    assert float(safe.float().mean()) > 0.2
    x, gscale = x[safe].contiguous(), gscale[safe]
    x64 = x.double().requires_grad_(True)
    want = _cin_fp64(x64, W64, B64)
    gout = torch.randn(want.shape, device=dev) * gscale
    (want * gout.double()).sum().backward()
    old = _lib.get_option("cin_math")
    try:
        _lib.set_option("cin_math", 1)
        for c in layer.conv1ds:
            c.weight.grad = c.bias.grad = None
        xg = x.clone().requires_grad_(True)
        out = layer(xg)
        assert _lib.get_option("last_fwd_kernel") == 1
        (out * gout).sum().backward()
        assert _lib.get_option("last_bwx_kernel") == 1 and _lib.get_option("last_bww_kernel") == 1
    finally:
        _lib.set_option("cin_math", old)
    # outputs: per feature map relative to that feature map's magnitude over the batch (the maps of small weight rows
    # are 1e6 x smaller than the huge row's) and per example
    e = (out.detach().double() - want.detach()).abs()
    per_map = (e / want.detach().abs().amax(dim=0, keepdim=True).clamp_min(1e-300)).max().item()
    per_ex = (e / want.detach().abs().amax(dim=1, keepdim=True).clamp_min(1e-300)).max().item()
    # dx: per (example, field) relative to that field's gradient magnitude in the example -- small fields on their own
    gx, wx = xg.grad.double(), x64.grad
    dx = ((gx - wx).abs().amax(dim=2) / wx.abs().amax(dim=2).clamp_min(1e-300)).max().item()
    # dW: per (level, weight row h, field j) group relative to the group's largest entry
    dw = 0.0
    for c, w in zip(layer.conv1ds, W64):
        H = w.shape[0]
        g, ww = c.weight.grad.double().reshape(H, -1, m), w.grad.reshape(H, -1, m)
        dw = max(dw, ((g - ww).abs().amax(dim=1) / ww.abs().amax(dim=1).clamp_min(1e-300)).max().item())
    # level 0 runs on folded weights W(i,j) + W(j,i), range-fitted with half the level's scale (the sums reach twice the
    # maximum): weights 2^20 below the maximum carry an absolute error of 2^-39 instead of 2^-40 of it -- visible only in
    # this corner (measured 1.7e-5; 8e-6 with the full (i, j) grid, option x3_sym = 0)
    dx_bound = 2.5e-5 if case == "weight_row" else 1e-5
    assert per_ex < 1e-5 and dx < dx_bound and dw < 1e-5, (case, per_map, per_ex, dx, dw)
    assert per_map < (1e-5 if case != "weight_row" else 4e-5), (case, per_map)


def test_cin_rejects_bad_input_like_reference():
    from deepctr.layers import CIN
    dev = _dev()
    layer = CIN(4, (8, 4), device=dev)
    with pytest.raises(ValueError):
        layer(torch.zeros(3, 4, device=dev))
    with pytest.raises(ValueError):
        CIN(4, ())
    with pytest.raises(ValueError):
        CIN(4, (7, 4))
    with pytest.raises(RuntimeError):
        CIN(4, (8, 4))(torch.zeros(2, 4, 8))       # CPU tensor: no fallback


@pytest.mark.parametrize("name", golden_names("attn_"))
def test_cin_attention_vs_reference_golden(name):
    from deepctr.layers import CINAttention, CINAttentionV2
    dev = _dev()
    g = load_golden(name)
    ls = tuple(int(v) for v in g["layer_size"])
    B, m, D = g["x"].shape
    kw = dict(num_heads=int(g["num_heads"]), use_layer_norm=bool(g["use_layer_norm"]),
              use_residual=bool(g["use_residual"]))
    if str(g["variant"]) == "attn":
        layer = CINAttention(m, D, ls, "relu", True, attn_dropout=0.0, device=dev, **kw)
    else:
        layer = CINAttentionV2(m, D, ls, "relu", True, attn_dropout=0.0, num_attn_layers=int(g["num_attn_layers"]),
                               device=dev, **kw)
    sd = {k[2:]: T(v) for k, v in g.items() if k.startswith("p:")}
    layer.load_state_dict(sd, strict=True)
    x = T(g["x"]).to(dev).requires_grad_(True)
    out = layer(x)
    close(out, g["out"], rtol=5e-5, atol=5e-6, msg="out")
    (out * T(g["gout"]).to(dev)).sum().backward()
    gclose(x.grad, g["dx"], "dx")
    for k, p in layer.named_parameters():
        if k.startswith("conv1ds"):
            gclose(p.grad, g["g:" + k], k)
        else:
            # gradients of the attention block pass through softmax / LayerNorm cancellations
            # (sum_s dscore_s = 0) and are O(1e-5) here, so the fp32 reference itself is only good to
            # ~1e-2 of the tensor's scale: compare against that scale, not element by element
            want = g["g:" + k]
            close(p.grad, want, rtol=2e-3, atol=1e-2 * float(np.abs(want).max()) + 1e-9, msg=k)


# --------------------------------------------------------------------------------------------- #
def _build_model(g, dev):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr import models
    vocab = [int(v) for v in g["vocab"]]
    nd, D = int(g["n_dense"]), int(g["emb_dim"])
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    kw = dict(zip([str(k) for k in g["kw_keys"]], [int(v) for v in g["kw_vals"]]))
    cls = getattr(models, str(g["cls"]))
    model = cls(cols, cols, dnn_hidden_units=tuple(int(v) for v in g["dnn"]),
                cin_layer_size=tuple(int(v) for v in g["cin"]), l2_reg_dnn=1e-5, device=dev, **kw)
    return model


@pytest.mark.parametrize("name", golden_names("model_"))
def test_model_vs_reference_golden(name, cin_math):
    dev = _dev()
    g = load_golden(name)
    model = _build_model(g, dev)
    # same seed -> the reference's own initial weights (RNG order parity)
    for k, v in model.state_dict().items():
        want = g["init:" + k]
        np.testing.assert_array_equal(v.cpu().numpy()[: want.shape[0]], want, err_msg="init " + k)
    model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
    B = int(g["B"])
    X, y = T(g["X"]).to(dev), T(g["y"]).to(dev)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    model.train()
    import warnings
    from xdfm_amd import _lib, ops
    ops._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        y_pred = model(X[:B])
        close(y_pred, g["y_pred"], rtol=2e-5, atol=1e-6, msg="y_pred")
        loss = torch.nn.functional.binary_cross_entropy(y_pred.squeeze(), y[:B].squeeze(), reduction="sum")
        reg = model.get_regularization_loss()
        assert abs(loss.item() - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
        assert abs(reg.item() - float(g["reg"])) <= 1e-5 * abs(float(g["reg"]))
        model.optim.zero_grad()
        (loss + reg).backward()
    if name.startswith("model_x3_") and cin_math == 1:
        assert not [w for w in caught if "fp32-MFMA arithmetic" in str(w.message)], [str(w.message) for w in caught]
        assert _lib.get_option("last_fwd_kernel") == _lib.get_option("last_bwx_kernel") == _lib.get_option("last_bww_kernel") == 1
    for k, p in model.named_parameters():
        gclose(p.grad, g["g:" + k], k)
    model.optim.zero_grad()
    # three Adam steps, as BaseModel.fit does them
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
    # logloss / AUC within the north-star tolerance of 1e-5 against the reference's predictions
    from xdfm_amd import metrics as M
    yn = g["y"]
    assert abs(M.log_loss(yn, pred) - M.log_loss(yn, g["pred_after"])) < 1e-5
    assert abs(M.roc_auc_score(yn, pred) - M.roc_auc_score(yn, g["pred_after"])) < 1e-5


def test_fit_history_vs_reference_golden(cin_math):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    dev = _dev()
    g = load_golden("fit_history")
    vocab, nd, D = [int(v) for v in g["vocab"]], int(g["n_dense"]), int(g["emb_dim"])
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(8,), cin_layer_size=(6, 4), l2_reg_dnn=1e-5, device=dev)
    for k, v in model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), g["s0:" + k], err_msg=k)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    for pg in model.optim.param_groups:
        pg["lr"] = 1e-2
    names = list(model.feature_index.keys())
    X, y, Xv, yv = g["X"], g["y"], g["Xv"], g["yv"]
    hist = model.fit({n: X[:, i] for i, n in enumerate(names)}, y, batch_size=64, epochs=2, verbose=2,
                     validation_data=({n: Xv[:, i] for i, n in enumerate(names)}, yv), shuffle=False)
    keys = sorted(hist.history.keys())
    assert keys == [str(k) for k in g["hist_keys"]]
    got = np.array([hist.history[k] for k in keys])
    np.testing.assert_allclose(got, g["hist_vals"], rtol=2e-4, atol=2e-5)
    pred = model.predict({n: Xv[:, i] for i, n in enumerate(names)}, 32)
    np.testing.assert_allclose(pred, g["pred"], rtol=2e-4, atol=1e-6)


# --------------------------------------------------------------------------------------------- #
def test_gather_scatter_vs_oracle():
    """K1/K2 alone: ids incl. 0, vocab-1 and repeats; D not a multiple of 4; partial last block."""
    from xdfm_amd import ops
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    for (B, vocab, nd, D) in [(37, [5, 9, 3, 17, 2], 3, 10), (300, [50] * 26, 13, 16), (1, [4, 4], 0, 3)]:
        m = len(vocab)
        X, _ = orc.synthetic_batch(B, vocab, nd, seed=B)
        X[0, :m] = 0
        X[-1, :m] = np.array(vocab) - 1
        spec = orc.Spec(["C%d" % i for i in range(m)], vocab, ["I%d" % i for i in range(nd)], D)
        g = torch.Generator().manual_seed(1)
        st = {}
        for n, v in zip(spec.sparse_names, vocab):
            st["embedding_dict.%s.weight" % n] = torch.randn(v, D, generator=g).requires_grad_(True)
            st["linear_model.embedding_dict.%s.weight" % n] = torch.randn(v, 1, generator=g).requires_grad_(True)
        if nd:
            st["linear_model.weight"] = torch.randn(nd, 1, generator=g).requires_grad_(True)
        Xt = T(X)
        emb = orc.embed_gather(Xt, st, spec)
        lin = orc.linear_logit(Xt, st, spec)
        dnn = orc.combined_dnn_input(emb, orc.dense_values(Xt, spec))
        ge, gd, gl = torch.randn(emb.shape, generator=g), torch.randn(dnn.shape, generator=g), \
            torch.randn(lin.shape, generator=g)
        ((emb * ge).sum() + (dnn * gd).sum() + (lin * gl).sum()).backward()

        plan = ops.EmbedPlan(list(range(m)), vocab, list(range(m, m + nd)), D)
        tabs = [st["embedding_dict.%s.weight" % n].detach().to(dev).requires_grad_(True) for n in spec.sparse_names]
        lins = [st["linear_model.embedding_dict.%s.weight" % n].detach().to(dev).requires_grad_(True)
                for n in spec.sparse_names]
        w = st["linear_model.weight"].detach().to(dev).requires_grad_(True) if nd else None
        emb_fm, dnn_in, lin_out = ops.EmbedGather.apply(Xt.to(dev), w, plan, True, *tabs, *lins)
        got_emb = ops.from_fm_layout(emb_fm, B, D)
        np.testing.assert_array_equal(got_emb.detach().cpu().numpy(), emb.detach().numpy())
        np.testing.assert_array_equal(dnn_in.detach().cpu().numpy(), dnn.detach().numpy())
        close(lin_out, lin.detach().numpy(), rtol=1e-6, atol=1e-6)
        ((got_emb * ge.to(dev)).sum() + (dnn_in * gd.to(dev)).sum() + (lin_out * gl.to(dev)).sum()).backward()
        for n, t, l in zip(spec.sparse_names, tabs, lins):
            gclose(t.grad, st["embedding_dict.%s.weight" % n].grad.numpy(), n)
            gclose(l.grad, st["linear_model.embedding_dict.%s.weight" % n].grad.numpy(), "lin " + n)
        if nd:
            gclose(w.grad, st["linear_model.weight"].grad.numpy(), "dense w")
        assert not plan.check_ids(dev)


def _scatter_raw(X, vocab, nd, D, d_emb, d_dnn, d_lin, dev, with_marks=False):
    """xdfm_embed_scatter_bwd_marked through the C ABI on host arrays -> (flat gradient buffer, offsets, marks)."""
    import ctypes
    from xdfm_amd import _lib
    lib = _lib.load()
    B, m = X.shape[0], len(vocab)
    sizes = [v * D for v in vocab] + [v for v in vocab]
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4
    total = off
    flat = torch.zeros(total + max(nd, 1) + 3, dtype=torch.float32, device=dev)
    marks = torch.zeros(flat.numel() // 4 + 2, dtype=torch.uint8, device=dev) if with_marks else None
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    i32 = dict(dtype=torch.int32, device=dev)
    cols, voc = torch.arange(m, **i32), torch.tensor(vocab, **i32)
    dcols = torch.arange(m, m + max(nd, 1), **i32)
    off_dev = torch.tensor(offs, dtype=torch.int64, device=dev)
    Xd = T(X).to(dev)
    de = None if d_emb is None else T(np.ascontiguousarray(d_emb.transpose(1, 0, 2).reshape(m, B * D))).to(dev)
    dd = None if d_dnn is None else T(d_dnn).to(dev)
    dl = None if d_lin is None else T(d_lin).to(dev)
    dw = flat[total:total + nd] if nd else None
    _lib.check(lib.xdfm_embed_scatter_bwd_marked(
        P(Xd), Xd.stride(0), B, P(cols), P(voc), m, D, P(dcols) if nd else None, nd, P(de), P(dd), 0, P(dl), 0,
        P(flat), P(off_dev[:m]), P(off_dev[m:]) if dl is not None else None, P(dw) if dl is not None else None,
        P(marks), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "scatter")
    torch.cuda.synchronize()
    return flat.cpu().numpy(), offs, total, (marks.cpu().numpy() if with_marks else None)


def _scatter_expected(X, vocab, nd, D, d_emb, d_dnn, d_lin):
    """Per destination element: the fp32-rounded exact (float64) sum of its fp32 addends g = d_emb + d_dnn."""
    B, m = X.shape[0], len(vocab)
    g = np.zeros((B, m, D), dtype=np.float32)
    if d_emb is not None:
        g = g + d_emb
    if d_dnn is not None:
        g = (g + d_dnn[:, :m * D].reshape(B, m, D)).astype(np.float32)
    tabs, lins = [], []
    for j, v in enumerate(vocab):
        ids = np.clip(X[:, j].astype(np.int64), 0, v - 1)
        t = np.zeros((v, D), dtype=np.float64)
        np.add.at(t, ids, g[:, j, :].astype(np.float64))
        tabs.append(t)
        l = np.zeros(v, dtype=np.float64)
        if d_lin is not None:
            np.add.at(l, ids, d_lin.astype(np.float64))
        lins.append(l)
    dw = None
    if nd and d_lin is not None:
        prod = (X[:, m:m + nd] * d_lin[:, None]).astype(np.float32)          # the kernel forms the products in fp32
        dw = prod.astype(np.float64).sum(0)
    return tabs, lins, dw


@pytest.mark.parametrize("B,vocab,nd,D,srcs", [
    (4096, [1000] * 26, 13, 16, "edl"),          # BASELINE config 2 shape: Zipf ids, hot rows of hundreds of examples
    (4096, [3, 1, 100000, 7] * 2, 2, 16, "edl"),    # a whole chunk on ONE row (vocab 1) and on three rows
    (5000, [50] * 5, 3, 32, "edl"),              # two chunks (4096 + 904) and two 16-column slices per field
    (777, [11, 300, 5], 0, 10, "ed"),            # D not a multiple of 4 (scalar lanes), no dense part, no linear part
    (64, [9] * 4, 1, 8, "d"),                    # only the DNN-side gradient
    (1, [4, 4], 0, 3, "e"),
])
def test_scatter_is_exact_deterministic_and_order_independent(B, vocab, nd, D, srcs):
    """K2 (`embed_scatter_grouped_kernel`): the examples of a chunk are grouped by id through a hash table in LDS (equal ids
    adjacent, the groups in no particular order), then a segmented, atomics-free reduce of the row gradients.  Checked here:
    (1) every element is the EXACT sum of its addends rounded to fp32, to within one ulp (float64 reference; an addend
        more than 2^14 below the largest of its run is first rounded to a grid 2^-13 fp32-ulp fine, which can turn a
        near-tie of the final rounding; the reference's CPU `embedding_dense_backward`, deepctr/inputs.py:168, sums
        the same addends in fp32 in example order, i.e. within a few ulp of this);
    (2) two runs give bit-identical buffers;
    (3) a permutation of the examples gives bit-identical buffers (identical scatter on every rank);
    (4) the chunk marks cover exactly the touched 16-byte chunks."""
    dev = _dev()
    m = len(vocab)
    rng = np.random.default_rng(B + D)
    X = np.zeros((B, m + nd), dtype=np.float32)
    for j, v in enumerate(vocab):
        X[:, j] = np.floor(v * rng.random(B) ** 3)
    X[:, m:] = rng.random((B, nd))
    mag = 10.0 ** rng.integers(-6, 2, size=(B, 1, 1))                       # rows of very different magnitudes
    d_emb = (rng.standard_normal((B, m, D)) * mag).astype(np.float32) if "e" in srcs else None
    d_dnn = (rng.standard_normal((B, m * D + nd)) * mag[:, 0]).astype(np.float32) if "d" in srcs else None
    d_lin = (rng.standard_normal(B) * mag[:, 0, 0]).astype(np.float32) if "l" in srcs else None
    flat, offs, total, marks = _scatter_raw(X, vocab, nd, D, d_emb, d_dnn, d_lin, dev, with_marks=True)
    tabs, lins, dw = _scatter_expected(X, vocab, nd, D, d_emb, d_dnn, d_lin)
    nchunk = (B + 4095) // 4096      # more than one chunk: the chunks' exact sums are added in fp32, in chunk order
    multi = nchunk > 1

    def check(got, exact, addends_max, n_addends, what):
        # half an ulp of the final rounding + the fixed-point grid of the addends (2^-38 of the run's largest
        # magnitude each); with several chunks the chunks' sums (each up to n * max) are added in fp32
        scale = n_addends * addends_max if multi else np.abs(exact)
        ulp = np.spacing(np.maximum(np.abs(exact), scale).astype(np.float32)).astype(np.float64)
        tol = (0.5 + 1e-3) * nchunk * ulp + n_addends * addends_max * 2.0 ** -37
        bad = np.abs(got.astype(np.float64) - exact) > tol
        assert not bad.any(), "%s: %d elements off, worst %g" % (what, int(bad.sum()), float(np.abs(got - exact).max()))

    g = np.zeros((B, m, D), dtype=np.float32)
    if d_emb is not None:
        g = g + d_emb
    if d_dnn is not None:
        g = (g + d_dnn[:, :m * D].reshape(B, m, D)).astype(np.float32)
    for j, v in enumerate(vocab):
        ids = np.clip(X[:, j].astype(np.int64), 0, v - 1)
        cnt = np.bincount(ids, minlength=v).astype(np.float64)
        gmax = np.zeros((v, D))
        np.maximum.at(gmax, ids, np.abs(g[:, j, :]).astype(np.float64))
        check(flat[offs[j]:offs[j] + v * D].reshape(v, D), tabs[j], gmax, cnt[:, None], "table %d" % j)
        if d_lin is not None:
            lmax = np.zeros(v)
            np.maximum.at(lmax, ids, np.abs(d_lin).astype(np.float64))
            check(flat[offs[m + j]:offs[m + j] + v], lins[j], lmax, cnt, "linear table %d" % j)
    if dw is not None:
        prod = np.abs((X[:, m:m + nd] * d_lin[:, None]).astype(np.float32)).astype(np.float64)
        check(flat[total:total + nd], dw, prod.max(0), float(B), "dense weight")
    # (4) marks: a chunk is marked iff the scatter wrote into it
    touched = np.zeros(flat.size // 4 + 2, dtype=bool)
    for j, v in enumerate(vocab):
        ids = np.unique(np.clip(X[:, j].astype(np.int64), 0, v - 1))
        e = (offs[j] + ids[:, None] * D + np.arange(D)[None, :]).reshape(-1)
        touched[e >> 2] = True
        if d_lin is not None:
            touched[(offs[m + j] + ids) >> 2] = True
    if dw is not None:
        touched[(total + np.arange(nd)) >> 2] = True
    np.testing.assert_array_equal(marks.astype(bool), touched)
    # (2) run to run
    flat2, _, _, _ = _scatter_raw(X, vocab, nd, D, d_emb, d_dnn, d_lin, dev)
    np.testing.assert_array_equal(flat2.view(np.uint32), flat.view(np.uint32))
    # (3) permuted examples (within one chunk the result is a function of the multiset of rows)
    if not multi:
        p = rng.permutation(B)
        pick = lambda a: None if a is None else np.ascontiguousarray(a[p])
        flat3, _, _, _ = _scatter_raw(np.ascontiguousarray(X[p]), vocab, nd, D, pick(d_emb), pick(d_dnn), pick(d_lin), dev)
        np.testing.assert_array_equal(flat3.view(np.uint32), flat.view(np.uint32))


def test_gather_flags_out_of_range_ids():
    from xdfm_amd import ops
    dev = _dev()
    plan = ops.EmbedPlan([0, 1], [4, 4], [], 4)
    tabs = [torch.randn(4, 4, device=dev) for _ in range(2)]
    X = torch.tensor([[1.0, 7.0], [0.0, 2.0]], device=dev)
    ops.EmbedGather.apply(X, None, plan, False, *tabs)
    assert plan.check_ids(dev)
    assert not plan.check_ids(dev)


def test_full_size_cin_rows_vs_oracle_subset(cin_math):
    """BASELINE config 2 shape (B=4096, m=26, D=16, cin=(256,128,128)): examples are independent,
    so 48 rows of the full-size launch are compared with the oracle run on just those rows, and
    gradients are checked through linearity: dW of the full batch restricted to a gout that is
    zero outside the subset equals the oracle's dW on the subset."""
    from deepctr.layers import CIN
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    B, m, D, ls = 4096, 26, 16, (256, 128, 128)
    torch.manual_seed(5)
    layer = CIN(m, ls, "relu", True, 0.0, 1024, device="cpu")
    x = torch.randn(B, m, D) * 0.5
    rows = torch.randperm(B)[:48]
    W = [c.weight.detach().clone().requires_grad_(True) for c in layer.conv1ds]
    Bs = [c.bias.detach().clone().requires_grad_(True) for c in layer.conv1ds]
    xs = x[rows].clone().requires_grad_(True)
    want = orc.cin_forward(xs, W, Bs, True, "relu")
    gsub = torch.randn(want.shape)
    (want * gsub).sum().backward()
    layer = layer.to(dev)
    xg = x.to(dev).requires_grad_(True)
    out = layer(xg)
    close(out[rows.to(dev)], want.detach().numpy(), msg="out rows")
    gout = torch.zeros(B, want.shape[1])
    gout[rows] = gsub
    (out * gout.to(dev)).sum().backward()
    gclose(xg.grad[rows.to(dev)], xs.grad.numpy(), "dx rows")
    mask = torch.ones(B, dtype=torch.bool)
    mask[rows] = False
    assert float(xg.grad[mask.to(dev)].abs().max()) == 0.0      # untouched examples get exactly zero
    for i, c in enumerate(layer.conv1ds):
        gclose(c.weight.grad, W[i].grad.numpy(), "dw%d" % i)
        gclose(c.bias.grad, Bs[i].grad.numpy(), "db%d" % i)


@pytest.mark.parametrize("cls_name,B,D,kw", [
    ("xDeepFMAttention", 512, 16, dict(cin_num_heads=4)),
    ("xDeepFMAttentionV2", 300, 8, dict(cin_num_heads=2, cin_num_attn_layers=2)),
    ("xDeepFMAttention", 96, 16, dict(cin_num_heads=4, cin_attn_dropout=0.2)),
], ids=["attn", "attn_v2_two_layers", "attn_dropout"])
def test_attention_step_gradients_are_bit_identical_run_to_run(cls_name, B, D, kw):
    """K5 (attention block): since round 3 its parameter gradients are per-workgroup shares added in workgroup order
    (xdfm_cin_attn_pool_bwd_det) and the block sums inside a workgroup go through LDS in wave order -- no float atomics.
    Forward + backward four times on one batch: prediction and every gradient (incl. W_q / W_k / W_v / W_o, LayerNorm
    and pooling parameters) must have the same bits each time; with dropout the seed is fixed per repetition."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr import models
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    vocab = [400] * 26
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(13)]
    torch.manual_seed(9)
    model = getattr(models, cls_name)(cols, cols, cin_layer_size=(64, 48), l2_reg_dnn=1e-5, device=dev, **kw)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k:
                p.mul_(3000.0)
    model.train()
    X, y = orc.synthetic_batch(B, vocab, 13, seed=12)
    X, y = T(X).to(dev), T(y).to(dev)
    ref = None
    for rep in range(4):
        torch.manual_seed(77)                    # the dropout seed is drawn from torch's generator
        model.zero_grad()
        out = model(X)
        torch.nn.functional.binary_cross_entropy(out.squeeze(), y.squeeze(), reduction="sum").backward()
        got = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        got["prediction"] = out.detach().clone()
        if ref is None:
            ref = got
            assert any("mhsa" in k for k in ref) and any("attn_pooling" in k for k in ref)
        else:
            for k in ref:
                assert torch.equal(got[k], ref[k]), "run %d: %s differs" % (rep, k)


@pytest.mark.parametrize("B,D", [(4096, 16), (256, 10)])
def test_whole_step_gradients_are_bit_identical_run_to_run(B, D, cin_math):
    """Forward + backward of the xDeepFM step five times on one batch: the prediction and EVERY parameter gradient must
    be the same bits each time, at BASELINE config 2's size and at the scripts' default embedding_dim = 10 (generic,
    non-vectorised code paths).  What this pins: K2 is an exact reduce, dW sums its slabs in a fixed order, and the CIN
    bias gradients are per-block partials added in block order (they were one float atomic per block: 16 blocks per row
    at B = 4096 -- found by the deferred-Adam bit-equality test).  The attention variants have their own test above."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    vocab = [1000] * 26
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(13)]
    torch.manual_seed(9)
    model = xDeepFM(cols, cols, cin_layer_size=(256, 128, 128) if B > 1000 else (64, 48), l2_reg_dnn=1e-5, device=dev)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k:
                p.mul_(3000.0)
    X, y = orc.synthetic_batch(B, vocab, 13, seed=11)
    X, y = T(X).to(dev), T(y).to(dev)
    ref = None
    for rep in range(5):
        model.zero_grad()
        out = model(X)
        torch.nn.functional.binary_cross_entropy(out.squeeze(), y.squeeze(), reduction="sum").backward()
        got = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        got["prediction"] = out.detach().clone()
        if ref is None:
            ref = got
            assert len(ref) >= 60
        else:
            for k in ref:
                assert torch.equal(got[k], ref[k]), "run %d: %s differs" % (rep, k)


def test_l2_regulariser_kernel_vs_torch():
    """K6: value and gradient of sum_t l2_t * sum(w_t^2) against the reference's per-tensor formula
    (deepctr/models/basemodel.py:412-428), on odd sizes / unaligned views."""
    from xdfm_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    base = torch.randn(200003, generator=g).to(dev)
    shapes = [(1,), (7, 3), (1000, 16), (50000, 1), (13, 1), (257,)]
    coeffs = [1e-5, 2e-5, 1e-5, 3e-4, 1e-5, 0.5]
    tensors, off = [], 1                      # offset 1 -> 4-byte aligned only
    for s in shapes:
        n = int(np.prod(s))
        tensors.append(base[off:off + n].view(s).detach().requires_grad_(True))
        off += n
    plan = ops.L2Plan(coeffs)
    val = ops.L2Reg.apply(plan, None, 0, *tensors)
    want = sum(torch.sum(c * torch.square(t.detach().double())) for c, t in zip(coeffs, tensors))
    assert abs(val.item() - want.item()) <= 2e-6 * abs(want.item())
    (val * 3.0).sum().backward()
    for c, t in zip(coeffs, tensors):
        close(t.grad, (2 * c * 3.0 * t.detach()).cpu().numpy(), rtol=1e-6, atol=0)
    # deterministic: same bits on a second evaluation
    assert ops.L2Reg.apply(plan, None, 0, *tensors).item() == val.item()


def test_train_on_batch_matches_unfused_sequence():
    """The model's own step hands the tables' L2 gradient to the gather's backward (deferred path);
    the gradients must equal those of the plain loss + reg sequence the reference runs."""
    dev = _dev()
    g = load_golden("model_sum_small")
    B = int(g["B"])
    X, y = T(g["X"]).to(dev), T(g["y"]).to(dev)
    grads = []
    for fused in (False, True):
        model = _build_model(g, dev)
        model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
        model.compile(torch.optim.SGD(model.parameters(), lr=0.0), "binary_crossentropy")
        model.train()
        if fused:
            model.train_on_batch(X[:B], y[:B])
        else:
            yp = model(X[:B]).squeeze()
            model.optim.zero_grad()
            (torch.nn.functional.binary_cross_entropy(yp, y[:B].squeeze(), reduction="sum")
             + model.get_regularization_loss() + model.aux_loss).backward()
        grads.append({k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters()})
    for k in grads[0]:
        gclose(grads[1][k], grads[0][k], k)
        gclose(grads[1][k], g["g:" + k], "vs reference " + k)


@pytest.mark.parametrize("variant,B,m,D,ls,heads,ln,res,nl", [
    ("attn", 5, 26, 16, (64, 48), 4, True, True, 1),       # S = 80
    ("attn", 3, 7, 8, (40, 24), 4, False, True, 1),
    ("attn_v2", 4, 22, 16, (48, 40), 2, True, False, 2),
    ("attn", 2, 26, 16, (256, 128, 128), 4, True, True, 1),  # BASELINE config-3 token count S = 320
    ("attn_v2", 3, 9, 32, (24, 20), 8, True, True, 1),
    ("attn", 3, 6, 10, (12, 10), 4, True, True, 1),          # 10 % 4 != 0 -> 2 heads
])
def test_attention_kernel_vs_float64_oracle(variant, B, m, D, ls, heads, ln, res, nl):
    """K5 forward/backward against the oracle evaluated in float64 (the attention gradients suffer
    cancellation, so the yardstick is the exact value, with a tolerance scaled to each tensor)."""
    from deepctr.layers import CINAttention, CINAttentionV2
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    torch.manual_seed(B + m + D)
    if variant == "attn":
        layer = CINAttention(m, D, ls, "relu", True, heads, 0.0, ln, res, 0.0, 1024, "cpu")
    else:
        layer = CINAttentionV2(m, D, ls, "relu", True, heads, 0.0, ln, res, nl, 0.0, 1024, "cpu")
    with torch.no_grad():
        for k, p in layer.named_parameters():
            if "layer_norm" in k or k.endswith("attention.0.bias"):
                p.add_(0.3 * torch.randn(p.shape))
    x = torch.randn(B, m, D) * 0.7
    spec = orc.Spec(["f%d" % i for i in range(m)], [1] * m, [], D, tuple(ls), True, "relu", (), variant, heads, ln,
                    res, nl)
    st64 = {"cin." + k: p.detach().double().requires_grad_(True) for k, p in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    want = orc.cin_attention_forward(x64, st64, "cin.", spec)
    gout = torch.randn(want.shape)
    (want * gout.double()).sum().backward()
    layer = layer.to(dev)
    xg = x.to(dev).requires_grad_(True)
    out = layer(xg)
    wn = want.detach().numpy()
    close(out, wn, rtol=1e-4, atol=1e-5 * float(np.abs(wn).max()) + 1e-7, msg="out")
    (out * gout.to(dev)).sum().backward()

    def scaled(got, ref, name):
        ref = ref.numpy()
        close(got, ref, rtol=2e-3, atol=2e-3 * float(np.abs(ref).max()) + 5e-6, msg=name)   # 5e-6: fp32 noise floor where the exact gradient vanishes
    scaled(xg.grad, x64.grad, "dx")
    for k, p in layer.named_parameters():
        scaled(p.grad, st64["cin." + k].grad, k)


@pytest.mark.parametrize("variant,p_drop", [("attn", 0.0), ("attn_v2", 0.0), ("attn", 0.2)])
def test_full_size_attention_rows_vs_oracle_subset(variant, p_drop):
    """K5 at BASELINE config 3's full size (B=4096, m=26, D=16, cin=(256,128,128) -> S=320 tokens, 4 heads; the
    2048-workgroup grid-stride path of the backward).  Examples are independent: 24 rows of the full launch are
    compared with the float64 oracle on just those rows; with a gout that is zero outside the subset the parameter
    gradients of the full batch equal the oracle's on the subset (linearity), and untouched examples get exactly 0."""
    from deepctr.layers import CINAttention, CINAttentionV2
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import ops
    dev = _dev()
    B, m, D, ls, heads, nl = 4096, 26, 16, (256, 128, 128), 4, (2 if variant == "attn_v2" else 1)
    torch.manual_seed(17)
    if variant == "attn":
        layer = CINAttention(m, D, ls, "relu", True, heads, p_drop, True, True, 0.0, 1024, "cpu")
    else:
        layer = CINAttentionV2(m, D, ls, "relu", True, heads, p_drop, True, True, nl, 0.0, 1024, "cpu")
    with torch.no_grad():
        for k, p in layer.named_parameters():
            if "layer_norm" in k or k.endswith("attention.0.bias"):
                p.add_(0.3 * torch.randn(p.shape))
    x = torch.randn(B, m, D) * 0.5
    rows = torch.randperm(B)[:24]
    rows[0], rows[1] = 0, B - 1
    spec = orc.Spec(["f%d" % i for i in range(m)], [1] * m, [], D, ls, True, "relu", (), variant, heads, True, True, nl)
    params = {k: p.detach().clone() for k, p in layer.named_parameters()}
    layer = layer.to(dev).train()
    xg = x.to(dev).requires_grad_(True)
    out = layer(xg)
    keep = None
    if p_drop > 0:
        S = sum(h // 2 for h in ls[:-1]) + ls[-1]
        keep = _attn_keep_mask(B, S, heads, nl, p_drop, ops.AttnPool.last_drop_seed, dev)[:, rows.to(dev)].cpu()
    st64 = {"cin." + k: p.double().requires_grad_(True) for k, p in params.items()}
    xs = x[rows].double().requires_grad_(True)
    want = orc.cin_attention_forward(xs, st64, "cin.", spec, keep=keep, p_drop=p_drop)
    gsub = torch.randn(want.shape)
    (want * gsub.double()).sum().backward()
    wn = want.detach().numpy()
    close(out[rows.to(dev)], wn, rtol=1e-4, atol=1e-5 * float(np.abs(wn).max()) + 1e-7, msg="out rows")
    gout = torch.zeros(B, want.shape[1])
    gout[rows] = gsub
    (out * gout.to(dev)).sum().backward()

    def scaled(got, ref, name):
        ref = ref.numpy()
        close(got, ref, rtol=2e-3, atol=2e-3 * float(np.abs(ref).max()) + 5e-6, msg=name)
    scaled(xg.grad[rows.to(dev)], xs.grad, "dx rows")
    mask = torch.ones(B, dtype=torch.bool)
    mask[rows] = False
    assert float(xg.grad[mask.to(dev)].abs().max()) == 0.0
    for k, p in layer.named_parameters():
        scaled(p.grad, st64["cin." + k].grad, k)


def _attn_keep_mask(B, S, nh, n_layers, p_drop, seed, dev):
    """The keep bits K5 generates for `seed` (device int64 scalar), through the C ABI: [n_layers, B, nh, S, S] uint8."""
    from xdfm_amd import _lib
    lib = _lib.load()
    keep = torch.empty((n_layers, B, nh, S, S), dtype=torch.uint8, device=dev)
    _lib.check(lib.xdfm_cin_attn_dropout_mask(B, S, nh, n_layers, float(p_drop), seed.data_ptr(), keep.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "mask")
    torch.cuda.synchronize()
    return keep


@pytest.mark.parametrize("variant,B,m,D,ls,heads,ln,res,nl,p_drop", [
    ("attn", 5, 26, 16, (64, 48), 4, True, True, 1, 0.3),
    ("attn_v2", 4, 22, 16, (48, 40), 2, True, False, 2, 0.5),
    ("attn", 2, 26, 16, (256, 128, 128), 4, True, True, 1, 0.1),   # S = 320
    ("attn_v2", 3, 9, 32, (24, 20), 8, True, True, 2, 0.25),
    ("attn", 3, 6, 10, (12, 10), 4, False, True, 1, 0.9),
])
def test_attention_dropout_forward_and_backward_use_one_mask(variant, B, m, D, ls, heads, ln, res, nl, p_drop):
    """cin_attn_dropout > 0 in training mode (cin_attention.py:86).  K5 stores no mask: forward and both backward passes
    regenerate it from (seed, example, layer, head, query, key).  The mask K5 used is read back through
    xdfm_cin_attn_dropout_mask and handed to the float64 oracle, which applies it where the reference applies
    nn.Dropout: output, dx and every parameter gradient must agree -- which they only do when the three passes of the
    kernel see the SAME bits.  (The bit stream itself is not torch's Philox stream: like the reference on CPU vs CUDA,
    the draw matches in distribution only; see test_attention_dropout_mask_statistics.)"""
    from deepctr.layers import CINAttention, CINAttentionV2
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import ops
    dev = _dev()
    torch.manual_seed(B + m + D)
    if variant == "attn":
        layer = CINAttention(m, D, ls, "relu", True, heads, p_drop, ln, res, 0.0, 1024, "cpu")
        nl = 1
    else:
        layer = CINAttentionV2(m, D, ls, "relu", True, heads, p_drop, ln, res, nl, 0.0, 1024, "cpu")
    with torch.no_grad():
        for k, p in layer.named_parameters():
            if "layer_norm" in k or k.endswith("attention.0.bias"):
                p.add_(0.3 * torch.randn(p.shape))
    x = torch.randn(B, m, D) * 0.7
    spec = orc.Spec(["f%d" % i for i in range(m)], [1] * m, [], D, tuple(ls), True, "relu", (), variant, heads, ln,
                    res, nl)
    params = {k: p.detach().clone() for k, p in layer.named_parameters()}
    layer = layer.to(dev).train()
    xg = x.to(dev).requires_grad_(True)
    out = layer(xg)
    seed = ops.AttnPool.last_drop_seed
    assert seed is not None
    S = sum(h // 2 for h in ls[:-1]) + ls[-1]
    nh = orc.valid_num_heads(D, heads)
    keep = _attn_keep_mask(B, S, nh, nl, p_drop, seed, dev).cpu()
    st64 = {"cin." + k: p.double().requires_grad_(True) for k, p in params.items()}
    x64 = x.double().requires_grad_(True)
    want = orc.cin_attention_forward(x64, st64, "cin.", spec, keep=keep, p_drop=p_drop)
    gout = torch.randn(want.shape)
    (want * gout.double()).sum().backward()
    wn = want.detach().numpy()
    close(out, wn, rtol=1e-4, atol=1e-5 * float(np.abs(wn).max()) + 1e-7, msg="out")
    (out * gout.to(dev)).sum().backward()

    def scaled(got, ref, name):
        ref = ref.numpy()
        close(got, ref, rtol=2e-3, atol=2e-3 * float(np.abs(ref).max()) + 5e-6, msg=name)
    scaled(xg.grad, x64.grad, "dx")
    for k, p in layer.named_parameters():
        scaled(p.grad, st64["cin." + k].grad, k)
    # evaluation mode ignores the rate (nn.Dropout is the identity under .eval())
    layer.eval()
    with torch.no_grad():
        ev = layer(x.to(dev))
    want_eval = orc.cin_attention_forward(x.double(), {k: v.detach() for k, v in st64.items()}, "cin.", spec).numpy()
    close(ev, want_eval, rtol=1e-4, atol=1e-5 * float(np.abs(want_eval).max()) + 1e-7, msg="eval")


def test_attention_dropout_mask_statistics():
    """The keep bits behave like nn.Dropout's Bernoulli(1-p) draw: rate within 5 sigma for every (layer, head) plane,
    no correlation between planes / examples / neighbouring keys, a new mask for a new seed, the same mask for the same
    seed; and the model draws a different seed on every call while torch.manual_seed repeats a run."""
    dev = _dev()
    B, S, nh, L = 64, 80, 4, 2
    for p_drop in (0.1, 0.5, 0.8):
        s1 = torch.tensor([1234567891011], dtype=torch.int64, device=dev)
        s2 = torch.tensor([1234567891012], dtype=torch.int64, device=dev)
        k1 = _attn_keep_mask(B, S, nh, L, p_drop, s1, dev)
        assert torch.equal(k1, _attn_keep_mask(B, S, nh, L, p_drop, s1, dev))
        k2 = _attn_keep_mask(B, S, nh, L, p_drop, s2, dev)
        a = k1.double().cpu().numpy()
        b = k2.double().cpu().numpy()
        q = 1.0 - p_drop
        n_plane = B * S * S
        rates = a.mean(axis=(1, 3, 4))                                      # [L, nh]
        assert np.all(np.abs(rates - q) < 5 * np.sqrt(q * p_drop / n_plane)), (p_drop, rates)
        per_example = a.mean(axis=(0, 2, 3, 4))
        assert np.all(np.abs(per_example - q) < 5 * np.sqrt(q * p_drop / (L * nh * S * S)))

        def corr(u, v):
            u = u.ravel() - u.mean()
            v = v.ravel() - v.mean()
            return float((u * v).mean() / np.sqrt((u * u).mean() * (v * v).mean()))
        n = a[0, :, 0].size
        lim = 5.0 / np.sqrt(n)
        assert abs(corr(a[0, :, 0], a[0, :, 1])) < lim                       # heads
        assert abs(corr(a[0, :, 0], a[1, :, 0])) < lim                       # layers
        assert abs(corr(a[0, :B // 2], a[0, B // 2:])) < 5.0 / np.sqrt(a[0, :B // 2].size)   # examples
        assert abs(corr(a[..., :-1], a[..., 1:])) < 5.0 / np.sqrt(a[..., 1:].size)      # neighbouring keys
        assert abs(corr(a[..., :-1, :], a[..., 1:, :])) < 5.0 / np.sqrt(a[..., 1:, :].size)  # neighbouring queries
        assert abs(corr(a, b)) < 5.0 / np.sqrt(a.size)                       # seeds
    from deepctr.layers import CINAttention
    from xdfm_amd import ops
    torch.manual_seed(3)
    layer = CINAttention(6, 8, (12, 10), "relu", True, 2, 0.4, True, True, 0.0, 1024, "cpu").to(dev).train()
    x = torch.randn(4, 6, 8, device=dev)
    torch.manual_seed(77)
    o1 = layer(x)
    sd1 = int(ops.AttnPool.last_drop_seed.item())
    o2 = layer(x)
    sd2 = int(ops.AttnPool.last_drop_seed.item())
    assert sd1 != sd2 and not torch.equal(o1, o2)
    torch.manual_seed(77)
    o3 = layer(x)
    assert int(ops.AttnPool.last_drop_seed.item()) == sd1 and torch.equal(o1, o3)


def test_full_size_logloss_auc_vs_cpu_path():
    """North-star check at BASELINE config-2 size: one 4096-row synthetic Criteo batch, identical weights,
    predictions of the HIP path vs the CPU oracle -> logloss and AUC must agree within 1e-5."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import metrics as M
    dev = _dev()
    vocab, nd, D, B = [3000] * 26, 13, 16, 4096
    names = ["C%d" % (i + 1) for i in range(26)]
    dnames = ["I%d" % (i + 1) for i in range(nd)]
    cols = [SparseFeat(n, v, D) for n, v in zip(names, vocab)] + [DenseFeat(n, 1) for n in dnames]
    model = xDeepFM(cols, cols, cin_layer_size=(256, 128, 128), dnn_hidden_units=(256, 256), device=dev)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():                      # lively weights so that the predictions spread over (0, 1)
        for k, p in model.named_parameters():
            if "embedding_dict" in k or "dnn" in k or k in ("linear_model.weight", "cin_linear.weight"):
                p.copy_((0.2 * torch.randn(p.shape, generator=g)).to(dev))
    X, y = orc.synthetic_batch(B, vocab, nd, seed=2025)
    pred = model.predict({n: X[:, i] for i, n in enumerate(names + dnames)}, batch_size=B)
    spec = orc.Spec(names, vocab, dnames, D, (256, 128, 128), True, "relu", (256, 256))
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want = orc.model_forward(T(X), state, spec).numpy().astype("float64")
    assert 0.02 < want.std()                                        # a non-degenerate batch
    assert abs(M.log_loss(y, pred) - M.log_loss(y, want)) < 1e-5
    assert abs(M.roc_auc_score(y, pred) - M.roc_auc_score(y, want)) < 1e-5
    np.testing.assert_allclose(pred, want, rtol=1e-4, atol=2e-6)


def test_graph_replay_of_train_step_matches_eager_launches():
    """xdfm_amd/graphstep.py: from the third step on the train step is replayed from a captured HIP graph.
    Same seed, same batches: the replayed run must follow the eager run, the captured graph must hold no memset
    node, and a change of the learning rate must be FOLLOWED by the same graph (K7 reads the rate from a device
    scalar, TableAdam.sync_lr) instead of forcing a new capture per value (a schedule would thrash the cache)."""
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import graphstep
    dev = _dev()
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]

    def run(use_graph):
        model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev)
        model.compile("adam", "binary_crossentropy", metrics=[])
        model.train()
        step = graphstep.GraphedStep(model)
        step.disabled = not use_graph
        model.__dict__["_graphed_step"] = step
        losses = []
        for s in range(14):
            if s == 9:
                for pg in model.optim.param_groups:
                    pg["lr"] = 3e-3
            X, y = orc.synthetic_batch(256 if s != 6 else 100, vocab, nd, seed=100 + s)     # one ragged batch
            out = model.train_on_batch(T(X).to(dev), T(y).to(dev))
            losses.append(float(out[2].detach().reshape(-1)[0]))
        return model, step, losses

    m_g, step_g, l_g = run(True)
    m_e, step_e, l_e = run(False)
    assert step_e.replays == 0 and step_g.replays >= 6, (step_g.replays, step_g.disabled)
    assert not step_g.disabled
    graphs = [e for e in step_g.entries.values() if e.graph is not None]
    assert len(graphs) == 1                                   # batch 256: ONE graph serves lr 1e-3 and lr 3e-3
    for e in graphs:
        n, n_memset, n_other = graphstep.census(e.graph)
        assert n > 20 and n_memset == 0 and n_other == 0
    np.testing.assert_allclose(l_g, l_e, rtol=2e-5)
    for (k, a), (_, b) in zip(m_g.state_dict().items(), m_e.state_dict().items()):
        close(a, b.cpu().numpy(), rtol=2e-3, atol=2e-6, msg=k)


def test_marked_gradients_skip_untouched_rows_bit_exactly():
    """xdfm_embed_scatter_bwd_marked + xdfm_adam_tensor.grad_marks: the scatter marks the 16-byte
    chunks of the flat gradient buffer it adds to; K7 given the marks must produce the very same parameters and
    moments as K7 reading the full dense gradient (bit-exact: same arithmetic, zeros not read instead of read), and
    must leave the gradient buffer and the marks all zero.  Through the C ABI."""
    import ctypes
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    m, D, nd, B = 5, 12, 3, 333
    vocab = [97, 1000, 13, 4096, 50]
    X = torch.cat([torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocab], 1).float(),
                   torch.rand(B, nd, generator=g)], 1).to(dev)
    sizes = [v * D for v in vocab] + list(vocab) + [nd]
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4
    total = off
    flat = torch.zeros(total, device=dev)
    marks = torch.zeros(total // 4 + 2, dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    cols, voc, dcols = torch.arange(m, **i32), torch.tensor(vocab, **i32), torch.arange(m, m + nd, **i32)
    off_dev = torch.tensor(offs[:2 * m], dtype=torch.int64, device=dev)
    d_emb = torch.randn(m, B * D, generator=g).to(dev)
    d_dnn = torch.randn(B, m * D + nd, generator=g).to(dev)
    d_lin = torch.randn(B, generator=g).to(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_w = flat[offs[-1]:offs[-1] + nd]
    # the strided form the row-parallel exchange uses: one buffer whose rows hold [d_dnn row | X row | d_lin]
    packed = torch.cat([d_dnn, X, d_lin.view(B, 1)], 1).contiguous()
    W_ = packed.shape[1]
    Pv = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.xdfm_embed_scatter_bwd_marked(Pv(packed[:, m * D + nd:]), W_, B, P(cols), P(voc), m, D, P(dcols), nd,
                                                 P(d_emb), Pv(packed), W_, Pv(packed[:, W_ - 1]), W_, P(flat),
                                                 P(off_dev[:m]), P(off_dev[m:]), P(d_w), P(marks), st), "scatter marked")
    plain = torch.zeros_like(flat)
    _lib.check(lib.xdfm_embed_scatter_bwd(P(X), X.stride(0), B, P(cols), P(voc), m, D, P(dcols), nd, P(d_emb), P(d_dnn),
                                          P(d_lin), P(plain), P(off_dev[:m]), P(off_dev[m:]),
                                          P(plain[offs[-1]:offs[-1] + nd]), st), "scatter")
    close(flat, plain.cpu().numpy(), rtol=1e-4, atol=3e-5)            # same sums (atomics order differs)
    chunk_nonzero = (flat.view(-1, 4) != 0).any(1)
    mk = marks[:total // 4].bool()
    assert bool((mk | ~chunk_nonzero).all())                          # every chunk that holds a gradient is marked
    touched_rows = sum(len(set(X[:, j].long().tolist())) for j in range(m))
    assert int(mk.sum()) <= touched_rows * (D // 4 + 1) + nd          # ... and only chunks of touched rows are

    # K7 over the same gradients: marked (sparse read) against unmarked (dense read) descriptors
    T_ = len(sizes)
    torch.manual_seed(5)
    pa = [torch.randn(n, device=dev) * 0.05 for n in sizes]
    ma = [torch.randn(n, device=dev) * 0.01 for n in sizes]
    va = [torch.rand(n, device=dev) * 1e-4 for n in sizes]
    pb, mb, vb = [t.clone() for t in pa], [t.clone() for t in ma], [t.clone() for t in va]
    step = torch.full((1,), 3.0, device=dev)
    dense_g, before = flat.clone(), flat.clone()

    def run(ps, ms, vs, gbuf, mark_buf):
        arr = (_lib.AdamTensor * T_)()
        for k in range(T_):
            arr[k].param, arr[k].exp_avg, arr[k].exp_avg_sq = ps[k].data_ptr(), ms[k].data_ptr(), vs[k].data_ptr()
            arr[k].grad = gbuf.data_ptr() + 4 * offs[k]
            arr[k].step, arr[k].numel, arr[k].l2 = step.data_ptr(), sizes[k], 1e-4 if k < m else 0.0
            arr[k].grad_marks = (mark_buf.data_ptr() + offs[k] // 4) if mark_buf is not None else None
        ws = torch.empty(lib.xdfm_adam_step_ws_elems(T_), device=dev)
        val = torch.empty(1, device=dev)
        _lib.check(lib.xdfm_adam_step(ctypes.cast(arr, ctypes.c_void_p), T_, 1e-3, 0.9, 0.999, 1e-8, P(ws), P(val), st), "adam")
        return val

    v_sparse = run(pa, ma, va, flat, marks)
    v_dense = run(pb, mb, vb, dense_g, None)
    torch.cuda.synchronize()
    assert float(v_sparse) == float(v_dense)
    bad = [(k, nm, int((a[k] != b[k]).sum()), float((a[k] - b[k]).abs().max()), (a[k] != b[k]).nonzero()[:6].flatten().tolist())
           for k in range(T_) for nm, a, b in (("p", pa, pb), ("m", ma, mb), ("v", va, vb)) if not torch.equal(a[k], b[k])]
    assert not bad, bad
    assert float(flat.abs().max()) == 0.0 and int(marks.max()) == 0
    assert torch.equal(dense_g, before)                               # the dense read leaves g alone


def test_train_step_keeps_table_gradients_clean_without_table_sized_fills():
    """The model's own train step (eager and graph-replayed) on the kept gradient buffer (ops.GradArena): same
    losses and parameters as with a fresh zero-filled buffer per step (XDFM_GRAD_ARENA=0), never the slow full
    clear, and buffer + marks all zero after every step."""
    _needs_default_env('graph')
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]

    def run(arena):
        os.environ["XDFM_GRAD_ARENA"] = "1" if arena else "0"
        try:
            model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev)
            model.compile("adam", "binary_crossentropy", metrics=[])
            model.train()
            losses = []
            for s in range(9):
                X, y = orc.synthetic_batch(256 if s != 4 else 100, vocab, nd, seed=300 + s)
                out = model.train_on_batch(T(X).to(dev), T(y).to(dev))
                losses.append(float(out[2].detach().reshape(-1)[0]))
                for a in model._plan.arenas():
                    assert not a.pending and a.full_clears == 0
                    assert float(a.flat.abs().max()) == 0.0 and int(a.marks.max()) == 0
            return model, losses
        finally:
            os.environ.pop("XDFM_GRAD_ARENA", None)

    m_a, l_a = run(True)
    m_z, l_z = run(False)
    assert len(m_a._plan.arenas()) == 1 and len(m_z._plan.arenas()) == 0
    assert m_a.__dict__["_graphed_step"].replays >= 3
    np.testing.assert_allclose(l_a, l_z, rtol=2e-5)
    for (k, a), (_, b) in zip(m_a.state_dict().items(), m_z.state_dict().items()):
        close(a, b.cpu().numpy(), rtol=2e-3, atol=2e-6, msg=k)


def test_dense_relu_matches_linear_plus_relu():
    """ops.DenseReLU (ReLU in the GEMM epilogue, mask + bias gradient in xdfm_relu_bwd_colsum) against
    relu(F.linear) with autograd (deepctr/layers/core.py:120-134), incl. a ragged row count and zeros in y."""
    from xdfm_amd import ops
    dev = _dev()
    torch.manual_seed(2)
    for rows, k, n in ((4096, 429, 256), (100, 37, 70), (1, 8, 5)):
        x = torch.randn(rows, k, device=dev)
        W = torch.randn(n, k, device=dev) * 0.1
        b = torch.randn(n, device=dev) * 0.1
        g = torch.randn(rows, n, device=dev)
        a = [t.clone().requires_grad_(True) for t in (x, W, b)]
        r = [t.clone().double().requires_grad_(True) for t in (x, W, b)]
        ya = ops.dense_relu(*a)
        yr = torch.relu(torch.nn.functional.linear(*r))
        ya.backward(g)
        yr.backward(g.double())
        close(ya, yr.detach().cpu().numpy(), rtol=2e-5, atol=2e-5)
        live = (yr.detach().abs() > 1e-4) | (yr.detach() == 0)          # away from the ReLU kink
        assert bool(((ya.detach() > 0) == (yr.detach() > 0))[live].all())
        for u, v, name in zip(a, r, "xWb"):
            close(u.grad, v.grad.cpu().numpy(), rtol=2e-4, atol=2e-4 * float(v.grad.abs().max()), msg=name)


def test_user_driven_loop_gets_plain_dense_table_gradients():
    """The kept gradient buffer is an internal of the model's own train step.  Code that drives autograd itself --
    here: two backward passes over different batches accumulated without zero_grad, then an edit of .grad -- must
    see ordinary dense gradients (not views of the kept buffer) so that TableAdam.step() honours everything such
    code put into them."""
    import torch.nn.functional as F
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    dev = _dev()
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-5, device=dev)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    batches = [orc.synthetic_batch(128, vocab, nd, seed=700 + s) for s in range(3)]
    X0, y0 = batches[0]
    model.train_on_batch(T(X0).to(dev), T(y0).to(dev))            # own step: the kept buffer is in use and clean again
    arena, = model._plan.arenas()
    assert not arena.pending and not model._plan.arena_on
    lo, hi = arena.base, arena.base + arena.nbytes

    def backward(k):
        X, y = batches[k]
        pred = model(T(X).to(dev))
        F.binary_cross_entropy(pred.squeeze(), T(y).to(dev).squeeze(), reduction="sum").backward()

    tables = [model.embedding_dict["C%d" % (i + 1)].weight for i in range(len(vocab))]
    single = []
    for k in (1, 2):
        model.optim.zero_grad()
        backward(k)
        assert all(not (lo <= t.grad.data_ptr() < hi) for t in tables) and not arena.pending
        single.append([t.grad.clone() for t in tables])
    model.optim.zero_grad()
    backward(1)
    backward(2)                                                   # accumulates into the existing .grad
    for t, a, b in zip(tables, single[0], single[1]):
        close(t.grad, (a + b).cpu().numpy(), rtol=1e-4, atol=1e-6)
    before = [t.detach().clone() for t in tables]
    for t in tables:
        t.grad.add_(1e-3)                                         # e.g. a hand-written regulariser: touches EVERY row
    model.optim.step()
    for t, b in zip(tables, before):
        assert bool(((t.detach() - b).abs() > 0).all())           # every row moved: nothing was skipped by marks
    assert not arena.pending and float(arena.flat.abs().max()) == 0.0


def test_table_adam_kernel_matches_torch_adam():
    """K7 (xdfm_adam_step) behind xdfm_amd.optim.TableAdam against torch.optim.Adam(fused=True): same state
    layout and, over 6 steps with fresh dense gradients, the same parameters / moments to fp32 rounding, with
    the armed L2 term equal to adding 2*l2*w to the gradients by hand.  Gradients are views of one flat buffer
    at odd offsets, as the gather's backward produces them."""
    from xdfm_amd.optim import TableAdam
    dev = _dev()
    torch.manual_seed(3)
    shapes = [(70001, 16), (100000, 1), (65536, 3), (300, 7), (11,)]          # three large (one odd-sized), two small
    init = [torch.randn(s, device=dev) * 0.05 for s in shapes]
    pa = [torch.nn.Parameter(t.clone()) for t in init]
    pb = [torch.nn.Parameter(t.clone()) for t in init]
    oa = TableAdam(pa, lr=2e-3)
    ob = torch.optim.Adam(pb, lr=2e-3, fused=True)
    l2 = [1e-3, 0.0, 5e-2]
    sizes = [p.numel() for p in pa]
    for step in range(6):
        flat = torch.randn(sum(sizes) + 8, device=dev) * (0.1 if step % 2 else 1e-3)
        flat[::7] = 0.0                                                       # rows without a data gradient
        off = 4                                                               # 16-byte aligned start
        for p, q, n in zip(pa, pb, sizes):
            p.grad = flat[off:off + n].view(p.shape)
            q.grad = flat[off:off + n].view(p.shape).clone()
            off += n
        if step % 2:                   # every other step with the L2 term armed: K7 adds 2*l2*w and returns the value
            oa.arm_l2(pa[:3], l2)
            want_value = sum(c * float((q.detach().double() ** 2).sum()) for q, c in zip(pb[:3], l2))
            for q, c in zip(pb[:3], l2):
                q.grad.add_(q.detach(), alpha=2 * c)
        oa.step()
        ob.step()
        if step % 2:
            assert abs(float(oa.l2_value) - want_value) <= 1e-5 * want_value
        else:
            assert oa.l2_value is None
    for i, (p, q) in enumerate(zip(pa, pb)):
        close(p, q.detach().cpu().numpy(), rtol=2e-6, atol=1e-8, msg="param %d" % i)
        sa, sb = oa.state[p], ob.state[q]
        assert sorted(sa.keys()) == sorted(sb.keys()) and float(sa["step"]) == float(sb["step"]) == 6.0
        close(sa["exp_avg"], sb["exp_avg"].cpu().numpy(), rtol=2e-6, atol=2e-8, msg="exp_avg %d" % i)
        close(sa["exp_avg_sq"], sb["exp_avg_sq"].cpu().numpy(), rtol=2e-6, atol=1e-10, msg="exp_avg_sq %d" % i)
    # state_dict round trip into a stock Adam
    oc = torch.optim.Adam([torch.nn.Parameter(t.clone()) for t in init], lr=2e-3, fused=True)
    oc.load_state_dict(oa.state_dict())
