"""GPU tests (-m gpu) of every fp32-MFMA (cin_math 0, v_mfma_f32_32x32x2_f32) template instance of the CIN contraction
kernels, driven one level at a time through the C ABI and compared with a float64 contraction computed by torch on the
device -- the kernels every level without an f16x3 / bf16 kernel runs in the default mode too:

  forward  xdfm_cin_fwd_pack + xdfm_cin_level_fwd         cin_fwd_kernel<MT, NF>, cin_fwd_mp_kernel<MT, NF, MPT>    act(W @ Z + b)
  dX       xdfm_cin_bwd_pack + xdfm_cin_level_bwd_x_ex    cin_bwd_x_kernel<HS4, JB>                                 autograd of W @ Z
  dW       xdfm_cin_level_bwd_w                           cin_bwd_w_kernel<MT, 2> (v1), cin_bwd_w_dma_kernel<MT, 2>,
                                                          cin_bwd_w_dma4_kernel<4, 2>, slab or atomic epilogue        dOut @ Z^T

Inputs, reference, comparison and the two input families (exact: small integers, every product and partial sum an integer
below 2^24, the result must equal float64 bit for bit -- also with the atomic epilogue, integers add exactly in any order;
normal: Gaussian) are those of tests/test_gpu_cin_instances.py.  Each SWEEP_F32 row names the instance the host must pick in
each direction; the probes last_fwd_f32 / last_bwx_f32 / last_bww_f32 (include/xdfm.h) must report exactly that one and
last_*_kernel 0.  tests/test_cin_f32_coverage.py checks on the CPU that the rows reach every instance the sources build, that
every claim follows from the host rules, and that the exact family's sums stay below 2^24.

Normal family, per element: |got - ref| <= k * mag + 2^-24 |ref|, mag = the same contraction on absolute values, with
k = min(K0, (L + 4) * 2^-24): L is the contraction length of the direction (Hp m forward, H + m dxp, H + Hp dx0, N dW) and
(L + 4) * 2^-24 what any summation order of correctly rounded fp32 products and sums meets, so no row is held to less than
that.  K0 is the smallest power of two at least 4x the worst (|got - ref| - 2^-24 |ref|) / mag measured on the healthy
kernels over the whole sweep (MI355X): K0 = 2^-19, worst 2.84e-7 (the forward of the row m 22, H 256, Hp 3, N 50, dbg 2;
dxp 1.49e-7, dx0 1.86e-7, dW 2.21e-7).  The ceiling is the lower of the two for L <= 28; no row came above its ceiling.

Every dX call and every dW call with bww_slab 1 runs twice and must repeat its bits; dW with bww_slab 0 (float atomics) is
only compared with the reference.  dX runs with XDFM_BWX_SET_DXP | XDFM_BWX_SET_DX0 and accumulating, on outputs filled
with non-zero values beforehand; a level of more than 256 rows takes its dX in calls of 256 rows as the layer does.

Beside the sweep: the error returns of shapes whose LDS need exceeds the workgroup's, xdfm_cin_direct_sum (three kernels)
and xdfm_cin_dout / xdfm_cin_dout_det with act 0 and 1 (cases of tests/cin_sigmoid_cases.py), all against float64.
"""
import numpy as np
import pytest
import torch

from test_gpu_cin_instances import F, K, _compare, _contraction, _dev, _inputs, _options, _p, _same_bits

pytestmark = pytest.mark.gpu

K0 = 2.0 ** -19
K_F16X3 = K[F]

# Probe values (include/xdfm.h):  forward MT * 1000 + NF * 100 + MPT (0: the generic kernel);  dX HS4 * 10 + JB;
# dW n-splits * 1000 + MT * 100 + KV * 10 + slab, KV 1 = v1 (register staging), 2 = dword LDS-DMA, 3 = dwordx4 LDS-DMA.
# fold 1: level 0, x_prev IS x0 (the same tensor).  how: "act" 0 = a linear forward (default ReLU); "off" 1 = the dW operands
# are views that start one float off a 16-byte boundary; "math" 1 = the row runs under the default arithmetic (its unaligned
# dW must fall back to the dword-DMA kernel; forward and dX probes read 0 where an f16x3 kernel exists).
#   m, H, Hp, N, fold, options, how, forward, dX, dW
SWEEP_F32 = [
    # forward tiles by H (MT 1 / 2 / 4 / 8), dX HS4 1 .. 32, dW MT 1 / 2 / 4; generic-kernel edges on the way
    (5, 1, 3, 33, 0, {}, {}, 1100, 11, 2121),                 # Hp m' = 9 k-steps: three dead ones behind the last quad
    (1, 8, 1, 1, 0, {}, {}, 1100, 11, 1121),                  # m = 1, Hp = 1, N = 1
    (7, 13, 32, 31, 0, {}, {}, 1100, 21, 1121),               # odd m: the last j-pair is half zero; a full x_prev chunk
    (4, 20, 33, 127, 0, {}, {}, 1100, 41, 4121),              # Hp = 33: one row behind a refill of the x_prev chunk
    (3, 27, 65, 129, 0, {}, {}, 1100, 41, 5121),
    (6, 32, 6, 256, 1, {}, {}, 1100, 41, 8121),               # level 0
    (9, 33, 5, 130, 0, {}, {}, 2100, 81, 5221),
    (10, 50, 7, 301, 0, {}, {}, 2100, 81, 10221),             # N = 301: dword-DMA, a 13-column tail
    (12, 64, 4, 128, 0, {}, {"act": 0}, 2100, 81, 4221),      # linear: negative outputs are kept
    (8, 65, 9, 200, 0, {}, {}, 4100, 161, 7431),
    (11, 100, 5, 300, 0, {"bww_nsplit": 3}, {}, 4100, 161, 3431),      # n-splits of 128 / 128 / 44 columns
    (3, 224, 2, 97, 0, {}, {}, 4100, 321, 4421),              # MT 4, N % 4 != 0: dword-DMA
    (5, 225, 3, 64, 0, {}, {}, 8100, 321, 2431),
    (4, 256, 33, 40, 0, {}, {}, 8100, 321, 2431),
    (6, 300, 2, 100, 0, {}, {}, 8100, 81, 4431),              # two forward row blocks, 44 live rows in the second (and in the last dX call)
    (50, 128, 2, 36, 0, {}, {}, 4100, 161, 2431),
    (2, 129, 1, 33, 0, {}, {}, 4100, 321, 2421),
    (5, 130, 3, 132, 0, {}, {}, 4100, 321, 5431),             # dW: two h-groups, 2 live rows in the second
    # cin_fwd_mp_kernel: m = 26, 25 (MPT 13), 22, 21 (MPT 11) at MT 4 and MT 8; Hp = 1, 5, 32, 37 for the loop unrolled by 4
    (26, 100, 26, 160, 1, {}, {}, 4113, 161, 5431),
    (26, 100, 5, 70, 0, {}, {}, 4113, 161, 3421),
    (25, 256, 1, 33, 0, {}, {}, 8113, 321, 2421),
    (22, 225, 32, 100, 0, {}, {}, 8111, 321, 4431),
    (21, 65, 37, 45, 0, {}, {}, 4111, 161, 2421),
    (26, 240, 37, 64, 0, {}, {}, 8113, 321, 2431),
    (22, 128, 1, 130, 0, {}, {}, 4111, 161, 5421),
    (25, 100, 32, 50, 0, {}, {}, 4113, 161, 2421),
    (21, 256, 5, 31, 0, {}, {}, 8111, 321, 1421),
    # fwd_nf 2: two column fragments per wave at MT 4 (the second one partial at N = 70), one at every other MT
    (8, 100, 3, 64, 0, {"fwd_nf": 2}, {}, 4200, 161, 2431),
    (7, 65, 4, 70, 0, {"fwd_nf": 2}, {}, 4200, 161, 3421),
    (26, 100, 5, 70, 0, {"fwd_nf": 2}, {}, 4213, 161, 3421),
    (22, 128, 37, 130, 0, {"fwd_nf": 2}, {}, 4211, 161, 5421),
    (21, 100, 2, 130, 0, {"fwd_nf": 2}, {}, 4211, 161, 5421),
    (25, 65, 3, 64, 0, {"fwd_nf": 2}, {}, 4213, 161, 2431),
    (26, 256, 2, 64, 0, {"fwd_nf": 2}, {}, 8113, 321, 2431),
    # dbg 2: the generic kernel at the field counts of the straight-line one
    (26, 100, 3, 50, 0, {"dbg": 2}, {}, 4100, 161, 2421),
    (22, 256, 3, 50, 0, {"dbg": 2}, {}, 8100, 321, 2421),
    (26, 225, 2, 33, 0, {"dbg": 2}, {}, 8100, 321, 2421),
    (22, 65, 5, 40, 0, {"dbg": 2}, {}, 4100, 161, 2431),
    (26, 100, 2, 70, 0, {"dbg": 2, "fwd_nf": 2}, {}, 4200, 161, 3421),
    # dbg 32: two interleaved dX chains per wave (even m, HS4 4 / 8 / 16); one chain with an odd m or another HS4
    (6, 27, 3, 33, 0, {"dbg": 32}, {}, 1100, 42, 2121),
    (6, 32, 6, 70, 1, {"dbg": 32}, {}, 1100, 42, 3121),
    (8, 50, 33, 127, 0, {"dbg": 32}, {}, 2100, 82, 4221),
    (26, 100, 2, 130, 0, {"dbg": 32}, {}, 4113, 162, 5421),
    (50, 128, 1, 31, 0, {"dbg": 32}, {}, 4100, 162, 1421),
    (7, 64, 3, 31, 0, {"dbg": 32}, {}, 2100, 81, 1221),
    (4, 256, 2, 33, 0, {"dbg": 32}, {}, 8100, 321, 2421),
    (4, 13, 2, 33, 0, {"dbg": 32}, {}, 1100, 21, 2121),
    # dW: bww_mt, the dword-DMA kernel at MT 4 (dbg 16, unaligned operands), v1 (dbg 8, atomics only)
    (4, 100, 3, 96, 0, {"bww_mt": 1}, {}, 4100, 161, 3121),
    (4, 100, 3, 96, 0, {"bww_mt": 2}, {}, 4100, 161, 3221),
    (4, 100, 3, 100, 0, {"bww_mt": 4}, {}, 4100, 161, 4431),
    (4, 20, 3, 64, 0, {"bww_mt": 4}, {}, 1100, 41, 2431),
    (6, 100, 3, 128, 0, {"dbg": 16}, {}, 4100, 161, 4421),
    (6, 100, 5, 128, 0, {}, {"off": 1}, 4100, 161, 4421),
    (5, 100, 3, 77, 0, {"dbg": 8, "bww_slab": 0}, {}, 4100, 161, 3410),
    (3, 20, 2, 40, 0, {"dbg": 8, "bww_slab": 0}, {}, 1100, 41, 2110),
    (3, 50, 33, 33, 0, {"dbg": 8, "bww_slab": 0}, {}, 2100, 81, 2210),
    # dW n-splits: forced, the default at N = 1000 (32 splits, the last one a tail only), N < 32, and the atomic epilogue
    (5, 100, 3, 200, 0, {"bww_nsplit": 1}, {}, 4100, 161, 1431),
    (4, 100, 3, 1000, 0, {}, {}, 4100, 161, 32431),
    (4, 100, 2, 20, 0, {}, {}, 4100, 161, 1431),
    (6, 50, 2, 28, 0, {}, {}, 2100, 81, 1221),
    (11, 100, 5, 300, 0, {"bww_nsplit": 3, "bww_slab": 0}, {}, 4100, 161, 3430),
    (4, 100, 3, 1000, 0, {"bww_slab": 0}, {}, 4100, 161, 32430),
    (6, 50, 2, 28, 0, {"bww_slab": 0}, {}, 2100, 81, 1220),
    (3, 100, 33, 301, 0, {"bww_slab": 0}, {}, 4100, 161, 10420),
    # the default arithmetic on unaligned dW operands: the f16x3 dX kernel, the fp32 forward (odd m) and dword-DMA dW
    (7, 100, 3, 128, 0, {}, {"math": 1, "off": 1}, 4100, 0, 4421),
]


def _row_id(r):
    extra = "".join("-%s%d" % (k, v) for d in (r[5], r[6]) for k, v in sorted(d.items()))
    return "m%d-H%d-Hp%d-N%d-l0%d%s" % (r[0], r[1], r[2], r[3], r[4], extra)


def _off_view(t):
    """a copy of t that starts one float behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _ceiling(L):
    return (L + 4) * 2.0 ** -24


def run_row_f32(row, family, k0=K0):
    """All three directions of one SWEEP_F32 row; returns {tensor: worst (|got - ref| - 2^-24 |ref|) / mag} (normal family)."""
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    m, H, Hp, N, fold, opts, how, want_fwd, want_bwx, want_bww = row
    math, act = how.get("math", 0), how.get("act", 1)
    seed = ((m * 1009 + H) * 1009 + Hp) * 100003 + N * 3 + fold + 5
    W, bias, xp, x0, dOut, pre_p, pre_0 = _inputs(m, H, Hp, N, fold, family, seed, dev)
    out_r, dxp_r, dx0_r, dW_r = _contraction(W, bias, xp, x0, dOut)
    if family == "normal":
        out_m, dxp_m, dx0_m, dW_m = _contraction(W.abs(), bias.abs(), xp.abs(), x0.abs(), dOut.abs())
    else:
        out_m = dxp_m = dx0_m = dW_m = None
    k_out, k_dxp, k_dx0, k_dW = (min(k0, _ceiling(L)) for L in (Hp * m, H + m, H + Hp, N))
    ratios = {}
    probes = {"last_fwd_f32": -1, "last_bwx_f32": -1, "last_bww_f32": -1, "last_fwd_inst": -1, "last_bwx_inst": -1, "last_bww_inst": -1}
    with _options(cin_math=math, **probes, **opts):
        # ---- forward
        pack = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_cin_fwd_pack(_p(W), H, Hp, m, _p(pack), st), "cin_fwd_pack")
        out = torch.full((H, N), 7.0, device=dev)
        _lib.check(lib.xdfm_cin_level_fwd(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, act, _p(out), st), "cin_level_fwd")
        assert _lib.get_option("last_fwd_f32") == want_fwd
        assert _lib.get_option("last_fwd_kernel") == (0 if want_fwd else math)
        assert want_fwd == 0 or _lib.get_option("last_fwd_inst") == 0
        ratios["out"] = _compare(out, torch.relu(out_r) if act == 1 else out_r, out_m, family, k_out, "out")
        if act == 0:
            assert bool((out < 0).any()), "a linear level must keep its negative outputs"

        # ---- dX: stored (flags 3) and accumulated (flags 0) onto non-zero prefills, each twice; at most 256 rows per call
        def bwx(flags):
            dxp, dx0 = pre_p.clone(), pre_0.clone()
            for h0 in range(0, H, 256):
                hc = min(256, H - h0)
                Wc, dOc = (W, dOut) if hc == H else (W[h0:h0 + hc].contiguous(), dOut[h0:h0 + hc].contiguous())
                wz = torch.empty(lib.xdfm_cin_bwd_pack_elems(hc, Hp, m), dtype=torch.float32, device=dev)
                _lib.check(lib.xdfm_cin_bwd_pack(_p(Wc), hc, Hp, m, _p(wz), st), "cin_bwd_pack")
                _lib.check(lib.xdfm_cin_level_bwd_x_ex(_p(dOc), _p(xp), _p(x0), _p(wz), hc, Hp, m, N, _p(dxp), _p(dx0),
                                                       flags if h0 == 0 else 0, st), "cin_level_bwd_x")
            return dxp, dx0

        for flags in (3, 0):
            (dxp, dx0), (dxp2, dx02) = bwx(flags), bwx(flags)
            _same_bits(dxp, dxp2, "dxp")
            _same_bits(dx0, dx02, "dx0")
            base_p, base_0 = (0.0, 0.0) if flags else (pre_p.double(), pre_0.double())
            what = "flags %d: " % flags
            # want_bwx 0: the f16x3 kernel of the cin_math 1 row, at that arithmetic's bar (tests/test_gpu_cin_instances.py)
            ratios["dxp"] = max(ratios.get("dxp", 0.0), _compare(dxp, base_p + dxp_r, dxp_m, family, k_dxp if want_bwx else K_F16X3, what + "dxp"))
            ratios["dx0"] = max(ratios.get("dx0", 0.0), _compare(dx0, base_0 + dx0_r, dx0_m, family, k_dx0 if want_bwx else K_F16X3, what + "dx0"))
        assert _lib.get_option("last_bwx_f32") == want_bwx
        assert _lib.get_option("last_bwx_kernel") == (0 if want_bwx else math)
        assert want_bwx == 0 or _lib.get_option("last_bwx_inst") == 0

        # ---- dW, twice
        dO_w, xp_w, x0_w = dOut, xp, x0
        if how.get("off"):
            dO_w, x0_w = _off_view(dOut), _off_view(x0)
            xp_w = x0_w if fold else _off_view(xp)
        ws = torch.empty(max(lib.xdfm_cin_bwd_w_ws_elems(H, Hp, m, N), 1), dtype=torch.float32, device=dev)

        def bww():
            dW = torch.full((H, Hp * m), 7.0, device=dev)
            _lib.check(lib.xdfm_cin_level_bwd_w(_p(dO_w), _p(xp_w), _p(x0_w), H, Hp, m, N, _p(ws), _p(dW), st), "cin_level_bwd_w")
            return dW

        dW, dW2 = bww(), bww()
        assert _lib.get_option("last_bww_f32") == want_bww
        assert (_lib.get_option("last_bww_kernel"), _lib.get_option("last_bww_inst")) == (0, 0)
        if want_bww % 10 == 1:
            _same_bits(dW, dW2, "dW")
        else:
            _compare(dW2, dW_r, dW_m, family, k_dW, "dW (second call)")
        ratios["dW"] = _compare(dW, dW_r, dW_m, family, k_dW, "dW")
    return ratios


@pytest.mark.parametrize("family", ["exact", "normal"])
@pytest.mark.parametrize("row", SWEEP_F32, ids=[_row_id(r) for r in SWEEP_F32])
def test_cin_f32_instance_vs_float64(row, family):
    run_row_f32(row, family)


# ---- shapes the kernels have no room for: XDFM_ERR_INVALID before any launch -------------------------------------------
@pytest.mark.parametrize("m,H,Hp,N,opts", [(290, 20, 2, 64, {}), (130, 100, 2, 64, {"fwd_nf": 2})],
                         ids=["m290-nf1", "m130-nf2"])
def test_forward_refuses_a_field_count_beyond_its_lds(m, H, Hp, N, opts):
    """the generic kernel keeps x0 for a wave's columns in LDS: 4 waves * (2 ceil(m / 2) + 32) rows * 32 NF columns of floats
    must fit 160 KB.  Correctly sized buffers; the output stays untouched and the probe keeps its value."""
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    W, bias, xp, x0, _, _, _ = _inputs(m, H, Hp, N, 0, "exact", m, dev)
    with _options(cin_math=0, last_fwd_f32=-1, **opts):
        pack = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_cin_fwd_pack(_p(W), H, Hp, m, _p(pack), st), "cin_fwd_pack")
        out = torch.full((H, N), 7.0, device=dev)
        rc = lib.xdfm_cin_level_fwd(_p(xp), _p(x0), _p(pack), _p(bias), H, Hp, m, N, 1, _p(out), st)
        assert rc == 1 and b"LDS" in lib.xdfm_last_error(), (rc, lib.xdfm_last_error())
        assert _lib.get_option("last_fwd_f32") == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_dx_refuses_a_field_count_beyond_its_lds():
    """dX keeps a wave's dx0 slice in LDS: 4 waves * m * 32 floats; m = 320 is the last that fits 160 KB"""
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    m, H, Hp, N = 321, 8, 1, 33
    W, _, xp, x0, dOut, pre_p, pre_0 = _inputs(m, H, Hp, N, 0, "exact", m, dev)
    with _options(cin_math=0, last_bwx_f32=-1):
        wz = torch.empty(lib.xdfm_cin_bwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_cin_bwd_pack(_p(W), H, Hp, m, _p(wz), st), "cin_bwd_pack")
        dxp, dx0 = pre_p.clone(), pre_0.clone()
        rc = lib.xdfm_cin_level_bwd_x_ex(_p(dOut), _p(xp), _p(x0), _p(wz), H, Hp, m, N, _p(dxp), _p(dx0), 3, st)
        assert rc == 1 and b"LDS" in lib.xdfm_last_error(), (rc, lib.xdfm_last_error())
        assert _lib.get_option("last_bwx_f32") == -1
    torch.cuda.synchronize()
    assert torch.equal(dxp, pre_p) and torch.equal(dx0, pre_0)


def test_dw_v1_refuses_the_slab_epilogue():
    """dbg 8 (cin_bwd_w_kernel) has the atomic epilogue only: with bww_slab 1 the call is refused and dW stays untouched"""
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    m, H, Hp, N = 5, 100, 3, 77
    _, _, xp, x0, dOut, _, _ = _inputs(m, H, Hp, N, 0, "exact", 8, dev)
    with _options(cin_math=0, dbg=8, bww_slab=1, last_bww_f32=-1):
        ws = torch.empty(lib.xdfm_cin_bwd_w_ws_elems(H, Hp, m, N), dtype=torch.float32, device=dev)
        dW = torch.full((H, Hp * m), 7.0, device=dev)
        rc = lib.xdfm_cin_level_bwd_w(_p(dOut), _p(xp), _p(x0), H, Hp, m, N, _p(ws), _p(dW), st)
        assert rc == 1 and b"bww_slab" in lib.xdfm_last_error(), (rc, lib.xdfm_last_error())
        assert _lib.get_option("last_bww_f32") == -1
    torch.cuda.synchronize()
    assert bool((dW == 7.0).all())


# ---- xdfm_cin_direct_sum: res[b][off + r] = sum_d A[row0 + r][b * D + d] -------------------------------------------------
#   D, B, offset of A in floats: float4 kernel (D = 4 .. 64 a power of two, N % 4 == 0, aligned), scalar power-of-two kernel
#   (D = 1, 2, or unaligned), generic kernel (other D)
DIRECT_SUM = [(4, 1100, 0), (16, 275, 0), (32, 32, 0), (64, 16, 0), (64, 69, 0), (4, 256, 0),
              (1, 300, 0), (2, 515, 0), (8, 130, 1),
              (10, 300, 0), (128, 9, 0)]


@pytest.mark.parametrize("family", ["exact", "normal"])
@pytest.mark.parametrize("D,B,a_off", DIRECT_SUM, ids=["D%d-B%d-off%d" % t for t in DIRECT_SUM])
def test_direct_sum_vs_float64(D, B, a_off, family):
    """rows [row0, row0 + rows) of a taller tensor into columns [off, off + rows) of a wider, prefilled result: every other
    cell keeps its bits.  Integers: exact.  Gaussian: a sum of D fp32 values in any order is within (D - 1) roundings of
    sum |a|; the bar is (D + 1) * 2^-24 * sum |a| per cell."""
    from xdfm_amd import _lib
    lib = _lib.load()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(D * 1000 + B)
    Ht, row0, rows, off, ldres = 7, 2, 4, 3, 10
    N = B * D
    buf = torch.empty(Ht * N + 8, device=dev)
    A = buf[a_off:a_off + Ht * N].view(Ht, N)
    assert A.data_ptr() % 16 == 4 * a_off
    if family == "exact":
        A.copy_(torch.randint(-50, 51, (Ht, N), generator=g, device=dev).float())
    else:
        A.copy_(torch.randn((Ht, N), generator=g, device=dev))
    pre = torch.randint(-9, 10, (B, ldres), generator=g, device=dev).float() + 0.25
    res = pre.clone()
    _lib.check(lib.xdfm_cin_direct_sum(_p(A), row0, rows, B, D, _p(res), ldres, off, st), "cin_direct_sum")
    A3 = A[row0:row0 + rows].double().view(rows, B, D)
    want, mag = A3.sum(dim=2).t(), A3.abs().sum(dim=2).t()
    got = res[:, off:off + rows].double()
    if family == "exact":
        assert torch.equal(got, want)
    else:
        err = (got - want).abs()
        bar = (D + 1) * 2.0 ** -24 * mag
        assert bool((err <= bar).all()), "worst |got - ref| / sum|a| = %.3g" % float((err / mag).max())
    keep = torch.ones(ldres, dtype=torch.bool, device=dev)
    keep[off:off + rows] = False
    _same_bits(res[:, keep].contiguous(), pre[:, keep].contiguous(), "cells outside [off, off + rows)")
    # rows = 0: OK, and nothing is written
    res2 = pre.clone()
    _lib.check(lib.xdfm_cin_direct_sum(_p(A), row0, 0, B, D, _p(res2), ldres, off, st), "cin_direct_sum")
    _same_bits(res2, pre, "rows = 0")


# ---- xdfm_cin_dout_det / xdfm_cin_dout with act 0 and 1 --------------------------------------------------------------------
_PLAIN = {}


def _plain_run(dev):
    import cin_sigmoid_cases as C
    if not _PLAIN:
        _PLAIN.update(C.run_cases(dev, C.ACT_CASES))
    return _PLAIN


def _check_dout(out, tag):
    """dOut = act'(A) (dHid + dDirect): at most one rounding (the sum of the two sources), exact zeros where ReLU's output
    is 0.0 or -0.0 and in rows without a source; dbias = dbias0 + row sums of the fp32 dOut within the column-sum bar of
    tests/head_reg_ref.py (gamma(n) sum |terms|, n = N + 1 terms with dbias0).  The second call and the in-place call
    (dOut is A) repeat the first one's bits; the atomic finish repeats dOut and meets the same dbias bar."""
    import cin_sigmoid_cases as C
    import head_reg_ref as R
    for name in C.ACT_CASES:
        c = C.make_case(name)
        gh, gd = C.sources64(c)
        A = c["A"]
        slope = (A > 0).astype(np.float64) if c["act"] == C.RELU else np.ones(A.shape)
        want = (gh + gd) * slope
        bound = 2.0 ** -24 * np.abs(want)
        d0 = out[name + "/0/dOut"]
        assert d0.dtype == np.float32 and np.isfinite(d0).all()
        err = np.abs(d0.astype(np.float64) - want)
        assert (err <= bound).all(), "%s %s: %d elements of dOut off by more than one rounding" % (tag, name, int((err > bound).sum()))
        if c["act"] == C.RELU:
            assert (A == 0).sum() >= 16 and np.signbit(A[A == 0]).any()
            assert not d0[A == 0].any(), "dOut must be exactly 0 where the ReLU output is 0.0 or -0.0"
        else:
            assert (want[A < 0] != 0).any() and (d0[A < 0] != 0).any(), "a linear level passes the gradient whatever A's sign"
        rows = np.arange(c["H"])
        has = ((rows >= c["hid0"]) & (rows < c["hid0"] + c["hid_rows"])) | ((rows >= c["dir0"]) & (rows < c["dir0"] + c["dir_rows"]))
        assert (~has).sum() >= 1 and has.sum() >= 1
        assert not d0[~has].any(), "rows without a gradient source must be exact zeros"
        b0 = out[name + "/0/dbias"]
        assert b0[~has].tobytes() == c["dbias0"][~has].tobytes(), "dbias of a row without a source must keep its bits"
        sums = d0.sum(axis=1, dtype=np.float64) + c["dbias0"]
        bbound = R.gamma(c["N"] + 1) * (np.abs(d0).sum(axis=1, dtype=np.float64) + np.abs(c["dbias0"]))
        for rep in ("0", "atomic"):
            b = out["%s/%s/dbias" % (name, rep)]
            frac = float((np.abs(b - sums) / bbound).max())
            print("%s %-26s dbias (%s): %.3g of the bound" % (tag, name, rep, frac))
            assert (np.abs(b - sums) <= bbound).all(), (name, rep, frac)
        for rep in ("1", "inplace", "atomic"):
            assert out["%s/%s/dOut" % (name, rep)].tobytes() == d0.tobytes(), "%s: dOut of the %s call has other bits" % (name, rep)
        for rep in ("1", "inplace"):
            assert out["%s/%s/dbias" % (name, rep)].tobytes() == b0.tobytes(), "%s: dbias of the %s call has other bits" % (name, rep)


def test_dout_relu_and_linear_vs_float64_two_launch_finish():
    _check_dout(_plain_run(_dev()), "two-launch")

