"""GPU tests (-m gpu) of K9 (csrc/vocab_ce_x3.hip) at the C ABI: xdfm_vocab_ce_pack_hidden[_n], _fwd[_n], _pack_g[_n],
_bwd_h[_n] and _bwd_w[_n] called through ctypes (tests/vocab_ce_ref.py `drive`) with buffers of the test's own, against a
float64 reference of the same operation (`reference`).

Large-plan cases (vocab_ce_ref.LARGE_CASES; few rows, large vocabularies; their plan facts are asserted on the CPU by
tests/test_vocab_ce_reference.py):
  L1  ranges of two stages in vx_hs_kernel (prefetch, re-publish, carried (max, sum) / dacc), a one-stage last range, 1029
      blocks: five workgroups of vx_ws_kernel take a second block, two of them in another field
  L2  the same with three fields and 10 row tiles: the two-tile instance with absent second tiles
  L3  ranges of three stages, 2051 blocks: every workgroup takes two trips, three take a third
  L4  two row groups (the second of the one-tile instance), ranges of two stages, a single trip
Edge cases E1 .. E7, each at K = 32 and K = 64: pitches and guard bands, clamped targets, NULL gradients, zero operands
(x3_pow2_scale(0, ..)), vocabulary and row edges, one hot target, operand magnitudes far apart.

Bars: those of tests/test_gpu_pro.py::test_vocab_heads_ce_fused_vs_materialised_logits -- ce rtol 2e-5, atol 2e-5;
gradients rtol 2e-4, atol 2e-5 x the tensor's largest reference magnitude.  The large cases also print the error of the
materialised fp32 path (torch linear + cross_entropy on the device) against the same reference: recorded in DESIGN.md,
not asserted."""
import faulthandler

import pytest
import torch

import vocab_ce_ref as VR

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
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


def _lib():
    from xdfm_amd import _lib, ops
    lib = _lib.load()
    assert ops.vocab_heads_ce_supported(32) and ops.vocab_heads_ce_supported(64)
    return lib


def _to(dev, inputs):
    h, Ws, bs, tgt, g = inputs
    return h.to(dev).contiguous(), [w.to(dev) for w in Ws], [b.to(dev) for b in bs], tgt.to(dev).contiguous(), g.to(dev).contiguous()


def _flat(ref):
    ce, dh, dWs, dbs = ref
    return [("ce", ce), ("dh", dh)] + [("dW%d" % f, t) for f, t in enumerate(dWs)] + [("db%d" % f, t) for f, t in enumerate(dbs)]


def _check(tag, out, ref, n=None):
    """Every output `out` holds against the reference, all of them before the first complaint; n: rows in front of a count."""
    want = dict(_flat(ref))
    bad = []
    for name, got in out.outputs():
        assert bool(torch.isfinite(got).all()), "%s %s holds a NaN or an infinity" % (tag, name)
        if n is not None and name in ("ce", "dh"):
            got = got[:, :n] if name == "ce" else got[:n]
        err, amax = VR.errors(got, want[name])
        print("%-22s %-4s kernel %.3e  largest reference magnitude %.3e" % (tag, name, err, amax))
        try:
            VR.assert_bars("%s %s" % (tag, name), got, want[name], is_ce=name == "ce")
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


def _same_bits(tag, a, b, also=("lse2", "wmax")):
    pairs = list(zip(a.outputs(), b.outputs())) + [((k, getattr(a, k)), (k, getattr(b, k))) for k in also]
    for (name, x), (name_b, y) in pairs:
        assert name == name_b
        assert torch.equal(VR.bits(x), VR.bits(y)), "%s: %s differs" % (tag, name)


# ----------------------------------------------------------------------------------------------- large-plan cases
def _large(name):
    if name not in _CACHE:
        dev, lib = _dev(), _lib()
        cpu = VR.large_inputs(name)
        d = _to(dev, cpu)
        _CACHE[name] = dict(dev=d, ref=VR.reference(*d), run=VR.drive(lib, *d))
    return _CACHE[name]


def _fp32_path(h, Ws, bs, tgt, g):
    """The materialised computation in fp32 on the device, one field at a time: torch linear + cross_entropy + autograd."""
    hd = h.clone().requires_grad_(True)
    ce, dWs, dbs = [], [], []
    for f, (W, b) in enumerate(zip(Ws, bs)):
        W, b = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        c = torch.nn.functional.cross_entropy(torch.nn.functional.linear(hd, W, b), tgt[f], reduction="none")
        (c * g[f]).sum().backward()
        ce.append(c.detach())
        dWs.append(W.grad)
        dbs.append(b.grad)
    return torch.stack(ce), hd.grad, dWs, dbs


@pytest.mark.parametrize("name", list(VR.LARGE_CASES))
def test_large_plan_case_against_float64(name):
    c = _large(name)
    R, K, Vs = VR.LARGE_CASES[name]
    tgt = c["dev"][3]
    assert all(int(tgt[f].min()) >= 0 and int(tgt[f].max()) == V - 1 for f, V in enumerate(Vs))
    lib_ = dict(_flat(_fp32_path(*c["dev"])))
    for (key, got), (_, want) in zip(c["run"].outputs(), _flat(c["ref"])):
        (e_k, amax), (e_l, _) = VR.errors(got, want), VR.errors(lib_[key], want)
        print("%s R=%d K=%d %-4s kernel %.3e / fp32 path %.3e  (largest reference magnitude %.3e)" % (name, R, K, key, e_k, e_l, amax))
    _check(name, c["run"], c["ref"])


@pytest.mark.parametrize("name", list(VR.LARGE_CASES))
def test_large_plan_case_two_runs_same_bits(name):
    """The second run on NaN-filled scratch: partial results are merged in a fixed order and nothing unwritten is read."""
    c = _large(name)
    _same_bits(name, VR.drive(_lib(), *c["dev"], poison=True), c["run"])


@pytest.mark.parametrize("n", [1, 20])
def test_large_plan_case_with_a_device_row_count(n):
    """L1 at a capacity of 33 rows with n in use: NaN hidden rows and gradients and far-out targets behind the count."""
    c = _large("L1")
    h, Ws, bs, tgt, g = c["dev"]
    h, tgt, g = h.clone(), tgt.clone(), g.clone()
    h[n:] = float("nan")
    g[:, n:] = float("nan")
    tgt[:, n:] = 1 << 40
    out = VR.drive(_lib(), h, Ws, bs, tgt, g, n_rows=n, poison=True)
    assert out.ce.shape[1] == h.shape[0] == 33
    assert bool((out.ce[:, n:] == 0).all()) and bool((out.dh[n:] == 0).all()), "rows behind the count: exact zeros"
    _check("L1 n=%d" % n, out, VR.reference(h, Ws, bs, tgt, g, n=n), n=n)


# ------------------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("K", [32, 64])
def test_e1_pitches_guard_bands_and_poisoned_scratch(K):
    dev, lib = _dev(), _lib()
    d = _to(dev, VR.make_inputs(70, K, VR.EDGE_VOCABS["E1"], seed=100 + K))
    plain = VR.drive(lib, *d)
    out = VR.drive(lib, *d, lddh=K + 8, ldh_fwd=K + 3, guards=True, poison=True)
    assert out.buffers["dh"].pitch == K + 8 and out.dh.stride(0) == K + 8 and out.keep[1].stride(0) == K + 3
    assert bool(torch.isnan(out.keep[1][:, K:]).all())
    assert out.written_outside() == [], "written outside its bounds (guard band or pad column)"
    for name, t in out.outputs() + [("lse2", out.lse2)]:
        assert bool(torch.isfinite(t).all()), name
    _same_bits("E1 K=%d pitched, guarded, poisoned against the plain call" % K, out, plain)
    _check("E1 K=%d" % K, out, VR.reference(*d))


@pytest.mark.parametrize("K", [32, 64])
def test_e2_targets_outside_the_vocabulary_are_clamped(K):
    dev, lib = _dev(), _lib()
    Vs = (300, 40)
    h, Ws, bs, tgt, g = VR.make_inputs(70, K, Vs, seed=200 + K)
    clamped = tgt.clone()
    for f, V in enumerate(Vs):
        tgt[f, 1:6] = torch.tensor([-1, -(1 << 40), V, V + 7, 1 << 40])
        clamped[f, 1:6] = torch.tensor([0, 0, V - 1, V - 1, V - 1])
        assert bool((g[f, 1:6] != 0).all())                                  # live rows
    d = _to(dev, (h, Ws, bs, tgt, g))
    out, want = VR.drive(lib, *d), VR.drive(lib, d[0], d[1], d[2], clamped.to(dev), d[4])
    _same_bits("E2 K=%d far-out targets against the host's clamp" % K, out, want)
    _check("E2 K=%d" % K, out, VR.reference(*d))


@pytest.mark.parametrize("K", [32, 64])
def test_e3_null_gradient_pointers_per_field(K):
    """Field 0: dW only; field 1: db only; field 2: neither."""
    dev, lib = _dev(), _lib()
    d = _to(dev, VR.make_inputs(70, K, (257, 33, 70), seed=300 + K))
    full = VR.drive(lib, *d, guards=True)
    part = VR.drive(lib, *d, want_dW=[True, False, False], want_db=[False, True, False], guards=True)
    assert part.written_outside() == [] and full.written_outside() == []
    assert [n for n, _ in part.outputs()] == ["ce", "dh", "dW0", "db1"]
    have = dict(full.outputs())
    for name, t in part.outputs() + [("lse2", part.lse2)]:
        assert torch.equal(VR.bits(t), VR.bits(have[name] if name in have else full.lse2)), "E3 K=%d %s" % (K, name)
    _check("E3 K=%d" % K, full, VR.reference(*d))


@pytest.mark.parametrize("K", [32, 64])
def test_e4a_a_field_whose_upstream_gradient_is_all_zero(K):
    dev, lib = _dev(), _lib()
    h, Ws, bs, tgt, g = VR.make_inputs(70, K, (300, 40, 130), seed=400 + K)
    g[1] = 0.0
    d = _to(dev, (h, Ws, bs, tgt, g))
    out = VR.drive(lib, *d, poison=True)
    assert bool((out.dWs[1] == 0).all()) and bool((out.dbs[1] == 0).all())
    keep = [0, 2]
    without = VR.drive(lib, d[0], [d[1][f] for f in keep], [d[2][f] for f in keep], d[3][keep].contiguous(), d[4][keep].contiguous())
    assert bool((out.dh == without.dh).all()), "dh with a zero-gradient field against the call without that field"
    _check("E4a K=%d" % K, out, VR.reference(*d))


@pytest.mark.parametrize("K", [32, 64])
def test_e4b_an_all_zero_hidden_layer(K):
    dev, lib = _dev(), _lib()
    h, Ws, bs, tgt, g = VR.make_inputs(70, K, (300, 40), seed=410 + K)
    h.zero_()
    d = _to(dev, (h, Ws, bs, tgt, g))
    out = VR.drive(lib, *d, poison=True)
    ref = VR.reference(*d)
    for f, b in enumerate(bs):
        want = torch.logsumexp(b.double(), 0) - b.double()[tgt[f]]
        assert torch.allclose(ref[0][f].cpu(), want, rtol=0, atol=1e-14)
        assert bool((out.dWs[f] == 0).all()), "dW%d with a zero hidden layer" % f
    assert float(ref[3][0].abs().max()) > 0
    _check("E4b K=%d" % K, out, ref)


@pytest.mark.parametrize("K", [32, 64])
def test_e4c_a_head_of_zero_weights_and_constant_bias(K):
    import math
    dev, lib = _dev(), _lib()
    Vs = (300, 40, 130)
    h, Ws, bs, tgt, g = VR.make_inputs(70, K, Vs, seed=420 + K)
    Ws[1].zero_()
    bs[1].fill_(0.75)
    d = _to(dev, (h, Ws, bs, tgt, g))
    out = VR.drive(lib, *d, poison=True)
    ref = VR.reference(*d)
    assert torch.allclose(ref[0][1].cpu(), torch.full((70,), math.log(Vs[1]), dtype=torch.float64), rtol=0, atol=1e-14)
    assert int(out.wmax[1]) == 0
    keep = [0, 2]
    without = VR.drive(lib, d[0], [d[1][f] for f in keep], [d[2][f] for f in keep], d[3][keep].contiguous(), d[4][keep].contiguous())
    assert bool((out.dh == without.dh).all()), "the zero head's share of dh is not exactly 0"
    _check("E4c K=%d" % K, out, ref)


@pytest.mark.parametrize("K", [32, 64])
def test_e4d_a_zero_block_inside_a_random_head(K):
    """Rows 64 .. 95: one 32-row block of the forward's per-block scale."""
    dev, lib = _dev(), _lib()
    h, Ws, bs, tgt, g = VR.make_inputs(70, K, (300,), seed=430 + K)
    Ws[0][64:96] = 0.0
    tgt[0, 1:4] = torch.tensor([64, 80, 95])
    d = _to(dev, (h, Ws, bs, tgt, g))
    _check("E4d K=%d" % K, VR.drive(lib, *d, poison=True), VR.reference(*d))


@pytest.mark.parametrize("R", [1, 256, 257])
@pytest.mark.parametrize("K", [32, 64])
def test_e5_vocabulary_and_row_edges_in_one_call(K, R):
    """Eight fields, V = 1 .. 513; R = 1 keeps its only row live (g = 4e-4 there: row 0 is otherwise a zero row of g)."""
    dev, lib = _dev(), _lib()
    Vs = VR.EDGE_VOCABS["E5"]
    h, Ws, bs, tgt, g = VR.make_inputs(R, K, Vs, seed=500 + K + R)
    if R == 1:
        g = torch.full_like(g, 4.0e-4)
    for f, V in enumerate(Vs):
        tgt[f, R - 1] = V - 1
    d = _to(dev, (h, Ws, bs, tgt, g))
    _check("E5 K=%d R=%d" % (K, R), VR.drive(lib, *d, poison=True), VR.reference(*d))


@pytest.mark.parametrize("hot", ["first", "last"])
@pytest.mark.parametrize("K", [32, 64])
def test_e6_every_row_has_the_same_target(K, hot):
    dev, lib = _dev(), _lib()
    V = 300
    h, Ws, bs, tgt, g = VR.make_inputs(70, K, (V,), seed=600 + K)
    tgt[:] = 0 if hot == "first" else V - 1
    d = _to(dev, (h, Ws, bs, tgt, g))
    _check("E6 K=%d %s" % (K, hot), VR.drive(lib, *d), VR.reference(*d))


@pytest.mark.parametrize("K", [32, 64])
def test_e7_operand_magnitudes_far_apart(K):
    """One head with 32-row blocks of scale 1e-4 (rows 64 .. 95) and 10 (rows 160 .. 191) among blocks of scale 0.3, hidden
    rows scaled from 1e-3 to 10: the forward and the dW kernel scale every block on its own, the dH kernel uses one scale
    per head.

    Found here: with one scale per head and accumulators started at -lse / cw, vx_ws_kernel's z differed from the forward's
    by a few ulp(lse2) (2.4e-4 each at lse2 = 2979), softmax = 2^(z - lse2) carried 2e-4 .. 5e-4 of relative error, and at
    K = 64 (logits to 2065) 17 elements of dW0, all in the large rows' dominant vocabulary row 163, missed rtol 2e-4: dW0
    1.4e-06 off float64 against 1.1e-09 for the materialised fp32 path.  The kernel now forms z with the forward's bits
    (DESIGN 4.5); kernel / fp32 path since: K = 64 ce 1.5e-04 / 2.1e-04, dh 1.9e-06 / 2.2e-08, dW0 1.1e-08 / 1.1e-09, db0
    2.4e-09 / 6.4e-10; K = 32 (logits to 1355) ce 9.4e-05 / 1.1e-04, dh 1.2e-06 / 3.1e-08, dW0 4.1e-09 / 4.5e-09, db0 1.0e-09 /
    1.5e-09."""
    dev, lib = _dev(), _lib()
    gen = torch.Generator().manual_seed(700 + K)
    h, Ws, bs, tgt, g = VR.make_inputs(70, K, (300,), seed=710 + K)
    Ws[0][64:96] = torch.randn(32, K, generator=gen) * 1e-4
    Ws[0][160:192] = torch.randn(32, K, generator=gen) * 10.0
    h *= torch.logspace(-3, 1, 70)[:, None]
    tgt[0, 1:5] = torch.tensor([64, 95, 160, 191])
    d = _to(dev, (h, Ws, bs, tgt, g))
    out, ref = VR.drive(lib, *d, poison=True), VR.reference(*d)
    for (key, got), (_, want) in zip(_flat(_fp32_path(*d)), _flat(ref)):
        print("E7 K=%d %-4s fp32 path %.3e" % (K, key, VR.errors(got, want)[0]))
    _check("E7 K=%d" % K, out, ref)


@pytest.mark.parametrize("R", [20, 70])
@pytest.mark.parametrize("K", [32, 64])
def test_odd_tile_count_with_a_logit_beyond_2_to_the_128(K, R):
    """Found by E7: vx_ws_kernel's ring slots hold two row tiles, and with an odd number of tiles (1 at R = 20, 3 at R = 70)
    the last slot repeats the last tile with zero gradients.  Its rows had lse2 = 0, so their z were the last tile's bare
    logits: above 128 in base 2 (88.7 in base e) 2^z = inf, and inf * 0 put NaN into every dW / db row of that block.  The
    last row's logit against W[7] is 96 here (h = +-12, W[7] = +-8 / K with h's signs: 138 in base 2, ulp 1.5e-5); its
    target is another row, so that every element keeps softmax's relative error, 1e-5 at this logit, against the bar's rtol."""
    dev, lib = _dev(), _lib()
    h, Ws, bs, tgt, g = VR.make_inputs(R, K, (300,), seed=800 + K + R)
    sign = torch.where(h[R - 1] < 0, -1.0, 1.0)
    h[R - 1] = 12.0 * sign
    Ws[0][7] = (8.0 / K) * sign
    tgt[0, R - 1] = 11
    assert float(g[0, R - 1]) != 0 and -(-R // 32) % 2 == 1
    d = _to(dev, (h, Ws, bs, tgt, g))
    ref = VR.reference(*d)
    assert float((d[0].double() @ d[1][0].double().t())[R - 1].max()) * 1.4427 > 128
    _check("odd tiles K=%d R=%d" % (K, R), VR.drive(lib, *d, poison=True), ref)
