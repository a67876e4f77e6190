"""CPU checks of what the K9 GPU tests (tests/test_gpu_vocab_ce_abi.py) lean on: tests/vocab_ce_ref.py's plan mirror against
xdfm_vocab_ce_plan (host-side code of csrc/vocab_ce_x3.hip), the structure of the library's plan, the plan facts every
large case exists for (a change of the planner that would turn them back into one-stage, one-trip cases fails HERE), and
the float64 reference against torch's cross_entropy + autograd."""
import numpy as np
import pytest
import torch

import vocab_ce_ref as VR

SUITE_SHAPES = [(300, 64, (50000, 77, 1000)), (1100, 64, (70001, 256)), (4096, 64, (3000, 129)), (1100, 32, (7, 300, 1000)),
                (1, 64, (5,)), (513, 32, (4097,))]                              # what the older K9 tests use
EDGE_SHAPES = [(70, K, VR.EDGE_VOCABS["E1"]) for K in (32, 64)] + \
              [(R, K, VR.EDGE_VOCABS["E5"]) for R in (1, 256, 257) for K in (32, 64)] + [(70, 32, (300,)), (70, 64, (300, 40))]
ALL_SHAPES = list(VR.LARGE_CASES.values()) + EDGE_SHAPES + SUITE_SHAPES + [VR.BENCH_SHAPE]


def _lib():
    from xdfm_amd import _lib
    return _lib.load()


def _id(shape):
    R, K, Vs = shape
    return "R%d-K%d-%s" % (R, K, "x".join(str(v) for v in Vs[:3]) + ("-F%d" % len(Vs) if len(Vs) > 3 else ""))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_plan_mirror_equals_the_library(shape):
    R, K, Vs = shape
    got, want = VR.plan_mirror(R, K, Vs), VR.library_plan(_lib(), R, K, Vs)
    assert got["n_blk"] == want["n_blk"] and got["ws_elems"] == want["ws_elems"] and got["rows_padded"] == want["rows_padded"]
    assert len(got["fields"]) == len(want["fields"]) == len(Vs)
    for f, (a, b) in enumerate(zip(got["fields"], want["fields"])):
        for key in ("V", "vr", "item0", "blk0", "ws_off"):
            assert a[key] == b[key], "field %d %s" % (f, key)
        assert a["items"] == b["items"], "field %d: stage intervals" % f
    if any(f["vr"] > 1 for f in want["fields"]):
        assert got["spr"] == want["spr"]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_library_plan_structure(shape):
    R, K, Vs = shape
    p = VR.library_plan(_lib(), R, K, Vs)
    rpad = -(-R // VR.VX_RG) * VR.VX_RG
    assert p["rows_padded"] == rpad
    blk = item = 0
    spans = []
    for V, fd in zip(Vs, p["fields"]):
        nsb = -(-V // VR.VX_SB)
        assert fd["V"] == V and fd["blk0"] == blk and fd["item0"] == item and len(fd["items"]) == fd["vr"] >= 1
        # the items partition [0, nsb) in ascending order, none empty, none longer than spr
        assert fd["items"][0][0] == 0 and fd["items"][-1][1] == nsb
        assert all(a < b <= a + p["spr"] for a, b in fd["items"])
        assert all(fd["items"][i][1] == fd["items"][i + 1][0] for i in range(fd["vr"] - 1))
        spans.append((fd["ws_off"], fd["ws_off"] + fd["vr"] * rpad * K))
        blk += nsb
        item += fd["vr"]
    assert p["n_blk"] == blk
    spans.sort()
    assert spans[0][0] == 0 and all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
    assert p["ws_elems"] == sum(b - a for a, b in spans) == spans[-1][1]


@pytest.mark.parametrize("name", list(VR.LARGE_CASES))
def test_large_cases_reach_what_they_exist_for(name):
    """The vacuity guard of tests/test_gpu_vocab_ce_abi.py's large cases, on the LIBRARY's plan: ranges of more than one
    stage (the prefetch, the re-publish and the carried state of vx_hs_kernel), short last ranges, more than 1024 blocks
    (second and third trips of vx_ws_kernel's persistent loop), workgroups whose next block lies in another field, and
    the row tiles that pick the one- or two-tile instance."""
    R, K, Vs = VR.LARGE_CASES[name]
    p = VR.library_plan(_lib(), R, K, Vs)
    facts, want = VR.plan_facts(p, R), VR.LARGE_FACTS[name]
    assert facts == want
    assert facts["spr"] >= 2 and any(n < facts["spr"] for n in facts["last"])
    if name != "L4":
        assert facts["n_blk"] > VR.VX_GRID and facts["second_trip"] > 0
    else:
        assert R > VR.VX_RG and 0 < facts["tiles"] - 16 <= 8             # a second row group, of the one-tile instance
    if name == "L2":
        assert 8 < facts["tiles"] < 16                                   # two-tile instance, absent second tiles
    # the planted targets: the second stage of a multi-stage range, and a block that a second trip serves
    tgt = VR.large_inputs(name)[3]
    planted = VR.planted_targets(R, K, Vs)
    in_later_stage = second_trip = False
    for f, (fd, vs) in enumerate(zip(p["fields"], planted)):
        assert tgt[f, 1:1 + len(vs)].tolist() == vs and vs[0] == fd["V"] - 1
        for v in vs:
            sb = v // VR.VX_SB
            a, b = next(it for it in fd["items"] if it[0] <= sb < it[1])
            in_later_stage |= sb > a
            second_trip |= fd["blk0"] + sb >= VR.VX_GRID
    assert in_later_stage and second_trip == (name != "L4")


def test_bench_shape_runs_the_same_regimes():
    R, K, Vs = VR.BENCH_SHAPE
    facts = VR.plan_facts(VR.library_plan(_lib(), R, K, Vs), R)
    assert facts["spr"] == 98 and set(facts["vr"]) == {4} and set(facts["last"]) == {97} and facts["n_blk"] == 10166


def _torch_ce(h, Ws, bs, tgt, g):
    h6 = h.double().requires_grad_(True)
    W6 = [w.double().requires_grad_(True) for w in Ws]
    b6 = [b.double().requires_grad_(True) for b in bs]
    ce = torch.stack([torch.nn.functional.cross_entropy(torch.nn.functional.linear(h6, w, b), tgt[f].clamp(0, w.shape[0] - 1),
                                                        reduction="none") for f, (w, b) in enumerate(zip(W6, b6))])
    (ce * g.double()).sum().backward()
    return ce.detach(), h6.grad, [w.grad for w in W6], [b.grad for b in b6]


@pytest.mark.parametrize("as_numpy", [False, True])
def test_reference_equals_torch_cross_entropy_in_float64(as_numpy):
    R, K, Vs = 9, 32, (5, 1, 40)
    h, Ws, bs, tgt, g = VR.make_inputs(R, K, Vs, seed=5)
    tgt[0, :5] = torch.tensor([-1, -(1 << 40), 5, 12, 1 << 40])                # clamped: 0, 0, 4, 4, 4
    tgt[2, 1] = 40
    args = (h, Ws, bs, tgt, g)
    if as_numpy:
        args = (h.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], tgt.numpy(), g.numpy())
    want = _torch_ce(h, Ws, bs, tgt, g)
    for n in (None, 4, 0):
        ce, dh, dWs, dbs = VR.reference(*args, n=n)
        assert isinstance(ce, np.ndarray) == as_numpy and str(ce.dtype).endswith("float64")
        m = R if n is None else n
        w = want if n is None else _torch_ce(h[:m], Ws, bs, tgt[:, :m], g[:, :m])
        assert ce.shape == (len(Vs), m) and dh.shape == (m, K)
        flat = lambda r: [r[0], r[1]] + list(r[2]) + list(r[3])
        for a, b in zip(flat((ce, dh, dWs, dbs)), flat(w)):
            np.testing.assert_allclose(np.asarray(a), b.numpy(), rtol=1e-12, atol=1e-15)
    # the clamp itself: a far-out target gives what the border row gives
    t2 = tgt.clone()
    t2[0, :5] = torch.tensor([0, 0, 4, 4, 4])
    t2[2, 1] = 39
    a, b = VR.reference(h, Ws, bs, tgt, g), VR.reference(h, Ws, bs, t2, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2] + a[3], b[2] + b[3]))


def test_reference_walks_rows_in_chunks():
    """More rows than one chunk: the same numbers as one pass over all rows."""
    R, K, Vs = VR.CHUNK + 37, 32, (19,)
    args = VR.make_inputs(R, K, Vs, seed=6)
    got, want = VR.reference(*args), _torch_ce(*args)
    for a, b in zip([got[0], got[1], got[2][0], got[3][0]], [want[0], want[1], want[2][0], want[3][0]]):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-11, atol=1e-15)
