"""GPU tests (-m gpu) of the deferred Adam replay (csrc/adam_math.h: adam_replay_pk, adam_replay_span) at the C ABI:
xdfm_adam_flush and xdfm_adam_catchup_rows against the dense sweep K7 (xdfm_adam_step), which replays nothing.

The yardstick: `t` steps of the dense sweep on a zero gradient (the L2 term alone moves the weights, which is what a
chunk no batch touched sees), every step's p, m, v kept.  A deferred state is put together from it -- a chunk whose
`last` byte is k holds the sweep's state after step k -- the clock is set to t, and one call has to bring every chunk it
owes to the sweep's state after step t: p, m, v compared as int32 bit patterns, `last` all 0 after a flush (t on the
chunks a catch-up claimed).  The L2 backlog is compared with the float64 sum of l2 * p^2 over the (chunk, step) pairs
the call replays, taken from the sweep's own states, to 1e-5 relative; where the call replays every chunk for every step
(`last` all 0) also with the sum of the sweep's own L2 values to 2e-6 relative -- the two bars of
tests/test_gpu_adam.py::test_deferred_scan_is_bit_identical_to_the_sweep.  Where nothing is owed (l2 = 0, or every chunk
current) the backlog must stay exactly 0.

One sweep of 200 steps per L2 strength serves every case (a run of t steps is its prefix); the clock's constant table is
filled once by 200 real ticks of xdfm_adam_step_deferred."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu

HP = "H0"
SIZES = (4, 12, 1020, 1024, 1028, 8192, 8196, 3 * 8192 + 4)     # one chunk .. one block .. a block and a chunk .. four blocks
T_ALL = (1, 3, 64, 200)
T_MAX = 200
L2_ALL = (0.0, 1e-5)
PATTERNS = ("zero", "current", "random", "one_stale", "alt_waves")
CAP = T_MAX + 2
F32 = np.float32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _state(sizes, seed):
    """[(p, m, v)]: weights of order 1 (an L2 value far above the backlog's 2^-40 fixed point even for one chunk and one
    step), moments as tests/adam_ref.py::make_state."""
    rng = np.random.RandomState(seed)
    return [((rng.randn(n)).astype(F32), (rng.randn(n) * 0.01).astype(F32), (rng.rand(n) * 1e-4 + 1e-8).astype(F32))
            for n in sizes]


_REF, _CONSTS = {}, {}


def _sweep(key, state, l2, steps):
    """`steps` dense steps on a zero gradient, one xdfm_adam_step call per tensor and step.
    -> {"snap": [tensor][0..2] = float32 [steps + 1, n], "val": float64 [steps, tensors] (the calls' L2 values),
        "cum": [tensor] = float64 [steps + 1, n], cum[s] = sum over r < s of p_r^2}"""
    if key in _REF:
        return _REF[key]
    dev = _dev()
    bank = R.Bank(state, dev)
    N = len(state)
    snaps = [[[getattr(bank, a)[k].clone()] for a in ("p", "m", "v")] for k in range(N)]
    vals = torch.zeros(steps, N, dtype=torch.float32, device=dev)
    for s in range(1, steps + 1):
        for k in range(N):
            out = R.adam_step(bank, [k], [l2], HP, s, want_l2=True)
            vals[s - 1, k:k + 1].copy_(out)
        for k in range(N):
            for j, a in enumerate(("p", "m", "v")):
                snaps[k][j].append(getattr(bank, a)[k].clone())
    torch.cuda.synchronize()
    snap = [[torch.stack(x).cpu().numpy() for x in snaps[k]] for k in range(N)]
    cum = []
    for k in range(N):
        c = np.zeros((steps + 1, state[k][0].size), np.float64)
        np.cumsum(snap[k][0][:steps].astype(np.float64) ** 2, axis=0, out=c[1:])
        cum.append(c)
    _REF[key] = {"snap": snap, "val": vals.cpu().numpy().astype(np.float64), "cum": cum}
    return _REF[key]


def _main_ref(l2):
    return _sweep(("main", l2), _state(SIZES, 31), l2, T_MAX)


def _consts():
    """The clock's table after T_MAX ticks from step counter 0 (tick s writes the constants of step s only)."""
    if "c" not in _CONSTS:
        dev = _dev()
        bank = R.Bank(_state([4], 5), dev)
        clk = R.Clock(dev, cap=CAP)
        for s in range(1, T_MAX + 1):
            R.adam_step(bank, [0], [0.0], HP, s, marked=True, flags=[R.DEFERRED], clk=clk)
        torch.cuda.synchronize()
        assert clk.read() == [T_MAX, 0]
        _CONSTS["c"] = clk.consts.clone()
    return _CONSTS["c"]


def _clock(t):
    dev = _dev()
    clk = R.Clock(dev, cap=CAP)
    clk.consts.copy_(_consts())
    clk.clock.copy_(torch.tensor([t, 0], dtype=torch.int32))
    return clk


def _last(pattern, n4, t, rng):
    w = np.arange(n4) // 64
    if pattern == "zero":
        return np.zeros(n4, np.uint8)
    if pattern == "current":
        return np.full(n4, t, np.uint8)
    if pattern == "random":
        return rng.randint(0, t + 1, n4).astype(np.uint8)
    if pattern == "one_stale":                          # lane 7 of every wave owes half the window, the others nothing
        out = np.full(n4, t, np.uint8)
        out[7::64] = t // 2
        if n4 < 8:
            out[-1] = t // 2
        return out
    assert pattern == "alt_waves"                       # even waves current, odd waves owe (t + 1) // 2 steps or more
    out = np.where(w % 2 == 0, t, rng.randint(0, t // 2 + 1, n4)).astype(np.uint8)
    return out


def _compose(ref, k, last):
    """(p, m, v) of tensor k of the sweep `ref` with chunk c at the sweep's state after step last[c]."""
    n = ref["snap"][k][0].shape[1]
    le = np.repeat(last.astype(np.int64), 4)
    assert le.size == n
    return tuple(np.ascontiguousarray(ref["snap"][k][j][le, np.arange(n)]) for j in range(3))


def _owed_l2(ref, k, last, t, l2, chunks=None):
    """float64: l2 * sum of p^2 over the steps last[c] + 1 .. t of the chunks c (all, or the boolean mask `chunks`)."""
    le = np.repeat(last.astype(np.int64), 4)
    c = ref["cum"][k]
    d = c[t] - c[np.minimum(le, t), np.arange(le.size)]
    if chunks is not None:
        d = d[np.repeat(chunks, 4)]
    return float(F32(l2)) * float(d.sum())


def _same_bits(dev_tensor, want):
    w = torch.from_numpy(np.ascontiguousarray(want)).to(dev_tensor.device)
    return torch.equal(dev_tensor.view(torch.int32), w.view(torch.int32))


def _check_state(bank, j, ref, k, t, what):
    for name, arr, a in (("p", bank.p, 0), ("m", bank.m, 1), ("v", bank.v, 2)):
        if not _same_bits(arr[j], ref["snap"][k][a][t]):
            got = arr[j].cpu().numpy().view(np.uint32)
            bad = np.nonzero(got != ref["snap"][k][a][t].view(np.uint32))[0]
            raise AssertionError("%s: %s of tensor %d differs from the sweep in %d of %d elements, first at %d" % (
                what, name, j, bad.size, got.size, int(bad[0])))


def _check_backlog(got, want_f64, want_dense, what):
    print("%s: backlog %.9g float64 %.9g dense %s" % (what, got, want_f64, "%.9g" % want_dense if want_dense is not None else "-"))
    if want_f64 == 0.0:
        assert got == 0.0, what
        return
    assert abs(got - want_f64) <= 1e-5 * want_f64, what
    if want_dense is not None:
        assert abs(got - want_dense) <= 2e-6 * want_dense, what


def _flush_case(ks, t, l2, pattern, seed=0):
    """Tensors ks (indices into SIZES, repeats allowed) in ONE xdfm_adam_flush call."""
    dev = _dev()
    ref = _main_ref(l2)
    rng = np.random.RandomState(1000 * t + 17 * len(ks) + seed)
    lasts = [_last(pattern, SIZES[k] // 4, t, rng) for k in ks]
    bank = R.Bank([_compose(ref, k, la) for k, la in zip(ks, lasts)], dev)
    for j, la in enumerate(lasts):
        bank.last[j][:la.size].copy_(torch.from_numpy(la))
    clk = _clock(t)
    R.adam_flush(bank, list(range(len(ks))), [l2] * len(ks), clk, HP)
    torch.cuda.synchronize()
    what = "flush of %s, t=%d l2=%g %s" % ([SIZES[k] for k in ks] if len(ks) < 4 else "%d tensors" % len(ks), t, l2, pattern)
    for j, k in enumerate(ks):
        _check_state(bank, j, ref, k, t, what)
    assert all(not bool(x.any()) for x in bank.last), what + ": a `last` byte survived"
    assert clk.read() == [0, t], what
    want = sum(_owed_l2(ref, k, la, t, l2) for k, la in zip(ks, lasts))
    dense = float(sum(ref["val"][:t, k].sum() for k in ks)) if pattern == "zero" else None
    _check_backlog(clk.take_backlog(), want, dense, what)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("l2", L2_ALL)
@pytest.mark.parametrize("t", T_ALL)
@pytest.mark.parametrize("k", range(len(SIZES)), ids=["n%d" % n for n in SIZES])
def test_flush_of_one_tensor_gives_the_sweeps_bits(k, t, l2, pattern):
    _flush_case([k], t, l2, pattern)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("l2", L2_ALL)
@pytest.mark.parametrize("t", T_ALL)
def test_flush_of_two_tensors_in_one_launch(t, l2, pattern):
    _flush_case([2, 6], t, l2, pattern)                 # 1020 and 8196 elements: a tail wave each


@pytest.mark.parametrize("pattern", ("zero", "random"))
@pytest.mark.parametrize("l2", L2_ALL)
@pytest.mark.parametrize("t", (3, 64))
def test_flush_of_65_tensors_takes_two_launches(t, l2, pattern):
    _flush_case([j % len(SIZES) for j in range(65)], t, l2, pattern)


# --------------------------------------------------------------------------------------------- the guard's edges
# One chunk per wave (lane 17) whose first element is seeded so that step 1 puts m' or v' of it ON an edge of the guard
# 0 < v' < 2^62, 2^-50 <= |m'| < 2^30; the other 63 lanes are ordinary.  The seeded elements have p = 0, so the step's
# gradient fma(2 l2, p, 0) is 0 whatever l2 is, m' = fma(w1, -m, m) and v' = RN(b2 v): both move by less than one ulp per
# ulp of the seed, so every float near the edge is reached, and the seed is found by walking ulps on the host.  That step 1
# lands where it should is asserted on the sweep's own state.
EDGES = ("v_zero", "v_denormal", "v_below_2^62", "v_at_2^62", "m_below_2^-50", "m_at_2^-50", "m_below_2^30", "m_at_2^30",
         "m_minus_zero", "m_negative_at_2^30")
EDGE_N = len(EDGES) * 64 * 4
EDGE_T = 3


def _fma32(a, b, c):
    """fmaf on float32 values (the product of two floats is exact in float64; the sum is within 2^-53 of exact, far from
    any float32 midpoint for the values walked here -- and the landing is asserted on the device anyway)."""
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def _seed_for(edge, step1, slope, at):
    """-> (x, step1(x)) with step1(x) == edge (`at`), else with step1(x) the largest value below `edge` that step 1 can
    give (the seeds of an edge at a power of two lie in the binade above it, where an ulp is two of the ulps below the
    edge), by walking ulps from edge / slope."""
    up, down = F32(np.inf), F32(-np.inf)
    x = F32(np.float64(edge) / slope)
    for _ in range(64):
        if step1(x) < edge:
            break
        x = np.nextafter(x, down, dtype=F32)
    for _ in range(64):                                 # the largest x whose image is still below the edge
        nx = np.nextafter(x, up, dtype=F32)
        if not step1(nx) < edge:
            break
        x = nx
    assert step1(x) < edge and not step1(np.nextafter(x, up, dtype=F32)) < edge
    if at:
        x = np.nextafter(x, up, dtype=F32)
        assert step1(x) == edge, "step 1 cannot land on %r" % edge
    return x, step1(x)


def _edge_state():
    _, b1, b2, _ = R.HYPER[HP]
    w1, b2f = F32(1.0 - b1), F32(b2)
    m1 = lambda m: _fma32(w1, -m, m)
    v1 = lambda v: F32(b2f * v)
    (p, m, v), = _state([EDGE_N], 77)
    want = {}
    for w, edge in enumerate(EDGES):
        e = 4 * (64 * w + 17)
        p[e] = 0.0
        if edge == "v_zero":
            v[e], want[edge] = 0.0, ("v", F32(0))
        elif edge == "v_denormal":
            v[e], want[edge] = F32(1e-40), ("v", v1(F32(1e-40)))
        elif edge.startswith("v_"):
            v[e], y = _seed_for(F32(2.0 ** 62), v1, 0.999, "at" in edge)
            want[edge] = ("v", y)
        elif edge == "m_minus_zero":
            m[e], want[edge] = F32(-0.0), ("m", F32(0.0))
        else:
            x, y = _seed_for(F32(2.0 ** (30 if "2^30" in edge else -50)), m1, 0.9, "at" in edge)
            sign = F32(-1.0 if "negative" in edge else 1.0)
            m[e], want[edge] = sign * x, ("m", sign * y)
        if "2^30" in edge:
            v[e] = F32(2.0 ** 60)                       # a large denominator: the weight stays small, and with it the L2 value
    return [(p, m, v)], want


@pytest.mark.parametrize("l2", L2_ALL)
def test_a_step_on_each_edge_of_the_guard(l2):
    """The whole tensor -- every wave holds one chunk on an edge -- flushed from `last` = 0 over EDGE_T steps, and from
    random `last` bytes: the sweep's bits."""
    dev = _dev()
    state, want = _edge_state()
    ref = _sweep(("edge", l2), state, l2, EDGE_T)
    for w, edge in enumerate(EDGES):                    # step 1 of the sweep landed on the edge
        a, x = want[edge]
        got = ref["snap"][0][1 if a == "m" else 2][1][4 * (64 * w + 17)]
        assert got.view(np.uint32) == F32(x).view(np.uint32), (edge, got, x)
    assert v_is_denormal(ref["snap"][0][2][1][4 * (64 * 1 + 17)])
    for pattern in ("zero", "random"):
        rng = np.random.RandomState(5)
        last = _last(pattern, EDGE_N // 4, EDGE_T, rng)
        last[17::64] = 0                                # the seeded chunks always replay step 1
        bank = R.Bank([_compose(ref, 0, last)], dev)
        bank.last[0][:last.size].copy_(torch.from_numpy(last))
        clk = _clock(EDGE_T)
        R.adam_flush(bank, [0], [l2], clk, HP)
        torch.cuda.synchronize()
        what = "guard edges, l2=%g %s" % (l2, pattern)
        _check_state(bank, 0, ref, 0, EDGE_T, what)
        assert not bool(bank.last[0].any()), what
        got, want_l2 = clk.take_backlog(), _owed_l2(ref, 0, last, EDGE_T, l2)
        print("%s: backlog %.9g float64 %.9g" % (what, got, want_l2))
        assert (got == 0.0) if want_l2 == 0.0 else abs(got - want_l2) <= 1e-5 * want_l2, what


def v_is_denormal(x):
    return 0.0 < float(x) < float(np.finfo(F32).tiny)


# --------------------------------------------------------------------------------------------- the catch-up of rows
ROWS_V, ROWS_B, ROWS_T = 256, 96, (1, 3, 64)
ROWS_D = {"by_row_D16": (16, 1), "by_chunk_D16": (16, 0), "by_chunk_D6": (6, 1)}     # D, option "adam_rows"


@pytest.mark.parametrize("pattern", ("zero", "random"))
@pytest.mark.parametrize("l2", L2_ALL)
@pytest.mark.parametrize("t", ROWS_T)
@pytest.mark.parametrize("case", sorted(ROWS_D))
def test_catchup_rows_gives_the_sweeps_bits(case, t, l2, pattern):
    """xdfm_adam_catchup_rows on one table [256, D]: the chunks of the 96 gathered rows (duplicates, id 0 and id V - 1
    among them) reach the sweep's state after step t and carry last == t; every other chunk keeps its state and its byte."""
    from xdfm_amd import _lib
    dev = _dev()
    D, opt = ROWS_D[case]
    n = ROWS_V * D
    ref = _sweep(("rows", D, l2), _state([n], 40 + D), l2, max(ROWS_T))
    rng = np.random.RandomState(100 * t + D)
    last = _last(pattern, n // 4, t, rng)
    ids = np.minimum((ROWS_V * rng.rand(ROWS_B) ** 2).astype(np.int64), ROWS_V - 1)
    ids[0], ids[1] = 0, ROWS_V - 1
    claimed = np.zeros(n // 4, dtype=bool)
    for i in np.unique(ids):
        claimed[i * D // 4:(i * D + D - 1) // 4 + 1] = True
    bank = R.Bank([_compose(ref, 0, last)], dev)
    bank.last[0][:last.size].copy_(torch.from_numpy(last))
    clk = _clock(t)
    X = torch.from_numpy(ids.astype(F32).reshape(-1, 1)).to(dev)
    cols = torch.zeros(1, dtype=torch.int32, device=dev)
    vocab = torch.tensor([ROWS_V], dtype=torch.int32, device=dev)
    emb = R.Rows(bank, [0], [l2], with_grads=False)
    before = _lib.get_option("adam_rows")
    _lib.set_option("adam_rows", opt)
    try:
        R.adam_catchup_rows(X, cols, vocab, 1, D, emb, None, clk, HP)
        assert _lib.get_option("last_adam_rows") == (1 if case == "by_row_D16" else 0)
    finally:
        _lib.set_option("adam_rows", before)
    torch.cuda.synchronize()
    what = "catch-up %s, t=%d l2=%g %s" % (case, t, l2, pattern)
    want_last = np.where(claimed, t, last).astype(np.uint8)
    want = _compose(ref, 0, want_last)
    for name, arr, a in (("p", bank.p, 0), ("m", bank.m, 1), ("v", bank.v, 2)):
        assert _same_bits(arr[0], want[a]), "%s: %s" % (what, name)
    assert np.array_equal(bank.last[0][:last.size].cpu().numpy(), want_last), what
    assert clk.read() == [t, 0], what
    _check_backlog(clk.take_backlog(), _owed_l2(ref, 0, last, t, l2, chunks=claimed), None, what)
