"""GPU tests (-m gpu) of the SGD / Adagrad / RMSprop kernels at the C ABI (K7s / K7g / K7r: csrc/sgd_adagrad.hip; K7sd /
K7gd / K7rd: csrc/sgd_adagrad_deferred.hip; the element update: csrc/opt_math.h) against numpy float64 (tests/opt_ref.py:
opt_f64, tied to torch by test_opt_reference.py) and, where two paths of the kernels must agree, bit for bit against the
path that float64 is tied to.  Sizes, hyper-parameter sets and planted chunks are those of opt_ref.py; DESIGN.md ("The SGD /
Adagrad / RMSprop kernel tests") lists which case reaches which loop of the kernels and the measured shares of the bars.

Bars against float64 (those of test_gpu_optim.py / test_gpu_adam.py): p rtol 2e-6 / atol 1e-8, accumulator 2e-6 / 1e-10, L2
value 1e-5 relative.  Every array a kernel may write lies between guard cells that the drivers check after every call."""
import contextlib

import numpy as np
import pytest
import torch

import opt_ref as R

pytestmark = pytest.mark.gpu
BX = pytest.mark.parametrize("bx", [0, 1], ids=["bx_default", "bx1"])
KIND = pytest.mark.parametrize("kind", R.KINDS)
N = len(R.SIZES)
ALL = list(range(N))
NAN_BITS = 0x7FC00000


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def _opt_bx(value):
    """Option "opt_bx" = most blocks one tensor gets (0: the defaults, 512 / 512 / 4096).  At 1 a tensor is one block: the
    40989 and 1 120 016 element tensors run many iterations of every unrolled loop and of the scan's paired-group loop."""
    from xdfm_amd import _lib
    before = _lib.get_option("opt_bx")
    _lib.set_option("opt_bx", value)
    try:
        yield
    finally:
        _lib.set_option("opt_bx", before)


def _i32(t):
    return t.view(torch.int32)


def _same_bits(a, b, sel=None):
    a, b = _i32(a), _i32(b)
    if sel is not None:
        a, b = a[sel], b[sel]
    return torch.equal(a, b)


def _assert_banks_equal(x, y, what, tensors=None):
    for t in (range(len(x.sizes)) if tensors is None else tensors):
        for name, xa, ya in (("p", x.p, y.p), ("s", x.s, y.s)):
            if not _same_bits(xa[t], ya[t]):
                bad = torch.nonzero(_i32(xa[t]) != _i32(ya[t])).flatten()
                raise AssertionError("%s: %s of tensor %d (%d elements) differs in %d elements, first at %d" % (
                    what, name, t, x.sizes[t], bad.numel(), int(bad[0])))


def _check_mark_pointers(bank, want=None):
    mods = [bank.mark_ptr(t) % 16 for t in range(len(bank.sizes))]
    if want is not None:
        assert mods == want, mods
    assert len(set(mods)) >= 3 and 0 in mods, mods


def _elem_sel(mask, n, dev, tail=True):
    """Element indices of the chunks of `mask`, plus (tail) the numel % 4 tail."""
    sel = np.repeat(mask, 4)
    sel = np.concatenate([sel, np.full(n - sel.size, tail, dtype=bool)])
    return torch.from_numpy(np.nonzero(sel)[0]).to(dev)


_F64 = {}


def _f64(key, kind, h, state, sizes, grads_of, l2, steps, lr_fn):
    if key not in _F64:
        _F64[key] = R.run_ref(R.opt_f64, kind, h, state, sizes, grads_of, l2, steps, lr_fn, np.float64)
    return _F64[key]


def _print_shares(what, sh):
    print("%s: share of the bar %s" % (what, " ".join("%s %.3f" % kv for kv in sorted(sh.items()))))


def _fixed_atol(count):
    """Every thread that stepped or replayed something truncates its l2-weighted sum of squares once, to a multiple of 2^-40."""
    return count / R.FIX


# --------------------------------------------------------------------------------------------- (a)
@BX
@pytest.mark.parametrize("kind,hp", R.CASES_F64)
def test_dense_sweep_vs_float64(kind, hp, bx):
    """Six steps of xdfm_sgd_step / _adagrad_step / _rmsprop_step over all seven sizes with fresh dense gradients (every 7th
    element zero, scale alternating 0.1 / 1e-3), L2 1e-3 / 0 / 5e-2 on the first three tensors, l2_value on odd steps: p
    and the accumulator against opt_f64 carried in float64 from the same fp32 start, l2_value against the float64 sum.  S1
    sends the rate through lr_dev (0 for steps 1-3): until then p keeps its bits where l2 == 0."""
    dev = _dev()
    h = R.hyper(kind, hp)
    state = R.make_state(h)
    lr_fn = lambda s: R.lr_of(hp, s)[0]
    want, want_l2 = _f64(("a", hp), kind, h, state, R.SIZES, lambda s: R.dense_grads(R.SIZES, s), R.L2_A, 6, lr_fn)
    with _opt_bx(bx):
        bank, start = R.Bank(kind, state, dev), R.Bank(kind, state, dev)
        got_l2 = {}
        for s in range(1, 7):
            flat, _ = R.dense_grads(R.SIZES, s)
            bank.set_grads(flat)
            lr, through_dev = R.lr_of(hp, s)
            out = R.opt_step(bank, ALL, R.L2_A, h, lr, lr_dev=through_dev, want_l2=bool(s % 2))
            if s % 2:
                got_l2[s] = float(out[0])
            assert np.array_equal(bank.flat.cpu().numpy(), flat), "a dense gradient was written to"
            if hp == "S1" and s <= 3:
                for t in ALL:
                    assert R.L2_A[t] != 0 or _same_bits(bank.p[t], start.p[t]), "lr_dev = 0, step %d, tensor %d" % (s, t)
        got = bank.snapshot()
    sh = R.shares_of(kind, got, want)
    sh["l2"] = max(abs(got_l2[s] - want_l2[s - 1]) / (R.L2_RTOL * want_l2[s - 1]) for s in got_l2)
    _print_shares("opt dense %s %s bx=%d" % (kind, hp, bx), sh)
    assert all(x <= 1.0 for x in sh.values()), sh


# --------------------------------------------------------------------------------------------- (b)
@KIND
def test_unaligned_tensors_take_the_scalar_path(kind):
    """Three steps on the values of (a) (the kind's first set), once with every pointer 16-byte aligned and once with each of
    p, g and the accumulator one float past an aligned address (`vec == false`: the whole tensor goes through the tail loop):
    within the bars of float64 and bit-identical to the aligned run.  grad_marks with such a pointer is refused
    (XDFM_ERR_INVALID) before any device work: state, gradient, marks and guards untouched."""
    dev = _dev()
    h = R.hyper(kind, "base")
    hp = R.BASE[kind]
    state = R.make_state(h)
    want, _ = _f64(("b", hp), kind, h, state, R.SIZES, lambda s: R.dense_grads(R.SIZES, s), R.L2_A, 3, lambda s: h["lr"])

    def run(mis):
        bank = R.Bank(kind, state, dev, mis=mis)
        for s in range(1, 4):
            flat, _ = R.dense_grads(R.SIZES, s)
            bank.set_grads(flat)
            R.opt_step(bank, ALL, R.L2_A, h, h["lr"], want_l2=bool(s % 2))
        return bank

    aligned = run(None)
    for which in ("pgs" if kind != "sgd" else "pg"):
        other = run({which: 1})
        ptr = {"p": other.p[0], "g": other.flat, "s": other.s[0]}[which].data_ptr()
        assert ptr % 16 == 4
        _assert_banks_equal(aligned, other, "%s one float off" % which)
        sh = R.shares_of(kind, other.snapshot(), want)
        _print_shares("opt scalar path %s, %s one float off" % (kind, which), sh)
        assert all(x <= 1.0 for x in sh.values()), sh
        # marks need aligned pointers
        flat, marks, _, _ = R.sparse_grads(R.SIZES, ["all"] * N, 4)
        other.set_grads(flat, marks)
        before = other.snapshot()
        rc = R.opt_step(other, ALL, R.L2_A, h, h["lr"], marked=True, want_l2=True, check=False)
        assert rc == R.ERR_INVALID
        after = other.snapshot()
        for t in ALL:
            assert np.array_equal(R.bits(before[t][0]), R.bits(after[t][0])) and np.array_equal(R.bits(before[t][1]), R.bits(after[t][1]))
        assert np.array_equal(other.flat.cpu().numpy(), flat) and np.array_equal(other.marks.cpu().numpy(), marks)


# --------------------------------------------------------------------------------------------- (c)
# mark pattern and L2 strength per tensor.  "l2_A": the two large tensors have an L2 term and take the `else if (marks)` branch,
# the small ones the scan.  "no_l2": every tensor takes the scan (SGD, Adagrad) -- at opt_bx 1 the 1 120 016- and the
# 40989-element tensor have 17500 / 639 groups of 16 mark bytes for 256 threads: the paired-group loop runs 34 times / once
CASES_C = {"l2_A": (["random3", "all", "ends", "tail", "none", "tail", "random3"], R.L2_A),
           "no_l2": (["random3", "all", "random3", "tail", "none", "ends", "all"], [0.0] * N)}
MARK_MODS = [0, 4, 5, 13, 14, 15, 0]


@BX
@pytest.mark.parametrize("case", sorted(CASES_C))
@KIND
def test_marked_gradients_match_dense_and_unmarked_chunks_are_not_read(kind, case, bx):
    """Two steps with the same mark pattern per tensor (3 % random chunks / all / first and last / only the tail / none) and
    fresh values.  The marked call sees a NaN in the gradient of every unmarked chunk (the header: unmarked chunks are not
    read), the dense call zeros there: p, the accumulator and the L2 value have the same bits; afterwards the marked
    gradient chunks, the tails and all mark bytes are zero and every NaN is still there.  l2 == 0: unmarked chunks of p
    keep their bits, the accumulator's too (SGD, Adagrad) or becomes fl32(fl32(alpha) * v) per step (RMSprop)."""
    dev = _dev()
    h = R.hyper(kind, "base")
    state = R.make_state(h)
    kinds_c, l2 = CASES_C[case]
    masks = None
    with _opt_bx(bx):
        dense, marked = R.Bank(kind, state, dev), R.Bank(kind, state, dev)
        _check_mark_pointers(marked, MARK_MODS)
        for s in (1, 2):
            flat, marks, masks, offs = R.sparse_grads(R.SIZES, kinds_c, s, chunks=masks)
            dense.set_grads(flat)
            vd = R.opt_step(dense, ALL, l2, h, h["lr"], want_l2=True)
            assert np.array_equal(dense.flat.cpu().numpy(), flat), "the dense run wrote to its gradient"
            poisoned = R.bits(flat).copy()
            after = np.zeros_like(poisoned)
            for t, n in enumerate(R.SIZES):
                un = np.nonzero(np.repeat(~masks[t], 4))[0] + offs[t]
                poisoned[un] = NAN_BITS
                after[un] = NAN_BITS
            marked.set_grads(poisoned.view(np.float32), marks)
            vm = R.opt_step(marked, ALL, l2, h, h["lr"], marked=True, want_l2=True)
            assert np.array_equal(R.bits(marked.flat.cpu().numpy()), after), "step %d: gradient not re-zeroed, or a NaN gone" % s
            assert not bool(marked.marks.any()), "step %d: marks not cleared" % s
            assert R.bits(vd)[0] == R.bits(vm)[0], (float(vd[0]), float(vm[0]))
            _assert_banks_equal(dense, marked, "marked against dense, step %d" % s)
    assert sum(int(k.sum()) for k in masks) > 8000 and not masks[3].size and not masks[4].any() and masks[1].all()
    assert (float(vd[0]) > 0) == (case == "l2_A")
    al = R.F32(h["alpha"])
    for t, n in enumerate(R.SIZES):
        p, v = marked.get(t)
        assert np.isfinite(p).all() and np.isfinite(v).all()
        if l2[t] == 0:
            rest = np.nonzero(np.repeat(~masks[t], 4))[0]
            assert np.array_equal(R.bits(p[rest]), R.bits(state[t][0][rest])), "an unmarked chunk of p moved, tensor %d" % t
            if kind != "sgd":
                v0 = state[t][1][rest]
                want_v = (al * (al * v0).astype(R.F32)).astype(R.F32) if kind == "rmsprop" else v0
                assert np.array_equal(R.bits(v[rest]), R.bits(want_v)), "the accumulator of an unmarked chunk, tensor %d" % t


# --------------------------------------------------------------------------------------------- (d)
SIZES_D = [(3, 67, 4099)[k % 3] for k in range(100)]


def _l2_d(T, which):
    """L2 strengths of the first T tensors: a third of them ("third": every third of each size) or two thirds."""
    on = (lambda k: (k // 3) % 3 == 0) if which == "third" else (lambda k: (k // 3) % 3 != 0)
    return [float(R.F32(1e-4 * (1 + (k * 7) % 13))) if on(k) else 0.0 for k in range(T)]


@KIND
def test_more_tensors_than_a_launch_holds(kind):
    """70 tensors (sizes cycling through 3, 67, 4099; a third with an L2 term) in one sweep call: two launches, the second
    one's L2 partials behind the first one's (`slot0`), one finish over both.  100 tensors with an L2 term on two thirds of
    them (66 deferred: more than the 48 a deferred launch holds; with a third it would be 33) in one deferred call and one
    flush: two scan launches, two flush launches, the other 34 through the sweep.  p and the accumulator bit-equal to one
    sweep call per tensor, l2_value (plus the backlog) against float64."""
    dev = _dev()
    h = R.hyper(kind, "base")
    for T, which, deferred in ((70, "third", False), (100, "two thirds", True)):
        sizes, l2 = SIZES_D[:T], _l2_d(T, which)
        idx = list(range(T))
        state = R.make_state(h, sizes, seed=11)
        is_def = [x > 0 for x in l2]
        assert sum(is_def) > 48 or not deferred
        grads = lambda s: R.sparse_grads(sizes, ["random3"] * T, s, seed=12)
        want, want_l2 = _f64(("d", kind, T), kind, h, state, sizes, lambda s: (grads(s)[0], grads(s)[3]), l2, 2, lambda s: h["lr"])
        one, single = R.Bank(kind, state, dev), R.Bank(kind, state, dev)
        total = 0.0
        for s in (1, 2):
            flat, marks, masks, _ = grads(s)
            one.set_grads(flat, marks)
            v = R.opt_step(one, idx, l2, h, h["lr"], marked=True, want_l2=True, deferred=is_def if deferred else None)
            total += float(v[0])
            assert not bool(one.flat.any()) and not bool(one.marks.any())
            if not deferred:
                assert abs(float(v[0]) - want_l2[s - 1]) <= R.L2_RTOL * want_l2[s - 1], (float(v[0]), want_l2[s - 1])
            single.set_grads(flat, marks)
            for t in idx:
                R.opt_step(single, [t], [l2[t]], h, h["lr"], marked=True)
        if deferred:
            assert one.read_clock() == [2, 0]
            dt = [t for t in idx if is_def[t]]
            R.opt_flush(one, dt, [l2[t] for t in dt], h)
            total += one.take_backlog()
            # per step at most two truncations per chunk (this step's and the replayed steps' squares) and one per tail element
            count = sum(2 * (2 * (sizes[t] // 4) + sizes[t] % 4) + sizes[t] // 4 for t in dt)
            assert abs(total - sum(want_l2)) <= R.L2_RTOL * sum(want_l2) + _fixed_atol(count), (total, sum(want_l2))
            assert one.read_clock() == [0, 2] and all(not bool(one.last[t].any()) for t in idx)
        _assert_banks_equal(one, single, "%d tensors in one call against one call per tensor" % T)
        _print_shares("opt %s %d tensors (printed only: the bit-equality ties them to (a))" % (kind, T),
                      R.shares_of(kind, one.snapshot(), want))


# --------------------------------------------------------------------------------------------- (e)
E_BEFORE = 5
E_DEF = [x > 0 for x in R.L2_A]            # the tensors with an L2 term are deferred, the others have no `last`


def _masks_e(step, sizes=R.SIZES, never=False, rate=0.03):
    """`rate` of the chunks drawn per step; the four planted chunks (near the start and in the middle) are marked at steps 4
    and 9 only -- the step's own replay brings them up -- or never (the flush does)."""
    out = []
    for t, n in enumerate(sizes):
        k = np.random.RandomState(1000 * step + t).rand(n // 4) < rate
        for c in R.planted_chunks(n):
            k[c:c + 4] = (not never) and step in (4, 9)
        out.append(k)
    return out


def _last_of(bank, t):
    return bank.last[t].cpu().numpy()


def _check_rates(bank, h, steps, lr_fn):
    got = R.bits(bank.rates.cpu().numpy())
    want = R.bits(np.array([-R.F32(lr_fn(s)) for s in steps], R.F32))
    assert np.array_equal(got[1:1 + len(steps)], want), "rates[1 .. t] are not the bits of -(float)lr"


@BX
@pytest.mark.parametrize("hp", ["base", "L"])
@KIND
def test_deferred_steps_and_flush_match_the_sweep(kind, hp, bx):
    """Bank A takes twelve sweep steps over marked sparse gradients; bank B defers its two tensors with an L2 term (cap 16),
    takes the same steps and is flushed once at the end, with no catch-up: every marked chunk replays what it missed inside
    `process`.  The rate goes through lr_dev, different every step, 0 at steps 3 and 8.  After every step: clock ==
    {t, before}, rates[1 .. t] the bits of -(float)lr_s, cell == 0, last[e] == the latest step that marked e (0: never) and
    the chunks with last == 0 hold the starting bits.  After the flush: all of p and the accumulator bit-equal to A (and,
    except L, within the bars of float64), every `last` byte 0, clock == {0, before + 12}, and the window's sum of l2_value
    plus the backlog equal to float64's sum of the sweep's values to 1e-5 plus 2^-40 per truncation."""
    dev = _dev()
    h = R.hyper(kind, hp)
    state = R.make_state(h)
    lr_fn = lambda s: R.lr_sched(h, s)
    grads = lambda s: R.sparse_grads(R.SIZES, None, s, seed=9, chunks=_masks_e(s))
    dt = [t for t in ALL if E_DEF[t]]
    total, count = 0.0, 0
    with _opt_bx(bx):
        A, B, start = (R.Bank(kind, state, dev, before=E_BEFORE) for _ in range(3))
        _check_mark_pointers(B, MARK_MODS)
        latest = [np.zeros(n // 4 + 4, np.uint8) for n in R.SIZES]
        for s in range(1, 13):
            flat, marks, masks, _ = grads(s)
            A.set_grads(flat, marks)
            R.opt_step(A, ALL, R.L2_A, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True)
            B.set_grads(flat, marks)
            v = R.opt_step(B, ALL, R.L2_A, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True, deferred=E_DEF)
            total += float(v[0])
            assert B.read_clock() == [s, E_BEFORE] and int(B.cell.item()) == 0
            _check_rates(B, h, range(1, s + 1), lr_fn)
            assert not bool(B.flat.any()) and not bool(B.marks.any()), "step %d: gradient / marks not re-zeroed" % s
            for t in ALL:
                n = R.SIZES[t]
                if E_DEF[t]:
                    latest[t][:n // 4][masks[t]] = s
                    count += 2 * int(masks[t].sum()) + n % 4
                    assert np.array_equal(_last_of(B, t), latest[t]), "step %d: `last` of tensor %d" % (s, t)
                    sel = _elem_sel(masks[t], n, dev)
                    assert _same_bits(B.p[t], A.p[t], sel) and _same_bits(B.s[t], A.s[t], sel), "step %d: marked chunks, tensor %d" % (s, t)
                    rest = _elem_sel(latest[t][:n // 4] == 0, n, dev, tail=False)
                    assert _same_bits(B.p[t], start.p[t], rest) and _same_bits(B.s[t], start.s[t], rest), \
                        "step %d: a chunk with last == 0 moved, tensor %d" % (s, t)
                else:
                    assert not _last_of(B, t).any()
            _assert_banks_equal(A, B, "step %d, the tensors that are not deferred" % s, [t for t in ALL if not E_DEF[t]])
        R.opt_flush(B, dt, [R.L2_A[t] for t in dt], h)
        count += sum(R.SIZES[t] // 4 for t in dt)
        total += B.take_backlog()
        _assert_banks_equal(A, B, "after the flush")
        assert all(not bool(x.any()) for x in B.last), "a `last` byte survived the flush"
        assert B.read_clock() == [0, E_BEFORE + 12] and int(B.cell.item()) == 0
        assert sum(int((x == 12).sum()) for x in latest) > 0
    want, want_l2 = _f64(("e", kind, hp), kind, h, state, R.SIZES, lambda s: (grads(s)[0], grads(s)[3]), R.L2_A, 12, lr_fn)
    got = B.snapshot()
    assert all(np.isfinite(p).all() and np.isfinite(v).all() for p, v in got)
    sh = R.shares_of(kind, got, want)
    sh["l2sum"] = abs(total - sum(want_l2)) / (R.L2_RTOL * sum(want_l2) + _fixed_atol(count))
    _print_shares("opt deferred %s %s bx=%d" % (kind, hp, bx), sh)
    if hp == "L":
        assert sh["l2sum"] <= 1.0, sh
    else:
        assert all(x <= 1.0 for x in sh.values()), sh


# --------------------------------------------------------------------------------------------- (f)
F_VOCAB = (5000, 31, 20003, 3)
F_B, F_M, F_LDX, F_COLS = 300, 4, 7, (4, 0, 2, 5)
F_L2_EMB, F_L2_LIN = [1e-3, 2e-3, 5e-2, 1e-2], [1e-2, 1e-3, 2e-3, 3e-3]
F_SKIP = 1                               # this field's `param` pointer is NULL in xdfm_opt_rows: not deferred
F_STEPS = 6


def _batch_f(step):
    """X [B, ldx] and the clamped ids per field.  Per field: one id 64 times in a row, the four neighbours id .. id + 3, the
    last row (in the numel % 4 tail where V * D % 4 != 0) and row 0, random ids with duplicates; field 0 has an id of V + 5
    and field 2 one of -1 (clamped, as the gather); field 3's ids carry a fraction (truncated)."""
    rng = np.random.RandomState(4000 + step)
    X = rng.rand(F_B, F_LDX).astype(np.float32)
    ids = []
    for f, V in enumerate(F_VOCAB):
        i = np.minimum((V * rng.rand(F_B) ** 2).astype(np.int64), V - 1)
        hot = int(rng.randint(V))
        i[10:74] = hot
        near = int(rng.randint(max(V - 3, 1)))
        i[80:84] = np.minimum(near + np.arange(4), V - 1)
        i[0], i[1] = 0, V - 1
        raw = i.astype(np.float32)
        if f == 0:
            raw[5], i[5] = V + 5, V - 1
        if f == 2:
            raw[6], i[6] = -1, 0
        X[:, F_COLS[f]] = raw + (0.25 if f == 3 else 0.0)
        ids.append(i)
    return X, ids


def _extra_f(step):
    """A few rows per field that get a gradient in `step` without being in its batch (no catch-up announced them)."""
    rng = np.random.RandomState(7000 + step)
    _, ids = _batch_f(step)
    out = []
    for f, V in enumerate(F_VOCAB):
        cand = rng.randint(V, size=5)
        out.append(np.array([c for c in cand if c not in ids[f]], dtype=np.int64))
    return out


def _row_chunks(ids, w, n):
    """Boolean [n // 4 + 1]: the chunks that the rows `ids` of width w touch (the last entry: the numel % 4 tail)."""
    mk = np.zeros(n // 4 + 1, dtype=bool)
    for i in np.unique(ids):
        mk[i * w // 4:min((i * w + w - 1) // 4, n // 4) + 1] = True
    return mk


def _case_f(kind, D, with_lin, dev):
    h = R.hyper(kind, "base")
    lr_fn = lambda s: R.lr_sched(h, s + 1)            # 0 at steps 2 and 7 of this schedule: step 2 is inside the window
    sizes = [V * D for V in F_VOCAB] + (list(F_VOCAB) if with_lin else [])
    l2 = F_L2_EMB + (F_L2_LIN if with_lin else [])
    T = len(sizes)
    idx = list(range(T))
    width = [D] * 4 + [1] * (T - 4)
    is_def = [t % 4 != F_SKIP for t in idx]
    dt = [t for t in idx if is_def[t]]
    state = R.make_state(h, sizes, seed=21)
    A, B, start = (R.Bank(kind, state, dev) for _ in range(3))
    cols = torch.tensor(F_COLS, dtype=torch.int32, device=dev)
    vocab = torch.tensor(F_VOCAB, dtype=torch.int32, device=dev)
    emb = R.Rows(B, idx[:4], F_L2_EMB, skip=(F_SKIP,))
    lin = R.Rows(B, idx[4:], F_L2_LIN, skip=(F_SKIP,)) if with_lin else None
    QT = (D + 3) // 4 + (1 if D % 4 else 0) + (1 if with_lin else 0)
    cache = {}

    def grads(s):
        if s not in cache:
            _, ids = _batch_f(s)
            extra = _extra_f(s)
            masks = [_row_chunks(np.concatenate([ids[t % 4], extra[t % 4]]), width[t], sizes[t])[:sizes[t] // 4] for t in idx]
            cache[s] = R.sparse_grads(sizes, None, s, seed=13, chunks=masks)
        return cache[s]

    def rows_sel(t, ids):
        w = width[t]
        return torch.from_numpy((np.unique(ids)[:, None] * w + np.arange(w)[None, :]).reshape(-1)).to(dev)

    touched = [np.zeros(n // 4, dtype=bool) for n in sizes]          # chunks a batch or a gradient reached so far
    total, count = 0.0, 0
    for s in range(1, F_STEPS + 1):
        Xn, ids = _batch_f(s)
        X = torch.from_numpy(Xn).to(dev)
        assert X.stride(0) == F_LDX > F_M
        R.opt_catchup(B, X, cols, vocab, F_M, D, emb, lin, h)
        count += F_B * F_M * QT
        flat, marks, masks, _ = grads(s)
        for t in idx:
            n = sizes[t]
            touched[t] |= _row_chunks(ids[t % 4], width[t], n)[:n // 4]
            sel = rows_sel(t, ids[t % 4])
            assert _same_bits(B.p[t], A.p[t], sel) and _same_bits(B.s[t], A.s[t], sel), \
                "step %d: the batch's rows after the catch-up, tensor %d" % (s, t)
            if is_def[t]:
                rest = _elem_sel(~touched[t], n, dev, tail=False)
                assert _same_bits(B.p[t], start.p[t], rest) and _same_bits(B.s[t], start.s[t], rest), \
                    "step %d: a chunk no batch and no gradient reached has moved, tensor %d" % (s, t)
                assert (_last_of(B, t)[:n // 4][~touched[t]] == 0).all()
            touched[t] |= masks[t]
        A.set_grads(flat, marks)
        R.opt_step(A, idx, l2, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True)
        B.set_grads(flat, marks)
        v = R.opt_step(B, idx, l2, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True, deferred=is_def)
        total += float(v[0])
        count += sum(2 * int(masks[t].sum()) + sizes[t] % 4 for t in dt)
        assert B.read_clock() == [s, 0] and int(B.cell.item()) == 0
        assert not bool(B.flat.any()) and not bool(B.marks.any())
        for t in idx:
            sel = rows_sel(t, ids[t % 4])
            assert _same_bits(B.p[t], A.p[t], sel) and _same_bits(B.s[t], A.s[t], sel), \
                "step %d: the batch's rows after the step, tensor %d" % (s, t)
    _check_rates(B, h, range(1, F_STEPS + 1), lr_fn)
    R.opt_flush(B, dt, [l2[t] for t in dt], h)
    count += sum(sizes[t] // 4 for t in dt)
    total += B.take_backlog()
    _assert_banks_equal(A, B, "after the flush")
    assert all(not bool(x.any()) for x in B.last) and B.read_clock() == [0, F_STEPS]
    # a catch-up at t == 0 changes nothing
    Xn, _ = _batch_f(F_STEPS + 1)
    R.opt_catchup(B, torch.from_numpy(Xn).to(dev), cols, vocab, F_M, D, emb, lin, h)
    _assert_banks_equal(A, B, "after a catch-up at t == 0")
    assert all(not bool(x.any()) for x in B.last) and int(B.backlog.item()) == 0 and B.read_clock() == [0, F_STEPS]
    _, want_l2 = _f64(("f", kind, D, with_lin), kind, h, state, sizes, lambda s: (grads(s)[0], grads(s)[3]), l2, F_STEPS, lr_fn)
    return abs(total - sum(want_l2)) / (R.L2_RTOL * sum(want_l2) + _fixed_atol(count))


@pytest.mark.parametrize("D", [16, 10, 4, 3])
@KIND
def test_catchup_of_the_rows_a_batch_gathers(kind, D):
    """xdfm_opt_catchup_rows / xdfm_rmsprop_catchup_rows called directly: m = 4 fields of vocabulary (5000, 31, 20003, 3),
    B = 300, ldx = 7, field 1's `param` NULL (it is stepped by the sweep), with and without the linear tables.  D = 4 and
    3 (and the linear tables) put several rows into one word of `last` bytes, D = 10 and 3 rows across chunks.  Six steps of
    a different batch each -- catch-up on B; the batch's rows bit-equal to the sweep's bank A as it is after the step
    before; chunks that no batch and no gradient reached so far unchanged; the step on both (a few rows get a gradient
    without being in the batch: `process` replays them); the batch's rows equal again -- then the flush and the whole
    banks, a catch-up at t == 0 that must change nothing, and the window's L2 sum as in the deferred test."""
    dev = _dev()
    for with_lin in (True, False):
        share = _case_f(kind, D, with_lin, dev)
        print("opt rows %s D=%d lin=%d: share of the bar, L2 sum against float64 %.3f" % (kind, D, with_lin, share))
        assert share <= 1.0


# --------------------------------------------------------------------------------------------- (g)
G_IDX = [t for t in ALL if R.SIZES[t] <= 40989]
G_SIZES = [R.SIZES[t] for t in G_IDX]
# the 40989-element tensor keeps its L2 term; the tensors of 67 and 4099 elements get one too, so that more than one
# tensor -- and numel % 4 tails, which are stepped densely in every one of the 255 steps -- live through the window
G_L2 = [{40989: 5e-2, 67: 2e-3, 4099: 3e-3}.get(n, 0.0) for n in G_SIZES]
G_DEF = [x > 0 for x in G_L2]


def _run_window(kind, dev, cap, steps, flush_every, rate):
    h = R.hyper(kind, "base")
    state = R.make_state(h, G_SIZES)
    T = len(G_SIZES)
    idx = list(range(T))
    dt = [t for t in idx if G_DEF[t]]
    lr_fn = lambda s: R.lr_sched(h, s)
    A, B = R.Bank(kind, state, dev, cap=cap), R.Bank(kind, state, dev, cap=cap)
    top = 0
    for s in range(1, steps + 1):
        flat, marks, _, _ = R.sparse_grads(G_SIZES, None, s, seed=17, chunks=_masks_e(s, G_SIZES, never=True, rate=rate))
        A.set_grads(flat, marks)
        R.opt_step(A, idx, G_L2, h, lr_fn(s), lr_dev=True, marked=True)
        B.set_grads(flat, marks)
        R.opt_step(B, idx, G_L2, h, lr_fn(s), lr_dev=True, marked=True, deferred=G_DEF)
        if s % flush_every == 0:
            assert B.read_clock()[0] == flush_every < cap
            top = max(top, max(int(_last_of(B, t).max()) for t in dt))
            R.opt_flush(B, dt, [G_L2[t] for t in dt], h)
            _assert_banks_equal(A, B, "after the flush at step %d" % s)
            assert all(not bool(x.any()) for x in B.last) and B.read_clock() == [0, s]
    return top


@KIND
def test_window_of_two_steps_at_cap_3(kind):
    """cap = 3, the smallest the header allows: six steps, a flush after every second one."""
    assert _run_window(kind, _dev(), 3, 6, 2, 0.03) == 2


@KIND
def test_window_of_255_steps_at_cap_256(kind):
    """cap = 256, the largest: 255 steps without a flush on the sizes up to 40989, 0.5 % of the chunks marked per step and
    the planted chunks never: the flush replays 255 steps from last == 0 and up to 254 from the chunks marked early; `last`
    reached 255 before it.  Afterwards B is bit-equal to the sweep after 255 steps ((a) ties the sweep to float64; no bar
    exists for 255 steps)."""
    assert _run_window(kind, _dev(), 256, 255, 255, 0.005) == 255
