"""GPU tests (-m gpu) of SGD with momentum at the C ABI (K7m: csrc/sgd_adagrad.hip; K7md: csrc/sgd_adagrad_deferred.hip; the
element update: csrc/opt_math.h, OPT_SGDM) against numpy float64 (tests/sgdm_ref.py: sgdm_f64, tied to torch.optim.SGD by
test_sgdm_reference.py) and, where two paths of the kernels must agree, bit for bit.  The model is test_gpu_opt_abi.py, whose
helpers, mark patterns and batches this file reuses: sizes and planted chunks are opt_ref's, every array a kernel may write lies
between guard cells that the drivers check after every call.

Bars against float64: opt_ref.TOL (p rtol 2e-6 / atol 1e-8; the buffer on the `s` bar, 2e-6 / 1e-10), L2 value 1e-5 relative.
The float64 comparisons run on inputs with one sign per element, the bit-for-bit ones on random signs too (sgdm_ref.py, "THE
SIGNS").  Every run whose weights and buffers are compared with float64 -- (a), (b), (d), (e) -- is made on two banks that take
the same calls: the same call gives the same bits.  ((f) and (g) compare a deferred bank with a sweep bank bit for bit.)"""
import numpy as np
import pytest
import torch

import opt_ref as R
import sgdm_ref as M
import test_gpu_opt_abi as O

pytestmark = pytest.mark.gpu
BX = pytest.mark.parametrize("bx", [0, 1], ids=["bx_default", "bx1"])
N = len(M.SIZES)
ALL = list(range(N))
NAN_BITS = 0x7FC00000
_F64 = {}


def _f64(key, h, state, sizes, grads_of, l2, steps, lr_fn):
    if key not in _F64:
        _F64[key] = M.run_ref(M.sgdm_f64, h, state, sizes, grads_of, l2, steps, lr_fn, np.float64)
    return _F64[key]


def _planted_ok(bank, sizes, what):
    """The planted chunk with p = buf = 0 (and g = 0) still holds zeros, and nothing became NaN or infinite."""
    for t, n in enumerate(sizes):
        p, b = bank.get(t)
        assert np.isfinite(p).all() and np.isfinite(b).all(), "%s: tensor %d" % (what, t)
        for c in M.planted_chunks(n):
            assert not p[4 * c:4 * c + 4].any() and not b[4 * c:4 * c + 4].any(), "%s: the all-zero chunk of tensor %d moved" % (what, t)


# --------------------------------------------------------------------------------------------- (a)
@BX
@pytest.mark.parametrize("hp", M.SETS)
def test_dense_sweep_vs_float64(hp, bx):
    """Six steps of xdfm_sgdm_step over all seven sizes with fresh dense gradients, L2 1e-3 / 0 / 5e-2 on the first three
    tensors, l2_value on odd steps: p and the buffer against sgdm_f64 carried in float64 from the same fp32 start, l2_value
    against the float64 sum.  MD sends the rate through lr_dev (0 for steps 1-3): until then p keeps its bits everywhere (the
    update is fma(-0, d, p)) while the buffer already moves.  Two banks take the same calls and end with the same bits."""
    dev = O._dev()
    h = M.HYPER[hp]
    state = M.make_state()
    signs = M.signs_of(state)
    lr_fn = lambda s: M.lr_of(hp, s)[0]
    want, want_l2 = _f64(("a", hp), h, state, M.SIZES, lambda s: M.dense_grads(M.SIZES, s, signs=signs), M.L2_A, 6, lr_fn)
    with O._opt_bx(bx):
        bank, twin, start = (M.bank(state, dev) for _ in range(3))
        got_l2 = {}
        for s in range(1, 7):
            flat, _ = M.dense_grads(M.SIZES, s, signs=signs)
            lr, through_dev = M.lr_of(hp, s)
            for b in (bank, twin):
                b.set_grads(flat)
                out = M.sgdm_step(b, ALL, M.L2_A, h, lr, lr_dev=through_dev, want_l2=bool(s % 2))
            if s % 2:
                got_l2[s] = float(out[0])
            assert np.array_equal(bank.flat.cpu().numpy(), flat), "a dense gradient was written to"
            if hp == "MD" and s <= 3:
                for t in ALL:
                    assert O._same_bits(bank.p[t], start.p[t]), "lr_dev = 0, step %d, tensor %d" % (s, t)
                assert not O._same_bits(bank.s[0], start.s[0]), "the buffer stood still"
        O._assert_banks_equal(bank, twin, "the same calls twice")
        got = bank.snapshot()
        _planted_ok(bank, M.SIZES, "dense sweep")
    sh = M.shares_of(got, want)
    sh["l2"] = max(abs(got_l2[s] - want_l2[s - 1]) / (R.L2_RTOL * want_l2[s - 1]) for s in got_l2)
    O._print_shares("sgdm dense %s bx=%d" % (hp, bx), sh)
    assert all(x <= 1.0 for x in sh.values()), sh


# --------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("hp", ["M0", "M1"])
def test_unaligned_tensors_take_the_scalar_path(hp):
    """Three steps on the values of (a), once with every pointer 16-byte aligned and once with each of p, g and the buffer one
    float past an aligned address (the whole tensor goes through the tail loop): within the bars of float64 and bit-identical
    to the aligned run.  grad_marks with such a pointer is refused (XDFM_ERR_INVALID) before any device work."""
    dev = O._dev()
    h = M.HYPER[hp]
    state = M.make_state()
    signs = M.signs_of(state)
    want, _ = _f64(("b", hp), h, state, M.SIZES, lambda s: M.dense_grads(M.SIZES, s, signs=signs), M.L2_A, 3, lambda s: h["lr"])

    def run(mis):
        bank = M.bank(state, dev, mis=mis)
        for s in range(1, 4):
            flat, _ = M.dense_grads(M.SIZES, s, signs=signs)
            bank.set_grads(flat)
            M.sgdm_step(bank, ALL, M.L2_A, h, h["lr"], want_l2=bool(s % 2))
        return bank

    aligned = run(None)
    O._assert_banks_equal(aligned, run(None), "the same calls twice")
    for which in "pgs":
        other = run({which: 1})
        ptr = {"p": other.p[0], "g": other.flat, "s": other.s[0]}[which].data_ptr()
        assert ptr % 16 == 4
        O._assert_banks_equal(aligned, other, "%s one float off" % which)
        sh = M.shares_of(other.snapshot(), want)
        O._print_shares("sgdm scalar path %s, %s one float off" % (hp, which), sh)
        assert all(x <= 1.0 for x in sh.values()), sh
        flat, marks, _, _ = M.sparse_grads(M.SIZES, ["all"] * N, 4)
        other.set_grads(flat, marks)
        before = other.snapshot()
        rc = M.sgdm_step(other, ALL, M.L2_A, h, h["lr"], marked=True, want_l2=True, check=False)
        assert rc == R.ERR_INVALID
        after = other.snapshot()
        for t in ALL:
            assert np.array_equal(R.bits(before[t][0]), R.bits(after[t][0])) and np.array_equal(R.bits(before[t][1]), R.bits(after[t][1]))
        assert np.array_equal(other.flat.cpu().numpy(), flat) and np.array_equal(other.marks.cpu().numpy(), marks)


# --------------------------------------------------------------------------------------------- (c)
@BX
@pytest.mark.parametrize("case", sorted(O.CASES_C))
@pytest.mark.parametrize("hp", ["M0", "L"])
def test_marked_gradients_match_dense_and_every_unmarked_chunk_moves(hp, case, bx):
    """Two steps with the same mark pattern per tensor and fresh values, random signs.  The marked call sees a NaN in the
    gradient of every unmarked chunk (unmarked chunks are not read), the dense call zeros there: p, the buffer and the L2 value
    have the same bits; afterwards the marked gradient chunks, the tails and all mark bytes are zero and every NaN is still
    there.  No shortcut: in a tensor WITHOUT an L2 term the buffer of an unmarked chunk is fl(mu fl(mu buf)) after the two
    steps and its weight has moved wherever the buffer can move it -- an instance of K7s' skip would leave both alone."""
    dev = O._dev()
    h = M.HYPER[hp]
    state = M.make_state(aligned=False)
    kinds_c, l2 = O.CASES_C[case]
    masks = None
    with O._opt_bx(bx):
        dense, marked = M.bank(state, dev), M.bank(state, dev)
        O._check_mark_pointers(marked, O.MARK_MODS)
        for s in (1, 2):
            flat, marks, masks, offs = M.sparse_grads(M.SIZES, kinds_c, s, chunks=masks)
            dense.set_grads(flat)
            vd = M.sgdm_step(dense, ALL, l2, h, h["lr"], want_l2=True)
            assert np.array_equal(dense.flat.cpu().numpy(), flat), "the dense run wrote to its gradient"
            poisoned = R.bits(flat).copy()
            after = np.zeros_like(poisoned)
            for t, n in enumerate(M.SIZES):
                un = np.nonzero(np.repeat(~masks[t], 4))[0] + offs[t]
                poisoned[un] = NAN_BITS
                after[un] = NAN_BITS
            marked.set_grads(poisoned.view(np.float32), marks)
            vm = M.sgdm_step(marked, ALL, l2, h, h["lr"], marked=True, want_l2=True)
            assert np.array_equal(R.bits(marked.flat.cpu().numpy()), after), "step %d: gradient not re-zeroed, or a NaN gone" % s
            assert not bool(marked.marks.any()), "step %d: marks not cleared" % s
            assert R.bits(vd)[0] == R.bits(vm)[0], (float(vd[0]), float(vm[0]))
            O._assert_banks_equal(dense, marked, "marked against dense, step %d" % s)
    assert sum(int(k.sum()) for k in masks) > 8000 and not masks[3].size and not masks[4].any() and masks[1].all()
    assert (float(vd[0]) > 0) == (case == "l2_A")
    mu, lr = R.F32(h["mu"]), h["lr"]
    moved = 0
    for t, n in enumerate(M.SIZES):
        p, b = marked.get(t)
        assert np.isfinite(p).all() and np.isfinite(b).all()
        if l2[t] == 0:
            rest = np.nonzero(np.repeat(~masks[t], 4))[0]
            p0, b0 = state[t][0][rest], state[t][1][rest]
            assert np.array_equal(R.bits(b[rest]), R.bits((mu * (mu * b0).astype(R.F32)).astype(R.F32))), \
                "the buffer of an unmarked chunk, tensor %d" % t
            must = lr * 0.81 * np.abs(b0) > 2 * np.spacing(np.abs(p0))         # the second step alone moves p by more than an ulp
            assert (p[rest][must] != p0[must]).all(), "an unmarked chunk with a buffer stood still, tensor %d" % t
            moved += int(must.sum())
    assert moved > 1000


# --------------------------------------------------------------------------------------------- (d)
def test_more_tensors_than_a_launch_holds():
    """70 tensors in one sweep call (two launches, one finish over both) and 100 tensors with 66 deferred in one deferred call
    and one flush (two scan launches, two flush launches, the other 34 through the sweep): bit-equal to one sweep call per
    tensor; l2_value (plus the backlog) against float64."""
    dev = O._dev()
    h = M.HYPER["M1"]
    for T, which, deferred in ((70, "third", False), (100, "two thirds", True)):
        sizes, l2 = O.SIZES_D[:T], O._l2_d(T, which)
        idx = list(range(T))
        state = M.make_state(sizes, seed=11)
        signs = M.signs_of(state)
        is_def = [x > 0 for x in l2]
        assert sum(is_def) > 48 or not deferred
        grads = lambda s: M.sparse_grads(sizes, ["random3"] * T, s, seed=12, signs=signs)
        want, want_l2 = _f64(("d", T), h, state, sizes, lambda s: (grads(s)[0], grads(s)[3]), l2, 2, lambda s: h["lr"])
        one, twin, single = (M.bank(state, dev) for _ in range(3))
        total = 0.0
        for s in (1, 2):
            flat, marks, masks, _ = grads(s)
            twin.set_grads(flat, marks)
            v2 = M.sgdm_step(twin, idx, l2, h, h["lr"], marked=True, want_l2=True, deferred=is_def if deferred else None)
            one.set_grads(flat, marks)
            v = M.sgdm_step(one, idx, l2, h, h["lr"], marked=True, want_l2=True, deferred=is_def if deferred else None)
            assert R.bits(v)[0] == R.bits(v2)[0]
            total += float(v[0])
            assert not bool(one.flat.any()) and not bool(one.marks.any())
            if not deferred:
                assert abs(float(v[0]) - want_l2[s - 1]) <= R.L2_RTOL * want_l2[s - 1], (float(v[0]), want_l2[s - 1])
            single.set_grads(flat, marks)
            for t in idx:
                M.sgdm_step(single, [t], [l2[t]], h, h["lr"], marked=True)
        if deferred:
            assert one.read_clock() == [2, 0]
            dt = [t for t in idx if is_def[t]]
            M.sgdm_flush(one, dt, [l2[t] for t in dt], h)
            M.sgdm_flush(twin, dt, [l2[t] for t in dt], h)
            assert int(one.backlog.item()) == int(twin.backlog.item())
            total += one.take_backlog()
            count = sum(2 * (2 * (sizes[t] // 4) + sizes[t] % 4) + sizes[t] // 4 for t in dt)
            assert abs(total - sum(want_l2)) <= R.L2_RTOL * sum(want_l2) + O._fixed_atol(count), (total, sum(want_l2))
            assert one.read_clock() == [0, 2] and all(not bool(one.last[t].any()) for t in idx)
        O._assert_banks_equal(one, twin, "%d tensors, the same calls twice" % T)
        O._assert_banks_equal(one, single, "%d tensors in one call against one call per tensor" % T)
        sh = M.shares_of(one.snapshot(), want)
        O._print_shares("sgdm %d tensors" % T, sh)
        assert all(x <= 1.0 for x in sh.values()), sh


# --------------------------------------------------------------------------------------------- (e)
@BX
@pytest.mark.parametrize("hp", [M.BASE, "M1", "L"])
def test_deferred_steps_and_flush_match_the_sweep(hp, bx):
    """Bank A takes twelve sweep steps over marked sparse gradients; bank B defers its two tensors with an L2 term (cap 16),
    takes the same steps and is flushed once at the end, with no catch-up: every marked chunk replays what it missed inside the
    step.  The rate goes through lr_dev, opt_ref.lr_sched: different every step, 0 at steps 3 and 8.  After every step: clock,
    rates, cell, `last`, the marked chunks bit-equal to A, the chunks with last == 0 at their starting bits -- buffer included.
    After the flush: all of p and the buffer bit-equal to A (set L: random signs, bits only; else within the bars of float64
    too), every `last` byte 0, and the window's sum of l2_value plus the backlog against float64's sum."""
    dev = O._dev()
    h = M.HYPER[hp]
    aligned = hp != "L"
    state = M.make_state(aligned=aligned)
    signs = M.signs_of(state) if aligned else None
    lr_fn = lambda s: R.lr_sched(h, s)
    dt = [t for t in ALL if O.E_DEF[t]]
    total, count = 0.0, 0
    with O._opt_bx(bx):
        A, B, B2, start = (M.bank(state, dev, before=O.E_BEFORE) for _ in range(4))
        O._check_mark_pointers(B, O.MARK_MODS)
        latest = [np.zeros(n // 4 + 4, np.uint8) for n in M.SIZES]
        for s in range(1, M.E_STEPS + 1):
            flat, marks, masks, _ = M.grads_e(s, signs)
            A.set_grads(flat, marks)
            M.sgdm_step(A, ALL, M.L2_A, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True)
            B.set_grads(flat, marks)
            v = M.sgdm_step(B, ALL, M.L2_A, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True, deferred=O.E_DEF)
            B2.set_grads(flat, marks)
            v2 = M.sgdm_step(B2, ALL, M.L2_A, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True, deferred=O.E_DEF)
            assert R.bits(v)[0] == R.bits(v2)[0], "step %d: the same call twice, l2_value" % s
            total += float(v[0])
            assert B.read_clock() == [s, O.E_BEFORE] and int(B.cell.item()) == 0
            O._check_rates(B, h, range(1, s + 1), lr_fn)
            assert not bool(B.flat.any()) and not bool(B.marks.any()), "step %d: gradient / marks not re-zeroed" % s
            for t in ALL:
                n = M.SIZES[t]
                if O.E_DEF[t]:
                    latest[t][:n // 4][masks[t]] = s
                    count += 2 * int(masks[t].sum()) + n % 4
                    assert np.array_equal(O._last_of(B, t), latest[t]), "step %d: `last` of tensor %d" % (s, t)
                    sel = O._elem_sel(masks[t], n, dev)
                    assert O._same_bits(B.p[t], A.p[t], sel) and O._same_bits(B.s[t], A.s[t], sel), "step %d: marked chunks, tensor %d" % (s, t)
                    rest = O._elem_sel(latest[t][:n // 4] == 0, n, dev, tail=False)
                    assert O._same_bits(B.p[t], start.p[t], rest) and O._same_bits(B.s[t], start.s[t], rest), \
                        "step %d: a chunk with last == 0 moved, tensor %d" % (s, t)
                else:
                    assert not O._last_of(B, t).any()
            O._assert_banks_equal(A, B, "step %d, the tensors that are not deferred" % s, [t for t in ALL if not O.E_DEF[t]])
        O._assert_banks_equal(B, B2, "the same deferred steps twice, before the flush")
        M.sgdm_flush(B, dt, [M.L2_A[t] for t in dt], h)
        M.sgdm_flush(B2, dt, [M.L2_A[t] for t in dt], h)
        O._assert_banks_equal(B, B2, "the same deferred steps and flush twice")
        assert int(B.backlog.item()) == int(B2.backlog.item())
        count += sum(M.SIZES[t] // 4 for t in dt)
        total += B.take_backlog()
        O._assert_banks_equal(A, B, "after the flush")
        assert all(not bool(x.any()) for x in B.last), "a `last` byte survived the flush"
        assert B.read_clock() == [0, O.E_BEFORE + M.E_STEPS] and int(B.cell.item()) == 0
        assert sum(int((x == M.E_STEPS).sum()) for x in latest) > 0
        _planted_ok(B, M.SIZES, "deferred")
    want, want_l2 = _f64(("e", hp), h, state, M.SIZES, lambda s: (lambda r: (r[0], r[3]))(M.grads_e(s, signs)), M.L2_A, M.E_STEPS, lr_fn)
    sh = M.shares_of(B.snapshot(), want)
    sh["l2sum"] = abs(total - sum(want_l2)) / (R.L2_RTOL * sum(want_l2) + O._fixed_atol(count))
    O._print_shares("sgdm deferred %s bx=%d" % (hp, bx), sh)
    if hp == "L":
        assert sh["l2sum"] <= 1.0, sh
    else:
        assert all(x <= 1.0 for x in sh.values()), sh


# --------------------------------------------------------------------------------------------- (f)
def _case_f(hp, D, with_lin, dev):
    """test_gpu_opt_abi._case_f for xdfm_sgdm_catchup_rows (its batches, extra rows, vocabularies and L2 strengths)."""
    h = M.HYPER[hp]
    lr_fn = lambda s: R.lr_sched(h, s + 1)
    sizes = [V * D for V in O.F_VOCAB] + (list(O.F_VOCAB) if with_lin else [])
    l2 = O.F_L2_EMB + (O.F_L2_LIN if with_lin else [])
    T = len(sizes)
    idx = list(range(T))
    width = [D] * 4 + [1] * (T - 4)
    is_def = [t % 4 != O.F_SKIP for t in idx]
    dt = [t for t in idx if is_def[t]]
    state = M.make_state(sizes, seed=21, aligned=False)
    A, B, start = (M.bank(state, dev) for _ in range(3))
    cols = torch.tensor(O.F_COLS, dtype=torch.int32, device=dev)
    vocab = torch.tensor(O.F_VOCAB, dtype=torch.int32, device=dev)
    emb = R.Rows(B, idx[:4], O.F_L2_EMB, skip=(O.F_SKIP,))
    lin = R.Rows(B, idx[4:], O.F_L2_LIN, skip=(O.F_SKIP,)) if with_lin else None
    QT = (D + 3) // 4 + (1 if D % 4 else 0) + (1 if with_lin else 0)
    cache = {}

    def grads(s):
        if s not in cache:
            _, ids = O._batch_f(s)
            extra = O._extra_f(s)
            masks = [O._row_chunks(np.concatenate([ids[t % 4], extra[t % 4]]), width[t], sizes[t])[:sizes[t] // 4] for t in idx]
            cache[s] = M.sparse_grads(sizes, None, s, seed=13, chunks=masks)
        return cache[s]

    def rows_sel(t, ids):
        w = width[t]
        return torch.from_numpy((np.unique(ids)[:, None] * w + np.arange(w)[None, :]).reshape(-1)).to(dev)

    touched = [np.zeros(n // 4, dtype=bool) for n in sizes]
    total, count = 0.0, 0
    for s in range(1, O.F_STEPS + 1):
        Xn, ids = O._batch_f(s)
        X = torch.from_numpy(Xn).to(dev)
        M.sgdm_catchup(B, X, cols, vocab, O.F_M, D, emb, lin, h)
        count += O.F_B * O.F_M * QT
        flat, marks, masks, _ = grads(s)
        for t in idx:
            n = sizes[t]
            touched[t] |= O._row_chunks(ids[t % 4], width[t], n)[:n // 4]
            sel = rows_sel(t, ids[t % 4])
            assert O._same_bits(B.p[t], A.p[t], sel) and O._same_bits(B.s[t], A.s[t], sel), \
                "step %d: the batch's rows after the catch-up, tensor %d" % (s, t)
            if is_def[t]:
                rest = O._elem_sel(~touched[t], n, dev, tail=False)
                assert O._same_bits(B.p[t], start.p[t], rest) and O._same_bits(B.s[t], start.s[t], rest), \
                    "step %d: a chunk no batch and no gradient reached has moved, tensor %d" % (s, t)
                assert (O._last_of(B, t)[:n // 4][~touched[t]] == 0).all()
            touched[t] |= masks[t]
        A.set_grads(flat, marks)
        M.sgdm_step(A, idx, l2, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True)
        B.set_grads(flat, marks)
        v = M.sgdm_step(B, idx, l2, h, lr_fn(s), lr_dev=True, marked=True, want_l2=True, deferred=is_def)
        total += float(v[0])
        count += sum(2 * int(masks[t].sum()) + sizes[t] % 4 for t in dt)
        assert B.read_clock() == [s, 0] and int(B.cell.item()) == 0
        assert not bool(B.flat.any()) and not bool(B.marks.any())
        for t in idx:
            sel = rows_sel(t, ids[t % 4])
            assert O._same_bits(B.p[t], A.p[t], sel) and O._same_bits(B.s[t], A.s[t], sel), \
                "step %d: the batch's rows after the step, tensor %d" % (s, t)
    O._check_rates(B, h, range(1, O.F_STEPS + 1), lr_fn)
    M.sgdm_flush(B, dt, [l2[t] for t in dt], h)
    count += sum(sizes[t] // 4 for t in dt)
    total += B.take_backlog()
    O._assert_banks_equal(A, B, "after the flush")
    assert all(not bool(x.any()) for x in B.last) and B.read_clock() == [0, O.F_STEPS]
    Xn, _ = O._batch_f(O.F_STEPS + 1)
    M.sgdm_catchup(B, torch.from_numpy(Xn).to(dev), cols, vocab, O.F_M, D, emb, lin, h)
    O._assert_banks_equal(A, B, "after a catch-up at t == 0")
    assert all(not bool(x.any()) for x in B.last) and int(B.backlog.item()) == 0 and B.read_clock() == [0, O.F_STEPS]
    _, want_l2 = _f64(("f", hp, D, with_lin), h, state, sizes, lambda s: (grads(s)[0], grads(s)[3]), l2, O.F_STEPS, lr_fn)
    return abs(total - sum(want_l2)) / (R.L2_RTOL * sum(want_l2) + O._fixed_atol(count))


@pytest.mark.parametrize("D", [16, 10, 4, 3])
@pytest.mark.parametrize("hp", ["M0", "M1"])
def test_catchup_of_the_rows_a_batch_gathers(hp, D):
    """xdfm_sgdm_catchup_rows called directly on the batches of test_gpu_opt_abi.py (m = 4 fields, B = 300, ldx = 7, field 1 not
    deferred, with and without the linear tables; random signs): after the catch-up the batch's rows -- weights and buffers --
    are bit-equal to the sweep's bank as it is after the step before; untouched chunks unchanged; the step on both; then the
    flush and the whole banks, a catch-up at t == 0 that must change nothing, and the window's L2 sum against float64."""
    dev = O._dev()
    for with_lin in (True, False):
        share = _case_f(hp, D, with_lin, dev)
        print("sgdm rows %s D=%d lin=%d: share of the bar, L2 sum against float64 %.3f" % (hp, D, with_lin, share))
        assert share <= 1.0


# --------------------------------------------------------------------------------------------- (g)
def _run_window(hp, dev, cap, steps, flush_every, rate):
    h = M.HYPER[hp]
    state = M.make_state(O.G_SIZES, aligned=False)
    idx = list(range(len(O.G_SIZES)))
    dt = [t for t in idx if O.G_DEF[t]]
    lr_fn = lambda s: R.lr_sched(h, s)
    A, B = M.bank(state, dev, cap=cap), M.bank(state, dev, cap=cap)
    top = 0
    for s in range(1, steps + 1):
        flat, marks, _, _ = M.sparse_grads(O.G_SIZES, None, s, seed=17, chunks=M.masks_e(s, O.G_SIZES, never=True, rate=rate))
        A.set_grads(flat, marks)
        M.sgdm_step(A, idx, O.G_L2, h, lr_fn(s), lr_dev=True, marked=True)
        B.set_grads(flat, marks)
        M.sgdm_step(B, idx, O.G_L2, h, lr_fn(s), lr_dev=True, marked=True, deferred=O.G_DEF)
        if s % flush_every == 0:
            assert B.read_clock()[0] == flush_every < cap
            top = max(top, max(int(O._last_of(B, t).max()) for t in dt))
            M.sgdm_flush(B, dt, [O.G_L2[t] for t in dt], h)
            O._assert_banks_equal(A, B, "after the flush at step %d" % s)
            assert all(not bool(x.any()) for x in B.last) and B.read_clock() == [0, s]
    assert all(np.isfinite(p).all() and np.isfinite(b).all() for p, b in B.snapshot())
    return top


@pytest.mark.parametrize("hp", ["M0", "M1"])
def test_window_of_two_steps_at_cap_3(hp):
    """cap = 3, the smallest the header allows: six steps, a flush after every second one."""
    assert _run_window(hp, O._dev(), 3, 6, 2, 0.03) == 2


@pytest.mark.parametrize("hp", ["M0", "M1"])
def test_window_of_255_steps_at_cap_256(hp):
    """cap = 256, the largest: 255 steps without a flush on the sizes up to 40989, 0.5 % of the chunks marked per step and the
    planted chunks never: the flush replays 255 steps from last == 0.  Afterwards B is bit-equal to the sweep after 255
    steps (the scheduled rate, random signs)."""
    assert _run_window(hp, O._dev(), 256, 255, 255, 0.005) == 255
