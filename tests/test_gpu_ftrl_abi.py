"""GPU tests (-m gpu) of the FTRL-Proximal step at the C ABI (K7f: csrc/ftrl.hip; the element update: csrc/opt_math.h, ftrl_one)
against numpy float64 (tests/ftrl_ref.py: ftrl_f64) and, where two paths of the kernel must agree, bit for bit.  The model is
test_gpu_opt_abi.py, whose mark patterns and helpers this file reuses; sizes and planted chunks are adam_ref's; every array the
kernel may write lies between guard cells that the driver checks after every call.

Bars against float64: ftrl_ref.TOL (p: the project's rtol 2e-6 / atol 1e-8; z 2e-6 / 1e-7 and n 2e-6 / 1e-10, set from the fp32
mirror, which test_ftrl_reference.py holds to half of them), L2 value 1e-5 relative; elements where kernel and float64 disagree
on |z'| <= l1 are left out, at most max(1, numel // 10000) per tensor and step.  The float64 comparisons run on inputs with one
sign per element, the bit-for-bit ones on random signs (ftrl_ref.py, "THE SIGNS")."""
import ctypes

import numpy as np
import pytest
import torch

import ftrl_ref as F
import test_gpu_opt_abi as O

pytestmark = pytest.mark.gpu
BX = pytest.mark.parametrize("bx", [0, 1], ids=["bx_default", "bx1"])
N = len(F.SIZES)
ALL = list(range(N))
NAN_BITS = 0x7FC00000


def _assert_banks_equal(x, y, what, tensors=None):
    for t in (range(len(x.sizes)) if tensors is None else tensors):
        for name, xa, ya in (("p", x.p, y.p), ("z", x.z, y.z), ("n", x.n, y.n)):
            if not O._same_bits(xa[t], ya[t]):
                bad = torch.nonzero(O._i32(xa[t]) != O._i32(ya[t])).flatten()
                raise AssertionError("%s: %s of tensor %d (%d elements) differs in %d elements, first at %d" % (
                    what, name, t, x.sizes[t], bad.numel(), int(bad[0])))


def _planted_ok(snap, state, what):
    """Nothing became NaN or infinite, and the planted chunk with p = 0 and g = 0 (g' == 0 with or without an L2 term) kept the
    bits of all three arrays -- at n == 0 (set Z) without a 0 / 0."""
    for t, (got, start) in enumerate(zip(snap, state)):
        assert all(np.isfinite(a).all() for a in got), "%s: tensor %d" % (what, t)
        for c in F.planted_chunks(got[0].size):
            for a, b in zip(got, start):
                assert np.array_equal(F.bits(a[4 * c:4 * c + 4]), F.bits(b[4 * c:4 * c + 4])), \
                    "%s: the chunk without a gradient moved, tensor %d" % (what, t)


# --------------------------------------------------------------------------------------------- (a)
@BX
@pytest.mark.parametrize("hp", F.SETS)
def test_dense_sweep_vs_float64(hp, bx):
    """Ten steps of xdfm_ftrl_step over all seven sizes with fresh dense gradients (every 7th element zero, scale alternating
    0.1 / 1e-3), the set's model L2 (F2: 1e-3 / 0 / 5e-2 on the first three tensors), l2_value on odd steps: p, z and n after
    EVERY step against ftrl_f64 carried in float64 from the same fp32 start, l2_value against the float64 sum.  FD sends the
    rate through lr_dev, another one every step.  The dense gradient is left alone.  At the default grid the final state is also
    compared with the fp32 mirror ftrl_f32: the number of differing elements is printed, and asserted to be 0 as it was measured."""
    dev = O._dev()
    h = F.HYPER[hp]
    state, signs, want, want_l2 = F.dense_case(hp)
    worst, left = dict.fromkeys("pzn", 0.0), 0
    with O._opt_bx(bx):
        bank = F.Bank(state, dev)
        for s in range(1, F.STEPS + 1):
            flat, _ = F.dense_grads(F.SIZES, s, signs=signs)
            lr, through_dev = F.lr_of(hp, s)
            bank.set_grads(flat)
            out = F.ftrl_step(bank, ALL, h["l2m"], h, lr, lr_dev=through_dev, want_l2=bool(s % 2) and any(h["l2m"]))
            if out is not None:
                assert abs(float(out[0]) - want_l2[s - 1]) <= F.L2_RTOL * want_l2[s - 1], (s, float(out[0]), want_l2[s - 1])
            if s in (1, F.STEPS):
                assert np.array_equal(bank.flat.cpu().numpy(), flat), "a dense gradient was written to"
            got = bank.snapshot()
            shares, out_n, excess = F.compare(got, want[s - 1], h["l1"])
            assert excess <= 0, "step %d: a tensor leaves %d elements more than its cap out" % (s, excess)
            worst = {q: max(worst[q], shares[q]) for q in "pzn"}
            left += out_n
        _planted_ok(got, state, "dense sweep")
    O._print_shares("ftrl dense %s bx=%d (%d elements left out)" % (hp, bx, left), worst)
    assert all(x <= 1.0 for x in worst.values()), worst
    if bx == 0:
        mirror, _ = F.run_ref(F.ftrl_f32, hp, state, F.SIZES, lambda st: F.dense_grads(F.SIZES, st, signs=signs), F.F32)
        diff = {q: sum(int((F.bits(got[t][k]) != F.bits(mirror[-1][t][k])).sum()) for t in ALL) for k, q in enumerate("pzn")}
        print("ftrl dense %s: elements whose bits differ from ftrl_f32 after %d steps: %r of %d" % (hp, F.STEPS, diff, sum(F.SIZES)))
        assert not any(diff.values()), diff                 # (0 of 1 173 370 on an MI355X for every set: asserted)


# --------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("hp", ["F2", "Z"])
def test_unaligned_tensors_take_the_scalar_path(hp):
    """Three steps, once with every pointer 16-byte aligned and once with each of p, g, z and n one float past an aligned
    address (the whole tensor goes through the scalar loop): bit-identical to the aligned run; the L2 value, summed over other
    partials, within its bar.  Random signs.
    grad_marks with such a pointer is refused before any device work: state, gradient, marks and guards untouched."""
    dev = O._dev()
    h = F.HYPER[hp]
    state = F.make_state(h, aligned=False)

    def run(mis):
        bank = F.Bank(state, dev, mis=mis)
        vals = []
        for s in range(1, 4):
            flat, _ = F.dense_grads(F.SIZES, s)
            bank.set_grads(flat)
            vals.append(F.ftrl_step(bank, ALL, F.L2_A, h, h["lr"], want_l2=True))
        return bank, vals

    aligned, vals = run(None)
    _planted_ok(aligned.snapshot(), state, "aligned")
    for which in "pgsn":
        other, ovals = run({which: 1})
        ptr = {"p": other.p[0], "g": other.flat, "s": other.z[0], "n": other.n[0]}[which].data_ptr()
        assert ptr % 16 == 4
        _assert_banks_equal(aligned, other, "%s one float off" % which)
        assert all(abs(float(a[0]) - float(b[0])) <= F.L2_RTOL * float(a[0]) for a, b in zip(vals, ovals))      # (other partials)
        flat, marks, _, _ = F.sparse_grads(F.SIZES, ["all"] * N, 4)
        other.set_grads(flat, marks)
        before = other.snapshot()
        rc = F.ftrl_step(other, ALL, F.L2_A, h, h["lr"], marked=True, want_l2=True, check=False)
        assert rc == F.R.ERR_INVALID
        after = other.snapshot()
        for t in ALL:
            assert all(np.array_equal(F.bits(a), F.bits(b)) for a, b in zip(before[t], after[t]))
        assert np.array_equal(other.flat.cpu().numpy(), flat) and np.array_equal(other.marks.cpu().numpy(), marks)


# --------------------------------------------------------------------------------------------- (c)
@BX
@pytest.mark.parametrize("case", sorted(O.CASES_C))
@pytest.mark.parametrize("hp", ["F1", "Z"])
def test_marks_on_and_off_give_the_same_bits_and_unmarked_chunks_are_not_read(hp, case, bx):
    """Two steps with the same mark pattern per tensor (3 % random chunks / all / first and last / only the tail / none) and
    fresh values, random signs.  The marked call sees a NaN in the gradient of every unmarked chunk (unmarked chunks are not
    read), the dense call zeros there: p, z, n and the L2 value have the same bits, with the model's L2 on the tensors (every
    chunk is an update) and without (the skip); afterwards the marked gradient chunks, the tails and all mark bytes are zero and
    every NaN is still there.  l2m == 0: the unmarked chunks of p, z and n keep their bits."""
    dev = O._dev()
    h = F.HYPER[hp]
    state = F.make_state(h, aligned=False)
    kinds_c, l2m = O.CASES_C[case]
    masks = None
    with O._opt_bx(bx):
        dense, marked = F.Bank(state, dev), F.Bank(state, dev)
        O._check_mark_pointers(marked, O.MARK_MODS)
        for s in (1, 2):
            flat, marks, masks, offs = F.sparse_grads(F.SIZES, kinds_c, s, chunks=masks)
            dense.set_grads(flat)
            vd = F.ftrl_step(dense, ALL, l2m, h, h["lr"], want_l2=True)
            assert np.array_equal(dense.flat.cpu().numpy(), flat), "the dense run wrote to its gradient"
            poisoned = F.bits(flat).copy()
            after = np.zeros_like(poisoned)
            for t in ALL:
                un = np.nonzero(np.repeat(~masks[t], 4))[0] + offs[t]
                poisoned[un] = NAN_BITS
                after[un] = NAN_BITS
            marked.set_grads(poisoned.view(np.float32), marks)
            vm = F.ftrl_step(marked, ALL, l2m, h, h["lr"], marked=True, want_l2=True)
            assert np.array_equal(F.bits(marked.flat.cpu().numpy()), after), "step %d: gradient not re-zeroed, or a NaN gone" % s
            assert not bool(marked.marks.any()), "step %d: marks not cleared" % s
            assert F.bits(vd)[0] == F.bits(vm)[0], (float(vd[0]), float(vm[0]))
            _assert_banks_equal(dense, marked, "marked against dense, step %d" % s)
    assert sum(int(k.sum()) for k in masks) > 8000 and not masks[3].size and not masks[4].any() and masks[1].all()
    assert (float(vd[0]) > 0) == (case == "l2_A")
    snap = marked.snapshot()
    _planted_ok(snap, state, "marked")
    moved = 0
    for t in ALL:
        sel = np.repeat(masks[t], 4)
        rest = np.nonzero(~sel)[0]
        if l2m[t] == 0:
            for a, b in zip(snap[t], state[t]):
                assert np.array_equal(F.bits(a[rest]), F.bits(b[rest])), "an unmarked chunk moved, tensor %d" % t
        else:
            live = rest[state[t][0][rest] != 0]                 # g' = 2 l2m p: a real update wherever p is not 0
            assert live.size > 100 and (snap[t][2][live] >= state[t][2][live]).all() and (snap[t][1][live] != state[t][1][live]).any()
        moved += int((snap[t][0][: sel.size][sel] != state[t][0][: sel.size][sel]).sum())
    assert moved > 8000
    if hp == "Z":                                               # l1 = 1e-2: the step leaves exact zeros behind
        assert sum(int((snap[t][0][: 4 * masks[t].size][np.repeat(masks[t], 4)] == 0.0).sum()) for t in ALL) > 100


# --------------------------------------------------------------------------------------------- (d)
def test_the_grid_does_not_change_the_bits():
    """Option "opt_bx" = 1 (a tensor is one block) against the built-in cap: three dense and two marked steps give the same
    bits of p, z and n (the L2 value is summed over other partials and only agrees within its bar)."""
    dev = O._dev()
    h = F.HYPER["Z"]
    state = F.make_state(h, aligned=False)
    kinds_c, _ = O.CASES_C["l2_A"]
    banks, vals = [], []
    for bx in (0, 1):
        with O._opt_bx(bx):
            bank = F.Bank(state, dev)
            for s in range(1, 4):
                flat, _ = F.dense_grads(F.SIZES, s)
                bank.set_grads(flat)
                v = F.ftrl_step(bank, ALL, F.L2_A, h, h["lr"], want_l2=True)
            for s in (4, 5):
                flat, marks, _, _ = F.sparse_grads(F.SIZES, kinds_c, s)
                bank.set_grads(flat, marks)
                F.ftrl_step(bank, ALL, F.L2_A if s == 4 else F.L2_0, h, h["lr"], marked=True)
        banks.append(bank)
        vals.append(float(v[0]))
    _assert_banks_equal(banks[0], banks[1], "opt_bx 1 against the built-in cap")
    assert abs(vals[0] - vals[1]) <= F.L2_RTOL * vals[0] and vals[0] > 0


# --------------------------------------------------------------------------------------------- (e)
def test_more_tensors_than_a_launch_holds():
    """70 tensors (sizes cycling through 3, 67, 4099; a third with a model L2 term) in one call: two launches, the second one's
    L2 partials behind the first one's, one finish over both.  p, z and n bit-equal to one call per tensor, l2_value against
    float64."""
    dev = O._dev()
    h = F.HYPER["F1"]
    T = 70
    sizes, l2m = O.SIZES_D[:T], O._l2_d(T, "third")
    idx = list(range(T))
    state = F.make_state(h, sizes, seed=11, aligned=False)
    one, single = F.Bank(state, dev), F.Bank(state, dev)
    cur = [tuple(a.astype(np.float64) for a in s) for s in state]
    for s in (1, 2):
        flat, marks, _, offs = F.sparse_grads(sizes, ["random3"] * T, s, seed=12)
        want = sum(float(F.F32(l2m[t])) * float(np.sum(cur[t][0] ** 2)) for t in idx)
        one.set_grads(flat, marks)
        v = F.ftrl_step(one, idx, l2m, h, h["lr"], marked=True, want_l2=True)
        assert abs(float(v[0]) - want) <= F.L2_RTOL * want, (float(v[0]), want)
        assert not bool(one.flat.any()) and not bool(one.marks.any())
        single.set_grads(flat, marks)
        for t in idx:
            F.ftrl_step(single, [t], [l2m[t]], h, h["lr"], marked=True)
        cur = [tuple(a.astype(np.float64) for a in x) for x in one.snapshot()]
    _assert_banks_equal(one, single, "%d tensors in one call against one call per tensor" % T)


# --------------------------------------------------------------------------------------------- (f)
def test_refusals_leave_the_device_alone():
    """lr <= 0, negative l1 / l2 / beta and a tensor without n, on real device pointers: XDFM_ERR_INVALID, nothing written."""
    dev = O._dev()
    h = F.HYPER["F1"]
    state = F.make_state(h, F.SIZES[1:4])
    bank = F.Bank(state, dev)
    idx = [0, 1, 2]
    flat, marks, _, _ = F.sparse_grads(bank.sizes, ["all"] * 3, 1)
    bank.set_grads(flat, marks)
    before = bank.snapshot()
    assert F.ftrl_step(bank, idx, [0.0] * 3, h, 0.0, marked=True, check=False) == F.R.ERR_INVALID
    assert F.ftrl_step(bank, idx, [0.0] * 3, h, -0.05, marked=True, check=False) == F.R.ERR_INVALID
    for key in ("l1", "l2", "beta"):
        assert F.ftrl_step(bank, idx, [0.0] * 3, h, 0.05, marked=True, check=False, **{key: -1e-3}) == F.R.ERR_INVALID
    arr = bank.descriptors(idx, [0.0] * 3, True)
    arr[1].n = None
    assert F.ftrl_step(bank, idx, [0.0] * 3, h, 0.05, check=False, arr=arr) == F.R.ERR_INVALID
    after = bank.snapshot()
    for t in idx:
        assert all(np.array_equal(F.bits(a), F.bits(b)) for a, b in zip(before[t], after[t]))
    assert np.array_equal(bank.flat.cpu().numpy(), flat) and np.array_equal(bank.marks.cpu().numpy(), marks)
    assert ctypes.sizeof(arr[0]) == 56
