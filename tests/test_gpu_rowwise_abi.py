"""GPU tests (-m gpu) of the row-wise Adagrad step at the C ABI (K7w: csrc/rowwise.hip; the arithmetic: csrc/opt_math.h, rw_*)
against numpy float64 (tests/rowwise_ref.py: rw_f64), against the fp32 mirror rw_f32 bit for bit and, where two paths of the
kernel must agree, bit for bit.  The model is test_gpu_ftrl_abi.py; every array the kernel may write lies between guard cells
that the driver checks after every call.

The cases are rowwise_ref.CASES: D = 1 (Adagrad itself), D in {4, 8, 16, 32, 64} on the lanes / rows paths, D = 12, 10, 100 on the
units path, 4099 x 16 with several blocks.  Bars against float64 are rowwise_ref's: C 2^-24 (|p| + |lr g' / den|) per element of
p, one step at a time from the fp32 state the step started with; the L2 value 1e-5 relative."""
import ctypes

import numpy as np
import pytest
import torch

import rowwise_ref as W
import test_gpu_opt_abi as O

pytestmark = pytest.mark.gpu
BX = pytest.mark.parametrize("bx", [0, 1], ids=["bx_default", "bx1"])
ALL = list(range(W.N))
NAN = np.float32("nan")


def _set(bank, gs, marks=None, fill=0.0):
    if marks is None:
        flat = W.flat_of(gs)
        bank.set_grads(flat)
        return flat, None
    flat, fm = W.flat_of(gs, fill=fill, marks=marks)
    bank.set_grads(flat, fm)
    return flat, fm


def _assert_banks_equal(x, y, what):
    for t in ALL:
        for name, xa, ya in (("p", x.p, y.p), ("s", x.s, y.s)):
            if not O._same_bits(xa[t], ya[t]):
                bad = torch.nonzero(O._i32(xa[t]) != O._i32(ya[t])).flatten()
                raise AssertionError("%s: %s of case %r differs in %d elements, first at %d" % (
                    what, name, W.CASES[t], bad.numel(), int(bad[0])))


# --------------------------------------------------------------------------------------------- (a)
@BX
@pytest.mark.parametrize("with_l2", [False, True], ids=["l2m_0", "l2m_1e-3"])
def test_dense_steps_equal_the_mirror_and_lie_within_the_bar(with_l2, bx):
    """Ten steps over all cases with fresh dense gradients (every 7th element zero, zero rows, scales alternating 1e-3 / 1e3,
    the underflow row), the rate through lr_dev on odd steps: after EVERY step p and s equal the mirror's bit for bit and lie
    within the bar of rw_f64 taken from the state the step started with; l2_value against the float64 sum; the dense gradient
    is left alone; nothing is NaN; rows without a gradient keep their bits when there is no L2 term."""
    dev = O._dev()
    l2m = W.L2_A if with_l2 else W.L2_0
    run = W.mirror_run(with_l2)
    worst_p = worst_s = 0.0
    with O._opt_bx(bx):
        bank = W.Bank(W.make_state(), dev)
        for st in range(1, W.STEPS + 1):
            gs = [r[2] for r in run[st - 1]]
            flat, _ = _set(bank, gs)
            lr, through_dev = W.lr_of(st)
            out = W.rw_step(bank, ALL, l2m, lr, lr_dev=through_dev, want_l2=with_l2)
            if st in (1, W.STEPS):
                assert np.array_equal(bank.flat.cpu().numpy(), flat), "a dense gradient was written to"
            got = bank.snapshot()
            value = 0.0
            for t, (p0, s0, g, p1, s1, _) in enumerate(run[st - 1]):
                assert np.isfinite(got[t][0]).all() and np.isfinite(got[t][1]).all(), (st, W.CASES[t])
                dp, ds = int((W.bits(got[t][0]) != W.bits(p1)).sum()), int((W.bits(got[t][1]) != W.bits(s1)).sum())
                assert dp == 0 and ds == 0, "step %d case %r: %d elements of p, %d of s differ from the mirror" % (st, W.CASES[t], dp, ds)
                rp, rs = W.ratios(got[t][0], got[t][1], p0, s0, g, lr, l2m[t], W.EPS)
                worst_p, worst_s = max(worst_p, rp), max(worst_s, rs)
                value += W.rw_f64(p0, s0, g, lr, l2m[t], W.EPS)[2]
                if not with_l2:
                    for r in W.zero_rows(p0.shape[0]):
                        assert np.array_equal(W.bits(got[t][0][r]), W.bits(p0[r])) and W.bits(got[t][1])[r] == W.bits(s0)[r]
            if with_l2:
                assert abs(float(out[0]) - value) <= W.L2_RTOL * value, (st, float(out[0]), value)
    print("row-wise dense l2=%s bx=%d: worst ratio p %.3f s %.3f (C = %g)" % (with_l2, bx, worst_p, worst_s, W.C_BAR))
    assert worst_p <= W.C_BAR and worst_s <= W.C_BAR


# --------------------------------------------------------------------------------------------- (b)
def test_unaligned_pointers_give_the_bits_of_the_aligned_run():
    """Three steps, once with every pointer 16-byte aligned and once with p, g and s each one float past an aligned address (every
    tensor goes by units of four rows, in scalar accesses): bit-identical, the L2 value within its bar."""
    dev = O._dev()

    def run(mis):
        bank = W.Bank(W.make_state(), dev, mis=mis)
        vals = []
        for st in range(1, 4):
            _set(bank, W.dense_grads(st))
            vals.append(W.rw_step(bank, ALL, W.L2_A, W.lr_of(st)[0], want_l2=True))
        return bank, vals

    aligned, vals = run(None)
    for mis in ({"p": 1, "g": 1, "s": 1}, {"p": 1}, {"g": 1}, {"s": 1}):
        other, ovals = run(mis)
        for which, t in (("p", other.p[0]), ("g", other.flat), ("s", other.s[0])):
            assert t.data_ptr() % 16 == 4 * mis.get(which, 0)
        _assert_banks_equal(aligned, other, "%r one float off" % sorted(mis))
        assert all(abs(float(a[0]) - float(b[0])) <= W.L2_RTOL * float(a[0]) for a, b in zip(vals, ovals))      # (other partials)


# --------------------------------------------------------------------------------------------- (c)
@BX
@pytest.mark.parametrize("kind", W.MARK_KINDS)
@pytest.mark.parametrize("with_l2", [False, True], ids=["l2m_0", "l2m_1e-3"])
def test_marks_on_and_off_give_the_same_bits_and_unmarked_chunks_are_not_read(with_l2, kind, bx):
    """Two steps with one pattern of touched rows per step (3 % random rows / all / the first and the last / only the tail rows /
    none / row 1 alone, whose first chunk at D = 10 straddles into row 0).  The marked call sees a NaN in the gradient of every
    unmarked chunk -- with or without an L2 term such a chunk is never read -- the dense call zeros.  Same bits of p and s; after
    the marked step the whole gradient is zero where it was marked, NaN where it was not, and every mark is cleared; without an L2
    term the rows no batch touched keep the bits of p and s."""
    dev = O._dev()
    l2m = W.L2_A if with_l2 else W.L2_0
    with O._opt_bx(bx):
        dense, marked = W.Bank(W.make_state(), dev), W.Bank(W.make_state(), dev)
        for st in (1, 2):
            gs, ms, ks = W.sparse_grads(kind, st)
            before = dense.snapshot()
            _set(dense, gs)
            vd = W.rw_step(dense, ALL, l2m, W.LR, want_l2=with_l2)
            _, fm = _set(marked, gs, marks=ms, fill=NAN)
            vm = W.rw_step(marked, ALL, l2m, W.LR, marked=True, want_l2=with_l2)
            _assert_banks_equal(dense, marked, "marks %s step %d" % (kind, st))
            after = marked.snapshot()
            assert all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in after)
            if with_l2:
                assert abs(float(vd[0]) - float(vm[0])) <= W.L2_RTOL * float(vd[0])
            flat = marked.flat.cpu().numpy()
            sel = np.repeat(fm.astype(bool), 4)
            assert (flat[sel] == 0).all(), "a marked chunk was not re-zeroed"
            assert np.isnan(flat[~sel]).all(), "an unmarked chunk was written to"
            assert int(marked.marks.max()) == 0, "a mark was left"
            if not with_l2:
                for t, k in enumerate(ks):
                    still = ~k
                    assert np.array_equal(W.bits(after[t][0][still]), W.bits(before[t][0][still])), (kind, W.CASES[t])
                    assert np.array_equal(W.bits(after[t][1][still]), W.bits(before[t][1][still])), (kind, W.CASES[t])
                    assert k.sum() == 0 or (after[t][1][k] > before[t][1][k]).any()


# --------------------------------------------------------------------------------------------- (d)
def test_the_grid_does_not_change_the_bits():
    """opt_bx 1 (one block per tensor), 3 and the default: three dense steps with an L2 term, the same bits."""
    dev = O._dev()
    banks = []
    for bx in (0, 1, 3):
        with O._opt_bx(bx):
            bank = W.Bank(W.make_state(), dev)
            for st in range(1, 4):
                _set(bank, W.dense_grads(st))
                W.rw_step(bank, ALL, W.L2_A, W.LR)
            banks.append(bank)
    _assert_banks_equal(banks[0], banks[1], "opt_bx 1")
    _assert_banks_equal(banks[0], banks[2], "opt_bx 3")


# --------------------------------------------------------------------------------------------- (e)
def test_seventy_tensors_go_out_in_two_launches():
    """70 small tensors of the first nine shapes in one call (64 descriptors per launch: two launches): the result equals 70
    single-tensor calls and the mirror bit for bit, and the L2 value -- whose second launch's slots start behind the first's --
    equals the float64 sum."""
    dev = O._dev()
    shapes = [W.CASES[k % 9] for k in range(70)]
    rng = np.random.RandomState(7)
    state = [((rng.randn(r, d) * 0.05).astype(W.F32), (rng.rand(r) * 1e-4).astype(W.F32)) for r, d in shapes]
    gs = [rng.randn(r, d).astype(W.F32) for r, d in shapes]
    l2m = [1e-3 * (1 + k % 3) for k in range(70)]

    import opt_ref as R
    offs, total = R.grad_offsets([p.size for p, _ in state])
    flat = np.zeros(total, W.F32)
    for t, g in enumerate(gs):
        flat[offs[t]:offs[t] + g.size] = g.ravel()
    together, single = W.Bank(state, dev), W.Bank(state, dev)
    together.set_grads(flat)
    single.set_grads(flat)
    idx = list(range(70))
    v = W.rw_step(together, idx, l2m, W.LR, want_l2=True)
    for t in idx:
        W.rw_step(single, [t], [l2m[t]], W.LR)
    for t in idx:
        assert O._same_bits(together.p[t], single.p[t]) and O._same_bits(together.s[t], single.s[t]), shapes[t]
    want = sum(W.rw_f64(p, s, g, W.LR, l, W.EPS)[2] for (p, s), g, l in zip(state, gs, l2m))
    assert abs(float(v[0]) - want) <= W.L2_RTOL * want, (float(v[0]), want)
    for t in idx:                                           # ... and each equals the mirror
        p1, s1, _ = W.rw_f32(state[t][0], state[t][1], gs[t], W.LR, l2m[t], W.EPS)
        got = together.get(t)
        assert np.array_equal(W.bits(got[0]), W.bits(p1)) and np.array_equal(W.bits(got[1]), W.bits(s1)), shapes[t]


# --------------------------------------------------------------------------------------------- (f)
def test_refusals_on_device_pointers_write_nothing():
    dev = O._dev()
    bank = W.Bank(W.make_state(), dev)
    gs, ms, _ = W.sparse_grads("all", 1)
    flat, fm = _set(bank, gs, marks=ms)
    before = bank.snapshot()
    idx = [2, 4, 5]

    def bad(**kw):
        arr = bank.descriptors(idx, [0.0] * 3, True)
        for k, v in kw.items():
            setattr(arr[1], k, v)
        return arr
    calls = [dict(lr=-0.05), dict(eps=0.0), dict(eps=-1.0), dict(arr=bad(dim=0)), dict(arr=bad(dim=2000)), dict(arr=bad(rows=-1)),
             dict(arr=bad(l2=-1.0)), dict(arr=bad(state=None)), dict(arr=bad(state=bank.s[4].data_ptr() + 2)),
             dict(arr=bad(param=bank.p[4].data_ptr() + 4)), dict(arr=bad(grad=bank.flat.data_ptr() + 4 * bank.goff[4] + 4))]
    for kw in calls:
        args = dict(lr=W.LR, marked=True, check=False)
        args.update(kw)
        lr = args.pop("lr")
        assert W.rw_step(bank, idx, [0.0] * 3, lr, **args) == O.R.ERR_INVALID, kw
    from xdfm_amd import _lib
    lib = _lib.load()
    arr = bank.descriptors(idx, [0.0] * 3, True)
    rc = lib.xdfm_rowwise_adagrad_step(ctypes.cast(arr, ctypes.c_void_p), 3, W.LR, None, W.EPS, None,
                                       ctypes.c_void_p(bank.l2_value.data_ptr()), O.R._stream())
    assert rc == O.R.ERR_INVALID and b"l2_value needs l2_ws" in lib.xdfm_last_error()
    torch.cuda.synchronize()
    bank.check_guards("refusals")
    after = bank.snapshot()
    for t in ALL:
        assert all(np.array_equal(W.bits(a), W.bits(b)) for a, b in zip(before[t], after[t]))
    assert np.array_equal(bank.flat.cpu().numpy(), flat) and np.array_equal(bank.marks.cpu().numpy(), fm)


# --------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("marks", [False, True], ids=["dense", "marked"])
@pytest.mark.parametrize("with_l2", [False, True], ids=["l2m_0", "l2m_1e-3"])
def test_dim_one_gives_the_bits_of_the_adagrad_step(with_l2, marks):
    """The same [4099] tensors as 4099 x 1 through xdfm_rowwise_adagrad_step and through xdfm_adagrad_step, three steps, dense
    and by marks: p and the accumulator bit for bit, the gradient and the marks left the same, the L2 value within its bar."""
    import opt_ref as R
    dev = O._dev()
    sizes = [4099, 5, 67]
    rng = np.random.RandomState(11)
    state = [((rng.randn(n) * 0.05).astype(W.F32), (rng.rand(n) * 1e-4).astype(W.F32)) for n in sizes]
    l2 = [1e-3 if with_l2 else 0.0] * 3
    a = R.Bank("adagrad", state, dev)
    b = R.Bank("adagrad", state, dev)
    h = dict(eps=W.EPS, alpha=0.0)
    lib_idx = [0, 1, 2]
    for st in range(1, 4):
        if marks:
            flat, fm, _, _ = R.sparse_grads(sizes, ["random3", "all", "ends"], st)
        else:
            flat, _ = R.dense_grads(sizes, st)
            fm = None
        a.set_grads(flat, fm)
        b.set_grads(flat, fm)
        va = R.opt_step(a, lib_idx, l2, h, W.LR, marked=marks, want_l2=with_l2)
        from xdfm_amd import _lib
        arr = (_lib.RowwiseTensor * 3)()
        for k in lib_idx:
            arr[k].param, arr[k].grad, arr[k].state = b.p[k].data_ptr(), b.flat.data_ptr() + 4 * b.goff[k], b.s[k].data_ptr()
            arr[k].rows, arr[k].dim, arr[k].l2 = sizes[k], 1, l2[k]
            arr[k].grad_marks = b.mark_ptr(k) if marks else None
        vb = W.rw_step(b, lib_idx, l2, W.LR, want_l2=with_l2, arr=arr)
        for k in lib_idx:
            assert O._same_bits(a.p[k], b.p[k]) and O._same_bits(a.s[k], b.s[k]), (st, sizes[k])
        assert torch.equal(a.flat, b.flat) and torch.equal(a.marks, b.marks)
        if with_l2:
            assert abs(float(va[0]) - float(vb[0])) <= W.L2_RTOL * float(va[0])
