"""GPU tests (-m gpu) of the Adam kernels at the C ABI (K7 / K7d: csrc/adam.hip, csrc/adam_math.h) against numpy float64
(tests/adam_ref.py: adam_f64) and, where two paths of the kernels must agree, bit for bit against the path that float64
is tied to.  Sizes, hyper-parameter sets and planted rows are those of adam_ref.py; DESIGN.md ("The Adam kernel tests")
lists which case reaches which path of adam_step_kernel and the measured shares of the bars.

Bars against float64 (those of test_table_adam_kernel_matches_torch_adam and test_gpu_optim.py): p rtol 2e-6 / atol 1e-8,
m 2e-6 / 2e-8, v 2e-6 / 1e-10, L2 value 1e-5 relative.  Stock fp32 torch.optim.Adam on the CPU, on the inputs of (a)
(adam_ref.make_state / dense_grads, six steps), uses at most 0.42 of them at H0-H4."""
import contextlib

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu
BX = pytest.mark.parametrize("bx", [0, 1], ids=["bx_default", "bx1"])
N = len(R.SIZES)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def _adam_bx(value):
    """Option "adam_bx" = most blocks one tensor gets (0: the default, 512).  At 1 a tensor is one block: the 40989 and
    1 120 016 element tensors run many iterations of every unrolled loop and of the deferred scan's paired-group loop."""
    from xdfm_amd import _lib
    before = _lib.get_option("adam_bx")
    _lib.set_option("adam_bx", value)
    try:
        yield
    finally:
        _lib.set_option("adam_bx", before)


def _i32(t):
    return t.view(torch.int32)


def _same_bits(a, b, sel=None):
    a, b = _i32(a), _i32(b)
    if sel is not None:
        a, b = a[sel], b[sel]
    return torch.equal(a, b)


def _assert_banks_equal(x, y, what, tensors=None):
    for t in (range(len(x.sizes)) if tensors is None else tensors):
        for name, xa, ya in (("p", x.p, y.p), ("m", x.m, y.m), ("v", x.v, y.v)):
            if not _same_bits(xa[t], ya[t]):
                bad = torch.nonzero(_i32(xa[t]) != _i32(ya[t])).flatten()
                raise AssertionError("%s: %s of tensor %d (%d elements) differs in %d elements, first at %d" % (
                    what, name, t, x.sizes[t], bad.numel(), int(bad[0])))


def _check_mark_pointers(bank):
    mods = {bank.mark_ptr(t) % 16 for t in range(len(bank.sizes))}
    assert len(mods) >= 3 and 0 in mods, mods


def _elem_sel(mask, n, dev):
    """Element indices of the marked chunks plus the numel % 4 tail."""
    sel = np.repeat(mask, 4)
    sel = np.concatenate([sel, np.ones(n - sel.size, dtype=bool)])
    return torch.from_numpy(np.nonzero(sel)[0]).to(dev)


# --------------------------------------------------------------------------------------------- float64 trajectories
_F64 = {}


def _f64_run(key, state, sizes, grads_of, l2, hp, steps, steps0=None):
    """Carry `state` through `steps` steps in float64 -> (final [(p, m, v)], [L2 value per step])."""
    if key in _F64:
        return _F64[key]
    _, b1, b2, eps = R.HYPER[hp]
    cur = [tuple(a.astype(np.float64) for a in s) for s in state]
    values = []
    for s in range(1, steps + 1):
        flat, offs = grads_of(s)
        lr, _ = R.lr_of(hp, s)
        tot = 0.0
        for t, n in enumerate(sizes):
            own = s + (0 if steps0 is None else steps0[t])
            p, m, v, val = R.adam_f64(cur[t][0], flat[offs[t]:offs[t] + n], cur[t][1], cur[t][2], own, lr, b1, b2, eps, l2[t])
            cur[t] = (p, m, v)
            tot += val
        values.append(tot)
    _F64[key] = (cur, values)
    return _F64[key]


# --------------------------------------------------------------------------------------------- (a)
@BX
@pytest.mark.parametrize("hp", ["H0", "H1", "H2", "H3", "H4"])
def test_dense_sweep_vs_float64(hp, bx):
    """Six steps of xdfm_adam_step_lr over all seven sizes with fresh dense gradients (every 7th element zero, scale
    alternating 0.1 / 1e-3), L2 1e-3 / 0 / 5e-2 on the first three tensors, l2_value on odd steps: p, m, v against adam_f64
    carried in float64 from the same fp32 start, l2_value against the float64 sum."""
    dev = _dev()
    state = R.make_state()
    want, want_l2 = _f64_run(("a", hp), state, R.SIZES, lambda s: R.dense_grads(R.SIZES, s), R.L2_A, hp, 6)
    with _adam_bx(bx):
        bank = R.Bank(state, dev)
        got_l2 = {}
        for s in range(1, 7):
            flat, _ = R.dense_grads(R.SIZES, s)
            bank.set_grads(flat)
            out = R.adam_step(bank, list(range(N)), R.L2_A, hp, s, want_l2=bool(s % 2))
            torch.cuda.synchronize()
            if s % 2:
                got_l2[s] = float(out.item())
            assert np.array_equal(bank.flat.cpu().numpy(), flat), "a dense gradient was written to"
        got = bank.snapshot()
    assert [float(x) for x in bank.steps.cpu()] == [6.0] * N
    shares = {}
    for k, name in enumerate("pmv"):
        rtol, atol = R.TOL[name]
        shares[name] = max(R.share(got[t][k], want[t][k], rtol, atol) for t in range(N))
    shares["l2"] = max(abs(got_l2[s] - want_l2[s - 1]) / (R.L2_RTOL * want_l2[s - 1]) for s in got_l2)
    print("adam dense %s bx=%d: share of the bar p %.3f m %.3f v %.3f l2 %.3f" % (hp, bx, shares["p"], shares["m"], shares["v"],
                                                                                 shares["l2"]))
    assert all(x <= 1.0 for x in shares.values()), shares


# --------------------------------------------------------------------------------------------- (b)
def test_unaligned_tensors_take_the_scalar_path_with_the_same_bits():
    """The values of (a) at H0, once with every pointer 16-byte aligned and once with each of p, g, m, v one float past
    an aligned address (`vec == false`: the whole tensor goes through the tail loop): p, m, v bit-identical to the aligned
    run, which (a) ties to float64."""
    dev = _dev()
    state = R.make_state()

    def run(mis):
        bank = R.Bank(state, dev, mis=mis)
        for s in range(1, 7):
            flat, _ = R.dense_grads(R.SIZES, s)
            bank.set_grads(flat)
            R.adam_step(bank, list(range(N)), R.L2_A, "H0", s, want_l2=bool(s % 2))
        torch.cuda.synchronize()
        return bank

    aligned = run(None)
    for which in "pgmv":
        other = run({which: 1})
        ptr = {"p": other.p[0], "g": other.flat, "m": other.m[0], "v": other.v[0]}[which].data_ptr()
        assert ptr % 16 == 4
        _assert_banks_equal(aligned, other, "%s one float off" % which)


# --------------------------------------------------------------------------------------------- (c)
KINDS_C = ["random3", "all", "ends", "tail", "none", "tail", "random3"]


@BX
@pytest.mark.parametrize("hp", ["H0", "H1"])
def test_marked_lazy_and_dense_gradients(hp, bx):
    """Two steps with the same mark pattern per tensor (3 % random chunks / all / first and last / only the tail / none)
    and fresh values.  Marked against dense: p, m, v and the L2 value have the same bits, the gradient buffer and the
    marks are all zero afterwards, the dense run leaves g alone.  XDFM_ADAM_LAZY: marked chunks have the dense run's bits,
    unmarked chunks keep the bits from before the first step, tail elements are updated."""
    dev = _dev()
    state = R.make_state()
    masks = None
    with _adam_bx(bx):
        dense, marked, lazy, start = (R.Bank(state, dev) for _ in range(4))
        _check_mark_pointers(marked)
        for s in (1, 2):
            flat, marks, masks, _ = R.sparse_grads(R.SIZES, KINDS_C, s, chunks=masks)
            dense.set_grads(flat)
            vd = R.adam_step(dense, list(range(N)), R.L2_A, hp, s, want_l2=True)
            torch.cuda.synchronize()
            assert np.array_equal(dense.flat.cpu().numpy(), flat), "the dense run wrote to its gradient"
            for bank, flags in ((marked, [0] * N), (lazy, [R.LAZY] * N)):
                bank.set_grads(flat, marks)
                vm = R.adam_step(bank, list(range(N)), R.L2_A, hp, s, marked=True, flags=flags, want_l2=True)
                torch.cuda.synchronize()
                assert not bool(bank.gbuf.any()), "gradient not re-zeroed (step %d, flags %d)" % (s, flags[0])
                assert not bool(bank.marks.any()), "marks not cleared (step %d, flags %d)" % (s, flags[0])
                if not flags[0]:
                    assert _same_bits(vd, vm), (float(vd), float(vm))
        _assert_banks_equal(dense, marked, "marked against dense")
    assert sum(int(k.sum()) for k in masks) > 8000 and not masks[3].size and not masks[4].any() and masks[1].all()
    for t, n in enumerate(R.SIZES):
        sel = _elem_sel(masks[t], n, dev)
        rest = _elem_sel(~masks[t], n, dev)[:4 * int((~masks[t]).sum())]          # whole unmarked chunks only
        for name, la, da, sa in (("p", lazy.p, dense.p, start.p), ("m", lazy.m, dense.m, start.m), ("v", lazy.v, dense.v, start.v)):
            assert _same_bits(la[t], da[t], sel), "lazy: marked chunks / tail of %s, tensor %d" % (name, t)
            assert _same_bits(la[t], sa[t], rest), "lazy: an unmarked chunk of %s moved, tensor %d" % (name, t)
        if n % 4:
            assert not _same_bits(lazy.p[t], start.p[t], torch.arange(n // 4 * 4, n, device=dev)), "lazy: tail not updated"


# --------------------------------------------------------------------------------------------- (d)
def test_more_than_64_tensors_take_two_launches():
    """T = 70 (the seven sizes ten times, different L2 strengths): two launches, tensors sorted by size and dealt
    round-robin, the L2 partials of both summed by the finish.  p, m, v bit-equal to 70 single-tensor calls; l2_value
    against float64 and bit-identical on a second run."""
    dev = _dev()
    state = R.make_state_70()
    want, want_l2 = _f64_run(("d",), state, R.SIZES_70, lambda s: R.dense_grads(R.SIZES_70, s, seed=12), R.L2_70, "H0", 2)
    snap1, l2_1 = R.run_70(dev, True, state=state)
    snap2, l2_2 = R.run_70(dev, True, state=state)
    snap0, _ = R.run_70(dev, False, state=state)
    for t in range(70):
        for k, name in enumerate("pmv"):
            assert np.array_equal(R.bits(snap1[t][k]), R.bits(snap0[t][k])), "%s of tensor %d: one call != single calls" % (name, t)
            assert np.array_equal(R.bits(snap1[t][k]), R.bits(snap2[t][k])), "%s of tensor %d: second run" % (name, t)
    share = 0.0
    for s in range(2):
        assert R.bits(l2_1[s]) == R.bits(l2_2[s]), "l2_value of step %d is not reproducible" % (s + 1)
        share = max(share, abs(float(l2_1[s][0]) - want_l2[s]) / (R.L2_RTOL * want_l2[s]))
    print("adam 70 tensors: share of the bar l2 %.3f (value %.9g)" % (share, float(l2_1[1][0])))
    assert share <= 1.0
    shares = [max(R.share(snap1[t][k], want[t][k], *R.TOL[name]) for t in range(70)) for k, name in enumerate("pmv")]
    print("adam 70 tensors: share of the bar p %.3f m %.3f v %.3f (printed only: the bit-equality above ties them to (a))" % tuple(shares))


# --------------------------------------------------------------------------------------------- (e)
E_DENSE, E_LAG = 4, 1                  # the tensor of 4 elements is not deferred; the one of 67 counts 3 behind the clock
E_START = 3                            # steps before the first one: the lagging counter starts at 0
E_L2 = [1e-3, 2e-3, 5e-2, 1e-2, 1e-3, 3e-3, 1e-4]


def _masks_e(step):
    """~3 % of the chunks per step: 1 % the same every step, 2 % drawn per step, most never.  The planted chunks near
    the start are marked at steps 4 and 9 only (the step's own replay brings them up), those in the middle never (the
    flush does).  Every chunk of the lagging tensor is marked every step: its missed steps would be replayed with the
    clock's constants (include/xdfm.h), so it must never fall behind."""
    out = []
    for t, n in enumerate(R.SIZES):
        n4 = n // 4
        hot = np.random.RandomState(77 + t).rand(n4) < 0.01
        k = hot | (np.random.RandomState(1000 * step + t).rand(n4) < 0.02)
        for c in R.planted_chunks(n):
            k[c:c + 4] = c == 5 and step in (4, 9)
        if t in (E_LAG, E_DENSE):
            k[:] = True
        out.append(k)
    return out


def _grads_e(step):
    flat, marks, masks, offs = R.sparse_grads(R.SIZES, None, step, seed=9, chunks=_masks_e(step))
    o = offs[E_DENSE] // 4
    marks[o:o + 2] = 0                 # the tensor that is not deferred has no marks
    return flat, marks, masks, offs


@BX
@pytest.mark.parametrize("hp", ["H0", "H1", "H2", "H3", "H4", "H5"])
def test_deferred_scan_is_bit_identical_to_the_sweep(hp, bx):
    """Twelve steps of xdfm_adam_step_deferred (cap 16, flushes after steps 5 and 12) against the dense sweep of the same
    gradients: after each step the chunks marked in it are bit-equal and carry last == clock[0]; after each flush p, m, v
    of every tensor are bit-equal, every `last` byte is 0 and clock == {0, steps so far}.  The sum of l2_value plus the
    backlog matches the dense sweep's sum to 2e-6 relative and float64 to 1e-5 (H5: no float64, and L2 strengths scaled by
    1e-6 -- the weights reach 2.4e4 there and the backlog's 2^-40 fixed point holds values below 2^23)."""
    dev = _dev()
    state = R.make_state()
    l2 = [x * (1e-6 if hp == "H5" else 1.0) for x in E_L2]
    steps0 = [0 if t == E_LAG else E_START for t in range(N)]
    deferred = [t for t in range(N) if t != E_DENSE]
    flags = [0 if t == E_DENSE else R.DEFERRED for t in range(N)]
    use_marks = [t != E_DENSE for t in range(N)]
    sum_d = sum_l = 0.0
    with _adam_bx(bx):
        dense, lazy = R.Bank(state, dev, steps0=steps0), R.Bank(state, dev, steps0=steps0)
        _check_mark_pointers(lazy)
        clk = R.Clock(dev, cap=16, before=E_START)
        for s in range(1, 13):
            flat, marks, masks, _ = _grads_e(s)
            dense.set_grads(flat)
            vd = R.adam_step(dense, list(range(N)), l2, hp, s, want_l2=True)
            lazy.set_grads(flat, marks)
            vl = R.adam_step(lazy, list(range(N)), l2, hp, s, marked=use_marks, flags=flags, want_l2=True, clk=clk)
            torch.cuda.synchronize()
            sum_d += float(vd.item())
            sum_l += float(vl.item())
            t_now = clk.read()[0]
            assert t_now == (s if s <= 5 else s - 5)
            o = lazy.goff[E_DENSE]
            lazy.flat[o:o + 4].zero_()
            assert not bool(lazy.gbuf.any()) and not bool(lazy.marks.any()), "step %d: gradient / marks not re-zeroed" % s
            for t in deferred:
                sel = _elem_sel(masks[t], R.SIZES[t], dev)
                for name, la, da in (("p", lazy.p, dense.p), ("m", lazy.m, dense.m), ("v", lazy.v, dense.v)):
                    assert _same_bits(la[t], da[t], sel), "step %d: marked chunks of %s, tensor %d" % (s, name, t)
                got = lazy.last[t][:R.SIZES[t] // 4].cpu().numpy()
                assert (got[masks[t]] == t_now).all(), "step %d: last != clock[0] on marked chunks of tensor %d" % (s, t)
                assert (got <= t_now).all()
            _assert_banks_equal(dense, lazy, "step %d, the tensor that is not deferred" % s, [E_DENSE])
            if s in (5, 12):
                R.adam_flush(lazy, deferred, [l2[t] for t in deferred], clk, hp)
                torch.cuda.synchronize()
                _assert_banks_equal(dense, lazy, "after the flush at step %d" % s)
                assert all(not bool(x.any()) for x in lazy.last), "a `last` byte survived the flush"
                assert clk.read() == [0, E_START + s]
        sum_l += clk.take_backlog()
    assert [float(x) for x in lazy.steps.cpu()] == [12.0 + x for x in steps0]
    rel = abs(sum_l - sum_d) / abs(sum_d)
    print("adam deferred %s bx=%d: L2 sum dense %.9g deferred+backlog %.9g rel %.3g" % (hp, bx, sum_d, sum_l, rel))
    assert np.isfinite(sum_d) and rel <= 2e-6
    if hp != "H5":
        _, want = _f64_run(("e", hp), state, R.SIZES, lambda s: (lambda r: (r[0], r[3]))(_grads_e(s)), l2, hp, 12, steps0)
        share = abs(sum_l - sum(want)) / (R.L2_RTOL * sum(want))
        print("adam deferred %s bx=%d: share of the bar, L2 sum against float64 %.3f" % (hp, bx, share))
        assert share <= 1.0


# --------------------------------------------------------------------------------------------- (f)
F_VOCAB = (257, 3, 1003, 31)
F_B, F_M, F_LDX, F_COLS = 64, 4, 7, (4, 0, 2, 5)
F_L2_EMB, F_L2_LIN, F_L2_DENSE = [1e-3, 2e-3, 5e-2, 1e-2], [1e-2, 1e-3, 2e-3, 3e-3], 1e-3
F_DENSE_N = 4099


def _batch_f(step):
    """X [B, ldx] with Zipf-like ids (duplicates; 0 and V - 1 present), one id of V + 5 and one of -1."""
    rng = np.random.RandomState(4000 + step)
    X = rng.rand(F_B, F_LDX).astype(np.float32)
    ids = []
    for f, V in enumerate(F_VOCAB):
        i = np.minimum((V * rng.rand(F_B) ** 3).astype(np.int64), V - 1)
        i[0], i[1] = 0, V - 1
        raw = i.astype(np.float32)
        if f == 0:
            raw[5] = V + 5
            i[5] = V - 1
        if f == 2:
            raw[6] = -1
            i[6] = 0
        X[:, F_COLS[f]] = raw + (0.25 if f == 3 else 0.0)          # truncation, as the gather
        ids.append(i)
    return X, ids


def _case_f(hp, D, with_lin, skip_field):
    dev = _dev()
    sizes = [V * D for V in F_VOCAB] + ([V for V in F_VOCAB] if with_lin else []) + [F_DENSE_N]
    l2 = F_L2_EMB + (F_L2_LIN if with_lin else []) + [F_L2_DENSE]
    T = len(sizes)
    emb_idx, lin_idx, dense_idx = list(range(4)), (list(range(4, 8)) if with_lin else []), T - 1
    tables = emb_idx + lin_idx
    state = R.make_state(sizes, seed=21)
    width = [D] * 4 + [1] * len(lin_idx)
    skip = () if skip_field is None else (skip_field,)
    scan = [t for k, t in enumerate(tables) if (k % 4) in skip]           # tables left to the step's mark scan
    dense, lazy = R.Bank(state, dev), R.Bank(state, dev)
    clk = R.Clock(dev, cap=16)
    cols = torch.tensor(F_COLS, dtype=torch.int32, device=dev)
    vocab = torch.tensor(F_VOCAB, dtype=torch.int32, device=dev)
    emb_c = R.Rows(lazy, emb_idx, F_L2_EMB, with_grads=False)
    lin_c = R.Rows(lazy, lin_idx, F_L2_LIN, with_grads=False) if with_lin else None
    emb_a = R.Rows(lazy, emb_idx, F_L2_EMB, skip=skip)
    lin_a = R.Rows(lazy, lin_idx, F_L2_LIN, skip=skip) if with_lin else None
    grads = {}

    def grads_of(s):
        if s not in grads:
            _, ids = _batch_f(s)
            masks = []
            for k, t in enumerate(tables):
                w, n4 = width[k], sizes[t] // 4
                mk = np.zeros(n4 + 1, dtype=bool)
                for i in np.unique(ids[k % 4]):
                    mk[i * w // 4:(i * w + w - 1) // 4 + 1] = True
                masks.append(mk[:n4])
            masks.append(np.ones(F_DENSE_N // 4, dtype=bool))
            flat, marks, _, offs = R.sparse_grads(sizes, None, s, seed=13, chunks=masks)
            o = offs[dense_idx] // 4
            marks[o:o + F_DENSE_N // 4 + 1] = 0
            grads[s] = (flat, marks, offs)
        return grads[s]

    sum_d = sum_l = 0.0
    for s in range(1, 11):
        Xn, ids = _batch_f(s)
        X = torch.from_numpy(Xn).to(dev)
        R.adam_catchup_rows(X, cols, vocab, F_M, D, emb_c, lin_c, clk, hp)
        torch.cuda.synchronize()
        for k, t in enumerate(tables):              # the rows the gather is about to read: the dense sweep's bits
            w = width[k]
            el = (np.unique(ids[k % 4])[:, None] * w + np.arange(w)[None, :]).reshape(-1)
            sel = torch.from_numpy(el).to(dev)
            for name, la, da in (("p", lazy.p, dense.p), ("m", lazy.m, dense.m), ("v", lazy.v, dense.v)):
                assert _same_bits(la[t], da[t], sel), "step %d: %s of the batch's rows after the catch-up, table %d" % (s, name, t)
        flat, marks, _ = grads_of(s)
        dense.set_grads(flat)
        vd = R.adam_step(dense, list(range(T)), l2, hp, s, want_l2=True)
        lazy.set_grads(flat, marks)
        others = scan + [dense_idx]
        R.adam_step(lazy, others, [l2[t] for t in others], hp, s, marked=[True] * len(scan) + [False],
                    flags=[R.DEFERRED] * len(scan) + [0], want_l2=True, clk=clk)
        R.adam_apply_rows(X, cols, vocab, F_M, D, emb_a, lin_a, clk, hp, lazy.l2_value)
        torch.cuda.synchronize()
        sum_d += float(vd.item())
        sum_l += float(lazy.l2_value.item())
        o = lazy.goff[dense_idx]
        lazy.flat[o:o + F_DENSE_N].zero_()
        assert not bool(lazy.gbuf.any()) and not bool(lazy.marks.any()), "step %d: gradient / marks not re-zeroed" % s
        assert int(clk.cell.item()) == 0
        if s in (4, 10):
            R.adam_flush(lazy, tables, [l2[t] for t in tables], clk, hp)
            torch.cuda.synchronize()
            _assert_banks_equal(dense, lazy, "after the flush at step %d" % s)
            assert all(not bool(lazy.last[t].any()) for t in tables) and clk.read() == [0, s]
    sum_l += clk.take_backlog()
    rel = abs(sum_l - sum_d) / abs(sum_d)
    assert rel <= 2e-6, (sum_d, sum_l)
    _, want = _f64_run(("f", hp, D, with_lin), state, sizes, lambda s: (grads_of(s)[0], grads_of(s)[2]), l2, hp, 10)
    return rel, abs(sum_l - sum(want)) / (R.L2_RTOL * sum(want))


@pytest.mark.parametrize("D", [16, 10, 3])
@pytest.mark.parametrize("hp", ["H0", "H1", "H3"])
def test_rows_api_catchup_and_apply(hp, D):
    """xdfm_adam_catchup_rows / xdfm_adam_apply_rows called directly: m = 4 fields of vocab (257, 3, 1003, 31), B = 64,
    Zipf-like ids with duplicates, 0, V - 1, V + 5 and -1 (clamped, as the gather), with and without the linear tables,
    and once with field 2's `param` NULL in xdfm_adam_rows (that field is stepped by the scan).  Ten steps of catch-up,
    xdfm_adam_step_deferred over the other tensors, apply; flushes after steps 4 and 10.  After every catch-up the batch's
    rows have the dense sweep's bits; after every flush everything has; l2_value plus the backlog as in the scan's test."""
    for with_lin in (True, False):
        for skip_field in (None, 2):
            rel, share = _case_f(hp, D, with_lin, skip_field)
            print("adam rows %s D=%d lin=%d skip=%s: L2 sum rel to dense %.3g, share of the bar against float64 %.3f" % (
                hp, D, with_lin, skip_field, rel, share))
            assert share <= 1.0
