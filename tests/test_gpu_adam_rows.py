"""GPU tests (-m gpu) of the by-row kernels behind xdfm_adam_catchup_rows / xdfm_adam_apply_rows (csrc/adam.hip:
adam_catchup_by_row_kernel, adam_apply_by_row_kernel; csrc/table_step.h: tbl_claim_row), which take the calls where
D % 4 == 0 and option "adam_rows" is 1 (the default).  The update is a pure function of each chunk's state and `last`
byte, so everything is compared bit for bit: against the dense sweep (xdfm_adam_step_lr over every tensor, the path
tests/test_gpu_adam.py ties to float64) and against the by-chunk kernels (option "adam_rows" = 0) run on a second bank
through the same sequence of calls.

Every case: m = 4 fields of vocab (257, 3, 1003, 31) as tests/test_gpu_adam.py::test_rows_api_catchup_and_apply, ids with
duplicates, 0, V - 1, V + 5 and -1 (clamped, as the gather), ten steps of catch-up, xdfm_adam_step_deferred over the other
tensors, apply; flushes after steps 4 and 10.  The thread index is (field, example) with the field outermost, so one
field's examples are consecutive lanes: B = 64 is one wave per field, B = 200 gives m * B = 800 threads -- four blocks,
waves that hold two fields, and duplicates of an id that meet across waves and across blocks."""
import contextlib

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu

VOCAB = (257, 3, 1003, 31)
M, LDX, COLS = 4, 7, (4, 0, 2, 5)
L2_EMB, L2_LIN, L2_DENSE = [1e-3, 2e-3, 5e-2, 1e-2], [1e-2, 1e-3, 2e-3, 3e-3], 1e-3
DENSE_N = 4099
STEPS, FLUSH_AT = 10, (4, 10)
BY_ROW, BY_CHUNK = 1, 0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def _adam_rows(value):
    from xdfm_amd import _lib
    before = _lib.get_option("adam_rows")
    _lib.set_option("adam_rows", value)
    try:
        yield
    finally:
        _lib.set_option("adam_rows", before)


def _ran():
    from xdfm_amd import _lib
    return _lib.get_option("last_adam_rows")


def _to_X(ids, B, step):
    """X [B, ldx] from per-field ids; example 5 of field 0 asks for V + 5, example 6 of field 2 for -1 (both clamped), field
    3 carries a fraction (truncated).  -> X, the ids the kernels use."""
    rng = np.random.RandomState(7000 + step)
    X = rng.rand(B, LDX).astype(np.float32)
    out = []
    for f, V in enumerate(VOCAB):
        i = ids[f].copy()
        raw = i.astype(np.float32)
        if f == 0:
            raw[5], i[5] = V + 5, V - 1
        if f == 2:
            raw[6], i[6] = -1, 0
        X[:, COLS[f]] = raw + (0.25 if f == 3 else 0.0)
        out.append(i)
    return X, out


def zipf_batch(step, B):
    """Zipf-like ids: many duplicates of the small ids, 0 and V - 1 present."""
    rng = np.random.RandomState(4000 + step)
    ids = []
    for V in VOCAB:
        i = np.minimum((V * rng.rand(B) ** 3).astype(np.int64), V - 1)
        i[0], i[1] = 0, V - 1
        ids.append(i)
    return _to_X(ids, B, step)


def neighbour_batch(step, B):
    """Consecutive examples ask for consecutive ids, each id twice in a row: the lanes next to each other in a wave hold
    the rows that share a `last` word (four rows at D = 4, two at D = 8) and a duplicate of each."""
    ids = [(5 * step + np.arange(B) // 2) % V for V in VOCAB]
    return _to_X([i.astype(np.int64) for i in ids], B, step)


def _equal_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _assert_same(x, y, tensors, what, last=True):
    for t in tensors:
        for name, xa, ya in (("p", x.p, y.p), ("m", x.m, y.m), ("v", x.v, y.v)):
            if not _equal_bits(xa[t], ya[t]):
                bad = torch.nonzero(xa[t].view(torch.int32) != ya[t].view(torch.int32)).flatten()
                raise AssertionError("%s: %s of tensor %d differs in %d of %d elements, first at %d" % (
                    what, name, t, bad.numel(), x.sizes[t], int(bad[0])))
        if last:
            assert torch.equal(x.last[t], y.last[t]), "%s: `last` bytes of tensor %d" % (what, t)


def run_case(D, with_lin, B, batch, hp="H0", skip_field=None, scan_steps=()):
    """The sequence of the module's docstring on three banks: dense sweep, by-row kernels, by-chunk kernels.
    skip_field: a field whose `param` is NULL in xdfm_adam_rows of every apply (stepped by the mark scan).
    scan_steps: steps at which field 2 is left to the mark scan, on a gradient that marks every third chunk of its tables
    -- whatever the batch holds -- so that the chunks of a row end the step at different `last` bytes.
    -> `last` bytes of the embedding table of field 2 on the by-row bank before each catch-up (for the caller's own checks)."""
    dev = _dev()
    want_mode = BY_ROW if D % 4 == 0 else BY_CHUNK
    sizes = [V * D for V in VOCAB] + ([V for V in VOCAB] if with_lin else []) + [DENSE_N]
    l2 = L2_EMB + (L2_LIN if with_lin else []) + [L2_DENSE]
    T = len(sizes)
    emb_idx, lin_idx, dense_idx = list(range(4)), (list(range(4, 8)) if with_lin else []), T - 1
    tables = emb_idx + lin_idx
    width = [D] * 4 + [1] * len(lin_idx)
    state = R.make_state(sizes, seed=21)
    dense = R.Bank(state, dev)
    bank = {BY_ROW: R.Bank(state, dev), BY_CHUNK: R.Bank(state, dev)}
    clk = {k: R.Clock(dev, cap=16) for k in bank}
    cols = torch.tensor(COLS, dtype=torch.int32, device=dev)
    vocab = torch.tensor(VOCAB, dtype=torch.int32, device=dev)
    rows = {}

    def rows_of(mode, skip, with_grads):
        key = (mode, skip, with_grads)
        if key not in rows:
            e = R.Rows(bank[mode], emb_idx, L2_EMB, skip=skip, with_grads=with_grads)
            li = R.Rows(bank[mode], lin_idx, L2_LIN, skip=skip, with_grads=with_grads) if with_lin else None
            rows[key] = (e, li)
        return rows[key]

    def skip_at(s):
        return tuple(sorted(({skip_field} if skip_field is not None else set()) | ({2} if s in scan_steps else set())))

    batches, grads = {}, {}

    def batch_of(s):
        if s not in batches:
            batches[s] = batch(s, B)
        return batches[s]

    def grads_of(s):
        if s not in grads:
            _, ids = batch_of(s)
            masks = []
            for k, t in enumerate(tables):
                w, n4 = width[k], sizes[t] // 4
                mk = np.zeros(n4 + 1, dtype=bool)
                if k % 4 == 2 and s in scan_steps:
                    mk[::3] = True
                else:
                    for i in np.unique(ids[k % 4]):
                        mk[i * w // 4:(i * w + w - 1) // 4 + 1] = True
                masks.append(mk[:n4])
            masks.append(np.ones(DENSE_N // 4, dtype=bool))
            flat, marks, _, offs = R.sparse_grads(sizes, None, s, seed=13, chunks=masks)
            o = offs[dense_idx] // 4
            marks[o:o + DENSE_N // 4 + 1] = 0
            grads[s] = (flat, marks)
        return grads[s]

    seen_last = []
    for s in range(1, STEPS + 1):
        Xn, ids = batch_of(s)
        X = torch.from_numpy(Xn).to(dev)
        seen_last.append(bank[BY_ROW].last[2].cpu().numpy().copy())
        for mode in (BY_ROW, BY_CHUNK):
            emb_c, lin_c = rows_of(mode, (), False)
            with _adam_rows(mode):
                R.adam_catchup_rows(X, cols, vocab, M, D, emb_c, lin_c, clk[mode], hp)
                assert _ran() == (mode if want_mode == BY_ROW else BY_CHUNK)
        torch.cuda.synchronize()
        for k, t in enumerate(tables):              # the rows the gather is about to read: the dense sweep's bits
            w = width[k]
            el = (np.unique(ids[k % 4])[:, None] * w + np.arange(w)[None, :]).reshape(-1)
            sel = torch.from_numpy(el).to(dev)
            for name, la, da in (("p", bank[BY_ROW].p, dense.p), ("m", bank[BY_ROW].m, dense.m), ("v", bank[BY_ROW].v, dense.v)):
                assert torch.equal(la[t].view(torch.int32)[sel], da[t].view(torch.int32)[sel]), \
                    "step %d: %s of the batch's rows after the catch-up, table %d" % (s, name, t)
        _assert_same(bank[BY_ROW], bank[BY_CHUNK], tables, "step %d, after the catch-up, by row against by chunk" % s)
        assert int(clk[BY_ROW].backlog.item()) == int(clk[BY_CHUNK].backlog.item()), "step %d: backlog after the catch-up" % s
        flat, marks = grads_of(s)
        dense.set_grads(flat)
        R.adam_step(dense, list(range(T)), l2, hp, s, want_l2=True)
        skip = skip_at(s)
        scan = [t for k, t in enumerate(tables) if (k % 4) in skip]
        others = scan + [dense_idx]
        for mode in (BY_ROW, BY_CHUNK):
            b = bank[mode]
            b.set_grads(flat, marks)
            emb_a, lin_a = rows_of(mode, skip, True)
            b.steps += 1.0                          # every tensor's counter, as the optimizer does: the scan may get a table at any step
            R.adam_step(b, others, [l2[t] for t in others], hp, s, marked=[True] * len(scan) + [False],
                        flags=[R.DEFERRED] * len(scan) + [0], want_l2=True, clk=clk[mode], bump=False)
            with _adam_rows(mode):
                R.adam_apply_rows(X, cols, vocab, M, D, emb_a, lin_a, clk[mode], hp, b.l2_value)
                assert _ran() == (mode if want_mode == BY_ROW else BY_CHUNK)
        torch.cuda.synchronize()
        _assert_same(bank[BY_ROW], bank[BY_CHUNK], tables, "step %d, after the apply, by row against by chunk" % s)
        assert _equal_bits(bank[BY_ROW].l2_value, bank[BY_CHUNK].l2_value), "step %d: l2_value" % s
        for mode in (BY_ROW, BY_CHUNK):
            b = bank[mode]
            o = b.goff[dense_idx]
            b.flat[o:o + DENSE_N].zero_()
            assert not bool(b.gbuf.any()) and not bool(b.marks.any()), "step %d: gradient / marks not re-zeroed (mode %d)" % (s, mode)
            assert int(clk[mode].cell.item()) == 0
        if s in FLUSH_AT:
            for mode in (BY_ROW, BY_CHUNK):
                R.adam_flush(bank[mode], tables, [l2[t] for t in tables], clk[mode], hp)
            torch.cuda.synchronize()
            _assert_same(dense, bank[BY_ROW], tables + [dense_idx], "after the flush at step %d, dense against by row" % s, last=False)
            _assert_same(bank[BY_ROW], bank[BY_CHUNK], tables, "after the flush at step %d, by row against by chunk" % s)
            for mode in (BY_ROW, BY_CHUNK):
                assert all(not bool(bank[mode].last[t].any()) for t in tables) and clk[mode].read() == [0, s]
            assert int(clk[BY_ROW].backlog.item()) == int(clk[BY_CHUNK].backlog.item()), "backlog after the flush at step %d" % s
    return seen_last


@pytest.mark.parametrize("B", [64, 200])
@pytest.mark.parametrize("with_lin", [True, False], ids=["lin", "nolin"])
@pytest.mark.parametrize("D", [4, 8, 16, 32])
def test_by_row_matches_dense_sweep_and_by_chunk(D, with_lin, B):
    """Zipf-like ids.  D = 4 / 8: four / two rows per `last` word; D = 16: a row is one word; D = 32: two words."""
    run_case(D, with_lin, B, zipf_batch)


@pytest.mark.parametrize("B", [64, 200])
@pytest.mark.parametrize("D", [4, 8])
def test_rows_that_share_a_last_word_meet_in_one_wave(D, B):
    """The shared-word race: neighbouring lanes claim different bytes of ONE word, and the next lane the same byte again;
    a lane whose CAS loses must retry on the word it got back without touching the other rows' bytes."""
    run_case(D, True, B, neighbour_batch)


@pytest.mark.parametrize("D", [8, 16, 32])
def test_chunks_of_a_row_start_from_different_last_bytes(D):
    """Steps 2, 5 and 6 leave field 2 to the mark scan (`param` NULL in xdfm_adam_rows for those steps) on a gradient that
    marks every third chunk of its tables: those chunks go to the step's number, their neighbours in the same row stay
    behind, and the following catch-ups by row must replay each chunk from its own byte."""
    seen = run_case(D, True, 200, zipf_batch, scan_steps=(2, 5, 6))
    q = D // 4
    mixed = 0
    for s in (3, 6, 7, 8):                           # `last` of field 2's table as the catch-up of step s found it
        rows = seen[s - 1][:1003 * q].reshape(1003, q)
        mixed += int((rows.min(axis=1) != rows.max(axis=1)).sum())
    assert mixed > 100, "the case did not produce rows whose chunks differ in `last` (%d)" % mixed


@pytest.mark.parametrize("D", [4, 16, 32])
def test_a_field_left_to_the_scan_throughout(D):
    """Field 2's `param` is NULL in xdfm_adam_rows of every apply: its rows are caught up by row and stepped by the scan."""
    run_case(D, True, 200, zipf_batch, skip_field=2)


@pytest.mark.parametrize("D", [10, 3])
def test_rows_that_are_not_whole_chunks_take_the_by_chunk_kernels(D):
    """D % 4 != 0 (a row straddles chunks, V * D % 4 != 0 can occur): by chunk whatever the option says -- run_case asserts
    the probe "last_adam_rows" after every call -- and both settings of the option give the dense sweep's bits."""
    run_case(D, True, 64, zipf_batch)


def test_option_is_read_at_the_call():
    from xdfm_amd import _lib
    assert _lib.get_option("adam_rows") == 1
    dev = _dev()
    sizes = [V * 16 for V in VOCAB]
    b = R.Bank(R.make_state(sizes, seed=5), dev)
    clk = R.Clock(dev, cap=16)
    cols = torch.tensor(COLS, dtype=torch.int32, device=dev)
    vocab = torch.tensor(VOCAB, dtype=torch.int32, device=dev)
    X = torch.from_numpy(zipf_batch(1, 64)[0]).to(dev)
    emb = R.Rows(b, list(range(4)), L2_EMB, with_grads=False)
    for mode in (BY_CHUNK, BY_ROW):
        with _adam_rows(mode):
            R.adam_catchup_rows(X, cols, vocab, M, 16, emb, None, clk, "H0")      # clock 0: nothing to catch up
            assert _ran() == mode
    torch.cuda.synchronize()
    assert all(not bool(x.any()) for x in b.last)
