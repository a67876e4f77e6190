"""GPU tests (-m gpu) of K2v over exchanged rows (xdfm_varlen_pool_bwd_rows) through the C ABI: the backward of the pooled
variable-length lookup that a row-parallel step runs on every rank over all ranks' rows, without the forward's argpos.

The inputs have the shape `RowParallel.exchange_rows` hands over: ONE packed buffer [R, mD + ncols + 1] per launch, whose
column ranges are the row gradients (example-major, field slot s at column s * D), the rows of X and the linear-logit
gradient -- three strided views, ldx = ld_g = ld_lin = mD + ncols + 1.  R = 70 rows, the last 6 all zeros (the pad rows of a
ragged rank); vocabulary 7, so every table row collects many addends and the order of the reduction matters.

Bars: against the float64 restatement (tests/varlen_ref.py) the one tests/test_gpu_varlen.py applies to xdfm_varlen_pool_bwd,
(n + 2) * eps * sum |addends| per element with n the addends of that row, rows without addends exactly zero; against
xdfm_varlen_pool_bwd itself (same rows, contiguous FM layout, the forward's saved argpos): the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import varlen_ref as vr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
EPS = vr.EPS32
MODES = ("sum", "mean", "max")
R, NPAD, V, SLOT0 = 70, 6, 7, 2
SHAPES = [(D, (Tn, Tn, Tn)) for D in (4, 16) for Tn in (1, 5, 255)] + [(4, (5, 1, 255))]
IDS = ["D%d-T%s" % (D, "x".join(map(str, sorted(set(t))))) for D, t in SHAPES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Rows:
    """F = 3 fields: sum with a length column, mean and max masked by id != 0.  X columns: one that belongs to nobody, the
    id columns of the three fields, the length column."""

    def __init__(self, D, maxlens, seed=0, ties=False):
        rng = np.random.default_rng(seed)
        self.D, self.F, self.maxlens = D, 3, maxlens
        self.live = live = R - NPAD
        self.ncols = ncols = 1 + sum(maxlens) + 1
        self.len_col = ncols - 1
        X = np.zeros((R, ncols), np.float32)
        X[:live, 0] = rng.integers(0, 5, live)
        self.desc, self.tables, self.lins = [], [], []
        col = 1
        for f, (mode, Tn) in enumerate(zip(MODES, maxlens)):
            L = rng.integers(1 if mode == "max" else 0, Tn + 1, live)
            L[1], L[2] = 0, Tn                                        # an empty sequence and a full one
            if mode == "sum":
                ids = rng.integers(0, V, (live, Tn))                  # padded positions hold ids too
                X[:live, self.len_col] = L
                len_col = self.len_col
            else:
                ids = rng.integers(1, V, (live, Tn))
                ids[np.arange(Tn)[None, :] >= L[:, None]] = 0
                len_col = -1
            if ties and mode == "max" and Tn >= 2:
                ids[3, :] = 4                                         # every position holds the same row: all columns tie
                ids[4, :] = 0
                ids[4, :min(Tn, 4)] = [5, 2, 2, 5][:min(Tn, 4)]       # two pairs of equal rows
            X[:live, col:col + Tn] = ids
            self.desc.append((col, Tn, len_col, f, V))
            self.tables.append(rng.standard_normal((V, D)).astype(np.float32))
            self.lins.append(rng.standard_normal((V, 1)).astype(np.float32))
            col += Tn
        self.X = X
        m = SLOT0 + self.F
        self.d_emb = rng.standard_normal((m, R, D)).astype(np.float32)       # FM layout [m][R * D]
        self.d_dnn = rng.standard_normal((R, m * D + 3)).astype(np.float32)
        self.d_lin = rng.standard_normal(R).astype(np.float32)
        for a in (self.d_emb[:, live:], self.d_dnn[live:], self.d_lin[live:]):
            a[...] = 0                                                # the exchange pads a ragged rank with zero rows

    def ids(self, f, X=None):
        X = self.X if X is None else X
        col, Tn, len_col, _, _ = self.desc[f]
        return X[:, col:col + Tn], (None if len_col < 0 else X[:, len_col])

    def upstream(self, f, d_emb=None, d_dnn=None):
        d_emb = self.d_emb if d_emb is None else d_emb
        d_dnn = self.d_dnn if d_dnn is None else d_dnn
        s = SLOT0 + f
        return d_emb[s] + d_dnn[:, s * self.D:(s + 1) * self.D]              # one fp32 add

    def permuted(self, perm):
        """(X, d_emb, d_dnn, d_lin) with the live rows in the order `perm`, the pad rows where they were."""
        order = np.concatenate([perm, np.arange(self.live, R)])
        return self.X[order].copy(), self.d_emb[:, order].copy(), self.d_dnn[order].copy(), self.d_lin[order].copy()


class Device:
    def __init__(self, case, dev):
        from xdfm_amd import _lib
        self.lib, self.c, self.dev = _lib.load(), case, dev
        c = case
        self.tables = [T(t).to(dev) for t in c.tables]
        self.lins = [T(t).to(dev) for t in c.lins]
        self.host = (_lib.VarLenField * c.F)()
        for f, (col, Tn, len_col, comb, vocab) in enumerate(c.desc):
            h = self.host[f]
            h.table, h.lin = self.tables[f].data_ptr(), self.lins[f].data_ptr()
            h.col, h.maxlen, h.len_col, h.combiner, h.vocab = col, Tn, len_col, comb, vocab
        self.desc = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(dev)
        self.hostp = ctypes.cast(self.host, ctypes.c_void_p)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        shapes = [t.shape for t in c.tables] + [t.shape for t in c.lins]
        self.shapes, self.offs, off = shapes, [], 0
        for sh in shapes:
            self.offs.append(off)
            off += (sh[0] * sh[1] + 3) // 4 * 4
        self.total = off
        self.off_dev = torch.tensor(self.offs, dtype=torch.int64, device=dev)
        self.cols = torch.arange(c.F, dtype=torch.int32, device=dev)
        self.vocab = torch.tensor([d[4] for d in c.desc], dtype=torch.int32, device=dev)
        self.Tmax = max(c.maxlens)

    def _split(self, flat):
        return [flat[o:o + sh[0] * sh[1]].view(tuple(sh)) for o, sh in zip(self.offs, self.shapes)]

    def contiguous(self, X=None, d_emb=None, d_dnn=None, d_lin=None):
        """The forward (for its argpos) and xdfm_varlen_pool_bwd on contiguous inputs in FM layout."""
        c, lib, dev = self.c, self.lib, self.dev
        Xd = T(np.ascontiguousarray(c.X if X is None else X)).to(dev)
        n = Xd.shape[0]
        de = T(np.ascontiguousarray(c.d_emb if d_emb is None else d_emb)).to(dev)
        dd = T(np.ascontiguousarray(c.d_dnn if d_dnn is None else d_dnn)).to(dev)
        dl = T(np.ascontiguousarray(c.d_lin if d_lin is None else d_lin)).to(dev)
        m = SLOT0 + c.F
        emb = torch.zeros((m, n * c.D), device=dev)
        lin = torch.zeros(n, device=dev)
        self.argpos = torch.zeros((n, c.F, c.D + 1), dtype=torch.uint8, device=dev)
        rc = lib.xdfm_varlen_pool_fwd(_p(Xd), Xd.stride(0), n, _p(self.desc), self.hostp, c.F, c.D, SLOT0, _p(emb), None, 0, 0,
                                      _p(lin), _p(self.argpos), None, None)
        assert rc == 0, lib.xdfm_last_error()
        flat = torch.zeros(self.total, device=dev)
        ws = torch.empty(lib.xdfm_varlen_pool_bwd_ws_elems(n, c.F, c.D, self.Tmax), device=dev)
        rc = lib.xdfm_varlen_pool_bwd(_p(Xd), Xd.stride(0), n, _p(self.desc), self.hostp, c.F, c.D, SLOT0, _p(de), _p(dd),
                                      dd.stride(0), SLOT0 * c.D, _p(dl), 1, _p(self.argpos), _p(self.cols), _p(self.vocab),
                                      _p(flat), _p(self.off_dev[:c.F]), _p(self.off_dev[c.F:]), _p(ws), None)
        assert rc == 0, lib.xdfm_last_error()
        torch.cuda.synchronize()
        return self._split(flat)

    def rows(self, X=None, d_emb=None, d_dnn=None, d_lin=None):
        """xdfm_varlen_pool_bwd_rows on three views of one packed buffer, built as `exchange_rows` builds it."""
        c, lib, dev = self.c, self.lib, self.dev
        X = c.X if X is None else X
        d_emb = c.d_emb if d_emb is None else d_emb
        d_dnn = c.d_dnn if d_dnn is None else d_dnn
        d_lin = c.d_lin if d_lin is None else d_lin
        n, ncols, mD = X.shape[0], c.ncols, (SLOT0 + c.F) * c.D
        Q = np.full((n, mD + ncols + 1), 7.0, np.float32)
        Q[:, :mD] = (d_dnn[:, :mD].reshape(n, -1, c.D) + d_emb.transpose(1, 0, 2)).reshape(n, mD)    # one fp32 add
        Q[:, mD:mD + ncols] = X
        Q[:, mD + ncols] = d_lin
        G = T(Q).to(dev)
        Xv, Gv, dl = G[:, mD:mD + ncols], G[:, :mD], G[:, mD + ncols]
        assert Xv.stride(0) > ncols and not Xv.is_contiguous() and not Gv.is_contiguous() and dl.stride(0) > 1
        flat = torch.zeros(self.total, device=dev)
        ws = torch.empty(lib.xdfm_varlen_pool_bwd_rows_ws_elems(n, c.F, c.D, self.Tmax), device=dev)
        rc = lib.xdfm_varlen_pool_bwd_rows(_p(Xv), Xv.stride(0), n, _p(self.desc), self.hostp, c.F, c.D, SLOT0, _p(Gv),
                                           Gv.stride(0), _p(dl), dl.stride(0), _p(self.cols), _p(self.vocab), _p(flat),
                                           _p(self.off_dev[:c.F]), _p(self.off_dev[c.F:]), _p(ws), _p(self.flag), None)
        assert rc == 0, lib.xdfm_last_error()
        torch.cuda.synchronize()
        return self._split(flat)


def _check_vs_float64(c, grads, X=None, ups=None, d_lin=None):
    d_lin = c.d_lin if d_lin is None else d_lin
    for f, mode in enumerate(MODES):
        ids, lengths = c.ids(f, X)
        up = c.upstream(f) if ups is None else ups[f]
        for got, table, g, what in ((grads[f], c.tables[f], up, "table"), (grads[c.F + f], c.lins[f], d_lin[:, None], "linear table")):
            got = got.cpu().numpy()
            want, ab, n = vr.pool_grad(ids, lengths, table, mode, g)
            err, bar = np.abs(got - want), (n[:, None] + 2) * EPS * ab
            print("field %d %s %s: worst share of the bar %.3f, most addends per row %d" % (
                f, mode, what, float((err / np.maximum(bar, 1e-300)).max()), int(n.max())))
            assert np.all(err <= bar), "field %d %s %s" % (f, mode, what)
            assert np.all(got[n == 0] == 0), "field %d: rows without addends must be exactly zero" % f


def _same_bits(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s: gradient %d differs, max |diff| %.3g" % (what, k, float((x - y).abs().max()))


@pytest.mark.parametrize("D,maxlens", SHAPES, ids=IDS)
def test_gradients_equal_the_contiguous_backward_with_the_forwards_argpos(D, maxlens):
    dev = _dev()
    c = Rows(D, maxlens, seed=D + sum(maxlens))
    lengths = c.X[:c.live, c.len_col]
    assert (lengths == 0).any() and (lengths == maxlens[0]).any()
    d = Device(c, dev)
    got = d.rows()
    assert int(d.flag.item()) == 0
    _same_bits(got, d.contiguous(), "rows vs contiguous")       # the recomputed positions and the summation order
    _check_vs_float64(c, got)
    _same_bits(got, d.rows(), "run to run")


@pytest.mark.parametrize("D,maxlens", [s for s in SHAPES if s[1][2] >= 2], ids=[i for i, s in zip(IDS, SHAPES) if s[1][2] >= 2])
def test_ties_go_where_the_forward_sends_them(D, maxlens):
    """Two positions of a sequence hold the same id, so their rows tie in every column: the forward takes the first maximum,
    and the recomputation must send the gradient to that very position."""
    dev = _dev()
    c = Rows(D, maxlens, seed=3 * D + sum(maxlens), ties=True)
    d = Device(c, dev)
    want = d.contiguous()
    argpos = d.argpos.cpu().numpy()
    assert np.all(argpos[3, 2] == 0)                             # all positions equal: the first one
    pair = argpos[4, 2, :D]
    assert set(np.unique(pair)) <= {0, 1} and np.array_equal(pair == 0, c.tables[2][5] >= c.tables[2][2])
    got = d.rows()
    _same_bits(got, want, "rows vs contiguous, ties")
    _check_vs_float64(c, got)


@pytest.mark.parametrize("D,maxlens", SHAPES, ids=IDS)
def test_permuting_the_rows(D, maxlens):
    """The reduce is exact per chunk of 4096 positions: inside one chunk a permutation of the rows changes no bit; across
    chunks it changes what it changes for xdfm_varlen_pool_bwd under the same permutation, and nothing else."""
    dev = _dev()
    c = Rows(D, maxlens, seed=7 * D + sum(maxlens))
    d = Device(c, dev)
    base = d.rows()
    perm = np.random.default_rng(1).permutation(c.live)
    Xp, de, dd, dl = c.permuted(perm)
    got = d.rows(Xp, de, dd, dl)
    _same_bits(got, d.contiguous(Xp, de, dd, dl), "rows vs contiguous, permuted")
    ups = [c.upstream(f, de, dd) for f in range(c.F)]
    _check_vs_float64(c, got, X=Xp, ups=ups, d_lin=dl)
    if R * max(maxlens) <= 4096:
        _same_bits(got, base, "permuted vs not, one chunk")
    else:                                    # the sum field against its own unpermuted result: each within the bar, so twice the bar apart
        ids, lengths = c.ids(0)
        for k, table, up in ((0, c.tables[0], c.upstream(0)), (c.F, c.lins[0], c.d_lin[:, None])):
            _, ab, n = vr.pool_grad(ids, lengths, table, "sum", up)
            assert np.all(np.abs((got[k] - base[k]).cpu().numpy()) <= 2 * (n[:, None] + 2) * EPS * ab)


@pytest.mark.parametrize("D,maxlens", [(4, (5, 5, 5)), (16, (255, 255, 255))], ids=["D4-T5", "D16-T255"])
def test_pad_rows_add_exactly_nothing(D, maxlens):
    """Rows of zeros (ids 0, length 0) with zero gradients, as the exchange pads a ragged rank: every gradient is exactly
    zero -- the max field treats a pad row as the empty sequence it is and adds its gradient, an exact zero, to row 0.
    With gradients that are not zero, which the exchange never ships, the sum and mean fields still add nothing, and the
    max field hands them to row 0 as for any empty sequence."""
    dev = _dev()
    c = Rows(D, maxlens, seed=11)
    rng = np.random.default_rng(2)
    n, m = NPAD, SLOT0 + c.F
    X = np.zeros((n, c.ncols), np.float32)
    d = Device(c, dev)
    got = d.rows(X, np.zeros((m, n, D), np.float32), np.zeros((n, m * D + 3), np.float32), np.zeros(n, np.float32))
    for g in got:
        assert torch.count_nonzero(g).item() == 0
    de, dd = rng.standard_normal((m, n, D)).astype(np.float32), rng.standard_normal((n, m * D + 3)).astype(np.float32)
    dl = rng.standard_normal(n).astype(np.float32)
    got = d.rows(X, de, dd, dl)
    for k in (0, 1, c.F, c.F + 1):                               # sum and mean: tables and linear tables
        assert torch.count_nonzero(got[k]).item() == 0
    for k in (2, c.F + 2):                                       # max: row 0 and nothing else
        assert torch.count_nonzero(got[k][0]).item() == got[k][0].numel() and torch.count_nonzero(got[k][1:]).item() == 0
    _check_vs_float64(c, got, X=X, ups=[c.upstream(f, de, dd) for f in range(c.F)], d_lin=dl)
    _same_bits(got, d.contiguous(X, de, dd, dl), "rows vs contiguous, pad rows")
    assert int(d.flag.item()) == 0


def test_out_of_range_id_raises_the_deferred_flag():
    """An id equal to the vocabulary size, at a valid position and at a masked one: clamped by the kernel's own bounds check
    (the gradient goes to the last row, as K2 does it), and the flag behind the deferred IndexError is raised."""
    from xdfm_amd import ops
    dev = _dev()
    c = Rows(4, (5, 5, 5), seed=13)
    d = Device(c, dev)
    d.rows()
    assert int(d.flag.item()) == 0
    for f, row, pos, length in ((0, 5, 4, 2), (0, 6, 1, 3), (2, 7, 0, None)):       # masked, valid, valid in the max field
        bad = c.X.copy()
        col = c.desc[f][0]
        if length is not None:
            bad[row, c.len_col] = length
        bad[row, col + pos] = V
        d.flag.zero_()
        got = d.rows(X=bad)
        assert int(d.flag.item()) == 1, (f, row, pos)
        clamped = bad.copy()
        clamped[row, col + pos] = V - 1
        d.flag.zero_()
        _same_bits(got, d.rows(X=clamped), "bad id vs the clamped id")
        assert int(d.flag.item()) == 0
        _check_vs_float64(c, got, X=bad)                         # the restatement clamps as the kernels do
    # the same through the host wrapper: the plan's flag is the one `BaseModel._raise_on_bad_ids` turns into IndexError
    plan = ops.VarLenPlan([x[0] for x in c.desc], list(c.maxlens), [None if x[2] < 0 else x[2] for x in c.desc], list(MODES), [V] * 3,
                          c.D, SLOT0, SLOT0 * c.D)
    desc = plan.descriptors(d.tables, d.lins, dev)
    mD = (SLOT0 + c.F) * c.D
    G = torch.zeros((R, mD + c.ncols + 1), device=dev)
    G[:, mD:mD + c.ncols] = T(bad).to(dev)
    req = (plan, desc, [tuple(s) for s in d.shapes], (True,) * 6)
    ops.varlen_rows_grads(req, G[:, mD:mD + c.ncols], G[:, :mD], G[:, mD + c.ncols], G.stride(0))
    assert plan.check_ids(dev) and not plan.check_ids(dev)
