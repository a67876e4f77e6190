"""GPU tests (-m gpu) of the pooled variable-length fields: K1v / K2v through the C ABI against the float64 restatement
(tests/varlen_ref.py, pinned to the reference by tests/test_varlen_host.py), and the models against the reference's goldens.

Bars of the kernel tests (derived, eps = 2^-24):
  max forward            exact: a valid position carries w itself, a masked one the single fp32 subtraction w - 1e9;
  sum / mean forward     (maxlen + 2) * eps * sum_t |w_t| per element (mean: both sides divided by the fp32 divisor): at most
                         maxlen - 1 roundings of partial sums that never exceed sum |w_t|, one for the division, one for the
                         divisor;
  table gradients        (n + 2) * eps * sum |addends| per element, n = addends of that row: holds for any fp32 summation order
                         (K2 itself rounds once per chunk of 4096 positions), and covers one rounding of each addend;
  rows without addends   exactly zero.
No other bar is used below: the edge cases (empty max sequences, masked positions that do not tie, lengths outside 0..maxlen,
fractional ids, maxlen 255, D = 1 and 33, absent optional pointers, a strided d_lin) compare at these bars or bit for bit.

Empty max sequences: an all-masked sequence pools to w - 1e9 and its gradient goes to the masked position that won, row 0
under the id != 0 mask (tests/golden/varlen_pool_max_empty.npz, from the reference).  That golden is fed through the C ABI
and through ops.VarLenPool.  There is no whole-model golden with empty max sequences, on purpose: a pooled value of -1e9
saturates the head (the logit's sigmoid is 0 or 1 to the last bit and the loss is at its clamp), so a comparison of
predictions and gradients there would be ill-conditioned and say nothing about this stage."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import varlen_ref as vr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
EPS = vr.EPS32
MODES = ("sum", "mean", "max")
ARGPOS_FILL = 0xEE                      # what the argpos bytes hold before a forward: only the ones it must not write keep it


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Case:
    """Random inputs of one launch: fields = [(combiner, 'zero' | 'len', maxlen, vocab)].
    empty_max: share of the max sequences that are empty (examples 0 and B - 1 always among them when it is > 0).
    wild_lengths: length columns drawn from -1 .. maxlen + 3, some stored with a fraction (2.75 counts as 2, -0.5 as 0).
    scale: magnitude of the table entries (about 3 * scale at most)."""

    def __init__(self, B, D, fields, has_lin=True, seed=0, slot0=2, pad=3, empty_max=0.0, wild_lengths=False, scale=1.0):
        rng = np.random.default_rng(seed)
        self.B, self.D, self.fields, self.has_lin, self.slot0 = B, D, fields, has_lin, slot0
        self.F = F = len(fields)
        self.dnn_off, self.ld = slot0 * D, (slot0 + F) * D + pad
        ncol = 1 + sum(f[2] for f in fields) + F
        self.X = np.zeros((B, ncol), np.float32)
        self.X[:, 0] = rng.integers(0, 5, B)                      # a column that belongs to nobody
        self.desc, self.tables, self.lins, self.L = [], [], [], []
        col = 1
        for f, (mode, kind, Tn, V) in enumerate(fields):
            lo = 1 if mode == "max" else 0                         # max: at least one valid item, unless empty_max asks otherwise
            L = rng.integers(lo, Tn + 1, B)
            if mode != "max":
                L[rng.random(B) < 0.15] = 0                       # empty mean and sum rows
            elif empty_max > 0:
                L[rng.random(B) < empty_max] = 0                  # empty max rows: pooled to w - 1e9, gradient to the winning masked position
                L[0] = L[B - 1] = 0
            stored = L.astype(np.float32)
            if wild_lengths and kind == "len":
                L = rng.integers(-1, Tn + 4, B)
                L[:4] = (-1, 0, Tn, Tn + 3)
                frac = np.where(rng.random(B) < 0.4, 0.75, 0.0)
                frac[2] = 0.75
                stored = np.where(L >= 0, L + frac, L - 2 * frac / 3).astype(np.float32)      # -1 -> -1.5, which is still -1
                stored[(L == 0) & (rng.random(B) < 0.5)] = -0.5                                # and -0.5 is 0
                stored[1] = -0.5
                assert np.array_equal(np.trunc(stored), L) and np.any(stored != L) and L.min() == -1 and L.max() == Tn + 3
            if kind == "zero":
                ids = rng.integers(1, V, (B, Tn))
                ids[np.arange(Tn)[None, :] >= L[:, None]] = 0
                len_col = -1
            else:
                ids = rng.integers(0, V, (B, Tn))                  # padded positions hold ids too
                len_col = ncol - F + f
                self.X[:, len_col] = stored
            ids[0, :] = ids[0, 0]                                  # a sequence with the same id repeated
            self.X[:, col:col + Tn] = ids
            self.desc.append((col, Tn, len_col, MODES.index(mode), V))
            self.L.append(L)
            self.tables.append((scale * rng.standard_normal((V, D))).astype(np.float32))
            self.lins.append((scale * rng.standard_normal((V, 1))).astype(np.float32))
            col += Tn
        self.lin0 = rng.standard_normal(B).astype(np.float32)
        self.d_emb = rng.standard_normal((slot0 + F, B * D)).astype(np.float32)
        self.d_dnn = rng.standard_normal((B, self.ld)).astype(np.float32)
        self.d_lin = rng.standard_normal(B).astype(np.float32)

    def ids(self, f, X=None):
        X = self.X if X is None else X
        col, Tn, len_col, _, _ = self.desc[f]
        return X[:, col:col + Tn], (None if len_col < 0 else X[:, len_col])


class Device:
    """The case's arrays on the GPU and the two entry points.  Every optional pointer can be left out (the keyword
    arguments); what a call leaves out keeps the value it was filled with."""

    def __init__(self, case, dev, X=None, null_tables=False):
        from xdfm_amd import _lib
        self.lib, self.c, self.dev = _lib.load(), case, dev
        c = case
        self.X = T(np.ascontiguousarray(c.X if X is None else X)).to(dev)
        self.tables = [T(t).to(dev) for t in c.tables]
        self.lins = [T(t).to(dev) for t in c.lins]
        self.host = (_lib.VarLenField * c.F)()
        for f, (col, Tn, len_col, comb, V) in enumerate(c.desc):
            h = self.host[f]
            h.table = None if null_tables else self.tables[f].data_ptr()
            h.lin = self.lins[f].data_ptr() if c.has_lin else None
            h.col, h.maxlen, h.len_col, h.combiner, h.vocab = col, Tn, len_col, comb, V
        self.desc = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def forward(self, lin0=None, emb=True, dnn=True, lin=True, argpos=True):
        c, B = self.c, self.X.shape[0]
        self.emb = torch.full((c.slot0 + c.F, B * c.D), 7.0, device=self.dev)
        self.dnn = torch.full((B, c.ld), 7.0, device=self.dev)
        self.lin = T((c.lin0 if lin0 is None else lin0).copy()).to(self.dev) if c.has_lin else None
        self.argpos = torch.full((B, c.F, c.D + 1), ARGPOS_FILL, dtype=torch.uint8, device=self.dev)
        rc = self.lib.xdfm_varlen_pool_fwd(_p(self.X), self.X.stride(0), B, _p(self.desc), ctypes.cast(self.host, ctypes.c_void_p),
                                           c.F, c.D, c.slot0, _p(self.emb if emb else None), _p(self.dnn if dnn else None), c.ld,
                                           c.dnn_off, _p(self.lin if lin else None), _p(self.argpos if argpos else None),
                                           _p(self.flag), None)
        assert rc == 0, self.lib.xdfm_last_error()
        torch.cuda.synchronize()
        return self.emb.cpu().numpy(), self.dnn.cpu().numpy(), (self.lin.cpu().numpy() if c.has_lin else None)

    def backward(self, d_emb=None, d_dnn=None, d_lin=None, use_emb=True, use_dnn=True, tab=True, lin=True, lin_pitch=1,
                 argpos=True, fill=0.0, rc=0):
        """The F table gradients, then the F linear-table gradients.  `fill`: what the gradient buffer holds before the call
        in the parts that the call must not touch (all of it when the call is to be refused, rc = 1)."""
        c, B = self.c, self.X.shape[0]
        shapes = [t.shape for t in c.tables] + ([t.shape for t in c.lins] if c.has_lin else [])
        offs, off = [], 0
        for sh in shapes:
            offs.append(off)
            off += (sh[0] * sh[1] + 3) // 4 * 4
        flat = torch.zeros(off, device=self.dev)
        for k, (o, sh) in enumerate(zip(offs, shapes)):
            if rc or not (tab if k < c.F else lin):
                flat[o:o + sh[0] * sh[1]] = fill
        off_dev = torch.tensor(offs, dtype=torch.int64, device=self.dev)
        cols = torch.arange(c.F, dtype=torch.int32, device=self.dev)
        vocab = torch.tensor([d[4] for d in c.desc], dtype=torch.int32, device=self.dev)
        Tmax = max(d[1] for d in c.desc)
        ws = torch.empty(self.lib.xdfm_varlen_pool_bwd_ws_elems(B, c.F, c.D, Tmax), device=self.dev)
        de = T(c.d_emb if d_emb is None else d_emb).to(self.dev) if use_emb else None
        dd = T(c.d_dnn if d_dnn is None else d_dnn).to(self.dev) if use_dnn else None
        dl = None
        if c.has_lin:
            buf = torch.full((B, lin_pitch), 1e30, device=self.dev)             # d_lin is column lin_pitch // 2 of it
            buf[:, lin_pitch // 2] = T(c.d_lin if d_lin is None else d_lin).to(self.dev)
            dl = buf[:, lin_pitch // 2]
        got = self.lib.xdfm_varlen_pool_bwd(_p(self.X), self.X.stride(0), B, _p(self.desc), ctypes.cast(self.host, ctypes.c_void_p),
                                            c.F, c.D, c.slot0, _p(de), _p(dd), c.ld, c.dnn_off, _p(dl), lin_pitch,
                                            _p(self.argpos if argpos else None), _p(cols), _p(vocab), _p(flat),
                                            _p(off_dev[:c.F]) if tab else None,
                                            _p(off_dev[c.F:]) if c.has_lin and lin else None, _p(ws), None)
        assert got == rc, self.lib.xdfm_last_error()
        torch.cuda.synchronize()
        flat = flat.cpu().numpy()
        return [flat[o:o + sh[0] * sh[1]].reshape(sh) for o, sh in zip(offs, shapes)]


def _check_forward(c, emb, dnn, lin, X=None):
    B, D, F = c.B, c.D, c.F
    lin_want, lin_bar = c.lin0.astype(np.float64), np.zeros(B)
    lin_mag = np.abs(c.lin0).astype(np.float64)
    for f, (mode, kind, Tn, V) in enumerate(c.fields):
        ids, lengths = c.ids(f, X)
        got = emb[c.slot0 + f].reshape(B, D)
        np.testing.assert_array_equal(got, dnn[:, c.dnn_off + f * D:c.dnn_off + (f + 1) * D])     # both consumers get the same bits
        want, mag, _ = vr.pool(ids, lengths, c.tables[f], mode)
        if mode == "max":
            np.testing.assert_array_equal(got, want, err_msg="field %d max" % f)
        else:
            err, bar = np.abs(got - want), (Tn + 2) * EPS * mag
            print("field %d %s/%s maxlen %d: worst share of the bar %.3f" % (f, mode, kind, Tn, float((err / np.maximum(bar, 1e-300)).max())))
            assert np.all(err <= bar), "field %d %s" % (f, mode)
            assert np.all(got[mag.sum(1) == 0] == 0)                                              # empty rows pool to zero
        if c.has_lin:
            lw, lm, _ = vr.pool(ids, lengths, c.lins[f], mode)
            lin_want += lw[:, 0].astype(np.float64)
            lin_mag += np.abs(lw[:, 0]).astype(np.float64)
            if mode != "max":
                lin_bar += (Tn + 2) * EPS * lm[:, 0]
    assert np.all(emb[:c.slot0] == 7.0) and np.all(dnn[:, :c.dnn_off] == 7.0) and np.all(dnn[:, c.dnn_off + F * D:] == 7.0)
    if c.has_lin:
        # the F pooled values are added up and then added to what was there: F + 1 more roundings of sums <= lin_mag
        assert np.all(np.abs(lin - lin_want) <= lin_bar + (F + 1) * EPS * lin_mag)


def _upstream(c, d_emb=None, d_dnn=None):
    d_emb = c.d_emb if d_emb is None else d_emb
    d_dnn = c.d_dnn if d_dnn is None else d_dnn
    return [d_emb[c.slot0 + f].reshape(-1, c.D) + d_dnn[:, c.dnn_off + f * c.D:c.dnn_off + (f + 1) * c.D] for f in range(c.F)]   # one fp32 add


def _check_backward(c, grads, X=None, ups=None, d_lin=None):
    ups = _upstream(c) if ups is None else ups
    d_lin = c.d_lin if d_lin is None else d_lin
    for f, (mode, kind, Tn, V) in enumerate(c.fields):
        ids, lengths = c.ids(f, X)
        todo = [(grads[f], c.tables[f], ups[f], "table")]
        if c.has_lin:
            todo.append((grads[c.F + f], c.lins[f], d_lin[:, None], "linear table"))
        for got, table, up, what in todo:
            want, ab, n = vr.pool_grad(ids, lengths, table, mode, up)
            err, bar = np.abs(got - want), (n[:, None] + 2) * EPS * ab
            print("field %d %s/%s %s: worst share of the bar %.3f, most addends per row %d" % (
                f, mode, kind, what, float((err / np.maximum(bar, 1e-300)).max()), int(n.max())))
            assert np.all(err <= bar), "field %d %s %s" % (f, mode, what)
            assert np.all(got[n == 0] == 0), "field %d: rows without addends must be exactly zero" % f


def _check_argpos(c, argpos, X=None):
    """The recorded positions against the restatement's first maxima, evaluated in fp32 as the kernel evaluates them: exact.
    Column D is the linear table's; 0 for sum and mean fields."""
    for f, (mode, kind, Tn, V) in enumerate(c.fields):
        ids, lengths = c.ids(f, X)
        want = np.zeros((c.B, c.D + 1), np.int64)
        if mode == "max":
            want[:, :c.D] = vr.pool(ids, lengths, c.tables[f], "max")[2]
            want[:, c.D] = vr.pool(ids, lengths, c.lins[f], "max")[2][:, 0]
        w = c.D + 1 if c.has_lin else c.D
        np.testing.assert_array_equal(argpos[:, f, :w], want[:, :w], err_msg="field %d argpos" % f)
        if not c.has_lin:
            assert np.all(argpos[:, f, c.D] == ARGPOS_FILL)


def _check_empty_max(c, grads):
    """Empty max sequences without the restatement.  Under the id != 0 mask id 0 sits at masked positions only, so row 0 of
    the table collects exactly the upstream gradients of the empty examples, and row 0 of the linear table their d_lin.
    (The length-masked max field, whose empty sequences hand their gradient to the row of whatever id won, is left to the
    restatement.)  Returns the number of rows checked."""
    ups = _upstream(c)
    seen = 0
    for f, (mode, kind, Tn, V) in enumerate(c.fields):
        if (mode, kind) != ("max", "zero"):
            continue
        ids, _ = c.ids(f)
        empty = np.all(ids == 0, axis=1)
        assert empty[0] and empty[-1] and np.array_equal(empty, c.L[f] == 0)
        assert empty.all() or 0.1 < empty.mean() < 0.35                  # about one in five
        todo = [(grads[f], ups[f].astype(np.float64), "table")]
        if c.has_lin:
            todo.append((grads[c.F + f], c.d_lin[:, None].astype(np.float64), "linear table"))
        for got, up, what in todo:
            want, ab = up[empty].sum(0), np.abs(up[empty]).sum(0)
            assert np.all(want != 0), "field %d %s: the case must put a gradient on row 0" % (f, what)
            err, bar = np.abs(got[0] - want), (int(empty.sum()) + 2) * EPS * ab
            print("field %d max/zero %s: row 0 collects %d empty sequences, worst share of the bar %.3f" % (
                f, what, int(empty.sum()), float((err / bar).max())))
            assert np.all(err <= bar), "field %d %s row 0" % (f, what)
            seen += 1
    return seen


def _dominating_row(c):
    """maxlen = 255: row V - 1 of the max table dominates every column (and the linear table); its id sits at position 254
    only in example 3 (a full sequence) and at position 128 only in example 5."""
    rng = np.random.default_rng(255)
    col, Tn, _, _, V = c.desc[0]
    assert Tn == 255 and c.fields[0][:2] == ("max", "zero")
    ids = c.X[:, col:col + Tn]
    ids[3] = rng.integers(1, V - 1, Tn)
    ids[5] = 0
    ids[5, :200] = rng.integers(1, V - 1, 200)
    ids[3, 254] = ids[5, 128] = V - 1
    c.tables[0][V - 1] = 50 + np.abs(c.tables[0][V - 1])
    c.lins[0][V - 1] = 50 + np.abs(c.lins[0][V - 1])
    c.want_pos = {3: 254, 5: 128}


MIX_A = lambda t: [("mean", "zero", t[0], 13), ("sum", "len", t[1], 7), ("max", "zero", t[2], 9)]
MIX_B = lambda t: [("max", "len", t[0], 11), ("mean", "len", t[1], 2), ("sum", "zero", t[2], 300)]
EMPTY = [("max", "zero", 5, 9), ("max", "len", 5, 9), ("mean", "zero", 3, 13)]
CASES = {
    "B1-D4-F1":            dict(B=1, D=4, fields=[("sum", "zero", 1, 5)]),
    "B67-D10-F3":          dict(B=67, D=10, fields=MIX_A((3, 20, 1))),
    "B300-D16-F3":         dict(B=300, D=16, fields=MIX_B((20, 3, 20))),          # 6000 positions per field: two chunks of K2's reduce
    "B67-D16-F1-vocab2":   dict(B=67, D=16, fields=[("mean", "len", 20, 2)], has_lin=False),   # every position hits one of two rows
    "B300-D4-F3-nolin":    dict(B=300, D=4, fields=MIX_A((1, 3, 20)), has_lin=False),
    "B1-D10-F3":           dict(B=1, D=10, fields=MIX_B((3, 1, 20))),
    "B300-D10-F1-max":     dict(B=300, D=10, fields=[("max", "zero", 20, 2)]),
    # about one max sequence in five is empty, examples 0 and B - 1 among them; then every sequence of a tiny batch
    "B67-D4-F3-emptymax":  dict(B=67, D=4, fields=EMPTY, empty_max=0.2),
    "B3-D4-F3-allempty":   dict(B=3, D=4, fields=EMPTY, empty_max=1.0),
    # table entries up to about 1e3: fp32 numbers are 64 apart at 1e9, so the masked values w - 1e9f differ between positions
    "B67-D4-F1-notie":     dict(B=67, D=4, fields=[("max", "len", 5, 7)], empty_max=0.2, scale=400.0),
    # lengths -1 .. 8 for maxlen 5, some with a fraction: the mean divides by float(long(length)) + 1e-8f, not by the count
    "B67-D10-F2-lengths":  dict(B=67, D=10, fields=[("mean", "len", 5, 7), ("sum", "len", 5, 7)], wild_lengths=True),
    # positions >= 128 in the byte, a short field padded up to Tmax = 255, B * Tmax = 4845: two chunks of K2's reduce
    "B19-D3-F2-T255":      dict(B=19, D=3, fields=[("max", "zero", 255, 9), ("sum", "len", 1, 5)], tweak=_dominating_row),
    # K2 takes the columns in slices: D = 1 is one slice with one live column, D = 33 leaves a slice with one column
    "B67-D1-F3":           dict(B=67, D=1, fields=MIX_A((3, 20, 1))),
    "B67-D33-F3":          dict(B=67, D=33, fields=MIX_A((3, 20, 1))),
}


def _case(name, seed=None):
    kw = dict(CASES[name])
    tweak = kw.pop("tweak", None)
    c = Case(seed=sum(map(ord, name)) if seed is None else seed, **kw)
    if tweak is not None:
        tweak(c)
    return c


@pytest.mark.parametrize("name", list(CASES))
def test_pool_kernels_vs_float64(name):
    dev = _dev()
    c = _case(name)
    d = Device(c, dev)
    emb, dnn, lin = d.forward()
    _check_forward(c, emb, dnn, lin)
    argpos = d.argpos.cpu().numpy()
    _check_argpos(c, argpos)
    assert int(d.flag.item()) == 0
    grads = d.backward()
    _check_backward(c, grads)
    again = d.backward()
    for a, b in zip(grads, again):
        np.testing.assert_array_equal(a, b)                                 # bit-identical from run to run
    if CASES[name].get("empty_max") and CASES[name]["fields"] is EMPTY:
        assert _check_empty_max(c, grads) == 2                              # row 0 of the zero-mask max table and of its linear table
    if name == "B67-D4-F1-notie":
        _check_notie(c, argpos)
    if name == "B67-D10-F2-lengths":
        _check_lengths(c, emb)
    if name == "B19-D3-F2-T255":
        for b, pos in c.want_pos.items():
            assert np.all(argpos[b, 0] == pos), (b, argpos[b, 0])
            assert np.all(emb[c.slot0].reshape(c.B, c.D)[b] == c.tables[0][-1])


def _check_notie(c, argpos):
    """The inputs do what the case is for: among the all-masked sequences some do not put their maximum at position 0, and a
    kernel that compared w before subtracting 1e9 (no rounding to the 64-spaced grid, so no ties) would pick another
    position than the first maximum of the rounded values somewhere."""
    ids, lengths = c.ids(0)
    empty = c.L[0] == 0
    rows = c.tables[0][ids.astype(np.int64)]                                  # [B, T, D] fp32
    v = rows - np.float32(1e9)
    assert v.dtype == np.float32 and np.unique(v[empty]).size > 8             # the masked values differ
    assert np.any(argpos[empty, 0, :c.D] != 0)
    assert np.any(rows[empty].argmax(1) != v[empty].argmax(1))
    partly = (c.L[0] > 0) & (c.L[0] < 5)
    assert partly.any() and np.all(argpos[partly, 0, :c.D] < c.L[0][partly, None])    # a valid item beats every masked one here


def _check_lengths(c, emb):
    """Lengths above maxlen without the restatement: all five positions count and the divisor is the length itself."""
    ids, _ = c.ids(0)
    L = c.L[0]
    over = L > 5
    assert over.sum() >= 5 and (L == -1).any() and (L == 0).any()
    rows = c.tables[0][ids.astype(np.int64)].astype(np.float64)
    div = (L[over].astype(np.float32) + np.float32(1e-8)).astype(np.float64)[:, None]
    want, mag = rows[over].sum(1) / div, np.abs(rows[over]).sum(1) / div
    got = emb[c.slot0].reshape(c.B, c.D)[over]
    assert np.all(np.abs(got - want) <= (5 + 2) * EPS * mag)                  # the mean forward's bar at maxlen 5
    assert np.all(emb[c.slot0].reshape(c.B, c.D)[L <= 0] == 0) and np.all(emb[c.slot0 + 1].reshape(c.B, c.D)[c.L[1] <= 0] == 0)


def test_permuting_the_examples():
    """The forward is a function of the example alone: bit-identical per example.  The table gradients are exact sums per
    chunk of K2's reduce; across the two chunks of this case the grouping changes with the order, so they keep the bar."""
    dev = _dev()
    c = _case("B300-D16-F3", seed=5)
    emb, dnn, lin = Device(c, dev).forward()
    perm = np.random.default_rng(1).permutation(c.B)
    Xp = c.X[perm]
    dp = Device(c, dev, X=Xp)
    emb_p, dnn_p, lin_p = dp.forward(lin0=c.lin0[perm])
    np.testing.assert_array_equal(emb_p[c.slot0:].reshape(c.F, c.B, c.D), emb[c.slot0:].reshape(c.F, c.B, c.D)[:, perm])
    np.testing.assert_array_equal(dnn_p, dnn[perm])
    np.testing.assert_array_equal(lin_p, lin[perm])
    d_emb_p = c.d_emb.reshape(-1, c.B, c.D)[:, perm].reshape(c.d_emb.shape).copy()
    d_dnn_p, d_lin_p = c.d_dnn[perm].copy(), c.d_lin[perm].copy()
    grads = dp.backward(d_emb_p, d_dnn_p, d_lin_p)
    _check_backward(c, grads, X=Xp, ups=_upstream(c, d_emb_p, d_dnn_p), d_lin=d_lin_p)


def test_out_of_range_id_at_a_padded_position_raises_the_flag():
    """The reference looks up every position, padded ones included (inputs.py:224-225), so an id outside the table is
    an error wherever it sits; the kernel clamps it and raises K1's deferred flag."""
    dev = _dev()
    c = Case(seed=9, B=67, D=4, fields=[("sum", "len", 3, 7), ("mean", "zero", 3, 5)])
    col, Tn, len_col, _, V = c.desc[0]
    c.X[5, len_col] = 1
    d = Device(c, dev)
    d.forward()
    assert int(d.flag.item()) == 0
    bad = c.X.copy()
    bad[5, col + 2] = V                                       # position 2 of a sequence of length 1
    d = Device(c, dev, X=bad)
    emb, dnn, lin = d.forward()
    assert int(d.flag.item()) == 1
    _check_forward(c, emb, dnn, lin, X=bad)                   # the masked position changes nothing
    neg = c.X.copy()
    neg[7, c.desc[1][0]] = -2.0
    d = Device(c, dev, X=neg)
    d.forward()
    assert int(d.flag.item()) == 1


def test_fractional_ids_truncate_like_tensor_long():
    """Zero-mask fields: 0.75 added to every id at a valid position leaves the id what it was, and -0.5 at padded positions
    truncates to 0 -- masked, not out of range, no flag.  Everything equals the whole-number twin bit for bit."""
    dev = _dev()
    c = Case(seed=33, B=67, D=4, fields=[("mean", "zero", 5, 13), ("max", "zero", 5, 9), ("sum", "zero", 3, 7)], empty_max=0.2)
    rng = np.random.default_rng(34)
    Xf = c.X.copy()
    for col, Tn, _, _, _ in c.desc:
        block = Xf[:, col:col + Tn]                              # a view
        valid = block != 0
        block[valid] += 0.75
        block[~valid & (rng.random(block.shape) < 0.5)] = -0.5
    assert np.any(Xf == -0.5) and np.any(Xf % 1 == 0.75) and np.array_equal(np.trunc(Xf), c.X)
    whole, frac = Device(c, dev), Device(c, dev, X=Xf)
    out_w, out_f = whole.forward(), frac.forward()
    assert int(whole.flag.item()) == 0 and int(frac.flag.item()) == 0
    for a, b in zip(out_w, out_f):
        np.testing.assert_array_equal(a, b)
    assert torch.equal(whole.argpos, frac.argpos)
    _check_forward(c, *out_f, X=Xf)
    for a, b in zip(whole.backward(), frac.backward()):
        np.testing.assert_array_equal(a, b)


def test_optional_pointers_and_strides():
    """Each output, gradient and offset array left out in turn: what is still computed has the bits of the full call, what
    is left out keeps its fill.  d_lin with a row stride.  A max field without argpos is refused before anything is launched."""
    dev = _dev()
    c = _case("B67-D10-F3")
    F, D, s0 = c.F, c.D, c.slot0
    d = Device(c, dev)
    emb, dnn, lin = d.forward()
    argpos = d.argpos.cpu().numpy()
    _check_forward(c, emb, dnn, lin)
    # ---- forward
    e, n, l = d.forward(dnn=False, lin=False)                              # emb_fm alone
    np.testing.assert_array_equal(e, emb)
    assert np.all(n == 7.0) and np.array_equal(l, c.lin0)
    a = d.argpos.cpu().numpy()
    assert np.array_equal(a[:, :, :D], argpos[:, :, :D]) and np.all(a[:, :, D] == ARGPOS_FILL)    # the linear column's thread does not run
    e, n, l = d.forward(emb=False, lin=False)                              # dnn_in alone
    np.testing.assert_array_equal(n, dnn)
    assert np.all(e == 7.0) and np.array_equal(l, c.lin0)
    nt = Device(c, dev, null_tables=True)                                  # lin_out alone, no table in the descriptors
    e, n, l = nt.forward(emb=False, dnn=False)
    np.testing.assert_array_equal(l, lin)
    assert np.all(e == 7.0) and np.all(n == 7.0)
    a = nt.argpos.cpu().numpy()
    assert np.array_equal(a[:, :, D], argpos[:, :, D]) and np.all(a[:, :, :D] == ARGPOS_FILL)
    d.forward()                                                            # the full call's argpos again, for the backward
    # ---- backward
    full = d.backward()
    _check_backward(c, full)
    zeros_e, zeros_d = np.zeros_like(c.d_emb), np.zeros_like(c.d_dnn)
    for kw, twin, ups in ((dict(use_dnn=False), dict(d_dnn=zeros_d), _upstream(c, d_dnn=zeros_d)),
                          (dict(use_emb=False), dict(d_emb=zeros_e), _upstream(c, d_emb=zeros_e))):
        got = d.backward(**kw)                                             # one of the two row gradients absent: it counts as zeros
        for x, y in zip(got, d.backward(**twin)):
            np.testing.assert_array_equal(x, y)
        _check_backward(c, got, ups=ups)
        for x, y in zip(got[F:], full[F:]):
            np.testing.assert_array_equal(x, y)
    got = d.backward(tab=False, fill=7.0)                                  # tab_off = NULL: the linear tables alone
    assert all(np.all(g == 7.0) for g in got[:F])
    for x, y in zip(got[F:], full[F:]):
        np.testing.assert_array_equal(x, y)
    got = d.backward(lin=False, fill=7.0)                                  # lin_off = NULL: the tables alone
    assert all(np.all(g == 7.0) for g in got[F:])
    for x, y in zip(got[:F], full[:F]):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(d.backward(lin_pitch=3), full):                        # d_lin = column 1 of a [B, 3] buffer
        np.testing.assert_array_equal(x, y)
    got = d.backward(argpos=False, fill=7.0, rc=1)                         # field 2 pools by max
    assert b"a max-pooled field needs argpos of the forward" in d.lib.xdfm_last_error()
    assert all(np.all(g == 7.0) for g in got)
    # ---- argpos = NULL where no field pools by max
    c2 = Case(seed=41, B=67, D=10, fields=[("mean", "zero", 3, 13), ("sum", "len", 20, 7)])
    d2 = Device(c2, dev)
    out = d2.forward()
    assert np.all(d2.argpos.cpu().numpy() == 0)
    full2 = d2.backward()
    _check_backward(c2, full2)
    for x, y in zip(d2.forward(argpos=False), out):
        np.testing.assert_array_equal(x, y)
    assert np.all(d2.argpos.cpu().numpy() == ARGPOS_FILL)
    for x, y in zip(d2.backward(argpos=False), full2):
        np.testing.assert_array_equal(x, y)


def _golden_case(g):
    """tests/golden/varlen_pool_max_empty.npz as a case of one field: the reference's upstream gradient arrives as d_emb_fm
    (d_dnn_in is zero, so the one fp32 add changes nothing), the linear table's as d_lin; lin_out starts at zero."""
    B, Tn = g["ids"].shape
    V, D = g["table"].shape
    c = Case(B=B, D=D, fields=[("max", "zero", Tn, V)], seed=1, slot0=0, pad=0)
    col = c.desc[0][0]
    c.X[:, col:col + Tn] = g["ids"]
    c.L[0] = (g["ids"] != 0).sum(1)
    c.tables, c.lins = [g["table"].copy()], [g["lin_table"].copy()]
    c.lin0 = np.zeros(B, np.float32)
    c.d_emb = np.ascontiguousarray(g["upstream"].reshape(1, B * D))
    c.d_dnn = np.zeros((B, c.ld), np.float32)
    c.d_lin = np.ascontiguousarray(g["lin_upstream"][:, 0])
    return c


def _check_golden_grads(g, got_table, got_lin):
    """The reference's own table gradients at the table-gradient bar; row 0 is the point of the golden."""
    for pre, got in (("", got_table), ("lin_", got_lin)):
        want = g[pre + "dtable"]
        assert np.all(want[0] != 0)
        _, ab, n = vr.pool_grad(g["ids"], None, g[pre + "table"], "max", g[pre + "upstream"])
        err, bar = np.abs(got - want.astype(np.float64)), (n[:, None] + 2) * EPS * ab
        print("golden %stable: worst share of the bar %.3f, row 0 alone %.3f" % (
            pre, float((err / np.maximum(bar, 1e-300)).max()), float((err[0] / bar[0]).max())))
        assert np.all(err <= bar) and np.all(got[n == 0] == 0)


def test_reference_golden_with_empty_max_sequences():
    dev = _dev()
    g = load_golden("varlen_pool_max_empty")
    c = _golden_case(g)
    d = Device(c, dev)
    emb, dnn, lin = d.forward()
    np.testing.assert_array_equal(emb[0].reshape(c.B, c.D), g["pooled"])
    np.testing.assert_array_equal(dnn, g["pooled"])
    np.testing.assert_array_equal(lin, g["lin_pooled"][:, 0])
    _check_argpos(c, d.argpos.cpu().numpy())
    assert int(d.flag.item()) == 0
    grads = d.backward()
    _check_golden_grads(g, grads[0], grads[1])
    _check_backward(c, grads)


# ------------------------------------------------------------------------------------------------- models
def close(got, want, rtol, atol, msg=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


@pytest.mark.parametrize("name", ["varlen_model_xdeepfm", "varlen_model_attn"])
def test_model_vs_reference_golden(name):
    """The bars are those of tests/test_gpu_parity.py::test_model_vs_reference_golden."""
    dev = _dev()
    g = load_golden(name)
    model = vr.golden_model(g, dev)
    for k, v in model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), g["init:" + k], err_msg="init " + k)
    model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
    B = int(g["B"])
    X, y = T(g["X"]).to(dev), T(g["y"]).to(dev)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    model.train()
    close(model.linear_model(X[:B]), g["lin_logit"], rtol=2e-5, atol=1e-6, msg="Linear called directly")
    y_pred = model(X[:B])
    close(y_pred, g["y_pred"], rtol=2e-5, atol=1e-6, msg="y_pred")
    loss = torch.nn.functional.binary_cross_entropy(y_pred.squeeze(), y[:B].squeeze(), reduction="sum")
    reg = model.get_regularization_loss()
    assert abs(loss.item() - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    assert abs(reg.item() - float(g["reg"])) <= 1e-5 * abs(float(g["reg"]))
    model.optim.zero_grad()
    (loss + reg).backward()
    for k, p in model.named_parameters():
        want = g["g:" + k]
        close(p.grad, want, rtol=2e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-9, msg=k)
    model.optim.zero_grad()
    losses = []
    for s in range(3):                                  # three Adam steps, as BaseModel.fit does them
        xb, yb = X[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        yp = model(xb).squeeze()
        model.optim.zero_grad()
        l = torch.nn.functional.binary_cross_entropy(yp, yb.squeeze(), reduction="sum")
        tot = l + model.get_regularization_loss() + model.aux_loss
        losses.append([l.item(), tot.item()])
        tot.backward()
        model.optim.step()
    np.testing.assert_allclose(np.array(losses), g["losses3"], rtol=2e-5)
    for k, v in model.state_dict().items():
        close(v, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="after 3 steps: " + k)
    idx = model.feature_index
    Xn = g["X"]
    feed = {n: Xn[:, a:b] for n, (a, b) in idx.items()}
    pred = model.predict(feed, batch_size=B)
    assert pred.dtype == np.float64 and pred.shape == (Xn.shape[0], 1)
    from xdfm_amd import metrics as M
    assert abs(M.log_loss(g["y"], pred) - M.log_loss(g["y"], g["pred_after"])) < 1e-5
    assert abs(M.roc_auc_score(g["y"], pred) - M.roc_auc_score(g["y"], g["pred_after"])) < 1e-5
    # an id outside the table, at a padded position of the length-masked column: IndexError at the end of predict
    bad = Xn.copy()
    a, b = idx["g_sum"]
    bad[4, idx["g_sum_len"][0]] = 1
    bad[4, b - 1] = 6
    with pytest.raises(IndexError, match="vocabulary_size"):
        model.predict({n: bad[:, lo:hi] for n, (lo, hi) in idx.items()}, batch_size=B)
    model.predict(feed, batch_size=B)                   # the flag was cleared


def test_train_step_replayed_from_the_graph_equals_the_eager_twin():
    from xdfm_amd import graphstep
    dev = _dev()
    g = load_golden("varlen_model_xdeepfm")
    X, y = T(g["X"]).to(dev), T(g["y"]).to(dev)
    B = int(g["B"])

    def run(use_graph):
        model = vr.golden_model(g, dev)
        model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
        model.compile("adam", "binary_crossentropy", metrics=[])
        model.train()
        step = graphstep.GraphedStep(model)
        step.disabled = not use_graph
        model.__dict__["_graphed_step"] = step
        for s in range(5):
            k = s % 3
            model.train_on_batch(X[k * B:(k + 1) * B], y[k * B:(k + 1) * B])
        torch.cuda.synchronize()
        return model, step

    m_g, st_g = run(True)
    m_e, st_e = run(False)
    assert st_g.replays == 3 and not st_g.disabled and st_e.replays == 0
    for (k, a), (_, b) in zip(m_g.state_dict().items(), m_e.state_dict().items()):
        assert torch.equal(a, b), k
    assert not torch.equal(m_g.state_dict()["embedding_dict.g_max.weight"].cpu(), T(g["s0:embedding_dict.g_max.weight"]))


def test_linear_called_directly_and_input_from_feature_columns():
    dev = _dev()
    g = load_golden("varlen_model_xdeepfm")
    model = vr.golden_model(g, dev)
    model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
    B = int(g["B"])
    X = T(g["X"][:B]).to(dev)
    from deepctr.models.basemodel import Linear
    sparse, varlen, dense = vr.golden_columns(g)
    lin = Linear(sparse + varlen + dense, model.feature_index, device=dev)
    lin.load_state_dict(model.linear_model.state_dict())
    close(lin(X), g["lin_logit"], rtol=2e-5, atol=1e-6, msg="linear logit")
    embs, dense_vals = model.input_from_feature_columns(X, model.dnn_feature_columns, model.embedding_dict)
    assert len(embs) == 6 and all(tuple(e.shape) == (B, 1, 4) for e in embs) and len(dense_vals) == 2
    emb_fm, dnn_in, _ = model.fused_inputs(X)
    for j, e in enumerate(embs):
        assert torch.equal(e.reshape(B, 4), emb_fm[j].reshape(B, 4)) and torch.equal(e.reshape(B, 4), dnn_in[:, 4 * j:4 * j + 4])
    for f, fc in enumerate(varlen):                     # the pooled rows against the restatement, through the public interface
        a, b = model.feature_index[fc.name]
        lengths = None if fc.length_name is None else g["X"][:B, model.feature_index[fc.length_name][0]]
        want, mag, _ = vr.pool(g["X"][:B, a:b], lengths, g["s0:embedding_dict.%s.weight" % fc.name], fc.combiner)
        got = embs[3 + f].detach().reshape(B, 4).cpu().numpy()
        if fc.combiner == "max":
            np.testing.assert_array_equal(got, want)
        else:
            assert np.all(np.abs(got - want) <= (fc.maxlen + 2) * EPS * mag)


def test_autograd_sends_the_gradient_of_empty_max_sequences_to_row_0():
    """ops.VarLenPool on the reference's golden with empty max sequences: the pooled rows exactly, and .grad of the table
    and of the linear table -- row 0 among them -- at the table-gradient bar."""
    from xdfm_amd import ops
    dev = _dev()
    g = load_golden("varlen_pool_max_empty")
    B, Tn = g["ids"].shape
    V, D = g["table"].shape
    plan = ops.VarLenPlan([0], [Tn], [None], ["max"], [V], D)
    table = T(g["table"]).to(dev).requires_grad_(True)
    lin_table = T(g["lin_table"]).to(dev).requires_grad_(True)
    emb, dnn, lin = ops.VarLenPool.apply(T(g["ids"]).to(dev), torch.zeros((1, B * D), device=dev), torch.zeros((B, D), device=dev),
                                         torch.zeros((B, 1), device=dev), plan, 1, table, lin_table)
    assert not plan.check_ids(dev)
    np.testing.assert_array_equal(emb.detach().view(B, D).cpu().numpy(), g["pooled"])
    np.testing.assert_array_equal(dnn.detach().cpu().numpy(), g["pooled"])
    np.testing.assert_array_equal(lin.detach().cpu().numpy(), g["lin_pooled"])
    ((emb.view(B, D) * T(g["upstream"]).to(dev)).sum() + (lin * T(g["lin_upstream"]).to(dev)).sum()).backward()
    _check_golden_grads(g, table.grad.cpu().numpy(), lin_table.grad.cpu().numpy())
