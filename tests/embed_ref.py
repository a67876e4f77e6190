"""What the K1 / K2 tests (csrc/embed.hip) share: a plain reference of the gather, the float64 sum and a bit-exact model of
the scatter's documented arithmetic, a literal simulation of its windows and chains (checked against the model on the
CPU), the case tables of tests/test_gpu_embed_abi.py with the facts each case exists for, and `drive_gather` /
`drive_scatter`: the C calls through ctypes as include/xdfm.h documents them, with guarded buffers of the test's own.
numpy only; torch is imported inside the drivers.  Checked by tests/test_embed_reference.py."""
import itertools
import math

import numpy as np

SC_ROWS, SC_W = 4096, 8                     # csrc/embed.hip: examples per chunk (one launch), list positions per window
GUARD = 64                                  # sentinel elements before and after every guarded buffer
SENTINEL = np.float32(-24681.357)           # never a result of these inputs; not a NaN, so bits compare as values
MARK_SENTINEL = 0xA5
F32, F64, I64 = np.float32, np.float64, np.int64


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def ids_of(xcol, V):
    """(ids clamped to [0, V), whether any was outside): truncation toward zero, as Tensor.long() on the fp32 column."""
    raw = np.trunc(np.asarray(xcol, dtype=F64)).astype(I64)
    return np.clip(raw, 0, V - 1), bool(((raw < 0) | (raw >= V)).any())


# ------------------------------------------------------------------------------------------------------- K1: gather
def gather_reference(X, tables, lin_tables, cols, vocab, dense_cols, dense_w, D):
    """emb [B, m, D] and dnn [B, m*D + nd] (copies: fp32, compared by bits), lin64 [B] = float64 sum of the linear rows in
    field order, then of the dense products; lin_abs [B] = the sum of their magnitudes; flag = 1 when an id was clamped.
    lin_tables / dense_w may be None (that part of lin64 is absent)."""
    B, m = X.shape[0], len(tables)
    nd = 0 if dense_cols is None else len(dense_cols)
    emb = np.empty((B, m, D), dtype=F32)
    lin64, lin_abs, flag = np.zeros(B), np.zeros(B), 0
    for j in range(m):
        ids, bad = ids_of(X[:, cols[j]], vocab[j])
        flag |= int(bad)
        emb[:, j] = tables[j][ids]
        if lin_tables is not None:
            l = lin_tables[j][ids].astype(F64)
            lin64 += l
            lin_abs += np.abs(l)
    dense = X[:, list(dense_cols)] if nd else np.zeros((B, 0), dtype=F32)
    dnn = np.concatenate([emb.reshape(B, m * D), dense], axis=1)
    if nd and dense_w is not None:
        p = dense.astype(F64) * np.asarray(dense_w, dtype=F64)
        lin64 += p.sum(1)
        lin_abs += np.abs(p).sum(1)
    return emb, dnn, lin64, lin_abs, flag


#  name: shape, then what the case claims to reach (asserted from the host code's formulas by gather_facts)
GATHER_CASES = {
    "G1": dict(B=37, m=33, D=8, nd=2, claims=dict(wide=True, partial=True, EB=16, vec=4)),
    "G2": dict(B=19, m=40, D=12, nd=0, no_lin=True, claims=dict(wide=True, partial=True, vec=4, DV=3, EB=16)),
    "G3": dict(B=21, m=32, D=4, nd=1, claims=dict(wide=False, m=32, partial=True, EB=16)),
    "G4": dict(B=35, m=4, D=8, nd=40, claims=dict(dense_tail=True, weight_loop=False, partial=True, EB=16)),
    "G5": dict(B=18, m=2, D=4, nd=300, ldx_extra=3, shuffled_cols=True,
               claims=dict(weight_loop=True, dense_tail=True, partial=True, EB=16)),
    "G6": dict(B=3, m=33, D=252, nd=1, claims=dict(EB=1, vec=4, DV=63, wide=True, mD=8316)),
    "G7": dict(B=17, m=3, D=6, nd=2, claims=dict(vec=2, DV=3, partial=True)),
    "G8": dict(B=9, m=1, D=1, nd=0, claims=dict(vec=1, DV=1, partial=True)),
    "G9": dict(B=23, m=5, D=10, nd=3, ld=dict(gap_fields=2, pad=4), claims=dict(vec=2, DV=5, partial=True)),
    "G10": dict(B=16, m=6, D=16, nd=2, special_ids="all", claims=dict(EB=16, partial=False, vec=4)),
    "G10b": dict(B=16, m=6, D=16, nd=2, special_ids="benign", claims=dict(EB=16, partial=False, vec=4)),
}
#  ids of G10 relative to the field's vocabulary V: (value, offset from V?, out of range)
SPECIAL_IDS = [(-3.0, False, True), (-0.5, False, False), (0.9, False, False), (-0.25, True, False), (0.0, True, True),
               (7.0, True, True), (2.7, False, False)]


def special_id_values(V, which):
    return [F32(v + V if rel else v) for v, rel, bad in SPECIAL_IDS if which == "all" or not bad]


def gather_facts(case):
    """What xdfm_embed_gather_fwd_ld derives from the shape: examples per block, vector width, ... (csrc/embed.hip)."""
    B, m, D, nd = case["B"], case["m"], case["D"], case["nd"]
    EB = max(1, min(16, 8192 // (m * D)))
    vec = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    return dict(EB=EB, vec=vec, DV=D // vec, wide=m > 32, m=m, mD=m * D, partial=B % EB != 0, dense_tail=min(B, EB) * nd > 512,
                weight_loop=nd > 256, blocks=-(-B // EB))


def gather_inputs(name):
    """The host arrays of a gather case: X [B, ldx], tables, lins, cols, vocab, dense_cols, dense_w and the dnn layout."""
    c = GATHER_CASES[name]
    B, m, D, nd = c["B"], c["m"], c["D"], c["nd"]
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    ldx = m + nd + c.get("ldx_extra", 0)
    if c.get("shuffled_cols"):
        where = rng.permutation(ldx)
        cols, dense_cols = where[:m], where[m:m + nd]
        # field and dense columns interleaved, neither list ascending
        assert (np.diff(cols) < 0).any() or m == 1
        assert (np.diff(dense_cols) < 0).any() and cols.min() < dense_cols.max() and dense_cols.min() < cols.max()
    else:
        cols, dense_cols = np.arange(m), np.arange(m, m + nd)
    special = c.get("special_ids")
    vocab = [3 + (5 * j) % 9 for j in range(m)] if special else [1 + (7 * j + B) % 11 for j in range(m)]
    X = np.full((B, ldx), 777.25, dtype=F32)                     # columns nobody names hold a far-out id
    for j, V in enumerate(vocab):
        ids = rng.integers(0, V, size=B).astype(F32)
        ids[0], ids[B - 1] = 0, V - 1
        if special:
            vals = special_id_values(V, special)
            for r in range(1, B - 1):
                if (r + j) % 2 == 0:
                    ids[r] = vals[(r // 2 + j) % len(vals)]
        X[:, cols[j]] = ids
    if nd:
        X[:, dense_cols] = rng.standard_normal((B, nd)).astype(F32)
    tables = [rng.standard_normal((V, D)).astype(F32) for V in vocab]
    lins = None if c.get("no_lin") else [rng.standard_normal(V).astype(F32) for V in vocab]
    dense_w = rng.standard_normal(nd).astype(F32) if nd else None
    out = dict(name=name, B=B, m=m, D=D, nd=nd, ldx=ldx, X=X, cols=cols.astype(np.int32), dense_cols=dense_cols.astype(np.int32),
               vocab=vocab, tables=tables, lins=lins, dense_w=dense_w, ld=None)
    if c.get("ld"):
        off = m * D + c["ld"]["gap_fields"] * D
        out["ld"] = dict(dense_off=off, ld_dnn=off + nd + c["ld"]["pad"])
    return out


def gather_expected(inp, with_lin=True):
    return gather_reference(inp["X"], inp["tables"], inp["lins"] if with_lin else None, inp["cols"], inp["vocab"],
                            inp["dense_cols"] if inp["nd"] else None, inp["dense_w"], inp["D"])


# ------------------------------------------------------------------------------------------------------ K2: scatter
def scale_exp(amax):
    """sc_scale_exp: s with amax * 2^s in [2^37, 2^38), from the biased exponent (0 counts as 1)."""
    E = (np.ascontiguousarray(amax, dtype=F32).view(np.uint32) >> 23) & 0xff
    return (37 - (np.maximum(E, 1).astype(I64) - 127)).astype(np.int32)


def _fix(v, s):
    """The addends on the grid 2^-s: rint(v * 2^s), ties to even, as int64 (exact: |v * 2^s| < 2^38)."""
    return np.rint(np.ldexp(v.astype(F64), s)).astype(I64)


def _unfix(total, s):
    """fp32(total * 2^-s): total < 2^51 is exact in float64, the product is a scaling, one rounding to fp32."""
    return np.ldexp(total.astype(F64), -s.astype(np.int32)).astype(F32)


def _reduce_multiset(ids, vals):
    """One chunk of one stream: (ids that occur, r [runs, W] fp32) -- per id and component the exact sum of the addends on
    the grid of the run's largest magnitude, rounded once.  A function of the multiset of rows of an id."""
    order = np.argsort(ids, kind="stable")
    sid, v = ids[order], vals[order]
    starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
    lens = np.diff(np.r_[starts, len(sid)])
    s = scale_exp(np.maximum.reduceat(np.abs(v), starts, axis=0))              # [runs, W]
    total = np.add.reduceat(_fix(v, np.repeat(s, lens, axis=0)), starts, axis=0)
    return sid[starts], _unfix(total, s)


def _exact_piece(seg):
    s = scale_exp(np.abs(seg).max(0))
    return _unfix(_fix(seg, s[None, :]).sum(0), s)


def _reduce_windows(ids, vals, rng=None):
    """The same chunk as the kernel walks it: the grouped list (equal ids adjacent; the runs in ascending id order, or in
    `rng`'s order with the rows of a run shuffled: the hash decides on the GPU) cut into windows of 8 positions.  Runs
    inside a window are finished there; the open pieces of a run that crosses windows are elements 2w (continues from the
    left) and 2w + 1 (goes on to the right) of chains e -> N[e], with 2w -> 2w + 1 in a window that one run passes through
    (`both`); pointer jumping gives every element the maximum of its chain and its head, the pieces are summed on the
    grid of that maximum, a second jumping adds them up, and the head writes."""
    n, W = vals.shape
    uniq, inv = np.unique(ids, return_inverse=True)
    if rng is None:
        order = np.argsort(inv, kind="stable")
    else:
        order = np.lexsort((rng.random(n), rng.permutation(len(uniq))[inv]))
    gid, v = ids[order], vals[order]
    nwin = -(-n // SC_W)
    E = 2 * nwin
    M = np.zeros((E, W), dtype=F32)
    N, H = np.full(E, -1), np.arange(E)
    pieces, owners, out = {}, [], {}
    for w in range(nwin):
        a, b = SC_W * w, min(n, SC_W * w + SC_W)
        idw, full = gid[a:b], b - a == SC_W
        contL = a > 0 and gid[a - 1] == idw[0]
        contR = full and b < n and gid[b] == idw[-1]
        single = full and idw[0] == idw[-1]
        both = contL and contR and single
        q = 0
        while q < b - a:
            e = q
            while e + 1 < b - a and idw[e + 1] == idw[q]:
                e += 1
            pieceL, pieceR = contL and idw[q] == idw[0], contR and idw[q] == idw[-1]
            seg = v[a + q:a + e + 1]
            if not pieceL and not pieceR:
                out[int(idw[q])] = _exact_piece(seg)
            else:
                el = 2 * w + (0 if pieceL else 1)
                M[el], pieces[el] = np.abs(seg).max(0), seg
            q = e + 1
        N[2 * w] = 2 * w + 1 if both else -1
        N[2 * w + 1] = 2 * w + 2 if contR else -1
        H[2 * w] = 2 * w - 1 if contL else 2 * w
        H[2 * w + 1] = 2 * w if both else 2 * w + 1
        if contR and not (contL and single):
            owners.append((2 * w + 1, int(idw[-1])))
    chain = N.copy()
    while (N >= 0).any() or (H[H] != H).any():                                # suffix maxima and heads
        has = N >= 0
        M = np.maximum(M, np.where(has[:, None], M[np.maximum(N, 0)], F32(0)))
        N, H = np.where(has, N[np.maximum(N, 0)], -1), H[H]
    s = scale_exp(M[H])                       # [E, W]: the grid of the run, at every piece
    S = np.zeros((E, W), dtype=I64)
    for el, seg in pieces.items():
        S[el] = _fix(seg, s[el][None, :]).sum(0)
    N = chain
    while (N >= 0).any():                                                     # suffix sums: integers, exact
        has = N >= 0
        S = S + np.where(has[:, None], S[np.maximum(N, 0)], 0)
        N = np.where(has, N[np.maximum(N, 0)], -1)
    for el, rid in owners:
        assert rid not in out
        out[rid] = _unfix(S[el], s[el])
    keys = np.array(sorted(out), dtype=I64)
    return keys, np.stack([out[int(k)] for k in keys])


def _rows(case):
    """g [B, m, D] = fp32(d_emb + d_dnn): one fp32 add, as autograd's accumulation of the two uses of the embedding."""
    B, m, D = case["B"], case["m"], case["D"]
    g = np.zeros((B, m, D), dtype=F32)
    if case["d_emb"] is not None:
        g = g + case["d_emb"]
    if case["d_dnn"] is not None:
        g = (g + case["d_dnn"][:, :m * D].reshape(B, m, D)).astype(F32)
    return g


def streams(case):
    """Everything the call reduces, as (ids [B], addends [B, W] fp32, first element in d_flat, W): element
    first + id * W + c receives the addends of the examples with that id.  Tables, linear tables, then the dense weights
    (one destination each: id 0; the addends are the fp32 products x * d_lin)."""
    m, D, nd, X = case["m"], case["D"], case["nd"], case["X"]
    ids = [ids_of(X[:, case["cols"][j]], case["vocab"][j])[0] for j in range(m)]
    out = []
    if case["tab_off"] is not None:
        g = _rows(case)
        out += [(ids[j], g[:, j, :], case["tab_off"][j], D) for j in range(m)]
    if case["d_lin"] is not None:
        dl = np.ascontiguousarray(case["d_lin"][:, 0])
        if case["lin_off"] is not None:
            out += [(ids[j], dl[:, None], case["lin_off"][j], 1) for j in range(m)]
        if nd and case["dw_off"] is not None:
            zero = np.zeros(case["B"], dtype=I64)
            out += [(zero, (X[:, case["dense_cols"][k]] * dl).astype(F32)[:, None], case["dw_off"] + k, 1) for k in range(nd)]
    return out


def _dest(ids, first, W):
    return first + ids[:, None] * W + np.arange(W)[None, :]


def scatter_exact(case):
    """float64: prefill + the true sum of the fp32 addends, per element of d_flat.  Also (for the bound) the number of
    addends and their largest magnitude per element."""
    exact = case["prefill"].astype(F64)
    cnt, amax = np.zeros(exact.size), np.zeros(exact.size)
    for ids, vals, first, W in streams(case):
        d = _dest(ids, first, W)
        np.add.at(exact, d, vals.astype(F64))
        np.add.at(cnt, d, 1.0)
        np.maximum.at(amax, d, np.abs(vals).astype(F64))
    return exact, cnt, amax


def scatter_bound(case):
    """nchunk * (0.5 + 1e-3) * ulp32(max(|exact|, n * amax)) + n * amax * 2^-37 per element: the final rounding of every
    chunk's sum plus the grid of the addends (tests/test_gpu_parity.py); with a prefill, half an ulp of the result for the
    add to what the buffer held."""
    exact, cnt, amax = scatter_exact(case)
    nchunk = -(-case["B"] // SC_ROWS)
    ulp = np.spacing(np.maximum(np.abs(exact), cnt * amax).astype(F32)).astype(F64)
    tol = nchunk * (0.5 + 1e-3) * ulp + cnt * amax * 2.0 ** -37
    if case["has_prefill"]:
        tol = tol + 0.5 * np.spacing(np.abs(exact).astype(F32)).astype(F64)
    return exact, tol


def scatter_model(case, windows=False, rng=None):
    """(d_flat [total] fp32, marks [ceil(total / 4)] bytes) the call must leave, to the bit: chunks of 4096 examples in
    ascending order; per chunk, id and component r = fp32(sum of rint(g * 2^s) * 2^-s) with s from the largest |g| of
    the id's rows in the chunk, then flat = fp32(flat + r).  windows=True computes every r as the kernel's windows and
    chains do (_reduce_windows): the same bits, or the kernel's scheme is no function of the multiset."""
    flat = case["prefill"].copy()
    marks = np.zeros((flat.size + 3) // 4, dtype=np.uint8)
    for b0 in range(0, case["B"], SC_ROWS):
        for ids, vals, first, W in streams(case):
            i, v = ids[b0:b0 + SC_ROWS], vals[b0:b0 + SC_ROWS]
            keys, r = _reduce_windows(i, v, rng) if windows else _reduce_multiset(i, v)
            d = _dest(keys, first, W)
            flat[d] = flat[d] + r
            marks[d >> 2] = 1
    return flat, marks


def scatter_in_example_order(case):
    """fp32 adds in example order (np.add.at), as the reference's CPU embedding_dense_backward."""
    flat = case["prefill"].copy()
    for ids, vals, first, W in streams(case):
        np.add.at(flat, _dest(ids, first, W), vals)
    return flat


def touched(case):
    t = np.zeros(case["prefill"].size, dtype=bool)
    for ids, vals, first, W in streams(case):
        t[_dest(ids, first, W)] = True
    return t


def permuted(case, p):
    out = dict(case)
    for k in ("X", "d_emb", "d_dnn", "d_lin"):
        out[k] = None if case[k] is None else np.ascontiguousarray(case[k][p])
    return out


def _lcm(a, b):
    return a * b // math.gcd(a, b)


S1_RUNS = (1, 7, 8, 9, 15, 16, 17, 24, 25)
G10_AS_SCATTER = "ids of G10"


def _s(B, vocab, D, **kw):
    return dict(B=B, vocab=list(vocab), D=D, **kw)


#  name: the call (see scatter_inputs for the keys), `facts` = what the case claims about its run layout (asserted by
#  tests/test_embed_reference.py from the ids alone)
SCATTER_CASES = {}
for _c in S1_RUNS:
    _B = 600 // _lcm(8, _c) * _lcm(8, _c)
    SCATTER_CASES["S1-c%d" % _c] = _s(_B, [_B // _c], 8, ids=("uniform", _c), marks=True)
SCATTER_CASES.update({
    "S2": _s(4096, [1, 2, 3], 4, ids=("counts", [[4096], [4095, 1], [8, 4080, 8]]), marks=True),
    "S4-B4097": _s(4097, [5, 700], 8, marks=True),
    "S4-B4104": _s(4104, [5, 700], 8, marks=True),
    "S5": _s(300, [3, 11, 50], 16, nd=2, prefill=True, marks=True),
    "S6": _s(300, [5, 9, 30], 8, off_mod=[1, 2, 3], marks=True),
    "S7-emb": _s(300, [5, 9, 30], 8, misalign="emb"),
    "S7-flat": _s(300, [5, 9, 30], 8, misalign="flat"),
    "S8-D6": _s(260, [4, 9, 40, 1], 6, marks=True),
    "S8-D20": _s(260, [4, 9, 40, 1], 20, marks=True),
    "S9": _s(200, [4, 9, 40], 8, nd=2, ldx_extra=3, ld_dnn_extra=5, ld_lin=3, shuffled_cols=True, marks=True),
    "S10": _s(64, [5, 3], 4, ids=G10_AS_SCATTER, marks=True),
    "S11-emb": _s(128, [4, 9, 40], 8, nd=2, srcs="e", lin=False, marks=True),
    "S11-dnn": _s(128, [4, 9, 40], 8, nd=2, srcs="d", lin=False, marks=True),
    "S11-dense-only": _s(128, [4, 9, 40], 8, nd=2, srcs="l", tab=False, lin=False, marks=True),
    "S11-lin-only": _s(128, [4, 9, 40], 8, nd=2, srcs="l", tab=False, marks=True),
})
for _B in (1, 5, 7, 8, 9):
    SCATTER_CASES["S3-B%d" % _B] = _s(_B, [3], 4, marks=True)
del _c, _B


def scatter_inputs(name):
    """The host arrays and the d_flat layout of a scatter case.  Keys of SCATTER_CASES[name]:
      ids          ("uniform", c): every id exactly c times, shuffled; ("counts", per field): id i that many times, shuffled;
                   G10_AS_SCATTER: G10's fractional, negative and far-out ids; default: V * u^3 (a few hot rows)
      srcs         which of d_emb_fm / d_dnn_in / d_lin are handed over ("edl"); tab / lin: False passes NULL offsets
      prefill      the tables, linear tables and dense weights of d_flat start from random values (else zeros)
      off_mod      table j starts at an element offset = off_mod[j] (mod 4); default 0
      misalign     "emb": d_emb_fm one float past a 16-byte boundary; "flat": d_flat
      ldx_extra, ld_dnn_extra, ld_lin, shuffled_cols      pitches beyond the dense ones, permuted id / dense columns
    The gaps between the tables of d_flat hold SENTINEL, in the prefill and so in scatter_model's result."""
    c = SCATTER_CASES[name]
    B, vocab, D, nd = c["B"], c["vocab"], c["D"], c.get("nd", 0)
    m = len(vocab)
    srcs = c.get("srcs", "edl")
    rng = np.random.default_rng(2000 + sum(map(ord, name)))
    ldx = m + nd + c.get("ldx_extra", 0)
    if c.get("shuffled_cols"):
        where = rng.permutation(ldx)
        cols, dense_cols = where[:m], where[m:m + nd]
    else:
        cols, dense_cols = np.arange(m), np.arange(m, m + nd)
    X = np.full((B, ldx), 777.25, dtype=F32)
    mode = c.get("ids")
    for j, V in enumerate(vocab):
        if mode is None:
            ids = np.floor(V * rng.random(B) ** 3)
        elif mode == G10_AS_SCATTER:
            vals = special_id_values(V, "all")
            ids = np.array([vals[(r + j) % len(vals)] if r % 3 else rng.integers(0, V) for r in range(B)])
        else:
            counts = [mode[1]] * V if mode[0] == "uniform" else mode[1][j]
            assert len(counts) == V and sum(counts) == B
            ids = rng.permutation(np.repeat(np.arange(V), counts))
        X[:, cols[j]] = ids.astype(F32)
    if nd:
        X[:, dense_cols] = rng.random((B, nd)).astype(F32)
    mag = 10.0 ** rng.integers(-6, 2, size=(B, 1, 1))                       # rows of very different magnitudes
    ld_dnn = m * D + nd + c.get("ld_dnn_extra", 0)
    ld_lin = c.get("ld_lin", 1)
    d_emb = (rng.standard_normal((B, m, D)) * mag).astype(F32) if "e" in srcs else None
    d_dnn = (rng.standard_normal((B, ld_dnn)) * mag[:, 0]).astype(F32) if "d" in srcs else None
    d_lin = (rng.standard_normal((B, ld_lin)) * mag[:, 0]).astype(F32) if "l" in srcs else None
    # d_flat: tables (at their residues mod 4), linear tables, dense weights; everything else is a gap
    off_mod = c.get("off_mod", [0] * m)
    pos, tab_off, lin_off = 0, [], []
    for j, V in enumerate(vocab):
        pos = (pos + 3) // 4 * 4 + off_mod[j]
        tab_off.append(pos)
        pos += V * D
    for V in vocab:
        pos = (pos + 3) // 4 * 4
        lin_off.append(pos)
        pos += V
    dw_off = (pos + 3) // 4 * 4
    total = dw_off + max(nd, 1) + 3
    prefill = np.full(total, SENTINEL, dtype=F32)
    fill = (lambda n: (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, size=n)).astype(F32)) if c.get("prefill") else \
        (lambda n: np.zeros(n, dtype=F32))
    for j, V in enumerate(vocab):
        prefill[tab_off[j]:tab_off[j] + V * D] = fill(V * D)
        prefill[lin_off[j]:lin_off[j] + V] = fill(V)
    prefill[dw_off:dw_off + nd] = fill(nd)
    return dict(name=name, B=B, m=m, D=D, nd=nd, vocab=vocab, ldx=ldx, X=X, cols=cols.astype(np.int32),
                dense_cols=dense_cols.astype(np.int32), d_emb=d_emb, d_dnn=d_dnn, d_lin=d_lin, ld_dnn=ld_dnn, ld_lin=ld_lin,
                tab_off=tab_off if c.get("tab", True) else None, lin_off=lin_off if c.get("lin", True) else None,
                dw_off=dw_off if nd else None, prefill=prefill, has_prefill=bool(c.get("prefill")), marks=bool(c.get("marks")),
                misalign=c.get("misalign"), dense_pitches=ld_dnn == m * D + nd and ld_lin == 1)


# ----------------------------------------------------------------------------------------- run layouts (structure facts)
def run_lengths(case, j, b0=0):
    """Sorted run lengths of field j in the chunk that starts at example b0: how often every id occurs."""
    ids = ids_of(case["X"][b0:b0 + SC_ROWS, case["cols"][j]], case["vocab"][j])[0]
    return sorted(np.bincount(ids)[np.bincount(ids) > 0].tolist())


def layout_facts(lengths):
    """What a grouped list with runs of these lengths, in this order, makes the windows do.  For equal lengths the order of
    the runs does not matter: run k covers [k c, (k + 1) c) whichever id the hash put there."""
    edges = np.r_[0, np.cumsum(lengths)]
    n = int(edges[-1])
    f = dict(starts_mod8=set(), closed_on_edge=0, open_ends_on_edge=0, both=0, both_then_one=0, spans={}, longest_chain=0,
             closed_beside_open=0, windows=-(-n // SC_W), last_window=n - (n - 1) // SC_W * SC_W)
    open_windows, closed_windows = set(), set()
    for a, b in zip(edges[:-1], edges[1:]):
        a, b = int(a), int(b)
        wa, wb = a // SC_W, (b - 1) // SC_W
        f["starts_mod8"].add(a % SC_W)
        span = wb - wa + 1
        if span == 1:
            closed_windows.add(wa)
            f["closed_on_edge"] += b % SC_W == 0
            continue
        f["spans"][span] = f["spans"].get(span, 0) + 1
        f["longest_chain"] = max(f["longest_chain"], span)
        f["open_ends_on_edge"] += b % SC_W == 0
        inner = [w for w in range(wa, wb + 1) if a < w * SC_W and (w + 1) * SC_W < b]   # one run from the left, on to the right
        f["both"] += len(inner)
        f["both_then_one"] += bool(inner) and inner[-1] == wb - 1 and b - wb * SC_W == 1
        open_windows.update(range(wa, wb + 1))
    f["closed_beside_open"] = len(open_windows & closed_windows)                      # a finished run and an open piece share a window
    only_closed = closed_windows - open_windows
    f["closed_next_to_open"] = sum(1 for w in only_closed if w - 1 in open_windows or w + 1 in open_windows)
    return f


def layouts(lengths):
    """The facts of every order of the runs (equal lengths: one order; few runs: all orders)."""
    if len(set(lengths)) == 1:
        return [layout_facts(lengths)]
    assert len(lengths) <= 4
    return [layout_facts(p) for p in sorted(set(itertools.permutations(lengths)))]


# ---------------------------------------------------------------------------------------------------------- drivers
class _Guarded:
    """n elements between two bands of GUARD sentinels (+ `shift` more in front: the payload then starts `shift` elements
    past the 16-byte boundary a band of 64 floats ends on)."""

    def __init__(self, payload, dev, shift=0):
        import torch
        payload = np.ascontiguousarray(payload)
        self.a, self.n = GUARD + shift, payload.size
        fill = float(SENTINEL) if payload.dtype == F32 else MARK_SENTINEL if payload.dtype == np.uint8 else -24681
        self.fill = np.full(1, fill, dtype=payload.dtype)
        self.buf = torch.full((self.a + self.n + GUARD,), fill, dtype=torch.from_numpy(payload[:0]).dtype, device=dev)
        self.t = self.buf[self.a:self.a + self.n]
        self.t.copy_(torch.from_numpy(payload.reshape(-1)))
        assert self.buf.data_ptr() % 16 == 0

    def get(self):
        return self.t.cpu().numpy()

    def untouched(self):
        whole = self.buf.cpu().numpy()
        bands = np.ascontiguousarray(np.r_[whole[:self.a], whole[self.a + self.n:]])
        return bool((bands.view(np.uint8) == np.repeat(self.fill, bands.size).view(np.uint8)).all())


def _up(a, dev, shift=0):
    """A host array on the device (None stays None), `shift` elements past an allocation's start."""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + shift, dtype=torch.from_numpy(a.reshape(-1)[:0]).dtype, device=dev)
    buf[shift:].copy_(torch.from_numpy(a.reshape(-1)))
    return buf[shift:]


def _P(t):
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    import ctypes
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def drive_gather(lib, dev, inp, null=(), override=None):
    """xdfm_embed_gather_fwd (or _ld where the case has a dnn layout of its own) on guarded outputs.  null: names among
    "lin_tables", "dnn_in", "lin_out", "err_flag" (and, for the argument checks, "dense_cols", "dense_w") handed over as
    NULL.  override: B, m, D or ldx as the call states them (argument checks only: the buffers keep the case's sizes).  Returns dict(rc, emb [B, m, D], dnn_wide
    [B, ld_dnn] (SENTINEL where nothing may be written), lin [B], flag, untouched = guard bands intact); an output
    that was not requested is None."""
    import torch
    B, m, D, nd = inp["B"], inp["m"], inp["D"], inp["nd"]
    ld = inp["ld"] or dict(dense_off=m * D, ld_dnn=m * D + nd)
    X = _up(inp["X"], dev)
    tabs = [_up(t, dev) for t in inp["tables"]]
    lins = None if inp["lins"] is None or "lin_tables" in null else [_up(t, dev) for t in inp["lins"]]
    tp = torch.tensor([t.data_ptr() for t in tabs], dtype=torch.int64, device=dev)
    lp = None if lins is None else torch.tensor([t.data_ptr() for t in lins], dtype=torch.int64, device=dev)
    cols, vocab = _up(inp["cols"], dev), _up(np.asarray(inp["vocab"], dtype=np.int32), dev)
    dcols, dw = (_up(inp["dense_cols"], dev), _up(inp["dense_w"], dev)) if nd else (None, None)
    dcols, dw = None if "dense_cols" in null else dcols, None if "dense_w" in null else dw
    o = {**dict(B=B, m=m, D=D, ldx=inp["ldx"]), **(override or {})}
    emb = _Guarded(np.full(m * B * D, SENTINEL, dtype=F32), dev)
    dnn = None if "dnn_in" in null else _Guarded(np.full(B * ld["ld_dnn"], SENTINEL, dtype=F32), dev)
    lin = None if "lin_out" in null else _Guarded(np.full(B, SENTINEL, dtype=F32), dev)
    flag = None if "err_flag" in null else _Guarded(np.zeros(1, dtype=np.int32), dev)
    g = lambda b: None if b is None else b.t
    if inp["ld"] is None:
        rc = lib.xdfm_embed_gather_fwd(_P(X), o["ldx"], o["B"], _P(tp), _P(lp), _P(cols), _P(vocab), o["m"], o["D"], _P(dcols), _P(dw), nd,
                                       _P(emb.t), _P(g(dnn)), _P(g(lin)), _P(g(flag)), _stream())
    else:
        rc = lib.xdfm_embed_gather_fwd_ld(_P(X), o["ldx"], o["B"], _P(tp), _P(lp), _P(cols), _P(vocab), o["m"], o["D"], _P(dcols), _P(dw), nd,
                                          _P(emb.t), _P(g(dnn)), ld["ld_dnn"], ld["dense_off"], _P(g(lin)), _P(g(flag)), _stream())
    torch.cuda.synchronize()
    bufs = [b for b in (emb, dnn, lin, flag) if b is not None]
    return dict(rc=rc, emb=emb.get().reshape(m, B, D).transpose(1, 0, 2), dnn_wide=None if dnn is None else dnn.get().reshape(B, ld["ld_dnn"]),
                lin=None if lin is None else lin.get(), flag=None if flag is None else int(flag.get()[0]),
                untouched=all(b.untouched() for b in bufs), layout=ld)


def drive_scatter(lib, dev, case, marked=True, null=(), ld_dnn=None, force_marks=False):
    """xdfm_embed_scatter_bwd_marked (marked=False: xdfm_embed_scatter_bwd, dense pitches only) on a guarded d_flat that
    starts as the case's prefill, and guarded marks where the case has them.  For the argument checks: null = names among
    "d_flat", "d_emb", "d_dnn" handed over as NULL, ld_dnn as the call states it, force_marks.  Returns dict(rc, flat [total], marks or
    None, untouched = guard bands intact)."""
    import torch
    B, m, D, nd = case["B"], case["m"], case["D"], case["nd"]
    X = _up(case["X"], dev)
    cols, vocab = _up(case["cols"], dev), _up(np.asarray(case["vocab"], dtype=np.int32), dev)
    dcols = _up(case["dense_cols"], dev) if nd else None
    de = None if case["d_emb"] is None else _up(case["d_emb"].transpose(1, 0, 2).reshape(m, B * D), dev,
                                                shift=1 if case["misalign"] == "emb" else 0)
    dd, dl = _up(case["d_dnn"], dev), _up(case["d_lin"], dev)
    flat = _Guarded(case["prefill"], dev, shift=1 if case["misalign"] == "flat" else 0)
    assert (flat.t.data_ptr() % 16 != 0) == (case["misalign"] == "flat") and (de is None or (de.data_ptr() % 16 != 0) == (case["misalign"] == "emb"))
    marks = _Guarded(np.zeros((case["prefill"].size + 3) // 4, dtype=np.uint8), dev) if marked and (case["marks"] or force_marks) else None
    de, dd = None if "d_emb" in null else de, None if "d_dnn" in null else dd
    fp = None if "d_flat" in null else flat.t
    to = None if case["tab_off"] is None else _up(np.asarray(case["tab_off"], dtype=I64), dev)
    lo = None if case["lin_off"] is None else _up(np.asarray(case["lin_off"], dtype=I64), dev)
    dwp = None if case["dw_off"] is None else flat.t[case["dw_off"]:]
    if marked:
        rc = lib.xdfm_embed_scatter_bwd_marked(_P(X), case["ldx"], B, _P(cols), _P(vocab), m, D, _P(dcols), nd, _P(de), _P(dd),
                                               case["ld_dnn"] if ld_dnn is None else ld_dnn, _P(dl), case["ld_lin"], _P(fp), _P(to), _P(lo), _P(dwp),
                                               _P(None if marks is None else marks.t), _stream())
    else:
        assert case["dense_pitches"]
        rc = lib.xdfm_embed_scatter_bwd(_P(X), case["ldx"], B, _P(cols), _P(vocab), m, D, _P(dcols), nd, _P(de), _P(dd), _P(dl),
                                        _P(flat.t), _P(to), _P(lo), _P(dwp), _stream())
    torch.cuda.synchronize()
    return dict(rc=rc, flat=flat.get(), marks=None if marks is None else marks.get(),
                untouched=flat.untouched() and (marks is None or marks.untouched()))
