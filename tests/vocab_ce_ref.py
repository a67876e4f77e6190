"""What the K9 tests (csrc/vocab_ce_x3.hip) share: a float64 reference of the heads' cross-entropy and its gradients, a
plain-Python mirror of xdfm_vocab_ce_plan, the case tables of tests/test_gpu_vocab_ce_abi.py with the plan facts each case
exists for, the input generators, and `drive`: the five C calls through ctypes as include/xdfm.h documents them, with
buffers of the test's own.  Nothing here needs a GPU except `drive`; checked by tests/test_vocab_ce_reference.py."""
import numpy as np
import torch

VX_SB, VX_RG, VX_GRID = 256, 512, 1024      # csrc/vocab_ce_x3.hip: vocabulary rows per stage (= per block of the weights-
#                                             stationary kernel), rows per row group, the workgroup target of the plan
#                                             (= the grid cap of the weights-stationary kernel)
GUARD = 64                                  # sentinel floats before and after every guarded buffer
SENTINEL = -24681.357                       # never a result of these inputs
CHUNK = 512                                 # rows the reference holds at a time: at most CHUNK x V doubles

#  name: (R, K, vocabularies)
LARGE_CASES = {
    "L1": (33, 64, (262700, 300)),
    "L2": (289, 32, (131200, 77, 131500)),
    "L3": (33, 32, (525000,)),
    "L4": (600, 64, (66000, 300, 66100)),
}
#  what each large case exists for: stages per range, ranges per field, stages of each field's last range, 256-row blocks
#  of all fields, the workgroups of the weights-stationary kernel whose second block lies in another field than their
#  first, the workgroups that take a third block, row tiles
LARGE_FACTS = {
    "L1": dict(spr=2, vr=(514, 1), last=(1, 2), n_blk=1029, second_trip=5, third_trip=0, change_field=(3, 4), tiles=2),
    "L2": dict(spr=2, vr=(257, 1, 257), last=(1, 1, 2), n_blk=1028, second_trip=4, third_trip=0, change_field=(0, 1, 2, 3), tiles=10),
    "L3": dict(spr=3, vr=(684,), last=(2,), n_blk=2051, second_trip=1024, third_trip=3, change_field=(), tiles=2),
    "L4": dict(spr=2, vr=(129, 1, 130), last=(2, 2, 1), n_blk=519, second_trip=0, third_trip=0, change_field=(), tiles=19),
}
EDGE_VOCABS = {
    "E1": (257, 33, 1),
    "E5": (1, 31, 32, 255, 256, 257, 511, 513),
}
BENCH_SHAPE = (4096, 64, (100000,) * 26)    # bench.py's criteo_pro heads


def _cd(a, b):
    return -(-a // b)


def plan_mirror(R, K, Vs):
    """xdfm_vocab_ce_plan in plain Python: dict(spr, n_blk, ws_elems, rows_padded, fields = [dict(V, vr, item0, blk0, ws_off,
    items = [(sb0, sb1), ...])]).  `spr` = vocabulary stages per range: every work item of the rows-stationary kernels
    covers spr stages of 256 vocabulary rows, a field's last item what is left."""
    assert K in (32, 64) and R > 0 and all(v > 0 for v in Vs)
    rg = _cd(R, VX_RG)
    rpad = rg * VX_RG
    nsb = [_cd(v, VX_SB) for v in Vs]
    spr = max(1, _cd(sum(nsb) * rg, VX_GRID))
    while sum(_cd(s, spr) for s in nsb) * rg > VX_GRID and spr < max(nsb):
        spr += 1
    fields, n, ws, blk = [], 0, 0, 0
    for v, s in zip(Vs, nsb):
        vr = _cd(s, spr)
        fields.append(dict(V=v, vr=vr, item0=n, blk0=blk, ws_off=ws, items=[(i * spr, min((i + 1) * spr, s)) for i in range(vr)]))
        n += vr
        ws += vr * rpad * K
        blk += s
    return dict(spr=spr, n_blk=blk, ws_elems=ws, rows_padded=rpad, fields=fields)


def plan_facts(mirror, R):
    """The facts of LARGE_FACTS, from a plan (mirror's or the library's in mirror form)."""
    n_blk = mirror["n_blk"]
    grid = min(n_blk, VX_GRID)
    blk0 = [f["blk0"] for f in mirror["fields"]]
    field_of = lambda gb: max(i for i, b in enumerate(blk0) if b <= gb)
    change = tuple(wg for wg in range(grid) if wg + grid < n_blk and field_of(wg + grid) != field_of(wg))
    return dict(spr=mirror["spr"], vr=tuple(f["vr"] for f in mirror["fields"]),
                last=tuple(f["items"][-1][1] - f["items"][-1][0] for f in mirror["fields"]), n_blk=n_blk,
                second_trip=max(0, min(grid, n_blk - grid)), third_trip=max(0, min(grid, n_blk - 2 * grid)),
                change_field=change, tiles=_cd(R, 32))


def library_plan(lib, R, K, Vs):
    """xdfm_vocab_ce_plan itself (host-side, no GPU), in the form of plan_mirror.  `spr` is read off the items: the length
    of the first item of a field that has more than one, else the longest item."""
    import ctypes
    from xdfm_amd import ops
    V = np.asarray(Vs, dtype=np.int32)
    fields = np.zeros(len(Vs), dtype=ops._VCE_FIELD)
    ws, nblk = ctypes.c_long(0), ctypes.c_int(0)
    n = lib.xdfm_vocab_ce_plan(len(Vs), V.ctypes.data, R, K, fields.ctypes.data, None, 0, ctypes.byref(ws), ctypes.byref(nblk))
    assert n > 0
    items = np.zeros(n, dtype=ops._VCE_ITEM)
    assert lib.xdfm_vocab_ce_plan(len(Vs), V.ctypes.data, R, K, fields.ctypes.data, items.ctypes.data, n, ctypes.byref(ws),
                                  ctypes.byref(nblk)) == n
    out, spr = [], None
    for f, fd in enumerate(fields):
        mine = items[int(fd["item0"]):int(fd["item0"]) + int(fd["vr"])]
        assert (mine["field"] == f).all() and (mine["range"] == np.arange(len(mine))).all()
        its = [(int(a), int(b)) for a, b in zip(mine["sb0"], mine["sb1"])]
        if len(its) > 1 and spr is None:
            spr = its[0][1] - its[0][0]
        out.append(dict(V=int(fd["V"]), vr=int(fd["vr"]), item0=int(fd["item0"]), blk0=int(fd["blk0"]), ws_off=int(fd["ws_off"]), items=its))
    assert int((items["field"] >= 0).sum()) == n == sum(f["vr"] for f in out)
    if spr is None:
        spr = max(b - a for f in out for a, b in f["items"])
    return dict(spr=spr, n_blk=int(nblk.value), ws_elems=int(ws.value), rows_padded=int(lib.xdfm_vocab_ce_rows_padded(R)), fields=out)


def reference(h, Ws, bs, tgt, g, n=None):
    """float64 (ce [F, n], dh [n, K], [dW_f], [db_f]) of the first n rows (default: all):
         ce[f][r] = logsumexp_v(h_r . W_f[v] + b_f[v]) - (h_r . W_f[t] + b_f[t]),  t = tgt[f][r] clamped to [0, V_f)
         G_f = g[f][:, None] * (softmax_f - onehot(t));  dh = sum_f G_f W_f;  dW_f = G_f^T h;  db_f = column sums of G_f.
    numpy arrays in, numpy arrays out; torch tensors in (any float type, any device), float64 tensors on that device out.
    One field and at most CHUNK rows at a time."""
    as_np = isinstance(h, np.ndarray)
    t_ = (lambda x: torch.from_numpy(np.ascontiguousarray(x))) if as_np else (lambda x: x)
    h6, g6, tg = t_(h).double(), t_(g).double(), t_(tgt).long()
    R, K = h6.shape
    n = R if n is None else int(n)
    assert 0 <= n <= R
    ce = torch.zeros(len(Ws), n, dtype=torch.float64, device=h6.device)
    dh = torch.zeros(n, K, dtype=torch.float64, device=h6.device)
    dWs, dbs = [], []
    for f, (W, b) in enumerate(zip(Ws, bs)):
        W6, b6 = t_(W).double(), t_(b).double()
        V = W6.shape[0]
        dW, db = torch.zeros_like(W6), torch.zeros_like(b6)
        for r0 in range(0, n, CHUNK):
            r1 = min(n, r0 + CHUNK)
            rows = torch.arange(r1 - r0, device=h6.device)
            t = tg[f, r0:r1].clamp(0, V - 1)
            z = h6[r0:r1] @ W6.t() + b6
            lse = torch.logsumexp(z, dim=1)
            ce[f, r0:r1] = lse - z[rows, t]
            G = torch.exp(z - lse[:, None])
            del z
            G[rows, t] -= 1.0
            G *= g6[f, r0:r1, None]
            dh[r0:r1] += G @ W6
            dW += G.t() @ h6[r0:r1]
            db += G.sum(0)
            del G
        dWs.append(dW)
        dbs.append(db)
    if as_np:
        return ce.numpy(), dh.numpy(), [w.numpy() for w in dWs], [b.numpy() for b in dbs]
    return ce, dh, dWs, dbs


def make_inputs(R, K, Vs, seed):
    """(h, Ws, bs, tgt, g) on the CPU as tests/test_gpu_pro.py draws them: h ~ N(0,1), W ~ 0.3 N(0,1), b ~ 0.3 N(0,1), uniform
    targets, g = (U(0,1) - 0.3) * 1e-3 with every seventh row exactly 0."""
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(R, K, generator=gen)
    Ws = [torch.randn(V, K, generator=gen) * 0.3 for V in Vs]
    bs = [torch.randn(V, generator=gen) * 0.3 for V in Vs]
    tgt = torch.stack([torch.randint(0, V, (R,), generator=gen) for V in Vs])
    g = (torch.rand(len(Vs), R, generator=gen) - 0.3) * 1e-3
    g[:, ::7] = 0.0
    return h, Ws, bs, tgt, g


def planted_targets(R, K, Vs):
    """Per field, the targets a large case puts on purpose (rows 1, 2, ... in this order; row 0 has g = 0): the last
    vocabulary row, the rows on both sides of every stage border inside the first range, and a row of the first block
    that a second trip of the weights-stationary kernel serves (block index >= 1024 over all fields)."""
    m = plan_mirror(R, K, Vs)
    out = []
    for fd in m["fields"]:
        V = fd["V"]
        want = [V - 1] + [v for s in range(1, m["spr"] + 1) for v in (VX_SB * s - 1, VX_SB * s)]
        want.append(max(0, VX_GRID - fd["blk0"]) * VX_SB + 5)
        out.append([v for v in want if 0 <= v < V])
    return out


def large_inputs(name):
    R, K, Vs = LARGE_CASES[name]
    h, Ws, bs, tgt, g = make_inputs(R, K, Vs, seed=9000 + R + K + len(Vs))
    for f, want in enumerate(planted_targets(R, K, Vs)):
        assert len(want) < R
        tgt[f, 1:1 + len(want)] = torch.tensor(want)
    return h, Ws, bs, tgt, g


def bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """`shape` floats between two bands of GUARD sentinels; the payload starts as `fill`.  pitch > shape[1]: rows `pitch`
    floats apart, the pad columns hold the sentinel as well."""

    def __init__(self, shape, fill, dev, pitch=None, guard=GUARD):
        shape = tuple(int(s) for s in shape)
        rows, cols = (shape if len(shape) == 2 else (1, shape[0]))
        self.pitch = int(pitch) if pitch is not None else cols
        assert self.pitch >= cols
        self.guard, self.n = guard, rows * self.pitch
        self.buf = torch.full((guard + self.n + guard,), SENTINEL, dtype=torch.float32, device=dev)
        self.wide = self.buf[guard:guard + self.n].view(rows, self.pitch)
        self.t = self.wide[:, :cols] if len(shape) == 2 else self.wide[0, :cols]
        self.t.fill_(fill)

    def untouched(self):
        """Both bands and every pad column still hold the sentinel's bits."""
        want = bits(torch.full((1,), SENTINEL, dtype=torch.float32, device=self.buf.device))
        g = self.guard
        outside = [self.buf[:g], self.buf[g + self.n:]] if g else []
        if self.pitch > self.t.shape[-1]:
            outside.append(self.wide[:, self.t.shape[-1]:])
        return all(bool((bits(o) == want).all()) for o in outside)


class Driven:
    """What `drive` hands back: ce [F, R], lse2 [F, rows_padded], wmax [F] (int32 bits), dh [R, K] (a view when pitched),
    dWs / dbs (None where not requested), `buffers` = name -> Guarded of every output, `scratch` = name -> tensor."""

    def outputs(self):
        return [("ce", self.ce), ("dh", self.dh)] + [("dW%d" % f, t) for f, t in enumerate(self.dWs) if t is not None] + \
               [("db%d" % f, t) for f, t in enumerate(self.dbs) if t is not None]

    def written_outside(self):
        return [name for name, b in self.buffers.items() if not b.untouched()]


def drive(lib, h, Ws, bs, tgt, g, n_rows=None, lddh=None, ldh_fwd=None, want_dW=None, want_db=None, poison=False, guards=False):
    """pack_hidden, fwd, pack_g, bwd_h, bwd_w on device tensors h [R, K], Ws, bs, tgt [F, R] int64, g [F, R], called through
    ctypes; the plan and the tables come from the library (ops._vce_plan / ops._vce_fields).
      n_rows    int: the `_n` entry points with this count in device memory; None: the entry points without a count
      lddh      row pitch of dh (default K); the pad columns hold SENTINEL
      ldh_fwd   fwd reads a copy of h with this pitch and NaN in the pad columns (pack_hidden keeps h: it wants ldh == K)
      want_dW / want_db   per field: False hands the kernel a NULL pointer
      poison    pack, gpack and both workspaces are NaN before the calls that write them (else uninitialised)
      guards    every output sits between bands of GUARD sentinels (else no bands; pad columns are still checked)"""
    from xdfm_amd import _lib, ops
    dev = h.device
    R, K = h.shape
    F_ = len(Ws)
    Vs = [int(w.shape[0]) for w in Ws]
    assert h.is_contiguous() and tgt.shape == (F_, R) and g.shape == (F_, R) and tgt.dtype == torch.int64
    want_dW = [True] * F_ if want_dW is None else list(want_dW)
    want_db = [True] * F_ if want_db is None else list(want_db)
    lddh = K if lddh is None else int(lddh)
    plan = ops._vce_plan(R, K, Vs, dev)
    rpad = int(lib.xdfm_vocab_ce_rows_padded(R))
    band = GUARD if guards else 0
    nan = float("nan")
    f32 = dict(dtype=torch.float32, device=dev)
    scratch = (lambda n: torch.full((int(n),), nan, **f32)) if poison else (lambda n: torch.empty(int(n), **f32))
    out = Driven()
    B = out.buffers = {}
    B["ce"] = Guarded((F_, R), nan, dev, guard=band)
    B["lse2"] = Guarded((F_, rpad), nan, dev, guard=band)
    B["wmax"] = Guarded((F_,), nan, dev, guard=band)
    B["dh"] = Guarded((R, K), nan, dev, pitch=lddh, guard=band)
    for f, V in enumerate(Vs):
        if want_dW[f]:
            B["dW%d" % f] = Guarded((V, K), nan, dev, guard=band)
        if want_db[f]:
            B["db%d" % f] = Guarded((V,), nan, dev, guard=band)
    out.dWs = [B["dW%d" % f].t if want_dW[f] else None for f in range(F_)]
    out.dbs = [B["db%d" % f].t if want_db[f] else None for f in range(F_)]
    out.ce, out.lse2, out.dh = B["ce"].t, B["lse2"].t, B["dh"].t
    out.wmax = B["wmax"].t.view(torch.int32)
    fields = ops._vce_fields(plan, Ws, bs, out.dWs, out.dbs, dev)
    items, n_items, ws_elems, n_blk = plan[1], plan[2], plan[3], plan[4]
    h_fwd, ldh = h, K
    if ldh_fwd is not None:
        ldh = int(ldh_fwd)
        wide = torch.full((R, ldh), nan, **f32)
        wide[:, :K] = h
        h_fwd = wide
    cnt = None if n_rows is None else torch.tensor([int(n_rows)], dtype=torch.int32, device=dev)
    P, st = ops._ptr, ops._stream()
    pack, ws1, gpack, ws2 = scratch(lib.xdfm_vocab_ce_pack_elems(R, K)), scratch(ws_elems), scratch(F_ * (4 + rpad)), scratch(ws_elems)
    out.scratch = dict(pack=pack, ws_fwd=ws1, gpack=gpack, ws_bwd=ws2)
    if cnt is None:
        _lib.check(lib.xdfm_vocab_ce_pack_hidden(P(h), K, R, K, P(pack), st), "pack_hidden")
        _lib.check(lib.xdfm_vocab_ce_fwd(P(pack), P(h_fwd), ldh, R, K, P(fields), F_, P(items), n_items, P(tgt), P(ws1), P(out.ce),
                                         P(out.lse2), P(out.wmax), st), "fwd")
        _lib.check(lib.xdfm_vocab_ce_pack_g(P(g), F_, R, P(gpack), st), "pack_g")
        _lib.check(lib.xdfm_vocab_ce_bwd_h(P(pack), R, K, P(fields), F_, P(items), n_items, P(tgt), P(g), P(gpack), P(out.lse2),
                                           P(out.wmax), P(ws2), P(out.dh), lddh, st), "bwd_h")
        _lib.check(lib.xdfm_vocab_ce_bwd_w(P(pack), R, K, P(fields), F_, n_blk, P(tgt), P(gpack), P(out.lse2), P(out.wmax), st), "bwd_w")
    else:
        _lib.check(lib.xdfm_vocab_ce_pack_hidden_n(P(h), K, R, K, P(pack), P(cnt), st), "pack_hidden_n")
        _lib.check(lib.xdfm_vocab_ce_fwd_n(P(pack), P(h_fwd), ldh, R, K, P(fields), F_, P(items), n_items, P(tgt), P(ws1), P(out.ce),
                                           P(out.lse2), P(out.wmax), P(cnt), st), "fwd_n")
        _lib.check(lib.xdfm_vocab_ce_pack_g_n(P(g), F_, R, P(gpack), P(cnt), st), "pack_g_n")
        _lib.check(lib.xdfm_vocab_ce_bwd_h_n(P(pack), R, K, P(fields), F_, P(items), n_items, P(tgt), P(g), P(gpack), P(out.lse2),
                                             P(out.wmax), P(ws2), P(out.dh), lddh, P(cnt), st), "bwd_h_n")
        _lib.check(lib.xdfm_vocab_ce_bwd_w_n(P(pack), R, K, P(fields), F_, n_blk, P(tgt), P(gpack), P(out.lse2), P(out.wmax), P(cnt),
                                             st), "bwd_w_n")
    torch.cuda.synchronize()
    out.keep = (fields, h_fwd, cnt, plan)
    return out


def errors(got, want):
    """(largest |got - want|, largest |want|) in float64."""
    want = want.double()
    if want.numel() == 0:
        return 0.0, 0.0
    return float((got.double() - want).abs().max()), float(want.abs().max())


def assert_bars(name, got, want, is_ce):
    """The bars of tests/test_gpu_pro.py::test_vocab_heads_ce_fused_vs_materialised_logits: ce rtol 2e-5, atol 2e-5;
    gradients rtol 2e-4, atol 2e-5 x the tensor's largest reference magnitude."""
    w = want.detach().cpu().double().numpy()
    assert tuple(got.shape) == w.shape, name
    if is_ce:
        np.testing.assert_allclose(got.detach().cpu().numpy(), w, rtol=2e-5, atol=2e-5, err_msg=name)
    else:
        amax = float(np.abs(w).max()) if w.size else 0.0
        np.testing.assert_allclose(got.detach().cpu().numpy(), w, rtol=2e-4, atol=2e-5 * amax, err_msg=name)
