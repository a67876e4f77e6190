"""K9 (csrc/vocab_ce_x3.hip) with a device-side row count: `ops.vocab_heads_ce(..., n_rows=...)` over a capacity of 1100 rows
(three row groups of 512, the last one partial) against a float64 numpy cross-entropy of the first n rows.  Everything
behind the count -- hidden rows, upstream gradients -- is NaN and the targets there are far out of range: nothing of it
may reach an output.  Tolerances: those of tests/test_gpu_pro.py::test_vocab_heads_ce_fused_vs_materialised_logits (the
f16x3 products carry ~2^-22 relative error per term, the base-2 exp / log ~1 ulp)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CAP = 1100
VOCABS = (7, 300, 1000)
COUNTS = [0, 1, 32, 33, 511, 512, 513, 1024, 1100]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(K):
    g = torch.Generator().manual_seed(1100 + K)
    h = torch.randn(CAP, K, generator=g)
    Ws = [torch.randn(V, K, generator=g) * 0.3 for V in VOCABS]
    bs = [torch.randn(V, generator=g) * 0.3 for V in VOCABS]
    tgt = torch.stack([torch.randint(0, V, (CAP,), generator=g) for V in VOCABS])
    gout = (torch.rand(len(VOCABS), CAP, generator=g) - 0.3) * 1e-3            # both signs
    gout[:, ::7] = 0.0                                                         # and exact zeros
    return h, Ws, bs, tgt, gout


def _reference(K, n):
    """float64: ce [F, n], dh [n, K], dW, db of the first n rows."""
    h, Ws, bs, tgt, gout = (_inputs(K))
    h64 = h[:n].double().numpy()
    dh = np.zeros((n, K))
    ce, dWs, dbs = [], [], []
    for f, (W, b) in enumerate(zip(Ws, bs)):
        W64, b64 = W.double().numpy(), b.double().numpy()
        z = h64 @ W64.T + b64
        m = z.max(axis=1, keepdims=True) if n else np.zeros((0, 1))
        e = np.exp(z - m)
        lse = m[:, 0] + np.log(e.sum(axis=1))
        t = tgt[f, :n].numpy()
        ce.append(lse - z[np.arange(n), t])
        G = e / e.sum(axis=1, keepdims=True)
        G[np.arange(n), t] -= 1.0
        G *= gout[f, :n].double().numpy()[:, None]
        dh += G @ W64
        dWs.append(G.T @ h64)
        dbs.append(G.sum(axis=0))
    return np.stack(ce), dh, dWs, dbs


def _run(K, n, dev, counted=True, poison=True):
    from xdfm_amd import ops
    h, Ws, bs, tgt, gout = (t.clone() if torch.is_tensor(t) else [u.clone() for u in t] for t in _inputs(K))
    if poison:
        h[n:] = float("nan")
        gout[:, n:] = float("nan")
        tgt[:, n:] = 1 << 40
    h = h.to(dev).requires_grad_(True)
    Ws = [w.to(dev).requires_grad_(True) for w in Ws]
    bs = [b.to(dev).requires_grad_(True) for b in bs]
    n_rows = torch.tensor([n], dtype=torch.int32, device=dev) if counted else None
    ce = ops.vocab_heads_ce(h, tgt.to(dev), Ws, bs, n_rows=n_rows)
    ce.backward(gout.to(dev))
    torch.cuda.synchronize()
    return ce.detach(), h.grad, [w.grad for w in Ws], [b.grad for b in bs]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("K", [32, 64])
def test_counted_heads_vs_float64_numpy(K, n):
    from xdfm_amd import ops
    dev = _dev()
    assert ops.vocab_heads_ce_supported(K)
    ce, dh, dWs, dbs = _run(K, n, dev)
    for name, t in [("ce", ce), ("dh", dh)] + [("dW%d" % f, t) for f, t in enumerate(dWs)] + [("db%d" % f, t) for f, t in enumerate(dbs)]:
        assert torch.isfinite(t).all(), name + " holds a NaN or an infinity"
    assert ce.shape == (len(VOCABS), CAP) and dh.shape == (CAP, K)
    assert (ce[:, n:] == 0).all() and (dh[n:] == 0).all()                      # absent rows: exact zeros
    want_ce, want_dh, want_dW, want_db = _reference(K, n)
    np.testing.assert_allclose(ce[:, :n].cpu().numpy(), want_ce, rtol=2e-5, atol=2e-5)
    pairs = [(dh[:n], want_dh, "dh")] + [(t, w, "dW%d" % f) for f, (t, w) in enumerate(zip(dWs, want_dW))] + \
            [(t, w, "db%d" % f) for f, (t, w) in enumerate(zip(dbs, want_db))]
    for got, w, name in pairs:
        amax = float(np.abs(w).max()) if w.size else 0.0
        np.testing.assert_allclose(got.cpu().numpy(), w, rtol=2e-4, atol=2e-5 * amax, err_msg=name)


def _old_entry_points(K, dev):
    """(ce, dh, dWs, dbs) from the entry points WITHOUT a count -- xdfm_vocab_ce_pack_hidden, _fwd, _pack_g, _bwd_h, _bwd_w --
    called through ctypes as include/xdfm.h documents them: the caller's plan, tables, pack, workspaces and a zeroed lse2."""
    from xdfm_amd import _lib, ops
    lib = _lib.load()
    h, Ws, bs, tgt, gout = _inputs(K)
    h, tgt, g = h.to(dev).contiguous(), tgt.to(dev).contiguous(), gout.to(dev).contiguous()
    Ws, bs = [w.to(dev) for w in Ws], [b.to(dev) for b in bs]
    F_, R = len(VOCABS), CAP
    f32 = dict(dtype=torch.float32, device=dev)
    plan = ops._vce_plan(R, K, list(VOCABS), dev)
    dWs, dbs = [torch.full_like(w, float("nan")) for w in Ws], [torch.full_like(b, float("nan")) for b in bs]
    fields = ops._vce_fields(plan, Ws, bs, dWs, dbs, dev)
    P, st = ops._ptr, ops._stream()
    Rpad = lib.xdfm_vocab_ce_rows_padded(R)
    pack = torch.empty(lib.xdfm_vocab_ce_pack_elems(R, K), **f32)
    _lib.check(lib.xdfm_vocab_ce_pack_hidden(P(h), K, R, K, P(pack), st), "pack_hidden")
    ce, lse2 = torch.full((F_, R), float("nan"), **f32), torch.zeros(F_, Rpad, **f32)
    wmax, ws = torch.empty(F_, dtype=torch.int32, device=dev), torch.empty(plan[3], **f32)
    _lib.check(lib.xdfm_vocab_ce_fwd(P(pack), P(h), K, R, K, P(fields), F_, P(plan[1]), plan[2], P(tgt), P(ws), P(ce), P(lse2),
                                     P(wmax), st), "fwd")
    gpack = torch.empty(F_ * (4 + Rpad), **f32)
    _lib.check(lib.xdfm_vocab_ce_pack_g(P(g), F_, R, P(gpack), st), "pack_g")
    dh, ws2 = torch.full((R, K), float("nan"), **f32), torch.empty(plan[3], **f32)
    _lib.check(lib.xdfm_vocab_ce_bwd_h(P(pack), R, K, P(fields), F_, P(plan[1]), plan[2], P(tgt), P(g), P(gpack), P(lse2), P(wmax),
                                       P(ws2), P(dh), K, st), "bwd_h")
    _lib.check(lib.xdfm_vocab_ce_bwd_w(P(pack), R, K, P(fields), F_, plan[4], P(tgt), P(gpack), P(lse2), P(wmax), st), "bwd_w")
    torch.cuda.synchronize()
    return ce, dh, dWs, dbs


@pytest.mark.parametrize("K", [32, 64])
def test_full_count_has_the_bits_of_the_uncounted_entry_points(K):
    """n == capacity: the plan, the tiles walked and every summation order are those of the entry points without a count.
    The reference arm calls the existing C symbols themselves; `ops.vocab_heads_ce` without a count (a null pointer handed
    to the `_n` symbols) must give the same bits as well."""
    dev = _dev()
    a = _run(K, CAP, dev, counted=True, poison=False)
    b = _old_entry_points(K, dev)
    c = _run(K, CAP, dev, counted=False, poison=False)
    flat = lambda r: [r[0], r[1]] + list(r[2]) + list(r[3])
    for i, (x, y, z) in enumerate(zip(flat(a), flat(b), flat(c))):
        assert torch.isfinite(y).all(), "output %d of the existing entry points" % i
        assert torch.equal(x, y), "output %d: counted call at n == capacity against the existing entry points" % i
        assert torch.equal(z, y), "output %d: call without a count against the existing entry points" % i


def test_kept_state_hands_out_the_same_gradients():
    """`ops.VocabHeadsState`: the field table and the dW / db tensors kept across steps -- two steps with different counts give
    what the stateless calls give, and the second step's table is the first one's (no upload)."""
    from xdfm_amd import ops
    dev = _dev()
    K = 32
    h0, Ws0, bs0, tgt, gout = _inputs(K)
    Ws = [w.to(dev).requires_grad_(True) for w in Ws0]
    bs = [b.to(dev).requires_grad_(True) for b in bs0]
    state = ops.VocabHeadsState()
    table = None
    for n in (513, 40):
        n_rows = torch.tensor([n], dtype=torch.int32, device=dev)
        outs = []
        for st in (state, None):
            h = h0.to(dev).requires_grad_(True)
            for p in Ws + bs:
                p.grad = None
            ce = ops.vocab_heads_ce(h, tgt.to(dev), Ws, bs, n_rows=n_rows, state=st)
            ce.backward(gout.to(dev))
            outs.append([ce.detach().clone(), h.grad.clone()] + [p.grad.clone() for p in Ws + bs])
        for x, y in zip(*outs):
            assert torch.equal(x, y)
        (_, t), = state.tables.values()
        assert table is None or t is table
        table = t
