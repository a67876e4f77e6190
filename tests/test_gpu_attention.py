"""GPU tests (-m gpu) of K5 (csrc/attn.hip: MHSA layers + attention pooling) driven directly on a feature map.

No CIN in front: the FM-layout tensor [S, B*D] is built here, so the token count S and the token distribution are
free.  The yardstick is the float64 composition cin_attention_forward applies (oracle.mhsa, residual, layer_norm,
oracle.attention_pooling); the bars are those of test_attention_kernel_vs_float64_oracle:
forward rtol 1e-4 / atol 1e-5 * max, gradients rtol 2e-3 / atol 2e-3 * max + 5e-6.

Random tokens at S in the hundreds give a nearly uniform softmax, under which a kernel that drops or double-counts
one key moves the result by about 1/S -- inside the gradient bar.  The needle and ramp inputs below are built so
that such a mistake changes the output at full size.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# Every (embedding_dim, heads) instance of ATTN_DISPATCH and its LDS envelope:
# (largest S the forward accepts, largest trainable S with 1 MHSA layer, with 2 layers).
# Pinned by test_lds_envelope_is_refused_past_the_limit; tests/test_attn_coverage.py checks that the keys are
# exactly the instances csrc/attn.hip builds.
ENVELOPE = {
    (4, 1): (1024, 1024, 1024), (4, 2): (1024, 1024, 1024), (4, 4): (1024, 1024, 1024),
    (8, 1): (1024, 1024, 1024), (8, 2): (1024, 1024, 1024), (8, 4): (1024, 960, 960),
    (10, 1): (1024, 1024, 1024), (10, 2): (1024, 1005, 990),
    (16, 1): (824, 702, 673), (16, 2): (824, 640, 633), (16, 4): (824, 572, 550), (16, 8): (824, 448, 446),
    (32, 2): (379, 256, 198), (32, 4): (379, 231, 192), (32, 8): (379, 192, 171),
}

# D, heads, S, B, n_layers, use_ln, use_res, train (False: only the forward fits at this S)
SWEEP = [
    (4, 1, 7, 3, 1, True, True, True), (4, 1, 1024, 2, 2, True, True, True),
    (4, 2, 65, 3, 1, False, True, True), (4, 2, 513, 2, 1, True, False, True),
    (4, 4, 1, 4, 2, True, True, True), (4, 4, 1024, 2, 1, True, True, True),
    (8, 1, 65, 3, 2, True, False, True), (8, 1, 1024, 2, 1, True, True, True),
    (8, 2, 7, 3, 1, True, True, True), (8, 2, 700, 2, 2, False, True, True),
    (8, 4, 100, 3, 1, True, True, True), (8, 4, 960, 2, 2, True, True, True),
    (10, 1, 33, 3, 1, True, True, True), (10, 1, 1024, 2, 1, False, True, True),
    (10, 2, 65, 3, 2, True, True, True), (10, 2, 990, 2, 2, True, True, True),
    (16, 1, 13, 3, 2, True, True, True), (16, 1, 702, 2, 1, True, True, True),
    (16, 2, 65, 3, 1, False, False, True), (16, 2, 640, 2, 1, True, True, True),
    (16, 4, 250, 3, 2, True, True, True), (16, 4, 512, 2, 1, True, True, True), (16, 4, 572, 2, 1, True, True, True),
    (16, 8, 129, 3, 2, True, True, True), (16, 8, 446, 2, 2, True, True, True), (16, 8, 824, 2, 1, True, True, False),
    (32, 2, 63, 3, 2, True, False, True), (32, 2, 256, 2, 1, True, True, True), (32, 2, 379, 2, 1, True, True, False),
    (32, 4, 31, 3, 1, True, True, True), (32, 4, 231, 2, 1, True, True, True), (32, 4, 379, 2, 2, False, True, False),
    (32, 8, 9, 3, 2, True, True, True), (32, 8, 171, 2, 2, True, True, True), (32, 8, 379, 2, 1, True, True, False),
]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close(got, want, rtol, atol, msg=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert np.isfinite(got).all(), msg + ": not finite"
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


def fclose(got, want, msg=""):
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    close(got, want, rtol=1e-4, atol=1e-5 * float(np.abs(want).max()) + 1e-7, msg=msg)


def gclose(got, want, msg=""):
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    close(got, want, rtol=2e-3, atol=2e-3 * float(np.abs(want).max()) + 5e-6, msg=msg)   # 5e-6: fp32 noise floor


class Block:
    """The modules K5 reads (CINAttentionV2's attention block without the CIN): n_layers x (MHSA, LayerNorm) and the
    pooling, built on the CPU; .params lists them in the order ops.attn_pool packs theta."""

    def __init__(self, D, nh, nl, ln, res, p_drop=0.0, seed=0):
        from xdfm_amd.layers import AttentionPooling, MultiHeadSelfAttention
        torch.manual_seed(seed)
        self.D, self.nl, self.ln, self.res = D, nl, ln, res
        self.mhsa = [MultiHeadSelfAttention(D, nh, p_drop) for _ in range(nl)]
        self.nh = self.mhsa[0].num_heads
        self.lns = [nn.LayerNorm(D) for _ in range(nl)] if ln else None
        self.pool = AttentionPooling(D, D)
        with torch.no_grad():                 # LayerNorm affine and pooling bias away from their identity init
            for m in (self.lns or []):
                m.weight.add_(0.3 * torch.randn(D))
                m.bias.add_(0.3 * torch.randn(D))
            self.pool.attention[0].bias.add_(0.3 * torch.randn(D))

    @property
    def params(self):
        out = []
        for l, a in enumerate(self.mhsa):
            out += [("W_q%d" % l, a.W_q.weight), ("W_k%d" % l, a.W_k.weight), ("W_v%d" % l, a.W_v.weight),
                    ("W_o%d" % l, a.W_o.weight)]
            if self.ln:
                out += [("gamma%d" % l, self.lns[l].weight), ("beta%d" % l, self.lns[l].bias)]
        return out + [("W1", self.pool.attention[0].weight), ("b1", self.pool.attention[0].bias),
                      ("w2", self.pool.attention[2].weight)]

    def to(self, dev):
        for m in self.mhsa + (self.lns or []) + [self.pool]:
            m.to(dev)
        return self

    def oracle(self, x, P, keep=None, p_drop=0.0, tokens=None):
        """float64 pooled output for tokens x [B, S, D] with parameters P (name -> tensor); `tokens` collects the
        output of every layer."""
        from oracle import xdeepfm_oracle as orc
        r = x
        for l in range(self.nl):
            a = orc.mhsa(r, P["W_q%d" % l], P["W_k%d" % l], P["W_v%d" % l], P["W_o%d" % l], self.nh,
                         None if keep is None else keep[l], p_drop)
            if self.res:
                a = a + r
            if self.ln:
                a = F.layer_norm(a, (self.D,), P["gamma%d" % l], P["beta%d" % l], 1e-5)
            r = a
            if tokens is not None:
                tokens.append(r)
        return orc.attention_pooling(r, P["W1"], P["b1"], P["w2"])


def to_fm(x):
    """[B, S, D] -> the FM layout [S, B*D] K5 reads."""
    B, S, D = x.shape
    return x.permute(1, 0, 2).reshape(S, B * D).contiguous()


def from_fm(fm, B, D):
    S = fm.shape[0]
    return fm.view(S, B, D).permute(1, 0, 2)


def keep_mask(B, S, nh, n_layers, p_drop, seed, dev):
    """The keep bits K5 generates for `seed`, through the C ABI: [n_layers, B, nh, S, S] uint8 (as _attn_keep_mask of
    test_gpu_parity.py)."""
    from xdfm_amd import _lib
    lib = _lib.load()
    keep = torch.empty((n_layers, B, nh, S, S), dtype=torch.uint8, device=dev)
    _lib.check(lib.xdfm_cin_attn_dropout_mask(B, S, nh, n_layers, float(p_drop), seed.data_ptr(), keep.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "mask")
    torch.cuda.synchronize()
    return keep


def run_and_compare(blk, x, gout=None, p_drop=0.0, train=True, what=""):
    """ops.attn_pool on the GPU against the float64 oracle: pooled output, dfm and every parameter gradient.  The
    backward runs twice on the same forward: both runs must give the same bits (no float atomics, fixed-order sums).
    Returns (pooled, dfm [B, S, D], grads) of the kernel."""
    from xdfm_amd import ops
    dev = _dev()
    B, S, D = x.shape
    P64 = {k: p.detach().double().requires_grad_(True) for k, p in blk.params}
    blk.to(dev)
    for m in blk.mhsa:
        m.train(p_drop > 0)
    fm = to_fm(x).to(dev).requires_grad_(True)
    out = ops.attn_pool(fm, B, D, blk.mhsa, blk.lns, blk.pool, blk.res)
    keep = None
    if p_drop > 0:
        seed = ops.AttnPool.last_drop_seed
        assert seed is not None
        keep = keep_mask(B, S, blk.nh, blk.nl, p_drop, seed, dev).cpu()
        assert 0 < float(keep.double().mean()) < 1
    x64 = x.double().requires_grad_(True)
    want = blk.oracle(x64, P64, keep, p_drop)
    fclose(out, want, what + " pooled")
    if not train:
        return out, None, None
    if gout is None:
        gout = torch.randn(B, D)
    (want * gout.double()).sum().backward()
    runs = []
    for _ in range(2):
        fm.grad = None
        for _, p in blk.params:
            p.grad = None
        (out * gout.to(dev)).sum().backward(retain_graph=True)
        runs.append((fm.grad.clone(), [p.grad.clone() for _, p in blk.params]))
    dfm = from_fm(runs[0][0], B, D)
    gclose(dfm, x64.grad, what + " dfm")
    for (name, _), g in zip(blk.params, runs[0][1]):
        gclose(g, P64[name].grad, what + " d" + name)
    assert torch.equal(runs[0][0], runs[1][0]), what + ": dfm differs between two backward runs"
    for (name, _), g0, g1 in zip(blk.params, runs[0][1], runs[1][1]):
        assert torch.equal(g0, g1), what + ": d%s differs between two backward runs" % name
    return out, dfm, runs[0][1]


def raw_fwd(blk, fm, B):
    """The forward through the C ABI, returning what it saves for the backward: pooled [B, D], layer outputs
    tok [L, B, S, D], attention outputs before W_o osv [L, B, S, D], softmax statistics ml [L, B, S, nh, 2]."""
    from xdfm_amd import _lib
    lib = _lib.load()
    S, D, L = fm.shape[0], blk.D, blk.nl
    theta = torch.cat([p.detach().reshape(-1) for _, p in blk.params]).to(fm.device)
    out = torch.empty((B, D), dtype=torch.float32, device=fm.device)
    tok = torch.empty((L, B, S, D), dtype=torch.float32, device=fm.device)
    osv = torch.empty_like(tok)
    ml = torch.empty((L, B, S, blk.nh, 2), dtype=torch.float32, device=fm.device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.xdfm_cin_attn_pool_fwd(P(fm), B, S, D, blk.nh, L, int(blk.ln), int(blk.res), P(theta), P(out), P(tok),
                                          P(osv), P(ml), 0.0, None, torch.cuda.current_stream().cuda_stream), "fwd")
    torch.cuda.synchronize()
    return theta, out, tok, osv, ml


# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("D,nh,S,B,nl,ln,res,train", SWEEP,
                         ids=["D%d_h%d_S%d_L%d%s%s%s" % (c[0], c[1], c[2], c[4], "" if c[5] else "_noln",
                                                         "" if c[6] else "_nores", "" if c[7] else "_fwd")
                              for c in SWEEP])
def test_every_instance_vs_float64_oracle(D, nh, S, B, nl, ln, res, train):
    """Every (D, heads) instance of ATTN_DISPATCH at S = 1 ... 1024: the 512-thread variant with a key-block tail
    (S % 8 != 0) and a last wave of one live thread (S = 65), the 1024-thread variant (S > 512) forward and backward up
    to the LDS limit of the backward; where only the forward fits past 512 (or at all), the forward."""
    blk = Block(D, nh, nl, ln, res, seed=D * 1000 + nh * 100 + S)
    assert blk.nh == nh
    fwd_max, train1, train2 = ENVELOPE[(D, nh)]
    assert S <= fwd_max and (not train or S <= (train1 if nl == 1 else train2))
    torch.manual_seed(S)
    x = 0.7 * torch.randn(B, S, D)
    run_and_compare(blk, x, train=train, what="D=%d heads=%d S=%d" % (D, nh, S))


def _needle_block(D, nh, ln):
    """Layer-0 weights under which one key t* of each example out-scores every other key by >= 40 for every query
    and head: q and k of head h read only element h*hd of the token, which is 1 for every token and 2 for t*."""
    blk = Block(D, nh, 1, ln, True, seed=D + nh)
    hd = D // nh
    c = 40.0 * hd ** 0.5                     # score(t*) - score(t) = c * x_s[h*hd] * (2 - 1) / sqrt(hd) >= 40
    with torch.no_grad():
        a = blk.mhsa[0]
        a.W_q.weight.zero_()
        a.W_k.weight.zero_()
        for h in range(nh):
            a.W_q.weight[h * hd, h * hd] = c
            a.W_k.weight[h * hd, h * hd] = 1.0
    return blk


@pytest.mark.parametrize("D,nh,S,tstar,ln", [
    (8, 4, 203, (0, 7, 8, 202), True),            # 512 threads: first key, block edges, the key-block tail (200..202)
    (10, 1, 1003, (511, 512, 513, 1002), False),  # 1024 threads, odd heads: keys around the 512 boundary, the tail
    (4, 1, 1001, (7, 8, 513, 1000), True),
    (16, 2, 603, (0, 511, 512, 602), False),
])
def test_attention_needle_selects_one_key(D, nh, S, tstar, ln):
    """With one key dominating every softmax row, the attention output of every query is v[t*] per head and the
    layer output is x + W_o v[t*] (before LayerNorm): a key dropped, double-counted or mis-addressed is an O(1) error
    whatever S is.  Example b has its needle at tstar[b]."""
    dev = _dev()
    blk = _needle_block(D, nh, ln)
    B, hd = len(tstar), D // nh
    torch.manual_seed(S)
    x = 0.5 * torch.randn(B, S, D)
    for h in range(nh):
        x[:, :, h * hd] = 1.0
        for b, t in enumerate(tstar):
            x[b, t, h * hd] = 2.0
    # exact attention output of the construction: v[t*] for every query
    x64 = x.double()
    Wv, Wo = blk.mhsa[0].W_v.weight.detach().double(), blk.mhsa[0].W_o.weight.detach().double()
    vstar = torch.stack([x64[b, t] @ Wv.t() for b, t in enumerate(tstar)])        # [B, D]
    o_want = vstar[:, None, :].expand(B, S, D)
    y_want = x64 + o_want @ Wo.t()
    # the oracle agrees with the construction (margin >= 40: other keys weigh < S * e^-40)
    toks = []
    P64 = {k: p.detach().double() for k, p in blk.params}
    blk.oracle(x64, P64, tokens=toks)
    want_tok = F.layer_norm(y_want, (D,), P64["gamma0"], P64["beta0"], 1e-5) if ln else y_want
    assert torch.allclose(toks[0], want_tok, rtol=1e-9, atol=1e-9)
    blk.to(dev)
    _, _, tok, osv, _ = raw_fwd(blk, to_fm(x).to(dev), B)
    fclose(osv[0], o_want, "attention output != v[t*]")
    fclose(tok[0], want_tok, "layer output != x + W_o v[t*]")
    run_and_compare(_needle_block(D, nh, ln), x, what="needle")


@pytest.mark.parametrize("D,nh,S,sp,ln", [
    (16, 4, 129, (128, 128), True),           # 512 threads: the one live thread of the last wave
    (8, 1, 577, (576, 576), False),           # 1024 threads: the same at S = 9 * 64 + 1
    (10, 2, 700, (699, 640), True),           # first and last live thread of a partly live last wave
])
def test_pooling_needle_in_the_last_wave(D, nh, S, sp, ln):
    """The pooling softmax dominated by one token sp[b] in the last, partly live wave: the pooled output is that
    token (the layer's output, read back from the forward's saved tokens) and must match float64 forward and back.
    Element 0 of every token is -2, of the needle +2; W_o is small so that the MHSA layer keeps the sign
    (use_res), W1 / w2 read element 0 only: score(needle) - score(other) ~ 80."""
    dev = _dev()
    blk = Block(D, nh, 1, ln, True, seed=S)
    with torch.no_grad():
        if ln:                                # LayerNorm keeps the sign of element 0
            blk.lns[0].weight[0] = 1.0
            blk.lns[0].bias[0] = 0.0
        blk.mhsa[0].W_o.weight.mul_(0.05)
        blk.pool.attention[0].weight.zero_()
        blk.pool.attention[0].weight[0, 0] = 5.0
        blk.pool.attention[0].bias.zero_()
        blk.pool.attention[2].weight.zero_()
        blk.pool.attention[2].weight[0, 0] = 40.0
    B = len(sp)
    torch.manual_seed(S + 1)
    x = 0.5 * torch.randn(B, S, D)
    x[:, :, 0] = -2.0
    for b, s in enumerate(sp):
        x[b, s, 0] = 2.0
    toks = []
    P64 = {k: p.detach().double() for k, p in blk.params}
    pooled = blk.oracle(x.double(), P64, tokens=toks)
    for b, s in enumerate(sp):
        assert torch.allclose(pooled[b], toks[0][b, s], rtol=1e-12, atol=1e-12)
    blk.to(dev)
    _, out, tok, _, _ = raw_fwd(blk, to_fm(x).to(dev), B)
    for b, s in enumerate(sp):
        fclose(out[b], tok[0, b, s], "pooled != token %d" % s)
    blk.to("cpu")
    run_and_compare(blk, x, what="pooling needle")


@pytest.mark.parametrize("D,nh,S,nl,direction", [
    (8, 1, 1000, 1, 1), (8, 1, 1000, 1, -1),
    (10, 2, 777, 2, 1),
    (16, 4, 500, 1, -1),
    (32, 8, 171, 1, 1),
])
def test_ramp_moves_the_running_maximum(D, nh, S, nl, direction):
    """Token norms along t as r_t = -1 ... 1 (direction 1) or 1 ... -1: for a query with r_s > 0 the scores rise along
    the keys and the running maximum of the one-pass softmax moves in every key block of 8; for r_s < 0 they fall.
    Scores reach +-100 in base-2 units (q = k = alpha x, alpha^2 = 100 sqrt(hd) / log2(e))."""
    import math
    blk = Block(D, nh, nl, True, True, seed=S + nl)
    hd = D // nh
    alpha = math.sqrt(100.0 * math.sqrt(hd) / math.log2(math.e))
    with torch.no_grad():
        for a in blk.mhsa[:1]:
            a.W_q.weight.copy_(alpha * torch.eye(D))
            a.W_k.weight.copy_(alpha * torch.eye(D))
    torch.manual_seed(S)
    B = 2
    r = torch.linspace(-1.0, 1.0, S) * direction
    u = torch.full((D,), 1.0 / math.sqrt(hd))                  # unit norm in every head
    x = r[None, :, None] * u + 0.05 * torch.randn(B, S, D)
    x[1] = x[1].flip(0) * 0.9                                   # example 1: the other direction, a little lower
    run_and_compare(blk, x, what="ramp")


@pytest.mark.parametrize("D,nh,S,B,nl,p_drop", [
    (8, 1, 777, 2, 2, 0.3),        # 1024 threads, odd heads
    (10, 1, 65, 3, 1, 0.5),        # 512 threads, odd heads
    (4, 2, 1000, 2, 1, 0.2),       # 1024 threads, heads interleaved
    (16, 4, 560, 2, 1, 0.1),       # 1024 threads at the default model's instance
])
def test_dropout_on_odd_heads_and_1024_threads(D, nh, S, B, nl, p_drop):
    """Attention dropout on the non-interleaved (odd heads) branches and the 1024-thread variant: the keep mask K5
    regenerated is read back with xdfm_cin_attn_dropout_mask and handed to the oracle; forward and every gradient
    must agree, which needs the forward and both backward passes to see the same bits."""
    blk = Block(D, nh, nl, True, True, p_drop=p_drop, seed=S)
    torch.manual_seed(S)
    x = 0.7 * torch.randn(B, S, D)
    run_and_compare(blk, x, p_drop=p_drop, what="dropout %g" % p_drop)


@pytest.mark.parametrize("D,nh,S,B,nl", [(10, 1, 20, 2049, 1), (4, 2, 9, 4097, 2), (4, 1, 70, 2049, 1)])
def test_workgroups_with_several_examples(D, nh, S, B, nl):
    """B > 2048: the backward's 2048 workgroups take examples b, b + 2048, ... and accumulate their parameter
    gradients across them; the per-example gradients must still be right for every example."""
    blk = Block(D, nh, nl, True, True, seed=B)
    torch.manual_seed(B)
    x = 0.7 * torch.randn(B, S, D)
    run_and_compare(blk, x, what="B=%d" % B)


def test_atomic_entry_point_matches_the_deterministic_one():
    """xdfm_cin_attn_pool_bwd (fp32 atomics into dtheta, no workspace) against xdfm_cin_attn_pool_bwd_det: the same
    dfm bits (dfm is written per thread, not summed across workgroups), dtheta to fp32 reordering."""
    from xdfm_amd import _lib
    dev = _dev()
    lib = _lib.load()
    D, nh, S, B, nl = 8, 1, 300, 5, 2
    blk = Block(D, nh, nl, True, True, seed=5).to(dev)
    torch.manual_seed(5)
    x = 0.7 * torch.randn(B, S, D)
    fm = to_fm(x).to(dev)
    theta, _, tok, osv, ml = raw_fwd(blk, fm, B)
    dout = torch.randn(B, D, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    dfm_det, dth_det = torch.empty_like(fm), torch.empty_like(theta)
    ws = torch.empty(lib.xdfm_cin_attn_pool_bwd_ws_elems(B, D, nl, 1), dtype=torch.float32, device=dev)
    _lib.check(lib.xdfm_cin_attn_pool_bwd_det(P(fm), B, S, D, nh, nl, 1, 1, P(theta), P(tok), P(osv), P(ml), P(dout),
                                              P(dfm_det), P(dth_det), P(ws), 0.0, None, st), "bwd_det")
    dfm_at, dth_at = torch.empty_like(fm), torch.zeros_like(theta)
    _lib.check(lib.xdfm_cin_attn_pool_bwd(P(fm), B, S, D, nh, nl, 1, 1, P(theta), P(tok), P(osv), P(ml), P(dout),
                                          P(dfm_at), P(dth_at), 0.0, None, st), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(dfm_at, dfm_det)
    close(dth_at, dth_det.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(dth_det.abs().max()))


# --------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("D,heads,nh", [(6, 4, 3), (64, 4, 4)])
def test_unbuilt_embedding_dim_is_refused(D, heads, nh):
    """No kernel instance for this D: a clear error at the forward that names D and the head count.  (Refused shapes
    come back as XDFM_ERR_INVALID, which _lib.check raises as ValueError.)"""
    from xdfm_amd import ops
    dev = _dev()
    blk = Block(D, heads, 1, True, True).to(dev)
    assert blk.nh == nh
    fm = torch.randn(8, 2 * D, device=dev)
    with pytest.raises(ValueError, match=r"embedding_dim %d, heads %d\) has no kernel instance" % (D, nh)):
        ops.attn_pool(fm, 2, D, blk.mhsa, blk.lns, blk.pool, True)


def test_more_than_1024_tokens_is_refused():
    from xdfm_amd import ops
    dev = _dev()
    blk = Block(4, 1, 1, True, True).to(dev)
    fm = torch.randn(1025, 2 * 4, device=dev)
    with pytest.raises(ValueError, match=r"bad shape B=2 S=1025"):
        ops.attn_pool(fm, 2, 4, blk.mhsa, blk.lns, blk.pool, True)


def test_forward_only_shape_refuses_the_backward():
    """D = 32, 4 heads at config 3's S = 320: the forward fits LDS (up to S = 379) and is right; the backward does not
    fit (up to S = 231) and must say so instead of launching."""
    from xdfm_amd import ops
    dev = _dev()
    blk = Block(32, 4, 1, True, True, seed=320)
    torch.manual_seed(320)
    x = 0.7 * torch.randn(2, 320, 32)
    run_and_compare(blk, x, train=False, what="D=32 S=320")
    fm = to_fm(x).to(dev).requires_grad_(True)
    out = ops.attn_pool(fm, 2, 32, blk.mhsa, blk.lns, blk.pool, True)
    with pytest.raises(ValueError, match=r"S=320 D=32 does not fit LDS"):
        out.sum().backward()


@pytest.mark.parametrize("D,nh", sorted(k for k, v in ENVELOPE.items() if min(v) < 1024))
def test_lds_envelope_is_refused_past_the_limit(D, nh):
    """The ENVELOPE table (also in DESIGN.md, K5): one token past the forward's limit is refused at the forward, one
    past the trainable limit (1 and 2 layers) at the backward.  The limits themselves run in the sweep above."""
    from xdfm_amd import ops
    dev = _dev()
    fwd_max, train1, train2 = ENVELOPE[(D, nh)]
    if fwd_max < 1024:
        blk = Block(D, nh, 1, True, True).to(dev)
        with pytest.raises(ValueError, match=r"S=%d D=%d does not fit LDS" % (fwd_max + 1, D)):
            ops.attn_pool(torch.randn(fwd_max + 1, D, device=dev), 1, D, blk.mhsa, blk.lns, blk.pool, True)
    for nl, lim in ((1, train1), (2, train2)):
        if lim >= min(fwd_max, 1024):
            continue
        blk = Block(D, nh, nl, True, True).to(dev)
        fm = torch.randn(lim + 1, D, device=dev, requires_grad=True)
        out = ops.attn_pool(fm, 1, D, blk.mhsa, blk.lns, blk.pool, True)
        with pytest.raises(ValueError, match=r"S=%d D=%d does not fit LDS" % (lim + 1, D)):
            out.sum().backward()
