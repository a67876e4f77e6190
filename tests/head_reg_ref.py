"""float64 references, error bounds and the shared case lists of the output head, the bias-gradient column sums and the
L2 regulariser (csrc/reg.hip).  Imported by test_head_reg_reference.py (CPU), test_gpu_head_reg.py and, through
head_reg_drivers.py (the GPU drivers of the same cases), head_reg_cases.py.

Everything here is plain numpy on the CPU; the operands are float32 arrays (what the kernels read), widened to float64
before any arithmetic.

Error model.  eps = 2^-24 is the unit roundoff of float32: one correctly rounded operation has a relative error of at
most eps.  A sum of n addends evaluated in ANY order, each addend the product of two float32 numbers (rounded, or fused
into the add), is within gamma(n) * sum |addends| of the exact sum, gamma(n) = n eps / (1 - n eps) (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: n - 1 additions and one rounding of the product are at most n roundings
on the path of any addend; additions of exact zeros are exact, so the fixed trees of the kernels, which add partials of
rows that do not exist as zeros, do not count).  gamma(n) is n * eps to first order; the second-order term is kept so
that the bound is a theorem at B = 65536 too.

"ulp" is the RELATIVE unit 2^-23 |x| = 2 eps |x|; k correctly rounded operations in a row are within k / 2 ulp.

Head.  fp32 saturation is part of the contract (ATen clamps the logs at -100 and the denominator of the BCE backward at
1e-12, and an fp32 sigmoid is exactly 0 below z ~ -88.7 and exactly 1 above z ~ 17.3), so the truth is staged:
  pred    against sigmoid(z64), z64 the float64 sum of the fp32 operands:
              |pred - p64| <= 0.25 gamma(n) A_b + 4 eps p64
          (A_b = sum of the absolute terms of row b, n their number; sigmoid' <= 1/4; expf is 1 ulp = 2 eps, 1 + e and
          the division one rounding each);
  loss    against the float64 sum of -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)) ON THE KERNEL'S OWN fp32 pred:
              |loss - loss64| <= gamma(B) S + 5 eps S + eps sum_b (1 - t_b),     S = sum_b (t |L1| + (1 - t) |L0|)
          -- the B addends, plus, as in the pred bound, the evaluation of one term: logf 1 ulp (2 eps), the product, the
          rounding of 1 - t, the add of the two halves (5 eps of the term in all); and fl(1 - p), which is exact for
          p >= 1/2 and otherwise off by at most 2^-25 of a number above 1/2, moves log(1 - p) by at most eps ABSOLUTE;
  g       = gloss (p - t) pq / max(pq, 1e-12), pq = p (1 - p), in float64 on the fp32 pred.  The kernel spells it
          ((gloss * (p - t)) / max(pq, 1e-12f)) * pq: four roundings (pq cancels where it is not clamped; where it is
          clamped p < 1e-12, fl(1 - p) = 1 and pq = p exactly) -> dlin within 2 ulp of g;
  du, dv  single products g_b * w[k] of the kernel's OWN fp32 g (its dlin): 2 ulp allowed, one rounding used;
  dwu, dwv, dbias   sums over b of g_b u[b][k] (g_b) with the kernel's own fp32 g: gamma(B) * sum_b |g_b u[b][k]|.

Column sums: gamma(rows) * sum_r |g[r][c]| per column.  L2 value: gamma(numel) * sum_t |c_t| sum w^2, numel the number of
elements of all tensors of the call; the fixed part of the reduction (the 4 accumulators, the wave shuffles, the 32
partials, the coefficient, the 256-wide tree: L2_TREE_DEPTH roundings) is covered by it only when the call holds at least
that many elements, which every case of L2_CASES does (asserted in l2_case).  That bar grows with the size of the call
(a third of the value at 2^22 elements), so the value is ALSO held to the bound that follows from the kernels' own walk
(l2_value_ref), which is tighter wherever a tensor is large.  L2 gradient: reproduced bit for bit in
float32, sc = fl(fl(2 c) * gs), g = fl(sc * w).
"""
import numpy as np

EPS = 2.0 ** -24
ULP = 2.0 ** -23            # relative
TINY = 2.0 ** -149          # the smallest fp32 denormal: the absolute slack of an "ulp" bound at the bottom of the range


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * EPS / (1.0 - n * EPS)


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------
# head
# ------------------------------------------------------------------------------------------------------------------
def sigmoid64(z):
    z = np.asarray(z, dtype=np.float64)
    return np.exp(-np.logaddexp(0.0, -z))


def head_logits(lin, u, wu, v, wv, bias):
    """(z64 [B], A [B], n) from the fp32 operands (each may be None): the float64 sum, the sum of the absolute terms
    and the number of terms of a row (scalars 0.0, 0.0, 0 when every operand is absent)."""
    z, A, n = 0.0, 0.0, 0
    if lin is not None:
        l = f64(lin).reshape(-1)
        z, A, n = z + l, A + np.abs(l), n + 1
    if u is not None:
        t = f64(u) * f64(wu).reshape(1, -1)
        z, A, n = z + t.sum(1), A + np.abs(t).sum(1), n + t.shape[1]
    if v is not None:
        t = f64(v) * f64(wv).reshape(1, -1)
        z, A, n = z + t.sum(1), A + np.abs(t).sum(1), n + t.shape[1]
    if bias is not None:
        b = float(f64(bias).reshape(-1)[0])
        z, A, n = z + b, A + abs(b), n + 1
    return z, A, n


def head_pred_ref(lin, u, wu, v, wv, bias, B):
    """(p64 [B], bound [B]) of the first stage."""
    z, A, n = head_logits(lin, u, wu, v, wv, bias)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (B,))
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), (B,))
    p = sigmoid64(z)
    return p, 0.25 * gamma(max(n, 1)) * A + 4.0 * EPS * p


def head_loss_ref(pred32, t32):
    """(loss64, bound, terms64 [B]) of the second stage: ATen's clamped BCE on the given fp32 pred, summed in float64."""
    p, t = f64(pred32).reshape(-1), f64(t32).reshape(-1)
    with np.errstate(divide="ignore"):
        L1 = np.maximum(np.log(p), -100.0)
        L0 = np.maximum(np.log1p(-p), -100.0)
    terms = -(t * L1 + (1.0 - t) * L0)
    S = float((t * np.abs(L1) + (1.0 - t) * np.abs(L0)).sum())
    bound = float(gamma(p.size)) * S + 5.0 * EPS * S + EPS * float((1.0 - t).sum())
    return float(terms.sum()), bound, terms


def head_g_ref(pred32, t32, gloss32):
    """g64 [B] = gloss (p - t) pq / max(pq, 1e-12) on the fp32 pred (the clamp constant is the fp32 1e-12f)."""
    p, t = f64(pred32).reshape(-1), f64(t32).reshape(-1)
    pq = p * (1.0 - p)
    return float(np.float32(gloss32)) * (p - t) * pq / np.maximum(pq, float(np.float32(1e-12)))


def ulp_bound(ref, k=2.0):
    return k * ULP * np.abs(ref) + k * TINY


def head_grads_ref(g32, u, wu, v, wv):
    """From the fp32 g the kernel produced: dict name -> (reference float64, bound) for du, dv, dwu, dwv, dbias."""
    g = f64(g32).reshape(-1)
    B = g.size
    out = {"dbias": (g.sum(), float(gamma(B)) * np.abs(g).sum())}
    for nm, x, w in (("u", u, wu), ("v", v, wv)):
        if x is None:
            continue
        d = g[:, None] * f64(w).reshape(1, -1)
        out["d" + nm] = (d, ulp_bound(d))
        t = g[:, None] * f64(x)
        out["dw" + nm] = (t.sum(0), float(gamma(B)) * np.abs(t).sum(0))
    return out


#      name              B      Ku    Kv   lin    bias   labels  misalign   z scale    what it is there for
HEAD_CASES = [
    # the 16 present / absent combinations of (u, v, lin, bias); Ku = 64 and Kv = 60 run the float4 kernels
    ("c0000",           17,     0,    0, False, False, "hard", None,     1.0),       # all absent: z = 0, p = 1/2
    ("c0001",           17,     0,    0, False, True,  "soft", None,     1.0),
    ("c0010",           17,     0,    0, True,  False, "hard", None,     1.0),
    ("c0011",           17,     0,    0, True,  True,  "soft", None,     1.0),
    ("c0100",           17,     0,   60, False, False, "hard", None,     1.0),
    ("c0101",           17,     0,   60, False, True,  "soft", None,     1.0),
    ("c0110",           17,     0,   60, True,  False, "hard", None,     1.0),
    ("c0111",           17,     0,   60, True,  True,  "soft", None,     1.0),
    ("c1000",           17,    64,    0, False, False, "hard", None,     1.0),
    ("c1001",           17,    64,    0, False, True,  "soft", None,     1.0),
    ("c1010",           17,    64,    0, True,  False, "hard", None,     1.0),
    ("c1011",           17,    64,    0, True,  True,  "soft", None,     1.0),
    ("c1100",           17,    64,   60, False, False, "hard", None,     1.0),
    ("c1101",           17,    64,   60, False, True,  "soft", None,     1.0),
    ("c1110",           17,    64,   60, True,  False, "hard", None,     1.0),
    ("c1111",           17,    64,   60, True,  True,  "soft", None,     1.0),
    # K and B sweep
    ("k1_b15",          15,     1,    0, True,  True,  "hard", None,     1.0),       # scalar: K % 4
    ("k3_k4_b16",       16,     3,    4, True,  True,  "soft", None,     1.0),       # scalar: odd Ku
    ("k3_k1_b1",         1,     3,    1, True,  True,  "hard", None,     1.0),       # scalar, B = 1
    ("k64_k60_b1",       1,    64,   60, True,  True,  "soft", None,     1.0),       # float4, B = 1
    ("k4_k68_b2047",  2047,     4,   68, True,  True,  "hard", None,     1.0),       # float4, one row short of a stride
    ("k512_k200_b2048", 2048, 512,  200, True,  True,  "sat",  None,    60.0),       # float4, its widest K, one stride, saturating
    ("k516_k64_b2049", 2049,  516,   64, True,  True,  "sat",  None,    60.0),       # scalar by size, saturating
    ("k200_k512_b4099", 4099, 200,  512, True,  False, "soft", None,     1.0),       # float4, ragged third stride
    ("k1000_b17",       17,  1000,    0, False, True,  "hard", None,     1.0),       # scalar by size
    ("k4000_k95_b16",   16,  4000,   95, True,  True,  "soft", None,     1.0),       # Ku + Kv = 4095: all of the 64 KiB of LDS
    ("k64_k4_b65536", 65536,   64,    4, True,  True,  "hard", None,     3.0),       # float4, 32 strides
    ("k5_k8_b65536",  65536,    5,    8, True,  True,  "soft", None,     3.0),       # scalar, 128 strides
    ("k64_k64_u_off", 2048,    64,   64, True,  True,  "hard", "u",      1.0),       # u one float off 16 bytes: scalar by alignment
    ("k64_k64_wv_off",  17,    64,   64, False, False, "soft", "wv",     1.0),       # wv one float off: scalar by alignment
]
HEAD_GLOSS = [0.37, 1.0, -2.5, 1.75]      # by position in HEAD_CASES; 1.0 occurs, the others are not 1


def head_case_names():
    return [c[0] for c in HEAD_CASES]


def head_vectorised(Ku, Kv, misalign):
    """The host's choice (xdfm_head_fwd / xdfm_head_bwd): the float4 kernels need K % 4 == 0, K <= 512 and 16-byte
    aligned operands; an absent operand counts as K = 0 and address 0."""
    return Ku % 4 == 0 and Kv % 4 == 0 and Ku <= 512 and Kv <= 512 and misalign is None


def make_head_case(name):
    """fp32 numpy operands of a case: dict with lin [B] | None, u, wu, v, wv, bias [1] | None, y [B], gloss (float32
    scalar), and B, Ku, Kv, misalign, labels.  The generator is seeded from the shape."""
    idx = head_case_names().index(name)
    _, B, Ku, Kv, has_lin, has_bias, labels, misalign, scale = HEAD_CASES[idx]
    r = np.random.default_rng(100003 * idx + 7 * B + 131 * Ku + 17 * Kv)
    K = max(Ku + Kv, 1)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c = dict(name=name, B=B, Ku=Ku, Kv=Kv, misalign=misalign, labels=labels, gloss=np.float32(HEAD_GLOSS[idx % 4]))
    c["u"] = f(r.standard_normal((B, Ku))) if Ku else None
    c["wu"] = f(r.standard_normal((1, Ku)) * scale / np.sqrt(K)) if Ku else None
    c["v"] = f(r.standard_normal((B, Kv))) if Kv else None
    c["wv"] = f(r.standard_normal((1, Kv)) * scale / np.sqrt(K)) if Kv else None
    c["lin"] = f(r.standard_normal(B) * (1.0 if labels != "sat" else 5.0)) if has_lin else None
    c["bias"] = f([0.3 * r.standard_normal()]) if has_bias else None
    if labels == "soft":
        y = r.uniform(0.02, 0.98, B)
    else:
        y = (r.uniform(size=B) < 0.5).astype(np.float64)          # both labels, independent of the logit's side
    c["y"] = f(y)
    return c


# ------------------------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------------------------
def colsum_ref(g, y=None):
    """(sums64 [cols], bound [cols], gz fp32 | None): float64 column sums of g, or of where(y > 0, g, 0)."""
    gz = None
    if y is not None:
        gz = np.where(np.asarray(y) > 0, g, np.float32(0.0)).astype(np.float32)
        g = gz
    rows = g.shape[0]
    s = g.sum(axis=0, dtype=np.float64)
    a = np.abs(g).sum(axis=0, dtype=np.float64)
    return s, gamma(rows) * a, gz


#                rows   cols
COLSUM_SHAPES = [(1, 1), (15, 63), (16, 64), (63, 65), (64, 429), (65, 1000), (1000, 429), (4099, 63), (4099, 1000),
                 (262144, 1), (262144, 64), (262144, 1000), (16, 65600)]


def colsum_pitches(cols):
    """(ld of the plain sum, ldg, ldy): all larger than cols, the two of the ReLU variant different from each other."""
    return cols + 5, cols + 3, cols + 8


def make_colsum_case(rows, cols, relu):
    """fp32 (g [rows][ldg], y [rows][ldy] | None) -- the kernels see the first `cols` columns of each.  y carries exact
    zeros, -0.0 and negative values; the columns beyond `cols` are drawn like the others (a kernel that reads them
    gets a wrong sum)."""
    r = np.random.default_rng(7 * rows + 131 * cols + (1 if relu else 0))
    ld, ldg, ldy = colsum_pitches(cols)
    g = r.standard_normal((rows, ldg if relu else ld), dtype=np.float32)
    if not relu:
        return g, None
    y = r.standard_normal((rows, ldy), dtype=np.float32)
    k = r.integers(0, 8, size=y.shape, dtype=np.int8)
    y[k == 0] = 0.0
    y[k == 1] = -0.0
    return g, y


# ------------------------------------------------------------------------------------------------------------------
# L2
# ------------------------------------------------------------------------------------------------------------------
L2_STRIDE = 32 * 256 * 4      # REG_BLOCKS * REG_THREADS * 4: the elements one grid stride of l2_sumsq_kernel's float4 walk covers
L2_GRAD_STRIDE = 4 * L2_STRIDE  # l2_grad_kernel runs 4 * REG_BLOCKS blocks per tensor
L2_TREE_DEPTH = 56            # 1 fma + 2 (accumulators) + 6 (shuffles) + 2 (waves) + 32 (partials) + 1 (coefficient)
                              # + 4 (T > 256 wrap, T <= 1024 here) + 8 (tree over tensors)
BIG = 2 ** 22 + 3             # 128 strides of the sum's float4 walk, 32 of the gradient's, and a 3-element scalar tail
#           name      T     first tensors: (size, offset in floats)   sizes cycled over the rest     what it is there for
L2_CASES = [
    ("t1",       1,    [(BIG, 0)],                                    []),            # aligned: many float4 strides + scalar tail
    ("t2",       2,    [(L2_STRIDE - 1, 0), (L2_STRIDE + 1, 3)],      []),            # either side of one stride
    ("t2_big",   2,    [(BIG, 0), (2 ** 21 + 1, 3)],                  []),            # float4 walk next to a long scalar walk (the
                                                                                      # second tensor and its gradient are misaligned)
    ("t256",     256,  [],                                            [5, 1, 3, 4]),  # every thread of the finish kernel busy
    ("t257",     257,  [(L2_STRIDE + 1, 0)],                          [4, 5, 1, 3]),  # the T > 256 wrap, one tensor deep
    ("t1000",    1000, [(L2_STRIDE - 1, 0)],                          [3, 4, 5, 1]),  # the wrap, four tensors deep
]


def l2_case(name):
    """dict: sizes, offs (base offset in floats, 0..3, of each tensor inside its own 16-byte aligned slot), coeffs
    (float32; one of them 0 when T > 1), ws (fp32 arrays; one of them all zeros when T > 2), gs (float32).  Tensor 0 is
    never the zero one and, where the case has a large tensor, is that tensor: a finish that loses a tensor shows."""
    idx = [c[0] for c in L2_CASES].index(name)
    _, T, first, cyc = L2_CASES[idx]
    r = np.random.default_rng(977 * T + 13 + idx)
    sizes = [n for n, _ in first] + [cyc[t % len(cyc)] for t in range(T - len(first))]
    offs = [o for _, o in first] + [(t + t // 4) % 4 for t in range(T - len(first))]   # all four offsets against every size
    coeffs = (10.0 ** r.uniform(-5, -2, T)).astype(np.float32)
    ws = [r.standard_normal(n, dtype=np.float32) for n in sizes]
    if T > 1:
        coeffs[T - 1] = 0.0
    if T > 2:
        ws[T // 2][:] = 0.0
    assert sum(sizes) >= L2_TREE_DEPTH + max(sizes) // L2_STRIDE, "the value bound needs numel >= the fixed tree depth"
    return dict(name=name, T=T, sizes=sizes, offs=offs, coeffs=coeffs, ws=ws, gs=np.float32(0.75 + 0.5 * idx))


def l2_value_ref(ws, coeffs):
    """(value64, bound, walk bound): sum_t c_t sum w^2 in float64; gamma(numel) * sum_t |c_t| sum w^2, the bar the value is
    held to as a whole; and the bound that follows from the kernels' own walk, sum_t gamma(d_t) |c_t| sum w_t^2 with
    d_t = ceil(n_t / 8192) + L2_TREE_DEPTH: a thread's chain of fused multiply-adds is at most ceil(n_t / (REG_BLOCKS *
    REG_THREADS)) long (one accumulator on the scalar walk, four on the float4 walk, each a quarter as long), and the
    fixed tree adds L2_TREE_DEPTH roundings.  gamma(numel) is a third of the value at 2^22 elements and cannot see a lost
    stride; the walk bound (3e-5 there) can."""
    per = np.array([float((f64(w) ** 2).sum()) for w in ws])
    c = f64(coeffs)
    sizes = np.array([int(w.size) for w in ws])
    depth = -(-sizes // (32 * 256)) + L2_TREE_DEPTH
    mag = np.abs(c) * per
    return float((c * per).sum()), float(gamma(sizes.sum())) * float(mag.sum()), float((gamma(depth) * mag).sum())


def l2_grad_ref(w32, c32, gs32):
    """The gradient as l2_grad_kernel spells it, in numpy float32: one rounding for sc, one for the product."""
    sc = np.float32(np.float32(np.float32(2.0) * np.float32(c32)) * np.float32(gs32))
    return (sc * np.asarray(w32, dtype=np.float32)).astype(np.float32), sc


def l2_grad_acc_ref(w32, c32, gs32, g32):
    """(reference float64, bound) of accumulate = 1: fma(sc, w, g) has ONE rounding -> within 1 ulp of the float64 value."""
    _, sc = l2_grad_ref(w32, c32, gs32)
    ref = float(sc) * f64(w32) + f64(g32)
    return ref, ulp_bound(ref, 1.0)

