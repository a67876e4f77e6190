"""float64 reference and error bounds of the output head with one weight per example (csrc/reg.hip: the WT instances of
head_fwd_kernel / head_bwd_kernel / head_bwd_vec_kernel; C ABI xdfm_head_fwd_w / xdfm_head_bwd_w).  Built on
head_reg_ref.py (error model: eps = 2^-24, gamma(n) = n eps / (1 - n eps), "k rounded operations in a row are within k / 2
ulp", ulp the relative unit 2^-23) and head_ex_ref.py (the mse / mae pairs).  Imported by test_head_w_host.py (CPU),
test_gpu_head_w_abi.py, head_w_drivers.py and test_gpu_sample_weight.py.

The weighted kernels differ from the unweighted ones in two products, each rounded on its own (never fused into the add
or fma that consumes it):
    term_b -> fl(w_b * term_b)          before it joins the running sum of the loss
    g_b    -> fl(w_b * g_b)             the row gradient d loss / d z; dlin, du, dv, dwu, dwv, dbias are formed from it as before
so the staged truth of head_reg_ref / head_ex_ref carries over with ONE more rounding per weighted value:
  pred   untouched by w: head_ex_ref.pred_ref;
  loss   against the float64 sum of w_b term64_b ON THE KERNEL'S OWN fp32 pred, w >= 0, S_w = sum_b w_b |term64_b|:
           mse / mae   gamma(B + k + 1) S_w, k = head_ex_ref.TERM_ROUNDINGS (3 / 1): the roundings of one term, the
                       weighting product, at most B additions; + B (1 + max w) 2^-149 for a square or a product that
                       underflows;
           bce         head_reg_ref's gamma(B) S + 5 eps S + eps sum (1 - t) becomes gamma(B + 6) S_w (the B additions, the 5
                       eps of one term, the weighting product; one gamma, so that the cross terms are covered too)
                       + eps (1 + gamma(B + 1)) sum_b w_b (1 - t_b)  (the absolute error of log(1 - p), weighted and summed)
                       + B 2^-149;
  g      w_b g64_b with g64 the unweighted float64 gradient on the fp32 pred (head_reg_ref.head_g_ref, head_ex_ref.g_ref):
         k + 1 roundings, k = 4 (bce) or head_ex_ref.HEAD_G_ROUNDINGS -> within (k + 1) / 2 ulp.  Where w_b = 0 (and pred is
         finite) the reference is 0 and the bound collapses to the denormal slack: g must be (+-)0, and with it du, dv;
  du, dv, dwu, dwv, dbias   head_reg_ref.head_grads_ref on the kernel's own fp32 g, unchanged.
None of these bars was fitted to what the kernels give.

`head_w64` is the whole weighted head in float64 from the fp32 operands (no staging): what the exact family of
test_gpu_head_w_abi.py must reproduce bit for bit, and what test_head_w_host.py holds against torch's float64 autograd of
sum_b w_b loss_b and against the unweighted head on the batch with every row repeated w_b times."""
import numpy as np

import head_ex_ref as X
import head_reg_ref as R

ALL_MODES = [(X.LINK_SIGMOID, X.LOSS_BCE)] + X.NEW_MODES
G_ROUNDINGS = {(X.LINK_SIGMOID, X.LOSS_BCE): 4, **X.HEAD_G_ROUNDINGS}       # of the unweighted g; the weight adds one


def mode_id(mode):
    return "%s_%s" % (X.LINK_NAMES[mode[0]], X.LOSS_NAMES[mode[1]])


def terms64(pred, t, loss):
    """(terms64 [B], |terms| as the bounds count them [B]) on the given pred."""
    if loss == X.LOSS_BCE:
        p, tt = R.f64(pred).reshape(-1), R.f64(t).reshape(-1)
        with np.errstate(divide="ignore"):
            L1 = np.maximum(np.log(p), -100.0)
            L0 = np.maximum(np.log1p(-p), -100.0)
        return -(tt * L1 + (1.0 - tt) * L0), tt * np.abs(L1) + (1.0 - tt) * np.abs(L0)
    terms = X.loss_ref(pred, t, loss)[2]
    return terms, np.abs(terms)


def loss_w_ref(pred, t, w, loss):
    """(loss64, bound) of the weighted second stage on the given pred (the kernel's own fp32 one)."""
    w = R.f64(w).reshape(-1)
    assert (w >= 0).all()
    terms, mags = terms64(pred, t, loss)
    B = terms.size
    S = float((w * mags).sum())
    wmax = float(w.max()) if B else 0.0
    if loss == X.LOSS_BCE:
        tt = R.f64(t).reshape(-1)
        bound = float(R.gamma(B + 6)) * S + R.EPS * (1.0 + float(R.gamma(B + 1))) * float((w * (1.0 - tt)).sum()) + B * R.TINY
    else:
        bound = float(R.gamma(B + X.TERM_ROUNDINGS[loss] + 1)) * S + B * (1.0 + wmax) * R.TINY
    return float((w * terms).sum()), bound


def g_unweighted64(pred, t, gloss, mode):
    if mode[1] == X.LOSS_BCE:
        return R.head_g_ref(pred, t, gloss)
    return X.g_ref(pred, t, gloss, mode)[0]


def g_w_ref(pred, t, w, gloss, mode):
    """(g64 [B], bound [B]) of the weighted third stage on the given pred."""
    g = R.f64(w).reshape(-1) * g_unweighted64(pred, t, gloss, mode)
    return g, R.ulp_bound(g, (G_ROUNDINGS[mode] + 1) / 2.0)


def head_w64(c, w, mode):
    """The whole head in float64 from the fp32 operands of a case dict (lin, u, wu, v, wv, bias, y, gloss; absent ones
    None) and weights w (None: unweighted) -> dict pred, loss, g (= dlin), du, dv, dwu, dwv, dbias (those present)."""
    link, loss = mode
    B = c["B"]
    z, _, _ = R.head_logits(c["lin"], c["u"], c["wu"], c["v"], c["wv"], c["bias"])
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (B,))
    p = R.sigmoid64(z) if link == X.LINK_SIGMOID else z.copy()
    t = R.f64(c["y"]).reshape(-1)
    ww = np.ones(B) if w is None else R.f64(w).reshape(-1)
    d = p - t
    if loss == X.LOSS_BCE:
        with np.errstate(divide="ignore"):
            terms = -(t * np.maximum(np.log(p), -100.0) + (1.0 - t) * np.maximum(np.log1p(-p), -100.0))
        g = float(c["gloss"]) * d                      # (p - t) / (p (1 - p)) * p (1 - p), unclamped
    else:
        terms = d * d if loss == X.LOSS_MSE else np.abs(d)
        g = float(c["gloss"]) * (2.0 * d if loss == X.LOSS_MSE else np.sign(d))
        if link == X.LINK_SIGMOID:
            g = g * p * (1.0 - p)
    g = ww * g
    out = dict(pred=p, loss=float((ww * terms).sum()), g=g, dbias=float(g.sum()))
    for nm, x, wt in (("u", c["u"], c["wu"]), ("v", c["v"], c["wv"])):
        if x is not None:
            out["d" + nm] = g[:, None] * R.f64(wt).reshape(1, -1)
            out["dw" + nm] = (g[:, None] * R.f64(x)).sum(0)
    return out


def repeat_rows(c, w):
    """The case with row b repeated int(w_b) times (w integral, >= 0): the unweighted head on it is the weighted head on c."""
    reps = np.asarray(w).astype(np.int64).reshape(-1)
    assert np.array_equal(reps, np.asarray(w).reshape(-1)) and (reps >= 0).all() and reps.sum() > 0
    idx = np.repeat(np.arange(c["B"]), reps)
    r = dict(c)
    r["B"] = int(idx.size)
    for k in ("lin", "u", "v", "y"):
        r[k] = None if c[k] is None else np.ascontiguousarray(c[k][idx])
    return r, idx


# ------------------------------------------------------------------------------------------------------------------
# the cases of test_gpu_head_w_abi.py: the vectorised kernels stride 2048 rows per sweep (128 blocks x 16 rows), the scalar
# ones 512; B = 1, a handful, one past a scalar sweep, one past a vector sweep, two vector sweeps and a ragged third
W_BATCHES = [1, 5, 513, 2049, 4100]
W_WIDTHS = [(8, 32), (7, 0), (0, 516)]            # float4 path; scalar by K % 4; scalar by K > 512
W_CASES = [(B, Ku, Kv, full) for B in W_BATCHES for (Ku, Kv) in W_WIDTHS for full in (True, False)]


def w_case_id(case):
    return "b%d_k%d_k%d_%s" % (case[0], case[1], case[2], "linbias" if case[3] else "bare")


def w_vectorised(Ku, Kv):
    return R.head_vectorised(Ku, Kv, None)


def make_w_case(case, link, exact=False):
    """fp32 operands + weights of a case.  exact: small integers everywhere (u, v in {-1, 0, 1}, wu, wv in {-1, 0, 1}, lin,
    bias, y in {-3..3}, gloss = 2, w in {0, 1, 2, 3}) so that, with the identity link, every product and every partial sum is
    an integer (`assert_exact_family` checks the magnitudes).  Otherwise random operands as head_reg_ref draws them and w
    uniform in [0, 4] with about one exact zero in five rows."""
    B, Ku, Kv, full = case
    r = np.random.default_rng(1009 * B + 31 * Ku + 7 * Kv + 3 * int(full) + 101 * link + (5 if exact else 0))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c = dict(name=w_case_id(case), B=B, Ku=Ku, Kv=Kv, misalign=None)
    K = max(Ku + Kv, 1)
    if exact:
        ints = lambda lo, hi, shape: f(r.integers(lo, hi + 1, size=shape))
        c["u"] = ints(-1, 1, (B, Ku)) if Ku else None
        c["wu"] = ints(-1, 1, (1, Ku)) if Ku else None
        c["v"] = ints(-1, 1, (B, Kv)) if Kv else None
        c["wv"] = ints(-1, 1, (1, Kv)) if Kv else None
        c["lin"] = ints(-3, 3, B) if full else None
        c["bias"] = f([2.0]) if full else None
        c["y"] = ints(-3, 3, B)
        c["gloss"] = np.float32(2.0)
        w = ints(0, 3, B)
        w[0] = 2.0                                                # never all zero (B = 1): the repeated batch is not empty
    else:
        c["u"] = f(r.standard_normal((B, Ku))) if Ku else None
        c["wu"] = f(r.standard_normal((1, Ku)) / np.sqrt(K)) if Ku else None
        c["v"] = f(r.standard_normal((B, Kv))) if Kv else None
        c["wv"] = f(r.standard_normal((1, Kv)) / np.sqrt(K)) if Kv else None
        c["lin"] = f(r.standard_normal(B)) if full else None
        c["bias"] = f([0.3 * r.standard_normal()]) if full else None
        if link == X.LINK_IDENTITY:
            c["y"] = f(0.5 + 1.5 * r.standard_normal(B))
        elif full:
            c["y"] = f(r.uniform(0.02, 0.98, B))                  # soft labels
        else:
            c["y"] = f(r.uniform(size=B) < 0.5)                   # hard labels
        c["gloss"] = np.float32([0.37, 1.0, -2.5, 1.75][(B + Ku) % 4])
        w = f(r.uniform(0.0, 4.0, B))
        w[r.uniform(size=B) < 0.2] = 0.0
        if B >= 5:
            w[1] = 0.0
    return c, w


def assert_exact_family(c, w, loss):
    """Every operand an integer and every sum the kernels can form, in any order, below 2^24: all of fp32 arithmetic on
    this case is exact, so the outputs have to equal the float64 reference bit for bit."""
    LIM = 2.0 ** 24
    for k in ("lin", "u", "wu", "v", "wv", "bias", "y"):
        if c[k] is not None:
            assert np.array_equal(c[k], np.round(c[k]))
    assert np.array_equal(w, np.round(w)) and w.min() >= 0 and w.max() <= 3 and float(c["gloss"]) == round(float(c["gloss"]))
    z, A, _ = R.head_logits(c["lin"], c["u"], c["wu"], c["v"], c["wv"], c["bias"])       # A: sum of |terms| of a logit
    assert float(np.max(A)) < LIM, "logit"                                                # so z is exact in any order
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (c["B"],))
    dmax = np.abs(z - R.f64(c["y"]))                                                       # |p - t|, exact
    ww = R.f64(w)
    term = dmax * dmax if loss == X.LOSS_MSE else dmax
    assert float((ww * term).sum()) < LIM, "loss"
    gmax = ww * abs(float(c["gloss"])) * (2.0 * dmax if loss == X.LOSS_MSE else 1.0)
    assert float(gmax.sum()) < LIM, "dbias"
    for x in (c["u"], c["v"]):
        if x is not None:
            assert float((gmax[:, None] * np.abs(R.f64(x))).sum(0).max()) < LIM, "dw"


def autograd_check_w(mode, B=257, seed=0):
    """Largest difference, relative to the scale of each quantity, between head_w64 and torch's float64 autograd of
    gloss * sum_b w_b loss(pred_b, y_b): (loss, g, dwu, dbias)."""
    import torch
    F = torch.nn.functional
    link, loss = mode
    c, w = make_w_case((B, 8, 32, True), link)
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    wu, bias, lin = T(c["wu"]).requires_grad_(True), T(c["bias"]).requires_grad_(True), T(c["lin"]).requires_grad_(True)
    z = lin + (T(c["u"]) * wu).sum(1) + (T(c["v"]) * T(c["wv"])).sum(1) + bias
    p = torch.sigmoid(z) if link == X.LINK_SIGMOID else z
    fn = {X.LOSS_BCE: F.binary_cross_entropy, X.LOSS_MSE: F.mse_loss, X.LOSS_MAE: F.l1_loss}[loss]
    L = (T(w) * fn(p, T(c["y"]), reduction="none")).sum()
    (float(c["gloss"]) * L).backward()
    ref = head_w64(c, w, mode)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(float(np.abs(np.asarray(b)).max()), 1.0)
    return (rel(ref["loss"], L.item()), rel(ref["g"], lin.grad.numpy()), rel(ref["dwu"], wu.grad.numpy().reshape(-1)),
            rel(ref["dbias"], bias.grad.numpy()))
