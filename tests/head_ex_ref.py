"""float64 references and error bounds of the output head's link / loss pairs beyond (sigmoid, bce): the regression task
(identity link) and the mse / mae losses (csrc/reg.hip: head_link, head_term, head_g; C ABI xdfm_head_fwd_ex /
xdfm_head_bwd_ex).  Built on head_reg_ref.py's helpers and error model: eps = 2^-24, gamma(n) = n eps / (1 - n eps) bounds
the product of n factors (1 + delta), |delta| <= eps; "k rounded operations in a row are within k / 2 ulp", ulp the
relative unit 2^-23.  Imported by test_head_ex_host.py (CPU), test_gpu_head_ex.py and head_ex_drivers.py.

The kernels spell, with z the fp32 logit of head_reg_ref (dot products and adds in any order), t = y[b], gl = gloss[0]:
    p    = 1 / (1 + expf(-z))     (sigmoid link)          p = z     (identity link)
    d    = fl(p - t)
    term = fl(d * d)  (mse)       |d|  (mae)              added to a running sum; d * d may be fused into that add
    s    = fl(2 d) = 2 d exactly  (mse)                   sgn(d) in {-1, 0, 1}, sgn(0) = 0  (mae)
    g    = fl(fl(gl * s) * fl(fl(1 - p) * p))  (sigmoid)  fl(gl * s)  (identity)
As in head_reg_ref the truth is staged, so that every stage is held to its own rounding only:
  pred   sigmoid: head_reg_ref.head_pred_ref (0.25 gamma(n) A_b + 4 eps p64).  identity: against z64, the float64 sum
         of the fp32 operands: |z - z64| <= gamma(n) A_b (A_b the sum of the absolute terms of row b, n their number);
  loss   against the float64 sum of (p - t)^2 or |p - t| ON THE KERNEL'S OWN fp32 pred.  A term carries the rounding of
         d and, for mse, its square's two factors and the product (3 in all, 1 for mae); the B addends at most B more
         on any path: |loss - loss64| <= gamma(B + 3) S (mse), gamma(B + 1) S (mae), S = sum of the float64 terms,
         + B * 2^-149 for a square that underflows.  All terms zero -> the loss is exactly 0;
  g      in float64 on the fp32 pred, gl 2 (p - t) p (1 - p) etc.  Roundings: d, gl * s, 1 - p, its product with p, the
         last product = 5 for (sigmoid, mse); sgn(d) is exact (a correctly rounded difference has the sign of the exact
         one) and so is gl * sgn(d): 3 for (sigmoid, mae); d and gl * s = 2 for (identity, mse); none for (identity, mae),
         held to 1 (half an ulp).  dlin is within k / 2 ulp of g (+ k denormal steps), HEAD_G_ROUNDINGS below;
         where d = 0 the reference is 0 and the bound collapses to the denormal slack, so g must be (+-)0;
  du, dv, dwu, dwv, dbias   head_reg_ref.head_grads_ref on the kernel's own fp32 g, unchanged.
None of these bars was fitted to what the kernels give.
"""
import numpy as np

import head_reg_ref as R

LINK_SIGMOID, LINK_IDENTITY = 0, 1
LOSS_BCE, LOSS_MSE, LOSS_MAE = 0, 1, 2
LINK_NAMES = {LINK_SIGMOID: "sigmoid", LINK_IDENTITY: "identity"}
LOSS_NAMES = {LOSS_BCE: "bce", LOSS_MSE: "mse", LOSS_MAE: "mae"}
NEW_MODES = [(LINK_SIGMOID, LOSS_MSE), (LINK_SIGMOID, LOSS_MAE), (LINK_IDENTITY, LOSS_MSE), (LINK_IDENTITY, LOSS_MAE)]
HEAD_G_ROUNDINGS = {(LINK_SIGMOID, LOSS_MSE): 5, (LINK_SIGMOID, LOSS_MAE): 3, (LINK_IDENTITY, LOSS_MSE): 2,
                    (LINK_IDENTITY, LOSS_MAE): 1}
TERM_ROUNDINGS = {LOSS_MSE: 3, LOSS_MAE: 1}

# both kernel families, both B = 1 cases, a ragged stride, the LDS limit, 32 strides and the misaligned fall-back
EX_CASES = ["c0000", "c0010", "c1111", "k3_k4_b16", "k3_k1_b1", "k64_k60_b1", "k4_k68_b2047", "k516_k64_b2049",
            "k200_k512_b4099", "k4000_k95_b16", "k64_k4_b65536", "k64_k64_u_off"]


def mode_id(mode):
    return "%s_%s" % (LINK_NAMES[mode[0]], LOSS_NAMES[mode[1]])


def make_ex_case(name, link):
    """head_reg_ref.make_head_case(name) for a link.  Identity: y is replaced by real-valued targets (seeded from the
    case).  c0010 (z = lin exactly): every third row gets y[b] = lin[b], which for the identity link is p - t = 0: a
    zero term and sgn(0) = 0; for the sigmoid link the rows b % 3 == 1 get lin[b] = 0 and y[b] = 1/2 to the same end
    (1 / (1 + expf(-0)) is exactly 1/2)."""
    c = R.make_head_case(name)
    B = c["B"]
    if link == LINK_IDENTITY:
        r = np.random.default_rng(7919 * R.head_case_names().index(name) + B)
        c["y"] = (0.5 + 1.5 * r.standard_normal(B)).astype(np.float32)
        c["labels"] = "real"
    if name == "c0010":
        c["y"] = c["y"].copy()
        c["y"][0::3] = c["lin"][0::3]
        if link == LINK_SIGMOID:
            c["lin"] = c["lin"].copy()
            c["lin"][1::3] = 0.0
            c["y"][1::3] = 0.5
    return c


def pred_ref(c, link):
    """(p64 [B], bound [B]) of the first stage."""
    args = (c["lin"], c["u"], c["wu"], c["v"], c["wv"], c["bias"])
    if link == LINK_SIGMOID:
        return R.head_pred_ref(*args, c["B"])
    z, A, n = R.head_logits(*args)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (c["B"],))
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), (c["B"],))
    return z, R.gamma(max(n, 1)) * A


def loss_ref(pred, t, loss):
    """(loss64, bound, terms64 [B]) of the second stage, on the given pred (the kernel's fp32 one, or any float64)."""
    p, t = R.f64(pred).reshape(-1), R.f64(t).reshape(-1)
    d = p - t
    terms = d * d if loss == LOSS_MSE else np.abs(d)
    S = float(terms.sum())
    return S, float(R.gamma(p.size + TERM_ROUNDINGS[loss])) * S + p.size * R.TINY * (loss == LOSS_MSE), terms


def g_ref(pred, t, gloss, mode):
    """(g64 [B], bound [B]) of the third stage: gloss * d loss / d z on the given pred."""
    link, loss = mode
    p, t = R.f64(pred).reshape(-1), R.f64(t).reshape(-1)
    d = p - t
    s = 2.0 * d if loss == LOSS_MSE else np.sign(d)
    g = float(gloss) * s
    if link == LINK_SIGMOID:
        g = g * (p * (1.0 - p))
    return g, R.ulp_bound(g, HEAD_G_ROUNDINGS[mode] / 2.0)


def autograd_check(mode, B=257, seed=0):
    """Largest difference, relative to the scale of each quantity, between the references above evaluated in float64 and
    torch's float64 autograd of F.mse_loss / F.l1_loss(reduction='sum') over sigmoid / identity: (loss, g)."""
    import torch
    link, loss = mode
    r = np.random.default_rng(seed + 10 * link + loss)
    z = r.standard_normal(B) * 2.0
    t = r.uniform(0.0, 1.0, B) if link == LINK_SIGMOID else 0.5 + 1.5 * r.standard_normal(B)
    t[::5] = (1.0 / (1.0 + np.exp(-z[::5]))) if link == LINK_SIGMOID else z[::5]      # exact zeros of p - t for identity
    gloss = -1.75
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    p = torch.sigmoid(zt) if link == LINK_SIGMOID else zt
    fn = torch.nn.functional.mse_loss if loss == LOSS_MSE else torch.nn.functional.l1_loss
    L = fn(p, torch.tensor(t, dtype=torch.float64), reduction="sum")
    (gloss * L).backward()
    p64 = p.detach().numpy()
    l64, _, _ = loss_ref(p64, t, loss)
    g64, _ = g_ref(p64, t, gloss, mode)
    dl = abs(l64 - L.item()) / max(abs(L.item()), 1.0)
    dg = float(np.abs(g64 - zt.grad.numpy()).max()) / max(float(np.abs(zt.grad.numpy()).max()), 1.0)
    return dl, dg
