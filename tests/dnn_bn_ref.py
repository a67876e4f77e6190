"""What the batch-norm tests (csrc/bn.hip) share: a float64 numpy reference of act(batch_norm(z)) -- training forward with
the running statistics, evaluation forward, backward for the three activations -- and the block-wise (mean, M2) merge the
kernels use, restated in float64.  No GPU needed; checked against torch in tests/test_dnn_bn_reference.py."""
import numpy as np

ACTS = ("linear", "relu", "sigmoid")


def act_fwd(v, act):
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    assert act == "linear", act
    return v


def act_bwd(y, g, act):
    """gm = act'(y) * g from the stored output y."""
    if act == "relu":
        return np.where(y > 0, g, 0.0)
    if act == "sigmoid":
        return g * y * (1.0 - y)
    assert act == "linear", act
    return g


def fwd_train(z, gamma, beta, eps, momentum, act, running_mean, running_var):
    """dict(y, xhat, mean, rstd, running_mean, running_var): batch statistics over the rows (biased variance for y, unbiased
    for running_var, as nn.BatchNorm1d)."""
    z, gamma, beta = (np.asarray(t, np.float64) for t in (z, gamma, beta))
    n = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (z - mean) * rstd
    y = act_fwd(gamma * xhat + beta, act)
    rm = (1.0 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
    rv = (1.0 - momentum) * np.asarray(running_var, np.float64) + momentum * var * n / (n - 1.0)
    return dict(y=y, xhat=xhat, mean=mean, rstd=rstd, running_mean=rm, running_var=rv)


def fwd_eval(z, gamma, beta, eps, act, running_mean, running_var):
    z, gamma, beta, rm, rv = (np.asarray(t, np.float64) for t in (z, gamma, beta, running_mean, running_var))
    return act_fwd(gamma * (z - rm) / np.sqrt(rv + eps) + beta, act)


def bwd(g, y, z, gamma, mean, rstd, act, frozen=False):
    """(dz, dgamma, dbeta) from the stored output y (its values decide the ReLU mask and the sigmoid slope, as in the kernel)
    and the saved statistics.  frozen: the statistics were constants of the forward (evaluation mode)."""
    g, y, z, gamma, mean, rstd = (np.asarray(t, np.float64) for t in (g, y, z, gamma, mean, rstd))
    n = z.shape[0]
    gm = act_bwd(y, g, act)
    xhat = (z - mean) * rstd
    s1, s2 = gm.sum(0), (gm * xhat).sum(0)
    if frozen:
        dz = gamma * rstd * gm
    else:
        dz = gamma * rstd * (gm - s1 / n - xhat * s2 / n)
    return dz, s2, s1


def merge(a, b):
    """Chan's formula: (n, mean, M2) of A followed by B."""
    na, ma, qa = a
    nb, mb, qb = b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    d = mb - ma
    return n, ma + d * nb / n, qa + qb + d * d * na * nb / n


def blockwise_mean_m2(z, row_block):
    """(mean, M2) per column by the kernels' plan: one pair per block of `row_block` rows; four runs of consecutive blocks
    merged in index order, then (0 + 1) + (2 + 3)."""
    z = np.asarray(z, np.float64)
    rows = z.shape[0]
    nrb = -(-rows // row_block)
    parts = []
    for k in range(nrb):
        blk = z[k * row_block:(k + 1) * row_block]
        m = blk.mean(0)
        parts.append((blk.shape[0], m, ((blk - m) ** 2).sum(0)))
    per = -(-nrb // 4)
    zero = (0, np.zeros(z.shape[1]), np.zeros(z.shape[1]))
    q = []
    for rg in range(4):
        s = zero
        for k in range(rg * per, min((rg + 1) * per, nrb)):
            s = merge(s, parts[k])
        q.append(s)
    n, mean, m2 = merge(merge(q[0], q[1]), merge(q[2], q[3]))
    assert n == rows
    return mean, m2
