"""What the synchronised batch-norm tests share: a float64 numpy mirror of the split the kernels of csrc/bn.hip make for
row-parallel training -- per-shard (count, mean, M2) triples, their Chan merge in rank order, the apply over the global
statistics, the per-shard backward sums and the backward over their rank-order totals -- with a shard that holds only a
stand-in row (count 0, dz = 0).  No GPU needed; checked against torch in tests/test_dnn_bn_sync_reference.py."""
import numpy as np

import dnn_bn_ref as B


def shards_of(t, sizes):
    """Rows of the global batch `t` per rank for the counts `sizes`; a rank with count 0 holds row 0 as a stand-in
    (dist.RowParallel.shard)."""
    t = np.asarray(t)
    assert sum(sizes) == t.shape[0], (sizes, t.shape)
    out, lo = [], 0
    for s in sizes:
        out.append(t[lo:lo + s] if s > 0 else t[0:1])
        lo += s
    return out


def stats(z):
    """(mean, M2) per column of one shard's rows (what xdfm_bn_stats leaves)."""
    z = np.asarray(z, np.float64)
    mean = z.mean(0)
    return mean, ((z - mean) ** 2).sum(0)


def merge_ranks(triples):
    """(n, mean, M2) of the global batch: the ranks' (count, mean, M2) merged in rank order, count 0 skipped."""
    s = (0, None, None)
    for t in triples:
        s = B.merge(s, t)
    return s


def fwd(z_shards, counts, gamma, beta, eps, momentum, act, running_mean, running_var):
    """dict(y (per shard), mean, rstd, running_mean, running_var, n): every shard normalised with the merged statistics;
    a stand-in's y too."""
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    triples = [(c,) + stats(z) for z, c in zip(z_shards, counts)]
    n, mean, m2 = merge_ranks(triples)
    assert n == sum(counts) and n >= 2
    rstd = 1.0 / np.sqrt(m2 / n + eps)
    y = [B.act_fwd(gamma * ((np.asarray(z, np.float64) - mean) * rstd) + beta, act) for z in z_shards]
    rm = (1.0 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
    rv = (1.0 - momentum) * np.asarray(running_var, np.float64) + momentum * m2 / (n - 1.0)
    return dict(y=y, mean=mean, rstd=rstd, running_mean=rm, running_var=rv, n=n)


def bwd_sums(g, y, z, mean, rstd, act):
    """(sum gm, sum gm * xhat) over one shard's rows (what xdfm_bn_bwd_sums leaves)."""
    g, y, z, mean, rstd = (np.asarray(t, np.float64) for t in (g, y, z, mean, rstd))
    gm = B.act_bwd(y, g, act)
    return gm.sum(0), (gm * ((z - mean) * rstd)).sum(0)


def bwd_apply(g, y, z, all_sums, rank, n_total, gamma, mean, rstd, act, counted):
    """(dz, dgamma, dbeta) of rank `rank`: dz over the rank-order totals of `all_sums` [(s1, s2) per rank] -- zeros for a
    stand-in (counted false) -- and the rank's OWN sums as dgamma, dbeta."""
    g, y, z, gamma, mean, rstd = (np.asarray(t, np.float64) for t in (g, y, z, gamma, mean, rstd))
    s1 = np.zeros_like(mean)
    s2 = np.zeros_like(mean)
    for a, b in all_sums:
        s1 = s1 + a
        s2 = s2 + b
    if counted:
        gm = B.act_bwd(y, g, act)
        dz = gamma * rstd * (gm - s1 / n_total - ((z - mean) * rstd) * s2 / n_total)
    else:
        dz = np.zeros_like(z)
    return dz, all_sums[rank][1], all_sums[rank][0]


def bwd(g_shards, y_shards, z_shards, counts, gamma, mean, rstd, act):
    """[(dz, dgamma, dbeta) per rank] through bwd_sums / bwd_apply."""
    sums = [bwd_sums(g, y, z, mean, rstd, act) for g, y, z in zip(g_shards, y_shards, z_shards)]
    n = sum(counts)
    return [bwd_apply(g, y, z, sums, r, n, gamma, mean, rstd, act, counts[r] > 0)
            for r, (g, y, z) in enumerate(zip(g_shards, y_shards, z_shards))]
