"""CPU: the float64 mirror of the synchronised batch norm (tests/bn_sync_ref.py) against torch.  Rows split into shards --
a one-row shard and a count-0 stand-in among them -- must reproduce float64 F.batch_norm + activation and its autograd on
the concatenated rows to 1e-12: y, the running statistics, dz on the counted rows, the sums of the local dgamma and dbeta;
and the stand-in's dz must be zeros."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_sync_ref as S
import dnn_bn_ref as B

EPS, MOM = 1e-5, 0.1
TOL = 1e-12
T_ACT = {"linear": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid}
SPLITS = [(67, 1, 0, 127), (70,), (1, 1), (0, 5, 0, 3), (33, 32)]


def _draw(n, cols, seed):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n, cols, generator=gen, dtype=torch.float64) * (0.5 + 2.5 * torch.rand(cols, generator=gen, dtype=torch.float64))
    z = z + 2.0 * torch.randn(cols, generator=gen, dtype=torch.float64)
    z[:, 0] = 1000.0 + torch.randn(n, generator=gen, dtype=torch.float64)
    # the shards' statistics differ: the rows drift with their index
    z = z + torch.linspace(0.0, 3.0, n, dtype=torch.float64)[:, None]
    g = torch.randn(n, cols, generator=gen, dtype=torch.float64)
    gamma = 0.5 + torch.rand(cols, generator=gen, dtype=torch.float64)
    beta = 0.5 * torch.randn(cols, generator=gen, dtype=torch.float64)
    rm = torch.randn(cols, generator=gen, dtype=torch.float64)
    rv = 0.5 + 1.5 * torch.rand(cols, generator=gen, dtype=torch.float64)
    return z, g, gamma, beta, rm, rv


def _close(got, want, what, scale=1.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max())
    assert err <= TOL * scale, (what, err)


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("sizes", SPLITS, ids=["-".join(map(str, s)) for s in SPLITS])
def test_shards_reproduce_float64_batch_norm_of_the_concatenated_rows(sizes, act):
    n, cols = sum(sizes), 7
    z, g, gamma, beta, rm, rv = _draw(n, cols, 100 + n)
    zt, gt, bt = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    rm_t, rv_t = rm.clone(), rv.clone()
    y_t = T_ACT[act](F.batch_norm(zt, rm_t, rv_t, gt, bt, True, MOM, EPS))
    y_t.backward(g)

    zs, gs = S.shards_of(z.numpy(), sizes), S.shards_of(g.numpy(), sizes)
    gs = [x if c > 0 else np.zeros_like(x) for x, c in zip(gs, sizes)]            # a stand-in's root gradient is zero
    f = S.fwd(zs, sizes, gamma.numpy(), beta.numpy(), EPS, MOM, act, rm.numpy(), rv.numpy())
    assert f["n"] == n
    y_counted = np.concatenate([y for y, c in zip(f["y"], sizes) if c > 0])
    _close(y_counted, y_t.detach().numpy(), "y")
    _close(f["running_mean"], rm_t.numpy(), "running_mean")
    _close(f["running_var"], rv_t.numpy(), "running_var")
    for r, c in enumerate(sizes):
        if c == 0:          # the stand-in is row 0 normalised with the global statistics
            _close(f["y"][r], y_t.detach().numpy()[0:1], "stand-in y")
    out = S.bwd(gs, f["y"], zs, sizes, gamma.numpy(), f["mean"], f["rstd"], act)
    dz_counted = np.concatenate([o[0] for o, c in zip(out, sizes) if c > 0])
    _close(dz_counted, zt.grad.numpy(), "dz")
    _close(sum(o[1] for o in out), gt.grad.numpy(), "sum of the local dgamma")
    _close(sum(o[2] for o in out), bt.grad.numpy(), "sum of the local dbeta")
    for o, c in zip(out, sizes):
        if c == 0:
            assert o[0].shape == (1, cols) and not o[0].any(), "a stand-in's dz must be zeros"
            assert not o[1].any() and not o[2].any()


def test_a_stand_in_with_a_live_gradient_would_leak_without_the_zeroing():
    """Why the flag exists: with the other ranks' sums in S1 / S2 the plain formula gives a stand-in row a non-zero dz even
    though its own gradient is zero."""
    sizes = (5, 0, 4)
    z, g, gamma, beta, rm, rv = _draw(9, 3, 5)
    zs, gs = S.shards_of(z.numpy(), sizes), S.shards_of(g.numpy(), sizes)
    gs[1] = np.zeros_like(gs[1])
    f = S.fwd(zs, sizes, gamma.numpy(), beta.numpy(), EPS, MOM, "linear", rm.numpy(), rv.numpy())
    sums = [S.bwd_sums(a, y, x, f["mean"], f["rstd"], "linear") for a, y, x in zip(gs, f["y"], zs)]
    leaky = S.bwd_apply(gs[1], f["y"][1], zs[1], sums, 1, 9, gamma.numpy(), f["mean"], f["rstd"], "linear", True)[0]
    assert np.abs(leaky).max() > 1e-3
    assert not S.bwd_apply(gs[1], f["y"][1], zs[1], sums, 1, 9, gamma.numpy(), f["mean"], f["rstd"], "linear", False)[0].any()


def test_merge_in_rank_order_equals_the_statistics_of_all_rows():
    z = _draw(200, 5, 9)[0].numpy()
    for sizes in [(64, 1, 0, 135), (200,), (0, 0, 200), (1, 199)]:
        n, mean, m2 = S.merge_ranks([(c,) + S.stats(x) for x, c in zip(S.shards_of(z, sizes), sizes)])
        assert n == 200
        _close(mean, z.mean(0), "mean", scale=float(np.abs(z.mean(0)).max()))      # relative: column 0 lies at 1000
        _close(m2, ((z - z.mean(0)) ** 2).sum(0), "M2", scale=float(((z - z.mean(0)) ** 2).sum(0).max()))
