"""CPU: the float64 reference of the batch-norm tests (tests/dnn_bn_ref.py) against torch's own F.batch_norm + activation in
float64 -- forward, running statistics (running_var's unbiased factor included) and autograd -- to 1e-12 relative, and the
block-wise (mean, M2) merge against the one-shot variance."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dnn_bn_ref as B

RTOL = 1e-12
T_ACT = {"linear": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid}


def _inputs(rows, cols, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, cols)) * rng.uniform(0.5, 3.0, cols) + rng.uniform(-2.0, 2.0, cols)
    return dict(z=z, gamma=rng.uniform(0.5, 1.5, cols), beta=rng.standard_normal(cols), g=rng.standard_normal((rows, cols)),
                rm=rng.standard_normal(cols), rv=rng.uniform(0.5, 2.0, cols))


def _close(got, want, what, scale=None):
    """1e-12 relative: of each value, or of `scale` -- the size of the terms a value is the difference of.  dz is
    gamma * rstd * (gm - mean(gm) - xhat * mean(gm * xhat)); over two rows its terms cancel to rounding, and the two float64
    evaluations then agree to 1e-12 of the terms, not of what is left of them."""
    want = np.asarray(want, np.float64)
    atol = RTOL * float(np.abs(want).max() if scale is None else scale)
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=RTOL, atol=atol, err_msg=what)


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("rows,cols", [(2, 1), (3, 5), (65, 33), (200, 7)])
def test_training_reference_equals_torch_float64(rows, cols, act):
    eps, mom = 1e-5, 0.1
    d = _inputs(rows, cols, 10 * rows + cols)
    ref = B.fwd_train(d["z"], d["gamma"], d["beta"], eps, mom, act, d["rm"], d["rv"])
    z, ga, be = (torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("z", "gamma", "beta"))
    rm, rv = torch.tensor(d["rm"]), torch.tensor(d["rv"])
    y = T_ACT[act](F.batch_norm(z, rm, rv, ga, be, True, mom, eps))
    y.backward(torch.tensor(d["g"]))
    _close(ref["y"], y.detach().numpy(), "y")
    _close(ref["running_mean"], rm.numpy(), "running_mean")
    _close(ref["running_var"], rv.numpy(), "running_var (unbiased: var * n / (n - 1))")
    want_rv = 0.9 * d["rv"] + 0.1 * d["z"].var(0, ddof=1)
    _close(ref["running_var"], want_rv, "running_var against numpy's ddof=1")
    dz, dg, db = B.bwd(d["g"], ref["y"], d["z"], d["gamma"], ref["mean"], ref["rstd"], act)
    _close(dz, z.grad.numpy(), "dz", scale=float(np.abs(d["gamma"] * ref["rstd"]).max() * np.abs(d["g"]).max()))
    _close(dg, ga.grad.numpy(), "dgamma")
    _close(db, be.grad.numpy(), "dbeta")


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("rows,cols", [(1, 4), (65, 33)])
def test_evaluation_reference_equals_torch_float64(rows, cols, act):
    eps = 1e-5
    d = _inputs(rows, cols, 7 * rows + cols)
    z, ga, be = (torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("z", "gamma", "beta"))
    rm, rv = torch.tensor(d["rm"]), torch.tensor(d["rv"])
    y = T_ACT[act](F.batch_norm(z, rm, rv, ga, be, False, 0.1, eps))
    y.backward(torch.tensor(d["g"]))
    assert np.array_equal(rm.numpy(), d["rm"]) and np.array_equal(rv.numpy(), d["rv"])
    ref = B.fwd_eval(d["z"], d["gamma"], d["beta"], eps, act, d["rm"], d["rv"])
    _close(ref, y.detach().numpy(), "y")
    dz, dg, db = B.bwd(d["g"], ref, d["z"], d["gamma"], d["rm"], 1.0 / np.sqrt(d["rv"] + eps), act, frozen=True)
    _close(dz, z.grad.numpy(), "dz")
    _close(dg, ga.grad.numpy(), "dgamma")
    _close(db, be.grad.numpy(), "dbeta")


@pytest.mark.parametrize("row_block", [1, 3, 64])
@pytest.mark.parametrize("rows", [2, 3, 63, 64, 65, 197, 1000])
def test_blockwise_merge_equals_the_one_shot_variance(rows, row_block):
    rng = np.random.default_rng(rows + row_block)
    z = rng.standard_normal((rows, 6))
    z[:, 0] += 1000.0                                   # the column the raw sum of squares loses in fp32
    mean, m2 = B.blockwise_mean_m2(z, row_block)
    np.testing.assert_allclose(mean, z.mean(0), rtol=1e-13)
    np.testing.assert_allclose(m2 / rows, z.var(0), rtol=1e-11)
    np.testing.assert_allclose(m2 / (rows - 1), z.var(0, ddof=1), rtol=1e-11)


def test_raw_sums_of_squares_lose_the_shifted_column_in_fp32_and_the_merge_does_not():
    """Why the kernels carry (mean, M2): E[z^2] - mean^2 in fp32 on 1000 + N(0, 1) is off by a large fraction of the variance;
    the same merge run in fp32 keeps it to rounding."""
    rng = np.random.default_rng(5)
    z = (1000.0 + rng.standard_normal(4096)).astype(np.float32)
    true_var = float(z.astype(np.float64).var())
    raw = float(np.float32(np.sum(z * z, dtype=np.float32) / np.float32(z.size)) - np.float32(np.mean(z, dtype=np.float32)) ** 2)
    n, mean, m2 = 0, np.float32(0), np.float32(0)
    for k in range(0, z.size, 64):
        blk = z[k:k + 64]
        bm = np.float32(blk.sum(dtype=np.float32) / np.float32(64))
        bq = np.float32(((blk - bm) ** 2).sum(dtype=np.float32))
        if n == 0:
            n, mean, m2 = 64, bm, bq
            continue
        d = np.float32(bm - mean)
        tot = n + 64
        mean = np.float32(mean + d * np.float32(64.0 / tot))
        m2 = np.float32(m2 + bq + d * d * np.float32(n * 64.0 / tot))
        n = tot
    assert abs(float(m2) / n - true_var) < 1e-4 * true_var
    assert abs(raw - true_var) > 1e-2 * true_var
