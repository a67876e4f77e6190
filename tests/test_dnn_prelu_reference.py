"""CPU: the float64 reference and the integer case builders of tests/dnn_prelu_ref.py, checked before the GPU tests lean on
them: the reference against float64 autograd of F.linear + F.prelu, and every integer case against its exactness condition."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dnn_prelu_ref as R


@pytest.mark.parametrize("alpha", R.ALPHAS + (-0.3,))
def test_reference_equals_float64_autograd(alpha):
    gen = torch.Generator().manual_seed(int(100 * abs(alpha)) + 3)
    x = torch.randn(37, 11, generator=gen, dtype=torch.float64, requires_grad=True)
    W = torch.randn(8, 11, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn(8, generator=gen, dtype=torch.float64, requires_grad=True)
    a = torch.tensor([alpha], dtype=torch.float64, requires_grad=True)
    g = torch.randn(37, 8, generator=gen, dtype=torch.float64)
    with torch.no_grad():                                 # cells at exactly zero: the alpha branch, nothing added to dalpha
        b[0] = 0.0
        x[5].zero_()
    z = F.linear(x, W, b)
    y = F.prelu(z, a)
    y.backward(g)
    xn, Wn, bn, gn = (t.detach().numpy() for t in (x, W, b, g))
    y_ref, z_ref = R.layer_ref(xn, Wn, bn, alpha)
    assert (z_ref[5, 0] == 0.0) and np.array_equal(z_ref, z.detach().numpy())
    np.testing.assert_array_equal(y_ref, y.detach().numpy())
    dx, dW, db, da = R.layer_bwd_ref(gn, z_ref, alpha, xn, Wn)
    np.testing.assert_allclose(dx, x.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(dW, W.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(db, b.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(da, a.grad.item(), rtol=1e-13, atol=1e-13)
    # the elementwise op alone
    u = torch.from_numpy(z_ref).requires_grad_(True)
    a2 = torch.tensor([alpha], dtype=torch.float64, requires_grad=True)
    F.prelu(u, a2).backward(g)
    du, da2 = R.prelu_bwd_ref(gn, z_ref, alpha)
    np.testing.assert_array_equal(du, u.grad.numpy())
    np.testing.assert_allclose(da2, a2.grad.item(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("name", sorted(R.DENSE_CASES))
def test_integer_layer_cases_are_exact(name):
    rows, k, out = R.DENSE_CASES[name]
    x, W, b, g = R.int_layer_case(rows, k, out)
    for a in (x, W, b, g):
        assert a.dtype == np.float32 and np.array_equal(a, np.round(a))
    ex = R.exactness(x, W, b, g)
    assert max(ex.values()) < R.EXACT_LIMIT, ex
    z = x.astype(np.int64) @ W.astype(np.int64).T + b.astype(np.int64)
    assert R.has_all_signs(z)
    # the float64 reference is exact, and so is its rounding to fp32, for every slope of the table
    for alpha in R.ALPHAS:
        y, z64 = R.layer_ref(x, W, b, alpha)
        assert np.array_equal(z64, z)
        for t in (y,) + R.layer_bwd_ref(g, z64, alpha, x, W)[:3]:
            assert np.array_equal(t * R.UNIT, np.round(t * R.UNIT)) and np.abs(t * R.UNIT).max() < R.EXACT_LIMIT
        da = R.layer_bwd_ref(g, z64, alpha, x, W)[3]
        assert da == int(da) and abs(da) < R.EXACT_LIMIT and float(np.float32(da)) == da


@pytest.mark.parametrize("shape", R.ELEMENTWISE_CASES, ids=lambda s: "%dx%d" % s)
def test_integer_elementwise_cases_are_exact(shape):
    u, g = R.int_elementwise_case(*shape)
    assert u.dtype == np.float32 and np.array_equal(u, np.round(u)) and np.array_equal(g, np.round(g))
    assert u.size < 3 or R.has_all_signs(u)
    assert R.UNIT * int(np.abs(g.astype(np.int64) * u.astype(np.int64)).sum()) < R.EXACT_LIMIT
    for alpha in R.ALPHAS:
        du, da = R.prelu_bwd_ref(g, u, alpha)
        assert np.array_equal(du * R.UNIT, np.round(du * R.UNIT)) and float(np.float32(da)) == da


def test_dalpha_bound_is_at_least_one_ulp():
    g, z = np.ones((4, 4), np.float32), -np.ones((4, 4), np.float32)
    assert R.dalpha_bound(g, z, -16.0) >= R.ulp32(-16.0) > 0
    assert R.ulp32(0.0) > 0
