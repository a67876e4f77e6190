"""K11 (csrc/compact.hip) at the C ABI against numpy: the positive rows of a batch, moved to the front of capacity-sized
outputs in torch.nonzero's order with the count on the device, and the backward that hands the decoder input its full
gradient.  Everything K11 does is a selection and a copy, so every comparison is exact; inv_n is one division (1 ulp)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _labels(kind, B, rng):
    if kind == "none":
        return np.zeros(B, np.float32)
    if kind == "all":
        return np.ones(B, np.float32)
    y = (rng.random(B) < 0.3).astype(np.float32)
    y[rng.integers(0, B)] = 1.0
    if B > 1:
        y[(int(np.argmax(y)) + 1) % B] = 0.0
    return y


def _run(B, W, F, y, positive_only, dev, pad=3, misalign=0, seed=0):
    """(outputs of the forward, gradient of the backward, inputs) through the C ABI; X has `pad` unused columns behind its own
    (a row stride wider than its columns), `misalign` floats shift dnn_in / d_rows / g off a 16-byte boundary."""
    from xdfm_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(seed + 7 * B + W + F)
    xcols = F + 2
    Xn = np.concatenate([rng.integers(0, 1000, (B, F)).astype(np.float32) + 0.25, rng.random((B, 2), np.float32)], axis=1)
    Xw = np.full((B, xcols + pad), np.nan, np.float32)
    Xw[:, :xcols] = Xn
    dn = rng.standard_normal((B, W)).astype(np.float32)
    gn = rng.standard_normal((B, W)).astype(np.float32)
    cols_n = rng.permutation(F).astype(np.int32)                    # the id columns in any order
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def shifted(a):                                                  # the array in a buffer that starts `misalign` floats late
        flat = torch.empty(a.size + misalign, dtype=torch.float32, device=dev)
        v = flat[misalign:].view(a.shape)
        v.copy_(torch.from_numpy(a))
        return v
    X, d_in, g = torch.from_numpy(Xw).to(dev), shifted(dn), shifted(gn)
    yt, cols = torch.from_numpy(y).to(dev), torch.from_numpy(cols_n).to(dev)
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    pos, n_rows = torch.full((B,), -7, **i32), torch.full((1,), -7, **i32)
    inv_n, valid, labels = torch.full((1,), np.nan, **f32), torch.full((B,), np.nan, **f32), torch.full((B,), np.nan, **f32)
    d_rows = shifted(np.full((B, W), np.nan, np.float32))
    targets = torch.full((F, B), -7, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.xdfm_compact_rows_fwd(P(X), X.stride(0), xcols, P(d_in), W, P(yt), B, W, P(cols), F, int(positive_only), P(pos),
                                         P(n_rows), P(inv_n), P(valid), P(d_rows), P(labels), P(targets), stream), "compact_rows_fwd")
    d_dnn = torch.full((B, W), np.nan, **f32)
    _lib.check(lib.xdfm_compact_rows_bwd(P(g), W, P(pos), B, W, P(d_dnn), stream), "compact_rows_bwd")
    torch.cuda.synchronize()
    got = dict(pos=pos, n_rows=n_rows, inv_n=inv_n, valid=valid, labels=labels, d_rows=d_rows, targets=targets, d_dnn=d_dnn)
    return {k: v.cpu().numpy() for k, v in got.items()}, dict(X=Xn, dnn_in=dn, g=gn, cols=cols_n)


def _check(got, inp, y, positive_only):
    B, W = inp["dnn_in"].shape
    F = inp["cols"].size
    rows = np.nonzero(y == 1)[0] if positive_only else np.arange(B)          # torch.nonzero's order: ascending
    n = rows.size
    assert got["n_rows"][0] == n
    want_inv = np.float32(1.0) / (np.float32(n) + np.float32(1e-8)) if positive_only else np.float32(1.0) / np.float32(B)
    assert abs(float(got["inv_n"][0]) - float(want_inv)) <= float(np.spacing(want_inv)), (got["inv_n"], want_inv)
    pos = np.full(B, -1, np.int32)
    pos[rows] = np.arange(n, dtype=np.int32)
    np.testing.assert_array_equal(got["pos"], pos)
    np.testing.assert_array_equal(got["valid"], (np.arange(B) < n).astype(np.float32))
    d_rows = np.zeros((B, W), np.float32)
    d_rows[:n] = inp["dnn_in"][rows]
    np.testing.assert_array_equal(got["d_rows"], d_rows)
    assert not np.signbit(got["d_rows"][n:]).any()                             # exact (positive) zeros behind the count
    labels = np.zeros(B, np.float32)
    labels[:n] = y[rows]
    np.testing.assert_array_equal(got["labels"], labels)
    targets = np.zeros((F, B), np.int64)
    targets[:, :n] = inp["X"][rows][:, inp["cols"]].astype(np.int64).T
    np.testing.assert_array_equal(got["targets"], targets)
    # backward: index_select's backward of a float64 twin, cast to fp32
    d64 = torch.from_numpy(inp["dnn_in"]).double().requires_grad_(True)
    sel = d64.index_select(0, torch.from_numpy(rows.astype(np.int64)))
    (sel * torch.from_numpy(inp["g"][:n]).double()).sum().backward()
    np.testing.assert_array_equal(got["d_dnn"], d64.grad.float().numpy())


@pytest.mark.parametrize("kind", ["none", "all", "mixed"])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("W", [5, 429])
@pytest.mark.parametrize("B", [1, 31, 64, 65, 1024, 5000])
def test_compact_rows_vs_numpy(B, W, F, kind):
    dev = _dev()
    y = _labels(kind, B, np.random.default_rng(B + W))
    got, inp = _run(B, W, F, y, True, dev)
    _check(got, inp, y, True)


@pytest.mark.parametrize("B,W,misalign", [(65, 432, 0), (1500, 8, 0), (65, 432, 1), (1500, 8, 2)])
def test_compact_rows_vector_path_and_its_alignment_guard(B, W, misalign):
    """W a multiple of 4 on 16-byte aligned buffers moves float4; the same shapes from buffers that start 4 or 8 bytes off take
    the element path (the host chooses by address)."""
    dev = _dev()
    y = _labels("mixed", B, np.random.default_rng(B))
    got, inp = _run(B, W, 2, y, True, dev, misalign=misalign)
    _check(got, inp, y, True)


@pytest.mark.parametrize("B,W", [(65, 5), (1024, 12)])
def test_compact_rows_all_rows_mode(B, W):
    """positive_only = 0: every row is selected whatever its label, inv_n = 1 / B."""
    dev = _dev()
    y = _labels("mixed", B, np.random.default_rng(B))
    got, inp = _run(B, W, 2, y, False, dev)
    _check(got, inp, y, False)


def test_compact_rows_largest_batch():
    """B = 65536, the documented maximum: 64 tiles of the single-workgroup scan."""
    dev = _dev()
    B = 65536
    y = _labels("mixed", B, np.random.default_rng(1))
    got, inp = _run(B, 5, 1, y, True, dev)
    _check(got, inp, y, True)


def test_compact_rows_autograd_function():
    """ops.compact_rows: the same values through the autograd Function; only d_rows carries a gradient."""
    from xdfm_amd import ops
    dev = _dev()
    B, W, F = 200, 13, 2
    rng = np.random.default_rng(5)
    y = _labels("mixed", B, rng)
    Xn = np.concatenate([rng.integers(0, 50, (B, F)).astype(np.float32), rng.random((B, 1), np.float32)], axis=1)
    dn = rng.standard_normal((B, W)).astype(np.float32)
    X, yt = torch.from_numpy(Xn).to(dev), torch.from_numpy(y).to(dev).reshape(B, 1)
    d_in = torch.from_numpy(dn).to(dev).requires_grad_(True)
    cols = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    n_rows, inv_n, valid, d_rows, labels, targets = ops.compact_rows(X, d_in, yt, cols, True)
    rows = np.nonzero(y == 1)[0]
    assert int(n_rows.item()) == rows.size and d_rows.requires_grad
    assert not any(t.requires_grad for t in (n_rows, inv_n, valid, labels, targets))
    np.testing.assert_array_equal(d_rows.detach().cpu().numpy()[:rows.size], dn[rows])
    np.testing.assert_array_equal(targets.cpu().numpy()[:, :rows.size], Xn[rows][:, :2].astype(np.int64).T)
    gn = rng.standard_normal((B, W)).astype(np.float32)
    d_rows.backward(torch.from_numpy(gn).to(dev))
    want = np.zeros((B, W), np.float32)
    want[rows] = gn[:rows.size]
    np.testing.assert_array_equal(d_in.grad.cpu().numpy(), want)
