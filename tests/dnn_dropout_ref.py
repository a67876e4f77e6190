"""What the DNN-tower dropout tests share: a numpy uint32 mirror of the keep-mask hash of csrc/dnn.hip (documented in
include/xdfm.h at xdfm_dense_fwd_drop) and a float64 forward / backward of one dense + ReLU + dropout layer given a mask.
No GPU needed; checked by tests/test_dnn_dropout_host.py."""
import numpy as np
import torch

import dnn_ref as R

M32 = np.uint64(0xFFFFFFFF)


def _mix(x):
    """drop_mix of csrc/xdfm_internal.h on uint64 arrays holding 32-bit values (the products wrap through the mask)."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def thresh(p):
    """min((unsigned)(p * 2^32), 2^32 - 1) with p rounded to fp32 first, as the C ABI receives it."""
    t = float(np.float32(p)) * 4294967296.0
    return 4294967295 if t >= 4294967295.0 else int(t)


def keep_scale(p):
    """The fp32 1.0f / (1.0f - p) of the kernels, as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(rows, out, p, seed, layer, row0=0):
    """keep[rows][out] (bool) of cell (layer, row0 + row, col)."""
    seed = int(seed)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    k = _mix(np.array([(int(lo) ^ ((layer * 0x9E3779B1) & 0xFFFFFFFF))], dtype=np.uint64))[0]
    r = (np.arange(rows, dtype=np.uint64) + np.uint64(row0)) & M32
    rk = _mix((k + hi + ((r * np.uint64(0x85EBCA77)) & M32)) & M32)
    c = np.arange(out, dtype=np.uint64)
    h = _mix((rk[:, None] + ((c * np.uint64(0x9E3779B1)) & M32)[None, :]) & M32)
    return h >= np.uint64(thresh(p))


def layer_ref(x, W, b, keep, p):
    """(z, d) in float64: z = x W^T + b, d = keep ? relu(z) * s : 0 with s the kernels' fp32 scale.  Zeros are +0.0."""
    z = x.double() @ W.double().t() + b.double()
    s = keep_scale(p)
    d = torch.where(torch.as_tensor(keep), torch.relu(z) * s, torch.zeros_like(z)) + 0.0
    return z, d


def layer_bwd_ref(g, d, x, W, p):
    """(dx, dW, db) in float64 from the stored output d: gz = (d > 0) ? fl32(g * s) : 0 -- the product is rounded to fp32 once,
    as native_dropout_backward rounds it, before the float64 sums."""
    s = keep_scale(p)
    gs = (g.float() * torch.tensor(s, dtype=torch.float32)).double() if g.dtype == torch.float32 else g.double() * s
    gz = torch.where(d > 0, gs, torch.zeros_like(gs))
    return gz @ W.double() + 0.0, gz.t() @ x.double() + 0.0, gz.sum(0) + 0.0


def corr(a, b):
    """Pearson correlation of two boolean arrays of one shape."""
    a = a.astype(np.float64).ravel()
    b = b.astype(np.float64).ravel()
    a -= a.mean()
    b -= b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


bits = R.bits
first_difference = R.first_difference
