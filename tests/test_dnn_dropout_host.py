"""CPU: the hashed keep mask of the DNN tower's native dropout (csrc/dnn.hip) through its numpy mirror -- rates,
independence, the row0 identity -- the four new symbols of the C ABI, argument validation before any device work, and the
torch path that layers.DNN keeps on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dnn_dropout_ref as D
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "xdfm.h")
NAMES = ["xdfm_dense_fwd_drop", "xdfm_dense_bwd_x_drop", "xdfm_dense_bwd_w_drop", "xdfm_dense_dropout_mask"]
P = ctypes.c_void_p
PS = (0.1, 0.5, 0.8)
SHAPES = ((4096, 256), (2049, 64), (520, 96))
LAYERS = (0, 1, 2)
SEEDS = (0, 7, 1234567891011, 1234567891012, 2 ** 62 - 1)
_MASKS = {}


def _mask(shape, p, seed, layer):
    key = (shape, p, seed, layer)
    if key not in _MASKS:
        _MASKS[key] = D.keep_mask(shape[0], shape[1], p, seed, layer)
    return _MASKS[key]


def _lib():
    from xdfm_amd import _lib
    return _lib, _lib.load()


# ------------------------------------------------------------------------------------------------ the scheme
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("shape", SHAPES)
def test_keep_rate_overall_and_per_column_within_5_sigma(p, shape):
    rows, out = shape
    q = 1.0 - float(np.float32(p))
    worst = 0.0
    for layer in LAYERS:
        for seed in SEEDS:
            m = _mask(shape, p, seed, layer)
            sd_all = np.sqrt(q * (1 - q) / m.size)
            sd_col = np.sqrt(q * (1 - q) / rows)
            dev_all = abs(m.mean() - q) / sd_all
            dev_col = float(np.abs(m.mean(0) - q).max() / sd_col)
            worst = max(worst, dev_all, dev_col)
            assert dev_all <= 5.0, (p, shape, layer, seed, "overall", dev_all)
            assert dev_col <= 5.0, (p, shape, layer, seed, "per column", dev_col)
    print("p=%g %dx%d worst deviation %.2f sigma" % (p, rows, out, worst))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("shape", SHAPES)
def test_neighbours_layers_and_consecutive_seeds_are_uncorrelated(p, shape):
    n = shape[0] * shape[1]
    worst = 0.0
    for layer in LAYERS:
        for seed in SEEDS:
            m = _mask(shape, p, seed, layer)
            nxt = _mask(shape, p, seed + 1, layer) if seed + 1 in SEEDS else D.keep_mask(shape[0], shape[1], p, seed + 1, layer)
            pairs = [("columns", m[:, :-1], m[:, 1:]), ("rows", m[:-1], m[1:]),
                     ("layers", m, _mask(shape, p, seed, (layer + 1) % 3)), ("seed and seed + 1", m, nxt)]
            for what, a, b in pairs:
                c = abs(D.corr(a, b)) * np.sqrt(a.size)
                worst = max(worst, c)
                assert c <= 5.0, (p, shape, layer, seed, what, c, n)
    print("p=%g %dx%d worst |corr| * sqrt(n) = %.2f" % (p, shape[0], shape[1], worst))


def test_masks_differ_where_they_should_and_repeat_where_they_should():
    a = D.keep_mask(520, 96, 0.5, 7, 0)
    assert np.array_equal(a, D.keep_mask(520, 96, 0.5, 7, 0))
    for other in (D.keep_mask(520, 96, 0.5, 8, 0), D.keep_mask(520, 96, 0.5, 7, 1), D.keep_mask(520, 96, 0.5, 7 + 2 ** 32, 0)):
        assert 0.4 < (a != other).mean() < 0.6
    assert D.keep_mask(64, 32, 0.0, 5, 0).all()                      # thresh 0
    assert D.thresh(0.5) == 2 ** 31 and D.thresh(0.75) == 3 * 2 ** 30
    assert D.keep_scale(0.5) == 2.0 and D.keep_scale(0.75) == 4.0
    assert D.keep_scale(0.1) == float(np.float32(1.0) / np.float32(0.9))


@pytest.mark.parametrize("k", [1, 63, 257, 2 ** 31 - 5, 2 ** 32 + 3])
def test_row0_addresses_the_rows_of_the_batch(k):
    """mask(row0 = k) is rows k .. of mask(row0 = 0); the row index wraps at 2^32 like the kernel's (unsigned) cast."""
    rows, out = 70, 96
    for p, seed, layer in ((0.5, 1234567891011, 1), (0.1, 7, 2)):
        shard = D.keep_mask(rows, out, p, seed, layer, row0=k)
        if k < 1000:
            whole = D.keep_mask(k + rows, out, p, seed, layer)
            assert np.array_equal(shard, whole[k:])
        else:
            again = np.stack([D.keep_mask(1, out, p, seed, layer, row0=k + r)[0] for r in range(rows)])
            assert np.array_equal(shard, again)
            if k >= 2 ** 32:
                assert np.array_equal(shard, D.keep_mask(rows, out, p, seed, layer, row0=k - 2 ** 32))


def test_float64_layer_reference_against_autograd():
    """layer_ref / layer_bwd_ref against torch's double autograd of dropout-by-mask after relu (s exact at p = 0.5)."""
    torch.manual_seed(3)
    x, W, b, g = (torch.randn(9, 5, dtype=torch.float64), torch.randn(32, 5, dtype=torch.float64),
                  torch.randn(32, dtype=torch.float64), torch.randn(9, 32, dtype=torch.float64))
    keep = D.keep_mask(9, 32, 0.5, 11, 0)
    xs, Ws, bs = (t.clone().requires_grad_(True) for t in (x, W, b))
    d_auto = torch.relu(xs @ Ws.t() + bs) * torch.as_tensor(keep) * 2.0
    d_auto.backward(g)
    z, d = D.layer_ref(x, W, b, keep, 0.5)
    assert torch.equal(d, d_auto.detach() + 0.0)
    assert bool(((d > 0) == (torch.as_tensor(keep) & (z > 0))).all())
    dx, dW, db = D.layer_bwd_ref(g, d, x, W, 0.5)
    for got, want in ((dx, xs.grad), (dW, Ws.grad), (db, bs.grad)):
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_in_header_binding_and_library():
    mod, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), "include/xdfm.h does not declare %s" % n
        assert n in mod.SIGNATURES, "xdfm_amd/_lib.py does not bind %s" % n
        assert hasattr(lib, n), "libxdfm_hip.so lacks %s" % n
    assert lib.xdfm_abi_version() == mod.ABI_VERSION == 9           # additions only
    text = open(HEADER).read()
    for word in ("0x7feb352d", "0x846ca68b", "0x9E3779B1", "0x85EBCA77", "in distribution only", "1.0f / (1.0f - p_drop)"):
        assert word in text, "include/xdfm.h does not document %r" % word


def test_validation_before_device_work():
    """rc 1 and a message that names the argument, with no GPU in the machine: the dropout arguments, then everything the
    plain entry points refuse."""
    mod, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)                        # a non-null host address: validation must reject before touching it

    def fwd(x=p, rows=8, k=13, ldx=13, W=p, out=32, b=p, act=1, y=p, ldy=32, p_drop=0.5, seed=p, layer=0, row0=0):
        return lib.xdfm_dense_fwd_drop(x, rows, k, ldx, W, out, b, act, y, ldy, p_drop, seed, layer, row0, None)

    def bwx(g=p, ldg=32, y=p, ldy=32, rows=8, out=32, W=p, k=13, dx=p, lddx=13, p_drop=0.5):
        return lib.xdfm_dense_bwd_x_drop(g, ldg, y, ldy, rows, out, W, k, dx, lddx, p_drop, None)

    def bww(g=p, ldg=32, y=p, ldy=32, x=p, ldx=13, rows=8, k=13, out=32, ws=p, dW=p, db=p, p_drop=0.5):
        return lib.xdfm_dense_bwd_w_drop(g, ldg, y, ldy, x, ldx, rows, k, out, ws, dW, db, p_drop, None)

    def msk(rows=8, out=32, p_drop=0.5, seed=p, layer=0, row0=0, keep=p):
        return lib.xdfm_dense_dropout_mask(rows, out, p_drop, seed, layer, row0, keep, None)

    def err():
        return lib.xdfm_last_error()

    names = {fwd: b"dense_fwd_drop", bwx: b"dense_bwd_x_drop", bww: b"dense_bwd_w_drop", msk: b"dense_dropout_mask"}
    for call, who in names.items():
        for bad in (1.0, 1.5, -0.1, float("nan")):
            assert call(p_drop=bad) == 1 and who in err() and b"p_drop" in err() and b"outside [0, 1)" in err(), (who, bad, err())
    for call in (fwd, msk):
        assert call(seed=None) == 1 and names[call] in err() and b"seed is NULL" in err(), err()
        assert call(layer=-1) == 1 and names[call] in err() and b"layer = -1" in err(), err()
        assert call(row0=-2) == 1 and names[call] in err() and b"row0 = -2" in err(), err()
    for act in (0, 2):
        assert fwd(act=act) == 1 and b"dense_fwd_drop" in err() and b"act = %d" % act in err() and b"relu" in err(), err()
    for call in (bwx, bww):
        assert call(y=None) == 1 and names[call] in err() and b"y is NULL" in err(), err()
    # ... and what the plain entry points refuse, under the new names
    for call, ptrs in ((fwd, ("x", "W", "y")), (bwx, ("g", "W", "dx")), (bww, ("g", "x", "dW")), (msk, ("keep",))):
        for arg in ptrs:
            if call in (bwx, bww) and arg == "y":
                continue
            assert call(**{arg: None}) == 1 and names[call] in err() and b"null pointer" in err(), (names[call], arg, err())
        for rows in (0, -5):
            assert call(rows=rows) == 1 and b"rows = %d" % rows in err(), (names[call], rows, err())
    for call in (fwd, bwx, bww):
        assert call(k=0) == 1 and b"in = 0" in err(), (names[call], err())
        for out in (48, 16, 0, 70):
            assert call(out=out) == 1 and b"out = %d" % out in err() and b"multiple of 32" in err(), (names[call], out, err())
    assert msk(out=0) == 1 and b"out = 0" in err()
    assert bww(ws=None) == 1 and b"workspace is NULL" in err()
    for call, kw, word in [(fwd, dict(ldx=12), b"ldx = 12"), (fwd, dict(ldy=31), b"ldy = 31"), (bwx, dict(ldg=31), b"ldg = 31"),
                           (bwx, dict(ldy=31), b"ldy = 31"), (bwx, dict(lddx=12), b"lddx = 12"), (bww, dict(ldg=31), b"ldg = 31"),
                           (bww, dict(ldy=31), b"ldy = 31"), (bww, dict(ldx=12), b"ldx = 12")]:
        assert call(**kw) == 1 and word in err() and names[call] in err(), (names[call], kw, err())
    for act in (3, -1, 7):
        assert fwd(act=act, p_drop=0.0) == 1 and b"act = %d" % act in err()
    with pytest.raises(ValueError, match="dense_fwd_drop"):
        mod.check(fwd(p_drop=1.0), "dense_fwd_drop")


# ------------------------------------------------------------------------------------------------ host routing
def test_switch_parsing():
    from xdfm_amd import ops
    assert ops._env_switch({}, "XDFM_DNN_DROPOUT_NATIVE") is True
    assert ops._env_switch({"XDFM_DNN_DROPOUT_NATIVE": "0"}, "XDFM_DNN_DROPOUT_NATIVE") is False
    assert ops.DNN_DROPOUT_NATIVE is ops._env_switch(os.environ, "XDFM_DNN_DROPOUT_NATIVE")
    x, W, b = torch.randn(9, 13), torch.randn(32, 13), torch.randn(32)
    assert not ops.dense_dropout_native(x, W, b, 0.5)               # CPU tensors
    with pytest.raises(ValueError, match="dense_relu_dropout"):
        ops.dense_relu_dropout(x, W, b, 0.5, torch.zeros(1, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="outside"):
        ops.dense_relu_dropout(x, W, b, 1.0, torch.zeros(1, dtype=torch.int64), 0)


def test_cpu_tower_with_dropout_trains_and_evaluates_through_torch(monkeypatch):
    """layers.DNN(..., dropout_rate = 0.5) on CPU tensors: the stock path as before -- never the new op, nn.Dropout's own
    draw in training (torch.manual_seed repeats it), the dropout-free value in eval()."""
    from xdfm_amd import layers, ops

    def boom(*a, **k):
        raise AssertionError("DenseReLUDropout ran on CPU tensors")

    monkeypatch.setattr(ops, "dense_relu_dropout", boom)
    tower = layers.DNN(13, (32, 32, 8), dropout_rate=0.5, init_std=0.5)
    twin = layers.DNN(13, (32, 32, 8), dropout_rate=0, init_std=0.5)
    twin.load_state_dict(tower.state_dict())
    x = torch.randn(40, 13)

    def stock(train):
        h = x
        for lin in tower.linears:
            h = torch.nn.functional.dropout(torch.relu(torch.nn.functional.linear(h, lin.weight, lin.bias)), 0.5, train)
        return h

    tower.train()
    torch.manual_seed(5)
    out = tower(x)
    torch.manual_seed(5)
    assert torch.equal(out, stock(True))
    assert tower.last_drop_seed is None
    out.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in tower.parameters())
    assert float((out == 0).float().mean()) > 0.4
    tower.eval()
    assert torch.equal(tower(x), stock(False)) and torch.equal(tower(x), twin.eval()(x))
