"""CPU: the C ABI of the native batch norm (csrc/bn.hip) -- symbols, the two queries and argument validation before any
device work -- and the host-side predicate / routing of ops.bn_act that needs no GPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "xdfm.h")
NAMES = ["xdfm_bn_row_block", "xdfm_bn_ws_elems", "xdfm_bn_fwd_train", "xdfm_bn_fwd_eval", "xdfm_bn_bwd", "xdfm_bn_bwd_eval"]
P = ctypes.c_void_p


def _lib():
    from xdfm_amd import _lib
    return _lib, _lib.load()


def test_symbols_in_header_binding_and_library():
    mod, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), "include/xdfm.h does not declare %s" % n
        assert n in mod.SIGNATURES, "xdfm_amd/_lib.py does not bind %s" % n
        assert hasattr(lib, n), "libxdfm_hip.so lacks %s" % n
    assert lib.xdfm_abi_version() == mod.ABI_VERSION == 9           # additions only


def test_queries_are_sane():
    _, lib = _lib()
    R = lib.xdfm_bn_row_block()
    assert R >= 1
    ws = lib.xdfm_bn_ws_elems
    rows_seq = [1, 2, 3, R - 1, R, R + 1, 2 * R, 3 * R + 5, 4096, 4097, 100000, 1 << 24]
    rows_seq = sorted(r for r in set(rows_seq) if r >= 1)
    for cols in (1, 31, 32, 33, 40, 256, 264):
        vals = [ws(r, cols) for r in rows_seq]
        assert all(v > 0 for v in vals) and vals == sorted(vals), (cols, vals)
        assert ws(R + 1, cols) > ws(R, cols) >= ws(1, cols)
    assert ws(4096, 256) == 4 * -(-4096 // R) * 256                 # one (mean, M2) pair of doubles per row block and column
    vals = [ws(4096, c) for c in (1, 2, 63, 64, 65, 256, 1000)]
    assert vals == sorted(vals) and vals[0] > 0
    for bad in [(0, 8), (-1, 8), (8, 0), (8, -3)]:
        assert ws(*bad) == 0, bad


def test_validation_before_device_work():
    """Every refusal of the header's list: rc 1 (XDFM_ERR_INVALID) and a message naming the argument, with no GPU in the
    machine -- the calls return before any device work."""
    mod, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)                        # a non-null host address: validation must reject before touching it

    def train(z=p, ldz=8, rows=4, cols=8, gamma=p, beta=p, eps=1e-5, momentum=0.1, act=1, y=p, ldy=8, save_mean=p, save_rstd=p,
              running_mean=p, running_var=p, ws=p):
        return lib.xdfm_bn_fwd_train(z, ldz, rows, cols, gamma, beta, eps, momentum, act, y, ldy, save_mean, save_rstd, running_mean,
                                     running_var, ws, None)

    def evalf(z=p, ldz=8, rows=4, cols=8, gamma=p, beta=p, eps=1e-5, act=1, y=p, ldy=8, running_mean=p, running_var=p):
        return lib.xdfm_bn_fwd_eval(z, ldz, rows, cols, gamma, beta, eps, act, y, ldy, running_mean, running_var, None)

    def bwd(fn):
        def call(g=p, ldg=8, y=p, ldy=8, z=p, ldz=8, rows=4, cols=8, gamma=p, save_mean=p, save_rstd=p, act=1, dz=p, lddz=8, dgamma=p,
                 dbeta=p, ws=p):
            return fn(g, ldg, y, ldy, z, ldz, rows, cols, gamma, save_mean, save_rstd, act, dz, lddz, dgamma, dbeta, ws, None)
        return call

    def err():
        return lib.xdfm_last_error()

    calls = {"bn_fwd_train": (train, ("z", "gamma", "beta", "y", "save_mean", "save_rstd", "running_mean", "running_var", "ws"), ("ldz", "ldy"), 2),
             "bn_fwd_eval": (evalf, ("z", "gamma", "beta", "y", "running_mean", "running_var"), ("ldz", "ldy"), 1),
             "bn_bwd": (bwd(lib.xdfm_bn_bwd), ("g", "y", "z", "gamma", "save_mean", "save_rstd", "ws"), ("ldg", "ldy", "ldz", "lddz"), 2),
             "bn_bwd_eval": (bwd(lib.xdfm_bn_bwd_eval), ("g", "y", "z", "gamma", "save_mean", "save_rstd", "ws"), ("ldg", "ldy", "ldz", "lddz"), 1)}
    for name, (call, ptrs, pitches, min_rows) in calls.items():
        tag = name.encode()
        for arg in ptrs:
            assert call(**{arg: None}) == 1 and tag in err() and (b"null pointer" in err() or b"NULL" in err()), (name, arg, err())
        for rows in (0, -5) + ((1,) if min_rows == 2 else ()):
            assert call(rows=rows) == 1 and b"rows = %d" % rows in err(), (name, rows, err())
        for cols in (0, -2):
            assert call(cols=cols) == 1 and b"cols = %d" % cols in err(), (name, cols, err())
        for pitch in pitches:
            assert call(**{pitch: 7}) == 1 and b"%s = 7" % pitch.encode() in err(), (name, pitch, err())
        for act in (3, -1, 7):
            assert call(act=act) == 1 and b"act = %d" % act in err(), (name, act, err())
    for call in (train, evalf):
        for eps in (0.0, -1e-5):
            assert call(eps=eps) == 1 and b"eps" in err(), err()
    for momentum in (-0.1, 1.5):
        assert train(momentum=momentum) == 1 and b"momentum" in err(), err()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)                  # the workspace holds doubles
    assert ctypes.addressof(buf) % 8 == 0
    for call in (train, calls["bn_bwd"][0], calls["bn_bwd_eval"][0]):
        assert call(ws=odd) == 1 and b"8-byte aligned" in err(), err()
    # evaluation accepts one row as far as validation goes: the one-row refusal is training's alone
    assert evalf(rows=1, cols=0) == 1 and b"cols = 0" in err()
    with pytest.raises(ValueError, match="bn_fwd_train"):
        mod.check(train(rows=1), "bn_fwd_train")


def test_switch_and_predicate_on_the_cpu():
    from xdfm_amd import layers, ops
    assert ops._env_switch({}, "XDFM_DNN_BN_NATIVE") is True
    assert ops._env_switch({"XDFM_DNN_BN_NATIVE": "0"}, "XDFM_DNN_BN_NATIVE") is False
    assert ops.DNN_BN_NATIVE is ops._env_switch(os.environ, "XDFM_DNN_BN_NATIVE")
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm1d(6)
    z = torch.randn(9, 6)
    assert not ops.bn_native(z, bn) and not ops.bn_native(z.double(), bn.double())
    bn = torch.nn.BatchNorm1d(6)
    want = torch.relu(torch.nn.functional.batch_norm(z, None, None, bn.weight, bn.bias, True, 0.1, bn.eps))
    got = ops.bn_act(z, bn, "relu", True)
    assert torch.equal(got, want) and int(bn.num_batches_tracked) == 1
    # a CPU tower is today's sequence, state_dict keys as they were
    net = layers.DNN(5, (6, 4), activation="sigmoid", use_bn=True, init_std=0.3)
    assert [k for k in net.state_dict() if k.startswith("bn.0.")] == ["bn.0.weight", "bn.0.bias", "bn.0.running_mean", "bn.0.running_var",
                                                                      "bn.0.num_batches_tracked"]
    x = torch.randn(7, 5)
    h = x
    for lin, b in zip(net.linears, net.bn):
        h = torch.sigmoid(torch.nn.functional.batch_norm(torch.nn.functional.linear(h, lin.weight, lin.bias), None, None, b.weight, b.bias, True, 0.1, b.eps))
    assert torch.equal(net(x), h)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net(x[:1])
