"""CPU: the C ABI of the synchronised batch norm (csrc/bn.hip: xdfm_bn_stats, xdfm_bn_fwd_apply_sync, xdfm_bn_bwd_sums,
xdfm_bn_bwd_apply_sync) -- symbols and argument validation before any device work -- and the host-side switch and
predicate of ops.bn_act_sync that need no GPU."""
import ctypes
import os
import re

import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "xdfm.h")
NAMES = ["xdfm_bn_stats", "xdfm_bn_fwd_apply_sync", "xdfm_bn_bwd_sums", "xdfm_bn_bwd_apply_sync"]
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


def test_validation_before_device_work():
    """Every refusal of the header's list: rc 1 (XDFM_ERR_INVALID) and a message naming the entry point and the argument,
    with no GPU in the machine -- the calls return before any device work."""
    mod, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, P)                        # a non-null host address: validation must reject before touching it

    def stats(z=p, ldz=8, rows=4, cols=8, pair=p, ws=p):
        return lib.xdfm_bn_stats(z, ldz, rows, cols, pair, ws, None)

    def fwd(z=p, ldz=8, rows=4, cols=8, all=p, world=2, gamma=p, beta=p, eps=1e-5, momentum=0.1, act=1, y=p, ldy=8, save_mean=p,
            save_rstd=p, running_mean=p, running_var=p):
        return lib.xdfm_bn_fwd_apply_sync(z, ldz, rows, cols, all, world, gamma, beta, eps, momentum, act, y, ldy, save_mean, save_rstd,
                                          running_mean, running_var, None)

    def sums(g=p, ldg=8, y=p, ldy=8, z=p, ldz=8, rows=4, cols=8, save_mean=p, save_rstd=p, act=1, sums=p, ws=p):
        return lib.xdfm_bn_bwd_sums(g, ldg, y, ldy, z, ldz, rows, cols, save_mean, save_rstd, act, sums, ws, None)

    def bwd(g=p, ldg=8, y=p, ldy=8, z=p, ldz=8, rows=4, rows_counted=None, cols=8, all=p, world=2, rank=1, n_total=9, gamma=p,
            save_mean=p, save_rstd=p, act=1, dz=p, lddz=8, dgamma=p, dbeta=p):
        counted = rows if rows_counted is None else rows_counted
        return lib.xdfm_bn_bwd_apply_sync(g, ldg, y, ldy, z, ldz, rows, counted, cols, all, world, rank, n_total, gamma, save_mean,
                                          save_rstd, act, dz, lddz, dgamma, dbeta, None)

    def err():
        return lib.xdfm_last_error()

    calls = {"bn_stats": (stats, ("z", "pair", "ws"), ("ldz",), False),
             "bn_fwd_apply_sync": (fwd, ("z", "all", "gamma", "beta", "y", "save_mean", "save_rstd", "running_mean", "running_var"),
                                   ("ldz", "ldy"), True),
             "bn_bwd_sums": (sums, ("g", "y", "z", "save_mean", "save_rstd", "sums", "ws"), ("ldg", "ldy", "ldz"), True),
             "bn_bwd_apply_sync": (bwd, ("g", "y", "z", "all", "gamma", "save_mean", "save_rstd"), ("ldg", "ldy", "ldz", "lddz"), True)}
    for name, (call, ptrs, pitches, has_act) in calls.items():
        tag = name.encode() + b":"
        for arg in ptrs:
            assert call(**{arg: None}) == 1 and tag in err() and (b"null pointer" in err() or b"NULL" in err()), (name, arg, err())
        for rows in (0, -5):
            assert call(rows=rows) == 1 and tag in err() and b"rows = %d" % rows in err(), (name, rows, err())
        for cols in (0, -2):
            assert call(cols=cols) == 1 and tag in err() and b"cols = %d" % cols in err(), (name, cols, err())
        for pitch in pitches:
            assert call(**{pitch: 7}) == 1 and tag in err() and b"%s = 7" % pitch.encode() in err(), (name, pitch, err())
        for act in ((3, -1, 7) if has_act else ()):
            assert call(act=act) == 1 and tag in err() and b"act = %d" % act in err(), (name, act, err())
        # one row is a shard like any other: the two-row floor is the global batch's
        assert call(rows=1, cols=0) == 1 and b"cols = 0" in err(), (name, err())
    for call, name in ((fwd, b"bn_fwd_apply_sync:"), (bwd, b"bn_bwd_apply_sync:")):
        for world in (0, -1):
            assert call(world=world) == 1 and name in err() and b"world = %d" % world in err(), err()
    for rank in (-1, 2, 5):
        assert bwd(rank=rank) == 1 and b"bn_bwd_apply_sync:" in err() and b"rank = %d" % rank in err(), err()
    assert bwd(world=1, rank=1) == 1 and b"rank = 1" in err(), err()
    for n_total in (1, 0, -3):
        assert bwd(n_total=n_total) == 1 and b"bn_bwd_apply_sync:" in err() and b"n_total = %d" % n_total in err(), err()
    for counted in (3, 5, -1):
        assert bwd(rows_counted=counted) == 1 and b"rows_counted = %d" % counted in err(), err()
    for eps in (0.0, -1e-5):
        assert fwd(eps=eps) == 1 and b"bn_fwd_apply_sync:" in err() and b"eps" in err(), err()
    for momentum in (-0.1, 1.5):
        assert fwd(momentum=momentum) == 1 and b"bn_fwd_apply_sync:" in err() and b"momentum" in err(), err()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)                  # workspace, pair, sums and all hold doubles
    assert ctypes.addressof(buf) % 8 == 0
    for bad in (stats(ws=odd), stats(pair=odd), sums(ws=odd), sums(sums=odd), fwd(all=odd), bwd(all=odd)):
        assert bad == 1 and b"8-byte aligned" in err(), err()
    try:
        mod.check(bwd(n_total=1), "bn_bwd_apply_sync")
    except ValueError as exc:
        assert "bn_bwd_apply_sync" in str(exc)
    else:
        raise AssertionError("check() let XDFM_ERR_INVALID pass")


def test_switch_is_off_by_default_and_read_like_its_neighbours():
    from xdfm_amd import ops
    assert isinstance(ops.DNN_BN_SYNC, bool)
    assert ops._env_switch({}, "XDFM_DNN_BN_SYNC", False) is False
    assert ops._env_switch({"XDFM_DNN_BN_SYNC": "0"}, "XDFM_DNN_BN_SYNC", False) is False
    assert ops._env_switch({"XDFM_DNN_BN_SYNC": "1"}, "XDFM_DNN_BN_SYNC", False) is True
    assert ops.DNN_BN_SYNC is ops._env_switch(os.environ, "XDFM_DNN_BN_SYNC", False)
    if "XDFM_DNN_BN_SYNC" not in os.environ:
        assert ops.DNN_BN_SYNC is False


class _FakeRowParallel(object):
    """Stands where a dist.RowParallel would; made one below without a process group."""


def test_predicate_on_the_cpu(monkeypatch):
    from xdfm_amd import dist, layers, ops
    bn = torch.nn.BatchNorm1d(6)
    z = torch.randn(9, 6)
    dp = dist.RowParallel.__new__(dist.RowParallel)                  # an instance without a process group
    dp.world, dp.rank, dp._n_global = 2, 0, None
    for switch in (False, True):
        monkeypatch.setattr(ops, "DNN_BN_SYNC", switch)
        assert not ops.bn_sync_native(z, bn, dp)                     # a CPU tensor
        assert not ops.bn_sync_native(z, bn, object())               # an opaque context
        assert not ops.bn_sync_native(z, bn, None)
    # with everything else in place only the switch decides
    monkeypatch.setattr(ops, "bn_native", lambda z, bn: True)
    monkeypatch.setattr(ops, "DNN_BN_SYNC", False)
    assert not ops.bn_sync_native(z, bn, dp)
    monkeypatch.setattr(ops, "DNN_BN_SYNC", True)
    assert ops.bn_sync_native(z, bn, dp)
    assert not ops.bn_sync_native(z, bn, object()) and not ops.bn_sync_native(z, bn, _FakeRowParallel())
    # the count that travels with the pair
    assert ops._bn_sync_count(z, dp) == 9                            # no shard() before the forward: every row counts
    dp._n_global = 3
    dp.world, dp.rank = 4, 0                                         # split points 0 0 1 2 3: rank 0 holds a stand-in
    assert dp.local_sizes() == [0, 1, 1, 1] and ops._bn_sync_count(z[:1], dp) == 0
    dp.rank = 2
    assert ops._bn_sync_count(z[:1], dp) == 1
    # a CPU tower never takes the route, whatever the switch says
    net = layers.DNN(5, (6, 4), activation="relu", use_bn=True)
    assert not net.takes_bn_sync(dp) and not net.takes_bn_sync(None)
