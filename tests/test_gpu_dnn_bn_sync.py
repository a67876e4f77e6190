"""GPU tests (-m gpu) of the host side of the synchronised batch norm (ops.bn_sync_native, ops.BatchNormActSync,
ops.bn_act_sync, the routing of layers.DNN) in ONE process: a dist.RowParallel of world 1 whose all-gather hands back what it
was given.  With one rank the split kernels merge the very pairs and sums the fused kernels merge, in the same order, so
every output must equal ops.bn_act's bit for bit -- y, dz, dgamma, dbeta, both running vectors, num_batches_tracked.  The
worlds above 1 are tests/test_gpu_dnn_bn_sync_abi.py (kernels) and tests/test_dist_bn_sync.py (processes)."""
import faulthandler

import pytest
import torch

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _one_rank():
    """A RowParallel of world 1 without a process group; counts its gathers."""
    from xdfm_amd import dist as xdist

    class OneRank(xdist.RowParallel):
        def __init__(self):
            self.group, self.world, self.rank, self.backend = None, 1, 0, "nccl"
            self._n_global, self._replicated, self.gathers = None, set(), []

        def all_gather_rows(self, t):
            self.gathers.append(tuple(t.shape))
            return t.contiguous().clone()

    return OneRank()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pair(cols, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    mods = []
    for _ in range(2):
        bn = torch.nn.BatchNorm1d(cols).to(dev)
        mods.append(bn)
    with torch.no_grad():
        w, b = 0.5 + torch.rand(cols, generator=gen), 0.5 * torch.randn(cols, generator=gen)
        rm, rv = torch.randn(cols, generator=gen), 0.5 + torch.rand(cols, generator=gen)
        for bn in mods:
            bn.weight.copy_(w.to(dev))
            bn.bias.copy_(b.to(dev))
            bn.running_mean.copy_(rm.to(dev))
            bn.running_var.copy_(rv.to(dev))
    return mods


@pytest.mark.parametrize("act", ["relu", "sigmoid", "linear"])
@pytest.mark.parametrize("rows,cols", [(70, 40), (131, 96), (2, 33)])
def test_one_rank_equals_the_fused_route_bit_for_bit(monkeypatch, rows, cols, act):
    from xdfm_amd import ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_BN_NATIVE", True)
    monkeypatch.setattr(ops, "DNN_BN_SYNC", True)
    dp = _one_rank()
    gen = torch.Generator().manual_seed(rows + cols)
    z0 = (torch.randn(rows, cols, generator=gen) * 2.0 + torch.linspace(0.0, 3.0, rows)[:, None]).to(dev)
    g = torch.randn(rows, cols, generator=gen).to(dev)
    bn_a, bn_b = _pair(cols, dev, 5)
    assert ops.bn_sync_native(z0, bn_b, dp) and not ops.bn_sync_native(z0, bn_b, object()) and not ops.bn_sync_native(z0.cpu(), bn_b, dp)
    for training in (True, False):
        bn_a.train(training)
        bn_b.train(training)
        za, zb = z0.clone().requires_grad_(True), z0.clone().requires_grad_(True)
        ya = ops.bn_act(za, bn_a, act, training)
        n_before = len(dp.gathers)
        yb = ops.bn_act_sync(zb, bn_b, act, training, dp)
        ya.backward(g)
        yb.backward(g)
        torch.cuda.synchronize()
        # one gather each way in training ([count | means | M2s], then the two sums); none in evaluation
        assert dp.gathers[n_before:] == ([(1, 1 + 2 * cols), (1, 2 * cols)] if training else []), dp.gathers[n_before:]
        for name, a, b in (("y", ya, yb), ("dz", za.grad, zb.grad), ("dgamma", bn_a.weight.grad, bn_b.weight.grad),
                           ("dbeta", bn_a.bias.grad, bn_b.bias.grad), ("running_mean", bn_a.running_mean, bn_b.running_mean),
                           ("running_var", bn_a.running_var, bn_b.running_var)):
            assert bool((_bits(a.detach()) == _bits(b.detach())).all()), (name, training)
        assert int(bn_a.num_batches_tracked) == int(bn_b.num_batches_tracked) == 1
        for bn in (bn_a, bn_b):
            bn.weight.grad = bn.bias.grad = None


def test_needs_input_grad_combinations_and_the_gather_every_rank_joins(monkeypatch):
    """Whatever this rank needs, the backward's gather runs (the other ranks wait in it), and what is asked for has the full
    call's bits."""
    from xdfm_amd import ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_BN_NATIVE", True)
    monkeypatch.setattr(ops, "DNN_BN_SYNC", True)
    rows, cols = 70, 40
    gen = torch.Generator().manual_seed(3)
    z0, g = torch.randn(rows, cols, generator=gen).to(dev), torch.randn(rows, cols, generator=gen).to(dev)
    full = None
    for needs in [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, False, True)]:
        dp = _one_rank()
        bn = _pair(cols, dev, 9)[0]
        z = z0.clone().requires_grad_(needs[0])
        bn.weight.requires_grad_(needs[1])
        bn.bias.requires_grad_(needs[2])
        ops.bn_act_sync(z, bn, "relu", True, dp).backward(g)
        torch.cuda.synchronize()
        assert dp.gathers == [(1, 1 + 2 * cols), (1, 2 * cols)], (needs, dp.gathers)
        got = (z.grad, bn.weight.grad, bn.bias.grad)
        if full is None:
            full = got
        for need, a, b in zip(needs, got, full):
            assert (a is not None) == need
            if need:
                assert bool((_bits(a) == _bits(b)).all()), needs


def test_fewer_than_two_global_rows_raise_after_the_gather_and_a_stand_in_counts_zero(monkeypatch):
    from xdfm_amd import ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_BN_NATIVE", True)
    monkeypatch.setattr(ops, "DNN_BN_SYNC", True)
    cols = 8
    bn = _pair(cols, dev, 1)[0]
    before = (bn.running_mean.clone(), bn.running_var.clone())
    z = torch.randn(1, cols, generator=torch.Generator().manual_seed(0)).to(dev)
    dp = _one_rank()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.bn_act_sync(z, bn, "relu", True, dp)
    assert dp.gathers == [(1, 1 + 2 * cols)], "every rank must have joined the gather before any of them raises"
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and int(bn.num_batches_tracked) == 0
    # evaluation takes a single row
    bn.eval()
    assert ops.bn_act_sync(z, bn, "relu", False, dp).shape == (1, cols)
    # a rank that shard() left with a stand-in row contributes count 0: alone in its world that is an empty batch
    bn.train()
    dp = _one_rank()
    dp._n_global, dp.world, dp.rank = 3, 4, 0
    assert dp.local_sizes()[0] == 0 and ops._bn_sync_count(z, dp) == 0
    dp.world = 1                                  # the gather below is still the one-rank stand-in
    dp.local_sizes = lambda: [0]
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.bn_act_sync(torch.randn(5, cols).to(dev), bn, "relu", True, dp)


@pytest.mark.parametrize("act", ["relu", "prelu"])
def test_tower_routing(monkeypatch, act):
    """layers.DNN under a RowParallel context: with the switch on both routing sites take ops.bn_act_sync once per layer, with it
    off the stock modules, as before; the model-level question `takes_bn_sync` follows."""
    from xdfm_amd import dist as xdist
    from xdfm_amd import layers, ops
    dev = _dev()
    monkeypatch.setattr(ops, "DNN_BN_NATIVE", True)
    dp = _one_rank()
    monkeypatch.setattr(xdist, "current", lambda: dp)
    calls = {"sync": 0, "native": 0}
    real_sync, real_native = ops.bn_act_sync, ops._bn_act_native
    monkeypatch.setattr(ops, "bn_act_sync", lambda *a: (calls.__setitem__("sync", calls["sync"] + 1), real_sync(*a))[1])
    monkeypatch.setattr(ops, "_bn_act_native", lambda *a: (calls.__setitem__("native", calls["native"] + 1), real_native(*a))[1])
    net = layers.DNN(40, (64, 40, 32), activation=act, use_bn=True, init_std=0.3, device=dev)
    keys = list(net.state_dict().keys())
    x = torch.randn(70, 40, generator=torch.Generator().manual_seed(2)).to(dev)
    for switch in (True, False):
        monkeypatch.setattr(ops, "DNN_BN_SYNC", switch)
        assert net.takes_bn_sync(dp) is switch and not net.takes_bn_sync(None) and not net.takes_bn_sync(object())
        calls["sync"] = calls["native"] = 0
        net.train()
        out = net(x)
        out.sum().backward()
        assert (calls["sync"], calls["native"]) == ((3, 0) if switch else (0, 0)), (switch, calls)
        assert bool(torch.isfinite(out).all()) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert list(net.state_dict().keys()) == keys
    assert [int(b.num_batches_tracked) for b in net.bn] == [2] * 3
