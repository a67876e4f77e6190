"""xDeepFMPro under row-parallel training (xdfm_amd/dist.py + xdfm_amd/pro.py): N ranks on N shards equal one process on
the global batch, as tests/test_dist.py checks for xDeepFM.  The SFG loss divides the summed losses of the positive rows by
the number of positives of the GLOBAL batch (deepctr/xdeepfm_pro/sfg_decoder.py:262-268); a rank sees a shard.

CPU tests (gloo, worlds 2 and 4): the product's `fit`, DP logic and normaliser hook (`BaseModelSFG.sfg_normaliser`) around
the arithmetic of the CPU oracle, whose locally normalised SFG term is rescaled by (P_local + 1e-8) / the product's
normaliser.  The labels leave rank 0 of world 2 without a positive in batch 0, the whole of batch 1 without one, and
batch 2 is ragged (22 rows).

GPU tests (gloo, two ranks on cuda:0): the real kernels on the dynamic route (XDFM_PRO_GRAPH=0: torch.nonzero, eager
launches) and on the static one (XDFM_PRO_GRAPH=1: K11 counts the global labels on the device, the collective-free half of
the step is replayed from a graph), each against the single-process run of the same setting.

The in-place gradient exchange (dist.RowParallel.reduce_dense_grads with a threshold) against the flat one, 2 ranks."""
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, ROOT
from test_dist import CIN, D, DNN, ND, VOCAB, _free_port

SFG_HIDDEN = (16, 32)
SPAWN_LIMIT_S = 150.0          # per spawn: a world of workers that does not finish in this time is killed and the test fails


def _labels(n_rows):
    """150 rows: zero except rows 32:64:2 and 128:150:3 -- global batches of 64: batch 0 has its positives in the second
    half only (rank 0 of 2 has none), batch 1 has none at all, batch 2 is the ragged tail.  Longer data (the GPU tests, 343
    rows = 5 full batches + 23) goes on with every fifth row from 200 on, so that the later full batches, which are
    replays on the static route, carry positives on both ranks and another count each."""
    y = np.zeros(n_rows, np.float32)
    y[32:64:2] = 1.0
    y[128:150:3] = 1.0
    y[200::5] = 1.0
    return y


def _make_model(device, oracle_backed):
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.xdeepfm_pro import xDeepFMPro
    from oracle import xdeepfm_oracle as orc
    names = ["C%d" % (i + 1) for i in range(len(VOCAB))]
    dnames = ["I%d" % (i + 1) for i in range(ND)]
    cols = [SparseFeat(n, v, D) for n, v in zip(names, VOCAB)] + [DenseFeat(n, 1) for n in dnames]
    spec = orc.Spec(names, VOCAB, dnames, D, CIN, True, "relu", DNN, l2_reg_dnn=1e-5)
    pro = orc.ProSpec(sfg_weight=0.1, sfg_hidden_units=SFG_HIDDEN)

    class OracleBacked(xDeepFMPro):
        """Product fit loop, DP logic and normaliser; arithmetic by the CPU oracle."""

        def forward_with_sfg(self, X, y=None):
            train = self.training and y is not None
            y_pred, sfg = orc.pro_forward_with_sfg(X, y, dict(self.named_parameters()), spec, pro, training=train)
            if sfg is None:
                return y_pred, None
            p_local = float((y.reshape(-1) == 1).sum())
            # the oracle divided by the shard's own count; the product says what to divide by
            return y_pred, {"sfg_loss": sfg * ((p_local + 1e-8) / self.sfg_normaliser(y))}

        def get_regularization_loss(self, _defer_tables=False, _part="all"):
            if _part == "tables":
                return torch.zeros((1,))
            return orc.regularization_loss(dict(self.named_parameters()), spec)

    cls = OracleBacked if oracle_backed else xDeepFMPro
    model = cls(cols, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, l2_reg_dnn=1e-5, device=device,
                sfg_hidden_units=SFG_HIDDEN, sfg_dropout=0)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy"])
    for pg in model.optim.param_groups:
        pg["lr"] = 1e-2
    return model, names + dnames, orc


def _run(device, oracle_backed, per_rank_bs, n_rows):
    model, names, orc = _make_model(device, oracle_backed)
    X, _ = orc.synthetic_batch(n_rows, VOCAB, ND, seed=5)
    y = _labels(n_rows)
    # no validation data: the loop, like the reference's, never returns to train mode after an evaluation, and a second
    # epoch in eval mode would not run the SFG branch
    hist = model.fit({n: X[:, i] for i, n in enumerate(names)}, y, batch_size=per_rank_bs, epochs=2, verbose=2, shuffle=False)
    state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    step = model.__dict__.get("_graphed_step")
    state["__replays__"] = np.array([step.replays if step is not None else 0])
    return {k: list(v) for k, v in hist.history.items()}, state


def _worker(rank, world, port, device, oracle_backed, out_dir, n_rows, per_rank_bs):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hist, state = _run(device, oracle_backed, per_rank_bs, n_rows)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), hist_keys=np.array(sorted(hist)),
                 hist_vals=np.array([hist[k] for k in sorted(hist)]), **{"p:" + k: v for k, v in state.items()})
    finally:
        dist.destroy_process_group()


def _spawn(fn, args, world, limit=SPAWN_LIMIT_S):
    """mp.spawn with a time limit of its own: workers that are still alive after `limit` seconds are killed."""
    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + limit
    while not ctx.join(timeout=max(0.1, min(5.0, deadline - time.monotonic()))):     # raises when a worker failed
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail("%d workers did not finish within %.0f s" % (world, limit))


@functools.lru_cache(maxsize=None)
def _single(device, oracle_backed, n_rows, setting):
    """The single-process run on global batches of 64, once per (device, rows, XDFM_PRO_GRAPH setting)."""
    return _run(device, oracle_backed, per_rank_bs=64, n_rows=n_rows)


def _check(tmp_path, device, oracle_backed, rtol, atol, n_rows=150, world=2):
    _spawn(_worker, (world, _free_port(), device, oracle_backed, str(tmp_path), n_rows, 64 // world), world)
    hist1, state1 = _single(device, oracle_backed, n_rows, os.environ.get("XDFM_PRO_GRAPH", "0"))
    state1 = dict(state1)
    ranks = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    r0 = ranks[0]
    keys = [str(k) for k in r0["hist_keys"]]
    assert keys == sorted(hist1) and "sfg_loss" in keys and "loss" in keys
    want = np.array([hist1[k] for k in keys])
    print("history keys %s\n%d ranks:\n%s\nsingle process:\n%s" % (keys, world, r0["hist_vals"], want))
    assert (want[keys.index("sfg_loss")] > 0).all()
    np.testing.assert_allclose(r0["hist_vals"], want, rtol=rtol, atol=atol)
    replays = tuple(int(r["p:__replays__"][0]) for r in ranks) + (int(state1.pop("__replays__")[0]),)
    for k, v in state1.items():
        np.testing.assert_allclose(r0["p:" + k], v, rtol=rtol, atol=atol, err_msg=k)
    for r in ranks[1:]:
        np.testing.assert_allclose(r["hist_vals"], r0["hist_vals"], rtol=1e-6, atol=1e-7)   # every rank logs the same
        for k in state1:
            np.testing.assert_array_equal(r["p:" + k], r0["p:" + k], err_msg="replicas differ: " + k)
    return replays


@pytest.mark.parametrize("world", [2, 4])
def test_row_parallel_pro_fit_equals_single_process_cpu_gloo(tmp_path, world):
    _check(tmp_path, "cpu", True, rtol=2e-4, atol=2e-6, world=world)


@pytest.mark.gpu
@pytest.mark.parametrize("pro_graph", ["0", "1"])
def test_row_parallel_pro_fit_equals_single_process_gpu(tmp_path, monkeypatch, pro_graph):
    """343 rows: 5 full global batches and a ragged one of 23 per epoch.  On the static route each rank replays the first half
    of its step from the third full batch on, with another count of global positives at every replay (16, 0, 8, 12,
    12)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("XDFM_PRO_GRAPH", pro_graph)
    replays = _check(tmp_path, "cuda:0", False, rtol=1e-3, atol=2e-5, n_rows=343)
    print("replays (rank 0, rank 1, single process): %r" % (replays,))
    if pro_graph == "1" and os.environ.get("XDFM_HIP_GRAPH", "1") != "0":
        assert min(replays) >= 2, replays
    if pro_graph == "0":
        assert max(replays) == 0, replays


# ------------------------------------------------------------------------------------------------- #
def _toy():
    torch.manual_seed(0)
    m = torch.nn.Module()
    m.small_a = torch.nn.Parameter(torch.zeros(7))
    m.big = torch.nn.Parameter(torch.zeros(37, 11))          # 407 elements: in place at a threshold of 100
    m.small_b = torch.nn.Parameter(torch.zeros(3, 5))
    return m


def _exchange_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from xdfm_amd import dist as xdist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dp = xdist.current()
        calls = []
        reduce_ = dp.all_reduce_sum
        dp.all_reduce_sum = lambda t: (calls.append(t.numel()), reduce_(t))[1]
        out = {}
        for name, kw in (("flat", {}), ("inplace", dict(inplace_min_numel=100)), ("strided", dict(inplace_min_numel=100))):
            m = _toy()
            g = torch.Generator().manual_seed(100 + rank)
            for p in m.parameters():
                p.grad = torch.randn(p.shape, generator=g)
            if name == "strided":                                    # the same values in a gradient that is not contiguous
                vals, m.big.grad = m.big.grad, torch.empty(11, 37).t()
                m.big.grad.copy_(vals)
                assert not m.big.grad.is_contiguous()
            ptrs = [p.grad.data_ptr() for p in m.parameters()]
            del calls[:]
            dp.reduce_dense_grads(m, **kw)
            assert ptrs == [p.grad.data_ptr() for p in m.parameters()]
            out[name + ":calls"] = np.array(calls)
            for k, p in m.named_parameters():
                out[name + ":" + k] = p.grad.numpy().copy()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    finally:
        dist.destroy_process_group()


def test_large_gradients_are_reduced_in_place_with_the_same_sums(tmp_path):
    from xdfm_amd import dist as xdist
    assert xdist.INPLACE_MIN_NUMEL > 407                     # the default keeps a model this small on the flat path
    _spawn(_exchange_worker, (2, _free_port(), str(tmp_path)), 2, limit=60.0)
    ranks = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(2)]
    for r in ranks:
        assert list(r["flat:calls"]) == [7 + 407 + 15]       # one flat collective
        assert list(r["inplace:calls"]) == [407, 7 + 15]     # the large gradient where it lies, the rest flat
        assert list(r["strided:calls"]) == [407, 7 + 15]     # the same collectives whatever the gradient's strides
        for k in ("small_a", "big", "small_b"):
            np.testing.assert_array_equal(r["inplace:" + k], r["flat:" + k], err_msg=k)
            np.testing.assert_array_equal(r["strided:" + k], r["flat:" + k], err_msg=k)
            np.testing.assert_array_equal(r["flat:" + k], ranks[0]["flat:" + k], err_msg="ranks differ: " + k)
    g = [torch.Generator().manual_seed(100 + r) for r in range(2)]
    first = [torch.randn(7, generator=x) for x in g]
    np.testing.assert_array_equal(ranks[0]["flat:small_a"], (first[0] + first[1]).numpy())     # and they are the sums


# ------------------------------------------------------------------------------------------------- #
def _direct_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model, _, _ = _make_model("cpu", True)
        model.train()
        x = torch.zeros(5, len(VOCAB) + ND)
        # rank 0: 2 positives of 5 rows; rank 1: 1 of 5; rank 2: only a stand-in row (a positive one, weight 0)
        y = [torch.tensor([1., 0, 1, 0, 0]), torch.tensor([0., 0, 0, 1, 0]), torch.tensor([1.])][rank]
        model.__dict__["_row_weight"] = 0.0 if rank == 2 else 1.0
        model._sfg_bind_normaliser(x[:y.numel()], y)                 # what train_on_batch does first: ONE all-reduce
        norm = model.sfg_norm_labels(y)
        got = [model.sfg_normaliser(y), float(norm.numel()), float((norm == 1).sum())]
        model.sfg_positive_only = False
        got.append(model.sfg_normaliser(y))
        model._global_batch_labels(torch.tensor([1., 1, 1, 0, 0, 0, 0]))      # what fit hands over wins, no collective
        model.sfg_positive_only = True
        model._sfg_bind_normaliser(x[:y.numel()], y)
        got.append(model.sfg_normaliser(y))
        model.eval()                                                 # no SFG branch outside training: the step's own labels
        model._sfg_bind_normaliser(x[:y.numel()], y)
        got.append(model.sfg_normaliser(y))
        np.save(os.path.join(out_dir, "direct%d.npy" % rank), np.array(got))
    finally:
        dist.destroy_process_group()


def test_train_on_batch_called_directly_exchanges_the_count(tmp_path):
    """Without `fit` the global labels are unknown: the ranks exchange (positives, rows) and every rank divides by the same
    global count; a stand-in row counts for nothing."""
    _spawn(_direct_worker, (3, _free_port(), str(tmp_path)), 3, limit=60.0)
    own = [2, 1, 1]
    for r in range(3):
        got = np.load(str(tmp_path / ("direct%d.npy" % r)))
        np.testing.assert_array_equal(got, [3 + 1e-8, 10.0, 3.0, 10.0, 3 + 1e-8, own[r] + 1e-8])


def test_normaliser_buffers_outlive_any_number_of_batch_sizes(monkeypatch):
    """A captured first half reads the global labels through the address of the buffer of its global batch size and is
    keyed on nothing that knows the buffer, so the model never releases one: after a dozen other sizes (ragged tails of
    `fit` calls on other data, direct calls) the first size still finds its first buffer, at its first address."""
    from xdfm_amd import pro
    model, _, _ = _make_model("cpu", True)
    model.train()
    monkeypatch.setattr(pro.xdist, "current", lambda: object())      # a process group exists; handed labels need no collective
    x = torch.zeros(4, len(VOCAB) + ND)

    def bind(n):
        model._global_batch_labels(torch.arange(n) % 3 == 1)
        model._sfg_bind_normaliser(x, torch.zeros(4))
        return model.__dict__["_sfg_norm_y"]
    first = bind(64)
    ptr = first.data_ptr()
    others = [bind(n) for n in range(5, 18)]                          # 13 further sizes
    assert len({b.data_ptr() for b in others} | {ptr}) == 14
    again = bind(64)
    assert again is first and again.data_ptr() == ptr and again.numel() == 64
    assert int((again == 1).sum()) == 21 and model.sfg_normaliser(torch.zeros(4)) == 21 + 1e-8
    assert all(model.__dict__["_sfg_norm_bufs"][(n, x.device)] is b for n, b in zip(range(5, 18), others))
