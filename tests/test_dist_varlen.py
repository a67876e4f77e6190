"""Row-parallel training (xdfm_amd/dist.py) of a model with VarLenSparseFeat columns.

The pooled fields ride on the gather's row exchange: every rank runs K2v once over all ranks' rows
(xdfm_varlen_pool_bwd_rows), so their table gradients are identical on every rank and equal to the single-process gradient
on the global batch.  CPU test (gloo, 2 ranks): the plan is built, the one case without an exchange is refused.  GPU tests
(gloo, all ranks on cuda:0, at most 4 of them): `fit` against the single-process run, replicas bit for bit, the captured
first half against the eager one, and the gradient of one step bit for bit."""
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, ROOT

VOCAB, VV, TLEN, D = [9, 6, 12], 11, 5, 4
CIN, DNN = (8, 4), (8,)
SPAWN_LIMIT_S = 240
VARLEN_KEYS = ["%s.%s.weight" % (mod, n) for mod in ("embedding_dict", "linear_model.embedding_dict") for n in ("g_sum", "g_mean", "g_max")]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(fn, args, world):
    """mp.spawn with a time limit: the workers are killed and the test fails when they are not done in time."""
    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + SPAWN_LIMIT_S
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the %d workers did not finish within %d s" % (world, SPAWN_LIMIT_S))


def _columns():
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from deepctr.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    sparse = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(VOCAB)]
    varlen = [VarLenSparseFeat(SparseFeat("g_sum", VV, D), maxlen=TLEN, combiner="sum", length_name="g_sum_len"),
              VarLenSparseFeat(SparseFeat("g_mean", VV, D), maxlen=TLEN, combiner="mean"),
              VarLenSparseFeat(SparseFeat("g_max", VV, D), maxlen=TLEN, combiner="max")]
    return sparse, varlen, [DenseFeat("I1", 1)]


def _make_model(device, stock=False):
    """stock: a torch.optim object instead of the native table optimizer -- no L2 term in the optimizer, so no split step:
    the row exchange then runs inside the gather's backward."""
    from deepctr.models import xDeepFM
    sparse, varlen, dense = _columns()
    cols = sparse + varlen + dense
    model = xDeepFM(cols, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, l2_reg_dnn=1e-5, device=device)
    model.compile(torch.optim.Adam(model.parameters()) if stock else "adam", "binary_crossentropy", metrics=["binary_crossentropy"])
    for pg in model.optim.param_groups:
        pg["lr"] = 1e-2
    return model


def _data(n_rows, seed=5):
    """Feed dict and labels: ids of the sparse columns, id != 0 masked sequences, a length-masked one whose padded
    positions hold ids too, empty and full sequences among them."""
    rng = np.random.default_rng(seed)
    feed = {"C%d" % (i + 1): rng.integers(0, v, n_rows).astype(np.float32) for i, v in enumerate(VOCAB)}
    L = rng.integers(0, TLEN + 1, n_rows)
    L[:2] = [0, TLEN]
    feed["g_sum"] = rng.integers(0, VV, (n_rows, TLEN)).astype(np.float32)
    feed["g_sum_len"] = L.astype(np.float32)
    for name, lo in (("g_mean", 0), ("g_max", 1)):
        L = rng.integers(lo, TLEN + 1, n_rows)
        ids = rng.integers(1, VV, (n_rows, TLEN))
        ids[np.arange(TLEN)[None, :] >= L[:, None]] = 0
        feed[name] = ids.astype(np.float32)
    feed["I1"] = rng.standard_normal(n_rows).astype(np.float32)
    y = (rng.random(n_rows) < 0.4).astype(np.float32)
    return feed, y


def _state(model):
    state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    step = model.__dict__.get("_graphed_step")
    state["__replays__"] = np.array([step.replays if step is not None else 0])
    return state


def _fit(device, per_rank_bs, runs, stock=False):
    """`runs` = [(n_rows, epochs)]: one model, one `fit` per entry."""
    model = _make_model(device, stock)
    for k, (n_rows, epochs) in enumerate(runs):
        feed, y = _data(n_rows, seed=5 + k)
        model.fit(feed, y, batch_size=per_rank_bs, epochs=epochs, verbose=0, shuffle=True)
    return _state(model), model


def _one_step_grads(device):
    """The data-loss gradients of the variable-length tables after one step on a global batch of 64 rows, taken before the
    optimizer runs, and the row gradients they are built from."""
    from xdfm_amd import dist as xdist
    from xdfm_amd import ops
    model = _make_model(device)
    feed, y = _data(64, seed=9)
    X, Y = model._resident([feed[n] for n in model.feature_index], y)
    model.train()
    dp = xdist.current()
    if dp is not None:
        X, Y = dp.shard(X), dp.shard(Y)
    y_pred, loss, stash = model._split_step_first(X.to(device), Y.to(device))
    (_, Xs, d_emb, d_dnn, d_lin) = stash[0][:5]
    mD = d_emb.shape[0] * D
    rows = d_dnn[:, :mD].view(-1, d_emb.shape[0], D) + d_emb.view(d_emb.shape[0], -1, D).permute(1, 0, 2)
    out = {"rows": rows.reshape(rows.shape[0], -1), "d_lin": d_lin.reshape(-1), "y_pred": y_pred.reshape(-1)}
    if dp is not None:
        out = {k: dp.gather_rows(v.contiguous()) for k, v in out.items()}
        dense_w = model.linear_model.weight
        ops.apply_stashed_scatter(stash, dense_w, model._gather_tables())
    named = dict(model.named_parameters())
    for k in VARLEN_KEYS:
        out["g:" + k] = named[k].grad
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}, model


def _gpu_worker(rank, world, port, out_dir, scenarios):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    keep = []         # RowParallel knows its replicated parameters by id(): a scenario's model outlives the next one's
    try:
        for name, graph_dp, runs in scenarios:
            os.environ["XDFM_HIP_GRAPH_DP"] = graph_dp
            res, model = _one_step_grads("cuda:0") if runs is None else _fit("cuda:0", 64 // world, runs, stock=name == "stock")
            keep.append(model)
            np.savez(os.path.join(out_dir, "%s_rank%d.npz" % (name, rank)), **res)
    finally:
        dist.destroy_process_group()


def _load(out_dir, name, world):
    return [dict(np.load(os.path.join(str(out_dir), "%s_rank%d.npz" % (name, r)))) for r in range(world)]


def _needs_gpu_and_graph():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if os.environ.get("XDFM_HIP_GRAPH", "1") == "0":
        pytest.skip("XDFM_HIP_GRAPH=0")


FIT_2 = [(150, 2)]                       # 2 full global batches of 64 and a ragged one of 22 rows per epoch
FIT_STOCK = [(150, 1)]


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    """ONE spawn of two ranks for the 2-rank tests: `fit` with the first half replayed, `fit` all eager, `fit` with a stock
    optimizer, one step."""
    _needs_gpu_and_graph()
    out = tmp_path_factory.mktemp("varlen_dp2")
    _spawn(_gpu_worker, (2, _free_port(), str(out), [("replay", "1", FIT_2), ("eager", "0", FIT_2), ("stock", "1", FIT_STOCK),
                                                      ("step", "0", None)]), 2)
    return out


# ------------------------------------------------------------------------------------------------- CPU
def _cpu_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from deepctr.models import xDeepFM
        from deepctr.xdeepfm_pro import xDeepFMPro
        from xdfm_amd import dist as xdist
        log = []
        dp = xdist.current()
        assert dp is not None and dp.world == 2
        model = _make_model("cpu")
        plan = model._gather_plan()                      # raised NotImplementedError before
        named = dict(model.named_parameters())
        owners = [named[k] for k in VARLEN_KEYS]
        assert model._fused_linear and model._vplan.gather is plan and model._vplan.exchanged()
        assert len(plan.varlen_owners) == 6 and all(a is b for a, b in zip(plan.varlen_owners, owners))
        assert all(id(p) in dp._replicated for p in owners)        # built from the exchanged rows: no second all-reduce
        log.append("built")
        sparse, varlen, dense = _columns()
        cols = sparse + varlen + dense
        other = xDeepFM(sparse + dense, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, device="cpu")
        try:
            other._gather_plan()
        except NotImplementedError as exc:
            log.append("mismatch: %s" % exc)
        try:
            xDeepFMPro(cols, cols, device="cpu")
        except NotImplementedError as exc:
            log.append("pro: %s" % exc)
        with open(os.path.join(out_dir, "rank%d.txt" % rank), "w") as fh:
            fh.write("\n".join(log))
    finally:
        dist.destroy_process_group()


def test_plan_is_built_under_two_ranks_and_the_case_without_an_exchange_is_refused(tmp_path):
    _spawn(_cpu_worker, (2, _free_port(), str(tmp_path)), 2)
    for rank in range(2):
        log = open(str(tmp_path / ("rank%d.txt" % rank))).read().split("\n")
        assert log[0] == "built"
        assert log[1].startswith("mismatch: row-parallel training takes VarLenSparseFeat columns only when"), log
        assert "same columns in the same order" in log[1] and "does not take" not in log[1]
        assert log[2].startswith("pro: xDeepFMPro does not take VarLenSparseFeat columns"), log


# ------------------------------------------------------------------------------------------------- GPU
def _replicas_equal(ranks):
    for r in ranks[1:]:
        assert sorted(r) == sorted(ranks[0])
        for k, v in ranks[0].items():
            np.testing.assert_array_equal(r[k], v, err_msg="replicas differ: " + k)


@pytest.mark.gpu
def test_fit_two_ranks_equals_single_process_and_the_eager_twin(two_ranks):
    """The bars are those of tests/test_dist.py::test_row_parallel_fit_equals_single_process_gpu."""
    _needs_gpu_and_graph()
    replay, eager = _load(two_ranks, "replay", 2), _load(two_ranks, "eager", 2)
    _replicas_equal(replay)
    _replicas_equal(eager)
    assert all(int(r["__replays__"][0]) >= 1 for r in replay) and all(int(r["__replays__"][0]) == 0 for r in eager)
    single, _ = _fit("cuda:0", 64, FIT_2)              # single process, global batch 64
    init = _state(_make_model("cuda:0"))
    for k in VARLEN_KEYS:
        assert not np.array_equal(single[k], init[k]), k + " was not trained"
        np.testing.assert_allclose(replay[0][k], single[k], rtol=1e-3, atol=2e-5, err_msg=k)
    for k, v in eager[0].items():
        if k != "__replays__":
            np.testing.assert_array_equal(replay[0][k], v, err_msg="replayed first half vs eager: " + k)


@pytest.mark.gpu
def test_fit_two_ranks_with_a_stock_optimizer_exchanges_inside_the_backward(two_ranks):
    """Without the L2 term in the optimizer the step is not split: the gather's backward exchanges the rows itself and the
    variable-length tables' gradients are accumulated from there, the L2 gradient on top.  Same bars."""
    _needs_gpu_and_graph()
    ranks = _load(two_ranks, "stock", 2)
    _replicas_equal(ranks)
    single, _ = _fit("cuda:0", 64, FIT_STOCK, stock=True)
    init = _state(_make_model("cuda:0"))
    for k in VARLEN_KEYS:
        assert not np.array_equal(single[k], init[k]), k + " was not trained"
        np.testing.assert_allclose(ranks[0][k], single[k], rtol=1e-3, atol=2e-5, err_msg=k)


@pytest.mark.gpu
def test_one_step_gradient_is_the_single_process_gradient_bit_for_bit(two_ranks):
    """The contract K2v over exchanged rows exists for: `.grad` of every variable-length table, before the optimizer runs,
    is the same on both ranks and equal to what one process computes on the global batch."""
    _needs_gpu_and_graph()
    ranks = _load(two_ranks, "step", 2)
    single, _ = _one_step_grads("cuda:0")
    for k in ("y_pred", "d_lin", "rows"):              # what the gradients are built from: printed, so that a miss names its origin
        print("%s: two ranks vs one process, max |diff| %.3g (max |value| %.3g)" % (
            k, float(np.abs(ranks[0][k] - single[k]).max()), float(np.abs(single[k]).max())))
    for k in VARLEN_KEYS:
        a, b, s = ranks[0]["g:" + k], ranks[1]["g:" + k], single["g:" + k]
        print("%s: max |grad| %.3g, two ranks vs one process max |diff| %.3g" % (k, float(np.abs(s).max()), float(np.abs(a - s).max())))
        assert np.abs(s).max() > 0
        assert torch.equal(torch.from_numpy(a), torch.from_numpy(b)), "ranks differ: " + k
    for k in VARLEN_KEYS:
        assert torch.equal(torch.from_numpy(ranks[0]["g:" + k]), torch.from_numpy(single["g:" + k])), "two ranks vs one process: " + k


@pytest.mark.gpu
def test_four_ranks_a_tail_smaller_than_the_world_and_ragged_shards(tmp_path):
    """131 rows = two global batches of 64 and a tail of 3: one rank has no row of it and ships a zero-weighted stand-in.
    Then 86 more rows in one epoch: a tail of 22 = 5 + 6 + 5 + 6, whose shorter shards are padded with zero rows.  Neither
    may move a table row (replicas bit-identical, the single-process result within the bars of tests/test_dist.py) nor
    raise the bad-id flag (`fit` would raise IndexError at the end of the epoch)."""
    _needs_gpu_and_graph()
    runs = [(131, 2), (86, 1)]
    _spawn(_gpu_worker, (4, _free_port(), str(tmp_path), [("fit", "1", runs)]), 4)
    ranks = _load(tmp_path, "fit", 4)
    _replicas_equal(ranks)
    single, _ = _fit("cuda:0", 64, runs)
    for k in VARLEN_KEYS:
        np.testing.assert_allclose(ranks[0][k], single[k], rtol=1e-3, atol=2e-5, err_msg=k)
