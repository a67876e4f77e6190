"""Row-parallel training with dnn_use_bn=True and XDFM_DNN_BN_SYNC=1 (GPU, gloo, all ranks on cuda:0): N ranks must equal
the single-process native run on the global batches -- history and every state_dict entry, the batch-norm buffers among
them -- and leave bit-identical replicas.  The harness is that of tests/test_dist.py.

Model: the small xDeepFM of tests/test_dist.py with dnn_use_bn=True and dnn_hidden_units=(64, 40) (a width the native dense
kernels take and one they leave to the library), livelier tower weights (0.3 * randn, as the golden generators use) so that
the tower's pre-activations follow the inputs.  Rows: the dense features grow with the row index (checked on the inputs),
shuffle=False, so the contiguous shards of a global batch have different statistics; `_shard_statistics_differ` asserts
from the float64 reference on the CPU that per-shard normalisation of the first batch is more than 10 x the comparison
tolerance away from global normalisation -- on the parent commit, where the row-parallel tower normalises per shard, the
comparison of the running statistics could not pass.

Optimizer: SGD, lr 1e-2.  A Linear in front of a batch norm has a bias whose gradient is zero in exact arithmetic; what
any implementation computes there is the rounding of its own sums (1e-8 here), which Adam turns into steps of up to lr
with the sign of that rounding (tests/golden/make_golden_bn.py derives this and takes those keys out of its comparison).
Under SGD the same rounding moves such a bias by lr * 1e-8, so EVERY entry, those biases and the running_mean that averages
them included, is held to rtol 1e-3, atol 2e-5 -- the tolerances of test_row_parallel_fit_equals_single_process_gpu.

Runs, 2 epochs each, global batch 64.  World 2 with 150 rows (a ragged tail of 22 = 11 + 11) and validation data, after
which `fit` -- like the reference's -- stays in evaluation mode: its second epoch covers the evaluation route and its
backward under a row-parallel context.  World 4 with 131 rows, whose tail of 3 rows leaves one rank with a stand-in row
(count 0 forward, zero dz backward).  World 2 with dnn_activation='prelu', the second routing site of layers.DNN.  The
last two run without validation data, so that both epochs normalise with batch statistics.  At most 5 processes hold the
GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, ROOT

import dnn_bn_ref as B

pytestmark = pytest.mark.gpu

VOCAB, ND, D = [9, 6, 12, 5, 7], 2, 4
CIN, DNN = (6, 4), (64, 40)
GLOBAL_BS, EPOCHS = 64, 2
RTOL, ATOL = 1e-3, 2e-5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_model(device, act):
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    names = ["C%d" % (i + 1) for i in range(len(VOCAB))]
    dnames = ["I%d" % (i + 1) for i in range(ND)]
    cols = [SparseFeat(n, v, D) for n, v in zip(names, VOCAB)] + [DenseFeat(n, 1) for n in dnames]
    model = xDeepFM(cols, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, l2_reg_dnn=1e-5, dnn_use_bn=True, dnn_activation=act,
                    device=device)
    gen = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k or k.startswith("dnn.linears") or k == "dnn_linear.weight":
                p.copy_((0.3 * torch.randn(p.shape, generator=gen)).to(p.device))
    model.compile("sgd", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    for pg in model.optim.param_groups:
        pg["lr"] = 1e-2
    return model, names + dnames, orc


def _data(orc, n_rows):
    X, y = orc.synthetic_batch(n_rows, VOCAB, ND, seed=5)
    # the dense features grow with the row index: contiguous shards of a batch see different parts of their range
    for j in range(ND):
        X[:, len(VOCAB) + j] = (j + 1) * 3.0 * np.arange(n_rows, dtype=np.float64) / (n_rows - 1)
    Xv, yv = orc.synthetic_batch(40, VOCAB, ND, seed=6)
    return X, y, Xv, yv


def _run(device, per_rank_bs, n_rows, act, validate):
    from xdfm_amd import ops
    model, names, orc = _make_model(device, act)
    X, y, Xv, yv = _data(orc, n_rows)
    calls = {"sync_train": 0, "sync_eval": 0, "native": 0}
    real_sync, real_native = getattr(ops, "bn_act_sync"), ops._bn_act_native

    def sync(z, bn, a, training, dp):
        calls["sync_train" if training else "sync_eval"] += 1
        return real_sync(z, bn, a, training, dp)

    def native(z, bn, code, training):
        calls["native"] += 1
        return real_native(z, bn, code, training)

    ops.bn_act_sync, ops._bn_act_native = sync, native
    try:
        hist = model.fit({n: X[:, i] for i, n in enumerate(names)}, y, batch_size=per_rank_bs, epochs=EPOCHS, verbose=2,
                         validation_data=({n: Xv[:, i] for i, n in enumerate(names)}, yv) if validate else None, shuffle=False)
    finally:
        ops.bn_act_sync, ops._bn_act_native = real_sync, real_native
    state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    step = model.__dict__.get("_graphed_step")
    state["__replays__"] = np.array([step.replays if step is not None else 0])
    state["__calls__"] = np.array([calls["sync_train"], calls["sync_eval"], calls["native"]])
    return {k: list(v) for k, v in hist.history.items()}, state


def _worker(rank, world, port, device, out_dir, n_rows, per_rank_bs, act, validate):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["XDFM_DNN_BN_SYNC"] = "1"              # read once, when xdfm_amd.ops is imported (in _run, below)
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for p in (ROOT, PKG):
            if p not in sys.path:
                sys.path.insert(0, p)
        from xdfm_amd import ops
        assert ops.DNN_BN_SYNC is True, "the worker's environment did not reach the switch"
        hist, state = _run(device, per_rank_bs, n_rows, act, validate)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), hist_keys=np.array(sorted(hist)),
                 hist_vals=np.array([hist[k] for k in sorted(hist)]), **{"p:" + k: v for k, v in state.items()})
    finally:
        dist.destroy_process_group()


def _shard_statistics_differ(world, n_rows, act):
    """From the inputs and the initial weights alone, in float64 on the CPU: the first global batch normalised per shard (what
    a row-parallel tower without the feature computes) against normalised over the whole batch, behind the first dense
    layer.  Must differ by more than 10 x the tolerance the runs are compared with."""
    model, _, orc = _make_model("cpu", act)
    sd = {k: v.detach().double().numpy() for k, v in model.state_dict().items()}
    X = _data(orc, n_rows)[0]
    nv = len(VOCAB)
    for j in range(ND):
        assert np.all(np.diff(X[:, nv + j]) > 0), "dense feature %d must grow with the row index" % j
    xb = X[:GLOBAL_BS]
    emb = [sd["embedding_dict.C%d.weight" % (i + 1)][xb[:, i].astype(np.int64)] for i in range(nv)]
    dnn_in = np.concatenate(emb + [xb[:, nv:].astype(np.float64)], axis=1)
    z = dnn_in @ sd["dnn.linears.0.weight"].T + sd["dnn.linears.0.bias"]
    gamma, beta, zeros, ones = sd["dnn.bn.0.weight"], sd["dnn.bn.0.bias"], np.zeros(DNN[0]), np.ones(DNN[0])
    code = "linear" if act == "prelu" else act
    whole = B.fwd_train(z, gamma, beta, 1e-5, 0.1, code, zeros, ones)
    p = [(r * GLOBAL_BS) // world for r in range(world + 1)]
    parts = [B.fwd_train(z[p[r]:p[r + 1]], gamma, beta, 1e-5, 0.1, code, zeros, ones) for r in range(world)]
    y_parts = np.concatenate([q["y"] for q in parts])
    gap_y = np.abs(y_parts - whole["y"]) - 10 * (ATOL + RTOL * np.abs(whole["y"]))
    gap_rm = np.abs(parts[0]["running_mean"] - whole["running_mean"]) - 10 * (ATOL + RTOL * np.abs(whole["running_mean"]))
    print("per-shard vs global normalisation of the first batch: y off by up to %.3g, rank 0's running_mean by up to %.3g"
          % (float(np.abs(y_parts - whole["y"]).max()), float(np.abs(parts[0]["running_mean"] - whole["running_mean"]).max())))
    assert gap_y.max() > 0 and gap_rm.max() > 0, "the shards' statistics do not differ enough for this test to tell the routes apart"


def _check(tmp_path, world, n_rows, act="relu", validate=False):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _shard_statistics_differ(world, n_rows, act)
    device = "cuda:0"
    port = _free_port()
    mp.spawn(_worker, args=(world, port, device, str(tmp_path), n_rows, GLOBAL_BS // world, act, validate), nprocs=world, join=True)
    hist1, state1 = _run(device, GLOBAL_BS, n_rows, act, validate)                     # single process, global batch 64, native batch norm
    ranks = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    r0 = ranks[0]
    keys = [str(k) for k in r0["hist_keys"]]
    assert keys == sorted(hist1)
    # `fit` enters training mode once, before the first epoch, and the validation behind an epoch leaves the model in
    # evaluation mode (the reference's loop does the same): with validation data only the first epoch's steps normalise
    # with batch statistics, the second epoch's run the evaluation route -- and its backward -- on the running statistics
    per_epoch = -(-n_rows // GLOBAL_BS)
    steps = per_epoch if validate else EPOCHS * per_epoch
    calls1 = state1.pop("__calls__")
    state1.pop("__replays__")
    # (its later steps are graph replays, which do not pass through the Python of the tower)
    assert calls1[0] == 0 and calls1[2] >= len(DNN), "the single-process run must take the native batch norm: %r" % (calls1,)
    for r in ranks:
        sync_train, sync_eval, native = (int(v) for v in r["p:__calls__"])
        # once per batch-norm layer and training-mode step
        assert sync_train == len(DNN) * steps, (sync_train, len(DNN), steps)
        assert sync_eval >= (len(DNN) * (EPOCHS * per_epoch - steps + EPOCHS) if validate else 0), sync_eval
        assert native == 0, "a row-parallel tower must not take the single-process route"
        assert int(r["p:__replays__"][0]) == 0, "the step of a tower with a collective inside must launch eagerly"
    np.testing.assert_allclose(r0["hist_vals"], np.array([hist1[k] for k in keys]), rtol=RTOL, atol=ATOL)
    assert any(k.endswith("running_mean") for k in state1) and any(k.endswith("running_var") for k in state1)
    for k, v in state1.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == steps
        np.testing.assert_allclose(r0["p:" + k], v, rtol=RTOL, atol=ATOL, err_msg=k)
    for r in ranks[1:]:
        np.testing.assert_allclose(r["hist_vals"], r0["hist_vals"], rtol=1e-6, atol=1e-7)   # every rank logs the same
        for k in state1:
            np.testing.assert_array_equal(r["p:" + k], r0["p:" + k], err_msg="replicas differ: " + k)


def test_two_ranks_equal_the_single_process_run(tmp_path):
    """With validation data, as tests/test_dist.py runs `fit`: the first epoch trains on batch statistics, the second on the
    running statistics the first left (evaluation route, no collective)."""
    _check(tmp_path, 2, 150, validate=True)


def test_four_ranks_with_a_stand_in_row_in_the_tail(tmp_path):
    """131 rows = 2 full global batches + a tail of 3: split points 0 0 1 2 3 leave rank 0 with a stand-in row."""
    from xdfm_amd.dist import split_points
    p = split_points(131 % GLOBAL_BS, 4)
    assert min(b - a for a, b in zip(p, p[1:])) == 0
    _check(tmp_path, 4, 131)


def test_two_ranks_with_prelu_behind_the_batch_norm(tmp_path):
    _check(tmp_path, 2, 150, act="prelu")
