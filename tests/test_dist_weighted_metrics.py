"""Weighted metrics under row-parallel training, world_size 2 on one GPU (gloo, as tests/test_dist_sample_weight.py, whose
rows, weights and one-row tail batch are reused): the `weighted_*` and `val_weighted_*` History keys of 2 ranks must equal the
single-process run on the global batch -- the weight shard is gathered beside labels and predictions (dist.gather_rows), and
the stand-in row of the rank without rows in the tail batch is not part of it.  Rows in their given order: the one-row tail
batch is the last row, whose weight is not zero by construction (a step whose rows all weigh 0 has W = 0 and logs NaN).  The
model's train step needs a GPU, so there is no CPU variant of this test."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import test_dist as TD
import test_dist_sample_weight as TW

WEIGHTED = ["binary_crossentropy", "mse", "acc"]           # no per-batch AUC: the one-row tail batch holds one class


def _run(device, per_rank_bs):
    model, names, orc = TD._make_model(device, False)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy"], weighted_metrics=WEIGHTED)
    for pg in model.optim.param_groups:
        pg["lr"] = 1e-2
    X, y, Xv, yv = TD._data(orc, TW.N_ROWS)
    vw = TW._weights(len(yv))
    hist = model.fit({n: X[:, i] for i, n in enumerate(names)}, y, batch_size=per_rank_bs, epochs=2, verbose=2,
                     validation_data=({n: Xv[:, i] for i, n in enumerate(names)}, yv, vw), shuffle=False,
                     sample_weight=TW._weights(TW.N_ROWS), class_weight=TW.CLASS_WEIGHT)
    return {k: list(v) for k, v in hist.history.items()}


def _worker(rank, world, port, device, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hist = _run(device, 64 // world)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), hist_keys=np.array(sorted(hist)),
                 hist_vals=np.array([hist[k] for k in sorted(hist)]))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_weighted_history_of_two_ranks_equals_single_process_gpu(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world, device = 2, "cuda:0"
    assert TW.N_ROWS % 64 < world                                   # the tail batch is smaller than the world
    mp.spawn(_worker, args=(world, TD._free_port(), device, str(tmp_path)), nprocs=world, join=True)
    hist1 = _run(device, 64)                                        # single process, global batch 64
    wkeys = ["weighted_" + n for n in WEIGHTED]
    assert [k for k in hist1 if "weighted" in k] == wkeys + ["val_" + k for k in wkeys]
    ranks = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    keys = [str(k) for k in ranks[0]["hist_keys"]]
    assert keys == sorted(hist1)
    # the tolerances of test_dist.py::test_row_parallel_fit_equals_single_process_gpu
    np.testing.assert_allclose(ranks[0]["hist_vals"], np.array([hist1[k] for k in keys]), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(ranks[1]["hist_vals"], ranks[0]["hist_vals"], rtol=1e-6, atol=1e-7)
    assert np.isfinite(ranks[0]["hist_vals"]).all()
    # the weights did something to the weighted keys
    assert abs(hist1["weighted_binary_crossentropy"][0] - hist1["binary_crossentropy"][0]) > 1e-4
