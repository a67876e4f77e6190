"""Example weights under row-parallel training, world_size 2 on one GPU (gloo, as tests/test_dist.py): a weighted `fit`
(sample_weight and class_weight together) on 2 ranks must equal the single-process run on the global batch -- the weights
are sharded beside the labels (dist.RowParallel.shard) -- and leave bit-identical replicas.  129 rows at a global batch of
64: the last batch holds ONE row, fewer than the world, so one rank runs it on a zero-weighted stand-in row."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import test_dist as TD

N_ROWS = 129
CLASS_WEIGHT = {0: 1.0, 1: 2.5}


def _weights(n):
    r = np.random.default_rng(17)
    w = r.uniform(0.0, 3.0, n).astype(np.float32)
    w[r.uniform(size=n) < 0.15] = 0.0
    w[-1] = 1.75                      # whichever row ends up alone in the tail batch, the tail is not all zero by construction
    return w


def _make_model(device):
    """test_dist's model without its per-batch AUC: the one-row tail batch holds one class."""
    model, names, orc = TD._make_model(device, False)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy"])
    for pg in model.optim.param_groups:
        pg["lr"] = 1e-2
    return model, names, orc


def _run(device, per_rank_bs):
    model, names, orc = _make_model(device)
    X, y, Xv, yv = TD._data(orc, N_ROWS)
    hist = model.fit({n: X[:, i] for i, n in enumerate(names)}, y, batch_size=per_rank_bs, epochs=2, verbose=2,
                     validation_data=({n: Xv[:, i] for i, n in enumerate(names)}, yv), shuffle=True,
                     sample_weight=_weights(N_ROWS), class_weight=CLASS_WEIGHT)
    state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    return {k: list(v) for k, v in hist.history.items()}, state


def _worker(rank, world, port, device, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from xdfm_amd import dist as xdist
        seen = []
        shard = xdist.RowParallel.shard

        def spy(self, t):                              # which ranks ever ran on a stand-in row
            out = shard(self, t)
            seen.append(self.row_weight())
            return out
        xdist.RowParallel.shard = spy
        hist, state = _run(device, 64 // world)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), hist_keys=np.array(sorted(hist)),
                 hist_vals=np.array([hist[k] for k in sorted(hist)]), stand_in=np.array(int(0.0 in seen)),
                 **{"p:" + k: v for k, v in state.items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_weighted_row_parallel_fit_equals_single_process_gpu(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world, device = 2, "cuda:0"
    assert N_ROWS % 64 < world                                      # the tail batch is smaller than the world
    mp.spawn(_worker, args=(world, TD._free_port(), device, str(tmp_path)), nprocs=world, join=True)
    hist1, state1 = _run(device, 64)                                # single process, global batch 64
    ranks = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    assert sorted(int(r["stand_in"]) for r in ranks) == [0, 1], "exactly one rank must have run on a stand-in row"
    r0 = ranks[0]
    keys = [str(k) for k in r0["hist_keys"]]
    assert keys == sorted(hist1)
    # the tolerances of test_dist.py::test_row_parallel_fit_equals_single_process_gpu
    rtol, atol = 1e-3, 2e-5
    np.testing.assert_allclose(r0["hist_vals"], np.array([hist1[k] for k in keys]), rtol=rtol, atol=atol)
    for k, v in state1.items():
        np.testing.assert_allclose(r0["p:" + k], v, rtol=rtol, atol=atol, err_msg=k)
    for r in ranks[1:]:
        np.testing.assert_allclose(r["hist_vals"], r0["hist_vals"], rtol=1e-6, atol=1e-7)
        for k in state1:
            np.testing.assert_array_equal(r["p:" + k], r0["p:" + k], err_msg="replicas differ: " + k)
    # the weights did something: an unweighted run ends elsewhere
    model, names, orc = _make_model(device)
    X, y, _, _ = TD._data(orc, N_ROWS)
    model.fit({n: X[:, i] for i, n in enumerate(names)}, y, batch_size=64, epochs=2, verbose=0, shuffle=True)
    far = max(float(np.abs(v.detach().cpu().numpy() - state1[k]).max()) for k, v in model.state_dict().items())
    assert far > 100 * atol, far
