"""Row-parallel replay across epochs (xdfm_amd/graphstep.py), with plain xDeepFM.  The second half of a row-parallel step
runs eagerly and reads the parameters' `.grad`.  An eager step of another batch shape -- the ragged tail of an epoch, whose
shards are unequal and never captured -- points `.grad` at its own tensors, so every replay has to bind the gradient
tensors its graph writes again; otherwise the all-reduce and the optimizer read the tail's stale gradients.  That shows
only when a graph is replayed after a tail: two epochs in train mode, i.e. a `fit` without validation data (an evaluation
between the epochs leaves the model in eval mode, which changes the graph's signature and re-captures)."""
import os

import numpy as np
import pytest
import torch

from test_dist import ND, VOCAB, _free_port, _make_model, _needs_default_env
from test_dist_pro import _spawn

N_ROWS = 343            # global batch 64: 5 full batches (2 eager, then replays) and a tail of 23 = 11 + 12 rows per epoch


def _run(device, per_rank_bs):
    model, names, orc = _make_model(device, False)
    X, y = orc.synthetic_batch(N_ROWS, VOCAB, ND, seed=5)
    hist = model.fit({n: X[:, i] for i, n in enumerate(names)}, y, batch_size=per_rank_bs, epochs=2, verbose=2, shuffle=False)
    state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    step = model.__dict__.get("_graphed_step")
    return {k: list(v) for k, v in hist.history.items()}, state, step.replays if step is not None else 0


def _worker(rank, world, port, device, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hist, state, replays = _run(device, 64 // world)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), hist_keys=np.array(sorted(hist)), replays=np.array([replays]),
                 hist_vals=np.array([hist[k] for k in sorted(hist)]), **{"p:" + k: v for k, v in state.items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_replays_after_an_eager_tail_step_use_their_own_gradients(tmp_path):
    """Two ranks on one GPU against the single process, tests/test_dist.py's GPU bars; the second epoch is 5 replays that
    follow the first epoch's eager tail step."""
    _needs_default_env('graph')
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _spawn(_worker, (2, _free_port(), "cuda:0", str(tmp_path)), 2)
    hist1, state1, replays1 = _run("cuda:0", 64)
    ranks = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(2)]
    keys = [str(k) for k in ranks[0]["hist_keys"]]
    assert keys == sorted(hist1)
    want = np.array([hist1[k] for k in keys])
    print("history keys %s\n2 ranks:\n%s\nsingle process:\n%s" % (keys, ranks[0]["hist_vals"], want))
    replays = (int(ranks[0]["replays"][0]), int(ranks[1]["replays"][0]), replays1)
    assert min(replays) >= 8, replays                    # 3 in the first epoch, all 5 full batches of the second
    np.testing.assert_allclose(ranks[0]["hist_vals"], want, rtol=1e-3, atol=2e-5)
    for k, v in state1.items():
        np.testing.assert_allclose(ranks[0]["p:" + k], v, rtol=1e-3, atol=2e-5, err_msg=k)
        np.testing.assert_array_equal(ranks[1]["p:" + k], ranks[0]["p:" + k], err_msg="replicas differ: " + k)
