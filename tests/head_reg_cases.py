"""The fixed list of cases behind test_gpu_head_reg.py::test_finish_cases_repeat_bit_for_bit.

run_cases(dev) runs every kernel family of csrc/reg.hip and csrc/adam.hip that leaves per-block partials to a finish (the
Adam step over 70 tensors, the head, the column sums) twice in a row, then six train steps of a small xDeepFM (eager, the
capture, graph replays), and returns all outputs as numpy arrays."""
import numpy as np

import adam_ref as A
import head_reg_drivers as D
import head_reg_ref as R

HEAD = ["c1111", "c0000", "k3_k4_b16", "k512_k200_b2048", "k516_k64_b2049", "k64_k4_b65536"]     # both kernels each way
COLSUM = [(1000, 429), (4099, 63), (16, 65600)]
TRAIN_STEPS = 6                # 2 eager steps, the capture, 3 replays


def _train(dev, out):
    import torch
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from oracle import xdeepfm_oracle as orc
    vocab, nd, D = [50, 31, 77, 12, 9, 40], 3, 8
    cols = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]
    torch.manual_seed(1234)
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=(16, 8), l2_reg_dnn=1e-4, l2_reg_embedding=1e-4,
                    device=dev)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    for s in range(TRAIN_STEPS):
        X, y = orc.synthetic_batch(256, vocab, nd, seed=300 + s)
        res = model.train_on_batch(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
        out["train/step%d_pred" % s] = res[0].detach().cpu().numpy().copy()
        out["train/step%d_loss" % s] = res[1].detach().cpu().numpy().copy()
        out["train/step%d_total" % s] = res[2].detach().cpu().numpy().copy()
    for k, v in model.state_dict().items():
        out["train/final_" + k] = v.detach().cpu().numpy().copy()
    return model.__dict__["_graphed_step"].replays


def _adam70(dev, out):
    """The 70-tensor Adam step of test_gpu_adam.py (two launches; the finish sums the L2 partials of both), with l2_value,
    twice in a row."""
    state = A.make_state_70()
    for rep in (0, 1):
        snap, values = A.run_70(dev, True, state=state)
        for s, v in enumerate(values):
            out["adam70/%d/l2_step%d" % (rep, s + 1)] = v
        small = [t for t, n in enumerate(A.SIZES_70) if n <= 40989]
        for k, name in enumerate("pmv"):
            out["adam70/%d/%s" % (rep, name)] = np.concatenate([snap[t][k] for t in small])


def run_cases(dev):
    out = {}
    _adam70(dev, out)
    for name in HEAD:
        c = R.make_head_case(name)
        for rep in (0, 1):
            for k, v in D.run_head(c, dev).items():
                out["head/%s/%d/%s" % (name, rep, k)] = v
        if c["lin"] is None:                                  # the backward of a case ops.Head cannot differentiate
            g, db = D.head_g_aux(out["head/%s/1/pred" % name], c["y"], c["gloss"], dev)
            out["head/%s/aux_g" % name], out["head/%s/aux_dbias" % name] = g, np.array(db)
    for rows, cols in COLSUM:
        for relu in (False, True):
            g, y = R.make_colsum_case(rows, cols, relu)
            for rep, r in enumerate(D.run_colsum(g, y, cols, dev)):
                tag = "colsum%s/%dx%d/%d" % ("_relu" if relu else "", rows, cols, rep)
                out[tag + "/out"] = r["out"]
                out[tag + "/guards"] = np.array(int(r["guards"]))
                if relu:
                    out[tag + "/gz"] = r["gz"]
    out["meta/replays"] = np.array(_train(dev, out))
    return out

