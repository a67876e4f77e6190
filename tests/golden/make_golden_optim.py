#!/usr/bin/env python3
"""Generate tests/golden/optim_<optimizer>_<case>.npz by RUNNING THE REFERENCE with `compile("sgd")` and
`compile("adagrad")` (deepctr/models/basemodel.py:447-461).

Same recipe as make_golden.py's gen_models (whose import recipe and MODEL_CASES are reused): the livelier copy of the
weights, the same batches, three optimizer steps exactly as BaseModel.fit does them (basemodel.py:241-262).  The
starting weights and the batches are those of model_<case>.npz (checked here, array by array), so a file holds only
what the optimizer changes: the three losses and the weights after three steps.  Runs only where the reference is
available; the .npz files are data.
Usage:  python tests/golden/make_golden_optim.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                      # noqa: E402  (registers the reference's deepctr package)
from make_golden import _columns, _np, _save, orc   # noqa: E402

CASES = ("model_sum_small", "model_sum_c1", "model_x3_cin")
OPTIMIZERS = ("sgd", "adagrad")


def gen_optim():
    for name, cls, vocab, nd, D, cin, dnn, B, kw in mg.MODEL_CASES:
        if name not in CASES:
            continue
        for optimizer in OPTIMIZERS:
            torch.manual_seed(1234)
            sparse, dense, cols = _columns(vocab, nd, D)
            model = cls(cols, cols, dnn_hidden_units=dnn, cin_layer_size=cin, l2_reg_dnn=1e-5, device="cpu", **kw)
            g = torch.Generator().manual_seed(5)
            with torch.no_grad():
                for k, p in model.named_parameters():
                    if "embedding_dict" in k or k == "linear_model.weight" or "dnn" in k or k == "cin_linear.weight":
                        p.copy_(0.3 * torch.randn(p.shape, generator=g))
            X, y = orc.synthetic_batch(3 * B, vocab, nd, seed=2025)
            model.compile(optimizer, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
            state0 = {k: _np(v) for k, v in model.state_dict().items()}
            model.train()
            losses = []
            for s in range(3):
                xb = torch.from_numpy(X[s * B:(s + 1) * B]).float()
                yb = torch.from_numpy(y[s * B:(s + 1) * B]).float()
                yp = model(xb).squeeze()
                model.optim.zero_grad()
                l = torch.nn.functional.binary_cross_entropy(yp, yb.squeeze(), reduction="sum")
                tot = l + model.get_regularization_loss() + model.aux_loss
                losses.append([l.item(), tot.item()])
                tot.backward()
                model.optim.step()
            base = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
            assert np.array_equal(base["X"], X) and np.array_equal(base["y"], y) and int(base["B"]) == B, name
            for k, v in state0.items():
                assert np.array_equal(base["s0:" + k], v), (name, k)
            arrays = dict(base=np.array(name), B=np.array(B), losses3=np.array(losses), optimizer=np.array(optimizer),
                          optim_class=np.array(type(model.optim).__name__), lr=np.array(model.optim.param_groups[0]["lr"]),
                          vocab=np.array(vocab), n_dense=np.array(nd), emb_dim=np.array(D), cin=np.array(cin),
                          dnn=np.array(dnn), cls=np.array(cls.__name__), kw_keys=np.array(sorted(kw.keys())),
                          kw_vals=np.array([kw[k] for k in sorted(kw)]))
            for k, v in model.state_dict().items():
                arrays["s3:" + k] = _np(v)
            _save("optim_%s_%s" % (optimizer, name[len("model_"):]), **arrays)


if __name__ == "__main__":
    torch.set_num_threads(4)
    gen_optim()
