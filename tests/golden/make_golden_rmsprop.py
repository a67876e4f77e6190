#!/usr/bin/env python3
"""Generate tests/golden/rms_<case>.npz by RUNNING THE REFERENCE with `compile("rmsprop")`
(deepctr/models/basemodel.py:447-461: torch.optim.RMSprop with torch's defaults).

make_golden_optim.py's recipe (make_golden.py's import recipe and MODEL_CASES reused): the livelier copy of the weights, the
batches of model_<case>.npz (both checked here, array by array), three optimizer steps exactly as BaseModel.fit does them
(basemodel.py:241-262).  The file records the class and the defaults compile() gave (`optim_class`, `lr0`, `alpha`, `eps`);
then every param group gets lr = 1e-4 -- what the trainer does with --learning_rate -- before the three steps (`lr`).

Why 1e-4: with the BCE *sum* loss the default 0.01 makes the run blow up (total loss of x3_cin 24.9 -> 538 -> 392), and the
reference in fp32 and in fp64 then part by more than the tests' bars (rtol 1e-3 / atol 2e-5) in up to 5 elements per tensor;
at 1e-3 two tensors of x3_cin still have such elements; at 1e-4 none has (worst element: 0.54 of the bar, x3_cin).  The
worst share of the bar between the two runs is printed and recorded (`bar_share_32_vs_64`).

The fp64 run's final state is stored too, in a companion file rms64_<case>.npz: with it inside, rms_x3_cin.npz would be
1.9 MB, and a committed file may not exceed 1 MiB.  For the same reason it is stored as the float32 difference to the fp32
run's state (`s3_64_minus_s3:*`; s3_64 = float64(s3) + float64(difference), exact to 1e-12 here -- asserted below).
Runs only where the reference is available; the .npz files are data.
Usage:  python tests/golden/make_golden_rmsprop.py
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
LR = 1e-4
RTOL, ATOL = 1e-3, 2e-5                       # the bars of the model golden tests (state after three steps)


def _run(cls, vocab, nd, D, cin, dnn, B, kw, dtype):
    torch.manual_seed(1234)
    sparse, dense, cols = _columns(vocab, nd, D)
    model = cls(cols, cols, dnn_hidden_units=dnn, cin_layer_size=cin, l2_reg_dnn=1e-5, device="cpu", **kw)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k or k == "linear_model.weight" or "dnn" in k or k == "cin_linear.weight":
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    state0 = {k: _np(v) for k, v in model.state_dict().items()}
    if dtype == torch.float64:
        model.double()
    X, y = orc.synthetic_batch(3 * B, vocab, nd, seed=2025)
    model.compile("rmsprop", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    grp = model.optim.param_groups[0]
    given = dict(optim_class=type(model.optim).__name__, lr0=grp["lr"], alpha=grp["alpha"], eps=grp["eps"])
    for pg in model.optim.param_groups:
        pg["lr"] = LR
    model.train()
    losses = []
    for s in range(3):
        xb = torch.from_numpy(X[s * B:(s + 1) * B]).to(dtype)
        yb = torch.from_numpy(y[s * B:(s + 1) * B]).to(dtype)
        yp = model(xb).squeeze()
        model.optim.zero_grad()
        l = torch.nn.functional.binary_cross_entropy(yp, yb.squeeze(), reduction="sum")
        tot = l + model.get_regularization_loss() + model.aux_loss
        losses.append([l.item(), tot.item()])
        tot.backward()
        model.optim.step()
    return X, y, state0, given, losses, {k: _np(v) for k, v in model.state_dict().items()}


def gen_rmsprop():
    for name, cls, vocab, nd, D, cin, dnn, B, kw in mg.MODEL_CASES:
        if name not in CASES:
            continue
        X, y, state0, given, losses, s3 = _run(cls, vocab, nd, D, cin, dnn, B, kw, torch.float32)
        _, _, _, _, losses64, s3_64 = _run(cls, vocab, nd, D, cin, dnn, B, kw, torch.float64)
        base = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
        assert np.array_equal(base["X"], X) and np.array_equal(base["y"], y) and int(base["B"]) == B, name
        for k, v in state0.items():
            assert np.array_equal(base["s0:" + k], v), (name, k)
        share = max(float((np.abs(s3[k].astype(np.float64) - s3_64[k]) / (ATOL + RTOL * np.abs(s3_64[k]))).max())
                    for k in s3 if s3[k].size)
        print("%s: fp32 against fp64 reference run, worst share of the bar %.4f; losses %s" % (name, share, losses))
        assert share < 1.0, (name, share)
        arrays = dict(base=np.array(name), B=np.array(B), losses3=np.array(losses), losses3_64=np.array(losses64),
                      optimizer=np.array("rmsprop"), optim_class=np.array(given["optim_class"]), lr0=np.array(given["lr0"]),
                      alpha=np.array(given["alpha"]), eps=np.array(given["eps"]), lr=np.array(LR),
                      bar_share_32_vs_64=np.array(share), vocab=np.array(vocab), n_dense=np.array(nd), emb_dim=np.array(D),
                      cin=np.array(cin), dnn=np.array(dnn), cls=np.array(cls.__name__), kw_keys=np.array(sorted(kw.keys())),
                      kw_vals=np.array([kw[k] for k in sorted(kw)]))
        wide = dict(base=np.array(name), losses3_64=np.array(losses64))
        for k, v in s3.items():
            arrays["s3:" + k] = v
            d = (s3_64[k] - v.astype(np.float64)).astype(np.float32)
            assert v.size == 0 or float(np.abs(v.astype(np.float64) + d - s3_64[k]).max()) < 1e-11, (name, k)
            wide["s3_64_minus_s3:" + k] = d
        _save("rms_%s" % name[len("model_"):], **arrays)
        _save("rms64_%s" % name[len("model_"):], **wide)


if __name__ == "__main__":
    torch.set_num_threads(4)
    gen_rmsprop()
