#!/usr/bin/env python3
"""Generate tests/golden/sgdm/sgdm_sum_small_<variant>.npz by RUNNING THE REFERENCE with a torch.optim.SGD OBJECT handed to
compile() (deepctr/models/basemodel.py:447-461 takes an optimizer object as it is): momentum 0.9 (`mom`) and momentum 0.9 with
nesterov=True (`nes`).

make_golden_rmsprop.py's recipe on the `sum_small` configuration: the livelier copy of the weights, the batches of
model_sum_small.npz (both checked here, array by array), three optimizer steps exactly as BaseModel.fit does them
(basemodel.py:241-262).  The rate is 1e-4, set on the object: with the BCE *sum* loss a step of 0.01 times a summed gradient
leaves the range in which the fp32 and fp64 runs of the reference stay within the tests' bars (rtol 1e-3 / atol 2e-5) of each
other; the worst share of the bar between the two runs is printed and recorded (`bar_share_32_vs_64`), for the parameters and
for the momentum buffers.

The files record the final parameters (`s3:*`), the final momentum buffers (`buf3:*`, by parameter name) and the fp64 run's
final state as the float32 difference to the fp32 run's (`s3_64_minus_s3:*`, `buf3_64_minus_buf3:*`).  They live in a directory
of their own, so that no golden test that globs tests/golden/ by prefix picks them up.
Runs only where the reference is available; the .npz files are data.
Usage:  python tests/golden/make_golden_sgdm.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                      # noqa: E402  (registers the reference's deepctr package)
from make_golden import _columns, _np, orc    # noqa: E402

CASE = "model_sum_small"
OUT = os.path.join(HERE, "sgdm")
LR, MOMENTUM = 1e-4, 0.9
VARIANTS = {"mom": False, "nes": True}        # name -> nesterov
RTOL, ATOL = 1e-3, 2e-5                       # the bars of the model golden tests (state after three steps)


def _run(cls, vocab, nd, D, cin, dnn, B, kw, dtype, nesterov):
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
    optim = torch.optim.SGD(model.parameters(), lr=LR, momentum=MOMENTUM, nesterov=nesterov)
    model.compile(optim, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    assert model.optim is optim
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
    bufs = {k: _np(optim.state[p]["momentum_buffer"]) for k, p in model.named_parameters() if p in optim.state}
    return X, y, state0, losses, {k: _np(v) for k, v in model.state_dict().items()}, bufs


def _share(a32, a64):
    return max(float((np.abs(a32[k].astype(np.float64) - a64[k]) / (ATOL + RTOL * np.abs(a64[k]))).max()) for k in a32 if a32[k].size)


def gen_sgdm():
    os.makedirs(OUT, exist_ok=True)
    name, cls, vocab, nd, D, cin, dnn, B, kw = [c for c in mg.MODEL_CASES if c[0] == CASE][0]
    base = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    for variant, nesterov in sorted(VARIANTS.items()):
        X, y, state0, losses, s3, buf3 = _run(cls, vocab, nd, D, cin, dnn, B, kw, torch.float32, nesterov)
        _, _, _, losses64, s3_64, buf3_64 = _run(cls, vocab, nd, D, cin, dnn, B, kw, torch.float64, nesterov)
        assert np.array_equal(base["X"], X) and np.array_equal(base["y"], y) and int(base["B"]) == B, name
        for k, v in state0.items():
            assert np.array_equal(base["s0:" + k], v), (name, k)
        share = max(_share(s3, s3_64), _share(buf3, buf3_64))
        print("%s %s: fp32 against fp64 reference run, worst share of the bar %.4f; losses %s" % (name, variant, share, losses))
        assert share < 1.0, (name, variant, share)
        arrays = dict(base=np.array(name), B=np.array(B), losses3=np.array(losses), losses3_64=np.array(losses64),
                      optim_class=np.array("SGD"), lr=np.array(LR), momentum=np.array(MOMENTUM), nesterov=np.array(nesterov),
                      bar_share_32_vs_64=np.array(share), vocab=np.array(vocab), n_dense=np.array(nd), emb_dim=np.array(D),
                      cin=np.array(cin), dnn=np.array(dnn), cls=np.array(cls.__name__), kw_keys=np.array(sorted(kw.keys())),
                      kw_vals=np.array([kw[k] for k in sorted(kw)]))
        for k, v in s3.items():
            arrays["s3:" + k] = v
            arrays["s3_64_minus_s3:" + k] = (s3_64[k] - v.astype(np.float64)).astype(np.float32)
        for k, v in buf3.items():
            arrays["buf3:" + k] = v
            arrays["buf3_64_minus_buf3:" + k] = (buf3_64[k] - v.astype(np.float64)).astype(np.float32)
        path = os.path.join(OUT, "sgdm_%s_%s.npz" % (name[len("model_"):], variant))
        np.savez_compressed(path, **arrays)
        print("wrote %s %.1f KB" % (os.path.relpath(path, HERE), os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    torch.set_num_threads(4)
    gen_sgdm()
