#!/usr/bin/env python3
"""Generate tests/golden/regression/{reg_xdeepfm_mse,reg_attn_mae,bin_xdeepfm_mse}.npz by RUNNING THE REFERENCE with
task="regression" (PredictionLayer without the sigmoid, deepctr/layers/core.py:150-160) and with the "mse" / "mae" losses
of compile() (F.mse_loss / F.l1_loss, deepctr/models/basemodel.py:463-480; summed over the batch, :254).

make_golden.py's import recipe is reused.  The files are data only and hold what the model_* goldens hold: the initial
state_dict after the constructor alone, the livelier weights (0.3 * randn, as make_golden.py), X and y, y_pred / loss / reg
and every gradient of step 1, the losses and the state after three Adam steps, predict.  They live in a directory of their
own because the tests of tests/golden/model_*.npz feed every such file to a binary / binary_crossentropy model.

Regression targets are real-valued, about 3 + 1.5 * randn; the binary file keeps 0 / 1 labels.

Two conditions are asserted here, printed, and recorded in every file:
  1. bar_share_32_vs_64: the model is also run in float64; the reference's own fp32 / fp64 difference uses at most 0.5 of
     each bar the GPU tests hold the product to (y_pred rtol 2e-5 / atol 1e-6; loss 2e-5 relative; gradients rtol 2e-4 /
     atol 2e-5 * max + 1e-9; state after three steps rtol 1e-3 / atol 2e-5; the losses of the three steps rtol 2e-5;
     predict rtol 1e-4 / atol 2e-6).
  2. min_abs_residual (the mae file): |pred - y| > 1e-3 on every row of every recorded step, in both precisions, so that no
     sgn(pred - y) can differ between two correct evaluations.
The seeds below are ones for which the reference alone meets both (Adam's first update is about +-lr whatever the
gradient's size, so an element whose gradient is rounding noise may move by 2 * lr differently in the two precisions;
a seed where that happens fails condition 1 and is not used).
Usage:  python tests/golden/make_golden_regression.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                      # noqa: E402  (registers the reference's deepctr package)
from make_golden import _np, _columns         # noqa: E402
from deepctr.models.xdeepfm import xDeepFM                      # noqa: E402
from deepctr.models.xdeepfm_attn import xDeepFMAttention        # noqa: E402
from oracle import xdeepfm_oracle as orc                        # noqa: E402

OUT = os.path.join(HERE, "regression")
VOCAB, ND, D, B = [7, 50, 11, 23], 2, 4, 6
CIN, DNN = (6, 4), (8, 4)
LOSSES = {"mse": torch.nn.functional.mse_loss, "mae": torch.nn.functional.l1_loss}
MIN_RESIDUAL = 1e-3
#        name               cls                task          loss   seed of the batch
CASES = [("reg_xdeepfm_mse", xDeepFM,          "regression", "mse", 2031),
         ("reg_attn_mae",    xDeepFMAttention, "regression", "mae", 2031),
         ("bin_xdeepfm_mse", xDeepFM,          "binary",     "mse", 2031)]


def _batch(task, seed):
    X, y = orc.synthetic_batch(3 * B, VOCAB, ND, seed=seed)
    if task == "regression":
        y = (3.0 + 1.5 * np.random.default_rng(seed).standard_normal(y.shape)).astype(np.float32)
    return X, y


def _run(cls, task, loss_name, seed, dtype):
    sparse, dense, cols = _columns(VOCAB, ND, D)
    model = cls(cols, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, l2_reg_dnn=1e-5, task=task, device="cpu")
    init = {k: _np(v) for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k or k == "linear_model.weight" or "dnn" in k or k == "cin_linear.weight":
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    X, y = _batch(task, seed)
    state0 = {k: _np(v) for k, v in model.state_dict().items()}
    if dtype == torch.float64:
        model.double()
    model.compile("adam", loss_name, metrics=["mse"])
    assert model.loss_func is LOSSES[loss_name]
    fn = LOSSES[loss_name]
    Xt, yt = torch.from_numpy(X[:B]).to(dtype), torch.from_numpy(y[:B]).to(dtype)
    model.train()
    y_pred = model(Xt)
    loss = fn(y_pred.squeeze(), yt.squeeze(), reduction="sum")
    reg = model.get_regularization_loss()
    model.optim.zero_grad()
    (loss + reg).backward()
    grads = {k: _np(p.grad) for k, p in model.named_parameters()}
    model.optim.zero_grad()
    losses, residual = [], float(np.abs(_np(y_pred).reshape(-1) - y[:B].reshape(-1)).min())
    for s in range(3):                         # three Adam steps exactly as BaseModel.fit does them (basemodel.py:241-262)
        xb = torch.from_numpy(X[s * B:(s + 1) * B]).to(dtype)
        yb = torch.from_numpy(y[s * B:(s + 1) * B]).to(dtype)
        yp = model(xb).squeeze()
        model.optim.zero_grad()
        l = fn(yp, yb.squeeze(), reduction="sum")
        tot = l + model.get_regularization_loss() + model.aux_loss
        losses.append([l.item(), tot.item()])
        residual = min(residual, float(np.abs(_np(yp).reshape(-1) - y[s * B:(s + 1) * B].reshape(-1)).min()))
        tot.backward()
        model.optim.step()
    state3 = {k: _np(v) for k, v in model.state_dict().items()}
    if dtype == torch.float32:
        pred_after = model.predict([X[:, i] for i in range(X.shape[1])], batch_size=B)
    else:
        model.eval()
        with torch.no_grad():
            pred_after = _np(model(torch.from_numpy(X).to(dtype)))
    return dict(X=X, y=y, init=init, state0=state0, y_pred=_np(y_pred), loss=loss.item(), reg=reg.item(), grads=grads,
                losses=losses, state3=state3, pred_after=np.asarray(pred_after), residual=residual)


def _share(got, want, rtol, atol):
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64).reshape(want.shape) - want) / (atol + rtol * np.abs(want))).max())


def shares_32_vs_64(r32, r64):
    s = {"y_pred": _share(r32["y_pred"], r64["y_pred"], 2e-5, 1e-6),
         "loss": _share(r32["loss"], r64["loss"], 2e-5, 0.0),
         "grad": max(_share(v, r64["grads"][k], 2e-4, 2e-5 * float(np.abs(r64["grads"][k]).max()) + 1e-9)
                     for k, v in r32["grads"].items()),
         "state3": max(_share(v, r64["state3"][k], 1e-3, 2e-5) for k, v in r32["state3"].items()),
         "losses3": _share(r32["losses"], r64["losses"], 2e-5, 0.0),
         "pred_after": _share(r32["pred_after"], r64["pred_after"], 1e-4, 2e-6)}
    return s


def gen(cases=CASES, write=True):
    ok = True
    os.makedirs(OUT, exist_ok=True)
    for name, cls, task, loss_name, seed in cases:
        r32, r64 = _run(cls, task, loss_name, seed, torch.float32), _run(cls, task, loss_name, seed, torch.float64)
        assert np.array_equal(r32["X"], r64["X"]) and all(np.array_equal(r32["state0"][k], r64["state0"][k]) for k in r32["state0"])
        shares = shares_32_vs_64(r32, r64)
        share, residual = max(shares.values()), min(r32["residual"], r64["residual"])
        print("%s (seed %d): fp32 against fp64 reference run, share of the bars %s; min |pred - y| %.4g; losses %s" % (
            name, seed, {k: round(v, 4) for k, v in shares.items()}, residual, r32["losses"]))
        good = share <= 0.5 and (loss_name != "mae" or residual > MIN_RESIDUAL)
        ok = ok and good
        if not write:
            continue
        assert share <= 0.5, (name, shares)
        if loss_name == "mae":
            assert residual > MIN_RESIDUAL, (name, residual)
        arrays = dict(X=r32["X"], y=r32["y"], B=np.array(B), y_pred=r32["y_pred"], loss=np.array(r32["loss"]),
                      reg=np.array(r32["reg"]), losses3=np.array(r32["losses"]), losses3_64=np.array(r64["losses"]),
                      pred_after=r32["pred_after"], vocab=np.array(VOCAB), n_dense=np.array(ND), emb_dim=np.array(D),
                      cin=np.array(CIN), dnn=np.array(DNN), cls=np.array(cls.__name__), task=np.array(task),
                      loss_name=np.array(loss_name), seed=np.array(seed), bar_share_32_vs_64=np.array(share),
                      min_abs_residual=np.array(residual), min_residual_required=np.array(MIN_RESIDUAL))
        for k, v in r32["init"].items():
            arrays["init:" + k] = v
        for k, v in r32["state0"].items():
            arrays["s0:" + k] = v
        for k, v in r32["grads"].items():
            arrays["g:" + k] = v
        for k, v in r32["state3"].items():
            arrays["s3:" + k] = v
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print("wrote regression/%-24s %7.1f KB" % (name + ".npz", os.path.getsize(path) / 1024.0))
    return ok


if __name__ == "__main__":
    torch.set_num_threads(4)
    if sys.argv[1:2] == ["--search"]:          # print which batch seeds meet both conditions; writes nothing
        for seed in range(2031, 2031 + int(sys.argv[2])):
            gen([(n, c, t, l, seed) for n, c, t, l, _ in CASES], write=False)
    else:
        gen()
