#!/usr/bin/env python3
"""Generate tests/golden/dnn_bn/{bn_xdeepfm_relu,bn_xdeepfm_sigmoid}.npz by RUNNING THE REFERENCE's xDeepFM with
dnn_use_bn=True (deepctr/layers/core.py:120-134: Linear -> BatchNorm1d -> activation -> Dropout) on a tiny model.

make_golden.py's import recipe is reused.  The files are data only and hold what the regression goldens hold -- the initial
state_dict after the constructor alone, the livelier weights (0.3 * randn; gamma in 0.5 .. 1.5, beta 0.3 * randn), X and y,
y_pred / loss / reg and every gradient of step 1, the losses and the state (parameters and batch-norm buffers) after three
Adam steps -- plus what lets the tower be checked alone, without the rest of the model: the
tower's input, its output and the gradients at both ends of step 1 (dnn_in, dnn_out, g:dnn_out, g:dnn_in).

A Linear in front of a BatchNorm1d has a bias whose gradient is identically zero in exact arithmetic (the batch mean is
subtracted right after it): what any implementation computes there is the rounding of its own sums, and Adam turns a
gradient of any size into a step of up to lr.  Those keys are listed in `zero_grad_keys`; the tests bound them (gradient
below `zero_grad_bound`, at most 3 * lr of movement in three steps) instead of comparing noise with noise, and every
comparison below leaves them out.  In training mode such a bias changes nothing downstream, with one exception:
running_mean averages batch mean + bias.  Two correct runs' biases differ by up to 2 * lr per step taken, the three steps'
forwards enter running_mean with the weights 0.081, 0.09 and 0.1 (momentum 0.1) after 0, 1 and 2 steps, so their
running_mean may differ by 0.09 * 2 lr + 0.1 * 4 lr = 0.58 lr: `running_mean_allowance`, added to that buffer's atol.
running_var does not see the bias.  An evaluation-mode prediction after the steps would inherit the same noise through
running_mean and is not recorded.

bar_share_32_vs_64, asserted here, printed and recorded: the model is also run in float64; the reference's own fp32 / fp64
difference uses at most 0.5 of each bar the tests hold the product to (those of make_golden_regression.py).
Usage:  python tests/golden/make_golden_bn.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                      # noqa: E402,F401  (registers the reference's deepctr package)
from make_golden import _np, _columns         # noqa: E402
from make_golden_regression import _share     # noqa: E402
from deepctr.models.xdeepfm import xDeepFM                      # noqa: E402
from oracle import xdeepfm_oracle as orc                        # noqa: E402

OUT = os.path.join(HERE, "dnn_bn")
VOCAB, ND, D, B = [7, 50, 11, 23], 2, 4, 8
CIN, DNN = (6, 4), (8, 5)
LR = 1e-3                                     # torch.optim.Adam's default, what compile("adam") builds
RM_ALLOWANCE = 0.58 * LR                      # see the docstring
#        name                  activation  seed of the batch
CASES = [("bn_xdeepfm_relu",    "relu",    2051),
         ("bn_xdeepfm_sigmoid", "sigmoid", 2051)]


def _zero_grad_keys(model):
    return ["dnn.linears.%d.bias" % i for i in range(len(model.dnn.linears))]


def _run(act, seed, dtype):
    sparse, dense, cols = _columns(VOCAB, ND, D)
    model = xDeepFM(cols, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, l2_reg_dnn=1e-5, dnn_use_bn=True, dnn_activation=act,
                    device="cpu")
    init = {k: _np(v) for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "dnn.bn" in k:
                p.copy_(0.5 + torch.rand(p.shape, generator=g) if k.endswith("weight") else 0.3 * torch.randn(p.shape, generator=g))
            elif "embedding_dict" in k or k == "linear_model.weight" or "dnn" in k or k == "cin_linear.weight":
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    X, y = orc.synthetic_batch(3 * B, VOCAB, ND, seed=seed)
    state0 = {k: _np(v) for k, v in model.state_dict().items()}
    if dtype == torch.float64:
        model.double()
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy"])
    fn = torch.nn.functional.binary_cross_entropy
    Xt, yt = torch.from_numpy(X[:B]).to(dtype), torch.from_numpy(y[:B]).to(dtype)
    model.train()
    ends = {}

    def hook(_mod, inp, out):
        ends["in"], ends["out"] = inp[0], out
        inp[0].retain_grad()
        out.retain_grad()

    h = model.dnn.register_forward_hook(hook)
    y_pred = model(Xt)
    h.remove()
    loss = fn(y_pred.squeeze(), yt.squeeze(), reduction="sum")
    reg = model.get_regularization_loss()
    model.optim.zero_grad()
    (loss + reg).backward()
    grads = {k: _np(p.grad) for k, p in model.named_parameters()}
    tower = dict(dnn_in=_np(ends["in"]), dnn_out=_np(ends["out"]), g_out=_np(ends["out"].grad), g_in=_np(ends["in"].grad))
    after1 = {k: _np(v) for k, v in model.state_dict().items() if "dnn.bn" in k and ("running" in k or "num_batches" in k)}
    model.optim.zero_grad()
    losses = []
    for s in range(3):                         # three Adam steps exactly as BaseModel.fit does them (basemodel.py:241-262)
        xb = torch.from_numpy(X[s * B:(s + 1) * B]).to(dtype)
        yb = torch.from_numpy(y[s * B:(s + 1) * B]).to(dtype)
        yp = model(xb).squeeze()
        model.optim.zero_grad()
        l = fn(yp, yb.squeeze(), reduction="sum")
        tot = l + model.get_regularization_loss() + model.aux_loss
        losses.append([l.item(), tot.item()])
        tot.backward()
        model.optim.step()
    state3 = {k: _np(v) for k, v in model.state_dict().items()}
    return dict(X=X, y=y, init=init, state0=state0, y_pred=_np(y_pred), loss=loss.item(), reg=reg.item(), grads=grads, tower=tower,
                after1=after1, losses=losses, state3=state3, zero=_zero_grad_keys(model))


def shares_32_vs_64(r32, r64):
    skip = set(r32["zero"])
    return {"y_pred": _share(r32["y_pred"], r64["y_pred"], 2e-5, 1e-6),
            "loss": _share(r32["loss"], r64["loss"], 2e-5, 0.0),
            "grad": max(_share(v, r64["grads"][k], 2e-4, 2e-5 * float(np.abs(r64["grads"][k]).max()) + 1e-9)
                        for k, v in r32["grads"].items() if k not in skip),
            "tower": max(_share(r32["tower"][k], r64["tower"][k], 2e-4, 2e-5 * float(np.abs(r64["tower"][k]).max()) + 1e-9)
                         for k in r32["tower"]),
            "state3": max(_share(v, r64["state3"][k], 1e-3, 2e-5 + (RM_ALLOWANCE if k.endswith("running_mean") else 0.0))
                          for k, v in r32["state3"].items() if k not in skip),
            "losses3": _share(r32["losses"], r64["losses"], 2e-5, 0.0)}


def zero_grad_bound(r64):
    """What rounding may leave in a gradient that is zero in exact arithmetic: the sum over B rows of fp32 values of the size
    of the largest weight gradient of the same layer, each off by half an ulp -- B * 2^-24 * that size, times 8 of margin."""
    big = max(float(np.abs(v).max()) for k, v in r64["grads"].items() if k.startswith("dnn.linears") and k.endswith("weight"))
    return 8.0 * B * 2.0 ** -24 * max(big, 1.0)


def gen(cases=CASES, write=True):
    ok = True
    os.makedirs(OUT, exist_ok=True)
    for name, act, seed in cases:
        r32, r64 = _run(act, seed, torch.float32), _run(act, seed, torch.float64)
        assert np.array_equal(r32["X"], r64["X"]) and all(np.array_equal(r32["state0"][k], r64["state0"][k]) for k in r32["state0"])
        shares = shares_32_vs_64(r32, r64)
        share, bound = max(shares.values()), zero_grad_bound(r64)
        noise = max(float(np.abs(r[1]["grads"][k]).max()) for r in (("32", r32), ("64", r64)) for k in r32["zero"])
        moved = max(float(np.abs(r32["state3"][k] - r32["state0"][k]).max()) for k in r32["zero"])
        print("%s (seed %d): fp32 against fp64 reference run, share of the bars %s; zero-gradient biases: |g| <= %.3g (bound %.3g), "
              "moved <= %.3g in three steps (3 lr = %.3g); losses %s" % (name, seed, {k: round(v, 4) for k, v in shares.items()}, noise,
                                                                        bound, moved, 3 * LR, r32["losses"]))
        good = share <= 0.5 and noise <= bound and moved <= 3 * LR * 1.0001
        ok = ok and good
        if not write:
            continue
        assert good, (name, shares, noise, bound, moved)
        arrays = dict(X=r32["X"], y=r32["y"], B=np.array(B), y_pred=r32["y_pred"], loss=np.array(r32["loss"]), reg=np.array(r32["reg"]),
                      losses3=np.array(r32["losses"]), losses3_64=np.array(r64["losses"]), running_mean_allowance=np.array(RM_ALLOWANCE),
                      vocab=np.array(VOCAB), n_dense=np.array(ND), emb_dim=np.array(D), cin=np.array(CIN), dnn=np.array(DNN),
                      cls=np.array("xDeepFM"), task=np.array("binary"), act=np.array(act), seed=np.array(seed), lr=np.array(LR),
                      bar_share_32_vs_64=np.array(share), zero_grad_keys=np.array(r32["zero"]), zero_grad_bound=np.array(bound),
                      dnn_in=r32["tower"]["dnn_in"], dnn_out=r32["tower"]["dnn_out"])
        arrays["g:dnn_out"], arrays["g:dnn_in"] = r32["tower"]["g_out"], r32["tower"]["g_in"]
        for k, v in r32["init"].items():
            arrays["init:" + k] = v
        for k, v in r32["state0"].items():
            arrays["s0:" + k] = v
        for k, v in r32["grads"].items():
            arrays["g:" + k] = v
        for k, v in r32["after1"].items():
            arrays["a1:" + k] = v
        for k, v in r32["state3"].items():
            arrays["s3:" + k] = v
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print("wrote dnn_bn/%-24s %7.1f KB" % (name + ".npz", os.path.getsize(path) / 1024.0))
    return ok


if __name__ == "__main__":
    torch.set_num_threads(4)
    if sys.argv[1:2] == ["--search"]:          # print which batch seeds meet the conditions; writes nothing
        for seed in range(2051, 2051 + int(sys.argv[2])):
            gen([(n, a, seed) for n, a, _ in CASES], write=False)
    else:
        gen()
