#!/usr/bin/env python3
"""Generate tests/golden/dnn_prelu/{prelu_xdeepfm,prelu_xdeepfm_bn}.npz by RUNNING THE REFERENCE's xDeepFM with
dnn_activation='prelu' (deepctr/layers/core.py:104-134: Linear -> [BatchNorm1d] -> nn.PReLU() -> Dropout), without and with
dnn_use_bn, on the tiny model of make_golden_bn.py.

make_golden.py's import recipe is reused.  The files are data only and hold what the batch-norm goldens hold: the initial
state_dict after the constructor alone (the slopes `dnn.activation_layers.{i}.weight`, shape [1], 0.25, and the key names),
the livelier weights (0.3 * randn; gamma in 0.5 .. 1.5, beta 0.3 * randn; the slopes 0.4 and -0.3: both signs), X and y,
y_pred / loss / reg and every gradient of step 1 (the slopes' included: the reference's filter puts them into the l2_reg_dnn
group, so their gradient carries the L2 term), the tower's two ends (dnn_in, dnn_out, g:dnn_out, g:dnn_in), the losses and the
state after three Adam steps.

The _bn case inherits make_golden_bn.py's treatment of the biases in front of a batch norm, whose gradient is zero in exact
arithmetic: `zero_grad_keys`, `zero_grad_bound`, `running_mean_allowance` (see there).  The plain case has no such key.

bar_share_32_vs_64, asserted here, printed and recorded: the model is also run in float64; the reference's own fp32 / fp64
difference uses at most 0.5 of each bar the tests hold the product to (those of make_golden_bn.py).
Usage:  python tests/golden/make_golden_prelu.py
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
import make_golden_bn as mb                   # noqa: E402
from deepctr.models.xdeepfm import xDeepFM                      # noqa: E402
from oracle import xdeepfm_oracle as orc                        # noqa: E402

OUT = os.path.join(HERE, "dnn_prelu")
VOCAB, ND, D, B, CIN, DNN, LR = mb.VOCAB, mb.ND, mb.D, mb.B, mb.CIN, mb.DNN, mb.LR
SLOPES = (0.4, -0.3)
#        name                use_bn  seed of the batch
CASES = [("prelu_xdeepfm",    False, 2051),
         ("prelu_xdeepfm_bn", True,  2051)]


def _run(use_bn, seed, dtype):
    sparse, dense, cols = _columns(VOCAB, ND, D)
    model = xDeepFM(cols, cols, dnn_hidden_units=DNN, cin_layer_size=CIN, l2_reg_dnn=1e-5, dnn_use_bn=use_bn, dnn_activation="prelu",
                    device="cpu")
    init = {k: _np(v) for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "dnn.activation_layers" in k:
                p.fill_(SLOPES[int(k.split(".")[2]) % len(SLOPES)])
            elif "dnn.bn" in k:
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
    l2_keys = [n for wl, _l1, l2 in model.regularization_weight if abs(l2 - 1e-5) < 1e-12 for n in
               (w[0] for w in wl if isinstance(w, tuple))]
    return dict(X=X, y=y, init=init, state0=state0, y_pred=_np(y_pred), loss=loss.item(), reg=reg.item(), grads=grads, tower=tower,
                after1=after1, losses=losses, state3=state3, zero=mb._zero_grad_keys(model) if use_bn else [], l2_keys=l2_keys)


def gen(cases=CASES, write=True):
    ok = True
    os.makedirs(OUT, exist_ok=True)
    for name, use_bn, seed in cases:
        r32, r64 = _run(use_bn, seed, torch.float32), _run(use_bn, seed, torch.float64)
        assert np.array_equal(r32["X"], r64["X"]) and all(np.array_equal(r32["state0"][k], r64["state0"][k]) for k in r32["state0"])
        slopes = [k for k in r32["init"] if "activation_layers" in k]
        assert slopes == ["dnn.activation_layers.%d.weight" % i for i in range(len(DNN))], slopes
        assert all(r32["init"][k].shape == (1,) and float(r32["init"][k][0]) == 0.25 for k in slopes)
        assert all(k[4:] in r32["l2_keys"] for k in slopes), r32["l2_keys"]          # the reference L2-regularises the slopes
        shares = mb.shares_32_vs_64(r32, r64)
        share, bound = max(shares.values()), mb.zero_grad_bound(r64)
        noise = max([float(np.abs(r["grads"][k]).max()) for r in (r32, r64) for k in r32["zero"]] + [0.0])
        moved = max([float(np.abs(r32["state3"][k] - r32["state0"][k]).max()) for k in r32["zero"]] + [0.0])
        print("%s (seed %d): fp32 against fp64 reference run, share of the bars %s; zero-gradient biases: |g| <= %.3g (bound %.3g), "
              "moved <= %.3g in three steps (3 lr = %.3g); losses %s" % (name, seed, {k: round(v, 4) for k, v in shares.items()}, noise,
                                                                        bound, moved, 3 * LR, r32["losses"]))
        good = share <= 0.5 and noise <= bound and moved <= 3 * LR * 1.0001
        ok = ok and good
        if not write:
            continue
        assert good, (name, shares, noise, bound, moved)
        arrays = dict(X=r32["X"], y=r32["y"], B=np.array(B), y_pred=r32["y_pred"], loss=np.array(r32["loss"]), reg=np.array(r32["reg"]),
                      losses3=np.array(r32["losses"]), losses3_64=np.array(r64["losses"]), running_mean_allowance=np.array(mb.RM_ALLOWANCE),
                      vocab=np.array(VOCAB), n_dense=np.array(ND), emb_dim=np.array(D), cin=np.array(CIN), dnn=np.array(DNN),
                      cls=np.array("xDeepFM"), task=np.array("binary"), act=np.array("prelu"), use_bn=np.array(use_bn), seed=np.array(seed),
                      lr=np.array(LR), slopes=np.array(SLOPES), l2_reg_dnn_keys=np.array(r32["l2_keys"]),
                      bar_share_32_vs_64=np.array(share), zero_grad_keys=np.array(r32["zero"], dtype=str), zero_grad_bound=np.array(bound),
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
        print("wrote dnn_prelu/%-24s %7.1f KB" % (name + ".npz", os.path.getsize(path) / 1024.0))
    return ok


if __name__ == "__main__":
    torch.set_num_threads(4)
    if sys.argv[1:2] == ["--search"]:          # print which batch seeds meet the conditions; writes nothing
        for seed in range(2051, 2051 + int(sys.argv[2])):
            gen([(n, b, seed) for n, b, _ in CASES], write=False)
    else:
        gen()
