"""GPU driver of the cases of head_ex_ref.py: one forward and backward of the output head through the C ABI
(xdfm_head_fwd_ex / xdfm_head_bwd_ex, or the entry points without a mode) with every output inside guard cells.  Below it
the fixed list of cases behind test_gpu_head_ex.py::test_head_ex_twice_in_a_row_bit_for_bit."""
import numpy as np
import torch

import head_ex_ref as X
import head_reg_drivers as D
from head_reg_drivers import _p, _put, _stream

OUTPUTS = ("pred", "loss", "dlin", "du", "dv", "grads")


def run_head_ex(c, mode, dev, ex=True):
    """-> dict of numpy arrays: pred [B], loss [1], dlin [B] (the kernel's own g: always asked for, whether the case has
    a `lin` or not), du / dv (operands present), grads [Ku + Kv + 1] = dwu | dwv | dbias, and guards (bool: every guard
    cell around pred, loss, dlin, du, dv, grads and both workspaces intact).  ex=False calls xdfm_head_fwd / xdfm_head_bwd,
    which take no mode."""
    from xdfm_amd import _lib
    lib = _lib.load()
    mis = c["misalign"]
    t = {k: _put(c[k], dev, 1 if mis == k else 0) for k in ("lin", "u", "wu", "v", "wv", "bias")}
    for k, a in t.items():
        if a is not None:
            assert a.data_ptr() % 16 == (4 if mis == k else 0)
    y = _put(c["y"], dev)
    gl = torch.tensor([float(c["gloss"])], dtype=torch.float32, device=dev)
    B, Ku, Kv = c["B"], c["Ku"], c["Kv"]
    nws = lib.xdfm_head_ws_elems(Ku, Kv)
    bufs = {"pred": D._guarded(B, dev), "loss": D._guarded(1, dev), "dlin": D._guarded(B, dev),
            "grads": D._guarded(Ku + Kv + 1, dev), "ws_f": D._guarded(nws, dev), "ws": D._guarded(nws, dev)}
    if Ku:
        bufs["du"] = D._guarded(B * Ku, dev)
    if Kv:
        bufs["dv"] = D._guarded(B * Kv, dev)
    o = {k: v[1] for k, v in bufs.items()}
    fwd = (_p(t["lin"]), _p(t["u"]), _p(t["wu"]), Ku, _p(t["v"]), _p(t["wv"]), Kv, _p(t["bias"]), _p(y), B, _p(o["pred"]),
           _p(o["loss"]), _p(o["ws_f"]))
    bwd = (_p(o["pred"]), _p(y), _p(gl), _p(t["u"]), _p(t["wu"]), Ku, _p(t["v"]), _p(t["wv"]), Kv, B, _p(o["dlin"]),
           _p(o.get("du")), _p(o.get("dv")), _p(o["grads"]), _p(o["ws"]))
    if ex:
        _lib.check(lib.xdfm_head_fwd_ex(*fwd, mode[0], mode[1], _stream()), "head_fwd_ex")
        _lib.check(lib.xdfm_head_bwd_ex(*bwd, mode[0], mode[1], _stream()), "head_bwd_ex")
    else:
        _lib.check(lib.xdfm_head_fwd(*fwd, _stream()), "head_fwd")
        _lib.check(lib.xdfm_head_bwd(*bwd, _stream()), "head_bwd")
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy().copy() for k in OUTPUTS if k in o}
    if "du" in out:
        out["du"] = out["du"].reshape(B, Ku)
    if "dv" in out:
        out["dv"] = out["dv"].reshape(B, Kv)
    out["guards"] = all(D.guards_intact(v[0]) for v in bufs.values())
    return out


# the head's (identity, mse) and (sigmoid, mae) instantiations on a 17-row case and on one a row short of a grid stride
REPEAT_MODES = [(X.LINK_IDENTITY, X.LOSS_MSE), (X.LINK_SIGMOID, X.LOSS_MAE)]
REPEAT_CASES = ["c1111", "k4_k68_b2047"]


def run_cases(dev):
    """Every (mode, case) of the two lists twice in a row -> {"head/<mode>/<case>/<rep>/<output>": array}."""
    out = {}
    for mode in REPEAT_MODES:
        for name in REPEAT_CASES:
            c = X.make_ex_case(name, mode[0])
            for rep in (0, 1):
                for k, v in run_head_ex(c, mode, dev).items():
                    out["head/%s/%s/%d/%s" % (X.mode_id(mode), name, rep, k)] = np.asarray(v)
    return out


def build_golden_model(g, dev):
    """The model of a golden of tests/golden/regression/ (4 SparseFeat + 2 DenseFeat, the recorded class, task and layer
    sizes), constructed as its generator constructed the reference's."""
    from deepctr import models
    from deepctr.inputs import DenseFeat, SparseFeat
    D = int(g["emb_dim"])
    cols = [SparseFeat("C%d" % (i + 1), int(v), D) for i, v in enumerate(g["vocab"])]
    cols += [DenseFeat("I%d" % (i + 1), 1) for i in range(int(g["n_dense"]))]
    return getattr(models, str(g["cls"]))(cols, cols, dnn_hidden_units=tuple(int(v) for v in g["dnn"]),
                                          cin_layer_size=tuple(int(v) for v in g["cin"]), l2_reg_dnn=1e-5,
                                          task=str(g["task"]), device=dev)
