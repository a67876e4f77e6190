"""GPU driver of the cases of head_w_ref.py: one forward and backward of the output head through xdfm_head_fwd_w /
xdfm_head_bwd_w (or the _ex entry points) with every output inside guard cells and both workspaces filled with NaN.
Below it the fixed list of cases behind test_gpu_head_w_abi.py::test_head_w_twice_in_a_row_bit_for_bit."""
import numpy as np
import torch

import head_ex_ref as X
import head_reg_drivers as D
import head_w_ref as W
from head_reg_drivers import _p, _put, _stream

OUTPUTS = ("pred", "loss", "dlin", "du", "dv", "grads")


def run_head_w(c, mode, dev, w=None, entry="w"):
    """-> dict of numpy arrays: pred [B], loss [1], dlin [B] (the kernel's own g, always asked for), du / dv (operands
    present), grads [Ku + Kv + 1] = dwu | dwv | dbias, and guards (bool: every guard cell around the outputs and both
    workspaces intact).  entry "w": the _w entry points with `w` (a float32 array, or None for a NULL pointer); "ex": the
    _ex entry points (w must be None).  The workspaces hold NaN before the calls: the kernels must not read what they
    have not written."""
    from xdfm_amd import _lib
    lib = _lib.load()
    t = {k: _put(c[k], dev) for k in ("lin", "u", "wu", "v", "wv", "bias")}
    y = _put(c["y"], dev)
    wt = _put(w, dev)
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
    o["ws_f"].fill_(float("nan"))
    o["ws"].fill_(float("nan"))
    fwd = (_p(t["lin"]), _p(t["u"]), _p(t["wu"]), Ku, _p(t["v"]), _p(t["wv"]), Kv, _p(t["bias"]), _p(y), B, _p(o["pred"]),
           _p(o["loss"]), _p(o["ws_f"]), mode[0], mode[1])
    bwd = (_p(o["pred"]), _p(y), _p(gl), _p(t["u"]), _p(t["wu"]), Ku, _p(t["v"]), _p(t["wv"]), Kv, B, _p(o["dlin"]),
           _p(o.get("du")), _p(o.get("dv")), _p(o["grads"]), _p(o["ws"]), mode[0], mode[1])
    if entry == "w":
        _lib.check(lib.xdfm_head_fwd_w(*fwd, _p(wt), _stream()), "head_fwd_w")
        _lib.check(lib.xdfm_head_bwd_w(*bwd, _p(wt), _stream()), "head_bwd_w")
    else:
        assert entry == "ex" and w is None
        _lib.check(lib.xdfm_head_fwd_ex(*fwd, _stream()), "head_fwd_ex")
        _lib.check(lib.xdfm_head_bwd_ex(*bwd, _stream()), "head_bwd_ex")
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy().copy() for k in OUTPUTS if k in o}
    if "du" in out:
        out["du"] = out["du"].reshape(B, Ku)
    if "dv" in out:
        out["dv"] = out["dv"].reshape(B, Kv)
    out["guards"] = all(D.guards_intact(v[0]) for v in bufs.values())
    return out


# the weighted head's (sigmoid, bce), (identity, mse) and (sigmoid, mae) instantiations on a vectorised and on a scalar case
# that run more than one sweep
REPEAT_MODES = [(X.LINK_SIGMOID, X.LOSS_BCE), (X.LINK_IDENTITY, X.LOSS_MSE), (X.LINK_SIGMOID, X.LOSS_MAE)]
REPEAT_CASES = [(2049, 8, 32, True), (513, 7, 0, False)]


def run_cases(dev):
    """Every (mode, case) of the two lists twice in a row -> {"head/<mode>/<case>/<rep>/<output>": array}."""
    out = {}
    for mode in REPEAT_MODES:
        for case in REPEAT_CASES:
            c, w = W.make_w_case(case, mode[0])
            for rep in (0, 1):
                for k, v in run_head_w(c, mode, dev, w).items():
                    out["head/%s/%s/%d/%s" % (W.mode_id(mode), W.w_case_id(case), rep, k)] = np.asarray(v)
    return out
