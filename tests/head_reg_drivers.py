"""GPU drivers of the cases of head_reg_ref.py: run a case through ops / the C ABI and hand back numpy arrays.  Shared by
test_gpu_head_reg.py and head_reg_cases.py."""
import ctypes

import numpy as np
import torch

GUARD, SENTINEL = 64, 12345.0
COL0_G, COL0_Y = 2, 3          # first column of the window inside g / y (the pitches of colsum_pitches leave room)


def _put(a, dev, off=0):
    """Device copy of `a` starting `off` floats past a 16-byte aligned address."""
    if a is None:
        return None
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def head_g_aux(pred, y, gloss, dev):
    """(g fp32 [B], dbias) from xdfm_head_bwd with no u and no v: the kernel's own g of a pred it produced, for the
    cases that have no `lin` and therefore no dlin."""
    from xdfm_amd import _lib
    lib = _lib.load()
    B = pred.size
    P, Y = _put(pred, dev), _put(y, dev)
    gl = torch.tensor([float(gloss)], dtype=torch.float32, device=dev)
    dlin = torch.empty(B, dtype=torch.float32, device=dev)
    grads = torch.empty(1, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.xdfm_head_ws_elems(0, 0), dtype=torch.float32, device=dev)
    _lib.check(lib.xdfm_head_bwd(_p(P), _p(Y), _p(gl), None, None, 0, None, None, 0, B, _p(dlin), None, None, _p(grads),
                                 _p(ws), _stream()), "head_bwd")
    torch.cuda.synchronize()
    return dlin.cpu().numpy(), grads.cpu().numpy()[0]


def run_head(c, dev):
    """One forward and backward of ops.Head on a case of make_head_case -> dict of numpy arrays (pred, loss, and the
    gradients of the operands present)."""
    from xdfm_amd import ops
    mis = c["misalign"]
    t = {k: _put(c[k], dev, 1 if mis == k else 0) for k in ("lin", "u", "wu", "v", "wv", "bias")}
    for k, a in t.items():
        if a is not None:
            assert a.data_ptr() % 16 == (4 if mis == k else 0)
            a.requires_grad_(True)
    y = _put(c["y"], dev)
    pred, loss = ops.Head.apply(y, t["bias"], t["lin"], t["u"], t["wu"], t["v"], t["wv"])
    out = {}
    if loss.requires_grad:
        loss.backward(torch.tensor([float(c["gloss"])], dtype=torch.float32, device=dev))
        for k, nm in (("lin", "dlin"), ("u", "du"), ("wu", "dwu"), ("v", "dv"), ("wv", "dwv"), ("bias", "dbias")):
            if t[k] is not None:
                out[nm] = t[k].grad.detach().cpu().numpy().copy()
    torch.cuda.synchronize()
    out["pred"], out["loss"] = pred.detach().cpu().numpy().copy(), loss.detach().cpu().numpy().copy()
    return out


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all())


def run_colsum(g, y, cols, dev, reps=2):
    """xdfm_colsum (y is None) or xdfm_relu_bwd_colsum on the column window of g (and y) that starts COL0 columns in.
    -> list of `reps` dicts (out, gz | None, guards: all guard cells of out, gz and the workspace intact)."""
    from xdfm_amd import _lib
    lib = _lib.load()
    rows = g.shape[0]
    G = torch.from_numpy(g).to(dev)
    Y = torch.from_numpy(y).to(dev) if y is not None else None
    res = []
    for _ in range(reps):
        wsb, ws = _guarded(lib.xdfm_colsum_ws_elems(cols), dev)
        ob, out = _guarded(cols, dev)
        if y is None:
            gw = G[:, COL0_G:]
            _lib.check(lib.xdfm_colsum(_p(gw), rows, cols, G.stride(0), _p(ws), _p(out), _stream()), "colsum")
            gzb = gz = None
        else:
            gw, yw = G[:, COL0_G:], Y[:, COL0_Y:]
            gzb, gz = _guarded(rows * cols, dev)
            _lib.check(lib.xdfm_relu_bwd_colsum(_p(gw), _p(yw), rows, cols, G.stride(0), Y.stride(0), _p(ws), _p(gz), _p(out),
                                                _stream()), "relu_bwd_colsum")
        torch.cuda.synchronize()
        ok = guards_intact(wsb) and guards_intact(ob) and (gzb is None or guards_intact(gzb))
        res.append(dict(out=out.cpu().numpy().copy(), gz=None if gz is None else gz.cpu().numpy().reshape(rows, cols).copy(),
                        guards=ok))
    return res



def run_l2(c, dev):
    """ops.L2Reg forward and backward on a case of l2_case -> (value fp32, [gradient arrays])."""
    from xdfm_amd import ops
    ts = [_put(w, dev, o).requires_grad_(True) for w, o in zip(c["ws"], c["offs"])]
    for t, o in zip(ts, c["offs"]):
        assert t.data_ptr() % 16 == 4 * o
    plan = ops.L2Plan([float(k) for k in c["coeffs"]])
    out = ops.L2Reg.apply(plan, None, 0, *ts)
    out.backward(torch.tensor([float(c["gs"])], dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy().copy()[0], [t.grad.cpu().numpy().copy() for t in ts]


def run_l2_accumulate(c, g0, dev):
    """xdfm_l2_reg_bwd with accumulate = 1 on the flat gradient g0 (fp32 [sum of sizes], tensor t at the running sum of
    the sizes) -> (flat gradient after the call, guard cells intact)."""
    from xdfm_amd import _lib
    lib = _lib.load()
    ts = [_put(w, dev, o) for w, o in zip(c["ws"], c["offs"])]
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    offs = np.concatenate([[0], np.cumsum(c["sizes"])[:-1]]).tolist()
    ptrs, numel, goff = i64([t.data_ptr() for t in ts]), i64(list(c["sizes"])), i64(offs)
    coeff = torch.from_numpy(c["coeffs"]).to(dev)
    gs = torch.tensor([float(c["gs"])], dtype=torch.float32, device=dev)
    fb, flat = _guarded(g0.size, dev)
    flat.copy_(torch.from_numpy(g0))
    _lib.check(lib.xdfm_l2_reg_bwd(_p(ptrs), _p(numel), _p(coeff), c["T"], _p(gs), _p(flat), _p(goff), 1, _stream()), "l2_reg_bwd")
    torch.cuda.synchronize()
    return flat.cpu().numpy().copy(), guards_intact(fb)
