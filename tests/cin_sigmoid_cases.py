"""The fixed backward cases behind tests/test_gpu_cin_sigmoid.py: xdfm_cin_dout_det and the fused xdfm_cin_bwd_prep
(+ xdfm_cin_level_bwd_w_prepared) with act = 2 (sigmoid), every call twice.

make_case(name) builds the inputs on the CPU from a seed; run_cases(dev) runs every case and returns the outputs as numpy
arrays.

ACT_CASES are the cases of tests/test_gpu_cin_f32_instances.py for act = 0 (linear) and 1 (ReLU), built by the same
make_case: hidden rows that start at hid0 > 0, rows with neither gradient source, a non-zero dbias before the call, the call
in place (dOut is A) and the atomic finish (ws = NULL) beside the workspace one.  run_cases(dev, ACT_CASES) runs those
instead of CASES."""
import ctypes

import numpy as np

SIGMOID = 2
LINEAR, RELU = 0, 1
# name: (H, B, D, split, dir_mode, cin_math, Hp, m)   Hp = 0: xdfm_cin_dout_det alone; otherwise the fused pass with the dW
#                                                      operands of a level (Hp, m) -- shapes of tests/test_gpu_cin_instances.py
CASES = {
    "dout_split_pooled": (37, 300, 4, True, 0, 1, 0, 0),         # float4 path, hidden and direct-connect halves, gradient of the pooled sum
    "dout_nosplit_scalar": (12, 77, 5, False, 0, 1, 0, 0),       # D = 5: the scalar path; every row has both gradient sources
    "dout_nosplit_fm": (20, 1100, 4, False, 1, 1, 0, 0),         # N = 4400: two blocks per row; feature-map layout of dDirect
    "prep_f16x3_split_pooled": (100, 512, 4, True, 0, 1, 13, 8),
    "prep_bf16_nosplit_fm": (65, 750, 4, False, 1, 2, 21, 8),
}
# name: (H, B, D, act, hid0, hid_rows, dir0, dir_rows, dir_mode): xdfm_cin_dout_det / xdfm_cin_dout alone, cin_math 0.  Rows outside
#       [hid0, hid0 + hid_rows) and [dir0, dir0 + dir_rows) have no gradient source: dOut exactly 0, dbias unchanged
ACT_CASES = {
    "relu_vec_hid0_gap": (37, 300, 4, RELU, 5, 12, 20, 15, 0),          # float4 path; rows 0-4, 17-19, 35-36 without a source
    "relu_scalar_d5": (12, 77, 5, RELU, 3, 7, 0, 7, 0),                 # D = 5: the scalar path; rows 3-6 have both sources, 10-11 none
    "relu_vec_two_blocks_fm": (9, 1100, 4, RELU, 2, 6, 0, 5, 1),        # N = 4400 > 4096: two float4 blocks per row; row 8 without a source
    "linear_vec_hid0_gap": (21, 260, 4, LINEAR, 4, 10, 9, 8, 1),        # rows 0-3, 17-20 without a source
    "linear_scalar_two_blocks": (11, 300, 5, LINEAR, 1, 6, 5, 5, 0),    # N = 1500 > 1024: two scalar blocks per row; row 0, 10 empty
}


def make_case(name):
    """fp32 inputs.  Sigmoid: A in [0, 1] with exact 0.0 and 1.0 and the fp32 neighbours of both within 2^-24.  ReLU: A =
    max(z, 0) with exact 0.0 and -0.0 (gradient 0) and the smallest positive values (gradient passes).  Linear: A of both
    signs (not read for its value).  dHid / dDirect of both signs with exact zeros."""
    if name in ACT_CASES:
        H, B, D, act, hid0, hid_rows, dir0, dir_rows, dir_mode = ACT_CASES[name]
        math, Hp, m = 0, 0, 0
        rng = np.random.default_rng(sorted(ACT_CASES).index(name) + 97)
    else:
        H, B, D, split, dir_mode, math, Hp, m = CASES[name]
        act, hid0 = SIGMOID, 0
        hid_rows = H // 2 if split else H
        dir0, dir_rows = (hid_rows, H - hid_rows) if split else (0, H)
        rng = np.random.default_rng(sorted(CASES).index(name) + 41)
    N = B * D
    if act == SIGMOID:
        A = (1.0 / (1.0 + np.exp(-2.5 * rng.standard_normal((H, N))))).astype(np.float32)
        special = np.array([0.0, 1.0, 2.0 ** -24, 2.0 ** -25, 0.25, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -23, 0.5], dtype=np.float32)
    else:
        A = rng.standard_normal((H, N)).astype(np.float32)
        if act == RELU:
            A = np.maximum(A, np.float32(0.0))
        special = np.array([0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 1.0, 2.0 ** -24, 3.0, 0.5], dtype=np.float32)
    pos = rng.choice(H * N, size=8 * special.size, replace=False)
    A.reshape(-1)[pos] = np.tile(special, 8)
    dhid = rng.standard_normal((hid_rows, N)).astype(np.float32)
    dhid[rng.random(dhid.shape) < 0.05] = 0.0
    dir_off = 3
    if dir_mode == 0:
        ddir = rng.standard_normal((B, dir_off + dir_rows + 2)).astype(np.float32)          # [example][pooled feature map]
    else:
        ddir = rng.standard_normal((dir_off + dir_rows, N)).astype(np.float32)              # feature-map layout
    ddir[rng.random(ddir.shape) < 0.05] = 0.0
    c = dict(name=name, H=H, B=B, D=D, N=N, math=math, Hp=Hp, m=m, A=A, dhid=dhid, ddir=ddir, hid_rows=hid_rows, dir0=dir0,
             dir_rows=dir_rows, dir_off=dir_off, dir_mode=dir_mode, act=act, hid0=hid0)
    if name in ACT_CASES:
        c["dbias0"] = rng.integers(-4, 5, H).astype(np.float32) + np.float32(0.5)       # never zero
    if Hp:
        c["xp"] = rng.standard_normal((Hp, N)).astype(np.float32)
        c["x0"] = rng.standard_normal((m, N)).astype(np.float32)
    return c


def sources64(c):
    """float64 (dHid, dDirect) spread over [H, N]: zero where a row has no such source"""
    H, N, D = c["H"], c["N"], c["D"]
    gh, gd = np.zeros((H, N)), np.zeros((H, N))
    gh[c["hid0"]:c["hid0"] + c["hid_rows"]] = c["dhid"]
    rows = slice(c["dir0"], c["dir0"] + c["dir_rows"])
    if c["dir_mode"] == 0:
        gd[rows] = np.repeat(c["ddir"][:, c["dir_off"]:c["dir_off"] + c["dir_rows"]].T.astype(np.float64), D, axis=1)
    else:
        gd[rows] = c["ddir"][c["dir_off"]:c["dir_off"] + c["dir_rows"]]
    return gh, gd


def _run(c, dev):
    import torch
    from xdfm_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    H, B, D, N, Hp, m = c["H"], c["B"], c["D"], c["N"], c["Hp"], c["m"]
    A, dhid, ddir = (torch.from_numpy(c[k]).to(dev) for k in ("A", "dhid", "ddir"))
    lddir = ddir.shape[1]
    p = lambda t: t.data_ptr()
    out = {}
    old = _lib.get_option("cin_math")
    _lib.set_option("cin_math", c["math"])
    act, hid0 = c["act"], c["hid0"]
    # the cases with a dbias0: a third call in place (dOut is A), and a fourth through xdfm_cin_dout (ws = NULL: atomics)
    reps = (0, 1, "inplace", "atomic") if "dbias0" in c else (0, 1)
    try:
        for rep in reps:
            dOut = A.clone() if rep == "inplace" else torch.full((H, N), 7.0, device=dev)
            src = dOut if rep == "inplace" else A
            dbias = torch.from_numpy(c["dbias0"]).to(dev) if "dbias0" in c else torch.zeros(H, device=dev)
            if rep == "atomic":
                _lib.check(lib.xdfm_cin_dout(p(src), H, B, D, act, p(dhid), hid0, c["hid_rows"], p(ddir), c["dir_mode"], lddir,
                                             c["dir_off"], c["dir0"], c["dir_rows"], p(dOut), p(dbias), st), "cin_dout")
            elif not Hp:
                ws = torch.empty(lib.xdfm_cin_dout_ws_elems(H, B, D), dtype=torch.float32, device=dev)
                _lib.check(lib.xdfm_cin_dout_det(p(src), H, B, D, act, p(dhid), hid0, c["hid_rows"], p(ddir), c["dir_mode"], lddir,
                                                 c["dir_off"], c["dir0"], c["dir_rows"], p(dOut), p(dbias), p(ws), st), "cin_dout_det")
            else:
                xp, x0 = torch.from_numpy(c["xp"]).to(dev), torch.from_numpy(c["x0"]).to(dev)
                dws = torch.empty(lib.xdfm_cin_bwd_prep_ws_elems(H, Hp, m, B, D), dtype=torch.float32, device=dev)
                ws = torch.empty(lib.xdfm_cin_bwd_w_ws_elems(H, Hp, m, N), dtype=torch.float32, device=dev)
                flag = ctypes.c_int(0)
                _lib.check(lib.xdfm_cin_bwd_prep(p(A), None, 0, H, B, D, act, p(dhid), hid0, c["hid_rows"], p(ddir), c["dir_mode"], lddir,
                                                 c["dir_off"], c["dir0"], c["dir_rows"], p(dOut), p(dbias), p(dws), p(xp), p(x0), Hp, m,
                                                 p(ws), ctypes.byref(flag), st), "cin_bwd_prep")
                assert flag.value == 1, "%s: the fused pass did not prepare the dW operands" % c["name"]
                dW = torch.full((H, Hp * m), 7.0, device=dev)
                _lib.set_option("last_bww_inst", -1)
                _lib.check(lib.xdfm_cin_level_bwd_w_prepared(p(dOut), p(xp), p(x0), H, Hp, m, N, p(ws), p(dW), st),
                           "cin_level_bwd_w_prepared")
                out["%s/%d/dW" % (c["name"], rep)] = dW.cpu().numpy()
                out["%s/%d/bww_inst" % (c["name"], rep)] = np.array(_lib.get_option("last_bww_inst"))
            torch.cuda.synchronize()
            out["%s/%s/dOut" % (c["name"], rep)] = dOut.cpu().numpy()
            out["%s/%s/dbias" % (c["name"], rep)] = dbias.cpu().numpy()
    finally:
        _lib.set_option("cin_math", old)
    return out


def run_cases(dev, cases=None):
    out = {}
    for name in (CASES if cases is None else cases):
        out.update(_run(make_case(name), dev))
    return out

