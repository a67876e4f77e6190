"""CPU: every f16x3 / bf16 instance of the CIN kernels that the sources build (csrc/cin_x3_fwd.h and the translation units
that instantiate it, cin_x3.hip, cin_x3_bwx_sym.hip, cin_x3_bww.hip) is reached by the GPU sweep of
tests/test_gpu_cin_instances.py, and every SWEEP row claims exactly the instances the host rules pick for its shape -- so
that a field count or a tile cannot be added untested, and a row cannot test something other than it says."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "xdeepfm-pytorch_amd", "csrc")
LDS = 160 * 1024                 # the launchers' LDS limit per workgroup
RING = 4                         # X3_BWX_RING (xdfm_internal.h)


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def code(T, NW, NT, SYM=False):
    """x3_inst_code (xdfm_internal.h): the value of the last_*_inst probes"""
    return T * 1000 + NW * 100 + NT * 10 + int(SYM)


def ceil_div(a, b):
    return -(-a // b)


def _waves(fr):
    """launch_x3 / launch_bwx3(_sym): NWMAX = FR % 8 == 0 ? 8 : 4 (FR = 1-KB LDS-DMA pieces of a ring stage)"""
    return (4, 8) if fr % 8 == 0 else (4,)


# ---- what the sources build ------------------------------------------------------------------------------------------
def sym_fields():
    line = re.search(r"bool x3_sym_m\(int m\)\s*\{[^}]*\}", _src("xdfm_internal.h")).group(0)
    return {int(v) for v in re.findall(r"m == (\d+)", line)}


def _fwd_arms(macro):
    src = _src("cin_x3_fwd.h")
    body = src[src.index("#define " + macro + "("):]
    end = body.find("\n\n")
    body = body if end < 0 else body[:end]
    arms = re.findall(r"launch_x3<(\d+),\s*MV,\s*(\d+)", body)
    assert len(arms) == body.count("launch_x3<"), "unparsed arm in " + macro
    return {(int(mt), int(nt)) for mt, nt in arms}


def built_fwd():
    """{(m, instance code)} of cin_fwd_x3_kernel"""
    ms = set()
    for f in ("cin_x3_fwd_ma.hip", "cin_x3_fwd_mb.hip", "cin_x3.hip"):
        ms |= {int(v) for v in re.findall(r"X3_FWD_DISPATCH_M\((\d+)\)", _src(f))}
    sym = {int(v) for v in re.findall(r"X3_FWD_DISPATCH_SYM\((\d+)\)", _src("cin_x3_fwd_sym.hip"))}
    assert sym == sym_fields(), "folded forward instances %s != x3_sym_m %s" % (sorted(sym), sorted(sym_fields()))
    out = set()
    for macro, fields, folded in (("X3_FWD_DISPATCH_M", ms, False), ("X3_FWD_DISPATCH_SYM", sym, True)):
        for mt, nt in _fwd_arms(macro):
            for nw in _waves((2 if nt == 3 else 1) * mt):
                out |= {(m, code(mt, nw, nt, folded)) for m in fields}
    return out


def _bwx_arms(body, launcher):
    """(HBT, NT) of the `case` / `default` lines of a dX dispatch; a case must launch its own HBT"""
    arms = re.findall(r"(case\s+(\d+)|default)\s*:\s*return\s+" + launcher + r"<(\d+),\s*(\d+)", body)
    n_default = len(re.findall(r"default\s*:\s*return\s+" + launcher + "<", body))
    assert len(arms) == len(re.findall(r"\bcase\s+\d+\s*:", body)) + n_default, "unparsed case line in the dX dispatch"
    out = set()
    for _, case, hbt, nt in arms:
        assert not case or case == hbt, "case %s launches HBT %s" % (case, hbt)
        out.add((int(hbt), int(nt)))
    return out


def _function(src, head):
    body = src[src.index(head):]
    return body[:body.index("\n}\n")]


def _bwx_codes(arms, folded):
    return {code(hbt, nw, nt, folded) for hbt, nt in arms for nw in _waves(min(hbt, 8) * (2 if nt == 3 else 1))}


def built_bwx():
    """instance codes of cin_bwd_x3_kernel (no field-count parameter), {(m, code)} of cin_bwd_x3_sym_kernel"""
    plain = _bwx_codes(_bwx_arms(_function(_src("cin_x3.hip"), "int x3_level_bwd_x("), "launch_bwx3"), False)
    src = _src("cin_x3_bwx_sym.hip")
    arms = _bwx_arms(_function(src, "static int dispatch_bwx3_sym("), "launch_bwx3_sym")
    ms = {int(v) for v in re.findall(r"dispatch_bwx3_sym<(\d+)>", _function(src, "int x3_level_bwd_x_sym("))}
    assert ms == sym_fields(), "folded dX instances %s != x3_sym_m %s" % (sorted(ms), sorted(sym_fields()))
    return plain, {(m, c) for m in ms for c in _bwx_codes(arms, True)}


def built_bww():
    calls = re.findall(r"BWW_LAUNCH(_SYM)?\((\d+),\s*(\d+)\);", _function(_src("cin_x3_bww.hip"), "int x3_level_bwd_w("))
    return {code(4, int(nw), int(nt), bool(s)) for s, nw, nt in calls}


# ---- the host rules, for one SWEEP row ---------------------------------------------------------------------------------
def expected(row):
    """(forward, dX, dW) instance codes the host picks for a row (0: the fp32-MFMA kernel), after x3_fwd_usable /
    x3_fwd_geom / launch_x3, x3_bwx_usable / x3_bwx_geom / launch_bwx3(_sym), x3_bww_usable / x3_bww_waves"""
    m, H, Hp, N, math, waves, fold, opts = row[:8]
    nt = {1: 3, 2: 1}[math]
    assert fold == 0 or Hp == m, "level 0 has x_prev = x0"
    assert H <= 256, "dX takes at most 256 rows per call"
    sym = fold == 1 and m in sym_fields()
    wide = waves != 4 and N >= 256 * 64                      # the 8-wave variants, where the ring stage allows them
    fwd = 0
    if 8 <= m <= 40 and m % 2 == 0 and H > (32 if nt == 3 else 64):
        t = ceil_div(H, 32)
        mt = 8 if t >= 8 else (4 if t > 2 else 2)
        cap = opts.get("x3_fwd_mt", 0)
        if cap in (2, 4) and mt > cap:
            mt = cap
        assert nt == 3 or mt >= 4, "no bf16 forward kernel for MT 2"
        fr = (2 if nt == 3 else 1) * mt
        fwd = code(mt, 8 if fr % 8 == 0 and wide else 4, nt, sym)
    bwx = 0
    if H > (16 if nt == 3 else 32):
        hb = ceil_div(H, 16)
        hbt = 16 if hb > 8 else (8 if hb > 4 else (4 if hb > 2 else 2))
        fr = min(hbt, 8) * (2 if nt == 3 else 1)
        lds8 = RING * fr * 1024 + 2 * 8 * m * 32 * 4
        assert RING * fr * 1024 + 8 * m * 32 * 4 <= LDS
        bwx = code(hbt, 8 if fr % 8 == 0 and wide and (sym or lds8 <= LDS) else 4, nt, sym)
    bww = code(4, 4 if waves == 4 else 8, nt, sym) if H > 64 and N % 4 == 0 and N >= 32 else 0
    return fwd, bwx, bww


def bww_splits(row):
    """(n-splits, columns of the last split, columns per split) of x3_bww_geometry(_sym) for a row"""
    m, H, Hp, N, math, waves, fold, opts = row[:8]
    nw = 4 if waves == 4 else 8
    if fold == 1 and m in sym_fields():
        tph = ceil_div(ceil_div(m // 2, 2), nw) * nw
    else:
        tph = ceil_div(ceil_div(m, 2) * ceil_div(Hp, 32), nw) * nw
    gx = ceil_div(H, 128) * tph // nw
    ns = opts.get("bww_nsplit", 0)
    if ns <= 0:
        ns = max((256 if nw == 8 else 512) // gx, 1)
    ns = min(ns, ceil_div(N, 32), 65535)
    per = ceil_div(ceil_div(N, ns), 32) * 32
    ns = ceil_div(N, per)
    return ns, ceil_div(N, 32) * 32 - (ns - 1) * per, per


# ---- the checks ---------------------------------------------------------------------------------------------------------
def test_every_cin_instance_is_in_the_gpu_sweep():
    from test_gpu_cin_instances import SWEEP
    fwd = built_fwd()
    plain, folded = built_bwx()
    bww = built_bww()
    assert len(fwd) >= 150 and len(plain) >= 12 and len(folded) >= 24 and len(bww) >= 8, (len(fwd), len(plain), len(folded), len(bww))
    got_fwd = {(r[0], r[8]) for r in SWEEP if r[8]}
    got_plain = {r[9] for r in SWEEP if r[9] and r[9] % 10 == 0}
    got_folded = {(r[0], r[9]) for r in SWEEP if r[9] % 10 == 1}
    got_bww = {r[10] for r in SWEEP if r[10]}
    for what, built, got in (("forward", fwd, got_fwd), ("dX", plain, got_plain), ("folded dX", folded, got_folded),
                             ("dW", bww, got_bww)):
        assert got == built, "%s instances missing from SWEEP: %s; in SWEEP but not built: %s" % (
            what, sorted(built - got), sorted(got - built))


def test_every_sweep_row_claims_what_the_host_rules_pick():
    from test_gpu_cin_instances import SWEEP
    assert len(set(r[:7] + (tuple(sorted(r[7].items())),) for r in SWEEP)) == len(SWEEP), "duplicate SWEEP row"
    for r in SWEEP:
        assert tuple(r[8:]) == expected(r), "row %s claims %s, the host picks %s" % (r[:8], r[8:], expected(r))


def test_the_sweep_holds_the_edges():
    from test_gpu_cin_instances import SWEEP
    Ns = {r[3] for r in SWEEP}
    assert {16383, 16384} <= Ns                                               # just under and at the 8-wave threshold
    assert any(n % 32 and n >= 16384 for n in Ns) and any(n % 128 and n % 32 == 0 for n in Ns)
    assert any(r[2] % 8 for r in SWEEP if r[8] and r[2] > 8)                   # ragged last x_prev block behind full ones
    assert any(r[2] % 32 for r in SWEEP if r[9])
    assert any(r[1] % 16 for r in SWEEP if r[8]) and any(r[1] % 32 == 16 for r in SWEEP if r[8])
    assert {8, 40} <= {r[0] for r in SWEEP if r[8]}
    for m, math in ((8, 1), (8, 2), (40, 1), (40, 2)):                        # both wave counts at the extreme field counts
        assert {4, 8} <= {r[8] // 100 % 10 for r in SWEEP if r[0] == m and r[4] == math and r[8] // 1000 >= 4}, (m, math)
    assert any(r[4] == 2 and r[1] == 64 for r in SWEEP) and any(r[4] == 2 and r[1] == 65 for r in SWEEP)
    assert {4, 6} <= {r[0] for r in SWEEP if r[8] == 0 and r[9]}              # even m < 8: forward falls back, dX does not
    assert any(r[3] % 4 and r[1] > 64 and r[10] == 0 for r in SWEEP)           # dW fallbacks: N % 4 != 0, N < 32
    assert any(r[3] < 32 and r[1] > 64 and r[10] == 0 for r in SWEEP)
    assert any(r[0] % 2 for r in SWEEP if r[9])                               # odd m: the dX kernel's last odd tile
    assert any(r[9] // 100 % 10 == 4 and r[3] >= 16384 and r[5] == 0 and r[9] // 1000 >= 8 for r in SWEEP)   # LDS rule
    assert {0, 1, 2} <= {r[6] for r in SWEEP}
    assert {4} <= {r[5] for r in SWEEP}
    assert {2, 4} <= {r[7].get("x3_fwd_mt", 0) for r in SWEEP}
    split = [bww_splits(r) for r in SWEEP if r[10]]
    assert any(r[7].get("bww_nsplit") == 1 for r in SWEEP if r[10])
    assert any(ns > 1 and last < per for ns, last, per in split)              # a short last n-split
    assert any(ns > 1 and last < per for (ns, last, per), r in zip(split, [r for r in SWEEP if r[10]]) if "bww_nsplit" in r[7])
