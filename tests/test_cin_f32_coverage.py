"""CPU: every fp32-MFMA (cin_math 0) instance of the CIN kernels that the dispatch of csrc/cin_fwd.hip and csrc/cin_bwd.hip can
launch is reached by the GPU sweep of tests/test_gpu_cin_f32_instances.py, every SWEEP_F32 row claims exactly the probe
values the host rules give for its shape, options and operand alignment, the edges the kernels' prefetch rings and
padding depend on are in the table, and the exact family's integers stay below 2^24 -- so that an instance or a dispatch
arm cannot be added without a row, and a row cannot test something other than it says."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "xdeepfm-pytorch_amd", "csrc")
LDS = 160 * 1024
OPTION_KEYS = {"fwd_nf", "dbg", "bww_mt", "bww_nsplit", "bww_slab"}
HOW_KEYS = {"act", "off", "math"}


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def ceil_div(a, b):
    return -(-a // b)


def _function(src, head):
    body = src[src.index(head):]
    return body[:body.index("\n}\n")]


# ---- what the dispatch can launch ------------------------------------------------------------------------------------
def built_fwd():
    """{(MT, NF, MPT)}: the launch_fwd<MT, NF> arms of xdfm_cin_level_fwd; inside launch_fwd the `MP ==` lines hand the
    field counts of the straight-line kernel to launch_fwd_mp<MT, NF, MPT> for MT >= the `if constexpr` threshold"""
    src = _src("cin_fwd.hip")
    body = _function(src, "int xdfm_cin_level_fwd(")
    arms = re.findall(r"launch_fwd<(\d+),\s*(\d+)>\(", body)
    assert len(arms) == body.count("launch_fwd<") and len(arms) == 5, "unparsed arm in xdfm_cin_level_fwd"
    lf = _function(src, "static int launch_fwd(")
    thr = re.findall(r"if constexpr \(MT >= (\d+)\)", lf)
    assert len(thr) == 1
    mps = re.findall(r"if \(MP == (\d+)\) return launch_fwd_mp<MT, NF, (\d+)>", lf)
    assert len(mps) == lf.count("MP ==") == lf.count("launch_fwd_mp<") and all(a == b for a, b in mps), "unparsed MP line"
    out = set()
    for mt, nf in arms:
        out.add((int(mt), int(nf), 0))
        if int(mt) >= int(thr[0]):
            out |= {(int(mt), int(nf), int(mp)) for mp, _ in mps}
    return out


def mp_fields():
    return {mpt for _, _, mpt in built_fwd() if mpt}


def _jb2_range():
    lf = _function(_src("cin_bwd.hip"), "static int launch_bwd_x(")
    cond = re.findall(r"HS4 <= (\d+) && HS4 >= (\d+) && m % 2 == 0 && \(xdfm_opt\(OPT_DBG\) & (\d+)\)", lf)
    assert len(cond) == 1 and lf.count("cin_bwd_x_kernel<HS4, 2>") == 1 and lf.count("cin_bwd_x_kernel<HS4, 1>") == 1
    return int(cond[0][1]), int(cond[0][0]), int(cond[0][2])


def built_bwx():
    """{(HS4, JB)}: the launch_bwd_x<HS4> cases of xdfm_cin_level_bwd_x_ex and the JB branch of launch_bwd_x"""
    body = _function(_src("cin_bwd.hip"), "int xdfm_cin_level_bwd_x_ex(")
    arms = re.findall(r"(case\s+(\d+)|default)\s*:\s*return\s+launch_bwd_x<(\d+)>", body)
    assert len(arms) == body.count("launch_bwd_x<"), "unparsed case of the dX dispatch"
    lo, hi, _ = _jb2_range()
    out = set()
    for _, case, hs4 in arms:
        assert not case or case == hs4
        out.add((int(hs4), 1))
        if lo <= int(hs4) <= hi:
            out.add((int(hs4), 2))
    return out


def built_bww():
    """{(MT, KV)}: the launch_bwd_w<MT> cases of xdfm_cin_level_bwd_w and the three kernel branches of launch_bwd_w
    (KV 1 = cin_bwd_w_kernel, 2 = cin_bwd_w_dma_kernel, 3 = cin_bwd_w_dma4_kernel, which its branch gives to MT 4 only)"""
    src = _src("cin_bwd.hip")
    body = _function(src, "int xdfm_cin_level_bwd_w(")
    arms = re.findall(r"(case\s+(\d+)|default)\s*:\s*return\s+launch_bwd_w<(\d+)>", body)
    assert len(arms) == body.count("launch_bwd_w<") == 3, "unparsed case of the dW dispatch"
    lw = _function(src, "static int launch_bwd_w(")
    kernels = re.findall(r"hipLaunchKernelGGL\(\((cin_bwd_w\w*_kernel)<MT, JT>\)", lw)
    assert kernels == ["cin_bwd_w_kernel", "cin_bwd_w_dma4_kernel", "cin_bwd_w_dma_kernel"], kernels
    only = re.findall(r"else if \(MT == (\d+) && N % 4 == 0 && !\(xdfm_opt\(OPT_DBG\) & 16\)", lw)
    assert len(only) == 1
    out = set()
    for _, case, mt in arms:
        assert not case or case == mt
        out |= {(int(mt), 1), (int(mt), 2)}
        if int(mt) == int(only[0]):
            out.add((int(mt), 3))
    return out


# ---- the host rules, for one SWEEP_F32 row ------------------------------------------------------------------------------
def fwd_mt(H):
    t = ceil_div(H, 32)
    return 8 if t >= 8 else (4 if t > 2 else t)


def fwd_mp(m):
    return (m + 1) // 2


def bwx_hs4(H):
    g, p = ceil_div(H, 8), 1
    while p < g:
        p *= 2
    return p


def bww_mt(H, opts):
    o = opts.get("bww_mt", 0)
    return o if o in (1, 2, 4) else (4 if H > 64 else (2 if H > 32 else 1))


def bww_geometry(row):
    """(MT, h-groups, workgroups per n-split, n-splits, columns per split) of bww_geometry (xdfm_internal.h)"""
    m, H, Hp, N, fold, opts = row[:6]
    mt = bww_mt(H, opts)
    IB, JP = ceil_div(Hp, 32), ceil_div(m, 2)
    tph = ceil_div(JP * IB, 4) * 4
    hg = ceil_div(H, 32 * mt)
    gx = hg * tph // 4
    ns = opts.get("bww_nsplit", 0)
    if ns <= 0:
        ns = max(512 // gx, 1)
    ns = min(ns, ceil_div(N, 32), 65535)
    per = ceil_div(ceil_div(N, ns), 32) * 32
    return mt, hg, gx, ceil_div(N, per), per


def last_dx_rows(H):
    """rows of the last dX call: the layer (and the sweep) walks H in calls of 256"""
    return H - 256 * ((H - 1) // 256)


def expected(row):
    """(last_fwd_f32, last_bwx_f32, last_bww_f32) after xdfm_cin_level_fwd / launch_fwd, xdfm_cin_level_bwd_x_ex /
    launch_bwd_x, xdfm_cin_level_bwd_w / launch_bwd_w; under cin_math 1 (how["math"]) 0 where x3_fwd_usable / x3_bwx_usable /
    x3_bww_usable hold"""
    m, H, Hp, N, fold, opts, how = row[:7]
    assert set(opts) <= OPTION_KEYS and set(how) <= HOW_KEYS
    assert fold in (0, 1) and (fold == 0 or Hp == m), "level 0 has x_prev = x0"
    dbg, f16x3 = opts.get("dbg", 0), how.get("math", 0) == 1
    assert how.get("math", 0) in (0, 1)
    assert dbg & ~(2 | 8 | 16 | 32) == 0, "dbg bits 1 and 4 are timing experiments (wrong results / LDS size)"
    # forward
    mt, mp = fwd_mt(H), fwd_mp(m)
    nf = 2 if opts.get("fwd_nf", 1) == 2 and mt == 4 else 1
    mpt = mp if mt >= 4 and not dbg & 2 and mp in mp_fields() else 0
    if not mpt:
        assert 4 * (2 * mp + 32) * 32 * nf * 4 <= LDS, "the generic forward kernel's LDS"
    fwd = mt * 1000 + nf * 100 + mpt
    if f16x3 and 8 <= m <= 40 and m % 2 == 0 and H > 32:
        fwd = 0
    # dX (the last call's rows)
    hl = last_dx_rows(H)
    hs4 = bwx_hs4(hl)
    lo, hi, bit = _jb2_range()
    assert 4 * m * 32 * 4 <= LDS, "the dX kernel's LDS"
    bwx = hs4 * 10 + (2 if lo <= hs4 <= hi and m % 2 == 0 and dbg & bit else 1)
    if f16x3 and 16 < hl <= 256:
        bwx = 0
    # dW
    bmt, hg, gx, ns, per = bww_geometry(row)
    slab = 1 if opts.get("bww_slab", 1) else 0
    aligned = not how.get("off")
    assert not (f16x3 and bmt == 4 and N % 4 == 0 and N >= 32 and aligned), "this row would run the f16x3 dW kernel"
    if dbg & 8:
        assert not slab, "dbg 8 needs bww_slab 0"
        kv = 1
    elif bmt == 4 and N % 4 == 0 and not dbg & 16 and aligned:
        kv = 3
    else:
        kv = 2
    return fwd, bwx, ns * 1000 + bmt * 100 + kv * 10 + slab


# ---- the checks ---------------------------------------------------------------------------------------------------------
def _sweep():
    from test_gpu_cin_f32_instances import SWEEP_F32
    return SWEEP_F32


def test_every_f32_instance_is_in_the_gpu_sweep():
    S = _sweep()
    fwd, bwx, bww = built_fwd(), built_bwx(), built_bww()
    assert len(fwd) >= 11 and len(bwx) >= 9 and len(bww) >= 7, (len(fwd), len(bwx), len(bww))
    got_fwd = {(r[7] // 1000, r[7] // 100 % 10, r[7] % 100) for r in S if r[7]}
    got_bwx = {(r[8] // 10, r[8] % 10) for r in S if r[8]}
    got_bww = {(r[9] // 100 % 10, r[9] // 10 % 10) for r in S if r[9]}
    for what, built, got in (("forward", fwd, got_fwd), ("dX", bwx, got_bwx), ("dW", bww, got_bww)):
        assert got == built, "%s instances missing from SWEEP_F32: %s; in SWEEP_F32 but not built: %s" % (
            what, sorted(built - got), sorted(got - built))
    # both epilogues of both LDS-DMA kernels (v1 has the atomic one only)
    assert {(r[9] // 10 % 10, r[9] % 10) for r in S} == {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1)}
    # the straight-line kernel: both parities of m behind each MPT, at MT 4 and MT 8
    for mpt in mp_fields():
        for mt in (4, 8):
            assert {2 * mpt, 2 * mpt - 1} <= {r[0] for r in S if r[7] // 1000 == mt and r[7] % 100 == mpt}, (mpt, mt)


def test_every_row_claims_what_the_host_rules_pick():
    S = _sweep()
    assert len(set(r[:5] + tuple(tuple(sorted(d.items())) for d in r[5:7]) for r in S)) == len(S), "duplicate SWEEP_F32 row"
    for r in S:
        assert tuple(r[7:]) == expected(r), "row %s claims %s, the host picks %s" % (r[:7], r[7:], expected(r))
        assert r[3] <= 4500


def test_the_exact_family_stays_below_2_to_24():
    """W in [-4, 4], x in [-3, 3], dOut in [-3, 3], bias in [-8, 8], dX prefill in [-5, 5] (_inputs of
    tests/test_gpu_cin_instances.py): bounds of every partial sum a kernel can form, per row"""
    for m, H, Hp, N in (r[:4] for r in _sweep()):
        hc = min(H, 256)
        dz = hc * 4 * 3                                       # |dZ[(i, j)][n]| over the rows of one dX call
        calls = ceil_div(H, 256)
        assert Hp * m * 36 + 8 < 2 ** 24                      # forward: Hp m products |W xp x0| <= 36, + bias
        assert calls * m * dz * 3 + 5 < 2 ** 24               # dxp: sum over j of dZ x0, onto the prefill
        assert calls * Hp * dz * 3 + 5 < 2 ** 24              # dx0
        assert 27 * N < 2 ** 24                               # dW: N products |dOut xp x0| <= 27


def test_the_sweep_holds_the_edges():
    S = _sweep()
    plain = [r for r in S if not r[6].get("math")]
    fwd_generic = [r for r in plain if r[7] % 100 == 0]
    fwd_mp_rows = [r for r in plain if r[7] % 100]
    # forward tiles by H
    Hs = {r[1] for r in S}
    assert {1, 20, 32, 33, 64, 65, 100, 224, 225, 256, 300} <= Hs
    # generic kernel: m = 1, odd m, dead k-steps behind the last quad, refills of the x_prev chunk, ragged N, level 0, linear
    assert any(r[0] == 1 for r in fwd_generic) and any(r[0] % 2 and r[0] > 1 for r in fwd_generic)
    assert any((r[2] * fwd_mp(r[0])) % 4 == 1 for r in fwd_generic), "three dead k-steps"
    assert {1, 32, 33, 65} <= {r[2] for r in fwd_generic}
    assert {1, 31, 33, 127, 129} <= {r[3] for r in fwd_generic} and any(r[3] % 128 == 0 for r in fwd_generic)
    assert any(r[4] for r in fwd_generic) and any(r[4] for r in fwd_mp_rows)
    assert sum(1 for r in S if r[6].get("act") == 0) >= 1
    assert any(r[1] > 256 and r[1] % 256 <= 64 for r in fwd_generic), "a second row block with few live rows"
    # straight-line kernel: Hp tails of the loop unrolled by 4, ragged N
    for mpt in mp_fields():
        rows = [r for r in fwd_mp_rows if r[7] % 100 == mpt]
        assert {1, 5, 32, 37} <= {r[2] for r in rows}, mpt
        assert any(r[3] % 32 for r in rows)
    nf2 = [r for r in S if r[7] // 100 % 10 == 2]
    assert {64, 70, 130} <= {r[3] for r in nf2} and {0} | mp_fields() <= {r[7] % 100 for r in nf2}
    assert any(r[5].get("fwd_nf") == 2 and r[7] // 100 % 10 == 1 for r in S), "fwd_nf 2 at an MT without NF 2"
    dbg2 = [r for r in S if r[5].get("dbg", 0) & 2]
    assert {(26, 4), (26, 8), (22, 4), (22, 8)} <= {(r[0], r[7] // 1000) for r in dbg2} and all(r[7] % 100 == 0 for r in dbg2)
    # dX: HS4 by H, odd H below 64, Hp, m, N, level 0, JB 2
    assert {8, 13, 27, 32, 50, 64, 65, 100, 128, 129, 256} <= Hs
    for hs4 in (2, 4, 8):
        assert any(r[1] % 2 for r in plain if r[8] // 10 == hs4 and r[1] < 64), hs4
    assert {1, 32, 33} <= {r[2] for r in plain} and {1, 26, 50} <= {r[0] for r in plain}
    assert {1, 31, 33, 127, 130} <= {r[3] for r in plain}
    jb2 = [r for r in S if r[8] % 10 == 2]
    assert {4, 8, 16} == {r[8] // 10 for r in jb2} and all(r[0] % 2 == 0 for r in jb2)
    asked = [r for r in S if r[5].get("dbg", 0) & 32 and r[8] % 10 == 1]
    assert any(r[0] % 2 for r in asked) and {2, 32} <= {r[8] // 10 for r in asked}, "dbg 32 without a JB 2 kernel"
    assert any(r[4] for r in jb2)
    # dW: tiles by H, forced tiles, the ways into the dword-DMA kernel, v1, n-splits
    assert {20, 50, 100, 130} <= Hs
    assert {1, 2, 4} <= {r[5].get("bww_mt") for r in S if r[1] == 100}
    dword = [r for r in plain if r[9] // 10 % 10 == 2]
    assert any(r[3] == 301 for r in dword) and {1, 2, 4} <= {r[9] // 100 % 10 for r in dword}
    assert any(r[5].get("dbg", 0) & 16 and r[3] % 4 == 0 and r[9] // 100 % 10 == 4 for r in dword)
    assert any(r[6].get("off") and r[3] % 4 == 0 and r[9] // 100 % 10 == 4 for r in dword)
    assert any(r[6].get("off") and r[9] // 10 % 10 == 2 and r[9] // 100 % 10 == 4 and r[3] % 4 == 0 and r[3] >= 32
               for r in S if r[6].get("math") == 1), "the default arithmetic on unaligned operands"
    geo = {i: bww_geometry(r) for i, r in enumerate(S)}
    assert any(r[1] == 130 and geo[i][1] == 2 for i, r in enumerate(S)), "a second h-group with 2 live rows"
    forced3 = [i for i, r in enumerate(S) if r[5].get("bww_nsplit") == 3 and r[3] == 300]
    assert forced3 and all(geo[i][3:] == (3, 128) for i in forced3)                # 128 / 128 / 44: full chunks in both buffers, 12-column tail
    assert any(r[5].get("bww_nsplit") == 1 for r in S)
    assert any(r[3] == 1000 and geo[i][3:] == (32, 32) and not r[5].get("bww_nsplit") for i, r in enumerate(S))
    assert {20, 28} <= {r[3] for r in S}
    assert sum(1 for r in S if r[9] % 10 == 0 and not r[5].get("dbg", 0) & 8) >= 3
    assert any(geo[i][3] > 1 and r[3] % geo[i][4] % 32 for i, r in enumerate(S) if r[9] // 10 % 10 == 3), "dwordx4-DMA: a masked tail chunk"
    assert {1, 33} <= {r[2] for r in S} and any(r[0] == 1 for r in S)
    assert any((ceil_div(r[0], 2) * ceil_div(r[2], 32)) % 2 for r in S if r[0] > 1), "an odd JP * IB: inactive waves"
