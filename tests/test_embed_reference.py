"""CPU checks of what the K1 / K2 GPU tests (tests/test_gpu_embed_abi.py) lean on: tests/embed_ref.py's bit-exact model of
the scatter against the float64 sum, against a literal simulation of the kernel's windows and chains, under permutation and
against fp32 adds in example order; the run layout every scatter case claims (from its ids alone: a change of a case
that would stop it reaching its path fails HERE); and, for the gather cases, the facts the host code derives from
the shape."""
import numpy as np
import pytest

import embed_ref as ER

SCATTER = list(ER.SCATTER_CASES)
_CACHE = {}


def _case(name):
    if name not in _CACHE:
        case = ER.scatter_inputs(name)
        _CACHE[name] = (case, ER.scatter_model(case))
    return _CACHE[name]


def _same_bits(a, b, what):
    assert a.shape == b.shape
    bad = np.flatnonzero(ER.bits(a) != ER.bits(b))
    assert bad.size == 0, "%s: %d elements differ, first at %d: %r / %r" % (what, bad.size, bad[0], a.flat[bad[0]], b.flat[bad[0]])


def _within(got, case, what):
    exact, tol = ER.scatter_bound(case)
    err = np.abs(got.astype(np.float64) - exact)
    bad = err > tol
    print("%s: worst error / bound %.3f" % (what, float((err / np.maximum(tol, 1e-300)).max())))
    assert not bad.any(), "%s: %d elements off, worst %g" % (what, int(bad.sum()), float(err[bad].max()))


# ----------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", SCATTER)
def test_model_is_within_the_bound_of_the_float64_sum(name):
    case, (flat, marks) = _case(name)
    _within(flat, case, name)
    t = ER.touched(case)
    _same_bits(flat[~t], case["prefill"][~t], "%s: untouched elements" % name)
    want = np.zeros_like(marks)
    want[np.flatnonzero(t) >> 2] = 1
    np.testing.assert_array_equal(marks, want)


@pytest.mark.parametrize("name", SCATTER)
def test_windows_and_chains_give_the_bits_of_the_model(name):
    """The kernel's scheme (finished runs per window, owner + chain of open pieces, one grid per run) is a function of
    the multiset of rows: whatever order the grouped list has, the model's bits."""
    case, (flat, _) = _case(name)
    _same_bits(ER.scatter_model(case, windows=True)[0], flat, "%s: runs in ascending id order" % name)
    _same_bits(ER.scatter_model(case, windows=True, rng=np.random.default_rng(5))[0], flat, "%s: runs in a random order" % name)


@pytest.mark.parametrize("name", [n for n in SCATTER if ER.SCATTER_CASES[n]["B"] <= ER.SC_ROWS])
def test_model_is_invariant_under_a_permutation_of_the_examples(name):
    case, (flat, marks) = _case(name)
    p = np.random.default_rng(11).permutation(case["B"])
    flat_p, marks_p = ER.scatter_model(ER.permuted(case, p))
    _same_bits(flat_p, flat, name)
    np.testing.assert_array_equal(marks_p, marks)


@pytest.mark.parametrize("name", SCATTER)
def test_model_against_fp32_adds_in_example_order(name):
    case, (flat, _) = _case(name)
    exact, tol = ER.scatter_bound(case)
    diff = np.abs(flat.astype(np.float64) - ER.scatter_in_example_order(case).astype(np.float64))
    assert not (diff > tol).any(), "%s: %d elements, worst %g" % (name, int((diff > tol).sum()), float(diff.max()))


def test_scale_exponent_and_grid():
    a = np.array([0.0, 1e-45, 2.0 ** -126, 1.0, 1.5, 2.0, 3e38], dtype=np.float32)
    assert ER.scale_exp(a).tolist() == [163, 163, 163, 37, 37, 36, 37 - 127]
    for v in a[3:]:
        assert 2.0 ** 37 <= float(v) * 2.0 ** int(ER.scale_exp(v).reshape(-1)[0]) < 2.0 ** 38
    # ties go to even; a run's sum is exact however the addends cancel
    assert ER._fix(np.array([0.5, 1.5, 2.5, -0.5], dtype=np.float32), 0).tolist() == [0, 2, 2, 0]
    ids = np.zeros(3, dtype=np.int64)
    vals = np.array([[1.0], [2.0 ** -30], [-1.0]], dtype=np.float32)
    keys, r = ER._reduce_multiset(ids, vals)
    assert keys.tolist() == [0] and r[0, 0] == np.float32(2.0 ** -30)            # fp32 adds in this order give 0


# ------------------------------------------------------------------------------------------- what the cases contain
def _layouts(case, j, b0=0):
    return ER.layouts(ER.run_lengths(case, j, b0))


ALL_MOD8 = set(range(8))


def _s1(c):
    case = _case("S1-c%d" % c)[0]
    V = case["vocab"][0]
    assert case["B"] % 8 == 0 and case["B"] <= 600 and ER.run_lengths(case, 0) == [c] * V
    (f,) = _layouts(case, 0)
    return f, V


def test_s1_run_lengths_reach_every_window_situation():
    f, V = _s1(1)
    assert f["spans"] == {} and f["closed_on_edge"] == V // 8
    f, V = _s1(7)
    assert f["starts_mod8"] == ALL_MOD8 and set(f["spans"]) == {2} and f["closed_on_edge"] >= 1 and f["both"] == 0
    f, V = _s1(8)
    assert f["spans"] == {} and f["closed_on_edge"] == V and f["starts_mod8"] == {0}      # every run ends on a window edge
    f, V = _s1(9)
    assert f["starts_mod8"] == ALL_MOD8 and set(f["spans"]) == {2} and f["open_ends_on_edge"] >= 1 and f["both"] == 0
    f, V = _s1(15)
    assert f["starts_mod8"] == ALL_MOD8 and set(f["spans"]) == {2, 3} and f["both"] >= 1
    f, V = _s1(16)
    assert f["spans"] == {2: V} and f["open_ends_on_edge"] == V and f["both"] == 0          # exactly two windows: owner + left piece
    f, V = _s1(17)
    assert f["starts_mod8"] == ALL_MOD8 and set(f["spans"]) == {3} and f["both_then_one"] >= 1 and f["both"] >= 1
    f, V = _s1(24)
    assert f["spans"] == {3: V} and f["both"] == V and f["open_ends_on_edge"] == V          # exactly three windows
    f, V = _s1(25)
    assert f["starts_mod8"] == ALL_MOD8 and set(f["spans"]) == {4} and f["both_then_one"] >= 1 and f["both"] >= 2 * V - 2
    for c in ER.S1_RUNS:
        assert ER.SCATTER_CASES["S1-c%d" % c]["D"] == 8


def test_s2_chains_of_a_whole_chunk():
    case = _case("S2")[0]
    assert case["B"] == ER.SC_ROWS and case["D"] == 4
    assert [ER.run_lengths(case, j) for j in range(3)] == [[4096], [1, 4095], [8, 8, 4080]]
    (f,) = _layouts(case, 0)
    assert f["spans"] == {512: 1} and f["both"] == 510 and f["longest_chain"] == 512
    for f in _layouts(case, 1):                                                  # either order of the two runs
        assert f["longest_chain"] == 512 and f["both"] == 510
    orders = _layouts(case, 2)
    assert len(orders) == 3
    for f in orders:
        assert f["longest_chain"] == 510 and f["both"] == 508 and f["closed_next_to_open"] >= 1 and f["closed_on_edge"] == 2


def test_s3_short_chunks_and_s4_second_chunks():
    for B in (1, 5, 7, 8, 9):
        case = _case("S3-B%d" % B)[0]
        lens = ER.run_lengths(case, 0)
        assert sum(lens) == B and case["vocab"] == [3] and case["D"] == 4
        for f in ER.layouts(lens):                                               # B < 8: one window, not full (nb < 8)
            assert f["windows"] == (2 if B == 9 else 1) and f["last_window"] == (1 if B == 9 else B)
    for B, rest in ((4097, 1), (4104, 8)):
        case = _case("S4-B%d" % B)[0]
        assert case["B"] - ER.SC_ROWS == rest and case["vocab"] == [5, 700] and case["D"] == 8
        for j in range(2):
            assert sum(ER.run_lengths(case, j, ER.SC_ROWS)) == rest
        first = set(ER.ids_of(case["X"][:ER.SC_ROWS, case["cols"][0]], 5)[0].tolist())
        second = set(ER.ids_of(case["X"][ER.SC_ROWS:, case["cols"][0]], 5)[0].tolist())
        assert second <= first                                                   # rows that receive a sum per chunk
        assert max(ER.run_lengths(case, 0)) > 512 and len(ER.run_lengths(case, 1)) > 100


def test_layout_and_source_claims_of_the_other_scatter_cases():
    s5 = _case("S5")[0]
    assert s5["has_prefill"] and s5["nd"] == 2 and s5["D"] == 16 and s5["B"] == 300 and s5["m"] == 3
    t = ER.touched(s5)
    mags = np.abs(s5["prefill"][t])
    assert mags.min() > 0 and mags.min() < 1e-2 and mags.max() > 1.0 and t[s5["dw_off"]:s5["dw_off"] + 2].all()
    s6 = _case("S6")[0]
    assert [o % 4 for o in s6["tab_off"]] == [1, 2, 3] and s6["D"] % 4 == 0 and s6["misalign"] is None and s6["marks"]
    for name, what in (("S7-emb", "emb"), ("S7-flat", "flat")):
        s7 = _case(name)[0]
        assert s7["misalign"] == what and s7["D"] % 4 == 0 and not s7["marks"] and s7["d_emb"] is not None
    for D, slices, live in ((6, 2, 2), (20, 5, 4)):
        s8 = _case("S8-D%d" % D)[0]
        assert s8["B"] == 260 and s8["m"] == 4 and -(-D // 4) == slices and D - 4 * (slices - 1) == live
    s9 = _case("S9")[0]
    assert s9["ld_dnn"] == s9["m"] * s9["D"] + s9["nd"] + 5 and s9["ld_lin"] == 3 and s9["ldx"] == s9["m"] + s9["nd"] + 3
    assert s9["cols"].tolist() != sorted(s9["cols"].tolist()) and not s9["dense_pitches"] and s9["B"] == 200
    for name, (e, d, l, tab, lin) in {"S11-emb": (1, 0, 0, 1, 0), "S11-dnn": (0, 1, 0, 1, 0), "S11-dense-only": (0, 0, 1, 0, 0),
                                      "S11-lin-only": (0, 0, 1, 0, 1)}.items():
        c = _case(name)[0]
        assert ((c["d_emb"] is not None, c["d_dnn"] is not None, c["d_lin"] is not None, c["tab_off"] is not None,
                 c["lin_off"] is not None) == (e, d, l, tab, lin)) and c["nd"] == 2 and c["B"] == 128
    # the cases with drawn ids: finished runs and runs that cross windows both occur
    for name in ("S5", "S6", "S7-emb", "S7-flat", "S8-D6", "S8-D20", "S9", "S11-emb"):
        c = _case(name)[0]
        lens = [n for j in range(c["m"]) for n in ER.run_lengths(c, j)]
        assert max(lens) > 16 and min(lens) < 8, name


def test_s10_touches_exactly_the_rows_the_gather_reads():
    case = _case("S10")[0]
    assert case["B"] == 64 and case["m"] == 2 and case["D"] == 4
    tables = [np.arange(V * 4, dtype=np.float32).reshape(V, 4) + 100 * j for j, V in enumerate(case["vocab"])]   # a row names itself
    emb, _, _, _, flag = ER.gather_reference(case["X"], tables, None, case["cols"], case["vocab"], None, None, 4)
    assert flag == 1
    t = ER.touched(case)
    for j, V in enumerate(case["vocab"]):
        col = case["X"][:, case["cols"][j]]
        for v in ER.special_id_values(V, "all"):
            assert (col == v).any()
        read = np.unique(((emb[:, j, 0] - 100 * j) / 4).astype(np.int64))
        rows = t[case["tab_off"][j]:case["tab_off"][j] + V * 4].reshape(V, 4)
        assert (rows.all(1) | ~rows.any(1)).all() and np.flatnonzero(rows[:, 0]).tolist() == read.tolist()
        assert 0 in read and V - 1 in read and 2 in read


# ------------------------------------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("name", list(ER.GATHER_CASES))
def test_gather_case_reaches_what_it_claims(name):
    c = ER.GATHER_CASES[name]
    facts = ER.gather_facts(c)
    for key, want in c["claims"].items():
        assert facts[key] == want, "%s: %s is %r" % (name, key, facts[key])
    inp = ER.gather_inputs(name)
    assert all(1 <= V <= 11 for V in inp["vocab"])
    assert sorted(np.r_[inp["cols"], inp["dense_cols"]].tolist()) == sorted(set(np.r_[inp["cols"], inp["dense_cols"]].tolist()))
    emb, dnn, lin64, lin_abs, flag = ER.gather_expected(inp)
    assert emb.shape == (c["B"], c["m"], c["D"]) and dnn.shape == (c["B"], c["m"] * c["D"] + c["nd"])
    assert flag == (1 if name == "G10" else 0)
    assert (lin_abs >= np.abs(lin64)).all()


def test_gather_case_shapes_are_the_ones_listed():
    shapes = {n: (c["B"], c["m"], c["D"], c["nd"]) for n, c in ER.GATHER_CASES.items()}
    assert shapes == {"G1": (37, 33, 8, 2), "G2": (19, 40, 12, 0), "G3": (21, 32, 4, 1), "G4": (35, 4, 8, 40), "G5": (18, 2, 4, 300),
                      "G6": (3, 33, 252, 1), "G7": (17, 3, 6, 2), "G8": (9, 1, 1, 0), "G9": (23, 5, 10, 3), "G10": (16, 6, 16, 2),
                      "G10b": (16, 6, 16, 2)}
    g5, g9 = ER.gather_inputs("G5"), ER.gather_inputs("G9")
    assert g5["ldx"] == 2 + 300 + 3 and g9["ld"] == dict(dense_off=50 + 20, ld_dnn=70 + 3 + 4)
    assert ER.gather_inputs("G2")["lins"] is None


def test_gather_reference_truncates_and_clamps():
    X = np.array([[-3.0], [-0.5], [0.9], [4.75], [5.0], [12.0], [2.7]], dtype=np.float32)
    tab = [np.arange(10, dtype=np.float32).reshape(5, 2)]
    emb, dnn, lin64, lin_abs, flag = ER.gather_reference(X, tab, [np.array([1, 2, 4, 8, 16], dtype=np.float32)], [0], [5], None, None, 2)
    assert (emb[:, 0, 0] / 2).tolist() == [0, 0, 0, 4, 4, 4, 2] and flag == 1 and lin64.tolist() == [1, 1, 1, 16, 16, 16, 4]
    assert np.array_equal(dnn, emb.reshape(7, 2))
    assert ER.gather_reference(X[[1, 2, 3, 6]], tab, None, [0], [5], None, None, 2)[4] == 0
    for which, n in (("all", 7), ("benign", 4)):
        inp = ER.gather_inputs("G10" if which == "all" else "G10b")
        for j, V in enumerate(inp["vocab"]):
            vals = ER.special_id_values(V, which)
            assert len(vals) == n and V >= 3 and all((inp["X"][:, inp["cols"][j]] == v).any() for v in vals)
