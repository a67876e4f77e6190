"""CPU: VarLenSparseFeat columns on the host side -- construction against the reference's goldens, the limits, and the
float64 restatement (tests/varlen_ref.py) against the reference's own SequencePoolingLayer results."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import varlen_ref as vr

MODELS = ("varlen_model_xdeepfm", "varlen_model_attn")


@pytest.mark.parametrize("name", MODELS)
def test_model_with_varlen_columns_constructs_like_the_reference(name):
    g = load_golden(name)
    assert float(g["bar_share_32_vs_64"]) < 0.5            # the golden itself: fp32 / fp64 reference runs agree well inside the bars
    model = vr.golden_model(g, "cpu")
    state = model.state_dict()
    assert list(state.keys()) == [str(k) for k in g["state_keys"]]
    for k, v in state.items():
        want = g["init:" + k]
        assert tuple(v.shape) == want.shape, k
        np.testing.assert_array_equal(v.numpy(), want, err_msg="initial " + k)      # same seed, same draws, same order
    names = [str(n) for n in g["feature_names"]]
    assert list(model.feature_index.keys()) == names
    for n, lo, hi in zip(names, g["feature_lo"], g["feature_hi"]):
        assert tuple(model.feature_index[n]) == (int(lo), int(hi)), n
    assert model.compute_input_dim(model.dnn_feature_columns) == int(g["dnn_input_dim"])
    assert len(model.embedding_dict) == 6 and model.cin.field_nums[0] == 6        # one CIN field per sparse and per pooled column


def _cols(**kw):
    from deepctr.inputs import SparseFeat, VarLenSparseFeat
    a = dict(maxlen=3, combiner="mean", D=4, emb_name=None)
    a.update(kw)
    return [SparseFeat("C1", 5, 4), VarLenSparseFeat(SparseFeat("tags", 6, a["D"], embedding_name=a["emb_name"]), a["maxlen"], a["combiner"])]


@pytest.mark.parametrize("kw", [dict(maxlen=0), dict(maxlen=256), dict(combiner="min"), dict(D=8), dict(emb_name="C1")])
def test_limits_raise_value_error(kw):
    from deepctr.models import xDeepFM, xDeepFMAttention
    cols = _cols(**kw)
    for cls in (xDeepFM, xDeepFMAttention):
        with pytest.raises(ValueError):
            cls(cols, cols, dnn_hidden_units=(4,), cin_layer_size=(4,), device="cpu")


def test_limits_accept_the_edges():
    from deepctr.models import xDeepFM
    for kw in (dict(maxlen=1), dict(maxlen=255), dict(combiner="sum"), dict(combiner="max")):
        cols = _cols(**kw)
        xDeepFM(cols, cols, dnn_hidden_units=(4,), cin_layer_size=(4,), device="cpu")


def test_pro_models_refuse_varlen_columns():
    from deepctr.xdeepfm_pro import xDeepFMPro, xDeepFMProLight
    cols = _cols()
    for cls in (xDeepFMPro, xDeepFMProLight):
        with pytest.raises(NotImplementedError):
            cls(cols, cols, device="cpu")


def test_plan_refuses_bad_fields_without_a_device():
    from xdfm_amd import ops
    with pytest.raises(ValueError):
        ops.VarLenPlan([1], [300], [None], ["sum"], [5], 4)
    with pytest.raises(ValueError):
        ops.VarLenPlan([1], [3], [None], ["median"], [5], 4)
    plan = ops.VarLenPlan([1, 4], [3, 20], [None, 24], ["sum", "max"], [5, 6], 4)
    assert plan.Tmax == 20 and plan.min_cols == 25 and plan.len_cols == [-1, 24]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.VarLenPool.apply(torch.zeros(2, 25), None, None, torch.zeros(2, 1), plan, 0, torch.zeros(5, 1), torch.zeros(6, 1))


def test_library_checks_descriptors_before_launching():
    import ctypes
    from xdfm_amd import _lib
    lib = _lib.load()
    host = (_lib.VarLenField * 1)()
    host[0].table, host[0].col, host[0].maxlen, host[0].len_col, host[0].combiner, host[0].vocab = 64, 2, 4, -1, 0, 5
    one = ctypes.c_void_p(64)                           # never dereferenced: every call below is refused on the host
    args = lambda ldx: (one, ldx, 3, one, ctypes.cast(host, ctypes.c_void_p), 1, 4, 0, one, None, 0, 0, None, None, None, None)
    assert lib.xdfm_varlen_pool_fwd(*args(5)) == 1 and b"outside X" in lib.xdfm_last_error()
    host[0].maxlen = 256
    assert lib.xdfm_varlen_pool_fwd(*args(400)) == 1 and b"maxlen" in lib.xdfm_last_error()
    host[0].maxlen, host[0].combiner = 3, 7
    assert lib.xdfm_varlen_pool_fwd(*args(8)) == 1 and b"combiner" in lib.xdfm_last_error()
    assert lib.xdfm_varlen_pool_bwd_ws_elems(300, 3, 16, 20) == 300 * 20 * 3 * 16 + 2 * 300 * 20 * 3
    assert lib.xdfm_varlen_pool_bwd_ws_elems(0, 3, 16, 20) == 0


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_float64_helper_reproduces_the_reference_pooling(mode):
    """Pins tests/varlen_ref.py to the reference.  Bar 1e-6 relative (to the element, plus 1e-6 of the array's largest
    magnitude where sums cancel): the goldens are fp32 results of at most 5 additions and one division, i.e. at most
    7 * 2^-24 = 4e-7 relative to the summed magnitudes; max is exact."""
    g = load_golden("varlen_pool_" + mode)
    table, up = g["table"], g["upstream"]
    for kind in ("zero", "len"):
        if "pooled_" + kind not in g:
            assert (mode, kind) == ("max", "len")      # the reference itself cannot run this combination
            continue
        ids = g["ids_" + kind]
        lengths = g["lengths"] if kind == "len" else None
        pooled, _, _ = vr.pool(ids, lengths, table, mode)
        want = g["pooled_" + kind]
        if mode == "max":
            np.testing.assert_array_equal(pooled, want)
        else:
            np.testing.assert_allclose(pooled, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
        dt, _, n = vr.pool_grad(ids, lengths, table, mode, up)
        wantg = g["dtable_" + kind]
        np.testing.assert_allclose(dt, wantg, rtol=1e-6, atol=1e-6 * np.abs(wantg).max())
        assert np.all(wantg[n == 0] == 0)


def test_float64_helper_reproduces_the_reference_on_empty_max_sequences():
    """The case the other pooling goldens leave out: max under the zero mask with all-masked sequences (1, 4 and 8 of
    varlen_pool_max_empty.npz).  The reference pools them to w[0] - 1e9 and autograd hands their gradient to position 0,
    i.e. to table row 0 -- through the [V, D] table and through the [V, 1] table of the linear logit alike.  Pooled values
    compare exactly, the table gradient at the bar of the test above."""
    g = load_golden("varlen_pool_max_empty")
    ids = g["ids"]
    assert list(np.flatnonzero((ids == 0).all(1))) == [1, 4, 8] and list(ids[2]) == [2, 0, 2, 0, 0] and np.all(ids[0] != 0)
    for pre in ("", "lin_"):
        table, up, want, wantg = g[pre + "table"], g[pre + "upstream"], g[pre + "pooled"], g[pre + "dtable"]
        assert np.all(wantg[0] != 0)                       # the golden does exercise the case
        pooled, _, pos = vr.pool(ids, None, table, "max")
        np.testing.assert_array_equal(pooled, want)
        np.testing.assert_array_equal(pooled[[1, 4, 8]], np.broadcast_to(table[0] - np.float32(1e9), (3, table.shape[1])))
        assert np.all(pos[[1, 4, 8]] == 0)
        dt, _, n = vr.pool_grad(ids, None, table, "max", up)
        np.testing.assert_allclose(dt, wantg, rtol=1e-6, atol=1e-6 * np.abs(wantg).max())
        assert n[0] >= 3 and np.all(wantg[n == 0] == 0)
