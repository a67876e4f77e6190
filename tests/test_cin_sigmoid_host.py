"""CPU checks of the sigmoid CIN activation: the host rules (activation code, constructors, what is still refused) and the
oracle against the three goldens the reference produced (tests/golden/make_golden_cin_sigmoid.py), at the bars
tests/test_oracle_golden.py applies to the relu goldens of the same kind."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import xdeepfm_oracle as orc

T = torch.from_numpy
MODEL_GOLDEN = "sigmoid/model_sigmoid_small"
CIN_GOLDENS = ["cin_sigmoid_split", "cin_sigmoid_nosplit"]


def _columns(g):
    from deepctr.inputs import DenseFeat, SparseFeat
    vocab, nd, D = [int(v) for v in g["vocab"]], int(g["n_dense"]), int(g["emb_dim"])
    return [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate(vocab)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(nd)]


def _spec(g):
    vocab, nd = [int(v) for v in g["vocab"]], int(g["n_dense"])
    return orc.Spec(["C%d" % (i + 1) for i in range(len(vocab))], vocab, ["I%d" % (i + 1) for i in range(nd)], int(g["emb_dim"]),
                    tuple(int(v) for v in g["cin"]), True, str(g["cin_activation"]), tuple(int(v) for v in g["dnn"]), "sum",
                    l2_reg_dnn=1e-5)


def test_activation_code():
    from xdfm_amd import ops
    assert ops.activation_code("sigmoid") == 2 and ops.activation_code("Sigmoid") == 2
    assert ops.activation_code("linear") == 0 and ops.activation_code("relu") == 1
    assert ops.ACT_CODES == {"linear": 0, "relu": 1, "sigmoid": 2}


def test_only_sigmoid_gives_up_the_lean_levels():
    from xdfm_amd import ops
    assert [ops.cin_lean_allowed(ops.activation_code(a)) for a in ("linear", "relu", "sigmoid")] == [True, True, False]


def test_model_constructs_with_the_reference_state():
    """same keys and, from seed 1024, the reference's own initial weights: the activation has no parameters"""
    from deepctr.models import xDeepFM
    g = load_golden(MODEL_GOLDEN)
    assert str(g["cin_activation"]) == "sigmoid" and str(g["cls"]) == "xDeepFM"
    cols = _columns(g)
    model = xDeepFM(cols, cols, dnn_hidden_units=tuple(int(v) for v in g["dnn"]), cin_layer_size=tuple(int(v) for v in g["cin"]),
                    l2_reg_dnn=1e-5, cin_activation="sigmoid", device="cpu")
    assert model.cin.activation == "sigmoid"
    sd = model.state_dict()
    assert sorted(sd.keys()) == sorted(k[5:] for k in g if k.startswith("init:")) == sorted(k[3:] for k in g if k.startswith("s0:"))
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), g["init:" + k], err_msg=k)
    relu = load_golden("model_sum_small")
    assert sorted(k for k in relu if k.startswith("init:")) == sorted(k for k in g if k.startswith("init:"))


@pytest.mark.parametrize("cls", ["xDeepFMAttention", "xDeepFMAttentionV2", "xDeepFMPro", "xDeepFMProLight"])
def test_every_model_class_takes_sigmoid(cls):
    from deepctr import models
    from deepctr import xdeepfm_pro
    g = load_golden(MODEL_GOLDEN)
    cols = _columns(g)
    ctor = getattr(models, cls, None) or getattr(xdeepfm_pro, cls)
    model = ctor(cols, cols, cin_layer_size=(8, 6), dnn_hidden_units=(8,), cin_activation="sigmoid", device="cpu")
    assert model.cin.activation == "sigmoid"


@pytest.mark.parametrize("bad", ["prelu", "dice", "PReLU", torch.nn.Sigmoid, torch.nn.Sigmoid()])
def test_other_activations_are_still_refused(bad):
    from deepctr.layers import CIN
    from deepctr.models import xDeepFM
    from xdfm_amd import ops
    g = load_golden(MODEL_GOLDEN)
    cols = _columns(g)
    with pytest.raises(NotImplementedError, match="'relu', 'linear' and 'sigmoid'"):
        ops.activation_code(bad)
    with pytest.raises(NotImplementedError):
        xDeepFM(cols, cols, cin_activation=bad, device="cpu")
    with pytest.raises(NotImplementedError):
        CIN(4, (6, 4), bad, True, 0.0, 1024, device="cpu")


@pytest.mark.parametrize("name", CIN_GOLDENS)
def test_oracle_cin_vs_sigmoid_golden(name):
    """the bars of test_oracle_golden.py::test_cin_forward_backward"""
    g = load_golden(name)
    assert str(g["activation"]) == "sigmoid" and bool(g["split_half"]) == (name == "cin_sigmoid_split")
    L = len(g["layer_size"])
    x = T(g["x"]).requires_grad_(True)
    W = [T(g["w%d" % i]).requires_grad_(True) for i in range(L)]
    Bs = [T(g["b%d" % i]).requires_grad_(True) for i in range(L)]
    out = orc.cin_forward(x, W, Bs, bool(g["split_half"]), "sigmoid")
    np.testing.assert_allclose(out.detach().numpy(), g["out"], rtol=1e-6, atol=1e-6)
    (out * T(g["gout"])).sum().backward()
    np.testing.assert_allclose(x.grad.numpy(), g["dx"], rtol=1e-4, atol=1e-5)
    for i in range(L):
        np.testing.assert_allclose(W[i].grad.numpy(), g["dw%d" % i], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(Bs[i].grad.numpy(), g["db%d" % i], rtol=1e-4, atol=1e-5)
    # the fixture is a sigmoid's: a relu or linear oracle is far outside the bar
    other = orc.cin_forward(x.detach(), [w.detach() for w in W], [b.detach() for b in Bs], bool(g["split_half"]), "relu")
    assert float((other - T(g["out"])).abs().max()) > 1e-2


def test_oracle_model_vs_sigmoid_golden():
    """the bars of test_oracle_golden.py::test_model_forward_grads_adam"""
    g = load_golden(MODEL_GOLDEN)
    spec = _spec(g)
    B = int(g["B"])
    X, y = T(g["X"]), T(g["y"])
    st = {k[3:]: T(v.copy()).requires_grad_(True) for k, v in g.items() if k.startswith("s0:")}
    tot, dl, yp = orc.total_loss(X[:B], y[:B], st, spec)
    np.testing.assert_allclose(yp.detach().numpy(), g["y_pred"].squeeze(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(dl.item(), float(g["loss"]), rtol=1e-6)
    np.testing.assert_allclose(orc.regularization_loss(st, spec).item(), float(g["reg"]), rtol=1e-5)
    tot.backward()
    for k, v in st.items():
        np.testing.assert_allclose(v.grad.numpy(), g["g:" + k], rtol=2e-4, atol=1e-5 * float(np.abs(g["g:" + k]).max()) + 1e-9, err_msg=k)
    st = {k[3:]: T(v.copy()).requires_grad_(True) for k, v in g.items() if k.startswith("s0:")}
    batches = [(X[s * B:(s + 1) * B], y[s * B:(s + 1) * B]) for s in range(3)]
    log = orc.train_steps(batches, st, spec, lr=1e-3)
    np.testing.assert_allclose(np.array(log), g["losses3"], rtol=1e-5)
    for k, v in st.items():
        np.testing.assert_allclose(v.detach().numpy(), g["s3:" + k], rtol=1e-4, atol=1e-6, err_msg=k)
    with torch.no_grad():
        pred = orc.model_forward(X, {k: v.detach() for k, v in st.items()}, spec)
    np.testing.assert_allclose(pred.numpy(), g["pred_after"], rtol=1e-5, atol=1e-7)


def test_train_script_flag():
    import importlib
    amd = importlib.import_module("xdftrain_amd")
    assert amd.parse_args(["--synthetic", "8"], None, None).cin_activation == "relu"
    assert amd.parse_args(["--synthetic", "8", "--cin_activation", "sigmoid"], None, None).cin_activation == "sigmoid"
    with pytest.raises(SystemExit):
        amd.parse_args(["--synthetic", "8", "--cin_activation", "prelu"], None, None)
