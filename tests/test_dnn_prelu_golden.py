"""CPU: the goldens of tests/golden/dnn_prelu/ (the reference's xDeepFM with dnn_activation='prelu', without and with
dnn_use_bn; tests/golden/make_golden_prelu.py) reload, meet the conditions their generator recorded, and pin the DNN tower alone:
layers.DNN on the CPU, loaded with the golden's `dnn.*` state, maps the recorded tower input to the recorded output and
gradients, the slopes' included.  The bars are those of tests/test_dnn_bn_golden.py.  The whole model against the same files
runs on the GPU (tests/test_gpu_dnn_prelu.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

NAMES = ["prelu_xdeepfm", "prelu_xdeepfm_bn"]
T = torch.from_numpy


def _tower_state(g, prefix="s0:"):
    return {k[len(prefix) + 4:]: T(v) for k, v in g.items() if k.startswith(prefix + "dnn.") and "dnn_linear" not in k}


@pytest.mark.parametrize("name", NAMES)
def test_goldens_reload_and_meet_their_generator_conditions(name):
    g = load_golden("dnn_prelu/" + name)
    use_bn = name.endswith("_bn")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dnn_prelu", name + ".npz")) < 100 * 1024
    assert str(g["cls"]) == "xDeepFM" and str(g["act"]) == "prelu" and str(g["task"]) == "binary" and bool(g["use_bn"]) == use_bn
    assert float(g["bar_share_32_vs_64"]) <= 0.5
    n = len(g["dnn"])
    slopes = ["dnn.activation_layers.%d.weight" % i for i in range(n)]
    for i, k in enumerate(slopes):
        assert g["init:" + k].shape == (1,) and float(g["init:" + k][0]) == 0.25
        assert float(g["s0:" + k][0]) == np.float32(g["slopes"][i % len(g["slopes"])])
        assert g["g:" + k].shape == (1,) and float(np.abs(g["g:" + k][0])) > 0
        assert float(np.abs(g["s3:" + k] - g["s0:" + k])[0]) > 0            # Adam moved them
    assert float(g["slopes"].min()) < 0 < float(g["slopes"].max())
    zero = [str(k) for k in g["zero_grad_keys"]]
    assert zero == (["dnn.linears.%d.bias" % i for i in range(n)] if use_bn else [])
    lr = float(g["lr"])
    for k in zero:
        assert float(np.abs(g["g:" + k]).max()) <= float(g["zero_grad_bound"])
        assert float(np.abs(g["s3:" + k] - g["s0:" + k]).max()) <= 3 * lr * 1.0001
    if use_bn:
        assert int(g["a1:dnn.bn.0.num_batches_tracked"]) == 1 and int(g["s3:dnn.bn.0.num_batches_tracked"]) == 4
    np.testing.assert_allclose(g["losses3"], g["losses3_64"], rtol=1e-5)
    assert np.isfinite(g["dnn_out"]).all() and g["dnn_in"].shape[0] == int(g["B"]) == g["g:dnn_out"].shape[0]


@pytest.mark.parametrize("name", NAMES)
def test_tower_on_the_cpu_reproduces_the_reference_tower(name):
    from xdfm_amd import layers
    g = load_golden("dnn_prelu/" + name)
    use_bn, hidden = bool(g["use_bn"]), tuple(int(v) for v in g["dnn"])
    net = layers.DNN(g["dnn_in"].shape[1], hidden, activation="prelu", l2_reg=1e-5, use_bn=use_bn, device="cpu")
    net.load_state_dict(_tower_state(g), strict=True)
    net.train()
    x = T(g["dnn_in"]).clone().requires_grad_(True)
    out = net(x)
    out.backward(T(g["g:dnn_out"]))

    def close(got, want, what):
        np.testing.assert_allclose(got.detach().numpy(), want, rtol=2e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-9, err_msg=what)

    close(out, g["dnn_out"], "tower output")
    close(x.grad, g["g:dnn_in"], "gradient at the tower's input")
    zero = set(str(k) for k in g["zero_grad_keys"])
    l2 = set(str(k) for k in g["l2_reg_dnn_keys"])
    seen = 0
    for k, p in net.named_parameters():
        key = "dnn." + k
        if key in zero:
            assert float(p.grad.abs().max()) <= float(g["zero_grad_bound"]), key
            continue
        grad = p.grad
        if k in l2:                                   # the golden's gradient is of loss + L2 (basemodel.py:412-428): the slopes' too
            grad = grad + 2 * 1e-5 * p.detach()
            seen += "activation_layers" in k
        close(grad, g["g:" + key], "grad " + key)
    assert seen == len(hidden)
    for k, v in net.state_dict().items():
        if "a1:dnn." + k in g:
            np.testing.assert_allclose(v.numpy(), g["a1:dnn." + k], rtol=1e-5, atol=1e-6, err_msg="after the first forward: " + k)
