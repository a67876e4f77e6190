"""CPU: the goldens of tests/golden/dnn_bn/ (the reference's xDeepFM with dnn_use_bn=True, tests/golden/make_golden_bn.py)
reload, meet the conditions their generator recorded, and pin the DNN tower alone on the stock path: layers.DNN on the CPU,
loaded with the golden's `dnn.*` state, maps the recorded tower input to the recorded output, gradients and buffers.  The whole
model against the same files runs on the GPU (tests/test_gpu_dnn_bn.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

NAMES = ["bn_xdeepfm_relu", "bn_xdeepfm_sigmoid"]
T = torch.from_numpy


@pytest.mark.parametrize("name", NAMES)
def test_goldens_reload_and_meet_their_generator_conditions(name):
    g = load_golden("dnn_bn/" + name)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dnn_bn", name + ".npz")) < 100 * 1024
    assert str(g["cls"]) == "xDeepFM" and str(g["act"]) == name.rsplit("_", 1)[1] and str(g["task"]) == "binary"
    assert float(g["bar_share_32_vs_64"]) <= 0.5
    zero = [str(k) for k in g["zero_grad_keys"]]
    assert zero == ["dnn.linears.%d.bias" % i for i in range(len(g["dnn"]))]
    lr = float(g["lr"])
    for k in zero:
        assert float(np.abs(g["g:" + k]).max()) <= float(g["zero_grad_bound"])
        assert float(np.abs(g["s3:" + k] - g["s0:" + k]).max()) <= 3 * lr * 1.0001
    assert abs(float(g["running_mean_allowance"]) - 0.58 * lr) < 1e-12
    keys = [k[3:] for k in g if k.startswith("s0:") and k.startswith("s0:dnn.bn.0.")]
    assert keys == ["dnn.bn.0." + n for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    assert int(g["a1:dnn.bn.0.num_batches_tracked"]) == 1 and int(g["s3:dnn.bn.0.num_batches_tracked"]) == 4
    np.testing.assert_allclose(g["losses3"], g["losses3_64"], rtol=1e-5)
    assert np.isfinite(g["dnn_out"]).all() and g["dnn_in"].shape[0] == int(g["B"]) == g["g:dnn_out"].shape[0]


@pytest.mark.parametrize("name", NAMES)
def test_stock_tower_on_the_cpu_reproduces_the_reference_tower(name):
    from xdfm_amd import layers
    g = load_golden("dnn_bn/" + name)
    act, hidden = str(g["act"]), tuple(int(v) for v in g["dnn"])
    net = layers.DNN(g["dnn_in"].shape[1], hidden, activation=act, l2_reg=1e-5, use_bn=True, device="cpu")
    assert sorted("dnn." + k for k in net.state_dict()) == sorted(k[3:] for k in g if k.startswith("s0:dnn.") and "dnn_linear" not in k)
    net.load_state_dict({k[7:]: T(v) for k, v in g.items() if k.startswith("s0:dnn.") and "dnn_linear" not in k}, strict=True)
    net.train()
    x = T(g["dnn_in"]).clone().requires_grad_(True)
    out = net(x)
    out.backward(T(g["g:dnn_out"]))

    def close(got, want, what):
        np.testing.assert_allclose(got.detach().numpy(), want, rtol=2e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-9, err_msg=what)

    close(out, g["dnn_out"], "tower output")
    close(x.grad, g["g:dnn_in"], "gradient at the tower's input")
    zero = set(str(k) for k in g["zero_grad_keys"])
    for k, p in net.named_parameters():
        key = "dnn." + k
        if key in zero:
            assert float(p.grad.abs().max()) <= float(g["zero_grad_bound"]), key
            continue
        grad = p.grad
        if "linears" in k and k.endswith("weight"):              # the golden's gradient is of loss + L2 (basemodel.py:412-428)
            grad = grad + 2 * 1e-5 * p.detach()
        close(grad, g["g:" + key], "grad " + key)
    for k, v in net.state_dict().items():
        if "a1:dnn." + k in g:
            np.testing.assert_allclose(v.numpy(), g["a1:dnn." + k], rtol=1e-5, atol=1e-6, err_msg="after the first forward: " + k)
