"""CPU: the C ABI of the PReLU kernels (the _prelu entry points of csrc/dnn.hip, csrc/prelu.hip) -- symbols, the workspace
queries and argument validation before any device work -- and everything of dnn_activation='prelu' that needs no GPU:
layers.DNN on the CPU against the torch composition, the reference's state_dict keys, the slopes' L2 group, the activations
that stay refused, and the trainer's flag."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "xdfm.h")
NAMES = ["xdfm_dense_prelu_fwd", "xdfm_dense_prelu_bwd_x", "xdfm_dense_prelu_bwd_w", "xdfm_dense_prelu_bwd_w_ws_elems",
         "xdfm_prelu_fwd", "xdfm_prelu_bwd", "xdfm_prelu_ws_elems"]
P = ctypes.c_void_p


def _lib():
    from xdfm_amd import _lib
    return _lib, _lib.load()


def test_symbols_in_header_binding_and_library():
    mod, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), "include/xdfm.h does not declare %s" % n
        assert n in mod.SIGNATURES, "xdfm_amd/_lib.py does not bind %s" % n
        assert hasattr(lib, n), "libxdfm_hip.so lacks %s" % n
    assert lib.xdfm_abi_version() == mod.ABI_VERSION
    assert "#define XDFM_ABI_VERSION %d\n" % mod.ABI_VERSION in open(HEADER).read()


def test_workspace_queries():
    _, lib = _lib()
    dw, plain, ew = lib.xdfm_dense_prelu_bwd_w_ws_elems, lib.xdfm_dense_bwd_w_ws_elems, lib.xdfm_prelu_ws_elems
    rows_seq = [1, 2, 63, 64, 65, 255, 256, 257, 520, 4096, 4097, 8200, 100000]
    for k, out in ((1, 32), (13, 32), (40, 64), (37, 96), (429, 256)):
        vals = [dw(r, k, out) for r in rows_seq]
        assert all(v > 0 for v in vals) and vals == sorted(vals), (k, out, vals)
        for r, v in zip(rows_seq, vals):
            # the plain call's slabs and bias partials, then one double per (64-wide tile of out, split)
            assert v >= plain(r, k, out) + 2 * -(-out // 64) and v % 2 == 0, (r, k, out, v)
        assert dw(257, k, out) > dw(256, k, out)
    assert plain(4096, 429, 256) == 16 * (256 * 429 + 256)         # unchanged by this addition
    for bad in [(0, 8, 32), (-1, 8, 32), (8, 0, 32), (8, 8, 0), (8, 8, 40), (8, 8, 31), (8, 8, -32)]:
        assert dw(*bad) == 0, bad
    for cols in (1, 31, 33, 64, 65, 256, 1000):
        vals = [ew(r, cols) for r in rows_seq]
        assert all(v > 0 for v in vals) and vals == sorted(vals) and all(v % 2 == 0 for v in vals), (cols, vals)
    vals = [ew(4096, c) for c in (1, 2, 63, 64, 65, 256, 1000)]
    assert vals == sorted(vals) and ew(4096, 65) > ew(4096, 64) and ew(65, 64) > ew(64, 64)
    for bad in [(0, 8), (-1, 8), (8, 0), (8, -3)]:
        assert ew(*bad) == 0, bad


def test_validation_before_device_work():
    """rc 1 (XDFM_ERR_INVALID) and a message naming the call and the argument, with no GPU in the machine: every refusal
    returns before any device work."""
    mod, lib = _lib()
    buf = (ctypes.c_float * 64)()
    buf2 = (ctypes.c_float * 64)()
    p, q = ctypes.cast(buf, P), ctypes.cast(buf2, P)      # non-null host addresses: validation must reject before touching them
    assert ctypes.addressof(buf) % 8 == 0
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)

    def err():
        return lib.xdfm_last_error()

    def fwd(x=p, rows=4, k=8, ldx=8, W=p, out=32, b=p, alpha=p, y=p, ldy=32, z=q, ldz=32):
        return lib.xdfm_dense_prelu_fwd(x, rows, k, ldx, W, out, b, alpha, y, ldy, z, ldz, None)

    def bwx(g=p, ldg=32, z=p, ldz=32, alpha=p, rows=4, out=32, W=p, k=8, dx=p, lddx=8):
        return lib.xdfm_dense_prelu_bwd_x(g, ldg, z, ldz, alpha, rows, out, W, k, dx, lddx, None)

    def bww(g=p, ldg=32, z=p, ldz=32, alpha=p, x=p, ldx=8, rows=4, k=8, out=32, ws=p, dW=p, db=p, dalpha=p):
        return lib.xdfm_dense_prelu_bwd_w(g, ldg, z, ldz, alpha, x, ldx, rows, k, out, ws, dW, db, dalpha, None)

    def efwd(u=p, ldu=8, rows=4, cols=8, alpha=p, y=p, ldy=8):
        return lib.xdfm_prelu_fwd(u, ldu, rows, cols, alpha, y, ldy, None)

    def ebwd(g=p, ldg=8, u=p, ldu=8, rows=4, cols=8, alpha=p, du=p, lddu=8, dalpha=p, ws=p):
        return lib.xdfm_prelu_bwd(g, ldg, u, ldu, rows, cols, alpha, du, lddu, dalpha, ws, None)

    dense = {"dense_prelu_fwd": (fwd, ("x", "W", "alpha", "y"), ("ldx", "ldy", "ldz")),
             "dense_prelu_bwd_x": (bwx, ("g", "z", "alpha", "W", "dx"), ("ldg", "ldz", "lddx")),
             "dense_prelu_bwd_w": (bww, ("g", "z", "alpha", "x", "dW", "ws"), ("ldg", "ldz", "ldx"))}
    for name, (call, ptrs, pitches) in dense.items():
        tag = name.encode()
        for arg in ptrs:
            assert call(**{arg: None}) == 1 and tag in err() and (b"null pointer" in err() or b"NULL" in err()), (name, arg, err())
        for rows in (0, -5):
            assert call(rows=rows) == 1 and b"rows = %d" % rows in err(), (name, rows, err())
        assert call(k=0) == 1 and b"in = 0" in err(), (name, err())
        for out in (0, 31, 40, -32):
            assert call(out=out) == 1 and tag in err() and b"out" in err(), (name, out, err())
        for pitch in pitches:
            assert call(**{pitch: 7}) == 1 and b"%s = 7" % pitch.encode() in err(), (name, pitch, err())
    assert fwd(y=p, z=p) == 1 and b"y == z" in err(), err()
    assert bww(ws=odd) == 1 and b"8-byte aligned" in err(), err()
    elem = {"prelu_fwd": (efwd, ("u", "alpha", "y"), ("ldu", "ldy")),
            "prelu_bwd": (ebwd, ("g", "u", "alpha"), ("ldg", "ldu", "lddu"))}
    for name, (call, ptrs, pitches) in elem.items():
        tag = name.encode()
        for arg in ptrs:
            assert call(**{arg: None}) == 1 and tag in err() and b"null pointer" in err(), (name, arg, err())
        for rows in (0, -5):
            assert call(rows=rows) == 1 and b"rows = %d" % rows in err(), (name, rows, err())
        for cols in (0, -2):
            assert call(cols=cols) == 1 and b"cols = %d" % cols in err(), (name, cols, err())
        for pitch in pitches:
            assert call(**{pitch: 7}) == 1 and b"%s = 7" % pitch.encode() in err(), (name, pitch, err())
    assert ebwd(du=None, dalpha=None) == 1 and b"both NULL" in err(), err()
    assert ebwd(ws=None) == 1 and b"workspace is NULL" in err(), err()
    assert ebwd(ws=odd) == 1 and b"8-byte aligned" in err(), err()
    # the plain forward's act stays {0, 1}
    assert lib.xdfm_dense_fwd(p, 4, 8, 8, p, 32, p, 2, p, 32, None) == 1 and b"act = 2" in err()
    with pytest.raises(ValueError, match="dense_prelu_fwd"):
        mod.check(fwd(rows=0), "dense_prelu_fwd")


def _composition(net, x):
    h = x
    for i, lin in enumerate(net.linears):
        h = F.linear(h, lin.weight, lin.bias)
        if net.use_bn:
            b = net.bn[i]
            h = F.batch_norm(h, None, None, b.weight, b.bias, True, 0.1, b.eps)
        h = F.prelu(h, net.activation_layers[i].weight)
    return h


@pytest.mark.parametrize("use_bn", [False, True])
def test_cpu_tower_equals_the_torch_composition(use_bn):
    from xdfm_amd import layers, ops
    assert ops._env_switch({"XDFM_DNN_PRELU_NATIVE": "0"}, "XDFM_DNN_PRELU_NATIVE") is False
    assert ops._env_switch({"XDFM_DNN_PRELU_NATIVE": "1"}, "XDFM_DNN_PRELU_NATIVE") is True
    assert isinstance(ops.DNN_PRELU_NATIVE, bool)
    torch.manual_seed(0)
    net = layers.DNN(5, (32, 6, 4), activation="PReLU", use_bn=use_bn, init_std=0.3)
    assert net.activation == "prelu" and len(net.activation_layers) == 3
    assert all(isinstance(m, torch.nn.PReLU) and m.weight.shape == (1,) and m.weight.item() == 0.25 for m in net.activation_layers)
    with torch.no_grad():
        for m, v in zip(net.activation_layers, (0.4, -0.3, 0.0)):
            m.weight.fill_(v)
    x = torch.randn(9, 5, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    assert not ops.dense_prelu_native(x, net.linears[0].weight, net.linears[0].bias, net.activation_layers[0].weight)
    assert not ops.prelu_native(x, net.activation_layers[0].weight)
    out = net(x)
    want = _composition(net, x2)
    assert torch.equal(out, want)
    g = torch.randn_like(out)
    params = list(net.parameters())
    got = torch.autograd.grad(out, [x] + params, g)
    ref = torch.autograd.grad(want, [x2] + params, g)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # float64 and other ranks go to torch as well
    a = torch.tensor([0.3], dtype=torch.float64)
    u = torch.randn(2, 3, 4, dtype=torch.float64)
    assert torch.equal(ops.prelu(u, a), F.prelu(u, a))


REFERENCE_KEYS = {False: ["linears.0.weight", "linears.0.bias", "linears.1.weight", "linears.1.bias",
                          "activation_layers.0.weight", "activation_layers.1.weight"],
                  True: ["linears.0.weight", "linears.0.bias", "linears.1.weight", "linears.1.bias"]
                  + ["bn.%d.%s" % (i, n) for i in (0, 1) for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
                  + ["activation_layers.0.weight", "activation_layers.1.weight"]}


@pytest.mark.parametrize("use_bn", [False, True])
def test_state_dict_keys_are_the_references(use_bn):
    from xdfm_amd import layers
    g = load_golden("dnn_prelu/prelu_xdeepfm" + ("_bn" if use_bn else ""))     # the list the reference itself wrote
    net = layers.DNN(g["dnn_in"].shape[1], tuple(int(v) for v in g["dnn"]), activation="prelu", use_bn=use_bn)
    assert list(net.state_dict()) == REFERENCE_KEYS[use_bn]
    recorded = [k[len("init:dnn."):] for k in g if k.startswith("init:dnn.")]
    assert recorded == REFERENCE_KEYS[use_bn]
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == g["init:dnn." + k].shape, k
        if "activation_layers" in k:
            assert v.item() == float(g["init:dnn." + k][0]) == 0.25


def _tiny_model(**kw):
    from deepctr.inputs import SparseFeat, DenseFeat
    from deepctr.models import xDeepFM
    cols = [SparseFeat("C%d" % i, 7, 4) for i in range(3)] + [DenseFeat("I0", 1)]
    return xDeepFM(cols, cols, cin_layer_size=(6, 4), dnn_hidden_units=(8, 5), l2_reg_dnn=1e-5, device="cpu", **kw)


def test_slopes_are_l2_regularised_with_l2_reg_dnn():
    model = _tiny_model(dnn_activation="prelu", dnn_use_bn=True)
    slopes = [m.weight for m in model.dnn.activation_layers]
    groups = {}
    for weight_list, l1, l2 in model.regularization_weight:
        for w in weight_list:
            groups[id(w[1] if isinstance(w, tuple) else w)] = (l1, l2)
    assert all(groups.get(id(p)) == (0.0, 1e-5) for p in slopes), groups
    assert all(id(p) not in groups for n, p in model.dnn.named_parameters() if "bn" in n)     # the reference's filter, unchanged
    g = load_golden("dnn_prelu/prelu_xdeepfm_bn")
    recorded = [str(k) for k in g["l2_reg_dnn_keys"]]            # what the reference's own filter selected
    assert all("activation_layers.%d.weight" % i in recorded for i in (0, 1)) and not [k for k in recorded if "bn" in k]


@pytest.mark.parametrize("act", ["relu", "sigmoid", "linear"])
def test_other_activations_have_no_activation_layers(act):
    from xdfm_amd import layers
    for use_bn in (False, True):
        net = layers.DNN(10, (8, 5), activation=act, use_bn=use_bn)
        assert not hasattr(net, "activation_layers")
        assert not [k for k in net.state_dict() if "activation" in k]
    assert not [k for k in _tiny_model(dnn_activation=act).state_dict() if "activation_layers" in k]


def test_refused_activations_stay_refused():
    from xdfm_amd import layers
    with pytest.raises(NotImplementedError, match="reference's own tower fails"):
        layers.DNN(10, (8, 5), activation="dice")
    with pytest.raises(NotImplementedError, match="reference's own tower fails"):
        layers.DNN(10, (8, 5), activation="Dice")
    for bad in (torch.nn.PReLU, torch.nn.PReLU(), torch.nn.ReLU, "tanh"):
        with pytest.raises(NotImplementedError):
            layers.DNN(10, (8, 5), activation=bad)
    with pytest.raises(NotImplementedError):
        _tiny_model(cin_activation="prelu")
    with pytest.raises(NotImplementedError):
        layers.CIN(5, (6, 4), activation="prelu")
    from xdfm_amd import ops
    assert ops.ACT_CODES == {"linear": 0, "relu": 1, "sigmoid": 2}


def test_trainer_parses_dnn_activation():
    import xdftrain_amd as tr
    assert tr.parse_args(["--synthetic", "64"]).dnn_activation == "relu"
    for act in ("relu", "linear", "sigmoid", "prelu"):
        assert tr.parse_args(["--synthetic", "64", "--dnn_activation", act]).dnn_activation == act
    with pytest.raises(SystemExit):
        tr.parse_args(["--synthetic", "64", "--dnn_activation", "dice"])
