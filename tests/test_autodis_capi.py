"""CPU: the C ABI of the native AutoDis op (csrc/autodis.hip) -- symbols, argument validation before any device work, the
envelope and the workspace formula of include/xdfm.h -- and AutoDisLayer's unchanged CPU behaviour: the stock per-field
loop, the reference's state_dict keys, shapes and seeded initial values."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "xdfm.h")
NAMES = ["xdfm_autodis_supported", "xdfm_autodis_ws_elems", "xdfm_autodis_fwd", "xdfm_autodis_bwd"]
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
    assert lib.xdfm_abi_version() == 9           # additive change


def test_supported_envelope_edges():
    _, lib = _lib()
    from xdfm_amd import ops
    for K, D, want in [(1, 1, 1), (6, 4, 1), (16, 16, 1), (32, 64, 1), (33, 64, 0), (32, 65, 0), (0, 8, 0), (8, 0, 0), (48, 8, 0),
                       (-1, 8, 0)]:
        assert lib.xdfm_autodis_supported(K, D) == want, (K, D)
        assert ops.autodis_supported(K, D) is bool(want)


def test_workspace_formula():
    """ceil(B / R) * F * (K * D + K * K + 3 * K + 1), R = 256 rows per workgroup for K <= 16 and 128 above (include/xdfm.h)."""
    _, lib = _lib()
    assert lib.xdfm_autodis_ws_elems(4096, 13, 16, 16) == 16 * 13 * (16 * 16 + 16 * 16 + 3 * 16 + 1)
    assert lib.xdfm_autodis_ws_elems(4099, 3, 32, 10) == 33 * 3 * (32 * 10 + 32 * 32 + 3 * 32 + 1)
    assert lib.xdfm_autodis_ws_elems(257, 40, 17, 64) == 3 * 40 * (17 * 64 + 17 * 17 + 3 * 17 + 1)
    assert lib.xdfm_autodis_ws_elems(1, 1, 1, 1) == 1 * 1 * (1 + 1 + 3 + 1)
    for bad in [(4096, 13, 33, 16), (4096, 13, 16, 65), (0, 13, 16, 16), (4096, 0, 16, 16)]:
        assert lib.xdfm_autodis_ws_elems(*bad) == 0, bad


def test_validation_before_device_work():
    """Null pointers and K, D, F, B out of range: rc 1 and a message, with no GPU in the machine."""
    mod, lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)                        # a non-null host address: validation must reject before touching it

    def fwd(x=p, ldx=13, B=8, F=13, K=16, D=16, meta=p, proj=p, temp=p, out=p):
        return lib.xdfm_autodis_fwd(x, ldx, B, F, K, D, meta, proj, temp, out, None)

    def bwd(x=p, ldx=13, B=8, F=13, K=16, D=16, meta=p, proj=p, temp=p, g=p, ldg=13 * 16, flags=127, ws=p, grads=p, dx=p):
        return lib.xdfm_autodis_bwd(x, ldx, B, F, K, D, meta, proj, temp, g, ldg, flags, ws, grads, dx, None)

    for arg in ("x", "meta", "proj", "temp", "out"):
        assert fwd(**{arg: None}) == 1 and b"null pointer" in lib.xdfm_last_error(), arg
    for arg in ("x", "meta", "proj", "temp", "g", "ws", "grads", "dx"):
        assert bwd(**{arg: None}) == 1 and b"null pointer" in lib.xdfm_last_error(), arg
    for call in (fwd, bwd):
        for kw, word in [(dict(K=0), b"K = 0"), (dict(K=33), b"K = 33"), (dict(D=0), b"D = 0"), (dict(D=65), b"D = 65"),
                         (dict(F=0), b"F = 0"), (dict(B=0), b"B = 0"), (dict(B=-5), b"B = -5"), (dict(ldx=12), b"ldx")]:
            assert call(**kw) == 1, kw
            assert word in lib.xdfm_last_error(), (kw, lib.xdfm_last_error())
    assert bwd(ldg=13 * 16 - 1) == 1 and b"ldg" in lib.xdfm_last_error()
    assert bwd(flags=0) == 1 and b"flags" in lib.xdfm_last_error()
    assert bwd(flags=128) == 1 and b"flags" in lib.xdfm_last_error()
    with pytest.raises(ValueError, match="autodis_fwd"):
        mod.check(fwd(K=40), "autodis_fwd")


def _composition(layer, dense_values):
    """deepctr/xdeepfm_pro/autodis.py:99-125, spelled out on the layer's parameters."""
    embs = []
    for i, v in enumerate(dense_values):
        if v.dim() == 1:
            v = v.unsqueeze(-1)
        seq = layer.bucket_projectors[i]
        h = F.linear(v, seq[0].weight, seq[0].bias)
        a = F.leaky_relu(h, 0.2)
        s = F.linear(a, seq[2].weight, seq[2].bias)
        w = F.softmax(s / layer.feature_temperatures[i], dim=-1)
        embs.append(torch.matmul(w, layer.meta_embeddings[i]).unsqueeze(1))
    return torch.cat(embs, dim=1).view(dense_values[0].shape[0], -1), embs


@pytest.mark.parametrize("K,D", [(6, 4), (16, 16), (48, 8)])
def test_cpu_layer_is_the_stock_loop_bit_for_bit(K, D):
    from deepctr.xdeepfm_pro.autodis import AutoDisLayer
    from xdfm_amd import ops
    torch.manual_seed(7)
    layer = AutoDisLayer(5, K, D, temperature=0.7)
    with torch.no_grad():
        layer.meta_embeddings.mul_(30.0)
    x = torch.randn(37, 5)
    x[::4] = 0.0
    vals = [x[:, i:i + 1].clone().requires_grad_(True) for i in range(5)]
    vals2 = [v.detach().clone().requires_grad_(True) for v in vals]
    before = ops.AutoDis.calls
    flat, lst = layer(vals)
    assert ops.AutoDis.calls == before, "CPU tensors must not reach the native op"
    want, want_lst = _composition(layer, vals2)
    assert flat.shape == (37, 5 * D) and torch.equal(flat, want)
    assert len(lst) == 5 and all(a.shape == (37, 1, D) and torch.equal(a, b) for a, b in zip(lst, want_lst))
    gout = torch.randn(37, 5 * D)
    (flat * gout).sum().backward()
    got = [p.grad.clone() for p in layer.parameters()] + [v.grad for v in vals]
    layer.zero_grad(set_to_none=True)
    (want * gout).sum().backward()
    for a, b in zip(got, [p.grad for p in layer.parameters()] + [v.grad for v in vals2]):
        assert torch.equal(a, b)
    # 1-D dense values are accepted as before
    flat1, _ = layer([x[:, i] for i in range(5)])
    assert torch.equal(flat1, want)


def test_state_dict_keys_shapes_and_seeded_init():
    """Same keys, shapes and initial draw order as the reference's constructor: randn meta-embeddings first, then per
    field Linear(1, K) and Linear(K, K), then the temperatures."""
    from deepctr.xdeepfm_pro.autodis import AutoDisLayer
    Fn, K, D = 3, 6, 4
    torch.manual_seed(1234)
    layer = AutoDisLayer(Fn, K, D, temperature=0.5)
    torch.manual_seed(1234)
    meta = torch.randn(Fn, K, D) * 0.01
    projs = [nn.Sequential(nn.Linear(1, K), nn.LeakyReLU(0.2), nn.Linear(K, K)) for _ in range(Fn)]
    want = {"meta_embeddings": meta, "feature_temperatures": torch.ones(Fn) * 0.5}
    for i, seq in enumerate(projs):
        for j in (0, 2):
            want["bucket_projectors.%d.%d.weight" % (i, j)] = seq[j].weight.detach()
            want["bucket_projectors.%d.%d.bias" % (i, j)] = seq[j].bias.detach()
    sd = layer.state_dict()
    assert sorted(sd.keys()) == sorted(want.keys())
    for k, v in want.items():
        assert sd[k].shape == v.shape, k
        assert torch.equal(sd[k], v), k
    assert sd["bucket_projectors.0.0.weight"].shape == (K, 1) and sd["bucket_projectors.0.2.weight"].shape == (K, K)
    assert [k for k, _ in layer.named_parameters()][0] == "meta_embeddings"
