#!/usr/bin/env python3
"""Generate tests/golden/varlen_pool_<mode>.npz, varlen_pool_max_empty.npz and varlen_model_{xdeepfm,attn}.npz by RUNNING THE REFERENCE on
multi-valued columns (VarLenSparseFeat: deepctr/inputs.py:141-155, :213-227; deepctr/layers/sequence.py:9-77).

make_golden.py's import recipe is reused.  The files are data only.

varlen_pool_<mode>.npz: the reference's own SequencePoolingLayer on rows looked up in a random [V, D] table, for both mask
kinds (`zero`: mask = id != 0; `len`: mask = t < length; max has no `len` golden, the reference raises there), with the gradient of the table for a random upstream gradient.
Their max sequences all hold a valid item; varlen_pool_max_empty.npz is the zero-mask max case with empty sequences.
A file whose arrays come out as they are stored is left untouched (an .npz carries its writing time).

varlen_model_*.npz: the whole reference model on 3 SparseFeat, 3 VarLenSparseFeat (mean / zero mask, sum / length column,
max / zero mask) and 2 DenseFeat: initial state_dict after the constructor alone, y_pred and every gradient of step 1 on the
livelier copy of the weights (0.3 * randn, as make_golden.py), the state after three Adam steps, the linear logit, predict.

The model is also run in float64; `bar_share_32_vs_64` is the worst share of the model-golden bars of tests/test_gpu_parity.py
(y_pred rtol 2e-5 / atol 1e-6; gradients rtol 2e-4 / atol 2e-5 * max + 1e-9; state after three steps rtol 1e-3 / atol 2e-5)
that the reference's own fp32 / fp64 difference uses.  It has to stay below 0.5.  Learning rate: Adam's first update is
lr * g / (|g| + eps), i.e. about +-lr whatever the gradient's size, so an element whose gradient is rounding noise may move
by 2 * lr differently in the two precisions.  At the default 1e-3 the share stays below 0.5 for the seeds below (printed
by this script), so the default rate is kept.
Usage:  python tests/golden/make_golden_varlen.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                      # noqa: E402  (registers the reference's deepctr package)
from make_golden import _np                   # noqa: E402
from deepctr.inputs import SparseFeat, DenseFeat, VarLenSparseFeat, build_input_features   # noqa: E402
from deepctr.layers.sequence import SequencePoolingLayer        # noqa: E402
from deepctr.models.xdeepfm import xDeepFM                      # noqa: E402
from deepctr.models.xdeepfm_attn import xDeepFMAttention        # noqa: E402

LR = 1e-3                                     # compile("adam")'s default; see the module docstring
D = 4
B = 6


def _save(name, **arrays):
    """Writes name.npz unless the file is there and already holds exactly these arrays: an .npz carries the time it was
    written, so rewriting equal data would still change the committed bytes."""
    path = os.path.join(HERE, name + ".npz")
    if os.path.exists(path):
        with np.load(path, allow_pickle=False) as z:
            old = {k: z[k] for k in z.files}
        if list(old) == list(arrays) and all(
                old[k].dtype == np.asarray(v).dtype and np.array_equal(old[k], np.asarray(v), equal_nan=old[k].dtype.kind == "f")
                for k, v in arrays.items()):
            print("kept  %-34s (same arrays, file untouched)" % (name + ".npz"))
            return
    mg._save(name, **arrays)


def gen_pool():
    Bp, T, V = 9, 5, 6
    for mode in ("sum", "mean", "max"):
        rng = np.random.default_rng({"sum": 11, "mean": 12, "max": 13}[mode])
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        table = torch.randn(V, D, generator=g)
        upstream = torch.randn(Bp, D, generator=g)
        lo = 1 if mode == "max" else 0        # max: at least one valid item per sequence
        # zero mask: ids 1..V-1 at the valid positions (a hole in the middle of row 2), 0 elsewhere
        n_valid = rng.integers(lo, T + 1, Bp)
        n_valid[0], n_valid[1] = T, lo        # a full row and (sum, mean) an empty one
        ids_zero = np.zeros((Bp, T), np.float32)
        for r in range(Bp):
            ids_zero[r, :n_valid[r]] = rng.integers(1, V, n_valid[r])
        ids_zero[2, :3] = (2, 0, 2)           # the same id twice, around a masked position
        # length mask: any id (0 included) at every position, padded ones too
        ids_len = rng.integers(0, V, (Bp, T)).astype(np.float32)
        lengths = rng.integers(lo, T + 1, Bp)
        lengths[0], lengths[1] = T, lo
        ids_len[3, :] = 4                      # one id repeated over the whole sequence
        arrays = dict(mode=np.array(mode), table=_np(table), upstream=_np(upstream), ids_zero=ids_zero, ids_len=ids_len,
                      lengths=lengths.astype(np.int64))
        for kind, ids in (("zero", ids_zero), ("len", ids_len)):
            if mode == "max" and kind == "len":
                # the reference itself raises here: _sequence_mask leaves the mask boolean (sequence.py:46 drops the result
                # of mask.type), and `1 - mask` of the max branch (:66) is not defined for bool tensors -- no golden
                continue
            w = table.clone().requires_grad_(True)
            idx = torch.from_numpy(ids).long()
            rows = w[idx]                                                       # [B, T, D], as nn.Embedding
            if kind == "zero":
                out = SequencePoolingLayer(mode=mode, supports_masking=True)([rows, idx != 0])
            else:
                out = SequencePoolingLayer(mode=mode, supports_masking=False)([rows, torch.from_numpy(lengths).long().view(-1, 1)])
            out = out.reshape(Bp, D)
            out.backward(upstream)
            arrays["pooled_" + kind] = _np(out)
            arrays["dtable_" + kind] = _np(w.grad)
        _save("varlen_pool_" + mode, **arrays)


def gen_pool_max_empty():
    """varlen_pool_max_empty.npz: max pooling under the zero mask with EMPTY sequences (1, 4 and 8), which gen_pool leaves
    out.  hist = emb - (1 - mask) * 1e9 and torch.max(hist, dim=1) (sequence.py:65-68): an all-masked sequence pools to
    w[0] - 1e9, and autograd sends its gradient to the first maximum, position 0, which looked row 0 up -- dtable[0] is not
    zero.  The same lookup through a [V, 1] table with an upstream gradient of its own is stored too (lin_*): the linear
    logit pools that table the same way."""
    Bp, T, V = 9, 5, 6
    rng = np.random.default_rng(14)
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    table, upstream = torch.randn(V, D, generator=g), torch.randn(Bp, D, generator=g)
    lin_table, lin_upstream = torch.randn(V, 1, generator=g), torch.randn(Bp, 1, generator=g)
    n_valid = rng.integers(1, T, Bp)
    n_valid[0] = T                            # a full row
    n_valid[[1, 4, 8]] = 0                    # the empty ones
    ids = np.zeros((Bp, T), np.float32)
    for r in range(Bp):
        ids[r, :n_valid[r]] = rng.integers(1, V, n_valid[r])
    ids[2] = (2, 0, 2, 0, 0)                  # the same id twice, around a masked position
    idx = torch.from_numpy(ids).long()
    arrays = dict(mode=np.array("max"), table=_np(table), upstream=_np(upstream), ids=ids, lin_table=_np(lin_table),
                  lin_upstream=_np(lin_upstream))
    for pre, tab, up in (("", table, upstream), ("lin_", lin_table, lin_upstream)):
        w = tab.clone().requires_grad_(True)
        out = SequencePoolingLayer(mode="max", supports_masking=True)([w[idx], idx != 0]).reshape(Bp, tab.shape[1])
        out.backward(up)
        arrays[pre + "pooled"], arrays[pre + "dtable"] = _np(out), _np(w.grad)
    empty = (ids == 0).all(1)
    assert list(np.flatnonzero(empty)) == [1, 4, 8] and np.all(arrays["dtable"][0] != 0) and np.all(arrays["lin_dtable"][0] != 0)
    _save("varlen_pool_max_empty", **arrays)


def columns():
    sparse = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate((7, 8, 9))]
    varlen = [VarLenSparseFeat(SparseFeat("g_mean", 9, D), maxlen=5, combiner="mean"),
              VarLenSparseFeat(SparseFeat("g_sum", 6, D), maxlen=3, combiner="sum", length_name="g_sum_len"),
              VarLenSparseFeat(SparseFeat("g_max", 8, D), maxlen=4, combiner="max")]
    dense = [DenseFeat("I1", 1), DenseFeat("I2", 2)]
    return sparse, varlen, dense


def batch(n, idx, sparse, varlen, seed):
    rng = np.random.default_rng(seed)
    X = np.zeros((n, max(v[1] for v in idx.values())), np.float32)
    for f in sparse:
        X[:, idx[f.name][0]] = rng.integers(0, f.vocabulary_size, n)
    for f in varlen:
        a, b = idx[f.name]
        for r in range(n):
            L = int(rng.integers(1 if f.combiner == "max" else 0, f.maxlen + 1))
            if f.combiner != "max" and r % 5 == 1:
                L = 0                                           # some empty mean and sum rows
            if f.length_name is None:
                ids = rng.integers(1, f.vocabulary_size, f.maxlen)
                ids[L:] = 0
            else:
                ids = rng.integers(0, f.vocabulary_size, f.maxlen)      # padded positions hold ids too
                X[r, idx[f.length_name][0]] = L
            X[r, a:b] = ids
    for name in ("I1", "I2"):
        a, b = idx[name]
        X[:, a:b] = rng.random((n, b - a))
    y = (rng.random(n) < 0.4).astype(np.float32)
    return X, y


def _run(cls, dtype):
    sparse, varlen, dense = columns()
    cols = sparse + varlen + dense
    model = cls(cols, cols, dnn_hidden_units=(8, 8), cin_layer_size=(8, 6), l2_reg_dnn=1e-5, device="cpu")
    init = {k: _np(v) for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding_dict" in k or k == "linear_model.weight" or "dnn" in k or k == "cin_linear.weight":
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    idx = model.feature_index
    X, y = batch(3 * B, idx, sparse, varlen, seed=2026)
    state0 = {k: _np(v) for k, v in model.state_dict().items()}
    if dtype == torch.float64:
        model.double()
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    for pg in model.optim.param_groups:
        pg["lr"] = LR
    Xt, yt = torch.from_numpy(X[:B]).to(dtype), torch.from_numpy(y[:B]).to(dtype)
    model.train()
    lin = _np(model.linear_model(Xt))
    y_pred = model(Xt)
    loss = torch.nn.functional.binary_cross_entropy(y_pred.squeeze(), yt.squeeze(), reduction="sum")
    reg = model.get_regularization_loss()
    model.optim.zero_grad()
    (loss + reg).backward()
    grads = {k: _np(p.grad) for k, p in model.named_parameters()}
    model.optim.zero_grad()
    losses = []
    for s in range(3):                         # three Adam steps exactly as BaseModel.fit does them (basemodel.py:241-262)
        xb = torch.from_numpy(X[s * B:(s + 1) * B]).to(dtype)
        yb = torch.from_numpy(y[s * B:(s + 1) * B]).to(dtype)
        yp = model(xb).squeeze()
        model.optim.zero_grad()
        l = torch.nn.functional.binary_cross_entropy(yp, yb.squeeze(), reduction="sum")
        tot = l + model.get_regularization_loss() + model.aux_loss
        losses.append([l.item(), tot.item()])
        tot.backward()
        model.optim.step()
    state3 = {k: _np(v) for k, v in model.state_dict().items()}
    pred_after = None
    if dtype == torch.float32:
        pred_after = model.predict([X[:, a:b] for a, b in idx.values()], batch_size=B)
    return dict(model=model, cols=cols, X=X, y=y, init=init, state0=state0, lin=lin, y_pred=_np(y_pred), loss=loss.item(),
                reg=reg.item(), grads=grads, losses=losses, state3=state3, pred_after=pred_after)


def _share(got, want, rtol, atol):
    want = np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    return float((np.abs(np.asarray(got, np.float64) - want) / (atol + rtol * np.abs(want))).max())


def gen_models():
    for name, cls in (("varlen_model_xdeepfm", xDeepFM), ("varlen_model_attn", xDeepFMAttention)):
        r32, r64 = _run(cls, torch.float32), _run(cls, torch.float64)
        assert np.array_equal(r32["X"], r64["X"]) and all(np.array_equal(r32["state0"][k], r64["state0"][k]) for k in r32["state0"])
        shares = {"y_pred": _share(r32["y_pred"], r64["y_pred"], 2e-5, 1e-6)}
        shares["grad"] = max(_share(v, r64["grads"][k], 2e-4, 2e-5 * float(np.abs(r64["grads"][k]).max()) + 1e-9)
                             for k, v in r32["grads"].items())
        shares["state3"] = max(_share(v, r64["state3"][k], 1e-3, 2e-5) for k, v in r32["state3"].items())
        share = max(shares.values())
        print("%s: fp32 against fp64 reference run, share of the bars %s; losses %s" % (name, shares, r32["losses"]))
        assert share < 0.5, (name, shares)
        model, idx = r32["model"], r32["model"].feature_index
        assert len(model.embedding_dict) == 6                      # one CIN field per sparse and per variable-length column
        arrays = dict(X=r32["X"], y=r32["y"], B=np.array(B), emb_dim=np.array(D), lr=np.array(LR), cls=np.array(cls.__name__),
                      y_pred=r32["y_pred"], loss=np.array(r32["loss"]), reg=np.array(r32["reg"]), lin_logit=r32["lin"],
                      losses3=np.array(r32["losses"]), losses3_64=np.array(r64["losses"]), pred_after=r32["pred_after"],
                      bar_share_32_vs_64=np.array(share), feature_names=np.array(list(idx.keys())),
                      feature_lo=np.array([v[0] for v in idx.values()]), feature_hi=np.array([v[1] for v in idx.values()]),
                      dnn_input_dim=np.array(model.compute_input_dim(r32["cols"])),
                      state_keys=np.array(list(r32["init"].keys())))
        for k, v in r32["init"].items():
            arrays["init:" + k] = v
        for k, v in r32["state0"].items():
            arrays["s0:" + k] = v
        for k, v in r32["grads"].items():
            arrays["g:" + k] = v
        for k, v in r32["state3"].items():
            arrays["s3:" + k] = v
        _save(name, **arrays)


if __name__ == "__main__":
    torch.set_num_threads(4)
    gen_pool()
    gen_pool_max_empty()
    gen_models()
