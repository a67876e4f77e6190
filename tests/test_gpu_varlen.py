"""GPU tests (-m gpu) of the pooled variable-length fields: K1v / K2v through the C ABI against the float64 restatement
(tests/varlen_ref.py, pinned to the reference by tests/test_varlen_host.py), and the models against the reference's goldens.

Bars of the kernel tests (derived, eps = 2^-24):
  max forward            exact: a valid position carries w itself, a masked one the single fp32 subtraction w - 1e9;
  sum / mean forward     (maxlen + 2) * eps * sum_t |w_t| per element (mean: both sides divided by the fp32 divisor): at most
                         maxlen - 1 roundings of partial sums that never exceed sum |w_t|, one for the division, one for the
                         divisor;
  table gradients        (n + 2) * eps * sum |addends| per element, n = addends of that row: holds for any fp32 summation order
                         (K2 itself rounds once per chunk of 4096 positions), and covers one rounding of each addend;
  rows without addends   exactly zero."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import varlen_ref as vr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
EPS = vr.EPS32
MODES = ("sum", "mean", "max")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Case:
    """Random inputs of one launch: fields = [(combiner, 'zero' | 'len', maxlen, vocab)]."""

    def __init__(self, B, D, fields, has_lin=True, seed=0, slot0=2, pad=3):
        rng = np.random.default_rng(seed)
        self.B, self.D, self.fields, self.has_lin, self.slot0 = B, D, fields, has_lin, slot0
        self.F = F = len(fields)
        self.dnn_off, self.ld = slot0 * D, (slot0 + F) * D + pad
        ncol = 1 + sum(f[2] for f in fields) + F
        self.X = np.zeros((B, ncol), np.float32)
        self.X[:, 0] = rng.integers(0, 5, B)                      # a column that belongs to nobody
        self.desc, self.tables, self.lins = [], [], []
        col = 1
        for f, (mode, kind, Tn, V) in enumerate(fields):
            lo = 1 if mode == "max" else 0                         # max: at least one valid item
            L = rng.integers(lo, Tn + 1, B)
            if mode != "max":
                L[rng.random(B) < 0.15] = 0                       # empty mean and sum rows
            if kind == "zero":
                ids = rng.integers(1, V, (B, Tn))
                ids[np.arange(Tn)[None, :] >= L[:, None]] = 0
                len_col = -1
            else:
                ids = rng.integers(0, V, (B, Tn))                  # padded positions hold ids too
                len_col = ncol - F + f
                self.X[:, len_col] = L
            ids[0, :] = ids[0, 0]                                  # a sequence with the same id repeated
            self.X[:, col:col + Tn] = ids
            self.desc.append((col, Tn, len_col, MODES.index(mode), V))
            self.tables.append(rng.standard_normal((V, D)).astype(np.float32))
            self.lins.append(rng.standard_normal((V, 1)).astype(np.float32))
            col += Tn
        self.lin0 = rng.standard_normal(B).astype(np.float32)
        self.d_emb = rng.standard_normal((slot0 + F, B * D)).astype(np.float32)
        self.d_dnn = rng.standard_normal((B, self.ld)).astype(np.float32)
        self.d_lin = rng.standard_normal(B).astype(np.float32)

    def ids(self, f, X=None):
        X = self.X if X is None else X
        col, Tn, len_col, _, _ = self.desc[f]
        return X[:, col:col + Tn], (None if len_col < 0 else X[:, len_col])


class Device:
    """The case's arrays on the GPU and the two entry points."""

    def __init__(self, case, dev, X=None):
        from xdfm_amd import _lib
        self.lib, self.c, self.dev = _lib.load(), case, dev
        c = case
        self.X = T(np.ascontiguousarray(c.X if X is None else X)).to(dev)
        self.tables = [T(t).to(dev) for t in c.tables]
        self.lins = [T(t).to(dev) for t in c.lins]
        self.host = (_lib.VarLenField * c.F)()
        for f, (col, Tn, len_col, comb, V) in enumerate(c.desc):
            h = self.host[f]
            h.table, h.lin = self.tables[f].data_ptr(), (self.lins[f].data_ptr() if c.has_lin else None)
            h.col, h.maxlen, h.len_col, h.combiner, h.vocab = col, Tn, len_col, comb, V
        self.desc = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def forward(self, lin0=None):
        c, B = self.c, self.X.shape[0]
        self.emb = torch.full((c.slot0 + c.F, B * c.D), 7.0, device=self.dev)
        self.dnn = torch.full((B, c.ld), 7.0, device=self.dev)
        self.lin = T((c.lin0 if lin0 is None else lin0).copy()).to(self.dev) if c.has_lin else None
        self.argpos = torch.zeros((B, c.F, c.D + 1), dtype=torch.uint8, device=self.dev)
        rc = self.lib.xdfm_varlen_pool_fwd(_p(self.X), self.X.stride(0), B, _p(self.desc), ctypes.cast(self.host, ctypes.c_void_p),
                                           c.F, c.D, c.slot0, _p(self.emb), _p(self.dnn), c.ld, c.dnn_off, _p(self.lin),
                                           _p(self.argpos), _p(self.flag), None)
        assert rc == 0, self.lib.xdfm_last_error()
        torch.cuda.synchronize()
        return self.emb.cpu().numpy(), self.dnn.cpu().numpy(), (self.lin.cpu().numpy() if c.has_lin else None)

    def backward(self, d_emb=None, d_dnn=None, d_lin=None):
        c, B = self.c, self.X.shape[0]
        shapes = [t.shape for t in c.tables] + ([t.shape for t in c.lins] if c.has_lin else [])
        offs, off = [], 0
        for sh in shapes:
            offs.append(off)
            off += (sh[0] * sh[1] + 3) // 4 * 4
        flat = torch.zeros(off, device=self.dev)
        off_dev = torch.tensor(offs, dtype=torch.int64, device=self.dev)
        cols = torch.arange(c.F, dtype=torch.int32, device=self.dev)
        vocab = torch.tensor([d[4] for d in c.desc], dtype=torch.int32, device=self.dev)
        Tmax = max(d[1] for d in c.desc)
        ws = torch.empty(self.lib.xdfm_varlen_pool_bwd_ws_elems(B, c.F, c.D, Tmax), device=self.dev)
        de = T(c.d_emb if d_emb is None else d_emb).to(self.dev)
        dd = T(c.d_dnn if d_dnn is None else d_dnn).to(self.dev)
        dl = T(c.d_lin if d_lin is None else d_lin).to(self.dev) if c.has_lin else None
        rc = self.lib.xdfm_varlen_pool_bwd(_p(self.X), self.X.stride(0), B, _p(self.desc), ctypes.cast(self.host, ctypes.c_void_p),
                                           c.F, c.D, c.slot0, _p(de), _p(dd), c.ld, c.dnn_off, _p(dl), 1, _p(self.argpos),
                                           _p(cols), _p(vocab), _p(flat), _p(off_dev[:c.F]),
                                           _p(off_dev[c.F:]) if c.has_lin else None, _p(ws), None)
        assert rc == 0, self.lib.xdfm_last_error()
        torch.cuda.synchronize()
        flat = flat.cpu().numpy()
        return [flat[o:o + sh[0] * sh[1]].reshape(sh) for o, sh in zip(offs, shapes)]


def _check_forward(c, emb, dnn, lin, X=None):
    B, D, F = c.B, c.D, c.F
    lin_want, lin_bar = c.lin0.astype(np.float64), np.zeros(B)
    lin_mag = np.abs(c.lin0).astype(np.float64)
    for f, (mode, kind, Tn, V) in enumerate(c.fields):
        ids, lengths = c.ids(f, X)
        got = emb[c.slot0 + f].reshape(B, D)
        np.testing.assert_array_equal(got, dnn[:, c.dnn_off + f * D:c.dnn_off + (f + 1) * D])     # both consumers get the same bits
        want, mag, _ = vr.pool(ids, lengths, c.tables[f], mode)
        if mode == "max":
            np.testing.assert_array_equal(got, want, err_msg="field %d max" % f)
        else:
            err, bar = np.abs(got - want), (Tn + 2) * EPS * mag
            print("field %d %s/%s maxlen %d: worst share of the bar %.3f" % (f, mode, kind, Tn, float((err / np.maximum(bar, 1e-300)).max())))
            assert np.all(err <= bar), "field %d %s" % (f, mode)
            assert np.all(got[mag.sum(1) == 0] == 0)                                              # empty rows pool to zero
        if c.has_lin:
            lw, lm, _ = vr.pool(ids, lengths, c.lins[f], mode)
            lin_want += lw[:, 0].astype(np.float64)
            lin_mag += np.abs(lw[:, 0]).astype(np.float64)
            if mode != "max":
                lin_bar += (Tn + 2) * EPS * lm[:, 0]
    assert np.all(emb[:c.slot0] == 7.0) and np.all(dnn[:, :c.dnn_off] == 7.0) and np.all(dnn[:, c.dnn_off + F * D:] == 7.0)
    if c.has_lin:
        # the F pooled values are added up and then added to what was there: F + 1 more roundings of sums <= lin_mag
        assert np.all(np.abs(lin - lin_want) <= lin_bar + (F + 1) * EPS * lin_mag)


def _upstream(c, d_emb=None, d_dnn=None):
    d_emb = c.d_emb if d_emb is None else d_emb
    d_dnn = c.d_dnn if d_dnn is None else d_dnn
    return [d_emb[c.slot0 + f].reshape(-1, c.D) + d_dnn[:, c.dnn_off + f * c.D:c.dnn_off + (f + 1) * c.D] for f in range(c.F)]   # one fp32 add


def _check_backward(c, grads, X=None, ups=None, d_lin=None):
    ups = _upstream(c) if ups is None else ups
    d_lin = c.d_lin if d_lin is None else d_lin
    for f, (mode, kind, Tn, V) in enumerate(c.fields):
        ids, lengths = c.ids(f, X)
        todo = [(grads[f], c.tables[f], ups[f], "table")]
        if c.has_lin:
            todo.append((grads[c.F + f], c.lins[f], d_lin[:, None], "linear table"))
        for got, table, up, what in todo:
            want, ab, n = vr.pool_grad(ids, lengths, table, mode, up)
            err, bar = np.abs(got - want), (n[:, None] + 2) * EPS * ab
            print("field %d %s/%s %s: worst share of the bar %.3f, most addends per row %d" % (
                f, mode, kind, what, float((err / np.maximum(bar, 1e-300)).max()), int(n.max())))
            assert np.all(err <= bar), "field %d %s %s" % (f, mode, what)
            assert np.all(got[n == 0] == 0), "field %d: rows without addends must be exactly zero" % f


MIX_A = lambda t: [("mean", "zero", t[0], 13), ("sum", "len", t[1], 7), ("max", "zero", t[2], 9)]
MIX_B = lambda t: [("max", "len", t[0], 11), ("mean", "len", t[1], 2), ("sum", "zero", t[2], 300)]
CASES = {
    "B1-D4-F1":            dict(B=1, D=4, fields=[("sum", "zero", 1, 5)]),
    "B67-D10-F3":          dict(B=67, D=10, fields=MIX_A((3, 20, 1))),
    "B300-D16-F3":         dict(B=300, D=16, fields=MIX_B((20, 3, 20))),          # 6000 positions per field: two chunks of K2's reduce
    "B67-D16-F1-vocab2":   dict(B=67, D=16, fields=[("mean", "len", 20, 2)], has_lin=False),   # every position hits one of two rows
    "B300-D4-F3-nolin":    dict(B=300, D=4, fields=MIX_A((1, 3, 20)), has_lin=False),
    "B1-D10-F3":           dict(B=1, D=10, fields=MIX_B((3, 1, 20))),
    "B300-D10-F1-max":     dict(B=300, D=10, fields=[("max", "zero", 20, 2)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_pool_kernels_vs_float64(name):
    dev = _dev()
    c = Case(seed=sum(map(ord, name)), **CASES[name])
    d = Device(c, dev)
    emb, dnn, lin = d.forward()
    _check_forward(c, emb, dnn, lin)
    assert int(d.flag.item()) == 0
    grads = d.backward()
    _check_backward(c, grads)
    again = d.backward()
    for a, b in zip(grads, again):
        np.testing.assert_array_equal(a, b)                                 # bit-identical from run to run


def test_permuting_the_examples():
    """The forward is a function of the example alone: bit-identical per example.  The table gradients are exact sums per
    chunk of K2's reduce; across the two chunks of this case the grouping changes with the order, so they keep the bar."""
    dev = _dev()
    c = Case(seed=5, **CASES["B300-D16-F3"])
    emb, dnn, lin = Device(c, dev).forward()
    perm = np.random.default_rng(1).permutation(c.B)
    Xp = c.X[perm]
    dp = Device(c, dev, X=Xp)
    emb_p, dnn_p, lin_p = dp.forward(lin0=c.lin0[perm])
    np.testing.assert_array_equal(emb_p[c.slot0:].reshape(c.F, c.B, c.D), emb[c.slot0:].reshape(c.F, c.B, c.D)[:, perm])
    np.testing.assert_array_equal(dnn_p, dnn[perm])
    np.testing.assert_array_equal(lin_p, lin[perm])
    d_emb_p = c.d_emb.reshape(-1, c.B, c.D)[:, perm].reshape(c.d_emb.shape).copy()
    d_dnn_p, d_lin_p = c.d_dnn[perm].copy(), c.d_lin[perm].copy()
    grads = dp.backward(d_emb_p, d_dnn_p, d_lin_p)
    _check_backward(c, grads, X=Xp, ups=_upstream(c, d_emb_p, d_dnn_p), d_lin=d_lin_p)


def test_out_of_range_id_at_a_padded_position_raises_the_flag():
    """The reference looks up every position, padded ones included (inputs.py:224-225), so an id outside the table is
    an error wherever it sits; the kernel clamps it and raises K1's deferred flag."""
    dev = _dev()
    c = Case(seed=9, B=67, D=4, fields=[("sum", "len", 3, 7), ("mean", "zero", 3, 5)])
    col, Tn, len_col, _, V = c.desc[0]
    c.X[5, len_col] = 1
    d = Device(c, dev)
    d.forward()
    assert int(d.flag.item()) == 0
    bad = c.X.copy()
    bad[5, col + 2] = V                                       # position 2 of a sequence of length 1
    d = Device(c, dev, X=bad)
    emb, dnn, lin = d.forward()
    assert int(d.flag.item()) == 1
    _check_forward(c, emb, dnn, lin, X=bad)                   # the masked position changes nothing
    neg = c.X.copy()
    neg[7, c.desc[1][0]] = -2.0
    d = Device(c, dev, X=neg)
    d.forward()
    assert int(d.flag.item()) == 1


# ------------------------------------------------------------------------------------------------- models
def close(got, want, rtol, atol, msg=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=msg)


@pytest.mark.parametrize("name", ["varlen_model_xdeepfm", "varlen_model_attn"])
def test_model_vs_reference_golden(name):
    """The bars are those of tests/test_gpu_parity.py::test_model_vs_reference_golden."""
    dev = _dev()
    g = load_golden(name)
    model = vr.golden_model(g, dev)
    for k, v in model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), g["init:" + k], err_msg="init " + k)
    model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
    B = int(g["B"])
    X, y = T(g["X"]).to(dev), T(g["y"]).to(dev)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    model.train()
    close(model.linear_model(X[:B]), g["lin_logit"], rtol=2e-5, atol=1e-6, msg="Linear called directly")
    y_pred = model(X[:B])
    close(y_pred, g["y_pred"], rtol=2e-5, atol=1e-6, msg="y_pred")
    loss = torch.nn.functional.binary_cross_entropy(y_pred.squeeze(), y[:B].squeeze(), reduction="sum")
    reg = model.get_regularization_loss()
    assert abs(loss.item() - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    assert abs(reg.item() - float(g["reg"])) <= 1e-5 * abs(float(g["reg"]))
    model.optim.zero_grad()
    (loss + reg).backward()
    for k, p in model.named_parameters():
        want = g["g:" + k]
        close(p.grad, want, rtol=2e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-9, msg=k)
    model.optim.zero_grad()
    losses = []
    for s in range(3):                                  # three Adam steps, as BaseModel.fit does them
        xb, yb = X[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        yp = model(xb).squeeze()
        model.optim.zero_grad()
        l = torch.nn.functional.binary_cross_entropy(yp, yb.squeeze(), reduction="sum")
        tot = l + model.get_regularization_loss() + model.aux_loss
        losses.append([l.item(), tot.item()])
        tot.backward()
        model.optim.step()
    np.testing.assert_allclose(np.array(losses), g["losses3"], rtol=2e-5)
    for k, v in model.state_dict().items():
        close(v, g["s3:" + k], rtol=1e-3, atol=2e-5, msg="after 3 steps: " + k)
    idx = model.feature_index
    Xn = g["X"]
    feed = {n: Xn[:, a:b] for n, (a, b) in idx.items()}
    pred = model.predict(feed, batch_size=B)
    assert pred.dtype == np.float64 and pred.shape == (Xn.shape[0], 1)
    from xdfm_amd import metrics as M
    assert abs(M.log_loss(g["y"], pred) - M.log_loss(g["y"], g["pred_after"])) < 1e-5
    assert abs(M.roc_auc_score(g["y"], pred) - M.roc_auc_score(g["y"], g["pred_after"])) < 1e-5
    # an id outside the table, at a padded position of the length-masked column: IndexError at the end of predict
    bad = Xn.copy()
    a, b = idx["g_sum"]
    bad[4, idx["g_sum_len"][0]] = 1
    bad[4, b - 1] = 6
    with pytest.raises(IndexError, match="vocabulary_size"):
        model.predict({n: bad[:, lo:hi] for n, (lo, hi) in idx.items()}, batch_size=B)
    model.predict(feed, batch_size=B)                   # the flag was cleared


def test_train_step_replayed_from_the_graph_equals_the_eager_twin():
    from xdfm_amd import graphstep
    dev = _dev()
    g = load_golden("varlen_model_xdeepfm")
    X, y = T(g["X"]).to(dev), T(g["y"]).to(dev)
    B = int(g["B"])

    def run(use_graph):
        model = vr.golden_model(g, dev)
        model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
        model.compile("adam", "binary_crossentropy", metrics=[])
        model.train()
        step = graphstep.GraphedStep(model)
        step.disabled = not use_graph
        model.__dict__["_graphed_step"] = step
        for s in range(5):
            k = s % 3
            model.train_on_batch(X[k * B:(k + 1) * B], y[k * B:(k + 1) * B])
        torch.cuda.synchronize()
        return model, step

    m_g, st_g = run(True)
    m_e, st_e = run(False)
    assert st_g.replays == 3 and not st_g.disabled and st_e.replays == 0
    for (k, a), (_, b) in zip(m_g.state_dict().items(), m_e.state_dict().items()):
        assert torch.equal(a, b), k
    assert not torch.equal(m_g.state_dict()["embedding_dict.g_max.weight"].cpu(), T(g["s0:embedding_dict.g_max.weight"]))


def test_linear_called_directly_and_input_from_feature_columns():
    dev = _dev()
    g = load_golden("varlen_model_xdeepfm")
    model = vr.golden_model(g, dev)
    model.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("s0:")}, strict=True)
    B = int(g["B"])
    X = T(g["X"][:B]).to(dev)
    from deepctr.models.basemodel import Linear
    sparse, varlen, dense = vr.golden_columns(g)
    lin = Linear(sparse + varlen + dense, model.feature_index, device=dev)
    lin.load_state_dict(model.linear_model.state_dict())
    close(lin(X), g["lin_logit"], rtol=2e-5, atol=1e-6, msg="linear logit")
    embs, dense_vals = model.input_from_feature_columns(X, model.dnn_feature_columns, model.embedding_dict)
    assert len(embs) == 6 and all(tuple(e.shape) == (B, 1, 4) for e in embs) and len(dense_vals) == 2
    emb_fm, dnn_in, _ = model.fused_inputs(X)
    for j, e in enumerate(embs):
        assert torch.equal(e.reshape(B, 4), emb_fm[j].reshape(B, 4)) and torch.equal(e.reshape(B, 4), dnn_in[:, 4 * j:4 * j + 4])
    for f, fc in enumerate(varlen):                     # the pooled rows against the restatement, through the public interface
        a, b = model.feature_index[fc.name]
        lengths = None if fc.length_name is None else g["X"][:B, model.feature_index[fc.length_name][0]]
        want, mag, _ = vr.pool(g["X"][:B, a:b], lengths, g["s0:embedding_dict.%s.weight" % fc.name], fc.combiner)
        got = embs[3 + f].detach().reshape(B, 4).cpu().numpy()
        if fc.combiner == "max":
            np.testing.assert_array_equal(got, want)
        else:
            assert np.all(np.abs(got - want) <= (fc.maxlen + 2) * EPS * mag)
