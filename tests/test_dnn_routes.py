"""Host test of the DNN tower's route table: which entry points of `ops` a layer of layers.DNN.forward and of
pro.SFGDecoder.hidden_native calls, in which order and with which route arguments, for every configuration.  The predicates
and entry points of `ops`, `dist.current`, the dropout and the stock batch-norm modules are replaced by recorders that return
a tensor of the right shape, so the tables below are the whole contract and no kernel runs.  Every recorder that takes the
running activation also checks that it got the previous stage's result."""
import itertools

import pytest
import torch
import torch.nn as nn

from xdfm_amd import dist as xdist
from xdfm_amd import layers, ops, pro

DP = object()          # the row-parallel context the patched `bn_sync_native` accepts
ANY = "any"            # dp: the row runs under None and under DP (its route must not consult the context at all)


class Recorder:
    """Calls per layer, as strings.  A call that names a layer's weight, batch norm or slope sets the running layer; the
    others (the dropout module, the seed draw, dist.current) belong to the layer that ran last."""

    def __init__(self, keyed):
        self.keyed = keyed                 # tensors / modules that identify a layer, one tuple per layer
        self.calls, self.layer, self.last = {}, None, None
        self.seeds, self.seeds_used = [], []

    def at(self, key):
        self.layer = next(i for i, ks in enumerate(self.keyed) if any(key is k for k in ks))

    def note(self, text):
        self.calls.setdefault(self.layer, []).append(text)

    def takes(self, x):
        assert self.last is None or x is self.last, "a stage did not get the previous stage's result"

    def gives(self, x, cols=None):
        self.last = x.new_zeros(x.shape[0], x.shape[1] if cols is None else cols)
        return self.last


class StandIn(nn.Module):
    """Recorder in the place of an nn.BatchNorm1d."""

    def __init__(self, rec, name):
        super().__init__()
        self.rec, self.name = rec, name

    def forward(self, x):
        self.rec.takes(x)
        self.rec.note(self.name)
        return self.rec.gives(x)


class DropoutStandIn(nn.Dropout):
    """Recorder in the place of an nn.Dropout (and one itself: hidden_native looks for the type); keeps `p` and `training`."""

    def __init__(self, rec, p):
        super().__init__(p)
        self.rec, self.name = rec, "dropout"

    forward = StandIn.forward


def _answer(rec, preds, name):
    v = preds.get(name)
    assert v is not None, "predicate %r is consulted on a route that must not reach it" % name
    return v[rec.layer] if isinstance(v, tuple) else v


def patch_ops(monkeypatch, rec, preds, dp):
    def predicate(name, text, key):
        def fn(*args):
            rec.at(args[key])
            rec.note(text(*args))
            return _answer(rec, preds, name) and (name != "sync" or args[2] is DP)
        return fn

    def stage(text, key, cols=None):
        def fn(x, *args):
            rec.takes(x)
            if key is not None:
                rec.at(args[key])
            rec.note(text(*args))
            return rec.gives(x, cols(*args) if cols else None)
        return fn

    def draw_dropout_seed(device):
        rec.note("draw_dropout_seed")
        rec.seeds.append(torch.zeros(1, dtype=torch.int64))
        return rec.seeds[-1]

    def dense_relu_dropout(x, W, b, p, seed, layer):
        rec.seeds_used.append(seed)
        return drop_stage(x, W, b, p, seed, layer)

    def current():
        rec.note("current")
        return dp

    real_dense_prelu = ops.dense_prelu

    def dense_prelu(x, W, b, alpha):           # recorded, then the real one over the patched predicate and entry points
        rec.takes(x)
        rec.at(W)
        rec.note("dense_prelu")
        return real_dense_prelu(x, W, b, alpha)

    wide = lambda W, *_: W.shape[0]
    drop_stage = stage(lambda W, b, p, seed, layer: "dense_relu_dropout(p=%g,layer=%d)" % (p, layer), 0, wide)
    for name, fn in {
        "dense_dropout_native": predicate("drop", lambda x, W, b, p: "dense_dropout_native?(p=%g)" % p, 1),
        "bn_native": predicate("bn", lambda z, bn: "bn_native?", 1),
        "bn_sync_native": predicate("sync", lambda z, bn, c: "bn_sync_native?(dp=%s)" % ("DP" if c is DP else c), 1),
        "dense_prelu_native": predicate("prelu", lambda x, W, b, alpha: "dense_prelu_native?", 1),
        "dense": stage(lambda W, b: "dense", 0, wide),
        "dense_relu": stage(lambda W, b: "dense_relu", 0, wide),
        "dense_relu_dropout": dense_relu_dropout,
        "dense_prelu": dense_prelu,
        "_dense_prelu_fused": stage(lambda W, b, alpha: "_dense_prelu_fused", 0, wide),
        "prelu": stage(lambda alpha: "prelu", 0),
        "bn_act": stage(lambda bn, act, training: "bn_act(%s,training=%s)" % (act, training), 0),
        "bn_act_sync": stage(lambda bn, act, training, c: "bn_act_sync(%s,training=%s,dp=%s)" % (act, training, "DP" if c is DP else c), 0),
        "draw_dropout_seed": draw_dropout_seed,
    }.items():
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(xdist, "current", current)
    monkeypatch.setattr(torch, "relu", stage(lambda: "torch.relu", None))
    monkeypatch.setattr(torch, "sigmoid", stage(lambda: "torch.sigmoid", None))


def expected(seq, n_layers, **subst):
    """The table's entry per layer: one list for every layer (the seed is drawn by the first only) or one list each."""
    per_layer = seq if isinstance(seq, tuple) else tuple(
        [c for c in seq if i == 0 or c != "draw_dropout_seed"] for i in range(n_layers))
    return {i: [c.format(i=i, **subst) for c in calls] for i, calls in enumerate(per_layer)}


def check_seeds(rec, module, seq):
    fused = sum("dense_relu_dropout" in c for calls in (seq if isinstance(seq, tuple) else (seq, seq)) for c in calls)
    assert len(rec.seeds) == (1 if fused else 0)                     # one draw per call of the tower
    assert len(rec.seeds_used) == fused and all(s is rec.seeds[0] for s in rec.seeds_used)
    assert module.last_drop_seed is (rec.seeds[0] if fused else None)


# (activation, use_bn, training (None: both), dp, predicates (absent: must not be consulted), calls of a layer).
# {p}: the dropout rate, {t}: the training flag, {i}: the layer's index.
FUSED = ["dense_dropout_native?(p={p})", "draw_dropout_seed", "dense_relu_dropout(p={p},layer={i})"]
UNFUSED = ["dense_dropout_native?(p={p})", "dense_relu", "dropout"]
DNN_ROUTES = [
    # ---- no batch norm: dist.current is never asked
    ("relu", False, False, ANY, {}, ["dense_relu", "dropout"]),
    ("relu", False, True, ANY, {"drop": True}, FUSED),
    ("relu", False, True, ANY, {"drop": False}, UNFUSED),
    ("relu", False, True, ANY, {"drop": (False, True)}, (UNFUSED, FUSED)),
    ("relu", False, True, ANY, {"drop": (True, False)}, (FUSED, UNFUSED)),
    ("linear", False, None, ANY, {}, ["dense", "dropout"]),
    ("sigmoid", False, None, ANY, {}, ["dense", "torch.sigmoid", "dropout"]),
    ("prelu", False, None, ANY, {"prelu": True}, ["dense_prelu", "dense_prelu_native?", "_dense_prelu_fused", "dropout"]),
    ("prelu", False, None, ANY, {"prelu": False}, ["dense_prelu", "dense_prelu_native?", "dense", "prelu", "dropout"]),
    # ---- batch norm, one process
    ("relu", True, None, None, {"bn": True}, ["dense", "current", "bn_native?", "bn_act(relu,training={t})", "dropout"]),
    ("linear", True, None, None, {"bn": True}, ["dense", "current", "bn_native?", "bn_act(linear,training={t})", "dropout"]),
    ("sigmoid", True, None, None, {"bn": True}, ["dense", "current", "bn_native?", "bn_act(sigmoid,training={t})", "dropout"]),
    ("prelu", True, None, None, {"bn": True}, ["dense", "current", "bn_native?", "bn_act(linear,training={t})", "prelu", "dropout"]),
    ("relu", True, None, None, {"bn": False, "sync": False},
     ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "torch.relu", "dropout"]),
    ("relu", True, None, None, {"bn": False, "sync": True},
     ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "torch.relu", "dropout"]),
    ("linear", True, None, None, {"bn": False, "sync": False},
     ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "dropout"]),
    ("linear", True, None, None, {"bn": False, "sync": True},
     ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "dropout"]),
    ("sigmoid", True, None, None, {"bn": False, "sync": False},
     ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "torch.sigmoid", "dropout"]),
    ("sigmoid", True, None, None, {"bn": False, "sync": True},
     ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "torch.sigmoid", "dropout"]),
    ("prelu", True, None, None, {"bn": False, "sync": False},
     ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "prelu", "dropout"]),
    ("prelu", True, None, None, {"bn": False, "sync": True},
     ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "prelu", "dropout"]),
    ("relu", True, None, None, {"bn": (True, False), "sync": False},
     (["dense", "current", "bn_native?", "bn_act(relu,training={t})", "dropout"],
      ["dense", "current", "bn_native?", "bn_sync_native?(dp=None)", "bn", "torch.relu", "dropout"])),
    # ---- batch norm under a row-parallel context: bn_native is not asked
    ("relu", True, None, DP, {"sync": True},
     ["dense", "current", "bn_sync_native?(dp=DP)", "bn_act_sync(relu,training={t},dp=DP)", "dropout"]),
    ("linear", True, None, DP, {"sync": True},
     ["dense", "current", "bn_sync_native?(dp=DP)", "bn_act_sync(linear,training={t},dp=DP)", "dropout"]),
    ("sigmoid", True, None, DP, {"sync": True},
     ["dense", "current", "bn_sync_native?(dp=DP)", "bn_act_sync(sigmoid,training={t},dp=DP)", "dropout"]),
    ("prelu", True, None, DP, {"sync": True},
     ["dense", "current", "bn_sync_native?(dp=DP)", "bn_act_sync(linear,training={t},dp=DP)", "prelu", "dropout"]),
    ("relu", True, None, DP, {"sync": False}, ["dense", "current", "bn_sync_native?(dp=DP)", "bn", "torch.relu", "dropout"]),
    ("linear", True, None, DP, {"sync": False}, ["dense", "current", "bn_sync_native?(dp=DP)", "bn", "dropout"]),
    ("sigmoid", True, None, DP, {"sync": False}, ["dense", "current", "bn_sync_native?(dp=DP)", "bn", "torch.sigmoid", "dropout"]),
    ("prelu", True, None, DP, {"sync": False}, ["dense", "current", "bn_sync_native?(dp=DP)", "bn", "prelu", "dropout"]),
    ("relu", True, None, DP, {"sync": (False, True)},
     (["dense", "current", "bn_sync_native?(dp=DP)", "bn", "torch.relu", "dropout"],
      ["dense", "current", "bn_sync_native?(dp=DP)", "bn_act_sync(relu,training={t},dp=DP)", "dropout"])),
]


def _dnn_cells():
    for act, use_bn, training, dp, preds, seq in DNN_ROUTES:
        for t, c, rate in itertools.product((False, True) if training is None else (training,),
                                            (None, DP) if dp is ANY else (dp,), (0, 0.5)):
            name = "%s-bn%d-train%d-p%g-%s-%s" % (act, use_bn, t, rate, "dp" if c is DP else "nodp",
                                                  ",".join("%s=%s" % kv for kv in sorted(preds.items())) or "nopred")
            yield pytest.param(act, use_bn, t, c, rate, preds, seq, id=name)


def test_the_table_covers_every_configuration():
    seen = {(act, use_bn, t, c is DP) for act, use_bn, training, dp, _, _ in DNN_ROUTES
            for t in ((False, True) if training is None else (training,)) for c in ((None, DP) if dp is ANY else (dp,))}
    assert seen == set(itertools.product(("relu", "linear", "sigmoid", "prelu"), (False, True), (False, True), (False, True)))


@pytest.mark.parametrize("act,use_bn,training,dp,rate,preds,seq", _dnn_cells())
def test_dnn_forward_routes(monkeypatch, act, use_bn, training, dp, rate, preds, seq):
    dnn = layers.DNN(6, (8, 4), activation=act, dropout_rate=rate, use_bn=use_bn)
    dnn.train(training)
    keyed = [(lin.weight,) for lin in dnn.linears]
    if act == "prelu":
        keyed = [k + (a.weight,) for k, a in zip(keyed, dnn.activation_layers)]
    rec = Recorder(keyed)
    dnn.dropout = DropoutStandIn(rec, rate)
    if use_bn:
        for i in range(2):
            dnn.bn[i] = StandIn(rec, "bn")
        rec.keyed = [k + (dnn.bn[i],) for i, k in enumerate(keyed)]
    dnn.train(training)
    patch_ops(monkeypatch, rec, preds, dp)
    out = dnn(torch.zeros(3, 6))
    assert out is rec.last and out.shape == (3, 4)
    assert rec.calls == expected(seq, 2, p="%g" % rate, t=training)
    check_seeds(rec, dnn, seq)


# SFGDecoder.hidden_native: (label attention on, labels given, modules in training, predicate, calls of a layer)
SFG_ROUTES = [
    (False, True, True, {"drop": True}, ["dense_dropout_native?(p=0.1)", "draw_dropout_seed", "dense_relu_dropout(p=0.1,layer={i})"]),
    (False, True, True, {"drop": False}, ["dense_dropout_native?(p=0.1)", "dense_relu", "dropout"]),
    (False, True, True, {"drop": (False, True)},
     (["dense_dropout_native?(p=0.1)", "dense_relu", "dropout"],
      ["dense_dropout_native?(p=0.1)", "draw_dropout_seed", "dense_relu_dropout(p=0.1,layer={i})"])),
    (False, True, True, {"drop": (True, False)},
     (["dense_dropout_native?(p=0.1)", "draw_dropout_seed", "dense_relu_dropout(p=0.1,layer={i})"],
      ["dense_dropout_native?(p=0.1)", "dense_relu", "dropout"])),
    (False, True, False, {}, ["dense_relu", "dropout"]),
    (True, True, True, {"drop": True}, ["dense_dropout_native?(p=0.1)", "draw_dropout_seed", "dense_relu_dropout(p=0.1,layer={i})"]),
    (True, True, True, {"drop": False}, ["dense_dropout_native?(p=0.1)", "dense_relu", "dropout"]),
    (True, True, False, {}, ["dense_relu", "dropout"]),
    (True, False, True, {"drop": True}, ["dense_dropout_native?(p=0.1)", "draw_dropout_seed", "dense_relu_dropout(p=0.1,layer={i})"]),
    (True, False, False, {}, ["dense_relu", "dropout"]),
]


@pytest.mark.parametrize("attention,labels,training,preds,seq", SFG_ROUTES)
def test_sfg_decoder_hidden_native_routes(monkeypatch, attention, labels, training, preds, seq):
    dec = pro.SFGDecoder(4, {"a": 5, "b": 7}, ["d"], hidden_units=(8, 4), dropout_rate=0.1, use_label_aware_attention=attention)
    mods = dec.shared_layers
    assert [type(m) for m in mods] == [nn.Linear, nn.ReLU, nn.Dropout] * 2
    rec = Recorder([(mods[0].weight,), (mods[3].weight,)])
    for j in (2, 5):
        mods[j] = DropoutStandIn(rec, 0.1)
    dec.train(training)
    patch_ops(monkeypatch, rec, preds, None)
    if attention:
        def forward_native(x, l):
            rec.note("label_attention.forward_native")
            return torch.ones_like(x)
        monkeypatch.setattr(dec.label_attention, "forward_native", forward_native)
    out = dec.hidden_native(torch.zeros(3, 9), torch.ones(3, 1) if labels else None)
    assert out is rec.last and out.shape == (3, 4)
    want = expected(seq, 2)              # {i} is the triple's index: module j of shared_layers is layer j // 3
    if attention and labels:
        want[None] = ["label_attention.forward_native"]
    assert rec.calls == want
    check_seeds(rec, dec, seq)
