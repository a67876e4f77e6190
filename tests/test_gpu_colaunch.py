"""GPU tests (-m gpu) of the shared launches behind option "colaunch" (include/xdfm.h): bodies that do not depend on each
other go out as workgroup ranges of ONE launch.  Which launch carries a body changes nothing in its arithmetic, its sums or
its partial layouts, so every comparison is torch.equal against the same calls with the option at 0, which issue the
separate launches.

Bit 2, the unpack riders (csrc/rider.h, csrc/cin_x3_bww.hip, csrc/embed.hip: inside a rider scope -- ops.rider_begin /
ops.rider_flush, which the model's own step opens around its backward -- the ordered sum of a level's dW slabs is not
launched by its dW call but rides, as extra workgroups, on the next level's x3_bwd_prep_kernel, level 0's on the embedding
scatter; what nobody carried leaves in the flush): ops.cin_stack forward + backward inside a scope (no scatter there: level
0's sum takes the flush) and the model's step (the scatter carries it) at colaunch 4 / 5 against 0, every gradient bit for bit.

Bit 1, the pack riders (csrc/cin_x3_pack.h: the CIN weight packs announced before the embedding gather -- xdfm_cin_pack_defer
behind ops.cin_announce_pack -- leave with deferred Adam's catch-up (the partial |W| maxima) and with the gather (the packs);
what no launch carried leaves in xdfm_cin_pack_flush): the packed buffers with their headers, byte for byte, against the
launches of xdfm_cin_pack_all, with the catch-up present, absent, and with no host at all.

Bit 0, the optimizer pair (csrc/adam.hip: adam_step_rows_kernel behind xdfm_colaunch_adam_step): the workgroups of
xdfm_adam_step_deferred's step over the dense tensors and the small tables (mark scan), followed by those of
xdfm_adam_apply_rows over the big tables' rows.  At the C ABI: two banks with the same state go through the same five
steps, one at colaunch = 1, one at 0.  Ids are Zipf-like (heavy duplication), with V + 5 and -1 among them (clamped, as
the gather clamps); the upper half of every vocabulary is hit at steps 1 and 5 only, so its rows go untouched for three
steps and the step that hits them again replays what they miss (no catch-up is called in between).  The whole step on a
model: seven train_on_batch steps, eager and with the later ones replayed from the captured graph, one predict in between."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu

B = 257
STEPS = 5
DENSE_N = 4099
L2_DENSE = 1e-3
HP = "H0"


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def _colaunch(value):
    from xdfm_amd import _lib
    before = _lib.get_option("colaunch")
    _lib.set_option("colaunch", value)
    try:
        yield
    finally:
        _lib.set_option("colaunch", before)


def _batch(vocab, cols, ldx, step):
    """X [B, ldx] and the ids the kernels make of it.  Steps 2 .. 4 stay in the lower half of every vocabulary."""
    rng = np.random.RandomState(9000 + step)
    X = rng.rand(B, ldx).astype(np.float32)
    ids = []
    for f, V in enumerate(vocab):
        top = V if step in (1, 5) else max(V // 2, 1)
        i = np.minimum((top * rng.rand(B) ** 3).astype(np.int64), top - 1)
        i[0], i[1] = 0, top - 1
        raw = i.astype(np.float32)
        raw[5], i[5] = V + 5, V - 1                 # out of range on both sides: clamped
        raw[6], i[6] = -1, 0
        X[:, cols[f]] = raw + (0.25 if f == 1 else 0.0)     # a fraction is truncated
        ids.append(i)
    return X, ids


def _step_rows(bank, others, l2, marked, flags, clk, step, X, cols, vocab, m, D, emb, lin):
    """xdfm_colaunch_adam_step: the step over the tensors `others` of `bank`, the rows update over emb / lin."""
    from xdfm_amd import _lib
    lib = _lib.load()
    lr, _ = R.lr_of(HP, step)
    _, b1, b2, eps = R.HYPER[HP]
    arr = bank.descriptors(others, l2, marked, flags)
    bank.ws = torch.zeros(lib.xdfm_adam_step_ws_elems(len(others)), dtype=torch.float32, device=bank.dev)
    _lib.check(lib.xdfm_colaunch_adam_step(
        ctypes.cast(arr, ctypes.c_void_p), len(others), ctypes.byref(clk.struct), lr, None, b1, b2, eps,
        ctypes.c_void_p(bank.ws.data_ptr()), ctypes.c_void_p(bank.l2_value.data_ptr()),
        ctypes.c_void_p(X.data_ptr()), X.stride(0), X.shape[0], ctypes.c_void_p(cols.data_ptr()), ctypes.c_void_p(vocab.data_ptr()),
        m, D, ctypes.byref(emb.struct), ctypes.byref(lin.struct) if lin is not None else None,
        ctypes.c_void_p(clk.cell.data_ptr()), R._stream()), "colaunch_adam_step")


def _run_pair(D, vocab_sizes, with_lin, n_dense):
    """Five steps on two banks (colaunch 1 / 0).  The last field's tables go by rows, the others' `param` is NULL in
    xdfm_adam_rows: they are the step's, by their marks.  n_dense dense tensors ride along (more than 64 tensors in all
    make the step two launches; the rows ride behind the first)."""
    from xdfm_amd import _lib
    dev = _dev()
    m = len(vocab_sizes)
    ldx, cols_h = m + 3, [(2 * f + 1) % (m + 3) for f in range(m)]
    assert len(set(cols_h)) == m
    sizes = [V * D for V in vocab_sizes] + (list(vocab_sizes) if with_lin else []) + [DENSE_N] + [37] * (n_dense - 1)
    l2_emb = [1e-3 * (1 + f) for f in range(m)]
    l2_lin = [2e-3 * (1 + f) for f in range(m)]
    l2 = l2_emb + (l2_lin if with_lin else []) + [L2_DENSE] * n_dense
    T = len(sizes)
    emb_idx, lin_idx = list(range(m)), (list(range(m, 2 * m)) if with_lin else [])
    tables = emb_idx + lin_idx
    dense_idx = list(range(len(tables), T))
    width = [D] * m + [1] * len(lin_idx)
    skip = tuple(range(m - 1))                      # every field but the last: by the scan
    scan = [t for k, t in enumerate(tables) if (k % m) in skip]
    others = scan + dense_idx
    state = R.make_state(sizes, seed=31)
    banks = {1: R.Bank(state, dev), 0: R.Bank(state, dev)}
    clks = {k: R.Clock(dev, cap=16) for k in banks}
    rows = {k: (R.Rows(b, emb_idx, l2_emb, skip=skip), R.Rows(b, lin_idx, l2_lin, skip=skip) if with_lin else None)
            for k, b in banks.items()}
    cols = torch.tensor(cols_h, dtype=torch.int32, device=dev)
    vocab = torch.tensor(vocab_sizes, dtype=torch.int32, device=dev)
    for s in range(1, STEPS + 1):
        Xn, ids = _batch(vocab_sizes, cols_h, ldx, s)
        X = torch.from_numpy(Xn).to(dev)
        masks = []
        for k, t in enumerate(tables):
            w, n4 = width[k], sizes[t] // 4
            mk = np.zeros(n4 + 1, dtype=bool)
            for i in np.unique(ids[k % m]):
                mk[i * w // 4:(i * w + w - 1) // 4 + 1] = True
            masks.append(mk[:n4])
        masks += [np.ones(sizes[t] // 4, dtype=bool) for t in dense_idx]
        flat, marks, _, offs = R.sparse_grads(sizes, None, s, seed=17, chunks=masks)
        for t in dense_idx:                         # the dense tensors' gradients are read in full, without marks
            o = offs[t] // 4
            marks[o:o + sizes[t] // 4 + 1] = 0
        for mode, b in banks.items():
            b.set_grads(flat, marks)
            b.steps += 1.0
            with _colaunch(mode):
                _step_rows(b, others, [l2[t] for t in others], [True] * len(scan) + [False] * len(dense_idx),
                           [R.DEFERRED] * len(scan) + [0] * len(dense_idx), clks[mode], s, X, cols, vocab, m, D, *rows[mode])
                assert _lib.get_option("last_colaunch") == mode
        torch.cuda.synchronize()
        x, y = banks[1], banks[0]
        what = "step %d" % s
        for t in range(T):
            for name, xa, ya in (("p", x.p, y.p), ("m", x.m, y.m), ("v", x.v, y.v)):
                assert torch.equal(xa[t].view(torch.int32), ya[t].view(torch.int32)), "%s: %s of tensor %d" % (what, name, t)
            assert torch.equal(x.last[t], y.last[t]), "%s: `last` bytes of tensor %d" % (what, t)
        assert torch.equal(x.l2_value.view(torch.int32), y.l2_value.view(torch.int32)), "%s: l2_value" % what
        assert torch.equal(x.ws, y.ws), "%s: the step's L2 partials" % what
        assert clks[1].read() == clks[0].read() == [s, 0]
        assert torch.equal(clks[1].consts, clks[0].consts)
        for mode, b in banks.items():
            for t in dense_idx:
                b.flat[b.goff[t]:b.goff[t] + sizes[t]].zero_()
            assert not bool(b.gbuf.any()) and not bool(b.marks.any()), "%s: gradient / marks not re-zeroed (colaunch %d)" % (what, mode)
            assert int(clks[mode].cell.item()) == 0, "%s: the rows cell (colaunch %d)" % (what, mode)
        assert int(clks[1].backlog.item()) == int(clks[0].backlog.item())
    # the case did what it is for: rows of the big table were behind when step 5 hit them
    assert int(banks[1].last[emb_idx[-1]].max()) == STEPS and bool((banks[1].last[emb_idx[-1]] == 1).any())


@pytest.mark.parametrize("with_lin", [True, False], ids=["lin", "nolin"])
def test_pair_by_row(with_lin):
    """D = 16: the last table is 70000 x 16 >= 2^20 elements and goes by rows (adam_apply_by_row's body), the others by the scan."""
    from xdfm_amd import _lib
    _run_pair(16, [3, 24, 1000, 70000], with_lin, 1)
    assert _lib.get_option("last_adam_rows") == 1


@pytest.mark.parametrize("with_lin", [True, False], ids=["lin", "nolin"])
def test_pair_by_chunk_with_live_tails(with_lin):
    """D = 10: rows straddle chunks, so the by-chunk body runs; 110001 x 10 % 4 = 2 and 110001 % 4 = 1: the tail elements
    that no chunk covers are live in the rows update."""
    from xdfm_amd import _lib
    _run_pair(10, [5, 110001], with_lin, 1)
    assert _lib.get_option("last_adam_rows") == 0


def test_pair_behind_the_first_of_two_step_launches():
    """70 tensors in the step: two launches, the rows update rides behind the first."""
    _run_pair(16, [24, 70000], True, 67)


@contextlib.contextmanager
def _cin_math(value):
    from xdfm_amd import _lib
    before = _lib.get_option("cin_math")
    _lib.set_option("cin_math", value)
    try:
        yield
    finally:
        _lib.set_option("cin_math", before)


def _cin_grads(dev, m, D, Bn, layers, mode):
    """ops.cin_stack forward + backward (ReLU, split halves, sum pooling) at colaunch `mode` -> (out, dx, [dW], [db], probes)."""
    from xdfm_amd import _lib, ops
    g = torch.Generator().manual_seed(1000 * m + layers[0])
    x = torch.randn((Bn, m, D), generator=g)
    levels, fm = ops.cin_geometry(m, layers, True)
    W = [torch.randn((H, Hp * m, 1), generator=g) * 0.1 for (H, Hp, *_r) in levels]
    Bs = [torch.randn((H,), generator=g) * 0.1 for (H, *_r) in levels]
    gout = torch.randn((Bn, fm), generator=g).to(dev)
    xg = x.to(dev).requires_grad_(True)
    Wg = [w.to(dev).requires_grad_(True) for w in W]
    Bg = [b.to(dev).requires_grad_(True) for b in Bs]
    with _colaunch(mode):
        _lib.set_option("last_riders", -1)
        out = ops.cin_stack(ops.to_fm_layout(xg), Bn, D, layers, True, "relu", "sum", Wg, Bg)
        ops.rider_begin()
        assert _lib.load().xdfm_rider_active() == (1 if mode & 4 else 0)
        (out * gout).sum().backward()
        ops.rider_flush()
        torch.cuda.synchronize()
        probes = (_lib.get_option("last_bww_kernel"), _lib.get_option("last_riders"), _lib.load().xdfm_rider_pending(),
                  bool(_lib.get_option("last_sym") & 4))
    return out.detach(), xg.grad, [w.grad for w in Wg], [b.grad for b in Bg], probes


# (m, D, B, CIN layers, whether the f16x3 / bf16 dW kernel -- and with it the riders -- runs: it needs more than 64 rows)
RIDER_CASES = [(8, 4, 96, (64, 64), False), (8, 4, 96, (96, 72), True), (8, 4, 96, (96, 80, 72), True),
               (26, 4, 64, (64,), False), (26, 4, 64, (96, 72), True)]


@pytest.mark.parametrize("math", [1, 2], ids=["f16x3", "bf16"])
@pytest.mark.parametrize("m,D,Bn,layers,rides", RIDER_CASES, ids=["m8-64", "m8-96", "m8-three", "m26-64", "m26-96"])
def test_unpack_riders_leave_dw_bit_identical(m, D, Bn, layers, rides, math):
    """dW of every level (and everything else the backward returns) with the slab sums riding on the next pre-pass against
    the separate launches.  m = 26: level 0 takes the folded dW kernel, whose sum -- the last one -- leaves in the flush."""
    dev = _dev()
    with _cin_math(math):
        out1, dx1, dW1, db1, probes1 = _cin_grads(dev, m, D, Bn, layers, 4)
        out0, dx0, dW0, db0, probes0 = _cin_grads(dev, m, D, Bn, layers, 0)
    assert torch.equal(out1, out0) and torch.equal(dx1, dx0)
    for l, (a, b) in enumerate(zip(dW1, dW0)):
        assert torch.equal(a, b), "dW of level %d" % l
    for l, (a, b) in enumerate(zip(db1, db0)):
        assert torch.equal(a, b), "dbias of level %d" % l
    assert all(bool(w.abs().sum() > 0) for w in dW1)
    assert probes1[2] == 0 and probes0[2] == 0, "a rider job was left pending"
    if rides:
        assert probes1[0] == math and probes0[0] == math, "the f16x3 / bf16 dW kernel did not run"
        # the last pre-pass of the backward is level 0's: it carried level 1's sum (one level: nothing to carry)
        assert probes1[1] == (1 if len(layers) > 1 else 0) and probes0[1] == 0, (probes1, probes0)
        assert probes1[3] == (m == 26), "folded level 0"


def test_rider_scope_errors_and_flush_without_jobs():
    from xdfm_amd import _lib
    _dev()
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.xdfm_rider_flush(st) == 0 and lib.xdfm_rider_pending() == 0          # no scope: nothing happens
    with _colaunch(4):
        assert lib.xdfm_rider_begin() == 0 and lib.xdfm_rider_active() == 1
        assert lib.xdfm_rider_begin() != 0 and "open already" in lib.xdfm_last_error().decode()
        assert lib.xdfm_rider_flush(st) == 0 and lib.xdfm_rider_active() == 0
        assert lib.xdfm_rider_begin() == 0 and lib.xdfm_rider_flush(st) == 0        # the flush closed the scope
    with _colaunch(0):
        assert lib.xdfm_rider_begin() == 0 and lib.xdfm_rider_active() == 0         # bit clear: a scope that records nothing
        assert lib.xdfm_rider_flush(st) == 0
    torch.cuda.synchronize()


VOCAB = [5000, 31, 20003, 3, 9, 402, 50, 7]         # m = 8; with the floor lowered the 5000- and 20003-row tables go by rows
ND, EMB_D, MODEL_B = 3, 4, 96


def _model(dev, use_graph, frozen=False, cin=(96, 72)):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    cols = [SparseFeat("C%d" % (i + 1), v, EMB_D) for i, v in enumerate(VOCAB)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(ND)]
    torch.manual_seed(4)
    model = xDeepFM(cols, cols, dnn_hidden_units=(32, 16), cin_layer_size=cin, l2_reg_dnn=1e-5, device=dev)
    with torch.no_grad():                           # weights large enough for the L2 pull to move bits every step
        for k, p in model.named_parameters():
            if "embedding_dict" in k:
                p.mul_(2000.0)
    if frozen:                                      # no dW, so no slab sums: the rider scope opens and closes empty
        names = [k for k, p in model.named_parameters() if k.startswith("cin.") and "weight" in k]
        assert len(names) == 2
        for k, p in model.named_parameters():
            if k in names:
                p.requires_grad_(False)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.optim.deferred = True
    model.train()
    step = graphstep.GraphedStep(model)
    step.disabled = not use_graph
    model.__dict__["_graphed_step"] = step
    return model, step


def _train(dev, mode, use_graph, frozen=False):
    """Seven train_on_batch steps (with the graph: eager ones, the capture, at least two replays), a predict after the second."""
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import _lib
    with _colaunch(mode):
        model, step = _model(dev, use_graph, frozen)
        seen = []
        for s in range(7):
            X, y = orc.synthetic_batch(MODEL_B, VOCAB, ND, seed=700 + s)
            out = model.train_on_batch(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
            seen.append([t.detach().clone() for t in out])          # y_pred, data loss, total loss
            if s == 1:
                seen.append([torch.from_numpy(model.predict([X[:, j] for j in range(X.shape[1])], batch_size=MODEL_B))])
                model.train()
        torch.cuda.synchronize()
        assert model.optim.path_counts["rows"] >= 2 and _lib.get_option("last_colaunch") == (mode & 1)
        assert _lib.get_option("last_riders") == (1 if mode & 4 and not frozen else 0) and _lib.load().xdfm_rider_pending() == 0
        assert _lib.get_option("last_pack_riders") == (3 if mode & 2 else 0) and _lib.load().xdfm_cin_pack_pending() == 0
        assert (step.replays >= 2 and not step.disabled) if use_graph else step.replays == 0
        nodes = max([e.nodes for e in step.entries.values()] + [0])
        moments = [(model.optim.state[p]["exp_avg"].clone(), model.optim.state[p]["exp_avg_sq"].clone())
                   for p in model.optim.param_groups[0]["params"] if "exp_avg" in model.optim.state[p]]      # (frozen: no state)
        return seen, {k: v.clone() for k, v in model.state_dict().items()}, moments, nodes


def _packs(dev, math, cin, route, monkeypatch):
    """The packs of a model's CIN weights by `route`, and by xdfm_cin_pack_all's own launches (colaunch 0) for the same
    weights -> ((forward packs, dX packs), the same of the reference, probe "last_pack_riders"), None where the levels are not
    packed at once.  "catchup": a model two train steps old, so the gather is preceded by deferred Adam's catch-up; "gather":
    a fresh model, no catch-up; "flush": no host launch at all."""
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import _lib, ops
    lib = _lib.load()
    _lib.set_option("cin_math", math)
    try:
        model, _ = _model(dev, False, cin=cin)
        X, y = orc.synthetic_batch(MODEL_B, VOCAB, ND, seed=800)
        x = torch.from_numpy(X).to(dev)
        if route == "catchup":
            for _ in range(2):
                model.train_on_batch(x, torch.from_numpy(y).to(dev))
        got = []
        for mode in (2, 0):
            with _colaunch(mode):
                # zero-filled buffers for this comparison: a pack's header has words no kernel writes
                monkeypatch.setattr(torch, "empty", torch.zeros)
                try:
                    model.cin.announce_pack()
                finally:
                    monkeypatch.undo()
                ann = ops._PACK_ANNOUNCED
                if ann is None:
                    return None                     # no level set that packs at once in this arithmetic: nothing to ride
                if mode == 2:
                    if route != "flush":
                        with torch.no_grad():
                            model.fused_inputs(x)
                    assert lib.xdfm_cin_pack_pending() == (0 if route != "flush" else (1 if math == 1 else 2))
                    probe = _lib.get_option("last_pack_riders")
                ops.cin_pack_drop()
                assert lib.xdfm_cin_pack_pending() == 0
                torch.cuda.synchronize()
                got.append(([w.view(torch.int32).clone() for w in ann[1]], [w.view(torch.int32).clone() for w in ann[2]]))
        return got[0], got[1], probe
    finally:
        _lib.set_option("cin_math", 1)


@pytest.mark.parametrize("cin", [(64, 64), (96, 72)], ids=["64-64", "96-72"])
@pytest.mark.parametrize("math", [1, 2], ids=["f16x3", "bf16"])
def test_pack_riders_leave_the_packs_byte_identical(math, cin, monkeypatch):
    dev = _dev()
    # the weights' maxima are a separate pass in f16x3 only
    want = {"catchup": 3 if math == 1 else 2, "gather": 2, "flush": 0}
    for route in ("catchup", "gather", "flush"):
        res = _packs(dev, math, cin, route, monkeypatch)
        if res is None:
            assert math == 2 and cin == (64, 64)    # bf16 has no kernels for 64-row levels: nothing is packed at once
            return
        (fwd, bwd), (fwd0, bwd0), probe = res
        assert probe == want[route], (route, probe)
        for l, (a, b) in enumerate(zip(fwd, fwd0)):
            assert torch.equal(a, b), "%s: forward pack of level %d" % (route, l)
        for l, (a, b) in enumerate(zip(bwd, bwd0)):
            assert torch.equal(a, b), "%s: dX pack of level %d" % (route, l)
        assert len(fwd) == len(cin) and all(bool(a.any()) for a in fwd + bwd)


@pytest.mark.parametrize("use_graph,frozen", [(False, False), (True, False), (False, True)], ids=["eager", "graph", "eager-frozen-cin"])
def test_whole_step_is_bit_identical(use_graph, frozen, monkeypatch):
    """The model's own step: parameters, moments, y_pred and both losses of every step, and the predict in between."""
    monkeypatch.setenv("XDFM_ADAM_ROWS_MIN_NUMEL", "15000")
    if frozen:
        # frozen CIN weights: no dW workspace, so the backward takes the pre-pass that writes dOut (ops.CINStack.backward reads
        # the switch at the call); no slab sum is recorded, the scope opens and closes empty
        monkeypatch.setenv("XDFM_CIN_NODOUT", "0")
    dev = _dev()
    seen1, sd1, mo1, nodes1 = _train(dev, 7, use_graph, frozen)
    seen0, sd0, mo0, nodes0 = _train(dev, 0, use_graph, frozen)
    for k, (a, b) in enumerate(zip(seen1, seen0)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), "output %d" % k
    for k in sd1:
        assert torch.equal(sd1[k], sd0[k]), k
    for (a, b), (c, d) in zip(mo1, mo0):
        assert torch.equal(a, c) and torch.equal(b, d)
    if use_graph:
        # one node less for the optimizer pair, one each for the slab sums of level 1 (on level 0's pre-pass) and 0 (on the
        # scatter), one each for the |W| maxima (on the catch-up) and the packs (on the gather)
        assert nodes1 == nodes0 - 5, "graph nodes %d against %d" % (nodes1, nodes0)
