"""GPU tests (-m gpu) of the finish batch (include/xdfm.h, xdfm_finish_batch_begin / _run / xdfm_finish).

C ABI: every family's finish over partials of the test's own, recorded in a batch against launched on its own -- bit for bit,
the batch's outputs pre-filled with NaN (the CIN dbias of a separate launch accumulates, so that one starts from zeros; the rows
finish adds to l2_value on both routes, so that one starts from a number).  Then the batch itself: every kind at once, more
jobs than one table holds, the finishes that feed each other (L2 value -> rows cell -> total loss), an empty _run and the
refused calls.  Last, whole train steps of a small xDeepFM with the option "finish_batch" at 1 and at 0: same bits, fewer nodes.

Every test sets the option itself and closes its batch in a `finally`."""
import ctypes
import faulthandler

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
CIN_DBIAS, DENSE_W, COLSUM, HEAD_FWD, HEAD_BWD, ADAM_L2, ADAM_ROWS, ADD = range(8)
TABLE = 16                       # FINISH_MAX_JOBS of csrc/finish_batch.h


@pytest.fixture(autouse=True)
def _step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(autouse=True)
def _option_on():
    from xdfm_amd import _lib
    if not torch.cuda.is_available():
        yield
        return
    before = _lib.get_option("finish_batch")
    _lib.set_option("finish_batch", 1)
    yield
    _lib.load().xdfm_finish_batch_run(_st())           # a test that failed half way leaves no batch open
    _lib.set_option("finish_batch", before)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _finish(kind, part=None, part2=None, out=None, out2=None, out3=None, n0=0, n1=0, i0=0, i1=0):
    from xdfm_amd import _lib
    _lib.check(_lib.load().xdfm_finish(kind, _p(part), _p(part2), _p(out), _p(out2), _p(out3), n0, n1, i0, i1, _st()), "xdfm_finish")


class Case:
    """One finish: `outs(batched)` makes fresh output tensors, `call(outs)` issues the finish."""

    def __init__(self, name, outs, call, data=None):
        self.name, self.outs, self.call, self.data = name, outs, call, data


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _rand(dev, gen, *shape, dtype=torch.float32):
    return (torch.randn(*shape, generator=gen, dtype=torch.float64) * 3.0).to(dtype).to(dev)


def _cin_dbias(dev, gen, gx):
    H = 65                                                       # two 64-thread blocks of the separate launch, one ragged
    part = _rand(dev, gen, H, gx)
    return Case("cin dbias gx=%d" % gx, lambda batched: [_nan(dev, H) if batched else torch.zeros(H, device=dev)],
                lambda o: _finish(CIN_DBIAS, part=part, out=o[0], i0=H, i1=gx))


def _dense(dev, gen, out, k, nsplit, with_db, prelu):
    ws = _rand(dev, gen, nsplit * (out * k + out))
    npart = 300 if prelu else 0                                  # more partials than the block has threads
    da_part = _rand(dev, gen, npart, dtype=torch.float64) if prelu else None

    def outs(batched):
        return [_nan(dev, out, k), _nan(dev, out) if with_db else None, _nan(dev, 1) if prelu else None]
    return Case("dense (%d, %d) nsplit=%d db=%s prelu=%s" % (out, k, nsplit, with_db, prelu), outs,
                lambda o: _finish(DENSE_W, part=ws, part2=da_part, out=o[0], out2=o[1], out3=o[2], n0=out, n1=k, i0=nsplit, i1=npart))


def _colsum(dev, gen, cols):
    part = _rand(dev, gen, 64, cols)
    return Case("colsum cols=%d" % cols, lambda batched: [_nan(dev, cols)], lambda o: _finish(COLSUM, part=part, out=o[0], i0=cols))


def _head_fwd(dev, gen):
    part = _rand(dev, gen, 128)
    return Case("head fwd", lambda batched: [_nan(dev, 1)], lambda o: _finish(HEAD_FWD, part=part, out=o[0]))


def _head_bwd(dev, gen, KT):
    part = _rand(dev, gen, 128, KT)
    return Case("head bwd KT=%d" % KT, lambda batched: [_nan(dev, KT)], lambda o: _finish(HEAD_BWD, part=part, out=o[0], i0=KT))


def _adam_l2(dev, gen, n):
    part = _rand(dev, gen, n).abs()                  # squares' sums are positive: no cancellation, every add rounds
    return Case("adam l2 n=%d" % n, lambda batched: [_nan(dev, 1)], lambda o: _finish(ADAM_L2, part=part, out=o[0], i0=n), data=part)


def _rows(dev, with_value):
    def outs(batched):
        cell = torch.tensor([3 * (1 << 40) + 123456789], dtype=torch.int64, device=dev)
        return [torch.full((1,), 0.7131, device=dev) if with_value else None, cell]
    return Case("rows l2_value=%s" % with_value, outs, lambda o: _finish(ADAM_ROWS, out=o[0], out2=o[1]))


def _families(dev):
    gen = torch.Generator().manual_seed(20)
    cases = [_cin_dbias(dev, gen, 1), _cin_dbias(dev, gen, 3)]
    for out, k in ((5, 7), (20, 15)):
        for nsplit in (1, 3):
            cases += [_dense(dev, gen, out, k, nsplit, True, False), _dense(dev, gen, out, k, nsplit, False, False),
                      _dense(dev, gen, out, k, nsplit, True, True)]
    cases += [_head_fwd(dev, gen), _head_bwd(dev, gen, 1), _head_bwd(dev, gen, 257)]
    cases += [_adam_l2(dev, gen, n) for n in (1, 1024, 1480)]
    cases += [_rows(dev, True), _rows(dev, False), _colsum(dev, gen, 70)]
    return cases


def _separate(case):
    outs = case.outs(False)
    case.call(outs)
    torch.cuda.synchronize()
    return outs


def _same(case, got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), "%s: output %d differs between the batch and the separate launch" % (case.name, k)


def _batch_of(cases):
    from xdfm_amd import _lib
    lib = _lib.load()
    outs = [c.outs(True) for c in cases]
    _lib.check(lib.xdfm_finish_batch_begin(), "begin")
    try:
        assert lib.xdfm_finish_batch_active() == 1
        for c, o in zip(cases, outs):
            c.call(o)
    finally:
        _lib.check(lib.xdfm_finish_batch_run(_st()), "run")
    assert lib.xdfm_finish_batch_active() == 0
    torch.cuda.synchronize()
    return outs


def test_each_family_in_a_batch_equals_its_separate_launch_bit_for_bit():
    dev = _dev()
    for case in _families(dev):
        want = _separate(case)
        got = _batch_of([case])[0]
        _same(case, got, want)
        if case.name.startswith("rows"):
            assert int(got[1]) == 0 and int(want[1]) == 0, "the cell reads 0 afterwards"
            if got[0] is not None:
                assert float(got[0]) != pytest.approx(0.7131), "the cell's value joined l2_value"
        elif case.name.startswith("dense") and "nsplit=1" in case.name:
            assert bool(torch.isnan(got[0]).all()), "one split: dW is the main kernel's, the finish leaves it alone"
        else:
            assert bool(torch.isfinite(got[0]).all()), case.name


def _l2_host(part, threads):
    """fp32, step by step: thread t of `threads` adds the partials t, t + threads, ..., then the tree adds t + threads / 2, ..."""
    acc = np.zeros(threads, dtype=np.float32)
    for k0 in range(0, len(part), threads):
        chunk = part[k0:k0 + threads]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    o = threads // 2
    while o:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o //= 2
    return acc[:1]


def test_l2_finish_keeps_the_order_of_1024_threads():
    """The batch's L2 finish runs in a block of 256 threads and must still add as 1024 threads would.  At 1480 partials the
    data are drawn until the two orders differ on the host, so that the test can tell them apart."""
    dev = _dev()
    for n in (1, 1024, 1480):
        for seed in range(21, 121):
            case = _adam_l2(dev, torch.Generator().manual_seed(seed), n)
            part = case.data.cpu().numpy()
            want = _l2_host(part, 1024)
            if n != 1480 or _l2_host(part, 256)[0] != want[0]:
                break
        else:
            raise AssertionError("no data set in 100 tells a stride of 256 from one of 1024")
        got = _batch_of([case])[0][0].cpu().numpy()
        assert got.view(np.int32)[0] == want.view(np.int32)[0], (n, seed, float(got[0]), float(want[0]))


def test_one_batch_with_every_kind_and_one_longer_than_a_table():
    dev = _dev()
    cases = _families(dev)
    assert len(cases) > TABLE, "more jobs than one table holds: the batch takes a second launch"
    want = [_separate(c) for c in cases]
    got = _batch_of(cases)
    for c, g, w in zip(cases, got, want):
        _same(c, g, w)
    gen = torch.Generator().manual_seed(22)
    many = [_head_bwd(dev, gen, 3) for _ in range(2 * TABLE + 3)]             # three launches, the last one ragged
    want = [_separate(c) for c in many]
    for c, g, w in zip(many, _batch_of(many), want):
        _same(c, g, w)


def test_finishes_that_feed_each_other_share_a_batch():
    """L2 value, then the rows' cell added to it, then total = loss + value: the order of the separate launches."""
    dev = _dev()
    gen = torch.Generator().manual_seed(23)
    l2 = _adam_l2(dev, gen, 1480)
    loss = torch.tensor([123.456], device=dev)

    def chain(batched):
        val, total = _nan(dev, 1), _nan(dev, 1)
        cell = torch.tensor([5 * (1 << 40) + 987654321], dtype=torch.int64, device=dev)
        l2.call([val])
        _finish(ADAM_ROWS, out=val, out2=cell)
        _finish(ADD, part=loss, part2=val, out=total)
        return val, total, cell
    want = chain(False)
    torch.cuda.synchronize()
    from xdfm_amd import _lib
    lib = _lib.load()
    for lone_rows in (False, True):                   # True: no L2 job in the batch, the rows finish stands alone in front of the add
        _lib.check(lib.xdfm_finish_batch_begin(), "begin")
        try:
            if lone_rows:
                val, total = want[0].clone(), _nan(dev, 1)
                cell = torch.tensor([7 * (1 << 40)], dtype=torch.int64, device=dev)
                _finish(ADAM_ROWS, out=val, out2=cell)
                _finish(ADD, part=loss, part2=val, out=total)
                got = (val, total, cell)
            else:
                got = chain(True)
        finally:
            _lib.check(lib.xdfm_finish_batch_run(_st()), "run")
        torch.cuda.synchronize()
        if lone_rows:
            assert float(got[0]) == float(want[0] + torch.tensor(7.0, device=dev)) and int(got[2]) == 0
            assert float(got[1]) == float(loss + got[0])
        else:
            for g, w in zip(got, want):
                assert torch.equal(_bits(g), _bits(w))
            assert float(got[1]) == float(loss + got[0]) and int(got[2]) == 0


def test_empty_run_and_refused_calls():
    from xdfm_amd import _lib
    dev = _dev()
    lib = _lib.load()
    assert lib.xdfm_finish_batch_run(_st()) == 0, "_run without _begin launches nothing"
    assert lib.xdfm_finish_batch_begin() == 0
    try:
        assert lib.xdfm_finish_batch_run(_st()) == 0, "an empty batch"
    finally:
        lib.xdfm_finish_batch_run(_st())
    assert lib.xdfm_finish_batch_active() == 0
    # a second _begin
    assert lib.xdfm_finish_batch_begin() == 0
    try:
        assert lib.xdfm_finish_batch_begin() == 1 and b"open" in lib.xdfm_last_error()
        assert lib.xdfm_finish_batch_active() == 1, "the refused call leaves the batch as it was"
    finally:
        assert lib.xdfm_finish_batch_run(_st()) == 0
    # _run on another stream than the jobs'
    gen = torch.Generator().manual_seed(24)
    case = _head_bwd(dev, gen, 257)
    want = _separate(case)
    other = torch.cuda.Stream(device=dev)
    outs = case.outs(True)
    assert lib.xdfm_finish_batch_begin() == 0
    try:
        case.call(outs)
        assert lib.xdfm_finish_batch_run(ctypes.c_void_p(other.cuda_stream)) == 1 and b"stream" in lib.xdfm_last_error()
        with torch.cuda.stream(other):                 # nor may a job join from another stream
            with pytest.raises(ValueError, match="stream"):
                case.call(case.outs(True))
    finally:
        assert lib.xdfm_finish_batch_run(_st()) == 0, "the refused _run left the batch open; this one runs it"
    torch.cuda.synchronize()
    _same(case, outs, want)
    # the option at 0: _begin opens nothing, the finish launches itself
    _lib.set_option("finish_batch", 0)
    assert lib.xdfm_finish_batch_begin() == 0 and lib.xdfm_finish_batch_active() == 0
    outs = case.outs(True)
    case.call(outs)
    torch.cuda.synchronize()
    _same(case, outs, want)
    assert lib.xdfm_finish_batch_run(_st()) == 0


# ------------------------------------------------------------------------------------------ whole step
def _model(dev, activation="relu", task="binary", loss="binary_crossentropy"):
    from deepctr.inputs import DenseFeat, SparseFeat
    from deepctr.models import xDeepFM
    from xdfm_amd import graphstep
    cols = [SparseFeat("C%d" % (i + 1), 50, 4) for i in range(4)] + [DenseFeat("I%d" % (i + 1), 1) for i in range(2)]
    model = xDeepFM(cols, cols, dnn_hidden_units=(8, 8), cin_layer_size=(8, 8), l2_reg_linear=1e-4, l2_reg_embedding=1e-4,
                    l2_reg_dnn=1e-4, l2_reg_cin=1e-4, init_std=0.1, seed=77, dnn_activation=activation, task=task, device=dev)
    model.compile("adam", loss, metrics=[])
    model.train()
    step = graphstep.GraphedStep(model)
    model.__dict__["_graphed_step"] = step
    return model, step


def _six_steps(dev, fb, **kw):
    from oracle import xdeepfm_oracle as orc
    from xdfm_amd import _lib, graphstep
    _lib.set_option("finish_batch", fb)
    model, step = _model(dev, **kw)
    assert model._l2_fusion() is not None, "the step under test: the L2 term in the optimizer"
    outs = []
    for s in range(6):
        X, y = orc.synthetic_batch(64, [50] * 4, 2, seed=900 + s)
        if kw.get("task") == "regression":
            y = y * 2.5 - 0.5
        out = model.train_on_batch(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
        outs.append([t.detach().clone() for t in out])
    torch.cuda.synchronize()
    graphs = [e for e in step.entries.values() if e.graph is not None]
    assert len(graphs) == 1 and not step.disabled
    census = graphstep.census(graphs[0].graph)
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    moments = {k: (model.optim.state[p]["exp_avg"].clone(), model.optim.state[p]["exp_avg_sq"].clone())
               for k, p in model.named_parameters()}
    return outs, params, moments, census, step.replays


@pytest.mark.parametrize("variant", ["relu_bce", "prelu", "regression_mse"])
def test_six_train_steps_with_and_without_the_batch_give_the_same_bits_in_fewer_nodes(monkeypatch, variant):
    monkeypatch.setenv("XDFM_HIP_GRAPH", "1")
    dev = _dev()
    kw = {"relu_bce": {}, "prelu": {"activation": "prelu"}, "regression_mse": {"task": "regression", "loss": "mse"}}[variant]
    on = _six_steps(dev, 1, **kw)
    off = _six_steps(dev, 0, **kw)
    for s, (a, b) in enumerate(zip(on[0], off[0])):
        for name, ta, tb in zip(("y_pred", "loss", "total loss"), a, b):
            assert ta.shape == tb.shape and torch.equal(ta, tb), "step %d: %s differs" % (s, name)
        assert bool(torch.isfinite(a[2]).all()) and float(a[2].reshape(-1)[0]) != float(a[1].reshape(-1)[0]), "the L2 value is in the total"
    assert list(on[1]) == list(off[1])
    for k in on[1]:
        assert torch.equal(on[1][k], off[1][k]), "parameter %s differs" % k
        assert torch.equal(on[2][k][0], off[2][k][0]) and torch.equal(on[2][k][1], off[2][k][1]), "Adam moments of %s differ" % k
    (n1, memset1, other1), (n0, memset0, other0) = on[3], off[3]
    print("captured train step (%s): %d nodes with the finish batch, %d without" % (variant, n1, n0))
    assert on[4] > 0 and off[4] > 0, "replays"
    assert memset1 == 0 and other1 == 0 and memset0 == 0
    assert n1 < n0, (n1, n0)
