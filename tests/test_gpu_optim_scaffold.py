"""GPU tests (-m gpu) of what the four table optimizers' shared host scaffold (`optim._TableStep`) must keep per class: what
`state_dict()` does to the deferred state, a `load_state_dict` round trip in the middle of a deferred run, and what becomes
of the backlog of replayed steps when the deferred state is dropped.  Every comparison is against the dense sweep of the
same class (`deferred=False`) over the same batches, bit for bit where the quantity is a tensor the optimizer writes."""
import pytest
import torch

from test_gpu_optim_deferred import ND, VOCAB, T, _big_vocab_model, _dev, _needs_default_env

pytestmark = pytest.mark.gpu
KINDS = ["adam", "sgd", "adagrad", "rmsprop"]
BATCH, STEPS = 32, 5


def _batches(dev):
    from oracle import xdeepfm_oracle as orc
    return [tuple(T(a).to(dev) for a in orc.synthetic_batch(BATCH, VOCAB, ND, seed=1300 + s)) for s in range(STEPS)]


_DENSE = {}


def _dense(kind):
    """The dense sweep over the STEPS batches, once per class: (parameters at the end, total loss summed up to each step)."""
    if kind not in _DENSE:
        dev = _dev()
        model, _ = _big_vocab_model(dev, kind, False, False)
        totals = []
        for X, y in _batches(dev):
            totals.append((totals[-1] if totals else 0.0) + float(model.train_on_batch(X, y)[2]))
        assert model.optim._def is None
        _DENSE[kind] = ([p.detach().clone() for p in model.parameters()], totals)
    return _DENSE[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_and_load_state_dict_in_the_middle_of_a_deferred_run(kind):
    """Three deferred steps (rows owe steps), `state_dict()` -- TableAdam keeps its deferred state and `generation`, the
    other three drop the state and raise `generation` --, `load_state_dict(state_dict())`, two more steps, a flush: the
    parameters are the dense sweep's, bit for bit."""
    _needs_default_env('arena')
    dev = _dev()
    model, _ = _big_vocab_model(dev, kind, True, False)
    opt = model.optim
    batches = _batches(dev)
    for X, y in batches[:3]:
        model.train_on_batch(X, y)
    assert opt._def is not None and len(opt._def["tensors"]) == 12 and opt._since >= 2
    gen = opt.generation
    sd = opt.state_dict()
    assert opt._since == 0                               # flushed: what was handed out is current
    if kind == "adam":
        assert opt._def is not None and opt.generation == gen
    else:
        assert opt._def is None and opt.generation > gen
    gen = opt.generation
    opt.load_state_dict(sd)
    assert opt._def is None and opt._since == 0 and opt.generation > gen
    for X, y in batches[3:]:
        model.train_on_batch(X, y)
    assert opt._def is not None and opt._since >= 1      # deferred again, by the first eager step after the load
    opt.flush()
    for a, b in zip(model.parameters(), _dense(kind)[0]):
        assert torch.equal(a.detach(), b)


@pytest.mark.parametrize("kind", KINDS)
def test_backlog_of_replayed_steps_across_a_dropped_deferred_state(kind):
    """`_invalidate()` with steps owed: SGD, Adagrad and RMSprop park the backlog cell, and `take_backlog()` still returns the
    L2 value of the replayed steps -- the per-step losses plus it agree with the dense sweep's sum within 2e-6 relative, the
    bound of test_deferred_epoch_loss_with_the_backlog_matches_the_dense_sweep for the same quantity.  TableAdam loses the
    cell with the state: 0.0."""
    _needs_default_env('arena')
    dev = _dev()
    model, _ = _big_vocab_model(dev, kind, True, False)
    opt = model.optim
    total = 0.0
    for X, y in _batches(dev)[:4]:
        total += float(model.train_on_batch(X, y)[2])
    assert opt._def is not None and opt._since >= 2
    opt._invalidate()
    assert opt._def is None and opt._since == 0
    backlog = opt.take_backlog()
    if kind == "adam":
        assert backlog == 0.0
        return
    dense = _dense(kind)[1][3]
    print("%s: dense %.9g deferred %.9g + backlog %.9g, rel %.3g" % (kind, dense, total, backlog, abs(dense - total - backlog) / abs(dense)))
    assert backlog > 0.0 and abs(dense - (total + backlog)) <= 2e-6 * abs(dense), (dense, total, backlog)
    assert opt.take_backlog() == 0.0                     # taken once
