"""CPU: the float64 reference of the SGD / Adagrad / RMSprop kernel tests (tests/opt_ref.py: opt_f64) is torch's formula, and
the bars of tests/test_gpu_opt_abi.py are reachable in fp32.

The first test ties opt_f64 to torch.optim.SGD / Adagrad / RMSprop on float64 CPU tensors, not to the kernels.  The second
runs a numpy fp32 emulation of the kernels' element update, in their order of operations (csrc/opt_math.h), on exactly the
inputs of the GPU test (a) and requires it to stay within HALF of every bar: a bar that correct fp32 arithmetic could not
keep would say nothing about a kernel.  The third shows why the large-rate set L is kept out of the float64 comparisons."""
import numpy as np
import pytest
import torch

import opt_ref as R

STEPS = 6


def _torch_opt(kind, h, params, state):
    """The stock optimizer with the fp32-rounded coefficients, its accumulators set to the case's."""
    lr, eps, alpha = (float(np.float32(h[k])) for k in ("lr", "eps", "alpha"))
    if kind == "sgd":
        return torch.optim.SGD(params, lr=lr)
    if kind == "adagrad":
        opt = torch.optim.Adagrad(params, lr=lr, eps=eps)
        for p, (_, s) in zip(params, state):
            opt.state[p]["sum"].copy_(torch.from_numpy(s.astype(np.float64)))
        return opt
    opt = torch.optim.RMSprop(params, lr=lr, alpha=alpha, eps=eps)
    for p, (_, s) in zip(params, state):               # created by the first step when absent (as zeros)
        opt.state[p] = {"step": torch.tensor(0.0), "square_avg": torch.from_numpy(s.astype(np.float64))}
    return opt


# alpha = 0.99 and 0.9 are no fp32 numbers, and fl32(alpha) + fl32(1 - alpha) != 1: the stock RMSprop, which takes 1 - alpha
# from the one alpha it is given, cannot be handed both of the kernels' weights.  The formula is therefore tied to
# torch.optim.RMSprop at the nearest alpha for which both roundings are exact, and the set's own alpha to the stock step's
# spelling in torch primitives (below)
DYADIC = {0.99: 1.0 - 2.0 ** -6, 0.9: 1.0 - 2.0 ** -3, 0.0: 0.0}


def _case(kind, hp):
    h = dict(R.hyper(kind, hp))
    sizes, l2 = [67, 4099, 8192], [5e-2, 0.0, 1e-3]
    return h, sizes, l2, R.make_state(h, sizes, seed=7)


def _lr(hp, h, st):
    return R.lr_of(hp, st)[0] if hp in R.HYPER else h["lr"]


@pytest.mark.parametrize("kind,hp", R.CASES_F64)
def test_opt_f64_is_torchs_formula(kind, hp):
    """Six steps of opt_f64 against the stock torch optimizer on float64 tensors, 2 * l2 * w added to the gradient by hand,
    torch fed the fp32-rounded coefficients: 1e-12 relative.  Every set that is compared with float64; set L runs the same
    function with other numbers and is never compared with it."""
    h, sizes, l2, state = _case(kind, hp)
    if kind == "rmsprop":
        h["alpha"] = DYADIC[h["alpha"]]
        assert float(np.float32(h["alpha"])) == h["alpha"] and float(np.float32(1.0 - h["alpha"])) == 1.0 - h["alpha"]
    ps = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p, _ in state]
    opt = _torch_opt(kind, h, ps, state)
    cur = [(p.astype(np.float64), s.astype(np.float64)) for p, s in state]
    for st in range(1, STEPS + 1):
        lr = _lr(hp, h, st)
        flat, offs = R.dense_grads(sizes, st, seed=7)
        for t, n in enumerate(sizes):
            g = flat[offs[t]:offs[t] + n].astype(np.float64)
            ps[t].grad = torch.from_numpy(g) + float(np.float32(2.0) * np.float32(l2[t])) * ps[t].detach()
            p, s, _ = R.opt_f64(kind, cur[t][0], cur[t][1], g, lr, l2[t], h["eps"], h["alpha"])
            cur[t] = (p, s)
        for grp in opt.param_groups:
            grp["lr"] = float(np.float32(lr))
        opt.step()
    key = {"adagrad": "sum", "rmsprop": "square_avg"}.get(kind)
    for t in range(len(sizes)):
        np.testing.assert_allclose(cur[t][0], ps[t].detach().numpy(), rtol=1e-12, atol=0)
        if key:
            np.testing.assert_allclose(cur[t][1], opt.state[ps[t]][key].numpy(), rtol=1e-12, atol=0)
    assert any(np.any(c[0] != s[0]) for c, s in zip(cur, state))


@pytest.mark.parametrize("hp", ["R0", "R1"])
def test_opt_f64_rmsprop_with_both_rounded_weights(hp):
    """The sets whose alpha is not dyadic, against the stock step spelled in torch's own primitives on float64 tensors
    (torch/optim/rmsprop.py: mul_(alpha), addcmul_(g, g, value=1 - alpha), sqrt().add_(eps), addcdiv_(g, avg, value=-lr))
    with fl32(alpha) and fl32(1 - alpha): 1e-12 relative."""
    h, sizes, l2, state = _case("rmsprop", hp)
    al, oma, eps = (float(np.float32(x)) for x in (h["alpha"], 1.0 - h["alpha"], h["eps"]))
    assert al + oma != 1.0
    for t, n in enumerate(sizes):
        p, v = (torch.from_numpy(a.astype(np.float64)) for a in state[t])
        cur = tuple(a.astype(np.float64) for a in state[t])
        for st in range(1, STEPS + 1):
            flat, offs = R.dense_grads(sizes, st, seed=7)
            g = flat[offs[t]:offs[t] + n].astype(np.float64)
            gt = torch.from_numpy(g) + float(np.float32(2.0) * np.float32(l2[t])) * p
            v.mul_(al).addcmul_(gt, gt, value=oma)
            p.addcdiv_(gt, v.sqrt().add_(eps), value=-float(np.float32(h["lr"])))
            cur = R.opt_f64("rmsprop", cur[0], cur[1], g, h["lr"], l2[t], h["eps"], h["alpha"])[:2]
        np.testing.assert_allclose(cur[0], p.numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(cur[1], v.numpy(), rtol=1e-12, atol=0)


def _shares(kind, hp):
    """Shares of the p, accumulator and L2-value bars that the fp32 emulation uses on the inputs of the GPU test (a)."""
    h = R.hyper(kind, hp)
    state = R.make_state(h)
    grads = {s: R.dense_grads(R.SIZES, s) for s in range(1, STEPS + 1)}
    lr_fn = (lambda s: R.lr_of(hp, s)[0]) if hp in R.HYPER else (lambda s: h["lr"])
    want, want_l2 = R.run_ref(R.opt_f64, kind, h, state, R.SIZES, grads.__getitem__, R.L2_A, STEPS, lr_fn, np.float64)
    got, got_l2 = R.run_ref(R.opt_f32, kind, h, state, R.SIZES, grads.__getitem__, R.L2_A, STEPS, lr_fn, np.float32)
    out = R.shares_of(kind, got, want)
    out["l2"] = max(abs(a - b) / (R.L2_RTOL * b) for a, b in zip(got_l2, want_l2))
    return out


@pytest.mark.parametrize("kind,hp", R.CASES_F64)
def test_bars_are_reachable_in_fp32(kind, hp):
    """A condition on the hyper-parameter sets, not a measurement of a kernel: plain fp32 in the kernels' order stays within
    half of every bar of test_gpu_opt_abi.py (a) on that test's inputs."""
    sh = _shares(kind, hp)
    print("fp32 emulation %s %s: share of the bar %s" % (kind, hp, " ".join("%s %.3f" % kv for kv in sorted(sh.items()))))
    assert all(x <= 0.5 for x in sh.values()), sh


@pytest.mark.parametrize("kind", R.KINDS)
def test_set_L_is_for_bit_comparisons_only(kind):
    """SGD at lr 0.5 and Adagrad at lr 1.0 miss the p bar in fp32 arithmetic alone (the update is as large as the weight and
    its rounding is that of the larger operand), so set L appears only where two GPU paths are compared bit for bit."""
    sh = _shares(kind, "L")
    print("fp32 emulation %s L: share of the bar %s" % (kind, " ".join("%s %.3f" % kv for kv in sorted(sh.items()))))
    if kind != "rmsprop":
        assert sh["p"] > 1.0, sh
