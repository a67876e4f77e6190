"""CPU: the float64 reference of the tests of SGD with momentum (tests/sgdm_ref.py: sgdm_f64) is torch's formula, and the bars
of tests/test_gpu_sgdm_abi.py are reachable in fp32 on that test's inputs.

The first test ties sgdm_f64 to torch.optim.SGD(momentum, nesterov) on float64 CPU tensors, not to the kernels.  The second
runs the numpy fp32 mirror of the kernels' element update (csrc/opt_math.h, OPT_SGDM: one fma per line) on exactly the inputs
of the GPU tests that are compared with float64 -- the six dense steps and the twelve scheduled sparse steps -- and requires
half of every bar (opt_ref.TOL: p 2e-6 / 1e-8, the buffer on the `s` bar 2e-6 / 1e-10).  The third keeps alive why those
inputs carry one sign per element (sgdm_ref.py, "THE SIGNS")."""
import numpy as np
import pytest
import torch

import opt_ref as R
import sgdm_ref as M

STEPS = 6


def _small():
    sizes, l2 = [67, 4099, 8192], [5e-2, 0.0, 1e-3]
    return sizes, l2, M.make_state(sizes, seed=7, aligned=False)


@pytest.mark.parametrize("first_step", [False, True], ids=["given_buffer", "first_step"])
@pytest.mark.parametrize("hp", M.SETS)
def test_sgdm_f64_is_torchs_formula(hp, first_step):
    """Six steps of sgdm_f64 against torch.optim.SGD(momentum=mu, nesterov=...) on float64 tensors, 2 * l2 * w added to the
    gradient by hand, torch fed the fp32-rounded rate and momentum: 1e-12 relative on p and on momentum_buffer.  `first_step`:
    torch starts without a buffer (it makes clone(g') at its first step), sgdm_f64 from zeros -- the same values.  Random
    signs: the formula has no sign convention."""
    h = M.HYPER[hp]
    sizes, l2, state = _small()
    if first_step:
        state = [(p, np.zeros_like(b)) for p, b in state]
    ps = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p, _ in state]
    opt = torch.optim.SGD(ps, lr=float(np.float32(h["lr"])), momentum=float(np.float32(h["mu"])), nesterov=h["nesterov"])
    if not first_step:
        for p, (_, b) in zip(ps, state):
            opt.state[p]["momentum_buffer"] = torch.from_numpy(b.astype(np.float64))
    cur = [(p.astype(np.float64), b.astype(np.float64)) for p, b in state]
    for st in range(1, STEPS + 1):
        lr = M.lr_of(hp, st)[0]
        flat, offs = M.dense_grads(sizes, st, seed=7)
        for t, n in enumerate(sizes):
            g = flat[offs[t]:offs[t] + n].astype(np.float64)
            ps[t].grad = torch.from_numpy(g) + float(np.float32(2.0) * np.float32(l2[t])) * ps[t].detach()
            cur[t] = M.sgdm_f64(cur[t][0], cur[t][1], g, lr, l2[t], h["mu"], h["nesterov"])[:2]
        for grp in opt.param_groups:
            grp["lr"] = float(np.float32(lr))
        opt.step()
    for t in range(len(sizes)):
        np.testing.assert_allclose(cur[t][0], ps[t].detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(cur[t][1], opt.state[ps[t]]["momentum_buffer"].numpy(), rtol=1e-12, atol=1e-300)
    assert any(np.any(c[0] != s[0]) for c, s in zip(cur, state))


def _shares_dense(hp, aligned, step_fn=None):
    """Shares of the p, buffer and L2-value bars that the fp32 mirror uses on the inputs of the GPU test (a)."""
    h = M.HYPER[hp]
    state = M.make_state(aligned=aligned)
    signs = M.signs_of(state) if aligned else None
    grads = {s: M.dense_grads(M.SIZES, s, signs=signs) for s in range(1, STEPS + 1)}
    lr_fn = lambda s: M.lr_of(hp, s)[0]
    want, want_l2 = M.run_ref(M.sgdm_f64, h, state, M.SIZES, grads.__getitem__, M.L2_A, STEPS, lr_fn, np.float64)
    got, got_l2 = M.run_ref(step_fn or M.sgdm_f32, h, state, M.SIZES, grads.__getitem__, M.L2_A, STEPS, lr_fn, np.float32)
    out = M.shares_of(got, want)
    if step_fn is None:
        out["l2"] = max(abs(a - b) / (R.L2_RTOL * b) for a, b in zip(got_l2, want_l2))
    return out


@pytest.mark.parametrize("hp", M.SETS)
def test_bars_are_reachable_in_fp32(hp):
    """A condition on the hyper-parameter sets and the inputs, not a measurement of a kernel: plain fp32 in the kernels' order
    stays within half of every bar on the inputs of test_gpu_sgdm_abi.py (a) -- and so does the spelling that rounds mu * buf
    on its own, as ATen's mul_ / add_ pair does: either is a correct fp32 step."""
    sh = _shares_dense(hp, True)
    two = _shares_dense(hp, True, M.sgdm_f32_two_roundings)
    print("fp32 mirror sgdm %s: share of the bar %s; with mu * buf rounded on its own %s" % (
        hp, " ".join("%s %.3f" % kv for kv in sorted(sh.items())), " ".join("%s %.3f" % kv for kv in sorted(two.items()))))
    assert all(x <= 0.5 for x in sh.values()), sh
    assert all(x <= 0.5 for x in two.values()), two


def test_bars_are_reachable_in_fp32_over_the_deferred_window():
    """The same for the twelve scheduled sparse steps of the deferred test (rate different every step, 0 at steps 3 and 8;
    unmarked chunks see g' = 2 l2 p only)."""
    h = M.HYPER[M.BASE]
    state = M.make_state()
    signs = M.signs_of(state)
    grads = lambda s: (lambda r: (r[0], r[3]))(M.grads_e(s, signs))
    lr_fn = lambda s: R.lr_sched(h, s)
    want, _ = M.run_ref(M.sgdm_f64, h, state, M.SIZES, grads, M.L2_A, M.E_STEPS, lr_fn, np.float64)
    got, _ = M.run_ref(M.sgdm_f32, h, state, M.SIZES, grads, M.L2_A, M.E_STEPS, lr_fn, np.float32)
    sh = M.shares_of(got, want)
    print("fp32 mirror sgdm deferred window: share of the bar %s" % " ".join("%s %.3f" % kv for kv in sorted(sh.items())))
    assert all(x <= 0.5 for x in sh.values()), sh


def test_random_signs_miss_the_buffer_bar_in_plain_fp32():
    """With the random signs of opt_ref.dense_grads the buffer cancels somewhere among a million elements, and correct fp32
    arithmetic misses the `s` bar there (measured: 169x on M0) while it keeps the p bar: the reason the float64 comparisons run
    on aligned inputs and random signs are left to the bit-for-bit tests."""
    sh = _shares_dense("M0", False)
    print("fp32 mirror sgdm M0, random signs: share of the bar %s" % " ".join("%s %.3f" % kv for kv in sorted(sh.items())))
    assert sh["s"] > 1.0 and sh["p"] <= 0.5, sh
