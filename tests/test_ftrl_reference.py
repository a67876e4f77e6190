"""CPU: the FTRL-Proximal reference of the kernel tests (ftrl_ref.py).  The fp32 mirror of ftrl_one stays within HALF of the
bars of the float64 step over every committed set, tensor and step -- ten-step trajectories on aligned inputs, single steps on
random signs -- and within the threshold cap; the zero-gradient rule; the
exact zeros of the L1 term; TableFTRL's torch-op path (CPU parameters) against float64."""
import numpy as np
import pytest
import torch

import ftrl_ref as F

F32 = F.F32


@pytest.mark.parametrize("name", F.SETS)
def test_the_fp32_mirror_stays_within_half_the_bars_and_the_threshold_cap(name):
    state, signs, want, values = F.dense_case(name)
    got, got_values = F.run_ref(F.ftrl_f32, name, state, F.SIZES, lambda st: F.dense_grads(F.SIZES, st, signs=signs), F32)
    worst, left = dict.fromkeys("pzn", 0.0), 0
    for k in range(F.STEPS):
        shares, out, excess = F.compare(got[k], want[k], F.HYPER[name]["l1"])
        assert excess <= 0, "step %d: a tensor leaves %d elements more than its cap out" % (k + 1, excess)
        worst = {q: max(worst[q], shares[q]) for q in "pzn"}
        left += out
    print("ftrl %s: mirror against float64, shares of the bars %r, %d elements left out" % (name, worst, left))
    assert all(worst[q] <= 0.5 for q in "pzn"), worst
    np.testing.assert_allclose(got_values, values, rtol=F.L2_RTOL)
    if any(F.HYPER[name]["l2m"]):
        assert min(values) > 0.0


@pytest.mark.parametrize("name", F.SETS)
def test_the_fp32_mirror_stays_within_half_the_bars_one_step_at_a_time_on_random_signs(name):
    worst, left = dict.fromkeys("pzn", 0.0), 0
    for k, (got, want) in enumerate(F.single_steps(name)):
        shares, out, excess = F.compare(got, want, F.HYPER[name]["l1"])
        assert excess <= 0, "step %d: a tensor leaves %d elements more than its cap out" % (k + 1, excess)
        worst = {q: max(worst[q], shares[q]) for q in "pzn"}
        left += out
    print("ftrl %s: mirror against float64, single steps on random signs, shares of the bars %r, %d elements left out" % (name, worst, left))
    assert all(worst[q] <= 0.5 for q in "pzn"), worst


@pytest.mark.parametrize("step_fn, dtype", [(F.ftrl_f64, np.float64), (F.ftrl_f32, F32)])
def test_a_zero_gradient_keeps_all_three_bits_and_n_zero_gives_no_nan(step_fn, dtype):
    p = np.array([0.3, -0.2, 0.0, 1e-20, 0.5, 0.0], F32)
    z = np.array([0.1, -7.0, 0.0, 3.0, 0.0, 0.0], F32)
    n = np.array([0.1, 0.0, 0.0, 2.0, 0.0, 0.0], F32)
    g = np.array([0.0, 0.0, 0.0, 0.0, 0.25, 0.0], F32)
    # no model L2 term: g' == g.  Elements 1, 2 and 5 have n == 0 with g == 0 (0 / 0 without the rule); the closed form would
    # send element 0 from 0.3 to -0.1 * lr / ... and element 1 to a large value
    p1, z1, n1, _ = step_fn(p, z, n, g, 0.05, 0.0, 1e-3, 1e-3, 1.0)
    for a, b in ((p1, p), (z1, z), (n1, n)):
        assert np.all(np.isfinite(a))
        assert np.array_equal(F.bits(np.delete(a, 4).astype(F32)), F.bits(np.delete(b, 4)))
    assert p1[4] != p[4] and z1[4] != 0.0 and n1[4] == dtype(0.0625)
    # with a model L2 term g' = 2 l2m p: only a weight that is 0 itself has g' == 0
    p2, z2, n2, value = step_fn(p, z, n, g, 0.05, 0.25, 1e-3, 1e-3, 1.0)
    still = np.array([False, False, True, False, False, True])
    for a, b in ((p2, p), (z2, z), (n2, n)):
        assert np.all(np.isfinite(a))
        assert np.array_equal(F.bits(a[still].astype(F32)), F.bits(b[still]))
    assert np.all(p2[~still] != p[~still])                # every other weight moved
    assert abs(value - 0.25 * float(np.sum(p.astype(np.float64) ** 2))) <= 1e-6 * value


@pytest.mark.parametrize("step_fn", [F.ftrl_f64, F.ftrl_f32])
def test_l1_gives_exact_zeros_that_stay_and_leave_again(step_fn):
    l1 = 1e-2
    p = np.array([0.05, -0.05, 0.05], F32)
    z = np.array([0.0, 0.0, 1.0], F32)
    n = np.full(3, 0.1, F32)
    g = np.array([1e-3, -1e-3, 1e-3], F32)
    p, z, n, _ = step_fn(p, z, n, g, 0.1, 0.0, l1, 0.0, 1.0)
    assert abs(z[0]) <= l1 and abs(z[1]) <= l1 and abs(z[2]) > l1
    assert p[0] == 0.0 and p[1] == 0.0 and not np.signbit(p[0]) and p[2] < 0.0          # clipped to +0.0, exactly
    kept = (p.copy(), z.copy(), n.copy())
    for _ in range(3):                                                                      # zero gradients: nothing moves
        p, z, n, _ = step_fn(p, z, n, np.zeros(3, F32), 0.1, 0.0, l1, 0.0, 1.0)
    assert all(np.array_equal(a, b) for a, b in zip((p, z, n), kept))
    p, z, n, _ = step_fn(p, z, n, np.array([0.5, -0.5, 0.0], F32), 0.1, 0.0, l1, 0.0, 1.0)   # a large gradient: off zero again
    assert p[0] < 0.0 and p[1] > 0.0 and p[2] == kept[0][2]


@pytest.mark.parametrize("name", ["F1", "F2"])
def test_table_ftrl_torch_op_path_on_cpu_tensors_against_float64(name):
    """TableFTRL on CPU parameters takes its torch-op step: ten steps on the dense case (the model's L2 term armed by hand for
    F2) within the bars of float64 and the threshold cap, the L2 value within its rtol."""
    from xdfm_amd.optim import TableFTRL
    h = F.HYPER[name]
    state, signs, want, values = F.dense_case(name)
    idx = [t for t in range(len(F.SIZES)) if F.SIZES[t] <= 50000]            # the 1.1 M-element tensor is the kernel tests'
    params = [torch.nn.Parameter(torch.from_numpy(state[t][0].copy())) for t in idx]
    opt = TableFTRL(params, lr=h["lr"], l1=h["l1"], l2=h["l2"], beta=h["beta"], initial_accumulator_value=h["init"])
    assert opt.deferred is False and opt._kind(opt.param_groups[0]) == "ftrl"
    worst = dict.fromkeys("pzn", 0.0)
    for k in range(F.STEPS):
        flat, offs = F.dense_grads(F.SIZES, k + 1, signs=signs)
        for q, t in zip(params, idx):
            q.grad = torch.from_numpy(flat[offs[t]:offs[t] + F.SIZES[t]].copy())
        if k == 0:                                          # the committed z is not zero: the first step creates the state
            for q, t in zip(params, idx):
                z, n = opt._zn(opt.param_groups[0], q)
                assert float(z.abs().max()) == 0.0 and float(n.min()) == float(n.max()) == float(F32(h["init"]))
                z.copy_(torch.from_numpy(state[t][1]))
                n.copy_(torch.from_numpy(state[t][2]))
        if any(h["l2m"]):
            opt.arm_l2(params, [h["l2m"][t] for t in idx])
        opt.step()
        got = [(q.detach().numpy(), opt.state[q]["z"].numpy(), opt.state[q]["n"].numpy()) for q in params]
        shares, _, excess = F.compare(got, [want[k][t] for t in idx], h["l1"])
        assert excess <= 0
        worst = {q: max(worst[q], shares[q]) for q in "pzn"}
        if any(h["l2m"]):
            ref = sum(float(F32(h["l2m"][t])) * float(np.sum(((state[t][0] if k == 0 else want[k - 1][t][0]).astype(np.float64)) ** 2))
                      for t in idx)
            assert abs(float(opt.l2_value) - ref) <= 1e-5 * ref
        else:
            assert opt.l2_value is None
    print("ftrl %s: torch-op path against float64, shares of the bars %r" % (name, worst))
    assert all(worst[q] <= 1.0 for q in "pzn"), worst
    assert all(opt.state[q]["z"].dtype == torch.float32 and opt.state[q]["n"].shape == q.shape for q in params)
