"""Reference, cases and C-ABI drivers of the FTRL-Proximal tests (K7f: csrc/ftrl.hip; the sweep's loops: csrc/table_step.h,
tbl_sweep, shared with K7s / K7g / K7r / K7m; the element update: csrc/opt_math.h, ftrl_one) -- opt_ref.py's counterpart for the
optimizer with two state arrays.  It imports opt_ref / adam_ref and changes neither.

ftrl_f64 is one step in numpy float64 with the fp32-rounded coefficients the kernel uses, ftrl_f32 the same step in numpy fp32 in
ftrl_one's order of operations; the builders make the states and gradients of tests/test_gpu_ftrl_abi.py (adam_ref's SIZES,
mark_pattern, planted_chunks and grad_offsets, through opt_ref's gradient builders); `Bank` puts a state on the device, every
array inside guard cells, and `ftrl_step` calls xdfm_ftrl_step on it.  Importing this module needs no GPU."""
import ctypes
import functools

import numpy as np

import opt_ref as R
from opt_ref import F32, L2_A, L2_RTOL, SIZES, bits, planted_chunks, share  # noqa: F401  (re-exported)

L2_0 = [0.0] * len(SIZES)
# lr, l1, l2 (the paper's lambda_2), beta, initial accumulator, the model's L2 strength per tensor
HYPER = {
    "F0": dict(lr=0.05, l1=0.0, l2=0.0, beta=0.0, init=0.1, l2m=L2_0),
    "F1": dict(lr=0.05, l1=1e-3, l2=1e-3, beta=1.0, init=0.1, l2m=L2_0),
    "F2": dict(lr=0.05, l1=1e-4, l2=1e-4, beta=1.0, init=0.1, l2m=L2_A),
    "FD": dict(lr=0.05, l1=0.0, l2=0.0, beta=0.0, init=0.1, l2m=L2_0),      # F0 with the rate through the device scalar, another every step
    # set Z: bit-for-bit tests only.  n starts at 0 (0 / 0 without the zero-gradient rule) and l1 is large: many weights sit at
    # the |z| = l1 threshold, where fp32 itself does not hold the float64 p bar
    "Z": dict(lr=0.1, l1=1e-2, l2=0.0, beta=1.0, init=0.0, l2m=L2_0),
}
SETS = ["F0", "F1", "F2", "FD"]             # compared with float64
STEPS = 10
# (rtol, atol) against float64.  p: the project's (opt_ref.TOL["p"]).  z and n: rtol 2e-6 and an atol set from the mirror: the
# smallest power of ten at which ftrl_f32's worst error against ftrl_f64 over the committed cases -- SETS x SIZES x 10 steps, as
# trajectories on aligned inputs (`dense_case`) and as single steps on random signs (`single_steps`), both below -- is at most
# half the bar; test_ftrl_reference.py asserts the half.  Measured shares of the bars, worst of the four sets:
#   trajectories:  p 0.248 (F0);   z 0.339 (F2) at 1e-9 already;   n 0.193 (F2)
#   single steps:  p 0.464 (F0);   z 0.418 (FD) at 1e-7 -- 2.33 at 1e-8, 12.5 at 1e-9;   n 0.050 (F2)
# so z takes 1e-7.  n has no smallest power: it is either >= the initial 0.1 or, on the planted chunks that never see a gradient,
# the exact 0 it started as, so its share is the same for every atol down to 0.  It takes opt_ref.TOL["s"]'s 1e-10, the
# project's bar for an accumulator.
TOL = {"p": R.TOL["p"], "z": (2e-6, 1e-7), "n": (2e-6, R.TOL["s"][1])}
# THE SIGNS.  z is a signed sum of gradients: z' = z + g' - sigma p.  With gradients of random sign it cancels -- a walk of steps
# of 0.1 passes through |z| = 0.003 -- while every step leaves an error of 2^-24 of the summands; p' = -z' lr / sqrt(n') (beta =
# l1 = 0) inherits that error relative to the SMALL z'.  Carried over ten steps with opt_ref.dense_grads as they are (random
# signs) plain fp32 misses the p bar: 1.13 of it at step nine of FD, element 262792 of the 1 120 016-element tensor, z = 0.00297
# (F0 0.97; with gradients ten times smaller 0.98 and 0.85).  The TRAJECTORIES that are compared with float64 therefore use
# ALIGNED inputs, as sgdm_ref.py's do: one sign per element, shared by its starting z, by -p and by its gradient of every step,
# so that |z| only grows.  Random signs are compared with float64 one step at a time, each step from the fp32 state it started
# with (`single_steps`; tests/test_gpu_ftrl.py does the same with a model's gradients): there the error of z' is that of ONE
# cancellation, a few 2^-24 of |z + g'| + |sigma p|, which is what the z bar's atol has to cover.  And random signs --
# cancellations and crossings of the |z| = l1 threshold included -- are what the bit-for-bit tests run on (set Z and
# `aligned=False`): two paths that must agree agree there too.


def lr_of(name, step):
    """Learning rate of 1-based `step` and whether it travels through the device scalar (never 0: the step divides by it)."""
    if name == "FD":
        return HYPER[name]["lr"] * (1.0 + 0.03125 * (step % 23)), True
    return HYPER[name]["lr"], False


def threshold_cap(numel):
    """Elements of a tensor that may be left out of one step's value comparison: those where the side under test and float64
    disagree on |z'| <= l1."""
    return max(1, numel // 10000)


def ftrl_f64(p, z, n, g, lr, l2m, l1, l2, beta):
    """One step in float64 -> (p, z, n, l2m * sum(p_before^2)).  2.f * l2m, (float)lr, (float)l1, (float)l2 and (float)beta
    are rounded to fp32 as the kernel rounds them.  sigma in the quotient form, as the kernel: the more accurate one in any
    precision."""
    p, z, n, g = (np.asarray(a, np.float64) for a in (p, z, n, g))
    g2, lrf = float(F32(2.0) * F32(l2m)), float(F32(lr))
    l1f, l2f, bf = float(F32(l1)), float(F32(l2)), float(F32(beta))
    value = float(F32(l2m)) * float(np.sum(p * p))
    gp = g + g2 * p
    live = gp != 0.0
    n1 = n + gp * gp
    r1 = np.sqrt(n1)
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = gp * gp / (lrf * (r1 + np.sqrt(n)))          # 0 / 0 where n == 0 and g' == 0: selected away
    z1 = z + gp - sigma * p
    p1 = np.where(np.abs(z1) <= l1f, 0.0, (np.sign(z1) * l1f - z1) / ((bf + r1) / lrf + l2f))
    return np.where(live, p1, p), np.where(live, z1, z), np.where(live, n1, n), value


def ftrl_f32(p, z, n, g, lr, l2m, l1, l2, beta):
    """The same step in numpy fp32 in the order of ftrl_one (csrc/opt_math.h) -> (p, z, n, value); the value as
    opt_ref.opt_f32 sums it."""
    p, z, n, g = (np.asarray(a, F32) for a in (p, z, n, g))
    g2, lrf = F32(2.0) * F32(l2m), F32(lr)
    l1f, l2f, bf = F32(l1), F32(l2), F32(beta)
    sq = p * p
    parts = np.array([sq[k:k + 8192].sum(dtype=F32) for k in range(0, sq.size, 8192)], F32)
    value = float((F32(l2m) * parts).sum(dtype=F32))
    with np.errstate(invalid="ignore", divide="ignore"):
        gp = R._fma32(g2, p, g)
        live = gp != 0
        n1 = R._fma32(gp, gp, n)
        r1, r0 = np.where(n1 > 0, np.sqrt(n1), np.abs(gp)), np.sqrt(n)      # n' == 0: n == 0 and g'^2 underflowed
        ds = (lrf * (r1 + r0)).astype(F32)
        sigma = np.where(ds > 0, ((gp * gp) / ds).astype(F32), F32(0.0))
        z1 = R._fma32(-sigma, p, z + gp)
        den = ((bf + r1) / lrf + l2f).astype(F32)
        p1 = np.where(np.abs(z1) <= l1f, F32(0.0), ((np.copysign(l1f, z1) - z1) / den).astype(F32))
    return np.where(live, p1, p), np.where(live, z1, z), np.where(live, n1, n), value


# --------------------------------------------------------------------------------------------- states and gradients
def make_state(h, sizes=SIZES, seed=3, aligned=True):
    """[(p, z, n)] fp32: p = randn * 0.05 with the planted chunks of opt_ref.make_state (p = 0 -- the gradient builders put
    g = 0 there --, |p| = 1e-20, p x 2000, |p| = 1e-20), z = randn * 0.02 (0 on the first and the last planted chunk, x 2000 on
    the third) with the sign of -p when `aligned`, n = the set's initial accumulator (0 on the first and the last planted chunk)."""
    base = R.make_state(dict(acc=h["init"]), sizes, seed)
    rng = np.random.RandomState(seed + 200)
    out = []
    for (p, n), size in zip(base, sizes):
        z = (rng.randn(size) * 0.02).astype(F32)
        if aligned:
            z = np.where(p < 0, np.abs(z), -np.abs(z)).astype(F32)
        for c in planted_chunks(size):
            e = 4 * c
            z[e:e + 4] = 0.0
            z[e + 8:e + 12] *= F32(2000.0)
            z[e + 12:e + 16] = 0.0
        out.append((p, z, n))
    return out


def signs_of(state):
    """One sign per element: that of its starting z (the sign of -p where z is 0, +1 where both are)."""
    return [np.where((z < 0) | ((z == 0) & (p > 0)), F32(-1.0), F32(1.0)).astype(F32) for p, z, _ in state]


def _align(flat, offs, sizes, signs):
    if signs is not None:
        for t, size in enumerate(sizes):
            flat[offs[t]:offs[t] + size] = np.abs(flat[offs[t]:offs[t] + size]) * signs[t]
    return flat


def dense_grads(sizes, step, seed=3, signs=None):
    """opt_ref.dense_grads (scale alternating between 0.1 and 1e-3, every 7th element zero, 0 on the planted all-zero chunk);
    with `signs` (signs_of) every element's gradient takes its element's sign."""
    flat, offs = R.dense_grads(sizes, step, seed)
    return _align(flat, offs, sizes, signs), offs


def sparse_grads(sizes, kinds, step, seed=5, chunks=None, signs=None):
    """opt_ref.sparse_grads -> (flat, marks, masks, offs): zero outside the marked chunks and the tails; aligned like dense_grads."""
    flat, marks, masks, offs = R.sparse_grads(sizes, kinds, step, seed, chunks)
    return _align(flat, offs, sizes, signs), marks, masks, offs


def run_ref(step_fn, name, state, sizes, grads_of, dtype, steps=STEPS, l2m=None):
    """Carry `state` through `steps` steps of step_fn (ftrl_f64 / ftrl_f32) with the set `name` -> ([state after every step],
    [L2 value per step]); a state is [(p, z, n)]."""
    h = HYPER[name]
    l2m = h["l2m"] if l2m is None else l2m
    cur = [tuple(a.astype(dtype) for a in s) for s in state]
    states, values = [], []
    for st in range(1, steps + 1):
        flat, offs = grads_of(st)
        tot = 0.0
        for t, size in enumerate(sizes):
            p, z, n, val = step_fn(cur[t][0], cur[t][1], cur[t][2], flat[offs[t]:offs[t] + size], lr_of(name, st)[0], l2m[t],
                                   h["l1"], h["l2"], h["beta"])
            cur[t] = (p, z, n)
            tot += val
        states.append(list(cur))
        values.append(tot)
    return states, values


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """The dense, aligned case of the set `name`, computed once and shared (nobody writes to it) -> (starting state, signs,
    float64 state after every step, float64 L2 value per step)."""
    state = make_state(HYPER[name])
    signs = signs_of(state)
    want, values = run_ref(ftrl_f64, name, state, SIZES, lambda st: dense_grads(SIZES, st, signs=signs), np.float64)
    return state, signs, want, values


def single_steps(name, step_fn=ftrl_f32, dtype=F32, steps=STEPS):
    """Random signs, one step at a time: the state is carried by `step_fn` (the fp32 mirror), and every step is also taken in
    float64 from the very state it started with -> [(state after the step by step_fn, the same by ftrl_f64)]."""
    h = HYPER[name]
    cur = [tuple(a.astype(dtype) for a in s) for s in make_state(h, aligned=False)]
    out = []
    for st in range(1, steps + 1):
        flat, offs = dense_grads(SIZES, st)
        args = [(cur[t][0], cur[t][1], cur[t][2], flat[offs[t]:offs[t] + size], lr_of(name, st)[0], h["l2m"][t], h["l1"], h["l2"],
                 h["beta"]) for t, size in enumerate(SIZES)]
        got, want = [step_fn(*a)[:3] for a in args], [ftrl_f64(*a)[:3] for a in args]
        out.append((got, want))
        cur = got
    return out


def compare(got, want, l1):
    """One step's states, [(p, z, n)] against float64's -> ({"p" | "z" | "n": largest share of its bar}, elements left out,
    largest excess of a tensor's left-out count over its cap: <= 0 when every tensor is within it).  Left out of the three
    value comparisons: elements where the two sides disagree on |z'| <= l1."""
    l1f = float(F32(l1))
    shares = dict.fromkeys("pzn", 0.0)
    left, excess = 0, -1
    for g, w in zip(got, want):
        out = (np.abs(np.asarray(g[1], np.float64)) <= l1f) != (np.abs(w[1]) <= l1f)
        out &= np.isfinite(g[0]) & np.isfinite(g[1]) & np.isfinite(g[2])           # a NaN is never left out
        left += int(out.sum())
        excess = max(excess, int(out.sum()) - threshold_cap(g[0].size))
        for k, name in enumerate("pzn"):
            shares[name] = max(shares[name], share(np.asarray(g[k])[~out], w[k][~out], *TOL[name]))
    return shares, left, excess


# --------------------------------------------------------------------------------------------- device side
class Bank(R.Bank):
    """An opt_ref.Bank with a third array per tensor: p, z (the base class's `s`) and n, each between its own guards.
    `mis` = {"p" | "g" | "s" | "n": floats of offset from a 16-byte boundary}."""

    def __init__(self, state, dev, mis=None):
        super().__init__("ftrl", [(p, z) for p, z, _ in state], dev, mis=mis)
        self.z = self.s
        self.n = [self._put(n, (mis or {}).get("n", 0)) for _, _, n in state]
        self._guards = [g for lo, hi in self._bufs for g in (lo, hi)]

    def descriptors(self, idx, l2, marked):
        from xdfm_amd import _lib
        arr = (_lib.FtrlTensor * len(idx))()
        for k, t in enumerate(idx):
            a = arr[k]
            a.param, a.grad = self.p[t].data_ptr(), self.flat.data_ptr() + 4 * self.goff[t]
            a.z, a.n = self.z[t].data_ptr(), self.n[t].data_ptr()
            a.numel, a.l2 = self.sizes[t], float(l2[k])
            use = marked[k] if isinstance(marked, (list, tuple)) else marked
            a.grad_marks = self.mark_ptr(t) if use else None
        return arr

    def get(self, t):
        return tuple(x[t].cpu().numpy().copy() for x in (self.p, self.z, self.n))


def ftrl_step(bank, idx, l2m, h, lr, lr_dev=False, marked=False, want_l2=False, check=True, arr=None, **over):
    """One xdfm_ftrl_step over the tensors `idx` of `bank`.  lr_dev: the rate travels through the device scalar (and the `lr`
    argument is a value the kernel must ignore).  `over`: l1 / l2 / beta that override the set's; `arr`: descriptors that
    replace the bank's.  -> the return code (check=False) or the fp32 L2 value as a numpy array (want_l2) or None."""
    from xdfm_amd import _lib
    lib = _lib.load()
    arr = bank.descriptors(idx, l2m, marked) if arr is None else arr
    a, T = ctypes.cast(arr, ctypes.c_void_p), len(idx)
    dev_p = None
    if lr_dev:
        bank.lr_dev.fill_(lr)
        dev_p, lr = ctypes.c_void_p(bank.lr_dev.data_ptr()), 123.0
    ws = out = None
    if want_l2:
        assert lib.xdfm_opt_step_ws_elems(T) == 512 * T <= bank.ws.numel()
        ws, out = ctypes.c_void_p(bank.ws.data_ptr()), ctypes.c_void_p(bank.l2_value.data_ptr())
    hyp = [over.get(k, h[k]) for k in ("l1", "l2", "beta")]
    rc = lib.xdfm_ftrl_step(a, T, lr, dev_p, *hyp, ws, out, R._stream())
    if not check:
        R._torch().cuda.synchronize()
        bank.check_guards("refused step")
        return rc
    _lib.check(rc, "ftrl_step")
    bank.check_guards("ftrl step")                     # synchronises
    return bank.l2_value.cpu().numpy().copy() if want_l2 else None
