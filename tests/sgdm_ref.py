"""Reference, cases and C-ABI drivers of the tests of SGD with momentum (K7m: csrc/sgd_adagrad.hip; K7md:
csrc/sgd_adagrad_deferred.hip; the sweep's loops: csrc/table_step.h, tbl_sweep; the element update: csrc/opt_math.h, OPT_SGDM) --
opt_ref.py's counterpart for the fourth kind.  It imports opt_ref / adam_ref and changes neither.

sgdm_f64 is one step in numpy float64 with the fp32-rounded coefficients the kernels use, sgdm_f32 the same step in numpy fp32 in
opt_one's order of operations (test_sgdm_reference.py ties the first to torch.optim.SGD and bounds the second by the bars);
the builders below make the states and gradients of tests/test_gpu_sgdm_abi.py; the drivers call xdfm_sgdm_step,
xdfm_sgdm_step_deferred, xdfm_sgdm_catchup_rows and xdfm_sgdm_flush on an opt_ref.Bank of kind "sgdm" (its `s` arrays are the
momentum buffers).  Importing this module needs no GPU.

THE SIGNS.  The buffer is signed: buf = mu * buf + g' cancels wherever g' is close to -mu * buf, and the error buf carries from
the step before (2^-24 of |mu buf| + |g'|) is then large against the `s` bar, which is relative to the small result.  With the
gradients of opt_ref.dense_grads (random signs) plain fp32 misses that bar by 169x after six steps of M0: element 592499 of the
1 120 016-element tensor, whose buffer has cancelled to -3.3e-6 (M1 126x, M2 26x, M3 24x, MD 120x;
test_sgdm_reference.py::test_random_signs_miss_the_buffer_bar_in_plain_fp32 keeps the measurement alive).
The sets that are compared with float64 therefore use ALIGNED inputs: one sign per element, shared by its p, its buffer and its
gradient of every step (`aligned`), so that buf only grows in magnitude and a cancellation can only come from a weight that
crossed zero, where 2 l2 p is small against buf.  Random signs -- cancellations included -- are what the bit-for-bit tests run on
(set L and `aligned=False`): two paths that must agree agree there too."""
import ctypes

import numpy as np

import opt_ref as R
from opt_ref import F32, L2_A, SIZES, TOL, bits, planted_chunks, share  # noqa: F401  (re-exported)

KIND = "sgdm"
HYPER = {
    "M0": dict(kind=KIND, lr=0.01, mu=0.9, nesterov=False),
    "M1": dict(kind=KIND, lr=0.01, mu=0.9, nesterov=True),
    "M2": dict(kind=KIND, lr=0.01, mu=0.5, nesterov=False),
    "M3": dict(kind=KIND, lr=0.01, mu=0.5, nesterov=True),
    "MD": dict(kind=KIND, lr=0.01, mu=0.9, nesterov=True),        # lr through the device scalar: 0 for steps 1-3
    # set L: a large rate, bit-for-bit tests only (with random signs; never compared with float64)
    "L": dict(kind=KIND, lr=0.5, mu=0.9, nesterov=True),
}
SETS = ["M0", "M1", "M2", "M3", "MD"]           # compared with float64
BASE = "M0"


def lr_of(name, step):
    """Learning rate of 1-based `step` in the dense tests and whether it travels through the device scalar."""
    if name == "MD":
        return (0.0 if step <= 3 else 0.01), True
    return HYPER[name]["lr"], False


def sgdm_f64(p, buf, g, lr, l2, mu, nesterov):
    """One step in float64 -> (p, buf, l2 * sum(p_before^2)): torch.optim.SGD with dampening 0 on g' = g + 2 l2 p.  2.f * l2,
    -(float)lr and (float)mu are rounded to fp32 as the kernels round them (csrc/opt_math.h)."""
    p, buf, g = (np.asarray(a, np.float64) for a in (p, buf, g))
    g2, nlr, muf = float(F32(2.0) * F32(l2)), float(-F32(lr)), float(F32(mu))
    value = float(F32(l2)) * float(np.sum(p * p))
    gp = g + g2 * p
    buf1 = muf * buf + gp
    d = gp + muf * buf1 if nesterov else buf1
    return p + nlr * d, buf1, value


def sgdm_f32(p, buf, g, lr, l2, mu, nesterov):
    """The same step in numpy fp32 in the order of opt_one<OPT_SGDM> (one fma per line) -> (p, buf, value); the value as
    opt_ref.opt_f32 sums it."""
    p, buf, g = (np.asarray(a, F32) for a in (p, buf, g))
    g2, nlr, muf = F32(2.0) * F32(l2), -F32(lr), F32(mu)
    sq = p * p
    parts = np.array([sq[k:k + 8192].sum(dtype=F32) for k in range(0, sq.size, 8192)], F32)
    value = float((F32(l2) * parts).sum(dtype=F32))
    gp = R._fma32(g2, p, g)
    buf1 = R._fma32(muf, buf, gp)
    d = R._fma32(muf, buf1, gp) if nesterov else buf1
    return R._fma32(nlr, d, p), buf1, value


def sgdm_f32_two_roundings(p, buf, g, lr, l2, mu, nesterov):
    """As sgdm_f32 with the buffer's line as ATen's two kernels spell it, mul_(mu) then add_(g'): fl(fl(mu buf) + g')."""
    p, buf, g = (np.asarray(a, F32) for a in (p, buf, g))
    g2, nlr, muf = F32(2.0) * F32(l2), -F32(lr), F32(mu)
    gp = R._fma32(g2, p, g)
    buf1 = ((muf * buf).astype(F32) + gp).astype(F32)
    d = R._fma32(muf, buf1, gp) if nesterov else buf1
    return R._fma32(nlr, d, p), buf1, 0.0


# --------------------------------------------------------------------------------------------- states and gradients
def signs_of(state):
    """One sign per element: that of the starting weight (+1 where it is zero)."""
    return [np.where(p < 0, F32(-1.0), F32(1.0)).astype(F32) for p, _ in state]


def make_state(sizes=SIZES, seed=3, aligned=True):
    """[(p, buf)] fp32: p = randn * 0.05 and the planted chunks of opt_ref.make_state (p = buf = 0; |p| = 1e-20; p and buf x 2000;
    |p| = 1e-20 with buf = 0); buf = randn * 0.02, with the sign of p when `aligned`."""
    base = R.make_state(dict(acc=None), sizes, seed)
    rng = np.random.RandomState(seed + 100)
    out = []
    for (p, _), n in zip(base, sizes):
        buf = (rng.randn(n) * 0.02).astype(F32)
        if aligned:
            buf = np.where(p < 0, -np.abs(buf), np.abs(buf)).astype(F32)
        for c in planted_chunks(n):
            e = 4 * c
            buf[e:e + 4] = 0.0
            buf[e + 8:e + 12] *= F32(2000.0)
            buf[e + 12:e + 16] = 0.0
        out.append((p, buf))
    return out


def _align(flat, offs, sizes, signs):
    if signs is not None:
        for t, n in enumerate(sizes):
            flat[offs[t]:offs[t] + n] = np.abs(flat[offs[t]:offs[t] + n]) * signs[t]
    return flat


def dense_grads(sizes, step, seed=3, signs=None):
    """opt_ref.dense_grads; with `signs` (signs_of) every element's gradient takes its element's sign."""
    flat, offs = R.dense_grads(sizes, step, seed)
    return _align(flat, offs, sizes, signs), offs


def sparse_grads(sizes, kinds, step, seed=5, chunks=None, signs=None):
    """opt_ref.sparse_grads -> (flat, marks, masks, offs), aligned like dense_grads."""
    flat, marks, masks, offs = R.sparse_grads(sizes, kinds, step, seed, chunks)
    return _align(flat, offs, sizes, signs), marks, masks, offs


def masks_e(step, sizes=SIZES, never=False, rate=0.03):
    """The chunk masks of the deferred tests (those of test_gpu_opt_abi.py): `rate` of the chunks drawn per step; the four
    planted chunks are marked at steps 4 and 9 only -- the step's own replay brings them up -- or never (the flush does)."""
    out = []
    for t, n in enumerate(sizes):
        k = np.random.RandomState(1000 * step + t).rand(n // 4) < rate
        for c in planted_chunks(n):
            k[c:c + 4] = (not never) and step in (4, 9)
        out.append(k)
    return out


E_STEPS = 12


def grads_e(step, signs=None):
    """(flat, marks, masks, offs) of 1-based `step` of the deferred test on SIZES."""
    return sparse_grads(SIZES, None, step, seed=9, chunks=masks_e(step), signs=signs)


def run_ref(step_fn, h, state, sizes, grads_of, l2, steps, lr_fn, dtype):
    """Carry `state` through `steps` steps of step_fn (sgdm_f64 / sgdm_f32) -> (final [(p, buf)], [L2 value per step])."""
    cur = [(p.astype(dtype), s.astype(dtype)) for p, s in state]
    values = []
    for st in range(1, steps + 1):
        flat, offs = grads_of(st)
        tot = 0.0
        for t, n in enumerate(sizes):
            p, s, val = step_fn(cur[t][0], cur[t][1], flat[offs[t]:offs[t] + n], lr_fn(st), l2[t], h["mu"], h["nesterov"])
            cur[t] = (p, s)
            tot += val
        values.append(tot)
    return cur, values


def shares_of(got, want, tensors=None):
    """Largest share of the p bar and of the `s` bar (the buffer's) over the tensors; got / want: [(p, buf)]."""
    return R.shares_of(KIND, got, want, tensors)


# --------------------------------------------------------------------------------------------- device side
def bank(state, dev, **kw):
    """An opt_ref.Bank whose `s` arrays are the momentum buffers."""
    return R.Bank(KIND, state, dev, **kw)


def sgdm_step(bank, idx, l2, h, lr, lr_dev=False, marked=False, want_l2=False, deferred=None, check=True, mu=None):
    """One step over the tensors `idx` of `bank`: xdfm_sgdm_step, or (deferred: one bool per tensor = it has `last` bytes)
    xdfm_sgdm_step_deferred on the bank's clock.  Arguments and result as opt_ref.opt_step; `mu` overrides the set's."""
    from xdfm_amd import _lib
    lib = _lib.load()
    arr = bank.descriptors(idx, l2, marked)
    a, T = ctypes.cast(arr, ctypes.c_void_p), len(idx)
    dev_p = None
    if lr_dev:
        bank.lr_dev.fill_(lr)
        dev_p, lr = ctypes.c_void_p(bank.lr_dev.data_ptr()), 123.0
    ws = out = None
    if want_l2:
        assert lib.xdfm_opt_step_ws_elems(T) == 512 * T <= bank.ws.numel()
        ws, out = ctypes.c_void_p(bank.ws.data_ptr()), ctypes.c_void_p(bank.l2_value.data_ptr())
    tail = (h["mu"] if mu is None else mu, int(h["nesterov"]), ws, out, R._stream())
    if deferred is None:
        rc = lib.xdfm_sgdm_step(a, T, lr, dev_p, *tail)
    else:
        last = (ctypes.c_void_p * T)(*[bank.last[t].data_ptr() if d else None for t, d in zip(idx, deferred)])
        clk = bank.clock_struct()
        rc = lib.xdfm_sgdm_step_deferred(a, ctypes.cast(last, ctypes.c_void_p), T, ctypes.byref(clk), lr, dev_p, *tail)
    if not check:
        R._torch().cuda.synchronize()
        bank.check_guards("refused step")
        return rc
    _lib.check(rc, "sgdm_step")
    bank.check_guards("sgdm step")                     # synchronises
    return bank.l2_value.cpu().numpy().copy() if want_l2 else None


def sgdm_flush(bank, idx, l2, h):
    """xdfm_sgdm_flush over the (deferred) tensors `idx`."""
    from xdfm_amd import _lib
    T = len(idx)
    arr = bank.descriptors(idx, l2, True)
    last = (ctypes.c_void_p * T)(*[bank.last[t].data_ptr() for t in idx])
    clk = bank.clock_struct()
    rc = _lib.load().xdfm_sgdm_flush(ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(last, ctypes.c_void_p), T, ctypes.byref(clk),
                                     h["mu"], int(h["nesterov"]), R._stream())
    _lib.check(rc, "sgdm_flush")
    bank.check_guards("flush")


def sgdm_catchup(bank, X, cols, vocab, m, D, emb, lin, h):
    """xdfm_sgdm_catchup_rows for the batch X [B, ldx] on the bank's clock (emb / lin: opt_ref.Rows)."""
    from xdfm_amd import _lib
    clk = bank.clock_struct()
    rc = _lib.load().xdfm_sgdm_catchup_rows(
        ctypes.c_void_p(X.data_ptr()), X.stride(0), X.shape[0], ctypes.c_void_p(cols.data_ptr()), ctypes.c_void_p(vocab.data_ptr()), m, D,
        ctypes.byref(emb.struct), ctypes.byref(lin.struct) if lin is not None else None, ctypes.byref(clk), h["mu"],
        int(h["nesterov"]), R._stream())
    _lib.check(rc, "sgdm_catchup_rows")
    bank.check_guards("catch-up")
