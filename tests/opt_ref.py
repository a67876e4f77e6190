"""Reference, cases and C-ABI drivers of the SGD / Adagrad / RMSprop kernel tests (K7s / K7g / K7r: csrc/sgd_adagrad.hip;
K7sd / K7gd / K7rd: csrc/sgd_adagrad_deferred.hip; the sweep's loops: csrc/table_step.h, tbl_sweep; the element update:
csrc/opt_math.h) -- the counterpart of adam_ref.py.

opt_f64 is one step in numpy float64 with the fp32-rounded coefficients the kernels use, opt_f32 the same step in numpy fp32
in the kernels' order of operations (test_opt_reference.py: the bars are reachable in fp32); the case builders make the
fixed-seed states and gradients of tests/test_gpu_opt_abi.py; `Bank` puts a state on the device, every array inside guard
cells, and the drivers below it call xdfm_sgd_step / _adagrad_step / _rmsprop_step, their _deferred forms,
xdfm_opt_catchup_rows / xdfm_rmsprop_catchup_rows and xdfm_opt_flush / xdfm_rmsprop_flush on it.  Importing this module
needs no GPU (torch is imported by the drivers only)."""
import ctypes

import numpy as np

import adam_ref as A
from adam_ref import F32, L2_A, SIZES, bits, grad_offsets, mark_pattern, planted_chunks, share  # noqa: F401  (re-exported)

KINDS = ("sgd", "adagrad", "rmsprop")
# lr, eps, alpha, initial accumulator (Adagrad: a constant, torch's initial_accumulator_value; RMSprop: rand * 1e-4, None)
HYPER = {
    "S0": dict(kind="sgd", lr=0.01, eps=0.0, alpha=0.0, acc=0.0),
    "S1": dict(kind="sgd", lr=0.01, eps=0.0, alpha=0.0, acc=0.0),           # lr through the device scalar: 0 for steps 1-3
    "G0": dict(kind="adagrad", lr=0.01, eps=1e-10, alpha=0.0, acc=0.0),
    "G1": dict(kind="adagrad", lr=2e-3, eps=1e-10, alpha=0.0, acc=0.1),
    "G2": dict(kind="adagrad", lr=0.01, eps=2.0, alpha=0.0, acc=0.0),
    "R0": dict(kind="rmsprop", lr=1e-4, eps=1e-8, alpha=0.99, acc=None),
    "R1": dict(kind="rmsprop", lr=2e-3, eps=1e-6, alpha=0.9, acc=None),
    # R2: eps 1e-6, not the 1e-8 first meant: with alpha = 0 the step is lr g' / (|g'| + eps), and where g and 2 l2 p cancel to
    # |g'| ~ eps (element 9934 of the 40989-element tensor: g' = 8e-9) fp32's rounding of p moves it by lr * 6e-8 |p| / eps,
    # twice the p bar at eps = 1e-8 in plain fp32 (test_opt_reference.py); the milder eps bounds that by 0.2 of the bar
    "R2": dict(kind="rmsprop", lr=1e-4, eps=1e-6, alpha=0.0, acc=None),
    # set L: large rates, bit-for-bit tests only (fp32 itself misses the float64 bars there: test_opt_reference.py)
    "L-sgd": dict(kind="sgd", lr=0.5, eps=0.0, alpha=0.0, acc=0.0),
    "L-adagrad": dict(kind="adagrad", lr=1.0, eps=1e-10, alpha=0.0, acc=0.0),
    "L-rmsprop": dict(kind="rmsprop", lr=0.01, eps=1e-8, alpha=0.99, acc=None),
}
SETS = {"sgd": ["S0", "S1"], "adagrad": ["G0", "G1", "G2"], "rmsprop": ["R0", "R1", "R2"]}       # compared with float64
BASE = {"sgd": "S0", "adagrad": "G0", "rmsprop": "R0"}
CASES_F64 = [(k, hp) for k in KINDS for hp in SETS[k]]
TOL = {"p": (2e-6, 1e-8), "s": (2e-6, 1e-10)}        # (rtol, atol) against float64: test_gpu_optim.py / test_gpu_adam.py
L2_RTOL = 1e-5
FIX = float(1 << 40)                                 # fixed-point scale of `backlog` and `cell`
ERR_INVALID = 1


def hyper(kind, name):
    """The set `name` of `kind`; "L" and "base" pick the kind's own."""
    if name == "L":
        name = "L-" + kind
    if name == "base":
        name = BASE[kind]
    h = HYPER[name]
    assert h["kind"] == kind
    return h


def lr_of(name, step):
    """Learning rate of 1-based `step` in the dense tests and whether it travels through the device scalar."""
    if name == "S1":
        return (0.0 if step <= 3 else 0.01), True
    return HYPER[name]["lr"], False


def lr_sched(h, step):
    """The deferred tests' rate, through the device scalar: different every step, 0 at steps 3 and 8."""
    return 0.0 if step in (3, 8) else h["lr"] * (1.0 + 0.03125 * (step % 23))


def opt_f64(kind, p, s, g, lr, l2, eps, alpha):
    """One step in float64 -> (p, s, l2 * sum(p_before^2)).  2.f * l2, -(float)lr, (float)eps, (float)alpha and
    (float)(1.0 - alpha) are rounded to fp32 as the kernels round them (csrc/opt_math.h)."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    s = None if s is None else np.asarray(s, np.float64)
    g2, nlr = float(F32(2.0) * F32(l2)), float(-F32(lr))
    epsf, al, oma = float(F32(eps)), float(F32(alpha)), float(F32(1.0 - alpha))
    value = float(F32(l2)) * float(np.sum(p * p))
    gp = g + g2 * p
    if kind == "sgd":
        return p + nlr * gp, s, value
    s1 = s + gp * gp if kind == "adagrad" else al * s + oma * gp * gp
    return p + nlr * gp / (np.sqrt(s1) + epsf), s1, value      # ATen's addcdiv: (value * t1) / t2


def _fma32(a, b, c):
    """fl32(a * b + c) for fp32 arrays: the product is exact in float64, the sum rounds once more before fp32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def opt_f32(kind, p, s, g, lr, l2, eps, alpha):
    """The same step in numpy fp32 in the order of opt_one (csrc/opt_math.h) -> (p, s, value).  The value is summed as the
    kernel's blocks see it only roughly: fp32 partial sums of 8192 elements, added in fp32."""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    g2, nlr = F32(2.0) * F32(l2), -F32(lr)
    epsf, al, oma = F32(eps), F32(alpha), F32(1.0 - alpha)
    sq = p * p
    parts = np.array([sq[k:k + 8192].sum(dtype=F32) for k in range(0, sq.size, 8192)], F32)
    value = float((F32(l2) * parts).sum(dtype=F32))
    gp = _fma32(g2, p, g)
    if kind == "sgd":
        return _fma32(nlr, gp, p), s, value
    s = np.asarray(s, F32)
    s1 = (s + gp * gp).astype(F32) if kind == "adagrad" else _fma32(oma, gp * gp, al * s)
    q = (gp / (np.sqrt(s1) + epsf).astype(F32)).astype(F32)
    return _fma32(nlr, q, p), s1, value


# --------------------------------------------------------------------------------------------- states and gradients
def make_state(h, sizes=SIZES, seed=3):
    """[(p, s)] fp32: p = randn * 0.05, s = the set's accumulator (a constant, or rand * 1e-4), with four planted chunks
    (four neighbouring lanes of one wave) near the start and, in large tensors, in the middle: p = s = 0 (the gradient
    builders put g = 0 there), |p| = 1e-20, p and s x 2000, |p| = 1e-20 with s = 0."""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        p = (rng.randn(n) * 0.05).astype(F32)
        r = (rng.rand(n) * 1e-4).astype(F32)
        s = r if h["acc"] is None else np.full(n, h["acc"], F32)
        for c in planted_chunks(n):
            e = 4 * c
            p[e:e + 4] = s[e:e + 4] = 0.0
            p[e + 4:e + 8] = np.array([1e-20, -1e-20, 1e-20, -1e-20], F32)
            p[e + 8:e + 12] *= F32(2000.0)
            s[e + 8:e + 12] *= F32(2000.0)
            p[e + 12:e + 16] = np.array([-1e-20, 1e-20, 1e-20, -1e-20], F32)
            s[e + 12:e + 16] = 0.0
        out.append((p, s))
    return out


def _zero_planted(flat, sizes, offs):
    for n, off in zip(sizes, offs):
        for c in planted_chunks(n):
            flat[off + 4 * c:off + 4 * c + 4] = 0.0


def dense_grads(sizes, step, seed=3):
    """adam_ref.dense_grads (scale alternating between 0.1 and 1e-3, every 7th element zero) with g = 0 on the planted
    all-zero chunk."""
    flat, offs = A.dense_grads(sizes, step, seed)
    _zero_planted(flat, sizes, offs)
    return flat, offs


def sparse_grads(sizes, kinds, step, seed=5, chunks=None):
    """adam_ref.sparse_grads with g = 0 on the planted all-zero chunk -> (flat, marks, masks, offs)."""
    flat, marks, masks, offs = A.sparse_grads(sizes, kinds, step, seed, chunks)
    _zero_planted(flat, sizes, offs)
    return flat, marks, masks, offs


def run_ref(step_fn, kind, h, state, sizes, grads_of, l2, steps, lr_fn, dtype):
    """Carry `state` through `steps` steps of step_fn (opt_f64 / opt_f32) -> (final [(p, s)], [L2 value per step])."""
    cur = [(p.astype(dtype), s.astype(dtype)) for p, s in state]
    values = []
    for st in range(1, steps + 1):
        flat, offs = grads_of(st)
        tot = 0.0
        for t, n in enumerate(sizes):
            p, s, val = step_fn(kind, cur[t][0], cur[t][1], flat[offs[t]:offs[t] + n], lr_fn(st), l2[t], h["eps"], h["alpha"])
            cur[t] = (p, s)
            tot += val
        values.append(tot)
    return cur, values


def shares_of(kind, got, want, tensors=None):
    """Largest share of the p and the accumulator bar over the tensors; got / want: [(p, s)]."""
    out = {}
    for k, name in enumerate("ps"):
        if name == "s" and kind == "sgd":
            continue
        out[name] = max(share(got[t][k], want[t][k], *TOL[name]) for t in (range(len(got)) if tensors is None else tensors))
    return out


# --------------------------------------------------------------------------------------------- device side
GUARD = 256              # guard bytes on either side of every device array
SENT = 0xA5


def _torch():
    import torch
    return torch


def _stream():
    return ctypes.c_void_p(_torch().cuda.current_stream().cuda_stream)


class Bank:
    """A state on the device.  p and the accumulator of every tensor, the flat gradient buffer, its mark bytes (one per
    16-byte chunk of it), the `last` bytes of every tensor (exactly numel / 4 + 4 of them), the clock, the rates table, the
    backlog, the cell, the L2 workspace and the L2 value each sit in an allocation of their own between two guards of
    256 bytes; every driver checks all guards after its call.  `mis` = {"p" | "g" | "s": floats of offset from a 16-byte
    boundary}."""

    def __init__(self, kind, state, dev, mis=None, cap=16, before=0):
        torch = _torch()
        mis = mis or {}
        self.kind, self.dev, self.sizes, self.cap = kind, dev, [p.size for p, _ in state], cap
        self._bufs = []
        self.p = [self._put(p, mis.get("p", 0)) for p, _ in state]
        self.s = [self._put(s, mis.get("s", 0)) for _, s in state]
        self.goff, total = grad_offsets(self.sizes)
        self.flat = self._new(total, torch.float32, mis.get("g", 0))
        self.marks = self._new(total // 4, torch.uint8)
        self.last = [self._new(n // 4 + 4, torch.uint8) for n in self.sizes]
        self.clock = self._new(2, torch.int32)
        self.clock[1] = before
        self.rates = self._new(cap, torch.float32)
        self.backlog, self.cell = self._new(1, torch.int64), self._new(1, torch.int64)
        self.l2_value = self._new(1, torch.float32)
        self.ws = self._new(512 * len(state), torch.float32)
        self.lr_dev = torch.zeros(1, dtype=torch.float64, device=dev)
        assert self.marks.data_ptr() % 16 == 0 and self.backlog.data_ptr() % 8 == 0 and self.cell.data_ptr() % 8 == 0
        assert all(x.data_ptr() % 4 == 0 for x in self.last)
        self._guards = [g for lo, hi in self._bufs for g in (lo, hi)]

    def _new(self, n, dtype, off=0):
        """n zeroed elements of `dtype`, `off` floats past a 16-byte boundary, between two guards."""
        torch = _torch()
        size = torch.empty((), dtype=dtype).element_size()
        buf = torch.full((2 * GUARD + 16 + n * size,), SENT, dtype=torch.uint8, device=self.dev)
        lo, hi = GUARD + 4 * off, GUARD + 4 * off + n * size
        view = buf[lo:hi].view(dtype)
        view.zero_()
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (4 * off) % 16
        self._bufs.append((buf[:lo], buf[hi:]))
        return view

    def _put(self, a, off=0):
        t = self._new(a.size, _torch().float32, off)
        t.copy_(_torch().from_numpy(np.ascontiguousarray(a)))
        return t

    def check_guards(self, what=""):
        torch = _torch()
        bad = bool((torch.cat(self._guards) != SENT).any())
        assert not bad, "a guard cell was written to (%s)" % what

    def mark_ptr(self, t):
        return self.marks.data_ptr() + self.goff[t] // 4

    def set_grads(self, flat, marks=None):
        torch = _torch()
        self.flat.copy_(torch.from_numpy(flat))
        if marks is not None:
            self.marks.copy_(torch.from_numpy(marks))

    def descriptors(self, idx, l2, marked):
        from xdfm_amd import _lib
        arr = (_lib.OptTensor * len(idx))()
        for k, t in enumerate(idx):
            a = arr[k]
            a.param, a.grad = self.p[t].data_ptr(), self.flat.data_ptr() + 4 * self.goff[t]
            a.state = self.s[t].data_ptr() if self.kind != "sgd" else None
            a.numel, a.l2 = self.sizes[t], float(l2[k])
            use = marked[k] if isinstance(marked, (list, tuple)) else marked
            a.grad_marks = self.mark_ptr(t) if use else None
        return arr

    def clock_struct(self):
        from xdfm_amd import _lib
        return _lib.OptClock(self.clock.data_ptr(), self.rates.data_ptr(), self.cap, self.backlog.data_ptr(), self.cell.data_ptr())

    def get(self, t):
        return self.p[t].cpu().numpy().copy(), self.s[t].cpu().numpy().copy()

    def snapshot(self):
        _torch().cuda.synchronize()
        return [self.get(t) for t in range(len(self.sizes))]

    def read_clock(self):
        return [int(x) for x in self.clock.cpu().numpy()]

    def take_backlog(self):
        v = float(int(self.backlog.item())) / FIX
        self.backlog.zero_()
        return v


def opt_step(bank, idx, l2, h, lr, lr_dev=False, marked=False, want_l2=False, deferred=None, check=True):
    """One step over the tensors `idx` of `bank`: xdfm_sgd_step / _adagrad_step / _rmsprop_step, or (deferred: one bool per
    tensor = it has `last` bytes) their _deferred form on the bank's clock.  lr_dev: the rate travels through the device
    scalar (and the `lr` argument is a value the kernels must ignore).  -> the return code (check=False) or the fp32 L2
    value as a numpy array (want_l2) or None."""
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
    tail = {"sgd": (), "adagrad": (h["eps"],), "rmsprop": (h["alpha"], h["eps"])}[bank.kind] + (ws, out, _stream())
    if deferred is None:
        rc = getattr(lib, "xdfm_%s_step" % bank.kind)(a, T, lr, dev_p, *tail)
    else:
        last = (ctypes.c_void_p * T)(*[bank.last[t].data_ptr() if d else None for t, d in zip(idx, deferred)])
        clk = bank.clock_struct()
        rc = getattr(lib, "xdfm_%s_step_deferred" % bank.kind)(a, ctypes.cast(last, ctypes.c_void_p), T, ctypes.byref(clk), lr, dev_p,
                                                                *tail)
    if not check:
        _torch().cuda.synchronize()
        bank.check_guards("refused step")
        return rc
    _lib.check(rc, "%s_step" % bank.kind)
    bank.check_guards("%s step" % bank.kind)           # synchronises
    return bank.l2_value.cpu().numpy().copy() if want_l2 else None


def opt_flush(bank, idx, l2, h):
    """xdfm_opt_flush / xdfm_rmsprop_flush over the (deferred) tensors `idx`."""
    from xdfm_amd import _lib
    lib = _lib.load()
    T = len(idx)
    arr = bank.descriptors(idx, l2, True)
    last = (ctypes.c_void_p * T)(*[bank.last[t].data_ptr() for t in idx])
    clk = bank.clock_struct()
    a, lp = ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(last, ctypes.c_void_p)
    if bank.kind == "rmsprop":
        rc = lib.xdfm_rmsprop_flush(a, lp, T, ctypes.byref(clk), h["alpha"], h["eps"], _stream())
    else:
        rc = lib.xdfm_opt_flush(int(bank.kind == "adagrad"), a, lp, T, ctypes.byref(clk), h["eps"], _stream())
    _lib.check(rc, "opt_flush")
    bank.check_guards("flush")


class Rows:
    """xdfm_opt_rows of some tensors of a bank (one per field); `skip`: fields whose `param` pointer is NULL (not deferred).
    Keeps the device pointer tables alive."""

    def __init__(self, bank, idx, l2, skip=()):
        torch = _torch()
        from xdfm_amd import _lib
        mk = lambda vals: torch.tensor(vals, dtype=torch.int64, device=bank.dev)
        self.keep = [mk([0 if f in skip else bank.p[t].data_ptr() for f, t in enumerate(idx)]),
                     mk([bank.s[t].data_ptr() for t in idx]), mk([bank.last[t].data_ptr() for t in idx]),
                     torch.tensor([float(x) for x in l2], dtype=torch.float32, device=bank.dev)]
        self.struct = _lib.OptRows(*[a.data_ptr() for a in self.keep])


def opt_catchup(bank, X, cols, vocab, m, D, emb, lin, h):
    """xdfm_opt_catchup_rows / xdfm_rmsprop_catchup_rows for the batch X [B, ldx] on the bank's clock."""
    from xdfm_amd import _lib
    lib = _lib.load()
    clk = bank.clock_struct()
    args = (ctypes.c_void_p(X.data_ptr()), X.stride(0), X.shape[0], ctypes.c_void_p(cols.data_ptr()), ctypes.c_void_p(vocab.data_ptr()),
            m, D, ctypes.byref(emb.struct), ctypes.byref(lin.struct) if lin is not None else None, ctypes.byref(clk))
    if bank.kind == "rmsprop":
        rc = lib.xdfm_rmsprop_catchup_rows(*args, h["alpha"], h["eps"], _stream())
    else:
        rc = lib.xdfm_opt_catchup_rows(int(bank.kind == "adagrad"), *args, h["eps"], _stream())
    _lib.check(rc, "opt_catchup_rows")
    bank.check_guards("catch-up")
