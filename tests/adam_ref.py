"""Reference, cases and C-ABI drivers of the Adam kernel tests (K7 / K7d: csrc/adam.hip; the chunk update:
csrc/adam_math.h, adam_four; the mark scan, the block's L2 partial and the launch loop: csrc/table_step.h).

adam_f64 is one Adam step in numpy float64 with the fp32-rounded coefficients the kernels use; the case builders make the
fixed-seed states and gradients of tests/test_gpu_adam.py; `Bank` and the drivers below it put a state on the device and
call xdfm_adam_step_lr / _step_deferred / _catchup_rows / _apply_rows / _flush on it.  Importing this module needs no GPU
(torch is imported by the drivers only)."""
import ctypes

import numpy as np

F32 = np.float32
SIZES = [1120016, 67, 40989, 3, 4, 4099, 8192]
# With the gradients of all tensors in one flat buffer (offsets rounded up to four floats) and one mark byte per 16-byte
# chunk of it, this order puts the tensors' mark pointers at 0, 4, 5, 13, 14, 15, 0 mod 16: the scan's `head` is
# 0 / 12 / 11 / 1 chunks for the tensors that have more than 16 chunks.
L2_A = [1e-3, 0.0, 5e-2, 0.0, 0.0, 0.0, 0.0]
# (lr, beta1, beta2, eps); H4's lr is 0 for steps 1-3 and goes through the device scalar
HYPER = {
    "H0": (1e-3, 0.9, 0.999, 1e-8),
    "H1": (1e-3, 0.9, 0.999, 1e-13),
    "H2": (1e-3, 0.9, 0.999, 2.0),
    "H3": (1e-3, 0.9, 0.99999, 1e-8),
    "H4": (1e-3, 0.9, 0.999, 1e-8),
    "H5": (2000.0, 0.9, 0.999, 1e-8),
}
TOL = {"p": (2e-6, 1e-8), "m": (2e-6, 2e-8), "v": (2e-6, 1e-10)}      # (rtol, atol) against float64
L2_RTOL = 1e-5
LAZY, DEFERRED = 1, 2


def lr_of(hp, step):
    """Learning rate of 1-based `step` and whether it travels through the device scalar."""
    if hp == "H4":
        return (0.0 if step <= 3 else 1e-3), True
    return HYPER[hp][0], False


def adam_f64(p, g, m, v, step, lr, b1, b2, eps, l2):
    """One Adam step in float64 -> (p, m, v, l2 * sum(p_before^2)).  1 - b1, b2, 1 - b2, eps, 2 * l2, the step size
    lr / (1 - b1^t) and the bias correction sqrt(1 - b2^t) are rounded to fp32 as the kernel rounds them."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    w1, b2f, w2, epsf = float(F32(1.0 - b1)), float(F32(b2)), float(F32(1.0 - b2)), float(F32(eps))
    l2f = float(F32(l2))
    ss = float(F32(lr / (1.0 - b1 ** float(step))))
    bc = float(F32(np.sqrt(1.0 - b2 ** float(step))))
    value = l2f * float(np.sum(p * p))
    g1 = g + float(F32(2.0) * F32(l2)) * p
    m1 = m + w1 * (g1 - m)
    v1 = b2f * v + w2 * g1 * g1
    p1 = p - ss * m1 / (np.sqrt(v1) / bc + epsf)
    return p1, m1, v1, value


def planted_chunks(n):
    """Chunk indices (zeros, |p| = 1e-20, x 2000, |p| = 1e-20 with |m| = 1e-18) planted in a tensor of n elements: four
    adjacent chunks = four neighbouring lanes of one wave, near the start and (large tensors) in the middle."""
    n4 = n // 4
    out = []
    if n4 >= 16:
        out.append(5)
    if n4 >= 1024:
        out.append(n4 // 2 + 1)
    return out


def make_state(sizes=SIZES, seed=3, scale=1.0):
    """[(p, m, v)] fp32: randn * 0.05, randn * 0.01, rand * 1e-4, with the planted rows."""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        p = (rng.randn(n) * 0.05 * scale).astype(F32)
        m = (rng.randn(n) * 0.01).astype(F32)
        v = (rng.rand(n) * 1e-4).astype(F32)
        for c in planted_chunks(n):
            e = 4 * c
            p[e:e + 4] = m[e:e + 4] = v[e:e + 4] = 0.0
            p[e + 4:e + 8] = np.array([1e-20, -1e-20, 1e-20, -1e-20], F32)
            for a in (p, m, v):
                a[e + 8:e + 12] *= F32(2000.0)
            p[e + 12:e + 16] = np.array([-1e-20, 1e-20, 1e-20, -1e-20], F32)
            m[e + 12:e + 16] = np.array([1e-18, -1e-18, -1e-18, 1e-18], F32)
        out.append((p, m, v))
    return out


def grad_offsets(sizes):
    """Offsets (in floats, multiples of 4) of the tensors' gradients in one flat buffer, and the buffer's length."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4
    return offs, off + 8


def dense_grads(sizes, step, seed=3):
    """Flat fresh gradient of 1-based `step`: scale alternating between 0.1 and 1e-3, every 7th element zero."""
    offs, total = grad_offsets(sizes)
    rng = np.random.RandomState(1000 * seed + step)
    flat = (rng.randn(total) * (0.1 if step % 2 else 1e-3)).astype(F32)
    flat[::7] = 0.0
    return flat, offs


def mark_pattern(kind, n, rng):
    """Boolean [n // 4]: which whole chunks of a tensor carry a gradient."""
    n4 = n // 4
    k = np.zeros(n4, dtype=bool)
    if kind == "random3":
        k[:] = rng.rand(n4) < 0.03
    elif kind == "all":
        k[:] = True
    elif kind == "ends" and n4:
        k[0] = k[-1] = True
    return k                     # "none", "tail": no whole chunk


def sparse_grads(sizes, kinds, step, seed=5, chunks=None):
    """Flat gradient that is zero outside the marked chunks and the numel % 4 tail elements (always non-zero), its
    mark bytes (one per chunk of the flat buffer; a tail's chunk is marked too, as the scatter does), and the per-tensor
    boolean chunk masks.  `chunks` (per-tensor boolean masks) overrides `kinds`."""
    offs, total = grad_offsets(sizes)
    rng = np.random.RandomState(1000 * seed + step)
    flat = np.zeros(total, F32)
    marks = np.zeros(total // 4, np.uint8)
    masks = []
    for t, (n, off) in enumerate(zip(sizes, offs)):
        k = chunks[t] if chunks is not None else mark_pattern(kinds[t], n, rng)
        g = (rng.randn(n) * (0.1 if step % 2 else 1e-3)).astype(F32)
        g[::7] = 0.0
        n4 = n // 4
        keep = np.zeros(n, dtype=bool)
        keep[:4 * n4] = np.repeat(k, 4)
        if n % 4:
            keep[4 * n4:] = True
            g[4 * n4:] = F32(0.01) * (1 + np.arange(n % 4, dtype=F32))
            marks[off // 4 + n4] = 1
        flat[off:off + n] = np.where(keep, g, F32(0.0))
        marks[off // 4:off // 4 + n4] = k
        masks.append(k)
    return flat, marks, masks, offs


def share(got, want, rtol, atol):
    """Largest |got - want| / (atol + rtol |want|): the share of the bar that is used (NaN counts as infinite)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    r = np.abs(got - want) / (atol + rtol * np.abs(want))
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max()) if r.size else 0.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# --------------------------------------------------------------------------------------------- device side
def _torch():
    import torch
    return torch


def put(a, dev, off=0):
    """Device copy of the fp32 array `a` starting `off` floats past a 16-byte aligned address."""
    torch = _torch()
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.data_ptr() % 16 == 4 * off
    return t


def _stream():
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Bank:
    """A state on the device: p, m, v per tensor (allocations of their own, `mis` = {"p" | "g" | "m" | "v": floats of
    offset}), the fp32 step counters, one flat gradient buffer with its mark bytes, and `last` bytes per tensor."""

    def __init__(self, state, dev, mis=None, steps0=None):
        torch = _torch()
        mis = mis or {}
        self.dev, self.sizes = dev, [s[0].size for s in state]
        self.p = [put(s[0], dev, mis.get("p", 0)) for s in state]
        self.m = [put(s[1], dev, mis.get("m", 0)) for s in state]
        self.v = [put(s[2], dev, mis.get("v", 0)) for s in state]
        self.goff, total = grad_offsets(self.sizes)
        self.gshift = mis.get("g", 0)
        self.gbuf = torch.zeros(total + 8, dtype=torch.float32, device=dev)
        self.flat = self.gbuf[self.gshift:self.gshift + total]
        self.marks = torch.zeros(total // 4 + 16, dtype=torch.uint8, device=dev)
        assert self.marks.data_ptr() % 16 == 0 and self.gbuf.data_ptr() % 16 == 0
        self.steps = torch.tensor([0.0] * len(state) if steps0 is None else [float(s) for s in steps0], dtype=torch.float32,
                                  device=dev)
        self.last = [torch.zeros(n // 4 + 8, dtype=torch.uint8, device=dev) for n in self.sizes]
        self.lr_dev = torch.zeros(1, dtype=torch.float64, device=dev)
        self.l2_value = torch.zeros(1, dtype=torch.float32, device=dev)

    def mark_ptr(self, t):
        return self.marks.data_ptr() + self.goff[t] // 4

    def set_grads(self, flat, marks=None):
        torch = _torch()
        self.flat.copy_(torch.from_numpy(flat))
        if marks is not None:
            self.marks[:marks.size].copy_(torch.from_numpy(marks))

    def tensor(self, t, l2=0.0, marked=False, flags=0):
        a = self.descriptors([t], [l2], marked, [flags])
        return a

    def descriptors(self, idx, l2, marked, flags):
        from xdfm_amd import _lib
        arr = (_lib.AdamTensor * len(idx))()
        for k, t in enumerate(idx):
            a = arr[k]
            a.param, a.exp_avg, a.exp_avg_sq = self.p[t].data_ptr(), self.m[t].data_ptr(), self.v[t].data_ptr()
            a.grad = self.flat.data_ptr() + 4 * self.goff[t]
            a.step = self.steps.data_ptr() + 4 * t
            a.numel, a.l2, a.flags = self.sizes[t], float(l2[k]), int(flags[k])
            use_marks = marked[k] if isinstance(marked, (list, tuple)) else marked
            a.grad_marks = self.mark_ptr(t) if use_marks else None
            a.last = self.last[t].data_ptr() if (flags[k] & DEFERRED) else None
        return arr

    def get(self, t):
        """(p, m, v) of tensor t as numpy copies."""
        return tuple(x[t].cpu().numpy().copy() for x in (self.p, self.m, self.v))

    def snapshot(self):
        torch = _torch()
        torch.cuda.synchronize()
        return [self.get(t) for t in range(len(self.sizes))]


def adam_step(bank, idx, l2, hp, step, marked=False, flags=None, want_l2=False, clk=None, bump=True):
    """xdfm_adam_step_lr (clk None) or xdfm_adam_step_deferred over the tensors `idx` of `bank`, as 1-based `step` of the
    hyper-parameter set `hp`; the step counters of these tensors advance first.  -> the device scalar that receives the L2
    value (None unless asked for)."""
    torch = _torch()
    from xdfm_amd import _lib
    lib = _lib.load()
    lr, through_dev = lr_of(hp, step)
    _, b1, b2, eps = HYPER[hp]
    if bump:
        bank.steps[torch.tensor(list(idx), device=bank.dev)] += 1.0
    flags = flags or [0] * len(idx)
    arr = bank.descriptors(idx, l2, marked, flags)
    lr_dev = None
    if through_dev:
        bank.lr_dev.fill_(lr)
        lr_dev, lr = ctypes.c_void_p(bank.lr_dev.data_ptr()), 123.0          # `lr` is ignored when lr_dev is given
    ws = out = None
    if want_l2:
        bank.ws = torch.zeros(lib.xdfm_adam_step_ws_elems(len(idx)), dtype=torch.float32, device=bank.dev)
        ws, out = ctypes.c_void_p(bank.ws.data_ptr()), ctypes.c_void_p(bank.l2_value.data_ptr())
    a = ctypes.cast(arr, ctypes.c_void_p)
    if clk is None:
        _lib.check(lib.xdfm_adam_step_lr(a, len(idx), lr, lr_dev, b1, b2, eps, ws, out, _stream()), "adam_step_lr")
    else:
        _lib.check(lib.xdfm_adam_step_deferred(a, len(idx), ctypes.byref(clk.struct), lr, lr_dev, b1, b2, eps, ws, out, _stream()),
                   "adam_step_deferred")
    return bank.l2_value if want_l2 else None


class Clock:
    """xdfm_adam_clock on the device plus the backlog and the scratch cell of the rows API."""

    def __init__(self, dev, cap=16, before=0):
        torch = _torch()
        from xdfm_amd import _lib
        self.clock = torch.tensor([0, before], dtype=torch.int32, device=dev)
        self.consts = torch.zeros(4 * cap, dtype=torch.float32, device=dev)
        self.backlog = torch.zeros(1, dtype=torch.int64, device=dev)
        self.cell = torch.zeros(1, dtype=torch.int64, device=dev)
        assert self.consts.data_ptr() % 16 == 0
        self.struct = _lib.AdamClock(self.clock.data_ptr(), self.consts.data_ptr(), cap)

    def read(self):
        return [int(x) for x in self.clock.cpu().numpy()]

    def take_backlog(self):
        v = float(int(self.backlog.item())) / float(1 << 40)
        self.backlog.zero_()
        return v


def adam_flush(bank, idx, l2, clk, hp):
    from xdfm_amd import _lib
    _, b1, b2, eps = HYPER[hp]
    arr = bank.descriptors(idx, l2, False, [DEFERRED] * len(idx))
    _lib.check(_lib.load().xdfm_adam_flush(ctypes.cast(arr, ctypes.c_void_p), len(idx), ctypes.byref(clk.struct), b1, b2, eps,
                                           ctypes.c_void_p(clk.backlog.data_ptr()), _stream()), "adam_flush")


class Rows:
    """xdfm_adam_rows of some tensors of a bank (one per field); `skip`: fields whose `param` pointer is NULL (left to
    the step's mark scan).  Keeps the device pointer tables alive."""

    def __init__(self, bank, idx, l2, skip=(), with_grads=True):
        torch = _torch()
        from xdfm_amd import _lib
        mk = lambda vals: torch.tensor(vals, dtype=torch.int64, device=bank.dev)
        self.keep = [mk([0 if f in skip else bank.p[t].data_ptr() for f, t in enumerate(idx)]),
                     mk([bank.m[t].data_ptr() for t in idx]), mk([bank.v[t].data_ptr() for t in idx]),
                     mk([bank.last[t].data_ptr() for t in idx]),
                     torch.tensor([float(x) for x in l2], dtype=torch.float32, device=bank.dev)]
        if with_grads:
            self.keep += [mk([bank.flat.data_ptr() + 4 * bank.goff[t] for t in idx]), mk([bank.mark_ptr(t) for t in idx])]
            self.struct = _lib.AdamRows(*[a.data_ptr() for a in self.keep])
        else:
            self.struct = _lib.AdamRows(*([a.data_ptr() for a in self.keep] + [None, None]))


def _rows_args(X, cols, vocab, m, D, emb, lin, clk, hp):
    _, b1, b2, eps = HYPER[hp]
    return (ctypes.c_void_p(X.data_ptr()), X.stride(0), X.shape[0], ctypes.c_void_p(cols.data_ptr()),
            ctypes.c_void_p(vocab.data_ptr()), m, D, ctypes.byref(emb.struct), ctypes.byref(lin.struct) if lin is not None else None,
            ctypes.byref(clk.struct), b1, b2, eps)


def adam_catchup_rows(X, cols, vocab, m, D, emb, lin, clk, hp):
    from xdfm_amd import _lib
    _lib.check(_lib.load().xdfm_adam_catchup_rows(*_rows_args(X, cols, vocab, m, D, emb, lin, clk, hp),
                                                  ctypes.c_void_p(clk.backlog.data_ptr()), _stream()), "adam_catchup_rows")


def adam_apply_rows(X, cols, vocab, m, D, emb, lin, clk, hp, l2_value):
    from xdfm_amd import _lib
    _lib.check(_lib.load().xdfm_adam_apply_rows(*_rows_args(X, cols, vocab, m, D, emb, lin, clk, hp),
                                                ctypes.c_void_p(clk.cell.data_ptr()), ctypes.c_void_p(l2_value.data_ptr()), _stream()),
               "adam_apply_rows")


# --------------------------------------------------------------------------------------------- case (d): 70 tensors
SIZES_70 = [n for _ in range(10) for n in SIZES]
L2_70 = [float(F32(1e-4 * (1 + (k * 7) % 13))) if k % 3 else 0.0 for k in range(70)]


def make_state_70():
    base = make_state(SIZES, seed=11)
    out = []
    for r in range(10):
        f = F32(1.0 + 0.03125 * r)
        out += [(p * f, m.copy(), v.copy()) for p, m, v in base]
    return out


def run_70(dev, batched=True, steps=2, state=None):
    """Case (d): `steps` steps over 70 tensors, in one call (two launches) or in 70 single-tensor calls.
    -> (snapshot, [l2_value of every step as fp32 arrays])."""
    torch = _torch()
    state = state or make_state_70()
    bank = Bank(state, dev)
    values = []
    for s in range(1, steps + 1):
        flat, _ = dense_grads(SIZES_70, s, seed=12)
        bank.set_grads(flat)
        if batched:
            out = adam_step(bank, list(range(70)), L2_70, "H0", s, want_l2=True)
            torch.cuda.synchronize()
            values.append(out.cpu().numpy().copy())
        else:
            for t in range(70):
                adam_step(bank, [t], [L2_70[t]], "H0", s)
    return bank.snapshot(), values
