"""Reference, cases and C-ABI drivers of the row-wise Adagrad tests (K7w: csrc/rowwise.hip; the block's L2 partial and the launch
loop: csrc/table_step.h; the arithmetic: csrc/opt_math.h, rw_*) -- ftrl_ref.py's counterpart for the optimizer with one
accumulator per table row.  It imports opt_ref and changes nothing there.  The reference has no such rule: float64 arithmetic
written out here is the reference.

rw_f64 is one step in numpy float64 with the fp32-rounded coefficients the kernel uses; rw_f32 the same step in numpy fp32 in
the kernel's order of operations (the fma emulation of opt_ref / ftrl_ref, the summation order documented in include/xdfm.h);
`Bank` puts a state on the device, every array inside guard cells, and `rw_step` calls xdfm_rowwise_adagrad_step on it.
Importing this module needs no GPU.

THE BAR.  Every comparison with float64 is ONE step: the float64 step starts from the fp32 state the side under test started
from, so errors do not compound.  Per element of p the bar is  C * 2^-24 * (|p| + |lr g' / den|)  (p: the weight before the
step).  Counting the roundings of the documented sequence, in units of u = 2^-24 and relative to the update U = lr g' / den:
g' = fma(..) 1; S is exact products added in double (2^-53: nothing); ms = (float)(S / D) 1 and s' = s + ms 1, which the root
halves (1 together); sqrtf 1; + eps 1 -- den carries 3; the quotient 1: U carries 5 u; the final fma rounds once more, u |p'| <=
u (|p| + |U|).  So |error| <= u |p| + 6 u |U| <= 6 u (|p| + |U|): the count gives C <= 6.  Measured on this project's build
machine (tests/test_rowwise_reference.py prints it): the mirror's worst ratio |error| / (2^-24 (|p| + |U|)) over all cases, both
L2 settings and ten steps is WORST_MEASURED below; C is twice that, rounded up, as the issue sets it.  The GPU tests use the same C.
The accumulator has two roundings, ms and the sum: |error| <= 2 u (s + ms) <= C u (s + ms); its bar adds 2^-149, the fp32
denormal quantum, for the row whose squares underflow in fp32 (float64 keeps 1e-50 where fp32 has 0)."""
import ctypes
import functools

import numpy as np

import opt_ref as R
from opt_ref import F32, bits  # noqa: F401  (re-exported)

U24 = 2.0 ** -24
WORST_MEASURED = 2.46       # the mirror's worst share of 2^-24 (|p| + |U|), measured (see above); the count allows 6
C_BAR = 5.0                 # ceil(2 * WORST_MEASURED)
S_FLOOR = 2.0 ** -149
L2_RTOL = R.L2_RTOL
# (rows, D): D = 1 is Adagrad itself; 4 .. 64 the lanes path; 12 and 100 multiples of 4 on the units path; 10 the trainer's default
# embedding dim (chunks straddle rows); (4099, 16) is 65 584 elements: several blocks, and 4099 % 4 == 3
CASES = [(1, 4), (5, 1), (7, 8), (6, 12), (67, 10), (130, 16), (33, 32), (9, 64), (3, 100), (4099, 16)]
N = len(CASES)
SIZES = [r * d for r, d in CASES]
LR, EPS = 0.01, 1e-10
L2_0 = [0.0] * N
L2_A = [1e-3] * N
STEPS = 10
UNDERFLOW_ROW = 2           # in every case with more than two rows: |g| = 1e-25 at s = 0


def lr_of(step):
    """The rate of 1-based `step` and whether it travels through the device scalar (odd steps do; another value every step)."""
    return LR * (1.0 + 0.03125 * (step % 23)), bool(step % 2)


def zero_rows(rows):
    """Rows that never get a gradient."""
    return [r for r in range(rows) if r % 5 == 3]


def tree_sum(sq):
    """The documented order of S for float64 squares [rows, D]: chunks of four left to right, the chunk sums padded with zeros
    to a power of two and added as a balanced tree, neighbouring pairs first."""
    rows, D = sq.shape
    C = (D + 3) // 4
    pad = np.zeros((rows, 4 * C), np.float64)
    pad[:, :D] = sq
    q = pad.reshape(rows, C, 4)
    t = ((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3]
    Cp = 1
    while Cp < C:
        Cp *= 2
    full = np.zeros((rows, Cp), np.float64)
    full[:, :C] = t
    while full.shape[1] > 1:
        full = full[:, 0::2] + full[:, 1::2]
    return full[:, 0]


def rw_f64(p, s, g, lr, l2m, eps):
    """One step in float64 -> (p', s', l2m * sum(p^2), |U|) for p, g [rows, D] and s [rows]; 2.f * l2m, (float)lr and (float)eps
    are rounded to fp32 as the kernel rounds them.  The plain formulas: no select is needed where nothing rounds to zero."""
    p, s, g = (np.asarray(a, np.float64) for a in (p, s, g))
    g2, lrf, epsf = float(F32(2.0) * F32(l2m)), float(F32(lr)), float(F32(eps))
    value = float(F32(l2m)) * float(np.sum(p * p))
    gp = g + g2 * p
    s1 = s + (gp * gp).sum(axis=1) / p.shape[1]
    upd = lrf * gp / (np.sqrt(s1) + epsf)[:, None]
    return p - upd, s1, value, np.abs(upd)


def rw_f32(p, s, g, lr, l2m, eps):
    """The same step in numpy fp32 in the kernel's order -> (p', s', value); D == 1 is opt_ref.opt_f32("adagrad")."""
    p, s, g = np.asarray(p, F32), np.asarray(s, F32), np.asarray(g, F32)
    rows, D = p.shape
    if D == 1:
        p1, s1, value = R.opt_f32("adagrad", p[:, 0], s, g[:, 0], lr, l2m, eps, 0.0)
        return p1.reshape(rows, 1), s1, value
    g2, nlr, epsf = F32(2.0) * F32(l2m), -F32(lr), F32(eps)
    sq = (p * p).ravel()
    parts = np.array([sq[k:k + 8192].sum(dtype=F32) for k in range(0, sq.size, 8192)], F32)
    value = float((F32(l2m) * parts).sum(dtype=F32))
    gp = R._fma32(g2, p, g)
    gd = gp.astype(np.float64)
    with np.errstate(under="ignore"):
        ms = (tree_sum(gd * gd) / float(D)).astype(F32)
    s1 = np.where(ms > 0, (s + ms).astype(F32), s)
    den = (np.sqrt(s1) + epsf).astype(F32)
    with np.errstate(under="ignore"):
        q = (gp / den[:, None]).astype(F32)
    return np.where(gp != 0, R._fma32(nlr, q, p), p).astype(F32), s1.astype(F32), value


# --------------------------------------------------------------------------------------------- states and gradients
def make_state(seed=3):
    """[(p [rows, D], s [rows])] fp32: p = randn * 0.05, s = rand * 1e-4, s = 0 on the underflow row."""
    rng = np.random.RandomState(seed)
    out = []
    for rows, D in CASES:
        p = (rng.randn(rows, D) * 0.05).astype(F32)
        s = (rng.rand(rows) * 1e-4).astype(F32)
        if rows > UNDERFLOW_ROW:
            s[UNDERFLOW_ROW] = 0.0
        out.append((p, s))
    return out


def dense_grads(step, seed=3):
    """[g [rows, D]] of 1-based `step`: scale alternating 1e-3 / 1e3, every 7th element zero, the zero rows zero, the underflow row
    |g| = 1e-25 (its squares underflow in fp32, not in double)."""
    rng = np.random.RandomState(1000 * seed + step)
    out = []
    for rows, D in CASES:
        g = (rng.randn(rows, D) * (1e-3 if step % 2 else 1e3)).astype(F32)
        g.reshape(-1)[::7] = 0.0
        g[zero_rows(rows)] = 0.0
        if rows > UNDERFLOW_ROW:
            g[UNDERFLOW_ROW] = np.where(rng.rand(D) < 0.5, F32(1e-25), F32(-1e-25))
        out.append(g)
    return out


MARK_KINDS = ["random3", "all", "ends", "tail", "none", "row1"]


def rows_with_gradient(kind, rows, rng):
    """Which rows a batch touched: 3 % at random (at least one) / all / the first and the last / the rows % 4 tail rows / none /
    row 1 alone (at D = 10 its first chunk straddles into row 0, which has no gradient)."""
    k = np.zeros(rows, bool)
    if kind == "random3":
        k[:] = rng.rand(rows) < 0.03
        k[rng.randint(rows)] = True
    elif kind == "all":
        k[:] = True
    elif kind == "ends":
        k[0] = k[-1] = True
    elif kind == "tail":
        k[rows - rows % 4:] = True
    elif kind == "row1" and rows > 1:
        k[1] = True
    return k


def on_units_path(D):
    """Whether K7w takes a tensor of this D by units of four rows (always, when a pointer is unaligned)."""
    return D not in (4, 8, 16, 32, 64)


def sparse_grads(kind, step, seed=5):
    """-> ([g [rows, D]], [marks uint8 [ceil(rows D / 4)]], [touched rows bool]): values on the touched rows (every 7th element
    zero), zeros elsewhere; a chunk is marked when it overlaps a touched row, as the scatter marks it.  On the units path the
    rows % 4 tail rows' chunks are marked too: the kernel always reads and zeroes them, touched or not."""
    rng = np.random.RandomState(1000 * seed + step)
    gs, ms, ks = [], [], []
    for rows, D in CASES:
        k = rows_with_gradient(kind, rows, rng)
        g = (rng.randn(rows, D) * (1e-3 if step % 2 else 1e3)).astype(F32)
        g.reshape(-1)[::7] = 0.0
        g[~k] = 0.0
        elem = np.repeat(k, D)
        if on_units_path(D):
            elem[(rows - rows % 4) * D:] = True
        pad = np.zeros((rows * D + 3) // 4 * 4, bool)
        pad[:rows * D] = elem
        gs.append(g)
        ms.append(pad.reshape(-1, 4).any(axis=1).astype(np.uint8))
        ks.append(k)
    return gs, ms, ks


def flat_of(gs, fill=0.0, marks=None):
    """The tensors' gradients in adam_ref's flat layout (+ the flat mark bytes when `marks`); `fill`: the value of the gaps and,
    with `marks`, of every unmarked chunk (NaN: a chunk the kernel must not read)."""
    offs, total = R.grad_offsets(SIZES)
    flat = np.full(total, fill, F32)
    fm = np.zeros(total // 4, np.uint8)
    for t, g in enumerate(gs):
        n = g.size
        flat[offs[t]:offs[t] + n] = g.ravel()
        if marks is not None:
            m = marks[t]
            fm[offs[t] // 4:offs[t] // 4 + m.size] = m
            flat[offs[t] + n:offs[t] + 4 * m.size] = 0.0                            # the gap behind a numel % 4 tail, inside its chunk
            flat[offs[t]:offs[t] + 4 * m.size].reshape(-1, 4)[m == 0] = fill       # (a view: the slot is a whole number of chunks)
    return (flat, fm) if marks is not None else flat


def ratios(got_p, got_s, p0, s0, g, lr, l2m, eps):
    """(worst |error of p| / (2^-24 (|p| + |U|)), worst |error of s| / (2^-24 (s + ms) + 2^-149 / C)) of one step that started at
    (p0, s0), against rw_f64 from that very state.  NaN counts as infinite."""
    wp, ws, _, upd = rw_f64(p0, s0, g, lr, l2m, eps)
    rp = np.abs(np.asarray(got_p, np.float64) - wp) / (U24 * (np.abs(np.asarray(p0, np.float64)) + upd))
    rs = np.abs(np.asarray(got_s, np.float64) - ws) / (U24 * ws + S_FLOOR / C_BAR)
    rp = np.where(np.isfinite(rp), rp, np.inf)
    rs = np.where(np.isfinite(rs), rs, np.inf)
    return float(rp.max()), float(rs.max())


@functools.lru_cache(maxsize=None)
def mirror_run(with_l2):
    """The mirror carried through STEPS dense steps from make_state(), computed once and shared (nobody writes to it) ->
    [per step: [(p0, s0, g, p1, s1, value)] per case]; the rate of step s is lr_of(s)."""
    l2m = L2_A if with_l2 else L2_0
    cur = make_state()
    out = []
    for st in range(1, STEPS + 1):
        gs = dense_grads(st)
        row = []
        for t in range(N):
            p1, s1, val = rw_f32(cur[t][0], cur[t][1], gs[t], lr_of(st)[0], l2m[t], EPS)
            row.append((cur[t][0], cur[t][1], gs[t], p1, s1, val))
        cur = [(r[3], r[4]) for r in row]
        out.append(row)
    return out


# --------------------------------------------------------------------------------------------- device side
class Bank(R.Bank):
    """An opt_ref.Bank whose tensors are [rows, D] with an accumulator of `rows` floats; `state`: [(p [rows, D], s [rows])]."""

    def __init__(self, state, dev, mis=None):
        self.shapes = [p.shape for p, _ in state]
        super().__init__("adagrad", [(p.ravel(), s) for p, s in state], dev, mis=mis)

    def descriptors(self, idx, l2, marked):
        from xdfm_amd import _lib
        arr = (_lib.RowwiseTensor * len(idx))()
        for k, t in enumerate(idx):
            a = arr[k]
            a.param, a.grad, a.state = self.p[t].data_ptr(), self.flat.data_ptr() + 4 * self.goff[t], self.s[t].data_ptr()
            a.rows, a.dim, a.l2 = self.shapes[t][0], self.shapes[t][1], float(l2[k])
            use = marked[k] if isinstance(marked, (list, tuple)) else marked
            a.grad_marks = self.mark_ptr(t) if use else None
        return arr

    def get(self, t):
        return self.p[t].cpu().numpy().copy().reshape(self.shapes[t]), self.s[t].cpu().numpy().copy()


def rw_step(bank, idx, l2m, lr, eps=EPS, lr_dev=False, marked=False, want_l2=False, check=True, arr=None):
    """One xdfm_rowwise_adagrad_step over the tensors `idx` of `bank`.  lr_dev: the rate travels through the device scalar (and
    the `lr` argument is a value the kernel must ignore).  -> the return code (check=False) or the fp32 L2 value as a numpy array
    (want_l2) or None."""
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
    rc = lib.xdfm_rowwise_adagrad_step(a, T, lr, dev_p, eps, ws, out, R._stream())
    if not check:
        R._torch().cuda.synchronize()
        bank.check_guards("refused step")
        return rc
    _lib.check(rc, "rowwise_adagrad_step")
    bank.check_guards("rowwise step")                  # synchronises
    return bank.l2_value.cpu().numpy().copy() if want_l2 else None
