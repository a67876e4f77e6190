"""Generator of tests/golden/sweep_pinned.json: SHA-256 digests of everything the table optimizers' sweeps (K7, K7s / K7g / K7r /
K7m, K7f, K7w) write, at the smallest shapes at which every loop of the sweep runs.  tests/test_gpu_sweep_pinned.py recomputes
`compute()` and compares; the JSON was recorded once, before csrc/table_step.h took the sweep over, and is not regenerated when a
kernel is edited: a digest that moves means the edit changed a result bit.

Every case drives the C ABI through the drivers of tests/{opt,sgdm,ftrl,rowwise,adam}_ref.py for 3 consecutive steps on inputs
from fixed seeds and records the digest of the inputs and of p, every state array, the gradient, the marks, the L2 partials up to
the step's block count and the L2 value afterwards; every array a kernel writes lies between guard cells, which are checked
after the steps (the L2 workspace and the clock of the Adam cases are adam_ref's own allocations).
Run on the GPU:  python tests/golden/make_sweep_pinned.py"""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, ROOT, os.path.join(ROOT, "xdeepfm-pytorch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import adam_ref as A  # noqa: E402
import ftrl_ref as F  # noqa: E402
import opt_ref as R  # noqa: E402
import rowwise_ref as W  # noqa: E402
import sgdm_ref as M  # noqa: E402

JSON = os.path.join(HERE, "sweep_pinned.json")
F32 = np.float32
STEPS = 3
# 17 587 = 4 * 4396 + 3: in one 256-thread block two NF = 8 (four NF = 4) unrolled iterations plus a remainder, a numel % 4 tail,
# and -- behind the 20-element tensor that only shifts the mark pointer to 5 bytes past a 16-byte boundary -- a scan with a head
# of 11 chunks, 274 groups (the paired loop and the unpaired group) and a tail of one chunk; 3 blocks at the built-in cap
BASE = [20, 17587]
L2 = 1e-3
FAMILIES = ("sgd", "adagrad", "rmsprop", "sgdm", "nesterov", "ftrl", "adam")
VARIANTS = ("dense", "marks", "marks_l2", "lr_dev")
SIZES_66 = [5 + (37 * k) % 596 for k in range(65)] + [600]


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%r" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _host(t):
    return t.detach().cpu().numpy().copy()


@contextlib.contextmanager
def _option(name, value):
    from xdfm_amd import _lib
    before = _lib.get_option(name)
    _lib.set_option(name, value)
    try:
        yield
    finally:
        _lib.set_option(name, before)


def _blocks(sizes, bx):
    """Blocks (= L2 slots) of a step over `sizes` as tbl_grid deals them: one per 8192 elements (OPT_ / FTRL_ / ROW_ /
    ADAM_BLOCK_ELEMS in csrc/), at least 1, at most 512 (OPT_BX, FTRL_BX, ROW_BX, ADAM_BX) or the option's cap.  If one of those
    constants changes, this changes with it: a wrong count hashes the wrong slots and reads as moved kernels."""
    cap = bx if 0 < bx < 512 else 512
    return sum(min(cap, max(1, -(-n // 8192))) for n in sizes)


class _AdamBank(A.Bank):
    """adam_ref.Bank (its descriptors and accessors, arrays of the same lengths) with every array between two guards of
    opt_ref.GUARD bytes, as opt_ref.Bank keeps its own; check_guards() after the steps."""

    def __init__(self, state, dev, mis=None):
        import torch
        mis = mis or {}
        self.dev, self.sizes, self._guards = dev, [s[0].size for s in state], []
        self.p = [self._new(s[0].size, torch.float32, mis.get("p", 0), s[0]) for s in state]
        self.m = [self._new(s[1].size, torch.float32, mis.get("m", 0), s[1]) for s in state]
        self.v = [self._new(s[2].size, torch.float32, mis.get("v", 0), s[2]) for s in state]
        self.goff, total = A.grad_offsets(self.sizes)
        self.gshift = 0
        self.gbuf = self.flat = self._new(total, torch.float32)
        self.marks = self._new(total // 4 + 16, torch.uint8)
        self.steps = self._new(len(state), torch.float32)
        self.last = [self._new(n // 4 + 8, torch.uint8) for n in self.sizes]
        self.lr_dev = torch.zeros(1, dtype=torch.float64, device=dev)
        self.l2_value = self._new(1, torch.float32)
        assert self.marks.data_ptr() % 16 == 0 and self.flat.data_ptr() % 16 == 0

    def _new(self, n, dtype, off=0, init=None):
        """n zeroed elements (or the array `init`), `off` floats past a 16-byte boundary, between two guards"""
        import torch
        size = torch.empty((), dtype=dtype).element_size()
        buf = torch.full((2 * R.GUARD + 16 + n * size,), R.SENT, dtype=torch.uint8, device=self.dev)
        lo, hi = R.GUARD + 4 * off, R.GUARD + 4 * off + n * size
        view = buf[lo:hi].view(dtype)
        view.zero_()
        if init is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init)))
        assert view.data_ptr() % 16 == (4 * off) % 16
        self._guards += [buf[:lo], buf[hi:]]
        return view

    def check_guards(self, what=""):
        import torch
        torch.cuda.synchronize()
        assert not bool((torch.cat(self._guards) != R.SENT).any()), "a guard cell was written to (%s)" % what


class _Family:
    """One optimizer: its starting state, its bank on the device and one step through the C ABI."""

    def __init__(self, name):
        self.name = name
        self.kind = {"nesterov": "sgdm"}.get(name, name)
        self.option = "adam_bx" if name == "adam" else "opt_bx"
        if self.kind in R.KINDS:
            self.h = R.hyper(self.kind, "base")
        elif self.kind == "sgdm":
            self.h = M.HYPER["M1" if name == "nesterov" else "M0"]
        elif self.kind == "ftrl":
            self.h = F.HYPER["F1"]

    def state(self, sizes):
        if self.kind in R.KINDS:
            return R.make_state(self.h, sizes, seed=21)
        if self.kind == "sgdm":
            return M.make_state(sizes, seed=21, aligned=False)
        if self.kind == "ftrl":
            return F.make_state(self.h, sizes, seed=21, aligned=False)
        return A.make_state(sizes, seed=21)

    def bank(self, state, dev, mis=None):
        if self.kind in R.KINDS or self.kind == "sgdm":
            return R.Bank(self.kind, state, dev, mis=mis)
        if self.kind == "ftrl":
            return F.Bank(state, dev, mis=mis)
        return _AdamBank(state, dev, mis=mis)

    def lr(self, step, lr_dev):
        base = 1e-3 if self.kind == "adam" else self.h["lr"]
        return base * (1.0 + 0.03125 * step) if lr_dev else base

    def step(self, bank, idx, l2, step, lr_dev, marked, flags=None, clk=None):
        """-> the L2 partials of the call, as a device tensor"""
        if self.kind == "adam":
            # adam_ref takes the rate from its sets: H0 (1e-3 as an argument), H4 (1e-3 through the device scalar from step 4 on)
            A.adam_step(bank, idx, l2, "H4" if lr_dev else "H0", step + 3, marked=marked, flags=flags, want_l2=True, clk=clk)
            return bank.ws
        lr = self.lr(step, lr_dev)
        if self.kind in R.KINDS:
            R.opt_step(bank, idx, l2, self.h, lr, lr_dev=lr_dev, marked=marked, want_l2=True)
        elif self.kind == "sgdm":
            M.sgdm_step(bank, idx, l2, self.h, lr, lr_dev=lr_dev, marked=marked, want_l2=True)
        else:
            F.ftrl_step(bank, idx, l2, self.h, lr, lr_dev=lr_dev, marked=marked, want_l2=True)
        return bank.ws

    def arrays(self, bank, idx):
        """name -> device tensors of everything a step may write, beside the L2 partials"""
        out = {"p": [bank.p[t] for t in idx], "grad": [bank.flat], "marks": [bank.marks], "l2_value": [bank.l2_value]}
        if self.kind == "adam":
            out["m"], out["v"] = [bank.m[t] for t in idx], [bank.v[t] for t in idx]
            out["last"] = [bank.last[t] for t in idx]
        elif self.kind == "ftrl":
            out["z"], out["n"] = [bank.z[t] for t in idx], [bank.n[t] for t in idx]
        elif self.kind != "sgd":
            out["s"] = [bank.s[t] for t in idx]
        return out


def _sweep(fam, dev, sizes, idx, l2, bx, marked=False, lr_dev=False, mis=None, flags=None, clock=False):
    """STEPS steps of `fam` over the tensors `idx` of a fresh bank -> {"inputs": digest, name: digest of what the steps left}."""
    import torch
    state = fam.state(sizes)
    inputs = [a for s in state for a in s]
    bank = fam.bank(state, dev, mis=mis)
    clk = A.Clock(dev, cap=16) if clock else None
    kinds = ["none" if t not in idx else "random3" for t in range(len(sizes))]
    parts = None
    with _option(fam.option, bx):
        for s in range(1, STEPS + 1):
            if marked:
                flat, marks, _, _ = R.sparse_grads(sizes, kinds, s, seed=23)
            else:
                flat, _ = R.dense_grads(sizes, s, seed=23)
                marks = np.zeros(flat.size // 4, np.uint8)
            inputs += [flat, marks]
            bank.set_grads(flat, marks)
            parts = fam.step(bank, idx, l2, s, lr_dev, marked, flags=flags, clk=clk)
    bank.check_guards(fam.name)                        # synchronises
    out = {k: _sha([_host(x) for x in v]) for k, v in fam.arrays(bank, idx).items()}
    out["l2_ws"] = _sha([_host(parts[:_blocks([sizes[t] for t in idx], bx)])])
    if clk is not None:
        out["clock"] = _sha([_host(clk.clock), _host(clk.consts), _host(clk.backlog)])
    out["inputs"] = _sha(inputs)
    return out


def _colaunch(dev):
    """Adam: xdfm_colaunch_adam_step on a 2-field gather at B = 64, D = 8.  The second field's table goes by rows, the first's by
    the step's mark scan, one dense tensor rides along."""
    import torch
    from xdfm_amd import _lib
    lib = _lib.load()
    B, D, vocab_h, cols_h, ldx = 64, 8, [40, 500], [1, 3], 5
    sizes = [V * D for V in vocab_h] + [4099]
    l2 = [1e-3, 2e-3, 1e-3]
    state = A.make_state(sizes, seed=21)
    inputs = [a for s in state for a in s]
    bank = _AdamBank(state, dev)
    clk = A.Clock(dev, cap=16)
    emb = A.Rows(bank, [0, 1], l2[:2], skip=(0,))
    cols = torch.tensor(cols_h, dtype=torch.int32, device=dev)
    vocab = torch.tensor(vocab_h, dtype=torch.int32, device=dev)
    others, marked, flags = [0, 2], [True, False], [A.DEFERRED, 0]
    lr, b1, b2, eps = A.HYPER["H0"]
    with _option("colaunch", 1):
        for s in range(1, STEPS + 1):
            rng = np.random.RandomState(7000 + s)
            Xn = rng.rand(B, ldx).astype(F32)
            masks = []
            for f, V in enumerate(vocab_h):
                top = V if s == STEPS else V // 2          # the last step reaches rows that are two steps behind
                ids = np.minimum((top * rng.rand(B) ** 2).astype(np.int64), top - 1)
                Xn[:, cols_h[f]] = ids.astype(F32)
                mk = np.zeros(sizes[f] // 4, dtype=bool)
                for i in np.unique(ids):
                    mk[i * D // 4:(i * D + D - 1) // 4 + 1] = True
                masks.append(mk)
            masks.append(np.ones(sizes[2] // 4, dtype=bool))
            flat, marks, _, offs = A.sparse_grads(sizes, None, s, seed=29, chunks=masks)
            marks[offs[2] // 4:offs[2] // 4 + sizes[2] // 4 + 1] = 0      # the dense tensor is read in full, without marks
            inputs += [Xn, flat, marks]
            X = torch.from_numpy(Xn).to(dev)
            bank.set_grads(flat, marks)
            bank.steps += 1.0
            arr = bank.descriptors(others, [l2[t] for t in others], marked, flags)
            bank.ws = torch.zeros(lib.xdfm_adam_step_ws_elems(len(others)), dtype=torch.float32, device=dev)
            _lib.check(lib.xdfm_colaunch_adam_step(
                ctypes.cast(arr, ctypes.c_void_p), len(others), ctypes.byref(clk.struct), lr, None, b1, b2, eps,
                ctypes.c_void_p(bank.ws.data_ptr()), ctypes.c_void_p(bank.l2_value.data_ptr()),
                ctypes.c_void_p(X.data_ptr()), X.stride(0), X.shape[0], ctypes.c_void_p(cols.data_ptr()),
                ctypes.c_void_p(vocab.data_ptr()), 2, D, ctypes.byref(emb.struct), None,
                ctypes.c_void_p(clk.cell.data_ptr()), A._stream()), "colaunch_adam_step")
            assert _lib.get_option("last_colaunch") == 1
    bank.check_guards("colaunch")                      # synchronises
    fam = _Family("adam")
    out = {k: _sha([_host(x) for x in v]) for k, v in fam.arrays(bank, [0, 1, 2]).items()}
    out["l2_ws"] = _sha([_host(bank.ws[:_blocks([sizes[t] for t in others], 0)])])
    out["clock"] = _sha([_host(clk.clock), _host(clk.consts), _host(clk.backlog), _host(clk.cell)])
    out["inputs"] = _sha(inputs)
    return out


def _rowwise(dev, rows, D, marked, l2m):
    """K7w on one [rows, D] tensor: dense, or with the rows 3 % of a batch touched marked."""
    import torch
    rng = np.random.RandomState(31)
    p = (rng.randn(rows, D) * 0.05).astype(F32)
    s = (rng.rand(rows) * 1e-4).astype(F32)
    bank = W.Bank([(p, s)], dev)
    inputs = [p, s]
    _, total = R.grad_offsets([rows * D])
    for st in range(1, STEPS + 1):
        g = (rng.randn(rows, D) * 0.1).astype(F32)
        g.reshape(-1)[::7] = 0.0
        flat, marks = np.zeros(total, F32), np.zeros(total // 4, np.uint8)
        if marked:
            k = rng.rand(rows) < 0.03
            g[~k] = 0.0
            marks[:rows * D // 4] = np.repeat(k, D).reshape(-1, 4).any(axis=1)
        flat[:rows * D] = g.ravel()
        inputs += [flat, marks]
        bank.set_grads(flat, marks)
        W.rw_step(bank, [0], [l2m], W.LR * (1.0 + 0.03125 * st), lr_dev=bool(st % 2), marked=marked, want_l2=True)
    torch.cuda.synchronize()
    out = {k: _sha([_host(x)]) for k, x in (("p", bank.p[0]), ("s", bank.s[0]), ("grad", bank.flat), ("marks", bank.marks),
                                            ("l2_value", bank.l2_value))}
    out["l2_ws"] = _sha([_host(bank.ws[:_blocks([rows * D], 0)])])
    out["inputs"] = _sha(inputs)
    return out


def cases():
    """name -> callable(dev) that runs the case and returns its digests"""
    out = {}
    for name in FAMILIES:
        fam = _Family(name)
        for bx in (1, 0):
            for v in VARIANTS:
                out["%s-%s-bx%d" % (name, v, bx)] = (
                    lambda dev, fam=fam, bx=bx, v=v: _sweep(fam, dev, BASE, [1], [0.0 if v == "marks" else L2], bx,
                                                            marked=v.startswith("marks"), lr_dev=v == "lr_dev"))
        # param 4 bytes off a 16-byte boundary: every element goes through the scalar loop
        out["%s-unaligned" % name] = lambda dev, fam=fam: _sweep(fam, dev, [1027], [0], [L2], 0, mis={"p": 1})
        # 66 tensors: two launches, the second with its slot0 offset
        out["%s-66" % name] = lambda dev, fam=fam: _sweep(
            fam, dev, SIZES_66, list(range(66)), [L2 * (1 + k % 5) if k % 3 else 0.0 for k in range(66)], 0)
    adam = _Family("adam")
    out["adam-lazy"] = lambda dev: _sweep(adam, dev, BASE, [1], [L2], 0, marked=True, flags=[A.LAZY])
    # the chunks a later step marks first are that many steps behind the clock: the replay loop runs
    out["adam-deferred"] = lambda dev: _sweep(adam, dev, BASE, [1], [L2], 0, marked=True, flags=[A.DEFERRED], clock=True)
    out["adam-colaunch"] = _colaunch
    out["rowwise-lanes"] = lambda dev: _rowwise(dev, 2200, 8, False, L2)
    out["rowwise-rows"] = lambda dev: _rowwise(dev, 2200, 8, True, 0.0)
    out["rowwise-units"] = lambda dev: _rowwise(dev, 2931, 6, False, L2)
    return out


def compute(dev, only=None):
    return {name: run(dev) for name, run in cases().items() if only is None or name in only}


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "the digests are recorded on the GPU"
    got = compute(torch.device("cuda:0"))
    with open(JSON, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(got), JSON))
