"""torch.autograd wrappers around the C ABI of libxdfm_hip.so.

PyTorch is plumbing here (device memory, the current HIP stream, the autograd tape); every
arithmetic step of the embedding gather and of the CIN stack runs in the hand-written kernels.
All ops require float32 CUDA (ROCm) tensors and raise otherwise -- there is no CPU path.
"""
import ctypes
import os

import numpy as np
from typing import List, Optional, Sequence

import torch

from . import _lib

ACT_CODES = {"linear": 0, "relu": 1, "sigmoid": 2}      # XDFM_ACT_* of include/xdfm.h

# bench.py sets this to a list to collect (name, algorithmic work, start event, end event) for each
# heavy launch; the events are recorded on torch's current stream, the one the kernels run on.
PROFILE = None


def _run(name, work, fn):
    if PROFILE is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn()
    e1.record()
    PROFILE.append((name, work, e0, e1))
    return rc


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# Finish batch (include/xdfm.h, xdfm_finish_batch_begin): inside the model's own train step the one-block finish launches of
# the backward, and those of the optimizer, are collected and run as one launch each.  A deferred finish reads its partials
# when the batch runs, long after the op that made them has returned and dropped its workspace: `finish_keep` holds those
# tensors until then (the caching allocator would hand their memory to the next op on the same stream).
FJ_ADD = 7                       # `kind` of xdfm_finish: out[0] = a[0] + b[0]
_FINISH_OPEN = False             # finish_batch_begin without its finish_batch_run yet
_FINISH_KEEP = None              # a list while the library records finishes for that batch


def finish_batch_begin():
    """Opens a batch on the current device (nothing opens with the option "finish_batch" at 0).  Pair with finish_batch_run."""
    global _FINISH_OPEN, _FINISH_KEEP
    lib = _lib.load()
    _lib.check(lib.xdfm_finish_batch_begin(), "finish_batch_begin")
    _FINISH_OPEN = True
    _FINISH_KEEP = [] if lib.xdfm_finish_batch_active() else None      # option at 0: nothing is recorded


def finish_batch_run(quiet=False):
    """Runs and closes the open batch (no-op without one); `quiet`: on an error path, never raises."""
    global _FINISH_OPEN, _FINISH_KEEP
    if not _FINISH_OPEN:
        return
    try:
        rc = _lib.load().xdfm_finish_batch_run(_stream())
        if not quiet:
            _lib.check(rc, "finish_batch_run")
            assert _lib.load().xdfm_rider_pending() == 0, "a rider job is pending at the end of a finish batch"
    except Exception:            # noqa: BLE001
        if not quiet:
            raise
    finally:
        _FINISH_OPEN, _FINISH_KEEP = False, None


# Rider scope (include/xdfm.h, xdfm_rider_begin; option "colaunch" bit 2): around the model's own backward the ordered sum of
# a CIN level's dW slabs is not launched by its dW call but rides on a later launch of the backward -- the next level's
# pre-pass, the embedding scatter behind level 0 -- and rider_flush issues what nobody carried.  The dW workspaces (they hold
# the slabs) of a scope stay alive until its flush.
_RIDER_KEEP = None               # list while a scope is open and records (option bit set), else None


def rider_begin():
    """Inside the scope a recorded level's dW is returned by CINStack.backward BEFORE the launch that writes it is issued (the
    carrying launch or rider_flush does that).  Nothing may read it until the flush: no tensor hook or retain_grad on a CIN
    weight, no accumulation into an existing `.grad` (the model's step leaves `.grad` None, so autograd only takes the
    tensor over)."""
    global _RIDER_KEEP
    lib = _lib.load()
    _lib.check(lib.xdfm_rider_begin(), "rider_begin")
    _RIDER_KEEP = [] if lib.xdfm_rider_active() else None


def rider_flush(quiet=False):
    """Issues the recorded jobs that no launch carried and closes the scope (no-op without one); `quiet`: never raises."""
    global _RIDER_KEEP
    try:
        rc = _lib.load().xdfm_rider_flush(_stream())
        if not quiet:
            _lib.check(rc, "rider_flush")
    finally:
        _RIDER_KEEP = None


def finish_batch_flush():
    """Runs what the open batch holds and opens the next one: before the host issues work that reads a deferred output."""
    if _FINISH_OPEN:
        finish_batch_run()
        finish_batch_begin()


def finish_active():
    """True when the library records the next finish instead of launching it: its output must not be read before
    finish_batch_run, its workspace goes to finish_keep."""
    return _FINISH_KEEP is not None and bool(_lib.load().xdfm_finish_batch_active())


def finish_add(a, b):
    """a + b where b may be a deferred output of the open batch (the step's total loss + the optimizer's L2 value): for two
    fp32 one-element tensors a job of that batch, run behind the finish that writes b -- the sum is then as deferred as b.
    Anything else: the batch is flushed and torch adds."""
    if finish_active() and a.numel() == 1 and b.numel() == 1 and a.dtype == b.dtype == torch.float32 and a.device == b.device:
        out = torch.empty(torch.broadcast_shapes(a.shape, b.shape), dtype=torch.float32, device=a.device)
        _lib.check(_lib.load().xdfm_finish(FJ_ADD, _ptr(a), _ptr(b), _ptr(out), None, None, 0, 0, 0, 0, _stream()), "finish add")
        finish_keep(a, b)
        return out
    finish_batch_flush()
    return a + b


def finish_keep(*tensors):
    if _FINISH_KEEP is not None:
        _FINISH_KEEP.extend(t for t in tensors if t is not None)


def _need_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(
            "xdfm: %s is on %s -- the xDeepFM hot path only runs on an MI355X through libxdfm_hip.so; "
            "there is no CPU fallback (the CPU restatement lives in oracle/ and is test-only)." % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("xdfm: %s must be float32, got %s" % (name, t.dtype))


def activation_code(name) -> int:
    key = name.lower() if isinstance(name, str) else name
    if key not in ACT_CODES:
        raise NotImplementedError("xdfm CIN kernels implement activation 'relu', 'linear' and 'sigmoid', got %r" % (name,))
    return ACT_CODES[key]


# --------------------------------------------------------------------------------------------- #
# embedding gather                                                                               #
# --------------------------------------------------------------------------------------------- #
class EmbedPlan:
    """Device-side metadata of one gather: which column of X feeds which table."""

    def __init__(self, sparse_cols: Sequence[int], vocab: Sequence[int], dense_cols: Sequence[int], emb_dim: int,
                 extra_fields: int = 0):
        self.m = len(sparse_cols)
        self.extra = int(extra_fields)     # field slots behind the sparse ones, filled by VarLenPool (0: K1's own layout)
        self.nd = len(dense_cols)
        self.D = int(emb_dim)
        self.sparse_cols = [int(c) for c in sparse_cols]
        self.vocab = [int(v) for v in vocab]
        self.dense_cols = [int(c) for c in dense_cols]
        self._dev = {}
        self._ptr_cache = {}
        self._off_cache = {}
        self.dp = None            # set by xdfm_amd.dist to exchange row gradients across ranks
        self.reg_defer = None     # (gscale, L2Plan) left by L2Reg.backward: table L2 gradient still owed
        self.stash = None         # list: gather backwards park their inputs here instead of scattering (split step)
        self.arena_on = False     # the model's train step sets this when its optimizer consumes marked gradients
        self._arenas = {}
        self.catchup = None       # set by optim.TableAdam (deferred update): brings the rows of X up to date before they are read
        self.last_gather = None   # (X, embedding tables, linear tables) of the latest gather: the rows a deferred update is keyed by
        self.varlen_req = None    # left by VarLenPool.backward when the pooled fields' table gradients wait for the exchange (dp)
        self.varlen_owners = None  # the parameters those gradients belong to: the F [V, D] tables, then the F [V, 1] tables

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            i32 = dict(dtype=torch.int32, device=device)
            self._dev[key] = (torch.tensor(self.sparse_cols, **i32), torch.tensor(self.vocab, **i32),
                              torch.tensor(self.dense_cols if self.nd else [0], **i32),
                              torch.zeros(1, **i32))
        return self._dev[key]

    def pointer_table(self, tensors: Sequence[torch.Tensor], tag: str):
        """int64 device array of base pointers (re-uploaded only when a pointer changed)."""
        ptrs = tuple(t.data_ptr() for t in tensors)
        hit = self._ptr_cache.get(tag)
        if hit is None or hit[0] != ptrs:
            hit = (ptrs, torch.tensor(ptrs, dtype=torch.int64, device=tensors[0].device))
            self._ptr_cache[tag] = hit
        return hit[1]

    def grad_layout(self, shapes, device):
        """Element offsets of every table gradient inside the flat gradient buffer (device int64)."""
        key = (tuple(shapes), str(device))
        hit = self._off_cache.get(key)
        if hit is None:
            sizes = [sh[0] * sh[1] for sh in shapes]
            offs, off = [], 0
            for n in sizes:                  # every gradient starts on a 16-byte boundary (K7's float4 path; marks)
                offs.append(off)
                off += (n + 3) // 4 * 4
            hit = (sizes, offs, off, torch.tensor(offs, dtype=torch.int64, device=device))
            self._off_cache[key] = hit
        return hit

    def arena(self, shapes, device):
        """The flat gradient buffer kept ACROSS steps (GradArena), or None when that mode is off."""
        if not self.arena_on or os.environ.get("XDFM_GRAD_ARENA", "1") == "0":
            return None
        key = (tuple(shapes), str(device))
        hit = self._arenas.get(key)
        if hit is None:
            _, _, total, _ = self.grad_layout(shapes, device)
            hit = self._arenas[key] = GradArena(total + max(self.nd, 1), device)
        return hit

    def arenas(self):
        return list(self._arenas.values())

    def check_ids(self, device) -> bool:
        """True when a gather since the last call saw an id outside [0, vocab) (syncs the stream)."""
        flag = self.on(device)[3]
        bad = bool(flag.item())
        flag.zero_()
        return bad


class GradArena:
    """Dense table gradients without the table-sized passes (`optim.zero_grad` of dense [V, D] grads).

    The reference's tables carry dense gradients (deepctr/inputs.py:168), all zeros except the <= B rows per table a
    batch touches; a step pays a table-sized zero fill and a table-sized gradient read in the optimizer for them.
    Here the flat gradient buffer lives across steps: the scatter marks the 16-byte chunks it adds to
    (`xdfm_embed_scatter_bwd_marked`), K7 reads only marked chunks and writes zeros back (`xdfm_adam_tensor.grad_marks`),
    so the buffer is clean again when the step ends.  `pending` = byte offsets of the views handed to autograd that
    no optimizer step has consumed yet; a scatter that finds leftovers (a step without K7, a gradient that autograd
    copied instead of adopting) clears everything the slow way first.  `EmbedPlan.arena_on` is raised by the model's
    own train step only (models.py::_own_step_scope): K7 never sees what other code adds to a gradient outside the
    marked chunks, so user-driven autograd loops get ordinary dense gradients.  Consequence worth knowing: after the
    model's own step the tables' `.grad` read zeros (they are views of this buffer)."""

    def __init__(self, numel, device):
        self.flat = torch.zeros(numel, dtype=torch.float32, device=device)
        self.marks = torch.zeros(numel // 4 + 2, dtype=torch.uint8, device=device)
        self.base, self.nbytes = self.flat.data_ptr(), numel * 4
        self.pending = set()
        self.full_clears = 0

    def begin(self):
        if self.pending:
            self.flat.zero_()
            self.marks.zero_()
            self.pending.clear()
            self.full_clears += 1

    def hand_out(self, views):
        for v in views:
            if v is not None:
                self.pending.add(v.data_ptr() - self.base)

    def marks_ptr(self, grad_ptr):
        """Address of the mark bytes of a gradient that is one of this arena's views (else None)."""
        off = grad_ptr - self.base
        if 0 <= off < self.nbytes and off % 16 == 0 and off in self.pending:
            return self.marks.data_ptr() + off // 16
        return None

    def consumed(self, grad_ptr):
        self.pending.discard(grad_ptr - self.base)


class EmbedGather(torch.autograd.Function):
    """X [B, cols] -> (emb_fm [m, B*D], dnn_in [B, m*D+nd], lin [B, 1]).

    replaces deepctr/models/basemodel.py:354-380 + :63-92 + deepctr/inputs.py:126-132."""

    @staticmethod
    def forward(ctx, X, dense_w, plan: EmbedPlan, has_lin: bool, *tables):
        _need_cuda(X, "X")
        lib = _lib.load()
        m, D, nd = plan.m, plan.D, plan.nd
        emb_tables = tables[:m]
        lin_tables = tables[m:2 * m] if has_lin else ()
        for t in tables:
            _need_cuda(t, "embedding table")
            if not t.is_contiguous():
                raise ValueError("xdfm: embedding tables must be contiguous")
        X = X.contiguous()
        B = X.shape[0]
        cols, vocab, dcols, flag = plan.on(X.device)
        mx = m + plan.extra                # with pooled variable-length fields behind the sparse ones (VarLenPool fills them)
        emb_fm = torch.empty((mx, B * D), dtype=torch.float32, device=X.device)
        dnn_in = torch.empty((B, mx * D + nd), dtype=torch.float32, device=X.device)
        lin = torch.empty((B, 1), dtype=torch.float32, device=X.device)
        plan.last_gather = (X, tuple(emb_tables), tuple(lin_tables))
        if plan.catchup is not None:
            plan.catchup(plan, X, emb_tables, lin_tables)
        tp = plan.pointer_table(emb_tables, "emb")
        lp = plan.pointer_table(lin_tables, "lin") if has_lin else None
        dw = dense_w.contiguous() if (dense_w is not None and nd > 0) else None
        # algorithmic bytes: X row + table rows (+ linear rows) + both outputs + logit
        nbytes = B * (4 * (m + nd) + m * (4 * D + (4 if has_lin else 0)) + 4 * m * D + 4 * (m * D + nd) + 4)
        if plan.extra == 0:
            _lib.check(_run("embed_gather_fwd[bytes]", nbytes, lambda: lib.xdfm_embed_gather_fwd(
                _ptr(X), X.stride(0), B, _ptr(tp), _ptr(lp), _ptr(cols), _ptr(vocab), m, D,
                _ptr(dcols) if nd else None, _ptr(dw), nd, _ptr(emb_fm), _ptr(dnn_in), _ptr(lin), _ptr(flag),
                _stream())), "embed_gather_fwd")
        else:
            _lib.check(_run("embed_gather_fwd[bytes]", nbytes, lambda: lib.xdfm_embed_gather_fwd_ld(
                _ptr(X), X.stride(0), B, _ptr(tp), _ptr(lp), _ptr(cols), _ptr(vocab), m, D,
                _ptr(dcols) if nd else None, _ptr(dw), nd, _ptr(emb_fm), _ptr(dnn_in), mx * D + nd, mx * D, _ptr(lin),
                _ptr(flag), _stream())), "embed_gather_fwd")
        plan.reg_defer = None      # a deferral is only valid between this forward and its backward
        ctx.plan, ctx.has_lin = plan, has_lin
        ctx.shapes = [tuple(t.shape) for t in tables]
        ctx.save_for_backward(X, *tables)
        return emb_fm, dnn_in, lin

    @staticmethod
    def backward(ctx, d_emb, d_dnn, d_lin):
        X = ctx.saved_tensors[0]
        tables = ctx.saved_tensors[1:]
        plan = ctx.plan
        varlen, plan.varlen_req = plan.varlen_req, None      # VarLenPool.backward ran just before: its fields ride on our exchange
        if plan.stash is not None:
            # split step (row-parallel run replayed from a HIP graph): the scatter needs the other ranks' rows, so
            # it runs after the exchange, outside the captured part -- see apply_stashed_scatter
            plan.stash.append((plan, X, d_emb, d_dnn, d_lin, ctx.has_lin, ctx.shapes, tables, ctx.needs_input_grad[1], varlen))
            return (None, None, None, None) + (None,) * len(tables)
        need_w = ctx.needs_input_grad[1]
        grads, d_w, vgrads = EmbedGather.scatter(plan, X, d_emb, d_dnn, d_lin, ctx.has_lin, ctx.shapes, tables, need_w, varlen)
        if vgrads is not None:
            # those tables are no inputs of this node: their gradients are accumulated the way AccumulateGrad would
            for p, g in _varlen_owned(plan, varlen, vgrads):
                p.grad = g if p.grad is None else p.grad + g
        return (None, d_w if (need_w and plan.nd) else None, None, None) + tuple(grads)

    @staticmethod
    def scatter(plan, X, d_emb, d_dnn, d_lin, has_lin, shapes, tables, need_w=True, varlen=None):
        """Dense table gradients (views of one flat buffer) and the dense-weight gradient from the row gradients; third,
        the table gradients of the pooled variable-length fields when their backward left a request (`varlen`, row-parallel
        only: K2v runs once over the same exchanged rows), else None."""
        lib = _lib.load()
        m, D, nd = plan.m, plan.D, plan.nd
        dev = X.device
        sizes, offs, total, off_dev = plan.grad_layout(shapes, dev)
        # ONE buffer holds every dense table gradient (+ the dense-weight gradient at its end).  It
        # starts as zeros, or -- when L2Reg.backward deferred the tables' L2 term to us -- as
        # 2*l2*gscale*w, which saves a memset, a table-sized temporary and one add per table.
        defer, plan.reg_defer = plan.reg_defer, None
        arena = plan.arena(shapes, dev) if plan.arena_on and defer is None and all(t.grad is None for t in tables) else None
        marks = None
        if arena is not None:
            arena.begin()
            flat, marks = arena.flat, arena.marks
        elif defer is not None:
            gscale, l2plan = defer
            flat = torch.empty(total + max(nd, 1), dtype=torch.float32, device=dev)
            flat[total:].zero_()
            ptrs, numel, coeff = l2plan.tables(tables)
            _lib.check(lib.xdfm_l2_reg_bwd(_ptr(ptrs), _ptr(numel), _ptr(coeff), len(tables), _ptr(gscale),
                                           _ptr(flat), _ptr(off_dev), 0, _stream()), "l2_reg_bwd (deferred)")
        else:
            flat = torch.zeros(total + max(nd, 1), dtype=torch.float32, device=dev)
        grads = [flat[o:o + n].view(sh) for o, n, sh in zip(offs, sizes, shapes)]
        d_w = flat[total:total + nd].view(nd, 1) if nd else None
        if arena is not None:
            arena.hand_out(grads + ([d_w] if need_w else []))
        cols, vocab, dcols, _ = plan.on(dev)
        tab_off = off_dev[:m]
        lin_off = off_dev[m:2 * m] if has_lin else None
        pieces = [(X, d_emb, d_dnn, d_lin)]
        if plan.dp is not None:
            pieces = plan.dp.exchange_rows(X, d_emb, d_dnn, d_lin)
        elif varlen is not None:
            raise RuntimeError("xdfm: the variable-length fields wait for a row exchange that this gather does not make")
        vgrads = None
        for (Xr, de, dd, dl) in pieces:
            B = Xr.shape[0]
            # the exchange hands over strided views of one gathered buffer: rows may be wider than their payload
            de = de.contiguous() if de is not None else None
            if dd is not None and dd.stride(-1) != 1:
                dd = dd.contiguous()
            dl = dl.reshape(B) if dl is not None else None
            ld_dnn = dd.stride(0) if dd is not None else 0
            ld_lin = dl.stride(0) if dl is not None and B > 1 else (1 if dl is not None else 0)
            nbytes = B * (4 * (m + nd) + 2 * 4 * m * D + 4 + 4 * m * (D + 1))
            _lib.check(_run("embed_scatter_bwd[bytes]", nbytes, lambda: lib.xdfm_embed_scatter_bwd_marked(
                _ptr(Xr), Xr.stride(0), B, _ptr(cols), _ptr(vocab), m, D, _ptr(dcols) if nd else None, nd,
                _ptr(de), _ptr(dd), ld_dnn, _ptr(dl), ld_lin, _ptr(flat), _ptr(tab_off), _ptr(lin_off), _ptr(d_w),
                _ptr(marks), _stream())), "embed_scatter_bwd")
            if varlen is not None:
                vgrads = varlen_rows_grads(varlen, Xr, dd, dl, ld_lin)
        return grads, d_w, vgrads


# --------------------------------------------------------------------------------------------- #
# pooled variable-length fields                                                                  #
# --------------------------------------------------------------------------------------------- #
POOL_CODES = {"sum": 0, "mean": 1, "max": 2}


class VarLenPlan:
    """Metadata of the pooled variable-length fields of one model: per field the first id column of X, maxlen, the
    length column (None: mask = id != 0), the combiner and the vocabulary size.  The device descriptors
    (xdfm_varlen_field) are built once per set of table addresses, never per step."""

    def __init__(self, cols: Sequence[int], maxlens: Sequence[int], len_cols, combiners: Sequence[str], vocab: Sequence[int],
                 emb_dim: int, slot0: int = 0, dnn_off: int = 0):
        self.F = len(cols)
        self.D = int(emb_dim)
        self.slot0, self.dnn_off = int(slot0), int(dnn_off)
        self.cols = [int(c) for c in cols]
        self.maxlens = [int(t) for t in maxlens]
        self.len_cols = [-1 if c is None else int(c) for c in len_cols]
        self.vocab = [int(v) for v in vocab]
        for t in self.maxlens:
            if not 1 <= t <= 255:
                raise ValueError("VarLenSparseFeat: maxlen must lie in 1..255, got %d" % t)
        for c in combiners:
            if c not in POOL_CODES:
                raise ValueError("VarLenSparseFeat: combiner must be one of sum, mean, max, got %r" % (c,))
        self.combiners = [POOL_CODES[c] for c in combiners]
        self.Tmax = max(self.maxlens)
        self.min_cols = max([c + t for c, t in zip(self.cols, self.maxlens)] + [c + 1 for c in self.len_cols])
        self._dev = {}
        self._desc = {}
        self._off_cache = {}
        self.gather = None        # row-parallel: the EmbedPlan whose row exchange carries these fields' ids and row gradients

    def exchanged(self):
        """True when the table gradients are built from all ranks' rows after the gather's exchange (xdfm_amd.dist)."""
        return self.gather is not None and self.gather.dp is not None

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            i32 = dict(dtype=torch.int32, device=device)
            self._dev[key] = (torch.arange(self.F, **i32), torch.tensor(self.vocab, **i32), torch.zeros(1, **i32))
        return self._dev[key]

    def descriptors(self, emb_tables, lin_tables, device):
        """(host array, device copy) of the field descriptors; re-uploaded only when a table address changed."""
        key = (tuple(t.data_ptr() for t in emb_tables), tuple(t.data_ptr() for t in lin_tables), str(device))
        hit = self._desc.get(key)
        if hit is None:
            host = (_lib.VarLenField * self.F)()
            for f in range(self.F):
                host[f].table = emb_tables[f].data_ptr() if emb_tables else None
                host[f].lin = lin_tables[f].data_ptr() if lin_tables else None
                host[f].col, host[f].maxlen, host[f].len_col = self.cols[f], self.maxlens[f], self.len_cols[f]
                host[f].combiner, host[f].vocab = self.combiners[f], self.vocab[f]
            dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device)
            self._desc.clear()                 # one live set of addresses per plan
            hit = self._desc[key] = (host, dev)
        return hit

    def grad_layout(self, shapes, device):
        """Element offsets of every table gradient inside one flat buffer, each on a 16-byte boundary (device int64)."""
        key = (tuple(shapes), str(device))
        hit = self._off_cache.get(key)
        if hit is None:
            sizes = [sh[0] * sh[1] for sh in shapes]
            offs, off = [], 0
            for n in sizes:
                offs.append(off)
                off += (n + 3) // 4 * 4
            hit = self._off_cache[key] = (sizes, offs, off, torch.tensor(offs if offs else [0], dtype=torch.int64, device=device))
        return hit

    def check_ids(self, device) -> bool:
        """True when a pooled lookup since the last call saw an id outside [0, vocab) (syncs the stream)."""
        flag = self.on(device)[2]
        bad = bool(flag.item())
        flag.zero_()
        return bad


class VarLenPool(torch.autograd.Function):
    """Pools the variable-length fields of X into the outputs of EmbedGather, in place: field f goes to slot
    plan.slot0 + f of emb_fm, to columns plan.dnn_off + f*D of dnn_in, and its pooled [V, 1] row is added to lin (any of
    the three may be None).  `tables` = the F [V, D] tables (n_emb == F, or none with n_emb == 0), then the F [V, 1]
    tables when lin is given.  The table gradients are ordinary dense tensors (views of one zero-filled buffer).

    replaces deepctr/inputs.py:141-155 + :213-227 + deepctr/layers/sequence.py:49-77."""

    @staticmethod
    def forward(ctx, X, emb_fm, dnn_in, lin, plan: VarLenPlan, n_emb: int, *tables):
        _need_cuda(X, "X")
        lib = _lib.load()
        F, D = plan.F, plan.D
        emb_tables = tables[:n_emb]
        lin_tables = tables[n_emb:]
        if n_emb not in (0, F) or len(lin_tables) not in (0, F) or (lin is not None) != (len(lin_tables) == F) or \
                ((emb_fm is not None or dnn_in is not None) != (n_emb == F)):
            raise ValueError("xdfm: VarLenPool needs one [V, D] table per field for emb_fm / dnn_in and one [V, 1] table per field for lin")
        for t in tables:
            _need_cuda(t, "embedding table")
            if not t.is_contiguous():
                raise ValueError("xdfm: embedding tables must be contiguous")
        for t, d in zip(emb_tables, [D] * F):
            if t.shape[1] != d:
                raise ValueError("xdfm: embedding_dim of a VarLenSparseFeat table is %d, the plan's is %d" % (t.shape[1], d))
        X = X.contiguous()
        B = X.shape[0]
        if X.shape[1] < plan.min_cols:
            raise ValueError("xdfm: X has %d columns, the variable-length fields need %d" % (X.shape[1], plan.min_cols))
        N = B * D
        if emb_fm is not None and not (emb_fm.is_contiguous() and emb_fm.shape[0] >= plan.slot0 + F and emb_fm.shape[1] == N):
            raise ValueError("xdfm: VarLenPool: emb_fm must be contiguous [>= slot0 + F, B*D]")
        if dnn_in is not None and not (dnn_in.stride(1) == 1 and dnn_in.shape[0] == B and dnn_in.shape[1] >= plan.dnn_off + F * D):
            raise ValueError("xdfm: VarLenPool: dnn_in must be [B, >= dnn_off + F*D] with unit column stride")
        if lin is not None and not (lin.is_contiguous() and lin.numel() == B):
            raise ValueError("xdfm: VarLenPool: lin must be contiguous [B, 1]")
        _, _, flag = plan.on(X.device)
        host, dev = plan.descriptors(emb_tables, lin_tables, X.device)
        # row-parallel: the backward runs over all ranks' rows and recomputes the positions of the maxima itself
        argpos = None if plan.exchanged() else torch.empty((B, F, D + 1), dtype=torch.uint8, device=X.device)
        # algorithmic bytes: ids + the looked-up rows (+ linear rows) + the pooled rows to both consumers
        T = sum(plan.maxlens)
        nbytes = B * (4 * T + T * ((4 * D if n_emb else 0) + (4 if lin_tables else 0)) + 2 * 4 * F * D)
        _lib.check(_run("varlen_pool_fwd[bytes]", nbytes, lambda: lib.xdfm_varlen_pool_fwd(
            _ptr(X), X.stride(0), B, _ptr(dev), ctypes.cast(host, ctypes.c_void_p), F, D, plan.slot0, _ptr(emb_fm), _ptr(dnn_in),
            dnn_in.stride(0) if dnn_in is not None else 0, plan.dnn_off, _ptr(lin), _ptr(argpos), _ptr(flag), _stream())),
            "varlen_pool_fwd")
        dirty = [t for t in (emb_fm, dnn_in, lin) if t is not None]
        ctx.mark_dirty(*dirty)
        ctx.plan, ctx.n_emb, ctx.n_lin = plan, n_emb, len(lin_tables)
        ctx.shapes = [tuple(t.shape) for t in tables]
        ctx.desc = (host, dev)
        ctx.exchanged = argpos is None
        ctx.save_for_backward(X, argpos)
        return emb_fm, dnn_in, lin

    @staticmethod
    def backward(ctx, d_emb, d_dnn, d_lin):
        X, argpos = ctx.saved_tensors
        plan = ctx.plan
        lib = _lib.load()
        F, D = plan.F, plan.D
        need = ctx.needs_input_grad[6:]
        grads = [None] * len(ctx.shapes)
        if ctx.exchanged:
            # row-parallel: no local table gradients.  The gather's backward, which runs next, takes this request along to
            # its row exchange (EmbedGather.scatter -> varlen_rows_grads); d_emb / d_dnn / d_lin go on to it unchanged.
            if any(need):
                if ctx.n_emb != F or ctx.n_lin != F:
                    raise RuntimeError("xdfm: row-parallel VarLenPool needs the [V, D] and the [V, 1] tables of every field")
                plan.gather.varlen_req = (plan, ctx.desc, ctx.shapes, tuple(need))
        elif any(need):
            dev = X.device
            B = X.shape[0]
            sizes, offs, total, off_dev = plan.grad_layout(ctx.shapes, dev)
            flat = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
            grads = [flat[o:o + n].view(sh) for o, n, sh in zip(offs, sizes, ctx.shapes)]
            cols, vocab, _ = plan.on(dev)
            host, desc = ctx.desc
            de = d_emb.contiguous() if d_emb is not None else None
            dd = d_dnn if (d_dnn is None or d_dnn.stride(1) == 1) else d_dnn.contiguous()
            dl = d_lin.reshape(B) if d_lin is not None else None
            ld_lin = dl.stride(0) if dl is not None and B > 1 else 1
            ws = torch.empty(lib.xdfm_varlen_pool_bwd_ws_elems(B, F, D, plan.Tmax), dtype=torch.float32, device=dev)
            tab_off = off_dev[:F] if ctx.n_emb else None
            lin_off = off_dev[ctx.n_emb:ctx.n_emb + F] if ctx.n_lin else None
            P = B * plan.Tmax
            nbytes = 4 * P * F * ((D if ctx.n_emb else 0) + (1 if ctx.n_lin else 0) + 1) * 2
            _lib.check(_run("varlen_pool_bwd[bytes]", nbytes, lambda: lib.xdfm_varlen_pool_bwd(
                _ptr(X), X.stride(0), B, _ptr(desc), ctypes.cast(host, ctypes.c_void_p), F, D, plan.slot0, _ptr(de), _ptr(dd),
                dd.stride(0) if dd is not None else 0, plan.dnn_off, _ptr(dl), ld_lin, _ptr(argpos), _ptr(cols), _ptr(vocab),
                _ptr(flat), _ptr(tab_off), _ptr(lin_off), _ptr(ws), _stream())), "varlen_pool_bwd")
            grads = [g if n else None for g, n in zip(grads, need)]
        # the gradients of the three outputs go on to the gather unchanged: K2 reads its own fields' part of them
        return (None, d_emb, d_dnn, d_lin, None, None) + tuple(grads)


def varlen_rows_grads(req, Xr, G, dl, ld_lin):
    """K2v over exchanged rows: the dense gradients of the F [V, D] tables and the F [V, 1] tables of a VarLenPool whose
    backward left `req`, from strided views of the gathered buffer -- Xr [R, ncols], G [R, >= (slot0 + F) * D] (row
    gradients, example-major), dl [R].  One call; the positions of the maxima are recomputed from the tables, which are the
    same on every rank until the optimizer runs."""
    vplan, (host, desc), shapes, _ = req
    lib = _lib.load()
    F, D = vplan.F, vplan.D
    dev, R = Xr.device, Xr.shape[0]
    if G is None or dl is None or Xr.stride(1) != 1 or G.stride(1) != 1 or G.shape[1] < (vplan.slot0 + F) * D:
        raise RuntimeError("xdfm: the exchanged rows do not carry the variable-length fields' gradients")
    sizes, offs, total, off_dev = vplan.grad_layout(shapes, dev)
    flat = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
    cols, vocab, flag = vplan.on(dev)
    ws = torch.empty(lib.xdfm_varlen_pool_bwd_rows_ws_elems(R, F, D, vplan.Tmax), dtype=torch.float32, device=dev)
    P = R * vplan.Tmax
    nbytes = 4 * P * F * (D + 2) * 2
    _lib.check(_run("varlen_pool_bwd_rows[bytes]", nbytes, lambda: lib.xdfm_varlen_pool_bwd_rows(
        _ptr(Xr), Xr.stride(0), R, _ptr(desc), ctypes.cast(host, ctypes.c_void_p), F, D, vplan.slot0, _ptr(G), G.stride(0),
        _ptr(dl), ld_lin, _ptr(cols), _ptr(vocab), _ptr(flat), _ptr(off_dev[:F]), _ptr(off_dev[F:2 * F]), _ptr(ws), _ptr(flag),
        _stream())), "varlen_pool_bwd_rows")
    return [flat[o:o + n].view(sh) for o, n, sh in zip(offs, sizes, shapes)]


def _varlen_owned(plan, req, vgrads):
    """(parameter, gradient) of the variable-length tables that want one."""
    owners = plan.varlen_owners
    if owners is None or len(owners) != len(vgrads):
        raise RuntimeError("xdfm: EmbedPlan.varlen_owners must name the %d variable-length tables" % len(vgrads))
    return [(p, g) for p, g, n in zip(owners, vgrads, req[3]) if n]


def apply_stashed_scatter(stash, dense_w, params=None):
    """Second half of a split step: exchange + scatter for every stashed gather backward; the gradients are
    assigned to `.grad` of the tables (`params`: the model's own parameter objects, in the gather's order) and of
    `dense_w`, the linear part's dense weight, directly.  A gather whose pooled variable-length fields wait for the same
    exchange hands their table gradients over too: assigned to `.grad` of `plan.varlen_owners`."""
    with torch.no_grad():
        for (plan, X, d_emb, d_dnn, d_lin, has_lin, shapes, tables, need_w, varlen) in stash:
            grads, d_w, vgrads = EmbedGather.scatter(plan, X, d_emb, d_dnn, d_lin, has_lin, shapes, tables,
                                                     bool(need_w and dense_w is not None), varlen)
            if vgrads is not None:
                for p, g in _varlen_owned(plan, varlen, vgrads):
                    p.grad = g
            owners = params if params is not None and len(params) == len(tables) else tables
            for t, g in zip(owners, grads):
                t.grad = g
            if need_w and d_w is not None and dense_w is not None:
                dense_w.grad = d_w if plan.arena_on else d_w.clone()


# --------------------------------------------------------------------------------------------- #
# CIN stack                                                                                      #
# --------------------------------------------------------------------------------------------- #
def cin_geometry(m: int, layer_size: Sequence[int], split_half: bool):
    """Per level: (H, Hp, hid_rows, dir0, dir_rows, dir_off).  Mirrors field_nums of
    deepctr/layers/interaction.py:183-201 and the split of :231-240."""
    levels, Hp, off = [], m, 0
    L = len(layer_size)
    for i, H in enumerate(layer_size):
        if split_half:
            if i != L - 1:
                hid, dir0, drows = H // 2, H // 2, H - H // 2
            else:
                hid, dir0, drows = 0, 0, H
        else:
            hid, dir0, drows = H, 0, H
        levels.append((H, Hp, hid, dir0, drows, off))
        off += drows
        Hp = hid
    return levels, off


_FALLBACK_WARNED = set()


def _warn_if_fp32_fallback(what, probe, H, Hp, m):
    """cin_math 1 / 2 asked for the f16 / bf16 MFMA kernels; a level they do not cover (forward: odd or > 40 field
    count, or H <= 32 / 64 rows) runs in the fp32-MFMA kernel -- same results, about a third of the rate.  Said once
    per shape instead of silently (the library records the arithmetic of its last launch in the probe option)."""
    want = _lib.get_option("cin_math")
    if want == 0 or _lib.get_option(probe) == want:
        return
    key = (what, want, H, Hp, m)
    if key in _FALLBACK_WARNED:
        return
    _FALLBACK_WARNED.add(key)
    import warnings
    warnings.warn("xdfm: CIN %s level (H=%d, H_prev=%d, fields=%d) has no %s kernel; it runs in fp32-MFMA arithmetic"
                  % (what, H, Hp, m, "f16x3" if want == 1 else "bf16"), RuntimeWarning, stacklevel=3)


def cin_lean_allowed(act: int) -> bool:
    """Whether a CIN stack with this activation may run the lean levels (and with them the dX path that forms dOut from the
    sign bits): both keep 1 bit per element, the sign of a ReLU output (for `linear` the bits are written and never read).
    The sigmoid's derivative y (1 - y) needs the output itself, so its levels store full fp32 outputs and materialise
    dOut -- the path XDFM_CIN_LEAN=0 selects for the others."""
    return act != ACT_CODES["sigmoid"]


_PACK_ANNOUNCED = None           # (key, forward packs, dX packs, weights) of cin_announce_pack until the forward that takes it


def _cin_pack_key(W2s, levels, m):
    return (tuple((w.data_ptr(), w._version) for w in W2s), tuple((H, Hp) for (H, Hp, *_r) in levels), m, _lib.get_option("cin_math"))


def _cin_pack_jobs(lib, W2s, levels, m, need_bwd, dev):
    """(job array, forward packs, dX packs) of xdfm_cin_pack_all / _defer for the levels' weights [H, Hp * m]."""
    jobs = (_lib.PackJob * len(levels))()
    wfs, wzs = [None] * len(levels), [None] * len(levels)
    for l, (H, Hp, *_r) in enumerate(levels):
        wfs[l] = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        if need_bwd:
            wzs[l] = torch.empty(lib.xdfm_cin_bwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
        jobs[l].W, jobs[l].H, jobs[l].Hp, jobs[l].m = W2s[l].data_ptr(), H, Hp, m
        jobs[l].fwd_pack = wfs[l].data_ptr()
        jobs[l].bwd_pack = wzs[l].data_ptr() if need_bwd else None
    return jobs, wfs, wzs


def cin_announce_pack(weights, m, layer_size, split_half):
    """The model's train step, before its embedding gather: the packs CINStack.forward would launch for these weights are
    deferred (xdfm_cin_pack_defer; option "colaunch" bit 1), so that deferred Adam's catch-up carries the |W| maxima and the
    gather the packs; CINStack.forward then takes the buffers and issues what nobody carried.  Nothing happens where the
    forward would not pack all levels at once.  Pair with cin_pack_drop behind the forward."""
    global _PACK_ANNOUNCED
    cin_pack_drop()
    lib = _lib.load()
    levels, _ = cin_geometry(m, layer_size, split_half)
    if not weights or not weights[0].is_cuda or len(levels) > 8 or \
            not all(lib.xdfm_cin_pack_all_supported(H, Hp, m) for (H, Hp, *_r) in levels):
        return
    W2s = [w.detach().reshape(H, Hp * m).contiguous() for w, (H, Hp, *_r) in zip(weights, levels)]
    jobs, wfs, wzs = _cin_pack_jobs(lib, W2s, levels, m, True, W2s[0].device)
    _lib.check(lib.xdfm_cin_pack_defer(ctypes.cast(jobs, ctypes.c_void_p), len(levels), _stream()), "cin_pack_defer")
    _PACK_ANNOUNCED = (_cin_pack_key(W2s, levels, m), wfs, wzs, W2s)


def cin_pack_drop(quiet=False):
    """An announcement no forward took: its packs are issued (the buffers may be in use by a captured graph) and forgotten."""
    global _PACK_ANNOUNCED
    if _PACK_ANNOUNCED is None:
        return
    _PACK_ANNOUNCED = None
    rc = _lib.load().xdfm_cin_pack_flush(_stream())
    if not quiet:
        _lib.check(rc, "cin_pack_flush")


class CINStack(torch.autograd.Function):
    """All CIN levels.  x0 is FM layout [m, B*D].

    pool == "sum": returns [B, featuremap_num]   (deepctr/layers/interaction.py:207-248)
    pool == "fm" : returns the direct-connect feature maps, FM layout [featuremap_num, B*D]
                   (the tensor deepctr/layers/cin_attention.py:292 feeds to the attention block).
    """

    @staticmethod
    def forward(ctx, x0, B, D, layer_size, split_half, act, pool, *params):
        _need_cuda(x0, "cin input")
        lib = _lib.load()
        m = x0.shape[0]
        N = B * D
        assert x0.shape[1] == N and x0.is_contiguous()
        levels, fm = cin_geometry(m, layer_size, split_half)
        dev = x0.device
        outs: List[torch.Tensor] = []
        xp = x0
        result = torch.empty((B, fm), dtype=torch.float32, device=dev) if pool == "sum" else None
        # The packed weights depend on the weights only.  When every level runs the f16x3 kernels both ways, all
        # forward packs and (if a backward will follow) all dX packs are produced by two launches up front.
        W2s = []
        for l, (H, Hp, hid, dir0, drows, off) in enumerate(levels):
            _need_cuda(params[2 * l], "cin weight")
            W2s.append(params[2 * l].reshape(H, Hp * m).contiguous())
        wfs, wzs = [None] * len(levels), None
        global _PACK_ANNOUNCED
        ann, _PACK_ANNOUNCED = _PACK_ANNOUNCED, None
        if ann is not None:
            # packs announced before the gather (cin_announce_pack): the catch-up and the gather have carried them; what
            # they did not carry leaves now.  An announcement for other weights is issued all the same and not used.
            _lib.check(lib.xdfm_cin_pack_flush(_stream()), "cin_pack_flush")
        if ann is not None and ann[0] == _cin_pack_key(W2s, levels, m):
            wfs, wzs = ann[1], (ann[2] if any(ctx.needs_input_grad) else None)
        elif len(levels) <= 8 and all(lib.xdfm_cin_pack_all_supported(H, Hp, m) for (H, Hp, *_r) in levels):
            need_bwd = any(ctx.needs_input_grad)
            jobs, wfs, wzs = _cin_pack_jobs(lib, W2s, levels, m, need_bwd, dev)
            _lib.check(lib.xdfm_cin_pack_all(ctypes.cast(jobs, ctypes.c_void_p), len(levels), _stream()), "cin_pack_all")
            if not need_bwd:
                wzs = None
        # "lean" levels (sum pooling, f16x3 / bf16 forward, D in {4, 8, 16, 32}): the forward's epilogue sums the direct-connect
        # rows into `result` and leaves the ReLU sign bits, so only the hidden rows (the next level's x_prev) are ever
        # written -- no direct_sum launches, no direct-connect half in memory, and the backward reads 1 bit per element
        # instead of the saved output (xdfm_cin_level_fwd_ex / xdfm_cin_bwd_prep)
        lean = cin_lean_allowed(act) and pool == "sum" and os.environ.get("XDFM_CIN_LEAN", "1") != "0" and \
            all(lib.xdfm_cin_level_fwd_ex_supported(H, Hp, m, D) for (H, Hp, *_r) in levels)
        need_bwd = any(ctx.needs_input_grad)
        masks = []
        mask_chunks = (N + 31) // 32
        for l, (H, Hp, hid, dir0, drows, off) in enumerate(levels):
            W, bias = params[2 * l], params[2 * l + 1]
            W2 = W2s[l]
            wf = wfs[l]
            if wf is None:
                wf = torch.empty(lib.xdfm_cin_fwd_pack_elems(H, Hp, m), dtype=torch.float32, device=dev)
                _lib.check(lib.xdfm_cin_fwd_pack(_ptr(W2), H, Hp, m, _ptr(wf), _stream()), "cin_fwd_pack")
            bias_c = bias.contiguous()
            if lean:
                A = torch.empty((hid, N), dtype=torch.float32, device=dev) if hid > 0 else None
                mask_ld = (H + 3) // 4 * 4
                mk = torch.empty((mask_chunks, mask_ld), dtype=torch.int32, device=dev) if need_bwd else None    # [chunk][row]
                _lib.check(_run("cin_level_fwd", 2.0 * H * Hp * m * N, lambda: lib.xdfm_cin_level_fwd_ex(
                    _ptr(xp), _ptr(x0), _ptr(wf), _ptr(bias_c), H, Hp, m, N, act, _ptr(A), hid, _ptr(result), fm, off, dir0, D,
                    _ptr(mk), mask_ld, _stream())), "cin_level_fwd")
                masks.append(mk)
                outs.append(A if A is not None else x0[:0])      # a placeholder keeps the saved-tensor list regular
                xp = A
                continue
            A = torch.empty((H, N), dtype=torch.float32, device=dev)
            _lib.check(_run("cin_level_fwd", 2.0 * H * Hp * m * N, lambda: lib.xdfm_cin_level_fwd(
                _ptr(xp), _ptr(x0), _ptr(wf), _ptr(bias_c), H, Hp, m, N, act, _ptr(A), _stream())), "cin_level_fwd")
            _warn_if_fp32_fallback("forward", "last_fwd_kernel", H, Hp, m)
            if pool == "sum":
                _lib.check(lib.xdfm_cin_direct_sum(_ptr(A), dir0, drows, B, D, _ptr(result), fm, off, _stream()),
                           "cin_direct_sum")
            outs.append(A)
            xp = A[:hid] if hid > 0 else None
        ctx.cfg = (B, D, tuple(layer_size), split_half, act, pool, m)
        ctx.wzs = wzs                                # dX packs made up front (or None), arithmetic mode they belong to
        ctx.cin_math = _lib.get_option("cin_math")
        ctx.lean = lean and need_bwd
        if ctx.lean:
            ctx.save_for_backward(x0, *outs, *params, *masks)
        else:
            ctx.save_for_backward(x0, *outs, *params)
        if pool == "sum":
            return result
        return torch.cat([A[dir0:dir0 + drows] for A, (H, Hp, hid, dir0, drows, off) in zip(outs, levels)], dim=0)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        B, D, layer_size, split_half, act, pool, m = ctx.cfg
        L = len(layer_size)
        saved = ctx.saved_tensors
        x0, outs, params = saved[0], saved[1:1 + L], saved[1 + L:1 + 3 * L]
        masks = saved[1 + 3 * L:] if ctx.lean else None        # lean levels: outs[l] holds the hidden rows only, the ReLU mask is bits
        N = B * D
        dev = x0.device
        levels, fm = cin_geometry(m, layer_size, split_half)
        g = g.contiguous()
        dx0 = torch.empty((m, N), dtype=torch.float32, device=dev)      # first dX launch stores, later ones add
        dx0_set = False
        grads = [None] * (2 * L)
        dhid = None                                  # gradient w.r.t. this level's hidden rows
        # one fill for all levels; none inside a finish batch, whose dbias finish stores 0 + sum instead of adding
        dbias_all = (torch.empty if finish_active() else torch.zeros)(sum(lv[0] for lv in levels), dtype=torch.float32, device=dev)
        dbias_off = [sum(lv[0] for lv in levels[:k]) for k in range(L)]
        for l in range(L - 1, -1, -1):
            H, Hp, hid, dir0, drows, off = levels[l]
            A = None if ctx.lean else outs[l]
            xp = x0 if l == 0 else outs[l - 1][:levels[l - 1][2]]
            W, bias = params[2 * l], params[2 * l + 1]
            mk = masks[l] if ctx.lean else None
            # lean levels with f16x3 / bf16 dW and dX kernels: dOut is never materialised in fp32 -- the dW kernel takes its
            # fp16 planes, the dX kernel forms its operand from dOut's sources (sign bits, dhid, pooled gradient) itself
            no_dout = mk is not None and bool(lib.xdfm_cin_bwd_nodout_supported(H, Hp, m, B, D)) and \
                os.environ.get("XDFM_CIN_NODOUT", "1") != "0"
            dOut = None if no_dout else torch.empty((H, N), dtype=torch.float32, device=dev)
            dbias = dbias_all[dbias_off[l]:dbias_off[l] + H]
            has_hid = dhid is not None and hid > 0
            need_dw = ctx.needs_input_grad[7 + 2 * l]
            # dOut (+ dbias), and in the same pass -- when the f16x3 / bf16 dW kernel will run for this level -- the fp16
            # planes of dOut and the dW kernel's scales, straight into the dW workspace (xdfm_cin_bwd_prep)
            dws = torch.empty(lib.xdfm_cin_bwd_prep_ws_elems(H, Hp, m, B, D), dtype=torch.float32, device=dev)   # fixed-order dbias
            ws = torch.empty(lib.xdfm_cin_bwd_w_ws_elems(H, Hp, m, N), dtype=torch.float32, device=dev) if need_dw else None
            finish_keep(dws)
            if _RIDER_KEEP is not None and ws is not None:
                _RIDER_KEEP.append(ws)                  # its slabs are read by whichever launch carries the level's sum
            prepared = ctypes.c_int(0)
            _lib.check(_run("cin_dout", 0.0, lambda: lib.xdfm_cin_bwd_prep(
                _ptr(A), _ptr(mk), mk.shape[1] if mk is not None else 0, H, B, D, act, _ptr(dhid) if has_hid else None, 0, hid if has_hid else 0, _ptr(g),
                0 if pool == "sum" else 1, fm if pool == "sum" else N, off, dir0, drows, _ptr(dOut), _ptr(dbias), _ptr(dws),
                _ptr(xp), _ptr(x0), Hp, m, _ptr(ws), ctypes.byref(prepared), _stream())), "cin_dout")
            if need_dw:
                dW = torch.empty((H, Hp * m), dtype=torch.float32, device=dev)
                if prepared.value:
                    call = lambda: lib.xdfm_cin_level_bwd_w_prepared(_ptr(dOut), _ptr(xp), _ptr(x0), H, Hp, m, N, _ptr(ws), _ptr(dW),
                                                                      _stream())
                else:
                    call = lambda: lib.xdfm_cin_level_bwd_w(_ptr(dOut), _ptr(xp), _ptr(x0), H, Hp, m, N, _ptr(ws), _ptr(dW),
                                                             _stream())
                if PROFILE is not None and _lib.get_option("cin_math") in (1, 2):
                    # per-kernel timing: run the call's three phases separately, events around the MFMA kernel only
                    # (a shape without an f16x3 dW kernel ignores the knob: its whole call then runs once, in phase 2)
                    try:
                        _lib.set_option("bww_phase", 1)
                        _lib.check(_run("cin_level_bwd_w passes", 0.0, call), "cin_level_bwd_w")
                        _lib.set_option("bww_phase", 2)
                        _lib.check(_run("cin_level_bwd_w", 2.0 * H * Hp * m * N, call), "cin_level_bwd_w")
                        _lib.set_option("bww_phase", 3)
                        _lib.check(_run("cin_level_bwd_w passes", 0.0, call), "cin_level_bwd_w")
                    finally:
                        _lib.set_option("bww_phase", 0)
                else:
                    _lib.check(_run("cin_level_bwd_w", 2.0 * H * Hp * m * N, call), "cin_level_bwd_w")
                grads[2 * l] = dW.view(W.shape)
            if ctx.needs_input_grad[8 + 2 * l]:
                grads[2 * l + 1] = dbias
            # dX: H <= 256 rows of the contraction per launch
            dxp = torch.empty((Hp, N), dtype=torch.float32, device=dev)
            W2 = W.reshape(H, Hp * m)
            hstep = _lib.get_option("x3_bwx_rows") or 256          # rows of the contraction per launch (<= 256)
            prepacked = ctx.wzs is not None and ctx.wzs[l] is not None and hstep >= H and \
                ctx.cin_math == _lib.get_option("cin_math")
            for h0 in range(0, H, hstep):
                hc = min(hstep, H - h0)
                if prepacked:
                    wz = ctx.wzs[l]
                else:
                    wz = torch.empty(lib.xdfm_cin_bwd_pack_elems(hc, Hp, m), dtype=torch.float32, device=dev)
                    wc = W2[h0:h0 + hc].contiguous()
                    _lib.check(lib.xdfm_cin_bwd_pack(_ptr(wc), hc, Hp, m, _ptr(wz), _stream()), "cin_bwd_pack")
                flags = (1 if h0 == 0 else 0) | (0 if dx0_set else 2)     # XDFM_BWX_SET_DXP | XDFM_BWX_SET_DX0
                if no_dout:
                    _lib.check(_run("cin_level_bwd_x", 2.0 * hc * Hp * m * N, lambda: lib.xdfm_cin_level_bwd_x_src(
                        _ptr(mk) if act == 1 else None, mk.shape[1], _ptr(dhid) if has_hid else None, hid if has_hid else 0, _ptr(g),
                        0 if pool == "sum" else 1, fm if pool == "sum" else N, off, dir0, drows, D, h0, _ptr(xp), _ptr(x0), _ptr(wz),
                        hc, Hp, m, N, _ptr(dxp), _ptr(dx0), flags, _stream())), "cin_level_bwd_x")
                else:
                    dOc = dOut[h0:h0 + hc]
                    _lib.check(_run("cin_level_bwd_x", 2.0 * hc * Hp * m * N, lambda: lib.xdfm_cin_level_bwd_x_ex(
                        _ptr(dOc), _ptr(xp), _ptr(x0), _ptr(wz), hc, Hp, m, N, _ptr(dxp), _ptr(dx0), flags, _stream())),
                        "cin_level_bwd_x")
                dx0_set = True
            if l == 0 and not all(lib.xdfm_cin_bwd_x_is_folded(min(hstep, H - h0), Hp, m, 1) for h0 in range(0, H, hstep)):
                dx0 += dxp                               # x_prev of level 0 is x0 itself (the folded dX kernel has put the
                #                                          whole gradient into dx0 already: include/xdfm.h, option x3_sym)
            dhid = dxp
        return (dx0, None, None, None, None, None, None) + tuple(grads)


def cin_stack(x0_fm, B, D, layer_size, split_half, activation, pool, weights, biases):
    act = activation_code(activation)
    params = []
    for w, b in zip(weights, biases):
        params += [w, b]
    return CINStack.apply(x0_fm, B, D, tuple(layer_size), bool(split_half), act, pool, *params)


def to_fm_layout(x: torch.Tensor) -> torch.Tensor:
    """[B, R, D] -> FM layout [R, B*D] (a transpose; used when a caller hands the reference layout)."""
    B, R, D = x.shape
    return x.permute(1, 0, 2).reshape(R, B * D).contiguous()


def from_fm_layout(t: torch.Tensor, B: int, D: int) -> torch.Tensor:
    """FM layout [R, B*D] -> [B, R, D]."""
    R = t.shape[0]
    return t.view(R, B, D).permute(1, 0, 2)


# --------------------------------------------------------------------------------------------- #
# attention pooling                                                                              #
# --------------------------------------------------------------------------------------------- #
class AttnPool(torch.autograd.Function):
    """FM-layout feature maps [S, B*D] -> pooled [B, D] through n_layers x (MHSA, +residual, LayerNorm)
    and the attention pooling (deepctr/layers/cin_attention.py:63-144, :302-313, :452-464).
    params: per layer Wq, Wk, Wv, Wo (+ gamma, beta when use_ln), then W1, b1, w2.
    p_drop > 0: attention dropout (cin_attention.py:86); the seed of the keep mask is drawn on the device from
    torch's generator (torch.manual_seed makes a run repeatable, a captured graph draws a new one per replay)
    and kept for backward, which regenerates the mask instead of storing it."""

    @staticmethod
    def forward(ctx, fm, B, D, nh, n_layers, use_ln, use_res, p_drop, *params):
        _need_cuda(fm, "feature maps")
        lib = _lib.load()
        S = fm.shape[0]
        assert fm.shape[1] == B * D and fm.is_contiguous()
        theta = torch.cat([p.reshape(-1) for p in params])
        assert theta.numel() == lib.xdfm_cin_attn_theta_elems(D, n_layers, int(use_ln))
        dev = fm.device
        out = torch.empty((B, D), dtype=torch.float32, device=dev)
        tok = torch.empty((n_layers, B, S, D), dtype=torch.float32, device=dev)
        osv = torch.empty((n_layers, B, S, D), dtype=torch.float32, device=dev)
        ml = torch.empty((n_layers, B, S, nh, 2), dtype=torch.float32, device=dev)
        # S^2 * (3 D FMA) per example and layer, counted as 2 FLOP per FMA
        flops = 2.0 * 3 * D * S * S * B * n_layers
        p_drop = float(p_drop)
        seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev) if p_drop > 0 else None
        _lib.check(_run("cin_attn_pool_fwd", flops, lambda: lib.xdfm_cin_attn_pool_fwd(
            _ptr(fm), B, S, D, nh, n_layers, int(use_ln), int(use_res), _ptr(theta), _ptr(out), _ptr(tok), _ptr(osv),
            _ptr(ml), p_drop, _ptr(seed) if seed is not None else None, _stream())), "cin_attn_pool_fwd")
        ctx.cfg = (B, D, nh, n_layers, use_ln, use_res, p_drop, [tuple(p.shape) for p in params])
        ctx.drop_seed = seed
        AttnPool.last_drop_seed = seed          # read by the parity tests (xdfm_cin_attn_dropout_mask)
        ctx.save_for_backward(fm, theta, tok, osv, ml)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        fm, theta, tok, osv, ml = ctx.saved_tensors
        B, D, nh, n_layers, use_ln, use_res, p_drop, shapes = ctx.cfg
        seed = ctx.drop_seed
        S = fm.shape[0]
        dfm = torch.empty_like(fm)
        dtheta = torch.empty_like(theta)         # overwritten: per-workgroup shares + a fixed-order sum, no float atomics
        ws = torch.empty(lib.xdfm_cin_attn_pool_bwd_ws_elems(B, D, n_layers, int(use_ln)), dtype=torch.float32, device=fm.device)
        dout = dout.contiguous()
        flops = 2.0 * 7 * D * S * S * B * n_layers
        _lib.check(_run("cin_attn_pool_bwd", flops, lambda: lib.xdfm_cin_attn_pool_bwd_det(
            _ptr(fm), B, S, D, nh, n_layers, int(use_ln), int(use_res), _ptr(theta), _ptr(tok), _ptr(osv), _ptr(ml),
            _ptr(dout), _ptr(dfm), _ptr(dtheta), _ptr(ws), p_drop, _ptr(seed) if seed is not None else None, _stream())),
            "cin_attn_pool_bwd")
        grads, off = [], 0
        for sh in shapes:
            n = 1
            for k in sh:
                n *= k
            grads.append(dtheta[off:off + n].view(sh))
            off += n
        return (dfm, None, None, None, None, None, None, None) + tuple(grads)


def attn_pool(fm, B, D, mhsa_layers, layer_norms, pooling, use_res):
    """mhsa_layers: modules with W_q/W_k/W_v/W_o (nn.Linear, bias-free) and .num_heads; layer_norms:
    matching nn.LayerNorm list or None; pooling: module whose .attention is Sequential(Linear, Tanh,
    Linear(bias=False))."""
    params = []
    for l, att in enumerate(mhsa_layers):
        params += [att.W_q.weight, att.W_k.weight, att.W_v.weight, att.W_o.weight]
        if layer_norms is not None:
            params += [layer_norms[l].weight, layer_norms[l].bias]
    params += [pooling.attention[0].weight, pooling.attention[0].bias, pooling.attention[2].weight]
    nh = mhsa_layers[0].num_heads
    att0 = mhsa_layers[0]
    p_drop = float(att0.dropout.p) if att0.training else 0.0      # every layer is built with the same attn_dropout
    if any(float(a.dropout.p) != float(att0.dropout.p) for a in mhsa_layers):
        raise ValueError("cin_attn_pool: the attention layers must share one dropout rate")
    if p_drop >= 1.0:
        raise ValueError("cin_attn_pool: attention dropout must be < 1, got %g" % p_drop)
    return AttnPool.apply(fm, B, D, nh, len(mhsa_layers), layer_norms is not None, bool(use_res), p_drop, *params)


# --------------------------------------------------------------------------------------------- #
# dense layer                                                                                    #
# --------------------------------------------------------------------------------------------- #
def _env_switch(environ, key, default=True):
    """'0' turns a switch off; unset or anything else leaves the default."""
    v = environ.get(key)
    return default if v is None else v != "0"


# XDFM_DNN_NATIVE (default 1): dense layers run the fp32-MFMA kernels of csrc/dnn.hip where xdfm_dense_supported says so.
# Read once, at import; tools/dnn_probe.py and the tests flip this attribute to run both paths in one process (a captured
# graph keeps the path it was captured with).
DNN_NATIVE = _env_switch(os.environ, "XDFM_DNN_NATIVE")
# Per operation: the forward kernel (xdfm_dense_fwd) does not beat its library counterpart at the flagship shapes (16.8
# against 16.0 us for 4096 x 429 -> 256, 11.5 against 9.9 us for 256 -> 256), so the forward stays on the
# library GEMM with its fused bias / ReLU epilogue.  The two backward kernels replace three launches each and do win.
DNN_NATIVE_FWD = False


def _ld(t):
    """Row pitch of a 2-D tensor whose rows are contiguous (a one-row tensor's stride(0) is arbitrary)."""
    return max(int(t.stride(0)), int(t.shape[1]))


def _rows_ok(t):
    return t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])


def dense_native(x, W, b=None):
    """Does y = x W^T + b run the native kernels?  fp32 device tensors, x [rows][in] with contiguous rows, W [out][in]
    contiguous, out a multiple of 32 (xdfm_dense_supported), and the XDFM_DNN_NATIVE switch on."""
    if not (DNN_NATIVE and x.is_cuda and W.is_cuda and x.dim() == 2 and W.dim() == 2 and x.dtype == torch.float32
            and W.dtype == torch.float32 and x.shape[0] >= 1 and x.shape[1] == W.shape[1] and W.is_contiguous() and _rows_ok(x)):
        return False
    if b is not None and not (b.is_cuda and b.dtype == torch.float32 and b.dim() == 1 and b.is_contiguous()):
        return False
    return bool(_lib.load().xdfm_dense_supported(x.shape[0], x.shape[1], W.shape[0]))


def _dense_fwd_native(x, W, b, act, p=None, seed=None, layer=0, alpha=None, need_z=False):
    """The forward launch of every native dense layer: y = act(x W^T + b); with `p` dropped as well (DenseReLUDropout);
    with `alpha` the PReLU layer, whose result is (y, z) -- z the pre-activation, stored only with need_z."""
    lib = _lib.load()
    rows, k = x.shape
    out = W.shape[0]
    y = torch.empty(rows, out, dtype=torch.float32, device=x.device)
    operands = (_ptr(x), rows, k, _ld(x), _ptr(W), out, _ptr(b))
    if alpha is not None:
        z = torch.empty(rows, out, dtype=torch.float32, device=x.device) if need_z else None
        name, args = "dense_prelu_fwd", operands + (_ptr(alpha), _ptr(y), out, _ptr(z), out)
    elif p is not None:
        name, args = "dense_fwd_drop", operands + (act, _ptr(y), out, p, _ptr(seed), int(layer), 0)
    else:
        name, args = "dense_fwd", operands + (act, _ptr(y), out)
    _lib.check(_run(name, 0.0, lambda: getattr(lib, "xdfm_" + name)(*args, _stream())), name)
    return y if alpha is None else (y, z)


def _dense_bwd_native(g, y, x, W, need_dx, need_dw, need_db, p=None, alpha=None, need_da=False):
    """(dx, dW, db) of one layer, with `alpha` (dx, dW, db, dalpha).  y gates g while the kernels load it: the ReLU layer's
    output; with `p` its dropped output (a kept cell's g is scaled by 1 / (1 - p)); with `alpha` the PReLU layer's
    pre-activation; None for no gate.  db, and dalpha, are by-products of the dW kernel: one call whatever the combination."""
    lib = _lib.load()
    rows, k = x.shape
    out = W.shape[0]
    if not _rows_ok(g):
        g = g.contiguous()
    dev = g.device
    ws_elems = lib.xdfm_dense_bwd_w_ws_elems
    if alpha is not None:
        name_x, name_w, ws_elems = "dense_prelu_bwd_x", "dense_prelu_bwd_w", lib.xdfm_dense_prelu_bwd_w_ws_elems
    elif p is not None:
        name_x, name_w = "dense_bwd_x_drop", "dense_bwd_w_drop"
    else:
        name_x, name_w = "dense_bwd_x", "dense_bwd_w"
    gated = (_ptr(g), _ld(g), _ptr(y), _ld(y) if y is not None else 0) + (() if alpha is None else (_ptr(alpha),))
    rate = () if p is None else (p,)
    dx = dW = db = da = None
    if need_dx:
        dx = torch.empty(rows, k, dtype=torch.float32, device=dev)
        _lib.check(_run(name_x, 0.0, lambda: getattr(lib, "xdfm_" + name_x)(*gated, rows, out, _ptr(W), k, _ptr(dx), k, *rate,
                                                                          _stream())), name_x)
    if need_dw or need_db or need_da:
        ws = torch.empty(ws_elems(rows, k, out), dtype=torch.float32, device=dev)
        dW = torch.empty(out, k, dtype=torch.float32, device=dev)
        db = torch.empty(out, dtype=torch.float32, device=dev) if need_db else None
        da = torch.empty(alpha.shape, dtype=torch.float32, device=dev) if need_da else None
        slope = () if alpha is None else (_ptr(da),)
        finish_keep(ws)
        _lib.check(_run(name_w, 0.0, lambda: getattr(lib, "xdfm_" + name_w)(*gated, _ptr(x), _ld(x), rows, k, out, _ptr(ws), _ptr(dW),
                                                                          _ptr(db), *slope, *rate, _stream())), name_w)
    grads = (dx, dW if need_dw else None, db)
    return grads if alpha is None else grads + (da,)


def _bias_grad_lib(g, y=None):
    """(gz, db) behind a library GEMM, g contiguous: db the column sums of gz by the library's own memset-free pass, gz = g
    or, with the ReLU layer's output y, (y > 0) ? g : 0 written by the same pass."""
    lib = _lib.load()
    rows, cols = g.shape
    ws = torch.empty(lib.xdfm_colsum_ws_elems(cols), dtype=torch.float32, device=g.device)
    db = torch.empty(cols, dtype=torch.float32, device=g.device)
    finish_keep(ws)
    if y is None:
        _lib.check(lib.xdfm_colsum(_ptr(g), rows, cols, g.stride(0), _ptr(ws), _ptr(db), _stream()), "colsum")
        return g, db
    gz = torch.empty_like(g)
    _lib.check(lib.xdfm_relu_bwd_colsum(_ptr(g), _ptr(y), rows, cols, g.stride(0), y.stride(0), _ptr(ws), _ptr(gz), _ptr(db),
                                        _stream()), "relu_bwd_colsum")
    return gz, db


class Dense(torch.autograd.Function):
    """y = x W^T + b (deepctr/layers/core.py:120-134).  Where `dense_native` holds, both gradients run the fp32-MFMA
    kernels of csrc/dnn.hip (the bias gradient comes out of the weight-gradient kernel; the forward only with
    DNN_NATIVE_FWD).  Elsewhere the three GEMMs stay with hipBLASLt and the bias gradient is the library's own column sum, because ATen's `sum(0)` zeroes a
    semaphore buffer with hipMemsetAsync and a memset node inside a captured HIP graph is not ordered reliably on this
    stack (tools/graph_memset_probe.py) -- either way the train step contains no memset at all."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        ctx.has_bias = b is not None
        if DNN_NATIVE_FWD and dense_native(x, W, b):
            return _dense_fwd_native(x, W, b, ACT_CODES["linear"])
        return torch.nn.functional.linear(x, W, b)

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        if dense_native(x, W):
            return _dense_bwd_native(g, None, x, W, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                     ctx.has_bias and ctx.needs_input_grad[2])
        g = g.contiguous()
        dx = g.mm(W) if ctx.needs_input_grad[0] else None
        dW = g.t().mm(x) if ctx.needs_input_grad[1] else None
        db = _bias_grad_lib(g)[1] if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dW, db


class DenseReLU(torch.autograd.Function):
    """y = relu(x W^T + b).  Native (`dense_native`): the backward kernels
    apply the mask (y > 0) while they load g, so no masked copy of g is allocated or written, and the bias gradient is a
    by-product of the weight-gradient kernel (with DNN_NATIVE_FWD, bias and ReLU in the epilogue of xdfm_dense_fwd too).
    Forward, and elsewhere the backward as well: the ReLU rides in the library GEMM's epilogue (hipBLASLt,
    `torch._addmm_activation`), and its backward mask is applied by the pass that sums the bias gradient
    (`xdfm_relu_bwd_colsum`) -- two launches fewer each way per hidden layer than linear + nn.ReLU
    (deepctr/layers/core.py:120-134)."""

    @staticmethod
    def forward(ctx, x, W, b):
        if DNN_NATIVE_FWD and dense_native(x, W, b):
            y = _dense_fwd_native(x, W, b, ACT_CODES["relu"])
        else:
            y = torch._addmm_activation(b, x, W.t(), use_gelu=False)
        ctx.save_for_backward(x, W, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x, W, y = ctx.saved_tensors
        if dense_native(x, W):
            return _dense_bwd_native(g, y, x, W, *ctx.needs_input_grad)
        gz, db = _bias_grad_lib(g.contiguous(), y)
        dx = gz.mm(W) if ctx.needs_input_grad[0] else None
        dW = gz.t().mm(x) if ctx.needs_input_grad[1] else None
        return dx, dW, db if ctx.needs_input_grad[2] else None


def dense_relu(x, W, b):
    if x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and b is not None and x.is_contiguous():
        return DenseReLU.apply(x, W, b)
    return torch.relu(dense(x, W, b))


def dense(x, W, b):
    if x.is_cuda and x.dim() == 2 and x.dtype == torch.float32:
        return Dense.apply(x, W, b)
    return torch.nn.functional.linear(x, W, b)


# XDFM_DNN_DROPOUT_NATIVE (default 1): in training, with 0 < p < 1, a ReLU layer that `dense_native` accepts runs
# DenseReLUDropout instead of dense_relu + nn.Dropout.  Read once, at import; a module attribute the tests and
# tools/dnn_probe.py flip, like DNN_NATIVE (which has to be on as well).
DNN_DROPOUT_NATIVE = _env_switch(os.environ, "XDFM_DNN_DROPOUT_NATIVE")


def dense_dropout_native(x, W, b, p):
    """Does dropout(relu(x W^T + b)) run in the dense kernels?  Both switches on, 0 < p < 1, a bias, and `dense_native`."""
    return bool(DNN_DROPOUT_NATIVE and DNN_NATIVE and 0.0 < float(p) < 1.0 and b is not None and dense_native(x, W, b))


def draw_dropout_seed(device):
    """The device scalar a hashed keep mask is keyed with, drawn as AttnPool draws its own: from torch's generator
    (torch.manual_seed repeats a run), on the device (a captured graph draws a new one at every replay)."""
    return torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device)


class DenseReLUDropout(torch.autograd.Function):
    """d = dropout(relu(x W^T + b)) in one launch (xdfm_dense_fwd_drop): keep ? relu(z) / (1 - p) : 0 with the keep bit a
    hash of (seed, layer, row, column).  d > 0 holds exactly where the cell was kept and z > 0, so d is all the backward
    needs: the two _drop kernels select on d > 0 and scale g by the same 1 / (1 - p) while they stage it.  Saved: x, W, d --
    no mask, no second activation.  seed: int64 device tensor of one element; layer: the layer's index in its tower."""

    @staticmethod
    def forward(ctx, x, W, b, p, seed, layer):
        _need_cuda(x, "x")
        ctx.p = float(p)
        d = _dense_fwd_native(x, W, b, ACT_CODES["relu"], p=ctx.p, seed=seed, layer=layer)
        ctx.save_for_backward(x, W, d)
        return d

    @staticmethod
    def backward(ctx, g):
        x, W, d = ctx.saved_tensors
        return _dense_bwd_native(g, d, x, W, *ctx.needs_input_grad[:3], p=ctx.p) + (None, None, None)


def dense_relu_dropout(x, W, b, p, seed, layer):
    """dropout(relu(x W^T + b)) through DenseReLUDropout; the caller has checked `dense_dropout_native` (anything else is an
    error here, not a fall-back)."""
    if not (0.0 < float(p) < 1.0):
        raise ValueError("dense_relu_dropout: p = %r outside (0, 1)" % (p,))
    if b is None or not dense_native(x, W, b):
        raise ValueError("dense_relu_dropout: the native dense kernels do not take these operands (fp32 device tensors, "
                         "contiguous rows, out a multiple of 32, XDFM_DNN_NATIVE on)")
    if not (seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1):
        raise ValueError("dense_relu_dropout: seed must be an int64 device tensor of one element")
    return DenseReLUDropout.apply(x, W, b, float(p), seed, int(layer))


def dense_relu_then_dropout(x, W, b, drop, training, seed, layer):
    """One ReLU layer of a tower and the nn.Dropout `drop` behind it -> (result, seed).  In training the dropout runs inside
    the dense kernels where `dense_dropout_native` says so: no mask tensor, no extra launch, keyed by `seed` --
    one per call of the tower, drawn by the first layer that needs it (pass None) and shared through the layers' indices.
    Everything else is dense_relu with `drop` applied to it."""
    if training and dense_dropout_native(x, W, b, drop.p):
        if seed is None:
            seed = draw_dropout_seed(x.device)
        return dense_relu_dropout(x, W, b, drop.p, seed, layer), seed
    return drop(dense_relu(x, W, b)), seed


# XDFM_DNN_PRELU_NATIVE: a dense layer followed by nn.PReLU() (layers.DNN with activation='prelu', no batch norm) runs
# DensePReLU -- the fused kernels of csrc/dnn.hip, forward included -- where `dense_prelu_native` holds; XDFM_DNN_NATIVE has to
# be on as well.  0: the library GEMMs of `dense` followed by the native elementwise op (`prelu`, csrc/prelu.hip).  Either way
# a GPU fp32 tower never runs torch's prelu_backward, whose `sum` puts a memset into a captured step.  Read once, at import; a
# module attribute the tests and tools/dnn_prelu_probe.py flip, like DNN_NATIVE.  Default 1: the fused route is not slower
# at either flagship layer (61.8 against 65.3 us, 45.9 against 49.2 us forward + backward) and ties in the step within its
# spread (40 graph nodes against 46): profiles/dnn_prelu_probe.md.
DNN_PRELU_NATIVE = _env_switch(os.environ, "XDFM_DNN_PRELU_NATIVE")


def _alpha_ok(alpha, ref):
    """One contiguous fp32 slope on ref's device (the weight of nn.PReLU())."""
    return (isinstance(alpha, torch.Tensor) and alpha.is_cuda and alpha.device == ref.device and alpha.dtype == torch.float32
            and alpha.numel() == 1 and alpha.is_contiguous())


def dense_prelu_native(x, W, b, alpha):
    """Does prelu(x W^T + b, alpha) run the fused kernels?  Both switches on, a bias, one fp32 device slope, and `dense_native`."""
    return bool(DNN_PRELU_NATIVE and DNN_NATIVE and b is not None and _alpha_ok(alpha, x) and dense_native(x, W, b))


class DensePReLU(torch.autograd.Function):
    """y = prelu(x W^T + b, alpha) with one scalar slope, in the fp32-MFMA kernels of csrc/dnn.hip: one forward launch that
    stores y and, when a gradient will be asked for, the pre-activation z (alpha may be 0, 1 or negative: y says neither the
    sign nor the value of z); the two backward kernels form gz = z > 0 ? g : alpha * g while they stage g, and the slope's
    gradient comes out of the weight-gradient kernel as the bias gradient does (double partials, a fixed-order finish).
    Saved: x, W, z, alpha.  The kernels read alpha from device memory: a replayed graph sees the optimizer's update."""

    @staticmethod
    def forward(ctx, x, W, b, alpha):
        _need_cuda(x, "x")
        y, z = _dense_fwd_native(x, W, b, ACT_CODES["linear"], alpha=alpha, need_z=any(ctx.needs_input_grad))
        ctx.save_for_backward(x, W, z, alpha)
        return y

    @staticmethod
    def backward(ctx, g):
        x, W, z, alpha = ctx.saved_tensors
        need_dx, need_dw, need_db, need_da = ctx.needs_input_grad
        return _dense_bwd_native(g, z, x, W, need_dx, need_dw, need_db, alpha=alpha, need_da=need_da)


def _dense_prelu_fused(x, W, b, alpha):
    """The fused branch of dense_prelu (a function of its own so that tests and tools can count its calls)."""
    return DensePReLU.apply(x, W, b, alpha)


def dense_prelu(x, W, b, alpha):
    """prelu(x W^T + b, alpha): DensePReLU where `dense_prelu_native` holds, else `dense` followed by `prelu`."""
    if dense_prelu_native(x, W, b, alpha):
        return _dense_prelu_fused(x, W, b, alpha)
    return prelu(dense(x, W, b), alpha)


def prelu_native(u, alpha):
    """Does prelu(u, alpha) run the elementwise kernels of csrc/prelu.hip?  A non-empty fp32 2-D device tensor with contiguous
    rows and one fp32 slope on its device.  No switch: the alternative is torch's prelu_backward and its memset."""
    return bool(isinstance(u, torch.Tensor) and u.is_cuda and u.dim() == 2 and u.dtype == torch.float32 and u.shape[0] >= 1
                and u.shape[1] >= 1 and _rows_ok(u) and _alpha_ok(alpha, u))


class PReLU(torch.autograd.Function):
    """y = u > 0 ? u : alpha * u with one scalar slope (csrc/prelu.hip): one launch forward; backward one launch for du and,
    when the slope wants its gradient, per-block double partials of sum g * u [u <= 0] and a one-block finish.  Saved: u, alpha."""

    @staticmethod
    def forward(ctx, u, alpha):
        _need_cuda(u, "u")
        lib = _lib.load()
        rows, cols = u.shape
        y = torch.empty(rows, cols, dtype=torch.float32, device=u.device)
        _lib.check(_run("prelu_fwd", 0.0, lambda: lib.xdfm_prelu_fwd(_ptr(u), _ld(u), rows, cols, _ptr(alpha), _ptr(y), cols, _stream())),
                   "prelu_fwd")
        ctx.save_for_backward(u, alpha)
        return y

    @staticmethod
    def backward(ctx, g):
        u, alpha = ctx.saved_tensors
        lib = _lib.load()
        rows, cols = u.shape
        need_du, need_da = ctx.needs_input_grad
        if not (need_du or need_da):
            return None, None
        if not _rows_ok(g):
            g = g.contiguous()
        dev = g.device
        du = torch.empty(rows, cols, dtype=torch.float32, device=dev) if need_du else None
        da = torch.empty(alpha.shape, dtype=torch.float32, device=dev) if need_da else None
        ws = torch.empty(lib.xdfm_prelu_ws_elems(rows, cols), dtype=torch.float32, device=dev) if need_da else None
        _lib.check(_run("prelu_bwd", 0.0, lambda: lib.xdfm_prelu_bwd(_ptr(g), _ld(g), _ptr(u), _ld(u), rows, cols, _ptr(alpha), _ptr(du), cols,
                                                                     _ptr(da), _ptr(ws), _stream())), "prelu_bwd")
        return du, da


def _prelu_native(u, alpha):
    """The native branch of prelu (a function of its own so that tests and tools can count its calls)."""
    return PReLU.apply(u, alpha)


def prelu(u, alpha):
    """torch's prelu with one slope: the elementwise kernels where `prelu_native` holds; everything else (CPU, float64, other
    ranks) is torch.nn.functional.prelu."""
    if prelu_native(u, alpha):
        return _prelu_native(u, alpha)
    return torch.nn.functional.prelu(u, alpha)


# XDFM_DNN_BN_NATIVE (default 1): a dense layer followed by nn.BatchNorm1d (layers.DNN with use_bn=True) runs its batch norm
# and its activation in the kernels of csrc/bn.hip instead of nn.BatchNorm1d + torch.relu / torch.sigmoid.  Read once, at
# import; a module attribute the tests and tools/dnn_bn_probe.py flip, like DNN_NATIVE (of which it is independent: the
# dense layer in front keeps whatever route `dense_native` gives it).
DNN_BN_NATIVE = _env_switch(os.environ, "XDFM_DNN_BN_NATIVE")


def bn_native(z, bn):
    """Does act(bn(z)) run the native kernels?  fp32 device tensor z [rows][cols] with contiguous rows; an nn.BatchNorm1d
    with affine parameters, track_running_stats and a float momentum (what layers.DNN builds), all fp32 on z's device; the
    XDFM_DNN_BN_NATIVE switch on."""
    if not (DNN_BN_NATIVE and isinstance(bn, torch.nn.BatchNorm1d) and z.is_cuda and z.dim() == 2 and z.dtype == torch.float32
            and z.shape[0] >= 1 and z.shape[1] == bn.num_features and _rows_ok(z)):
        return False
    if not (bn.affine and bn.track_running_stats and isinstance(bn.momentum, float) and 0.0 <= bn.momentum <= 1.0 and bn.eps > 0):
        return False
    return all(t is not None and t.device == z.device and t.dtype == torch.float32 and t.is_contiguous()
               for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))


class BatchNormAct(torch.autograd.Function):
    """y = act(batch_norm(z)) over the rows of z [rows][cols] (deepctr/layers/core.py:120-134 with use_bn): two launches in
    training (per-block (mean, M2) pairs, then a Chan merge + apply, which also updates running_mean / running_var in
    place), one in evaluation (running statistics).  Backward: two launches, gm = act'(y) * g formed while g is loaded.
    Saved: z, y, gamma, mean, rstd -- no normalised copy, no mask, no second activation.  In evaluation the statistics
    are constants and the backward (xdfm_bn_bwd_eval) has no mean terms."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, eps, momentum, act, training):
        _need_cuda(z, "z")
        lib = _lib.load()
        rows, cols = z.shape
        dev = z.device
        y = torch.empty(rows, cols, dtype=torch.float32, device=dev)
        if training:
            stats = torch.empty(2, cols, dtype=torch.float32, device=dev)
            mean, rstd = stats[0], stats[1]
            ws = torch.empty(lib.xdfm_bn_ws_elems(rows, cols), dtype=torch.float32, device=dev)
            _lib.check(_run("bn_fwd_train", 0.0, lambda: lib.xdfm_bn_fwd_train(
                _ptr(z), _ld(z), rows, cols, _ptr(gamma), _ptr(beta), float(eps), float(momentum), int(act), _ptr(y), cols, _ptr(mean),
                _ptr(rstd), _ptr(running_mean), _ptr(running_var), _ptr(ws), _stream())), "bn_fwd_train")
        else:
            _lib.check(_run("bn_fwd_eval", 0.0, lambda: lib.xdfm_bn_fwd_eval(
                _ptr(z), _ld(z), rows, cols, _ptr(gamma), _ptr(beta), float(eps), int(act), _ptr(y), cols, _ptr(running_mean),
                _ptr(running_var), _stream())), "bn_fwd_eval")
            mean, rstd = running_mean, None
            if any(ctx.needs_input_grad[:3]):
                mean, rstd = running_mean.clone(), torch.rsqrt(running_var + float(eps))
        ctx.act, ctx.training = int(act), bool(training)
        ctx.save_for_backward(z, y, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, g):
        z, y, gamma, mean, rstd = ctx.saved_tensors
        lib = _lib.load()
        rows, cols = z.shape
        need_dz, need_dg, need_db = ctx.needs_input_grad[:3]
        if not _rows_ok(g):
            g = g.contiguous()
        dev = g.device
        dz = torch.empty(rows, cols, dtype=torch.float32, device=dev) if need_dz else None
        dgamma = torch.empty(cols, dtype=torch.float32, device=dev) if need_dg else None
        dbeta = torch.empty(cols, dtype=torch.float32, device=dev) if need_db else None
        if need_dz or need_dg or need_db:
            ws = torch.empty(lib.xdfm_bn_ws_elems(rows, cols), dtype=torch.float32, device=dev)
            fn, name = (lib.xdfm_bn_bwd, "bn_bwd") if ctx.training else (lib.xdfm_bn_bwd_eval, "bn_bwd_eval")
            _lib.check(_run(name, 0.0, lambda: fn(_ptr(g), _ld(g), _ptr(y), _ld(y), _ptr(z), _ld(z), rows, cols, _ptr(gamma), _ptr(mean),
                                                  _ptr(rstd), ctx.act, _ptr(dz), cols, _ptr(dgamma), _ptr(dbeta), _ptr(ws), _stream())), name)
        return dz, dgamma, dbeta, None, None, None, None, None, None


def bn_act(z, bn, act, training):
    """act(bn(z)) for an nn.BatchNorm1d `bn` that stays the holder of gamma, beta and the running statistics (state_dict keys
    unchanged).  Where `bn_native` holds: BatchNormAct, with num_batches_tracked incremented on the device in training (a
    captured step replays it).  Elsewhere: the stock sequence, bn(z) then torch.relu / torch.sigmoid."""
    code = activation_code(act)
    if bn_native(z, bn):
        return _bn_act_native(z, bn, code, bool(training))
    x = bn(z)
    if code == ACT_CODES["relu"]:
        return torch.relu(x)
    if code == ACT_CODES["sigmoid"]:
        return torch.sigmoid(x)
    return x


def _bn_act_native(z, bn, code, training):
    """The native branch of bn_act (a function of its own so that tests and tools can count its calls)."""
    if training:
        if z.shape[0] < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (z.size(),))
        bn.num_batches_tracked.add_(1)
    return BatchNormAct.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps), float(bn.momentum), code, training)


# XDFM_DNN_BN_SYNC (default 0): under row-parallel training (xdfm_amd/dist.py) the batch norm of the DNN tower takes its mean
# and variance over the GLOBAL batch, as torch's SyncBatchNorm does, in the native kernels: N ranks then equal one process
# on the global batch and the running statistics of a checkpoint are those of the whole batch.  Off, a row-parallel tower
# keeps the stock nn.BatchNorm1d over each rank's shard, as before.  Opt-in because it changes what a row-parallel run with
# dnn_use_bn=True computes, adds two small collectives per batch-norm layer and direction, and keeps the row-parallel step
# out of the captured graph (a collective sits inside the tower).  Read once, at import, like its neighbours.
DNN_BN_SYNC = _env_switch(os.environ, "XDFM_DNN_BN_SYNC", False)


def bn_sync_native(z, bn, dp):
    """Does act(bn(z)) run the synchronised native kernels?  The XDFM_DNN_BN_SYNC switch on, `bn_native(z, bn)`, and `dp` a
    dist.RowParallel context (anything else -- no context, an object of another kind -- keeps the caller's other routes)."""
    if not DNN_BN_SYNC or dp is None:
        return False
    from . import dist as xdist
    return isinstance(dp, xdist.RowParallel) and bn_native(z, bn)


def _bn_sync_count(z, dp):
    """Rows of this rank that belong to the global batch: all of z's, or 0 for a rank that holds only a stand-in row
    (dist.RowParallel.shard).  Without a preceding shard() every row counts."""
    if dp._n_global is not None and dp.local_sizes()[dp.rank] == 0:
        return 0
    return int(z.shape[0])


class BatchNormActSync(torch.autograd.Function):
    """BatchNormAct in training mode with the statistics of the global batch of a row-parallel step.  Forward: this rank's
    (mean, M2) pair (xdfm_bn_stats), ONE all-gather of [count | means | M2s] doubles, then the Chan merge of the ranks'
    triples in rank order + apply (xdfm_bn_fwd_apply_sync), which also updates the running statistics -- from the same
    gathered bytes on every rank, so the replicas' buffers stay bit-identical.  Backward: this rank's two column sums
    (xdfm_bn_bwd_sums), ONE all-gather, then dz over the global sums (xdfm_bn_bwd_apply_sync); dgamma and dbeta are this
    rank's own sums, which the flat all-reduce of the dense gradients makes global like every other dense weight's.  A
    rank that holds only a stand-in row contributes count 0 and gets exact zeros for dz."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, eps, momentum, act, dp, count):
        _need_cuda(z, "z")
        lib = _lib.load()
        rows, cols = z.shape
        dev = z.device
        ws = torch.empty(lib.xdfm_bn_ws_elems(rows, cols), dtype=torch.float32, device=dev)
        mine = torch.empty(1, 1 + 2 * cols, dtype=torch.float64, device=dev)
        mine[0, 0] = float(count)
        pair = mine[0, 1:]
        _lib.check(_run("bn_stats", 0.0, lambda: lib.xdfm_bn_stats(_ptr(z), _ld(z), rows, cols, _ptr(pair), _ptr(ws), _stream())),
                   "bn_stats")
        gathered = dp.all_gather_rows(mine)
        # the counts follow from the sharding alone, but they are read off the gathered buffer: what every rank checks is
        # what the kernel will merge, and all ranks take the same decision after the same collective
        n_total = int(round(float(gathered[:, 0].sum().item())))
        if n_total < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s over %d ranks"
                             % (tuple(z.size()), dp.world))
        y = torch.empty(rows, cols, dtype=torch.float32, device=dev)
        stats = torch.empty(2, cols, dtype=torch.float32, device=dev)
        mean, rstd = stats[0], stats[1]
        _lib.check(_run("bn_fwd_apply_sync", 0.0, lambda: lib.xdfm_bn_fwd_apply_sync(
            _ptr(z), _ld(z), rows, cols, _ptr(gathered), dp.world, _ptr(gamma), _ptr(beta), float(eps), float(momentum), int(act),
            _ptr(y), cols, _ptr(mean), _ptr(rstd), _ptr(running_mean), _ptr(running_var), _stream())), "bn_fwd_apply_sync")
        ctx.act, ctx.dp, ctx.counted, ctx.n_total = int(act), dp, rows if count else 0, n_total
        ctx.save_for_backward(z, y, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, g):
        z, y, gamma, mean, rstd = ctx.saved_tensors
        lib = _lib.load()
        dp = ctx.dp
        rows, cols = z.shape
        need_dz, need_dg, need_db = ctx.needs_input_grad[:3]
        if not _rows_ok(g):
            g = g.contiguous()
        dev = g.device
        # the collective runs whatever this rank needs: every rank joins it
        ws = torch.empty(lib.xdfm_bn_ws_elems(rows, cols), dtype=torch.float32, device=dev)
        mine = torch.empty(1, 2 * cols, dtype=torch.float64, device=dev)
        _lib.check(_run("bn_bwd_sums", 0.0, lambda: lib.xdfm_bn_bwd_sums(
            _ptr(g), _ld(g), _ptr(y), _ld(y), _ptr(z), _ld(z), rows, cols, _ptr(mean), _ptr(rstd), ctx.act, _ptr(mine), _ptr(ws),
            _stream())), "bn_bwd_sums")
        gathered = dp.all_gather_rows(mine)
        dz = torch.empty(rows, cols, dtype=torch.float32, device=dev) if need_dz else None
        dgamma = torch.empty(cols, dtype=torch.float32, device=dev) if need_dg else None
        dbeta = torch.empty(cols, dtype=torch.float32, device=dev) if need_db else None
        if need_dz or need_dg or need_db:
            _lib.check(_run("bn_bwd_apply_sync", 0.0, lambda: lib.xdfm_bn_bwd_apply_sync(
                _ptr(g), _ld(g), _ptr(y), _ld(y), _ptr(z), _ld(z), rows, ctx.counted, cols, _ptr(gathered), dp.world, dp.rank,
                ctx.n_total, _ptr(gamma), _ptr(mean), _ptr(rstd), ctx.act, _ptr(dz), cols, _ptr(dgamma), _ptr(dbeta), _stream())),
                "bn_bwd_apply_sync")
        return dz, dgamma, dbeta, None, None, None, None, None, None, None


def bn_act_sync(z, bn, act, training, dp):
    """act(bn(z)) with the statistics of the global batch of the row-parallel context `dp` (callers test `bn_sync_native`
    first).  Training: BatchNormActSync, num_batches_tracked incremented on the device as in `_bn_act_native`; fewer than two
    rows in the global batch raise the stock module's ValueError on every rank, after the gather all of them have joined.
    Evaluation: the running statistics are identical on all replicas, so it is BatchNormAct's evaluation branch
    (xdfm_bn_fwd_eval / xdfm_bn_bwd_eval) with no collective."""
    code = activation_code(act)
    if not training:
        return BatchNormAct.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps), float(bn.momentum), code,
                                  False)
    y = BatchNormActSync.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps), float(bn.momentum), code, dp,
                               _bn_sync_count(z, dp))
    bn.num_batches_tracked.add_(1)
    return y


# --------------------------------------------------------------------------------------------- #
# output head                                                                                    #
# --------------------------------------------------------------------------------------------- #
LINK_SIGMOID, LINK_IDENTITY = 0, 1          # XDFM_LINK_* of include/xdfm.h
LOSS_BCE, LOSS_MSE, LOSS_MAE = 0, 1, 2      # XDFM_LOSS_*


def head_mode(task, loss_func):
    """(link, loss) of the native head (K8) for a model's task and compiled loss, or None when the stock tail has to
    run: 'binary' -> sigmoid, 'regression' -> identity (PredictionLayer, core.py:150-160); F.binary_cross_entropy /
    F.mse_loss / F.l1_loss -> bce / mse / mae, matched by identity (what compile() stores for "binary_crossentropy",
    "mse", "mae"; basemodel.py:463-480).  None for 'multiclass', a list of losses, any other callable and
    (regression, bce), which has no kernel.  Pure: needs no device."""
    link = {"binary": LINK_SIGMOID, "regression": LINK_IDENTITY}.get(task) if isinstance(task, str) else None
    if link is None or isinstance(loss_func, (list, tuple)):
        return None
    F = torch.nn.functional
    for fn, loss in ((F.binary_cross_entropy, LOSS_BCE), (F.mse_loss, LOSS_MSE), (F.l1_loss, LOSS_MAE)):
        if loss_func is fn:
            return None if (link == LINK_IDENTITY and loss == LOSS_BCE) else (link, loss)
    return None


class Head(torch.autograd.Function):
    """(y [B,1], bias [1]|None, lin [B,1]|None, u [B,Ku]|None, wu [1,Ku]|None, v [B,Kv]|None, wv [1,Kv]|None,
    link = sigmoid, loss = bce) -> (pred [B], loss [1]) with pred = LINK(lin + u wu^T + v wv^T + bias), loss = sum
    LOSS(pred, y): cin_linear / dnn_linear + logit sum (deepctr/models/xdeepfm.py:95-105) + PredictionLayer
    (core.py:150-160) + the summed loss of the batch loop (basemodel.py:254; F.binary_cross_entropy, F.mse_loss or
    F.l1_loss with reduction='sum'), two launches each way (K8).  `link` / `loss` are the pairs of head_mode().  `pred`
    is returned for metrics and is not differentiable here (the model's train step differentiates the loss only).
    `w` ([B] or [B,1] float32 on the device, or None): one weight per example, loss = sum w_b LOSS(pred_b, y_b) through
    xdfm_head_fwd_w / _bwd_w; it is kept for the backward and has no gradient.  Without it the _ex entry points run, as
    they always did."""

    @staticmethod
    def forward(ctx, y, bias, lin, u, wu, v, wv, link=LINK_SIGMOID, loss=LOSS_BCE, w=None):
        lib = _lib.load()
        yv = y.reshape(-1).contiguous()
        B = yv.numel()
        dev = yv.device
        linv = lin.reshape(-1).contiguous() if lin is not None else None
        u = u.contiguous() if u is not None else None
        v = v.contiguous() if v is not None else None
        wu = wu.reshape(-1).contiguous() if wu is not None else None
        wv = wv.reshape(-1).contiguous() if wv is not None else None
        Ku = u.shape[1] if u is not None else 0
        Kv = v.shape[1] if v is not None else 0
        for t, k in ((u, Ku), (v, Kv)):
            if t is not None and (t.dim() != 2 or t.shape[0] != B):
                raise ValueError("xdfm head: operands must be [B, K]")
        if w is not None:
            if w.dtype != torch.float32 or w.device != dev or w.numel() != B or w.dim() > 2:
                raise ValueError("xdfm head: w must be a float32 [B] or [B,1] tensor on the device of y")
            w = w.reshape(-1).contiguous()
        pred = torch.empty(B, dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.xdfm_head_ws_elems(Ku, Kv), dtype=torch.float32, device=dev)
        finish_keep(ws)
        if w is None:
            _lib.check(lib.xdfm_head_fwd_ex(_ptr(linv), _ptr(u), _ptr(wu), Ku, _ptr(v), _ptr(wv), Kv, _ptr(bias), _ptr(yv), B,
                                            _ptr(pred), _ptr(out), _ptr(ws), int(link), int(loss), _stream()), "head_fwd")
        else:
            _lib.check(lib.xdfm_head_fwd_w(_ptr(linv), _ptr(u), _ptr(wu), Ku, _ptr(v), _ptr(wv), Kv, _ptr(bias), _ptr(yv), B,
                                           _ptr(pred), _ptr(out), _ptr(ws), int(link), int(loss), _ptr(w), _stream()),
                       "head_fwd_w")
        ctx.save_for_backward(pred, yv, u, wu, v, wv, w)
        ctx.cfg = (bias is not None, lin is not None, tuple(lin.shape) if lin is not None else None, Ku, Kv)
        ctx.mode = (int(link), int(loss))
        ctx.mark_non_differentiable(pred)
        ctx.set_materialize_grads(False)          # no [B] zero fill for pred's (unused) gradient slot
        return pred, out

    @staticmethod
    def backward(ctx, _gpred, gloss):
        if gloss is None:
            return (None,) * 10
        lib = _lib.load()
        pred, yv, u, wu, v, wv, w = ctx.saved_tensors
        has_bias, has_lin, lin_shape, Ku, Kv = ctx.cfg
        B = pred.numel()
        dev = pred.device
        f32 = dict(dtype=torch.float32, device=dev)
        dlin = torch.empty(B, **f32) if has_lin else None
        du = torch.empty((B, Ku), **f32) if u is not None else None
        dv = torch.empty((B, Kv), **f32) if v is not None else None
        grads = torch.empty(Ku + Kv + 1, **f32)
        ws = torch.empty(lib.xdfm_head_ws_elems(Ku, Kv), **f32)
        finish_keep(ws)
        gl = gloss.reshape(1).contiguous()
        if w is None:
            _lib.check(lib.xdfm_head_bwd_ex(_ptr(pred), _ptr(yv), _ptr(gl), _ptr(u), _ptr(wu), Ku, _ptr(v), _ptr(wv), Kv, B,
                                            _ptr(dlin), _ptr(du), _ptr(dv), _ptr(grads), _ptr(ws), ctx.mode[0], ctx.mode[1],
                                            _stream()), "head_bwd")
        else:
            _lib.check(lib.xdfm_head_bwd_w(_ptr(pred), _ptr(yv), _ptr(gl), _ptr(u), _ptr(wu), Ku, _ptr(v), _ptr(wv), Kv, B,
                                           _ptr(dlin), _ptr(du), _ptr(dv), _ptr(grads), _ptr(ws), ctx.mode[0], ctx.mode[1],
                                           _ptr(w), _stream()), "head_bwd_w")
        return (None, grads[Ku + Kv:Ku + Kv + 1] if has_bias else None,
                dlin.view(lin_shape) if has_lin else None,
                du, grads[:Ku].view(1, Ku) if u is not None else None,
                dv, grads[Ku:Ku + Kv].view(1, Kv) if v is not None else None, None, None, None)


# --------------------------------------------------------------------------------------------- #
# vocabulary-wide softmax cross-entropy (SFG decoder heads)                                       #
# --------------------------------------------------------------------------------------------- #
VOCAB_TILE_BYTES = 256 << 20        # logits of one vocabulary tile kept at a time ([rows, tile] fp32)


class VocabSoftmaxCE(torch.autograd.Function):
    """ce[r] = logsumexp_v(h_r . W_v + b_v) - (h_r . W_t + b_t), t = target[r]: nn.Linear(K, V) followed by
    F.cross_entropy(reduction='none') (deepctr/xdeepfm_pro/sfg_decoder.py:146-149, :277-283) WITHOUT the [rows, V]
    logits: the vocabulary is walked in tiles with an online log-sum-exp, and the backward recomputes each tile
    (softmax - onehot) for the three products.  At Criteo-scale vocabularies the logits of one field would be
    4096 x 10 M x 4 B = 164 GB.  The tile GEMMs are library GEMMs (hipBLASLt); everything stays on the device.
    hidden [rows, K], W [V, K], b [V], target [rows] (ids as float or integer, truncated like Tensor.long())."""

    @staticmethod
    def _tile(rows, V):
        return int(max(1024, min(V, VOCAB_TILE_BYTES // (4 * max(rows, 1)))))

    @staticmethod
    def forward(ctx, hidden, W, b, target):
        rows, V = hidden.shape[0], W.shape[0]
        tgt = target.long()
        T = VocabSoftmaxCE._tile(rows, V)
        m = torch.full((rows,), float("-inf"), dtype=torch.float32, device=hidden.device)
        ssum = torch.zeros(rows, dtype=torch.float32, device=hidden.device)
        lib = _lib.load()
        for v0 in range(0, V, T):
            z = torch.addmm(b[v0:v0 + T], hidden, W[v0:v0 + T].t())
            # one read of the tile: row maxima, then sum of exp against the running maximum (m, ssum updated in place)
            if rows > 0:
                _lib.check(lib.xdfm_vocab_lse_update(_ptr(z), z.stride(0), rows, z.shape[1], _ptr(m), _ptr(ssum), _stream()),
                           "vocab_lse_update")
        lse = m + torch.log(ssum)
        zt = (hidden * W.index_select(0, tgt)).sum(dim=1) + b.index_select(0, tgt)
        ctx.save_for_backward(hidden, W, b, tgt, lse)
        return lse - zt

    @staticmethod
    def backward(ctx, g):
        hidden, W, b, tgt, lse = ctx.saved_tensors
        rows, V = hidden.shape[0], W.shape[0]
        T = VocabSoftmaxCE._tile(rows, V)
        g = g.contiguous()
        dW = torch.empty_like(W) if ctx.needs_input_grad[1] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[2] else None
        dh = torch.zeros_like(hidden) if ctx.needs_input_grad[0] else None
        for v0 in range(0, V, T):
            dz = torch.addmm(b[v0:v0 + T], hidden, W[v0:v0 + T].t())
            if rows > 0:                                                 # g * softmax, in place
                _lib.check(_lib.load().xdfm_vocab_softmax_grad(_ptr(dz), dz.stride(0), rows, dz.shape[1], _ptr(lse), _ptr(g),
                                                               _stream()), "vocab_softmax_grad")
            if dW is not None:
                torch.mm(dz.t(), hidden, out=dW[v0:v0 + T])
            if db is not None:
                torch.sum(dz, dim=0, out=db[v0:v0 + T])
            if dh is not None:
                dh.addmm_(dz, W[v0:v0 + T])
        # - g * onehot(target)
        if dW is not None:
            dW.index_add_(0, tgt, -(g[:, None] * hidden))
        if db is not None:
            db.index_add_(0, tgt, -g)
        if dh is not None:
            dh.sub_(g[:, None] * W.index_select(0, tgt))
        return dh, dW, db, None


def vocab_softmax_ce(hidden, W, b, target):
    _need_cuda(hidden, "decoder hidden layer")
    return VocabSoftmaxCE.apply(hidden, W, b, target)


_VCE_FIELD = np.dtype([("W", "u8"), ("bias", "u8"), ("dW", "u8"), ("db", "u8"), ("ws_off", "i8"), ("V", "i4"), ("vr", "i4"),
                       ("item0", "i4"), ("blk0", "i4")])            # xdfm_vce_field (include/xdfm.h)
_VCE_ITEM = np.dtype([("field", "i4"), ("sb0", "i4"), ("sb1", "i4"), ("range", "i4")])      # xdfm_vce_item
_VCE_PLANS = {}


def _vce_plan(R, K, vocabs, dev):
    """Host tables of xdfm_vocab_ce_plan for (R, K, vocabularies) + the items on the device (they hold no pointers)."""
    key = (R, K, tuple(vocabs), dev)
    plan = _VCE_PLANS.get(key)
    if plan is None:
        lib = _lib.load()
        V = np.asarray(vocabs, dtype=np.int32)
        fields = np.zeros(len(vocabs), dtype=_VCE_FIELD)
        ws, nblk = ctypes.c_long(0), ctypes.c_int(0)
        n = lib.xdfm_vocab_ce_plan(len(vocabs), V.ctypes.data, R, K, fields.ctypes.data, None, 0, ctypes.byref(ws), ctypes.byref(nblk))
        if n <= 0:
            raise _lib.XdfmError("vocab_ce_plan: " + lib.xdfm_last_error().decode("utf-8", "replace"))
        items = np.zeros(n, dtype=_VCE_ITEM)
        lib.xdfm_vocab_ce_plan(len(vocabs), V.ctypes.data, R, K, fields.ctypes.data, items.ctypes.data, n, ctypes.byref(ws),
                               ctypes.byref(nblk))
        items_dev = torch.from_numpy(items.view(np.uint8)).to(dev)
        if len(_VCE_PLANS) > 64:               # the dynamic route asks for a new row count almost every step; a plan a captured
            _VCE_PLANS.clear()                 # step uses is also held by its VocabHeadsState, which never lets go of it
        plan = _VCE_PLANS[key] = (fields, items_dev, int(n), int(ws.value), int(nblk.value))
    return plan


def _vce_fields(plan, Ws, bs, dWs, dbs, dev):
    fields = plan[0].copy()
    fields["W"] = [w.data_ptr() for w in Ws]
    fields["bias"] = [b.data_ptr() for b in bs]
    fields["dW"] = [0 if t is None else t.data_ptr() for t in dWs]
    fields["db"] = [0 if t is None else t.data_ptr() for t in dbs]
    return torch.from_numpy(fields.view(np.uint8)).to(dev)


class VocabHeadsState:
    """What `VocabHeadsCE` keeps across steps for one set of heads (a model owns one): the gradient tensors of the head
    parameters and, per (capacity, K), the field table on the device.  The table holds the pointers of W, bias, dW and
    db; all four are stable from step to step, so it is uploaded once -- outside any graph capture -- and again only
    when a pointer changed (`EmbedPlan.pointer_table` is the same pattern).  The forward and the backward read the same
    table.  The gradients handed to autograd are fresh views of the kept tensors: a second backward before the optimizer
    step would overwrite the first one's result, so the state serves a train step with ONE backward per forward (the
    models pass it inside their own step only; everything else allocates per call)."""

    def __init__(self):
        self.grads = None        # (key, dWs, dbs)
        # (plan key, pointers) -> (plan, device table).  Nothing is ever evicted: a captured train step addresses the
        # plan's work items, the table and the gradient tensors by raw pointer and replays without running Python, so
        # this object is their only owner for as long as the model lives.  One entry per batch shape (a few hundred
        # bytes each) and per set of parameter addresses.
        self.tables = {}
        self.current = {}        # plan key -> the pointers of the table in use
        self.retired = []        # gradient tensors replaced after the parameters moved

    def grad_buffers(self, Ws, bs):
        key = tuple((t.data_ptr(), tuple(t.shape), t.device) for t in tuple(Ws) + tuple(bs))
        if self.grads is None or self.grads[0] != key:
            if self.grads is not None:
                self.retired.append(self.grads)
            self.grads = (key, [torch.empty_like(w) for w in Ws], [torch.empty_like(b) for b in bs])
        return self.grads[1], self.grads[2]

    def table(self, plan_key, Ws, bs, dWs, dbs, dev):
        """(plan, device table) for this capacity and these tensors."""
        ptrs = tuple(t.data_ptr() for t in tuple(Ws) + tuple(bs) + tuple(dWs) + tuple(dbs))
        hit = self.tables.get((plan_key, ptrs))
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("xdfm: the vocabulary heads' field table is stale inside a graph capture -- run the step "
                                   "once eagerly with these parameters and this batch shape before capturing it")
            R, K, vocabs, _ = plan_key
            plan = _vce_plan(R, K, list(vocabs), dev)
            hit = self.tables[(plan_key, ptrs)] = (plan, _vce_fields(plan, Ws, bs, dWs, dbs, dev))
        self.current[plan_key] = ptrs
        return hit


class VocabHeadsCE(torch.autograd.Function):
    """ce[f][r] of ALL sparse fields' heads over the same hidden rows, logits never in HBM (csrc/vocab_ce_x3.hip; the
    heads of deepctr/xdeepfm_pro/sfg_decoder.py:146-149 + F.cross_entropy of :277-283).  hidden [R, K] (K = 32 or 64),
    targets [F, R] int64, n_rows (None, or one int32 on the device: the rows in use, R is then a capacity -- rows behind the
    count are never read, their ce and dh are exact zeros, they add nothing to dW / db, and every launch and shape is that
    of the capacity), state (None or a `VocabHeadsState`), then the F weights [V_f, K] and the F biases [V_f].  The hidden
    layer is packed into MFMA fragments once per pass; all fields share each launch (a table of per-field pointers and
    work items): log-sum-exp partials + merge in the forward; in the backward the hidden gradient (partial slabs summed in
    a fixed order) and the weight / bias gradients (every row written once, the target's -g included)."""

    calls = 0                 # forward passes taken (tests assert that a golden reached this path)

    @staticmethod
    def forward(ctx, hidden, targets, n_rows, state, *params):
        lib = _lib.load()
        VocabHeadsCE.calls += 1
        F_ = len(params) // 2
        Ws, bs = params[:F_], params[F_:]
        R, K = hidden.shape
        dev = hidden.device
        hidden = hidden.contiguous()
        targets = targets.contiguous()
        for t in params:
            if not t.is_contiguous():
                raise ValueError("xdfm: head parameters must be contiguous")
        if n_rows is not None and not (n_rows.is_cuda and n_rows.dtype == torch.int32 and n_rows.numel() == 1):
            raise ValueError("xdfm: n_rows must be one int32 on the device")
        plan_key = (R, K, tuple(w.shape[0] for w in Ws), dev)
        need = ctx.needs_input_grad
        # kept gradient tensors only when nothing is accumulated into: a .grad left in place would alias them
        if state is not None and all(need[4:]) and all(p.grad is None for p in params):
            dWs, dbs = state.grad_buffers(Ws, bs)
            plan, fields = state.table(plan_key, Ws, bs, dWs, dbs, dev)
            ctx.kept = (fields, dWs, dbs)
        else:
            plan = _vce_plan(R, K, [w.shape[0] for w in Ws], dev)
            fields = _vce_fields(plan, Ws, bs, [None] * F_, [None] * F_, dev)
            ctx.kept = None
        pack = torch.empty(lib.xdfm_vocab_ce_pack_elems(R, K), dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_vocab_ce_pack_hidden_n(_ptr(hidden), K, R, K, _ptr(pack), _ptr(n_rows), _stream()), "vocab_ce_pack_hidden")
        Rpad = lib.xdfm_vocab_ce_rows_padded(R)
        ce = torch.empty(F_, R, dtype=torch.float32, device=dev)
        lse2 = torch.empty(F_, Rpad, dtype=torch.float32, device=dev)
        wmax = torch.empty(F_, dtype=torch.int32, device=dev)
        ws = torch.empty(plan[3], dtype=torch.float32, device=dev)
        flops = 2.0 * R * K * sum(w.shape[0] for w in Ws)                  # of the reference's nn.Linear, all heads
        _lib.check(_run("vocab_ce_fwd", flops, lambda: lib.xdfm_vocab_ce_fwd_n(
            _ptr(pack), _ptr(hidden), K, R, K, _ptr(fields), F_, _ptr(plan[1]), plan[2], _ptr(targets), _ptr(ws), _ptr(ce), _ptr(lse2),
            _ptr(wmax), _ptr(n_rows), _stream())), "vocab_ce_fwd")
        ctx.save_for_backward(hidden, targets, pack, lse2, wmax, *params)
        ctx.plan = plan
        ctx.n_rows = n_rows
        return ce

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        hidden, targets, pack, lse2, wmax = ctx.saved_tensors[:5]
        params = ctx.saved_tensors[5:]
        F_ = len(params) // 2
        Ws, bs = params[:F_], params[F_:]
        R, K = hidden.shape
        dev = hidden.device
        plan = ctx.plan
        n_rows = ctx.n_rows
        g = g.contiguous()
        Rpad = lib.xdfm_vocab_ce_rows_padded(R)
        gpack = torch.empty(F_ * (4 + Rpad), dtype=torch.float32, device=dev)
        flops = 2.0 * R * K * sum(w.shape[0] for w in Ws)     # per product of the reference's backward (dH; dW), recompute not counted
        _lib.check(lib.xdfm_vocab_ce_pack_g_n(_ptr(g), F_, R, _ptr(gpack), _ptr(n_rows), _stream()), "vocab_ce_pack_g")
        if ctx.kept is not None:
            fields, dWs, dbs = ctx.kept
        else:
            dWs = [torch.empty_like(Ws[f]) if ctx.needs_input_grad[4 + f] else None for f in range(F_)]
            dbs = [torch.empty_like(bs[f]) if ctx.needs_input_grad[4 + F_ + f] else None for f in range(F_)]
            fields = _vce_fields(plan, Ws, bs, dWs, dbs, dev)
        dh = None
        if ctx.needs_input_grad[0]:
            dh = torch.empty_like(hidden)
            ws = torch.empty(plan[3], dtype=torch.float32, device=dev)
            _lib.check(_run("vocab_ce_bwd_h", flops, lambda: lib.xdfm_vocab_ce_bwd_h_n(
                _ptr(pack), R, K, _ptr(fields), F_, _ptr(plan[1]), plan[2], _ptr(targets), _ptr(g), _ptr(gpack), _ptr(lse2), _ptr(wmax),
                _ptr(ws), _ptr(dh), K, _ptr(n_rows), _stream())), "vocab_ce_bwd_h")
        if any(t is not None for t in dWs + dbs):
            _lib.check(_run("vocab_ce_bwd_w", flops, lambda: lib.xdfm_vocab_ce_bwd_w_n(
                _ptr(pack), R, K, _ptr(fields), F_, plan[4], _ptr(targets), _ptr(gpack), _ptr(lse2), _ptr(wmax), _ptr(n_rows),
                _stream())), "vocab_ce_bwd_w")
        if ctx.kept is not None:                  # fresh views: autograd may adopt them as .grad without a copy
            dWs, dbs = [t.view_as(t) for t in dWs], [t.view_as(t) for t in dbs]
        return (dh, None, None, None, *dWs, *dbs)


def vocab_heads_ce_supported(K: int) -> bool:
    return bool(_lib.load().xdfm_vocab_ce_x3_supported(int(K)))


def vocab_heads_ce(hidden, targets, weights, biases, n_rows=None, state=None):
    """[F, R] cross-entropies of F heads (weights[f] [V_f, K], biases[f] [V_f]) over hidden [R, K], targets [F, R] int64.
    n_rows: one int32 on the device = the rows in use (R is a capacity then); state: a `VocabHeadsState` kept by the caller."""
    _need_cuda(hidden, "decoder hidden layer")
    return VocabHeadsCE.apply(hidden, targets, n_rows, state, *weights, *biases)


# --------------------------------------------------------------------------------------------- #
# positive-row compaction                                                                        #
# --------------------------------------------------------------------------------------------- #
class CompactRows(torch.autograd.Function):
    """K11 (csrc/compact.hip): the rows of a batch whose label is 1 (or all rows), moved to the front of tensors that keep
    the batch's capacity B, in the order torch.nonzero gives; the count stays on the device.  X [B, cols] (any row
    stride), dnn_in [B, W], y [B], cols (device int32 [F]: the id column of each sparse field) ->
    (n_rows [1] int32, inv_n [1] = 1 / (n + 1e-8) or 1 / B, valid [B] 1 / 0, d_rows [B, W] with exact zeros behind the
    count, labels [B], targets [F, B] int64).  Only d_rows is differentiable: the backward hands dnn_in a full [B, W]
    gradient, the selected rows' rows of d(d_rows) and zeros elsewhere.  With `count_y` (float labels of the GLOBAL batch
    of a row-parallel step, any length) inv_n = 1 / (#{count_y == 1} + 1e-8) or 1 / count_y.numel(); everything else still
    comes from y.  The kernel reads count_y from the device at every launch, so a captured step follows its contents."""

    @staticmethod
    def forward(ctx, X, dnn_in, y, cols, positive_only, count_y=None):
        lib = _lib.load()
        B, W = dnn_in.shape
        dev = dnn_in.device
        F_ = int(cols.numel())
        if X.stride(1) != 1 or X.stride(0) < X.shape[1]:
            X = X.contiguous()
        if dnn_in.stride(1) != 1 or dnn_in.stride(0) < W:
            dnn_in = dnn_in.contiguous()
        y = y.reshape(-1).contiguous()
        if y.numel() != B or X.shape[0] != B:
            raise ValueError("xdfm: compact_rows needs one label per row, got %d labels for %d rows" % (y.numel(), B))
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        pos, n_rows = torch.empty(B, **i32), torch.empty(1, **i32)
        inv_n, valid, labels = torch.empty(1, **f32), torch.empty(B, **f32), torch.empty(B, **f32)
        d_rows = torch.empty(B, W, **f32)
        targets = torch.empty(F_, B, dtype=torch.int64, device=dev)
        if count_y is None:
            _lib.check(lib.xdfm_compact_rows_fwd(_ptr(X), X.stride(0), X.shape[1], _ptr(dnn_in), dnn_in.stride(0), _ptr(y), B, W,
                                                 _ptr(cols), F_, 1 if positive_only else 0, _ptr(pos), _ptr(n_rows), _ptr(inv_n),
                                                 _ptr(valid), _ptr(d_rows), _ptr(labels), _ptr(targets), _stream()), "compact_rows_fwd")
        else:
            _lib.check(lib.xdfm_compact_rows_fwd_n(_ptr(X), X.stride(0), X.shape[1], _ptr(dnn_in), dnn_in.stride(0), _ptr(y), B, W,
                                                   _ptr(cols), F_, 1 if positive_only else 0, _ptr(count_y), count_y.numel(),
                                                   _ptr(pos), _ptr(n_rows), _ptr(inv_n), _ptr(valid), _ptr(d_rows), _ptr(labels),
                                                   _ptr(targets), _stream()), "compact_rows_fwd_n")
        ctx.save_for_backward(pos)
        ctx.mark_non_differentiable(n_rows, inv_n, valid, labels, targets)
        return n_rows, inv_n, valid, d_rows, labels, targets

    @staticmethod
    def backward(ctx, _gn, _gi, _gv, g, _gl, _gt):
        if g is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        lib = _lib.load()
        pos, = ctx.saved_tensors
        B, W = g.shape
        if g.stride(1) != 1 or g.stride(0) < W:
            g = g.contiguous()
        d_dnn = torch.empty(B, W, dtype=torch.float32, device=g.device)
        _lib.check(lib.xdfm_compact_rows_bwd(_ptr(g), g.stride(0), _ptr(pos), B, W, _ptr(d_dnn), _stream()), "compact_rows_bwd")
        return None, d_dnn, None, None, None, None


def compact_rows(X, dnn_in, y, cols, positive_only=True, count_y=None):
    y = y.to(torch.float32)             # K11 reads float labels; `labels == 1` of the dynamic route takes any dtype
    _need_cuda(dnn_in, "decoder input")
    _need_cuda(X, "model input")
    _need_cuda(y, "labels")
    if count_y is not None:
        _need_cuda(count_y, "labels of the global batch")
        if count_y.dtype != torch.float32 or not count_y.is_contiguous() or count_y.numel() < 1:
            # no silent copy: a captured step must keep reading the caller's buffer
            raise ValueError("xdfm: compact_rows needs count_y as a non-empty contiguous float32 tensor")
    return CompactRows.apply(X, dnn_in, y, cols, bool(positive_only), count_y)


# --------------------------------------------------------------------------------------------- #
# AutoDis                                                                                        #
# --------------------------------------------------------------------------------------------- #
def autodis_supported(K: int, D: int) -> bool:
    """True when csrc/autodis.hip serves K buckets and embedding width D (1 <= K <= 32, 1 <= D <= 64)."""
    return bool(_lib.load().xdfm_autodis_supported(int(K), int(D)))


def _autodis_table(proj, dev, cache: dict):
    """Device array of the 4 * F projector pointers, kept in `cache` and rebuilt only when a data_ptr changes
    (load_state_dict into fresh storage, .to()).  The rebuild is a blocking host-to-device copy, so it must happen
    outside a graph capture: run the op once eagerly first."""
    key = (dev,) + tuple(t.data_ptr() for t in proj)
    hit = cache.get("autodis_table")
    if hit is not None and hit[0] == key:
        return hit[1]
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("xdfm: the AutoDis pointer table is stale inside a graph capture -- call the layer once eagerly "
                           "with these parameters before capturing it")
    table = torch.tensor(key[1:], dtype=torch.int64).to(dev)
    cache["autodis_table"] = (key, table)
    return table


class AutoDis(torch.autograd.Function):
    """out [B, F * D] of AutoDisLayer (deepctr/xdeepfm_pro/autodis.py:99-125) for all F fields in one launch, backward in one
    launch + a fixed-order finish (csrc/autodis.hip).  x [B, F] (any row stride: the dense columns of a wider matrix
    are read in place), meta [F, K, D], temp [F], table (_autodis_table), then per field Linear(1,K).weight, .bias,
    Linear(K,K).weight, .bias.  Only x is kept for the backward; the gradients come back as views of one flat buffer."""

    calls = 0                 # forward passes taken (tests assert that a model reached this path)

    @staticmethod
    def forward(ctx, x, meta, temp, table, *proj):
        lib = _lib.load()
        AutoDis.calls += 1
        B, F_ = x.shape
        _, K, D = meta.shape
        if x.stride(1) != 1 or x.stride(0) < F_:
            x = x.contiguous()
        for t in (meta, temp) + proj:
            if not t.is_contiguous():
                raise ValueError("xdfm: AutoDis parameters must be contiguous")
        out = torch.empty(B, F_ * D, dtype=torch.float32, device=x.device)
        _lib.check(lib.xdfm_autodis_fwd(_ptr(x), x.stride(0), B, F_, K, D, _ptr(meta), _ptr(table), _ptr(temp), _ptr(out), _stream()),
                   "autodis_fwd")
        ctx.save_for_backward(x, meta, temp, table, *proj)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, meta, temp, table = ctx.saved_tensors[:4]
        B, F_ = x.shape
        _, K, D = meta.shape
        need = ctx.needs_input_grad
        pneed = [any(need[4 + 4 * f + i] for f in range(F_)) for i in range(4)]
        flags = (1 if need[1] else 0) | (2 if pneed[0] else 0) | (4 if pneed[1] else 0) | (8 if pneed[2] else 0) | \
            (16 if pneed[3] else 0) | (32 if need[2] else 0) | (64 if need[0] else 0)
        if flags == 0:
            return (None,) * (4 + 4 * F_)
        if g.stride(1) != 1 or g.stride(0) < F_ * D:
            g = g.contiguous()
        dev = x.device
        grads = ws = dx = None
        if flags & 63:
            grads = torch.empty(F_ * (K * D + K * K + 3 * K + 1), dtype=torch.float32, device=dev)
            ws = torch.empty(lib.xdfm_autodis_ws_elems(B, F_, K, D), dtype=torch.float32, device=dev)
        if flags & 64:
            dx = torch.empty(B, F_, dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_autodis_bwd(_ptr(x), x.stride(0), B, F_, K, D, _ptr(meta), _ptr(table), _ptr(temp), _ptr(g), g.stride(0),
                                        flags, _ptr(ws), _ptr(grads), _ptr(dx), _stream()), "autodis_bwd")
        FK, FKD, FKK = F_ * K, F_ * K * D, F_ * K * K
        dmeta = grads[:FKD].view(F_, K, D) if need[1] else None
        dtemp = grads[FKD + 3 * FK + FKK:] if need[2] else None
        dproj = []
        for f in range(F_):
            parts = (grads[FKD + f * K:FKD + (f + 1) * K].view(K, 1) if need[4 + 4 * f] else None,
                     grads[FKD + FK + f * K:FKD + FK + (f + 1) * K] if need[5 + 4 * f] else None,
                     grads[FKD + 2 * FK + f * K * K:FKD + 2 * FK + (f + 1) * K * K].view(K, K) if need[6 + 4 * f] else None,
                     grads[FKD + 2 * FK + FKK + f * K:FKD + 2 * FK + FKK + (f + 1) * K] if need[7 + 4 * f] else None)
            dproj.extend(parts)
        return (dx, dmeta, dtemp, None, *dproj)


def autodis(x, meta, projectors, temp, cache: dict):
    """[B, F * D] AutoDis embeddings of the dense values x [B, F].  projectors: the 4 * F tensors Linear(1,K).weight, .bias,
    Linear(K,K).weight, .bias of each field in turn; cache: a dict the caller keeps (it holds the device pointer table)."""
    _need_cuda(x, "dense values")
    return AutoDis.apply(x, meta, temp, _autodis_table(projectors, x.device, cache), *projectors)


# --------------------------------------------------------------------------------------------- #
# L2 regulariser                                                                                 #
# --------------------------------------------------------------------------------------------- #
class L2Plan:
    """Device-side description (pointers, sizes, strengths) of the tensors one L2 term covers."""

    def __init__(self, coeffs: Sequence[float]):
        self.coeffs = [float(c) for c in coeffs]
        self._key = None
        self._dev = None

    def tables(self, tensors: Sequence[torch.Tensor]):
        key = tuple((t.data_ptr(), t.numel()) for t in tensors)
        if key != self._key:
            dev = tensors[0].device
            offs, off = [], 0
            for k in key:
                offs.append(off)
                off += k[1]
            self._dev = (torch.tensor([k[0] for k in key], dtype=torch.int64, device=dev),
                         torch.tensor([k[1] for k in key], dtype=torch.int64, device=dev),
                         torch.tensor(self.coeffs, dtype=torch.float32, device=dev))
            self._offsets = (offs, off, torch.tensor(offs, dtype=torch.int64, device=dev))
            self._key = key
        return self._dev

    def offsets(self):
        return self._offsets


class L2Reg(torch.autograd.Function):
    """sum_t coeff_t * sum(w_t^2) -> tensor of shape [1]  (deepctr/models/basemodel.py:412-428, l1 == 0).

    `defer` = (EmbedPlan, L2Plan of the first n_defer tensors, L2Plan of the others) or None.  When
    given, the first n_defer tensors are exactly the tables of that gather, in its order: their L2
    gradient is not returned here but handed to EmbedGather.backward, which uses it as the initial
    content of the dense table gradients it has to build anyway.  Only the model's own train step
    passes `defer` (it guarantees that the gather's backward runs in the same pass)."""

    @staticmethod
    def forward(ctx, plan: L2Plan, defer, n_defer, *tensors):
        lib = _lib.load()
        for t in tensors:
            _need_cuda(t, "regularised tensor")
            if not t.is_contiguous():
                raise ValueError("xdfm: regularised tensors must be contiguous")
        ptrs, numel, coeff = plan.tables(tensors)
        T = len(tensors)
        dev = tensors[0].device
        partials = torch.empty(32 * T, dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(lib.xdfm_l2_reg_fwd(_ptr(ptrs), _ptr(numel), _ptr(coeff), T, _ptr(partials), _ptr(out), _stream()),
                   "l2_reg_fwd")
        ctx.plan, ctx.defer, ctx.n_defer = plan, defer, n_defer
        ctx.save_for_backward(*tensors)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        tensors = ctx.saved_tensors
        gs = g.reshape(1).contiguous()
        skip, plan = 0, ctx.plan
        if ctx.defer is not None:
            embed_plan, sub_plan, plan = ctx.defer
            embed_plan.reg_defer = (gs, sub_plan)
            skip = ctx.n_defer
        rest = tensors[skip:]
        grads = [None] * skip
        if rest:
            ptrs, numel, coeff = plan.tables(rest)
            offs, total, off_dev = plan.offsets()
            flat = torch.empty(total, dtype=torch.float32, device=rest[0].device)
            _lib.check(lib.xdfm_l2_reg_bwd(_ptr(ptrs), _ptr(numel), _ptr(coeff), len(rest), _ptr(gs), _ptr(flat),
                                           _ptr(off_dev), 0, _stream()), "l2_reg_bwd")
            grads += [flat[o:o + t.numel()].view(t.shape) for o, t in zip(offs, rest)]
        return (None, None, None) + tuple(grads)


def l2_regulariser(tensors, coeffs, cache: dict, embed_plan=None, n_defer=0):
    """Evaluate the L2 term with plans cached in `cache` (a dict owned by the model)."""
    n_defer = n_defer if embed_plan is not None else 0
    key = (tuple(float(c) for c in coeffs), n_defer)
    plans = cache.get(key)
    if plans is None:
        plans = cache[key] = (L2Plan(coeffs), L2Plan(coeffs[:n_defer]) if n_defer else None,
                              L2Plan(coeffs[n_defer:]) if n_defer and len(coeffs) > n_defer else None)
    full, sub, rest = plans
    defer = (embed_plan, sub, rest) if n_defer else None
    return L2Reg.apply(full, defer, n_defer, *tensors)


# --------------------------------------------------------------------------------------------- #
# per-batch training metrics (K14, csrc/metrics.hip)                                             #
# --------------------------------------------------------------------------------------------- #
# XDFM_METRICS_NATIVE (default 1): `fit(verbose > 0)` takes the per-step logloss / AUC / mse / accuracy of a batch from
# `batch_metrics` (two launches for all of them) instead of the float64 compositions of metrics.py (*_device) and, for the
# accuracy, a host copy with its sync.  Read once, at import; a module attribute the tests and tools/metrics_probe.py flip.
# The default follows profiles/metrics_probe.md.
METRICS_NATIVE = _env_switch(os.environ, "XDFM_METRICS_NATIVE")
METRIC_LOGLOSS, METRIC_AUC, METRIC_MSE, METRIC_ACC = 1, 2, 4, 8         # XDFM_METRIC_* of include/xdfm.h: slot k is bit 1 << k
METRICS_MAX_ROWS = 65536
_METRICS_WS = {}


def batch_metrics_supported(y, p):
    """Can `batch_metrics` take this (labels, predictions) pair?  fp32 device tensors of one numel within the kernel's cap."""
    return bool(isinstance(y, torch.Tensor) and isinstance(p, torch.Tensor) and y.is_cuda and p.is_cuda and y.device == p.device
                and y.dtype == torch.float32 and p.dtype == torch.float32 and y.numel() == p.numel()
                and 1 <= y.numel() <= METRICS_MAX_ROWS)


def batch_metrics(y, p, which, out):
    """out[k] = metric k of (y, p) for every bit k of `which` (logloss | auc | mse | accuracy; xdfm_batch_metrics): two launches
    on the current stream, nothing reaches the host.  y, p: fp32 device tensors of equal numel (any shape; at most 65536
    elements); out: a float64 [4] view on the same device, whose other slots keep their values.  One workspace per device,
    sized for the cap, is kept: calls on one stream follow each other, which is how `fit` uses it."""
    _need_cuda(y, "y")
    _need_cuda(p, "p")
    if y.numel() != p.numel() or y.device != p.device:
        raise ValueError("xdfm batch_metrics: y has %d elements on %s, p %d on %s" % (y.numel(), y.device, p.numel(), p.device))
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.numel() == 4 and out.is_contiguous()
            and out.device == y.device):
        raise ValueError("xdfm batch_metrics: out must be a contiguous float64 [4] view on %s" % (y.device,))
    lib = _lib.load()
    y, p = y.detach().reshape(-1), p.detach().reshape(-1)
    y = y if y.is_contiguous() else y.contiguous()
    p = p if p.is_contiguous() else p.contiguous()
    B = y.numel()
    if lib.xdfm_batch_metrics_ws_bytes(B, int(which)) == 0:
        raise ValueError("xdfm batch_metrics: B=%d, which=%d outside the supported range (1 <= B <= %d, 1 <= which <= 15)"
                         % (B, int(which), METRICS_MAX_ROWS))
    idx = y.device.index if y.device.index is not None else torch.cuda.current_device()
    ws = _METRICS_WS.get(idx)
    if ws is None:
        ws = torch.empty(lib.xdfm_batch_metrics_ws_bytes(METRICS_MAX_ROWS, 15) // 8, dtype=torch.float64, device=y.device)
        if not torch.cuda.is_current_stream_capturing():          # a tensor born inside a capture belongs to that graph's pool
            _METRICS_WS[idx] = ws
    _lib.check(_run("batch_metrics", 0.0, lambda: lib.xdfm_batch_metrics(_ptr(y), _ptr(p), B, int(which), _ptr(ws), _ptr(out), _stream())),
               "batch_metrics")
    return out


# --------------------------------------------------------------------------------------------- #
# evaluation metrics for any row count (K14s, csrc/eval_metrics.hip)                             #
# --------------------------------------------------------------------------------------------- #
# XDFM_EVAL_NATIVE: `evaluate` (and with it the validation of `fit`) keeps the predictions on the device and takes logloss /
# AUC / mse / accuracy from one `eval_metrics` call (a radix sort for the AUC) instead of copying the predictions to the host
# and running the numpy functions of metrics.py there.  Read once, at import; a module attribute the tests and
# tools/eval_probe.py flip.  The default follows profiles/eval_probe.md.
EVAL_NATIVE = _env_switch(os.environ, "XDFM_EVAL_NATIVE", default=True)
EVAL_MAX_ROWS = 1 << 27
_EVAL_WS = {}


def eval_metrics_supported(y, p):
    """Can `eval_metrics` take this (labels, predictions) pair?  fp32, contiguous, 1-D device tensors of one length within the
    kernel's cap."""
    return bool(isinstance(y, torch.Tensor) and isinstance(p, torch.Tensor) and y.is_cuda and p.is_cuda and y.device == p.device
                and y.dtype == torch.float32 and p.dtype == torch.float32 and y.dim() == 1 and p.dim() == 1
                and y.is_contiguous() and p.is_contiguous() and y.numel() == p.numel() and 1 <= y.numel() <= EVAL_MAX_ROWS)


def eval_metrics(y, p, which):
    """A float64 [4] device tensor whose slot k holds metric k of (y, p) for every bit k of `which` (logloss | auc | mse |
    accuracy; xdfm_eval_metrics) and NaN elsewhere: launches on the current stream, nothing reaches the host.  y, p: what
    `eval_metrics_supported` accepts.  One workspace per device is kept and grown on demand: calls on one stream follow each
    other."""
    _need_cuda(y, "y")
    _need_cuda(p, "p")
    if not eval_metrics_supported(y, p):
        raise ValueError("xdfm eval_metrics: y %s on %s and p %s on %s must be contiguous 1-D tensors of one length in [1, %d]"
                         % (tuple(y.shape), y.device, tuple(p.shape), p.device, EVAL_MAX_ROWS))
    lib = _lib.load()
    y, p = y.detach(), p.detach()
    N = y.numel()
    need = lib.xdfm_eval_metrics_ws_bytes(N, int(which))
    if need == 0:
        raise ValueError("xdfm eval_metrics: N=%d, which=%d outside the supported range (1 <= N <= %d, 1 <= which <= 15)"
                         % (N, int(which), EVAL_MAX_ROWS))
    idx = y.device.index if y.device.index is not None else torch.cuda.current_device()
    ws = _EVAL_WS.get(idx)
    if ws is None or ws.numel() * 8 < need:
        ws = None
        _EVAL_WS.pop(idx, None)                                   # both references go: the smaller one is freed before the larger one comes
        ws = torch.empty(need // 8, dtype=torch.float64, device=y.device)
        if not torch.cuda.is_current_stream_capturing():          # a tensor born inside a capture belongs to that graph's pool
            _EVAL_WS[idx] = ws
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=y.device)
    _lib.check(_run("eval_metrics", 0.0, lambda: lib.xdfm_eval_metrics(_ptr(y), _ptr(p), N, int(which), _ptr(ws), _ptr(out), _stream())),
               "eval_metrics")
    return out


# --------------------------------------------------------------------------------------------- #
# sample-weighted evaluation metrics (K14w, csrc/eval_metrics_w.hip)                             #
# --------------------------------------------------------------------------------------------- #
# XDFM_EVAL_W_NATIVE: the `weighted_*` entries of `evaluate` and of the per-batch log of `fit` (compile(weighted_metrics=...))
# come from one `eval_metrics_w` call on the device instead of metrics.py's weighted numpy functions on host copies.  Read once,
# at import; a module attribute the tests and tools/weighted_eval_probe.py flip.  The default follows
# profiles/weighted_eval_probe.md.
EVAL_W_NATIVE = _env_switch(os.environ, "XDFM_EVAL_W_NATIVE", default=True)
_EVAL_W_WS = {}


def eval_metrics_w_supported(y, p, w):
    """Can `eval_metrics_w` take this (labels, predictions, weights) triple?  What `eval_metrics_supported` asks of (y, p), and
    the same of w."""
    return bool(eval_metrics_supported(y, p) and isinstance(w, torch.Tensor) and w.is_cuda and w.device == y.device
                and w.dtype == torch.float32 and w.dim() == 1 and w.is_contiguous() and w.numel() == y.numel())


def eval_metrics_w(y, p, w, which, out=None):
    """`eval_metrics` with one weight per row (xdfm_eval_metrics_w): a float64 [4] device tensor, slot k the weighted metric k
    for every bit k of `which` and NaN elsewhere; launches on the current stream, nothing reaches the host.  w: finite and
    >= 0 -- the caller's contract (`models.example_weights` checks it on the host).  Its own workspace per device, grown on
    demand.  out: a contiguous float64 [4] device tensor (a row of `fit`'s log) to write the named slots into instead; its
    other slots keep what they hold."""
    _need_cuda(y, "y")
    _need_cuda(p, "p")
    _need_cuda(w, "w")
    if not eval_metrics_w_supported(y, p, w):
        raise ValueError("xdfm eval_metrics_w: y %s on %s, p %s on %s and w %s on %s must be contiguous 1-D float32 tensors of one "
                         "length in [1, %d]" % (tuple(y.shape), y.device, tuple(p.shape), p.device, tuple(w.shape), w.device,
                                                EVAL_MAX_ROWS))
    lib = _lib.load()
    y, p, w = y.detach(), p.detach(), w.detach()
    N = y.numel()
    need = lib.xdfm_eval_metrics_w_ws_bytes(N, int(which))
    if need == 0:
        raise ValueError("xdfm eval_metrics_w: N=%d, which=%d outside the supported range (1 <= N <= %d, 1 <= which <= 15)"
                         % (N, int(which), EVAL_MAX_ROWS))
    idx = y.device.index if y.device.index is not None else torch.cuda.current_device()
    ws = _EVAL_W_WS.get(idx)
    if ws is None or ws.numel() * 8 < need:
        ws = None
        _EVAL_W_WS.pop(idx, None)                                 # both references go: the smaller one is freed before the larger one comes
        ws = torch.empty(need // 8, dtype=torch.float64, device=y.device)
        if not torch.cuda.is_current_stream_capturing():          # a tensor born inside a capture belongs to that graph's pool
            _EVAL_W_WS[idx] = ws
    if out is None:
        out = torch.full((4,), float("nan"), dtype=torch.float64, device=y.device)
    elif not (out.is_cuda and out.device == y.device and out.dtype == torch.float64 and out.shape == (4,) and out.is_contiguous()):
        raise ValueError("xdfm eval_metrics_w: out must be a contiguous float64 [4] tensor on %s" % (y.device,))
    _lib.check(_run("eval_metrics_w", 0.0,
                    lambda: lib.xdfm_eval_metrics_w(_ptr(y), _ptr(p), _ptr(w), N, int(which), _ptr(ws), _ptr(out), _stream())),
               "eval_metrics_w")
    return out
