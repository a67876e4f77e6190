"""torch.optim.Adam whose step is the library's streaming kernel (K7, `xdfm_adam_step`): one launch per 52
tensors for every fp32 CUDA parameter -- at BASELINE config 2 the embedding / linear tables are 44 M of the 45 M
parameters, ATen's multi-tensor kernel moves them at 3.2 TB/s, K7 at 5.7 TB/s, and the ~15 small tensors stop
costing a 47 us latency-bound launch of their own.  State layout (`step`, `exp_avg`, `exp_avg_sq` per
parameter, device-resident fp32 step counters) and hyper-parameters are torch's, so `state_dict()` /
`load_state_dict()` and code that edits `param_groups` keep working; anything the kernel does not implement
(amsgrad, weight decay, maximize, tensor learning rates, non-fp32 parameters) falls back to
`torch.optim.Adam.step`.  The update rule is the one basemodel.py:452 selects (torch.optim.Adam, defaults).

The model's own train step may *arm* an L2 term for one step (`arm_l2`): K7 then adds 2*l2*w to the gradients
while it streams the weights and returns the term's value (`l2_value`), which removes the regulariser's own
passes over the parameters (basemodel.py:412-428) from the step.

Gradients that are views of a kept gradient buffer (`ops.GradArena`, registered through `grad_sources`) are read by
their chunk marks: K7 skips the untouched rows of the dense table gradients and re-zeroes the touched ones.

`TableSGD`, `TableAdagrad` and `TableRMSprop` (K7s / K7g / K7r, `xdfm_sgd_step` / `xdfm_adagrad_step` / `xdfm_rmsprop_step`;
TableSGD with a momentum: K7m, `xdfm_sgdm_step`)
give the other optimizer strings of basemodel.py:447-461 (`--optimizer sgd|adagrad|rmsprop`) the same sweep, armed L2 term,
marked gradients and device-resident learning rate; their state layout is that of torch.optim.SGD / Adagrad / RMSprop.
Tables with an L2 term may take the deferred (exact) form of those steps (K7sd / K7gd / K7rd, `xdfm_sgd_step_deferred` /
`xdfm_adagrad_step_deferred` / `xdfm_rmsprop_step_deferred`), as TableAdam's do.

`TableFTRL` (K7f, `xdfm_ftrl_step`) is per-coordinate FTRL-Proximal, which torch does not have: the same sweep over two state
arrays, `z` and `n`; its fallback is the class's own step in torch ops, and it has no deferred form.

`TableRowwiseAdagrad` (K7w, `xdfm_rowwise_adagrad_step`) is row-wise Adagrad, the usual rule for large CTR embedding tables: one
accumulator per table row for the groups marked `rowwise`, K7g for everything else; torch-op fallback, no deferred form.

All six classes are the mixin `_TableStep` in front of the stock class (torch.optim.Optimizer for the two rules torch does not
have): the host scaffold (fields, learning rate on the device, invalidation, flush, backlog, pickling, the armed L2 term) exists
once; a class brings its clock and what its kernel implements, and `KINDS` says which C functions a kernel kind calls and with
which hyper-parameters.  TableAdam keeps a step of its own."""
import ctypes
import os

import torch

from . import _lib

DEFER_CAP = 256          # steps the clock's constant table holds (the `last` bytes count steps since the last flush)
DEFER_MIN_NUMEL = int(os.environ.get("XDFM_ADAM_DEFER_MIN_NUMEL", 1 << 26))   # "auto": tables of fewer parameters in total take the dense sweep
# The floor of "auto" for TableSGD / TableAdagrad (K7sd / K7gd), never below Adam's.  Measured: the sweep wins by
# 5 % at 44 M table parameters, the deferral by 29 % (SGD) / 36 % (Adagrad) at 574 M; the straight line between the two puts
# the crossover near 94 M (SGD) / 79 M (Adagrad).  2^27 is above both.
OPT_DEFER_MIN_NUMEL = max(int(os.environ.get("XDFM_OPT_DEFER_MIN_NUMEL", 1 << 27)), 1 << 26)
ROWS_MIN_NUMEL = 1 << 20  # tables at least this large get the step's update by the batch's rows (XDFM_ADAM_ROWS_MIN_NUMEL overrides)
# XDFM_SGD_MOMENTUM_NATIVE (default 1): TableSGD with 0 < momentum < 1 and dampening 0 (plain or Nesterov) runs K7m / K7md;
# 0 gives the stock torch.optim.SGD.step back for it.  Read once, at import; tools/optim_probe.py and the tests flip this
# attribute to run both routes in one process (a captured graph keeps the route it was captured with).
SGD_MOMENTUM_NATIVE = os.environ.get("XDFM_SGD_MOMENTUM_NATIVE", "1") != "0"


class _Kind(object):
    """A kernel kind of `_TableStep.step`.  step / deferred / catchup / flush: the names of its C functions (None: the kind has no
    such form).  hyper: param group -> the arguments of a step between the rate and the L2 workspace.  lead, replay: the
    arguments of a catch-up and of a flush in front of the common ones (xdfm_opt_*'s `adagrad` flag), and d["eps"] -> those
    behind them.  per_param: descriptor -> bytes the sweep moves per parameter beside the gradient (the byte model of
    DESIGN.md).  skip: an unmarked chunk of a tensor without an L2 term is an exact no-op that the sweep does not read (the
    rule's SKIP in csrc/; not RMSprop, whose accumulator decays, nor SGDM, whose buffer moves its weight, in every step)."""

    def __init__(self, step, hyper, per_param, skip=True, deferred=None, catchup=None, flush=None, lead=(), replay=None):
        self.step, self.hyper, self.per_param, self.skip = step, hyper, per_param, skip
        self.deferred, self.catchup, self.flush, self.lead, self.replay = deferred, catchup, flush, lead, replay


_eps = lambda g: (float(g["eps"]),)
_eps_replay = lambda e: (float(e or 0.0),)
KINDS = {
    "sgd": _Kind(step="xdfm_sgd_step", hyper=lambda g: (), per_param=lambda a: 8.0,
                 deferred="xdfm_sgd_step_deferred", catchup="xdfm_opt_catchup_rows", flush="xdfm_opt_flush", lead=(0,),
                 replay=_eps_replay),
    "adagrad": _Kind(step="xdfm_adagrad_step", hyper=_eps, per_param=lambda a: 16.0,
                     deferred="xdfm_adagrad_step_deferred", catchup="xdfm_opt_catchup_rows", flush="xdfm_opt_flush", lead=(1,),
                     replay=_eps_replay),
    "rmsprop": _Kind(step="xdfm_rmsprop_step", hyper=lambda g: (float(g["alpha"]), float(g["eps"])), per_param=lambda a: 16.0,
                     skip=False, deferred="xdfm_rmsprop_step_deferred", catchup="xdfm_rmsprop_catchup_rows",
                     flush="xdfm_rmsprop_flush", replay=lambda e: (float(e[0]), float(e[1]))),       # d["eps"]: (alpha, eps)
    "sgdm": _Kind(step="xdfm_sgdm_step", hyper=lambda g: (float(g["momentum"]), int(bool(g["nesterov"]))),
                  per_param=lambda a: 16.0, skip=False, deferred="xdfm_sgdm_step_deferred", catchup="xdfm_sgdm_catchup_rows",
                  flush="xdfm_sgdm_flush", replay=lambda e: (float(e[0]), int(e[1]))),                # d["eps"]: (mu, nesterov)
    "ftrl": _Kind(step="xdfm_ftrl_step", hyper=lambda g: (float(g["l1"]), float(g["l2"]), float(g["beta"])),
                  per_param=lambda a: 24.0),                                                         # p, z and n
    # K7w: p read and written, the row's accumulator once per row
    "rowwise": _Kind(step="xdfm_rowwise_adagrad_step", hyper=_eps, per_param=lambda a: 8.0 + 8.0 / a.dim),
}


def _ptr_tables(struct, ts, ent, cols, tolerate, pad=0):
    """(`struct` over one device array per column, the arrays to keep alive) for the tables `ts` of a gather: cols[j] =
    (dtype, k -> column j's value for table k), called for the tables that have an entry in `ent`.  A table without one (not deferred) gets a
    null entry when `tolerate`, and (None, None) comes back when none has; without `tolerate` one missing entry gives
    (None, None).  `pad`: trailing members of `struct` left null."""
    miss = [e is None for e in ent]
    if not ts or (all(miss) if tolerate else any(miss)):
        return None, None
    arrs = [torch.tensor([0 if miss[k] else get(k) for k in range(len(ts))], dtype=dtype, device=ts[0].device) for dtype, get in cols]
    return struct(*([a.data_ptr() for a in arrs] + [None] * pad)), arrs


class _TableStep(object):
    """The host side of the six table optimizers, and what the model's train step duck-types on (`table_step`): `arm_l2`,
    `owns`, `l2_value`, `grad_sources`, `sync_lr`, `generation`, `note_replay`, `flush`, `take_backlog`.  A mixin in front of
    the stock class.  A class brings its clock layout and C calls (`_deferred_state`, `_catchup`, `_flush_launch`), what its
    kernel implements (`_plain`, `_state_of`, `_hyper`) and the class attributes below; `step` here is the one of TableSGD,
    TableAdagrad, TableRMSprop, TableFTRL and TableRowwiseAdagrad, TableAdam has its own."""
    table_step = True
    _KERNEL = None               # "sgd" / "adagrad" / "rmsprop" / "ftrl" ("sgdm" is TableSGD's second kernel, "rowwise" TableRowwiseAdagrad's: `_kind`)
    _ENV = "XDFM_OPT"            # the environment's <_ENV>_DEFERRED / <_ENV>_FLUSH_EVERY
    _PATHS = ("scan",)           # keys of `path_counts`
    _FLOOR = "OPT_DEFER_MIN_NUMEL"      # the module constant "auto" compares with (by name: read when the decision is taken)
    _OWN = {}                    # fields of the class itself that a pickle keeps -> their value for a pickle without them
    _PARKS_BACKLOG = True        # a dropped deferred state leaves its backlog cell to the next one (TableAdam loses it)
    _STATE_DICT_DROPS = True     # state_dict() drops the deferred state and bumps `generation` (TableAdam keeps both)

    def _table_init(self, deferred=None, flush_every=64):
        # Deferred (exact) update of the tables, include/xdfm.h "K7d" / "K7sd / K7gd": same bits as the dense sweep, but a
        # row is brought up to date when a batch gathers it, when a gradient arrives for it, and every `flush_every` steps
        # for all rows.  `deferred`: True / False / "auto" (None: <_ENV>_DEFERRED = 1 / 0 / auto, default auto): "auto"
        # defers when the gathers' tables hold at least `_FLOOR` parameters.  Applies, like the marks, inside the model's
        # own train step.
        env = os.environ.get(self._ENV + "_DEFERRED", "auto")
        self.deferred = (False if env == "0" else True if env == "1" else "auto") if deferred is None else \
            (deferred if deferred == "auto" else bool(deferred))
        self.flush_every = max(1, min(int(os.environ.get(self._ENV + "_FLUSH_EVERY", flush_every)), DEFER_CAP - 8))
        self._def = None            # clock, rates / constants, per-table `last` bytes, backlog (built by the first deferred step)
        self._since = 0             # steps since the last flush (host count of what the device clock holds)
        self._auto_numel = None
        self.path_counts = dict.fromkeys(self._PATHS, 0)      # deferred steps issued (or captured) by path: keyed by the batch's rows / by the mark bytes
        self._armed = None          # id(parameter) -> L2 strength, for the next step only
        self._desc = {}             # group index -> (key, ctypes array of xdfm_adam_tensor / xdfm_opt_tensor)
        self.l2_value = None        # [1] device tensor: value of the armed L2 term at the last step
        self.grad_sources = []      # objects with .arenas() -> [ops.GradArena]: gradients the kernel may read by their marks
        self._lr_dev = {}           # group index -> [host value, [1] float64 device tensor the kernel reads the rate from]
        self._replay_steps = None   # host step counters a captured step advances (its Python does not run on replay)
        self.generation = 0         # bumped whenever state tensors may have been replaced (part of the graph key)

    # The kernels take the learning rate from device memory, so a captured train step follows `param_groups[i]["lr"]`
    # edits without a new capture; the scalar is rewritten OUTSIDE any capture (GraphedStep calls this before a replay).
    def sync_lr(self):
        for gi, group in enumerate(self.param_groups):
            lr = group["lr"]
            if not isinstance(lr, float) or not group["params"]:
                continue
            hit = self._lr_dev.get(gi)
            dev = group["params"][0].device
            if hit is None or hit[1].device != dev:
                if dev.type != "cuda" or torch.cuda.is_current_stream_capturing():
                    continue
                hit = self._lr_dev[gi] = [None, torch.empty(1, dtype=torch.float64, device=dev)]
            if hit[0] != lr:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("xdfm %s: learning rate changed inside a HIP-graph capture" % type(self).__name__)
                hit[1].fill_(lr)
                hit[0] = lr

    def _invalidate(self):
        """State tensors may have been replaced: forget the cached descriptors and make every captured graph that baked
        their addresses stale (graphstep._signature hashes `generation`)."""
        self.flush()                 # no-op when the caller flushed before it replaced the state
        self._desc = {}
        self._lr_dev = {}
        self._replay_steps = None
        self.generation += 1
        self._auto_numel = None      # the "auto" decision follows the param groups
        self._drop_deferred()

    def load_state_dict(self, state_dict):
        self.flush()                 # rows that still owe replayed steps get them from the OLD accumulators, before those go
        out = super().load_state_dict(state_dict)
        self._invalidate()
        return out

    def add_param_group(self, param_group):
        if hasattr(self, "_desc"):              # the base constructor comes here before _table_init
            self.flush()
        out = super().add_param_group(param_group)
        if hasattr(self, "_desc"):
            self._invalidate()
        return out

    def state_dict(self):
        # flush, then drop the deferred state: what is handed out is current and shares nothing with the deferral.  A graph
        # captured with the catch-up and the clock baked in is stale from here on (`generation`); the next eager step of
        # the model builds the state again.
        self.flush()
        if self._STATE_DICT_DROPS and self.__dict__.get("_def") is not None:
            self._drop_deferred()
            self.generation += 1
        return super().state_dict()

    # ------------------------------------------------------------------ deferred update of the tables
    def _drop_deferred(self):
        d = self.__dict__.get("_def")
        if d is not None:
            for plan in d["plans"]:
                plan.catchup = None
            if self._PARKS_BACKLOG:
                self.__dict__["_backlog_kept"] = d["backlog"]      # the L2 value of replayed steps nobody has taken yet survives
        self._def = None
        self._since = 0

    def _deferred_state(self, dev):
        if self._def is None:
            i64 = dict(dtype=torch.int64, device=dev)
            kept = self.__dict__.pop("_backlog_kept", None)
            d = self._def = dict(clock=torch.zeros(2, dtype=torch.int32, device=dev),
                                 rates=torch.zeros(DEFER_CAP, dtype=torch.float32, device=dev),
                                 backlog=kept if kept is not None and kept.device == dev else torch.zeros(1, **i64),
                                 cell=torch.zeros(1, **i64), last={}, tensors={}, rows={}, plans=[], eps=None, kind=self._KERNEL)
            d["clk"] = _lib.OptClock(d["clock"].data_ptr(), d["rates"].data_ptr(), DEFER_CAP, d["backlog"].data_ptr(),
                                     d["cell"].data_ptr())
            for src in self.grad_sources:             # the gathers whose rows must be current before they are read
                if hasattr(src, "catchup"):
                    src.catchup = self._catchup
                    d["plans"].append(src)
            self.generation += 1                       # a step captured without the catch-up launch is stale
        return self._def

    def _last_bytes(self, p):
        d = self._def
        hit = d["last"].get(p.data_ptr())
        if hit is None:
            hit = d["last"][p.data_ptr()] = torch.zeros(p.numel() // 4 + 8, dtype=torch.uint8, device=p.device)
        return hit

    def _catchup(self, plan, X, emb_tables, lin_tables):
        """Called by the gather (ops.EmbedGather.forward) before it reads the rows of X."""
        d = self.__dict__.get("_def")
        if d is None or not d["tensors"]:
            return
        if self._since == 0 and not torch.cuda.is_current_stream_capturing():
            return
        key = (tuple(t.data_ptr() for t in emb_tables), tuple(t.data_ptr() for t in lin_tables))
        rows = d["rows"].get(key)
        if rows is None:
            # The pointer tables are built with torch.tensor(..., device=): a host-to-device copy from pageable memory, which
            # must not happen inside a capture.  It does not: GraphedStep captures after eager warm-up steps, `_def` is built
            # by an eager step (which makes every older graph stale), and the eager step after that one comes here with
            # `_since > 0` and fills this cache for the same tables.  Should a capture get here first all the same, the copy
            # fails the capture and the model falls back to eager steps (graphstep._capture).
            def table_of(ts):
                # a field whose table is not deferred (no L2 term, frozen) has a null entry: the kernel leaves it alone
                ent = [d["tensors"].get(t.data_ptr()) for t in ts]
                return _ptr_tables(_lib.OptRows, ts, ent, [
                    (torch.int64, lambda k: ts[k].data_ptr()),
                    (torch.int64, lambda k: ent[k][0].data_ptr() if ent[k][0] is not None else 0),
                    (torch.int64, lambda k: ent[k][1].data_ptr()), (torch.float32, lambda k: ent[k][2])], tolerate=True)
            e_struct, e_keep = table_of(list(emb_tables))
            l_struct, l_keep = table_of(list(lin_tables))
            if e_struct is None and l_struct is not None:      # only linear tables are deferred: an all-null embedding side
                dev = X.device
                nul = torch.zeros(len(emb_tables), dtype=torch.int64, device=dev)
                zl2 = torch.zeros(len(emb_tables), dtype=torch.float32, device=dev)
                e_struct, e_keep = _lib.OptRows(nul.data_ptr(), nul.data_ptr(), nul.data_ptr(), zl2.data_ptr()), (nul, zl2)
            rows = d["rows"][key] = (e_struct, l_struct, e_keep, l_keep)
        e_struct, l_struct = rows[0], rows[1]
        if e_struct is None:
            return                                      # tables this optimizer does not update by deferral
        cols, vocab, _, _ = plan.on(X.device)
        head = (X.data_ptr(), X.stride(0), X.shape[0], cols.data_ptr(), vocab.data_ptr(), plan.m, plan.D, ctypes.byref(e_struct),
                ctypes.byref(l_struct) if l_struct is not None else None, ctypes.byref(d["clk"]))
        stream = torch.cuda.current_stream(X.device).cuda_stream
        k = KINDS[d["kind"]]                            # the kernel of the steps the replays stand for, and its d["eps"]
        rc = getattr(_lib.load(), k.catchup)(*(k.lead + head + k.replay(d["eps"]) + (stream,)))
        _lib.check(rc, "opt_catchup_rows")

    @torch.no_grad()
    def flush(self):
        """Every deferred chunk up to date; afterwards parameters and accumulators are what the dense sweep would hold."""
        d = self.__dict__.get("_def")
        if d is None or self._since == 0:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("xdfm %s: flush inside a HIP-graph capture" % type(self).__name__)
        if d["tensors"]:
            self._flush_launch(d, torch.cuda.current_stream(d["clock"].device).cuda_stream)
        self._since = 0

    def _flush_launch(self, d, stream):
        """flush()'s descriptors and C call for the tables of d["tensors"] (there is at least one)."""
        ent = list(d["tensors"].items())
        arr = (_lib.OptTensor * len(ent))()
        last = (ctypes.c_void_p * len(ent))()
        for k, (ptr, (state, lb, l2, numel)) in enumerate(ent):
            arr[k].param, arr[k].numel, arr[k].l2 = ptr, numel, l2
            arr[k].state = state.data_ptr() if state is not None else None
            last[k] = lb.data_ptr()
        head = (ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(last, ctypes.c_void_p), len(ent), ctypes.byref(d["clk"]))
        k = KINDS[d["kind"]]
        rc = getattr(_lib.load(), k.flush)(*(k.lead + head + k.replay(d["eps"]) + (stream,)))
        _lib.check(rc, "opt_flush")

    def take_backlog(self):
        """L2 value of the replayed steps since the last call (a host float; syncs).  Over an epoch, the per-step L2 values
        plus this equal the dense path's sum."""
        d = self.__dict__.get("_def")
        cell = d["backlog"] if d is not None else self.__dict__.get("_backlog_kept")
        if cell is None:
            return 0.0
        v = float(cell.item()) / float(1 << 40)
        cell.zero_()
        return v

    def __getstate__(self):
        self.flush()                            # a pickled optimizer (torch.save(model)) goes with current rows
        state = dict(super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__)
        for k in ("_desc", "_lr_dev"):          # ctypes descriptors / device scalars: rebuilt on use
            state[k] = {}
        for k in ("_armed", "l2_value", "_replay_steps", "_def", "_auto_numel", "_backlog_kept"):
            state[k] = None
        state["_since"] = 0
        state["grad_sources"] = []
        state["generation"] = self.generation
        state["deferred"], state["flush_every"] = self.deferred, self.flush_every
        for k in self._OWN:
            state[k] = getattr(self, k)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        gen = self.__dict__.get("generation", 0)
        for k in ("_desc", "_lr_dev"):
            self.__dict__.setdefault(k, {})
        for k in ("_armed", "l2_value", "_replay_steps"):
            self.__dict__.setdefault(k, None)
        self.__dict__.setdefault("grad_sources", [])
        self.__dict__.setdefault("deferred", False)
        self.__dict__.setdefault("flush_every", 64)
        self.__dict__.setdefault("path_counts", dict.fromkeys(self._PATHS, 0))
        for k, v in self._OWN.items():
            self.__dict__.setdefault(k, v)
        self.__dict__["_def"] = None
        self.__dict__["_since"] = 0
        self.__dict__["_auto_numel"] = None
        self.generation = gen + 1

    def owns(self, tensors):
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        return all(id(t) in mine for t in tensors)

    def arm_l2(self, tensors, coeffs):
        """The next step() adds the gradient of sum_t coeffs[t] * sum(tensors[t]^2) itself and reports its value."""
        self._armed = {}
        for t, c in zip(tensors, coeffs):
            self._armed[id(t)] = self._armed.get(id(t), 0.0) + float(c)

    def note_replay(self):
        """Called before a captured step is replayed (its Python does not run): the host-side step counters (Adagrad)
        still count it; deferred update: periodic flush, step count."""
        if self._replay_steps:
            torch._foreach_add_(self._replay_steps, 1)
        if self.__dict__.get("_def") is not None:
            if self._since >= self.flush_every:
                self.flush()
            self._since += 1

    def _l2_by_hand(self, armed):
        """Fallback path: apply the armed term with ATen ops before torch's own step."""
        value = None
        for group in self.param_groups:
            for p in group["params"]:
                c = armed.get(id(p), 0.0)
                if c and p.grad is not None:
                    p.grad.add_(p.detach(), alpha=2.0 * c)
                    term = c * p.detach().square().sum()
                    value = term if value is None else value + term
        self.l2_value = None if value is None else value.reshape(1)

    # ------------------------------------------------------------------ what the step() bodies share
    def _gather_tables(self):
        """Addresses of the tables of the gathers that feed this optimizer (their rows are what a batch touches)."""
        ptrs = set()
        for src in self.grad_sources:
            lg = getattr(src, "last_gather", None)
            if lg is not None:
                ptrs.update(t.data_ptr() for t in lg[1])
                ptrs.update(t.data_ptr() for t in lg[2])
        return ptrs

    def _auto_defer(self, params, table_ptrs):
        """`deferred == "auto"`: whether the gathers' tables hold at least `_FLOOR` parameters (True for `deferred=True`)."""
        if self.deferred != "auto":
            return True
        if self._auto_numel is None:                # the tables' sizes do not change: decided once
            self._auto_numel = sum(p.numel() for p in params if p.data_ptr() in table_ptrs)
        return self._auto_numel >= globals()[self._FLOOR]

    def _l2_scratch(self, ws_elems, T, l2, dev):
        """(workspace of the per-block partials, [1] value) for a group's armed L2 term, (None, None) without one."""
        if l2 is None or not any(l2):
            return None, None
        from . import ops
        ws = torch.empty(ws_elems(T), dtype=torch.float32, device=dev)
        ops.finish_keep(ws)                     # inside a finish batch the partials are read when the batch runs
        return ws, torch.empty(1, dtype=torch.float32, device=dev)

    def _add_l2(self, val):
        if val is not None:
            if self.l2_value is not None:
                from . import ops
                ops.finish_batch_flush()        # a further group's value: both must be final before they are added
            self.l2_value = val if self.l2_value is None else self.l2_value + val

    def _plain(self, group):                    # hyper-parameters the kernel implements
        raise NotImplementedError

    def _state_of(self, group, p):              # (accumulator or None, host step counter or None[, a second state array])
        raise NotImplementedError

    def _hyper(self, group):                    # what the replays of a deferred step assume beside the rate: a change flushes
        return None

    def _kind(self, group):                     # the kernel a group's step runs (TableSGD has two)
        return self._KERNEL

    _DESC = _lib.OptTensor                      # the kernel's descriptor (TableFTRL: two state arrays, _lib.FtrlTensor)

    def _desc_type(self, kind):                 # ... by the group's kernel (TableRowwiseAdagrad has two)
        return self._DESC

    def _set_state(self, desc, st):             # st: what `_state_of` gave -> the state pointers written into `desc`
        desc.state = st[0].data_ptr() if st[0] is not None else None
        return (desc.state,)

    def _stock_step(self, closure):             # what the kernel does not implement: the stock class behind the mixin
        return super().step(closure)

    def _native(self):
        """True when every group can take the kernel: plain hyper-parameters, dense contiguous fp32 CUDA tensors."""
        if getattr(self, "grad_scale", None) is not None or getattr(self, "found_inf", None) is not None:
            return False
        for group in self.param_groups:
            # (.get: TableFTRL's groups have none of the stock classes' three switches)
            if not self._plain(group) or not isinstance(group["lr"], float) or group.get("maximize") or \
                    group.get("differentiable") or group.get("weight_decay", 0) != 0:
                return False
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and not g.is_sparse and
                        g.dtype == torch.float32 and g.is_contiguous() and g.device == p.device):
                    return False
        return True

    @torch.no_grad()
    def step(self, closure=None):
        armed, self._armed = self._armed, None
        self.l2_value = None
        if closure is not None or not self._native():
            self.flush()                               # the stock step updates every row: they must be current
            if armed:
                self._l2_by_hand(armed)
            return self._stock_step(closure)
        self.sync_lr()
        lib = _lib.load()
        from . import ops                              # per-kernel timing hook of bench.py
        from . import dist as xdist
        capturing = torch.cuda.is_current_stream_capturing()
        host_steps = []
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            kind = self._kind(group)
            grads = [p.grad for p in params]
            states = [self._state_of(group, p) for p in params]
            host_steps += [st[1] for st in states if st[1] is not None]
            T = len(params)
            l2 = tuple(armed.get(id(p), 0.0) for p in params) if armed else None
            key = (tuple(p.data_ptr() for p in params),
                   tuple(s.data_ptr() for st in states for s in (st[0],) + tuple(st[2:]) if s is not None), l2)
            hit = self._desc.get(gi)
            if hit is None or hit[0] != key:
                arr = (self._desc_type(kind) * T)()
                aligned = []                           # the tensor's state may be read by float4: a condition of the marks
                for k in range(T):
                    arr[k].param = params[k].data_ptr()
                    if kind == "rowwise":              # K7w: [rows, dim], one accumulator per row
                        arr[k].rows, arr[k].dim = params[k].shape
                    else:
                        arr[k].numel = params[k].numel()
                    aligned.append(all((q or 0) % 16 == 0 for q in self._set_state(arr[k], states[k])))
                    arr[k].l2 = l2[k] if l2 is not None else 0.0
                hit = self._desc[gi] = (key, arr, aligned)
            arr, state_aligned = hit[1], hit[2]
            arenas = [a for src in self.grad_sources for a in src.arenas() if a.pending]
            # Deferral: the tables of the gathers that feed this optimizer, in group 0, with an L2 term and marked gradients,
            # in a single process (a row-parallel run keeps the sweep).  With l2 == 0 the sweep's exact shortcut already
            # skips untouched chunks: nothing to defer.
            defer_ok = bool(self.deferred) and gi == 0 and l2 is not None and xdist.current() is None
            table_ptrs = self._gather_tables() if defer_ok else set()
            defer_ok = defer_ok and self._auto_defer(params, table_ptrs)
            deferred_now = []
            for k in range(T):
                gp = grads[k].data_ptr()
                arr[k].grad, arr[k].grad_marks = gp, None
                for a in arenas:                       # a view of a kept gradient buffer: read it by its marks
                    mp = a.marks_ptr(gp)
                    if mp is not None and params[k].data_ptr() % 16 == 0 and state_aligned[k]:
                        arr[k].grad_marks = mp
                        if defer_ok and l2[k] > 0.0 and params[k].data_ptr() in table_ptrs:
                            deferred_now.append(k)
                        a.consumed(gp)
                        break
            dev = params[0].device
            d = self.__dict__.get("_def")
            last_arr = None
            if gi != 0:
                pass                                   # the deferred tables live in group 0: a later group leaves their clock alone
            elif d is not None and not deferred_now:
                # tables that were deferred arrive without marks (a user-driven loop) or may no longer be deferred: bring
                # everything up to date and take this step densely.  Inside a capture with steps owed, flush() raises: the
                # capture fails and GraphedStep goes on eagerly (its warm-up steps come through here first, so a capture
                # normally finds `_since == 0` or marked gradients).
                self.flush()
            elif deferred_now:
                if d is None and not capturing:        # state is built by an eager step, never inside a capture
                    d = self._deferred_state(dev)
                if d is None:
                    deferred_now = []
                else:
                    want = {params[k].data_ptr(): (states[k][0], float(l2[k]), params[k].numel()) for k in deferred_now}
                    eps = self._hyper(group)
                    same = d["kind"] == kind and d["eps"] == eps and len(want) == len(d["tensors"]) and all(
                        ptr in d["tensors"] and d["tensors"][ptr][0] is w[0] and d["tensors"][ptr][2] == w[1]
                        for ptr, w in want.items())
                    if not same:
                        # the set of deferred tables, an L2 strength, eps, alpha, the momentum or the kernel changed: the replays
                        # assumed the old ones (the flush below still runs with them)
                        if capturing:                  # (the `last` bytes are allocated and zeroed by an eager step)
                            raise RuntimeError("xdfm %s: the deferred tables changed inside a HIP-graph capture" % type(self).__name__)
                        self.flush()
                        byptr = {params[k].data_ptr(): params[k] for k in deferred_now}
                        d["tensors"] = {ptr: (w[0], self._last_bytes(byptr[ptr]), w[1], w[2]) for ptr, w in want.items()}
                        d["rows"], d["eps"], d["kind"] = {}, eps, kind
                    if not capturing and self._since >= self.flush_every:
                        self.flush()
                    last_arr = (ctypes.c_void_p * T)()
                    for k in deferred_now:
                        last_arr[k] = d["tensors"][params[k].data_ptr()][1].data_ptr()
            nbytes = 0.0
            for k in range(T):
                per = KINDS[kind].per_param(arr[k])
                if arr[k].grad_marks:
                    skip = (arr[k].l2 == 0.0 and KINDS[kind].skip) or (last_arr is not None and last_arr[k])
                    nbytes += params[k].numel() * (0.0625 if skip else per + 0.0625)
                else:
                    nbytes += params[k].numel() * (per + 4.0)
            ws, val = self._l2_scratch(lib.xdfm_opt_step_ws_elems, T, l2, dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            lr_dev = self._lr_dev.get(gi)
            lr_ptr = lr_dev[1].data_ptr() if lr_dev is not None else None
            ws_ptr, val_ptr = (ws.data_ptr(), val.data_ptr()) if val is not None else (None, None)
            entry = KINDS[kind]
            tail = (float(group["lr"]), lr_ptr) + entry.hyper(group) + (ws_ptr, val_ptr, stream)
            if last_arr is not None:
                head = (ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(last_arr, ctypes.c_void_p), T, ctypes.byref(d["clk"]))
                launch = lambda: getattr(lib, entry.deferred)(*(head + tail))
                self.path_counts["scan"] += 1
                if not capturing:
                    self._since += 1
            else:
                launch = lambda: getattr(lib, entry.step)(ctypes.cast(arr, ctypes.c_void_p), T, *tail)
            _lib.check(ops._run("%s_step[bytes]" % kind, nbytes, launch), "%s_step" % kind)
            self._add_l2(val)
        if host_steps:
            if capturing:
                self._replay_steps = host_steps        # nothing runs during a capture: every replay counts (note_replay)
            else:
                torch._foreach_add_(host_steps, 1)
        return None



class TableAdam(_TableStep, torch.optim.Adam):
    """torch.optim.Adam whose step is K7 (`xdfm_adam_step_lr`), the tables' deferred form K7d (module docstring).  The host
    scaffold is `_TableStep`'s; here are the clock of K7d, its C calls and the step.  Where it differs from the other three:
    `state_dict()` flushes but keeps the deferred state and `generation`; a dropped deferred state takes its backlog cell
    with it (a known wart); the deferral needs neither an L2 term nor a single process."""
    _ENV = "XDFM_ADAM"
    _PATHS = ("rows", "scan")
    _FLOOR = "DEFER_MIN_NUMEL"
    _OWN = {"lazy_rows": False}
    _PARKS_BACKLOG = False
    _STATE_DICT_DROPS = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, lazy_rows=False, deferred=None, flush_every=64):
        super().__init__(params, lr=lr, betas=betas, eps=eps, fused=True, capturable=True)
        # K7d moves the sweep's 24 bytes per table parameter once per `flush_every` steps instead of every step.  Both ways
        # give the same bits; the deferred path costs ~0.27 ms per step whatever the tables' size (catch-up and update by
        # rows, the amortised flush), the sweep 5 us per million parameters: 1.50 against 1.55 ms per step at 44 M table
        # parameters, 4.1 against 2.13 ms at 575 M -- hence "auto" and DEFER_MIN_NUMEL.
        self._table_init(deferred, flush_every)
        # OPT-IN deviation from the reference: rows of the embedding tables that a batch does not touch
        # are not updated at all (no moment decay, no L2 pull) -- "lazy" Adam.  The reference's dense Adam updates every
        # row every step; with `lazy_rows` the step's cost follows the batch instead of the vocabulary.  Applies only to
        # gradients that arrive through the kept, marked gradient buffer (the model's own train step).
        self.lazy_rows = bool(lazy_rows)

    # ------------------------------------------------------------------ deferred update of the tables (K7d)
    def _deferred_state(self, dev, steps_done):
        if self._def is None:
            clock = torch.zeros(2, dtype=torch.int32, device=dev)
            clock[1] = int(steps_done)
            self._def = dict(clock=clock, consts=torch.zeros(4 * DEFER_CAP, dtype=torch.float32, device=dev),
                             backlog=torch.zeros(1, dtype=torch.int64, device=dev), last={}, l2={}, rows={}, plans=[],
                             tensors={})
            self._def["clk"] = _lib.AdamClock(clock.data_ptr(), self._def["consts"].data_ptr(), DEFER_CAP)
            for src in self.grad_sources:             # the gathers whose rows must be current before they are read
                if hasattr(src, "catchup"):
                    src.catchup = self._catchup
                    self._def["plans"].append(src)
            self.generation += 1                       # a step captured without the catch-up launch is stale
        return self._def

    @staticmethod
    def _row_columns(ent, param_of):
        """The first five columns of xdfm_adam_rows for `_ptr_tables` (param, exp_avg, exp_avg_sq, last, l2) from the entries
        of d["tensors"]: (exp_avg, exp_avg_sq, `last` bytes, l2, numel)."""
        return ([(torch.int64, param_of)] + [(torch.int64, lambda j, c=c: ent[j][c].data_ptr()) for c in range(3)] +
                [(torch.float32, lambda j: ent[j][3])])

    def _rows_for_apply(self, d, params, grads, arr, deferred_now):
        """(plan, X, emb rows, lin rows, indices of the tensors K7 proper still handles) when the step's update of the BIG
        deferred tables can be keyed by the batch of the one gather that feeds them -- a single process, one gather whose
        fields are exactly the deferred tables, at least one table of ROWS_MIN_NUMEL elements -- else None (every deferred
        table is updated by the scan of its mark bytes)."""
        from . import dist as xdist
        # Big tables only (ROWS_MIN_NUMEL): in a small table an id occurs hundreds of times per batch and every occurrence
        # contends for the claim of the same `last` word (all tables by rows: 0.36 ms per step at the Criteo-card
        # benchmark against 0.18 ms for the scan); small tables stay with the step's mark scan, where they cost nothing.
        if xdist.current() is not None or len(d["plans"]) != 1 or os.environ.get("XDFM_ADAM_ROWS", "1") == "0":
            return None
        plan = d["plans"][0]
        if plan.last_gather is None:
            return None
        X, emb_tables, lin_tables = plan.last_gather
        index = {params[k].data_ptr(): k for k in deferred_now}
        fields = list(emb_tables) + list(lin_tables)
        if len(fields) != len(index) or any(t.data_ptr() not in index for t in fields) or X.shape[0] <= 0:
            return None
        min_numel = int(os.environ.get("XDFM_ADAM_ROWS_MIN_NUMEL", ROWS_MIN_NUMEL))
        key = ("apply", min_numel, tuple(t.data_ptr() for t in fields), tuple(grads[index[t.data_ptr()]].data_ptr() for t in fields))
        hit = d["rows"].get(key)
        if hit is None:
            by_rows_k = set()

            def table_of(ts):
                ent = [d["tensors"][t.data_ptr()] for t in ts]
                ks = [index[t.data_ptr()] for t in ts]
                big = [t.numel() >= min_numel for t in ts]
                by_rows_k.update(k for k, b in zip(ks, big) if b)
                return _ptr_tables(_lib.AdamRows, ts, ent, self._row_columns(ent, lambda j: ts[j].data_ptr() if big[j] else 0) + [
                    (torch.int64, lambda j: grads[ks[j]].data_ptr()), (torch.int64, lambda j: arr[ks[j]].grad_marks)], tolerate=False)
            e_struct, e_keep = table_of(list(emb_tables))
            l_struct, l_keep = table_of(list(lin_tables))
            hit = d["rows"][key] = (e_struct, l_struct, e_keep, l_keep, frozenset(by_rows_k))
        if "cell" not in d:
            d["cell"] = torch.zeros(1, dtype=torch.int64, device=X.device)
        if not hit[4]:
            return None                                 # no table is big enough: everything by the scan
        rest = [k for k in range(len(params)) if k not in hit[4]]      # K7 proper: dense tensors + the small deferred tables
        if not rest:
            return None
        return plan, X, hit[0], hit[1], rest

    def _catchup(self, plan, X, emb_tables, lin_tables):
        """Called by the gather (ops.EmbedGather.forward) before it reads the rows of X."""
        d = self._def
        if d is None:
            return
        if self._since == 0 and not torch.cuda.is_current_stream_capturing():
            return
        key = (tuple(t.data_ptr() for t in emb_tables), tuple(t.data_ptr() for t in lin_tables))
        rows = d["rows"].get(key)
        if rows is None:
            def table_of(ts):                           # one table that is not deferred: no struct, no catch-up
                ent = [d["tensors"].get(t.data_ptr()) for t in ts]
                return _ptr_tables(_lib.AdamRows, ts, ent, self._row_columns(ent, lambda j: ts[j].data_ptr()), tolerate=False, pad=2)
            e_struct, e_keep = table_of(emb_tables)
            l_struct, l_keep = table_of(lin_tables)
            rows = d["rows"][key] = (e_struct, l_struct, e_keep, l_keep)
        e_struct, l_struct = rows[0], rows[1]
        if e_struct is None or (lin_tables and l_struct is None):
            return                                      # tables this optimizer does not update by deferral
        group = self.param_groups[0]
        beta1, beta2 = group["betas"]
        cols, vocab, _, _ = plan.on(X.device)
        lib = _lib.load()
        _lib.check(lib.xdfm_adam_catchup_rows(
            X.data_ptr(), X.stride(0), X.shape[0], cols.data_ptr(), vocab.data_ptr(), plan.m, plan.D, ctypes.byref(e_struct),
            ctypes.byref(l_struct) if l_struct is not None else None, ctypes.byref(d["clk"]), float(beta1), float(beta2),
            float(group["eps"]), d["backlog"].data_ptr(), torch.cuda.current_stream(X.device).cuda_stream),
            "adam_catchup_rows")

    def _flush_launch(self, d, stream):
        ent = list(d["tensors"].items())
        arr = (_lib.AdamTensor * len(ent))()
        for k, (ptr, (m, v, last, l2, numel)) in enumerate(ent):
            arr[k].param, arr[k].exp_avg, arr[k].exp_avg_sq, arr[k].last = ptr, m.data_ptr(), v.data_ptr(), last.data_ptr()
            arr[k].numel, arr[k].l2, arr[k].flags = numel, l2, 2
        group = self.param_groups[0]
        beta1, beta2 = group["betas"]
        _lib.check(_lib.load().xdfm_adam_flush(ctypes.cast(arr, ctypes.c_void_p), len(ent), ctypes.byref(d["clk"]), float(beta1),
                                               float(beta2), float(group["eps"]), d["backlog"].data_ptr(), stream), "adam_flush")

    def _plain(self, group):
        return (not group["amsgrad"] and group["weight_decay"] == 0 and not group["maximize"] and
                not group["differentiable"] and not group.get("decoupled_weight_decay", False) and
                isinstance(group["lr"], float) and all(isinstance(b, float) for b in group["betas"]) and
                getattr(self, "grad_scale", None) is None and getattr(self, "found_inf", None) is None)

    @torch.no_grad()
    def step(self, closure=None):
        armed, self._armed = self._armed, None
        self.l2_value = None
        if closure is not None or not all(self._plain(g) for g in self.param_groups):
            if armed:
                self._l2_by_hand(armed)
            return torch.optim.Adam.step(self, closure)      # (not super(): the mixin's step is the other three's)
        self._cuda_graph_capture_health_check()
        self.sync_lr()
        lib = _lib.load()
        for gi, group in enumerate(self.param_groups):
            params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps = [], [], [], [], [], []
            has_complex = self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps)
            if not params:
                continue
            ok = not has_complex and all(
                p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous() and
                g.is_contiguous() and g.device == p.device for p, g in zip(params, grads))
            if not ok:
                raise RuntimeError("xdfm TableAdam: parameters and gradients must be contiguous fp32 CUDA tensors")
            beta1, beta2 = group["betas"]
            T = len(params)
            l2 = tuple(armed.get(id(p), 0.0) for p in params) if armed else None
            key = (tuple(p.data_ptr() for p in params), tuple(m.data_ptr() for m in exp_avgs), l2)
            hit = self._desc.get(gi)
            if hit is None or hit[0] != key:
                arr = (_lib.AdamTensor * T)()
                for k in range(T):
                    arr[k].param, arr[k].exp_avg, arr[k].exp_avg_sq = params[k].data_ptr(), exp_avgs[k].data_ptr(), exp_avg_sqs[k].data_ptr()
                    arr[k].step, arr[k].numel = steps[k].data_ptr(), params[k].numel()
                    arr[k].l2 = l2[k] if l2 is not None else 0.0
                hit = self._desc[gi] = (key, arr)
            arr = hit[1]
            arenas = [a for src in self.grad_sources for a in src.arenas() if a.pending]
            capturing = torch.cuda.is_current_stream_capturing()
            # row-parallel runs included: a rank's own rows are brought up to date before its gather, the rows the other
            # ranks touched arrive with their marks and are replayed inside the step -- every replica ends with the same bits
            defer_ok = bool(self.deferred) and not self.lazy_rows and gi == 0
            table_ptrs = self._gather_tables() if defer_ok else set()
            defer_ok = defer_ok and self._auto_defer(params, table_ptrs)
            deferred_now = []
            for k in range(T):
                gp = grads[k].data_ptr()
                arr[k].grad, arr[k].grad_marks, arr[k].flags, arr[k].last = gp, None, 0, None
                for a in arenas:                       # a view of a kept gradient buffer: read it by its marks
                    mp = a.marks_ptr(gp)
                    if mp is not None and params[k].data_ptr() % 16 == 0:
                        arr[k].grad_marks = mp
                        table = params[k].dim() == 2 and params[k].shape[0] > 1
                        arr[k].flags = 1 if (self.lazy_rows and table) else 0
                        if defer_ok and params[k].data_ptr() in table_ptrs:
                            deferred_now.append(k)
                        a.consumed(gp)
                        break
            dev = params[0].device
            d = self._def
            if gi != 0:
                # the deferred tables live in group 0 (`defer_ok`); a later group has nothing to do with their clock: it
                # must neither flush them nor tick `clock[1]` a second time for the same step
                pass
            elif d is not None and len(deferred_now) != len(d["tensors"]):
                # tables that were deferred arrive without marks (a user-driven loop, a row-parallel run): bring
                # everything up to date and take this step densely; the clock only notes that a step passed
                self.flush()
                deferred_now = []
                d["clock"][1:2].add_(1)
            elif deferred_now:
                if d is None:
                    if capturing:
                        deferred_now = []              # state is built by an eager step, never inside a capture
                    else:
                        d = self._deferred_state(dev, int(round(float(steps[deferred_now[0]].item()))))
                if d is not None:
                    if not capturing and self._since >= self.flush_every:
                        self.flush()
                    for k in deferred_now:
                        ptr = params[k].data_ptr()
                        ent = d["tensors"].get(ptr)
                        lk = float(l2[k]) if l2 is not None else 0.0
                        if ent is None or ent[3] != lk:
                            if ent is not None:
                                self.flush()           # the L2 strength of a table changed: the replays assumed the old one
                            ent = d["tensors"][ptr] = (exp_avgs[k], exp_avg_sqs[k], self._last_bytes(params[k]), lk, params[k].numel())
                            d["rows"] = {}
                        arr[k].flags, arr[k].last = 2, ent[2].data_ptr()
            torch._foreach_add_(steps, 1)
            ws, val = self._l2_scratch(lib.xdfm_adam_step_ws_elems, T, l2, dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            lr_dev = self._lr_dev.get(gi)
            from . import ops                          # per-kernel timing hook of bench.py (HIP events on the launch stream)
            nbytes = sum(params[k].numel() * (0.0625 if arr[k].flags == 2 else (24.25 if arr[k].grad_marks else 28.0)) for k in range(T))
            if deferred_now and d is not None:
                by_rows = self._rows_for_apply(d, params, grads, arr, deferred_now)
                self.path_counts["rows" if by_rows is not None else "scan"] += 1
                if by_rows is None:
                    # the mark bytes say which chunks have a gradient (row-parallel runs: rows of every rank)
                    _lib.check(ops._run("adam_step[bytes]", nbytes, lambda: lib.xdfm_adam_step_deferred(
                        ctypes.cast(arr, ctypes.c_void_p), T, ctypes.byref(d["clk"]), float(group["lr"]),
                        lr_dev[1].data_ptr() if lr_dev is not None else None, float(beta1), float(beta2), float(group["eps"]),
                        ws.data_ptr() if ws is not None else None, val.data_ptr() if val is not None else None, stream)),
                        "adam_step_deferred")
                else:
                    # single process: the chunks with a gradient are the rows of the batch -- no scan of the mark bytes
                    plan, X, e_struct, l_struct, rest = by_rows
                    arr2 = (_lib.AdamTensor * max(len(rest), 1))()
                    for j, k in enumerate(rest):
                        ctypes.memmove(ctypes.byref(arr2[j]), ctypes.byref(arr[k]), ctypes.sizeof(_lib.AdamTensor))
                    cols, vocab, _, _ = plan.on(X.device)

                    def launch():
                        # the step over `rest` and the rows update: one launch behind the tick (option "colaunch" bit 0)
                        return lib.xdfm_colaunch_adam_step(
                            ctypes.cast(arr2, ctypes.c_void_p), len(rest), ctypes.byref(d["clk"]), float(group["lr"]),
                            lr_dev[1].data_ptr() if lr_dev is not None else None, float(beta1), float(beta2), float(group["eps"]),
                            ws.data_ptr() if ws is not None else None, val.data_ptr() if val is not None else None,
                            X.data_ptr(), X.stride(0), X.shape[0], cols.data_ptr(), vocab.data_ptr(), plan.m, plan.D,
                            ctypes.byref(e_struct), ctypes.byref(l_struct) if l_struct is not None else None,
                            d["cell"].data_ptr(), stream)
                    _lib.check(ops._run("adam_step[bytes]", nbytes, launch), "adam_step_deferred (rows)")
                if not capturing:
                    self._since += 1
            else:
                _lib.check(ops._run("adam_step[bytes]", nbytes, lambda: lib.xdfm_adam_step_lr(ctypes.cast(arr, ctypes.c_void_p), T, float(group["lr"]),
                                             lr_dev[1].data_ptr() if lr_dev is not None else None, float(beta1),
                                             float(beta2), float(group["eps"]), ws.data_ptr() if ws is not None else None,
                                             val.data_ptr() if val is not None else None, stream)), "adam_step")
            self._add_l2(val)
        return None



class TableSGD(_TableStep, torch.optim.SGD):
    """torch.optim.SGD whose step is K7s (`xdfm_sgd_step`) for momentum 0 (the reference's `compile("sgd")`, lr 0.01) and K7m
    (`xdfm_sgdm_step`) for 0 < momentum < 1 with dampening 0, plain or Nesterov; tables with an L2 term may take the deferred
    forms (K7sd / K7md).  With momentum the state is torch's: `momentum_buffer` per parameter, created by the first eager step,
    never inside a capture.  Dampening, a momentum outside (0, 1), weight decay, maximize, tensor learning rates, sparse /
    non-fp32 / non-CUDA tensors and closures -- and every momentum with XDFM_SGD_MOMENTUM_NATIVE=0 -- fall back to
    torch.optim.SGD.step with the armed L2 term applied by hand."""
    _KERNEL = "sgd"              # momentum 0; "sgdm" otherwise (`_kind`)

    def __init__(self, params, lr=0.01, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 deferred=None, flush_every=64):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov, maximize=maximize)
        self._table_init(deferred, flush_every)

    def _plain(self, group):
        mu = group["momentum"]
        if mu == 0:
            return group["dampening"] == 0 and not group["nesterov"]
        # (torch itself allows nesterov only with a momentum and dampening 0)
        return SGD_MOMENTUM_NATIVE and isinstance(mu, float) and 0.0 < mu < 1.0 and group["dampening"] == 0

    def _kind(self, group):
        return "sgd" if group["momentum"] == 0 else "sgdm"

    def _state_of(self, group, p):
        if group["momentum"] == 0:
            return None, None
        st = self.state[p]
        buf = st.get("momentum_buffer")         # None: absent (a torch.optim.SGD checkpoint saved before any step)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("xdfm TableSGD: the state is created by an eager step, not inside a HIP-graph capture")
            # torch makes the buffer at the first step as clone(g'); zeros give the same first value, mu * 0 + g' -- it differs
            # only in the sign of a zero (g' == -0 gives +0 here)
            buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()):
            raise RuntimeError("xdfm TableSGD: the momentum buffer of a CUDA parameter must be a contiguous fp32 CUDA tensor")
        return buf, None

    def _hyper(self, group):
        return None if group["momentum"] == 0 else (float(group["momentum"]), bool(group["nesterov"]))


class TableAdagrad(_TableStep, torch.optim.Adagrad):
    """torch.optim.Adagrad whose step is K7g (`xdfm_adagrad_step`) for lr_decay 0 (the reference's `compile("adagrad")`:
    lr 0.01, eps 1e-10).  State is torch's: `sum` per parameter and a host-resident `step` counter, which the update does
    not read but which still counts every step, replayed ones included (`note_replay`).  A non-zero
    `initial_accumulator_value` is only an initial state.  lr_decay, weight decay, maximize, tensor learning rates,
    sparse / non-fp32 / non-CUDA tensors and closures fall back to torch.optim.Adagrad.step."""
    _KERNEL = "adagrad"

    def __init__(self, params, lr=0.01, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10, *,
                 maximize=False, deferred=None, flush_every=64):
        super().__init__(params, lr=lr, lr_decay=lr_decay, weight_decay=weight_decay,
                         initial_accumulator_value=initial_accumulator_value, eps=eps, maximize=maximize)
        self._table_init(deferred, flush_every)

    def _plain(self, group):
        return group["lr_decay"] == 0 and group["eps"] > 0 and not group.get("fused")

    def _state_of(self, group, p):
        st = self.state[p]
        acc = st["sum"]
        if not (acc.is_cuda and acc.dtype == torch.float32 and acc.is_contiguous()):
            raise RuntimeError("xdfm TableAdagrad: the accumulator of a CUDA parameter must be a contiguous fp32 CUDA tensor")
        return acc, st["step"]

    def _hyper(self, group):
        return float(group["eps"])


class TableRMSprop(_TableStep, torch.optim.RMSprop):
    """torch.optim.RMSprop whose step is K7r (`xdfm_rmsprop_step`) for momentum 0, not centered (the reference's
    `compile("rmsprop")`: lr 0.01, alpha 0.99, eps 1e-8); tables with an L2 term may take its deferred form (K7rd).  State is
    torch's: `square_avg` per parameter and a host-resident `step` counter, which the update does not read but which counts
    every step, replayed ones included (`note_replay`); it is created by the first eager step, as the stock class creates
    it, never inside a capture.  Momentum, centered, weight decay, maximize, capturable, foreach, differentiable, tensor
    learning rates, eps == 0, alpha == 1, sparse / non-fp32 / non-CUDA tensors and closures fall back to
    torch.optim.RMSprop.step with the armed L2 term applied by hand."""
    _KERNEL = "rmsprop"

    def __init__(self, params, lr=0.01, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False, *, deferred=None, flush_every=64):
        super().__init__(params, lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=centered,
                         capturable=capturable, foreach=foreach, maximize=maximize, differentiable=differentiable)
        self._table_init(deferred, flush_every)

    def _plain(self, group):
        return (group["momentum"] == 0 and not group["centered"] and not group["capturable"] and group["foreach"] is None and
                isinstance(group["alpha"], float) and 0.0 <= group["alpha"] < 1.0 and group["eps"] > 0)

    def _state_of(self, group, p):
        st = self.state[p]
        if len(st) == 0:                        # torch.optim.RMSprop._init_group's layout for these hyper-parameters
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("xdfm TableRMSprop: the state is created by an eager step, not inside a HIP-graph capture")
            st["step"] = torch.zeros((), dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
            st["square_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        acc = st["square_avg"]
        if not (acc.is_cuda and acc.dtype == torch.float32 and acc.is_contiguous()):
            raise RuntimeError("xdfm TableRMSprop: the accumulator of a CUDA parameter must be a contiguous fp32 CUDA tensor")
        return acc, st["step"]

    def _hyper(self, group):
        return (float(group["alpha"]), float(group["eps"]))


class TableFTRL(_TableStep, torch.optim.Optimizer):
    """Per-coordinate FTRL-Proximal (McMahan et al., "Ad click prediction: a view from the trenches", 2013; lr_power -0.5)
    whose step is K7f (`xdfm_ftrl_step`).  torch has no such class: this one stands on torch.optim.Optimizer, and what the
    kernel does not take -- CPU parameters, closures, non-fp32 / non-contiguous / sparse tensors, tensor learning rates --
    runs the same formulas in torch ops (`_stock_step`), with the armed L2 term applied by hand.  Per element, with the
    model's armed L2 strength l2m for the tensor:

        g' = g + 2 l2m p;   g' == 0: the element is not touched
        n' = n + g'^2;   sigma = g'^2 / (lr (sqrt(n') + sqrt(n)));   z' = z + g' - sigma p
        p' = 0 where |z'| <= l1, else (sign(z') l1 - z') / ((beta + sqrt(n')) / lr + l2)

    `l1` clips weights to exactly 0.0.  `l2` is the paper's lambda_2 and enters the denominator as it is: TensorFlow's
    `l2_regularization_strength` is HALF of it (tf.keras.optimizers.Ftrl(l2_regularization_strength=x) is l2 = 2 x here).  It
    is proximal, not a gradient term: a row without a gradient does not move, so with the model's own L2 off
    (l2_reg_embedding = l2_reg_linear = 0) the step reads the gradient marks and the batch's rows only.  sigma is the paper's
    (sqrt(n') - sqrt(n)) / lr as a quotient, without the cancellation.  State per parameter: `z` and `n`, fp32 tensors of the
    parameter's shape, `n` filled with `initial_accumulator_value`; created by the first eager step, never inside a capture.
    There is no deferred form (`deferred` is False; `flush` and `take_backlog` are no-ops), no lr_power other than -0.5 and no
    l2_shrinkage."""
    _KERNEL = "ftrl"
    _DESC = _lib.FtrlTensor

    def __init__(self, params, lr=0.05, l1=0.0, l2=0.0, beta=1.0, initial_accumulator_value=0.1):
        if not isinstance(lr, torch.Tensor) and not lr > 0.0:
            raise ValueError("xdfm TableFTRL: lr %r is not above 0 (the step divides by it)" % (lr,))
        for name, v in (("l1", l1), ("l2", l2), ("beta", beta), ("initial_accumulator_value", initial_accumulator_value)):
            if not v >= 0.0:
                raise ValueError("xdfm TableFTRL: %s %r is negative" % (name, v))
        super().__init__(params, dict(lr=lr, l1=l1, l2=l2, beta=beta, initial_accumulator_value=initial_accumulator_value))
        self._table_init(deferred=False)

    @staticmethod
    def _check_lr(lr):
        if not (lr > 0.0 if isinstance(lr, float) else bool((torch.as_tensor(lr) > 0).all())):
            raise ValueError("xdfm TableFTRL: lr %r is not above 0 (the step divides by it)" % (lr,))

    def sync_lr(self):
        for group in self.param_groups:         # a rate <= 0 never reaches the device scalar: the kernel divides by it
            self._check_lr(group["lr"])
        super().sync_lr()

    def _plain(self, group):
        return all(isinstance(group[k], (int, float)) and group[k] >= 0 for k in ("l1", "l2", "beta"))

    def _hyper(self, group):
        return (float(group["l1"]), float(group["l2"]), float(group["beta"]))

    def _zn(self, group, p):
        st = self.state[p]
        if "z" not in st or "n" not in st:
            if p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("xdfm TableFTRL: the state is created by an eager step, not inside a HIP-graph capture")
            like = dict(dtype=torch.float32, memory_format=torch.contiguous_format)
            st["z"] = torch.zeros_like(p, **like)
            st["n"] = torch.full_like(p, float(group["initial_accumulator_value"]), **like)
        return st["z"], st["n"]

    def _state_of(self, group, p):
        z, n = self._zn(group, p)
        if not all(s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() for s in (z, n)):
            raise RuntimeError("xdfm TableFTRL: z and n of a CUDA parameter must be contiguous fp32 CUDA tensors")
        return z, None, n

    def _set_state(self, desc, st):
        desc.z, desc.n = st[0].data_ptr(), st[2].data_ptr()
        return desc.z, desc.n

    @torch.no_grad()
    def _stock_step(self, closure):
        """The formulas of the class docstring in torch ops, the zero-gradient rule included (fp32; float64 for a float64
        parameter).  The armed L2 term is in the gradients already (`_l2_by_hand`)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, l1, l2, beta = group["lr"], group["l1"], group["l2"], group["beta"]
            self._check_lr(lr)
            for p in group["params"]:
                if p.grad is None:
                    continue
                z, n = self._zn(group, p)
                ct = torch.float64 if p.dtype == torch.float64 else torch.float32
                g = (p.grad.to_dense() if p.grad.is_sparse else p.grad).to(ct)
                w, z0, n0 = p.to(ct), z.to(ct), n.to(ct)
                live = g != 0
                n1 = torch.addcmul(n0, g, g)
                r1 = torch.where(n1 > 0, n1.sqrt(), g.abs())         # n' == 0: n == 0 and g'^2 underflowed; the exact root is |g'|
                ds = lr * (r1 + n0.sqrt())
                sigma = torch.where(ds > 0, (g * g) / ds, torch.zeros_like(ds))
                z1 = torch.addcmul(z0 + g, sigma, w, value=-1.0)
                w1 = torch.where(z1.abs() <= l1, torch.zeros_like(z1), (torch.sign(z1) * l1 - z1) / ((beta + r1) / lr + l2))
                p.copy_(torch.where(live, w1, w))
                z.copy_(torch.where(live, z1, z0))
                n.copy_(torch.where(live, n1, n0))
        return loss


class TableRowwiseAdagrad(_TableStep, torch.optim.Optimizer):
    """Row-wise Adagrad -- the rule large CTR embedding tables are usually trained with (the DLRM / TorchRec default, FBGEMM's
    "exact row-wise Adagrad") -- whose step is K7w (`xdfm_rowwise_adagrad_step`) for the param groups with `rowwise=True` and K7g
    (`xdfm_adagrad_step`, plain Adagrad) for the others.  A row-wise group takes 2-D parameters only and keeps ONE accumulator
    per row, the running sum of the row's mean squared gradient; with the model's armed L2 strength l2m for the tensor:

        g' = g + 2 l2m p;   s' = s + mean_d(g'_d^2);   p' = p - lr g' / (sqrt(s') + eps)

    (the mean is taken in float64 and rounded to fp32; a row whose g' is all zeros keeps the bits of s and p).  State per
    parameter: `sum`, fp32, of shape [rows] for a row-wise parameter -- 1 / D of Adagrad's state -- and of the parameter's shape
    otherwise, filled with `initial_accumulator_value`; created by the first eager step, never inside a capture.
    `for_model(model)` builds the two groups: the `nn.Embedding` weights of `model.embedding_dict` and
    `model.linear_model.embedding_dict` are row-wise, everything else is element-wise.  With an L2 term on the tables every row is
    a real update in every step (the sweep moves 8 + 8 / D bytes per parameter, K7g 16); with `l2_reg_embedding = l2_reg_linear =
    0` -- the recommended configuration -- a row without a gradient does not move, exactly, and the step reads the gradient marks
    and the batch's rows only.  What the kernels do not take -- CPU parameters, closures, non-fp32 / non-contiguous / sparse
    tensors, tensor learning rates -- runs the same formulas in torch ops (`_stock_step`), with the armed L2 term applied by hand.
    There is no deferred form (`deferred` is False; `flush` and `take_backlog` are no-ops), no lr_decay, no weight decay, none
    of FBGEMM's weighted / counter variants.  Row-parallel runs need no code of their own but are untested on more than one
    process."""
    _KERNEL = "adagrad"          # the element-wise groups; "rowwise" for the others (`_kind`)

    def __init__(self, params, lr=0.01, eps=1e-10, initial_accumulator_value=0.0):
        if not isinstance(lr, torch.Tensor) and not lr >= 0.0:
            raise ValueError("xdfm TableRowwiseAdagrad: lr %r is negative" % (lr,))
        if not eps > 0.0:
            raise ValueError("xdfm TableRowwiseAdagrad: eps %r is not above 0" % (eps,))
        if not initial_accumulator_value >= 0.0:
            raise ValueError("xdfm TableRowwiseAdagrad: initial_accumulator_value %r is negative" % (initial_accumulator_value,))
        super().__init__(params, dict(lr=lr, eps=eps, initial_accumulator_value=initial_accumulator_value, rowwise=False))
        self._table_init(deferred=False)

    @classmethod
    def for_model(cls, model, **kw):
        """The optimizer over `model.parameters()` in two groups: row-wise for the embedding tables (VarLenSparseFeat tables
        included) and the 1-wide linear tables, element-wise for everything else.  An empty group is left out."""
        tables = []
        for holder in (model, getattr(model, "linear_model", None)):
            ed = getattr(holder, "embedding_dict", None)
            if ed is not None:
                tables += [m.weight for m in ed.values() if isinstance(m, torch.nn.Embedding)]
        row_ids = {id(p) for p in tables}
        rest = [p for p in model.parameters() if id(p) not in row_ids]
        rows = [p for p in model.parameters() if id(p) in row_ids]
        groups = [dict(params=ps, rowwise=rw) for ps, rw in ((rows, True), (rest, False)) if ps]
        return cls(groups, **kw)

    def add_param_group(self, param_group):
        if param_group.get("rowwise", False):
            ps = param_group["params"]
            ps = param_group["params"] = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            for p in ps:
                if p.dim() != 2:
                    raise ValueError("xdfm TableRowwiseAdagrad: a row-wise group takes 2-D parameters only (got shape %s)"
                                     % (tuple(p.shape),))
        return super().add_param_group(param_group)

    def _plain(self, group):
        return isinstance(group["eps"], float) and group["eps"] > 0

    def _kind(self, group):
        return "rowwise" if group.get("rowwise") else "adagrad"

    def _desc_type(self, kind):
        return _lib.RowwiseTensor if kind == "rowwise" else _lib.OptTensor

    def _sum(self, group, p):
        st = self.state[p]
        if "sum" not in st:
            if p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("xdfm TableRowwiseAdagrad: the state is created by an eager step, not inside a HIP-graph capture")
            shape = (p.shape[0],) if group.get("rowwise") else tuple(p.shape)
            st["sum"] = torch.full(shape, float(group["initial_accumulator_value"]), dtype=torch.float32, device=p.device)
        return st["sum"]

    def _state_of(self, group, p):
        acc = self._sum(group, p)
        want = (p.shape[0],) if group.get("rowwise") else tuple(p.shape)
        if not (acc.is_cuda and acc.dtype == torch.float32 and acc.is_contiguous() and tuple(acc.shape) == want):
            raise RuntimeError("xdfm TableRowwiseAdagrad: the accumulator of a CUDA parameter must be a contiguous fp32 CUDA tensor "
                               "of shape %s" % (want,))
        return acc, None

    def _set_state(self, desc, st):
        desc.state = st[0].data_ptr()
        # K7w reads the row's accumulator as one float: no 16-byte condition on it for the marks
        return () if isinstance(desc, _lib.RowwiseTensor) else (desc.state,)

    def _hyper(self, group):
        return float(group["eps"])

    @torch.no_grad()
    def _stock_step(self, closure):
        """The formulas of the class docstring in torch ops (fp32; the row sum in float64; float64 throughout for a float64
        parameter).  The armed L2 term is in the gradients already (`_l2_by_hand`)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, eps = group["lr"], group["eps"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                acc = self._sum(group, p)
                ct = torch.float64 if p.dtype == torch.float64 else torch.float32
                g = (p.grad.to_dense() if p.grad.is_sparse else p.grad).to(ct)
                w, s0 = p.to(ct), acc.to(ct)
                if group.get("rowwise"):
                    ms = g.double().square().sum(dim=1).div(g.shape[1]).to(ct)
                    s1 = torch.where(ms > 0, s0 + ms, s0)
                    den = (s1.sqrt() + eps).unsqueeze(1)
                else:
                    s1 = s0 + g * g
                    den = s1.sqrt() + eps
                w1 = torch.where(g != 0, w - lr * (g / den), w)
                p.copy_(w1)
                acc.copy_(s1)
        return loss
