"""xDeepFM model family on the MI355X kernels, behind the reference's Keras-like API.

Public surface (names, positional order, defaults, state_dict keys) follows
deepctr/models/basemodel.py:95-527, deepctr/models/xdeepfm.py:17-107 and
deepctr/models/xdeepfm_attn.py:25-301 so that the xdftrain*.py flows run unchanged:
`Model(linear_cols, dnn_cols, ...)`, `compile`, `fit`, `evaluate`, `predict`, `state_dict`.

What differs underneath: `forward` is one fused gather launch (embeddings in FM layout, DNN input
and linear logit together), the CIN stack on MFMA kernels, and a handful of tiny torch GEMMs; with
torch.distributed initialised (one process per GPU, RCCL) `fit` shards every global batch row-wise
over the ranks (xdfm_amd/dist.py).
"""
import contextlib
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dist as xdist
from . import metrics as M
from . import ops
from .callbacks import CallbackList, History
from .inputs import (DenseFeat, SparseFeat, VarLenSparseFeat, build_input_features, create_embedding_matrix,
                     split_columns)
from .layers import CIN, DNN, CINAttention, CINAttentionV2, PredictionLayer

try:
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    tqdm = None


def _slice(arrays, start=None, stop=None):
    """x[start:stop] for one array or each array of a list (deepctr/layers/utils.py:19-70 as fit uses it)."""
    if isinstance(arrays, (list, tuple)):
        return [None if a is None else a[start:stop] for a in arrays]
    return arrays[start:stop]


def epoch_order(n, shuffle):
    """Row order of one epoch, drawn exactly as `DataLoader(TensorDataset, shuffle=shuffle)` draws it
    (basemodel.py:213-214, :241): creating the iterator takes one int64 from the default generator (its
    base seed), then RandomSampler takes one more as the seed of a fresh generator for randperm.  The
    same primitives in the same order give the same batches as the reference for a given torch seed --
    without DataLoader's per-sample indexing and 4096-way collate (tens of ms per batch)."""
    torch.empty((), dtype=torch.int64).random_()
    if not shuffle:
        return None
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    gen = torch.Generator()
    gen.manual_seed(seed)
    return torch.randperm(n, generator=gen)


RESIDENT_LIMIT_BYTES = 64 << 30     # keep the packed fp32 input matrix on the device up to this size


def _check_varlen(cols):
    """Limits of the pooled variable-length fields (K1v): refused here, on the host, before anything is built."""
    sparse, _, varlen = split_columns(cols)
    if not varlen:
        return
    for fc in varlen:
        if not isinstance(fc.maxlen, (int, np.integer)) or not 1 <= fc.maxlen <= 255:
            raise ValueError("VarLenSparseFeat %r: maxlen must be an integer in 1..255, got %r" % (fc.name, fc.maxlen))
        if fc.combiner not in ops.POOL_CODES:
            raise ValueError("VarLenSparseFeat %r: combiner must be one of sum, mean, max, got %r" % (fc.name, fc.combiner))
    dims = {fc.embedding_dim for fc in sparse + varlen}
    if len(dims) > 1:
        raise ValueError("embedding_dim of SparseFeat and VarlenSparseFeat must be same in this model!")
    owner = {}
    for fc in sparse + varlen:
        # the reference counts CIN fields by tables (len(embedding_dict)) and breaks when two columns share one
        if owner.setdefault(fc.embedding_name, fc.name) != fc.name:
            raise ValueError("VarLenSparseFeat: columns %r and %r share embedding_name %r; every column needs a table of its own"
                             % (owner[fc.embedding_name], fc.name, fc.embedding_name))


def _varlen_plan(varlen, feature_index, emb_dim, slot0=0, dnn_off=0):
    return ops.VarLenPlan([feature_index[fc.name][0] for fc in varlen], [fc.maxlen for fc in varlen],
                          [None if fc.length_name is None else feature_index[fc.length_name][0] for fc in varlen],
                          [fc.combiner for fc in varlen], [fc.vocabulary_size for fc in varlen], emb_dim, slot0, dnn_off)


class Linear(nn.Module):
    """Parameters of the linear part: one [vocab,1] table per sparse field and a [n_dense,1] weight
    (deepctr/models/basemodel.py:34-92).  Inside the models its logit comes out of the fused gather;
    calling the module directly runs the same kernel for the linear part alone."""

    def __init__(self, feature_columns, feature_index, init_std=0.0001, device='cpu'):
        super().__init__()
        self.feature_index = feature_index
        self.device = device
        self.sparse_feature_columns, self.dense_feature_columns, self.varlen_sparse_feature_columns = \
            split_columns(feature_columns)
        _check_varlen(feature_columns)
        # All draws happen on the CPU generator and the module moves afterwards, so a seed gives the
        # same initial weights on every device (= the reference's CPU path; on a CUDA device the
        # reference itself would take these two draws from the device generator, basemodel.py:47-61).
        self.embedding_dict = create_embedding_matrix(feature_columns, init_std, linear=True, sparse=False,
                                                      device='cpu')
        for emb in self.embedding_dict.values():          # second draw, basemodel.py:55-56
            nn.init.normal_(emb.weight, mean=0, std=init_std)
        n_dense = sum(fc.dimension for fc in self.dense_feature_columns)
        if n_dense > 0:
            self.weight = nn.Parameter(torch.Tensor(n_dense, 1))
            nn.init.normal_(self.weight, mean=0, std=init_std)
        self._plan = self._vplan = None
        self.to(device)

    def tables(self):
        return [self.embedding_dict[fc.embedding_name].weight for fc in self.sparse_feature_columns]

    def varlen_tables(self):
        return [self.embedding_dict[fc.embedding_name].weight for fc in self.varlen_sparse_feature_columns]

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_plan"] = state["_vplan"] = None
        return state

    def forward(self, X, sparse_feat_refine_weight=None):
        if sparse_feat_refine_weight is not None:
            raise NotImplementedError("refine weights belong to IFM/DIFM, not to the xDeepFM path")
        if self._plan is None:
            dense_cols = [c for fc in self.dense_feature_columns for c in range(*self.feature_index[fc.name])]
            self._plan = ops.EmbedPlan([self.feature_index[fc.name][0] for fc in self.sparse_feature_columns],
                                       [fc.vocabulary_size for fc in self.sparse_feature_columns], dense_cols, 1)
            if self.varlen_sparse_feature_columns:
                self._vplan = _varlen_plan(self.varlen_sparse_feature_columns, self.feature_index, 1)
        if self.varlen_sparse_feature_columns and not self.sparse_feature_columns:
            raise NotImplementedError("the linear part needs at least one SparseFeat beside its VarLenSparseFeat columns")
        if not self.sparse_feature_columns:
            out = torch.zeros([X.shape[0], 1], device=X.device)
            if self.dense_feature_columns:
                cols = self._plan.dense_cols
                out = out + X[:, cols].matmul(self.weight)
            return out
        tabs = self.tables()
        w = self.weight if self.dense_feature_columns else None
        _, _, lin = ops.EmbedGather.apply(X, w, self._plan, True, *tabs, *tabs)
        if self.__dict__.get("_vplan") is not None:        # pooled [V, 1] rows of the variable-length fields, added in place
            _, _, lin = ops.VarLenPool.apply(X, None, None, lin, self._vplan, 0, *self.varlen_tables())
        return lin


def example_weights(y, sample_weight=None, class_weight=None, task="binary"):
    """The weight vector of `fit(sample_weight=, class_weight=)`: float32 [n], row i the weight of example i, or None when
    neither is given.  Checked once, on the host: `sample_weight` is one finite, non-negative weight per example (1-D or
    [n,1]); `class_weight` is {0: a, 1: b} with finite, non-negative values, for task 'binary' with labels that are
    exactly 0 or 1.  The effective weight is sample_weight * class_weight[y], formed here in float32 -- the kernels see
    one vector and no classes.  Anything else is a ValueError."""
    if sample_weight is None and class_weight is None:
        return None
    labels = np.asarray(y)
    n = labels.shape[0]
    w = np.ones((n,), dtype=np.float32)
    if sample_weight is not None:
        sw = np.asarray(sample_weight)
        if sw.dtype.kind not in "fiub" or not (sw.ndim == 1 or (sw.ndim == 2 and sw.shape[1] == 1)):
            raise ValueError("sample_weight must be a numeric 1-D array (or [n,1]), got dtype %s shape %s" % (sw.dtype, sw.shape))
        sw = sw.reshape(-1)
        if sw.shape[0] != n:
            raise ValueError("sample_weight has %d entries for %d examples" % (sw.shape[0], n))
        with np.errstate(over="ignore"):               # a weight beyond fp32 becomes inf and is refused below
            w = sw.astype(np.float32)
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("sample_weight must be finite and non-negative (also after the cast to float32)")
    if class_weight is not None:
        if task != "binary":
            raise ValueError("class_weight needs task='binary', the model's task is %r" % (task,))
        if not isinstance(class_weight, dict) or set(class_weight.keys()) != {0, 1}:
            raise ValueError("class_weight must be a dict {0: weight, 1: weight}, got %r" % (class_weight,))
        cw = np.asarray([class_weight[0], class_weight[1]], dtype=np.float32)
        if not np.all(np.isfinite(cw)) or np.any(cw < 0):
            raise ValueError("class_weight values must be finite and non-negative, got %r" % (class_weight,))
        flat = labels.reshape(-1)
        if flat.shape[0] != n or not np.all((flat == 0) | (flat == 1)):
            raise ValueError("class_weight needs one label per example, each exactly 0 or 1")
        w = w * cw[flat.astype(np.int64)]
    return np.ascontiguousarray(w, dtype=np.float32)


class BaseModel(nn.Module):
    _VARLEN = True      # the model's input stage pools VarLenSparseFeat columns (K1v); xDeepFMPro's does not

    def __init__(self, linear_feature_columns, dnn_feature_columns, l2_reg_linear=1e-5, l2_reg_embedding=1e-5,
                 init_std=0.0001, seed=1024, task='binary', device='cpu', gpus=None):
        super().__init__()
        torch.manual_seed(seed)                              # basemodel.py:100
        if gpus:
            raise ValueError("`gpus=` (single-process nn.DataParallel, basemodel.py:206-209) is replaced by one "
                             "process per GPU: launch with torch.distributed.run and leave gpus=None")
        self.dnn_feature_columns = dnn_feature_columns
        self.linear_feature_columns = linear_feature_columns
        self.device = device
        self.gpus = gpus
        self.reg_loss = torch.zeros((1,), device=device)
        self.aux_loss = torch.zeros((1,), device=device)
        self._aux_unset = True              # aux_loss is still the initial zero: the train step need not add it
        _check_varlen(linear_feature_columns)
        _check_varlen(dnn_feature_columns)
        if not self._VARLEN and split_columns(list(linear_feature_columns) + list(dnn_feature_columns))[2]:
            raise NotImplementedError("%s does not take VarLenSparseFeat columns (xDeepFM, xDeepFMAttention and "
                                      "xDeepFMAttentionV2 do)" % type(self).__name__)
        self.feature_index = build_input_features(list(linear_feature_columns) + list(dnn_feature_columns))
        self.embedding_dict = create_embedding_matrix(dnn_feature_columns, init_std, sparse=False, device=device)
        self.linear_model = Linear(linear_feature_columns, self.feature_index, device=device)
        self.regularization_weight = []
        self.add_regularization_weight(self.embedding_dict.parameters(), l2=l2_reg_embedding)
        self.add_regularization_weight(self.linear_model.parameters(), l2=l2_reg_linear)
        self.out = PredictionLayer(task, )
        self.to(device)
        self._is_graph_network = True       # attributes Keras callbacks look at (basemodel.py:133-135)
        self._ckpt_saved_epoch = False
        self.history = History()
        self.stop_training = False
        self._plan = None

    # ------------------------------------------------------------------ pickling (ModelCheckpoint with
    # save_weights_only=False calls torch.save(model), deepctr/callbacks.py:41-73)
    _UNPICKLED = ("_graphed_step", "_plan", "_l2_cache", "_unit_grad_cache", "_sparse_cols", "_fused_linear", "_own_step",
                  "_row_weight", "_vplan", "_varlen_cols")

    def __getstate__(self):
        state = self.__dict__.copy()
        for k in self._UNPICKLED:           # captured graphs, ctypes descriptors, device-side plans: rebuilt on first use
            state.pop(k, None)
        state["_plan"] = None
        return state

    # The optimizer may hold table rows that are several steps behind (optim.TableAdam, deferred update): whoever reads
    # or replaces the parameters as a whole -- evaluation, a checkpoint, a reload -- gets them brought up to date first.
    def _flush_optim(self):
        opt = self.__dict__.get("optim")
        if opt is not None and hasattr(opt, "flush"):
            opt.flush()

    def train(self, mode=True):
        if not mode:
            self._flush_optim()
        return super().train(mode)

    def state_dict(self, *args, **kwargs):
        self._flush_optim()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._flush_optim()
        return super().load_state_dict(*args, **kwargs)

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault("_plan", None)
        lm = self.__dict__.get("_modules", {}).get("linear_model")
        if lm is not None:
            lm._plan = lm._vplan = None

    def _plans(self):
        plans = [self._plan, getattr(self.linear_model, "_plan", None)]
        if self._plan is not None:
            plans.append(self.__dict__.get("_vplan"))
        plans.append(self.linear_model.__dict__.get("_vplan"))
        return [p for p in plans if p is not None]

    def _raise_on_bad_ids(self):
        """The reference's nn.Embedding raises IndexError (CPU) or device-asserts on an id outside [0, vocabulary_size)
        (basemodel.py:368-370).  K1 clamps such an id and raises a device flag instead of stopping the stream; the flag
        is read where the host synchronises anyway -- the per-epoch loss read-back of `fit`, the final copy of
        `predict` / `evaluate` -- so the error is deferred to the end of the epoch / call, never lost."""
        dev = torch.device(self.device) if not isinstance(self.device, torch.device) else self.device
        if dev.type != "cuda":
            return
        dp = xdist.current()
        for plan in self._plans():
            bad = plan.check_ids(dev)
            if dp is not None:
                bad = dp.any_flag(bad)       # every rank raises together: a lone IndexError would leave the others in a collective
            if bad:
                bounds = ", ".join("%d" % v for v in plan.vocab[:8]) + (" ..." if len(plan.vocab) > 8 else "")
                raise IndexError("index out of range in self: a sparse feature id lies outside [0, vocabulary_size) "
                                 "(vocabulary sizes: %s) -- check SparseFeat(vocabulary_size=max_id + 1)" % bounds)

    def _drop_table_grads(self):
        """After the model's own step the tables' `.grad` are views of the kept gradient buffer (all zeros again once K7
        has consumed them).  They are released so that code which drives autograd itself afterwards gets fresh dense
        gradients instead of accumulating into that buffer behind the optimizer's back."""
        tables = self._gather_tables()
        if tables is None or self._plan is None or not self._plan.arenas():
            return
        for t in tables:
            t.grad = None
        w = getattr(self.linear_model, "weight", None)
        if w is not None:
            w.grad = None

    # ------------------------------------------------------------------ fused input stage
    def _gather_plan(self):
        if self._plan is None:
            sparse, dense, varlen = split_columns(self.dnn_feature_columns)
            dims = {fc.embedding_dim for fc in sparse + varlen}
            if len(dims) > 1:
                raise ValueError("embedding_dim of SparseFeat and VarlenSparseFeat must be same in this model!")
            dp = xdist.current()
            lin_sparse = self.linear_model.sparse_feature_columns
            self._fused_linear = [fc.name for fc in lin_sparse] == [fc.name for fc in sparse] and \
                [fc.name for fc in self.linear_model.dense_feature_columns] == [fc.name for fc in dense] and \
                [fc.name for fc in self.linear_model.varlen_sparse_feature_columns] == [fc.name for fc in varlen]
            if dp is not None and not self._fused_linear and (varlen or self.linear_model.varlen_sparse_feature_columns):
                # without the fused gather there is no row exchange for the pooled fields' ids and gradients to ride on
                raise NotImplementedError("row-parallel training takes VarLenSparseFeat columns only when "
                                          "linear_feature_columns and dnn_feature_columns list the same columns in the same order")
            dense_cols = [c for fc in dense for c in range(*self.feature_index[fc.name])]
            D = dims.pop() if dims else 1
            # the pooled variable-length fields follow the sparse ones: field slots m .. m+F-1 of the CIN input,
            # columns m*D .. of the DNN input (sparse_embedding_list + varlen_sparse_embedding_list, basemodel.py:377)
            self._plan = ops.EmbedPlan([self.feature_index[fc.name][0] for fc in sparse],
                                       [fc.vocabulary_size for fc in sparse], dense_cols, D, extra_fields=len(varlen))
            self._vplan = _varlen_plan(varlen, self.feature_index, D, len(sparse), len(sparse) * D) if varlen else None
            self._sparse_cols = sparse
            self._varlen_cols = varlen
            if dp is not None and self._fused_linear:
                # these gradients are built from the all-gathered rows and are identical on every rank
                self._plan.dp = dp
                dp.mark_replicated([self.embedding_dict[fc.embedding_name].weight for fc in sparse])
                dp.mark_replicated(self.linear_model.parameters())
                if varlen:
                    # the pooled fields ride on the same exchange: K2v runs over all ranks' rows (ops.varlen_rows_grads)
                    vtabs = [self.embedding_dict[fc.embedding_name].weight for fc in varlen]
                    self._vplan.gather = self._plan
                    self._plan.varlen_owners = vtabs + self.linear_model.varlen_tables()
                    dp.mark_replicated(vtabs)
        return self._plan

    def fused_inputs(self, X):
        """(emb_fm [m, B*D], dnn_in [B, m*D+nd], linear_logit [B,1]) from ONE gather launch
        (input_from_feature_columns + linear_model + both concatenations of the reference forward).  With F
        variable-length columns m counts them too: a second launch pools them into their slots of the same tensors."""
        plan = self._gather_plan()
        self._use_grad_arena(plan)
        if not self._sparse_cols:
            raise NotImplementedError("the xDeepFM path needs at least one SparseFeat")
        tabs = [self.embedding_dict[fc.embedding_name].weight for fc in self._sparse_cols]
        vplan = self._vplan
        vtabs = [self.embedding_dict[fc.embedding_name].weight for fc in self._varlen_cols]
        if self._fused_linear:
            w = getattr(self.linear_model, "weight", None)
            out = ops.EmbedGather.apply(X, w, plan, True, *tabs, *self.linear_model.tables())
            if vplan is None:
                return out
            return ops.VarLenPool.apply(X, out[0], out[1], out[2], vplan, vplan.F, *vtabs, *self.linear_model.varlen_tables())
        emb_fm, dnn_in, _ = ops.EmbedGather.apply(X, None, plan, False, *tabs)
        if vplan is not None:
            emb_fm, dnn_in, _ = ops.VarLenPool.apply(X, emb_fm, dnn_in, None, vplan, vplan.F, *vtabs)
        return emb_fm, dnn_in, self.linear_model(X)

    def input_from_feature_columns(self, X, feature_columns, embedding_dict, support_dense=True):
        """API of basemodel.py:354-380: ([B,1,D] per sparse field, then per pooled variable-length field; [B,k] per
        dense field)."""
        sparse, dense, varlen = split_columns(feature_columns)
        _check_varlen(feature_columns)
        if not support_dense and len(dense) > 0:
            raise ValueError("DenseFeat is not supported in dnn_feature_columns")
        if varlen and not sparse:
            raise NotImplementedError("the xDeepFM path needs at least one SparseFeat")
        emb_list = []
        if sparse:
            plan = ops.EmbedPlan([self.feature_index[fc.name][0] for fc in sparse],
                                 [fc.vocabulary_size for fc in sparse], [], sparse[0].embedding_dim, extra_fields=len(varlen))
            tabs = [embedding_dict[fc.embedding_name].weight for fc in sparse]
            emb_fm, _, _ = ops.EmbedGather.apply(X, None, plan, False, *tabs)
            if varlen:
                vplan = _varlen_plan(varlen, self.feature_index, plan.D, plan.m, plan.m * plan.D)
                emb_fm, _, _ = ops.VarLenPool.apply(X, emb_fm, None, None, vplan, vplan.F,
                                                    *[embedding_dict[fc.embedding_name].weight for fc in varlen])
            B = X.shape[0]
            emb_list = [emb_fm[j].view(B, 1, plan.D) for j in range(plan.m + len(varlen))]
        dense_list = [X[:, self.feature_index[fc.name][0]:self.feature_index[fc.name][1]] for fc in dense]
        return emb_list, dense_list

    def compute_input_dim(self, feature_columns, include_sparse=True, include_dense=True, feature_group=False):
        sparse, dense, varlen = split_columns(feature_columns)
        sparse = sparse + varlen
        dim = 0
        if include_sparse:
            dim += len(sparse) if feature_group else sum(fc.embedding_dim for fc in sparse)
        if include_dense:
            dim += sum(fc.dimension for fc in dense)
        return dim

    @property
    def embedding_size(self):
        sparse, _, varlen = split_columns(self.dnn_feature_columns)
        sizes = {fc.embedding_dim for fc in sparse + varlen}
        if len(sizes) > 1:
            raise ValueError("embedding_dim of SparseFeat and VarlenSparseFeat must be same in this model!")
        return list(sizes)[0]

    # ------------------------------------------------------------------ regularisation
    def add_regularization_weight(self, weight_list, l1=0.0, l2=0.0):
        weight_list = [weight_list] if isinstance(weight_list, nn.parameter.Parameter) else list(weight_list)
        self.regularization_weight.append((weight_list, l1, l2))

    def _l2_terms(self):
        """[(tensor, l2 strength)] of every regularised tensor with l2 > 0, and the summed l1 term."""
        l2_terms, l1_total = [], None
        for weight_list, l1, l2 in self.regularization_weight:
            for w in weight_list:
                p = w[1] if isinstance(w, tuple) else w
                if l1 > 0:
                    term = torch.sum(l1 * torch.abs(p))
                    l1_total = term if l1_total is None else l1_total + term
                if l2 > 0:
                    l2_terms.append((p, float(l2)))
        return l2_terms, l1_total

    def _l2_fusion(self):
        """(tensors, strengths) of the whole L2 term when the optimizer applies it itself while it streams the
        weights (xdfm_amd.optim.TableAdam / TableSGD / TableAdagrad / TableRMSprop: K7, K7s, K7g, K7r), else None.  Only the model's own
        train step uses this."""
        opt = getattr(self, "optim", None)
        if not getattr(opt, "table_step", False):
            return None
        tensors, coeffs = [], []
        for weight_list, l1, l2 in self.regularization_weight:
            for w in weight_list:
                p = w[1] if isinstance(w, tuple) else w
                if l1 > 0 or not p.is_cuda:
                    return None
                if l2 > 0:
                    tensors.append(p)
                    coeffs.append(float(l2))
        if not opt.owns(tensors):
            return None
        return tensors, coeffs

    def _gather_tables(self):
        """The tensors the fused gather reads, in its order (None before the first forward)."""
        if self._plan is None or not getattr(self, "_fused_linear", False):
            return None
        return [self.embedding_dict[fc.embedding_name].weight for fc in self._sparse_cols] + \
            self.linear_model.tables()

    def get_regularization_loss(self, _defer_tables=False, _part="all"):
        """sum over groups of l1*|w| + l2*w^2 (basemodel.py:412-428), shape [1].  All l2 groups are
        evaluated by one multi-tensor launch (K6) instead of four ATen calls per tensor.

        The private arguments are used by the model's own train step only.  `_defer_tables`: the L2
        gradient of the embedding tables is produced inside the gather's backward (as the initial value
        of the dense table gradients) instead of as table-sized tensors that autograd has to add.
        `_part`: "all", or "tables" / "rest" to split the term (row-parallel training adds the rest
        after the gradient all-reduce)."""
        l2_terms, total = self._l2_terms()
        tables = self._gather_tables()
        table_ids = {id(t) for t in tables} if tables is not None else set()
        if _part == "tables":
            l2_terms, total = [x for x in l2_terms if id(x[0]) in table_ids], None
        elif _part == "rest":
            l2_terms = [x for x in l2_terms if id(x[0]) not in table_ids]
        if l2_terms:
            cache = self.__dict__.setdefault("_l2_cache", {})
            embed_plan, n_defer = None, 0
            if _defer_tables and tables is not None and _part != "rest":
                coeff_of = {id(p): c for p, c in l2_terms}
                if all(id(t) in coeff_of for t in tables) and all(t.requires_grad for t in tables):
                    l2_terms = [(t, coeff_of[id(t)]) for t in tables] + [x for x in l2_terms if id(x[0]) not in table_ids]
                    embed_plan, n_defer = self._plan, len(tables)
            term = ops.l2_regulariser([p for p, _ in l2_terms], [c for _, c in l2_terms], cache, embed_plan, n_defer)
            total = term if total is None else total + term
        if total is None:
            total = torch.zeros((1,), device=self.device)
        return total.reshape(1)

    def train_on_batch(self, x, y, sample_weight=None):
        """One optimisation step = the body of the reference's batch loop (basemodel.py:245-262):
        forward, BCE(sum) + L2 (+ aux), backward, optimizer step.  Returns (y_pred, data_loss,
        total_loss) as device tensors -- no host synchronisation.  On a GPU, from the third step of a
        batch shape on, the step is replayed from a captured HIP graph (xdfm_amd/graphstep.py); the
        returned tensors are then the graph's static outputs, valid until the next call.
        `sample_weight` ([B] or [B,1] float32 on the device of `y`, or None): the data loss becomes
        sum_b w_b loss(pred_b, y_b) (the native head takes the vector, K8); the L2 term is not weighted."""
        step = self.__dict__.get("_graphed_step")
        if step is None:
            from .graphstep import GraphedStep
            step = self.__dict__["_graphed_step"] = GraphedStep(self)
        if sample_weight is None:
            return step(x, y)
        if sample_weight.numel() != x.shape[0] or sample_weight.dim() > 2:
            raise ValueError("sample_weight must hold one weight per row of x ([B] or [B,1]), got shape %s"
                             % (tuple(sample_weight.shape),))
        return step(x, y, sample_weight)

    def _fused_head(self, x, y, sw=None):
        """(y_pred, summed data loss) through one launch (ops.Head) when the model is of the xDeepFM family (it has
        `head_inputs`) and its task and compiled loss have a native head (ops.head_mode: binary / regression with
        binary_crossentropy / mse / mae, except regression + binary_crossentropy); None otherwise."""
        if not hasattr(self, "head_inputs") or not x.is_cuda:
            return None
        out = self.out
        mode = ops.head_mode(getattr(out, "task", None), self.loss_func)
        if mode is None or y.numel() != x.shape[0]:
            return None
        lin, cin_out, dnn_out = self.head_inputs(x)
        return ops.Head.apply(y, out.bias if out.use_bias else None, lin,
                              cin_out, self.cin_linear.weight if cin_out is not None else None,
                              dnn_out, self.dnn_linear.weight if dnn_out is not None else None, *mode,
                              *(() if sw is None else (sw.float(),)))

    def _loss_forward(self, x, y, sw=None):
        """(y_pred, data loss): forward + loss of the reference's batch loop (basemodel.py:250-254).  With example
        weights `sw` the loss is sum_b sw_b loss(pred_b, y_b): by the native head, or (stock tail) by the loss function
        with reduction='none'."""
        head = self._fused_head(x, y) if sw is None else self._fused_head(x, y, sw)
        if head is not None:
            y_pred, loss = head
            return y_pred, loss.reshape(())
        y_pred = self(x).squeeze()
        loss_func = self.loss_func
        if isinstance(loss_func, list):
            assert len(loss_func) == self.num_tasks, "the length of `loss_func` should be equal with `self.num_tasks`"
            if sw is not None:
                raise NotImplementedError("sample_weight with a list of losses")
            loss = sum(loss_func[i](y_pred[:, i], y[:, i], reduction='sum') for i in range(self.num_tasks))
        elif sw is not None:
            loss = (sw.reshape(-1).to(y_pred.dtype) * loss_func(y_pred.reshape(-1), y.reshape(-1), reduction='none')).sum()
        else:
            loss = loss_func(y_pred, y.squeeze(), reduction='sum')
        return y_pred, loss

    # Row-parallel step with the L2 term in K7, in two halves.  The first (forward, loss, backward down to the
    # row gradients of the gather) contains no collective, so it can be replayed from a HIP graph; the second
    # exchanges the rows, scatters, all-reduces the dense gradients and runs the optimizer, eagerly.
    def _use_grad_arena(self, plan):
        """Keep the dense table gradients across steps when the optimizer can consume them by their marks -- inside the
        model's OWN train step only (`_own_step`): there nothing touches a gradient between the scatter and K7.  A
        user-driven loop (model(x); loss.backward(); edit .grad; optim.step()) gets ordinary dense gradients, because
        K7 would not see what such code adds outside the marked chunks."""
        plan.arena_on = bool(self.__dict__.get("_own_step")) and bool(getattr(getattr(self, "optim", None), "table_step", False))
        if plan.arena_on and plan not in self.optim.grad_sources:
            self.optim.grad_sources.append(plan)

    @contextlib.contextmanager
    def _own_step_scope(self):
        prev = self.__dict__.get("_own_step", False)
        self.__dict__["_own_step"] = True
        if self._plan is not None:
            self._use_grad_arena(self._plan)
        try:
            yield
        finally:
            self.__dict__["_own_step"] = prev
            if self._plan is not None and not prev:
                self._plan.arena_on = False

    def _with_step_extra(self, total):
        """A model's `_loss_forward` may leave a further differentiable term of the step's objective in `_step_extra`
        (xDeepFMPro: sfg_weight * sfg_loss, basemodel_sfg.py:343) and a value for the epoch log in `_step_log`."""
        extra = self.__dict__.get("_step_extra")
        return total if extra is None else total + extra.reshape(total.shape)

    def _unit_grad(self, loss):
        """Root gradient of a backward pass, cached: autograd would otherwise fill a fresh ones tensor every step.
        A rank that holds only a stand-in row (a global batch with fewer rows than ranks, dist.RowParallel.shard)
        differentiates with a zero root: all its data gradients are exact zeros."""
        if self.__dict__.get("_row_weight", 1.0) == 0.0:
            return torch.zeros_like(loss)
        key = (tuple(loss.shape), loss.device, loss.dtype)
        hit = self.__dict__.get("_unit_grad_cache")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_unit_grad_cache"] = (key, torch.ones_like(loss))
        return hit[1]

    def _split_step_first(self, x, y, sw=None):
        with self._own_step_scope():
            return self._split_step_first_body(x, y, sw)

    def _split_step_first_body(self, x, y, sw=None):
        self.optim.zero_grad()
        plan = self._gather_plan()
        plan.stash = []
        try:
            y_pred, loss = self._loss_forward(x, y) if sw is None else self._loss_forward(x, y, sw)
            root = loss if self._aux_unset else loss + self.aux_loss
            root = self._with_step_extra(root)
            root.backward(self._unit_grad(root))
            stash = plan.stash
        finally:
            plan.stash = None
        return y_pred.detach(), loss.detach(), stash

    def _split_step_second(self, y_pred, loss, stash, fuse):
        with self._own_step_scope():
            out = self._split_step_second_body(y_pred, loss, stash, fuse)
        self._drop_table_grads()
        return out

    def _split_step_second_body(self, y_pred, loss, stash, fuse):
        dp = xdist.current()
        dense_w = self.linear_model.weight if getattr(self.linear_model, "dense_feature_columns", None) else None
        ops.apply_stashed_scatter(stash, dense_w, self._gather_tables())
        if dp is not None:
            dp.reduce_dense_grads(self)
        self.optim.arm_l2(*fuse)
        self.optim.step()
        total_loss = loss if self._aux_unset else loss + self.aux_loss.detach()
        if self.__dict__.get("_step_extra") is not None:
            total_loss = total_loss + self._step_extra.detach().reshape(total_loss.shape)
        if self.optim.l2_value is not None:
            total_loss = total_loss + self.optim.l2_value
        return y_pred, loss, total_loss.detach()

    def _can_split_step(self, dp, fuse):
        if dp is None or fuse is None:
            return False
        # a tower with synchronised batch norm (XDFM_DNN_BN_SYNC) holds collectives in its forward and backward: no
        # collective-free first half to capture, the step runs by the eager branch below
        if any(isinstance(mod, DNN) and mod.takes_bn_sync(dp) for mod in self.modules()):
            return False
        self._gather_plan()
        return bool(getattr(self, "_fused_linear", False))

    def _train_step_eager(self, x, y, sw=None):
        with self._own_step_scope():
            out = self._train_step_eager_body(x, y, sw)
        self._drop_table_grads()
        return out

    def _train_step_eager_body(self, x, y, sw=None):
        dp = xdist.current()
        fuse = self._l2_fusion()
        if self._can_split_step(dp, fuse):
            y_pred, loss, stash = self._split_step_first(x, y, sw)
            return self._split_step_second(y_pred, loss, stash, fuse)
        self.optim.zero_grad()
        if fuse is not None:
            return self._train_step_fused_l2(x, y, sw, dp, fuse)
        y_pred, loss = self._loss_forward(x, y) if sw is None else self._loss_forward(x, y, sw)
        if dp is None:
            reg_loss = self.get_regularization_loss(_defer_tables=True)
            total_loss = self._with_step_extra(loss + reg_loss + self.aux_loss)
            total_loss.backward()
        else:
            # Data-loss gradients are SUMMED over ranks (the loss is a sum over the global batch); the L2
            # term is identical on every replica and must be applied once.  Tables: their gradient is
            # built from the all-gathered rows (identical on all ranks) with the L2 term folded in.
            # Dense weights: all-reduce the data gradients, then add the L2 gradient locally.
            reg_t = self.get_regularization_loss(_defer_tables=True, _part="tables")
            reg_d = self.get_regularization_loss(_part="rest")
            # A model's further term (`_step_extra`) is a sum over the rows of the shard like the data loss.
            self._with_step_extra(loss * self.__dict__.get("_row_weight", 1.0) + reg_t).backward()
            dp.reduce_dense_grads(self)
            (reg_d + self.aux_loss).backward()
            total_loss = self._with_step_extra(loss.detach() + reg_t.detach() + reg_d.detach() + self.aux_loss).detach()
        self.optim.step()
        # detached: a caller that keeps these alive must not keep the step's autograd graph (and with it the
        # parameters' AccumulateGrad nodes and their stream) alive into the next step
        return y_pred.detach(), loss.detach(), total_loss.detach()

    def _train_step_fused_l2(self, x, y, sw, dp, fuse):
        """The step whose L2 term (gradient and value) comes from K7 (added after the gradient all-reduce when row-parallel:
        the term is identical on every replica and must count once).  Its one-block finish launches run as two finish batches
        (ops.finish_batch_begin): one for forward + backward, run before anything reads a gradient, and one for the
        optimizer.  The head's loss value joins the first: with the data loss as the whole objective nothing reads it before
        the step's last line; a further term (aux_loss, `_step_extra`) is added to it on the device, so the batch runs first."""
        ops.finish_batch_begin()
        try:
            cin = getattr(self, "cin", None)
            if getattr(self, "use_cin", False) and x.is_cuda and hasattr(cin, "announce_pack"):
                cin.announce_pack()                     # the CIN weight packs ride on the catch-up and the gather
            y_pred, loss = self._loss_forward(x, y) if sw is None else self._loss_forward(x, y, sw)
            ops.cin_pack_drop()                         # (no CIN forward took them: issued all the same)
            self.optim.arm_l2(*fuse)
            if not self._aux_unset or self.__dict__.get("_step_extra") is not None:
                ops.finish_batch_flush()
            total_loss = loss if self._aux_unset else loss + self.aux_loss
            total_loss = self._with_step_extra(total_loss)
            # the dW slab sums of the CIN levels ride on later launches of the backward; until the flush nothing may read a CIN
            # weight gradient (zero_grad left `.grad` None: no accumulation kernel, no hooks here) -- see ops.rider_begin
            ops.rider_begin()
            total_loss.backward(self._unit_grad(total_loss))
            ops.rider_flush()
            ops.finish_batch_run()
            if dp is not None:
                dp.reduce_dense_grads(self)
            ops.finish_batch_begin()
            self.optim.step()
            l2 = self.optim.l2_value
            if l2 is not None:
                a = total_loss.detach()
                total_loss = ops.finish_add(a, l2)      # behind the finish that leaves the value, in the optimizer's batch
            ops.finish_batch_run()
        except BaseException:
            ops.cin_pack_drop(quiet=True)
            ops.rider_flush(quiet=True)
            ops.finish_batch_run(quiet=True)
            raise
        return y_pred.detach(), loss.detach(), total_loss.detach()

    def _global_batch_labels(self, y):
        """`fit` under row-parallel training: the labels of the global batch, before they are sharded.  A model whose
        objective has a term normalised over the global batch (xDeepFMPro's SFG loss) keeps them for the step."""

    def add_auxiliary_loss(self, aux_loss, alpha):
        self.aux_loss = aux_loss * alpha
        self._aux_unset = False

    # ------------------------------------------------------------------ compile
    def compile(self, optimizer, loss=None, metrics=None, weighted_metrics=None):
        """`weighted_metrics` (Keras's name): the same names as `metrics`; each gives a `weighted_<name>` entry computed with
        the example weights of `fit` / `evaluate` (xdfm_amd.metrics.weighted_*).  None or []: nothing about the model changes."""
        self.metrics_names = ["loss"]
        self._optim_capturable = False
        self._flush_optim()                # a previous optimizer may still owe table rows their latest steps
        self.optim = self._get_optim(optimizer)
        # the table optimizers (optim.TableAdam / TableSGD / TableAdagrad / TableRMSprop / TableFTRL / TableRowwiseAdagrad), also when handed in as an object, e.g.
        # TableAdam(..., lazy_rows=True); an object of a stock torch class keeps the stock path
        if getattr(self.optim, "table_step", False):
            self._optim_capturable = all(p.is_cuda for g in self.optim.param_groups for p in g["params"])
        self.loss_func = self._get_loss_func(loss)
        self.metrics = self._get_metrics(metrics)
        self.weighted_metrics = self._get_weighted_metrics(weighted_metrics)

    def _get_weighted_metrics(self, names):
        """{"weighted_" + name: weighted function} for the names `_get_metrics` knows, in the order given; as there, a name it
        does not know gets a History name and no function."""
        table = {"binary_crossentropy": M.weighted_log_loss, "logloss": M.weighted_log_loss, "auc": M.weighted_roc_auc_score,
                 "mse": M.weighted_mean_squared_error, "accuracy": M.weighted_accuracy_score, "acc": M.weighted_accuracy_score}
        out = {}
        for name in (names or []):
            if name in table:
                out["weighted_" + name] = table[name]
            self.metrics_names.append("weighted_" + name)
        return out

    @staticmethod
    def _weighted_slots():
        """{weighted function `compile` wires in: (its slot of out4, the unweighted function it equals under unit weights)}"""
        return {M.weighted_log_loss: (0, M.log_loss), M.weighted_roc_auc_score: (1, M.roc_auc_score),
                M.weighted_mean_squared_error: (2, M.mean_squared_error),
                M.weighted_accuracy_score: (3, BaseModel._accuracy_score)}

    def _get_optim(self, optimizer):
        if not isinstance(optimizer, str):
            return optimizer
        def adam(params):
            # same update rule as basemodel.py:452; on a GPU use torch's single-pass multi-tensor kernel
            params = list(params)
            on_gpu = len(params) > 0 and all(p.is_cuda for p in params)
            # capturable: the step counters live on the device, so the step can be replayed from a HIP graph
            self._optim_capturable = on_gpu
            if on_gpu:
                from .optim import TableAdam
                return TableAdam(params)
            return torch.optim.Adam(params)
        def native(table_cls, stock):
            # SGD / Adagrad / RMSprop through K7s / K7g / K7r on a GPU (xdfm_amd.optim); on the CPU the stock class, as the reference
            def make(params):
                params = list(params)
                if len(params) > 0 and all(p.is_cuda for p in params):
                    from . import optim
                    return getattr(optim, table_cls)(params)
                return stock(params)
            return make
        table = {"sgd": native("TableSGD", lambda p: torch.optim.SGD(p, lr=0.01)), "adam": adam,
                 "adagrad": native("TableAdagrad", torch.optim.Adagrad),
                 "rmsprop": native("TableRMSprop", torch.optim.RMSprop)}

        def ftrl(params):
            # per-coordinate FTRL-Proximal: the reference has none; TableFTRL on a CPU model too, where it takes its torch-op path
            from .optim import TableFTRL
            return TableFTRL(list(params))
        table["ftrl"] = ftrl
        if optimizer == "rowwise_adagrad":
            # row-wise Adagrad: the reference has none; its groups come from the model (tables row-wise, the rest element-wise), on
            # a CPU model too, where it takes its torch-op path
            from .optim import TableRowwiseAdagrad
            return TableRowwiseAdagrad.for_model(self)
        if optimizer not in table:
            raise NotImplementedError
        return table[optimizer](self.parameters())

    def _get_loss_func(self, loss):
        names = {"binary_crossentropy": F.binary_cross_entropy, "mse": F.mse_loss, "mae": F.l1_loss}

        def one(name):
            if name not in names:
                raise NotImplementedError
            return names[name]
        if isinstance(loss, str):
            return one(loss)
        if isinstance(loss, list):
            return [one(l) for l in loss]
        return loss

    @staticmethod
    def _accuracy_score(y_true, y_pred):
        return M.accuracy_score(y_true, np.where(y_pred > 0.5, 1, 0))

    def _get_metrics(self, metrics, set_eps=False):
        out = {}
        for name in (metrics or []):
            if name in ("binary_crossentropy", "logloss"):
                out[name] = M.log_loss
            if name == "auc":
                out[name] = M.roc_auc_score
            if name == "mse":
                out[name] = M.mean_squared_error
            if name in ("accuracy", "acc"):
                out[name] = self._accuracy_score
            self.metrics_names.append(name)
        return out

    def _native_metric_slots(self, y_true, y_pred, max_rows):
        """{History key: slot of xdfm_batch_metrics' out4} for the entries of `self.metrics` that K14 serves in this fit: the
        switch ops.METRICS_NATIVE on, fp32 labels and predictions on a GPU, a global batch within the kernel's cap, and the
        entry still the function `_get_metrics` wires in (a callable the user put there keeps the path it had)."""
        if not (ops.METRICS_NATIVE and max_rows <= ops.METRICS_MAX_ROWS and ops.batch_metrics_supported(y_true, y_pred)):
            return {}
        table = self._wired_slots()
        return {name: table[fn] for name, fn in self.metrics.items() if fn in table}

    @staticmethod
    def _wired_slots():
        """{function `_get_metrics` wires in: its slot of out4} -- the table of K14 (`fit`) and K14s (`evaluate`)."""
        return {M.log_loss: 0, M.roc_auc_score: 1, M.mean_squared_error: 2, BaseModel._accuracy_score: 3}

    def _in_multi_worker_mode(self):
        return None

    # ------------------------------------------------------------------ data plumbing
    def _as_matrix(self, x):
        """dict / list of per-feature arrays -> one [N, n_cols] array in feature_index order
        (basemodel.py:155-156,191-197)."""
        if isinstance(x, dict):
            x = [x[name] for name in self.feature_index]
        x = [np.expand_dims(a, axis=1) if len(a.shape) == 1 else a for a in x]
        return np.concatenate(x, axis=-1)

    def _resident(self, x, y=None):
        """The packed inputs as float32 tensors -- what `x.to(device).float()` (basemodel.py:242-243) yields
        batch by batch -- placed on the model's device once when they fit, otherwise kept on the host."""
        X = torch.from_numpy(np.ascontiguousarray(self._as_matrix(x))).float()
        Y = None if y is None else torch.from_numpy(np.asarray(y)).float()
        if X.numel() * 4 <= RESIDENT_LIMIT_BYTES:
            X = X.to(self.device)
            Y = None if Y is None else Y.to(self.device)
        return X, Y

    @staticmethod
    def _rows(t, order, start, stop):
        if order is None:
            return t[start:stop]
        return t.index_select(0, order[start:stop])

    # ------------------------------------------------------------------ fit / evaluate / predict
    def fit(self, x=None, y=None, batch_size=None, epochs=1, verbose=1, initial_epoch=0, validation_split=0.,
            validation_data=None, shuffle=True, callbacks=None, sample_weight=None, class_weight=None):
        """Training loop with the observable behaviour of basemodel.py:137-309: same batch order for a
        given torch seed (the stock DataLoader draws it), BCE(sum) + L2, History keys, callbacks.
        `sample_weight` / `class_weight` (see `example_weights`): the data loss of a step is sum_b w_b loss_b.  The
        History `loss` stays (sum of weighted data loss + L2) / sample_num -- the reference's normaliser, not sum(w).
        The unweighted metrics and `predict` take no weights.  A model compiled with `weighted_metrics` also logs
        `weighted_<name>` per step from the step's weights (unit weights without any) and `val_weighted_<name>` from the
        validation weights: the tail of the weight vector under `validation_split`, else the third item of `validation_data`
        times `class_weight`; on any other model that third item is accepted and ignored, as in the reference."""
        if isinstance(x, dict):
            x = [x[name] for name in self.feature_index]
        task = getattr(self.out, "task", None)
        w_all = example_weights(y, sample_weight, class_weight, task)
        wm = getattr(self, "weighted_metrics", None) or {}
        do_validation = False
        val_x, val_y, val_w = [], [], None
        if validation_data:
            do_validation = True
            if len(validation_data) == 2:
                val_x, val_y = validation_data
            elif len(validation_data) == 3:
                val_x, val_y, val_w = validation_data
            else:
                raise ValueError('When passing a `validation_data` argument, it must contain either 2 items '
                                 '(x_val, y_val), or 3 items (x_val, y_val, val_sample_weights). '
                                 'However we received `validation_data=%s`' % (validation_data,))
            if isinstance(val_x, dict):
                val_x = [val_x[name] for name in self.feature_index]
            val_w = example_weights(val_y, val_w, class_weight, task) if wm else None
        elif validation_split and 0. < validation_split < 1.:
            do_validation = True
            n0 = x[0].shape[0] if hasattr(x[0], 'shape') else len(x[0])
            split_at = int(n0 * (1. - validation_split))
            x, val_x = _slice(x, 0, split_at), _slice(x, split_at)
            y, val_y = _slice(y, 0, split_at), _slice(y, split_at)
            if w_all is not None:
                # the validation part's weights serve the weighted metrics alone: the unweighted validation takes none
                w_all, val_w = w_all[:split_at], (w_all[split_at:] if wm else None)

        X_all, Y_all = self._resident(x, y)
        W_all = None if w_all is None else torch.from_numpy(w_all).to(X_all.device)    # resident with X / Y
        if batch_size is None:
            batch_size = 256
        self.train()
        dp = xdist.current()
        if dp is not None and verbose > 0:
            print("row-parallel on %d ranks (RCCL), global batch %d" % (dp.world, batch_size * dp.world))
        if dp is None:
            print(self.device)
        global_bs = batch_size * (dp.world if dp is not None else 1)   # `batch_size` is per GPU, as basemodel.py:209
        sample_num = X_all.shape[0]
        steps_per_epoch = (sample_num - 1) // global_bs + 1

        cbs = CallbackList((callbacks or []) + [self.history])
        cbs.set_model(self)
        cbs.on_train_begin()
        cbs.set_model(self)
        self.stop_training = False
        print("Train on {0} samples, validate on {1} samples, {2} steps per epoch".format(
            sample_num, len(val_y), steps_per_epoch))
        loss_log = metric_log = native_log = wnative_log = None
        for epoch in range(initial_epoch, epochs):
            cbs.on_epoch_begin(epoch)
            epoch_logs, train_result = {}, {}
            t_epoch = time.time()
            total_loss_epoch = 0.0
            step_no = 0
            logged = {}
            native_logged = {}
            wlogged, wresult = {}, {}
            has_extra = False
            order = epoch_order(sample_num, shuffle)
            if order is not None:
                order = order.to(X_all.device)
            it = range(0, sample_num, global_bs)
            bar = tqdm(it, disable=verbose != 1) if tqdm is not None else None
            try:
                for start in (bar if bar is not None else it):
                    xb = self._rows(X_all, order, start, start + global_bs)
                    yb = self._rows(Y_all, order, start, start + global_bs)
                    wb = None if W_all is None else self._rows(W_all, order, start, start + global_bs)
                    if dp is not None:
                        self._global_batch_labels(yb)
                        xb, yb = dp.shard(xb), dp.shard(yb)
                        wb = None if wb is None else dp.shard(wb)
                        self.__dict__["_row_weight"] = dp.row_weight()
                    xd = xb.to(self.device)
                    yd = yb.to(self.device)
                    wd = None if wb is None else wb.to(self.device)
                    if wd is None:
                        y_pred, loss, total_loss = self.train_on_batch(xd, yd)
                    else:
                        y_pred, loss, total_loss = self.train_on_batch(xd, yd, wd)
                    if dp is not None and dp.row_weight() == 0.0:
                        # stand-in row of a rank without rows in this (tail) batch: contributes nothing
                        total_loss = total_loss - loss
                        loss = loss * 0.0
                    # The reference reads the loss back every step (`total_loss.item()`, basemodel.py:262): a host
                    # sync per step that leaves the GPU idle while the next step is being enqueued.  The values are
                    # parked on the device instead and read once per epoch, summed in the same order in double.
                    if loss_log is None or loss_log.device != total_loss.device:
                        loss_log = torch.zeros((steps_per_epoch + 1, 4), dtype=torch.float32, device=total_loss.device)
                    loss_log[step_no, 0:1].copy_(loss.detach().reshape(1))
                    loss_log[step_no, 1:2].copy_(total_loss.detach().reshape(1))
                    step_log = self.__dict__.get("_step_log")           # (name, value) a model wants summed per epoch
                    if step_log is not None:
                        loss_log[step_no, 2:3].copy_(step_log[1].reshape(1))
                    step_extra = self.__dict__.get("_step_extra")       # the further term of the step's objective, if any
                    if step_extra is not None:              # a step without the term leaves the zero the column holds
                        has_extra = True
                        loss_log[step_no, 3:4].copy_(step_extra.detach().reshape(1))
                    step_no += 1
                    if verbose > 0:
                        yt, yp = yd, y_pred
                        if dp is not None:
                            yt, yp = dp.gather_rows(yd.reshape(-1)), dp.gather_rows(y_pred.detach().reshape(-1))
                        # K14: every metric that is still the function `compile` put there, from ONE ops.batch_metrics call
                        # (two launches) into a float64 log read once per epoch
                        native = self._native_metric_slots(yt, yp, global_bs)
                        if native:
                            if native_log is None or native_log.device != yt.device:
                                native_log = torch.empty((steps_per_epoch + 1, 4), dtype=torch.float64, device=yt.device)
                            ops.batch_metrics(yt, yp, sum({1 << s for s in native.values()}), native_log[step_no - 1])
                            native_logged.update(native)
                        for k, (name, fn) in enumerate(self.metrics.items()):
                            if name in native:
                                continue
                            dev_fn = M.DEVICE.get(fn) if yt.is_cuda else None
                            if dev_fn is None:
                                train_result.setdefault(name, []).append(
                                    fn(yt.cpu().data.numpy(), yp.cpu().data.numpy().astype("float64")))
                                continue
                            # same metric on the device, parked beside the losses and read once per epoch
                            if metric_log is None or metric_log.device != yt.device:
                                metric_log = torch.empty((steps_per_epoch + 1, max(len(self.metrics), 1)),
                                                         dtype=torch.float64, device=yt.device)
                            metric_log[step_no - 1, k:k + 1].copy_(dev_fn(yt, yp.detach()).reshape(1))
                            logged[name] = k
                        if wm:
                            wt = wd if wd is None or dp is None else dp.gather_rows(wd.reshape(-1))
                            wnative_log = self._log_weighted_step(yt, yp.detach(), wt, global_bs, steps_per_epoch, step_no - 1,
                                                                  wnative_log, wlogged, wresult)
            except KeyboardInterrupt:
                if bar is not None:
                    bar.close()
                raise
            if bar is not None:
                bar.close()
            self.__dict__["_row_weight"] = 1.0
            if step_no:
                data_l, total_l = loss_log[:step_no, 0], loss_log[:step_no, 1]
                if dp is not None:
                    # the data loss is a SUM over the global batch; the L2 part (total - data) is the same on every rank
                    data_sum = dp.all_reduce_sum(data_l.clone())
                    vals = [a + (t - d) for a, t, d in zip(data_sum.tolist(), total_l.tolist(), data_l.tolist())]
                    if has_extra or self.__dict__.get("_step_log") is not None:
                        # a model's further term and its logged value are sums over the shard's rows too: each rank's own
                        # share leaves the total, the sum over ranks enters it
                        # (a step that set neither left zeros: the columns are cleared after every epoch)
                        own = loss_log[:step_no, 2:4]
                        both = dp.all_reduce_sum(own.clone())
                        vals = [v - e + s for v, e, s in zip(vals, own[:, 1].tolist(), both[:, 1].tolist())]
                        loss_log[:step_no, 2].copy_(both[:, 0])
                else:
                    vals = total_l.tolist()
                for v in vals:
                    total_loss_epoch += v
            self._raise_on_bad_ids()          # deferred IndexError of the epoch's gathers (host is in sync here anyway)
            if hasattr(self.optim, "take_backlog"):
                # deferred table update: the L2 value of the steps a row was updated late for belongs to this epoch's sum
                self.optim.flush()
                total_loss_epoch += self.optim.take_backlog()
            epoch_logs["loss"] = total_loss_epoch / sample_num
            step_log = self.__dict__.get("_step_log")
            if step_log is not None and step_no:     # e.g. "sfg_loss": sum of the steps' values / sample_num (basemodel_sfg.py:365-366)
                extra_sum = 0.0
                for v in loss_log[:step_no, 2].tolist():
                    extra_sum += v
                epoch_logs[step_log[0]] = extra_sum / sample_num
            if loss_log is not None and step_no:
                loss_log[:step_no, 2:4].zero_()      # only steps that have such a value write it: the rest must read as zero
            for name, k in logged.items():
                vals = metric_log[:step_no, k].tolist()
                if name == "auc" and any(v != v for v in vals):
                    raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
                train_result[name] = vals
            for name, slot in native_logged.items():
                vals = native_log[:step_no, slot].tolist()
                if slot == 1 and any(v != v for v in vals):
                    raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
                train_result[name] = vals
            for name, (log, slot) in wlogged.items():             # K14w's rows, or K14's for a batch without weights
                vals = log[:step_no, slot].tolist()
                if slot == 1 and any(v != v for v in vals):
                    raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
                wresult[name] = vals
            for name in self.metrics:                             # History keys in the order `compile` was given
                if name in train_result:
                    epoch_logs[name] = np.sum(train_result[name]) / steps_per_epoch
            for name, fn in wm.items():
                if name not in wresult and w_all is None and fn in self._weighted_slots():
                    # unit weights, and the unweighted function is one of `self.metrics`: its values
                    twin = [k for k, f in self.metrics.items() if f is self._weighted_slots()[fn][1] and k in train_result]
                    if twin:
                        wresult[name] = train_result[twin[0]]
                if name in wresult:
                    epoch_logs[name] = np.sum(wresult[name]) / steps_per_epoch
            if do_validation:
                val_logs = self.evaluate(val_x, val_y, batch_size, sample_weight=val_w) if wm else self.evaluate(val_x, val_y, batch_size)
                for name, val in val_logs.items():
                    epoch_logs["val_" + name] = val
            if verbose > 0 and (dp is None or dp.rank == 0):
                msg = "{0}s - loss: {1: .4f}".format(int(time.time() - t_epoch), epoch_logs["loss"])
                if "sfg_loss" in epoch_logs:
                    msg += " - sfg_loss: {0: .4f}".format(epoch_logs["sfg_loss"])
                for name in list(self.metrics) + list(wm):
                    msg += " - " + name + ": {0: .4f}".format(epoch_logs[name])
                if do_validation:
                    for name in list(self.metrics) + list(wm):
                        msg += " - val_" + name + ": {0: .4f}".format(epoch_logs["val_" + name])
                print('Epoch {0}/{1}'.format(epoch + 1, epochs))
                print(msg)
            if dp is None or dp.rank == 0:
                cbs.on_epoch_end(epoch, epoch_logs)
            else:
                self.history.on_epoch_end(epoch, epoch_logs)
            if dp is not None:
                self.stop_training = dp.any_flag(self.stop_training)
            if self.stop_training:
                break
        cbs.on_train_end()
        return self.history

    def _log_weighted_step(self, yt, yp, wt, max_rows, steps_per_epoch, row, log, wlogged, wresult):
        """One step's `weighted_*` values of `fit` (labels yt, predictions yp, weights wt of the global batch; wt None: unit
        weights).  On a GPU with fp32 tensors every wired entry comes from ONE ops.eval_metrics_w call (K14w) into row `row`
        of the float64 log, read once per epoch -- for a batch without weights from ops.batch_metrics (K14), whose values are
        the unweighted ones, unless the unweighted function is logged anyway (`fit` takes those values at the epoch's end).
        Everything else: the numpy functions on host copies, appended to wresult[name].  Returns the log; wlogged[name] =
        (log, slot) for what it holds."""
        wtable = self._weighted_slots()
        y1, p1 = yt.reshape(-1), yp.reshape(-1)
        native = {}
        if wt is not None:
            w1 = wt.reshape(-1)
            if ops.EVAL_W_NATIVE and ops.eval_metrics_w_supported(y1, p1, w1):
                native = {name: wtable[fn][0] for name, fn in self.weighted_metrics.items() if fn in wtable}
        elif ops.METRICS_NATIVE and max_rows <= ops.METRICS_MAX_ROWS and ops.batch_metrics_supported(yt, yp):
            native = {name: wtable[fn][0] for name, fn in self.weighted_metrics.items()
                      if fn in wtable and wtable[fn][1] not in self.metrics.values()}
        if native:
            if log is None or log.device != yt.device:
                log = torch.empty((steps_per_epoch + 1, 4), dtype=torch.float64, device=yt.device)
            which = sum({1 << s for s in native.values()})
            if wt is not None:
                ops.eval_metrics_w(y1, p1, w1, which, log[row])
            else:
                ops.batch_metrics(yt, yp, which, log[row])
            wlogged.update({name: (log, slot) for name, slot in native.items()})
        host = None
        for name, fn in self.weighted_metrics.items():
            if name in native or (wt is None and fn in wtable and wtable[fn][1] in self.metrics.values()):
                continue
            if host is None:
                host = (yt.cpu().data.numpy(), yp.cpu().data.numpy().astype("float64"),
                        None if wt is None else wt.cpu().data.numpy())
            if wt is None and fn in wtable:
                wresult.setdefault(name, []).append(wtable[fn][1](host[0], host[1]))
            else:
                wresult.setdefault(name, []).append(fn(host[0], host[1], np.ones(host[0].size, np.float32) if wt is None else host[2]))
        return log

    def _eval_native_plan(self, y):
        """(float32 labels [N], {metrics key: slot of xdfm_eval_metrics' out4}) when `evaluate` may take K14s for these labels,
        else None: the switch ops.EVAL_NATIVE on, the model on a GPU, numeric labels that survive the round trip through
        float32 unchanged, and at least one entry of `self.metrics` still the function `_get_metrics` wired in."""
        table = self._wired_slots()
        slots = {name: table[fn] for name, fn in self.metrics.items() if fn in table}
        y32 = self._eval_native_labels(y) if ops.EVAL_NATIVE and slots else None
        return None if y32 is None else (y32, slots)

    def _eval_native_labels(self, y):
        """The labels as float32 [N] when K14s / K14w may take them (the model on a GPU, numeric labels that survive the round
        trip through float32 unchanged, a row count within the kernels' cap), else None."""
        if torch.device(self.device).type != "cuda":
            return None
        ya = np.asarray(y)
        if ya.dtype.kind not in "buif" or not 1 <= ya.size <= ops.EVAL_MAX_ROWS:
            return None
        y32 = np.ascontiguousarray(ya.reshape(-1), dtype=np.float32)
        if not np.array_equal(y32.astype(ya.dtype), ya.reshape(-1)):          # soft float64 labels, a NaN: the host's arithmetic
            return None
        return y32

    def evaluate(self, x, y, batch_size=256, sample_weight=None):
        """{metrics key: value} of the predictions for x against y.  With a plan from `_eval_native_plan` the predictions stay
        on the device, the labels go there once and ONE ops.eval_metrics call (K14s) with one host read serves every wired
        entry; a callable the user put into `self.metrics` still gets host arrays, the predictions copied once for them.
        Otherwise: the numpy functions on `predict`'s output.
        A model compiled with `weighted_metrics` returns those entries after the unweighted ones (`_evaluate_weighted`);
        `sample_weight` (one finite weight >= 0 per row; None: unit weights) is refused on any other model."""
        if getattr(self, "weighted_metrics", None):
            return self._evaluate_weighted(x, y, batch_size, sample_weight)
        if sample_weight is not None:
            raise ValueError("evaluate(sample_weight=...) needs a model compiled with weighted_metrics: no entry of this "
                             "model would use the weights")
        plan = self._eval_native_plan(y)
        if plan is None:
            pred = self.predict(x, batch_size)
            return {name: fn(y, pred) for name, fn in self.metrics.items()}
        y32, slots = plan
        dev = self._predict_device(x, batch_size)
        if dev is None or dev.numel() != y32.size or dev.dtype != torch.float32:       # not one label per row
            pred = self._predictions_to_host(dev)
            return {name: fn(y, pred) for name, fn in self.metrics.items()}
        vals = ops.eval_metrics(torch.from_numpy(y32).to(dev.device), dev.reshape(-1),
                                sum(1 << s for s in set(slots.values()))).tolist()      # the one host read
        self._raise_on_bad_ids()
        n_pos = int((y32 > 0.5).sum())
        if 1 in slots.values() and vals[1] != vals[1] and n_pos in (0, y32.size):
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        pred = self._predictions_to_host(dev) if len(slots) < len(self.metrics) else None
        return {name: vals[slots[name]] if name in slots else fn(y, pred) for name, fn in self.metrics.items()}

    def _evaluate_weighted(self, x, y, batch_size, sample_weight):
        """`evaluate` of a model compiled with `weighted_metrics`: the unweighted entries as `evaluate` computes them (K14s when
        its conditions hold, else the host), then the `weighted_*` entries.  With weights and ops.EVAL_W_NATIVE, on the
        conditions of the native route, the weights go to the device once and ONE ops.eval_metrics_w call (K14w) serves every
        wired weighted entry; both calls' values come back in one host read.  Without weights (unit weights) a wired weighted
        entry is the value of its unweighted function, taken from the same computation.  Otherwise: metrics.py's weighted
        numpy functions on the host copy of the predictions."""
        w = example_weights(y, sample_weight, None, getattr(self.out, "task", None))
        table, wtable = self._wired_slots(), self._weighted_slots()
        unit = {name: wtable[fn][1] for name, fn in self.weighted_metrics.items() if w is None and fn in wtable}
        y32 = self._eval_native_labels(y)
        dev = self._predict_device(x, batch_size)
        on_dev = y32 is not None and dev is not None and dev.numel() == y32.size and dev.dtype == torch.float32
        u_slots, a_slots, w_slots = {}, {}, {}
        if on_dev and ops.EVAL_NATIVE:
            u_slots = {name: table[fn] for name, fn in self.metrics.items() if fn in table}
            a_slots = {name: table[fn] for name, fn in unit.items()}
        if on_dev and ops.EVAL_W_NATIVE and w is not None:
            w_slots = {name: wtable[fn][0] for name, fn in self.weighted_metrics.items() if fn in wtable}
        uvals = wvals = None
        if u_slots or a_slots or w_slots:
            yd, pd, parts = torch.from_numpy(y32).to(dev.device), dev.reshape(-1), []
            if u_slots or a_slots:
                parts.append(ops.eval_metrics(yd, pd, sum(1 << s for s in set(u_slots.values()) | set(a_slots.values()))))
            if w_slots:
                parts.append(ops.eval_metrics_w(yd, pd, torch.from_numpy(w).to(dev.device), sum(1 << s for s in set(w_slots.values()))))
            vals = torch.cat(parts).tolist()                                            # the one host read
            uvals, wvals = (vals[:4] if u_slots or a_slots else None), (vals[-4:] if w_slots else None)
            self._raise_on_bad_ids()
            one_class = ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
            pos = y32 > 0.5
            if uvals is not None and 1 in set(u_slots.values()) | set(a_slots.values()) and uvals[1] != uvals[1] \
                    and int(pos.sum()) in (0, y32.size):
                raise one_class
            if wvals is not None and 1 in w_slots.values() and wvals[1] != wvals[1] \
                    and float(w[pos].sum(dtype=np.float64)) * float(w[~pos].sum(dtype=np.float64)) == 0:
                raise one_class
        served = set(u_slots) | set(a_slots) | set(w_slots)
        pred = self._predictions_to_host(dev) if len(served) < len(self.metrics) + len(self.weighted_metrics) else None
        out, by_fn = {}, {}
        for name, fn in self.metrics.items():
            out[name] = by_fn[fn] = uvals[u_slots[name]] if name in u_slots else fn(y, pred)
        for name, fn in self.weighted_metrics.items():
            if name in w_slots:
                out[name] = wvals[w_slots[name]]
            elif name in a_slots:
                out[name] = uvals[a_slots[name]]
            elif name in unit:
                out[name] = by_fn[unit[name]] if unit[name] in by_fn else unit[name](y, pred)
            else:
                out[name] = fn(y, pred, np.ones(len(pred), np.float32) if w is None else w)
        return out

    def _predict_device(self, x, batch_size):
        """The batch loop of `predict`: the fp32 predictions for every row of x on the model's device, one per row in the
        model's output shape ([N, 1]); None without rows."""
        self.eval()
        X_all, _ = self._resident(x)
        chunks = []
        with torch.no_grad():
            for start in range(0, X_all.shape[0], batch_size):
                chunks.append(self(X_all[start:start + batch_size].to(self.device)))
        return torch.cat(chunks) if chunks else None

    def _predictions_to_host(self, dev):
        """What `predict` returns for the loop's output: float64 on the host, after the deferred id check."""
        if dev is None:
            return np.zeros((0, 1), dtype="float64")
        out = dev.cpu().data.numpy().astype("float64")      # one device-to-host copy
        self._raise_on_bad_ids()
        return out

    def predict(self, x, batch_size=256):
        """float64 [N, 1] predictions (basemodel.py:325-352)."""
        return self._predictions_to_host(self._predict_device(x, batch_size))


# ------------------------------------------------------------------------------------------------- #
class _XDeepFMBase(BaseModel):
    """Shared wiring of the three variants (deepctr/models/xdeepfm.py:42-107)."""

    def _build_dnn(self, dnn_feature_columns, dnn_hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, dnn_use_bn,
                   init_std, device):
        self.dnn_hidden_units = dnn_hidden_units
        self.use_dnn = len(dnn_feature_columns) > 0 and len(dnn_hidden_units) > 0
        if self.use_dnn:
            self.dnn = DNN(self.compute_input_dim(dnn_feature_columns), dnn_hidden_units, activation=dnn_activation,
                           l2_reg=l2_reg_dnn, dropout_rate=dnn_dropout, use_bn=dnn_use_bn, init_std=init_std,
                           device=device)
            self.dnn_linear = nn.Linear(dnn_hidden_units[-1], 1, bias=False).to(device)
            self.add_regularization_weight(
                filter(lambda x: 'weight' in x[0] and 'bn' not in x[0], self.dnn.named_parameters()), l2=l2_reg_dnn)
            self.add_regularization_weight(self.dnn_linear.weight, l2=l2_reg_dnn)

    def _finish_cin(self, cin_out_dim, l2_reg_cin, device):
        self.cin_linear = nn.Linear(cin_out_dim, 1, bias=False).to(device)
        self.add_regularization_weight(filter(lambda x: 'weight' in x[0], self.cin.named_parameters()), l2=l2_reg_cin)

    def head_inputs(self, X):
        """(linear logit [B,1], CIN output [B, featuremap_num] or None, DNN output [B, hidden] or None): what the
        last stage (cin_linear, dnn_linear, sum, PredictionLayer; deepctr/models/xdeepfm.py:95-107) consumes."""
        emb_fm, dnn_in, logit = self.fused_inputs(X)
        B = X.shape[0]
        cin_out = self.cin.forward_fm(emb_fm, B, self._plan.D) if self.use_cin else None
        dnn_out = self.dnn(dnn_in) if self.use_dnn else None
        return logit, cin_out, dnn_out

    def forward(self, X):
        logit, cin_out, dnn_out = self.head_inputs(X)
        if cin_out is not None:
            logit = logit + self.cin_linear(cin_out)
        if dnn_out is not None:
            logit = logit + self.dnn_linear(dnn_out)
        return self.out(logit)


class xDeepFM(_XDeepFMBase):
    """xDeepFM (deepctr/models/xdeepfm.py:17-107)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 256),
                 cin_layer_size=(256, 128,), cin_split_half=True, cin_activation='relu', l2_reg_linear=0.00001,
                 l2_reg_embedding=0.00001, l2_reg_dnn=0, l2_reg_cin=0, init_std=0.0001, seed=1024, dnn_dropout=0,
                 dnn_activation='relu', dnn_use_bn=False, task='binary', device='cpu', gpus=None):
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                         l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task, device=device,
                         gpus=gpus)
        self._build_dnn(dnn_feature_columns, dnn_hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, dnn_use_bn,
                        init_std, device)
        self.cin_layer_size = cin_layer_size
        self.use_cin = len(cin_layer_size) > 0 and len(dnn_feature_columns) > 0
        if self.use_cin:
            self.featuremap_num = (sum(cin_layer_size[:-1]) // 2 + cin_layer_size[-1]) if cin_split_half \
                else sum(cin_layer_size)
            self.cin = CIN(len(self.embedding_dict), cin_layer_size, cin_activation, cin_split_half, l2_reg_cin, seed,
                           device=device)
            self._finish_cin(self.featuremap_num, l2_reg_cin, device)
        self.to(device)


class xDeepFMAttention(_XDeepFMBase):
    """xDeepFM whose CIN ends in attention pooling (deepctr/models/xdeepfm_attn.py:25-173)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 256),
                 cin_layer_size=(256, 128,), cin_split_half=True, cin_activation='relu', cin_num_heads=4,
                 cin_attn_dropout=0.0, cin_use_layer_norm=True, cin_use_residual=True, l2_reg_linear=0.00001,
                 l2_reg_embedding=0.00001, l2_reg_dnn=0, l2_reg_cin=0, init_std=0.0001, seed=1024, dnn_dropout=0,
                 dnn_activation='relu', dnn_use_bn=False, task='binary', device='cpu', gpus=None):
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                         l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task, device=device,
                         gpus=gpus)
        self._build_dnn(dnn_feature_columns, dnn_hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, dnn_use_bn,
                        init_std, device)
        self.cin_layer_size = cin_layer_size
        self.use_cin = len(cin_layer_size) > 0 and len(dnn_feature_columns) > 0
        if self.use_cin:
            emb = next(fc.embedding_dim for fc in dnn_feature_columns if isinstance(fc, SparseFeat))
            self.featuremap_num = (sum(cin_layer_size[:-1]) // 2 + cin_layer_size[-1]) if cin_split_half \
                else sum(cin_layer_size)
            self.cin = CINAttention(field_size=len(self.embedding_dict), embedding_size=emb,
                                    layer_size=cin_layer_size, activation=cin_activation, split_half=cin_split_half,
                                    num_heads=cin_num_heads, attn_dropout=cin_attn_dropout,
                                    use_layer_norm=cin_use_layer_norm, use_residual=cin_use_residual,
                                    l2_reg=l2_reg_cin, seed=seed, device=device)
            self._finish_cin(self.featuremap_num, l2_reg_cin, device)
        self.to(device)


class xDeepFMAttentionV2(_XDeepFMBase):
    """Variant without the output projection: the CIN block returns [B, D]
    (deepctr/models/xdeepfm_attn.py:176-301)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 256),
                 cin_layer_size=(256, 128,), cin_split_half=True, cin_activation='relu', cin_num_heads=4,
                 cin_attn_dropout=0.0, cin_use_layer_norm=True, cin_use_residual=True, cin_num_attn_layers=1,
                 l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0, l2_reg_cin=0, init_std=0.0001,
                 seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task='binary', device='cpu',
                 gpus=None):
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                         l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task, device=device,
                         gpus=gpus)
        self._build_dnn(dnn_feature_columns, dnn_hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, dnn_use_bn,
                        init_std, device)
        self.cin_layer_size = cin_layer_size
        self.use_cin = len(cin_layer_size) > 0 and len(dnn_feature_columns) > 0
        if self.use_cin:
            emb = next(fc.embedding_dim for fc in dnn_feature_columns if isinstance(fc, SparseFeat))
            self.cin = CINAttentionV2(field_size=len(self.embedding_dict), embedding_size=emb,
                                      layer_size=cin_layer_size, activation=cin_activation,
                                      split_half=cin_split_half, num_heads=cin_num_heads,
                                      attn_dropout=cin_attn_dropout, use_layer_norm=cin_use_layer_norm,
                                      use_residual=cin_use_residual, num_attn_layers=cin_num_attn_layers,
                                      l2_reg=l2_reg_cin, seed=seed, device=device)
            self._finish_cin(emb, l2_reg_cin, device)
        self.to(device)
