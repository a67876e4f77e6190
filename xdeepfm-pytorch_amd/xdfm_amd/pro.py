"""xDeepFM "Pro": xDeepFM + Supervised Feature Generation (SFG) decoder + optional AutoDis, behind the interface of
deepctr/xdeepfm_pro (reference files cited per class).  Same constructor signatures, module structure and
state_dict keys as the reference, so `.pth` files interchange and `xdftrain_pro.py`'s flow runs unchanged.

What runs where:
  * embeddings / linear logit / DNN input: the fused gather K1; CIN: the MFMA kernels K3 / K4 -- exactly as xDeepFM;
  * the SFG decoder's input IS K1's `dnn_in` output ([sparse embeddings field-major | dense values],
    sfg_decoder.py:113-136), so the decoder costs no extra gather;
  * the 26 vocabulary-wide softmax heads + masked cross-entropy (sfg_decoder.py:146-149, :277-293) never materialise
    the [B, V_f] logits: `ops.VocabSoftmaxCE` walks the vocabulary in tiles with an online log-sum-exp and recomputes the
    tiles in the backward; with `sfg_positive_only` (the default) only the rows with label 1 enter the decoder at all --
    masked rows contribute exact zeros to loss and gradients in the reference too (`ce_loss * positive_mask`).  The tile
    GEMMs are library GEMMs (hipBLASLt through torch); a hand-written MFMA kernel for them is the next step;
  * AutoDis runs in one fused launch forward and one (+ a fixed-order finish) backward for all dense fields
    (`ops.AutoDis`, csrc/autodis.hip) on float32 GPU tensors with K <= 32 buckets and D <= 64; outside that envelope, on
    the CPU or with XDFM_AUTODIS_NATIVE=0 it is the reference's per-field loop on torch ops;
  * the decoder MLP and LabelAwareAttention are small dense layers on torch ops.
The SFG branch has two routes (`BaseModelSFG.compute_sfg_loss_fused`).  The static route (XDFM_PRO_GRAPH=1, a GPU model whose heads the
fused kernels serve): K11 (`ops.compact_rows`, csrc/compact.hip) moves the positive rows to the front of
tensors that keep the batch's capacity and leaves their number on the device, the decoder runs on the capacity rows and the
heads' kernels take the count from the device -- every shape depends on the batch shape only, so the train step is captured
and replayed like every other model's (xdfm_amd/graphstep.py).  The dynamic route (the default, and everything else) selects the
rows with torch.nonzero, whose shape reaches the host: that step launches eagerly.
Row-parallel training (xdfm_amd/dist.py): every rank runs the branch on the positive rows of its shard and divides by the
number of positives of the GLOBAL batch (`BaseModelSFG.sfg_norm_labels`), so the ranks' terms and gradients add up to those
of one process on the global batch.
"""
import os
import warnings
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dist as xdist
from . import ops
from .inputs import DenseFeat, SparseFeat
from .layers import CIN, DNN
from .models import BaseModel


def pro_graph_enabled() -> bool:
    """XDFM_PRO_GRAPH (default 0): 1 puts the SFG branch on the static route, whose train step is captured and replayed;
    unset, empty or 0 keeps the dynamic route (torch.nonzero; eager launches)."""
    return os.environ.get("XDFM_PRO_GRAPH", "0").strip() not in ("", "0")


# ------------------------------------------------------------------------------------------------- #
class LabelAwareAttention(nn.Module):
    """sigmoid gate from [input | label embedding] (deepctr/xdeepfm_pro/sfg_decoder.py:160-206)."""

    def __init__(self, input_dim: int, hidden_dim: int = 64, device: str = 'cpu'):
        super().__init__()
        self.label_embedding = nn.Embedding(2, hidden_dim)
        self.attention_net = nn.Sequential(nn.Linear(input_dim + hidden_dim, hidden_dim), nn.ReLU(),
                                           nn.Linear(hidden_dim, input_dim), nn.Sigmoid())
        self.to(device)

    def forward(self, x: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        if len(labels.shape) > 1:
            labels = labels.squeeze(-1)
        label_emb = self.label_embedding(labels.long())
        return self.attention_net(torch.cat([x, label_emb], dim=-1))

    def forward_native(self, x: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """forward's value on `ops.dense` / `ops.dense_relu` (their bias gradients are the library's column sums: no memset
        node in a captured step).  The embedding lookup of a 0 / 1 label is the product [1 - l, l] . E: exact, and its
        backward is a GEMM instead of an index scatter."""
        l = labels.reshape(-1).to(x.dtype).trunc()
        label_emb = ops.dense(torch.stack([1.0 - l, l], dim=1), self.label_embedding.weight.t(), None)
        net = self.attention_net
        gate = ops.dense_relu(torch.cat([x, label_emb], dim=-1), net[0].weight, net[0].bias)
        return torch.sigmoid(ops.dense(gate, net[2].weight, net[2].bias))


class SFGDecoder(nn.Module):
    """MLP decoder with one vocabulary-wide head per sparse field and one regression head for the dense fields
    (deepctr/xdeepfm_pro/sfg_decoder.py:19-157)."""

    def __init__(self, embedding_dim: int, sparse_feature_dims: Dict[str, int], dense_feature_names: List[str],
                 hidden_units: Tuple[int, ...] = (128, 64), dropout_rate: float = 0.1,
                 use_label_aware_attention: bool = True, device: str = 'cpu'):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.sparse_feature_dims = sparse_feature_dims
        self.dense_feature_names = dense_feature_names
        self.use_label_aware_attention = use_label_aware_attention
        self.device = device
        self.num_sparse_features = len(sparse_feature_dims)
        self.num_dense_features = len(dense_feature_names)
        input_dim = self.num_sparse_features * embedding_dim + self.num_dense_features
        layers, prev_dim = [], input_dim
        for hidden_dim in hidden_units:
            layers += [nn.Linear(prev_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout_rate)]
            prev_dim = hidden_dim
        self.shared_layers = nn.Sequential(*layers)
        self.sparse_heads = nn.ModuleDict()
        for feat_name, vocab_size in sparse_feature_dims.items():
            self.sparse_heads[feat_name] = nn.Linear(prev_dim, vocab_size)
        self.dense_head = nn.Linear(prev_dim, self.num_dense_features) if self.num_dense_features > 0 else None
        if use_label_aware_attention:
            self.label_attention = LabelAwareAttention(input_dim=input_dim,
                                                       hidden_dim=hidden_units[0] if hidden_units else 64, device=device)
        self.to(device)

    def hidden(self, decoder_input: torch.Tensor, labels: Optional[torch.Tensor]) -> torch.Tensor:
        """decoder input [rows, m*D + nd] -> last hidden layer (sfg_decoder.py:138-143)."""
        if self.use_label_aware_attention and labels is not None:
            decoder_input = decoder_input * self.label_attention(decoder_input, labels)
        return self.shared_layers(decoder_input)

    def hidden_native(self, decoder_input: torch.Tensor, labels: Optional[torch.Tensor]) -> torch.Tensor:
        """`hidden` with every nn.Linear routed through `ops.dense` / `ops.dense_relu` (same modules, same values)."""
        if self.use_label_aware_attention and labels is not None:
            decoder_input = decoder_input * self.label_attention.forward_native(decoder_input, labels)
        x = decoder_input
        mods = list(self.shared_layers)                             # (nn.Linear, nn.ReLU, nn.Dropout) per hidden layer
        seed = None                                                 # one per call, shared by the layers through their index
        for i in range(len(mods) // 3):
            lin, _, drop = mods[3 * i:3 * i + 3]
            x, seed = ops.dense_relu_then_dropout(x, lin.weight, lin.bias, drop, drop.training, seed, i)
        if seed is not None:
            self.last_drop_seed = seed
        return x

    last_drop_seed = None        # the seed of the last hidden_native call that ran the native dropout (read by the tests)

    def forward(self, sparse_embeddings, dense_values, labels=None):
        """The reference's signature (lists of [B,1,D] / [B,1] tensors) -> (dict of [B, V_f] logits, [B, nd]).  This
        materialises the logits and exists for API compatibility; the models' loss goes through `hidden` + the tiled
        cross-entropy instead."""
        sparse_concat = torch.cat([e.squeeze(1) if len(e.shape) == 3 else e for e in sparse_embeddings], dim=-1)
        dense_concat = torch.cat(dense_values, dim=-1) if len(dense_values) > 0 else \
            torch.zeros(sparse_concat.shape[0], 0, device=sparse_concat.device)
        hidden = self.hidden(torch.cat([sparse_concat, dense_concat], dim=-1), labels)
        sparse_logits = {name: self.sparse_heads[name](hidden) for name in self.sparse_feature_dims.keys()}
        dense_preds = self.dense_head(hidden) if self.dense_head is not None else \
            torch.zeros(hidden.shape[0], 0, device=hidden.device)
        return sparse_logits, dense_preds


class SFGLoss(nn.Module):
    """Masked reconstruction loss: cross-entropy per sparse field + MSE over the dense fields, summed over the
    positive rows and divided by their number (deepctr/xdeepfm_pro/sfg_decoder.py:209-311)."""

    def __init__(self, sparse_feature_names: List[str], dense_feature_names: List[str], sparse_weight: float = 1.0,
                 dense_weight: float = 1.0, positive_only: bool = True, label_smooth: float = 0.0, device: str = 'cpu'):
        super().__init__()
        self.sparse_feature_names = sparse_feature_names
        self.dense_feature_names = dense_feature_names
        self.sparse_weight, self.dense_weight = sparse_weight, dense_weight
        self.positive_only = positive_only
        self.label_smooth = label_smooth
        self.device = device

    def forward(self, sparse_logits, dense_preds, sparse_targets, dense_targets, labels):
        if len(labels.shape) > 1:
            labels = labels.squeeze(-1)
        if self.positive_only:
            positive_mask = (labels == 1).float()
            num_positive = positive_mask.sum() + 1e-8
        else:
            positive_mask = torch.ones_like(labels).float()
            num_positive = labels.shape[0]
        loss_dict = {}
        total_sparse = torch.zeros((), device=labels.device)
        total_dense = torch.zeros((), device=labels.device)
        for name in self.sparse_feature_names:
            if name in sparse_logits and name in sparse_targets:
                targets = sparse_targets[name].long()
                if len(targets.shape) > 1:
                    targets = targets.squeeze(-1)
                ce = F.cross_entropy(sparse_logits[name], targets, reduction='none')
                masked = (ce * positive_mask).sum() / num_positive
                total_sparse = total_sparse + masked
                loss_dict['sfg_sparse_%s' % name] = masked
        if len(self.dense_feature_names) > 0 and dense_preds.shape[1] > 0:
            mse = F.mse_loss(dense_preds, dense_targets, reduction='none').mean(dim=-1)
            total_dense = (mse * positive_mask).sum() / num_positive
            loss_dict['sfg_dense'] = total_dense
        total = self.sparse_weight * total_sparse + self.dense_weight * total_dense
        loss_dict['sfg_total'] = total
        return total, loss_dict


class _ZeroLoss(torch.autograd.Function):
    """A zero that depends on `params`: its backward hands each of them an exact zero gradient."""

    @staticmethod
    def forward(ctx, *params):
        ctx.save_for_backward(*params)
        return torch.zeros((), dtype=params[0].dtype, device=params[0].device)

    @staticmethod
    def backward(ctx, g):
        return tuple(torch.zeros_like(p) for p in ctx.saved_tensors)


# ------------------------------------------------------------------------------------------------- #
class AutoDisLayer(nn.Module):
    """Soft discretisation of dense features into bucket-embedding mixtures (deepctr/xdeepfm_pro/autodis.py:20-149)."""

    def __init__(self, num_features: int, num_buckets: int = 16, embedding_dim: int = 8, temperature: float = 1.0,
                 keep_raw: bool = True, device: str = 'cpu'):
        super().__init__()
        self.num_features, self.num_buckets, self.embedding_dim = num_features, num_buckets, embedding_dim
        self.temperature, self.keep_raw, self.device = temperature, keep_raw, device
        if num_features > 0:
            self.meta_embeddings = nn.Parameter(torch.randn(num_features, num_buckets, embedding_dim) * 0.01)
            self.bucket_projectors = nn.ModuleList([
                nn.Sequential(nn.Linear(1, num_buckets), nn.LeakyReLU(0.2), nn.Linear(num_buckets, num_buckets))
                for _ in range(num_features)])
            self.feature_temperatures = nn.Parameter(torch.ones(num_features) * temperature)
        self._native_cache = {}            # device pointer table of the projectors (ops.autodis)
        self.to(device)

    def forward(self, dense_values: List[torch.Tensor]):
        if self.num_features == 0 or len(dense_values) == 0:
            batch_size = dense_values[0].shape[0] if dense_values else 1
            return torch.zeros(batch_size, 0, device=self.device), []
        batch_size = dense_values[0].shape[0]
        if self._native(dense_values):
            return self.forward_native(torch.cat([v.reshape(batch_size, 1) for v in dense_values], dim=-1))
        dense_embeddings = []
        for i, dense_val in enumerate(dense_values):
            if len(dense_val.shape) == 1:
                dense_val = dense_val.unsqueeze(-1)
            scores = self.bucket_projectors[i](dense_val)
            weights = F.softmax(scores / self.feature_temperatures[i], dim=-1)
            dense_embeddings.append(torch.matmul(weights, self.meta_embeddings[i]).unsqueeze(1))
        return torch.cat(dense_embeddings, dim=1).view(batch_size, -1), dense_embeddings

    def _native(self, dense_values) -> bool:
        """The fused kernels (ops.AutoDis) serve float32 GPU tensors inside ops.autodis_supported's envelope unless
        XDFM_AUTODIS_NATIVE=0; everything else keeps the per-field loop below."""
        if os.environ.get("XDFM_AUTODIS_NATIVE", "1") == "0":
            return False
        if torch.is_tensor(dense_values):
            tensors = [dense_values]
            if dense_values.dim() != 2 or dense_values.shape[1] != self.num_features:
                return False
        else:
            tensors = list(dense_values)
            if len(tensors) != self.num_features or any(t.numel() != tensors[0].shape[0] for t in tensors):
                return False
        tensors += [self.meta_embeddings, self.feature_temperatures] + list(self.bucket_projectors.parameters())
        if not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
            return False
        return ops.autodis_supported(self.num_buckets, self.embedding_dim)

    def forward_native(self, x: torch.Tensor):
        """forward's result from the dense values as ONE [B, F] tensor (any row stride: a column slice of a wider matrix
        is read in place): one launch for all fields; the list entries are views of the flat output."""
        proj = [t for seq in self.bucket_projectors for t in (seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias)]
        flat = ops.autodis(x, self.meta_embeddings, proj, self.feature_temperatures, self._native_cache)
        D = self.embedding_dim
        return flat, [flat[:, i * D:(i + 1) * D].unsqueeze(1) for i in range(self.num_features)]

    def get_bucket_indices(self, dense_values: List[torch.Tensor]) -> List[torch.Tensor]:
        out = []
        for i, dense_val in enumerate(dense_values):
            if len(dense_val.shape) == 1:
                dense_val = dense_val.unsqueeze(-1)
            out.append(self.bucket_projectors[i](dense_val).argmax(dim=-1))
        return out


class DenseFeatureEncoder(nn.Module):
    """AutoDis or raw values behind one interface (deepctr/xdeepfm_pro/autodis.py:152-238)."""

    def __init__(self, dense_feature_names: List[str], embedding_dim: int = 8, use_autodis: bool = True,
                 num_buckets: int = 16, temperature: float = 1.0, device: str = 'cpu'):
        super().__init__()
        self.dense_feature_names = dense_feature_names
        self.embedding_dim, self.use_autodis = embedding_dim, use_autodis
        self.num_features = len(dense_feature_names)
        self.device = device
        self.autodis = AutoDisLayer(self.num_features, num_buckets, embedding_dim, temperature, device=device) \
            if use_autodis and self.num_features > 0 else None
        self.to(device)

    def forward(self, dense_values: List[torch.Tensor]):
        if self.num_features == 0 or len(dense_values) == 0:
            batch_size = dense_values[0].shape[0] if dense_values else 1
            z = torch.zeros(batch_size, 0, device=self.device)
            return z, [], z
        raw_values = torch.cat(dense_values, dim=-1)
        if self.use_autodis and self.autodis is not None:
            flat, emb_list = self.autodis(dense_values)
            return flat, emb_list, raw_values
        return raw_values, [dv.unsqueeze(-1) for dv in dense_values], raw_values

    def get_output_dim(self) -> int:
        return self.num_features * self.embedding_dim if self.use_autodis else self.num_features


# ------------------------------------------------------------------------------------------------- #
class BaseModelSFG(BaseModel):
    _VARLEN = False     # the SFG decoder and AutoDis are built on one id per field
    """BaseModel + SFG decoder / loss and the `sfg_loss` History entry (deepctr/xdeepfm_pro/basemodel_sfg.py:96-476).
    The training loop is BaseModel.fit: the step adds `sfg_weight * sfg_loss` to the total (basemodel_sfg.py:343) and
    the epoch logs gain `sfg_loss` = sum of the steps' values / sample_num (:365-366)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, l2_reg_linear=1e-5, l2_reg_embedding=1e-5,
                 init_std=0.0001, seed=1024, task='binary', device='cpu', gpus=None, use_sfg=True, sfg_weight=0.1,
                 sfg_hidden_units=(128, 64), sfg_dropout=0.1, sfg_positive_only=True, sfg_use_label_attention=True):
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                         l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task, device=device,
                         gpus=gpus)
        self.use_sfg = use_sfg
        self.sfg_weight = sfg_weight
        self.sfg_positive_only = sfg_positive_only
        self.sfg_loss = torch.zeros((1,), device=device)
        self.sparse_feature_columns = [fc for fc in dnn_feature_columns if isinstance(fc, SparseFeat)] \
            if dnn_feature_columns else []
        self.dense_feature_columns = [fc for fc in dnn_feature_columns if isinstance(fc, DenseFeat)] \
            if dnn_feature_columns else []
        self.embedding_dim = self.sparse_feature_columns[0].embedding_dim if self.sparse_feature_columns else 8
        if use_sfg:
            dense_names = [fc.name for fc in self.dense_feature_columns]
            self.sfg_decoder = SFGDecoder(
                embedding_dim=self.embedding_dim,
                sparse_feature_dims={fc.name: fc.vocabulary_size for fc in self.sparse_feature_columns},
                dense_feature_names=dense_names, hidden_units=sfg_hidden_units, dropout_rate=sfg_dropout,
                use_label_aware_attention=sfg_use_label_attention, device=device)
            self.sfg_loss_fn = SFGLoss([fc.name for fc in self.sparse_feature_columns], dense_names,
                                       positive_only=sfg_positive_only, device=device)
        else:
            self.sfg_decoder = None
            self.sfg_loss_fn = None
        self.to(device)

    def compile(self, optimizer, loss=None, metrics=None, weighted_metrics=None):
        if weighted_metrics:
            # the weights such metrics would follow are refused by train_on_batch below, for the reason given there
            raise NotImplementedError("weighted_metrics are not supported by %s: its SFG term is normalised on its own; "
                                      "train it without example weights" % type(self).__name__)
        super().compile(optimizer, loss, metrics)
        if self.use_sfg:                                   # basemodel_sfg.py:588-590
            self.metrics_names.insert(1, "sfg_loss")
        if not (self.use_sfg and self._sfg_static()):
            self._optim_capturable = False                 # eager launches: the dynamic route's row selection is data dependent

    def forward_with_sfg(self, X, y=None):
        raise NotImplementedError("Subclass must implement forward_with_sfg")

    def forward(self, X):
        return self.forward_with_sfg(X, None)[0]

    # ------------------------------------------------------------------ the normaliser of the SFG loss
    # SFGLoss divides the summed losses of the selected rows by their number in the batch (sfg_decoder.py:262-268).  Under
    # row-parallel training "the batch" is the global one, of which a rank holds a shard: `sfg_norm_labels` is the one
    # place that says which labels define the step's normaliser, and both routes ask it.
    def _global_batch_labels(self, y):
        """BaseModel.fit hands over the labels of the global batch before it shards them."""
        if self.use_sfg:
            self.__dict__["_sfg_handed"] = y

    def _sfg_bind_normaliser(self, x, y):
        """Before a train step, outside any capture: fix the labels that define this step's normaliser.  A single process:
        None, i.e. the step's own labels.  Row-parallel: the labels `fit` handed over, or -- `train_on_batch` called
        directly -- as many ones and zeros as one all-reduce of (local positives, local rows) counts; a stand-in row
        (weight 0) counts for nothing.  They are kept in one buffer per global batch size, whose address a captured step
        reads again at every replay.  No buffer is ever released: a captured first half holds the address of its buffer,
        replays without running Python and is keyed on nothing that knows the buffer, so this dict is the buffer's only
        owner for as long as the model lives (`ops.VocabHeadsState` keeps its tables for the same reason).  One float per
        row of a global batch size the model has seen: 128 KB at 8 ranks of 4096 rows."""
        handed = self.__dict__.pop("_sfg_handed", None)
        dp = xdist.current()
        if dp is None or not self.use_sfg or not self.training:
            self.__dict__["_sfg_norm_y"] = None
            return
        if handed is None:
            lab = y.reshape(-1)
            rw = float(self.__dict__.get("_row_weight", 1.0))
            v = torch.stack([(lab == 1).sum().to(torch.float64) * rw, torch.tensor(lab.numel() * rw, dtype=torch.float64,
                                                                                   device=lab.device)]).to(dp.flag_device())
            n_pos, n_all = (int(round(c)) for c in dp.all_reduce_sum(v).tolist())
            handed = torch.zeros(max(n_all, 1), dtype=torch.float32)
            handed[:n_pos] = 1.0
        handed = handed.reshape(-1)
        bufs = self.__dict__.setdefault("_sfg_norm_bufs", {})
        key = (handed.numel(), x.device)
        buf = bufs.get(key)
        if buf is None:
            buf = bufs[key] = torch.empty(handed.numel(), dtype=torch.float32, device=x.device)
        buf.copy_(handed)
        self.__dict__["_sfg_norm_y"] = buf

    def sfg_norm_labels(self, labels):
        """The labels that define this step's normaliser: the step's own in a single process (and whenever nothing was
        bound), those of the global batch under row-parallel training."""
        norm_y = self.__dict__.get("_sfg_norm_y")
        return labels.reshape(-1) if norm_y is None else norm_y

    def sfg_normaliser(self, labels) -> float:
        """What the summed losses of the selected rows are divided by: (number of positives among `sfg_norm_labels`) + 1e-8,
        or the number of rows without `sfg_positive_only` (sfg_decoder.py:262-268).  Reads the count back to the host."""
        norm_y = self.sfg_norm_labels(labels)
        if self.sfg_positive_only:
            return int((norm_y == 1).sum()) + 1e-8
        return float(norm_y.numel())

    def _sfg_row_weight(self) -> float:
        """0 on a rank that holds only a stand-in row of a global batch with fewer rows than ranks (dist.RowParallel.shard):
        that row adds nothing to the SFG term either."""
        return float(self.__dict__.get("_row_weight", 1.0))

    def train_on_batch(self, x, y, sample_weight=None):
        if sample_weight is not None:
            # the SFG term has a normaliser of its own (the positives of the batch): what a weight means there is undecided
            raise NotImplementedError("sample_weight is not supported by %s: its SFG term is normalised on its own; "
                                      "train it without example weights" % type(self).__name__)
        self._sfg_bind_normaliser(x, y)
        try:
            return super().train_on_batch(x, y)
        finally:
            self.__dict__["_sfg_norm_y"] = None         # a loss computed by hand afterwards is normalised by its own labels

    # ------------------------------------------------------------------ SFG loss on the fused layouts
    def _sfg_static(self, X=None, dnn_in=None) -> bool:
        """True when the SFG branch takes the static route: XDFM_PRO_GRAPH is 1, the model (and the batch at hand) is
        float32 on a GPU, and the heads are of a width the fused kernels serve.  Everything else keeps the dynamic route."""
        if not pro_graph_enabled() or self.sfg_decoder is None or not self.sparse_feature_columns:
            return False
        heads = [self.sfg_decoder.sparse_heads[fc.name] for fc in self.sparse_feature_columns]
        tensors = [t for h in heads for t in (h.weight, h.bias)] + [t for t in (X, dnn_in) if t is not None]
        if not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
            return False
        if dnn_in is not None and (dnn_in.dim() != 2 or dnn_in.shape[0] > 65536 or
                                   dnn_in.shape[1] != len(heads) * self.embedding_dim + self._sfg_dense_width()):
            return False
        return ops.vocab_heads_ce_supported(heads[0].weight.shape[1])

    def _sfg_dense_width(self) -> int:
        return sum(b - a for a, b in (self.feature_index[fc.name] for fc in self.dense_feature_columns))

    def _sfg_loss_static(self, X, dnn_in, labels):
        """The static route: K11, the decoder on the capacity rows, K9 by the device-side count, per-field sums times
        inv_n (which K11 counts over `sfg_norm_labels` when those are not the step's own: no host read).  Rows behind the
        count are zero rows of the decoder input; their cross-entropies and hidden gradients are exact zeros (K9) and the
        dense head's squared error is weighted by `valid`, so they add nothing to the loss or to any gradient -- the
        values are those of the dynamic route."""
        dec, fn = self.sfg_decoder, self.sfg_loss_fn
        fcs = list(self.sparse_feature_columns)
        key = (X.device, tuple(self.feature_index[fc.name][0] for fc in fcs))
        hit = self.__dict__.get("_sfg_cols")
        if hit is None or hit[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("xdfm: first SFG step inside a graph capture -- run the step once eagerly before")
            hit = self.__dict__["_sfg_cols"] = (key, torch.tensor(key[1], dtype=torch.int32, device=X.device), ops.VocabHeadsState())
        _, cols, state = hit
        n_rows, inv_n, valid, d_rows, l_rows, targets = ops.compact_rows(X, dnn_in, labels, cols, fn.positive_only,
                                                                         count_y=self.__dict__.get("_sfg_norm_y"))
        hidden = dec.hidden_native(d_rows, l_rows)
        heads = [dec.sparse_heads[fc.name] for fc in fcs]
        ce_all = ops.vocab_heads_ce(hidden, targets, [h.weight for h in heads], [h.bias for h in heads], n_rows=n_rows,
                                    state=state if self.__dict__.get("_own_step") else None)
        per_field = ce_all.sum(dim=1) * inv_n
        loss_dict = {'sfg_sparse_%s' % fc.name: per_field[k] for k, fc in enumerate(fcs)}
        total_sparse = per_field.sum()
        total_dense = torch.zeros((), device=X.device)
        if dec.dense_head is not None:
            nd = self._sfg_dense_width()
            want = d_rows[:, d_rows.shape[1] - nd:].detach()        # the dense values of the selected rows, as K1 copied them
            err = ops.dense(hidden, dec.dense_head.weight, dec.dense_head.bias) - want
            total_dense = (((err * err).mean(dim=-1) * valid).sum() * inv_n).reshape(())
            loss_dict['sfg_dense'] = total_dense
        total = fn.sparse_weight * total_sparse + fn.dense_weight * total_dense
        loss_dict['sfg_total'] = total
        return total, {'sfg_loss': total, 'sfg_loss_dict': loss_dict}

    def compute_sfg_loss_fused(self, X, dnn_in, labels):
        """sfg loss from K1's `dnn_in` rows ([sparse embeddings | dense values] = the decoder input of
        sfg_decoder.py:113-136) -- arithmetic of compute_sfg_loss (basemodel_sfg.py:420-476) + SFGLoss, with the rows
        the mask zeroes left out and the vocabulary heads evaluated tile by tile."""
        if torch.is_grad_enabled() and not self.__dict__.get("_own_step"):
            # driven by hand (forward_with_sfg + a backward of the caller's): that backward binds the parameters' gradient
            # accumulators to the caller's stream -- the default stream, which must not take part in a capture -- for as
            # long as the caller keeps the loss alive (xdfm_amd/graphstep.py).  Such a model keeps eager launches.
            if getattr(self, "_optim_capturable", False):
                warnings.warn("xdfm: this %s was driven by hand (its SFG loss was computed with gradients outside "
                              "train_on_batch / fit); its train step launches eagerly from now on instead of being replayed "
                              "from a captured graph, until compile() is called again" % type(self).__name__)
            self._optim_capturable = False
        if self._sfg_static(X, dnn_in):
            return self._sfg_loss_static(X, dnn_in, labels)
        dec, fn = self.sfg_decoder, self.sfg_loss_fn
        lab = labels.reshape(-1)
        if fn.positive_only:
            rows = torch.nonzero(lab == 1).reshape(-1)      # host-visible shape: this step is not graph-captured
            num_positive = rows.numel() + 1e-8 if self.__dict__.get("_sfg_norm_y") is None else self.sfg_normaliser(lab)
            x_rows, d_rows, l_rows = X.index_select(0, rows), dnn_in.index_select(0, rows), lab.index_select(0, rows)
        else:
            x_rows, d_rows, l_rows, num_positive = X, dnn_in, lab, self.sfg_normaliser(lab)
        loss_dict = {}
        total_sparse = torch.zeros((), device=X.device)
        total_dense = torch.zeros((), device=X.device)
        if x_rows.shape[0] > 0:
            hidden = dec.hidden(d_rows, l_rows)
            fcs = list(self.sparse_feature_columns)
            if fcs and ops.vocab_heads_ce_supported(hidden.shape[1]):
                # all heads in one autograd node: the hidden rows are packed once, no logits in HBM (ops.VocabHeadsCE)
                cols = [self.feature_index[fc.name][0] for fc in fcs]
                targets = x_rows[:, cols].long().t().contiguous()
                heads = [dec.sparse_heads[fc.name] for fc in fcs]
                ce_all = ops.vocab_heads_ce(hidden, targets, [h.weight for h in heads], [h.bias for h in heads])
                per_field = ce_all.sum(dim=1) / num_positive
                for k, fc in enumerate(fcs):
                    total_sparse = total_sparse + per_field[k]
                    loss_dict['sfg_sparse_%s' % fc.name] = per_field[k]
            else:
                for fc in fcs:
                    col = self.feature_index[fc.name][0]
                    head = dec.sparse_heads[fc.name]
                    ce = ops.vocab_softmax_ce(hidden, head.weight, head.bias, x_rows[:, col])
                    masked = ce.sum() / num_positive
                    total_sparse = total_sparse + masked
                    loss_dict['sfg_sparse_%s' % fc.name] = masked
            if dec.dense_head is not None:
                cols = [c for fc in self.dense_feature_columns for c in range(*self.feature_index[fc.name])]
                mse = F.mse_loss(dec.dense_head(hidden), x_rows[:, cols], reduction='none').mean(dim=-1)
                total_dense = mse.sum() / num_positive
                loss_dict['sfg_dense'] = total_dense
        else:
            # no selected row (row-parallel: none on THIS rank; it still joins every collective of the step, with exact zeros):
            # the reference's masked loss (`ce_loss * positive_mask`, sfg_decoder.py:285-293) is a zero whose
            # gradients are zero TENSORS, so its optimizer steps the decoder's parameters (moments decay, counters advance);
            # absent gradients would make it skip them
            total_sparse = total_sparse + _ZeroLoss.apply(*[p for p in dec.parameters() if p.requires_grad])
        total = fn.sparse_weight * total_sparse + fn.dense_weight * total_dense
        loss_dict['sfg_total'] = total
        return total, {'sfg_loss': total, 'sfg_loss_dict': loss_dict}

    def compute_sfg_loss(self, X, sparse_embedding_list, dense_value_list, labels):
        """Reference signature (basemodel_sfg.py:420-476): lists of [B,1,D] embeddings and [B,1] dense values."""
        if not self.use_sfg or self.sfg_decoder is None:
            return torch.tensor(0.0, device=X.device), {}
        sparse_concat = torch.cat([e.squeeze(1) if len(e.shape) == 3 else e for e in sparse_embedding_list], dim=-1)
        dense_concat = torch.cat(dense_value_list, dim=-1) if dense_value_list else \
            torch.zeros(X.shape[0], 0, device=X.device)
        return self.compute_sfg_loss_fused(X, torch.cat([sparse_concat, dense_concat], dim=-1), labels)

    # ------------------------------------------------------------------ hooks of BaseModel's train step
    def _loss_forward(self, x, y):
        y_pred, sfg_info = self.forward_with_sfg(x, y)
        y_pred = y_pred.squeeze()
        loss = self.loss_func(y_pred, y.squeeze(), reduction='sum')
        self._step_extra = None
        # the reference logs sfg_loss every epoch when use_sfg, also when it is zero (an epoch after the first
        # validation runs in eval mode there -- fit never calls train() again, basemodel_sfg.py:276 / :493 -- so its
        # forward_with_sfg returns no sfg_info; same here, BaseModel.fit shares that behaviour)
        self._step_log = ("sfg_loss", torch.zeros((), device=loss.device)) if self.use_sfg else None
        if self.use_sfg and sfg_info is not None:
            sfg = sfg_info['sfg_loss']
            if self._sfg_row_weight() != 1.0:
                sfg = sfg * self._sfg_row_weight()
            self._step_extra = self.sfg_weight * sfg
            self._step_log = ("sfg_loss", sfg.detach())
        return y_pred, loss


class xDeepFMPro(BaseModelSFG):
    """xDeepFM + SFG (+ AutoDis) (deepctr/xdeepfm_pro/xdeepfm_pro.py:31-393)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 256), cin_layer_size=(256, 128),
                 cin_split_half=True, cin_activation='relu', l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0,
                 l2_reg_cin=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False,
                 task='binary', device='cpu', gpus=None, use_sfg=True, sfg_weight=0.1, sfg_hidden_units=(128, 64),
                 sfg_dropout=0.1, sfg_positive_only=True, sfg_use_label_attention=True, use_autodis=False,
                 autodis_buckets=16, autodis_temperature=1.0):
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                         l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task, device=device,
                         gpus=gpus, use_sfg=use_sfg, sfg_weight=sfg_weight, sfg_hidden_units=sfg_hidden_units,
                         sfg_dropout=sfg_dropout, sfg_positive_only=sfg_positive_only,
                         sfg_use_label_attention=sfg_use_label_attention)
        self.dnn_hidden_units = dnn_hidden_units
        self.use_dnn = len(dnn_feature_columns) > 0 and len(dnn_hidden_units) > 0
        self.use_autodis = use_autodis
        if use_autodis and len(self.dense_feature_columns) > 0:
            self.autodis_encoder = DenseFeatureEncoder([fc.name for fc in self.dense_feature_columns],
                                                       embedding_dim=self.embedding_dim, use_autodis=True,
                                                       num_buckets=autodis_buckets, temperature=autodis_temperature,
                                                       device=device)
            autodis_output_dim = self.autodis_encoder.get_output_dim()
        else:
            self.autodis_encoder = None
            autodis_output_dim = 0
        if self.use_dnn:
            dnn_input_dim = self.compute_input_dim(dnn_feature_columns)
            if use_autodis and self.autodis_encoder is not None:
                dnn_input_dim += autodis_output_dim - sum(fc.dimension for fc in self.dense_feature_columns)
            self.dnn = DNN(dnn_input_dim, dnn_hidden_units, activation=dnn_activation, l2_reg=l2_reg_dnn,
                           dropout_rate=dnn_dropout, use_bn=dnn_use_bn, init_std=init_std, device=device)
            self.dnn_linear = nn.Linear(dnn_hidden_units[-1], 1, bias=False).to(device)
            self.add_regularization_weight(
                filter(lambda x: 'weight' in x[0] and 'bn' not in x[0], self.dnn.named_parameters()), l2=l2_reg_dnn)
            self.add_regularization_weight(self.dnn_linear.weight, l2=l2_reg_dnn)
        self.cin_layer_size = cin_layer_size
        self.use_cin = len(cin_layer_size) > 0 and len(dnn_feature_columns) > 0
        if self.use_cin:
            self.featuremap_num = (sum(cin_layer_size[:-1]) // 2 + cin_layer_size[-1]) if cin_split_half \
                else sum(cin_layer_size)
            self.cin = CIN(len(self.embedding_dict), cin_layer_size, cin_activation, cin_split_half, l2_reg_cin, seed,
                           device=device)
            self.cin_linear = nn.Linear(self.featuremap_num, 1, bias=False).to(device)
            self.add_regularization_weight(filter(lambda x: 'weight' in x[0], self.cin.named_parameters()), l2=l2_reg_cin)
        self.to(device)

    def forward_with_sfg(self, X, y=None):
        """(y_pred, sfg_info) (xdeepfm_pro.py:203-274) on the fused layouts: one gather launch feeds the CIN (FM
        layout), the DNN, the linear logit and the SFG decoder."""
        emb_fm, dnn_in, logit = self.fused_inputs(X)
        B = X.shape[0]
        plan = self._plan
        if self.use_cin:
            logit = logit + self.cin_linear(self.cin.forward_fm(emb_fm, B, plan.D))
        if self.use_dnn:
            dnn_input = dnn_in
            if self.use_autodis and self.autodis_encoder is not None and plan.nd > 0:
                mD = plan.m * plan.D
                ad = self.autodis_encoder.autodis
                if ad is not None and ad._native(dnn_in[:, mD:]):
                    autodis_out, _ = ad.forward_native(dnn_in[:, mD:])      # the dense columns in place, one launch
                else:
                    dense_list = [dnn_in[:, mD + k:mD + k + 1] for k in range(plan.nd)]
                    autodis_out, _, _ = self.autodis_encoder(dense_list)
                dnn_input = torch.cat([dnn_in[:, :mD], autodis_out], dim=-1)
            logit = logit + self.dnn_linear(self.dnn(dnn_input))
        y_pred = self.out(logit)
        sfg_info = None
        if self.use_sfg and y is not None and self.training:
            sfg_loss, sfg_info = self.compute_sfg_loss_fused(X, dnn_in, y)
            sfg_info['sfg_loss'] = sfg_loss
        return y_pred, sfg_info

    def get_embedding_analysis(self, X):
        """Embedding statistics (xdeepfm_pro.py:281-324)."""
        with torch.no_grad():
            emb_fm, _, _ = self.fused_inputs(X)
            B = X.shape[0]
            all_emb = ops.from_fm_layout(emb_fm, B, self._plan.D)
            flat = all_emb.reshape(B, -1)
            normalized = flat / (flat.norm(dim=1, keepdim=True) + 1e-8)
            cos = torch.mm(normalized, normalized.t())
            return {'mean_embedding': all_emb.mean(dim=0), 'std_embedding': all_emb.std(dim=0),
                    'embedding_variance': all_emb.var(dim=0).mean(),
                    'avg_sample_cosine_similarity': (cos.sum() - cos.trace()) / (cos.numel() - cos.shape[0]),
                    'num_fields': all_emb.shape[1], 'embedding_dim': all_emb.shape[2]}


class xDeepFMProLight(xDeepFMPro):
    """Smaller defaults (deepctr/xdeepfm_pro/xdeepfm_pro.py:327-393)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(128, 64), cin_layer_size=(128, 64),
                 cin_split_half=True, cin_activation='relu', l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0,
                 l2_reg_cin=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False,
                 task='binary', device='cpu', gpus=None, use_sfg=True, sfg_weight=0.05, sfg_hidden_units=(64, 32),
                 sfg_dropout=0.1, sfg_positive_only=True, sfg_use_label_attention=True, use_autodis=False,
                 autodis_buckets=8, autodis_temperature=1.0):
        super().__init__(linear_feature_columns, dnn_feature_columns, dnn_hidden_units=dnn_hidden_units,
                         cin_layer_size=cin_layer_size, cin_split_half=cin_split_half, cin_activation=cin_activation,
                         l2_reg_linear=l2_reg_linear, l2_reg_embedding=l2_reg_embedding, l2_reg_dnn=l2_reg_dnn,
                         l2_reg_cin=l2_reg_cin, init_std=init_std, seed=seed, dnn_dropout=dnn_dropout,
                         dnn_activation=dnn_activation, dnn_use_bn=dnn_use_bn, task=task, device=device, gpus=gpus,
                         use_sfg=use_sfg, sfg_weight=sfg_weight, sfg_hidden_units=sfg_hidden_units, sfg_dropout=sfg_dropout,
                         sfg_positive_only=sfg_positive_only, sfg_use_label_attention=sfg_use_label_attention,
                         use_autodis=use_autodis, autodis_buckets=autodis_buckets, autodis_temperature=autodis_temperature)
