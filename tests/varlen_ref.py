"""Restatement of the pooled variable-length lookup (deepctr/inputs.py:141-155, :213-227 with
deepctr/layers/sequence.py:49-77) in numpy, for the tests of K1v / K2v.  Test-only.

Sums run in float64.  What the reference fixes in fp32 is kept in fp32: the mean's divisor float32(len) + float32(1e-8),
and the max branch, which involves no sum at all -- its value is w, or the single fp32 subtraction w - 1e9 at a masked
position, so it is evaluated in the table's own dtype and compared exactly.  tests/test_varlen_host.py pins this file to
the reference's own results (tests/golden/varlen_pool_*.npz)."""
import numpy as np

EPS32 = 2.0 ** -24


def valid_mask(ids, lengths):
    """[B, T] bool: id != 0 (lengths None) or t < length; ids are truncated as Tensor.long() does."""
    ids = np.asarray(ids).astype(np.int64)
    if lengths is None:
        return ids != 0
    return np.arange(ids.shape[1])[None, :] < np.asarray(lengths).astype(np.int64)[:, None]


def divisor(ids, lengths):
    """[B] float64 value of the fp32 divisor of the mean: float(count or length) + 1e-8."""
    n = valid_mask(ids, lengths).sum(1) if lengths is None else np.asarray(lengths).astype(np.int64)
    return (n.astype(np.float32) + np.float32(1e-8)).astype(np.float64)


def pool(ids, lengths, table, mode):
    """(pooled [B, D], sum_t |w_t| over the valid positions [B, D], argmax position [B, D]).  Ids are clamped to the table
    as the kernels clamp them."""
    table = np.asarray(table)
    idx = np.clip(np.asarray(ids).astype(np.int64), 0, table.shape[0] - 1)
    valid = valid_mask(ids, lengths)
    rows = table[idx]                                                    # [B, T, D]
    if mode == "max":
        v = np.where(valid[:, :, None], rows, rows - rows.dtype.type(1e9))
        pos = v.argmax(1)                                                # the first maximum
        return np.take_along_axis(v, pos[:, None, :], 1)[:, 0], None, pos
    r64 = rows.astype(np.float64) * valid[:, :, None]
    s, a = r64.sum(1), np.abs(r64).sum(1)
    if mode == "mean":
        d = divisor(ids, lengths)[:, None]
        s, a = s / d, a / d
    return s, a, None


def pool_grad(ids, lengths, table, mode, upstream):
    """(dtable [V, D] float64, sum of |addends| [V, D], number of addends per row [V]) for the upstream gradient [B, D] of
    the pooled rows: g for sum and g / divisor for mean at the valid positions, nothing at masked ones; for max g at the
    position of the first maximum WHETHER OR NOT that position is valid, as autograd of torch.max over emb - (1 - mask) * 1e9
    (sequence.py:65-68) sends it: an all-masked sequence hands its gradient to the row its winning masked position looked up
    (row 0 under the zero mask).  n counts, for max, every valid position and every position that won a column, so it is
    an upper bound of the addends and 0 only for rows that receive nothing."""
    table = np.asarray(table)
    V, D = table.shape
    idx = np.clip(np.asarray(ids).astype(np.int64), 0, V - 1)
    valid = valid_mask(ids, lengths)
    g = np.asarray(upstream, np.float64)
    B, T = idx.shape
    coef = np.broadcast_to(g[:, None, :], (B, T, D)).copy()
    if mode == "mean":
        coef = (coef.astype(np.float32) / divisor(ids, lengths).astype(np.float32)[:, None, None]).astype(np.float64)   # an fp32 division per addend
    elif mode == "max":
        _, _, pos = pool(ids, lengths, table, "max")
        won = np.arange(T)[None, :, None] == pos[:, None, :]
        coef = coef * won
        counted = valid | won.any(2)
    if mode != "max":
        coef = coef * valid[:, :, None]
        counted = valid
    dt, ab, n = np.zeros((V, D)), np.zeros((V, D)), np.zeros(V, np.int64)
    np.add.at(dt, idx.reshape(-1), coef.reshape(-1, D))
    np.add.at(ab, idx.reshape(-1), np.abs(coef).reshape(-1, D))
    np.add.at(n, idx.reshape(-1), counted.reshape(-1).astype(np.int64))
    return dt, ab, n


def golden_columns(g):
    """The feature columns of tests/golden/varlen_model_*.npz (make_golden_varlen.py::columns)."""
    from deepctr.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    D = int(g["emb_dim"])
    sparse = [SparseFeat("C%d" % (i + 1), v, D) for i, v in enumerate((7, 8, 9))]
    varlen = [VarLenSparseFeat(SparseFeat("g_mean", 9, D), maxlen=5, combiner="mean"),
              VarLenSparseFeat(SparseFeat("g_sum", 6, D), maxlen=3, combiner="sum", length_name="g_sum_len"),
              VarLenSparseFeat(SparseFeat("g_max", 8, D), maxlen=4, combiner="max")]
    dense = [DenseFeat("I1", 1), DenseFeat("I2", 2)]
    return sparse, varlen, dense


def golden_model(g, device):
    from deepctr import models
    sparse, varlen, dense = golden_columns(g)
    cols = sparse + varlen + dense
    return getattr(models, str(g["cls"]))(cols, cols, dnn_hidden_units=(8, 8), cin_layer_size=(8, 6), l2_reg_dnn=1e-5, device=device)
