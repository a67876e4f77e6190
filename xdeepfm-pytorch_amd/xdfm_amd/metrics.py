"""numpy metrics with the semantics of the sklearn functions the reference's `compile` wires in
(deepctr/models/basemodel.py:496-512: log_loss, roc_auc_score, mean_squared_error, accuracy)."""
import numpy as np
import torch


def log_loss(y_true, y_pred):
    """Binary cross-entropy, mean over samples; probabilities clipped to [eps, 1-eps] with
    eps = machine epsilon of y_pred's dtype (sklearn >= 1.5 behaviour; the reference always passes
    float64 predictions, basemodel.py:269,352)."""
    y = np.asarray(y_true, dtype=np.float64).ravel()
    p = np.asarray(y_pred)
    eps = np.finfo(p.dtype if p.dtype.kind == "f" else np.float64).eps
    p = np.clip(p.astype(np.float64).ravel(), eps, 1 - eps)
    return float(-np.mean(y * np.log(p) + (1 - y) * np.log(1 - p)))


def roc_auc_score(y_true, y_score):
    """Area under the ROC curve for binary labels (Mann-Whitney statistic with mid-ranks for ties)."""
    y = np.asarray(y_true).ravel() > 0.5
    s = np.asarray(y_score, dtype=np.float64).ravel()
    n_pos = int(y.sum())
    n_neg = int(y.size - n_pos)
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(s, kind="mergesort")
    ss = s[order]
    # mid-rank of each tie group
    boundaries = np.flatnonzero(np.concatenate(([True], ss[1:] != ss[:-1], [True])))
    starts, ends = boundaries[:-1], boundaries[1:]
    mid = 0.5 * (starts + ends - 1) + 1.0
    ranks = np.empty(s.size, dtype=np.float64)
    ranks[order] = np.repeat(mid, ends - starts)
    return float((ranks[y].sum() - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * n_neg))


def mean_squared_error(y_true, y_pred):
    d = np.asarray(y_true, dtype=np.float64).ravel() - np.asarray(y_pred, dtype=np.float64).ravel()
    return float(np.mean(d * d))


def accuracy_score(y_true, y_pred):
    return float(np.mean(np.asarray(y_true).ravel() == np.asarray(y_pred).ravel()))


# ------------------------------------------------------------------------------------------------------------------
# Sample-weighted versions (compile(weighted_metrics=...)), float64 throughout.  A row with w == 0 contributes nothing: it is
# selected away before any arithmetic, not multiplied, so a NaN score on it is harmless.  Positives are y > 0.5.
# W = sum w, Wpos = sum over the positives, Wneg = sum over the others: each its own sum, Wneg is never W - Wpos.
# W == 0 gives NaN (for the AUC: the one-class error, as there is no weighted pair).  With unit weights each function returns
# the bits of its unweighted namesake.
# ------------------------------------------------------------------------------------------------------------------
def _live(y_true, y_pred, w):
    y = np.asarray(y_true, dtype=np.float64).ravel()
    p = np.asarray(y_pred, dtype=np.float64).ravel()
    w = np.asarray(w, dtype=np.float64).ravel()
    if not (y.size == p.size == w.size):
        raise ValueError("weighted metric: %d labels, %d predictions, %d weights" % (y.size, p.size, w.size))
    keep = w > 0
    return y[keep], p[keep], w[keep]


def _ratio(num, den):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(num) / np.float64(den))


def weighted_log_loss(y_true, y_pred, w):
    """-sum w (y log pc + (1 - y) log(1 - pc)) / sum w, pc the clamp of `log_loss` for float64 predictions."""
    y, p, w = _live(y_true, y_pred, w)
    eps = np.finfo(np.float64).eps
    p = np.clip(p, eps, 1 - eps)
    return -_ratio(np.sum(w * (y * np.log(p) + (1 - y) * np.log(1 - p))), np.sum(w))


def weighted_mean_squared_error(y_true, y_pred, w):
    y, p, w = _live(y_true, y_pred, w)
    d = y - p
    return _ratio(np.sum(w * (d * d)), np.sum(w))


def weighted_accuracy_score(y_true, y_pred, w):
    """sum w [(p > 0.5 ? 1 : 0) == y] / sum w: y_pred are scores, thresholded as `compile`'s accuracy does."""
    y, p, w = _live(y_true, y_pred, w)
    return _ratio(np.sum(np.where(np.where(p > 0.5, 1.0, 0.0) == y, w, 0.0)), np.sum(w))


def weighted_roc_auc_score(y_true, y_score, w):
    """Weighted Mann-Whitney statistic with mid-rank ties: (C * 0.5) / (Wpos * Wneg), C = sum over the positives i of
    w_i (cum[lb_i] + cum[ub_i]), where cum is the exclusive prefix sum of the non-positives' weights in ascending (stable)
    score order and lb / ub are the lower / upper bound of the positive's score among those scores (-0.0 == +0.0).
    NaN for a NaN score on a row with w > 0; ValueError when Wpos * Wneg == 0."""
    y, s, w = _live(y_true, y_score, w)
    pos = y > 0.5
    w_pos, w_neg = w[pos], w[~pos]
    Wpos, Wneg = np.sum(w_pos), np.sum(w_neg)
    if Wpos * Wneg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    if np.isnan(s).any():
        return float("nan")
    order = np.argsort(s[~pos], kind="mergesort")
    neg = s[~pos][order]
    cum = np.concatenate(([0.0], np.cumsum(w_neg[order])))
    lb = np.searchsorted(neg, s[pos], side="left")
    ub = np.searchsorted(neg, s[pos], side="right")
    C = np.sum(w_pos * (cum[lb] + cum[ub]))
    return _ratio(C * 0.5, Wpos * Wneg)


WEIGHTED = {log_loss: weighted_log_loss, roc_auc_score: weighted_roc_auc_score, mean_squared_error: weighted_mean_squared_error}


# ------------------------------------------------------------------------------------------------------------------
# The same metrics on device tensors, each returning a 0-d float64 tensor without any host synchronisation: `fit`
# logs them per step (basemodel.py:264-269 calls the sklearn functions on host copies of every batch -- a device
# to host copy, a sync and a CPU sort per step) and reads the epoch's values back once.
# ------------------------------------------------------------------------------------------------------------------
def log_loss_device(y_true, y_pred):
    y = y_true.reshape(-1).double()
    eps = float(np.finfo(np.float64).eps)              # the reference hands float64 predictions to sklearn
    p = y_pred.reshape(-1).double().clamp(eps, 1 - eps)
    return -(y * torch.log(p) + (1 - y) * torch.log(1 - p)).mean()


def roc_auc_score_device(y_true, y_score):
    """Mann-Whitney statistic with mid-ranks, as roc_auc_score above: ranks are multiples of 0.5, so their float64 sum
    is exact in any order and the result equals the numpy version bit for bit.  A batch with a single class gives NaN
    (the host version raises there; `fit` raises the same error when it reads the epoch's values)."""
    pos = (y_true.reshape(-1) > 0.5).double()
    s = y_score.reshape(-1).double()
    ss, _ = torch.sort(s)
    lo = torch.searchsorted(ss, s, right=False)
    hi = torch.searchsorted(ss, s, right=True)
    ranks = 0.5 * (lo + hi - 1).double() + 1.0
    n_pos = pos.sum()
    n_neg = pos.numel() - n_pos
    return ((ranks * pos).sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg)


def mean_squared_error_device(y_true, y_pred):
    d = y_true.reshape(-1).double() - y_pred.reshape(-1).double()
    return (d * d).mean()


DEVICE = {log_loss: log_loss_device, roc_auc_score: roc_auc_score_device, mean_squared_error: mean_squared_error_device}
