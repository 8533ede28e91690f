"""Float64 restatement of pointops.segmentation_loss (csrc/seg_loss.hip): cross-entropy with an ignore label (or the reference's smoothed
form), L1 on the shift head, their weighted sum, the per-class IoU counts of the argmax, and both gradients.

    row n is valid when 0 <= target[n] < C and target[n] != ignore_index; any other label is never used as an index
    m = max_c x;  lse = m + log(sum_c exp(x - m));  logp = x - lse
    loss_n = -logp[target]                                                   (eps == 0)
           = -((1 - eps) * logp[target] + eps / (C - 1) * sum_{c != target} logp_c)   (eps > 0)
    ce = sum_valid loss_n / n_valid;  l1 = sum |shift_pred - shift| / (3 N) over all rows;  total = ce + offset_weight * l1
    pred = numpy's argmax (first maximum, the first NaN if any); over the valid rows counts[0, k] = #(pred == target == k),
    counts[1, k] = #(pred == k) + #(target == k) - counts[0, k], counts[2, k] = #(target == k); rows = (valid, label out of range)
    a = g[0] + g[2];  b = g[1] + offset_weight * g[2]
    grad_logits = a / n_valid * (exp(x - lse) - w) on valid rows, 0 elsewhere;  grad_shift_pred = b / (3 N) * sign(shift_pred - shift)

Plain numpy, row by row independent: a non-finite logit stays in its row's lse and gradient and reaches only the scalar sums.
"""
import numpy as np


def valid_rows(target, c, ignore_index):
    target = np.asarray(target, np.int64)
    return (target >= 0) & (target < c) & (target != ignore_index)


def weights(target, valid, c, eps):
    """the target weights w [n, C] (rows that are not valid: zeros)"""
    w = np.zeros((target.shape[0], c))
    idx = np.nonzero(valid)[0]
    if eps > 0:
        w[idx] = eps / (c - 1)
        w[idx, target[idx]] = 1.0 - eps
    else:
        w[idx, target[idx]] = 1.0
    return w


def segmentation_loss(logits, target, shift_pred=None, shift=None, grad_losses=(0.0, 0.0, 1.0), ignore_index=-100, offset_weight=1.0, smooth_eps=0.0):
    """-> dict(losses [3], lse [n], counts [3, C] int64, rows [2] int64, grad_logits [n, C], grad_shift_pred [n, 3] or None), float64"""
    x, target = np.asarray(logits, np.float64), np.asarray(target, np.int64)
    n, c = x.shape
    g = np.asarray(grad_losses, np.float64)
    valid = valid_rows(target, c, ignore_index)
    n_valid = int(valid.sum())
    w = weights(target, valid, c, smooth_eps)
    with np.errstate(all="ignore"):
        m = x.max(axis=1) if n else np.zeros(0)
        lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
        logp = x - lse[:, None]
        if smooth_eps > 0:
            loss = -np.where(w != 0, w * logp, 0.0).sum(axis=1)   # (every weight of a valid row is non-zero)
        else:
            loss = -np.where(w != 0, logp, 0.0).sum(axis=1)       # the target's entry alone: a -inf elsewhere in the row does not reach it
        ce = loss[valid].sum() / n_valid if n_valid else np.nan
        a = g[0] + g[2]
        grad_logits = np.where(valid[:, None], a / np.float64(n_valid) * (np.exp(logp) - w), 0.0)
        if shift_pred is None:
            l1, total, grad_shift = 0.0, ce, None
        else:
            d = np.asarray(shift_pred, np.float64) - np.asarray(shift, np.float64)
            l1 = np.abs(d).sum() / np.float64(3 * n)
            total = ce + offset_weight * l1
            grad_shift = (g[1] + offset_weight * g[2]) / np.float64(3 * n) * ((d > 0).astype(np.float64) - (d < 0))
    pred = x.argmax(axis=1) if n else np.zeros(0, np.int64)
    tv, pv = target[valid], pred[valid]
    inter = np.bincount(tv[pv == tv], minlength=c)
    tgt = np.bincount(tv, minlength=c)
    counts = np.stack([inter, np.bincount(pv, minlength=c) + tgt - inter, tgt]).astype(np.int64)
    rows = np.array([n_valid, int((~valid & (target != ignore_index)).sum())], np.int64)
    return dict(losses=np.array([ce, l1, total], np.float64), lse=lse, counts=counts, rows=rows, grad_logits=grad_logits, grad_shift_pred=grad_shift)
