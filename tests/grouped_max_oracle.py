"""Float64 restatement of the grouped maximum (pointops.grouped_max, csrc/grouped_max.hip) and of the composite it replaces,
TransitionDown's tail (model/stratified_transformer.py:106-109), for the tests.  numpy / torch on the CPU; no HIP runs here.

    forward:   out[i, ch] = max_n feat[idx[i, n], ch], arg[i, ch] = the smallest n that attains it (nn.MaxPool1d's rule); a NaN among
               the k values gives NaN, arg = the n of the first NaN; idx entries outside [0, n_s) are skipped; a row with no valid
               entry gives 0 and arg 255
    backward:  grad_feat[j, ch] = sum over (i, n) with idx[i, n] == j and arg[i, ch] == n of grad_out[i, ch]
"""
import numpy as np
import torch

NO_ARG = 255


def forward(feat, idx):
    """feat [n_s, c] float64 (a widened f32 / f16 / bf16 array: widening is exact, and so is the selection), idx [m, k] integers
    -> out [m, c] float64 (every entry an element of feat, or 0), arg [m, c] uint8"""
    feat, idx = np.asarray(feat, np.float64), np.asarray(idx).astype(np.int64)
    (m, k), (n_s, c) = idx.shape, feat.shape
    out = np.zeros((m, c), np.float64)
    arg = np.full((m, c), NO_ARG, np.uint8)
    if m == 0 or n_s == 0:
        return out, arg
    for n in range(k):                                                            # MaxPool1d walks the window in order
        j = idx[:, n]
        valid = (j >= 0) & (j < n_s)
        x = feat[np.where(valid, j, 0)]
        with np.errstate(invalid="ignore"):
            take = valid[:, None] & ((arg == NO_ARG) | (x > out) | (np.isnan(x) & ~np.isnan(out)))
        out = np.where(take, x, out)
        arg = np.where(take, np.uint8(n), arg)
    return out, arg


def backward(grad_out, idx, arg, n_s):
    """float64 sums -> grad_feat [n_s, c] float64, terms [n_s, c] (how many grad_out entries each sum has), abs_sum [n_s, c] (sum |term|)"""
    grad_out, idx, arg = np.asarray(grad_out).astype(np.float64), np.asarray(idx).astype(np.int64), np.asarray(arg)
    (m, k), c = idx.shape, grad_out.shape[1]
    grad = np.zeros((n_s, c), np.float64)
    terms = np.zeros((n_s, c), np.int64)
    abs_sum = np.zeros((n_s, c), np.float64)
    if m == 0 or n_s == 0:
        return grad, terms, abs_sum
    rows = np.arange(m)[:, None].repeat(c, 1)
    cols = np.arange(c)[None, :].repeat(m, 0)
    has = arg != NO_ARG
    src = idx[rows[has], arg[has].astype(np.int64)]                               # the source row each (i, ch) took its maximum from
    np.add.at(grad, (src, cols[has]), grad_out[has])
    np.add.at(terms, (src, cols[has]), 1)
    np.add.at(abs_sum, (src, cols[has]), np.abs(grad_out[has]))
    return grad, terms, abs_sum


def per_source(feats, knn, norm_weight, norm_bias, weight, eps=1e-5):
    """y = linear(norm(feats)) on the source rows, float64 torch -> (pooled [m, c_out], y [n, c_out]); differentiable"""
    x = feats
    if norm_weight is not None:
        x = torch.nn.functional.layer_norm(x, (x.shape[1],), norm_weight, norm_bias, eps)
    y = x @ weight.t()
    return y[knn.long()].max(dim=1).values, y


def composite(feats, knn, norm_weight, norm_bias, weight, eps=1e-5):
    """:106-109 as the reference orders it, float64 torch: gather the k rows of every group, norm and linear on the m * k rows, then
    MaxPool1d(k) over the transposed [m, c_out, k] -> pooled [m, c_out]; differentiable"""
    m, k = knn.shape
    rows = feats[knn.reshape(-1).long(), :]
    if norm_weight is not None:
        rows = torch.nn.functional.layer_norm(rows, (rows.shape[1],), norm_weight, norm_bias, eps)
    rows = (rows @ weight.t()).view(m, k, -1).transpose(1, 2).contiguous()
    return torch.nn.functional.max_pool1d(rows, k).squeeze(-1)
