"""numpy restatement of the gather-add (pointops.gather_add, csrc/upsample.hip) for the tests: the kernel's operations in the kernel's
order, in fp32 - numpy multiplies and adds float32 arrays as two separately rounded operations - so the GPU result is compared
bit for bit.  numpy / torch on the CPU; no HIP runs here.

    forward:   t = 0; for i = 0 .. k-1: t = t + (float(feat[idx[n, i], ch]) * weight[n, i]);  out[n, ch] = float(base[n, ch]) + t
               (base None: out = t); idx entries outside [0, m) are skipped
    backward:  grad_feat[j, ch] = sum over the pairs (n, i) with idx[n, i] == j, in ascending pair id n * k + i, from 0, of
               (grad_out[n, ch] * weight[n, i]), rounded once to feat's dtype; a source row nobody references gets zeros

Operands are torch CPU tensors (f32, f16 or bf16: widening to fp32 is exact, torch's narrowing rounds to nearest even) or arrays.
"""
import numpy as np
import torch


def _f32(x):
    if torch.is_tensor(x):
        return x.detach().cpu().float().numpy()
    return np.asarray(x, np.float32)


def _idx(idx):
    return (idx.detach().cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)).astype(np.int64)


def forward(feat, idx, weight, base=None):
    """-> out [n, c] float32"""
    f, w, idx = _f32(feat), _f32(weight), _idx(idx)
    (n, k), (m, c) = idx.shape, f.shape
    t = np.zeros((n, c), np.float32)
    with np.errstate(all="ignore"):
        for i in range(k):
            j = idx[:, i]
            valid = (j >= 0) & (j < m)
            if m == 0 or not valid.any():
                continue
            prod = f[np.where(valid, j, 0)] * w[:, i:i + 1]             # rounded product
            t = np.where(valid[:, None], t + prod, t)                     # rounded add; a skipped entry adds nothing
        return t if base is None else _f32(base) + t


def source_pairs(idx, m):
    """the key-major view of idx: (pair ids sorted by source row then ascending, their source rows, their rank within the row,
    pair count per source row [m])"""
    flat = _idx(idx).reshape(-1)
    pairs = np.nonzero((flat >= 0) & (flat < m))[0]
    keys = flat[pairs]
    order = np.argsort(keys, kind="stable")
    pairs, keys = pairs[order], keys[order]
    rank = np.arange(keys.shape[0]) - np.searchsorted(keys, keys, side="left")
    return pairs, keys, rank, np.bincount(keys, minlength=m)[:m] if m > 0 else np.zeros(0, np.int64)


def backward(grad_out, idx, weight, m, dtype=torch.float32):
    """-> grad_feat [m, c], a torch tensor of `dtype`"""
    g, w = _f32(grad_out), _f32(weight).reshape(-1)
    k, c = _idx(idx).shape[1], g.shape[1]
    pairs, keys, rank, _ = source_pairs(idx, m)
    acc = np.zeros((m, c), np.float32)
    with np.errstate(all="ignore"):
        for r in range(int(rank.max()) + 1 if rank.size else 0):          # the r-th pair of every source row that has one
            sel = rank == r
            p, j = pairs[sel], keys[sel]
            acc[j] = acc[j] + g[p // k] * w[p][:, None]
    return torch.from_numpy(acc).to(dtype)


def backward_float64(grad_out, idx, weight, m):
    """float64 autograd of the forward's formula -> (grad_feat [m, c] float64, abs_sum [m, c] = sum |grad_out * weight| per element,
    pair count per source row [m])"""
    g = torch.from_numpy(_f32(grad_out)).double()
    w = torch.from_numpy(_f32(weight)).double()
    idx = torch.from_numpy(_idx(idx))
    n, k = idx.shape
    valid = (idx >= 0) & (idx < m)
    safe = torch.where(valid, idx, torch.zeros_like(idx))

    def run(go, ww):
        feat = torch.zeros((max(m, 1), go.shape[1]), dtype=torch.float64, requires_grad=True)
        out = sum(feat[safe[:, i]] * (ww[:, i] * valid[:, i]).unsqueeze(1) for i in range(k))
        out.backward(go)
        return feat.grad[:m]
    return run(g, w).numpy(), run(g.abs(), w.abs()).numpy(), source_pairs(idx, m)[3]
