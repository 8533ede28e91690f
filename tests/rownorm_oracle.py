"""Float64 restatement of pointops.residual_norm (csrc/rownorm.hip): residual add with a DropPath row scale, LayerNorm, and their backward.

    z = x + s[:, None] * y      (s None: x + y;  y None: x)
    o = (z - mean) * rstd * gamma + beta      mean, var (biased) over the channels of a row, rstd = 1 / sqrt(var + eps)
    xhat = (z - mean) * rstd;  g = dO * gamma;  dz = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)) + dZ
    dx = dz;  dy = s[:, None] * dz;  dgamma = sum_n dO * xhat;  dbeta = sum_n dO

Plain numpy, row by row independent: a non-finite entry stays in its row of z, o, dx, dy (and reaches dgamma / dbeta as the sums say).
"""
import numpy as np


def forward(x, y, s, gamma, beta, eps=1e-5):
    """-> z, o, stat [n, 2] = (mean, rstd)"""
    x, gamma, beta = (np.asarray(t, np.float64) for t in (x, gamma, beta))
    with np.errstate(all="ignore"):
        if y is None:
            z = x.copy()
        else:
            y = np.asarray(y, np.float64)
            z = x + (y if s is None else np.asarray(s, np.float64)[:, None] * y)
        mean = z.mean(axis=1) if z.shape[0] else np.zeros(0)
        d = z - mean[:, None]
        var = (d * d).mean(axis=1) if z.shape[0] else np.zeros(0)
        rstd = 1.0 / np.sqrt(var + eps)
        o = d * rstd[:, None] * gamma + beta
    return z, o, np.stack([mean, rstd], axis=1)


def backward(grad_o, grad_z, z, stat, s, gamma, has_y=True):
    """-> dx, dy (None without y), dgamma, dbeta; grad_o or grad_z may be None (a zero gradient)"""
    z, gamma = np.asarray(z, np.float64), np.asarray(gamma, np.float64)
    mean, rstd = stat[:, 0], stat[:, 1]
    with np.errstate(all="ignore"):
        if grad_o is None:
            dz = np.zeros_like(z)
            dgamma, dbeta = np.zeros_like(gamma), np.zeros_like(gamma)
        else:
            grad_o = np.asarray(grad_o, np.float64)
            xhat = (z - mean[:, None]) * rstd[:, None]
            g = grad_o * gamma
            dz = rstd[:, None] * (g - g.mean(axis=1, keepdims=True) - xhat * (g * xhat).mean(axis=1, keepdims=True))
            dgamma, dbeta = (grad_o * xhat).sum(axis=0), grad_o.sum(axis=0)
        if grad_z is not None:
            dz = dz + np.asarray(grad_z, np.float64)
        dy = None if not has_y else dz.copy() if s is None else np.asarray(s, np.float64)[:, None] * dz
    return dz, dy, dgamma, dbeta


def residual_norm(x, y, s, gamma, beta, grad_o, grad_z, eps=1e-5):
    """-> dict(z, o, stat, dx, dy, dgamma, dbeta), everything float64"""
    z, o, stat = forward(x, y, s, gamma, beta, eps)
    dx, dy, dgamma, dbeta = backward(grad_o, grad_z, z, stat, s, gamma, has_y=y is not None)
    return dict(z=z, o=o, stat=stat, dx=dx, dy=dy, dgamma=dgamma, dbeta=dbeta)


# ---- scaffolding of the block tests: transformer blocks whose attention is a plain Linear (no index needed) ----
import contextlib  # noqa: E402
import copy  # noqa: E402

import torch  # noqa: E402
from torch import nn  # noqa: E402


class LinearAttention(nn.Module):
    """stands where WindowAttention stands in a block; ignores the index arguments of either call convention"""

    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Linear(dim, dim)

    def forward(self, feats, *index_arguments):
        return self.proj(feats)


class FixedDropPath(nn.Module):
    """DropPath with its masks given: the k-th call multiplies the rows by scales[k] (mask / keep_prob)"""

    def __init__(self, scales):
        super().__init__()
        self.scales, self.calls = scales, 0

    def forward(self, x):
        s = self.scales[self.calls]
        self.calls += 1
        return x * s.to(x.dtype).unsqueeze(1)


def make_blocks(block_cls, depth, c, drop_prob, seed):
    """`depth` blocks of block_cls(dim, heads, window, quant) with a LinearAttention and compat.DropPath(drop_prob), non-trivial norms"""
    from stratified_transformer_amd import compat
    torch.manual_seed(seed)
    blocks = nn.ModuleList()
    for _ in range(depth):
        blk = block_cls(c, 3, 0.16, 0.04)
        blk.attn = LinearAttention(c)
        blk.drop_path = compat.DropPath(drop_prob) if drop_prob else nn.Identity()
        for norm in (blk.norm1, blk.norm2):
            nn.init.normal_(norm.weight, 1.0, 0.2)
            nn.init.normal_(norm.bias, 0.0, 0.2)
        blocks.append(blk)
    return blocks


def run_blocks(blocks, feats, swin, chained=True):
    """the layer's loop: every block called with its convention's argument count, successors named when `chained`"""
    from stratified_transformer_amd import layers
    index_arguments = (None,) * (6 if swin else 5)
    with layers.chained_blocks(blocks) if chained else contextlib.nullcontext():
        for blk in blocks:
            feats = blk(feats, *index_arguments)
    return feats


def blocks_float64(blocks, feats, scales, swin):
    """the same blocks in float64 on the CPU with DropPath's row scales given (two per block: attention branch, MLP branch)
    -> output, input gradient of sum(output * go) is left to the caller: returns (output, blocks64, leaf)"""
    b64 = copy.deepcopy(blocks).cpu().double()
    for i, blk in enumerate(b64):
        blk.drop_path = FixedDropPath([s.cpu().double() for s in scales[2 * i:2 * i + 2]])
    leaf = feats.detach().cpu().double().requires_grad_(True)
    return run_blocks(b64, leaf, swin, chained=False), b64, leaf
