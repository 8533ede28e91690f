"""numpy restatement of what csrc/optim.hip adds to the AdamW step of tests/optim_oracle.py: torch.optim.SGD's update (dampening = 0,
maximize = False) and the clip by the global gradient norm (torch.nn.utils.clip_grad_norm_), in the device's operations and order.

SGD, per element, nothing fused (dtype=np.float32: the device's bits; dtype=np.float64: the accuracy yardstick):

    g = (grad * inv_scale) * coef
    if weight_decay != 0:  g = g + (p * weight_decay)
    if momentum != 0:      buf = (buf * momentum) + g;   g = g + (buf * momentum) if nesterov else buf
    p = p - (g * lr)

The buffer starts as zeros, so the first step leaves g in it.

The squared norm: a chunk is 4096 elements of one tensor (the last one padded with zeros, which add nothing); element i of a chunk belongs
to thread (i / 4) % 256, i.e. the chunk viewed as [s = 4, thread = 256, c = 4]; a thread adds double(x) * double(x), x = grad * inv_scale
in `dtype`, over (s, c) in ascending order; the 256 sums are folded by a halving tree (stride 128 ... 1: a[j] = a[j] + a[j + stride]); the
chunks' sums, in table order, are added by thread j = chunk % 256 in ascending order and folded by the same tree.
"""
import numpy as np

from tests import optim_oracle as O

CHUNK, THREADS = 4096, 256


def _tree(a):
    """halving tree over the last axis (THREADS long) -> that axis removed"""
    a = np.array(a, dtype=np.float64)
    stride = THREADS // 2
    while stride >= 1:
        a[..., :stride] = a[..., :stride] + a[..., stride:2 * stride]
        stride //= 2
    return a[..., 0]


def chunk_partials(grad, scale=None, dtype=np.float32):
    """the float64 partial of every chunk of one gradient"""
    x = np.asarray(grad, dtype=dtype).reshape(-1) * O.inv_scale_of(scale, dtype)
    n_chunks = -(-x.size // CHUNK)
    sq = np.zeros(n_chunks * CHUNK, np.float64)
    sq[:x.size] = x.astype(np.float64) * x.astype(np.float64)
    sq = sq.reshape(n_chunks, CHUNK // (4 * THREADS), THREADS, 4)
    acc = np.zeros((n_chunks, THREADS), np.float64)
    for s in range(sq.shape[1]):
        for c in range(4):
            acc = acc + sq[:, s, :, c]
    return _tree(acc)


def grad_sq_sum(grads, scale=None, dtype=np.float32):
    """S, the sum of squares of all the unscaled gradients (None entries are left out), a float64"""
    partial = np.concatenate([np.zeros(0)] + [chunk_partials(g, scale, dtype) for g in grads if g is not None])
    padded = np.zeros(-(-max(partial.size, 1) // THREADS) * THREADS, np.float64)
    padded[:partial.size] = partial
    acc = np.zeros(THREADS, np.float64)
    with np.errstate(invalid="ignore"):
        for row in padded.reshape(-1, THREADS):
            acc = acc + row
        return np.float64(_tree(acc))


def clip_coef(S, max_norm, dtype=np.float32):
    """(the norm as the device reports it, the factor on every gradient): torch's clip_grad_norm_ formula, rounded to `dtype` once"""
    with np.errstate(invalid="ignore"):
        norm = np.sqrt(np.float64(S))
        r = np.float64(max_norm) / (norm + np.float64(1e-6))
    return dtype(norm), dtype(r if r < 1.0 else 1.0)


def sgd_tensor(p, grad, buf, group, scale=None, coef=None, dtype=np.float32):
    """one update of one tensor; group = dict(lr, momentum, weight_decay, nesterov); buf may be None when momentum is 0 -> (p, buf)"""
    lr, momentum, wd = dtype(group["lr"]), dtype(group["momentum"]), dtype(group["weight_decay"])
    p, grad = np.asarray(p, dtype=dtype), np.asarray(grad, dtype=dtype)
    g = (grad * O.inv_scale_of(scale, dtype)) * dtype(1.0 if coef is None else coef)
    if wd != 0:
        g = g + (p * wd)
    if momentum != 0:
        buf = (np.asarray(buf, dtype=dtype) * momentum) + g
        g = g + (buf * momentum) if group.get("nesterov") else buf
    p = p - (g * lr)
    assert p.dtype == dtype and (buf is None or buf.dtype == dtype)
    return p, buf


class State:
    """params and optimizer state of a list of tensors under kind "adamw" (m, v, t: optim_oracle's) or "sgd" (m: the momentum buffer),
    stepped with skip, scale and clip as the device steps them"""

    def __init__(self, kind, params, groups, group_of, dtype=np.float32, max_norm=None):
        assert kind in ("adamw", "sgd")
        self.kind, self.dtype, self.max_norm = kind, dtype, max_norm
        self.p = [np.array(a, dtype=dtype) for a in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.t = [0] * len(self.p)
        self.groups, self.group_of = groups, list(group_of)
        self.norm, self.coef = None, None

    def step(self, grads, scale=None, found_inf=None):
        """grads: one array or None (skipped) per tensor -> whether the whole step was skipped (a gradient is not finite; found_inf None:
        checked here).  With max_norm, self.norm and self.coef are this step's, skipped or not"""
        live = [g for g in grads if g is not None]
        self.norm, self.coef = None, None
        if self.max_norm is not None and live:
            self.norm, self.coef = clip_coef(grad_sq_sum(grads, scale, self.dtype), self.max_norm, self.dtype)
        skipped = O.non_finite(live) if found_inf is None else bool(found_inf)
        if skipped:
            return True
        coef = self.dtype(1.0) if self.coef is None else self.coef
        for i, g in enumerate(grads):
            if g is None:
                continue
            group = self.groups[self.group_of[i]]
            if self.kind == "sgd":
                self.p[i], self.m[i] = sgd_tensor(self.p[i], g, self.m[i], group, scale, coef, self.dtype)
                self.t[i] += 1
            else:   # the unscaled, clipped gradient goes in; adamw_tensor's own unscale is then a multiplication by 1
                g = (np.asarray(g, dtype=self.dtype) * O.inv_scale_of(scale, self.dtype)) * coef
                self.p[i], self.m[i], self.v[i], self.t[i] = O.adamw_tensor(self.p[i], g, self.m[i], self.v[i], self.t[i], group, None, self.dtype)
        return False
