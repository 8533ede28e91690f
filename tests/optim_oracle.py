"""numpy restatement of the optimizer step of csrc/optim.hip (torch.optim.AdamW, amsgrad=False, maximize=False, under a loss scale).

dtype=np.float32: exactly the device's operations in the device's order - beta^t by binary exponentiation in float64 with multiplications
only, every per-tensor constant computed in float64 and rounded to fp32 once, then per element (nothing fused):

    g = grad * inv_scale;  p1 = p * decay;  m = (m * beta1) + (g * omb1);  v = (v * beta2) + ((g * g) * omb2)
    denom = (sqrt(v) / sqrt_bias2) + eps;  p = p1 - (step_size * (m / denom))

dtype=np.float64: the same formulas with nothing rounded to fp32 - the accuracy yardstick.
"""
import numpy as np


def pow_by_squaring(beta, n):
    """beta ** n in float64, multiplications only, in the kernel's order"""
    r, b, n = np.float64(1.0), np.float64(beta), int(n)
    while n:
        if n & 1:
            r = r * b
        n >>= 1
        if n:
            b = b * b
    return r


def inv_scale_of(scale, dtype=np.float32):
    """the factor the gradients are multiplied by: float(1.0 / double(float32 scale)), or 1 without a scale"""
    if scale is None:
        return dtype(1.0)
    return dtype(np.float64(1.0) / np.float64(np.float32(scale)))


def constants(t, group, dtype=np.float32):
    """the prologue's record for step count t (already advanced) and group = dict(lr, betas, eps, weight_decay)"""
    lr, (beta1, beta2) = np.float64(group["lr"]), (np.float64(b) for b in group["betas"])
    eps, wd = np.float64(group["eps"]), np.float64(group["weight_decay"])
    bias1 = np.float64(1.0) - pow_by_squaring(beta1, t)
    bias2 = np.float64(1.0) - pow_by_squaring(beta2, t)
    with np.errstate(divide="ignore"):
        return dict(step_size=dtype(lr / bias1), sqrt_bias2=dtype(np.sqrt(bias2)), beta1=dtype(beta1), omb1=dtype(np.float64(1.0) - beta1),
                    beta2=dtype(beta2), omb2=dtype(np.float64(1.0) - beta2), eps=dtype(eps), decay=dtype(np.float64(1.0) - lr * wd))


def non_finite(grads):
    return any(not np.isfinite(g).all() for g in grads)


def adamw_tensor(p, grad, m, v, step, group, scale=None, dtype=np.float32):
    """one update of one tensor -> (p, m, v, step), new arrays"""
    t = int(step) + 1
    c = constants(t, group, dtype)
    p, grad, m, v = (np.asarray(a, dtype=dtype) for a in (p, grad, m, v))
    g = grad * inv_scale_of(scale, dtype)
    p1 = p * c["decay"]
    m = (m * c["beta1"]) + (g * c["omb1"])
    v = (v * c["beta2"]) + ((g * g) * c["omb2"])
    denom = (np.sqrt(v) / c["sqrt_bias2"]) + c["eps"]
    p = p1 - (c["step_size"] * (m / denom))
    assert all(a.dtype == dtype for a in (p, m, v))
    return p, m, v, t


class State:
    """params / exp_avg / exp_avg_sq / step of a list of tensors, each with its group's hyperparameters"""

    def __init__(self, params, groups, group_of, dtype=np.float32):
        self.dtype = dtype
        self.p = [np.array(a, dtype=dtype) for a in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.t = [0] * len(self.p)
        self.groups, self.group_of = groups, list(group_of)

    def step(self, grads, scale=None, found_inf=None):
        """grads: one array or None (skipped) per tensor.  The whole step is skipped when a gradient is not finite (found_inf None: checked
        here) -> whether it was skipped"""
        live = [g for g in grads if g is not None]
        skipped = non_finite(live) if found_inf is None else bool(found_inf)
        if skipped:
            return True
        for i, g in enumerate(grads):
            if g is not None:
                self.p[i], self.m[i], self.v[i], self.t[i] = adamw_tensor(self.p[i], g, self.m[i], self.v[i], self.t[i], self.groups[self.group_of[i]],
                                                                          scale, self.dtype)
        return False
