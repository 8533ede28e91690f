"""Float64 restatement of pointops.batch_norm_act (csrc/batchnorm.hip): BatchNorm1d over the rows, an activation, a residual add, and
their backward.

    training (or no running statistics):  mean_c = sum_n x / N,  var_c = sum_n (x - mean_c)^2 / N (biased)
        running_mean = (1 - m) running_mean + m mean_c,  running_var = (1 - m) running_var + m var_c N / (N - 1)   (training, when given)
    eval with running statistics:         mean_c = running_mean,  var_c = running_var
    rstd_c = 1 / sqrt(var_c + eps);  xhat = (x - mean_c) * rstd_c;  pre = xhat * gamma + beta;  o = act(pre) (+ residual)
    g = dO * act'(pre);  dbeta = sum_n g;  dgamma = sum_n g * xhat;  dresidual = dO
    dx = gamma * rstd * (g - dbeta / N - xhat * dgamma / N)   with batch statistics,   g * gamma * rstd   with running statistics
    act: none | relu (pre <= 0 ? 0 : pre) | leaky_relu (pre > 0 ? pre : slope * pre) | tanh; the derivative takes the forward's branch

Plain numpy, channel by channel independent: a non-finite entry stays in its column of o and dx (and of every per-channel result).
"""
import numpy as np

ACTS = ("none", "relu", "leaky_relu", "tanh")


def _act(pre, act, slope):
    if act == "relu":
        return np.where(pre <= 0, 0.0, pre)
    if act == "leaky_relu":
        return np.where(pre > 0, pre, pre * slope)
    if act == "tanh":
        return np.tanh(pre)
    assert act == "none", act
    return pre


def _act_grad(pre, go, act, slope):
    if act == "relu":
        return np.where(pre <= 0, 0.0, go)
    if act == "leaky_relu":
        return np.where(pre > 0, go, go * slope)
    if act == "tanh":
        return go * (1.0 - np.tanh(pre) ** 2)
    return go


def batch_norm_act(x, gamma, beta, grad_o=None, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5, act="none",
                   negative_slope=0.01, residual=None):
    """-> dict(o, mean, rstd, running_mean, running_var (after the call; None when not given), and with grad_o: dx, dgamma, dbeta, dresidual)"""
    x, gamma, beta = (np.asarray(t, np.float64) for t in (x, gamma, beta))
    n, c = x.shape
    have = running_mean is not None
    rm, rv = (np.asarray(t, np.float64).copy() for t in (running_mean, running_var)) if have else (None, None)
    batch = training or not have
    with np.errstate(all="ignore"):
        if batch:
            mean = x.mean(axis=0) if n else np.zeros(c)
            d = x - mean
            var = (d * d).mean(axis=0) if n else np.zeros(c)
            if training and have and n > 0:
                rm = (1 - momentum) * rm + momentum * mean
                rv = (1 - momentum) * rv + momentum * (var * n / (n - 1))
        else:
            mean, var = rm, rv
        rstd = 1.0 / np.sqrt(var + eps)
        xhat = (x - mean) * rstd
        pre = xhat * gamma + beta
        o = _act(pre, act, negative_slope)
        if residual is not None:
            o = o + np.asarray(residual, np.float64)
        out = dict(o=o, mean=mean, rstd=rstd, running_mean=rm, running_var=rv)
        if grad_o is not None:
            grad_o = np.asarray(grad_o, np.float64)
            g = _act_grad(pre, grad_o, act, negative_slope)
            dbeta, dgamma = g.sum(axis=0), (g * xhat).sum(axis=0)
            dx = gamma * rstd * (g - dbeta / n - xhat * (dgamma / n)) if batch else g * gamma * rstd
            out.update(dx=dx, dgamma=dgamma, dbeta=dbeta, dresidual=grad_o.copy() if residual is not None else None)
    return out
