"""Float64 restatement of pointops.sync_batch_norm_act: batch norm in training mode over the rows of ALL ranks, an activation, a residual
add, and their backward as each rank sees it.

The ranks' rows are concatenated and tests/batchnorm_oracle.batch_norm_act runs on them with the global N (training mode: batch
statistics, the running statistics updated with the unbiased global variance).  o and dx are sliced back per rank.  The parameter
gradients stay LOCAL, as in torch's SyncBatchNorm (DDP averages them afterwards): rank r's dgamma / dbeta are the sums of g * xhat and g
over its OWN rows, with g = dO * act'(pre) and xhat from the global statistics; they add up to the whole batch's.
"""
import numpy as np

from tests import batchnorm_oracle as O


def sync_batch_norm_act(xs, gamma, beta, grad_os=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, act="none",
                        negative_slope=0.01, residuals=None):
    """xs, grad_os, residuals: one [n_r, c] array per rank (n_r = 0: an empty rank; residuals None: no residual) -> dict(o, dx, dgamma,
    dbeta: lists with one entry per rank; mean, rstd, running_mean, running_var, total: of the whole batch, equal on every rank)"""
    xs = [np.asarray(x, np.float64) for x in xs]
    sizes = [x.shape[0] for x in xs]
    cuts = np.cumsum([0] + sizes)
    cat = lambda parts: None if parts is None else np.concatenate([np.asarray(p, np.float64) for p in parts], 0)
    whole = O.batch_norm_act(cat(xs), gamma, beta, cat(grad_os), running_mean, running_var, True, momentum, eps, act, negative_slope, cat(residuals))
    cut = lambda t: [t[cuts[r]:cuts[r + 1]] for r in range(len(xs))]
    out = dict(o=cut(whole["o"]), mean=whole["mean"], rstd=whole["rstd"], running_mean=whole["running_mean"], running_var=whole["running_var"],
               total=int(cuts[-1]))
    if grad_os is not None:
        gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
        dgamma, dbeta = [], []
        with np.errstate(all="ignore"):
            for x, go in zip(xs, grad_os):
                xhat = (x - whole["mean"]) * whole["rstd"]
                g = O._act_grad(xhat * gamma + beta, np.asarray(go, np.float64), act, negative_slope)
                dgamma.append((g * xhat).sum(axis=0))
                dbeta.append(g.sum(axis=0))
        out.update(dx=cut(whole["dx"]), dgamma=dgamma, dbeta=dbeta, whole_dgamma=whole["dgamma"], whole_dbeta=whole["dbeta"])
    return out
