"""Float64 reference of the Linear parameter gradients and the per-element error bound an fp32 implementation has to keep.

    dW[o, i] = sum_n g[n, o] * x[n, i]        db[o] = sum_n g[n, o]

    tol_W[o, i] = gamma_N * sum_n |g[n, o] * x[n, i]|        tol_b[o] = gamma_N * sum_n |g[n, o]|
    gamma_N = N u / (1 - N u),  u = 2^-24

gamma_N bounds the relative error of a sum of N products accumulated in fp32 in ANY order, by fused multiply-adds or by rounded
products and additions (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: no term passes through more than N
roundings).  It therefore holds for every chunk length and every number of chunks and is not taken from the code under test.
The float64 reference's own error (u64 = 2^-53 in place of u) is 2^-29 of the bound and is ignored.
"""
import numpy as np

U32 = 2.0 ** -24


def gamma(n, u=U32):
    n = float(n)
    assert n * u < 1
    return n * u / (1.0 - n * u)


def widen(t):
    """a torch tensor of any row type -> float64 numpy, exactly"""
    return t.detach().cpu().double().numpy()


def reference(x, g):
    """x [N, in], g [N, out] float64 -> dict(dW, db, tol_W, tol_b) float64.  Non-finite operands give the non-finite results of
    IEEE arithmetic; the bounds at those elements are non-finite too and mean nothing."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    assert x.ndim == 2 and g.ndim == 2 and x.shape[0] == g.shape[0]
    gam = gamma(x.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        return {"dW": g.T @ x, "db": g.sum(0), "tol_W": gam * (np.abs(g).T @ np.abs(x)), "tol_b": gam * np.abs(g).sum(0)}


def reference_int(x, g):
    """the exact gradients of integer-valued operands, as fp32 (see linear_grads_cases.INT_*: every sum stays below 2^24)"""
    xi, gi = np.rint(np.asarray(x, np.float64)).astype(np.int64), np.rint(np.asarray(g, np.float64)).astype(np.int64)
    dW, db = gi.T @ xi, gi.sum(0)
    assert np.abs(dW).max(initial=0) < 2 ** 24 and np.abs(db).max(initial=0) < 2 ** 24
    return dW.astype(np.float32), db.astype(np.float32)


def input_grad_reference(g, w, u_store=0.0):
    """dX = g @ w for g [N, out], w [out, in] float64, with the bound of an fp32 accumulation over `out` terms whose result is then
    rounded once to a storage type of unit roundoff u_store (0: it stays fp32): |err| <= (gamma_out (1 + u_store) + u_store) sum |g w|"""
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    gam = gamma(w.shape[0])
    return g @ w, (gam * (1.0 + u_store) + u_store) * (np.abs(g) @ np.abs(w))
