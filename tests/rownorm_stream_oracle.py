"""Numpy restatement of pointops.residual_norm_stream (csrc/rownorm.hip with a half x_type): the rounding rule of a half residual stream.

    p   = fp32(s[n] * y)        x, y widened exactly; s None: p = y
    z32 = fp32(x + p)
    z   = round_T(z32)          ONE rounding to the stream type T (f16: numpy's float16 cast; bf16: torch's CPU cast; both nearest even)
    y None: z is x itself, nothing is rounded.

Everything else is tests/rownorm_oracle.py in float64 evaluated on the STORED z: mean, variance, stat and o are the LayerNorm of the tensor
the caller holds, and the backward reads that tensor again.  dx and dy are returned unrounded (float64): the operator rounds each once.
"""
import numpy as np
import torch

from tests import rownorm_oracle as O

U = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def round_to(v32, name):
    """the fp32 array v32 rounded once to the type `name`, as the fp32 values a tensor of that type holds"""
    v32 = np.ascontiguousarray(v32, np.float32)
    with np.errstate(all="ignore"):
        if name == "f32":
            return v32.copy()
        if name == "f16":
            return v32.astype(np.float16).astype(np.float32)
    assert name == "bf16", name
    return torch.from_numpy(v32).to(torch.bfloat16).float().numpy()


def stream_z(x, y, s, name):
    """-> z32, z: the fp32 sum and the stored z (both fp32 arrays); x must hold values of the type `name`, y of any row type"""
    x32 = np.ascontiguousarray(x, np.float32)
    assert np.array_equal(round_to(x32, name), x32, equal_nan=True), "x is not a tensor of the stream type"
    if y is None:
        return x32.copy(), x32.copy()
    y32 = np.ascontiguousarray(y, np.float32)
    with np.errstate(all="ignore"):
        p = y32 if s is None else (np.ascontiguousarray(s, np.float32)[:, None] * y32).astype(np.float32)
        z32 = (x32 + p).astype(np.float32)
    return z32, round_to(z32, name)


def z_float64(x, y, s):
    """z without any rounding"""
    return O.forward(x, y, s, np.ones(np.shape(x)[1]), np.zeros(np.shape(x)[1]))[0]


def on_stored_z(z, s, gamma, beta, grad_o, grad_z, has_y, eps=1e-5):
    """what follows z, in float64, for a z as some side stored it -> dict(o, stat, dx, dy, dgamma, dbeta)"""
    _, o, stat = O.forward(z, None, None, gamma, beta, eps)
    dx, dy, dgamma, dbeta = O.backward(grad_o, grad_z, z, stat, s, gamma, has_y=has_y)
    return dict(o=o, stat=stat, dx=dx, dy=dy, dgamma=dgamma, dbeta=dbeta)


def residual_norm_stream(x, y, s, gamma, beta, grad_o, grad_z, name, eps=1e-5):
    """-> dict(z32, z (stored, fp32 array), o, stat, dx, dy, dgamma, dbeta): the rule above, then float64 on the stored z"""
    z32, z = stream_z(x, y, s, name)
    out = on_stored_z(z, s, gamma, beta, grad_o, grad_z, y is not None, eps)
    out.update(z32=z32, z=z)
    return out


def z_bound(x, y, s, name):
    """per element: u_T * |z64| + 2^-23 * (|x| + |s * y|), plus half the smallest f16 subnormal - the bar on |z - z64|
    (one rounding of the product and one of the sum in fp32, one to T; an f16 result below 2^-14 is rounded to a multiple of 2^-24)"""
    x64 = np.asarray(x, np.float64)
    sy = 0.0 if y is None else np.abs(np.asarray(y, np.float64) * (1.0 if s is None else np.asarray(s, np.float64)[:, None]))
    z64 = z_float64(x, y, s)
    return U[name] * np.abs(z64) + 2.0 ** -23 * (np.abs(x64) + sy) + (2.0 ** -25 if name == "f16" else 0.0)
