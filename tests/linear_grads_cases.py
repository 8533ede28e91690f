"""The shapes, row types and operands on which pointops.linear_param_grads is tested (tests/test_linear_grads_cpu.py checks the cases
themselves, tests/test_linear_grads_hip.py runs them).  Torch on the CPU and numpy only.

R is the chunk length of csrc/linear_grads.hip, as the package exposes it; the row counts sit around it and nothing else reads it."""
import functools

import numpy as np
import torch

from tests import linear_grads_oracle as oracle
from stratified_transformer_amd._lib import LINEAR_GRADS_ROWS as R

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
N_LIST = (0, 1, 3, 4, 5, 63, 64, 65, R - 1, R, R + 1, 3 * R + 5)
SHAPES = ((1, 1), (3, 13), (15, 17), (16, 16), (17, 15), (48, 48), (48, 192), (192, 48), (384, 1536))  # (in, out)
TYPE_PAIRS = ((F32, F32), (F16, F16), (BF16, BF16), (F16, F32))  # (x, g)
INT_MAX_ABS, INT_MAX_N = 3, 4096  # integer-valued operands: every partial sum is below 9 * 4096 < 2^24, exact in fp32 in any order


def _case(n, shape, types=(F32, F32), bias=True, view=None):
    """view: None, "strided" (x and g are column slices of wider tensors: they need .contiguous()) or "3d" ([n / 16, 16, features])"""
    assert shape != (384, 1536) or n <= 65
    assert view != "3d" or n % 16 == 0
    return {"n": n, "in": shape[0], "out": shape[1], "x_dtype": types[0], "g_dtype": types[1], "bias": bias, "view": view}


def _cases():
    out = [_case(n, (48, 192)) for n in N_LIST]                                   # the full row list on the shape to plan for
    out += [_case(n, (15, 17), (F16, F16)) for n in N_LIST]                       # and on odd half rows
    small = (5, 65, R + 1)
    for j, shape in enumerate(SHAPES):                                            # every shape with every type pair, rows rotating
        for t, types in enumerate(TYPE_PAIRS):
            n = small[(j + t) % 3] if shape != (384, 1536) else (4, 65)[t % 2]
            if (shape, types) in (((48, 192), (F32, F32)), ((15, 17), (F16, F16))):
                continue
            if shape == (384, 1536) and types[0] != types[1]:
                continue
            out.append(_case(n, shape, types, bias=(j + t) % 4 != 3))
    out.append(_case(3 * R + 5, (48, 48), (BF16, BF16)))
    out.append(_case(3 * R + 5, (17, 15), (F16, F32), bias=False))
    out.append(_case(R - 1, (192, 48), (F32, F32), bias=False))
    out.append(_case(R + 1, (48, 192), (F16, F16), view="strided"))
    out.append(_case(65, (17, 15), (F32, F32), view="strided"))
    out.append(_case(5 * 16, (48, 192), (F32, F32), view="3d"))
    out.append(_case(R + 16, (15, 17), (BF16, BF16), view="3d", bias=False))
    return out


CASES = _cases()


def case_id(c):
    name = {F32: "f32", F16: "f16", BF16: "bf16"}
    return (f"n{c['n']}-{c['in']}x{c['out']}-{name[c['x_dtype']]}-{name[c['g_dtype']]}" + ("" if c["bias"] else "-nobias")
            + (f"-{c['view']}" if c["view"] else ""))


def _seed(c, kind):
    return [c["n"], c["in"], c["out"], TYPE_PAIRS.index((c["x_dtype"], c["g_dtype"])), {"int": 0, "random": 1}[kind]]


def _as_view(t, view):
    """the stored values of t [n, f] behind the case's view"""
    if view == "strided":
        wide = torch.zeros((t.shape[0], 2 * t.shape[1] + 1), dtype=t.dtype, device=t.device)
        wide[:, 1::2] = t
        v = wide[:, 1::2]
        assert not v.is_contiguous() and torch.equal(v, t)
        return v
    if view == "3d":
        return t.reshape(t.shape[0] // 16, 16, t.shape[1])
    return t


@functools.lru_cache(maxsize=None)
def _operands(idx, kind):
    c = CASES[idx]
    rng = np.random.default_rng(_seed(c, kind))
    shapes = ((c["n"], c["in"]), (c["n"], c["out"]))
    if kind == "int":
        x, g = (rng.integers(-INT_MAX_ABS, INT_MAX_ABS + 1, s).astype(np.float32) for s in shapes)
    else:
        x, g = (rng.standard_normal(s).astype(np.float32) for s in shapes)
    return torch.from_numpy(x).to(c["x_dtype"]), torch.from_numpy(g).to(c["g_dtype"])  # (random: rounded once to the stored type)


def operands(idx, kind, device="cpu"):
    """(x, g): tensors of the case's row types on `device` behind the case's view (made there: a copy to another device would lose the
    strides); kind "int" (entries in {-3 .. 3}) or "random" (standard normal)"""
    x, g = _operands(idx, kind)
    view = CASES[idx]["view"]
    return _as_view(x.to(device), view), _as_view(g.to(device), view)


@functools.lru_cache(maxsize=None)
def expected(idx, kind):
    """the reference of the case, computed once: "int" -> (dW, db) exact fp32; "random" -> oracle.reference's dict, from the stored values widened"""
    x, g = _operands(idx, kind)
    if kind == "int":
        return oracle.reference_int(oracle.widen(x), oracle.widen(g))
    return oracle.reference(oracle.widen(x), oracle.widen(g))
