"""CPU: the declarations of pointops.residual_norm_stream (header, C ABI table, signature, argument checks, the missing CPU path), the
switch layers.HALF_STREAM, and the numpy restatement of the half stream's rounding rule (tests/rownorm_stream_oracle.py) against
float64.  No HIP compute runs here."""
import inspect

import numpy as np
import pytest
import torch

from stratified_transformer_amd import _lib, layers, pointops, pointops2_cuda, standin
from tests import abi_header
from tests import rownorm_stream_oracle as S
from tests import swin_standin
from tests import rownorm_oracle as O


def test_launchers_are_declared_and_exported():
    I, P, Fl = _lib.I, _lib.P, _lib.F
    assert _lib.SIGNATURES["residual_norm_stream_forward_launcher"] == [I] * 5 + [P] * 5 + [Fl] + [P] * 3
    assert _lib.SIGNATURES["residual_norm_stream_backward_launcher"] == [I] * 5 + [P] * 9 + [I] + [P] * 2
    declared = list(abi_header.declarations())
    for name, old in (("residual_norm_stream_forward_launcher", "residual_norm_forward_launcher"),
                      ("residual_norm_stream_backward_launcher", "residual_norm_backward_launcher")):
        args = abi_header.parameters(name)
        assert len(args) == len(_lib.SIGNATURES[name]) == len(_lib.SIGNATURES[old]) + 1
        assert args[:5] == ["int n", "int c", "int x_type", "int y_type", "int o_type"]               # x_type in front of y_type
        stream = {"forward": ("x", "z"), "backward": ("grad_z", "z", "grad_x")}["forward" if "forward" in name else "backward"]
        for operand in stream:                                                                          # the stream operands are void *
            assert {"void *" + operand, "const void *" + operand} & set(args), (name, operand)
        assert declared.index(name) > declared.index("optim_step_launcher")                           # appended


def test_public_signature():
    assert str(inspect.signature(pointops.residual_norm_stream)) == "(x, y, row_scale, weight, bias, eps=1e-05, out_dtype=None)"
    assert str(inspect.signature(pointops.residual_norm)) == "(x, y, row_scale, weight, bias, eps=1e-05, out_dtype=None)"
    assert issubclass(pointops.ResidualNormStream, torch.autograd.Function)
    from lib.pointops2.functions import pointops as drop_in
    assert drop_in.residual_norm_stream is pointops.residual_norm_stream


def test_half_stream_is_off_by_default():
    assert layers.HALF_STREAM is False


def test_cpu_tensors_raise_no_cpu_fallback():
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x, y, s, w, b = torch.rand(6, 8).to(dt), torch.rand(6, 8).to(dt), torch.ones(6), torch.ones(8), torch.zeros(8)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pointops.residual_norm_stream(x, y, s, w, b)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pointops.residual_norm_stream(x, None, None, w, b)
        z, o, stat = torch.empty(6, 8, dtype=dt), torch.empty(6, 8), torch.empty(6, 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pointops2_cuda.residual_norm_stream_forward(6, 8, x, y, s, w, b, 1e-5, z, o, stat)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pointops2_cuda.residual_norm_stream_backward(6, 8, o, None, z, stat, s, w, torch.empty(6, 8, dtype=dt), torch.empty(6, 8, dtype=dt),
                                                         torch.empty(2, 2, 8), torch.empty(8), torch.empty(8))


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _g(t):
    return None if t is None else _OnGpu(t)


H = torch.float16


@pytest.mark.parametrize("x,y,s,w,b,out_dtype,error,names", [
    (torch.rand(6, 1025).to(H), torch.rand(6, 1025), None, torch.ones(1025), torch.zeros(1025), None, ValueError, "c must be"),
    (torch.rand(6, 8).double(), torch.rand(6, 8), None, torch.ones(8), torch.zeros(8), None, TypeError, "x must be f32, f16 or bf16"),
    (torch.zeros(6, 8, dtype=torch.int16), torch.rand(6, 8), None, torch.ones(8), torch.zeros(8), None, TypeError, "x must be f32, f16 or bf16"),
    (torch.rand(48).to(H), torch.rand(48), None, torch.ones(8), torch.zeros(8), None, ValueError, "x must be"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8).double(), None, torch.ones(8), torch.zeros(8), None, TypeError, "y must be"),
    (torch.rand(6, 8).to(H), torch.rand(5, 8).to(H), None, torch.ones(8), torch.zeros(8), None, ValueError, "y must be"),
    (torch.rand(6, 8).bfloat16(), torch.rand(6, 8), None, torch.ones(7), torch.zeros(8), None, ValueError, "weight must be"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), None, torch.ones(8), torch.zeros(9), None, ValueError, "bias must be"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), None, torch.ones(8).half(), torch.zeros(8), None, TypeError, "weight must be"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), None, torch.ones(8), None, None, ValueError, "bias is None"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), torch.ones(6, 1), torch.ones(8), torch.zeros(8), None, ValueError, "row_scale must be"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), torch.ones(5), torch.ones(8), torch.zeros(8), None, ValueError, "row_scale must be"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), torch.ones(6).half(), torch.ones(8), torch.zeros(8), None, TypeError, "row_scale must be"),
    (torch.rand(6, 8).to(H), None, torch.ones(6), torch.ones(8), torch.zeros(8), None, ValueError, "row_scale needs y"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), None, torch.ones(8), torch.zeros(8), torch.float64, TypeError, "out_dtype"),
    (torch.rand(8, 6).to(H).t(), torch.rand(6, 8), None, torch.ones(8), torch.zeros(8), None, ValueError, "x must be contiguous"),
    (torch.rand(6, 8).to(H), torch.rand(6, 16)[:, ::2], None, torch.ones(8), torch.zeros(8), None, ValueError, "y must be contiguous"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), torch.ones(12)[::2], torch.ones(8), torch.zeros(8), None, ValueError, "row_scale must be contiguous"),
    (torch.rand(6, 8).to(H), torch.rand(6, 8), None, torch.ones(16)[::2], torch.zeros(8), None, ValueError, "weight must be contiguous"),
])
def test_operator_rejects_bad_arguments(x, y, s, w, b, out_dtype, error, names):
    with pytest.raises(error, match="residual_norm_stream: .*" + names):
        pointops.residual_norm_stream(_g(x), _g(y), _g(s), _g(w), _g(b), out_dtype=out_dtype)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_residual_norm_still_rejects_a_half_stream(dt):
    x, y, w, b = torch.rand(6, 8).to(dt), torch.rand(6, 8).to(dt), torch.ones(8), torch.zeros(8)
    with pytest.raises(TypeError, match="residual_norm: x must be f32"):
        pointops.residual_norm(_g(x), _g(y), None, _g(w), _g(b))
    f32 = lambda *s: _OnGpu(torch.zeros(*s))
    with pytest.raises(TypeError, match="x"):
        pointops2_cuda.residual_norm_forward(6, 8, _g(x), _g(y), None, f32(8), f32(8), 1e-5, f32(6, 8), f32(6, 8), f32(6, 2))


def test_binding_rejects_bad_shapes_and_dtypes():
    C = pointops2_cuda
    f32 = lambda *s: _OnGpu(torch.zeros(*s))
    f16 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.float16))
    bf16 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.bfloat16))
    f64 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.float64))
    ok = lambda: dict(x=f16(6, 8), y=f32(6, 8), row_scale=f32(6), weight=f32(8), bias=f32(8), eps=1e-5, z=f16(6, 8), o=bf16(6, 8), stat=f32(6, 2))
    cases = [("c", ValueError, dict(c=1025)), ("c", ValueError, dict(c=0)), ("n", ValueError, dict(n=-1)),
             ("x", TypeError, dict(x=f64(6, 8))), ("x", ValueError, dict(x=f16(5, 8))), ("x", RuntimeError, dict(x=_OnGpu(torch.zeros(8, 6).half().t()))),
             ("z", TypeError, dict(z=f32(6, 8))), ("z", TypeError, dict(z=bf16(6, 8))), ("z", ValueError, dict(z=f16(6, 7))),
             ("y", TypeError, dict(y=f64(6, 8))), ("y", ValueError, dict(y=f16(6, 9))),
             ("row_scale", ValueError, dict(row_scale=f32(6, 1))), ("row_scale", TypeError, dict(row_scale=f16(6))),
             ("row_scale", ValueError, dict(y=None)),
             ("weight", ValueError, dict(weight=f32(7))), ("bias", TypeError, dict(bias=f16(8))),
             ("o", TypeError, dict(o=_OnGpu(torch.zeros(6, 8, dtype=torch.int32)))), ("o", ValueError, dict(o=f16(6, 7))),
             ("stat", ValueError, dict(stat=f32(6)))]
    for name, error, change in cases:
        kw = dict(ok(), n=6, c=8)
        kw.update(change)
        with pytest.raises(error, match=name):
            C.residual_norm_stream_forward(kw["n"], kw["c"], kw["x"], kw["y"], kw["row_scale"], kw["weight"], kw["bias"], kw["eps"], kw["z"], kw["o"],
                                           kw["stat"])
    okb = lambda: dict(grad_o=f16(6, 8), grad_z=bf16(6, 8), z=bf16(6, 8), stat=f32(6, 2), row_scale=f32(6), weight=f32(8), grad_x=bf16(6, 8),
                       grad_y=f16(6, 8), partials=f32(2, 2, 8), grad_weight=f32(8), grad_bias=f32(8))
    cases = [("grad_o", ValueError, dict(grad_o=f16(6, 7))), ("z", ValueError, dict(z=bf16(7, 8))), ("z", TypeError, dict(z=f64(6, 8))),
             ("grad_z", TypeError, dict(grad_z=f16(6, 8))), ("grad_z", TypeError, dict(grad_z=f32(6, 8))), ("grad_z", ValueError, dict(grad_z=bf16(6, 9))),
             ("grad_x", TypeError, dict(grad_x=f16(6, 8))), ("grad_x", TypeError, dict(grad_x=f32(6, 8))), ("grad_x", ValueError, dict(grad_x=bf16(5, 8))),
             ("stat", ValueError, dict(stat=f32(6, 3))), ("grad_y", ValueError, dict(grad_y=f16(5, 8))),
             ("partials", ValueError, dict(partials=f32(2, 2, 7))), ("partials", ValueError, dict(partials=f32(1025, 2, 8))),
             ("partials", ValueError, dict(partials=None)), ("grad_weight", ValueError, dict(grad_weight=f32(9))),
             ("grad_bias", ValueError, dict(grad_bias=None)), ("c", ValueError, dict(c=1025))]
    for name, error, change in cases:
        kw = dict(okb(), n=6, c=8)
        kw.update(change)
        with pytest.raises(error, match=name):
            C.residual_norm_stream_backward(kw["n"], kw["c"], kw["grad_o"], kw["grad_z"], kw["z"], kw["stat"], kw["row_scale"], kw["weight"],
                                            kw["grad_x"], kw["grad_y"], kw["partials"], kw["grad_weight"], kw["grad_bias"])


@pytest.mark.parametrize("swin", [False, True])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_half_stream_on_cpu_tensors_runs_the_original_forward(swin, dt):
    """the switch changes nothing where the fused path cannot run: half CPU feats go through the original forward, same bits, same draws"""
    cls = swin_standin.SwinTransformerBlock if swin else standin.SwinTransformerBlock
    blocks = O.make_blocks(cls, 2, 24, 0.3, seed=3).train().to(dt)
    feats = torch.randn(50, 24, generator=torch.Generator().manual_seed(4)).to(dt)
    torch.manual_seed(9)
    want = O.run_blocks(blocks, feats, swin, chained=False)
    state = torch.get_rng_state()
    try:
        layers.HALF_STREAM = True
        layers.patch_block_classes(swin_block_cls=cls) if swin else layers.patch_block_classes(cls)
        torch.manual_seed(9)
        got = O.run_blocks(blocks, feats, swin, chained=True)
        assert got.dtype == dt and torch.equal(got, want) and torch.equal(torch.get_rng_state(), state)
    finally:
        layers.HALF_STREAM = False
        layers.uninstall_fast_layers()
    assert not layers._ORIGINAL


@pytest.mark.parametrize("name", ["f16", "bf16"])
@pytest.mark.parametrize("with_s", [True, False])
def test_restatement_is_within_the_bound_of_float64(name, with_s):
    """z of the restatement: |z - z64| <= u_T |z64| + 2^-23 (|x| + |s y|) (+ 2^-25 for f16); z is a value of T; a dropped row is x"""
    g = torch.Generator().manual_seed(17)
    n, c = 257, 40
    x = (torch.randn(n, c, generator=g) * torch.logspace(-6, 2, n).unsqueeze(1)).to(S.TORCH[name])           # rows from 1e-6 (f16 subnormals) to 1e2
    y = (torch.randn(n, c, generator=g) * torch.logspace(2, -6, n).unsqueeze(1)).to(S.TORCH[name])
    s = ((torch.rand(n, generator=g) >= 0.3).float() / 0.7) if with_s else None
    xn, yn, sn = x.float().numpy(), y.float().numpy(), None if s is None else s.numpy()
    z32, z = S.stream_z(xn, yn, sn, name)
    assert z32.dtype == z.dtype == np.float32 and np.array_equal(S.round_to(z, name), z)
    z64 = S.z_float64(xn, yn, sn)
    excess = float((np.abs(z.astype(np.float64) - z64) - S.z_bound(xn, yn, sn, name)).max())
    worst = float((np.abs(z.astype(np.float64) - z64) / np.maximum(np.abs(z64), 2.0 ** -14)).max())
    print(f"restatement {name} s={'mask' if with_s else 'None'}: z excess {excess:.1e}, worst relative error {worst:.2e} (u = {S.U[name]:.2e})")
    assert excess <= 0.0
    assert float(np.abs(z.astype(np.float64) - z64).max()) > 0.0                                                # and it does round
    if with_s:
        assert np.array_equal(z[sn == 0], xn[sn == 0]) and int((sn == 0).sum()) > 30
    # y None: z is x, bit for bit
    z32, z = S.stream_z(xn, None, None, name)
    assert np.array_equal(z.view(np.uint32), xn.view(np.uint32)) and np.array_equal(z32.view(np.uint32), xn.view(np.uint32))
    # and what follows is rownorm_oracle on the stored z
    gamma, beta = np.linspace(0.5, 1.5, c), np.linspace(-0.2, 0.2, c)
    go, gz = torch.randn(n, c, generator=g).numpy(), torch.randn(n, c, generator=g).numpy()
    full = S.residual_norm_stream(xn, yn, sn, gamma, beta, go, gz, name)
    z_, o_, stat_ = O.forward(full["z"], None, None, gamma, beta)
    assert np.array_equal(o_, full["o"]) and np.array_equal(stat_, full["stat"]) and np.array_equal(z_, full["z"].astype(np.float64))
    dx, dy, dgamma, dbeta = O.backward(go, gz, full["z"], stat_, sn, gamma)
    assert np.array_equal(dx, full["dx"]) and np.array_equal(dy, full["dy"]) and np.array_equal(dgamma, full["dgamma"])
