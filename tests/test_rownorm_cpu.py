"""CPU: the declarations of pointops.residual_norm (C ABI table, signatures, argument checks, the missing CPU path), its float64 oracle
(tests/rownorm_oracle.py) against torch's float64 autograd, DropPath's row scale, and the fused block forwards on CPU tensors, where
they must run the original forward.  No HIP compute runs here."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, compat, layers, pointops, pointops2_cuda, standin
from tests import rownorm_oracle as O
from tests import swin_standin


def test_launchers_are_declared_and_exported():
    I, P, Fl = _lib.I, _lib.P, _lib.F
    assert _lib.SIGNATURES["residual_norm_forward_launcher"] == [I] * 4 + [P] * 5 + [Fl] + [P] * 3
    assert _lib.SIGNATURES["residual_norm_backward_launcher"] == [I] * 4 + [P] * 9 + [I] + [P] * 2


def test_public_signatures():
    assert str(inspect.signature(pointops.residual_norm)) == "(x, y, row_scale, weight, bias, eps=1e-05, out_dtype=None)"
    assert str(inspect.signature(sta.install)) == "(third_party=True, fast_layers=False, pooled_transition=False)"
    assert str(inspect.signature(layers.patch_block_classes)) == "(block_cls=None, swin_block_cls=None)"
    assert str(inspect.signature(layers.install_fused_blocks)) == "(module=None)"
    assert sta.install_fused_blocks is layers.install_fused_blocks and "install_fused_blocks" in sta.__all__
    assert issubclass(pointops.ResidualNorm, torch.autograd.Function)
    from lib.pointops2.functions import pointops as drop_in
    assert drop_in.residual_norm is pointops.residual_norm and drop_in.ResidualNorm is pointops.ResidualNorm


def test_cpu_tensors_raise_no_cpu_fallback():
    x, y, s, w, b = torch.rand(6, 8), torch.rand(6, 8), torch.ones(6), torch.ones(8), torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops.residual_norm(x, y, s, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops.residual_norm(x, None, None, w, b)
    z, o, stat = torch.empty(6, 8), torch.empty(6, 8), torch.empty(6, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.residual_norm_forward(6, 8, x, y, s, w, b, 1e-5, z, o, stat)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.residual_norm_backward(6, 8, o, None, z, stat, s, w, torch.empty(6, 8), torch.empty(6, 8), torch.empty(2, 2, 8),
                                              torch.empty(8), torch.empty(8))


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _g(t):
    return None if t is None else _OnGpu(t)


@pytest.mark.parametrize("x,y,s,w,b,out_dtype,error,names", [
    (torch.rand(6, 1025), torch.rand(6, 1025), None, torch.ones(1025), torch.zeros(1025), None, ValueError, "c must be"),   # C = 1025
    (torch.rand(6, 8).double(), torch.rand(6, 8), None, torch.ones(8), torch.zeros(8), None, TypeError, "x must be f32"),
    (torch.rand(6, 8).half(), torch.rand(6, 8), None, torch.ones(8), torch.zeros(8), None, TypeError, "x must be f32"),
    (torch.rand(48), torch.rand(48), None, torch.ones(8), torch.zeros(8), None, ValueError, "x must be"),
    (torch.rand(6, 8), torch.rand(6, 8).double(), None, torch.ones(8), torch.zeros(8), None, TypeError, "y must be"),
    (torch.rand(6, 8), torch.rand(5, 8), None, torch.ones(8), torch.zeros(8), None, ValueError, "y must be"),
    (torch.rand(6, 8), torch.rand(6, 8), None, torch.ones(7), torch.zeros(8), None, ValueError, "weight must be"),          # another length
    (torch.rand(6, 8), torch.rand(6, 8), None, torch.ones(8), torch.zeros(9), None, ValueError, "bias must be"),
    (torch.rand(6, 8), torch.rand(6, 8), None, torch.ones(8).half(), torch.zeros(8), None, TypeError, "weight must be"),
    (torch.rand(6, 8), torch.rand(6, 8), torch.ones(6, 1), torch.ones(8), torch.zeros(8), None, ValueError, "row_scale must be"),   # not [N]
    (torch.rand(6, 8), torch.rand(6, 8), torch.ones(5), torch.ones(8), torch.zeros(8), None, ValueError, "row_scale must be"),
    (torch.rand(6, 8), torch.rand(6, 8), torch.ones(6).half(), torch.ones(8), torch.zeros(8), None, TypeError, "row_scale must be"),
    (torch.rand(6, 8), None, torch.ones(6), torch.ones(8), torch.zeros(8), None, ValueError, "row_scale needs y"),
    (torch.rand(6, 8), torch.rand(6, 8), None, torch.ones(8), torch.zeros(8), torch.float64, TypeError, "out_dtype"),
    (torch.rand(8, 6).t(), torch.rand(6, 8), None, torch.ones(8), torch.zeros(8), None, ValueError, "x must be contiguous"),
    (torch.rand(6, 8), torch.rand(6, 16)[:, ::2], None, torch.ones(8), torch.zeros(8), None, ValueError, "y must be contiguous"),
    (torch.rand(6, 8), torch.rand(6, 8), torch.ones(12)[::2], torch.ones(8), torch.zeros(8), None, ValueError, "row_scale must be contiguous"),
    (torch.rand(6, 8), torch.rand(6, 8), None, torch.ones(16)[::2], torch.zeros(8), None, ValueError, "weight must be contiguous"),
])
def test_operator_rejects_bad_arguments(x, y, s, w, b, out_dtype, error, names):
    with pytest.raises(error, match="residual_norm: .*" + names):
        pointops.residual_norm(_g(x), _g(y), _g(s), _g(w), _g(b), out_dtype=out_dtype)


def test_binding_rejects_bad_shapes_and_dtypes():
    C = pointops2_cuda
    f32 = lambda *s: _OnGpu(torch.zeros(*s))
    f16 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.float16))
    ok = lambda: dict(x=f32(6, 8), y=f16(6, 8), row_scale=f32(6), weight=f32(8), bias=f32(8), eps=1e-5, z=f32(6, 8), o=f16(6, 8), stat=f32(6, 2))
    cases = [("c", ValueError, dict(c=1025)), ("c", ValueError, dict(c=0)), ("n", ValueError, dict(n=-1)),
             ("x", TypeError, dict(x=f16(6, 8))), ("x", ValueError, dict(x=f32(5, 8))), ("x", RuntimeError, dict(x=_OnGpu(torch.zeros(8, 6).t()))),
             ("y", TypeError, dict(y=_OnGpu(torch.zeros(6, 8, dtype=torch.float64)))), ("y", ValueError, dict(y=f16(6, 9))),
             ("row_scale", ValueError, dict(row_scale=f32(6, 1))), ("row_scale", TypeError, dict(row_scale=f16(6))),
             ("row_scale", ValueError, dict(y=None)),
             ("weight", ValueError, dict(weight=f32(7))), ("bias", TypeError, dict(bias=f16(8))),
             ("z", TypeError, dict(z=f16(6, 8))), ("o", TypeError, dict(o=_OnGpu(torch.zeros(6, 8, dtype=torch.int32)))),
             ("o", ValueError, dict(o=f16(6, 7))), ("stat", ValueError, dict(stat=f32(6)))]
    for name, error, change in cases:
        kw = dict(ok(), n=6, c=8)
        kw.update(change)
        with pytest.raises(error, match=name):
            C.residual_norm_forward(kw["n"], kw["c"], kw["x"], kw["y"], kw["row_scale"], kw["weight"], kw["bias"], kw["eps"], kw["z"], kw["o"], kw["stat"])
    okb = lambda: dict(grad_o=f16(6, 8), grad_z=f32(6, 8), z=f32(6, 8), stat=f32(6, 2), row_scale=f32(6), weight=f32(8), grad_x=f32(6, 8),
                       grad_y=f16(6, 8), partials=f32(2, 2, 8), grad_weight=f32(8), grad_bias=f32(8))
    cases = [("grad_o", ValueError, dict(grad_o=f16(6, 7))), ("grad_z", TypeError, dict(grad_z=f16(6, 8))), ("z", ValueError, dict(z=f32(7, 8))),
             ("stat", ValueError, dict(stat=f32(6, 3))), ("grad_x", TypeError, dict(grad_x=f16(6, 8))), ("grad_y", ValueError, dict(grad_y=f16(5, 8))),
             ("partials", ValueError, dict(partials=f32(2, 2, 7))), ("partials", ValueError, dict(partials=f32(1025, 2, 8))),
             ("partials", ValueError, dict(partials=None)), ("grad_weight", ValueError, dict(grad_weight=f32(9))),
             ("grad_bias", ValueError, dict(grad_bias=None)), ("c", ValueError, dict(c=1025))]
    for name, error, change in cases:
        kw = dict(okb(), n=6, c=8)
        kw.update(change)
        with pytest.raises(error, match=name):
            C.residual_norm_backward(kw["n"], kw["c"], kw["grad_o"], kw["grad_z"], kw["z"], kw["stat"], kw["row_scale"], kw["weight"], kw["grad_x"],
                                     kw["grad_y"], kw["partials"], kw["grad_weight"], kw["grad_bias"])


# (row scale, y) x (dZ, dO): a row scale scales y, and one gradient at least arrives
VARIANTS = [(s, y, gz, go) for s, y in ((True, True), (False, True), (False, False)) for gz, go in ((True, True), (False, True), (True, False))]


@pytest.mark.parametrize("with_s,with_y,with_gz,with_go", VARIANTS)
def test_oracle_is_torch_float64_autograd(with_s, with_y, with_gz, with_go):
    g = torch.Generator().manual_seed(5)
    n, c = 37, 24
    x, y, go, gz = (torch.randn(n, c, generator=g, dtype=torch.float64) for _ in range(4))
    s = (torch.rand(n, generator=g, dtype=torch.float64) > 0.3).double() / 0.7
    gamma, beta = torch.randn(c, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (x, y, gamma, beta)]
    z = leaves[0] + (leaves[1] * s[:, None] if with_s else leaves[1]) if with_y else leaves[0] * 1.0
    o = F.layer_norm(z, (c,), leaves[2], leaves[3], 1e-5)
    loss = (o * go).sum() * float(with_go) + (z * gz).sum() * float(with_gz)
    loss.backward()
    got = O.residual_norm(x.numpy(), y.numpy() if with_y else None, s.numpy() if with_s else None, gamma.numpy(), beta.numpy(),
                          go.numpy() if with_go else None, gz.numpy() if with_gz else None)
    want = dict(z=z.detach(), o=o.detach(), dx=leaves[0].grad, dy=leaves[1].grad if with_y else None,
                dgamma=leaves[2].grad if with_go else torch.zeros(c), dbeta=leaves[3].grad if with_go else torch.zeros(c))
    for name, w in want.items():
        if w is None:
            assert got[name] is None
            continue
        scale = max(1.0, float(w.abs().max()))
        assert float(np.abs(got[name] - w.numpy()).max()) <= 1e-12 * scale, name
    mean, var = z.detach().mean(1), z.detach().var(1, unbiased=False)
    assert float((torch.from_numpy(got["stat"][:, 0]) - mean).abs().max()) <= 1e-12
    assert float((torch.from_numpy(got["stat"][:, 1]) - (var + 1e-5).rsqrt()).abs().max()) <= 1e-12 * float((var + 1e-5).rsqrt().max())


def test_row_scale_is_what_drop_path_applies():
    dp = compat.DropPath(0.3).train()
    ones = torch.ones(500, 6)
    torch.manual_seed(11)
    want = dp(ones)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    s = layers.drop_path_row_scale(dp, ones)
    assert torch.equal(torch.get_rng_state(), state)                            # the same draw: the generator stands where the module leaves it
    assert s.dtype == torch.float32 and tuple(s.shape) == (500,)
    assert torch.equal((s == 0), (want[:, 0] == 0)) and 0.2 < float((s == 0).float().mean()) < 0.4
    assert float((s[:, None].expand_as(want) - want).abs().max()) <= 2.0 ** -23 * float(want.max())   # x / keep * mask against mask / keep
    torch.manual_seed(11)
    half = layers.drop_path_row_scale(dp, ones.half())                          # the module draws in its argument's dtype
    torch.manual_seed(11)
    assert torch.equal(half == 0, dp(ones.half())[:, 0] == 0) and half.dtype == torch.float32
    state = torch.get_rng_state()
    assert layers.drop_path_row_scale(dp.eval(), ones) is None
    assert layers.drop_path_row_scale(nn.Identity(), ones) is None
    assert layers.drop_path_row_scale(compat.DropPath(0.0).train(), ones) is None
    assert layers.drop_path_row_scale(compat.DropPath(None).train(), ones) is None
    assert torch.equal(torch.get_rng_state(), state)                            # and nothing is drawn where the module draws nothing


@pytest.mark.parametrize("swin", [False, True])
def test_patched_blocks_on_cpu_tensors_run_the_original_forward(swin):
    cls = swin_standin.SwinTransformerBlock if swin else standin.SwinTransformerBlock
    before = cls.forward
    blocks = O.make_blocks(cls, 3, 24, 0.3, seed=3).train()
    feats = torch.randn(200, 24, generator=torch.Generator().manual_seed(4))
    torch.manual_seed(9)
    want = O.run_blocks(blocks, feats, swin, chained=False)
    state = torch.get_rng_state()
    try:
        done = layers.patch_block_classes(swin_block_cls=cls) if swin else layers.patch_block_classes(cls)
        assert done == [cls] and cls.forward is (layers.swin_fused_block_forward if swin else layers.fused_block_forward)
        torch.manual_seed(9)
        got = O.run_blocks(blocks, feats, swin, chained=True)
        assert torch.equal(got, want) and torch.equal(torch.get_rng_state(), state)
        assert all("_sta_next" not in b.__dict__ and "_sta_norm1" not in b.__dict__ for b in blocks)
        assert set(blocks.state_dict()) == set(O.make_blocks(cls, 3, 24, 0.3, seed=3).state_dict())   # naming a successor registers no submodule
    finally:
        layers.uninstall_fast_layers()
    assert cls.forward is before and not layers._ORIGINAL


def test_nothing_is_patched_by_default():
    assert standin.SwinTransformerBlock.forward is not layers.fused_block_forward
    assert swin_standin.SwinTransformerBlock.forward is not layers.swin_fused_block_forward
    assert not layers._ORIGINAL
