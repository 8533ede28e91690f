"""CPU: the KPConv stem's modules (stratified_transformer_amd.compat.KPConvLayer / FastBatchNorm1d, registered as
torch_points3d.modules.KPConv.kernels.KPConvLayer and torch_points3d.core.common_modules.FastBatchNorm1d): construction, state dict,
the documented kernel-point disposition, unsupported options, the missing CPU path.  No HIP compute runs here."""
import numpy as np
import pytest
import torch

from stratified_transformer_amd import _lib, compat
from tests.kpconv_oracle import influences


@pytest.mark.parametrize("c_in,c_out,add_one", [(3, 48, False), (6, 48, False), (12, 12, False), (3, 48, True)])
def test_kpconv_layer_parameters(c_in, c_out, add_one):
    e = 0.04
    layer = compat.KPConvLayer(c_in, c_out, point_influence=e, add_one=add_one)
    assert tuple(layer.K_points.shape) == (15, 3) and layer.K_points.dtype == torch.float32
    assert tuple(layer.weight.shape) == (15, c_in + (1 if add_one else 0), c_out) and layer.weight.dtype == torch.float32
    assert isinstance(layer.K_points, torch.nn.Parameter) and isinstance(layer.weight, torch.nn.Parameter)
    assert layer.K_points.requires_grad is False and layer.weight.requires_grad is True
    assert list(layer.state_dict().keys()) == ["K_points", "weight"]
    assert layer.point_influence == e and layer.kernel_radius == 1.5 * e
    assert float(layer.weight.detach().abs().max()) > 0  # xavier_normal_, not zeros


def test_kernel_point_disposition():
    e = 0.04 * 1.0
    k = compat.KPConvLayer(3, 48, point_influence=e).K_points.detach()
    assert torch.equal(k[0], torch.zeros(3))
    norms = k[1:].double().norm(dim=1).numpy()
    np.testing.assert_allclose(norms, np.full(14, np.float64(np.float32(e))), rtol=2 ** -22, atol=0)  # a few fp32 roundings
    unit = (k.double() / e).numpy()
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    np.testing.assert_allclose(unit[1:7], np.array(axes, np.float64), atol=1e-6)
    np.testing.assert_allclose(np.abs(unit[7:15]), np.full((8, 3), 3 ** -0.5), atol=1e-6)
    assert len({tuple(np.sign(r).astype(int)) for r in unit[7:15]}) == 8  # all eight corners
    again = compat.KPConvLayer(12, 12, point_influence=e).K_points.detach()
    assert torch.equal(k, again)  # bit-identical from one construction to the next


def test_load_state_dict_replaces_kernel_points():
    a, b = compat.KPConvLayer(3, 8, point_influence=0.04), compat.KPConvLayer(3, 8, point_influence=0.04)
    other = torch.randn(15, 3, generator=torch.Generator().manual_seed(3)) * 0.02
    sd = a.state_dict()
    sd["K_points"] = other.clone()
    b.load_state_dict(sd)
    assert torch.equal(b.K_points.detach(), other) and torch.equal(b.weight.detach(), a.weight.detach())
    assert b.K_points.requires_grad is False


@pytest.mark.parametrize("option,value", [("KP_influence", "gaussian"), ("KP_influence", "constant"), ("aggregation_mode", "closest"),
                                          ("dimension", 2), ("fixed", "verticals"), ("n_kernel_points", 13)])
def test_unsupported_options_raise(option, value):
    with pytest.raises(NotImplementedError, match=option):
        compat.KPConvLayer(3, 8, point_influence=0.04, **{option: value})


def test_cpu_tensors_raise_no_cpu_fallback():
    layer = compat.KPConvLayer(3, 8, point_influence=0.04)
    xyz, x = torch.rand(10, 3), torch.rand(10, 3)
    nb = torch.zeros(10, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(xyz, xyz, nb, x)


def test_registered_modules_are_the_real_ones():
    import stratified_transformer_amd as sta
    sta.install()
    from torch_points3d.core.common_modules import FastBatchNorm1d
    from torch_points3d.modules.KPConv.kernels import KPConvLayer
    import torch_points3d.modules.KPConv.kernels as kernels
    if getattr(kernels, "__stratified_transformer_amd_shim__", False):
        assert KPConvLayer is compat.KPConvLayer and FastBatchNorm1d is compat.FastBatchNorm1d
    layer = KPConvLayer(3, 48, point_influence=0.04, add_one=False)  # the model's call (model/stratified_transformer.py:347)
    assert tuple(layer.weight.shape) == (15, 3, 48)
    assert tuple(FastBatchNorm1d(48, momentum=0.02).batch_norm.weight.shape) == (48,)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", [(50, 12), (4, 50, 12)])
def test_fast_batch_norm_equals_batch_norm(shape, training):
    g = torch.Generator().manual_seed(5)
    fbn, bn = compat.FastBatchNorm1d(12, momentum=0.02), torch.nn.BatchNorm1d(12, momentum=0.02)
    with torch.no_grad():
        fbn.batch_norm.weight.copy_(torch.randn(12, generator=g))
        fbn.batch_norm.bias.copy_(torch.randn(12, generator=g))
        fbn.batch_norm.running_mean.copy_(torch.randn(12, generator=g))
        fbn.batch_norm.running_var.copy_(torch.rand(12, generator=g) + 0.5)
    bn.load_state_dict(fbn.batch_norm.state_dict())
    fbn.train(training), bn.train(training)
    x = torch.randn(*shape, generator=g)
    got = fbn(x)
    want = bn(x) if x.dim() == 2 else bn(x.transpose(1, 2)).transpose(1, 2)
    assert got.shape == x.shape and torch.equal(got, want)
    assert torch.equal(fbn.batch_norm.running_mean, bn.running_mean) and torch.equal(fbn.batch_norm.running_var, bn.running_var)
    assert int(fbn.batch_norm.num_batches_tracked) == int(bn.num_batches_tracked) == (1 if training else 0)


def test_fast_batch_norm_rank_and_state_dict():
    fbn = compat.FastBatchNorm1d(12, momentum=0.02)
    assert fbn.batch_norm.momentum == 0.02
    assert list(fbn.state_dict().keys()) == ["batch_norm.weight", "batch_norm.bias", "batch_norm.running_mean", "batch_norm.running_var",
                                             "batch_norm.num_batches_tracked"]
    with pytest.raises(ValueError):
        fbn(torch.zeros(2, 3, 12, 4))
    with pytest.raises(ValueError):
        fbn(torch.zeros(12))


def test_disposition_reach_is_two_influences():
    """Every kernel point lies within point_influence of the origin and its influence ends at point_influence, so a neighbour at
    2.5 * point_influence (the stem's search radius, train_backup.py:362) or beyond has no influence at all; one at the centre has
    influence 1 on kernel point 0 and (to rounding) none on the others."""
    e = 0.04
    k = compat.KPConvLayer(3, 8, point_influence=e).K_points.detach()
    rng = np.random.default_rng(2)
    d = rng.standard_normal((200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([np.full(100, 2.5 * e), 2.5 * e * (1 + rng.random(100))])
    support = torch.from_numpy(np.concatenate([np.zeros((1, 3)), d * r[:, None] * (1 + 1e-9)]))
    query = torch.zeros(1, 3, dtype=torch.float64)
    nb = torch.arange(201)[None, :]
    w, _ = influences(query, support, nb, k, e)
    assert w.shape == (1, 15, 201)
    assert float(w[0, 0, 0]) == 1.0 and float(w[0, 1:, 0].abs().max()) < 1e-6
    assert float(w[0, :, 1:].abs().max()) == 0.0


def test_kpconv_launchers_are_declared():
    I, P, F = _lib.I, _lib.P, _lib.F
    assert _lib.SIGNATURES["kpconv_aggregate_forward_launcher"] == [I] * 5 + [P] * 5 + [F, P]
    assert _lib.SIGNATURES["kpconv_aggregate_backward_launcher"] == [I] * 5 + [P] * 4 + [F, P, P]
