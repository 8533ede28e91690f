"""GPU (-m gpu): the KPConv stem on the HIP aggregation kernels (csrc/kpconv.hip): the C-ABI launchers kpconv_aggregate_{forward,
backward}_launcher, pointops.kpconv, compat.KPConvLayer.forward and the stem blocks as the model composes them
(model/stratified_transformer.py:344-392), against the float64 oracle of tests/kpconv_oracle.py evaluated on the CPU.

The bars are the cell attention's (tests/test_cell_qkv_hip.py): forward rtol 2e-5 / atol 1e-4, gradient of x rtol 2e-5 / atol 2e-4,
gradient of weight (and of every other parameter) over max(1, |want|.max()) rtol 2e-4 / atol 2e-4.  The fp32 torch evaluation of the
same formulas sits two orders inside each (forward <= 6e-7 on values <= 3, grad x <= 8e-7, grad weight <= 6e-5 on values <= 140).
"""
import copy

import numpy as np
import pytest
import torch

from stratified_transformer_amd import scene
from tests.kpconv_oracle import kpconv_oracle
from tests.util import dev

pytestmark = pytest.mark.gpu

FTOL = dict(rtol=2e-5, atol=1e-4)
GTOL = dict(rtol=2e-5, atol=2e-4)
TTOL = dict(rtol=2e-4, atol=2e-4)
GRID = 0.04  # prev_grid_size of both shipped configurations; sigma = 1: point_influence = 0.04, search radius 2.5 * 0.04


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


def _np(t):
    return t.detach().float().cpu().numpy()


def _scaled(got, want, what):
    s = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(got / s, want / s, err_msg=what, **TTOL)


_SCENES = {}


def _scene(P, sizes, seed, max_num=34):
    """surface rooms at GRID, neighbours of the stem's ball query: xyz [n,3] f32 (numpy), neighbours [n, max_num] int32 (GPU)"""
    key = (tuple(sizes), seed, max_num)
    if key not in _SCENES:
        xyz, offset = scene.make_batch(list(sizes), seed=seed)
        nb, _ = P.ball_query(2.5 * GRID, max_num, dev(xyz), dev(xyz), dev(offset), dev(offset))
        _SCENES[key] = (xyz, nb.contiguous())
    return _SCENES[key]


def _operands(n_s, c, out, seed, n_q=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_s, c), dtype=np.float32)
    weight = rng.standard_normal((15, c, out), dtype=np.float32) * np.float32((2.0 / (15 * (c + out))) ** 0.5 * 4)
    go = rng.standard_normal((n_q if n_q is not None else n_s, out), dtype=np.float32)
    return x, weight, go


def _k_points(e=GRID):
    from stratified_transformer_amd.compat import kpconv_kernel_points
    return kpconv_kernel_points(e)


def _oracle(query, support, nb, x, kp, weight, e, go, add_one=False):
    """float64 on the CPU: out, grad x, grad weight (numpy)"""
    x64 = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    w64 = torch.from_numpy(np.asarray(weight, np.float64)).requires_grad_(True)
    out = kpconv_oracle(torch.from_numpy(query), torch.from_numpy(support), nb.cpu(), x64, kp, w64, e, add_one=add_one)
    (out * torch.from_numpy(np.asarray(go, np.float64))).sum().backward()
    return out.detach().numpy(), x64.grad.numpy(), w64.grad.numpy()


def _check_op(P, query, support, nb, x, weight, go, e=GRID, kp=None, what=""):
    """pointops.kpconv forward and backward against the oracle; returns the GPU output"""
    kp = _k_points(e) if kp is None else kp
    xg, wg = dev(x).requires_grad_(True), dev(weight).requires_grad_(True)
    out = P.kpconv(dev(query), dev(support), nb, xg, kp.cuda(), wg, e)
    assert out.dtype == torch.float32 and tuple(out.shape) == (query.shape[0], weight.shape[2])
    out.backward(dev(go))
    torch.cuda.synchronize()
    want, want_gx, want_gw = _oracle(query, support, nb, x, kp, weight, e, go)
    np.testing.assert_allclose(_np(out), want, err_msg=f"{what} forward", **FTOL)
    np.testing.assert_allclose(_np(xg.grad), want_gx, err_msg=f"{what} grad x", **GTOL)
    _scaled(_np(wg.grad), want_gw, f"{what} grad weight")
    return out


BIG = ((12000, 9000), 71)  # 21 000 points, two batch elements


@pytest.mark.parametrize("c,out", [(3, 48), (6, 48), (12, 12)])
def test_launchers_against_the_oracle(P, c, out):
    """wf [n, 15, c] of the forward launcher and grad_feat of the backward launcher (for a random grad_wf)"""
    from stratified_transformer_amd import pointops2_cuda as C
    xyz, nb = _scene(P, *BIG)
    n = xyz.shape[0]
    valid = (nb >= 0).sum(1)
    assert n >= 20000 and float(valid.float().mean()) > 15 and int(valid.min()) < 34  # a real neighbourhood, and padded rows
    x, weight, _ = _operands(n, c, out, seed=c)
    kp = _k_points()
    xyz_g, x_g, kp_g = dev(xyz), dev(x), kp.cuda()
    wf = torch.full((n, 15, c), float("nan"), device="cuda")
    C.kpconv_aggregate_forward(n, n, 34, c, 15, xyz_g, xyz_g, nb, x_g, kp_g, GRID, wf)
    x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    _, want_wf = kpconv_oracle(torch.from_numpy(xyz), torch.from_numpy(xyz), nb.cpu(), x64, kp, torch.from_numpy(weight), GRID, return_wf=True)
    np.testing.assert_allclose(_np(wf), want_wf.detach().numpy(), **FTOL)
    g_wf = np.random.default_rng(9).standard_normal((n, 15, c), dtype=np.float32)
    g_feat = torch.zeros(n, c, device="cuda")
    C.kpconv_aggregate_backward(n, n, 34, c, 15, xyz_g, xyz_g, nb, kp_g, GRID, dev(g_wf), g_feat)
    (want_wf * torch.from_numpy(g_wf.astype(np.float64))).sum().backward()
    np.testing.assert_allclose(_np(g_feat), x64.grad.numpy(), **GTOL)


@pytest.mark.parametrize("c,out", [(3, 48), (6, 48), (12, 12)])
def test_operator_against_the_oracle(P, c, out):
    xyz, nb = _scene(P, *BIG)
    x, weight, go = _operands(xyz.shape[0], c, out, seed=10 + c)
    _check_op(P, xyz, xyz, nb, x, weight, go, what=f"kpconv {c}->{out}")


@pytest.mark.parametrize("c,out,add_one", [(3, 48, False), (6, 48, False), (12, 12, False), (3, 48, True)])
def test_layer_against_the_oracle(P, c, out, add_one):
    from stratified_transformer_amd.compat import KPConvLayer
    xyz, nb = _scene(P, *BIG)
    n = xyz.shape[0]
    x, _, go = _operands(n, c, out, seed=20 + c)
    torch.manual_seed(c)
    layer = KPConvLayer(c, out, point_influence=GRID * 1.0, add_one=add_one).cuda()
    xg = dev(x).requires_grad_(True)
    got = layer(dev(xyz), dev(xyz), nb.long(), xg)   # the model passes int64 neighbours
    got.backward(dev(go))
    x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    w64 = layer.weight.detach().cpu().double().requires_grad_(True)
    want = kpconv_oracle(torch.from_numpy(xyz), torch.from_numpy(xyz), nb.cpu(), x64, layer.K_points.detach().cpu(), w64, GRID, add_one=add_one)
    (want * torch.from_numpy(go.astype(np.float64))).sum().backward()
    np.testing.assert_allclose(_np(got), want.detach().numpy(), **FTOL)
    np.testing.assert_allclose(_np(xg.grad), x64.grad.numpy(), **GTOL)
    _scaled(_np(layer.weight.grad), w64.grad.numpy(), "grad weight")
    assert layer.K_points.grad is None


SMALL = ((2500, 1500), 61)


def test_padding_rows_self_rows_and_shadow_index(P):
    """rows of all -1 give exactly 0; a row whose only neighbour is the point itself; index n_s is padding like -1"""
    xyz, nb = _scene(P, *SMALL)
    n = xyz.shape[0]
    nb = nb.clone()
    nb[5:40] = -1
    nb[100:130, 1:] = -1
    assert bool((nb[100:130, 0] == torch.arange(100, 130, device="cuda")).all())
    x, weight, go = _operands(n, 6, 48, seed=31)
    out = _check_op(P, xyz, xyz, nb, x, weight, go, what="edges")
    assert float(out.detach()[5:40].abs().max()) == 0.0
    # only itself: influence 1 on kernel point 0 and (to rounding) none on the others
    np.testing.assert_allclose(_np(out[100:130]), x[100:130].astype(np.float64) @ weight[0].astype(np.float64), **FTOL)
    shadow = torch.where(nb < 0, torch.full_like(nb, n), nb)
    out2 = P.kpconv(dev(xyz), dev(xyz), shadow, dev(x), _k_points().cuda(), dev(weight), GRID)
    assert torch.equal(out2, out.detach())


def test_int64_neighbours_and_subset_queries(P):
    """n_q != n_s: the queries are every third point, their neighbours searched among all points; int64 equals int32"""
    xyz, offset = scene.make_batch([2500, 1500], seed=62)
    q = np.ascontiguousarray(xyz[::3])
    q_off = np.array([len(range(0, 2500, 3)), q.shape[0]], np.int32)
    nb, _ = P.ball_query(2.5 * GRID, 34, dev(xyz), dev(q), dev(offset), dev(q_off))
    assert q.shape[0] != xyz.shape[0] and tuple(nb.shape) == (q.shape[0], 34)
    x, weight, go = _operands(xyz.shape[0], 12, 12, seed=32, n_q=q.shape[0])
    out = _check_op(P, q, xyz, nb.contiguous(), x, weight, go, what="subset")
    out64 = P.kpconv(dev(q), dev(xyz), nb.long(), dev(x), _k_points().cuda(), dev(weight), GRID)
    assert torch.equal(out64, out.detach())


@pytest.mark.parametrize("n_nb", [1, 16, 40])
def test_neighbour_counts(P, n_nb):
    xyz, nb = _scene(P, (3000,), 63, max_num=n_nb)
    x, weight, go = _operands(xyz.shape[0], 3, 48, seed=33)
    _check_op(P, xyz, xyz, nb, x, weight, go, what=f"n_nb={n_nb}")


@pytest.mark.parametrize("c", [1, 64])
def test_channel_extremes(P, c):
    xyz, nb = _scene(P, (3000,), 63)
    x, weight, go = _operands(xyz.shape[0], c, 16, seed=34)
    _check_op(P, xyz, xyz, nb, x, weight, go, what=f"c={c}")


def test_empty_cloud(P):
    from stratified_transformer_amd import _lib
    f = dict(device="cuda", dtype=torch.float32)
    x = torch.zeros(0, 3, **f).requires_grad_(True)
    weight = torch.randn(15, 3, 48, **f).requires_grad_(True)
    before = _lib.CALLS[0]
    out = P.kpconv(torch.zeros(0, 3, **f), torch.zeros(0, 3, **f), torch.zeros(0, 34, dtype=torch.int32, device="cuda"), x, _k_points().cuda(), weight, GRID)
    assert tuple(out.shape) == (0, 48) and out.dtype == torch.float32
    out.sum().backward()
    assert _lib.CALLS[0] == before  # nothing was launched
    assert tuple(x.grad.shape) == (0, 3) and float(weight.grad.abs().max()) == 0.0


def test_out_of_range_arguments_are_recorded_errors(P):
    """c, n_nb, n_kp outside the supported ranges: an error, and no launch (the output keeps its sentinel)"""
    from stratified_transformer_amd import pointops2_cuda as C
    n = 64
    f = dict(device="cuda", dtype=torch.float32)
    xyz = torch.rand(n, 3, **f)
    for c, n_nb, n_kp, word in ((65, 34, 15, "c must"), (0, 34, 15, "c must"), (3, 65, 15, "n_nb must"), (3, 0, 15, "n_nb must"),
                                (3, 34, 33, "n_kp must"), (3, 34, 0, "n_kp must")):
        nb = torch.zeros(n, max(n_nb, 1), dtype=torch.int32, device="cuda")
        feat, kp = torch.rand(n, max(c, 1), **f), torch.rand(max(n_kp, 1), 3, **f)
        wf = torch.full((n, max(n_kp, 1), max(c, 1)), 7.0, **f)
        with pytest.raises(RuntimeError, match=word):
            C.kpconv_aggregate_forward(n, n, n_nb, c, n_kp, xyz, xyz, nb, feat, kp, GRID, wf)
        g = torch.full((n, max(c, 1)), 7.0, **f)
        with pytest.raises(RuntimeError, match=word):
            C.kpconv_aggregate_backward(n, n, n_nb, c, n_kp, xyz, xyz, nb, kp, GRID, wf, g)
        torch.cuda.synchronize()
        assert float(wf.min()) == 7.0 == float(wf.max()) and float(g.min()) == 7.0 == float(g.max())
    with pytest.raises(RuntimeError, match="extent"):
        C.kpconv_aggregate_forward(n, n, 4, 3, 15, xyz, xyz, torch.zeros(n, 4, dtype=torch.int32, device="cuda"), torch.rand(n, 3, **f),
                                   torch.rand(15, 3, **f), 0.0, torch.zeros(n, 15, 3, **f))
    with pytest.raises(RuntimeError, match="c must"):   # and through the operator
        P.kpconv(xyz, xyz, torch.zeros(n, 4, dtype=torch.int32, device="cuda"), torch.rand(n, 65, **f), torch.rand(15, 3, **f), torch.rand(15, 65, 8, **f), GRID)
    with pytest.raises(ValueError):
        P.kpconv(xyz, xyz, torch.zeros(n + 1, 4, dtype=torch.int32, device="cuda"), torch.rand(n, 3, **f), torch.rand(15, 3, **f), torch.rand(15, 3, 8, **f), GRID)


def test_forward_is_bitwise_reproducible(P):
    xyz, nb = _scene(P, *BIG)
    x, weight, _ = _operands(xyz.shape[0], 12, 12, seed=35)
    args = (dev(xyz), dev(xyz), nb, dev(x), _k_points().cuda(), dev(weight), GRID)
    a = P.kpconv(*args)
    b = P.kpconv(*args)
    assert torch.equal(a, b)


def test_input_without_gradient_launches_no_backward_kernel(P):
    """the model's first block: x is data.  The weight gradient is right and the backward makes no library launch (so no
    grad_feat buffer is written)."""
    from stratified_transformer_amd import _lib
    xyz, nb = _scene(P, *SMALL)
    x, weight, go = _operands(xyz.shape[0], 3, 48, seed=36)
    xg, wg = dev(x), dev(weight).requires_grad_(True)
    out = P.kpconv(dev(xyz), dev(xyz), nb, xg, _k_points().cuda(), wg, GRID)
    before = _lib.CALLS[0]
    out.backward(dev(go))
    torch.cuda.synchronize()
    assert _lib.CALLS[0] == before and xg.grad is None
    want, _, want_gw = _oracle(xyz, xyz, nb, x, _k_points(), weight, GRID, go)
    np.testing.assert_allclose(_np(out), want, **FTOL)
    _scaled(_np(wg.grad), want_gw, "grad weight")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_rows_under_autocast(P, dtype):
    """a half x (what a preceding Linear yields under autocast): the rows are widened exactly, arithmetic and result are fp32 - equal
    to the fp32 run on the widened rows, bit for bit in the forward (no atomics) - and the gradient comes back in x's dtype, within
    one unit of that format's last place (2^-10 f16, 2^-7 bf16) of the rounded fp32 gradient."""
    xyz, nb = _scene(P, *SMALL)
    x, weight, go = _operands(xyz.shape[0], 12, 12, seed=37)
    kp = _k_points().cuda()
    xh = dev(x).to(dtype).requires_grad_(True)
    wh = dev(weight).requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        out = P.kpconv(dev(xyz), dev(xyz), nb, xh, kp, wh, GRID)
    assert out.dtype == torch.float32
    out.backward(dev(go))
    xw = xh.detach().float().requires_grad_(True)
    ww = dev(weight).requires_grad_(True)
    ref = P.kpconv(dev(xyz), dev(xyz), nb, xw, kp, ww, GRID)
    ref.backward(dev(go))
    assert torch.equal(out, ref)
    assert xh.grad.dtype == dtype and wh.grad.dtype == torch.float32
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    np.testing.assert_allclose(_np(xh.grad), _np(xw.grad), rtol=ulp, atol=1e-5)
    assert torch.equal(wh.grad, ww.grad)
    # and against the oracle on the widened rows
    want, _, _ = _oracle(xyz, xyz, nb, _np(xw), _k_points(), weight, GRID, go)
    np.testing.assert_allclose(_np(out), want, **FTOL)


def test_coordinate_gradient_raises(P):
    xyz, nb = _scene(P, *SMALL)
    x, weight, go = _operands(xyz.shape[0], 3, 48, seed=38)
    for which in ("query", "support", "k_points"):
        q, s, kp = dev(xyz), dev(xyz), _k_points().cuda()
        if which == "query":
            q.requires_grad_(True)
        elif which == "support":
            s.requires_grad_(True)
        else:
            kp.requires_grad_(True)
        out = P.kpconv(q, s, nb, dev(x), kp, dev(weight).requires_grad_(True), GRID)
        with pytest.raises(RuntimeError, match="not implemented"):
            out.backward(dev(go))


# ---- the stem as the model composes it (model/stratified_transformer.py:344-392, 406-417) ----
class _Simple(torch.nn.Module):
    """KPConvSimpleBlock (:344-359)"""

    def __init__(self, c_in, c_out):
        super().__init__()
        from stratified_transformer_amd.compat import FastBatchNorm1d, KPConvLayer
        self.kpconv = KPConvLayer(c_in, c_out, point_influence=GRID * 1.0, add_one=False)
        self.bn = FastBatchNorm1d(c_out, momentum=0.02)
        self.activation = torch.nn.LeakyReLU(negative_slope=0.2)

    def forward(self, feats, xyz, nb, conv):
        return self.activation(self.bn(conv(self.kpconv, xyz, nb, feats)))


class _Res(torch.nn.Module):
    """KPConvResBlock (:362-392) with in_channels == out_channels (the model's use, :414): the shortcut is the identity"""

    def __init__(self, c):
        super().__init__()
        from stratified_transformer_amd.compat import FastBatchNorm1d, KPConvLayer
        d_2 = c // 4
        act = torch.nn.LeakyReLU(negative_slope=0.2)
        self.unary_1 = torch.nn.Sequential(torch.nn.Linear(c, d_2, bias=False), FastBatchNorm1d(d_2, momentum=0.02), act)
        self.unary_2 = torch.nn.Sequential(torch.nn.Linear(d_2, c, bias=False), FastBatchNorm1d(c, momentum=0.02), act)
        self.kpconv = KPConvLayer(d_2, d_2, point_influence=GRID * 1.0, add_one=False)

    def forward(self, feats, xyz, nb, conv):
        shortcut = feats
        feats = self.unary_1(feats)
        feats = conv(self.kpconv, xyz, nb, feats)
        feats = self.unary_2(feats)
        feats += shortcut
        return feats


def _conv_hip(layer, xyz, nb, feats):
    return layer(xyz, xyz, nb, feats)


def _conv_oracle(layer, xyz, nb, feats):
    return kpconv_oracle(xyz, xyz, nb, feats, layer.K_points.detach(), layer.weight, layer.point_influence)


def test_stem_blocks_train_mode(P):
    """KPConvSimpleBlock(3 -> 48) then KPConvResBlock(48 -> 48, d_2 = 12), train mode (batch statistics), forward and backward,
    against the same modules in float64 on the CPU with the oracle convolution"""
    xyz, nb = _scene(P, *BIG)
    n = xyz.shape[0]
    torch.manual_seed(4)
    stem = torch.nn.ModuleList([_Simple(3, 48), _Res(48)])
    rng = np.random.default_rng(40)
    with torch.no_grad():  # affine parameters away from their (1, 0) defaults, so their gradients are exercised
        for m in stem.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.from_numpy(1 + 0.2 * rng.standard_normal(m.weight.shape[0]).astype(np.float32)))
                m.bias.copy_(torch.from_numpy(0.2 * rng.standard_normal(m.bias.shape[0]).astype(np.float32)))
    want_stem = copy.deepcopy(stem).double()
    stem = stem.cuda().train()
    want_stem.train()
    feats = rng.random((n, 3), dtype=np.float32)
    go = rng.standard_normal((n, 48), dtype=np.float32)

    got = dev(feats)
    for block in stem:
        got = block(got, dev(xyz), nb.long(), _conv_hip)
    got.backward(dev(go))
    torch.cuda.synchronize()
    want = torch.from_numpy(feats.astype(np.float64))
    for block in want_stem:
        want = block(want, torch.from_numpy(xyz).double(), nb.cpu(), _conv_oracle)
    (want * torch.from_numpy(go.astype(np.float64))).sum().backward()

    np.testing.assert_allclose(_np(got), want.detach().numpy(), **FTOL)
    got_params, want_params = dict(stem.named_parameters()), dict(want_stem.named_parameters())
    assert set(got_params) == set(want_params) and len(got_params) == 12
    for name, p in want_params.items():
        if name.endswith("K_points"):
            assert p.grad is None and got_params[name].grad is None
            continue
        _scaled(_np(got_params[name].grad), p.grad.numpy(), f"grad {name}")
    for (name, b), (_, wb) in zip(stem.named_buffers(), want_stem.named_buffers()):
        if name.endswith("running_mean") or name.endswith("running_var"):
            np.testing.assert_allclose(_np(b), wb.numpy(), err_msg=name, **FTOL)
