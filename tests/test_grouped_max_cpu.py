"""CPU: the grouped maximum's declarations (C ABI table, signatures, argument checks, the missing CPU path) and its float64 oracle
(tests/grouped_max_oracle.py) against nn.MaxPool1d and against the per-group composite of TransitionDown.  No HIP compute runs here."""
import inspect

import numpy as np
import pytest
import torch

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, layers, pointops, pointops2_cuda
from tests import grouped_max_oracle as O


def test_launchers_are_declared_and_exported():
    I, P = _lib.I, _lib.P
    assert _lib.SIGNATURES["grouped_max_forward_launcher"] == [I] * 5 + [P] * 4
    assert _lib.SIGNATURES["grouped_max_backward_launcher"] == [I] * 5 + [P] * 5


def test_public_signatures():
    assert str(inspect.signature(pointops.grouped_max)) == "(feat, idx)"
    assert str(inspect.signature(sta.install)) == "(third_party=True, fast_layers=False, pooled_transition=False)"
    assert issubclass(pointops.GroupedMax, torch.autograd.Function)
    from lib.pointops2.functions import pointops as drop_in
    assert drop_in.grouped_max is pointops.grouped_max


def test_install_sets_the_flag_and_the_default_is_off():
    assert layers.POOLED_TRANSITION is False
    try:
        sta.install(pooled_transition=True)
        assert layers.POOLED_TRANSITION is True
        sta.install()
        assert layers.POOLED_TRANSITION is False
        sta.install(True, False)  # positional use as before
        assert layers.POOLED_TRANSITION is False
    finally:
        layers.POOLED_TRANSITION = False


def test_cpu_tensors_raise_no_cpu_fallback():
    feat, idx = torch.rand(10, 8), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops.grouped_max(feat, idx)
    out, arg = torch.empty(4, 8), torch.empty(4, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.grouped_max_forward(4, 10, 3, 8, feat, idx.int(), out, arg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.grouped_max_backward(4, 10, 3, 8, out, arg, torch.zeros(11, dtype=torch.int32), torch.zeros(12, dtype=torch.int32), torch.empty(10, 8))


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


@pytest.mark.parametrize("feat,idx,error", [
    (torch.rand(10), torch.zeros(4, 3, dtype=torch.int32), ValueError),                       # feat not [n_s, c]
    (torch.rand(10, 8).double(), torch.zeros(4, 3, dtype=torch.int32), TypeError),            # feat dtype
    (torch.rand(10, 8), torch.zeros(4, 3, dtype=torch.int16), ValueError),                    # idx dtype
    (torch.rand(10, 8), torch.zeros(12, dtype=torch.int32), ValueError),                      # idx not [m, k]
    (torch.rand(10, 8), torch.zeros(4, 65, dtype=torch.int32), ValueError),                   # k > 64
    (torch.rand(10, 8), torch.zeros(4, 0, dtype=torch.int32), ValueError),                    # k < 1
    (torch.rand(10, 1025), torch.zeros(4, 3, dtype=torch.int32), ValueError),                 # c > 1024
])
def test_operator_rejects_bad_arguments(feat, idx, error):
    with pytest.raises(error, match="grouped_max"):
        pointops.grouped_max(_OnGpu(feat), _OnGpu(idx))


def test_binding_rejects_bad_shapes_and_dtypes():
    C = pointops2_cuda
    f32 = lambda *s: _OnGpu(torch.zeros(*s))
    i32 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.int32))
    u8 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.uint8))
    with pytest.raises(ValueError, match="feat"):
        C.grouped_max_forward(4, 10, 3, 8, f32(9, 8), i32(4, 3), f32(4, 8), u8(4, 8))
    with pytest.raises(ValueError, match="idx"):
        C.grouped_max_forward(4, 10, 3, 8, f32(10, 8), i32(4, 4), f32(4, 8), u8(4, 8))
    with pytest.raises(ValueError, match="out"):
        C.grouped_max_forward(4, 10, 3, 8, f32(10, 8), i32(4, 3), f32(5, 8), u8(4, 8))
    with pytest.raises(ValueError, match="arg"):
        C.grouped_max_forward(4, 10, 3, 8, f32(10, 8), i32(4, 3), f32(4, 8), u8(4, 7))
    with pytest.raises(TypeError, match="arg"):
        C.grouped_max_forward(4, 10, 3, 8, f32(10, 8), i32(4, 3), f32(4, 8), i32(4, 8))
    with pytest.raises(TypeError, match="idx"):
        C.grouped_max_forward(4, 10, 3, 8, f32(10, 8), _OnGpu(torch.zeros(4, 3, dtype=torch.int64)), f32(4, 8), u8(4, 8))
    with pytest.raises(TypeError, match="out"):
        C.grouped_max_forward(4, 10, 3, 8, f32(10, 8), i32(4, 3), _OnGpu(torch.zeros(4, 8, dtype=torch.float16)), u8(4, 8))
    with pytest.raises(TypeError, match="feat"):
        C.grouped_max_forward(4, 10, 3, 8, _OnGpu(torch.zeros(10, 8, dtype=torch.float64)), i32(4, 3), f32(4, 8), u8(4, 8))
    with pytest.raises(RuntimeError, match="contiguous"):
        C.grouped_max_forward(4, 10, 3, 8, _OnGpu(torch.zeros(8, 10).t()), i32(4, 3), f32(4, 8), u8(4, 8))
    with pytest.raises(ValueError, match="src_offsets"):
        C.grouped_max_backward(4, 10, 3, 8, f32(4, 8), u8(4, 8), i32(10), i32(12), f32(10, 8))
    with pytest.raises(ValueError, match="src_pair"):
        C.grouped_max_backward(4, 10, 3, 8, f32(4, 8), u8(4, 8), i32(11), i32(13), f32(10, 8))
    with pytest.raises(ValueError, match="grad_feat"):
        C.grouped_max_backward(4, 10, 3, 8, f32(4, 8), u8(4, 8), i32(11), i32(12), f32(11, 8))
    with pytest.raises(TypeError, match="grad_feat"):
        C.grouped_max_backward(4, 10, 3, 8, f32(4, 8), u8(4, 8), i32(11), i32(12), _OnGpu(torch.zeros(10, 8, dtype=torch.bfloat16)))


def _tied_problem(seed, n_s, m, k, c, levels=5):
    """values on a coarse grid (exact ties are common) and index rows with duplicates"""
    rng = np.random.default_rng(seed)
    feat = rng.integers(-levels, levels + 1, (n_s, c)).astype(np.float64) / 4
    idx = rng.integers(0, n_s, (m, k))
    idx[::3, k // 2:] = idx[::3, :1]  # duplicate rows, as the kNN returns for a batch element with fewer than k points
    return feat, idx


@pytest.mark.parametrize("k,c,n_s", [(1, 3, 1), (3, 5, 7), (16, 24, 200), (34, 7, 50), (64, 9, 40)])
def test_oracle_forward_is_max_pool1d_with_its_tie_rule(k, c, n_s):
    feat, idx = _tied_problem(k, n_s, 60, k, c)
    out, arg = O.forward(feat, idx)
    gathered = torch.from_numpy(feat)[torch.from_numpy(idx)]                     # [m, k, c]
    want, where = torch.nn.MaxPool1d(k, return_indices=True)(gathered.transpose(1, 2).contiguous())
    assert np.array_equal(out, want.squeeze(-1).numpy())
    assert np.array_equal(arg.astype(np.int64), where.squeeze(-1).numpy())
    if k >= 3:
        assert float((np.sort(gathered.numpy(), 1)[:, -1] == np.sort(gathered.numpy(), 1)[:, -2]).mean()) > 0.2  # ties ARE common here


def test_oracle_forward_nan_and_skip_rules():
    feat = np.array([[1.0, -np.inf], [np.nan, 2.0], [3.0, np.inf], [np.nan, -1.0]])
    idx = np.array([[0, 1, 2, 3],      # NaN wins over a later larger value; arg = the first NaN
                    [2, -1, 4, 0],     # -1 and n_s are skipped
                    [-1, 4, 99, -7],   # no valid entry
                    [0, 0, 0, 0]])     # all equal: the first
    out, arg = O.forward(feat, idx)
    assert np.isnan(out[0, 0]) and arg[0, 0] == 1 and out[0, 1] == np.inf and arg[0, 1] == 2
    assert out[1].tolist() == [3.0, np.inf] and arg[1].tolist() == [0, 0]
    assert out[2].tolist() == [0.0, 0.0] and arg[2].tolist() == [O.NO_ARG, O.NO_ARG]
    assert out[3].tolist() == [1.0, -np.inf] and arg[3].tolist() == [0, 0]
    want = torch.nn.functional.max_pool1d(torch.from_numpy(feat)[torch.from_numpy(idx[:1])].transpose(1, 2).contiguous(), 4).squeeze(-1)
    assert np.array_equal(out[:1], want.numpy(), equal_nan=True)                 # max_pool1d propagates the NaN too
    grad, terms, abs_sum = O.backward(np.ones((4, 2)), idx, arg, 4)
    assert grad[:, 0].tolist() == [1.0, 1.0, 1.0, 0.0] and grad[:, 1].tolist() == [1.0, 0.0, 2.0, 0.0]
    assert terms[2, 1] == 2 and abs_sum[2, 1] == 2.0 and terms.sum() == 6     # the all-invalid row carries no gradient


def test_oracle_backward_is_autograd_of_the_gathered_maximum():
    feat, idx = _tied_problem(3, 30, 50, 8, 6, levels=1000)                      # fine grid: no ties, autograd's choice is unambiguous
    feat += np.random.default_rng(4).random(feat.shape) * 1e-3
    _, arg = O.forward(feat, idx)
    go = np.random.default_rng(5).standard_normal((50, 6))
    x = torch.from_numpy(feat).requires_grad_(True)
    (x[torch.from_numpy(idx)].max(dim=1).values * torch.from_numpy(go)).sum().backward()
    grad, terms, abs_sum = O.backward(go, idx, arg, 30)
    np.testing.assert_allclose(grad, x.grad.numpy(), rtol=0, atol=1e-12)
    assert int(terms.sum()) == 50 * 6 and np.all(abs_sum >= np.abs(grad) - 1e-12)


@pytest.mark.parametrize("c_in,c_out", [(48, 96), (192, 384)])
def test_per_source_formulation_equals_the_per_group_composite(c_in, c_out):
    """the identity the feature rests on: LayerNorm and a bias-free Linear act row by row, so they commute with the gather"""
    g = torch.Generator().manual_seed(c_in)
    n, m, k = 600, 150, 16
    feats = torch.randn(n, c_in, generator=g, dtype=torch.float64)
    knn = torch.randint(0, n, (m, k), generator=g)
    lin = torch.nn.Linear(c_in, c_out, bias=False).double()
    nw, nb = torch.randn(c_in, generator=g, dtype=torch.float64), torch.randn(c_in, generator=g, dtype=torch.float64)
    go = torch.randn(m, c_out, generator=g, dtype=torch.float64)
    grads = {}
    for name, fn in (("source", lambda *a: O.per_source(*a)[0]), ("group", O.composite)):
        leaves = [t.clone().requires_grad_(True) for t in (feats, nw, nb, lin.weight.detach())]
        out = fn(leaves[0], knn, leaves[1], leaves[2], leaves[3])
        (out * go).sum().backward()
        grads[name] = [out.detach()] + [t.grad for t in leaves]
    for a, b in zip(grads["source"], grads["group"]):
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 1e-12 * scale
    # and the oracle's forward on y is that pooled tensor
    pooled, y = O.per_source(feats, knn, nw, nb, lin.weight.detach())
    out, _ = O.forward(y.numpy(), knn.numpy())
    assert np.array_equal(out, pooled.numpy())
    assert float((O.composite(feats, knn, None, None, lin.weight.detach()) - O.per_source(feats, knn, None, None, lin.weight.detach())[0]).abs().max()) <= 1e-12
