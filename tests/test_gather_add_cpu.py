"""CPU: the gather-add's declarations (C ABI table, signatures, argument checks, the missing CPU path, the decoder's installer) and its
fp32 oracle (tests/gather_add_oracle.py) against the reference's own interpolation term (tests/golden/upsample_reference.npz) and
against float64 autograd.  No HIP compute runs here."""
import inspect
import os

import numpy as np
import pytest
import torch

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, layers, pointops, pointops2_cuda
from tests import decoder_standin
from tests import gather_add_cases as cases
from tests import gather_add_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upsample_reference.npz")
EPS = float(np.finfo(np.float32).eps)


def test_launchers_are_declared_and_exported():
    I, P = _lib.I, _lib.P
    assert _lib.SIGNATURES["gather_add_forward_launcher"] == [I] * 6 + [P] * 5
    assert _lib.SIGNATURES["gather_add_backward_launcher"] == [I] * 5 + [P] * 5


def test_public_signatures():
    assert str(inspect.signature(pointops.gather_add)) == "(feat, idx, weight, base=None)"
    assert str(inspect.signature(pointops.interpolate_add)) == "(xyz, new_xyz, feat, offset, new_offset, base=None, k=3)"
    assert str(inspect.signature(layers.upsample_forward)) == str(inspect.signature(decoder_standin.Upsample.forward))
    assert issubclass(pointops.GatherAdd, torch.autograd.Function)
    assert sta.install_fast_decoder is layers.install_fast_decoder and "install_fast_decoder" in sta.__all__
    from lib.pointops2.functions import pointops as drop_in
    assert drop_in.gather_add is pointops.gather_add


def test_golden_holds_arrays_only_and_the_stated_sizes():
    g = np.load(GOLDEN, allow_pickle=False)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert g["xyz"].shape == (64, 3) and g["support_xyz"].shape == (257, 3) and list(g["config"]) == [3, 32, 16]
    assert g["feats"].shape == g["grad_feats"].shape == (64, 32) and g["support_feats"].shape == g["grad_support_feats"].shape == (257, 16)
    assert g["out"].shape == g["grad_out"].shape == g["interpolated"].shape == (257, 16)
    assert g["knn_idx"].shape == g["knn_weight"].shape == (257, 3) and list(g["offset"]) == [30, 64] and list(g["support_offset"]) == [120, 257]
    keys = sorted(k[6:] for k in g.files if k.startswith("param."))
    assert keys == sorted(decoder_standin.Upsample(3, 32, 16).state_dict()) == sorted(k[5:] for k in g.files if k.startswith("grad."))


def test_oracle_reproduces_the_reference_interpolation_term():
    """The reference's loop on CPU, from the stored indices and weights.  Torch's CPU kernels contract and reorder nothing in a gather, a
    broadcast multiply and an add, so each of the k products and k adds differs by at most one rounding: 2 k eps sum_i |w_i f_i| bounds
    the difference.  Where the term matches bit for bit (it does with the torch this fixture was written under) that is asserted."""
    g = np.load(GOLDEN)
    f, idx, w, want = g["linear2_out"], g["knn_idx"], g["knn_weight"], g["interpolated"]
    got = O.forward(f, idx, w)
    k = idx.shape[1]
    bound = 2 * k * EPS * sum(np.abs(f[idx[:, i]].astype(np.float64) * w[:, i:i + 1]) for i in range(k))
    err = np.abs(got.astype(np.float64) - want)
    print("oracle vs golden: max err", err.max(), "bitwise", np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    assert (err <= bound).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_oracle_backward_is_float64_autograd_within_gamma_d(shape):
    """fp32 sums of d rounded products in pair order against float64 autograd of the formula: |err| <= gamma_d * sum |g w|, gamma_d =
    d u / (1 - d u), u = 2^-24 (one rounding per product, at most d - 1 per partial sum), d the source row's pair count"""
    n, m, k, c = shape
    p = cases.operands(n, m, k, c)
    got = O.backward(p["grad_out"], p["idx"], p["weight"], m).numpy().astype(np.float64)
    want, abs_sum, d = O.backward_float64(p["grad_out"], p["idx"], p["weight"], m)
    u = 2.0 ** -24
    gamma = (d * u / (1 - d * u))[:, None]
    assert (np.abs(got - want) <= gamma * abs_sum).all()
    assert (got[d == 0] == 0).all()


def test_oracle_forward_skips_invalid_entries_and_keeps_the_order():
    feat = torch.tensor([[1.0], [2.0 ** -24], [-1.0]])
    w = torch.ones(1, 3)
    assert O.forward(feat, torch.tensor([[0, 1, 2]]), w)[0, 0] == 0.0                 # (1 + 2^-24) rounds to 1, then - 1
    assert O.forward(feat, torch.tensor([[0, 2, 1]]), w)[0, 0] == np.float32(2.0 ** -24)
    assert O.forward(feat, torch.tensor([[-1, 3, 1]]), w, base=torch.tensor([[4.0]]))[0, 0] == 4.0   # 4 + 2^-24 rounds to 4
    assert O.forward(feat, torch.tensor([[-1, 3, 3]]), w)[0, 0] == 0.0
    half = O.backward(torch.tensor([[1.0 + 2.0 ** -11]]), torch.tensor([[0, 0, 5]]), w, 3, torch.float16)
    assert half.dtype == torch.float16 and half[0, 0] == 2.0 and (half[1:] == 0).all()   # 2 + 2^-10 -> a tie, to even


def test_cpu_tensors_raise_no_cpu_fallback():
    feat, idx, w = torch.rand(10, 8), torch.zeros(4, 3, dtype=torch.int32), torch.rand(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops.gather_add(feat, idx, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops.gather_add(feat, idx, w, torch.rand(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.gather_add_forward(4, 10, 3, 8, feat, idx, w, None, torch.empty(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.gather_add_backward(4, 10, 3, 8, torch.empty(4, 8), w, torch.zeros(11, dtype=torch.int32),
                                           torch.zeros(12, dtype=torch.int32), torch.empty(10, 8))


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _i32(*s):
    return torch.zeros(*s, dtype=torch.int32)


@pytest.mark.parametrize("feat,idx,weight,base,error", [
    (torch.rand(10), _i32(4, 3), torch.rand(4, 3), None, ValueError),                          # feat not [m, c]
    (torch.rand(10, 8).double(), _i32(4, 3), torch.rand(4, 3), None, TypeError),               # feat dtype
    (torch.rand(10, 8), torch.zeros(4, 3, dtype=torch.int16), torch.rand(4, 3), None, ValueError),   # idx dtype
    (torch.rand(10, 8), _i32(12), torch.rand(4, 3), None, ValueError),                         # idx not [n, k]
    (torch.rand(10, 8), _i32(4, 0), torch.rand(4, 0), None, ValueError),                       # k = 0
    (torch.rand(10, 8), _i32(4, 65), torch.rand(4, 65), None, ValueError),                     # k = 65
    (torch.rand(10, 1025), _i32(4, 3), torch.rand(4, 3), None, ValueError),                    # c = 1025
    (torch.rand(10, 8), _i32(4, 3), torch.rand(4, 3).half(), None, TypeError),                 # weight dtype
    (torch.rand(10, 8), _i32(4, 3), torch.rand(4, 2), None, ValueError),                       # weight shape
    (torch.rand(10, 8), _i32(4, 3), torch.rand(4, 3), torch.rand(4, 8).double(), TypeError),   # base dtype
    (torch.rand(10, 8), _i32(4, 3), torch.rand(4, 3), torch.rand(5, 8), ValueError),           # base shape
])
def test_operator_rejects_bad_arguments_before_any_launch(feat, idx, weight, base, error, monkeypatch):
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a launch was attempted"))
    with pytest.raises(error, match="gather_add"):
        pointops.gather_add(_OnGpu(feat), _OnGpu(idx), _OnGpu(weight), None if base is None else _OnGpu(base))


def test_binding_rejects_bad_shapes_and_dtypes(monkeypatch):
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a launch was attempted"))
    C = pointops2_cuda
    f32 = lambda *s: _OnGpu(torch.zeros(*s))
    i32 = lambda *s: _OnGpu(_i32(*s))
    for bad, error, name in (
            (dict(feat=f32(9, 8)), ValueError, "feat"), (dict(idx=i32(4, 4)), ValueError, "idx"), (dict(weight=f32(4, 4)), ValueError, "weight"),
            (dict(out=f32(5, 8)), ValueError, "out"), (dict(base=f32(4, 7)), ValueError, "base"),
            (dict(out=_OnGpu(torch.zeros(4, 8, dtype=torch.float16))), TypeError, "out"),
            (dict(weight=_OnGpu(torch.zeros(4, 3, dtype=torch.float16))), TypeError, "weight"),
            (dict(idx=_OnGpu(torch.zeros(4, 3, dtype=torch.int64))), TypeError, "idx"),
            (dict(base=_OnGpu(torch.zeros(4, 8, dtype=torch.float64))), TypeError, "base"),
            (dict(feat=_OnGpu(torch.zeros(8, 10).t())), RuntimeError, "contiguous")):
        args = dict(feat=f32(10, 8), idx=i32(4, 3), weight=f32(4, 3), base=f32(4, 8), out=f32(4, 8))
        args.update(bad)
        with pytest.raises(error, match=name):
            C.gather_add_forward(4, 10, 3, 8, args["feat"], args["idx"], args["weight"], args["base"], args["out"])
    for bad, error, name in (
            (dict(src_offsets=i32(10)), ValueError, "src_offsets"), (dict(src_pair=i32(13)), ValueError, "src_pair"),
            (dict(grad_feat=f32(11, 8)), ValueError, "grad_feat"), (dict(grad_out=_OnGpu(torch.zeros(4, 8, dtype=torch.float16))), TypeError, "grad_out"),
            (dict(grad_feat=_OnGpu(torch.zeros(10, 8, dtype=torch.float64))), TypeError, "grad_feat")):
        args = dict(grad_out=f32(4, 8), weight=f32(4, 3), src_offsets=i32(11), src_pair=i32(12), grad_feat=f32(10, 8))
        args.update(bad)
        with pytest.raises(error, match=name):
            C.gather_add_backward(4, 10, 3, 8, args["grad_out"], args["weight"], args["src_offsets"], args["src_pair"], args["grad_feat"])


def test_installer_patches_and_restores_the_standin_and_install_leaves_it_alone():
    original = decoder_standin.Upsample.forward
    assert original is not layers.upsample_forward
    try:
        sta.install()
        sta.install(third_party=False, fast_layers=False)
        assert decoder_standin.Upsample.forward is original
        assert layers.patch_classes(None, None, None) == [] and decoder_standin.Upsample.forward is original
        assert sta.install_fast_decoder(decoder_standin) == [decoder_standin.Upsample]
        assert decoder_standin.Upsample.forward is layers.upsample_forward
        layers.uninstall_fast_layers()
        assert decoder_standin.Upsample.forward is original
        assert layers.patch_upsample_class(decoder_standin.Upsample) == [decoder_standin.Upsample]
    finally:
        layers.uninstall_fast_layers()
    assert decoder_standin.Upsample.forward is original


def test_patched_class_runs_the_original_forward_for_cpu_tensors_and_without_support_feats():
    class Marked(decoder_standin.Upsample):
        def forward(self, feats, xyz, support_xyz, offset, support_offset, support_feats=None):
            return "original"

    try:
        assert layers.patch_upsample_class(Marked) == [Marked] and Marked.forward is layers.upsample_forward
        up, off = Marked(3, 8, 4), torch.tensor([5], dtype=torch.int32)
        assert up(torch.rand(5, 8), torch.rand(5, 3), torch.rand(9, 3), off, off, torch.rand(9, 4)) == "original"
        assert up(_OnGpu(torch.rand(5, 8)), _OnGpu(torch.rand(5, 3)), _OnGpu(torch.rand(9, 3)), off, off) == "original"
    finally:
        layers.uninstall_fast_layers()
    assert Marked(3, 8, 4)(None, None, None, None, None) == "original"
