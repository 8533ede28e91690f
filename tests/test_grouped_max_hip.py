"""GPU (-m gpu): the grouped maximum on csrc/grouped_max.hip - the launchers, pointops.grouped_max and the installed TransitionDown.forward
with layers.POOLED_TRANSITION - against the float64 oracle of tests/grouped_max_oracle.py evaluated on the CPU.

Bars.  Forward of the operator: bit-identical (the maximum is a selection).  Backward of the operator, per element:
|got - want64| <= (terms - 1) * 2^-24 * sum|term| + ulp(want64), the last term 0 for f32 and half an ulp of the row type for f16 / bf16
(fp32 accumulation in a fixed order, one rounding; the rounding itself - csrc/row_types.h, shared by every operator on f16 / bf16 rows -
is pinned bit for bit at its ties, at the overflow to inf and on a NaN by test_backward_rounds_once_to_nearest_even).  Layer, fp32: err_on <= 4 * err_off + 2^-24 * max|.|, both errors against float64 (the
two paths are fp32 dot products of the same length in another order); gradients after the upstream gradient is zeroed, the same way
on every side, where the float64 top-two gap of a group is below delta = 1e-4 * max|y| (a near-tie lets the two paths route a gradient to
different rows), at most 0.5 % of the entries.  Layer, autocast(f16): forward within one f16 ulp of the larger magnitude (both round an
fp32 sum once); gradients with delta = 2^-9 * max|y| (four f16 half-ulps of max|y|: either value may move by one rounding on either
path), at most 3 % masked, and the floor 2^-11 * max|.|, the unit roundoff of f16.

Measured on one MI355X (max abs error against float64, flag on / flag off; share of the upstream gradient masked):
    fp32      48 -> 96   forward 6.7e-07 / 6.7e-07   grad feats 6.2e-07 / 6.4e-07   masked 0.109 %
    fp32      192 -> 384 forward 2.0e-06 / 2.0e-06   grad feats 1.0e-06 / 4.6e-07   masked 0.084 %
    autocast  48 -> 96   forward 1.3e-03 / 1.3e-03   grad feats 1.5e-03 / 1.3e-03   masked 1.730 %   (on and off bit-identical)
    autocast  192 -> 384 forward 1.3e-03 / 1.3e-03   grad feats 1.2e-03 / 1.1e-03   masked 1.621 %   (on and off bit-identical)
The operator's backward met its bound with (err - bound) <= 0 at every case; every test prints its figures.
"""
import numpy as np
import pytest
import torch

from stratified_transformer_amd import scene
from tests import grouped_max_oracle as O
from tests.util import dev

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MANT = {"f32": 23, "f16": 10, "bf16": 7}
EMIN = {"f32": -126, "f16": -14, "bf16": -126}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


def _half_ulp(x, name):
    """half an ulp of the row type at |x| (0 for f32: the accumulator IS the result)"""
    if name == "f32":
        return np.zeros_like(x)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** EMIN[name])))
    return 0.5 * 2.0 ** (np.maximum(e, EMIN[name]) - MANT[name])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(got, want64, dtype, what):
    """got (GPU, row type) against float64 values that are elements of the row type: same NaNs, same bits elsewhere (the sign of zero too)"""
    want = torch.from_numpy(want64).to(dtype)
    got = got.cpu()
    assert got.dtype == dtype and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what + ": NaN pattern"
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), what + ": bits"


_KNN = {}


def _knn_lists(P, k):
    """kNN-k lists of a two-element batch, 3998 + 2 points, every fourth point (and both points of the small element) a query: the small
    element has fewer than k points for k >= 3, so its rows repeat indices"""
    if k not in _KNN:
        room = scene.make_room(3998, 11)
        xyz = np.concatenate([room, room[:2] + np.float32(0.5)]).astype(np.float32)
        q = np.concatenate([np.arange(0, 3998, 4), [3998, 3999]])
        x, off, n_off = dev(xyz), dev(np.array([3998, 4000], np.int32)), dev(np.array([len(q) - 2, len(q)], np.int32))
        idx, _ = P.knnquery(k, x, dev(np.ascontiguousarray(xyz[q])), off, n_off)
        torch.cuda.synchronize()
        idx_h = idx.cpu().numpy()
        assert idx_h.shape == (1002, k) and idx_h.min() >= 0 and idx_h.max() < 4000
        if k >= 3:
            assert len(np.unique(idx_h[-1])) < k                                  # duplicates, as the model meets them
        _KNN[k] = idx.contiguous()
    return _KNN[k]


def _lists(P, n_s, k, seed):
    if n_s == 4000:
        return _knn_lists(P, k)
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_s, (37, k)).astype(np.int32)
    idx[::2, k // 2:] = idx[::2, :1]
    return dev(idx)


def _grid_rows(n, c, dtype, seed, levels=6):
    """values on a coarse grid (multiples of 1/4: exact in every row type, exact ties common)"""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(-levels, levels + 1, (n, c)).astype(np.float32) / 4).to(dtype)


CASES = [(k, c, "f32 f16 bf16".split()[(ki + ci) % 3], 4000) for ki, k in enumerate((1, 3, 16, 34, 64)) for ci, c in enumerate((1, 3, 48, 96, 100, 384, 1024))]
CASES += [(k, c, t, 4000) for k in (16, 34) for c in (96, 100, 384) for t in DTYPES if (k, c, t, 4000) not in CASES]
CASES += [(k, c, t, n_s) for n_s in (1, 5) for k in (1, 3, 16, 64) for c, t in ((3, "f32"), (96, "f16"), (100, "bf16"), (8, "bf16"), (48, "f32"))]


@pytest.mark.parametrize("k,c,name,n_s", CASES)
def test_operator_against_the_oracle(P, k, c, name, n_s):
    dtype = DTYPES[name]
    idx = _lists(P, n_s, k, seed=k + c)
    m = idx.shape[0]
    feat_h = _grid_rows(n_s, c, dtype, seed=7 * k + c)
    go_h = _grid_rows(m, c, dtype, seed=k + 3 * c, levels=40)
    want_out, want_arg = O.forward(feat_h.double().numpy(), idx.cpu().numpy())
    want_g, terms, abs_sum = O.backward(go_h.double().numpy(), idx.cpu().numpy(), want_arg, n_s)
    runs = []
    for _ in range(2):
        feat = feat_h.cuda().requires_grad_(True)
        out = P.grouped_max(feat, idx)
        arg = [t for t in out.grad_fn.saved_tensors if t.dtype == torch.uint8]
        assert len(arg) == 1
        out.backward(go_h.cuda())
        torch.cuda.synchronize()
        runs.append((out.detach(), arg[0].clone(), feat.grad.clone()))
    out, arg, grad = runs[0]
    _same_bits(out, want_out, dtype, "out")
    assert np.array_equal(arg.cpu().numpy(), want_arg), "arg"
    assert grad.dtype == dtype and tuple(grad.shape) == (n_s, c)
    err = np.abs(grad.double().cpu().numpy() - want_g)
    bound = np.maximum(terms - 1, 0) * 2.0 ** -24 * abs_sum + _half_ulp(want_g, name)
    worst = float((err - bound).max())
    print(f"grouped_max k={k} c={c} {name} n_s={n_s}: max err {err.max():.3e}, max (err - bound) {worst:.3e}, max terms {int(terms.max())}")
    assert worst <= 0.0
    assert float(err[terms == 0].max(initial=0.0)) == 0.0                        # rows nobody took a maximum from: exactly 0
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(_bits(a) if a.dtype != torch.uint8 else a, _bits(b) if b.dtype != torch.uint8 else b)  # bitwise, run to run


def test_no_arg_without_a_gradient(P):
    idx = _knn_lists(P, 16)
    feat = _grid_rows(4000, 96, torch.float32, 1).cuda()
    before = P.GROUPED_MAX_ARGS
    out = P.grouped_max(feat, idx)
    with torch.no_grad():
        P.grouped_max(feat.clone().requires_grad_(True), idx)
    assert P.GROUPED_MAX_ARGS == before and out.grad_fn is None and not out.requires_grad
    out = P.grouped_max(feat.clone().requires_grad_(True), idx)
    assert P.GROUPED_MAX_ARGS == before + 1
    assert sorted(str(t.dtype) for t in out.grad_fn.saved_tensors) == ["torch.int32", "torch.uint8"]


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("c", [8, 5])
def test_non_finite_rows(P, name, c):
    dtype = DTYPES[name]
    feat_h = _grid_rows(12, c, dtype, 2)
    feat_h[1] = float("nan")
    feat_h[2] = float("inf")
    feat_h[3] = float("-inf")
    feat_h[4, ::2] = float("nan")
    idx_h = np.array([[0, 1, 2, 5], [2, 1, 1, 0], [3, 3, 3, 3], [3, 0, 5, 6], [2, 6, 7, 3], [4, 2, 1, 0], [7, 8, 9, 10]], np.int32)
    want_out, want_arg = O.forward(feat_h.double().numpy(), idx_h)
    assert np.isnan(want_out[0]).all() and (want_arg[0] == 1).all() and (want_arg[1] == 1).all()     # the first NaN
    assert np.isneginf(want_out[2]).all() and (want_arg[2] == 0).all() and np.isposinf(want_out[4]).all()
    feat = feat_h.cuda().requires_grad_(True)
    out = P.grouped_max(feat, dev(idx_h))
    arg = next(t for t in out.grad_fn.saved_tensors if t.dtype == torch.uint8)
    go_h = _grid_rows(7, c, dtype, 3)
    out.backward(go_h.cuda())
    torch.cuda.synchronize()
    _same_bits(out.detach(), want_out, dtype, "out")
    assert np.array_equal(arg.cpu().numpy(), want_arg)
    want_g, _, _ = O.backward(go_h.double().numpy(), idx_h, want_arg, 12)
    assert np.array_equal(feat.grad.double().cpu().numpy(), want_g)              # grid values, at most a few terms: exact


# one rounding of an fp32 sum to the row type, nearest even: (bits of a, bits of b, bits of round(a + b)); None: a NaN
NAN = {"bf16": 0x7fc0, "f16": 0x7e00}
ONE = {"bf16": 0x3f80, "f16": 0x3c00}
ROUNDING = {
    "bf16": [(0x3f80, 0x3b80, 0x3f80),   # 1 + 2^-8: a tie, down to the even 1
             (0x3f81, 0x3b80, 0x3f82),   # (1 + 2^-7) + 2^-8: a tie, up to the even 1 + 2^-6
             (0x7f7f, 0x7b00, 0x7f80),   # the largest finite value + half its ulp: inf
             (0xbf80, 0xbb80, 0xbf80),   # the first tie, negative
             (NAN["bf16"], ONE["bf16"], None)],
    "f16": [(0x3c00, 0x1000, 0x3c00),    # 1 + 2^-11: a tie, down to the even 1
            (0x3c01, 0x1000, 0x3c02),    # (1 + 2^-10) + 2^-11: a tie, up to the even 1 + 2^-9
            (0x7bff, 0x4c00, 0x7c00),    # 65504 + 16: inf
            (0xbc00, 0x9000, 0xbc00),
            (NAN["f16"], ONE["f16"], None)],
}


@pytest.mark.parametrize("name", list(ROUNDING))
@pytest.mark.parametrize("c", [8, 5])
def test_backward_rounds_once_to_nearest_even(P, name, c):
    """k = 1 and both queries on source row 0: the backward is round(grad_out[0] + grad_out[1]), one rounding of an fp32 sum to the row
    type - at its ties, at the overflow to inf and on a NaN; c = 8: the 16-byte chunk kernel, c = 5: one thread per element"""
    dtype = DTYPES[name]
    rows = ROUNDING[name] + ROUNDING[name][:c - 5]
    def as_rows(col):
        raw = np.array([[r[col] for r in rows]], np.uint16).view(np.int16)
        return torch.from_numpy(raw).view(dtype)
    go_h = torch.cat([as_rows(0), as_rows(1)])
    want = [r[2] for r in rows]
    by_torch = (go_h[0].float() + go_h[1].float()).to(dtype)                     # the table agrees with torch on the CPU: fp32 add, one rounding
    for ch, w in enumerate(want):
        assert bool(torch.isnan(by_torch[ch])) if w is None else int(_bits(by_torch)[ch]) & 0xffff == w, ch
    feat = torch.ones(1, c, dtype=dtype, device="cuda").requires_grad_(True)
    out = P.grouped_max(feat, torch.zeros((2, 1), dtype=torch.int32, device="cuda"))
    out.backward(go_h.cuda())
    torch.cuda.synchronize()
    assert feat.grad.dtype == dtype and tuple(feat.grad.shape) == (1, c)
    got = _bits(feat.grad.cpu())[0].numpy().view(np.uint16)
    print(f"grouped_max rounding {name} c={c}: got {[hex(int(g)) for g in got]}")
    for ch, w in enumerate(want):
        if w is None:
            assert bool(torch.isnan(feat.grad[0, ch])), ch
        else:
            assert int(got[ch]) == w, (ch, hex(int(got[ch])), hex(w))


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name,c", [("f32", 96), ("f16", 96), ("bf16", 7)])
def test_out_of_range_entries_are_skipped(P, name, c, idx_dtype):
    dtype, n_s = DTYPES[name], 50
    rng = np.random.default_rng(8)
    idx_h = rng.integers(0, n_s, (40, 16)).astype(np.int64)
    big = 2 ** 30 if idx_dtype == torch.int32 else 2 ** 40
    idx_h[rng.random(idx_h.shape) < 0.3] = -1
    idx_h[rng.random(idx_h.shape) < 0.1] = n_s
    idx_h[rng.random(idx_h.shape) < 0.1] = big
    idx_h[rng.random(idx_h.shape) < 0.05] = -(2 ** 31)
    idx_h[5] = [-1, n_s, big, -5] * 4                                            # no valid entry at all
    idx_h[6, :] = -1
    feat_h = _grid_rows(n_s, c, dtype, 9)
    go_h = _grid_rows(40, c, dtype, 10)
    want_out, want_arg = O.forward(feat_h.double().numpy(), idx_h)
    assert (want_arg[5] == O.NO_ARG).all() and (want_out[5] == 0).all()
    feat = feat_h.cuda().requires_grad_(True)
    out = P.grouped_max(feat, torch.from_numpy(idx_h).to(idx_dtype).cuda())
    arg = next(t for t in out.grad_fn.saved_tensors if t.dtype == torch.uint8)
    out.backward(go_h.cuda())
    torch.cuda.synchronize()
    _same_bits(out.detach(), want_out, dtype, "out")
    assert np.array_equal(arg.cpu().numpy(), want_arg)
    want_g, terms, abs_sum = O.backward(go_h.double().numpy(), idx_h, want_arg, n_s)
    err = np.abs(feat.grad.double().cpu().numpy() - want_g)
    assert float((err - (np.maximum(terms - 1, 0) * 2.0 ** -24 * abs_sum + _half_ulp(want_g, name))).max()) <= 0.0
    assert int(terms.sum()) == int((want_arg != O.NO_ARG).sum()) < 40 * c        # the all-invalid rows carry no gradient


def test_all_invalid_and_empty(P):
    feat = _grid_rows(9, 48, torch.float32, 4).cuda().requires_grad_(True)
    out = P.grouped_max(feat, torch.full((6, 16), -1, dtype=torch.int32, device="cuda"))
    out.sum().backward()
    torch.cuda.synchronize()
    assert float(out.detach().abs().max()) == 0.0 and float(feat.grad.abs().max()) == 0.0
    feat.grad = None
    out = P.grouped_max(feat, torch.zeros((0, 16), dtype=torch.int32, device="cuda"))                 # m = 0
    assert tuple(out.shape) == (0, 48) and out.dtype == torch.float32
    out.sum().backward()
    assert tuple(feat.grad.shape) == (9, 48) and float(feat.grad.abs().max()) == 0.0
    empty = torch.zeros((0, 48), device="cuda")                                                       # n_s = 0: every entry is invalid
    out = P.grouped_max(empty, torch.zeros((6, 16), dtype=torch.int32, device="cuda"))
    assert tuple(out.shape) == (6, 48) and float(out.abs().max()) == 0.0


def test_launcher_limits_record_an_error(P):
    from stratified_transformer_amd import pointops2_cuda as C
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    with pytest.raises(RuntimeError, match=r"k must be in \[1, 64\]"):
        C.grouped_max_forward(4, 10, 65, 8, z(10, 8), z(4, 65, dt=torch.int32), z(4, 8), z(4, 8, dt=torch.uint8))
    with pytest.raises(RuntimeError, match=r"c must be in \[1, 1024\]"):
        C.grouped_max_forward(4, 10, 3, 1025, z(10, 1025), z(4, 3, dt=torch.int32), z(4, 1025), None)
    with pytest.raises(RuntimeError, match=r"k must be in \[1, 64\]"):
        C.grouped_max_backward(4, 10, 65, 8, z(4, 8), z(4, 8, dt=torch.uint8), z(11, dt=torch.int32), z(260, dt=torch.int32), z(10, 8))
    with pytest.raises(RuntimeError, match=r"c must be in \[1, 1024\]"):
        C.grouped_max_backward(4, 10, 3, 1025, z(4, 1025), z(4, 1025, dt=torch.uint8), z(11, dt=torch.int32), z(12, dt=torch.int32), z(10, 1025))
    out, arg = torch.full((4, 8), 7.0, device="cuda"), z(4, 8, dt=torch.uint8)                        # and the library works on
    C.grouped_max_forward(4, 10, 3, 8, torch.ones(10, 8, device="cuda"), z(4, 3, dt=torch.int32), out, arg)
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == 1.0 and int(arg.max()) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the layer
# ------------------------------------------------------------------------------------------------------------------------------
SIZES, RATIO, K = (2500, 1500), 0.25, 16


@pytest.fixture()
def patched():
    """standin.TransitionDown with the installed forward; the flag and the class are restored afterwards"""
    from stratified_transformer_amd import layers, standin
    layers.patch_classes(transition_down_cls=standin.TransitionDown)
    try:
        yield layers, standin
    finally:
        layers.POOLED_TRANSITION = False
        layers.uninstall_fast_layers()


def _geometry(P, xyz, offset):
    from stratified_transformer_amd import index_build
    n_off = dev(np.asarray(index_build.transition_down_offset(offset.tolist(), RATIO), np.int32))
    idx = P.furthestsampling(dev(xyz), dev(offset), n_off)
    n_xyz = dev(xyz)[idx.long(), :]
    knn, _ = P.knnquery(K, dev(xyz), n_xyz, dev(offset), n_off)
    return knn.cpu(), n_xyz.cpu(), n_off.cpu()


def _layer_problem(P, c_in, c_out, standin):
    xyz, offset = scene.make_batch(list(SIZES), seed=c_in)
    torch.manual_seed(c_in)
    td = standin.TransitionDown(c_in, c_out, RATIO, K)
    with torch.no_grad():
        td.norm.weight.add_(0.1 * torch.randn(c_in))
        td.norm.bias.add_(0.1 * torch.randn(c_in))
    feats = torch.randn(xyz.shape[0], c_in)
    knn, n_xyz, n_off = _geometry(P, xyz, offset)
    go = torch.randn(knn.shape[0], c_out)
    return xyz, offset, td, feats, knn, n_xyz, n_off, go


def _float64_side(td, feats, knn, go, delta_rel):
    """the composite :106-109 in float64 with the upstream gradient masked at near-ties: out, the mask, max|y|, gradients"""
    leaves = [t.detach().double().requires_grad_(True) for t in (feats, td.norm.weight, td.norm.bias, td.linear.weight)]
    out = O.composite(leaves[0], knn, leaves[1], leaves[2], leaves[3], td.norm.eps)
    with torch.no_grad():
        _, y = O.per_source(leaves[0], knn, leaves[1], leaves[2], leaves[3], td.norm.eps)
        top = y[knn.long()].topk(2, dim=1).values
        y_max = float(y.abs().max())
        masked = (top[:, 0] - top[:, 1]) < delta_rel * y_max
    (out * (go.double() * ~masked)).sum().backward()
    return out.detach(), masked, y_max, [t.grad for t in leaves]


def _gpu_side(layers, td, feats, xyz, offset, go_masked, on, amp):
    layers.POOLED_TRANSITION = on
    layers.forget_clouds()
    mod = td.cuda()
    mod.zero_grad(set_to_none=True)
    f = feats.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        out, n_xyz, n_off = mod(f, dev(xyz), dev(offset))
    out.backward(go_masked.cuda().to(out.dtype))
    torch.cuda.synchronize()
    return out.detach().cpu(), n_xyz.cpu(), n_off.cpu(), [t.grad.detach().cpu() for t in (f, mod.norm.weight, mod.norm.bias, mod.linear.weight)]


GRADS = ("feats", "norm.weight", "norm.bias", "linear.weight")


@pytest.mark.parametrize("c_in,c_out", [(48, 96), (192, 384)])
def test_pooled_transition_fp32(P, patched, c_in, c_out):
    layers, standin = patched
    xyz, offset, td, feats, knn, n_xyz, n_off, go = _layer_problem(P, c_in, c_out, standin)
    want, masked, y_max, want_g = _float64_side(td, feats, knn, go, 1e-4)
    share = float(masked.double().mean())
    go_masked = go * ~masked
    off = _gpu_side(layers, td, feats, xyz, offset, go_masked, False, False)
    on = _gpu_side(layers, td, feats, xyz, offset, go_masked, True, False)
    for side in (off, on):
        assert side[0].dtype == torch.float32 and torch.equal(side[1], n_xyz) and torch.equal(side[2], n_off)
    err_on, err_off = float((on[0].double() - want).abs().max()), float((off[0].double() - want).abs().max())
    print(f"pooled transition fp32 {c_in}->{c_out}: forward err on {err_on:.3e} off {err_off:.3e} (max|y| {y_max:.3f}); masked {100 * share:.3f} %")
    assert err_on <= 4 * err_off + 2.0 ** -24 * y_max
    assert share <= 0.005
    for name, g_on, g_off, g64 in zip(GRADS, on[3], off[3], want_g):
        e_on, e_off, top = float((g_on.double() - g64).abs().max()), float((g_off.double() - g64).abs().max()), float(g64.abs().max())
        print(f"    grad {name}: err on {e_on:.3e} off {e_off:.3e} (max {top:.3f})")
        assert e_on <= 4 * e_off + 2.0 ** -24 * top, name


@pytest.mark.parametrize("c_in,c_out", [(48, 96), (192, 384)])
def test_pooled_transition_autocast_f16(P, patched, c_in, c_out):
    layers, standin = patched
    xyz, offset, td, feats, knn, n_xyz, n_off, go = _layer_problem(P, c_in, c_out, standin)
    want, masked, y_max, want_g = _float64_side(td, feats, knn, go, 2.0 ** -9)
    share = float(masked.double().mean())
    go_masked = go * ~masked
    off = _gpu_side(layers, td, feats, xyz, offset, go_masked, False, True)
    on = _gpu_side(layers, td, feats, xyz, offset, go_masked, True, True)
    for side in (off, on):
        assert side[0].dtype == torch.float16 and torch.equal(side[1], n_xyz) and torch.equal(side[2], n_off)
    a, b = on[0].double().numpy(), off[0].double().numpy()
    ulp = 2 * _half_ulp(np.maximum(np.abs(a), np.abs(b)), "f16")
    err_on, err_off = float(np.abs(a - want.numpy()).max()), float(np.abs(b - want.numpy()).max())
    print(f"pooled transition autocast {c_in}->{c_out}: forward err on {err_on:.3e} off {err_off:.3e}; on/off differ at "
          f"{100 * float((a != b).mean()):.3f} % by at most {float((np.abs(a - b) / ulp).max()):.2f} ulp; masked {100 * share:.3f} %")
    assert float((np.abs(a - b) - ulp).max()) <= 0.0
    assert share <= 0.03
    for name, g_on, g_off, g64 in zip(GRADS, on[3], off[3], want_g):
        e_on, e_off, top = float((g_on.double() - g64).abs().max()), float((g_off.double() - g64).abs().max()), float(g64.abs().max())
        print(f"    grad {name}: err on {e_on:.3e} off {e_off:.3e} (max {top:.3f})")
        assert e_on <= 4 * e_off + 2.0 ** -11 * top, name


def test_pooled_transition_geometry_prefetched_or_not(P):
    """flag on with the geometry BasicLayer.forward prefetched == flag on on a bare TransitionDown call; the next cloud and its offsets are
    bit-identical to the flag-off results either way"""
    from stratified_transformer_amd import layers, standin
    xyz, offset = scene.make_batch(list(SIZES), seed=5)
    torch.manual_seed(5)
    layer = standin.BasicLayer(8, 2, 48, 3, 0.16, 0.01, ratio=RATIO, k=K, out_channels=96).cuda()
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if "relative_pos" in name:
                p.copy_(torch.randn_like(p) * 0.3)
    feats = torch.randn(xyz.shape[0], 48, device="cuda")
    runs, before = {}, layers.STATS["transitions_prefetched"]
    try:
        layers.patch_classes(standin.BasicLayer, standin.WindowAttention, standin.TransitionDown)
        for on in (False, True):
            layers.POOLED_TRANSITION = on
            layers.forget_clouds()
            P.clear_caches()
            with torch.no_grad():
                f, _, _, f_down, x_down, o_down = layer(feats, dev(xyz), dev(offset))
                bare = layer.downsample(f, dev(xyz), dev(offset))                 # a new xyz tensor: nothing prefetched for it
            torch.cuda.synchronize()
            runs[on] = (f, f_down, x_down, o_down) + tuple(bare)
    finally:
        layers.POOLED_TRANSITION = False
        layers.uninstall_fast_layers()
    assert layers.STATS["transitions_prefetched"] - before == 2
    off, on = runs[False], runs[True]
    assert torch.equal(off[0], on[0])                                             # the blocks do not see the flag
    for side in (off, on):
        assert torch.equal(side[2], side[5]) and torch.equal(side[3], side[6])    # prefetched == bare: next cloud, offsets
    assert torch.equal(on[2], off[2]) and torch.equal(on[3], off[3]) and on[3].dtype == torch.int32
    assert torch.equal(on[1], on[4])                                              # pooled rows: prefetched == bare, bit for bit
    assert float((on[1] - off[1]).abs().max()) <= 1e-4 * float(off[1].abs().max())
