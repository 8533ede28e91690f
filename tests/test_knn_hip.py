"""GPU (-m gpu): the exact kNN on every kernel path, k boundary and degenerate cloud of tests/knn_cases.py, and the operators
that consume its indices (ball_query, interpolation, queryandgroup, Divide2Patch), against the CPU oracle.

Bars: indices and distances of the kNN bit for bit (ties included), grouped tensors exact, interpolation values within the
tolerances of test_hip_parity.py::test_grouping_and_interpolation (1e-5 forward, 1e-4 backward and interpolation_v2).
tests/test_knn_cases_cpu.py establishes, without a GPU, which kernel each case reaches and how many of its queries are replayed."""
import numpy as np
import pytest
import torch

from oracle import pointops_ref as ref
from tests import knn_cases as C
from tests.util import dev

pytestmark = pytest.mark.gpu

ALL = sorted(C.CASES)
_ORACLE = {}


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()
    return pointops


def _np(t):
    return t.detach().cpu().numpy()


def _oracle(name):
    """(idx, dist) of the full heap scan, computed once per case and never written to"""
    if name not in _ORACLE:
        c = C.CASES[name]
        i, d = ref.knnquery(c.k, c.xyz, c.new_xyz, c.offset, c.new_offset)
        i.setflags(write=False), d.setflags(write=False)
        _ORACLE[name] = (i, d)
    return _ORACLE[name]


def _run(P, c):
    idx, dist = P.knnquery(c.k, dev(c.xyz), dev(c.new_xyz), dev(c.offset), dev(c.new_offset))
    return _np(idx), _np(dist)


def _assert_same(got, want, what):
    (i_got, d_got), (i_want, d_want) = got, want
    bad = np.flatnonzero((i_got != i_want).any(1) | (d_got != d_want).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(i_got)} queries differ, first {bad[:8].tolist()}"
    assert np.array_equal(i_got, i_want) and np.array_equal(d_got, d_want), what


@pytest.mark.parametrize("name", ALL)
def test_knn_case_is_bit_exact(P, name):
    c = C.CASES[name]
    _assert_same(_run(P, c), _oracle(name), f"{name} ({C.kernel_of(c)})")


def test_threshold_pair_scan_and_grid_agree_on_one_cloud(P):
    """n = 4096 through the grid (workspace lent) and through the option-free launcher (knn_kernel, the scan): same squared
    distances and indices; n = 4095 of the same cloud (scanned either way) is covered by test_knn_case_is_bit_exact"""
    from stratified_transformer_amd import pointops2_cuda
    c = C.CASES["threshold_at-k16"]
    m = len(c.new_xyz)
    idx = torch.zeros((m, c.k), dtype=torch.int32, device="cuda")
    d2 = torch.zeros((m, c.k), device="cuda")
    pointops2_cuda.knnquery_cuda(m, c.k, dev(c.xyz), dev(c.new_xyz), dev(c.offset), dev(c.new_offset), idx, d2)  # (no launch options)
    g_idx, g_d2 = P.knn_squared(c.k, dev(c.xyz), dev(c.new_xyz), dev(c.offset), dev(c.new_offset))
    _assert_same((_np(idx), _np(d2)), (_np(g_idx), _np(g_d2)), "scan vs grid")
    _assert_same((_np(idx), np.sqrt(_np(d2))), _oracle(c.name), "scan vs oracle")


@pytest.mark.parametrize("k", C.DEGENERATE_KS)
def test_translation_does_not_change_the_gpu_result(P, k):
    """every coordinate, difference and d2 of the family is exact in fp32 at every T (tests/test_knn_cases_cpu.py): what the
    grid returns at T must be what it returns at T = 0, and both the oracle's"""
    base = _run(P, C.CASES[f"translate_0-k{k}"])
    _assert_same(base, _oracle(f"translate_0-k{k}"), "T = 0 vs oracle")
    for T in C.TRANSLATIONS[1:]:
        got = _run(P, C.CASES[f"translate_{T}-k{k}"])
        _assert_same(got, base, f"T = {T} vs T = 0")
        _assert_same(got, _oracle(f"translate_{T}-k{k}"), f"T = {T} vs oracle")


@pytest.mark.parametrize("n", [1500, 4096])
def test_knn_squared_of_a_cloud_with_itself(P, n):
    """new_xyz=None: the cloud is its own query set (n = 1500: scanned; n = 4096: grid).  The squared distances are compared with
    the fma chain restated in numpy (ref.ball_query with a radius that holds everything), the order with the oracle's heap."""
    c = C.CASES["sweep_random-k16"]
    xyz, off = np.ascontiguousarray(c.xyz[:n]), np.array([n], np.int32)
    idx, d2 = P.knn_squared(16, dev(xyz), None, dev(off), dev(off))
    idx, d2 = _np(idx), _np(d2)
    i_ref, d_ref = ref.knnquery(16, xyz, None, off, off)
    assert np.array_equal(idx, i_ref) and np.array_equal(np.sqrt(d2), d_ref)
    assert (idx[:, 0] == np.arange(n)).all() and (d2[:, 0] == 0).all()
    _, d2_ref = ref.ball_query(1e3, 16, xyz, xyz[:512], off, np.array([512], np.int32))
    assert np.array_equal(d2[:512], d2_ref)


def _assert_ball_rows(idx, d2, widx, wd2):
    """the rule of test_hip_parity.py::test_ball_query_on_the_knn_grid: the sorted distance rows are identical, padding included;
    indices may differ only inside runs of equal distance"""
    np.testing.assert_array_equal(d2, wd2)
    assert ((idx >= 0) == (widx >= 0)).all()
    same = idx == widx
    for r in np.flatnonzero(~same.all(1)):
        for dval in np.unique(d2[r][~same[r]]):
            sel = d2[r] == dval
            assert sorted(idx[r][sel]) == sorted(widx[r][sel])


@pytest.fixture(scope="module")
def ball_scene():
    """supports: an element of 20 points in a box of edge 0.1 (fewer than max_num, most of them in reach of its queries) and one of
    4096 in the unit cube; queries: 6 + 1024 uniform draws in the same boxes, none a support point"""
    rng = np.random.default_rng(31)
    x = rng.random((20 + 4096, 3), dtype=np.float32)
    y = rng.random((6 + 1024, 3), dtype=np.float32)
    x[:20] *= np.float32(0.1)
    y[:6] *= np.float32(0.1)
    off_x, off_y = np.array([20, 4116], np.int32), np.array([6, 1030], np.int32)
    _, nearest = ref.knnquery(1, x, y, off_x, off_y)
    assert nearest.min() > 0
    return x, y, off_x, off_y, float(nearest.min())


@pytest.mark.parametrize("max_num", [34, 64])
def test_ball_query_off_support_queries_and_a_short_element(P, ball_scene, max_num):
    x, y, off_x, off_y, _ = ball_scene
    radius = 0.12   # about 30 of the 4096 points: rows that fill up and rows that do not, for either max_num
    idx, d2 = P.ball_query(radius, max_num, dev(x), dev(y), dev(off_x), dev(off_y))
    widx, wd2 = ref.ball_query(radius, max_num, x, y, off_x, off_y)
    idx, d2 = _np(idx), _np(d2)
    assert idx.shape == widx.shape == (1030, max_num)
    _assert_ball_rows(idx, d2, widx, wd2)
    filled = (widx >= 0).sum(1)
    assert filled[6:].min() < max_num and (filled[6:].max() == max_num) == (max_num == 34)   # rows fill up at 34, none does at 64
    assert (filled[:6] >= 10).all() and (filled[:6] <= 20).all()       # the short element: its points, then padding - never its filler
    assert (idx[:6] < 20).all() and (idx[6:][idx[6:] >= 0] >= 20).all()   # never across batch elements


@pytest.mark.parametrize("max_num", [34, 64])
def test_ball_query_with_nothing_in_reach_is_all_padding(P, ball_scene, max_num):
    x, y, off_x, off_y, nearest = ball_scene
    radius = 0.5 * nearest                                             # smaller than every query's nearest distance
    idx, d2 = P.ball_query(radius, max_num, dev(x), dev(y), dev(off_x), dev(off_y))
    widx, wd2 = ref.ball_query(radius, max_num, x, y, off_x, off_y)
    assert (widx == -1).all() and (wd2 == -1).all()
    assert np.array_equal(_np(idx), widx) and np.array_equal(_np(d2), wd2)


@pytest.fixture(scope="module")
def interp_scene():
    """supports: an element of 2 points (fewer than k = 3: the third neighbour is the filler, index 0 at distance sqrt(1e10)) and
    one of 1500; queries: 8 + 3000, a quarter of them exactly on support points (d = 0: the weight 1 / (0 + 1e-8)).  m * n is
    above the grid threshold.  Expected weights as in test_hip_parity.py::test_grouping_and_interpolation."""
    rng = np.random.default_rng(32)
    sup = rng.random((2 + 1500, 3), dtype=np.float32)
    qry = rng.random((8 + 3000, 3), dtype=np.float32)
    qry[:2] = sup[:2]
    qry[8:8 + 750] = sup[2 + rng.permutation(1500)[:750]]
    s_off, q_off = np.array([2, 1502], np.int32), np.array([8, 3008], np.int32)
    i3, d3 = ref.knnquery(3, sup, qry, s_off, q_off)
    assert (d3[:, 0] == 0).mean() == 752 / 3008 and (i3[:8, 2] == 0).all() and (d3[:8, 2] == np.sqrt(np.float32(1e10))).all()
    wgt = 1.0 / (d3 + 1e-8)
    wgt = (wgt / wgt.sum(1, keepdims=True)).astype(np.float32)
    assert (wgt[8:8 + 750, 0] > 0.9999).all() and (wgt[:8, 2] < 1e-5).all()   # a coincident support takes the row; the filler nothing
    d_v2 = np.sqrt(((qry[:, None, :] - sup[i3]) ** 2).sum(-1) + np.float32(1e-8))     # its own distances (sqrt(d^2 + 1e-8))
    w_v2 = 1.0 / (d_v2 + np.float32(1e-8))
    w_v2 = (w_v2 / w_v2.sum(1, keepdims=True)).astype(np.float32)
    return dict(sup=sup, qry=qry, s_off=s_off, q_off=q_off, i3=i3, wgt=wgt, w_v2=w_v2)


@pytest.mark.parametrize("c", [1, 24, 33])
def test_interpolation_with_coincident_queries_and_a_short_support_element(P, interp_scene, c):
    s = interp_scene
    rng = np.random.default_rng(33 + c)
    feat = rng.standard_normal((1502, c), dtype=np.float32)
    go = rng.standard_normal((3008, c), dtype=np.float32)
    want = ref.interpolation_forward(feat, s["i3"], s["wgt"])
    want_grad = ref.interpolation_backward(go, s["i3"], s["wgt"], 1502)
    args = (dev(s["sup"]), dev(s["qry"]))
    offs = (dev(s["s_off"]), dev(s["q_off"]))
    f1 = dev(feat).requires_grad_(True)
    got1 = P.interpolation(*args, f1, *offs)
    np.testing.assert_allclose(_np(got1), want, rtol=1e-5, atol=1e-5)
    f2 = dev(feat).requires_grad_(True)
    got2 = P.interpolation2(*args, f2, *offs, 3)
    np.testing.assert_allclose(_np(got2), want, rtol=1e-5, atol=1e-5)
    assert torch.equal(got1, got2)
    got1.backward(dev(go))
    got2.backward(dev(go))
    np.testing.assert_allclose(_np(f1.grad), want_grad, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(_np(f2.grad), want_grad, rtol=1e-4, atol=1e-4)
    f3 = dev(feat).requires_grad_(True)
    got3 = P.interpolation_v2(*args, f3, *offs)
    np.testing.assert_allclose(_np(got3), ref.interpolation_forward(feat, s["i3"], s["w_v2"]), rtol=1e-4, atol=1e-4)
    got3.backward(dev(go))
    np.testing.assert_allclose(_np(f3.grad), ref.interpolation_backward(go, s["i3"], s["w_v2"], 1502), rtol=1e-4, atol=1e-4)


def test_queryandgroup_with_relative_coordinates(P):
    """use_xyz=True: [xyz[idx] - new_xyz | feat[idx]], exact (one fp32 subtraction per coordinate); on the grid path"""
    c = C.CASES["threshold_at-k16"]
    feat = np.random.default_rng(34).standard_normal((len(c.xyz), 5), dtype=np.float32)
    i_ref, _ = _oracle(c.name)
    want = ref.grouping(np.concatenate([c.xyz, feat], 1), i_ref)
    want[:, :, :3] -= c.new_xyz[:, None, :]
    got, idx = P.queryandgroup(c.k, dev(c.xyz), dev(c.new_xyz), dev(feat), None, dev(c.offset), dev(c.new_offset), use_xyz=True, return_indx=True)
    assert np.array_equal(_np(idx), i_ref)
    assert got.shape == (1024, 16, 8)
    np.testing.assert_array_equal(_np(got), want)


def test_divide2patch_on_a_ragged_batch(P):
    """[70, 3, 900] points, 16 per patch: 4, 0 and 56 patches - the element of 3 points yields none - each patch the 16 nearest of
    an FPS anchor within its element; against the oracle's FPS followed by the oracle's kNN"""
    rng = np.random.default_rng(35)
    xyz = rng.random((973, 3), dtype=np.float32)
    offset = np.array([70, 73, 973], np.int32)
    want_off = np.array([4, 4, 60], np.int32)
    anchors = ref.furthestsampling(xyz, offset, want_off)
    want, _ = ref.knnquery(16, xyz, np.ascontiguousarray(xyz[anchors]), offset, want_off)
    P.clear_caches()
    p_idx, new_offset = P.Divide2Patch(16, dev(xyz), dev(offset), return_offset=True)
    assert new_offset.dtype == torch.int32 and _np(new_offset).tolist() == want_off.tolist()
    assert np.array_equal(_np(p_idx), want)
    assert ((want[:4] < 70).all() and (want[4:] >= 73).all())          # no patch touches the 3-point element
    assert np.array_equal(_np(P.Divide2Patch(16, dev(xyz), dev(offset))), want)
