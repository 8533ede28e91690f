"""GPU (-m gpu): the segment softmax on every (kernel, head-width) region and length boundary, the CSC build, the CSR helpers and
the row gathers, on the cases of tests/pair_ops_cases.py against float64 references at the bounds derived there (no hand-picked
tolerance).  tests/test_pair_ops_cases_cpu.py establishes, without a GPU, what each case reaches, that a correct fp32
implementation meets the bounds and that wrong ones miss them.  Each test prints the largest fraction of its bound."""
import numpy as np
import pytest
import torch

from oracle import pointops_ref as ref
from tests import pair_ops_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()
    return pointops


def dev(a):
    """a device copy (the case arrays are read-only and stay so)"""
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _softmax(P, x, offsets, gy=None):
    """-> (y, grad_x or None) as numpy, through the operator"""
    src = dev(x).requires_grad_(gy is not None)
    y = P.segment_softmax(src, offsets)
    if gy is None:
        return _np(y), None
    y.backward(gy)
    return _np(y), _np(src.grad)


# ---------------------------------------------------------------------------------------------------------------------
# segment softmax
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hn", C.SOFTMAX_CASES, ids=C.softmax_id)
def test_segment_softmax_case(P, hn):
    c = C.softmax_case(*hn)
    offsets, gy = dev(c.offsets), dev(c.gy)
    y, gx = _softmax(P, c.x, offsets, gy)
    f = C.check_softmax_fwd(y, c)
    b = C.check_softmax_bwd(gx, y, c)
    print(f"fraction softmax_fwd {c.name} {C.kernel_of(c.N, c.h)} {f:.4f}")
    print(f"fraction softmax_bwd {c.name} {C.kernel_of(c.N, c.h)} {b:.4f}")
    y2, gx2 = _softmax(P, c.x, offsets, gy)  # no atomics in these kernels: the same bits every time
    assert np.array_equal(_bits(y), _bits(y2)) and np.array_equal(_bits(gx), _bits(gx2))


@pytest.mark.parametrize("hn", C.NONFINITE_BASES, ids=C.softmax_id)
def test_segment_softmax_nonfinite_heads_stay_contained(P, hn):
    """a (segment, head) with a NaN, a +inf or only -inf is NaN throughout; everything else keeps its bits"""
    c = C.softmax_case(*hn)
    x, poisoned = C.nonfinite_variant(c)
    offsets = dev(c.offsets)
    clean, _ = _softmax(P, c.x, offsets)
    got, _ = _softmax(P, x, offsets)
    assert np.isnan(got[poisoned]).all()
    assert np.array_equal(_bits(got)[~poisoned], _bits(clean)[~poisoned])


@pytest.mark.parametrize("hn", [(3, 20000), (12, 20000), (65, 200)], ids=C.softmax_id)
def test_segment_softmax_masked_entries(P, hn):
    """-inf next to finite logits: exactly 0 there forward and backward, the rest renormalised over the finite ones"""
    c = C.softmax_case(*hn)
    y, gx = _softmax(P, c.x, dev(c.offsets), dev(c.gy))
    masked = np.isneginf(c.x)
    assert masked.any() and not y[masked].any() and not gx[masked].any()
    _, bound = c.reference()
    for r in c.rows:
        if r.family == "masked":  # the finite entries alone sum to 1, within the sum of their own bounds
            seg = slice(r.start, r.start + r.length)
            total = np.where(masked[seg], 0.0, y[seg].astype(np.float64)).sum(0)
            assert (np.abs(total - 1) <= bound[seg].sum(0)).all(), (r, total)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("hn", [(3, 20000), (12, 20000)], ids=C.softmax_id)
def test_scatter_softmax_shim_with_skipped_ids(P, hn, dtype):
    """compat.scatter_softmax with an ascending index that skips ids: without a remembered CSR (the shim compacts the runs
    into offsets of its own: 39 rows, so h > 4 runs the block kernel) and with one (the table's offsets, verified on the device)"""
    from stratified_transformer_amd.compat import scatter_softmax
    c = C.softmax_case(*hn)
    index = torch.from_numpy(C.csr_expand_ref(c.offsets)).to("cuda", dtype)
    assert len(torch.unique(index)) == len(c.rows) < c.N
    P.clear_caches()
    assert P.last_csr(index.device.index, c.M) is None
    f0 = C.check_softmax_fwd(_np(scatter_softmax(dev(c.x), index, dim=0)), c, "compacted ")
    offsets = dev(c.offsets)
    P.remember_csr(offsets, c.M)
    assert bool(P.csr_matches(offsets, index))
    src = dev(c.x).requires_grad_(True)
    y = scatter_softmax(src, index, dim=0)
    f1 = C.check_softmax_fwd(_np(y), c, "remembered ")
    y.backward(dev(c.gy))
    b1 = C.check_softmax_bwd(_np(src.grad), _np(y), c, "remembered ")
    P.clear_caches()
    print(f"fraction scatter_softmax {c.name} {max(f0, f1):.4f} bwd {b1:.4f}")


# ---------------------------------------------------------------------------------------------------------------------
# CSC build, CSR expand and matches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.CSC_ROWS)
def test_csc_build_equals_the_stable_argsort(P, N):
    for c in C.csc_cases(N):
        got = [_np(t) for t in P._csc_build(dev(c.offsets), dev(c.index_1), c.n_keys)]
        want = C.csc_ref(c.index_0, c.index_1, c.n_keys)
        for name, g, w in zip(("offsets", "pair", "query"), got, want):
            assert g.dtype == np.int32 and np.array_equal(g, w), f"{c.name}: {name} differs at {np.flatnonzero(g != w)[:8].tolist()}"


@pytest.mark.parametrize("N,n_keys", [(1, 1), (5, 13), (257, 128)])
def test_csc_build_of_an_empty_pair_list(P, N, n_keys):
    offsets, pair, query = P._csc_build(torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
                                        torch.zeros(0, dtype=torch.int32, device="cuda"), n_keys)
    assert offsets.shape == (n_keys + 1,) and not offsets.any() and pair.numel() == 0 and query.numel() == 0


def _expand(offsets, M, preset):
    from stratified_transformer_amd import _lib
    index0 = torch.full((M,), preset, dtype=torch.int32, device="cuda")
    o = dev(offsets)
    _lib.call("csr_expand_launcher", len(offsets) - 1, M, _lib.ptr(o), _lib.ptr(index0), device=o.device)
    return _np(index0)


@pytest.mark.parametrize("name", sorted(C.MATCH_LENS))
def test_csr_expand_equals_repeat(P, name):
    offsets, index = C.match_list(name)
    M = len(index)
    assert np.array_equal(_expand(offsets, M, -7), index) and np.array_equal(index, np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)))
    # positions no segment covers keep their preset: five in front, four behind
    got = _expand(offsets + 5, M + 9, -7)
    assert np.array_equal(got, np.concatenate([np.full(5, -7), index, np.full(4, -7)]))


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name", sorted(C.MATCH_LENS))
def test_csr_matches_finds_every_single_defect(P, name, dtype):
    offsets, index = C.match_list(name, dtype)
    assert bool(P.csr_matches(dev(offsets), dev(index))), "the matching list (an empty segment in its middle)"
    missed = [what for what, o, i in C.match_mutations(name, dtype) if bool(P.csr_matches(dev(o), dev(i)))]
    assert not missed, f"csr_matches accepts {missed}"


# ---------------------------------------------------------------------------------------------------------------------
# row gathers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.GATHER_C)
def test_grouping_cases(P, c):
    worst = 0.0
    for g in C.group_cases(c):
        inp = dev(g.inp).requires_grad_(True)
        out = P.grouping(inp, dev(g.idx))
        assert np.array_equal(_bits(_np(out)), _bits(g.inp[g.idx])), g.name
        out.backward(dev(g.go))
        worst = max(worst, C.check_grouping_bwd(_np(inp.grad), g, g.name))
    print(f"fraction grouping_bwd c{c} {worst:.4f}")


@pytest.mark.parametrize("c", C.GATHER_C)
def test_weighted_gather_cases(P, c):
    from stratified_transformer_amd import pointops2_cuda
    worst_f = worst_b = 0.0
    for g in C.gather_cases(c):
        n, k = g.idx.shape
        idx, weight, out = dev(g.idx), dev(g.weight), dev(g.preset.copy())
        pointops2_cuda.interpolation_forward_cuda(n, c, k, dev(g.inp), idx, weight, out)
        worst_f = max(worst_f, C.check_gather_fwd(_np(out), g, g.name))
        gi = torch.zeros((C.SRC_ROWS, c), device="cuda")
        pointops2_cuda.interpolation_backward_cuda(n, c, k, dev(g.go), idx, weight, gi)
        worst_b = max(worst_b, C.check_gather_bwd(_np(gi), g, g.name))
    print(f"fraction gather_fwd c{c} {worst_f:.4f}")
    print(f"fraction gather_bwd c{c} {worst_b:.4f}")


def test_interpolation_onto_a_two_point_support_element(P):
    """k = 3 over a support element of two points: the kNN's third slot is its filler (the element's first row at distance 1e5), which the
    operator weighs like any neighbour; against the float64 restatement on the oracle's kNN output"""
    p = C.interpolation_case()
    idx, dist = ref.knnquery(p["k"], p["xyz"], p["new_xyz"], p["offset"], p["new_offset"])
    assert (idx[60:, 2] == 40).all() and (dist[60:, 2] == 1e5).all() and (idx[60:, :2] >= 40).all() and (idx[:60] < 40).all()
    want, bound = C.interpolation_f64(p["feat"], idx, dist)
    feat = dev(p["feat"]).requires_grad_(True)
    got = P.interpolation(dev(p["xyz"]), dev(p["new_xyz"]), feat, dev(p["offset"]), dev(p["new_offset"]), p["k"])
    f = C.fraction_of_bound(_np(got), want, bound, "interpolation")
    go = np.random.default_rng(8).standard_normal(want.shape, dtype=np.float32)
    got.backward(dev(go))
    r = 1.0 / (dist.astype(np.float64) + 1e-8)
    w = r / r.sum(1, keepdims=True)
    gwant, K, S = C.scatter_sum_f64(idx.reshape(-1), (go.astype(np.float64)[:, None, :] * w[:, :, None]).reshape(idx.size, -1), 42)
    # the atomic bound with the products' and the fp32 weights' rounding ((k + 2)u, tests/pair_ops_cases.py interpolation_f64)
    b = C.fraction_of_bound(_np(feat.grad), gwant, np.maximum((K + p["k"] + 3) * C.U * S, 1e-300), "interpolation backward")
    print(f"fraction interpolation_fwd {f:.4f}")
    print(f"fraction interpolation_bwd {b:.4f}")
