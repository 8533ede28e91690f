"""CPU: the cases of tests/kpconv_cases.py are what they claim, a plain fp32 numpy evaluation of the formulas meets the derived
bounds on every one of them (so a correct fp32 kernel can), and deliberately wrong variants miss them (so the bounds have teeth).
No HIP."""
import numpy as np
import pytest

from tests import kpconv_cases as C

CUS = 256  # the MI355X's; the device test takes the count from the device


def _finite_cases():
    yield C.n_valid_sweep_case()
    for shape in C.EDGE_SHAPES:
        yield C.edge_case(*shape)
    for which in C.LDS_SHAPES:
        yield C.lds_case(which)
    for n_q in C.QUERY_COUNTS:
        yield C.query_count_case(n_q)
    yield C.past_cap_case(CUS)
    yield C.single_support_case()
    yield C.empty_support_case()
    yield C.exact_case()
    yield C.off_origin_case()
    yield C.duplicate_row_case()
    yield C.one_support_row_case()
    yield C.plain_case()


def _inside(case, wf, gf):
    return C.check_forward(wf, case), C.check_backward(gf, case)


def _outside(case, wf, gf, forward=True, backward=True):
    if forward:
        with pytest.raises(C.OutsideBound):
            C.check_forward(wf, case)
    if backward:
        with pytest.raises(C.OutsideBound):
            C.check_backward(gf, case)


# ---------------------------------------------------------------------------------------------------------------------
# the restated arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def test_small_div_is_exact_on_its_claimed_range():
    """csrc/kpconv.hip small_div: t / d for 0 <= t < 4096, 1 <= d <= 64"""
    t = np.arange(4096)[:, None]
    d = np.arange(1, 65)[None, :]
    assert np.array_equal(C.small_div(t, d), t // d)
    # the comment's reason: (t + 0.5) / d is at least 1 / 128 from an integer, far more than the two roundings move it
    frac = ((t + 0.5) / d) % 1.0
    assert frac.min() >= 1 / 128 and (1 - frac).min() >= 1 / 128


def test_lds_sizes_fall_where_stated():
    sizes = {w: C.lds_bytes(n_nb, c, n_kp) for w, (c, n_nb, n_kp) in C.LDS_SHAPES.items()}
    assert sizes == {"small": 45632, "mid": 53568, "large": 85440, "max": 103296}
    assert sizes["small"] < 48 * 1024 < sizes["mid"] < 64 * 1024 < sizes["large"] < sizes["max"] <= 160 * 1024
    assert sizes["max"] == max(C.lds_bytes(n, c, k) for n in (1, 63, 64) for c in (1, 63, 64) for k in (1, 31, 32))
    assert C.LDS_SHAPES["max"] == (C.MAX_C, C.MAX_NB, C.MAX_KP)
    assert C.LDS_ORDER[:4] == ("small", "max", "small", "mid") and set(C.LDS_ORDER) == set(C.LDS_SHAPES)
    for w in C.LDS_SHAPES:
        case = C.lds_case(w)
        assert case.lds == sizes[w] and int(case.valid.sum(1).max()) == case.n_nb
    # everything else stays below the opt-in threshold except the sweeps at large c
    assert C.edge_case(32, 64).lds < 48 * 1024 and C.c_sweep_case(64).lds == sizes["max"]
    # the padding of the kernel-point block and the `rows` region sized by n_kp at the edges
    assert [(3 * k + 3) & ~3 for k in C.KP_EDGES] == [4, 8, 48, 48, 96, 96]
    assert any(k > n for k, n in C.EDGE_SHAPES) and any(k < n for k, n in C.EDGE_SHAPES) and (16, 16) not in C.EDGE_SHAPES


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def test_divisor_coverage_is_complete():
    """every divisor d = 1..64 with the largest t each loop can reach: 64 d - 1 and 32 d - 1 for d = c, 32 d - 1 for d = n_valid"""
    for c in range(1, 65):
        case = C.c_sweep_case(c)
        nv = case.valid.sum(1)
        assert (case.c, case.n_nb, case.n_kp, case.n_q) == (c, 64, 32, 130) and int(nv.max()) == 64 and int(nv.min()) < 64
        assert int(nv.max()) * c - 1 == 64 * c - 1 < 4096 and case.n_kp * c - 1 == 32 * c - 1
        assert (np.diff(np.where(case.valid, 0, 1), axis=1) >= 0).all() == bool(c % 2)  # prefix padding on odd c, holes on even
    case = C.n_valid_sweep_case()
    nv = case.valid.sum(1)
    assert sorted(nv.tolist()) == sorted(list(range(65)) * 2) and case.n_kp == 32 and case.n_nb == 64
    assert 32 * 64 - 1 < 4096
    assert any(abs(int(a) - int(b)) >= 32 for a, b in zip(nv[:-1], nv[1:]))  # shuffled
    holes = [(np.diff(np.flatnonzero(v)) > 1).any() for v in case.valid if 2 <= v.sum() < 60]
    assert np.mean(holes) > 0.9                                                # valid entries at scattered positions
    pad = case.nb[~case.valid]
    assert set(np.unique(pad).tolist()) == {-1, case.n_s, C.INT_MAX, C.INT_MIN}


@pytest.mark.parametrize("shape", C.EDGE_SHAPES, ids=lambda s: "kp%d-nb%d" % s)
def test_edge_cases_are_what_they_claim(shape):
    n_kp, n_nb = shape
    case = C.edge_case(n_kp, n_nb)
    nv = case.valid.sum(1)
    assert (case.n_kp, case.n_nb, case.c, case.n_q) == (n_kp, n_nb, 7, 37) and case.n_q % C.KP_WAVES == 1
    assert (nv[:4] == n_nb).all() and nv[4] == 0
    if n_nb == 64:
        assert case.valid[0].all() and case.valid[0, 63]  # lane 63 valid


def test_query_count_and_past_cap_cases():
    assert [C.query_count_case(n).n_q for n in C.QUERY_COUNTS] == [1, 3, 4, 5] and C.KP_WAVES == 4
    case = C.past_cap_case(CUS)
    cap = case.marks["cap"]
    assert cap == 64 * CUS and case.n_q == cap + 3 and (case.c, case.n_nb) == (3, 4)
    nv = case.valid.sum(1)
    # wave w of workgroup 0 takes queries w and cap + w: a full row then an empty one, a full row then one neighbour, one then four
    assert [(int(nv[w]), int(nv[cap + w])) for w in range(3)] == [(4, 0), (4, 1), (1, 4)]


def test_degenerate_supports():
    one = C.single_support_case()
    assert one.n_s == 1 and set(np.unique(one.nb[one.valid]).tolist()) == {0} and 0 < one.valid.sum() < one.valid.size
    none = C.empty_support_case()
    assert none.n_s == 0 and none.n_q > 0 and not none.valid.any() and (none.nb == 0).any()
    ref = none.reference()
    assert ref.wf.shape == (none.n_q, none.n_kp, none.c) and not ref.wf.any() and ref.gf.shape == (0, none.c)


@pytest.mark.parametrize("nonfinite", [False, True])
def test_exact_geometry_is_exact_in_fp32(nonfinite):
    case = C.exact_case(nonfinite)
    ref = case.reference()
    assert case.extent == C.EXACT_EXTENT == 0.3125
    for a in (case.query, case.support, case.kp):
        assert np.array_equal(a * 16, np.round(a * 16)) and np.abs(a).max() < 8  # the lattice: sums and differences are exact
    assert (ref.n_valid == 1).all()
    w32, d32 = C.influences_f32(case)
    kinds = {C.ON: (0.0, 1.0), C.AT_EXTENT: (C.EXACT_EXTENT, 0.0), C.TWICE: (2 * C.EXACT_EXTENT, 0.0)}
    seen = set()
    for i, k, kind in case.marks["designated"]:
        (n,) = np.flatnonzero(ref.valid[i])
        d, w = kinds[kind]
        assert float(d32[i, k, n]) == d == ref.r[i, k, n] * case.extent and float(w32[i, k, n]) == w == ref.w[i, k, n]
        assert not np.signbit(w32[i, k, n])
        seen.add((k, kind))
    assert seen == {(k, kind) for k in range(case.n_kp) for kind in kinds}
    referenced = set(ref.j[ref.valid].tolist())
    assert 0 not in referenced and case.n_s - 1 not in referenced
    assert (np.diff(np.flatnonzero(ref.valid.ravel()) % case.n_nb) != 0).any()  # the one valid entry moves about the row
    # no influence sits where the fp32 clamp could decide differently from the float64 one: exactly on the edge, or well off it
    assert ((ref.r == 1.0) | (np.abs(ref.r - 1.0) > 1e-3))[ref.valid[:, None, :].repeat(case.n_kp, 1)].all()
    if nonfinite:
        assert np.isnan(case.x[0]).all() and np.isnan(case.x[-1]).all()
        for kind, qs in case.marks["poison"].items():
            rows = [int(ref.j[i][ref.valid[i]][0]) for i in qs]
            assert np.isnan(case.x[rows[0]]).all() and np.isinf(case.x[rows[1]]).all() and (case.x[rows[1]] > 0).any() and (case.x[rows[1]] < 0).any()
            assert np.isposinf(case.x[rows[2], 0]) and np.isneginf(case.x[rows[2], 1]) and np.isnan(case.x[rows[2], 2])
        # reached with positive weight: signed infinities; with weight exactly 0: 0 * Inf = NaN; untouched queries stay finite
        i, k, _ = next(d for d in case.marks["designated"] if d[2] == C.ON and d[0] == case.marks["poison"][C.ON][1])
        assert np.array_equal(ref.wf[i, k], case.x[int(ref.j[i][ref.valid[i]][0])].astype(np.float64))
        i, k, _ = next(d for d in case.marks["designated"] if d[2] == C.TWICE and d[0] == case.marks["poison"][C.TWICE][1])
        assert np.isnan(ref.wf[i, k]).all()
        poisoned = {i for qs in case.marks["poison"].values() for i in qs}
        clean = [i for i in range(case.n_q) if i not in poisoned]
        assert np.isfinite(ref.wf[clean]).all() and not np.isfinite(ref.wf[sorted(poisoned)]).all() and np.isfinite(ref.gf).all()
    else:
        assert np.isfinite(ref.wf).all()


def test_off_origin_duplicates_and_nonfinite_coordinates():
    case = C.off_origin_case()
    assert np.allclose(case.support.mean(0), C.OFF_ORIGIN, atol=0.1) and np.allclose(case.query.mean(0), C.OFF_ORIGIN, atol=0.1)
    ref = case.reference()
    assert (ref.w > 0).mean() > 0.05  # the neighbourhood survived the shift
    # the bound follows |support - query|, not the coordinates: their own rounding is in the fp32 inputs, the reference's too
    assert np.abs(ref.bw).max() < 16 * C.U

    dup = C.duplicate_row_case()
    assert (dup.nb[3] == 17).all() and dup.n_nb == 40 and set(dup.nb[4].tolist()) == {5, 9} and dup.reference().hits[17] >= 50
    one = C.one_support_row_case()
    assert not one.nb.any() and one.reference().hits[0] == one.n_q * one.n_nb == 768 and not one.reference().hits[1:].any()

    bad = C.nonfinite_coordinate_case()
    ref = bad.reference()
    assert np.isnan(bad.support[7, 1]) and np.isposinf(bad.support[11, 0]) and np.isnan(bad.query[3, 2]) and np.isposinf(bad.query[9, 0])
    assert np.isnan(ref.wf[3]).all()                                    # a NaN query: everything it reaches
    for i in (0, 5, 21):
        assert np.isnan(ref.wf[i]).all()                                # a NaN support point: every query that lists it
    assert np.isnan(ref.wf[9]).all() and (bad.nb[9] == 11).any()         # Inf - Inf
    assert np.isfinite(ref.wf[1]).all() and (bad.nb[1] == 11).any()      # a finite query, an infinitely far point: weight 0
    n = int(np.flatnonzero(bad.nb[1] == 11)[0])
    assert not ref.w[1, :, n].any() and not ref.bw[1, :, n].any()
    assert np.isnan(ref.gf[7]).all() and np.isnan(ref.gf[11]).all()      # 11 through query 9
    touched_by_bad_query = set(bad.nb[3][bad.valid[3]].tolist()) | set(bad.nb[9][bad.valid[9]].tolist())
    clean = [j for j in range(bad.n_s) if j not in touched_by_bad_query | {7, 11}]
    assert len(clean) > 30 and np.isfinite(ref.gf[clean]).all()

    far = C.out_of_int32_neighbours(C.plain_case())
    assert far.dtype == np.int64 and np.array_equal((far >= 0) & (far < C.plain_case().n_s), C.plain_case().valid)
    low = far[~C.plain_case().valid].astype(np.int32)                   # what a plain narrowing would leave
    assert ((low >= 0) & (low < C.plain_case().n_s)).any()


# ---------------------------------------------------------------------------------------------------------------------
# margin: plain fp32 is inside every bound
# ---------------------------------------------------------------------------------------------------------------------
def test_fp32_evaluation_is_inside_every_bound(capsys):
    worst = [0.0, 0.0]
    for case in _finite_cases():
        f, b = _inside(case, *C.evaluate_f32(case))
        worst = [max(worst[0], f), max(worst[1], b)]
        assert np.isfinite(case.reference().wf).all() and np.isfinite(case.reference().gf).all()
    for case in (C.exact_case(True), C.nonfinite_coordinate_case()):
        _inside(case, *C.evaluate_f32(case))
    C.check_exact_geometry(C.evaluate_f32(C.exact_case())[0], C.exact_case())
    C.check_exact_geometry(C.evaluate_f32(C.exact_case(True))[0], C.exact_case(True))
    with capsys.disabled():
        print(f"\nfraction kpconv_fwd fp32-numpy {worst[0]:.3f}\nfraction kpconv_bwd fp32-numpy {worst[1]:.3f}")
    assert 0.0 < worst[0] <= 1.0 and 0.0 < worst[1] <= 1.0


def test_fp32_evaluation_is_inside_the_bounds_of_the_c_sweep():
    for c in range(1, 65):
        case = C.c_sweep_case(c)
        _inside(case, *C.evaluate_f32(case))


# ---------------------------------------------------------------------------------------------------------------------
# selectivity: wrong variants are outside
# ---------------------------------------------------------------------------------------------------------------------
def _selectivity_cases():
    return [C.n_valid_sweep_case(), C.plain_case(), C.edge_case(2, 63), C.edge_case(32, 1), C.duplicate_row_case(), C.exact_case()]


def test_influence_against_the_next_kernel_point_is_outside():
    for case in _selectivity_cases() + [C.lds_case("mid"), C.off_origin_case()]:
        _outside(case, *C.variant_next_kernel_point(case))


def test_one_dropped_neighbour_of_small_weight_is_outside():
    for case in _selectivity_cases()[:5] + [C.query_count_case(5), C.off_origin_case()]:
        i, n = C.small_neighbour(case)
        assert 1e-3 <= case.reference().w[i, :, n].max() < 0.2
        _outside(case, *C.variant_dropped_neighbour(case))
    # 768 atomics on one row: the backward's bound grows with the hits and one small term of 768 fits in it; the forward's does not
    case = C.one_support_row_case()
    _outside(case, *C.variant_dropped_neighbour(case), backward=False)


def test_unclamped_negative_influence_is_outside():
    for case in _selectivity_cases() + [C.single_support_case()]:
        _outside(case, *C.variant_unclamped(case))
    # ... also where the overshoot is as small as it gets: a neighbour 1 % beyond the extent of every kernel point but one
    case = C.exact_case()
    w = C.influences_f32(case, clamp=False)[0]
    assert w.min() == -1.0 or w.min() < -1.0


def test_a_quotient_off_by_one_is_outside():
    """at a single (t, d), for each of the three divisions: the forward's output index, the backward's slot index (d = c) and
    the influence index (d = n_valid)"""
    for c, t in ((1, 31), (3, 3 * 32 - 1), (7, 7), (64, 64 * 32 - 1), (63, 63 * 17 + 5)):
        case = C.c_sweep_case(c)
        _outside(case, *C.variant_quotient_forward(case, t), backward=False)
    for c, t in ((1, 63), (3, 3 * 64 - 1), (7, 7), (64, 64 * 64 - 1), (33, 33 * 40 + 2)):
        case = C.c_sweep_case(c)
        _outside(case, *C.variant_quotient_backward(case, t), forward=False)
    case = C.n_valid_sweep_case()
    ref = case.reference()
    for n_valid in (2, 3, 5, 33, 63, 64):  # (the two rows with one neighbour have no positive influence at k >= 1)
        rows = np.flatnonzero(ref.n_valid == n_valid)
        order = np.argsort(~case.valid, axis=1, kind="stable")
        # a (k, n) whose influence is positive in one of the rows with this count
        k, n = next((k, n) for k in range(1, case.n_kp) for n in range(n_valid) if (ref.w[rows, k, order[rows, n]] > 1e-2).any())
        _outside(case, *C.variant_quotient_influence(case, k * n_valid + n, n_valid))
