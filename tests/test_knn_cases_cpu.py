"""CPU: the kNN cases of tests/knn_cases.py are what they claim to be, so that a pass of tests/test_knn_hip.py cannot be hollow.
The kernel of every case follows from its sizes by the launcher's own conditions; the tie content (what reaches the replay list and
what does not) and the exactness of the translation family are established with the oracle.  No HIP compute runs here."""
import numpy as np
import pytest

from oracle import pointops_ref as ref
from tests import knn_cases as C

ALL = sorted(C.CASES)


def _tie_rows(case):
    """per query: do two of its k + 1 best distances coincide (fillers excluded)?  That is the test knn_grid_kernel /
    knn_lanes_kernel apply before they hand a query to knn_replay_kernel.  (The oracle's rows are ascending; sqrt keeps
    equal distances equal.)"""
    _, d = ref.knnquery(case.k + 1, case.xyz, case.new_xyz, case.offset, case.new_offset)
    real = d[:, :-1] < np.float32(1e5)
    return ((d[:, :-1] == d[:, 1:]) & real).any(1)


def _expected_kernel(k, m, n):
    if m * n < (1 << 22):
        return C.SCAN
    if k + 1 <= 16:
        return C.LANES16
    if k + 1 <= 32:
        return C.LANES32
    if k + 1 <= 64:
        return C.LANES64
    return C.GRID


@pytest.mark.parametrize("name", ALL)
def test_the_table_names_the_kernel_the_sizes_select(name):
    c = C.CASES[name]
    n, m = len(c.xyz), len(c.new_xyz)
    assert 1 <= c.k <= 100 and n <= 8000 and m <= 2000
    assert C.kernel_of(c) == _expected_kernel(c.k, m, n)
    assert c.xyz.dtype == c.new_xyz.dtype == np.float32 and c.offset.dtype == c.new_offset.dtype == np.int32
    assert np.isfinite(c.xyz).all() and np.isfinite(c.new_xyz).all()
    assert (np.diff(c.offset) > 0).all() and (np.diff(c.new_offset) > 0).all()
    if C.kernel_of(c) != C.SCAN:   # grid cases sit at the smallest size the launcher sends to the grid, or just above it
        assert n * m >= C.GRID_THRESHOLD and n <= 4096 + 65 and m <= 1024 + 65


def test_every_kernel_and_lane_boundary_has_a_case():
    used = {(C.kernel_of(c), c.k) for c in C.CASES.values()}
    for want in ((C.SCAN, 3), (C.SCAN, 100), (C.GRID, 64), (C.GRID, 100),
                 (C.LANES16, 15), (C.LANES32, 16), (C.LANES32, 31), (C.LANES64, 32), (C.LANES64, 63)):
        assert want in used, want
    for lq, kernel in ((16, C.LANES16), (32, C.LANES32), (64, C.LANES64)):
        assert (kernel, lq - 1) in used                      # k + 1 == LQ: the group is exactly full
    assert set(C.REPLAY_FAMILIES) <= set(C.KERNELS)


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith("sweep_random")])
def test_random_sweep_clouds_have_no_exact_ties(name):
    assert not _tie_rows(C.CASES[name]).any()


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith("sweep_mixed")])
def test_mixed_sweep_clouds_split_between_replay_and_direct(name):
    c = C.CASES[name]
    tie = _tie_rows(c)
    assert 0.2 <= tie.mean() <= 0.8, tie.mean()
    assert tie[c.lattice_queries].all()                      # every lattice query is replayed
    assert c.lattice_queries.sum() * 2 == len(tie)
    # both batch elements (where there are two) carry both kinds
    lo = 0
    for hi in c.new_offset:
        assert tie[lo:hi].any() and not tie[lo:hi].all()
        lo = hi


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith(("scan_lattice", "coincident"))])
def test_lattice_and_coincident_queries_all_tie(name):
    c = C.CASES[name]
    assert _tie_rows(c)[c.lattice_queries].all() and c.lattice_queries.all()


@pytest.mark.parametrize("k", C.BOUNDARY_KS)
def test_boundary_tie_cases_tie_in_the_last_slot_only_and_the_heap_keeps_the_higher_index(k):
    """queries whose single exact tie is between the k-th and the (k+1)-th best, and for which the heap's k-th neighbour is the
    HIGHER of the two indices: a kernel that does not see that tie (it has to compare slot k - 1 with slot k) writes the lower
    index and fails on every one of them.  At least 16 per case."""
    c = C.CASES[f"boundary_tie-k{k}"]
    i1, d1 = ref.knnquery(k + 1, c.xyz, c.new_xyz, c.offset, c.new_offset)
    i0, _ = ref.knnquery(k, c.xyz, c.new_xyz, c.offset, c.new_offset)
    eq = d1[:, :-1] == d1[:, 1:]
    last_only = eq[:, -1] & ~eq[:, :-1].any(1)
    assert np.array_equal(i0[last_only, :k - 1], i1[last_only, :k - 1])     # the k - 1 nearer ones are distinct: no choice there
    keeps_higher = last_only & (i0[:, k - 1] == i1[:, k - 1:].max(1))
    assert keeps_higher.sum() >= 16, keeps_higher.sum()
    assert (~eq.any(1)).sum() >= 256                                        # and queries without any tie beside them


def test_threshold_pair_is_one_cloud_on_both_sides_of_the_line():
    a, b = C.CASES["threshold_below-k16"], C.CASES["threshold_at-k16"]
    assert len(a.xyz) == 4095 and len(b.xyz) == 4096 and len(a.new_xyz) == len(b.new_xyz) == 1024
    assert np.array_equal(a.xyz, b.xyz[:4095]) and np.array_equal(a.new_xyz, b.new_xyz)
    assert len(a.xyz) * 1024 < C.GRID_THRESHOLD == len(b.xyz) * 1024


@pytest.mark.parametrize("family", ["scan_random", "scan_lattice"])
def test_scan_cases_put_three_elements_and_tile_cuts_under_one_workgroup(family):
    for k in C.SCAN_KS:
        c = C.CASES[f"{family}-k{k}"]
        assert c.offset.tolist() == [30, 2300, 5000] and c.new_offset.tolist() == [10, 50, 800]
        assert c.new_offset[1] < 64 <= c.new_offset[2]        # queries 0..63 (workgroup 0) reach into the third element
        assert c.offset[0] < 2048 < c.offset[1] < 4096 < c.offset[2]   # tile boundaries inside elements 1 and 2


def test_short_elements_have_k_minus_one_k_and_k_plus_one_points():
    for k in C.SHORT_KS:
        for family, delta in (("short_km1", -1), ("short_k", 0), ("short_kp1", 1)):
            c = C.CASES[f"{family}-k{k}"]
            assert c.offset.tolist() == [k + delta, k + delta + 4096] and c.new_offset.tolist() == [k + delta, k + delta + 1024]
            _, d = ref.knnquery(k + 1, c.xyz, c.new_xyz, c.offset, c.new_offset)
            first = d[: k + delta]
            filler = np.sqrt(np.float32(1e10))
            assert ((first == filler).sum(1) == 1 - delta).all()           # 2, 1, 0 unfilled slots among the k + 1 best
            assert (d[k + delta:] < 2.0).all()                              # the ordinary element fills every slot


def test_degenerate_clouds_are_degenerate():
    for k in C.DEGENERATE_KS:
        ext = lambda name: np.ptp(C.CASES[f"{name}-k{k}"].xyz, axis=0)
        assert (ext("planar") > 0.9).tolist() == [True, True, False] and ext("planar")[2] == 0
        assert ext("collinear")[0] > 0.9 and ext("collinear")[1] == 0 and ext("collinear")[2] == 0
        assert (ext("coincident") == 0).all()
        far = C.CASES[f"far_apart-k{k}"]
        assert far.xyz[2048:, 0].min() - far.xyz[:2048, 0].max() > 999 and far.offset.tolist() == [2048, 4096]
        assert (far.new_xyz[:512, 0] < 2).all() and (far.new_xyz[512:, 0] > 999).all()


@pytest.mark.parametrize("k", C.DEGENERATE_KS)
def test_translation_changes_nothing_for_the_oracle(k):
    """the builder's exactness argument: coordinates stay multiples of 1/256, and the full scan returns the same indices and the
    same distances, bit for bit, at every T"""
    base = C.CASES[f"translate_0-k{k}"]
    i0, d0 = ref.knnquery(k, base.xyz, base.new_xyz, base.offset, base.new_offset)
    tie0 = _tie_rows(base)
    assert tie0.sum() >= 16 and (~tie0).sum() >= 900    # most queries stay on the grid's own path (the stopping rule), some are replayed
    for T in C.TRANSLATIONS:
        c = C.CASES[f"translate_{T}-k{k}"]
        for a, a0 in ((c.xyz, base.xyz), (c.new_xyz, base.new_xyz)):
            assert np.array_equal(a.astype(np.float64) - T, a0.astype(np.float64))   # the translation was exact
            assert np.array_equal(a * 256, np.round(a * 256))
        i, d = ref.knnquery(k, c.xyz, c.new_xyz, c.offset, c.new_offset)
        assert np.array_equal(i, i0) and np.array_equal(d, d0), T
