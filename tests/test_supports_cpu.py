"""CPU: the oracle of cluster.clean_supports (tests/supports_oracle.py) on hand-made cases whose results are written out by hand and on
the five supports of the two golden object scenes (tests/golden/objects_reference.npz), the declarations of csrc/supports.hip's launchers,
and every argument check that needs no GPU.  No HIP compute runs here."""
import inspect
import os

import numpy as np
import pytest
import torch

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, cluster
from tests import supports_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = torch.int64
F32 = np.float32


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


# ---- the oracle on cases small enough to work out by hand (voxel 0.25: origin = lo - 0.125, faces at lo + 0.125 + 0.25 k, all exact) ----
def test_four_points_in_one_voxel_give_their_float64_mean():
    xyz = np.array([[0, 0, 0], [2 ** -7, 2 ** -6, 0], [2 ** -6, 0, 2 ** -4], [2 ** -7, 2 ** -6, 2 ** -4]], F32)
    index, mean, size = O.voxel_means(xyz, 0.25)
    assert index.tolist() == [[0, 0, 0]] and size.tolist() == [4]
    assert mean.dtype == F32 and mean.tolist() == [[2 ** -7, 2 ** -7, 2 ** -5]]
    # a sum that fp32 would round at every step and float64 holds exactly: fp32(0.995) + 1 + 1 + 1, divided by 4 (exact), rounded ONCE
    # to fp32; with lo = fp32(0.995) the voxel is [0.975, 1.015)
    xyz = np.array([[0.995, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]], F32)
    index, mean, size = O.voxel_means(xyz, 0.04)
    assert size.tolist() == [4] and mean[0, 0] == F32((np.float64(F32(0.995)) + 3.0) / 4.0)
    points, obj, source, n = O.clean_supports(xyz, np.zeros(4, int), nb_points=0)
    assert n == 1 and points.shape == (1, 3) and obj.tolist() == [0] and source.tolist() == [0]


def test_a_point_on_each_side_of_a_voxel_face():
    below = np.nextafter(F32(0.125), F32(0))
    for axis in range(3):
        xyz = np.zeros((3, 3), F32)
        xyz[1, axis], xyz[2, axis] = below, 0.125                         # lo = 0: the face between voxel 0 and 1 is at exactly 0.125
        index, mean, size = O.voxel_means(xyz, 0.25)
        assert index[:, axis].tolist() == [0, 1] and size.tolist() == [2, 1]
        assert mean[0, axis] == below / 2 and mean[1, axis] == F32(0.125)  # halving is exact
    # negative coordinates: floor, not truncation - with lo = -1 the point -0.9 is 0.225 above the origin: voxel 0, and -0.87 voxel 1
    xyz = np.array([[-1, 0, 0], [-0.9, 0, 0], [-0.87, 0, 0]], F32)
    index, _, size = O.voxel_means(xyz, 0.25)
    assert index[:, 0].tolist() == [0, 1] and size.tolist() == [2, 1]
    # the order of the voxels: vz slowest, vx fastest
    xyz = np.array([[0.3, 0, 0], [0, 0.3, 0], [0, 0, 0.3], [0, 0, 0]], F32)
    index, mean, _ = O.voxel_means(xyz, 0.25)
    assert index.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]


def _square(at=0.0):
    return np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0.25, 0.25, 0]], F32) + F32(at)


def test_a_lattice_with_exactly_nb_points_and_one_more_neighbour():
    """four means on a square of edge 0.25: within 0.3 each has itself and its two neighbours (3), within 0.36 the diagonal too (4)"""
    xyz = _square()
    assert O.near_counts(xyz, 0.3).tolist() == [3] * 4 and O.near_counts(xyz, 0.36).tolist() == [4] * 4
    assert O.near_counts(xyz, 0.25).tolist() == [1] * 4                    # strict: a neighbour at exactly the radius is not in reach
    label = np.zeros(4, int)
    assert O.clean_supports(xyz, label, voxel=0.25, radius=0.3, nb_points=3)[3] == 0           # exactly nb_points: removed
    points, obj, source, n = O.clean_supports(xyz, label, voxel=0.25, radius=0.36, nb_points=3)   # one more: kept
    assert n == 1 and np.array_equal(points, xyz[[0, 1, 2, 3]]) and obj.tolist() == [0] * 4
    points, _, _, n = O.clean_supports(xyz, label, voxel=0.25, radius=0.3, nb_points=2)
    assert n == 1 and len(points) == 4
    # the point itself counts: nb_points = 0 keeps an isolated point
    assert O.clean_supports(xyz[:1], label[:1], nb_points=0)[3] == 1 and O.clean_supports(xyz[:1], label[:1], nb_points=1)[3] == 0


def test_an_object_that_vanishes_and_the_renumbering_around_it():
    stray = np.array([[5, 5, 5], [7, 5, 5], [5, 7, 5]], F32)               # three isolated points: every count is 1
    xyz = np.concatenate([_square(0), stray, _square(2), np.full((1, 3), 9, F32)])
    label = np.array([0] * 4 + [1] * 3 + [3] * 4 + [-1])                   # number 2 has no point at all, the last point no object
    detail = {}
    points, obj, source, n = O.clean_supports(xyz, label, 5, voxel=0.25, radius=0.36, nb_points=3, detail=detail)
    assert n == 2 and source.tolist() == [0, 3] and obj.tolist() == [0] * 4 + [1] * 4
    assert np.array_equal(points, np.concatenate([_square(0), _square(2)]))
    assert sorted(detail) == [0, 1, 3] and detail[1][3].tolist() == [1, 1, 1]
    # the neighbours of another object do not count: the same square split over two objects loses everything
    assert O.clean_supports(_square(), np.array([0, 0, 1, 1]), voxel=0.25, radius=0.36, nb_points=3)[3] == 0
    assert O.clean_supports(np.zeros((0, 3), F32), np.zeros(0, int), 3)[3] == 0


# ---- the golden object scenes ----
@pytest.mark.parametrize("s,before,after", [("a", [1229, 5287], [528, 2277]), ("b", [2941, 2513, 429], [1278, 1071, 192])])
def test_the_golden_supports_shrink_to_the_recorded_voxel_counts_and_keep_every_mean(s, before, after):
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "objects_reference.npz"), allow_pickle=False))
    coord, obj, n = gold[f"coord_{s}"], gold[f"object_{s}"], int(gold[f"n_objects_{s}"])
    assert np.bincount(obj[obj >= 0], minlength=n).tolist() == before
    detail = {}
    points, new_obj, source, n_new = O.clean_supports(coord, obj, n, detail=detail)
    assert [len(detail[o][1]) for o in range(n)] == after and max(int(detail[o][2].max()) for o in range(n)) <= 4
    assert n_new == n and source.tolist() == list(range(n)) and np.bincount(new_obj).tolist() == after      # every mean is kept
    assert points.dtype == F32 and new_obj.dtype == np.int32 and source.dtype == np.int32
    for o in range(n):                                                     # a mean lies in its object's box
        mine = coord[obj == o]
        assert (points[new_obj == o] >= mine.min(0)).all() and (points[new_obj == o] <= mine.max(0)).all()


# ---- declarations ----
def test_launchers_are_declared_and_exported():
    makefile = open(os.path.join(ROOT, "stratified_transformer_amd", "csrc", "Makefile")).read()
    assert "supports.hip" in makefile


def test_public_interface():
    assert sta.clean_supports is cluster.clean_supports and sta.box_supports is cluster.box_supports
    assert {"clean_supports", "box_supports"} <= set(sta.__all__)
    assert (cluster.SUPPORT_VOXEL, cluster.SUPPORT_RADIUS, cluster.SUPPORT_NB_POINTS) == (0.04, 0.1, 3)
    assert str(inspect.signature(cluster.clean_supports)) == "(coord, obj, n_objects=None, voxel=0.04, radius=0.1, nb_points=3)"
    assert list(inspect.signature(cluster.box_supports).parameters)[:3] == ["coord", "shift", "pred"]
    assert set(cluster.LAST_SUPPORTS) == {"launches", "readbacks"}
    doc = cluster.clean_supports.__doc__
    assert "UNPINNED" in doc and "rounded ONCE to fp32" in doc and "strict" in doc and "hash map" in doc
    assert "not reproduced; the Open3D" in cluster.objects.__doc__ and "clean_supports" in cluster.objects.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.14" in design and "clean_supports" in design[design.index("### 4.12"):design.index("### 4.13")]


# ---- host-side rejections ----
GOOD = (torch.zeros(10, 3), torch.zeros(10, dtype=L))


def test_cpu_tensors_raise_no_cpu_fallback():
    xyz, label = GOOD
    for a, b in ((xyz, label), (_OnGpu(xyz), label), (xyz, _OnGpu(label))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.clean_supports(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.box_supports(xyz, xyz, label)


@pytest.mark.parametrize("xyz,label,kw,error", [
    (torch.zeros(10, 2), GOOD[1], {}, ValueError),                                  # coord not [N, 3]
    (torch.zeros(30), GOOD[1], {}, ValueError),
    (torch.zeros(10, 3, dtype=torch.float64), GOOD[1], {}, TypeError),
    (GOOD[0], torch.zeros(9, dtype=L), {}, ValueError),                             # obj not [N]
    (GOOD[0], torch.zeros(10, 1, dtype=L), {}, ValueError),
    (GOOD[0], torch.zeros(10), {}, TypeError),                                      # obj dtype
    (GOOD[0], torch.zeros(10, dtype=torch.int16), {}, TypeError),
    (GOOD[0], GOOD[1], {"n_objects": -1}, ValueError),
    (GOOD[0], GOOD[1], {"n_objects": 2.0}, TypeError),
    (GOOD[0], GOOD[1], {"n_objects": True}, TypeError),
    (GOOD[0], GOOD[1], {"n_objects": cluster.MAX_LABELS + 1}, ValueError),
    (GOOD[0], GOOD[1], {"radius": 0.0}, ValueError),
    (GOOD[0], GOOD[1], {"radius": -0.1}, ValueError),
    (GOOD[0], GOOD[1], {"radius": float("nan")}, ValueError),
    (GOOD[0], GOOD[1], {"radius": float("inf")}, ValueError),
    (GOOD[0], GOOD[1], {"radius": 1e-30}, ValueError),                              # underflows in fp32
    (GOOD[0], GOOD[1], {"radius": "0.1"}, TypeError),
    (GOOD[0], GOOD[1], {"voxel": 0.0}, ValueError),
    (GOOD[0], GOOD[1], {"voxel": -0.04}, ValueError),
    (GOOD[0], GOOD[1], {"voxel": float("nan")}, ValueError),
    (GOOD[0], GOOD[1], {"voxel": float("inf")}, ValueError),
    (GOOD[0], GOOD[1], {"voxel": "0.04"}, TypeError),
    (GOOD[0], GOOD[1], {"voxel": True}, TypeError),
    (GOOD[0], GOOD[1], {"nb_points": -1}, ValueError),
    (GOOD[0], GOOD[1], {"nb_points": 2.5}, ValueError),
    (GOOD[0], GOOD[1], {"nb_points": True}, ValueError),
    (GOOD[0], GOOD[1], {"nb_points": 2 ** 31}, ValueError),
])
def test_clean_supports_rejects_bad_arguments_before_any_launch(xyz, label, kw, error):
    calls = _lib.CALLS[0]
    with pytest.raises(error, match="clean_supports"):
        cluster.clean_supports(_OnGpu(xyz), _OnGpu(label), **kw)
    assert _lib.CALLS[0] == calls


def test_box_supports_checks_the_clean_up_settings_before_the_first_step():
    calls = _lib.CALLS[0]
    xyz, pred = _OnGpu(torch.rand(10, 3)), _OnGpu(torch.zeros(10, dtype=L))
    for kw in ({"voxel": 0.0}, {"radius": float("nan")}, {"nb_points": -1}):
        with pytest.raises(ValueError, match="clean_supports"):
            cluster.box_supports(xyz, xyz, pred, **kw)
    assert _lib.CALLS[0] == calls


def test_the_checks_behind_the_first_read_back_raise_before_any_launch():
    calls = _lib.CALLS[0]
    xyz, label = torch.zeros(10, 3), torch.zeros(10, dtype=L)
    with pytest.raises(ValueError, match="label values"):
        cluster.clean_supports(_OnGpu(xyz), _OnGpu(label + 3), 3)             # a label beyond the count
    with pytest.raises(ValueError, match="label values"):
        cluster.clean_supports(_OnGpu(xyz), _OnGpu(label - 2))                # below -1
    for bad_value in (float("nan"), float("inf")):
        bad = xyz.clone()
        bad[3, 1] = bad_value
        with pytest.raises(ValueError, match="finite"):
            cluster.clean_supports(_OnGpu(bad), _OnGpu(label))
    wide = xyz.clone()
    wide[0, 0] = 1e6                                                          # 2.5e7 voxels along x: more than MAX_CELLS_PER_AXIS
    with pytest.raises(ValueError, match="voxel keys"):
        cluster.clean_supports(_OnGpu(wide), _OnGpu(label))
    wide[0] = 2e4                                                             # 5e5 voxels per axis: fine per axis, 1.25e17 in all - times 300
    with pytest.raises(ValueError, match="voxel keys"):
        cluster.clean_supports(_OnGpu(wide), _OnGpu(label), 300)
    with pytest.raises(ValueError, match="voxel keys"):
        cluster.clean_supports(_OnGpu(xyz + torch.arange(10)[:, None]), _OnGpu(label), voxel=1e-300)
    wide[0] = 3e3                                                             # the voxels fit (coarse ones), the cells of the radius grid do not
    with pytest.raises(ValueError, match="cells"):
        cluster.clean_supports(_OnGpu(wide), _OnGpu(label), 300, voxel=1.0, radius=0.001)
    assert _lib.CALLS[0] == calls


def test_no_points_returns_the_empty_results_without_a_launch():
    calls = _lib.CALLS[0]
    empty = (_OnGpu(torch.zeros(0, 3)), _OnGpu(torch.zeros(0, dtype=L)))
    for args in ((), (3,)):
        points, obj, source, n = cluster.clean_supports(*empty, *args)
        assert points.shape == (0, 3) and points.dtype == torch.float32 and obj.shape == (0,) and obj.dtype == torch.int32
        assert source.shape == (0,) and source.dtype == torch.int32 and n == 0
    assert cluster.LAST_SUPPORTS == {"launches": 0, "readbacks": 0}
    points, obj, source, n = cluster.clean_supports(_OnGpu(torch.rand(20, 3)), _OnGpu(torch.full((20,), -1, dtype=L)), 4)
    assert points.shape == (0, 3) and n == 0 and cluster.LAST_SUPPORTS == {"launches": 0, "readbacks": 1}
    assert _lib.CALLS[0] == calls
