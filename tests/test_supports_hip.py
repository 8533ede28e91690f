"""GPU (-m gpu): stratified_transformer_amd.cluster.clean_supports / box_supports on csrc/supports.hip against the restatement of
tests/supports_oracle.py evaluated on the CPU.  No tolerance anywhere: the points are compared as bit patterns (a mean is one float64 sum
in a fixed order, one division and one rounding), objects and sources as integers."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import supports_oracle as O
from tests.util import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LAUNCHES = 6        # label_boxes, voxel keys, means, grid keys, grid prepare, count


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def C():
    from stratified_transformer_amd import cluster
    return cluster


def _same(got, want, what):
    points, obj, source, n = got
    assert points.dtype == torch.float32 and obj.dtype == torch.int32 and source.dtype == torch.int32 and isinstance(n, int)
    points, obj, source = points.cpu().numpy(), obj.cpu().numpy(), source.cpu().numpy()
    assert n == want[3] and source.tolist() == want[2].tolist(), f"{what}: objects {source.tolist()} for {want[2].tolist()}"
    assert points.shape == want[0].shape and obj.shape == want[1].shape, f"{what}: {points.shape[0]} points for {want[0].shape[0]}"
    assert np.array_equal(obj, want[1]), f"{what}: objects differ"
    assert np.array_equal(points.view(np.int32), want[0].view(np.int32)), f"{what}: points differ at {np.argwhere(points.view(np.int32) != want[0].view(np.int32))[:10].tolist()}"


def _check(C, xyz, obj, n_objects=None, what="", **kw):
    """clean_supports on the device equals the oracle -> (the oracle's result, its detail per object)"""
    xyz, obj = np.asarray(xyz, F32), np.asarray(obj)
    got = C.clean_supports(dev(xyz), dev(obj), n_objects, **kw)
    torch.cuda.synchronize()
    calls = dict(C.LAST_SUPPORTS)
    detail = {}
    want = O.clean_supports(xyz, obj, n_objects, detail=detail, **kw)
    voxels = sum(len(d[1]) for d in detail.values())
    print(f"{what}: n {len(xyz)}, objects {len(detail)} -> {want[3]}, voxels {voxels}, kept {len(want[0])}, longest run "
          f"{max([int(d[2].max()) for d in detail.values()], default=0)}, {calls}")
    _same(got, want, what)
    return want, detail, calls


def _blobs(n, seed, n_blobs, sigma=0.05, extent=2.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, extent, (n_blobs, 3))
    which = rng.integers(0, n_blobs, n)
    which[:min(n, n_blobs)] = np.arange(min(n, n_blobs))                  # every blob is there, the last one included
    return (centres[which] + rng.normal(0, sigma, (n, 3))).astype(F32), which


# ---- sizes ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_wave_and_block_edges_in_the_number_of_points(C, n):
    rng = np.random.default_rng(n)
    xyz = rng.uniform(-0.5, 0.5, (n, 3)).astype(F32) * F32(0.06 * n ** (1 / 3))
    obj = rng.integers(0, 3, n)
    for nb_points in (0, 3):
        want, detail, _ = _check(C, xyz, obj, 3, what=f"n {n}, nb_points {nb_points}", nb_points=nb_points)
        if nb_points == 0:
            assert len(want[0]) == sum(len(d[1]) for d in detail.values()) >= 1          # every mean is kept: the means themselves
    if n == 5000:
        assert 0 < len(want[0]) < sum(len(d[1]) for d in detail.values())                 # at 3: some removed, some kept


@pytest.mark.parametrize("n_objects", [1, 2, 64, 65, 300])
def test_the_number_of_objects(C, n_objects):
    xyz, obj = _blobs(3000, n_objects, n_objects, extent=1.0 + 0.01 * n_objects)
    want, detail, _ = _check(C, xyz, obj, what=f"objects {n_objects}")
    assert len(detail) == n_objects and want[3] >= 1


# ---- long runs ----
def test_voxels_of_300_and_1000_points_across_wave_and_workgroup_boundaries(C):
    """200 single-point voxels at z = 0, then one voxel of 300 points (sorted positions 200 .. 499: across the wave boundary at 256, which is
    the workgroup's too) and one of 1000 (500 .. 1499); the points shuffled, so the order of summation is the stable sort's work"""
    rng = np.random.default_rng(5)
    row = np.stack([np.arange(200) * 0.04, np.zeros(200), np.zeros(200)], 1)
    big = [np.array([0.0, 0.0, z]) + rng.uniform(0, 0.015, (k, 3)) * [1, 1, 0.5] for z, k in ((0.08, 300), (0.16, 1000))]
    xyz = np.concatenate([row] + big).astype(F32)
    xyz = xyz[rng.permutation(len(xyz))]
    want, detail, _ = _check(C, xyz, np.zeros(len(xyz), int), what="long runs", nb_points=0)
    index, _, size, _ = detail[0]
    assert size.tolist() == [1] * 200 + [300, 1000] and index[200:].tolist() == [[0, 0, 2], [0, 0, 4]] and len(want[0]) == 202


def test_a_cloud_of_identical_points_is_one_mean_of_count_one(C):
    xyz = np.full((700, 3), 0.37, F32) * np.array([1, -2, 3], F32)
    want, detail, calls = _check(C, xyz, np.zeros(700, int), what="identical, nb_points 3")
    assert want[3] == 0 and detail[0][2].tolist() == [700] and detail[0][3].tolist() == [1] and calls["launches"] == LAUNCHES
    want, _, _ = _check(C, xyz, np.zeros(700, int), what="identical, nb_points 0", nb_points=0)
    assert want[0].shape == (1, 3)


# ---- voxel faces ----
@pytest.mark.parametrize("base", [(0.0, 0.0, 0.0), (-3.7, -2.2, -1.9), (1000.0, 1000.0, 1000.0)])
@pytest.mark.parametrize("voxel", [0.04, 0.25])
def test_points_on_voxel_faces_and_a_step_to_either_side(C, base, voxel):
    """faces lie at lo + (k + 0.5) * voxel: the fp32 value nearest to each, and its two neighbours, on every axis - negative coordinates,
    where floor and truncation differ, and 1000 m from the origin, where an fp32 step is 6e-5"""
    lo = np.array(base, F32)
    pts = [lo.copy()]
    for axis in range(3):
        for k in range(6):
            face = F32(np.float64(lo[axis]) + (k + 0.5) * voxel)
            for v in (np.nextafter(face, F32(-np.inf)), face, np.nextafter(face, F32(np.inf))):
                p = lo.copy()
                p[axis] = v
                pts.append(p)
    xyz = np.array(pts, F32)[np.random.default_rng(1).permutation(len(pts))]
    want, detail, _ = _check(C, xyz, np.zeros(len(xyz), int), what=f"faces at {base}, voxel {voxel}", voxel=voxel, nb_points=0)
    index, _, size, _ = detail[0]
    assert 12 <= len(index) <= 19 and size.sum() == 55 and index.min() == 0 and index.max() == 6
    two = np.concatenate([xyz, xyz + F32(0.013)])                         # a second object with another minimum: other faces, same space
    _check(C, two, np.repeat([0, 1], len(xyz)), what="two minima", voxel=voxel, nb_points=0)


# ---- interleaved objects ----
def test_interleaved_objects_do_not_share_voxels_or_neighbours(C):
    """object 4: a 4 x 4 x 3 lattice of 48 points at spacing 0.04; object 1: three points in its middle (2 neighbours of their own, more than
    30 of the other object within reach: removed) and a 2 x 2 x 2 lattice apart (kept); unlabelled points among them, gaps in the numbers"""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 0.04
    three = np.array([[0.039, 0.06, 0.04], [0.081, 0.06, 0.04], [0.06, 0.06, 0.081]])
    apart = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3) * 0.05 + [0.6, 0.0, 0.0]
    loose = np.random.default_rng(2).uniform(0, 0.12, (20, 3))
    xyz = np.concatenate([g, three, apart, loose]).astype(F32)
    obj = np.array([4] * 48 + [1] * 3 + [1] * 8 + [-1] * 20)
    perm = np.random.default_rng(3).permutation(len(obj))
    xyz, obj = xyz[perm], obj[perm]
    want, detail, _ = _check(C, xyz, obj, 6, what="interleaved")
    index, mean, size, count = detail[1]
    assert size.tolist() == [1] * 11 and sorted(count.tolist()) == [3] * 3 + [8] * 8
    lattice = detail[4][1]
    for m in mean[count == 3]:
        assert (O.near_counts(np.concatenate([m[None], lattice]), 0.1)[0] - 1) >= 30
    assert detail[4][2].tolist() == [1] * 48 and want[2].tolist() == [1, 4] and np.bincount(want[1]).tolist() == [8, 48]
    # without the unlabelled points: the same
    again = O.clean_supports(xyz[obj >= 0], obj[obj >= 0], 6)
    assert all(np.array_equal(a, b) for a, b in zip(want[:3], again[:3]))


# ---- exact lattices ----
def test_a_lattice_at_spacing_exactly_the_radius_and_a_step_to_either_side(C):
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    xyz = (g * 0.25).astype(F32)[np.random.default_rng(1).permutation(64)]
    obj = np.zeros(64, int)
    below, above = float(np.nextafter(F32(0.25), F32(0))), float(np.nextafter(F32(0.25), F32(1)))
    for radius in (below, 0.25):                                          # strict: d2 == r2 at exactly 0.25 - nobody has a neighbour
        want, detail, _ = _check(C, xyz, obj, what=f"lattice, radius {radius!r}", radius=radius, nb_points=0)
        assert detail[0][3].tolist() == [1] * 64 and len(want[0]) == 64
        assert _check(C, xyz, obj, what="nb_points 1", radius=radius, nb_points=1)[0][3] == 0
    want, detail, _ = _check(C, xyz, obj, what="lattice, radius one step above", radius=above, nb_points=3)
    assert sorted(np.bincount(detail[0][3]).tolist()) == [0, 0, 0, 0, 8, 8, 24, 24] and len(want[0]) == 64      # corners have 4: kept at 3
    want, _, _ = _check(C, xyz, obj, what="nb_points 4", radius=above, nb_points=4)
    assert len(want[0]) == 56                                             # the eight corners have exactly 4: removed


@pytest.mark.parametrize("nb_points", [0, 3, 40])
def test_exactly_nb_points_is_removed_and_one_more_is_kept(C, nb_points):
    """objects on a 0.01 lattice (voxel 0.01: one point per voxel), all points of an object within the radius of each other: object 0 has
    nb_points points, object 1 one more"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 0.01
    xyz = np.concatenate([g[:nb_points], g[:nb_points + 1] + [0.5, 0, 0]]).astype(F32)
    obj = np.array([0] * nb_points + [1] * (nb_points + 1))
    want, detail, _ = _check(C, xyz, obj, 2, what=f"nb_points {nb_points}", voxel=0.01, nb_points=nb_points)
    assert detail[1][3].tolist() == [nb_points + 1] * (nb_points + 1) and (nb_points == 0 or detail[0][3].tolist() == [nb_points] * nb_points)
    assert want[2].tolist() == [1] and len(want[0]) == nb_points + 1


# ---- vanishing objects ----
def test_objects_that_vanish(C):
    from stratified_transformer_amd import _lib
    a, _ = _blobs(400, 1, 1, sigma=0.04)
    stray = np.array([[5, 5, 5], [7, 5, 5], [5, 7, 5]], F32)
    xyz = np.concatenate([a, stray, a + F32(3)])
    obj = np.array([0] * 400 + [1] * 3 + [2] * 400)
    want, detail, _ = _check(C, xyz, obj, what="the middle one vanishes")
    assert want[2].tolist() == [0, 2] and detail[1][3].tolist() == [1, 1, 1] and set(want[1].tolist()) == {0, 1}
    # all of them: nothing is launched behind the count
    far = np.concatenate([stray, stray + F32(20), stray - F32(20)])
    calls = _lib.CALLS[0]
    want, _, counters = _check(C, far, np.repeat([0, 1, 2], 3), what="all vanish")
    assert want[3] == 0 and counters == {"launches": LAUNCHES, "readbacks": 3} and _lib.CALLS[0] == calls + LAUNCHES
    # no points, and no point in an object: nothing is launched at all
    calls = _lib.CALLS[0]
    got = C.clean_supports(torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), 3)
    assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[2].shape == (0,) and got[3] == 0 and C.LAST_SUPPORTS == {"launches": 0, "readbacks": 0}
    got = C.clean_supports(dev(a), dev(np.full(400, -1)), 3)
    assert got[0].shape == (0, 3) and got[3] == 0 and C.LAST_SUPPORTS == {"launches": 0, "readbacks": 1}
    assert C.clean_supports(dev(a), dev(np.full(400, -1)))[3] == 0 and _lib.CALLS[0] == calls


# ---- grid extremes ----
def test_a_single_grid_cell_more_than_1024_cells_and_keys_beyond_32_bits(C):
    xyz = np.random.default_rng(4).uniform(0, 0.05, (600, 3)).astype(F32)
    assert np.all(np.floor(np.ptp(xyz, 0) / (0.1 * C.CELL_MARGIN)) == 0)
    want, detail, _ = _check(C, xyz, np.arange(600) % 2, what="one cell", voxel=0.01)
    assert len(want[0]) == sum(len(d[1]) for d in detail.values()) > 100  # everybody reaches everybody
    xyz, obj = _blobs(3000, 3, 12, extent=4.0)
    assert np.prod(np.floor(np.ptp(xyz, 0) / (0.1 * C.CELL_MARGIN)) + 1) > 1024
    _check(C, xyz, obj, what="many cells")
    rng = np.random.default_rng(8)
    centres = rng.uniform(0, [20, 20, 4], (300, 3))
    which = np.arange(4500) % 300
    xyz = (centres[which] + rng.normal(0, 0.04, (4500, 3))).astype(F32)
    assert 300 * np.prod(np.floor(np.ptp(xyz, 0).astype(np.float64) / 0.04) + 2) > 2 ** 32
    want, _, _ = _check(C, xyz, which, what="300 objects on a wide scene")
    assert 100 < want[3] <= 300


# ---- input forms ----
def test_label_dtypes_a_strided_coord_and_two_identical_runs(C):
    xyz, obj = _blobs(4000, 6, 5)
    obj[::7] = -1
    want = O.clean_supports(xyz, obj, 5)
    wide = dev(np.concatenate([xyz, xyz[::-1]], 1))
    assert not wide[:, :3].is_contiguous()
    for label in (dev(obj.astype(np.int32)), dev(obj.astype(np.int64))):
        _same(C.clean_supports(wide[:, :3], label, 5), want, f"{label.dtype}")
    a, b = C.clean_supports(dev(xyz), dev(obj), 5), C.clean_supports(dev(xyz), dev(obj), 5)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("n_objects", [2, 40, 70])
def test_three_read_backs_whatever_the_number_of_objects(C, n_objects):
    xyz, obj = _blobs(4000, 40, n_objects, extent=3.0)
    _, _, calls = _check(C, xyz, obj, n_objects, what=f"{n_objects} objects")
    assert calls == {"launches": LAUNCHES, "readbacks": 3}


# ---- rejections ----
def test_rejections_on_the_device(C):
    from stratified_transformer_amd import _lib
    xyz, label = torch.zeros(10, 3, device="cuda"), torch.zeros(10, dtype=torch.int64, device="cuda")
    calls = _lib.CALLS[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.clean_supports(xyz.cpu(), label)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.box_supports(xyz.cpu(), xyz, label)
    with pytest.raises(TypeError, match="float32"):
        C.clean_supports(xyz.double(), label)
    with pytest.raises(ValueError, match="label values"):
        C.clean_supports(xyz, label + 3, 3)                                # a label beyond the count
    with pytest.raises(ValueError, match="label values"):
        C.clean_supports(xyz, label - 2)                                   # below -1
    bad = xyz.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        C.clean_supports(bad, label)
    wide = xyz.clone()
    wide[0, 0] = 1e6
    with pytest.raises(ValueError, match="voxel keys"):
        C.clean_supports(wide, label)                                      # 2.5e7 voxels along x
    wide[0] = 2e4
    with pytest.raises(ValueError, match="voxel keys"):
        C.clean_supports(wide, label, 300)                                 # 300 * (5e5)^3 >= 2^61
    for kw in ({"voxel": 0.0}, {"voxel": float("inf")}, {"radius": -1.0}, {"radius": float("nan")}, {"nb_points": -1}, {"nb_points": 1.5}):
        with pytest.raises(ValueError, match="clean_supports"):
            C.clean_supports(xyz, label, **kw)
        with pytest.raises(ValueError, match="clean_supports"):
            C.box_supports(xyz, xyz, label, **kw)
    assert _lib.CALLS[0] == calls                                          # all of them before any launch


# ---- the chain ----
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "objects_reference.npz"), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def _oracle_chain(s):
    """a golden scene through instances -> objects -> clean_supports -> merge on the four oracles, computed once"""
    from tests import contacts_oracle, dbscan_oracle, merge_oracle
    gold = np.load(os.path.join(ROOT, "tests", "golden", "objects_reference.npz"), allow_pickle=False)
    coord, pred = gold[f"coord_{s}"], gold[f"pred_{s}"]
    instance, cls, size = dbscan_oracle.instances(coord, np.zeros_like(coord), pred, gold["eps"], gold["min_samples"], gold["min_points"])
    obj, _, n_objects = contacts_oracle.scene_objects(coord, instance, cls, size)
    supports = O.clean_supports(coord, obj, n_objects)
    return dict(instance=instance, obj=obj, supports=supports, merge=merge_oracle.merge_literal(*supports[:2], supports[3]))


def _same_merge(got, want, obj):
    from tests import merge_oracle
    merged, set_of, boxes, n_sets = got
    want_of, want_sets, want_boxes = want
    assert n_sets == len(want_sets) and np.array_equal(set_of.cpu().numpy(), want_of) and np.array_equal(boxes.cpu().numpy(), want_boxes)
    assert np.array_equal(merged.cpu().numpy(), merge_oracle.merged_points(obj, want_of))


@pytest.mark.parametrize("s", ["a", "b"])
def test_golden_scenes_through_the_chain_equal_the_oracles(C, gold, s):
    want = _oracle_chain(s)
    coord, pred = dev(gold[f"coord_{s}"]), dev(gold[f"pred_{s}"])
    instance, cls, size = C.instances(coord, torch.zeros_like(coord), pred)
    obj, _, n_objects = C.objects(coord, instance, cls, size)
    assert np.array_equal(instance.cpu().numpy(), want["instance"]) and np.array_equal(obj.cpu().numpy(), want["obj"])
    supports = C.clean_supports(coord, obj, n_objects)
    _same(supports, want["supports"], f"scene {s}")
    assert C.LAST_SUPPORTS == {"launches": LAUNCHES, "readbacks": 3}
    assert np.bincount(want["supports"][1]).tolist() == {"a": [528, 2277], "b": [1278, 1071, 192]}[s]
    _same_merge(C.merge_objects(supports[0], supports[1], supports[3]), want["merge"], want["supports"][1])
    # the same in one call
    together = C.box_supports(coord, torch.zeros_like(coord), pred)
    assert len(together) == 6
    _same(together[:4], want["supports"], f"scene {s}, box_supports")
    assert together[4].dtype == torch.int32 and np.array_equal(together[4].cpu().numpy(), want["instance"])
    assert together[5].dtype == torch.int32 and np.array_equal(together[5].cpu().numpy(), want["obj"])
    _same_merge(C.merge_objects(together[0], together[1], together[3]), want["merge"], want["supports"][1])
    print(f"scene {s}: {int((want['obj'] >= 0).sum())} support points -> {len(want['supports'][0])} means, sets {want['merge'][1]}")


def test_a_box_scene_with_strays_loses_them_and_its_boxes_shrink(C):
    """boxes of points on two opposite faces, and per box three stray points 0.3 to 0.6 outside it under the same object number: the
    clean-up removes them, and the box that merge_objects takes from the cleaned support is smaller than the raw points' box"""
    from tests import merge_oracle
    rng = np.random.default_rng(17)
    xyz, label = [], []
    for b in range(6):
        corner, edge = np.array([1.5 * (b % 3), 1.5 * (b // 3), 0.0]), rng.uniform(0.3, 0.6, 3)
        pts = corner + rng.uniform(0, 1, (700, 3)) * edge
        pts[:, 2] = corner[2] + np.where(rng.random(700) < 0.5, 0.0, edge[2])
        stray = corner + edge + rng.uniform(0.3, 0.6, (3, 3))                # three: their counts cannot exceed 3
        xyz += [pts, stray]
        label += [b] * 703
    xyz, label = np.concatenate(xyz).astype(F32), np.array(label)
    perm = rng.permutation(len(label))
    xyz, label = xyz[perm], label[perm]
    want, detail, _ = _check(C, xyz, label, 6, what="strays")
    removed = sum(int((d[3] <= 3).sum()) for d in detail.values())
    assert removed >= 6 * 3 and want[3] == 6
    raw_lo, raw_hi, _ = merge_oracle.boxes(xyz, label, 6)
    lo, hi, _ = merge_oracle.boxes(want[0], want[1], 6)
    assert (hi < raw_hi - 0.25).all() and (lo >= raw_lo).all()           # every box lost its strays
    points, obj, source, n = C.clean_supports(dev(xyz), dev(label), 6)
    got = C.merge_objects(points, obj, n)
    _same_merge(got, merge_oracle.merge_literal(want[0], want[1], 6), want[1])
    raw = C.merge_objects(dev(xyz), dev(label), 6)
    assert got[3] == raw[3] == 6 and (got[2][:, 3:] < raw[2][:, 3:] - 0.25).all()
