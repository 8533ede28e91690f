"""GPU (-m gpu): stratified_transformer_amd.cluster.label_boxes / merge_objects on csrc/boxes.hip against the brute-force oracle of
tests/merge_oracle.py evaluated on the CPU.  No tolerance anywhere: integer sizes, minima and maxima of fp32 values, and rows whose every
bit is defined by one fp32 comparison.  The golden scenes pin merge_objects to the sets and boxes that the reference's own functions
recorded inside its merge loop (tests/golden/merge_reference.npz)."""
import os

import numpy as np
import pytest
import torch

from tests import merge_oracle as O
from tests.util import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def C():
    from stratified_transformer_amd import cluster
    return cluster


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "merge_reference.npz"), allow_pickle=False))


# ---- label_boxes ----
def _check_boxes(C, xyz, label, n_labels=None, what=""):
    lo, hi, size = C.label_boxes(dev(np.asarray(xyz, np.float32)), dev(np.asarray(label)), n_labels)
    torch.cuda.synchronize()
    assert lo.dtype == torch.float32 and hi.dtype == torch.float32 and size.dtype == torch.int32
    got = lo.cpu().numpy(), hi.cpu().numpy(), size.cpu().numpy()
    want = O.boxes(xyz, label, n_labels)
    print(f"{what}: n {len(xyz)}, labels {len(want[2])}, empty {int((want[2] == 0).sum())}, launches {C.LAST_MERGE['launches']}")
    for g, w, name in zip(got, want, ("lo", "hi", "size")):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs at {np.argwhere(g != w)[:10].tolist()}"   # by value
    return want


def _cloud(n, seed):
    """coordinates of both signs around zero, a few exact zeros of both signs among them"""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0, 1.5, (n, 3)).astype(np.float32)
    xyz[rng.random((n, 3)) < 0.05] = 0.0
    xyz[rng.random((n, 3)) < 0.05] = -0.0
    return xyz, rng


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_boxes_wave_block_and_tile_edges(C, n):
    xyz, rng = _cloud(n, n)
    lo, hi, size = _check_boxes(C, xyz, rng.integers(0, 3, n), 3, what=f"n {n}")
    assert size.sum() == n


@pytest.mark.parametrize("n_labels", [1, 64, 65, 1023, 1024, 1025, 5000])
def test_boxes_on_both_sides_of_the_lds_table_and_on_the_global_path(C, n_labels):
    xyz, rng = _cloud(6000, n_labels)
    label = rng.integers(0, n_labels, 6000)
    label[:min(n_labels, 6000)] = np.arange(min(n_labels, 6000))         # the last label is there
    label[-1] = n_labels - 1
    lo, hi, size = _check_boxes(C, xyz, label, what=f"labels {n_labels}")
    assert len(size) == n_labels and size[-1] >= 1 and (lo[size > 0] <= hi[size > 0]).all()


def test_boxes_negative_coordinates_and_zeros_of_both_signs(C):
    xyz = np.array([[-1.5, -0.0, 2.0], [-3.25, 0.0, -2.0], [-2.0, -0.0, -0.0], [-1e-30, 1e-30, -7.0],        # label 0: a tiny negative maximum
                    [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0],                                                      # label 1: both zeros, one value
                    [-5.0, -6.0, -7.0], [-5.5, -5.5, -7.5]], np.float32)                                      # label 2: all negative
    label = np.array([0, 0, 0, 0, 1, 1, 2, 2])
    lo, hi, _ = _check_boxes(C, xyz, label, what="signs")
    assert lo[0].tolist() == [-3.25, 0.0, -7.0] and hi[0].tolist() == [np.float32(-1e-30), np.float32(1e-30), 2.0]
    assert not lo[1].any() and not hi[1].any()
    assert lo[2].tolist() == [-5.5, -6.0, -7.5] and hi[2].tolist() == [-5.0, -5.5, -7.0]


def test_boxes_of_identical_points_unlabelled_points_and_labels_without_a_point(C):
    lo, hi, size = _check_boxes(C, np.full((300, 3), -1.37, np.float32), np.array([0] * 120 + [2] * 180), 4, what="duplicates")
    assert size.tolist() == [120, 0, 180, 0] and (lo[[0, 2]] == np.float32(-1.37)).all() and (hi[[0, 2]] == np.float32(-1.37)).all()
    assert np.isposinf(lo[[1, 3]]).all() and np.isneginf(hi[[1, 3]]).all()
    xyz, rng = _cloud(3000, 5)
    label = rng.integers(-1, 70, 3000)
    label[label == 33] = -1
    for n_labels in (70, 2000):                                           # the table in LDS and the global path
        lo, hi, size = _check_boxes(C, xyz, label, n_labels, what=f"40 unlabelled, {n_labels}")
        assert size[33] == 0 and size.sum() == (label >= 0).sum()
    lo, hi, size = _check_boxes(C, xyz, np.full(3000, -1), 5, what="nobody")
    assert not size.any() and np.isposinf(lo).all()


def test_boxes_twice_gives_identical_tensors(C):
    xyz, rng = _cloud(20000, 9)
    label = dev(rng.integers(-1, 1500, 20000))
    a, b = C.label_boxes(dev(xyz), label, 1500), C.label_boxes(dev(xyz), label, 1500)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- reach rows, through the pattern table that merge_objects reads back ----
def _device_patterns(C, xyz, label, radius, n_labels):
    """the device's rows as merge_objects builds them -> (rows uint32 [N, words] in the order of the input points, its pattern table)"""
    x, lab = dev(np.asarray(xyz, np.float32)), dev(np.asarray(label)).to(torch.int32)
    member = lab >= 0
    n_valid = int(member.sum().item())
    r = np.float32(radius)
    cell = float(r) * C.CELL_MARGIN
    origin = xyz[label >= 0].min(0).astype(np.float64)
    dims = [int(np.floor((float(xyz[label >= 0][:, a].max()) - origin[a]) / cell)) + 1 for a in range(3)]
    slabel, rows = C._reach_rows(x, lab, member, len(xyz), n_valid, n_labels, origin, cell, dims, np.float32(r * r), x.device)
    pat, count = C._patterns(slabel, rows)
    torch.cuda.synchronize()
    return slabel.cpu().numpy(), rows.cpu().numpy().view(np.uint32), pat.cpu().numpy(), count.cpu().numpy(), dims


def _check_rows(C, xyz, label, radius, n_labels=None, what=""):
    label = np.asarray(label)
    n_labels = int(label.max()) + 1 if n_labels is None else n_labels
    slabel, rows, pat, count, dims = _device_patterns(C, xyz, label, radius, n_labels)
    want_rows = O.reach_rows(xyz, label, radius, n_labels)
    want = O.patterns(label, want_rows)
    print(f"{what}: n {len(xyz)}, labels {n_labels}, cells {dims}, border points {int(want_rows.any(1).sum())}, patterns {len(want[0])}")
    # the rows themselves, as multisets per label (the device keeps the grid's order): sorted rows of (label, words)
    valid = label >= 0
    mine = np.concatenate([slabel[:, None].astype(np.int64), rows.astype(np.int64)], 1)
    theirs = np.concatenate([label[valid, None].astype(np.int64), want_rows[valid].astype(np.int64)], 1)
    assert mine.shape == theirs.shape
    assert np.array_equal(mine[np.lexsort(mine.T[::-1])], theirs[np.lexsort(theirs.T[::-1])]), f"{what}: rows differ"
    # the pattern table: the same (object, row) -> count map
    got = {(int(p[0]),) + tuple(int(w) & 0xffffffff for w in p[1:]): int(c) for p, c in zip(pat, count)}
    ref = {(int(o),) + tuple(int(w) for w in r): int(c) for o, r, c in zip(*want)}
    assert got == ref, f"{what}: patterns differ"
    return want_rows, want


def _blobs(n, seed, n_blobs=6, sigma=0.06, extent=2.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.3, extent - 0.3, (n_blobs, 3))
    which = rng.integers(0, n_blobs, n)
    return (centres[which] + rng.normal(0, sigma, (n, 3))).astype(np.float32), which


@pytest.mark.parametrize("n_labels", [1, 31, 32, 33, 64, 65, 300])
def test_rows_at_word_edges_and_the_register_boundary(C, n_labels):
    xyz, _ = _blobs(2000, 7, n_blobs=5, sigma=0.08, extent=1.2)
    label = np.random.default_rng(n_labels).integers(0, n_labels, 2000)
    label[:n_labels] = np.arange(n_labels)                                # every label is there, the last one included
    rows, _ = _check_rows(C, xyz, label, 0.1, what=f"labels {n_labels}")
    own = (rows[np.arange(2000), label >> 5] >> (label & 31).astype(np.uint32)) & 1
    assert not own.any() and (rows.any() or n_labels == 1)                # the own bit is cleared; one label: no border at all
    if n_labels > 1:
        last = (rows[:, (n_labels - 1) >> 5] >> np.uint32((n_labels - 1) & 31)) & 1
        assert last.any()                                                 # somebody reaches the last label: its bit, the last of the last word


def test_rows_on_a_lattice_at_spacing_exactly_the_radius(C):
    """spacing 0.25 = radius: d2 == r2 exactly in fp32, so under the strict comparison nobody reaches a neighbour; a radius one fp32 step
    up and everybody does"""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    order = np.random.default_rng(1).permutation(len(g))
    xyz, label = (g * 0.25).astype(np.float32)[order], (g.sum(1) % 2)[order]        # a 3-d checkerboard: every neighbour has the other label
    rows, want = _check_rows(C, xyz, label, 0.25, what="lattice, radius 0.25")
    assert not rows.any() and len(want[0]) == 0
    rows, want = _check_rows(C, xyz, label, 0.2500001, what="lattice, radius 0.2500001")
    assert np.float32(0.2500001) > np.float32(0.25) and (rows[:, 0] == np.where(label == 0, 2, 1)).all() and sorted(want[2].tolist()) == [60, 60]


def test_rows_with_unlabelled_points(C):
    xyz, which = _blobs(1200, 11, n_blobs=4, sigma=0.08, extent=1.0)
    label = which.copy()
    label[np.random.default_rng(0).random(1200) < 0.4] = -1
    rows, want = _check_rows(C, xyz, label, 0.1, 4, what="40 % unlabelled")
    keep = label >= 0
    _, again = _check_rows(C, xyz[keep], label[keep], 0.1, 4, what="without them")
    assert all(np.array_equal(a, b) for a, b in zip(want, again)) and rows.any()


def test_rows_in_a_single_cell_and_in_more_than_1024_cells(C):
    xyz, label = _blobs(2000, 3, n_blobs=12, sigma=0.05, extent=4.0)
    assert np.prod(np.floor(np.ptp(xyz, 0) / (0.1 * C.CELL_MARGIN)) + 1) > 1024
    _check_rows(C, xyz, label, 0.1, what="many cells")
    xyz = np.random.default_rng(4).uniform(0, 0.05, (500, 3)).astype(np.float32)
    assert np.all(np.floor(np.ptp(xyz, 0) / (0.1 * C.CELL_MARGIN)) == 0)
    rows, want = _check_rows(C, xyz, np.arange(500) % 4, 0.1, what="one cell")
    assert want[2].tolist() == [125] * 4                                  # everybody reaches the three other labels


# ---- merge_objects ----
def _merge(C, coord, obj, n_objects=None, **kw):
    merged, set_of, boxes, n_sets = C.merge_objects(dev(np.asarray(coord, np.float32)), dev(np.asarray(obj)), n_objects, **kw)
    torch.cuda.synchronize()
    assert merged.dtype == torch.int32 and set_of.dtype == torch.int32 and boxes.dtype == torch.float32 and isinstance(n_sets, int)
    assert boxes.shape == (n_sets, 6) and merged.shape == (len(coord),)
    return merged.cpu().numpy(), set_of.cpu().numpy(), boxes.cpu().numpy(), n_sets


@pytest.mark.parametrize("s", ["a", "b"])
def test_golden_scenes_equal_the_reference(C, gold, s):
    coord, obj, n = gold[f"coord_{s}"], gold[f"object_{s}"], int(gold[f"n_objects_{s}"])
    merged, set_of, boxes, n_sets = _merge(C, coord, obj, n)
    print(f"scene {s}: {len(coord)} points, {n} objects, {n_sets} sets {set_of.tolist()}, launches {C.LAST_MERGE['launches']}, "
          f"read-backs {C.LAST_MERGE['readbacks']}")
    assert np.array_equal(set_of, gold[f"set_of_object_{s}"]) and n_sets == len(gold[f"boxes_{s}"])
    assert np.array_equal(boxes.astype(np.float64), gold[f"boxes_{s}"])                                # by value
    assert np.array_equal(merged, O.merged_points(obj, gold[f"set_of_object_{s}"]))
    assert C.LAST_MERGE["readbacks"] == 2
    got = C.box_detection(torch.from_numpy(boxes), gold[f"gt_boxes_{s}"], float(gold["iou_threshold"]))
    assert got[0] == gold[f"tp_{s}"].tolist() and got[1] == gold[f"fp_{s}"].tolist() and got[2] == int(gold[f"fn_{s}"])
    assert got[3] == float(gold[f"precision_{s}"]) and got[4] == float(gold[f"recall_{s}"])


def _box_scene(seed, n_boxes, target):
    """boxes of random size in a 2.3 x 2.3 x 1.1 room, their points uniform in the volume but on two opposite faces along one axis;
    `target` points in all, a tenth unlabelled"""
    rng = np.random.default_rng(seed)
    xyz, label = [], []
    for b in range(n_boxes):
        corner, edge = rng.uniform(0, [1.6, 1.6, 0.4]), rng.uniform(0.25, 0.7, 3)
        pts = corner + rng.uniform(0, 1, (target // n_boxes, 3)) * edge
        axis = int(rng.integers(0, 3))
        pts[:, axis] = corner[axis] + np.where(rng.random(len(pts)) < 0.5, 0.0, edge[axis])
        xyz.append(pts)
        label += [b] * len(pts)
    xyz, label = np.concatenate(xyz).astype(np.float32), np.array(label)
    perm = rng.permutation(len(label))
    xyz, label = xyz[perm], label[perm]
    label[rng.random(len(label)) < 0.1] = -1
    return xyz, label


@pytest.mark.parametrize("seed,n_boxes,target", [(41, 9, 5000), (42, 14, 10000)])
def test_seeded_box_scenes_equal_the_oracle(C, seed, n_boxes, target):
    xyz, label = _box_scene(seed, n_boxes, target)
    log = []
    want_of, want_sets, want_boxes = O.merge_literal(xyz, label, n_boxes, log=log)
    merged, set_of, boxes, n_sets = _merge(C, xyz, label, n_boxes)
    n_merged = sum((a or b) and n > 10 for _, _, a, b, n in log)
    print(f"seed {seed}: {len(xyz)} points, {n_boxes} boxes -> {n_sets} sets {want_sets}, {len(log)} pairs evaluated, {n_merged} merges")
    assert n_sets == len(want_sets) and np.array_equal(set_of, want_of) and np.array_equal(boxes, want_boxes)
    assert np.array_equal(merged, O.merged_points(label, want_of))
    assert 1 < n_sets < n_boxes and n_merged >= 2                          # something merged, something did not


def test_the_chain_instances_objects_merge_objects(C):
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "objects_reference.npz"), allow_pickle=False))
    coord, pred = dev(gold["coord_a"]), dev(gold["pred_a"])
    instance, cls, size = C.instances(coord, torch.zeros_like(coord), pred)
    obj, _, n_objects = C.objects(coord, instance, cls, size)
    assert n_objects == int(gold["n_objects_a"]) and np.array_equal(obj.cpu().numpy(), gold["object_a"])
    merged, set_of, boxes, n_sets = C.merge_objects(coord, obj, n_objects)
    want_of, want_sets, want_boxes = O.merge_literal(gold["coord_a"], obj.cpu().numpy(), n_objects)
    print(f"chain: {n_objects} objects -> {n_sets} sets {want_sets}")
    assert n_sets == len(want_sets) and np.array_equal(set_of.cpu().numpy(), want_of) and np.array_equal(boxes.cpu().numpy(), want_boxes)
    assert np.array_equal(merged.cpu().numpy(), O.merged_points(obj.cpu().numpy(), want_of))


@pytest.mark.parametrize("n_objects", [2, 40])
def test_two_read_backs_whatever_the_number_of_objects(C, n_objects):
    xyz, which = _blobs(4000, 40, n_blobs=n_objects, sigma=0.1, extent=3.0)
    merged, set_of, boxes, n_sets = _merge(C, xyz, which, n_objects)
    assert C.LAST_MERGE["readbacks"] == 2 and C.LAST_MERGE["launches"] == 4     # boxes, keys, prepare, rows
    want_of, want_sets, want_boxes = O.merge_literal(xyz, which, n_objects)
    assert np.array_equal(set_of, want_of) and np.array_equal(boxes, want_boxes)


def test_more_than_64_objects_and_int32_labels(C):
    xyz, which = _blobs(3000, 77, n_blobs=70, sigma=0.08, extent=3.0)
    want_of, want_sets, want_boxes = O.merge_literal(xyz, which, 70)
    for dtype in (np.int32, np.int64):
        merged, set_of, boxes, n_sets = _merge(C, xyz, which.astype(dtype), 70)
        assert np.array_equal(set_of, want_of) and np.array_equal(boxes, want_boxes) and 1 < n_sets < 70


def test_no_points_and_no_labelled_point_launch_nothing(C):
    from stratified_transformer_amd import _lib
    calls = _lib.CALLS[0]
    merged, set_of, boxes, n_sets = _merge(C, np.zeros((0, 3), np.float32), np.zeros(0, np.int64), 3)
    assert n_sets == 0 and set_of.tolist() == [-1, -1, -1] and C.LAST_MERGE == {"launches": 0, "readbacks": 0}
    xyz, _ = _blobs(500, 1)
    merged, set_of, boxes, n_sets = _merge(C, xyz, np.full(500, -1), 3)
    assert n_sets == 0 and (merged == -1).all() and set_of.tolist() == [-1, -1, -1] and C.LAST_MERGE == {"launches": 0, "readbacks": 1}
    merged, set_of, boxes, n_sets = _merge(C, xyz, np.full(500, -1))
    assert n_sets == 0 and set_of.shape == (0,)
    lo, hi, size = C.label_boxes(dev(xyz), dev(np.full(500, -1)))
    assert lo.shape == (0, 3) and size.shape == (0,)
    assert _lib.CALLS[0] == calls


def test_rejections_on_the_device(C):
    from stratified_transformer_amd import _lib
    xyz, label = torch.zeros(10, 3, device="cuda"), torch.zeros(10, dtype=torch.int64, device="cuda")
    calls = _lib.CALLS[0]
    for fn in (C.label_boxes, C.merge_objects):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(xyz.cpu(), label)
        with pytest.raises(ValueError, match="label values"):
            fn(xyz, label + 3, 3)                                          # a label beyond the count
        with pytest.raises(ValueError, match="label values"):
            fn(xyz, label - 2)                                             # below -1
        bad = xyz.clone()
        bad[3, 1] = float("nan")
        with pytest.raises(ValueError, match="finite"):
            fn(bad, label)
    wide = xyz.clone()
    wide[0, 0] = 1e6
    with pytest.raises(ValueError, match="cells"):
        C.merge_objects(wide, label)
    big = torch.zeros(300000, 3, device="cuda")
    with pytest.raises(ValueError, match="bitmap"):
        C.merge_objects(big, torch.zeros(300000, dtype=torch.int32, device="cuda"), 32768)   # 300000 * 1024 * 4 bytes > 1 GiB
    assert _lib.CALLS[0] == calls                                          # all of them before any launch
