"""CPU: the oracle of cluster.merge_objects / box_detection (tests/merge_oracle.py) against the reference's recorded merging and detection
score (tests/golden/merge_reference.npz, written by the reference's own compute_partial_iou and DetectionMAP inside its merge loop), the
pattern formulation of stratified_transformer_amd.cluster.merge_sets against the literal per-pair loop on point arrays, box_detection on
hand-made boxes, and the argument checks that need no GPU.  No HIP compute runs here."""
import functools
import inspect
import os

import numpy as np
import pytest
import torch

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, cluster
from tests import merge_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = torch.int64


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "merge_reference.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def gold_tables(gold):
    """per golden scene, computed once: the oracle's boxes, rows and patterns, and its literal loop with the log of evaluated pairs"""
    out = {}
    for s in "ab":
        coord, obj, n = gold[f"coord_{s}"], gold[f"object_{s}"], int(gold[f"n_objects_{s}"])
        log = []
        literal = O.merge_literal(coord, obj, n, log=log)
        rows = O.reach_rows(coord, obj, 0.2, n)
        out[s] = dict(boxes=O.boxes(coord, obj, n), rows=rows, patterns=O.patterns(obj, rows), literal=literal, log=log)
    return out


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _sets_from_tables(xyz, label, n_labels=None, **kw):
    """cluster.merge_sets fed with the oracle's boxes and patterns"""
    rows = O.reach_rows(xyz, label, kw.pop("radius", 0.2), n_labels)
    lo, hi, size = O.boxes(xyz, label, n_labels)
    return cluster.merge_sets(lo, hi, size, *O.patterns(label, rows), **kw)


def test_fixture_holds_the_scenes_the_issue_asks_for(gold):
    assert float(gold["radius"]) == cluster.MERGE_RADIUS == 0.2 and float(gold["overlap"]) == cluster.MERGE_OVERLAP == 0.3
    assert int(gold["min_neighbors"]) == cluster.MERGE_MIN_NEIGHBORS == 10 and float(gold["iou_threshold"]) == 0.5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "merge_reference.npz")) < 1 << 20
    for s in "ab":
        assert gold[f"coord_{s}"].dtype == np.float32 and 5000 <= len(gold[f"coord_{s}"]) <= 12000
        assert len(gold[f"boxes_{s}"]) == gold[f"set_of_object_{s}"].max() + 1
    pairs = {(int(c), int(t)): (bool(a), bool(b), int(n)) for c, t, a, b, n in gold["pairs_a"]}     # (the last evaluation of a pair of firsts)
    assert pairs[(0, 1)][:2] == (False, True) and pairs[(0, 1)][2] > 10                              # (a) a merge decided by one side, and a seam
    assert gold["set_of_object_a"][0] == gold["set_of_object_a"][1]
    assert any(c == 3 and t == 0 and not a and not b and n > 100 for c, t, a, b, n in gold["pairs_a"])          # (b) a seam, no box overlap
    assert gold["set_of_object_a"][3] == gold["set_of_object_a"][4] != gold["set_of_object_a"][0]    # (d) two merged sets, which met: [0, ..] vs [3, ..]
    assert any(c == 0 and t == 3 and n > 10 for c, t, a, b, n in gold["pairs_a"])
    flat = gold["coord_a"][gold["object_a"] == 6]
    assert len(flat) > 100 and np.ptp(flat[:, 2]) == 0                                                # (e) the flat object, near others, never overlapping
    assert all(not a and not b for c, t, a, b, n in gold["pairs_a"] if 6 in (c, t)) and any(n > 10 for c, t, a, b, n in gold["pairs_a"] if 6 in (c, t))
    assert not (gold["object_a"] == 5).any() and gold["set_of_object_a"][5] == -1                    # (f) an object number without a point
    few = [(a or b, n) for c, t, a, b, n in gold["pairs_b"] if {int(c), int(t)} == {0, 1}]             # (c) box overlap, 10 or fewer near points
    assert len(few) >= 2 and all(over and 0 < n <= 10 for over, n in few) and gold["set_of_object_b"][0] != gold["set_of_object_b"][1]


@pytest.mark.parametrize("s", ["a", "b"])
def test_oracle_merging_equals_the_references(gold, gold_tables, s):
    set_of, final, boxes = gold_tables[s]["literal"]
    assert np.array_equal(set_of, gold[f"set_of_object_{s}"])                                         # the sets and their order in the final list
    assert boxes.dtype == np.float32 and np.array_equal(boxes.astype(np.float64), gold[f"boxes_{s}"])  # by value
    pairs = [[c[0], t[0], a, b, n] for c, t, a, b, n in gold_tables[s]["log"]]
    assert np.array_equal(np.array(pairs, np.int32), gold[f"pairs_{s}"])                              # decision for decision
    # the host loop of the package on the oracle's boxes and patterns: the same list
    lo, hi, size = gold_tables[s]["boxes"]
    got_of, got_sets = cluster.merge_sets(lo, hi, size, *gold_tables[s]["patterns"])
    assert got_of.dtype == np.int32 and np.array_equal(got_of, set_of) and got_sets == final
    border = gold_tables[s]["rows"].any(1)
    print(f"scene {s}: {len(border)} points, {int(border.sum())} border points, {len(gold_tables[s]['patterns'][0])} patterns, final list {final}")


@pytest.mark.parametrize("s", ["a", "b"])
def test_oracle_detection_equals_the_references(gold, s):
    for fn in (O.detection, cluster.box_detection):
        tp, fp, n_fn, precision, recall = fn(gold[f"boxes_{s}"], gold[f"gt_boxes_{s}"], float(gold["iou_threshold"]))
        assert tp == gold[f"tp_{s}"].tolist() and fp == gold[f"fp_{s}"].tolist() and n_fn == int(gold[f"fn_{s}"])
        assert precision == float(gold[f"precision_{s}"]) and recall == float(gold[f"recall_{s}"])
    assert len(gold[f"tp_{s}"]) and len(gold[f"fp_{s}"]) and int(gold[f"fn_{s}"])


def test_the_order_of_the_objects_decides(gold, gold_tables):
    """scene a with E (object 4) first in the list: E takes B before A does, and the partition is another"""
    coord, obj = gold["coord_a"], gold["object_a"]
    first = np.array([1, 2, 3, 4, 0, 5, 6])                                                           # new number of every object
    renamed = np.where(obj >= 0, first[obj], -1)
    want_of, want_sets, _ = O.merge_literal(coord, renamed, 7)
    got_of, got_sets = _sets_from_tables(coord, renamed, 7)
    assert np.array_equal(got_of, want_of) and got_sets == want_sets
    back = np.argsort(first)
    partition = {frozenset(int(back[o]) for o in s) for s in got_sets}
    original = {frozenset(s) for s in gold_tables["a"]["literal"][1]}
    assert partition != original and frozenset([0, 1]) in original and any({1, 4} <= s for s in partition)


@functools.lru_cache(maxsize=None)
def _random_scene(seed):
    """3 to 8 small boxes of 40 to 120 points each (a quarter of them of 4 to 12), close enough to overlap and to touch; an object number may stay empty"""
    rng = np.random.default_rng(1000 + seed)
    n_boxes = int(rng.integers(3, 9))
    xyz, label = [], []
    for b in range(n_boxes):
        corner, edge = rng.uniform(0, 0.9, 3), rng.uniform(0.15, 0.6, 3)
        pts = corner + rng.uniform(0, 1, (int(rng.integers(4, 13) if rng.random() < 0.25 else rng.integers(40, 121)), 3)) * edge   # a quarter: sparse
        if rng.random() < 0.15:
            pts[:, int(rng.integers(0, 3))] = corner[0]                                               # a flat one
        xyz.append(pts)
        label += [b + (b >= 2 and seed % 5 == 0)] * len(pts)                                          # every fifth scene: number 2 is empty
    xyz, label = np.concatenate(xyz).astype(np.float32), np.array(label)
    perm = rng.permutation(len(label))
    xyz, label = xyz[perm], label[perm]
    label[rng.random(len(label)) < 0.05] = -1
    log = []
    want = O.merge_literal(xyz, label, log=log)
    return xyz, label, want, log


@pytest.mark.parametrize("seed", range(60))
def test_pattern_loop_equals_the_literal_loop_on_random_scenes(seed):
    xyz, label, (want_of, want_sets, _), _ = _random_scene(seed)
    got_of, got_sets = _sets_from_tables(xyz, label)
    assert got_sets == want_sets and np.array_equal(got_of, want_of)


def test_the_random_scenes_decide_both_ways():
    logs = [e for seed in range(60) for e in _random_scene(seed)[3]]
    merged = [e for e in logs if (e[2] or e[3]) and e[4] > 10]
    assert len(merged) > 30 and any(len(e[0]) > 1 and len(e[1]) > 1 for e in logs)                    # merges, and merged sets that meet
    assert any((e[2] or e[3]) and e[4] <= 10 for e in logs) and any(not (e[2] or e[3]) and e[4] > 10 for e in logs)
    assert any(e[2] != e[3] for e in merged)                                                          # decided by one side
    sizes = [len(s) for seed in range(60) for s in _random_scene(seed)[2][1]]
    assert min(sizes) == 1 and max(sizes) >= 3


def test_a_point_that_reaches_two_members_of_the_current_set_counts_once():
    """0 and 1: two slabs that overlap and touch along their whole length, four points each beside 2 and sixteen 0.5 away; 2: six points
    between them within the radius of BOTH.  [0, 1] meets [2] with num_neighbor 6 - not 12 - and 6 is no seam"""
    rng = np.random.default_rng(3)

    def slab(x0):
        y = np.concatenate([rng.uniform(-0.02, 0.02, 4), rng.uniform(0.45, 0.55, 16)])
        return np.stack([rng.uniform(x0, x0 + 0.12, 20), y, rng.uniform(0, 0.1, 20)], 1)

    two = np.stack([rng.uniform(-0.02, 0.02, 6), rng.uniform(-0.02, 0.02, 6), rng.uniform(0.03, 0.07, 6)], 1)
    xyz = np.concatenate([slab(-0.08), slab(-0.04), two]).astype(np.float32)
    label = np.array([0] * 20 + [1] * 20 + [2] * 6)
    rows = O.reach_rows(xyz, label, 0.2)
    assert (rows[label == 2, 0] == 0b011).all()                                                      # every point of 2 reaches 0 and 1
    log = []
    want_of, want_sets, _ = O.merge_literal(xyz, label, log=log)
    assert ([0, 1], [2], False, True, 6) in log and ([2], [0, 1], True, False, 8) in log and want_sets == [[2], [0, 1]]
    got_of, got_sets = _sets_from_tables(xyz, label)
    assert got_sets == want_sets and got_of.tolist() == [1, 1, 0]
    # counted per member it would be 12 > 10, a merge
    lo, hi, size = O.boxes(xyz, label)
    pat_object, pat_rows, pat_count = O.patterns(label, rows)
    double = np.concatenate([pat_count, pat_count[(pat_object == 2)]])
    assert cluster.merge_sets(lo, hi, size, np.concatenate([pat_object, pat_object[pat_object == 2]]),
                              np.concatenate([pat_rows, pat_rows[pat_object == 2]]), double)[1] == [[0, 1, 2]]


def test_zero_objects_one_object_and_an_empty_object_number():
    none = cluster.merge_sets(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), np.zeros((0, 0), np.uint32), np.zeros(0))
    assert none[0].shape == (0,) and none[0].dtype == np.int32 and none[1] == []
    lo, hi = np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    set_of, sets = cluster.merge_sets(lo, hi, [5], [], np.zeros((0, 1), np.uint32), [])
    assert set_of.tolist() == [0] and sets == [[0]]
    # three numbers, the middle one without a point: one object left, no loop; and two left, which merge
    lo3 = np.array([[0, 0, 0], [np.inf] * 3, [0.5, 0, 0]], np.float32)
    hi3 = np.array([[1, 1, 1], [-np.inf] * 3, [1.5, 1, 1]], np.float32)
    set_of, sets = cluster.merge_sets(lo3, hi3, [9, 0, 0], [], np.zeros((0, 1), np.uint32), [])
    assert set_of.tolist() == [0, -1, -1] and sets == [[0]]
    set_of, sets = cluster.merge_sets(lo3, hi3, [30, 0, 30], [2], np.array([[0b001]], np.uint32), [11])
    assert set_of.tolist() == [0, -1, 0] and sets == [[0, 2]]
    set_of, sets = cluster.merge_sets(lo3, hi3, [30, 0, 30], [2], np.array([[0b001]], np.uint32), [10])   # 10 is not more than 10
    assert set_of.tolist() == [0, -1, 1] and sets == [[0], [2]]                                      # two rounds: the list has rotated twice
    xyz, label = np.random.default_rng(0).random((50, 3)).astype(np.float32), np.zeros(50, np.int64)
    assert O.merge_literal(xyz, label)[1] == [[0]] and O.merge_literal(xyz, label - 1, 2)[1] == []


def test_boxes_that_only_touch_do_not_overlap():
    lo = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    hi = np.array([[1, 1, 1], [2, 1, 1]], np.float32)
    assert cluster.merge_sets(lo, hi, [50, 50], [1], np.array([[1]], np.uint32), [40])[1] == [[0], [1]]
    lo[1, 0] = np.nextafter(np.float32(1), np.float32(0))                                              # one fp32 step inside: an overlap, of a ratio far below 0.3
    assert cluster.merge_sets(lo, hi, [50, 50], [1], np.array([[1]], np.uint32), [40])[1] == [[0], [1]]
    assert cluster.merge_sets(lo, hi, [50, 50], [1], np.array([[1]], np.uint32), [40], overlap=0.0)[1] == [[0, 1]]


def test_box_detection_corners():
    unit = np.array([[0, 0, 0, 1, 1, 1]], float)
    assert cluster.box_detection(np.zeros((0, 6)), np.concatenate([unit, unit + 3])) == ([], [], 2, None, 0.0)   # the reference: FN = 6
    assert cluster.box_detection([], unit) == ([], [], 1, None, 0.0)
    assert cluster.box_detection(unit, np.zeros((0, 6))) == ([], [-1.0], 0, 0.0, None)
    assert cluster.box_detection(np.zeros((0, 6)), np.zeros((0, 6))) == ([], [], 0, None, None)
    # two predictions compete for one ground-truth box: the FIRST takes it, although the second fits better
    pred = np.array([[0, 0, 0, 1, 1, 0.75], [0, 0, 0, 1, 1, 1]], float)
    for fn in (cluster.box_detection, O.detection):
        tp, fp, n_fn, precision, recall = fn(pred, unit)
        assert tp == [0.75] and fp == [-1.0] and n_fn == 0 and precision == 0.5 and recall == 1.0
        tp, fp, n_fn, _, _ = fn(pred[::-1], unit)
        assert tp == [1.0] and fp == [-1.0] and n_fn == 0
        # one prediction, two ground-truth boxes: the larger IoU, and the first among equals
        tp, fp, n_fn, _, _ = fn(unit, pred)
        assert tp == [1.0] and fp == [] and n_fn == 1
        assert fn(unit, np.concatenate([unit, unit]))[:3] == ([1.0], [], 1)
        # the clip quirk: no pair intersects on any axis, the upper bound is negative and every edge becomes it: negative IoU, no match
        far = fn(unit, unit + 3)
        assert far == ([], [-1.0], 1, 0.0, 0.0)
        # below the threshold
        assert fn(unit, unit + np.array([0.5, 0, 0, 0.5, 0, 0]))[:3] == ([], [-1.0], 1)
        assert fn(unit, unit + np.array([0.5, 0, 0, 0.5, 0, 0]), 0.3)[:3] == ([1 / 3], [], 0)
    t = torch.tensor(pred, dtype=torch.float32)
    assert cluster.box_detection(t, torch.tensor(unit))[0] == [0.75]
    with pytest.raises(ValueError, match="box_detection"):
        cluster.box_detection(np.zeros((2, 5)), unit)
    with pytest.raises(ValueError, match="overlap_threshold"):
        cluster.box_detection(unit, unit, float("nan"))


def test_the_clip_quirk_is_the_references_arithmetic():
    """all differences negative: np.clip(x, 0, negative bound) yields the bound, the product of three is negative, and so is the IoU"""
    a, b = np.array([[0, 0, 0, 1, 1, 1]], float), np.array([[3, 3, 3, 4, 4, 4]], float)
    diff = np.minimum(a[:, None, 3:], b[None, :, 3:]) - np.maximum(a[:, None, :3], b[None, :, :3])
    assert (np.clip(diff, a_min=0, a_max=np.max(diff)) == -2).all()
    # a mixed case is NOT clipped to zero volume wrongly: boxes apart along x only keep a zero edge
    c = np.array([[3, 0, 0, 4, 1, 1]], float)
    assert cluster.box_detection(a, c)[:3] == ([], [-1.0], 1) and O.detection(a, c)[:3] == ([], [-1.0], 1)


def test_public_interface():
    assert sta.label_boxes is cluster.label_boxes and sta.merge_objects is cluster.merge_objects and sta.box_detection is cluster.box_detection
    assert {"label_boxes", "merge_objects", "box_detection"} <= set(sta.__all__)
    assert str(inspect.signature(cluster.label_boxes)) == "(xyz, label, n_labels=None)"
    assert str(inspect.signature(cluster.merge_objects)) == "(coord, obj, n_objects=None, radius=0.2, overlap=0.3, min_neighbors=10)"
    assert str(inspect.signature(cluster.merge_sets)) == "(lo, hi, size, pat_object, pat_rows, pat_count, overlap=0.3, min_neighbors=10)"
    assert str(inspect.signature(cluster.box_detection)) == "(pred_box, gt_box, overlap_threshold=0.5)"
    assert "merge_objects" in cluster.objects.__doc__ and "test.py:277" in cluster.merge_sets.__doc__
    assert "trimesh" in cluster.merge_objects.__doc__ and "FN = 6" in cluster.box_detection.__doc__


def test_cpu_tensors_raise_no_cpu_fallback():
    xyz, label = torch.rand(10, 3), torch.zeros(10, dtype=L)
    for a, b in ((xyz, label), (_OnGpu(xyz), label), (xyz, _OnGpu(label))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.label_boxes(a, b)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.merge_objects(a, b)


GOOD = (torch.zeros(10, 3), torch.zeros(10, dtype=L))


@pytest.mark.parametrize("xyz,label,kw,error", [
    (torch.zeros(10, 2), GOOD[1], {}, ValueError),                                  # xyz not [N, 3]
    (torch.zeros(30), GOOD[1], {}, ValueError),
    (torch.zeros(10, 3, dtype=torch.float64), GOOD[1], {}, TypeError),
    (GOOD[0], torch.zeros(9, dtype=L), {}, ValueError),                             # label not [N]
    (GOOD[0], torch.zeros(10, 1, dtype=L), {}, ValueError),
    (GOOD[0], torch.zeros(10), {}, TypeError),                                      # label dtype
    (GOOD[0], torch.zeros(10, dtype=torch.int16), {}, TypeError),
    (GOOD[0], GOOD[1], {"n_objects": -1}, ValueError),
    (GOOD[0], GOOD[1], {"n_objects": 2.0}, TypeError),
    (GOOD[0], GOOD[1], {"n_objects": True}, TypeError),
    (GOOD[0], GOOD[1], {"n_objects": cluster.MAX_LABELS + 1}, ValueError),
    (GOOD[0], GOOD[1], {"radius": 0.0}, ValueError),
    (GOOD[0], GOOD[1], {"radius": -0.2}, ValueError),
    (GOOD[0], GOOD[1], {"radius": float("nan")}, ValueError),
    (GOOD[0], GOOD[1], {"radius": float("inf")}, ValueError),
    (GOOD[0], GOOD[1], {"radius": 1e-30}, ValueError),                              # underflows in fp32
    (GOOD[0], GOOD[1], {"radius": "0.2"}, TypeError),
    (GOOD[0], GOOD[1], {"overlap": float("nan")}, ValueError),
    (GOOD[0], GOOD[1], {"overlap": -0.1}, ValueError),
    (GOOD[0], GOOD[1], {"min_neighbors": -1}, ValueError),
    (GOOD[0], GOOD[1], {"min_neighbors": 2.5}, ValueError),
])
def test_merge_objects_rejects_bad_arguments_before_any_launch(xyz, label, kw, error):
    calls = _lib.CALLS[0]
    with pytest.raises(error, match="merge_objects|merge_sets"):
        cluster.merge_objects(_OnGpu(xyz), _OnGpu(label), **kw)
    assert _lib.CALLS[0] == calls
    if not kw:
        with pytest.raises(error, match="label_boxes"):
            cluster.label_boxes(_OnGpu(xyz), _OnGpu(label))
    elif "n_objects" in kw:
        with pytest.raises(error, match="label_boxes"):
            cluster.label_boxes(_OnGpu(GOOD[0]), _OnGpu(GOOD[1]), kw["n_objects"])
    assert _lib.CALLS[0] == calls


def test_merge_sets_rejects_bad_tables():
    lo, hi = np.zeros((2, 3)), np.ones((2, 3))
    rows = np.zeros((1, 1), np.uint32)
    with pytest.raises(ValueError, match="lo and hi"):
        cluster.merge_sets(lo[:1], hi, [1, 1], [0], rows, [1])
    with pytest.raises(ValueError, match="pat_rows"):
        cluster.merge_sets(lo, hi, [1, 1], [0], np.zeros((1, 2), np.uint32), [1])
    with pytest.raises(ValueError, match="pat_count"):
        cluster.merge_sets(lo, hi, [1, 1], [0], rows, [1, 2])
    with pytest.raises(TypeError, match="32-bit words"):
        cluster.merge_sets(lo, hi, [1, 1], [0], rows.astype(np.float32), [1])
    with pytest.raises(ValueError, match="pat_object"):
        cluster.merge_sets(lo, hi, [1, 1], [2], rows, [1])


def test_no_points_returns_the_empty_results_without_a_launch():
    calls = _lib.CALLS[0]
    empty = (_OnGpu(torch.zeros(0, 3)), _OnGpu(torch.zeros(0, dtype=L)))
    lo, hi, size = cluster.label_boxes(*empty, 3)
    assert lo.shape == (3, 3) and torch.isinf(lo).all() and (lo > 0).all() and torch.isinf(hi).all() and (hi < 0).all()
    assert size.dtype == torch.int32 and size.tolist() == [0, 0, 0] and cluster.label_boxes(*empty)[0].shape == (0, 3)
    merged, set_of, boxes, n_sets = cluster.merge_objects(*empty, 3)
    assert merged.shape == (0,) and merged.dtype == torch.int32 and set_of.tolist() == [-1, -1, -1] and boxes.shape == (0, 6) and n_sets == 0
    assert cluster.merge_objects(*empty)[1].shape == (0,)
    assert _lib.CALLS[0] == calls and cluster.LAST_MERGE == {"launches": 0, "readbacks": 0}


def test_the_checks_behind_the_first_read_back_raise_before_any_launch():
    calls = _lib.CALLS[0]
    xyz, label = torch.zeros(10, 3), torch.zeros(10, dtype=L)
    for fn in (cluster.label_boxes, cluster.merge_objects):
        with pytest.raises(ValueError, match="label values"):
            fn(_OnGpu(xyz), _OnGpu(label + 3), 3)                              # a label beyond the count
        with pytest.raises(ValueError, match="label values"):
            fn(_OnGpu(xyz), _OnGpu(label - 2))                                 # below -1
        for bad_value in (float("nan"), float("inf")):
            bad = xyz.clone()
            bad[3, 1] = bad_value
            with pytest.raises(ValueError, match="finite"):
                fn(_OnGpu(bad), _OnGpu(label))
    wide = xyz.clone()
    wide[0, 0] = 1e6
    with pytest.raises(ValueError, match="cells"):
        cluster.merge_objects(_OnGpu(wide), _OnGpu(label))                     # 5e6 cells along x
    with pytest.raises(ValueError, match="bitmap"):
        cluster.merge_objects(_OnGpu(torch.zeros(300000, 3)), _OnGpu(torch.zeros(300000, dtype=torch.int32)), 32768)   # 300000 * 1024 * 4 bytes > 1 GiB
    assert _lib.CALLS[0] == calls
