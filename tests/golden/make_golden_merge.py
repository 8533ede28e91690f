"""Writes tests/golden/merge_reference.npz: the reference's OBB merging (test.py:294-326, the same loop at test_iou.py:373-406) and its box
detection score (test_iou.py:409-466, util/evaluation.py) on two synthetic scenes of axis-aligned boxes.  Run on the CPU where the
reference checkout and scipy are at hand (nothing of the reference is copied):

    python tests/golden/make_golden_merge.py --reference PATH_OF_THE_REFERENCE_CHECKOUT

The loop is inline in the reference's test scripts and cannot be imported, so `reference_loop` restates it with its line numbers; what
CAN be imported is: `compute_partial_iou` from util.train_utils (with the `open3d` stand-in of make_golden_objects.py) and `DetectionMAP`
from util.evaluation (scikit-image is not needed by anything called here: an empty stand-in module serves its import).  The loop runs on
float64 copies of the fp32 scenes with scipy.spatial.distance.cdist, as the reference does.  trimesh is not at hand:
`trimesh.points.PointCloud(p).bounding_box` is taken as the box of the bounds, centroid = (min + max) / 2, extents = max - min.

Scenes: boxes with faces on a 0.025 grid (inset 0.05 from the box's edges, jittered by up to 0.004 inside the face's plane), every box
one object, the points shuffled.
  a: A (0) without its top face; B (1) reaches out of A: its box covers half of B and a seventh of A - a merge decided by one side - and
     lies within 0.2 of A's faces; C (2) stands apart; D (3) stands 0.03 beside B: a seam of several hundred near points, no box overlap,
     no merge; E (4) overlaps B's box (40 % of E) and D's.  B is merged into A before E meets it, and the box of A + B covers 27 % of D + E:
     the order decides - E before A in the list gives another result (tests/test_merge_cpu.py) -, and the merged set [3, 4] meets the
     merged set [0, 1] in a later round.  Object 5 has no point.  F (6) is one horizontal face inside A's and B's boxes, within 0.2 of
     B's points: zero extent along z, so it never overlaps anything.
  b: G (0) is the floor and the ceiling of a room, H (1) a small box floating in its middle, more than 0.2 from both, with four stray
     points 0.197 above the floor: H's box lies wholly inside G's, and 10 or fewer points are near in either direction - no merge;
     I (2) and J (3) overlap by half of each and merge; K (4) stands apart.
Conditions on the inputs, asserted here (not tolerances - offending points are removed before anything is recorded):
  - for every pair of sets the loop evaluates, |num_neighbor - 10| exceeds the number of target points whose nearest distance lies
    within 1e-5 of 0.2 (those points are removed first, so that number is 0 in what is recorded);
  - every overlap ratio the loop computes is at least 0.02 away from 0.3;
  - on no axis are the two coordinates that decide min_max > max_min closer than 1e-6 - except where both are the two faces of ONE box of
    zero extent (the flat object F), which are the same fp32 number;
  - every IoU of a predicted and a ground-truth box is at least 0.02 away from the threshold 0.5;
  - the reference's box rows, centroid -/+ extents / 2 in float64 (test_iou.py:422), equal the fp32 minima / maxima of the sets exactly.
Per scene s in "a", "b": coord_s [n, 3] f32, object_s [n] i32, n_objects_s, set_of_object_s [O] i32 (the position of the object's set in
the reference's final list, -1 for an object without a point), boxes_s [S, 6] f64 (pred_box), gt_boxes_s [G, 6] f64, tp_s / fp_s (the
lists of DetectionMAP.compute_TP_FP_FN), fn_s, precision_s, recall_s (what DetectionMAP.evaluate appends, :95-96), and pairs_s [E, 5] i32:
per evaluated pair (first object of the current set, first object of the target set, overlap a, overlap b, num_neighbor); and the
settings radius, overlap, min_neighbors, iou_threshold."""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_objects import open3d_stand_in  # noqa: E402

MARGIN = 1e-5
STEP, INSET, JITTER = 0.025, 0.05, 0.004
RADIUS, OVERLAP, MIN_NEIGHBORS, IOU_THRESHOLD = 0.2, 0.3, 10, 0.5


def faces(rng, lo, size, skip=()):
    """the faces of a box as points; skip: (axis, side) pairs left out"""
    lo = np.asarray(lo, float)
    hi = lo + np.asarray(size, float)
    out = []
    for axis in range(3):
        for side in (0, 1):
            if (axis, side) in skip:
                continue
            u, v = [a for a in range(3) if a != axis]
            gu = np.arange(lo[u] + INSET, hi[u] - INSET + 1e-9, STEP)
            gv = np.arange(lo[v] + INSET, hi[v] - INSET + 1e-9, STEP)
            uu, vv = np.meshgrid(gu, gv, indexing="ij")
            p = np.zeros((uu.size, 3))
            p[:, u], p[:, v] = uu.ravel(), vv.ravel()
            p[:, [u, v]] += rng.uniform(-JITTER, JITTER, (len(p), 2))
            p[:, axis] = hi[axis] if side else lo[axis]
            out.append(p)
    return np.concatenate(out)


ALL_BUT_Z1 = tuple((a, s) for a in range(3) for s in (0, 1) if (a, s) != (2, 1))
ONLY_Z = tuple((a, s) for a in (0, 1) for s in (0, 1))


def scene_a(rng):
    """-> ({object number: points}, n_objects, ground-truth boxes)"""
    parts = {0: faces(rng, (0, 0, 0), (1, 1, 0.5), skip=((2, 1),)),
             1: faces(rng, (0.6, 0.2, 0.1), (0.8, 0.6, 0.3)),
             2: faces(rng, (3, 3, 0), (0.4, 0.4, 0.4)),
             3: faces(rng, (1.43, 0.0, 0), (0.5, 0.5, 0.5)),
             4: faces(rng, (1.2, 0.3, 0.15), (0.5, 0.3, 0.2)),
             6: faces(rng, (0.55, 0.25, 0.25), (0.4, 0.4, 0.0), skip=ALL_BUT_Z1)}
    gt = np.array([[0.05, 0.05, 0.0, 1.35, 0.95, 0.5],          # A + B
                   [1.25, 0.05, 0.0, 1.93, 0.55, 0.5],          # D + E
                   [3.17, 3.05, 0.0, 3.52, 3.35, 0.4],          # C, shifted: below the threshold
                   [5.0, 5.0, 0.0, 5.5, 5.5, 0.5]])             # nothing there
    return parts, 7, gt


def scene_b(rng):
    h = faces(rng, (0.375, 0.375, 0.275), (0.25, 0.25, 0.25))
    stray = np.array([[0.5, 0.5, 0.197]]) + np.concatenate([rng.uniform(-0.004, 0.004, (4, 2)), np.zeros((4, 1))], 1)
    parts = {0: faces(rng, (0, 0, 0), (1.0, 1.0, 0.8), skip=ONLY_Z),
             1: np.concatenate([h, stray]),
             2: faces(rng, (2.0, 0.0, 0.0), (0.6, 0.5, 0.4)),
             3: faces(rng, (2.3, 0.0, 0.0), (0.6, 0.5, 0.4)),
             4: faces(rng, (0.0, 2.5, 0.0), (0.5, 0.5, 0.5))}
    gt = np.array([[0.05, 0.05, 0.0, 0.95, 0.95, 0.8],          # G
                   [2.05, 0.05, 0.0, 2.85, 0.45, 0.4],          # I + J
                   [2.05, 0.05, 0.0, 2.80, 0.45, 0.4],          # nearly the same box again: one prediction, two candidates
                   [0.05, 2.55, 0.0, 0.45, 2.95, 0.5]])         # K
    return parts, 5, gt


def bounding_box(points):
    """trimesh.points.PointCloud(points).bounding_box as (centroid, extents): the box of the bounds"""
    lo, hi = points.min(0), points.max(0)
    return (lo + hi) / 2, hi - lo


def reference_loop(train_utils, instances, log):
    """test.py:294-326 / test_iou.py:373-406 on (object numbers, float64 points) entries; the geometry calls are the reference's own"""
    from scipy.spatial import distance
    inst_list = list(instances)                                                      # :294
    cnt, end_cnt = 0, len(instances)                                                 # :295
    while cnt < end_cnt:                                                             # :296
        cur_inst = inst_list.pop(0)                                                  # :297
        merge_list, remain_list = [cur_inst], []                                     # :298-299
        while len(inst_list) != 0:                                                   # :300
            targ_inst = inst_list.pop(0)                                             # :301
            cur_box, targ_box = bounding_box(cur_inst[1]), bounding_box(targ_inst[1])                        # :303-304
            cur_box_param, targ_box_param = np.concatenate(cur_box), np.concatenate(targ_box)                # :305-306
            is_overlap1, is_overlap2 = train_utils.compute_partial_iou(cur_box_param, targ_box_param)        # :307
            nearest = np.min(distance.cdist(cur_inst[1], targ_inst[1]), axis=0)                              # :311
            num_neighbor = np.sum(nearest < RADIUS)
            log.append(dict(cur=cur_inst[0], targ=targ_inst[0], over=(bool(is_overlap1), bool(is_overlap2)), near=int(num_neighbor),
                            on_edge=np.nonzero(np.abs(nearest - RADIUS) < MARGIN)[0], cur_box=cur_box_param, targ_box=targ_box_param))
            if (is_overlap1 or is_overlap2) and num_neighbor > MIN_NEIGHBORS:         # :312-314
                merge_list.append(targ_inst)                                         # :316
            else:
                remain_list.append(targ_inst)                                        # :319
        remain_list.append((sum((m[0] for m in merge_list), []), np.concatenate([m[1] for m in merge_list])))   # :322-323
        inst_list = remain_list                                                      # :324
        cnt += 1                                                                     # :326
    return inst_list


def check_pair(entry):
    """the conditions on one evaluated pair"""
    a, b = entry["cur_box"], entry["targ_box"]
    assert abs(entry["near"] - MIN_NEIGHBORS) > len(entry["on_edge"]), entry
    top = np.minimum(a[:3] + a[3:] / 2, b[:3] + b[3:] / 2)
    bottom = np.maximum(a[:3] - a[3:] / 2, b[:3] - b[3:] / 2)
    for k in range(3):
        one_flat_box = any(box[3 + k] == 0 and top[k] == box[k] and bottom[k] == box[k] for box in (a, b))
        assert abs(top[k] - bottom[k]) >= 1e-6 or one_flat_box, entry
    if (top > bottom).all():
        inter = (top - bottom).prod()
        for box in (a, b):
            assert abs(inter / box[3:].prod() - OVERLAP) >= 0.02, entry


def run_scene(train_utils, evaluation, rng, make):
    parts, n_objects, gt = make(rng)
    coord = np.concatenate(list(parts.values())).astype(np.float32)
    obj = np.concatenate([np.full(len(p), o, np.int32) for o, p in parts.items()])
    perm = rng.permutation(len(obj))
    coord, obj = coord[perm], obj[perm]
    for _ in range(6):                                          # remove the points on the 0.2 threshold, then assert
        x = coord.astype(np.float64)
        log = []
        final = reference_loop(train_utils, [([o], x[obj == o]) for o in range(n_objects) if (obj == o).any()], log)
        drop = []
        for e in log:
            order = np.concatenate([np.nonzero(obj == o)[0] for o in e["targ"]])   # the rows of the target set as the loop concatenated them
            drop.append(order[e["on_edge"]])
        drop = np.unique(np.concatenate(drop))
        if len(drop) == 0:
            break
        print(f"  removing {len(drop)} points on the threshold")
        coord, obj = np.delete(coord, drop, 0), np.delete(obj, drop)
    assert len(drop) == 0
    for e in log:
        check_pair(e)
    assert len(np.unique(coord, axis=0)) == len(coord)

    set_of = np.full(n_objects, -1, np.int32)
    pred_box = []
    for k, (members, pts) in enumerate(final):
        set_of[members] = k
        centroid, extents = bounding_box(pts)
        pred_box.append(np.hstack((centroid - extents / 2, centroid + extents / 2)))                        # test_iou.py:422
        lo32, hi32 = coord[np.isin(obj, members)].min(0), coord[np.isin(obj, members)].max(0)
        assert np.array_equal(pred_box[-1], np.concatenate([lo32, hi32]).astype(np.float64)), (members, pred_box[-1])
    pred_box = np.vstack(pred_box)                                                                          # :423

    iou = evaluation.DetectionMAP.compute_IoU(pred_box, gt)                                                 # evaluation.py:84
    assert (np.abs(iou - IOU_THRESHOLD) >= 0.02).all(), iou
    iou[iou < IOU_THRESHOLD] = 0                                                                            # :86
    tp, fp, fn = evaluation.DetectionMAP.compute_TP_FP_FN(iou.copy())                                       # :91
    score = evaluation.DetectionMAP(1, overlap_threshold=IOU_THRESHOLD)
    score.evaluate(pred_box.copy(), gt.copy())                                                              # test_iou.py:455
    acc = score.total_accumulators[0]
    assert acc.TP == len(tp) and acc.FN == fn and len(acc.predictions) == len(tp) + len(fp)
    pairs = np.array([[e["cur"][0], e["targ"][0], e["over"][0], e["over"][1], e["near"]] for e in log], np.int32)
    return dict(coord=coord, object=obj, n_objects=np.int32(n_objects), set_of_object=set_of, boxes=pred_box, gt_boxes=gt,
                tp=np.array(tp, np.float64), fp=np.array(fp, np.float64), fn=np.int32(fn), precision=np.float64(acc.precision[0]),
                recall=np.float64(acc.recall[0]), pairs=pairs), log, final


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    sys.modules["open3d"] = open3d_stand_in()
    sys.modules["skimage"] = types.ModuleType("skimage")
    sys.modules["skimage.transform"] = types.ModuleType("skimage.transform")
    sys.modules["skimage"].transform = sys.modules["skimage.transform"]
    sys.path.insert(0, a.reference)
    from util import evaluation, train_utils                    # the reference

    out = dict(radius=np.float64(RADIUS), overlap=np.float64(OVERLAP), min_neighbors=np.int32(MIN_NEIGHBORS), iou_threshold=np.float64(IOU_THRESHOLD))
    rng = np.random.default_rng(20261018)
    for name, make in (("a", scene_a), ("b", scene_b)):
        print(f"scene {name}")
        rec, log, final = run_scene(train_utils, evaluation, rng, make)
        assert 5000 <= len(rec["coord"]) <= 12000, len(rec["coord"])
        for e in log:
            print(f"  {e['cur']} vs {e['targ']}: overlap {e['over']}, near {e['near']}")
        print(f"  {len(rec['coord'])} points, final list {[m for m, _ in final]}, TP {rec['tp'].tolist()}, FP {rec['fp'].tolist()}, FN {int(rec['fn'])}, "
              f"precision {float(rec['precision']):.3f}, recall {float(rec['recall']):.3f}")
        near = {(tuple(e["cur"]), tuple(e["targ"])): e for e in log}
        if name == "a":
            assert [m for m, _ in final] == [[3, 4], [6], [0, 1], [2]]
            e = near[((0,), (1,))]
            assert e["over"] == (False, True) and e["near"] > MIN_NEIGHBORS                                    # (a) decided by one side
            e = near[((3,), (0, 1))]
            assert e["over"] == (False, False) and e["near"] > 100                                             # (b) a seam, no box overlap
            assert any(len(e["cur"]) > 1 and len(e["targ"]) > 1 for e in log)                                  # (d) two merged sets meet
            assert all(e["over"] == (False, False) for e in log if e["cur"] == [6] or e["targ"] == [6])        # (e) the flat object
            assert any(e["near"] > MIN_NEIGHBORS for e in log if e["cur"] == [6] or e["targ"] == [6])
            assert rec["set_of_object"][5] == -1 and rec["set_of_object"][6] >= 0                              # (f)
        else:
            for key in (((0,), (1,)), ((1,), (0,))):                                                          # (c) overlap, few near points
                if key in near:
                    assert any(near[key]["over"]) and 0 < near[key]["near"] <= MIN_NEIGHBORS, near[key]
            assert ((0,), (1,)) in near and ((1,), (0,)) in near
            assert rec["set_of_object"][2] == rec["set_of_object"][3] and len(final) == 4
        out.update({f"{k}_{name}": v for k, v in rec.items()})
    path = os.path.join(HERE, "merge_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
