"""Writes tests/golden/objects_reference.npz: the reference's own `instantiation_eval` (util/train_utils.py:547-737) on two synthetic
scenes of axis-aligned boxes - which face instances it groups into one object ("box support").  Run on the CPU where the reference
checkout, scikit-learn and scipy are at hand (nothing of the reference is copied):

    python tests/golden/make_golden_objects.py [--reference /root/reference]

Open3D is not needed: `open3d` is replaced in sys.modules by a pass-through stand-in that lives in THIS script (voxel_down_sample returns
the cloud, remove_radius_outlier returns (cloud, None)), so the clean-up of :716-720 hands every support back as it was and the face
instances of a support are recovered by matching its point rows.  The function is called on float64 copies of the fp32 scenes with a
zero shift.  DBSCAN.fit refuses an empty array, so every class 0 .. 17 has at least a few points; a class "absent from the scene" is a
dozen scattered points that form no instance.

Scenes: boxes with faces on a 0.025 grid (inset 0.05 from the box's edges, jittered by up to 0.004 inside the face's plane so that no
lattice distance sits on a threshold), 60 points per edge; face classes 0 = +z, 5 = -z, 1 = +x, 4 = -x, 2 = +y, 3 = -y; edge class =
6 + position of its face pair in lookup_face (:600).
  A: three boxes.  a is complete; b stands 0.02 beside a and has no +z face, so its (-x, +z) edge links a's +z face and the component
     spans both boxes; c stands apart and has a single edge.
  B: class 5 (-z) absent, so the four edge classes beside it are discarded although every such edge has a face beside it (:606-607);
     d and e without their -z faces, f a +x face with one edge whose other face is missing: an object of one face.
Conditions on the inputs, asserted here (not tolerances - offending points are removed before anything is recorded):
  - no same-class pair lies within 1e-5 of its DBSCAN eps (float64 distances of the fp32 coordinates);
  - for every (edge instance, face instance of its two face classes) |2 * count - size| exceeds the number of the edge's points whose
    nearest face distance lies within 1e-5 of 0.08;
  - the reference's returned supports are pairwise disjoint, i.e. its merge loop (:666) reached the fixed point;
  - every cluster is at least 5 points clear of its size threshold.
Per scene s in "a", "b": coord_s [n, 3] f32, pred_s [n] i32, object_s [n] i32 (objects numbered by ascending smallest face instance, -1 =
in none), instance_s [n] i32, instance_class_s / instance_size_s [I] (the reference's instance numbering, class-major), n_objects_s;
and the settings: radius, share, lookup_face, eps / min_samples / min_points per class."""
import argparse
import os
import sys
import types

import numpy as np

MARGIN = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
LOOKUP_FACE = [[0, 1], [0, 2], [1, 2], [0, 3], [1, 3], [0, 4], [2, 4], [3, 4], [1, 5], [2, 5], [3, 5], [4, 5]]
# face class -> (axis, side)
FACE = {0: (2, 1), 5: (2, 0), 1: (0, 1), 4: (0, 0), 2: (1, 1), 3: (1, 0)}
STEP, INSET, JITTER, EDGE_POINTS = 0.025, 0.05, 0.004, 60
RADIUS, SHARE = 0.08, 0.5
EPS = np.array([0.1] * 6 + [0.15] * 12)
MIN_SAMPLES = np.array([5] * 6 + [3] * 12, np.int32)
MIN_POINTS = np.array([50] * 6 + [20] * 12, np.int32)


def open3d_stand_in():
    class PointCloud:
        points = None

        def voxel_down_sample(self, voxel_size):
            return self

        def remove_radius_outlier(self, nb_points, radius):
            return self, None

    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a))
    return o3d


def face_points(rng, lo, hi, cls):
    axis, side = FACE[cls]
    u, v = [a for a in range(3) if a != axis]
    gu = np.arange(lo[u] + INSET, hi[u] - INSET + 1e-9, STEP)
    gv = np.arange(lo[v] + INSET, hi[v] - INSET + 1e-9, STEP)
    pts = np.zeros((len(gu) * len(gv), 3))
    uu, vv = np.meshgrid(gu, gv, indexing="ij")
    pts[:, u], pts[:, v] = uu.ravel(), vv.ravel()
    pts[:, [u, v]] += rng.uniform(-JITTER, JITTER, (len(pts), 2))
    pts[:, axis] = hi[axis] if side else lo[axis]
    return pts


def edge_points(rng, lo, hi, pair):
    (a1, s1), (a2, s2) = FACE[pair[0]], FACE[pair[1]]
    along = 3 - a1 - a2
    pts = np.zeros((EDGE_POINTS, 3))
    pts[:, along] = np.linspace(lo[along] + 0.01, hi[along] - 0.01, EDGE_POINTS) + rng.uniform(-JITTER, JITTER, EDGE_POINTS)
    pts[:, a1] = hi[a1] if s1 else lo[a1]
    pts[:, a2] = hi[a2] if s2 else lo[a2]
    return pts


def box(rng, lo, size, faces=range(6), edges=range(12)):
    lo = np.asarray(lo, float)
    hi = lo + np.asarray(size, float)
    coord, pred = [], []
    for c in faces:
        p = face_points(rng, lo, hi, c)
        coord.append(p)
        pred += [c] * len(p)
    for e in edges:
        p = edge_points(rng, lo, hi, LOOKUP_FACE[e])
        coord.append(p)
        pred += [6 + e] * len(p)
    return np.concatenate(coord), np.array(pred, np.int32)


def stray(rng, cls, corner, count=12):
    """a class that is there for DBSCAN.fit but forms no instance: points 0.4 apart"""
    pts = np.asarray(corner, float) + 0.4 * np.stack(np.unravel_index(np.arange(count), (3, 2, 2)), 1) + rng.uniform(-0.01, 0.01, (count, 3))
    return pts, np.full(count, cls, np.int32)


def scene_a(rng):
    parts = [box(rng, (0.0, 0.0, 0.0), (0.7, 0.6, 0.5)),
             box(rng, (0.72, -0.2, 0.0), (0.6, 1.0, 0.5), faces=[5, 1, 4, 2, 3]),   # (its x-parallel edges 0.2 off a's: separate instances)
             box(rng, (0.3, 1.5, 0.0), (0.8, 0.7, 0.6), edges=[0])]
    return parts


def scene_b(rng):
    parts = [box(rng, (0.0, 0.0, 0.0), (0.8, 0.7, 0.5), faces=[0, 1, 4, 2, 3]),
             box(rng, (1.4, 0.1, 0.0), (0.7, 0.8, 0.6), faces=[0, 1, 4, 2, 3]),
             box(rng, (0.2, 1.6, 0.0), (0.6, 0.6, 0.6), faces=[1], edges=[0]),
             stray(rng, 5, (2.6, 2.6, 1.0))]
    return parts


def near_threshold(x32, eps):
    """indices of the points that belong to a pair with |dist - eps| < MARGIN (float64 distances of the fp32 coordinates)"""
    x = x32.astype(np.float64)
    out = []
    for r0 in range(0, len(x), 1024):
        d = np.sqrt(((x[r0:r0 + 1024, None, :] - x[None, :, :]) ** 2).sum(-1))
        i, j = np.nonzero(np.abs(d - float(eps)) < MARGIN)
        out += [i + r0, j]
    return np.unique(np.concatenate(out)) if out else np.zeros(0, np.int64)


def build_scene(rng, parts):
    coord = np.concatenate([p[0] for p in parts]).astype(np.float32)
    pred = np.concatenate([p[1] for p in parts])
    perm = rng.permutation(len(pred))
    coord, pred = coord[perm], pred[perm]
    for _ in range(4):                                          # the condition on the DBSCAN inputs: remove, then assert
        drop = [np.nonzero(pred == c)[0][near_threshold(coord[pred == c], np.float32(EPS[c]))] for c in range(18)]
        drop = np.unique(np.concatenate(drop))
        if len(drop) == 0:
            break
        coord, pred = np.delete(coord, drop, 0), np.delete(pred, drop)
    assert all(len(near_threshold(coord[pred == c], np.float32(EPS[c]))) == 0 for c in range(18))
    assert len(np.unique(coord, axis=0)) == len(coord)          # rows are matched by value below
    assert set(np.unique(pred)) == set(range(18))
    return coord, pred


def reference_instances(coord, pred):
    """the reference's loop (:553-592) restated for the instance of every POINT (the reference keeps point arrays only)"""
    from sklearn.cluster import DBSCAN
    instance, inst_class, inst_size = np.full(len(pred), -1, np.int32), [], []
    x = coord.astype(np.float64)
    for c in range(int(pred.max()) + 1):
        rows = np.nonzero(pred == c)[0]
        labels = DBSCAN(eps=EPS[c], min_samples=int(MIN_SAMPLES[c])).fit(x[rows]).labels_
        for j in range(labels.max() + 1):
            size = int((labels == j).sum())
            assert abs(size - int(MIN_POINTS[c])) >= 5, (c, j, size)
            if size > MIN_POINTS[c]:
                instance[rows[labels == j]] = len(inst_class)
                inst_class.append(c)
                inst_size.append(size)
    return instance, np.array(inst_class, np.int32), np.array(inst_size, np.int32)


def check_contacts(coord, instance, inst_class):
    """every (edge instance, candidate face instance) decides clear of the points that sit on the 0.08 threshold"""
    from scipy.spatial import distance
    x = coord.astype(np.float64)
    for e in np.nonzero((inst_class >= 6) & (inst_class < 18))[0]:
        pe = x[instance == e]
        for k in np.nonzero(np.isin(inst_class, LOOKUP_FACE[inst_class[e] - 6]))[0]:
            d = np.min(distance.cdist(pe, x[instance == k]), axis=1)
            count, on_edge = int(np.sum(d < RADIUS)), int(np.sum(np.abs(d - RADIUS) < MARGIN))
            assert abs(2 * count - len(pe)) > on_edge, (e, k, count, len(pe), on_edge)


def run_reference(train_utils, coord, pred):
    x = coord.astype(np.float64)
    supports = train_utils.instantiation_eval("", "golden", x, np.zeros_like(x), pred.astype(np.int64))
    row_of = {r.tobytes(): i for i, r in enumerate(x)}
    return [np.array([row_of[np.ascontiguousarray(r).tobytes()] for r in np.asarray(s)], np.int64) for s in supports]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    sys.modules["open3d"] = open3d_stand_in()
    sys.path.insert(0, a.reference)
    from util import train_utils                                # the reference

    out = dict(radius=np.float64(RADIUS), share=np.float64(SHARE), lookup_face=np.array(LOOKUP_FACE, np.int32), eps=EPS,
               min_samples=MIN_SAMPLES, min_points=MIN_POINTS)
    rng = np.random.default_rng(20261019)
    for name, make in (("a", scene_a), ("b", scene_b)):
        coord, pred = build_scene(rng, make(rng))
        assert 5000 <= len(coord) <= 12000, len(coord)
        instance, inst_class, inst_size = reference_instances(coord, pred)
        check_contacts(coord, instance, inst_class)
        supports = run_reference(train_utils, coord, pred)
        obj = np.full(len(coord), -1, np.int32)
        keys = []
        for rows in supports:
            assert (obj[rows] == -1).all(), "the reference's supports overlap: its merge loop has not reached the fixed point"
            faces = np.unique(instance[rows])
            assert faces.min() >= 0 and (inst_class[faces] < 6).all()
            assert len(rows) == int(inst_size[faces].sum())     # whole face instances, nothing else
            obj[rows] = len(keys)
            keys.append(int(faces.min()))
        rank = np.argsort(np.argsort(keys)).astype(np.int32)    # numbered by ascending smallest face instance
        obj[obj >= 0] = rank[obj[obj >= 0]]
        print(f"scene {name}: {len(coord)} points, {int((inst_class < 6).sum())} face and {int((inst_class >= 6).sum())} edge instances, "
              f"{len(supports)} objects of {[int(len(np.unique(instance[obj == o]))) for o in range(len(supports))]} faces")
        out.update({f"coord_{name}": coord, f"pred_{name}": pred, f"object_{name}": obj, f"instance_{name}": instance,
                    f"instance_class_{name}": inst_class, f"instance_size_{name}": inst_size, f"n_objects_{name}": np.int32(len(supports))})
    path = os.path.join(HERE, "objects_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
