"""numpy restatement of the fork's box-detection pass in front of the clustering, the oracle of stratified_transformer_amd.evaluate's
scene_predict / dense_points / SceneVotes(shifts=True) and of cluster.detect_boxes:

    votes_shift_add     test_iou.py:337-338      pred[idx, :] += softmax(logits); pred_shift[idx, :] += shift - two indexed assignments
    scene_predict       test_iou.py:266-338      evaltile_oracle.scene_eval's loop with the second accumulator and no normalisation
    dense_points        test_iou.py:147-151      one DBSCAN of the scene, the clusters with more than 50 points, cluster by cluster
    chain               test_iou.py:356-422      instances -> objects -> clean_supports -> merge, on the four existing oracles

PARITY UNPINNED as in evaltile_oracle: the loop sits inline in the fork's test() and cannot be executed on its own.  The dense-point
filter is pinned by tests/test_detect_cpu.py against scikit-learn itself.  The votes stay in float64 (evaltile_oracle.votes_add); the
shift accumulator is fp32 like the fork's `torch.zeros((len(coord), 3)).cuda()`: one fp32 add per write, so the device is compared
bit for bit.

The scenes of the tests are built here as well: the three-blob cloud of the filter and the labelled box scene of the detection."""
import numpy as np

from tests import contacts_oracle, dbscan_oracle, merge_oracle, supports_oracle
from tests import evaltile_oracle as E

FACE = {0: (2, 1), 5: (2, 0), 1: (0, 1), 4: (0, 0), 2: (1, 1), 3: (1, 0)}   # face class -> (axis, side), as tests/golden/make_golden_objects.py
EDGE_FACES = ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (0, 4), (2, 4), (3, 4), (1, 5), (2, 5), (3, 5), (4, 5))   # cluster.EDGE_FACES
CLASSES = 18
FACE_SETTINGS, EDGE_SETTINGS = (0.1, 5, 50), (0.15, 3, 20)


def votes_shift_add(pred, shift, logits, shift_rows, idx):
    """:337-338 on pred float64 [n_points, classes] and shift float32 [n_points, 3], in place.  Votes as evaltile_oracle.votes_add.  Shift:
    every row computes shift[idx[r]] + float32(shift_rows[r]) in fp32 from the values BEFORE the call, then the rows are assigned in
    order - the last row of a repeated index stays, the same row that wrote the votes."""
    assert shift.dtype == np.float32
    E.votes_add(pred, logits, idx)
    rows = shift[idx] + np.asarray(shift_rows).astype(np.float32)
    assert rows.dtype == np.float32
    for r in range(len(idx)):
        shift[idx[r]] = rows[r]
    return pred, shift


def scene_predict(model_fn, coord, feat, voxelize, voxel_size, voxel_max, classes, batch_size_test=5, feat_div=255.0, concat_xyz=False,
                  priority=None):
    """:266-338 for one scene; arguments as evaltile_oracle.scene_eval, model_fn(feat f32, coord f32, offset i32, batch i64) -> (logits, shift).
    -> (pred float64 [N, classes], RAW; shift float32 [N, 3]: per point the SUM over the batches that wrote it; visits int64 [N]: the
    number of batches that wrote the point; the number of crops)"""
    n = coord.shape[0]
    if voxel_size:
        coord = coord - coord.min(0)
        parts = E.scene_parts(*voxelize(coord, voxel_size))
    else:
        parts = E.scene_parts(None, None, n)
    items = []
    for i, idx_part in enumerate(parts):
        coord_part, feat_part = coord[idx_part], feat[idx_part]
        if voxel_max and len(idx_part) > voxel_max:
            for crop in E.crop_cover(coord_part, voxel_max, priority[i])[0]:
                items.append((idx_part[crop],) + E.input_normalize(coord_part[crop], feat_part[crop], feat_div))
        else:
            items.append((idx_part,) + E.input_normalize(coord_part, feat_part, feat_div))
    pred, shift, visits = np.zeros((n, classes)), np.zeros((n, 3), np.float32), np.zeros(n, np.int64)
    for s in range(0, len(items), batch_size_test):
        chunk = items[s:s + batch_size_test]
        idx_b, coord_b, feat_b = (np.concatenate([c[k] for c in chunk]) for k in range(3))
        sizes = np.array([len(c[0]) for c in chunk])
        offset, batch = np.cumsum(sizes).astype(np.int32), np.repeat(np.arange(len(chunk)), sizes)
        if concat_xyz:
            feat_b = np.concatenate([feat_b, coord_b], 1)
        logits, shift_rows = model_fn(feat_b, coord_b, offset, batch)
        votes_shift_add(pred, shift, logits, shift_rows, idx_b)
        visits[np.unique(idx_b)] += 1
    return pred, shift, visits, len(items)


def lookup_model(table, shift_table, classes):
    """model_fn of the end-to-end tests: the first feature column carries the point's own index (exact in fp32 below 2^24);
    logits = 8 * one_hot(table[i]), shift = shift_table[i]"""
    def model_fn(feat, coord, offset, batch):
        i = feat[:, 0].astype(np.int64)
        assert np.array_equal(i.astype(np.float32), feat[:, 0])
        logits = np.zeros((len(i), classes), np.float32)
        logits[np.arange(len(i)), table[i]] = 8.0
        return logits, shift_table[i]
    return model_fn


def dense_points(coord, eps=0.1, min_samples=5, min_points=50):
    """:147-151 on dbscan_oracle (fp32 distances) -> (coord_kept, index int64 [K] into coord): the clusters with MORE than min_points
    points in ascending cluster number, every cluster in ascending original index; noise (-1) is in no cluster"""
    labels = dbscan_oracle.dbscan(coord, eps, min_samples)[0] if len(coord) else np.zeros(0, np.int32)
    kept = [np.nonzero(labels == c)[0] for c in range(int(labels.max()) + 1 if len(labels) else 0)]
    index = np.concatenate([k for k in kept if len(k) > min_points] + [np.zeros(0, np.int64)]).astype(np.int64)
    return coord[index], index


def blob_cloud(seed=2, sizes=(60, 51, 50), noise=25):
    """the filter's cloud: blobs of `sizes` points, each uniform in a cube of edge 0.05 (every pair closer than eps 0.1: all of a blob's points
    are core points of one cluster) 1 apart, `noise` scattered points on a 0.5 lattice 3 away from them; shuffled, so that the cluster
    numbers (ascending smallest index) are not the order of `sizes` by construction and a cluster's points are interleaved with the others
    -> (coord float64 [sum + noise, 3], blob int64: the blob of every point, -1 for the scattered ones)"""
    rng = np.random.default_rng(seed)
    pts = [np.array([1.0 * b, 0.0, 0.0]) + rng.uniform(0, 0.05, (s, 3)) for b, s in enumerate(sizes)]
    pts.append(np.array([0.0, 3.0, 0.0]) + 0.5 * np.stack([np.arange(noise) % 5, np.arange(noise) // 5, np.zeros(noise)], 1) + rng.uniform(0, 0.01, (noise, 3)))
    blob = np.concatenate([np.full(s, b) for b, s in enumerate(sizes)] + [np.full(noise, -1)])
    perm = rng.permutation(len(blob))
    return np.concatenate(pts)[perm], blob[perm]


def labelled_box(rng, lo, size, edge_points=30):
    """one box: its six faces on a 0.025 grid (inset 0.05, jittered inside the plane) and edge_points per edge, classes 0..5 and 6..17"""
    lo = np.asarray(lo, float)
    hi = lo + np.asarray(size, float)
    coord, pred = [], []
    for c, (axis, side) in FACE.items():
        u, v = [a for a in range(3) if a != axis]
        uu, vv = np.meshgrid(np.arange(lo[u] + 0.05, hi[u] - 0.05 + 1e-9, 0.025), np.arange(lo[v] + 0.05, hi[v] - 0.05 + 1e-9, 0.025), indexing="ij")
        p = np.zeros((uu.size, 3))
        p[:, u], p[:, v], p[:, axis] = uu.ravel(), vv.ravel(), hi[axis] if side else lo[axis]
        p[:, [u, v]] += rng.uniform(-0.004, 0.004, (len(p), 2))
        coord.append(p)
        pred += [c] * len(p)
    for e, (f1, f2) in enumerate(EDGE_FACES):
        (a1, s1), (a2, s2) = FACE[f1], FACE[f2]
        along = 3 - a1 - a2
        p = np.zeros((edge_points, 3))
        p[:, along] = np.linspace(lo[along] + 0.01, hi[along] - 0.01, edge_points)
        p[:, a1], p[:, a2] = hi[a1] if s1 else lo[a1], hi[a2] if s2 else lo[a2]
        p += rng.normal(0, 0.004, p.shape)
        coord.append(p)
        pred += [6 + e] * edge_points
    return np.concatenate(coord), np.array(pred, np.int64)


def box_scene(seed=3, corners=((0.0, 0.0, 0.0), (0.13, 0.13, 0.13), (1.5, 0.0, 0.0), (0.0, 1.5, 0.0)), size=(0.6, 0.5, 0.4), strays=6, loose=40):
    """The detection scene: one labelled_box per corner - the first two 0.13 apart on every axis, so that no face or edge instance of one
    joins the other's (0.13 > eps 0.1; 0.184 > eps 0.15 for the edges) while their boxes overlap by more than the merge's 0.3 and hundreds
    of points lie within its 0.2: they merge.  Per box `strays` points of face class 0 that the model's shift carries onto the top face
    from 0.4 to 0.6 above it: part of the instance (DBSCAN runs on coord + shift) and of the object, removed by the clean-up of the support.
    `loose` scattered points 3 away on a 0.5 lattice: in a class, in no instance.  Every other shift is a few millimetres.  Shuffled.
    -> (coord float32 [N, 3], table int64 [N]: the class the model gives every point, shift_table float32 [N, 3],
        gt_box float64 [len(corners), 6] = lo | hi of every box)"""
    rng = np.random.default_rng(seed)
    coord, table, shift = [], [], []
    for corner in corners:
        c, p = labelled_box(rng, corner, size)
        on_top = np.asarray(corner) + np.asarray(size) * np.concatenate([rng.uniform(0.2, 0.8, (strays, 2)), np.ones((strays, 1))], 1)
        lift = np.concatenate([np.zeros((strays, 2)), rng.uniform(0.4, 0.6, (strays, 1))], 1)
        coord += [c, on_top + lift]
        table += [p, np.zeros(strays, np.int64)]
        shift += [rng.normal(0, 0.002, c.shape), 0.0 - lift]                            # (0.0 - 0.0: no negative zeros)
    if loose:
        coord.append(np.array([0.0, 0.0, 3.0]) + 0.5 * np.stack([np.arange(loose) % 7, np.arange(loose) // 7, np.zeros(loose)], 1))
        table.append(rng.integers(0, CLASSES, loose))
        shift.append(np.zeros((loose, 3)))
    coord, table, shift = np.concatenate(coord).astype(np.float32), np.concatenate(table), np.concatenate(shift).astype(np.float32)
    perm = rng.permutation(len(table))
    gt = np.array([np.concatenate([np.asarray(c, float), np.asarray(c, float) + np.asarray(size, float)]) for c in corners]).reshape(len(corners), 6)
    return coord[perm], table[perm], shift[perm], gt


def chain(coord, shift, pred):
    """:356-422 on the four existing oracles with the reference's settings -> dict(instance, obj, supports = clean_supports' tuple,
    merge = merge_literal's (set_of_object, sets, boxes))"""
    n_classes = CLASSES
    eps = np.array([FACE_SETTINGS[0] if c < 6 else EDGE_SETTINGS[0] for c in range(n_classes)], np.float32)
    ms = np.array([FACE_SETTINGS[1] if c < 6 else EDGE_SETTINGS[1] for c in range(n_classes)], np.int32)
    mp = np.array([FACE_SETTINGS[2] if c < 6 else EDGE_SETTINGS[2] for c in range(n_classes)], np.int32)
    instance, cls, size = dbscan_oracle.instances(coord, shift, pred, eps, ms, mp)
    obj, _, n_objects = contacts_oracle.scene_objects(coord, instance, cls, size)
    supports = supports_oracle.clean_supports(coord, obj, n_objects)
    return dict(instance=instance, obj=obj, n_objects=n_objects, supports=supports,
                merge=merge_oracle.merge_literal(supports[0], supports[1], supports[3]))
