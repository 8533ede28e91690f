"""Oracle of csrc/boxes.hip and of cluster.merge_objects / box_detection: numpy, brute force over all pairs, the kernel's fp32 arithmetic.

    boxes:       lo / hi [I, 3] = min / max of the points of every label (+inf / -inf for an empty one), size [I];
    reach_rows:  [N, ceil(I / 32)] uint32, bit b of row p = some q of label b has d2(p, q) < r2 (strict), p's own bit cleared, zeros for
                 an unlabelled p; d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = xp - xq, every operation rounded to fp32, r2 = fp32(r) *
                 fp32(r) rounded once (tests/contacts_oracle.pair_d2);
    patterns:    the distinct (object, row) pairs of the points whose row is not empty, and their counts.

`merge_literal` is the rotating loop of test.py:294-326 ON POINT ARRAYS: every set is the array of its points, its box is taken from the
points, and num_neighbor is counted per pair of sets by brute force over their points (in the device's fp32 arithmetic).  It knows
nothing of rows or patterns, so it checks cluster.merge_sets' pattern formulation instead of restating it.  `detection` is the matching of
util/evaluation.py:68-96, :109-152, :194-239 written out with loops.  scipy and trimesh are not imported here."""
import numpy as np

from tests.contacts_oracle import ROWS, pair_d2


def _inputs(xyz, label, n_labels):
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    label = np.asarray(label).astype(np.int64).reshape(-1)
    n_labels = int(n_labels) if n_labels is not None else (max(int(label.max()) + 1, 0) if len(label) else 0)
    return x, label, n_labels


def boxes(xyz, label, n_labels=None):
    """-> (lo float32 [I, 3], hi float32 [I, 3], size int32 [I])"""
    x, label, n_labels = _inputs(xyz, label, n_labels)
    lo = np.full((n_labels, 3), np.inf, dtype=np.float32)
    hi = np.full((n_labels, 3), -np.inf, dtype=np.float32)
    size = np.zeros(n_labels, dtype=np.int32)
    for a in np.unique(label[label >= 0]).tolist():
        pts = x[label == a]
        lo[a], hi[a], size[a] = pts.min(0), pts.max(0), len(pts)
    return lo, hi, size


def reach_rows(xyz, label, radius, n_labels=None):
    """-> uint32 [N, ceil(I / 32)], in the order of the input points"""
    x, label, n_labels = _inputs(xyz, label, n_labels)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    rows = np.zeros((len(x), (n_labels + 31) // 32), dtype=np.uint32)
    valid = np.nonzero(label >= 0)[0]
    valid = valid[np.argsort(label[valid], kind="stable")]                # the columns of one label side by side
    xv, lv = x[valid], label[valid]
    present, starts = np.unique(lv, return_index=True)
    for r0 in range(0, len(valid), ROWS):
        mine = valid[r0:r0 + ROWS]
        near = np.logical_or.reduceat(pair_d2(x[mine], xv) < r2, starts, axis=1)           # [rows, present]
        near[np.arange(len(mine)), np.searchsorted(present, label[mine])] = False        # the point's own label
        for k, b in enumerate(present.tolist()):
            rows[mine, b >> 5] |= near[:, k].astype(np.uint32) << np.uint32(b & 31)
    return rows


def patterns(label, rows):
    """-> (pat_object int32 [P], pat_rows uint32 [P, words], pat_count int64 [P]) of the points whose row is not empty"""
    label = np.asarray(label).astype(np.int64).reshape(-1)
    border = rows.any(1)
    keyed = np.concatenate([label[border, None], rows[border].astype(np.int64)], 1)
    if len(keyed) == 0:
        return np.zeros(0, np.int32), np.zeros((0, rows.shape[1]), np.uint32), np.zeros(0, np.int64)
    pat, count = np.unique(keyed, axis=0, return_counts=True)
    return pat[:, 0].astype(np.int32), pat[:, 1:].astype(np.uint32), count


def box_overlaps(pts_a, pts_b, overlap=0.3):
    """the two covered-share tests of util/train_utils.py:840-862 for the boxes around two float64 point arrays, written per axis"""
    lo_a, hi_a, lo_b, hi_b = pts_a.min(0), pts_a.max(0), pts_b.min(0), pts_b.max(0)
    c_a, e_a, c_b, e_b = (lo_a + hi_a) / 2, hi_a - lo_a, (lo_b + hi_b) / 2, hi_b - lo_b
    inter = 1.0
    for k in range(3):
        upper = min(c_a[k] + e_a[k] / 2, c_b[k] + e_b[k] / 2)
        lower = max(c_a[k] - e_a[k] / 2, c_b[k] - e_b[k] / 2)
        if not upper > lower:
            return False, False
    for k in range(3):                                                    # numpy's prod: left to right
        inter = inter * (min(c_a[k] + e_a[k] / 2, c_b[k] + e_b[k] / 2) - max(c_a[k] - e_a[k] / 2, c_b[k] - e_b[k] / 2))
    return inter / (e_a[0] * e_a[1] * e_a[2]) > overlap, inter / (e_b[0] * e_b[1] * e_b[2]) > overlap


def near_count(cur32, targ32, r2):
    """points of targ with some point of cur at d2 < r2, fp32 (the device's arithmetic)"""
    if len(cur32) == 0 or len(targ32) == 0:
        return 0
    hit = np.zeros(len(targ32), dtype=bool)
    for r0 in range(0, len(targ32), ROWS):
        hit[r0:r0 + ROWS] = (pair_d2(targ32[r0:r0 + ROWS], cur32) < r2).any(1)
    return int(hit.sum())


def merge_literal(xyz, label, n_labels=None, radius=0.2, overlap=0.3, min_neighbors=10, log=None):
    """the loop of test.py:294-326 on point arrays -> (set_of_object int32 [I], the final list as lists of objects, boxes float32 [S, 6]);
    log: a list that receives (current, target, overlap a, overlap b, num_neighbor) per evaluated pair"""
    x, label, n_labels = _inputs(xyz, label, n_labels)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    inst_list = [([a], x[label == a]) for a in range(n_labels) if (label == a).any()]
    cnt, end_cnt = 0, len(inst_list)
    while cnt < end_cnt and end_cnt >= 2:
        cur = inst_list.pop(0)
        merge_list, remain_list = [cur], []
        while len(inst_list) != 0:
            targ = inst_list.pop(0)
            over_a, over_b = box_overlaps(cur[1].astype(np.float64), targ[1].astype(np.float64), overlap)
            num_neighbor = near_count(cur[1], targ[1], r2)
            if log is not None:
                log.append((list(cur[0]), list(targ[0]), bool(over_a), bool(over_b), num_neighbor))
            if (over_a or over_b) and num_neighbor > min_neighbors:
                merge_list.append(targ)
            else:
                remain_list.append(targ)
        remain_list.append((sum((m[0] for m in merge_list), []), np.concatenate([m[1] for m in merge_list])))
        inst_list = remain_list
        cnt += 1
    set_of = np.full(n_labels, -1, dtype=np.int32)
    for number, (members, _) in enumerate(inst_list):
        set_of[members] = number
    box = np.array([np.concatenate([p.min(0), p.max(0)]) for _, p in inst_list], dtype=np.float32).reshape(len(inst_list), 6)
    return set_of, [m for m, _ in inst_list], box


def merged_points(label, set_of):
    """the per-point result of cluster.merge_objects"""
    label = np.asarray(label).astype(np.int64)
    table = np.concatenate([np.asarray(set_of, np.int32), np.full(1, -1, np.int32)])
    return table[label]


def detection(pred_box, gt_box, threshold=0.5):
    """-> (tp list, fp list, fn, precision or None, recall or None); IoU pair by pair with loops, the clip bound of
    util/evaluation.py:125 (the largest difference over all pairs and axes) included"""
    pred, gt = np.asarray(pred_box, np.float64).reshape(-1, 6), np.asarray(gt_box, np.float64).reshape(-1, 6)
    iou = np.zeros((len(pred), len(gt)))
    if len(pred) and len(gt):
        bound = max(min(p[3 + k], g[3 + k]) - max(p[k], g[k]) for p in pred for g in gt for k in range(3))
        for i, p in enumerate(pred):
            for j, g in enumerate(gt):
                edge = [min(p[3 + k], g[3 + k]) - max(p[k], g[k]) for k in range(3)]
                edge = [min(max(e, 0.0), bound) for e in edge]                    # numpy's clip: the upper bound wins
                inter = edge[0] * edge[1] * edge[2]
                union = (p[3] - p[0]) * (p[4] - p[1]) * (p[5] - p[2]) + (g[3] - g[0]) * (g[4] - g[1]) * (g[5] - g[2]) - inter
                with np.errstate(all="ignore"):
                    iou[i, j] = np.float64(inter) / np.float64(union)
    iou[iou < threshold] = 0
    used, tp, fp = set(), [], []
    for i in range(len(pred)):
        cands = [(iou[i, j], -j) for j in range(len(gt)) if iou[i, j] != 0 and j not in used]
        if cands:
            value, minus_j = max(cands)                                             # the largest IoU, the first ground-truth box among equals
            used.add(-minus_j)
            tp.append(float(value))
        else:
            fp.append(-1.0)
    fn = len(gt) - len(used)
    return tp, fp, fn, (len(tp) / (len(tp) + len(fp)) if tp or fp else None), (len(tp) / (len(tp) + fn) if len(tp) + fn else None)
