"""Oracle of csrc/contacts.hip and of cluster.objects: numpy, brute force over all pairs, the kernel's fp32 arithmetic.

    count[a, b]  = points p of label a for which some q of label b has d2(p, q) < r2 (strict; once per b; p is its own partner);
    min_d2[a, b] = min of d2(p, q) over p in a, q in b, +inf where either label is empty;
    d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = xp - xq, every operation rounded to fp32, r2 = fp32(r) * fp32(r) rounded once.

`objects_literal` restates the pairing and the merge loop of `instantiation_eval` (util/train_utils.py:595-689) line by line, `objects`
the rules 1-6 of cluster.link_objects.  scipy is not imported here."""
import numpy as np

ROWS = 512  # rows of the pair matrix evaluated at a time
EDGE_FACES = [[0, 1], [0, 2], [1, 2], [0, 3], [1, 3], [0, 4], [2, 4], [3, 4], [1, 5], [2, 5], [3, 5], [4, 5]]  # lookup_face, :600


def pair_d2(xp, xq):
    """fp32 [len(xp), len(xq)]"""
    d = xp[:, None, :] - xq[None, :, :]                                   # fp32 differences
    sq = d * d                                                            # fp32 products, rounded before they are summed
    d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    assert d2.dtype == np.float32
    return d2


def contacts(xyz, label, radius, n_labels=None):
    """-> (count int32 [I, I], min_d2 float32 [I, I]), as stratified_transformer_amd.cluster.contacts defines them"""
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    label = np.asarray(label).astype(np.int64).reshape(-1)
    n_labels = int(n_labels) if n_labels is not None else (max(int(label.max()) + 1, 0) if len(label) else 0)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    count = np.zeros((n_labels, n_labels), dtype=np.int32)
    min_d2 = np.full((n_labels, n_labels), np.inf, dtype=np.float32)
    valid = np.nonzero(label >= 0)[0]
    valid = valid[np.argsort(label[valid], kind="stable")]                # the columns of one label side by side
    xv, lv = x[valid], label[valid]
    present, starts = np.unique(lv, return_index=True)                    # the labels that have points, and their first column
    for a in present.tolist():
        rows = valid[lv == a]
        for r0 in range(0, len(rows), ROWS):
            d2 = pair_d2(x[rows[r0:r0 + ROWS]], xv)                       # [rows, n_valid]
            near = np.logical_or.reduceat(d2 < r2, starts, axis=1)        # [rows, present]: some q of the label within reach
            count[a, present] += near.sum(0).astype(np.int32)
            min_d2[a, present] = np.minimum(min_d2[a, present], np.minimum.reduceat(d2, starts, axis=1).min(0))
    return count, min_d2


def pair_list(count, size, cls, share=0.5, face_classes=6, edge_faces=None):
    """:601-647 on the tables: per edge instance the face instances it links, in the reference's order of edge classes and instances"""
    edge_faces = EDGE_FACES if edge_faces is None else edge_faces
    cls = np.asarray(cls).astype(np.int64)
    indice_list = [np.nonzero(cls == c)[0].tolist() for c in range(face_classes)]                  # :589-592
    pairs, edges = [], []
    for cls_idx in range(len(edge_faces)):                                                         # e_cls_list[:12]
        f_inst_id1, f_inst_id2 = indice_list[edge_faces[cls_idx][0]], indice_list[edge_faces[cls_idx][1]]
        if len(f_inst_id1) == 0 or len(f_inst_id2) == 0:                                           # :606-607
            continue
        for e in np.nonzero(cls == face_classes + cls_idx)[0].tolist():
            paired = []
            for ids in (f_inst_id1, f_inst_id2):
                for k in ids:
                    r1 = int(count[e, k]) / int(size[e])                                           # :629 np.sum(dist1 < 0.08) / len(dist1)
                    if r1 > share:
                        paired.append(k)
                        break
            if paired:
                pairs.append(paired)
                edges.append(e)
    return pairs, edges


def merge_literal(pairs):
    """the merge loop of :666-689 as written: len + 100 rotations -> (list of sets, whether they are pairwise disjoint = fixed point)"""
    pair_list_ = [list(p) for p in pairs]
    for m in range(len(pair_list_) + 100):
        new_pair_list = []
        start = pair_list_[0]
        pair_list_ = pair_list_[1:]
        new_set = start
        for pair in pair_list_:
            intersect = set.intersection(set(start), set(pair))
            if intersect:
                new_set = new_set + pair
            else:
                new_pair_list.append(pair)
        new_pair_list.append(list(set(new_set)))
        pair_list_ = new_pair_list
    sets = [frozenset(p) for p in pair_list_]
    disjoint = all(not (a & b) for i, a in enumerate(sets) for b in sets[i + 1:])
    return sets, disjoint


def objects_literal(count, size, cls, share=0.5, face_classes=6, edge_faces=None):
    """the reference's pairing and its literal merge loop -> (set of frozensets of face instances, fixed point reached).  With no link
    the reference raises IndexError (pair_list[0], :670), and so does this."""
    pairs, _ = pair_list(count, size, cls, share, face_classes, edge_faces)
    sets, disjoint = merge_literal(pairs)
    return set(sets), disjoint


def components(pairs, n_inst):
    """connected components over the linked faces -> list of sorted lists, ascending smallest member"""
    parent = list(range(n_inst))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i

    for p in pairs:
        for k in p[1:]:
            a, b = find(p[0]), find(k)
            if a != b:
                parent[max(a, b)] = min(a, b)
    groups = {}
    for k in sorted({k for p in pairs for k in p}):
        groups.setdefault(find(k), []).append(k)
    return [groups[r] for r in sorted(groups)]


def objects(count, size, cls, share=0.5, face_classes=6, edge_faces=None):
    """rules 1-6 -> (object_of_instance int32 [I], n_objects)"""
    cls = np.asarray(cls).astype(np.int64)
    if share == 0.5:                                                       # rule 3 in integers
        pairs, edges = pair_list(2 * np.asarray(count).astype(np.int64), 2 * np.asarray(size).astype(np.int64), cls, 0.5, face_classes, edge_faces)
        check, _ = pair_list(count, size, cls, 0.5, face_classes, edge_faces)
        assert pairs == check
    else:
        pairs, edges = pair_list(count, size, cls, share, face_classes, edge_faces)
    comps = components(pairs, len(cls))
    object_of = np.full(len(cls), -1, dtype=np.int32)
    for number, faces in enumerate(comps):
        object_of[faces] = number
    for e, p in zip(edges, pairs):
        object_of[e] = object_of[p[0]]
    return object_of, len(comps)


def scene_objects(coord, instance, cls, size=None, radius=0.08, share=0.5, face_classes=6, edge_faces=None, count=None):
    """cluster.objects on the oracle -> (object int32 [N], object_of_instance int32 [I], n_objects); count: the contact counts, if at hand"""
    instance, cls = np.asarray(instance).astype(np.int64), np.asarray(cls).astype(np.int64)
    if count is None:
        count, _ = contacts(coord, instance, radius, len(cls))
    size = np.bincount(instance[instance >= 0], minlength=len(cls)) if size is None else np.asarray(size)
    object_of, n_objects = objects(count, size, cls, share, face_classes, edge_faces)
    face_object = np.where(cls < face_classes, object_of, -1).astype(np.int32)
    obj = np.where(instance >= 0, face_object[np.clip(instance, 0, None)] if len(cls) else -1, -1).astype(np.int32)
    return obj, object_of, n_objects
