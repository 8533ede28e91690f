"""The step directly behind the model, on the device: the DCF fork's evaluation and training utilities add the predicted shift to
the coordinates, split the points by predicted class and run sklearn.cluster.DBSCAN per class on the host (util/train_utils.py:218-237,
:547-566; test.py:272-276).  `dbscan` is that clustering on csrc/dbscan.hip for all classes of a scene at once, `instances` the
clustering of `instantiation_eval` with its size threshold and instance numbering.  scikit-learn is not needed (and not imported).

Semantics (scikit-learn's, pinned by tests/golden/dbscan_sklearn.npz):
  1. j is a neighbour of i when both are in the same group and dist(i, j) <= eps (inclusive; i is its own neighbour);
  2. i is a core point when it has at least min_samples neighbours;
  3. the clusters are the connected components of the core points, numbered 0, 1, ... PER GROUP by ascending smallest core index;
  4. a non-core point with a core neighbour takes the smallest cluster number among its core neighbours, every other point gets -1.
Distances are evaluated in fp32 as ((dx*dx) + (dy*dy)) + (dz*dz) <= eps*eps (scikit-learn: float64), so a pair whose distance is within
about 1e-6 of eps may fall on the other side; everything else is equal label for label.

The second half of `instantiation_eval` (util/train_utils.py:595-714: which face instances an edge instance links, merged into objects)
is `objects`, on `contacts` (csrc/contacts.hip): per pair of labels, how many points of one set have a point of the other within a
radius, and how close the two sets come - the question the fork also asks at :251-261 and test.py:311.  `link_objects` is the pairing
and merging on plain host arrays.  scipy is not needed (and not imported).

The step behind that, the OBB merging of test.py:294-326 (test_iou.py:373-406), is `merge_objects` on `label_boxes` and the reach rows of
csrc/boxes.hip; `merge_sets` is its rotating loop on plain host arrays, `box_detection` the score test_iou.py:455-464 takes from the
merged boxes (util/evaluation.py).  trimesh is not needed (and not imported).

Between the two the reference cleans every support with Open3D (util/train_utils.py:716-723: voxel means, then radius outliers):
`clean_supports` on csrc/supports.hip; `box_supports` is instances -> objects -> clean_supports in one call, what `instantiation_eval`
returns.  Open3D is not needed (and not imported).

dbscan, contacts / objects, clean_supports and merge_objects stand on ONE fixed-radius grid: `_scan` (the read-back up front), `_dims` and `_grid` (cell
keys, torch's sort, the nine prepared runs per point) build it here, csrc/radius_grid.h walks it on the device for all of them.
"""
import contextlib
import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import ptr

MAX_ROUNDS = 64            # of the component loop: the trees at least halve per round (csrc/dbscan.hip), so 2^31 points need 32
CELL_MARGIN = 1.0 + 2.0 ** -7   # the grid's cells are this much wider than the largest eps (fp32 rounding of the distance test)
MAX_CELLS_PER_AXIS = 1 << 20
REG_LABELS = 64             # csrc/radius_grid.h keeps rows of up to this many labels in registers: no bitmap
MAX_BITMAP_BYTES = 1 << 30  # of the [n_valid, ceil(I / 32)] rows of labels in reach (more than REG_LABELS labels)
MAX_LABELS = 1 << 15        # the [I, I] tables are indexed with ints
LAST = {"rounds": 0, "launches": 0}   # of the most recent dbscan() call (tools/bench_dbscan.py, the chain test)

# instantiation_eval's settings (util/train_utils.py:558-563): faces (classes below 6) and edges
FACE_CLASSES = 6
FACE_SETTINGS = (0.1, 5, 50)
EDGE_SETTINGS = (0.15, 3, 20)


def _gpu(t, who, name):
    if not getattr(t, "is_cuda", False):
        raise RuntimeError(f"{who}: {name}: expected a GPU tensor (the pointops2 HIP path has no CPU fallback), got {getattr(t, 'device', type(t).__name__)}")


def _per_group(value, n_groups, dtype, name):
    """scalar / sequence / tensor -> numpy [G] (G taken from the value when n_groups is None)"""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    a = np.asarray(value)
    if a.dtype == object or a.dtype.kind not in "fiu":
        raise TypeError(f"dbscan: {name} must be numeric, got {a.dtype}")
    if dtype == np.int32 and a.dtype.kind == "f":
        if not np.all(a == np.floor(a)):
            raise ValueError(f"dbscan: {name} must be whole numbers")
    if a.ndim == 0:
        return None, a.astype(dtype)
    if a.ndim != 1 or a.shape[0] < 1:
        raise ValueError(f"dbscan: {name} must be a scalar or a sequence of length G, got shape {a.shape}")
    if n_groups is not None and a.shape[0] != n_groups:
        raise ValueError(f"dbscan: {name} has {a.shape[0]} entries for {n_groups} groups")
    return a.shape[0], a.astype(dtype)


def _settings(eps, min_samples, n_groups):
    """-> (G or None when both are scalars, eps f32 [G] or scalar, min_samples i32 [G] or scalar), validated"""
    g1, e = _per_group(eps, n_groups, np.float32, "eps")
    g2, m = _per_group(min_samples, n_groups, np.int32, "min_samples")
    if g1 is not None and g2 is not None and g1 != g2:
        raise ValueError(f"dbscan: eps has {g1} entries and min_samples {g2}")
    if not np.all(np.isfinite(e)) or not np.all(e > 0):
        raise ValueError("dbscan: eps must be finite and > 0")
    if not np.all(m >= 1):
        raise ValueError("dbscan: min_samples must be >= 1")
    return (g1 if g1 is not None else g2), e, m


def _check_tensors(who, xyz, label, noun):
    """xyz [N, 3] fp32 and its per-point `noun` ("group" / "label") int32 / int64 [N] or None, on one GPU"""
    _gpu(xyz, who, "xyz")
    if label is not None:
        _gpu(label, who, noun)
        if label.device != xyz.device:
            raise RuntimeError(f"{who}: {noun} is on {label.device}, xyz on {xyz.device}")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{who}: xyz must be [N, 3], got {tuple(xyz.shape)}")
    if xyz.dtype != torch.float32:
        raise TypeError(f"{who}: xyz must be float32, got {xyz.dtype}")
    if label is not None:
        if label.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{who}: {noun} must be int32 / int64, got {label.dtype}")
        if label.dim() != 1 or label.shape[0] != xyz.shape[0]:
            raise ValueError(f"{who}: {noun} must be [N] = [{xyz.shape[0]}], got {tuple(label.shape)}")


def _radius(who, radius):
    """-> (fp32(radius), its fp32 square, rounded once), both finite and > 0"""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: radius must be a number, got {type(radius).__name__}")
    with np.errstate(all="ignore"):
        r = np.float32(radius)
        if not np.isfinite(radius) or not radius > 0 or not np.isfinite(r * r) or not r * r > 0:
            raise ValueError(f"{who}: radius must be finite and > 0, also when squared in fp32, got {radius}")
    return r, np.float32(r * r)


def _label_count(who, n_labels, name="n_labels"):
    if n_labels is None:
        return None
    if isinstance(n_labels, bool) or not isinstance(n_labels, (int, np.integer)):
        raise TypeError(f"{who}: {name} must be an int, got {type(n_labels).__name__}")
    if n_labels < 0:
        raise ValueError(f"{who}: {name} must be >= 0, got {n_labels}")
    if n_labels > MAX_LABELS:
        raise ValueError(f"{who}: {n_labels} labels: at most {MAX_LABELS}")
    return int(n_labels)


def _label_range(who, n_labels, l_min, l_max, name="n_labels"):
    """-> the number of labels (n_labels, or l_max + 1), with every label in -1 .. that number - 1"""
    if n_labels is None:
        n_labels = _label_count(who, max(l_max + 1, 0), name)
    if l_min < -1 or l_max >= n_labels:
        raise ValueError(f"{who}: label values must be in -1 .. {n_labels - 1}, got {l_min} .. {l_max}")
    return n_labels


def _row_words(who, n_valid, n_labels):
    """-> words of a row of labels in reach; the rows of n_valid points must fit MAX_BITMAP_BYTES where they are kept in memory"""
    words = (n_labels + 31) // 32
    if n_labels > REG_LABELS and n_valid * words * 4 > MAX_BITMAP_BYTES:
        raise ValueError(f"{who}: the bitmap of {n_valid} points x {n_labels} labels takes {n_valid * words * 4} bytes, more than {MAX_BITMAP_BYTES}")
    return words


def _launch(counter, dev, name, *args):
    """one library launch on `dev`, counted in `counter` (LAST, LAST_CONTACTS or LAST_MERGE)"""
    counter["launches"] += 1
    with contextlib.nullcontext() if dev.index == torch.cuda.current_device() else torch.cuda.device(dev):
        _lib.call(name, *args, device=dev)


def _scan(who, xyz, label):
    """The one read-back up front: the label (group) range, the points that take part (label >= 0) and their bounding box
    -> (member bool [N], l_min, l_max, n_valid, origin float64 [3], top float64 [3]); ValueError for non-finite coordinates."""
    member = label >= 0
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=xyz.device)
    lo = torch.where(member[:, None], xyz, inf).amin(0)
    hi = torch.where(member[:, None], xyz, -inf).amax(0)
    finite = torch.isfinite(xyz).all()
    head = torch.cat([label.min()[None].double(), label.max()[None].double(), member.sum()[None].double(), finite[None].double(),
                      lo.double(), hi.double()]).cpu().numpy()
    if not head[3]:
        raise ValueError(f"{who}: xyz must be finite")
    return member, int(head[0]), int(head[1]), int(head[2]), head[4:7], head[7:10]


def _dims(who, n_groups, origin, top, cell):
    """-> the grid's cells per axis [nx, ny, nz]; ValueError when n_groups such grids do not fit the 64-bit cell keys"""
    dims = [int(np.floor((top[a] - origin[a]) / cell)) + 1 for a in range(3)]
    if max(dims) > MAX_CELLS_PER_AXIS or n_groups * dims[0] * dims[1] * dims[2] >= 2 ** 61:
        raise ValueError(f"{who}: the cloud spans {dims} cells of edge {cell:g}: too many for the 64-bit cell keys")
    return dims


def _grid(launch, xyz, group, n_groups, n_valid, origin, cell, dims):
    """The fixed-radius grid of csrc/radius_grid.h over the points with a group in 0 .. n_groups-1: cell keys, torch's stable sort, the
    nine runs per point -> (pts float32 [n_valid, 4] = x, y, z, original index as bits, in the grid's order; order int64 [N]: the sort's
    permutation, the n_valid points that take part first; sorted_group int32 [n_valid]; ranges int32 [18, n_valid])."""
    dev, n = xyz.device, xyz.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    launch("pointops2_dbscan_keys_launcher", n, n_groups, ptr(xyz), ptr(group), ctypes.c_double(origin[0]), ctypes.c_double(origin[1]),
           ctypes.c_double(origin[2]), ctypes.c_double(cell), dims[0], dims[1], dims[2], ptr(keys))
    skeys, order = torch.sort(keys, stable=True)
    pts = torch.empty(n_valid, 4, dtype=torch.float32, device=dev)
    sgroup = torch.empty(n_valid, dtype=torch.int32, device=dev)
    ranges = torch.empty(18, n_valid, dtype=torch.int32, device=dev)
    launch("pointops2_dbscan_prepare_launcher", n, n_valid, dims[0], dims[1], dims[2], ptr(xyz), ptr(skeys), ptr(order), ptr(pts), ptr(sgroup),
           ptr(ranges))
    return pts, order, sgroup, ranges


def dbscan(xyz, eps, min_samples, group=None):
    """DBSCAN of xyz [N, 3] fp32 (GPU) -> (labels int32 [N], core bool [N], n_clusters int32 [G]).

    group: int32 / int64 [N] with values in -1 .. G-1, None = one group.  Two points are neighbours only inside the same group, a point
    of group -1 is never a neighbour and keeps label -1; cluster numbers start at 0 in every group.  eps, min_samples: scalars, or
    sequences / tensors of length G looked up per group (G is their length; with scalars and a `group` G = group.max() + 1).
    Raises before any launch: RuntimeError for a CPU tensor, ValueError / TypeError for a wrong shape or dtype, ValueError for
    eps <= 0, min_samples < 1, a group outside -1 .. G-1 or non-finite coordinates.  RuntimeError when the component loop has not
    settled after MAX_ROUNDS rounds."""
    _check_tensors("dbscan", xyz, group, "group")
    n_groups, eps_h, ms_h = _settings(eps, min_samples, 1 if group is None else None)
    dev, n = xyz.device, xyz.shape[0]
    LAST["rounds"], LAST["launches"] = 0, 0
    if n == 0:
        g = n_groups if n_groups is not None else 1
        return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.bool, device=dev),
                torch.zeros(g, dtype=torch.int32, device=dev))
    xyz = xyz.contiguous()
    if group is None:
        group = torch.zeros(n, dtype=torch.int32, device=dev)
    group = group.to(torch.int32).contiguous()

    _, g_min, g_max, n_valid, origin, top = _scan("dbscan", xyz, group)
    if n_groups is None:
        n_groups = max(g_max + 1, 1)
    if g_min < -1 or g_max >= n_groups:
        raise ValueError(f"dbscan: group values must be in -1 .. {n_groups - 1}, got {g_min} .. {g_max}")
    eps_h = np.broadcast_to(eps_h, (n_groups,)).astype(np.float32)
    ms_h = np.broadcast_to(ms_h, (n_groups,)).astype(np.int32)

    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    core = torch.zeros(n, dtype=torch.uint8, device=dev)
    n_clusters = torch.zeros(n_groups, dtype=torch.int32, device=dev)
    if n_valid == 0:
        return labels, core.bool(), n_clusters

    cell = float(np.float32(eps_h.max())) * CELL_MARGIN
    dims = _dims("dbscan", n_groups, origin, top, cell)
    eps2 = torch.from_numpy(eps_h * eps_h).to(dev)          # fp32 product, rounded once
    ms = torch.from_numpy(ms_h).to(dev)

    call = functools.partial(_launch, LAST, dev)
    pts, _, sgroup, ranges = _grid(call, xyz, group, n_groups, n_valid, origin, cell, dims)
    score = torch.empty(n_valid, dtype=torch.uint8, device=dev)
    parent = torch.full((n,), -1, dtype=torch.int32, device=dev)
    call("pointops2_dbscan_core_launcher", n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(ms), ptr(score), ptr(core),
         ptr(parent))

    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for rounds in range(1, MAX_ROUNDS + 1):
        call("pointops2_dbscan_round_launcher", n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(score), ptr(parent),
             ptr(changed))
        LAST["launches"] += 1                                # (a round is two kernels)
        LAST["rounds"] = rounds
        if int(changed.item()) == 0:                         # the one small read-back per round
            break
    else:
        raise RuntimeError(f"dbscan: the component loop has not settled after {MAX_ROUNDS} rounds")

    # roots -> cluster numbers: per group, ascending root (= smallest core index).  nonzero yields the roots in ascending order and
    # the stable sort by group keeps it.
    roots = torch.nonzero(parent == torch.arange(n, dtype=torch.int32, device=dev)).flatten()
    cluster_of_root = torch.full((n,), -1, dtype=torch.int32, device=dev)
    if roots.numel() > 0:
        root_group = group[roots].long()
        sorted_group, by_group = torch.sort(root_group, stable=True)
        counts = torch.bincount(root_group, minlength=n_groups)
        n_clusters = counts.to(torch.int32)
        starts = torch.cumsum(counts, 0) - counts
        number = torch.arange(roots.numel(), device=dev) - starts[sorted_group]
        cluster_of_root[roots[by_group]] = number.to(torch.int32)
    call("pointops2_dbscan_label_launcher", n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(score), ptr(parent),
         ptr(cluster_of_root), ptr(labels))
    return labels, core.bool(), n_clusters


def _class_settings(value, n_classes, face, edge, dtype, name):
    if value is None:
        return np.asarray([face if c < FACE_CLASSES else edge for c in range(n_classes)], dtype=dtype)
    g, a = _per_group(value, n_classes, dtype, name)
    return np.full(n_classes, a, dtype=dtype) if g is None else a


def _length(value):
    """entries of a per-class setting, None for a scalar or a default"""
    if value is None:
        return None
    shape = tuple(value.shape) if hasattr(value, "shape") else np.shape(value)
    return shape[0] if len(shape) == 1 else None


def instances(coord, shift, pred, eps=None, min_samples=None, min_points=None):
    """The clustering of `instantiation_eval` (util/train_utils.py:549-566) on the device: DBSCAN of coord + shift per predicted class,
    the clusters with MORE than min_points[class] points kept, numbered class-major, then by cluster number, dropped clusters skipped.

    coord, shift [N, 3] fp32 and pred int32 / int64 [N] (classes 0 .. C-1; -1 = in no class) on the GPU.  eps, min_samples, min_points:
    scalars or per-class sequences of one length C > max(pred); None = the reference's settings: classes below 6 eps 0.1,
    min_samples 5, min_points 50, the others 0.15, 3, 20.
    -> (instance int32 [N]: the instance of every point or -1, instance_class int32 [I], instance_size int32 [I])."""
    _check_tensors("dbscan", coord, pred, "group")
    _gpu(shift, "dbscan", "shift")
    if shift.shape != coord.shape or shift.dtype != torch.float32:
        raise ValueError(f"dbscan: shift must be float32 {tuple(coord.shape)}, got {shift.dtype} {tuple(shift.shape)}")
    if shift.device != coord.device:
        raise RuntimeError(f"dbscan: shift is on {shift.device}, coord on {coord.device}")
    dev, n = coord.device, coord.shape[0]
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    lengths = {l for l in map(_length, (eps, min_samples, min_points)) if l is not None}
    if len(lengths) > 1:
        raise ValueError(f"dbscan: eps, min_samples and min_points must agree on the number of classes, got {sorted(lengths)}")
    n_classes = lengths.pop() if lengths else (max(int(pred.max().item()) + 1, 1) if n > 0 else 1)
    eps_h = _class_settings(eps, n_classes, FACE_SETTINGS[0], EDGE_SETTINGS[0], np.float32, "eps")
    ms_h = _class_settings(min_samples, n_classes, FACE_SETTINGS[1], EDGE_SETTINGS[1], np.int32, "min_samples")
    mp_h = _class_settings(min_points, n_classes, FACE_SETTINGS[2], EDGE_SETTINGS[2], np.int32, "min_points")
    _settings(eps_h, ms_h, n_classes)
    if n == 0:
        return empty, empty.clone(), empty.clone()
    labels, _, n_clusters = dbscan(coord + shift, eps_h, ms_h, pred)
    total = int(n_clusters.sum().item())
    if total == 0:
        return torch.full((n,), -1, dtype=torch.int32, device=dev), empty, empty.clone()
    counts = n_clusters.long()
    starts = torch.cumsum(counts, 0) - counts                                   # first flat cluster id of every class
    cluster_class = torch.repeat_interleave(torch.arange(n_classes, device=dev), counts, output_size=total)
    in_cluster = labels >= 0
    flat = torch.where(in_cluster, starts[pred.long().clamp(min=0)] + labels.long(), torch.zeros_like(labels, dtype=torch.int64))
    size = torch.bincount(flat[in_cluster], minlength=total)
    keep = size > torch.from_numpy(mp_h).to(dev).long()[cluster_class]
    number = torch.cumsum(keep.long(), 0) - 1
    number = torch.where(keep, number, torch.full_like(number, -1))
    instance = torch.where(in_cluster, number[flat], torch.full_like(flat, -1)).to(torch.int32)
    return instance, cluster_class[keep].to(torch.int32), size[keep].to(torch.int32)


# ---- contacts between labelled point sets, and the grouping of face instances into objects built on them (csrc/contacts.hip) ----
# instantiation_eval's settings (util/train_utils.py:600, :629-631): the two face classes beside edge class 6 + c
EDGE_FACES = ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (0, 4), (2, 4), (3, 4), (1, 5), (2, 5), (3, 5), (4, 5))
CONTACT_RADIUS = 0.08
CONTACT_SHARE = 0.5
LAST_CONTACTS = {"launches": 0, "readbacks": 0}   # of the most recent contacts() / objects() call (tools/bench_contacts.py)


def _contacts(xyz, label, radius, n_labels, want_min, who):
    """-> (count int32 [I, I], min_d2 float32 [I, I] or None, I)"""
    _check_tensors(who, xyz, label, "label")
    r, r2 = _radius(who, radius)
    n_labels = _label_count(who, n_labels)
    dev, n = xyz.device, xyz.shape[0]
    LAST_CONTACTS["launches"], LAST_CONTACTS["readbacks"] = 0, 0

    def tables(i):
        return (torch.zeros(i, i, dtype=torch.int32, device=dev),
                torch.full((i, i), float("inf"), dtype=torch.float32, device=dev) if want_min else None, i)

    if n == 0:
        return tables(n_labels or 0)
    xyz = xyz.contiguous()
    label = label.to(torch.int32).contiguous()

    LAST_CONTACTS["readbacks"] += 1
    member, l_min, l_max, n_valid, origin, top = _scan(who, xyz, label)
    n_labels = _label_range(who, n_labels, l_min, l_max)
    words = _row_words(who, n_valid, n_labels)
    if n_valid == 0 or n_labels == 0:
        return tables(n_labels)
    cell = float(r) * CELL_MARGIN
    dims = _dims(who, 1, origin, top, cell)
    count, min_d2, _ = tables(n_labels)
    call = functools.partial(_launch, LAST_CONTACTS, dev)
    group = member.to(torch.int32) - 1                       # one group: 0 for a labelled point, -1 for the others
    pts, order, _, ranges = _grid(call, xyz, group, 1, n_valid, origin, cell, dims)
    slabel = label[order[:n_valid]].contiguous()
    bitmap = torch.zeros(n_valid, words, dtype=torch.int32, device=dev) if n_labels > REG_LABELS else None
    call("pointops2_contacts_count_launcher", n_valid, n_labels, ptr(pts), ptr(slabel), ptr(ranges), ctypes.c_float(r2), ptr(bitmap), ptr(count))
    if want_min:
        llabel, by_label = torch.sort(slabel, stable=True)   # ascending label; inside a label the grid's order, which keeps tiles compact
        label_pts = torch.cat([pts[by_label, :3], llabel.view(torch.float32)[:, None]], 1).contiguous()
        call("pointops2_contacts_min_launcher", n_valid, n_labels, ptr(label_pts), ptr(min_d2))
    return count, min_d2, n_labels


def contacts(xyz, label, radius, n_labels=None):
    """Which labelled point sets touch, and how close they come: xyz [N, 3] fp32 and label int32 / int64 [N] in -1 .. I-1 (GPU; -1 = the
    point takes no part) -> (count int32 [I, I], min_d2 float32 [I, I]) with I = n_labels, or label.max() + 1.

    count[a, b]: the points p of label a for which SOME point q of label b has d2(p, q) < radius^2 - strict, as the reference's
    `dist < 0.08` (util/train_utils.py:629); p counts once per b however many q are near, and is its own partner, so count[a, a] is the
    size of a.  count is not symmetric.  min_d2[a, b]: the minimum of d2(p, q) over p in a and q in b (symmetric), +inf where either
    label is empty.  d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32, dx = xp - xq, compared with fp32(radius) * fp32(radius) rounded once.
    count comes from a fixed-radius grid walk, min_d2 from a sweep over all pairs: quadratic in the labelled points (csrc/contacts.hip).

    Raises before any launch: RuntimeError for a CPU tensor or mismatched devices; TypeError / ValueError for a wrong dtype or shape,
    radius <= 0 or non-finite, a label outside -1 .. I-1 or non-finite coordinates; ValueError when the rows of labels in reach
    (n_valid * ceil(I / 32) * 4 bytes, needed above 64 labels) would exceed MAX_BITMAP_BYTES = 1 GiB, when I > MAX_LABELS, or when the grid
    exceeds MAX_CELLS_PER_AXIS.  N = 0 or no labelled point: the tables of zeros / +inf, nothing launched."""
    count, min_d2, _ = _contacts(xyz, label, radius, n_labels, True, "contacts")
    return count, min_d2


def link_objects(count, size, instance_class, share=CONTACT_SHARE, face_classes=FACE_CLASSES, edge_faces=None):
    """The pairing and merging of `instantiation_eval` (util/train_utils.py:595-714) on plain arrays - no GPU: count [I, I] (contacts),
    size [I], instance_class [I] (ascending, as instances() numbers them) -> (object_of_instance int32 [I], n_objects).

      1. only the edge classes face_classes + c, c < len(edge_faces), take part; instances of higher classes are ignored;
      2. an edge class is skipped entirely when either of its two face classes has no instance (:606-607);
      3. an edge instance e links, for each of its two face classes in turn, the FIRST face instance k of that class in ascending
         instance number with count[e, k] / size[e] > share (:627-639).  share = 0.5 is decided in integers, 2 * count > size (what the
         Python float comparison decides for integers below 2^52); another share as count > share * size in float64;
      4. objects = the connected components over the linked face instances, two faces joined when one edge linked both; a face no edge
         linked is in no object, an edge that linked a single face makes it an object of its own;
      5. objects are numbered by ascending smallest face instance number; an edge instance gets the object of its first linked face."""
    count = np.asarray(count)
    size = np.asarray(size).astype(np.int64).reshape(-1)
    cls = np.asarray(instance_class).astype(np.int64).reshape(-1)
    n_inst = cls.shape[0]
    if count.shape != (n_inst, n_inst) or size.shape != (n_inst,):
        raise ValueError(f"objects: count must be [I, I] and size [I] for the {n_inst} instances, got {count.shape} and {size.shape}")
    if isinstance(share, bool) or not isinstance(share, (int, float, np.integer, np.floating)) or not np.isfinite(share) or share < 0:
        raise ValueError(f"objects: share must be a finite number >= 0, got {share!r}")
    edge_faces = EDGE_FACES if edge_faces is None else tuple(tuple(int(f) for f in pair) for pair in edge_faces)
    face_classes = int(face_classes)
    if any(len(pair) != 2 or not all(0 <= f < face_classes for f in pair) for pair in edge_faces):
        raise ValueError(f"objects: edge_faces must hold pairs of face classes below {face_classes}")
    count = count.astype(np.int64)
    of_class = [np.nonzero(cls == c)[0] for c in range(face_classes)]             # ascending instance numbers
    parent = np.arange(n_inst)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    linked = np.zeros(n_inst, dtype=bool)
    first_face = np.full(n_inst, -1, dtype=np.int64)
    for c, (f1, f2) in enumerate(edge_faces):
        if len(of_class[f1]) == 0 or len(of_class[f2]) == 0:                      # rule 2
            continue
        for e in np.nonzero(cls == face_classes + c)[0].tolist():
            paired = []
            for faces in (of_class[f1], of_class[f2]):
                near = 2 * count[e, faces] > size[e] if share == 0.5 else count[e, faces].astype(np.float64) > np.float64(share) * np.float64(size[e])
                hit = np.nonzero(near)[0]
                if len(hit):
                    paired.append(int(faces[hit[0]]))                             # the first match (break at :633, :639)
            if not paired:
                continue
            first_face[e] = paired[0]
            linked[paired] = True
            a, b = find(paired[0]), find(paired[-1])
            if a != b:
                parent[max(a, b)] = min(a, b)                                     # the root is the smallest face of its component
    object_of = np.full(n_inst, -1, dtype=np.int32)
    faces = np.nonzero(linked)[0]
    roots = np.array([find(i) for i in faces.tolist()], dtype=np.int64)
    numbered = np.unique(roots)                                                   # ascending smallest face instance
    object_of[faces] = np.searchsorted(numbered, roots)
    edges = np.nonzero(first_face >= 0)[0]
    object_of[edges] = object_of[first_face[edges]]
    return object_of, int(len(numbered))


def objects(coord, instance, instance_class, instance_size=None, radius=CONTACT_RADIUS, share=CONTACT_SHARE, face_classes=FACE_CLASSES,
            edge_faces=None):
    """The grouping of `instantiation_eval` (util/train_utils.py:595-714) on the output of instances(): which face instances form one
    object ("box support").  coord [N, 3] fp32: the ORIGINAL coordinates (the reference pairs on pts_ori, not on the shifted points);
    instance int32 / int64 [N] and instance_class [I] as instances() returns them; instance_size [I] defaults to a bincount of instance.
    -> (object int32 [N]: the object of the point's FACE instance or -1 - the reference's supports hold face points only,
        object_of_instance int32 [I]: for an edge instance the object of its first linked face, -1 = in no object, n_objects int).

    An edge instance links, per face class beside its edge class (edge_faces, default the reference's lookup_face: edge class
    face_classes + c -> two face classes, c < 12), the first face instance with more than `share` of the edge's points within `radius`
    of it; objects are the connected components over the linked faces, numbered by ascending smallest face instance (rules 1-5 of
    link_objects, which does this part on the host from ONE read-back of the contact counts; count comes from contacts' grid walk, the
    quadratic min_d2 sweep is not run).  Two deliberate departures from the reference: with no link at all it raises IndexError
    (pair_list[0], :670) - here the result is zero objects; its merge loop runs len + 100 iterations (:666) and equals the components
    only when that reaches its fixed point - here the result is always the components.  The reference's list order (an artefact of the
    rotating merge loop) is not reproduced; the Open3D clean-up of every support (:716-720) is clean_supports, on this function's
    output; the OBB merging of test.py:294-326 is the step behind that, merge_objects.
    Raises as contacts() does; ValueError for an instance_class / instance_size that is not [I]."""
    _check_tensors("objects", coord, instance, "label")
    dev = coord.device
    if not isinstance(instance_class, torch.Tensor) or instance_class.dim() != 1 or instance_class.dtype not in (torch.int32, torch.int64):
        raise ValueError("objects: instance_class must be an int32 / int64 tensor [I]")
    n_inst = instance_class.shape[0]
    if instance_size is not None and (not isinstance(instance_size, torch.Tensor) or tuple(instance_size.shape) != (n_inst,)
                                      or instance_size.dtype not in (torch.int32, torch.int64)):
        raise ValueError(f"objects: instance_size must be an int32 / int64 tensor [{n_inst}]")
    link_objects(np.zeros((0, 0), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), share, face_classes, edge_faces)  # the settings
    count, _, _ = _contacts(coord, instance, radius, n_inst, False, "objects")
    n = coord.shape[0]
    if instance_size is None:
        instance_size = torch.bincount(instance[instance >= 0].long(), minlength=n_inst) if n > 0 else torch.zeros(n_inst, dtype=torch.int64)
    head = torch.cat([count.flatten().long(), instance_size.to(dev).long(), instance_class.to(dev).long()]).cpu().numpy()   # the one read-back
    LAST_CONTACTS["readbacks"] += 1
    object_of, n_objects = link_objects(head[:n_inst * n_inst].reshape(n_inst, n_inst), head[n_inst * n_inst:n_inst * n_inst + n_inst],
                                        head[n_inst * n_inst + n_inst:], share, face_classes, edge_faces)
    face_object = np.where(head[n_inst * n_inst + n_inst:] < int(face_classes), object_of, -1).astype(np.int32)
    table = torch.from_numpy(np.concatenate([face_object, np.full(1, -1, np.int32)])).to(dev)                # (the last entry serves -1)
    obj = table[instance.long()] if n > 0 else torch.empty(0, dtype=torch.int32, device=dev)
    return obj, torch.from_numpy(object_of).to(dev), n_objects


# ---- the OBB merging behind the grouping (test.py:294-326, the same loop at test_iou.py:373-406) and the box detection score that
# test_iou.py:409-466 takes from the merged sets, on csrc/boxes.hip ----
MERGE_RADIUS = 0.2          # test.py:310 pc_thre
MERGE_OVERLAP = 0.3         # util/train_utils.py:861 thre
MERGE_MIN_NEIGHBORS = 10    # test.py:312
LAST_MERGE = {"launches": 0, "readbacks": 0}   # of the most recent label_boxes() / merge_objects() call (tools/bench_merge.py)


def _boxes(xyz, label, n_labels, dev, counter=LAST_MERGE):
    """the launch of label_boxes on checked, contiguous inputs, counted in `counter` -> (lo, hi, size)"""
    lo = torch.full((n_labels, 3), float("inf"), dtype=torch.float32, device=dev)
    hi = torch.full((n_labels, 3), float("-inf"), dtype=torch.float32, device=dev)
    size = torch.zeros(n_labels, dtype=torch.int32, device=dev)
    if xyz.shape[0] > 0 and n_labels > 0:
        _launch(counter, dev, "pointops2_label_boxes_launcher", xyz.shape[0], n_labels, ptr(xyz), ptr(label), ptr(lo), ptr(hi), ptr(size))
    return lo, hi, size


def label_boxes(xyz, label, n_labels=None):
    """The axis-aligned box and the size of every labelled point set: xyz [N, 3] fp32 and label int32 / int64 [N] in -1 .. I-1 (GPU; -1 =
    the point takes no part) -> (lo float32 [I, 3], hi float32 [I, 3], size int32 [I]) with I = n_labels, or label.max() + 1.

    lo / hi: the componentwise minimum / maximum of the label's points, exact (integer atomics on an order-preserving image of the fp32
    values, csrc/boxes.hip); -0.0 counts as +0.0, so compare by value.  A label without a point keeps +inf / -inf / 0.
    Raises before any launch: RuntimeError for a CPU tensor or mismatched devices; TypeError / ValueError for a wrong dtype or shape, a
    label outside -1 .. I-1, non-finite coordinates or I > MAX_LABELS.  N = 0 or I = 0 launches nothing."""
    _check_tensors("label_boxes", xyz, label, "label")
    n_labels = _label_count("label_boxes", n_labels)
    dev, n = xyz.device, xyz.shape[0]
    LAST_MERGE["launches"], LAST_MERGE["readbacks"] = 0, 0
    if n == 0:
        return _boxes(xyz, label, n_labels or 0, dev)
    xyz = xyz.contiguous()
    label = label.to(torch.int32).contiguous()
    head = torch.cat([label.min()[None].long(), label.max()[None].long(), torch.isfinite(xyz).all()[None].long()]).cpu().numpy()
    LAST_MERGE["readbacks"] += 1
    l_min, l_max, all_finite = int(head[0]), int(head[1]), bool(head[2])
    n_labels = _label_range("label_boxes", n_labels, l_min, l_max)
    if not all_finite:
        raise ValueError("label_boxes: xyz must be finite")
    return _boxes(xyz, label, n_labels, dev)


def _overlaps(lo_a, hi_a, lo_b, hi_b, overlap):
    """compute_partial_iou (util/train_utils.py:840-862) on the boxes that trimesh's PointCloud.bounding_box gives for the two point sets
    (centre = (lo + hi) / 2, extents = hi - lo), in float64, operation for operation -> (a is covered, b is covered).  The boxes are
    sequences of three Python floats - IEEE doubles, the arithmetic of the reference's numpy arrays without their per-call cost."""
    edges, extent_a, extent_b = [], [], []
    for k in range(3):
        centre_a, e_a = (lo_a[k] + hi_a[k]) / 2, hi_a[k] - lo_a[k]
        centre_b, e_b = (lo_b[k] + hi_b[k]) / 2, hi_b[k] - lo_b[k]
        top = min(centre_a + e_a / 2, centre_b + e_b / 2)
        bottom = max(centre_a - e_a / 2, centre_b - e_b / 2)
        if not top > bottom:                                                       # strict: boxes that only touch, and flat boxes, never overlap
            return False, False
        edges.append(top - bottom)
        extent_a.append(e_a)
        extent_b.append(e_b)
    inter = edges[0] * edges[1] * edges[2]
    return inter / (extent_a[0] * extent_a[1] * extent_a[2]) > overlap, inter / (extent_b[0] * extent_b[1] * extent_b[2]) > overlap


def merge_sets(lo, hi, size, pat_object, pat_rows, pat_count, overlap=MERGE_OVERLAP, min_neighbors=MERGE_MIN_NEIGHBORS):
    """The rotating merge loop of test.py:294-326 on plain arrays - no GPU: lo / hi [O, 3] and size [O] (label_boxes), and the pattern
    table of the border points: pat_object [P], pat_rows [P, ceil(O / 32)] (bit b: an object-b point within the radius, own bit cleared),
    pat_count [P] = points of that (object, row) -> (set_of_object int32 [O], members: the final list, a list of lists of objects).

    The loop as the reference runs it: the list starts with the objects of non-zero size in ascending object number and end_cnt is its
    length; every round pops the first set, compares it with every remaining set - always against the set as it was popped - and
    appends the popped set with everything it merged LAST.  The loop's sets are unions of whole objects, so
      - a set's box is the minimum / maximum of its members' lo / hi (float64; exact from fp32), and its overlap test is
        compute_partial_iou (util/train_utils.py:840-862) in float64, operation for operation: either ratio > overlap, and none when
        the boxes do not intersect strictly on every axis;
      - num_neighbor = np.sum(np.min(cdist(cur, targ), axis=0) < 0.2) is the number of border points whose object is in the target set
        and whose row meets the current set - a point that reaches two members of the current set counts once;
    and target merges when its box overlaps and num_neighbor > min_neighbors.  Sets are numbered in the order of the loop's final list,
    the row order of the reference's pred_box (test_iou.py:409-423); an object of size 0 is in set -1.  With fewer than two objects the
    reference returns before the loop (test.py:277); here nothing merges and every object is its own set."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    size = np.asarray(size).astype(np.int64).reshape(-1)
    n_obj = size.shape[0]
    words = (n_obj + 31) // 32
    pat_object = np.asarray(pat_object).astype(np.int64).reshape(-1)
    pat_count = np.asarray(pat_count).astype(np.int64).reshape(-1)
    pat_rows = np.asarray(pat_rows)
    if lo.shape != (n_obj, 3) or hi.shape != (n_obj, 3):
        raise ValueError(f"merge_sets: lo and hi must be [O, 3] for the {n_obj} objects, got {lo.shape} and {hi.shape}")
    n_pat = pat_object.shape[0]
    if pat_rows.dtype.kind not in "iu":
        raise TypeError(f"merge_sets: pat_rows must hold 32-bit words, got {pat_rows.dtype}")
    pat_rows = pat_rows.astype(np.int64).astype(np.uint32).reshape(n_pat, -1) if n_pat else np.zeros((0, words), np.uint32)
    if pat_rows.shape != (n_pat, words) or pat_count.shape != (n_pat,):
        raise ValueError(f"merge_sets: pat_rows must be [P, {words}] and pat_count [P] for the {n_pat} patterns, got {pat_rows.shape} and {pat_count.shape}")
    if n_pat and (pat_object.min() < 0 or pat_object.max() >= n_obj):
        raise ValueError(f"merge_sets: pat_object must be in 0 .. {n_obj - 1}")
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float, np.integer, np.floating)) or not np.isfinite(overlap) or overlap < 0:
        raise ValueError(f"merge_sets: overlap must be a finite number >= 0, got {overlap!r}")
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, (int, np.integer)) or min_neighbors < 0:
        raise ValueError(f"merge_sets: min_neighbors must be an int >= 0, got {min_neighbors!r}")

    lo_l, hi_l = lo.tolist(), hi.tolist()                                           # Python floats: exact copies of the float64 values

    def box_of(members):
        return ([min(lo_l[o][k] for o in members) for k in range(3)], [max(hi_l[o][k] for o in members) for k in range(3)])

    sets = [[int(o)] for o in np.nonzero(size > 0)[0]]
    box = [box_of(s) for s in sets]
    rounds = len(sets) if len(sets) >= 2 else 0
    for _ in range(rounds):
        cur, (cur_lo, cur_hi) = sets.pop(0), box.pop(0)
        mask = np.zeros(words, dtype=np.uint32)
        for o in cur:
            mask[o >> 5] |= np.uint32(1 << (o & 31))
        reaches_cur = (pat_rows & mask).any(1)                                      # the patterns that meet the current set, each once
        near_of = np.bincount(pat_object[reaches_cur], weights=pat_count[reaches_cur], minlength=n_obj).astype(np.int64).tolist()   # exact below 2^53
        merged, remain, remain_box = list(cur), [], []
        for targ, (targ_lo, targ_hi) in zip(sets, box):
            over_a, over_b = _overlaps(cur_lo, cur_hi, targ_lo, targ_hi, overlap)
            if (over_a or over_b) and sum(near_of[o] for o in targ) > min_neighbors:
                merged += targ
            else:
                remain.append(targ)
                remain_box.append((targ_lo, targ_hi))
        sets, box = remain + [merged], remain_box + [box_of(merged)]
    set_of = np.full(n_obj, -1, dtype=np.int32)
    for number, members in enumerate(sets):
        set_of[members] = number
    return set_of, sets


def merge_objects(coord, obj, n_objects=None, radius=MERGE_RADIUS, overlap=MERGE_OVERLAP, min_neighbors=MERGE_MIN_NEIGHBORS):
    """The OBB merging of test.py:294-326 (the same loop at test_iou.py:373-406) on the output of objects(): which objects the rotating
    loop merges into one box.  coord [N, 3] fp32 and obj int32 / int64 [N] in -1 .. O-1 (GPU; -1 = in no object), O = n_objects or
    obj.max() + 1 -> (merged int32 [N]: the set of the point's object or -1, set_of_object int32 [O] (-1 for an object without a point),
    boxes float32 [S, 6] = lo | hi of every set, the reference's pred_box rows (test_iou.py:422), n_sets int).

    The reference builds two trimesh boxes and one dense cdist per pair of sets in every rotation.  Here the device computes, once: the
    box and size of every object (label_boxes), the row of objects within `radius` of every point (csrc/boxes.hip on the grid of
    csrc/radius_grid.h; strict <, as `< pc_thre`), and - with torch - the table of distinct (object, row) patterns of the border points with
    their counts.  ONE read-back of boxes, sizes and patterns later merge_sets runs the whole loop on the host; two read-backs in all
    (LAST_MERGE), whatever the number of objects.  Distances are evaluated in fp32 as ((dx*dx) + (dy*dy)) + (dz*dz) < fp32(radius)^2
    (the reference: float64 cdist), so a pair within about 1e-6 of the radius may fall on the other side.  Not reproduced: the Open3D
    clean-up that the reference has commented out around the boxes, the .obj exports, and trimesh itself - PointCloud.bounding_box is
    taken as the box of the bounds (min / max per axis), its published behaviour, which no fixture here pins.
    Raises as contacts() does, before any launch.  N = 0 or no point in an object: no set, nothing launched."""
    who = "merge_objects"
    _check_tensors(who, coord, obj, "label")
    r, r2 = _radius(who, radius)
    n_objects = _label_count(who, n_objects, "n_objects")
    merge_sets(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), np.zeros((0, 0), np.int32), np.zeros(0), overlap, min_neighbors)  # the settings
    dev, n = coord.device, coord.shape[0]
    LAST_MERGE["launches"], LAST_MERGE["readbacks"] = 0, 0

    def nothing(o):
        return (torch.full((n,), -1, dtype=torch.int32, device=dev), torch.full((o,), -1, dtype=torch.int32, device=dev),
                torch.zeros(0, 6, dtype=torch.float32, device=dev), 0)

    if n == 0:
        return nothing(n_objects or 0)
    coord = coord.contiguous()
    label = obj.to(torch.int32).contiguous()

    LAST_MERGE["readbacks"] += 1
    member, l_min, l_max, n_valid, origin, top = _scan(who, coord, label)
    n_objects = _label_range(who, n_objects, l_min, l_max, "n_objects")
    words = _row_words(who, n_valid, n_objects)
    if n_valid == 0 or n_objects == 0:
        return nothing(n_objects)
    cell = float(r) * CELL_MARGIN
    dims = _dims(who, 1, origin, top, cell)

    lo, hi, size = _boxes(coord, label, n_objects, dev)
    slabel, rows = _reach_rows(coord, label, member, n, n_valid, n_objects, origin, cell, dims, r2, dev)
    pat, pat_count = _patterns(slabel, rows)

    # the one final read-back: boxes, sizes and patterns as one array of 32-bit words
    n_pat = pat.shape[0]
    flat = torch.cat([lo.view(torch.int32).flatten(), hi.view(torch.int32).flatten(), size, pat.flatten(), pat_count.to(torch.int32)]).cpu().numpy()
    LAST_MERGE["readbacks"] += 1
    at = np.cumsum([0, 3 * n_objects, 3 * n_objects, n_objects, n_pat * (1 + words), n_pat])
    lo_h, hi_h = (flat[at[k]:at[k + 1]].view(np.float32).reshape(n_objects, 3) for k in (0, 1))
    pat_h = flat[at[3]:at[4]].reshape(n_pat, 1 + words)
    set_of, sets = merge_sets(lo_h, hi_h, flat[at[2]:at[3]], pat_h[:, 0], pat_h[:, 1:], flat[at[4]:at[5]], overlap, min_neighbors)
    boxes = np.array([np.concatenate([lo_h[s].min(0), hi_h[s].max(0)]) for s in sets], dtype=np.float32).reshape(len(sets), 6)
    table = torch.from_numpy(np.concatenate([set_of, np.full(1, -1, np.int32)])).to(dev)                     # (the last entry serves -1)
    return table[label.long()], table[:n_objects], torch.from_numpy(boxes).to(dev), len(sets)


def _reach_rows(coord, label, member, n, n_valid, n_objects, origin, cell, dims, r2, dev):
    """the grid over the labelled points and the reach rows on it -> (sorted_label int32 [n_valid], rows int32 [n_valid, words]: the objects
    within reach of every point, its own left out), both in the grid's order"""
    call = functools.partial(_launch, LAST_MERGE, dev)
    group = member.to(torch.int32) - 1                       # one group: 0 for a point in an object, -1 for the others
    pts, order, _, ranges = _grid(call, coord, group, 1, n_valid, origin, cell, dims)
    slabel = label[order[:n_valid]].contiguous()
    rows = torch.zeros(n_valid, (n_objects + 31) // 32, dtype=torch.int32, device=dev)
    call("pointops2_reach_rows_launcher", n_valid, n_objects, ptr(pts), ptr(slabel), ptr(ranges), ctypes.c_float(r2), ptr(rows))
    return slabel, rows


def _patterns(slabel, rows):
    """the distinct (object, row) patterns of the border points - the points whose row is not empty - and how many points show each
    -> (pat int32 [P, 1 + words], count int64 [P]); on the device"""
    border = (rows != 0).any(1)
    keyed = torch.cat([slabel[border, None], rows[border]], 1)
    if keyed.shape[0] == 0:
        return keyed, torch.zeros(0, dtype=torch.int64, device=rows.device)
    return torch.unique(keyed, dim=0, return_counts=True)


def box_detection(pred_box, gt_box, overlap_threshold=0.5):
    """The box detection score that test_iou.py:455-464 takes from the merged boxes, on host arrays - no GPU: pred_box [P, 6] and gt_box
    [G, 6] as x1 y1 z1 x2 y2 z2 -> (tp_iou: the IoU of every matched prediction, fp: -1.0 per unmatched prediction, fn int: ground-truth
    boxes left over, precision = TP / (TP + FP), recall = TP / (TP + FN)).

    Follows util/evaluation.py in float64: DetectionMAP.intersect_area / jaccard (:109-152) - including the upper clip bound, which is the
    LARGEST difference of the whole [P, G, 3] array: when no pair of boxes intersects on any axis that bound is negative and every
    "intersection" becomes its cube, a negative volume, hence a negative IoU -; IoU < overlap_threshold -> 0 (:86); compute_TP_FP_FN
    (:194-239): predictions in their given order, each takes the ground-truth box of largest remaining IoU, a ground-truth box is used
    once; the two ratios of :95-96.  Two departures: with no prediction the reference's jaccard returns an array shaped [0, 6] and
    reports FN = 6 - here FN is the number of ground-truth boxes; and a zero denominator gives None instead of ZeroDivisionError."""
    pred = np.asarray(pred_box.detach().cpu().numpy() if isinstance(pred_box, torch.Tensor) else pred_box, dtype=np.float64)
    gt = np.asarray(gt_box.detach().cpu().numpy() if isinstance(gt_box, torch.Tensor) else gt_box, dtype=np.float64)
    pred, gt = pred.reshape(-1, 6) if pred.size == 0 else pred, gt.reshape(-1, 6) if gt.size == 0 else gt
    if pred.ndim != 2 or pred.shape[1] != 6 or gt.ndim != 2 or gt.shape[1] != 6:
        raise ValueError(f"box_detection: pred_box and gt_box must be [P, 6] and [G, 6], got {pred.shape} and {gt.shape}")
    if isinstance(overlap_threshold, bool) or not isinstance(overlap_threshold, (int, float, np.integer, np.floating)) or not np.isfinite(overlap_threshold):
        raise ValueError(f"box_detection: overlap_threshold must be a finite number, got {overlap_threshold!r}")
    n_pred, n_gt = pred.shape[0], gt.shape[0]
    iou = np.zeros((n_pred, n_gt))
    if n_pred and n_gt:
        diff = np.minimum(pred[:, None, 3:], gt[None, :, 3:]) - np.maximum(pred[:, None, :3], gt[None, :, :3])
        with np.errstate(all="ignore"):
            edge = np.clip(diff, a_min=0, a_max=np.max(diff))
            inter = edge[:, :, 0] * edge[:, :, 1] * edge[:, :, 2]
            vol_p = (pred[:, 3] - pred[:, 0]) * (pred[:, 4] - pred[:, 1]) * (pred[:, 5] - pred[:, 2])
            vol_g = (gt[:, 3] - gt[:, 0]) * (gt[:, 4] - gt[:, 1]) * (gt[:, 5] - gt[:, 2])
            iou = inter / (vol_p[:, None] + vol_g[None, :] - inter)
        iou[iou < overlap_threshold] = 0
    free = iou != 0
    tp, fp, fn = [], [], n_gt
    for i in range(n_pred):
        best, best_iou = -1, -1
        for j in range(n_gt):
            if free[i, j] and iou[i, j] > best_iou:
                best, best_iou = j, iou[i, j]
        if best != -1:
            tp.append(float(best_iou))
            free[:, best] = False
            fn -= 1
        else:
            fp.append(float(best_iou))
    precision = len(tp) / (len(tp) + len(fp)) if tp or fp else None
    recall = len(tp) / (len(tp) + fn) if len(tp) + fn else None
    return tp, fp, fn, precision, recall


# ---- the clean-up of every support behind the grouping (util/train_utils.py:716-723), on csrc/supports.hip ----
SUPPORT_VOXEL = 0.04        # util/train_utils.py:717 voxel_down_sample(voxel_size=0.04)
SUPPORT_RADIUS = 0.1        # util/train_utils.py:718 remove_radius_outlier(nb_points=3, radius=0.1)
SUPPORT_NB_POINTS = 3
LAST_SUPPORTS = {"launches": 0, "readbacks": 0}   # of the most recent clean_supports() / box_supports() call (tools/bench_supports.py)


def _support_settings(who, voxel, radius, nb_points):
    """-> (voxel as a float, fp32(radius), its fp32 square, nb_points as an int), validated"""
    r, r2 = _radius(who, radius)
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: voxel must be a number, got {type(voxel).__name__}")
    if not np.isfinite(voxel) or not voxel > 0:
        raise ValueError(f"{who}: voxel must be finite and > 0, got {voxel}")
    if isinstance(nb_points, bool) or not isinstance(nb_points, (int, np.integer)) or nb_points < 0 or nb_points >= 2 ** 31:
        raise ValueError(f"{who}: nb_points must be an int >= 0, got {nb_points!r}")
    return float(voxel), r, r2, int(nb_points)


def _voxel_dims(who, n_objects, origin, top, voxel):
    """-> the voxels per axis [nx, ny, nz] that no object of the scene exceeds: an object's voxel origin lies half a voxel below its own
    minimum, so its points reach at most floor(extent / voxel + 0.5) <= floor(scene extent / voxel) + 1; ValueError when the keys of
    n_objects such blocks do not fit 64 bits"""
    with np.errstate(all="ignore"):
        extent = np.floor((np.asarray(top, np.float64) - np.asarray(origin, np.float64)) / voxel)
    if not np.all(extent < MAX_CELLS_PER_AXIS):
        raise ValueError(f"{who}: the cloud spans {extent.tolist()} voxels of edge {voxel:g}: too many for the 64-bit voxel keys")
    dims = [int(e) + 2 for e in extent]
    if max(dims) > MAX_CELLS_PER_AXIS or n_objects * dims[0] * dims[1] * dims[2] >= 2 ** 61:
        raise ValueError(f"{who}: {n_objects} objects in a cloud of {dims} voxels of edge {voxel:g}: too many for the 64-bit voxel keys")
    return dims


def _voxel_means(call, coord, label, n_objects, n_valid, lo, voxel, dims):
    """voxel keys from every object's own minimum `lo` (device), torch's stable sort, the head flags and their scan
    -> (sorted_keys int64 [N], order int64 [N], slot int64 [n_valid], n_voxels: a 0-d device tensor - the caller reads it back)"""
    n = coord.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=coord.device)
    call("pointops2_supports_keys_launcher", n, n_objects, ptr(coord), ptr(label), ptr(lo), ctypes.c_double(voxel), dims[0], dims[1], dims[2],
         ptr(keys))
    skeys, order = torch.sort(keys, stable=True)
    head = torch.ones(n_valid, dtype=torch.int64, device=coord.device)
    head[1:] = skeys[1:n_valid] != skeys[:n_valid - 1]
    slot = torch.cumsum(head, 0) - 1                         # the exclusive count of heads, at a head
    return skeys, order, slot, slot[-1] + 1


def _means(call, coord, label, n_valid, n_voxels, skeys, order, slot):
    """-> (mean float32 [V, 3], mean_object int32 [V], mean_size int32 [V]) in the order of the keys: object, then vz, vy, vx"""
    dev = coord.device
    mean = torch.empty(n_voxels, 3, dtype=torch.float32, device=dev)
    mean_object = torch.empty(n_voxels, dtype=torch.int32, device=dev)
    mean_size = torch.empty(n_voxels, dtype=torch.int32, device=dev)
    call("pointops2_supports_means_launcher", coord.shape[0], n_valid, n_voxels, ptr(coord), ptr(label), ptr(skeys), ptr(order), ptr(slot),
         ptr(mean), ptr(mean_object), ptr(mean_size))
    return mean, mean_object, mean_size


def _inliers(call, pts, ranges, r2, nb_points):
    """-> keep uint8 [V] by original index of the mean: more than nb_points means of its object within reach, itself included"""
    n_means = pts.shape[0]
    keep = torch.zeros(n_means, dtype=torch.uint8, device=pts.device)
    call("pointops2_supports_count_launcher", n_means, ptr(pts), ptr(ranges), ctypes.c_float(r2), nb_points, ptr(keep))
    return keep


def _survivors(keep, mean_object, n_objects):
    """-> (kept: 0-d int64 on the device, alive bool [O]: the objects with a surviving mean); the caller reads kept and alive.sum() back"""
    per_object = torch.zeros(n_objects, dtype=torch.int64, device=keep.device).index_add_(0, mean_object.long(), keep.long())
    return keep.sum(), per_object > 0


def _compact(mean, mean_object, keep, alive, n_kept, n_alive):
    """the kept means in their order, their objects renumbered over the surviving objects -> (points, object, source); sizes from the host,
    so no step waits for the device"""
    dev, n_means = mean.device, mean.shape[0]
    keep = keep.bool()
    at = torch.where(keep, torch.cumsum(keep.long(), 0) - 1, torch.full((), n_kept, dtype=torch.int64, device=dev))
    index = torch.empty(n_kept + 1, dtype=torch.int64, device=dev).index_copy_(0, at, torch.arange(n_means, device=dev))[:n_kept]  # (the last slot takes the rest)
    number = torch.cumsum(alive.long(), 0) - 1
    to = torch.where(alive, number, torch.full((), n_alive, dtype=torch.int64, device=dev))
    source = torch.empty(n_alive + 1, dtype=torch.int64, device=dev).index_copy_(0, to, torch.arange(alive.shape[0], device=dev))[:n_alive]
    return mean[index], number[mean_object[index].long()].to(torch.int32), source.to(torch.int32)


def clean_supports(coord, obj, n_objects=None, voxel=SUPPORT_VOXEL, radius=SUPPORT_RADIUS, nb_points=SUPPORT_NB_POINTS):
    """The clean-up that `instantiation_eval` gives every support before it returns it (util/train_utils.py:716-723: Open3D's
    voxel_down_sample(voxel_size=0.04), then remove_radius_outlier(nb_points=3, radius=0.1); a support left empty is dropped), on the
    output of objects(): coord [N, 3] fp32 and obj int32 / int64 [N] in -1 .. O-1 (GPU; -1 = in no object), O = n_objects or obj.max() + 1
    -> (points float32 [K, 3], object int32 [K] in 0 .. O'-1, source int32 [O']: the original number of every surviving object,
    n_objects int = O').  points / object feed merge_objects(points, object, n_objects) unchanged.

    Per object, independently of all others (csrc/supports.hip):
      1. voxel index: origin = double(lo) - voxel * 0.5 per axis, lo the OBJECT's own componentwise minimum (label_boxes; Open3D:
         GetMinBound() - voxel_size * 0.5); v = floor((double(p) - origin) / voxel), all in float64 with a true division;
      2. every occupied voxel gives one point: the float64 sum of its points in ascending original index, from 0.0, divided by their number
         as a double, rounded ONCE to fp32 - the departure: Open3D keeps doubles, every later step here takes fp32;
      3. a mean is kept when MORE than nb_points means of its object lie at d2 < fp32(radius)^2 of it, itself included; fp32,
         d2 = ((dx*dx) + (dy*dy)) + (dz*dz), as every radius test of this module;
      4. output order: ascending object, then ascending voxel (vz, vy, vx), vx fastest; an object with no surviving mean is dropped and the
         others are renumbered 0 .. O'-1 in ascending original number.
    UNPINNED - Open3D is on no machine the tests run on, no fixture records it: the half-voxel origin, floor, the mean in double and the
    self-inclusive count > nb_points are Open3D's published behaviour; whether its radius search is strict or inclusive at exactly
    `radius` is not known - strict here, as everywhere in this module; its output order is a hash map's iteration order and unspecified -
    ours is rule 4.
    Three read-backs whatever the number of objects (LAST_SUPPORTS): the range / bounding box up front, the number of voxels, the numbers
    of kept means and surviving objects.  The boxes stay on the device.
    Raises before any launch: RuntimeError for a CPU tensor or mismatched devices; TypeError / ValueError for a wrong dtype or shape, a
    label outside -1 .. O-1, non-finite coordinates, voxel or radius not finite and > 0, nb_points not an int >= 0, O > MAX_LABELS;
    ValueError when O * nx * ny * nz >= 2^61 for the voxels (or the cells of the radius grid) of the scene's box, or an axis exceeds
    MAX_CELLS_PER_AXIS.  N = 0, no point in an object or no surviving mean: empty tensors, nothing launched where nothing is to do."""
    who = "clean_supports"
    _check_tensors(who, coord, obj, "label")
    voxel, r, r2, nb_points = _support_settings(who, voxel, radius, nb_points)
    n_objects = _label_count(who, n_objects, "n_objects")
    dev, n = coord.device, coord.shape[0]
    LAST_SUPPORTS["launches"], LAST_SUPPORTS["readbacks"] = 0, 0

    def nothing():
        return (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev), 0)

    if n == 0:
        return nothing()
    coord = coord.contiguous()
    label = obj.to(torch.int32).contiguous()

    LAST_SUPPORTS["readbacks"] += 1
    _, l_min, l_max, n_valid, origin, top = _scan(who, coord, label)
    n_objects = _label_range(who, n_objects, l_min, l_max, "n_objects")
    if n_valid == 0 or n_objects == 0:
        return nothing()
    vdims = _voxel_dims(who, n_objects, origin, top, voxel)
    cell = float(r) * CELL_MARGIN
    dims = _dims(who, n_objects, origin, top, cell)

    call = functools.partial(_launch, LAST_SUPPORTS, dev)
    lo, _, _ = _boxes(coord, label, n_objects, dev, LAST_SUPPORTS)
    skeys, order, slot, n_voxels = _voxel_means(call, coord, label, n_objects, n_valid, lo, voxel, vdims)
    n_voxels = int(n_voxels.item())
    LAST_SUPPORTS["readbacks"] += 1
    mean, mean_object, _ = _means(call, coord, label, n_valid, n_voxels, skeys, order, slot)

    # the means lie inside the scene's box (a mean of fp32 values, rounded to fp32, does not leave their range), so its grid serves
    pts, _, _, ranges = _grid(call, mean, mean_object, n_objects, n_voxels, origin, cell, dims)
    keep = _inliers(call, pts, ranges, r2, nb_points)
    kept, alive = _survivors(keep, mean_object, n_objects)
    n_kept, n_alive = (int(v) for v in torch.stack([kept, alive.sum()]).cpu().numpy())
    LAST_SUPPORTS["readbacks"] += 1
    if n_kept == 0:
        return nothing()
    return _compact(mean, mean_object, keep, alive, n_kept, n_alive) + (n_alive,)


def box_supports(coord, shift, pred, eps=None, min_samples=None, min_points=None, contact_radius=CONTACT_RADIUS, share=CONTACT_SHARE,
                 face_classes=FACE_CLASSES, edge_faces=None, voxel=SUPPORT_VOXEL, radius=SUPPORT_RADIUS, nb_points=SUPPORT_NB_POINTS):
    """What `instantiation_eval` (util/train_utils.py:547-737) returns, in one call: instances() -> objects() -> clean_supports().
    coord, shift [N, 3] fp32 and pred int32 / int64 [N] on the GPU; eps, min_samples, min_points as instances() takes them,
    contact_radius (objects' radius), share, face_classes, edge_faces as objects() does, voxel, radius, nb_points as clean_supports().
    -> (points float32 [K, 3], object int32 [K], source int32 [O'], n_objects int - clean_supports' tuple: the cleaned supports, which
        feed merge_objects(points, object, n_objects) unchanged -, instance int32 [N], point_object int32 [N]: the per-point results of
        the first two steps, point_object in objects()' numbering, which `source` maps the cleaned objects back to).
    LAST, LAST_CONTACTS and LAST_SUPPORTS hold the counters of the three steps.  Raises as they do; the clean-up's settings are checked
    before the first step."""
    _support_settings("clean_supports", voxel, radius, nb_points)
    instance, instance_class, instance_size = instances(coord, shift, pred, eps, min_samples, min_points)
    point_object, _, n_objects = objects(coord, instance, instance_class, instance_size, contact_radius, share, face_classes, edge_faces)
    return clean_supports(coord, point_object, n_objects, voxel, radius, nb_points) + (instance, point_object)


# ---- the whole pass behind the model: supports, then boxes (test_iou.py:356-422) ----
def detect_settings(voxel=SUPPORT_VOXEL, radius=SUPPORT_RADIUS, nb_points=SUPPORT_NB_POINTS, merge_radius=MERGE_RADIUS, overlap=MERGE_OVERLAP,
                    min_neighbors=MERGE_MIN_NEIGHBORS, **instance_settings):
    """detect_boxes' settings that can be checked without the scene - the clean-up's and the merge's - raise here as their steps would, and
    a keyword that detect_boxes does not take raises TypeError.  The per-class settings of instances() and the settings of objects() need
    the scene's classes and are checked by those steps, before their own first launch."""
    unknown = sorted(set(instance_settings) - {"eps", "min_samples", "min_points", "contact_radius", "share", "face_classes", "edge_faces"})
    if unknown:
        raise TypeError(f"detect_boxes: unexpected settings {unknown}")
    _support_settings("clean_supports", voxel, radius, nb_points)
    _radius("merge_objects", merge_radius)
    merge_sets(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), np.zeros((0, 0), np.int32), np.zeros(0), overlap, min_neighbors)


def detect_boxes(coord, shift, pred, eps=None, min_samples=None, min_points=None, contact_radius=CONTACT_RADIUS, share=CONTACT_SHARE,
                 face_classes=FACE_CLASSES, edge_faces=None, voxel=SUPPORT_VOXEL, radius=SUPPORT_RADIUS, nb_points=SUPPORT_NB_POINTS,
                 merge_radius=MERGE_RADIUS, overlap=MERGE_OVERLAP, min_neighbors=MERGE_MIN_NEIGHBORS):
    """From the model's per-point outputs to the predicted boxes (test_iou.py:356-422) in one call: box_supports(), then
    merge_objects(points, object, n_objects) on its cleaned supports.  coord, shift [N, 3] fp32 and pred int32 / int64 [N] on the GPU; the
    settings up to nb_points are box_supports', merge_radius / overlap / min_neighbors are merge_objects' radius / overlap / min_neighbors.
    -> (boxes float32 [S, 6] = lo | hi per merged set, the reference's pred_box; points float32 [K, 3]: the cleaned support points;
        merged int32 [K]: the set of every support point; n_sets int = S; instance int32 [N], point_object int32 [N]: box_supports' per-point
        results).
    Pure composition: no step of its own, it raises as its parts do; the clean-up's and the merge's settings are checked before the first
    launch.  Fewer than two supports are not a special case: their zero or one boxes are returned."""
    detect_settings(voxel=voxel, radius=radius, nb_points=nb_points, merge_radius=merge_radius, overlap=overlap, min_neighbors=min_neighbors)
    points, obj, _, n_objects, instance, point_object = box_supports(coord, shift, pred, eps, min_samples, min_points, contact_radius, share,
                                                                      face_classes, edge_faces, voxel, radius, nb_points)
    merged, _, boxes, n_sets = merge_objects(points, obj, n_objects, merge_radius, overlap, min_neighbors)
    return boxes, points, merged, n_sets, instance, point_object
