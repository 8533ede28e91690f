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

dbscan, contacts / objects, clean_supports and merge_objects stand on ONE fixed-radius grid: `_dims` and `_grid` (cell keys, torch's sort,
the nine prepared runs per point) build it here, csrc/radius_grid.h walks it on the device for all of them.  Every public call opens a
`_Call`: its `launch` and `read` are the library launch and the device-to-host transfer, counted in the stage's LAST_* where they happen.
The stages on a labelled cloud share the prologue `_labelled` (with `_scan`, the read-back up front) and the one-group grid `_label_grid`.
"""
import collections
import ctypes
import itertools

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
LAST = {"rounds": 0, "launches": 0}   # of the most recent dbscan() call (tools/bench_dbscan.py, the chain test); no "readbacks": see _Call.read

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


def dbscan_settings(eps, min_samples, n_groups):
    """dbscan's checks of eps and min_samples (scalars, or sequences / tensors of length n_groups; None = take the length from them)
    -> (G or None when both are scalars, eps f32 [G] or scalar, min_samples i32 [G] or scalar), validated"""
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


def _is_real(x):
    """a Python or numpy real number; a bool is none"""
    return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))


def _is_int(x):
    """a Python or numpy integer; a bool is none"""
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def _radius(who, radius):
    """-> (fp32(radius), its fp32 square, rounded once), both finite and > 0"""
    if not _is_real(radius):
        raise TypeError(f"{who}: radius must be a number, got {type(radius).__name__}")
    with np.errstate(all="ignore"):
        r = np.float32(radius)
        if not np.isfinite(radius) or not radius > 0 or not np.isfinite(r * r) or not r * r > 0:
            raise ValueError(f"{who}: radius must be finite and > 0, also when squared in fp32, got {radius}")
    return r, np.float32(r * r)


def _label_count(who, n_labels, name="n_labels"):
    if n_labels is None:
        return None
    if not _is_int(n_labels):
        raise TypeError(f"{who}: {name} must be an int, got {type(n_labels).__name__}")
    if n_labels < 0:
        raise ValueError(f"{who}: {name} must be >= 0, got {n_labels}")
    if n_labels > MAX_LABELS:
        raise ValueError(f"{who}: {n_labels} labels: at most {MAX_LABELS}")
    return int(n_labels)


def _row_words(who, n_valid, n_labels):
    """-> words of a row of labels in reach; the rows of n_valid points must fit MAX_BITMAP_BYTES where they are kept in memory"""
    words = (n_labels + 31) // 32
    if n_labels > REG_LABELS and n_valid * words * 4 > MAX_BITMAP_BYTES:
        raise ValueError(f"{who}: the bitmap of {n_valid} points x {n_labels} labels takes {n_valid * words * 4} bytes, more than {MAX_BITMAP_BYTES}")
    return words


class _Call:
    """One public call: the tensor checks (they give the device), who raises, and the stage's LAST_* dictionary, reset here.  Every
    library launch of this module goes through `launch`, every device-to-host transfer through `read`; each counts itself."""

    def __init__(self, who, counter, xyz, label, noun="label"):
        _check_tensors(who, xyz, label, noun)
        self.who, self.dev, self.counter = who, xyz.device, counter
        for key in counter:
            counter[key] = 0

    def count(self, key):
        if key in self.counter:
            self.counter[key] += 1

    def launch(self, name, *args):
        self.count("launches")
        _lib.call(name, *args, device=self.dev)

    def read(self, *tensors):
        """ONE transfer: the tensors (of one dtype) concatenated, brought to the host and split again -> a numpy array per tensor, in its
        shape.  Counted where the stage keeps "readbacks": LAST does not - dbscan's measure is its rounds, its scan up front is uncounted."""
        self.count("readbacks")
        if len(tensors) == 1:
            return [tensors[0].cpu().numpy()]
        flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
        ends = list(itertools.accumulate(t.numel() for t in tensors))
        return [flat[end - t.numel():end].reshape(tuple(t.shape)) for end, t in zip(ends, tensors)]


def _scan(call, xyz, label):
    """The one read-back up front: the label (group) range, the points that take part (label >= 0) and their bounding box
    -> (member bool [N], l_min, l_max, n_valid, finite: whether every coordinate is, origin float64 [3], top float64 [3])."""
    member = label >= 0
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=xyz.device)
    lo = torch.where(member[:, None], xyz, inf).amin(0)
    hi = torch.where(member[:, None], xyz, -inf).amax(0)
    l_min, l_max, n_valid, finite, origin, top = call.read(label.min().double(), label.max().double(), member.sum().double(),
                                                           torch.isfinite(xyz).all().double(), lo.double(), hi.double())
    return member, int(l_min), int(l_max), int(n_valid), bool(finite), origin, top


# a labelled cloud as the stages take it: xyz and label (int32) contiguous, member = label >= 0, n_valid labelled points in the box origin .. top
_Labelled = collections.namedtuple("_Labelled", "xyz label member n_labels n_valid origin top dev n")


def _labelled(call, xyz, label, n_labels, name="n_labels"):
    """The prologue of every stage on a labelled cloud, behind the call's tensor checks and the stage's settings: the label count, N = 0
    (nothing is read, n_valid = 0), the copies, the one read-back up front, the label range, then finite coordinates -> _Labelled.
    The caller returns its empty result when n_valid == 0 or n_labels == 0; `readbacks` 0 / 1 tells no point from no labelled point."""
    n_labels = _label_count(call.who, n_labels, name)
    n = xyz.shape[0]
    if n == 0:
        return _Labelled(xyz, label, None, n_labels or 0, 0, None, None, call.dev, 0)
    xyz = xyz.contiguous()
    label = label.to(torch.int32).contiguous()
    member, l_min, l_max, n_valid, finite, origin, top = _scan(call, xyz, label)
    if n_labels is None:
        n_labels = _label_count(call.who, max(l_max + 1, 0), name)
    if l_min < -1 or l_max >= n_labels:
        raise ValueError(f"{call.who}: label values must be in -1 .. {n_labels - 1}, got {l_min} .. {l_max}")
    if not finite:
        raise ValueError(f"{call.who}: xyz must be finite")
    return _Labelled(xyz, label, member, n_labels, n_valid, origin, top, call.dev, n)


def _dims(who, n_groups, origin, top, r):
    """The cells of the grid for a largest radius r, CELL_MARGIN wider than it -> (cell edge, cells per axis [nx, ny, nz]); ValueError
    when n_groups such grids do not fit the 64-bit cell keys"""
    cell = float(r) * CELL_MARGIN
    dims = [int(np.floor((top[a] - origin[a]) / cell)) + 1 for a in range(3)]
    if max(dims) > MAX_CELLS_PER_AXIS or n_groups * dims[0] * dims[1] * dims[2] >= 2 ** 61:
        raise ValueError(f"{who}: the cloud spans {dims} cells of edge {cell:g}: too many for the 64-bit cell keys")
    return cell, dims


def _grid(call, xyz, group, n_groups, n_valid, origin, cell, dims):
    """The fixed-radius grid of csrc/radius_grid.h over the points with a group in 0 .. n_groups-1: cell keys, torch's stable sort, the
    nine runs per point -> (pts float32 [n_valid, 4] = x, y, z, original index as bits, in the grid's order; order int64 [N]: the sort's
    permutation, the n_valid points that take part first; sorted_group int32 [n_valid]; ranges int32 [18, n_valid])."""
    dev, n = xyz.device, xyz.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    call.launch("pointops2_dbscan_keys_launcher", n, n_groups, ptr(xyz), ptr(group), ctypes.c_double(origin[0]), ctypes.c_double(origin[1]),
                ctypes.c_double(origin[2]), ctypes.c_double(cell), dims[0], dims[1], dims[2], ptr(keys))
    skeys, order = torch.sort(keys, stable=True)
    pts = torch.empty(n_valid, 4, dtype=torch.float32, device=dev)
    sgroup = torch.empty(n_valid, dtype=torch.int32, device=dev)
    ranges = torch.empty(18, n_valid, dtype=torch.int32, device=dev)
    call.launch("pointops2_dbscan_prepare_launcher", n, n_valid, dims[0], dims[1], dims[2], ptr(xyz), ptr(skeys), ptr(order), ptr(pts),
                ptr(sgroup), ptr(ranges))
    return pts, order, sgroup, ranges


def _label_grid(call, p, r):
    """the grid over the labelled points of p (_Labelled) for radius r, as ONE group; raises as _dims does, before its first launch
    -> (pts float32 [n_valid, 4], sorted_label int32 [n_valid], ranges int32 [18, n_valid]), all in the grid's order"""
    cell, dims = _dims(call.who, 1, p.origin, p.top, r)
    return _member_grid(call, p.xyz, p.label, p.member, p.n_valid, p.origin, cell, dims)


def _member_grid(call, xyz, label, member, n_valid, origin, cell, dims):
    """_label_grid on cells that the caller has laid out"""
    group = member.to(torch.int32) - 1                       # one group: 0 for a labelled point, -1 for the others
    pts, order, _, ranges = _grid(call, xyz, group, 1, n_valid, origin, cell, dims)
    return pts, label[order[:n_valid]].contiguous(), ranges


def _lookup(values, label, dev):
    """host values int32 [I] looked up per point, -1 for label -1 -> (per point int32 [N], the table on the device int32 [I + 1])"""
    table = torch.from_numpy(np.concatenate([values, np.full(1, -1, np.int32)])).to(dev)                     # (the last entry serves -1)
    return table[label.long()], table


def dbscan(xyz, eps, min_samples, group=None):
    """DBSCAN of xyz [N, 3] fp32 (GPU) -> (labels int32 [N], core bool [N], n_clusters int32 [G]).

    group: int32 / int64 [N] with values in -1 .. G-1, None = one group.  Two points are neighbours only inside the same group, a point
    of group -1 is never a neighbour and keeps label -1; cluster numbers start at 0 in every group.  eps, min_samples: scalars, or
    sequences / tensors of length G looked up per group (G is their length; with scalars and a `group` G = group.max() + 1).
    Raises before any launch: RuntimeError for a CPU tensor, ValueError / TypeError for a wrong shape or dtype, ValueError for
    eps <= 0, min_samples < 1, a group outside -1 .. G-1 or non-finite coordinates.  RuntimeError when the component loop has not
    settled after MAX_ROUNDS rounds."""
    # not on _labelled: G comes from eps / min_samples and `group` may be None, which would be a second path inside the shared prologue
    call = _Call("dbscan", LAST, xyz, group, "group")
    n_groups, eps_h, ms_h = dbscan_settings(eps, min_samples, 1 if group is None else None)
    dev, n = call.dev, xyz.shape[0]
    if n == 0:
        g = n_groups if n_groups is not None else 1
        return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.bool, device=dev),
                torch.zeros(g, dtype=torch.int32, device=dev))
    xyz = xyz.contiguous()
    if group is None:
        group = torch.zeros(n, dtype=torch.int32, device=dev)
    group = group.to(torch.int32).contiguous()

    _, g_min, g_max, n_valid, finite, origin, top = _scan(call, xyz, group)
    if not finite:
        raise ValueError("dbscan: xyz must be finite")
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

    cell, dims = _dims("dbscan", n_groups, origin, top, np.float32(eps_h.max()))
    eps2 = torch.from_numpy(eps_h * eps_h).to(dev)          # fp32 product, rounded once
    ms = torch.from_numpy(ms_h).to(dev)

    pts, _, sgroup, ranges = _grid(call, xyz, group, n_groups, n_valid, origin, cell, dims)
    score = torch.empty(n_valid, dtype=torch.uint8, device=dev)
    parent = torch.full((n,), -1, dtype=torch.int32, device=dev)
    call.launch("pointops2_dbscan_core_launcher", n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(ms), ptr(score), ptr(core),
                ptr(parent))

    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for rounds in range(1, MAX_ROUNDS + 1):
        call.launch("pointops2_dbscan_round_launcher", n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(score), ptr(parent),
                    ptr(changed))
        call.count("launches")                               # (a round is two kernels)
        LAST["rounds"] = rounds
        if int(changed.item()) == 0:                         # the one small read-back per round: LAST["rounds"] is its count, so not through call.read
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
    call.launch("pointops2_dbscan_label_launcher", n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(score), ptr(parent),
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
    # (the two .item() of this function are outside any counted stage: dbscan, which it calls, owns LAST and resets it)
    n_classes = lengths.pop() if lengths else (max(int(pred.max().item()) + 1, 1) if n > 0 else 1)
    eps_h = _class_settings(eps, n_classes, FACE_SETTINGS[0], EDGE_SETTINGS[0], np.float32, "eps")
    ms_h = _class_settings(min_samples, n_classes, FACE_SETTINGS[1], EDGE_SETTINGS[1], np.int32, "min_samples")
    mp_h = _class_settings(min_points, n_classes, FACE_SETTINGS[2], EDGE_SETTINGS[2], np.int32, "min_points")
    dbscan_settings(eps_h, ms_h, n_classes)
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


def _contact_tables(call, p, r, r2, want_min):
    """the tables of contacts() over the labelled cloud p (_Labelled): zeros / +inf when it holds no labelled point, else the grid, its walk
    and - want_min - the sweep over all pairs -> (count int32 [I, I], min_d2 float32 [I, I] or None)"""
    count = torch.zeros(p.n_labels, p.n_labels, dtype=torch.int32, device=p.dev)
    min_d2 = torch.full((p.n_labels, p.n_labels), float("inf"), dtype=torch.float32, device=p.dev) if want_min else None
    if p.n_valid == 0 or p.n_labels == 0:
        return count, min_d2
    words = _row_words(call.who, p.n_valid, p.n_labels)
    pts, slabel, ranges = _label_grid(call, p, r)
    bitmap = torch.zeros(p.n_valid, words, dtype=torch.int32, device=p.dev) if p.n_labels > REG_LABELS else None
    call.launch("pointops2_contacts_count_launcher", p.n_valid, p.n_labels, ptr(pts), ptr(slabel), ptr(ranges), ctypes.c_float(r2), ptr(bitmap),
                ptr(count))
    if want_min:
        llabel, by_label = torch.sort(slabel, stable=True)   # ascending label; inside a label the grid's order, which keeps tiles compact
        label_pts = torch.cat([pts[by_label, :3], llabel.view(torch.float32)[:, None]], 1).contiguous()
        call.launch("pointops2_contacts_min_launcher", p.n_valid, p.n_labels, ptr(label_pts), ptr(min_d2))
    return count, min_d2


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
    call = _Call("contacts", LAST_CONTACTS, xyz, label)
    r, r2 = _radius(call.who, radius)
    return _contact_tables(call, _labelled(call, xyz, label, n_labels), r, r2, True)


def _link_settings(share, face_classes, edge_faces):
    """link_objects' settings -> (face_classes as an int, edge_faces as a tuple of pairs of ints), validated"""
    if not _is_real(share) or not np.isfinite(share) or share < 0:
        raise ValueError(f"objects: share must be a finite number >= 0, got {share!r}")
    edge_faces = EDGE_FACES if edge_faces is None else tuple(tuple(int(f) for f in pair) for pair in edge_faces)
    face_classes = int(face_classes)
    if any(len(pair) != 2 or not all(0 <= f < face_classes for f in pair) for pair in edge_faces):
        raise ValueError(f"objects: edge_faces must hold pairs of face classes below {face_classes}")
    return face_classes, edge_faces


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
    face_classes, edge_faces = _link_settings(share, face_classes, edge_faces)
    count = np.asarray(count)
    size = np.asarray(size).astype(np.int64).reshape(-1)
    cls = np.asarray(instance_class).astype(np.int64).reshape(-1)
    n_inst = cls.shape[0]
    if count.shape != (n_inst, n_inst) or size.shape != (n_inst,):
        raise ValueError(f"objects: count must be [I, I] and size [I] for the {n_inst} instances, got {count.shape} and {size.shape}")
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
    call = _Call("objects", LAST_CONTACTS, coord, instance)
    dev = call.dev
    if not isinstance(instance_class, torch.Tensor) or instance_class.dim() != 1 or instance_class.dtype not in (torch.int32, torch.int64):
        raise ValueError("objects: instance_class must be an int32 / int64 tensor [I]")
    n_inst = instance_class.shape[0]
    if instance_size is not None and (not isinstance(instance_size, torch.Tensor) or tuple(instance_size.shape) != (n_inst,)
                                      or instance_size.dtype not in (torch.int32, torch.int64)):
        raise ValueError(f"objects: instance_size must be an int32 / int64 tensor [{n_inst}]")
    _link_settings(share, face_classes, edge_faces)
    r, r2 = _radius(call.who, radius)
    count, _ = _contact_tables(call, _labelled(call, coord, instance, n_inst), r, r2, False)
    if instance_size is None:
        instance_size = torch.bincount(instance[instance >= 0].long(), minlength=n_inst) if coord.shape[0] > 0 else torch.zeros(n_inst, dtype=torch.int64)
    count_h, size_h, class_h = call.read(count.long(), instance_size.to(dev).long(), instance_class.to(dev).long())   # the one read-back
    object_of, n_objects = link_objects(count_h, size_h, class_h, share, face_classes, edge_faces)
    face_object = np.where(class_h < int(face_classes), object_of, -1).astype(np.int32)
    return _lookup(face_object, instance, dev)[0], torch.from_numpy(object_of).to(dev), n_objects


# ---- the OBB merging behind the grouping (test.py:294-326, the same loop at test_iou.py:373-406) and the box detection score that
# test_iou.py:409-466 takes from the merged sets, on csrc/boxes.hip ----
MERGE_RADIUS = 0.2          # test.py:310 pc_thre
MERGE_OVERLAP = 0.3         # util/train_utils.py:861 thre
MERGE_MIN_NEIGHBORS = 10    # test.py:312
LAST_MERGE = {"launches": 0, "readbacks": 0}   # of the most recent label_boxes() / merge_objects() call (tools/bench_merge.py)


def _boxes(call, p):
    """the launch of label_boxes on the labelled cloud p (_Labelled) -> (lo, hi, size)"""
    lo = torch.full((p.n_labels, 3), float("inf"), dtype=torch.float32, device=p.dev)
    hi = torch.full((p.n_labels, 3), float("-inf"), dtype=torch.float32, device=p.dev)
    size = torch.zeros(p.n_labels, dtype=torch.int32, device=p.dev)
    if p.n > 0 and p.n_labels > 0:
        call.launch("pointops2_label_boxes_launcher", p.n, p.n_labels, ptr(p.xyz), ptr(p.label), ptr(lo), ptr(hi), ptr(size))
    return lo, hi, size


def label_boxes(xyz, label, n_labels=None):
    """The axis-aligned box and the size of every labelled point set: xyz [N, 3] fp32 and label int32 / int64 [N] in -1 .. I-1 (GPU; -1 =
    the point takes no part) -> (lo float32 [I, 3], hi float32 [I, 3], size int32 [I]) with I = n_labels, or label.max() + 1.

    lo / hi: the componentwise minimum / maximum of the label's points, exact (integer atomics on an order-preserving image of the fp32
    values, csrc/boxes.hip); -0.0 counts as +0.0, so compare by value.  A label without a point keeps +inf / -inf / 0.
    Raises before any launch: RuntimeError for a CPU tensor or mismatched devices; TypeError / ValueError for a wrong dtype or shape, a
    label outside -1 .. I-1, non-finite coordinates or I > MAX_LABELS.  N = 0 or I = 0 launches nothing."""
    call = _Call("label_boxes", LAST_MERGE, xyz, label)
    return _boxes(call, _labelled(call, xyz, label, n_labels))


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


def _merge_settings(overlap, min_neighbors):
    """merge_sets' settings, validated"""
    if not _is_real(overlap) or not np.isfinite(overlap) or overlap < 0:
        raise ValueError(f"merge_sets: overlap must be a finite number >= 0, got {overlap!r}")
    if not _is_int(min_neighbors) or min_neighbors < 0:
        raise ValueError(f"merge_sets: min_neighbors must be an int >= 0, got {min_neighbors!r}")


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
    _merge_settings(overlap, min_neighbors)
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
    call = _Call("merge_objects", LAST_MERGE, coord, obj)
    r, r2 = _radius(call.who, radius)
    _merge_settings(overlap, min_neighbors)
    p = _labelled(call, coord, obj, n_objects, "n_objects")
    if p.n_valid == 0 or p.n_labels == 0:
        return (torch.full((p.n,), -1, dtype=torch.int32, device=p.dev), torch.full((p.n_labels,), -1, dtype=torch.int32, device=p.dev),
                torch.zeros(0, 6, dtype=torch.float32, device=p.dev), 0)
    _row_words(call.who, p.n_valid, p.n_labels)

    pts, slabel, ranges = _label_grid(call, p, r)
    lo, hi, size = _boxes(call, p)
    rows = _rows(call, pts, slabel, ranges, p.n_labels, r2)
    pat, pat_count = _patterns(slabel, rows)
    tables = _merge_tables(call, lo, hi, size, pat, pat_count)
    set_of, sets = merge_sets(*tables, overlap, min_neighbors)
    boxes = np.array([np.concatenate([tables[0][s].min(0), tables[1][s].max(0)]) for s in sets], dtype=np.float32).reshape(len(sets), 6)
    merged, table = _lookup(set_of, p.label, p.dev)
    return merged, table[:p.n_labels], torch.from_numpy(boxes).to(p.dev), len(sets)


def _rows(call, pts, slabel, ranges, n_objects, r2):
    """the reach rows on the grid of _label_grid -> rows int32 [n_valid, words]: the objects within reach of every point, its own left out,
    in the grid's order"""
    rows = torch.zeros(pts.shape[0], (n_objects + 31) // 32, dtype=torch.int32, device=pts.device)
    call.launch("pointops2_reach_rows_launcher", pts.shape[0], n_objects, ptr(pts), ptr(slabel), ptr(ranges), ctypes.c_float(r2), ptr(rows))
    return rows


def _reach_rows(coord, label, member, n, n_valid, n_objects, origin, cell, dims, r2, dev):
    """merge_objects' two device steps, _member_grid and _rows, in a call of their own and on cells that the caller has laid out - the
    entry of tests/test_merge_hip.py, which checks the rows on its own cells -> (sorted_label int32 [n_valid], rows int32 [n_valid, words])"""
    call = _Call("merge_objects", LAST_MERGE, coord, label)
    pts, slabel, ranges = _member_grid(call, coord, label, member, n_valid, origin, cell, dims)
    return slabel, _rows(call, pts, slabel, ranges, n_objects, r2)


def _patterns(slabel, rows):
    """the distinct (object, row) patterns of the border points - the points whose row is not empty - and how many points show each
    -> (pat int32 [P, 1 + words], count int64 [P]); on the device"""
    border = (rows != 0).any(1)
    keyed = torch.cat([slabel[border, None], rows[border]], 1)
    if keyed.shape[0] == 0:
        return keyed, torch.zeros(0, dtype=torch.int64, device=rows.device)
    return torch.unique(keyed, dim=0, return_counts=True)


def _merge_tables(call, lo, hi, size, pat, pat_count):
    """the one final read-back of merge_objects: boxes, sizes and patterns as one array of 32-bit words -> merge_sets' six tables"""
    lo_h, hi_h, size_h, pat_h, count_h = call.read(lo.view(torch.int32), hi.view(torch.int32), size, pat, pat_count.to(torch.int32))
    return lo_h.view(np.float32), hi_h.view(np.float32), size_h, pat_h[:, 0], pat_h[:, 1:], count_h


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
    if not _is_real(overlap_threshold) or not np.isfinite(overlap_threshold):
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
    if not _is_real(voxel):
        raise TypeError(f"{who}: voxel must be a number, got {type(voxel).__name__}")
    if not np.isfinite(voxel) or not voxel > 0:
        raise ValueError(f"{who}: voxel must be finite and > 0, got {voxel}")
    if not _is_int(nb_points) or nb_points < 0 or nb_points >= 2 ** 31:
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


def _voxel_means(call, p, lo, voxel, dims):
    """voxel keys from every object's own minimum `lo` (device), torch's stable sort, the head flags and their scan
    -> (sorted_keys int64 [N], order int64 [N], slot int64 [n_valid], n_voxels: read back here, the second read-back of clean_supports)"""
    keys = torch.empty(p.n, dtype=torch.int64, device=p.dev)
    call.launch("pointops2_supports_keys_launcher", p.n, p.n_labels, ptr(p.xyz), ptr(p.label), ptr(lo), ctypes.c_double(voxel), dims[0], dims[1],
                dims[2], ptr(keys))
    skeys, order = torch.sort(keys, stable=True)
    head = torch.ones(p.n_valid, dtype=torch.int64, device=p.dev)
    head[1:] = skeys[1:p.n_valid] != skeys[:p.n_valid - 1]
    slot = torch.cumsum(head, 0) - 1                         # the exclusive count of heads, at a head
    return skeys, order, slot, int(call.read(slot[-1] + 1)[0])


def _means(call, p, n_voxels, skeys, order, slot):
    """-> (mean float32 [V, 3], mean_object int32 [V], mean_size int32 [V]) in the order of the keys: object, then vz, vy, vx"""
    mean = torch.empty(n_voxels, 3, dtype=torch.float32, device=p.dev)
    mean_object = torch.empty(n_voxels, dtype=torch.int32, device=p.dev)
    mean_size = torch.empty(n_voxels, dtype=torch.int32, device=p.dev)
    call.launch("pointops2_supports_means_launcher", p.n, p.n_valid, n_voxels, ptr(p.xyz), ptr(p.label), ptr(skeys), ptr(order), ptr(slot),
                ptr(mean), ptr(mean_object), ptr(mean_size))
    return mean, mean_object, mean_size


def _inliers(call, pts, ranges, r2, nb_points):
    """-> keep uint8 [V] by original index of the mean: more than nb_points means of its object within reach, itself included"""
    n_means = pts.shape[0]
    keep = torch.zeros(n_means, dtype=torch.uint8, device=pts.device)
    call.launch("pointops2_supports_count_launcher", n_means, ptr(pts), ptr(ranges), ctypes.c_float(r2), nb_points, ptr(keep))
    return keep


def _survivors(call, keep, mean_object, n_objects):
    """-> (alive bool [O]: the objects with a surviving mean, the number of kept means, the number of such objects: both read back here, the
    third read-back of clean_supports)"""
    alive = torch.zeros(n_objects, dtype=torch.int64, device=keep.device).index_add_(0, mean_object.long(), keep.long()) > 0
    n_kept, n_alive = call.read(torch.stack([keep.sum(), alive.sum()]))[0]
    return alive, int(n_kept), int(n_alive)


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
    call = _Call("clean_supports", LAST_SUPPORTS, coord, obj)
    voxel, r, r2, nb_points = _support_settings(call.who, voxel, radius, nb_points)
    p = _labelled(call, coord, obj, n_objects, "n_objects")

    def nothing():
        return (torch.zeros(0, 3, dtype=torch.float32, device=p.dev), torch.zeros(0, dtype=torch.int32, device=p.dev),
                torch.zeros(0, dtype=torch.int32, device=p.dev), 0)

    if p.n_valid == 0 or p.n_labels == 0:
        return nothing()
    vdims = _voxel_dims(call.who, p.n_labels, p.origin, p.top, voxel)
    cell, dims = _dims(call.who, p.n_labels, p.origin, p.top, r)

    lo, _, _ = _boxes(call, p)
    skeys, order, slot, n_voxels = _voxel_means(call, p, lo, voxel, vdims)
    mean, mean_object, _ = _means(call, p, n_voxels, skeys, order, slot)

    # the means lie inside the scene's box (a mean of fp32 values, rounded to fp32, does not leave their range), so its grid serves
    pts, _, _, ranges = _grid(call, mean, mean_object, p.n_labels, n_voxels, p.origin, cell, dims)
    keep = _inliers(call, pts, ranges, r2, nb_points)
    alive, n_kept, n_alive = _survivors(call, keep, mean_object, p.n_labels)
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
    _merge_settings(overlap, min_neighbors)


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
