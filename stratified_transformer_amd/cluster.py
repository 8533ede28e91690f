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
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import ptr

MAX_ROUNDS = 64            # of the component loop: the trees at least halve per round (csrc/dbscan.hip), so 2^31 points need 32
CELL_MARGIN = 1.0 + 2.0 ** -7   # the grid's cells are this much wider than the largest eps (fp32 rounding of the distance test)
MAX_CELLS_PER_AXIS = 1 << 20
LAST = {"rounds": 0, "launches": 0}   # of the most recent dbscan() call (tools/bench_dbscan.py, the chain test)

# instantiation_eval's settings (util/train_utils.py:558-563): faces (classes below 6) and edges
FACE_CLASSES = 6
FACE_SETTINGS = (0.1, 5, 50)
EDGE_SETTINGS = (0.15, 3, 20)


def _gpu(t, name):
    if not getattr(t, "is_cuda", False):
        raise RuntimeError(f"dbscan: {name}: expected a GPU tensor (the pointops2 HIP path has no CPU fallback), got {getattr(t, 'device', type(t).__name__)}")


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


def _check_inputs(xyz, group):
    _gpu(xyz, "xyz")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"dbscan: xyz must be [N, 3], got {tuple(xyz.shape)}")
    if xyz.dtype != torch.float32:
        raise TypeError(f"dbscan: xyz must be float32, got {xyz.dtype}")
    if group is not None:
        _gpu(group, "group")
        if group.device != xyz.device:
            raise RuntimeError(f"dbscan: group is on {group.device}, xyz on {xyz.device}")
        if group.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"dbscan: group must be int32 / int64, got {group.dtype}")
        if group.dim() != 1 or group.shape[0] != xyz.shape[0]:
            raise ValueError(f"dbscan: group must be [N] = [{xyz.shape[0]}], got {tuple(group.shape)}")


def _call(name, ref, *args):
    LAST["launches"] += 1
    if ref.device.index == torch.cuda.current_device():
        _lib.call(name, *args, device=ref.device)
    else:
        with torch.cuda.device(ref.device):
            _lib.call(name, *args, device=ref.device)


def dbscan(xyz, eps, min_samples, group=None):
    """DBSCAN of xyz [N, 3] fp32 (GPU) -> (labels int32 [N], core bool [N], n_clusters int32 [G]).

    group: int32 / int64 [N] with values in -1 .. G-1, None = one group.  Two points are neighbours only inside the same group, a point
    of group -1 is never a neighbour and keeps label -1; cluster numbers start at 0 in every group.  eps, min_samples: scalars, or
    sequences / tensors of length G looked up per group (G is their length; with scalars and a `group` G = group.max() + 1).
    Raises before any launch: RuntimeError for a CPU tensor, ValueError / TypeError for a wrong shape or dtype, ValueError for
    eps <= 0, min_samples < 1, a group outside -1 .. G-1 or non-finite coordinates.  RuntimeError when the component loop has not
    settled after MAX_ROUNDS rounds."""
    _check_inputs(xyz, group)
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

    # one read-back up front: the group range, the points that take part and their bounding box
    member = group >= 0
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    lo = torch.where(member[:, None], xyz, inf).amin(0)
    hi = torch.where(member[:, None], xyz, -inf).amax(0)
    finite = torch.isfinite(xyz).all()
    head = torch.cat([group.min()[None].double(), group.max()[None].double(), member.sum()[None].double(), finite[None].double(),
                      lo.double(), hi.double()]).cpu().numpy()
    g_min, g_max, n_valid, all_finite = int(head[0]), int(head[1]), int(head[2]), bool(head[3])
    if n_groups is None:
        n_groups = max(g_max + 1, 1)
    if g_min < -1 or g_max >= n_groups:
        raise ValueError(f"dbscan: group values must be in -1 .. {n_groups - 1}, got {g_min} .. {g_max}")
    if not all_finite:
        raise ValueError("dbscan: xyz must be finite")
    eps_h = np.broadcast_to(eps_h, (n_groups,)).astype(np.float32)
    ms_h = np.broadcast_to(ms_h, (n_groups,)).astype(np.int32)

    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    core = torch.zeros(n, dtype=torch.uint8, device=dev)
    n_clusters = torch.zeros(n_groups, dtype=torch.int32, device=dev)
    if n_valid == 0:
        return labels, core.bool(), n_clusters

    cell = float(np.float32(eps_h.max())) * CELL_MARGIN
    origin, top = head[4:7], head[7:10]
    dims = [int(np.floor((top[a] - origin[a]) / cell)) + 1 for a in range(3)]
    if max(dims) > MAX_CELLS_PER_AXIS or n_groups * dims[0] * dims[1] * dims[2] >= 2 ** 61:
        raise ValueError(f"dbscan: the cloud spans {dims} cells of edge {cell:g}: too many for the 64-bit cell keys")
    eps2 = torch.from_numpy(eps_h * eps_h).to(dev)          # fp32 product, rounded once
    ms = torch.from_numpy(ms_h).to(dev)

    keys = torch.empty(n, dtype=torch.int64, device=dev)
    _call("pointops2_dbscan_keys_launcher", xyz, n, n_groups, ptr(xyz), ptr(group), ctypes.c_double(origin[0]), ctypes.c_double(origin[1]),
          ctypes.c_double(origin[2]), ctypes.c_double(cell), dims[0], dims[1], dims[2], ptr(keys))
    skeys, order = torch.sort(keys, stable=True)
    pts = torch.empty(n_valid, 4, dtype=torch.float32, device=dev)
    sgroup = torch.empty(n_valid, dtype=torch.int32, device=dev)
    ranges = torch.empty(18, n_valid, dtype=torch.int32, device=dev)
    _call("pointops2_dbscan_prepare_launcher", xyz, n, n_valid, dims[0], dims[1], dims[2], ptr(xyz), ptr(skeys), ptr(order), ptr(pts),
          ptr(sgroup), ptr(ranges))
    score = torch.empty(n_valid, dtype=torch.uint8, device=dev)
    parent = torch.full((n,), -1, dtype=torch.int32, device=dev)
    _call("pointops2_dbscan_core_launcher", xyz, n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(ms), ptr(score), ptr(core),
          ptr(parent))

    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for rounds in range(1, MAX_ROUNDS + 1):
        _call("pointops2_dbscan_round_launcher", xyz, n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(score), ptr(parent),
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
    _call("pointops2_dbscan_label_launcher", xyz, n, n_valid, ptr(pts), ptr(sgroup), ptr(ranges), ptr(eps2), ptr(score), ptr(parent),
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
    _check_inputs(coord, pred)
    _gpu(shift, "shift")
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
