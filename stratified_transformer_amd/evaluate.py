"""How a trained model is evaluated, on the device: the reference's test loop (test_backup.py:177-187, :230-287; the fork's test.py has
the same structure) splits a room into voxel-round-robin parts, tiles every part larger than `voxel_max` with overlapping
nearest-neighbour crops in a sequential numpy loop, batches the crops through the model, adds softmax(logits) into a per-point vote
tensor, normalises, takes the arg-max and counts intersection / union.  Here the scene stays on the GPU: the seed (argmin), the
distances, the priority update and the vote are HIP kernels (csrc/evaltile.hip), the sort is the stable device sort that
dataprep.crop_nearest uses.  Where numpy's unstable argsort leaves the order among equal distances unspecified the ascending-index
order is pinned - every such order is a valid output of the reference.

Kept quirk of the reference: `pred[idx_part, :] += pred_part` (:281) is an indexed assignment without accumulation - when a point
appears more than once in one batch (overlapping crops of one batch: the normal case) only one of its rows is added.  CPU torch lets
the row at the last position write, and so does SceneVotes.add; CUDA may pick any of them.

The DCF fork's detection pass (test_iou.py / test.py) is here as well: its model returns (logits, shift) and its loop keeps a second
accumulator, `pred_shift[idx_part, :] += shift_part` - SceneVotes(..., shifts=True) and scene_predict, on the fused vote of
csrc/evaltile.hip -; dense_points is its loader's outlier filter, detect_scene the whole pass from the scene to the boxes and their score.

Not covered: the test-time transforms (host numpy callables; the caller sums scene_eval over them), file reading / writing, the
meters and the logging, the fork's accumulation of the score over scenes and its .obj exports."""
import collections

import torch

from . import _lib, cluster, pointops
from ._lib import ptr
from .dataprep import _coord, voxelize

STATUS_DMAX_ZERO, STATUS_BAD_INDEX = 1, 2   # ET_STATUS_* of csrc/evaltile.hip
MAX_CLASSES = 64
LAST = {"crops": 0, "reads": 0}             # of the most recent crop_cover() call (tools/bench_evaltile.py, the read-back test)


def _gpu(t, name):
    if not getattr(t, "is_cuda", False):
        raise RuntimeError(f"{name}: expected a GPU tensor (the pointops2 HIP path has no CPU fallback), got {getattr(t, 'device', type(t).__name__)}")


def scene_parts(coord, voxel_size):
    """test_backup.py:179-187: the voxel-round-robin parts of a scene.  coord [N,3] f32 / f64 on the GPU, already shifted to its
    minimum (:179-180).  Part i takes from every occupied voxel its (i % count)-th point, in the order of
    dataprep.voxelize(mode=1) (ascending index inside a voxel) -> parts [count.max(), n_voxels] int64; a falsy voxel_size gives the
    single row arange(N) (:187).  One host read: count.max()."""
    coord = _coord(coord)
    if not voxel_size:
        return torch.arange(coord.shape[0], device=coord.device)[None]
    idx_sort, count = voxelize(coord, voxel_size, mode=1)
    start = torch.cumsum(count, 0) - count
    rows = torch.arange(int(count.max()), device=coord.device)
    return idx_sort[start[None] + rows[:, None] % count[None]]


def crop_cover(coord, voxel_max, priority=None):
    """test_backup.py:239-251 for one part: overlapping crops of the `voxel_max` points nearest to a seed, until every point is in one.
    coord [n,3] f32 / f64 on the GPU with n > voxel_max; priority float64 [n] replays `np.random.rand(n) * 1e-3` (omitted: drawn
    here; not modified).  Per crop: seed = argmin(priority), lowest index among equal values; crop = the first voxel_max entries of
    the stable ascending sort of the squared distances to the seed (ties by index); priority[crop] += (1 - dist / dist.max())^2 in
    the coordinates' dtype.  -> (crops int64 [n_crops, voxel_max], seeds int64 [n_crops], the final priority float64 [n]).

    The seed's own priority rises by exactly 1 and an uncovered point stays below 1e-3, so no point is the seed twice before
    the loop ends: more than n crops raise RuntimeError.  ValueError when voxel_max points coincide with a seed (the largest
    distance of the crop is 0: the reference divides 0 / 0 there and never ends).  One small read-back per crop (covered count and
    status); the seed index stays on the device."""
    coord = _coord(coord)
    n, dev = coord.shape[0], coord.device
    voxel_max = int(voxel_max)
    if voxel_max < 1 or n <= voxel_max:
        raise ValueError(f"crop_cover: need 1 <= voxel_max < n, got voxel_max {voxel_max} for {n} points (a part this small is used as a whole)")
    if priority is None:
        priority = torch.rand(n, dtype=torch.float64, device=dev) * 1e-3
    else:
        _gpu(priority, "crop_cover: priority")
        if priority.dtype != torch.float64 or priority.shape != (n,):
            raise ValueError(f"crop_cover: priority must be float64 [{n}], got {priority.dtype} {tuple(priority.shape)}")
        priority = priority.to(dev).clone()
    is_f64 = int(coord.dtype == torch.float64)
    parts = _lib.lib().pointops2_evaltile_max_parts()
    part_value = torch.empty(parts, dtype=torch.float64, device=dev)
    part_index = torch.empty(parts, dtype=torch.int32, device=dev)
    seed = torch.empty(1, dtype=torch.int64, device=dev)
    dist = torch.empty(n, dtype=coord.dtype, device=dev)
    covered = torch.zeros(n, dtype=torch.uint8, device=dev)
    report = torch.zeros(2, dtype=torch.int32, device=dev)
    crops, seeds = [], []
    LAST["crops"], LAST["reads"] = 0, 0
    # (no device guard: the two launches get theirs from _lib.call; the sort, the clones and the read-backs are torch operators on
    # tensors of `dev`, which run on their operands' device whichever is current)
    while True:
        if len(crops) == n:
            raise RuntimeError(f"crop_cover: {n} crops have not covered the {n} points")
        _lib.call("pointops2_evaltile_seed_dist_launcher", n, is_f64, ptr(coord), ptr(priority), ptr(part_value), ptr(part_index), ptr(seed),
                  ptr(dist), device=dev)
        crop = torch.sort(dist, stable=True)[1][:voxel_max].clone()
        _lib.call("pointops2_evaltile_update_launcher", n, voxel_max, is_f64, ptr(dist), ptr(crop), ptr(priority), ptr(covered), ptr(report),
                  device=dev)
        crops.append(crop)
        seeds.append(seed.clone())
        n_covered, status = report.tolist()                      # the one small read-back per crop
        LAST["crops"], LAST["reads"] = len(crops), LAST["reads"] + 1
        if status == STATUS_DMAX_ZERO:
            raise ValueError(f"crop_cover: the {voxel_max} points nearest to seed point {int(seed)} (crop {len(crops) - 1}) coincide with it "
                             f"(largest distance 0; {n_covered} of {n} points covered): the reference's loop divides 0 / 0 here and never ends")
        if status != 0:
            raise RuntimeError(f"crop_cover: the sort returned an index outside [0, {n}) (status {status})")
        if n_covered == n:
            break
    return torch.stack(crops), torch.cat(seeds), priority


class SceneVotes:
    """The per-point vote tensor of test_backup.py:231, :278-283.  add(logits, idx): pred[idx, :] += softmax(logits, -1) with the
    reference's indexed-assignment semantics - when an index repeats inside one call only the row at its LAST position writes.
    logits [m, classes] f32 / f16 / bf16 (arithmetic fp32), idx int64 [m], on the GPU.  result(): pred / (pred.sum(-1)[:, None] + 1e-8);
    labels(): the arg-max of the raw votes, int64 [n_points] (the fork's `pred.max(1)[1]`, test_iou.py:343).

    shifts=True: the fork's second accumulator (test_iou.py:267, :285, :338) - the object also owns `shift`, float32 [n_points, 3], and is a
    SceneShiftVotes, whose add(logits, idx, shift) takes the model's shift rows [m, 3] (f32 / f16 / bf16, independent of the logits' type)
    and does `shift[idx, :] += shift_rows` under the same rule in the same kernel: the row that writes the votes of a point writes its
    shift.  Without shifts nothing changes: the same launcher, the same kernels."""

    def __new__(cls, n_points=None, classes=None, device="cuda", shifts=False):
        return object.__new__(SceneShiftVotes if shifts and cls is SceneVotes else cls)

    def __init__(self, n_points, classes, device="cuda", shifts=False):
        n_points, classes = int(n_points), int(classes)
        if n_points < 1 or not 1 <= classes <= MAX_CLASSES:
            raise ValueError(f"SceneVotes: need n_points >= 1 and 1 <= classes <= {MAX_CLASSES}, got {n_points}, {classes}")
        self.pred = torch.zeros(n_points, classes, dtype=torch.float32, device=device)
        self._stamp = torch.full((n_points,), -1, dtype=torch.int32, device=device)   # largest row number per point inside a call
        self._status = torch.zeros(1, dtype=torch.int32, device=device)
        self.shift = torch.zeros(n_points, 3, dtype=torch.float32, device=device) if shifts else None

    def _rows(self, logits, idx):
        _gpu(logits, "SceneVotes.add: logits")
        _gpu(idx, "SceneVotes.add: idx")
        classes = self.pred.shape[1]
        if logits.dim() != 2 or logits.shape[1] != classes or logits.dtype not in _lib.ROW_TYPES:
            raise ValueError(f"SceneVotes.add: logits must be [m, {classes}] float32 / float16 / bfloat16, got {logits.dtype} {tuple(logits.shape)}")
        if idx.dtype != torch.int64 or idx.shape != (logits.shape[0],):
            raise ValueError(f"SceneVotes.add: idx must be int64 [{logits.shape[0]}], got {idx.dtype} {tuple(idx.shape)}")
        if logits.device != self.pred.device or idx.device != self.pred.device:
            raise RuntimeError(f"SceneVotes.add: logits on {logits.device}, idx on {idx.device}, the votes on {self.pred.device}")
        return logits.detach().contiguous(), idx.contiguous()

    def add(self, logits, idx):
        logits, idx = self._rows(logits, idx)
        n_points, classes = self.pred.shape
        _lib.call("pointops2_evaltile_vote_launcher", logits.shape[0], classes, n_points, _lib.ROW_TYPES[logits.dtype], ptr(logits), ptr(idx),
                  ptr(self._stamp), ptr(self.pred), ptr(self._status), device=self.pred.device)

    def _check(self):
        if int(self._status.item()) != 0:
            raise IndexError(f"SceneVotes: an index given to add() was outside [0, {self.pred.shape[0]})")

    def result(self):
        self._check()
        return self.pred / (self.pred.sum(-1)[:, None] + 1e-8)

    def labels(self):
        self._check()
        return self.pred.max(1)[1]


class SceneShiftVotes(SceneVotes):
    """SceneVotes(..., shifts=True): the votes and the summed shifts of the fork's test loop.  add() needs the shift rows."""

    def __init__(self, n_points, classes, device="cuda", shifts=True):
        if not shifts:
            raise ValueError("SceneVotes: a SceneShiftVotes has shifts; SceneVotes(..., shifts=False) is the object without")
        super().__init__(n_points, classes, device, True)

    def add(self, logits, idx, shift=None):
        if shift is None:
            raise ValueError("SceneVotes.add: this object was built with shifts=True: add(logits, idx, shift) needs the shift rows [m, 3]")
        _gpu(shift, "SceneVotes.add: shift")
        logits, idx = self._rows(logits, idx)
        if shift.dim() != 2 or shift.shape != (logits.shape[0], 3) or shift.dtype not in _lib.ROW_TYPES:
            raise ValueError(f"SceneVotes.add: shift must be [{logits.shape[0]}, 3] float32 / float16 / bfloat16, got {shift.dtype} {tuple(shift.shape)}")
        if shift.device != self.pred.device:
            raise RuntimeError(f"SceneVotes.add: shift on {shift.device}, the votes on {self.pred.device}")
        shift = shift.detach().contiguous()
        n_points, classes = self.pred.shape
        _lib.call("pointops2_evaltile_vote_shift_launcher", logits.shape[0], classes, n_points, _lib.ROW_TYPES[logits.dtype], ptr(logits),
                  _lib.ROW_TYPES[shift.dtype], ptr(shift), ptr(idx), ptr(self._stamp), ptr(self.pred), ptr(self.shift), ptr(self._status),
                  device=self.pred.device)


def intersection_and_union(output, target, K, ignore_index=255):
    """util/common_util.py:45-57 with torch.bincount: (area_intersection, area_union, area_target), int64 [K], equal to the numpy
    original count for count (np.histogram's last bin is closed: a value K counts in bin K-1).  `output` is NOT written (the
    reference's GPU form at :66 overwrites it).  Integer tensors of one shape, on any one device (no kernel of this package runs)."""
    if output.shape != target.shape:
        raise ValueError(f"intersection_and_union: output {tuple(output.shape)} and target {tuple(target.shape)} differ in shape")
    if output.is_floating_point() or target.is_floating_point() or output.device != target.device:
        raise ValueError("intersection_and_union: output and target must be integer tensors on one device")
    K = int(K)
    target = target.reshape(-1).long()
    output = torch.where(target == ignore_index, torch.full_like(target, ignore_index), output.reshape(-1).long())

    def area(x):
        count = torch.bincount(x[(x >= 0) & (x <= K)], minlength=K + 1)
        count[K - 1] += count[K]
        return count[:K]
    inter, out, tgt = area(output[output == target]), area(output), area(target)
    return inter, out + tgt - inter, tgt


def _normalize(coord, feat, feat_div):
    """input_normalize (test_backup.py:191-196) and the casts of :260-261: minimum and division in the arrays' dtype, then fp32"""
    coord = coord - coord.min(0)[0]
    if feat_div:  # a true division (dataprep.data_prepare): on the GPU `tensor / python scalar` multiplies by the reciprocal instead
        if not feat.is_floating_point():
            feat = feat.double()   # numpy: integer array / 255. is float64
        feat = torch.div(feat, torch.tensor(float(feat_div), dtype=feat.dtype, device=feat.device))
    return coord.float(), feat.float()


def scene_eval(model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors=34, batch_size_test=5, feat_div=255.0,
               concat_xyz=False, priority=None):
    """test_backup.py:230-283 for ONE test-time transform: the normalised votes pred [N, classes] fp32 of a whole scene.
    coord [N,3] f32 / f64 and feat [N,C] on the GPU.  The scene is shifted to its minimum and split by scene_parts (:179-187); a part
    larger than voxel_max is tiled by crop_cover, a smaller one used as a whole (:238-254); every crop is normalised (minimum
    subtracted, feat / feat_div - None for ScanNet -, fp32); batches of `batch_size_test` consecutive crops ACROSS parts (:255-262:
    offset = cumulative sizes int32, batch = per-point element id int64) go through
        model_fn(feat, coord, offset, batch, neighbor_idx)      neighbor_idx = pointops.ball_query(2.5 * grid_size, max_num_neighbors, ...)[0]
    under torch.no_grad() (a tuple result: its first element - the fork returns (out, shift)), and SceneVotes.add collects
    softmax(logits).  priority: one float64 [n_part] tensor per part (or None), replaying the draws of :239.
    The caller sums the result over its transforms, takes the arg-max and calls intersection_and_union."""
    return _scene_votes("scene_eval", False, model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors, batch_size_test,
                        feat_div, concat_xyz, priority).result()


def _scene_votes(who, shifts, model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors, batch_size_test, feat_div,
                 concat_xyz, priority):
    """the tiling, normalisation, batching and ball_query that scene_eval and scene_predict share -> the filled SceneVotes.
    shifts False: model_fn's logits (a tuple result: its first element) are voted; True: model_fn must return (logits, shift)."""
    coord = _coord(coord)
    _gpu(feat, f"{who}: feat")
    if feat.dim() != 2 or feat.shape[0] != coord.shape[0] or feat.device != coord.device:
        raise ValueError(f"{who}: feat must be [{coord.shape[0]}, C] on {coord.device}, got {tuple(feat.shape)} on {feat.device}")
    if int(batch_size_test) < 1:
        raise ValueError(f"{who}: batch_size_test must be >= 1")
    dev = coord.device
    votes = SceneVotes(coord.shape[0], classes, dev, shifts)
    if voxel_size:
        coord = coord - coord.min(0)[0]
    parts = scene_parts(coord, voxel_size)
    if priority is not None and len(priority) != parts.shape[0]:
        raise ValueError(f"{who}: {len(priority)} priorities for {parts.shape[0]} parts")
    items = []   # (idx, coord, feat) of every crop, in the order of idx_list
    for i in range(parts.shape[0]):
        idx_part = parts[i]
        coord_part, feat_part = coord[idx_part], feat[idx_part]
        if voxel_max and idx_part.shape[0] > voxel_max:
            crops = crop_cover(coord_part, voxel_max, None if priority is None else priority[i])[0]
            for crop in crops:
                items.append((idx_part[crop],) + _normalize(coord_part[crop], feat_part[crop], feat_div))
        else:
            items.append((idx_part,) + _normalize(coord_part, feat_part, feat_div))
    step = int(batch_size_test)
    with torch.no_grad():
        for s in range(0, len(items), step):
            chunk = items[s:s + step]
            sizes = torch.tensor([c[0].shape[0] for c in chunk])
            idx_b, coord_b, feat_b = (torch.cat([c[k] for c in chunk]) for k in range(3))
            offset = torch.cumsum(sizes, 0).to(torch.int32).to(dev)
            batch = torch.repeat_interleave(torch.arange(len(chunk)), sizes).to(dev)
            neighbor_idx = pointops.ball_query(2.5 * grid_size, max_num_neighbors, coord_b, coord_b, offset, offset)[0]
            if concat_xyz:
                feat_b = torch.cat([feat_b, coord_b], 1)
            out = model_fn(feat_b, coord_b, offset, batch, neighbor_idx)
            if shifts:
                if not isinstance(out, (tuple, list)) or len(out) != 2:
                    raise TypeError(f"{who}: model_fn must return the pair (logits, shift), got {type(out).__name__}"
                                    + (f" of {len(out)}" if isinstance(out, (tuple, list)) else ""))
                votes.add(out[0], idx_b, out[1])
            else:
                votes.add(out[0] if isinstance(out, (tuple, list)) else out, idx_b)
    return votes


def scene_predict(model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors=34, batch_size_test=5, feat_div=255.0,
                  concat_xyz=False, priority=None):
    """The fork's test loop up to its two accumulators (test_iou.py:266-338; the same lines in test.py), on the device:
    -> (votes float32 [N, classes], shift float32 [N, 3]).  Tiling, normalisation, batching and ball_query are scene_eval's, argument for
    argument; model_fn(feat, coord, offset, batch, neighbor_idx) must return the pair (logits [m, classes], shift [m, 3]), each f32 / f16 /
    bf16 - anything else raises TypeError.  Per batch `pred[idx, :] += softmax(logits)` and `pred_shift[idx, :] += shift` (:337-338), both
    with SceneVotes' last-writer rule inside a batch.

    The votes are RAW: the fork has the normalisation of :340 commented out and takes `pred.max(1)[1]` of the sums (:343).
    Kept quirk: the shift of a point that k batches visited is the SUM of its k predictions, not their mean - the fork adds `pred_shift`
    to the coordinates as it is (:344, :356), so a point in two overlapping crops moves by both predictions."""
    votes = _scene_votes("scene_predict", True, model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors,
                         batch_size_test, feat_div, concat_xyz, priority)
    votes._check()
    return votes.pred, votes.shift


def dense_points(coord, eps=0.1, min_samples=5, min_points=50):
    """The loader's outlier filter (test_iou.py:147-151, test.py:122): one DBSCAN of the whole scene; the clusters with MORE than
    min_points points are kept, concatenated cluster by cluster; noise is dropped.  coord [N, 3] f32 / f64 on the GPU (clustered in fp32
    by cluster.dbscan) -> (coord_kept [K, 3] in coord's dtype, index int64 [K] into coord: ascending cluster number, then ascending
    original index - the reference's order).  N = 0: nothing is launched; nothing kept: empty tensors."""
    coord = _coord(coord)
    if isinstance(min_points, bool) or not isinstance(min_points, int) or min_points < 0:
        raise ValueError(f"dense_points: min_points must be an int >= 0, got {min_points!r}")
    none = torch.empty(0, dtype=torch.int64, device=coord.device)
    if coord.shape[0] == 0:
        cluster.dbscan_settings(eps, min_samples, 1)
        return coord[:0], none
    labels, _, n_clusters = cluster.dbscan(coord.float(), eps, min_samples)
    if int(n_clusters.sum().item()) == 0:
        return coord[:0], none
    labels = labels.long()
    size = torch.bincount(labels[labels >= 0])
    kept = torch.nonzero((labels >= 0) & (size[labels.clamp(min=0)] > min_points)).flatten()      # ascending original index
    if kept.numel() == 0:
        return coord[:0], none
    index = kept[torch.sort(labels[kept], stable=True)[1]]
    return coord[index], index


DetectedScene = collections.namedtuple("DetectedScene", ["boxes", "label", "shift", "points", "merged", "n_sets", "score"])


def detect_scene(model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors=34, batch_size_test=5, feat_div=255.0,
                 concat_xyz=False, priority=None, gt_box=None, overlap_threshold=0.25, **cluster_settings):
    """The fork's detection pass for one scene (test_iou.py:266-464) in one call on device tensors:
        scene_predict -> label = arg-max of the raw votes (:343), shift = the summed shifts
        cluster.detect_boxes(coord.float(), shift, label, **cluster_settings)     instantiation_eval (:356) and the merging loop (:373-422)
        cluster.box_detection(boxes, gt_box, overlap_threshold)                   when gt_box is given; 0.25 is the fork's (:268)
    The arguments up to `priority` are scene_predict's; cluster_settings are detect_boxes' keywords.
    -> DetectedScene(boxes float32 [S, 6] = lo | hi, label int64 [N], shift float32 [N, 3], points float32 [K, 3]: the cleaned support
       points, merged int32 [K]: the merged set (= row of boxes) of every support point, n_sets = S, score: box_detection's tuple or None).

    Two departures from the fork.  It subtracts the minimum before the loop and adds it back (:344), so it detects on
    `(coord - min) + min` in the array's dtype; here detection runs on the original coordinates cast to fp32.  And it `return`s from
    its whole test function when instantiation_eval finds fewer than two supports (:357-358); here the boxes of the zero or one
    supports are returned (and scored)."""
    cluster.detect_settings(**cluster_settings)              # a wrong setting raises before the scene goes through the model
    votes, shift = scene_predict(model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors, batch_size_test, feat_div,
                                 concat_xyz, priority)
    label = votes.max(1)[1]
    boxes, points, merged, n_sets, _, _ = cluster.detect_boxes(coord.float(), shift, label, **cluster_settings)
    score = None if gt_box is None else cluster.box_detection(boxes, gt_box, overlap_threshold)
    return DetectedScene(boxes, label, shift, points, merged, n_sets, score)
