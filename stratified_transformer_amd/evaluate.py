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

Not covered: the test-time transforms (host numpy callables; the caller sums scene_eval over them), file reading / writing, the
meters and the logging, and the fork's DCF evaluation."""
import torch

from . import _lib, pointops
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
    with torch.cuda.device(dev):
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
    logits [m, classes] f32 / f16 / bf16 (arithmetic fp32), idx int64 [m], on the GPU.  result(): pred / (pred.sum(-1)[:, None] + 1e-8)."""

    def __init__(self, n_points, classes, device="cuda"):
        n_points, classes = int(n_points), int(classes)
        if n_points < 1 or not 1 <= classes <= MAX_CLASSES:
            raise ValueError(f"SceneVotes: need n_points >= 1 and 1 <= classes <= {MAX_CLASSES}, got {n_points}, {classes}")
        self.pred = torch.zeros(n_points, classes, dtype=torch.float32, device=device)
        self._stamp = torch.full((n_points,), -1, dtype=torch.int32, device=device)   # largest row number per point inside a call
        self._status = torch.zeros(1, dtype=torch.int32, device=device)

    def add(self, logits, idx):
        _gpu(logits, "SceneVotes.add: logits")
        _gpu(idx, "SceneVotes.add: idx")
        n_points, classes = self.pred.shape
        if logits.dim() != 2 or logits.shape[1] != classes or logits.dtype not in _lib.ROW_TYPES:
            raise ValueError(f"SceneVotes.add: logits must be [m, {classes}] float32 / float16 / bfloat16, got {logits.dtype} {tuple(logits.shape)}")
        if idx.dtype != torch.int64 or idx.shape != (logits.shape[0],):
            raise ValueError(f"SceneVotes.add: idx must be int64 [{logits.shape[0]}], got {idx.dtype} {tuple(idx.shape)}")
        if logits.device != self.pred.device or idx.device != self.pred.device:
            raise RuntimeError(f"SceneVotes.add: logits on {logits.device}, idx on {idx.device}, the votes on {self.pred.device}")
        logits, idx = logits.detach().contiguous(), idx.contiguous()
        with torch.cuda.device(self.pred.device):
            _lib.call("pointops2_evaltile_vote_launcher", logits.shape[0], classes, n_points, _lib.ROW_TYPES[logits.dtype], ptr(logits), ptr(idx),
                      ptr(self._stamp), ptr(self.pred), ptr(self._status), device=self.pred.device)

    def result(self):
        if int(self._status.item()) != 0:
            raise IndexError(f"SceneVotes: an index given to add() was outside [0, {self.pred.shape[0]})")
        return self.pred / (self.pred.sum(-1)[:, None] + 1e-8)


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
    coord = _coord(coord)
    _gpu(feat, "scene_eval: feat")
    if feat.dim() != 2 or feat.shape[0] != coord.shape[0] or feat.device != coord.device:
        raise ValueError(f"scene_eval: feat must be [{coord.shape[0]}, C] on {coord.device}, got {tuple(feat.shape)} on {feat.device}")
    if int(batch_size_test) < 1:
        raise ValueError("scene_eval: batch_size_test must be >= 1")
    dev = coord.device
    votes = SceneVotes(coord.shape[0], classes, dev)
    if voxel_size:
        coord = coord - coord.min(0)[0]
    parts = scene_parts(coord, voxel_size)
    if priority is not None and len(priority) != parts.shape[0]:
        raise ValueError(f"scene_eval: {len(priority)} priorities for {parts.shape[0]} parts")
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
            votes.add(out[0] if isinstance(out, (tuple, list)) else out, idx_b)
    return votes.result()
