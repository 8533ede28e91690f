"""numpy restatement of the reference's whole-scene evaluation, the oracle of stratified_transformer_amd.evaluate:

    scene_parts             test_backup.py:179-185   the voxel-round-robin parts from voxelize(mode=1)'s (idx_sort, count)
    crop_cover              test_backup.py:238-251   the tiling loop of one part
    votes_add, votes_result test_backup.py:278-283   pred[idx, :] += softmax(logits, -1); pred / (pred.sum(-1)[:, None] + 1e-8)
    intersection_and_union  util/common_util.py:45-57
    scene_eval              test_backup.py:230-283   all of it for one transform, the model a numpy callable

PARITY UNPINNED for the tiling loop and the vote: they sit inline in the reference's test(), between the file reading and the model
call, and cannot be executed on their own - they are restated here line by line.  scene_parts is pinned: tests/golden/voxelize_crop.npz
holds the (idx_sort, count) that executing util/voxelize.py produced, and :182-185 are three lines of integer arithmetic on them.

Two places where the reference leaves the result open are pinned the way the device code pins them:
  - np.argsort (:243) is unstable: among equal distances any order is a valid output.  kind="stable" (ascending index), as
    oracle/index_ref.py does for crop_nearest; stable=False gives numpy's default for the tie-free comparison.
  - `pred[idx_part, :] += pred_part` (:281) with a repeated index is an indexed assignment: ONE of the rows writes.  CPU torch lets
    the last one write; votes_add is that sequential loop.
The votes are kept in float64 (softmax in float64 of the logits as given): the device's fp32 is measured against it, with
vote_tolerance() as the bound.
"""
import numpy as np


def room(n, seed):
    """the test clouds: a 4 x 3 x 2.5 room, the first half of the points on its floor (z in [0, 0.02)) -> (coord f64 [n,3], priority)"""
    rng = np.random.default_rng(seed)
    coord = rng.uniform(0, 1, (n, 3)) * np.array([4, 3, 2.5])
    coord[: n // 2, 2] = rng.uniform(0, 0.02, n // 2)
    return coord, rng.random(n) * 1e-3


def lattice(seed=1, shape=(16, 16, 8), step=0.04):
    """a shuffled lattice: equal distances everywhere -> (coord f64 [prod(shape),3], priority)"""
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3) * step
    return grid[rng.permutation(len(grid))], rng.random(len(grid)) * 1e-3


def eval_scene(dtype, n=6000, seed=4, classes=13):
    """the end-to-end scene: room(n) in `dtype`, rgb features 0..255, the weights [6, classes] of the linear stand-in model"""
    coord = room(n, seed)[0].astype(dtype)
    rng = np.random.default_rng(seed + 102)
    feat = rng.integers(0, 256, (n, 3)).astype(dtype)
    weights = rng.standard_normal((6, classes)) * np.array([4.0, 4.0, 4.0, 0.25, 0.25, 0.25])[:, None]
    return coord, feat, weights


def linear_model(weights):
    """model_fn of the end-to-end test: logits = [feat, coord] @ weights, evaluated column by column in float64 (one multiply and one
    add per step, the same steps as the torch twin in tests/test_evaltile_hip.py: identical logits), rounded to fp32"""
    def model_fn(feat, coord, offset, batch):
        x = np.concatenate([feat, coord], 1).astype(np.float64)
        logits = x[:, 0:1] * weights[0]
        for k in range(1, x.shape[1]):
            logits = logits + x[:, k:k + 1] * weights[k]
        return logits.astype(np.float32)
    return model_fn


def scene_parts(idx_sort, count, n_points=None):
    """:182-185 (idx_sort, count of voxelize(coord, voxel_size, mode=1)); idx_sort None: the single part of :187"""
    if idx_sort is None:
        return np.arange(n_points)[None]
    start = np.cumsum(np.insert(count, 0, 0)[0:-1])
    return np.stack([idx_sort[start + i % count] for i in range(count.max())]).astype(np.int64)


def squared_distance(coord, seed):
    """:242, in the array's dtype (np.power(x, 2) is x * x; a 3-element row is summed left to right)"""
    return np.sum(np.power(coord - coord[seed], 2), 1)


def crop_cover(coord, voxel_max, priority, stable=True):
    """:239-251 for one part with more than voxel_max points -> (crops [n_crops, voxel_max] i64, seeds [n_crops] i64, final priority).
    priority replays np.random.rand(n) * 1e-3 of :239.  ValueError where the reference would divide 0 / 0 and loop for ever."""
    n = coord.shape[0]
    assert n > voxel_max >= 1
    priority = np.array(priority, dtype=np.float64)
    covered = np.zeros(n, bool)                                      # :250 keeps np.unique of all indices seen; only its size is used
    crops, seeds = [], []
    while not covered.all():
        if len(crops) == n:
            raise RuntimeError("more crops than points")
        seed = int(np.argmin(priority))                              # :241
        dist = squared_distance(coord, seed)                         # :242
        crop = np.argsort(dist, kind="stable" if stable else None)[:voxel_max]   # :243
        dist = dist[crop]                                            # :245
        if np.max(dist) == 0:
            raise ValueError(f"the {voxel_max} points nearest to seed {seed} coincide with it")
        delta = np.square(1 - dist / np.max(dist))                   # :246, in coord's dtype
        assert delta.dtype == coord.dtype
        priority[crop] += delta                                      # :247
        covered[crop] = True
        crops.append(crop)
        seeds.append(seed)
    return np.stack(crops).astype(np.int64), np.array(seeds, np.int64), priority


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def votes_add(pred, logits, idx):
    """:278, :281 on pred float64 [n_points, classes], in place: every row computes pred[idx[r]] + softmax(logits[r]) from the values
    BEFORE the call, then the rows are assigned in order - the last row of a repeated index stays"""
    rows = pred[idx] + softmax64(logits)
    for r in range(len(idx)):
        pred[idx[r]] = rows[r]
    return pred


def votes_result(pred):
    """:283"""
    return pred / (pred.sum(-1)[:, None] + 1e-8)


def vote_tolerance(softmax_error):
    """Bound on |device votes - this oracle's|, for the votes and for the normalised result alike: twice the error that torch's own
    fp32 softmax has against softmax64 on the same device and logits (`softmax_error`, measured by the test).  Both are an fp32 exp
    and a sum of at most 64 terms; the votes of a point are a few such rows added in fp32 and are compared against the float64 sum."""
    return 2.0 * softmax_error


def intersection_and_union(output, target, K, ignore_index=255):
    """util/common_util.py:45-57: per-class areas of intersection, union and target; np.histogram's bins arange(K + 1)"""
    output, target = np.asarray(output).reshape(-1).copy(), np.asarray(target).reshape(-1)
    output[target == ignore_index] = ignore_index
    bins = np.arange(K + 1)
    area_i = np.histogram(output[output == target], bins=bins)[0]
    area_o = np.histogram(output, bins=bins)[0]
    area_t = np.histogram(target, bins=bins)[0]
    return area_i, area_o + area_t - area_i, area_t


def input_normalize(coord, feat, feat_div=255.0):
    """:191-196 and the FloatTensor casts of :260-261"""
    coord = coord - coord.min(0)
    if feat_div:
        feat = feat / feat_div
    return coord.astype(np.float32), feat.astype(np.float32)


def scene_eval(model_fn, coord, feat, voxelize, voxel_size, voxel_max, classes, batch_size_test=5, feat_div=255.0, concat_xyz=False,
               priority=None):
    """:230-283 for one transform.  voxelize(coord, voxel_size) -> (idx_sort, count) stands for util/voxelize.py's mode 1 (the tests
    pass oracle/index_ref.voxelize); model_fn(feat f32, coord f32, offset i32, batch i64) -> logits; priority: one array per part.
    -> (pred float64 [N, classes], the largest number of writes any point received, the number of crops)"""
    n = coord.shape[0]
    if voxel_size:
        coord = coord - coord.min(0)                                 # :179-180
        parts = scene_parts(*voxelize(coord, voxel_size))
    else:
        parts = scene_parts(None, None, n)
    items = []
    for i, idx_part in enumerate(parts):                             # :234-254
        coord_part, feat_part = coord[idx_part], feat[idx_part]
        if voxel_max and len(idx_part) > voxel_max:
            for crop in crop_cover(coord_part, voxel_max, priority[i])[0]:
                items.append((idx_part[crop],) + input_normalize(coord_part[crop], feat_part[crop], feat_div))
        else:
            items.append((idx_part,) + input_normalize(coord_part, feat_part, feat_div))
    pred, writes = np.zeros((n, classes)), np.zeros(n, np.int64)
    for s in range(0, len(items), batch_size_test):                  # :255-281
        chunk = items[s:s + batch_size_test]
        idx_b, coord_b, feat_b = (np.concatenate([c[k] for c in chunk]) for k in range(3))
        sizes = np.array([len(c[0]) for c in chunk])
        offset, batch = np.cumsum(sizes).astype(np.int32), np.repeat(np.arange(len(chunk)), sizes)
        if concat_xyz:
            feat_b = np.concatenate([feat_b, coord_b], 1)
        votes_add(pred, model_fn(feat_b, coord_b, offset, batch), idx_b)
        writes[np.unique(idx_b)] += 1
    return votes_result(pred), int(writes.max()), len(items)
