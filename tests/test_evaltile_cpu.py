"""CPU: the oracle of the whole-scene evaluation (tests/evaltile_oracle.py) on the clouds the GPU tests use - crop counts, where the
stable and numpy's default argsort agree and where they do not, the condition on the end-to-end scene - and the host side of
stratified_transformer_amd.evaluate: declarations, exports, argument checks, the missing CPU path.  No HIP compute runs here."""
import inspect
import os

import numpy as np
import pytest
import torch

import stratified_transformer_amd as sta
from oracle import index_ref
from stratified_transformer_amd import _lib, evaluate
from tests import evaltile_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# n, voxel_max, seed of O.room, crops (the same in f32 and f64)
ROOMS = [(3000, 512, 0, 14), (1500, 1024, 1, 4), (4097, 1000, 2, 9), (600, 599, 3, 2)]


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _duplicate_distances(coord, seeds):
    return sum(len(coord) - len(np.unique(O.squared_distance(coord, s))) for s in seeds)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,voxel_max,seed,n_crops", ROOMS)
def test_oracle_crop_counts_and_the_unstable_sort_on_tie_free_clouds(n, voxel_max, seed, n_crops, dtype):
    coord, priority = O.room(n, seed)
    coord = coord.astype(dtype)
    crops, seeds, final = O.crop_cover(coord, voxel_max, priority)
    assert crops.shape == (n_crops, voxel_max) and seeds.shape == (n_crops,)
    assert len(np.unique(crops)) == n and all(len(np.unique(c)) == voxel_max for c in crops)     # a cover; distinct inside a crop
    assert len(np.unique(seeds)) == n_crops and all(seeds[k] in crops[k] for k in range(n_crops))
    assert np.all(final >= priority) and np.all(final[seeds] >= 1.0)                            # a seed's own priority rises by exactly 1
    unstable = O.crop_cover(coord, voxel_max, priority, stable=False)
    if (n, dtype) == (4097, np.float32):      # equal fp32 distances: the two orders differ, the stable one is pinned
        assert _duplicate_distances(coord, seeds) > 0
        assert unstable[0].shape != crops.shape or not np.array_equal(unstable[0], crops)
    else:
        assert _duplicate_distances(coord, seeds) == 0
        assert all(np.array_equal(a, b) for a, b in zip(unstable, (crops, seeds, final)))
    if n == 600:                              # the second seed is a point the first crop already covered
        assert seeds[1] in crops[0]
    if n == 4097:                             # more than one argmin workgroup (1024 points each)
        assert n > 4 * 1024


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_oracle_on_the_lattice_ties_everywhere(dtype):
    coord, priority = O.lattice()
    coord = coord.astype(dtype)
    assert coord.shape == (2048, 3)
    crops, seeds, _ = O.crop_cover(coord, 500, priority)
    assert crops.shape == (11, 500)
    assert all(len(np.unique(O.squared_distance(coord, s))) < 1024 for s in seeds)   # most distances occur more than once
    unstable = O.crop_cover(coord, 500, priority, stable=False)[0]
    assert unstable.shape != crops.shape or not np.array_equal(unstable, crops)


def test_oracle_distance_is_the_left_to_right_sum():
    for dtype in (np.float32, np.float64):
        coord = O.room(4097, 2)[0].astype(dtype)
        d = coord - coord[17]
        sq = d * d
        assert np.array_equal(O.squared_distance(coord, 17), (sq[:, 0] + sq[:, 1]) + sq[:, 2])


def test_oracle_refuses_coincident_points_and_takes_index_0_of_equal_priorities():
    coord = np.concatenate([np.full((513, 3), 0.5), O.room(1000, 6)[0]]).astype(np.float32)
    priority = np.full(len(coord), 1e-4)
    priority[100] = 0.0
    with pytest.raises(ValueError, match="seed 100"):
        O.crop_cover(coord, 512, priority)
    coord = O.room(1500, 1)[0]
    assert O.crop_cover(coord, 1024, np.zeros(1500))[1][0] == 0


def test_oracle_vote_is_cpu_torchs_indexed_assignment():
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 40, 200)
    logits = rng.standard_normal((200, 5)).astype(np.float32)
    pred = O.votes_add(np.zeros((60, 5)), logits, idx)
    t = torch.zeros(60, 5, dtype=torch.float64)
    t[torch.from_numpy(idx), :] += torch.softmax(torch.from_numpy(logits).double(), -1)      # test_backup.py:278, :281
    assert np.allclose(pred, t.numpy(), rtol=0, atol=1e-15)
    last = {int(i): r for r, i in enumerate(idx)}
    for i, r in last.items():
        assert np.array_equal(pred[i], O.softmax64(logits[r]))
    assert np.all(pred[[i for i in range(60) if i not in last]] == 0)
    assert O.vote_tolerance(1e-7) == 2e-7


def test_oracle_scene_parts_on_the_reference_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "voxelize_crop.npz"))
    for tag in ("f64", "f32"):
        idx_sort, count = g[f"{tag}_val_idx_sort"], g[f"{tag}_val_count"]
        parts = O.scene_parts(idx_sort, count)
        assert parts.shape == (count.max(), len(count)) and parts.dtype == np.int64
        start = np.cumsum(count) - count
        assert np.array_equal(parts[0], idx_sort[start])
        assert np.array_equal(np.unique(parts), np.arange(len(idx_sort)))                        # every point is in some part
        v = int(np.argmax(count))
        assert np.array_equal(parts[:, v], idx_sort[start[v]:start[v] + count[v]])               # the fullest voxel: one point per part
    assert np.array_equal(O.scene_parts(None, None, 7), np.arange(7)[None])


def test_end_to_end_scene_meets_its_condition_under_the_oracle_alone():
    """the GPU test compares labels only where the oracle's top-two margin exceeds the tolerance, and at most 1 % of the points may be
    left out that way: shown here for a tolerance of 1e-4, far above anything tests/test_evaltile_hip.py can arrive at (it asserts so)"""
    for dtype in (np.float64, np.float32):
        coord, feat, weights = O.eval_scene(dtype)
        rng = np.random.default_rng(7)
        parts = O.scene_parts(*index_ref.voxelize(coord - coord.min(0), 0.04, 1))
        assert parts.shape[0] >= 3 and parts.shape[1] > 1500
        priority = [rng.random(parts.shape[1]) * 1e-3 for _ in parts]
        pred, writes, n_crops = O.scene_eval(O.linear_model(weights), coord, feat, lambda c, v: index_ref.voxelize(c, v, 1), 0.04, 1500, 13,
                                             priority=priority)
        assert pred.shape == (6000, 13) and np.allclose(pred.sum(-1), 1.0) and n_crops > 5 * parts.shape[0] > writes >= 2
        top = np.sort(pred, 1)
        assert np.mean(top[:, -1] - top[:, -2] <= 1e-4) <= 0.01
        assert (np.bincount(pred.argmax(1), minlength=13) > 0).sum() >= 5                        # not one label everywhere
        assert O.vote_tolerance(1e-6) < 1e-4


@pytest.mark.parametrize("K,ignore", [(13, 255), (4, -1)])
def test_intersection_and_union_is_the_numpy_originals(K, ignore):
    rng = np.random.default_rng(K)
    target = rng.integers(0, K, 5000)
    target[target == 2] = 1                                      # class 2 is absent from the target ...
    output = rng.integers(0, K, 5000)
    output[output == 3] = 0                                      # ... and class 3 from the output
    target[rng.random(5000) < 0.1] = ignore
    want = O.intersection_and_union(output, target, K, ignore)
    out_t = torch.from_numpy(output)
    got = evaluate.intersection_and_union(out_t, torch.from_numpy(target), K, ignore)
    assert np.array_equal(out_t.numpy(), output)                 # not written (util/common_util.py:66 overwrites its argument)
    for a, b in zip(got, want):
        assert a.dtype == torch.int64 and np.array_equal(a.numpy(), b)
    assert want[2][2] == 0 and want[0][3] == 0 and want[1].sum() > 0
    got2 = evaluate.intersection_and_union(out_t.reshape(50, 100).int(), torch.from_numpy(target).reshape(50, 100), K, ignore)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(got2, want))
    with pytest.raises(ValueError):
        evaluate.intersection_and_union(out_t, torch.from_numpy(target)[:-1], K, ignore)
    with pytest.raises(ValueError):
        evaluate.intersection_and_union(out_t.float(), torch.from_numpy(target), K, ignore)


def test_launchers_are_declared_and_exported():
    assert _lib.RESULTS["pointops2_evaltile_max_parts"] == ([], _lib.I)
    assert _lib.lib().pointops2_evaltile_max_parts() >= 64
    assert "evaltile.hip" in open(os.path.join(ROOT, "stratified_transformer_amd", "csrc", "Makefile")).read()


def test_public_interface():
    assert sta.scene_eval is evaluate.scene_eval and "scene_eval" in sta.__all__
    assert str(inspect.signature(evaluate.scene_eval)) == ("(model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors=34, "
                                                           "batch_size_test=5, feat_div=255.0, concat_xyz=False, priority=None)")
    assert str(inspect.signature(evaluate.scene_parts)) == "(coord, voxel_size)"
    assert str(inspect.signature(evaluate.crop_cover)) == "(coord, voxel_max, priority=None)"
    assert str(inspect.signature(evaluate.intersection_and_union)) == "(output, target, K, ignore_index=255)"
    assert list(inspect.signature(evaluate.SceneVotes.add).parameters) == ["self", "logits", "idx"]
    assert "accumulate" not in inspect.signature(evaluate.SceneVotes.__init__).parameters    # the last-writer vote is the only mode


def test_cpu_tensors_raise_no_cpu_fallback():
    coord, feat = torch.rand(100, 3), torch.rand(100, 3)
    calls = _lib.CALLS[0]
    for fn in (lambda: evaluate.scene_parts(coord, 0.04), lambda: evaluate.scene_parts(coord, None), lambda: evaluate.crop_cover(coord, 50),
               lambda: evaluate.scene_eval(lambda *a: None, coord, feat, 0.04, 50, 13, 0.04),
               lambda: evaluate.scene_eval(lambda *a: None, _OnGpu(coord), feat, 0.04, 50, 13, 0.04),
               lambda: evaluate.crop_cover(_OnGpu(coord), 50, torch.zeros(100, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            fn()
    votes = evaluate.SceneVotes(100, 13, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        votes.add(torch.zeros(10, 13), torch.zeros(10, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        votes.add(_OnGpu(torch.zeros(10, 13)), torch.zeros(10, dtype=torch.int64))
    assert _lib.CALLS[0] == calls


F64 = torch.float64


@pytest.mark.parametrize("coord,voxel_max,priority,error", [
    (torch.zeros(100, 2), 50, None, RuntimeError),                                      # coord not [n, 3]
    (torch.zeros(300), 50, None, RuntimeError),
    (torch.zeros(100, 3, dtype=torch.float16), 50, None, RuntimeError),                 # coord dtype
    (torch.zeros(100, 3), 100, None, ValueError),                                       # n <= voxel_max: the part is used as a whole
    (torch.zeros(100, 3), 200, None, ValueError),
    (torch.zeros(100, 3), 0, None, ValueError),
    (torch.zeros(100, 3), 50, torch.zeros(100), ValueError),                            # priority dtype
    (torch.zeros(100, 3), 50, torch.zeros(99, dtype=F64), ValueError),                  # priority not [n]
    (torch.zeros(100, 3), 50, torch.zeros(100, 1, dtype=F64), ValueError),
])
def test_crop_cover_rejects_bad_arguments_before_any_launch(coord, voxel_max, priority, error):
    calls = _lib.CALLS[0]
    with pytest.raises(error):
        evaluate.crop_cover(_OnGpu(coord), voxel_max, None if priority is None else _OnGpu(priority))
    assert _lib.CALLS[0] == calls


def test_votes_reject_bad_arguments_before_any_launch():
    calls = _lib.CALLS[0]
    for n_points, classes in ((0, 13), (100, 0), (100, 65)):
        with pytest.raises(ValueError, match="SceneVotes"):
            evaluate.SceneVotes(n_points, classes, device="cpu")
    votes = evaluate.SceneVotes(100, 13, device="cpu")
    idx = _OnGpu(torch.zeros(10, dtype=torch.int64))
    for logits, ix in ((torch.zeros(10, 12), idx), (torch.zeros(10, 13, dtype=F64), idx), (torch.zeros(130), idx),
                       (torch.zeros(10, 13), _OnGpu(torch.zeros(10, dtype=torch.int32))), (torch.zeros(10, 13), _OnGpu(torch.zeros(9, dtype=torch.int64)))):
        with pytest.raises(ValueError, match="SceneVotes.add"):
            votes.add(_OnGpu(logits), ix)
    assert _lib.CALLS[0] == calls and votes.result().shape == (100, 13) and float(votes.result().abs().max()) == 0.0
