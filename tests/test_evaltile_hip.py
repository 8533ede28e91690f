"""GPU: stratified_transformer_amd.evaluate (csrc/evaltile.hip) against the numpy oracle tests/evaltile_oracle.py.
crop_cover: crops, seeds and the final float64 priority bit for bit, in f32 and f64.  Votes: the last row of a repeated index writes;
values within twice the error that torch's own fp32 softmax has on the same device and logits against a float64 softmax (measured
in the test and printed: O.vote_tolerance)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import index_ref
from stratified_transformer_amd import _lib, evaluate
from tests import evaltile_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP = {"f32": np.float32, "f64": np.float64}
# name -> (cloud, voxel_max, crops the oracle needs)
CLOUDS = {"room3000": (lambda: O.room(3000, 0), 512, 14), "room1500": (lambda: O.room(1500, 1), 1024, 4),
          "room4097": (lambda: O.room(4097, 2), 1000, 9), "room600": (lambda: O.room(600, 3), 599, 2), "lattice2048": (O.lattice, 500, 11)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def cover_case(name, tag):
    """(coord, priority, voxel_max, the oracle's (crops, seeds, final priority)), computed once"""
    make, voxel_max, n_crops = CLOUDS[name]
    coord, priority = make()
    coord = coord.astype(NP[tag])
    want = O.crop_cover(coord, voxel_max, priority)
    assert len(want[0]) == n_crops
    return coord, priority, voxel_max, want


def check_cover(coord, priority, voxel_max, want):
    p_dev = dev(priority)
    crops, seeds, final = evaluate.crop_cover(dev(coord), voxel_max, p_dev)
    assert crops.dtype == torch.int64 and seeds.dtype == torch.int64 and final.dtype == torch.float64
    assert crops.shape == want[0].shape and np.array_equal(host(crops), want[0])
    assert np.array_equal(host(seeds), want[1])
    assert np.array_equal(host(final).view(np.uint64), want[2].view(np.uint64))                 # float64, bit for bit
    assert np.array_equal(host(p_dev), priority)                                                # the caller's tensor is not written
    assert evaluate.LAST == {"crops": len(want[0]), "reads": len(want[0])}                      # one read-back per crop


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("name", list(CLOUDS))
def test_crop_cover_is_the_oracles_bit_for_bit(name, tag):
    coord, priority, voxel_max, want = cover_case(name, tag)
    if name == "room4097":
        assert len(coord) > 4 * 1024                                                            # several argmin workgroups
    if name == "room600":
        assert want[1][1] in want[0][0]                                                         # the second seed is already covered
    if (name, tag) == ("room4097", "f32") or name == "lattice2048":                             # equal distances: the stable order decides
        unstable = O.crop_cover(coord, voxel_max, priority, stable=False)[0]
        assert unstable.shape != want[0].shape or not np.array_equal(unstable, want[0])
    check_cover(coord, priority, voxel_max, want)


def test_crop_cover_many_partials():
    coord, priority = O.room(70000, 5)
    coord = coord.astype(np.float32)
    want = O.crop_cover(coord, 20000, priority)
    assert 70000 > 64 * 1024 and len(want[0]) >= 4                                              # more pairs than one wave reduces
    check_cover(coord, priority, 20000, want)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_crop_cover_equal_priorities_start_at_index_0(tag):
    coord = O.room(1500, 1)[0].astype(NP[tag])
    priority = np.zeros(1500)
    want = O.crop_cover(coord, 1024, priority)
    assert want[1][0] == 0
    check_cover(coord, priority, 1024, want)
    assert int(evaluate.crop_cover(dev(coord), 1024)[0].shape[1]) == 1024                       # a priority drawn on the device


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_crop_cover_refuses_coincident_points(tag):
    voxel_max = 512
    coord = np.concatenate([np.full((voxel_max + 1, 3), 0.5), O.room(1000, 6)[0]]).astype(NP[tag])
    priority = np.full(len(coord), 1e-4)
    priority[100] = 0.0
    with pytest.raises(ValueError):
        O.crop_cover(coord, voxel_max, priority)
    p_dev = dev(priority)
    with pytest.raises(ValueError, match=r"seed point 100 .*0 of 1513 points covered"):
        evaluate.crop_cover(dev(coord), voxel_max, p_dev)
    assert np.array_equal(host(p_dev), priority)
    # the kernel itself writes nothing in that case: priority, covered flags and count stay
    n = len(coord)
    c_dev, prio, covered, report = dev(coord), dev(priority), torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    dist = torch.empty(n, dtype=c_dev.dtype, device="cuda")
    parts = _lib.lib().pointops2_evaltile_max_parts()
    pv, pi, seed = torch.empty(parts, dtype=torch.float64, device="cuda"), torch.empty(parts, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    _lib.call("pointops2_evaltile_seed_dist_launcher", n, int(tag == "f64"), c_dev.data_ptr(), prio.data_ptr(), pv.data_ptr(), pi.data_ptr(), seed.data_ptr(),
              dist.data_ptr(), device=c_dev.device)
    crop = torch.sort(dist, stable=True)[1][:voxel_max].clone()
    _lib.call("pointops2_evaltile_update_launcher", n, voxel_max, int(tag == "f64"), dist.data_ptr(), crop.data_ptr(), prio.data_ptr(), covered.data_ptr(),
              report.data_ptr(), device=c_dev.device)
    assert int(seed) == 100 and report.tolist() == [0, evaluate.STATUS_DMAX_ZERO]
    assert np.array_equal(host(prio), priority) and int(covered.sum()) == 0
    # voxel_max - 1 coincident points: the crop's farthest point is a real neighbour, and the loop runs as the oracle's
    check_cover(coord[2:], priority[2:], voxel_max, O.crop_cover(coord[2:], voxel_max, priority[2:]))


def test_launchers_record_bad_sizes_before_any_launch():
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    for name, args in (("pointops2_evaltile_seed_dist_launcher", (0, 0, p, p, p, p, p, p)), ("pointops2_evaltile_seed_dist_launcher", (4, 0, p, None, p, p, p, p)),
                       ("pointops2_evaltile_update_launcher", (4, 5, 0, p, p, p, p, p)), ("pointops2_evaltile_update_launcher", (4, 0, 0, p, p, p, p, p)),
                       ("pointops2_evaltile_vote_launcher", (4, 65, 4, 0, p, p, p, p, p)), ("pointops2_evaltile_vote_launcher", (4, 4, 0, 0, p, p, p, p, p)),
                       ("pointops2_evaltile_vote_launcher", (4, 4, 4, 3, p, p, p, p, p)), ("pointops2_evaltile_vote_launcher", (4, 4, 4, 0, p, p, None, p, p))):
        with pytest.raises(RuntimeError, match="evaltile"):
            _lib.call(name, *args, device=t.device)
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_scene_parts_on_the_reference_golden(tag):
    g = np.load(os.path.join(ROOT, "tests", "golden", "voxelize_crop.npz"))
    coord = g[f"{tag}_coord"]
    coord = coord - coord.min(0)
    idx_sort, count = index_ref.voxelize(coord, 0.04, 1)
    want = O.scene_parts(idx_sort, count)
    if np.array_equal(coord, g[f"{tag}_coord"]):                                                # (the golden cloud starts at its minimum)
        assert np.array_equal(idx_sort, g[f"{tag}_val_idx_sort"]) and np.array_equal(count, g[f"{tag}_val_count"])
    parts = evaluate.scene_parts(dev(coord), 0.04)
    assert parts.dtype == torch.int64 and parts.shape == want.shape and np.array_equal(host(parts), want)
    # and from the recorded arrays themselves, on the unshifted cloud they were recorded for
    parts = evaluate.scene_parts(dev(g[f"{tag}_coord"]), 0.04)
    assert np.array_equal(host(parts), O.scene_parts(g[f"{tag}_val_idx_sort"], g[f"{tag}_val_count"]))
    row = evaluate.scene_parts(dev(coord), None)
    assert row.dtype == torch.int64 and np.array_equal(host(row), np.arange(len(coord))[None])


def softmax_error(logits):
    """torch's own fp32 softmax on the device against the float64 softmax of the same logits (CPU): the yardstick of the vote"""
    got = host(torch.softmax(logits.float(), -1)).astype(np.float64)
    return float(np.abs(got - O.softmax64(host(logits.float()))).max())


TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def vote_inputs(rng, n_points, m, classes, dtype):
    """m rows; half of the points are hit once, the other half share the remaining rows (about four rows each), in random order"""
    perm = rng.permutation(n_points)
    idx = np.concatenate([perm[: n_points // 2], rng.choice(perm[n_points // 2:], m - n_points // 2)])
    idx = idx[rng.permutation(m)].astype(np.int64)
    logits = torch.from_numpy(rng.standard_normal((m, classes)) * 3.0).to(dtype).cuda()      # rows differ by O(1): a wrong writer shows
    return logits, idx


@pytest.mark.parametrize("tag", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("classes", [13, 20])
def test_votes_last_writer_within_twice_torchs_softmax_error(classes, tag):
    rng = np.random.default_rng(classes)
    n_points, m = 1000, 2500
    votes = evaluate.SceneVotes(n_points, classes)
    want = np.zeros((n_points, classes))
    writes, errors = np.zeros(n_points, np.int64), []
    for call in range(2):                                                                       # the second call finds the stamps reset
        logits, idx = vote_inputs(rng, n_points, m, classes, TORCH[tag])
        counts = np.bincount(idx, minlength=n_points)
        assert 0.4 * n_points <= (counts >= 2).sum() <= 0.5 * n_points and (counts == 1).sum() >= 0.5 * n_points
        errors.append(softmax_error(logits))
        O.votes_add(want, host(logits.float()), idx)
        writes[np.unique(idx)] += 1
        votes.add(logits, dev(idx))
        assert int((votes._stamp != -1).sum()) == 0
        got = host(votes.pred).astype(np.float64)
        tol = O.vote_tolerance(max(errors))
        print(f"votes classes={classes} {tag} call {call}: torch softmax error {errors[-1]:.3e}, tolerance {tol:.3e}, measured {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= tol
        assert np.all(got[writes == 0] == 0)
    assert max(errors) < 1e-6 and writes.max() == 2
    result = host(votes.result()).astype(np.float64)
    assert np.abs(result[writes > 0].sum(-1) - 1.0).max() <= classes * 2.0 ** -23 and np.all(result[writes == 0] == 0)


@pytest.mark.parametrize("classes", [1, 5, 8, 9, 33, 64])
def test_votes_every_row_width(classes):
    """the lanes-per-row variants of the vote kernel (8, 16, 32, 64) at their edges"""
    rng = np.random.default_rng(100 + classes)
    votes = evaluate.SceneVotes(300, classes)
    logits, idx = vote_inputs(rng, 300, 701, classes, torch.float32)
    votes.add(logits, dev(idx))
    want = O.votes_add(np.zeros((300, classes)), host(logits), idx)
    tol = O.vote_tolerance(softmax_error(logits))
    assert np.abs(host(votes.pred).astype(np.float64) - want).max() <= tol
    votes.add(logits[:0], dev(idx[:0]))                                                         # no rows: nothing happens
    assert np.abs(host(votes.pred).astype(np.float64) - want).max() <= tol


def test_votes_report_an_index_out_of_range():
    votes = evaluate.SceneVotes(50, 13)
    logits = torch.randn(20, 13, device="cuda")
    idx = torch.arange(20, device="cuda")
    idx[7] = 50
    votes.add(logits, idx)
    with pytest.raises(IndexError):
        votes.result()
    assert float(votes.pred[7:8].abs().sum()) == 0.0 and float(votes.pred[8].sum()) > 0.99


def test_intersection_and_union_on_the_device():
    rng = np.random.default_rng(3)
    K = 13
    target = rng.integers(0, K, 20000)
    target[target == 2] = 1                                                                     # class 2 absent from the target
    output = rng.integers(0, K, 20000)
    output[output == 3] = 0                                                                     # class 3 absent from the output
    target[rng.random(20000) < 0.1] = 255
    out_dev = dev(output)
    got = evaluate.intersection_and_union(out_dev, dev(target), K, 255)
    want = O.intersection_and_union(output, target, K, 255)
    for a, b in zip(got, want):
        assert a.is_cuda and a.dtype == torch.int64 and np.array_equal(host(a), b)
    assert np.array_equal(host(out_dev), output) and want[2][2] == 0 and want[0][3] == 0


def torch_linear_model(weights, seen):
    """the torch twin of O.linear_model: the same float64 multiply-add steps, so the logits are identical"""
    w = dev(weights)

    def model_fn(feat, coord, offset, batch, neighbor_idx):
        assert feat.dtype == coord.dtype == torch.float32 and offset.dtype == torch.int32 and batch.dtype == torch.int64
        assert neighbor_idx.shape[0] == coord.shape[0] == batch.shape[0] == int(offset[-1]) and not torch.is_grad_enabled()
        x = torch.cat([feat, coord], 1).double()
        logits = x[:, 0:1] * w[0]
        for k in range(1, x.shape[1]):
            logits = logits + x[:, k:k + 1] * w[k]
        logits = logits.float()
        seen.append((tuple(offset.tolist()), tuple(neighbor_idx.shape), softmax_error(logits), int(batch.max())))
        return logits, None                                                                     # a tuple, as the fork's model returns
    return model_fn


def test_scene_eval_uses_a_small_part_as_a_whole():
    coord, feat, weights = O.eval_scene(np.float32, n=1000)
    seen = []
    pred = evaluate.scene_eval(torch_linear_model(weights, seen), dev(coord), dev(feat), None, 1500, 13, 0.04)
    assert [s[0] for s in seen] == [(1000,)] and seen[0][1] == (1000, 34) and seen[0][3] == 0   # one crop: the whole scene (:252-254)
    want, writes, n_crops = O.scene_eval(O.linear_model(weights), coord, feat, None, None, 1500, 13)
    assert (writes, n_crops) == (1, 1)
    assert np.abs(host(pred).astype(np.float64) - want).max() <= O.vote_tolerance(seen[0][2])


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_scene_eval_end_to_end(tag):
    coord, feat, weights = O.eval_scene(NP[tag])
    rng = np.random.default_rng(7)
    n_parts, part_size = O.scene_parts(*index_ref.voxelize(coord - coord.min(0), 0.04, 1)).shape
    priority = [rng.random(part_size) * 1e-3 for _ in range(n_parts)]
    want, writes, n_crops = O.scene_eval(O.linear_model(weights), coord, feat, lambda c, v: index_ref.voxelize(c, v, 1), 0.04, 1500, 13,
                                         priority=priority)
    seen = []
    pred = evaluate.scene_eval(torch_linear_model(weights, seen), dev(coord), dev(feat), 0.04, 1500, 13, 0.04, priority=[dev(p) for p in priority])
    assert pred.shape == (6000, 13) and pred.dtype == torch.float32
    assert sum(len(s[0]) for s in seen) == n_crops and all(len(s[0]) == 5 for s in seen[:-1]) and all(s[1][1] == 34 for s in seen)
    tol = O.vote_tolerance(max(s[2] for s in seen))
    got = host(pred).astype(np.float64)
    top = np.sort(want, 1)
    clear = top[:, -1] - top[:, -2] > tol
    print(f"scene_eval {tag}: {n_crops} crops, {writes} writes at most, torch softmax error {max(s[2] for s in seen):.3e}, tolerance {tol:.3e}, "
          f"measured {np.abs(got - want).max():.3e}, {int((~clear).sum())} points left out of the label comparison")
    assert tol < 1e-4 and np.mean(~clear) <= 0.01        # the condition tests/test_evaltile_cpu.py shows for this scene
    assert np.abs(got - want).max() <= tol
    assert np.array_equal(got.argmax(1)[clear], want.argmax(1)[clear])
    # and the counts that come out of it, against the numpy original on the oracle's labels
    label = rng.integers(0, 13, 6000)
    label[rng.random(6000) < 0.05] = 255
    if clear.all():
        got_iou = evaluate.intersection_and_union(pred.argmax(1), dev(label), 13, 255)
        assert all(np.array_equal(host(a), b) for a, b in zip(got_iou, O.intersection_and_union(want.argmax(1), label, 13, 255)))
