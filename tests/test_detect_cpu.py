"""CPU: the oracle of the whole-scene box detection (tests/detect_oracle.py) - the dense-point filter against scikit-learn itself, the
last-writer rule of the two accumulators, the scenes the GPU tests use - and the host side of what stratified_transformer_amd adds for
it: the declaration and export of the new launcher, the package's names, the argument checks.  No HIP compute runs here."""
import inspect

import numpy as np
import pytest
import torch

import stratified_transformer_amd as sta
from oracle import index_ref
from stratified_transformer_amd import _lib, cluster, evaluate
from tests import abi_header
from tests import detect_oracle as D
from tests import evaltile_oracle as E

LAUNCHER = "pointops2_evaltile_vote_shift_launcher"


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)

    def __getitem__(self, key):
        return self._t[key]


# ---- the dense-point filter ----
def test_dense_points_is_the_loaders_filter_run_with_scikit_learn():
    """test_iou.py:147-151 as the loader runs them, on the three-blob cloud: 60 and 51 points stay, 50 do not (> 50, not >= 50)"""
    DBSCAN = pytest.importorskip("sklearn.cluster").DBSCAN
    coord, blob = D.blob_cloud()
    fit = DBSCAN(eps=0.1, min_samples=5).fit(coord)
    clusters = [coord[fit.labels_ == c] for c in range(fit.labels_.max() + 1)]
    want = np.concatenate([c for c in clusters if len(c) > 50])
    assert sorted(len(c) for c in clusters) == [50, 51, 60] and int((fit.labels_ == -1).sum()) == 25
    kept, index = D.dense_points(coord)
    assert index.dtype == np.int64 and np.array_equal(kept, want) and np.array_equal(coord[index], want)
    assert len(index) == 111 and set(blob[index].tolist()) == {0, 1}                            # the 50-point blob and the noise are gone
    # the order: cluster by cluster in ascending cluster number - here NOT the order of the blobs' numbers -, ascending index inside
    first = blob[index[0]]
    size = {0: 60, 1: 51}[int(first)]
    assert first == 1 and np.all(blob[index[:size]] == first) and np.all(blob[index[size:]] == 1 - first)
    assert np.all(np.diff(index[:size]) > 0) and np.all(np.diff(index[size:]) > 0) and index[size] < index[size - 1]
    # at >= the third blob would stay; with everything dropped and with no point nothing is left
    assert len(D.dense_points(coord, min_points=49)[1]) == 161
    assert D.dense_points(coord, min_points=60)[0].shape == (0, 3) and D.dense_points(coord[:0])[1].shape == (0,)
    assert D.dense_points(coord[blob == -1])[1].shape == (0,)                                   # all noise


# ---- the two accumulators ----
def test_votes_shift_add_lets_the_last_row_of_a_repeated_index_write_both():
    idx = np.array([2, 0, 2, 1, 2])
    logits = np.array([[0, 1, 2], [3, 0, 0], [0, 5, 0], [1, 1, 1], [0, 0, 4]], np.float32)
    rows = np.array([[1, 2, 3], [10, 20, 30], [100, 200, 300], [0.5, 0.25, 0.125], [-7, -8, -9]], np.float32)
    pred, shift = np.zeros((4, 3)), np.zeros((4, 3), np.float32)
    shift[2] = [0.5, 0.5, 0.5]
    D.votes_shift_add(pred, shift, logits, rows, idx)
    assert shift.dtype == np.float32 and shift.tolist() == [[10, 20, 30], [0.5, 0.25, 0.125], [-6.5, -7.5, -8.5], [0, 0, 0]]
    assert np.array_equal(pred[2], E.softmax64(logits[4])) and np.array_equal(pred[0], E.softmax64(logits[1])) and np.all(pred[3] == 0)
    # CPU torch's indexed assignment does the same to both tensors
    t_pred, t_shift = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3)
    t_shift[2] = 0.5
    t_pred[torch.from_numpy(idx), :] += torch.softmax(torch.from_numpy(logits).double(), -1)    # test_iou.py:337
    t_shift[torch.from_numpy(idx), :] += torch.from_numpy(rows)                                 # test_iou.py:338
    assert np.array_equal(t_shift.numpy(), shift) and np.allclose(t_pred.numpy(), pred, rtol=0, atol=1e-15)
    # a second call adds to the first: the sum over calls, one fp32 add each
    D.votes_shift_add(pred, shift, logits[:2], rows[:2].astype(np.float16), np.array([2, 2]))
    assert shift[2].tolist() == [3.5, 12.5, 21.5] and np.array_equal(pred[2], E.softmax64(logits[4]) + E.softmax64(logits[1]))


def test_oracle_scene_predict_sums_the_shifts_of_every_visit():
    """the end-to-end scene of the GPU test: some points are written by two or more batches, and their shift is the SUM"""
    coord, feat, table, shift_table, voxelize, priority = D_scene(np.float64)
    pred, shift, visits, n_crops = D.scene_predict(D.lookup_model(table, shift_table, 13), coord, feat, voxelize, 0.04, 1500, 13, feat_div=None,
                                                   priority=priority)
    assert n_crops > 5 and visits.min() >= 1 and visits.max() >= 2 and (visits >= 2).sum() > 100
    assert np.array_equal(pred.argmax(1), table)
    once, twice = visits == 1, visits == 2
    assert np.array_equal(shift[once], shift_table[once]) and np.array_equal(shift[twice], shift_table[twice] + shift_table[twice])
    assert not np.array_equal(shift[twice], shift_table[twice])
    assert np.allclose(pred.sum(1), visits)                                                     # raw votes: one softmax row per visit


def D_scene(dtype, n=6000):
    """evaltile_oracle.eval_scene with the point's own index as the one feature column, the lookup tables and the parts' priorities"""
    coord = E.eval_scene(dtype, n=n)[0]
    rng = np.random.default_rng(11)
    feat = np.arange(n, dtype=dtype)[:, None]
    table, shift_table = rng.integers(0, 13, n), rng.standard_normal((n, 3)).astype(np.float32)

    def voxelize(c, v):
        return index_ref.voxelize(c, v, 1)
    n_parts, part_size = E.scene_parts(*voxelize(coord - coord.min(0), 0.04)).shape
    return coord, feat, table, shift_table, voxelize, [rng.random(part_size) * 1e-3 for _ in range(n_parts)]


def test_the_detection_scene_merges_two_boxes_and_loses_its_strays_under_the_oracles():
    coord, table, shift, gt = D.box_scene()
    assert len(coord) <= 12000 and gt.shape == (4, 6) and set(table.tolist()) == set(range(18))
    want = D.chain(coord, shift, table)
    set_of, sets, boxes = want["merge"]
    assert want["n_objects"] == 4 and want["supports"][3] == 4 and sorted(map(len, sets)) == [1, 1, 2]   # the two close boxes merge
    assert int((want["obj"] >= 0).sum()) - int((D.chain(coord, np.zeros_like(shift), table)["obj"] >= 0).sum()) == 4 * 6   # the strays, by their shift
    assert boxes[:, 5].max() < gt[:, 5].max() + 0.05                                           # ... and the clean-up removed them again
    tp, fp, fn, precision, recall = cluster.box_detection(boxes, gt, 0.25)
    assert (len(tp), fp, fn, precision, recall) == (3, [], 1, 1.0, 0.75)
    one = D.box_scene(seed=4, corners=((0.0, 0.0, 0.0),), loose=10)
    assert D.chain(one[0], one[2], one[1])["merge"][1] == [[0]]                                 # fewer than two supports: one box


# ---- the host side ----
def test_the_launcher_is_declared_and_exported():
    args = abi_header.parameters(LAUNCHER)
    assert [a.split()[-1].lstrip("*") for a in args] == ["m", "classes", "n_points", "row_type", "logits", "shift_row_type", "shift", "idx", "stamp",
                                                           "pred", "pred_shift", "status"]
    assert _lib.SIGNATURES["pointops2_evaltile_vote_launcher"] == [_lib.I] * 4 + [_lib.P] * 5                # the vote alone: as it was


def test_public_interface():
    for name, home in (("scene_predict", evaluate), ("dense_points", evaluate), ("detect_scene", evaluate), ("detect_boxes", cluster)):
        assert getattr(sta, name) is getattr(home, name) and name in sta.__all__
    head = "(model_fn, coord, feat, voxel_size, voxel_max, classes, grid_size, max_num_neighbors=34, batch_size_test=5, feat_div=255.0, concat_xyz=False, priority=None"
    assert str(inspect.signature(evaluate.scene_predict)) == head + ")"
    assert str(inspect.signature(evaluate.scene_predict)) == str(inspect.signature(evaluate.scene_eval))
    assert str(inspect.signature(evaluate.detect_scene)) == head + ", gt_box=None, overlap_threshold=0.25, **cluster_settings)"
    assert str(inspect.signature(evaluate.dense_points)) == "(coord, eps=0.1, min_samples=5, min_points=50)"
    assert str(inspect.signature(evaluate.SceneVotes.__init__)) == "(self, n_points, classes, device='cuda', shifts=False)"
    votes = evaluate.SceneVotes(10, 3, device="cpu", shifts=True)
    assert list(inspect.signature(votes.add).parameters) == ["logits", "idx", "shift"] and isinstance(votes, evaluate.SceneVotes)
    params = list(inspect.signature(cluster.detect_boxes).parameters)
    assert params[:13] == list(inspect.signature(cluster.box_supports).parameters) and params[13:] == ["merge_radius", "overlap", "min_neighbors"]
    assert evaluate.DetectedScene._fields == ("boxes", "label", "shift", "points", "merged", "n_sets", "score")
    for fn, words in ((evaluate.scene_predict, ("SUM", "not their mean")), (evaluate.detect_scene, ("cast to fp32", "fewer than two supports"))):
        assert all(w in fn.__doc__ for w in words)


def test_votes_check_the_shift_against_the_constructor_flag_before_any_launch():
    calls = _lib.CALLS[0]
    plain, both = evaluate.SceneVotes(100, 13, device="cpu"), evaluate.SceneVotes(100, 13, device="cpu", shifts=True)
    assert plain.shift is None and both.shift.shape == (100, 3) and both.shift.dtype == torch.float32 and float(both.shift.abs().sum()) == 0.0
    logits, idx = _OnGpu(torch.zeros(10, 13)), _OnGpu(torch.zeros(10, dtype=torch.int64))
    with pytest.raises(ValueError, match="shifts=True"):
        both.add(logits, idx)                                                                   # built with shifts: the rows are required
    with pytest.raises(TypeError):
        plain.add(logits, idx, torch.zeros(10, 3))                                              # built without: add takes no third argument
    with pytest.raises(TypeError):
        plain.add(logits, idx, shift=torch.zeros(10, 3))
    for shift in (torch.zeros(10, 2), torch.zeros(9, 3), torch.zeros(30), torch.zeros(10, 3, 1), torch.zeros(10, 3, dtype=torch.float64),
                  torch.zeros(10, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="SceneVotes.add: shift"):
            both.add(logits, idx, _OnGpu(shift))
    with pytest.raises(ValueError, match="SceneVotes.add: logits"):
        both.add(_OnGpu(torch.zeros(10, 12)), idx, _OnGpu(torch.zeros(10, 3)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        both.add(logits, idx, torch.zeros(10, 3))                                               # a CPU shift
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        both.add(torch.zeros(10, 13), idx, _OnGpu(torch.zeros(10, 3)))                          # CPU logits
    assert _lib.CALLS[0] == calls
    assert both.labels().dtype == torch.int64 and both.labels().shape == (100,) and both.result().shape == (100, 13)


def test_scene_predict_wants_a_pair_from_the_model(monkeypatch):
    """the tiling and the ball query stubbed out (they need the GPU): the check on what model_fn returns sits in front of the vote"""
    coord, feat = torch.rand(50, 3), torch.rand(50, 1)
    monkeypatch.setattr(evaluate, "scene_parts", lambda c, v: torch.arange(50)[None])
    monkeypatch.setattr(evaluate.pointops, "ball_query", lambda *a: (torch.zeros(50, 4, dtype=torch.int32), None))
    calls = _lib.CALLS[0]
    for out in (torch.zeros(50, 13), (torch.zeros(50, 13),), (torch.zeros(50, 13), torch.zeros(50, 3), None), None):
        with pytest.raises(TypeError, match="scene_predict: model_fn must return the pair"):
            evaluate.scene_predict(lambda *a: out, _OnGpu(coord), _OnGpu(feat), None, None, 13, 0.04)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        evaluate.scene_predict(lambda *a: None, coord, feat, None, None, 13, 0.04)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        evaluate.detect_scene(lambda *a: None, coord, feat, None, None, 13, 0.04)
    assert _lib.CALLS[0] == calls


def test_dense_points_and_detect_boxes_reject_bad_arguments_before_any_launch():
    calls = _lib.CALLS[0]
    coord = torch.zeros(100, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        evaluate.dense_points(coord)
    for kw in ({"min_points": -1}, {"min_points": 1.5}, {"min_points": True}):
        with pytest.raises(ValueError, match="dense_points"):
            evaluate.dense_points(_OnGpu(coord), **kw)
    for kw in ({"eps": 0.0}, {"min_samples": 0}):
        with pytest.raises(ValueError, match="dbscan"):
            evaluate.dense_points(_OnGpu(coord[:0]), **kw)
    kept, index = evaluate.dense_points(_OnGpu(coord[:0]))                                      # no point: nothing to launch
    assert kept.shape == (0, 3) and index.shape == (0,) and index.dtype == torch.int64
    xyz, pred = _OnGpu(coord), _OnGpu(torch.zeros(100, dtype=torch.int64))
    for kw, where in (({"voxel": 0.0}, "clean_supports"), ({"nb_points": -1}, "clean_supports"), ({"merge_radius": -1.0}, "merge_objects"),
                      ({"merge_radius": float("nan")}, "merge_objects")):
        with pytest.raises(ValueError, match=where):
            cluster.detect_boxes(xyz, xyz, pred, **kw)
        with pytest.raises(ValueError, match=where):
            evaluate.detect_scene(lambda *a: None, xyz, xyz, None, None, 18, 0.04, **kw)        # ... and before the model runs
    for kw in ({"overlap": "a"}, {"min_neighbors": None}):
        with pytest.raises(ValueError, match="merge_sets"):
            cluster.detect_boxes(xyz, xyz, pred, **kw)
    with pytest.raises(TypeError, match="unexpected settings"):
        evaluate.detect_scene(lambda *a: None, xyz, xyz, None, None, 18, 0.04, merge_overlap=0.3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.detect_boxes(coord, coord, torch.zeros(100, dtype=torch.int64))
    assert _lib.CALLS[0] == calls
