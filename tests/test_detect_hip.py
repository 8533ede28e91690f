"""GPU (-m gpu): the whole-scene box detection - SceneVotes(shifts=True) on csrc/evaltile.hip's fused vote, dense_points, scene_predict,
cluster.detect_boxes and detect_scene - against the numpy oracle tests/detect_oracle.py.  The summed shifts are compared as bit patterns
(one fp32 add per write), the votes within evaltile_oracle.vote_tolerance of the torch softmax error measured on the same device and
logits, as tests/test_evaltile_hip.py measures it; everything behind the votes (labels, supports, sets, boxes, score) exactly."""
import functools

import numpy as np
import pytest
import torch

from oracle import index_ref
from stratified_transformer_amd import _lib, cluster, evaluate
from tests import detect_oracle as D
from tests import evaltile_oracle as E
from tests.util import dev

pytestmark = pytest.mark.gpu
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NP = {"f32": np.float32, "f64": np.float64}
OTHER = {"f32": "f16", "f16": "bf16", "bf16": "f32"}          # shift type -> a different logit type


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def softmax_error(logits):
    """torch's own fp32 softmax on the device against the float64 softmax of the same logits (CPU): the yardstick of the vote"""
    got = host(torch.softmax(logits.float(), -1)).astype(np.float64)
    return float(np.abs(got - E.softmax64(host(logits.float()))).max())


# ---- the fused vote ----
N_POINTS, M, HIT = 97, 301, 80      # m is no multiple of 32, 16, 8 or 4 rows per workgroup; points HIT .. 96 are never indexed
RANGES = ((0, 60), (40, HIT))       # the points the first and the second call draw from: 40 .. 59 are written by both


def vote_rows(rng, classes, logit_tag, shift_tag, lo=0, hi=HIT):
    idx = rng.integers(lo, hi, M).astype(np.int64)
    logits = torch.from_numpy(rng.standard_normal((M, classes)) * 3.0).to(TORCH[logit_tag]).cuda()
    shift = torch.from_numpy(rng.standard_normal((M, 3))).to(TORCH[shift_tag]).cuda()      # rows differ: a wrong writer shows
    return logits, shift, idx


@pytest.mark.parametrize("shift_tag", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("classes", [1, 2, 8, 9, 13, 64])
def test_votes_with_shifts_at_every_row_width(classes, shift_tag):
    """two consecutive calls with overlapping indices (RANGES): the second finds the stamps reset, adds to the points both calls hit and
    leaves the points of the first call alone.  classes 1 and 2 have fewer class lanes than shift components; 8 | 9 and 13 | 64 sit on
    both sides of the lane widths 8, 16, 64.
    The bound on the votes is the project's (twice torch's softmax error on the same logits) and is tight at two classes: torch's error
    is 8e-8 there (1.3e-7 .. 2.4e-7 from 8 classes on), and an fp32 sum that reaches 1 is rounded by up to 6e-8 more, which the rule
    does not budget for.  With both calls drawing from the same 80 points the case (2, bf16 shift, f32 logits) measured 1.864e-7
    against 1.649e-7, bit-identical to the shift-less kernel; with the ranges above the six two-class cases measure 1.02e-7 .. 1.31e-7
    against 1.65e-7 .. 1.71e-7 (MI355X)."""
    logit_tag = OTHER[shift_tag] if classes != 13 else shift_tag                                # different types, and once the same
    rng = np.random.default_rng(1000 * classes + len(shift_tag))
    votes = evaluate.SceneVotes(N_POINTS, classes, shifts=True)
    plain = evaluate.SceneVotes(N_POINTS, classes)
    assert votes.shift.shape == (N_POINTS, 3) and votes.shift.dtype == torch.float32 and plain.shift is None
    want, want_shift = np.zeros((N_POINTS, classes)), np.zeros((N_POINTS, 3), np.float32)
    errors = []
    for call in range(2):
        logits, shift, idx = vote_rows(rng, classes, logit_tag, shift_tag, *RANGES[call])
        counts = np.bincount(idx, minlength=N_POINTS)
        assert counts.max() >= 2 and counts[HIT:].sum() == 0
        first_only = slice(0, RANGES[1][0])
        kept = (votes.pred[first_only].clone(), votes.shift[first_only].clone())
        errors.append(softmax_error(logits))
        D.votes_shift_add(want, want_shift, host(logits.float()), host(shift.float()), idx)
        votes.add(logits, dev(idx), shift)
        plain.add(logits, dev(idx))
        assert int((votes._stamp != -1).sum()) == 0                                             # the stamps are reset
        got, got_shift = host(votes.pred).astype(np.float64), host(votes.shift)
        tol = E.vote_tolerance(max(errors))
        print(f"shift votes classes={classes} logits {logit_tag} shift {shift_tag} call {call}: torch softmax error {errors[-1]:.3e}, "
              f"tolerance {tol:.3e}, measured {np.abs(got - want).max():.3e}")
        assert np.array_equal(bits(got_shift), bits(want_shift)), f"shift differs at {np.argwhere(bits(got_shift) != bits(want_shift))[:8].tolist()}"
        assert np.abs(got - want).max() <= tol
        assert np.all(got[HIT:] == 0) and np.all(bits(got_shift[HIT:]) == 0)                    # never indexed: exactly zero in both
        assert torch.equal(votes.pred, plain.pred)                                              # the vote alone: the same bits
        if call == 1:                                                                           # not hit by the second call: untouched
            assert torch.equal(votes.pred[first_only], kept[0]) and torch.equal(votes.shift[first_only], kept[1]) and float(kept[1].abs().sum()) > 0
    assert np.count_nonzero(want_shift[:HIT]) > 0 and max(errors) < 1e-6
    # no rows: nothing happens
    before, before_shift = votes.pred.clone(), votes.shift.clone()
    calls = _lib.CALLS[0]
    votes.add(logits[:0], dev(idx[:0]), shift[:0])
    torch.cuda.synchronize()
    assert torch.equal(votes.pred, before) and torch.equal(votes.shift, before_shift) and _lib.CALLS[0] == calls + 1
    assert np.array_equal(host(votes.labels()), host(votes.pred).argmax(1)) or classes == 1
    assert votes.labels().dtype == torch.int64 and votes.labels().shape == (N_POINTS,)


def test_votes_without_shifts_take_the_existing_launcher_bit_for_bit():
    rng = np.random.default_rng(5)
    logits, _, idx = vote_rows(rng, 13, "f32", "f32")
    votes = evaluate.SceneVotes(N_POINTS, 13, shifts=False)
    assert type(votes) is evaluate.SceneVotes
    votes.add(logits, dev(idx))
    pred = torch.zeros(N_POINTS, 13, device="cuda")
    stamp, status = torch.full((N_POINTS,), -1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.call("pointops2_evaltile_vote_launcher", M, 13, N_POINTS, 0, logits.data_ptr(), dev(idx).data_ptr(), stamp.data_ptr(), pred.data_ptr(),
              status.data_ptr(), device=pred.device)
    assert torch.equal(votes.pred, pred) and int(status) == 0 and float(pred.sum()) > 0
    assert np.array_equal(host(votes.labels()), host(pred).argmax(1))


def test_an_index_out_of_range_raises_from_labels_and_result_and_its_row_writes_nothing():
    votes = evaluate.SceneVotes(50, 2, shifts=True)
    logits, shift = torch.randn(20, 2, device="cuda"), torch.randn(20, 3, device="cuda") + 5.0
    idx = torch.arange(20, device="cuda")
    idx[7], idx[9] = 50, -1
    votes.add(logits, idx, shift)
    with pytest.raises(IndexError):
        votes.labels()
    with pytest.raises(IndexError):
        votes.result()
    for bad in (7, 9):
        assert float(votes.pred[bad].abs().sum()) == 0.0 and float(votes.shift[bad].abs().sum()) == 0.0
    assert float(votes.pred[8].sum()) > 0.99 and torch.equal(votes.shift[8], shift[8]) and torch.equal(votes.shift[:7], shift[:7])
    assert float(votes.pred[20:].abs().sum()) == 0.0 and float(votes.shift[20:].abs().sum()) == 0.0


def test_the_launcher_records_bad_arguments_before_any_launch():
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    name = "pointops2_evaltile_vote_shift_launcher"
    for args in ((4, 65, 4, 0, p, 0, p, p, p, p, p, p), (4, 0, 4, 0, p, 0, p, p, p, p, p, p), (4, 4, 0, 0, p, 0, p, p, p, p, p, p),
                 (-1, 4, 4, 0, p, 0, p, p, p, p, p, p), (4, 4, 4, 3, p, 0, p, p, p, p, p, p), (4, 4, 4, 0, p, 3, p, p, p, p, p, p),
                 (4, 4, 4, 0, p, -1, p, p, p, p, p, p), (4, 4, 4, 0, p, 0, None, p, p, p, p, p), (4, 4, 4, 0, p, 0, p, p, p, p, None, p),
                 (4, 4, 4, 0, p, 0, p, p, None, p, p, p)):
        with pytest.raises(RuntimeError, match="evaltile_vote_shift"):
            _lib.call(name, *args, device=t.device)
    _lib.call(name, 0, 4, 4, 0, None, 0, None, None, None, None, None, None, device=t.device)    # m = 0: a no-op, whatever the arrays
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0


# ---- the dense-point filter ----
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_dense_points_equal_the_oracle(tag):
    coord, blob = D.blob_cloud()
    coord = coord.astype(NP[tag])
    want, want_index = D.dense_points(coord)
    assert len(want_index) == 111
    kept, index = evaluate.dense_points(dev(coord))
    assert index.dtype == torch.int64 and kept.dtype == dev(coord).dtype and kept.shape == (111, 3)
    assert np.array_equal(host(index), want_index) and np.array_equal(host(kept), want)
    assert len(host(evaluate.dense_points(dev(coord), min_points=49)[1])) == 161                # >=: the 50-point blob would stay
    # all noise, everything dropped, and no point: empty results; no launch where there is no point
    for cloud, kw in ((coord[blob == -1], {}), (coord, {"min_points": 60})):
        kept, index = evaluate.dense_points(dev(cloud), **kw)
        assert kept.shape == (0, 3) and index.shape == (0,) and index.dtype == torch.int64
    calls = _lib.CALLS[0]
    kept, index = evaluate.dense_points(dev(coord[:0]))
    assert kept.shape == (0, 3) and index.shape == (0,) and index.dtype == torch.int64 and _lib.CALLS[0] == calls


# ---- scene_predict ----
def torch_lookup_model(table, shift_table, classes, seen, shift_dtype=torch.float32):
    """the torch twin of D.lookup_model"""
    tab, sh = dev(table), dev(shift_table)

    def model_fn(feat, coord, offset, batch, neighbor_idx):
        assert feat.dtype == coord.dtype == torch.float32 and offset.dtype == torch.int32 and batch.dtype == torch.int64
        assert neighbor_idx.shape[0] == coord.shape[0] == batch.shape[0] == int(offset[-1]) and not torch.is_grad_enabled()
        i = feat[:, 0].long()
        logits = 8.0 * torch.nn.functional.one_hot(tab[i], classes).float()
        seen.append((len(offset), softmax_error(logits)))
        return logits, sh[i].to(shift_dtype)
    return model_fn


@functools.lru_cache(maxsize=None)
def predict_case(tag, voxel_max, batch):
    """the scene, its tables and the oracle's (pred, shift, visits, n_crops), computed once"""
    n = 6000
    coord = E.eval_scene(NP[tag], n=n)[0]
    rng = np.random.default_rng(11)
    feat = np.arange(n, dtype=NP[tag])[:, None]
    table, shift_table = rng.integers(0, 13, n), rng.standard_normal((n, 3)).astype(np.float32)

    def voxelize(c, v):
        return index_ref.voxelize(c, v, 1)
    n_parts, part_size = E.scene_parts(*voxelize(coord - coord.min(0), 0.04)).shape
    priority = [rng.random(part_size) * 1e-3 for _ in range(n_parts)]
    want = D.scene_predict(D.lookup_model(table, shift_table, 13), coord, feat, voxelize, 0.04, voxel_max, 13, batch_size_test=batch, feat_div=None,
                           priority=priority)
    return coord, feat, table, shift_table, priority, part_size, want


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_scene_predict_end_to_end(tag):
    """voxel_max 4000 tiles every part (5446 points) into three or four overlapping crops, 18 in all; batches of 9 crops make two
    batches, so a point is written once or twice.  The shift of a point written twice is the sum of both predictions, bit for bit.
    The raw votes of such a point are p + p, exact in fp32, so the one tolerance of the vote - twice torch's own softmax error -
    holds for them as for a single row; with more visits per point the sum would be rounded at the ulp of 3 .. 10 instead."""
    coord, feat, table, shift_table, priority, part_size, (want, want_shift, visits, n_crops) = predict_case(tag, 4000, 9)
    assert part_size > 4000 and n_crops >= 3 * len(priority) and visits.min() >= 1 and visits.max() == 2 and (visits == 2).sum() > 1000
    seen = []
    pred, shift = evaluate.scene_predict(torch_lookup_model(table, shift_table, 13, seen), dev(coord), dev(feat), 0.04, 4000, 13, 0.04,
                                         batch_size_test=9, feat_div=None, priority=[dev(p) for p in priority])
    assert pred.shape == (6000, 13) and pred.dtype == torch.float32 and shift.shape == (6000, 3) and shift.dtype == torch.float32
    assert [s[0] for s in seen] == [9] * (n_crops // 9) + ([n_crops % 9] if n_crops % 9 else [])
    got, got_shift = host(pred).astype(np.float64), host(shift)
    tol = E.vote_tolerance(max(s[1] for s in seen))
    print(f"scene_predict {tag}: {n_crops} crops, visits {np.bincount(visits).tolist()}, torch softmax error {max(s[1] for s in seen):.3e}, "
          f"tolerance {tol:.3e}, measured {np.abs(got - want).max():.3e}")
    assert np.array_equal(bits(got_shift), bits(want_shift))
    twice = visits == 2
    assert np.array_equal(got_shift[twice], shift_table[twice] + shift_table[twice]) and np.array_equal(got_shift[~twice], shift_table[~twice])
    assert np.array_equal(got.argmax(1), table)                                                 # every point was visited
    assert np.abs(got - want).max() <= tol
    assert np.abs(got.sum(1) - visits).max() < 1e-5                                             # raw: not normalised


def test_scene_predict_sums_the_shifts_of_many_visits_in_half_precision():
    """the default batches of five crops at voxel_max 1500: up to ten writes per point; the model's shift in f16"""
    coord, feat, table, shift_table, priority, _, (want, want_shift, visits, n_crops) = predict_case("f32", 1500, 5)
    shift_table = shift_table.astype(np.float16).astype(np.float32)                             # (the oracle saw f32 rows: redo it on the f16 values)
    want_shift = D.scene_predict(D.lookup_model(table, shift_table, 13), coord, feat, lambda c, v: index_ref.voxelize(c, v, 1), 0.04, 1500, 13,
                                 feat_div=None, priority=priority)[1]
    assert visits.max() >= 5
    seen = []
    pred, shift = evaluate.scene_predict(torch_lookup_model(table, shift_table, 13, seen, torch.float16), dev(coord), dev(feat), 0.04, 1500, 13, 0.04,
                                         feat_div=None, priority=[dev(p) for p in priority])
    assert len(seen) == -(-n_crops // 5) and np.array_equal(bits(host(shift)), bits(want_shift))
    assert np.array_equal(host(pred).argmax(1), table) and np.abs(host(pred).sum(1) - visits).max() < 1e-4


def test_scene_predict_wants_a_pair_from_the_model():
    coord, feat = dev(E.room(500, 9)[0].astype(np.float32)), torch.arange(500, dtype=torch.float32, device="cuda")[:, None]
    for out in (torch.zeros(500, 13, device="cuda"), (torch.zeros(500, 13, device="cuda"),)):
        with pytest.raises(TypeError, match="model_fn must return the pair"):
            evaluate.scene_predict(lambda *a: out, coord, feat, None, None, 13, 0.04, feat_div=None)
    # scene_eval still takes both forms
    votes = evaluate.scene_eval(lambda *a: torch.zeros(500, 13, device="cuda"), coord, feat, None, None, 13, 0.04, feat_div=None)
    assert votes.shape == (500, 13)


# ---- detect_boxes / detect_scene ----
@functools.lru_cache(maxsize=None)
def detect_case(which):
    if which == "four":
        return D.box_scene()
    if which == "one":
        return D.box_scene(seed=4, corners=((0.0, 0.0, 0.0),), loose=10)
    coord, table, shift, gt = D.box_scene(seed=5, corners=(), loose=60)                         # "none": scattered points only
    return coord, table, shift, np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0]])


def run_detect(which, **settings):
    coord, table, shift_table, gt = detect_case(which)
    n = len(coord)
    feat = np.arange(n, dtype=np.float32)[:, None]
    # the oracle's (coord, shift, pred): one crop, one batch - every point is written once
    pred64, want_shift, visits, n_crops = D.scene_predict(D.lookup_model(table, shift_table, D.CLASSES), coord, feat, None, None, None, D.CLASSES,
                                                          feat_div=None)
    assert n_crops == 1 and visits.max() == 1 and np.array_equal(pred64.argmax(1), table) and np.array_equal(bits(want_shift), bits(shift_table))
    seen = []
    got = evaluate.detect_scene(torch_lookup_model(table, shift_table, D.CLASSES, seen), dev(coord), dev(feat), None, None, D.CLASSES, 0.04,
                                feat_div=None, gt_box=gt, **settings)
    # by hand: the existing public functions on the oracle's outputs
    c, s, p = dev(coord), dev(want_shift), dev(pred64.argmax(1))
    points, obj, source, n_objects, instance, point_object = cluster.box_supports(c, s, p, **{k: v for k, v in settings.items() if not k.startswith("merge_")})
    merged, set_of, boxes, n_sets = cluster.merge_objects(points, obj, n_objects, **({"radius": settings["merge_radius"]} if "merge_radius" in settings else {}))
    assert isinstance(got, evaluate.DetectedScene) and got.n_sets == n_sets and got.boxes.shape == (n_sets, 6) and got.boxes.dtype == torch.float32
    assert torch.equal(got.boxes, boxes) and torch.equal(got.points, points) and torch.equal(got.merged, merged)
    assert got.label.dtype == torch.int64 and np.array_equal(host(got.label), table) and np.array_equal(bits(host(got.shift)), bits(want_shift))
    assert got.score == cluster.box_detection(boxes, gt, 0.25)
    # and detect_boxes, with the per-point results
    again = cluster.detect_boxes(c, s, p, **settings)
    assert len(again) == 6 and torch.equal(again[0], boxes) and torch.equal(again[1], points) and torch.equal(again[2], merged) and again[3] == n_sets
    assert again[4].dtype == again[5].dtype == torch.int32 and torch.equal(again[4], instance) and torch.equal(again[5], point_object)
    return got, (points, obj, n_objects, instance, point_object), gt


def test_detect_scene_equals_the_chain_of_the_public_functions():
    got, (points, obj, n_objects, instance, point_object), gt = run_detect("four")
    coord, table, shift_table, _ = detect_case("four")
    assert len(coord) <= 12000
    # the structure the CPU test shows for this scene under the oracles: four objects, the two close boxes merge, the strays are gone
    assert n_objects == 4 and got.n_sets == 3 and sorted(np.bincount(host(got.merged)).tolist())[-1] > len(points) // 3
    stray = np.abs(shift_table[:, 2]) > 0.3
    assert stray.sum() == 24 and np.all(host(point_object)[stray] >= 0) and float(got.boxes[:, 5].max()) < gt[:, 5].max() + 0.05
    tp, fp, fn, precision, recall = got.score
    assert (len(tp), fp, fn, precision, recall) == (3, [], 1, 1.0, 0.75)
    assert evaluate.detect_scene(lambda f, *a: (8.0 * torch.nn.functional.one_hot(dev(table)[f[:, 0].long()], 18).float(), dev(shift_table)[f[:, 0].long()]),
                                 dev(coord), dev(np.arange(len(coord), dtype=np.float32)[:, None]), None, None, 18, 0.04, feat_div=None).score is None
    # other settings reach their steps: a merge radius too small for any neighbour leaves the four boxes apart
    apart, _, _ = run_detect("four", merge_radius=0.001)
    assert apart.n_sets == 4


@pytest.mark.parametrize("which,n_boxes", [("one", 1), ("none", 0)])
def test_fewer_than_two_supports_return_their_boxes(which, n_boxes):
    got, (points, obj, n_objects, _, _), gt = run_detect(which)
    assert n_objects == n_boxes and got.n_sets == n_boxes and got.boxes.shape == (n_boxes, 6) and got.points.shape[0] == got.merged.shape[0]
    tp, fp, fn, precision, recall = got.score
    assert (len(tp), fp, fn) == (n_boxes, [], 1 - n_boxes)
    if n_boxes:
        assert np.abs(host(got.boxes)[0] - gt[0]).max() < 0.02
