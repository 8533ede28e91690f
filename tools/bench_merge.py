"""The OBB merging behind the grouping (stratified_transformer_amd.cluster.merge_objects on csrc/boxes.hip) on the box scene of
tools/bench_contacts.py: about 100k points, the reference's settings (radius 0.2, overlap 0.3, more than 10 near points).  Prints ONE
JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_merge.py [--points 100000] [--spacing 1.3] [--reps 30] [--warmup 3] [--host-points 12000] [--no-host]
                                [--out profiles/merge_bench.json]

The objects come from cluster.instances and cluster.objects on the same scene with a zero shift (not timed).  `merge_ms`: median over
`reps` calls of merge_objects after `warmup` calls, device events around the call; it ends in a read-back, so `merge_host_ms` gives the
host clock around the same calls.  The parts are merge_objects' own step functions on its prologue's result, each timed the same way on
its own: `grid_ms` (keys, torch.sort, prepare), `boxes_ms` (label_boxes' launch), `rows_ms` (the fixed-radius walk), `unique_ms` (border
selection and torch.unique) and `host_loop_ms` (merge_sets on the read-back tables, host clock).
`--spacing`: distance between the boxes' corners; at the default 1.3 of bench_contacts the boxes stand 0.5 apart and nothing is within reach of anything, at 0.85 neighbours are 0.05 / 0.15 apart and most points are border points.
The host reference is the literal loop of tests/merge_oracle.py (per pair of sets one brute-force pass over all pairs of their points,
what the reference's cdist does) on the same machine, on a scene of `--host-points` points, where one pair's matrix still fits;
`small_*` are the device's times on that same scene and `small_agrees` says whether both give the same sets and boxes."""
import argparse
import statistics
import time

import numpy as np
import torch

import timing  # first: it puts the repository root on sys.path
from bench_contacts import box  # noqa: E402
from stratified_transformer_amd import cluster  # noqa: E402


def make_scene(points, spacing, seed=0):
    """tools/bench_contacts.make_scene with the distance between the boxes as a parameter"""
    rng = np.random.default_rng(seed)
    probe, _ = box(rng, (0, 0, 0), (0.8, 0.7, 0.6), 1)
    face_points = len(probe) - 12
    edge_points = int(round(face_points * 0.4 / 0.6 / 12))
    n_boxes = max(1, int(round(points / (face_points + 12 * edge_points))))
    side = int(np.ceil(np.sqrt(n_boxes)))
    parts = [box(rng, (spacing * (b % side), spacing * (b // side), 0.0), (0.8, 0.7, 0.6), edge_points) for b in range(n_boxes)]
    coord, pred = np.concatenate([p[0] for p in parts]).astype(np.float32), np.concatenate([p[1] for p in parts])
    perm = rng.permutation(len(pred))
    return coord[perm], pred[perm], n_boxes


def objects_of(coord_h, pred_h):
    coord, pred = torch.from_numpy(coord_h).cuda(), torch.from_numpy(pred_h).cuda()
    instance, cls, size = cluster.instances(coord, torch.zeros_like(coord), pred)
    obj, _, n_objects = cluster.objects(coord, instance, cls, size)
    return coord, obj, n_objects


def parts_ms(coord, obj, n_objects, reps, warmup):
    """the steps of merge_objects one by one: its own step functions, in its order, on the prologue's result"""
    call = cluster._Call("merge_objects", cluster.LAST_MERGE, coord, obj)
    r, r2 = cluster._radius(call.who, cluster.MERGE_RADIUS)
    p = cluster._labelled(call, coord, obj, n_objects, "n_objects")
    out = {}
    out["grid_ms"], _, (pts, slabel, ranges) = timing.device_ms(lambda: cluster._label_grid(call, p, r), reps, warmup)
    out["boxes_ms"], _, (lo, hi, size) = timing.device_ms(lambda: cluster._boxes(call, p), reps, warmup)
    out["rows_ms"], _, rows = timing.device_ms(lambda: cluster._rows(call, pts, slabel, ranges, p.n_labels, r2), reps, warmup)
    out["unique_ms"], _, (pat, count) = timing.device_ms(lambda: cluster._patterns(slabel, rows), reps, warmup)
    tables = cluster._merge_tables(call, lo, hi, size, pat, count)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        cluster.merge_sets(*tables)
        times.append((time.perf_counter() - t0) * 1e3)
    out["host_loop_ms"] = statistics.median(times)
    out = {k: round(v, 4) for k, v in out.items()}
    out.update(cells=cluster._dims(call.who, 1, p.origin, p.top, r)[1], labelled_points=p.n_valid, border_points=int((rows != 0).any(1).sum().item()), patterns=int(pat.shape[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--spacing", type=float, default=1.3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=12000)
    ap.add_argument("--no-host", action="store_true", help="skip the literal host loop")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timing.need_gpu("bench_merge")
    if a.reps < 20:
        raise SystemExit("bench_merge: at least 20 timed calls")
    coord_h, pred_h, n_boxes = make_scene(a.points, a.spacing)
    coord, obj, n_objects = objects_of(coord_h, pred_h)
    merge_ms, merge_host_ms, (merged, set_of, boxes, n_sets) = timing.device_ms(lambda: cluster.merge_objects(coord, obj, n_objects), a.reps, a.warmup)
    calls = dict(cluster.LAST_MERGE)
    result = {"tool": "bench_merge", "device": torch.cuda.get_device_name(0), "points": len(coord_h), "boxes": n_boxes, "spacing": a.spacing,
              "objects": n_objects, "sets": n_sets, "radius": cluster.MERGE_RADIUS, "overlap": cluster.MERGE_OVERLAP,
              "min_neighbors": cluster.MERGE_MIN_NEIGHBORS, "reps": a.reps, "warmup": a.warmup, "merge_ms": round(merge_ms, 4),
              "merge_host_ms": round(merge_host_ms, 4), "library_launches": calls["launches"], "readbacks": calls["readbacks"]}
    result.update(parts_ms(coord, obj, n_objects, a.reps, a.warmup))
    if not a.no_host:
        from tests import merge_oracle
        small_h, small_pred, small_boxes = make_scene(a.host_points, a.spacing)
        small, small_obj, small_n = objects_of(small_h, small_pred)
        ms, host_ms, got = timing.device_ms(lambda: cluster.merge_objects(small, small_obj, small_n), a.reps, a.warmup)
        obj_h = small_obj.cpu().numpy()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            want_of, want_sets, want_boxes = merge_oracle.merge_literal(small_h, obj_h, small_n)
            times.append((time.perf_counter() - t0) * 1e3)
        result.update(small_points=len(small_h), small_boxes=small_boxes, small_objects=small_n, small_sets=got[3], small_merge_ms=round(ms, 4),
                      small_merge_host_ms=round(host_ms, 4), small_literal_loop_ms=round(statistics.median(times), 2),
                      small_agrees=bool(np.array_equal(got[1].cpu().numpy(), want_of) and np.array_equal(got[2].cpu().numpy(), want_boxes)))
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
