"""The clean-up of the box supports (stratified_transformer_amd.cluster.clean_supports on csrc/supports.hip) on the box scene of
tools/bench_contacts.py: about 100k points, the reference's settings (voxel 0.04, radius 0.1, more than 3 neighbours).  Prints ONE JSON
line (GPU box only; a missing GPU is an error).

    python tools/bench_supports.py [--points 100000] [--strays 40] [--reps 30] [--warmup 3] [--host-points 12000] [--no-host]
                                   [--out profiles/supports_bench.json]

The objects come from cluster.instances and cluster.objects on the same scene with a zero shift (not timed).  Every object then gets
`--strays` seeded stray points under its number, 0.15 to 0.5 outside its box, so that the outlier pass removes something.
`supports_ms`: median over `reps` calls of clean_supports after `warmup` calls, device events around the call; it ends in a read-back, so
`supports_host_ms` gives the host clock around the same calls.  The parts are clean_supports' own step functions on its prologue's result,
each timed the same way on its own: `boxes_ms` (label_boxes' launch), `keys_sort_ms` (voxel keys, torch.sort, head flags, their scan and
the read-back of the number of voxels), `means_ms`, `grid_ms` (keys, torch.sort, prepare on the means), `count_ms` (the fixed-radius walk)
and `compact_ms` (survivors per object with their read-back, compaction and renumbering with torch).
The host restatement is the per-object loop of tests/supports_oracle.py (a dict of float64 sums per voxel, in Python - Open3D itself is on
no machine here) on the same machine in the same run (median of 3), with scipy's cKDTree for the counts where scipy imports
(`host_counts: "ckdtree"`, float64 distances: a pair within about 1e-6 of the radius may fall on the other side, `host_kept` is reported
beside `kept`); otherwise with the oracle's dense fp32 matrix on a scene of `--host-points` points, where it fits (`host_counts: "dense"`,
`host_points` says the size, `small_*` are the device's times on that same scene)."""
import argparse
import statistics
import time

import numpy as np
import torch

import timing  # first: it puts the repository root on sys.path
from bench_contacts import make_scene  # noqa: E402
from stratified_transformer_amd import cluster  # noqa: E402

NOT_MEASURED = ["more than 16 objects", "clouds of millions of points", "a per-kernel profile (no run under rocprofv3 was taken)",
                "voxel runs of thousands of points (one thread walks a run)"]


def scene_with_strays(points, strays, seed=0):
    """-> (coord float32 [N + O * strays, 3] on the host, obj int32 on the host, n_objects): the box scene, its objects from objects(), and
    `strays` points per object 0.15 to 0.5 outside the object's box on every axis, under the object's number; shuffled"""
    coord_h, pred_h, n_boxes = make_scene(points)
    coord, pred = torch.from_numpy(coord_h).cuda(), torch.from_numpy(pred_h).cuda()
    instance, cls, size = cluster.instances(coord, torch.zeros_like(coord), pred)
    obj, _, n_objects = cluster.objects(coord, instance, cls, size)
    obj_h = obj.cpu().numpy()
    rng = np.random.default_rng(seed + 1)
    extra, extra_obj = [], []
    for o in range(n_objects):
        hi = coord_h[obj_h == o].max(0)
        extra.append(hi + rng.uniform(0.15, 0.5, (strays, 3)))
        extra_obj += [o] * strays
    coord_h = np.concatenate([coord_h] + extra).astype(np.float32)
    obj_h = np.concatenate([obj_h, np.array(extra_obj, np.int32)]).astype(np.int32)
    perm = rng.permutation(len(obj_h))
    return coord_h[perm], obj_h[perm], n_objects, n_boxes


def parts_ms(coord, obj, n_objects, reps, warmup):
    """the steps of clean_supports one by one: its own step functions, in its order, on the prologue's result"""
    call = cluster._Call("clean_supports", cluster.LAST_SUPPORTS, coord, obj)
    voxel, r, r2, nb_points = cluster._support_settings(call.who, cluster.SUPPORT_VOXEL, cluster.SUPPORT_RADIUS, cluster.SUPPORT_NB_POINTS)
    p = cluster._labelled(call, coord, obj, n_objects, "n_objects")
    vdims = cluster._voxel_dims(call.who, p.n_labels, p.origin, p.top, voxel)
    cell, dims = cluster._dims(call.who, p.n_labels, p.origin, p.top, r)

    def compact():
        alive, n_kept, n_alive = cluster._survivors(call, keep, mean_object, p.n_labels)
        return cluster._compact(mean, mean_object, keep, alive, n_kept, n_alive)

    out = {}
    out["boxes_ms"], _, (lo, _, _) = timing.device_ms(lambda: cluster._boxes(call, p), reps, warmup)
    out["keys_sort_ms"], _, (skeys, order, slot, n_voxels) = timing.device_ms(lambda: cluster._voxel_means(call, p, lo, voxel, vdims), reps, warmup)
    out["means_ms"], _, (mean, mean_object, mean_size) = timing.device_ms(lambda: cluster._means(call, p, n_voxels, skeys, order, slot), reps, warmup)
    out["grid_ms"], _, (pts, _, _, ranges) = timing.device_ms(
        lambda: cluster._grid(call, mean, mean_object, p.n_labels, n_voxels, p.origin, cell, dims), reps, warmup)
    out["count_ms"], _, keep = timing.device_ms(lambda: cluster._inliers(call, pts, ranges, r2, nb_points), reps, warmup)
    out["compact_ms"], _, _ = timing.device_ms(compact, reps, warmup)
    out = {k: round(v, 4) for k, v in out.items()}
    out.update(voxel_dims=vdims, cells=dims, labelled_points=p.n_valid, voxels=n_voxels, longest_run=int(mean_size.max().item()),
               mean_run=round(p.n_valid / n_voxels, 3))
    return out


def host_loop(coord_h, obj_h, n_objects, tree):
    """the oracle's per-object loop -> (points, object, source, n); tree: scipy's cKDTree for the counts, None = the oracle's dense matrix"""
    from tests import supports_oracle
    if tree is None:
        return supports_oracle.clean_supports(coord_h, obj_h, n_objects)
    points, objects, source = [], [], []
    for o in range(n_objects):
        mine = coord_h[obj_h == o]
        if len(mine) == 0:
            continue
        _, mean, _ = supports_oracle.voxel_means(mine, cluster.SUPPORT_VOXEL)
        near = tree(mean.astype(np.float64)).query_ball_point(mean.astype(np.float64), cluster.SUPPORT_RADIUS, return_length=True)
        kept = mean[near > cluster.SUPPORT_NB_POINTS]
        if len(kept):
            points.append(kept)
            objects.append(np.full(len(kept), len(source), np.int32))
            source.append(o)
    return np.concatenate(points), np.concatenate(objects), np.array(source, np.int32), len(source)


def timed_host(coord_h, obj_h, n_objects, tree):
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = host_loop(coord_h, obj_h, n_objects, tree)
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--strays", type=int, default=40)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=12000)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timing.need_gpu("bench_supports")
    if a.reps < 20:
        raise SystemExit("bench_supports: at least 20 timed calls")
    coord_h, obj_h, n_objects, n_boxes = scene_with_strays(a.points, a.strays)
    coord, obj = torch.from_numpy(coord_h).cuda(), torch.from_numpy(obj_h).cuda()
    ms, host_ms, (points, new_obj, source, n_new) = timing.device_ms(lambda: cluster.clean_supports(coord, obj, n_objects), a.reps, a.warmup)
    calls = dict(cluster.LAST_SUPPORTS)
    result = {"tool": "bench_supports", "device": torch.cuda.get_device_name(0), "points": len(coord_h), "boxes": n_boxes, "objects": n_objects,
              "strays_per_object": a.strays, "voxel": cluster.SUPPORT_VOXEL, "radius": cluster.SUPPORT_RADIUS,
              "nb_points": cluster.SUPPORT_NB_POINTS, "reps": a.reps, "warmup": a.warmup, "supports_ms": round(ms, 4),
              "supports_host_ms": round(host_ms, 4), "library_launches": calls["launches"], "readbacks": calls["readbacks"],
              "kept": int(points.shape[0]), "objects_left": n_new}
    result.update(parts_ms(coord, obj, n_objects, a.reps, a.warmup))
    result["removed"] = result["voxels"] - result["kept"]
    if not a.no_host:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        if cKDTree is not None:
            loop_ms, want = timed_host(coord_h, obj_h, n_objects, cKDTree)
            same_shape = want[0].shape == tuple(points.shape)
            result.update(host_counts="ckdtree", host_points=len(coord_h), host_loop_ms=round(loop_ms, 2), host_kept=int(len(want[0])),
                          host_agrees=bool(same_shape and np.array_equal(want[0].view(np.int32), points.cpu().numpy().view(np.int32))
                                           and np.array_equal(want[1], new_obj.cpu().numpy())),
                          ratio_to_host_loop=round(loop_ms / ms, 1))
        else:
            small_h, small_obj_h, small_n, small_boxes = scene_with_strays(a.host_points, a.strays)
            small, small_obj = torch.from_numpy(small_h).cuda(), torch.from_numpy(small_obj_h).cuda()
            small_ms, small_host_ms, got = timing.device_ms(lambda: cluster.clean_supports(small, small_obj, small_n), a.reps, a.warmup)
            loop_ms, want = timed_host(small_h, small_obj_h, small_n, None)
            result.update(host_counts="dense", host_points=len(small_h), small_boxes=small_boxes, small_objects=small_n,
                          small_supports_ms=round(small_ms, 4), small_supports_host_ms=round(small_host_ms, 4),
                          host_loop_ms=round(loop_ms, 2), host_kept=int(len(want[0])), small_kept=int(got[0].shape[0]),
                          host_agrees=bool(want[0].shape == tuple(got[0].shape) and np.array_equal(want[0].view(np.int32), got[0].cpu().numpy().view(np.int32))
                                           and np.array_equal(want[1], got[1].cpu().numpy())),
                          ratio_to_host_loop=round(loop_ms / small_ms, 1))
    result["not_measured"] = NOT_MEASURED
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
