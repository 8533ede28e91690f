"""The clustering behind the model (stratified_transformer_amd.cluster.dbscan on csrc/dbscan.hip) on the 100k-point room of scene.py,
eight classes assigned by position, the reference's settings (classes below 6: eps 0.1 / min_samples 5, the others 0.15 / 3).
Prints ONE JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_dbscan.py [--points 100000] [--reps 30] [--warmup 3] [--out profiles/dbscan_bench.json]

`total_ms`: median over `reps` of a whole dbscan() call after `warmup` calls, a host clock around work that ends in a device
synchronise (the call reads back once per round of the component loop, so events alone would miss the host's share).  `phase_ms`: the
same call with a synchronise in front of every library launch, medians per phase (keys_and_sort: the key kernel and torch's sort;
components_and_ranking: every round with its read-back, then the ranking of the roots in torch); the bounding-box read-back in front of
the first launch is in total_ms only.
`instances_ms`: cluster.instances on the same cloud with a zero shift."""
import argparse
import statistics
import time

import numpy as np
import torch

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import _lib, cluster, scene  # noqa: E402

# a phase runs from its launcher's call to the next launcher's call, so it holds the torch work that follows the launch as well
PHASES = {"pointops2_dbscan_keys_launcher": "keys_and_sort", "pointops2_dbscan_prepare_launcher": "ranges",
          "pointops2_dbscan_core_launcher": "core", "pointops2_dbscan_round_launcher": "components_and_ranking",
          "pointops2_dbscan_label_launcher": "label"}


def classes_by_position(xyz, n_classes=8):
    """a 4 x 2 checkerboard of classes over the floor plan"""
    lo, hi = xyz.min(0), xyz.max(0)
    u = np.minimum(((xyz[:, 0] - lo[0]) / (hi[0] - lo[0]) * 4).astype(np.int64), 3)
    v = np.minimum(((xyz[:, 1] - lo[1]) / (hi[1] - lo[1]) * 2).astype(np.int64), 1)
    return (u * 2 + v) % n_classes


def phase_times(fn):
    """one call with a synchronise in front of every library launch: host time from phase start to the next phase's start"""
    marks, real = [], _lib.call

    def call(name, *args, **kw):
        torch.cuda.synchronize()
        marks.append((PHASES[name], time.perf_counter()))
        return real(name, *args, **kw)

    _lib.call = call
    try:
        fn()
        torch.cuda.synchronize()
        marks.append(("end", time.perf_counter()))
    finally:
        _lib.call = real
    out = {}
    for (name, t0), (_, t1) in zip(marks, marks[1:]):
        out[name] = out.get(name, 0.0) + (t1 - t0) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timing.need_gpu("bench_dbscan")
    room = scene.make_room(a.points, 0)
    pred_h = classes_by_position(room)
    xyz, pred = torch.from_numpy(room).cuda(), torch.from_numpy(pred_h).cuda()
    eps = [0.1] * 6 + [0.15] * 2
    ms = [5] * 6 + [3] * 2
    run = lambda: cluster.dbscan(xyz, eps, ms, pred)
    times, (labels, core, n_clusters) = timing.wall_times(run, a.reps, a.warmup)
    rounds, launches = cluster.LAST["rounds"], cluster.LAST["launches"]
    phases = [phase_times(run) for _ in range(a.reps)]
    zero = torch.zeros_like(xyz)
    inst_times = timing.wall_times(lambda: cluster.instances(xyz, zero, pred), a.reps, a.warmup)[0]
    inst = cluster.instances(xyz, zero, pred)
    result = {"tool": "bench_dbscan", "device": torch.cuda.get_device_name(0), "points": a.points, "classes": 8, "eps": eps, "min_samples": ms,
              "reps": a.reps, "warmup": a.warmup,
              "total_ms": round(statistics.median(times), 4), "total_ms_min": round(min(times), 4), "total_ms_max": round(max(times), 4),
              "phase_ms": {k: round(statistics.median(p[k] for p in phases), 4) for k in phases[0]},
              "rounds": rounds, "library_launches": launches,
              "instances_ms": round(statistics.median(inst_times), 4),
              "clusters_per_class": n_clusters.tolist(), "core_points": int(core.sum()), "noise_points": int((labels < 0).sum()),
              "instances": int(inst[1].numel())}
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
