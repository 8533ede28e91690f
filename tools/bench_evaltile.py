"""The crop cover of the whole-scene evaluation (stratified_transformer_amd.evaluate.crop_cover on csrc/evaltile.hip) on one part of a
large room - 400 000 points, voxel_max 80 000, the room generator of tests/evaltile_oracle.py - against the reference's numpy loop
(test_backup.py:239-251 as restated in tests/evaltile_oracle.crop_cover) timed on the host of the same machine in the same run.
Prints ONE JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_evaltile.py [--points 400000] [--voxel-max 80000] [--dtype f32] [--reps 10] [--warmup 2] [--limit 120]
                                   [--out profiles/evaltile_bench.json]

`device.total_ms`: median over `reps` of a whole crop_cover() call after `warmup` calls - a host clock around work that ends in a
device synchronise (the call reads back once per crop, so events alone would miss the host's share); `per_crop_ms` = total / crops.
`device.step_ms`: the steps of ONE crop timed on their own, each ending in a synchronise: the two kernels of seed_dist, torch's stable
sort of the n distances, the update kernel with its read-back.  `host`: the numpy loop, best of `--host-reps`, with the cores it may use.
`identical`: the device's crops, seeds and final priority equal the numpy loop's bit for bit at this size.
Every GPU step runs under its own time limit (`--limit` seconds, SIGALRM ends the process: nothing more is started on the device)."""
import argparse
import os
import statistics
import time

import numpy as np
import torch

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import _lib, evaluate  # noqa: E402
from stratified_transformer_amd._lib import ptr  # noqa: E402
from tests import evaltile_oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=400000)
    ap.add_argument("--voxel-max", type=int, default=80000)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(timing.ROOT, "profiles", "evaltile_bench.json"))
    a = ap.parse_args()
    timing.need_gpu("bench_evaltile")
    n, vm = a.points, a.voxel_max
    coord_h, priority_h = O.room(n, 0)
    coord_h = coord_h.astype(np.float32 if a.dtype == "f32" else np.float64)

    host_times = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        want = O.crop_cover(coord_h, vm, priority_h)
        host_times.append((time.perf_counter() - t0) * 1e3)
    n_crops = int(want[0].shape[0])

    coord, priority = torch.from_numpy(coord_h).cuda(), torch.from_numpy(priority_h).cuda()
    with timing.limited(a.limit):
        times = timing.wall_times(lambda: evaluate.crop_cover(coord, vm, priority), a.reps, a.warmup)[0]
        crops, seeds, final = evaluate.crop_cover(coord, vm, priority)
        identical = bool(np.array_equal(crops.cpu().numpy(), want[0]) and np.array_equal(seeds.cpu().numpy(), want[1])
                         and np.array_equal(final.cpu().numpy().view(np.uint64), want[2].view(np.uint64)))
        reads = evaluate.LAST["reads"]

    # the steps of one crop on their own
    is_f64 = int(a.dtype == "f64")
    parts = _lib.lib().pointops2_evaltile_max_parts()
    pv, pi = torch.empty(parts, dtype=torch.float64, device="cuda"), torch.empty(parts, dtype=torch.int32, device="cuda")
    seed, dist = torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=coord.dtype, device="cuda")
    covered, report, prio = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), priority.clone()
    seed_dist = lambda: _lib.call("pointops2_evaltile_seed_dist_launcher", n, is_f64, ptr(coord), ptr(prio), ptr(pv), ptr(pi), ptr(seed), ptr(dist),
                                  device=coord.device)
    with timing.limited(a.limit):
        seed_dist_ms = timing.median_wall_ms(seed_dist, a.reps, a.warmup)
        sort_ms = timing.median_wall_ms(lambda: torch.sort(dist, stable=True)[1][:vm].clone(), a.reps, a.warmup)
        crop = torch.sort(dist, stable=True)[1][:vm].clone()

        def update():
            _lib.call("pointops2_evaltile_update_launcher", n, vm, is_f64, ptr(dist), ptr(crop), ptr(prio), ptr(covered), ptr(report), device=coord.device)
            return report.tolist()
        update_ms = timing.median_wall_ms(update, a.reps, a.warmup)

    total = statistics.median(times)
    result = {"tool": "bench_evaltile", "device_name": torch.cuda.get_device_name(0), "points": n, "voxel_max": vm, "dtype": a.dtype, "crops": n_crops,
              "reps": a.reps, "warmup": a.warmup, "identical": identical, "read_backs": reads,
              "device": {"total_ms": round(total, 4), "total_ms_min": round(min(times), 4), "total_ms_max": round(max(times), 4),
                         "per_crop_ms": round(total / n_crops, 4),
                         "step_ms": {"seed_dist": round(seed_dist_ms, 4), "sort": round(sort_ms, 4), "update_and_read_back": round(update_ms, 4)}},
              "host": {"total_ms": round(min(host_times), 2), "per_crop_ms": round(min(host_times) / n_crops, 3), "reps": a.host_reps,
                       "cores": len(os.sched_getaffinity(0)), "numpy": np.__version__},
              "speedup_over_host_loop": round(min(host_times) / total, 2)}
    timing.emit(result, a.out)
    if not identical:
        raise SystemExit("bench_evaltile: the device's crops differ from the numpy loop's")


if __name__ == "__main__":
    main()
