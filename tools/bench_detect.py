"""The whole-scene box detection (stratified_transformer_amd.evaluate.detect_scene and its parts) on the box scene of
tools/bench_contacts.py: about 100k points, the reference's settings.  Prints ONE JSON line and writes it to --out (GPU box only; a
missing GPU is an error).

    python tools/bench_detect.py [--points 100000] [--rows 400000] [--classes 18] [--reps 30] [--warmup 3] [--host-points 12000] [--no-host]
                                 [--limit 300] [--out profiles/detect_bench.json]

`vote`: SceneVotes.add with and without the shift rows at m = `--rows` (5 x 80 000: one batch of the fork's test loop) and `--classes`
classes on m / 2 points, random f32 logits and shifts; the two objects take turns inside ONE loop in one process, device events around
each call, medians over `reps` turns after `warmup`; `extra_ms` is the difference of the medians, `shift_bytes` what the second accumulator
moves at most (m rows read, m rows read-modify-written).
`dense_points_ms`, `detect_boxes_ms`, `detect_scene_ms`: medians of whole calls, a host clock around work that ends in a device
synchronise (every one of them reads back); the model of detect_scene is a table lookup (logits = 8 * one_hot(table[i]), shift =
shift_table[i], the point's index in the one feature column), so the time is the pass around the model: tiling, ball query, votes, boxes.
`host`: the same pass through the numpy restatement (tests/detect_oracle.py: scene_predict, then the chain of the four oracles) on the
same machine in the same run, on a scene of `--host-points` points - the oracles are quadratic - with the device's times on that same
scene (`small_*`) and whether the boxes agree.
Every GPU step runs under its own time limit (`--limit` seconds, SIGALRM ends the process: nothing more is started on the device)."""
import argparse
import os
import statistics
import time

import numpy as np
import torch

import timing  # first: it puts the repository root on sys.path
from bench_contacts import make_scene  # noqa: E402
from stratified_transformer_amd import cluster, evaluate  # noqa: E402

NOT_MEASURED = ["a per-kernel profile (no run under rocprofv3 was taken)", "scenes of more than about 100k points", "a real model behind model_fn",
                "half-precision logits or shifts", "scenes whose parts exceed voxel_max (the crop cover: tools/bench_evaltile.py)"]


def vote_bench(m, classes, reps, warmup):
    n_points = max(m // 2, 1)
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(m, classes, device="cuda", generator=g) * 3.0
    shift = torch.randn(m, 3, device="cuda", generator=g)
    idx = torch.randint(0, n_points, (m,), device="cuda", generator=g)
    plain, both = evaluate.SceneVotes(n_points, classes), evaluate.SceneVotes(n_points, classes, shifts=True)
    arms = {"vote_ms": lambda: plain.add(logits, idx), "vote_shift_ms": lambda: both.add(logits, idx, shift)}
    # the arms take turns: one process, one device, the same clocks
    times = {name: dev for name, (dev, _, _) in zip(arms, timing.calls(list(arms.values()), reps, warmup))}
    out = {k: round(statistics.median(v), 4) for k, v in times.items()}
    out.update({k.replace("_ms", "_ms_min"): round(min(v), 4) for k, v in times.items()})
    out.update(rows=m, classes=classes, points=n_points, extra_ms=round(out["vote_shift_ms"] - out["vote_ms"], 4), shift_bytes=m * 12 * 3,
               same_votes=bool(torch.equal(plain.pred, both.pred)))
    return out


def lookup_model(table, shift_table, classes):
    def model_fn(feat, coord, offset, batch, neighbor_idx):
        i = feat[:, 0].long()
        return 8.0 * torch.nn.functional.one_hot(table[i], classes).float(), shift_table[i]
    return model_fn


def device_pass(coord_h, pred_h, classes, reps, warmup, voxel_size, voxel_max):
    n = len(coord_h)
    coord, table = torch.from_numpy(coord_h).cuda(), torch.from_numpy(pred_h).cuda()
    shift_table = torch.from_numpy(np.random.default_rng(1).normal(0, 0.002, (n, 3)).astype(np.float32)).cuda()
    feat = torch.arange(n, dtype=torch.float32, device="cuda")[:, None]
    model = lookup_model(table, shift_table, classes)
    out = {"points": n}
    out["dense_points_ms"] = round(timing.median_wall_ms(lambda: evaluate.dense_points(coord), reps, warmup), 4)
    out["dense_points_kept"] = int(evaluate.dense_points(coord)[1].shape[0])
    out["detect_boxes_ms"] = round(timing.median_wall_ms(lambda: cluster.detect_boxes(coord, shift_table, table), reps, warmup), 4)
    run = lambda: evaluate.detect_scene(model, coord, feat, voxel_size, voxel_max, classes, 0.04, feat_div=None)  # noqa: E731
    out["detect_scene_ms"] = round(timing.median_wall_ms(run, reps, warmup), 4)
    got = run()
    out.update(sets=got.n_sets, support_points=int(got.points.shape[0]), labels_right=bool(torch.equal(got.label, table)))
    return out, got, shift_table.cpu().numpy()


def host_pass(coord_h, pred_h, shift_h, classes, voxel_size, voxel_max):
    from oracle import index_ref
    from tests import detect_oracle as D
    n = len(coord_h)
    feat = np.arange(n, dtype=np.float32)[:, None]
    t0 = time.perf_counter()
    pred, shift, _, n_crops = D.scene_predict(D.lookup_model(pred_h, shift_h, classes), coord_h, feat, lambda c, v: index_ref.voxelize(c, v, 1), voxel_size,
                                              voxel_max, classes, feat_div=None, priority=None)
    t1 = time.perf_counter()
    want = D.chain(coord_h, shift, pred.argmax(1))
    t2 = time.perf_counter()
    return {"predict_ms": round((t1 - t0) * 1e3, 2), "chain_ms": round((t2 - t1) * 1e3, 2), "total_ms": round((t2 - t0) * 1e3, 2), "crops": n_crops,
            "cores": len(os.sched_getaffinity(0)), "numpy": np.__version__}, want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=400000)
    ap.add_argument("--classes", type=int, default=18)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=12000)
    ap.add_argument("--voxel-size", type=float, default=0.04)
    ap.add_argument("--voxel-max", type=int, default=80000)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(timing.ROOT, "profiles", "detect_bench.json"))
    a = ap.parse_args()
    timing.need_gpu("bench_detect")
    result = {"tool": "bench_detect", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "voxel_size": a.voxel_size,
              "voxel_max": a.voxel_max}
    with timing.limited(a.limit):
        result["vote"] = vote_bench(a.rows, a.classes, a.reps, a.warmup)
    coord_h, pred_h, n_boxes = make_scene(a.points)
    with timing.limited(a.limit):
        result["scene"], _, _ = device_pass(coord_h, pred_h, 18, a.reps, a.warmup, a.voxel_size, a.voxel_max)
    result["scene"]["boxes"] = n_boxes
    if not a.no_host:
        small_h, small_pred_h, small_boxes = make_scene(a.host_points)
        with timing.limited(a.limit):
            small, got, shift_h = device_pass(small_h, small_pred_h, 18, a.reps, a.warmup, a.voxel_size, a.voxel_max)
        host, want = host_pass(small_h, small_pred_h, shift_h, 18, a.voxel_size, a.voxel_max)
        host.update(points=len(small_h), boxes=small_boxes, small_dense_points_ms=small["dense_points_ms"], small_detect_boxes_ms=small["detect_boxes_ms"],
                    small_detect_scene_ms=small["detect_scene_ms"], sets=len(want["merge"][1]),
                    agrees=bool(np.array_equal(got.boxes.cpu().numpy(), want["merge"][2])),
                    ratio_to_host_pass=round(host["total_ms"] / small["detect_scene_ms"], 1))
        result["host"] = host
    result["not_measured"] = NOT_MEASURED
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
