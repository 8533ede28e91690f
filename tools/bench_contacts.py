"""The grouping behind the clustering (stratified_transformer_amd.cluster.objects / contacts on csrc/contacts.hip) on a scene of boxes:
about 100k points, 40 % of them edge points, the reference's settings (radius 0.08, share 0.5).  Prints ONE JSON line (GPU box only; a
missing GPU is an error).

    python tools/bench_contacts.py [--points 100000] [--reps 30] [--warmup 3] [--no-host] [--out profiles/contacts_bench.json]

The instances come from cluster.instances on the same scene with a zero shift (not timed).  `objects_ms`, `contacts_ms` (count and the
quadratic min_d2 sweep) and `count_ms` (the grid and its walk alone, the step objects runs behind its read-back up front): medians over `reps` calls after `warmup` calls, device
events around the call; objects() ends in a read-back, so `objects_host_ms` gives the host clock around the same calls as well.
`host_loop_ms`: the pairing loop of `instantiation_eval` (util/train_utils.py:601-647) as tests/contacts_oracle.pair_list restates it,
with one scipy.spatial.distance.cdist per (edge instance, face instance) as the reference computes it, on the same instances and the
same machine (median of 3; needs scipy).  The per-kernel split is taken in a run of its own under `rocprofv3 --kernel-trace --stats`."""
import argparse
import statistics
import time

import numpy as np
import torch

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import cluster  # noqa: E402

FACE = {0: (2, 1), 5: (2, 0), 1: (0, 1), 4: (0, 0), 2: (1, 1), 3: (1, 0)}   # face class -> (axis, side)


def box(rng, lo, size, edge_points):
    """faces on a 0.025 grid (inset 0.05, jittered inside the plane), edge_points per edge; classes as in tests/golden/make_golden_objects.py"""
    lo = np.asarray(lo, float)
    hi = lo + np.asarray(size, float)
    coord, pred = [], []
    for c, (axis, side) in FACE.items():
        u, v = [a for a in range(3) if a != axis]
        uu, vv = np.meshgrid(np.arange(lo[u] + 0.05, hi[u] - 0.05 + 1e-9, 0.025), np.arange(lo[v] + 0.05, hi[v] - 0.05 + 1e-9, 0.025), indexing="ij")
        p = np.zeros((uu.size, 3))
        p[:, u], p[:, v], p[:, axis] = uu.ravel(), vv.ravel(), hi[axis] if side else lo[axis]
        p[:, [u, v]] += rng.uniform(-0.004, 0.004, (len(p), 2))
        coord.append(p)
        pred += [c] * len(p)
    for e, (f1, f2) in enumerate(cluster.EDGE_FACES):
        (a1, s1), (a2, s2) = FACE[f1], FACE[f2]
        along = 3 - a1 - a2
        p = np.zeros((edge_points, 3))
        p[:, along] = np.linspace(lo[along] + 0.01, hi[along] - 0.01, edge_points)
        p[:, a1], p[:, a2] = hi[a1] if s1 else lo[a1], hi[a2] if s2 else lo[a2]
        p += rng.normal(0, 0.004, p.shape)
        coord.append(p)
        pred += [6 + e] * edge_points
    return np.concatenate(coord), np.array(pred, np.int64)


def make_scene(points, seed=0):
    """boxes of 0.8 x 0.7 x 0.6 on a floor grid, 1.3 apart, until `points` are reached; 40 % edge points"""
    rng = np.random.default_rng(seed)
    probe, _ = box(rng, (0, 0, 0), (0.8, 0.7, 0.6), 1)
    face_points = len(probe) - 12
    edge_points = int(round(face_points * 0.4 / 0.6 / 12))
    n_boxes = max(1, int(round(points / (face_points + 12 * edge_points))))
    side = int(np.ceil(np.sqrt(n_boxes)))
    parts = [box(rng, (1.3 * (b % side), 1.3 * (b // side), 0.0), (0.8, 0.7, 0.6), edge_points) for b in range(n_boxes)]
    coord, pred = np.concatenate([p[0] for p in parts]).astype(np.float32), np.concatenate([p[1] for p in parts])
    perm = rng.permutation(len(pred))
    return coord[perm], pred[perm], n_boxes


def host_loop(coord, instance, cls, size):
    """the reference's pairing loop with its dense cdist per pair -> the list of linked face instances per edge"""
    from scipy.spatial import distance
    x = coord.astype(np.float64)
    supp = [x[instance == i] for i in range(len(cls))]
    of_class = [np.nonzero(cls == c)[0].tolist() for c in range(6)]
    pairs = []
    for c, (f1, f2) in enumerate(cluster.EDGE_FACES):
        if not of_class[f1] or not of_class[f2]:
            continue
        for e in np.nonzero(cls == 6 + c)[0].tolist():
            paired = []
            for ids in (of_class[f1], of_class[f2]):
                for k in ids:
                    d = np.min(distance.cdist(supp[e], supp[k]), axis=1)
                    if np.sum(d < 0.08) / len(d) > 0.5:
                        paired.append(k)
                        break
            if paired:
                pairs.append(paired)
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host loop (the profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timing.need_gpu("bench_contacts")
    coord_h, pred_h, n_boxes = make_scene(a.points)
    coord, pred = torch.from_numpy(coord_h).cuda(), torch.from_numpy(pred_h).cuda()
    instance, cls, size = cluster.instances(coord, torch.zeros_like(coord), pred)
    n_inst = int(cls.numel())

    objects_ms, objects_host_ms, (obj, object_of, n_objects) = timing.device_ms(lambda: cluster.objects(coord, instance, cls, size), a.reps, a.warmup)
    objects_calls = dict(cluster.LAST_CONTACTS)
    contacts_ms, contacts_host_ms, (count, min_d2) = timing.device_ms(lambda: cluster.contacts(coord, instance, 0.08, n_inst), a.reps, a.warmup)
    contacts_calls = dict(cluster.LAST_CONTACTS)
    call = cluster._Call("objects", cluster.LAST_CONTACTS, coord, instance)         # objects' count step, on its prologue's result
    r, r2 = cluster._radius(call.who, 0.08)
    p = cluster._labelled(call, coord, instance, n_inst)
    count_ms, count_host_ms, _ = timing.device_ms(lambda: cluster._contact_tables(call, p, r, r2, False), a.reps, a.warmup)

    result = {"tool": "bench_contacts", "device": torch.cuda.get_device_name(0), "points": len(coord_h), "boxes": n_boxes,
              "edge_point_share": round(float((pred_h >= 6).mean()), 4), "instances": n_inst, "face_instances": int((cls < 6).sum()),
              "edge_instances": int((cls >= 6).sum()), "objects": n_objects, "radius": 0.08, "share": 0.5, "reps": a.reps, "warmup": a.warmup,
              "objects_ms": round(objects_ms, 4), "objects_host_ms": round(objects_host_ms, 4),
              "contacts_ms": round(contacts_ms, 4), "contacts_host_ms": round(contacts_host_ms, 4),
              "count_ms": round(count_ms, 4), "count_host_ms": round(count_host_ms, 4),
              "objects_library_launches": objects_calls["launches"], "objects_readbacks": objects_calls["readbacks"],
              "contacts_library_launches": contacts_calls["launches"], "contacts_readbacks": contacts_calls["readbacks"],
              "pairs_in_contact": int((count > 0).sum().item()) - n_inst, "finite_min_d2": int(torch.isfinite(min_d2).sum().item())}
    if not a.no_host:
        inst_h, cls_h, size_h = instance.cpu().numpy(), cls.cpu().numpy(), size.cpu().numpy()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            pairs = host_loop(coord_h, inst_h, cls_h, size_h)
            times.append((time.perf_counter() - t0) * 1e3)
        result["host_loop_ms"] = round(statistics.median(times), 2)
        result["host_loop_links"] = len(pairs)
        linked = sorted({k for p in pairs for k in p})
        result["host_loop_agrees"] = bool(linked == np.nonzero((object_of.cpu().numpy() >= 0) & (cls_h < 6))[0].tolist())
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
