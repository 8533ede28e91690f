"""The train-time augmentations on the device (stratified_transformer_amd.augment on csrc/augment.hip) against the host and against plain
torch: the S3DIS training chain and the full chain of tests/augment_cases.py (elastic x2, flip, rotate, scale, auto-contrast, colour
translation, colour jitter, hue / saturation), on one 100 000-point room and on a 600 000-row batch of six rooms, float32 and float64.
Prints ONE JSON line (GPU box only; a missing GPU is an error).  There is no threshold: the numbers are reported as they come out.

    python tools/bench_augment.py [--points 100000] [--scenes 6] [--reps 30] [--warmup 3] [--host-reps 3] [--out profiles/augment_bench.json]

Per (chain, shape, dtype):
  fused_ms       median over `reps` calls, after `warmup`, of t(coord, feat, offset, rng=..., generator=...) with fresh draws every call:
                 device events around the call; fused_host_ms the host clock around the same calls (a call with ElasticDistortion ends
                 each of its read-backs in a synchronisation, so the two are close); *_spread = [min, lower quartile, upper quartile, max]
  torch_ms       the same chain written as plain torch device ops in the storage dtype, scene by scene (the reference's expressions on
                 tensors, torch's own min / max / matmul; elastic with padded slices for the box filters and a gather for the trilinear
                 sample), replaying the draws of the last fused call; timed the same way, in the same run, alternating with the fused call
  torch_max_diff the largest absolute difference between the two results (coord, feat) - a sanity check, not a bound: torch computes in
                 the storage dtype and in its own order
  host_ms        the numpy restatement (tests/augment_oracle.py, float64, scene by scene) with the same draws: median of `host-reps`
                 runs on this machine's host, host clock; host_upload_ms: the copy of its result to the device, which a host pipeline pays
  passes, readbacks   of the fused call (augment.Transform.last_counts)
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import augment as A, scene  # noqa: E402
from tests import augment_cases as cases  # noqa: E402
from tests import augment_oracle as O  # noqa: E402

NOT_MEASURED = ["a per-kernel profile (no run under rocprofv3 was taken)", "batches of more than 6 scenes", "achieved bytes per second",
                "the loader's end-to-end step time with and without the device chain"]


# ---- the chains as plain torch ops on one scene (storage dtype), replaying the draws `d` (tests/augment_cases.scene_draws' layout) ----
def _t(v, like):
    return torch.as_tensor(np.asarray(v), dtype=like.dtype, device=like.device)


def torch_blur(g):
    for _ in range(2):
        for axis in range(3):
            p = torch.nn.functional.pad(g.movedim(axis, 0), (0, 0) * (g.dim() - 1) + (1, 1)).movedim(0, axis)
            n = g.shape[axis]
            g = (p.narrow(axis, 0, n) + p.narrow(axis, 1, n) + p.narrow(axis, 2, n)) / 3
    return g


def torch_elastic(c, granularity, magnitude, noise):
    lo = c.min(0)[0]
    dim = noise.shape[:3]
    grid = torch_blur(noise.to(c.dtype))
    u = (c - (lo - granularity)) / granularity                       # node coordinates: the axes are evenly spaced
    i = [u[:, k].floor().long().clamp(0, dim[k] - 2) for k in range(3)]
    y = [u[:, k] - i[k] for k in range(3)]
    value = torch.zeros_like(c)
    for corner in range(8):
        b = [(corner >> 2) & 1, (corner >> 1) & 1, corner & 1]
        w = torch.ones_like(y[0])
        for k in range(3):
            w = w * (y[k] if b[k] else 1 - y[k])
        value = value + grid[i[0] + b[0], i[1] + b[1], i[2] + b[2]] * w[:, None]
    return c + value * magnitude


def torch_hue_saturation(f, hue_val, sat_ratio):
    rgb = (f + 1.0) * 127.5
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    maxc, minc = rgb.max(1)[0], rgb.min(1)[0]
    mask = maxc != minc
    span = torch.where(mask, maxc - minc, torch.ones_like(maxc))
    s = torch.where(mask, span / maxc, torch.zeros_like(maxc))
    rc, gc, bc = [torch.where(mask, (maxc - x) / span, torch.zeros_like(x)) for x in (r, g, b)]
    h = torch.where(r == maxc, bc - gc, torch.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
    h = torch.remainder(h / 6.0, 1.0)
    h = torch.remainder(hue_val + h + 1, 1)
    s = (sat_ratio * s).clamp(0, 1)
    v = maxc
    i = (h * 6.0).to(torch.uint8)
    fr = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * fr), v * (1.0 - s * (1.0 - fr))
    i = i % 6
    grey = s == 0.0
    pick = lambda options: torch.where(grey, v, torch.stack(options, 1).gather(1, i.long()[:, None])[:, 0])
    out = torch.stack([pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])], 1)
    return out.to(torch.uint8).to(f.dtype) / 127.5 - 1


def torch_chain(spec, c, f, ds):
    for (name, kw), d in zip(spec, ds):
        if name == "RandomRotate":
            c = c @ _t(O.rotate_matrix(d["u"] * 2 * np.pi, kw.get("along_z", True)), c)
        elif name == "RandomScale":
            c = c * float(d["scale"])
        elif name == "RandomJitter":
            c = c + (kw["sigma"] * d["noise"].to(c.dtype)).clamp(-kw["clip"], kw["clip"])
        elif name == "RandomDropColor":
            if d["u"] > kw.get("p", 0.8):
                f = f * kw["color_augment"]
        elif name == "ElasticDistortion":
            if d["gate"] < 0.95:
                for (granularity, magnitude), noise in zip(kw["distortion_params"], d["noise"]):
                    c = torch_elastic(c, granularity, magnitude, noise)
        elif name == "RandomHorizontalFlip":
            if d["gate"] < 0.95:
                c = c.clone()
                for ax, u in zip((0, 1), d["axes"]):
                    if u < 0.5:
                        c[:, ax] = c[:, ax].max() - c[:, ax]
        elif name == "ChromaticAutoContrast":
            f = (f + 1.0) * 127.5
            if d["gate"] < 0.2:
                lo, hi = f.min(0, keepdim=True)[0], f.max(0, keepdim=True)[0]
                f = (1 - float(d["blend"])) * f + float(d["blend"]) * ((f - lo) * (255 / (hi - lo)))
            f = f / 127.5 - 1
        elif name == "ChromaticTranslation":
            f = (f + 1.0) * 127.5
            if d["gate"] < 0.95:
                f = (_t((np.asarray(d["u"]).reshape(1, 3) - 0.5) * 255 * 2 * kw["trans_range_ratio"], f) + f).clamp(0, 255)
            f = f / 127.5 - 1
        elif name == "ChromaticJitter":
            f = (f + 1.0) * 127.5
            if d["gate"] < 0.95:
                f = (d["noise"].to(f.dtype) * (kw["std"] * 255) + f).clamp(0, 255)
            f = f / 127.5 - 1
        elif name == "HueSaturationTranslation":
            f = torch_hue_saturation(f, (float(d["hue_u"]) - 0.5) * 2 * kw["hue_max"], 1 + (float(d["sat_u"]) - 0.5) * 2 * kw["saturation_max"])
        else:
            raise KeyError(name)
    return c, f


def device_draws(records, s, lo, hi):
    """tests/augment_cases.scene_draws without the copies to the host: noise stays on the device"""
    out = []
    for rec in records:
        d = {}
        for k, v in rec.items():
            if k == "noise" and isinstance(v, list):
                d[k] = [e[s] for e in v if e[s] is not None]
            elif isinstance(v, torch.Tensor):
                d[k] = v[lo:hi]
            else:
                d[k] = np.asarray(v)[s]
        out.append(d)
    return out


def torch_batch(spec, coord, feat, ends, records):
    cs, fs, lo = [], [], 0
    for s, hi in enumerate(ends):
        c, f = torch_chain(spec, coord[lo:hi], feat[lo:hi], device_draws(records, s, lo, hi))
        cs.append(c)
        fs.append(f)
        lo = hi
    return torch.cat(cs), torch.cat(fs)


def host_batch(spec, coord, feat, ends, draws):
    cs, fs, lo = [], [], 0
    with np.errstate(all="ignore"):
        for s, hi in enumerate(ends):
            c, f = O.Compose(cases.build(O, spec))(coord[lo:hi], feat[lo:hi], draws[s])
            cs.append(c)
            fs.append(f)
            lo = hi
    return np.concatenate(cs), np.concatenate(fs)


def measure(spec, coord_h, feat_h, ends, dtype, reps, warmup, host_reps):
    coord, feat = torch.from_numpy(coord_h).cuda().to(dtype), torch.from_numpy(feat_h).cuda().to(dtype)
    offset = torch.tensor(ends, dtype=torch.int32, device="cuda")
    t = A.Compose(cases.build(A, spec))
    rng, gen = np.random.default_rng(0), torch.Generator(device="cuda").manual_seed(0)
    t(coord, feat, offset, rng=rng, generator=gen)
    records = t.last_draws.records
    (fd, fh, _), (td, th, tres) = timing.calls([lambda: t(coord, feat, offset, rng=rng, generator=gen),
                                               lambda: torch_batch(spec, coord, feat, ends, records)], reps, warmup)
    got = t(coord, feat, offset, draws=A.Draws(records))
    diff = max(float((got[0] - tres[0]).abs().nan_to_num(0).max()), float((got[1] - tres[1]).abs().nan_to_num(0).max()))
    draws, lo = [], 0
    for s, hi in enumerate(ends):
        draws.append(cases.scene_draws(records, s, lo, hi))
        lo = hi
    seen_c, seen_f = coord.double().cpu().numpy(), feat.double().cpu().numpy()
    host_t, up_t = [], []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        hc, hf = host_batch(spec, seen_c, seen_f, ends, draws)
        host_t.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        torch.from_numpy(hc).to(dtype).cuda(), torch.from_numpy(hf).to(dtype).cuda()
        torch.cuda.synchronize()
        up_t.append((time.perf_counter() - t0) * 1e3)
    same = bool(cases.same_bits(got[0].cpu().numpy(), hc.astype(coord_h.dtype if dtype == torch.float64 else np.float32))
                and cases.same_bits(got[1].cpu().numpy(), hf.astype(np.float64 if dtype == torch.float64 else np.float32)))
    return {"rows": int(ends[-1]), "scenes": len(ends), "dtype": str(dtype).split(".")[1], "passes": t.last_counts["passes"],
            "readbacks": t.last_counts["readbacks"], "fused_ms": round(statistics.median(fd), 4), "fused_ms_spread": timing.spread(fd),
            "fused_host_ms": round(statistics.median(fh), 4), "torch_ms": round(statistics.median(td), 4), "torch_ms_spread": timing.spread(td),
            "torch_host_ms": round(statistics.median(th), 4), "torch_max_diff": diff, "host_ms": round(statistics.median(host_t), 2),
            "host_ms_spread": [round(min(host_t), 2), round(max(host_t), 2)], "host_upload_ms": round(statistics.median(up_t), 3),
            "bitwise_equal_to_host": same, "torch_over_fused": round(statistics.median(td) / statistics.median(fd), 2),
            "host_over_fused": round(statistics.median(host_t) / statistics.median(fd), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--scenes", type=int, default=6)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timing.need_gpu("bench_augment")
    if a.reps < 20:
        raise SystemExit("bench_augment: at least 20 timed calls")
    rooms = [scene.make_room(a.points, seed=s).astype(np.float64) for s in range(a.scenes)]
    rng = np.random.default_rng(1)
    feats = [cases.narrow(rng.integers(0, 256, (a.points, 3)) / 127.5 - 1) for _ in rooms]
    shapes = {"room": (rooms[0], feats[0], [a.points]),
              "batch": (np.concatenate(rooms), np.concatenate(feats), [a.points * (s + 1) for s in range(a.scenes)])}
    result = {"tool": "bench_augment", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "host_reps": a.host_reps,
              "results": {}}
    for chain_name, spec in (("s3dis", cases.S3DIS_CHAIN), ("full", cases.FULL_CHAIN)):
        for shape_name, (c, f, ends) in shapes.items():
            for dtype in (torch.float32, torch.float64):
                key = f"{chain_name}.{shape_name}.{str(dtype).split('.')[1]}"
                result["results"][key] = measure(spec, c, f, ends, dtype, a.reps, a.warmup, a.host_reps)
                print(key, json.dumps(result["results"][key]), file=sys.stderr, flush=True)
    result["not_measured"] = NOT_MEASURED
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
