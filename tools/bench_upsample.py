"""The decoder (model/stratified_transformer.py:329-342): the stand-in Upsample as the operator API runs it (two Sequential(LayerNorm, Linear),
pointops.interpolation, one add) beside the same module with layers.upsample_forward installed (the LayerNorms on pointops.residual_norm,
pointops.interpolate_add: csrc/upsample.hip), in one process on the same GPU and inputs, the two sides alternating window by window.
Prints ONE JSON line and writes it to --out (GPU box only; a missing GPU is an error).

    python tools/bench_upsample.py [--points 100000] [--reps 30] [--warmup 5] [--out profiles/upsample_bench.json]

Scene: a surface room and its FPS chain at ratio 0.25, which gives the three S3DIS decoder sites: 25 001 -> 100 000 points with 96 -> 48
channels, 6 251 -> 25 001 with 192 -> 96, 1 563 -> 6 251 with 384 -> 192.  Modes: fp32 and autocast(f16).  Per site and mode:
  layer       forward + backward of the whole module (kNN search included: it is the same call on both sides), gradients of both feature
              inputs and all parameters
  gather_add  forward + backward of pointops.gather_add(b, idx, w, a) against _WeightedGather(b, idx, w) + a - what `interpolation` runs
              behind its search - on fixed indices and weights, b and a in the mode's dtype (f16: the parent's side makes its fp32 copy)
each as median and spread (max - min) over `reps` windows of one call, events on the stream, gradients cleared outside the window;
`ratio` = parent / new (> 1: the new path is faster) and `faster_beyond_spread` as timing.summary defines them.
"""
import argparse
import os

import torch

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import index_build, layers, pointops as P, scene  # noqa: E402
from tests import decoder_standin  # noqa: E402

RATIO, K = 0.25, 3


class Installed(decoder_standin.Upsample):
    """the class layers.upsample_forward is bound to; the unpatched side stays decoder_standin.Upsample itself"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(timing.ROOT, "profiles", "upsample_bench.json"))
    a = ap.parse_args()
    timing.need_gpu("bench_upsample")
    clouds, off_host = [torch.from_numpy(scene.make_room(a.points, 0)).cuda()], [[a.points]]
    for _ in range(3):
        xyz, off = clouds[-1], off_host[-1]
        n_off = index_build.transition_down_offset(off, RATIO)
        idx = P.furthestsampling(xyz, torch.tensor(off, dtype=torch.int32, device="cuda"), torch.tensor(n_off, dtype=torch.int32, device="cuda"))
        clouds.append(xyz[idx.long(), :].contiguous())
        off_host.append(n_off)
    result = {"tool": "bench_upsample", "device": torch.cuda.get_device_name(0), "points": a.points, "k": K, "reps": a.reps,
              "warmup": a.warmup, "sites": []}
    assert layers.patch_upsample_class(Installed) == [Installed]
    for level, (c_in, c_out) in enumerate(((96, 48), (192, 96), (384, 192))):
        support_xyz, xyz = clouds[level], clouds[level + 1]
        support_offset = torch.tensor(off_host[level], dtype=torch.int32, device="cuda")
        offset = torch.tensor(off_host[level + 1], dtype=torch.int32, device="cuda")
        n, m = support_xyz.shape[0], xyz.shape[0]
        torch.manual_seed(c_in)
        mods = {"unpatched": decoder_standin.Upsample(K, c_in, c_out).cuda(), "installed": Installed(K, c_in, c_out).cuda()}
        mods["installed"].load_state_dict(mods["unpatched"].state_dict())
        g = torch.Generator(device="cuda").manual_seed(c_in)
        feats = torch.randn(m, c_in, device="cuda", generator=g).requires_grad_(True)
        support_feats = torch.randn(n, c_out, device="cuda", generator=g).requires_grad_(True)
        go = torch.randn(n, c_out, device="cuda", generator=g)
        idx, dist = P.knnquery(K, xyz, support_xyz, offset, support_offset)
        w = P._inverse_distance_weights(dist).contiguous()
        row = {"m": m, "n": n, "c_in": c_in, "c_out": c_out}
        for mode, amp in (("fp32", False), ("autocast_f16", True)):
            # ---- the layer ----
            def clear():
                feats.grad = support_feats.grad = None
                for mod in mods.values():
                    mod.zero_grad(set_to_none=True)

            outs = {}

            def layer(side):
                with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                    out = mods[side](feats, xyz, support_xyz, offset, support_offset, support_feats)[0]
                out.backward(go)
                outs[side] = out.detach()

            times = timing.windows({s: (lambda s=s: layer(s)) for s in mods}, a.reps, a.warmup, prepare=clear)
            r = {"layer": timing.summary(times, "unpatched", "installed"),
                 "layer_max_abs_diff_out": float((outs["unpatched"] - outs["installed"]).abs().max())}
            # ---- the operator behind the search ----
            dt = torch.float16 if amp else torch.float32
            b = torch.randn(m, c_out, device="cuda", generator=g).to(dt).requires_grad_(True)
            base = torch.randn(n, c_out, device="cuda", generator=g).to(dt).requires_grad_(True)

            def clear_op():
                b.grad = base.grad = None

            def parent():
                out = P._WeightedGather.apply(*P._gather_operands(b, idx, w)) + base
                out.backward(go)
                outs["parent"] = out.detach()

            def gather_add():
                out = P.gather_add(b, idx, w, base)
                out.backward(go)
                outs["gather_add"] = out.detach()

            times = timing.windows({"parent": parent, "gather_add": gather_add}, a.reps, a.warmup, prepare=clear_op)
            r["gather_add"] = timing.summary(times, "parent", "gather_add")
            r["gather_add_max_abs_diff_out"] = float((outs["parent"] - outs["gather_add"]).abs().max())
            row[mode] = r
        result["sites"].append(row)
    layers.uninstall_fast_layers()
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
