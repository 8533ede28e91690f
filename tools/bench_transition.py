"""TransitionDown's tail (model/stratified_transformer.py:106-109): the composite the installed layer runs by default (gather the k rows of
every sampled point, LayerNorm + Linear on the m * k rows, transpose, MaxPool1d) beside the pooled form of layers.POOLED_TRANSITION
(LayerNorm + Linear on the N source rows, pointops.grouped_max: csrc/grouped_max.hip), on the same GPU, same inputs, geometry excluded.
Prints ONE JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_transition.py [--points 100000] [--reps 30] [--warmup 5] [--out FILE]

Scene: a surface room with its real FPS samples (ratio 0.25) and kNN-16 lists, down the three S3DIS transitions: 48 -> 96 at N,
96 -> 192 at N/4, 192 -> 384 at N/16.  Modes: fp32 and autocast(fp16).  Per shape, mode and side: median over `reps` of the forward and of
forward + backward (gradients of the features, the norm and the linear), each bracketed by events on the stream, the two sides
alternating; `ratio_*` = composite / pooled (> 1: the pooled tail is faster).
"""
import argparse

import torch

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import index_build, pointops as P, scene, standin  # noqa: E402

RATIO, K = 0.25, 16


def composite(td, feats, xyz, n_xyz, knn, offset, n_offset):
    """what layers.transition_down_forward executes from `queryandgroup` on with the flag off"""
    grouped = P.queryandgroup(K, xyz, n_xyz, feats.contiguous(), knn, offset, n_offset, use_xyz=False)
    m, k, c = grouped.shape
    rows = td.norm(grouped.view(m * k, c))
    return td.pool(td.linear(rows.view(m, k, c)).transpose(1, 2).contiguous()).squeeze(-1)


def pooled(td, feats, xyz, n_xyz, knn, offset, n_offset):
    """the same with layers.POOLED_TRANSITION"""
    return P.grouped_max(td.linear(td.norm(feats)).contiguous(), knn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timing.need_gpu("bench_transition")
    xyz = torch.from_numpy(scene.make_room(a.points, 0)).cuda()
    off_host = [a.points]
    result = {"tool": "bench_transition", "device": torch.cuda.get_device_name(0), "points": a.points, "k": K, "ratio": RATIO,
              "reps": a.reps, "warmup": a.warmup, "shapes": []}
    for c_in, c_out in ((48, 96), (96, 192), (192, 384)):
        n = xyz.shape[0]
        offset = torch.tensor(off_host, dtype=torch.int32, device="cuda")
        n_host = index_build.transition_down_offset(off_host, RATIO)
        n_offset = torch.tensor(n_host, dtype=torch.int32, device="cuda")
        n_xyz = xyz[P.furthestsampling(xyz, offset, n_offset).long(), :].contiguous()
        knn, _ = P.knnquery(K, xyz, n_xyz, offset, n_offset)
        knn = knn.contiguous()
        m = n_xyz.shape[0]
        torch.manual_seed(c_in)
        td = standin.TransitionDown(c_in, c_out, RATIO, K).cuda()
        g = torch.Generator(device="cuda").manual_seed(c_in)
        feats = torch.randn(n, c_in, device="cuda", generator=g).requires_grad_(True)
        go = torch.randn(m, c_out, device="cuda", generator=g)
        sides = {"pooled": lambda f: pooled(td, f, xyz, n_xyz, knn, offset, n_offset),
                 "composite": lambda f: composite(td, f, xyz, n_xyz, knn, offset, n_offset)}
        row = {"n": n, "m": m, "c_in": c_in, "c_out": c_out}

        def clear():
            feats.grad = None
            td.zero_grad(set_to_none=True)

        for mode, amp in (("fp32", False), ("autocast_f16", True)):
            def forward(fn):
                with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                    return fn(feats)

            times, last = timing.fwd_bwd_windows({s: (lambda fn=fn: forward(fn)) for s, fn in sides.items()}, clear,
                                                 lambda out: out.backward(go.to(out.dtype)), a.reps, a.warmup)
            outs = {s: last[s][0].detach().float() for s in sides}
            r = {"max_abs_diff_out": float((outs["pooled"] - outs["composite"]).abs().max())}
            for s in sides:
                r[s] = timing.fwd_bwd_summary(times, s)
            r["ratio_fwd"] = round(r["composite"]["fwd_ms"] / r["pooled"]["fwd_ms"], 2)
            r["ratio_fwd_bwd"] = round(r["composite"]["fwd_bwd_ms"] / r["pooled"]["fwd_bwd_ms"], 2)
            row[mode] = r
        result["shapes"].append(row)
        xyz, off_host = n_xyz, n_host
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
