"""KPConv stem convolution: the HIP path (pointops.kpconv: csrc/kpconv.hip + matrix products) beside the torch formulation of the
same three formulas, on the same GPU, same inputs.  Prints ONE JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_kpconv.py [--points 100000] [--reps 30] [--warmup 5] [--out FILE]

Scene: a surface room at voxel 0.04, neighbours from pointops.ball_query(0.1, 34, ...) - the stem's search.  Shapes: (3 -> 48), the
model's first block, whose input is data (no gradient of x: the backward kernel is not launched), and (12 -> 12), the residual
block's convolution (gradients of x and weight).  Per shape and side: median over `reps` of the forward and of forward + backward,
each bracketed by events on the stream, the two sides alternating; `ratio_fwd_bwd` = torch / HIP (> 1: the HIP path is faster).
"""
import argparse

import torch

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import pointops as P, scene  # noqa: E402
from stratified_transformer_amd.compat import kpconv_kernel_points  # noqa: E402

EXTENT = 0.04


def kpconv_torch(query, support, nb, x, kp, weight, extent):
    """the composite: w = max(0, 1 - |rel - K| / e) masked, wf = w @ x[j], out = wf @ weight"""
    n_s = support.shape[0]
    nbl = nb.long()
    valid = (nbl >= 0) & (nbl < n_s)
    j = nbl.clamp(0, n_s - 1)
    rel = support[j] - query[:, None, :]
    dist = (rel[:, None, :, :] - kp[None, :, None, :]).pow(2).sum(-1).sqrt()
    w = (1.0 - dist / extent).clamp(min=0.0) * valid[:, None, :]
    wf = w @ x[j]
    return wf.reshape(wf.shape[0], -1) @ weight.reshape(-1, weight.shape[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timing.need_gpu("bench_kpconv")
    n = a.points
    xyz = torch.from_numpy(scene.make_room(n, 0)).cuda()
    off = torch.tensor([n], dtype=torch.int32, device="cuda")
    nb, _ = P.ball_query(2.5 * EXTENT, 34, xyz, xyz, off, off)
    nb = nb.contiguous()
    kp = kpconv_kernel_points(EXTENT).cuda()
    result = {"tool": "bench_kpconv", "device": torch.cuda.get_device_name(0), "points": n, "n_nb": 34, "n_kp": 15,
              "mean_valid_neighbours": round(float((nb >= 0).sum(1).float().mean()), 2), "reps": a.reps, "warmup": a.warmup, "shapes": []}
    for c, out_c, x_grad in ((3, 48, False), (12, 12, True)):
        g = torch.Generator(device="cuda").manual_seed(c)
        x = torch.randn(n, c, device="cuda", generator=g).requires_grad_(x_grad)
        weight = (torch.randn(15, c, out_c, device="cuda", generator=g) * 0.2).requires_grad_(True)
        go = torch.randn(n, out_c, device="cuda", generator=g)
        sides = {"hip": lambda: P.kpconv(xyz, xyz, nb, x, kp, weight, EXTENT), "torch": lambda: kpconv_torch(xyz, xyz, nb, x, kp, weight, EXTENT)}

        def clear():
            x.grad = weight.grad = None

        def backward(out):
            out.backward(go)
            return weight.grad

        times, last = timing.fwd_bwd_windows(sides, clear, backward, a.reps, a.warmup)
        outs, grads = {s: last[s][0].detach() for s in sides}, {s: last[s][1].detach() for s in sides}
        row = {"c": c, "out": out_c, "x_requires_grad": x_grad,
               "max_abs_diff_out": float((outs["hip"] - outs["torch"]).abs().max()),
               "max_rel_diff_grad_weight": float(((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max()))}
        for s in sides:
            row[s] = timing.fwd_bwd_summary(times, s)
        row["ratio_fwd"] = round(row["torch"]["fwd_ms"] / row["hip"]["fwd_ms"], 2)
        row["ratio_fwd_bwd"] = round(row["torch"]["fwd_bwd_ms"] / row["hip"]["fwd_bwd_ms"], 2)
        result["shapes"].append(row)
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
