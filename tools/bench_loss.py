"""The loss tail of a training step - cross-entropy with an ignore label, L1 on the shift head, their weighted sum, backward - as torch runs it
(the composite) beside pointops.segmentation_loss (csrc/seg_loss.hip), on the same GPU and inputs, the sides alternating.  Prints ONE JSON
line (GPU box only; a missing GPU is an error).

    python tools/bench_loss.py [--reps 20] [--warmup 5] [--inner 50] [--out FILE] [--trace-loop N]

Shapes: (N, C) = (100 000, 19), (100 000, 13), (25 000, 19), each in fp32 and under autocast(f16) (logits and shift_pred in half, as the heads
yield them), 10 % of the rows carrying the ignore label.  Two pairs of sides per shape, every side one forward + backward:
  "loss":  composite = F.cross_entropy(ignore_index) + F.l1_loss + weighted sum + backward;  fused = segmentation_loss + total.backward()
  "step":  the same plus what a training loop adds: composite = the argmax, intersectionAndUnionGPU's overwrite and three histc
           (util/common_util.py:60-73) and the two `.item()` read-backs; fused = one `.losses.tolist()` (its counts come with the forward)

Every shape and precision is set up first and each of its four sides run `inner` times untimed, so that no timed window pays for a first
call of anything; then every figure: median over `reps` windows of `inner` iterations between two device events (the second
synchronised), in ms per iteration; `spread` = max - min of a side over its windows.  `bytes` = what the fused forward and backward must move, from the shapes (fused_bytes
below); `achieved_bytes_per_s` = those bytes over the fused time - launch gaps, allocations and autograd included, so it is a call's
rate, not a kernel's.  `faster_beyond_spread`: composite - fused > the composite's spread.
"""
import argparse

import torch
import torch.nn.functional as F

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import pointops as P  # noqa: E402

IGNORE, WEIGHT = 255, 0.5
SHAPES = ((100000, 19), (100000, 13), (25000, 19))


def fused_bytes(n, c, half):
    """forward: logits, target, shift_pred, shift read, stat written; backward: logits, target, stat, shift_pred, shift read, both gradients written"""
    b = 2 if half else 4
    fwd = n * (b * c + 8 + 3 * b + 12 + 8)
    bwd = n * (b * c + 8 + 8 + 3 * b + 12 + b * c + 3 * b)
    return fwd, bwd


def iou_counts_torch(logits, target, classes):
    """what the fork's training loop runs per step for its IoU meters (util/common_util.py:60-73 on `output.max(1)[1]`): an argmax, an
    indexed overwrite of the ignored rows and three histc over [0, classes - 1] -> (intersection, union, target)"""
    pred = logits.detach().max(1)[1]
    pred[target == IGNORE] = IGNORE
    hist = lambda v: torch.histc(v.float(), bins=classes, min=0, max=classes - 1)
    inter, out, tgt = hist(pred[pred == target]), hist(pred), hist(target)
    return inter, out + tgt - inter, tgt


def case(n, c, amp, a):
    g = torch.Generator(device="cuda").manual_seed(n + c)
    half = torch.float16 if amp else torch.float32
    logits = (3.0 * torch.randn(n, c, device="cuda", generator=g)).to(half).requires_grad_(True)
    shift_pred = torch.randn(n, 3, device="cuda", generator=g).to(half).requires_grad_(True)
    shift = torch.randn(n, 3, device="cuda", generator=g)
    target = torch.randint(0, c, (n,), device="cuda", generator=g)
    target[torch.rand(n, device="cuda", generator=g) < 0.1] = IGNORE

    def composite(step):
        logits.grad = shift_pred.grad = None
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            ce = F.cross_entropy(logits, target, ignore_index=IGNORE)
            l1 = F.l1_loss(shift_pred, shift)
            total = ce + WEIGHT * l1
        total.backward()
        if step:
            counts = iou_counts_torch(logits, target, c)
            return ce.item(), l1.item(), counts
        return total

    def fused(step):
        logits.grad = shift_pred.grad = None
        res = P.segmentation_loss(logits, target, shift_pred, shift, ignore_index=IGNORE, offset_weight=WEIGHT)
        res.total.backward()
        if step:
            return res.losses.tolist(), res.counts
        return res.total

    ce_c, l1_c, counts_c = composite(True)
    gl_c, gs_c = logits.grad.clone(), shift_pred.grad.clone()
    (ce_f, l1_f, _), counts_f = fused(True)
    row = {"n": n, "c": c, "ce": [ce_c, ce_f], "l1": [l1_c, l1_f],
           "max_abs_diff_grad_logits": float((gl_c.float() - logits.grad.float()).abs().max()),
           "max_abs_diff_grad_shift_pred": float((gs_c.float() - shift_pred.grad.float()).abs().max()),
           "counts_equal": bool(all(torch.equal(x.long(), y) for x, y in zip(counts_c, counts_f)))}
    sides = {key: {"composite": (lambda step=step: composite(step)), "fused": (lambda step=step: fused(step))} for key, step in (("loss", False), ("step", True))}
    for pair in sides.values():
        for fn in pair.values():
            for _ in range(a.inner):
                fn()
    torch.cuda.synchronize()
    return row, sides


def timed_row(row, sides, amp, a):
    fwd_b, bwd_b = fused_bytes(row["n"], row["c"], amp)
    for key, pair in sides.items():
        row[key] = timing.summary(timing.windows(pair, a.reps, a.warmup, a.inner), "composite", "fused")
        row[key]["bytes"] = fwd_b + bwd_b
        row[key]["achieved_bytes_per_s"] = round(row[key]["bytes"] / (row[key]["fused_ms"] * 1e-3), 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--trace-loop", type=int, default=0, help="only loop the fused side this many times per shape and dtype (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("bench_loss: at least five repeats a side")
    timing.need_gpu("bench_loss")
    if a.trace_loop:
        # for a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_loss.py --trace-loop 200`: the fused side only
        for n, c in SHAPES:
            for half in (torch.float32, torch.float16):
                logits = torch.randn(n, c, device="cuda").to(half).requires_grad_(True)
                shift_pred, shift = torch.randn(n, 3, device="cuda").to(half).requires_grad_(True), torch.randn(n, 3, device="cuda")
                target = torch.randint(0, c, (n,), device="cuda")
                for _ in range(a.trace_loop):
                    P.segmentation_loss(logits, target, shift_pred, shift, ignore_index=IGNORE, offset_weight=WEIGHT).total.backward()
                torch.cuda.synchronize()
        return
    result = {"tool": "bench_loss", "device": torch.cuda.get_device_name(0), "ignored_rows": 0.1, "offset_weight": WEIGHT, "reps": a.reps, "warmup": a.warmup,
              "inner": a.inner, "cases": {}}
    modes = (("fp32", False), ("autocast_f16", True))
    built = {mode: [case(n, c, amp, a) for n, c in SHAPES] for mode, amp in modes}   # all set up and run once before any timing
    for mode, amp in modes:
        result["cases"][mode] = [timed_row(row, sides, amp, a) for row, sides in built[mode]]
    result["all_faster_beyond_spread"] = bool(all(r[k]["faster_beyond_spread"] for rows in result["cases"].values() for r in rows for k in ("loss", "step")))
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
