"""The glue of a pre-norm transformer block - DropPath, residual add, LayerNorm and the cast in front of the next Linear - as torch runs it
(the composite) beside pointops.residual_norm (csrc/rownorm.hip), on the same GPU and inputs, the two sides alternating.  Prints ONE JSON
line (GPU box only; a missing GPU is an error).

    python tools/bench_block.py [--points 100000] [--reps 20] [--warmup 5] [--inner 10] [--out FILE] [--half-stream]

(a) "operator": one residual site at the four S3DIS stage shapes (N = points, points / 4 + 1, ...; C = 48, 96, 192, 384), fp32 and
    autocast(f16) (y and o in half), training mode, drop_prob 0.3.  Composite: compat.DropPath(0.3)(y), x + ., nn.LayerNorm, and under
    autocast the `.half()` the next Linear would apply.  Fused: layers.drop_path_row_scale + pointops.residual_norm.  Forward, and
    forward + backward (gradients arrive at both z and o; x, y, weight, bias receive theirs).
(b) "blocks": four stand-in BasicLayers of depth 2 (standin.SwinTransformerBlock with DropPath(0.3), the installed BasicLayer /
    WindowAttention / TransitionDown: the real attention) strung as the model strings them on the room scene, forward + backward, with
    layers.patch_block_classes applied or not.  Under autocast only stage 0 is fused: TransitionDown's Linear hands the later stages
    half features, and a half residual stream takes the original forward.

--half-stream measures the half residual stream instead (layers.HALF_STREAM, pointops.residual_norm_stream), by the same method:
(c) "site": one residual site forward + backward at the four stage shapes with x, y, o and the incoming gradients in half, under
    autocast(f16) and autocast(bf16).  Composite: x + compat.DropPath(0.3)(y) in half, F.layer_norm (autocast runs it in fp32), the cast.
(d) "blocks": the four stand-in layers of (b) under autocast(f16) three ways in one run, alternating: unpatched, patched with
    HALF_STREAM off (only stage 0 fused) and patched with it on (every stage fused).

Every figure: median over `reps` windows of `inner` iterations between two device events (the second synchronised), in ms per
iteration; `spread` = max - min of the composite / unpatched side over its windows.  `bytes` = what the fused forward and backward must
move, from the shapes (fused_bytes below); `achieved_bytes_per_s` = those bytes over the fused time - launch gaps and DropPath's rand
included, so it is a call's rate, not a kernel's.  `faster_beyond_spread`: composite - fused > the composite's spread.
"""
import argparse
import statistics

import torch

import timing  # first: it puts the repository root on sys.path
import standin_layers  # noqa: E402
from stratified_transformer_amd import compat, layers, pipeline, pointops as P, scene, standin  # noqa: E402

DROP = 0.3


def fused_bytes(n, c, half):
    """bytes one site must move: forward reads x, y, s and writes z, o, stat; backward reads dO, dZ, z, stat, s and writes dx, dy
    (gamma, beta and the parameter-gradient partials: at most 1024 * 2 * c floats, left out)"""
    b = 2 if half else 4
    fwd = n * (4 * c + b * c + 4 + 4 * c + b * c + 8)
    bwd = n * (b * c + 4 * c + 4 * c + 8 + 4 + 4 * c + b * c)
    return fwd, bwd


def operator_case(n, c, amp, a):
    g = torch.Generator(device="cuda").manual_seed(c)
    half = torch.float16 if amp else torch.float32
    x = torch.randn(n, c, device="cuda", generator=g).requires_grad_(True)
    y = torch.randn(n, c, device="cuda", generator=g).to(half).requires_grad_(True)
    gz, go = torch.randn(n, c, device="cuda", generator=g), torch.randn(n, c, device="cuda", generator=g).to(half)
    norm, dp = torch.nn.LayerNorm(c).cuda(), compat.DropPath(DROP).train()

    def composite():
        z = x + dp(y)
        o = norm(z)
        return z, (o.half() if amp else o)

    def fused():
        return P.residual_norm(x, y, layers.drop_path_row_scale(dp, y), norm.weight, norm.bias, norm.eps, half)

    def with_backward(fn):
        def run():
            x.grad = y.grad = None
            norm.zero_grad(set_to_none=True)
            z, o = fn()
            torch.autograd.backward([z, o], [gz, go])
        return run

    torch.manual_seed(1)
    zc, oc = composite()
    torch.manual_seed(1)
    zf, of = fused()
    row = {"n": n, "c": c, "max_abs_diff_z": float((zc - zf).abs().max()), "max_abs_diff_o": float((oc.float() - of.float()).abs().max())}
    fwd_b, bwd_b = fused_bytes(n, c, amp)
    with torch.no_grad():
        row["fwd"] = timing.summary(timing.windows({"composite": composite, "fused": fused}, a.reps, a.warmup, a.inner), "composite", "fused")
    row["fwd_bwd"] = timing.summary(timing.windows({"composite": with_backward(composite), "fused": with_backward(fused)}, a.reps, a.warmup, a.inner), "composite", "fused")
    row["fwd"]["bytes"], row["fwd_bwd"]["bytes"] = fwd_b, fwd_b + bwd_b
    for k in ("fwd", "fwd_bwd"):
        row[k]["achieved_bytes_per_s"] = round(row[k]["bytes"] / (row[k]["fused_ms"] * 1e-3), 1)
    return row


def stream_bytes(n, c):
    """fused_bytes with the stream operands x, z, dZ, dx in half as well"""
    return n * (2 * c + 2 * c + 4 + 2 * c + 2 * c + 8), n * (2 * c + 2 * c + 2 * c + 8 + 4 + 2 * c + 2 * c)


def half_stream_site(n, c, dt, a):
    """one residual site on a half stream, forward + backward under autocast(dt): composite beside pointops.residual_norm_stream"""
    g = torch.Generator(device="cuda").manual_seed(c)
    x = torch.randn(n, c, device="cuda", generator=g).to(dt).requires_grad_(True)
    y = torch.randn(n, c, device="cuda", generator=g).to(dt).requires_grad_(True)
    gz, go = torch.randn(n, c, device="cuda", generator=g).to(dt), torch.randn(n, c, device="cuda", generator=g).to(dt)
    norm, dp = torch.nn.LayerNorm(c).cuda(), compat.DropPath(DROP).train()

    def composite():
        z = x + dp(y)
        return z, torch.nn.functional.layer_norm(z, (c,), norm.weight, norm.bias, norm.eps).to(dt)

    def fused():
        return P.residual_norm_stream(x, y, layers.drop_path_row_scale(dp, y), norm.weight, norm.bias, norm.eps, dt)

    def with_backward(fn):
        def run():
            x.grad = y.grad = None
            norm.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=dt):
                z, o = fn()
            torch.autograd.backward([z, o], [gz, go])
        return run

    with torch.autocast("cuda", dtype=dt):
        torch.manual_seed(1)
        zc, oc = composite()
        torch.manual_seed(1)
        zf, of = fused()
    assert zc.dtype == zf.dtype == oc.dtype == of.dtype == dt
    row = {"n": n, "c": c, "max_abs_diff_z": float((zc.float() - zf.float()).abs().max()), "max_abs_diff_o": float((oc.float() - of.float()).abs().max())}
    row["fwd_bwd"] = timing.summary(timing.windows({"composite": with_backward(composite), "fused": with_backward(fused)}, a.reps, a.warmup, a.inner), "composite", "fused")
    row["fwd_bwd"]["bytes"] = sum(stream_bytes(n, c))
    row["fwd_bwd"]["achieved_bytes_per_s"] = round(row["fwd_bwd"]["bytes"] / (row["fwd_bwd"]["fused_ms"] * 1e-3), 1)
    return row


def half_stream_blocks(a):
    """the four stand-in layers under autocast(f16): unpatched, patched with HALF_STREAM off (stage 0 fused), patched with it on"""
    step, sites = _stand_in_step(a, True)
    calls = {"off": 0, "on": 0}

    def unpatched():
        if (standin.SwinTransformerBlock, "forward") in layers._ORIGINAL:
            standin.SwinTransformerBlock.forward = layers._ORIGINAL.pop((standin.SwinTransformerBlock, "forward"))
        step()

    def patched(on):
        real = P.residual_norm_stream

        def counted(*args, **kw):
            calls["on" if on else "off"] += 1
            return real(*args, **kw)

        def run():
            layers.HALF_STREAM = on
            layers.patch_block_classes(standin.SwinTransformerBlock)
            P.residual_norm_stream = counted
            try:
                step()
            finally:
                P.residual_norm_stream = real
                layers.HALF_STREAM = False
        return run

    try:
        layers.patch_classes(standin.BasicLayer, standin.WindowAttention, standin.TransitionDown)
        times = timing.windows({"unpatched": unpatched, "patched_half_stream_off": patched(False), "patched_half_stream_on": patched(True)}, a.reps, a.warmup, 1)
    finally:
        layers.HALF_STREAM = False
        layers.uninstall_fast_layers()
    r = {k + "_ms": round(statistics.median(v), 5) for k, v in times.items()}
    r.update({k + "_spread_ms": round(max(v) - min(v), 5) for k, v in times.items()})
    for k in ("unpatched", "patched_half_stream_off"):
        r["on_faster_than_" + k + "_beyond_spread"] = bool(r[k + "_ms"] - r["patched_half_stream_on_ms"] > r[k + "_spread_ms"])
    steps = a.reps + a.warmup
    r["stream_calls_per_step"] = {k: v / steps for k, v in calls.items()}     # off: 0; on: 3 stages x (1 + 2 + 1) sites
    r["stage_rows"] = [n for n, _ in sites]
    return r


def _stand_in_step(a, amp):
    """-> step(), [(rows, channels) per stage]: one forward + backward of four stand-in BasicLayers strung as the model strings them"""
    return standin_layers.stand_in_step(a.points, amp, DROP)[:2]


def blocks_leg(a, amp):
    step, sites = _stand_in_step(a, amp)

    def patched():
        layers.patch_block_classes(standin.SwinTransformerBlock)
        step()

    def unpatched():
        if (standin.SwinTransformerBlock, "forward") in layers._ORIGINAL:
            standin.SwinTransformerBlock.forward = layers._ORIGINAL.pop((standin.SwinTransformerBlock, "forward"))
        step()

    try:
        layers.patch_classes(standin.BasicLayer, standin.WindowAttention, standin.TransitionDown)
        r = timing.summary(timing.windows({"unpatched": unpatched, "patched": patched}, a.reps, a.warmup, 1), "unpatched", "patched")
    finally:
        layers.uninstall_fast_layers()
    # Under autocast TransitionDown's Linear hands the later stages HALF features: their residual stream is half, which the fused
    # forward leaves to the original one - only stage 0 is fused then.
    fused_sites = sites[:1] if amp else sites
    # per block two sites (attention branch, MLP branch) and, for the first block of a layer, its norm1 alone (x read, o written; twice: backward)
    r["bytes"] = sum(2 * 2 * sum(fused_bytes(n, c, amp)) + n * c * (4 + (2 if amp else 4)) * 2 for n, c in fused_sites)
    r["achieved_bytes_per_s_whole_step"] = round(r["bytes"] / (r["patched_ms"] * 1e-3), 1)
    r["stage_rows"], r["fused_stages"] = [n for n, _ in sites], len(fused_sites)
    return r


_stage_rows = standin_layers.stage_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--skip-blocks", action="store_true")
    ap.add_argument("--trace-loop", type=int, default=0, help="only loop the fused site this many times per stage shape (for a kernel trace)")
    ap.add_argument("--half-stream", action="store_true", help="measure the half residual stream (layers.HALF_STREAM) instead: (c) and (d) above")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("bench_block: at least five repeats a side")
    timing.need_gpu("bench_block")
    if a.trace_loop:
        # for a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_block.py --trace-loop 160`: the fused site only
        for n, c in zip(_stage_rows(a.points, pipeline.s3dis_config()), (48, 96, 192, 384)):
            x, y = (torch.randn(n, c, device="cuda", requires_grad=True) for _ in range(2))
            gz, go = torch.randn(n, c, device="cuda"), torch.randn(n, c, device="cuda")
            norm, dp = torch.nn.LayerNorm(c).cuda(), compat.DropPath(DROP).train()
            for _ in range(a.trace_loop):
                z, o = P.residual_norm(x, y, layers.drop_path_row_scale(dp, y), norm.weight, norm.bias, norm.eps)
                torch.autograd.backward([z, o], [gz, go])
            torch.cuda.synchronize()
        return
    if a.half_stream:
        result = {"tool": "bench_block --half-stream", "device": torch.cuda.get_device_name(0), "points": a.points, "drop_prob": DROP, "reps": a.reps,
                  "warmup": a.warmup, "inner": a.inner, "site": {}, "blocks": {}}
        rows = _stage_rows(a.points, pipeline.s3dis_config())
        for mode, dt in (("autocast_f16", torch.float16), ("autocast_bf16", torch.bfloat16)):
            result["site"][mode] = [half_stream_site(n, c, dt, a) for n, c in zip(rows, (48, 96, 192, 384))]
        if not a.skip_blocks:
            result["blocks"]["autocast_f16"] = half_stream_blocks(a)
        result["not_measured"] = ["a counter profile", "bf16 timings beyond one site", "the unmodified model end to end"]
        return timing.emit(result, a.out)
    result = {"tool": "bench_block", "device": torch.cuda.get_device_name(0), "points": a.points, "drop_prob": DROP, "reps": a.reps, "warmup": a.warmup,
              "inner": a.inner, "operator": {}, "blocks": {}}
    rows = _stage_rows(a.points, pipeline.s3dis_config())
    for mode, amp in (("fp32", False), ("autocast_f16", True)):
        result["operator"][mode] = [operator_case(n, c, amp, a) for n, c in zip(rows, (48, 96, 192, 384))]
        if not a.skip_blocks:
            result["blocks"][mode] = blocks_leg(a, amp)
    stage0 = [result["operator"][m][0]["fwd_bwd"]["faster_beyond_spread"] for m in ("fp32", "autocast_f16")]
    result["stage0_fwd_bwd_faster_beyond_spread"] = bool(all(stage0))
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
