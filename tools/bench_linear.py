"""The parameter gradients of the model's Linear layers as torch computes them beside pointops.linear_param_grads (csrc/linear_grads.hip),
on the same GPU and operands, the two sides alternating.  Prints ONE JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_linear.py [--reps 15] [--warmup 5] [--inner 10] [--skip-blocks] [--out profiles/linear_grads_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_linear.py --trace-loop 50
    python tools/bench_linear.py --kernel-stats DIR/NAME_results.db --out profiles/linear_grads_bench.json      (no GPU: merges "kernels")

Shapes: qkv C -> 3C, proj C -> C, fc1 C -> 4C, fc2 4C -> C at (rows, C) = (100 000, 48), (25 001, 96), (6 251, 192), (1 563, 384), and the
heads 100 000 x 48 -> 48 and 48 -> 13; in fp32 and under autocast(f16) (half rows and half incoming gradients, fp32 parameters).

(a) "param_grads": grad_out.t() @ x plus grad_out.sum(0) - what torch's Linear backward runs for the two parameters (under autocast the
    half product is then cast to the fp32 parameter, included) - beside pointops.linear_param_grads(x, grad_out).
(b) "linear": one nn.Linear forward + backward (input and parameters want gradients), unbound beside bound by layers.fuse_linear_grads
    with the rule forced on, so that every shape is measured whatever the rule says.
(c) "blocks": four stand-in BasicLayers of depth 2 with the installed attention on the room scene, forward + backward, exactly the step
    of tools/bench_block.py: unpatched, layers.fuse_linear_grads (the rule as shipped), and fuse_linear_grads together with
    install_fused_blocks' block forward.

Every figure: median over `reps` windows of `inner` iterations between two device events (the second synchronised), ms per iteration;
`*_spread_ms` = max - min over a side's windows; `faster_beyond_spread`: torch - fused > torch's spread.  `bytes` = one read of x and
grad_out; `achieved_bytes_per_s` = those over the fused time, launch gaps and the two allocations included: a call's rate, not a kernel's.
Every GPU step runs under timing.limited.
"""
import argparse
import statistics

import torch

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import layers, pointops as P, standin  # noqa: E402
import standin_layers  # noqa: E402  (the stand-in step of bench_block: a workload builder)

STAGES = ((100000, 48), (25001, 96), (6251, 192), (1563, 384))
TRACE_SHAPE = (100000, 48, 192)
DROP = 0.3  # bench_block's


def shapes():
    out = []
    for n, c in STAGES:
        out += [("qkv", n, c, 3 * c), ("proj", n, c, c), ("fc1", n, c, 4 * c), ("fc2", n, 4 * c, c)]
    return out + [("head", 100000, 48, 48), ("classes", 100000, 48, 13)]


def param_grads_case(name, n, n_in, n_out, half, a):
    gen = torch.Generator(device="cuda").manual_seed(n_in * 7 + n_out)
    dt = torch.float16 if half else torch.float32
    x, g = torch.randn(n, n_in, device="cuda", generator=gen).to(dt), torch.randn(n, n_out, device="cuda", generator=gen).to(dt)

    def composite():
        dW, db = g.t() @ x, g.sum(0)
        return (dW.float(), db.float()) if half else (dW, db)

    def fused():
        return P.linear_param_grads(x, g)

    (cw, cb), (fw, fb) = composite(), fused()
    scale = float(fw.abs().max())
    row = {"layer": name, "n": n, "in": n_in, "out": n_out, "max_abs_diff_w_over_scale": float((cw - fw).abs().max()) / scale,
           "max_abs_diff_b": float((cb - fb).abs().max())}
    row.update(timing.summary(timing.windows({"torch": composite, "fused": fused}, a.reps, a.warmup, a.inner), "torch", "fused"))
    row["bytes"] = n * (n_in + n_out) * (2 if half else 4)
    row["achieved_bytes_per_s"] = round(row["bytes"] / (row["fused_ms"] * 1e-3), 1)
    return row


def linear_case(name, n, n_in, n_out, half, a):
    torch.manual_seed(n_in)
    lin_a, lin_b = torch.nn.Linear(n_in, n_out).cuda(), torch.nn.Linear(n_in, n_out).cuda()
    lin_b.load_state_dict(lin_a.state_dict())
    layers.fuse_linear_grads(lin_b)
    gen = torch.Generator(device="cuda").manual_seed(n_out)
    x = torch.randn(n, n_in, device="cuda", generator=gen).requires_grad_(True)
    go = torch.randn(n, n_out, device="cuda", generator=gen).to(torch.float16 if half else torch.float32)

    def run(lin):
        def step():
            x.grad = None
            lin.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=half):
                out = lin(x)
            out.backward(go)
        return step

    rule, layers.linear_grads_worth_it = layers.linear_grads_worth_it, lambda *args: True
    try:
        run(lin_a)(), run(lin_b)()
        scale = float(lin_a.weight.grad.abs().max())
        row = {"layer": name, "n": n, "in": n_in, "out": n_out,
               "max_abs_diff_w_over_scale": float((lin_a.weight.grad - lin_b.weight.grad).abs().max()) / scale}
        row.update(timing.summary(timing.windows({"unbound": run(lin_a), "bound": run(lin_b)}, a.reps, a.warmup, a.inner), "unbound", "bound"))
    finally:
        layers.linear_grads_worth_it = rule
    row["rule_admits"] = bool(rule(n, n_in, n_out, torch.float16 if half else torch.float32))
    return row


def blocks_leg(a, half):
    """the stand-in step of bench_block three ways in one run, alternating"""
    taken = {"n": 0}
    real = P.linear_rows

    def counted(*args_, **kw):
        taken["n"] += 1
        return real(*args_, **kw)

    step, sites, net = standin_layers.stand_in_step(a.points, half, DROP)  # one net, bound and unbound around the windows

    def unblock():
        if (standin.SwinTransformerBlock, "forward") in layers._ORIGINAL:
            standin.SwinTransformerBlock.forward = layers._ORIGINAL.pop((standin.SwinTransformerBlock, "forward"))

    def unpatched():
        unblock()
        layers.unfuse_linear_grads(net)
        step()

    def fused():
        unblock()
        layers.fuse_linear_grads(net)
        P.linear_rows = counted
        try:
            step()
        finally:
            P.linear_rows = real

    def fused_blocks():
        layers.patch_block_classes(standin.SwinTransformerBlock)
        layers.fuse_linear_grads(net)
        step()

    try:
        layers.patch_classes(standin.BasicLayer, standin.WindowAttention, standin.TransitionDown)
        times = timing.windows({"unpatched": unpatched, "fuse_linear_grads": fused, "fuse_linear_grads_and_blocks": fused_blocks}, a.reps, a.warmup, 1)
    finally:
        layers.unfuse_linear_grads(net)
        layers.uninstall_fast_layers()
    r = {k + "_ms": round(statistics.median(v), 5) for k, v in times.items()}
    r.update({k + "_spread_ms": round(max(v) - min(v), 5) for k, v in times.items()})
    for k in ("fuse_linear_grads", "fuse_linear_grads_and_blocks"):
        r[k + "_faster_beyond_spread"] = bool(r["unpatched_ms"] - r[k + "_ms"] > r["unpatched_spread_ms"])
    r["linear_rows_calls_per_step"] = taken["n"] / (a.reps + a.warmup)
    r["linears_bound"] = len(layers.fuse_linear_grads(net))
    layers.unfuse_linear_grads(net)
    r["stage_rows"] = [n for n, _ in sites]
    return r


def trace_loop(loop):
    """for a run of its own under `rocprofv3 --kernel-trace --stats`: the fused operator alone at TRACE_SHAPE, fp32 then half rows"""
    n, n_in, n_out = TRACE_SHAPE
    for dt in (torch.float32, torch.float16):
        x, g = torch.randn(n, n_in, device="cuda").to(dt), torch.randn(n, n_out, device="cuda").to(dt)
        with timing.limited(120):
            for _ in range(loop):
                P.linear_param_grads(x, g)
            torch.cuda.synchronize()


def kernel_stats(db_path, out_path):
    """the two kernels' times from the database a --trace-loop run left: dispatches in start order, the first half fp32 rows, the second half rows"""
    n, n_in, n_out = TRACE_SHAPE
    times = timing.kernel_times_db(db_path)
    rows = -(-n // P.LINEAR_GRADS_ROWS)
    result = {"shape": {"n": n, "in": n_in, "out": n_out}, "bound_us_from_measured_rates": [16, 20]}
    for kernel, moved in (("linear_grads_partial_kernel", lambda b: n * (n_in + n_out) * b + rows * n_out * (n_in + 1) * 4),
                          ("linear_grads_reduce_kernel", lambda b: rows * n_out * (n_in + 1) * 4 + n_out * (n_in + 1) * 4)):
        us = [t for name, t in times if kernel in name]
        if len(us) < 2:
            raise SystemExit(f"bench_linear: no dispatches of {kernel} in {db_path}")
        for mode, part, b in (("fp32", us[:len(us) // 2], 4), ("f16", us[len(us) // 2:], 2)):
            part = part[len(part) // 5:]  # (behind the first fifth: clocks and caches settled)
            med = statistics.median(part)
            result.setdefault(mode, {})[kernel] = {"calls": len(part), "median_us": round(med, 2), "min_us": round(min(part), 2), "max_us": round(max(part), 2),
                                                  "bytes": moved(b), "achieved_bytes_per_s": round(moved(b) / (med * 1e-6), 1)}
    timing.merge(out_path, "kernels", result)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--skip-blocks", action="store_true")
    ap.add_argument("--trace-loop", type=int, default=0, help="only loop the fused operator this many times (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, metavar="DB", help="no GPU work: merge the kernel times of a --trace-loop run into --out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        if not a.out:
            raise SystemExit("bench_linear: --kernel-stats DB needs --out FILE (the JSON to merge into)")
        return kernel_stats(a.kernel_stats, a.out)
    if a.reps < 5:
        raise SystemExit("bench_linear: at least five repeats a side")
    timing.need_gpu("bench_linear")
    if a.trace_loop:
        return trace_loop(a.trace_loop)
    result = {"tool": "bench_linear", "device": torch.cuda.get_device_name(0), "points": a.points, "reps": a.reps, "warmup": a.warmup, "inner": a.inner,
              "chunk_rows": P.LINEAR_GRADS_ROWS, "param_grads": {}, "linear": {}, "blocks": {}}
    for mode, half in (("fp32", False), ("autocast_f16", True)):
        result["param_grads"][mode], result["linear"][mode] = [], []
        for case in shapes():
            with timing.limited(120):
                result["param_grads"][mode].append(param_grads_case(*case, half, a))
            with timing.limited(120):
                result["linear"][mode].append(linear_case(*case, half, a))
        if not a.skip_blocks:
            with timing.limited(300):
                result["blocks"][mode] = blocks_leg(a, half)
    result["not_measured"] = ["a training step of the unmodified model", "bf16 rows", "hardware counters"]
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
