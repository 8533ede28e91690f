"""optim.SGD and the in-call clip by the global gradient norm (stratified_transformer_amd.optim on csrc/optim.hip) against torch's own
SGD, GradScaler and clip_grad_norm_, on the S3DIS parameter set of tools/bench_optim.py (228 tensors, 8.0 M elements, two groups).
Prints ONE JSON line (GPU box only; a missing GPU is an error).  There is no threshold.

    python tools/bench_sgd_clip.py [--windows 15] [--steps 20] [--warmup 3] [--out profiles/optim_sgd_clip_bench.json]
    python tools/bench_sgd_clip.py --parent-json A1.json A2.json --branch-json B1.json B2.json --merge profiles/optim_sgd_clip_bench.json
        # adds the unclipped AdamW rows of tools/bench_optim.py runs (the parent commit's and this one's, alternating in one session); no GPU
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_sgd_clip.py --trace-steps 50 --trace-leg sgd_clipped+scaler
    python tools/bench_sgd_clip.py --kernel-trace DIR/.../*_kernel_trace.csv --trace-leg sgd_clipped+scaler --merge profiles/optim_sgd_clip_bench.json

Legs (one step each; gradients are seeded, finite and stay in place; the scale is 1 and never grows, as in tools/bench_optim.py):
    sgd+scaler / sgd          scaler.step(opt); scaler.update()  /  opt.step()          momentum 0.9, weight_decay 1e-4
    sgd_clipped+scaler        ours: opt.max_grad_norm = 1.0, the same two lines;  torch: scaler.unscale_(opt);
    adamw_clipped+scaler      clip_grad_norm_(params, 1.0); scaler.step(opt); scaler.update() on torch's fused optimizer
torch's clip_grad_norm_ rescales the gradients in place, so over the windows its gradients shrink until their norm is 1 and the factor
clamps to 1 - the passes and launches stay the same; ours never writes a gradient, its norm stays near 2833 and every step clips.
A window is `steps` steps between two host clock readings, the second after torch.cuda.synchronize(); the variants alternate window by
window within the one run; per variant the median over `windows` windows (after `warmup` unrecorded ones) and [min, lower quartile,
upper quartile, max], in ms per step.
"""
import argparse
import json
import statistics
import sys

import torch

import timing  # first: it puts the repository root on sys.path
import bench_optim as B  # noqa: E402  (workload only: the parameter set, Variant, the traced kernels and their byte bounds)

MAX_NORM = 1.0
SGD_BYTES_PER_ELEMENT = 20   # reads p, g, buf; writes p, buf
NOT_MEASURED = ["a whole training step of the unmodified model with and without the fused step", "hardware counters (no --pmc run was taken)",
                "parameter sets of other configurations", "SGD without a momentum, Nesterov", "gradients that are not already in the last-level cache"]


class Variant(B.Variant):
    def __init__(self, name, shapes, make_opt, make_scaler, clip):
        super().__init__(name, shapes, make_opt, make_scaler)
        self.clip = clip   # None, "ours" (the optimizer's max_grad_norm) or "torch" (unscale_ + clip_grad_norm_)
        if clip == "ours":
            self.opt.max_grad_norm = MAX_NORM

    def step(self):
        if self.clip == "torch":
            self.scaler.unscale_(self.opt)
            torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
            self.scaler.step(self.opt)
            self.scaler.update()
        else:
            super().step()


def makers():
    from stratified_transformer_amd import optim
    sgd, adamw = dict(momentum=0.9, weight_decay=1e-4), dict(weight_decay=0.01)
    ours_scaler = lambda: optim.GradScaler("cuda", init_scale=1.0, growth_interval=10 ** 9)          # noqa: E731
    torch_scaler = lambda: torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=10 ** 9)     # noqa: E731
    out = {}
    for with_scaler in (True, False):
        tail = "+scaler" if with_scaler else ""
        out["sgd" + tail] = {
            "ours": (lambda g: optim.SGD(g, **sgd), ours_scaler if with_scaler else None, None),
            "torch_default": (lambda g: torch.optim.SGD(g, **sgd), torch_scaler if with_scaler else None, None),
            "torch_single": (lambda g: torch.optim.SGD(g, foreach=False, **sgd), torch_scaler if with_scaler else None, None),
            "torch_fused": (lambda g: torch.optim.SGD(g, fused=True, **sgd), torch_scaler if with_scaler else None, None),
        }
    out["sgd_clipped+scaler"] = {
        "ours": (lambda g: optim.SGD(g, **sgd), ours_scaler, "ours"),
        "torch_fused": (lambda g: torch.optim.SGD(g, fused=True, **sgd), torch_scaler, "torch"),
    }
    out["adamw_clipped+scaler"] = {
        "ours": (lambda g: optim.AdamW(g, **adamw), ours_scaler, "ours"),
        "torch_fused": (lambda g: torch.optim.AdamW(g, fused=True, **adamw), torch_scaler, "torch"),
    }
    out["adamw+scaler"] = {"ours": (lambda g: optim.AdamW(g, **adamw), ours_scaler, None)}           # the unclipped step next to the clipped one
    return out


def variants(shapes, only=None):
    out, missing = [], {}
    for leg, sides in makers().items():
        for side, (make_opt, make_scaler, clip) in sides.items():
            name = f"{leg}/{side}"
            if only is not None and name not in only:
                continue
            try:
                out.append(Variant(name, shapes, make_opt, make_scaler, clip))
            except (RuntimeError, ValueError, TypeError) as e:   # a torch without fused SGD says so at construction
                if side == "ours":
                    raise
                missing[name] = f"{type(e).__name__}: {e}"
    return out, missing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0, help="run only this many steps of --trace-leg's own side (for a run under rocprofv3)")
    ap.add_argument("--trace-leg", default="sgd_clipped+scaler")
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 kernel_trace.csv of a --trace-steps run to summarise")
    ap.add_argument("--parent-json", nargs="+", default=None, help="tools/bench_optim.py's results on the parent commit")
    ap.add_argument("--branch-json", nargs="+", default=None, help="tools/bench_optim.py's results on this commit, same session, alternating")
    ap.add_argument("--merge", default=None, help="the bench JSON to add a summary to")
    args = ap.parse_args()
    shapes = B.s3dis_shapes()
    elements = sum(B.numel(s) for _, s in shapes)
    counts = dict(tensors=len(shapes), elements=elements, chunks=sum(-(-B.numel(s) // 4096) for _, s in shapes))
    if args.parent_json:
        rows = {}
        for side, paths in (("parent", args.parent_json), ("branch", args.branch_json)):
            runs = [json.load(open(path))["variants"] for path in paths]
            rows[side] = {k: [v[k] for v in runs] for k in ("fused+scaler", "fused")}   # one entry per run, in the order they were taken
        timing.merge(args.merge, "adamw_without_clipping", rows)
        return
    if args.kernel_trace:
        summary = B.trace_summary(args.kernel_trace, elements)
        B.byte_share(summary, "optim_sgd_kernel", SGD_BYTES_PER_ELEMENT * elements)
        timing.merge(args.merge, "kernel_trace:" + args.trace_leg, summary)
        return
    timing.need_gpu("bench_sgd_clip")
    print("parameter set:", counts, file=sys.stderr)
    if args.trace_steps:
        v = variants(shapes, only=[args.trace_leg + "/ours"])[0][0]
        for _ in range(args.trace_steps):
            v.step()
        torch.cuda.synchronize()
        print(json.dumps(dict(traced_steps=args.trace_steps, leg=args.trace_leg, **counts)))
        return
    vs, missing = variants(shapes)
    times = timing.wall_windows({v.name: v.step for v in vs}, args.windows, args.warmup, args.steps)
    norms = {v.name: float(v.opt.last_grad_norm) for v in vs if getattr(v.opt, "last_grad_norm", None) is not None}
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, parameter_set=counts, steps_per_window=args.steps,
                  windows=args.windows, warmup_windows=args.warmup, max_norm=MAX_NORM,
                  unit="ms per step, host clock around a window that ends in a synchronise",
                  byte_bound_us=dict(sgd_update=round(SGD_BYTES_PER_ELEMENT * elements / B.HBM_BYTES_PER_S * 1e6, 1),
                                     check_and_norm=round(4 * elements / B.HBM_BYTES_PER_S * 1e6, 1)),
                  variants={k: dict(median_ms=round(statistics.median(v), 4), spread=timing.spread(v)) for k, v in times.items()},
                  last_grad_norm=norms, not_available=missing, not_measured=NOT_MEASURED)
    timing.emit(result, args.out)


if __name__ == "__main__":
    main()
