"""The optimizer step on the device (stratified_transformer_amd.optim on csrc/optim.hip) against torch's own AdamW + GradScaler, on the
parameter set of the S3DIS configuration (config/s3dis/s3dis_stratified_transformer.yaml: channels 48 / 96 / 192 / 384, depths 2 / 2 / 6 / 2,
heads 3 / 6 / 12 / 24, rel-pos tables [64, h, 16, 3], stem_transformer, 13 classes; the tensors whose name contains "blocks" form the second
group, tool/train.py:137-146).  Prints ONE JSON line (GPU box only; a missing GPU is an error).  There is no threshold.

    python tools/bench_optim.py [--windows 15] [--steps 20] [--warmup 3] [--out profiles/optim_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_optim.py --trace-steps 50      # the separate traced run
    python tools/bench_optim.py --kernel-trace DIR/.../*_kernel_trace.csv --merge profiles/optim_bench.json  # its summary, no GPU needed

One step = scaler.step(optimizer); scaler.update() (or optimizer.step() in the rows without a scaler) on seeded finite gradients that stay
in place.  The scale is 1 and never grows, so torch's in-place unscale leaves them as they are and every step of every variant does the
same arithmetic; the kernels do not special-case it (torch's unscale kernel still reads and writes every gradient).
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

CHANNELS, DEPTHS, HEADS, CLASSES, TABLE_ROWS, KERNEL_POINTS, FEA_DIM = [48, 96, 192, 384], [2, 2, 6, 2], [3, 6, 12, 24], 13, 64, 15, 6
HBM_BYTES_PER_S = 6.3e12        # what a float4 copy reaches on the chip
UPDATE_BYTES_PER_ELEMENT = 28   # reads p, g, m, v; writes p, m, v
KERNELS = r"optim_\w+_kernel|amp_update_scale|fillBuffer\w*"   # what a traced step launches
NOT_MEASURED = ["a whole training step of the unmodified model with and without the fused step", "gradient clipping between unscale_ and step",
                "hardware counters (no --pmc run was taken)", "parameter sets of other configurations"]


def s3dis_shapes():
    """[(name, shape)] of the trainable parameters of Stratified(...) under the S3DIS yaml, in module order"""
    out = [("stem_layer.0.kpconv.weight", (KERNEL_POINTS, FEA_DIM, CHANNELS[0])), ("stem_layer.0.bn.weight", (CHANNELS[0],)),
           ("stem_layer.0.bn.bias", (CHANNELS[0],))]
    for i, (c, depth, h) in enumerate(zip(CHANNELS, DEPTHS, HEADS)):
        for b in range(depth):
            pre = f"layers.{i}.blocks.{b}."
            out += [(pre + "norm1.weight", (c,)), (pre + "norm1.bias", (c,))]
            out += [(pre + f"attn.relative_pos_{t}_table", (TABLE_ROWS, h, c // h, 3)) for t in ("query", "key", "value")]
            out += [(pre + "attn.qkv.weight", (3 * c, c)), (pre + "attn.qkv.bias", (3 * c,)), (pre + "attn.proj.weight", (c, c)),
                    (pre + "attn.proj.bias", (c,)), (pre + "norm2.weight", (c,)), (pre + "norm2.bias", (c,)),
                    (pre + "mlp.fc1.weight", (4 * c, c)), (pre + "mlp.fc1.bias", (4 * c,)), (pre + "mlp.fc2.weight", (c, 4 * c)),
                    (pre + "mlp.fc2.bias", (c,))]
        if i + 1 < len(CHANNELS):
            pre = f"layers.{i}.downsample."
            out += [(pre + "norm.weight", (c,)), (pre + "norm.bias", (c,)), (pre + "linear.weight", (CHANNELS[i + 1], c))]
    for j, i in enumerate(range(len(CHANNELS) - 1, 0, -1)):
        cin, cout = CHANNELS[i], CHANNELS[i - 1]
        pre = f"upsamples.{j}."
        out += [(pre + "linear1.0.weight", (cout,)), (pre + "linear1.0.bias", (cout,)), (pre + "linear1.1.weight", (cout, cout)),
                (pre + "linear1.1.bias", (cout,)), (pre + "linear2.0.weight", (cin,)), (pre + "linear2.0.bias", (cin,)),
                (pre + "linear2.1.weight", (cout, cin)), (pre + "linear2.1.bias", (cout,))]
    for head, width in (("classifier", CLASSES), ("regressor", 3)):
        c = CHANNELS[0]
        out += [(f"{head}.0.weight", (c, c)), (f"{head}.0.bias", (c,)), (f"{head}.1.weight", (c,)), (f"{head}.1.bias", (c,)),
                (f"{head}.3.weight", (width, c)), (f"{head}.3.bias", (width,))]
    return out


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class Variant:
    def __init__(self, name, shapes, make_opt, make_scaler, seed=0):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.name = name
        self.params = [(torch.randn(s, device="cuda", generator=gen) * 0.02).requires_grad_(True) for _, s in shapes]
        for p in self.params:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen)
        blocks = [p for (n, _), p in zip(shapes, self.params) if "blocks" in n]
        rest = [p for (n, _), p in zip(shapes, self.params) if "blocks" not in n]
        self.opt = make_opt([dict(params=rest, lr=6e-3), dict(params=blocks, lr=6e-4)])
        self.scaler = make_scaler() if make_scaler is not None else None
        if self.scaler is not None:
            self.scaler.scale(torch.zeros((), device="cuda"))

    def step(self):
        if self.scaler is None:
            self.opt.step()
        else:
            self.scaler.step(self.opt)
            self.scaler.update()

def variants(shapes, only=None):
    from stratified_transformer_amd import optim
    kw = dict(weight_decay=0.01)
    scaler_kw = dict(init_scale=1.0, growth_interval=10 ** 9)
    makers = {
        "fused": (lambda g: optim.AdamW(g, **kw), lambda: optim.GradScaler("cuda", **scaler_kw)),
        "torch_foreach": (lambda g: torch.optim.AdamW(g, **kw), lambda: torch.amp.GradScaler("cuda", **scaler_kw)),
        "torch_fused": (lambda g: torch.optim.AdamW(g, fused=True, **kw), lambda: torch.amp.GradScaler("cuda", **scaler_kw)),
        "torch_single": (lambda g: torch.optim.AdamW(g, foreach=False, **kw), lambda: torch.amp.GradScaler("cuda", **scaler_kw)),
    }
    out = []
    for name, (make_opt, make_scaler) in makers.items():
        for with_scaler in (True, False):
            full = name + ("+scaler" if with_scaler else "")
            if only is None or full in only:
                out.append(Variant(full, shapes, make_opt, make_scaler if with_scaler else None))
    return out


def byte_share(summary, kernel, nbytes):
    """adds to a kernel's row of timing.kernel_summary the bytes it must move and their share of the byte bound at its median time"""
    if kernel in summary:
        summary[kernel]["bytes"] = nbytes
        summary[kernel]["share_of_6.3TB/s"] = round(nbytes / (summary[kernel]["median_us"] * 1e-6) / HBM_BYTES_PER_S, 3)


def trace_summary(path, elements):
    """the optimizer step's kernels in a rocprofv3 kernel_trace.csv, with the update's and the check's share of the byte bound"""
    out = timing.kernel_summary(timing.kernel_times_csv(path), KERNELS)
    byte_share(out, "optim_adamw_kernel", UPDATE_BYTES_PER_ELEMENT * elements)
    byte_share(out, "optim_check_kernel", 4 * elements)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0, help="run only this many fused steps with a scaler (for a run under rocprofv3)")
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 kernel_trace.csv of a --trace-steps run to summarise")
    ap.add_argument("--merge", default=None, help="with --kernel-trace: the bench JSON to add the summary to")
    args = ap.parse_args()
    shapes = s3dis_shapes()
    elements = sum(numel(s) for _, s in shapes)
    counts = dict(tensors=len(shapes), elements=elements, blocks_tensors=sum("blocks" in n for n, _ in shapes),
                  smallest=min(numel(s) for _, s in shapes), largest=max(numel(s) for _, s in shapes))
    if args.kernel_trace:
        summary = trace_summary(args.kernel_trace, elements)
        if args.merge:
            timing.merge(args.merge, "kernel_trace", summary)
        else:
            print(json.dumps(dict(kernel_trace=summary)))
        return
    timing.need_gpu("bench_optim")
    print("parameter set:", counts, file=sys.stderr)
    if args.trace_steps:
        v = variants(shapes, only=["fused+scaler"])[0]
        for _ in range(args.trace_steps):
            v.step()
        torch.cuda.synchronize()
        print(json.dumps(dict(traced_steps=args.trace_steps, **counts)))
        return
    times = timing.wall_windows({v.name: v.step for v in variants(shapes)}, args.windows, args.warmup, args.steps)
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, parameter_set=counts, steps_per_window=args.steps,
                  windows=args.windows, warmup_windows=args.warmup, unit="ms per step, host clock around a window that ends in a synchronise",
                  byte_bound_us=dict(update=round(UPDATE_BYTES_PER_ELEMENT * elements / HBM_BYTES_PER_S * 1e6, 1),
                                     check=round(4 * elements / HBM_BYTES_PER_S * 1e6, 1)),
                  variants={k: dict(median_ms=round(statistics.median(v), 4), spread=timing.spread(v)) for k, v in times.items()},
                  not_measured=NOT_MEASURED)
    timing.emit(result, args.out)


if __name__ == "__main__":
    main()
