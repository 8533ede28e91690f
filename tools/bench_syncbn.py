"""One synchronised batch-norm site in training mode - the norm, leaky_relu(0.2), backward - as ONE rank of four runs it, on one GPU:

    sync         pointops.sync_batch_norm_act (csrc/batchnorm.hip: moments + row kernel, merge, normalise; sums + param kernel, dx)
    plain        pointops.batch_norm_act at the same shape: the unsynchronised operator, which this path extends by the two small kernels
                 and the two gathers (its code and its launches are the parent commit's)
    torch_chain  torch's own kernel chain for nn.SyncBatchNorm in the order of torch.nn.modules._functions.SyncBatchNorm:
                 batch_norm_stats, batch_norm_gather_stats_with_counts, batch_norm_elemt, the activation; batch_norm_backward_reduce,
                 batch_norm_backward_elemt

ONE GPU is what there is, so this is the per-rank DEVICE work: on the sync and the torch_chain side alike every collective is replaced by
a local copy of this rank's row into a buffer of world = 4 rows (four ranks holding the same rows: the statistics are the rank's own, the
count is 4 n).  No collective runs: RCCL's latency, a real multi-GPU step and the unmodified model under DDP are NOT measured here.
Prints ONE JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_syncbn.py [--reps 15] [--warmup 5] [--inner 20] [--out profiles/syncbn_bench.json]

Sites: 25 000 x 48 (a rank's share of a room) and 100 000 x 48 (a whole room), fp32 rows and f16 rows as under autocast.  A side is one
forward + backward to x, weight, bias.  Every side runs `inner` times untimed first; then every figure is the median over `reps` windows
of `inner` iterations between two device events, in ms per iteration, the sides alternating window by window; `spread` = max - min of a
side over its windows.  `gain_over_torch_chain_beyond_both_spreads`: torch_chain - sync > max(the two spreads).
"""
import argparse
import statistics

import torch
import torch.nn.functional as F

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import pointops as P  # noqa: E402
from stratified_transformer_amd import sharding  # noqa: E402

SLOPE, MOMENTUM, EPS, WORLD = 0.2, 0.02, 1e-5, 4
ROWS, CHANNELS = (25000, 100000), 48


def local_gather(row, group=None):
    """what stands in for sharding.all_gather_rows: this rank's row copied into each of WORLD rows, on the device"""
    return row.unsqueeze(0).expand((WORLD,) + tuple(row.shape)).contiguous()


class TorchSyncChain(torch.autograd.Function):
    """torch.nn.modules._functions.SyncBatchNorm's kernels in its order, its all_gather and all_reduce replaced by local copies"""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, momentum):
        mean, invstd = torch.batch_norm_stats(x, eps)
        count = torch.full((1,), x.shape[0], dtype=mean.dtype, device=x.device)
        combined = local_gather(torch.cat([mean, invstd, count], 0))                      # [world, 2 C + 1], as the module gathers it
        mean_all, invstd_all, count_all = torch.split(combined, x.shape[1], dim=1)
        mean, invstd = torch.batch_norm_gather_stats_with_counts(x, mean_all, invstd_all, running_mean, running_var, momentum, eps, count_all.view(-1))
        ctx.save_for_backward(x, weight, mean, invstd, count_all.to(torch.int32))
        return torch.batch_norm_elemt(x, weight, bias, mean, invstd, eps)

    @staticmethod
    def backward(ctx, grad_output):
        grad_output = grad_output.contiguous()
        x, weight, mean, invstd, count = ctx.saved_tensors
        sum_dy, sum_dy_xmu, grad_weight, grad_bias = torch.batch_norm_backward_reduce(grad_output, x, mean, invstd, weight, True, True, True)
        combined = torch.cat([sum_dy, sum_dy_xmu], 0).clone()                              # (the module all-reduces this buffer)
        sum_dy, sum_dy_xmu = torch.split(combined, x.shape[1])
        grad_input = torch.batch_norm_backward_elemt(grad_output, x, mean, invstd, weight, sum_dy, sum_dy_xmu, count.view(-1))
        return grad_input, grad_weight, grad_bias, None, None, None, None


def site(n, c, half, a):
    g = torch.Generator(device="cuda").manual_seed(n + c)
    dt = torch.float16 if half else torch.float32
    x = (0.3 + 1.5 * torch.randn(n, c, device="cuda", generator=g)).to(dt).requires_grad_(True)
    go = torch.randn(n, c, device="cuda", generator=g).to(dt)
    w = (1 + 0.2 * torch.randn(c, device="cuda", generator=g)).requires_grad_(True)
    b = (0.2 * torch.randn(c, device="cuda", generator=g)).requires_grad_(True)
    stats = {s: (torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")) for s in ("sync", "plain", "torch_chain")}
    leaves = (x, w, b)

    def run(make):
        for t in leaves:
            t.grad = None
        o = make()
        o.backward(go)
        return o

    sides = {
        "sync": lambda: run(lambda: P.sync_batch_norm_act(x, w, b, *stats["sync"], MOMENTUM, EPS, "leaky_relu", SLOPE)),
        "plain": lambda: run(lambda: P.batch_norm_act(x, w, b, *stats["plain"], True, MOMENTUM, EPS, "leaky_relu", SLOPE)),
        "torch_chain": lambda: run(lambda: F.leaky_relu(TorchSyncChain.apply(x, w, b, *stats["torch_chain"], EPS, MOMENTUM), SLOPE)),
    }
    outs, grads = {}, {}
    for name, fn in sides.items():
        outs[name] = fn().detach().float()
        grads[name] = x.grad.detach().float().clone()
    row = {"n": n, "c": c, "rows": "f16" if half else "f32", "act": "leaky_relu", "world_rows": WORLD,
           "max_abs_diff_o_sync_plain": float((outs["sync"] - outs["plain"]).abs().max()),
           "max_abs_diff_dx_sync_plain": float((grads["sync"] - grads["plain"]).abs().max()),
           "max_abs_diff_o_sync_torch_chain": float((outs["sync"] - outs["torch_chain"]).abs().max())}
    for fn in sides.values():
        for _ in range(a.inner):
            fn()
    torch.cuda.synchronize()
    times = timing.windows(sides, a.reps, a.warmup, a.inner)
    for name, t in times.items():
        row[name + "_ms"] = round(statistics.median(t), 5)
        row[name + "_spread_ms"] = round(max(t) - min(t), 5)
    row["sync_minus_plain_ms"] = round(row["sync_ms"] - row["plain_ms"], 5)
    row["ratio_torch_chain_over_sync"] = round(row["torch_chain_ms"] / row["sync_ms"], 3)
    row["gain_over_torch_chain_beyond_both_spreads"] = bool(row["torch_chain_ms"] - row["sync_ms"] > max(row["torch_chain_spread_ms"], row["sync_spread_ms"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("bench_syncbn: at least five repeats a side")
    timing.need_gpu("bench_syncbn")
    sharding.all_gather_rows = local_gather                    # the collectives of the sync side: a local copy (module docstring)
    result = {"tool": "bench_syncbn", "device": torch.cuda.get_device_name(0), "negative_slope": SLOPE, "momentum": MOMENTUM, "reps": a.reps,
              "warmup": a.warmup, "inner": a.inner, "world_rows": WORLD,
              "collectives": "replaced by a local copy on the sync and the torch_chain side: per-rank device work only",
              "not_measured": ["a real multi-GPU step", "RCCL latency", "the unmodified model end to end under DDP"], "sites": []}
    for half in (False, True):
        for n in ROWS:
            result["sites"].append(site(n, CHANNELS, half, a))
            torch.cuda.empty_cache()
    result["sites_with_gain_over_torch_chain"] = sum(r["gain_over_torch_chain_beyond_both_spreads"] for r in result["sites"])
    result["sites_total"] = len(result["sites"])
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
