"""One batch-norm site of the stem and the heads - BatchNorm1d in training mode, the activation, for unary_2 the shortcut add, backward - as
torch runs it (the composite: F.batch_norm, the activation, `+=`) beside pointops.batch_norm_act (csrc/batchnorm.hip), on the same GPU and
inputs, the sides alternating; then the stand-in stem + heads of tests/stem_standin.py, unfused beside layers.fuse_batch_norms.  Prints ONE
JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_norm.py [--reps 15] [--warmup 5] [--inner 20] [--out FILE] [--trace-loop N] [--no-model]
    python tools/bench_norm.py --kernel-stats DIR/NAME_results.db --trace-loop N --out profiles/batchnorm_kernel_stats.csv     (no GPU: kernel_stats below)

Sites: N in (100 000, 600 000) x C in (12, 48), in fp32 and as under autocast(f16) (the rows in half, as the Linear in front yields them;
parameters and the shortcut fp32), with leaky_relu(0.2), relu and tanh; at C = 48 also with the residual; and the eval-mode forward
alone under no_grad.  A side is one forward + backward to x, weight, bias (and the residual).  Model: StemHeads (Simple(3 -> 48),
Res(48), a ReLU classifier to 19 classes, a Tanh regressor) with the real KPConvLayer on a room of 100 000 points, train mode,
forward + backward.

Every case is set up first and each of its sides run `inner` times untimed, so that no timed window pays for a first call of anything; then
every figure: median over `reps` windows of `inner` iterations between two device events (the second synchronised), in ms per iteration;
`spread` = max - min of a side over its windows.  `bytes` = what the fused passes must move, from the shapes (fused_bytes below);
`achieved_bytes_per_s` = those bytes over the fused time - launch gaps, allocations and autograd included, so it is a call's rate, not a
kernel's.  `faster_beyond_spread`: composite - fused > the composite's spread.
"""
import argparse
import statistics

import torch
import torch.nn.functional as F

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import layers, scene  # noqa: E402
from stratified_transformer_amd import pointops as P  # noqa: E402

SLOPE, MOMENTUM = 0.2, 0.02
ROWS, CHANNELS, ACTS = (100000, 600000), (12, 48), ("leaky_relu", "relu", "tanh")


def fused_bytes(n, c, half, residual, training=True, backward=True):
    """per kernel, from the shapes: moments reads x; forward reads x (and the fp32 residual), writes o; the sums read x and dO; dx reads x
    and dO, writes dx.  The [C]-sized operands and the partials (at most 1024 x 3 x C floats) are left out."""
    b = 2 if half else 4
    k = {"bn_moments_kernel": n * c * b if training else 0, "bn_fwd_kernel": n * c * (2 * b + (4 if residual else 0))}
    if backward:
        k["bn_bwd_kernel<sums>"] = n * c * 2 * b
        k["bn_bwd_kernel<dx>"] = n * c * 3 * b
    return k


def _act(pre, act):
    return F.leaky_relu(pre, SLOPE) if act == "leaky_relu" else F.relu(pre) if act == "relu" else torch.tanh(pre)


def site(n, c, half, act, residual, eval_forward, a):
    """-> (row, sides) of one site; eval_forward: the eval-mode forward alone, under no_grad"""
    g = torch.Generator(device="cuda").manual_seed(n + c)
    dt = torch.float16 if half else torch.float32
    x = (0.3 + 1.5 * torch.randn(n, c, device="cuda", generator=g)).to(dt).requires_grad_(not eval_forward)
    go = torch.randn(n, c, device="cuda", generator=g).to(dt)
    res = torch.randn(n, c, device="cuda", generator=g).requires_grad_(True) if residual else None
    w = (1 + 0.2 * torch.randn(c, device="cuda", generator=g)).requires_grad_(not eval_forward)
    b = (0.2 * torch.randn(c, device="cuda", generator=g)).requires_grad_(not eval_forward)
    stats = {s: (torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")) for s in ("composite", "fused")}
    leaves = [t for t in (x, w, b, res) if t is not None]

    def composite():
        rm, rv = stats["composite"]
        if eval_forward:
            with torch.no_grad():
                return _act(F.batch_norm(x, rm, rv, w, b, False, MOMENTUM, 1e-5), act)
        for t in leaves:
            t.grad = None
        o = _act(F.batch_norm(x, rm, rv, w, b, True, MOMENTUM, 1e-5), act)
        if res is not None:
            o += res                                              # model/stratified_transformer.py:391, in place on the rows
        o.backward(go)
        return o

    def fused():
        rm, rv = stats["fused"]
        if eval_forward:
            with torch.no_grad():
                return P.batch_norm_act(x, w, b, rm, rv, False, MOMENTUM, 1e-5, act, SLOPE)
        for t in leaves:
            t.grad = None
        o = P.batch_norm_act(x, w, b, rm, rv, True, MOMENTUM, 1e-5, act, SLOPE, res)
        o.backward(go)
        return o

    oc = composite().detach().float()
    gc = None if eval_forward else x.grad.detach().float().clone()
    of = fused().detach().float()
    row = {"n": n, "c": c, "rows": "f16" if half else "f32", "act": act, "residual": bool(residual), "eval_forward": bool(eval_forward),
           "max_abs_diff_o": float((oc - of).abs().max()), "max_abs_diff_dx": None if eval_forward else float((gc - x.grad.float()).abs().max())}
    sides = {"composite": composite, "fused": fused}
    for fn in sides.values():
        for _ in range(a.inner):
            fn()
    torch.cuda.synchronize()
    return row, sides


def timed_row(row, sides, a):
    row.update(timing.summary(timing.windows(sides, a.reps, a.warmup, a.inner), "composite", "fused"))
    row["kernel_bytes"] = fused_bytes(row["n"], row["c"], row["rows"] == "f16", row["residual"], not row["eval_forward"], not row["eval_forward"])
    row["bytes"] = sum(row["kernel_bytes"].values())
    row["achieved_bytes_per_s"] = round(row["bytes"] / (row["fused_ms"] * 1e-3), 1)
    return row


def site_cases():
    for half in (False, True):
        for n in ROWS:
            for c in CHANNELS:
                for act in ACTS:
                    yield n, c, half, act, False, False
                if c == 48:
                    yield n, c, half, "leaky_relu", True, False
                yield n, c, half, "leaky_relu", False, True


def trace_cases():
    """the sites --trace-loop runs, in its order: (n, c, half, residual)"""
    return [(n, c, half, c == 48) for half in (False, True) for n in ROWS for c in CHANNELS]


def kernel_stats(db_path, loop, out_path):
    """Per-shape kernel times from the database `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_norm.py --trace-loop
    LOOP` leaves (DIR/NAME_results.db; `--stats` itself aggregates by kernel name over all shapes).  Every fused call dispatches each of the six
    kernels once and the sites run one after the other, so the dispatches of a kernel, in start order, fall into runs of LOOP + 2 per site
    (site() calls the fused side twice while setting up); the medians are over the LOOP calls behind those two.  Writes
    kernel,n,c,dtype,residual,calls,median_us,min_us,max_us,bytes,tbytes_per_s_at_median."""
    import csv
    import re
    per = {}
    for name, us in timing.kernel_times_db(db_path):
        m = re.search(r"(bn_\w+_kernel)(<[^>]*>)?", name)
        if m is None:
            continue
        key = m.group(1)
        if key == "bn_bwd_kernel":
            key += "<sums>" if "true" in (m.group(2) or "") else "<dx>"
        per.setdefault(key, []).append(us)
    cases, calls = trace_cases(), loop + 2
    with open(out_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("kernel", "n", "c", "dtype", "residual", "calls", "median_us", "min_us", "max_us", "bytes", "tbytes_per_s_at_median"))
        for key, times in per.items():
            if len(times) != calls * len(cases):
                raise SystemExit(f"bench_norm: {key}: {len(times)} dispatches, expected {calls} x {len(cases)} (was the trace made with --trace-loop {loop}?)")
            for i, (n, c, half, residual) in enumerate(cases):
                t = times[calls * i + 2:calls * (i + 1)]
                med, nbytes = statistics.median(t), fused_bytes(n, c, half, residual).get(key)
                w.writerow((key, n, c, "f16" if half else "f32", int(residual), len(t), round(med, 2), round(min(t), 2), round(max(t), 2),
                            nbytes if nbytes else "", round(nbytes / (med * 1e-6) / 1e12, 3) if nbytes else ""))


def model_case(n_points, amp, a):
    """the stand-in stem + heads, unfused beside fused (two copies of one model), forward + backward in train mode"""
    import copy
    from tests import stem_standin as S
    xyz_h, offset_h = scene.make_batch([n_points], seed=7)
    xyz, offset = torch.from_numpy(xyz_h).cuda(), torch.from_numpy(offset_h).cuda()
    nb, _ = P.ball_query(2.5 * S.GRID, 34, xyz, xyz, offset, offset)
    nb = nb.contiguous()
    n = xyz.shape[0]
    torch.manual_seed(3)
    models = {"composite": S.shake_norms(S.StemHeads(S.kp_conv), 4).cuda().train()}
    models["fused"] = copy.deepcopy(models["composite"])
    sites = layers.fuse_batch_norms(models["fused"])
    g = torch.Generator(device="cuda").manual_seed(5)
    feats = torch.rand(n, 3, device="cuda", generator=g)
    go = (torch.randn(n, 19, device="cuda", generator=g), torch.randn(n, 3, device="cuda", generator=g))

    def run(model):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            cls, reg = model(feats, xyz, None, nb)
        torch.autograd.backward([cls, reg], [go[0].to(cls.dtype), go[1].to(reg.dtype)])
        return cls

    outs = {k: run(m).detach().float() for k, m in models.items()}
    row = {"points": n, "precision": "autocast_f16" if amp else "fp32", "sites": sites,
           "max_abs_diff_classes": float((outs["composite"] - outs["fused"]).abs().max())}
    sides = {k: (lambda m=m: run(m)) for k, m in models.items()}
    for fn in sides.values():
        for _ in range(max(2, a.inner // 4)):
            fn()
    torch.cuda.synchronize()
    return row, sides


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--trace-loop", type=int, default=0, help="only loop the fused side this many times per site (for a kernel trace)")
    ap.add_argument("--no-model", action="store_true", help="the sites alone")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, metavar="DB", help="no GPU work: split the kernel trace DB of a --trace-loop N run by site into --out (csv)")
    a = ap.parse_args()
    if a.kernel_stats:
        if not (a.trace_loop and a.out):
            raise SystemExit("bench_norm: --kernel-stats DB needs --trace-loop N (as the traced run had it) and --out FILE")
        return kernel_stats(a.kernel_stats, a.trace_loop, a.out)
    if a.reps < 5:
        raise SystemExit("bench_norm: at least five repeats a side")
    timing.need_gpu("bench_norm")
    if a.trace_loop:
        # for a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_norm.py --trace-loop 50`: the fused side only,
        # one site per (N, C, precision) - leaky_relu, with the residual at C = 48 - so that the per-kernel averages belong to one shape each
        for n, c, half, residual in trace_cases():
            _, sides = site(n, c, half, "leaky_relu", residual, False, argparse.Namespace(inner=1))
            for _ in range(a.trace_loop):
                sides["fused"]()
            torch.cuda.synchronize()
        return
    result = {"tool": "bench_norm", "device": torch.cuda.get_device_name(0), "negative_slope": SLOPE, "momentum": MOMENTUM, "reps": a.reps,
              "warmup": a.warmup, "inner": a.inner, "sites": [], "model": []}
    for args in site_cases():                      # (a case at a time: 600 000 x 48 rows in four copies a side are not kept for all cases at once)
        row, sides = site(*args, a)
        result["sites"].append(timed_row(row, sides, a))
        del sides
        torch.cuda.empty_cache()
    if not a.no_model:
        inner = max(2, a.inner // 4)
        for amp in (False, True):
            row, sides = model_case(100000, amp, a)
            row.update(timing.summary(timing.windows(sides, a.reps, a.warmup, inner), "composite", "fused"))
            result["model"].append(row)
    result["sites_faster_beyond_spread"] = sum(r["faster_beyond_spread"] for r in result["sites"])
    result["sites_total"] = len(result["sites"])
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
