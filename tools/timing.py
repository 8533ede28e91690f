"""How the tools under tools/ time: every bench_*.py takes its loops, its summaries and its output tail from here, and none takes a timing
helper from another tool (scene and workload builders are what they still share).  Importing this module also puts the repository root on
sys.path, so a tool run as `python tools/NAME.py` writes `import timing` ahead of its imports from the package and from tests/.

The four loops - which one a tool uses is part of what its numbers mean, so they stay apart:

    windows       device events around a window of `inner` calls, the second event synchronised, no synchronise in front; the sides
                  alternate window by window.  `prepare` runs ahead of a window's first event (gradients cleared outside the timed region).
                  bench_block, bench_norm, bench_loss, bench_syncbn; bench_kpconv, bench_transition, bench_swin, bench_upsample (inner 1, with prepare);
                  bench_ops, bench_stages (one_window_us: one window of one side)
    calls         one call at a time: synchronise, host clock, event, the call, event, synchronise; the callables alternate.  Device and
                  host ms per call.  bench_augment, bench_detect's vote, knn_only; as device_ms (medians of one callable) bench_contacts,
                  bench_merge, bench_supports
    wall_ms       host clock around one call between two synchronises, for calls that read back; wall_times / median_wall_ms repeat it.
                  bench_evaltile, bench_dbscan, bench_detect
    wall_windows  host clock around a window of `inner` calls between two synchronises, the sides alternating.  bench_optim, bench_sgd_clip

Loops that are none of these stay in their tools: bench_cell (three events: forward and backward apart), fps_only (chained host stamps),
pass_times (no synchronise in front of a pass), bench_dbscan.phase_times (a synchronise in front of every library launch).

The two kernel-time readers read different files and stay two: kernel_times_db the sqlite database `rocprofv3 --kernel-trace --stats -d DIR
-o NAME` leaves (DIR/NAME_results.db; bench_norm --kernel-stats), kernel_times_csv the *_kernel_trace.csv of `rocprofv3 --kernel-trace
--output-format csv` (bench_optim / bench_sgd_clip --kernel-trace).  Both give [(kernel name, us)]; kernel_summary groups them by a
pattern of names (bench_optim, bench_sgd_clip); bench_norm splits its by site, which only it knows.
"""
import json
import os
import signal
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def need_gpu(tool_name):
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool_name}: needs the GPU (no CPU timing is meaningful)")


class limited:
    """a GPU step under its own time limit: the alarm's default action ends the process"""

    def __init__(self, seconds):
        self.seconds = int(seconds)

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


# ---- the loops ----
def windows(sides, reps, warmup, inner=1, prepare=None):
    """sides: name -> fn(); -> name -> list of ms per iteration, the sides alternating window by window.  prepare: fn() run ahead of
    every window, outside its events"""
    times = {s: [] for s in sides}
    for it in range(warmup + reps):
        for s, fn in sides.items():
            if prepare is not None:
                prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[s].append(e0.elapsed_time(e1) / inner)
    return times


def one_window_us(fn, inner=10, warmup=3):
    """`warmup` untimed calls, a synchronise, then one window of `inner` calls -> us per call.  The window ends in the second event's
    synchronize(), where bench_ops / bench_stages had torch.cuda.synchronize(): one synchronisation either way, and the same wait as
    long as everything runs on the one current stream, which it does in both tools"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return windows({"fn": fn}, 1, 0, inner)["fn"][0] * 1e3


def fwd_bwd_windows(sides, clear, backward, reps, warmup):
    """sides: name -> fn() giving the output.  Per side a window of the forward and a window of forward + backward(out), one call each,
    clear() ahead of each window's events (gradients go outside the timed region).
    -> (times keyed (side, with backward), name -> (output, what backward returned) of the side's last forward + backward)"""
    last = {}

    def run(s, with_backward):
        out = sides[s]()
        if with_backward:
            last[s] = (out, backward(out))

    runs = {(s, b): (lambda s=s, b=b: run(s, b)) for s in sides for b in (False, True)}
    return windows(runs, reps, warmup, prepare=clear), last


def calls(fns, reps, warmup):
    """alternate the callables; -> per callable (device ms list, host ms list, last result)"""
    dev = [[] for _ in fns]
    host = [[] for _ in fns]
    out = [None] * len(fns)
    for it in range(warmup + reps):
        for k, fn in enumerate(fns):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            out[k] = fn()
            end.record()
            torch.cuda.synchronize()
            if it >= warmup:
                dev[k].append(start.elapsed_time(end))
                host[k].append((time.perf_counter() - t0) * 1e3)
    return [(dev[k], host[k], out[k]) for k in range(len(fns))]


def device_ms(fn, reps, warmup):
    """-> (median device ms, median host ms, last result)"""
    dev, host, out = calls([fn], reps, warmup)[0]
    return statistics.median(dev), statistics.median(host), out


def wall_ms(fn):
    """-> (host ms between two synchronises, result)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def wall_times(fn, reps, warmup):
    """-> (wall_ms of each of `reps` calls after `warmup` calls, last result)"""
    times, out = [], None
    for it in range(warmup + reps):
        ms, out = wall_ms(fn)
        if it >= warmup:
            times.append(ms)
    return times, out


def median_wall_ms(fn, reps, warmup):
    return statistics.median(wall_times(fn, reps, warmup)[0])


def wall_windows(sides, reps, warmup, inner):
    """windows on the host clock: name -> list of ms per iteration, each window between two synchronises"""
    def window(fn):
        for _ in range(inner):
            fn()

    times = {s: [] for s in sides}
    for it in range(warmup + reps):
        for s, fn in sides.items():
            ms = wall_ms(lambda: window(fn))[0] / inner
            if it >= warmup:
                times[s].append(ms)
    return times


# ---- what is reported of a list of times ----
def summary(times, base, new):
    r = {base + "_ms": round(statistics.median(times[base]), 5), new + "_ms": round(statistics.median(times[new]), 5),
         base + "_spread_ms": round(max(times[base]) - min(times[base]), 5), new + "_spread_ms": round(max(times[new]) - min(times[new]), 5)}
    r["ratio"] = round(r[base + "_ms"] / r[new + "_ms"], 3)
    r["faster_beyond_spread"] = bool(r[base + "_ms"] - r[new + "_ms"] > r[base + "_spread_ms"])
    return r


def spread(ts):
    """[min, lower quartile, upper quartile, max] (bench_augment, bench_optim, bench_sgd_clip: they had one definition between them)"""
    q = statistics.quantiles(ts, n=4)
    return [round(min(ts), 4), round(q[0], 4), round(q[2], 4), round(max(ts), 4)]


def fwd_bwd_summary(times, side):
    """times: (side, backward) -> ms list of a windows() run over forward and forward + backward"""
    fwd, both = times[(side, False)], times[(side, True)]
    return {"fwd_ms": round(statistics.median(fwd), 4), "fwd_bwd_ms": round(statistics.median(both), 4),
            "fwd_bwd_ms_min": round(min(both), 4), "fwd_bwd_ms_max": round(max(both), 4)}


# ---- the output tail ----
def emit(result, out_path=None):
    """print the result as ONE JSON line and write the same line to out_path"""
    line = json.dumps(result)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


def merge(path, key, value):
    """set one key of the JSON file at path (made if it is not there) and print that key"""
    result = json.load(open(path)) if os.path.exists(path) else {}
    result[key] = value
    with open(path, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps({key: value}))


# ---- kernel times from a rocprofv3 run (module docstring: two file formats) ----
def kernel_times_db(db_path):
    """[(kernel name, us)] in start order"""
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, start, end from kernels order by start").fetchall()
    return [(name, (end - start) / 1000.0) for name, start, end in rows]


def kernel_times_csv(path):
    """[(kernel name, us)] in file order"""
    import csv
    return [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(path))]


def kernel_summary(times, pattern):
    """times: [(kernel name, us)]; -> matched part of the name -> calls, median / min / max us, for the names `pattern` finds"""
    import re
    per = {}
    for name, us in times:
        m = re.search(pattern, name)
        if m is not None:
            per.setdefault(m.group(0), []).append(us)
    return {k: dict(calls=len(v), median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in per.items()}
