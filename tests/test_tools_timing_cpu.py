"""tools/timing.py without a GPU: what the bench tools report of a list of times (summary, spread), their output tail (emit, merge), and
that every tools/bench_*.py imports on its own and keeps no timing helper of its own."""
import ast
import glob
import importlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
BENCH_TOOLS = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "bench_*.py")))
HELPER_NAMES = {"windows", "summary", "spread", "device_ms", "timed_pair", "median_ms", "timeit", "merge", "timed", "host_ms", "limited", "summarize_trace", "kernel_summary"}
# what one tool may take from another: scene and workload builders.  bench_optim's are its parameter set, its Variant (an optimizer on
# that set: no clock in it), the kernels a traced step launches and the bytes they must move
SHARED_BUILDERS = {"bench_contacts": {"make_scene", "box"},
                   "bench_optim": {"s3dis_shapes", "variants", "Variant", "numel", "HBM_BYTES_PER_S", "trace_summary", "byte_share"}}


@pytest.fixture(scope="module")
def timing():
    sys.path.insert(0, TOOLS)
    try:
        yield importlib.import_module("timing")
    finally:
        sys.path.remove(TOOLS)


def test_summary_gain_within_the_spread(timing):
    times = {"composite": [1.0, 1.2, 1.1, 1.4, 1.3], "fused": [0.9, 1.0, 0.8, 1.0, 0.9]}
    assert timing.summary(times, "composite", "fused") == {
        "composite_ms": 1.2, "fused_ms": 0.9, "composite_spread_ms": 0.4, "fused_spread_ms": 0.2, "ratio": 1.333, "faster_beyond_spread": False}


def test_summary_gain_beyond_the_spread(timing):
    times = {"a": [2.0, 2.1, 2.2], "b": [1.0, 1.0, 1.5]}
    assert timing.summary(times, "a", "b") == {"a_ms": 2.1, "b_ms": 1.0, "a_spread_ms": 0.2, "b_spread_ms": 0.5, "ratio": 2.1,
                                               "faster_beyond_spread": True}


def test_summary_gain_equal_to_the_spread_is_not_beyond_it(timing):
    times = {"a": [2.0, 2.5, 3.0], "b": [1.5, 1.5, 1.5]}        # binary fractions: 2.5 - 1.5 == 3.0 - 2.0 exactly
    r = timing.summary(times, "a", "b")
    assert r == {"a_ms": 2.5, "b_ms": 1.5, "a_spread_ms": 1.0, "b_spread_ms": 0.0, "ratio": 1.667, "faster_beyond_spread": False}
    assert r["a_ms"] - r["b_ms"] == r["a_spread_ms"]


def test_summary_slower_side(timing):
    times = {"a": [1.0, 1.0, 1.0], "b": [2.0, 2.25, 2.0]}
    r = timing.summary(times, "a", "b")
    assert r == {"a_ms": 1.0, "b_ms": 2.0, "a_spread_ms": 0.0, "b_spread_ms": 0.25, "ratio": 0.5, "faster_beyond_spread": False}
    assert type(r["faster_beyond_spread"]) is bool


def test_spread_of_five(timing):
    assert timing.spread([3.0, 1.0, 5.0, 2.0, 4.0]) == [1.0, 1.5, 4.5, 5.0]
    assert timing.spread([0.123456, 0.2, 0.3, 0.4, 0.567891]) == [0.1235, 0.1617, 0.4839, 0.5679]


def test_fwd_bwd_summary(timing):
    times = {("hip", False): [0.2, 0.1, 0.3], ("hip", True): [0.5, 0.7, 0.6]}
    assert timing.fwd_bwd_summary(times, "hip") == {"fwd_ms": 0.2, "fwd_bwd_ms": 0.6, "fwd_bwd_ms_min": 0.5, "fwd_bwd_ms_max": 0.7}


def test_merge_creates_then_adds(timing, tmp_path, capsys):
    path = str(tmp_path / "bench.json")
    timing.merge(path, "first", {"x": 1})
    assert json.load(open(path)) == {"first": {"x": 1}}
    timing.merge(path, "second", [1, 2])
    assert json.load(open(path)) == {"first": {"x": 1}, "second": [1, 2]}
    assert capsys.readouterr().out.splitlines() == ['{"first": {"x": 1}}', '{"second": [1, 2]}']


def test_emit_writes_the_printed_line(timing, tmp_path, capsys):
    path = str(tmp_path / "out.json")
    result = {"tool": "t", "ms": 0.25, "rows": [1, 2]}
    timing.emit(result, path)
    printed = capsys.readouterr().out
    assert printed == json.dumps(result) + "\n"
    assert open(path).read() == printed
    timing.emit(result)                                           # no --out: the line alone
    assert capsys.readouterr().out == printed


def test_need_gpu_message(timing, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match=r"bench_x: needs the GPU \(no CPU timing is meaningful\)"):
        timing.need_gpu("bench_x")


def test_timing_imports_torch_and_the_standard_library_only():
    tree = ast.parse(open(os.path.join(TOOLS, "timing.py")).read())
    mods = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    mods |= {n.module.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert mods - {"torch"} <= set(sys.stdlib_module_names)


@pytest.mark.parametrize("name", BENCH_TOOLS)
def test_bench_tool_imports_without_a_gpu(timing, name, monkeypatch):
    monkeypatch.setattr(sys, "argv", [name + ".py"])
    mod = importlib.import_module(name)
    assert callable(mod.main)


def test_bench_tools_keep_no_timing_helper():
    assert len(BENCH_TOOLS) >= 19
    for name in BENCH_TOOLS:
        tree = ast.parse(open(os.path.join(TOOLS, name + ".py")).read())
        defined = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
        assert not defined & HELPER_NAMES, (name, defined & HELPER_NAMES)
        for n in ast.walk(tree):
            if isinstance(n, ast.ImportFrom) and n.module and n.module.startswith("bench_"):
                assert {a.name for a in n.names} <= SHARED_BUILDERS.get(n.module, set()), (name, n.module)
            if isinstance(n, ast.Import):
                for a in n.names:
                    if a.name.startswith("bench_"):                # a tool imported whole: every attribute taken from it
                        alias = a.asname or a.name
                        taken = {x.attr for x in ast.walk(tree) if isinstance(x, ast.Attribute) and isinstance(x.value, ast.Name) and x.value.id == alias}
                        assert taken <= SHARED_BUILDERS.get(a.name, set()), (name, a.name, taken)
