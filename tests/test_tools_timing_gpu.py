"""tools/timing.py on the device: the loops call what they are given as often and in the order they say, and return what they say.  Nothing
here asserts a speed."""
import importlib
import math
import os
import sys

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
REPS, WARMUP, INNER = 3, 1, 2


@pytest.fixture(scope="module")
def timing():
    sys.path.insert(0, TOOLS)
    try:
        yield importlib.import_module("timing")
    finally:
        sys.path.remove(TOOLS)


def two_sides():
    x = torch.arange(1024, dtype=torch.float32, device="cuda")
    order = []

    def side(name, op):
        def fn():
            order.append(name)
            return op(x)
        return fn

    return {"add": side("add", lambda t: t + 1.0), "mul": side("mul", lambda t: t * 2.0)}, order, x


@pytest.mark.gpu
def test_windows_calls_and_wall_ms(timing):
    sides, order, x = two_sides()
    times = timing.windows(sides, REPS, WARMUP, INNER)
    assert list(times) == ["add", "mul"]
    for ts in times.values():
        assert len(ts) == REPS and all(math.isfinite(t) and t > 0 for t in ts)
    assert order == (["add"] * INNER + ["mul"] * INNER) * (WARMUP + REPS)

    prepared = []
    timing.windows(sides, REPS, WARMUP, INNER, prepare=lambda: prepared.append(len(order)))
    assert prepared == [len(order) // 2 + INNER * i for i in range(2 * (WARMUP + REPS))]      # once ahead of every window

    del order[:]
    (add_dev, add_host, add_out), (mul_dev, mul_host, mul_out) = timing.calls(list(sides.values()), REPS, WARMUP)
    assert order == ["add", "mul"] * (WARMUP + REPS)
    for ts in (add_dev, add_host, mul_dev, mul_host):
        assert len(ts) == REPS and all(math.isfinite(t) and t > 0 for t in ts)
    assert torch.equal(add_out, x + 1.0) and torch.equal(mul_out, x * 2.0)

    ms, out = timing.wall_ms(sides["mul"])
    assert math.isfinite(ms) and ms > 0 and torch.equal(out, x * 2.0)
    dev, host, out = timing.device_ms(sides["add"], REPS, WARMUP)
    assert dev > 0 and host > 0 and torch.equal(out, x + 1.0)
