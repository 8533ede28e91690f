"""CPU: what the GPU tests of pointops.linear_param_grads stand on - the cases (tests/linear_grads_cases.py) and the oracle's bound
(tests/linear_grads_oracle.py) - and everything of the feature that runs without a GPU: layers.fuse_linear_grads on CPU tensors and
below the rule (torch's own bits), the rule itself, the ABI table.  No HIP compute runs here."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, layers, pointops
from tests import abi_header
from tests import linear_grads_cases as C
from tests import linear_grads_oracle as O

R = C.R


def test_the_cases_cover_every_value_the_issue_lists():
    assert pointops.LINEAR_GRADS_ROWS == R == _lib.LINEAR_GRADS_ROWS and R >= 66
    assert C.N_LIST == (0, 1, 3, 4, 5, 63, 64, 65, R - 1, R, R + 1, 3 * R + 5)
    for shape, types in (((48, 192), (C.F32, C.F32)), ((15, 17), (C.F16, C.F16))):
        ns = {c["n"] for c in C.CASES if (c["in"], c["out"]) == shape and (c["x_dtype"], c["g_dtype"]) == types and c["view"] is None}
        assert ns >= set(C.N_LIST)
    assert {(c["in"], c["out"]) for c in C.CASES} == set(C.SHAPES)
    assert {(c["x_dtype"], c["g_dtype"]) for c in C.CASES} == set(C.TYPE_PAIRS)
    assert {c["bias"] for c in C.CASES} == {True, False}
    assert {c["view"] for c in C.CASES} == {None, "strided", "3d"}
    assert all(c["n"] <= 65 for c in C.CASES if (c["in"], c["out"]) == (384, 1536))
    assert len({C.case_id(c) for c in C.CASES}) == len(C.CASES)
    for i, c in enumerate(C.CASES):
        if c["view"] is None:
            continue
        x, g = C.operands(i, "int")
        assert (x.dim() == 3 and x.shape[1] == 16) if c["view"] == "3d" else not (x.is_contiguous() or g.is_contiguous())


def test_the_exact_cases_are_exact_in_any_order():
    """entries in {-3 .. 3}, N <= 4096: every partial sum of products is bounded by 9 * 4096 < 2^24, so fp32 adds them exactly in
    any order; the entries are f16 and bf16 values"""
    assert C.INT_MAX_ABS ** 2 * C.INT_MAX_N < 2 ** 24
    for i, c in enumerate(C.CASES):
        assert c["n"] <= C.INT_MAX_N
        for t in C.operands(i, "int"):
            v = O.widen(t)
            assert np.array_equal(v, np.rint(v)) and np.abs(v).max(initial=0) <= C.INT_MAX_ABS
            for dt in (torch.float16, torch.bfloat16):
                assert np.array_equal(O.widen(t.float().to(dt)), v)
        dW, db = C.expected(i, "int")
        assert dW.dtype == np.float32 and dW.shape == (c["out"], c["in"]) and db.shape == (c["out"],)


def _accumulate32(x, g, order):
    """dW, db by a plain fp32 accumulation over the rows in `order`: rounded products, rounded additions"""
    dW, db = np.zeros((g.shape[1], x.shape[1]), np.float32), np.zeros(g.shape[1], np.float32)
    for n in order:
        dW += g[n][:, None] * x[n][None, :]
        db += g[n]
    return dW, db


@pytest.mark.parametrize("idx", [i for i, c in enumerate(C.CASES) if c["in"] * c["out"] <= 48 * 192 and c["view"] is None][::3],
                         ids=lambda i: C.case_id(C.CASES[i]))
def test_the_bound_holds_for_fp32_accumulation_in_row_order_and_shuffled(idx):
    x, g = (O.widen(t).astype(np.float32) for t in C.operands(idx, "random"))
    want = C.expected(idx, "random")
    n = x.shape[0]
    for order in (range(n), np.random.default_rng(idx).permutation(n)):
        dW, db = _accumulate32(x, g, order)
        assert (np.abs(dW - want["dW"]) <= want["tol_W"]).all()
        assert (np.abs(db - want["db"]) <= want["tol_b"]).all()


def test_the_bound_catches_one_dropped_row():
    idx = next(i for i, c in enumerate(C.CASES) if (c["n"], c["in"], c["out"]) == (65, 48, 192))
    x, g = (O.widen(t).astype(np.float32) for t in C.operands(idx, "random"))
    want = C.expected(idx, "random")
    dW, db = _accumulate32(x, g, range(x.shape[0] - 1))
    assert (np.abs(dW - want["dW"]) > want["tol_W"]).mean() > 0.9 and (np.abs(db - want["db"]) > want["tol_b"]).mean() > 0.9


def _mlp(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(6, 10), nn.GELU(), nn.Linear(10, 3, bias=False))


def _grads(model, x):
    model.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    out = model(xx)
    out.square().sum().backward()
    return [out.detach(), xx.grad] + [p.grad.clone() for p in model.parameters()]


def test_the_hook_on_cpu_tensors_gives_torchs_own_bits(monkeypatch):
    monkeypatch.setattr(layers, "linear_grads_worth_it", lambda *a: True)  # (even when the rule admits the shape: a CPU tensor never enters)
    model, x = _mlp(), torch.randn(7, 6)
    before = _grads(model, x)
    assert sta.fuse_linear_grads(model) == ["0", "2"]
    out = model(x.clone().requires_grad_(True))
    assert type(out.grad_fn).__name__ != "LinearRowsBackward" and "LinearRows" not in type(out.grad_fn).__name__
    for a, b in zip(before, _grads(model, x)):
        assert torch.equal(a, b)


def test_bind_and_unbind_round_trip_and_foreign_forwards_are_left_alone():
    model = nn.Sequential(nn.Linear(4, 4), nn.Sequential(nn.Linear(4, 5), nn.ReLU()), nn.LayerNorm(5), nn.Linear(5, 2))
    foreign = lambda inp: inp.new_zeros(inp.shape[0], 5)
    model[1][0].__dict__["forward"] = foreign
    keys = list(model.state_dict())
    assert sta.fuse_linear_grads(model) == ["0", "3"]  # module order, the foreign one not named
    assert model[1][0].__dict__["forward"] is foreign
    assert all(m.__dict__["forward"].__func__ is layers.fused_linear_forward for m in (model[0], model[3]))
    assert sta.fuse_linear_grads(model) == ["0", "3"]  # binding again is the same binding
    assert list(model.state_dict()) == keys
    sta.unfuse_linear_grads(model)
    assert "forward" not in model[0].__dict__ and "forward" not in model[3].__dict__ and model[1][0].__dict__["forward"] is foreign
    del model[1][0].__dict__["forward"]
    assert sta.fuse_linear_grads(model) == ["0", "1.0", "3"]
    sta.unfuse_linear_grads(model)
    assert not any("forward" in m.__dict__ for m in model.modules())
    assert "fuse_linear_grads" in sta.__all__ and "unfuse_linear_grads" in sta.__all__
    assert sta.fuse_linear_grads is layers.fuse_linear_grads and sta.unfuse_linear_grads is layers.unfuse_linear_grads


def test_the_rule_is_a_pure_function_of_its_four_arguments(monkeypatch):
    assert list(inspect.signature(layers.linear_grads_worth_it).parameters) == ["n", "in_features", "out_features", "row_type"]
    args = [(n, i, o, t) for n in (0, 1, 1563, 6251, 25001, 100000, 400000) for i, o in ((48, 144), (48, 192), (192, 48), (384, 1536), (48, 13))
            for t in C.TYPE_PAIRS[0][:1] + (torch.float16, torch.bfloat16)]
    first = [layers.linear_grads_worth_it(*a) for a in args]
    assert all(isinstance(v, bool) for v in first)
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "24")
    torch.manual_seed(1)
    with torch.no_grad():
        assert [layers.linear_grads_worth_it(*a) for a in reversed(args)] == first[::-1]


def test_the_abi_table_names_the_three_entry_points_with_the_headers_arity():
    I, P = _lib.I, _lib.P
    assert _lib.RESULTS["pointops2_linear_grads_partial_rows"] == ([I, I, I], I)
    assert _lib.SIGNATURES["linear_grads_partial_launcher"] == [I] * 5 + [P] * 3 + [I]
    assert _lib.SIGNATURES["linear_grads_reduce_launcher"] == [I] * 3 + [P, I, P, P]
    assert abi_header.defines()["POINTOPS2_LINEAR_GRADS_ROWS"] == R
    rows = _lib.lib().pointops2_linear_grads_partial_rows  # (host arithmetic only: G is a function of n alone)
    assert [rows(n, 48, 192) for n in (0, 1, R, R + 1, 3 * R + 5)] == [1, 1, 1, 2, 4] == [rows(n, 1, 1536) for n in (0, 1, R, R + 1, 3 * R + 5)]
    assert rows(-1, 48, 192) == 0 and rows(5, 0, 192) == 0 and rows(5, 48, 1537) == 0


def test_the_operator_rejects_cpu_tensors_and_bad_operands():
    x, g = torch.zeros(4, 3), torch.zeros(4, 5)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pointops.linear_param_grads(x, g)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pointops.linear_rows(x, torch.zeros(5, 3), None)
    with pytest.raises(TypeError):
        pointops.linear_param_grads(None, g)
    assert pointops.LINEAR_GRADS_MAX_DIM == 1536
