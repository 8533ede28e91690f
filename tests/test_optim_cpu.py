"""CPU: the declarations of csrc/optim.hip's launcher, its refusals (checked before anything is enqueued, so they need no GPU), the
signatures and refusals of optim.AdamW / optim.GradScaler, the numpy oracle (tests/optim_oracle.py) against torch.optim.AdamW, and a state
dict written by torch.optim.AdamW loaded into optim.AdamW.  No HIP compute runs.

Bounds:
  * oracle float64 against torch.optim.AdamW(foreach=False) on float64 CPU tensors, 20 steps: 1e-12 relative to max(|p|, lr) - four orders
    above eps x operations x steps (2.2e-16 x 12 x 20 = 5e-14 of |p|), far below a wrong bias correction or a coupled decay (1e-3 and more);
  * oracle float32 against oracle float64 after those 20 steps, per-tensor max-abs error: at most 2 x the error of torch.optim.AdamW
    (foreach=False) in fp32 on the CPU against the same float64 oracle, measured here on the same inputs.  Both are chains of the same
    dozen correctly rounded fp32 operations per element and step in a different order; 2 x leaves room for the order.
"""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from stratified_transformer_amd import _lib, optim
from tests import optim_cases as C
from tests import optim_oracle as O

# ---- the C ABI (declarations, struct layouts and POINTOPS2_OPTIM_CHUNK against their mirrors: tests/test_abi_cpu.py) ----
def test_launcher_is_declared_bound_and_exported():
    assert "optim.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()


def _table(rows, groups):
    """host table of rows (param, grad, exp_avg, exp_avg_sq, step, numel, group) and groups (5 doubles) -> int64 array"""
    words = np.zeros(7 * len(rows) + 5 * len(groups), np.int64)
    if rows:
        words[:7 * len(rows)].reshape(-1, 7)[:] = rows
    if groups:
        words[7 * len(rows):].view(np.float64).reshape(-1, 5)[:] = groups
    return words


def _launch(n_t, n_g, table, workspace_bytes=1 << 20, found_inf=64):
    # the pointers are never followed: every call below is refused before anything is enqueued
    l = _lib.lib()
    l.pointops2_last_error()
    l.optim_adamw_step_launcher(n_t, n_g, table.ctypes.data_as(ctypes.c_void_p) if table is not None else None, 4096, workspace_bytes, None,
                                found_inf, 1)
    err = l.pointops2_last_error()
    return None if err is None else err.decode()


def test_launcher_refusals():
    group = [(1e-3, 0.9, 0.999, 1e-8, 0.01)]
    row = (64, 64, 64, 64, 64, 10, 0)
    assert "negative tensor count" in _launch(-1, 1, _table([row], group))
    assert "negative group count" in _launch(1, -1, _table([row], group))
    assert "numel" in _launch(1, 1, _table([row[:5] + (2 ** 31, 0)], group))
    assert "numel" in _launch(1, 1, _table([row[:5] + (-1, 0)], group))
    assert "group index" in _launch(1, 1, _table([row[:6] + (1,)], group))
    assert "group index" in _launch(2, 1, _table([row, row[:6] + (0xffffffff,)], group))          # group = -1
    assert "group index" in _launch(1, 0, _table([row], []))
    assert "NULL" in _launch(1, 1, _table([(0,) + row[1:]], group))
    assert "NULL" in _launch(1, 1, _table([row], group), found_inf=None)
    assert "NULL" in _launch(1, 1, None)
    assert "workspace" in _launch(1, 1, _table([row], group), workspace_bytes=8)
    assert _lib.lib().pointops2_last_error() is None                                             # reading clears
    need = _lib.lib().pointops2_optim_workspace_bytes
    assert need(1, 1) >= 56 + 40 + 36 and need(300, 2) >= 300 * (56 + 36) + 80 and need(-1, 1) == 0


# ---- the Python interface ----
def test_signatures():
    sig = inspect.signature(optim.AdamW)
    assert list(sig.parameters) == ["params", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "capturable", "differentiable"]
    assert [sig.parameters[k].default for k in ("lr", "betas", "eps", "weight_decay")] == [1e-3, (0.9, 0.999), 1e-8, 1e-2]
    ref = inspect.signature(torch.optim.AdamW)
    assert all(sig.parameters[k].default == ref.parameters[k].default and sig.parameters[k].kind == ref.parameters[k].kind
               for k in sig.parameters)
    assert list(inspect.signature(optim.AdamW.step).parameters) == ["self", "closure"]
    assert list(inspect.signature(optim.GradScaler.step).parameters) == list(inspect.signature(torch.amp.GradScaler.step).parameters)
    assert inspect.signature(optim.GradScaler) == inspect.signature(torch.amp.GradScaler)
    assert optim.GradScaler.update is torch.amp.GradScaler.update and optim.GradScaler.state_dict is torch.amp.GradScaler.state_dict
    assert issubclass(optim.AdamW, torch.optim.Optimizer) and optim.AdamW._step_supports_amp_scaling is True
    import stratified_transformer_amd as sta
    assert sta.optim is optim


def test_param_groups_carry_torchs_keys():
    p = [torch.zeros(3, requires_grad=True), torch.zeros(2, requires_grad=True)]
    ours = optim.AdamW([dict(params=[p[0]]), dict(params=[p[1]], lr=6e-4)], lr=6e-3, weight_decay=0.02)
    theirs = torch.optim.AdamW([dict(params=[p[0]]), dict(params=[p[1]], lr=6e-4)], lr=6e-3, weight_decay=0.02)
    assert [set(g) for g in ours.param_groups] == [set(g) for g in theirs.param_groups]
    for a, b in zip(ours.param_groups, theirs.param_groups):
        assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in b.items() if k != "params"}
    sched = torch.optim.lr_scheduler.LambdaLR(ours, [lambda e: 0.5, lambda e: 0.25])   # util/lr.py's schedulers are LambdaLR on group['lr']
    assert [g["lr"] for g in ours.param_groups] == [3e-3, 1.5e-4] and sched.get_last_lr() == [3e-3, 1.5e-4]


@pytest.mark.parametrize("name", ["amsgrad", "maximize", "capturable", "differentiable"])
def test_unsupported_flags_raise_at_construction(name):
    with pytest.raises(ValueError, match=name):
        optim.AdamW([torch.zeros(3, requires_grad=True)], **{name: True})


def test_step_refusals_name_the_argument():
    def stepped(p, g):
        p.grad = g
        optim.AdamW([p]).step()
    with pytest.raises(RuntimeError, match="params.*GPU"):
        stepped(torch.zeros(4, requires_grad=True), torch.zeros(4))
    with pytest.raises(TypeError, match="params.*float32"):
        stepped(torch.zeros(4, dtype=torch.float64, requires_grad=True), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError, match="params.*float32"):
        stepped(torch.zeros(4, dtype=torch.float16, requires_grad=True), torch.zeros(4, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="params.*contiguous"):
        stepped(torch.zeros(4, 4).t().requires_grad_(True), torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="grad.*sparse"):
        stepped(torch.zeros(4, 4, requires_grad=True), torch.zeros(4, 4).to_sparse())
    # a state dict that asks for what the kernel does not do is refused at the first step
    p = torch.zeros(4, requires_grad=True)
    theirs = torch.optim.AdamW([p], amsgrad=True)
    ours = optim.AdamW([p])
    ours.load_state_dict(theirs.state_dict())
    p.grad = torch.zeros(4)
    with pytest.raises(ValueError, match="amsgrad"):
        ours.step()
    # nothing to do is no error, on any device
    none = torch.zeros(4, requires_grad=True)
    frozen = torch.zeros(4)
    opt = optim.AdamW([none, frozen])
    assert opt.step() is None and len(opt.state) == 0 and opt.step(lambda: 3.0) == 3.0


# ---- the oracle ----
def test_power_by_squaring():
    for beta in (0.9, 0.999):
        for n in (0, 1, 2, 3, 7, 20, 1000, 123457):
            got = O.pow_by_squaring(beta, n)
            # a product of n factors by any bracketing: at most n - 1 roundings of 2^-53 each (1 + second order); pow() itself is within an ulp
            assert isinstance(got, np.float64) and abs(got - beta ** n) <= (1.01 * n + 2) * 2.0 ** -53 * beta ** n
    assert O.pow_by_squaring(0.9, 5) == 0.9 * ((0.9 * 0.9) * (0.9 * 0.9))                  # 5 = 0b101: b, then b^4 from two squarings
    assert O.inv_scale_of(None) == 1 and O.inv_scale_of(65536.0) == np.float32(2.0 ** -16)
    assert O.inv_scale_of(3000.0) == np.float32(1.0 / 3000.0) and O.inv_scale_of(3000.0).dtype == np.float32
    assert float(O.inv_scale_of(3000.0)) != 1.0 / 3000.0 and float(O.inv_scale_of(65536.0)) == 1.0 / 65536.0   # one is rounded, one is not


@pytest.fixture(scope="module")
def sequence():
    params, grads = C.params_and_grads(C.SEQUENCE_SIZES, C.SEQUENCE_STEPS, seed=7)
    return params, grads, C.oracle_run(params, grads, np.float64)


def test_oracle_f64_against_torch(sequence):
    params, grads, o64 = sequence
    want = C.torch_run(params, grads, torch.float64)
    for i, (a, b) in enumerate(zip(o64.p, want)):
        lr = C.GROUPS[C.group_of(len(params))[i]]["lr"]
        rel = np.max(np.abs(a - b) / np.maximum(np.abs(b), lr))
        print("tensor", i, "max deviation relative to max(|p|, lr):", rel)
        assert a.dtype == np.float64 and rel <= 1e-12
    assert o64.t == [C.SEQUENCE_STEPS] * len(params)
    # the yardstick can tell: a coupled decay or a missing bias correction is orders away
    assert np.max(np.abs(o64.p[0] - params[0])) > 1e-2


def test_oracle_f32_against_oracle_f64(sequence):
    params, grads, o64 = sequence
    o32 = C.oracle_run(params, grads, np.float32)
    assert all(a.dtype == np.float32 for a in o32.p + o32.m + o32.v)
    ours = C.max_abs_errors(o32.p, o64.p)
    torchs = C.max_abs_errors(C.torch_run(params, grads, torch.float32), o64.p)
    for i, (a, b) in enumerate(zip(ours, torchs)):
        print("tensor", i, "oracle f32 error", a, "torch f32 error", b, "ratio", a / b)
        assert b > 0 and a <= 2 * b


def test_skips_and_scales_in_the_oracle():
    params, grads = C.params_and_grads([5, 3], 2, seed=1)
    st = O.State(params, C.GROUPS, [0, 1])
    bad = [grads[0][0].copy(), grads[0][1]]
    bad[0][2] = np.inf
    assert st.step(bad) is True and st.t == [0, 0] and all(np.array_equal(a, b) for a, b in zip(st.p, params))
    assert st.step([grads[0][0], None]) is False and st.t == [1, 0] and np.array_equal(st.p[1], params[1])
    scaled = O.State(params, C.GROUPS, [0, 1])
    scaled.step([g * np.float32(65536) for g in grads[0]], scale=65536.0)                       # a power of two: the same bits
    plain = O.State(params, C.GROUPS, [0, 1])
    plain.step(grads[0])
    assert all(np.array_equal(a, b) for a, b in zip(scaled.p + scaled.m + scaled.v, plain.p + plain.m + plain.v))


# ---- state dicts ----
def test_a_torch_state_dict_loads_and_comes_back():
    params, grads = C.params_and_grads([6, 4, 3, 2], 3, seed=2)
    ps = [torch.tensor(a).requires_grad_(True) for a in params]
    theirs = torch.optim.AdamW(C.torch_groups(ps), foreach=False)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g)
        theirs.step()
    sd = theirs.state_dict()
    ours = optim.AdamW(C.torch_groups([torch.tensor(a).requires_grad_(True) for a in params]))
    ours.load_state_dict(sd)
    back = ours.state_dict()
    assert back["param_groups"] == sd["param_groups"] and set(back["state"]) == set(sd["state"]) == {0, 1, 2, 3}
    for k, st in sd["state"].items():
        assert set(back["state"][k]) == set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(back["state"][k]["step"]) == float(st["step"]) == 3.0
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][k][name], st[name]) and back["state"][k][name].dtype == torch.float32
    # and our own round-trips, into torch as well
    again = optim.AdamW(C.torch_groups([torch.tensor(a).requires_grad_(True) for a in params]))
    again.load_state_dict(back)
    assert again.state_dict()["param_groups"] == back["param_groups"]
    theirs.load_state_dict(back)
