"""CPU: the declarations and refusals of optim_step_launcher (checked before anything is enqueued, so they need no GPU), the signature,
param_groups, refusals and state dicts of optim.SGD against the installed torch.optim.SGD, the `max_grad_norm` attribute, and the numpy
oracle (tests/optim_sgd_clip_oracle.py) against torch.optim.SGD and torch.nn.utils.clip_grad_norm_.  No HIP compute runs.

Bounds:
  * oracle float64 against torch.optim.SGD(foreach=False) on float64 CPU tensors, 20 steps, with and without clipping, and clipped AdamW:
    1e-12 relative to max(|p|, lr), the bound tests/test_optim_cpu.py derives for AdamW (SGD has fewer operations per step);
  * the oracle's float64 norm against clip_grad_norm_'s on float64 tensors: (n + 4) * 2^-53 relative, n the total element count - a sum of
    n exact squares in any order is within (n - 1) * 2^-53 of the true sum, both sides take one square root, torch one more per tensor;
  * oracle float32 against oracle float64 after 20 steps, per-tensor max-abs error: at most 2 x the error of torch in fp32 on the CPU
    against the same float64 oracle on the same inputs (tests/test_optim_cpu.py's rule).
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from stratified_transformer_amd import _lib, optim
from tests import optim_cases as C
from tests import optim_oracle as O
from tests import optim_sgd_clip_cases as K
from tests import optim_sgd_clip_oracle as S
from tests import abi_header
from tests.test_optim_cpu import _table

ADAMW, SGD = 0, 1


# ---- the C ABI ----
def test_the_general_launcher_is_declared_bound_and_exported():
    kinds = {k: abi_header.defines()[f"POINTOPS2_OPTIM_{k.upper()}"] for k in ("adamw", "sgd")}
    assert kinds == _lib.OPTIM_KINDS == dict(adamw=ADAMW, sgd=SGD)
    assert optim.AdamW._KIND == ADAMW and optim.SGD._KIND == SGD
    need, old = _lib.lib().pointops2_optim_step_workspace_bytes, _lib.lib().pointops2_optim_workspace_bytes
    assert need(300, 2, 1000) >= old(300, 2) + 8 * 1000 + 4 and need(1, 1, 0) >= old(1, 1) + 4
    assert need(-1, 1, 0) == 0 and need(1, 1, -1) == 0
    assert 1 << optim._CHUNK_SHIFT == abi_header.defines()["POINTOPS2_OPTIM_CHUNK"] == S.CHUNK


def _launch(kind, n_t, n_g, table, workspace_bytes=1 << 20, found_inf=64, max_norm=0.0, grad_norm=None):
    # the device pointers are never followed: every call below is refused before anything is enqueued
    l = _lib.lib()
    l.pointops2_last_error()
    l.optim_step_launcher(kind, n_t, n_g, table.ctypes.data_as(ctypes.c_void_p) if table is not None else None, 4096, workspace_bytes, None,
                          found_inf, 1, max_norm, grad_norm)
    err = l.pointops2_last_error()
    return None if err is None else err.decode()


@pytest.mark.parametrize("kind", [ADAMW, SGD])
def test_launcher_refusals(kind):
    group = [(1e-3, 0.9, 0.999, 1e-8, 0.01)]
    row = (64, 64, 64, 64, 64, 10, 0)
    assert "negative tensor count" in _launch(kind, -1, 1, _table([row], group))
    assert "negative group count" in _launch(kind, 1, -1, _table([row], group))
    assert "numel" in _launch(kind, 1, 1, _table([row[:5] + (2 ** 31, 0)], group))
    assert "numel" in _launch(kind, 1, 1, _table([row[:5] + (-1, 0)], group))
    assert "group index" in _launch(kind, 1, 1, _table([row[:6] + (1,)], group))
    assert "group index" in _launch(kind, 2, 1, _table([row, row[:6] + (0xffffffff,)], group))
    assert "group index" in _launch(kind, 1, 0, _table([row], []))
    assert "NULL" in _launch(kind, 1, 1, _table([(0,) + row[1:]], group))                        # param
    assert "NULL" in _launch(kind, 1, 1, _table([row[:1] + (0,) + row[2:]], group))              # grad
    assert "NULL" in _launch(kind, 1, 1, _table([row[:2] + (0,) + row[3:]], group))              # exp_avg: AdamW's, or SGD's buffer under a momentum
    assert "NULL" in _launch(kind, 1, 1, _table([row], group), found_inf=None)
    assert "NULL" in _launch(kind, 1, 1, None)
    assert "workspace" in _launch(kind, 1, 1, _table([row], group), workspace_bytes=8)
    assert _lib.lib().pointops2_last_error() is None                                             # reading clears
    # what the general entry point adds
    for bad in (2, -1, 7):
        assert "kind" in _launch(bad, 1, 1, _table([row], group))
    assert "NaN" in _launch(kind, 1, 1, _table([row], group), max_norm=float("nan"), grad_norm=64)
    assert "NaN" in _launch(kind, 1, 1, _table([row], group), max_norm=float("nan"))
    old = _lib.lib().pointops2_optim_workspace_bytes(2, 1)
    big = row[:5] + (3 * S.CHUNK + 1, 0)                                                         # 4 + 1 chunks: 40 bytes of partials and the factor
    assert _lib.lib().pointops2_optim_step_workspace_bytes(2, 1, 5) > old
    msg = _launch(kind, 2, 1, _table([big, row], group), workspace_bytes=old, max_norm=1.0, grad_norm=64)
    assert "workspace" in msg and "pointops2_optim_step_workspace_bytes" in msg
    assert "workspace" in _launch(kind, 2, 1, _table([big, row], group), workspace_bytes=_lib.lib().pointops2_optim_step_workspace_bytes(2, 1, 4),
                                  max_norm=1.0, grad_norm=64)


def test_the_old_launcher_keeps_its_messages():
    l = _lib.lib()
    l.pointops2_last_error()
    words = _table([(64, 64, 64, 64, 0, 10, 0)], [(1e-3, 0.9, 0.999, 1e-8, 0.01)])
    l.optim_adamw_step_launcher(1, 1, words.ctypes.data_as(ctypes.c_void_p), 4096, 1 << 20, None, 64, 1)
    assert l.pointops2_last_error().decode() == "optim_adamw_step: a tensor's param, grad, exp_avg, exp_avg_sq and step must not be NULL"
    l.optim_adamw_step_launcher(1, 1, words.ctypes.data_as(ctypes.c_void_p), 4096, 8, None, 64, 1)
    assert l.pointops2_last_error().decode() == "optim_adamw_step: workspace smaller than pointops2_optim_workspace_bytes(n_tensors, n_groups)"


# ---- the Python interface ----
def test_signatures():
    sig, ref = inspect.signature(optim.SGD), inspect.signature(torch.optim.SGD)
    assert list(sig.parameters) == list(ref.parameters)
    assert list(sig.parameters) == ["params", "lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "foreach", "differentiable",
                                    "fused"]
    for k in sig.parameters:
        assert sig.parameters[k].default == ref.parameters[k].default and sig.parameters[k].kind == ref.parameters[k].kind, k
    assert list(inspect.signature(optim.SGD.step).parameters) == ["self", "closure"]
    assert issubclass(optim.SGD, torch.optim.Optimizer) and optim.SGD._step_supports_amp_scaling is True
    assert "SGD" in optim.__all__ and "AdamW" in optim.__all__
    # AdamW is what it was
    assert list(inspect.signature(optim.AdamW).parameters) == ["params", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "capturable",
                                                               "differentiable"]
    assert optim.AdamW._step_supports_amp_scaling is True and type(optim.AdamW).__name__ == "type"
    assert optim.AdamW.__mro__[1] is optim.SGD.__mro__[1] and issubclass(optim.AdamW.__mro__[1], torch.optim.Optimizer)   # the shared base


def test_param_groups_carry_torchs_keys():
    p = [torch.zeros(3, requires_grad=True), torch.zeros(2, requires_grad=True)]
    kw = dict(lr=6e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)
    ours = optim.SGD([dict(params=[p[0]]), dict(params=[p[1]], lr=6e-4)], **kw)
    theirs = torch.optim.SGD([dict(params=[p[0]]), dict(params=[p[1]], lr=6e-4)], **kw)
    assert [set(g) for g in ours.param_groups] == [set(g) for g in theirs.param_groups]
    for a, b in zip(ours.param_groups, theirs.param_groups):
        assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in b.items() if k != "params"}
    sched = torch.optim.lr_scheduler.LambdaLR(ours, [lambda e: 0.5, lambda e: 0.25])
    assert [g["lr"] for g in ours.param_groups] == [3e-3, 1.5e-4] and sched.get_last_lr() == [3e-3, 1.5e-4]
    for opt in (ours, optim.AdamW(p)):
        assert opt.max_grad_norm is None and opt.last_grad_norm is None
        opt.max_grad_norm = 2.0
        assert all("max_grad_norm" not in g and "last_grad_norm" not in g for g in opt.param_groups)
        assert set(opt.state_dict()) == {"state", "param_groups"} and "max_grad_norm" not in str(opt.state_dict())
        opt.__setstate__(dict(defaults=opt.defaults, state=opt.state, param_groups=opt.param_groups))
        assert opt.max_grad_norm == 2.0                                                        # kept where it is set ...
        del opt.__dict__["max_grad_norm"], opt.__dict__["last_grad_norm"]
        opt.__setstate__(dict(defaults=opt.defaults, state=opt.state, param_groups=opt.param_groups))
        assert opt.max_grad_norm is None and opt.last_grad_norm is None                        # ... and defaulted where it is not


@pytest.mark.parametrize("kw, name", [(dict(dampening=0.1, momentum=0.9), "dampening"), (dict(maximize=True), "maximize"),
                                      (dict(differentiable=True), "differentiable"), (dict(nesterov=True), "nesterov"),
                                      (dict(nesterov=True, momentum=0.0), "nesterov"), (dict(lr=torch.tensor(1e-3)), "lr"),
                                      (dict(lr=-1.0), "lr"), (dict(momentum=-0.5), "momentum"), (dict(weight_decay=-1.0), "weight_decay")])
def test_unsupported_arguments_raise_at_construction(kw, name):
    with pytest.raises(ValueError, match=name):
        optim.SGD([torch.zeros(3, requires_grad=True)], **kw)


def test_step_refusals_name_the_argument():
    def stepped(p, g, make=optim.SGD):
        p.grad = g
        make([p]).step()
    with pytest.raises(RuntimeError, match="SGD: params.*GPU"):
        stepped(torch.zeros(4, requires_grad=True), torch.zeros(4))
    with pytest.raises(TypeError, match="SGD: params.*float32"):
        stepped(torch.zeros(4, dtype=torch.float64, requires_grad=True), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="SGD: params.*contiguous"):
        stepped(torch.zeros(4, 4).t().requires_grad_(True), torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="SGD: grad.*sparse"):
        stepped(torch.zeros(4, 4, requires_grad=True), torch.zeros(4, 4).to_sparse())
    # a state dict that asks for what the kernel does not do is refused at the first step
    for kw, name in ((dict(dampening=0.5, momentum=0.9), "dampening"), (dict(maximize=True), "maximize"), (dict(differentiable=True), "differentiable")):
        p = torch.zeros(4, requires_grad=True)
        ours = optim.SGD([p], momentum=0.9)
        ours.load_state_dict(torch.optim.SGD([p], **kw).state_dict())
        p.grad = torch.zeros(4)
        with pytest.raises(ValueError, match=rf"param_groups\[0\].*{name}"):
            ours.step()
    p = torch.zeros(4, requires_grad=True)
    p.grad = torch.zeros(4)
    ours = optim.SGD([p], momentum=0.9, nesterov=True)
    ours.param_groups[0]["momentum"] = 0.0
    with pytest.raises(ValueError, match="nesterov"):
        ours.step()
    ours = optim.SGD([p])
    ours.param_groups[0]["lr"] = torch.tensor(1e-3)
    with pytest.raises(ValueError, match="lr"):
        ours.step()
    # nothing to do is no error, on any device
    opt = optim.SGD([torch.zeros(4, requires_grad=True), torch.zeros(4)], momentum=0.9)
    assert opt.step() is None and len(opt.state) == 0 and opt.step(lambda: 3.0) == 3.0 and opt.last_grad_norm is None


@pytest.mark.parametrize("make", [optim.SGD, optim.AdamW])
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan"), "1.0", True, torch.tensor(1.0), [1.0]])
def test_max_grad_norm_is_checked_at_step(make, bad):
    opt = make([torch.zeros(4, requires_grad=True)])
    opt.max_grad_norm = bad
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step()
    for good in (None, 1, 0.5, 1e30):
        opt.max_grad_norm = good
        assert opt.step() is None                                                              # no gradient: nothing runs


# ---- state dicts ----
def test_state_dicts_travel_both_ways():
    params, grads = C.params_and_grads([6, 4, 3, 2], 3, seed=2)
    groups = K.SGD_CONFIGS["momentum"]
    ps = [torch.tensor(a).requires_grad_(True) for a in params]
    theirs = torch.optim.SGD(K.param_groups(ps, groups), foreach=False)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g)
        theirs.step()
    sd = theirs.state_dict()
    ours = optim.SGD(K.param_groups([torch.tensor(a).requires_grad_(True) for a in params], groups))
    ours.load_state_dict(sd)
    back = ours.state_dict()
    assert back["param_groups"] == sd["param_groups"] and set(back["state"]) == set(sd["state"]) == {0, 1, 2, 3}
    for k, st in sd["state"].items():
        assert set(back["state"][k]) == set(st) == {"momentum_buffer"}
        assert torch.equal(back["state"][k]["momentum_buffer"], st["momentum_buffer"]) and back["state"][k]["momentum_buffer"].dtype == torch.float32
    again = optim.SGD(K.param_groups([torch.tensor(a).requires_grad_(True) for a in params], groups))
    again.load_state_dict(back)
    assert again.state_dict()["param_groups"] == back["param_groups"]
    theirs.load_state_dict(back)                                                               # ours into torch's
    for p, g in zip(ps, grads[0]):
        p.grad = torch.tensor(g)
    theirs.step()
    # without a momentum torch writes a buffer of None: it loads and counts as absent; our empty state loads into torch's
    plain = torch.optim.SGD(K.param_groups(ps, K.SGD_CONFIGS["plain"]), foreach=False)
    plain.step()
    sd0 = plain.state_dict()
    assert all(st.get("momentum_buffer") is None for st in sd0["state"].values())
    ours0 = optim.SGD(K.param_groups([torch.tensor(a).requires_grad_(True) for a in params], K.SGD_CONFIGS["plain"]))
    ours0.load_state_dict(sd0)
    assert all(st.get("momentum_buffer") is None for st in ours0.state.values())
    fresh = optim.SGD(K.param_groups([torch.tensor(a).requires_grad_(True) for a in params], K.SGD_CONFIGS["plain"]))
    assert fresh.state_dict()["state"] == {}
    plain.load_state_dict(fresh.state_dict())
    plain.step()


# ---- the oracle ----
@pytest.fixture(scope="module")
def sequence():
    return C.params_and_grads(C.SEQUENCE_SIZES, C.SEQUENCE_STEPS, seed=7)


CASES = [("sgd", "momentum", None), ("sgd", "nesterov", None), ("sgd", "plain", None), ("sgd", "momentum", K.MAX_NORM), ("adamw", None, K.MAX_NORM)]
_runs = {}


def _o64(case, sequence):
    """the float64 oracle's run of a case, computed once"""
    if case not in _runs:
        kind, config, max_norm = case
        _runs[case] = K.oracle_run(kind, K.groups_of(kind, config), *sequence, np.float64, max_norm=max_norm)
    return _runs[case]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_oracle_f64_against_torch(case, sequence):
    kind, config, max_norm = case
    params, grads = sequence
    groups = K.groups_of(kind, config)
    o64, coefs = _o64(case, sequence)
    want, norms = K.torch_run(kind, groups, params, grads, torch.float64, max_norm=max_norm)
    for i, (a, b) in enumerate(zip(o64.p, want)):
        lr = groups[C.group_of(len(params))[i]]["lr"]
        rel = np.max(np.abs(a - b) / np.maximum(np.abs(b), lr))
        print("tensor", i, "max deviation relative to max(|p|, lr):", rel)
        assert a.dtype == np.float64 and rel <= 1e-12
    assert o64.t == [C.SEQUENCE_STEPS] * len(params)
    assert np.max(np.abs(o64.p[0] - params[0])) > (1e-2 if max_norm is None else 1e-4)          # the parameters did move
    if max_norm is not None:
        assert len(coefs) == C.SEQUENCE_STEPS and all(c.dtype == np.float64 and 0 < c < 1 for c in coefs)
        print("clip factors", min(coefs), "...", max(coefs))


def test_norm_against_clip_grad_norm(sequence):
    params, grads = sequence
    n = sum(a.size for a in params)
    _, norms = K.torch_run("sgd", K.SGD_CONFIGS["momentum"], params, grads, torch.float64, max_norm=K.MAX_NORM)
    for gs, want in zip(grads, norms):
        got, coef = S.clip_coef(S.grad_sq_sum(gs, None, np.float64), K.MAX_NORM, np.float64)
        rel = abs(float(got) - want) / want
        print("norm", float(got), "torch", want, "relative difference", rel, "bound", (n + 4) * 2.0 ** -53)
        assert rel <= (n + 4) * 2.0 ** -53 and coef < 1
        assert coef == K.MAX_NORM / (float(got) + 1e-6)
    # the reduction is the one written down: against a plain loop over one small case with three chunks and a tail
    g = grads[0][1][:4097].astype(np.float32)
    x = g.astype(np.float64) ** 2
    partial = []
    for c0 in range(0, x.size, S.CHUNK):
        chunk = x[c0:c0 + S.CHUNK]
        a = [0.0] * S.THREADS
        for i in range(chunk.size):                                                            # ascending i: a thread meets its elements in order
            a[(i // 4) % S.THREADS] += chunk[i]
        stride = S.THREADS // 2
        while stride:
            for j in range(stride):
                a[j] = a[j] + a[j + stride]
            stride //= 2
        partial.append(a[0])
    assert np.array_equal(S.chunk_partials(g), np.array(partial))
    assert S.grad_sq_sum([g, None, g[:5]]) == (partial[0] + S.chunk_partials(g[:5])[0]) + partial[1]   # thread 0: chunks 0..; thread 1; tree


@pytest.mark.parametrize("case", CASES, ids=str)
def test_oracle_f32_against_oracle_f64(case, sequence):
    kind, config, max_norm = case
    params, grads = sequence
    groups = K.groups_of(kind, config)
    o64, _ = _o64(case, sequence)
    o32, coefs = K.oracle_run(kind, groups, params, grads, np.float32, max_norm=max_norm)
    assert all(a.dtype == np.float32 for a in o32.p + o32.m + o32.v)
    assert max_norm is None or all(c.dtype == np.float32 and 0 < c < 1 for c in coefs)
    ours = C.max_abs_errors(o32.p, o64.p)
    torchs = C.max_abs_errors(K.torch_run(kind, groups, params, grads, torch.float32, max_norm=max_norm)[0], o64.p)
    for i, (a, b) in enumerate(zip(ours, torchs)):
        print("tensor", i, "oracle f32 error", a, "torch f32 error", b, "ratio", a / b if b else float("nan"))
        assert a <= 2 * b


# ---- properties of the oracle ----
@pytest.mark.parametrize("kind, config", [("sgd", "momentum"), ("sgd", "nesterov"), ("adamw", None)])
def test_scales_clips_and_skips_in_the_oracle(kind, config):
    params, grads = C.params_and_grads([5, 4100, 3], 3, seed=1)
    groups, gof = K.groups_of(kind, config), C.group_of(3)

    def run(scale=None, max_norm=None, factor=1.0):
        st = S.State(kind, params, groups, gof, max_norm=max_norm)
        for gs in grads:
            st.step([g * np.float32(factor) for g in gs], scale)
        return st

    def same(a, b):
        return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a.p + a.m + a.v, b.p + b.m + b.v))

    plain = run()
    assert same(run(scale=65536.0, factor=65536.0), plain)                                     # a power of two: the same bits
    assert not same(run(scale=3000.0, factor=3000.0), plain)
    clipped = run(max_norm=1.0)
    assert clipped.coef < 1 and clipped.coef.dtype == np.float32 and clipped.norm.dtype == np.float32 and not same(clipped, plain)
    assert same(run(scale=65536.0, factor=65536.0, max_norm=1.0), clipped)
    loose = run(max_norm=1e6)
    assert loose.coef == np.float32(1.0) and abs(float(loose.norm) - 64.0) < 8 and same(loose, plain)
    # a non-finite gradient: the step is skipped, nothing moves, the next step goes on from there
    st = S.State(kind, params, groups, gof, max_norm=1.0)
    st.step(grads[0])
    before = [a.copy() for a in st.p + st.m + st.v]
    for value in (np.inf, np.nan):
        bad = [g.copy() for g in grads[1]]
        bad[1][4099] = value
        assert st.step(bad) is True and st.t == [1, 1, 1]
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, st.p + st.m + st.v))
    assert st.step([grads[1][0], None, grads[1][2]]) is False and st.t == [2, 1, 2] and np.array_equal(st.p[1], before[1])
    assert st.norm == S.clip_coef(S.grad_sq_sum([grads[1][0], grads[1][2]]), 1.0)[0]            # a tensor without a gradient is left out
