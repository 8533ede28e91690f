"""GPU (-m gpu): the pair-list attention operators A1, A2, A4 and the fused window attention on every kernel path, head-group edge,
table length and row length of tests/attention_cases.py, against float64 references at the bounds derived there (no hand-picked
tolerance).  tests/test_attention_cases_cpu.py establishes, without a GPU, that the case table reaches every region of the
dispatch, that a correct fp32 implementation meets the bounds and that wrong ones miss them.  Every test id carries the path the
launchers take; every check prints `fraction <check> <case> <path> <largest fraction of its bound>`."""
import numpy as np
import pytest
import torch

from tests import attention_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()
    yield pointops
    pointops.clear_caches()


@pytest.fixture
def ops(P, monkeypatch, request):
    """the operator module as the case wants it: without a key-major view where the case says so (the backward then takes the
    by-query kernels with atomics), caches dropped afterwards"""
    spec = request.node.callspec.params["spec"]
    if not spec.csc:
        monkeypatch.setattr(P, "csc_of", lambda *a, **k: None)
    yield P
    if not spec.csc:
        P.clear_caches()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class _Tensors:
    """device copies of a case's arrays, made on first use"""

    def __init__(self, c):
        self._c, self._t = c, {}

    def __getattr__(self, name):
        if name not in self._t:
            self._t[name] = dev(getattr(self._c, name))
        return self._t[name]

    def leaf(self, name):
        return dev(getattr(self._c, name)).requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------------
# through the public operators
# ---------------------------------------------------------------------------------------------------------------------
def _a1(P, c, T):
    q, k = T.leaf("q"), T.leaf("k")
    out = P.attention_step1_v2(q, k, T.index_1, T.offsets, c.n_max)
    out.backward(T.go_pairs)
    return {"a1.out": _np(out), "a1.gq": _np(q.grad), "a1.gk": _np(k.grad)}


def _a2(P, c, T, backward=True):
    q, k, tq, tk = T.leaf("q"), T.leaf("k"), T.leaf("table_q"), T.leaf("table_k")
    out = P.dot_prod_with_idx_v3(q, T.offsets, c.n_max, k, T.index_1, tq, tk, T.rel_idx)
    if not backward:
        return {"a2.out": _np(out)}
    out.backward(T.go_pairs)
    return {"a2.out": _np(out), "a2.gq": _np(q.grad), "a2.gk": _np(k.grad), "a2.gtq": _np(tq.grad), "a2.gtk": _np(tk.grad)}


def _a4(P, c, T, backward=True):
    a, v, tv = T.leaf("attn"), T.leaf("v"), T.leaf("table_v")
    out = P.attention_step2_with_rel_pos_value_v2(a, v, T.offsets, c.n_max, T.index_1, tv, T.rel_idx)
    if not backward:
        return {"a4.out": _np(out)}
    out.backward(T.go_rows)
    return {"a4.out": _np(out), "a4.ga": _np(a.grad), "a4.gv": _np(v.grad), "a4.gt": _np(tv.grad)}


def _fused(P, c, T, backward=True):
    from stratified_transformer_amd import fused
    leaves = [T.leaf(n) for n in ("q", "k", "v", "table_q", "table_k", "table_v")]
    out = fused.window_attention(*leaves, T.offsets, T.index_1, T.rel_idx)
    got = {"f.out": _np(out), "f.attn": _np(out.grad_fn.saved_tensors[-1])}  # (the softmax the forward kept for its backward)
    if backward:
        out.backward(T.go_rows)
        got.update(zip(("f.gq", "f.gk", "f.gv", "f.gtq", "f.gtk", "f.gtv"), [_np(x.grad) for x in leaves]))
    return got


def _device_logits(P, c, T):
    """what the fused forward takes the softmax of, from the separate operators: A1 + A2, added in fp32 on the device"""
    with torch.no_grad():
        return _np(P.attention_step1_v2(T.q, T.k, T.index_1, T.offsets, c.n_max)
                   + P.dot_prod_with_idx_v3(T.q, T.offsets, c.n_max, T.k, T.index_1, T.table_q, T.table_k, T.rel_idx))


# ---------------------------------------------------------------------------------------------------------------------
# through the C ABI: the launches without a table length, and the launches that must be refused
# ---------------------------------------------------------------------------------------------------------------------
def _shapes(c):
    pairs, rows, table = (c.M, c.h), (c.N, c.h, c.d), (c.L, c.h, c.d, 3)
    return {"a2.out": pairs, "a2.gq": rows, "a2.gk": rows, "a2.gtq": table, "a2.gtk": table, "a4.out": rows, "a4.ga": pairs,
            "a4.gv": rows, "a4.gt": table, "attn": pairs}


STAGE_OUTPUTS = {"a2_fwd": ("a2.out",), "a2_bwd": ("a2.gq", "a2.gk", "a2.gtq", "a2.gtk"), "a4_fwd": ("a4.out",),
                 "a4_bwd": ("a4.ga", "a4.gv", "a4.gt"), "wlogit_fwd": ("attn",)}


def _alloc(c, stage, fill):
    return {n: torch.full(_shapes(c)[n], fill, dtype=torch.float32, device="cuda") for n in STAGE_OUTPUTS[stage]}


def _opts(P, c, T, stage):
    """the launch options the wrappers would pass: the table length where the case has one, the key-major view for a backward"""
    from stratified_transformer_amd import _lib
    s = c.spec
    csc = P.csc_of(T.offsets, T.index_1, c.N) if s.csc and stage.endswith("bwd") else None
    opts = P.pair_opts(T.offsets, T.index_1, csc=csc)
    return _lib.with_table_rows(opts, c.L) if s.table_rows else opts


def _launch(c, T, stage, o, opts):
    from stratified_transformer_amd import _lib
    p = _lib.ptr
    dims = (c.N, c.M, c.h, c.d)
    args = {
        "a2_fwd": ("dot_prod_with_idx_forward_cuda_launcher_v3", *dims, c.n_max, p(T.q), p(T.offsets), p(T.k), p(T.index_1), p(T.table_q),
                   p(T.table_k), p(T.rel_idx), *(p(o[n]) for n in STAGE_OUTPUTS[stage])),
        "a2_bwd": ("dot_prod_with_idx_backward_cuda_launcher_v3", *dims, c.n_max, p(T.go_pairs), p(T.q), p(T.offsets), p(T.k), p(T.index_1),
                   p(T.table_q), p(T.table_k), p(T.rel_idx), *(p(o[n]) for n in STAGE_OUTPUTS[stage])),
        "a4_fwd": ("attention_step2_with_rel_pos_value_forward_cuda_launcher_v2", *dims, c.n_max, p(T.attn), p(T.v), p(T.offsets), p(T.index_1),
                   p(T.table_v), p(T.rel_idx), *(p(o[n]) for n in STAGE_OUTPUTS[stage])),
        "a4_bwd": ("attention_step2_with_rel_pos_value_backward_cuda_launcher_v2", *dims, c.n_max, p(T.go_rows), p(T.offsets), p(T.index_1),
                   p(T.attn), p(T.v), p(T.table_v), p(T.rel_idx), *(p(o[n]) for n in STAGE_OUTPUTS[stage])),
        "wlogit_fwd": ("window_logits_softmax_forward_launcher", *dims, p(T.q), p(T.offsets), p(T.k), p(T.index_1), p(T.table_q), p(T.table_k),
                       p(T.rel_idx), *(p(o[n]) for n in STAGE_OUTPUTS[stage])),
    }[stage]
    _lib.call(*args, device=T.q.device, opts=opts)


def _refused(P, c, T, stage):
    """the launcher raises before any launch: every output keeps the value it was preset to"""
    o = _alloc(c, stage, 7.0)
    with pytest.raises(RuntimeError, match="does not fit in LDS"):
        _launch(c, T, stage, o, _opts(P, c, T, stage))
    torch.cuda.synchronize()
    for name, t in o.items():
        assert bool((t == 7.0).all()), f"{c.spec.name} {stage}: {name} was written to"
    s = c.spec
    print(f"fraction refused.{stage} {s.name} {C.path_id(C.path_of(stage, s.N, s.h, s.d, s.L, s.csc, s.table_rows))} 0.0000")


def _raw(P, c, T, group):
    """forward and backward of a2 / a4 with the reference's allocation pattern (zero-filled outputs), no table length"""
    got = {}
    for stage in C.OPS_OF[group]:
        o = _alloc(c, stage, 0.0)
        _launch(c, T, stage, o, _opts(P, c, T, stage))
        got.update({n: _np(t) for n, t in o.items()})
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
def _check(spec, group, got, paths, refs=None):
    c = C.case(spec)
    fwd_names = {"a1.out", "a2.out", "a4.out", "f.out", "f.attn"}
    for name in sorted(got):
        f = C.check(c, group, name, got[name], refs=refs)
        print(f"fraction {name} {spec.name} {C.path_id(paths[0] if name in fwd_names else paths[1])} {f:.4f}")


def _run_group(P, spec, group, run):
    """one operator group on one case: refused launches where path_of says so, otherwise every output against its bound, and
    the outputs that no float atomic touches bit for bit on a second call"""
    c, paths = C.case(spec), C.paths(spec, group)
    T = _Tensors(c)
    fwd, bwd = paths
    if fwd.family == "fallback-global":
        runs = [_raw(P, c, T, group) for _ in range(2)]
    elif fwd.family == "error":
        _refused(P, c, T, C.OPS_OF[group][0])
        if bwd.family == "error":
            _refused(P, c, T, C.OPS_OF[group][1])
        return
    elif bwd.family == "error":
        _refused(P, c, T, C.OPS_OF[group][1])
        runs = [run(P, c, T, backward=False) for _ in range(2)]
    else:
        runs = [run(P, c, T) for _ in range(2)]
    _check(spec, group, runs[0], paths)
    for name in C.repeatable(spec, group):
        if name in runs[0]:
            assert np.array_equal(_bits(runs[0][name]), _bits(runs[1][name])), f"{spec.name} {name}: a second call gives other bits"


@pytest.mark.parametrize("spec", C.specs_of("a1"), ids=C.spec_id("a1"))
def test_attention_step1_v2(ops, spec):
    c = C.case(spec)
    runs = [_a1(ops, c, _Tensors(c)) for _ in range(2)]
    _check(spec, "a1", runs[0], C.paths(spec, "a1"))
    for name in C.repeatable(spec, "a1"):
        assert np.array_equal(_bits(runs[0][name]), _bits(runs[1][name])), f"{spec.name} {name}: a second call gives other bits"


@pytest.mark.parametrize("spec", C.specs_of("a2"), ids=C.spec_id("a2"))
def test_dot_prod_with_idx_v3(ops, spec):
    _run_group(ops, spec, "a2", _a2)


@pytest.mark.parametrize("spec", C.specs_of("a4"), ids=C.spec_id("a4"))
def test_attention_step2_with_rel_pos_value_v2(ops, spec):
    _run_group(ops, spec, "a4", _a4)


@pytest.mark.parametrize("spec", C.specs_of("fused"), ids=C.spec_id("fused"))
def test_fused_window_attention(ops, spec):
    """attn against the float64 softmax of the device's own logits, everything behind it against float64 from the device's attn"""
    c, (fwd, bwd) = C.case(spec), C.paths(spec, "fused")
    T = _Tensors(c)
    if fwd.family == "error":
        _refused(ops, c, T, "wlogit_fwd")
        with pytest.raises(RuntimeError, match="does not fit in LDS"):
            _fused(ops, c, T, backward=False)
        return
    # without the fused backward the operators' own launchers run, and refuse what they refuse on their own
    chain_refuses = bwd.family == "operators" and "error" in (C.paths(spec, "a2")[1].family, C.paths(spec, "a4")[1].family)
    if chain_refuses:
        with pytest.raises(RuntimeError, match="does not fit in LDS"):
            _fused(ops, c, T)
    runs = [_fused(ops, c, T, backward=not chain_refuses) for _ in range(2)]
    _check(spec, "fused", runs[0], (fwd, bwd), C.fused_reference(c, _device_logits(ops, c, T), runs[0]["f.attn"]))
    for name in C.repeatable(spec, "fused"):
        if name in runs[0]:
            assert np.array_equal(_bits(runs[0][name]), _bits(runs[1][name])), f"{spec.name} {name}: a second call gives other bits"
