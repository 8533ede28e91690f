"""CPU: the declarations of pointops.batch_norm_act (C ABI table, signatures, re-exports, argument checks, the missing CPU path), its float64
oracle (tests/batchnorm_oracle.py) against torch's float64 autograd, and layers.fuse_batch_norms on CPU tensors, where every site must run
its own modules and give torch's bits.  No HIP compute runs here."""
import copy
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, layers, pointops, pointops2_cuda
from tests import batchnorm_oracle as O
from tests import stem_standin as S
from tests.test_rownorm_cpu import _OnGpu, _g


def test_launchers_are_declared_and_exported():
    I, P, Fl = _lib.I, _lib.P, _lib.F
    assert _lib.SIGNATURES["batch_norm_act_stats_launcher"] == [I] * 3 + [P] * 2 + [I] + [Fl] * 2 + [P] * 3
    assert _lib.SIGNATURES["batch_norm_act_forward_launcher"] == [I] * 5 + [Fl] + [P] * 3 + [I] + [Fl] + [P] * 5
    assert _lib.SIGNATURES["batch_norm_act_backward_launcher"] == [I] * 4 + [Fl] + [I] + [P] * 6 + [I] + [P] * 3
    assert _lib.ACTIVATIONS == {"none": 0, "relu": 1, "leaky_relu": 2, "tanh": 3}


def test_public_signatures():
    assert str(inspect.signature(pointops.batch_norm_act)) == (
        "(x, weight, bias, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-05, act='none', negative_slope=0.01, "
        "residual=None)")
    assert str(inspect.signature(layers.fuse_batch_norms)) == "(model)" and str(inspect.signature(layers.unfuse_batch_norms)) == "(model)"
    assert sta.fuse_batch_norms is layers.fuse_batch_norms and sta.unfuse_batch_norms is layers.unfuse_batch_norms
    assert "fuse_batch_norms" in sta.__all__ and "unfuse_batch_norms" in sta.__all__
    assert str(inspect.signature(sta.install)) == "(third_party=True, fast_layers=False, pooled_transition=False)"
    assert issubclass(pointops.BatchNormAct, torch.autograd.Function)
    from lib.pointops2.functions import pointops as drop_in
    assert drop_in.batch_norm_act is pointops.batch_norm_act and drop_in.BatchNormAct is pointops.BatchNormAct


def test_cpu_tensors_raise_no_cpu_fallback():
    x, w, b, rm, rv = torch.rand(6, 8), torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops.batch_norm_act(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops.batch_norm_act(x, w, b, rm, rv, training=False, act="tanh", residual=torch.rand(6, 8))
    o, stat = torch.empty(6, 8), torch.empty(2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.batch_norm_act_stats(6, 8, x, torch.empty(2, 3, 8), 1e-5, 0.1, rm, rv, stat)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.batch_norm_act_forward(6, 8, x, stat[0], stat[1], False, 1e-5, w, b, "relu", 0.0, None, o, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.batch_norm_act_backward(6, 8, x, o, stat, w, b, "relu", 0.0, True, torch.empty(2, 2, 8), torch.empty(8), torch.empty(8),
                                               torch.empty(6, 8))


def _case(**change):
    kw = dict(x=torch.rand(6, 8), weight=torch.ones(8), bias=torch.zeros(8), running_mean=torch.zeros(8), running_var=torch.ones(8),
              residual=torch.rand(6, 8), act="relu", momentum=0.1)
    kw.update(change)
    return kw


@pytest.mark.parametrize("change,error,names", [
    (dict(x=torch.rand(6, 1025), weight=torch.ones(1025), bias=torch.zeros(1025), running_mean=None, running_var=None, residual=None), ValueError, "c must be"),
    (dict(x=torch.rand(6, 8).double()), TypeError, "x must be f32, f16 or bf16"),
    (dict(x=torch.rand(48)), ValueError, "x must be"),
    (dict(x=torch.rand(2, 6, 8)), ValueError, "x must be"),
    (dict(x=torch.rand(8, 6).t()), ValueError, "x must be contiguous"),
    (dict(weight=None), ValueError, "weight is None"),
    (dict(bias=None), ValueError, "bias is None"),
    (dict(weight=torch.ones(7)), ValueError, "weight must be"),
    (dict(bias=torch.zeros(9)), ValueError, "bias must be"),
    (dict(weight=torch.ones(8).half()), TypeError, "weight must be"),
    (dict(weight=torch.ones(16)[::2]), ValueError, "weight must be contiguous"),
    (dict(running_mean=None), ValueError, "running_mean"),
    (dict(running_var=None), ValueError, "running_var"),
    (dict(running_mean=torch.zeros(9)), ValueError, "running_mean must be"),
    (dict(running_var=torch.ones(8).double()), TypeError, "running_var must be"),
    (dict(residual=torch.rand(5, 8)), ValueError, "residual must be"),
    (dict(residual=torch.rand(6, 8).double()), TypeError, "residual must be"),
    (dict(residual=torch.rand(6, 16)[:, ::2]), ValueError, "residual must be contiguous"),
    (dict(act="gelu"), ValueError, "act must be"),
    (dict(momentum=None), ValueError, "momentum"),
])
def test_operator_rejects_bad_arguments(change, error, names):
    kw = _case(**change)
    with pytest.raises(error, match="batch_norm_act: .*" + names):
        pointops.batch_norm_act(_g(kw["x"]), _g(kw["weight"]), _g(kw["bias"]), _g(kw["running_mean"]), _g(kw["running_var"]), True, kw["momentum"],
                                1e-5, kw["act"], 0.01, _g(kw["residual"]))


def test_one_row_in_training_raises_as_torch_does():
    x, w, b = torch.rand(1, 8), torch.ones(8), torch.zeros(8)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training") as ours:
        pointops.batch_norm_act(_g(x), _g(w), _g(b))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training") as theirs:
        F.batch_norm(x, None, None, w, b, True)
    assert str(ours.value) == str(theirs.value)


def test_binding_rejects_bad_shapes_and_dtypes():
    C = pointops2_cuda
    f32 = lambda *s: _OnGpu(torch.zeros(*s))
    f16 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.float16))
    f64 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.float64))
    ok = lambda: dict(n=6, c=8, x=f16(6, 8), partials=f32(2, 3, 8), eps=1e-5, momentum=0.1, running_mean=f32(8), running_var=f32(8), stat=f32(2, 8))
    cases = [("c", ValueError, dict(c=1025)), ("c", ValueError, dict(c=0)), ("n", ValueError, dict(n=-1)), ("x", TypeError, dict(x=f64(6, 8))),
             ("x", ValueError, dict(x=f16(5, 8))), ("x", RuntimeError, dict(x=_OnGpu(torch.zeros(8, 6).t()))), ("partials", ValueError, dict(partials=f32(2, 2, 8))),
             ("partials", ValueError, dict(partials=f32(1025, 3, 8))), ("partials", TypeError, dict(partials=f16(2, 3, 8))),
             ("running_var", ValueError, dict(running_var=None)), ("running_mean", ValueError, dict(running_mean=f32(7))),
             ("stat", ValueError, dict(stat=f32(8, 2))), ("stat", TypeError, dict(stat=f16(2, 8)))]
    for name, error, change in cases:
        kw = dict(ok())
        kw.update(change)
        with pytest.raises(error, match=name):
            C.batch_norm_act_stats(*(kw[k] for k in ("n", "c", "x", "partials", "eps", "momentum", "running_mean", "running_var", "stat")))
    ok = lambda: dict(n=6, c=8, x=f16(6, 8), mean=f32(8), scale=f32(8), scale_is_var=False, eps=1e-5, weight=f32(8), bias=f32(8), act="tanh",
                      negative_slope=0.0, residual=f32(6, 8), o=f16(6, 8), stat_out=f32(2, 8))
    cases = [("c", ValueError, dict(c=1025)), ("x", TypeError, dict(x=f64(6, 8))), ("mean", ValueError, dict(mean=f32(7))), ("scale", TypeError, dict(scale=f16(8))),
             ("weight", ValueError, dict(weight=f32(9))), ("bias", TypeError, dict(bias=f16(8))), ("act", ValueError, dict(act="gelu")),
             ("residual", TypeError, dict(residual=f64(6, 8))), ("residual", ValueError, dict(residual=f16(6, 7))), ("o", TypeError, dict(o=f32(6, 8))),
             ("o", ValueError, dict(o=f16(5, 8))), ("stat_out", ValueError, dict(stat_out=f32(8)))]
    for name, error, change in cases:
        kw = dict(ok())
        kw.update(change)
        with pytest.raises(error, match=name):
            C.batch_norm_act_forward(*(kw[k] for k in ("n", "c", "x", "mean", "scale", "scale_is_var", "eps", "weight", "bias", "act", "negative_slope",
                                                       "residual", "o", "stat_out")))
    ok = lambda: dict(n=6, c=8, x=f16(6, 8), grad_o=f16(6, 8), stat=f32(2, 8), weight=f32(8), bias=f32(8), act="relu", negative_slope=0.0, training=True,
                      partials=f32(2, 2, 8), grad_weight=f32(8), grad_bias=f32(8), grad_x=f16(6, 8))
    cases = [("c", ValueError, dict(c=0)), ("grad_o", TypeError, dict(grad_o=f32(6, 8))), ("grad_o", ValueError, dict(grad_o=f16(6, 7))),
             ("stat", ValueError, dict(stat=f32(2, 7))), ("act", ValueError, dict(act="sigmoid")), ("partials", ValueError, dict(partials=f32(2, 3, 8))),
             ("grad_weight", ValueError, dict(grad_weight=None)), ("grad_bias", ValueError, dict(grad_bias=f32(9))), ("grad_x", TypeError, dict(grad_x=f32(6, 8))),
             ("grad_weight", ValueError, dict(partials=None, grad_weight=None)), ("partials", ValueError, dict(partials=None, grad_x=None))]
    for name, error, change in cases:
        kw = dict(ok())
        kw.update(change)
        with pytest.raises(error, match=name):
            C.batch_norm_act_backward(*(kw[k] for k in ("n", "c", "x", "grad_o", "stat", "weight", "bias", "act", "negative_slope", "training", "partials",
                                                        "grad_weight", "grad_bias", "grad_x")))


def _torch_act(pre, act, slope):
    return {"none": lambda t: t, "relu": F.relu, "leaky_relu": lambda t: F.leaky_relu(t, slope), "tanh": torch.tanh}[act](pre)


@pytest.mark.parametrize("momentum", [0.02, 0.1])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("act", O.ACTS)
@pytest.mark.parametrize("training,running", [(True, True), (True, False), (False, True), (False, False)])
def test_oracle_is_torch_float64_autograd(training, running, act, with_residual, momentum):
    g = torch.Generator().manual_seed(5)
    n, c, slope = 37, 24, 0.2
    x, go, res = (torch.randn(n, c, generator=g, dtype=torch.float64) for _ in range(3))
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(c, generator=g, dtype=torch.float64), 0.5 + torch.rand(c, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta, res)]
    trm, trv = (rm.clone(), rv.clone()) if running else (None, None)
    # without running statistics nn.BatchNorm1d normalises with batch statistics in eval mode too (its `bn_training`)
    pre = F.batch_norm(leaves[0], trm, trv, leaves[1], leaves[2], training or not running, momentum, 1e-5)
    o = _torch_act(pre, act, slope) + (leaves[3] if with_residual else 0.0)
    (o * go).sum().backward()
    got = O.batch_norm_act(x.numpy(), gamma.numpy(), beta.numpy(), go.numpy(), rm.numpy() if running else None, rv.numpy() if running else None,
                           training, momentum, 1e-5, act, slope, res.numpy() if with_residual else None)
    want = dict(o=o.detach(), dx=leaves[0].grad, dgamma=leaves[1].grad, dbeta=leaves[2].grad, dresidual=leaves[3].grad if with_residual else None,
                running_mean=trm, running_var=trv)
    for name, w in want.items():
        if w is None:
            assert got[name] is None, name
            continue
        scale = max(1.0, float(w.abs().max()))
        assert float(np.abs(got[name] - w.numpy()).max()) <= 1e-12 * scale, name
    if running and not training:
        assert np.array_equal(got["running_mean"], rm.numpy()) and np.array_equal(got["running_var"], rv.numpy())   # eval mode updates nothing


# ---- layers.fuse_batch_norms on CPU tensors ----
SITES = ["stem_layer.0", "stem_layer.1.unary_1", "stem_layer.1.unary_2", "classifier", "regressor"]


def _problem(n=200, seed=3):
    g = torch.Generator().manual_seed(seed)
    feats, xyz = torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g)
    nb = torch.randint(-1, n, (n, 8), generator=g)
    go = (torch.randn(n, 19, generator=g), torch.randn(n, 3, generator=g))
    return feats, xyz, nb, go


def _make(seed=1):
    torch.manual_seed(seed)
    return S.shake_norms(S.StemHeads(S.MeanConv), seed + 1)


def _run(model, feats, xyz, nb, go, train=True):
    model.train(train)
    model.zero_grad(set_to_none=True)
    leaf = feats.clone().requires_grad_(True)
    cls, reg = model(leaf, xyz, None, nb)
    torch.autograd.backward([cls, reg], list(go))
    out = [cls.detach(), reg.detach(), leaf.grad] + [p.grad for _, p in sorted(model.named_parameters())]
    return out + [b.detach().clone() for _, b in sorted(model.named_buffers())]


def _same(want, got):
    """bit-identical lists; a None (the gradient of Res's unused `bn`) on both sides"""
    return len(want) == len(got) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("train", [True, False])
def test_fused_model_on_cpu_tensors_gives_torchs_bits(train):
    problem = _problem()
    plain, fused = _make(), _make()
    keys = list(fused.state_dict())
    assert layers.fuse_batch_norms(fused) == SITES
    assert list(fused.state_dict()) == keys == list(plain.state_dict())
    assert sum("forward" in m.__dict__ for m in fused.modules()) == 4             # Simple, Res (two sites), classifier, regressor
    for _ in range(2):                                                            # twice: the running statistics and the counters move
        want, got = _run(plain, *problem, train=train), _run(fused, *problem, train=train)
        assert _same(want, got)
    tracked = [int(b) for n, b in fused.named_buffers() if n.endswith("num_batches_tracked")]
    assert sorted(tracked) == ([0] + [2] * 5 if train else [0] * 6)               # (Res keeps an unused `bn`, as the model's)
    clone = copy.deepcopy(fused)                                                  # the copy is fused too, and bound to itself
    assert all(m.__dict__["forward"].__self__ is m for m in clone.modules() if "forward" in m.__dict__)
    assert _same(_run(plain, *problem, train=train), _run(clone, *problem, train=train))
    assert layers.fuse_batch_norms(fused) == SITES                                # again: the same sites, bound once
    layers.unfuse_batch_norms(fused)
    assert not any("forward" in m.__dict__ for m in fused.modules()) and list(fused.state_dict()) == keys
    layers.unfuse_batch_norms(plain)                                              # nothing to undo: nothing happens


def test_sites_the_fuser_does_not_recognise():
    model = nn.ModuleDict(dict(
        sync=nn.Sequential(nn.Linear(8, 8), nn.SyncBatchNorm(8), nn.ReLU()),
        gelu=nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8), nn.GELU()),
        relu6=nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8), nn.ReLU6()),
        layer=nn.Sequential(nn.Linear(8, 8), nn.LayerNorm(8), nn.ReLU()),
        bare=nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8)),                                   # a norm that ends its container: act "none"
        mixed=nn.Sequential(nn.BatchNorm1d(8), nn.GELU(), nn.Linear(8, 8), S.FastBatchNorm1d(8), nn.Tanh()),   # the second pair only
    ))
    assert layers.fuse_batch_norms(model) == ["bare", "mixed"]
    assert [n for n, m in model.named_modules() if "forward" in m.__dict__] == ["bare", "mixed"]
    assert {i: (a, s) for i, (_, a, s) in layers._seq_pairs(model["mixed"]).items()} == {3: (("tanh", 0.0), 2)}
    assert {i: (a, s) for i, (_, a, s) in layers._seq_pairs(model["bare"]).items()} == {1: (("none", 0.0), 1)}
    layers.unfuse_batch_norms(model)


class _CountCalls:
    def __init__(self, monkeypatch):
        self.calls = []
        real = pointops.batch_norm_act
        monkeypatch.setattr(pointops, "batch_norm_act", lambda *a, **kw: (self.calls.append(a), real(*a, **kw))[1])


@pytest.mark.parametrize("variant", ["affine=False", "momentum=None", "3-D input", "f64 rows", "half parameters"])
def test_recognised_sites_that_run_their_own_modules(variant, monkeypatch):
    """the conditions of the fused pass are checked at every call, device aside: a stand-in that claims to be a GPU tensor must not
    reach pointops.batch_norm_act"""
    counter = _CountCalls(monkeypatch)
    kw = dict(affine=False) if variant == "affine=False" else dict(momentum=None) if variant == "momentum=None" else {}
    torch.manual_seed(2)
    norm = S.FastBatchNorm1d(8, **kw)
    if variant == "half parameters":
        norm = norm.half()
    seq = nn.Sequential(norm, nn.LeakyReLU(0.2))
    plain = copy.deepcopy(seq)
    x = torch.randn(5, 6, 8) if variant == "3-D input" else torch.randn(30, 8)
    x = x.double() if variant == "f64 rows" else x.half() if variant == "half parameters" else x
    assert layers.fuse_batch_norms(seq) == [""]
    assert layers._bn_call(layers._bn_of(norm), _OnGpu(x), ("leaky_relu", 0.2)) is None
    if variant not in ("f64 rows", "half parameters"):                            # (those two have no CPU kernel to compare with)
        for _ in range(2):
            assert torch.equal(seq(x), plain(x))
        assert all(torch.equal(a, b) for a, b in zip(seq.state_dict().values(), plain.state_dict().values()))
    assert counter.calls == []
