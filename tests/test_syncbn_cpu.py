"""CPU: the declarations of pointops.sync_batch_norm_act (C ABI table, bindings, signatures, argument checks), its float64 oracle
(tests/syncbn_oracle.py), the rank-order Chan merge the kernels implement restated in numpy, sharding.all_gather_rows on a one-rank gloo
group, and layers.fuse_sync_batch_norms(model) on CPU tensors, where every site must run its own modules and give torch's bits.
No HIP compute runs here."""
import copy
import inspect

import numpy as np
import pytest
import torch
from torch import nn

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, layers, pointops, pointops2_cuda, sharding
from tests import batchnorm_oracle as O
from tests import stem_standin as S
from tests import syncbn_oracle as SO
from tests.test_rownorm_cpu import _OnGpu, _g


def test_launchers_are_declared_and_exported():
    I, P, Fl = _lib.I, _lib.P, _lib.F
    assert _lib.SIGNATURES["batch_norm_act_moments_launcher"] == [I] * 3 + [P] * 2 + [I] + [P]
    assert _lib.SIGNATURES["batch_norm_act_merge_launcher"] == [I] * 2 + [P] + [Fl] * 2 + [P] * 4
    assert _lib.SIGNATURES["batch_norm_act_sync_backward_launcher"] == [I] * 4 + [Fl] + [P] * 5 + [I] + [P] * 3
    for name in ("batch_norm_act_moments", "batch_norm_act_merge", "batch_norm_act_sync_backward"):
        assert callable(getattr(pointops2_cuda, name))
    assert pointops2_cuda.BATCH_NORM_MAX_ROWS == 2 ** 24


def test_public_signatures():
    assert str(inspect.signature(pointops.sync_batch_norm_act)) == (
        "(x, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-05, act='none', negative_slope=0.01, residual=None, "
        "group=None)")
    assert str(inspect.signature(layers.fuse_sync_batch_norms)) == "(model)" == str(inspect.signature(layers.fuse_batch_norms))
    assert sta.fuse_sync_batch_norms is layers.fuse_sync_batch_norms and "fuse_sync_batch_norms" in sta.__all__
    assert issubclass(pointops.SyncBatchNormAct, torch.autograd.Function)
    assert str(inspect.signature(sharding.all_gather_rows)) == "(row, group=None)"
    from lib.pointops2.functions import pointops as drop_in
    assert drop_in.sync_batch_norm_act is pointops.sync_batch_norm_act


# ---- the oracle, and the merge the kernels implement ----
SHARDS = [(333,), (5, 0, 328), (1, 1, 1, 1, 1, 1, 1, 2), (200, 133), (0, 7, 0)]


def _ranks(sizes, c, seed):
    g = np.random.default_rng(seed)
    xs = [0.3 + 1.5 * g.standard_normal((n, c)) for n in sizes]
    gos = [g.standard_normal((n, c)) + 0.25 for n in sizes]
    res = [g.standard_normal((n, c)) for n in sizes]
    return xs, gos, res, 1 + 0.2 * g.standard_normal(c), 0.2 * g.standard_normal(c), 0.1 * g.standard_normal(c), 1 + 0.3 * g.random(c)


@pytest.mark.parametrize("act", O.ACTS)
@pytest.mark.parametrize("sizes", SHARDS)
def test_oracle_slices_the_whole_batch_and_the_local_gradients_add_up(sizes, act):
    xs, gos, res, gamma, beta, rm, rv = _ranks(sizes, 6, seed=sum(sizes))
    got = SO.sync_batch_norm_act(xs, gamma, beta, gos, rm, rv, 0.02, 1e-5, act, 0.2, res)
    whole = O.batch_norm_act(np.concatenate(xs), gamma, beta, np.concatenate(gos), rm, rv, True, 0.02, 1e-5, act, 0.2, np.concatenate(res))
    assert got["total"] == sum(sizes) and [o.shape[0] for o in got["o"]] == list(sizes) == [d.shape[0] for d in got["dx"]]
    assert np.array_equal(np.concatenate(got["o"]), whole["o"]) and np.array_equal(np.concatenate(got["dx"]), whole["dx"])
    assert np.array_equal(got["running_mean"], whole["running_mean"]) and np.array_equal(got["running_var"], whole["running_var"])
    for name in ("dgamma", "dbeta"):
        assert len(got[name]) == len(sizes)
        total = np.sum(got[name], axis=0)
        assert float(np.abs(total - whole[name]).max()) <= 1e-12 * max(1.0, float(np.abs(whole[name]).max())), name
        for n, d in zip(sizes, got[name]):
            assert n > 0 or not d.any()                                       # an empty rank: zero parameter gradients
    # the oracle against torch's float64 autograd with per-rank leaf copies of gamma / beta outside a non-affine norm: the local sums
    x = torch.from_numpy(np.concatenate(xs)).requires_grad_(True)
    pre_hat = torch.nn.functional.batch_norm(x, None, None, None, None, True, 0.0, 1e-5)
    leaves, outs, at = [], [], 0
    for n in sizes:
        w, b = torch.from_numpy(gamma).clone().requires_grad_(True), torch.from_numpy(beta).clone().requires_grad_(True)
        pre = pre_hat[at:at + n] * w + b
        outs.append({"none": lambda t: t, "relu": torch.relu, "leaky_relu": lambda t: torch.nn.functional.leaky_relu(t, 0.2), "tanh": torch.tanh}[act](pre))
        leaves.append((w, b))
        at += n
    torch.cat(outs).backward(torch.from_numpy(np.concatenate(gos)))
    assert float(np.abs(x.grad.numpy() - whole["dx"]).max()) <= 1e-11
    for r, (w, b) in enumerate(leaves):
        assert float(np.abs(w.grad.numpy() - got["dgamma"][r]).max()) <= 1e-11 and float(np.abs(b.grad.numpy() - got["dbeta"][r]).max()) <= 1e-11


def _chan(a, b):
    """csrc/batchnorm.hip's chan_merge on (count, mean, M2) rows [3, c]"""
    if b[0][0] == 0:
        return a
    if a[0][0] == 0:
        return b
    n, delta = a[0] + b[0], b[1] - a[1]
    return np.stack([n, a[1] + delta * (b[0] / n), (a[2] + b[2]) + (delta * delta) * (a[0] * b[0] / n)])


@pytest.mark.parametrize("sizes", SHARDS + [(2050, 2049)])
def test_rank_order_chan_merge_reproduces_the_whole_batch_moments(sizes):
    c = 5
    g = np.random.default_rng(7)
    xs = [1e3 + g.standard_normal((n, c)) for n in sizes]
    rows = [np.stack([np.full(c, float(n)), x.mean(0) if n else np.zeros(c), ((x - x.mean(0)) ** 2).sum(0) if n else np.zeros(c)]) for n, x in zip(sizes, xs)]
    m = np.zeros((3, c))
    for row in rows:                                                          # rank order 0 .. world-1
        m = _chan(m, row)
    whole = np.concatenate(xs)
    assert m[0][0] == sum(sizes)
    assert float(np.abs(m[1] - whole.mean(0)).max()) <= 1e-12 * 1e3
    assert float(np.abs(m[2] - ((whole - whole.mean(0)) ** 2).sum(0)).max()) <= 1e-9 * max(1.0, float(m[2].max()))
    # constant within each rank, different between ranks: the variance comes from the deltas alone
    rows = [np.stack([np.full(c, 200.0), np.full(c, 1.0), np.zeros(c)]), np.stack([np.full(c, 133.0), np.full(c, 3.0), np.zeros(c)])]
    m = _chan(_chan(np.zeros((3, c)), rows[0]), rows[1])
    col = np.concatenate([np.full(200, 1.0), np.full(133, 3.0)])
    assert abs(m[1][0] - col.mean()) <= 1e-15 and abs(m[2][0] - ((col - col.mean()) ** 2).sum()) <= 1e-12


# ---- argument checks ----
def _case(**change):
    kw = dict(x=torch.rand(6, 8), weight=torch.ones(8), bias=torch.zeros(8), running_mean=torch.zeros(8), running_var=torch.ones(8),
              residual=torch.rand(6, 8), act="relu", momentum=0.1)
    kw.update(change)
    return kw


@pytest.mark.parametrize("change,error,names", [
    (dict(x=torch.rand(6, 1025), weight=torch.ones(1025), bias=torch.zeros(1025), running_mean=None, running_var=None, residual=None), ValueError, "c must be"),
    (dict(x=torch.rand(6, 8).double()), TypeError, "x must be f32, f16 or bf16"),
    (dict(x=torch.rand(48)), ValueError, "x must be"),
    (dict(x=torch.rand(8, 6).t()), ValueError, "x must be contiguous"),
    (dict(weight=None), ValueError, "weight is None"),
    (dict(bias=torch.zeros(9)), ValueError, "bias must be"),
    (dict(weight=torch.ones(8).half()), TypeError, "weight must be"),
    (dict(running_mean=None), ValueError, "running_mean"),
    (dict(running_var=torch.ones(8).double()), TypeError, "running_var must be"),
    (dict(residual=torch.rand(5, 8)), ValueError, "residual must be"),
    (dict(residual=torch.rand(6, 8).double()), TypeError, "residual must be"),
    (dict(act="gelu"), ValueError, "act must be"),
    (dict(momentum=None), ValueError, "momentum"),
    (dict(x=torch.empty(2 ** 24, 1, dtype=torch.float16), weight=torch.ones(1), bias=torch.zeros(1), running_mean=None, running_var=None,
          residual=None), ValueError, "rows on this rank"),
])
def test_operator_rejects_bad_arguments(change, error, names):
    kw = _case(**change)
    with pytest.raises(error, match="sync_batch_norm_act: .*" + names):
        pointops.sync_batch_norm_act(_g(kw["x"]), _g(kw["weight"]), _g(kw["bias"]), _g(kw["running_mean"]), _g(kw["running_var"]), kw["momentum"],
                                     1e-5, kw["act"], 0.01, _g(kw["residual"]))


def test_cpu_tensors_raise_no_cpu_fallback():
    x, w, b = torch.rand(6, 8), torch.ones(8), torch.zeros(8)
    with pytest.raises(RuntimeError, match="sync_batch_norm_act: .*no CPU fallback"):
        pointops.sync_batch_norm_act(x, w, b)
    C = pointops2_cuda
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.batch_norm_act_moments(6, 8, x, torch.empty(2, 3, 8), torch.empty(3, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.batch_norm_act_merge(2, 8, torch.empty(2, 3, 8), 1e-5, 0.1, None, None, torch.empty(2, 8), torch.empty(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.batch_norm_act_sync_backward(6, 8, x, x, torch.empty(2, 8), w, b, "relu", 0.0, 2, torch.empty(2, 2, 8), torch.empty(1), torch.empty(6, 8))


def test_binding_rejects_bad_shapes_and_dtypes():
    C = pointops2_cuda
    f32 = lambda *s: _OnGpu(torch.zeros(*s))
    f16 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.float16))
    ok = lambda: dict(n=6, c=8, x=f16(6, 8), partials=f32(2, 3, 8), row=f32(3, 8))
    for name, error, change in [("c", ValueError, dict(c=1025)), ("n", ValueError, dict(n=-1)), ("x", ValueError, dict(x=f16(5, 8))),
                                ("partials", ValueError, dict(partials=f32(2, 2, 8))), ("partials", ValueError, dict(partials=None)),
                                ("row", ValueError, dict(row=f32(2, 8))), ("row", TypeError, dict(row=f16(3, 8)))]:
        kw = dict(ok())
        kw.update(change)
        with pytest.raises(error, match=name):
            C.batch_norm_act_moments(*(kw[k] for k in ("n", "c", "x", "partials", "row")))
    ok = lambda: dict(world=2, c=8, rows=f32(2, 3, 8), eps=1e-5, momentum=0.1, running_mean=f32(8), running_var=f32(8), stat=f32(2, 8), total=f32(1))
    for name, error, change in [("c", ValueError, dict(c=0)), ("rows", ValueError, dict(rows=f32(3, 3, 8))), ("rows", ValueError, dict(rows=f32(2, 2, 8))),
                                ("rows", ValueError, dict(world=1025, rows=f32(1025, 3, 8))), ("rows", TypeError, dict(rows=f16(2, 3, 8))),
                                ("running_var", ValueError, dict(running_var=None)), ("running_mean", ValueError, dict(running_mean=f32(7))),
                                ("stat", ValueError, dict(stat=f32(8, 2))), ("total", ValueError, dict(total=f32(2)))]:
        kw = dict(ok())
        kw.update(change)
        with pytest.raises(error, match=name):
            C.batch_norm_act_merge(*(kw[k] for k in ("world", "c", "rows", "eps", "momentum", "running_mean", "running_var", "stat", "total")))
    ok = lambda: dict(n=6, c=8, x=f16(6, 8), grad_o=f16(6, 8), stat=f32(2, 8), weight=f32(8), bias=f32(8), act="relu", negative_slope=0.0, world=2,
                      sums=f32(2, 2, 8), total=f32(1), grad_x=f16(6, 8))
    for name, error, change in [("grad_o", TypeError, dict(grad_o=f32(6, 8))), ("stat", ValueError, dict(stat=f32(2, 7))), ("act", ValueError, dict(act="gelu")),
                                ("sums", ValueError, dict(sums=f32(2, 3, 8))), ("sums", ValueError, dict(world=3)), ("total", TypeError, dict(total=f16(1))),
                                ("grad_x", TypeError, dict(grad_x=f32(6, 8))), ("grad_x", ValueError, dict(grad_x=f16(5, 8)))]:
        kw = dict(ok())
        kw.update(change)
        with pytest.raises(error, match=name):
            C.batch_norm_act_sync_backward(*(kw[k] for k in ("n", "c", "x", "grad_o", "stat", "weight", "bias", "act", "negative_slope", "world", "sums",
                                                             "total", "grad_x")))


# ---- sharding.all_gather_rows ----
def test_all_gather_rows_on_a_one_rank_gloo_group(tmp_path):
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        calls, real = [], sharding._comm
        sharding._comm = lambda name, fn, *a, **k: (calls.append(name), real(name, fn, *a, **k))[1]
        try:
            sharding.reset_bytes()
            row = torch.arange(3 * 8, dtype=torch.float32).view(3, 8)
            out = sharding.all_gather_rows(row, dist.group.WORLD)
        finally:
            sharding._comm = real
        assert tuple(out.shape) == (1, 3, 8) and torch.equal(out[0], row) and calls == ["all_gather"]
        assert sharding.BYTES_MOVED == 3 * 8 * 4
        # a SyncBatchNorm whose group has one rank does not synchronise: the fused site runs batch_norm_act's path, torch's own on CPU tensors
        assert layers._sync_group(nn.SyncBatchNorm(8).train()) is None
    finally:
        dist.destroy_process_group()
        sharding.reset_bytes()


# ---- layers.fuse_sync_batch_norms(model) ----
def test_sync_sites_are_recognised_only_on_request():
    def make():
        return nn.ModuleDict(dict(
            sync=nn.Sequential(nn.Linear(8, 8), nn.SyncBatchNorm(8), nn.ReLU()),
            gelu=nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8), nn.GELU()),
            relu6=nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8), nn.ReLU6()),
            layer=nn.Sequential(nn.Linear(8, 8), nn.LayerNorm(8), nn.ReLU()),
            bare=nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8)),
            mixed=nn.Sequential(nn.BatchNorm1d(8), nn.GELU(), nn.Linear(8, 8), S.FastBatchNorm1d(8), nn.Tanh()),
        ))
    model = make()
    assert layers.fuse_sync_batch_norms(model) == ["sync", "bare", "mixed"]
    assert [n for n, m in model.named_modules() if "forward" in m.__dict__] == ["sync", "bare", "mixed"]
    assert {i: (a, s) for i, (_, a, s) in layers._seq_pairs(model["sync"], True).items()} == {1: (("relu", 0.0), 2)}
    assert layers._seq_pairs(model["sync"]) == {}
    layers.unfuse_batch_norms(model)
    assert not any("forward" in m.__dict__ for m in model.modules())
    model = make()
    assert layers.fuse_batch_norms(model) == ["bare", "mixed"]
    assert "forward" not in model["sync"].__dict__


def _sync_sites(seed=1):
    torch.manual_seed(seed)
    model = nn.ModuleDict(dict(seq=nn.Sequential(nn.Linear(48, 48), nn.BatchNorm1d(48), nn.ReLU()), simple=S.Simple(3, 48, S.MeanConv),
                               res=S.Res(48, 48, S.MeanConv)))
    return S.shake_norms(nn.SyncBatchNorm.convert_sync_batchnorm(model), seed + 1)


def _run_sites(model, feats, xyz, nb, go, train):
    model.train(train)
    model.zero_grad(set_to_none=True)
    leaf = feats.clone().requires_grad_(True)
    rows = model["simple"](leaf, xyz, None, nb)
    out = model["seq"](model["res"](rows, xyz, None, nb))
    out.backward(go)
    return [out.detach(), leaf.grad] + [p.grad for _, p in sorted(model.named_parameters())] + [b.detach().clone() for _, b in sorted(model.named_buffers())]


@pytest.mark.parametrize("train", [True, False])
def test_fused_sync_sites_on_cpu_tensors_run_their_own_modules(train, monkeypatch):
    calls = []
    for name in ("batch_norm_act", "sync_batch_norm_act"):
        monkeypatch.setattr(pointops, name, lambda *a, _n=name, **kw: calls.append(_n))
    g = torch.Generator().manual_seed(3)
    n = 120
    problem = (torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g), torch.randint(-1, n, (n, 8), generator=g), torch.randn(n, 48, generator=g))
    plain, fused = _sync_sites(), _sync_sites()
    assert sum(isinstance(m, nn.SyncBatchNorm) for m in fused.modules()) == 5      # seq, simple, res: unary_1, unary_2, the unused bn
    keys = list(fused.state_dict())
    assert layers.fuse_batch_norms(fused) == []                                     # the default leaves them alone
    assert layers.fuse_sync_batch_norms(fused) == ["seq", "simple", "res.unary_1", "res.unary_2"]
    assert list(fused.state_dict()) == keys == list(plain.state_dict())
    same = lambda want, got: len(want) == len(got) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(want, got))
    for _ in range(2):
        assert same(_run_sites(plain, *problem, train), _run_sites(fused, *problem, train))
    clone = copy.deepcopy(fused)
    bound = [m.__dict__["forward"] for m in clone.modules() if "forward" in m.__dict__]
    assert len(bound) == 3 and all(f.__func__ in layers._BN_SYNC_FORWARDS for f in bound)
    assert all(m.__dict__["forward"].__self__ is m for m in clone.modules() if "forward" in m.__dict__)
    assert same(_run_sites(plain, *problem, train), _run_sites(clone, *problem, train))
    tracked = sorted(int(b) for k, b in fused.named_buffers() if k.endswith("num_batches_tracked"))
    assert tracked == ([0] + [2] * 4 if train else [0] * 5)
    layers.unfuse_batch_norms(fused)
    assert not any("forward" in m.__dict__ for m in fused.modules()) and calls == []
    # a stand-in that claims to be a GPU tensor reaches batch_norm_act, not the collective path: no process group, no synchronisation
    bn = fused["seq"][1].train(train)
    out = layers._bn_call(bn, _OnGpu(torch.randn(30, 48)), ("relu", 0.0))
    assert calls == ["batch_norm_act"] and out == (None, False)
