"""GPU (-m gpu): batch norm + activation (+ residual) with the statistics of several ranks' rows - the launchers
batch_norm_act_moments / _merge / _sync_backward of csrc/batchnorm.hip, pointops.sync_batch_norm_act and the fused sites of
layers.fuse_sync_batch_norms(model) - against the float64 oracle of tests/syncbn_oracle.py on the same inputs.

Bars: those of tests/test_batchnorm_hip.py.  err(.) = max |. - float64 oracle|; u = 2^-24 / 2^-11 / 2^-8 for f32 / f16 / bf16 results;
"composite" = torch's own chain on the CONCATENATED rows on the GPU in the same test: a non-affine F.batch_norm (which also updates the
running statistics), then per-rank leaf copies of gamma / beta applied to each rank's slice, the activation, the add rounded to the rows'
type - so autograd yields each rank's LOCAL parameter sums, as SyncBatchNorm leaves them.
    o, dx (the ranks' rows concatenated), dgamma, dbeta (the ranks' rows stacked [world, C]), running_mean, running_var:
        err(fused) <= 4 * err(composite) + u * max|want|
Each named tensor is held to the bar as a whole, as in that file: a rank of one row has twelve values whose error is a global quantity's
(the mean, the sums over all ranks), so a bar per rank would compare two noises on a dozen draws.
Inputs, the dO recipe and the settling of x away from relu's / leaky_relu's kink are that file's `_inputs` / `_settle` on the concatenated
rows, i.e. on the GLOBAL statistics.  Two runs: the same bits.  World 1: the bits of batch_norm_act.  A NaN / Inf column: the oracle's set
of non-finite entries on every rank, every other column bit-identical to the clean run.

Ranks are emulated on the one device at launcher level (moments per shard; stack; merge; forward, local sums and dx per shard), run as two
processes over gloo through the fused sites, and as one process over nccl (RCCL) on device tensors.  Through the sites, what each norm
was fed and returned is recorded per rank (x, dO, residual in; o, dx, the local parameter gradients, the running statistics out) and the
parent holds it to the oracle on the ranks' concatenated rows.

BYTES_MOVED: sharding counts what a rank hands to a collective.  A site call gathers a [3, C] row in the forward and a [2, C] row in
the backward: 5 * C * 4 bytes per site call and rank (every rank receives world times that).

Measured on one MI355X (max abs error against float64, fused / composite; leaky_relu(0.2), momentum 0.02):
    fp32  333 (world 1)      c=48    o 6.4e-07 / 6.1e-07   dx 3.4e-07 / 5.5e-07   dgamma 1.2e-05 / 1.2e-05   dbeta 9.7e-06 / 9.6e-06   running_mean 3.2e-08 / 3.2e-08   running_var 2.3e-07 / 2.3e-07
    fp32  5+0+328            c=48    o 6.9e-07 / 6.1e-07   dx 4.3e-07 / 5.5e-07   dgamma 1.4e-05 / 1.2e-05   dbeta 9.5e-06 / 8.0e-06   running_mean 3.2e-08 / 3.2e-08   running_var 2.3e-07 / 2.3e-07
    fp32  1+1+1+1+1+1+1+2    c=12    o 2.7e-07 / 2.7e-07   dx 2.2e-07 / 1.5e-07   dgamma 2.5e-07 / 4.9e-07   dbeta 1.8e-08 / 1.8e-08   running_mean 2.0e-08 / 2.0e-08   running_var 2.0e-07 / 2.0e-07
    fp32  2050+2049          c=48    o 8.3e-07 / 8.3e-07   dx 4.9e-07 / 5.1e-07   dgamma 6.1e-05 / 1.3e-04   dbeta 5.2e-05 / 5.2e-05   running_mean 2.9e-08 / 3.4e-08   running_var 2.7e-07 / 2.7e-07
    fp32  3+2                c=1024  o 6.2e-07 / 5.9e-07   dx 1.4e-06 / 1.0e-06   dgamma 7.1e-07 / 1.2e-06   dbeta 2.4e-07 / 2.4e-07   running_mean 5.5e-08 / 5.5e-08   running_var 2.7e-07 / 2.7e-07
    (c=100: 25 chunks in a 32-lane segment; c=96 misaligned and c=70: one channel a lane, 16 a lane)
    fp32  200+133            c=100   o 7.1e-07 / 9.8e-07   dx 5.1e-07 / 4.6e-07   dgamma 1.0e-05 / 1.1e-05   dbeta 6.2e-06 / 6.1e-06   running_mean 6.2e-08 / 6.2e-08   running_var 2.6e-07 / 2.6e-07
    fp32  200+133 misaligned c=96    o 6.8e-07 / 7.5e-07   dx 4.4e-07 / 3.9e-07   dgamma 9.4e-06 / 1.2e-05   dbeta 4.8e-06 / 4.2e-06   running_mean 5.4e-08 / 5.4e-08   running_var 2.3e-07 / 2.3e-07
    f16   200+133            c=48    o 2.0e-03 / 3.8e-03   dx 9.2e-04 / 3.0e-03   dgamma 8.6e-06 / 2.1e-02   dbeta 6.5e-06 / 2.5e-02   running_mean 3.5e-08 / 3.5e-08   running_var 2.4e-07 / 2.4e-07
    bf16  200+133            c=48    o 1.6e-02 / 4.0e-02   dx 7.8e-03 / 6.7e-01   dgamma 8.4e-06 / 1.6e-01   dbeta 9.2e-06 / 8.7e-01   running_mean 4.7e-08 / 4.7e-08   running_var 2.4e-07 / 2.4e-07
    (half rows: the composite multiplies by gamma and adds beta in the half type; the fused passes round once)
    hard columns, constant            o 0 / 0               dx 6.7e-05 / 9.1e-05   dgamma 0 / 0             running_var 1.4e-08 / 1.4e-08
    hard columns, 1e3 + N(0, 1)       o 1.3e-05 / 1.3e-05   dx 9.2e-06 / 1.6e-05   dgamma 3.4e-04 / 2.9e-04   running_var 1.7e-07 / 1.7e-07   (variance 1.044463 for 1.044457)
    hard columns, 1.0 | 3.0 per rank  o 6.1e-08 / 6.1e-08   dx 1.7e-07 / 2.0e-07   dgamma 8.1e-07 / 8.1e-07   running_var 4.5e-08 / 4.5e-08   (variance 0.9595182 for 0.9595181)
    two processes, gloo, 333 + 120 rows, what each norm was fed (the ranks' running statistics bit-equal in every call):
    fp32  simple c=48 leaky_relu          o 4.8e-07 / 5.9e-07   dx 2.7e-05 / 1.7e-05   dgamma 7.9e-06 / 9.7e-06   dbeta 1.0e-05 / 9.3e-06
    fp32  res.unary_1 c=12 leaky_relu     o 5.0e-07 / 5.2e-07   dx 6.9e-06 / 3.6e-06   dgamma 9.3e-06 / 9.3e-06   dbeta 5.5e-06 / 4.4e-06
    fp32  res.unary_2 c=48 + residual     o 1.3e-06 / 6.4e-07   dx 5.2e-06 / 5.2e-06   dgamma 3.1e-06 / 5.5e-06   dbeta 2.3e-06 / 2.5e-06
    fp32  seq c=48 relu                   o 9.6e-07 / 9.6e-07   dx 1.4e-06 / 1.4e-06   dgamma 6.0e-06 / 1.7e-05   dbeta 3.9e-06 / 7.6e-06
    f16   simple c=48 leaky_relu          o 1.3e-03 / 3.3e-03   dx 4.6e-02 / 1.2e-01   dgamma 1.0e-05 / 2.4e-02   dbeta 6.1e-06 / 2.9e-02
    f16   res.unary_1 c=12 leaky_relu     o 1.9e-03 / 5.1e-03   dx 1.3e-02 / 1.9e-02   dgamma 3.1e-06 / 1.7e-02   dbeta 3.1e-06 / 2.1e-02
    f16   res.unary_2 c=48 + f16 residual o 1.9e-03 / 4.3e-03   dx 1.5e-02 / 3.7e-01   dgamma 3.8e-06 / 3.3e-02   dbeta 2.6e-06 / 8.0e-02
    f16   seq c=48 relu                   o 1.9e-03 / 5.7e-03   dx 3.6e-03 / 8.3e-03   dgamma 8.2e-06 / 2.0e-02   dbeta 3.8e-06 / 2.0e-02
    nccl (RCCL) with two ranks needs two devices and was skipped on the one-GPU box these figures come from.
Every test prints its figures.
"""
import copy
import os
import time
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F
from torch import nn

from tests import batchnorm_oracle as O
from tests import stem_standin as S
from tests import syncbn_oracle as SO
from tests.test_batchnorm_hip import DTYPES, SLOPE, U, _bits, _f64, _fused, _inputs, _mode, _settle, _to, _torch_act
from tests.test_sharded_hip import _free_port

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAMES = ("o", "dx", "dgamma", "dbeta", "running_mean", "running_var")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


def _cuts(sizes):
    at = np.cumsum([0] + list(sizes))
    return [(int(at[r]), int(at[r + 1])) for r in range(len(sizes))]


def _shards(p, sizes):
    """the host tensors of one case cut into the ranks' rows"""
    cut = lambda t: None if t is None else [t[a:b].contiguous() for a, b in _cuts(sizes)]
    return cut(p["x"]), cut(p["go"]), cut(p["res"])


def _oracle(p, sizes, momentum):
    xs, gos, res = _shards(p, sizes)
    f = lambda parts: None if parts is None else [_f64(t) for t in parts]
    return SO.sync_batch_norm_act(f(xs), _f64(p["gamma"]), _f64(p["beta"]), f(gos), _f64(p["rm"]), _f64(p["rv"]), momentum, EPS, p["act"], SLOPE, f(res))


def _emulate(P, p, sizes, momentum):
    """the ranks of one step on one device, launcher by launcher, each rank with its own copies of the running statistics -> per-name lists
    over the ranks, plus every rank's stat and total"""
    from stratified_transformer_amd import pointops2_cuda as C
    mis, world, c = p["misaligned"], len(sizes), p["x"].shape[1]
    xs, gos, res = _shards(p, sizes)
    xs, gos = [_to(t, mis) for t in xs], [_to(t, mis) for t in gos]
    res = [None] * world if res is None else [_to(t, mis) for t in res]
    w, b = p["gamma"].cuda(), p["beta"].cuda()
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    rows = []
    for x in xs:
        row = f32(3, c)
        C.batch_norm_act_moments(x.shape[0], c, x, P._batch_norm_partials(x.shape[0], c, 3, x) if x.shape[0] else None, row)
        rows.append(row)
    rows = torch.stack(rows)
    out = dict(o=[], dx=[], dgamma=[], dbeta=[], running_mean=[], running_var=[], stat=[], total=[], rows=rows)
    for x, r in zip(xs, res):
        rm, rv, stat, total = p["rm"].cuda(), p["rv"].cuda(), f32(2, c), f32(1)
        C.batch_norm_act_merge(world, c, rows, EPS, momentum, rm, rv, stat, total)
        o = torch.empty_like(x)
        C.batch_norm_act_forward(x.shape[0], c, x, stat[0], stat[1], False, EPS, w, b, p["act"], SLOPE, r, o, None)
        for name, t in (("o", o), ("running_mean", rm), ("running_var", rv), ("stat", stat), ("total", total)):
            out[name].append(t)
    sums = []
    for x, go, stat in zip(xs, gos, out["stat"]):
        n = x.shape[0]
        local = torch.zeros(2, c, device="cuda")
        if n:
            C.batch_norm_act_backward(n, c, x, go, stat, w, b, p["act"], SLOPE, True, P._batch_norm_partials(n, c, 2, x), local[0], local[1], None)
        sums.append(local)
    sums = torch.stack(sums)
    for r, (x, go) in enumerate(zip(xs, gos)):
        dx = torch.empty_like(x)
        C.batch_norm_act_sync_backward(x.shape[0], c, x, go, out["stat"][r], w, b, p["act"], SLOPE, world, sums, out["total"][r], dx)
        out["dx"].append(dx)
        out["dgamma"].append(sums[r, 0])
        out["dbeta"].append(sums[r, 1])
    torch.cuda.synchronize()
    return out


def _composite(xs, gos, res, gamma, beta, rm, rv, momentum, act, slope=SLOPE):
    """torch's chain on the concatenated rows (module docstring); every argument a list of device tensors per rank or a device tensor"""
    sizes = [x.shape[0] for x in xs]
    x = torch.cat(xs).requires_grad_(True)
    rm, rv = rm.clone(), rv.clone()
    xhat = F.batch_norm(x, rm, rv, None, None, True, momentum, EPS)
    leaves, outs = [], []
    for r, (a, b) in enumerate(_cuts(sizes)):
        w, bb = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        o = _torch_act_slope(xhat[a:b] * w.to(x.dtype) + bb.to(x.dtype), act, slope)
        if res is not None and res[r] is not None:
            o = (o + res[r]).to(x.dtype)
        outs.append(o)
        leaves.append((w, bb))
    torch.cat(outs).backward(torch.cat(gos))
    torch.cuda.synchronize()
    zero = torch.zeros_like(gamma)
    return dict(o=[o.detach() for o in outs], dx=[x.grad[a:b] for a, b in _cuts(sizes)], dgamma=[w.grad if w.grad is not None else zero for w, _ in leaves],
                dbeta=[b.grad if b.grad is not None else zero for _, b in leaves], running_mean=rm, running_var=rv)


def _torch_act_slope(pre, act, slope):
    return F.leaky_relu(pre, slope) if act == "leaky_relu" else _torch_act(pre, act)


def _whole(t, name):
    """a per-rank list as the one tensor the bar is applied to; the running statistics: rank 0's"""
    if name in ("o", "dx"):
        return np.concatenate([_f64(q) if torch.is_tensor(q) else q for q in t], 0)
    if name in ("dgamma", "dbeta"):
        return np.stack([_f64(q) if torch.is_tensor(q) else q for q in t], 0)
    t = t[0] if isinstance(t, list) else t
    return _f64(t) if torch.is_tensor(t) else t


def _hold(label, want, got, comp, dt):
    figures, ok = [], True
    for name in NAMES:
        w = _whole(want[name], name)
        u = U[dt] if name in ("o", "dx") else U[torch.float32]
        e_f = float(np.abs(_whole(got[name], name) - w).max(initial=0.0))
        e_c = float(np.abs(_whole(comp[name], name) - w).max(initial=0.0))
        top = float(np.abs(w).max(initial=0.0))
        figures.append(f"{name} {e_f:.2e}/{e_c:.2e}")
        ok = ok and e_f <= 4 * e_c + u * top
    print(f"sync_batch_norm_act {label}: " + "  ".join(figures) + ("" if ok else "   <-- over the bar"))
    assert ok, label


def _check(P, sizes, c, xname="f32", rname=None, act="leaky_relu", misaligned=False, momentum=0.02, seed=None):
    p = _inputs(sum(sizes), c, xname, rname, act, seed=c + sum(sizes) if seed is None else seed, misaligned=misaligned)
    want, got = _oracle(p, sizes, momentum), _emulate(P, p, sizes, momentum)
    xs, gos, res = _shards(p, sizes)
    dev = lambda parts: None if parts is None else [t.cuda() for t in parts]
    comp = _composite(dev(xs), dev(gos), dev(res), p["gamma"].cuda(), p["beta"].cuda(), p["rm"].cuda(), p["rv"].cuda(), momentum, act)
    dt = DTYPES[xname]
    for r, n in enumerate(sizes):
        assert got["o"][r].dtype == got["dx"][r].dtype == dt and tuple(got["o"][r].shape) == tuple(got["dx"][r].shape) == (n, c)
        assert float(got["total"][r]) == float(sum(sizes))
        for name in ("stat", "total", "running_mean", "running_var"):                      # the same stacked rows: the same bits on every rank
            assert torch.equal(_bits(got[name][r]), _bits(got[name][0])), (name, r)
    label = f"{xname} ranks={'+'.join(map(str, sizes))} c={c} {act} residual={rname}{' misaligned' if misaligned else ''}"
    _hold(label, want, got, comp, dt)
    return p, got


# ---- 1. emulated ranks, launcher level ----
def test_world_one_gives_batch_norm_acts_bits(P):
    p, got = _check(P, (333,), 48, rname="f32")
    ref = _fused(P, p, _mode(momentum=0.02))
    for name in NAMES:
        assert torch.equal(_bits(got[name][0]), _bits(ref[name])), name


@pytest.mark.parametrize("sizes,c,misaligned", [((5, 0, 328), 48, False), ((1, 1, 1, 1, 1, 1, 1, 2), 12, False), ((2050, 2049), 48, False),
                                                ((3, 2), 1024, False), ((200, 133), 100, False), ((200, 133), 96, True),
                                                ((200, 133), 70, False)])
@pytest.mark.parametrize("with_res", [True, False])
def test_emulated_ranks_fp32(P, sizes, c, misaligned, with_res):
    _check(P, sizes, c, rname="f32" if with_res else None, misaligned=misaligned)


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_emulated_ranks_half_rows(P, name):
    _check(P, (200, 133), 48, xname=name, rname="f32")


@pytest.mark.parametrize("act", O.ACTS)
def test_emulated_ranks_activations(P, act):
    _check(P, (200, 133), 48, rname="f32", act=act, momentum=0.1, seed=17)


# ---- 2. the same bits ----
def test_two_runs_give_the_same_bits(P):
    for xname in ("f32", "f16"):
        p = _inputs(333, 48, xname, "f32", "leaky_relu", seed=3)
        a, b = _emulate(P, p, (200, 133), 0.02), _emulate(P, p, (200, 133), 0.02)
        assert torch.equal(_bits(a["rows"]), _bits(b["rows"]))
        for name in NAMES + ("stat", "total"):
            for r in range(2):
                assert torch.equal(_bits(a[name][r]), _bits(b[name][r])), (xname, name, r)
                if name in ("stat", "total", "running_mean", "running_var"):
                    assert torch.equal(_bits(a[name][r]), _bits(a[name][0])), (xname, name, r)


# ---- 3. hard columns ----
def test_hard_columns(P):
    """(200, 133) x 48.  Column 0: constant over all ranks.  Column 2: constant within each rank, 1.0 on rank 0 and 3.0 on rank 1 - every
    rank's M2 is 0 and the variance comes from the merge's delta term alone.  Column 1: 1e3 + N(0, 1).  Column 4: one NaN on rank 0.
    Column 9: one +Inf on rank 1.  The poison reaches BOTH ranks' rows of its column, and no other column."""
    sizes, c, momentum = (200, 133), 48, 0.02
    n = sum(sizes)
    p = _inputs(n, c, "f32", None, "leaky_relu", seed=21)
    p["x"][:, 0], p["beta"][0] = 1.5, 0.3
    p["x"][:, 1] = 1e3 + torch.randn(n, generator=torch.Generator().manual_seed(1))
    p["x"][:200, 2], p["x"][200:, 2] = 1.0, 3.0
    p = _settle(p, _mode(momentum=momentum))
    assert float(p["x"][:200, 2].max()) == float(p["x"][:200, 2].min()) and float(p["x"][200:, 2].max()) == float(p["x"][200:, 2].min())
    clean = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in p.items()}
    p["x"][40, 4] = float("nan")
    p["x"][200 + 7, 9] = float("inf")
    want, got, ref = _oracle(p, sizes, momentum), _emulate(P, p, sizes, momentum), _emulate(P, clean, sizes, momentum)
    xs, gos, _ = _shards(p, sizes)
    comp = _composite([t.cuda() for t in xs], [t.cuda() for t in gos], None, p["gamma"].cuda(), p["beta"].cuda(), p["rm"].cuda(), p["rv"].cuda(),
                      momentum, "leaky_relu")
    cols = [k for k in range(c) if k not in (4, 9)]
    for name in NAMES:
        for r in range(2):
            g = _f64(got[name][r])
            w = want[name][r] if isinstance(want[name], list) else want[name]
            assert np.array_equal(np.isfinite(g), np.isfinite(w)), (name, r)               # the oracle's set of non-finite entries, on every rank
            assert np.isfinite(w[..., cols]).all(), name
            if name != "dbeta":                                                            # (leaky_relu's derivative of a NaN is its slope: dbeta stays finite)
                assert not np.isfinite(w[..., [4, 9]]).any(), (name, r)
            assert torch.equal(_bits(got[name][r][..., cols]), _bits(ref[name][r][..., cols])), (name, r)   # the other columns: as without the poison
    for k, what in ((0, "constant"), (1, "1e3 + N(0,1)"), (2, "constant per rank, 1.0 | 3.0")):
        figures = []
        for name in NAMES:
            w = _whole(want[name], name)[..., k]
            e_f, e_c = (float(np.abs(_whole(t[name], name)[..., k] - w).max()) for t in (got, comp))
            top = float(np.abs(w).max())
            figures.append(f"{name} {e_f:.2e}/{e_c:.2e}")
            assert e_f <= 4 * e_c + U[torch.float32] * top, (what, name, e_f, e_c, top)
        print(f"sync_batch_norm_act hard columns, {what}: " + "  ".join(figures))
    keep = np.float32(1.0) - np.float32(momentum)
    for r in range(2):
        assert float(got["rows"][r, 2, 0]) == 0.0 and float(got["rows"][r, 2, 2]) == 0.0   # every rank's own M2 of the two constant columns
        assert float(got["stat"][r][0, 0]) == 1.5                                          # the mean, exactly
        assert float((got["o"][r][:, 0] - 0.3).abs().max()) == 0.0                         # variance 0: o is act(beta), exactly
        assert float(got["running_var"][r][0]) == float(keep * np.float32(float(p["rv"][0])))   # and the merged M2 is exactly 0
    var2 = float(1.0 / got["stat"][0][1, 2] ** 2 - EPS)
    exact = float(_f64(p["x"][:, 2]).var())
    print(f"sync_batch_norm_act hard columns, variance of the 1.0 | 3.0 column: {var2:.7f} (float64: {exact:.7f})")
    assert abs(var2 - exact) <= 1e-5 * exact
    var1 = float(1.0 / got["stat"][0][1, 1] ** 2 - EPS)
    print(f"sync_batch_norm_act hard columns, variance of the 1e3 + N(0,1) column: {var1:.6f} (float64: {float(_f64(p['x'][:, 1]).var()):.6f})")
    assert abs(var1 - float(_f64(p["x"][:, 1]).var())) <= 1e-3


# ---- 4. an empty rank ----
def test_an_empty_rank_changes_nothing(P):
    p = _inputs(333, 48, "f32", "f32", "leaky_relu", seed=5)
    two, three = _emulate(P, p, (200, 133), 0.02), _emulate(P, p, (200, 0, 133), 0.02)
    assert tuple(three["o"][1].shape) == tuple(three["dx"][1].shape) == (0, 48)
    assert float(three["rows"][1].abs().max()) == 0.0                                      # its moments row: zeros, count included
    assert float(three["dgamma"][1].abs().max()) == 0.0 and float(three["dbeta"][1].abs().max()) == 0.0
    for name in NAMES + ("stat", "total"):
        for r2, r3 in ((0, 0), (1, 2)):
            assert torch.equal(_bits(two[name][r2]), _bits(three[name][r3])), (name, r2)
        assert name in ("o", "dx", "dgamma", "dbeta") or torch.equal(_bits(three[name][1]), _bits(three[name][0])), name   # it holds the statistics too


# ---- 5., 7. two processes through the fused sites ----
SITE_ROWS = (333, 120)
SITE_NAMES = ["seq", "simple", "res.unary_1", "res.unary_2"]
SITE_C = [48, 12, 48, 48]                                                                  # in call order: simple, res.unary_1, res.unary_2, seq


def _site_model(which, seed=4):
    torch.manual_seed(seed)
    mods = dict(seq=nn.Sequential(nn.Linear(48, 48), nn.BatchNorm1d(48), nn.ReLU()))
    if which == "all":
        mods.update(simple=S.Simple(3, 48, S.MeanConv), res=S.Res(48, 48, S.MeanConv))
    return S.shake_norms(nn.SyncBatchNorm.convert_sync_batchnorm(nn.ModuleDict(mods)), seed + 1)


def _site_inputs(which, seed=6):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in SITE_ROWS:
        out.append(dict(feats=torch.randn(n, 3 if which == "all" else 48, generator=g).numpy(), xyz=torch.rand(n, 3, generator=g).numpy(),
                        nb=torch.randint(-1, n, (n, 8), generator=g).numpy(), go=(torch.randn(n, 48, generator=g) + 0.25).numpy()))
    return out


def _run_sites(model, which, feats, xyz, nb, go, amp):
    leaf = feats.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        rows = leaf
        if which == "all":
            rows = model["res"](model["simple"](rows, xyz, None, nb), xyz, None, nb)
        out = model["seq"](rows)
    out.backward(go.to(out.dtype))
    torch.cuda.synchronize()
    return out, leaf


def _site_worker(rank, world, port, backend, which, inputs, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        from stratified_transformer_amd import layers, pointops as P, sharding
        base = _site_model(which).to(dev).train()
        keys = list(base.state_dict())
        assert layers.fuse_sync_batch_norms(base) == (SITE_NAMES if which == "all" else ["seq"]) and list(base.state_dict()) == keys
        records, comms = [], []
        real_op, real_plain, real_comm = P.sync_batch_norm_act, P.batch_norm_act, sharding._comm
        plain_calls = []

        def recording(x, weight, bias, rm, rv, momentum, eps, act, slope, residual, group):
            rec = dict(x=x.detach().clone(), act=act, slope=slope, momentum=momentum, eps=eps, weight=weight, bias=bias,
                       gamma=weight.detach().clone(), beta=bias.detach().clone(), rm0=rm.clone(), rv0=rv.clone(), rm=rm, rv=rv,
                       res=None if residual is None else residual.detach().clone())
            o = real_op(x, weight, bias, rm, rv, momentum, eps, act, slope, residual, group)
            rec["o"] = o.detach().clone()
            x.register_hook(lambda g, rec=rec: rec.__setitem__("dx", g.detach().clone()))   # (the norm is x's only consumer)
            o.register_hook(lambda g, rec=rec: rec.__setitem__("go", g.detach().clone()))
            records.append(rec)
            return o

        P.sync_batch_norm_act = recording
        P.batch_norm_act = lambda *a, **k: (plain_calls.append(1), real_plain(*a, **k))[1]
        sharding._comm = lambda name, fn, *a, **k: (comms.append(name), real_comm(name, fn, *a, **k))[1]
        d = inputs[rank]
        t = lambda a: torch.from_numpy(a).to(dev)
        feats, xyz, nb, go = t(d["feats"]), t(d["xyz"]), t(d["nb"]), t(d["go"])
        res = {}
        n_sites = len(SITE_C) if which == "all" else 1
        for tag, amp in (("fp32", False), ("amp", True)):
            model = copy.deepcopy(base)
            del records[:], comms[:], plain_calls[:]
            sharding.reset_bytes()
            model.zero_grad(set_to_none=True)
            _run_sites(model, which, feats, xyz, nb, go, amp)
            assert len(records) == n_sites and plain_calls == [] and comms == ["all_gather"] * (2 * n_sites), (len(records), comms)
            res[f"{tag}_bytes"] = np.int64(sharding.BYTES_MOVED)
            assert list(model.state_dict()) == keys
            for i, rec in enumerate(records):
                assert rec["x"].dtype == (torch.float16 if amp else torch.float32)
                for name in ("x", "o", "go", "dx", "gamma", "beta", "rm0", "rv0", "rm", "rv", "res"):
                    if rec[name] is not None:
                        res[f"{tag}_{i}_{name}"] = rec[name].detach().float().cpu().numpy()
                res[f"{tag}_{i}_dgamma"], res[f"{tag}_{i}_dbeta"] = rec["weight"].grad.cpu().numpy(), rec["bias"].grad.cpu().numpy()
                res[f"{tag}_{i}_meta"] = np.array([rec["act"], str(rec["slope"]), str(rec["momentum"]), str(rec["x"].dtype).split(".")[1],
                                                   "None" if rec["res"] is None else str(rec["res"].dtype).split(".")[1]])
            res[f"{tag}_tracked"] = np.array([int(b) for k, b in sorted(model.named_buffers()) if k.endswith("num_batches_tracked")])
            # eval mode: the same sites, no collective, the plain operator
            model.eval()
            del records[:], comms[:], plain_calls[:]
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                rows = feats
                if which == "all":
                    rows = model["res"](model["simple"](rows, xyz, None, nb), xyz, None, nb)
                model["seq"](rows)
            torch.cuda.synchronize()
            assert comms == [] and records == [] and len(plain_calls) == n_sites, (comms, len(records), len(plain_calls))
        # an empty rank through the operator: rank 1 hands in no rows
        P.sync_batch_norm_act = real_op
        n = 120 if rank == 0 else 0
        g = torch.Generator().manual_seed(8)
        x = (0.3 + 1.5 * torch.randn(120, 48, generator=g))[:n].to(dev).requires_grad_(True)
        w, b = (1 + 0.2 * torch.randn(48, generator=g)).to(dev).requires_grad_(True), (0.2 * torch.randn(48, generator=g)).to(dev).requires_grad_(True)
        rm, rv = torch.zeros(48, device=dev), torch.ones(48, device=dev)
        o = real_op(x, w, b, rm, rv, 0.1, EPS, "tanh", 0.0, None, dist.group.WORLD)
        o.backward((torch.randn(120, 48, generator=g) + 0.25)[:n].to(dev))
        torch.cuda.synchronize()
        for name, v in (("o", o.detach()), ("dx", x.grad), ("dgamma", w.grad), ("dbeta", b.grad), ("rm", rm), ("rv", rv)):
            res[f"empty_{name}"] = v.cpu().numpy()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


def _spawn(worker, args, world, limit=300.0):
    """mp.spawn with a limit: a worker that raises ends its peer (ProcessContext.join terminates the others and re-raises); past the limit
    the children are ended and the test fails"""
    ctx = mp.spawn(worker, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=5.0):
            assert time.monotonic() < deadline, "the ranks did not finish in time"
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.terminate()
        for proc in ctx.processes:
            proc.join(10)


def _check_sites(P, tmp_path, which, backend):
    world = 2
    inputs = _site_inputs(which)
    _spawn(_site_worker, (world, _free_port(), backend, which, inputs, str(tmp_path)), world)
    ranks = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(world)]
    site_c = SITE_C if which == "all" else [48]
    for tag in ("fp32", "amp"):
        for r in ranks:
            assert int(r[f"{tag}_bytes"]) == sum(5 * c * 4 for c in site_c)                # per rank: a [3, C] and a [2, C] row per site call
            assert r[f"{tag}_tracked"].tolist() == ([0] + [1] * 4 if which == "all" else [1])   # (Res keeps an unused `bn`)
        for i, c in enumerate(site_c):
            act, slope, momentum, xdt, rdt = ranks[0][f"{tag}_{i}_meta"].tolist()
            assert ranks[1][f"{tag}_{i}_meta"].tolist() == [act, slope, momentum, xdt, rdt]
            slope, momentum, dt = float(slope), float(momentum), getattr(torch, xdt)
            has_res = rdt != "None"
            get = lambda name: [r[f"{tag}_{i}_{name}"] for r in ranks]
            for name in ("gamma", "beta", "rm0", "rv0"):
                assert np.array_equal(*get(name)), name
            for name in ("rm", "rv"):                                                      # bit-equal across the ranks
                assert np.array_equal(get(name)[0].view(np.int32), get(name)[1].view(np.int32)), (tag, i, name)
            xs, gos, res = get("x"), get("go"), get("res") if has_res else None
            assert [x.shape for x in xs] == [(n, c) for n in SITE_ROWS]
            gamma, beta, rm0, rv0 = (get(name)[0] for name in ("gamma", "beta", "rm0", "rv0"))
            want = SO.sync_batch_norm_act(xs, gamma, beta, gos, rm0, rv0, momentum, EPS, act, slope, res)
            pre = np.concatenate(xs).astype(np.float64)
            pre = (pre - pre.mean(0)) / np.sqrt(pre.var(0) + EPS) * gamma + beta
            print(f"sites {backend} {tag} call {i} ({act}, {xdt} rows, residual {rdt}): smallest |pre| {float(np.abs(pre).min()):.2e}")
            cu = lambda parts, d: None if parts is None else [torch.from_numpy(a).cuda().to(d) for a in parts]
            comp = _composite(cu(xs, dt), cu(gos, dt), cu(res, getattr(torch, rdt)) if has_res else None, torch.from_numpy(gamma).cuda(),
                              torch.from_numpy(beta).cuda(), torch.from_numpy(rm0).cuda(), torch.from_numpy(rv0).cuda(), momentum, act, slope)
            got = dict(o=get("o"), dx=get("dx"), dgamma=get("dgamma"), dbeta=get("dbeta"), running_mean=get("rm")[0], running_var=get("rv")[0])
            _hold(f"sites {backend} {tag} call {i} c={c} {act} rows={xdt} residual={rdt}", want, got, comp, dt)
    # the empty rank: shapes, zero parameter gradients, and rank 0 alone is batch_norm_act on its rows
    e0, e1 = ranks
    assert e1["empty_o"].shape == e1["empty_dx"].shape == (0, 48) and not e1["empty_dgamma"].any() and not e1["empty_dbeta"].any()
    assert np.array_equal(e0["empty_rm"].view(np.int32), e1["empty_rm"].view(np.int32)) and np.array_equal(e0["empty_rv"].view(np.int32), e1["empty_rv"].view(np.int32))
    g = torch.Generator().manual_seed(8)
    x = (0.3 + 1.5 * torch.randn(120, 48, generator=g)).cuda().requires_grad_(True)
    w, b = (1 + 0.2 * torch.randn(48, generator=g)).cuda().requires_grad_(True), (0.2 * torch.randn(48, generator=g)).cuda().requires_grad_(True)
    rm, rv = torch.zeros(48, device="cuda"), torch.ones(48, device="cuda")
    o = P.batch_norm_act(x, w, b, rm, rv, True, 0.1, EPS, "tanh", 0.0, None)
    o.backward((torch.randn(120, 48, generator=g) + 0.25).cuda())
    for name, v in (("o", o.detach()), ("dx", x.grad), ("dgamma", w.grad), ("dbeta", b.grad), ("rm", rm), ("rv", rv)):
        assert np.array_equal(e0[f"empty_{name}"].view(np.int32), v.cpu().numpy().view(np.int32)), name


def test_two_processes_gloo(P, tmp_path):
    """two ranks of 333 and 120 rows on the one GPU, collectives over gloo (staged through the host): the Sequential, the
    KPConvSimpleBlock-shaped and the res-block-shaped site with nn.SyncBatchNorm, fused with fuse_sync_batch_norms, fp32 and autocast(f16)"""
    _check_sites(P, tmp_path, "all", "gloo")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="nccl (RCCL) with two ranks needs two devices: RCCL refuses two ranks on one")
def test_two_processes_nccl(P, tmp_path):
    """the Sequential site, one device per rank, collectives over RCCL on device tensors"""
    _check_sites(P, tmp_path, "seq", "nccl")


# ---- 6. nccl, world 1 ----
def _nccl_world1(port, out_path):
    """a fresh process: backend "nccl" (= RCCL) with ONE rank, the gather on device tensors without host staging"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, timeout=timedelta(seconds=120))
    try:
        from stratified_transformer_amd import pointops as P, sharding
        assert dist.get_backend() == "nccl" and not sharding._host_staged(dist.group.WORLD)
        seen, real = [], sharding._comm
        sharding._comm = lambda name, fn, *a, **k: (seen.append((name, a[1].is_cuda)), real(name, fn, *a, **k))[1]
        p = _inputs(333, 48, "f16", "f32", "leaky_relu", seed=11)
        x, res = p["x"].cuda().requires_grad_(True), p["res"].cuda().requires_grad_(True)
        w, b, rm, rv = p["gamma"].cuda().requires_grad_(True), p["beta"].cuda().requires_grad_(True), p["rm"].cuda(), p["rv"].cuda()
        sharding.reset_bytes()
        o = P.sync_batch_norm_act(x, w, b, rm, rv, 0.02, EPS, "leaky_relu", SLOPE, res, dist.group.WORLD)
        o.backward(p["go"].cuda())
        torch.cuda.synchronize()
        assert seen == [("all_gather", True), ("all_gather", True)] and sharding.BYTES_MOVED == 5 * 48 * 4
        np.savez(out_path, o=o.detach().float().cpu().numpy(), dx=x.grad.float().cpu().numpy(), dgamma=w.grad.cpu().numpy(), dbeta=b.grad.cpu().numpy(),
                 dresidual=res.grad.cpu().numpy(), running_mean=rm.cpu().numpy(), running_var=rv.cpu().numpy())
    finally:
        dist.destroy_process_group()


def test_nccl_world_one_gives_batch_norm_acts_bits(P, tmp_path):
    out_path = os.path.join(str(tmp_path), "nccl1.npz")
    proc = mp.get_context("spawn").Process(target=_nccl_world1, args=(_free_port(), out_path))
    proc.start()
    proc.join(300)
    if proc.is_alive():
        proc.terminate()
        proc.join(10)
    assert proc.exitcode == 0, proc.exitcode
    got = np.load(out_path)
    p = _inputs(333, 48, "f16", "f32", "leaky_relu", seed=11)
    ref = _fused(P, p, _mode(momentum=0.02))
    for name in NAMES + ("dresidual",):
        assert np.array_equal(got[name].view(np.int32), ref[name].float().cpu().numpy().view(np.int32)), name
