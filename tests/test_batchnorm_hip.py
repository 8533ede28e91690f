"""GPU (-m gpu): BatchNorm1d + activation (+ residual) on csrc/batchnorm.hip - pointops.batch_norm_act and the fused forwards of
layers.fuse_batch_norms - against the float64 oracle of tests/batchnorm_oracle.py evaluated on the CPU on the same inputs.

Bars.  err(.) = max |. - float64 oracle|; u = 2^-24 / 2^-11 / 2^-8 for f32 / f16 / bf16 results; "composite" = torch's own unfused chain
(F.batch_norm, the activation, the add rounded to the rows' type) run on the GPU in the same test.
  o, dx, dgamma, dbeta, running_mean, running_var:   err(fused) <= 4 * err(composite) + u * max|want|   (fp32 sums of one length in another order)
  the residual's gradient:                           dO cast to the residual's type, bit for bit
  stem + heads, fp32:                                fused against unfused within 1e-4 of each tensor's own scale (the two Linear biases in
                                                     front of a norm, whose gradient is exactly 0: 1e-4 of their weight gradient's scale)
  heads under autocast(f16):                         the first bar, against the heads in float64 on the CPU
relu and leaky_relu have a kink at pre = 0, where the derivative jumps and a rounding error of pre picks the side.  The operator tests
therefore move every x whose float64 |pre| is below 1e-4 (a hundred times the fp32 error of pre) by 1/8 before anything runs; the model
test takes the first of its seeds at which no pre-activation of the unfused run is within 1e-5 of 0.
The incoming gradient dO is N(0, 1) plus a mean of 0.25 and a 0.25 share of the row's own deviation, as a loss's gradient has: with a
zero-mean dO independent of x, dgamma and dbeta are sums that cancel to about 0 while the rounding of their sqrt(N)-sized partial sums
does not, so `u * max|want|` would scale with nothing, and at a single channel (C = 1: one draw on either side, no maximum over
channels to even them out) the comparison of two such noises would be decided by chance.
Two runs: the same bits.  A NaN / Inf column: the oracle's set of non-finite entries, every other column bit-identical to the run
without the poison.

Measured on one MI355X (max abs error against float64, fused / composite; leaky_relu(0.2), an fp32 residual, momentum 0.02):
    fp32  c=12   n=4099     o 7.3e-07 / 6.3e-07   dx 3.1e-07 / 2.9e-07   dgamma 1.1e-04 / 1.2e-04   dbeta 6.9e-05 / 5.3e-05   running_mean 2.2e-08 / 2.2e-08   running_var 2.1e-07 / 2.1e-07
    fp32  c=48   n=4099     o 1.0e-06 / 7.7e-07   dx 5.1e-07 / 5.7e-07   dgamma 1.4e-04 / 1.9e-04   dbeta 1.2e-04 / 8.3e-05   running_mean 2.9e-08 / 3.4e-08   running_var 2.7e-07 / 2.7e-07
    fp32  c=384  n=4099     o 9.9e-07 / 9.3e-07   dx 5.4e-07 / 7.1e-07   dgamma 1.9e-04 / 2.5e-04   dbeta 9.9e-05 / 1.2e-04   running_mean 6.5e-08 / 6.5e-08   running_var 2.6e-07 / 2.6e-07
    fp32  c=7    n=65       o 3.1e-07 / 4.1e-07   dx 3.2e-07 / 2.5e-07   dgamma 1.3e-06 / 1.3e-06   dbeta 2.4e-06 / 1.5e-06
    fp32  c=1    n=333 (no residual)   o 3.9e-07 / 1.9e-07   dx 2.6e-07 / 1.3e-07   dgamma 5.2e-06 / 2.5e-06   dbeta 4.9e-07 / 4.9e-07
    fp32  c=1024 n=3        o 8.1e-07 / 2.3e-06   dx 8.4e-06 / 1.6e-05   dgamma 8.9e-07 / 3.7e-06   dbeta 2.4e-07 / 2.4e-07
    fp32  c=48   n=333 misaligned   o 6.4e-07 / 4.6e-07   dx 3.6e-07 / 3.6e-07   dgamma 1.2e-05 / 1.3e-05   dbeta 6.8e-06 / 9.6e-06
    fp32  c=100  n=333 (25 chunks in a 32-lane segment)   o 5.8e-07 / 5.9e-07   dx 4.0e-07 / 4.0e-07   dgamma 1.6e-05 / 1.9e-05   dbeta 8.0e-06 / 8.7e-06
    fp32  c=96   n=333 misaligned (16 channels a lane)  o 6.8e-07 / 8.1e-07   dx 4.2e-07 / 4.7e-07   dgamma 1.4e-05 / 1.7e-05   dbeta 9.7e-06 / 9.2e-06
    fp32  c=48   n=400000   o 1.1e-06 / 1.0e-06   dx 6.8e-07 / 5.6e-07   dgamma 1.4e-02 / 2.0e-02   dbeta 8.2e-03 / 7.4e-03   (sums of about 1e5)
    f16   c=48   n=333      o 1.9e-03 / 2.8e-03   dx 1.9e-03 / 1.9e-03   dgamma 1.0e-05 / 1.5e-03   dbeta 9.2e-06 / 1.1e-03
    bf16  c=48   n=333      o 1.5e-02 / 2.0e-02   dx 9.9e-03 / 9.9e-03   dgamma 1.0e-05 / 9.5e-03   dbeta 6.9e-06 / 1.0e-02
    (half rows: torch rounds the normalised rows and the activation's gradient to the half type between its kernels, the fused passes do not)
    eval  c=48   n=333 relu o 6.2e-07 / 5.3e-07   dx 2.8e-07 / 2.8e-07   dgamma 1.6e-05 / 1.6e-05   dbeta 9.2e-06 / 6.4e-06
    hard columns, constant        o 0 / 0               dx 6.7e-05 / 1.4e-04   dgamma 0 / 0   running_var 1.4e-08 / 1.4e-08
    hard columns, 1e3 + N(0, 1)   o 1.3e-05 / 1.3e-05   dx 6.6e-06 / 1.6e-05   dgamma 6.4e-04 / 4.3e-04   running_var 7.3e-08 / 1.7e-07   (variance 1.044450 for 1.044457)
    stem + heads fp32: |fused - unfused| <= 1.3e-04 on gradients of magnitude 179 (stem_layer.0.kpconv.weight), i.e. 7e-07 of the scale; outputs 1.2e-06 of 2.8;
    the two zero-gradient biases 8.6e-06 and 5.0e-06 against weight-gradient scales of 111 and 33
    heads autocast(f16): fused and unfused equally far from float64 (classes 1.65e-03 both, classifier.0.weight's gradient 4.31 of 111 both:
    the f16 rounding of the Linear's output in front of the norm, which both sides read)
Every test prints its figures.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stratified_transformer_amd import scene
from tests import batchnorm_oracle as O
from tests import stem_standin as S
from tests.util import dev

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SLOPE = 0.2
KINK = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _f64(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _oracle(p, mode, with_grad=True):
    return O.batch_norm_act(_f64(p["x"]), _f64(p["gamma"]), _f64(p["beta"]), _f64(p["go"]) if with_grad else None,
                            _f64(p["rm"]) if mode["running"] else None, _f64(p["rv"]) if mode["running"] else None, mode["training"],
                            mode["momentum"], 1e-5, p["act"], SLOPE, _f64(p["res"]))


def _mode(training=True, running=True, momentum=0.02):
    return dict(training=training, running=running, momentum=momentum)


def _inputs(n, c, xname, rname, act, seed, mode=None, misaligned=False):
    """host tensors of one case; rname: the residual's type or None; misaligned: every [n, c] operand is a contiguous view one element into
    its buffer (made on the GPU by _to).  x is settled away from the activation's kink (module docstring)."""
    g = torch.Generator().manual_seed(seed)
    dt = DTYPES[xname]
    z = torch.randn(n, c, generator=g)
    p = dict(x=(0.3 + 1.5 * z).to(dt), go=(torch.randn(n, c, generator=g) + 0.25 + 0.25 * z).to(dt),   # (dO: module docstring)
             res=None if rname is None else torch.randn(n, c, generator=g).to(DTYPES[rname]), gamma=1 + 0.2 * torch.randn(c, generator=g),
             beta=0.2 * torch.randn(c, generator=g), rm=0.3 + 0.1 * torch.randn(c, generator=g), rv=2.0 + 0.5 * torch.rand(c, generator=g),
             act=act, misaligned=misaligned)
    return _settle(p, mode or _mode())


def _settle(p, mode):
    if p["act"] not in ("relu", "leaky_relu") or p["x"].shape[0] == 0:
        return p
    for _ in range(20):
        x64, gamma, beta = _f64(p["x"]), _f64(p["gamma"]), _f64(p["beta"])
        with np.errstate(all="ignore"):
            batch = mode["training"] or not mode["running"]
            mean, var = (x64.mean(0), x64.var(0)) if batch else (_f64(p["rm"]), _f64(p["rv"]))
            pre = (x64 - mean) / np.sqrt(var + 1e-5) * gamma + beta
            bad = np.abs(pre) < KINK
        if not bad.any():
            return p
        p["x"] = (p["x"].float() + 0.125 * torch.from_numpy(bad).float()).to(p["x"].dtype)
    raise AssertionError("the inputs did not settle away from the kink")


def _to(t, misaligned=False):
    if t is None:
        return None
    if not misaligned or t.dim() != 2:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _leaves(p, need, mis=False):
    x, res = _to(p["x"], mis), _to(p["res"], mis)
    w, b = p["gamma"].cuda(), p["beta"].cuda()
    for t, flag in ((x, need[0]), (w, need[1]), (b, need[1]), (res, need[2])):
        if t is not None:
            t.requires_grad_(flag)
    return x, w, b, res, p["rm"].cuda(), p["rv"].cuda()


def _results(o, x, w, b, res, rm, rv, mode):
    return dict(o=o.detach(), dx=x.grad, dgamma=w.grad, dbeta=b.grad, dresidual=None if res is None else res.grad,
                running_mean=rm if mode["running"] else None, running_var=rv if mode["running"] else None)


def _fused(P, p, mode, need=(True, True, True), backward=True):
    x, w, b, res, rm, rv = _leaves(p, need, p["misaligned"])
    o = P.batch_norm_act(x, w, b, rm if mode["running"] else None, rv if mode["running"] else None, mode["training"], mode["momentum"], 1e-5,
                         p["act"], SLOPE, res)
    if backward and o.requires_grad:
        o.backward(_to(p["go"], p["misaligned"]))
    torch.cuda.synchronize()
    return _results(o, x, w, b, res, rm, rv, mode)


def _torch_act(pre, act):
    return {"none": lambda t: t, "relu": F.relu, "leaky_relu": lambda t: F.leaky_relu(t, SLOPE), "tanh": torch.tanh}[act](pre)


def _composite(p, mode):
    """what the parent's model runs at one site: F.batch_norm in the rows' dtype, the activation, the add - which the model does in place
    on the rows (`feats += shortcut`), so its sum is rounded to their type"""
    x, w, b, res, rm, rv = _leaves(p, (True, True, True))
    have = mode["running"]
    pre = F.batch_norm(x, rm if have else None, rv if have else None, w, b, mode["training"] or not have, mode["momentum"], 1e-5)
    o = _torch_act(pre, p["act"])
    if res is not None:
        o = (o + res).to(x.dtype)
    o.backward(p["go"].cuda())
    torch.cuda.synchronize()
    return _results(o, x, w, b, res, rm, rv, mode)


def _check(P, p, label, mode=None):
    mode = mode or _mode()
    want, got, comp = _oracle(p, mode), _fused(P, p, mode), _composite(p, mode)
    n, c = p["x"].shape
    dt = p["x"].dtype
    assert got["o"].dtype == dt and got["dx"].dtype == dt and tuple(got["o"].shape) == tuple(got["dx"].shape) == (n, c)
    assert got["dgamma"].dtype == got["dbeta"].dtype == torch.float32 and tuple(got["dgamma"].shape) == tuple(got["dbeta"].shape) == (c,)
    if p["res"] is not None:
        assert got["dresidual"].dtype == p["res"].dtype and torch.equal(_bits(got["dresidual"]), _bits(p["go"].cuda().to(p["res"].dtype)))
    figures, ok = [], True
    for name in ("o", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
        if want[name] is None:
            assert got[name] is None, name
            continue
        u = U[dt] if name in ("o", "dx") else U[torch.float32]
        e_f = float(np.abs(_f64(got[name]) - want[name]).max(initial=0.0))
        e_c = float(np.abs(_f64(comp[name]) - want[name]).max(initial=0.0))
        top = float(np.abs(want[name]).max(initial=0.0))
        figures.append(f"{name} {e_f:.2e}/{e_c:.2e}")
        ok = ok and e_f <= 4 * e_c + u * top
    print(f"batch_norm_act {label}: " + "  ".join(figures) + ("" if ok else "   <-- over the bar"))
    assert ok
    if mode["running"] and not mode["training"]:
        assert torch.equal(got["running_mean"], p["rm"].cuda()) and torch.equal(got["running_var"], p["rv"].cuda())   # eval updates nothing
    return got


FP32_CASES = [(c, n, False) for c in (12, 48, 96, 384) for n in (2, 5, 333, 4099)] + [(7, 65, False), (1, 333, False), (1024, 3, False), (48, 333, True),
                                                                                          (100, 333, False), (96, 333, True), (70, 333, False)]
# (7 and 1: one channel a lane in a segment; 100: 25 chunks in a 32-lane segment; 96 misaligned and 70: one channel a lane, 16 a lane -
# tests/row_lanes_cases.py restates the choice, tests/test_row_lanes_hip.py runs every instance and segment width)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("c,n,misaligned", FP32_CASES)
def test_training_fp32(P, c, n, misaligned, with_res):
    p = _inputs(n, c, "f32", "f32" if with_res else None, "leaky_relu", seed=c + n, misaligned=misaligned)
    _check(P, p, f"fp32 c={c} n={n} leaky_relu residual={'f32' if with_res else 'None'}{' misaligned' if misaligned else ''}")


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("act", O.ACTS)
def test_training_fp32_activations(P, act, with_res):
    p = _inputs(333, 48, "f32", "f32" if with_res else None, act, seed=17)
    _check(P, p, f"fp32 c=48 n=333 {act} residual={'f32' if with_res else 'None'}", _mode(momentum=0.1))


@pytest.mark.parametrize("same_type_res", [False, True])
@pytest.mark.parametrize("name", ["f16", "bf16"])
@pytest.mark.parametrize("c,n", [(12, 333), (48, 333)])
def test_half_rows(P, c, n, name, same_type_res):
    """the residual in fp32 (the stem under autocast adds the fp32 shortcut to half rows) and in the rows' own type"""
    rname = name if same_type_res else "f32"
    p = _inputs(n, c, name, rname, "leaky_relu", seed=c + n + 1)
    _check(P, p, f"{name} c={c} n={n} leaky_relu residual={rname}")


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("c,n", [(48, 333), (12, 4099)])
def test_eval_mode(P, c, n, act):
    mode = _mode(training=False)
    p = _inputs(n, c, "f32", "f32", act, seed=c + n + 2, mode=mode)
    checked = _check(P, p, f"eval fp32 c={c} n={n} {act}", mode)
    with torch.no_grad():                                                                  # nothing is saved: the same pass, the same bits
        got = _fused(P, p, mode, backward=False)
    want = _oracle(p, mode, with_grad=False)
    err, top = float(np.abs(_f64(got["o"]) - want["o"]).max()), float(np.abs(want["o"]).max())
    print(f"batch_norm_act eval under no_grad c={c} n={n} {act}: o {err:.2e} (max {top:.2f})")
    assert got["dx"] is None and torch.equal(_bits(got["o"]), _bits(checked["o"]))         # (which _check held against the oracle)


@pytest.mark.parametrize("training", [True, False])
def test_without_running_statistics(P, training):
    """running_mean=None: batch statistics in both modes, nothing to update"""
    mode = _mode(training=training, running=False)
    p = _inputs(333, 48, "f32", None, "leaky_relu", seed=23, mode=mode)
    _check(P, p, f"fp32 c=48 n=333 no running statistics, training={training}", mode)


def test_grid_stride(P):
    """400 000 rows of 48 channels: 25 000 workgroups' worth of rows, past the row passes' cap of num_cus() * 64 and the reductions' 1024"""
    p = _inputs(400000, 48, "f32", "f32", "leaky_relu", seed=2)
    _check(P, p, "fp32 c=48 n=400000 leaky_relu residual=f32")


def test_without_rows(P):
    x = torch.zeros(0, 48, device="cuda", dtype=torch.float16, requires_grad=True)
    w, b = torch.ones(48, device="cuda", requires_grad=True), torch.zeros(48, device="cuda", requires_grad=True)
    rm, rv = torch.full((48,), 0.25, device="cuda"), torch.full((48,), 2.0, device="cuda")
    res = torch.zeros(0, 48, device="cuda", requires_grad=True)
    for training in (True, False):
        o = P.batch_norm_act(x, w, b, rm, rv, training, 0.1, 1e-5, "relu", 0.0, res)
        assert tuple(o.shape) == (0, 48) and o.dtype == torch.float16
        o.float().sum().backward()
        assert tuple(x.grad.shape) == (0, 48) and x.grad.dtype == torch.float16 and tuple(res.grad.shape) == (0, 48)
        assert float(w.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0
    assert float((rm - 0.25).abs().max()) == 0.0 and float((rv - 2.0).abs().max()) == 0.0


def test_two_runs_give_the_same_bits(P):
    for name in ("f32", "f16"):
        p = _inputs(4099, 48, name, "f32", "leaky_relu", seed=3)
        a, b = _fused(P, p, _mode()), _fused(P, p, _mode())
        for key in a:
            assert torch.equal(_bits(a[key]), _bits(b[key])), (name, key)


def test_hard_columns(P):
    """C = 48, N = 333: a constant column (variance 0), a column of 1e3 + N(0, 1) (E[x^2] - mean^2 in fp32 gives 1.125 for its variance of
    1.0445 and fails the bar), a column holding one NaN and a column holding +Inf - each column against the oracle, the poison confined to
    its column"""
    n, c, mode = 333, 48, _mode()
    p = _inputs(n, c, "f32", None, "leaky_relu", seed=21)
    p["x"][:, 0], p["beta"][0] = 1.5, 0.3
    p["x"][:, 1] = 1e3 + torch.randn(n, generator=torch.Generator().manual_seed(1))
    p = _settle(p, mode)
    clean = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in p.items()}
    p["x"][40, 4] = float("nan")
    p["x"][7, 9] = float("inf")
    want, got, comp, ref = _oracle(p, mode), _fused(P, p, mode), _composite(p, mode), _fused(P, clean, mode)
    cols = [k for k in range(c) if k not in (4, 9)]
    for name in ("o", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
        g, w = _f64(got[name]), want[name]
        assert np.array_equal(np.isfinite(g), np.isfinite(w)), name                        # the oracle's set of non-finite entries
        assert np.isfinite(w[..., cols]).all(), name
        if name != "dbeta":                                                                # (leaky_relu's derivative of a NaN is its slope: dbeta stays finite)
            assert not np.isfinite(w[..., [4, 9]]).any(), name
        assert torch.equal(_bits(got[name][..., cols]), _bits(ref[name][..., cols])), name  # the other columns: as without the poison
    for k, what in ((0, "constant"), (1, "1e3 + N(0,1)")):
        figures = []
        for name in ("o", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
            e_f, e_c = (float(np.abs(_f64(t[name])[..., k] - want[name][..., k]).max()) for t in (got, comp))
            top = float(np.abs(want[name][..., k]).max())
            figures.append(f"{name} {e_f:.2e}/{e_c:.2e}")
            assert e_f <= 4 * e_c + U[torch.float32] * top, (what, name, e_f, e_c, top)
        print(f"batch_norm_act hard columns, {what}: " + "  ".join(figures))
    assert float((got["o"][:, 0] - 0.3).abs().max()) == 0.0                                # variance 0: o is act(beta), exactly
    keep = np.float32(1.0) - np.float32(mode["momentum"])
    assert float(got["running_var"][0]) == float(keep * np.float32(float(p["rv"][0])))     # and M2 is exactly 0
    var1 = float(1.0 / got_rstd(P, p["x"][:, 1:2]) ** 2 - 1e-5)
    print(f"batch_norm_act hard columns, variance of the 1e3 + N(0,1) column: {var1:.6f} (float64: {float(_f64(p['x'][:, 1]).var()):.6f})")
    assert abs(var1 - float(_f64(p["x"][:, 1]).var())) <= 1e-3


def got_rstd(P, column):
    """rstd of one column, read from the statistics launcher through the binding"""
    from stratified_transformer_amd import pointops2_cuda as C
    x = column.contiguous().cuda()
    stat = torch.empty(2, 1, device="cuda")
    C.batch_norm_act_stats(x.shape[0], 1, x, torch.empty(84, 3, 1, device="cuda"), 1e-5, 0.0, None, None, stat)
    return float(stat[1, 0])


def test_no_work_for_absent_gradients(P, monkeypatch):
    """counted through the binding: (the parameter sums ran, dx ran) per backward call.  With batch statistics dx reads the two sums, so
    frozen parameters spare them only where the running statistics normalise (eval mode)."""
    from stratified_transformer_amd import pointops2_cuda as C
    calls, real = [], C.batch_norm_act_backward

    def counting(n, c, x, grad_o, stat, weight, bias, act, slope, training, partials, grad_weight, grad_bias, grad_x, **kw):
        calls.append((partials is not None, grad_x is not None))
        return real(n, c, x, grad_o, stat, weight, bias, act, slope, training, partials, grad_weight, grad_bias, grad_x, **kw)

    monkeypatch.setattr(C, "batch_norm_act_backward", counting)
    train, evalm = _mode(), _mode(training=False)
    p = _inputs(333, 48, "f32", "f32", "leaky_relu", seed=31)
    want = _oracle(p, train)
    got = _fused(P, p, train, need=(False, True, False))
    assert calls == [(True, False)] and got["dx"] is None and got["dresidual"] is None
    assert float(np.abs(_f64(got["dgamma"]) - want["dgamma"]).max()) <= 1e-4 * float(np.abs(want["dgamma"]).max())
    del calls[:]
    got = _fused(P, p, train, need=(True, False, False))
    assert calls == [(True, True)] and got["dgamma"] is None and got["dbeta"] is None
    assert float(np.abs(_f64(got["dx"]) - want["dx"]).max()) <= 1e-4 * float(np.abs(want["dx"]).max())
    del calls[:]
    pe = _inputs(333, 48, "f32", "f32", "leaky_relu", seed=31, mode=evalm)
    want = _oracle(pe, evalm)
    got = _fused(P, pe, evalm, need=(True, False, False))
    assert calls == [(False, True)] and got["dgamma"] is None
    assert float(np.abs(_f64(got["dx"]) - want["dx"]).max()) <= 1e-5 * float(np.abs(want["dx"]).max())
    del calls[:]
    got = _fused(P, p, train, need=(False, False, True))                                   # the residual alone: no kernel at all
    assert calls == [] and got["dx"] is None and torch.equal(got["dresidual"], p["go"].cuda())
    got = _fused(P, p, train, need=(False, False, False))
    assert calls == [] and not got["o"].requires_grad


# ---- the model's composition ----
def _room(P):
    xyz, offset = scene.make_batch([1400], seed=9)
    nb, _ = P.ball_query(2.5 * S.GRID, 34, dev(xyz), dev(xyz), dev(offset), dev(offset))
    return dev(xyz), nb.contiguous()


def _run_model(model, feats, xyz, nb, go, amp=False):
    model.zero_grad(set_to_none=True)
    leaf = feats.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        cls, reg = model(leaf, xyz, None, nb)
    torch.autograd.backward([cls, reg], [go[0].to(cls.dtype), go[1].to(reg.dtype)])
    torch.cuda.synchronize()
    named = dict(classes=cls.detach(), shifts=reg.detach(), input_gradient=leaf.grad)
    named.update({"grad " + k: q.grad for k, q in sorted(model.named_parameters()) if q.grad is not None})
    named.update({k: b.detach().clone() for k, b in sorted(model.named_buffers())})
    return named


def _smallest_pre(model, feats, xyz, nb):
    """the smallest |pre-activation| in front of a relu / leaky_relu over the sites of an unfused forward (of a copy: the statistics move)"""
    probe, seen = copy.deepcopy(model), []
    kinked = [probe.stem_layer[0].bn.batch_norm, probe.stem_layer[1].unary_1[1].batch_norm, probe.stem_layer[1].unary_2[1].batch_norm, probe.classifier[1]]
    hooks = [m.register_forward_hook(lambda _m, _i, out: seen.append(float(out.abs().min()))) for m in kinked]
    with torch.no_grad():
        probe(feats, xyz, None, nb)
    for h in hooks:
        h.remove()
    assert len(seen) == 4
    return min(seen)


def _model_problem(P):
    xyz, nb = _room(P)
    n = xyz.shape[0]
    for seed in range(64):
        torch.manual_seed(seed)
        model = S.shake_norms(S.StemHeads(S.kp_conv), seed + 100).cuda().train()
        g = torch.Generator().manual_seed(seed + 200)
        feats = torch.rand(n, 3, generator=g).cuda()
        go = (torch.randn(n, 19, generator=g).cuda(), torch.randn(n, 3, generator=g).cuda())
        if _smallest_pre(model, feats, xyz, nb) >= 1e-5:
            print(f"stem + heads: seed {seed}, {n} points")
            return model, feats, xyz, nb, go
    raise AssertionError("no seed keeps every pre-activation away from the kink")


def test_stem_and_heads_fp32(P, monkeypatch):
    from stratified_transformer_amd import layers
    model, feats, xyz, nb, go = _model_problem(P)
    assert 1300 <= feats.shape[0] <= 1500
    plain, fused, back = copy.deepcopy(model), copy.deepcopy(model), copy.deepcopy(model)
    off = _run_model(plain, feats, xyz, nb, go)
    calls, real = [], P.batch_norm_act
    monkeypatch.setattr(P, "batch_norm_act", lambda x, w, b, rm, rv, training, momentum, eps, act, slope, residual: (
        calls.append((act, slope, residual is not None, momentum, training)), real(x, w, b, rm, rv, training, momentum, eps, act, slope, residual))[1])
    assert layers.fuse_batch_norms(fused) == ["stem_layer.0", "stem_layer.1.unary_1", "stem_layer.1.unary_2", "classifier", "regressor"]
    on = _run_model(fused, feats, xyz, nb, go)
    assert calls == [("leaky_relu", 0.2, False, 0.02, True), ("leaky_relu", 0.2, False, 0.02, True), ("leaky_relu", 0.2, True, 0.02, True),
                     ("relu", 0.0, False, 0.1, True), ("tanh", 0.0, False, 0.1, True)]
    assert set(on) == set(off) and len(on) == 3 + 22 + 18               # results, parameter gradients, buffers
    # Each tensor against its own scale.  The one exception, by name: the bias of a Linear directly in front of a training-mode BatchNorm has a
    # gradient of exactly 0 (the norm subtracts the mean), so either side holds only the rounding noise of a sum over the rows and the
    # tensor has no scale of its own; these two are held to an absolute 1e-4 of the scale of the same Linear's weight gradient, whose
    # terms the sum shares.
    zero = {"grad classifier.0.bias": "grad classifier.0.weight", "grad regressor.0.bias": "grad regressor.0.weight"}

    def scale_of(name):
        return max(float(off[zero.get(name, name)].abs().max()), 1e-6)

    assert all(float(off[name].abs().max()) <= 1e-5 * scale_of(name) for name in zero)   # (they are noise, on the unfused side too)
    worst = 0.0
    for name in off:
        if name.endswith("num_batches_tracked"):
            assert torch.equal(on[name], off[name]), name
            continue
        diff, top = float((on[name] - off[name]).abs().max()), scale_of(name)
        print(f"stem + heads fp32 {name}: |fused - unfused| {diff:.2e} (scale {top:.2f}{', of ' + zero[name] if name in zero else ''})")
        worst = max(worst, diff / top)
    assert worst <= 1e-4
    # unfused again: the unfused bits return.  The convolution's backward adds its input gradient with float atomics (csrc/kpconv.hip), so
    # what lies upstream of stem_layer.1.kpconv's input - the input gradient, stem_layer.0's and unary_1's gradients - differs from run to
    # run of the unfused model itself and is compared by value; everything else bit for bit.
    del calls[:]
    layers.fuse_batch_norms(back)
    layers.unfuse_batch_norms(back)
    again = _run_model(back, feats, xyz, nb, go)
    assert calls == [] and not any("forward" in m.__dict__ for m in back.modules())
    for name in off:
        if name == "input_gradient" or name.startswith(("grad stem_layer.0.", "grad stem_layer.1.unary_1.")):
            assert float((again[name] - off[name]).abs().max()) <= 1e-5 * scale_of(name), name
        else:
            assert torch.equal(again[name], off[name]), name


def _heads64(heads, feats, go):
    """classifier and regressor in float64 on the CPU -> outputs, the input gradient, the parameter gradients"""
    h64 = copy.deepcopy(heads).double().cpu().train()
    leaf = feats.detach().double().cpu().requires_grad_(True)
    cls, reg = h64[0](leaf), h64[1](leaf)
    torch.autograd.backward([cls, reg], [go[0].double().cpu(), go[1].double().cpu()])
    named = dict(classes=cls.detach(), shifts=reg.detach(), input_gradient=leaf.grad)
    named.update({"grad " + k: q.grad for k, q in sorted(h64.named_parameters())})
    named.update({k: b.detach().clone() for k, b in sorted(h64.named_buffers()) if not k.endswith("num_batches_tracked")})
    return named


def test_stem_and_heads_autocast(P, monkeypatch):
    """autocast(f16): the whole stand-in runs fused (half rows, the fp32 shortcut as the residual); the heads, on the unfused stem's output,
    against themselves in float64 on the CPU"""
    from stratified_transformer_amd import layers
    model, feats, xyz, nb, go = _model_problem(P)
    plain, fused = copy.deepcopy(model), copy.deepcopy(model)
    off = _run_model(plain, feats, xyz, nb, go, amp=True)
    calls, real = [], P.batch_norm_act
    monkeypatch.setattr(P, "batch_norm_act", lambda x, w, b, rm, rv, training, momentum, eps, act, slope, residual: (
        calls.append((act, x.dtype, None if residual is None else residual.dtype)), real(x, w, b, rm, rv, training, momentum, eps, act, slope, residual))[1])
    layers.fuse_batch_norms(fused)
    on = _run_model(fused, feats, xyz, nb, go, amp=True)
    h, f = torch.float16, torch.float32
    assert [c[0] for c in calls] == ["leaky_relu", "leaky_relu", "leaky_relu", "relu", "tanh"]
    assert [c[1] for c in calls[1:]] == [h, h, h, h] and calls[2][2] in (h, f) and all(c[2] is None for c in calls[:2] + calls[3:])
    for name in off:
        assert on[name].dtype == off[name].dtype and bool(torch.isfinite(on[name]).all()), name
        diff, top = float((on[name].float() - off[name].float()).abs().max()), max(float(off[name].float().abs().max()), 1e-6)
        print(f"stem + heads autocast(f16) {name}: |fused - unfused| {diff:.2e} (max {top:.2f})")
    # the heads alone, both ways on the same rows, against float64
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        rows = feats
        for layer in copy.deepcopy(model).stem_layer:
            rows = layer(rows, xyz, None, nb)
    rows = rows.float()
    heads = torch.nn.ModuleList([model.classifier, model.regressor])
    want = _heads64(heads, rows, go)
    runs = {}
    for which in ("fused", "unfused"):
        hd = copy.deepcopy(heads).train()
        if which == "fused":
            assert layers.fuse_batch_norms(hd) == ["0", "1"]
        leaf = rows.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            cls, reg = hd[0](leaf), hd[1](leaf)
        torch.autograd.backward([cls, reg], [go[0].to(cls.dtype), go[1].to(reg.dtype)])
        named = dict(classes=cls.detach(), shifts=reg.detach(), input_gradient=leaf.grad)
        named.update({"grad " + k: q.grad for k, q in sorted(hd.named_parameters())})
        named.update({k: b.detach().clone() for k, b in sorted(hd.named_buffers()) if not k.endswith("num_batches_tracked")})
        runs[which] = named
    worst = 0.0
    for name, w in want.items():
        e_on, e_off = (float((runs[k][name].double().cpu() - w).abs().max()) for k in ("fused", "unfused"))
        top = float(w.abs().max())
        print(f"heads autocast(f16) {name}: err fused {e_on:.2e} unfused {e_off:.2e} (max {top:.2f})")
        worst = max(worst, e_on - (4 * e_off + U[runs['fused'][name].dtype] * top))
    assert worst <= 0.0
