"""CPU: the declarations of pointops.segmentation_loss (the pinned C ABI table, signatures, exports, argument checks, the missing
CPU path) and its float64 oracle (tests/loss_oracle.py) against torch's float64 autograd, the reference's smoothed formula and
evaluate.intersection_and_union.  No HIP compute runs here."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, evaluate, pointops, pointops2_cuda
from tests import loss_oracle as O

def test_launchers_are_declared_and_exported():
    I, P, Q, Fl = _lib.I, _lib.P, _lib.Q, _lib.F
    assert _lib.SIGNATURES["seg_loss_forward_launcher"] == [I] * 4 + [P] * 4 + [Q, Fl, Fl] + [P] * 2 + [I] + [P] * 3
    assert _lib.SIGNATURES["seg_loss_backward_launcher"] == [I] * 4 + [P] * 7 + [Q, Fl, Fl] + [P] * 2


def test_public_signatures_and_exports():
    assert str(inspect.signature(pointops.segmentation_loss)) == \
        "(logits, target, shift_pred=None, shift=None, *, ignore_index=-100, offset_weight=1.0, smooth_eps=0.0)"
    assert issubclass(pointops.SegmentationLoss, torch.autograd.Function)
    assert sta.segmentation_loss is pointops.segmentation_loss and "segmentation_loss" in sta.__all__
    from lib.pointops2.functions import pointops as drop_in
    assert drop_in.segmentation_loss is pointops.segmentation_loss and drop_in.SegmentationLoss is pointops.SegmentationLoss
    for fn in (pointops2_cuda.seg_loss_forward, pointops2_cuda.seg_loss_backward):
        opts = inspect.signature(fn).parameters["opts"]
        assert opts.kind is inspect.Parameter.KEYWORD_ONLY and opts.default is None


def test_cpu_tensors_raise_no_cpu_fallback():
    x, t, sp, s = torch.rand(6, 5), torch.zeros(6, dtype=torch.int64), torch.rand(6, 3), torch.rand(6, 3)
    with pytest.raises(RuntimeError, match="segmentation_loss: logits: .*no CPU fallback"):
        pointops.segmentation_loss(x, t, sp, s)
    with pytest.raises(RuntimeError, match="segmentation_loss: target: .*no CPU fallback"):
        pointops.segmentation_loss(_OnGpu(x), t)
    with pytest.raises(RuntimeError, match="segmentation_loss: shift: .*no CPU fallback"):
        pointops.segmentation_loss(_OnGpu(x), _OnGpu(t), _OnGpu(sp), s)
    stat, partials, counts, rows, losses = torch.empty(6, 2), torch.empty(1, 2, dtype=torch.float64), torch.zeros(3, 5, dtype=torch.int64), \
        torch.zeros(2, dtype=torch.int64), torch.empty(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.seg_loss_forward(6, 5, x, t, sp, s, -100, 0.0, 1.0, stat, partials, counts, rows, losses)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointops2_cuda.seg_loss_backward(6, 5, x, t, stat, sp, s, torch.ones(3), rows, -100, 0.0, 1.0, torch.empty(6, 5), torch.empty(6, 3))


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t, device=None):
        self._t = t
        if device is not None:
            self.device = torch.device(device)

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _g(t):
    return None if t is None else _OnGpu(t)


_X, _T, _SP, _S = torch.rand(6, 5), torch.zeros(6, dtype=torch.int64), torch.rand(6, 3), torch.rand(6, 3)


@pytest.mark.parametrize("x,t,sp,s,kw,error,names", [
    (torch.rand(30), _T, None, None, {}, ValueError, r"logits: must be \[n, C\]"),
    (torch.rand(6, 5).double(), _T, None, None, {}, TypeError, "logits: must be f32, f16 or bf16"),
    (torch.rand(6, 65), _T, None, None, {}, ValueError, "logits: C must be in"),                            # C = 65
    (torch.rand(6, 0), _T, None, None, {}, ValueError, "logits: C must be in"),                             # C = 0
    (_X, _T.int(), None, None, {}, TypeError, "target: must be int64"),
    (_X, torch.zeros(5, dtype=torch.int64), None, None, {}, ValueError, "target: must be"),
    (_X, torch.zeros(6, 1, dtype=torch.int64), None, None, {}, ValueError, "target: must be"),
    (_X, _T, _SP, None, {}, ValueError, "shift_pred: given without shift"),
    (_X, _T, None, _S, {}, ValueError, "shift: given without shift_pred"),
    (_X, _T, _SP.double(), _S, {}, TypeError, "shift_pred: must be f32, f16 or bf16"),
    (_X, _T, _SP, _S.half(), {}, TypeError, "shift: must be f32"),
    (_X, _T, torch.rand(6, 4), _S, {}, ValueError, "shift_pred: must be"),
    (_X, _T, _SP, torch.rand(5, 3), {}, ValueError, "shift: must be"),
    (torch.rand(5, 6).t(), _T, None, None, {}, ValueError, "logits: must be contiguous"),
    (_X, torch.zeros(12, dtype=torch.int64)[::2], None, None, {}, ValueError, "target: must be contiguous"),
    (_X, _T, torch.rand(6, 6)[:, ::2], _S, {}, ValueError, "shift_pred: must be contiguous"),
    (_X, _T, _SP, torch.rand(3, 6).t(), {}, ValueError, "shift: must be contiguous"),
    (_X, _T, None, None, dict(smooth_eps=-0.1), ValueError, "smooth_eps: must be in"),
    (_X, _T, None, None, dict(smooth_eps=1.0), ValueError, "smooth_eps: must be in"),
    (torch.rand(6, 1), _T, None, None, dict(smooth_eps=0.1), ValueError, "smooth_eps: .* needs C >= 2"),
])
def test_operator_rejects_bad_arguments(x, t, sp, s, kw, error, names):
    with pytest.raises(error, match="segmentation_loss: " + names):
        pointops.segmentation_loss(_g(x), _g(t), _g(sp), _g(s), **kw)


@pytest.mark.parametrize("name", ["target", "shift_pred", "shift"])
def test_operator_rejects_tensors_on_another_device(name):
    args = dict(logits=_OnGpu(_X, "cuda:0"), target=_OnGpu(_T, "cuda:0"), shift_pred=_OnGpu(_SP, "cuda:0"), shift=_OnGpu(_S, "cuda:0"))
    args[name] = _OnGpu(args[name]._t, "cuda:1")
    with pytest.raises(RuntimeError, match=f"segmentation_loss: {name}: is on cuda:1, logits on cuda:0"):
        pointops.segmentation_loss(**args)


def test_binding_rejects_bad_shapes_and_dtypes():
    C = pointops2_cuda
    f32 = lambda *s: _OnGpu(torch.zeros(*s))
    f16 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.float16))
    i64 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.int64))
    f64 = lambda *s: _OnGpu(torch.zeros(*s, dtype=torch.float64))
    ok = lambda: dict(n=6, c=5, logits=f16(6, 5), target=i64(6), shift_pred=f16(6, 3), shift=f32(6, 3), ignore_index=-100, smooth_eps=0.0,
                      offset_weight=1.0, stat=f32(6, 2), partials=f64(1, 2), counts=i64(3, 5), rows=i64(2), losses=f32(3))
    cases = [("c", ValueError, dict(c=65)), ("c", ValueError, dict(c=0)), ("n", ValueError, dict(n=-1)), ("smooth_eps", ValueError, dict(smooth_eps=1.0)),
             ("smooth_eps", ValueError, dict(smooth_eps=0.5, c=1, logits=f16(6, 1), counts=i64(3, 1))),
             ("logits", TypeError, dict(logits=f64(6, 5))), ("logits", ValueError, dict(logits=f16(5, 5))),
             ("logits", RuntimeError, dict(logits=_OnGpu(torch.zeros(5, 6).t()))), ("target", TypeError, dict(target=f32(6))),
             ("target", ValueError, dict(target=i64(7))), ("shift_pred", ValueError, dict(shift_pred=f16(6, 4))), ("shift", TypeError, dict(shift=f16(6, 3))),
             ("shift", ValueError, dict(shift=None)), ("shift_pred", ValueError, dict(shift_pred=None)), ("stat", ValueError, dict(stat=f32(6))),
             ("partials", TypeError, dict(partials=f32(1, 2))), ("partials", ValueError, dict(partials=f64(1025, 2))),
             ("partials", ValueError, dict(partials=f64(2))), ("counts", ValueError, dict(counts=i64(3, 4))), ("counts", TypeError, dict(counts=f32(3, 5))),
             ("rows", ValueError, dict(rows=i64(3))), ("losses", ValueError, dict(losses=f32(2)))]
    order = ("n", "c", "logits", "target", "shift_pred", "shift", "ignore_index", "smooth_eps", "offset_weight", "stat", "partials", "counts", "rows", "losses")
    for name, error, change in cases:
        kw = ok()
        kw.update(change)
        with pytest.raises(error, match=name):
            C.seg_loss_forward(*(kw[k] for k in order))
    okb = lambda: dict(n=6, c=5, logits=f16(6, 5), target=i64(6), stat=f32(6, 2), shift_pred=f32(6, 3), shift=f32(6, 3), grad_losses=f32(3), rows=i64(2),
                       ignore_index=-100, smooth_eps=0.0, offset_weight=1.0, grad_logits=f16(6, 5), grad_shift_pred=f32(6, 3))
    cases = [("grad_logits", TypeError, dict(grad_logits=f32(6, 5))), ("grad_logits", ValueError, dict(grad_logits=f16(6, 4))),
             ("grad_shift_pred", TypeError, dict(grad_shift_pred=f16(6, 3))), ("grad_shift_pred", ValueError, dict(shift_pred=None, shift=None)),
             ("grad_losses", ValueError, dict(grad_losses=f32(2))), ("grad_losses", TypeError, dict(grad_losses=f16(3))), ("rows", TypeError, dict(rows=f32(2))),
             ("stat", ValueError, dict(stat=f32(6, 1))), ("c", ValueError, dict(c=65))]
    order = ("n", "c", "logits", "target", "stat", "shift_pred", "shift", "grad_losses", "rows", "ignore_index", "smooth_eps", "offset_weight", "grad_logits",
             "grad_shift_pred")
    for name, error, change in cases:
        kw = okb()
        kw.update(change)
        with pytest.raises(error, match=name):
            C.seg_loss_backward(*(kw[k] for k in order))


def _case(n, c, seed, ignore_index=-100, ignored=0.1):
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(n, c, generator=g, dtype=torch.float64)
    t = torch.randint(0, c, (n,), generator=g)
    t[torch.rand(n, generator=g) < ignored] = ignore_index
    sp, s = torch.randn(n, 3, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g, dtype=torch.float64)
    sp[0, 0] = s[0, 0]                                                                     # sign(0) = 0
    return x, t, sp, s


def _close(got, want, name):
    want = np.asarray(want, np.float64)
    scale = max(1.0, float(np.abs(want).max(initial=0.0)))
    assert float(np.abs(np.asarray(got) - want).max(initial=0.0)) <= 1e-12 * scale, name


@pytest.mark.parametrize("n,c,offset_weight,grad_losses,ignore_index,with_shift", [
    (37, 13, 1.0, (0.0, 0.0, 1.0), -100, True), (64, 19, 0.5, (0.0, 0.0, 65536.0), 255, True), (5, 20, 2.0, (0.7, -1.3, 0.4), -100, True),
    (41, 2, 1.0, (1.0, 0.0, 0.0), -100, True), (33, 1, 3.0, (0.0, 1.0, 0.0), -100, True), (29, 64, 1.0, (0.3, 0.0, 1.1), 7, False)])
def test_oracle_is_torch_float64_autograd(n, c, offset_weight, grad_losses, ignore_index, with_shift):
    x, t, sp, s = _case(n, c, seed=n + c, ignore_index=ignore_index)
    xl, spl = x.clone().requires_grad_(True), sp.clone().requires_grad_(True)
    ce = F.cross_entropy(xl, t, ignore_index=ignore_index)
    l1 = F.l1_loss(spl, s) if with_shift else torch.zeros((), dtype=torch.float64)
    total = ce + offset_weight * l1 if with_shift else ce * 1.0
    losses = torch.stack([ce, l1, total])
    losses.backward(torch.tensor(grad_losses, dtype=torch.float64))
    got = O.segmentation_loss(x.numpy(), t.numpy(), sp.numpy() if with_shift else None, s.numpy() if with_shift else None, grad_losses,
                              ignore_index=ignore_index, offset_weight=offset_weight)
    _close(got["losses"], losses.detach().numpy(), "losses")
    _close(got["lse"], torch.logsumexp(x, 1).numpy(), "lse")
    _close(got["grad_logits"], xl.grad.numpy(), "grad_logits")
    if with_shift:
        _close(got["grad_shift_pred"], spl.grad.numpy(), "grad_shift_pred")
        assert got["grad_shift_pred"][0, 0] == 0.0
    else:
        assert got["grad_shift_pred"] is None and got["losses"][1] == 0.0 and got["losses"][2] == got["losses"][0]
    valid = (t != ignore_index).numpy()
    assert got["rows"].tolist() == [int(valid.sum()), 0] and not got["grad_logits"][~valid].any()


@pytest.mark.parametrize("n,c,eps", [(37, 19, 0.1), (12, 2, 0.3), (50, 13, 0.05)])
def test_oracle_smoothed_form_is_the_reference_formula(n, c, eps):
    x, t, _, _ = _case(n, c, seed=3 * n + c, ignored=0.0)
    xl = x.clone().requires_grad_(True)
    hot = F.one_hot(t, c).double()                                                          # util/common_util.py:180-185: its weighting, written out
    w = hot * (1 - eps) + (1 - hot) * (eps / (c - 1))
    loss = -(w * F.log_softmax(xl, dim=1)).sum(dim=1).mean()
    loss.backward()
    got = O.segmentation_loss(x.numpy(), t.numpy(), smooth_eps=eps)
    _close(got["losses"][0], loss.item(), "ce")
    _close(got["grad_logits"], xl.grad.numpy(), "grad_logits")
    assert got["losses"][2] == got["losses"][0] and got["rows"].tolist() == [n, 0]


@pytest.mark.parametrize("n,c,ignore_index", [(500, 13, -100), (500, 19, 255), (333, 20, -1), (64, 1, -100)])
def test_oracle_counts_are_intersection_and_union(n, c, ignore_index):
    x, t, _, _ = _case(n, c, seed=n + 7 * c, ignore_index=ignore_index, ignored=0.2)
    x[::3] = torch.round(x[::3])                                                           # ties: the first maximum is the prediction
    got = O.segmentation_loss(x.numpy(), t.numpy(), ignore_index=ignore_index)
    want = evaluate.intersection_and_union(torch.from_numpy(x.numpy().argmax(1)), t, c, ignore_index)
    for k in range(3):
        assert got["counts"][k].tolist() == want[k].tolist(), k
    assert got["counts"].dtype == np.int64 and got["counts"][2].sum() == got["rows"][0] == int((t != ignore_index).sum())


def test_oracle_argmax_takes_the_first_maximum_and_the_first_nan():
    x = np.zeros((3, 4))
    x[0] = [1.0, 2.0, 2.0, 0.0]
    x[1] = [0.0, np.nan, 5.0, np.nan]
    x[2] = [-np.inf, -np.inf, -np.inf, -np.inf]
    got = O.segmentation_loss(x, np.array([1, 1, 0]))
    assert got["counts"][0].tolist() == [1, 2, 0, 0] and got["counts"][1].tolist() == [1, 2, 0, 0] and got["counts"][2].tolist() == [1, 2, 0, 0]


@pytest.mark.parametrize("bad", [19, -1, 1000, -7])
def test_out_of_range_label_is_skipped_and_counted(bad):
    c = 19
    x, t, sp, s = _case(40, c, seed=9, ignored=0.1)
    t[11] = -100
    ignored = O.segmentation_loss(x.numpy(), t.numpy(), sp.numpy(), s.numpy(), (0.5, 0.25, 1.0))
    t[11] = bad
    got = O.segmentation_loss(x.numpy(), t.numpy(), sp.numpy(), s.numpy(), (0.5, 0.25, 1.0))
    assert got["rows"].tolist() == [ignored["rows"][0], 1] and ignored["rows"][1] == 0
    for name in ("losses", "lse", "counts", "grad_logits", "grad_shift_pred"):
        assert np.array_equal(got[name], ignored[name]), name
    assert not got["grad_logits"][11].any()
