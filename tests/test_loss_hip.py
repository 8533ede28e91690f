"""GPU (-m gpu): the fused training loss on csrc/seg_loss.hip - pointops.segmentation_loss: cross-entropy with an ignore label, L1 on the shift
head, their weighted sum, the IoU counts and both gradients - against the float64 oracle of tests/loss_oracle.py evaluated on the CPU on
the same inputs.

Bars.  err(.) = max |. - float64 oracle|; u = 2^-24 / 2^-11 / 2^-8 for f32 / f16 / bf16 outputs; "composite" = torch's own chain
(F.cross_entropy(ignore_index) on the logits widened to fp32 as autocast widens them, F.l1_loss, the weighted sum, autograd) run on the
GPU in the same test.
  grad_logits, grad_shift_pred:   err(fused) <= 4 * err(composite) + u * max|want|     (fp32 sums of one length in another order)
  ce, l1, total:                  the same form with u of f32
  counts, rows:                   equal to the oracle's
  end to end (two heads under autocast(f16) with a GradScaler): every parameter gradient and the input gradient under the first bar, u of f16
Rows that are not valid: grad_logits exactly 0.  Two runs: the same bits.  A label out of range (C and -1, with ignore_index = -100, the operator's
default; every other test ignores 255): counted in rows[1], everything else bit-identical to the run where it is ignore_index.  A NaN / Inf row: the oracle's set of non-finite gradient entries, every other row
bit-identical to the run without the poison.

Measured on one MI355X (max abs error against float64, fused / composite):
    fp32  C=13 n=4099      ce 2.1e-07 / 2.7e-07   l1 2.8e-08 / 2.8e-08   total 2.5e-07 / 2.2e-07   grad_logits 9.4e-11 / 6.4e-11   grad_shift_pred 1.2e-12 / 1.2e-12
    fp32  C=19 n=4099      ce 1.7e-07 / 3.1e-07   l1 6.0e-08 / 6.0e-08   total 2.0e-07 / 2.8e-07   grad_logits 1.3e-10 / 5.4e-11   grad_shift_pred 1.2e-12 / 1.2e-12
    fp32  C=20 n=4099      ce 8.8e-08 / 5.6e-07   l1 3.7e-09 / 1.2e-07   total 8.9e-08 / 5.7e-07   grad_logits 1.1e-10 / 5.9e-11   grad_shift_pred 1.2e-12 / 1.2e-12
    fp32  C=19 n=5         ce 1.9e-07 / 2.8e-07   l1 4.5e-08 / 7.4e-08   total 4.1e-07 / 6.8e-08   grad_logits 2.7e-08 / 1.6e-08   (total: within 4 * 6.8e-08 + 2^-24 * |total|)
    fp32  C=7  n=65        ce 9.3e-09 / 4.9e-07   total 2.1e-07 / 2.1e-07   grad_logits 1.7e-09 / 1.8e-09
    fp32  C=64 n=333       ce 4.9e-08 / 5.3e-07   total 3.2e-07 / 3.2e-07   grad_logits 1.2e-09 / 7.4e-10
    fp32  C=19 n=333 misaligned   ce 4.3e-08 / 4.3e-08   grad_logits 8.4e-10 / 7.4e-10   grad_shift_pred 7.3e-12 / 7.3e-12   (the aligned case's figures: same results)
    fp32  C=19 n=300000    ce 6.3e-08 / 6.3e-08   l1 4.2e-09 / 4.2e-09   grad_logits 1.9e-12 / 1.0e-12   grad_shift_pred 1.8e-14 / 1.8e-14
    f16   C=19 n=333       ce 5.1e-08 / 5.1e-08   grad_logits 9.4e-07 / 9.4e-07   grad_shift_pred 1.8e-07 / 1.8e-07   (with a loss scale of 65536: 9.5e-07 / 9.5e-07)
    bf16  C=19 n=333       ce 9.5e-08 / 9.5e-08   grad_logits 7.6e-06 / 7.6e-06   grad_shift_pred 7.8e-07 / 7.8e-07
    smooth_eps 0.1         ce 2.7e-07 / 2.7e-07   grad_logits 9.5e-10 / 7.5e-10
    ignore_index -100      ce 2.4e-07 / 2.4e-07   grad_logits 1.7e-09 / 1.0e-09   grad_shift_pred 1.8e-11 / 1.8e-11   (C=19 n=333, upstream (0.5, 0.25, 1))
    hard rows: saturated row 1.5e-09 / 1.5e-09, equal logits 5.3e-09 / 2.2e-09, 1e4 + N(0,1) 1.1e-09 / 1.1e-09, -inf beside the target 2.7e-09 / 2.7e-09
    lse rebuilt from stat (maximum + log-sum): 3.2e-07 on values up to 11.3
    two heads under autocast(f16), scale 65536: input gradient 2.5e-05 / 2.5e-05 (max 2.3e-04); cls.3.weight 9.9e-06 / 1.7e-05; cls.0.weight 3.9e-04 / 3.9e-04
    (max 1.1e-02); the shift head's parameters equal to the composite's in every printed digit
Every test prints its figures.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import loss_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
U = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
IGNORE = 255


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _f64(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _inputs(n, c, lname="f32", sname="f32", seed=0, ignored=0.1, shift=True, misaligned=False, eps=0.0, weight=0.5, ignore_index=IGNORE):
    """host tensors of one case; misaligned: every [n, *] operand is a contiguous view one element into its buffer (made on the GPU by _to)"""
    g = torch.Generator().manual_seed(seed)
    p = dict(x=(3.0 * torch.randn(n, c, generator=g)).to(DTYPES[lname]), t=torch.randint(0, c, (n,), generator=g))
    p["t"][torch.rand(n, generator=g) < ignored] = ignore_index
    if n and ignored < 1.0:
        p["t"][0] = c - 1                                                                   # one valid row at least
    p["sp"] = torch.randn(n, 3, generator=g).to(DTYPES[sname]) if shift else None
    p["s"] = torch.randn(n, 3, generator=g) if shift else None
    if shift and n:
        p["s"][0, 0] = p["sp"][0, 0].float()                                                # sign(0) = 0
    p.update(misaligned=misaligned, eps=eps, weight=weight, lname=lname, sname=sname, ignore=ignore_index)
    return p


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


def _call(P, p, x, sp):
    return P.segmentation_loss(x, p["t"].cuda(), sp, _to(p["s"], p["misaligned"]), ignore_index=p["ignore"], offset_weight=p["weight"], smooth_eps=p["eps"])


def _fused(P, p, g=(0.0, 0.0, 1.0)):
    mis = p["misaligned"]
    x = _to(p["x"], mis).requires_grad_(True)
    sp = None if p["sp"] is None else _to(p["sp"], mis).requires_grad_(True)
    res = _call(P, p, x, sp)
    res.losses.backward(torch.tensor(g, device="cuda"))
    torch.cuda.synchronize()
    return dict(losses=res.losses.detach(), counts=res.counts, rows=res.rows, grad_logits=x.grad, grad_shift_pred=None if sp is None else sp.grad)


def _composite(p, g=(0.0, 0.0, 1.0)):
    """torch's chain as a training step runs it: the logits widened to fp32 (autocast's cast), cross-entropy or the reference's smooth_loss,
    L1, the weighted sum, backward"""
    x = p["x"].cuda().requires_grad_(True)
    sp = None if p["sp"] is None else p["sp"].cuda().requires_grad_(True)
    t = p["t"].cuda()
    if p["eps"] > 0:
        keep = t != p["ignore"]
        hot = F.one_hot(t[keep], x.shape[1]).float()
        w = hot * (1 - p["eps"]) + (1 - hot) * (p["eps"] / (x.shape[1] - 1))
        ce = -(w * F.log_softmax(x[keep].float(), dim=1)).sum(dim=1).mean()
    else:
        ce = F.cross_entropy(x.float(), t, ignore_index=p["ignore"])
    l1 = F.l1_loss(sp.float(), p["s"].cuda()) if sp is not None else torch.zeros((), device="cuda")
    total = ce + p["weight"] * l1 if sp is not None else ce * 1.0
    losses = torch.stack([ce, l1, total])
    losses.backward(torch.tensor(g, device="cuda"))
    torch.cuda.synchronize()
    return dict(losses=losses.detach(), grad_logits=x.grad, grad_shift_pred=None if sp is None else sp.grad)


def _oracle(p, g=(0.0, 0.0, 1.0)):
    return O.segmentation_loss(_f64(p["x"]), p["t"].numpy(), _f64(p["sp"]), _f64(p["s"]), g, ignore_index=p["ignore"], offset_weight=p["weight"],
                               smooth_eps=p["eps"])


def _under_bar(name, got, comp, want, u, scale=1.0):
    """the standing bar on one tensor; -> (ok, figure)"""
    e_f = float(np.abs(_f64(got) / scale - want / scale).max(initial=0.0))
    e_c = float(np.abs(_f64(comp) / scale - want / scale).max(initial=0.0))
    top = float(np.abs(want / scale).max(initial=0.0))
    return e_f <= 4 * e_c + u * top, f"{name} {e_f:.2e}/{e_c:.2e}"


def _check(P, p, label, g=(0.0, 0.0, 1.0), scale=1.0):
    want, got, comp = _oracle(p, g), _fused(P, p, g), _composite(p, g)
    n, c = p["x"].shape
    assert got["losses"].dtype == torch.float32 and tuple(got["losses"].shape) == (3,)
    assert got["grad_logits"].dtype == p["x"].dtype and tuple(got["grad_logits"].shape) == (n, c)
    assert got["counts"].dtype == torch.int64 and tuple(got["counts"].shape) == (3, c) and got["rows"].dtype == torch.int64
    assert np.array_equal(got["counts"].cpu().numpy(), want["counts"]) and got["rows"].tolist() == want["rows"].tolist()
    ok, figures = True, []
    for k, name in enumerate(("ce", "l1", "total")):
        fine, fig = _under_bar(name, got["losses"][k], comp["losses"][k], want["losses"][k], U["f32"])
        ok, figures = ok and fine, figures + [fig]
    fine, fig = _under_bar("grad_logits", got["grad_logits"], comp["grad_logits"], want["grad_logits"], U[p["lname"]], scale)
    ok, figures = ok and fine, figures + [fig]
    if p["sp"] is None:
        assert got["grad_shift_pred"] is None and want["grad_shift_pred"] is None
        assert float(got["losses"][1]) == 0.0 and _bits(got["losses"][2:]).item() == _bits(got["losses"][:1]).item()
    else:
        assert got["grad_shift_pred"].dtype == p["sp"].dtype and tuple(got["grad_shift_pred"].shape) == (n, 3)
        fine, fig = _under_bar("grad_shift_pred", got["grad_shift_pred"], comp["grad_shift_pred"], want["grad_shift_pred"], U[p["sname"]], scale)
        ok, figures = ok and fine, figures + [fig]
        assert float(got["grad_shift_pred"][0, 0]) == 0.0
    print(f"segmentation_loss {label}: " + "  ".join(figures) + ("" if ok else "   <-- over the bar"))
    assert ok
    invalid = torch.from_numpy(~O.valid_rows(p["t"].numpy(), c, p["ignore"])).cuda()
    assert not bool(_bits(got["grad_logits"][invalid]).any())                               # exactly zero (and +0)
    return got


FP32_CASES = [(c, n, False) for c in (13, 19, 20) for n in (1, 5, 333, 4099)] + [(1, 65, False), (2, 65, False), (7, 65, False), (64, 3, False),
                                                                                 (64, 333, False), (19, 333, True)]


@pytest.mark.parametrize("c,n,misaligned", FP32_CASES)
def test_operator_fp32(P, c, n, misaligned):
    p = _inputs(n, c, seed=c + n, misaligned=misaligned)
    _check(P, p, f"fp32 C={c} n={n}{' misaligned' if misaligned else ''}")


@pytest.mark.parametrize("lname,sname", [("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("f32", "f16")])
def test_operator_half_and_mixed_rows(P, lname, sname):
    p = _inputs(333, 19, lname, sname, seed=41)
    _check(P, p, f"{lname} logits, {sname} shift_pred C=19 n=333")


def test_operator_under_a_loss_scale(P):
    """the GradScaler case: grad_losses = [0, 0, 65536] on f16 logits; the scale is applied before the one rounding to f16"""
    p = _inputs(333, 19, "f16", "f16", seed=42)
    _check(P, p, "f16 C=19 n=333, loss scale 65536", g=(0.0, 0.0, 65536.0), scale=65536.0)


def test_operator_without_the_shift_pair(P):
    p = _inputs(333, 19, seed=43, shift=False)
    _check(P, p, "fp32 C=19 n=333, no shift pair")


def test_operator_smoothed(P):
    p = _inputs(333, 19, seed=44, eps=0.1)
    _check(P, p, "fp32 C=19 n=333, smooth_eps 0.1")


@pytest.mark.parametrize("through", ["ce", "shift", "all three"])
def test_backward_through_each_loss(P, through):
    p = _inputs(333, 19, "f16", "f32", seed=45)
    g = {"ce": (1.0, 0.0, 0.0), "shift": (0.0, 1.0, 0.0), "all three": (0.7, -1.3, 0.4)}[through]
    want = _oracle(p, g)
    x, sp = p["x"].cuda().requires_grad_(True), p["sp"].cuda().requires_grad_(True)
    res = _call(P, p, x, sp)
    assert res.ce.dim() == res.shift.dim() == res.total.dim() == 0 and res.ce.data_ptr() == res.losses.data_ptr()
    if through == "all three":
        torch.autograd.backward([res.ce, res.shift, res.total], [torch.tensor(v, device="cuda") for v in g])
    else:
        getattr(res, through).backward()
    torch.cuda.synchronize()
    comp = _composite(p, g)
    ok, figures = True, []
    for name, grad, u in (("grad_logits", x.grad, U["f16"]), ("grad_shift_pred", sp.grad, U["f32"])):
        fine, fig = _under_bar(name, grad, comp[name], want[name], u)
        ok, figures = ok and fine, figures + [fig]
    print(f"segmentation_loss backward through {through}: " + "  ".join(figures))
    assert ok
    if through == "shift":
        assert not bool(x.grad.abs().max() > 0)
    if through == "ce":
        assert not bool(sp.grad.abs().max() > 0)


def test_grid_stride(P):
    """300 000 rows of 19 classes: 1172 tiles of 256 rows, past the forward's cap of 1024 workgroups (262 144 rows)"""
    p = _inputs(300000, 19, seed=2)
    _check(P, p, "fp32 C=19 n=300000")


def test_two_runs_give_the_same_bits(P):
    for lname in ("f32", "f16"):
        p = _inputs(4099, 19, lname, lname, seed=3)
        a, b = _fused(P, p), _fused(P, p)
        for name in a:
            assert torch.equal(_bits(a[name]), _bits(b[name])), (lname, name)


def test_stat_is_the_oracles_lse(P):
    from stratified_transformer_amd import pointops2_cuda as C
    p = _inputs(333, 19, seed=4)
    x, t = p["x"].cuda(), p["t"].cuda()
    stat, partials = torch.empty(333, 2, device="cuda"), torch.empty(2, 2, device="cuda", dtype=torch.float64)
    counts, rows, losses = torch.zeros(3, 19, device="cuda", dtype=torch.int64), torch.zeros(2, device="cuda", dtype=torch.int64), torch.empty(3, device="cuda")
    C.seg_loss_forward(333, 19, x, t, None, None, IGNORE, 0.0, 1.0, stat, partials, counts, rows, losses)
    want = _oracle(dict(p, sp=None, s=None))
    err = float(np.abs(_f64(stat).sum(1) - want["lse"]).max())
    print(f"segmentation_loss lse: err {err:.2e} on values up to {float(np.abs(want['lse']).max()):.2f}")
    assert err <= 4 * U["f32"] * float(np.abs(want["lse"]).max()) and np.array_equal(_f64(stat)[:, 0], _f64(x).max(1))
    assert np.array_equal(counts.cpu().numpy(), want["counts"]) and rows.tolist() == want["rows"].tolist()


def test_all_rows_ignored(P):
    p = _inputs(333, 19, seed=5, ignored=1.0)
    assert bool((p["t"] == IGNORE).all())
    want, got = _oracle(p), _fused(P, p)
    ce, l1, total = got["losses"].tolist()
    assert np.isnan(ce) and np.isnan(total) and np.isfinite(l1) and abs(l1 - want["losses"][1]) <= 4 * U["f32"] * want["losses"][1]
    assert not bool(_bits(got["grad_logits"]).any()) and got["rows"].tolist() == [0, 0] and not bool(got["counts"].any())
    err = float(np.abs(_f64(got["grad_shift_pred"]) - want["grad_shift_pred"]).max())
    print(f"segmentation_loss all rows ignored: l1 {l1:.6f} grad_shift_pred err {err:.2e}")
    assert err <= U["f32"] * float(np.abs(want["grad_shift_pred"]).max())


def test_operator_without_rows(P):
    x = torch.zeros(0, 19, device="cuda", dtype=torch.float16, requires_grad=True)
    sp = torch.zeros(0, 3, device="cuda", requires_grad=True)
    res = P.segmentation_loss(x, torch.zeros(0, device="cuda", dtype=torch.int64), sp, torch.zeros(0, 3, device="cuda"))
    assert tuple(res.losses.shape) == (3,) and tuple(res.counts.shape) == (3, 19) and tuple(res.rows.shape) == (2,)
    assert all(np.isnan(v) for v in res.losses.tolist()) and not bool(res.counts.any()) and res.rows.tolist() == [0, 0]
    res.total.backward()
    assert tuple(x.grad.shape) == (0, 19) and x.grad.dtype == torch.float16 and tuple(sp.grad.shape) == (0, 3)
    res = P.segmentation_loss(x, torch.zeros(0, device="cuda", dtype=torch.int64))
    assert np.isnan(res.ce.item()) and res.shift.item() == 0.0 and np.isnan(res.total.item())


@pytest.mark.parametrize("bad", [19, -1])
def test_out_of_range_label(P, bad):
    """torch traps such a label on the device; here it is skipped and counted, and never used as an index.  ignore_index = -100, the
    operator's default: the ignored rows carry a negative label beside the bad one"""
    p = _inputs(333, 19, seed=6, ignore_index=-100)
    p["t"][11] = -100
    assert int((p["t"] == -100).sum()) > 20
    _check(P, p, f"fp32 C=19 n=333, ignore_index -100 (before the label {bad})", (0.5, 0.25, 1.0))
    ignored = _fused(P, p, (0.5, 0.25, 1.0))
    p["t"][11] = bad
    got = _fused(P, p, (0.5, 0.25, 1.0))
    assert got["rows"].tolist() == [int(ignored["rows"][0]), 1] and int(ignored["rows"][1]) == 0
    for name in ("losses", "counts", "grad_logits", "grad_shift_pred"):
        assert torch.equal(_bits(got[name]), _bits(ignored[name])), name
    assert np.array_equal(got["counts"].cpu().numpy(), _oracle(p)["counts"])


@pytest.mark.parametrize("lname", ["f32", "f16"])
def test_argmax_ties(P, lname):
    """logits drawn from {0, 1, 2}: most rows have several equal maxima; the smallest index is the prediction"""
    p = _inputs(4099, 19, lname, seed=7)
    p["x"] = torch.randint(0, 3, (4099, 19), generator=torch.Generator().manual_seed(8)).to(DTYPES[lname])
    p["x"][5] = 1.0
    want, got = _oracle(p), _fused(P, p)
    tied = int(((p["x"].float() == p["x"].float().max(1, keepdim=True)[0]).sum(1) > 1).sum())
    print(f"segmentation_loss argmax ties {lname}: {tied} of 4099 rows tied, intersection {int(want['counts'][0].sum())}")
    assert tied > 3000 and np.array_equal(got["counts"].cpu().numpy(), want["counts"])


def test_hard_rows(P):
    """C = 19, n = 10: a saturated softmax whose target is not the maximum, a row of equal logits, a row of 1e4 + N(0, 1), a -inf beside the
    target; then a NaN and a +inf - each row against the oracle, the poison confined to its row"""
    n, c = 10, 19
    p = _inputs(n, c, seed=21, ignored=0.0)
    gen = torch.Generator().manual_seed(1)
    p["x"][0, 4] += 60.0
    p["t"][0] = 9
    p["x"][1] = 0.75
    p["x"][2] = 1e4 + torch.randn(c, generator=gen)
    p["t"][3] = 2
    p["x"][3, 11] = float("-inf")
    clean = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in p.items()}
    p["x"][5, 17] = float("nan")
    p["x"][7, 18] = float("inf")
    want, got, ref = _oracle(p), _fused(P, p), _fused(P, clean)
    want_clean, comp = _oracle(clean), _composite(clean)
    rows = [r for r in range(n) if r not in (5, 7)]
    assert np.array_equal(np.isfinite(_f64(got["grad_logits"])), np.isfinite(want["grad_logits"]))   # the oracle's set of non-finite entries
    assert not np.isfinite(want["grad_logits"][[5, 7]]).any() and np.isfinite(want["grad_logits"][rows]).all()
    assert torch.equal(_bits(got["grad_logits"][rows]), _bits(ref["grad_logits"][rows]))               # the other rows: as without the poison
    assert got["rows"].tolist() == ref["rows"].tolist() == [n, 0]
    assert np.array_equal(got["counts"].cpu().numpy(), want["counts"]) and np.array_equal(ref["counts"].cpu().numpy(), want_clean["counts"])
    assert np.array_equal(np.isnan(_f64(got["losses"])), np.isnan(want["losses"])) and np.isnan(want["losses"][[0, 2]]).all()
    assert np.isfinite(_f64(got["losses"])[1]) and torch.equal(_bits(got["grad_shift_pred"]), _bits(ref["grad_shift_pred"]))
    names = {0: " (one logit 60 above, target elsewhere)", 1: " (equal logits)", 2: " (1e4 + N(0,1))", 3: " (-inf beside the target)"}
    for r in range(n):
        fine, fig = _under_bar("grad_logits", ref["grad_logits"][r], comp["grad_logits"][r], want_clean["grad_logits"][r], U["f32"])
        print(f"segmentation_loss hard rows, row {r}{names.get(r, '')}: {fig}")
        assert fine, r
    ok, figures = True, []
    for k, name in enumerate(("ce", "l1", "total")):
        fine, fig = _under_bar(name, ref["losses"][k], comp["losses"][k], want_clean["losses"][k], U["f32"])
        ok, figures = ok and fine, figures + [fig]
    print("segmentation_loss hard rows, losses: " + "  ".join(figures))
    assert ok


# ---- end to end: two heads under autocast with a GradScaler ----
class _Heads(nn.Module):
    def __init__(self, c_in, classes):
        super().__init__()
        self.cls = nn.Sequential(nn.Linear(c_in, c_in), nn.BatchNorm1d(c_in), nn.ReLU(inplace=True), nn.Linear(c_in, classes))
        self.shift = nn.Sequential(nn.Linear(c_in, c_in), nn.BatchNorm1d(c_in), nn.ReLU(inplace=True), nn.Linear(c_in, 3))

    def forward(self, feats):
        return self.cls(feats), self.shift(feats)


def _grads(module, leaf):
    return [leaf.grad.detach().clone()] + [q.grad.detach().clone() for _, q in sorted(module.named_parameters())]


def test_two_heads_under_autocast_with_a_grad_scaler(P):
    n, c_in, classes, weight = 1400, 48, 19, 0.5
    torch.manual_seed(12)
    heads = _Heads(c_in, classes).train()
    g = torch.Generator().manual_seed(13)
    feats0, shift = torch.randn(n, c_in, generator=g), torch.randn(n, 3, generator=g)
    target = torch.randint(0, classes, (n,), generator=g)
    target[torch.rand(n, generator=g) < 0.1] = IGNORE
    h64 = copy.deepcopy(heads).double()
    leaf = feats0.double().requires_grad_(True)
    out, sh = h64(leaf)
    (F.cross_entropy(out, target, ignore_index=IGNORE) + weight * F.l1_loss(sh, shift.double())).backward()
    want = _grads(h64, leaf)
    runs = {}
    for fused in (False, True):
        net = copy.deepcopy(heads).cuda().train()
        scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
        feats = feats0.cuda().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            out, sh = net(feats)
            assert out.dtype == torch.float16 and sh.dtype == torch.float16
            if fused:
                res = P.segmentation_loss(out, target.cuda(), sh, shift.cuda(), ignore_index=IGNORE, offset_weight=weight)
                total, pair = res.total, res.losses.tolist()[:2]
            else:
                ce, l1 = nn.CrossEntropyLoss(ignore_index=IGNORE)(out, target.cuda()), nn.L1Loss()(sh, shift.cuda())
                total, pair = ce + weight * l1, [ce.item(), l1.item()]
        scaler.scale(total).backward()
        torch.cuda.synchronize()
        runs[fused] = ([t / 65536.0 for t in _grads(net, feats)], pair)
    print(f"two heads: losses fused {runs[True][1]} composite {runs[False][1]}")
    assert all(abs(a - b) <= 1e-3 * abs(b) for a, b in zip(runs[True][1], runs[False][1]))
    worst = 0.0
    for name, w64, a, b in zip(["input"] + [k for k, _ in sorted(heads.named_parameters())], want, runs[True][0], runs[False][0]):
        e_on, e_off, top = float((a.double().cpu() - w64).abs().max()), float((b.double().cpu() - w64).abs().max()), float(w64.abs().max())
        print(f"two heads {name}: err fused {e_on:.2e} composite {e_off:.2e} (max {top:.2e})")
        worst = max(worst, e_on - (4 * e_off + U["f16"] * top))
    assert worst <= 0.0
