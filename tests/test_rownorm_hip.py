"""GPU (-m gpu): residual add + DropPath row scale + LayerNorm on csrc/rownorm.hip - pointops.residual_norm and the fused block forwards of
layers.patch_block_classes - against the float64 oracle of tests/rownorm_oracle.py evaluated on the CPU on the same inputs.

Bars.  err(.) = max |. - float64 oracle|; u = 2^-24 / 2^-11 / 2^-8 for f32 / f16 / bf16 outputs; "composite" = torch's own unfused chain
(DropPath's x.div(keep) * mask, add, F.layer_norm, cast) run on the GPU in the same test.
  z, per element:                     |z - z64| <= 2^-23 * (|x| + |s * y|)                        (two roundings)
  o, dx, dy, dgamma, dbeta:           err(fused) <= 4 * err(composite) + u * max|want|            (fp32 sums of one length in another order)
  blocks (output, input gradient, every parameter gradient): err(patched) <= 4 * err(unpatched) + u * max|want|, u of f32, under autocast of f16
  layer with the real attention:      patched against unpatched within 1e-4 of each tensor's scale
A row with s[n] == 0: z[n] == x[n] bit for bit, dy[n] == 0.  Two runs: the same bits.  A NaN / Inf row: the oracle's set of non-finite
entries, every other row bit-identical to the run without the poison.

Measured on one MI355X (max abs error against float64, fused / composite; s = a mask with 30 % zeros; z never above its bound):
    fp32  c=48   n=4099     o 8.6e-07 / 8.1e-07   dx 9.4e-07 / 9.6e-07   dy 9.0e-07 / 1.2e-06   dgamma 1.6e-05 / 2.0e-05   dbeta 1.7e-05 / 1.5e-05
    fp32  c=96   n=4099     o 9.6e-07 / 9.7e-07   dx 9.9e-07 / 1.0e-06   dy 8.5e-07 / 1.0e-06   dgamma 2.5e-05 / 2.3e-05   dbeta 1.9e-05 / 2.1e-05
    fp32  c=192  n=4099     o 9.4e-07 / 9.1e-07   dx 1.3e-06 / 1.2e-06   dy 1.1e-06 / 9.6e-07   dgamma 2.2e-05 / 3.3e-05   dbeta 2.1e-05 / 2.2e-05
    fp32  c=384  n=4099     o 1.1e-06 / 8.9e-07   dx 1.0e-06 / 1.1e-06   dy 1.1e-06 / 1.1e-06   dgamma 2.6e-05 / 2.7e-05   dbeta 2.7e-05 / 2.1e-05
    fp32  c=7    n=65       o 3.7e-07 / 3.1e-07   dx 6.3e-07 / 9.3e-07   dy 9.0e-07 / 1.3e-06   dgamma 1.5e-06 / 1.1e-06   dbeta 6.7e-07 / 3.3e-06
    fp32  c=1024 n=3        o 4.9e-07 / 4.7e-07   dx 6.6e-07 / 3.9e-07   dy 4.4e-07 / 3.8e-07   dgamma 9.6e-07 / 1.3e-06   dbeta 3.3e-07 / 3.3e-07
    fp32  c=48   n=333 misaligned   o 6.6e-07 / 6.1e-07   dx 8.2e-07 / 6.7e-07   dy 8.6e-07 / 7.2e-07   dgamma 4.6e-06 / 6.1e-06   dbeta 4.4e-06 / 3.9e-06
    fp32  c=48   n=400000   o 1.1e-06 / 1.1e-06   dx 1.5e-06 / 1.3e-06   dy 1.3e-06 / 1.5e-06   dgamma 3.5e-04 / 4.7e-04   dbeta 3.2e-04 / 5.5e-04
    f16   c=48   n=333      o 1.7e-03 / 2.4e-03   dx 5.7e-07 / 2.2e-04   dy 2.0e-03 / 3.5e-03   dgamma 6.8e-06 / 6.5e-03   dbeta 9.5e-07 / 9.5e-07
    bf16  c=384  n=333      o 1.5e-02 / 1.9e-02   dx 7.5e-07 / 7.4e-04   dy 1.6e-02 / 3.5e-02   dgamma 1.4e-05 / 6.0e-02   dbeta 1.9e-06 / 1.9e-06
    (half rows: the composite rounds y / keep to the half type before the add, the fused pass does not - hence its smaller dx and dgamma)
    hard rows, constant row     o 0 / 3.2e-04         dx 1.1e-04 / 7.2e-05       row of 1e3 + N(0,1)   o 6.7e-05 / 3.3e-04   dx 6.2e-06 / 4.6e-05
    blocks fp32          output 1.8e-06 patched / 1.7e-06 unpatched   input gradient 2.5e-06 / 2.5e-06      (both call conventions alike)
    blocks autocast(f16) output 3.0e-03 patched / 4.3e-03 unpatched   input gradient 3.9e-03 / 4.1e-03
    layer with the real attention: |patched - unpatched| <= 3.8e-05 on gradients of magnitude 86 (fc2.weight), i.e. 4e-07 of the scale
Every test prints its figures.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stratified_transformer_amd import scene
from tests import rownorm_oracle as O
from tests.util import dev

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
U = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
KEEP = 0.7


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


def _inputs(n, c, yname, oname, with_s, seed, misaligned=False):
    """host tensors of one case; misaligned: every [n, c] operand is a contiguous view one element into its buffer (made on the GPU by _to)"""
    g = torch.Generator().manual_seed(seed)
    p = dict(x=torch.randn(n, c, generator=g), y=torch.randn(n, c, generator=g).to(DTYPES[yname]), go=torch.randn(n, c, generator=g).to(DTYPES[oname]),
             gz=torch.randn(n, c, generator=g), gamma=1 + 0.2 * torch.randn(c, generator=g), beta=0.2 * torch.randn(c, generator=g))
    mask = (torch.rand(n, generator=g) >= 0.3).float()                                   # zeros in about 30 % of the rows
    p["mask"], p["s"] = (mask, mask / KEEP) if with_s else (None, None)
    p["misaligned"], p["odt"] = misaligned, DTYPES[oname]
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


def _fused(P, p):
    mis = p["misaligned"]
    x, y = _to(p["x"], mis).requires_grad_(True), None if p["y"] is None else _to(p["y"], mis).requires_grad_(True)
    w, b = p["gamma"].cuda().requires_grad_(True), p["beta"].cuda().requires_grad_(True)
    z, o = P.residual_norm(x, y, _to(p["s"]), w, b, 1e-5, p["odt"])
    assert y is not None or z is x
    _backward(z, o, _to(p["gz"], mis), _to(p["go"], mis))
    return dict(z=z.detach(), o=o.detach(), dx=x.grad, dy=None if y is None else y.grad, dgamma=w.grad, dbeta=b.grad)


def _backward(z, o, gz, go):
    """either incoming gradient may be absent (None in p)"""
    pairs = [(t, g) for t, g in ((z, gz), (o, go)) if g is not None]
    torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
    torch.cuda.synchronize()


def _composite(p):
    """what the parent's block runs at one site: DropPath's arithmetic in y's dtype, the add, F.layer_norm, the cast for the next Linear"""
    x, y = p["x"].cuda().requires_grad_(True), None if p["y"] is None else p["y"].cuda().requires_grad_(True)
    w, b = p["gamma"].cuda().requires_grad_(True), p["beta"].cuda().requires_grad_(True)
    if y is None:
        z = x * 1.0
    else:
        z = x + (y if p["mask"] is None else y.div(KEEP) * p["mask"].cuda().to(y.dtype).unsqueeze(1))
    o = F.layer_norm(z, (z.shape[1],), w, b, 1e-5).to(p["odt"])
    _backward(z, o, _to(p["gz"]), _to(p["go"]))
    return dict(z=z.detach(), o=o.detach(), dx=x.grad, dy=None if y is None else y.grad, dgamma=w.grad, dbeta=b.grad)


def _check(P, p, label, yname, oname):
    want = O.residual_norm(_f64(p["x"]), _f64(p["y"]), _f64(p["s"]), _f64(p["gamma"]), _f64(p["beta"]), _f64(p["go"]), _f64(p["gz"]))
    got, comp = _fused(P, p), _composite(p)
    n, c = p["x"].shape
    assert got["z"].dtype == torch.float32 and got["o"].dtype == p["odt"] and got["dx"].dtype == torch.float32
    assert all(tuple(got[k].shape) == (n, c) for k in ("z", "o", "dx"))
    if p["y"] is not None:
        assert got["dy"].dtype == p["y"].dtype and tuple(got["dy"].shape) == (n, c)
    sy = 0.0 if p["y"] is None else np.abs(_f64(p["y"]) * (1.0 if p["s"] is None else _f64(p["s"])[:, None]))
    z_excess = float((np.abs(_f64(got["z"]) - want["z"]) - 2.0 ** -23 * (np.abs(_f64(p["x"])) + sy)).max(initial=-1.0))
    figures = [f"z excess {z_excess:.1e}"]
    ok = z_excess <= 0.0
    for name, u in (("o", U[oname]), ("dx", U["f32"]), ("dy", U[yname]), ("dgamma", U["f32"]), ("dbeta", U["f32"])):
        if got[name] is None:                                                             # no y, or no dO: no such gradient on either side
            assert comp[name] is None and (want[name] is None or not want[name].any()), name
            continue
        assert tuple(got[name].shape) == tuple(want[name].shape), name
        e_f = float(np.abs(_f64(got[name]) - want[name]).max(initial=0.0))
        e_c = float(np.abs(_f64(comp[name]) - want[name]).max(initial=0.0))
        top = float(np.abs(want[name]).max(initial=0.0))
        figures.append(f"{name} {e_f:.2e}/{e_c:.2e}")
        ok = ok and e_f <= 4 * e_c + u * top
    print(f"residual_norm {label}: " + "  ".join(figures) + ("" if ok else "   <-- over the bar"))
    assert ok
    if p["s"] is not None:
        dropped = (p["s"] == 0).cuda()
        assert torch.equal(_bits(got["z"][dropped]), _bits(_to(p["x"])[dropped]))        # z[n] == x[n] bit for bit
        assert float(got["dy"][dropped].float().abs().max().item() if bool(dropped.any()) else 0.0) == 0.0
    return got


FP32_CASES = [(c, n, False) for c in (48, 96, 192, 384) for n in (1, 5, 333, 4099)] + [(7, 65, False), (1024, 3, False), (48, 333, True)]


@pytest.mark.parametrize("with_s", [True, False])
@pytest.mark.parametrize("c,n,misaligned", FP32_CASES)
def test_operator_fp32(P, c, n, misaligned, with_s):
    p = _inputs(n, c, "f32", "f32", with_s, seed=c + n, misaligned=misaligned)
    _check(P, p, f"fp32 c={c} n={n} s={'mask' if with_s else 'None'}{' misaligned' if misaligned else ''}", "f32", "f32")


def test_operator_without_rows(P):
    x = torch.zeros(0, 48, device="cuda", requires_grad=True)
    w, b = torch.ones(48, device="cuda", requires_grad=True), torch.zeros(48, device="cuda", requires_grad=True)
    z, o = P.residual_norm(x, torch.zeros(0, 48, device="cuda", dtype=torch.float16), torch.zeros(0, device="cuda"), w, b, out_dtype=torch.float16)
    assert tuple(z.shape) == tuple(o.shape) == (0, 48) and z.dtype == torch.float32 and o.dtype == torch.float16
    (z.sum() + o.float().sum()).backward()
    assert tuple(x.grad.shape) == (0, 48) and float(w.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0
    z, o = P.residual_norm(x, None, None, w, b)
    assert z is x and tuple(o.shape) == (0, 48) and o.dtype == torch.float32


@pytest.mark.parametrize("with_s", [True, False])
@pytest.mark.parametrize("name", ["f16", "bf16"])
@pytest.mark.parametrize("c,n", [(48, 333), (384, 333)])
def test_operator_half_rows(P, c, n, name, with_s):
    p = _inputs(n, c, name, name, with_s, seed=c + n + 1)
    _check(P, p, f"{name} c={c} n={n} s={'mask' if with_s else 'None'}", name, name)


@pytest.mark.parametrize("variant", ["y None", "dZ None", "dO None", "y None, dZ None"])
def test_operator_absent_operands(P, variant):
    """y None (z is x itself: the norm alone) and either incoming gradient None, o in f16 as under autocast"""
    p = _inputs(333, 96, "f32", "f16", False, seed=8)
    for key, gone in (("y", "y None"), ("gz", "dZ None"), ("go", "dO None")):
        if gone in variant:
            p[key] = None
    _check(P, p, f"f32 -> f16 c=96 n=333, {variant}", "f32", "f16")


def test_grid_stride(P):
    """400 000 rows of 48 channels: 25 000 workgroups' worth of rows, past the forward's cap of num_cus() * 64 and the backward's 1024"""
    p = _inputs(400000, 48, "f32", "f32", True, seed=2)
    _check(P, p, "fp32 c=48 n=400000 s=mask", "f32", "f32")


def test_two_runs_give_the_same_bits(P):
    p = _inputs(4099, 48, "f32", "f32", True, seed=3)
    a, b = _fused(P, p), _fused(P, p)
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name
    p = _inputs(4099, 48, "f16", "f16", True, seed=3)
    a, b = _fused(P, p), _fused(P, p)
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name


def test_hard_rows(P):
    """C = 96: a constant row (variance 0), a row of 1e3 + N(0, 1) (a cancelling variance formula fails the o bar there), a row holding a
    NaN and a row holding +Inf - each row against the oracle, the poison confined to its row"""
    n, c = 10, 96
    p = _inputs(n, c, "f32", "f32", False, seed=21)
    p["x"][0], p["y"][0] = 1.5, 0.5                                                      # z = 2 in every channel: all sums exact
    p["x"][1] = 1e3 + torch.randn(c, generator=torch.Generator().manual_seed(1))
    clean = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in p.items()}
    p["y"][4, 17] = float("nan")
    p["x"][7, 95] = float("inf")
    want = O.residual_norm(_f64(p["x"]), _f64(p["y"]), _f64(p["s"]), _f64(p["gamma"]), _f64(p["beta"]), _f64(p["go"]), _f64(p["gz"]))
    got, comp, ref = _fused(P, p), _composite(p), _fused(P, clean)
    rows = [r for r in range(n) if r not in (4, 7)]
    for name in ("z", "o", "dx", "dy"):
        assert np.array_equal(np.isfinite(_f64(got[name])), np.isfinite(want[name])), name   # the oracle's set of non-finite entries
        assert not np.isfinite(want[name][[4, 7]]).all() and np.isfinite(want[name][rows]).all()
        assert torch.equal(_bits(got[name][rows]), _bits(ref[name][rows])), name           # the other rows: as without the poison
    for name in ("dgamma", "dbeta"):
        assert np.array_equal(np.isfinite(_f64(got[name])), np.isfinite(want[name])), name
        assert np.array_equal(np.isnan(_f64(got[name])), np.isnan(want[name])), name
    for r in rows:
        sy = np.abs(_f64(p["y"])[r])
        assert float((np.abs(_f64(got["z"])[r] - want["z"][r]) - 2.0 ** -23 * (np.abs(_f64(p["x"])[r]) + sy)).max()) <= 0.0
        figures = []
        for name in ("o", "dx", "dy"):
            e_f, e_c = (float(np.abs(_f64(t[name])[r] - want[name][r]).max()) for t in (got, comp))
            top = float(np.abs(want[name][r]).max())
            figures.append(f"{name} {e_f:.2e}/{e_c:.2e}")
            assert e_f <= 4 * e_c + U["f32"] * top, (r, name, e_f, e_c, top)
        print(f"residual_norm hard rows, row {r}{' (constant)' if r == 0 else ' (1e3 + N(0,1))' if r == 1 else ''}: " + "  ".join(figures))
    assert float(np.abs(_f64(got["o"])[0] - _f64(p["beta"])).max()) == 0.0                # variance 0: o is beta


# ---- blocks ----
def _grads(module, leaf):
    return [leaf.grad.detach().clone()] + [q.grad.detach().clone() for _, q in sorted(module.named_parameters())]


def _names(module):
    return ["input"] + [n for n, _ in sorted(module.named_parameters())]


def _run_blocks(blocks, feats0, go, swin, amp, seed):
    torch.manual_seed(seed)
    blocks.zero_grad(set_to_none=True)
    feats = feats0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        out = O.run_blocks(blocks, feats, swin, chained=True)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), _grads(blocks, feats)


def _replayed_scales(n, count, amp, seed):
    """the row scales DropPath draws under `seed`: `count` calls of torch.rand([n, 1]) in the dtype of the branch (f16 under autocast)"""
    torch.manual_seed(seed)
    draws = [torch.rand((n, 1), dtype=torch.float16 if amp else torch.float32, device="cuda") for _ in range(count)]
    return [(KEEP + d).floor_().double().view(-1) / KEEP for d in draws]


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("swin", [False, True])
def test_blocks_with_a_stand_in_attention(P, swin, amp):
    from stratified_transformer_amd import layers, standin
    from tests import swin_standin
    cls = swin_standin.SwinTransformerBlock if swin else standin.SwinTransformerBlock
    n, c, depth, seed = 1400, 48, 3, 77
    blocks = O.make_blocks(cls, depth, c, 1 - KEEP, seed=5).cuda().train()
    g = torch.Generator().manual_seed(6)
    feats0, go = torch.randn(n, c, generator=g).cuda(), torch.randn(n, c, generator=g).cuda()
    scales = _replayed_scales(n, 2 * depth, amp, seed)
    out64, b64, leaf = O.blocks_float64(blocks, feats0, scales, swin)
    out64.backward(go.double().cpu())
    want = [out64.detach()] + _grads(b64, leaf)
    off = _run_blocks(blocks, feats0, go, swin, amp, seed)
    off1 = _run_blocks(blocks[:1], feats0, go, swin, amp, seed)
    calls = []
    real = P.residual_norm
    try:
        layers.patch_block_classes(swin_block_cls=cls) if swin else layers.patch_block_classes(cls)
        P.residual_norm = lambda x, y, *a, **kw: (calls.append(y is None), real(x, y, *a, **kw))[1]
        on = _run_blocks(blocks, feats0, go, swin, amp, seed)
        assert calls == [True, False, False, False, False, False]                          # one norm1 alone; three attention sites, two hand-offs
        on1 = _run_blocks(blocks[:1], feats0, go, swin, amp, seed)
    finally:
        P.residual_norm = real
        layers.uninstall_fast_layers()
    assert on[0].dtype == torch.float32 and all("_sta_next" not in b.__dict__ and "_sta_norm1" not in b.__dict__ for b in blocks)
    u = U["f16"] if amp else U["f32"]
    mode = ("swin3d" if swin else "stratified") + (" autocast(f16)" if amp else " fp32")
    worst = 0.0
    for name, w64, a, b in zip(["output"] + _names(blocks), want, [on[0]] + on[1], [off[0]] + off[1]):
        e_on, e_off, top = float((a.double().cpu() - w64).abs().max()), float((b.double().cpu() - w64).abs().max()), float(w64.abs().max())
        print(f"blocks {mode} {name}: err patched {e_on:.2e} unpatched {e_off:.2e} (max {top:.2f})")
        worst = max(worst, e_on - (4 * e_off + u * top))
    assert worst <= 0.0
    # the same masks, directly: the rows every draw dropped come back untouched
    dropped = torch.stack([s == 0 for s in scales]).all(0)
    assert torch.equal((on[0] == feats0).all(1), (off[0] == feats0).all(1)) and torch.equal((off[0] == feats0).all(1).cpu(), dropped.cpu())
    dropped1 = (scales[0] == 0) & (scales[1] == 0)                                         # one block: 9 % of the rows
    assert 60 <= int(dropped1.sum()) <= 200
    assert torch.equal((on1[0] == feats0).all(1).cpu(), dropped1.cpu()) and torch.equal((off1[0] == feats0).all(1).cpu(), dropped1.cpu())


def test_layer_with_the_real_attention(P):
    from stratified_transformer_amd import layers, standin
    classes = (standin.BasicLayer, standin.WindowAttention, standin.TransitionDown, standin.SwinTransformerBlock)
    before = [cls.forward for cls in classes]
    xyz = scene.make_room(1400, 9)
    offset = np.array([1400], np.int32)
    torch.manual_seed(5)
    layer = standin.BasicLayer(8, 2, 48, 3, 0.16, 0.01, ratio=0.25, k=16, out_channels=96).cuda().train()
    with torch.no_grad():
        for name, q in layer.named_parameters():
            if "relative_pos" in name:
                q.copy_(torch.randn_like(q) * 0.3)
    g = torch.Generator().manual_seed(4)
    feats0, go, go_down = torch.randn(1400, 48, generator=g).cuda(), torch.randn(1400, 48, generator=g).cuda(), torch.randn(351, 96, generator=g).cuda()
    runs = {}
    try:
        layers.patch_classes(standin.BasicLayer, standin.WindowAttention, standin.TransitionDown)
        for fused_blocks in (False, True):
            if fused_blocks:
                assert layers.patch_block_classes(standin.SwinTransformerBlock) == [standin.SwinTransformerBlock]
            layers.forget_clouds()
            P.clear_caches()
            layer.zero_grad(set_to_none=True)
            feats = feats0.clone().requires_grad_(True)
            f, _, _, f_down, _, _ = layer(feats, dev(xyz), dev(offset))
            assert tuple(f_down.shape) == tuple(go_down.shape)
            torch.autograd.backward([f, f_down], [go, go_down])
            torch.cuda.synchronize()
            runs[fused_blocks] = [f.detach(), f_down.detach()] + _grads(layer, feats)
    finally:
        layers.uninstall_fast_layers()
    assert [cls.forward for cls in classes] == before and not layers._ORIGINAL
    for name, a, b in zip(["output", "down-sampled output"] + _names(layer), runs[True], runs[False]):
        diff, top = float((a - b).abs().max()), max(float(b.abs().max()), 1e-6)
        print(f"layer {name}: |patched - unpatched| {diff:.2e} (max {top:.2f})")
        assert diff <= 1e-4 * top, name
