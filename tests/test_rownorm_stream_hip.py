"""GPU (-m gpu): the half residual stream of csrc/rownorm.hip - pointops.residual_norm_stream and the fused block forwards under
layers.HALF_STREAM - against the float64 oracle of tests/rownorm_oracle.py and the rounding rule of tests/rownorm_stream_oracle.py.

Bars.  T = the stream type (f16 / bf16), u_T = 2^-11 / 2^-8; u of an f32 tensor = 2^-24.  "composite" = what the unpatched block runs at a
site under autocast(T), on the GPU in the same test: half x + y.div(keep) * mask, F.layer_norm, the cast.
  z, per element:            |z - z64| <= u_T * |z64| + 2^-23 * (|x| + |s * y|) (+ 2^-25 for f16), and z is bit-equal to the restatement
  o, dgamma, dbeta, dx, dy:  err(fused) <= 4 * err(composite) + u * max|want|, u of the tensor's type; each side's error is taken against
                             the float64 oracle evaluated on that side's OWN stored z (o is the LayerNorm of the tensor the caller holds)
  blocks (output, input gradient, every parameter gradient): err(patched) <= 4 * err(unpatched) + u_T * max|want| against the float64 blocks
A row with s[n] == 0: z[n] == x[n] bit for bit, dy[n] == 0.  Two runs: the same bits.  A NaN / Inf row: the oracle's set of non-finite
entries, every other row bit-identical to the run without the poison.  x in f32: the bits of pointops.residual_norm.

Measured on one MI355X (max abs error against float64 on the side's own z, fused / composite; s = a mask with 30 % zeros; z never above
its bound and always the restatement's bits):
    f16  y,o=f16  c=48   n=333   o 1.9e-03 / 1.8e-03   dx 2.0e-03 / 2.8e-03   dy 2.0e-03 / 4.0e-03   dgamma 5.6e-06 / 4.7e-06   dbeta 1.9e-06 / 1.9e-06
    f16  y,o=f32  c=48   n=333   o 7.1e-07 / 5.7e-07   dx 2.0e-03 / 2.4e-03   dy 7.3e-07 / 3.3e-03   dgamma 5.4e-06 / 8.8e-06   dbeta 5.5e-06 / 3.9e-06
    bf16 y,o=bf16 c=48   n=333   o 1.5e-02 / 1.6e-02   dx 1.6e-02 / 2.3e-02   dy 1.6e-02 / 3.3e-02   dgamma 3.0e-06 / 4.7e-06   dbeta 0 / 9.5e-07
    bf16 y,o=f32  c=48   n=333   o 5.9e-07 / 5.2e-07   dx 1.5e-02 / 2.8e-02   dy 5.6e-07 / 2.7e-02   dgamma 5.7e-06 / 5.5e-06   dbeta 5.5e-06 / 3.9e-06
    f16  y,o=f16  c=96   n=333   o 1.9e-03 / 1.9e-03   dx 1.9e-03 / 2.9e-03   dy 1.9e-03 / 3.5e-03   dgamma 5.7e-06 / 5.0e-06   dbeta 2.0e-06 / 3.3e-06
    f16  y,o=f16  c=192  n=65    o 1.8e-03 / 1.8e-03   dx 1.9e-03 / 2.8e-03   dy 2.0e-03 / 4.9e-03   dgamma 3.2e-06 / 4.3e-06   dbeta 7.2e-07 / 7.2e-07
    f16  y,o=f16  c=384  n=333   o 1.9e-03 / 1.9e-03   dx 2.0e-03 / 2.9e-03   dy 3.6e-03 / 4.9e-03   dgamma 7.8e-06 / 7.6e-06   dbeta 2.4e-06 / 3.0e-06
    bf16 y,o=bf16 c=384  n=333   o 1.6e-02 / 1.5e-02   dx 1.6e-02 / 2.3e-02   dy 1.6e-02 / 4.1e-02   dgamma 7.1e-06 / 6.3e-06   dbeta 1.9e-06 / 1.9e-06
    f16  y,o=f16  c=1024 n=3     o 9.7e-04 / 9.7e-04   dx 1.9e-03 / 3.1e-03   dy 1.9e-03 / 2.8e-03   dgamma 7.0e-07 / 7.8e-07   dbeta 0 / 0
    bf16 y,o=bf16 c=7    n=65    o 7.8e-03 / 7.4e-03   dx 9.1e-03 / 1.1e-02   dy 1.0e-02 / 1.7e-02   dgamma 1.6e-06 / 3.0e-06   dbeta 0 / 0
    f16  y,o=f16  c=70   n=65    o 1.5e-03 / 1.4e-03   dx 1.7e-03 / 2.8e-03   dy 1.9e-03 / 3.0e-03   dgamma 1.8e-06 / 2.6e-06   dbeta 0 / 0
    f16  y,o=f16  c=48   n=333 misaligned   o 1.9e-03 / 1.8e-03   dx 2.0e-03 / 2.8e-03   dy 2.0e-03 / 4.0e-03   dgamma 5.6e-06 / 4.7e-06   dbeta 1.9e-06 / 1.9e-06
    (dx, dy: one rounding of the fp32 gradient on the fused side, where autograd adds two rounded half gradients and rounds y's product twice)
    blocks autocast(f16)  c=48   output 6.3e-03 patched / 6.5e-03 unpatched   input gradient 6.0e-03 / 6.9e-03      (both call conventions alike)
    blocks autocast(f16)  c=96   output 5.8e-03 / 6.2e-03   input gradient 5.7e-03 / 6.2e-03
    blocks autocast(bf16) c=48   output 6.0e-02 / 4.5e-02   input gradient 5.2e-02 / 5.4e-02
    blocks autocast(bf16) c=96   output 5.1e-02 / 5.9e-02   input gradient 6.2e-02 / 6.2e-02
Every test prints its figures.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rownorm_oracle as O
from tests import rownorm_stream_oracle as S

pytestmark = pytest.mark.gpu

DTYPES, U = S.TORCH, S.U
KEEP = 0.7
# (c, n, misaligned): every lane layout - segments of 16, 32, 64 lanes, a wave with two and with four chunks a lane, scalar segments,
# scalar long rows, and the scalar path on a chunkable width (views one element into the buffer)
SHAPES = [(48, 333, False), (96, 333, False), (192, 65, False), (384, 333, False), (1024, 3, False), (7, 65, False), (70, 65, False), (48, 333, True)]


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


def _f32(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _inputs(n, c, tname, yname, oname, with_s, seed, misaligned=False):
    """host tensors of one case: x and dZ of the stream type, y and dO of their own; misaligned: see _to"""
    g = torch.Generator().manual_seed(seed)
    p = dict(x=torch.randn(n, c, generator=g).to(DTYPES[tname]), y=torch.randn(n, c, generator=g).to(DTYPES[yname]),
             go=torch.randn(n, c, generator=g).to(DTYPES[oname]), gz=torch.randn(n, c, generator=g).to(DTYPES[tname]),
             gamma=1 + 0.2 * torch.randn(c, generator=g), beta=0.2 * torch.randn(c, generator=g))
    mask = (torch.rand(n, generator=g) >= 0.3).float()                                   # zeros in about 30 % of the rows
    p["mask"], p["s"] = (mask, mask / KEEP) if with_s else (None, None)
    p["misaligned"], p["odt"], p["tname"] = misaligned, DTYPES[oname], tname
    return p


def _to(t, misaligned=False):
    """misaligned: a contiguous [n, c] view one element into its buffer - 2 or 4 bytes off every chunk boundary"""
    if t is None:
        return None
    if not misaligned or t.dim() != 2:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 8 != 0
    return view


def _backward(z, o, gz, go):
    """either incoming gradient may be absent (None in p)"""
    pairs = [(t, g) for t, g in ((z, gz), (o, go)) if g is not None]
    torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
    torch.cuda.synchronize()


def _fused(P, p, op=None):
    mis = p["misaligned"]
    x, y = _to(p["x"], mis).requires_grad_(True), None if p["y"] is None else _to(p["y"], mis).requires_grad_(True)
    w, b = p["gamma"].cuda().requires_grad_(True), p["beta"].cuda().requires_grad_(True)
    z, o = (op or P.residual_norm_stream)(x, y, _to(p["s"]), w, b, 1e-5, p["odt"])
    assert y is not None or z is x
    _backward(z, o, _to(p["gz"], mis), _to(p["go"], mis))
    return dict(z=z.detach(), o=o.detach(), dx=x.grad, dy=None if y is None else y.grad, dgamma=w.grad, dbeta=b.grad)


def _composite(p):
    """what the unpatched block runs at one site under autocast(T): DropPath's arithmetic in y's dtype, the add in the stream's dtype,
    F.layer_norm (autocast runs it in fp32), the cast for the next Linear"""
    tdt = DTYPES[p["tname"]]
    x, y = p["x"].cuda().requires_grad_(True), None if p["y"] is None else p["y"].cuda().requires_grad_(True)
    w, b = p["gamma"].cuda().requires_grad_(True), p["beta"].cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=tdt, enabled=tdt != torch.float32):
        if y is None:
            z = x * 1.0
        else:
            z = x + (y if p["mask"] is None else y.div(KEEP) * p["mask"].cuda().to(y.dtype).unsqueeze(1))
            z = z if z.dtype == tdt else z.to(tdt)                                        # an f32 y promotes the sum: the stream stays T
        o = F.layer_norm(z, (z.shape[1],), w, b, 1e-5).to(p["odt"])
    _backward(z, o, _to(p["gz"]), _to(p["go"]))
    return dict(z=z.detach(), o=o.detach(), dx=x.grad, dy=None if y is None else y.grad, dgamma=w.grad, dbeta=b.grad)


def _wants(p, side):
    """the float64 oracle on the z this side stored"""
    return S.on_stored_z(_f32(side["z"]), _f64(p["s"]), _f64(p["gamma"]), _f64(p["beta"]), _f64(p["go"]), _f64(p["gz"]), p["y"] is not None)


def _check(P, p, label, yname, oname):
    tname = p["tname"]
    got, comp = _fused(P, p), _composite(p)
    n, c = p["x"].shape
    assert got["z"].dtype == got["dx"].dtype == DTYPES[tname] and got["o"].dtype == p["odt"] and comp["z"].dtype == DTYPES[tname]
    assert all(tuple(got[k].shape) == (n, c) for k in ("z", "o", "dx"))
    if p["y"] is not None:
        assert got["dy"].dtype == p["y"].dtype and tuple(got["dy"].shape) == (n, c)
    # z: the bar against float64, and the restatement's bits
    rule = S.stream_z(_f32(p["x"]), _f32(p["y"]), _f32(p["s"]), tname)[1]
    z_excess = float((np.abs(_f64(got["z"]) - S.z_float64(_f64(p["x"]), _f64(p["y"]), _f64(p["s"]))) -
                      S.z_bound(_f64(p["x"]), _f64(p["y"]), _f64(p["s"]), tname)).max(initial=-1.0))
    z_same = np.array_equal(_f32(got["z"]).view(np.uint32), rule.view(np.uint32))
    figures = [f"z excess {z_excess:.1e} bits {'equal' if z_same else 'DIFFER'}"]
    ok = z_excess <= 0.0 and z_same
    want_f, want_c = _wants(p, got), _wants(p, comp)
    for name, u in (("o", U[oname]), ("dx", U[tname]), ("dy", U[yname]), ("dgamma", U["f32"]), ("dbeta", U["f32"])):
        if got[name] is None:                                                             # no y, or no dO: no such gradient on either side
            assert comp[name] is None and (want_f[name] is None or not want_f[name].any()), name
            continue
        assert tuple(got[name].shape) == tuple(want_f[name].shape), name
        e_f = float(np.abs(_f64(got[name]) - want_f[name]).max(initial=0.0))
        e_c = float(np.abs(_f64(comp[name]) - want_c[name]).max(initial=0.0))
        top = float(np.abs(want_f[name]).max(initial=0.0))
        figures.append(f"{name} {e_f:.2e}/{e_c:.2e}")
        ok = ok and e_f <= 4 * e_c + u * top
    print(f"residual_norm_stream {label}: " + "  ".join(figures) + ("" if ok else "   <-- over the bar"))
    assert ok
    if p["s"] is not None:
        dropped = (p["s"] == 0).cuda()
        assert int(dropped.sum()) > 0 or n < 10
        assert torch.equal(_bits(got["z"][dropped]), _bits(_to(p["x"])[dropped]))        # z[n] == x[n] bit for bit
        assert float(got["dy"][dropped].float().abs().max().item() if bool(dropped.any()) else 0.0) == 0.0
    return got


@pytest.mark.parametrize("with_s", [True, False])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("tname", ["f16", "bf16"])
@pytest.mark.parametrize("c,n,misaligned", SHAPES)
def test_operator_half_stream(P, c, n, misaligned, tname, wide, with_s):
    """(y, o) typed (T, T) as under autocast, or (f32, f32)"""
    yo = "f32" if wide else tname
    p = _inputs(n, c, tname, yo, yo, with_s, seed=c + n, misaligned=misaligned)
    _check(P, p, f"{tname} y,o={yo} c={c} n={n} s={'mask' if with_s else 'None'}{' misaligned' if misaligned else ''}", yo, yo)


@pytest.mark.parametrize("variant", ["y None", "dZ None", "dO None"])
@pytest.mark.parametrize("tname", ["f16", "bf16"])
def test_operator_absent_operands(P, tname, variant):
    """y None (z is x itself: the norm alone on the widened x) and either incoming gradient None"""
    p = _inputs(333, 96, tname, tname, tname, False, seed=8)
    for key, gone in (("y", "y None"), ("gz", "dZ None"), ("go", "dO None")):
        if gone in variant:
            p[key] = None
    _check(P, p, f"{tname} c=96 n=333, {variant}", tname, tname)


@pytest.mark.parametrize("tname", ["f16", "bf16"])
def test_operator_without_rows(P, tname):
    dt = DTYPES[tname]
    x = torch.zeros(0, 48, device="cuda", dtype=dt, requires_grad=True)
    w, b = torch.ones(48, device="cuda", requires_grad=True), torch.zeros(48, device="cuda", requires_grad=True)
    y = torch.zeros(0, 48, device="cuda", requires_grad=True)
    z, o = P.residual_norm_stream(x, y, torch.zeros(0, device="cuda"), w, b, out_dtype=torch.float16)
    assert tuple(z.shape) == tuple(o.shape) == (0, 48) and z.dtype == dt and o.dtype == torch.float16
    (z.float().sum() + o.float().sum()).backward()
    assert tuple(x.grad.shape) == (0, 48) and x.grad.dtype == dt and y.grad.dtype == torch.float32 and tuple(y.grad.shape) == (0, 48)
    assert float(w.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0
    z, o = P.residual_norm_stream(x, None, None, w, b)
    assert z is x and tuple(o.shape) == (0, 48) and o.dtype == torch.float32


@pytest.mark.parametrize("tname", ["f16", "bf16"])
def test_two_runs_give_the_same_bits(P, tname):
    p = _inputs(4099, 48, tname, tname, tname, True, seed=3)                             # 257 workgroups' partials behind the backward
    a, b = _fused(P, p), _fused(P, p)
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name


@pytest.mark.parametrize("c,n,misaligned,yname,oname,variant", [
    (48, 333, False, "f16", "f16", ""), (96, 333, False, "f32", "f32", ""), (384, 65, False, "bf16", "f16", ""), (1024, 3, False, "f32", "bf16", ""),
    (7, 65, False, "f32", "f32", ""), (70, 65, False, "f16", "f32", ""), (48, 333, True, "f32", "f16", ""),
    (96, 333, False, "f32", "f16", "y None"), (96, 333, False, "f16", "f16", "dZ None"), (96, 333, False, "f16", "f16", "dO None")])
def test_an_f32_stream_gives_the_bits_of_residual_norm(P, c, n, misaligned, yname, oname, variant):
    p = _inputs(n, c, "f32", yname, oname, variant == "", seed=c + n + 2, misaligned=misaligned)
    for key, gone in (("y", "y None"), ("gz", "dZ None"), ("go", "dO None")):
        if gone == variant:
            p[key] = None
    new, old = _fused(P, p), _fused(P, p, op=P.residual_norm)
    for name in ("z", "o", "dx", "dy", "dgamma", "dbeta"):
        assert (new[name] is None) == (old[name] is None), name
        if new[name] is not None:
            assert new[name].dtype == old[name].dtype and torch.equal(_bits(new[name]), _bits(old[name])), name


@pytest.mark.parametrize("tname", ["f16", "bf16"])
def test_poisoned_rows(P, tname):
    """a row holding a NaN (in y) and a row holding +Inf (in x): the oracle's set of non-finite entries, the poison confined to its row"""
    n, c = 10, 96
    p = _inputs(n, c, tname, tname, tname, False, seed=21)
    clean = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in p.items()}
    p["y"][4, 17] = float("nan")
    p["x"][7, 95] = float("inf")
    want = S.residual_norm_stream(_f32(p["x"]), _f32(p["y"]), None, _f64(p["gamma"]), _f64(p["beta"]), _f64(p["go"]), _f64(p["gz"]), tname)
    got, ref = _fused(P, p), _fused(P, clean)
    rows = [r for r in range(n) if r not in (4, 7)]
    for name in ("z", "o", "dx", "dy"):
        assert np.array_equal(np.isfinite(_f64(got[name])), np.isfinite(want[name])), name   # the oracle's set of non-finite entries
        assert np.array_equal(np.isnan(_f64(got[name])), np.isnan(want[name])), name
        assert not np.isfinite(want[name][[4, 7]]).all() and np.isfinite(want[name][rows]).all()
        assert torch.equal(_bits(got[name][rows]), _bits(ref[name][rows])), name           # the other rows: as without the poison
    for name in ("dgamma", "dbeta"):
        assert np.array_equal(np.isfinite(_f64(got[name])), np.isfinite(want[name])), name
        assert np.array_equal(np.isnan(_f64(got[name])), np.isnan(want[name])), name
    print(f"residual_norm_stream {tname} poisoned rows: non-finite z {int((~np.isfinite(want['z'])).sum())}, o {int((~np.isfinite(want['o'])).sum())}, "
          f"dx {int((~np.isfinite(want['dx'])).sum())}; rows {rows} keep their bits")


# ---- blocks ----
def _grads(module, leaf):
    return [leaf.grad.detach().clone()] + [q.grad.detach().clone() for _, q in sorted(module.named_parameters())]


def _names(module):
    return ["input"] + [n for n, _ in sorted(module.named_parameters())]


def _run_blocks(blocks, feats0, go, swin, dt, seed):
    torch.manual_seed(seed)
    blocks.zero_grad(set_to_none=True)
    feats = feats0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dt):
        out = O.run_blocks(blocks, feats, swin, chained=True)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), _grads(blocks, feats)


def _replayed_scales(n, count, dt, seed):
    """the row scales DropPath draws under `seed`: `count` calls of torch.rand([n, 1]) in the dtype of the branch (autocast's)"""
    torch.manual_seed(seed)
    draws = [torch.rand((n, 1), dtype=dt, device="cuda") for _ in range(count)]
    return [(KEEP + d).floor_().double().view(-1) / KEEP for d in draws]


def _block_class(swin):
    from stratified_transformer_amd import standin
    from tests import swin_standin
    return swin_standin.SwinTransformerBlock if swin else standin.SwinTransformerBlock


def _patch(layers, cls, swin):
    return layers.patch_block_classes(swin_block_cls=cls) if swin else layers.patch_block_classes(cls)


@pytest.mark.parametrize("c", [48, 96])
@pytest.mark.parametrize("tname", ["f16", "bf16"])
@pytest.mark.parametrize("swin", [False, True])
def test_blocks_on_a_half_stream(P, swin, tname, c):
    from stratified_transformer_amd import layers
    cls, dt = _block_class(swin), DTYPES[tname]
    n, depth, seed = 333, 3, 77
    blocks = O.make_blocks(cls, depth, c, 1 - KEEP, seed=5).cuda().train()
    g = torch.Generator().manual_seed(6)
    feats0, go = torch.randn(n, c, generator=g).to(dt).cuda(), torch.randn(n, c, generator=g).to(dt).cuda()
    scales = _replayed_scales(n, 2 * depth, dt, seed)
    out64, b64, leaf = O.blocks_float64(blocks, feats0, scales, swin)
    out64.backward(go.double().cpu())
    want = [out64.detach()] + _grads(b64, leaf)
    off = _run_blocks(blocks, feats0, go, swin, dt, seed)
    off1 = _run_blocks(blocks[:1], feats0, go, swin, dt, seed)
    calls, fp32_calls = [], []
    real, real32 = P.residual_norm_stream, P.residual_norm
    try:
        layers.HALF_STREAM = True
        _patch(layers, cls, swin)
        P.residual_norm_stream = lambda x, y, *a, **kw: (calls.append((y is None, x.dtype)), real(x, y, *a, **kw))[1]
        P.residual_norm = lambda *a, **kw: (fp32_calls.append(1), real32(*a, **kw))[1]
        on = _run_blocks(blocks, feats0, go, swin, dt, seed)
        # every site of the chain: the first block's norm1 alone, then per block the attention site and the hand-off to the successor's
        # norm1 - the last block has no successor, its second add stays with torch
        assert calls == [(True, dt)] + [(False, dt)] * (2 * depth - 1) and not fp32_calls
        on1 = _run_blocks(blocks[:1], feats0, go, swin, dt, seed)
    finally:
        P.residual_norm_stream, P.residual_norm = real, real32
        layers.HALF_STREAM = False
        layers.uninstall_fast_layers()
    assert on[0].dtype == off[0].dtype == dt and on[1][0].dtype == dt
    assert all("_sta_next" not in b.__dict__ and "_sta_norm1" not in b.__dict__ for b in blocks)
    mode = ("swin3d" if swin else "stratified") + f" autocast({tname}) c={c}"
    worst = 0.0
    for name, w64, a, b in zip(["output"] + _names(blocks), want, [on[0]] + on[1], [off[0]] + off[1]):
        e_on, e_off, top = float((a.double().cpu() - w64).abs().max()), float((b.double().cpu() - w64).abs().max()), float(w64.abs().max())
        print(f"blocks {mode} {name}: err patched {e_on:.2e} unpatched {e_off:.2e} (max {top:.2f})")
        worst = max(worst, e_on - (4 * e_off + U[tname] * top))
    assert worst <= 0.0
    # the same masks, directly: the rows every draw dropped come back untouched
    dropped = torch.stack([s == 0 for s in scales]).all(0)
    assert torch.equal((on[0] == feats0).all(1), (off[0] == feats0).all(1)) and torch.equal((off[0] == feats0).all(1).cpu(), dropped.cpu())
    dropped1 = (scales[0] == 0) & (scales[1] == 0)                                         # one block: 9 % of the rows
    assert 10 <= int(dropped1.sum()) <= 60
    assert torch.equal((on1[0] == feats0).all(1).cpu(), dropped1.cpu()) and torch.equal((off1[0] == feats0).all(1).cpu(), dropped1.cpu())


@pytest.mark.parametrize("tname", ["f16", "bf16"])
@pytest.mark.parametrize("swin", [False, True])
def test_blocks_with_the_switch_off_give_the_unpatched_bits(P, swin, tname):
    """HALF_STREAM = False (the default): patched blocks leave a half stream to the original forward"""
    from stratified_transformer_amd import layers
    cls, dt = _block_class(swin), DTYPES[tname]
    n, c, depth, seed = 333, 48, 3, 77
    blocks = O.make_blocks(cls, depth, c, 1 - KEEP, seed=5).cuda().train()
    g = torch.Generator().manual_seed(6)
    feats0, go = torch.randn(n, c, generator=g).to(dt).cuda(), torch.randn(n, c, generator=g).to(dt).cuda()
    off = _run_blocks(blocks, feats0, go, swin, dt, seed)
    calls = []
    real32 = P.residual_norm
    try:
        layers.HALF_STREAM = False
        _patch(layers, cls, swin)
        P.residual_norm = lambda *a, **kw: (calls.append(1), real32(*a, **kw))[1]
        on = _run_blocks(blocks, feats0, go, swin, dt, seed)
    finally:
        P.residual_norm = real32
        layers.uninstall_fast_layers()
    assert not calls
    for name, a, b in zip(["output"] + _names(blocks), [on[0]] + on[1], [off[0]] + off[1]):
        assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), name
