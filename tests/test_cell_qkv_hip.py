"""GPU (-m gpu): the cell attention on the packed qkv projection [N, 3, h, 16] (fp32, fp16 or bf16 rows, fp32 tables): the C-ABI
launchers cell_attention_qkv_{forward,backward}_launcher, fused.cell_attention_qkv, the installed WindowAttention.forward under
autocast, and pointops.interpolation / interpolation_v2 on a half `feat`.

The kernels widen the rows exactly and compute in fp32, and q is scaled as torch scales it (`query * self.scale` in q's dtype), so the
oracle is fed q' = (qkv[:, 0] * scale) computed by torch in the row dtype and widened, k and v widened, and the bars are those of the
fp32 kernels (tests/test_hip_parity.py::_cell_variant_vs_oracle): forward rtol 2e-5 / atol 1e-4, row gradients rtol 2e-5 / atol 2e-4,
TTOL on the table gradients over their scale.  (Scene builders and launch helpers: tests/cell_edges.py.)
"""
import os

import numpy as np
import pytest
import torch

from tests.cell_edges import (_CELL_VARIANT_SCENES, _SCALES, _cell_scene, _np, _oracle_attention, _oracle_operands, _packed_operands, _qkv_launch,
                              _variant_scene)
from tests.util import dev

pytestmark = pytest.mark.gpu

TTOL = dict(rtol=2e-4, atol=2e-4)
FTOL = dict(rtol=2e-5, atol=1e-4)
GTOL = dict(rtol=2e-5, atol=2e-4)
_TABLES = ("table_q", "table_k", "table_v")
_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()


def _unpacked_launch(plan, ops, L, go=None):
    """the existing fp32 launchers on q, k, v [n, h, 16] and the tables: out, pbuf, the six gradients"""
    from stratified_transformer_amd import _lib
    n, h, _ = ops[0].shape
    f32 = dict(dtype=torch.float32, device="cuda")
    out, ml, pbuf = torch.empty(n, h, 16, **f32), torch.empty(n, h, 2, **f32), torch.zeros(h, max(plan.n_pairs, 1), **f32)
    ptrs = [_lib.ptr(t) for t in ops]
    _lib.call("cell_attention_forward_launcher", plan.c_arg(), h, 16, L, *ptrs, _lib.ptr(out), _lib.ptr(ml), _lib.ptr(pbuf), device=out.device)
    if go is None:
        return out, pbuf, None
    gsbuf = torch.empty_like(pbuf)
    grads = [torch.empty(n, h, 16, **f32)] + [torch.zeros(t.shape, **f32) for t in ops[1:]]
    _lib.call("cell_attention_backward_launcher", plan.c_arg(), h, 16, L, _lib.ptr(dev(go)), *ptrs[:3], _lib.ptr(out), *ptrs[3:], _lib.ptr(pbuf),
              _lib.ptr(gsbuf), *[_lib.ptr(g) for g in grads], device=out.device)
    return out, pbuf, dict(zip(("q", "k", "v") + _TABLES, grads))


def _check_grads(got_qkv, got_tabs, want, scale, what):
    """got_qkv [n, 3, h, 16] against (scale * grad_q', grad_k, grad_v), the table gradients over their scale"""
    np.testing.assert_allclose(got_qkv[:, 0], np.float32(scale) * want["q"], err_msg=f"{what} grad q", **GTOL)
    np.testing.assert_allclose(got_qkv[:, 1], want["k"], err_msg=f"{what} grad k", **GTOL)
    np.testing.assert_allclose(got_qkv[:, 2], want["v"], err_msg=f"{what} grad v", **GTOL)
    for name in _TABLES:
        s = max(1.0, float(np.abs(want[name]).max()))
        np.testing.assert_allclose(got_tabs[name] / s, want[name] / s, err_msg=f"{what} grad {name}", **TTOL)


def _qkv_vs_oracle(blk, L, h, dtype, expect, seed, backward=True):
    from stratified_transformer_amd import _lib
    # the packed launchers run what pointops2_cell_forward_variant names for fp32 tables, whatever the rows' type
    got = _lib.cell_forward_variant(blk.cells, h, L, bf16=False)
    assert got == expect, (got, expect, blk.cells.n_points * h, blk.cells.n_pairs / max(blk.cells.n_keyslots, 1))
    scale = _SCALES[dtype]
    qkv, tabs, go = _packed_operands(blk.cells.n_points, h, L, seed, _DTYPES[dtype])
    out, _, grads = _qkv_launch(blk.cells, qkv, scale, tabs, L, go if backward else None)
    p = _oracle_operands(qkv, scale, tabs)
    i1, offs, rel = _np(blk.index_1), _np(blk.offsets), np.clip(_np(blk.rel_idx), 0, L - 1).astype(np.int32)
    want, wgrads = _oracle_attention(p, i1, offs, rel, go if backward else None)
    np.testing.assert_allclose(_np(out), want, err_msg=f"{expect} {dtype} forward", **FTOL)
    if backward:
        _check_grads(_np(grads["qkv"]), {t: _np(grads[t]) for t in _TABLES}, wgrads, scale, f"{expect} {dtype}")



@pytest.mark.parametrize("dtype", list(_DTYPES))
@pytest.mark.parametrize("case", list(_CELL_VARIANT_SCENES))
def test_packed_qkv_variant_matches_the_oracle(case, dtype):
    """Forward and backward of the packed launchers, every forward instance (MFMA64, MFMA80, VALU80 on both sides of n * h = 96000,
    cells of two and of three or more register chunks) and every row type, even and odd pattern, against the oracle's operator chain
    at the bars of the fp32 kernels; grad_qkv[:, 0] against scale * the oracle's grad_q.  The fp16 and bf16 scales are no powers of two."""
    blocks, variants, L, h = _variant_scene(case)
    for blk, variant in zip(blocks, variants):
        _qkv_vs_oracle(blk, L, h, dtype, variant, seed=h)


@pytest.mark.parametrize("case", list(_CELL_VARIANT_SCENES))
def test_packed_fp32_equals_the_unpacked_launchers(case):
    """fp32 rows: out and pbuf of the packed launcher equal those of cell_attention_forward_launcher on q * scale, k, v copied out of
    the same qkv, bit for bit (the existing launcher first reproduces itself over two runs); the gradients, summed with atomics, at
    the bars of the oracle comparison."""
    blocks, variants, L, h = _variant_scene(case)
    scale = 0.3  # the fp32 product is rounded: the kernel's q' must be torch's
    for blk in blocks:
        plan = blk.cells
        qkv, tabs, go = _packed_operands(plan.n_points, h, L, h + 1, torch.float32)
        ops = [(qkv[:, 0] * scale).contiguous(), qkv[:, 1].contiguous(), qkv[:, 2].contiguous()] + tabs
        out_a, pbuf_a, _ = _unpacked_launch(plan, ops, L)
        out_b, pbuf_b, grads_u = _unpacked_launch(plan, ops, L, go)
        assert torch.equal(out_a, out_b) and torch.equal(pbuf_a, pbuf_b), "the unpacked forward does not reproduce itself"
        out, pbuf, grads = _qkv_launch(plan, qkv, scale, tabs, L, go)
        assert torch.equal(out, out_a), float((out - out_a).abs().max())
        assert torch.equal(pbuf, pbuf_a), float((pbuf - pbuf_a).abs().max())
        want = {x: _np(grads_u[x]) for x in ("k", "v") + _TABLES}
        want["q"] = _np(grads_u["q"])  # dL/dq': _check_grads multiplies by scale
        _check_grads(_np(grads["qkv"]), {t: _np(grads[t]) for t in _TABLES}, want, scale, "packed vs unpacked")


@pytest.mark.parametrize("dtype", list(_DTYPES))
@pytest.mark.parametrize("L", [96, 160])
def test_packed_qkv_forward_with_more_than_80_table_rows(L, dtype):
    """the forward-only instance for 80 < L <= 160 on packed rows, against the oracle's forward chain"""
    n, h, w, quant = dict([(96, (4000, 3, 0.24, 0.01)), (160, (3000, 2, 0.2, 0.005))])[L]
    assert 2 * int((2 * w + 1e-4) // quant) == L
    _, _, even, odd = _cell_scene(n, 1, w, quant, seed=L, L=L, cap=16)
    if L == 96:
        assert even.cells.nk_max > 128, even.cells.nk_max
    for blk in (even, odd):
        _qkv_vs_oracle(blk, L, h, dtype, "valu160", seed=L, backward=False)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_cell_attention_qkv_autograd(dtype):
    """fused.cell_attention_qkv: qkv.grad has qkv's dtype and shape and is the launcher's fp32 buffer rounded once to that type (row
    bars widened by one rounding: rtol 2^-10 for fp16, 2^-7 for bf16; the accumulated k / v gradients differ run to run within the
    row bars); the table gradients are fp32.  Then the error paths."""
    from stratified_transformer_amd import fused
    n, h, w, quant, L = 4000, 3, 0.16, 0.01, 64
    _, _, even, _ = _cell_scene(n, 1, w, quant, seed=21, L=L, cap=16)
    plan, scale, td = even.cells, _SCALES[dtype], _DTYPES[dtype]
    qkv, tabs, go = _packed_operands(n, h, L, 22, td)
    out_c, _, grads_c = _qkv_launch(plan, qkv, scale, tabs, L, go)
    leaf = qkv.clone().requires_grad_(True)
    tl = [t.clone().requires_grad_(True) for t in tabs]
    out = fused.cell_attention_qkv(leaf, scale, *tl, plan)
    assert out.dtype == torch.float32 and out.shape == (n, h, 16)
    assert torch.equal(out, out_c)
    out.backward(dev(go))
    assert leaf.grad.dtype == td and leaf.grad.shape == qkv.shape
    rtol = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7, "float32": 2e-5}[dtype]
    np.testing.assert_allclose(_np(leaf.grad.float()), _np(grads_c["qkv"]), rtol=rtol, atol=2e-4)
    for t, name in zip(tl, _TABLES):
        assert t.grad.dtype == torch.float32
        s = max(1.0, float(grads_c[name].abs().max()))
        np.testing.assert_allclose(_np(t.grad) / s, _np(grads_c[name]) / s, **TTOL)
    # error paths
    with pytest.raises(RuntimeError, match=r"\[N, 3, h, 16\]"):
        fused.cell_attention_qkv(qkv.view(n, 3 * h, 16), scale, *tabs, plan)
    with pytest.raises(RuntimeError, match=r"\[N, 3, h, 16\]"):
        fused.cell_attention_qkv(qkv[:, :2].contiguous(), scale, *tabs, plan)
    with pytest.raises(RuntimeError, match="d != 16"):
        fused.cell_attention_qkv(qkv.view(n, 3, 2 * h, 8), scale, *tabs, plan)
    with pytest.raises(TypeError):
        fused.cell_attention_qkv(qkv, scale, *[t.half() for t in tabs], plan)
    with pytest.raises(RuntimeError, match="plan was built for"):
        fused.cell_attention_qkv(qkv[:-1].contiguous(), scale, *tabs, plan)
    short = [t[: L - 8].contiguous() for t in tabs]
    with pytest.raises(RuntimeError, match="table"):
        fused.cell_attention_qkv(qkv, scale, *short, plan)
    _, _, even96, _ = _cell_scene(n, 1, 0.24, 0.01, seed=3, L=96, cap=16)
    qkv96, tabs96, _ = _packed_operands(n, h, 96, 23, td)
    with torch.no_grad():
        assert bool(torch.isfinite(fused.cell_attention_qkv(qkv96, scale, *tabs96, even96.cells)).all())
    with pytest.raises(RuntimeError, match="80 table rows"):
        fused.cell_attention_qkv(qkv96.clone().requires_grad_(True), scale, *tabs96, even96.cells)


def test_packed_launchers_record_errors():
    """the C entry points themselves: unknown row_type, d != 16, tables of another row count than the plan's, L > 80 in the backward"""
    from stratified_transformer_amd import _lib
    n, h, L = 3000, 2, 64
    _, _, even, _ = _cell_scene(n, 1, 0.16, 0.01, seed=31, L=L, cap=16)
    plan = even.cells
    qkv, tabs, go = _packed_operands(n, h, L, 32, torch.float16)
    f32 = dict(dtype=torch.float32, device="cuda")
    out, ml, pbuf = torch.zeros(n, h, 16, **f32), torch.empty(n, h, 2, **f32), torch.zeros(h, plan.n_pairs, **f32)
    tp = [_lib.ptr(t) for t in tabs]

    def fwd(hdim, rows, rt):
        _lib.call("cell_attention_qkv_forward_launcher", plan.c_arg(), h, hdim, rows, _lib.ptr(qkv), rt, 0.25, *tp, _lib.ptr(out), _lib.ptr(ml),
                  _lib.ptr(pbuf), device=out.device)
    with pytest.raises(RuntimeError, match="row_type"):
        fwd(16, L, 3)
    with pytest.raises(RuntimeError, match="d != 16"):
        fwd(8, L, 1)
    with pytest.raises(RuntimeError, match="table_rows"):
        fwd(16, L - 8, 1)
    g = torch.zeros(n, 3, h, 16, **f32)
    gt = [torch.zeros(t.shape, **f32) for t in tabs]

    def bwd(rows, rt):
        _lib.call("cell_attention_qkv_backward_launcher", plan.c_arg(), h, 16, rows, _lib.ptr(dev(go)), _lib.ptr(qkv), rt, 0.25, _lib.ptr(out), *tp,
                  _lib.ptr(pbuf), _lib.ptr(pbuf.clone()), _lib.ptr(g), *[_lib.ptr(x) for x in gt], device=out.device)
    with pytest.raises(RuntimeError, match="row_type"):
        bwd(L, -1)
    with pytest.raises(RuntimeError, match="1..80"):
        bwd(96, 1)
    torch.cuda.synchronize()
    assert float(g.abs().max()) == 0.0  # a refused launch writes nothing


def _five_operators(q, k, v, tq, tk, tv, offs, i1, rel):
    """the reference's operator sequence (:183-208) through the operator API"""
    from stratified_transformer_amd import pointops as P
    n_max = (offs[1:] - offs[:-1]).max()
    a = P.attention_step1_v2(q, k, i1, offs, n_max) + P.dot_prod_with_idx_v3(q, offs, n_max, k, i1, tq, tk, rel)
    return P.attention_step2_with_rel_pos_value_v2(P.segment_softmax(a, offs), v, offs, n_max, i1, tv, rel)


def test_installed_layer_under_autocast_reads_the_half_qkv_in_place():
    """The stand-in BasicLayer of tests/golden/basic_layer_1400.npz (depth 2, TransitionDown, two batch elements) with the installed
    forwards, forward and backward, three times on the same weights and inputs:
      new       under torch.autocast(fp16): every block runs fused.cell_attention_qkv on the half qkv
      ops_amp   under torch.autocast(fp16) with the cell plans hidden and fused.window_attention replaced by the five operators of the
                operator API: the model's own glue (permute, scale, three casts) around the reference's operator sequence
      ops_fp32  the same without autocast
    new and ops_amp see the same half qkv and differ by the order of the sums and by where the q / k / v gradients are rounded to
    half.  The bar is not a number chosen in advance: |new - ops_amp| must stay below |ops_amp - ops_fp32|, the cost of autocast
    itself on code this path does not touch.  One figure each: the largest difference over the outputs, the input gradient and every
    parameter gradient, each over its tensor's largest magnitude.  Both are printed (DESIGN.md 4.6 records a run).
    Also: the packed Function ran once per block, fused.cell_attention not at all, and what it saved for the backward is qkv (half),
    the tables, out and pbuf - no fp32 [N, h, 16] copy of q, k or v."""
    import model_standin as ms
    from stratified_transformer_amd import fused, layers
    from stratified_transformer_amd import pointops as P
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "basic_layer_1400.npz"))
    scale, depth, C, C_out, h, k = (int(v) for v in g["config"])
    layer = ms.BasicLayer(scale, depth, C, h, float(g["window_size"]), float(g["quant_size"]), ratio=0.25, k=k, out_channels=C_out).cuda()
    layer.load_state_dict({n[6:]: torch.from_numpy(g[n]) for n in g.files if n.startswith("param.")}, strict=True)
    N = int(g["feats"].shape[0])
    calls = {"qkv": 0, "cell": 0, "ops": 0}
    saved = []
    real_qkv, real_cell, real_window, real_stage = fused.cell_attention_qkv, fused.cell_attention, fused.window_attention, layers.index_build.stage_index_hip

    def counting_qkv(qkv, *a, **kw):
        calls["qkv"] += 1
        assert qkv.dtype == torch.float16 and tuple(qkv.shape) == (N, 3, h, 16)
        kept = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (kept.append(t), t)[1], lambda t: t):
            out = real_qkv(qkv, *a, **kw)
        saved.append((qkv, out, kept))
        return out

    def counting_cell(*a, **kw):
        calls["cell"] += 1
        return real_cell(*a, **kw)

    def counting_ops(*a):
        calls["ops"] += 1
        return _five_operators(*a)

    def no_cells(*a, **kw):
        import dataclasses
        even, odd, rest = real_stage(*a, **kw)
        return dataclasses.replace(even, cells=None), dataclasses.replace(odd, cells=None), rest

    def run(amp, hide):
        P.clear_caches()
        layers.forget_clouds()
        layer.zero_grad(set_to_none=True)
        feats = dev(g["feats"]).requires_grad_(True)
        layers.index_build.stage_index_hip = no_cells if hide else real_stage
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            f, _, _, f_down, _, _ = layer(feats, dev(g["xyz"]), dev(g["offset"]))
        ((f.float() * dev(g["grad_out"])).sum() + (f_down.float() * dev(g["grad_out_down"])).sum()).backward()
        torch.cuda.synchronize()
        res = {"out": _np(f.float()), "out_down": _np(f_down.float()), "grad_feats": _np(feats.grad)}
        res.update({"grad." + name: _np(p.grad.float()) for name, p in layer.named_parameters()})
        return res

    fused.cell_attention_qkv, fused.cell_attention, fused.window_attention = counting_qkv, counting_cell, counting_ops
    try:
        assert layers.patch_classes(ms.BasicLayer, ms.WindowAttention) == [ms.BasicLayer, ms.WindowAttention]
        new = run(True, False)
        assert calls == {"qkv": depth, "cell": 0, "ops": 0}, calls
        ops_amp = run(True, True)
        assert calls == {"qkv": depth, "cell": 0, "ops": depth}, calls
        ops_fp32 = run(False, True)
        assert calls == {"qkv": depth, "cell": 0, "ops": 2 * depth}, calls
    finally:
        fused.cell_attention_qkv, fused.cell_attention, fused.window_attention = real_qkv, real_cell, real_window
        layers.index_build.stage_index_hip = real_stage
        layers.uninstall_fast_layers()
    # what the packed Function keeps for the backward
    assert len(saved) == depth
    for qkv, out, kept in saved:
        assert any(t.data_ptr() == qkv.data_ptr() and t.dtype == torch.float16 and tuple(t.shape) == (N, 3, h, 16) for t in kept)
        rows = [t for t in kept if t.dtype == torch.float32 and tuple(t.shape) == (N, h, 16)]
        assert len(rows) == 1 and rows[0].data_ptr() == out.data_ptr(), [tuple(t.shape) for t in kept]   # `out` alone
        assert len(kept) == 6, [(tuple(t.shape), t.dtype) for t in kept]  # qkv, three tables, out, pbuf

    def distance(a, b):
        worst, where = 0.0, None
        for name in b:
            assert a[name].shape == b[name].shape and np.isfinite(a[name]).all(), name
            d = float(np.abs(a[name] - b[name]).max()) / max(float(np.abs(b[name]).max()), 1e-6)
            if d > worst:
                worst, where = d, name
        return worst, where
    d_new, w_new = distance(new, ops_amp)
    d_amp, w_amp = distance(ops_amp, ops_fp32)
    print("autocast layer: |new - ops_amp| = %.3e (%s)   |ops_amp - ops_fp32| = %.3e (%s)" % (d_new, w_new, d_amp, w_amp))
    assert d_new < d_amp, (d_new, w_new, d_amp, w_amp)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_interpolation_accepts_a_half_feat(dtype):
    """pointops.interpolation / interpolation_v2 (Upsample under autocast, :341) on a half `feat`: the forward equals the fp32 call on
    feat.float() (the reference's loop promotes half x fp32 to fp32, :767-769); feat.grad has feat's dtype and is the fp32 gradient
    rounded once.  The backward kernel scatters with float atomics, so two fp32 runs differ by the order of ~12 terms of order 1
    (a few fp32 ulp: atol 1e-5) and a value that falls next to a rounding boundary may land on either neighbour: one ulp of the half
    type, rtol 2^-10 for fp16 and 2^-7 for bf16."""
    from stratified_transformer_amd import pointops as P
    td = _DTYPES[dtype]
    rng = np.random.default_rng(6)
    xyz = rng.random((3000, 3), dtype=np.float32)
    new_xyz = np.ascontiguousarray(xyz[::4])
    off, noff = dev(np.array([3000], np.int32)), dev(np.array([750], np.int32))
    feat = dev(rng.standard_normal((750, 24), dtype=np.float32)).to(td)
    go = dev(rng.standard_normal((3000, 24), dtype=np.float32))
    for fn in (P.interpolation, P.interpolation_v2):
        half, full = feat.clone().requires_grad_(True), feat.float().requires_grad_(True)
        got = fn(dev(new_xyz), dev(xyz), half, noff, off)
        want = fn(dev(new_xyz), dev(xyz), full, noff, off)
        assert got.dtype == torch.float32 and torch.equal(got, want), fn.__name__
        got.backward(go)
        want.backward(go)
        assert half.grad.dtype == td and half.grad.shape == feat.shape
        np.testing.assert_allclose(_np(half.grad.float()), _np(full.grad), rtol=2.0 ** (-10 if td == torch.float16 else -7), atol=1e-5, err_msg=fn.__name__)
