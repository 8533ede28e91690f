"""GPU (-m gpu): the cell attention where random finite rows with logits of a few units cannot show an error (helpers and their CPU
checks: tests/cell_edges.py, tests/test_cell_edges_cpu.py).

A. One non-finite operand row per run (v = +inf, k = NaN, q = NaN, grad_out = +inf; row 0 - which every padded key or query slot of
   the kernels reads -, the last key of a cell whose key count is no multiple of 16, row n - 1).  Expected: the oracle's operator chain
   on the same operands.  out / grad_q / grad_k / grad_v: the set of non-finite rows equals the oracle's exactly and every other row
   is within the standing bars (forward rtol 2e-5 / atol 1e-4, gradients atol 2e-4).  Table gradients (histogram x rows on the matrix
   cores: a NaN row spreads over its product tile): wholly finite and within TTOL where the oracle's is, at least one
   non-finite entry where the oracle's has one.
B. q scaled by 16 (64 on two scenes): at least a quarter of the oracle's softmax weights are exactly 0, some row is one-hot, and in the
   multi-chunk scenes (a planted key) rows whose maximum lies in the first / the last chunk and rows whose running maximum rises by
   more than 88 between two chunks.  The oracle is fp32 and an absolute logit error of s * eps is a relative weight error, so kernel
   and oracle are both compared with the float64 restatement: max|kernel - f64| <= max(standing bar, 4 * max|oracle - f64|) per
   output.  Measured ratios: DESIGN.md 4.6.

Every instance runs on the even and the odd pattern of the smallest scene of _CELL_VARIANT_SCENES that reaches it.
"""
import numpy as np
import pytest
import torch

from tests import cell_edges as ce
from tests.cell_edges import _SCALES, _TABLES, _np
from tests.util import dev

pytestmark = pytest.mark.gpu

# instance: (scene, launcher, row type of the packed launchers, expected forward variant (None: the scene's fp32 variants), backward)
_INSTANCES = {
    "fp32_mfma64": ("mfma64_h1", "fp32", None, None, True),
    "fp32_mfma80": ("mfma80_h3", "fp32", None, None, True),
    "fp32_valu80_single_chunk": ("stage0_h3_cap8", "fp32", None, None, True),
    "fp32_valu80_multi_chunk": ("two_chunks_L80_h8_cap8", "fp32", None, None, True),
    "fp32_valu160_L96_forward": ("L96", "fp32", None, "valu160", False),
    "bf16_valu80_L64_TA4": ("mfma64_h1", "bf16", None, "valu80", True),
    "bf16_valu80_L80_TA5": ("mfma80_h3", "bf16", None, "valu80", True),
    "packed_fp16_mfma64": ("mfma64_h1", "packed", "float16", None, True),
    "packed_bf16_mfma64": ("mfma64_h1", "packed", "bfloat16", None, True),
    "packed_fp16_valu80": ("stage0_h3_cap8", "packed", "float16", None, True),
    "packed_bf16_valu80": ("stage0_h3_cap8", "packed", "bfloat16", None, True),
    "packed_fp32_mfma80": ("mfma80_h3", "packed", "float32", None, True),
}
_MULTI_CHUNK = ("two_chunks_L80_h8_cap8", "L96")
_ROW0_RUNS = [(kind, "row0") for kind in ce.POISONS] + [("v_inf", "last_key_of_ragged_cell"), ("k_nan", "last_row")]
_ALL_RUNS = [(kind, row) for kind in ce.POISONS for row in ("row0", "last_key_of_ragged_cell", "last_row")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()


def _scene(name):
    """(even, odd) blocks, expected fp32 variants, L, h; every pattern holds a cell with nk % 16 != 0 and a piece with nq % 16 != 0"""
    if name == "L96":
        _, _, even, odd = ce._cell_scene(4000, 1, 0.24, 0.01, seed=96, L=96, cap=16)
        blocks, variants, L, h = (even, odd), ("valu160", "valu160"), 96, 3
        assert even.cells.nk_max > 128
        nk = ce._cell_nk(even.cells)
        assert ((nk > 128) & (nk % 16 != 0)).any()
    else:
        blocks, variants, L, h = ce._variant_scene(name)
    for blk in blocks:
        assert (ce._cell_nk(blk.cells) % 16 != 0).any() and (ce._cell_nq(blk.cells) % 16 != 0).any()
    return blocks, variants, L, h


def _raw_operands(n, h, L, seed):
    """standard normal q, k, v, grad_out, tables of half that scale: the standing operand distribution"""
    return ce._cell_operands(n, h, L, seed)


def _run(inst, blk, L, p, go, s=1.0):
    """One instance on raw operands `p` (numpy; q scaled by s, by the launch scale for the packed launchers) and grad_out `go` (None:
    forward only).  Returns the kernel's results (out, q, k, v -> [n, h, 16]; the table gradients), the operand dict the oracle and the
    float64 chain take, and the factor on their grad_q (the packed launchers differentiate to the raw q)."""
    _, launcher, dtype, _, _ = _INSTANCES[inst]
    plan = blk.cells
    if launcher == "packed":
        td = ce._dtypes()[dtype]
        scale = _SCALES[dtype] * (1.0 if s == 1.0 else 4.0 * s)  # B: 64 * _SCALES at s = 16 (q' = 16, 19.2, 12.2 times a standard normal)
        qkv = dev(np.stack([p["q"], p["k"], p["v"]], axis=1)).to(td).contiguous()
        tabs = [dev(p[t]) for t in _TABLES]
        out, _, g = ce._qkv_launch(plan, qkv, scale, tabs, L, go)
        rows = dict(out=_np(out))
        if g is not None:
            gq = _np(g["qkv"])
            rows.update(q=gq[:, 0], k=gq[:, 1], v=gq[:, 2])
        return rows, ({t: _np(g[t]) for t in _TABLES} if g else {}), ce._oracle_operands(qkv, scale, tabs), np.float32(scale)
    q = p["q"] * np.float32(s)
    ops = [dev(x) for x in (q, p["k"], p["v"], p["table_q"], p["table_k"], p["table_v"])]
    if launcher == "bf16":
        ops = [t.bfloat16() for t in ops]
    pw = {x: _np(t.float()) for x, t in zip(ce._CELL_GRADS, ops)}
    out, g = ce._cell_launch(plan, ops, L, go)
    rows = dict(out=_np(out))
    if g is not None:
        rows.update({x: _np(g[x]) for x in ("q", "k", "v")})
    return rows, ({t: _np(g[t]) for t in _TABLES} if g else {}), pw, np.float32(1.0)


def _oracle(pw, i1, offs, rel, go, qfac, sm=None):
    out, g = ce._oracle_attention(pw, i1, offs, rel, go, sm=sm)
    rows = dict(out=out)
    if g is not None:
        rows.update(q=qfac * g["q"], k=g["k"], v=g["v"])
    return rows, ({t: g[t] for t in _TABLES} if g else {})


def _expect_variant(inst, blk, variant, h, L):
    """asserts the forward instance the launcher picks for this pattern; returns its name"""
    from stratified_transformer_amd import _lib
    _, launcher, _, expect, _ = _INSTANCES[inst]
    expect = expect or variant
    got = _lib.cell_forward_variant(blk.cells, h, L, bf16=launcher == "bf16")
    assert got == expect, (inst, got, expect)
    return got


@pytest.mark.parametrize("inst", list(_INSTANCES))
def test_one_nonfinite_row_stays_in_its_window_and_reaches_the_gradients(inst):
    """Contract A of the module docstring on every forward instance and its backward, even and odd pattern."""
    scene, launcher, _, _, backward = _INSTANCES[inst]
    blocks, variants, L, h = _scene(scene)
    n = blocks[0].cells.n_points
    p, go = _raw_operands(n, h, L, seed=h + 40)
    for blk, variant in zip(blocks, variants):
        variant = _expect_variant(inst, blk, variant, h, L)
        plan = blk.cells
        i0, i1, offs, rel = ce._pair_list(blk, L)
        targets = ce.poison_rows(ce._cell_nk(plan), _np(plan.cell_kbase), _np(plan.cell_keys), n)
        # the standing distribution: no weight underflows, so the oracle has no 0 * inf of its own
        _, _, pw, _ = _run(inst, blk, L, p, None)
        sm = ce._oracle_softmax(pw, i1, offs, rel)
        assert np.isfinite(sm).all() and (sm > 0).all()
        for kind, where in _ALL_RUNS:
            if kind == "go_inf" and not backward:
                continue
            r = targets[where]
            pp, gg = ce.poison(p, go, kind, r)
            rows, tabs, pw, qfac = _run(inst, blk, L, pp, gg if backward else None)
            # (a v or grad_out row does not enter the softmax: the oracle's weights of the clean operands stand)
            want_rows, want_tabs = _oracle(pw, i1, offs, rel, gg if backward else None, qfac, sm=sm if kind in ("v_inf", "go_inf") else None)
            pred_rows, pred_tabs = ce.predicted_nonfinite(n, i0, i1, kind, r)
            for name in want_rows:  # the oracle's sets are the ones tests/test_cell_edges_cpu.py derives from the pair list
                assert np.array_equal(ce.nonfinite_rows(want_rows[name]), pred_rows[name]), (inst, kind, where, name)
            for name in want_tabs:
                assert (not np.isfinite(want_tabs[name]).all()) == pred_tabs[name], (inst, kind, where, name)
            ce.check_poisoned(f"{inst} {variant} {kind} at {where} ({r})", rows, tabs, want_rows, want_tabs)


_S64 = ("fp32_mfma64", "fp32_valu80_multi_chunk")


@pytest.mark.parametrize("inst,s", [(i, 16.0) for i in _INSTANCES] + [(i, 64.0) for i in _S64])
def test_saturated_softmax_against_the_float64_chain(inst, s):
    """Contract B of the module docstring.  Ratios max|kernel - f64| / max|oracle - f64| measured on the MI355X (the table per instance
    and output is in DESIGN.md 4.6): between 0.54 and 1.91 over every launcher, output and pattern at s = 16, between 0.81 and 1.83 at
    s = 64; K = 4 was never approached.  The oracle's own distance from float64 at s = 16: out 3e-5 .. 1.1e-4, grad_k 1e-3 .. 6.5e-3."""
    scene, launcher, _, _, backward = _INSTANCES[inst]
    blocks, variants, L, h = _scene(scene)
    n = blocks[0].cells.n_points
    multi = scene in _MULTI_CHUNK
    for blk, variant in zip(blocks, variants):
        variant = _expect_variant(inst, blk, variant, h, L)
        p, go = _raw_operands(n, h, L, seed=h + 50)
        if multi:
            ce.plant_late_maximum(p["k"], blk.cells)
        i0, i1, offs, rel = ce._pair_list(blk, L)
        rows, tabs, pw, qfac = _run(inst, blk, L, p, go if backward else None, s=s)
        sm = ce._oracle_softmax(pw, i1, offs, rel)
        want_rows, want_tabs = _oracle(pw, i1, offs, rel, go if backward else None, qfac, sm=sm)
        out64, g64, lg = ce.attention_f64(pw, i0, i1, offs, rel, go if backward else None)
        slot, nk = ce.pair_slots(blk.cells) if multi else (None, None)
        res = ce.saturation_conditions(lg, sm, offs, slot, nk)
        print(f"{inst} {variant} s={s}: {res}")
        ce.assert_saturated(res, multi_chunk=multi)
        f64 = dict(out=out64)
        if backward:
            f64.update(q=float(qfac) * g64["q"], k=g64["k"], v=g64["v"], **{t: g64[t] for t in _TABLES})
        ce.check_against_f64(f"{inst} {variant} s={s}", dict(rows, **tabs), dict(want_rows, **want_tabs), f64, ce.standing_bars(backward))


def _autograd_case():
    blocks, variants, L, h = _scene("mfma64_h1")
    blk = blocks[0]
    n = blk.cells.n_points
    p, go = _raw_operands(n, h, L, seed=h + 60)
    return blk, L, h, n, p, go


@pytest.mark.parametrize("api", ["cell_attention", "cell_attention_qkv_fp16", "window_attention"])
def test_fused_entry_points_keep_the_nonfinite_contract_through_autograd(api):
    """fused.cell_attention, fused.cell_attention_qkv (fp16 qkv: the poison must survive the dtype round of qkv.grad; finite rows within
    one fp16 rounding, rtol 2^-10, of the standing bars) and fused.window_attention (the pair-list form: the two attention paths are held
    to one rule), every poison at row 0 and v = inf at the last key of a ragged cell; then s = 16 against the float64 chain (measured
    ratios at most 1.39, except the fp16 qkv.grad: 41 .. 83 on the row gradients, the one fp16 rounding of a gradient of magnitude 200
    against an oracle 2e-3 from float64 - that case holds on the standing bar with the fp16 unit roundoff)."""
    from stratified_transformer_amd import fused
    blk, L, h, n, p, go = _autograd_case()
    plan = blk.cells
    i0, i1, offs, rel = ce._pair_list(blk, L)
    half = api == "cell_attention_qkv_fp16"
    scale = _SCALES["float16"]

    def run(p, go, scale):
        tl = [dev(p[t]).requires_grad_(True) for t in _TABLES]
        if half:
            leaf = dev(np.stack([p["q"], p["k"], p["v"]], axis=1)).half().contiguous().requires_grad_(True)
            out = fused.cell_attention_qkv(leaf, scale, *tl, plan)
            pw = ce._oracle_operands(leaf.detach(), scale, [t.detach() for t in tl])
        else:
            leaves = [dev(p[x]).requires_grad_(True) for x in ("q", "k", "v")]
            if api == "cell_attention":
                out = fused.cell_attention(*leaves, *tl, plan)
            else:
                out = fused.window_attention(*leaves, *tl, blk.offsets, blk.index_1, dev(rel))
            pw = {x: p[x] for x in ce._CELL_GRADS}
        out.backward(dev(go))
        if half:
            assert leaf.grad.dtype == torch.float16
            g = _np(leaf.grad.float())
            rows = dict(out=_np(out), q=g[:, 0], k=g[:, 1], v=g[:, 2])
        else:
            rows = dict(out=_np(out), **{x: _np(t.grad) for x, t in zip(("q", "k", "v"), leaves)})
        return rows, {t: _np(x.grad) for t, x in zip(_TABLES, tl)}, pw

    targets = ce.poison_rows(ce._cell_nk(plan), _np(plan.cell_kbase), _np(plan.cell_keys), n)
    for kind, where in _ROW0_RUNS:
        pp, gg = ce.poison(p, go, kind, targets[where])
        rows, tabs, pw = run(pp, gg, scale)
        want_rows, want_tabs = _oracle(pw, i1, offs, rel, gg, np.float32(scale) if half else np.float32(1.0))
        ce.check_poisoned(f"{api} {kind} at {where}", rows, tabs, want_rows, want_tabs, grad_rtol=2.0 ** -10 if half else None)
    # saturated: q' = 16 (fp32) or 19.2 (fp16) times a standard normal
    ps = p if half else dict(p, q=p["q"] * np.float32(16.0))
    rows, tabs, pw = run(ps, go, 64 * scale)
    qfac = np.float32(64 * scale) if half else np.float32(1.0)
    sm = ce._oracle_softmax(pw, i1, offs, rel)
    want_rows, want_tabs = _oracle(pw, i1, offs, rel, go, qfac, sm=sm)
    out64, g64, lg = ce.attention_f64(pw, i0, i1, offs, rel, go)
    ce.assert_saturated(ce.saturation_conditions(lg, sm, offs), multi_chunk=False)
    f64 = dict(out=out64, q=float(qfac) * g64["q"], k=g64["k"], v=g64["v"], **{t: g64[t] for t in _TABLES})
    bars = ce.standing_bars()
    if half:  # qkv.grad is rounded once to fp16
        bars.update({x: (2.0 ** -10, ce.GTOL["atol"], False) for x in ("q", "k", "v")})
    ce.check_against_f64(f"{api} s=16", dict(rows, **tabs), dict(want_rows, **want_tabs), f64, bars)
