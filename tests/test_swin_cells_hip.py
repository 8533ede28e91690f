"""GPU (-m gpu): the Swin3D variant on the cell path - index_build.swin_stage_index_hip(..., cell_table_rows=L): the per-point
quantisation, the pair list's rel-pos index and the cell plans by the HIP kernels of csrc/index.hip (swin_quant_kernel,
swin_pairs_rel_kernel, cell_fill_swin_kernel), and fused.cell_attention / cell_attention_qkv on those plans (31-row tables, cells
without sampled keys) against the operator chain on the same device index.

Bars (none new): cell against operator chain - forward rtol = atol = 1e-4, row gradients TOL, table gradients TTOL over their scale
(tests/test_hip_parity.py); packed rows - forward FTOL, row gradients GTOL widened by the one rounding of a half gradient (rtol 2^-10
fp16, 2^-7 bf16), tables TTOL (tests/test_cell_qkv_hip.py); the fixture's module output rtol 1e-4 / atol 2e-4 and the share of rel-pos
entries that differ from CPU torch < 1e-3 (test_swin3d_consumer_against_reference_golden).
"""
import os

import numpy as np
import pytest
import torch

from tests.cell_edges import _SCALES, _cell_operands, _np, _packed_operands
from tests.util import dev

pytestmark = pytest.mark.gpu

TOL = dict(rtol=2e-5, atol=2e-5)
TTOL = dict(rtol=2e-4, atol=2e-4)
FTOL = dict(rtol=2e-5, atol=1e-4)
GTOL = dict(rtol=2e-5, atol=2e-4)
_TABLES = ("table_q", "table_k", "table_v")
_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
L31, CAP = 31, 16
# the edge scene: two rooms of 800 and 400 points, windows of 0.2 with 16 quantisation steps (31-row tables)
EDGE_SIZES, EDGE_SEED, EDGE_W, EDGE_QUANT = [800, 400], 2, 0.2, 0.0125


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()
    return pointops


def _stage(xyz_np, offset_np, w, quant):
    from stratified_transformer_amd import index_build
    xyz, offset = dev(xyz_np), dev(offset_np)
    even, odd, _ = index_build.swin_stage_index_hip(xyz, offset, w, quant, cell_table_rows=L31, cell_max_queries=CAP)
    ws = torch.tensor([w] * 3).type_as(xyz)
    return dict(xyz=xyz, offset=offset, w=w, quant=quant, blocks=(even, odd), shifts=(0.0, 1 / 2 * ws))


@pytest.fixture(scope="module")
def fix(P):
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "swin3d_window_attention.npz")))
    s = _stage(g["xyz"], g["offset"], float(g["window_size"]), float(g["quant_size"]))
    s["g"] = g
    return s


@pytest.fixture(scope="module")
def edge(P):
    from stratified_transformer_amd import scene
    xyz, offset = scene.make_batch(EDGE_SIZES, seed=EDGE_SEED)
    return _stage(xyz, offset, EDGE_W, EDGE_QUANT)


# ---- 1. the index ---------------------------------------------------------------------------------------------------------------
def _check_rel_is_torchs(s):
    """rel_idx of the pair kernel == swin_rel_pos_index by torch ops on the device, bit for bit; inside the table"""
    from stratified_transformer_amd import index_build
    for blk, shift in zip(s["blocks"], s["shifts"]):
        want = index_build.swin_rel_pos_index(s["xyz"], blk.index_0, blk.index_1, s["w"], s["quant"], shift)
        assert blk.rel_idx.dtype == torch.int32 and blk.rel_idx.shape == want.shape
        assert torch.equal(blk.rel_idx, want), int((blk.rel_idx != want).sum())
        assert int(blk.rel_idx.min()) >= 0 and int(blk.rel_idx.max()) <= L31 - 1


def test_fixture_index_both_patterns(fix):
    g = fix["g"]
    from stratified_transformer_amd import index_build
    assert index_build.swin_table_rows(fix["w"], fix["quant"]) == L31
    for pat, blk in enumerate(fix["blocks"]):
        assert np.array_equal(_np(blk.index_0), g[f"p{pat}_index_0"].astype(np.int32)) and np.array_equal(_np(blk.index_1), g[f"p{pat}_index_1"].astype(np.int32))
        assert np.array_equal(_np(blk.offsets), g[f"p{pat}_offsets"]) and int(blk.n_max) == int(g[f"p{pat}_n_max"])
        rel = _np(blk.rel_idx)
        assert rel.min() >= 0 and rel.max() <= 30
        assert (rel != g[f"p{pat}_rel_idx_cpu"].astype(np.int32)).mean() < 1e-3   # torch CPU vs torch GPU `%` / `//` at bin edges
    _check_rel_is_torchs(fix)


def test_edge_scene_index(edge):
    """The edge scene holds what it was chosen for - in both patterns a window of more than 64 points (the fill's second lane round), a
    window of exactly one point, windows of more than cell_max_queries points (cut cells), and two batch elements that share window
    coordinates but no pair - and its rel-pos index is torch's."""
    off = _np(edge["offset"])
    batch = np.searchsorted(off, np.arange(off[-1]), side="right")
    xyz = _np(edge["xyz"])
    for pat, blk in enumerate(edge["blocks"]):
        counts = np.diff(_np(blk.offsets))
        assert counts.max() > 64 and counts.min() == 1 and (counts == 1).sum() >= 1, (pat, counts.max(), counts.min())
        plan = blk.cells
        assert plan.n_cells > plan.n_parents and np.diff(_np(plan.cell_qstart)[: plan.n_cells + 1]).max() == CAP
        i0, i1 = _np(blk.index_0), _np(blk.index_1)
        assert np.array_equal(batch[i0], batch[i1])                     # no pair across the batch boundary ...
        vox = np.floor((xyz - xyz.min(0) + (0.5 * np.float32(EDGE_W) if pat else 0.0)) / np.float32(EDGE_W)).astype(np.int64)
        key = (vox[:, 0] * 1000 + vox[:, 1]) * 1000 + vox[:, 2]
        assert np.intersect1d(key[batch == 0], key[batch == 1]).size > 0   # ... although the two rooms meet in space
    _check_rel_is_torchs(edge)


# ---- 2. the plan is the pair list -------------------------------------------------------------------------------------------------
def _check_plan(blk):
    plan = blk.cells
    n = plan.n_points
    assert plan.table_rows == L31 and plan.max_queries == CAP
    nC = plan.n_cells
    qstart, kbase, pbase = (_np(t) for t in (plan.cell_qstart, plan.cell_kbase, plan.cell_pbase))
    order, keys, relp = _np(plan.cell_order), _np(plan.cell_keys), _np(plan.relp).view(np.uint32)
    offs, i0, i1, rel = _np(blk.offsets), _np(blk.index_0), _np(blk.index_1), _np(blk.rel_idx)
    assert np.array_equal(np.sort(order), np.arange(n)) and qstart[nC] == n
    assert kbase[nC] == plan.n_keyslots and pbase[nC] == plan.n_pairs == i1.shape[0]   # no sampled keys: every tile entry is a pair
    assert np.array_equal(_np(plan.kcell)[: plan.n_keyslots], np.repeat(np.arange(nC), np.diff(kbase[: nC + 1])))
    for c in range(nC):
        nq, nk = qstart[c + 1] - qstart[c], kbase[c + 1] - kbase[c]
        assert 1 <= nq <= CAP
        ck = keys[kbase[c]: kbase[c + 1]]
        tile = relp[pbase[c]: pbase[c] + nq * nk].reshape(nq, nk)
        assert not (tile >> 31).any() and not ((tile >> 24) & 127).any()
        for il, qi in enumerate(order[qstart[c]: qstart[c + 1]]):
            a, b = offs[qi], offs[qi + 1]
            assert b - a == nk and np.array_equal(ck, i1[a:b]) and (i0[a:b] == qi).all()   # the key list: the query's segment, in order
            got = np.stack([tile[il] & 255, (tile[il] >> 8) & 255, (tile[il] >> 16) & 255], 1).astype(np.int32)
            assert np.array_equal(got, rel[a:b]), (c, int(qi))


def test_fixture_plan_is_the_pair_list(fix):
    for blk in fix["blocks"]:
        _check_plan(blk)


def test_edge_scene_plan_is_the_pair_list(edge):
    for blk in edge["blocks"]:
        _check_plan(blk)


# ---- 3. numbers -------------------------------------------------------------------------------------------------------------------
def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _op_chain(P, q, k, v, tq, tk, tv, blk):
    a = P.attention_step1_v2(q, k, blk.index_1, blk.offsets, 0) + P.dot_prod_with_idx_v3(q, blk.offsets, 0, k, blk.index_1, tq, tk, blk.rel_idx)
    return P.attention_step2_with_rel_pos_value_v2(P.segment_softmax(a, blk.offsets), v, blk.offsets, 0, blk.index_1, tv, blk.rel_idx)


def _table_close(got, want, what):
    s = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(got / s, want / s, err_msg=what, **TTOL)


def _check_cell_attention(P, blk, h, seed):
    from stratified_transformer_amd import fused
    p, go = _cell_operands(blk.cells.n_points, h, L31, seed)
    names = ("q", "k", "v") + _TABLES
    want_l, got_l = [_leaf(dev(p[x])) for x in names], [_leaf(dev(p[x])) for x in names]
    want = _op_chain(P, *want_l, blk)
    got = fused.cell_attention(*got_l, blk.cells)
    np.testing.assert_allclose(_np(got), _np(want), rtol=1e-4, atol=1e-4)
    want.backward(dev(go))
    got.backward(dev(go))
    for name, a, b in zip(names, got_l, want_l):
        if name in _TABLES:
            _table_close(_np(a.grad), _np(b.grad), f"grad {name}")
        else:
            np.testing.assert_allclose(_np(a.grad), _np(b.grad), err_msg=f"grad {name}", **TOL)


def _check_cell_attention_qkv(P, blk, h, seed, dtype):
    from stratified_transformer_amd import fused
    td, scale = _DTYPES[dtype], _SCALES[dtype]
    qkv, tabs, go = _packed_operands(blk.cells.n_points, h, L31, seed, td)
    # the chain's operands as the model hands them over: (query * scale) taken by torch in qkv's dtype, then widened
    rows = [_leaf((qkv[:, 0] * scale).float().contiguous()), _leaf(qkv[:, 1].float().contiguous()), _leaf(qkv[:, 2].float().contiguous())]
    wt = [_leaf(t) for t in tabs]
    want = _op_chain(P, *rows, *wt, blk)
    leaf, gt = _leaf(qkv), [_leaf(t) for t in tabs]
    got = fused.cell_attention_qkv(leaf, scale, *gt, blk.cells)
    assert got.dtype == torch.float32
    np.testing.assert_allclose(_np(got), _np(want), err_msg=f"{dtype} forward", **FTOL)
    want.backward(dev(go))
    got.backward(dev(go))
    assert leaf.grad.dtype == td
    gtol = dict(GTOL, rtol={"float32": GTOL["rtol"], "float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}[dtype])
    g = _np(leaf.grad.float())
    np.testing.assert_allclose(g[:, 0], np.float32(scale) * _np(rows[0].grad), err_msg=f"{dtype} grad q", **gtol)
    np.testing.assert_allclose(g[:, 1], _np(rows[1].grad), err_msg=f"{dtype} grad k", **gtol)
    np.testing.assert_allclose(g[:, 2], _np(rows[2].grad), err_msg=f"{dtype} grad v", **gtol)
    for name, a, b in zip(_TABLES, gt, wt):
        _table_close(_np(a.grad), _np(b.grad), f"{dtype} grad {name}")


def test_fixture_cell_attention_matches_the_operator_chain(P, fix):
    for pat, blk in enumerate(fix["blocks"]):
        _check_cell_attention(P, blk, 3, 40 + pat)


@pytest.mark.parametrize("dtype", list(_DTYPES))
def test_fixture_cell_attention_qkv_matches_the_operator_chain(P, fix, dtype):
    for pat, blk in enumerate(fix["blocks"]):
        _check_cell_attention_qkv(P, blk, 3, 50 + pat, dtype)


def test_edge_scene_cell_attention_matches_the_operator_chain(P, edge):
    for pat, blk in enumerate(edge["blocks"]):
        _check_cell_attention(P, blk, 2, 60 + pat)


@pytest.mark.parametrize("dtype", list(_DTYPES))
def test_edge_scene_cell_attention_qkv_matches_the_operator_chain(P, edge, dtype):
    for pat, blk in enumerate(edge["blocks"]):
        _check_cell_attention_qkv(P, blk, 2, 70 + pat, dtype)


def test_fixture_module_output_on_the_device_index(P, fix):
    """the reference module's output (swin3d_transformer.py:143-176, recorded in the fixture) from the operator chain on the DEVICE-built
    pair list and rel-pos index, and from the cell kernels on the plan"""
    from stratified_transformer_amd import fused
    g = fix["g"]
    N, C = g["feats"].shape
    h = g["table_q"].shape[1]
    tabs = [dev(g[x]) for x in _TABLES]
    qkv = torch.nn.functional.linear(dev(g["feats"]), dev(g["qkv_weight"]), dev(g["qkv_bias"])).reshape(N, 3, h, C // h).permute(1, 0, 2, 3).contiguous()
    q, k, v = qkv[0] * (C // h) ** -0.5, qkv[1], qkv[2]
    for pat, blk in enumerate(fix["blocks"]):
        x = _op_chain(P, q, k, v, *tabs, blk)
        y = torch.nn.functional.linear(x.view(N, C), dev(g["proj_weight"]), dev(g["proj_bias"]))
        np.testing.assert_allclose(_np(y), g[f"p{pat}_out"], rtol=1e-4, atol=2e-4)
        xc = fused.cell_attention(q, k, v, *tabs, blk.cells)
        np.testing.assert_allclose(_np(xc), _np(x), rtol=1e-4, atol=1e-4)


# ---- 5. argument errors -------------------------------------------------------------------------------------------------------------
def test_swin_launchers_record_errors(fix):
    from stratified_transformer_amd import _lib, index_build
    d = fix["xyz"].device
    blk = fix["blocks"][0]
    plan = blk.cells
    n, ptr = plan.n_points, _lib.ptr
    q = torch.zeros(n, 3, dtype=torch.int32, device=d)
    bbox = torch.zeros(6, device=d)
    rel = torch.zeros_like(blk.rel_idx)
    M = int(blk.index_0.shape[0])
    with pytest.raises(RuntimeError, match="swin_quant"):
        _lib.call("pointops2_swin_quant_launcher", -1, ptr(fix["xyz"]), ptr(bbox), 0.16, 0.01, 0, ptr(q), device=d)
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("pointops2_swin_quant_launcher", n, ptr(fix["xyz"]), None, 0.16, 0.01, 0, ptr(q), device=d)
    with pytest.raises(RuntimeError, match="swin_pairs_rel"):
        _lib.call("pointops2_swin_pairs_rel_launcher", n, -1, ptr(blk.index_0), ptr(blk.index_1), ptr(q), 16, ptr(rel), device=d)
    with pytest.raises(RuntimeError, match="1..255"):
        _lib.call("pointops2_swin_pairs_rel_launcher", n, M, ptr(blk.index_0), ptr(blk.index_1), ptr(q), 129, ptr(rel), device=d)
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("pointops2_swin_pairs_rel_launcher", n, M, ptr(blk.index_0), ptr(blk.index_1), None, 16, ptr(rel), device=d)
    keys, kcell, relp = torch.zeros_like(plan.cell_keys), torch.zeros_like(plan.kcell), torch.zeros_like(plan.relp)
    wc = torch.zeros(n, 3, device=d)
    ls = torch.zeros(1, dtype=torch.int32, device=d)
    s_order = fix["blocks"][0].parts["small"].order

    def fill(npts, rows, qq):
        _lib.call("pointops2_swin_cell_fill_launcher", npts, rows, 16, qq, ptr(s_order), ptr(ls), ptr(wc), ptr(plan.cell_order), ptr(plan.qcell),
                  ptr(plan.cell_qstart), ptr(plan.cell_desc), ptr(plan.cell_kbase), ptr(plan.cell_pbase), ptr(keys), ptr(kcell), ptr(relp), device=d)
    with pytest.raises(RuntimeError, match="swin_cell_fill"):
        fill(-1, L31, ptr(q))
    for rows in (0, 256):
        with pytest.raises(RuntimeError, match="1..255"):
            fill(n, rows, ptr(q))
    with pytest.raises(RuntimeError, match="null"):
        fill(n, L31, None)
    torch.cuda.synchronize()
    assert not keys.any() and not relp.any() and not rel.any()          # a refused launch wrote nothing
    with pytest.raises(ValueError, match="cell_table_rows"):
        index_build.swin_stage_index_hip(fix["xyz"], fix["offset"], fix["w"], fix["quant"], cell_table_rows=32)
