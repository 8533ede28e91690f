"""GPU (-m gpu): the index build (csrc/index.hip, index_build.py) and the data-side keys (csrc/dataprep.hip) on the clouds of
tests/index_cases.py - lattices, scenes away from the origin, degenerate extents - against oracle/index_ref.py.  Every comparison is
array_equal; the cell attention on duplicated pairs uses the standing bars of tests/cell_edges.py (FTOL rows, TTOL tables over scale).

What the census of a case counts (tests/test_index_cases_cpu.py holds the cases to it) is what these tests need the device to reproduce:
points whose partition window and window coordinate disagree, pairs listed twice, rel-pos indices outside [0, L)."""
import numpy as np
import pytest
import torch

from tests import index_cases as ic
from tests.cell_edges import FTOL, TTOL, _CELL_GRADS, _cell_launch, _cell_operands, _np, _oracle_attention, _pair_list, check_cell_plan_is_the_pair_list
from tests.util import dev

pytestmark = pytest.mark.gpu

FIELDS = ("index_0", "index_1", "offsets", "rel_idx")
_BLOCKS = {}


def _stage(name, cap=None):
    """(even, odd, parts) of stage_index_hip on a case; cap = None: no cell plans.  Built once per (case, cap)."""
    from stratified_transformer_amd import index_build
    if (name, cap) not in _BLOCKS:
        c = ic.case(name)
        kw = {} if cap is None else dict(cell_table_rows=ic.table_rows(c), cell_max_queries=cap)
        _BLOCKS[(name, cap)] = index_build.stage_index_hip(dev(c.xyz), dev(c.offset), c.w, c.quant, dev(ic.downsample(c)), **kw)
    return _BLOCKS[(name, cap)]


def _bbox(xyz):
    from stratified_transformer_amd import _lib
    bbox = torch.empty(6, dtype=torch.float32, device=xyz.device)
    _lib.call("pointops2_bbox_launcher", xyz.shape[0], _lib.ptr(xyz), _lib.ptr(bbox), device=xyz.device)
    return bbox


@pytest.mark.parametrize("name", ic.NAMES)
def test_partitions_equal_grid_sample(name):
    """The four partitions by one sort on the fixed-width key, by four sorts with host-sized keys, and the oracle's grid_sample:
    cluster, per-window counts, order, n_windows; no coordinate overflows the key."""
    from stratified_transformer_amd import index_build
    c = ic.case(name)
    xyz, off = dev(c.xyz), dev(c.offset)
    one = index_build.stage_partitions_hip(xyz, off, c.w, one_sort=True)
    four = index_build.stage_partitions_hip(xyz, off, c.w, one_sort=False)
    assert int(one["overflow"].item()) == 0 and four["overflow"] is None
    want = ic.oracle_partitions(name)
    for part in ic.PARTITIONS:
        cluster, counts, order = want[part]
        for how, ctx in (("one sort", one), ("four sorts", four)):
            got = ctx["parts"][part]
            nw = int(got.n_windows.item())
            assert nw == counts.shape[0], (part, how)
            assert np.array_equal(_np(got.cluster), cluster), (part, how)
            assert np.array_equal(np.diff(_np(got.starts)[: nw + 1]), counts), (part, how)
            assert np.array_equal(_np(got.order), order), (part, how)


@pytest.mark.parametrize("name", ic.NAMES)
def test_pair_lists_equal_the_oracle_and_the_torch_path(name):
    """index_0, index_1, offsets, n_max and the raw rel_idx (the -1 and >= L entries included) of stage_index_hip against
    index_ref.build_stage_indices(div_mode="cuda"), and against the torch-op path on the same device."""
    from stratified_transformer_amd import index_build
    c = ic.case(name)
    xyz, off, ds = dev(c.xyz), dev(c.offset), dev(ic.downsample(c))
    even, odd, _ = _stage(name)
    parts = index_build.stage_partitions(xyz, off, c.w)            # torch-op path on the same device
    for par, blk in enumerate((even, odd)):
        want = ic.oracle_block(name, par)
        for f in FIELDS:
            assert np.array_equal(_np(getattr(blk, f)), want[f]), (par, f)
        assert int(blk.n_max) == int(want["n_max"]), par
        stats = ic.census(name)[par]
        rel = _np(blk.rel_idx)
        assert (int(rel.min()), int(rel.max())) == (stats["rel_min"], stats["rel_max"])
        assert ic.duplicated_pairs(_np(blk.index_0), _np(blk.index_1), len(c.xyz)) == stats["duplicates"]
        s, l = ("small", "large") if par == 0 else ("small_shift", "large_shift")
        tb = index_build.build_block_index(xyz, parts[s], parts[l], ds, c.w, c.quant, par == 1)
        assert torch.equal(tb.index_0, blk.index_0) and torch.equal(tb.index_1, blk.index_1), par
        assert torch.equal(tb.rel_idx, blk.rel_idx) and torch.equal(tb.offsets, blk.offsets), par


@pytest.mark.parametrize("name", ic.NAMES)
def test_window_coordinate_bits_equal_the_oracle(name):
    """the wc buffer of pointops2_window_coord_launcher against index_ref.window_coord, as bit patterns (-0.0 is not +0.0)"""
    from oracle import index_ref
    from stratified_transformer_amd import _lib
    c = ic.case(name)
    xyz = dev(c.xyz)
    bbox = _bbox(xyz)
    assert np.array_equal(_np(bbox), np.concatenate([c.xyz.min(0), c.xyz.max(0)]))
    for shifted in (0, 1):
        wc = torch.full((len(c.xyz), 3), float("nan"), dtype=torch.float32, device=xyz.device)
        _lib.call("pointops2_window_coord_launcher", len(c.xyz), _lib.ptr(xyz), _lib.ptr(bbox), float(np.float32(c.w)), shifted, _lib.ptr(wc), device=xyz.device)
        want = index_ref.window_coord(torch.from_numpy(c.xyz), c.w, shifted == 1).numpy()
        got = _np(wc)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (shifted, int((got.view(np.int32) != want.view(np.int32)).sum()))


def _duplicated_entries(expanded, n):
    return ic.duplicated_pairs(expanded[:, 0], expanded[:, 1], n)


@pytest.mark.parametrize("cap", [0, 8])
@pytest.mark.parametrize("name", ic.NAMES)
def test_cell_plan_is_the_pair_list_on_every_case(name, cap):
    """the assertions of test_cell_plan_is_the_pair_list, against the clamped rel-pos index; and a point that is a dense and a
    stratified key of one query is in the tiles twice (the census count, from the oracle)"""
    c = ic.case(name)
    L = ic.table_rows(c)
    even, odd, _ = _stage(name, cap)
    for par, blk in enumerate((even, odd)):
        assert blk.cells.n_points == len(c.xyz) and blk.cells.table_rows == L
        got = check_cell_plan_is_the_pair_list(blk, L, cap)
        assert _duplicated_entries(got, len(c.xyz)) == ic.census(name)[par]["duplicates"], par
        want = ic.oracle_block(name, par)   # (the plan's pattern has the pair list of the plain build)
        for f in FIELDS:
            assert np.array_equal(_np(getattr(blk, f)), want[f]), (par, f)


@pytest.mark.parametrize("name", ic.NAMES)
def test_swin_index_and_cells_equal_the_oracle(name):
    """swin_stage_index_hip (device rel-pos index and cell plans) against index_ref.swin_stage_indices, both patterns: the pair
    list, the raw rel_idx, the per-point quantised coordinate of pointops2_swin_quant_launcher; the tiles are the pair list."""
    from stratified_transformer_amd import _lib, index_build
    c = ic.case(name)
    n = len(c.xyz)
    L = index_build.swin_table_rows(c.w, c.quant)
    xyz, off = dev(c.xyz), dev(c.offset)
    cap = 16
    even, odd, _ = index_build.swin_stage_index_hip(xyz, off, c.w, c.quant, cell_table_rows=L, cell_max_queries=cap)
    bbox = _bbox(xyz)
    for par, blk in enumerate((even, odd)):
        want = ic.oracle_swin_block(name, par)
        for f in FIELDS:
            assert np.array_equal(_np(getattr(blk, f)), want[f]), (par, f)
        assert int(blk.n_max) == int(want["n_max"]), par
        q = torch.full((n, 3), -99, dtype=torch.int32, device=xyz.device)
        _lib.call("pointops2_swin_quant_launcher", n, _lib.ptr(xyz), _lib.ptr(bbox), float(np.float32(c.w)), float(np.float32(c.quant)), par, _lib.ptr(q),
                  device=xyz.device)
        assert np.array_equal(_np(q), ic.oracle_swin_quant(c, par)), par
        got = check_cell_plan_is_the_pair_list(blk, L, cap)
        assert _duplicated_entries(got, n) == 0      # dense windows alone: no pair twice


@pytest.mark.parametrize("cap", [0, 16])
def test_cell_attention_on_duplicated_pairs_matches_the_oracle(cap):
    """lattice_far_origin, odd block: queries that list one key twice (once dense, once stratified), every rel-pos index inside the
    tables (tests/test_index_cases_cpu.py).  Forward and the six gradients of the cell kernels against the oracle's operator chain on
    the block's pair list: the key's weight, value and gradients count twice."""
    name, h = "lattice_far_origin", 3
    c = ic.case(name)
    n, L = len(c.xyz), ic.table_rows(c)
    blk = _stage(name, cap)[1]
    i0, i1, offs, rel = _pair_list(blk, L)
    raw = _np(blk.rel_idx)
    assert raw.min() >= 0 and raw.max() < L and L == 64
    assert ic.duplicated_pairs(i0, i1, n) == ic.census(name)[1]["duplicates"] > 0
    p, go = _cell_operands(n, h, L, seed=11 + cap)
    out, grads = _cell_launch(blk.cells, [dev(p[x]) for x in _CELL_GRADS], L, go)
    want, wgrads = _oracle_attention(p, i1, offs, rel, go)
    got = dict(out=_np(out), **{x: _np(grads[x]) for x in _CELL_GRADS})
    wgrads = dict(out=want, **wgrads)
    for x in ("out",) + _CELL_GRADS:
        scale = max(1.0, float(np.abs(wgrads[x]).max())) if x.startswith("table") else 1.0
        print(f"cap {cap} {x}: max |kernel - oracle| = {np.abs(got[x] - wgrads[x]).max() / scale:.3e} (over scale {scale:.3g})")
    for x in ("out",) + _CELL_GRADS:
        tol = TTOL if x.startswith("table") else FTOL
        scale = max(1.0, float(np.abs(wgrads[x]).max())) if x.startswith("table") else 1.0
        np.testing.assert_allclose(got[x] / scale, wgrads[x] / scale, err_msg=f"cap {cap} {x}", **tol)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_voxelize_and_crop_on_a_lattice_off_the_origin(dtype):
    """dataprep.voxel_keys, voxelize (modes 0 and 1) and crop_nearest on k * 0.04 + 17.3 shifted to minimum 0, where the floor of
    coord / voxel falls below the nearest integer for some k: device result == numpy restatement, bit for bit."""
    from oracle import index_ref
    from stratified_transformer_amd import dataprep
    coord = ic.data_lattice(np.dtype(dtype).type)
    assert ic.floors_below_nearest(coord[:, 0]) > 0
    voxel = ic.DATA_VOXEL
    c_d = torch.from_numpy(coord).cuda()
    keys = dataprep.voxel_keys(c_d, voxel).cpu().numpy().view(np.uint64)
    assert np.array_equal(keys, index_ref.fnv_hash_vec(np.floor(coord / np.asarray(voxel, dtype=coord.dtype))))
    idx_sort, count = dataprep.voxelize(c_d, voxel, mode=1)
    w_sort, w_count = index_ref.voxelize(coord, voxel, mode=1)
    assert w_count.max() > 1
    assert np.array_equal(idx_sort.cpu().numpy(), w_sort) and np.array_equal(count.cpu().numpy(), w_count)
    rand = np.random.default_rng(8).integers(0, int(w_count.max()), w_count.size)
    uniq = dataprep.voxelize(c_d, voxel, mode=0, rand=torch.from_numpy(rand).cuda())
    w_uniq = index_ref.voxelize(coord, voxel, mode=0, rand=rand)
    assert np.array_equal(uniq.cpu().numpy(), w_uniq)
    sub = np.ascontiguousarray(coord[w_uniq])
    seed = len(sub) // 2
    crop = dataprep.crop_nearest(torch.from_numpy(sub).cuda(), 8000, seed)
    assert np.array_equal(crop.cpu().numpy(), index_ref.crop_nearest(sub, 8000, seed))
