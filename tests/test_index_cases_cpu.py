"""CPU: the clouds of tests/index_cases.py hold what they were built for (conditions on the inputs, counted from the oracle alone),
and the torch-op path of index_build.py is the oracle on every one of them."""
import numpy as np
import pytest
import torch

from oracle import index_ref
from stratified_transformer_amd import index_build
from tests import index_cases as ic

FIELDS = ("index_0", "index_1", "offsets", "rel_idx")


def test_the_cases_are_seeded_float32_clouds_of_the_stated_sizes():
    for name in ic.NAMES:
        c = ic.case(name)
        assert c.name == name and c.xyz.dtype == np.float32 and c.offset.dtype == np.int32 and c.offset[-1] == len(c.xyz)
        assert (1600 if name != "extent_on_face" else 1000) <= len(c.xyz) <= 2400, (name, len(c.xyz))
        again = dict(zip(ic.NAMES, ic._BUILDERS))[name]()
        assert np.array_equal(again.xyz, c.xyz) and np.array_equal(again.offset, c.offset)
        ds = ic.downsample(c)
        assert ds.shape[0] == len(c.xyz) // 4 + len(c.offset) and np.all(np.diff(ds) > 0)
        if name != "flat_z":   # (its columns of cells collapse onto coincident points)
            assert len(np.unique(c.xyz, axis=0)) == len(c.xyz), name   # one point per cell
    assert ic.case("batch_mixed_origins").offset.tolist() == [800, 801, 1601]
    assert np.array_equal(ic.case("batch_mixed_origins").xyz[800], np.array([0.16, 0.32, 0.64], np.float32))
    assert (ic.case("lattice_negative").xyz < 0).all()
    assert np.unique(ic.case("flat_z").xyz[:, 2]).shape[0] == 1


def test_census_meets_the_purpose_of_every_case():
    stats = {name: ic.census(name) for name in ic.NAMES}
    print("\n" + ic.census_table())
    for name in ("lattice_far_origin", "batch_mixed_origins"):
        for par in (0, 1):
            assert stats[name][par]["disagree"] > 0 and stats[name][par]["duplicates"] > 0, (name, par, stats[name][par])
    for name in ("lattice_origin", "flat_z"):
        for par in (0, 1):
            assert stats[name][par]["on_face"] >= 0.10, (name, par, stats[name][par])
    for name in ("lattice_negative", "lattice_far_origin"):
        assert stats[name][0]["rel_outside"] > 0, (name, stats[name][0])
        assert stats[name][0]["rel_min"] < 0, (name, stats[name][0])
    # the control: exact arithmetic, the roundings cannot disagree
    for par in (0, 1):
        s = stats["pow2_lattice"][par]
        assert s["disagree"] == 0 and s["duplicates"] == 0 and s["rel_outside"] == 0, (par, s)
        assert s["on_face"] >= 0.10    # (it IS a lattice: the faces are populated, and still nothing diverges)
    # the cell-attention test on duplicated pairs runs the kernels on this block: every index inside the tables
    odd = stats["lattice_far_origin"][1]
    assert odd["duplicates"] > 0 and odd["rel_outside"] == 0 and odd["rel_min"] >= 0 and odd["rel_max"] < stats["lattice_far_origin"]["L"], odd
    assert stats["lattice_far_origin"]["L"] == 64
    # flat_z: no extent along z
    assert stats["flat_z"]["extent_w"][2] == 0 and stats["flat_z"]["extent_2w"][2] == 0
    # extent_on_face: the truncated quotient of the extent IS the number of windows, on every axis and for both window sizes
    e = stats["extent_on_face"]
    assert e["extent_2w"] == list(ic.EXTENT_BOXES) and e["extent_w"] == [2 * k for k in ic.EXTENT_BOXES], e
    c = ic.case("extent_on_face")
    parts = ic.oracle_partitions("extent_on_face")
    top = int(np.flatnonzero((c.xyz == c.xyz.max(0)).all(1))[0])   # the corner point: alone in the last window of both partitions
    for part in ("small", "large"):
        cluster, counts, _ = parts[part]
        assert cluster[top] == counts.shape[0] - 1 and counts[-1] == 1, part


@pytest.mark.parametrize("name", ic.NAMES)
def test_torch_op_path_equals_the_oracle(name):
    """index_build.stage_partitions + build_block_index on CPU tensors against index_ref.build_stage_indices(div_mode="cuda"): the four
    fields, n_max, n_dense, and the four partitions against grid_sample."""
    c = ic.case(name)
    x, ds = torch.from_numpy(c.xyz), torch.from_numpy(ic.downsample(c))
    parts = index_build.stage_partitions(x, torch.from_numpy(c.offset), c.w)
    want_parts = ic.oracle_partitions(name)
    for part in ic.PARTITIONS:
        cluster, counts, order = want_parts[part]
        got = parts[part]
        assert got.n_windows == counts.shape[0], part
        assert np.array_equal(got.cluster.numpy(), cluster) and np.array_equal(got.order.numpy(), order), part
        assert np.array_equal(np.diff(got.starts.numpy()), counts), part
    for par in (0, 1):
        want = ic.oracle_block(name, par)
        s, l = ("small", "large") if par == 0 else ("small_shift", "large_shift")
        tb = index_build.build_block_index(x, parts[s], parts[l], ds, c.w, c.quant, par == 1)
        for f in FIELDS:
            assert np.array_equal(getattr(tb, f).numpy(), want[f]), (par, f)
        assert int(tb.n_max) == int(want["n_max"])
        assert np.array_equal(tb.n_dense.numpy(), want_parts[s][1][want_parts[s][0]]), par   # dense keys: the query's whole window


@pytest.mark.parametrize("name", ic.NAMES)
def test_swin_rel_pos_index_equals_the_oracle(name):
    c = ic.case(name)
    x = torch.from_numpy(c.xyz)
    ws = torch.tensor([c.w] * 3).type_as(x)
    for par, shift in ((0, 0.0), (1, 1 / 2 * ws)):
        want = ic.oracle_swin_block(name, par)
        i0, i1 = torch.from_numpy(want["index_0"]), torch.from_numpy(want["index_1"])
        got = index_build.swin_rel_pos_index(x, i0, i1, c.w, c.quant, shift)
        assert np.array_equal(got.numpy(), want["rel_idx"]), par
        assert np.array_equal(index_ref.swin_rel_pos_index(x, i0, i1, c.w, c.quant, shift).numpy(), want["rel_idx"])
        q = ic.oracle_swin_quant(c, par)       # the per-point coordinate the device test compares: its differences are the index
        qgl = int(c.w / c.quant)
        assert np.array_equal(q[want["index_0"]] - q[want["index_1"]] + qgl - 1, want["rel_idx"]), par


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_data_side_lattice_has_floors_below_the_nearest_integer(dtype):
    """coord = k * 0.04 + 17.3 - min: np.floor(coord / voxel) - the voxel a point is kept or dropped on - falls one below the nearest
    integer for some k in either dtype; the 3-D set of the device test has such values too, and voxels with several points."""
    axis = ic.data_axis(np.dtype(dtype).type)
    below = ic.floors_below_nearest(axis)
    print(f"\n{dtype}: {below} of {ic.DATA_STEPS} floors below the nearest integer")
    assert axis.dtype == np.dtype(dtype) and below > 0
    coord = ic.data_lattice(np.dtype(dtype).type)
    assert coord.dtype == np.dtype(dtype) and coord.shape == (20000, 3) and (coord.min(0) == 0).all()
    assert ic.floors_below_nearest(coord[:, 0]) > 0
    _, count = index_ref.voxelize(coord, coord.dtype.type(ic.DATA_VOXEL), mode=1)
    assert count.max() > 1 and count.shape[0] < coord.shape[0]
