"""No GPU: the surface of the deterministic cell-attention backward - the exported symbols and their ctypes signatures, the ABI
version, the public `deterministic` argument and the two module switches - and the numpy restatement of the sequential sum that
tests/test_cell_det_hip.py holds the reduce kernels to."""
import ctypes
import inspect

import numpy as np

from tests import cell_det

NEW_LAUNCHERS = ("cell_key_grads_reduce_launcher", "cell_table_grads_reduce_launcher", "cell_attention_det_backward_launcher",
                 "cell_attention_det_backward_bf16_launcher", "cell_attention_qkv_det_backward_launcher")


def test_the_library_exports_the_deterministic_entry_points():
    from stratified_transformer_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_LAUNCHERS + ("pointops2_cell_table_partial_rows",):
        assert hasattr(raw, name), name
        assert name in _lib.exported_symbols(), name
    I, P, Z, F = _lib.I, _lib.P, _lib.Z, _lib.F
    tail = [P, P, P, Z, P, Z]  # slot_offsets, slot_order, key_partials, its floats, table_partials, its floats
    assert _lib.SIGNATURES["cell_attention_det_backward_launcher"] == _lib.SIGNATURES["cell_attention_backward_launcher"] + tail
    assert _lib.SIGNATURES["cell_attention_det_backward_bf16_launcher"] == _lib.SIGNATURES["cell_attention_backward_bf16_launcher"] + tail
    assert _lib.SIGNATURES["cell_attention_qkv_det_backward_launcher"] == _lib.SIGNATURES["cell_attention_qkv_backward_launcher"] + tail
    assert _lib.SIGNATURES["cell_key_grads_reduce_launcher"] == [I, I, P, P, P, P, I]
    assert _lib.SIGNATURES["cell_table_grads_reduce_launcher"] == [I, I, I, P, P, P, P]
    assert _lib.RESULTS["pointops2_cell_table_partial_rows"] == ([P, I], I)
    assert F in _lib.SIGNATURES["cell_attention_qkv_det_backward_launcher"]
    assert _lib.lib().pointops2_abi_version() == 5  # additions only: pointops2_cell_plan is unchanged


def test_partial_rows_is_host_arithmetic():
    """one workgroup per table body, head and CU at most, never more than the cells need: 1 for a plan of up to eight cells"""
    from stratified_transformer_amd import _lib, index_build
    plan = index_build.CellPlanStruct()
    plan.n_points, plan.n_cells = 100, 8
    rows = _lib.lib().pointops2_cell_table_partial_rows
    assert rows(ctypes.byref(plan), 3) == 1
    plan.n_cells = 9
    assert rows(ctypes.byref(plan), 3) == 2
    plan.n_cells = 10 ** 6
    many = rows(ctypes.byref(plan), 1)
    assert many >= 2 and rows(ctypes.byref(plan), 2) == max(1, many // 2)


def test_the_public_argument_and_the_switches():
    from stratified_transformer_amd import fused, index_build, layers
    for fn in (fused.cell_attention, fused.cell_attention_qkv):
        par = inspect.signature(fn).parameters
        assert "deterministic" in par and par["deterministic"].default is None, fn.__name__
    assert fused.DETERMINISTIC is False
    assert layers.DETERMINISTIC_ATTENTION is False
    fields = {f.name: f for f in index_build.CellPlan.__dataclass_fields__.values()}
    assert fields["key_view"].default is None


def test_sequential_sum_restatement_agrees_with_a_plain_loop():
    """20 slots over 7 keys (two without a slot, one with 9), rows scaled by 2^+-20 so that the order of the adds shows: the vectorised
    restatement equals the one-add-at-a-time loop bit for bit, and differs from the sum in sorted slot order."""
    rng = np.random.default_rng(5)
    counts = np.array([0, 3, 1, 0, 9, 2, 5])
    assert counts.sum() == 20
    offsets = np.r_[0, np.cumsum(counts)]
    order = rng.permutation(20)
    partials = cell_det.scaled_normals(rng, (20, 2, 16))
    got, want = cell_det.sequential_sum(partials, offsets, order), cell_det.sequential_sum_loop(partials, offsets, order)
    assert got.dtype == np.float32 and got.shape == (7, 2, 16)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[0].any() and not got[3].any()
    assert np.array_equal(got[2], partials[order[offsets[2]]])
    resorted = np.concatenate([np.sort(order[a:b]) for a, b in zip(offsets[:-1], offsets[1:])])
    other = cell_det.sequential_sum(partials, offsets, resorted)
    assert not np.array_equal(got.view(np.uint32), other.view(np.uint32)), "the operands do not show the order of the adds"
    # the ascending sum over rows and the image -> table layout
    rows = cell_det.scaled_normals(rng, (5, 3, 2 * 48))
    s = cell_det.ascending_sum(rows)
    assert np.array_equal(s, (((rows[0] + rows[1]) + rows[2]) + rows[3]) + rows[4])
    tab = cell_det.table_from_images(s, 2)
    assert tab.shape == (2, 3, 16, 3) and tab[1, 2, 5, 1] == s[2, 48 + 5 * 3 + 1]
