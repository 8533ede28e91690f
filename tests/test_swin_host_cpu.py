"""CPU: host logic of the Swin3D variant on the cell path - table rows, argument checks before any library call, the patch bookkeeping
of layers.patch_swin_classes, and a numpy restatement of the per-point quantisation the HIP kernel implements against the oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import index_ref
from stratified_transformer_amd import index_build, layers

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "swin3d_window_attention.npz")


@pytest.mark.parametrize("w,quant,rows", [(0.16, 0.01, 31), (0.32, 0.02, 31), (0.2, 0.0125, 31), (0.1, 0.005, 39), (0.4, 0.01, 79), (0.04, 0.04, 1)])
def test_swin_table_rows(w, quant, rows):
    assert index_build.swin_table_rows(w, quant) == rows == 2 * int(w / quant) - 1


def test_wrong_cell_table_rows_is_refused_before_any_device_work(monkeypatch):
    from stratified_transformer_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    xyz, offset = torch.zeros(10, 3), torch.tensor([10], dtype=torch.int32)
    for rows in (30, 32, 64, 0):
        with pytest.raises(ValueError, match="cell_table_rows"):
            index_build.swin_stage_index_hip(xyz, offset, 0.16, 0.01, cell_table_rows=rows, cell_max_queries=16)


def test_patch_and_unpatch_bookkeeping():
    class BL:
        def forward(self, feats, xyz, offset):
            return "bl"

    class WA:
        def forward(self, feats, xyz, index_0, index_0_offsets, n_max, index_1, shift_size):
            return "wa"

    class TD:
        def forward(self, feats, xyz, offset):
            return "td"

    class Module:
        BasicLayer, WindowAttention, TransitionDown = BL, WA, TD
    orig = (BL.forward, WA.forward, TD.forward)
    assert not layers._ORIGINAL
    try:
        assert layers.patch_swin_classes(BL, WA) == [BL, WA]
        assert BL.forward is layers.swin_basic_layer_forward and WA.forward is layers.swin_window_attention_forward and TD.forward is orig[2]
        assert layers.patch_swin_classes(BL, WA) == [BL, WA]                  # twice: the first originals are kept
        assert layers._ORIGINAL[BL, "forward"] is orig[0] and layers._ORIGINAL[WA, "forward"] is orig[1]
        # CPU tensors / a missing table: the installed forwards hand over to the originals
        wa = WA()
        wa.rel_query, wa.rel_key, wa.rel_value = True, True, True
        assert wa.forward(torch.zeros(2, 4), None, None, None, None, None, 0.0) == "wa"
        layers.uninstall_fast_layers()
        assert (BL.forward, WA.forward, TD.forward) == orig and not layers._ORIGINAL
        assert layers.install_swin_layers(Module) == [BL, WA, TD]
        assert TD.forward is layers.transition_down_forward
        assert TD().forward(torch.zeros(2, 4), torch.zeros(2, 3), torch.tensor([2])) == "td"
    finally:
        layers.uninstall_fast_layers()
    assert (BL.forward, WA.forward, TD.forward) == orig and not layers._ORIGINAL


def _div_floor(a, b):
    """c10::div_floor_floating in fp32 (torch `//`), elementwise on numpy float32"""
    a, b = np.asarray(a, np.float32), np.float32(b)
    mod = np.fmod(a, b)
    div = ((a - mod) / b).astype(np.float32)
    div = np.where((mod != 0) & ((b < 0) != (mod < 0)), (div - np.float32(1)).astype(np.float32), div)
    fl = np.floor(div)
    fl = np.where((div - fl).astype(np.float32) > np.float32(0.5), fl + np.float32(1), fl)
    return np.where(div != 0, fl, np.copysign(np.float32(0), a / b)).astype(np.float32)


def _quantise(xyz, w, quant, shifted):
    """what swin_quant_kernel computes per point and axis, one rounded fp32 operation at a time"""
    w32, q32 = np.float32(w), np.float32(quant)
    v = (xyz - xyz.min(0)).astype(np.float32)
    if shifted:
        v = (v + np.float32(0.5) * w32).astype(np.float32)
    mod = np.fmod(v, w32)
    mod = np.where((mod != 0) & ((w32 < 0) != (mod < 0)), (mod + w32).astype(np.float32), mod)
    return _div_floor(mod, q32).astype(np.int32)


def test_numpy_restatement_of_the_quantisation_agrees_with_the_oracle():
    g = np.load(GOLDEN)
    xyz = g["xyz"]
    w, quant = float(g["window_size"]), float(g["quant_size"])
    qgl = int(w / quant)
    for pat in (0, 1):
        i0, i1 = g[f"p{pat}_index_0"].astype(np.int64), g[f"p{pat}_index_1"].astype(np.int64)
        shift = 0.0 if pat == 0 else 1 / 2 * torch.tensor([w] * 3)
        want = index_ref.swin_rel_pos_index(torch.from_numpy(xyz), torch.from_numpy(i0), torch.from_numpy(i1), w, quant, shift).numpy()
        q = _quantise(xyz, w, quant, bool(pat))
        assert q.min() >= 0 and q.max() <= qgl - 1
        got = q[i0] - q[i1] + qgl - 1
        assert np.array_equal(got, want.astype(np.int64))
