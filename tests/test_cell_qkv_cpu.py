"""CPU: the C-ABI surface of the cell attention on the packed qkv projection (ABI version 5).  No HIP compute runs here."""
import ctypes

import torch

from stratified_transformer_amd import _lib, index_build
from tests import abi_header

NEW = ("cell_attention_qkv_forward_launcher", "cell_attention_qkv_backward_launcher")


def test_header_compiles_as_c_with_the_packed_prototypes(tmp_path):
    """The header is C: a C99 translation unit that takes the address of both launchers with their full prototypes and uses the
    row-type constants compiles without warnings."""
    abi_header.compile_c(
        "typedef void (*fwd_t)(const pointops2_cell_plan *, int, int, int, const void *, int, float, const float *, const float *,\n"
        "                      const float *, float *, float *, float *);\n"
        "typedef void (*bwd_t)(const pointops2_cell_plan *, int, int, int, const float *, const void *, int, float, const float *,\n"
        "                      const float *, const float *, const float *, const float *, float *, float *, float *, float *, float *);\n"
        "fwd_t f = cell_attention_qkv_forward_launcher;\nbwd_t b = cell_attention_qkv_backward_launcher;\n"
        "int row_types[3] = {POINTOPS2_ROWS_F32, POINTOPS2_ROWS_F16, POINTOPS2_ROWS_BF16};\n", tmp_path, "abi", link=False)
    rows = abi_header.codes("POINTOPS2_ROWS_")
    assert rows == {"f32": 0, "f16": 1, "bf16": 2}
    assert _lib.ROW_TYPES == {torch.float32: rows["f32"], torch.float16: rows["f16"], torch.bfloat16: rows["bf16"]}


def test_library_exports_the_packed_launchers_at_abi_version_5():
    # plan, h, hdim, L, qkv, row_type, scale, three tables, out, ml, pbuf
    I, P, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    assert _lib.SIGNATURES[NEW[0]] == [P, I, I, I, P, I, F, P, P, P, P, P, P]
    # plan, h, hdim, L, grad_out, qkv, row_type, scale, out, three tables, pbuf, gsbuf, grad_qkv, three table gradients
    assert _lib.SIGNATURES[NEW[1]] == [P, I, I, I, P, P, I, F, P, P, P, P, P, P, P, P, P, P]
    assert _lib.lib().cell_attention_qkv_forward_launcher.argtypes == _lib.SIGNATURES[NEW[0]]


def _cell_plan_struct(n_points, n_pairs, n_keyslots, table_rows):
    """a pointops2_cell_plan with the host fields the forward dispatch reads and no device arrays"""
    return index_build.CellPlanStruct(n_points=n_points, n_cells=1, n_parents=1, n_pairs=n_pairs, n_keyslots=n_keyslots, table_rows=table_rows)


def test_cell_forward_dispatch_table_is_unchanged():
    """pointops2_cell_forward_variant keeps its results (the table of test_host_cpu.py::test_cell_forward_dispatch_table): the packed
    launchers run what it names for bf16 = 0, since their tables are fp32."""
    v = _lib.cell_forward_variant
    small, big = 15 * 10, 149  # n_pairs over 10 key slots: an average of 15.0 / 14.9 queries per cell
    for L, mfma in ((1, "mfma64"), (64, "mfma64"), (65, "mfma80"), (80, "mfma80")):
        for n, h in ((95999, 1), (96000, 1), (31999, 3), (32000, 3), (7999, 12), (8000, 12)):
            wide = n * h >= 96000
            assert v(_cell_plan_struct(n, small, 10, L), h, L) == mfma, (L, n, h)
            assert v(_cell_plan_struct(n, big, 10, L), h, L) == ("valu80" if wide else mfma), (L, n, h)
            for pairs in (small, big):
                assert v(_cell_plan_struct(n, pairs, 10, L), h, L, bf16=True) == "valu80", (L, n, h, pairs)
        assert v(_cell_plan_struct(96000, 14, 0, L), 1, L) == "valu80"
        assert v(_cell_plan_struct(96000, 15, 0, L), 1, L) == mfma
    for L in (81, 96, 160):
        for n, pairs, bf16 in ((100, 10, False), (96000, big, False), (96000, small, True), (100, 10, True)):
            assert v(_cell_plan_struct(n, pairs, 10, L), 1, L, bf16=bf16) == "valu160", (L, n, bf16)
    for bf16 in (False, True):
        assert v(_cell_plan_struct(100, 10, 10, 161), 1, 161, bf16=bf16) == "error"
        assert v(_cell_plan_struct(100, 10, 10, 0), 1, 0, bf16=bf16) == "error"
        for hdim in (8, 15, 17, 32):
            assert v(_cell_plan_struct(100, 10, 10, 64), 1, 64, bf16=bf16, hdim=hdim) == "error", hdim
        for L in (63, 65, 96):
            assert v(_cell_plan_struct(100, 10, 10, 64), 1, L, bf16=bf16) == "error", L
        assert v(None, 1, 64, bf16=bf16) == "none"
        assert v(_cell_plan_struct(0, 0, 0, 64), 1, 64, bf16=bf16) == "none"
