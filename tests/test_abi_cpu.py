"""CPU: the C ABI.  Python hands the library raw addresses through hand-written mirrors of include/pointops2_hip.h - the ctypes table
and the constant tables of _lib.py, index_build.CellPlanStruct, the words optim.py packs - and a wrong entry is no error but a
misplaced pointer.  Here every declaration, struct and constant of the header (read by tests/abi_header.py, the only reader) is
compared with its mirror, and the header with what the built library exports.  The operator tests pin their own launchers' literal
signatures on top of this; none of them reads the header's types again."""
import ctypes
import os
import subprocess

import pytest
import torch

from stratified_transformer_amd import _lib, index_build, optim
from tests import abi_header


def _table():
    return {**{name: (None, argtypes) for name, argtypes in _lib.SIGNATURES.items()},
            **{name: (restype, argtypes) for name, (argtypes, restype) in _lib.RESULTS.items()}}


# ---- every declaration against the table ----
def test_every_declaration_matches_the_ctypes_table():
    declared, table = abi_header.declarations(), _table()
    assert len(declared) >= 114
    assert not set(_lib.SIGNATURES) & set(_lib.RESULTS)
    assert set(declared) == set(table) == set(_lib.exported_symbols()), set(declared) ^ set(table)
    wrong = {name: (declared[name], table[name]) for name in declared if not abi_header.same_signature(declared[name], table[name])}
    assert not wrong, wrong
    # the one parameter bound as a typed pointer, and the rule that admits it
    opts, plan = ctypes.POINTER(_lib.LaunchOpts), ctypes.POINTER(index_build.CellPlanStruct)
    assert _lib.SIGNATURES["pointops2_set_launch_opts"] == declared["pointops2_set_launch_opts"][1] == [opts]
    assert declared["cell_attention_forward_launcher"][1][0] is plan

    def fits(d, b):
        return abi_header.same_signature((None, [d]), (None, [b]))
    assert fits(opts, _lib.P) and not fits(opts, plan) and not fits(_lib.P, opts) and not fits(_lib.I, _lib.U) and not fits(_lib.I, _lib.P)
    assert not abi_header.same_signature((_lib.P, []), (ctypes.c_char_p, [])) and not abi_header.same_signature((None, [_lib.I]), (None, []))
    for decl, result in (("short n", False), ("uint16_t q", False), ("int", False), ("float *", True)):  # unknown types are errors
        with pytest.raises(ValueError, match="some_launcher"):
            abi_header._ctype(decl, "some_launcher", result)


def test_the_loaded_library_carries_the_table():
    l = _lib.lib()
    for name, (restype, argtypes) in _table().items():
        fn = getattr(l, name)
        assert fn.restype is restype and len(fn.argtypes) == len(argtypes) and all(a is b for a, b in zip(fn.argtypes, argtypes)), name


# ---- exports, both ways ----
def test_library_exports_every_symbol_of_the_header():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    names = sorted(abi_header.declarations())
    assert len(names) >= 30
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(l, n), f"{n} declared in include/pointops2_hip.h but not exported"
    assert set(_lib.exported_symbols()) == set(names), set(_lib.exported_symbols()) ^ set(names)
    # and the reverse: every ABI-named symbol the library exports is declared in the header
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    abi = {l.split()[-1] for l in nm.splitlines() if l.strip()}
    abi = {n for n in abi if n.startswith("pointops2_") or n.endswith("_launcher")}
    assert len(abi) >= 30
    assert abi <= set(names), f"exported but not declared in include/pointops2_hip.h: {sorted(abi - set(names))}"


def test_abi_version():
    """bumped when a signature changes; entry points that are only added leave it"""
    assert _lib.lib().pointops2_abi_version() == 5


# ---- struct layouts ----
def _ctypes_layout(struct):
    return {"sizeof": ctypes.sizeof(struct), **{name: getattr(struct, name).offset for name, _ in struct._fields_}}


def test_struct_layouts_match_the_header(tmp_path):
    """The ctypes mirrors and the words optim.py packs against sizeof and every offsetof the host C compiler reports for the
    header's structs: a layout mismatch would hand the library misplaced pointers without any error."""
    names = ["pointops2_launch_opts", "pointops2_cell_plan", "pointops2_optim_tensor", "pointops2_optim_group"]
    got = abi_header.struct_layout(names, tmp_path)
    for name, mirror in (("pointops2_launch_opts", _lib.LaunchOpts), ("pointops2_cell_plan", index_build.CellPlanStruct)):
        assert abi_header.MIRRORS[name] is mirror
        # the header declares the mirror's fields, all of them and in its order
        assert abi_header.struct_fields(name) == [f for f, _ in mirror._fields_], name
        assert got[name] == _ctypes_layout(mirror), name
    assert (got["pointops2_launch_opts"]["sizeof"], got["pointops2_cell_plan"]["sizeof"]) == (96, 144)
    # pointops2_optim_tensor: 7 eight-byte words, param .. step at words 0-4, numel at word 5, group the low and first_chunk the high
    # half of word 6 (optim.py packs group | first_chunk << 32 into one little-endian int64)
    assert abi_header.struct_fields("pointops2_optim_tensor") == ["param", "grad", "exp_avg", "exp_avg_sq", "step", "numel", "group",
                                                                  "first_chunk"]
    assert got["pointops2_optim_tensor"] == {"sizeof": 56, "param": 0, "grad": 8, "exp_avg": 16, "exp_avg_sq": 24, "step": 32,
                                             "numel": 40, "group": 48, "first_chunk": 52}
    # pointops2_optim_group: 5 doubles
    assert abi_header.struct_fields("pointops2_optim_group") == ["lr", "beta1", "beta2", "eps", "weight_decay"]
    assert got["pointops2_optim_group"] == {"sizeof": 40, "lr": 0, "beta1": 8, "beta2": 16, "eps": 24, "weight_decay": 32}
    assert (optim._TENSOR_WORDS, optim._GROUP_WORDS) == (7, 5)
    assert (8 * optim._TENSOR_WORDS, 8 * optim._GROUP_WORDS) == (got["pointops2_optim_tensor"]["sizeof"], got["pointops2_optim_group"]["sizeof"])


# ---- constants ----
def test_constant_tables_match_the_defines():
    defines, codes = abi_header.defines(), abi_header.codes
    assert codes("POINTOPS2_CELL_FWD_") == _lib.CELL_FWD
    rows = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    assert {rows[k]: v for k, v in codes("POINTOPS2_ROWS_").items()} == _lib.ROW_TYPES
    assert codes("POINTOPS2_ACT_") == _lib.ACTIVATIONS
    optim_codes = codes("POINTOPS2_OPTIM_")
    assert optim_codes.pop("chunk") == defines["POINTOPS2_OPTIM_CHUNK"] == 1 << optim._CHUNK_SHIFT == 4096
    assert optim_codes == _lib.OPTIM_KINDS
    assert defines["POINTOPS2_LINEAR_GRADS_ROWS"] == _lib.LINEAR_GRADS_ROWS
