"""The one reader of include/pointops2_hip.h for the tests: its function declarations as ctypes types, its integer #defines, the
field names of its structs and their layout as the host C compiler sees it.  tests/test_abi_cpu.py compares them with the hand-written
mirrors (the tables of _lib.py, index_build.CellPlanStruct, the words optim.py packs); operator tests take their constants from here."""
import ctypes
import functools
import os
import re
import subprocess

from stratified_transformer_amd import _lib, index_build

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int": ctypes.c_int, "unsigned int": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}
RESULTS = {"void": None, "void *": ctypes.c_void_p, "char *": ctypes.c_char_p}
# structs of the header with a ctypes mirror: a parameter `const <struct> *` may be bound as POINTER(mirror)
MIRRORS = {"pointops2_launch_opts": _lib.LaunchOpts, "pointops2_cell_plan": index_build.CellPlanStruct}
_STRUCT = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;"


@functools.lru_cache(maxsize=None)
def _text(code=False):
    """the header; with `code`, without its comments and preprocessor lines"""
    with open(os.path.join(INCLUDE, "pointops2_hip.h")) as f:
        text = f.read()
    if code:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    return text


@functools.lru_cache(maxsize=None)
def _prototypes():
    """{name: (result, [parameters])} as the header spells them (`const void *x`), in its order; whatever stands outside the structs
    and is no function declaration is an error"""
    code = re.sub(_STRUCT, " ", _text(code=True), flags=re.S).replace('extern "C" {', " ", 1)
    code = re.sub(r"\}\s*$", " ", code, count=1)  # the closing brace of extern "C", the last token of the header
    out = {}
    for statement in code.split(";"):
        statement = re.sub(r"\s*\*\s*", " *", " ".join(statement.split()))
        m = re.fullmatch(r"([\w \*]+?)\b(\w+) ?\(([^()]*)\)", statement)
        if statement and (m is None or m.group(2) in out):
            raise ValueError(f"include/pointops2_hip.h: not a function declaration, or a second one of its name: {statement!r}")
        if statement:
            out[m.group(2)] = (m.group(1).strip(), [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")])
    return out


def _ctype(decl, where, result=False):
    """ctypes type of a parameter (`const float *xyz`: its type, then its name) or of a result type"""
    words = [w for w in decl.split() if w != "const"]
    kind = " ".join(words if result else words[:-1])
    if result and kind in RESULTS:
        return RESULTS[kind]
    if not result and words[-1].startswith("*"):
        return ctypes.POINTER(MIRRORS[kind]) if kind in MIRRORS else ctypes.c_void_p
    if kind not in SCALARS:
        raise ValueError(f"{where}: the type of {decl!r} is not known to tests/abi_header.py")
    return SCALARS[kind]


def declarations():
    """{name: (restype, [argtypes])} of every function the header declares, in its order and in the ctypes objects _lib uses: the
    scalars of SCALARS, c_void_p for a pointer parameter (POINTER(mirror) for a pointer to a struct of MIRRORS - see same_signature),
    and as a result None for void, c_void_p for `void *`, c_char_p for `const char *`.  Any other type is an error, never skipped."""
    return {name: (_ctype(result, name, True), [_ctype(p, name) for p in params]) for name, (result, params) in _prototypes().items()}


def parameters(name):
    """the parameters of a declared function as the header spells them: ["int n", "const void *x", ...]"""
    return list(_prototypes()[name][1])


def same_signature(declared, bound):
    """whether (restype, argtypes) of the binding fits the declared pair: the same ctypes objects in the same order; where the header
    has a pointer to a mirrored struct, POINTER(mirror) or c_void_p and nothing else"""
    typed = [ctypes.POINTER(m) for m in MIRRORS.values()]
    return bound[0] is declared[0] and len(bound[1]) == len(declared[1]) and all(
        b is d or (d in typed and b is ctypes.c_void_p) for d, b in zip(declared[1], bound[1]))


def codes(prefix="POINTOPS2_"):
    """{rest of the name, in lower case: value} of every `#define <prefix>* <integer>`; a negative value stands in parentheses"""
    found = re.finditer(r"^[ \t]*#[ \t]*define[ \t]+" + prefix + r"(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*(?:/\*|//|$)", _text(), flags=re.M)
    return {m.group(1).lower(): int(m.group(2)) for m in found}


def defines():
    """{NAME: value} of every `#define POINTOPS2_* <integer>`"""
    return {"POINTOPS2_" + name.upper(): value for name, value in codes().items()}


def struct_fields(name):
    """field names of `typedef struct name {...} name;` in declaration order (`double lr, beta1, ...;` declares several)"""
    body = dict(re.findall(_STRUCT, _text(code=True), flags=re.S))[name]
    return [re.search(r"(\w+)\s*$", field).group(1) for decl in body.split(";") if decl.strip() for field in decl.split(",")]


def compile_c(body, tmp_path, stem, link=True):
    """Builds the C99 translation unit `#include "pointops2_hip.h"` + body with the host C compiler ($CC, or cc) under -Wall -Werror
    and returns the path of the program, or with link=False of the object file."""
    src, out = tmp_path / (stem + ".c"), tmp_path / (stem if link else stem + ".o")
    src.write_text('#include "pointops2_hip.h"\n' + body)
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE] + ([] if link else ["-c"]) + [str(src), "-o", str(out)],
                   check=True)
    return out


def struct_layout(names, tmp_path):
    """{struct: {"sizeof": n, field: offset, ...}} as the host C compiler lays the named structs out: one C99 program that prints
    sizeof and every offsetof"""
    prints = "".join(f'printf("{name} sizeof %zu\\n", sizeof({name}));\n'
                     + "".join(f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));\n' for field in struct_fields(name))
                     for name in names)
    exe = compile_c("#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n" + prints + "return 0;\n}\n", tmp_path, "layout")
    out = {name: {} for name in names}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        name, field, value = line.split()
        out[name][field] = int(value)
    return out
