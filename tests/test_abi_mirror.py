"""CPU: the ctypes mirror in e3dge_amd/_lib.py against include/e3dge_hip.h, whole and from _lib's own tables: every argument struct
(size, and offset and size of every field, from one compiled C program), every prototype by parameter kind, every constant the two
share, and the ABI version.  A wrong offset in the mirror is a wild device pointer, so nothing here is a hand-picked sample."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib

HEADER = os.path.join(REPO, "include", "e3dge_hip.h")
UNDECLARED = {"e3dge_debug_stamps", "e3dge_debug_stamps_clear"}      # csrc/stamps.h: outside the header; _lib._stamps_call binds the first on use


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _mirrors():
    return {"E3dge" + c.__name__: c for c in _lib._Args.__subclasses__() if c.__module__ == _lib.__name__}


def _constants(text):
    """Names X of `#define E3DGE_X <value>` that _lib also has."""
    return [x for x in re.findall(r"^#define\s+E3DGE_(\w+)[ \t]+\S", text, flags=re.M) if hasattr(_lib, x)]


@pytest.fixture(scope="module")
def c_facts(tmp_path_factory):
    """What the C compiler says: {"sizeof Struct" | "Struct.field" | "#X": numbers}, from one program."""
    lines = []
    for struct, cls in _mirrors().items():
        lines.append(f'  printf("sizeof {struct}|%zu\\n", sizeof({struct}));')
        for name, *_ in cls._fields_:
            f = name[:-1] if name.endswith("_") else name
            lines.append(f'  printf("{struct}.{name}|%zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));')
    for x in _constants(_header()):
        lines.append(f'  printf("#{x}|%lld\\n", (long long)(E3DGE_{x}));')
    d = tmp_path_factory.mktemp("abi_mirror")
    src, exe = str(d / "mirror.c"), str(d / "mirror")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "e3dge_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0; }\n")
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {key: [int(v) for v in values.split()] for key, values in (ln.split("|") for ln in out.splitlines())}


def test_every_struct_mirror_has_the_c_layout(c_facts):
    mirrors = _mirrors()
    assert len(mirrors) >= 27
    assert set(re.findall(r"typedef\s+struct\s+(E3dge\w+)", _header())) == set(mirrors)
    wrong, n_fields = [], 0
    for struct, cls in mirrors.items():
        if c_facts[f"sizeof {struct}"] != [ctypes.sizeof(cls)]:
            wrong.append((struct, "sizeof", c_facts[f"sizeof {struct}"], ctypes.sizeof(cls)))
        for name, *_ in cls._fields_:
            n_fields += 1
            d = getattr(cls, name)
            if c_facts[f"{struct}.{name}"] != [d.offset, d.size]:
                wrong.append((struct, name, c_facts[f"{struct}.{name}"], [d.offset, d.size]))
    assert not wrong, wrong
    assert n_fields >= 458


def _kind_of_c(decl):
    """'ptr', 'int', 'i64' or 'f32' of a C return type or parameter declaration (the name, if any, is dropped)."""
    decl = decl.strip()
    if "*" in decl or re.match(r"(const\s+)?e3dge_stream_t\b", decl):
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    base = {"int": "int", "int64_t": "i64", "float": "f32"}.get(words[0]) if words else None
    assert base and len(words) <= 2, f"cannot classify {decl!r}"
    return base


def _kind_of_ctypes(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    return {ctypes.c_int: "int", ctypes.c_int64: "i64", ctypes.c_float: "f32"}[t]


def test_every_prototype_matches_its_signature_row(lib):
    text = _header()
    protos = re.findall(r"^[ \t]*((?:const\s+)?\w+[ \t]*\*?)[ \t]*(e3dge_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M)
    declared = {name for _, name, _ in protos}
    assert len(protos) == len(declared) >= 127
    assert declared == set(re.findall(r"\b(e3dge_[a-z0-9_]+)\s*\(", text))          # the strict pattern skipped none
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()[-1].startswith("e3dge_")}
    assert exported - UNDECLARED == declared, (exported - UNDECLARED) ^ declared
    wrong = []
    for ret, name, params in protos:
        params = [] if params.strip() in ("", "void") else params.split(",")
        want = (_kind_of_c(ret), [_kind_of_c(p) for p in params])
        res, args = _lib.SIGNATURES[name]
        got = (_kind_of_ctypes(res), [_kind_of_ctypes(a) for a in args])
        if want != got:
            wrong.append((name, want, got))
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes or []) == list(args), name     # load() bound the row, not something else
    assert not wrong, wrong


def test_shared_constants_are_equal(c_facts):
    names = _constants(_header())
    must = {"AMAX_FLOATS", "DEC2_MAX_UP", "MC_MAX_TRIS", "MESH_MAX_FACES_PER_PIXEL", "NOISE_PROJECT_FACES_PER_PIXEL", "NOISE_PROJECT_MAX_MAPS",
            "IDNET_CONVS", "IDNET_BNS", "IDNET_UNITS", "IDNET_TAPS", "IDNET_PRELUS", "SHAPE_LOSS_SEGMENTS", "SHAPE_SMOOTH_L1", "SHAPE_EIKONAL",
            "DISC_MAX_BLOCKS", "DISC_TAP_STDDEV", "DISC_TAP_FINAL", "DISC_TAP_STEM", "DISC_TAPS", "PREC_F32", "PREC_F16X3", "PREC_F16X3_V1",
            "PREC_F16X3_G2"}
    assert must <= set(names), must - set(names)
    assert {x: c_facts["#" + x][0] for x in names} == {x: getattr(_lib, x) for x in names}


def test_abi_version(lib):
    assert lib.e3dge_abi_version() == _lib.ABI_VERSION == 17
