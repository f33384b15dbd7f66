"""Host only: libsta_surf.so exports exactly include/sta_surf.h, the ctypes table mirrors it, no name collides with the other six tables,
every declaration that takes a stream has a row in tests/surf_stream_cases.py (and the other way round) and none of them may wait, the
header's constants are those of vista_slam_amd/surface.py and tests/surf_cases.py, the plan is the restatement's.  That no
library is built from another's own files is tests/test_library_table.py's to check."""
import ctypes as C
import inspect
import os
import pathlib
import re

import pytest

import surf_cases as SF
import surf_stream_cases as SS
from test_cabi_symbols import all_exported, declared_symbols, exported_symbols
from test_stream_inventory import stream_entry_points

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "sta_surf.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 5, every
    assert set(every) == set(_lib.SURF_SIGNATURES), set(every) ^ set(_lib.SURF_SIGNATURES)
    assert all_exported(_lib.SURF_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.SURF_LIB_PATH) - LINKER ^ set(every))
    for table in (_lib.SIGNATURES, _lib.TEST_SIGNATURES, _lib.CLOUD_SIGNATURES, _lib.RASTER_SIGNATURES, _lib.TSDF_SIGNATURES, _lib.MESH_SIGNATURES):
        assert not set(every) & set(table), sorted(set(every) & set(table))
    lib = _lib.load_surf()
    for name in every:
        assert hasattr(lib, name), name
    assert not build.is_stale(build.SURF_LIB, build.SURF_HASH_FILE, build.SURF_DEPS)
    assert inspect.signature(build.build_lib).parameters["surf"].default is True
    assert build.SURF_SOURCES == ["sta_surf.hip"] and os.path.basename(build.SURF_LIB) == "libsta_surf.so"


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_surf.h maps to: the host array is typed, device pointers are void*"""
    p = re.sub(r"\bconst\b", "", param).strip()
    name = re.search(r"(\w+)$", p).group(1)
    base = p[:-len(name)].replace(" ", "")
    if base.endswith("*"):
        return C.POINTER(C.c_int64) if name == "sizes_out" else C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64}[base]


def test_the_ctypes_table_mirrors_the_header():
    from vista_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bSTA_API\b\s*([^;(]*?)\b(sta_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(decls) == 5
    for ret, name, params in decls:
        res, args = _lib.SURF_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            assert a is _ctype_of(p), (name, p, a, _ctype_of(p))


def test_the_constants_of_the_header_are_repeated_faithfully():
    from vista_slam_amd import surface
    text = HEADER.read_text()
    defs = dict(re.findall(r"#define\s+(STA_SURF_\w+)\s+([^\s/]+)", text))
    assert int(defs["STA_SURF_CHUNK"]) == SF.CHUNK == surface.CHUNK == 1024
    assert int(defs["STA_SURF_STATUS_BOUND"]) == SF.STATUS_BOUND == surface.STATUS_BOUND == 1
    assert int(defs["STA_SURF_PLAN_SIZES"]) == SF.PLAN_SIZES == surface.PLAN_SIZES == len(surface.Plan._fields) == 3
    for k in (SF.GOLDEN, SF.MIX_1, SF.MIX_2):
        assert f"0x{k:016X}" in text, hex(k)
    for z in SF.KNOWN_ANSWERS.values():
        assert f"{z:016x}" in text, hex(z)
    kernels = (HEADER.parents[1] / "vista_slam_amd" / "csrc" / "surf.h").read_text()
    for k in (SF.GOLDEN, SF.MIX_1, SF.MIX_2):
        assert f"0x{k:016X}ull" in kernels, hex(k)
    fields = re.search(r"typedef struct sta_surf_sizes \{(.*?)\}", text, flags=re.S).group(1)
    assert tuple(re.findall(r"int64_t (\w+);", fields)) == surface.Plan._fields
    assert "share a VERTEX, not only when" in " ".join(text.replace(" * ", " ").split())        # the stated difference from Open3D


PLANS = ((0, 0, 0), (1, 3, 1), (2124, 1064, 100001), (1023, 7, 0), (1024, 64, 5), (1025, 65, 5), (10 ** 6, 2 * 10 ** 6, 2 * 10 ** 6),
         (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))
BAD_PLANS = ((-1, 3, 0), (2 ** 31, 3, 0), (3, -1, 0), (3, 2 ** 31, 0), (3, 3, -1), (3, 3, 2 ** 31))


def test_the_plan_is_the_restatements():
    from vista_slam_amd import _lib, surface
    lib = _lib.load_surf()
    out = (C.c_int64 * 3)()
    for nt, nv, ns in PLANS:
        assert lib.sta_surf_plan(nt, nv, ns, out) == 0 and tuple(out) == SF.plan(nt, nv, ns) == tuple(surface.plan(nt, nv, ns)), (nt, nv, ns)
    for nt, nv, ns in BAD_PLANS:
        assert lib.sta_surf_plan(nt, nv, ns, out) == -1
        with pytest.raises(ValueError) as e:
            SF.plan(nt, nv, ns)
        assert str(e.value) == lib.sta_surf_last_error().decode()
        with pytest.raises(ValueError) as e2:
            surface.plan(nt, nv, ns)
        assert str(e2.value) == str(e.value)


def test_every_stream_entry_point_has_a_row_and_none_may_wait():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_surf_components", "sta_surf_sample", "sta_surf_weights"], taking
    named = SS.named_entries()
    assert not (named & set(SS.EXEMPT))
    assert not set(taking) - named - set(SS.EXEMPT), sorted(set(taking) - named - set(SS.EXEMPT))
    assert not (named | set(SS.EXEMPT)) - set(taking) - SS.OTHER_LIBRARIES, sorted((named | set(SS.EXEMPT)) - set(taking))
    names = [r.name for r in SS.ROWS]
    assert len(names) == len(set(names))
    for r in SS.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run) and callable(r.make_b), r.name
        assert not SS.may_wait(r)
    assert SS.SYNCS == {}, "no call of this library may wait"
    header = " ".join(HEADER.read_text().split())
    assert "NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES" in header.replace(" * ", " ")

