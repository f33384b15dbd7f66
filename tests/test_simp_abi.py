"""Host only: libsta_simp.so exports exactly include/sta_simp.h, the ctypes table mirrors it, no name collides with the other seven
tables, every declaration that takes a stream has a row in tests/simp_stream_cases.py (and the other way round) and none of them may wait,
the header's constants are those of vista_slam_amd/simplify.py and tests/simp_cases.py.  That no
library is built from another's own files is tests/test_library_table.py's to check."""
import ctypes as C
import inspect
import os
import pathlib
import re

import simp_cases as SP
import simp_stream_cases as SS
from test_cabi_symbols import all_exported, declared_symbols, exported_symbols
from test_stream_inventory import stream_entry_points

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "sta_simp.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 5, every
    assert set(every) == set(_lib.SIMP_SIGNATURES), set(every) ^ set(_lib.SIMP_SIGNATURES)
    assert all_exported(_lib.SIMP_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.SIMP_LIB_PATH) - LINKER ^ set(every))
    for table in (_lib.SIGNATURES, _lib.TEST_SIGNATURES, _lib.CLOUD_SIGNATURES, _lib.RASTER_SIGNATURES, _lib.TSDF_SIGNATURES, _lib.MESH_SIGNATURES,
                  _lib.SURF_SIGNATURES):
        assert not set(every) & set(table), sorted(set(every) & set(table))
    lib = _lib.load_simp()
    for name in every:
        assert hasattr(lib, name), name
    assert not build.is_stale(build.SIMP_LIB, build.SIMP_HASH_FILE, build.SIMP_DEPS)
    assert inspect.signature(build.build_lib).parameters["simp"].default is True
    assert build.SIMP_SOURCES == ["sta_simp.hip"] and os.path.basename(build.SIMP_LIB) == "libsta_simp.so"


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_simp.h maps to: the host array is typed, device pointers are void*"""
    p = re.sub(r"\bconst\b", "", param).strip()
    name = re.search(r"(\w+)$", p).group(1)
    base = p[:-len(name)].replace(" ", "")
    if base.endswith("*"):
        return C.POINTER(C.c_int64) if name == "sizes_out" else C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}[base]


def test_the_ctypes_table_mirrors_the_header():
    from vista_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bSTA_API\b\s*([^;(]*?)\b(sta_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(decls) == 5
    for ret, name, params in decls:
        res, args = _lib.SIMP_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            assert a is _ctype_of(p), (name, p, a, _ctype_of(p))


def test_the_constants_of_the_header_are_repeated_faithfully():
    from vista_slam_amd import simplify
    text = HEADER.read_text()
    defs = dict(re.findall(r"#define\s+(STA_SIMP_\w+)\s+([^\s/]+)", text))
    assert int(defs["STA_SIMP_SWEEPS"]) == SP.SWEEPS == simplify.SWEEPS == 8
    assert int(defs["STA_SIMP_INDEX_BITS"]) == SP.INDEX_BITS == simplify.INDEX_BITS == 21 and SP.BIAS == 1 << (SP.INDEX_BITS - 1)
    assert int(defs["STA_SIMP_PLACE_MEAN"]) == SP.PLACE_MEAN == simplify.PLACEMENTS["mean"] == 0
    assert int(defs["STA_SIMP_PLACE_QUADRIC"]) == SP.PLACE_QUADRIC == simplify.PLACEMENTS["quadric"] == 1
    assert int(defs["STA_SIMP_PLAN_SIZES"]) == SP.PLAN_SIZES == simplify.PLAN_SIZES == len(simplify.Plan._fields) == 3
    assert int(defs["STA_SIMP_COUNTERS"]) == len(SP.COUNTERS) == len(simplify.COUNTERS) == len(simplify.Counters._fields) == 8
    layout = ("N_CELLS", "N_VERTS", "N_TRIS", "N_DROPPED", "N_INVALID", "N_COLLAPSED", "N_DUPLICATE", "N_FALLBACK")
    assert [int(defs["STA_SIMP_" + k]) for k in layout] == list(range(8))
    assert SP.COUNTERS == simplify.COUNTERS == simplify.Counters._fields
    for want, field in zip(("cell", "vert", "tri", "dropped", "invalid", "collapsed", "duplicate", "fallback"), SP.COUNTERS):
        assert want in field, (want, field)
    fields = re.search(r"typedef struct sta_simp_sizes \{(.*?)\}", text, flags=re.S).group(1)
    assert tuple(re.findall(r"int64_t (\w+);", fields)) == simplify.Plan._fields
    kernels = (HEADER.parents[1] / "vista_slam_amd" / "csrc" / "simp.h").read_text()
    assert re.search(r"#define SP_SWEEPS 8\b", kernels) and "#pragma clang fp contract(off)" in kernels
    flat = " ".join(text.replace(" * ", " ").split())
    for sentence in ("It is not iterative edge collapse", "there is no target triangle count", "no guarantee of manifoldness",
                     "no boundary or colour quadrics", "Normals are not preserved", "not compared with Open3D's simplify_vertex_clustering or MeshLab"):
        assert sentence in flat, sentence


def test_every_stream_entry_point_has_a_row_and_none_may_wait():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_simp_cells", "sta_simp_place", "sta_simp_triangles"], taking
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

