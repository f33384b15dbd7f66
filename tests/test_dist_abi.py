"""Host only: libsta_dist.so exports exactly include/sta_dist.h, the ctypes table mirrors it, no name collides with the other eight
tables, every declaration that takes a stream has a row in tests/dist_stream_cases.py (and the other way round) and none of them may wait,
the header's constants are those of vista_slam_amd/meshdist.py and tests/dist_cases.py.  That no
library is built from another's own files is tests/test_library_table.py's to check."""
import ctypes as C
import inspect
import os
import pathlib
import re

import dist_cases as D
import dist_stream_cases as DS
from test_cabi_symbols import all_exported, declared_symbols, exported_symbols
from test_stream_inventory import stream_entry_points

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "sta_dist.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 4, every
    assert set(every) == set(_lib.DIST_SIGNATURES), set(every) ^ set(_lib.DIST_SIGNATURES)
    assert all_exported(_lib.DIST_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.DIST_LIB_PATH) - LINKER ^ set(every))
    for table in (_lib.SIGNATURES, _lib.TEST_SIGNATURES, _lib.CLOUD_SIGNATURES, _lib.RASTER_SIGNATURES, _lib.TSDF_SIGNATURES, _lib.MESH_SIGNATURES,
                  _lib.SURF_SIGNATURES, _lib.SIMP_SIGNATURES):
        assert not set(every) & set(table), sorted(set(every) & set(table))
    lib = _lib.load_dist()
    for name in every:
        assert hasattr(lib, name), name
    assert not build.is_stale(build.DIST_LIB, build.DIST_HASH_FILE, build.DIST_DEPS)
    assert inspect.signature(build.build_lib).parameters["dist"].default is True
    assert build.DIST_SOURCES == ["sta_dist.hip"] and os.path.basename(build.DIST_LIB) == "libsta_dist.so"


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_dist.h maps to: the host size array is typed, every other pointer (device memory and
    the host struct sta_tri_index) is void*"""
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
    assert len(decls) == 4
    for ret, name, params in decls:
        res, args = _lib.DIST_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            assert a is _ctype_of(p), (name, p, a, _ctype_of(p))
    # the host struct, field by field
    body = re.search(r"typedef struct sta_tri_index \{(.*?)\} sta_tri_index;", text, flags=re.S).group(1)
    fields = re.findall(r"(float\*|int32_t\*|int64_t|int32_t)\s+(\w+)(\[[^\]]+\])?;", body)
    kinds = {"float*": C.c_void_p, "int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [f[1] for f in fields] == [n for n, _t in _lib.StaTriIndex._fields_]
    for (kind, name, arr), (_n, ctype) in zip(fields, _lib.StaTriIndex._fields_):
        if arr:
            assert arr == "[STA_DIST_MAX_LEVELS + 1]" and ctype._length_ == D.MAX_LEVELS + 1 and ctype._type_ is kinds[kind], name
        else:
            assert ctype is kinds[kind], name


def test_the_constants_of_the_header_are_repeated_faithfully():
    from vista_slam_amd import meshdist
    text = HEADER.read_text()
    defs = dict(re.findall(r"#define\s+(STA_DIST_\w+)\s+([^\s/]+)", text))
    assert int(defs["STA_DIST_FANOUT"]) == D.FANOUT == meshdist.FANOUT == 8
    assert int(defs["STA_DIST_MAX_LEVELS"]) == D.MAX_LEVELS == meshdist.MAX_LEVELS == 9 and D.FANOUT ** D.MAX_LEVELS >= 1 << 27
    assert int(defs["STA_DIST_KEY_BITS"]) == D.KEY_BITS == meshdist.KEY_BITS == 21
    assert int(defs["STA_DIST_PLAN_SIZES"]) == D.PLAN_SIZES == meshdist.PLAN_SIZES == len(meshdist.Plan._fields) == 2
    assert int(defs["STA_DIST_COUNTERS"]) == len(D.COUNTERS) == len(meshdist.COUNTERS) == 8
    layout = ("N_VALID", "N_BAD_INDEX", "N_NON_FINITE", "N_NO_AREA", "STATUS")
    assert [int(defs["STA_DIST_" + k]) for k in layout] == list(range(5)) == [D.VALID, D.BAD_INDEX, D.NON_FINITE, D.NO_AREA, 4]
    assert int(defs["STA_DIST_STATUS_BOUND"]) == D.STATUS_BOUND == meshdist.STATUS_BOUND == 1
    assert D.COUNTERS == meshdist.COUNTERS
    for want, field in zip(("valid", "bad_index", "non_finite", "no_area", "status"), D.COUNTERS):
        assert want == field
    fields = re.search(r"typedef struct sta_dist_sizes \{(.*?)\}", text, flags=re.S).group(1)
    assert tuple(re.findall(r"int64_t (\w+);", fields)) == meshdist.Plan._fields
    kernels = (HEADER.parents[1] / "vista_slam_amd" / "csrc" / "dist.h").read_text()
    assert re.search(r"#define DS_F 8\b", kernels) and re.search(r"#define DS_MAX_LEVELS 9\b", kernels) and "#pragma clang fp contract(off)" in kernels
    assert "atomicAdd" not in kernels and "atomicMin" not in kernels and "atomicMax" not in kernels          # the one atomic is the integer status OR
    flat = " ".join(text.replace(" * ", " ").split())
    for sentence in ("No signed distance", "no ray casting", "no point-to-plane ICP against the mesh", "THE CLAMP IS PART OF THE CONTRACT",
                     "with no margin at all", "must still be visited, for the tie rule", "It was not compared with Open3D's RaycastingScene"):
        assert sentence in flat, sentence


def test_every_stream_entry_point_has_a_row_and_none_may_wait():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_tri_build", "sta_tri_query"], taking
    named = DS.named_entries()
    assert not (named & set(DS.EXEMPT))
    assert not set(taking) - named - set(DS.EXEMPT), sorted(set(taking) - named - set(DS.EXEMPT))
    assert not (named | set(DS.EXEMPT)) - set(taking) - DS.OTHER_LIBRARIES, sorted((named | set(DS.EXEMPT)) - set(taking))
    names = [r.name for r in DS.ROWS]
    assert len(names) == len(set(names))
    for r in DS.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run) and callable(r.make_b), r.name
        assert not DS.may_wait(r)
    assert DS.SYNCS == {}, "no call of this library may wait"
    header = " ".join(HEADER.read_text().split())
    assert "NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES" in header.replace(" * ", " ")

