"""Host only: libsta_mesh.so exports exactly include/sta_mesh.h, the ctypes table mirrors it, no name collides with the other five tables,
every declaration that takes a stream has a row in tests/mesh_stream_cases.py (and the other way round) and none of them may wait, the
header's constants are those of vista_slam_amd/render.py and tests/mesh_cases.py.  That no
library is built from another's own files is tests/test_library_table.py's to check."""
import ctypes as C
import inspect
import os
import pathlib
import re

import mesh_stream_cases as MS
from test_cabi_symbols import all_exported, declared_symbols, exported_symbols
from test_stream_inventory import stream_entry_points

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "sta_mesh.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 4, every
    assert set(every) == set(_lib.MESH_SIGNATURES), set(every) ^ set(_lib.MESH_SIGNATURES)
    assert all_exported(_lib.MESH_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.MESH_LIB_PATH) - LINKER ^ set(every))
    for table in (_lib.SIGNATURES, _lib.TEST_SIGNATURES, _lib.CLOUD_SIGNATURES, _lib.RASTER_SIGNATURES, _lib.TSDF_SIGNATURES):
        assert not set(every) & set(table), sorted(set(every) & set(table))
    lib = _lib.load_mesh()
    for name in every:
        assert hasattr(lib, name), name
    assert not build.is_stale(build.MESH_LIB, build.MESH_HASH_FILE, build.MESH_DEPS)
    assert inspect.signature(build.build_lib).parameters["mesh"].default is True
    assert build.MESH_SOURCES == ["sta_mesh.hip"] and os.path.basename(build.MESH_LIB) == "libsta_mesh.so"


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_mesh.h maps to: host arrays are typed, device pointers are void*"""
    p = re.sub(r"\bconst\b", "", param).strip()
    name = re.search(r"(\w+)$", p).group(1)
    base = p[:-len(name)].replace(" ", "")
    if base.endswith("*"):
        if name.endswith("_host") or name == "sizes_out":
            return {"int64_t*": C.POINTER(C.c_int64), "double*": C.POINTER(C.c_double)}[base]
        return C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}[base]


def test_the_ctypes_table_mirrors_the_header():
    from vista_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bSTA_API\b\s*([^;(]*?)\b(sta_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(decls) == 4
    for ret, name, params in decls:
        res, args = _lib.MESH_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            assert a is _ctype_of(p), (name, p, a, _ctype_of(p))


def test_the_constants_of_the_header_are_repeated_faithfully():
    import mesh_cases as MC
    import render_cases as RC
    from vista_slam_amd import render
    defs = dict(re.findall(r"#define\s+(STA_MESH_\w+)\s+([^\s/]+)", HEADER.read_text()))
    assert int(defs["STA_MESH_SUBPIXEL"]) == MC.SUBPIXEL == 256 and int(defs["STA_MESH_MAX_SNAP"]) == MC.MAX_SNAP == 1 << 28
    assert (int(defs["STA_MESH_PAYLOAD_ID"]), int(defs["STA_MESH_PAYLOAD_COLOR"]), int(defs["STA_MESH_PAYLOAD_NORMAL"])) == (MC.ID, MC.COLOR, MC.NORMAL)
    assert render.MESH_MODES == {"id": MC.ID, "color": MC.COLOR, "shaded": MC.COLOR, "normal": MC.NORMAL}
    assert (int(defs["STA_MESH_CULL_NONE"]), int(defs["STA_MESH_CULL_BACK"]), int(defs["STA_MESH_CULL_FRONT"])) == (MC.CULL_NONE, MC.CULL_BACK, MC.CULL_FRONT)
    assert render.MESH_CULL == {"none": MC.CULL_NONE, "back": MC.CULL_BACK, "front": MC.CULL_FRONT}
    assert int(defs["STA_MESH_COUNTERS"]) == MC.N_COUNTERS == len(render.MESH_COUNTERS) == 8 and int(defs["STA_MESH_PLAN_SIZES"]) == MC.PLAN_SIZES == 2
    fields = re.search(r"typedef struct sta_mesh_counters \{(.*?)\}", HEADER.read_text(), flags=re.S).group(1)
    assert tuple(re.findall(r"uint64_t (\w+);", fields)) == render.MESH_COUNTERS
    assert [getattr(MC, n.upper()) for n in render.MESH_COUNTERS] == list(range(8))
    assert (render.MAX_DIM, render.MIN_NEAR, render.MAX_FAR) == (RC.MAX_DIM, RC.MIN_NEAR, RC.MAX_FAR)


def test_the_plan_is_the_restatements():
    import mesh_cases as MC
    from vista_slam_amd import _lib
    lib = _lib.load_mesh()
    out = (C.c_int64 * 2)()
    for nt, nv in ((0, 0), (1, 3), (2124, 1064), (341, 7), (342, 7), (10 ** 6, 10 ** 6), (2 ** 31 - 1, 2 ** 31 - 1), (715827882, 5), (715827883, 5)):
        assert lib.sta_mesh_plan(nt, nv, out) == 0 and tuple(out) == MC.plan(nt, nv), (nt, nv)
    for nt, nv in ((-1, 3), (2 ** 31, 3), (3, -1), (3, 2 ** 31)):
        assert lib.sta_mesh_plan(nt, nv, out) == -1
        try:
            MC.plan(nt, nv)
            raise AssertionError("the restatement accepts it")
        except ValueError as e:
            assert str(e) == lib.sta_mesh_last_error().decode()


def test_every_stream_entry_point_has_a_row_and_none_may_wait():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_mesh_triangles", "sta_mesh_vertex_normals"], taking
    named = MS.named_entries()
    assert not (named & set(MS.EXEMPT))
    assert not set(taking) - named - set(MS.EXEMPT), sorted(set(taking) - named - set(MS.EXEMPT))
    assert not (named | set(MS.EXEMPT)) - set(taking) - MS.OTHER_LIBRARIES, sorted((named | set(MS.EXEMPT)) - set(taking))
    names = [r.name for r in MS.ROWS]
    assert len(names) == len(set(names))
    for r in MS.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run) and callable(r.make_b), r.name
        assert not MS.may_wait(r)
    assert MS.SYNCS == {}, "no call of this library may wait"
    header = " ".join(HEADER.read_text().split())
    assert "NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES" in header.replace(" * ", " ")

