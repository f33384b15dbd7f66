"""Host only: libsta_raster.so exports exactly include/sta_raster.h, the ctypes table mirrors it, no name collides with the other
tables, every declaration that takes a stream has a row in tests/render_stream_cases.py (and the other way round).  That no
library is built from another's own files is tests/test_library_table.py's to check."""
import ctypes as C
import pathlib
import re

import render_stream_cases as RS
from test_cabi_symbols import all_exported, declared_symbols, exported_symbols
from test_stream_inventory import stream_entry_points

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "sta_raster.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 6, every
    assert set(every) == set(_lib.RASTER_SIGNATURES), set(every) ^ set(_lib.RASTER_SIGNATURES)
    assert all_exported(_lib.RASTER_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.RASTER_LIB_PATH) - LINKER ^ set(every))
    for table in (_lib.SIGNATURES, _lib.TEST_SIGNATURES, _lib.CLOUD_SIGNATURES):
        assert not set(every) & set(table), sorted(set(every) & set(table))
    lib = _lib.load_raster()
    for name in every:
        assert hasattr(lib, name), name
    assert not build.is_stale(build.RASTER_LIB, build.RASTER_HASH_FILE, build.RASTER_DEPS)


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_raster.h maps to"""
    p = re.sub(r"\bconst\b", "", param).strip()
    base = re.sub(r"\s*\w+$", "", p).strip() if not p.endswith("*") else p           # drop the parameter's name
    if "*" in base:
        kind = base.replace(" ", "")
        return {"int64_t*": C.POINTER(C.c_int64), "double*": C.POINTER(C.c_double)}.get(kind, C.c_void_p) if param.strip().endswith("_host") or \
            kind == "int64_t*" else C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}[base]


def test_the_ctypes_table_mirrors_the_header():
    from vista_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bSTA_API\b\s*([^;(]*?)\b(sta_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(decls) == 6
    for ret, name, params in decls:
        res, args = _lib.RASTER_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            want = _ctype_of(p)
            if p.endswith("background_host"):
                want = C.POINTER(C.c_uint8)
            assert a is want or (want is C.c_void_p and a is C.c_void_p), (name, p, a, want)
    # the constants of the header that the Python layer and the restatement repeat
    import render_cases as RC
    from vista_slam_amd import render
    defs = dict(re.findall(r"#define\s+(STA_RASTER_\w+)\s+([^\s/]+)", HEADER.read_text()))
    assert int(defs["STA_RASTER_MAX_DIM"]) == render.MAX_DIM == RC.MAX_DIM and int(defs["STA_RASTER_MAX_SIZE"]) == render.MAX_SIZE == RC.MAX_SIZE
    assert int(defs["STA_RASTER_CLIP_MARGIN"]) == RC.MARGIN and float(defs["STA_RASTER_MAX_COORD"]) == RC.MAX_COORD
    assert (float(defs["STA_RASTER_MIN_NEAR"]), float(defs["STA_RASTER_MAX_FAR"])) == (render.MIN_NEAR, render.MAX_FAR) == (RC.MIN_NEAR, RC.MAX_FAR)


def test_every_stream_entry_point_has_a_row():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_raster_clear", "sta_raster_lines", "sta_raster_points", "sta_raster_resolve"], taking
    named = RS.named_entries()
    assert not (named & set(RS.EXEMPT))
    assert not set(taking) - named - set(RS.EXEMPT), sorted(set(taking) - named - set(RS.EXEMPT))
    assert not (named | set(RS.EXEMPT)) - set(taking), sorted((named | set(RS.EXEMPT)) - set(taking))
    names = [r.name for r in RS.ROWS]
    assert len(names) == len(set(names))
    for r in RS.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run) and callable(r.make_b), r.name
    assert not RS.SYNCS, "no entry point of include/sta_raster.h may wait for its stream"
    header = HEADER.read_text()
    assert "no call allocates, copies to the host or synchronises" in header

