"""Host only: libsta_tsdf.so exports exactly include/sta_tsdf.h, the ctypes table mirrors it, no name collides with the other tables,
every declaration that takes a stream has a row in tests/tsdf_stream_cases.py (and the other way round), the header's constants are those
of vista_slam_amd/tsdf.py and tests/tsdf_cases.py.  That no
library is built from another's own files is tests/test_library_table.py's to check."""
import ctypes as C
import pathlib
import re

import tsdf_stream_cases as TS
from test_cabi_symbols import all_exported, declared_symbols, exported_symbols
from test_stream_inventory import stream_entry_points

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "sta_tsdf.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 7, every
    assert set(every) == set(_lib.TSDF_SIGNATURES), set(every) ^ set(_lib.TSDF_SIGNATURES)
    assert all_exported(_lib.TSDF_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.TSDF_LIB_PATH) - LINKER ^ set(every))
    for table in (_lib.SIGNATURES, _lib.TEST_SIGNATURES, _lib.CLOUD_SIGNATURES, _lib.RASTER_SIGNATURES):
        assert not set(every) & set(table), sorted(set(every) & set(table))
    lib = _lib.load_tsdf()
    for name in every:
        assert hasattr(lib, name), name
    assert not build.is_stale(build.TSDF_LIB, build.TSDF_HASH_FILE, build.TSDF_DEPS)
    assert "tsdf" in __import__("inspect").signature(build.build_lib).parameters


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_tsdf.h maps to: host arrays are typed, device pointers are void*"""
    p = re.sub(r"\bconst\b", "", param).strip()
    name = re.search(r"(\w+)$", p).group(1)
    base = p[:-len(name)].replace(" ", "")
    if base.endswith("*"):
        if name.endswith("_host") or name == "sizes_out":
            return {"int64_t*": C.POINTER(C.c_int64), "double*": C.POINTER(C.c_double), "int8_t*": C.POINTER(C.c_int8)}[base]
        return C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}[base]


def test_the_ctypes_table_mirrors_the_header():
    from vista_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bSTA_API\b\s*([^;(]*?)\b(sta_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(decls) == 7
    for ret, name, params in decls:
        res, args = _lib.TSDF_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            assert a is _ctype_of(p), (name, p, a, _ctype_of(p))


def test_the_constants_of_the_header_are_repeated_faithfully():
    import tsdf_cases as TC
    from vista_slam_amd import tsdf
    defs = dict(re.findall(r"#define\s+(STA_TSDF_\w+)\s+([^\s/]+)", HEADER.read_text()))
    assert int(defs["STA_TSDF_BLOCK"]) == tsdf.BLOCK == TC.BLOCK == 8 and int(defs["STA_TSDF_BLOCK_POINTS"]) == tsdf.BLOCK_POINTS == TC.BLOCK_POINTS == 8 ** 3
    assert int(defs["STA_TSDF_MAX_TRUNC_VOXELS"]) == tsdf.MAX_TRUNC_VOXELS == TC.MAX_TRUNC_VOXELS
    assert int(defs["STA_TSDF_MAX_BLOCKS"]) == tsdf.MAX_BLOCKS == TC.MAX_BLOCKS == 1 << 24
    assert int(defs["STA_TSDF_MAX_PIXELS"]) == tsdf.MAX_PIXELS == TC.MAX_PIXELS == 1 << 28
    assert int(defs["STA_TSDF_BLOCK_BIAS"]) == TC.BIAS == 1 << 20 and int(defs["STA_TSDF_KEY_SENTINEL"].rstrip("ul"), 16) == TC.SENTINEL
    assert int(defs["STA_TSDF_PLAN_SIZES"]) == tsdf.PLAN_SIZES == TC.PLAN_SIZES == len(tsdf.Plan._fields)
    assert int(defs["STA_TSDF_TABLE_ROW"]) == TC.TABLE_ROW == TC.make_table().shape[2]


def test_every_stream_entry_point_has_a_row():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_tsdf_blocks", "sta_tsdf_clear", "sta_tsdf_integrate", "sta_tsdf_mesh"], taking
    named = TS.named_entries()
    assert not (named & set(TS.EXEMPT))
    assert not set(taking) - named - set(TS.EXEMPT), sorted(set(taking) - named - set(TS.EXEMPT))
    assert not (named | set(TS.EXEMPT)) - set(taking), sorted((named | set(TS.EXEMPT)) - set(taking))
    names = [r.name for r in TS.ROWS]
    assert len(names) == len(set(names))
    for r in TS.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run) and callable(r.make_b), r.name
    assert {k for k in TS.SYNCS if k.startswith("sta_")} == {"sta_tsdf_blocks", "sta_tsdf_mesh"}, "the two entry points that return counts wait; no other may"
    assert not TS.may_wait(TS.by_name("tsdf_integrate"))
    header = " ".join(HEADER.read_text().split())
    assert "sta_tsdf_blocks and sta_tsdf_mesh synchronise their stream once, to return their counts" in header.replace(" * ", " ")
    from vista_slam_amd import tsdf
    assert "allocate and mesh wait for the stream once each (their counts come back); integrate does not" in " ".join(tsdf.TSDFVolume.__doc__.split())

