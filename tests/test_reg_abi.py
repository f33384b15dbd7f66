"""Host only: libsta_reg.so exports exactly include/sta_reg.h, the ctypes table mirrors it, no name collides with the ten other tables,
the library is a library of its own (for the tenth what tests/test_library_table.py checks for eight and tests/test_ray_abi.py for the
ninth: own files, hash, staleness), the constants it restates are those of include/sta_dist.h, the plan refuses what the header says,
and every declaration that takes a stream has a row in tests/reg_stream_cases.py (and the other way round) and none of them may wait."""
import ctypes as C
import inspect
import os
import pathlib
import re

import pytest

import reg_cases as RG
import reg_stream_cases as RS
from test_cabi_symbols import all_exported
from test_library_table import MARKS
from test_stream_inventory import stream_entry_points

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "sta_reg.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}
OTHERS = ("SIGNATURES", "TEST_SIGNATURES", "SKEW_SIGNATURES", "CLOUD_SIGNATURES", "RASTER_SIGNATURES", "TSDF_SIGNATURES", "MESH_SIGNATURES", "SURF_SIGNATURES",
          "SIMP_SIGNATURES", "DIST_SIGNATURES", "RAY_SIGNATURES")
INCLUDE = r'#include\s+[<"]([^>"]+)[>"]'


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 3, every
    assert set(every) == set(_lib.REG_SIGNATURES) == {"sta_reg_plan", "sta_reg_pass", "sta_reg_last_error"}
    assert all_exported(_lib.REG_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.REG_LIB_PATH) - LINKER ^ set(every))
    for table in OTHERS:
        assert not set(every) & set(getattr(_lib, table)), (table, sorted(set(every) & set(getattr(_lib, table))))
    # the marks of tests/test_library_table.py: none of its names carries another library's, nobody else's carries its prefix
    for name in every:
        assert not [k for k, mark in MARKS.items() if mark(name)] and not name.startswith("sta_ray_"), name
    lib = _lib.load_reg()
    for name in every:
        assert hasattr(lib, name), name
    for name in list(build.SATELLITES) + list(build.ADDONS):
        assert not {s for s in all_exported(getattr(build, name.upper() + "_LIB")) if s.startswith("sta_reg_")}, name
    assert not {s for table in OTHERS for s in getattr(_lib, table) if s.startswith("sta_reg_")}


def test_it_is_a_library_of_its_own():
    from vista_slam_amd import _lib, build
    build.build_lib()
    assert list(build.EXTENSIONS) == ["reg"] and list(build.ADDONS) == ["ray"] and len(build.SATELLITES) == 7
    assert not set(build.EXTENSIONS) & (set(build.ADDONS) | set(build.SATELLITES))
    inc = os.path.join("..", "..", "include")
    own = set(build.EXTENSIONS["reg"][1])
    assert own == {"sta_reg.hip", "reg.h", os.path.join(inc, "sta_reg.h")}
    assert sorted(build.REG_DEPS) == sorted(own | {"sta_exports.map", "sta_common.h", "sta_hostkit.h"}) and len(build.REG_DEPS) == len(set(build.REG_DEPS))
    for d in build.REG_DEPS:
        assert os.path.exists(os.path.join(build.CSRC, d)), d
    assert build.REG_SOURCES == ["sta_reg.hip"] and os.path.basename(build.REG_LIB) == "libsta_reg.so" and build.REG_HASH_FILE == build.REG_LIB + ".srchash"
    assert _lib.REG_LIB_PATH == build.REG_LIB
    assert inspect.signature(build.build_lib).parameters["reg"].default is True
    others = {"mi355": (build.DEPS, {"sta_api.hip", "sta_launch.inc", "sta_forward.inc", "sta_debug.inc", "sta_rows.inc", "sta_bench.inc",
                                     os.path.join(inc, "sta_mi355.h"), os.path.join(inc, "sta_mi355_debug.h")})}
    for name, (_what, mine, _shared) in list(build.SATELLITES.items()) + list(build.ADDONS.items()):
        others[name] = (getattr(build, name.upper() + "_DEPS"), set(mine))
    assert len(others) == 9
    for name, (deps, mine) in others.items():
        assert not own & set(deps), (name, own & set(deps))            # none of its own files is in another library's list
        assert not mine & set(build.REG_DEPS), (name, mine & set(build.REG_DEPS))          # ... and none of theirs in its list
    # ten other hashes: the nine libraries and the skew build of the product's translation unit
    hashes = {build.source_hash(deps) for deps, _mine in others.values()} | {build.source_hash(None, build.SKEW_FLAGS)}
    assert len(hashes) == 10 and build.source_hash(build.REG_DEPS) not in hashes
    assert not build.is_stale(build.REG_LIB, build.REG_HASH_FILE, build.REG_DEPS)
    # the translation unit and the kernels include nothing of libsta_dist.so or libsta_ray.so, and the kernels sta_common.h alone
    for f in ("sta_reg.hip", "reg.h"):
        includes = re.findall(INCLUDE, (pathlib.Path(build.CSRC) / f).read_text())
        assert not [i for i in includes if "dist" in i or "ray" in i or i in ("voxel.h", "select.h", "elementwise.h")], (f, includes)
    assert re.findall(INCLUDE, (pathlib.Path(build.CSRC) / "reg.h").read_text()) == ["sta_common.h"]
    assert re.findall(INCLUDE, (pathlib.Path(build.CSRC) / "sta_reg.hip").read_text()) == ["../../include/sta_reg.h", "sta_common.h", "sta_hostkit.h", "reg.h"]
    assert re.findall(INCLUDE, HEADER.read_text()) == ["stdint.h"]


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_reg.h maps to: the host arrays are typed, every other pointer is void*"""
    p = re.sub(r"\bconst\b", "", param).strip()
    name = re.search(r"(\w+)$", p).group(1)
    base = p[:-len(name)].replace(" ", "")
    if base.endswith("*"):
        return C.POINTER(C.c_int64) if name == "sizes_out" else C.POINTER(C.c_double) if name.endswith("_host") else C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}[base]


def test_the_ctypes_table_mirrors_the_header():
    from vista_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bSTA_API\b\s*([^;(]*?)\b(sta_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(decls) == 3
    for ret, name, params in decls:
        res, args = _lib.REG_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            assert a is _ctype_of(p), (name, p, a, _ctype_of(p))
    # the index goes in as the four pointers and nt of sta_tri_index, in the order of its fields
    dist = (ROOT / "include" / "sta_dist.h").read_text()
    body = re.search(r"typedef struct sta_tri_index \{(.*?)\} sta_tri_index;", dist, flags=re.S).group(1)
    fields = [n for _k, n in re.findall(r"(float\*|int32_t\*|int64_t|int32_t)\s+(\w+)(?:\[[^\]]+\])?;", body)][:5]
    params = next(p for _r, n, p in decls if n == "sta_reg_pass")
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in params.split(",")]
    assert names[:5] == fields == ["tri", "src", "boxes", "counters", "nt"]
    assert names[5:] == ["qry", "qnrm", "Q", "T_host", "pivot_host", "radius", "min_cos", "d2_out", "tri_out", "point_out", "resid_out", "record_out", "work",
                         "work_bytes", "status", "stream"]


def test_the_constants_are_those_of_the_index():
    from vista_slam_amd import meshdist
    text = HEADER.read_text()
    defs = dict(re.findall(r"#define\s+(STA_REG_\w+)\s+([^\s/]+)", text))
    dist = dict(re.findall(r"#define\s+(STA_DIST_\w+)\s+([^\s/]+)", (ROOT / "include" / "sta_dist.h").read_text()))
    assert int(defs["STA_REG_FANOUT"]) == int(dist["STA_DIST_FANOUT"]) == RG.FANOUT == meshdist.FANOUT == 8
    assert int(defs["STA_REG_MAX_LEVELS"]) == int(dist["STA_DIST_MAX_LEVELS"]) == RG.MAX_LEVELS == meshdist.MAX_LEVELS == 9
    assert int(defs["STA_REG_N_VALID"]) == int(dist["STA_DIST_N_VALID"]) == RG.N_VALID == 0
    assert int(defs["STA_REG_STATUS_BOUND"]) == RG.STATUS_BOUND == meshdist.REG_STATUS_BOUND == 1
    assert int(defs["STA_REG_PLAN_SIZES"]) == RG.PLAN_SIZES == meshdist.REG_PLAN_SIZES == 2
    assert int(defs["STA_REG_RECORD"]) == RG.RECORD == meshdist.REG_RECORD == 64
    kernels = (ROOT / "vista_slam_amd" / "csrc" / "reg.h").read_text()
    assert re.search(r"#define RG_F 8\b", kernels) and re.search(r"#define RG_MAX_LEVELS 9\b", kernels) and "#pragma clang fp contract(off)" in kernels
    assert re.search(r"#define RG_RECORD 64\b", kernels) and re.search(r"#define RG_USED 50\b", kernels)
    # the one atomic is the integer OR of the status bit
    assert re.findall(r"\batomic\w+\s*\(", kernels) == ["atomicOr("] and "atomicOr(P.status, RG_STATUS_BOUND)" in kernels
    flat = " ".join(text.replace(" * ", " ").split())
    for sentence in ("q' IS NOT ROUNDED TO FLOAT32", "THE CLAMP IS PART OF THE CONTRACT", "THAT ARGUMENT NOWHERE USES THAT q IS A FLOAT32",
                     "still visited, for the tie rule", "Rejection happens AFTER the search", "without floating-point atomics",
                     "in an order that depends on Q alone", "cloud.kabsch takes it as it is"):
        assert sentence in flat, sentence
    # the two libraries it sits next to keep their own sentences: nothing of them changed
    for other in ("sta_dist.h", "sta_ray.h"):
        assert "no point-to-plane ICP against the mesh" in " ".join((ROOT / "include" / other).read_text().replace(" * ", " ").split())


def test_the_plan_and_the_refusals_without_a_gpu():
    from vista_slam_amd import meshdist
    for nt, Q in ((1, 1), (8, 255), (9, 256), (65, 257), (513, 256 * 257 + 1), ((1 << 27) - 1, (1 << 30) - 1)):
        assert tuple(meshdist.reg_plan(nt, Q)) == RG.plan(nt, Q), (nt, Q)
        assert meshdist.reg_plan(nt, Q).nodes == meshdist.ray_plan(nt)
    for nt, Q in ((0, 1), (-3, 1), (1 << 27, 1), (1, 0), (1, 1 << 30)):
        with pytest.raises(ValueError) as lib:
            meshdist.reg_plan(nt, Q)
        with pytest.raises(ValueError) as mine:
            RG.plan(nt, Q)
        assert str(lib.value) == str(mine.value) and str(nt if not 1 <= nt < 1 << 27 else Q) in str(lib.value)
        with pytest.raises(ValueError, match="reg_pass: (nt|Q) must be in"):
            meshdist.reg_check(nt, Q)
    meshdist.reg_check(100, 1000)
    meshdist.reg_check(100, 1000, radius=float("inf"), min_cos=-1.0)
    meshdist.reg_check(100, 1000, radius=0.0, min_cos=2.0)
    for radius in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="reg_pass: radius must be >= 0"):
            meshdist.reg_check(100, 1000, radius=radius)
    with pytest.raises(ValueError, match="reg_pass: min_cos must not be NaN"):
        meshdist.reg_check(100, 1000, min_cos=float("nan"))
    # a record without a workspace, or with a short one: the numbers are in the message
    from vista_slam_amd import _lib
    lib = _lib.load_reg()
    one = (C.c_double * 64)()
    for work, nbytes in ((None, 1 << 20), (C.addressof(one), 1024)):
        rc = lib.sta_reg_pass(None, None, None, None, 100, None, None, 1000, None, None, 1.0, 0.0, None, None, None, None, C.addressof(one), work, nbytes, None, None)
        assert rc != 0 and b"reg_pass: work of 2048 bytes is required for Q = 1000" in lib.sta_reg_last_error()


def test_every_stream_entry_point_has_a_row_and_none_may_wait():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_reg_pass"], taking
    named = RS.named_entries()
    assert not (named & set(RS.EXEMPT))
    assert not set(taking) - named - set(RS.EXEMPT), sorted(set(taking) - named - set(RS.EXEMPT))
    assert not (named | set(RS.EXEMPT)) - set(taking) - RS.OTHER_LIBRARIES, sorted((named | set(RS.EXEMPT)) - set(taking))
    names = [r.name for r in RS.ROWS]
    assert len(names) == len(set(names))
    for r in RS.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run) and callable(r.make_b), r.name
        assert not RS.may_wait(r)
    assert RS.SYNCS == {}, "no call of this library may wait"
    header = " ".join(HEADER.read_text().split())
    assert "NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES" in header.replace(" * ", " ")
    # ... and the translation unit holds no call that could: no allocation, no copy, no synchronisation
    unit = (ROOT / "vista_slam_amd" / "csrc" / "sta_reg.hip").read_text()
    assert not re.findall(r"\bhip(?:Malloc|Free|Memcpy|Memset|StreamSynchronize|DeviceSynchronize|EventSynchronize)\w*\s*\(", unit)
