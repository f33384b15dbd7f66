"""Host only: libsta_ray.so exports exactly include/sta_ray.h, the ctypes table mirrors it, no name collides with the nine other tables,
the library is a library of its own (for the ninth what tests/test_library_table.py checks for eight: own files, hash, staleness), the
constants it restates are those of include/sta_dist.h, and every declaration that takes a stream has a row in
tests/ray_stream_cases.py (and the other way round) and none of them may wait."""
import ctypes as C
import inspect
import os
import pathlib
import re

import ray_cases as RC
import ray_stream_cases as RS
from test_cabi_symbols import all_exported
from test_stream_inventory import stream_entry_points

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "sta_ray.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}
OTHERS = ("SIGNATURES", "TEST_SIGNATURES", "CLOUD_SIGNATURES", "RASTER_SIGNATURES", "TSDF_SIGNATURES", "MESH_SIGNATURES", "SURF_SIGNATURES", "SIMP_SIGNATURES",
          "DIST_SIGNATURES")


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 4, every
    assert set(every) == set(_lib.RAY_SIGNATURES), set(every) ^ set(_lib.RAY_SIGNATURES)
    assert all(name.startswith("sta_ray_") for name in every)
    assert all_exported(_lib.RAY_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.RAY_LIB_PATH) - LINKER ^ set(every))
    for table in OTHERS:
        assert not set(every) & set(getattr(_lib, table)), (table, sorted(set(every) & set(getattr(_lib, table))))
    lib = _lib.load_ray()
    for name in every:
        assert hasattr(lib, name), name
    # no other handle-free library exports a name with this one's prefix (the product's sta_ray_depth is older than libsta_ray.so)
    for name in build.SATELLITES:
        assert not {s for s in all_exported(getattr(build, name.upper() + "_LIB")) if s.startswith("sta_ray_")}, name
    assert {s for s in _lib.SIGNATURES if s.startswith("sta_ray_")} == {"sta_ray_depth"}


def test_it_is_a_library_of_its_own():
    from vista_slam_amd import _lib, build
    build.build_lib()
    assert list(build.ADDONS) == ["ray"] and len(build.SATELLITES) == 7 and not set(build.ADDONS) & set(build.SATELLITES)
    inc = os.path.join("..", "..", "include")
    own = set(build.ADDONS["ray"][1])
    assert own == {"sta_ray.hip", "ray.h", os.path.join(inc, "sta_ray.h")}
    assert sorted(build.RAY_DEPS) == sorted(own | {"sta_exports.map", "sta_common.h", "sta_hostkit.h"}) and len(build.RAY_DEPS) == len(set(build.RAY_DEPS))
    for d in build.RAY_DEPS:
        assert os.path.exists(os.path.join(build.CSRC, d)), d
    assert build.RAY_SOURCES == ["sta_ray.hip"] and os.path.basename(build.RAY_LIB) == "libsta_ray.so" and build.RAY_HASH_FILE == build.RAY_LIB + ".srchash"
    assert _lib.RAY_LIB_PATH == build.RAY_LIB
    assert inspect.signature(build.build_lib).parameters["ray"].default is True
    others = {"mi355": (build.DEPS, {"sta_api.hip", "sta_launch.inc", "sta_forward.inc", "sta_debug.inc", "sta_rows.inc", "sta_bench.inc",
                                     os.path.join(inc, "sta_mi355.h"), os.path.join(inc, "sta_mi355_debug.h")})}
    for name, (_what, mine, _shared) in build.SATELLITES.items():
        others[name] = (getattr(build, name.upper() + "_DEPS"), set(mine))
    assert len(others) == 8
    for name, (deps, mine) in others.items():
        assert not own & set(deps), (name, own & set(deps))            # none of its own files is in another library's list
        assert not mine & set(build.RAY_DEPS), (name, mine & set(build.RAY_DEPS))          # ... and none of theirs in its list
    hashes = {build.source_hash(deps) for deps, _mine in others.values()}
    assert len(hashes) == 8 and build.source_hash(build.RAY_DEPS) not in hashes
    assert not build.is_stale(build.RAY_LIB, build.RAY_HASH_FILE, build.RAY_DEPS)
    # the translation unit and the kernels include nothing of libsta_dist.so
    for f in ("sta_ray.hip", "ray.h"):
        text = (pathlib.Path(build.CSRC) / f).read_text()
        includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
        assert not [i for i in includes if "dist" in i or i in ("voxel.h", "select.h", "elementwise.h")], (f, includes)
    assert "sta_dist.h" not in re.findall(r'#include\s+[<"]([^>"]+)[>"]', HEADER.read_text())


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_ray.h maps to: the host size array is typed, every other pointer is void*"""
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
        res, args = _lib.RAY_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            assert a is _ctype_of(p), (name, p, a, _ctype_of(p))
    # the index goes in as the four pointers and nt of sta_tri_index, in the order of its fields
    dist = (ROOT / "include" / "sta_dist.h").read_text()
    body = re.search(r"typedef struct sta_tri_index \{(.*?)\} sta_tri_index;", dist, flags=re.S).group(1)
    fields = [n for _k, n in re.findall(r"(float\*|int32_t\*|int64_t|int32_t)\s+(\w+)(?:\[[^\]]+\])?;", body)][:5]
    for _ret, name, params in decls:
        if name in ("sta_ray_cast", "sta_ray_occluded"):
            assert [re.search(r"(\w+)$", p.strip()).group(1) for p in params.split(",")][:5] == fields == ["tri", "src", "boxes", "counters", "nt"]


def test_the_constants_are_those_of_the_index():
    from vista_slam_amd import meshdist
    text = HEADER.read_text()
    defs = dict(re.findall(r"#define\s+(STA_RAY_\w+)\s+([^\s/]+)", text))
    dist = dict(re.findall(r"#define\s+(STA_DIST_\w+)\s+([^\s/]+)", (ROOT / "include" / "sta_dist.h").read_text()))
    assert int(defs["STA_RAY_FANOUT"]) == int(dist["STA_DIST_FANOUT"]) == RC.FANOUT == meshdist.FANOUT == 8
    assert int(defs["STA_RAY_MAX_LEVELS"]) == int(dist["STA_DIST_MAX_LEVELS"]) == RC.MAX_LEVELS == meshdist.MAX_LEVELS == 9
    assert int(defs["STA_RAY_N_VALID"]) == int(dist["STA_DIST_N_VALID"]) == RC.N_VALID == 0
    assert int(defs["STA_RAY_STATUS_BOUND"]) == RC.STATUS_BOUND == meshdist.RAY_STATUS_BOUND == 1
    assert int(defs["STA_RAY_PLAN_SIZES"]) == RC.PLAN_SIZES == meshdist.RAY_PLAN_SIZES == 1
    kernels = (ROOT / "vista_slam_amd" / "csrc" / "ray.h").read_text()
    assert re.search(r"#define RY_F 8\b", kernels) and re.search(r"#define RY_MAX_LEVELS 9\b", kernels) and "#pragma clang fp contract(off)" in kernels
    assert "atomicAdd" not in kernels and "atomicMin" not in kernels and "atomicMax" not in kernels          # the one atomic is the integer status OR
    assert len(re.findall(r"\batomic\w+\s*\(", kernels)) == 1 and "atomicOr(P.status" in kernels
    flat = " ".join(text.replace(" * ", " ").split())
    for sentence in ("No signed distance", "no crossing parity", "no all-hits list", "no point-to-plane ICP against the mesh",
                     "THE OWN-BOX TEST AND THE CLAMP ARE PART OF THE CONTRACT", "with no margin at all", "still be visited, for the tie rule",
                     "It was not compared with Open3D's RaycastingScene", "NOT normalised"):
        assert sentence in flat, sentence
    # sta_dist.h keeps its own sentences (tests/test_dist_abi.py): nothing of that library changed
    assert "no ray casting" in " ".join((ROOT / "include" / "sta_dist.h").read_text().replace(" * ", " ").split())


def test_every_stream_entry_point_has_a_row_and_none_may_wait():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_ray_cast", "sta_ray_occluded"], taking
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
    unit = (ROOT / "vista_slam_amd" / "csrc" / "sta_ray.hip").read_text()
    assert not re.findall(r"\bhip(?:Malloc|Free|Memcpy|Memset|StreamSynchronize|DeviceSynchronize|EventSynchronize)\w*\s*\(", unit)
