"""Host only: libsta_knn.so exports exactly include/sta_knn.h, the ctypes table mirrors it, no name collides with the eleven other
tables, sta_knn_grid restates sta_nn_index field by field, the constants hold, the library is a library of its own (own files, hash,
staleness; no file of the cloud library in its list and the other way round), the plan refuses what the header says with the numbers
in the message, and every declaration that takes a stream has a row in tests/knn_stream_cases.py (and the other way round) and none of
them may wait.  This test pins the library's OWN row of build.LATER, not the length of that table: the next library is one more row."""
import ctypes as C
import inspect
import os
import pathlib
import re

import pytest

import knn_cases as KC
import knn_stream_cases as KS
from test_cabi_symbols import all_exported
from test_library_table import MARKS
from test_stream_inventory import stream_entry_points

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "sta_knn.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}
OTHERS = ("SIGNATURES", "TEST_SIGNATURES", "SKEW_SIGNATURES", "CLOUD_SIGNATURES", "RASTER_SIGNATURES", "TSDF_SIGNATURES", "MESH_SIGNATURES", "SURF_SIGNATURES",
          "SIMP_SIGNATURES", "DIST_SIGNATURES", "RAY_SIGNATURES", "REG_SIGNATURES")
INCLUDE = r'#include\s+[<"]([^>"]+)[>"]'
NAMES = {"sta_knn_plan", "sta_knn_query", "sta_knn_moments", "sta_knn_last_error"}


def _earlier(build):
    return list(build.SATELLITES) + list(build.ADDONS) + list(build.EXTENSIONS)


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 4, every
    assert set(every) == set(_lib.KNN_SIGNATURES) == NAMES
    assert all_exported(_lib.KNN_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.KNN_LIB_PATH) - LINKER ^ set(every))
    for table in OTHERS:
        assert not set(every) & set(getattr(_lib, table)), (table, sorted(set(every) & set(getattr(_lib, table))))
    # the marks of tests/test_library_table.py: none of its names carries another library's, nobody else's carries its prefix
    for name in every:
        assert not [k for k, mark in MARKS.items() if mark(name)] and not name.startswith(("sta_ray_", "sta_reg_")), name
    lib = _lib.load_knn()
    for name in every:
        assert hasattr(lib, name), name
    for name in _earlier(build):
        assert not {s for s in all_exported(getattr(build, name.upper() + "_LIB")) if s.startswith("sta_knn_")}, name
    assert not {s for table in OTHERS for s in getattr(_lib, table) if s.startswith("sta_knn_")}


def test_it_is_a_library_of_its_own():
    from vista_slam_amd import _lib, build
    build.build_lib()
    assert "knn" in build.LATER and not set(build.LATER) & set(_earlier(build))          # its own row, not the table's length
    inc = os.path.join("..", "..", "include")
    own = set(build.LATER["knn"][1])
    assert own == {"sta_knn.hip", "knn.h", os.path.join(inc, "sta_knn.h")} and build.LATER["knn"][2] == []
    assert sorted(build.KNN_DEPS) == sorted(own | {"sta_exports.map", "sta_common.h", "sta_hostkit.h"}) and len(build.KNN_DEPS) == len(set(build.KNN_DEPS))
    for d in build.KNN_DEPS:
        assert os.path.exists(os.path.join(build.CSRC, d)), d
    assert build.KNN_SOURCES == ["sta_knn.hip"] and os.path.basename(build.KNN_LIB) == "libsta_knn.so" and build.KNN_HASH_FILE == build.KNN_LIB + ".srchash"
    assert _lib.KNN_LIB_PATH == build.KNN_LIB
    assert inspect.signature(build.build_lib).parameters["knn"].default is True
    others = {"mi355": (build.DEPS, {"sta_api.hip", "sta_launch.inc", "sta_forward.inc", "sta_debug.inc", "sta_rows.inc", "sta_bench.inc",
                                     os.path.join(inc, "sta_mi355.h"), os.path.join(inc, "sta_mi355_debug.h")})}
    for table in (build.SATELLITES, build.ADDONS, build.EXTENSIONS, build.LATER):
        for name, (_what, mine, _shared) in table.items():
            if name != "knn":
                others[name] = (getattr(build, name.upper() + "_DEPS"), set(mine))
    assert len(others) >= 10 and "cloud" in others
    for name, (deps, mine) in others.items():
        assert not own & set(deps), (name, own & set(deps))            # none of its own files is in another library's list
        assert not mine & set(build.KNN_DEPS), (name, mine & set(build.KNN_DEPS))          # ... and none of theirs in its list
    assert others["cloud"][1] == {"sta_cloud.hip", "cloud.h", os.path.join(inc, "sta_cloud.h")}
    hashes = {build.source_hash(deps) for deps, _mine in others.values()} | {build.source_hash(None, build.SKEW_FLAGS)}
    assert len(hashes) == len(others) + 1 and build.source_hash(build.KNN_DEPS) not in hashes
    assert not build.is_stale(build.KNN_LIB, build.KNN_HASH_FILE, build.KNN_DEPS)
    # the translation unit and the kernels include nothing of libsta_cloud.so or of the sort, and the kernels sta_common.h alone
    for f in ("sta_knn.hip", "knn.h"):
        includes = re.findall(INCLUDE, (pathlib.Path(build.CSRC) / f).read_text())
        assert not [i for i in includes if "cloud" in i or i in ("voxel.h", "select.h", "elementwise.h")], (f, includes)
    assert re.findall(INCLUDE, (pathlib.Path(build.CSRC) / "knn.h").read_text()) == ["sta_common.h"]
    assert re.findall(INCLUDE, (pathlib.Path(build.CSRC) / "sta_knn.hip").read_text()) == ["../../include/sta_knn.h", "sta_common.h", "sta_hostkit.h", "knn.h", "cmath"]
    assert re.findall(INCLUDE, HEADER.read_text()) == ["stdint.h"]
    # ... and nothing of the cloud library names this one
    for f in ("sta_cloud.hip", "cloud.h", os.path.join(inc, "sta_cloud.h")):
        assert "knn" not in (pathlib.Path(build.CSRC) / f).read_text().lower(), f


def _ctype_of(param):
    """the ctypes type a C parameter of include/sta_knn.h maps to: the host arrays are typed, every other pointer is void*"""
    from vista_slam_amd import _lib
    p = re.sub(r"\bconst\b", "", param).strip()
    name = re.search(r"(\w+)$", p).group(1)
    base = p[:-len(name)].replace(" ", "")
    if base.endswith("*"):
        if name == "grid_host":
            return C.POINTER(_lib.StaNNIndex)
        return C.POINTER(C.c_int64) if name == "sizes_out" else C.POINTER(C.c_double) if name.endswith("_host") else C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}[base]


def _fields(text, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    return [(" ".join(t.split()), n, dim) for t, n, dim in re.findall(r"([\w ]+?\*?)\s*(\w+)(\[[^\]]+\])?;", body)]


def test_the_ctypes_table_mirrors_the_header():
    from vista_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bSTA_API\b\s*([^;(]*?)\b(sta_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(decls) == 4
    for ret, name, params in decls:
        res, args = _lib.KNN_SIGNATURES[name]
        assert res is (C.c_char_p if "char" in ret else C.c_int), name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert len(plist) == len(args), (name, len(plist), len(args))
        for p, a in zip(plist, args):
            assert a is _ctype_of(p), (name, p, a, _ctype_of(p))
    names = {n: [re.search(r"(\w+)$", p.strip()).group(1) for p in params.split(",")] for _r, n, params in decls}
    assert names["sta_knn_plan"] == ["M", "Q", "k", "sizes_out"]
    assert names["sta_knn_query"] == ["grid_host", "qry", "Q", "order", "self_base", "k", "radius", "d2_out", "idx_out", "count_out", "status", "stream"]
    assert names["sta_knn_moments"] == ["ref", "M", "qry", "Q", "d2", "idx", "count", "k", "view", "view_host", "min_count", "normal_out", "curv_out",
                                        "mean_dist_out", "record_out", "work", "work_bytes", "stream"]


def test_the_grid_struct_is_the_index_of_the_cloud_library():
    from vista_slam_amd import _lib
    mine = _fields(HEADER.read_text(), "sta_knn_grid")
    theirs = _fields((ROOT / "include" / "sta_cloud.h").read_text(), "sta_nn_index")
    assert mine == theirs and len(mine) == 10, (mine, theirs)
    assert [n for _t, n, _d in mine] == [n for n, _t in _lib.StaNNIndex._fields_]
    assert [n for _t, n, _d in mine] == ["cell_key", "cell_start", "sorted_pts", "sorted_idx", "lo", "ext", "cell", "M", "n_finite", "C"]


def test_the_constants_hold():
    from vista_slam_amd import cloud
    text = HEADER.read_text()
    defs = dict(re.findall(r"#define\s+(STA_KNN_\w+)\s+([^\s/]+)", text))
    nn = dict(re.findall(r"#define\s+(STA_NN_\w+)\s+([^\s/]+)", (ROOT / "include" / "sta_cloud.h").read_text()))
    assert int(defs["STA_KNN_MAX_RINGS"]) == int(nn["STA_NN_MAX_RINGS"]) == KC.MAX_RINGS == cloud.MAX_RINGS == 32
    assert int(defs["STA_KNN_MAX_K"]) == KC.MAX_K == cloud.KNN_MAX_K == 64
    assert int(defs["STA_KNN_RECORD"]) == KC.RECORD == cloud.KNN_RECORD == 8
    assert int(defs["STA_KNN_MIN_COUNT"]) == KC.MIN_COUNT == cloud.KNN_MIN_COUNT == 3
    assert int(defs["STA_KNN_PLAN_SIZES"]) == len(cloud.KnnPlan._fields) == 3
    assert (int(defs["STA_KNN_STATUS_BOUND"]), int(defs["STA_KNN_STATUS_ORDER"])) == (KC.STATUS_BOUND, KC.STATUS_ORDER) == (cloud.KNN_STATUS_BOUND, cloud.KNN_STATUS_ORDER) == (1, 2)
    kernels = (ROOT / "vista_slam_amd" / "csrc" / "knn.h").read_text()
    assert re.search(r"#define KN_MAX_K 64\b", kernels) and re.search(r"#define KN_RECORD 8\b", kernels) and re.search(r"#define KN_SWEEPS 8\b", kernels)
    assert "#pragma clang fp contract(off)" in kernels and "1.0 - 9.313225746154785e-10" in kernels and 1.0 - 9.313225746154785e-10 == 1.0 - 2.0 ** -30
    assert "1.0 - 9.313225746154785e-10" in (ROOT / "vista_slam_amd" / "csrc" / "cloud.h").read_text()          # the margin of sta_nn_query
    # the only atomics are integer ORs of a status bit
    assert set(re.findall(r"\batomic\w+\s*\(", kernels)) == {"atomicOr("}
    assert set(re.findall(r"atomicOr\(([^)]*)\)", kernels)) == {"P.status, KN_STATUS_BOUND", "P.status, KN_STATUS_ORDER"}
    # the list lives in dynamic LDS and no private array is indexed at run time: the kernels declare no local array at all
    assert "extern __shared__ __attribute__((aligned(16))) char kn_smem[];" in kernels
    code = "\n".join(line.split("//")[0] for line in kernels.splitlines())
    code = re.sub(r"struct \w+ \{[^}]*\};", "", code)                     # (kernel arguments: indexed by constants only)
    assert not re.findall(r"^\s+(?:const\s+)?(?:double|float|int|long long)\s+\w+\[[^\]]+\]\s*(?:=|;)", code, flags=re.M)
    flat = " ".join(text.replace(" * ", " ").split())
    for sentence in ("NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES", "There is no T", "Why that is exact for the k-th element",
                     "The argument nowhere uses k", "never a bit of the output", "without floating-point atomics", "in an order that depends on Q alone",
                     "An entry outside [0, Q) is skipped", "an index outside [0, M) ends that query's list there", "Negation is exact"):
        assert sentence in flat, sentence


def test_the_plan_and_the_refusals_without_a_gpu():
    from vista_slam_amd import _lib, cloud
    lib = _lib.load_knn()
    for M, Q, k in ((1, 1, 1), (8, 255, 7), (9, 256, 64), (3000, 257, 33), (5, 256 * 2048 + 1, 2), ((1 << 30) - 1, (1 << 30) - 1, 64)):
        out = (C.c_int64 * 3)()
        assert lib.sta_knn_plan(M, Q, k, out) == 0
        assert tuple(out) == KC.plan(M, Q, k) == tuple(cloud.knn_plan(M, Q, k)), (M, Q, k)
    for M, Q, k in ((0, 1, 1), (-3, 1, 1), (1 << 30, 1, 1), (1, 0, 1), (1, 1 << 30, 1), (1, 1, 0), (1, 1, 65)):
        out = (C.c_int64 * 3)()
        assert lib.sta_knn_plan(M, Q, k, out) != 0
        said = lib.sta_knn_last_error().decode()
        with pytest.raises(ValueError) as mine:
            KC.plan(M, Q, k)
        assert said == str(mine.value) and str(M if not 1 <= M < 1 << 30 else Q if not 1 <= Q < 1 << 30 else k) in said
    # the query's refusals, on a struct that names no memory: all are decided before anything is launched
    g = _lib.StaNNIndex()
    g.cell, g.M, g.n_finite, g.C = 0.125, 100, 100, 10
    for a in range(3):
        g.ext[a] = 4
    one = (C.c_int32 * 1)()

    def query(Q=10, k=8, radius=1.0, grid=g):
        rc = lib.sta_knn_query(C.byref(grid), None, Q, None, -1, k, radius, None, None, None, C.addressof(one), None)
        assert rc != 0
        return lib.sta_knn_last_error().decode()
    assert query(radius=float("nan")).startswith("knn_query: radius must be finite and >= 0") and "radius must be finite" in query(radius=-0.5)
    assert "radius must be finite" in query(radius=float("inf"))
    assert query(radius=4.0) == "knn_query: null argument"                          # exactly 32 cells passes the radius check
    assert "is more than 32 cells of 0.125" in query(radius=4.000000000000001)
    assert "k must be in [1, 64] (got 65)" in query(k=65) and "k must be in [1, 64] (got 0)" in query(k=0) and "Q must be in [1, 2^30) (got 0)" in query(Q=0)
    bad = _lib.StaNNIndex()
    assert query(grid=bad) == "knn_query: not an index of sta_nn_build"
    # the moments' refusals
    def moments(M=100, Q=10, k=8, min_count=3, record=None, work=None, nbytes=0):
        rc = lib.sta_knn_moments(None, M, None, Q, None, None, None, k, None, None, min_count, None, None, None, record, work, nbytes, None)
        assert rc != 0
        return lib.sta_knn_last_error().decode()
    assert moments() == "knn_moments: null argument"
    assert "min_count must be at least 3 (got 2)" in moments(min_count=2) and "M must be in [1, 2^30) (got 0)" in moments(M=0)
    rec = (C.c_double * 8)()
    for work, nbytes in ((None, 1 << 20), (C.addressof(rec), 64)):
        assert "knn_moments: work of 256 bytes is required for Q = 1000" in moments(Q=1000, record=C.addressof(rec), work=work, nbytes=nbytes)


def test_every_stream_entry_point_has_a_row_and_none_may_wait():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_knn_moments", "sta_knn_query"], taking
    named = KS.named_entries()
    assert not (named & set(KS.EXEMPT))
    assert not set(taking) - named - set(KS.EXEMPT), sorted(set(taking) - named - set(KS.EXEMPT))
    assert not (named | set(KS.EXEMPT)) - set(taking) - KS.OTHER_LIBRARIES, sorted((named | set(KS.EXEMPT)) - set(taking))
    names = [r.name for r in KS.ROWS]
    assert len(names) == len(set(names))
    for r in KS.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run) and callable(r.make_b), r.name
        assert not KS.may_wait(r)
    assert KS.SYNCS == {}, "no call of this library may wait"
    header = " ".join(HEADER.read_text().split())
    assert "NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES" in header.replace(" * ", " ")
    # ... and the translation unit holds no call that could: no allocation, no copy, no synchronisation
    unit = (ROOT / "vista_slam_amd" / "csrc" / "sta_knn.hip").read_text()
    assert not re.findall(r"\bhip(?:Malloc|Free|Memcpy|Memset|StreamSynchronize|DeviceSynchronize|EventSynchronize)\w*\s*\(", unit)
