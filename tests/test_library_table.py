"""Host only: the eight libraries are libraries of their own.  Over every ordered pair of them, no library's own files are among the
sources another one's content hash covers, the eight hashes differ, the export tables are pairwise disjoint, no library exports a name
with another's prefix, none is stale after build_lib(), and the product exports exactly include/sta_mi355.h."""
import itertools
import os

from test_cabi_symbols import all_exported, declared_symbols, exported_symbols

LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}
# what marks an exported name as a library's own (the product's sta_world_pointcloud is older than libsta_cloud.so)
MARKS = {
    "cloud": lambda s: ("cloud_" in s or s.startswith("sta_nn_")) and s != "sta_world_pointcloud",
    "raster": lambda s: "raster" in s,
    "tsdf": lambda s: "tsdf" in s,
    "mesh": lambda s: s.startswith("sta_mesh"),
    "surf": lambda s: s.startswith("sta_surf"),
    "simp": lambda s: s.startswith("sta_simp"),
    "dist": lambda s: s.startswith("sta_tri"),
}


def table():
    """name -> (library, hash file, dependency list, own files, ctypes table); the product is "mi355" """
    from vista_slam_amd import _lib, build
    own = {"sta_api.hip", "sta_launch.inc", "sta_forward.inc", "sta_debug.inc", "sta_rows.inc", "sta_bench.inc", os.path.join("..", "..", "include", "sta_mi355.h"),
           os.path.join("..", "..", "include", "sta_mi355_debug.h")}
    rows = {"mi355": (build.LIB, build.HASH_FILE, build.DEPS, own, _lib.SIGNATURES)}
    for name, (_what, mine, _shared) in build.SATELLITES.items():
        up = name.upper()
        rows[name] = (getattr(build, up + "_LIB"), getattr(build, up + "_HASH_FILE"), getattr(build, up + "_DEPS"), set(mine), getattr(_lib, up + "_SIGNATURES"))
        assert getattr(_lib, up + "_LIB_PATH") == rows[name][0] and getattr(build, up + "_SOURCES") == ["sta_%s.hip" % name]
        assert os.path.basename(rows[name][0]) == "libsta_%s.so" % name and rows[name][1] == rows[name][0] + ".srchash"
    return rows


def test_the_table_names_eight_libraries_and_their_own_files():
    from vista_slam_amd import build
    rows = table()
    assert list(rows) == ["mi355", "cloud", "raster", "tsdf", "mesh", "surf", "simp", "dist"] == ["mi355"] + list(MARKS)
    inc = os.path.join("..", "..", "include")
    for name, (_lib_path, _hf, deps, own, _sig) in rows.items():
        assert own <= set(deps) and len(deps) == len(set(deps)), name
        for d in deps:
            assert os.path.exists(os.path.join(build.CSRC, d)), (name, d)
        if name not in ("mi355", "raster"):
            assert own == {"sta_%s.hip" % name, name + ".h", os.path.join(inc, "sta_%s.h" % name)}
    # the rasteriser's kernel header and limits are shared with the mesh library alone
    for shared in ("raster.h", os.path.join(inc, "sta_raster.h")):
        assert [n for n, row in rows.items() if shared in row[2]] == ["raster", "mesh"]
    assert rows["raster"][3] == {"sta_raster.hip"}
    # the host kit is every handle-free library's and not the product's, whose REQUIRE, HIPCHK and Bump are its own
    assert [n for n, row in rows.items() if "sta_hostkit.h" in row[2]] == list(MARKS)


def test_no_library_is_built_from_anothers_own_files():
    rows = table()
    for a, b in itertools.permutations(rows, 2):
        assert not rows[a][3] & set(rows[b][2]), (a, b, rows[a][3] & set(rows[b][2]))


def test_the_eight_hashes_differ_and_none_is_stale():
    from vista_slam_amd import build
    build.build_lib()
    rows = table()
    assert len({build.source_hash(row[2]) for row in rows.values()}) == 8
    assert build.source_hash() == build.source_hash(build.DEPS)
    for name, (lib, hash_file, deps, _own, _sig) in rows.items():
        assert not build.is_stale(lib, hash_file, deps), name
    assert not build.is_stale(build.TEST_LIB, build.TEST_HASH_FILE)
    assert not build.is_stale(build.SKEW_LIB, build.SKEW_HASH_FILE, None, build.SKEW_FLAGS)
    assert build.is_stale(build.SKEW_LIB, build.SKEW_HASH_FILE)       # its hash covers its flags: not the product's hash


def test_the_exports_are_disjoint_and_the_product_exports_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    rows = table()
    exported = {name: all_exported(row[0]) - LINKER for name, row in rows.items()}
    assert exported_symbols(_lib.LIB_PATH) == declared_symbols("sta_mi355.h") == set(_lib.SIGNATURES) == exported["mi355"]
    for name, row in rows.items():
        assert exported[name] == set(row[4]), (name, exported[name] ^ set(row[4]))
    for a, b in itertools.permutations(rows, 2):
        assert not exported[a] & exported[b], (a, b, exported[a] & exported[b])
        assert not set(rows[a][4]) & set(_lib.TEST_SIGNATURES)
        if a != "mi355":
            assert not {s for s in exported[b] if MARKS[a](s)}, (a, b)
    for name, mark in MARKS.items():
        assert all(mark(s) for s in exported[name]), (name, [s for s in exported[name] if not mark(s)])
