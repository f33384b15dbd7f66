"""Build the gfx950 C-ABI libraries in-tree with hipcc (no torch, no cmake).

    python -m vista_slam_amd.build          # -> vista_slam_amd/libsta_mi355.so        the product: exports include/sta_mi355.h only
                                            #    vista_slam_amd/libsta_mi355_test.so   the same translation unit + -DSTA_TEST_HOOKS:
                                            #    additionally the kernel-level test / micro-benchmark entry points of
                                            #    include/sta_mi355_debug.h (loaded by tests/ and tools/ only)
                                            #    vista_slam_amd/libsta_mi355_skew.so   the same again + -DSTA_WAVE_SKEW: the skew points of
                                            #    csrc/sta_skew.h are live and the two sta_debug_*wave_skew* entries exist
                                            #    (tests/test_skew_gpu.py only; in every other library the points expand to nothing)
                                            #    vista_slam_amd/libsta_<name>.so       one handle-free library per row of SATELLITES:
                                            #    of ADDONS, of EXTENSIONS and of LATER: a translation unit of its own (csrc/sta_<name>.hip) that exports
                                            #    include/sta_<name>.h

A library's content hash covers its own files and the shared headers it includes, nothing of any other library: the product's hash does
not move when a satellite's own files change, and the other way round (tests/test_library_table.py).
"""
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libsta_mi355.so")
TEST_LIB = os.path.join(PKG, "libsta_mi355_test.so")
SKEW_LIB = os.path.join(PKG, "libsta_mi355_skew.so")
SOURCES = ["sta_api.hip"]
DEPS = ["sta_exports.map", "sta_api.hip", "sta_launch.inc", "sta_forward.inc", "sta_debug.inc", "sta_rows.inc", "sta_bench.inc", "gemm.h", "gemm2.h", "conv3h.h", "attention.h", "elementwise.h", "geo.h", "select.h", "voxel.h", "flow.h", "loop.h", "pgo.h", "graph.h", "sta_common.h", "sta_skew.h",
        os.path.join("..", "..", "include", "sta_mi355.h"), os.path.join("..", "..", "include", "sta_mi355_debug.h"),
        os.path.join("..", "..", "include", "sta_mi355_skew.h")]


def _inc(name):
    return os.path.join("..", "..", "include", name)


# The handle-free libraries.  name: (what it is, its own files, the shared headers it includes).  A library's own files are in no other
# library's dependency list; a shared header is in several.  raster.h and include/sta_raster.h are shared: the mesh library includes
# them for the camera and the limits of the canvas.
_SORT = ["voxel.h", "select.h", "elementwise.h", "sta_skew.h"]      # the sort and scan kernels with their launch code, and what they include (the
                                                                     # skew points of sta_skew.h expand to nothing in these libraries)
_RASTER = ["raster.h", _inc("sta_raster.h")]
SATELLITES = {
    "cloud": ("nearest neighbours between clouds for the offline metrics", ["sta_cloud.hip", "cloud.h", _inc("sta_cloud.h")], _SORT),
    "raster": ("the headless z-buffer rasteriser of vista_slam_amd/render.py", ["sta_raster.hip"], _RASTER),
    "tsdf": ("sparse TSDF fusion and marching tetrahedra of vista_slam_amd/tsdf.py", ["sta_tsdf.hip", "tsdf.h", _inc("sta_tsdf.h")], _SORT),
    "mesh": ("triangles for the rasteriser's key buffer and vertex normals", ["sta_mesh.hip", "mesh.h", _inc("sta_mesh.h")], _RASTER + _SORT),
    "surf": ("connected components and area-uniform surface samples of a mesh", ["sta_surf.hip", "surf.h", _inc("sta_surf.h")], []),
    "simp": ("mesh simplification by vertex clustering with quadrics", ["sta_simp.hip", "simp.h", _inc("sta_simp.h")], _SORT),
    "dist": ("exact point-to-triangle distances over an implicit BVH", ["sta_dist.hip", "dist.h", _inc("sta_dist.h")], _SORT),
}
# The libraries that came after the table of seven was pinned (tests/test_library_table.py): rows of the same shape, expanded and built
# by the same loops.  libsta_ray.so reads the index of libsta_dist.so through plain arguments and holds no own file of another library.
ADDONS = {
    "ray": ("first hit and occlusion of rays over the triangle index of libsta_dist.so", ["sta_ray.hip", "ray.h", _inc("sta_ray.h")], []),
}
# ... and the libraries that came after that table of one was pinned in its turn (tests/test_ray_abi.py): the same rows, the same loops.
# libsta_reg.so reads the index of libsta_dist.so through plain arguments, as libsta_ray.so does.
EXTENSIONS = {
    "reg": ("point-to-plane and point-to-point registration against the triangle index of libsta_dist.so", ["sta_reg.hip", "reg.h", _inc("sta_reg.h")], []),
}
# ... and the libraries that came after that table of one was pinned as well (tests/test_reg_abi.py): the same rows, the same loops.
# Deliberately, the ABI test of a library in THIS table (tests/test_knn_abi.py) pins its own row and not the table's length, so the next
# library is one more row here and needs no fifth table.  libsta_knn.so reads the index of libsta_cloud.so through a host struct that
# its header restates and holds no own file of another library.
LATER = {
    "knn": ("k nearest neighbours on the grid of libsta_cloud.so and the moments of the neighbourhoods: cloud filters and normals",
            ["sta_knn.hip", "knn.h", _inc("sta_knn.h")], []),
}
# CLOUD_LIB, CLOUD_SOURCES, CLOUD_DEPS, CLOUD_HASH_FILE ... DIST_LIB, DIST_SOURCES, DIST_DEPS, DIST_HASH_FILE, RAY_LIB, RAY_SOURCES,
# RAY_DEPS, RAY_HASH_FILE, REG_LIB, REG_SOURCES, REG_DEPS, REG_HASH_FILE, KNN_LIB, KNN_SOURCES, KNN_DEPS, KNN_HASH_FILE: the rows of the four
# tables under the names that tools/ and tests/ use.  Every row is built from sta_common.h and the host kit as well.
for _name, (_what, _own, _shared) in list(SATELLITES.items()) + list(ADDONS.items()) + list(EXTENSIONS.items()) + list(LATER.items()):
    _so = os.path.join(PKG, "libsta_%s.so" % _name)
    globals().update({_name.upper() + "_LIB": _so, _name.upper() + "_SOURCES": _own[:1], _name.upper() + "_HASH_FILE": _so + ".srchash",
                      _name.upper() + "_DEPS": ["sta_exports.map"] + _own + _shared + ["sta_common.h", "sta_hostkit.h"]})


def hipcc_path():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


# -fvisibility=hidden: the dynamic symbol table is the STA_API declarations of include/*.h and nothing else (no __device_stub__
# launch stubs, no helpers); tests/test_cabi_symbols.py asserts it
# + a linker version script (csrc/sta_exports.map) for what visibility attributes cannot reach: hipcc's kernel handle objects,
# libstdc++ template instantiations, the __hip_cuid_ marker
BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-value",
              "-Wl,--version-script=" + os.path.join(CSRC, "sta_exports.map")]
HASH_FILE = LIB + ".srchash"
TEST_HASH_FILE = TEST_LIB + ".srchash"
SKEW_HASH_FILE = SKEW_LIB + ".srchash"
SKEW_FLAGS = ["-DSTA_TEST_HOOKS", "-DSTA_WAVE_SKEW"]


def extra_flags():
    """STA_DEV_FAST=1: development build without the precision-f16 kernel forms (half the compile time; the f16 tests fail
    loudly on it).  STA_BENCH_EXPERIMENTS=1: the retired tile shapes / main-loop ablations of tools/gemm_tiles.py."""
    f = []
    if os.environ.get("STA_DEV_FAST") == "1":
        f.append("-DSTA_DEV_FAST")
    if os.environ.get("STA_BENCH_EXPERIMENTS") == "1":
        f.append("-DSTA_BENCH_EXPERIMENTS")
    return f


def source_hash(deps=None, flags=()):
    """Content hash of every source the library is built from (mtimes do not survive the gpurun
    snapshot copy, so staleness is decided by content) and of the build flags.  deps: DEPS (the product and test-hooks
    libraries) unless given (a satellite's <NAME>_DEPS).  flags: further build flags that tell two builds of the same sources apart (the skew
    library's SKEW_FLAGS)."""
    import hashlib
    h = hashlib.sha256()
    h.update(" ".join([f.replace(CSRC, "csrc") for f in BASE_FLAGS] + extra_flags() + list(flags)).encode())      # (path-independent: the snapshot on the GPU box lives elsewhere)
    for d in (DEPS if deps is None else deps):
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def is_stale(lib=LIB, hash_file=HASH_FILE, deps=None, flags=()):
    if not os.path.exists(lib) or not os.path.exists(hash_file):
        return True
    with open(hash_file) as f:
        return f.read().strip() != source_hash(deps, flags)


def _cmd(hipcc, out, hooks, sources=None):
    """hooks: False, True (-DSTA_TEST_HOOKS) or a list of flags (SKEW_FLAGS)."""
    return ([hipcc] + BASE_FLAGS + ["-o", out] + extra_flags() +
            (list(hooks) if isinstance(hooks, list) else ["-DSTA_TEST_HOOKS"] if hooks else []) + [os.path.join(CSRC, s) for s in (SOURCES if sources is None else sources)])


def build_lib(force=False, verbose=True, test_hooks=True, skew=True, cloud=True, raster=True, tsdf=True, mesh=True, surf=True, simp=True, dist=True,
              ray=True, reg=True, knn=True):
    """Build the product library, (test_hooks) the test-hooks library, (skew) the wave-skew library and, each under the keyword of its name, the libraries of
    SATELLITES, ADDONS, EXTENSIONS and LATER; all compile concurrently (one hipcc process each, ~100 s).  Returns the product library's path."""
    wanted = dict(cloud=cloud, raster=raster, tsdf=tsdf, mesh=mesh, surf=surf, simp=simp, dist=dist, ray=ray, reg=reg, knn=knn)
    assert list(wanted) == list(SATELLITES) + list(ADDONS) + list(EXTENSIONS) + list(LATER)
    jobs = []           # (output, hash file, test hooks, sources, deps)
    if force or is_stale(LIB, HASH_FILE):
        jobs.append((LIB, HASH_FILE, False, None, None))
    if test_hooks and (force or is_stale(TEST_LIB, TEST_HASH_FILE)):
        jobs.append((TEST_LIB, TEST_HASH_FILE, True, None, None))
    if skew and (force or is_stale(SKEW_LIB, SKEW_HASH_FILE, None, SKEW_FLAGS)):
        jobs.append((SKEW_LIB, SKEW_HASH_FILE, SKEW_FLAGS, None, None))
    for name in wanted:
        lib, hash_file, sources, deps = (globals()[name.upper() + k] for k in ("_LIB", "_HASH_FILE", "_SOURCES", "_DEPS"))
        if wanted[name] and (force or is_stale(lib, hash_file, deps)):
            jobs.append((lib, hash_file, False, sources, deps))
    if not jobs:
        return LIB
    hipcc = hipcc_path()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot build libsta_mi355.so (ROCm toolchain required)")
    procs = []
    for out, _hf, hooks, sources, _deps in jobs:
        cmd = _cmd(hipcc, out, hooks, sources)
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        procs.append((subprocess.Popen(cmd, cwd=CSRC), cmd))
    failed = None
    for (p, cmd), (out, hf, hooks, _sources, deps) in zip(procs, jobs):
        if failed is not None:             # a sibling compile already failed: do not leave this one running un-waited
            p.kill()
            p.wait()
            continue
        if p.wait() != 0:
            failed = subprocess.CalledProcessError(p.returncode, cmd)
            continue
        with open(hf, "w") as f:
            f.write(source_hash(deps, hooks if isinstance(hooks, list) else ()))
    if failed is not None:
        raise failed
    return LIB


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)
    print(LIB)
