"""Build the gfx950 C-ABI libraries in-tree with hipcc (no torch, no cmake).

    python -m vista_slam_amd.build          # -> vista_slam_amd/libsta_mi355.so        the product: exports include/sta_mi355.h only
                                            #    vista_slam_amd/libsta_mi355_test.so   the same translation unit + -DSTA_TEST_HOOKS:
                                            #    additionally the kernel-level test / micro-benchmark entry points of
                                            #    include/sta_mi355_debug.h (loaded by tests/ and tools/ only)
                                            #    vista_slam_amd/libsta_cloud.so        a second, handle-free library: exports include/sta_cloud.h
                                            #    (nearest neighbours between clouds for the offline metrics; its own translation unit)
                                            #    vista_slam_amd/libsta_raster.so       a third, handle-free library: exports include/sta_raster.h
                                            #    (the headless z-buffer rasteriser of vista_slam_amd/render.py; its own translation unit)
                                            #    vista_slam_amd/libsta_tsdf.so         a fourth, handle-free library: exports include/sta_tsdf.h
                                            #    (sparse TSDF fusion and marching tetrahedra of vista_slam_amd/tsdf.py; its own translation unit)
                                            #    vista_slam_amd/libsta_mesh.so         a fifth, handle-free library: exports include/sta_mesh.h
                                            #    (triangles for the rasteriser's key buffer and vertex normals; its own translation unit)
                                            #    vista_slam_amd/libsta_surf.so         a sixth, handle-free library: exports include/sta_surf.h
                                            #    (connected components and area-uniform surface samples of a mesh; its own translation unit)
                                            #    vista_slam_amd/libsta_simp.so         a seventh, handle-free library: exports include/sta_simp.h
                                            #    (mesh simplification by vertex clustering with quadrics; its own translation unit)
                                            #    vista_slam_amd/libsta_dist.so         an eighth, handle-free library: exports include/sta_dist.h
                                            #    (exact point-to-triangle distances over an implicit BVH; its own translation unit)
"""
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libsta_mi355.so")
TEST_LIB = os.path.join(PKG, "libsta_mi355_test.so")
SOURCES = ["sta_api.hip"]
DEPS = ["sta_exports.map", "sta_api.hip", "sta_launch.inc", "sta_forward.inc", "sta_debug.inc", "sta_rows.inc", "sta_bench.inc", "gemm.h", "gemm2.h", "conv3h.h", "attention.h", "elementwise.h", "geo.h", "select.h", "voxel.h", "flow.h", "loop.h", "pgo.h", "graph.h", "sta_common.h",
        os.path.join("..", "..", "include", "sta_mi355.h"), os.path.join("..", "..", "include", "sta_mi355_debug.h")]
# libsta_cloud.so: nothing of it is in DEPS, so the product library's source_hash() does not move when it changes
CLOUD_LIB = os.path.join(PKG, "libsta_cloud.so")
CLOUD_SOURCES = ["sta_cloud.hip"]
CLOUD_DEPS = ["sta_exports.map", "sta_cloud.hip", "cloud.h", "voxel.h", "select.h", "elementwise.h", "sta_common.h",
              os.path.join("..", "..", "include", "sta_cloud.h")]
# libsta_raster.so: likewise a library of its own; neither of the hashes above covers it
RASTER_LIB = os.path.join(PKG, "libsta_raster.so")
RASTER_SOURCES = ["sta_raster.hip"]
RASTER_DEPS = ["sta_exports.map", "sta_raster.hip", "raster.h", "sta_common.h", os.path.join("..", "..", "include", "sta_raster.h")]
# libsta_tsdf.so: likewise; it includes voxel.h, select.h and elementwise.h unchanged and none of the hashes above covers its own files
TSDF_LIB = os.path.join(PKG, "libsta_tsdf.so")
TSDF_SOURCES = ["sta_tsdf.hip"]
TSDF_DEPS = ["sta_exports.map", "sta_tsdf.hip", "tsdf.h", "voxel.h", "select.h", "elementwise.h", "sta_common.h",
             os.path.join("..", "..", "include", "sta_tsdf.h")]
# libsta_mesh.so: likewise; it includes raster.h, voxel.h, select.h and elementwise.h unchanged (and include/sta_raster.h for its limits)
MESH_LIB = os.path.join(PKG, "libsta_mesh.so")
MESH_SOURCES = ["sta_mesh.hip"]
MESH_DEPS = ["sta_exports.map", "sta_mesh.hip", "mesh.h", "raster.h", "voxel.h", "select.h", "elementwise.h", "sta_common.h",
             os.path.join("..", "..", "include", "sta_mesh.h"), os.path.join("..", "..", "include", "sta_raster.h")]
# libsta_surf.so: likewise; of the shared kernel headers it includes sta_common.h alone, unchanged
SURF_LIB = os.path.join(PKG, "libsta_surf.so")
SURF_SOURCES = ["sta_surf.hip"]
SURF_DEPS = ["sta_exports.map", "sta_surf.hip", "surf.h", "sta_common.h", os.path.join("..", "..", "include", "sta_surf.h")]
# libsta_simp.so: likewise; it includes voxel.h, select.h, elementwise.h and sta_common.h unchanged
SIMP_LIB = os.path.join(PKG, "libsta_simp.so")
SIMP_SOURCES = ["sta_simp.hip"]
SIMP_DEPS = ["sta_exports.map", "sta_simp.hip", "simp.h", "voxel.h", "select.h", "elementwise.h", "sta_common.h",
             os.path.join("..", "..", "include", "sta_simp.h")]
# libsta_dist.so: likewise; it includes voxel.h, select.h, elementwise.h and sta_common.h unchanged
DIST_LIB = os.path.join(PKG, "libsta_dist.so")
DIST_SOURCES = ["sta_dist.hip"]
DIST_DEPS = ["sta_exports.map", "sta_dist.hip", "dist.h", "voxel.h", "select.h", "elementwise.h", "sta_common.h",
             os.path.join("..", "..", "include", "sta_dist.h")]


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
CLOUD_HASH_FILE = CLOUD_LIB + ".srchash"
RASTER_HASH_FILE = RASTER_LIB + ".srchash"
TSDF_HASH_FILE = TSDF_LIB + ".srchash"
MESH_HASH_FILE = MESH_LIB + ".srchash"
SURF_HASH_FILE = SURF_LIB + ".srchash"
SIMP_HASH_FILE = SIMP_LIB + ".srchash"
DIST_HASH_FILE = DIST_LIB + ".srchash"


def extra_flags():
    """STA_DEV_FAST=1: development build without the precision-f16 kernel forms (half the compile time; the f16 tests fail
    loudly on it).  STA_BENCH_EXPERIMENTS=1: the retired tile shapes / main-loop ablations of tools/gemm_tiles.py."""
    f = []
    if os.environ.get("STA_DEV_FAST") == "1":
        f.append("-DSTA_DEV_FAST")
    if os.environ.get("STA_BENCH_EXPERIMENTS") == "1":
        f.append("-DSTA_BENCH_EXPERIMENTS")
    return f


def source_hash(deps=None):
    """Content hash of every source the library is built from (mtimes do not survive the gpurun
    snapshot copy, so staleness is decided by content) and of the build flags.  deps: DEPS (the product and test-hooks
    libraries) unless given (CLOUD_DEPS, RASTER_DEPS, TSDF_DEPS, MESH_DEPS, SURF_DEPS, SIMP_DEPS, DIST_DEPS)."""
    import hashlib
    h = hashlib.sha256()
    h.update(" ".join([f.replace(CSRC, "csrc") for f in BASE_FLAGS] + extra_flags()).encode())      # (path-independent: the snapshot on the GPU box lives elsewhere)
    for d in (DEPS if deps is None else deps):
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def is_stale(lib=LIB, hash_file=HASH_FILE, deps=None):
    if not os.path.exists(lib) or not os.path.exists(hash_file):
        return True
    with open(hash_file) as f:
        return f.read().strip() != source_hash(deps)


def _cmd(hipcc, out, hooks, sources=None):
    return ([hipcc] + BASE_FLAGS + ["-o", out] + extra_flags() +
            (["-DSTA_TEST_HOOKS"] if hooks else []) + [os.path.join(CSRC, s) for s in (SOURCES if sources is None else sources)])


def build_lib(force=False, verbose=True, test_hooks=True, cloud=True, raster=True, tsdf=True, mesh=True, surf=True, simp=True, dist=True):
    """Build the product library, (test_hooks) the test-hooks library, (cloud) libsta_cloud.so, (raster) libsta_raster.so, (tsdf)
    libsta_tsdf.so, (mesh) libsta_mesh.so, (surf) libsta_surf.so, (simp) libsta_simp.so and (dist) libsta_dist.so; all compile concurrently (one hipcc process each, ~100 s).  Returns the product library's path."""
    jobs = []           # (output, hash file, test hooks, sources, deps)
    if force or is_stale(LIB, HASH_FILE):
        jobs.append((LIB, HASH_FILE, False, None, None))
    if test_hooks and (force or is_stale(TEST_LIB, TEST_HASH_FILE)):
        jobs.append((TEST_LIB, TEST_HASH_FILE, True, None, None))
    if cloud and (force or is_stale(CLOUD_LIB, CLOUD_HASH_FILE, CLOUD_DEPS)):
        jobs.append((CLOUD_LIB, CLOUD_HASH_FILE, False, CLOUD_SOURCES, CLOUD_DEPS))
    if raster and (force or is_stale(RASTER_LIB, RASTER_HASH_FILE, RASTER_DEPS)):
        jobs.append((RASTER_LIB, RASTER_HASH_FILE, False, RASTER_SOURCES, RASTER_DEPS))
    if tsdf and (force or is_stale(TSDF_LIB, TSDF_HASH_FILE, TSDF_DEPS)):
        jobs.append((TSDF_LIB, TSDF_HASH_FILE, False, TSDF_SOURCES, TSDF_DEPS))
    if mesh and (force or is_stale(MESH_LIB, MESH_HASH_FILE, MESH_DEPS)):
        jobs.append((MESH_LIB, MESH_HASH_FILE, False, MESH_SOURCES, MESH_DEPS))
    if surf and (force or is_stale(SURF_LIB, SURF_HASH_FILE, SURF_DEPS)):
        jobs.append((SURF_LIB, SURF_HASH_FILE, False, SURF_SOURCES, SURF_DEPS))
    if simp and (force or is_stale(SIMP_LIB, SIMP_HASH_FILE, SIMP_DEPS)):
        jobs.append((SIMP_LIB, SIMP_HASH_FILE, False, SIMP_SOURCES, SIMP_DEPS))
    if dist and (force or is_stale(DIST_LIB, DIST_HASH_FILE, DIST_DEPS)):
        jobs.append((DIST_LIB, DIST_HASH_FILE, False, DIST_SOURCES, DIST_DEPS))
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
    for (p, cmd), (out, hf, _hooks, _sources, deps) in zip(procs, jobs):
        if failed is not None:             # a sibling compile already failed: do not leave this one running un-waited
            p.kill()
            p.wait()
            continue
        if p.wait() != 0:
            failed = subprocess.CalledProcessError(p.returncode, cmd)
            continue
        with open(hf, "w") as f:
            f.write(source_hash(deps))
    if failed is not None:
        raise failed
    return LIB


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)
    print(LIB)
