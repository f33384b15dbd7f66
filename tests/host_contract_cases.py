"""The host contract of the seven handle-free libraries: the calls whose answer is decided before the first HIP call - plan sizes, and
the return code and error text of null arguments, range checks and buffers one byte short.  tools/capture_host_contract.py records the
answers of one build into tests/golden/host_contract.json; tests/test_host_contract.py replays the file against the build under test.

A call is (library, function, arguments).  An argument is a number or one of
    "null"             NULL
    "ptr"              a non-null address that nothing may dereference: these calls return before they would
    "out"              int64[16] on the host, reported back as the call's `sizes` (a plan's sizes_out, a call's counts_out_host)
    "buf"              256 bytes on the host for a struct the call may fill
    {"f64": [...]}     a host array of doubles
    {"nn_index": M}    an sta_nn_index of M points in no cell, its pointers non-null"""
import ctypes as C

LIBRARIES = ("cloud", "raster", "tsdf", "mesh", "surf", "simp", "dist")
LAST_ERROR = {"cloud": "sta_cloud_last_error", "raster": "sta_raster_last_error", "tsdf": "sta_tsdf_last_error", "mesh": "sta_mesh_last_error",
              "surf": "sta_surf_last_error", "simp": "sta_simp_last_error", "dist": "sta_tri_last_error"}
# the boundaries of the 256-thread block and of VOX_TILE = 1024
COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 4097)
FAKE = 0x7F0000100000
SMALL = 5          # the value of a count-like argument while another one varies

T_HOST = {"f64": [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]}
K_HOST = {"f64": [50.0, 50.0, 16.0, 16.0]}


def signatures(_lib, name):
    return getattr(_lib, name.upper() + "_SIGNATURES")


def call(_lib, lib, name, fn, args):
    """One call -> {"rc", "error", "sizes"}: error is the library's last error if rc != 0, sizes the "out" array up to its last entry
    that the call wrote."""
    res, argtypes = signatures(_lib, name)[fn]
    assert res is C.c_int and len(argtypes) == len(args), (fn, len(argtypes), len(args))
    keep, cargs, out = [], [], None
    for a, t in zip(args, argtypes):
        if a == "null":
            v = None
        elif a == "ptr":
            assert t is C.c_void_p, (fn, a, t)
            v = FAKE
        elif a == "out":
            out = (C.c_int64 * 16)(*([-7777] * 16))
            v = C.cast(out, t) if t is not C.c_void_p else C.addressof(out)
        elif a == "buf":
            keep.append(C.create_string_buffer(256))
            v = C.cast(keep[-1], t) if t is not C.c_void_p else C.addressof(keep[-1])
        elif isinstance(a, dict) and "f64" in a:
            keep.append((C.c_double * len(a["f64"]))(*a["f64"]))
            v = C.cast(keep[-1], t)
        elif isinstance(a, dict) and "nn_index" in a:
            ix = _lib.StaNNIndex(cell_key=FAKE, cell_start=FAKE, sorted_pts=FAKE, sorted_idx=FAKE, cell=1.0, M=a["nn_index"], n_finite=a["nn_index"], C=0)
            keep.append(ix)
            v = C.byref(ix)
        else:
            assert isinstance(a, (int, float)) and not isinstance(a, bool), (fn, a)
            v = a
        cargs.append(v)
    rc = getattr(lib, fn)(*cargs)
    sizes = None
    if out is not None:
        sizes = list(out)
        while sizes and sizes[-1] == -7777:
            sizes.pop()
    return {"rc": rc, "error": getattr(lib, LAST_ERROR[name])().decode() if rc != 0 else None, "sizes": sizes}


# ---------------------------------------------------------------------------------------------------------
# Every entry point with arguments that pass its checks for the counts n (the primary count) and m (the other one); `work` / `index`:
# the position of the byte count of the workspace / index buffer and the entry of the plan's sizes that it needs.
def _entries(n, m, sizes):
    """sizes: name -> the plan's sizes for these counts"""
    def need(name, k):
        return sizes[name][k]
    hw = (4, 8)
    grid = (0.01, 0.03)         # voxel_size, trunc
    return {
        "cloud": {
            "sta_nn_build": (["ptr", n, 0.5, "ptr", need("cloud", 0), "ptr", need("cloud", 1), "buf", "null"], {"index": (4, 0), "work": (6, 1)}),
            "sta_nn_query": ([{"nn_index": n}, "ptr", m, "null", 0.25, "ptr", "ptr", "ptr", "ptr", need("cloud", 2), "null"], {"work": (9, 2)}),
            "sta_cloud_transform": (["ptr", n, "null", "ptr", "null"], {}),
        },
        "raster": {
            "sta_raster_clear": (["ptr", 4, 8, 2, "null"], {}),
            "sta_raster_points": (["ptr", 4, 8, 2, "ptr", "null", 0, 0, n, T_HOST, K_HOST, 0.1, 10.0, 1, "null", "null"], {}),
            "sta_raster_lines": (["ptr", 4, 8, 2, "ptr", "ptr", n, T_HOST, K_HOST, 0.1, 10.0, 1, "null"], {}),
            "sta_raster_resolve": (["ptr", 4, 8, 2, "null", "null", "ptr", "null", "null"], {}),
        },
        "tsdf": {
            "sta_tsdf_table": (["buf"], {}),
            "sta_tsdf_blocks": (["ptr"] * 5 + [n, *hw, *grid, "null", 5.0, "ptr", m, "ptr", need("tsdf", 0), "out", "null"], {"work": (15, 0)}),
            "sta_tsdf_clear": (["ptr", "ptr", "null", n, "null"], {}),
            "sta_tsdf_integrate": (["ptr", m] + ["ptr"] * 3 + ["ptr"] * 5 + ["null", n, *hw, 0, n, *grid, "null", 5.0, 64.0, "null"], {}),
            "sta_tsdf_mesh": (["ptr", m, "ptr", "ptr", "null", 0.01, "null", 1.0, "ptr", "null", "ptr", SMALL, SMALL, "ptr", need("tsdf", 4), "out", "null"],
                              {"work": (14, 4)}),
        },
        "mesh": {
            "sta_mesh_triangles": (["ptr", 4, 8, 2, "ptr", m, "ptr", n, "null", "null", "null", 0, 0, 0, T_HOST, K_HOST, 0.1, 10.0, "null", "ptr",
                                    need("mesh", 0), "null"], {"work": (20, 0)}),
            "sta_mesh_vertex_normals": (["ptr", m, "ptr", n, "ptr", "ptr", need("mesh", 1), "null"], {"work": (6, 1)}),
        },
        "surf": {
            "sta_surf_components": (["ptr", n, m, "ptr", "ptr", "ptr", "ptr", "ptr", need("surf", 0), "null"], {"work": (8, 0)}),
            "sta_surf_weights": (["ptr", m, "ptr", n, "null", "ptr", "ptr", "ptr", need("surf", 1), "null"], {"work": (8, 1)}),
            "sta_surf_sample": (["ptr", m, "ptr", n, "ptr", "ptr", "null", SMALL, 7, "ptr", "ptr", "null", "null", "null"], {}),
        },
        "simp": {
            "sta_simp_cells": (["ptr", m, 0.5, 0.0, 0.0, 0.0, "ptr", "ptr", "ptr", need("simp", 0), "null"], {"work": (9, 0)}),
            "sta_simp_triangles": (["ptr", n, m] + ["ptr"] * 7 + [need("simp", 1), "null"], {"work": (10, 1)}),
            "sta_simp_place": (["ptr", "null", m, "ptr", n, "ptr", "ptr", 0.5, 0.0, 0.0, 0.0, 0, 0.0, "ptr", "null", "ptr", "ptr", need("simp", 2), "null"],
                               {"work": (17, 2)}),
        },
        "dist": {
            "sta_tri_build": (["ptr", SMALL, "ptr", n, "ptr", need("dist", 0), "ptr", need("dist", 1), "buf", "ptr", "null"], {"index": (5, 0), "work": (7, 1)}),
            "sta_tri_query": (["buf", "ptr", m, 1.0, "ptr", "ptr", "ptr", "null"], {}),
        },
    }


def _plan_args(n, m):
    """the plan call that goes with _entries(n, m): tsdf plans n views and m blocks, surf n triangles, m vertices and SMALL samples"""
    return {"cloud": ("sta_nn_plan", [n, m, "out"]), "tsdf": ("sta_tsdf_plan", [n, 4, 8, 0.01, 0.03, m, SMALL, SMALL, "out"]),
            "mesh": ("sta_mesh_plan", [n, m, "out"]), "surf": ("sta_surf_plan", [n, m, SMALL, "out"]), "simp": ("sta_simp_plan", [n, m, "out"]),
            "dist": ("sta_tri_plan", [n, m, "out"])}


# plan function -> (arguments that pass, the positions of its count-like arguments)
PLANS = {
    "cloud": ("sta_nn_plan", [SMALL, SMALL, "out"], (0, 1)),
    "raster": ("sta_raster_plan", [4, 8, 1, "out"], ()),
    "tsdf": ("sta_tsdf_plan", [2, 4, 8, 0.01, 0.03, SMALL, SMALL, SMALL, "out"], (0, 5, 6, 7)),
    "mesh": ("sta_mesh_plan", [SMALL, SMALL, "out"], (0, 1)),
    "surf": ("sta_surf_plan", [SMALL, SMALL, SMALL, "out"], (0, 1, 2)),
    "simp": ("sta_simp_plan", [SMALL, SMALL, "out"], (0, 1)),
    "dist": ("sta_tri_plan", [SMALL, SMALL, "out"], (0, 1)),
}
CANVASES = ((1, 1, 1), (4, 8, 2), (480, 640, 1), (33, 17, 4), (2048, 2048, 4), (8192, 8192, 1))           # H, W, ssaa
VIEWS = ((1, 1, 1), (2, 4, 8), (3, 33, 17), (1, 480, 640), (16, 224, 224))                               # V, H, W
# the range checks that the plan functions reach: (position, value)
RANGES = {
    "cloud": ((0, 0), (0, 1 << 30), (1, 0), (1, 1 << 30)),
    "raster": ((0, 0), (1, 0), (2, 3), (0, 8193), (1, 8193)),
    "tsdf": ((3, 0.0), (4, 0.0), (4, 0.05), (1, 0), (0, 0), (0, 1 << 28), (5, 0), (5, 1 << 24), (6, -1), (7, 1 << 31)),
    "mesh": ((0, -1), (0, 1 << 31), (1, -1), (1, 1 << 31)),
    "surf": ((0, -1), (0, 1 << 31), (1, -1), (1, 1 << 31), (2, -1), (2, 1 << 31)),
    "simp": ((1, -1), (1, 1 << 31), (0, -1), (0, 715827883)),
    "dist": ((0, 0), (0, 1 << 27), (1, 0), (1, 1 << 30)),
}
# the argument whose absence every other entry point reports, where it is not the first pointer
NULL_AT = {"sta_nn_query": 1, "sta_raster_points": 9, "sta_raster_lines": 7, "sta_tsdf_mesh": 15, "sta_mesh_triangles": 14, "sta_surf_components": 6,
           "sta_surf_weights": 6, "sta_surf_sample": 5, "sta_simp_cells": 7, "sta_simp_triangles": 8, "sta_simp_place": 15}


def _with(args, pos, value):
    return args[:pos] + [value] + args[pos + 1:]


def cases(plan):
    """Every call of the contract as (name, kind, fn, args).  plan(name, fn, args) -> the sizes of a plan call that succeeds: the byte
    counts of the short-buffer calls come from it."""
    out = []
    for name in LIBRARIES:
        fn, good, counts = PLANS[name]
        for pos in counts:
            for n in COUNTS:
                out.append((name, "plan", fn, _with(good, pos, n)))
        for pos, v in RANGES[name]:
            out.append((name, "range", fn, _with(good, pos, v)))
        out.append((name, "null", fn, _with(good, len(good) - 1, "null")))
    for h, w, s in CANVASES:
        out.append(("raster", "plan", "sta_raster_plan", [h, w, s, "out"]))
    for v, h, w in VIEWS:
        out.append(("tsdf", "plan", "sta_tsdf_plan", [v, h, w, 0.01, 0.03, SMALL, SMALL, SMALL, "out"]))
    # a null argument: with buffers of the planned size, so that the null check is the one that fails
    sizes = {name: plan(name, *args) for name, args in _plan_args(SMALL, SMALL).items()}
    for name, entries in _entries(SMALL, SMALL, sizes).items():
        for fn, (args, _short) in entries.items():
            pos = NULL_AT.get(fn, next(i for i, a in enumerate(args) if a in ("ptr", "buf")))
            out.append((name, "null", fn, _with(args, pos, "null")))
    # one byte short
    for n in COUNTS:
        for primary in (True, False):
            cn, cm = (n, SMALL) if primary else (SMALL, n)
            sizes = {name: plan(name, *args) for name, args in _plan_args(cn, cm).items()}
            for name, entries in _entries(cn, cm, sizes).items():
                for fn, (args, short) in entries.items():
                    for kind, (pos, _k) in short.items():
                        out.append((name, kind + "_short", fn, _with(args, pos, args[pos] - 1)))
    seen, unique = set(), []
    for c in out:
        if repr(c) not in seen:
            seen.add(repr(c))
            unique.append(c)
    return unique
