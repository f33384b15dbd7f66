"""The stream-order rows of libsta_surf.so and of the Python layer on it, in the shape of tests/stream_cases.py (its Row, its harness):
every call is ordered by its stream alone, also behind pending work.  tests/test_surf_abi.py holds the entry points named here against the
declarations of include/sta_surf.h that take a `void* stream`, in both directions; tests/test_surf_stream_gpu.py runs the rows.  The
poison of a floating-point input is NaN (a weight that is not finite counts as 0, a total of 0 gives triangles of -1 and NaN points), of
the indices 0 (every triangle names vertex 0 three times: one component of one vertex, no area), of the keep mask 255: values the
kernels take as data, never as a fault.

SYNCS is empty: no call of this library may wait for its stream.  (`surface.clean_mesh` reads the status word and is not a row.)"""
from stream_cases import Row, _up

SYNCS = {}
EXEMPT = {}
OTHER_LIBRARIES = set()


def _mesh(seed):
    import numpy as np
    import surf_cases as SF
    v, t = SF.three_spheres(seed + 5)
    r = np.random.default_rng(seed)
    col = r.random(v.shape).astype(np.float32)
    return (v + r.uniform(-0.05, 0.05, v.shape).astype(np.float32)), t, col


def _mk(seed):
    def make(m):
        import numpy as np
        v, t, col = _mesh(seed)
        keep = (np.random.default_rng(seed + 1).random(len(t)) < 0.7).astype(np.uint8)
        return {"verts": _up(v), "tris": _up(t), "colors": _up(col), "keep": _up(keep)}
    return make


def _of(x):
    from vista_slam_amd import tsdf
    return tsdf.Mesh(x["verts"], x["colors"], x["tris"])


def _run_components(m, x, between=None):
    from vista_slam_amd import surface
    return list(zip(("vlabel", "tlabel", "tcount", "status"), surface.components(_of(x), return_status=True)))


def _run_weights(m, x, between=None):
    from vista_slam_amd import surface
    P, total = surface.weights(_of(x), x["keep"])
    return [("P", P), ("total", total), ("area", surface.area(_of(x)).reshape(1))]


def _run_sample(m, x, between=None):
    from vista_slam_amd import surface
    s = surface.sample_surface(_of(x), 5000, seed=9, tri_keep=x["keep"], colors=True, normals=True)
    return [("points", s.points), ("tri", s.triangles), ("colors", s.colors), ("normals", s.normals)]


def _seeded(name, entries, run, shapes, layer=()):
    return Row(name, entries, _mk(0), run, shapes, (), _mk(1), layer)


ROWS = [
    _seeded("surf_components", ("sta_surf_components",), _run_components, "surface.components of three spheres under a permutation: 3192 vertices, 6372 triangles",
            layer=("surface.components",)),
    _seeded("surf_weights", ("sta_surf_weights",), _run_weights, "surface.weights with a keep mask, and surface.area: 6372 triangles, 7 chunks",
            layer=("surface.weights", "surface.area")),
    _seeded("surf_sample", ("sta_surf_sample", "sta_surf_weights"), _run_sample, "surface.sample_surface: 5000 samples with colours and normals, a keep mask",
            layer=("surface.sample_surface",)),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
