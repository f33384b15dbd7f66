"""The stream-order rows of libsta_mesh.so and of the Python layer on it, in the shape of tests/stream_cases.py (its Row, its harness):
every call is ordered by its stream alone, also behind pending work.  tests/test_mesh_abi.py holds the entry points named here against the
declarations of include/sta_mesh.h that take a `void* stream`, in both directions; tests/test_mesh_stream_gpu.py runs the rows.  The
poison of a floating-point input is NaN (a vertex whose camera coordinate is not finite: the triangle is dropped; a normal sum that is not
finite: zero), of the indices 0 (every triangle names vertex 0 three times: degenerate): values the kernels take as data, never as a fault.

SYNCS is empty: no call of this library may wait for its stream."""
from stream_cases import Row, _up

SYNCS = {}
EXEMPT = {}
OTHER_LIBRARIES = {"sta_raster_clear", "sta_raster_resolve"}      # the canvas around the triangle pass: rows of tests/render_stream_cases.py too
H, W, SSAA = 24, 32, 2


def _mesh(seed):
    import numpy as np
    import mesh_cases as MC
    v, t, col = MC.sphere_mesh()
    r = np.random.default_rng(seed)
    return (v + r.uniform(-0.05, 0.05, v.shape).astype(np.float32)), t.copy(), col.copy()


def _mk_triangles(seed):
    def make(m):
        from vista_slam_amd import render
        v, t, col = _mesh(seed)
        return {"verts": _up(v), "tris": _up(t), "colors": _up(col), "_cv": render.Canvas("cuda:0", H, W, SSAA)}
    return make


def _camera():
    import numpy as np
    import mesh_cases as MC
    from vista_slam_amd import render
    c = MC.inside_cam(0.05, H, W)
    return render.Camera(np.asarray(c["K"]), c["T"], c["near"], c["far"])


def _run_triangles(m, x, between=None):
    cv = x["_cv"]
    cam = _camera()
    cv.clear().mesh(cam, x["verts"], x["tris"], x["colors"], mode="shaded")
    out = [("keys", cv.keys.clone()), ("image", cv.image()), ("counters", cv._mesh_counters.clone())]
    cv.clear().mesh(cam, x["verts"], x["tris"], mode="id", cull="front")
    return out + [("ids", cv.ids()), ("depth", cv.depth())]


def _mk_normals(seed):
    def make(m):
        v, t, _ = _mesh(seed)
        return {"verts": _up(v), "tris": _up(t)}
    return make


def _run_normals(m, x, between=None):
    from vista_slam_amd import tsdf
    return [("normals", tsdf.vertex_normals(tsdf.Mesh(x["verts"], None, x["tris"])))]


def _seeded(name, entries, mk, run, shapes, layer=()):
    return Row(name, entries, mk(0), run, shapes, (), mk(1), layer)


ROWS = [
    _seeded("mesh_triangles", ("sta_mesh_triangles", "sta_raster_clear", "sta_raster_resolve"), _mk_triangles, _run_triangles,
            "Canvas.clear + mesh (shaded, then ids with cull) + image / ids / depth: the sphere of 2124 triangles from inside, 24x32 at ssaa 2, both paths",
            layer=("render.Canvas.mesh",)),
    _seeded("mesh_vertex_normals", ("sta_mesh_vertex_normals",), _mk_normals, _run_normals, "tsdf.vertex_normals of the sphere: 1064 vertices, 6372 pairs, 2 sort passes",
            layer=("tsdf.vertex_normals",)),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
