"""The stream-order rows of libsta_simp.so and of the Python layer on it, in the shape of tests/stream_cases.py (its Row, its harness):
every call is ordered by its stream alone, also behind pending work.  tests/test_simp_abi.py holds the entry points named here against the
declarations of include/sta_simp.h that take a `void* stream`, in both directions; tests/test_simp_stream_gpu.py runs the rows.  The
poison of a floating-point input is NaN (every vertex is dropped: no cell, every triangle invalid), of the indices 0 (every triangle names
vertex 0 three times: all collapse): values the kernels take as data, never as a fault.

SYNCS is empty: no call of this library may wait for its stream.  (`simplify.simplify_mesh` reads the counters and is not a row.)"""
from stream_cases import Row, _up

SYNCS = {}
EXEMPT = {}
OTHER_LIBRARIES = set()
CELL = 0.5


def _mk(seed):
    def make(m):
        import numpy as np
        import surf_cases as SF
        v, t = SF.three_spheres(seed + 5)
        r = np.random.default_rng(seed)
        return {"verts": _up(v + r.uniform(-0.05, 0.05, v.shape).astype(np.float32)), "tris": _up(t), "colors": _up(r.random(v.shape).astype(np.float32))}
    return make


def _of(x):
    from vista_slam_amd import tsdf
    return tsdf.Mesh(x["verts"], x["colors"], x["tris"])


def _run_cells(m, x, between=None):
    from vista_slam_amd import simplify
    return list(zip(("vcell", "counters"), simplify.cells(_of(x), CELL, (0.1, 0.2, 0.3))))


def _run_triangles(m, x, between=None):
    from vista_slam_amd import simplify
    return list(zip(simplify.Clusters._fields, simplify.cluster_triangles(_of(x), CELL)))


def _run_place(m, x, between=None):
    from vista_slam_amd import simplify
    cl = simplify.cluster_triangles(_of(x), CELL)
    qv, qc = simplify.place_vertices(_of(x), cl, CELL, placement="quadric")
    mv, mc = simplify.place_vertices(_of(x), cl, CELL, placement="mean")
    return [("quadric", qv), ("quadric colors", qc), ("mean", mv), ("mean colors", mc), ("counters", cl.counters)]


def _seeded(name, entries, run, shapes, layer=()):
    return Row(name, entries, _mk(0), run, shapes, (), _mk(1), layer)


ROWS = [
    _seeded("simp_cells", ("sta_simp_cells",), _run_cells, "simplify.cells of three spheres at a shifted origin: 3192 vertices", layer=("simplify.cells",)),
    _seeded("simp_triangles", ("sta_simp_triangles", "sta_simp_cells"), _run_triangles, "simplify.cluster_triangles: 3192 vertices, 6372 triangles",
            layer=("simplify.cluster_triangles",)),
    _seeded("simp_place", ("sta_simp_place", "sta_simp_triangles", "sta_simp_cells"), _run_place,
            "simplify.place_vertices, quadric and mean, with colours, on the clusters of the same call", layer=("simplify.place_vertices",)),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
