"""The stream-order rows of libsta_dist.so and of the Python layer on it, in the shape of tests/stream_cases.py (its Row, its harness):
every call is ordered by its stream alone, also behind pending work.  tests/test_dist_abi.py holds the entry points named here against the
declarations of include/sta_dist.h that take a `void* stream`, in both directions; tests/test_dist_stream_gpu.py runs the rows.  The
poison of a floating-point input is NaN (every triangle is non-finite and no query is finite: every answer is unmatched), of the indices 0
(every triangle names vertex 0 three times: none has area): values the kernels take as data, never as a fault.

SYNCS is empty: no call of this library may wait for its stream."""
from stream_cases import Row, _up

SYNCS = {}
EXEMPT = {}
OTHER_LIBRARIES = set()
RADIUS = 0.75


def _mk(seed):
    def make(m):
        import numpy as np
        import surf_cases as SF
        v, t = SF.three_spheres(seed + 5)
        r = np.random.default_rng(seed)
        q = (v[r.integers(0, len(v), 3000)] + r.standard_normal((3000, 3)) * 0.5).astype(np.float32)
        return {"verts": _up(v + r.uniform(-0.05, 0.05, v.shape).astype(np.float32)), "tris": _up(t), "qry": _up(q)}
    return make


def _of(x):
    from vista_slam_amd import tsdf
    return tsdf.Mesh(x["verts"], None, x["tris"])


def _run_build(m, x, between=None):
    from vista_slam_amd import meshdist
    idx = meshdist.TriIndex.build(_of(x))
    return [("tri", idx.tri), ("src", idx.src), ("boxes", idx.boxes), ("counters", idx.counters)]


def _run_query(m, x, between=None):
    from vista_slam_amd import meshdist
    idx = meshdist.TriIndex.build(_of(x))
    near = idx.query(x["qry"], RADIUS)
    far = idx.query(x["qry"])
    return [("d2", near[0]), ("tri", near[1]), ("point", near[2]), ("d2 inf", far[0]), ("tri inf", far[1]), ("point inf", far[2]),
            ("counters", idx.counters)]


def _seeded(name, entries, run, shapes, layer=()):
    return Row(name, entries, _mk(0), run, shapes, (), _mk(1), layer)


ROWS = [
    _seeded("tri_build", ("sta_tri_build",), _run_build, "meshdist.TriIndex.build of three spheres: 3192 vertices, 6372 triangles",
            layer=("meshdist.TriIndex.build",)),
    _seeded("tri_query", ("sta_tri_query", "sta_tri_build"), _run_query, "TriIndex.query of 3000 points at radius 0.75 and +inf on the index of the same call",
            layer=("meshdist.TriIndex.query",)),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
