"""The stream-order rows of libsta_reg.so and of the Python layer on it, in the shape of tests/ray_stream_cases.py (the Row and the
harness of tests/stream_cases.py): every call is ordered by its stream alone, also behind pending work.  tests/test_reg_abi.py holds the
entry points named here against the declarations of include/sta_reg.h that take a `void* stream`, in both directions;
tests/test_reg_stream_gpu.py runs the rows.  The poison of a floating-point input is NaN (every triangle is non-finite and no query is
finite: every answer is unmatched), of the indices 0 (every triangle names vertex 0 three times: none has area): values the kernels take
as data, never as a fault.

SYNCS is empty: no call of this library may wait for its stream.  (meshdist.icp reads a record back per evaluation and so waits by
design: it is a loop on the host, not an entry point, and has no row.)"""
from stream_cases import Row, _up

SYNCS = {}
EXEMPT = {}
OTHER_LIBRARIES = {"sta_tri_build"}          # the index is built in the same call, by libsta_dist.so
RADIUS = 0.5


def _mk(seed):
    def make(m):
        import numpy as np
        import reg_cases as RG
        import surf_cases as SF
        v, t = SF.three_spheres(seed + 5)
        r = np.random.default_rng(seed)
        v = v + r.uniform(-0.05, 0.05, v.shape).astype(np.float32)
        pick = r.integers(0, len(t), 3000)
        q = (v[t[pick, 0]] + r.standard_normal((3000, 3)) * 0.2).astype(np.float32)
        n = RG.face_normals(v, t, pick) * np.where(r.random(3000) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
        return {"verts": _up(v), "tris": _up(t), "qry": _up(q), "nrm": _up(n)}
    return make


def _of(x):
    from vista_slam_amd import tsdf
    return tsdf.Mesh(x["verts"], None, x["tris"])


def _run_pass(m, x, between=None):
    import reg_cases as RG
    from vista_slam_amd import meshdist
    idx = meshdist.TriIndex.build(_of(x))
    T = RG.TRANSFORMS["rotation"]()
    want = ("record", "d2", "tri", "point", "resid")
    plain = idx.register_pass(x["qry"], T, RADIUS, pivot=(20.0, 20.0, 20.0), want=want)
    checked = idx.register_pass(x["qry"], None, RADIUS, x["nrm"], 0.0, want=want)
    return [(w, a) for w, a in zip(want, plain)] + [(w + " with normals", a) for w, a in zip(want, checked)] + [("status", idx.reg_status)]


ROWS = [
    Row("reg_pass", ("sta_reg_pass", "sta_tri_build"), _mk(0), _run_pass, "TriIndex.register_pass of 3000 points under a rotation about a pivot and, with "
        "normals and min_cos 0, under the identity, every output, on the index of three spheres (6372 triangles) built in the same call", (), _mk(1),
        ("meshdist.TriIndex.register_pass",)),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
