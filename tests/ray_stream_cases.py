"""The stream-order rows of libsta_ray.so and of the Python layer on it, in the shape of tests/dist_stream_cases.py (the Row and the
harness of tests/stream_cases.py): every call is ordered by its stream alone, also behind pending work.  tests/test_ray_abi.py holds the
entry points named here against the declarations of include/sta_ray.h that take a `void* stream`, in both directions;
tests/test_ray_stream_gpu.py runs the rows.  The poison of a floating-point input is NaN (every triangle is non-finite and no ray is
usable: every answer is unmatched), of the indices 0 (every triangle names vertex 0 three times: none has area): values the kernels take
as data, never as a fault.

SYNCS is empty: no call of this library may wait for its stream."""
from stream_cases import Row, _up

SYNCS = {}
EXEMPT = {}
OTHER_LIBRARIES = {"sta_tri_build"}          # the index is built in the same call, by libsta_dist.so
T_NEAR = (0.25, 1.0)


def _mk(seed):
    def make(m):
        import numpy as np
        import surf_cases as SF
        v, t = SF.three_spheres(seed + 5)
        r = np.random.default_rng(seed)
        v = v + r.uniform(-0.05, 0.05, v.shape).astype(np.float32)
        o = (v[r.integers(0, len(v), 3000)] + r.standard_normal((3000, 3)) * 2.0).astype(np.float32)
        d = (v[r.integers(0, len(v), 3000)] - o).astype(np.float32)
        return {"verts": _up(v), "tris": _up(t), "org": _up(o), "dir": _up(d)}
    return make


def _of(x):
    from vista_slam_amd import tsdf
    return tsdf.Mesh(x["verts"], None, x["tris"])


def _run_cast(m, x, between=None):
    from vista_slam_amd import meshdist
    idx = meshdist.TriIndex.build(_of(x))
    far = idx.cast(x["org"], x["dir"])
    near = idx.cast(x["org"], x["dir"], *T_NEAR)
    return [("t", far[0]), ("tri", far[1]), ("bary", far[2]), ("t near", near[0]), ("tri near", near[1]), ("bary near", near[2]), ("status", idx.ray_status)]


def _run_occluded(m, x, between=None):
    from vista_slam_amd import meshdist
    idx = meshdist.TriIndex.build(_of(x))
    return [("occluded", idx.occluded(x["org"], x["dir"])), ("occluded near", idx.occluded(x["org"], x["dir"], *T_NEAR)),
            ("visible", meshdist.visible(idx, x["org"], x["verts"][:3000])), ("status", idx.ray_status)]


def _seeded(name, entries, run, shapes, layer=()):
    return Row(name, entries, _mk(0), run, shapes, (), _mk(1), layer)


ROWS = [
    _seeded("ray_cast", ("sta_ray_cast", "sta_tri_build"), _run_cast, "TriIndex.cast of 3000 rays in [0, inf) and in [0.25, 1] on the index of three spheres "
            "(6372 triangles) built in the same call", layer=("meshdist.TriIndex.cast",)),
    _seeded("ray_occluded", ("sta_ray_occluded", "sta_tri_build"), _run_occluded, "TriIndex.occluded of the same rays and ranges and meshdist.visible of 3000 "
            "segments, on the index of the same call", layer=("meshdist.TriIndex.occluded", "meshdist.visible")),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
