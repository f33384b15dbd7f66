"""The stream-order rows of libsta_knn.so and of the Python layer on it, in the shape of tests/reg_stream_cases.py (the Row and the
harness of tests/stream_cases.py): every call is ordered by its stream alone, also behind pending work.  tests/test_knn_abi.py holds the
entry points named here against the declarations of include/sta_knn.h that take a `void* stream`, in both directions;
tests/test_knn_stream_gpu.py runs the rows.  The poison of a floating-point input is NaN (no query is finite: every list is empty, every
moment NaN or +inf): values the kernels take as data, never as a fault.  The index is the row's own (built before the row runs, by
libsta_cloud.so, whose build waits for its stream by contract) and is not poisoned.

SYNCS is empty: no call of this library may wait for its stream.  (The filters of vista_slam_amd/cloud.py read a record back and the
wrappers build an index: they wait by design, are loops of the host layer over these two entry points, and have no row.)"""
from stream_cases import Row, _up

SYNCS = {}
EXEMPT = {}
OTHER_LIBRARIES = set()
RADIUS, CELL, K = 0.6, 0.3, 16


def _mk(seed):
    def make(m):
        import numpy as np
        import cloud_cases as CC
        from vista_slam_amd import cloud
        ref = CC.box_room(1500, 60 + seed)
        r = np.random.default_rng(seed)
        qry = (ref[r.permutation(1500)[:700]] + r.normal(0.0, 0.05, (700, 3))).astype(np.float32)
        view = (qry + r.normal(0.0, 1.0, (700, 3))).astype(np.float32)
        return {"qry": _up(qry), "view": _up(view), "ref": _up(ref), "_index": cloud.NNIndex.build(_up(ref), CELL)}
    return make


def _run(m, x, between=None):
    from vista_slam_amd import cloud
    index = x["_index"]
    lists = index.knn(x["qry"], K, RADIUS)
    mo = cloud.knn_moments(x["ref"], lists, x["qry"], x["view"])
    return [(k, lists[k]) for k in ("d2", "idx", "count")] + [(k, mo[k]) for k in ("normal", "curv", "mean_dist", "record")] + [("status", index.knn_status)]


ROWS = [
    Row("knn_query_and_moments", ("sta_knn_query", "sta_knn_moments"), _mk(0), _run, "NNIndex.knn of 700 queries at k = 16 on a prebuilt index of 1500 points, "
        "then cloud.knn_moments with each point's own viewpoint, every output", (), _mk(1), ("cloud.NNIndex.knn", "cloud.knn_moments")),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
