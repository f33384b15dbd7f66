"""The stream-order rows of libsta_cloud.so and vista_slam_amd.cloud, in the shape of tests/stream_cases.py (its Row, its harness):
every call is ordered by its stream alone, also behind pending work.  tests/test_cloud_abi.py holds the entry points named here
against the declarations of include/sta_cloud.h that take a `void* stream`, in both directions; tests/test_cloud_stream_gpu.py runs
the rows.  The poison of a floating-point input is NaN: the kernels must take it as data (a dropped reference point, an unmatched
query), never as a fault."""
from stream_cases import Row, _up

# Entry points and callables that are documented to wait for their stream: the sentence that says so.
SYNCS = {
    "sta_nn_build": "include/sta_cloud.h, sta_nn_build: 'The call SYNCHRONISES `stream` once, at its end, for the extent check and C: index_out_host "
                    "is complete on return.'",
    "cloud.icp": "vista_slam_amd/cloud.py, icp: 'Each evaluation is one sta_nn_query under T and one 192-byte readback (which waits for the stream).'",
    "cloud.chamfer": "vista_slam_amd/cloud.py, chamfer: two NNIndex.build calls (sta_nn_build's synchronisation) and the readback of the two records",
}
EXEMPT = {}


def _room(seed, n=700):
    import cloud_cases as CC
    ref, src, _move = CC.box_room_pair(n, seed=30 + seed)
    return ref, src


def _mk_build(seed):
    def make(m):
        return {"ref": _up(_room(seed)[0])}
    return make


def _index_outputs(index):
    """the index as tensors: the struct's numbers and the used parts of its four arrays (views of the index buffer)"""
    import torch
    info, buf = index.info, index._buf
    base = buf.data_ptr()
    def view(ptr, nbytes):
        return buf[ptr - base:ptr - base + nbytes].clone()
    C, n = int(info.C), int(info.n_finite)
    head = torch.tensor([int(info.M), n, C, *info.lo, *info.ext], dtype=torch.int64)
    return [("info", head), ("cell_key", view(info.cell_key, 8 * C)), ("cell_start", view(info.cell_start, 4 * (C + 1))),
            ("sorted_pts", view(info.sorted_pts, 12 * n)), ("sorted_idx", view(info.sorted_idx, 4 * n))]


def _run_build(m, x, between=None):
    from vista_slam_amd import cloud
    return _index_outputs(cloud.NNIndex.build(x["ref"], 0.1))


def _mk_query(seed):
    def make(m):
        from vista_slam_amd import cloud
        ref, src = _room(seed)
        return {"qry": _up(src), "_index": cloud.NNIndex.build(_up(ref), 0.1)}
    return make


def _run_query(m, x, between=None):
    import cloud_cases as CC
    T = [[1.0, 0.001, 0.0, 0.002], [-0.001, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -0.001]]
    out = x["_index"].query(x["qry"], 0.1, T=T)
    assert CC.RECORD == out["record"].numel()
    return [(k, out[k]) for k in ("d2", "idx", "record")]


def _mk_transform(seed):
    def make(m):
        return {"pts": _up(_room(seed)[1])}
    return make


def _run_transform(m, x, between=None):
    from vista_slam_amd import cloud
    return [("out", cloud.transform(x["pts"], [[0.5, 0.1, 0.0, 1.0], [0.0, 1.5, 0.2, -2.0], [0.3, 0.0, 0.9, 0.25]]))]


def _mk_icp(seed):
    def make(m):
        from vista_slam_amd import cloud
        ref, src = _room(seed)
        return {"src": _up(src), "_index": cloud.NNIndex.build(_up(ref), 0.1)}
    return make


def _run_icp(m, x, between=None):
    import torch
    from vista_slam_amd import cloud
    r = cloud.icp(x["src"], x["_index"], 0.1)
    return [("T", torch.from_numpy(r.T)), ("numbers", torch.tensor([r.fitness, r.inlier_rmse, float(r.iterations)], dtype=torch.float64))]


def _mk_chamfer(seed):
    def make(m):
        ref, src = _room(seed)
        return {"ref": _up(ref), "est": _up(src)}
    return make


def _run_chamfer(m, x, between=None):
    import torch
    from vista_slam_amd import cloud
    c = cloud.chamfer(x["ref"], x["est"], 0.05, return_distances=True)
    return [("numbers", torch.tensor([c.chamfer, c.rmse_1, c.rmse_2], dtype=torch.float64)), ("dist_1", c.dist_1), ("dist_2", c.dist_2)]


def _seeded(name, entries, mk, run, shapes, layer=()):
    return Row(name, entries, mk(0), run, shapes, (), mk(1), layer)


ROWS = [
    _seeded("nn_build", ("sta_nn_build",), _mk_build, _run_build, "700 points on a box, cell 0.1"),
    _seeded("nn_query", ("sta_nn_query",), _mk_query, _run_query, "700 queries under a non-identity T, all three outputs"),
    _seeded("cloud_transform", ("sta_cloud_transform",), _mk_transform, _run_transform, "700 points"),
    _seeded("icp", ("sta_nn_query",), _mk_icp, _run_icp, "cloud.icp, 700 points onto a prebuilt index", layer=("cloud.icp",)),
    _seeded("chamfer", ("sta_nn_build", "sta_nn_query"), _mk_chamfer, _run_chamfer, "cloud.chamfer, 700 / 700 points with distances", layer=("cloud.chamfer",)),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
