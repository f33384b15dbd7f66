"""The stream-order rows of libsta_tsdf.so and vista_slam_amd.tsdf, in the shape of tests/stream_cases.py (its Row, its harness): every
call is ordered by its stream alone, also behind pending work.  tests/test_tsdf_abi.py holds the entry points named here against the
declarations of include/sta_tsdf.h that take a `void* stream`, in both directions; tests/test_tsdf_stream_gpu.py runs the rows.  The
poison of a floating-point input is NaN (a pixel that is not observed, a projection that fails every range test, a lattice point that is
not known), of the keys 0 (one block index repeated: every search stays inside the list): values the kernels take as data, never as a
fault."""
from stream_cases import Row, _up

SYNCS = {
    "sta_tsdf_blocks": "include/sta_tsdf.h: 'sta_tsdf_blocks and sta_tsdf_mesh synchronise their stream once, to return their counts' - counts_out_host",
    "sta_tsdf_mesh": "include/sta_tsdf.h: 'sta_tsdf_blocks and sta_tsdf_mesh synchronise their stream once, to return their counts' - counts_out_host",
    "tsdf.TSDFVolume.allocate": "tsdf.TSDFVolume: 'allocate and mesh wait for the stream once each (their counts come back); integrate does not'",
    "tsdf.TSDFVolume.mesh": "tsdf.TSDFVolume: 'allocate and mesh wait for the stream once each ...' - a counting call, then one into buffers of that size",
}
EXEMPT = {}
VOXEL = 0.125


def _views(seed):
    import tsdf_cases as TC
    from vista_slam_amd import tsdf
    s = TC.room_scene(9, 13, 4 - seed, seed)
    return tsdf.views(s["depths"], s["scales"], s["intrinsics"], s["poses"], s["confs"], s["imgs"], conf_thres=s["conf_thres"])


def _mk_blocks(seed):
    def make(m):
        from vista_slam_amd import tsdf
        return {"views": _views(seed), "_vol": tsdf.TSDFVolume("cuda:0", VOXEL)}
    return make


def _run_blocks(m, x, between=None):
    vol = x["_vol"].allocate(x["views"])
    return [("keys", vol.keys.clone()), ("tsdf", vol.tsdf.clone()), ("weight", vol.weight.clone()), ("rgb", vol.rgb.clone())]


def _mk_integrate(seed):
    def make(m):
        import torch
        from vista_slam_amd import tsdf
        v = _views(seed)
        vol = tsdf.TSDFVolume("cuda:0", VOXEL).allocate(v)
        torch.cuda.synchronize()
        return {"views": v, "keys": vol.keys, "_vol": vol}
    return make


def _run_integrate(m, x, between=None):
    vol = x["_vol"]
    vol.clear().integrate(x["views"], 0, 2).integrate(x["views"], 2)
    return [("tsdf", vol.tsdf.clone()), ("weight", vol.weight.clone()), ("rgb", vol.rgb.clone())]


def _mk_mesh(seed):
    def make(m):
        import numpy as np
        import tsdf_cases as TC
        from vista_slam_amd import tsdf
        keys, t, w, rgb = TC.random_volume(11 + seed)
        vol = tsdf.TSDFVolume("cuda:0", VOXEL)
        vol.keys, vol.tsdf, vol.weight, vol.rgb = _up(keys.view(np.int64)), _up(t), _up(w), _up(rgb)
        return {"keys": vol.keys, "tsdf": vol.tsdf, "weight": vol.weight, "rgb": vol.rgb, "_vol": vol}
    return make


def _run_mesh(m, x, between=None):
    mesh = x["_vol"].mesh()
    return [("vertices", mesh.vertices), ("colors", mesh.colors), ("triangles", mesh.triangles)]


def _seeded(name, entries, mk, run, shapes, layer=()):
    return Row(name, entries, mk(0), run, shapes, (), mk(1), layer)


ROWS = [
    _seeded("tsdf_blocks", ("sta_tsdf_blocks", "sta_tsdf_clear"), _mk_blocks, _run_blocks, "TSDFVolume.allocate, 4 views of 9x13 at voxel 1/8",
            layer=("tsdf.TSDFVolume.allocate",)),
    _seeded("tsdf_integrate", ("sta_tsdf_clear", "sta_tsdf_integrate"), _mk_integrate, _run_integrate,
            "TSDFVolume.clear + integrate [0,2) + [2,4), 4 views of 9x13 at voxel 1/8", layer=("tsdf.TSDFVolume.integrate",)),
    _seeded("tsdf_mesh", ("sta_tsdf_mesh",), _mk_mesh, _run_mesh, "TSDFVolume.mesh of a random volume of 8 blocks with colours", layer=("tsdf.TSDFVolume.mesh",)),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
