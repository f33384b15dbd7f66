"""GPU: libsta_simp.so against the numpy restatement of tests/simp_cases.py, stage by stage and bit for bit - vcell and the cell count,
the output triangles, tri_src, cell_out, vmap, the eight counters, positions and colours for both placements - through the C ABI with
guard bytes behind every buffer; two calls and a call on a shuffled workspace give the same bits; the Python layer
(simplify.simplify_mesh, cells, cluster_triangles) equals the C ABI; save_data_all(mesh_simplify_cell=) writes the simplified mesh and
leaves every other file alone."""
import ctypes as C

import numpy as np
import pytest

import simp_cases as SP

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


def _guarded(nbytes, fill=FILL):
    import torch
    return torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")


def _shuffled(nbytes, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    buf = torch.randint(0, 256, (nbytes + GUARD,), dtype=torch.uint8, device="cuda", generator=g)
    buf[nbytes:] = FILL
    return buf


def _tail_untouched(buf, nbytes, what):
    assert bool((buf[nbytes:] == FILL).all()), f"{what}: the guard behind its {nbytes} bytes was written"


def _up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the shared cases are read-only


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _take(buf, nbytes, dtype, shape):
    return buf[:nbytes].cpu().numpy().view(dtype).reshape(shape)


def simplify_abi(v, col, t, cell, origin, placement, sv_ratio=1e-3, work_seed=None):
    """the three stages through the C ABI -> dict of host arrays (worst-case sizes) and the counters"""
    import torch
    from vista_slam_amd import _lib
    lib = _lib.load_simp()
    nv, nt = len(v), len(t)
    o = (0.0, 0.0, 0.0) if origin is None else tuple(float(x) for x in origin)
    sizes = (C.c_int64 * 3)()
    assert lib.sta_simp_plan(nt, nv, sizes) == 0 and tuple(sizes) == SP.plan(nt, nv)
    dv, dt = (_up(v) if nv else None), (_up(t.astype(np.int32)) if nt else None)
    dc = _guarded(0) if col is not None and not nv else (_up(col) if col is not None else None)      # (no rows: any pointer that is not null)
    mk = (lambda n, k: _guarded(n)) if work_seed is None else (lambda n, k: _shuffled(n, work_seed + k))
    size = {"vcell": 4 * nv, "tris_out": 12 * nt, "tri_src": 4 * nt, "cell_out": 4 * nv, "vmap": 4 * nv, "verts_out": 12 * nv, "colors_out": 12 * nv,
            "counters": 64, "work0": int(sizes[0]), "work1": int(sizes[1]), "work2": int(sizes[2])}
    b = {k: (mk(n, i) if k.startswith("work") else _guarded(n)) for i, (k, n) in enumerate(size.items())}
    p = {k: x.data_ptr() for k, x in b.items()}
    _lib.check_simp(lib.sta_simp_cells(_ptr(dv), nv, float(cell), o[0], o[1], o[2], p["vcell"], p["counters"], p["work0"], size["work0"], _st()))
    _lib.check_simp(lib.sta_simp_triangles(_ptr(dt), nt, nv, p["vcell"], p["tris_out"], p["tri_src"], p["cell_out"], p["vmap"], p["counters"], p["work1"],
                                           size["work1"], _st()))
    _lib.check_simp(lib.sta_simp_place(_ptr(dv), dc.data_ptr() if dc is not None else None, nv, _ptr(dt), nt, p["vcell"], p["cell_out"], float(cell), o[0], o[1], o[2], placement, sv_ratio,
                                       p["verts_out"], p["colors_out"] if dc is not None else None, p["counters"], p["work2"], size["work2"], _st()))
    torch.cuda.synchronize()
    for k, n in size.items():
        _tail_untouched(b[k], n, k)
    out = {"vcell": _take(b["vcell"], 4 * nv, np.int32, nv), "tris_out": _take(b["tris_out"], 12 * nt, np.int32, (nt, 3)),
           "tri_src": _take(b["tri_src"], 4 * nt, np.int32, nt), "cell_out": _take(b["cell_out"], 4 * nv, np.int32, nv),
           "vmap": _take(b["vmap"], 4 * nv, np.int32, nv), "counters": tuple(int(x) for x in _take(b["counters"], 64, np.int64, 8))}
    n_out = out["counters"][1]
    out["verts"] = _take(b["verts_out"], 12 * nv, np.float32, (nv, 3))[:n_out]
    out["colors"] = _take(b["colors_out"], 12 * nv, np.float32, (nv, 3))[:n_out] if dc is not None else None
    assert bool((b["verts_out"][12 * n_out:12 * nv] == FILL).all()), "rows behind the output vertices were written"
    return out


INTEGER_KEYS = ("vcell", "tris_out", "tri_src", "cell_out", "vmap")


def same_bits(got, want, what):
    for k in INTEGER_KEYS:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.nonzero(np.atleast_1d((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1)))[0][:8]}"
    assert tuple(got["counters"]) == tuple(want["counters"]), (what, got["counters"], want["counters"])
    for k in ("verts", "colors"):
        if want[k] is None:
            assert got[k] is None
            continue
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        same = got[k].view(np.uint32) == want[k].view(np.uint32)
        assert same.all(), (f"{what}: {k} differs in {int((~same).any(axis=1).sum())} of {len(same)} rows, first {np.nonzero((~same).any(axis=1))[0][:5]}, "
                            f"largest |difference| {np.nanmax(np.abs(got[k].astype(np.float64) - want[k].astype(np.float64))):.3e}")


@pytest.mark.parametrize("placement", (SP.PLACE_MEAN, SP.PLACE_QUADRIC))
@pytest.mark.parametrize("name", list(SP.CASES))
def test_every_stage_against_the_restatement(name, placement):
    v, col, t, cell, origin = SP.CASES[name]()
    want = SP.expected(name, placement)
    got = simplify_abi(v, col, t, cell, origin, placement)
    print(f"[simp] {name} placement {placement}: {dict(zip(SP.COUNTERS, got['counters']))}")
    same_bits(got, want, f"{name} / placement {placement}")


def test_without_colours_and_with_another_sv_ratio():
    v, _col, t, cell, origin = SP.CASES["hostile"]()
    for sv in (0.0, 0.25):
        want = SP.simplify(v, None, t, cell, origin, SP.PLACE_QUADRIC, sv)
        same_bits(simplify_abi(v, None, t, cell, origin, SP.PLACE_QUADRIC, sv), want, f"hostile without colours, sv_ratio {sv}")


@pytest.mark.parametrize("name", ("hostile", "crease"))
def test_two_calls_and_a_shuffled_workspace_give_the_same_bits(name):
    v, col, t, cell, origin = SP.CASES[name]()
    a = simplify_abi(v, col, t, cell, origin, SP.PLACE_QUADRIC)
    b = simplify_abi(v, col, t, cell, origin, SP.PLACE_QUADRIC)
    c = simplify_abi(v, col, t, cell, origin, SP.PLACE_QUADRIC, work_seed=7)
    same_bits(b, a, f"{name}: second call")
    same_bits(c, a, f"{name}: shuffled workspace")


def test_refusals():
    from vista_slam_amd import _lib
    lib = _lib.load_simp()
    N = None
    cases = ((lib.sta_simp_cells, (N, -1, 1.0, 0.0, 0.0, 0.0, N, N, N, 0, N), r"simp_cells: nv must be in \[0, 2\^31\) \(got -1\)"),
             (lib.sta_simp_cells, (N, 3, 0.0, 0.0, 0.0, 0.0, N, N, N, 0, N), r"simp_cells: cell must be finite and > 0 \(got 0\)"),
             (lib.sta_simp_cells, (N, 3, float("inf"), 0.0, 0.0, 0.0, N, N, N, 0, N), r"cell must be finite and > 0 \(got inf\)"),
             (lib.sta_simp_cells, (N, 3, 1.0, 0.0, float("nan"), 0.0, N, N, N, 0, N), r"the origin must be finite \(got 0, nan, 0\)"),
             (lib.sta_simp_cells, (N, 3, 1.0, 0.0, 0.0, 0.0, N, N, N, 100, N), rf"work of 100 bytes, {SP.plan(0, 3)[0]} needed for 3 vertices"),
             (lib.sta_simp_cells, (N, 3, 1.0, 0.0, 0.0, 0.0, N, N, N, 1 << 20, N), r"null argument"),
             (lib.sta_simp_triangles, (N, 2 ** 31 // 3 + 1, 3, N, N, N, N, N, N, N, 0, N), r"simp_triangles: nt must be >= 0 and 3 \* nt below 2\^31 \(got nt = 715827883\)"),
             (lib.sta_simp_triangles, (N, 5, 3, N, N, N, N, N, N, N, 100, N), rf"work of 100 bytes, {SP.plan(5, 3)[1]} needed for 5 triangles and 3 vertices"),
             (lib.sta_simp_triangles, (N, 5, 3, N, N, N, N, N, N, N, 1 << 20, N), r"null argument"),
             (lib.sta_simp_place, (N, N, 3, N, 5, N, N, 1.0, 0.0, 0.0, 0.0, 2, 1e-3, N, N, N, N, 0, N), r"simp_place: placement must be 0 or 1 \(got 2\)"),
             (lib.sta_simp_place, (N, N, 3, N, 5, N, N, 1.0, 0.0, 0.0, 0.0, 1, 1.0, N, N, N, N, 0, N), r"sv_ratio must be in \[0, 1\) \(got 1\)"),
             (lib.sta_simp_place, (N, N, 3, N, 5, N, N, 1.0, 0.0, 0.0, 0.0, 1, float("nan"), N, N, N, N, 0, N), r"sv_ratio must be in"),
             (lib.sta_simp_place, (N, 1, 3, N, 5, N, N, 1.0, 0.0, 0.0, 0.0, 1, 1e-3, N, N, N, N, 0, N), r"colors \(given\) and colors_out \(NULL\) go together"),
             (lib.sta_simp_place, (N, N, 3, N, 5, N, N, 1.0, 0.0, 0.0, 0.0, 1, 1e-3, N, N, N, N, 100, N), rf"work of 100 bytes, {SP.plan(5, 3)[2]} needed"),
             (lib.sta_simp_place, (N, N, 3, N, 5, N, N, 1.0, 0.0, 0.0, 0.0, 1, 1e-3, N, N, N, N, 1 << 20, N), r"null argument"))
    for fn, args, msg in cases:
        with pytest.raises(_lib.StaError, match=msg):
            _lib.check_simp(fn(*args))


# ------------------------------------------------------------------------------------------ the Python layer
def _mesh_of(v, t, col=None):
    from vista_slam_amd import tsdf
    return tsdf.Mesh(_up(v), _up(col) if col is not None else None, _up(t))


@pytest.mark.parametrize("name", ("sphere_shifted", "hostile", "empty"))
def test_simplify_mesh_equals_the_restatement(name):
    from vista_slam_amd import simplify
    v, col, t, cell, origin = SP.CASES[name]()
    for placement, code in (("mean", SP.PLACE_MEAN), ("quadric", SP.PLACE_QUADRIC)):
        want = SP.expected(name, code)
        mesh, maps = simplify.simplify_mesh(_mesh_of(v, t, col), cell, origin=origin, placement=placement, return_maps=True)
        n_v, n_t = want["counters"][1], want["counters"][2]
        assert tuple(maps.counters) == tuple(want["counters"]) and maps.counters._fields == SP.COUNTERS
        assert np.array_equal(mesh.triangles.cpu().numpy(), want["tris_out"][:n_t]) and np.array_equal(maps.tri_src.cpu().numpy(), want["tri_src"][:n_t])
        assert np.array_equal(maps.vmap.cpu().numpy(), want["vmap"])
        assert mesh.vertices.shape == (n_v, 3) and np.array_equal(mesh.vertices.cpu().numpy().view(np.uint32), want["verts"].view(np.uint32))
        assert np.array_equal(mesh.colors.cpu().numpy().view(np.uint32), want["colors"].view(np.uint32))
    plain = simplify.simplify_mesh(_mesh_of(v, t), cell, origin=origin)
    assert plain.colors is None and np.array_equal(plain.vertices.cpu().numpy().view(np.uint32), SP.expected(name)["verts"].view(np.uint32))
    vcell, counters = simplify.cells(_mesh_of(v, t), cell, origin)
    cl = simplify.cluster_triangles(_mesh_of(v, t), cell, origin)
    want = SP.expected(name)
    assert np.array_equal(vcell.cpu().numpy(), want["vcell"]) and np.array_equal(cl.vcell.cpu().numpy(), want["vcell"])
    assert counters.tolist() == [want["counters"][0], 0, 0, want["counters"][3], 0, 0, 0, 0]
    assert cl.counters.tolist() == list(want["counters"][:7]) + [0]
    for k, got in (("tris_out", cl.triangles), ("tri_src", cl.tri_src), ("cell_out", cl.cell_out), ("vmap", cl.vmap)):
        assert np.array_equal(got.cpu().numpy(), want[k]), k
    with pytest.raises(ValueError, match="placement must be"):
        simplify.simplify_mesh(_mesh_of(v, t), cell, placement="median")
    with pytest.raises(ValueError, match=r"simp_cells: cell must be finite and > 0 \(got -1\)"):
        simplify.simplify_mesh(_mesh_of(v, t), -1.0)
    with pytest.raises(ValueError, match=r"sv_ratio must be in \[0, 1\) \(got 1\)"):
        simplify.simplify_mesh(_mesh_of(v, t), cell, sv_ratio=1.0)


def test_save_data_all_simplifies_the_mesh_and_leaves_the_other_files_alone(tmp_path):
    import filecmp
    import os
    import tsdf_cases as TC
    from vista_slam_amd import formats, simplify, tsdf
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    s = TC.room_scene(9, 13, 4)
    kw = dict(poses=s["poses"], scales=s["scales"], depths=s["depths"], confs=s["confs"], intrinsics=s["intrinsics"], imgs=s["imgs"], conf_thres=s["conf_thres"],
              view_graph={0: [1]}, loop_min_dist=3, view_names=["a", "b", "c", "d"], mesh_voxel_size=0.125)
    _v, (_keys, _t, _w, _c, verts, cols, tris) = TC.room_expected(9, 13, 4)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    formats.save_data_all(m, a, **kw)
    formats.save_data_all(m, b, **kw, mesh_simplify_cell=0.5)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in os.listdir(a):
        if f != "mesh.ply":
            assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
    # without the keyword: the fused mesh as it was written before the keyword existed
    tsdf.write_mesh_ply(str(tmp_path / "plain.ply"), _mesh_of(verts, tris, cols))
    assert filecmp.cmp(os.path.join(a, "mesh.ply"), str(tmp_path / "plain.ply"), shallow=False)
    # with it: the file that write_mesh_ply writes for simplify_mesh of that mesh, which is the restatement's mesh
    small = simplify.simplify_mesh(_mesh_of(verts, tris, cols), 0.5)
    tsdf.write_mesh_ply(str(tmp_path / "small.ply"), small)
    assert filecmp.cmp(os.path.join(b, "mesh.ply"), str(tmp_path / "small.ply"), shallow=False)
    want = SP.simplify(verts, cols, tris, 0.5)
    rec, got = tsdf.read_mesh_ply(os.path.join(b, "mesh.ply"))
    n_v, n_t = want["counters"][1], want["counters"][2]
    print(f"[simp] save_data_all: {len(tris)} -> {n_t} triangles, {len(verts)} -> {n_v} vertices at a cell of 0.5")
    assert 0 < n_t < len(tris) and np.array_equal(got, want["tris_out"][:n_t])
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), want["verts"].astype(np.float64))
