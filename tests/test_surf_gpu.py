"""GPU: libsta_surf.so (csrc/surf.h) against the numpy restatement of its contract (tests/surf_cases.py), through the C ABI into buffers of
exactly the planned size with a guard region behind every one, and the Python layer on top of it (surface.components, clean_mesh, area,
sample_surface; evaluate.eval_mesh, mesh_depth_l1).  Every comparison is array_equal (NaN equal to NaN) on labels, counts, prefixes,
samples, colours and normals; the float64 means of eval_mesh are torch device sums in another order and are compared at 1e-12 relative,
its two ratios by their integer counts."""
import ctypes as C

import numpy as np
import pytest

import cloud_cases as CC
import mesh_cases as MC
import render_cases as RC
import surf_cases as SF

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


def _guarded(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")


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


def components_abi(tris, nv):
    """sta_surf_components through the C ABI -> (vlabel, tlabel, tcount, status)"""
    import torch
    from vista_slam_amd import _lib
    lib = _lib.load_surf()
    nt = len(tris)
    sizes = (C.c_int64 * 3)()
    assert lib.sta_surf_plan(nt, nv, 0, sizes) == 0 and tuple(sizes) == SF.plan(nt, nv)
    d = _up(tris.astype(np.int32)) if nt else None
    bufs = {"vlabel": _guarded(4 * nv), "tlabel": _guarded(4 * nt), "tcount": _guarded(4 * nv), "status": _guarded(4), "work": _guarded(int(sizes[0]))}
    _lib.check_surf(lib.sta_surf_components(_ptr(d), nt, nv, bufs["vlabel"].data_ptr(), bufs["tlabel"].data_ptr(), bufs["tcount"].data_ptr(),
                                            bufs["status"].data_ptr(), bufs["work"].data_ptr(), int(sizes[0]), _st()))
    torch.cuda.synchronize()
    for k, n in (("vlabel", 4 * nv), ("tlabel", 4 * nt), ("tcount", 4 * nv), ("status", 4), ("work", int(sizes[0]))):
        _tail_untouched(bufs[k], n, k)
    return (_take(bufs["vlabel"], 4 * nv, np.int32, nv), _take(bufs["tlabel"], 4 * nt, np.int32, nt), _take(bufs["tcount"], 4 * nv, np.int32, nv),
            int(_take(bufs["status"], 4, np.int32, 1)[0]))


@pytest.mark.parametrize("name", list(SF.COMPONENT_CASES))
def test_components_against_the_restatement(name):
    tris, nv = SF.COMPONENT_CASES[name]()
    want = SF.components(tris, nv)
    got = components_abi(tris, nv)
    print(f"[surf] {name}: {len(tris)} triangles, {nv} vertices, {np.count_nonzero(want[2])} components, status {got[3]}")
    assert got[3] == 0
    for g, w, what in zip(got[:3], want, ("vlabel", "tlabel", "tcount")):
        assert np.array_equal(g, w), (name, what)
    again = components_abi(tris, nv)                         # two calls give the same bits
    assert again[3] == 0 and all(np.array_equal(a, g) for a, g in zip(again[:3], got[:3]))
    p = np.random.default_rng(4).permutation(len(tris))      # the order of the triangles does not matter
    shuffled = components_abi(tris[p], nv)
    assert shuffled[3] == 0 and np.array_equal(shuffled[0], got[0]) and np.array_equal(shuffled[2], got[2]) and np.array_equal(shuffled[1], got[1][p])


def weights_abi(v, t, keep=None):
    import torch
    from vista_slam_amd import _lib
    lib = _lib.load_surf()
    nt, nv = len(t), len(v)
    sizes = (C.c_int64 * 3)()
    assert lib.sta_surf_plan(nt, nv, 0, sizes) == 0 and tuple(sizes) == SF.plan(nt, nv)
    dv, dt, dk = _up(v), _up(t), (_up(keep.astype(np.uint8)) if keep is not None else None)
    P, total, work = _guarded(8 * nt), _guarded(8), _guarded(int(sizes[1]))
    _lib.check_surf(lib.sta_surf_weights(_ptr(dv), nv, _ptr(dt), nt, _ptr(dk), P.data_ptr(), total.data_ptr(), work.data_ptr(), int(sizes[1]), _st()))
    torch.cuda.synchronize()
    for buf, n, what in ((P, 8 * nt, "P"), (total, 8, "total"), (work, int(sizes[1]), "work")):
        _tail_untouched(buf, n, what)
    return _take(P, 8 * nt, np.float64, nt), _take(total, 8, np.float64, 1)[0], (dv, dt, P, total)


@pytest.mark.parametrize("nt", SF.PREFIX_SIZES)
def test_the_prefix_at_the_chunk_boundaries(nt):
    v, t = SF.prefix_mesh(nt)
    P, total, _ = weights_abi(v, t)
    wantP, want_total = SF.prefix(SF.tri_weights(v, t))
    assert np.array_equal(P, wantP) and total == want_total == P[-1] and total > 0


def test_the_prefix_of_the_hostile_set_and_of_a_keep_mask():
    v, t = SF.hostile()
    P, total, _ = weights_abi(v, t)
    wantP, want_total = SF.prefix(SF.tri_weights(v, t))
    assert np.array_equal(P, wantP) and total == want_total and np.isfinite(total) and np.all(np.diff(P) >= 0)
    keep = np.random.default_rng(8).random(len(t)) < 0.5
    P, total, _ = weights_abi(v, t, keep)
    wantP, want_total = SF.prefix(SF.tri_weights(v, t, keep))
    assert np.array_equal(P, wantP) and total == want_total
    P, total, _ = weights_abi(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert len(P) == 0 and total == 0.0


def sample_abi(v, t, ns, seed=0, keep=None, colors=None, normals=False):
    import torch
    from vista_slam_amd import _lib
    lib = _lib.load_surf()
    _P, _total, (dv, dt, P, total) = weights_abi(v, t, keep)
    dc = _up(np.asarray(colors, dtype=np.float32)) if colors is not None else None
    out = {"points": _guarded(12 * ns), "tri": _guarded(4 * ns), "colors": _guarded(12 * ns) if colors is not None else None,
           "normals": _guarded(12 * ns) if normals else None}
    _lib.check_surf(lib.sta_surf_sample(_ptr(dv), len(v), _ptr(dt), len(t), P.data_ptr(), total.data_ptr(), _ptr(dc), ns, seed, out["points"].data_ptr(),
                                        out["tri"].data_ptr(), out["colors"].data_ptr() if out["colors"] is not None else None,
                                        out["normals"].data_ptr() if out["normals"] is not None else None, _st()))
    torch.cuda.synchronize()
    got = {}
    for k, b in out.items():
        if b is not None:
            n = 4 * ns if k == "tri" else 12 * ns
            _tail_untouched(b, n, k)
            got[k] = _take(b, n, np.int32 if k == "tri" else np.float32, (ns,) if k == "tri" else (ns, 3))
    return got


def same_samples(got, want, what):
    for k, g in got.items():
        assert np.array_equal(g, want[k], equal_nan=k != "tri"), (what, k)


@pytest.fixture(scope="module")
def sphere_expected():
    """the restatement's samples of the sphere: computed once, shared, never changed"""
    v, t, col = SF.sphere()
    return {(ns, seed): SF.sample(v, t, ns, seed=seed, colors=col, normals=True) for ns in SF.SAMPLE_SIZES for seed in (SF.SEEDS if ns == 4096 else SF.SEEDS[:1])}


@pytest.mark.parametrize("ns", SF.SAMPLE_SIZES)
def test_samples_of_the_sphere(sphere_expected, ns):
    v, t, col = SF.sphere()
    got = sample_abi(v, t, ns, 0, colors=col, normals=True)
    same_samples(got, sphere_expected[(ns, 0)], f"ns = {ns}")
    if ns:
        assert got["tri"].min() >= 0 and np.isfinite(got["points"]).all()
    if ns == 4096:
        seed = SF.SEEDS[1]
        other = sample_abi(v, t, ns, seed, colors=col, normals=True)
        same_samples(other, sphere_expected[(ns, seed)], f"ns = {ns}, seed 2^63 + 5")
        assert not np.array_equal(other["points"], got["points"])
        plain = sample_abi(v, t, ns, 0)                      # without colours and normals: the same points
        assert set(plain) == {"points", "tri"} and np.array_equal(plain["points"], got["points"]) and np.array_equal(plain["tri"], got["tri"])


def test_samples_of_the_hostile_set_a_keep_mask_and_a_mesh_without_area():
    v, t = SF.hostile()
    same_samples(sample_abi(v, t, 50000, SF.SEEDS[1]), SF.sample(v, t, 50000, seed=SF.SEEDS[1]), "hostile")
    v, t, col = SF.sphere()
    keep = np.arange(len(t)) % 3 == 0
    got = sample_abi(v, t, 4096, 7, keep=keep, normals=True)
    same_samples(got, SF.sample(v, t, 4096, seed=7, keep=keep, normals=True), "keep")
    assert keep[got["tri"]].all()
    v, t = SF.flat_mesh()
    got = sample_abi(v, t, 7, 0, colors=np.ones((5, 3), np.float32), normals=True)
    assert (got["tri"] == -1).all() and all(np.isnan(got[k]).all() for k in ("points", "colors", "normals"))
    same_samples(got, SF.sample(v, t, 7, colors=np.ones((5, 3), np.float32), normals=True), "flat")


def test_refusals():
    from vista_slam_amd import _lib
    lib = _lib.load_surf()
    cases = ((lib.sta_surf_components, (None, -1, 3, None, None, None, None, None, 0, None), r"surf_components: nt must be in \[0, 2\^31\) \(got -1\)"),
             (lib.sta_surf_components, (None, 1, 2 ** 31, None, None, None, None, None, 0, None), r"nv must be in"),
             (lib.sta_surf_components, (None, 1, 100, None, None, None, None, None, 100, None), r"work of 100 bytes, 512 needed for 100 vertices"),
             (lib.sta_surf_components, (None, 1, 3, None, None, None, None, None, 256, None), r"null argument"),
             (lib.sta_surf_weights, (None, 3, None, 2000, None, None, None, None, 100, None), r"work of 100 bytes, 512 needed for 2000 triangles"),
             (lib.sta_surf_weights, (None, 3, None, 2 ** 31, None, None, None, None, 0, None), r"nt must be in"),
             (lib.sta_surf_sample, (None, 3, None, 1, None, None, None, 2 ** 31, 0, None, None, None, None, None), r"ns must be in \[0, 2\^31\) \(got 2147483648\)"),
             (lib.sta_surf_sample, (None, 3, None, 1, None, None, None, 5, 0, None, None, 1, None, None), r"colors_out without colors"),
             (lib.sta_surf_sample, (None, 3, None, 1, None, None, None, 5, 0, None, None, None, None, None), r"null argument"))
    for fn, args, msg in cases:
        with pytest.raises(_lib.StaError, match=msg):
            _lib.check_surf(fn(*args))
    assert lib.sta_surf_sample(None, 3, None, 1, None, None, None, 0, 0, None, None, None, None, None) == 0        # ns == 0 launches nothing


# ------------------------------------------------------------------------------------------ the Python layer
def _mesh_of(v, t, col=None):
    from vista_slam_amd import tsdf
    return tsdf.Mesh(_up(v), _up(col) if col is not None else None, _up(t))


def _floaters():
    """the sphere, its first 40 triangles twice more far away (two floaters that tie piece by piece), a lone triangle and a bad one"""
    v, t, col = SF.sphere()
    nv = len(v)
    a, b = t[:40], t[:40]
    V = np.concatenate([v, v + np.float32(30.0), v + np.float32(60.0), np.zeros((3, 3), np.float32)])
    T = np.concatenate([b + 2 * nv, t, a + nv, [[3 * nv, 3 * nv + 1, 3 * nv + 2]], [[0, 1, -1]]]).astype(np.int32)
    return V, T, np.concatenate([col, col, col, np.ones((3, 3), np.float32)])


def test_clean_mesh_and_components():
    from vista_slam_amd import surface
    V, T, col = _floaters()
    mesh = _mesh_of(V, T, col)
    vlabel, tlabel, tcount = [a.cpu().numpy() for a in surface.components(mesh)]
    want = SF.components(T, len(V))
    assert all(np.array_equal(g, w) for g, w in zip((vlabel, tlabel, tcount), want))
    sizes = sorted(tcount[tcount > 0].tolist())
    print(f"[surf] floaters: component sizes {sizes}")
    assert sizes[-1] >= 2000 and sizes.count(1) >= 1
    for kw in (dict(min_triangles=2), dict(min_triangles=100), dict(keep_largest=1), dict(keep_largest=2), dict(keep_largest=3), dict(min_triangles=2, keep_largest=1000),
               dict(keep_largest=0), dict(min_triangles=10 ** 6)):
        got = surface.clean_mesh(mesh, **kw)
        keep = SF.clean_keep(want[1], want[2], **kw)
        wv, wc, wt = SF.cull_mesh(V, col, T, keep)
        assert np.array_equal(got.vertices.cpu().numpy(), wv) and np.array_equal(got.colors.cpu().numpy(), wc) and np.array_equal(got.triangles.cpu().numpy(), wt), kw
    # a tie: the pieces of the two floaters have equal counts somewhere, and the lower root wins
    roots = np.nonzero(want[2])[0]
    counts = want[2][roots]
    assert len(set(counts.tolist())) < len(counts), "the floaters were meant to tie"
    with pytest.raises(ValueError):
        surface.clean_mesh(mesh)
    assert float(surface.area(_mesh_of(*SF.sphere()[:2])).cpu()) == SF.prefix(SF.tri_weights(*SF.sphere()[:2]))[1] * 0.5


def test_sample_surface_equals_the_c_abi():
    from vista_slam_amd import surface
    v, t, col = SF.sphere()
    s = surface.sample_surface(_mesh_of(v, t, col), 4096, seed=SF.SEEDS[1] - 2 ** 64, colors=True, normals=True)      # seeds are taken modulo 2^64
    want = SF.sample(v, t, 4096, seed=SF.SEEDS[1], colors=col, normals=True)
    same_samples({"points": s.points.cpu().numpy(), "tri": s.triangles.cpu().numpy(), "colors": s.colors.cpu().numpy(), "normals": s.normals.cpu().numpy()}, want, "layer")
    s = surface.sample_surface(_mesh_of(v, t), 7)
    assert s.colors is None and s.normals is None and np.array_equal(s.points.cpu().numpy(), SF.sample(v, t, 7)["points"])
    with pytest.raises(ValueError, match="colors=True"):
        surface.sample_surface(_mesh_of(v, t), 7, colors=True)
    with pytest.raises(ValueError, match=r"ns must be in"):
        surface.sample_surface(_mesh_of(v, t), -1)


def test_eval_mesh_sphere_against_shifted_sphere():
    from vista_slam_amd import evaluate
    v, t, col = SF.sphere()
    n, d = 2000, np.array([0.03125, 0.0, 0.0], dtype=np.float32)
    est = SF.sample(v + d, t, n, seed=3)["points"]
    gt = SF.sample(v, t, n, seed=4)["points"]
    for T in (None, np.concatenate([np.eye(3), -d[:, None].astype(np.float64)], axis=1)):
        e = est if T is None else CC.transform(est, T)
        want = SF.eval_points(e, gt, threshold=0.05, max_error=0.5)
        got = evaluate.eval_mesh("cuda:0", _mesh_of(v + d, t, col), _mesh_of(v, t), n_samples=n, threshold=0.05, max_error=0.5, T=T, seed=3)
        assert np.array_equal(got.est_points.cpu().numpy(), e) and np.array_equal(got.gt_points.cpu().numpy(), gt)
        assert (got.n_precise, got.n_complete) == (want["n_precise"], want["n_complete"])
        assert got.precision == want["precision"] and got.completion_ratio == want["completion_ratio"] and got.fscore == want["fscore"]
        for k in ("accuracy", "completion", "chamfer"):
            assert abs(getattr(got, k) - want[k]) <= 1e-12 * want[k], (k, getattr(got, k), want[k])
        print(f"[surf] eval_mesh T {'given' if T is not None else 'None'}: accuracy {got.accuracy:.5f} completion {got.completion:.5f} fscore {got.fscore:.4f}")
    cloud = evaluate.eval_mesh("cuda:0", _mesh_of(v, t), gt, n_samples=n, seed=4)          # a cloud is taken as it is; the same samples score 0
    assert cloud.accuracy == 0.0 and cloud.completion == 0.0 and cloud.fscore == 1.0 and cloud.n_precise == n
    with pytest.raises(ValueError, match="threshold must be <= max_error"):
        evaluate.eval_mesh("cuda:0", _mesh_of(v, t), _mesh_of(v, t), threshold=0.6, max_error=0.5)


def test_mesh_depth_l1():
    from vista_slam_amd import evaluate, render
    v, t, _ = SF.sphere()
    H, W, f, _sub = MC.OUTSIDE["24x32"]
    cams = [MC.outside_cam(H, W, f), MC.outside_cam(H, W, f, MC.OBLIQUE_EYE)]
    rc = [render.Camera(np.asarray(c["K"], dtype=np.float64), c["T"], c["near"], c["far"]) for c in cams]
    mesh = _mesh_of(v, t)
    l1, count = evaluate.mesh_depth_l1("cuda:0", mesh, mesh, rc, H, W)
    assert l1 == 0.0 and count > 200
    moved = v + np.array([0.0, 0.0, 0.25], dtype=np.float32)
    total, n = 0.0, 0
    for c in cams:
        depth = []
        for verts in (moved, v):
            keys = RC.new_keys(H, W, 1)
            MC.triangles(keys, 1, verts, t, kind=MC.ID, **c)
            depth.append(RC.resolve(keys, 1)[1].astype(np.float64))
        both = np.isfinite(depth[0]) & np.isfinite(depth[1])
        total += float(np.abs(np.where(both, depth[0], 0.0) - np.where(both, depth[1], 0.0)).sum())
        n += int(both.sum())
    l1, count = evaluate.mesh_depth_l1("cuda:0", _mesh_of(moved, t), mesh, rc, H, W)
    print(f"[surf] mesh_depth_l1: {l1:.6f} over {count} pixels")
    assert count == n > 200 and abs(l1 - total / n) <= 1e-12 * (total / n) and 0.1 < l1 < 0.4


def test_save_data_all_cleans_the_mesh_and_leaves_the_other_files_alone(tmp_path):
    import filecmp
    import os
    import tsdf_cases as TC
    from vista_slam_amd import formats, tsdf
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    s = TC.room_scene(9, 13, 4)
    kw = dict(poses=s["poses"], scales=s["scales"], depths=s["depths"], confs=s["confs"], intrinsics=s["intrinsics"], imgs=s["imgs"], conf_thres=s["conf_thres"],
              view_graph={0: [1]}, loop_min_dist=3, view_names=["a", "b", "c", "d"], mesh_voxel_size=0.125)
    _v, (_keys, _t, _w, _c, verts, cols, tris) = TC.room_expected(9, 13, 4)
    tcount = SF.components(tris, len(verts))[2]
    sizes = sorted(tcount[tcount > 0].tolist())
    cut = sizes[-1]                                           # the scene has floaters of 1 .. 779 triangles: only the largest component stays
    a, b, c = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    formats.save_data_all(m, a, **kw)
    formats.save_data_all(m, b, **kw, mesh_min_triangles=cut)
    formats.save_data_all(m, c, **kw, mesh_min_triangles=0)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == sorted(os.listdir(c))
    for f in os.listdir(a):
        assert filecmp.cmp(os.path.join(a, f), os.path.join(c, f), shallow=False), f          # nothing is small enough to go: byte for byte
        if f != "mesh.ply":
            assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
    rec, got = tsdf.read_mesh_ply(os.path.join(b, "mesh.ply"))
    vlabel, tlabel, tcount = SF.components(tris, len(verts))
    wv, _wc, wt = SF.cull_mesh(verts, cols, tris, SF.clean_keep(tlabel, tcount, min_triangles=cut))
    print(f"[surf] save_data_all: component sizes {sizes}, {len(wt)} of {len(tris)} triangles stay at min_triangles = {cut}")
    assert np.array_equal(got, wt) and np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), wv.astype(np.float64))
