"""GPU: libsta_ray.so through vista_slam_amd/meshdist.py against tests/ray_cases.py, the numpy restatement of include/sta_ray.h.  Every
comparison is array_equal: t, tri and bary of every ray against the brute force over all valid triangles, and occluded against tri >= 0.
The shapes are the smallest at which the code can go wrong: triangle counts around the powers of the fan-out, ray counts around the
wavefront, edges, vertices, ties, both ends of the range, zero components, invalid triangles, hostile magnitudes."""
import math

import numpy as np
import pytest

import dist_cases as D
import ray_cases as RC

pytestmark = pytest.mark.gpu
F = RC.FANOUT


def _mesh(v, t):
    import torch
    from vista_slam_amd import tsdf
    return tsdf.Mesh(torch.from_numpy(np.array(v)).cuda(), None, torch.from_numpy(np.array(t)).cuda())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def check(v, t, o, d, t_min=0.0, t_max=math.inf, ref_answer=None, idx=None):
    """build, cast and test occlusion on the device, brute force in numpy: everything equal, the status word 0 -> the restatement's
    (t, tri, bary, occluded)"""
    import torch
    from vista_slam_amd import meshdist
    idx = meshdist.TriIndex.build(_mesh(v, t)) if idx is None else idx
    want = RC.brute(D.Index(v, t), o, d, t_min, t_max) if ref_answer is None else ref_answer
    od, dd = torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(d)).cuda()
    tt, tri, bary = idx.cast(od, dd, t_min, t_max)
    occ = idx.occluded(od, dd, t_min, t_max)
    got = (tt.cpu().numpy(), tri.cpu().numpy(), bary.cpu().numpy(), occ.cpu().numpy())
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and got[3].dtype == np.uint8
    for name, g, w in zip(("t", "tri", "bary", "occluded"), got, want):
        bad = np.nonzero(~((g == w) | ((g != g) & (w != w))).reshape(len(d), -1).all(axis=1))[0]
        assert _same(g, w), f"{name}: {len(bad)} of {len(d)} rays differ, first {bad[:1]}: got {g[bad[:1]]}, restatement {w[bad[:1]]}"
    assert _same(got[3], (got[1] >= 0).astype(np.uint8))
    assert int(idx.ray_status.item()) == 0, "the status word stays 0"
    return want


@pytest.mark.parametrize("nt", [1, F - 1, F, F + 1, F * F, F * F + 1, F ** 3 + 1])
def test_triangle_counts_around_the_powers_of_the_fan_out(nt):
    v, t = D.soup(nt, seed=nt)
    o, d = RC.soup_rays(65, seed=nt + 1)
    check(v, t, o, d)
    check(v, t, o, d, 0.25, 1.0)


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1000])
def test_ray_counts_around_the_wavefront(R):
    v, t = D.soup(F ** 3 + 1, seed=2)
    o, d = RC.soup_rays(R, seed=R)
    _t, tri, _b, _occ = check(v, t, o, d)
    check(v, t, o, d, 0.0, 0.5)
    if R == 1000:
        assert 100 < (tri >= 0).sum() < 1000


def test_one_triangle_edges_vertices_both_ends_of_the_range_and_zero_components():
    v, t = RC.one_triangle()
    o, d = RC.one_triangle_rays()
    tt, tri, bary, _occ = check(v, t, o, d)
    up = (d[:, 0] == 0) & (d[:, 1] == 0) & (d[:, 2] == 1) & (o[:, 2] == 0) & np.isfinite(o).all(axis=1)
    x, y = o[:, 0].astype(np.float64), o[:, 1].astype(np.float64)
    inside = up & (x >= 0) & (y >= 0) & (x + y <= 4)          # interior, edges, vertices, one step inside an edge, one from a face of the box: all hit, at t = 2 exactly
    assert inside.sum() == 12 and (tri[inside] == 0).all() and (tt[inside] == 2.0).all()
    assert np.array_equal(bary[0], [0.5, 0.25, 0.25]) and np.array_equal(bary[5], [1, 0, 0]) and np.array_equal(bary[6], [0, 1, 0])
    assert (tri[up & ~inside] == -1).all() and (up & ~inside).sum() == 4, "one float32 step outside an edge is a miss"
    assert (tri[15:19] == -1).all(), "parallel to the plane and in the plane: det == 0"
    assert tri[19] == -1 and tri[20] == 0 and tt[20] == 1.0, "a hit behind the origin is none"
    assert np.array_equal(tt[21:24], [1.0, 4.0, 0.125]), "t is in units of |d|"
    assert tri[30] == 0 and tt[30] == 0.0, "the origin on the triangle: t = 0 with t_min = 0"
    assert (tri[31:] == -1).all() and np.isinf(tt[31:]).all() and np.isnan(bary[31:]).all(), "d = 0 and rays that are not finite are unmatched"
    for t_min, t_max in RC.RANGES[1:]:
        tr, trr, _b, _o = check(v, t, o, d, t_min, t_max)
        assert ((trr >= 0) == ((tri >= 0) & (tt >= np.float64(t_min)) & (tt <= np.float64(t_max)))).all(), "both ends are inclusive"
    assert check(v, t, o, d, 2.0, 2.0)[1][0] == 0 and check(v, t, o, d, 0.0, math.inf)[1][0] == 0


def test_ties_the_lowest_index_wins():
    v, t, o, d = RC.coplanar_pair()
    tt, tri, _b, _occ = check(v, t, o, d)
    assert (tt[:7] == 1.0).all() and tt[7] == 2.0
    assert (tri[:5] == 0).all() and tri[7] == 0, "on the shared edge all four qualify: the lowest index"
    assert tri[5] == 1 and tri[6] == 0, "inside one triangle: it or its reversed copy, whichever is lower"
    for seed in range(3):          # the same under permutations that change which index is lowest and where it sits in the sorted order
        perm = np.random.default_rng(seed).permutation(len(t))
        check(v, t[perm], o, d)
    # duplicated and reversed triangles at equal t on a lattice of shared edges and vertices
    v, t = D.lattice()
    q = D.lattice_queries()
    o = (q + np.array([0, 0, 1], dtype=np.float32)).astype(np.float32)
    d = np.tile(np.array([[0, 0, -1]], dtype=np.float32), (len(q), 1))
    tt, tri, _b, _occ = check(v, t, o, d)
    assert (tri >= 0).all(), "a ray onto an edge or a vertex of a lattice never passes between the triangles"
    v2, t2 = D.reversed_duplicated(v, t)
    assert (check(v2, t2, o, d)[1] < len(t)).all(), "of a triangle and its reversed copy the lower index is the copy"


def test_invalid_triangles_are_never_returned_and_a_mesh_without_a_valid_one_matches_nothing():
    v0, t0 = D.soup(100, seed=3)
    v, t = D.with_bad(v0, t0)
    o, d = RC.soup_rays(500, seed=2)
    _t, tri, _b, _occ = check(v, t, o, d)
    cls = D.classify(v, t)
    assert (cls != D.VALID).sum() == 54 and (tri >= 0).sum() > 50 and (cls[tri[tri >= 0]] == D.VALID).all()
    none = check(np.zeros((3, 3), dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32), o, d)
    assert (none[1] == -1).all() and not none[3].any()


def test_one_room_sized_triangle_among_small_ones():
    v, t = D.room()
    o, d = RC.soup_rays(600, seed=5)
    _t, tri, _b, _occ = check(v, t, o, d)
    assert (tri == 150).sum() > 50 and ((tri >= 0) & (tri != 150)).sum() > 10


def test_the_hostile_soup():
    v, t = RC.hostile_mesh()
    o, d = RC.hostile_rays(600, 10, v)
    _t, tri, _b, _occ = check(v, t, o, d)
    assert (tri >= 0).sum() > 100
    check(v, t, o, d, 0.5, 2.0)
    v, t = D.same_centre()
    check(v, t, *RC.soup_rays(300, 4, 4.0, -2.0))


def test_three_spheres_from_inside_and_outside_and_two_casts_give_identical_bits():
    import torch
    from vista_slam_amd import meshdist
    v, t, o, d, ans, near = RC.spheres_case()
    idx = meshdist.TriIndex.build(_mesh(v, t))
    check(v, t, o, d, ref_answer=ans, idx=idx)
    check(v, t, o, d, 0.5, 1.0, ref_answer=near, idx=idx)
    assert 1000 < (ans[1] >= 0).sum() < 2000 and 200 < (near[1] >= 0).sum() < (ans[1] >= 0).sum()
    od, dd = torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(d)).cuda()
    a, b = idx.cast(od, dd), meshdist.ray_cast(od, dd, _mesh(v, t))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    only_t, = idx.cast(od, dd, want=("t",))
    assert torch.equal(only_t, a[0])
    # a single origin is broadcast
    one = idx.cast(od[0], dd[:64])
    assert _same(one[1].cpu().numpy(), RC.brute(D.Index(v, t), o[0], d[:64])[1])
    with pytest.raises(ValueError, match="ray_cast: 0 <= t_min <= t_max"):
        idx.cast(od, dd, 2.0, 1.0)
    with pytest.raises(ValueError, match="want must name"):
        idx.cast(od, dd, want=("d2",))


def _plane(z=2.0, half=8.0):
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def test_ray_depth_of_a_camera_equals_the_restatement_and_visible_is_its_segment_form():
    import torch
    from vista_slam_amd import meshdist, render
    import mesh_cases as MC
    v, t, _ = MC.sphere_mesh()
    H, W = 24, 32
    cam = render.Camera.look_at(MC.OBLIQUE_EYE, MC.SPHERE_CENTRE, (0.0, -1.0, 0.0), 40.0, 40.0, H, W, near=0.5, far=100.0)
    idx = meshdist.TriIndex.build(_mesh(v, t))
    depth = meshdist.ray_depth(idx, cam, H, W)
    o, d = meshdist.camera_rays(cam, H, W)
    want = RC.brute(D.Index(v, t), o.numpy(), d.numpy(), 0.5, 100.0)
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (H, W)
    assert _same(depth.cpu().numpy(), want[0].astype(np.float32).reshape(H, W))
    hit = want[1].reshape(H, W) >= 0
    assert 100 < hit.sum() < H * W and hit[H // 2, W // 2] and not hit[0, 0], "row-major pixels: the sphere in the middle, none in the corner"
    dist = np.linalg.norm(MC.OBLIQUE_EYE - MC.SPHERE_CENTRE)
    assert abs(float(depth[H // 2, W // 2]) - (dist - MC.SPHERE_RADIUS)) < 0.5
    # line of sight: from the eye to points behind the sphere and beside it
    a = np.asarray(MC.OBLIQUE_EYE, dtype=np.float32)
    b = (MC.SPHERE_CENTRE + np.random.default_rng(5).standard_normal((300, 3)) * 6.0).astype(np.float32)
    seen = meshdist.visible(idx, a, b, eps=1e-6).cpu().numpy()
    ref = RC.brute(D.Index(v, t), a, (b.astype(np.float64) - a.astype(np.float64)).astype(np.float32), 1e-6, 1.0 - 1e-6)[3] == 0
    assert seen.dtype == np.bool_ and np.array_equal(seen, ref) and 20 < seen.sum() < 280


def test_pointmap_range_error_is_zero_for_points_on_a_dyadic_plane():
    """Centres at z = 0 and points on the plane z = 2 with |dx|, |dy| <= 2 on a lattice of 1/8: d_z = 2 is the largest component, so
    Sx, Sy, Sz and every sheared coordinate are dyadic and exact, U + V + W = det exactly and t = Sz * 2 = 1 exactly: the error is 0,
    not small.  Points pushed off the plane along their rays score exactly their push."""
    import torch
    from vista_slam_amd import evaluate
    v, t = _plane()
    centres = np.array([[0, 0, 0], [0.5, -0.25, 0], [-1, 1, 0]], dtype=np.float32)
    g = (np.arange(17, dtype=np.float32) - 8) / 8 * 2
    pts = np.stack([np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2) + c[:2] for c in centres])
    pts = np.concatenate([pts, np.full(pts.shape[:2] + (1,), 2.0, dtype=np.float32)], axis=-1).astype(np.float32)          # [3, 289, 3]
    mesh = _mesh(v, t)
    r = evaluate.pointmap_range_error("cuda:0", mesh, centres, pts)
    assert (r.n_hit, r.n_miss) == (3 * 289, 0) and r.abs_mean == 0.0 and r.abs_median == 0.0 and r.rel_mean == 0.0 and r.rel_median == 0.0
    # half of the first view's points moved to 3/4 of their range: the surface is at t = 4/3, |t - 1| = 1/3 of the (shorter) range
    pts2 = pts.copy()
    pts2[0, ::2] = (centres[0] + (pts[0, ::2] - centres[0]) * np.float32(0.75)).astype(np.float32)
    valid = np.ones(pts.shape[:2], dtype=bool)
    valid[2] = False
    from vista_slam_amd import meshdist
    r2 = evaluate.pointmap_range_error("cuda:0", meshdist.TriIndex.build(mesh), torch.from_numpy(centres), torch.from_numpy(pts2).cuda(), valid=valid)
    d = (pts2[0, ::2] - centres[0]).astype(np.float64)
    want_abs = np.concatenate([np.abs(RC.brute(D.Index(v, t), centres[0], d.astype(np.float32))[0] - 1.0) * np.linalg.norm(d, axis=1), np.zeros(2 * 289 - len(d))])
    assert (r2.n_hit, r2.n_miss) == (2 * 289, 0)
    assert abs(r2.abs_mean - want_abs.mean()) <= 1e-12 * want_abs.mean() and r2.abs_median == np.sort(want_abs)[(len(want_abs) - 1) // 2] == 0.0
    assert abs(r2.rel_mean - (len(d) / 3.0) / (2 * 289)) <= 1e-9
    # a point beside the plane is a miss, a NaN point too
    pts3 = pts[:1, :4].copy()
    pts3[0, 0] = [100, 0, 2]
    pts3[0, 1] = [np.nan, 0, 2]
    r3 = evaluate.pointmap_range_error("cuda:0", mesh, centres[:1], pts3)
    assert (r3.n_hit, r3.n_miss) == (2, 2) and r3.abs_mean == 0.0


def test_mesh_depth_l1_by_rays_of_a_mesh_against_itself_is_zero_and_the_raster_default_does_not_move():
    from vista_slam_amd import evaluate, render
    import mesh_cases as MC
    v, t, _ = MC.sphere_mesh()
    mesh = _mesh(v, t)
    H, W = 24, 32
    cams = [render.Camera.look_at(eye, MC.SPHERE_CENTRE, (0.0, -1.0, 0.0), 40.0, 40.0, H, W, near=0.5, far=100.0) for eye in (MC.OUTSIDE_EYE, MC.OBLIQUE_EYE)]
    l1, n = evaluate.mesh_depth_l1("cuda:0", mesh, mesh, cams, H, W, method="rays")
    assert l1 == 0.0 and 200 < n < 2 * H * W
    assert evaluate.mesh_depth_l1("cuda:0", mesh, mesh, cams, H, W) == evaluate.mesh_depth_l1("cuda:0", mesh, mesh, cams, H, W, method="raster")
    # against a copy moved by 1/4 along the first camera's axis: the restatement's two depth maps, pixel by pixel
    from vista_slam_amd import meshdist
    vm = v + np.array([0, 0, 0.25], dtype=np.float32)
    l1m, nm = evaluate.mesh_depth_l1("cuda:0", mesh, _mesh(vm, t), cams[:1], H, W, method="rays")
    o, d = [a.numpy() for a in meshdist.camera_rays(cams[0], H, W)]
    da, db = [RC.brute(D.Index(x, t), o, d, 0.5, 100.0)[0].astype(np.float32).astype(np.float64) for x in (v, vm)]
    both = np.isfinite(da) & np.isfinite(db)
    want = np.abs(da[both] - db[both]).sum() / both.sum()
    assert nm == both.sum() > 100 and abs(l1m - want) <= 1e-12 * want and 0.25 <= want < 0.5
    with pytest.raises(ValueError, match="method must be"):
        evaluate.mesh_depth_l1("cuda:0", mesh, mesh, cams, H, W, method="both")
