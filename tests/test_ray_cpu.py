"""Host only: tests/ray_cases.py, the numpy restatement of include/sta_ray.h, against a second, independent statement (Moeller-Trumbore
in numpy.longdouble) on hits that lie inside their triangle; the containment chain of the header's rule 6, exactly, on hostile floats;
the no-leak property of the sheared triangle test on closed meshes; and every refusal of libsta_ray.so through vista_slam_amd.meshdist."""
import numpy as np
import pytest

import dist_cases as D
import mesh_cases as MC
import ray_cases as RC

f32, f64, ld = np.float32, np.float64, np.longdouble


def moeller_trumbore(o, d, A, B, Cc):
    """(t, weights of A, B, C) in numpy.longdouble: the 3-D form with cross products, nothing shared with the sheared form"""
    o, d, A, B, Cc = (np.asarray(x, dtype=f32).astype(ld) for x in (o, d, A, B, Cc))
    e1, e2 = B - A, Cc - A
    p = np.cross(d, e2)
    det = (e1 * p).sum(axis=-1)
    tv = o - A
    u = (tv * p).sum(axis=-1) / det
    q = np.cross(tv, e1)
    v = (d * q).sum(axis=-1) / det
    return (e2 * q).sum(axis=-1) / det, np.stack([1 - u - v, u, v], axis=-1)


SECOND_CASES = [(2, 1.3, (0, 0, 0)), (2, 4.4, (0, 0, 0)), (2, 1e-3, (0, 0, 0)), (2, 1000.0, (5000, -3000, 100)), (1, 1e4, (0, 0, 0)), (2, 0.25, (-3, 2, 40))]


def test_the_restatement_agrees_with_moeller_trumbore_in_extended_precision():
    worst, worst_b, n = 0.0, 0.0, 0
    for level, scale, offset in SECOND_CASES:
        v, t = RC.icosphere(level, scale, offset)
        index = D.Index(v, t)
        for origin in (np.zeros(3), np.array([0.3, -0.2, 0.4])):
            o = (origin * scale + np.asarray(offset)).astype(f32)
            dirs = (np.random.default_rng(level).standard_normal((1500, 3)) * scale * 0.01).astype(f32)          # not normalised: t is large
            tc, tri, bary, _occ = RC.brute(index, o, dirs)
            assert (tri >= 0).all()
            P = D.corners(v, t[tri])
            t2, w2 = moeller_trumbore(o, dirs, P[:, 0], P[:, 1], P[:, 2])
            inside = (w2 >= RC.SECOND_STATEMENT_MARGIN).all(axis=1)
            assert inside.sum() > 1000
            rel = np.abs(tc.astype(ld) - t2) / np.maximum(np.abs(t2), ld(1e-300))
            worst, worst_b, n = max(worst, float(rel[inside].max())), max(worst_b, float(np.abs(bary.astype(ld) - w2)[inside].max())), n + int(inside.sum())
    print(f"[ray second statement] {n} hits: largest relative difference of t {worst:.3g}, largest difference of a weight {worst_b:.3g}")
    assert worst <= RC.SECOND_STATEMENT_FACTOR * RC.SECOND_STATEMENT_MEASURED
    assert worst_b <= 2.0 ** -23          # the weights are float32 in [0, 1]: one rounding, half a step of 2^-23 at the most, plus the above


def chain_cases():
    v, t = RC.hostile_mesh()
    yield "hostile", v, t, RC.hostile_rays(600, 10, v), (0.0, np.inf)
    yield "hostile, bounded", v, t, RC.hostile_rays(600, 12, v), (0.5, 2.0)
    v, t = D.soup(300, 2)
    o, d = RC.soup_rays(500, 3)
    d[::5, 0] = 0
    d[1::9, 1:] = 0
    yield "soup", v, t, (o, d), (0.0, np.inf)
    yield "soup, a segment", v, t, (o, d), (0.25, 1.0)
    v, t = D.room()
    yield "room", v, t, RC.soup_rays(400, 5), (0.0, 4.0)


@pytest.mark.parametrize("case", list(chain_cases()), ids=lambda c: c[0])
def test_the_containment_chain_holds_exactly(case):
    """rule 6: for every pair of a ray and a qualifying triangle, every node above the triangle passes rule 2 and
    enter_node <= enter_own <= t_c <= exit_own <= exit_node in the computed values - no margin"""
    _name, v, t, (o, d), (t_min, t_max) = case
    index = D.Index(v, t)
    n = index.n_valid
    T = index.tri[:n].reshape(n, 3, 3)
    use = RC.usable(o, d)
    o, d = o[use], d[use]
    q, tc, _b, enter, exit_, _t, _h = RC.qualify(o[:, None], d[:, None], T[None, :, 0], T[None, :, 1], T[None, :, 2], t_min, t_max)
    assert q.sum() >= 100, q.sum()
    assert ((enter <= tc) & (tc <= exit_))[q].all()
    assert ((f64(t_min) <= tc) & (tc <= f64(t_max)))[q].all()
    for level, anc in enumerate(RC.ancestors(index)):
        box = index.boxes[level][anc]          # [n, 6]
        assert (box[:, :3] <= T.min(axis=1)).all() and (box[:, 3:] >= T.max(axis=1)).all()
        p, en, ex = RC.slab(o[:, None], d[:, None], box[None, :, :3], box[None, :, 3:], t_min, t_max)
        assert p[q].all(), (level, int((~p[q]).sum()))
        assert (en <= enter)[q].all() and (exit_ <= ex)[q].all(), level
    # ... so the brute force over the qualifying pairs is what a search that skips a node with enter_node > best finds
    want = RC.brute(index, o, d, t_min, t_max)
    m = np.where(q, tc, np.inf).min(axis=1)
    assert np.array_equal(np.where(q.any(axis=1), m, np.inf), want[0])


def closed_meshes():
    v, t, _ = MC.sphere_mesh()
    c = MC.SPHERE_CENTRE
    yield "tsdf sphere", v, t, [c, c + np.array([1.0, 2.0, -2.0])]
    v, t = RC.icosphere(3, 1.3)
    yield "icosphere", v, t, [np.zeros(3), np.array([0.4, -0.3, 0.5])]


@pytest.mark.parametrize("case", list(closed_meshes()), ids=lambda c: c[0])
def test_no_ray_leaks_through_a_closed_mesh(case):
    """every ray from two interior origins towards every vertex, every edge midpoint, every edge 1/4 point, 2000 random directions and
    nine axis / diagonal ones has a qualifying triangle: 0 misses.  A condition, not a measurement."""
    _name, v, t, origins = case
    index = D.Index(v, t)
    assert index.n_valid == len(t)
    for k, origin in enumerate(origins):
        o = np.asarray(origin, dtype=f32)
        d = RC.aimed_dirs(v, t, o, 2000, seed=k)
        tc, tri, bary, occ = RC.brute(index, o, d)
        assert (tri >= 0).all(), int((tri < 0).sum())
        assert np.isfinite(tc).all() and (tc > 0).all() and occ.all() and np.isfinite(bary).all()


def test_the_own_box_must_be_widened_and_the_clamp_rarely_moves():
    """what the header's rule 4 is there for, counted on one case: with the own box as it is, accepted triangles are lost"""
    v, t = RC.icosphere(3, 1.3)
    o = np.zeros(3, dtype=f32)
    d = RC.aimed_dirs(v, t, o, 500)
    P = D.corners(v, t)
    lost = moved = rejected = 0
    for s in range(0, len(d), 256):
        args = (o, d[s:s + 256, None], P[None, :, 0], P[None, :, 1], P[None, :, 2])
        q, tc, _b, _e, _x, traw, hit = RC.qualify(*args)
        q0 = RC.qualify(*args, widened=False)[0]
        lost += int((q & ~q0).sum())
        moved += int((q & (tc != traw)).sum())
        rejected += int((hit & (traw >= 0) & ~q).sum())
    print(f"[ray own box] lost without widening {lost}, answers moved by the clamp {moved}, rule-3 hits rejected by the widened own box {rejected}")
    assert lost > 0 and rejected == 0


def test_every_refusal_is_the_librarys_and_in_its_words():
    from vista_slam_amd import build, meshdist
    build.build_lib()
    assert meshdist.ray_plan(6372, 3000) == RC.plan(6372, 3000)[0] == 913
    for nt in (1, 7, 8, 9, 64, 65, 513, (1 << 27) - 1):
        assert meshdist.ray_plan(nt) == sum(D.level_counts(nt)) == sum(meshdist.level_counts(nt))
    for nt, R in ((0, 1), (-3, 1), (1 << 27, 1), (5, 0), (5, -1), (5, 1 << 30)):
        with pytest.raises(ValueError) as mine:
            RC.plan(nt, R)
        with pytest.raises(ValueError) as theirs:
            meshdist.ray_plan(nt, R)
        assert str(mine.value) == str(theirs.value) and str(nt if not 1 <= nt < 1 << 27 else R) in str(mine.value)
        for occluded, who in ((False, "ray_cast"), (True, "ray_occluded")):
            with pytest.raises(ValueError) as theirs:
                meshdist.ray_check(nt, R, occluded=occluded)
            assert str(theirs.value) == str(mine.value).replace("ray_plan", who)
    nan = float("nan")
    for t_min, t_max in ((-1.0, 1.0), (-0.5, np.inf), (2.0, 1.0), (np.inf, 1.0), (nan, 1.0), (0.0, nan), (nan, nan), (0.0, -1.0)):
        for occluded, who in ((False, "ray_cast"), (True, "ray_occluded")):
            with pytest.raises(ValueError) as mine:
                RC.check_range(who, t_min, t_max)
            with pytest.raises(ValueError) as theirs:
                meshdist.ray_check(5, 5, t_min, t_max, occluded=occluded)
            assert str(mine.value) == str(theirs.value) and str(mine.value).startswith(who + ": 0 <= t_min <= t_max is required")
    for t_min, t_max in ((0.0, 0.0), (0.0, np.inf), (3.0, 3.0), (np.inf, np.inf)):
        meshdist.ray_check(5, 5, t_min, t_max)
        meshdist.ray_check(5, 5, t_min, t_max, occluded=True)
        RC.check_range("ray_cast", t_min, t_max)
    # null arguments: the plan's, and a call without its buffers
    import ctypes as C
    from vista_slam_amd import _lib
    lib = _lib.load_ray()
    assert lib.sta_ray_plan(5, 5, None) == -1 and lib.sta_ray_last_error() == b"ray_plan: null argument"
    assert lib.sta_ray_cast(None, None, None, None, 5, None, None, 5, 0.0, 1.0, None, None, None, None, None) == -1
    assert lib.sta_ray_last_error() == b"ray_cast: null argument"
    assert lib.sta_ray_occluded(None, None, None, None, 5, None, None, 5, 0.0, 1.0, None, None, None) == -1
    assert lib.sta_ray_last_error() == b"ray_occluded: null argument"
    # the shapes the Python layer refuses before anything reaches the device
    z = np.zeros
    for o, d in ((z(3), z(3)), (z((4, 3)), z((5, 3))), (z(2), z((5, 3))), (z((5, 3)), z((5, 2))), (z((5, 3)), z((1, 5, 3)))):
        with pytest.raises(ValueError):
            meshdist._rays(o, d, None)
    o, d = meshdist._rays(np.arange(3.0), z((5, 3)), None)
    assert tuple(o.shape) == tuple(d.shape) == (5, 3) and o.is_contiguous() and o[4].tolist() == [0.0, 1.0, 2.0]
    assert meshdist.RAY_WANT == ("t", "tri", "bary") and meshdist.RAY_STATUS_BOUND == RC.STATUS_BOUND == 1


def test_camera_rays_are_row_major_with_unit_camera_depth():
    from vista_slam_amd import meshdist, render
    H, W = 5, 7
    cam = render.Camera.look_at((1.0, 2.0, -3.0), (0.5, 0.0, 4.0), (0.0, -1.0, 0.0), 6.0, 5.0, H, W)
    o, d = meshdist.camera_rays(cam, H, W)
    assert o.dtype == d.dtype and str(o.dtype) == "torch.float32" and tuple(o.shape) == (3,) and tuple(d.shape) == (H * W, 3)
    R, tv = cam.w2c[:, :3], cam.w2c[:, 3]
    assert np.abs(R @ o.numpy().astype(f64) + tv).max() < 1e-6
    dc = d.numpy().astype(f64) @ R.T          # back in the camera
    fx, fy, cx, cy = cam.K
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    want = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones((H, W))], axis=-1).reshape(-1, 3)
    assert np.abs(dc - want).max() < 1e-6 and np.abs(dc[:, 2] - 1).max() < 1e-6
