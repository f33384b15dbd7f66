"""GPU: libsta_dist.so through vista_slam_amd/meshdist.py against tests/dist_cases.py, the numpy restatement of include/sta_dist.h.  Every
comparison is array_equal: the counters, the sorted order, the sorted coordinates, every level's boxes, and d2, tri and point of every
query against the brute force over all valid triangles.  The shapes are the smallest at which the code can go wrong: triangle counts
around the powers of the fan-out, query counts around the wavefront, ties, invalid triangles, equal keys, hostile magnitudes."""
import math

import numpy as np
import pytest

import dist_cases as D

pytestmark = pytest.mark.gpu
F = D.FANOUT


def _mesh(v, t):
    import torch
    from vista_slam_amd import tsdf
    return tsdf.Mesh(torch.from_numpy(np.array(v)).cuda(), None, torch.from_numpy(np.array(t)).cuda())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def check_build(v, t):
    """build on the device and in numpy; the counters, the order, the coordinates and every level's boxes must be equal -> (gpu, numpy)"""
    from vista_slam_amd import meshdist
    ref = D.Index(v, t)
    idx = meshdist.TriIndex.build(_mesh(v, t))
    assert (idx.nt, idx.levels) == (ref.nt, len(ref.counts))
    assert idx.level_offset[:idx.levels + 1] == np.concatenate([[0], np.cumsum(ref.counts)]).tolist()
    assert _same(idx.counters.cpu().numpy(), ref.counters), (idx.counters.cpu().numpy(), ref.counters)
    assert _same(idx.src.cpu().numpy(), ref.src)
    assert _same(idx.tri.cpu().numpy(), ref.tri)
    for level, boxes in enumerate(ref.boxes):
        assert _same(idx.level_boxes(level).cpu().numpy(), boxes), level
    return idx, ref


def check(v, t, q, radius=math.inf, ref_answer=None):
    """build and query on the device and in numpy: everything equal, the status bit 0 -> (d2, tri, point) of the restatement"""
    import torch
    idx, ref = check_build(v, t)
    want = D.brute(ref, q, radius) if ref_answer is None else ref_answer
    d2, tri, point = idx.query(torch.from_numpy(np.array(q)).cuda(), radius)
    got = (d2.cpu().numpy(), tri.cpu().numpy(), point.cpu().numpy())
    for name, g, w in zip(("d2", "tri", "point"), got, want):
        bad = np.nonzero(~((g == w) | ((g != g) & (w != w))).reshape(len(q), -1).all(axis=1))[0]
        assert _same(g, w), f"{name}: {len(bad)} of {len(q)} queries differ, first {bad[:1]}: got {g[bad[:1]]}, restatement {w[bad[:1]]}"
    assert _same(idx.counters.cpu().numpy(), ref.counters) and int(idx.counters[4]) == 0, "the status bit stays 0"
    return want


@pytest.mark.parametrize("nt", [1, F - 1, F, F + 1, F * F, F * F + 1, F ** 3 + 1])
def test_triangle_counts_around_the_powers_of_the_fan_out(nt):
    v, t = D.soup(nt, seed=nt)
    q = D.soup_queries(65, seed=nt + 1)
    for radius in (math.inf, 0.25):
        check(v, t, q, radius)


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 1000])
def test_query_counts_around_the_wavefront(Q):
    v, t = D.soup(F ** 3 + 1, seed=2)
    check(v, t, D.soup_queries(Q, seed=Q), 0.3)
    check(v, t, D.soup_queries(Q, seed=Q))


def test_one_triangle_all_seven_regions_and_their_borders():
    v, t = D.one_triangle()
    d2, tri, pt = check(v, t, D.regions())
    assert (tri == 0).all() and (pt[:, 2] == 0).all()


def test_equidistant_triangles_the_lowest_index_wins():
    v, t = D.lattice()
    q = D.lattice_queries()
    _d2, tri, _pt = check(v, t, q)
    # above the interior vertex (2, 2) of the 4 x 4 grid six triangles meet; the answer is the lowest of them
    centre = np.nonzero((q[:, 0] == 0.5) & (q[:, 1] == 0.5))[0]
    six = np.nonzero((t == 2 * 5 + 2).any(axis=1))[0]
    assert len(six) == 6 and (tri[centre] == six.min()).all()
    v2, t2 = D.reversed_duplicated(v, t)
    _d2, tri2, _pt = check(v2, t2, q)
    assert (tri2 < len(t)).all(), "of a triangle and its reversed copy the lower index is the copy"
    # the same under a permutation that changes which index is lowest
    perm = np.random.default_rng(1).permutation(len(t2))
    check(v2, t2[perm], q)


def test_invalid_triangles_are_counted_and_never_returned():
    v, t = D.with_bad(*D.lattice())
    q = np.concatenate([D.lattice_queries(), D.soup_queries(100, 3, 2.0)])
    _d2, tri, _pt = check(v, t, q)
    cls = D.classify(v, t)
    assert (cls[tri] == D.VALID).all() and set(np.unique(cls)) == {0, 1, 2, 3}


def test_a_mesh_without_a_valid_triangle_matches_nothing():
    v, t = D.with_bad(*D.lattice())
    bad = t[D.classify(v, t) != D.VALID]
    for tris in (bad, bad[:1], bad[:F + 1]):
        d2, tri, pt = check(v, tris, D.lattice_queries())
        assert np.isposinf(d2).all() and (tri == -1).all() and np.isnan(pt).all()


def test_radius_is_inclusive_zero_and_infinite():
    from vista_slam_amd import meshdist
    import torch
    v, t = D.one_triangle()
    q = np.array([[1, 1, 3], [0, 0, 0], [4, 0, 0], [1, 1, 0], [0, 0, 1]], dtype=np.float32)
    d2, tri, _ = check(v, t, q, 3.0)
    assert d2[0] == 9.0 and tri[0] == 0, "a query exactly at the radius is matched"
    d2, tri, _ = check(v, t, q, float(np.nextafter(3.0, 0.0)))
    assert d2[0] == np.inf and tri[0] == -1 and tri[4] == 0, "a float64 step beyond the radius is not"
    d2, tri, _ = check(v, t, q, 0.0)
    assert tri.tolist() == [-1, 0, 0, 0, -1] and (d2[1:4] == 0).all()
    d2, tri, _ = check(v, t, (q * np.float32(1e18)), math.inf)
    assert (tri == 0).all() and np.isfinite(d2).all()
    idx = meshdist.TriIndex.build(_mesh(v, t))
    for radius in (-1.0, -0.0 - 1e-300, float("nan")):
        with pytest.raises(ValueError, match="tri_query: radius"):
            idx.query(torch.from_numpy(np.array(q)).cuda(), radius)
    with pytest.raises(ValueError, match="want"):
        idx.query(torch.from_numpy(np.array(q)).cuda(), want=("d2", "normal"))
    with pytest.raises(ValueError, match=r"tri_query: Q must be in \[1, 2\^30\) \(got 0\)"):
        idx.query(torch.zeros(0, 3).cuda())
    (only,) = idx.query(torch.from_numpy(np.array(q)).cuda(), 3.0, want=("tri",))
    assert only.cpu().numpy().tolist() == [0, 0, 0, 0, 0]


def test_queries_that_are_not_finite_are_unmatched():
    v, t = D.soup(F * F + 1, seed=5)
    q = D.soup_queries(70, seed=6)
    q[3, 0], q[10, 1], q[64, 2], q[65] = np.nan, np.inf, -np.inf, np.nan
    d2, tri, pt = check(v, t, q)
    for i in (3, 10, 64, 65):
        assert d2[i] == np.inf and tri[i] == -1 and np.isnan(pt[i]).all()
    assert (np.delete(tri, [3, 10, 64, 65]) >= 0).all()


def test_one_room_sized_triangle_among_small_ones():
    v, t = D.room()
    q = np.concatenate([D.soup_queries(200, 7), D.soup_queries(100, 8, 20.0, -8.0)])
    _d2, tri, _pt = check(v, t, q)
    big = len(t) // 2
    assert (tri == big).any() and (tri != big).any()


def test_equal_keys_a_planar_mesh_and_hostile_magnitudes():
    v, t = D.same_centre()
    idx, ref = check_build(v, t)
    assert len(np.unique(ref.key)) == 1 and np.array_equal(ref.src, np.arange(len(t)))
    check(v, t, D.soup_queries(200, 5, 8.0, -4.0))
    v, t = D.lattice(9, 0.125)                     # planar: U == L on z; 162 triangles, three levels
    ref = check_build(v, t)[1]
    assert len(ref.counts) == 3
    check(v, t, D.soup_queries(200, 9, 1.5), 0.4)
    v, t = D.soup(300, 2, 1.0, 0.2, 1.0e6)         # coordinates near 1e6
    check(v, t, D.soup_queries(200, 3, 1.0, 1.0e6))
    check(v, t, D.soup_queries(200, 3, 1.0, 1.0e6), 0.05)
    v, t = D.hostile_soup()
    check(v, t, D.hostile_queries())
    check(v, t, D.hostile_queries(), 1.0e3)


def test_three_spheres_with_2000_queries():
    v, t, q, ans = D.spheres_case()
    check(v, t, q, ref_answer=ans)
    r2 = 0.5 * 0.5
    near = (np.where(ans[0] <= r2, ans[0], np.inf), np.where(ans[0] <= r2, ans[1], -1).astype(np.int32),
            np.where((ans[0] <= r2)[:, None], ans[2], np.float32(np.nan)))
    assert 100 < (near[1] >= 0).sum() < 1900
    check(v, t, q, 0.5, ref_answer=near)             # within a radius the answer is the unrestricted one or nothing


def test_two_builds_and_two_queries_give_identical_bits():
    import torch
    from vista_slam_amd import meshdist
    v, t, q, _ans = D.spheres_case()
    mesh, qd = _mesh(v, t), torch.from_numpy(np.array(q)).cuda()
    a, b = meshdist.TriIndex.build(mesh), meshdist.TriIndex.build(mesh)
    for x, y in ((a.tri, b.tri), (a.src, b.src), (a.boxes, b.boxes), (a.counters, b.counters)):
        assert _same(x.cpu().numpy(), y.cpu().numpy())
    one, two, other = a.query(qd, 2.0), a.query(qd, 2.0), b.query(qd, 2.0)
    for x, y, z in zip(one, two, other):
        assert _same(x.cpu().numpy(), y.cpu().numpy()) and _same(x.cpu().numpy(), z.cpu().numpy())
    pm = meshdist.point_to_mesh(qd, mesh, 2.0)
    for x, y in zip(one, pm):
        assert _same(x.cpu().numpy(), y.cpu().numpy())
    assert int(a.counters[4]) == 0 and int(b.counters[4]) == 0
