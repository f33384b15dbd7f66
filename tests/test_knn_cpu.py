"""Host only: the numpy restatement of include/sta_knn.h (tests/knn_cases.py) against independent statements - scipy's cKDTree and
cloud_cases.nn_brute for the lists, numpy.linalg.eigh for the Jacobi sweeps, the scalar-loop moments for the array ones -, the
measurement of its tolerances, and the conditions the filters and the normals must meet on the room with floaters and on the sphere.
The figures printed here are the ones written into knn_cases and into the docstrings below."""
import numpy as np
import pytest

import cloud_cases as CC
import knn_cases as KC


# ------------------------------------------------------------------------------------------ the lists
@pytest.mark.parametrize("k", [1, 7, 16])
def test_the_lists_equal_the_kdtree_on_tie_free_clouds(k):
    rng = np.random.default_rng(k)
    ref = rng.normal(0.0, 1.0, (1500, 3)).astype(np.float32)
    qry = rng.normal(0.0, 1.0, (300, 3)).astype(np.float32)
    d2, idx, cnt = KC.knn_brute(ref, qry, k, 0.35)
    kidx, kcnt = KC.knn_kdtree(ref, qry, k, 0.35)
    for row in d2:                                                 # tie-free: no list holds a distance twice
        f = row[np.isfinite(row)]
        assert len(np.unique(f)) == len(f)
    assert np.array_equal(cnt, kcnt) and np.array_equal(idx, kidx)
    assert 0 < (cnt < k).sum() < len(cnt) or k == 1              # both full and sparse neighbourhoods are in the case


def test_k_1_is_the_nearest_neighbour_of_the_cloud_contract():
    for name in ("duplicates_and_lattice_ties", "nan_and_inf", "far_queries", "m257", "at_the_radius", "one_step_beyond_the_radius"):
        c = CC.CASES[name]()
        d2, idx, _q = CC.nn_brute(c["ref"], c["qry"], None, c["radius"])
        k2, kidx, cnt = KC.knn_brute(c["ref"], c["qry"], 1, c["radius"])
        assert np.array_equal(k2[:, 0], d2) and np.array_equal(kidx[:, 0], idx) and np.array_equal(cnt, (idx >= 0).astype(np.int32)), name


def test_order_ties_self_and_padding():
    ref = KC.dyadic_lattice(257, 41)
    d2, idx, cnt = KC.knn_brute(ref, ref, 7, 1.0)
    s2, sidx, scnt = KC.knn_brute(ref, ref, 7, 1.0, self_base=0)
    rows = np.arange(257)
    assert (d2[:, 0] == 0).all() and not (sidx == rows[:, None]).any()
    for a2, ai, ac in ((d2, idx, cnt), (s2, sidx, scnt)):
        for i in range(257):
            c = ac[i]
            pairs = list(zip(a2[i, :c].tolist(), ai[i, :c].tolist()))
            assert pairs == sorted(pairs) and (a2[i, c:] == np.inf).all() and (ai[i, c:] == -1).all()
    assert (np.diff(d2, axis=1) == 0).any()          # the case has equal distances inside its lists
    # chunks of 100 with self_base give the whole
    parts = [KC.knn_brute(ref, ref[s:s + 100], 7, 1.0, self_base=s) for s in range(0, 257, 100)]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), sidx) and np.array_equal(np.concatenate([p[0] for p in parts]), s2)


# ------------------------------------------------------------------------------------------ the moments
def _room_lists(k=8, radius=0.6):
    pts, floater = KC.room_with_floaters()
    return pts, floater, KC.knn_brute(pts, pts, k, radius)


def test_the_array_moments_are_the_scalar_loops():
    pts, _fl, (d2, idx, cnt) = _room_lists()
    view = np.array([2.0, 1.5, 1.25])
    cases = [(pts, d2, idx, cnt, None), (pts, d2, idx, cnt, view), (pts, d2, idx, cnt, (pts + np.float32(0.25)))]
    lat = KC.dyadic_lattice(200, 3)
    cases.append((lat, *KC.knn_brute(lat, lat, 16, 0.5), None))
    for ref, a2, ai, ac, v in cases:
        ai = ai.copy()
        ai[5, 2] = len(ref) + 3                      # an index outside [0, M) ends the list there
        mo = KC.moments(ref, ref, a2, ai, ac, v)
        ref64 = ref.astype(np.float64)
        for i in list(range(0, len(ref), 37)) + [5]:
            vi = None if v is None else (v if np.ndim(v) == 1 else v[i].astype(np.float64))
            n, curv, md, c = KC.moments_one(ref64, ref64[i], a2[i], ai[i], ac[i], ai.shape[1], vi, KC.MIN_COUNT)
            assert np.array_equal(n, mo["normal"][i], equal_nan=True) and c == mo["c"][i], i
            assert np.array_equal(curv, mo["curv"][i], equal_nan=True) and md == mo["mean_dist"][i], i
        assert mo["c"][5] == 2 and np.isnan(mo["normal"][5]).all()


def _covariances():
    out = []
    for pts, k, r in ((KC.room_with_floaters()[0], 8, 0.6), (KC.sphere(), 16, 0.5)):
        d2, idx, cnt = KC.knn_brute(pts, pts, k, r)
        p = pts.astype(np.float64)
        for i in np.flatnonzero(cnt >= 3)[::3]:
            nb = p[idx[i, :cnt[i]]]
            d = nb - nb.mean(axis=0)
            out.append(d.T @ d)
    return out


def test_jacobi_against_eigh():
    """Measured: eigenvalues 1.15e-15 of the largest eigenvalue, eigenvector of l0 5.73e-15 (sine of the angle, gap >= 1e-3 l2); asserted
    at 16 times the recorded constants of knn_cases."""
    worst_l, worst_v = 0.0, 0.0
    for A in _covariances():
        l, V = KC.jacobi(A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2])
        w, E = np.linalg.eigh(A)
        rk = KC.ranks(l)
        mine = np.array([KC._pick(rk, l, r) for r in range(3)])
        if w[2] <= 0:
            continue
        worst_l = max(worst_l, float(np.abs(mine - w).max() / w[2]))
        if w[1] - w[0] >= 1e-3 * w[2]:
            e = np.array([KC._pick(rk, V[a], 0) for a in range(3)])
            worst_v = max(worst_v, float(np.linalg.norm(np.cross(e / np.linalg.norm(e), E[:, 0]))))
    print(f"[knn cpu] jacobi vs eigh: eigenvalues {worst_l:.2e} of l2, eigenvector of l0 {worst_v:.2e}")
    assert worst_l <= 16 * KC.TOL_EIG_MEASURED and worst_v <= 16 * KC.TOL_VEC_MEASURED


def test_the_record_and_its_tolerance():
    """Measured: the spread of a record entry between the three summation orders, relative to the sum of |contributions|, 1.49e-15."""
    worst = 0.0
    for name, ref, _qry, _T, radius in CC.hostile_cases():
        d2, idx, cnt = KC.knn_brute(ref, ref, 16, 3 * radius, self_base=0)
        mo = KC.moments(ref, ref, d2, idx, cnt)
        con = KC.contributions(mo["mean_dist"], mo["c"])
        sums = [CC.sum_rows(con, o) for o in KC.ORDERS]
        scale = np.abs(con).sum(axis=0)
        for s in sums[1:]:
            assert np.array_equal(s[[0, 3]], sums[0][[0, 3]])                 # the counts are exact in every order
            worst = max(worst, float((np.abs(s - sums[0])[1:3] / scale[1:3]).max()))
        assert sums[0][0] == (cnt >= 1).sum() and sums[0][3] == (mo["c"] >= 3).sum() and (sums[0][4:] == 0).all()
    print(f"[knn cpu] record: spread between summation orders {worst:.2e} of the sum of |contributions|")
    assert worst <= KC.TOL_SUM_MEASURED
    # dyadic inputs whose distances are dyadic too: every order gives the same bits
    line = (np.arange(64)[:, None] * np.array([[0.25, 0.0, 0.0]])).astype(np.float32)
    d2, idx, cnt = KC.knn_brute(line, line, 2, 0.25, self_base=0)
    mo = KC.moments(line, line, d2, idx, cnt)
    con = KC.contributions(mo["mean_dist"], mo["c"])
    assert all(np.array_equal(CC.sum_rows(con, o), CC.sum_rows(con)) for o in KC.ORDERS) and CC.sum_rows(con)[1] == 16.0


# ------------------------------------------------------------------------------------------ the conditions
def test_statistical_filter_on_the_room_with_floaters():
    """nb 16, ratio 2.0, radius 1.0.  Measured on the restatement: all 40 floaters and 6 of the 2000 room points removed."""
    pts, floater = KC.room_with_floaters()
    kept, mask, _md, rec = KC.remove_statistical_outlier(pts, 16, 2.0, 1.0)
    gone_room = int((~mask[~floater]).sum())
    print(f"[knn cpu] statistical filter: removed {int((~mask[floater]).sum())} of 40 floaters and {gone_room} of 2000 room points; record {rec[:4]}")
    assert not mask[floater].any() and gone_room <= 20
    assert np.array_equal(kept, np.flatnonzero(mask)) and kept.dtype == np.int64
    for order in KC.ORDERS[1:]:                      # the kept set does not hang on the last bits of the two sums
        assert np.array_equal(KC.remove_statistical_outlier(pts, 16, 2.0, 1.0, order=order)[1], mask)


def test_radius_filter_on_the_room_with_floaters():
    """radius 0.4, nb 4.  Measured on the restatement: all 40 floaters and 0 room points removed."""
    pts, floater = KC.room_with_floaters()
    kept, mask = KC.remove_radius_outlier(pts, 4, 0.4)
    print(f"[knn cpu] radius filter: removed {int((~mask[floater]).sum())} of 40 floaters and {int((~mask[~floater]).sum())} of 2000 room points")
    assert not mask[floater].any() and mask[~floater].all() and np.array_equal(kept, np.arange(2000))


def test_normals_of_the_room_and_the_sphere():
    """Measured on the restatement: room, k = 8, every point at least 0.5 from an edge within 1e-3 degrees of its wall's axis (asserted at
    0.01); 3000 points of the unit sphere (default_rng(3)), k = 16 with the point itself, worst angle to the radial direction 5.25 degrees
    (asserted at 6)."""
    room = CC.box_room(2000, 0)
    n, curv = KC.estimate_normals(room, 8, 1.0)
    rows, axis = KC.wall_axis(room, 0.5)
    assert len(rows) > 500 and not np.isnan(n[rows]).any()
    ang = KC.angle_deg(n[rows], np.eye(3)[axis])
    print(f"[knn cpu] room normals: {len(rows)} inner points, worst angle to the wall's axis {ang.max():.2e} degrees, largest curvature {np.abs(curv[rows]).max():.2e}")
    assert ang.max() <= 0.01
    big = np.abs(n[rows].astype(np.float64))[np.arange(len(rows)), axis]
    assert (n[rows][np.arange(len(rows)), axis] > 0).all() and (big > 0.999).all()          # the largest component is positive
    # towards a viewpoint inside the room every wall's normal points inwards
    nv, _ = KC.estimate_normals(room, 8, 1.0, view=np.array([2.0, 1.5, 1.25]))
    inward = np.where(room[rows, axis] == 0.0, 1.0, -1.0)
    assert (np.sign(nv[rows][np.arange(len(rows)), axis]) == inward).all()
    sph = KC.sphere()
    ns, _ = KC.estimate_normals(sph, 16, 0.5, view=np.zeros(3))
    assert not np.isnan(ns).any()
    ang = KC.angle_deg(ns, sph)
    print(f"[knn cpu] sphere normals: worst angle to the radial direction {ang.max():.2f} degrees")
    assert ang.max() <= 6.0
    assert ((ns.astype(np.float64) * sph).sum(axis=1) < 0).all()                            # ... towards the centre


def test_plan_and_refusals_of_the_python_layer():
    from vista_slam_amd import cloud
    for M, Q, k in ((1, 1, 1), (100, 257, 64), ((1 << 30) - 1, 1 << 20, 30), (5, 256 * 2048 + 1, 7)):
        assert tuple(cloud.knn_plan(M, Q, k)) == KC.plan(M, Q, k)
    for M, Q, k in ((0, 1, 1), (1 << 30, 1, 1), (1, 0, 1), (1, 1 << 30, 1), (1, 1, 0), (1, 1, 65)):
        with pytest.raises(ValueError) as a:
            cloud.knn_plan(M, Q, k)
        with pytest.raises(ValueError) as b:
            KC.plan(M, Q, k)
        assert str(a.value) == str(b.value)
        with pytest.raises(ValueError, match=r"knn: (M|Q|k) must be in"):
            cloud.knn_check(M, Q, k)
    assert cloud.knn_check(10, 10, 8, 4.0, 0.125) == 4.0 and cloud.knn_check(10, 10, 8, 0.0, 1.0, min_count=3) == 0.0
    assert cloud.MAX_RINGS == KC.MAX_RINGS and cloud.KNN_MAX_K == KC.MAX_K and cloud.KNN_RECORD == KC.RECORD and cloud.KNN_MIN_COUNT == KC.MIN_COUNT
    for r in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="knn_query: radius must be finite and >= 0"):
            cloud.knn_check(10, 10, 8, r, 1.0)
    with pytest.raises(ValueError, match="is more than 32 cells"):
        cloud.knn_check(10, 10, 8, np.nextafter(4.0, 5.0), 0.125)
    with pytest.raises(ValueError, match="min_count must be at least 3 .got 2."):
        cloud.knn_check(10, 10, 8, min_count=2)
    assert cloud.knn_chunk_rows(64) == 349440 and cloud.knn_chunk_rows(64) * 64 * 12 <= cloud.KNN_LIST_BYTES and cloud.knn_chunk_rows(1) % 256 == 0
    with pytest.raises(ValueError, match="outlier must be"):
        cloud.filter_outliers(np.zeros((4, 3), np.float32), ("median", 3))
