"""Host only: tests/reg_cases.py, the numpy restatement of include/sta_reg.h and of meshdist.plane_step / icp, against second statements -
the search against dist_cases.brute, the Jacobian row against central differences, H and g against dense products, the first twenty
entries of the record against cloud_cases.contributions, the degenerate directions of a single wall, the recovery of known motions - and
the measurement of the tolerances that reg_cases.py carries."""
import numpy as np
import pytest

import cloud_cases as CC
import dist_cases as DC
import reg_cases as RG

EPS = 2.0 ** -52


def _general():
    """the room under a general rotation: (index, pass, T, pivot)"""
    v, t = DC.room()
    idx = DC.Index(v, t)
    T, pivot = RG.TRANSFORMS["rotation"](), np.array([0.4, 0.5, 0.45])
    return idx, RG.pass_(idx, DC.soup_queries(300, seed=3), T, 0.3, pivot=pivot), T, pivot


def test_the_search_on_doubles_is_the_search_of_dist_cases_wherever_the_query_is_a_float32():
    for (v, t), q in ((DC.room(), DC.soup_queries(300, 3)), (DC.hostile_soup(), DC.hostile_queries()), (DC.with_bad(*DC.lattice()), DC.lattice_queries()),
                      (DC.reversed_duplicated(*DC.lattice()), RG.poisoned(DC.lattice_queries()))):
        idx = DC.Index(v, t)
        P = DC.corners(idx.verts, idx.tris[idx.cls == DC.VALID])
        a, b = DC.closest(q[:, None], P[None, :, 0], P[None, :, 1], P[None, :, 2]), RG.closest(q.astype(np.float64)[:, None], P[None, :, 0], P[None, :, 1], P[None, :, 2])
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)
        for radius in (np.inf, 0.3, 0.0):
            want, got = DC.brute(idx, q, radius), RG.search(idx, q.astype(np.float64), radius)
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
            assert np.array_equal(want[2], got[2].astype(np.float32), equal_nan=True)


def test_plan_and_its_refusals():
    assert RG.plan(1, 1) == (1, 512) and RG.plan(9, 257) == (3, 1024) and RG.plan(513, 256 * 257 + 1) == (65 + 9 + 2 + 1, 258 * 512)
    for nt, Q, words in ((0, 1, "nt must be in [1, 2^27) (got 0)"), (1 << 27, 1, "(got 134217728)"), (1, 0, "Q must be in [1, 2^30) (got 0)"),
                         (1, 1 << 30, "(got 1073741824)")):
        with pytest.raises(ValueError, match="reg_plan") as e:
            RG.plan(nt, Q)
        assert words in str(e.value)


def test_J_is_the_derivative_of_r_under_a_twist_about_the_pivot():
    """r(omega, v) = dot(Exp(omega)(q' - pivot) + pivot + v - c, nhat) with c and nhat held; central differences with h = 1e-5 have a
    truncation error of h^2 / 6 times the third derivative (<= |x|) and a rounding error of about eps |q'| / h: both below 1e-9 (1 + |x|)
    for the room's coordinates of order 1."""
    _idx, p, _T, pivot = _general()
    M = np.nonzero(p["matched"])[0]
    assert len(M) > 100
    q, c, nhat, h = p["q"][M], p["c"][M], p["nhat"][M], 1e-5
    worst = 0.0
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rp, rm = [RG.dot(CC.apply_T(q, RG.twist_update(s * d[:3], s * d[3:], pivot)) - c, nhat) for s in (1.0, -1.0)]
        err = np.abs((rp - rm) / (2 * h) - p["J"][M, k]) / (1.0 + np.linalg.norm(q - pivot, axis=1))
        worst = max(worst, err.max())
    print(f"[reg cpu] J against central differences: {worst:.2e}")
    assert worst < 1e-9
    assert np.allclose(RG.dot(q - c, nhat), p["resid"][M], rtol=0, atol=0)


def test_H_and_g_are_the_dense_products_of_the_stacked_rows():
    """the record's sums in ascending order against BLAS products of the same rows: two orders of the same n terms differ by at most
    n eps sum |term|"""
    for p in (_general()[1], RG.pass_(DC.Index(*RG.hostile_case()[:2]), *RG.hostile_case()[2:])):
        M = p["matched"]
        rec, J, r, n = RG.record(p["terms"]), p["J"][M], p["resid"][M], int(M.sum())
        H, g = J.T @ J, J.T @ r
        sH, sg = np.abs(J).T @ np.abs(J), np.abs(J).T @ np.abs(r)
        assert (np.abs(RG.H_of(rec) - H) <= n * EPS * sH).all() and (np.abs(rec[23:29] - g) <= n * EPS * sg).all()
        assert abs(rec[21] - r @ r) <= n * EPS * (r @ r) and abs(rec[22] - np.abs(r).sum()) <= n * EPS * np.abs(r).sum()
        assert (rec[50:] == 0).all() and rec[1] == n


def test_the_first_twenty_entries_are_the_record_of_the_cloud_library():
    # where the closest points are float32 values (the dyadic case), cloud_cases.contributions fed the same matches gives the same rows
    v, t, q, T, pivot = RG.dyadic_case()
    qq = np.concatenate([RG.poisoned(q), q + np.float32(8.0)])          # NaN and inf, and queries out of reach
    p = RG.pass_(DC.Index(v, t), qq, T, 0.75, pivot=pivot)
    assert p["matched"].sum() > 100 and (~p["found"] & p["finite"]).sum() > 100 and (~p["finite"]).sum() > 10
    ref = np.where(p["found"][:, None], p["c"], 0.0).astype(np.float32)
    assert np.array_equal(ref.astype(np.float64)[p["found"]], p["c"][p["found"]])
    idx = np.where(p["found"], np.arange(len(qq)), -1).astype(np.int32)
    assert np.array_equal(p["terms"][:, :20], CC.contributions(ref, p["q"], p["d2"], idx, 0.75)[:, :20])
    # a general case: every entry that does not hold a closest point
    _idx, p, _T, _pivot = _general()
    con = CC.contributions(np.where(p["found"][:, None], p["c"], 0.0).astype(np.float32), p["q"], p["d2"], np.where(p["found"], np.arange(len(p["q"])), -1), 0.3)
    for k in (0, 1, 2, 3, 4, 5, 6, 19):
        assert np.array_equal(p["terms"][:, k], con[:, k]), k


def test_the_dyadic_case_is_exact():
    v, t, q, T, pivot = RG.dyadic_case()
    p = RG.pass_(DC.Index(v, t), q, T, np.inf, pivot=pivot)
    assert p["matched"].all() and (p["nhat"] == np.array([0.0, 0.0, 1.0])).all()
    recs = [RG.record(p["terms"], o) for o in RG.ORDERS]
    assert np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2])
    assert np.array_equal(p["resid"], p["q"][:, 2]) and recs[0][1] == len(q)


def test_a_single_wall_moves_the_scan_along_its_normal_and_about_the_in_plane_axes_only():
    """the plane z = 0: J = (x_y, -x_x, 0, 0, 0, 1), so H has no weight on the rotation about z and on the translations along x and y;
    eigh's vectors are orthonormal to a few eps, so what leaks into those directions is below 1e-14 of the step"""
    v, t = DC.lattice(4, 0.25)
    idx = DC.Index(v, t)
    q = DC.lattice_queries(4, 0.25)
    pivot = np.array([0.5, 0.5, 0.0])
    up = q.copy()
    up[:, 2] = 0.125
    U = RG.plane_step(RG.record(RG.pass_(idx, up, None, np.inf, pivot=pivot)["terms"]), pivot)
    assert np.abs(U - np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -0.125]])).max() < 1e-14
    # a tilted scan: the step turns about x and y and shifts along z, nothing else
    tilt = CC.transform(q[q[:, 2] == 0], RG.twist_update((0.01, -0.02, 0.0), (0.0, 0.0, 0.05), pivot))
    rec = RG.record(RG.pass_(idx, tilt, None, np.inf, pivot=pivot)["terms"])
    lam = np.linalg.eigvalsh(RG.H_of(rec))
    assert (lam[:3] <= 1e-9 * lam[-1]).all() and (lam[3:] > 1e-9 * lam[-1]).all()
    U = RG.plane_step(rec, pivot)
    R, tv = U[:, :3], U[:, 3] - (pivot - U[:, :3] @ pivot)
    assert abs(R[1, 0] - R[0, 1]) < 1e-14 and abs(tv[0]) < 1e-14 and abs(tv[1]) < 1e-14          # no rotation about z, no shift in the plane
    assert abs(R[2, 1] - R[1, 2]) > 1e-3 and abs(tv[2]) > 1e-3
    from vista_slam_amd import meshdist
    assert np.array_equal(meshdist.plane_step(rec, pivot), U) and np.array_equal(meshdist.RegRecord.from_array(rec).H, RG.H_of(rec))
    # fewer than three directions: nothing to solve, the identity
    assert np.array_equal(RG.plane_step(np.zeros(64), pivot), np.eye(4)[:3])


@pytest.mark.parametrize("name", ["room", "spheres"])
def test_known_motions_are_recovered_in_both_modes(name):
    _v, _t, src, M = RG.recovery_case(name)
    assert RG.motion_error(np.eye(4), M) > 0.03
    its = {}
    for mode in ("plane", "point"):
        a = RG.recovery_answer(name, mode)
        err = RG.motion_error(a["T"], M)
        its[mode] = a["iterations"]
        print(f"[reg cpu] {name} {mode}: {a['iterations']} iterations, {a['status']}, fitness {a['fitness']:.4f}, rmse {a['inlier_rmse']:.3e}, "
              f"|T o M - I| {err:.3e} (measured {RG.RECOVERY_MEASURED[(name, mode)]:.1e})")
        assert err <= RG.RECOVERY_FACTOR * RG.RECOVERY_MEASURED[(name, mode)]
        assert err <= RG.RECOVERY_MEASURED[(name, mode)], "the constant is the measured figure rounded up"
        assert a["fitness"] == 1.0
    assert RG.recovery_answer(name, "plane")["status"] == "converged"
    print(f"[reg cpu] {name}: iterations plane / point = {its['plane']} / {its['point']} (reported, not asserted)")


def test_the_tolerances_are_the_measured_spreads():
    v, t, q, T, radius = RG.hostile_case()
    p = RG.pass_(DC.Index(v, t), q, T, radius)
    recs = np.stack([RG.record(p["terms"], o) for o in RG.ORDERS])
    scale = np.abs(p["terms"]).sum(axis=0)
    spread = ((recs.max(axis=0) - recs.min(axis=0)) / np.where(scale > 0, scale, 1.0)).max()
    assert p["matched"].sum() > 250 and spread > 0, "the hostile case must round"
    print(f"[reg cpu] TOL_REG_SUM: measured {spread:.3e}, constant {RG.TOL_REG_SUM_MEASURED:.1e}")
    assert spread <= RG.TOL_REG_SUM_MEASURED
    worst = 0.0
    for name in ("room", "spheres"):
        for mode in ("plane", "point"):
            runs = [RG.recovery_answer(name, mode, o) for o in RG.ORDERS]
            assert len({(r["iterations"], r["status"]) for r in runs}) == 1
            d = max(np.abs(r["T"] - runs[0]["T"]).max() for r in runs)
            print(f"[reg cpu] TOL_REG_ICP {name} {mode}: {d:.3e}")
            worst = max(worst, d)
    assert worst <= RG.TOL_REG_ICP_MEASURED
