"""GPU: libsta_reg.so through vista_slam_amd/meshdist.py against tests/reg_cases.py, the numpy restatement of include/sta_reg.h.  The
per-query outputs (d2, tri, point, resid) are compared with array_equal; the record with array_equal where every sum is exact (the dyadic
case), within TOL_REG_SUM of the sum of absolute terms elsewhere, its counts always exactly; meshdist.icp against the restated loop
within TOL_REG_ICP with the same iteration count and status.  The shapes are the smallest at which the code can go wrong: triangle
counts that give one to four levels with a ragged last node, query counts around the wavefront, the workgroup and 256 workgroups, ties,
invalid triangles, hostile magnitudes, queries that are not finite."""
import math

import numpy as np
import pytest

import cloud_cases as CC
import dist_cases as DC
import reg_cases as RG

pytestmark = pytest.mark.gpu
WANT = ("record", "d2", "tri", "point", "resid")
COUNTS = (0, 1, 19, 20)


def _mesh(v, t):
    import torch
    from vista_slam_amd import tsdf
    return tsdf.Mesh(torch.from_numpy(np.array(v)).cuda(), None, torch.from_numpy(np.array(t)).cuda())


def _index(v, t):
    from vista_slam_amd import meshdist
    return meshdist.TriIndex.build(_mesh(v, t))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def run(idx, q, T=None, radius=math.inf, normals=None, min_cos=None, pivot=None):
    import torch
    out = idx.register_pass(torch.from_numpy(np.array(q)).cuda(), T, radius, None if normals is None else torch.from_numpy(np.array(normals)).cuda(),
                            min_cos, pivot, want=WANT)
    return {w: a.cpu().numpy() for w, a in zip(WANT, out)}


def check(v, t, q, T=None, radius=math.inf, normals=None, min_cos=None, pivot=None, exact=False, idx=None, ref=None):
    """one pass on the device and in numpy: every per-query output equal, the counts equal, the record equal (exact) or within
    TOL_REG_SUM, the status word 0 -> (device outputs, restatement)"""
    idx = _index(v, t) if idx is None else idx
    ref = DC.Index(v, t) if ref is None else ref
    got = run(idx, q, T, radius, normals, min_cos, pivot)
    want = RG.pass_(ref, q, T, radius, normals, 0.0 if min_cos is None else min_cos, pivot)
    for name in ("d2", "tri", "point", "resid"):
        g, w = got[name], want[name]
        bad = np.nonzero(~((g == w) | ((g != g) & (w != w))).reshape(len(q), -1).all(axis=1))[0]
        assert _same(g, w), f"{name}: {len(bad)} of {len(q)} queries differ, first {bad[:1]}: got {g[bad[:1]]}, restatement {w[bad[:1]]}"
    rec = RG.record(want["terms"])
    assert got["record"].shape == (64,) and (got["record"][50:] == 0).all()
    assert np.array_equal(got["record"][list(COUNTS)], rec[list(COUNTS)]), (got["record"][list(COUNTS)], rec[list(COUNTS)])
    if exact:
        assert np.array_equal(RG.record(want["terms"], "rev"), rec) and np.array_equal(RG.record(want["terms"], "pairwise"), rec), "the case is not exact"
        assert _same(got["record"], rec), np.nonzero(got["record"] != rec)[0]
    else:
        scale = np.abs(want["terms"]).sum(axis=0)
        with np.errstate(invalid="ignore"):
            err = np.abs(got["record"] - rec)
        ok = (err <= RG.TOL_REG_SUM * scale) | (got["record"] == rec)          # (== covers +inf: an unmatched query under radius = +inf)
        assert ok.all(), (np.nonzero(~ok)[0], got["record"][~ok], rec[~ok], scale[~ok])
    assert int(idx.reg_status[0]) == 0 and int(idx.counters[4]) == 0, "the status bits stay 0"
    return got, want


@pytest.mark.parametrize("nt", [1, 8, 9, 65, 513])
def test_one_to_four_levels_with_a_ragged_last_node(nt):
    v, t = DC.soup(nt, seed=nt)
    idx, ref = _index(v, t), DC.Index(v, t)
    assert idx.levels == len(DC.level_counts(nt)) == {1: 1, 8: 1, 9: 2, 65: 3, 513: 4}[nt]
    q = DC.soup_queries(257, seed=nt + 1)
    for name in ("rotation", "identity"):
        for radius in (math.inf, 0.25):
            check(v, t, q, RG.TRANSFORMS[name](), radius, pivot=(0.5, 0.5, 0.5), idx=idx, ref=ref)


def _in_footprint(Q, seed):
    """Q dyadic queries whose images under the dyadic translation lie above the lattice's footprint: every term of the record is exact"""
    r = np.random.default_rng(seed)
    T = RG.TRANSFORMS["dyadic_translation"]()
    moved = np.stack([r.integers(0, 17, Q) / 16.0, r.integers(0, 17, Q) / 16.0, r.integers(-8, 9, Q) / 8.0], axis=1)
    return (moved - T[:, 3]).astype(np.float32), T


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 255, 256, 257, 256 * 257 + 1])
def test_query_counts_around_the_wavefront_the_workgroup_and_256_workgroups(Q):
    """the last one gives 258 partial rows: the fold's threads 0 and 1 take a second row.  Exact sums, so the record is compared
    with array_equal at every count."""
    v, t = DC.lattice(4, 0.25)
    q, T = _in_footprint(Q, Q)
    got, want = check(v, t, q, T, 1.0, pivot=(0.5, 0.25, -0.125), exact=True)
    assert got["record"][1] == Q and np.array_equal(got["resid"], want["q"][:, 2])
    if Q == 65:
        vs, ts = DC.soup(65, seed=2)
        check(vs, ts, DC.soup_queries(Q, seed=Q), RG.TRANSFORMS["similarity"](), 0.3)


def test_the_record_of_the_dyadic_case_is_exact_and_two_calls_are_bit_identical():
    v, t, q, T, pivot = RG.dyadic_case()
    idx = _index(v, t)
    got, want = check(v, t, q, T, math.inf, pivot=pivot, exact=True, idx=idx)
    assert (want["nhat"] == np.array([0.0, 0.0, 1.0])).all() and got["record"][1] == len(q)
    again = run(idx, q, T, math.inf, pivot=pivot)
    for w in WANT:
        assert _same(got[w], again[w]), w
    # ties: every surface point on two triangles, the lower index wins; the record does not see which
    v2, t2 = DC.reversed_duplicated(v, t)
    got2, _ = check(v2, t2, q, T, math.inf, pivot=pivot, exact=True)
    assert (got2["tri"] < len(t)).all() and _same(got2["record"][:29], got["record"][:29])


@pytest.mark.parametrize("name", list(RG.TRANSFORMS))
def test_the_hostile_case_invalid_triangles_and_queries_that_are_not_finite_under_every_kind_of_transform(name):
    T = RG.TRANSFORMS[name]()
    v, t, q = DC.hostile_soup()[0], DC.hostile_soup()[1], DC.hostile_queries()
    idx = _index(v, t)
    got, _ = check(v, t, q, T, math.inf, pivot=(1.0, -2.0, 0.5), idx=idx)
    again = run(idx, q, T, math.inf, pivot=(1.0, -2.0, 0.5))
    assert _same(got["record"], again["record"]), "two calls are bit-identical"
    vb, tb = DC.with_bad(*DC.soup(200, seed=5))
    qb = RG.poisoned(DC.soup_queries(300, seed=6))
    got, want = check(vb, tb, qb, T, 0.3, pivot=(0.5, 0.5, 0.5))
    assert got["record"][19] == (~want["finite"]).sum() > 50 and 0 < got["record"][1] < got["record"][0]
    vd, td = DC.reversed_duplicated(*DC.lattice())
    check(vd, td, RG.poisoned(DC.lattice_queries()), T, math.inf)


def test_radius_zero_a_radius_that_matches_nothing_and_infinity():
    v, t = DC.lattice()
    q = DC.lattice_queries()
    idx, ref = _index(v, t), DC.Index(v, t)
    got, _ = check(v, t, q, None, 0.0, idx=idx, ref=ref, exact=True)          # the queries in the plane are at distance 0: inclusive
    assert 0 < got["record"][1] == (q[:, 2] == 0).sum() < len(q) and got["record"][2] == 0 and got["record"][3] == 0
    far = q + np.float32(64.0)
    got, _ = check(v, t, far, None, 1.0, idx=idx, ref=ref, exact=True)
    assert got["record"][1] == 0 and got["record"][0] == len(q) == got["record"][3] and (got["tri"] == -1).all() and np.isnan(got["resid"]).all()
    assert (got["record"][4:19] == 0).all() and (got["record"][21:] == 0).all(), "an unmatched query adds 0, never a NaN"
    got, _ = check(v, t, far, None, math.inf, idx=idx, ref=ref, exact=True)
    assert got["record"][1] == len(q)
    # a mesh without a valid triangle: every finite query is unmatched, also under radius = +inf
    vz, tz = DC.lattice()
    got, _ = check(vz, np.zeros_like(tz), q, None, math.inf)
    assert got["record"][1] == 0 and got["record"][3] == math.inf and (got["tri"] == -1).all()


def test_normals_reject_exactly_the_flipped_half_after_the_search():
    v, t = DC.room()
    idx, ref = _index(v, t), DC.Index(v, t)
    q = DC.soup_queries(600, seed=12)
    T, radius = RG.TRANSFORMS["rotation"](), 0.4
    plain, base = check(v, t, q, T, radius, idx=idx, ref=ref)
    found = base["found"]
    assert 100 < found.sum() < len(q)
    # the query's normal in ITS frame: the matched triangle's, turned back by R^T, and flipped for every second query
    flip = np.arange(len(q)) % 2 == 1
    nrm = (np.where(found[:, None], base["nhat"], 1.0) @ T[:, :3]) * np.where(flip, -1.0, 1.0)[:, None]
    nrm = nrm.astype(np.float32)
    got, want = check(v, t, q, T, radius, nrm, 0.0, idx=idx, ref=ref)
    assert np.array_equal(want["rejected"], found & flip) and got["record"][20] == (found & flip).sum() > 50
    assert got["record"][1] == (found & ~flip).sum() and got["record"][0] == plain["record"][0]
    for w in ("d2", "tri", "point", "resid"):
        assert _same(got[w], plain[w]), f"{w}: a rejected query keeps the triangle it found"
    r2 = radius * radius
    grown = plain["record"][3] + (r2 - base["d2"][found & flip]).sum()          # each rejected query now contributes r2 in place of its d2
    assert abs(got["record"][3] - grown) <= RG.TOL_REG_SUM * (np.abs(want["terms"][:, 3]).sum() + np.abs(base["terms"][:, 3]).sum())
    # min_cos = -1 rejects nothing: asserted where the comparison is exact - the axis-aligned lattice under the identity, normals
    # +-(0, 0, 1), so the flipped half sits exactly ON the bound, -1 < -1 * 1 being false.  (On the room the flipped normals are float32
    # roundings of a rotated vector: within an ulp of the bound on either side, where the restatement decides.)
    vl, tl = DC.lattice()
    ql = DC.lattice_queries()
    nl = np.zeros((len(ql), 3), np.float32)
    nl[:, 2] = np.where(np.arange(len(ql)) % 2 == 1, -1.0, 1.0)
    il, rl = _index(vl, tl), DC.Index(vl, tl)
    open_, _ = check(vl, tl, ql, None, math.inf, idx=il, ref=rl, exact=True)
    got, _ = check(vl, tl, ql, None, math.inf, nl, -1.0, idx=il, ref=rl, exact=True)
    assert got["record"][20] == 0 and _same(got["record"], open_["record"]), "min_cos = -1 rejects nothing"
    got, _ = check(vl, tl, ql, None, math.inf, nl, 0.0, idx=il, ref=rl, exact=True)
    assert got["record"][20] == len(ql) // 2
    check(v, t, q, T, radius, nrm, -1.0, idx=idx, ref=ref)
    nan = nrm.copy()
    nan[::3] = np.nan
    got, _ = check(v, t, q, T, radius, nan, 2.0, idx=idx, ref=ref)          # min_cos above 1 rejects every finite normal; a NaN normal rejects nothing
    assert got["record"][1] == (found & (np.arange(len(q)) % 3 == 0)).sum() > 0


@pytest.mark.parametrize("case", ["room", "hostile_soup", "spheres_case"])
def test_with_the_identity_the_search_is_the_distance_query_of_the_same_points(case):
    """the drift guard: two statements of one search, in two libraries"""
    import torch
    if case == "spheres_case":
        v, t, q, _ans = DC.spheres_case()
    else:
        v, t = getattr(DC, case)()
        q = DC.hostile_queries() if case == "hostile_soup" else DC.soup_queries(1000, seed=7)
    idx = _index(v, t)
    qd = torch.from_numpy(np.array(RG.poisoned(q))).cuda()
    for radius in (math.inf, 0.5):
        a = idx.query(qd, radius)
        b = idx.register_pass(qd, None, radius, want=("d2", "tri", "point"))
        for name, x, y in zip(("d2", "tri", "point"), a, b):
            assert _same(x.cpu().numpy(), y.cpu().numpy()), (case, radius, name)
    assert int(idx.reg_status[0]) == 0 and int(idx.counters[4]) == 0


def test_refusals_of_the_python_layer():
    from vista_slam_amd import meshdist
    v, t = DC.lattice()
    idx = _index(v, t)
    q = DC.lattice_queries()
    with pytest.raises(ValueError, match="reg_pass: radius"):
        run(idx, q, None, -1.0)
    with pytest.raises(ValueError, match="min_cos needs normals"):
        run(idx, q, None, 1.0, None, 0.5)
    with pytest.raises(ValueError, match="want must name"):
        idx.register_pass(q, want=("record", "bary"))
    with pytest.raises(ValueError, match="mode must be"):
        meshdist.icp(q, idx, 0.2, mode="sphere")
    r = meshdist.icp(q + np.float32(64.0), idx, 0.2)
    assert r.status == "too_few_matches" and r.iterations == 0 and r.fitness == 0.0


@pytest.mark.parametrize("name", ["room", "spheres"])
@pytest.mark.parametrize("mode", ["plane", "point"])
def test_icp_is_the_restated_loop(name, mode):
    from vista_slam_amd import cloud, meshdist
    v, t, src, M = RG.recovery_case(name)
    want = RG.recovery_answer(name, mode)
    idx = _index(v, t)
    got = meshdist.icp(src, idx, RG.MAX_CORR, mode=mode, max_iter=RG.RECOVERY_MAX_ITER)
    print(f"[reg gpu] {name} {mode}: {got.iterations} iterations, {got.status}, |T - restatement| {np.abs(got.T - want['T']).max():.2e}, "
          f"|T o M - I| {RG.motion_error(got.T, M):.2e}")
    assert (got.iterations, got.status) == (want["iterations"], want["status"])
    assert np.abs(got.T - want["T"]).max() <= RG.TOL_REG_ICP
    assert abs(got.fitness - want["fitness"]) == 0 and abs(got.inlier_rmse - want["inlier_rmse"]) <= RG.TOL_REG_ICP
    assert RG.motion_error(got.T, M) <= RG.RECOVERY_FACTOR * RG.RECOVERY_MEASURED[(name, mode)]
    if mode == "point":
        # one update from the identity is cloud.kabsch of the first twenty entries of the first record
        rec, = idx.register_pass(src, None, RG.MAX_CORR)
        one = meshdist.icp(src, idx, RG.MAX_CORR, mode="point", max_iter=1)
        assert np.array_equal(one.T[:3], cloud.kabsch(rec.cpu().numpy()[:24])) and one.iterations == 1


def test_eval_mesh_refines_the_transform_before_it_scores():
    """the three spheres of the recovery case moved by its known motion and scored against themselves: refine="plane" returns the inverse
    motion to within the bound measured on the CPU, and the surface-mode accuracy falls below the unrefined one; without refine= the
    score is what it was"""
    import torch
    from vista_slam_amd import evaluate
    v, t = DC.spheres_case()[:2]
    M = RG.recovery_case("spheres")[3]
    moved = CC.transform(v, M)
    kw = dict(n_samples=4000, threshold=0.05, max_error=0.5, seed=3, mode="surface")
    plain = evaluate.eval_mesh("cuda:0", _mesh(moved, t), _mesh(v, t), **kw)
    again = evaluate.eval_mesh("cuda:0", _mesh(moved, t), _mesh(v, t), refine=None, **kw)
    assert plain.T is None and again.T is None and len(plain) == 11
    for a, b in zip(plain[:10], again[:10]):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
    fine = evaluate.eval_mesh("cuda:0", _mesh(moved, t), _mesh(v, t), refine="plane", refine_max_corr=RG.MAX_CORR, **kw)
    err = RG.motion_error(fine.T, M)
    print(f"[reg gpu] eval_mesh(refine='plane'): |T o M - I| {err:.2e}, accuracy {plain.accuracy:.3e} -> {fine.accuracy:.3e}, completion {plain.completion:.3e} -> "
          f"{fine.completion:.3e}")
    assert fine.T.shape == (4, 4) and err <= RG.RECOVERY_FACTOR * RG.RECOVERY_MEASURED[("spheres", "plane")]
    assert fine.accuracy < plain.accuracy and fine.completion < plain.completion and plain.accuracy > 1e-3
    with_normals = evaluate.eval_mesh("cuda:0", _mesh(moved, t), _mesh(v, t), refine="plane", refine_max_corr=RG.MAX_CORR, refine_min_cos=0.5, **kw)
    assert RG.motion_error(with_normals.T, M) <= RG.RECOVERY_FACTOR * RG.RECOVERY_MEASURED[("spheres", "plane")]
    with pytest.raises(ValueError, match="gt must be a mesh"):
        evaluate.eval_mesh("cuda:0", _mesh(moved, t), torch.from_numpy(np.array(v)).cuda(), refine="plane", **kw)
    with pytest.raises(ValueError, match="refine must be"):
        evaluate.eval_mesh("cuda:0", _mesh(moved, t), _mesh(v, t), refine="sphere", **kw)
