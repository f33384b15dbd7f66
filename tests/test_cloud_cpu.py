"""Host only: the numpy restatement of the cloud contract (tests/cloud_cases.py) against scipy's cKDTree and against known
answers, the host halves of vista_slam_amd/cloud.py and evaluate.py, and the measurement of the two tolerances of cloud_cases."""
import ctypes as C

import numpy as np
import pytest

import cloud_cases as CC


def test_brute_force_agrees_with_ckdtree():
    pytest.importorskip("scipy")
    from scipy.spatial import cKDTree
    for name, ref, qry, T, radius in CC.hostile_cases():
        d2, idx, q = CC.nn_brute(ref, qry, T, radius)
        ref64 = ref.astype(np.float64)
        dist, j = cKDTree(ref64).query(q, k=2)
        unique = dist[:, 0] < dist[:, 1]
        hit = idx >= 0
        assert hit.sum() > len(qry) // 2, name
        assert np.array_equal(idx[hit & unique], j[hit & unique, 0]), name
        near = np.sqrt(d2[hit])
        assert np.all(np.abs(near - dist[hit, 0]) <= 4 * np.spacing(np.maximum(near, dist[hit, 0]))), name
        assert np.all(dist[~hit, 0] > radius * (1 - 1e-15)), name
        # and the kd-tree form of the restatement is the same function where the minimum is unique
        d2k, idxk, _ = CC.nn_kdtree(ref, qry, T, radius)
        assert np.array_equal(idxk[unique], idx[unique]) and np.array_equal(d2k[unique], d2[unique]), name


def test_brute_force_rules():
    ref = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0]], dtype=np.float32)
    qry = np.array([[0.5, 0, 0], [1, 0, 0], [0, 1, 0], [np.inf, 0, 0], [9, 9, 9]], dtype=np.float32)
    d2, idx, _ = CC.nn_brute(ref, qry, None, 1.0)
    assert idx.tolist() == [0, 1, 0, -1, -1]                    # ties to the lowest index, exactly at the radius qualifies
    assert d2.tolist() == [0.25, 0.0, 1.0, np.inf, np.inf]
    _, _, rec = CC.nn_record(ref, qry, None, 1.0)
    assert rec[:4].tolist() == [4.0, 3.0, 1.25, 2.25] and rec[19] == 1.0
    d2, idx, _ = CC.nn_brute(ref, qry, None, np.nextafter(1.0, 0.0))
    assert idx.tolist() == [0, 1, -1, -1, -1]


def test_umeyama_recovers_a_known_sim3():
    from vista_slam_amd import evaluate
    rng = np.random.default_rng(3)
    x = rng.normal(0, 2, (50, 3))
    R, t, c = CC.rotation((0.2, -1.0, 0.7), 37.0), np.array([0.5, -2.0, 1.5]), 1.9
    y = c * (x @ R.T) + t
    for fn in (CC.umeyama, evaluate.umeyama):
        R2, t2, c2 = fn(x, y)
        assert np.abs(R2 - R).max() < 1e-12 and np.abs(t2 - t).max() < 1e-12 and abs(c2 - c) < 1e-12
    # no perturbation of the result lowers the cost (noisy targets: the minimum is not zero)
    y = y + rng.normal(0, 0.05, y.shape)
    R2, t2, c2 = evaluate.umeyama(x, y)
    cost = lambda R, t, c: ((y - (c * (x @ R.T) + t)) ** 2).sum()
    best = cost(R2, t2, c2)
    for k in range(40):
        dR = CC.rotation(rng.normal(size=3), rng.normal(0, 0.5))
        assert cost(dR @ R2, t2 + rng.normal(0, 1e-3, 3), c2 * (1 + rng.normal(0, 1e-3))) >= best
    assert np.linalg.det(R2) > 0


def test_align_traj_and_ape():
    from vista_slam_amd import evaluate
    rng = np.random.default_rng(4)
    n = 12
    est = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        est[i, :3, :3] = CC.rotation(rng.normal(size=3), rng.uniform(0, 90))
        est[i, :3, 3] = rng.normal(0, 1, 3)
    R, t, c = CC.rotation((1, 1, 0), 25.0), np.array([1.0, 2.0, 3.0]), 0.6
    ref = est.copy()
    ref[:, :3, :3] = R @ est[:, :3, :3]
    ref[:, :3, 3] = c * (est[:, :3, 3] @ R.T) + t
    ref[5] = np.nan                                             # dropped, as eval_traj.py:14-21 does
    r_a, t_a, s, al, rf = evaluate.align_traj(est, ref)
    assert len(al) == len(rf) == n - 1
    assert np.abs(r_a - R).max() < 1e-12 and np.abs(t_a - t).max() < 1e-12 and abs(s - c) < 1e-12
    assert np.abs(al - rf).max() < 1e-12
    stats = evaluate.ape_translation(al, rf)
    assert set(stats) == {"rmse", "mean", "median", "std", "min", "max", "sse"} and stats["rmse"] < 1e-12
    out = evaluate.full_traj_eval(est, ref, "unused", "unused")
    assert len(out) == 6 and out[5] == stats
    e = np.array([3.0, 4.0, 0.0])
    a, b = np.tile(np.eye(4), (3, 1, 1)), np.tile(np.eye(4), (3, 1, 1))
    a[:, 0, 3] = e
    assert evaluate.ape_translation(a, b) == CC.ape(a[:, :3, 3], b[:, :3, 3])
    assert evaluate.ape_translation(a, b)["sse"] == 25.0 and evaluate.ape_translation(a, b)["median"] == 3.0


def test_kabsch_returns_a_proper_rotation_on_a_reflection():
    from vista_slam_amd import cloud
    rng = np.random.default_rng(5)
    q = rng.normal(0, 1, (40, 3))
    q[:, 2] *= 1e-3                                             # nearly planar: the reflected fit is as good as the rotated one
    p = q * np.array([1.0, 1.0, -1.0])                           # a reflection
    c = np.zeros((40, CC.RECORD))
    c[:, 0] = c[:, 1] = 1.0
    for a in range(3):
        c[:, 4 + a], c[:, 7 + a] = q[:, a], p[:, a]
        for b in range(3):
            c[:, 10 + 3 * a + b] = q[:, a] * p[:, b]
    rec = CC.sum_rows(c)
    for T in (cloud.kabsch(rec), CC.kabsch(rec)):
        R = T[:, :3]
        assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    assert np.array_equal(cloud.kabsch(rec), CC.kabsch(rec))
    A, B = cloud.kabsch(rec), np.concatenate([CC.rotation((0, 0, 1), 5.0), [[1.0], [2.0], [3.0]]], axis=1)
    assert np.array_equal(cloud.compose(A, B), CC.compose(A, B))


def test_icp_recovers_the_box_room_motion():
    """Measured with scipy's tree in float64: 5 iterations, translation error 2.3e-9, inlier_rmse 8.7e-8 (printed below).  The bound
    on the translation error, 1e-6, is about 400 x that and the size of fp32 rounding at 4 m."""
    pytest.importorskip("scipy")
    ref, src, move = CC.box_room_pair()
    r = CC.icp(src, ref, 0.1, nn=CC.nn_kdtree)
    inv_R = move[:, :3].T
    inv_t = -inv_R @ move[:, 3]
    err_t = np.linalg.norm(r["T"][:3, 3] - inv_t)
    print(f"box room ICP: {r['iterations']} iterations, status {r['status']}, fitness {r['fitness']}, inlier_rmse {r['inlier_rmse']:.3g}, "
          f"translation error {err_t:.3g}, rotation error {np.abs(r['T'][:3, :3] - inv_R).max():.3g}")
    assert r["status"] == "converged" and r["iterations"] < 30
    assert r["fitness"] == 1.0
    assert np.array_equal(r["idx"], np.arange(len(src)))
    assert err_t < 1e-6
    few = CC.icp(src[:2], ref, 0.1, nn=CC.nn_kdtree)
    assert few["status"] == "too_few_matches" and few["iterations"] == 0


def test_tolerances_are_the_measured_spread():
    """TOL_SUM and TOL_ICP of cloud_cases: measured here on the restatement alone, printed, and held against the constants."""
    pytest.importorskip("scipy")
    worst = 0.0
    for name, ref, qry, T, radius in CC.hostile_cases():
        d2, idx, q = CC.nn_brute(ref, qry, T, radius)
        c = CC.contributions(ref, q, d2, idx, radius)
        sums = [CC.sum_rows(c, o) for o in CC.ORDERS]
        scale = np.abs(c).sum(axis=0)
        spread = np.maximum.reduce([np.abs(a - b) for a in sums for b in sums])
        rel = np.where(scale > 0, spread / np.where(scale > 0, scale, 1.0), 0.0).max()
        print(f"TOL_SUM case {name}: relative spread {rel:.3g}")
        worst = max(worst, rel)
    print(f"TOL_SUM measured {worst:.3g} -> x16 = {16 * worst:.3g} (constant {CC.TOL_SUM:.3g})")
    assert worst <= CC.TOL_SUM_MEASURED and CC.TOL_SUM == 16 * CC.TOL_SUM_MEASURED
    ref, src, _move = CC.box_room_pair()
    runs = [CC.icp(src, ref, 0.1, order=o, nn=CC.nn_kdtree) for o in CC.ORDERS]
    for r in runs[1:]:              # the condition the tolerance rests on: change the input, not the tolerance, if this fails
        assert r["iterations"] == runs[0]["iterations"] and r["status"] == runs[0]["status"]
        assert len(r["sets"]) == len(runs[0]["sets"]) and all(np.array_equal(a, b) for a, b in zip(r["sets"], runs[0]["sets"]))
    dT = max(np.abs(a["T"] - b["T"]).max() for a in runs for b in runs)
    dF = max(abs(a["fitness"] - b["fitness"]) for a in runs for b in runs)
    dR = max(abs(a["inlier_rmse"] - b["inlier_rmse"]) for a in runs for b in runs)
    print(f"TOL_ICP measured: transform {dT:.3g}, fitness {dF:.3g}, rmse {dR:.3g} -> x16 = {16 * max(dT, dF, dR):.3g} (constant {CC.TOL_ICP:.3g})")
    assert max(dT, dF, dR) <= CC.TOL_ICP_MEASURED and CC.TOL_ICP == 16 * CC.TOL_ICP_MEASURED


def test_plan_and_its_refusals():
    from vista_slam_amd import _lib, cloud
    lib = _lib.load_cloud()
    for M, Q in [(1, 1), (255, 257), (1024, 1025), (262145, 64), (20_000_000, 3), (3, 600_000), ((1 << 30) - 1, (1 << 30) - 1)]:
        out = (C.c_int64 * 3)()
        assert lib.sta_nn_plan(M, Q, out) == 0
        assert tuple(out) == tuple(cloud.plan(M, Q)), (M, Q)
    for M, Q in [(0, 1), (1, 0), (1 << 30, 1), (1, 1 << 30), (-5, 5)]:
        with pytest.raises(ValueError) as e:
            cloud.plan(M, Q)
        out = (C.c_int64 * 3)()
        assert lib.sta_nn_plan(M, Q, out) != 0
        assert lib.sta_cloud_last_error().decode() == str(e.value)
    with pytest.raises(ValueError, match="more than 32 cells"):
        cloud.check_radius(np.nextafter(3.2, 4.0), 0.1)
    assert cloud.check_radius(32 * 0.1, 0.1) == 32 * 0.1
    with pytest.raises(ValueError, match="finite and >= 0"):
        cloud.check_radius(-1.0, 0.1)


def test_load_data_reads_a_saved_folder(tmp_path):
    from vista_slam_amd import evaluate
    rng = np.random.default_rng(6)
    N, H, W = 3, 4, 5
    np.save(tmp_path / "trajectory.npy", np.tile(np.eye(4, dtype=np.float32), (N, 1, 1)))
    np.save(tmp_path / "scales.npy", rng.uniform(1, 2, (N, 1)).astype(np.float32))
    np.save(tmp_path / "depths.npy", rng.uniform(1, 2, (N, H, W)).astype(np.float32))
    np.savez(tmp_path / "confs.npz", confs=rng.uniform(0, 9, (N, H, W)).astype(np.float32), thres=4.2)
    np.save(tmp_path / "intrinsics.npy", np.tile(np.eye(3, dtype=np.float32), (N, 1, 1)))
    np.savez(tmp_path / "view_graph.npz", view_graph={0: [1], 1: [0, 2], 2: [1]}, loop_min_dist=40, view_names=["a", "b", "c"])
    np.save(tmp_path / "gt_poses.npy", np.tile(np.eye(4, dtype=np.float32), (N, 1, 1)))
    np.save(tmp_path / "gt_depths.npy", rng.uniform(1, 2, (N, H, W)).astype(np.float32))
    np.save(tmp_path / "gt_intrinsics.npy", np.eye(3))
    d = evaluate.load_data(str(tmp_path))
    assert d.view_graph == {0: [1], 1: [0, 2], 2: [1]} and d.loop_min_dist == 40 and d.view_names == ["a", "b", "c"]
    assert d.scales.shape == (N, 1, 1) and d.unscaled_depths.shape == (N, H, W) and d.conf_thres == 4.2
    assert d.gt_depths.shape == (N, H, W) and d.gt_poses.shape == (N, 4, 4) and d.gt_intrinsic.shape == (3, 3) and d.poses.shape == (N, 4, 4)
    d = evaluate.load_data(str(tmp_path), load_view_graph=False, load_gt_depths=False)
    assert not hasattr(d, "view_graph") and not hasattr(d, "gt_depths")
