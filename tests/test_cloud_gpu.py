"""GPU: libsta_cloud.so (csrc/cloud.h) against the numpy restatement of its contract (tests/cloud_cases.py), through the C ABI with
guard regions behind every buffer, and vista_slam_amd.cloud / evaluate on top of it.  d2 and idx are compared with array_equal; so is
the record on the integer and dyadic lattices, and within TOL_SUM (of the sum of the absolute contributions) on the hostile floats.
The shapes are the smallest at which the kernels can go wrong: cloud_cases.CASES names them."""
import ctypes as C

import numpy as np
import pytest

import cloud_cases as CC

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256              # bytes behind every buffer


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")


def _tail_untouched(buf, nbytes, what):
    raw = buf[nbytes:].cpu().numpy()
    assert (raw == FILL).all(), f"{what}: bytes past its {nbytes} were written"


def run_raw(case, want=("d2", "idx", "record")):
    """sta_nn_build + sta_nn_query through the C ABI into pattern-filled buffers of exactly the planned size plus a guard.
    -> (index struct, dict of host arrays)."""
    import torch
    from vista_slam_amd import _lib
    lib = _lib.load_cloud()
    ref, qry = _up(case["ref"]), _up(case["qry"])
    M, Q = len(case["ref"]), len(case["qry"])
    sizes = (C.c_int64 * 3)()
    _lib.check_cloud(lib.sta_nn_plan(M, Q, sizes))
    ib, bw, qw = _guarded(sizes[0]), _guarded(sizes[1]), _guarded(sizes[2])
    info = _lib.StaNNIndex()
    st = torch.cuda.current_stream().cuda_stream
    _lib.check_cloud(lib.sta_nn_build(ref.data_ptr(), M, case["cell"], ib.data_ptr(), sizes[0], bw.data_ptr(), sizes[1], C.byref(info), st))
    d2, idx, rec = _guarded(Q * 8), _guarded(Q * 4), _guarded(CC.RECORD * 8)
    T = None if case["T"] is None else (C.c_double * 12)(*np.asarray(case["T"], dtype=np.float64)[:3].reshape(12).tolist())
    _lib.check_cloud(lib.sta_nn_query(C.byref(info), qry.data_ptr(), Q, T, case["radius"], d2.data_ptr() if "d2" in want else None,
                                      idx.data_ptr() if "idx" in want else None, rec.data_ptr() if "record" in want else None,
                                      qw.data_ptr() if "record" in want else None, sizes[2], st))
    torch.cuda.synchronize()
    for buf, n, what in ((ib, sizes[0], "index_buf"), (bw, sizes[1], "build work"), (qw, sizes[2] if "record" in want else 0, "query work"),
                         (d2, Q * 8 if "d2" in want else 0, "d2_out"), (idx, Q * 4 if "idx" in want else 0, "idx_out"),
                         (rec, CC.RECORD * 8 if "record" in want else 0, "record_out")):
        _tail_untouched(buf, n, what)
    out = {"index_buf": ib}
    if "d2" in want:
        out["d2"] = d2[:Q * 8].cpu().numpy().view(np.float64)
    if "idx" in want:
        out["idx"] = idx[:Q * 4].cpu().numpy().view(np.int32)
    if "record" in want:
        out["record"] = rec[:CC.RECORD * 8].cpu().numpy().view(np.float64)
    return info, out


def check_record(got, exp, exact, what):
    assert np.array_equal(got[[0, 1, 19]], exp["record"][[0, 1, 19]]) and np.array_equal(got[20:], np.zeros(4)), (what, got)
    if exact:
        assert np.array_equal(got, exp["record"]), (what, got, exp["record"])
        return
    rel = np.abs(got - exp["record"]) / np.where(exp["scale"] > 0, exp["scale"], 1.0)
    print(f"[cloud] {what}: record differs from the ascending-order sum by at most {rel.max():.3g} of sum |contribution| (TOL_SUM {CC.TOL_SUM:.3g})")
    assert (rel <= CC.TOL_SUM).all(), (what, rel.max())


def check_index(info, buf, grid, M, what, ref):
    assert (int(info.M), int(info.n_finite), int(info.C)) == (M, grid["n_finite"], grid["C"]), what
    assert tuple(info.ext) == grid["ext"], (what, tuple(info.ext), grid["ext"])
    if grid["n_finite"]:
        assert tuple(info.lo) == grid["lo"], (what, tuple(info.lo), grid["lo"])
    base = buf.data_ptr()
    raw = buf.cpu().numpy()
    def arr(ptr, n, dt):
        o = ptr - base
        return raw[o:o + n * np.dtype(dt).itemsize].view(dt)
    Cn, n = grid["C"], grid["n_finite"]
    assert np.array_equal(arr(info.cell_key, Cn, np.uint64), grid["cell_key"]), what
    assert np.array_equal(arr(info.cell_start, Cn + 1, np.int32), grid["cell_start"]), what
    assert np.array_equal(arr(info.sorted_idx, n, np.int32), grid["sorted_idx"]), what
    assert np.array_equal(arr(info.sorted_pts, 3 * n, np.float32).reshape(n, 3), ref[grid["sorted_idx"]]), what      # what the query reads


@pytest.mark.parametrize("name", list(CC.CASES))
def test_case_against_the_restatement(name):
    case, exp = CC.expected_of(name)
    info, out = run_raw(case)
    check_index(info, out["index_buf"], exp["grid"], len(case["ref"]), name, case["ref"])
    bad = np.flatnonzero(out["idx"] != exp["idx"])
    assert bad.size == 0, f"{name}: idx differs at {bad.size} of {len(exp['idx'])} queries, first {bad[:6].tolist()}: got {out['idx'][bad[:6]].tolist()}, expected {exp['idx'][bad[:6]].tolist()}"
    assert np.array_equal(out["d2"], exp["d2"]), name
    check_record(out["record"], exp, case["exact"], name)
    # a second call is bit-identical; outputs that were not asked for are not written (run_raw's guards cover the whole buffer)
    _info2, again = run_raw(case)
    assert all(np.array_equal(again[k], out[k]) for k in ("d2", "idx", "record")), name
    _i, only = run_raw(case, want=("idx",))
    assert np.array_equal(only["idx"], out["idx"]), name


@pytest.mark.parametrize("name", list(CC.REFUSED))
def test_refusals(name):
    from vista_slam_amd import _lib, cloud
    make, msg = CC.REFUSED[name]
    case = make()
    with pytest.raises(_lib.StaError, match=msg):
        run_raw(case)
    with pytest.raises(ValueError, match=msg):
        cloud.NNIndex.build(case["ref"], case["cell"]).query(case["qry"], case["radius"])


def test_transform_rounds_once_and_treats_non_finite_as_data():
    """float(T p), one rounding.  A non-finite coordinate is not special: it goes through the same arithmetic, so under the identity an
    Inf on one axis makes the other two NaN (0 * inf) - the header says so; the restatement does the same."""
    from vista_slam_amd import cloud
    _n, ref, qry, T, _r = CC.hostile_cases()[2]
    pts = np.concatenate([qry, [[np.nan, 0, 1], [np.inf, 1, 2], [3e38, -3e38, 1e30]]]).astype(np.float32)
    for M in (1, 255, 256, 257, len(pts)):
        got = cloud.transform(pts[-M:], T).cpu().numpy()
        assert np.array_equal(got, CC.transform(pts[-M:], T), equal_nan=True), M
    ident = cloud.transform(pts, None).cpu().numpy()
    assert np.array_equal(ident, CC.transform(pts, None), equal_nan=True)
    assert np.array_equal(ident[:-3], pts[:-3]) and np.array_equal(ident[-1], pts[-1])          # finite points, 3e38 included, unchanged
    assert np.isnan(ident[-3]).all() and np.isinf(ident[-2, 0]) and np.isnan(ident[-2, 1:]).all()
    assert cloud.transform(np.zeros((0, 3), np.float32), T).shape == (0, 3)


def test_python_layer_equals_the_c_abi():
    from vista_slam_amd import cloud
    case, exp = CC.expected_of("scaled_T")
    index = cloud.NNIndex.build(case["ref"], case["cell"])
    g = exp["grid"]
    assert (index.M, index.finite, index.cells, index.lo, index.extent) == (len(case["ref"]), g["n_finite"], g["C"], g["lo"], g["ext"])
    out = index.query(case["qry"], case["radius"], T=case["T"])
    assert np.array_equal(out["d2"].cpu().numpy(), exp["d2"]) and np.array_equal(out["idx"].cpu().numpy(), exp["idx"])
    check_record(out["record"].cpu().numpy(), exp, False, "scaled_T through cloud.NNIndex")
    assert set(index.query(case["qry"], case["radius"], T=case["T"], want=("idx",))) == {"idx"}


def test_icp_and_chamfer_on_the_box_room():
    from vista_slam_amd import cloud
    ref, src, move = CC.box_room_pair()
    exp = CC.icp(src, ref, 0.1)
    index = cloud.NNIndex.build(ref, 0.1)
    got = cloud.icp(src, index, 0.1)
    print(f"[cloud] box room ICP: {got.iterations} iterations, {got.status}, fitness {got.fitness}, rmse {got.inlier_rmse:.3g}; "
          f"|T - restated| {np.abs(got.T - exp['T']).max():.3g}, |rmse - restated| {abs(got.inlier_rmse - exp['inlier_rmse']):.3g} (TOL_ICP {CC.TOL_ICP:.3g})")
    assert (got.iterations, got.status) == (exp["iterations"], exp["status"]) and got.status == "converged"
    assert got.fitness == exp["fitness"] == 1.0
    assert np.abs(got.T - exp["T"]).max() <= CC.TOL_ICP and abs(got.inlier_rmse - exp["inlier_rmse"]) <= CC.TOL_ICP
    inv_t = -move[:, :3].T @ move[:, 3]
    assert np.linalg.norm(got.T[:3, 3] - inv_t) < 1e-6
    final = index.query(src, 0.1, T=got.T, want=("idx",))["idx"].cpu().numpy()
    assert np.array_equal(final, np.arange(len(src)))
    again = cloud.icp(src, index, 0.1)
    assert np.array_equal(again.T, got.T) and again[1:] == got[1:]
    few = cloud.icp(src[:2], index, 0.1)
    assert few.status == "too_few_matches" and few.iterations == 0
    # chamfer: the moved cloud against the room, clipped at 0.05 (most of the points are further than that from their neighbour's copy)
    for cell in (None, 0.05, 0.011):
        c = cloud.chamfer(ref, src, 0.05, cell=cell, return_distances=True)
        e = CC.chamfer(ref, src, 0.05)
        assert abs(c.rmse_1 - e[1]) <= CC.TOL_SUM * e[1] and abs(c.rmse_2 - e[2]) <= CC.TOL_SUM * e[2], (cell, c[:3], e[:3])
        assert abs(c.chamfer - e[0]) <= CC.TOL_SUM * e[0]
        for got, ref_d in ((c.dist_1, e[3]), (c.dist_2, e[4])):          # sqrt of bit-equal d2: one float64 step for the device's sqrt
            assert (np.abs(got.cpu().numpy() - ref_d) <= np.spacing(ref_d)).all(), cell


@pytest.fixture(scope="module")
def fe():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield m
    del m


def test_eval_recon_stage_by_stage(fe, tmp_path):
    """Every stage equals the restatement of that stage fed with the GPU's own previous stage."""
    import post_cases as PC
    import voxel_cases as V
    from vista_slam_amd import evaluate, formats
    s = CC.recon_scene()
    assert not np.array_equal(s["est_intris"][0], s["gt_intri"]) and not np.array_equal(s["est_intris"][0], s["est_intris"][1])
    acc, comp, ch, gt_pts, est_pts, st = evaluate.eval_recon(fe, **s, return_stages=True)
    host = lambda t: t.cpu().numpy()
    gt_mask = s["gt_depths"] > 0
    N = len(s["gt_depths"])
    # 1: both world clouds against the float64 statement depth -> K^-1 -> pose on the masked pixels, in view-major raster order,
    # within the bound tests/test_post_gpu.py holds sta_world_pointcloud to (post_cases.CLOUD_BOUND x the terms' magnitudes)
    for got, depths, K, poses, mask, what in ((gt_pts, s["gt_depths"], np.tile(s["gt_intri"], (N, 1, 1)), s["gt_poses"], gt_mask, "gt"),
                                              (st["est_raw"], s["est_depths"], s["est_intris"], s["est_poses"], (s["est_masks"] > 0) & gt_mask, "est")):
        world, mag = PC.cloud_ref64(depths, np.ones(N, np.float32), K, poses)
        assert got.shape == (int(mask.sum()), 3), what
        err = np.abs(host(got).astype(np.float64) - world[mask]) / mag[mask]
        print(f"[cloud] eval_recon stage 1, {what}: {len(got)} points, worst |got - float64| / magnitude {err.max():.3g} (bound {PC.CLOUD_BOUND:.3g})")
        assert (err <= PC.CLOUD_BOUND).all(), what
    assert np.array_equal(st["rel"], np.concatenate([s["rel_s"] * s["rel_R"], s["rel_t"][:, None]], axis=1))
    assert np.array_equal(host(st["est_pts"]), CC.transform(host(st["est_raw"]), st["rel"]))                        # 2
    for got, src in ((st["est_down"], st["est_pts"]), (st["gt_down"], gt_pts)):                                       # 3
        ref = V.expected(host(src), voxel_size=0.05)["points"]
        assert got.shape == ref.shape and (np.abs(host(got).astype(np.float64) - ref) <= np.spacing(np.abs(ref))).all()
    orders = [CC.icp(host(st["est_down"]), host(st["gt_down"]), 0.1, order=o) for o in CC.ORDERS]                   # 4
    e = orders[0]
    for o in orders[1:]:            # what TOL_ICP rests on, for THIS scene: the same correspondences and iterations under every order
        assert (o["iterations"], o["status"]) == (e["iterations"], e["status"]) and len(o["sets"]) == len(e["sets"])
        assert all(np.array_equal(a, b) for a, b in zip(o["sets"], e["sets"]))
    reg = st["icp"]
    print(f"[cloud] eval_recon ICP: {reg.iterations} iterations, {reg.status}, fitness {reg.fitness:.4f}, rmse {reg.inlier_rmse:.4g}, "
          f"|T - restated| {np.abs(reg.T - e['T']).max():.3g}; acc {acc:.5f} comp {comp:.5f} chamfer {ch:.5f}")
    assert (reg.iterations, reg.status, reg.fitness) == (e["iterations"], e["status"], e["fitness"])
    assert np.abs(reg.T - e["T"]).max() <= CC.TOL_ICP and abs(reg.inlier_rmse - e["inlier_rmse"]) <= CC.TOL_ICP
    assert np.array_equal(host(est_pts), CC.transform(host(st["est_pts"]), reg.T))                                  # 5
    c = CC.chamfer(host(gt_pts), host(est_pts), 0.5)                                                                 # 6
    assert abs(acc - c[1]) <= CC.TOL_SUM * c[1] and abs(comp - c[2]) <= CC.TOL_SUM * c[2] and abs(ch - c[0]) <= CC.TOL_SUM * c[0]
    assert acc < 0.05 and comp < 0.05                         # the estimate IS the ground truth up to 0.2 % depth noise
    again = evaluate.eval_recon(fe, **s)
    assert again[:3] == (acc, comp, ch) and np.array_equal(host(again[4]), host(est_pts))
    # the same numbers from a folder in save_data_all's layout
    formats.save_data_all(fe, str(tmp_path), poses=s["est_poses"], scales=np.ones((N, 1), np.float32), depths=s["est_depths"],
                          confs=s["est_masks"], intrinsics=s["est_intris"], imgs=None, conf_thres=0.5, save_view_graph=False, save_images=False,
                          save_ply=False, gt_poses=s["gt_poses"], gt_depths=s["gt_depths"], gt_intrinsics=s["gt_intri"])
    saved = evaluate.eval_recon_from_saved_data(fe, str(tmp_path), rel_est_gt=[s["rel_R"], s["rel_t"], s["rel_s"]])
    assert saved[:3] == (acc, comp, ch)
    auto = evaluate.eval_recon_from_saved_data(fe, str(tmp_path))          # align_traj of three poses instead of the known Sim(3)
    assert abs(auto[2] - ch) < 0.01


def test_eval_slam_returns_a_known_sim3():
    """seq_tum_tiny_48x64 through OnlineSLAM.step; the ground truth is the estimate moved by a known Sim(3) and rounded to fp32, so
    the alignment returns that Sim(3) and the APE is what the rounding left: e_i <= sqrt(3) * 2^-24 * max |gt coordinate| up to the
    alignment's own shift, asserted with a factor of 4."""
    import torch
    from helpers import load_golden, seq_meta
    from oracle.seq_protocol import seq_frames
    from test_slam_gpu import StubDetector, vocabulary
    from vista_slam_amd import evaluate
    from vista_slam_amd import weights as W
    from vista_slam_amd.slam import OnlineSLAM
    from vista_slam_amd.sta_frontend import STAFrontend
    g, meta = load_golden("seq_tum_tiny_48x64")
    sm = seq_meta(meta)
    H, Wd, nkf, nb, lp = sm["H"], sm["W"], sm["nkf"], sm["neighbor_edge_num"], sm["loop_edge_num"]
    m = STAFrontend(W.TINY, "cuda:0", precision="f16x3h").load_procedural(seed=sm["seed"], qk_gain=float(meta.get("qk_gain", 1.0)))
    slam = OnlineSLAM(None, vocabulary()[1], max_view_num=nkf, neighbor_edge_num=nb, loop_edge_num=lp, rel_pose_thres=float(g["thres"]),
                      pgo_every=10 ** 6, frontend=m)
    slam.lc_detector = StubDetector(nb, lp, sm["loop_dist_min"])
    frames = torch.from_numpy(seq_frames(W, nkf, H, Wd, sm["seed"], sm["tag"])).cuda()
    for i in range(nkf):
        slam.step({"rgb": frames[i:i + 1], "shape": torch.tensor([[H, Wd]]), "gray": None, "view_name": f"kf{i}"})
    est = slam.pose_graph.export(view_num=slam.view_num).poses.cpu().numpy().astype(np.float64)
    R, t, c = CC.rotation((0.5, -0.2, 1.0), 40.0), np.array([0.7, -1.1, 0.4]), 1.6
    gt = est.copy()
    gt[:, :3, :3] = R @ est[:, :3, :3]
    gt[:, :3, 3] = c * (est[:, :3, 3] @ R.T) + t
    gt = gt.astype(np.float32)
    out = evaluate.eval_slam(slam, gt)
    bound = 4 * np.sqrt(3.0) * 2.0 ** -24 * max(1.0, float(np.abs(gt[:, :3, 3]).max()))
    spread = float(np.linalg.norm(est[:, :3, 3] - est[:, :3, 3].mean(axis=0), axis=1).max())
    print(f"[cloud] eval_slam: {nkf} poses, spread {spread:.3g}, ape rmse {out['ape']['rmse']:.3g} (bound {bound:.3g}), |s - c| {abs(out['s'] - c):.3g}")
    assert out["ape"]["rmse"] <= bound and out["ape"]["max"] <= 2 * bound
    tol = 64 * 2.0 ** -24 * max(1.0, float(np.abs(gt[:, :3, 3]).max())) / spread       # the rounding, seen through a lever of the trajectory's size
    assert np.abs(out["r_a"] - R).max() <= tol and abs(out["s"] - c) <= c * tol and np.abs(out["t_a"] - t).max() <= 4 * tol * max(1.0, np.abs(t).max())
    # with ground-truth maps: the estimate's own maps in the moved frame score (near) zero
    slam.conf_thres = 0.0                                   # every pixel: the procedural model's confidences are not a real run's
    ex = slam.pose_graph.export(view_num=slam.view_num)
    depths = (ex.depths * ex.scales.reshape(-1, 1, 1) * c).cpu().numpy()
    full = evaluate.eval_slam(slam, gt, gt_depths=depths, gt_intrinsic=ex.intrinsics.cpu().numpy())
    assert set(full) == {"ape", "r_a", "t_a", "s", "rmse_acc", "rmse_comp", "chamfer"} and full["ape"] == out["ape"]
    print(f"[cloud] eval_slam recon: acc {full['rmse_acc']:.3g} comp {full['rmse_comp']:.3g} chamfer {full['chamfer']:.3g}")
    assert np.isfinite(full["chamfer"]) and full["chamfer"] <= 0.5
