"""GPU: libsta_knn.so through vista_slam_amd/cloud.py against tests/knn_cases.py, the numpy restatement of include/sta_knn.h.  The lists,
the normals, the curvature and the mean distance are compared bit for bit (array_equal); the record is exact where its sums are and
within 16 times the restatement's own spread between summation orders elsewhere; its counts are always exact."""
import numpy as np
import pytest

import cloud_cases as CC
import knn_cases as KC

pytestmark = pytest.mark.gpu


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _index(c):
    from vista_slam_amd import cloud
    return cloud.NNIndex.build(_up(c["ref"]), c["cell"])


def _same(got, want, what):
    g = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert g.shape == want.shape and g.dtype == want.dtype, (what, g.shape, g.dtype, want.shape, want.dtype)
    assert np.array_equal(g, want, equal_nan=True), (what, int((~((g == want) | ((g != g) & (want != want)))).sum()))


def _check_lists(out, want, what):
    for key in ("d2", "idx", "count"):
        _same(out[key], want[key], f"{what}: {key}")


def _check_record(rec, mean_dist, c, exact, what, min_count=KC.MIN_COUNT):
    rec = rec.cpu().numpy()
    con = KC.contributions(mean_dist, c, min_count)
    want = CC.sum_rows(con)
    assert rec.shape == (KC.RECORD,) and np.array_equal(rec[[0, 3]], want[[0, 3]]) and (rec[4:] == 0).all(), (what, rec, want)
    if exact:
        assert np.array_equal(rec, want), (what, rec, want)
    else:
        err = np.abs(rec - want)[1:3] / np.maximum(np.abs(con).sum(axis=0)[1:3], 1e-300)
        print(f"[knn] {what}: record against the ascending sum {err.max():.2e} of the sum of |contributions| (bound {KC.TOL_SUM:.1e})")
        assert (err <= KC.TOL_SUM).all(), (what, err)


def _check_moments(ref, qry, lists_dev, lists, view_np, what, min_count=KC.MIN_COUNT, exact_record=False):
    from vista_slam_amd import cloud
    mo = cloud.knn_moments(_up(ref), lists_dev, _up(qry), None if view_np is None else (view_np.tolist() if view_np.ndim == 1 else _up(view_np)), min_count)
    want = KC.moments(ref, qry, lists["d2"], lists["idx"], lists["count"], view_np, min_count)
    _same(mo["normal"], want["normal"], f"{what}: normal")
    _same(mo["curv"], want["curv"], f"{what}: curv")
    _same(mo["mean_dist"], want["mean_dist"], f"{what}: mean_dist")
    _check_record(mo["record"], want["mean_dist"], want["c"], exact_record, what, min_count)
    return want


@pytest.mark.parametrize("name", list(KC.CASES))
def test_lists_and_moments_equal_the_restatement(name):
    import torch
    c, want = KC.expected_of(name)
    index = _index(c)
    qry = _up(c["qry"])
    Q = len(c["qry"])
    out = index.knn(qry, c["k"], c["radius"])
    _check_lists(out, want, name)
    # an order changes which lanes sit together, never a bit of the output
    perm = torch.from_numpy(np.random.default_rng(1).permutation(Q).astype(np.int32)).cuda()
    _check_lists(index.knn(qry, c["k"], c["radius"], order=perm), want, name + " under a permutation")
    # single outputs
    _same(index.knn(qry, c["k"], c["radius"], want=("count",))["count"], want["count"], name + ": count alone")
    _same(index.knn(qry, c["k"], c["radius"], want=("idx",))["idx"], want["idx"], name + ": idx alone")
    # k = 1 is sta_nn_query: the two statements of the search cannot drift
    one = index.knn(qry, 1, c["radius"])
    nn = index.query(qry, c["radius"], want=("d2", "idx"))
    assert torch.equal(one["d2"][:, 0], nn["d2"]) and torch.equal(one["idx"][:, 0], nn["idx"]) and torch.equal(one["count"], (nn["idx"] >= 0).int())
    # the moments under the three orientation rules
    rng = np.random.default_rng(2)
    per_point = (c["qry"] + rng.normal(0.0, 1.0, c["qry"].shape)).astype(np.float32)
    for tag, view in (("largest component", None), ("one viewpoint", np.array([0.3, -0.2, 5.0])), ("per-point viewpoints", per_point)):
        w = _check_moments(c["ref"], c["qry"], out, want, view, f"{name}, {tag}")
    assert int(index.knn_status.item()) == 0
    print(f"[knn] {name}: M {len(c['ref'])}, Q {Q}, k {c['k']}: counts {np.bincount(want['count'], minlength=c['k'] + 1).nonzero()[0].tolist()}, "
          f"{int(np.isnan(w['normal'][:, 0]).sum())} of {Q} normals NaN")


@pytest.mark.parametrize("name", list(KC.SELF_CASES))
def test_a_cloud_against_itself_whole_and_in_chunks(name):
    import torch
    c, want = KC.expected_of(name, 0)
    index = _index(c)
    pts = _up(c["ref"])
    M = len(c["ref"])
    whole = index.knn(pts, c["k"], c["radius"], exclude_self=True)
    _check_lists(whole, want, name)
    assert not (want["idx"] == np.arange(M)[:, None]).any()
    _check_lists(index.knn(pts, c["k"], c["radius"], exclude_self=True, order=index.sorted_idx), want, name + " in the grid's order")
    assert sorted(index.sorted_idx.cpu().tolist()) == list(range(M))
    parts = [index.knn(pts[s:s + 100], c["k"], c["radius"], exclude_self=True, self_base=s) for s in range(0, M, 100)]
    for key in ("d2", "idx", "count"):
        assert torch.equal(torch.cat([p[key] for p in parts]), whole[key]), key
    _c2, with_self = KC.expected_of(name, -1)
    _check_lists(index.knn(pts, c["k"], c["radius"]), with_self, name + " with self")
    assert (with_self["idx"][:, 0] >= 0).all() and (with_self["d2"][:, 0] == 0).all()
    _check_moments(c["ref"], c["ref"], whole, want, None, name, min_count=5)
    assert int(index.knn_status.item()) == 0


def test_an_order_outside_the_queries_sets_its_status_bit_and_skips_the_slot():
    import torch
    c, want = KC.expected_of("m300_q257_k16")
    index = _index(c)
    order = torch.arange(257, dtype=torch.int32, device="cuda")
    order[7], order[200] = -1, 257
    d2 = torch.full((257, 16), -5.0, dtype=torch.float64, device="cuda")
    from vista_slam_amd import _lib
    import ctypes as C
    index.knn(_up(c["qry"]), 16, c["radius"])                     # (makes the status word)
    _lib.check_knn(_lib.load_knn().sta_knn_query(C.byref(index.info), _up(c["qry"]).data_ptr(), 257, order.data_ptr(), -1, 16, c["radius"], d2.data_ptr(),
                                                 None, None, index.knn_status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    got = d2.cpu().numpy()
    keep = np.ones(257, bool)
    keep[[7, 200]] = False
    assert np.array_equal(got[keep], want["d2"][keep]) and (got[~keep] == -5.0).all()
    assert int(index.knn_status.item()) == KC.STATUS_ORDER


def test_planes_of_a_dyadic_lattice_give_exact_normals():
    from vista_slam_amd import cloud
    pts = KC.lattice_planes()
    index = cloud.NNIndex.build(_up(pts), 0.25)
    lists = index.knn(_up(pts), 8, 0.5)
    top = pts[:, 2] == 3.0
    per_point = (pts - np.array([0.0, 0.0, 1.0])).astype(np.float32)
    for view, sign in ((None, np.ones(162)), (np.array([1.0, 1.0, 10.0]), np.ones(162)), (np.array([1.0, 1.0, 1.5]), np.where(top, -1.0, 1.0)),
                       (per_point, -np.ones(162))):
        mo = cloud.knn_moments(_up(pts), lists, _up(pts), None if view is None else (view.tolist() if view.ndim == 1 else _up(view)))
        n = mo["normal"].cpu().numpy()
        assert np.array_equal(n, np.stack([np.zeros(162), np.zeros(162), sign], axis=1).astype(np.float32)), view
        assert (mo["curv"].cpu().numpy() == 0).all()
    got = cloud.estimate_normals(_up(pts), 8, radius=0.5, viewpoint=[1.0, 1.0, 1.5], index=index, return_curvature=True)
    assert np.array_equal(got[0].cpu().numpy()[:, 2], np.where(top, -1.0, 1.0).astype(np.float32)) and (got[1] == 0).all()


@pytest.mark.parametrize("Q", [70000, 256 * 2048 + 300])
def test_the_record_is_exact_on_dyadic_sums(Q):
    """points and queries on one dyadic line: every distance, mean and square is dyadic, so every sum is exact in any order.  70000
    queries fold more than 256 partial rows; more than 2048 * 256 make a thread of the moments kernel take a second query."""
    from vista_slam_amd import cloud
    line = (np.arange(64)[:, None] * np.array([[0.25, 0.0, 0.0]])).astype(np.float32)
    rng = np.random.default_rng(Q)
    qry = (rng.integers(-2, 70, Q)[:, None] * np.array([[0.25, 0.0, 0.0]])).astype(np.float32)
    qry[::19, 1] = np.nan
    d2, idx, cnt = KC.knn_brute(line, qry, 2, 0.5, chunk=8192)
    index = cloud.NNIndex.build(_up(line), 0.25)
    lists = index.knn(_up(qry), 2, 0.5)
    _check_lists(lists, dict(d2=d2, idx=idx, count=cnt), f"line, Q {Q}")
    mo = cloud.knn_moments(_up(line), lists)
    want = KC.moments(line, qry, d2, idx, cnt)
    _same(mo["mean_dist"], want["mean_dist"], "mean_dist")
    _check_record(mo["record"], want["mean_dist"], want["c"], True, f"line, Q {Q}")
    assert np.isnan(mo["normal"].cpu().numpy()).all()              # two neighbours are below every min_count


def test_both_filters_return_the_restatement_on_the_room_with_floaters(monkeypatch):
    import torch
    from vista_slam_amd import cloud
    pts, floater = KC.room_with_floaters()
    dev = _up(pts)
    kept, mask, md, rec = KC.remove_statistical_outlier(pts, 16, 2.0, 1.0)
    got_kept, got_mask = cloud.remove_statistical_outlier(dev, 16, 2.0, radius=1.0)
    assert got_kept.dtype == torch.int64 and np.array_equal(got_kept.cpu().numpy(), kept) and np.array_equal(got_mask.cpu().numpy(), mask)
    assert not mask[floater].any() and (~mask[~floater]).sum() <= 20
    rkept, rmask = KC.remove_radius_outlier(pts, 4, 0.4)
    got_kept, got_mask = cloud.remove_radius_outlier(dev, 4, 0.4)
    assert np.array_equal(got_kept.cpu().numpy(), rkept) and np.array_equal(got_mask.cpu().numpy(), rmask) and np.array_equal(rkept, np.arange(2000))
    normals, curv = cloud.estimate_normals(dev, 8, radius=1.0, return_curvature=True)
    wn, wc = KC.estimate_normals(pts, 8, 1.0)
    _same(normals, wn, "estimate_normals")
    _same(curv, wc, "curvature")
    view = (pts + np.float32(0.5)).astype(np.float32)
    _same(cloud.estimate_normals(dev, 8, radius=1.0, viewpoint=_up(view), cell=1.0), KC.estimate_normals(pts, 8, 1.0, view)[0], "normals, own viewpoints, cell = radius")
    # in chunks (of 256 queries here): per-point results are the same bits, the kept lists the same lists
    whole = cloud._neighbourhoods(dev, 16, 1.0, None, None, True, None, 3, ("mean_dist", "normal", "record"))
    monkeypatch.setattr(cloud, "KNN_LIST_BYTES", 256 * 16 * 12)
    assert cloud.knn_chunk_rows(16) == 256
    chunks = cloud._neighbourhoods(dev, 16, 1.0, None, None, True, None, 3, ("mean_dist", "normal", "record"))
    for key in ("mean_dist", "count", "normal"):
        assert torch.equal(chunks[key].view(torch.uint8), whole[key].view(torch.uint8)), key
    assert torch.equal(chunks["record"][[0, 3]], whole["record"][[0, 3]])
    assert np.array_equal(cloud.remove_statistical_outlier(dev, 16, 2.0, radius=1.0)[0].cpu().numpy(), kept)
    assert np.array_equal(cloud.remove_radius_outlier(dev, 4, 0.4)[0].cpu().numpy(), rkept)
    _same(cloud.estimate_normals(dev, 8, radius=1.0, viewpoint=_up(view)), KC.estimate_normals(pts, 8, 1.0, view)[0], "normals in chunks")
    _check_record(whole["record"], md, whole["count"].cpu().numpy(), False, "room with floaters")          # (every index is valid: c = count)


def test_refusals_reach_the_caller_as_value_errors():
    from vista_slam_amd import cloud
    c, _want = KC.expected_of("m300_q257_k16")
    index = _index(c)
    q = _up(c["qry"])
    with pytest.raises(ValueError, match="is more than 32 cells"):
        index.knn(q, 4, np.nextafter(32 * c["cell"], 1e9))
    with pytest.raises(ValueError, match=r"k must be in \[1, 64\] \(got 65\)"):
        index.knn(q, 65, 1.0)
    with pytest.raises(ValueError, match="unknown outputs"):
        index.knn(q, 4, 1.0, want=("d2", "record"))
    with pytest.raises(ValueError, match="order must be"):
        index.knn(q, 4, 1.0, order=np.arange(5))
    with pytest.raises(ValueError, match="min_count must be at least 3"):
        cloud.knn_moments(_up(c["ref"]), index.knn(q, 4, 1.0), min_count=2)
    with pytest.raises(ValueError, match="the index holds 300 points, the cloud 257"):
        cloud.estimate_normals(q, 8, radius=1.0, index=index)


def test_save_data_all_filters_the_cloud_and_leaves_the_other_files_alone(tmp_path):
    import filecmp
    import os
    import tsdf_cases as TC
    from vista_slam_amd import formats
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    s = TC.room_scene(9, 13, 4)
    args = dict(poses=s["poses"], scales=s["scales"], depths=s["depths"], confs=s["confs"], intrinsics=s["intrinsics"], imgs=s["imgs"], conf_thres=s["conf_thres"])
    kw = dict(args, view_graph={0: [1]}, loop_min_dist=3, view_names=["a", "b", "c", "d"])
    a, b, c = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    formats.save_data_all(m, a, **kw)
    # without the keyword: the cloud as it was written before the keyword existed
    pts, _col, records = formats.world_pointcloud(m, args["depths"], args["scales"], args["intrinsics"], args["poses"], args["confs"], args["imgs"],
                                                  args["conf_thres"], want_records=True)
    formats.write_ply(str(tmp_path / "plain.ply"), records)
    assert filecmp.cmp(os.path.join(a, "pointcloud.ply"), str(tmp_path / "plain.ply"), shallow=False)
    host = pts.cpu().numpy()
    span = float(np.linalg.norm(host.max(axis=0) - host.min(axis=0)))
    radius = span / 12.0
    for folder, outlier, kept in ((b, ("statistical", 8, 1.0, radius), KC.remove_statistical_outlier(host, 8, 1.0, radius)[0]),
                                  (c, ("radius", 6, radius / 2), KC.remove_radius_outlier(host, 6, radius / 2)[0])):
        formats.save_data_all(m, folder, **kw, ply_outlier=outlier)
        assert sorted(os.listdir(a)) == sorted(os.listdir(folder))
        for f in os.listdir(a):
            if f != "pointcloud.ply":
                assert filecmp.cmp(os.path.join(a, f), os.path.join(folder, f), shallow=False), f
        got = formats.read_ply(os.path.join(folder, "pointcloud.ply"))
        print(f"[knn] save_data_all {outlier[0]}: {len(records)} -> {len(got)} points")
        assert 0 < len(kept) < len(records) and np.array_equal(got, records[kept])
        p2, c2 = formats.world_pointcloud(m, args["depths"], args["scales"], args["intrinsics"], args["poses"], args["confs"], args["imgs"], args["conf_thres"],
                                          outlier=outlier)
        assert np.array_equal(p2.cpu().numpy(), host[kept]) and c2.shape == p2.shape
    with pytest.raises(ValueError, match="outlier must be"):
        formats.world_pointcloud(m, args["depths"], args["scales"], args["intrinsics"], args["poses"], args["confs"], args["imgs"], args["conf_thres"],
                                 outlier=("median", 3))
