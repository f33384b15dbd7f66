"""GPU: sta_voxel_downsample (csrc/voxel.h) against the numpy restatement of its contract (tests/voxel_cases.py), through the C ABI
with guard regions behind every output and through vista_slam_amd.formats.  Counts, indices, inverse, V, n_dropped and the record
bytes are compared with array_equal; so are the means wherever the case's float64 sums are exact (the dyadic lattices).  The two
hostile-float cases ask for |got - ref| <= one float32 step with at most 1e-4 of the elements differing at all.  The shapes are the
smallest at which the kernels can go wrong: one point, the wave and workgroup boundaries, more than 1024 workgroups of 256 (the
single-block scan walks more than one count per thread), more than 256 sort tiles (the histogram scan's second chunk), one voxel
that holds every point, rows either side of the 1024-point threshold between the wave and the workgroup reduction, key widths
either side of a sort pass and the 63-bit edge."""
import ctypes as C

import numpy as np
import pytest

import post_cases as PC
import voxel_cases as V

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 8                # rows behind every output
ROW_BYTES = {"points": 12, "colors": 12, "counts": 4, "index": 12, "inverse": 4, "records": 27}
ORDER = ("points", "colors", "counts", "index", "inverse", "records")


@pytest.fixture(scope="module")
def m():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    fe = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield fe
    del fe


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def run_raw(m, pts, col, voxel_size, origin=None, min_points=1, want=ORDER):
    """One call through the C ABI into buffers of M + GUARD rows filled with a pattern -> dict of host arrays cut at V (inverse: at M),
    after asserting that every byte past them - and every byte of an output that was not requested - still holds the pattern."""
    import torch
    from vista_slam_amd import _lib
    M = len(pts)
    pd, cd = _up(pts), _up(col)
    bufs = {k: torch.full(((M + GUARD) * ROW_BYTES[k],), FILL, dtype=torch.uint8, device="cuda") for k in ORDER}
    ptr = [bufs[k].data_ptr() if k in want else None for k in ORDER]
    cnt = (C.c_int64 * 2)(-1, -1)
    org = (C.c_double * 3)(*origin) if origin is not None else None
    _lib.check(m.lib.sta_voxel_downsample(m._h, pd.data_ptr(), cd.data_ptr() if cd is not None else None, M, float(voxel_size), org,
                                          int(min_points), *ptr, cnt, m._stream()))
    torch.cuda.synchronize()
    Vn, dropped = int(cnt[0]), int(cnt[1])
    assert 0 <= Vn <= M and 0 <= dropped <= M
    out = {"V": Vn, "n_dropped": dropped}
    for k in ORDER:
        rows = (M if k == "inverse" else Vn) if k in want else 0
        raw = bufs[k].cpu().numpy()
        assert (raw[rows * ROW_BYTES[k]:] == FILL).all(), f"{k}: bytes at or past row {rows} were written"
        raw = raw[:rows * ROW_BYTES[k]]
        if k in ("points", "colors"):
            out[k] = raw.view(np.float32).reshape(rows, 3)
        elif k in ("counts", "inverse"):
            out[k] = raw.view(np.int32)
        elif k == "index":
            out[k] = raw.view(np.int32).reshape(rows, 3)
        else:
            out[k] = raw.reshape(rows, 27)
    return out


def records_of(points, colors):
    """The PLY vertex records of returned rows: double(fp32 mean), rint(clamp(c, 0, 1) * 255)."""
    from vista_slam_amd.formats import PLY_RECORD
    rec = np.zeros(len(points), PLY_RECORD)
    rec["x"], rec["y"], rec["z"] = (points[:, a].astype(np.float64) for a in range(3))
    rec["red"], rec["green"], rec["blue"] = (PC.color_byte(colors[:, a]) for a in range(3))
    return rec


def check_means(got, ref, exact, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (what, got.shape, ref.shape)
    if exact:
        bad = np.flatnonzero((got != ref).reshape(-1))
        assert bad.size == 0, f"{what}: {bad.size} of {got.size} means differ, first at {bad[:4].tolist()}: got {got.reshape(-1)[bad[:4]].tolist()}, expected {ref.reshape(-1)[bad[:4]].tolist()}"
        return
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    step = np.spacing(np.abs(ref)).astype(np.float64)
    n_diff = int((diff != 0).sum())
    print(f"[voxel] {what}: {n_diff} of {got.size} means differ from the ascending-order sum, worst {float((diff / step).max()) if got.size else 0.0:.2f} steps")
    assert (diff <= step).all(), (what, float((diff / step).max()))
    assert n_diff <= 1e-4 * got.size, (what, n_diff, got.size)


def check_against(out, exp, case, what):
    assert out["V"] == exp["V"] and out["n_dropped"] == exp["n_dropped"], (what, out["V"], exp["V"], out["n_dropped"], exp["n_dropped"])
    for k in ("counts", "index", "inverse"):
        if not np.array_equal(out[k], exp[k]):
            bad = np.flatnonzero((out[k] != exp[k]).reshape(-1))
            raise AssertionError(f"{what}: {k} differs at {bad.size} of {out[k].size} places, first {bad[:6].tolist()}: "
                                 f"got {out[k].reshape(-1)[bad[:6]].tolist()}, expected {exp[k].reshape(-1)[bad[:6]].tolist()}")
    check_means(out["points"], exp["points"], case["exact"], what + " points")
    check_means(out["colors"], exp["colors"], case["exact"], what + " colors")
    assert out["records"].tobytes() == records_of(out["points"], out["colors"]).tobytes(), what


@pytest.mark.parametrize("name", list(V.CASES))
def test_case_against_the_restatement(m, name):
    case, exp = V.expected_of(name)
    kw = dict(voxel_size=case["voxel_size"], origin=case["origin"], min_points=case["min_points"])
    out = run_raw(m, case["pts"], case["col"], **kw)
    check_against(out, exp, case, name)
    again = run_raw(m, case["pts"], case["col"], **kw)                # two calls on one input: bit-identical in every output
    for k in ORDER:
        assert out[k].tobytes() == again[k].tobytes(), (name, k)
    assert (out["V"], out["n_dropped"]) == (again["V"], again["n_dropped"])


def test_too_wide_a_grid_is_refused_with_the_extent(m):
    from vista_slam_amd import _lib, formats
    pts = V.too_wide()
    with pytest.raises(_lib.StaError) as raw:
        run_raw(m, pts, None, 1.0)
    with pytest.raises(ValueError) as wrapped:
        formats.voxel_downsample(m, _up(pts), voxel_size=1.0)
    with pytest.raises(ValueError) as planned:
        formats.voxel_plan(pts.min(axis=0), pts.max(axis=0), 1.0)
    assert str(raw.value) == str(wrapped.value) == str(planned.value)
    assert "2097153 x 4 x 4" in str(raw.value)
    # the handle is usable afterwards
    case, exp = V.expected_of("m65")
    check_against(run_raw(m, case["pts"], case["col"], case["voxel_size"]), exp, case, "after a refusal")


def test_two_halves_with_one_origin_share_the_grid(m):
    """index rows of two calls with the same origin are comparable: each half equals the restatement of that half, and the union of
    their voxels is the whole cloud's."""
    rng = np.random.default_rng(1750)
    pts, col, origin = V.lattice(rng, 6000, -3.0, 3.0), V.lattice_colors(rng, 6000), (-7.0, 0.125, 5.0)
    case = {"exact": True}
    seen = set()
    for half in (slice(0, 3000), slice(3000, 6000)):
        exp = V.expected(pts[half], col[half], voxel_size=0.5, origin=origin)
        out = run_raw(m, pts[half], col[half], 0.5, origin)
        check_against(out, exp, case, f"half {half}")
        seen |= {tuple(r) for r in out["index"].tolist()}
    whole = run_raw(m, pts, col, 0.5, origin)
    assert seen == {tuple(r) for r in whole["index"].tolist()}


@pytest.mark.parametrize("want", [("points",), ("colors",), ("counts",), ("index",), ("inverse",), ("records",), ()], ids=lambda w: "+".join(w) or "none")
def test_outputs_alone(m, want):
    """Any output may be NULL: the others are untouched (run_raw), V and n_dropped still come back."""
    case, exp = V.expected_of("nan_scatter")
    out = run_raw(m, case["pts"], case["col"], case["voxel_size"], want=want)
    assert out["V"] == exp["V"] and out["n_dropped"] == exp["n_dropped"]
    for k in want:
        if k == "records":
            assert out[k].tobytes() == records_of(exp["points"], exp["colors"]).tobytes()
        else:
            assert np.array_equal(out[k], exp[k]), k


def test_python_wrapper_trims_and_orders_its_results(m):
    import torch
    from vista_slam_amd import formats
    case, exp = V.expected_of("min_points_2")
    pd, cd = _up(case["pts"]), _up(case["col"])
    p, c = formats.voxel_downsample(m, pd, cd, voxel_size=case["voxel_size"], min_points=2)
    assert p.dtype == c.dtype == torch.float32 and tuple(p.shape) == tuple(c.shape) == (exp["V"], 3)
    assert np.array_equal(p.cpu().numpy(), exp["points"]) and np.array_equal(c.cpu().numpy(), exp["colors"])
    p, c, n, i, inv, rec = formats.voxel_downsample(m, pd, cd, voxel_size=case["voxel_size"], min_points=2, return_counts=True, return_index=True,
                                                    return_inverse=True, want_records=True)
    assert n.dtype == i.dtype == inv.dtype == torch.int32
    assert np.array_equal(n.cpu().numpy(), exp["counts"]) and np.array_equal(i.cpu().numpy(), exp["index"])
    assert np.array_equal(inv.cpu().numpy(), exp["inverse"]) and len(inv) == len(case["pts"])
    assert rec.dtype == formats.PLY_RECORD and rec.tobytes() == records_of(exp["points"], exp["colors"]).tobytes()
    # colors=None: no colour tensor, records carry colour 0
    p, c, rec = formats.voxel_downsample(m, pd, voxel_size=case["voxel_size"], min_points=2, want_records=True)
    assert c is None and np.array_equal(p.cpu().numpy(), exp["points"])
    assert rec.tobytes() == records_of(exp["points"], np.zeros_like(exp["points"])).tobytes()
    # every voxel filtered, every point dropped, no point at all: empty tensors
    p, c, inv = formats.voxel_downsample(m, pd, cd, voxel_size=case["voxel_size"], min_points=10 ** 6, return_inverse=True)
    assert tuple(p.shape) == tuple(c.shape) == (0, 3) and bool((inv == -1).all())
    p, c, n = formats.voxel_downsample(m, torch.full((70, 3), float("nan"), device="cuda"), voxel_size=1.0, return_counts=True)
    assert tuple(p.shape) == (0, 3) and c is None and tuple(n.shape) == (0,)
    p, c, inv = formats.voxel_downsample(m, torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda"), voxel_size=1.0, return_inverse=True)
    assert tuple(p.shape) == tuple(c.shape) == (0, 3) and tuple(inv.shape) == (0,)
    for bad in (dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(voxel_size=1.0, min_points=0), dict(voxel_size=1.0, origin=(0.0, float("inf"), 0.0))):
        with pytest.raises(ValueError):
            formats.voxel_downsample(m, pd, cd, **bad)
    with pytest.raises(ValueError, match=r"points must be \[M, 3\]"):
        formats.voxel_downsample(m, torch.zeros(5, 4, device="cuda"), voxel_size=1.0)


def test_world_pointcloud_voxel_keyword_is_one_downsample_of_the_cloud(m, tmp_path):
    """world_pointcloud(voxel_size=...) == voxel_downsample(world_pointcloud()), bit for bit, and save_data_all(ply_voxel_size=...)
    writes those records; the fused cloud is smaller where two views overlap."""
    from vista_slam_amd import formats
    depths, scales, K, poses, confs, imgs, thres = V.wall_scene()
    args = (m, depths, scales, K, poses, confs, imgs, thres)
    pts, col = formats.world_pointcloud(*args)
    ref_p, ref_c, ref_r = formats.voxel_downsample(m, pts, col, voxel_size=0.1, want_records=True)
    got_p, got_c, got_r = formats.world_pointcloud(*args, voxel_size=0.1, want_records=True)
    assert 0 < len(got_p) < len(pts)
    assert np.array_equal(got_p.cpu().numpy(), ref_p.cpu().numpy()) and np.array_equal(got_c.cpu().numpy(), ref_c.cpu().numpy())
    assert got_r.tobytes() == ref_r.tobytes()
    exp = V.expected(pts.cpu().numpy(), col.cpu().numpy(), voxel_size=0.1)
    assert len(got_p) == exp["V"]
    check_means(got_p.cpu().numpy(), exp["points"], False, "wall scene points")
    # origin and min_points are passed through
    o_p, o_c = formats.world_pointcloud(*args, voxel_size=0.1, voxel_origin=(-3.0, -3.0, 0.0), min_points=3)
    r_p, r_c = formats.voxel_downsample(m, pts, col, voxel_size=0.1, origin=(-3.0, -3.0, 0.0), min_points=3)
    assert 0 < len(o_p) < len(got_p) and np.array_equal(o_p.cpu().numpy(), r_p.cpu().numpy()) and np.array_equal(o_c.cpu().numpy(), r_c.cpu().numpy())
    formats.save_data_all(m, str(tmp_path), poses=poses, scales=scales[:, None], depths=depths, confs=confs, intrinsics=K, imgs=imgs, conf_thres=thres,
                          save_view_graph=False, save_poses=False, save_images=False, save_scales=False, save_depths=False, save_intrinsics=False,
                          save_confs=False, ply_voxel_size=0.1)
    assert formats.read_ply(str(tmp_path / "pointcloud.ply")).tobytes() == ref_r.tobytes()


def test_world_pointcloud_without_the_keyword_is_what_it_was(m):
    """The exact class of tests/post_cases.py: fp32 evaluates the cloud exactly, so the float64 reference IS the output - points,
    colours and record bytes - with and without the new keywords at their defaults."""
    from vista_slam_amd import formats
    geom = PC.CLOUD_GEOMS[1]
    depths, scales, K, poses, imgs = PC.cloud_inputs(geom, "exact")
    world, _mag = PC.cloud_ref64(depths, scales, K, poses)
    conf, keep = PC.cloud_conf(geom, "random")
    col = np.ascontiguousarray(PC.color_of(imgs).transpose(0, 2, 3, 1))[keep]
    for kw in ({}, dict(voxel_size=None, voxel_origin=None, min_points=1)):
        p, c, rec = formats.world_pointcloud(m, depths, scales, K, poses, conf, imgs, PC.CLOUD_THRES, want_records=True, **kw)
        assert len(p) == int(keep.sum())
        assert np.array_equal(p.cpu().numpy().astype(np.float64), world[keep])
        assert np.array_equal(c.cpu().numpy(), col)
        assert rec.tobytes() == records_of(p.cpu().numpy(), c.cpu().numpy()).tobytes()
