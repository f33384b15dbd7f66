"""GPU: libsta_raster.so (csrc/raster.h) against the numpy restatement of its contract (tests/render_cases.py), through the C ABI into
pattern-filled buffers with guard regions behind every one, and vista_slam_amd.render on top of it.  Every comparison is array_equal on
keys, rgba, depth and ids.  The canvases are tiny: nothing here depends on size beyond wave and tile tails; render_cases.CASES names them."""
import ctypes as C
import os

import numpy as np
import pytest

import render_cases as RC

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


def _cam(a):
    T = (C.c_double * 12)(*np.asarray(a.get("T", RC.IDENT), dtype=np.float64).reshape(12).tolist())
    K = (C.c_double * 4)(*[float(v) for v in a.get("K", (1, 1, 0, 0))])
    return T, K, float(a.get("near", 1e-3)), float(a.get("far", 1e4))


def draw(lib, keys, H, W, s, kind, a, counters, st):
    """one op of a case through the C ABI -> the return code"""
    T, K, near, far = _cam(a)
    if kind == "points":
        pts = _up(np.asarray(a["pts"], dtype=np.float32).reshape(-1, 3))
        col = a.get("colors")
        ck = 0 if col is None else 1 if np.asarray(col).dtype == np.uint8 else 2
        cold = _up(np.asarray(col)) if col is not None else None
        return lib.sta_raster_points(keys.data_ptr(), H, W, s, pts.data_ptr(), cold.data_ptr() if cold is not None else None, ck, int(a.get("id_base", 0)),
                                     len(pts), T, K, near, far, int(a.get("psize", 1)), counters.data_ptr() if counters is not None else None, st)
    segs = _up(np.asarray(a["segs"], dtype=np.float32).reshape(-1, 2, 3))
    cold = _up(np.asarray(a["colors"], dtype=np.uint8).reshape(-1, 3))
    return lib.sta_raster_lines(keys.data_ptr(), H, W, s, segs.data_ptr(), cold.data_ptr(), len(segs), T, K, near, far, int(a.get("width", 1)), st)


def run_raw(case, want=("rgba", "depth", "ids"), ops=None):
    """clear + every op + resolve through the C ABI into pattern-filled buffers of exactly the planned size plus a guard -> dict of
    host arrays"""
    import torch
    from vista_slam_amd import _lib
    lib = _lib.load_raster()
    H, W, s = case["H"], case["W"], case["ssaa"]
    sizes = (C.c_int64 * 3)()
    _lib.check_raster(lib.sta_raster_plan(H, W, s, sizes))
    assert tuple(sizes) == RC.plan(H, W, s)
    keys, cnt = _guarded(sizes[0]), torch.zeros(32 + GUARD, dtype=torch.uint8, device="cuda")
    cnt[32:] = FILL
    st = torch.cuda.current_stream().cuda_stream
    _lib.check_raster(lib.sta_raster_clear(keys.data_ptr(), H, W, s, st))
    for kind, a in (case["ops"] if ops is None else ops):
        _lib.check_raster(draw(lib, keys, H, W, s, kind, a, cnt, st))
    rgba, depth, ids = _guarded(H * W * 4), _guarded(H * W * 4), _guarded(H * W * 4)
    bg = (C.c_uint8 * 4)(*case["background"])
    _lib.check_raster(lib.sta_raster_resolve(keys.data_ptr(), H, W, s, bg, rgba.data_ptr() if "rgba" in want else None,
                                             depth.data_ptr() if "depth" in want else None, ids.data_ptr() if "ids" in want else None, st))
    torch.cuda.synchronize()
    for buf, n, what in ((keys, sizes[0], "keys"), (cnt, 32, "counters"), (rgba, H * W * 4 if "rgba" in want else 0, "rgba_out"),
                         (depth, H * W * 4 if "depth" in want else 0, "depth_out"), (ids, H * W * 4 if "ids" in want else 0, "id_out")):
        _tail_untouched(buf, n, what)
    out = {"keys": keys[:sizes[0]].cpu().numpy().view(np.uint64).reshape(sizes[1], sizes[2]), "counters": cnt[:32].cpu().numpy().view(np.uint64)}
    if "rgba" in want:
        out["rgba"] = rgba[:H * W * 4].cpu().numpy().reshape(H, W, 4)
    if "depth" in want:
        out["depth"] = depth[:H * W * 4].cpu().numpy().view(np.float32).reshape(H, W)
    if "ids" in want:
        out["ids"] = ids[:H * W * 4].cpu().numpy().view(np.uint32).reshape(H, W)
    return out


def same(got, exp, name, fields=("keys", "counters", "rgba", "depth", "ids")):
    for k in fields:
        bad = np.argwhere(np.asarray(got[k] != exp[k]))
        assert bad.size == 0, f"{name}: {k} differs at {len(bad)} places, first {bad[:4].tolist()}: got {got[k][tuple(bad[0])]}, expected {exp[k][tuple(bad[0])]}"


@pytest.mark.parametrize("name", list(RC.CASES))
def test_case_against_the_restatement(name):
    case, exp = RC.expected_of(name)
    got = run_raw(case)
    same(got, exp, name)
    again = run_raw(case)                                   # repeatability: two runs are bit-identical
    same(again, got, name + " (second run)")
    only = run_raw(case, want=("depth",))                   # outputs that were not asked for are not written (the guards cover the whole buffer)
    assert np.array_equal(only["depth"], exp["depth"]), name


def test_contention_does_not_depend_on_the_order():
    case, exp = RC.expected_of("contention")
    pts = case["ops"][0][1]["pts"]
    # ids follow the order, so compare the depth image; with colours the whole key
    r = np.random.default_rng(9)
    col = r.integers(0, 4, (len(pts), 3), dtype=np.uint8)               # few colours: many equal keys
    perm = r.permutation(len(pts))
    a = run_raw(case, ops=[("points", dict(pts=pts, colors=col, **RC.UNIT))])
    b = run_raw(case, ops=[("points", dict(pts=pts[perm], colors=col[perm], **RC.UNIT))])
    same(b, a, "contention, shuffled")
    keys = RC.new_keys(case["H"], case["W"], 1)
    RC.points(keys, 1, pts, col, **RC.UNIT)
    assert np.array_equal(a["keys"], keys) and np.array_equal(a["depth"], exp["depth"])


def test_accumulation_is_order_free():
    case, _exp = RC.expected_of("points_257")
    first, second = case["ops"]
    both = run_raw(case)
    swapped = run_raw(case, ops=[second, first])
    same(swapped, both, "two calls, swapped")
    # one call on the concatenation (both with colours: one payload kind per call)
    r = np.random.default_rng(4)
    a, b = first[1], dict(second[1], colors=r.integers(0, 256, (len(second[1]["pts"]), 3), dtype=np.uint8))
    b.pop("id_base")
    two = run_raw(case, ops=[("points", a), ("points", b)])
    one = run_raw(case, ops=[("points", dict(a, pts=np.concatenate([a["pts"], b["pts"]]), colors=np.concatenate([a["colors"], b["colors"]])))])
    same(one, two, "one call on the concatenation")
    # lines and points in either order
    wall, _e = RC.expected_of("wall")
    same(run_raw(wall, ops=wall["ops"][::-1]), run_raw(wall), "wall, reversed", fields=("keys", "rgba", "depth", "ids"))


def test_u8_and_f32_colours_give_the_same_keys():
    case, _exp = RC.expected_of("points_65")
    a = case["ops"][0][1]
    u8 = run_raw(case, ops=[("points", a)])
    f32 = run_raw(case, ops=[("points", dict(a, colors=(a["colors"].astype(np.float64) / 255.0).astype(np.float32)))])
    same(f32, u8, "fp32 colours k / 255 against uint8 k")


@pytest.mark.parametrize("name", list(RC.PLAN_REFUSED))
def test_plan_refusals(name):
    from vista_slam_amd import _lib, render
    args, msg = RC.PLAN_REFUSED[name]
    lib = _lib.load_raster()
    with pytest.raises(_lib.StaError, match=msg):
        _lib.check_raster(lib.sta_raster_plan(*args, (C.c_int64 * 3)()))
    with pytest.raises(ValueError, match=msg):
        render.Canvas("cuda:0", *args)


@pytest.mark.parametrize("name", list(RC.DRAW_REFUSED))
def test_draw_refusals(name):
    """a refused call launches nothing: the keys stay as they were"""
    import torch
    from vista_slam_amd import _lib
    kind, over, msg = RC.DRAW_REFUSED[name]
    lib = _lib.load_raster()
    base = dict(pts=np.array([[1, 1, 1], [2, 2, 1]], dtype=np.float32), **RC.UNIT) if kind == "points" else \
        dict(segs=np.array([[[0, 0, 1], [3, 3, 1]]], dtype=np.float32), colors=np.uint8([[1, 2, 3]]), **RC.UNIT)
    keys = _guarded(5 * 7 * 8)
    with pytest.raises(_lib.StaError, match=msg):
        _lib.check_raster(draw(lib, keys, 5, 7, 1, kind, dict(base, **over), None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (keys.cpu().numpy() == FILL).all()


def test_python_layer_equals_the_c_abi():
    import torch
    from vista_slam_amd import render
    for name in ("ssaa_2", "frusta_trajectory_graph", "point_size_3", "dropped"):
        case, exp = RC.expected_of(name)
        cv = render.Canvas("cuda:0", case["H"], case["W"], case["ssaa"])
        for kind, a in case["ops"]:
            cam = render.Camera(np.asarray(a.get("K", (1, 1, 0, 0)), dtype=np.float64), a.get("T", RC.IDENT), a.get("near", 1e-3), a.get("far", 1e4))
            if kind == "points":
                cv.points(cam, a["pts"], a.get("colors"), a.get("psize", 1), a.get("id_base", 0))
            else:
                cv.lines(cam, a["segs"], a["colors"], a.get("width", 1))
        assert np.array_equal(cv.keys.cpu().numpy().view(np.uint64), exp["keys"]), name
        assert np.array_equal(cv.image(case["background"]).cpu().numpy(), exp["rgba"]), name
        assert np.array_equal(cv.depth().cpu().numpy(), exp["depth"]), name
        assert np.array_equal(cv.ids().cpu().numpy().view(np.uint32), exp["ids"]), name
        assert list(cv.counters().values()) == exp["counters"].tolist(), name
        # the drawing methods allocate nothing when they are given the entry point's own tensors
        a = next(a for kind, a in case["ops"] if kind == "points") if name != "frusta_trajectory_graph" else None
        if a is not None and a.get("colors") is not None:
            pts, col = _up(np.asarray(a["pts"], dtype=np.float32)), _up(np.asarray(a["colors"]))
            cam = render.Camera(np.asarray(a["K"], dtype=np.float64), a["T"])
            torch.cuda.synchronize()
            before = torch.cuda.memory_stats()["allocation.all.allocated"]
            cv.clear().points(cam, pts, col)
            assert torch.cuda.memory_stats()["allocation.all.allocated"] == before, name
    # the scene through the named methods
    case, exp = RC.expected_of("frusta_trajectory_graph")
    poses, K, graph, lmd = RC.three_cameras()
    c = RC.overview_camera(case["H"], case["W"])
    cam = render.Camera(np.asarray(c["K"]), c["T"])
    cv = render.Canvas("cuda:0", case["H"], case["W"])
    cv.cameras(cam, poses, K, (64, 48), 0.3, (153, 204, 255)).trajectory(cam, poses, (255, 0, 0), line_width=2).view_graph(cam, graph, poses, lmd)
    assert np.array_equal(cv.keys.cpu().numpy().view(np.uint64), exp["keys"])
    cv.clear()
    assert (cv.keys.cpu().numpy().view(np.uint64) == RC.EMPTY).all() and cv.counters()["seen"] == 0


@pytest.fixture(scope="module")
def fe():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield m
    del m


@pytest.mark.parametrize("mode", ["topdown", "follow"])
def test_render_folder_equals_the_restatement(fe, tmp_path, mode):
    """A four-view 48x64 save_data_all folder of a procedural room with one mid-run snapshot.  Every PNG equals the restatement's, fed with
    the GPU's own world cloud of that frame (formats.world_pointcloud has its own tests and bound): colours / 1.5, frusta, edges, resolve."""
    import torch
    from vista_slam_amd import formats, render
    run = RC.room_run()
    folder, out = str(tmp_path / "run"), str(tmp_path / "frames")
    formats.save_data_all(fe, folder, poses=run["poses"], scales=run["scales"], depths=run["depths"], confs=run["confs"], intrinsics=run["intrinsics"],
                          imgs=torch.from_numpy(run["imgs"]), conf_thres=1.0, view_graph=run["view_graph"], loop_min_dist=run["loop_min_dist"],
                          view_names=[f"v{i}" for i in range(4)], save_ply=False)
    for i, (p, s) in run["snapshots"].items():
        np.save(f"{folder}/trajectory_{i}.npy", p)
        np.save(f"{folder}/scales_{i}.npy", s)
    H, W, ssaa = 48, 64, 2
    bg = (0, 0, 0, 0)
    paths = render.render_folder(fe, folder, out, mode=mode, H=H, W=W, ssaa=ssaa, point_size=2, background=bg)
    assert [os.path.basename(p) for p in paths] == [f"{v:04d}.png" for v in range(4)]
    images = np.load(f"{folder}/images.npy")
    imgs = torch.from_numpy(images).permute(0, 3, 1, 2) * 2.0 - 1.0
    top = render.Camera.fit(run["poses"], H, W, "topdown")
    K_out = [0.5 * min(H, W) / np.tan(np.deg2rad(30.0))] * 2 + [(W - 1) / 2.0, (H - 1) / 2.0]
    covered = 0
    for v in range(4):
        traj, scales = run["snapshots"][1] if v <= 1 else (run["poses"], run["scales"])
        cam = top if mode == "topdown" else render.Camera.from_pose(traj[v], K_out, render.follow_offset())
        c = dict(T=cam.w2c, K=cam.K, near=cam.near, far=cam.far)
        pts, col = formats.world_pointcloud(fe, run["depths"][:v + 1], scales[:v + 1], run["intrinsics"][:v + 1], traj[:v + 1], run["confs"][:v + 1],
                                            imgs[:v + 1], 1.0)
        keys = RC.new_keys(H, W, ssaa)
        RC.points(keys, ssaa, pts.cpu().numpy(), col.cpu().numpy() * np.float32(1.0 / 1.5), psize=2, **c)
        size = (run["depths"].shape[2], run["depths"].shape[1])
        if v > 0:
            fr = RC.camera_segments(traj[:v], run["intrinsics"][:v], size, 0.1)
            RC.lines(keys, ssaa, fr, np.tile(np.uint8(render.CAMERA_COLOR), (len(fr), 1)), **c)
        fr = RC.camera_segments(traj[v:v + 1], run["intrinsics"][v:v + 1], size, 1.0)
        RC.lines(keys, ssaa, fr, np.tile(np.uint8(render.CUR_CAMERA_COLOR), (len(fr), 1)), **c)
        RC.lines(keys, ssaa, *RC.view_graph_segments(run["view_graph"], traj, run["loop_min_dist"], upto=v + 1), **c)
        want = RC.resolve(keys, ssaa, bg)[0]
        got = render.read_png(paths[v])
        assert got.shape == (H, W, 4) and np.array_equal(got, want), (mode, v, int((got != want).any(axis=2).sum()))
        covered += int((want[..., 3] > 0).sum())
    assert covered > 4 * 100, "the frames are (nearly) empty: they prove nothing"


def test_render_map_and_ids(fe):
    """render_map on the arguments of an export: the colour image, and with imgs=None the id image, whose ids index the world cloud"""
    import torch
    from vista_slam_amd import formats, render
    run = RC.room_run()
    H, W = 48, 64
    cam = render.Camera.fit(run["poses"], H, W, "oblique")
    args = dict(depths=run["depths"], scales=run["scales"], intrinsics=run["intrinsics"], poses=run["poses"], confs=run["confs"], conf_thres=1.0)
    pts, col = formats.world_pointcloud(fe, imgs=torch.from_numpy(run["imgs"]), **args)
    c = dict(T=cam.w2c, K=cam.K, near=cam.near, far=cam.far)
    cv = render.render_map(fe, cam, imgs=torch.from_numpy(run["imgs"]), H=H, W=W, **args)
    keys = RC.new_keys(H, W, 1)
    cnt = RC.points(keys, 1, pts.cpu().numpy(), col.cpu().numpy(), **c)
    assert np.array_equal(cv.keys.cpu().numpy().view(np.uint64), keys) and list(cv.counters().values()) == cnt.tolist()
    ids = render.render_map(fe, cam, imgs=None, canvas=cv, **args).ids().cpu().numpy()
    keys = RC.new_keys(H, W, 1)
    RC.points(keys, 1, pts.cpu().numpy(), None, **c)
    assert np.array_equal(ids.view(np.uint32), RC.resolve(keys, 1)[2]) and (ids >= 0).sum() > 100 and ids.max() < len(pts)
