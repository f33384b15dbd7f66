"""GPU: libsta_mesh.so (csrc/mesh.h) against the numpy restatement of its contract (tests/mesh_cases.py), through the C ABI into
pattern-filled buffers with guard regions behind every one, and the Python layer on top of it (render.Canvas.mesh, render_mesh,
mesh_depth, render_folder(mesh=); tsdf.vertex_normals, visible_triangles, cull_mesh, write_mesh_ply(normals=)).  Every comparison is
array_equal on keys, rgba, depth, ids, counters and normals.  The canvases are tiny; mesh_cases.CASES names them."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases as MC
import render_cases as RC
import test_render_gpu as TR
from test_render_gpu import FILL, GUARD, _guarded, _tail_untouched, _up, same

pytestmark = pytest.mark.gpu


def _dbl(a, n):
    return None if a is None else (C.c_double * n)(*[float(v) for v in a])


def draw_triangles(lib, keys, H, W, s, a, counters, st, over=None):
    """one triangles op through the C ABI into a work buffer of exactly the planned size plus a guard -> (return code, check)"""
    over = over or {}
    T, K, near, far = TR._cam(dict(a, **{k: over[k] for k in ("T", "K", "near", "far") if k in over}))
    verts = _up(np.asarray(a["verts"], dtype=np.float32).reshape(-1, 3))
    tris = _up(np.asarray(a["tris"], dtype=np.int32).reshape(-1, 3))
    col = a.get("colors")
    cold = _up(np.asarray(col, dtype=np.float32)) if col is not None else None
    nt, nv = over.get("nt", len(tris)), over.get("nv", len(verts))
    sizes = (C.c_int64 * 2)()
    if 0 <= nt < 2 ** 31 and 0 <= nv < 2 ** 31:
        assert lib.sta_mesh_plan(nt, nv, sizes) == 0 and tuple(sizes) == MC.plan(nt, nv)
    work = _guarded(int(sizes[0]))
    rc = lib.sta_mesh_triangles(keys.data_ptr(), over.get("H", H), W, over.get("ssaa", s), verts.data_ptr(), nv, tris.data_ptr(), nt,
                                cold.data_ptr() if cold is not None else None, _dbl(over.get("color", a.get("color")), 3), _dbl(over.get("light", a.get("light")), 4),
                                int(over.get("kind", a.get("kind", MC.ID))), int(over.get("cull", a.get("cull", 0))), int(over.get("id_base", a.get("id_base", 0))),
                                T, K, near, far, counters.data_ptr() if counters is not None else None, work.data_ptr(),
                                int(over.get("work_bytes", sizes[0])), st)
    return rc, lambda: _tail_untouched(work, int(sizes[0]), "work")


def run_raw(case, ops=None):
    """clear + every op + resolve through the C ABI -> dict of host arrays"""
    import torch
    from vista_slam_amd import _lib
    rl, ml = _lib.load_raster(), _lib.load_mesh()
    H, W, s = case["H"], case["W"], case["ssaa"]
    nbytes, Hs, Ws = RC.plan(H, W, s)
    keys = _guarded(nbytes)
    cnt = torch.zeros(64 + GUARD, dtype=torch.uint8, device="cuda")
    cnt[64:] = FILL
    st = torch.cuda.current_stream().cuda_stream
    _lib.check_raster(rl.sta_raster_clear(keys.data_ptr(), H, W, s, st))
    checks = []
    for kind, a in (case["ops"] if ops is None else ops):
        if kind == "triangles":
            rc, chk = draw_triangles(ml, keys, H, W, s, a, cnt, st)
            _lib.check_mesh(rc)
            checks.append(chk)
        else:
            _lib.check_raster(TR.draw(rl, keys, H, W, s, kind, a, None, st))
    rgba, depth, ids = _guarded(H * W * 4), _guarded(H * W * 4), _guarded(H * W * 4)
    bg = (C.c_uint8 * 4)(*case["background"])
    _lib.check_raster(rl.sta_raster_resolve(keys.data_ptr(), H, W, s, bg, rgba.data_ptr(), depth.data_ptr(), ids.data_ptr(), st))
    torch.cuda.synchronize()
    for buf, n, what in ((keys, nbytes, "keys"), (cnt, 64, "counters"), (rgba, H * W * 4, "rgba_out"), (depth, H * W * 4, "depth_out"), (ids, H * W * 4, "id_out")):
        _tail_untouched(buf, n, what)
    for chk in checks:
        chk()
    return {"keys": keys[:nbytes].cpu().numpy().view(np.uint64).reshape(Hs, Ws), "counters": cnt[:64].cpu().numpy().view(np.uint64),
            "rgba": rgba[:H * W * 4].cpu().numpy().reshape(H, W, 4), "depth": depth[:H * W * 4].cpu().numpy().view(np.float32).reshape(H, W),
            "ids": ids[:H * W * 4].cpu().numpy().view(np.uint32).reshape(H, W)}


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_against_the_restatement(name):
    case, exp = MC.expected_of(name)
    got = run_raw(case)
    print(f"[mesh] {name}: counters {got['counters'].tolist()}, {int((got['keys'] != RC.EMPTY).sum())} keys written")
    same(got, exp, name)
    again = run_raw(case)                                   # two runs are bit-identical
    same(again, got, name + " (second run)")


def test_the_cases_reach_what_they_are_named_for():
    c = {n: MC.expected_of(n)[1]["counters"] for n in ("sliver", "near_plane", "too_large", "bad_index_nan", "off_canvas", "sphere_inside_id_cull0",
                                                       "sphere_outside_id_cull1", "full_canvas_ssaa4", "no_triangles")}
    assert c["sliver"][MC.DEGENERATE] == 3 and c["bad_index_nan"][MC.BAD] == 5 and c["too_large"][MC.TOO_LARGE] == 3 and c["too_large"][MC.CLIPPED] == 1
    assert c["near_plane"][MC.BEHIND] == 2 and c["near_plane"][MC.CLIPPED] == 8 and c["off_canvas"][MC.OFF_CANVAS] == 2
    assert c["sphere_inside_id_cull0"][MC.CLIPPED] > 40 and c["sphere_outside_id_cull1"][MC.CULLED] > 500 and c["no_triangles"].sum() == 0
    full = MC.expected_of("full_canvas_ssaa4")[1]["keys"]
    assert full.shape == (192, 256) and (full != RC.EMPTY).all()
    far = MC.expected_of("far")[1]["keys"]
    assert 0 < (far != RC.EMPTY).sum() < 100
    co = MC.expected_of("coincident")[1]["ids"]
    assert set(np.unique(co)) == {3, 0xFFFFFFFF}, "of coincident triangles the smallest id wins"


def test_points_lines_and_triangles_share_the_canvas_in_any_order():
    a, b = MC.expected_of("mixed_ptl"), MC.expected_of("mixed_ltp")
    assert np.array_equal(a[1]["keys"], b[1]["keys"])
    ga, gb = run_raw(a[0]), run_raw(b[0])
    assert np.array_equal(ga["keys"], gb["keys"]) and np.array_equal(ga["keys"], a[1]["keys"])
    kinds = [{(k >> np.uint64(32)) for k in run_raw(a[0], ops=[op])["keys"].reshape(-1) if k != RC.EMPTY} for op in a[0]["ops"]]
    assert all(kinds), "one of the three draws nothing"


@pytest.mark.parametrize("name", list(MC.REFUSED))
def test_refusals(name):
    import torch
    from vista_slam_amd import _lib
    over, msg = MC.REFUSED[name]
    lib = _lib.load_mesh()
    a = dict(verts=np.array([[1, 1, 1], [5, 1, 1], [1, 4, 1]], dtype=np.float32), tris=np.array([[0, 1, 2]], dtype=np.int32), **MC.UNIT)
    keys = _guarded(5 * 7 * 8)
    rc, chk = draw_triangles(lib, keys, 5, 7, 1, a, None, torch.cuda.current_stream().cuda_stream, over)
    with pytest.raises(_lib.StaError, match=msg):
        _lib.check_mesh(rc)
    torch.cuda.synchronize()
    assert (keys.cpu().numpy() == FILL).all()
    chk()


def _normals_raw(v, t):
    import torch
    from vista_slam_amd import _lib
    lib = _lib.load_mesh()
    sizes = (C.c_int64 * 2)()
    _lib.check_mesh(lib.sta_mesh_plan(len(t), len(v), sizes))
    assert tuple(sizes) == MC.plan(len(t), len(v))
    work, out = _guarded(int(sizes[1])), _guarded(len(v) * 12)
    vd, td = _up(np.asarray(v, dtype=np.float32)), _up(np.asarray(t, dtype=np.int32).reshape(-1, 3))
    _lib.check_mesh(lib.sta_mesh_vertex_normals(vd.data_ptr(), len(v), td.data_ptr() if len(t) else None, len(t), out.data_ptr(), work.data_ptr(), int(sizes[1]),
                                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    _tail_untouched(work, int(sizes[1]), "work")
    _tail_untouched(out, len(v) * 12, "normals_out")
    return out[:len(v) * 12].cpu().numpy().view(np.float32).reshape(-1, 3)


@pytest.mark.parametrize("name", list(MC.NORMAL_MESHES))
def test_vertex_normals_against_the_restatement(name):
    v, t = MC.NORMAL_MESHES[name]()
    want = MC.vertex_normals(v, t)
    got = _normals_raw(v, t)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, int((got != want).any(axis=1).sum()))
    assert np.array_equal(_normals_raw(v, t).view(np.uint32), got.view(np.uint32)), "two calls give the same bits"


def test_vertex_normals_refusals():
    from vista_slam_amd import _lib
    lib = _lib.load_mesh()
    for args, msg in (((None, 3, None, 2 ** 31 // 3 + 1, None, None, 0, None), r"3 \* nt must be below 2\^31"), ((None, -1, None, 0, None, None, 0, None), r"nv must be in"),
                      ((None, 3, None, 1, None, None, 100, None), r"work of 100 bytes, 3072 needed for 1 triangles")):
        with pytest.raises(_lib.StaError, match=msg):
            _lib.check_mesh(lib.sta_mesh_vertex_normals(*args))


# ------------------------------------------------------------------------------------------ the Python layer
def _camera(c):
    from vista_slam_amd import render
    return render.Camera(np.asarray(c["K"], dtype=np.float64), c["T"], c.get("near", 1e-3), c.get("far", 1e4))


def _mesh_of(v, t, col):
    from vista_slam_amd import tsdf
    return tsdf.Mesh(_up(v), _up(col) if col is not None else None, _up(t))


def test_canvas_mesh_equals_the_c_abi():
    """colour, normal and id modes, every cull, points and lines on the same canvas; "shaded" (the light at the camera's centre) is held
    by test_render_mesh_on_the_room"""
    from vista_slam_amd import render
    modes = {MC.ID: "id", MC.NORMAL: "normal", MC.COLOR: "color"}
    for name in ("sphere_inside_color_cull0", "sphere_outside_normal_cull1", "sphere_outside_id_cull2", "near_plane", "mixed_ptl"):
        case, exp = MC.expected_of(name)
        cv = render.Canvas("cuda:0", case["H"], case["W"], case["ssaa"])
        for kind, a in case["ops"]:
            cam = _camera(a)
            if kind == "points":
                cv.points(cam, a["pts"], a.get("colors"), a.get("psize", 1), a.get("id_base", 0))
            elif kind == "lines":
                cv.lines(cam, a["segs"], a["colors"], a.get("width", 1))
            else:
                assert a.get("light") is None
                cv.mesh(cam, a["verts"], a["tris"], a.get("colors"), mode=modes[a.get("kind", MC.ID)], cull=("none", "back", "front")[a.get("cull", 0)],
                        id_base=a.get("id_base", 0))
        assert np.array_equal(cv.keys.cpu().numpy().view(np.uint64), exp["keys"]), name
        assert np.array_equal(cv.image(case["background"]).cpu().numpy(), exp["rgba"]), name
        assert list(cv.mesh_counters().values()) == exp["counters"].tolist(), name


def test_canvas_mesh_refusals():
    from vista_slam_amd import render
    canvas, camera = render.Canvas("cuda:0", 5, 7), _camera(MC.UNIT)
    tri = (np.array([[1, 1, 1], [5, 1, 1], [1, 4, 1]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32))
    with pytest.raises(ValueError, match="mode must be one of"):
        canvas.mesh(camera, *tri, mode="wire")
    with pytest.raises(ValueError, match="cull must be one of"):
        canvas.mesh(camera, *tri, cull="both")
    with pytest.raises(ValueError, match=r"would reach 2\^32 - 1"):
        canvas.mesh(camera, *tri, mode="id", id_base=2 ** 32 - 1)
    assert (canvas.keys.cpu().numpy().view(np.uint64) == RC.EMPTY).all()


@pytest.fixture(scope="module")
def room():
    v, t, col = MC.room_mesh()
    H, W = 24, 32
    cams = [MC.cam(H, W, 20.0, (0.1, 0.2, -1.9), (0.25, -0.125, 0.5), near=0.05, far=50.0), MC.cam(H, W, 14.0, (-1.5, -1.0, 1.5), (0.25, -0.125, 0.5), near=0.05, far=50.0)]
    return v, t, col, H, W, cams


def _eye(c):
    T = np.asarray(c["T"], dtype=np.float64)
    return -np.linalg.solve(T[:, :3], T[:, 3])


def test_render_mesh_on_the_room(room):
    from vista_slam_amd import render
    v, t, col, H, W, cams = room
    mesh = _mesh_of(v, t, col)
    poses, K, graph, lmd = RC.three_cameras()
    for s, c in ((1, cams[0]), (2, cams[1])):
        img = render.render_mesh("cuda:0", _camera(c), mesh, H=H, W=W, ssaa=s, mode="shaded", cull="none", background=RC.BG, poses=poses, intrinsics=K, size=(64, 48),
                                 view_graph=graph, loop_min_dist=lmd, ambient=0.25)
        keys = RC.new_keys(H, W, s)
        cnt = MC.triangles(keys, s, v, t, colors=col, kind=MC.COLOR, light=tuple(_eye(c)) + (0.25,), **c)
        fr = RC.camera_segments(poses, K, (64, 48), 0.1)
        RC.lines(keys, s, fr, np.tile(np.uint8(render.CAMERA_COLOR), (len(fr), 1)), **c)
        tr = RC.trajectory_segments(poses)
        RC.lines(keys, s, tr, np.tile(np.uint8(render.TRAJECTORY_COLOR), (len(tr), 1)), **c)
        RC.lines(keys, s, *RC.view_graph_segments(graph, poses, lmd), **c)
        want = RC.resolve(keys, s, RC.BG)[0]
        assert np.array_equal(img.cpu().numpy(), want), (s, int((img.cpu().numpy() != want).any(axis=2).sum()))
        assert (keys != RC.EMPTY).sum() > 200 * s * s and cnt[MC.CLIPPED] > 0
    # without colours: the uniform grey of the keyword
    grey = render.render_mesh("cuda:0", _camera(cams[0]), _mesh_of(v, t, None), H=H, W=W, mode="color", background=RC.BG).cpu().numpy()
    keys = RC.new_keys(H, W, 1)
    MC.triangles(keys, 1, v, t, kind=MC.COLOR, color=MC.GREY, **cams[0])
    assert np.array_equal(grey, RC.resolve(keys, 1, RC.BG)[0])


def test_mesh_depth_visible_triangles_and_cull_mesh(room):
    from vista_slam_amd import render, tsdf
    v, t, col, H, W, cams = room
    mesh = _mesh_of(v, t, col)
    seen = np.zeros(len(t), dtype=bool)
    for c in cams:
        keys = RC.new_keys(H, W, 1)
        MC.triangles(keys, 1, v, t, kind=MC.ID, **c)
        _, depth, ids = RC.resolve(keys, 1)
        got = render.mesh_depth("cuda:0", mesh, _camera(c), H, W).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), depth.view(np.uint32)) and np.isfinite(got).sum() > 200 and np.isinf(got).any()
        seen[ids[ids != 0xFFFFFFFF]] = True
    vis = tsdf.visible_triangles("cuda:0", mesh, [_camera(c) for c in cams], H, W)
    assert vis.dtype.is_floating_point is False and np.array_equal(vis.cpu().numpy(), seen) and 100 < seen.sum() < len(t) // 4
    small = tsdf.cull_mesh(mesh, vis)
    used = np.unique(t[seen])
    assert np.array_equal(small.vertices.cpu().numpy(), v[used]) and np.array_equal(small.colors.cpu().numpy(), col[used])
    assert np.array_equal(small.triangles.cpu().numpy(), np.searchsorted(used, t[seen]).astype(np.int32))
    for c in cams:                                           # the culled mesh is what those cameras saw: the same depth maps
        assert np.array_equal(render.mesh_depth("cuda:0", small, _camera(c), H, W).cpu().numpy(), render.mesh_depth("cuda:0", mesh, _camera(c), H, W).cpu().numpy())


def test_vertex_normals_into_a_ply(room, tmp_path):
    from vista_slam_amd import tsdf
    v, t, col, *_ = room
    mesh = _mesh_of(v, t, col)
    n = tsdf.vertex_normals(mesh)
    want = MC.vertex_normals(v, t)
    assert np.array_equal(n.cpu().numpy().view(np.uint32), want.view(np.uint32))
    path = str(tmp_path / "mesh.ply")
    tsdf.write_mesh_ply(path, mesh, normals=n)
    rec, tris = tsdf.read_mesh_ply(path)
    assert np.array_equal(tris, t) and np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1), want.astype(np.float64))
    back = tsdf.mesh_from_ply(path)
    assert np.array_equal(back.vertices.cpu().numpy(), v) and np.array_equal(back.triangles.cpu().numpy(), t)


def test_render_folder_without_a_mesh_is_what_it_was(tmp_path):
    """the comparison of tests/test_render_gpu.py itself: every PNG against the restatement's keys of the cloud, the frusta and the edges"""
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    TR.test_render_folder_equals_the_restatement(m, tmp_path, "topdown")


def test_render_folder_with_a_mesh(room, tmp_path):
    import torch
    from vista_slam_amd import formats, render, tsdf
    from vista_slam_amd import weights as Wt
    from vista_slam_amd.sta_frontend import STAFrontend
    fe = STAFrontend(Wt.TINY, "cuda:0").load_procedural(seed=43)
    v, t, col, *_ = room
    run = RC.room_run()
    folder, out = str(tmp_path / "run"), str(tmp_path / "frames")
    formats.save_data_all(fe, folder, poses=run["poses"], scales=run["scales"], depths=run["depths"], confs=run["confs"], intrinsics=run["intrinsics"],
                          imgs=torch.from_numpy(run["imgs"]), conf_thres=1.0, view_graph=run["view_graph"], loop_min_dist=run["loop_min_dist"],
                          view_names=[f"v{i}" for i in range(4)], save_ply=False)
    ply = str(tmp_path / "mesh.ply")
    tsdf.write_mesh_ply(ply, _mesh_of(v, t, col))
    rec, _ = tsdf.read_mesh_ply(ply)
    col8 = (np.stack([rec["red"], rec["green"], rec["blue"]], 1).astype(np.float32) / np.float32(255.0))
    H, W, ssaa, bg = 24, 32, 2, (0, 0, 0, 0)
    paths = render.render_folder(fe, folder, out, mode="follow", H=H, W=W, ssaa=ssaa, background=bg, mesh=ply, mesh_cull="back")
    K_out = [0.5 * min(H, W) / np.tan(np.deg2rad(30.0))] * 2 + [(W - 1) / 2.0, (H - 1) / 2.0]
    size = (run["depths"].shape[2], run["depths"].shape[1])
    for vw in (0, 3):
        traj = run["poses"]
        cam = render.Camera.from_pose(traj[vw], K_out, render.follow_offset())
        c = dict(T=cam.w2c, K=cam.K, near=cam.near, far=cam.far)
        keys = RC.new_keys(H, W, ssaa)
        MC.triangles(keys, ssaa, v, t, colors=col8, kind=MC.COLOR, cull=MC.CULL_BACK, light=tuple(_eye(c)) + (0.3,), **c)
        if vw > 0:
            fr = RC.camera_segments(traj[:vw], run["intrinsics"][:vw], size, 0.1)
            RC.lines(keys, ssaa, fr, np.tile(np.uint8(render.CAMERA_COLOR), (len(fr), 1)), **c)
        fr = RC.camera_segments(traj[vw:vw + 1], run["intrinsics"][vw:vw + 1], size, 1.0)
        RC.lines(keys, ssaa, fr, np.tile(np.uint8(render.CUR_CAMERA_COLOR), (len(fr), 1)), **c)
        RC.lines(keys, ssaa, *RC.view_graph_segments(run["view_graph"], traj, run["loop_min_dist"], upto=vw + 1), **c)
        got = render.read_png(paths[vw])
        want = RC.resolve(keys, ssaa, bg)[0]
        assert np.array_equal(got, want), (vw, int((got != want).any(axis=2).sum()))
        assert (want[..., 3] > 0).sum() > 50
