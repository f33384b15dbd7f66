"""Host only: the numpy restatement of include/sta_raster.h (tests/render_cases.py) against a second, naive statement - a scalar Python
loop per point, footprint pixel and line step that keeps the smaller key by explicit comparison, on Python floats (IEEE float64) - and
the properties the header promises: a segment inside the canvas leaves the 2-D clip bit-identical, the DDA's pixels form an 8-connected
chain between the end pixels within half a pixel (on each axis) of the float segment, every refusal of `plan`, and the PNG writer."""
import math
import struct

import numpy as np
import pytest

import render_cases as RC

EMPTY = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------ the naive statement
def f32_bits(z):
    return struct.unpack("<I", struct.pack("<f", z))[0]


def cam_of(T, p):
    T = np.asarray(T, dtype=np.float64).reshape(-1)[:12].tolist()
    x, y, z = float(p[0]), float(p[1]), float(p[2])
    return [((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3] for a in range(3)]


def proj(K, x, y, z, s):
    fx, fy, cx, cy = [float(v) for v in K]
    off = (s - 1) * 0.5
    return (fx * (x / z) + cx) * float(s) + off, (fy * (y / z) + cy) * float(s) + off


def put(keys, Hs, Ws, ix, iy, p, key):
    for y in range(iy - (p - 1) // 2, iy + p // 2 + 1):
        for x in range(ix - (p - 1) // 2, ix + p // 2 + 1):
            if 0 <= x < Ws and 0 <= y < Hs and key < keys[y][x]:
                keys[y][x] = key


def channel(c):
    c = float(np.float32(c))
    if c != c:
        return 0
    return int(round(min(max(c, 0.0), 1.0) * 255.0))          # round(): half to even, like rint


def naive_points(keys, Hs, Ws, s, pts, colors=None, id_base=0, psize=1, T=RC.IDENT, K=(1, 1, 0, 0), near=1e-3, far=1e4):
    cnt = [0, 0, 0, 0]
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    for i in range(len(pts)):
        cnt[0] += 1
        pc = cam_of(T, pts[i])
        if not all(math.isfinite(v) for v in pc):
            cnt[1] += 1
            continue
        if not (near <= pc[2] <= far):
            cnt[2] += 1
            continue
        us, vs = proj(K, pc[0], pc[1], pc[2], s)
        if not (math.isfinite(us) and math.isfinite(vs)):
            cnt[3] += 1
            continue
        fx, fy = math.floor(us + 0.5), math.floor(vs + 0.5)
        lo, hi = (psize - 1) // 2, psize // 2
        if not (fx + hi >= 0 and fx - lo <= Ws - 1 and fy + hi >= 0 and fy - lo <= Hs - 1):
            cnt[3] += 1
            continue
        if colors is None:
            pay = id_base + i
        elif np.asarray(colors).dtype == np.uint8:
            pay = (int(colors[i][0]) << 24) | (int(colors[i][1]) << 16) | (int(colors[i][2]) << 8) | 255
        else:
            pay = (channel(colors[i][0]) << 24) | (channel(colors[i][1]) << 16) | (channel(colors[i][2]) << 8) | 255
        put(keys, Hs, Ws, fx, fy, psize, (f32_bits(pc[2]) << 32) | pay)
    return cnt


def naive_clip(a, b, K, near, far, s, Hs, Ws):
    if not all(math.isfinite(v) for v in a + b):
        return None
    za, zb = a[2], b[2]
    if (za < near and zb < near) or (za > far and zb > far):
        return None
    ends = []
    for zend, own in ((za, a), (zb, b)):
        if near <= zend <= far:
            ends.append(own)
        else:
            plane = near if zend < near else far
            t = (plane - za) / (zb - za)
            ends.append([a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), plane])
    u0, v0 = proj(K, *ends[0], s)
    u1, v1 = proj(K, *ends[1], s)
    w0, w1 = 1.0 / ends[0][2], 1.0 / ends[1][2]
    if not all(abs(c) <= 2.0 ** 40 for c in (u0, v0, u1, v1)):
        return None
    dx, dy = u1 - u0, v1 - v0
    e0, e1 = 0.0, 1.0
    for p, q in ((-dx, u0 - (-8.5)), (dx, ((Ws - 0.5) + 8.0) - u0), (-dy, v0 - (-8.5)), (dy, ((Hs - 0.5) + 8.0) - v0)):
        if p == 0.0:
            if q < 0.0:
                return None
            continue
        r = q / p
        if p < 0.0:
            if r > e1:
                return None
            e0 = max(e0, r)
        else:
            if r < e0:
                return None
            e1 = min(e1, r)
    first = (u0, v0, w0) if e0 == 0.0 else (u0 + e0 * dx, v0 + e0 * dy, w0 + e0 * (w1 - w0))
    last = (u1, v1, w1) if e1 == 1.0 else (u0 + e1 * dx, v0 + e1 * dy, w0 + e1 * (w1 - w0))
    return first + last


def naive_lines(keys, Hs, Ws, s, segs, colors, width=1, T=RC.IDENT, K=(1, 1, 0, 0), near=1e-3, far=1e4):
    segs = np.asarray(segs, dtype=np.float32).reshape(-1, 2, 3)
    for j in range(len(segs)):
        c = naive_clip(cam_of(T, segs[j, 0]), cam_of(T, segs[j, 1]), K, float(near), float(far), s, Hs, Ws)
        if c is None:
            continue
        U0, V0, W0, U1, V1, W1 = c
        ax, ay, bx, by = [math.floor(v + 0.5) for v in (U0, V0, U1, V1)]
        n = max(abs(bx - ax), abs(by - ay))
        pay = (int(colors[j][0]) << 24) | (int(colors[j][1]) << 16) | (int(colors[j][2]) << 8) | 255
        for k in range(n + 1):
            t = k / n if n else 0.0
            x, y = math.floor((U0 + t * (U1 - U0)) + 0.5), math.floor((V0 + t * (V1 - V0)) + 0.5)
            put(keys, Hs, Ws, x, y, width, (f32_bits(1.0 / (W0 + t * (W1 - W0))) << 32) | pay)


def naive_resolve(keys, H, W, s, bg):
    rgba, depth, ids = np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.float32), np.zeros((H, W), np.uint32)
    for y in range(H):
        for x in range(W):
            block = [keys[y * s + sy][x * s + sx] for sy in range(s) for sx in range(s)]
            best = min(block)
            total = [0, 0, 0, 0]
            for k in block:
                p = k & 0xFFFFFFFF
                px = list(bg) if k == EMPTY else [p >> 24, (p >> 16) & 255, (p >> 8) & 255, (p & 255) if s == 1 else 255]
                total = [a + b for a, b in zip(total, px)]
            rgba[y, x] = [(v + s * s // 2) // (s * s) for v in total]
            depth[y, x] = np.inf if best == EMPTY else struct.unpack("<f", struct.pack("<I", best >> 32))[0]
            ids[y, x] = best & 0xFFFFFFFF
    return rgba, depth, ids


def naive_case(case):
    s = case["ssaa"]
    Hs, Ws = case["H"] * s, case["W"] * s
    keys = [[EMPTY] * Ws for _ in range(Hs)]
    cnt = np.zeros(4, dtype=np.uint64)
    for kind, a in case["ops"]:
        if kind == "points":
            cnt += np.array(naive_points(keys, Hs, Ws, s, **a), dtype=np.uint64)
        else:
            naive_lines(keys, Hs, Ws, s, **a)
    return np.array(keys, dtype=np.uint64), cnt, naive_resolve(keys, case["H"], case["W"], s, case["background"])


@pytest.mark.parametrize("name", list(RC.CASES))
def test_the_restatement_equals_the_naive_statement(name):
    case, exp = RC.expected_of(name)
    keys, cnt, (rgba, depth, ids) = naive_case(case)
    assert np.array_equal(keys, exp["keys"]), (name, np.argwhere(keys != exp["keys"])[:5])
    assert np.array_equal(cnt, exp["counters"]), (name, cnt, exp["counters"])
    assert np.array_equal(rgba, exp["rgba"]) and np.array_equal(depth, exp["depth"]) and np.array_equal(ids, exp["ids"]), name
    assert (exp["keys"] != RC.EMPTY).any(), f"{name} draws nothing: it proves nothing"


def test_the_cases_reach_what_they_are_named_for():
    e = RC.expected_of("depth_limits")[1]
    assert np.array_equal(e["depth"][0, :6] < np.inf, [True, False, True, True, True, False]) and e["counters"][2] == 2
    d = RC.expected_of("dropped")[1]["counters"]
    assert d[1] >= 8 and d[2] >= 4 and d[3] >= 2
    t = RC.expected_of("ties")[1]["rgba"]
    assert t[2, 2].tolist() == [3, 200, 7, 255] and t[2, 3].tolist() == [3, 200, 7, 255] and t[2, 4].tolist() == [250, 250, 250, 255]
    c = RC.expected_of("contention")[1]
    assert (c["keys"] != RC.EMPTY).sum() == 1 and c["depth"][2, 3] == 1.0
    b = RC.expected_of("pixel_boundaries")[1]["ids"]
    assert (b[:, 0] != 0xFFFFFFFF).any() and (b[:, -1] != 0xFFFFFFFF).any() and RC.expected_of("pixel_boundaries")[1]["counters"][3] > 0
    for s in (2, 4):
        a = RC.expected_of(f"ssaa_{s}")[1]["rgba"][..., 3]
        assert ((a > 40) & (a < 255)).any(), "no partly covered block"
    w = RC.expected_of("wall")[1]["rgba"]
    assert w[15, 5].tolist() == [128, 128, 128, 255] and w[15, 25].tolist() == [255, 0, 0, 255] and w[10, 5].tolist() == [0, 255, 0, 255]
    colours = RC.quantise_f32(RC.boundary_colours())
    assert len(np.unique(colours)) == 256


def test_u8_and_f32_colours_agree_on_the_lattice():
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(RC.quantise_f32((k.astype(np.float64) / 255.0).astype(np.float32)), k)
    assert np.array_equal(RC.quantise_f32(np.float32([np.nan, -3.0, 7.0, np.inf, -np.inf])), [0, 0, 255, 255, 0])


def _inside_segments(Hs, Ws, n=200, seed=1):
    r = np.random.default_rng(seed)
    z = r.uniform(0.5, 3.0, (n, 2))
    u, v = r.uniform(-8.0, Ws + 7.0, (n, 2)), r.uniform(-8.0, Hs + 7.0, (n, 2))
    return np.stack([u * z, v * z, z], axis=-1)


def test_a_segment_inside_the_window_leaves_the_clip_bit_identical():
    Hs, Ws = 17, 33
    for seg in _inside_segments(Hs, Ws):
        a, b = seg.astype(np.float32).astype(np.float64)
        out = RC.clip_segment(a, b, (1.0, 1.0, 0.0, 0.0), 0.25, 10.0, 1, Hs, Ws)
        u0, v0 = RC.project((1.0, 1.0, 0.0, 0.0), a[0], a[1], a[2], 1)
        u1, v1 = RC.project((1.0, 1.0, 0.0, 0.0), b[0], b[1], b[2], 1)
        want = np.array([u0, v0, 1.0 / a[2], u1, v1, 1.0 / b[2]])
        assert np.array_equal(np.array(out).view(np.uint64), want.view(np.uint64))


def test_dda_pixels_form_a_chain_within_half_a_pixel():
    Hs, Ws = 48, 64
    r = np.random.default_rng(2)
    segs = list(_inside_segments(Hs, Ws, 100, seed=3)) + [np.array([[x0, y0, 1.0], [x1, y1, 1.0]]) for x0, y0, x1, y1 in
                                                          r.uniform(-200, 300, (100, 4)).tolist() + [[0, 0, 63, 47], [5, 5, 5, 5], [3, 40, 60, 41], [10, 2, 11, 45]]]
    drawn = 0
    for seg in segs:
        c = RC.clip_segment(seg[0], seg[1], (1.0, 1.0, 0.0, 0.0), 0.25, 10.0, 1, Hs, Ws)
        if c is None:
            continue
        x, y, w = RC.dda(c)
        U0, V0, _W0, U1, V1, _W1 = c
        drawn += 1
        assert (x[0], y[0]) == (np.floor(U0 + 0.5), np.floor(V0 + 0.5)) and (x[-1], y[-1]) == (np.floor(U1 + 0.5), np.floor(V1 + 0.5))
        assert (np.abs(np.diff(x)) <= 1).all() and (np.abs(np.diff(y)) <= 1).all(), "not 8-connected"
        assert (np.maximum(np.abs(np.diff(x)), np.abs(np.diff(y))) == 1).all() or len(x) == 1, "a repeated pixel along the major axis"
        # every drawn pixel centre is within half a pixel (on both axes) of a point of the float segment: the one the step sampled
        t = np.arange(len(x)) / max(len(x) - 1, 1)
        fu, fv = U0 + t * (U1 - U0), V0 + t * (V1 - V0)
        assert (np.abs(x - fu) <= 0.5 + 1e-9).all() and (np.abs(y - fv) <= 0.5 + 1e-9).all()
        assert (w > 0).all()
    assert drawn > 100


@pytest.mark.parametrize("name", list(RC.PLAN_REFUSED))
def test_plan_refusals(name):
    from vista_slam_amd import render
    args, msg = RC.PLAN_REFUSED[name]
    with pytest.raises(ValueError, match=msg):
        render.plan(*args)
    with pytest.raises(ValueError, match=msg):
        RC.plan(*args)


def test_plan_sizes():
    from vista_slam_amd import render
    for H, W, s in ((1, 1, 1), (5, 7, 2), (2048, 2048, 4), (8192, 8192, 1), (480, 720, 2)):
        assert tuple(render.plan(H, W, s)) == RC.plan(H, W, s) == (H * s * W * s * 8, H * s, W * s)


def test_host_geometry_equals_its_restatement():
    from vista_slam_amd import render
    poses, K, graph, lmd = RC.three_cameras()
    assert np.array_equal(render.camera_segments(poses, K, (64, 48), 0.3), RC.camera_segments(poses, K, (64, 48), 0.3))
    assert render.camera_segments(poses, K, (64, 48), 0.3).shape == (24, 2, 3)
    assert np.array_equal(render.trajectory_segments(poses), RC.trajectory_segments(poses))
    for upto in (None, 2):
        a, b = render.view_graph_segments(graph, poses, lmd, upto), RC.view_graph_segments(graph, poses, lmd, upto)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    segs, cols = render.view_graph_segments(graph, poses, lmd)
    assert len(segs) == 3 and cols.tolist() == [[0, 0, 255], [255, 128, 0], [0, 0, 255]]
    assert (render.NEIGHBOR_EDGE_COLOR, render.LOOP_EDGE_COLOR) == (RC.NEIGHBOR_EDGE, RC.LOOP_EDGE)


def test_cameras_see_what_they_are_fitted_to():
    from vista_slam_amd import render
    H, W = 48, 64
    cam = render.Camera.look_at([0, 0, -2], [0, 0, 0], [0, -1, 0], 50.0, 50.0, H, W)
    assert np.allclose(cam.w2c, [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2]]) and cam.K.tolist() == [50.0, 50.0, 31.5, 23.5]
    pts = np.random.default_rng(0).uniform(-3, 5, (500, 3))
    for direction in ("topdown", "oblique"):
        c = render.Camera.fit(pts, H, W, direction)
        pc = RC.to_camera(c.w2c, pts.astype(np.float32))
        u, v = RC.project(c.K, pc[:, 0], pc[:, 1], pc[:, 2], 1)
        assert (pc[:, 2] >= c.near).all() and (pc[:, 2] <= c.far).all()
        assert (u >= 0).all() and (u <= W - 1).all() and (v >= 0).all() and (v <= H - 1).all(), direction
        assert np.allclose(c.w2c[:, :3] @ c.w2c[:, :3].T, np.eye(3)) and np.linalg.det(c.w2c[:, :3]) > 0
    top = render.Camera.fit(pts, H, W, "topdown")
    assert np.allclose(top.w2c[2, :3], [0, 1, 0]) and np.allclose(top.w2c[1, :3], [0, 0, -1])          # looks along +y; +z is up in the image
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[:, :3, 3] = pts[:3]
    assert np.allclose(render.Camera.fit(poses, H, W).w2c, render.Camera.fit(pts[:3], H, W).w2c)
    off = render.follow_offset()
    f = render.Camera.from_pose(poses[1], [50, 50, 31.5, 23.5], off)
    assert np.allclose(f.w2c, (off @ np.linalg.inv(poses[1]))[:3])


def test_png_round_trip(tmp_path):
    from vista_slam_amd import render
    r = np.random.default_rng(0)
    for shape in ((5, 7, 4), (1, 1, 4), (48, 64, 3)):
        img = r.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / f"a{shape[0]}.png")
        render.write_png(path, img)
        assert np.array_equal(render.read_png(path), img)
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(path) as im:
            assert im.mode == ("RGBA" if shape[2] == 4 else "RGB") and np.array_equal(np.asarray(im), img)
    with pytest.raises(ValueError):
        render.write_png(str(tmp_path / "b.png"), np.zeros((4, 4), np.uint8))
