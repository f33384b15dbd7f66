"""The yardstick of the headless rasteriser: a vectorised numpy restatement of include/sta_raster.h (every floating-point operation is
one numpy float64 ufunc call in the header's order, so nothing is contracted), the host geometry of vista_slam_amd/render.py restated
(frusta, trajectory, view-graph edges), and the case builders of tests/test_render_gpu.py.  Host-only importable.

It is NOT Open3D (not available): square footprints, this DDA, box supersampling, ties to the smaller payload - DESIGN.md section 9.

A case is {"H", "W", "ssaa", "background", "ops"}; an op is ("points", {...}) or ("lines", {...}) with the arguments of the entry point.
`expected_of(name)` -> (case, {"keys", "rgba", "depth", "ids", "counters"}), computed once per process and never changed."""
import functools

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_DIM, MAX_SIZE, MARGIN = 8192, 8, 8
MIN_NEAR, MAX_FAR, MAX_COORD = 1e-30, 1e30, 2.0 ** 40
IDENT = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


# ------------------------------------------------------------------------------------------ the contract
def plan(H, W, ssaa):
    """sta_raster_plan: (bytes, Hs, Ws); its refusals as ValueError with the library's text."""
    if H < 1 or W < 1:
        raise ValueError(f"raster_plan: H and W must be >= 1 (got {H} x {W})")
    if ssaa not in (1, 2, 4):
        raise ValueError(f"raster_plan: ssaa must be 1, 2 or 4 (got {ssaa})")
    if H * ssaa > MAX_DIM or W * ssaa > MAX_DIM:
        raise ValueError(f"raster_plan: {H} x {W} at ssaa {ssaa} is a key buffer of {H * ssaa} x {W * ssaa}, at most {MAX_DIM} per axis")
    return H * ssaa * W * ssaa * 8, H * ssaa, W * ssaa


def new_keys(H, W, ssaa):
    return np.full((H * ssaa, W * ssaa), EMPTY, dtype=np.uint64)


def to_camera(T, p):
    """pc = ((T0*x + T1*y) + T2*z) + T3 per axis on double(p); p [...,3] float32 -> [...,3] float64"""
    T = np.asarray(T, dtype=np.float64).reshape(-1)[:12].reshape(3, 4)
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=-1)


def project(K, x, y, z, s):
    fx, fy, cx, cy = [np.float64(v) for v in K]
    off = np.float64((s - 1) * 0.5)
    with np.errstate(all="ignore"):
        u = fx * (x / z) + cx
        v = fy * (y / z) + cy
        return u * np.float64(s) + off, v * np.float64(s) + off


def depth_bits(z):
    with np.errstate(all="ignore"):
        return np.asarray(z, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)


def pack_u8(c):
    c = np.asarray(c, dtype=np.uint8).astype(np.uint64)
    return (c[..., 0] << np.uint64(24)) | (c[..., 1] << np.uint64(16)) | (c[..., 2] << np.uint64(8)) | np.uint64(255)


def quantise_f32(c):
    d = np.asarray(c, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        q = np.rint(np.minimum(np.maximum(d, 0.0), 1.0) * 255.0)
    return np.where(np.isnan(d), 0.0, q).astype(np.uint8)


def splat(keys, ix, iy, key, p):
    """the footprint of size p around integer pixels (ix, iy): the minimum with `key` at every footprint pixel on the canvas"""
    Hs, Ws = keys.shape
    flat = keys.reshape(-1)
    for dy in range(-((p - 1) // 2), p // 2 + 1):
        for dx in range(-((p - 1) // 2), p // 2 + 1):
            x, y = ix + dx, iy + dy
            ok = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
            np.minimum.at(flat, (y[ok] * Ws + x[ok]).astype(np.int64), key[ok])


def points(keys, ssaa, pts, colors=None, id_base=0, psize=1, T=IDENT, K=(1, 1, 0, 0), near=1e-3, far=1e4):
    """sta_raster_points on keys [Hs,Ws] in place -> counters [4] uint64"""
    Hs, Ws = keys.shape
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    M = len(pts)
    pc = to_camera(T, pts)
    finite = np.isfinite(pc).all(axis=1)
    z = pc[:, 2]
    with np.errstate(all="ignore"):
        inz = finite & (near <= z) & (z <= far)
        us, vs = project(K, pc[:, 0], pc[:, 1], z, ssaa)
        fx, fy = np.floor(us + 0.5), np.floor(vs + 0.5)
        lo, hi = float((psize - 1) // 2), float(psize // 2)
        on = (fx + hi >= 0.0) & (fx - lo <= float(Ws - 1)) & (fy + hi >= 0.0) & (fy - lo <= float(Hs - 1))
    keep = inz & on
    counters = np.array([M, (~finite).sum(), (finite & ~inz).sum(), (inz & ~on).sum()], dtype=np.uint64)
    if colors is None:
        assert id_base >= 0 and id_base + M <= 2 ** 32 - 1
        payload = (np.uint64(id_base) + np.arange(M, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    elif np.asarray(colors).dtype == np.uint8:
        payload = pack_u8(colors)
    else:
        payload = pack_u8(quantise_f32(colors))
    key = (depth_bits(z) << np.uint64(32)) | payload
    splat(keys, fx[keep].astype(np.int64), fy[keep].astype(np.int64), key[keep], psize)
    return counters


def clip_segment(a, b, K, near, far, ssaa, Hs, Ws):
    """camera-space ends a, b [3] float64 -> None (dropped) or (U0, V0, W0, U1, V1, W1), float64 scalars"""
    f = np.float64
    a, b = [f(v) for v in a], [f(v) for v in b]
    near, far = f(near), f(far)
    with np.errstate(all="ignore"):
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            return None
        za, zb = a[2], b[2]
        dz = zb - za
        if (za < near and zb < near) or (za > far and zb > far):
            return None
        ends = []
        for zend, own in ((za, a), (zb, b)):
            if zend < near or zend > far:
                plane = near if zend < near else far
                t = (plane - za) / dz
                ends.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), plane))
            else:
                ends.append(tuple(own))
        (x0, y0, z0), (x1, y1, z1) = ends
        us0, vs0 = project(K, x0, y0, z0, ssaa)
        us1, vs1 = project(K, x1, y1, z1, ssaa)
        w0, w1 = f(1.0) / z0, f(1.0) / z1
        if not all(abs(c) <= MAX_COORD for c in (us0, vs0, us1, vs1)):          # (a NaN fails it)
            return None
        xmin, xmax = f(-0.5) - f(MARGIN), (f(Ws) - f(0.5)) + f(MARGIN)
        ymin, ymax = f(-0.5) - f(MARGIN), (f(Hs) - f(0.5)) + f(MARGIN)
        dx, dy = us1 - us0, vs1 - vs0
        e0, e1 = f(0.0), f(1.0)
        for p, q in ((-dx, us0 - xmin), (dx, xmax - us0), (-dy, vs0 - ymin), (dy, ymax - vs0)):
            if p == 0.0:
                if q < 0.0:
                    return None
            elif p < 0.0:
                r = q / p
                if r > e1:
                    return None
                if r > e0:
                    e0 = r
            else:
                r = q / p
                if r < e0:
                    return None
                if r < e1:
                    e1 = r
        dw = w1 - w0
        U0, V0, W0 = (us0, vs0, w0) if e0 == 0.0 else (us0 + e0 * dx, vs0 + e0 * dy, w0 + e0 * dw)
        U1, V1, W1 = (us1, vs1, w1) if e1 == 1.0 else (us0 + e1 * dx, vs0 + e1 * dy, w0 + e1 * dw)
        return U0, V0, W0, U1, V1, W1


def dda(clipped):
    """-> (x [n+1] float64 pixel columns, y, w) of the DDA over a clipped segment, or None when an end pixel is out of range"""
    U0, V0, W0, U1, V1, W1 = clipped
    with np.errstate(all="ignore"):
        ends = [np.floor(c + 0.5) for c in (U0, V0, U1, V1)]
        if not all(-16.0 <= e < 8192.0 + 16.0 for e in ends):
            return None
        ax, ay, bx, by = [int(e) for e in ends]
        n = max(abs(bx - ax), abs(by - ay))
        k = np.arange(n + 1, dtype=np.float64)
        t = k / np.float64(n) if n > 0 else np.zeros(1)
        x = np.floor((U0 + t * (U1 - U0)) + 0.5)
        y = np.floor((V0 + t * (V1 - V0)) + 0.5)
        w = W0 + t * (W1 - W0)
    return x, y, w


def lines(keys, ssaa, segs, colors, width=1, T=IDENT, K=(1, 1, 0, 0), near=1e-3, far=1e4):
    """sta_raster_lines on keys in place"""
    Hs, Ws = keys.shape
    segs = np.asarray(segs, dtype=np.float32).reshape(-1, 2, 3)
    pc = to_camera(T, segs)
    payload = pack_u8(np.asarray(colors, dtype=np.uint8).reshape(-1, 3))
    for j in range(len(segs)):
        c = clip_segment(pc[j, 0], pc[j, 1], K, near, far, ssaa, Hs, Ws)
        steps = dda(c) if c is not None else None
        if steps is None:
            continue
        x, y, w = steps
        with np.errstate(all="ignore"):
            key = (depth_bits(1.0 / w) << np.uint64(32)) | payload[j]
        splat(keys, x.astype(np.int64), y.astype(np.int64), key, width)


def resolve(keys, ssaa, background=(255, 255, 255, 255)):
    """sta_raster_resolve -> (rgba [H,W,4] uint8, depth [H,W] float32, ids [H,W] uint32)"""
    Hs, Ws = keys.shape
    s = ssaa
    H, W = Hs // s, Ws // s
    blocks = keys.reshape(H, s, W, s).transpose(0, 2, 1, 3).reshape(H, W, s * s)
    best = blocks.min(axis=2)
    empty = blocks == EMPTY
    pay = (blocks & np.uint64(0xFFFFFFFF)).astype(np.int64)
    bg = np.asarray(background, dtype=np.int64)
    chans = [pay >> 24, (pay >> 16) & 255, (pay >> 8) & 255, (pay & 255) if s == 1 else np.full_like(pay, 255)]
    rgba = np.stack([(np.where(empty, bg[c], chans[c]).sum(axis=2) + (s * s) // 2) // (s * s) for c in range(4)], axis=-1).astype(np.uint8)
    depth = (best >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    depth[best == EMPTY] = np.inf
    ids = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return rgba, depth, ids


def run_case(case):
    keys = new_keys(case["H"], case["W"], case["ssaa"])
    counters = np.zeros(4, dtype=np.uint64)
    for kind, a in case["ops"]:
        if kind == "points":
            counters += points(keys, case["ssaa"], **a)
        else:
            lines(keys, case["ssaa"], **a)
    rgba, depth, ids = resolve(keys, case["ssaa"], case["background"])
    return {"keys": keys, "rgba": rgba, "depth": depth, "ids": ids, "counters": counters}


# ------------------------------------------------------------------------------------------ the host geometry of render.py, restated
FRUSTUM_LINES = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1))


def camera_segments(poses, intrinsics, size, scale):
    """The eight segments of Open3D's create_camera_visualization per camera: the centre to the four image corners at depth `scale`, and the
    rectangle.  poses [N,4,4] camera-to-world, intrinsics [N,3,3] or [3,3], size (width_px, height_px) -> [N*8,2,3] float32"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    Ks = np.broadcast_to(np.asarray(intrinsics, dtype=np.float64), (len(poses), 3, 3))
    w, h = float(size[0]), float(size[1])
    out = []
    for c2w, Kc in zip(poses, Ks):
        corners = np.array([[0, 0, 1], [w, 0, 1], [w, h, 1], [0, h, 1]], dtype=np.float64)
        local = np.concatenate([np.zeros((1, 3)), (np.linalg.inv(Kc) @ corners.T).T * float(scale)])
        world = local @ c2w[:3, :3].T + c2w[:3, 3]
        out.append(np.stack([np.stack([world[i], world[j]]) for i, j in FRUSTUM_LINES]))
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 2, 3), np.float32)


def trajectory_segments(poses):
    c = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)[:, :3, 3]
    return np.stack([c[:-1], c[1:]], axis=1).astype(np.float32)


NEIGHBOR_EDGE, LOOP_EDGE = (0, 0, 255), (255, 128, 0)          # video.py:163-164: [0, 0, 1.0] and [1, 0.5, 0] (0.5 * 255 rounds to even: 128)


def view_graph_segments(view_graph, poses, loop_min_dist, upto=None):
    """video.py:162-188 for every view v (< upto): an edge to each neighbour nv <= v, orange when |v - nv| >= loop_min_dist, else blue"""
    c = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)[:, :3, 3]
    segs, cols = [], []
    for v in sorted(view_graph):
        if upto is not None and v >= upto:
            continue
        for nv in view_graph[v]:
            if nv > v:
                continue
            segs.append(np.stack([c[v], c[nv]]))
            cols.append(LOOP_EDGE if abs(v - nv) >= loop_min_dist else NEIGHBOR_EDGE)
    return np.asarray(segs, dtype=np.float32).reshape(-1, 2, 3), np.asarray(cols, dtype=np.uint8).reshape(-1, 3)


# ------------------------------------------------------------------------------------------ cases
BG = (10, 20, 30, 40)
UNIT = dict(T=IDENT, K=(1.0, 1.0, 0.0, 0.0))        # z = 1 puts a point at the pixel coordinate (x, y) exactly


def _case(H, W, ops, ssaa=1, background=(255, 255, 255, 255)):
    return {"H": H, "W": W, "ssaa": ssaa, "background": background, "ops": ops}


def rotation(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def view_camera(H, W, seed=0):
    """a non-trivial camera: rotated, translated, focal length of about the canvas"""
    R = rotation((0.3, 1.0, -0.2), 12.0 + seed)
    T = np.concatenate([R, np.array([[0.05], [-0.1], [0.4]])], axis=1)
    return dict(T=T, K=(0.9 * W, 0.8 * W, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.125))


def random_points(M, seed, spread=1.2):
    r = np.random.default_rng(seed)
    p = np.stack([r.uniform(-spread, spread, M), r.uniform(-spread, spread, M), r.uniform(0.3, 4.0, M)], axis=1)
    return p.astype(np.float32)


def _count_case(M):
    H, W = (48, 64) if M > 1000 else (17, 33)
    cam = view_camera(H, W)
    pts = random_points(M, 100 + M)
    r = np.random.default_rng(M)
    ops = [("points", dict(pts=pts, colors=r.integers(0, 256, (M, 3), dtype=np.uint8), near=0.5, far=3.5, **cam)),
           ("points", dict(pts=random_points(M, 200 + M), colors=None, id_base=7, near=0.5, far=3.5, **cam))]
    return _case(H, W, ops)


def _grid_case():
    H, W = 5, 7
    xs = [-1.5, -0.5, W - 1.5, W - 0.5, 2.0, 2.5, 2.4999998]
    ys = [-1.5, -0.5, H - 1.5, H - 0.5, 1.0, 1.5]
    pts = np.array([[x, y, 1.0] for x in xs for y in ys], dtype=np.float32)
    return _case(H, W, [("points", dict(pts=pts, **UNIT))])


def _depth_limit_case():
    near, far = np.float32(0.5), np.float32(2.0)
    zs = [near, np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(9)), far, np.nextafter(far, np.float32(0)),
          np.nextafter(far, np.float32(9))]
    pts = np.array([[float(i) * float(z), 0.0, float(z)] for i, z in enumerate(zs)], dtype=np.float32)     # pixel i of row 0 (x / z rounds to i)
    return _case(1, 7, [("points", dict(pts=pts, near=0.5, far=2.0, **UNIT))])


def _dropped_case():
    n, i = np.nan, np.inf
    pts = np.array([[1, 1, 1], [1, 1, 0], [1, 1, -1], [n, 1, 1], [1, n, 1], [1, 1, n], [i, 1, 1], [1, -i, 1], [1, 1, i], [1, 1, -i],
                    [2, 1, 1], [3e38, 1, 1], [100, 1, 1], [1, -100, 1], [2, 2, 1e-4], [2, 2, 2e4]], dtype=np.float32)
    T = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    big = np.array([[3e38, 3e38, 1]], dtype=np.float32)                 # finite input, finite matrix: the camera coordinate overflows to +inf
    ops = [("points", dict(pts=pts, T=T, K=(1.0, 1.0, 0.0, 0.0))),
           ("points", dict(pts=big, T=np.array([[1e308, 1e308, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]), K=(1.0, 1.0, 0.0, 0.0)))]
    return _case(5, 7, ops)


def _tie_case():
    pts = np.array([[3, 3, 1.5], [3, 3, 1.5], [4.5, 3, 1.5], [4.5, 3, 1.5], [6, 3, 1.5], [6, 3, 1.5000001]], dtype=np.float32)      # pixels (2..4, 2)
    col = np.array([[9, 0, 0], [3, 200, 7], [3, 200, 7], [9, 0, 0], [250, 250, 250], [1, 1, 1]], dtype=np.uint8)
    return _case(5, 7, [("points", dict(pts=pts, colors=col, **UNIT))])


def contention_points(seed=5, n=4096):
    r = np.random.default_rng(seed)
    z = r.choice(np.array([1.0, 1.25, 1.5, 2.0, 3.0]), n)
    return np.stack([3.0 * z, 2.0 * z, z], axis=1).astype(np.float32)            # all on pixel (3, 2)


def _contention_case():
    return _case(5, 7, [("points", dict(pts=contention_points(), colors=None, **UNIT))])


def _size_case(p):
    H, W = 5, 7
    at = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (3, 0), (3, H - 1), (0, 2), (W - 1, 2), (3, 2)]
    at += [(-d, 2) for d in range(1, p + 2)] + [(W - 1 + d, 2) for d in range(1, p + 2)]
    at += [(3, -d) for d in range(1, p + 2)] + [(3, H - 1 + d) for d in range(1, p + 2)] + [(-2, -2), (W + 1, H + 1)]
    pts = np.array([[x * (1 + 0.25 * i), y * (1 + 0.25 * i), 1 + 0.25 * i] for i, (x, y) in enumerate(at)], dtype=np.float32)
    return _case(H, W, [("points", dict(pts=pts, colors=None, id_base=1000, psize=p, **UNIT))])


def boundary_colours():
    k = np.arange(0, 256, dtype=np.float64)
    c = np.concatenate([k / 255.0, (k + 0.5) / 255.0, [np.nan, -1.0, 2.0, np.inf, -np.inf, -0.0, 1e-9]]).astype(np.float32)
    c = np.concatenate([c, np.nextafter(c[256:512], np.float32(0)), np.nextafter(c[256:512], np.float32(2))])
    n = (len(c) + 2) // 3 * 3
    return np.resize(c, n).reshape(-1, 3)


def _colour_case():
    col = boundary_colours()
    M = len(col)
    W, H = 33, (M + 32) // 33
    pts = np.array([[i % W, i // W, 1.0] for i in range(M)], dtype=np.float32)
    return _case(H, W, [("points", dict(pts=pts, colors=col, **UNIT))])


def _ssaa_case(s):
    H, W = 17, 33
    cam = view_camera(H, W)
    r = np.random.default_rng(s)
    segs = np.array([[[-1.0, -0.6, 1.0], [1.2, 0.7, 3.0]], [[-0.5, 0.5, 2.0], [0.5, 0.5, 2.0]]], dtype=np.float32)
    ops = [("points", dict(pts=random_points(150, 40 + s, 0.8), colors=r.integers(0, 256, (150, 3), dtype=np.uint8), **cam)),
           ("points", dict(pts=random_points(40, 50 + s, 0.8), colors=r.random((40, 3), dtype=np.float32), psize=3, **cam)),
           ("lines", dict(segs=segs, colors=np.array([[255, 0, 0], [0, 99, 255]], dtype=np.uint8), width=2, **cam))]
    return _case(H, W, ops, ssaa=s, background=BG)


def _lines_case():
    H, W = 17, 33
    z = 2.0
    px = [((2, 3), (20, 3)), ((5, 1), (5, 15)), ((1, 1), (12, 12)), ((30, 2), (27, 16)), ((9, 9), (9, 9)), ((9.4, 10.4), (9.3, 10.2)),      # h, v, 45, steep, one pixel twice
          ((0, 0), (W - 1, 0)), ((W - 1, 0), (W - 1, H - 1)), ((-0.5, 5), (W - 0.5, 5)), ((4, -0.5), (4, H - 0.5)),                          # ends on the border
          ((-40, 8), (80, 9)), ((-5, 3), (4, -6)), ((W - 3, H + 4), (W + 5, H - 4)), ((-3, -3), (40, 25)),                                    # through, across corners
          ((-50, -50), (-20, 100)), ((50, -50), (60, 100)), ((0, 40), (32, 41))]                                                               # wholly outside
    segs = [[[a[0] * z, a[1] * z, z], [b[0] * z, b[1] * z, z]] for a, b in px]
    segs += [[[3.0, 4.0, -1.0], [20.0, 20.0, 1.0]],            # crosses near
             [[3.0, 4.0, -1.0], [5.0, 6.0, -0.5]],             # wholly behind the camera
             [[2.0, 2.0, 0.5], [60.0, 20.0, 30.0]],            # crosses far (far = 10)
             [[10.0, 2.0, 20.0], [12.0, 2.0, 30.0]],           # wholly beyond far
             [[-30.0, 10.0, -2.0], [300.0, 10.0, 20.0]],       # crosses near and far
             [[np.nan, 0.0, 1.0], [1.0, 1.0, 1.0]], [[0.0, 0.0, 1.0], [np.inf, 1.0, 1.0]],
             [[8.0, 24.0, 1.0], [16.0, 12.0, 1.0]], [[8.0, 24.0, 1.0], [16.0, 12.0, 1.0]]]      # the same segment twice, two colours: the smaller wins
    r = np.random.default_rng(3)
    col = r.integers(0, 256, (len(segs), 3), dtype=np.uint8)
    ops = [("lines", dict(segs=np.array(segs, dtype=np.float32), colors=col, near=0.25, far=10.0, **UNIT)),
           ("lines", dict(segs=np.array(segs[:6], dtype=np.float32) + np.float32(1.0), colors=col[:6], width=3, near=0.25, far=10.0, **UNIT))]
    return _case(H, W, ops)


def _wall_case():
    H, W = 17, 33
    wall = np.array([[x * 2.0, y * 2.0, 2.0] for y in range(H) for x in range(17)], dtype=np.float32)
    segs = np.array([[[0.0, 45.0, 3.0], [96.0, 45.0, 3.0]],          # behind the wall on the left half, visible on the right
                     [[0.0, 10.0, 1.0], [32.0, 10.0, 1.0]],          # in front of it
                     [[0.0, 0.0, 1.0], [64.0, 32.0, 4.0]]], dtype=np.float32)     # passes through it
    col = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=np.uint8)
    grey = np.full((len(wall), 3), 128, dtype=np.uint8)
    return _case(H, W, [("lines", dict(segs=segs[:1], colors=col[:1], **UNIT)), ("points", dict(pts=wall, colors=grey, **UNIT)),
                        ("lines", dict(segs=segs[1:], colors=col[1:], **UNIT))])


def three_cameras():
    """three camera-to-world poses, their intrinsics and a view graph with a loop edge"""
    poses = np.tile(np.eye(4), (3, 1, 1))
    for i in range(3):
        poses[i, :3, :3] = rotation((0.1, 1.0, 0.0), 25.0 * i)
        poses[i, :3, 3] = [0.6 * i - 0.6, 0.05 * i, 0.3 * i]
    K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1.0]])
    return poses, K, {0: [1, 2], 1: [0, 2], 2: [0, 1]}, 2


def overview_camera(H, W):
    """looks at the three cameras from above and behind"""
    R = rotation((1.0, 0.0, 0.0), -35.0)
    T = np.concatenate([R, np.array([[0.0], [0.3], [2.5]])], axis=1)
    return dict(T=T, K=(0.7 * W, 0.7 * W, (W - 1) / 2, (H - 1) / 2))


def _scene_case():
    H, W = 48, 64
    poses, K, graph, lmd = three_cameras()
    cam = overview_camera(H, W)
    fr = camera_segments(poses, K, (64, 48), 0.3)
    tr = trajectory_segments(poses)
    vg, vg_col = view_graph_segments(graph, poses, lmd)
    ops = [("lines", dict(segs=fr, colors=np.tile(np.uint8([153, 204, 255]), (len(fr), 1)), **cam)),
           ("lines", dict(segs=tr, colors=np.tile(np.uint8([255, 0, 0]), (len(tr), 1)), width=2, **cam)),
           ("lines", dict(segs=vg, colors=vg_col, **cam))]
    return _case(H, W, ops)


CASES = {
    **{f"points_{M}": functools.partial(_count_case, M) for M in (1, 63, 64, 65, 257, 100000)},
    "one_pixel_canvas": lambda: _case(1, 1, [("points", dict(pts=np.array([[0, 0, 1], [0.4, -0.4, 0.5], [1, 0, 0.25]], dtype=np.float32), **UNIT)),
                                             ("lines", dict(segs=np.array([[[-5, -5, 1], [5, 5, 1]]], dtype=np.float32), colors=np.uint8([[1, 2, 3]]), **UNIT))]),
    "pixel_boundaries": _grid_case,
    "depth_limits": _depth_limit_case,
    "dropped": _dropped_case,
    "ties": _tie_case,
    "contention": _contention_case,
    **{f"point_size_{p}": functools.partial(_size_case, p) for p in (1, 2, 3, 8)},
    "colours_f32": _colour_case,
    "ssaa_2": functools.partial(_ssaa_case, 2),
    "ssaa_4": functools.partial(_ssaa_case, 4),
    "lines": _lines_case,
    "wall": _wall_case,
    "frusta_trajectory_graph": _scene_case,
}


@functools.lru_cache(maxsize=None)
def expected_of(name):
    case = CASES[name]()
    exp = run_case(case)
    for v in exp.values():
        v.setflags(write=False)
    return case, exp


# (text the library refuses with, arguments of plan) - every refusal of sta_raster_plan
PLAN_REFUSED = {
    "H_zero": ((0, 5, 1), r"H and W must be >= 1 \(got 0 x 5\)"),
    "W_negative": ((5, -1, 1), r"H and W must be >= 1 \(got 5 x -1\)"),
    "ssaa_3": ((5, 5, 3), r"ssaa must be 1, 2 or 4 \(got 3\)"),
    "ssaa_0": ((5, 5, 0), r"ssaa must be 1, 2 or 4 \(got 0\)"),
    "H_too_large": ((8193, 5, 1), r"8193 x 5 at ssaa 1 is a key buffer of 8193 x 5, at most 8192 per axis"),
    "W_too_large_ssaa": ((5, 2049, 4), r"5 x 2049 at ssaa 4 is a key buffer of 20 x 8196, at most 8192 per axis"),
}
# refusals of the drawing calls on two points / one segment: (op kind, overrides, text)
DRAW_REFUSED = {
    "point_size_0": ("points", dict(psize=0), r"point_size must be in \[1, 8\] \(got 0\)"),
    "point_size_9": ("points", dict(psize=9), r"point_size must be in \[1, 8\] \(got 9\)"),
    "near_zero": ("points", dict(near=0.0), r"near / far must satisfy"),
    "far_below_near": ("points", dict(near=2.0, far=1.0), r"near / far must satisfy"),
    "far_huge": ("points", dict(far=1e31), r"near / far must satisfy"),
    "T_nan": ("points", dict(T=np.full((3, 4), np.nan)), r"T_host\[0\] is not finite"),
    "K_inf": ("points", dict(K=(1.0, np.inf, 0.0, 0.0)), r"K_host\[1\] is not finite"),
    "id_overflow": ("points", dict(id_base=2 ** 32 - 2), r"would reach 2\^32 - 1"),
    "line_width_9": ("lines", dict(width=9), r"line_width must be in \[1, 8\] \(got 9\)"),
}


# ------------------------------------------------------------------------------------------ a saved run: a procedural room
def room_run(N=4, H=48, W=64, seed=0):
    """A four-view run in the arguments of formats.save_data_all: cameras on an arc inside a box room looking at its far wall, exact depths
    by ray casting against the box, colours from the position.  -> dict(poses, scales, depths, confs, intrinsics, imgs, view_graph,
    loop_min_dist, snapshots = {view index: (poses, scales)})"""
    r = np.random.default_rng(seed)
    K = np.array([[0.9 * W, 0, (W - 1) / 2], [0, 0.9 * W, (H - 1) / 2], [0, 0, 1.0]])
    lo, hi = np.array([-2.0, -1.0, -1.0]), np.array([2.0, 1.0, 3.0])
    poses = np.tile(np.eye(4), (N, 1, 1))
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs, dtype=np.float64)], axis=-1)
    depths, imgs = [], []
    for i in range(N):
        poses[i, :3, :3] = rotation((0.0, 1.0, 0.0), -15.0 + 10.0 * i)
        poses[i, :3, 3] = [-0.6 + 0.4 * i, 0.1, 0.1 * i]
        d = rays @ poses[i, :3, :3].T
        o = poses[i, :3, 3]
        with np.errstate(all="ignore"):
            t = np.where(d > 0, (hi - o) / d, (lo - o) / d).min(axis=-1)            # exit distance of the ray from the box, in units of the ray (z = 1)
        depths.append(t)
        hit = o + d * t[..., None]
        imgs.append(np.clip(np.stack([(hit[..., 0] - lo[0]) / 4, (hit[..., 1] - lo[1]) / 2, (hit[..., 2] - lo[2]) / 4]), 0, 1) * 2 - 1)
    depths = np.asarray(depths, dtype=np.float32)
    confs = r.uniform(0.0, 2.0, depths.shape).astype(np.float32)
    poses = poses.astype(np.float32)
    scales = np.ones((N, 1), dtype=np.float32)
    early = poses.copy()
    early[:, :3, 3] += np.float32(0.05)
    return dict(poses=poses, scales=scales, depths=depths, confs=confs, intrinsics=np.tile(K.astype(np.float32), (N, 1, 1)),
                imgs=np.asarray(imgs, dtype=np.float32), view_graph={0: [1], 1: [0, 2], 2: [1, 3, 0], 3: [2, 0]}, loop_min_dist=2,
                snapshots={1: (early, (scales * np.float32(1.25)))})
