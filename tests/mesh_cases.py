"""The yardstick of libsta_mesh.so: a numpy restatement of include/sta_mesh.h (every floating-point operation is one numpy float64
operation in the header's order, so nothing is contracted; coverage is exact integer arithmetic), a naive scalar per-pixel statement of
the same rule for tests/test_mesh_cpu.py, the vertex normals, and the case builders of tests/test_mesh_gpu.py.  Host-only importable.

It is NOT a GL rasteriser (none is available): no far-plane or 2-D polygon clipping, flat lighting per face, pixel centres at the
integers, ties to the smaller payload - DESIGN.md section 9.

A case is {"H", "W", "ssaa", "background", "ops"}; an op is ("points" | "lines" | "triangles", {...}): the first two are render_cases',
the third has the arguments of `triangles` below.  `expected_of(name)` -> (case, {"keys", "rgba", "depth", "ids", "counters"}), computed
once per process and never changed; "counters" are the eight of the triangle ops."""
import functools

import numpy as np

import render_cases as RC
import tsdf_cases as TC

SUBPIXEL = 256
MAX_SNAP = 1 << 28
ID, COLOR, NORMAL = 0, 1, 2
CULL_NONE, CULL_BACK, CULL_FRONT = 0, 1, 2
N_COUNTERS = 8
PLAN_SIZES = 2
SEEN, BAD, BEHIND, CLIPPED, TOO_LARGE, DEGENERATE, CULLED, OFF_CANVAS = range(8)
VOX_TILE = 1024

# The restatement's own vertex normals on tsdf_cases.sphere_volume()'s mesh against the analytic normal (p - centre) / |p - centre|: the
# largest angle is 0.1940 rad (measured with `sphere_normal_error()` below; the error is the mesh's - marching tetrahedra on a lattice of
# spacing 1 and a radius of 4.4 - not the arithmetic's, which is float64).  The bound of the test is that value with a margin of 2.
SPHERE_NORMAL_ERROR = 0.1940
SPHERE_NORMAL_MARGIN = 2.0
SPHERE_NORMAL_BOUND = SPHERE_NORMAL_ERROR * SPHERE_NORMAL_MARGIN


def _r256(n):
    return (n + 255) // 256 * 256


def plan(nt, nv):
    """sta_mesh_plan: (bytes of the triangles' work, bytes of the normals' work or -1); its refusals as ValueError."""
    if not 0 <= nt < 2 ** 31:
        raise ValueError(f"mesh_plan: nt must be in [0, 2^31) (got {nt})")
    if not 0 <= nv < 2 ** 31:
        raise ValueError(f"mesh_plan: nv must be in [0, 2^31) (got {nv})")
    m = 3 * nt
    nbs = (m + VOX_TILE - 1) // VOX_TILE
    return 256 + _r256(8 * nt), (2 * _r256(8 * m) + 2 * _r256(4 * m) + _r256(1024 * nbs) + 1024) if m < 2 ** 31 else -1


# ------------------------------------------------------------------------------------------ the contract: per triangle
f64 = np.float64


def face_normal(A, B, Cc):
    """(B - A) x (C - A) on the double of float32 world vertices -> (nx, ny, nz, |n|)"""
    ax, ay, az = [f64(v) for v in A]
    ux, uy, uz = f64(B[0]) - ax, f64(B[1]) - ay, f64(B[2]) - az
    vx, vy, vz = f64(Cc[0]) - ax, f64(Cc[1]) - ay, f64(Cc[2]) - az
    with np.errstate(all="ignore"):
        nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        return nx, ny, nz, np.sqrt((nx * nx + ny * ny) + nz * nz)


def channel(c):
    """the channel rule of sta_raster_points on float64 (scalar or array) -> int"""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = np.rint(np.minimum(np.maximum(c, 0.0), 1.0) * 255.0)
    return np.where(np.isnan(c), 0.0, q).astype(np.uint64)


def pack(r, g, b):
    return (channel(r) << np.uint64(24)) | (channel(g) << np.uint64(16)) | (channel(b) << np.uint64(8)) | np.uint64(255)


def light_factor(A, B, Cc, light):
    nx, ny, nz, nn = face_normal(A, B, Cc)
    amb = f64(light[3])
    with np.errstate(all="ignore"):
        dx, dy, dz = f64(light[0]) - f64(A[0]), f64(light[1]) - f64(A[1]), f64(light[2]) - f64(A[2])
        dd = np.sqrt((dx * dx + dy * dy) + dz * dz)
        dot = (nx * dx + ny * dy) + nz * dz
        if nn > 0.0 and dd > 0.0:
            return amb + (f64(1.0) - amb) * (np.abs(dot) / (nn * dd))
    return amb


def normal_payload(A, B, Cc):
    nx, ny, nz, nn = face_normal(A, B, Cc)
    if not nn > 0.0:
        return pack(0.5, 0.5, 0.5)
    with np.errstate(all="ignore"):
        return pack((nx / nn) * f64(0.5) + f64(0.5), (ny / nn) * f64(0.5) + f64(0.5), (nz / nn) * f64(0.5) + f64(0.5))


def cut(vin, vout, near):
    """P(in, out) of the header on vertices (x, y, z, c0, c1, c2): every component with the same t, z exactly near"""
    with np.errstate(all="ignore"):
        t = (near - vin[2]) / (vout[2] - vin[2])
        r = [a + t * (b - a) for a, b in zip(vin, vout)]
    r[2] = near
    return tuple(r)


def clip_triangle(V, near):
    """three camera-space vertices (tuples of float64: x, y, z, then attributes) with at least one z >= near -> (pieces, clipped)"""
    inn = [v[2] >= near for v in V]
    n = sum(inn)
    if n == 3:
        return [tuple(V)], False
    if n == 1:
        i = inn.index(True)
        vi, vj, vk = V[i], V[(i + 1) % 3], V[(i + 2) % 3]
        return [(vi, cut(vi, vj, near), cut(vi, vk, near))], True
    i = inn.index(False)
    vi, vj, vk = V[i], V[(i + 1) % 3], V[(i + 2) % 3]
    pk, pj = cut(vk, vi, near), cut(vj, vi, near)
    return [(vj, vk, pk), (vj, pk, pj)], True


def snap_piece(piece, K, ssaa, sub=SUBPIXEL):
    """-> None (too large) or ([X0, X1, X2], [Y0, Y1, Y2]) as Python ints"""
    X, Y = [], []
    for v in piece:
        us, vs = RC.project(K, v[0], v[1], v[2], ssaa)
        with np.errstate(all="ignore"):
            xd, yd = np.floor(us * f64(sub) + f64(0.5)), np.floor(vs * f64(sub) + f64(0.5))
        if not (abs(xd) <= MAX_SNAP and abs(yd) <= MAX_SNAP):
            return None
        X.append(int(xd)); Y.append(int(yd))
    return X, Y


def setup_piece(piece, K, ssaa, cull, Hs, Ws, sub=SUBPIXEL):
    """-> (reason, None) with reason in TOO_LARGE, DEGENERATE, CULLED, OFF_CANVAS, or (None, (X, Y, A2, order, front, box)): the snapped
    vertices after the winding is normalised, order = the piece's vertex of each slot, box = (x0, x1, y0, y1) clamped to the canvas"""
    sn = snap_piece(piece, K, ssaa, sub)
    if sn is None:
        return TOO_LARGE, None
    X, Y = sn
    A2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if A2 == 0:
        return DEGENERATE, None
    front = A2 < 0
    if (cull == CULL_BACK and not front) or (cull == CULL_FRONT and front):
        return CULLED, None
    order = [0, 1, 2]
    if A2 < 0:
        A2, order = -A2, [0, 2, 1]
        X, Y = [X[0], X[2], X[1]], [Y[0], Y[2], Y[1]]
    x0, x1 = max(-(-min(X) // sub), 0), min(max(X) // sub, Ws - 1)
    y0, y1 = max(-(-min(Y) // sub), 0), min(max(Y) // sub, Hs - 1)
    if x0 > x1 or y0 > y1:
        return OFF_CANVAS, None
    return None, (X, Y, A2, order, front, (x0, x1, y0, y1))


def top_left(dx, dy):
    return dy < 0 or (dy == 0 and dx > 0)


def edges(X, Y, px, py):
    """the three int64 edge functions at pixel centres (px, py) (arrays or ints) and the coverage"""
    out, inside = [], True
    for p, q in ((1, 2), (2, 0), (0, 1)):
        dx, dy = X[q] - X[p], Y[q] - Y[p]
        e = dx * (py - Y[p]) - dy * (px - X[p])
        out.append(e)
        inside = inside & ((e > 0) | ((e == 0) & top_left(dx, dy)))
    return out, inside


def triangles(keys, ssaa, verts, tris, colors=None, color=None, light=None, kind=ID, cull=CULL_NONE, id_base=0, T=RC.IDENT, K=(1, 1, 0, 0),
              near=1e-3, far=1e4, cover=None, sub=SUBPIXEL, prefilter=True, stats=None):
    """sta_mesh_triangles on keys [Hs,Ws] in place -> counters [8] uint64.  prefilter: the triangles that draw nothing and are not cut are
    counted by `_classify`, the same rules on whole arrays, and skipped (a scene of 30 000 triangles of which 500 reach the canvas);
    tests/test_mesh_cpu.py holds the two ways against each other.  stats: None or a dict that receives "max_cut_snap", the largest
    |snapped coordinate| among the pieces of the triangles that are cut (0 without any).  cover: None or int arrays (front [Hs,Ws], back [Hs,Ws]) that
    count the covering pieces per pixel by facing, before the far test (tests/test_mesh_cpu.py)."""
    Hs, Ws = keys.shape
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    nv, nt = len(verts), len(tris)
    cnt = np.zeros(N_COUNTERS, dtype=np.uint64)
    cnt[SEEN] = nt
    pc = RC.to_camera(T, verts) if nv else np.zeros((0, 3))
    near, far = f64(near), f64(far)
    vcol = kind == COLOR and colors is not None
    if vcol:
        colors = np.asarray(colors, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    if kind == ID:
        assert id_base >= 0 and id_base + nt <= 2 ** 32 - 1
    early = _classify(pc, tris, K, ssaa, cull, Hs, Ws, near, sub) if prefilter and nt else np.full(nt, -1)
    cnt += np.bincount(early[early >= 0], minlength=N_COUNTERS).astype(np.uint64)
    for t in np.nonzero(early < 0)[0]:
        idx = [int(i) for i in tris[t]]
        if any(i < 0 or i >= nv for i in idx) or not np.isfinite(pc[idx]).all():
            cnt[BAD] += 1
            continue
        V = [tuple(pc[i]) + (tuple(colors[i]) if vcol else ()) for i in idx]
        if not any(v[2] >= near for v in V):
            cnt[BEHIND] += 1
            continue
        A, B, Cc = verts[idx[0]], verts[idx[1]], verts[idx[2]]
        L = light_factor(A, B, Cc, light) if light is not None else f64(1.0)
        if kind == ID:
            payload = np.uint64((id_base + t) & 0xFFFFFFFF)
        elif kind == NORMAL:
            payload = normal_payload(A, B, Cc)
        elif not vcol:
            payload = pack(f64(color[0]) * L, f64(color[1]) * L, f64(color[2]) * L)
        pieces, clipped = clip_triangle(V, near)
        cnt[CLIPPED] += int(clipped)
        if stats is not None and clipped:
            for piece in pieces:
                sn = snap_piece(piece, K, ssaa, sub)
                if sn is not None:
                    stats["max_cut_snap"] = max(stats.get("max_cut_snap", 0), max(abs(c) for c in sn[0] + sn[1]))
        for piece in pieces:
            why, S = setup_piece(piece, K, ssaa, cull, Hs, Ws, sub)
            if why is not None:
                cnt[why] += 1
                continue
            X, Y, A2, order, front, (x0, x1, y0, y1) = S
            ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
            (e0, e1, e2), inside = edges([np.int64(v) for v in X], [np.int64(v) for v in Y], xs.astype(np.int64) * sub, ys.astype(np.int64) * sub)
            if cover is not None:
                cover[0 if front else 1][y0:y1 + 1, x0:x1 + 1] += inside
            if not inside.any():
                continue
            pv = [piece[o] for o in order]
            with np.errstate(all="ignore"):
                w3 = [f64(1.0) / v[2] for v in pv]
                g0, g1, g2, fa = e0[inside].astype(np.float64), e1[inside].astype(np.float64), e2[inside].astype(np.float64), f64(A2)
                w = ((g0 * w3[0] + g1 * w3[1]) + g2 * w3[2]) / fa
                depth = f64(1.0) / w
                ok = depth <= far
                if vcol:
                    ch = []
                    for c in range(3):
                        q = [pv[k][3 + c] * w3[k] for k in range(3)]
                        cw = ((g0 * q[0] + g1 * q[1]) + g2 * q[2]) / fa
                        cc = cw / w
                        ch.append(cc * L if light is not None else cc)
                    pay = pack(*ch)
                else:
                    pay = np.full(len(w), payload, dtype=np.uint64)
            key = (RC.depth_bits(depth) << np.uint64(32)) | pay
            flat = keys.reshape(-1)
            at = (ys[inside] * Ws + xs[inside])[ok]
            np.minimum.at(flat, at, key[ok])
    return cnt


def _classify(pc, tris, K, ssaa, cull, Hs, Ws, near, sub):
    """-> [nt] the counter a triangle that draws nothing ends in (BAD, BEHIND, or for a triangle that is not cut TOO_LARGE, DEGENERATE,
    CULLED, OFF_CANVAS), -1 for the others.  Elementwise the operations of `snap_piece` and `setup_piece`."""
    nv = len(pc)
    out = np.full(len(tris), -1)
    okidx = ((tris >= 0) & (tris < nv)).all(axis=1)
    ti = np.where(okidx[:, None], tris, 0)
    if nv == 0:
        out[:] = BAD
        return out
    fin = np.isfinite(pc).all(axis=1)[ti].all(axis=1) & okidx
    out[~fin] = BAD
    z = pc[:, 2][ti]
    inn = z >= near
    out[fin & ~inn.any(axis=1)] = BEHIND
    whole = fin & inn.all(axis=1)
    us, vs = RC.project(K, pc[:, 0], pc[:, 1], pc[:, 2], ssaa)
    with np.errstate(all="ignore"):
        xd, yd = np.floor(us * f64(sub) + f64(0.5)), np.floor(vs * f64(sub) + f64(0.5))
        small = (np.abs(xd) <= MAX_SNAP) & (np.abs(yd) <= MAX_SNAP)
    X, Y = np.where(small, xd, 0).astype(np.int64)[ti], np.where(small, yd, 0).astype(np.int64)[ti]
    big = ~small[ti].all(axis=1)
    A2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    culled = ((cull == CULL_BACK) & (A2 > 0)) | ((cull == CULL_FRONT) & (A2 < 0))
    x0, x1 = np.maximum(-(-X.min(axis=1) // sub), 0), np.minimum(X.max(axis=1) // sub, Ws - 1)
    y0, y1 = np.maximum(-(-Y.min(axis=1) // sub), 0), np.minimum(Y.max(axis=1) // sub, Hs - 1)
    off = (x0 > x1) | (y0 > y1)
    reason = np.where(big, TOO_LARGE, np.where(A2 == 0, DEGENERATE, np.where(culled, CULLED, np.where(off, OFF_CANVAS, -1))))
    out[whole] = reason[whole]
    return out


def naive_triangles(Hs, Ws, ssaa, verts, tris, T, K, near, far, cull=CULL_NONE, id_base=0):
    """The same rule said the slow way, for small cases: every pixel of the canvas against every piece with Python integers and one float64
    at a time; ids only.  It shares `clip_triangle` (and the camera) with the restatement and nothing else.  -> keys [Hs,Ws] uint64"""
    keys = RC.new_keys(Hs, Ws, 1)
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    pc = RC.to_camera(T, verts)
    fx, fy, cx, cy = [float(v) for v in K]
    s, off = float(ssaa), (ssaa - 1) * 0.5
    for t, idx in enumerate(np.asarray(tris).reshape(-1, 3).tolist()):
        if any(i < 0 or i >= len(verts) for i in idx) or not np.isfinite(pc[idx]).all():
            continue
        V = [tuple(pc[i]) for i in idx]
        if not any(v[2] >= near for v in V):
            continue
        for piece in clip_triangle(V, f64(near))[0]:
            P = []
            for v in piece:
                x, y, z = float(v[0]), float(v[1]), float(v[2])
                us, vs = (fx * (x / z) + cx) * s + off, (fy * (y / z) + cy) * s + off
                xd, yd = np.floor(us * 256.0 + 0.5), np.floor(vs * 256.0 + 0.5)
                P.append((xd, yd, 1.0 / z))
            if not all(abs(p[0]) <= MAX_SNAP and abs(p[1]) <= MAX_SNAP for p in P):
                continue
            P = [(int(p[0]), int(p[1]), p[2]) for p in P]
            A2 = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[1][1] - P[0][1]) * (P[2][0] - P[0][0])
            if A2 == 0 or (cull == CULL_BACK and A2 > 0) or (cull == CULL_FRONT and A2 < 0):
                continue
            if A2 < 0:
                P, A2 = [P[0], P[2], P[1]], -A2
            for y in range(Hs):
                for x in range(Ws):
                    e, inside = [], True
                    for p, q in ((1, 2), (2, 0), (0, 1)):
                        dx, dy = P[q][0] - P[p][0], P[q][1] - P[p][1]
                        v = dx * (256 * y - P[p][1]) - dy * (256 * x - P[p][0])
                        inside = inside and (v > 0 or (v == 0 and (dy < 0 or (dy == 0 and dx > 0))))
                        e.append(v)
                    if not inside:
                        continue
                    assert sum(e) == A2 and min(e) >= 0
                    w = ((float(e[0]) * P[0][2] + float(e[1]) * P[1][2]) + float(e[2]) * P[2][2]) / float(A2)
                    depth = 1.0 / w
                    if not depth <= far:
                        continue
                    key = (int(np.float32(depth).view(np.uint32)) << 32) | ((id_base + t) & 0xFFFFFFFF)
                    keys[y, x] = min(int(keys[y, x]), key)
    return keys


def vertex_normals(verts, tris):
    """sta_mesh_vertex_normals -> [nv,3] float32"""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    nv = len(verts)
    S = np.zeros((nv, 3))
    ok = ((tris >= 0) & (tris < nv)).all(axis=1)
    with np.errstate(all="ignore"):
        for t in np.nonzero(ok)[0]:                       # ascending t, corners in order: the sums of a vertex are taken in the header's order
            A, B, Cc = verts[tris[t]]
            nx, ny, nz, _ = face_normal(A, B, Cc)
            for v in tris[t]:
                S[v, 0] = S[v, 0] + nx; S[v, 1] = S[v, 1] + ny; S[v, 2] = S[v, 2] + nz
        ln = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
        good = (ln > 0.0) & np.isfinite(ln)
        out = np.where(good[:, None], S / ln[:, None], 0.0)
    return out.astype(np.float32)


def run_case(case):
    keys = RC.new_keys(case["H"], case["W"], case["ssaa"])
    counters = np.zeros(N_COUNTERS, dtype=np.uint64)
    for kind, a in case["ops"]:
        if kind == "points":
            RC.points(keys, case["ssaa"], **a)
        elif kind == "lines":
            RC.lines(keys, case["ssaa"], **a)
        else:
            counters += triangles(keys, case["ssaa"], **a)
    rgba, depth, ids = RC.resolve(keys, case["ssaa"], case["background"])
    return {"keys": keys, "rgba": rgba, "depth": depth, "ids": ids, "counters": counters}


# ------------------------------------------------------------------------------------------ meshes and cameras
SPHERE_CENTRE = np.array([3.5, 4.25, 2.75])
SPHERE_RADIUS = 4.4


@functools.lru_cache(None)
def sphere_mesh():
    """tsdf_cases.sphere_volume()'s mesh: 1064 vertices, 2124 triangles, closed, normals outwards; vertex colours from the position"""
    v, _c, t = TC.mesh(*TC.sphere_volume())
    col = np.clip((v.astype(np.float64) - SPHERE_CENTRE) / (2 * SPHERE_RADIUS) + 0.5, 0, 1).astype(np.float32)
    for a in (v, t, col):
        a.setflags(write=False)
    return v, t, col


@functools.lru_cache(None)
def random_mesh(seed=3):
    v, c, t = TC.mesh(*TC.random_volume(seed))
    return v, t, c


@functools.lru_cache(None)
def room_mesh():
    """the restatement's fusion of tsdf_cases.room_scene(24, 32)"""
    out = TC.room_expected(24, 32)[1]
    return out[4], out[6], out[5]


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """a 3x4 world-to-camera matrix, x right, y down, z forward (render.Camera.look_at restated)"""
    eye, target, up = [np.asarray(a, dtype=np.float64) for a in (eye, target, up)]
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up); x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ eye)[:, None]], axis=1)


def cam(H, W, f, eye, target, near=1e-3, far=1e4, up=(0.0, -1.0, 0.0)):
    return dict(T=look_at(eye, target, up), K=(float(f), float(f), (W - 1) / 2.0, (H - 1) / 2.0), near=near, far=far)


OUTSIDE_EYE = SPHERE_CENTRE + np.array([0.0, 0.0, -12.0])            # along an axis: every pixel has at most one front and one back face
OBLIQUE_EYE = SPHERE_CENTRE + np.array([3.0, -5.0, -11.0])           # the mesh is not convex: near the silhouette a pixel may have two of each
INSIDE_EYE = SPHERE_CENTRE + np.array([1.0, 2.0, -2.0])              # 3 voxels off the centre, 1.4 from the surface
OUTSIDE = {"48x64": (48, 64, 40.0, 256), "24x32": (24, 32, 20.0, 16), "96x128": (96, 128, 90.0, 256)}        # H, W, f, sub-pixel grid
INSIDE_NEARS = (0.5, 0.05, 1e-3)
# What the restatement gives for `inside_cam(near)` on the sphere mesh, pinned so that a change of the clip or snap rule cannot pass
# silently: near -> (the eight counters, the largest |snapped coordinate| among the pieces of the cut triangles).  Filled in from
# `inside_numbers()`; tests/test_mesh_cpu.py asserts them exactly.
INSIDE_EXPECTED = {
    0.5: ([2124, 0, 650, 122, 0, 0, 0, 924], 33690),            # 2^15.04
    0.05: ([2124, 0, 548, 119, 0, 0, 0, 1023], 352143),            # 2^18.43
    0.001: ([2124, 0, 537, 121, 0, 0, 0, 1035], 17675909),            # 2^24.08
}


def outside_cam(H, W, f, eye=None):
    return cam(H, W, f, OUTSIDE_EYE if eye is None else eye, SPHERE_CENTRE)


def inside_cam(near, H=24, W=32, f=12.0):
    return cam(H, W, f, INSIDE_EYE, INSIDE_EYE + np.array([0.2, -0.1, 1.0]), near=near)


def inside_numbers(near):
    v, t, _ = sphere_mesh()
    st = {}
    cnt = triangles(RC.new_keys(24, 32, 1), 1, v, t, stats=st, **inside_cam(near))
    return cnt.tolist(), st.get("max_cut_snap", 0)


def sphere_normal_error():
    v, t, _ = sphere_mesh()
    n = vertex_normals(v, t).astype(np.float64)
    a = v.astype(np.float64) - SPHERE_CENTRE
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    return float(np.arccos(np.clip((n * a).sum(1), -1, 1)).max())


# ------------------------------------------------------------------------------------------ cases
LIGHT = (1.5, -2.0, -6.0, 0.3)
GREY = (200 / 255.0, 200 / 255.0, 200 / 255.0)
PAYLOADS = {
    "id": dict(kind=ID, id_base=5),
    "color": dict(kind=COLOR, colors="vertex"),
    "lit": dict(kind=COLOR, colors="vertex", light=LIGHT),
    "uniform": dict(kind=COLOR, color=GREY, light=LIGHT),
    "normal": dict(kind=NORMAL),
}


def _case(H, W, ops, ssaa=1, background=RC.BG):
    return {"H": H, "W": W, "ssaa": ssaa, "background": background, "ops": ops}


def _tri_op(verts, tris, cols=None, **kw):
    a = dict(verts=np.asarray(verts, dtype=np.float32), tris=np.asarray(tris, dtype=np.int32))
    if kw.get("colors") == "vertex":
        kw["colors"] = cols
    a.update(kw)
    return ("triangles", a)


def _sphere_case(where, payload, cull, ssaa=1):
    v, t, col = sphere_mesh()
    H, W = 24, 32
    c = outside_cam(H, W, 20.0, OBLIQUE_EYE) if where == "outside" else inside_cam(0.05)
    return _case(H, W, [_tri_op(v, t, col, cull=cull, **PAYLOADS[payload], **c)], ssaa)


def _random_case():
    v, t, col = random_mesh()
    lo, hi = v.min(0), v.max(0)
    c = cam(30, 40, 30.0, (lo + hi) / 2 + np.array([4.0, -9.0, -22.0]), (lo + hi) / 2)
    return _case(30, 40, [_tri_op(v, t, col, **PAYLOADS["lit"], **c)])


UNIT = dict(T=RC.IDENT, K=(1.0, 1.0, 0.0, 0.0))        # z = 1 puts a vertex at the pixel coordinate (x, y) exactly


def _px(points, z=1.0):
    return [[x * z, y * z, z] for x, y in points]


def _shared_edge_case():
    """two triangles whose common edge (2,2)-(8,8) runs through pixel centres, a vertex exactly on the centre (2,2), an edge along row 2
    and one along column 8: every centre on a shared edge belongs to exactly one triangle"""
    v = _px([(2, 2), (8, 8), (8, 2), (2, 8), (5, 11), (11, 5)])
    t = [[0, 2, 1], [0, 1, 3], [3, 1, 4], [2, 5, 1]]
    return _case(12, 13, [_tri_op(v, t, kind=ID, **UNIT)])


def _sliver_case():
    v = _px([(1, 1), (9, 1.001), (5, 1.0005), (1, 3), (9, 3), (5, 3.0000001), (2, 5), (2, 5), (6, 7)])
    return _case(9, 11, [_tri_op(v, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], kind=ID, **UNIT)])


def _near_case():
    """behind the camera; one vertex in front; two in front; a pair sharing a crossing edge (the two cut points have the same bits, so the
    pair leaves no gap and no pixel twice); vertex colours carried through the cut"""
    v = [[1, 1, -1], [9, 2, -2], [4, 8, -0.5],                  # behind
         [5, 5, 3], [-20, 4, -1], [30, 9, -1],                  # one in front
         [2, 2, 2], [12, 3, 2.5], [6, 40, -1],                  # two in front
         [3, 10, 2], [14, 12, 3], [8, 9, -2], [10, 30, -1]]     # the pair: (9, 10) in front, 11 and 12 behind; the edges 9-11... are shared
    t = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [10, 9, 12]]
    r = np.random.default_rng(1)
    col = r.random((len(v), 3), dtype=np.float32)
    k = dict(T=RC.IDENT, K=(4.0, 4.0, 6.0, 5.0), near=0.75, far=100.0)
    return _case(16, 20, [_tri_op(v, t, col, kind=COLOR, colors="vertex", **k), _tri_op(np.asarray(v) + [0, 0, 0.25], t, kind=ID, id_base=100, **k)])


def _full_canvas_case():
    v = [[-40, -30, 1], [200, -30, 1], [-40, 200, 1], [0.2, 0.1, 0.5], [0.9, 0.2, 0.5], [0.3, 0.8, 0.5]]
    col = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=np.float32)
    return _case(48, 64, [_tri_op(v, [[0, 1, 2], [3, 4, 5]], col, kind=COLOR, colors="vertex", **UNIT)], ssaa=4)


def _off_canvas_case():
    v = _px([(-30, -20), (4, 3), (-25, 9), (100, 100), (120, 100), (100, 130), (5.25, 5.25), (5.75, 5.3), (5.4, 5.8)])
    return _case(10, 12, [_tri_op(v, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], kind=ID, **UNIT)])


def _too_large_case():
    v = [[0, 0, 1], [5, 0, 1], [2e6, 9, 1], [1, 1, 2], [8, 2, 2], [3, 9, 1e-7], [2, 2, 1], [9, 2, 1], [2, 8, 1]]      # 2e6 * 256 > 2^28; the second is cut at near 1e-6: both pieces have a point at x / z of 3e6
    return _case(10, 12, [_tri_op(v, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], kind=ID, near=1e-6, **UNIT)])


def _bad_case():
    n, i = np.nan, np.inf
    v = _px([(1, 1), (9, 1), (1, 9)]) + [[n, 0, 1], [0, i, 1], [0, 0, -i]]
    t = [[0, 1, 2], [0, 1, 6], [-1, 1, 2], [0, 1, 3], [4, 1, 2], [0, 5, 2], [0, 2, 1]]
    return _case(10, 12, [_tri_op(v, t, kind=NORMAL, **UNIT)])


def _coincident_case():
    v = _px([(1, 1), (9, 1), (1, 9)])
    return _case(10, 12, [_tri_op(v, [[0, 1, 2], [0, 1, 2], [1, 2, 0]], kind=ID, id_base=9, **UNIT), _tri_op(v, [[0, 1, 2]], kind=ID, id_base=3, **UNIT)])


def _far_case():
    v = [[0, 0, 1], [40, 0, 4], [0, 40, 4]]
    return _case(12, 14, [_tri_op(v, [[0, 1, 2]], kind=ID, far=2.5, **UNIT)])


def _mixed_ops():
    H, W = 17, 33
    c = RC.view_camera(H, W)
    r = np.random.default_rng(8)
    v = np.array([[-0.9, -0.6, 1.5], [1.0, -0.5, 2.5], [0.1, 0.7, 1.0], [-1.0, 0.6, 3.0], [1.1, 0.6, 0.8]], dtype=np.float32)
    col = r.random((5, 3), dtype=np.float32)
    segs = np.array([[[-1.0, -0.6, 1.0], [1.2, 0.7, 3.0]], [[-0.5, 0.5, 2.0], [0.5, 0.5, 2.0]]], dtype=np.float32)
    return H, W, [("points", dict(pts=RC.random_points(150, 41, 0.8), colors=r.integers(0, 256, (150, 3), dtype=np.uint8), psize=2, **c)),
                  _tri_op(v, [[0, 1, 2], [0, 2, 3], [2, 1, 4]], col, kind=COLOR, colors="vertex", **c),
                  ("lines", dict(segs=segs, colors=np.array([[255, 0, 0], [0, 99, 255]], dtype=np.uint8), width=2, **c))]


def _mixed_case(order, ssaa=2):
    H, W, ops = _mixed_ops()
    return _case(H, W, [ops[i] for i in order], ssaa)


def _ssaa_case(s):
    v, t, col = sphere_mesh()
    return _case(12, 16, [_tri_op(v, t, col, **PAYLOADS["lit"], **outside_cam(12, 16, 10.0, OBLIQUE_EYE))], ssaa=s)


CASES = {
    **{f"sphere_outside_{p}_cull{c}": functools.partial(_sphere_case, "outside", p, c) for p in PAYLOADS for c in (0, 1, 2)},
    **{f"sphere_inside_{p}_cull{c}": functools.partial(_sphere_case, "inside", p, c) for p in PAYLOADS for c in (0, 1, 2)},
    "random_volume": _random_case,
    "shared_edge": _shared_edge_case,
    "sliver": _sliver_case,
    "near_plane": _near_case,
    "full_canvas_ssaa4": _full_canvas_case,
    "off_canvas": _off_canvas_case,
    "too_large": _too_large_case,
    "bad_index_nan": _bad_case,
    "coincident": _coincident_case,
    "far": _far_case,
    **{f"ssaa_{s}": functools.partial(_ssaa_case, s) for s in (1, 2, 4)},
    "mixed_ptl": functools.partial(_mixed_case, (0, 1, 2)),
    "mixed_ltp": functools.partial(_mixed_case, (2, 1, 0)),
    "no_triangles": lambda: _case(5, 7, [_tri_op(_px([(1, 1), (3, 1), (1, 3)]), np.zeros((0, 3), np.int32), kind=ID, **UNIT)]),
}


@functools.lru_cache(maxsize=None)
def expected_of(name):
    case = CASES[name]()
    exp = run_case(case)
    for v in exp.values():
        v.setflags(write=False)
    return case, exp


def fan_mesh(n=40):
    """n triangles around vertex 0, not planar"""
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rim = np.stack([np.cos(a), np.sin(a), 0.2 * np.sin(3 * a)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(np.float32)
    t = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], dtype=np.int32)
    return v, t


def odd_mesh():
    """an isolated vertex (4), a degenerate triangle (two equal corners), a bad index, a zero-area triangle of three distinct corners"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5], [2, 0, 0], [3, 0, 0]], dtype=np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3], [1, 1, 3], [0, 1, 9], [0, 5, 6], [3, 2, 1]], dtype=np.int32)
    return v, t


NORMAL_MESHES = {"sphere": lambda: sphere_mesh()[:2], "odd": odd_mesh, "fan_40": fan_mesh, "random_volume": lambda: random_mesh()[:2],
                 "no_triangles": lambda: (odd_mesh()[0], np.zeros((0, 3), np.int32))}

# (overrides of a valid one-triangle call, text of the refusal)
REFUSED = {
    "nt_negative": (dict(nt=-1), r"nt must be in \[0, 2\^31\) \(got -1\)"),
    "nv_huge": (dict(nv=2 ** 31), r"nv must be in \[0, 2\^31\) \(got 2147483648\)"),
    "ssaa_3": (dict(ssaa=3), r"ssaa must be 1, 2 or 4 \(got 3\)"),
    "H_zero": (dict(H=0), r"H and W must be >= 1 \(got 0 x 7\)"),
    "near_zero": (dict(near=0.0), r"near / far must satisfy"),
    "far_huge": (dict(far=1e31), r"near / far must satisfy"),
    "T_nan": (dict(T=np.full((3, 4), np.nan)), r"T_host\[0\] is not finite"),
    "K_inf": (dict(K=(1.0, np.inf, 0.0, 0.0)), r"K_host\[1\] is not finite"),
    "light_nan": (dict(kind=COLOR, color=GREY, light=(0.0, np.nan, 0.0, 0.3)), r"light_host\[1\] is not finite"),
    "ambient_2": (dict(kind=COLOR, color=GREY, light=(0.0, 0.0, 0.0, 2.0)), r"ambient must be in \[0, 1\] \(got 2\)"),
    "id_with_color": (dict(kind=ID, color=GREY), r"payload_kind 0 takes no colors"),
    "color_without": (dict(kind=COLOR), r"payload_kind 1 takes exactly one of colors"),
    "kind_3": (dict(kind=3), r"payload_kind must be 0, 1 or 2 \(got 3\)"),
    "cull_3": (dict(cull=3), r"cull must be 0, 1 or 2 \(got 3\)"),
    "id_overflow": (dict(id_base=2 ** 32 - 1), r"would reach 2\^32 - 1"),
    "work_small": (dict(work_bytes=8), r"work of 8 bytes, 512 needed for 1 triangles"),
}
