"""include/sta_ray.h restated in numpy: a usable ray, the slab interval of a widened box, the sheared triangle test, qualification with the
own-box test and the clamp, and a brute force over all valid triangles with the tie rule (every numpy operation below is one IEEE operation
per element, in the header's order).  The index is dist_cases.Index, the restatement of the build.  The GPU tests compare with array_equal;
tests/test_ray_cpu.py holds this file against a second, independent statement (Moeller-Trumbore in numpy.longdouble) and asserts the
containment chain of the header's rule 6 exactly.

It is not Open3D's RaycastingScene: that is not available."""
import functools

import numpy as np

import dist_cases as D

f32, f64 = np.float32, np.float64
FANOUT = 8
MAX_LEVELS = 9
N_VALID = 0
PLAN_SIZES = 1
STATUS_BOUND = 1

# The largest |t of the restatement - t of Moeller-Trumbore in numpy.longdouble| relative to max(|t|, 1e-300), measured by
# tests/test_ray_cpu.py on its cases (hits that lie inside the triangle by the barycentric margin SECOND_STATEMENT_MARGIN: every weight
# >= the margin; icospheres over seven decades of scale, two of them far from the origin, two ray origins each, 17 852 hits): 4.6e-16.
# The test asserts SECOND_STATEMENT_FACTOR times this (the factor of tests/dist_cases.py; the margin covers other longdouble widths).
SECOND_STATEMENT_MEASURED = 4.6e-16
SECOND_STATEMENT_FACTOR = 4.0
SECOND_STATEMENT_MARGIN = 1e-3


def plan(nt, R=1):
    """(nodes,) of sta_ray_plan, its refusals as ValueError with the library's words"""
    nt, R = int(nt), int(R)
    if not 1 <= nt < 1 << 27:
        raise ValueError(f"ray_plan: nt must be in [1, 2^27) (got {nt})")
    if not 1 <= R < 1 << 30:
        raise ValueError(f"ray_plan: R must be in [1, 2^30) (got {R})")
    return (sum(D.level_counts(nt)),)


# ------------------------------------------------------------------------------------------ rules 1 to 4
def usable(org, dirs):
    org, dirs = np.asarray(org, dtype=f32), np.asarray(dirs, dtype=f32)
    return np.isfinite(org).all(axis=-1) & np.isfinite(dirs).all(axis=-1) & (dirs != 0).any(axis=-1)


def widen(lo, hi):
    return np.nextafter(np.asarray(lo, dtype=f32), f32(-np.inf)), np.nextafter(np.asarray(hi, dtype=f32), f32(np.inf))


def slab(org, dirs, lo, hi, t_min=0.0, t_max=np.inf):
    """rule 2: (passes, enter, exit) of the boxes (lo, hi) [...,3] float32 for the rays (org, dirs) [...,3] float32, broadcast together"""
    lo, hi = widen(lo, hi)
    lo, hi, o, d = (np.asarray(x, dtype=f32).astype(f64) for x in (lo, hi, org, dirs))
    shape = np.broadcast(lo, o, d).shape[:-1]
    enter, exit_ = np.full(shape, f64(t_min)), np.full(shape, f64(t_max))
    ok = np.ones(shape, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            dk, ok_ = np.broadcast_to(d[..., k], shape), np.broadcast_to(o[..., k], shape)
            nz = dk != 0
            inv = 1.0 / dk
            near, far = np.where(dk > 0, lo[..., k], hi[..., k]), np.where(dk > 0, hi[..., k], lo[..., k])
            tn, tf = (near - ok_) * inv, (far - ok_) * inv
            enter = np.where(nz & (tn > enter), tn, enter)
            exit_ = np.where(nz & (tf < exit_), tf, exit_)
            ok = ok & (nz | ((lo[..., k] <= ok_) & (ok_ <= hi[..., k])))
        return ok & (enter <= exit_), enter, exit_


def shear_of(dirs):
    """per ray: kz (the first axis of the largest |d_k|) and (Sx, Sy, Sz)"""
    d32 = np.asarray(dirs, dtype=f32)
    kz = np.argmax(np.abs(d32), axis=-1)          # the first maximum
    d = d32.astype(f64)
    pick = lambda k: np.take_along_axis(d, k[..., None], axis=-1)[..., 0]
    with np.errstate(all="ignore"):
        dz = pick(kz)
        return kz, pick((kz + 1) % 3) / dz, pick((kz + 2) % 3) / dz, 1.0 / dz


def sheared(org, P, kz, Sx, Sy, Sz):
    """the 2-D position and the scaled depth of the vertices P [...,3] float32 for rays org [...,3]: ONE computation per (ray, vertex)"""
    q = np.asarray(P, dtype=f32).astype(f64) - np.asarray(org, dtype=f32).astype(f64)
    shape = np.broadcast(q[..., 0], kz).shape
    q, kz = np.broadcast_to(q, shape + (3,)), np.broadcast_to(kz, shape)
    pick = lambda k: np.take_along_axis(q, k[..., None], axis=-1)[..., 0]
    with np.errstate(all="ignore"):
        c = pick(kz)
        return pick((kz + 1) % 3) - Sx * c, pick((kz + 2) % 3) - Sy * c, Sz * c


def triangle(org, dirs, A, B, Cc):
    """rule 3: (passes, t, U / det, V / det, W / det) in float64, before any range test"""
    kz, Sx, Sy, Sz = shear_of(dirs)
    Ax, Ay, Az = sheared(org, A, kz, Sx, Sy, Sz)
    Bx, By, Bz = sheared(org, B, kz, Sx, Sy, Sz)
    Cx, Cy, Cz = sheared(org, Cc, kz, Sx, Sy, Sz)
    with np.errstate(all="ignore"):
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        det = (U + V) + W
        ok = (((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))) & (det != 0)
        t = ((U * Az + V * Bz) + W * Cz) / det
        return ok, t, U / det, V / det, W / det


def qualify(org, dirs, A, B, Cc, t_min=0.0, t_max=np.inf, widened=True):
    """rule 4: (qualifies, t_c, bary [...,3] float32, enter_own, exit_own, the raw t, rule 3 passes).  widened=False: the own box as it is
    (for the measurement of why it must be widened; never the contract)"""
    A, B, Cc = (np.asarray(x, dtype=f32) for x in (A, B, Cc))
    lo, hi = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
    if not widened:
        lo, hi = np.nextafter(lo, f32(np.inf)), np.nextafter(hi, f32(-np.inf))          # slab() widens them back
    own, enter, exit_ = slab(org, dirs, lo, hi, t_min, t_max)
    hit, t, bu, bv, bw = triangle(org, dirs, A, B, Cc)
    with np.errstate(all="ignore"):
        q = own & hit & (f64(t_min) <= t) & (t <= f64(t_max))
        tc = np.where(t >= enter, t, enter)
        tc = np.where(tc <= exit_, tc, exit_)
        bary = np.stack(np.broadcast_arrays(bu, bv, bw), axis=-1).astype(f32)
    return q, tc, bary, enter, exit_, t, hit


def check_range(who, t_min, t_max):
    if not (f64(t_min) >= 0 and f64(t_min) <= f64(t_max)):
        raise ValueError(f"{who}: 0 <= t_min <= t_max is required, t_max = +inf allowed (got {float(t_min):g}, {float(t_max):g})")


# ------------------------------------------------------------------------------------------ rule 5: brute force
def brute(index, org, dirs, t_min=0.0, t_max=np.inf, chunk=128):
    """(t [R] float64, tri [R] int32, bary [R,3] float32, occluded [R] uint8): over ALL valid triangles, smallest t_c, lowest index among
    equals.  org may be [3]."""
    check_range("ray_cast", t_min, t_max)
    dirs = np.asarray(dirs, dtype=f32).reshape(-1, 3)
    org = np.broadcast_to(np.asarray(org, dtype=f32), dirs.shape)
    R = len(dirs)
    to, trio, bo = np.full(R, np.inf), np.full(R, -1, dtype=np.int32), np.full((R, 3), np.nan, dtype=f32)
    ids = np.nonzero(index.cls == D.VALID)[0]          # ascending
    if not len(ids):
        return to, trio, bo, np.zeros(R, dtype=np.uint8)
    P = D.corners(index.verts, index.tris[ids])
    lo, hi = P.min(axis=1), P.max(axis=1)
    use = usable(org, dirs)
    for s in range(0, R, chunk):
        o, d = org[s:s + chunk], dirs[s:s + chunk]
        # rule 4 (a) first, over all pairs; rules 3 and 4 (b), (c) only where the own box passes: the same functions, fewer pairs
        own = slab(o[:, None], d[:, None], lo[None], hi[None], t_min, t_max)[0] & use[s:s + chunk, None]
        r, k = np.nonzero(own)
        qp, tcp, baryp, _e, _x, _t, _h = qualify(o[r], d[r], P[k, 0], P[k, 1], P[k, 2], t_min, t_max)
        q, tc = np.zeros(own.shape, dtype=bool), np.full(own.shape, np.inf)
        q[r, k], tc[r, k] = qp, tcp
        m = np.where(q, tc, np.inf).min(axis=1)
        j = np.argmax(q & (tc == m[:, None]), axis=1)          # the first, i.e. the lowest index, of the smallest t_c
        rows, ok = np.arange(len(m)), q.any(axis=1)
        bary = np.full(own.shape + (3,), np.nan, dtype=f32)
        bary[r, k] = baryp
        to[s:s + chunk][ok] = tc[rows, j][ok]
        trio[s:s + chunk][ok] = ids[j][ok]
        bo[s:s + chunk][ok] = bary[rows, j][ok]
    return to, trio, bo, (trio >= 0).astype(np.uint8)


def ancestors(index):
    """[levels][n_valid] the node of every level above each sorted position, and the boxes of every level"""
    pos = np.arange(index.n_valid)
    return [pos // FANOUT ** (l + 1) for l in range(len(index.counts))]


# ------------------------------------------------------------------------------------------ meshes and rays
def icosphere(level=2, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """a closed sphere of 20 * 4^level triangles with shared vertices, float32 -> (verts, tris)"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(x, dtype=f64) / np.linalg.norm(x) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    return (np.array(v) * scale + np.asarray(offset, dtype=f64)).astype(f32), np.array(t, dtype=np.int32)


def edges(tris):
    t = np.asarray(tris)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0)


def aimed_dirs(verts, tris, origin, n_random=2000, seed=0):
    """float32 directions from `origin` at every vertex, every edge midpoint, every edge 1/4 point (float32 targets), n_random random
    directions and 9 axis / diagonal ones"""
    v = np.asarray(verts, dtype=f32)
    e = edges(tris)
    a, b = v[e[:, 0]].astype(f64), v[e[:, 1]].astype(f64)
    targets = np.concatenate([v, ((a + b) * 0.5).astype(f32), (a * 0.75 + b * 0.25).astype(f32)])
    o = np.asarray(origin, dtype=f32)
    r = np.random.default_rng(seed)
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 0], [0, 1, 1], [1, 1, 1]], dtype=f32)
    return np.concatenate([(targets - o).astype(f32), r.standard_normal((n_random, 3)).astype(f32), axes])


def one_triangle():
    """a dyadic triangle in the plane z = 2"""
    return np.array([[0, 0, 2], [4, 0, 2], [0, 4, 2]], dtype=f32), np.array([[0, 1, 2]], dtype=np.int32)


def one_triangle_rays():
    """(org, dirs, t_min, t_max) groups against one_triangle(): every step is exact where the numbers are dyadic"""
    up = lambda x, y: ((x, y, 0.0), (0.0, 0.0, 1.0))          # from z = 0 straight up: t = 2
    step = lambda x, s: float(np.nextafter(f32(x), f32(s)))
    rays = [up(1, 1), up(0.5, 3), up(2, 0), up(0, 2), up(2, 2), up(0, 0), up(4, 0), up(0, 4),            # interior, edges, vertices
            up(2, step(0, -1)), up(step(0, -1), 2), up(step(2, 3), 2), up(2, step(2, 3)),                  # one float32 step outside each edge
            up(2, step(0, 1)), up(step(0, 1), 2), up(step(2, 1), 2),                                       # ... and one step inside
            ((1, 1, 0), (1, 0, 0)), ((1, 1, 0), (1, 1, 0)),                                                # parallel to the plane: det == 0
            ((-1, 1, 2), (1, 0, 0)), ((1, 1, 2), (0, 1, 0)),                                               # in the plane
            ((1, 1, 3), (0, 0, 1)), ((1, 1, 3), (0, 0, -1)),                                               # behind the origin; in front, from above
            ((1, 1, 0), (0, 0, 2)), ((1, 1, 0), (0, 0, 0.5)), ((1, 1, 1), (0, 0, 8)),                      # t = 1, 4, 1/8: d is not normalised
            ((1, 1, 0), (0.25, 0, 1)), ((1, 1, 0), (0.5, 0.25, 1)), ((3, 3, 0), (-0.5, -0.5, 1)),           # one, no zero component
            ((0, 1, 0), (0, 0, 1)), ((1, 0, 1), (0, 0, 1)), ((4, 0, 1), (0, 0, 1)),                        # the origin on a face of the box (x = 0, y = 0, the corner)
            ((1, 1, 2), (0, 0, 1)),                                                                        # the origin ON the triangle: t = 0
            ((1, 1, 0), (0, 0, 0)), ((np.nan, 1, 0), (0, 0, 1)), ((1, 1, 0), (0, np.inf, 1)), ((1, -np.inf, 0), (0, 0, 1))]      # not usable
    org, dirs = np.array([r[0] for r in rays], dtype=f32), np.array([r[1] for r in rays], dtype=f32)
    return org, dirs


RANGES = [(0.0, np.inf), (0.0, 2.0), (2.0, 4.0), (2.0, 2.0), (0.0, 1.9999999), (2.0000001, np.inf), (0.125, 0.125), (1.0, 1.0)]


def coplanar_pair():
    """two coplanar triangles sharing the edge (0,0,1)-(2,2,1) and, behind them, the pair again with reversed winding: a ray onto the
    shared edge qualifies for four triangles, a ray into one of them for two"""
    v = np.array([[0, 0, 1], [2, 0, 1], [2, 2, 1], [0, 2, 1]], dtype=f32)
    t = np.array([[0, 2, 3], [0, 1, 2], [2, 1, 0], [3, 2, 0]], dtype=np.int32)
    org = np.array([[1, 1, 0], [0.5, 0.5, 0], [1.5, 1.5, 0], [0, 0, 0], [2, 2, 0], [1.5, 0.5, 0], [0.5, 1.5, 0], [1, 1, 3]], dtype=f32)
    dirs = np.array([[0, 0, 1]] * 7 + [[0, 0, -1]], dtype=f32)
    return v, t, org, dirs


def soup_rays(R, seed=1, scale=1.0, offset=0.0):
    """rays between random points of the soup's cube and around it"""
    r = np.random.default_rng(seed)
    a = ((r.random((R, 3)) * 1.5 - 0.25) * scale + offset).astype(f32)
    b = ((r.random((R, 3)) * 1.5 - 0.25) * scale + offset).astype(f32)
    return a, (b - a).astype(f32)


def hostile_rays(R=300, seed=10, verts=None):
    """origins and directions over many decades, a third of them aimed at vertices of the soup, some with zero components"""
    r = np.random.default_rng(seed)
    o = (r.standard_normal((R, 3)) * 10.0 ** r.integers(-6, 12, (R, 1))).astype(f32)
    d = (r.standard_normal((R, 3)) * 10.0 ** r.integers(-20, 18, (R, 1))).astype(f32)
    if verts is not None:
        k = np.arange(0, R, 3)
        with np.errstate(all="ignore"):
            d[k] = (np.asarray(verts, dtype=f32)[r.integers(0, len(verts), len(k))] - o[k]).astype(f32)
    d[1::7, 0] = 0
    d[2::11, 1:] = 0
    d[~np.isfinite(d).all(axis=1)] = 1.0
    return o, d


def hostile_mesh(nt=200, seed=8):
    """dist_cases.hostile_soup with axis-aligned triangles (two equal coordinates on an axis: a box without thickness) among them"""
    v, t = D.hostile_soup(nt, seed)
    v = v.copy()
    for k in range(0, nt, 5):
        v[3 * k:3 * k + 3, k % 3] = v[3 * k, k % 3]
    return v, t


@functools.lru_cache(None)
def spheres_case():
    """three_spheres of surf_cases, 2000 rays from inside and outside, and the brute-force answers for [0, inf) and for a bounded range
    (computed once, read only)"""
    import surf_cases as SF
    v, t = SF.three_spheres()
    r = np.random.default_rng(23)
    sph =SF.sphere()[0].astype(f64).mean(axis=0)
    centres = np.stack([sph + 20.0 * k for k in range(3)])
    o = (centres[r.integers(0, 3, 2000)] + r.standard_normal((2000, 3)) * 1.0).astype(f32)          # inside a sphere
    o[::3] = (centres[1] + r.standard_normal((len(o[::3]), 3)) * 30.0).astype(f32)                    # outside all of them
    d = (v[r.integers(0, len(v), 2000)] - o).astype(f32)                                              # aimed at vertices: segments, t = 1 at the vertex
    d[1::2] = r.standard_normal((1000, 3)).astype(f32)
    index = D.Index(v, t)
    ans = brute(index, o, d)
    near = brute(index, o, d, 0.5, 1.0)
    for a in (v, t, o, d) + ans + near:
        a.setflags(write=False)
    return v, t, o, d, ans, near
