"""include/sta_dist.h restated in numpy: the class of a triangle, the Morton key, the sorted order, the boxes of every level, the closest point
of a triangle in float64 steps (every numpy operation below is one IEEE operation per element, in the header's order), the clamp, and a
brute force over all valid triangles with the tie rule.  The GPU tests compare with array_equal; tests/test_meshdist_cpu.py holds this file
against a second, independent statement (plane and segment projections in numpy.longdouble) and checks the lower-bound property.

It is not Open3D or trimesh: neither is available."""
import functools

import numpy as np

import surf_cases as SF

f64 = np.float64
FANOUT = 8
MAX_LEVELS = 9
KEY_BITS = 21
PLAN_SIZES = 2
COUNTERS = ("valid", "bad_index", "non_finite", "no_area", "status", "reserved_5", "reserved_6", "reserved_7")
VALID, BAD_INDEX, NON_FINITE, NO_AREA = 0, 1, 2, 3
STATUS_BOUND = 1
INVALID_KEY = np.uint64(1) << np.uint64(63)

# The largest |restatement - longdouble statement| of the closest point's DISTANCE, relative to the scale of the case (the largest
# |coordinate| of triangle and query), measured by tests/test_meshdist_cpu.py on its cases (regions(), lattice queries, 4000 random
# triangle / query pairs over six decades, 11851 pairs in all): 2.6e-16.  The test asserts SECOND_STATEMENT_FACTOR times this.
SECOND_STATEMENT_MEASURED = 2.6e-16
SECOND_STATEMENT_FACTOR = 4.0


def _r256(n):
    return (int(n) + 255) & ~255


def level_counts(nt):
    counts = [(int(nt) + FANOUT - 1) // FANOUT]
    while counts[-1] > 1:
        counts.append((counts[-1] + FANOUT - 1) // FANOUT)
    return counts


def plan(nt, Q=1):
    """(index_bytes, build_work_bytes) of sta_tri_plan, its refusals as ValueError with the library's words"""
    nt, Q = int(nt), int(Q)
    if not 1 <= nt < 1 << 27:
        raise ValueError(f"tri_plan: nt must be in [1, 2^27) (got {nt})")
    if not 1 <= Q < 1 << 30:
        raise ValueError(f"tri_plan: Q must be in [1, 2^30) (got {Q})")
    nodes, nbs = sum(level_counts(nt)), (nt + 1023) // 1024
    index = _r256(36 * nt) + _r256(4 * nt) + _r256(24 * nodes) + _r256(32)
    work = 2 * _r256(8 * nt) + 2 * _r256(4 * nt) + _r256(1024 * nbs) + _r256(1024) + _r256(1024 * 64) + _r256(64)
    return index, work


# ------------------------------------------------------------------------------------------ build
def corners(verts, tris):
    """[n,3,3] float32 corners of triangles whose indices are in range"""
    return np.asarray(verts, dtype=np.float32).reshape(-1, 3)[np.asarray(tris).reshape(-1, 3)]


def classify(verts, tris):
    """[nt] class of every triangle: VALID, BAD_INDEX, NON_FINITE, NO_AREA, decided in that order of tests"""
    verts, tris = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    nv = len(verts)
    cls = np.full(len(tris), BAD_INDEX, dtype=np.int32)
    inr = ((tris >= 0) & (tris < nv)).all(axis=1)
    P = corners(verts, tris[inr])
    fin = np.isfinite(P).all(axis=(1, 2))
    sub = np.full(len(P), NON_FINITE, dtype=np.int32)
    w = SF.face(verts, tris[inr][fin])[4]
    sub[fin] = np.where(np.isfinite(w) & (w > 0), VALID, NO_AREA)
    cls[inr] = sub
    return cls


def counters(cls):
    return np.array([(cls == k).sum() for k in range(4)] + [0, 0, 0, 0], dtype=np.int32)


def spread(g):
    """bit b of g -> bit 3 b, one bit at a time"""
    g = np.asarray(g, dtype=np.uint64)
    out = np.zeros_like(g)
    for b in range(KEY_BITS):
        out |= ((g >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def keys(verts, tris, cls=None):
    """[nt] uint64: the Morton key of the box centre of a valid triangle, 2^63 otherwise"""
    cls = classify(verts, tris) if cls is None else cls
    key = np.full(len(cls), INVALID_KEY, dtype=np.uint64)
    ok = cls == VALID
    if not ok.any():
        return key
    P = corners(verts, np.asarray(tris).reshape(-1, 3)[ok])
    m = (P.min(axis=1).astype(f64) + P.max(axis=1).astype(f64)) * 0.5          # [n,3]
    L, U = m.min(axis=0), m.max(axis=0)
    k = np.zeros(len(m), dtype=np.uint64)
    for a in range(3):
        if U[a] == L[a]:
            g = np.zeros(len(m))
        else:
            g = np.floor(((m[:, a] - L[a]) / (U[a] - L[a])) * 2097152.0)
            g = np.minimum(np.maximum(g, 0.0), 2097151.0)
        k |= spread(g.astype(np.uint64)) << np.uint64(a)
    key[ok] = k
    return key


class Index:
    def __init__(self, verts, tris):
        self.verts, self.tris = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(tris, dtype=np.int32).reshape(-1, 3)
        self.nt = len(self.tris)
        self.cls = classify(self.verts, self.tris)
        self.counters = counters(self.cls)
        self.key = keys(self.verts, self.tris, self.cls)
        self.src = np.argsort(self.key, kind="stable").astype(np.int32)          # ascending key, equal keys in ascending index
        self.n_valid = int(self.counters[0])
        self.tri = np.full((self.nt, 9), np.nan, dtype=np.float32)
        self.tri[:self.n_valid] = corners(self.verts, self.tris[self.src[:self.n_valid]]).reshape(-1, 9)
        self.counts = level_counts(self.nt)
        self.boxes = self._boxes()

    def _boxes(self):
        """per level [count, 6] float32: lo xyz, hi xyz; (+inf, -inf) for a node without a valid triangle"""
        inf = np.float32(np.inf)
        n0 = self.counts[0]
        lo, hi = np.full((n0 * FANOUT, 3), inf, dtype=np.float32), np.full((n0 * FANOUT, 3), -inf, dtype=np.float32)
        T = self.tri[:self.n_valid].reshape(-1, 3, 3)
        lo[:self.n_valid], hi[:self.n_valid] = T.min(axis=1), T.max(axis=1)
        out = []
        for cnt in self.counts:
            lo, hi = lo.reshape(cnt, FANOUT, 3).min(axis=1), hi.reshape(cnt, FANOUT, 3).max(axis=1)
            out.append(np.concatenate([lo, hi], axis=1))
            nxt = (cnt + FANOUT - 1) // FANOUT * FANOUT
            lo = np.concatenate([lo, np.full((nxt - cnt, 3), inf, dtype=np.float32)])
            hi = np.concatenate([hi, np.full((nxt - cnt, 3), -inf, dtype=np.float32)])
        return out


# ------------------------------------------------------------------------------------------ query
def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest(q, A, B, Cc):
    """The clamped closest point c [...,3] float64 and d2 [...] of triangles (A, B, C) for queries q, all float32 values broadcast together:
    the rules of the header in their order, the first that applies decides."""
    q, a, b, c = (np.asarray(x, dtype=np.float32).astype(f64) for x in (q, A, B, Cc))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, q - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = q - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = q - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        denom = 1.0 / ((va + vb) + vc)
        v, w = vb * denom, vc * denom
        p = (a + ab * v[..., None]) + ac * w[..., None]
        rules = [
            (va <= 0) & (e1 >= 0) & (e2 >= 0), b + (c - b) * (e1 / (e1 + e2))[..., None],
            (vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * (d2 / (d2 - d6))[..., None],
            (d6 >= 0) & (d5 <= d6), c,
            (vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * (d1 / (d1 - d3))[..., None],
            (d3 >= 0) & (d4 <= d3), b,
            (d1 <= 0) & (d2 <= 0), a,
        ]
        for cond, val in zip(rules[0::2], rules[1::2]):          # the last written is the first rule
            val = np.broadcast_to(val, p.shape)
            p = np.where(cond[..., None], val, p)
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        lo, hi = np.broadcast_to(lo, p.shape), np.broadcast_to(hi, p.shape)
        r = np.where(p >= lo, p, lo)
        r = np.where(r <= hi, r, hi)
        d = q - r
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return r, dd


def brute(index, qry, radius=np.inf, chunk=256):
    """(d2 [Q] float64, tri [Q] int32, point [Q,3] float32): the minimum over ALL valid triangles, lowest index among equal d2"""
    qry = np.asarray(qry, dtype=np.float32).reshape(-1, 3)
    Q = len(qry)
    d2o, trio, pto = np.full(Q, np.inf), np.full(Q, -1, dtype=np.int32), np.full((Q, 3), np.nan, dtype=np.float32)
    ids = np.nonzero(index.cls == VALID)[0]          # ascending, so argmin's first minimum is the lowest index
    if not len(ids):
        return d2o, trio, pto
    P = corners(index.verts, index.tris[ids])
    with np.errstate(all="ignore"):
        r2 = f64(radius) * f64(radius)
    fin = np.isfinite(qry).all(axis=1)
    for s in range(0, Q, chunk):
        q = qry[s:s + chunk]
        c, dd = closest(q[:, None, :], P[None, :, 0], P[None, :, 1], P[None, :, 2])
        j = np.argmin(dd, axis=1)
        rows = np.arange(len(q))
        best = dd[rows, j]
        ok = fin[s:s + chunk] & (best <= r2)
        d2o[s:s + chunk][ok] = best[ok]
        trio[s:s + chunk][ok] = ids[j][ok]
        pto[s:s + chunk][ok] = c[rows, j][ok].astype(np.float32)
    return d2o, trio, pto


def bound(box, q):
    """the lower bound of a box [...,6] float32 for queries q [...,3] float32, in the order of d2's sum"""
    box, q = np.asarray(box, dtype=np.float32).astype(f64), np.asarray(q, dtype=np.float32).astype(f64)
    with np.errstate(all="ignore"):
        e = np.maximum(np.maximum(box[..., :3] - q, q - box[..., 3:]), 0.0)
        return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


# ------------------------------------------------------------------------------------------ meshes and queries
def one_triangle():
    return np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def regions():
    """queries in all seven regions of one_triangle() and on their borders (dyadic, so every step is exact), above, below and in the plane"""
    xy = [(1, 1), (-1, -1), (5, -1), (-1, 5), (2, -1), (-1, 2), (3, 3),           # interior, vertices a b c, edges ab ac bc
          (0, 0), (4, 0), (0, 4), (2, 0), (0, 2), (2, 2),                        # on the corners and edges
          (-1, 0), (0, -1), (4, -1), (5, 0), (5, 1), (-1, 4), (0, 5), (1, 5),      # on the borders between vertex and edge regions
          (6, -2), (-2, 6), (1.5, 2.5), (0.5, 0.25)]
    return np.array([(x, y, z) for z in (0.0, 0.5, -2.0) for x, y in xy], dtype=np.float32)


def lattice(n=4, h=0.25):
    """an (n x n)-quad grid in the plane z = 0 on the dyadic lattice of step h, two triangles per quad -> (verts, tris)"""
    g = np.arange(n + 1, dtype=np.float32) * np.float32(h)
    v = np.stack([np.tile(g, n + 1), np.repeat(g, n + 1), np.zeros((n + 1) ** 2, dtype=np.float32)], axis=1)
    t = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            t += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return v, np.array(t, dtype=np.int32)


def lattice_queries(n=4, h=0.25):
    """queries above shared edges (two triangles at the same distance), above the diagonal, above boundary and interior vertices (four
    and six triangles), at dyadic heights"""
    q = []
    for z in (0.0, 0.125, -0.5):
        for j in range(n + 1):
            for i in range(n + 1):
                q.append((i * h, j * h, z))                      # above a vertex: 1, 2, 3 or 6 triangles
                if i < n:
                    q.append((i * h + h / 2, j * h, z))          # above a horizontal edge
                if j < n:
                    q.append((i * h, j * h + h / 2, z))          # above a vertical edge
                if i < n and j < n:
                    q.append((i * h + h / 2, j * h + h / 2, z))  # above the diagonal
    return np.array(q, dtype=np.float32)


def reversed_duplicated(verts, tris):
    """the triangles reversed in order and winding, then the originals again: every surface point belongs to two triangles"""
    return verts, np.concatenate([tris[::-1, ::-1], tris]).astype(np.int32)


def with_bad(verts, tris, seed=3):
    """bad-index, NaN-vertex and zero-area triangles mixed in under a permutation -> (verts, tris)"""
    r = np.random.default_rng(seed)
    nv = len(verts)
    v = np.concatenate([verts, np.array([[np.nan, 0, 0], [0, np.inf, 0]], dtype=np.float32)])
    k = 9
    extra = np.concatenate([
        np.stack([r.integers(0, nv, k), r.integers(0, nv, k), np.full(k, nv + 2)], axis=1),         # index beyond nv + 2 vertices
        np.stack([np.full(k, -1), r.integers(0, nv, k), r.integers(0, nv, k)], axis=1),
        np.stack([r.integers(0, nv, k), np.full(k, nv), r.integers(0, nv, k)], axis=1),             # the NaN vertex
        np.stack([r.integers(0, nv, k), r.integers(0, nv, k), np.full(k, nv + 1)], axis=1),         # the infinite vertex
        np.repeat(r.integers(0, nv, (k, 1)), 3, axis=1),                                            # a point
        np.stack([np.arange(k), np.arange(k), np.arange(k) + 1], axis=1),                           # an edge
    ]).astype(np.int32)
    t = np.concatenate([tris, extra])
    return v, t[r.permutation(len(t))]


def soup(nt, seed=0, scale=1.0, size=0.2, offset=0.0):
    """nt random small triangles in a cube of side `scale` at `offset`, each on three vertices of its own"""
    r = np.random.default_rng(seed)
    c = r.random((nt, 1, 3)) * scale
    v = (c + (r.random((nt, 3, 3)) - 0.5) * size * scale + offset).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * nt, dtype=np.int32).reshape(nt, 3)


def soup_queries(Q, seed=1, scale=1.0, offset=0.0):
    r = np.random.default_rng(seed)
    return ((r.random((Q, 3)) * 1.5 - 0.25) * scale + offset).astype(np.float32)


def room(n=300, seed=4):
    """one room-sized triangle among n small ones"""
    v, t = soup(n, seed, 1.0, 0.05)
    big = np.array([[-10, -10, 0.5], [12, -10, 0.5], [0, 14, 0.5]], dtype=np.float32)
    return np.concatenate([v, big]), np.concatenate([t[:n // 2], [[3 * n, 3 * n + 1, 3 * n + 2]], t[n // 2:]]).astype(np.int32)


def same_centre(n=70, seed=6):
    """n triangles whose boxes are all [-s, s]^3 for dyadic s: one box centre, every key equal"""
    r = np.random.default_rng(seed)
    v, t = [], []
    for k in range(n):
        s = np.float32(2.0 ** (k % 5 - 2))
        a, b, c = (r.uniform(-1.0, 1.0, 3) * s).astype(np.float32)
        v.append(np.array([[-s, -s, -s], [s, s, a], [b, c, s]], dtype=np.float32))          # every axis reaches -s and +s
        t.append([3 * k, 3 * k + 1, 3 * k + 2])
    return np.concatenate(v), np.array(t, dtype=np.int32)


def hostile_soup(nt=200, seed=8):
    """triangles over many decades of scale, some at 1e6, some huge"""
    r = np.random.default_rng(seed)
    scale = 10.0 ** r.integers(-6, 12, (nt, 1, 1))
    v = (r.standard_normal((nt, 3, 3)) * scale).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * nt, dtype=np.int32).reshape(nt, 3)


def hostile_queries(Q=300, seed=9):
    r = np.random.default_rng(seed)
    return (r.standard_normal((Q, 3)) * 10.0 ** r.integers(-6, 12, (Q, 1))).astype(np.float32)


@functools.lru_cache(None)
def spheres_case():
    """three_spheres of surf_cases, 2000 queries around and between them, and the brute-force answer (computed once, read only)"""
    v, t = SF.three_spheres()
    r = np.random.default_rng(21)
    centre = v.reshape(-1, 3).astype(f64).mean(axis=0)
    q = (v[r.integers(0, len(v), 2000)] + r.standard_normal((2000, 3)) * 0.8).astype(np.float32)
    q[::7] = (centre + r.standard_normal((len(q[::7]), 3)) * 15.0).astype(np.float32)
    ans = brute(Index(v, t), q)
    for a in (v, t, q) + ans:
        a.setflags(write=False)
    return v, t, q, ans
