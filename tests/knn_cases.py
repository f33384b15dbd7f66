"""The numpy restatement that defines the contract of include/sta_knn.h and of the neighbourhood half of vista_slam_amd/cloud.py, and the
case builders of tests/test_knn_cpu.py, tests/test_knn_gpu.py and tests/knn_stream_cases.py.

Every floating-point operation is one float64 operation in the order the header writes it.  `knn_brute` is O(Q M), chunked, and sorts
by (d2, index) with a stable argsort over ascending indices.  The moments come twice: `moments_one` is the header in scalar Python
loops, one query at a time; `moments` runs the same operations over all queries at once - the loop over the list slots stays a
loop, so every query sees its own operations in its own order (numpy's elementwise kernels do not contract) - and
tests/test_knn_cpu.py holds the two against each other bit for bit.
"""
import math

import numpy as np

import cloud_cases as CC

MAX_K = 64
MAX_RINGS = 32
RECORD = 8
MIN_COUNT = 3
SWEEPS = 8
STATUS_BOUND, STATUS_ORDER = 1, 2
ORDERS = ("asc", "rev", "pairwise")

# Measured on this restatement alone by tests/test_knn_cpu.py, which prints them again (the constants are the measured figures rounded up
# to two digits):
#   TOL_EIG   the largest difference between the 8-sweep Jacobi eigenvalues and numpy.linalg.eigh's, relative to the largest
#             eigenvalue, over the covariance matrices of the room and of the sphere (measured 1.15e-15); the eigenvector of l0 against
#             eigh's, as the sine of the angle between them, where the gap l1 - l0 is at least 1e-3 of l2 (measured 5.73e-15).  numpy's own
#             error is part of both figures, so the CPU test asserts 16 times them and not the figures themselves.
#   TOL_SUM   a record entry on floats whose sums round, relative to the sum of |contributions|: the largest spread between the
#             ascending, reversed and pairwise sums over cloud_cases.hostile_cases() (measured 1.49e-15); the GPU's fixed tree is a further order, hence the 16.
TOL_EIG_MEASURED = 1.2e-15
TOL_VEC_MEASURED = 5.8e-15
TOL_SUM_MEASURED = 1.5e-15
TOL_SUM = 16 * TOL_SUM_MEASURED


# ---------------------------------------------------------------------------------------------------------
def plan(M, Q, k):
    for name, v in (("M", M), ("Q", Q)):
        if not 1 <= v < 1 << 30:
            raise ValueError(f"knn_plan: {name} must be in [1, 2^30) (got {v})")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn_plan: k must be in [1, {MAX_K}] (got {k})")
    return (8 * Q * k, 4 * Q * k, (min((Q + 255) // 256, 2048) * RECORD * 8 + 255) & ~255)


def knn_brute(ref, qry, k, radius, self_base=-1, chunk=1024):
    """-> d2 [Q,k] float64 (+inf), idx [Q,k] int32 (-1), count [Q] int32: the k smallest (d2, index) among d2 <= radius*radius;
    non-finite reference points are left out, a non-finite query gets count 0, query i skips reference self_base + i."""
    ref = np.asarray(ref, dtype=np.float32).astype(np.float64)
    q = np.asarray(qry, dtype=np.float32).astype(np.float64)
    Q, M = q.shape[0], ref.shape[0]
    r2 = float(radius) * float(radius)
    ok_ref = np.isfinite(ref).all(axis=1)
    refc = np.where(ok_ref[:, None], ref, 0.0)
    ok_q = np.isfinite(q).all(axis=1)
    d2o, ido, cnt = np.full((Q, k), np.inf), np.full((Q, k), -1, dtype=np.int32), np.zeros(Q, np.int32)
    kk = min(k, M)
    for s in range(0, Q, chunk):
        qq = np.where(ok_q[s:s + chunk, None], q[s:s + chunk], 0.0)
        dx = qq[:, None, 0] - refc[None, :, 0]
        dy = qq[:, None, 1] - refc[None, :, 1]
        dz = qq[:, None, 2] - refc[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        bad = ~ok_ref[None, :] | ~(d2 <= r2) | ~ok_q[s:s + chunk, None]
        if self_base >= 0:
            rows = np.arange(d2.shape[0])
            me = self_base + s + rows
            inside = me < M
            bad[rows[inside], me[inside]] = True
        d2 = np.where(bad, np.inf, d2)
        order = np.argsort(d2, axis=1, kind="stable")[:, :kk]          # stable: the lowest index first among equal d2
        top = np.take_along_axis(d2, order, axis=1)
        hit = np.isfinite(top)
        d2o[s:s + chunk, :kk] = np.where(hit, top, np.inf)
        ido[s:s + chunk, :kk] = np.where(hit, order, -1)
        cnt[s:s + chunk] = hit.sum(axis=1)
    return d2o, ido, cnt


def knn_kdtree(ref, qry, k, radius):
    """The same lists through scipy's cKDTree (float64), for clouds without equal distances: indices and counts only."""
    from scipy.spatial import cKDTree
    ref64 = np.asarray(ref, dtype=np.float32).astype(np.float64)
    q = np.asarray(qry, dtype=np.float32).astype(np.float64)
    kk = min(k, len(ref64))
    _d, j = cKDTree(ref64).query(q, k=kk)
    j = np.asarray(j).reshape(len(q), kk)
    p = ref64[j]
    dx, dy, dz = q[:, None, 0] - p[..., 0], q[:, None, 1] - p[..., 1], q[:, None, 2] - p[..., 2]
    hit = (dx * dx + dy * dy) + dz * dz <= float(radius) * float(radius)
    idx = np.full((len(q), k), -1, np.int32)
    idx[:, :kk] = np.where(hit, j, -1)
    return idx, hit.sum(axis=1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------
def _div(a, b):
    """IEEE division, also by zero"""
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _rot(a, V, p, q, r):
    """one rotation of the header on the upper triangle a (a dict keyed by (i, j), i <= j) and the eigenvector matrix V (3 lists)"""
    apq = a[(p, q)]
    if not apq != 0.0:
        return
    rp, rq = (min(r, p), max(r, p)), (min(r, q), max(r, q))
    theta = _div(a[(q, q)] - a[(p, p)], 2.0 * apq)
    h = math.sqrt(theta * theta + 1.0) if theta == theta else math.nan
    t = _div(1.0, abs(theta) + h)
    if theta < 0.0:
        t = -t
    c = _div(1.0, math.sqrt(t * t + 1.0)) if t == t else math.nan
    s = t * c
    z = t * apq
    a[(p, p)] = a[(p, p)] - z
    a[(q, q)] = a[(q, q)] + z
    a[(p, q)] = 0.0
    arp, arq = a[rp], a[rq]
    a[rp], a[rq] = c * arp - s * arq, s * arp + c * arq
    for k in range(3):
        vp, vq = V[k][p], V[k][q]
        V[k][p], V[k][q] = c * vp - s * vq, s * vp + c * vq


def jacobi(a00, a01, a02, a11, a12, a22):
    """-> ([a00, a11, a22], V) after SWEEPS cyclic sweeps over (0,1), (0,2), (1,2)"""
    a = {(0, 0): float(a00), (0, 1): float(a01), (0, 2): float(a02), (1, 1): float(a11), (1, 2): float(a12), (2, 2): float(a22)}
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        _rot(a, V, 0, 1, 2)
        _rot(a, V, 0, 2, 1)
        _rot(a, V, 1, 2, 0)
    return [a[(0, 0)], a[(1, 1)], a[(2, 2)]], V


def ranks(l):
    """the rank of each of three values in the stable ascending order (the lowest column first among equals)"""
    return (int(l[1] < l[0]) + int(l[2] < l[0]), int(l[0] <= l[1]) + int(l[2] < l[1]), int(l[0] <= l[2]) + int(l[1] <= l[2]))


def _pick(rk, vals, want):
    return vals[0] if rk[0] == want else vals[1] if rk[1] == want else vals[2]


def moments_one(ref64, q, d2, idx, count, k, view, min_count):
    """The header for one query in scalar loops -> (normal [3] float32, curv, mean_dist, c).  ref64: [M,3] float64 of the fp32
    reference; q: the query as 3 floats or None; view: 3 floats or None."""
    M = len(ref64)
    c = min(max(int(count), 0), k)
    sd = sx = sy = sz = 0.0
    for j in range(c):
        v = int(idx[j])
        if v < 0 or v >= M:
            c = j
            break
        sd = sd + math.sqrt(d2[j])
        sx = sx + ref64[v][0]; sy = sy + ref64[v][1]; sz = sz + ref64[v][2]
    md = sd / c if c >= 1 else math.inf
    nan = math.nan
    if c < min_count:
        return np.array([nan, nan, nan], np.float32), nan, md, c
    mx, my, mz = sx / c, sy / c, sz / c
    a00 = a01 = a02 = a11 = a12 = a22 = 0.0
    for j in range(c):
        p = ref64[int(idx[j])]
        dx, dy, dz = p[0] - mx, p[1] - my, p[2] - mz
        a00 = a00 + dx * dx; a01 = a01 + dx * dy; a02 = a02 + dx * dz
        a11 = a11 + dy * dy; a12 = a12 + dy * dz; a22 = a22 + dz * dz
    l, V = jacobi(a00, a01, a02, a11, a12, a22)
    rk = ranks(l)
    l0, l1, l2 = _pick(rk, l, 0), _pick(rk, l, 1), _pick(rk, l, 2)
    e = [_pick(rk, V[a], 0) for a in range(3)]
    ln = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    n = [_div(e[0], ln), _div(e[1], ln), _div(e[2], ln)]
    if view is not None:
        flip = ((view[0] - q[0]) * n[0] + (view[1] - q[1]) * n[1]) + (view[2] - q[2]) * n[2] < 0.0
    else:
        big = n[0]
        if abs(n[1]) > abs(big):
            big = n[1]
        if abs(n[2]) > abs(big):
            big = n[2]
        flip = big < 0.0
    if flip:
        n = [-n[0], -n[1], -n[2]]
    tr = (l0 + l1) + l2
    with np.errstate(over="ignore"):
        return np.array(n, np.float64).astype(np.float32), (0.0 if tr == 0.0 else _div(l0, tr)), md, c


def _vrot(A, V, p, q, r):
    """_rot over arrays: A a dict of [Q] arrays, V a 3x3 list of [Q] arrays; a query whose a_pq is 0 keeps its values"""
    apq = A[(p, q)]
    on = apq != 0.0
    rp, rq = (min(r, p), max(r, p)), (min(r, q), max(r, q))
    safe = np.where(on, apq, 1.0)
    theta = (A[(q, q)] - A[(p, p)]) / (2.0 * safe)
    h = np.sqrt(theta * theta + 1.0)
    t = 1.0 / (np.abs(theta) + h)
    t = np.where(theta < 0.0, -t, t)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    z = t * safe
    A[(p, p)] = np.where(on, A[(p, p)] - z, A[(p, p)])
    A[(q, q)] = np.where(on, A[(q, q)] + z, A[(q, q)])
    A[(p, q)] = np.where(on, 0.0, apq)
    arp, arq = A[rp], A[rq]
    A[rp], A[rq] = np.where(on, c * arp - s * arq, arp), np.where(on, s * arp + c * arq, arq)
    for k in range(3):
        vp, vq = V[k][p], V[k][q]
        V[k][p], V[k][q] = np.where(on, c * vp - s * vq, vp), np.where(on, s * vp + c * vq, vq)


def moments(ref, qry, d2, idx, count, view=None, min_count=MIN_COUNT):
    """-> dict(normal [Q,3] float32, curv [Q], mean_dist [Q], c [Q]) - `moments_one` for every query, the same operations in the same
    order.  view: None, [3] or [Q,3]."""
    ref64 = np.asarray(ref, dtype=np.float32).astype(np.float64)
    M = len(ref64)
    Q, k = idx.shape
    c = np.clip(np.asarray(count, np.int64), 0, k)
    slot = np.arange(k)[None, :]
    bad = ((idx < 0) | (idx >= M)) & (slot < c[:, None])
    c = np.where(bad.any(axis=1), np.argmax(bad, axis=1), c)
    sd, s = np.zeros(Q), [np.zeros(Q), np.zeros(Q), np.zeros(Q)]
    safe = np.where((idx >= 0) & (idx < M), idx, 0)
    with np.errstate(all="ignore"):
        for j in range(k):
            on = j < c
            if not on.any():
                break
            sd = np.where(on, sd + np.sqrt(np.where(on, d2[:, j], 0.0)), sd)
            p = ref64[safe[:, j]]
            for a in range(3):
                s[a] = np.where(on, s[a] + p[:, a], s[a])
        n = c.astype(np.float64)
        md = np.where(c >= 1, sd / np.where(c >= 1, n, 1.0), np.inf)
        full = c >= min_count
        if not full.any():
            return dict(normal=np.full((Q, 3), np.nan, np.float32), curv=np.full(Q, np.nan), mean_dist=md, c=c.astype(np.int32))
        nn = np.where(full, n, 1.0)
        m = [s[a] / nn for a in range(3)]
        keys = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        A = {key: np.zeros(Q) for key in keys}
        for j in range(k):
            on = j < c
            if not on.any():
                break
            p = ref64[safe[:, j]]
            d = [p[:, a] - m[a] for a in range(3)]
            for (a, b) in keys:
                A[(a, b)] = np.where(on, A[(a, b)] + d[a] * d[b], A[(a, b)])
        V = [[np.full(Q, 1.0 if a == b else 0.0) for b in range(3)] for a in range(3)]
        for _ in range(SWEEPS):
            _vrot(A, V, 0, 1, 2)
            _vrot(A, V, 0, 2, 1)
            _vrot(A, V, 1, 2, 0)
        l = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
        rk = ((l[1] < l[0]).astype(int) + (l[2] < l[0]), (l[0] <= l[1]).astype(int) + (l[2] < l[1]), (l[0] <= l[2]).astype(int) + (l[1] <= l[2]))

        def pick(vals, want):
            return np.where(rk[0] == want, vals[0], np.where(rk[1] == want, vals[1], vals[2]))
        l0, l1, l2 = pick(l, 0), pick(l, 1), pick(l, 2)
        e = [pick(V[a], 0) for a in range(3)]
        ln = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        nv = [e[a] / ln for a in range(3)]
        if view is not None:
            q = np.asarray(qry, dtype=np.float32).astype(np.float64)
            w = np.asarray(view)
            w = np.broadcast_to(w.astype(np.float64) if w.ndim == 1 else w.astype(np.float32).astype(np.float64), (Q, 3))
            flip = ((w[:, 0] - q[:, 0]) * nv[0] + (w[:, 1] - q[:, 1]) * nv[1]) + (w[:, 2] - q[:, 2]) * nv[2] < 0.0
        else:
            big = nv[0]
            big = np.where(np.abs(nv[1]) > np.abs(big), nv[1], big)
            big = np.where(np.abs(nv[2]) > np.abs(big), nv[2], big)
            flip = big < 0.0
        nv = [np.where(flip, -x, x) for x in nv]
        tr = (l0 + l1) + l2
        curv = np.where(tr == 0.0, 0.0, l0 / np.where(tr == 0.0, 1.0, tr))
        normal = np.stack([np.where(full, x, np.nan) for x in nv], axis=1).astype(np.float32)
    return dict(normal=normal, curv=np.where(full, curv, np.nan), mean_dist=md, c=c.astype(np.int32))


def contributions(mean_dist, c, min_count=MIN_COUNT):
    """[Q, 8]: what each query adds to the record"""
    out = np.zeros((len(c), RECORD))
    has = c >= 1
    out[has, 0] = 1.0
    out[has, 1] = mean_dist[has]
    out[has, 2] = mean_dist[has] * mean_dist[has]
    out[c >= min_count, 3] = 1.0
    return out


def record(mean_dist, c, min_count=MIN_COUNT, order="asc"):
    return CC.sum_rows(contributions(mean_dist, c, min_count), order)


# ---------------------------------------------------------------------------------------------------------
# the filters and the normals of vista_slam_amd/cloud.py
def statistical_threshold(rec, std_ratio):
    r0, r1, r2 = float(rec[0]), float(rec[1]), float(rec[2])
    mean = r1 / r0 if r0 > 0 else 0.0
    std = float(np.sqrt(max(0.0, (r2 - r0 * mean * mean) / (r0 - 1.0)))) if r0 > 1 else 0.0
    return mean + float(std_ratio) * std


def remove_statistical_outlier(points, nb_neighbors, std_ratio, radius, order="asc", nn=None):
    """-> (kept indices int64, mask, mean_dist, record)"""
    d2, idx, cnt = knn_brute(points, points, nb_neighbors, radius, self_base=0) if nn is None else nn
    mo = moments(points, points, d2, idx, cnt)
    rec = record(mo["mean_dist"], mo["c"], order=order)
    mask = mo["mean_dist"] <= statistical_threshold(rec, std_ratio)
    return np.flatnonzero(mask).astype(np.int64), mask, mo["mean_dist"], rec


def remove_radius_outlier(points, nb_points, radius):
    _d2, _idx, cnt = knn_brute(points, points, nb_points, radius, self_base=0)
    mask = cnt >= nb_points
    return np.flatnonzero(mask).astype(np.int64), mask


def estimate_normals(points, k, radius, view=None, min_count=MIN_COUNT):
    d2, idx, cnt = knn_brute(points, points, k, radius)
    mo = moments(points, points, d2, idx, cnt, view, min_count)
    return mo["normal"], mo["curv"]


# ---------------------------------------------------------------------------------------------------------
# case builders
ROOM_SIZE = (4.0, 3.0, 2.5)


def room_with_floaters():
    """cloud_cases.box_room(2000, 0) and 40 floaters drawn uniformly at least 0.4 inside it (default_rng(5)) -> (points [2040,3] fp32,
    is_floater [2040] bool)"""
    room = CC.box_room(2000, 0)
    rng = np.random.default_rng(5)
    fl = (0.4 + rng.uniform(0.0, 1.0, (40, 3)) * (np.asarray(ROOM_SIZE) - 0.8)).astype(np.float32)
    return np.concatenate([room, fl]), np.arange(2040) >= 2000


def wall_axis(points, margin=0.5):
    """For the room points at least `margin` from every edge of their wall: (rows, the axis of the wall)"""
    p = np.asarray(points, np.float64)
    size = np.asarray(ROOM_SIZE)
    on = (p == 0.0) | (p == size[None, :])
    one = on.sum(axis=1) == 1
    axis = np.argmax(on, axis=1)
    inner = np.ones(len(p), bool)
    for a in range(3):
        off = (axis != a)
        inner &= ~off | ((p[:, a] >= margin) & (p[:, a] <= size[a] - margin))
    rows = np.flatnonzero(one & inner)
    return rows, axis[rows]


def sphere(n=3000, seed=3):
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, 1.0, (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def angle_deg(n, axis_vec):
    """the unsigned angle between the rows of n and of axis_vec, in degrees"""
    n = np.asarray(n, np.float64)
    a = np.asarray(axis_vec, np.float64)
    cr = np.linalg.norm(np.cross(n, a), axis=1)
    dt = np.abs((n * a).sum(axis=1))
    return np.degrees(np.arctan2(cr, dt))


def dyadic_lattice(M, seed, span=6, step=0.25):
    """M points on a dyadic lattice, many of them equal or equidistant: the tie rule decides most lists"""
    return CC.lattice(M, step, seed=seed, span=span)


def lattice_planes():
    """a 9 x 9 dyadic lattice in each of the planes z = 0.5 and z = 3: every covariance sum is exact and a_02 = a_12 = a_22 = 0"""
    g = np.stack(np.meshgrid(np.arange(9) * 0.25, np.arange(9) * 0.25, indexing="ij"), axis=-1).reshape(-1, 2)
    return np.concatenate([np.concatenate([g, np.full((81, 1), z)], axis=1) for z in (0.5, 3.0)]).astype(np.float32)


def _case(ref, qry, k, radius, cell, exact=True):
    return dict(ref=np.ascontiguousarray(ref, dtype=np.float32), qry=np.ascontiguousarray(qry, dtype=np.float32), k=int(k), radius=float(radius),
                cell=float(cell), exact=exact)


def _sized(M, Q, k, seed=0):
    rng = np.random.default_rng(1000 * k + Q + seed)
    return _case(dyadic_lattice(M, M + k + seed), rng.integers(-14, 15, (Q, 3)) * 0.125, k, 1.0, 0.5)


def _poisoned():
    c = _sized(700, 257, 7, seed=4)
    ref, qry = c["ref"].copy(), c["qry"].copy()
    ref[::7, 0] = np.nan
    ref[3::11, 2] = np.inf
    ref[5::13, 1] = -np.inf
    qry[::5, 1] = np.nan
    qry[1::9, 0] = np.inf
    return _case(ref, qry, 7, 1.0, 0.5)


def _far():
    c = _sized(500, 40, 16, seed=5)
    far = np.array([[3e38, 0, 0], [-3e38, 3e38, -3e38], [0, 1e30, 0], [1e30, 1e30, 1e30], [0, 0, -1e30], [3e38, 3e38, 3e38]])
    return _case(c["ref"], np.concatenate([c["qry"], far]), 16, 1.0, 0.5)


def _hostile(i, k):
    name, ref, qry, _T, radius = CC.hostile_cases()[i]
    cell = 0.1 if name != "offset_1e4" else 0.05
    return _case(ref, qry[:257], k, 10.0 * radius if name != "offset_1e4" else 1.5, cell, exact=False)      # 10 and 30 cells: full lists at k = 7, most at 33


# k in {1, 2, 7, 16, 33, 64} x Q in {1, 63, 64, 65, 257} x M from 1 to about 3000, spread over the cases
CASES = {
    "m1_q1_k1": lambda: _case([[0.25, -0.5, 1.0]], [[0.5, -0.5, 1.0]], 1, 0.25, 0.5),
    "m1_q63_k2_k_above_m": lambda: _sized(1, 63, 2),
    "m5_q64_k7_k_above_m": lambda: _sized(5, 64, 7),
    "m40_q65_k64_k_above_m": lambda: _sized(40, 65, 64),
    "m300_q257_k16": lambda: _sized(300, 257, 16),
    "m1000_q65_k33": lambda: _sized(1000, 65, 33),
    "m3000_q257_k64": lambda: _sized(3000, 257, 64),
    "m3000_q64_k2": lambda: _sized(3000, 64, 2),
    "m2000_q63_k1": lambda: _sized(2000, 63, 1),
    "one_point_100_times": lambda: _case(np.concatenate([np.tile([[0.5, 0.25, -0.75]], (100, 1)), dyadic_lattice(50, 3)]),
                                         np.concatenate([[[0.5, 0.25, -0.75]], dyadic_lattice(64, 9, span=4)]), 33, 1.0, 0.5),
    "fewer_than_k_in_the_radius": lambda: _case(dyadic_lattice(400, 21, span=12), dyadic_lattice(65, 22, span=12), 16, 0.25, 0.25),
    "radius_0": lambda: _case(dyadic_lattice(600, 31, span=3), dyadic_lattice(65, 32, span=3), 7, 0.0, 0.25),
    "radius_of_32_cells": lambda: _case(CC.lattice(300, 0.25, seed=6, span=40), CC.lattice(63, 0.25, seed=7, span=60), 16, 32 * 0.125, 0.125),
    "nan_and_inf": _poisoned,
    "far_queries": _far,
    "nothing_finite": lambda: _case([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf]], [[0, 0, 0], [1, 2, 3]], 2, 1.0, 0.5),
    "hostile_normal_k7": lambda: _hostile(0, 7),
    "hostile_offset_1e4_k16": lambda: _hostile(1, 16),
    "hostile_normal_k33": lambda: _hostile(0, 33),
}
SELF_CASES = {                       # a cloud against itself: exclude_self whole and in chunks, with and without `order`
    "self_lattice_k7": lambda: _case(dyadic_lattice(257, 41), dyadic_lattice(257, 41), 7, 1.0, 0.5),
    "self_lattice_k64": lambda: _case(dyadic_lattice(333, 42, span=3), dyadic_lattice(333, 42, span=3), 64, 1.0, 0.5),
    "self_hostile_k16": lambda: _case(CC.hostile_cases()[0][1][:700], CC.hostile_cases()[0][1][:700], 16, 0.6, 0.2, exact=False),
}

_expected = {}


def expected_of(name, self_base=-1):
    """(case, dict(d2, idx, count)) - computed once per session"""
    key = (name, self_base)
    if key not in _expected:
        c = (CASES.get(name) or SELF_CASES[name])()
        d2, idx, cnt = knn_brute(c["ref"], c["qry"], c["k"], c["radius"], self_base)
        _expected[key] = (c, dict(d2=d2, idx=idx, count=cnt))
    return _expected[key]
