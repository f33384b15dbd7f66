"""The yardstick of libsta_simp.so: a numpy restatement of include/sta_simp.h - cells and their ranks, the surviving triangles, the used
cells, and the placement in scalar float64 loops (every floating-point operation is one Python float operation, which is one IEEE float64
operation: nothing is contracted) -, and the case builders of tests/test_simp_cpu.py and tests/test_simp_gpu.py.  Host-only importable.

It is NOT Open3D's simplify_vertex_clustering and not MeshLab's clustering decimation: neither was available to compare against -
DESIGN.md section 9.  tests/test_simp_cpu.py holds it against a second, naive statement (dicts and sets, numpy.linalg.eigh / lstsq).

Measured there, on every case of PLACE_CASES (the largest |difference| of a float64 position, quadric placement):
  Jacobi restatement against numpy.linalg.eigh with the same threshold rule: JACOBI_VS_EIGH_MEASURED, asserted at 16 times that.
  On `crease` and `corner`, restatement against numpy.linalg.lstsq of the stacked plane equations: LSTSQ_MEASURED, asserted at 16 times that.
"""
import functools
import math

import numpy as np

import mesh_cases as MC

SWEEPS = 8
INDEX_BITS = 21
BIAS = 1 << 20
PLAN_SIZES = 3
COUNTERS = ("cells", "vertices", "triangles", "dropped_vertices", "invalid_triangles", "collapsed", "duplicates", "fallbacks")
PLACE_MEAN, PLACE_QUADRIC = 0, 1
VOX_TILE = 1024
f64 = np.float64

JACOBI_VS_EIGH_MEASURED = 2.0e-14     # largest over PLACE_CASES: sphere_shifted 1.954e-14 (sphere_2 1.843e-14, hostile 2.2e-15, crease and corner 0)
JACOBI_VS_EIGH_BOUND = 16 * JACOBI_VS_EIGH_MEASURED
LSTSQ_MEASURED = 1.2e-16              # crease: 1.110e-16 off the lstsq point, 0 off both planes; corner: 0 off the lstsq point and the corner
LSTSQ_BOUND = 16 * LSTSQ_MEASURED


def _r256(n):
    return (n + 255) // 256 * 256


def _sort_bytes(m):
    return 2 * _r256(8 * m) + 2 * _r256(4 * m) + _r256(256 * 4 * ((m + VOX_TILE - 1) // VOX_TILE)) + _r256(256 * 4)


def _scan_bytes(n):
    nb = (n + 255) // 256
    return _r256(4 * nb) + _r256(8 * (nb + 1))


def plan(nt, nv):
    """sta_simp_plan: (bytes of the work of cells, triangles, place); its refusals as ValueError."""
    if not 0 <= nv < 2 ** 31:
        raise ValueError(f"simp_plan: nv must be in [0, 2^31) (got {nv})")
    if not (0 <= nt < 2 ** 31 and 3 * nt < 2 ** 31):
        raise ValueError(f"simp_plan: nt must be >= 0 and 3 * nt below 2^31 (got nt = {nt})")
    return (_sort_bytes(nv) + _scan_bytes(nv),
            _sort_bytes(nt) + _scan_bytes(nt) + _scan_bytes(nv) + _r256(4 * nt) + _r256(4 * nv),
            _sort_bytes(nv) + _sort_bytes(3 * nt))


def _origin(origin):
    return np.zeros(3, f64) if origin is None else np.asarray(origin, f64).reshape(3)


# ------------------------------------------------------------------------------------------ stage 1
def cell_indices(verts, cell, origin=None):
    """-> (kept [nv] bool, index [nv,3] int64 (0 where dropped))"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        f = np.floor((verts.astype(f64) - _origin(origin)) / f64(cell))
        kept = np.isfinite(verts).all(axis=1) & ((f >= -BIAS) & (f < BIAS)).all(axis=1)
    return kept, np.where(kept[:, None], f, 0.0).astype(np.int64)


def cells(verts, cell, origin=None):
    """-> (vcell [nv] int32, number of cells, number of dropped vertices)"""
    kept, i = cell_indices(verts, cell, origin)
    key = ((i[:, 2] + BIAS) << 42) | ((i[:, 1] + BIAS) << 21) | (i[:, 0] + BIAS)
    uniq, inv = np.unique(key[kept], return_inverse=True)
    vcell = np.full(len(kept), -1, np.int32)
    vcell[kept] = inv.astype(np.int32)
    return vcell, len(uniq), int((~kept).sum())


# ------------------------------------------------------------------------------------------ stage 2
def triples(tris, nv, vcell):
    """-> (valid [nt] bool, collapsed [nt] bool, cluster triples [nt,3] (anything where not valid))"""
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    inside = ((tris >= 0) & (tris < nv)).all(axis=1)
    c = vcell[np.clip(tris, 0, max(nv - 1, 0))] if nv else np.full(tris.shape, -1, np.int32)
    valid = inside & (c >= 0).all(axis=1)
    collapsed = valid & ((c[:, 0] == c[:, 1]) | (c[:, 1] == c[:, 2]) | (c[:, 0] == c[:, 2]))
    return valid, collapsed, c


def triangles(tris, nv, vcell):
    """-> dict(tris_out [nt,3], tri_src [nt], cell_out [nv], vmap [nv], n_verts, n_tris, invalid, collapsed, duplicates)"""
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    nt = len(tris)
    valid, collapsed, c = triples(tris, nv, vcell)
    cand = np.nonzero(valid & ~collapsed)[0]
    s = np.sort(c[cand], axis=1)
    order = np.lexsort((cand, s[:, 2], s[:, 1], s[:, 0]))
    ss = s[order]
    first = np.ones(len(order), bool)
    first[1:] = (ss[1:] != ss[:-1]).any(axis=1)
    surv = np.sort(cand[order[first]])
    cs = c[surv]
    k = cs.argmin(axis=1) if len(surv) else np.zeros(0, np.int64)
    rot = np.stack([cs[np.arange(len(surv)), (k + j) % 3] for j in range(3)], axis=1) if len(surv) else np.zeros((0, 3), np.int32)
    cell_out = np.full(nv, -1, np.int32)
    used = np.unique(rot)
    cell_out[used] = np.arange(len(used), dtype=np.int32)
    tris_out = np.full((nt, 3), -1, np.int32)
    tris_out[:len(surv)] = cell_out[rot]
    tri_src = np.full(nt, -1, np.int32)
    tri_src[:len(surv)] = surv
    vmap = np.where(vcell >= 0, cell_out[np.clip(vcell, 0, None)], -1).astype(np.int32) if nv else np.zeros(0, np.int32)
    return {"tris_out": tris_out, "tri_src": tri_src, "cell_out": cell_out, "vmap": vmap, "n_verts": len(used), "n_tris": len(surv),
            "invalid": int((~valid).sum()), "collapsed": int(collapsed.sum()), "duplicates": len(cand) - len(surv)}


# ------------------------------------------------------------------------------------------ stage 3
def _div(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _rot(a, V, p, q, r):
    """one rotation of the header on the upper triangle a (a dict keyed by (i, j), i <= j) and the eigenvector matrix V (3 lists)"""
    pq = (p, q)
    apq = a[pq]
    if apq == 0.0:
        return
    rp, rq = (min(r, p), max(r, p)), (min(r, q), max(r, q))
    theta = _div(a[(q, q)] - a[(p, p)], 2.0 * apq)
    h = math.sqrt(theta * theta + 1.0)
    t = _div(1.0, abs(theta) + h)
    if theta < 0.0:
        t = -t
    c = _div(1.0, math.sqrt(t * t + 1.0))
    s = t * c
    z = t * apq
    a[(p, p)] = a[(p, p)] - z
    a[(q, q)] = a[(q, q)] + z
    a[pq] = 0.0
    arp, arq = a[rp], a[rq]
    a[rp], a[rq] = c * arp - s * arq, s * arp + c * arq
    for k in range(3):
        vp, vq = V[k][p], V[k][q]
        V[k][p], V[k][q] = c * vp - s * vq, s * vp + c * vq


def jacobi(q00, q01, q02, q11, q12, q22):
    """-> ([l_0, l_1, l_2], V) after SWEEPS cyclic sweeps in the header's order"""
    a = {(0, 0): float(q00), (0, 1): float(q01), (0, 2): float(q02), (1, 1): float(q11), (1, 2): float(q12), (2, 2): float(q22)}
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        _rot(a, V, 0, 1, 2)
        _rot(a, V, 0, 2, 1)
        _rot(a, V, 1, 2, 0)
    return [a[(0, 0)], a[(1, 1)], a[(2, 2)]], V


def _finite(x):
    return abs(x) <= 1.7976931348623157e308


def quadric_of(vd, tri_list, m):
    """the nine sums of a cell: Q (six entries) and g, over its (triangle, corner) pairs in the given order"""
    q00 = q01 = q02 = q11 = q12 = q22 = g0 = g1 = g2 = 0.0
    for ia, ib, ic in tri_list:
        A, B, C = vd[ia], vd[ib], vd[ic]
        ux, uy, uz = B[0] - A[0], B[1] - A[1], B[2] - A[2]
        wx, wy, wz = C[0] - A[0], C[1] - A[1], C[2] - A[2]
        nx, ny, nz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
        if not (_finite(nx) and _finite(ny) and _finite(nz)):
            continue
        q00 = q00 + nx * nx; q01 = q01 + nx * ny; q02 = q02 + nx * nz
        q11 = q11 + ny * ny; q12 = q12 + ny * nz; q22 = q22 + nz * nz
        d = (nx * (m[0] - A[0]) + ny * (m[1] - A[1])) + nz * (m[2] - A[2])
        g0 = g0 + nx * d; g1 = g1 + ny * d; g2 = g2 + nz * d
    return (q00, q01, q02, q11, q12, q22), (g0, g1, g2)


def solve(Q, g, m, sv_ratio):
    """-> (x, lmax) of the header from the nine sums"""
    l, V = jacobi(*Q)
    lmax = l[0]
    if l[1] > lmax:
        lmax = l[1]
    if l[2] > lmax:
        lmax = l[2]
    thr = sv_ratio * lmax
    y = [0.0, 0.0, 0.0]
    for i in range(3):
        if l[i] > thr:
            w = _div((V[0][i] * g[0] + V[1][i] * g[1]) + V[2][i] * g[2], l[i])
            for k in range(3):
                y[k] = y[k] + V[k][i] * w
    return [m[k] - y[k] for k in range(3)], lmax


def cell_members(tris, nv, vcell, cell_out):
    """-> (vertices of every used cell in ascending v, (i0, i1, i2) of every (valid triangle, corner) pair of it in ascending 3 t + j)"""
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    members = {int(c): [] for c in np.nonzero(cell_out >= 0)[0]}
    pairs = {c: [] for c in members}
    for v in range(nv):
        c = int(vcell[v])
        if c in members:
            members[c].append(v)
    valid, _collapsed, c3 = triples(tris, nv, vcell)
    tl = tris.tolist()
    for t in np.nonzero(valid)[0]:
        for j in range(3):
            c = int(c3[t, j])
            if c in pairs:
                pairs[c].append(tuple(tl[t]))
    return members, pairs


def place(verts, colors, tris, vcell, cell_out, cell, origin=None, placement=PLACE_QUADRIC, sv_ratio=1e-3):
    """-> dict(verts [n,3] f32, colors [n,3] f32 or None, x64 [n,3] f64 (before the rounding), mean64 [n,3], fallbacks, fell [n] bool)"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    nv = len(verts)
    o = _origin(origin).tolist()
    cell = float(cell)
    n_out = int((cell_out >= 0).sum())
    vd = verts.astype(f64).tolist()
    cd = None if colors is None else np.asarray(colors, np.float32).astype(f64).tolist()
    _kept, index = cell_indices(verts, cell, origin)
    members, pairs = cell_members(tris, nv, vcell, cell_out)
    x64 = np.zeros((n_out, 3), f64)
    m64 = np.zeros((n_out, 3), f64)
    c64 = np.zeros((n_out, 3), f64)
    fell = np.zeros(n_out, bool)
    for c, vs in members.items():
        row = int(cell_out[c])
        s = [0.0, 0.0, 0.0]
        sc = [0.0, 0.0, 0.0]
        for v in vs:
            for k in range(3):
                s[k] = s[k] + vd[v][k]
                if cd is not None:
                    sc[k] = sc[k] + cd[v][k]
        n = float(len(vs))
        m = [s[k] / n for k in range(3)]
        m64[row] = m
        c64[row] = [sc[k] / n for k in range(3)]
        x = m
        if placement == PLACE_QUADRIC:
            Q, g = quadric_of(vd, pairs[c], m)
            q, lmax = solve(Q, g, m, float(sv_ratio))
            ok = lmax > 0.0 and all(_finite(v) for v in q)
            if ok:
                i3 = index[vs[0]].tolist()
                for k in range(3):
                    lo, hi = o[k] + float(i3[k]) * cell, o[k] + float(i3[k] + 1) * cell
                    ok = ok and lo <= q[k] <= hi
            if ok:
                x = q
            else:
                fell[row] = True
        x64[row] = x
    with np.errstate(over="ignore"):
        return {"verts": x64.astype(np.float32), "colors": None if colors is None else c64.astype(np.float32), "x64": x64, "mean64": m64,
                "fallbacks": int(fell.sum()), "fell": fell}


def simplify(verts, colors, tris, cell, origin=None, placement=PLACE_QUADRIC, sv_ratio=1e-3):
    """the whole contract -> dict: vcell, the outputs of `triangles`, of `place`, and counters (the eight, in the header's order)"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    nv = len(verts)
    vcell, n_cells, dropped = cells(verts, cell, origin)
    out = triangles(tris, nv, vcell)
    out.update(place(verts, colors, tris, vcell, out["cell_out"], cell, origin, placement, sv_ratio))
    out["vcell"] = vcell
    out["counters"] = (n_cells, out["n_verts"], out["n_tris"], dropped, out["invalid"], out["collapsed"], out["duplicates"], out["fallbacks"])
    return out


# ------------------------------------------------------------------------------------------ cases: (verts, colors, tris, cell, origin)
def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def sphere(cell=2.0, origin=None):
    """the analytic TSDF sphere (1064 vertices, 2124 triangles, voxel size 1)"""
    v, t, col = MC.sphere_mesh()
    return v, col, t, cell, origin


@functools.lru_cache(None)
def identity():
    """the sphere on cells of half its smallest Chebyshev vertex distance: every vertex has a cell of its own"""
    v, t, col = MC.sphere_mesh()
    p = v.astype(f64)
    best = np.inf
    for i in range(len(p) - 1):
        best = min(best, np.abs(p[i + 1:] - p[i]).max(axis=1).min())
    assert best > 0
    return v, col, t, float(best) / 2.0, None


def one_cell():
    v, t, col = MC.sphere_mesh()
    return v, col, t, 64.0, (-32.0, -32.0, -32.0)


@functools.lru_cache(None)
def hostile():
    """4101 triangles on 1501 vertices, cell 0.5: dyadic coordinates in [-4, 4) (many exactly on cell faces, negative indices), NaN / Inf
    vertices, vertices beyond and exactly at the +-2^20 range, indices out of range, repeated indices, triangles inside one cell and
    across two, copies of triangles in both windings and all rotations, different triangles of the same three cells, collinear (zero-area)
    triangles across three cells, and a vertex that no triangle names in a cell that is used."""
    r = np.random.default_rng(41)
    nv, nt, cell = 1501, 4101, 0.5
    v = (r.integers(-32, 32, (nv, 3)) / 8.0).astype(np.float32)
    v[r.choice(nv, 300, replace=False)] += r.uniform(0, 0.124, (300, 3)).astype(np.float32)
    col = r.random((nv, 3)).astype(np.float32)
    v[5] = np.nan
    v[6, 1] = np.inf
    v[7, 2] = -np.inf
    v[8] = (1e7, 0, 0)                    # beyond the range
    v[9] = (0, 524288.0, 0)               # index 2^20 exactly: dropped
    v[10] = (0, 0, -524288.0)             # index -2^20 exactly: kept
    v[11] = (0, 0, -524288.5)             # index -2^20 - 1: dropped
    v[12], v[13], v[14] = (0, 0, 0), (1, 0, 0), (2, 0, 0)         # collinear, three cells
    v[15] = v[20]                         # never named below, shares its cell with vertex 20
    t = r.integers(16, nv, (nt, 3)).astype(np.int32)
    vc, _n, _d = cells(v, cell)
    by_cell = np.argsort(vc, kind="stable")
    by_cell = by_cell[vc[by_cell] >= 0]
    by_cell = by_cell[by_cell >= 16]
    for i in range(0, 600):              # neighbours in cell order: inside one cell, across two, and repeats of the same three cells
        j = r.integers(0, len(by_cell) - 6)
        t[i] = by_cell[j + r.permutation(6)[:3]]
    src = r.integers(600, 1500, 500)      # copies in all rotations and both windings
    for n, s in enumerate(src):
        a, b, c = t[s]
        t[1500 + n] = ((a, b, c), (b, c, a), (c, a, b), (a, c, b), (c, b, a), (b, a, c))[n % 6]
    bad = r.choice(np.arange(2000, nt), 240, replace=False)
    t[bad[:40], 0] = -1
    t[bad[40:80], 2] = nv
    t[bad[80:100], 1] = 2 ** 31 - 1
    t[bad[100:120], 1] = -2 ** 31
    t[bad[120:160], 1] = t[bad[120:160], 0]
    t[bad[160:200], 2] = t[bad[160:200], 0]
    t[bad[200:220], 0] = r.integers(5, 12, 20)
    t[bad[220:]] = (12, 13, 14)
    t[bad[230:]] = (14, 13, 12)
    assert 15 not in t
    return _frozen(v, col, t) + (cell, None)


@functools.lru_cache(None)
def crease():
    """A roof z = Z0 - SLOPE * |x - RIDGE| on a 41 x 41 grid of spacing H: 3200 triangles, column 22 exactly on the ridge, so every triangle
    lies in one of the two planes; every coordinate is dyadic, so the float32 vertices lie on the planes exactly.  Cells of 4 H; the ridge
    is 2 H from the cell faces in x and Z0 is 1.625 H above a face in z."""
    n = 41
    ix, iy = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    x, y = ix * CREASE_H, iy * CREASE_H
    z = CREASE_Z0 - CREASE_SLOPE * np.abs(x - CREASE_RIDGE)
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    assert (v.astype(f64) == np.stack([x, y, z], axis=-1).reshape(-1, 3)).all()
    i = (iy * n + ix)[:-1, :-1].reshape(-1)
    t = np.concatenate([np.stack([i, i + 1, i + n + 1], axis=1), np.stack([i, i + n + 1, i + n], axis=1)]).astype(np.int32)
    col = np.clip(v / 10.0, 0, 1).astype(np.float32)
    return _frozen(v, col, t) + (4 * CREASE_H, None)


CREASE_H, CREASE_SLOPE, CREASE_RIDGE, CREASE_Z0 = 0.25, 0.5, 5.5, 0.40625
# The mean of a straddling cell's vertices sits below the ridge: its columns are at x - RIDGE = -2 H, -H, 0, H, so the mean of |x - RIDGE|
# is H and z_mean = Z0 - SLOPE * H, at x_mean = RIDGE - H / 2.  The plane of the far side, extended to x_mean, is at Z0 + SLOPE * H / 2: a
# vertical gap of 1.5 SLOPE H, at least SLOPE * H, and a perpendicular one of at least SLOPE * H / sqrt(1 + SLOPE^2) = 0.1118 cells / 4.
CREASE_MEAN_OFF = CREASE_SLOPE * CREASE_H / math.sqrt(1.0 + CREASE_SLOPE ** 2)


def crease_planes():
    """(normal, offset) of the two planes: normal . p == offset"""
    return ((np.array([-CREASE_SLOPE, 0.0, 1.0]), CREASE_Z0 - CREASE_SLOPE * CREASE_RIDGE),
            (np.array([CREASE_SLOPE, 0.0, 1.0]), CREASE_Z0 + CREASE_SLOPE * CREASE_RIDGE))


CORNER = (2.5, 2.5, 2.5)


@functools.lru_cache(None)
def corner():
    """The outer corner of a box at CORNER: three faces x = 2.5, y = 2.5, z = 2.5, each a grid of spacing 0.25 over [0, 2.5]^2, sharing
    the vertices of their common edges; 600 triangles; cells of 1, so the corner is in the middle of cell (2, 2, 2)."""
    h, n = 0.25, 11
    ids, verts, tris = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(verts)
            verts.append(p)
        return ids[p]
    for axis in range(3):
        for a in range(n - 1):
            for b in range(n - 1):
                quad = []
                for da, db in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    p = [0.0, 0.0, 0.0]
                    p[axis] = CORNER[axis]
                    p[(axis + 1) % 3] = (a + da) * h
                    p[(axis + 2) % 3] = (b + db) * h
                    quad.append(vid(tuple(p)))
                tris.append((quad[0], quad[1], quad[2]))
                tris.append((quad[0], quad[2], quad[3]))
    v = np.array(verts, np.float32)
    t = np.array(tris, np.int32)
    col = np.clip(v / 2.5, 0, 1).astype(np.float32)
    return _frozen(v, col, t) + (1.0, None)


def empty():
    return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0, None


def no_triangles():
    """vertices without a triangle: cells are counted, nothing is used"""
    v, t, col = MC.sphere_mesh()
    return v, col, t[:0], 2.0, None


CASES = {
    "sphere_2": lambda: sphere(2.0),
    "sphere_3": lambda: sphere(3.0),
    "sphere_shifted": lambda: sphere(2.0, (0.3, -0.7, 0.11)),
    "identity": identity,
    "one_cell": one_cell,
    "hostile": hostile,
    "crease": crease,
    "corner": corner,
    "empty": empty,
    "no_triangles": no_triangles,
}
PLACE_CASES = ("sphere_2", "sphere_3", "sphere_shifted", "hostile", "crease", "corner")


@functools.lru_cache(None)
def expected(name, placement=PLACE_QUADRIC):
    """the restatement's answer for a case, computed once and shared (treat as read-only)"""
    v, col, t, cell, origin = CASES[name]()
    return simplify(v, col, t, cell, origin, placement)
