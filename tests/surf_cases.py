"""The yardstick of libsta_surf.so: a numpy restatement of include/sta_surf.h - components by iterated minimum propagation to a fixed
point, the weights and their prefix in the header's order (every floating-point operation is one numpy float64 operation, so nothing is
contracted), splitmix64 in uint64 and the stratified sampler -, the restated arithmetic of evaluate.eval_mesh and surface.clean_mesh, and
the case builders of tests/test_surf_cpu.py and tests/test_surf_gpu.py.  Host-only importable.

It is NOT Open3D's cluster_connected_triangles (adjacency is by shared vertex, not by shared edge) and not trimesh's sampler: neither was
available to compare against - DESIGN.md section 9."""
import functools

import numpy as np

import mesh_cases as MC

CHUNK = 1024
STATUS_BOUND = 1
PLAN_SIZES = 3
GOLDEN = 0x9E3779B97F4A7C15
MIX_1 = 0xBF58476D1CE4E5B9
MIX_2 = 0x94D049BB133111EB
KNOWN_ANSWERS = {1: 0xE220A8397B1DCDAF, 2: 0x6E789E6AA1B965F4, 3: 0x06C45D188009454F}      # seed 0
f64 = np.float64


def _r256(n):
    return (n + 255) // 256 * 256


def plan(nt, nv, ns=0):
    """sta_surf_plan: (bytes of the components' work, of the weights' work, 0); its refusals as ValueError."""
    for name, n in (("nt", nt), ("nv", nv), ("ns", ns)):
        if not 0 <= n < 2 ** 31:
            raise ValueError(f"surf_plan: {name} must be in [0, 2^31) (got {n})")
    return _r256(4 * nv), 2 * _r256(8 * ((nt + CHUNK - 1) // CHUNK)), 0


def valid(tris, nv):
    tris = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    return ((tris >= 0) & (tris < nv)).all(axis=1)


# ------------------------------------------------------------------------------------------ components
def components(tris, nv):
    """sta_surf_components -> (vlabel [nv], tlabel [nt], tcount [nv]) int32.  Every vertex starts with its own index; each round gives
    the three vertices of every valid triangle the smallest of their labels, then every vertex the label of its label (both only ever
    lower a label, to the index of a vertex of the same component); the fixed point is the component's smallest index."""
    tris = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    ok = valid(tris, nv)
    tv = tris[ok].astype(np.int64)
    lab = np.arange(nv, dtype=np.int64)
    while True:
        new = lab.copy()
        if len(tv):
            m = lab[tv].min(axis=1)
            for k in range(3):
                np.minimum.at(new, tv[:, k], m)
        new = np.minimum(new, new[new])
        if np.array_equal(new, lab):
            break
        lab = new
    named = np.zeros(nv, dtype=bool)
    named[tv.reshape(-1)] = True
    vlabel = np.where(named, lab, -1).astype(np.int32)
    tlabel = np.full(len(tris), -1, dtype=np.int32)
    tlabel[ok] = lab[tv[:, 0]]
    tcount = np.bincount(tlabel[ok], minlength=nv).astype(np.int32)
    return vlabel, tlabel, tcount


def clean_keep(tlabel, tcount, min_triangles=None, keep_largest=None):
    """surface.clean_mesh's mask: the triangles of the components with at least min_triangles triangles and, of those, the keep_largest
    with the most (among equal counts the lower root wins)."""
    tcount = np.asarray(tcount, dtype=np.int64)
    roots = [r for r in np.nonzero(tcount > 0)[0] if min_triangles is None or tcount[r] >= min_triangles]
    if keep_largest is not None:
        roots = sorted(roots, key=lambda r: (-tcount[r], r))[:keep_largest]
    return np.isin(tlabel, np.asarray(roots, dtype=np.int64)) & (np.asarray(tlabel) >= 0)


def cull_mesh(v, col, t, keep):
    """tsdf.cull_mesh: the kept triangles and the vertices they name, re-indexed in ascending order"""
    used = np.unique(t[keep])
    return v[used], (col[used] if col is not None else None), np.searchsorted(used, t[keep]).astype(np.int32)


# ------------------------------------------------------------------------------------------ weights and prefix
def face(verts, tris):
    """per triangle (rows of valid indices): A, B, C [n,3] float64, n [n,3], |n| [n], as include/sta_mesh.h writes them"""
    V = np.asarray(verts, dtype=np.float32).astype(f64)
    A, B, Cc = V[tris[:, 0]], V[tris[:, 1]], V[tris[:, 2]]
    with np.errstate(all="ignore"):
        u, w = B - A, Cc - A
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return A, B, Cc, n, ln


def tri_weights(verts, tris, keep=None):
    """w [nt] float64: |n|, 0 for a triangle that is not valid, not kept, or whose |n| is not finite"""
    tris = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    nv = len(np.asarray(verts).reshape(-1, 3))
    ok = valid(tris, nv)
    if keep is not None:
        ok = ok & (np.asarray(keep).astype(np.uint8) != 0)
    w = np.zeros(len(tris))
    ln = face(verts, tris[ok])[4]
    w[ok] = np.where(np.isfinite(ln), ln, 0.0)
    return w


def prefix(w):
    """(P [nt], total): chunks of 1024, sequential inside a chunk (np.add.accumulate adds in ascending order), the chunk sums sequential
    again; tests/test_surf_cpu.py holds it against a plain Python loop"""
    nt = len(w)
    nch = (nt + CHUNK - 1) // CHUNK
    pad = np.zeros(nch * CHUNK)
    pad[:nt] = w
    I = np.add.accumulate(pad.reshape(nch, CHUNK), axis=1)
    S = I[:, -1] if nch else np.zeros(0)
    O = np.concatenate([[0.0], np.add.accumulate(S)])        # 0 + S[0] == S[0] exactly
    P = (O[:nch, None] + I).reshape(-1)[:nt]
    return P, f64(O[nch])


def prefix_loop(w):
    """the same order as a plain Python loop"""
    nt = len(w)
    nch = (nt + CHUNK - 1) // CHUNK
    I, S = [0.0] * nt, []
    for c in range(nch):
        acc = 0.0
        for j in range(CHUNK):
            t = c * CHUNK + j
            acc = acc + (float(w[t]) if t < nt else 0.0)
            if t < nt:
                I[t] = acc
        S.append(acc)
    O = [0.0]
    for c in range(nch):
        O.append(O[c] + S[c])
    return np.array([O[t // CHUNK] + I[t] for t in range(nt)], dtype=f64), f64(O[nch])


# ------------------------------------------------------------------------------------------ the generator and the sampler
def mix_int(seed, i):
    """splitmix64 in Python integers"""
    M = (1 << 64) - 1
    z = (seed + i * GOLDEN) & M
    z = ((z ^ (z >> 30)) * MIX_1) & M
    z = ((z ^ (z >> 27)) * MIX_2) & M
    return z ^ (z >> 31)


def mix(seed, i):
    """splitmix64 in numpy uint64 (wrapping)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed % (1 << 64)) + np.asarray(i, dtype=np.uint64) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX_1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX_2)
        return z ^ (z >> np.uint64(31))


def units(seed, ns):
    """u [ns,3] float64 in [0, 1): u_j of sample k from the counter 3 k + j + 1"""
    k = np.arange(ns, dtype=np.uint64)
    return np.stack([(mix(seed, np.uint64(3) * k + np.uint64(j + 1)) >> np.uint64(11)).astype(f64) * f64(2.0 ** -53) for j in range(3)], axis=1)


def choose(P, total, ns, u0):
    """tri [ns] int64: the smallest t with P[t] > x, else the smallest with P[t] >= total; -1 everywhere unless total > 0 and finite"""
    if not (total > 0 and np.isfinite(total)):
        return np.full(ns, -1, dtype=np.int64)
    x = ((np.arange(ns, dtype=f64) + u0) / f64(ns)) * f64(total)
    t = np.searchsorted(P, x, side="right")
    t = np.where(t >= len(P), np.searchsorted(P, total, side="left"), t)
    return np.where(t >= len(P), -1, t).astype(np.int64)


def barycentric(u):
    with np.errstate(all="ignore"):
        r = np.sqrt(u[:, 1])
        return 1.0 - r, r * (1.0 - u[:, 2]), r * u[:, 2]


def sample(verts, tris, ns, seed=0, keep=None, colors=None, normals=False):
    """sta_surf_weights + sta_surf_sample -> {"points" [ns,3] f32, "tri" [ns] int32, "colors", "normals" ([ns,3] f32 or None), "P", "total",
    "w", "b" (the barycentric weights [ns,3])}"""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    w = tri_weights(verts, tris, keep)
    P, total = prefix(w)
    u = units(seed, ns)
    t = choose(P, total, ns, u[:, 0])
    if ns and len(tris):                    # a chosen triangle that is not valid cannot happen with the P of the same mesh
        t = np.where((t >= 0) & valid(tris[np.maximum(t, 0)], len(verts)), t, -1)
    hit = t >= 0
    b0, b1, b2 = barycentric(u)
    pts = np.full((ns, 3), np.nan)
    cols = np.full((ns, 3), np.nan) if colors is not None else None
    nrm = np.full((ns, 3), np.nan) if normals else None
    if hit.any():
        A, B, Cc, n, ln = face(verts, tris[t[hit]])
        h0, h1, h2 = b0[hit, None], b1[hit, None], b2[hit, None]
        pts[hit] = (h0 * A + h1 * B) + h2 * Cc
        if colors is not None:
            c = np.asarray(colors, dtype=np.float32).astype(f64)
            ca, cb, cc = c[tris[t[hit], 0]], c[tris[t[hit], 1]], c[tris[t[hit], 2]]
            cols[hit] = (h0 * ca + h1 * cb) + h2 * cc
        if normals:
            with np.errstate(all="ignore"):
                nrm[hit] = n / ln[:, None]
    f32 = lambda a: None if a is None else a.astype(np.float32)
    return {"points": f32(pts), "tri": t.astype(np.int32), "colors": f32(cols), "normals": f32(nrm), "P": P, "total": total, "w": w,
            "b": np.stack([b0, b1, b2], axis=1)}


# ------------------------------------------------------------------------------------------ evaluate.eval_mesh, restated
def eval_points(est_pts, gt_pts, threshold=0.05, max_error=0.5, nn=None):
    """the arithmetic of evaluate.eval_mesh on two sample sets, with cloud_cases.nn_brute: clipped distances sqrt(min(d2, max_error^2))"""
    import cloud_cases as CC
    nn = CC.nn_brute if nn is None else nn
    r2 = float(max_error) * float(max_error)
    d_est = np.sqrt(np.minimum(nn(gt_pts, est_pts, None, max_error)[0], r2))
    d_gt = np.sqrt(np.minimum(nn(est_pts, gt_pts, None, max_error)[0], r2))
    acc, comp = float(d_est.sum() / len(d_est)), float(d_gt.sum() / len(d_gt))
    n_precise, n_complete = int((d_est <= threshold).sum()), int((d_gt <= threshold).sum())
    p, r = n_precise / len(d_est), n_complete / len(d_gt)
    return {"accuracy": acc, "completion": comp, "completion_ratio": r, "precision": p, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0,
            "chamfer": (acc + comp) / 2.0, "n_precise": n_precise, "n_complete": n_complete, "d_est": d_est, "d_gt": d_gt}


# ------------------------------------------------------------------------------------------ meshes
def sphere():
    """mesh_cases.sphere_mesh(): 1064 vertices, 2124 triangles, closed -> (verts, tris, colours)"""
    return MC.sphere_mesh()


def sphere_radii():
    """(the smallest distance from the centre to a triangle's plane, the largest distance from the centre to a vertex): every point of
    every triangle lies between the two (a point of a triangle is at least as far from the centre as its plane, and a convex combination
    of the vertices is at most as far as the farthest of them).  Derived from the mesh, not fitted."""
    v, t, _ = sphere()
    A, _B, _C, n, ln = face(v, t)
    plane = np.abs(((A - MC.SPHERE_CENTRE) * n).sum(axis=1)) / ln
    return float(plane.min()), float(np.linalg.norm(v.astype(f64) - MC.SPHERE_CENTRE, axis=1).max())


@functools.lru_cache(None)
def hostile():
    """3073 triangles (3 chunks and one) on 600 vertices: coordinates over 16 decades of scale (so weights from 1e-16 to 1e16 and prefix
    sums that absorb the small ones), triangles with an index of -1 or nv, with repeated indices (zero area), an infinite and a NaN vertex"""
    r = np.random.default_rng(29)
    nv, nt = 600, 3 * CHUNK + 1
    scale = 10.0 ** r.integers(-8, 9, nv)
    v = (r.standard_normal((nv, 3)) * scale[:, None]).astype(np.float32)
    v[17] = np.inf
    v[18, 1] = np.nan
    t = r.integers(0, nv, (nt, 3)).astype(np.int32)
    # runs of small triangles among similar scales, so that small weights meet large prefixes
    order = np.argsort(scale, kind="stable")
    for i in range(0, nt, 7):
        t[i] = order[r.integers(0, 40)], order[r.integers(0, 40)], order[r.integers(0, 40)]
    bad = r.choice(nt, 200, replace=False)
    t[bad[:50], 0] = -1
    t[bad[50:100], 2] = nv
    t[bad[100:150], 1] = t[bad[100:150], 0]
    t[bad[150:], 2] = t[bad[150:], 0]
    for a in (v, t):
        a.setflags(write=False)
    return v, t


def three_spheres(seed=5):
    """three copies of the sphere, far apart, under a random permutation of the vertex ids and of the triangles -> (verts, tris)"""
    v, t, _ = sphere()
    r = np.random.default_rng(seed)
    nv = len(v)
    V = np.concatenate([v + np.float32(20.0 * k) for k in range(3)])
    T = np.concatenate([t + nv * k for k in range(3)])
    perm = r.permutation(3 * nv)                      # old id -> new id
    V2 = np.empty_like(V)
    V2[perm] = V
    return V2, perm[T].astype(np.int32)[r.permutation(len(T))]


def strip(n=65536):
    """a triangle strip whose vertex ids DESCEND along the strip: triangle k names n-1-k, n-2-k, n-3-k - the longest parent chains a mesh
    of this size can make"""
    k = np.arange(n - 2)
    return np.stack([n - 1 - k, n - 2 - k, n - 3 - k], axis=1).astype(np.int32), n


def fan(n=4096):
    """n triangles around the LAST vertex: every uniting meets on one word"""
    nv = n + 2
    k = np.arange(n)
    return np.stack([np.full(n, nv - 1), k, k + 1], axis=1).astype(np.int32), nv


def soup(nt=30000, nv=20000, seed=11):
    """uniformly random triangles: 4.5 corners per vertex, so one giant component next to the vertices nobody names"""
    return np.random.default_rng(seed).integers(0, nv, (nt, 3)).astype(np.int32), nv


def islands(nt=12000, nv=20000, seed=12):
    """random triangles whose three indices lie within 4 of each other: thousands of components of every small size"""
    r = np.random.default_rng(seed)
    return np.clip(r.integers(0, nv, (nt, 1)) + r.integers(0, 4, (nt, 3)), 0, nv - 1).astype(np.int32), nv


def odd():
    """bad indices (-1 and nv), repeated indices, duplicate triangles, a triangle (v, v, v), vertices nobody names"""
    nv = 14
    t = np.array([[0, 1, 2], [2, 1, 0], [0, 1, 2], [3, 3, 4], [5, 5, 5], [-1, 6, 7], [6, 7, nv], [6, 6, nv], [9, 8, 9], [8, 10, 10], [12, 11, 4], [13, 13, -1]],
                 dtype=np.int32)
    return t, nv


COMPONENT_CASES = {
    "empty": lambda: (np.zeros((0, 3), np.int32), 5),
    "no_vertices": lambda: (np.array([[0, 1, 2]], np.int32), 0),
    "one": lambda: (np.array([[2, 0, 1]], np.int32), 3),
    "odd": odd,
    "three_spheres": lambda: (three_spheres()[1], 3 * 1064),
    "strip_65536": strip,
    "fan_4096": fan,
    "soup": soup,
    "islands": islands,
}


def flat_mesh():
    """an all-zero mesh: every weight is 0"""
    return np.zeros((5, 3), np.float32), np.array([[0, 1, 2], [2, 3, 4]], np.int32)


def prefix_mesh(nt, seed=3):
    """nt random triangles on 64 vertices, a tenth of them with a repeated index (weight 0)"""
    r = np.random.default_rng(seed + nt)
    v = r.standard_normal((64, 3)).astype(np.float32)
    t = r.integers(0, 64, (nt, 3)).astype(np.int32)
    z = r.random(nt) < 0.1
    t[z, 1] = t[z, 0]
    return v, t


PREFIX_SIZES = (1, 1023, 1024, 1025, 3 * CHUNK + 1)
SAMPLE_SIZES = (0, 1, 7, 4096, 100001)
SEEDS = (0, 2 ** 63 + 5)
