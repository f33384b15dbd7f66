"""include/sta_reg.h restated in numpy, and vista_slam_amd/meshdist.py's plane_step and icp on top of it: the moved query in float64, the
search of tests/dist_cases.py on it (its classes, keys, corners and Index are used as they are; its `closest` rounds the query to float32
on entry, so the seven rules stand here once more on three doubles and tests/test_reg_cpu.py holds the two against each other bit for bit
wherever the query IS a float32), the plane of the winner, the residual, the Jacobian row, the 50 terms of the record and the loop.
Every numpy operation below is one IEEE operation per element, in the header's order.  The GPU tests compare the per-query outputs with
array_equal, the record with array_equal where every sum is exact and within TOL_REG_SUM elsewhere.

It is not Open3D's registration_icp: that is not available."""
import functools

import numpy as np

import cloud_cases as CC
import dist_cases as DC
import surf_cases as SF

f64 = np.float64
RECORD = 64
USED = 50
PLAN_SIZES = 2
FANOUT, MAX_LEVELS, N_VALID, STATUS_BOUND = DC.FANOUT, DC.MAX_LEVELS, 0, 1
ORDERS = CC.ORDERS
TRIU = np.triu_indices(6)

# Tolerances that are not array_equal, measured on this restatement alone (tests/test_reg_cpu.py measures them again, prints them and
# asserts that they are not above the *_MEASURED constants, which are the measured figures rounded up to two digits):
#   TOL_REG_SUM   an entry of the record on the hostile case (hostile_case(): triangles and queries over 18 decades, a similarity of
#                 scale 1.7), relative to sum_i |term_i| of that entry: the largest spread between the ascending, reversed and pairwise
#                 sums.  Measured 1.96e-15; times 16 because the GPU's fixed tree is a further order.
#   TOL_REG_ICP   absolute, on the entries of the final transform of the restated ICP on the two recovery cases, both modes, under the
#                 three orders (whose iteration counts and statuses are identical: the CPU test asserts it).  Measured: room plane
#                 6.9e-17, point 1.1e-14; spheres (coordinates up to 41, so a lever of that length) plane 3.8e-15, point 5.2e-13;
#                 times 16 likewise.
#   RECOVERY      the final error max |T o M - I| of the restated ICP (ascending order, RECOVERY_MAX_ITER updates at the most) on the
#                 recovery cases, per (case, mode): what is left of a known motion M of the noise-free samples, whose initial error is
#                 0.04 and more.  The tests assert 16 times these.  Iterations plane / point: room 4 / 100 (the closest-point mode
#                 slides along the one large wall and has not converged after 100 updates), spheres 4 / 22.
TOL_REG_SUM_MEASURED = 2.0e-15
TOL_REG_SUM = 16 * TOL_REG_SUM_MEASURED
TOL_REG_ICP_MEASURED = 5.2e-13
TOL_REG_ICP = 16 * TOL_REG_ICP_MEASURED
RECOVERY_MEASURED = {("spheres", "plane"): 2.4e-7, ("spheres", "point"): 6.0e-4, ("room", "plane"): 5.7e-9, ("room", "point"): 4.5e-3}
RECOVERY_FACTOR = 16.0


def plan(nt, Q=1):
    """(nodes, work_bytes) of sta_reg_plan, its refusals as ValueError with the library's words"""
    nt, Q = int(nt), int(Q)
    if not 1 <= nt < 1 << 27:
        raise ValueError(f"reg_plan: nt must be in [1, 2^27) (got {nt})")
    if not 1 <= Q < 1 << 30:
        raise ValueError(f"reg_plan: Q must be in [1, 2^30) (got {Q})")
    return sum(DC.level_counts(nt)), ((Q + 255) // 256 * RECORD * 8 + 255) & ~255


# ------------------------------------------------------------------------------------------ the search on doubles
def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest(q, A, B, Cc):
    """dist_cases.closest with the query taken as float64 as it stands (A, B, C are float32 values): the clamped closest point and d2"""
    q = np.asarray(q, dtype=f64)
    a, b, c = (np.asarray(x, dtype=np.float32).astype(f64) for x in (A, B, Cc))
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
            p = np.where(cond[..., None], np.broadcast_to(val, p.shape), p)
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        r = np.where(p >= lo, p, np.broadcast_to(lo, p.shape))
        r = np.where(r <= hi, r, np.broadcast_to(hi, p.shape))
        d = q - r
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return r, dd


def search(index, q, radius=np.inf, chunk=256):
    """(d2 [Q] float64, tri [Q] int32, c [Q,3] float64) of the float64 queries q: the minimum over ALL valid triangles of `index` (a
    dist_cases.Index) that qualify, the lowest input index among equal d2; +inf, -1, NaN otherwise.  A triangle whose own box is farther
    than the radius is not scored: its computed bound is <= its computed d2 (the argument of the header), so it cannot qualify."""
    q = np.asarray(q, dtype=f64).reshape(-1, 3)
    Q = len(q)
    d2o, trio, co = np.full(Q, np.inf), np.full(Q, -1, dtype=np.int32), np.full((Q, 3), np.nan)
    ids = np.nonzero(index.cls == DC.VALID)[0]          # ascending
    if not len(ids):
        return d2o, trio, co
    P = DC.corners(index.verts, index.tris[ids])
    lo, hi = P.min(axis=1).astype(f64), P.max(axis=1).astype(f64)
    with np.errstate(all="ignore"):
        r2 = f64(radius) * f64(radius)
    rows = np.nonzero(np.isfinite(q).all(axis=1))[0]
    rows = rows[np.argsort(q[rows, 0], kind="stable")]          # slabs along x: a chunk's queries are near each other
    for s in range(0, len(rows), chunk):
        rr = rows[s:s + chunk]
        qq = q[rr]
        near = np.arange(len(ids))
        if np.isfinite(r2):
            # a triangle whose box is farther than the radius (and a margin) from the chunk's box on an axis has e_k > radius for every
            # query of the chunk: it cannot qualify
            reach = float(radius) * (1.0 + 1e-9) + 1e-300
            near = np.nonzero(((lo <= qq.max(axis=0) + reach) & (hi >= qq.min(axis=0) - reach)).all(axis=1))[0]
            if not len(near):
                continue
        with np.errstate(all="ignore"):
            e = [np.maximum(np.maximum(lo[None, near, k] - qq[:, None, k], qq[:, None, k] - hi[None, near, k]), 0.0) for k in range(3)]
            bound = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        qi, tj = np.nonzero(bound <= r2)
        if not len(qi):
            continue
        tj = near[tj]          # (ascending with near: the order among equals is the index order)
        c, dd = closest(qq[qi], P[tj, 0], P[tj, 1], P[tj, 2])
        ok = dd <= r2
        qi, tj, c, dd = qi[ok], tj[ok], c[ok], dd[ok]
        if not len(qi):
            continue
        head = np.concatenate([[True], qi[1:] != qi[:-1]])
        mins = np.minimum.reduceat(dd, np.flatnonzero(head))
        k = np.flatnonzero(dd == mins[np.cumsum(head) - 1])
        uq, first = np.unique(qi[k], return_index=True)          # qi ascending, tj ascending inside: the first is the lowest index
        sel = k[first]
        d2o[rr[uq]], trio[rr[uq]], co[rr[uq]] = dd[sel], ids[tj[sel]], c[sel]
    return d2o, trio, co


# ------------------------------------------------------------------------------------------ one pass
def pass_(index, qry, T=None, radius=np.inf, qnrm=None, min_cos=0.0, pivot=None):
    """Rules 1 to 6 of the header -> dict(q [Q,3] float64, d2, tri, point [Q,3] float32, resid, c, nhat, J [Q,6], finite, found, rejected,
    matched [Q] bool, terms [Q,64] float64: what each query adds to the record)."""
    qry = np.asarray(qry, dtype=np.float32).reshape(-1, 3)
    Q = len(qry)
    q = CC.apply_T(qry, T)
    Tm = np.eye(4)[:3] if T is None else np.asarray(T, dtype=f64)[:3]
    pivot = np.zeros(3) if pivot is None else np.asarray(pivot, dtype=f64).reshape(3)
    finite = np.isfinite(q).all(axis=1)
    d2, tri, c = search(index, q, radius)
    found = tri >= 0
    with np.errstate(all="ignore"):
        r2 = f64(radius) * f64(radius)
        valid = np.nonzero(index.cls == DC.VALID)[0]
        if len(valid):          # (a query without a triangle reads some valid one: its values are dropped)
            P = DC.corners(index.verts, index.tris[np.where(found, tri, valid[0])]).astype(f64)
        else:
            P = np.full((Q, 3, 3), np.nan)
        u, v = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        w = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        nhat = n / w[:, None]
        r = dot(q - c, nhat)
        x = q - pivot
        J = np.stack([x[:, 1] * nhat[:, 2] - x[:, 2] * nhat[:, 1], x[:, 2] * nhat[:, 0] - x[:, 0] * nhat[:, 2], x[:, 0] * nhat[:, 1] - x[:, 1] * nhat[:, 0],
                      nhat[:, 0], nhat[:, 1], nhat[:, 2]], axis=1)
        rejected = np.zeros(Q, bool)
        if qnrm is not None:
            nq = np.asarray(qnrm, dtype=np.float32).reshape(-1, 3).astype(f64)
            m = np.stack([(Tm[a, 0] * nq[:, 0] + Tm[a, 1] * nq[:, 1]) + Tm[a, 2] * nq[:, 2] for a in range(3)], axis=1)
            rejected = found & (dot(m, nhat) < f64(min_cos) * np.sqrt(dot(m, m)))
    matched = found & ~rejected
    terms = np.zeros((Q, RECORD))
    terms[finite, 0] = 1.0
    terms[matched, 1] = 1.0
    terms[matched, 2] = d2[matched]
    terms[finite, 3] = np.where(matched[finite], d2[finite], r2)
    M = matched
    with np.errstate(all="ignore"):
        for a in range(3):
            terms[M, 4 + a] = q[M, a]
            terms[M, 7 + a] = c[M, a]
            for b in range(3):
                terms[M, 10 + 3 * a + b] = q[M, a] * c[M, b]
        terms[~finite, 19] = 1.0
        terms[rejected, 20] = 1.0
        terms[M, 21] = r[M] * r[M]
        terms[M, 22] = np.abs(r[M])
        for a in range(6):
            terms[M, 23 + a] = J[M, a] * r[M]
        for k, (a, b) in enumerate(zip(*TRIU)):
            terms[M, 29 + k] = J[M, a] * J[M, b]
    nan = np.float32(np.nan)
    return dict(q=q, d2=d2, tri=tri, point=np.where(found[:, None], c, nan).astype(np.float32), resid=np.where(found, r, np.nan), c=c, nhat=nhat, J=J,
                finite=finite, found=found, rejected=rejected, matched=matched, terms=terms)


def record(terms, order="asc"):
    return CC.sum_rows(terms, order) if len(terms) else np.zeros(RECORD)


def H_of(rec):
    H = np.zeros((6, 6))
    H[TRIU] = rec[29:50]
    return H + np.triu(H, 1).T


# ------------------------------------------------------------------------------------------ the steps and the loop
def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    w = np.asarray(w, dtype=f64).reshape(3)
    t = float(np.sqrt(w @ w))
    K = skew(w)
    a, b = (1.0 - t * t / 6.0, 0.5 - t * t / 24.0) if t < 1e-8 else (np.sin(t) / t, (1.0 - np.cos(t)) / (t * t))
    return np.eye(3) + a * K + b * (K @ K)


def twist_update(omega, v, pivot):
    """the 3x4 matrix of x -> Exp(omega)(x - pivot) + pivot + v"""
    R, pivot = exp_so3(omega), np.asarray(pivot, dtype=f64)
    return np.concatenate([R, (pivot - R @ pivot + np.asarray(v, dtype=f64))[:, None]], axis=1)


def plane_step(rec, pivot, sv_ratio=1e-9):
    lam, V = np.linalg.eigh(H_of(rec))
    keep = lam > sv_ratio * lam[-1] if lam[-1] > 0.0 else np.zeros(6, bool)
    coef = np.where(keep, (V.T @ -rec[23:29]) / np.where(keep, lam, 1.0), 0.0)
    delta = V @ coef
    return twist_update(delta[:3], delta[3:], pivot)


def icp(source, index, max_corr, init=None, mode="plane", normals=None, min_cos=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, order="asc"):
    """meshdist.icp restated -> dict(T [4,4], fitness, inlier_rmse, iterations, status, records = the record of every evaluation)"""
    source = np.asarray(source, dtype=np.float32).reshape(-1, 3)
    T = np.eye(4)[:3] if init is None else np.asarray(init, dtype=f64)[:3].copy()
    Q, need = len(source), 6 if mode == "plane" else 3
    fin = np.isfinite(source).all(axis=1)
    centre = source[fin].astype(f64).mean(axis=0) if mode == "plane" and fin.any() else np.zeros(3)
    if normals is not None and min_cos is None:
        min_cos = 0.0
    records = []

    def evaluate(T):
        pivot = T[:, :3] @ centre + T[:, 3]
        rec = record(pass_(index, source, T, max_corr, normals, min_cos if normals is not None else 0.0, pivot)["terms"], order)
        records.append(rec)
        return rec, rec[1] / Q, (np.sqrt(rec[2] / rec[1]) if rec[1] else 0.0), pivot
    rec, fit, rmse, pivot = evaluate(T)
    status, it = "max_iter", 0
    while it < max_iter:
        if rec[1] < need:
            status = "too_few_matches"
            break
        T = CC.compose(plane_step(rec, pivot) if mode == "plane" else CC.kabsch(rec), T)
        it += 1
        rec, f2, r2, pivot = evaluate(T)
        done = abs(f2 - fit) < rel_fitness and abs(r2 - rmse) < rel_rmse
        fit, rmse = f2, r2
        if done:
            status = "converged"
            break
    if rec[1] < need and status == "max_iter":
        status = "too_few_matches"
    return dict(T=np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]], axis=0), fitness=float(fit), inlier_rmse=float(rmse), iterations=it, status=status,
                records=records)


# ------------------------------------------------------------------------------------------ cases
def similarity():
    """a general similarity of scale 1.7 (cloud_cases' scaled_T)"""
    return np.concatenate([1.7 * CC.rotation((0.3, -1.0, 0.5), 11.0), np.array([[0.4], [-0.2], [0.1]])], axis=1)


TRANSFORMS = {
    "identity": lambda: None,
    "dyadic_translation": lambda: np.concatenate([np.eye(3), np.array([[0.25], [-0.5], [0.125]])], axis=1),
    "rotation": lambda: np.concatenate([CC.rotation((1.0, 2.0, 3.0), 17.0), np.array([[0.03], [-0.01], [0.02]])], axis=1),
    "similarity": similarity,
}


def poisoned(q):
    """queries with NaN and inf mixed in"""
    q = np.array(q, dtype=np.float32)
    q[::5, 1] = np.nan
    q[1::9, 0] = np.inf
    q[2::11, 2] = -np.inf
    return q


def hostile_case():
    """(verts, tris, queries, T, radius): dist_cases' hostile soup and queries under the similarity: every sum rounds"""
    v, t = DC.hostile_soup()
    return v, t, DC.hostile_queries(), similarity(), np.inf


def dyadic_case():
    """(verts, tris, queries, T, pivot): dist_cases.lattice(4, 0.25) - axis-aligned, legs 0.25, so every w = 0.0625 is an exact square
    root and every nhat is (0, 0, 1) - with its lattice queries under a dyadic translation: every term and every sum is exact"""
    v, t = DC.lattice(4, 0.25)
    return v, t, DC.lattice_queries(4, 0.25), TRANSFORMS["dyadic_translation"](), np.array([0.5, 0.25, -0.125])


def surface_points(v, t, per_tri, seed):
    """per_tri noise-free points of every triangle: float64 barycentric combinations rounded to float32 once -> (points, triangle of each)"""
    r = np.random.default_rng(seed)
    P = DC.corners(v, t).astype(f64)
    b = r.dirichlet((1.0, 1.0, 1.0), (len(t), per_tri))
    pts = np.einsum("tkc,tcx->tkx", b, P).reshape(-1, 3).astype(np.float32)
    return pts, np.repeat(np.arange(len(t), dtype=np.int32), per_tri)


def face_normals(v, t, tri):
    """float32 unit normals of the triangles `tri` (float64 cross product, normalised, rounded once)"""
    P = DC.corners(v, np.asarray(t)[tri]).astype(f64)
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def small_motion(seed, centre, angle, axis=None, shift=0.04):
    """a rigid 3x4 motion: `angle` rad about `axis` (random when None) through `centre`, then `shift` units along a random direction"""
    r = np.random.default_rng(seed)
    w, tv = r.standard_normal(3), r.standard_normal(3)
    w = w if axis is None else np.asarray(axis, dtype=f64)
    return twist_update(angle * w / np.linalg.norm(w), shift * tv / np.linalg.norm(tv), centre)


MAX_CORR = 0.2
RECOVERY_MAX_ITER = 100          # the closest-point mode converges linearly: it needs more than the default 30 updates


@functools.lru_cache(None)
def recovery_case(name):
    """(verts, tris, source, M): noise-free samples of the mesh moved by the known small motion M (rounded to float32 once); ICP from the
    identity must return M^-1.  Both motions are within 0.05 rad and 0.05 units and turn about the centre of the samples, so that no
    sample starts farther than MAX_CORR from its surface.
    spheres: 400 samples by area of dist_cases.spheres_case()'s three spheres (surf_cases.sample), whose centres lie on one line 69 units
      long: 0.003 rad about an axis ACROSS that line (about the line itself a sphere turns in place, which closest points cannot see) and
      0.04 units.
    room: two points of every triangle of dist_cases.room() and 300 more by area, which land on its one large triangle: 0.02 rad about a
      random axis and 0.04 units."""
    if name == "spheres":
        v, t = DC.spheres_case()[:2]
        pts = SF.sample(v, t, 400, seed=3)["points"]
        M = small_motion(41, pts.astype(f64).mean(axis=0), 0.003, axis=(1.0, -1.0, 0.0))
    else:
        v, t = DC.room()
        pts = np.concatenate([surface_points(v, t, 2, 5)[0], SF.sample(v, t, 300, seed=6)["points"]])
        M = small_motion(42, pts.astype(f64).mean(axis=0), 0.02)
    src = CC.transform(pts, M)
    for a in (src, M):
        a.setflags(write=False)
    return v, t, src, M


@functools.lru_cache(None)
def recovery_answer(name, mode, order="asc"):
    """the restated ICP of a recovery case (computed once, read only)"""
    v, t, src, _M = recovery_case(name)
    return icp(src, index_of(name), MAX_CORR, mode=mode, max_iter=RECOVERY_MAX_ITER, order=order)


@functools.lru_cache(None)
def index_of(name):
    v, t = (DC.spheres_case()[:2] if name == "spheres" else DC.room())
    return DC.Index(v, t)


def motion_error(T, M):
    """max |T o M - I| over the twelve entries"""
    return float(np.abs(CC.compose(np.asarray(T)[:3], np.asarray(M)[:3]) - np.eye(4)[:3]).max())
