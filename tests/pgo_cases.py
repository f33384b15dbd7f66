"""The pose-graph contract of include/sta_mi355.h (sta_sim3_op / sta_pgo_index / sta_pgo_linearize / sta_pgo_solve / sta_pgo_optimize)
restated in numpy: the yardstick of csrc/pgo.h.  Every function is dtype-generic (float64 or np.longdouble: nothing here calls LAPACK),
batched over the leading axis, and follows the header's order of operations up to the order inside a sum.  Also the graph generators
of the tests.  It is NOT pypose: the stated differences are in the header.

A Sim(3) element is 8 numbers (tx,ty,tz, qx,qy,qz,qw, s) acting as x -> s R(q) x + t; a tangent is (tau, phi, sigma).
"""
import os

import numpy as np

# ---- the constants of the contract (the same names in csrc/pgo.h) ----
PHI_SERIES = 0.25        # |phi| below: W's A and B from the moment series (above: the closed forms)
MOMENT_START = 48        # the backward recurrence m_(k-1) = (e^sigma - sigma m_k) / k starts at m_48 = e^sigma / 49
MOMENT_TERMS = 6         # terms of the theta^2 series of A and B
QUAT_SERIES = 1e-4       # |phi| (Exp) or |q.xyz| (Log) below: the two-term series of sin(theta/2)/theta, 2 atan2(n, w)/n
JL_TERMS = 32            # Jl = I + ad/2 (I + ad/3 (... (I + ad/33))): Horner over 32 powers

ST_INDEX, ST_NONFINITE, ST_MAXITER, ST_BREAKDOWN, ST_CHOL, ST_UNCHANGED = 1, 2, 4, 8, 16, 32

# ---- the tolerances of tests/test_pgo_gpu.py, measured by tests/test_pgo_cpu.py (which fails if a rule below no longer gives them) ----
# TOL_EDGE: the larger of 1e-13 and 64 x the float64-versus-longdouble error of this restatement (relative to 1 + max|row|) over the
# inputs of the GPU tests: op_inputs() through every op, and r, S, v, g, the diagonal blocks and f of every graph of linearize_graphs().
# Measured 8.454e-14 (worst: g of slam_graph(12), whose v_e = M_e^T (w r) carries the error of r, 3.3e-15, times |M| |w|; every sim3 op
# stays below 8e-16), x 64 = 5.41e-12, rounded up to two digits.
TOL_EDGE = 5.5e-12
# TOL_LM: 10 x the spread of the float64 restatement between two edge orderings of the same graph (the edge list reversed, which
# reverses every node sum and the cost sum), on the final cost (relative to 1 + f) and on X_a^-1 X_b along every edge (as matrices,
# relative to 1 + max|row|), over lm_graphs() with LM_ARGS (below).  Measured 4.885e-15 (slam_graph(40),
# windowed), x 10 = 4.9e-14, rounded up to two digits.  It is this small because LM ends at a fixed point: each accepted step corrects the rounding of the one before.
TOL_LM = 4.9e-14

# the systems of the GPU solve test: name -> (radius, max_iter); test_pgo_cpu checks that the restatement's own PCG at rtol = 1e-10
# reaches a true relative residual <= 1e-9 on each.  The all-free triangle (gauge held by the damping alone, condition 2e5) needs 35
# iterations for its 21 unknowns, so it gets room above the default of 7 n.
SOLVE_SYSTEMS = {"chain2 one fixed": (1e4, None), "triangle": (1e4, 200), "slam12": (1e4, None), "slam120": (1e4, None)}


def _arr(x, dt):
    return np.asarray(x, dtype=dt)


def hat(v):
    o = np.zeros(v.shape[:-1] + (3, 3), v.dtype)
    o[..., 0, 1], o[..., 0, 2], o[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    o[..., 1, 2], o[..., 2, 0], o[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    return o


def rot(q):
    """R of a unit quaternion (x, y, z, w)."""
    x, y, z, w = (q[..., i] for i in range(4))
    R = np.empty(q.shape[:-1] + (3, 3), q.dtype)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R


def _norm_q(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def matrix(T):
    T = np.asarray(T)
    M = np.zeros(T.shape[:-1] + (4, 4), T.dtype)
    M[..., :3, :3] = T[..., 7, None, None] * rot(T[..., 3:7])
    M[..., :3, 3] = T[..., :3]
    M[..., 3, 3] = 1
    return M


def mul(a, b):
    a, b = np.asarray(a), np.asarray(b)
    o = np.empty(np.broadcast(a, b).shape, a.dtype)
    o[..., :3] = a[..., 7:8] * (rot(a[..., 3:7]) @ b[..., :3, None])[..., 0] + a[..., :3]
    x1, y1, z1, w1 = (a[..., i] for i in range(3, 7))
    x2, y2, z2, w2 = (b[..., i] for i in range(3, 7))
    q = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                  w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)
    o[..., 3:7] = _norm_q(q)
    o[..., 7] = a[..., 7] * b[..., 7]
    return o


def inv(a):
    a = np.asarray(a)
    o = np.empty_like(a)
    Rt = np.swapaxes(rot(a[..., 3:7]), -1, -2)
    o[..., :3] = -(Rt @ a[..., :3, None])[..., 0] / a[..., 7:8]
    o[..., 3:6] = -a[..., 3:6]
    o[..., 6] = a[..., 6]
    o[..., 3:7] = _norm_q(o[..., 3:7])
    o[..., 7] = 1 / a[..., 7]
    return o


def between(a, b):
    return mul(inv(a), b)


def w_coef(theta, sigma):
    """(A, B, C) of W(phi, sigma) = C I + A phi^ + B phi^ phi^."""
    dt = theta.dtype
    one = dt.type(1)
    with np.errstate(all="ignore"):
        es = np.exp(sigma)
        C = np.where(sigma != 0, np.expm1(sigma) / np.where(sigma != 0, sigma, one), one)
        # closed forms
        den = sigma * sigma + theta * theta
        Is = (es * (sigma * np.sin(theta) - theta * np.cos(theta)) + theta) / den
        Ic = (es * (sigma * np.cos(theta) + theta * np.sin(theta)) - sigma) / den
        Ac, Bc = Is / theta, (C - Ic) / (theta * theta)
    # the moment series
    m = [None] * (MOMENT_START + 1)
    m[MOMENT_START] = es / dt.type(MOMENT_START + 1)
    for k in range(MOMENT_START, 0, -1):
        m[k - 1] = (es - sigma * m[k]) / dt.type(k)
    t2 = theta * theta
    As, Bs, p, fa, fb = np.zeros_like(theta), np.zeros_like(theta), np.ones_like(theta), one, dt.type(2)
    for j in range(MOMENT_TERMS):
        As = As + p * m[2 * j + 1] / fa
        Bs = Bs + p * m[2 * j + 2] / fb
        p = -p * t2
        fa = fa * dt.type((2 * j + 2) * (2 * j + 3))
        fb = fb * dt.type((2 * j + 3) * (2 * j + 4))
    small = theta < dt.type(PHI_SERIES)
    return np.where(small, As, Ac), np.where(small, Bs, Bc), C


def _w_apply(phi, sigma, x):
    theta = np.sqrt((phi * phi).sum(-1))
    A, B, C = w_coef(theta, sigma)
    px = np.cross(phi, x)
    return C[..., None] * x + A[..., None] * px + B[..., None] * np.cross(phi, px)


def exp(xi):
    xi = np.asarray(xi)
    dt = xi.dtype
    tau, phi, sigma = xi[..., :3], xi[..., 3:6], xi[..., 6]
    theta = np.sqrt((phi * phi).sum(-1))
    with np.errstate(all="ignore"):
        k = np.where(theta < dt.type(QUAT_SERIES), dt.type(0.5) - theta * theta / dt.type(48), np.sin(theta / 2) / theta)
    o = np.empty(xi.shape[:-1] + (8,), dt)
    o[..., :3] = _w_apply(phi, sigma, tau)
    o[..., 3:6] = k[..., None] * phi
    o[..., 6] = np.cos(theta / 2)
    o[..., 3:7] = _norm_q(o[..., 3:7])
    o[..., 7] = np.exp(sigma)
    return o


def solve3(W, t):
    """W^-1 t by the adjugate."""
    a, b, c, d, e, f, g, h, i = (W[..., r, s] for r in range(3) for s in range(3))
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * c00 + b * c10 + c * c20
    x, y, z = t[..., 0], t[..., 1], t[..., 2]
    return np.stack([c00 * x + c01 * y + c02 * z, c10 * x + c11 * y + c12 * z, c20 * x + c21 * y + c22 * z], -1) / det[..., None]


def log(T):
    T = np.asarray(T)
    dt = T.dtype
    q = _norm_q(T[..., 3:7])
    q = np.where(q[..., 3:4] < 0, -q, q)
    v, w = q[..., :3], q[..., 3]
    n = np.sqrt((v * v).sum(-1))
    with np.errstate(all="ignore"):
        f = np.where(n < dt.type(QUAT_SERIES), (2 / w) * (1 - n * n / (3 * w * w)), 2 * np.arctan2(n, w) / n)
    phi = f[..., None] * v
    sigma = np.log(T[..., 7])
    theta = np.sqrt((phi * phi).sum(-1))
    A, B, C = w_coef(theta, sigma)
    P = hat(phi)
    W = C[..., None, None] * np.eye(3, dtype=dt) + A[..., None, None] * P + B[..., None, None] * (P @ P)
    o = np.empty(T.shape[:-1] + (7,), dt)
    o[..., :3] = solve3(W, T[..., :3])
    o[..., 3:6] = phi
    o[..., 6] = sigma
    return o


def retract(d, a, mask=None):
    o = mul(exp(d), a)
    if mask is not None:
        o = np.where(np.asarray(mask, bool)[..., None], o, a)
    return o


def Ad(T):
    T = np.asarray(T)
    R, t, s = rot(T[..., 3:7]), T[..., :3], T[..., 7]
    M = np.zeros(T.shape[:-1] + (7, 7), T.dtype)
    M[..., :3, :3] = s[..., None, None] * R
    M[..., :3, 3:6] = hat(t) @ R
    M[..., :3, 6] = -t
    M[..., 3:6, 3:6] = R
    M[..., 6, 6] = 1
    return M


def ad(xi):
    xi = np.asarray(xi)
    M = np.zeros(xi.shape[:-1] + (7, 7), xi.dtype)
    M[..., :3, :3] = xi[..., 6, None, None] * np.eye(3, dtype=xi.dtype) + hat(xi[..., 3:6])
    M[..., :3, 3:6] = hat(xi[..., :3])
    M[..., :3, 6] = -xi[..., :3]
    M[..., 3:6, 3:6] = hat(xi[..., 3:6])
    return M


def Jl(xi, terms=JL_TERMS):
    a = ad(xi)
    I = np.broadcast_to(np.eye(7, dtype=a.dtype), a.shape)
    Y = I.copy()
    for n in range(terms, 0, -1):
        Y = I + (a @ Y) / a.dtype.type(n + 1)
    return Y


def elim_solve(A, B):
    """A^-1 B, batched [N,m,m] x [N,m,k]: Gaussian elimination with partial pivoting (the first largest |entry| of the column)."""
    A, B = np.array(A), np.array(B)
    N, m = A.shape[0], A.shape[1]
    ar = np.arange(N)
    for c in range(m):
        p = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
        tmpA, tmpB = A[ar, p].copy(), B[ar, p].copy()
        A[ar, p], B[ar, p] = A[:, c], B[:, c]
        A[:, c], B[:, c] = tmpA, tmpB
        for r in range(c + 1, m):
            f = A[:, r, c] / A[:, c, c]
            A[:, r] = A[:, r] - f[:, None] * A[:, c]
            B[:, r] = B[:, r] - f[:, None] * B[:, c]
    X = np.empty_like(B)
    for r in range(m - 1, -1, -1):
        acc = B[:, r].copy()
        for c in range(r + 1, m):
            acc = acc - A[:, r, c, None] * X[:, c]
        X[:, r] = acc / A[:, r, r, None]
    return X


def chol7(A):
    """The lower Cholesky factor, batched [N,m,m] -> (L, ok [N])."""
    m = A.shape[1]
    L = np.zeros_like(A)
    ok = np.ones(A.shape[0], bool)
    with np.errstate(all="ignore"):
        for j in range(m):
            d = A[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(-1)
            ok &= d > 0
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, m):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(-1)) / L[:, j, j]
    return L, ok


def chol_solve(L, b):
    m = L.shape[1]
    y = np.zeros_like(b)
    for i in range(m):
        y[:, i] = (b[:, i] - (L[:, i, :i] * y[:, :i]).sum(-1)) / L[:, i, i]
    x = np.zeros_like(b)
    for i in range(m - 1, -1, -1):
        x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(-1)) / L[:, i, i]
    return x


# ---- the graph side ----
def opt_mask(n, opt_idx="all"):
    m = np.zeros(n, bool)
    if isinstance(opt_idx, str):
        m[:] = True
    else:
        m[np.asarray(opt_idx, np.int64)] = True
    return m


def active_edges(edges, opt, n):
    """-> (active [E], status): a != b, both in [0, n), at least one endpoint optimised; an out-of-range index sets ST_INDEX."""
    e = np.asarray(edges, np.int64)
    inr = ((e >= 0) & (e < n)).all(1)
    a, b = np.clip(e[:, 0], 0, n - 1), np.clip(e[:, 1], 0, n - 1)
    return inr & (a != b) & (opt[a] | opt[b]), (0 if inr.all() else ST_INDEX)


def index(edges, opt, n):
    """-> (off int32 [n+1], inc int32 [off[n]] = edge * 2 + side, ascending by edge within a node, status)."""
    act, status = active_edges(edges, opt, n)
    lists = [[] for _ in range(n)]
    for e in np.flatnonzero(act):
        for side in (0, 1):
            k = int(edges[e][side])
            if opt[k]:
                lists[k].append(2 * int(e) + side)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([h for l in lists for h in l], np.int32), status


def linearize(nodes, edges, poses, confs, opt, dtype=np.float64):
    """r [E,7], S [E,7,7], v [E,7], c [E] (zeros on inactive edges), f, g [n,7], blocks [n,7,7] (zeros on fixed nodes), status."""
    X, P, w = _arr(nodes, dtype), _arr(poses, dtype), _arr(confs, dtype)
    n, E = X.shape[0], P.shape[0]
    act, status = active_edges(edges, opt, n)
    e = np.asarray(edges, np.int64)
    a, b = np.where(act, e[:, 0], 0), np.where(act, e[:, 1], 0)
    with np.errstate(all="ignore"):
        Ae = mul(P, inv(X[a]))
        r = log(mul(Ae, X[b]))
        M = elim_solve(Jl(r), Ad(Ae))
        S = np.swapaxes(M, 1, 2) @ (w[:, :, None] * M)
        v = (np.swapaxes(M, 1, 2) @ (w * r)[:, :, None])[..., 0]
        c = (w * r * r).sum(-1)
    z = ~act
    r[z], S[z], v[z], c[z] = 0, 0, 0, 0
    f = c[act].sum() if act.any() else dtype(0)
    g, blocks = np.zeros((n, 7), dtype), np.zeros((n, 7, 7), dtype)
    off, inc, _ = index(edges, opt, n)
    for k in range(n):
        for h in inc[off[k]:off[k + 1]]:
            ed, side = h >> 1, h & 1
            g[k] += v[ed] if side else -v[ed]
            blocks[k] += S[ed]
    if not np.isfinite(f):
        status |= ST_NONFINITE
    return dict(act=act, a=a, b=b, r=r, S=S, v=v, c=c, f=f, g=g, blocks=blocks, off=off, inc=inc, opt=np.asarray(opt, bool), status=status, n=n)


def cost(nodes, edges, poses, confs, opt, dtype=np.float64):
    X, P, w = _arr(nodes, dtype), _arr(poses, dtype), _arr(confs, dtype)
    act, _ = active_edges(edges, opt, X.shape[0])
    if not act.any():
        return dtype(0)
    e = np.asarray(edges, np.int64)[act]
    with np.errstate(all="ignore"):
        r = log(mul(mul(P[act], inv(X[e[:, 0]])), X[e[:, 1]]))
    return (w[act] * r * r).sum(-1).sum()


def hprod(lin, x):
    """H x: per edge d_e = S_e (x_b - x_a) (x = 0 at a fixed node), per node the signed sum over its list."""
    xo = np.where(lin["opt"][:, None], x, 0)
    d = (lin["S"] @ (xo[lin["b"]] - xo[lin["a"]])[:, :, None])[..., 0]
    y = np.zeros_like(x)
    off, inc = lin["off"], lin["inc"]
    for k in range(lin["n"]):
        for h in inc[off[k]:off[k + 1]]:
            y[k] += d[h >> 1] if h & 1 else -d[h >> 1]
    return y


def damping(lin, dmin, dmax):
    dt = lin["g"].dtype
    return np.clip(np.einsum("nii->ni", lin["blocks"]), dt.type(dmin), dt.type(dmax)) * lin["opt"][:, None]


def pcg(lin, radius, dmin=1e-6, dmax=1e32, rtol=1e-4, max_iter=None):
    """-> d [n,7], stats = (iterations, |r|/|g| by recurrence, model decrease, status)."""
    g, opt, n = lin["g"], lin["opt"], lin["n"]
    dt = g.dtype
    if max_iter is None:
        max_iter = 7 * n
    D = damping(lin, dmin, dmax) / dt.type(radius)
    blk = lin["blocks"] + D[:, :, None] * np.eye(7, dtype=dt)
    blk[~opt] = np.eye(7, dtype=dt)
    L, ok = chol7(blk)
    status = 0 if ok.all() else ST_CHOL

    def A(p):
        return hprod(lin, p) + D * p
    x = np.zeros_like(g)
    r = np.where(opt[:, None], -g, 0)
    gn = np.sqrt((r * r).sum())
    z = np.where(opt[:, None], chol_solve(L, r), 0)
    p = z.copy()
    rz, rn, it = (r * z).sum(), gn, 0
    if ok.all() and gn > 0 and np.isfinite(gn):
        for it in range(1, max_iter + 1):
            Ap = A(p)
            pAp = (p * Ap).sum()
            if not (pAp > 0) or not np.isfinite(pAp):
                status |= ST_BREAKDOWN
                it -= 1
                break
            alpha = rz / pAp
            x, r = x + alpha * p, r - alpha * Ap
            z = np.where(opt[:, None], chol_solve(L, r), 0)
            rz_new, rn = (r * z).sum(), np.sqrt((r * r).sum())
            if not np.isfinite(rz_new) or not np.isfinite(rn):
                status |= ST_BREAKDOWN
                break
            if rn <= dt.type(rtol) * gn:
                break
            p = z + (rz_new / rz) * p
            rz = rz_new
        else:
            status |= ST_MAXITER
    elif not np.isfinite(gn):
        status |= ST_BREAKDOWN
    mdec = -2 * (x * g).sum() - (x * hprod(lin, x)).sum()
    return x, (it, (rn / gn if gn > 0 else dt.type(0)), mdec, status)


def true_residual(lin, x, radius, dmin=1e-6, dmax=1e32):
    """|(H + D / radius) x + g| / |g| over the optimised nodes, with the restated product (numpy, float64)."""
    opt = lin["opt"][:, None]
    D = damping(lin, dmin, dmax) / lin["g"].dtype.type(radius)
    res = np.where(opt, hprod(lin, x) + D * x + lin["g"], 0)
    return float(np.sqrt((res * res).sum()) / np.sqrt((np.where(opt, lin["g"], 0) ** 2).sum()))


def dense_system(lin, radius=None, dmin=1e-6, dmax=1e32):
    """(H [+ D/radius]) as a dense [7n,7n] matrix from the per-edge Jacobians (rows and columns of fixed nodes are zero), and g."""
    n = lin["n"]
    dt = lin["g"].dtype
    H = np.zeros((7 * n, 7 * n), dt)
    for e in np.flatnonzero(lin["act"]):
        a, b = lin["a"][e], lin["b"][e]
        for (i, si) in ((a, -1), (b, 1)):
            for (j, sj) in ((a, -1), (b, 1)):
                if lin["opt"][i] and lin["opt"][j]:
                    H[7 * i:7 * i + 7, 7 * j:7 * j + 7] += si * sj * lin["S"][e]
    if radius is not None:
        H[np.arange(7 * n), np.arange(7 * n)] += (damping(lin, dmin, dmax) / dt.type(radius)).reshape(-1)
    return H, lin["g"].reshape(-1)


def dense_solve(lin, radius, dmin=1e-6, dmax=1e32):
    H, g = dense_system(lin, radius, dmin, dmax)
    keep = np.repeat(lin["opt"], 7)
    x = np.zeros_like(g)
    x[keep] = np.linalg.solve(H[np.ix_(keep, keep)].astype(np.float64), -g[keep].astype(np.float64))
    x = x.reshape(-1, 7)
    return x, (0, 0.0, -2 * (x * lin["g"]).sum() - (x * hprod(lin, x)).sum(), 0)


def lm(nodes, edges, poses, confs, opt_idx="all", *, radius=1e4, dmin=1e-6, dmax=1e32, steps=20, patience=3, decreasing=1e-4, reject=16,
       high=0.5, low=1e-3, up=2.0, down=0.5, pcg_rtol=1e-4, pcg_max_iter=None, solver="pcg", dtype=np.float64):
    """The rule of sta_pgo_optimize -> (nodes, info rows (f, f', rho, radius, iterations, status), status)."""
    X = _arr(nodes, dtype).copy()
    opt = opt_mask(X.shape[0], opt_idx)
    info, status, stall = [], 0, 0
    for _ in range(steps):
        lin = linearize(X, edges, poses, confs, opt, dtype)
        f = lin["f"]
        status |= lin["status"] & ST_INDEX
        if not np.isfinite(f):
            return _arr(nodes, dtype).copy(), info, status | ST_NONFINITE | ST_UNCHANGED
        accepted, good = False, False
        for _t in range(reject):
            if solver == "pcg":
                d, st = pcg(lin, radius, dmin, dmax, pcg_rtol, pcg_max_iter)
            else:
                d, st = dense_solve(lin, radius, dmin, dmax)
            Xn = retract(d, X, opt)
            fn = cost(Xn, edges, poses, confs, opt, dtype)
            rho = (f - fn) / st[2] if (st[2] > 0 and np.isfinite(fn)) else -np.inf
            info.append((float(f), float(fn), float(rho), float(radius), int(st[0]), int(st[3])))
            if rho > high:
                radius *= up
            elif rho < low:
                radius *= down
            if np.isfinite(fn) and fn < f:
                accepted, good = True, (f - fn) >= decreasing * f
                X = Xn
                break
        stall = 0 if (accepted and good) else stall + 1
        if stall >= patience:
            break
    return X, info, status


# ---- graphs ----
def _rng_sim3(rng, n, t=1.0, ang=1.0, ls=0.3):
    xi = np.concatenate([rng.normal(0, t, (n, 3)), rng.normal(0, ang, (n, 3)), rng.normal(0, ls, (n, 1))], 1)
    return exp(xi)


def slam_graph(V, neighbor=4, noise=0.01, seed=0, init_noise=0.0):
    """A two-lap loop of V views (lap = V // 2): view i connects to its `neighbor` predecessors and, on the second lap, to the view one
    lap back.  Every connection makes two nodes (one per view, both at the pair's own scale), a scale edge from each node to the first
    node of its view (weights [2]*6 + [c], identity SE(3), the scale ratio), and a pose edge (n_i, n_j, X_j^-1 X_i at scale 1, one
    confidence for all 7), as the reference's connect_view_i_j does; the nodes are initialised by chaining the measurements."""
    rng = np.random.default_rng(seed)
    lap = max(V // 2, 1)
    ang = 2 * np.pi * np.arange(V) / lap
    view = np.zeros((V, 8))
    view[:, 0], view[:, 1], view[:, 2] = 3 * np.cos(ang), 3 * np.sin(ang), 0.2 * np.sin(3 * ang)
    xi = np.zeros((V, 7))
    xi[:, 5], xi[:, 3] = ang + np.pi / 2, 0.1 * np.cos(2 * ang)
    view[:, 3:7], view[:, 7] = exp(xi)[:, 3:7], 1.0
    gt, init, edges, poses, confs, v2n = [], [], [], [], [], [[] for _ in range(V)]

    def noisy(T, scale_only=False):
        d = rng.normal(0, noise, 7)
        if scale_only:
            d[:6] = 0
        else:
            d[6] = 0
        return mul(exp(d), T)

    for i in range(V):
        js = list(range(i - 1, max(i - neighbor, 0) - 1, -1)) if i else []
        if i >= lap and i - lap not in js:
            js.append(i - lap)
        for j in js:
            s = float(np.exp(rng.normal(0, 0.3)))
            idx = {}
            i_new = True
            for v in (i, j):
                k = len(gt)
                g = view[v].copy()
                g[7] = s
                gt.append(g)
                init.append(np.array([0, 0, 0, 0, 0, 0, 1, 1.0]))
                v2n[v].append(k)
                idx[v] = k
                if len(v2n[v]) > 1:
                    if v == i:
                        i_new = False
                    o = v2n[v][0]
                    m = noisy(np.array([0, 0, 0, 0, 0, 0, 1, s / gt[o][7]]), True)
                    edges.append((k, o)); poses.append(m); confs.append([2.0] * 6 + [rng.uniform(1, 5)])
                    init[k] = mul(init[o], m)
            m = between(gt[idx[j]], gt[idx[i]])
            m[7] = 1.0
            m = noisy(m)
            if i_new:
                init[idx[i]] = mul(init[idx[j]], m)
            edges.append((idx[i], idx[j])); poses.append(m); confs.append([rng.uniform(0.8, 3)] * 7)
    init = np.array(init)
    if init_noise:
        init = mul(exp(rng.normal(0, init_noise, (len(init), 7))), init)
    return dict(nodes=init, edges=np.array(edges, np.int64), poses=np.array(poses), confs=np.array(confs), view_to_node=v2n, gt=np.array(gt),
                V=V)


def _graph(nodes, pairs, rng, noise=0.05):
    gt = _rng_sim3(rng, nodes)
    e = np.array(pairs, np.int64).reshape(-1, 2)
    ok = ((e >= 0) & (e < nodes)).all(1)
    a, b = np.where(ok, e[:, 0], 0), np.where(ok, e[:, 1], 0)
    poses = mul(exp(rng.normal(0, noise, (len(e), 7))), between(gt[b], gt[a]))
    init = mul(exp(rng.normal(0, 0.1, (nodes, 7))), gt)
    return dict(nodes=init, edges=e, poses=poses, confs=rng.uniform(0.5, 3, (len(e), 7)), gt=gt)


def chain(n, seed=1):
    return _graph(n, [(i + 1, i) for i in range(n - 1)] or [(0, 0)], np.random.default_rng(seed))


def triangle(seed=2):
    return _graph(3, [(1, 0), (2, 1), (0, 2)], np.random.default_rng(seed))


def star(deg=40, seed=3):
    """A hub (node 5) with `deg` leaves; the hub is the a side of odd edges and the b side of even ones."""
    n, hub = deg + 1, 5
    leaves = [k for k in range(n) if k != hub]
    return _graph(n, [(hub, l) if i & 1 else (l, hub) for i, l in enumerate(leaves)], np.random.default_rng(seed))


def odd_graph(seed=4):
    """8 nodes; duplicate edges, a self edge, an edge between two fixed nodes (6, 7: see ODD_OPT) and an index of -1."""
    return _graph(8, [(1, 0), (2, 1), (1, 0), (3, 3), (7, 6), (4, -1), (3, 2), (4, 3), (5, 4), (2, 1), (6, 5), (0, 5)], np.random.default_rng(seed))


ODD_OPT = [0, 1, 2, 3, 4, 5]


def random_graph(n, E, seed=5):
    """n nodes, E edges: a spanning chain first (as far as E allows), random pairs after (self edges and repeats included)."""
    rng = np.random.default_rng(seed)
    pairs = [(i + 1, i) for i in range(min(n - 1, E))]
    while len(pairs) < E:
        pairs.append((int(rng.integers(n)), int(rng.integers(n))))
    return _graph(n, pairs, rng)


def window_nodes(view_to_node, view_num, window, loop_related=()):
    s = set()
    for v in range(max(0, view_num - window), view_num):
        s.update(view_to_node[v])
    s.update(loop_related)
    return sorted(s)


GRAPHS = {
    "slam12": lambda: (slam_graph(12), "all"),
    "slam12 window": lambda: (slam_graph(12), "window"),
    "chain2 one fixed": lambda: (chain(2), [1]),
    "triangle": lambda: (triangle(), "all"),
    "star40": lambda: (star(40), "all"),
    "odd": lambda: (odd_graph(), ODD_OPT),
    "slam120": lambda: (slam_graph(120), "all"),
}
LINEARIZE_GRAPHS = ["slam12", "slam12 window", "chain2 one fixed", "triangle", "star40", "odd"]
_CACHE = {}


def get_graph(name):
    """-> (graph, opt_idx, opt mask) of a named graph (built once; nobody writes into it)."""
    if name not in _CACHE:
        g, oi = GRAPHS[name]()
        if oi == "window":
            oi = window_nodes(g["view_to_node"], g["V"], 4)
        _CACHE[name] = (g, oi, opt_mask(len(g["nodes"]), oi))
    return _CACHE[name]


# The arguments of the optimize comparisons.  patience = 2, not the default 3: the rule accepts a trial iff f' < f, and on the noisy
# graphs the third small step in a row lowers f by a few 1e-16 - about 10 roundings of f - so whether it is accepted is decided by
# rounding noise, and two correct implementations end one step (1e-11 in X_a^-1 X_b) apart.  With patience = 2 every decision of the run
# is taken at least DECISION_MARGIN * f away from its threshold (test_pgo_cpu asserts it on the restatement), so both sides take the
# same path and differ by their arithmetic alone.  The noise-free graph needs no such care: its cost falls to 1e-29, where X is exact
# to rounding whatever the last trials decide.
LM_ARGS = dict(pcg_rtol=1e-12, patience=2)
DECISION_MARGIN = 1e-12        # (a sum of 470 positive terms is off by at most 470 * 1.1e-16 = 5e-14 of f, whatever its order)


def lm_graphs():
    """The graphs of the optimize tests: (name, graph, opt_idx)."""
    out = []
    for V in (12, 40):
        g = slam_graph(V)
        out.append((f"slam{V} all", g, "all"))
        out.append((f"slam{V} window", g, window_nodes(g["view_to_node"], V, V // 2, [0])))
    out.append(("noise-free, perturbed start", slam_graph(12, noise=0.0, init_noise=0.05, seed=3), "all"))
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgo_lm.npz")


def write_golden(path=GOLDEN):
    """`python tests/pgo_cases.py`: the restatement's LM results on lm_graphs() at pcg_rtol = 1e-12 (final nodes, float64), recorded so that
    the GPU test does not spend a minute in numpy; test_pgo_cpu checks the record against a fresh run."""
    out = {}
    for name, g, oi in lm_graphs():
        X, info, status = lm(g["nodes"], g["edges"], g["poses"], g["confs"], oi, **LM_ARGS)
        assert status == 0, (name, status)
        out[name] = X
    np.savez_compressed(path, **out)


def load_golden(path=GOLDEN):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def edge_quantities(X, edges):
    """X_a^-1 X_b along every edge with both indices in range, as matrices: what the gauge leaves alone."""
    e = np.asarray(edges, np.int64)
    ok = ((e >= 0) & (e < len(X))).all(1)
    return matrix(between(X[e[ok, 0]], X[e[ok, 1]]))


def op_inputs(count, seed=7, dtype=np.float64):
    """Elements and tangents for the sim3_op tests: both series branches, |phi| within 1e-9 of 0 and of pi, s from 1e-3 to 1e3."""
    rng = np.random.default_rng(seed)
    xi = np.concatenate([rng.normal(0, 1, (count, 3)), rng.normal(0, 1, (count, 3)), rng.uniform(-1, 1, (count, 1))], 1)
    xi[:, 3:6] *= np.minimum(1.0, 3.0 / np.linalg.norm(xi[:, 3:6], axis=1, keepdims=True))
    u = rng.normal(size=(count, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    special = [0.0, 1e-9, 1e-5, 0.9e-4, 1.1e-4, 0.2499, 0.2501, np.pi - 1e-9, np.pi - 1e-3, 3.0, 1.0, 0.1]
    sig = [0.0, 1e-9, -1e-5, np.log(1e-3), np.log(1e3), 0.3, -0.3, 1e-9, 0.0, 2.0, -2.0, 1e-3]
    for i in range(count):
        j = i % 16
        if j < len(special):
            xi[i, 3:6] = special[j] * u[i]
            xi[i, 6] = sig[(i // 16 + j) % len(sig)]
    a = exp(xi)
    xi2 = np.roll(xi, 3, axis=0) * 0.7
    b = exp(xi2)
    return a.astype(dtype), b.astype(dtype), xi.astype(dtype)


if __name__ == "__main__":
    write_golden()
