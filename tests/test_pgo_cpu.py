"""Host only: the pose-graph contract (include/sta_mi355.h: sta_sim3_op / sta_pgo_*) - the numpy restatement tests/pgo_cases.py against
second statements (a scaled-Taylor expm of the generator, central differences, a dense J^T W J, numpy.linalg.solve, LM with the dense
solve), sta_pgo_plan's values and refusals through the built library, the ctypes signatures, and the measurement of the two tolerances
the GPU tests use (TOL_EDGE, TOL_LM: the rules are in pgo_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import pgo_cases as P

LD = np.longdouble


def expm(G):
    """Scaled Taylor: exp(G / 2^10) by 24 terms, squared 10 times (longdouble in, longdouble out)."""
    G = G / LD(1024)
    M = np.broadcast_to(np.eye(G.shape[-1], dtype=G.dtype), G.shape).copy()
    T = M.copy()
    for k in range(1, 25):
        T = T @ G / LD(k)
        M = M + T
    for _ in range(10):
        M = M @ M
    return M


def generator(xi):
    G = np.zeros(xi.shape[:-1] + (4, 4), xi.dtype)
    G[..., :3, :3] = xi[..., 6, None, None] * np.eye(3, dtype=xi.dtype) + P.hat(xi[..., 3:6])
    G[..., :3, 3] = xi[..., :3]
    return G


def rel(a, b):
    """max over rows of |a - b| relative to 1 + max|row of b|"""
    a, b = np.asarray(a, LD).reshape(len(a), -1), np.asarray(b, LD).reshape(len(b), -1)
    return float((np.abs(a - b).max(1) / (1 + np.abs(b).max(1))).max())


def test_exp_equals_expm_of_the_generator():
    _, _, xi = P.op_inputs(1025)
    assert rel(P.matrix(P.exp(xi)), expm(generator(xi.astype(LD)))) < 1e-14
    # (ten squarings cost expm itself about 2^10 longdouble roundings: 1e-16)
    assert rel(P.matrix(P.exp(xi.astype(LD))), expm(generator(xi.astype(LD)))) < 1e-15


def test_log_inverts_exp_across_the_branches():
    _, _, xi = P.op_inputs(1025)
    theta = np.linalg.norm(xi[:, 3:6], axis=1)
    assert (theta < P.QUAT_SERIES).any() and ((theta > P.QUAT_SERIES) & (theta < P.PHI_SERIES)).any() and (theta > P.PHI_SERIES).any()
    assert (theta > np.pi - 1e-8).any() and (np.abs(xi[:, 6]) < 1e-8).any() and (np.abs(xi[:, 6]) > 6.9).any() and theta.max() <= np.pi
    back = P.log(P.exp(xi))
    near_pi = theta > np.pi - 1e-6          # phi and -phi are the same rotation at pi: compare the elements there
    assert rel(back[~near_pi], xi[~near_pi]) < 1e-12
    assert rel(P.matrix(P.exp(back)), P.matrix(P.exp(xi))) < 1e-12
    a, b, _ = P.op_inputs(65)
    assert rel(P.matrix(P.mul(a, P.inv(a))), np.broadcast_to(np.eye(4), (65, 4, 4))) < 1e-13
    assert rel(P.matrix(P.mul(a, b)), P.matrix(a) @ P.matrix(b)) < 1e-13
    assert rel(P.matrix(P.between(a, b)), np.linalg.inv(P.matrix(a)) @ P.matrix(b)) < 1e-11


def test_adjoint_identities():
    a, _, xi = P.op_inputs(65)
    xi = xi * 0.5
    Ta, G = P.matrix(a), generator(xi)
    lhs = generator((P.Ad(a) @ xi[:, :, None])[..., 0])
    assert rel(lhs, Ta @ G @ np.linalg.inv(Ta)) < 1e-10
    eta = np.roll(xi, 1, axis=0)
    Ge = generator(eta)
    assert rel(generator((P.ad(xi) @ eta[:, :, None])[..., 0]), G @ Ge - Ge @ G) < 1e-14
    # Jl by 32 Horner terms against 48
    big = xi / np.linalg.norm(xi, axis=1, keepdims=True) * 3.5
    assert rel(P.Jl(big.astype(LD)), P.Jl(big.astype(LD), terms=48)) < 1e-14


def test_edge_jacobian_equals_central_differences():
    g = P.triangle()
    X, h = g["nodes"], 1e-6
    opt = P.opt_mask(3)
    lin = P.linearize(X, g["edges"], g["poses"], g["confs"], opt)
    M = P.elim_solve(P.Jl(lin["r"]), P.Ad(P.mul(g["poses"], P.inv(X[lin["a"]]))))

    def res(Xp):
        return P.log(P.mul(P.mul(g["poses"], P.inv(Xp[lin["a"]])), Xp[lin["b"]]))
    for e in range(3):
        for node, sign in ((lin["b"][e], 1.0), (lin["a"][e], -1.0)):
            for col in range(7):
                d = np.zeros((3, 7))
                d[node, col] = h
                num = (res(P.retract(d, X))[e] - res(P.retract(-d, X))[e]) / (2 * h)
                assert np.abs(num - sign * M[e][:, col]).max() < 1e-7


GRAPHS = P.LINEARIZE_GRAPHS
_get = P.get_graph


@pytest.mark.parametrize("name", GRAPHS)
def test_laplacian_product_equals_dense_jtwj(name):
    g, _, opt = _get(name)
    lin = P.linearize(g["nodes"], g["edges"], g["poses"], g["confs"], opt)
    n = lin["n"]
    # J from the per-edge Jacobians, W from the weights
    act = np.flatnonzero(lin["act"])
    J = np.zeros((7 * len(act), 7 * n))
    X = g["nodes"]
    M = P.elim_solve(P.Jl(lin["r"]), P.Ad(P.mul(g["poses"], P.inv(X[lin["a"]]))))
    for i, e in enumerate(act):
        a, b = lin["a"][e], lin["b"][e]
        if opt[b]:
            J[7 * i:7 * i + 7, 7 * b:7 * b + 7] = M[e]
        if opt[a]:
            J[7 * i:7 * i + 7, 7 * a:7 * a + 7] = -M[e]
    W = np.diag(g["confs"][act].reshape(-1))
    H = J.T @ W @ J
    x = np.random.default_rng(0).normal(size=(n, 7)) * opt[:, None]
    scale = 1 + np.abs(H @ x.reshape(-1)).max()
    assert np.abs(P.hprod(lin, x).reshape(-1) - H @ x.reshape(-1)).max() < 1e-12 * scale
    assert np.abs(lin["g"].reshape(-1) - J.T @ W @ lin["r"][act].reshape(-1)).max() < 1e-12 * scale
    assert np.abs(P.dense_system(lin)[0] - H).max() < 1e-12 * scale
    assert abs(lin["f"] - P.cost(X, g["edges"], g["poses"], g["confs"], opt)) <= 1e-14 * (1 + lin["f"])
    if name == "odd":
        assert lin["status"] == P.ST_INDEX and list(lin["act"]) == [True, True, True, False, False, False, True, True, True, True, True, True]


@pytest.mark.parametrize("name", list(P.SOLVE_SYSTEMS))
def test_pcg_equals_the_dense_solve(name):
    """The systems of the GPU solve test: the restatement's own PCG at rtol = 1e-10 reaches a TRUE relative residual <= 1e-9."""
    g, _, opt = _get(name)
    radius, max_iter = P.SOLVE_SYSTEMS[name]
    lin = P.linearize(g["nodes"], g["edges"], g["poses"], g["confs"], opt)
    d, st = P.pcg(lin, radius, rtol=1e-10, max_iter=max_iter)
    res = P.true_residual(lin, d, radius)
    assert st[3] == 0 and st[0] <= (max_iter or 7 * lin["n"]) and res <= 1e-9, (st, res)
    if lin["n"] <= 100:               # (the product itself is checked against the dense J^T W J above)
        A, gg = P.dense_system(lin, radius)
        keep = np.repeat(opt, 7)
        assert abs(np.linalg.norm((A @ d.reshape(-1) + gg)[keep]) / np.linalg.norm(gg[keep]) - res) <= 1e-12
        ref = np.linalg.solve(A[np.ix_(keep, keep)], -gg[keep])
        assert np.abs(d.reshape(-1)[keep] - ref).max() <= 1e-6 * (1 + np.abs(ref).max())
    assert (d[~opt] == 0).all()


def test_pcg_exits_report_their_status():
    g, _, opt = _get("slam12")
    lin = P.linearize(g["nodes"], g["edges"], g["poses"], g["confs"], opt)
    _, st = P.pcg(lin, 1e4, rtol=1e-10, max_iter=3)
    assert st[0] == 3 and st[3] == P.ST_MAXITER
    bad = dict(lin)
    bad["S"] = -lin["S"]                       # p^T A p < 0 with a positive definite preconditioner: a breakdown
    _, st = P.pcg(bad, 1e4, rtol=1e-10)
    assert st[3] & P.ST_BREAKDOWN and st[0] == 0


edge_quantities, lm_graphs = P.edge_quantities, P.lm_graphs


def test_lm_with_pcg_equals_lm_with_the_dense_solve():
    g = P.slam_graph(12)
    Xp, ip, sp = P.lm(g["nodes"], g["edges"], g["poses"], g["confs"], pcg_rtol=1e-12)
    Xd, idn, sd = P.lm(g["nodes"], g["edges"], g["poses"], g["confs"], solver="dense")
    assert sp == 0 and sd == 0 and ip[0][0] > 100 * ip[-1][1]
    assert abs(ip[-1][1] - idn[-1][1]) <= 1e-8 * idn[-1][1]
    assert rel(edge_quantities(Xp, g["edges"]), edge_quantities(Xd, g["edges"])) < 1e-6
    # a noise-free graph from a perturbed start ends at a cost of zero
    g0 = P.slam_graph(12, noise=0.0, init_noise=0.05, seed=3)
    X0, i0, _ = P.lm(g0["nodes"], g0["edges"], g0["poses"], g0["confs"], pcg_rtol=1e-12)
    assert i0[0][0] > 1e-2 and i0[-1][1] < 1e-20 * max(i0[0][0], 1)
    assert rel(edge_quantities(X0, g0["edges"]), edge_quantities(g0["gt"], g0["edges"])) < 1e-9
    # a non-finite measurement: the nodes come back unchanged, the status says so
    poses = g["poses"].copy()
    poses[3, 0] = np.nan
    Xn, _, sn = P.lm(g["nodes"], g["edges"], poses, g["confs"])
    assert sn & P.ST_UNCHANGED and sn & P.ST_NONFINITE and np.array_equal(Xn, g["nodes"])


def linearize_graphs():
    return [_get(k) for k in GRAPHS]


def test_tol_edge_is_what_its_rule_gives():
    """64 x the float64-versus-longdouble error of the restatement on the GPU test inputs, at least 1e-13."""
    worst = 0.0
    a, b, xi = P.op_inputs(1025)
    al, bl, xil = a.astype(LD), b.astype(LD), xi.astype(LD)
    for f64, fl in ((P.exp(xi), P.exp(xil)), (P.mul(a, b), P.mul(al, bl)), (P.inv(a), P.inv(al)), (P.between(a, b), P.between(al, bl)),
                    (P.retract(xi, b), P.retract(xil, bl))):
        worst = max(worst, rel(P.matrix(f64), P.matrix(fl)))
    ll = P.log(al)
    near_pi = np.linalg.norm(ll[:, 3:6], axis=1) > np.pi - 1e-6
    worst = max(worst, rel(P.log(a)[~near_pi], ll[~near_pi]), rel(P.matrix(P.exp(P.log(a))), P.matrix(P.exp(ll))))
    for g, _, opt in linearize_graphs():
        l64 = P.linearize(g["nodes"], g["edges"], g["poses"], g["confs"], opt)
        lld = P.linearize(g["nodes"], g["edges"], g["poses"], g["confs"], opt, LD)
        for k in ("r", "S", "v", "g", "blocks"):
            worst = max(worst, rel(l64[k], lld[k]))
        worst = max(worst, float(abs(l64["f"] - lld["f"]) / (1 + lld["f"])))
    print(f"float64 versus longdouble: {worst:.3e}; rule: {max(1e-13, 64 * worst):.3e}; TOL_EDGE = {P.TOL_EDGE:.3e}")
    rule = max(1e-13, 64 * worst)
    assert rule <= P.TOL_EDGE <= 1.25 * rule, (worst, rule, P.TOL_EDGE)


def test_tol_lm_is_what_its_rule_gives():
    """10 x the spread of the float64 restatement between two edge orderings (the edge list reversed) on the final cost and on
    X_a^-1 X_b along every edge."""
    worst, golden = 0.0, P.load_golden()
    for name, g, oi in lm_graphs():
        X1, i1, _ = P.lm(g["nodes"], g["edges"], g["poses"], g["confs"], oi, **P.LM_ARGS)
        if not name.startswith("noise-free"):
            # every decision of the run stands clear of rounding: accept (f' < f), plateau (f - f' against 1e-4 f), radius (rho against 0.5)
            for f, fn, rho, _radius, _it, st in i1:
                assert st == 0 and f - fn >= P.DECISION_MARGIN * f and abs((f - fn) - 1e-4 * f) >= P.DECISION_MARGIN * f and abs(rho - 0.5) > 0.1, (name, f, fn, rho)
        # the record the GPU test compares with (tests/golden/pgo_lm.npz) is this run
        assert rel(edge_quantities(golden[name], g["edges"]), edge_quantities(X1, g["edges"])) <= P.TOL_LM / 2
        X2, i2, _ = P.lm(g["nodes"], g["edges"][::-1].copy(), g["poses"][::-1].copy(), g["confs"][::-1].copy(), oi, **P.LM_ARGS)
        f1, f2 = i1[-1][1], i2[-1][1]
        spread = max(abs(f1 - f2) / (1 + max(f1, f2)), rel(edge_quantities(X1, g["edges"]), edge_quantities(X2, g["edges"])))
        print(f"{name}: spread {spread:.3e} (f {f1:.6e} / {f2:.6e}, trials {len(i1)} / {len(i2)})")
        worst = max(worst, spread)
    print(f"rule: {10 * worst:.3e}; TOL_LM = {P.TOL_LM:.3e}")
    assert 10 * worst <= P.TOL_LM <= 12.5 * worst, (worst, P.TOL_LM)       # (the constant is the rule's value rounded up to two digits)


def test_index_lists_are_ascending_and_hold_active_half_edges_only():
    for name in GRAPHS:
        g, _, opt = _get(name)
        n = len(g["nodes"])
        off, inc, status = P.index(g["edges"], opt, n)
        act, _ = P.active_edges(g["edges"], opt, n)
        for k in range(n):
            lst = inc[off[k]:off[k + 1]]
            assert (np.diff(lst) > 0).all() and all(act[h >> 1] and g["edges"][h >> 1][h & 1] == k and opt[k] for h in lst)
        assert off[n] == sum(int(opt[a]) + int(opt[b]) for (a, b), on in zip(g["edges"], act) if on)
    g = P.star(40)
    off, inc, _ = P.index(g["edges"], P.opt_mask(41), 41)
    assert off[6] - off[5] == 40 and (inc[off[5]:off[6]] >> 1 == np.arange(40)).all()


def test_window_nodes_is_the_reference_set():
    from vista_slam_amd import pgo
    v2n = {0: [0, 3], 1: [1, 2, 5], 2: [4], 3: [6, 7], 4: []}
    assert pgo.window_nodes(v2n, 4, 2, {0}) == [0, 4, 6, 7] == P.window_nodes(v2n, 4, 2, {0})
    assert pgo.window_nodes(v2n, 2, 10) == [0, 1, 2, 3, 5]


def test_plan_values_and_refusals():
    from vista_slam_amd import _lib, pgo
    p = pgo.plan(1062, 1473)
    assert (p.n, p.E, p.off_bytes, p.inc_bytes, p.index_workspace_bytes) == (1062, 1473, 1063 * 4, 1473 * 8, 1473 * 16)
    assert p.solve_workspace_bytes == 8 * (1062 * 84 + 1473 * 36)
    assert p.workspace_bytes % 256 == 0 and p.workspace_bytes >= p.solve_workspace_bytes + 8 * (1473 * 64 + 1062 * 71)
    assert pgo.plan(8192, 16384).workspace_bytes < 32 << 20 and pgo.plan(1, 1).n == 1
    lib = _lib.load()
    for n, E, words in ((0, 5, b"n must lie in [1, 8192] (got 0)"), (8193, 5, b"(got 8193)"), (5, 0, b"E must lie in [1, 16384] (got 0)"),
                        (5, 16385, b"(got 16385)")):
        assert lib.sta_pgo_plan(n, E, (C.c_int64 * 8)()) == -1 and words in lib.sta_last_error()
        with pytest.raises(ValueError):
            pgo.plan(n, E)
    assert lib.sta_pgo_plan(5, 5, None) == -1


def test_ctypes_signatures():
    from vista_slam_amd import _lib
    _i, _vp, _i64, _d = C.c_int, C.c_void_p, C.c_int64, C.c_double
    S = _lib.SIGNATURES
    assert S["sta_pgo_plan"] == (_i, [_i, _i, C.POINTER(_i64)])
    assert S["sta_sim3_op"] == (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i64, _vp])
    assert S["sta_pgo_index"] == (_i, [_vp, _vp, _vp, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp])
    assert S["sta_pgo_linearize"] == (_i, [_vp] * 9 + [_i, _i, _i] + [_vp] * 8)
    assert S["sta_pgo_solve"] == (_i, [_vp] * 8 + [_i, _i, _d, _d, _d, _d, _i, _vp, _i64, _vp, _vp, _vp])
    assert S["sta_pgo_optimize"] == (_i, [_vp] * 6 + [_i, _i, _d, _d, _d, _i, _i, _d, _i, _d, _d, _d, _d, _d, _i, _vp, _i64, C.POINTER(_d), _i,
                                          C.POINTER(_i), C.POINTER(_i), _vp])
    from vista_slam_amd import build
    assert "pgo.h" in build.DEPS
