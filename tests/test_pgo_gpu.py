"""GPU: the Sim(3) pose graph (csrc/pgo.h: sta_sim3_op / sta_pgo_index / sta_pgo_linearize / sta_pgo_solve / sta_pgo_optimize,
vista_slam_amd.pgo) against the numpy restatement of its contract (tests/pgo_cases.py), through the C ABI with guard regions behind
every output and the workspace, and through the Python layer.  The index lists are compared with array_equal; group elements as
matrices and every per-edge / per-node quantity at TOL_EDGE relative to 1 + max|row|; LM results at TOL_LM on what the gauge leaves
alone (the final cost, X_a^-1 X_b along every edge).  Both tolerances are measured on the restatement alone by tests/test_pgo_cpu.py; the
rules are in pgo_cases.py.  The graphs are the smallest that can go wrong: 1 and 2 nodes, sizes either side of a wave, more than 1024
nodes and edges (a second round of the one-workgroup loops), a degree-40 star, duplicate edges, a self edge, an edge between fixed
nodes, an index of -1.  The restatement's LM results come from tests/golden/pgo_lm.npz (checked against a fresh run by the CPU test)."""
import functools

import numpy as np
import pytest

import pgo_cases as P

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256


@pytest.fixture(scope="module")
def m():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    fe = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield fe
    del fe


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Out:
    """`nbytes` of device memory filled with a pattern, with a guard region behind it."""

    def __init__(self, nbytes):
        import torch
        self.nbytes = int(nbytes)
        self.t = torch.full((self.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr()

    def raw(self):
        return self.t.cpu().numpy()

    def get(self, dtype, shape=(-1,)):
        raw = self.raw()
        assert (raw[self.nbytes:] == FILL).all(), "bytes behind an output were written"
        return raw[:self.nbytes].view(dtype).reshape(shape).copy()


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    assert a.shape == b.shape and np.isfinite(a).all()
    return float((np.abs(a - b).max(1) / (1 + np.abs(b).max(1))).max()) if a.size else 0.0


def sim3(m, op, a, b=None, mask=None, width=8):
    import torch
    from vista_slam_amd import _lib
    n = len(a)
    out = Out(n * width * 8)
    ta, tb, tm = _up(a), (None if b is None else _up(b)), (None if mask is None else _up(mask.astype(np.uint8)))
    _lib.check(m.lib.sta_sim3_op(m._h, op, ta.data_ptr(), None if tb is None else tb.data_ptr(), None if tm is None else tm.data_ptr(), out.ptr, n, m._stream()))
    torch.cuda.synchronize()
    return out.get(np.float64, (n, width))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1025])
def test_sim3_ops(m, count):
    a, b, xi = P.op_inputs(count)
    theta = np.linalg.norm(xi[:, 3:6], axis=1)
    if count >= 63:
        assert (theta < 1e-8).any() and (theta > np.pi - 1e-8).any() and (theta < P.PHI_SERIES).any() and (np.abs(xi[:, 6]) > 6.9).any()
    worst = {}
    for name, got, ref in (("mul", sim3(m, 0, a, b), P.mul(a, b)), ("inv", sim3(m, 1, a), P.inv(a)), ("between", sim3(m, 2, a, b), P.between(a, b)),
                           ("exp", sim3(m, 3, xi), P.exp(xi)), ("retract", sim3(m, 5, xi, b), P.retract(xi, b))):
        worst[name] = rel(P.matrix(got), P.matrix(ref))
        assert np.abs(np.linalg.norm(got[:, 3:7], axis=1) - 1).max() < 1e-15, name
    got, ref = sim3(m, 4, a, width=7), P.log(a)
    away = np.linalg.norm(ref[:, 3:6], axis=1) < np.pi - 1e-6          # (phi and -phi are one rotation at pi)
    worst["log"] = max(rel(got[away], ref[away]), rel(P.matrix(P.exp(got)), P.matrix(P.exp(ref))))
    assert (np.linalg.norm(got[:, 3:6], axis=1) <= np.pi + 1e-15).all()
    print(count, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= P.TOL_EDGE, worst
    mask = (np.arange(count) % 3 != 1)
    got = sim3(m, 5, xi, b, mask)
    assert np.array_equal(got[~mask], b[~mask]) and rel(P.matrix(got), P.matrix(P.retract(xi, b, mask))) <= P.TOL_EDGE


class Dev:
    """A graph on the device through the C ABI: index -> linearize -> solve, every output guarded."""

    def __init__(self, m, g, opt):
        from vista_slam_amd import pgo
        self.m, self.g, self.opt_np = m, g, opt
        self.n, self.E = len(g["nodes"]), len(g["edges"])
        self.plan = pgo.plan(self.n, self.E)
        self.edges, self.opt = _up(g["edges"].astype(np.int32)), _up(opt.astype(np.uint8))
        self.nodes, self.poses, self.confs = _up(g["nodes"]), _up(g["poses"]), _up(g["confs"])

    def index(self):
        import torch
        from vista_slam_amd import _lib
        m, p = self.m, self.plan
        self.ws, self.off, self.inc, self.status = Out(p.index_workspace_bytes), Out(p.off_bytes), Out(p.inc_bytes), Out(4)
        _lib.check(m.lib.sta_pgo_index(m._h, self.edges.data_ptr(), self.opt.data_ptr(), self.n, self.E, self.ws.ptr, p.index_workspace_bytes, self.off.ptr,
                                       self.inc.ptr, self.status.ptr, m._stream()))
        torch.cuda.synchronize()
        self.ws.get(np.uint8)
        return self.off.get(np.int32), self.inc.get(np.int32), int(self.status.get(np.int32)[0])

    def linearize(self, full=True, nodes=None):
        import torch
        from vista_slam_amd import _lib
        m, n, E = self.m, self.n, self.E
        o = {k: Out(8 * s) for k, s in (("r", E * 7), ("S", E * 49), ("v", E * 7), ("c", E), ("g", n * 7), ("blocks", n * 49), ("rec", 2))}
        p = (lambda k: o[k].ptr) if full else (lambda k: o[k].ptr if k in ("c", "rec") else None)
        X = self.nodes if nodes is None else nodes
        _lib.check(m.lib.sta_pgo_linearize(m._h, X.data_ptr(), self.edges.data_ptr(), self.poses.data_ptr(), self.confs.data_ptr(), self.opt.data_ptr(),
                                           self.off.ptr, self.inc.ptr, self.status.ptr, n, E, 1 if full else 0, p("r"), p("S"), p("v"), p("c"), p("g"),
                                           p("blocks"), p("rec"), m._stream()))
        torch.cuda.synchronize()
        self.lin = o
        out = {k: o[k].get(np.float64, s) for k, s in (("r", (E, 7)), ("S", (E, 7, 7)), ("v", (E, 7)), ("c", (E,)), ("g", (n, 7)), ("blocks", (n, 7, 7)),
                                                       ("rec", (2,)))}
        if not full:
            for k in ("r", "S", "v", "g", "blocks"):
                assert (out[k].view(np.uint8) == FILL).all(), f"the cost-only form wrote {k}"
        return out

    def solve(self, radius, rtol, max_iter, S=None):
        import torch
        from vista_slam_amd import _lib
        m, p = self.m, self.plan
        ws, d, stats = Out(p.solve_workspace_bytes), Out(self.n * 56), Out(32)
        _lib.check(m.lib.sta_pgo_solve(m._h, self.edges.data_ptr(), self.opt.data_ptr(), self.off.ptr, self.inc.ptr, self.lin["S"].ptr if S is None else S.data_ptr(),
                                       self.lin["g"].ptr, self.lin["blocks"].ptr, self.n, self.E, radius, 1e-6, 1e32, rtol, max_iter, ws.ptr,
                                       p.solve_workspace_bytes, d.ptr, stats.ptr, m._stream()))
        torch.cuda.synchronize()
        ws.get(np.uint8)
        return d.get(np.float64, (self.n, 7)), stats.get(np.float64)


def _random(n, E):
    g = P.random_graph(n, E)
    return g, P.opt_mask(n, [k for k in range(n) if k % 3 != 2] if n > 2 else "all")


@pytest.mark.parametrize("name", P.LINEARIZE_GRAPHS + ["random 1/1", "random 2/2", "random 2/1", "random 64/64", "random 65/65", "random 1030/2100"])
def test_index_equals_the_restatement(m, name):
    if name.startswith("random"):
        g, opt = _random(*(int(t) for t in name.split()[1].split("/")))
    else:
        g, _, opt = P.get_graph(name)
    n = len(g["nodes"])
    exp_off, exp_inc, exp_status = P.index(g["edges"], opt, n)
    off, inc, status = Dev(m, g, opt).index()
    assert np.array_equal(off, exp_off) and np.array_equal(inc[:off[n]], exp_inc) and status == exp_status
    assert (inc[off[n]:].view(np.uint8) == FILL).all(), "entries past off[n] were written"
    if name == "star40":
        assert off[6] - off[5] == 40 and np.array_equal(inc[off[5]:off[6]] >> 1, np.arange(40))
    if name == "odd":
        assert status == P.ST_INDEX and not {3, 4, 5} & set((inc[:off[n]] >> 1).tolist())       # the self edge, fixed-fixed, the -1: absent


@functools.lru_cache(maxsize=None)
def _ref_lin(name):
    g, _, opt = P.get_graph(name)
    return P.linearize(g["nodes"], g["edges"], g["poses"], g["confs"], opt)


@pytest.mark.parametrize("name", P.LINEARIZE_GRAPHS)
def test_linearize_equals_the_restatement(m, name):
    g, _, opt = P.get_graph(name)
    ref = _ref_lin(name)
    d = Dev(m, g, opt)
    d.index()
    got = d.linearize()
    worst = {k: rel(got[k], ref[k]) for k in ("r", "S", "v", "g", "blocks")}
    worst["c"] = rel(got["c"][:, None], ref["c"][:, None])
    worst["f"] = abs(got["rec"][0] - ref["f"]) / (1 + ref["f"])
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= P.TOL_EDGE, worst
    assert int(got["rec"][1]) == ref["status"]
    z = ~ref["act"]
    assert not got["r"][z].any() and not got["S"][z].any() and not got["v"][z].any() and not got["c"][z].any() and not got["g"][~opt].any()
    cost = d.linearize(full=False)
    assert cost["rec"].tobytes() == got["rec"].tobytes() and cost["c"].tobytes() == got["c"].tobytes()


@pytest.mark.parametrize("name", list(P.SOLVE_SYSTEMS))
def test_solve_reaches_the_residual(m, name):
    g, _, opt = P.get_graph(name)
    radius, max_iter = P.SOLVE_SYSTEMS[name]
    max_iter = max_iter or 7 * len(g["nodes"])
    d = Dev(m, g, opt)
    d.index()
    lin = d.linearize()
    x, stats = d.solve(radius, 1e-10, max_iter)
    ref = dict(_ref_lin(name) if name in P.LINEARIZE_GRAPHS else P.linearize(g["nodes"], g["edges"], g["poses"], g["confs"], opt))
    res = P.true_residual(ref, x, radius)
    print(name, "iterations", stats[0], "recurrence", stats[1], "true", res, "model decrease", stats[2])
    assert stats[3] == 0 and 1 <= stats[0] <= max_iter and stats[1] <= 1e-10 and res <= 1e-8
    assert not x[~opt].any()
    mdec = -2 * (x * ref["g"]).sum() - (x * P.hprod(ref, x)).sum()
    assert abs(stats[2] - mdec) <= 1e-9 * abs(mdec)
    x2, stats2 = d.solve(radius, 1e-10, max_iter)
    assert x2.tobytes() == x.tobytes() and stats2.tobytes() == stats.tobytes(), "two runs differ"
    if name == "slam12":
        x3, stats3 = d.solve(radius, 1e-10, 3)
        assert stats3[0] == 3 and int(stats3[3]) == P.ST_MAXITER and np.isfinite(x3).all()
        import torch
        neg = -_up(lin["S"])                                   # p^T A p < 0 under a positive definite preconditioner
        x4, stats4 = d.solve(radius, 1e-10, max_iter, S=neg)
        torch.cuda.synchronize()
        assert stats4[0] == 0 and int(stats4[3]) == P.ST_BREAKDOWN and not x4.any()


def _gauge_free(X, g, opt_idx):
    opt = P.opt_mask(len(X), opt_idx)
    return P.cost(X, g["edges"], g["poses"], g["confs"], opt), P.edge_quantities(X, g["edges"])


@pytest.mark.parametrize("index", range(5))
def test_optimize_ends_where_the_restatement_ends(m, index):
    from vista_slam_amd import pgo
    name, g, oi = P.lm_graphs()[index]
    ref = P.load_golden()[name]
    X, info = pgo.optimize(m, g["nodes"], g["edges"], g["poses"], g["confs"], oi, return_info=True, **P.LM_ARGS)
    X = X.cpu().numpy()
    assert X.dtype == np.float64 and info["status"] == 0 and len(info["f"]) >= 3
    f, Q = _gauge_free(X, g, oi)
    f_ref, Q_ref = _gauge_free(ref, g, oi)
    spread = max(abs(f - f_ref) / (1 + max(f, f_ref)), rel(Q, Q_ref))
    print(name, "f", info["f"][0], "->", f, "restatement", f_ref, "spread", spread, "trials", len(info["f"]))
    for row in list(zip(info["f"], info["f_new"], info["rho"], info["radius"], info["pcg_iterations"], info["pcg_status"]))[:12]:
        print("   ", row)
    assert spread <= P.TOL_LM, (spread, P.TOL_LM)
    fixed = ~P.opt_mask(len(X), oi)
    assert np.array_equal(X[fixed], g["nodes"][fixed])
    if name.startswith("noise-free"):
        assert info["f"][0] > 1e-2 and f < 1e-20 and rel(Q, P.edge_quantities(g["gt"], g["edges"])) < 1e-9


def test_optimize_refuses_a_non_finite_measurement_and_keeps_float32(m):
    import torch
    from vista_slam_amd import pgo
    g = P.slam_graph(12)
    poses = g["poses"].copy()
    poses[3, 0] = np.nan
    X, info = pgo.optimize(m, g["nodes"], g["edges"], poses, g["confs"], return_info=True)
    assert info["status"] & P.ST_UNCHANGED and info["status"] & P.ST_NONFINITE
    assert X.cpu().numpy().tobytes() == g["nodes"].tobytes()
    n32 = torch.from_numpy(g["nodes"].astype(np.float32)).cuda()
    X32, info = pgo.optimize(m, n32, torch.from_numpy(g["edges"]).cuda(), torch.from_numpy(g["poses"].astype(np.float32)).cuda(),
                             torch.from_numpy(g["confs"].astype(np.float32)).cuda(), return_info=True)
    assert X32.dtype == torch.float32 and X32.shape == n32.shape and X32.is_cuda and info["status"] == 0
    X64 = pgo.optimize(m, n32.double(), g["edges"], g["poses"].astype(np.float32), g["confs"].astype(np.float32))
    assert torch.equal(X32, X64.float())                       # float32 in: the same float64 problem, rounded once at the end
    f0 = P.cost(g["nodes"], g["edges"], g["poses"], g["confs"], P.opt_mask(len(g["nodes"])))
    f1 = P.cost(X32.double().cpu().numpy(), g["edges"], g["poses"], g["confs"], P.opt_mask(len(g["nodes"])))
    assert f1 < 0.01 * f0
