"""The Sim(3) pose graph on the GPU: what `OnlineSLAM.pose_graph_optimize` (vista_slam/slam.py:108-140, pose_graph.py:70-154) does with
pypose's LM, a dense autograd Jacobian and a dense Cholesky solve.  Here the Gauss-Newton matrix is never formed: it is a graph
Laplacian with 7x7 weights, applied edge by edge and summed node by node, inside a Levenberg-Marquardt loop whose linear solve is a
block-Jacobi preconditioned CG in ONE workgroup.

    nodes = pgo.optimize(slam.frontend, graph.poses[:node_num].tensor(), edges.edges[:edge_num], edges.poses[:edge_num].tensor(),
                         edges.confs[:edge_num], pgo.window_nodes(graph.view_to_node, view_num, window, loop_related))

The contract is written out in include/sta_mi355.h; the yardstick is the numpy restatement tests/pgo_cases.py.  It is not pypose: the
stated differences (float64 inside, inexact PCG steps, 7 tangent unknowns per node, LM constants restated from memory and therefore
keyword arguments) are in the header.  Kernels: csrc/pgo.h.  `plan` holds every size and refusal and needs no GPU.  The sim3 ops,
`index`, `linearize` and `solve` launch and return; `optimize` reads one 64-byte record back per trial step.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .sta_frontend import STAFrontend

MAX_NODES, MAX_EDGES = 8192, 16384
ST_INDEX, ST_NONFINITE, ST_MAXITER, ST_BREAKDOWN, ST_CHOL, ST_UNCHANGED = 1, 2, 4, 8, 16, 32
_MUL, _INV, _BETWEEN, _EXP, _LOG, _RETRACT = range(6)


class Plan(NamedTuple):
    n: int
    E: int
    off_bytes: int
    inc_bytes: int
    index_workspace_bytes: int
    solve_workspace_bytes: int
    workspace_bytes: int


def plan(n: int, E: int) -> Plan:
    """Every size and refusal, on the host (`sta_pgo_plan`; no GPU).  ValueError, with the numbers in the message, for n outside
    [1, 8192] or E outside [1, 16384]."""
    out = (C.c_int64 * 8)()
    lib = _lib.load()
    if lib.sta_pgo_plan(int(n), int(E), out) != 0:
        raise ValueError((lib.sta_last_error() or b"sta_pgo_plan failed").decode())
    return Plan(int(out[5]), int(out[6]), int(out[0]), int(out[1]), int(out[2]), int(out[3]), int(out[4]))


def _f64(fe: STAFrontend, a, width: int) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"expected [count, {width}] (got {tuple(t.shape)})")
    return t.to(device=fe.device, dtype=torch.float64).contiguous()


def _op(fe: STAFrontend, op: int, a, b=None, mask=None) -> torch.Tensor:
    a = _f64(fe, a, 7 if op in (_EXP, _RETRACT) else 8)
    n = a.shape[0]
    if b is not None:
        b = _f64(fe, b, 8)
        if b.shape[0] != n:
            raise ValueError(f"operands of {n} and {b.shape[0]} elements")
    if mask is not None:
        mask = torch.as_tensor(mask).to(device=fe.device).to(torch.uint8).contiguous()
        if mask.shape != (n,):
            raise ValueError(f"mask is [count] (got {tuple(mask.shape)})")
    out = torch.empty(n, 7 if op == _LOG else 8, device=fe.device, dtype=torch.float64)
    _lib.check(fe.lib.sta_sim3_op(fe._h, op, a.data_ptr(), None if b is None else b.data_ptr(), None if mask is None else mask.data_ptr(),
                                  out.data_ptr(), n, fe._stream()))
    return out


def sim3_mul(frontend, a, b):
    return _op(frontend, _MUL, a, b)


def sim3_inv(frontend, a):
    return _op(frontend, _INV, a)


def sim3_between(frontend, a, b):
    """inv(a) b"""
    return _op(frontend, _BETWEEN, a, b)


def sim3_exp(frontend, xi):
    return _op(frontend, _EXP, xi)


def sim3_log(frontend, a):
    return _op(frontend, _LOG, a)


def sim3_retract(frontend, d, a, mask=None):
    """Exp(d) a where mask (None: everywhere) is set, a copy of a elsewhere."""
    return _op(frontend, _RETRACT, d, a, mask)


def sim3_matrix(frontend, a) -> torch.Tensor:
    """[count,8] -> the 4x4 matrices [[sR, t],[0,1]] (torch on the device: a convenience for comparisons, not a hot path)."""
    a = _f64(frontend, a, 8)
    x, y, z, w = a[:, 3], a[:, 4], a[:, 5], a[:, 6]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = torch.zeros(a.shape[0], 4, 4, device=a.device, dtype=torch.float64)
    M[:, :3, :3] = a[:, 7, None, None] * R
    M[:, :3, 3] = a[:, :3]
    M[:, 3, 3] = 1
    return M


def window_nodes(view_to_node, view_num: int, window: int, loop_related: Iterable[int] = ()) -> list:
    """The optimised set of slam.py:115-121, on the host: the nodes of the views [max(0, view_num - window), view_num) and
    `loop_related`, sorted.  (The reference puts its loop_related_views - view ids - into the node set as they are; so does this.)"""
    s = set()
    for v in range(max(0, view_num - window), view_num):
        s.update(view_to_node[v])
    s.update(int(k) for k in loop_related)
    return sorted(s)


class Graph:
    """The device side of one problem: edges int32 [E,2], the opt mask uint8 [n], measurements and weights in float64."""

    def __init__(self, frontend: STAFrontend, n: int, edges, poses, confs, opt_idx: Union[str, Sequence[int], torch.Tensor] = "all"):
        fe = self.frontend = frontend
        e = edges if isinstance(edges, torch.Tensor) else torch.as_tensor(np.asarray(edges))
        if e.dim() != 2 or e.shape[1] != 2:
            raise ValueError(f"edges are [E,2] (got {tuple(e.shape)})")
        self.n, self.E = int(n), int(e.shape[0])
        self.plan = plan(self.n, self.E)
        self.edges = e.to(device=fe.device).clamp(-1, 1 << 30).to(torch.int32).contiguous()
        self.poses, self.confs = _f64(fe, poses, 8), _f64(fe, confs, 7)
        if self.poses.shape[0] != self.E or self.confs.shape[0] != self.E:
            raise ValueError(f"{self.E} edges with {self.poses.shape[0]} measurements and {self.confs.shape[0]} weight rows")
        if isinstance(opt_idx, str):
            if opt_idx != "all":
                raise ValueError(f"opt_idx is 'all' or a list of node indices (got {opt_idx!r})")
            self.opt = torch.ones(self.n, device=fe.device, dtype=torch.uint8)
        else:
            idx = torch.as_tensor(opt_idx, dtype=torch.int64).reshape(-1)
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n):
                raise ValueError(f"opt_idx must lie in [0, {self.n}) (got {int(idx.min())} .. {int(idx.max())})")
            self.opt = torch.zeros(self.n, dtype=torch.uint8)
            self.opt[idx] = 1
            self.opt = self.opt.to(fe.device)
        self.off = self.inc = self.status = None

    def index(self):
        """`sta_pgo_index` -> (off int32 [n+1], inc int32 [2E] of which off[n] are written, status int32 [1]), on the device."""
        fe, dev = self.frontend, self.frontend.device
        ws = torch.empty(self.plan.index_workspace_bytes, device=dev, dtype=torch.uint8)
        self.off = torch.empty(self.n + 1, device=dev, dtype=torch.int32)
        self.inc = torch.empty(2 * self.E, device=dev, dtype=torch.int32)
        self.status = torch.empty(1, device=dev, dtype=torch.int32)
        _lib.check(fe.lib.sta_pgo_index(fe._h, self.edges.data_ptr(), self.opt.data_ptr(), self.n, self.E, ws.data_ptr(), ws.numel(), self.off.data_ptr(),
                                        self.inc.data_ptr(), self.status.data_ptr(), fe._stream()))
        return self.off, self.inc, self.status


def linearize(graph: Graph, nodes, full: bool = True) -> dict:
    """`sta_pgo_linearize` at `nodes` [n,8] -> device tensors r, S, v, c, g, blocks and rec = (f, status) (c and rec alone for
    full=False)."""
    fe, dev = graph.frontend, graph.frontend.device
    X = _f64(fe, nodes, 8)
    if X.shape[0] != graph.n:
        raise ValueError(f"{X.shape[0]} nodes for a graph of {graph.n}")
    if graph.off is None:
        graph.index()
    n, E = graph.n, graph.E
    o = {"c": torch.empty(E, device=dev, dtype=torch.float64), "rec": torch.empty(2, device=dev, dtype=torch.float64)}
    if full:
        o.update(r=torch.empty(E, 7, device=dev, dtype=torch.float64), S=torch.empty(E, 7, 7, device=dev, dtype=torch.float64),
                 v=torch.empty(E, 7, device=dev, dtype=torch.float64), g=torch.empty(n, 7, device=dev, dtype=torch.float64),
                 blocks=torch.empty(n, 7, 7, device=dev, dtype=torch.float64))
    p = lambda k: o[k].data_ptr() if k in o else None
    _lib.check(fe.lib.sta_pgo_linearize(fe._h, X.data_ptr(), graph.edges.data_ptr(), graph.poses.data_ptr(), graph.confs.data_ptr(), graph.opt.data_ptr(),
                                        graph.off.data_ptr(), graph.inc.data_ptr(), graph.status.data_ptr(), n, E, 1 if full else 0, p("r"), p("S"), p("v"),
                                        p("c"), p("g"), p("blocks"), p("rec"), fe._stream()))
    return o


def solve(graph: Graph, lin: dict, radius: float = 1e4, dmin: float = 1e-6, dmax: float = 1e32, rtol: float = 1e-4, max_iter: Optional[int] = None):
    """`sta_pgo_solve` -> (d [n,7], stats float64 [4] = iterations, |r|/|g|, model decrease, status), on the device."""
    fe, dev = graph.frontend, graph.frontend.device
    ws = torch.empty(graph.plan.solve_workspace_bytes, device=dev, dtype=torch.uint8)
    d = torch.empty(graph.n, 7, device=dev, dtype=torch.float64)
    stats = torch.empty(4, device=dev, dtype=torch.float64)
    _lib.check(fe.lib.sta_pgo_solve(fe._h, graph.edges.data_ptr(), graph.opt.data_ptr(), graph.off.data_ptr(), graph.inc.data_ptr(), lin["S"].data_ptr(),
                                    lin["g"].data_ptr(), lin["blocks"].data_ptr(), graph.n, graph.E, float(radius), float(dmin), float(dmax), float(rtol),
                                    int(7 * graph.n if max_iter is None else max_iter), ws.data_ptr(), ws.numel(), d.data_ptr(), stats.data_ptr(), fe._stream()))
    return d, stats


def optimize(frontend: STAFrontend, nodes, edges, poses, confs, opt_idx="all", *, radius: float = 1e4, dmin: float = 1e-6, dmax: float = 1e32,
             steps: int = 20, patience: int = 3, decreasing: float = 1e-4, reject: int = 16, high: float = 0.5, low: float = 1e-3, up: float = 2.0,
             down: float = 0.5, pcg_rtol: float = 1e-4, pcg_max_iter: Optional[int] = None, return_info: bool = False):
    """The LM loop (`sta_pgo_optimize`) -> the nodes [n,8] in the input's dtype and on the frontend's device (with return_info: and a dict
    of per-trial lists f, f_new, rho, radius, pcg_iterations, pcg_status, pcg_residual, model_decrease, and `status`).  Tensors as
    `PoseGraphNodes.poses[:node_num].tensor()` and `PoseGraphEdges.edges / .poses.tensor() / .confs` hold them; a confs of [E] or [E,1]
    is one weight for all 7.  A non-finite cost returns the input's values with status bits 2 | 32."""
    fe = frontend
    src = nodes if isinstance(nodes, torch.Tensor) else torch.as_tensor(np.asarray(nodes))
    if src.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"nodes are float32 or float64 (got {src.dtype})")
    X = _f64(fe, src, 8)
    if X.data_ptr() == src.data_ptr():
        X = X.clone()
    confs = confs if isinstance(confs, torch.Tensor) else torch.as_tensor(np.asarray(confs))
    if confs.dim() == 1:
        confs = confs[:, None]
    if confs.shape[1] == 1:
        confs = confs.expand(-1, 7)
    g = Graph(fe, X.shape[0], edges, poses, confs, opt_idx)
    ws = torch.empty(g.plan.workspace_bytes + 256, device=fe.device, dtype=torch.uint8)
    skip = (-ws.data_ptr()) % 256
    rows = int(steps) * int(reject)
    info = (C.c_double * (8 * rows))()
    n_info, status = C.c_int(0), C.c_int(0)
    _lib.check(fe.lib.sta_pgo_optimize(fe._h, X.data_ptr(), g.edges.data_ptr(), g.poses.data_ptr(), g.confs.data_ptr(), g.opt.data_ptr(), g.n, g.E,
                                       float(radius), float(dmin), float(dmax), int(steps), int(patience), float(decreasing), int(reject), float(high),
                                       float(low), float(up), float(down), float(pcg_rtol), int(7 * g.n if pcg_max_iter is None else pcg_max_iter),
                                       ws.data_ptr() + skip, g.plan.workspace_bytes, info, rows, C.byref(n_info), C.byref(status), fe._stream()))
    out = src.to(fe.device).clone() if status.value & ST_UNCHANGED else X.to(src.dtype)
    if not return_info:
        return out
    a = np.frombuffer(info, np.float64).reshape(rows, 8)[:n_info.value]
    return out, {"f": a[:, 0].tolist(), "f_new": a[:, 1].tolist(), "rho": a[:, 2].tolist(), "radius": a[:, 3].tolist(),
                 "pcg_iterations": a[:, 4].astype(int).tolist(), "pcg_status": a[:, 5].astype(int).tolist(), "pcg_residual": a[:, 6].tolist(),
                 "model_decrease": a[:, 7].tolist(), "status": int(status.value)}
