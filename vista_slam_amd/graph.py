"""The pose graph of `OnlineSLAM` on the device: `PoseGraphNodes` / `PoseGraphEdges` (vista_slam/pose_graph.py:5-54) and the bookkeeping of
`connect_view_i_j` (slam.py:191-241).  The reference keeps every node's depth and confidence map on the host and copies them up again
for every scale edge, runs about a dozen small torch launches per node, reads `.item()` twice per node and multiplies in pypose.  Here
the poses, edges, weights, the map pool and the per-view tables are device arrays allocated once; `commit` performs `connect_view_i_j`
for all candidate edges of a keyframe in two launches (`sta_graph_commit`), `export` gathers every view's best node in one
(`sta_graph_export`), `optimize` hands the store to `pgo.optimize` as it is.

    g = graph.PoseGraph(frontend, graph.plan(max_view_num, neighbor_edge_num, loop_edge_num, H, W))
    g.commit(i, js, slam_scheduler.regress_views(frontend, feat_i, [feats[j] for j in js], [i - j == 1 for j in js], thres, H, W))

The contract is written out in include/sta_mi355.h; the yardstick is the numpy restatement tests/graph_cases.py on the float64 group
operations of tests/pgo_cases.py.  It is not pypose, which is absent wherever this runs.  Stated differences: float64 state and float64
sums (float32 there), one call per keyframe, maps kept on the device.  Kernels: csrc/graph.h.  `plan` holds every size and refusal
and needs no GPU.  The host keeps the structure only (counts, node_to_view, node_to_connected_view, view_to_node, loop_related_views):
it knows every accept / reject decision from the scheduler's read-back.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, pgo
from .sta_frontend import STAFrontend

MAX_CALL_EDGES = 16


class Plan(NamedTuple):
    max_view_num: int
    neighbor_edge_num: int
    loop_edge_num: int
    H: int
    W: int
    max_nodes: int
    max_edges: int
    max_views: int              # rows of the per-view tables and of the export buffers: max_view_num + 1 (run.py:209 checks after the step)
    chunk: int
    chunks: int
    poses_bytes: int
    edges_bytes: int
    edge_poses_bytes: int
    edge_confs_bytes: int
    pool_bytes: int             # depth + conf + intri of every node: the reference keeps the same maps, on the host
    mean_conf_bytes: int
    tables_bytes: int
    partials_bytes: int
    state_bytes: int            # the sum of the above
    export_bytes: int           # the buffers `export` gathers into (allocated once as well)


def plan(max_view_num: int = 400, neighbor_edge_num: int = 3, loop_edge_num: int = 3, H: int = 224, W: int = 224) -> Plan:
    """Every size and refusal, on the host (`sta_graph_plan`; no GPU).  max_nodes and max_edges are slam.py:33-36.  ValueError, with the
    numbers in the message, for a graph beyond `pgo.plan`'s limits (8192 nodes, 16384 edges), for H or W that is no positive multiple of
    16, and for counts that are not positive (loop_edge_num may be 0)."""
    out = (C.c_int64 * 16)()
    lib = _lib.load()
    if lib.sta_graph_plan(int(max_view_num), int(neighbor_edge_num), int(loop_edge_num), int(H), int(W), out) != 0:
        raise ValueError((lib.sta_last_error() or b"sta_graph_plan failed").decode())
    o = [int(v) for v in out]
    export = o[13] * (2 * int(H) * int(W) + 16 + 1 + 9) * 4
    return Plan(int(max_view_num), int(neighbor_edge_num), int(loop_edge_num), int(H), int(W), o[0], o[1], o[13], o[2], o[3], o[4], o[5], o[6], o[7], o[8],
                o[9], o[10], o[11], o[12], export)


class Export(NamedTuple):
    """The best node of every view, on the device: the arguments of `formats.save_data_all` and `formats.world_pointcloud`.  Views of
    the graph's own buffers: the next `export` overwrites them."""
    poses: torch.Tensor         # [N,4,4] fp32: rotation and translation of the node's Sim(3)
    scales: torch.Tensor        # [N,1]
    depths: torch.Tensor        # [N,H,W]
    confs: torch.Tensor         # [N,H,W]
    intrinsics: torch.Tensor    # [N,3,3]


class Mirror:
    """The host side of a pose graph: its structure, and every refusal of `commit`.  Needs no GPU."""

    def __init__(self, plan_: Plan):
        self.plan = plan_
        self.reset_mirror()

    def reset_mirror(self):
        self.num_nodes = self.num_edges = self.view_num = 0
        self.node_to_view: List[int] = []
        self.node_to_connected_view: List[int] = []
        self.view_to_node: Dict[int, List[int]] = {v: [] for v in range(self.plan.max_views)}
        self.loop_related_views = set()
        self.last_new_nodes = 0

    def get_view_graph(self) -> Dict[int, List[int]]:
        """slam.py:328-336"""
        return {v: [self.node_to_connected_view[u] for u in self.view_to_node[v]] for v in range(self.view_num)}

    def first(self, v: int) -> int:
        return self.view_to_node[v][0] if self.view_to_node[v] else -1

    def check(self, i: int, js: Sequence[int], acc: Sequence[bool]):
        """ValueError for what `commit` refuses: a repeated view, j >= i, more than 16 edges, a full pool or edge store, a view past the tables."""
        p, k = self.plan, len(js)
        if k != len(acc):
            raise ValueError(f"{k} candidate views and {len(acc)} results")
        if not 1 <= k <= MAX_CALL_EDGES:
            raise ValueError(f"1 .. {MAX_CALL_EDGES} candidate edges per call (got {k})")
        if len(set(js)) != k:
            raise ValueError(f"a view is a candidate of view {i} twice: {list(js)}")
        if any(j < 0 or j >= i for j in js):
            raise ValueError(f"every candidate of view {i} must lie in [0, {i}) (got {list(js)})")
        if i >= p.max_views:
            raise ValueError(f"view {i} in a graph planned for {p.max_view_num} views")
        seen, extra = {v for v in [i] + list(js) if self.view_to_node[v]}, 0                    # edges this call appends: a scale edge per node of a
        for j, a in zip(js, acc):                                                               # view that has one already, a pose edge per accepted edge
            if a:
                extra += 1 + (i in seen) + (j in seen)
                seen.update((i, j))
        if self.num_nodes + 2 * sum(acc) > p.max_nodes or self.num_edges + extra > p.max_edges:
            raise ValueError(f"the graph is full: {self.num_nodes} of {p.max_nodes} nodes and {self.num_edges} of {p.max_edges} edges before "
                             f"{sum(acc)} accepted edges of view {i}")

    def record(self, i: int, js: Sequence[int], acc: Sequence[bool]) -> List[Optional[Tuple[int, int]]]:
        """The lists after `connect_view_i_j(i, j)` for the accepted edges in order (slam.py:199-215, pose_graph.py:36-45)."""
        out: List[Optional[Tuple[int, int]]] = []
        for j, a in zip(js, acc):
            if not a:
                out.append(None)
                continue
            if i - j > self.plan.neighbor_edge_num:
                self.loop_related_views.update((i, j))
            pair = []
            for v, other in ((i, j), (j, i)):
                n = self.num_nodes
                self.node_to_view.append(v)
                self.node_to_connected_view.append(other)
                self.num_edges += 1 if self.view_to_node[v] else 0
                self.view_to_node[v].append(n)
                self.num_nodes += 1
                pair.append(n)
            self.num_edges += 1
            out.append((pair[0], pair[1]))
        if any(acc):
            self.view_num = max(self.view_num, i + 1)
        self.last_new_nodes = 2 * sum(acc)
        return out


class PoseGraph(Mirror):
    """The device arrays of one pose graph and the host mirror of its structure.  Everything is allocated here; `commit`, `export` and
    `reset` allocate nothing, copy nothing to the host and never synchronise."""

    def __init__(self, frontend: STAFrontend, plan_: Plan):
        fe, p = frontend, plan_
        self.frontend, self.plan = fe, p
        dev, f64, f32 = fe.device, torch.float64, torch.float32
        self.poses = torch.empty(p.max_nodes, 8, device=dev, dtype=f64)
        self.edges = torch.empty(p.max_edges, 2, device=dev, dtype=torch.int64)
        self.edge_poses = torch.empty(p.max_edges, 8, device=dev, dtype=f64)
        self.edge_confs = torch.empty(p.max_edges, 7, device=dev, dtype=f64)
        self.depth = torch.empty(p.max_nodes, p.H, p.W, device=dev, dtype=f32)
        self.conf = torch.empty(p.max_nodes, p.H, p.W, device=dev, dtype=f32)
        self.intri = torch.empty(p.max_nodes, 3, 3, device=dev, dtype=f32)
        self.mean_conf = torch.empty(p.max_nodes, device=dev, dtype=f64)
        self.first_node = torch.empty(p.max_views, device=dev, dtype=torch.int32)
        self.best_node = torch.empty(p.max_views, device=dev, dtype=torch.int32)
        self.best_conf = torch.empty(p.max_views, device=dev, dtype=f64)
        self._partials = torch.empty(2 * MAX_CALL_EDGES, p.chunks, 4, device=dev, dtype=f64)
        self._out = Export(torch.empty(p.max_views, 4, 4, device=dev, dtype=f32), torch.empty(p.max_views, 1, device=dev, dtype=f32),
                           torch.empty(p.max_views, p.H, p.W, device=dev, dtype=f32), torch.empty(p.max_views, p.H, p.W, device=dev, dtype=f32),
                           torch.empty(p.max_views, 3, 3, device=dev, dtype=f32))
        s = self._state = _lib.StaGraphState()
        s.max_nodes, s.max_edges, s.max_views, s.H, s.W, s.chunks = p.max_nodes, p.max_edges, p.max_views, p.H, p.W, p.chunks
        for name, t in (("poses", self.poses), ("edges", self.edges), ("edge_poses", self.edge_poses), ("edge_confs", self.edge_confs), ("depth", self.depth),
                        ("conf", self.conf), ("intri", self.intri), ("mean_conf", self.mean_conf), ("first_node", self.first_node),
                        ("best_node", self.best_node), ("best_conf", self.best_conf), ("partials", self._partials)):
            setattr(s, name, t.data_ptr())
        self.reset()

    # ------------------------------------------------------------------------------------------------------------ host mirror
    def reset(self):
        """`PoseGraphNodes.reset` + `PoseGraphEdges.reset` (one launch) and an empty mirror."""
        fe = self.frontend
        _lib.check(fe.lib.sta_graph_reset(fe._h, C.byref(self._state), fe._stream()))
        self.reset_mirror()

    # ------------------------------------------------------------------------------------------------------------ commit
    def _maps(self, t: torch.Tensor, what: str) -> torch.Tensor:
        """[2,H,W] fp32 as the scheduler returns it: contiguous, or - for a portrait frame - the transposed view of contiguous memory"""
        p = self.plan
        if t.dtype != torch.float32 or t.device != self.poses.device or t.dim() != 3:
            raise ValueError(f"{what} are fp32 [2, H, W] on {self.poses.device} (got {t.dtype} {tuple(t.shape)} on {t.device})")
        if not t.is_contiguous():
            t = t.swapaxes(1, 2)
        if tuple(t.shape) != (2, p.H, p.W) or not t.is_contiguous():
            raise ValueError(f"{what} of a graph of {p.H} x {p.W} maps have shape {tuple(t.shape)}, strides {t.stride()}")
        return t

    def commit(self, i: int, js: Sequence[int], results: Sequence) -> List[Optional[Tuple[int, int]]]:
        """`connect_view_i_j(i, j)` for the candidate edges (i, js[e]) in order, from one scheduler call's `EdgeResult`s (`.pose` [4,4],
        `.rel_pose_conf`, `.accepted`, and for an accepted edge `.confs`, `.depths` [2,H,W] and `.intri` [3,3], all on the device).  Two
        launches.  -> per edge (n_i, n_j), or None for a rejected edge, which leaves no trace.  ValueError: a repeated view, j >= i,
        more than 16 edges, a full pool or edge store, a view past the tables."""
        fe = self.frontend
        i, js, k = int(i), [int(j) for j in js], len(js)
        acc = [bool(r.accepted) for r in results]
        self.check(i, js, acc)
        first = self.first
        vp = C.c_void_p * k
        pose, depths, confs, intri, keep = vp(), vp(), vp(), vp(), []
        for e, r in enumerate(results):
            t = r.pose
            if t.dtype != torch.float32 or tuple(t.shape) != (4, 4) or not t.is_contiguous() or t.device != self.poses.device:
                raise ValueError(f"the pose of edge {e} is a contiguous fp32 [4, 4] on {self.poses.device} (got {t.dtype} {tuple(t.shape)} on {t.device})")
            pose[e] = t.data_ptr()
            keep.append(t)
            if acc[e]:
                d, c, K = self._maps(r.depths, "depths"), self._maps(r.confs, "confs"), r.intri
                if K.dtype != torch.float32 or tuple(K.shape) != (3, 3) or not K.is_contiguous() or K.device != self.poses.device:
                    raise ValueError(f"the intrinsics of edge {e} are a contiguous fp32 [3, 3] on {self.poses.device}")
                depths[e], confs[e], intri[e] = d.data_ptr(), c.data_ptr(), K.data_ptr()
                keep += [d, c, K]
        nn, ne = C.c_int(0), C.c_int(0)
        _lib.check(fe.lib.sta_graph_commit(fe._h, C.byref(self._state), self.num_nodes, self.num_edges, i, first(i), k, (C.c_int32 * k)(*js),
                                           (C.c_int32 * k)(*[first(j) for j in js]), bytes(bytearray(1 if a else 0 for a in acc)),
                                           (C.c_double * k)(*[float(r.rel_pose_conf) for r in results]), pose, depths, confs, intri,
                                           C.byref(nn), C.byref(ne), fe._stream()))
        out = self.record(i, js, acc)
        assert (self.num_nodes, self.num_edges) == (nn.value, ne.value), (self.num_nodes, self.num_edges, nn.value, ne.value)
        return out

    def call_partials(self) -> torch.Tensor:
        """The chunk partials of the most recent `commit`, float64 [new nodes, chunks, 4] = per chunk (sum c, sum w Dn Df, sum w Dn Dn,
        sum sqrt(cn cf)), zeros in the last three for a node without a scale edge: a view of the scratch the next `commit` overwrites."""
        return self._partials[:self.last_new_nodes]

    # ------------------------------------------------------------------------------------------------------------ export
    def export(self, conf_thres: Optional[float] = None, filter_outlier: bool = False, scaled: bool = False, view_num: Optional[int] = None) -> Export:
        """The best node of every view < view_num (default: every view committed so far), one launch.  scaled: depths * scale;
        filter_outlier: depths = 0 where conf < conf_thres (`get_view`, slam.py:313-320).  A portrait graph (H > W) returns the
        transposed views of its maps, as the scheduler does."""
        fe, p = self.frontend, self.plan
        N = self.view_num if view_num is None else int(view_num)
        if not 1 <= N <= p.max_views:
            raise ValueError(f"export of {N} views from a graph of {self.view_num} (at most {p.max_views})")
        missing = [v for v in range(N) if not self.view_to_node[v]]
        if missing:
            raise ValueError(f"views {missing} have no node yet")
        if filter_outlier and conf_thres is None:
            raise ValueError("filter_outlier needs conf_thres")
        o = self._out
        _lib.check(fe.lib.sta_graph_export(fe._h, C.byref(self._state), N, 1 if scaled else 0, 1 if filter_outlier else 0,
                                           float(conf_thres) if conf_thres is not None else 0.0, o.poses.data_ptr(), o.scales.data_ptr(), o.depths.data_ptr(),
                                           o.confs.data_ptr(), o.intrinsics.data_ptr(), fe._stream()))
        depths, confs = o.depths[:N], o.confs[:N]
        if p.H > p.W:
            depths, confs = depths.swapaxes(1, 2), confs.swapaxes(1, 2)
        return Export(o.poses[:N], o.scales[:N], depths, confs, o.intrinsics[:N])

    # ------------------------------------------------------------------------------------------------------------ optimise
    def optimize(self, view_num: int, window: int, **lm_kwargs):
        """`pose_graph_optimize` (slam.py:108-140): `pgo.optimize` on the first num_nodes nodes and num_edges edges of the store, with
        `pgo.window_nodes` (which keeps the reference's quirk of view ids in the node set); the result is written back and
        `loop_related_views` cleared.  The state goes in as it is: no dtype conversion.  -> the info dict with return_info=True."""
        n, E = self.num_nodes, self.num_edges
        info = None
        if n >= 1 and E >= 1:
            opt = [k for k in pgo.window_nodes(self.view_to_node, int(view_num), int(window), self.loop_related_views) if k < n]
            res = pgo.optimize(self.frontend, self.poses[:n], self.edges[:E], self.edge_poses[:E], self.edge_confs[:E], opt, **lm_kwargs)
            if lm_kwargs.get("return_info"):
                res, info = res
            self.poses[:n].copy_(res)
        self.loop_related_views = set()
        return info

    # ------------------------------------------------------------------------------------------------------------ for tests and tools
    def snapshot(self) -> dict:
        """Host copies of the used part of every array (synchronises; not for the hot path)."""
        n, E, V = self.num_nodes, self.num_edges, self.plan.max_views
        c = lambda t: t.detach().cpu().numpy().copy()
        return {"poses": c(self.poses[:n]), "edges": c(self.edges[:E]), "edge_poses": c(self.edge_poses[:E]), "edge_confs": c(self.edge_confs[:E]),
                "depth": c(self.depth[:n]), "conf": c(self.conf[:n]), "intri": c(self.intri[:n]), "mean_conf": c(self.mean_conf[:n]),
                "first_node": c(self.first_node[:V]), "best_node": c(self.best_node[:V]), "best_conf": c(self.best_conf[:V]),
                "num_nodes": n, "num_edges": E}
