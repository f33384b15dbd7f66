"""The pose-graph state of `OnlineSLAM` restated in numpy, statement by statement: `PoseGraphNodes.add_node`, `PoseGraphEdges.add_edge`
(vista_slam/pose_graph.py:5-54), `connect_view_i_j` (slam.py:191-241), `get_view` (:299-326) and the gather of `save_data_all`
(:353-379).  The group operations are the float64 ones of tests/pgo_cases.py - NOT pypose, which is absent wherever this suite runs.
This is the yardstick of vista_slam_amd.graph (csrc/graph.h): float64 state and float64 sums where the reference has float32 (the
stated differences of include/sta_mi355.h).  TEST INFRASTRUCTURE: no product import.

The sums are taken by numpy in its own (pairwise) order; the device takes them in a fixed tree.  Two float64 sums of N terms in
different orders differ by at most N * 2^-53 of the sum of the absolute terms (N <= 3840 here: 4.3e-13) and by about sqrt(N) * 2^-53
(7e-15) typically; the tests compare at 1e-12 of that sum, the bar tests/test_flow_gpu.py and tests/test_loop_gpu.py use."""
import numpy as np

import pgo_cases as P

F64 = np.float64
SUM_TOL = 1e-12
ID_POSE_CONF = 2.0                      # pose_graph.py:11
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1, 1], F64)


def sizes(max_view_num, neighbor_edge_num, loop_edge_num):
    """slam.py:33-36"""
    max_nodes = max_view_num * (neighbor_edge_num * 2 + loop_edge_num)
    scale_edges_num = neighbor_edge_num * 2 + loop_edge_num - 1
    pose_edges_num = (neighbor_edge_num * 2 + loop_edge_num) // 2 + 1
    max_edges = max_view_num * (scale_edges_num + pose_edges_num)
    return max_nodes, max_edges


def mat_to_sim3(pose):
    """pp.mat2SE3 by the branch rule of sta_mat_to_se3 (Shepperd, the largest component first, qw >= 0), in float64, scale 1"""
    M = np.asarray(pose, F64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (M[r, c] for r in range(3) for c in range(3))
    tr = m00 + m11 + m22
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2.0
        qw, qx, qy, qz = 0.25 * s, (m21 - m12) / s, (m02 - m20) / s, (m10 - m01) / s
    elif m00 > m11 and m00 > m22:
        s = np.sqrt(1.0 + m00 - m11 - m22) * 2.0
        qw, qx, qy, qz = (m21 - m12) / s, 0.25 * s, (m01 + m10) / s, (m02 + m20) / s
    elif m11 > m22:
        s = np.sqrt(1.0 + m11 - m00 - m22) * 2.0
        qw, qx, qy, qz = (m02 - m20) / s, (m01 + m10) / s, 0.25 * s, (m12 + m21) / s
    else:
        s = np.sqrt(1.0 + m22 - m00 - m11) * 2.0
        qw, qx, qy, qz = (m10 - m01) / s, (m02 + m20) / s, (m12 + m21) / s, 0.25 * s
    nrm = (-1.0 if qw < 0 else 1.0) / np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
    return np.array([M[0, 3], M[1, 3], M[2, 3], qx * nrm, qy * nrm, qz * nrm, qw * nrm, 1.0], F64)


def scale_sums(depth, depth_other, conf, conf_other):
    """The three sums of slam.py:224-227 (estimate_scale_with_depth_and_confidence(depth, depth_other, conf, conf_other) and the
    sqrt-mean confidence), every term in float64 from the fp32 inputs -> (sums [3], the sums of the absolute terms [3])."""
    Di, Dj = np.asarray(depth, np.float32).astype(F64).ravel(), np.asarray(depth_other, np.float32).astype(F64).ravel()
    ci, cj = np.asarray(conf, np.float32).astype(F64).ravel(), np.asarray(conf_other, np.float32).astype(F64).ravel()
    cc = ci * cj
    w = np.maximum(cc, 1e-6)
    num, den, sq = (w * Di) * Dj, (w * Di) * Di, np.sqrt(cc)
    return np.array([num.sum(), den.sum(), sq.sum()]), np.array([np.abs(num).sum(), den.sum(), sq.sum()])


class RefGraph:
    """PoseGraphNodes + PoseGraphEdges + the part of OnlineSLAM that writes them."""

    def __init__(self, max_nodes, max_edges, neighbor_edge_num=3):
        self.max_nodes, self.max_edges, self.neighbor_edge_num = max_nodes, max_edges, neighbor_edge_num
        self.reset()

    def reset(self):
        self.poses = np.tile(IDENTITY, (self.max_nodes, 1))                  # pose_graph.py:48
        self.node_to_view = [-1] * self.max_nodes
        self.node_to_connected_view = [-1] * self.max_nodes
        self.view_to_node = {v: [] for v in range(self.max_nodes)}
        self.view_to_best_node = {v: (-1, -100) for v in range(self.max_nodes)}
        self.pcl = []
        self.num_nodes = 0
        self.edge_poses = np.tile(IDENTITY, (self.max_edges, 1))             # pose_graph.py:20-23
        self.edges = -np.ones((self.max_edges, 2), np.int64)
        self.confs = np.ones((self.max_edges, 7), F64)
        self.num_edges = 0
        self.loop_related_views = set()
        self.mean_conf = []
        self.node_sums = []             # per node: None or (sums [3], abs sums [3]) of its scale edge
        self.conf_sums = []             # per node: the sum of its confidence map

    def add_node(self, view_id, depth, conf, intri, connected_view):
        n_idx = self.num_nodes
        self.pcl.append((np.asarray(depth, np.float32).copy(), np.asarray(conf, np.float32).copy(), np.asarray(intri, np.float32).copy()))
        self.node_to_view[n_idx] = view_id
        self.node_to_connected_view[n_idx] = connected_view
        self.view_to_node[view_id].append(n_idx)
        total = float(np.asarray(conf, np.float32).astype(F64).sum())
        mean_conf = total / np.asarray(conf).size
        self.conf_sums.append(total)
        self.mean_conf.append(mean_conf)
        self.node_sums.append(None)
        if mean_conf > self.view_to_best_node[view_id][1]:
            self.view_to_best_node[view_id] = (n_idx, mean_conf)
        self.num_nodes += 1
        return n_idx

    def add_edge(self, i, j, T, conf):
        self.edges[self.num_edges] = (i, j)
        self.edge_poses[self.num_edges] = T
        self.confs[self.num_edges] = conf
        self.num_edges += 1

    def connect_view_i_j(self, i, j, pose, rel_pose_conf, confs, intri, depths):
        """slam.py:199-241 for an ACCEPTED edge (a rejected one returns before any of it)"""
        assert i > j
        if i - j > self.neighbor_edge_num:
            self.loop_related_views.add(i)
            self.loop_related_views.add(j)
        sim3_ij = mat_to_sim3(pose)
        node_idx_of_ij = {i: None, j: None}
        view_i_is_new = True
        for v, depth, pcl_conf, v_other in zip([i, j], depths, confs, [j, i]):
            n_idx = self.add_node(view_id=v, depth=depth, conf=pcl_conf, intri=intri, connected_view=v_other)
            node_idx_of_ij[v] = n_idx
            if len(self.view_to_node[v]) > 1:
                if v == i:
                    view_i_is_new = False
                n_idx_other = self.view_to_node[v][0]
                depth_other, pcl_conf_other, _ = self.pcl[n_idx_other]
                sums, asums = scale_sums(depth, depth_other, pcl_conf, pcl_conf_other)
                self.node_sums[n_idx] = (sums, asums)
                scale = sums[0] / sums[1]
                scale_conf = sums[2] / np.asarray(pcl_conf).size
                edge_weight = np.array([ID_POSE_CONF] * 6 + [scale_conf], F64)
                sim3 = np.array([0, 0, 0, 0, 0, 0, 1, scale], F64)
                self.add_edge(n_idx, n_idx_other, sim3, edge_weight)
                self.poses[n_idx] = P.mul(self.poses[n_idx_other], sim3)
        if view_i_is_new:
            self.poses[node_idx_of_ij[i]] = P.mul(self.poses[node_idx_of_ij[j]], sim3_ij)
        self.add_edge(node_idx_of_ij[i], node_idx_of_ij[j], sim3_ij, float(rel_pose_conf))
        return node_idx_of_ij[i], node_idx_of_ij[j]

    # ------------------------------------------------------------------------------------------------------------ readers
    def get_view_graph(self, view_num):
        return {v: [self.node_to_connected_view[u] for u in self.view_to_node[v]] for v in range(view_num)}

    def get_view(self, v, conf_thres, filter_outlier=True):
        """slam.py:299-326 -> (pose [4,4], depth [H,W], intri [3,3]) in fp32 like the reference's"""
        best_node = self.view_to_best_node[v][0]
        T = self.poses[best_node]
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = P.rot(T[3:7]).astype(np.float32)
        pose[:3, 3] = T[:3].astype(np.float32)
        depth = self.pcl[best_node][0] * np.float32(T[7])
        if filter_outlier:
            depth[self.pcl[best_node][1] < np.float32(conf_thres)] = 0.0
        return pose, depth, self.pcl[best_node][2]

    def gather(self, view_num):
        """slam.py:353-379 -> poses [N,4,4], scales [N,1], depths, confs [N,H,W], intrinsics [N,3,3], fp32"""
        poses, scales, depths, confs, intrinsics = [], [], [], [], []
        for v in range(view_num):
            best_node = self.view_to_best_node[v][0]
            T = self.poses[best_node]
            pose = np.eye(4, dtype=np.float32)
            pose[:3, :3] = P.rot(T[3:7]).astype(np.float32)
            pose[:3, 3] = T[:3].astype(np.float32)
            poses.append(pose)
            scales.append(np.array([T[7]], np.float32))
            depths.append(self.pcl[best_node][0])
            confs.append(self.pcl[best_node][1])
            intrinsics.append(self.pcl[best_node][2])
        return np.stack(poses), np.stack(scales), np.stack(depths), np.stack(confs), np.stack(intrinsics)

    def tables(self, n_views):
        first = np.array([self.view_to_node[v][0] if self.view_to_node[v] else -1 for v in range(n_views)], np.int32)
        best = np.array([self.view_to_best_node[v][0] for v in range(n_views)], np.int32)
        return first, best


# ---------------------------------------------------------------------------------------------------------------- inputs
class Edge:
    """What the scheduler returns for one edge (slam_scheduler.EdgeResult's fields), as numpy"""

    def __init__(self, pose, rel_pose_conf, accepted, confs=None, intri=None, depths=None):
        self.pose, self.rel_pose_conf, self.accepted = pose, rel_pose_conf, accepted
        self.confs, self.intri, self.depths = confs, intri, depths


def random_pose(rng):
    """a rigid 4x4 in fp32 (rotation of any angle, so every branch of the quaternion rule is met over a sequence)"""
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    M = np.eye(4)
    M[:3, :3] = P.rot(np.array([q[0], q[1], q[2], q[3]]))
    M[:3, 3] = rng.randn(3)
    return M.astype(np.float32)


def random_edge(rng, H, W, accepted=True, rel_pose_conf=None, conf_mean=None):
    """positive confidences (some below 1e-3, so that the clamp of w at 1e-6 is met), depths of both signs"""
    pose = random_pose(rng)
    c = float(rng.uniform(0.5, 3.0)) if rel_pose_conf is None else rel_pose_conf
    if not accepted:
        return Edge(pose, c, False)
    confs = np.exp(rng.randn(2, H, W) * 1.5).astype(np.float32)
    confs[rng.rand(2, H, W) < 0.05] *= np.float32(1e-4)
    if conf_mean is not None:               # a constant map: its float64 mean is exact whatever the order of the sum
        confs[0] = np.float32(conf_mean)
        confs[1] = np.float32(conf_mean)
    depths = (rng.randn(2, H, W) * 2.0 + 1.0).astype(np.float32)
    intri = np.array([[W * 0.9, 0, W / 2], [0, W * 0.9, H / 2], [0, 0, 1]], np.float32) + rng.rand(3, 3).astype(np.float32)
    return Edge(pose, c, True, confs, intri, depths)


def scripted(name, H, W, seed=0):
    """The sequences of tests/test_graph_gpu.py: [(i, js, [Edge])] per keyframe, in order."""
    rng = np.random.RandomState(seed + 17 * H + W)
    E = lambda **kw: random_edge(rng, H, W, **kw)
    R = lambda: random_edge(rng, H, W, accepted=False)
    if name == "keyframe 1":                        # both views new
        return [(1, [0], [E()])]
    if name == "keyframe 2":                        # its second accepted edge scales against the node its first edge made in the same call
        return [(1, [0], [E()]), (2, [0, 1], [E(), E()])]
    if name == "rejected between":                  # a rejected edge between two accepted ones
        return [(1, [0], [E()]), (2, [0, 1], [E(), E()]), (3, [0, 1, 2], [E(), R(), E()])]
    if name == "non-adjacent rejected":             # all non-adjacent edges rejected
        return [(1, [0], [E()]), (2, [0, 1], [R(), E()]), (3, [0, 1, 2], [R(), R(), E()]), (4, [1, 2, 3], [R(), R(), E()])]
    if name == "view reused":                       # view 0 is a candidate of five keyframes
        return [(i, [0] + ([i - 1] if i > 1 else []), [E() for _ in range(1 + (i > 1))]) for i in range(1, 6)]
    if name == "equal means":                       # the three nodes of view 0 have the same mean confidence: the earliest stays best
        return [(1, [0], [E(conf_mean=1.25)]), (2, [0, 1], [E(conf_mean=1.25), E()]), (3, [0, 2], [E(conf_mean=1.25), E()])]
    if name == "k = 6":
        seq = [(i, list(range(max(0, i - 3), i)), None) for i in range(1, 7)]
        seq = [(i, js, [E() for _ in js]) for i, js, _ in seq]
        return seq + [(7, [4, 5, 6, 0, 2, 1], [E(), E(), E(), E(), R(), E()])]
    raise KeyError(name)


SCRIPTS = ["keyframe 1", "keyframe 2", "rejected between", "non-adjacent rejected", "view reused", "equal means", "k = 6"]
SIZES = [(16, 16), (16, 48), (48, 64), (48, 80)]


def replay(seq, max_nodes=64, max_edges=128, neighbor_edge_num=3):
    """The restatement fed with a scripted sequence -> RefGraph"""
    g = RefGraph(max_nodes, max_edges, neighbor_edge_num)
    for i, js, edges in seq:
        for j, e in zip(js, edges):
            if e.accepted:
                g.connect_view_i_j(i, j, e.pose, e.rel_pose_conf, e.confs, e.intri, e.depths)
    return g


# ---------------------------------------------------------------------------------------------------------------- comparison
def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    assert a.shape == b.shape and np.isfinite(a).all()
    return float((np.abs(a - b).max(1) / (1 + np.abs(b).max(1))).max()) if a.size else 0.0


def check_state(g, ref, n_views):
    """A `vista_slam_amd.graph.PoseGraph` (its snapshot and its host mirror) against the restatement -> (worst pose error, worst edge measurement error)"""
    s = g.snapshot()
    n, E, hw = ref.num_nodes, ref.num_edges, g.plan.H * g.plan.W
    assert (s["num_nodes"], s["num_edges"]) == (n, E)
    assert np.array_equal(s["edges"], ref.edges[:E])
    first, best = ref.tables(g.plan.max_views)
    assert np.array_equal(s["first_node"], first) and np.array_equal(s["best_node"], best)
    assert g.node_to_view == ref.node_to_view[:n] and g.node_to_connected_view == ref.node_to_connected_view[:n]
    assert all(g.view_to_node[v] == ref.view_to_node[v] for v in range(g.plan.max_views))
    assert g.view_num == n_views and g.get_view_graph() == ref.get_view_graph(n_views)
    assert g.loop_related_views == ref.loop_related_views
    assert np.array_equal(s["depth"], np.stack([p[0] for p in ref.pcl])) and np.array_equal(s["conf"], np.stack([p[1] for p in ref.pcl]))
    assert np.array_equal(s["intri"], np.stack([p[2] for p in ref.pcl]))
    for k in range(n):
        assert abs(s["mean_conf"][k] - ref.mean_conf[k]) <= SUM_TOL * ref.mean_conf[k]
    for v in range(g.plan.max_views):
        assert s["best_conf"][v] == (s["mean_conf"][best[v]] if best[v] >= 0 else -100.0)
    for e in range(E):
        a, b = ref.edges[e]
        if ref.node_to_view[a] == ref.node_to_view[b]:                   # a scale edge
            sums, mag = ref.node_sums[a]
            assert np.array_equal(s["edge_poses"][e, :7], IDENTITY[:7]) and np.array_equal(s["edge_confs"][e, :6], np.full(6, 2.0))
            # both sums are within SUM_TOL of their absolute terms: the ratio is within SUM_TOL (|num|_1 + |num|) / den
            assert abs(s["edge_poses"][e, 7] - sums[0] / sums[1]) <= SUM_TOL * (mag[0] + abs(sums[0])) / sums[1]
            assert abs(s["edge_confs"][e, 6] - sums[2] / hw) <= SUM_TOL * sums[2] / hw
        else:
            assert np.array_equal(s["edge_confs"][e], ref.confs[e])
    e_pose, e_edge = rel(P.matrix(s["poses"]), P.matrix(ref.poses[:n])), rel(P.matrix(s["edge_poses"]), P.matrix(ref.edge_poses[:E]))
    assert e_pose <= P.TOL_EDGE and e_edge <= P.TOL_EDGE, (e_pose, e_edge)
    return e_pose, e_edge
