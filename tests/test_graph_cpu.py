"""Host only: the plan, the refusals and the host mirror of the device-resident pose graph (vista_slam_amd.graph) against the numpy
restatement tests/graph_cases.py, and the places the new entry points have to appear in.  Nothing here touches a GPU."""
import os
import re

import numpy as np
import pytest

import graph_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the three yaml regimes: (max_view_num, neighbor_edge_num, loop_edge_num) of tumrgbd.yaml, 7scenes.yaml and default.yaml
REGIMES = {"tumrgbd": (400, 3, 2), "7scenes": (400, 2, 3), "default": (400, 3, 3)}


def test_the_modules_import():
    import vista_slam_amd.graph  # noqa: F401
    import vista_slam_amd.slam  # noqa: F401


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("hw", [(224, 224), (384, 512), (48, 64)])
def test_plan_sizes_are_the_reference_s(regime, hw):
    from vista_slam_amd import graph
    V, nb, lp = REGIMES[regime]
    H, W = hw
    p = graph.plan(V, nb, lp, H, W)
    assert (p.max_nodes, p.max_edges) == GC.sizes(V, nb, lp)
    assert p.max_views == V + 1 and p.chunks == -(-H * W // p.chunk) and p.chunk % 256 == 0
    assert p.poses_bytes == p.max_nodes * 64 and p.edges_bytes == p.max_edges * 16
    assert p.edge_poses_bytes == p.max_edges * 64 and p.edge_confs_bytes == p.max_edges * 56
    assert p.pool_bytes == p.max_nodes * (2 * H * W + 9) * 4 and p.mean_conf_bytes == p.max_nodes * 8
    assert p.tables_bytes == p.max_views * 16 and p.partials_bytes == 32 * p.chunks * 32
    assert p.state_bytes == (p.poses_bytes + p.edges_bytes + p.edge_poses_bytes + p.edge_confs_bytes + p.pool_bytes + p.mean_conf_bytes + p.tables_bytes +
                             p.partials_bytes)
    assert p.export_bytes == p.max_views * (2 * H * W + 26) * 4


def test_plan_reports_the_pool_of_the_default_configuration():
    """about 1.4 GB at 224 x 224 and 5.7 GB at 384 x 512 for 400 views of the default regime: the maps the reference keeps on the host"""
    from vista_slam_amd import graph
    assert round(graph.plan(400, 3, 3, 224, 224).pool_bytes / 1e9, 1) == 1.4
    assert round(graph.plan(400, 3, 3, 384, 512).pool_bytes / 1e9, 1) == 5.7


@pytest.mark.parametrize("args, match", [
    ((911, 3, 3, 224, 224), r"911 views .* need 8199 nodes and 11843 edges, above the optimiser's limits of 8192 and 16384"),
    ((2000, 3, 3, 224, 224), r"18000 nodes and 26000 edges"),
    ((400, 3, 3, 220, 224), r"multiples of 16 .*220 x 224"),
    ((400, 3, 3, 224, 8), r"multiples of 16 .*224 x 8"),
    ((400, 3, 3, 0, 224), r"multiples of 16"),
    ((0, 3, 3, 224, 224), r"must be positive.*\(got 0, 3, 3\)"),
    ((400, 0, 3, 224, 224), r"must be positive.*\(got 400, 0, 3\)"),
    ((400, 3, -1, 224, 224), r"loop_edge_num >= 0 \(got 400, 3, -1\)"),
])
def test_plan_refusals(args, match):
    from vista_slam_amd import graph
    with pytest.raises(ValueError, match=match):
        graph.plan(*args)


def test_plan_limits_are_pgo_s():
    from vista_slam_amd import graph, pgo
    assert graph.plan(1024, 3, 2, 32, 32).max_nodes == pgo.MAX_NODES == 8192          # exactly at the limit
    with pytest.raises(ValueError, match="8200 nodes"):
        graph.plan(1025, 3, 2, 32, 32)


def _mirror(V=8, nb=3, lp=3):
    from vista_slam_amd import graph
    return graph.Mirror(graph.plan(V, nb, lp, 16, 16))


def test_commit_refusals_on_the_host():
    m = _mirror()
    with pytest.raises(ValueError, match="twice"):
        m.check(3, [0, 1, 0], [True, True, True])
    with pytest.raises(ValueError, match=r"must lie in \[0, 3\)"):
        m.check(3, [0, 3], [True, True])
    with pytest.raises(ValueError, match=r"must lie in \[0, 3\)"):
        m.check(3, [-1], [True])
    with pytest.raises(ValueError, match="1 .. 16 candidate edges"):
        m.check(20, list(range(17)), [True] * 17)
    with pytest.raises(ValueError, match="1 .. 16 candidate edges"):
        m.check(2, [], [])
    with pytest.raises(ValueError, match="2 candidate views and 1 results"):
        m.check(2, [0, 1], [True])
    with pytest.raises(ValueError, match="view 9 in a graph planned for 8 views"):
        m.check(9, [8], [True])
    m.check(8, [7], [True])                               # one view past max_view_num is held (run.py:209 checks after the step)
    assert m.num_nodes == 0 and m.num_edges == 0          # a check records nothing


def test_a_full_pool_and_a_full_edge_store_are_refused():
    from vista_slam_amd import graph
    m = graph.Mirror(graph.plan(2, 1, 0, 16, 16))         # 4 nodes, 6 edges, views 0 .. 2
    assert (m.plan.max_nodes, m.plan.max_edges, m.plan.max_views) == (4, 6, 3)
    m.record(1, [0], [True])
    assert (m.num_nodes, m.num_edges) == (2, 1)
    with pytest.raises(ValueError, match="the graph is full: 2 of 4 nodes and 1 of 6 edges before 2 accepted edges of view 2"):
        m.check(2, [0, 1], [True, True])                  # 4 more nodes
    m.check(2, [0, 1], [False, True])                     # a rejected edge needs no room
    m.num_edges = 5                                       # as if four more edges were stored: a scale edge and a pose edge do not fit
    with pytest.raises(ValueError, match="2 of 4 nodes and 5 of 6 edges"):
        m.check(2, [1], [True])
    m.num_edges = 4
    m.check(2, [1], [True])
    m.record(2, [1], [True])
    assert (m.num_nodes, m.num_edges) == (4, 6)
    with pytest.raises(ValueError, match="4 of 4 nodes"):
        m.check(2, [0], [True])


@pytest.mark.parametrize("name", GC.SCRIPTS)
def test_host_mirror_equals_the_restatement(name):
    """The mirror after a scripted sequence of decisions holds the restatement's lists and counts."""
    from vista_slam_amd import graph
    seq = GC.scripted(name, 16, 16)
    ref = GC.replay(seq)
    m = graph.Mirror(graph.plan(8, 3, 3, 16, 16))
    pairs = []
    for i, js, edges in seq:
        acc = [e.accepted for e in edges]
        m.check(i, js, acc)
        pairs += m.record(i, js, acc)
    n = ref.num_nodes
    assert (m.num_nodes, m.num_edges) == (ref.num_nodes, ref.num_edges)
    assert m.node_to_view == ref.node_to_view[:n] and m.node_to_connected_view == ref.node_to_connected_view[:n]
    V = seq[-1][0] + 1
    assert m.view_num == V
    assert all(m.view_to_node[v] == ref.view_to_node[v] for v in range(m.plan.max_views))
    assert m.loop_related_views == ref.loop_related_views
    assert m.get_view_graph() == ref.get_view_graph(V)
    got = [p for p in pairs if p is not None]
    want = [(int(a), int(b)) for a, b in ref.edges[:ref.num_edges] if ref.node_to_view[a] != ref.node_to_view[b]]
    assert got == want                                    # the pose edges are the (n_i, n_j) the mirror hands back
    assert sum(p is None for p in pairs) == sum(not e.accepted for _, _, es in seq for e in es)
    m.reset_mirror()
    assert (m.num_nodes, m.num_edges, m.view_num, m.node_to_view, m.loop_related_views) == (0, 0, 0, [], set())


def test_scripts_cover_what_they_claim():
    ref = GC.replay(GC.scripted("keyframe 2", 16, 16))
    assert ref.view_to_node[2] == [2, 4] and ref.edges[3].tolist() == [4, 2]            # the scale edge against a node of the same call
    ref = GC.replay(GC.scripted("equal means", 16, 16))
    assert len(ref.view_to_node[0]) == 3 and len({ref.mean_conf[n] for n in ref.view_to_node[0]}) == 1 and ref.view_to_best_node[0][0] == ref.view_to_node[0][0]
    ref = GC.replay(GC.scripted("view reused", 16, 16))
    assert len(ref.view_to_node[0]) == 5
    seq = GC.scripted("k = 6", 16, 16)
    assert len(seq[-1][1]) == 6 and ref.num_nodes <= 72
    ref = GC.replay(seq)
    assert ref.loop_related_views == {7, 0, 1}
    branches = set()
    for name in GC.SCRIPTS:                               # every branch of the quaternion rule is met by the scripts' poses
        for _, _, es in GC.scripted(name, 16, 16):
            for e in es:
                M = e.pose.astype(np.float64)
                tr = M[0, 0] + M[1, 1] + M[2, 2]
                branches.add(0 if tr > 0 else 1 if (M[0, 0] > M[1, 1] and M[0, 0] > M[2, 2]) else 2 if M[1, 1] > M[2, 2] else 3)
    assert branches == {0, 1, 2, 3}


def test_mat_to_sim3_inverts_the_matrix():
    import pgo_cases as P
    rng = np.random.RandomState(5)
    for _ in range(50):
        M = GC.random_pose(rng)
        T = GC.mat_to_sim3(M)
        assert T[6] >= 0 and T[7] == 1.0 and abs(np.linalg.norm(T[3:7]) - 1) < 1e-15
        assert np.abs(P.matrix(T) - M.astype(np.float64)).max() < 1e-6          # the fp32 matrix is orthogonal to fp32 rounding only


def test_header_and_bindings_declare_the_entry_points():
    from vista_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sta_mi355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("sta_graph_plan", "sta_graph_reset", "sta_graph_commit", "sta_graph_export"):
        assert re.search(r"STA_API int %s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    fields = re.search(r"typedef struct sta_graph_state \{(.*?)\} sta_graph_state;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", fields)
    assert names == [f for f, _ in _lib.StaGraphState._fields_]
    assert "tests/graph_cases.py" in hdr and "NOT pypose" in hdr          # the contract names its yardstick


def test_graph_h_has_no_fp16_plane_writer_and_no_float_atomic():
    src = open(os.path.join(ROOT, "vista_slam_amd", "csrc", "graph.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\bf16\b|__half|_Float16|to_f16_sat|split_f16", code)
    assert not re.search(r"atomic", code, flags=re.I)
