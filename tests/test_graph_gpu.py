"""GPU: the device-resident pose graph (csrc/graph.h: sta_graph_reset / sta_graph_commit / sta_graph_export, vista_slam_amd.graph)
against the numpy restatement of the reference's statements (tests/graph_cases.py; not pypose).  Index arrays, tables, counts and the
gathered maps are compared with array_equal; the float64 sums at 1e-12 of the sum of their absolute terms (graph_cases.SUM_TOL: two
float64 sums of <= 3840 terms in different orders); node poses and edge measurements, as matrices, at pgo_cases.TOL_EDGE relative to
1 + max|row|.  Map sizes: 16x16 (one vector pass of one wave), 16x48 (less than a chunk, three of the four waves), 48x64 (a chunk and
a half), 48x80 (a chunk and a partial one of 7 waves' worth).  Inputs: positive confidences, some tiny enough for the 1e-6 clamp,
depths of both signs."""
import functools

import numpy as np
import pytest

import graph_cases as GC
import pgo_cases as P

pytestmark = pytest.mark.gpu

VIEWS, NB, LP = 8, 3, 3


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


def upload(seq):
    """[(i, js, [Edge numpy])] -> the same with device `EdgeResult`s"""
    from vista_slam_amd.slam_scheduler import EdgeResult
    out = []
    for i, js, edges in seq:
        rs = [EdgeResult(_up(e.pose), e.rel_pose_conf, e.accepted, *((_up(e.confs), _up(e.intri), _up(e.depths)) if e.accepted else ())) for e in edges]
        out.append((i, js, rs))
    return out


@functools.lru_cache(maxsize=None)
def case(name, H, W):
    """the scripted sequence and the restatement's graph after it: computed once, shared, never changed"""
    seq = GC.scripted(name, H, W)
    return seq, GC.replay(seq, *GC.sizes(VIEWS, NB, LP), NB)


def new_graph(m, H, W):
    from vista_slam_amd import graph
    return graph.PoseGraph(m, graph.plan(VIEWS, NB, LP, H, W))


def seq_sum(x):
    """sum over axis 0 in ascending order from 0.0, as graph_link_kernel takes it"""
    acc = np.zeros(x.shape[1:], np.float64)
    for row in x:
        acc = acc + row
    return acc


def run(g, dev_seq, ref=None, per_edge=False):
    """commit the sequence; with `ref`: after every call the chunk partials against the restatement's sums"""
    worst = 0.0
    for i, js, rs in dev_seq:
        calls = [(i, [j], [r]) for j, r in zip(js, rs)] if per_edge else [(i, js, rs)]
        for ci, cjs, crs in calls:
            n0 = g.num_nodes
            g.commit(ci, cjs, crs)
            if ref is None:
                continue
            part = g.call_partials().cpu().numpy()
            assert part.shape == (g.num_nodes - n0, g.plan.chunks, 4)
            hw = g.plan.H * g.plan.W
            for s in range(part.shape[0]):
                node, sums = n0 + s, seq_sum(part[s])
                want = [ref.conf_sums[node]] + (list(ref.node_sums[node][0]) if ref.node_sums[node] else [0.0, 0.0, 0.0])
                mag = [ref.conf_sums[node]] + (list(ref.node_sums[node][1]) if ref.node_sums[node] else [0.0, 0.0, 0.0])
                for q in range(4):
                    err = abs(sums[q] - want[q])
                    assert err <= GC.SUM_TOL * mag[q], (node, q, sums[q], want[q], mag[q])
                    worst = max(worst, err / mag[q] if mag[q] else 0.0)
                assert float(g.mean_conf[node]) == sums[0] / hw          # the link kernel sums the chunks in ascending order
    return worst


check_state = GC.check_state


@pytest.mark.parametrize("hw", GC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", GC.SCRIPTS)
def test_commit_against_the_restatement(m, name, hw):
    H, W = hw
    seq, ref = case(name, H, W)
    g = new_graph(m, H, W)
    worst = run(g, upload(seq), ref)
    e_pose, e_edge = check_state(g, ref, seq[-1][0] + 1)
    print(f"[graph] {name} {H}x{W}: nodes={ref.num_nodes} edges={ref.num_edges} sums={worst:.1e} poses={e_pose:.1e} edge_poses={e_edge:.1e}")


def test_reset_state_is_the_reference_s(m):
    g = new_graph(m, 16, 16)
    run(g, upload(case("keyframe 2", 16, 16)[0]))
    g.reset()
    ref = GC.RefGraph(*GC.sizes(VIEWS, NB, LP), NB)
    assert np.array_equal(g.poses.cpu().numpy(), ref.poses) and np.array_equal(g.edges.cpu().numpy(), ref.edges)
    assert np.array_equal(g.edge_poses.cpu().numpy(), ref.edge_poses) and np.array_equal(g.edge_confs.cpu().numpy(), ref.confs)
    assert (g.first_node.cpu().numpy() == -1).all() and (g.best_node.cpu().numpy() == -1).all() and (g.best_conf.cpu().numpy() == -100.0).all()
    assert (g.num_nodes, g.num_edges, g.view_num) == (0, 0, 0)


@pytest.mark.parametrize("name, hw", [("k = 6", (48, 80)), ("rejected between", (16, 48)), ("keyframe 2", (48, 64))])
def test_one_call_one_call_per_edge_and_after_reset_are_bit_identical(m, name, hw):
    H, W = hw
    dev = upload(case(name, H, W)[0])
    g = new_graph(m, H, W)
    run(g, dev)
    a = g.snapshot()
    g.reset()
    run(g, dev)
    b = g.snapshot()
    h = new_graph(m, H, W)
    run(h, dev, per_edge=True)
    c = h.snapshot()
    for key in a:
        assert np.array_equal(a[key], b[key]), ("after reset", key)
        assert np.array_equal(a[key], c[key]), ("one call per edge", key)
    assert (g.node_to_view, g.view_to_node, g.loop_related_views) == (h.node_to_view, h.view_to_node, h.loop_related_views)


def test_commit_and_export_neither_allocate_nor_synchronise(m):
    import torch
    H, W = 48, 80
    dev = upload(case("k = 6", H, W)[0])
    g = new_graph(m, H, W)
    run(g, dev[:2])
    g.export()
    torch.cuda.synchronize()
    before = (m.alloc_stats(), torch.cuda.memory_allocated())
    run(g, dev[2:])
    mid = (m.alloc_stats(), torch.cuda.memory_allocated())
    ex = g.export(conf_thres=1.0, filter_outlier=True, scaled=True)
    after = (m.alloc_stats(), torch.cuda.memory_allocated())
    assert before == mid == after
    assert ex.depths.shape == (8, H, W)
    g.reset()
    assert (m.alloc_stats(), torch.cuda.memory_allocated()) == before


@pytest.mark.parametrize("hw", [(16, 48), (48, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_export_against_the_restatement_and_through_save_data_all(m, hw, tmp_path):
    import torch
    from vista_slam_amd import formats
    H, W = hw
    seq, ref = case("k = 6", H, W)
    g = new_graph(m, H, W)
    run(g, upload(seq))
    N = 8
    ex = g.export()
    poses, scales, depths, confs, intri = (t.cpu().numpy().copy() for t in ex)
    rp, rs, rd, rc, rk = ref.gather(N)
    assert poses.dtype == scales.dtype == depths.dtype == np.float32 and poses.shape == (N, 4, 4) and scales.shape == (N, 1)
    assert np.array_equal(depths, rd) and np.array_equal(confs, rc) and np.array_equal(intri, rk)
    # the fp32 matrices: TOL_EDGE on the float64 state behind them, and half an fp32 ulp for the output's own rounding
    T64 = np.stack([ref.poses[ref.view_to_best_node[v][0]] for v in range(N)])
    M64 = np.zeros((N, 4, 4))
    M64[:, :3, :3], M64[:, :3, 3], M64[:, 3, 3] = P.rot(T64[:, 3:7]), T64[:, :3], 1.0
    bound = P.TOL_EDGE * (1 + np.abs(M64).reshape(N, -1).max(1))[:, None, None] + 2.0 ** -24 * np.abs(M64)
    assert (np.abs(poses.astype(np.float64) - M64) <= bound).all() and np.array_equal(poses[:, 3], np.tile([0, 0, 0, 1], (N, 1)).astype(np.float32))
    assert (np.abs(scales[:, 0].astype(np.float64) - T64[:, 7]) <= P.TOL_EDGE * (1 + np.abs(T64[:, 7])) + 2.0 ** -24 * np.abs(T64[:, 7])).all()
    assert rp.shape == poses.shape and rs.shape == scales.shape
    # get_view: depth * scale (fp32, the exported scale), then the outliers zeroed
    thres = float(np.median(rc))
    for filt in (False, True):
        sd = g.export(conf_thres=thres, filter_outlier=filt, scaled=True).depths.cpu().numpy()
        want = rd * scales[:, :, None]
        if filt:
            want[rc < np.float32(thres)] = 0.0
            assert (want == 0).sum() > 0.4 * want.size
        assert np.array_equal(sd, want)
    for v in (0, N - 1):                                                  # ... which is the restatement's get_view up to the scale's own rounding
        _pose, depth, K = ref.get_view(v, thres, True)
        assert np.abs(sd[v] - depth).max() <= 2.0 ** -22 * np.abs(depth).max() and np.array_equal(K, intri[v])
    unfiltered = g.export(conf_thres=thres, filter_outlier=True).depths.cpu().numpy()
    assert np.array_equal(unfiltered != 0, (rc >= np.float32(thres)) & (rd != 0))
    with pytest.raises(ValueError, match="needs conf_thres"):
        g.export(filter_outlier=True)
    with pytest.raises(ValueError, match="export of 10 views"):
        g.export(view_num=10)
    # the files
    ex = g.export()
    imgs = torch.zeros(N, 3, H, W, device="cuda")
    formats.save_data_all(m, str(tmp_path), poses=ex.poses, scales=ex.scales, depths=ex.depths, confs=ex.confs, intrinsics=ex.intrinsics, imgs=imgs,
                          conf_thres=thres, view_graph=g.get_view_graph(), loop_min_dist=3, view_names=[str(v) for v in range(N)])
    assert np.array_equal(np.load(tmp_path / "trajectory.npy"), poses) and np.array_equal(np.load(tmp_path / "scales.npy"), scales)
    assert np.array_equal(np.load(tmp_path / "depths.npy"), rd) and np.array_equal(np.load(tmp_path / "intrinsics.npy"), rk)
    z = np.load(tmp_path / "confs.npz")
    assert np.array_equal(z["confs"], rc) and float(z["thres"]) == thres
    vg = np.load(tmp_path / "view_graph.npz", allow_pickle=True)
    assert vg["view_graph"].item() == ref.get_view_graph(N)
    assert len(formats.read_ply(str(tmp_path / "pointcloud.ply"))) == int((rc > np.float32(thres)).sum())


def test_export_refuses_a_view_without_a_node(m):
    g = new_graph(m, 16, 16)
    run(g, upload(case("keyframe 1", 16, 16)[0]))
    assert g.export().poses.shape == (2, 4, 4)
    with pytest.raises(ValueError, match=r"views \[2\] have no node"):
        g.export(view_num=3)


def test_portrait_maps_are_the_transposed_views_the_scheduler_returns(m):
    """A portrait frame's maps arrive as transposed views of contiguous [2, H, W] memory (H > W); the pool keeps the memory order and
    `export` hands the same views back."""
    H, W = 48, 32
    seq, ref = case("keyframe 2", H, W)
    dev = upload(seq)
    for _i, _js, rs in dev:
        for r in rs:
            r.confs, r.depths = r.confs.swapaxes(1, 2), r.depths.swapaxes(1, 2)
            assert not r.confs.is_contiguous() and r.confs.shape == (2, W, H)
    g = new_graph(m, H, W)
    run(g, dev, ref)
    check_state(g, ref, 3)
    ex = g.export()
    assert ex.depths.shape == (3, W, H) and np.array_equal(ex.depths.cpu().numpy(), ref.gather(3)[2].swapaxes(1, 2))
    with pytest.raises(ValueError, match="maps have shape"):
        new_graph(m, 48, 64).commit(1, [0], dev[0][2])


def test_the_library_refuses_what_the_host_check_refuses(m):
    """sta_graph_commit itself (the C ABI) refuses a repeated view, j >= i and k > 16: the Python check is not the only one."""
    import ctypes as C
    g = new_graph(m, 16, 16)
    dev = upload(case("keyframe 2", 16, 16)[0])
    r = dev[1][2]

    def call(i, js, rs):
        k = len(js)
        vp = C.c_void_p * k
        nn, ne = C.c_int(0), C.c_int(0)
        return m.lib.sta_graph_commit(m._h, C.byref(g._state), 0, 0, i, -1, k, (C.c_int32 * k)(*js), (C.c_int32 * k)(*[-1] * k), bytes([1] * k),
                                      (C.c_double * k)(*[1.0] * k), vp(*[x.pose.data_ptr() for x in rs]), vp(*[x.depths.data_ptr() for x in rs]),
                                      vp(*[x.confs.data_ptr() for x in rs]), vp(*[x.intri.data_ptr() for x in rs]), C.byref(nn), C.byref(ne), m._stream())
    for i, js, rs, msg in [(2, [0, 0], r, b"twice"), (2, [0, 2], r, b"j must lie in [0, i)"), (20, list(range(17)), r * 9, b"1 .. 16 candidate edges"),
                           (9, [0], r[:1], b"view i must lie in [1, 9)")]:
        assert call(i, js, rs[:len(js)]) != 0
        assert msg in m.lib.sta_last_error(), m.lib.sta_last_error()
    assert g.snapshot()["num_nodes"] == 0 and (g.first_node.cpu().numpy() == -1).all()
