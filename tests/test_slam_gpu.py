"""GPU: `vista_slam_amd.slam.OnlineSLAM` and `run_sequence`.

(1) `step` over the frames of the reference's sequence fixtures (oracle/gen_golden.py gen_seq: add_view + connect_view_i_j replayed on
the imported reference model), a stub loop detector returning the fixture protocol's candidates: every edge's pose, confidence,
decision, intrinsics, maps, scale and scale confidence held to the fixture by the rules of
test_gpu_parity.py::test_keyframe_sequence_vs_reference_golden (helpers.compare_seq_edges, scales judged against e*_scale_abs); the
graph after the run equals the restatement tests/graph_cases.py fed with the GPU's own edge results.  Nothing here reads the reference.
(2) The whole loop: 60 procedural frames that return to their start through `run_sequence` with the real keyframe gate, the real loop
detector on a procedural vocabulary and the forced final optimisation; keyframes and candidates equal the restatements'
(tests/flow_cases.py, tests/loop_cases.py), the graph equals the restatement driven by the same decisions, the optimisation does not
raise the cost, a repeat after reset() is bit-identical, and one flow_stride restart."""
import numpy as np
import pytest

import flow_cases as F
import graph_cases as GC
import loop_cases as L

pytestmark = pytest.mark.gpu

TOL = 1e-3
DEFAULT = "f16x3h"
SEQ = ["seq_tum_tiny_48x64", "seq_7scenes_tiny_48x64", "seq_default_tiny_48x64"]


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    yield gpu_checks
    gpu_checks.drop_models()


def vocabulary():
    from vista_slam_amd import loop
    V = L.vocab_arrays(L.make_vocab(10, 2, seed=5))
    return V, loop.Vocabulary.from_arrays(V.node_desc, V.child_first, V.child_count, V.word_of, V.word_weight)


class StubDetector:
    """the fixture protocol's loop candidates (oracle/seq_protocol.py) behind `LoopDetector.detect_loop`'s signature"""

    def __init__(self, nb, lp, dist):
        self.nb, self.lp, self.loop_dist_min, self.n = nb, lp, dist, 0

    def reset(self):
        self.n = 0

    def detect_loop(self, image, farthest_neighbor):
        from oracle.seq_protocol import seq_edge_list
        i, self.n = self.n, self.n + 1
        js, far = seq_edge_list(i, self.nb, self.lp, self.loop_dist_min)
        assert far == farthest_neighbor
        return [(j, 1.0) for j in js[i - far:]]


def numpy_edges(log):
    """[(i, js, [EdgeResult])] -> the same with graph_cases.Edge (numpy)"""
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    return [(i, js, [GC.Edge(n(r.pose), r.rel_pose_conf, bool(r.accepted), n(r.confs), n(r.intri), n(r.depths)) for r in rs]) for i, js, rs in log if js]


class Frozen:
    """a `PoseGraph` at one moment: its snapshot and a copy of its host mirror (what graph_cases.check_state reads)"""

    def __init__(self, g):
        import copy
        self._snap, self.plan, self.view_num = g.snapshot(), g.plan, g.view_num
        self.node_to_view, self.node_to_connected_view = list(g.node_to_view), list(g.node_to_connected_view)
        self.view_to_node, self.loop_related_views = copy.deepcopy(g.view_to_node), set(g.loop_related_views)
        self._view_graph = g.get_view_graph()

    def snapshot(self):
        return self._snap

    def get_view_graph(self):
        return self._view_graph


def restatement(slam, log):
    p = slam.pose_graph.plan
    return GC.replay(numpy_edges(log), p.max_nodes, p.max_edges, p.neighbor_edge_num)


@pytest.mark.parametrize("case", SEQ)
def test_step_over_the_reference_sequences(G, case):
    import torch
    from helpers import compare_seq_edges, load_golden, seq_meta
    from oracle.seq_protocol import seq_edge_list, seq_frames
    from vista_slam_amd import weights as W
    from vista_slam_amd.slam import OnlineSLAM
    g, meta = load_golden(case)
    sm = seq_meta(meta)
    H, Wd, nkf, nb, lp = sm["H"], sm["W"], sm["nkf"], sm["neighbor_edge_num"], sm["loop_edge_num"]
    m = G.model("tiny", float(meta.get("qk_gain", 1.0)), DEFAULT, sm["seed"])
    m.range_report(reset=True)
    slam = OnlineSLAM(None, vocabulary()[1], max_view_num=nkf, neighbor_edge_num=nb, loop_edge_num=lp, rel_pose_thres=float(g["thres"]), pgo_every=10 ** 6,
                      frontend=m)
    slam.lc_detector = StubDetector(nb, lp, sm["loop_dist_min"])
    frames = torch.from_numpy(seq_frames(W, nkf, H, Wd, sm["seed"], sm["tag"])).cuda()
    log = []
    for i in range(nkf):
        assert slam.step({"rgb": frames[i:i + 1], "shape": torch.tensor([[H, Wd]]), "gray": None, "view_name": f"kf{i}"}) is False
        assert slam.last_edges[1] == seq_edge_list(i, nb, lp, sm["loop_dist_min"])[0]
        log.append(slam.last_edges)
    torch.cuda.synchronize()
    assert slam.view_num == nkf and slam.view_names == [f"kf{i}" for i in range(nkf)] and len(slam.enc_features) == len(slam.imgs) == nkf
    pg = slam.pose_graph
    snap = pg.snapshot()
    index = {(int(a), int(b)): e for e, (a, b) in enumerate(snap["edges"])}
    # the scale edges of each accepted edge's two nodes, out of the graph's own arrays
    seen, node, edges = {v: [] for v in range(nkf)}, 0, []
    for i, js, rs in numpy_edges(log):
        for j, r in zip(js, rs):
            scales, scale_confs = [None, None], [None, None]
            if r.accepted:
                for side, v in enumerate((i, j)):
                    if seen[v]:
                        e = index[(node, seen[v][0])]
                        scales[side], scale_confs[side] = float(snap["edge_poses"][e, 7]), float(snap["edge_confs"][e, 6])
                    seen[v].append(node)
                    node += 1
            edges.append(dict(i=i, j=j, pose=r.pose, conf=float(r.rel_pose_conf), accepted=r.accepted, confs=r.confs, intri=r.intri, depths=r.depths,
                              scales=scales, scale_confs=scale_confs))
    worst = compare_seq_edges(edges, g, meta, tol=TOL)
    acc = [e["accepted"] for e in edges]
    assert any(acc) and not all(acc)
    assert any(e["i"] - e["j"] != 1 and e["accepted"] for e in edges), "no accepted non-adjacent edge in the fixture"
    assert m.range_report() == (0, 0)
    # the graph = the restatement fed with the GPU's own edge results
    ref = restatement(slam, log)
    e_pose, e_edge = GC.check_state(pg, ref, nkf)
    assert slam.loop_related_views == ref.loop_related_views and slam.get_view_graph() == ref.get_view_graph(nkf)
    t = slam.get_time_dict()
    assert set(t) == {"prepare_data", "encoder", "decoder", "lc", "pgo", "graph_construction", "total"}
    assert t["encoder"] > 0 and t["decoder"] > 0 and t["graph_construction"] > 0 and t["pgo"] == 0 and abs(t["total"] - sum(v for k, v in t.items() if k != "total")) < 1e-9
    print(f"[slam] {case}: " + " ".join(f"{k}={v:.1e}" for k, v in sorted(worst.items())) + f" poses={e_pose:.1e} edge_poses={e_edge:.1e}")


def test_single_edge_methods_and_readers(G, tmp_path):
    """`regress_two_views` / `connect_view_i_j` (the reference's per-edge surface) build the same graph as `step`; `get_view`,
    `get_pointmap_vis` and `save_data_all` return the reference's shapes and dtypes and write its files."""
    import torch
    from helpers import load_golden, seq_meta
    from oracle.seq_protocol import seq_frames
    from vista_slam_amd import weights as W
    from vista_slam_amd.slam import OnlineSLAM
    g, meta = load_golden(SEQ[0])
    sm = seq_meta(meta)
    H, Wd, nb, lp, nkf = sm["H"], sm["W"], sm["neighbor_edge_num"], sm["loop_edge_num"], 5
    m = G.model("tiny", float(meta.get("qk_gain", 1.0)), DEFAULT, sm["seed"])
    frames = torch.from_numpy(seq_frames(W, sm["nkf"], H, Wd, sm["seed"], sm["tag"])).cuda()
    mk = lambda: OnlineSLAM(None, vocabulary()[1], max_view_num=nkf, neighbor_edge_num=nb, loop_edge_num=lp, rel_pose_thres=float(g["thres"]),
                            conf_thres=1.0, pgo_every=10 ** 6, frontend=m)
    a, b = mk(), mk()
    a.lc_detector = StubDetector(nb, lp, sm["loop_dist_min"])
    for i in range(nkf):
        a.step({"rgb": frames[i:i + 1], "shape": torch.tensor([[H, Wd]]), "gray": None, "view_name": str(i)})
        b.add_view(frames[i:i + 1], torch.tensor([[H, Wd]]), str(i))
        b._graph_for(H, Wd)
        for j, r in zip(a.last_edges[1], a.last_edges[2]):
            assert b.connect_view_i_j(i, j) is bool(r.accepted)
    sa, sb = a.pose_graph.snapshot(), b.pose_graph.snapshot()
    for key in ("edges", "first_node", "best_node", "num_nodes", "num_edges"):
        assert np.array_equal(sa[key], sb[key]), key
    for key in ("depth", "conf"):      # B = 1 decodes against one batched decode: each is within 1e-3 of the fixture in the max norm
        assert np.abs(sa[key] - sb[key]).max() <= 2e-3 * np.abs(sa[key]).max(), key
    se3, conf, confs, intri, depths = a.regress_two_views(1, 0)
    assert se3.shape == (1, 7) and se3.dtype == torch.float32 and conf.shape == (1,) and confs.shape == depths.shape == (2, H, Wd) and intri.shape == (3, 3)
    view = a.get_view(2)
    assert view.pose.shape == (4, 4) and view.pose.dtype == torch.float32 and not view.pose.is_cuda and view.depth.shape == (H, Wd) and view.intri.shape == (3, 3)
    ex = a.pose_graph.export(conf_thres=1.0, filter_outlier=True, scaled=True)
    assert torch.equal(view.depth, ex.depths[2].cpu()) and set(a.get_view(1, return_depth=False)) == {"pose", "intri"}
    img, pcl = a.get_pointmap_vis(3)
    assert img.shape == (H, Wd, 3) and img.dtype == np.uint8 and pcl.shape == (H, Wd, 3)
    gt = np.tile(np.eye(4), (nkf, 1, 1))
    a.save_data_all(str(tmp_path), gt_poses=gt)
    ex = a.pose_graph.export()
    assert np.array_equal(np.load(tmp_path / "trajectory.npy"), ex.poses.cpu().numpy()) and np.load(tmp_path / "scales.npy").shape == (nkf, 1)
    assert np.load(tmp_path / "images.npy").shape == (nkf, H, Wd, 3) and np.load(tmp_path / "depths.npy").shape == (nkf, H, Wd)
    assert np.load(tmp_path / "gt_poses.npy").dtype == np.float32 and (tmp_path / "pointcloud.ply").exists()
    vg = np.load(tmp_path / "view_graph.npz", allow_pickle=True)
    assert vg["view_graph"].item() == a.get_view_graph() and int(vg["loop_min_dist"]) == sm["loop_dist_min"] and list(vg["view_names"]) == [str(i) for i in range(nkf)]
    a.save_pointmap(3, str(tmp_path))
    assert np.array_equal(np.load(tmp_path / "pointmap_cam_3.npy"), pcl)


# ------------------------------------------------------------------------------------------------------------ the whole loop
FLOW_THRES = 18.0            # the sequence moves about 12 px per frame: every second frame is a keyframe; no mean within 0.6 px of it
DIST_MIN, NMS, NB, LP = 10, 5, 3, 3
# The tiny configuration's procedural weights give depths of both signs, so a scale edge sum(w Dn Df) / sum(w Dn Dn) can come out negative,
# and the cost (a Log of it) is then undefined - in the reference as much as here; pgo.optimize reports status 2 | 32 and leaves the nodes.
# Of the weight seeds 43 .. 52, eight give 179 positive scale edges on this sequence (43 and 44 do not); 46 has the narrowest spread
# (0.88 .. ), and the test checks that they are positive before it looks at the cost.
LOOP_SEED = 46
ORB = dict(nfeatures=300, nlevels=3, edge=22)


def loop_frames():
    import torch
    out = []
    for t, f in enumerate(L.loop_sequence()):
        x = torch.from_numpy(f).cuda()
        rgb = (x.float() / 127.5 - 1.0)[None].expand(3, -1, -1).contiguous()
        out.append({"rgb": rgb, "gray": x, "img_name": f"f{t:02d}"})
    return out


def expected_loop():
    """the restatements on the same frames: the keyframes (flow_cases.RefTracker) and each keyframe's candidates (loop_cases)"""
    seq = L.loop_sequence()
    rt = F.RefTracker(FLOW_THRES)
    kf = [t for t, f in enumerate(seq) if rt.compute_disparity(f)]
    means = [r[4] / r[3] for r in rt.log if r[3]]
    assert min(abs(x - FLOW_THRES) for x in means) > 0.5 and all(r[1] in ("first", "moved", "still") for r in rt.log)
    V, pattern, trig = vocabulary()[0], L.default_pattern(), L.trig_table()
    feats, cands, margins = [], [], []
    for i, t in enumerate(kf):
        d = L.extract(seq[t], pattern=pattern, trig=trig, **ORB)[2]
        feats.append(None if len(d) == 0 else L.transform(d, V))
        present = [x is not None for x in feats]
        sim = [L.score((feats[i][0], feats[i][2]), (feats[j][0], feats[j][2])) if present[i] and present[j] else 0.0 for j in range(i)]
        far = max(0, i - NB)
        cands.append(L.reference_detect_loop(list(feats), lambda a, b: L.score((a[0], a[2]), (b[0], b[2])), DIST_MIN, NMS, NB, far))
        margins.append(L.detect_loop_margins(present, sim, i, far, DIST_MIN, NMS, NB)[0])
    assert min(margins) > 1e-9 and any(len(c) >= 2 for c in cands)
    return kf, cands


def test_whole_loop_with_the_real_gate_detector_and_optimiser(G):
    import torch
    from vista_slam_amd import loop
    from vista_slam_amd.slam import OnlineSLAM, run_sequence
    m = G.model("tiny", 1.0, DEFAULT, LOOP_SEED)
    frames = loop_frames()
    kf, cands = expected_loop()
    slam = OnlineSLAM(None, vocabulary()[1], max_view_num=40, neighbor_edge_num=NB, loop_edge_num=LP, loop_dist_min=DIST_MIN, loop_nms=NMS,
                      loop_cand_thresh_neighbor=NB, rel_pose_thres=0.0, flow_thres=FLOW_THRES, pgo_every=10 ** 6, frontend=m)
    slam.lc_detector = loop.LoopDetector(m, vocabulary()[1], DIST_MIN, NMS, NB, **ORB)

    def run():
        """-> (run_sequence's result, every keyframe's edges, the graph as it was when the optimisation began)"""
        log, before = [], []
        step, optimize = slam.step, slam.pose_graph_optimize

        def logged(value, **kw):
            out = step(value, **kw)
            log.append(slam.last_edges)
            return out

        def frozen():
            log.append(slam.last_edges)                   # the forced optimisation runs inside the last step
            before.append(Frozen(slam.pose_graph))
            optimize()
        slam.step, slam.pose_graph_optimize = logged, frozen
        try:
            res = run_sequence(slam, frames, "flow")
        finally:
            del slam.step, slam.pose_graph_optimize
        torch.cuda.synchronize()
        assert len(before) == 1 and log[-1] is log[-2]
        return res, log[:-1], before[0]
    res, log, pre = run()
    assert res == {"keyframes": kf, "restarted": False, "is_optimized": True}
    assert slam.view_names == [f"f{t:02d}" for t in kf]
    for i, (_i, js, _rs) in enumerate(log):
        far = max(0, i - NB)
        assert js == list(range(far, i)) + [j for j, _ in cands[i][:LP]], (i, js, cands[i])
    assert any(len(js) > NB for _i, js, _rs in log), "no loop edge in the run"
    # the graph before the optimisation = the restatement driven by the same decisions; only the node poses move afterwards
    ref = restatement(slam, log)
    GC.check_state(pre, ref, len(kf))
    snap = slam.pose_graph.snapshot()
    after = snap["poses"]
    info = slam.last_pgo_info
    scale_edges = [e for e in range(ref.num_edges) if ref.node_to_view[ref.edges[e, 0]] == ref.node_to_view[ref.edges[e, 1]]]
    scales = snap["edge_poses"][scale_edges, 7]
    print(f"[slam] loop: {len(scales)} scale edges in [{scales.min():.3g}, {scales.max():.3g}], {int((scales <= 0).sum())} not positive; status {info['status']}")
    assert (scales > 0).all(), "a scale edge is not positive: the cost is undefined for these weights"
    assert info is not None and info["status"] == 0 and len(info["f"]) >= 1 and ref.loop_related_views and slam.loop_related_views == set()
    for key in snap:
        assert key == "poses" or np.array_equal(snap[key], pre.snapshot()[key]), key
    accepted = [fn for f, fn in zip(info["f"], info["f_new"]) if fn < f]
    final = accepted[-1] if accepted else info["f"][0]
    assert np.isfinite(final) and final <= info["f"][0], (final, info["f"][0])
    assert accepted, "the forced optimisation accepted no step"
    assert GC.rel(after, ref.poses[:ref.num_nodes]) > 1e-9                     # ... and it did move the nodes
    t = slam.get_time_dict()
    assert all(t[k] > 0 for k in ("encoder", "decoder", "lc", "pgo", "graph_construction"))
    # a repeat after reset(): bit-identical
    slam.reset()
    res2, log2, pre2 = run()
    snap2 = slam.pose_graph.snapshot()
    assert res2 == res and [e[1] for e in log2] == [e[1] for e in log]
    for key in snap:
        assert np.array_equal(snap2[key], snap[key]) and np.array_equal(pre2.snapshot()[key], pre.snapshot()[key]), key
    print(f"[slam] loop: {len(kf)} keyframes, {ref.num_nodes} nodes, {ref.num_edges} edges, cost {info['f'][0]:.4g} -> {final:.4g} in {len(info['f'])} trials, "
          + " ".join(f"{k}={v * 1e3:.1f}ms" for k, v in t.items()))


def test_flow_stride_restart(G):
    """more than max_view_num = 4 keyframes from the gate: `slam.reset()` and a restart by stride (run.py:209-232)"""
    from vista_slam_amd import loop
    from vista_slam_amd.slam import OnlineSLAM, run_sequence
    m = G.model("tiny", 1.0, DEFAULT)
    frames = loop_frames()
    slam = OnlineSLAM(None, vocabulary()[1], max_view_num=4, neighbor_edge_num=NB, loop_edge_num=LP, loop_dist_min=DIST_MIN, loop_nms=NMS,
                      loop_cand_thresh_neighbor=NB, rel_pose_thres=0.0, flow_thres=FLOW_THRES, pgo_every=10 ** 6, frontend=m)
    slam.lc_detector = loop.LoopDetector(m, vocabulary()[1], DIST_MIN, NMS, NB, **ORB)
    res = run_sequence(slam, frames, "flow_stride", stride=20, max_view_num=4)
    assert res == {"keyframes": [1, 21, 41], "restarted": True, "is_optimized": True}
    assert slam.view_num == 3 and slam.view_names == ["f01", "f21", "f41"] and slam.pose_graph.view_num == 3
    assert slam.pose_graph.num_nodes == 6 and len(slam.lc_detector.bow_feats) == 3
    with pytest.raises(ValueError, match="keyframe_detection"):
        run_sequence(slam, frames, "optical")
