"""`OnlineSLAM.step` with all stages, and one `PoseGraph.commit` against what it replaces, timed on the GPU.

    python tools/slam_bench.py [reps] [--parent-lib PATH/libsta_mi355.so]      # default 20 alternating runs

Synthetic frames (a camera panning over a procedural blob panorama, tests/flow_cases.py), procedural weights of the full-size model,
224 x 224 and 384 x 512, the default regime (3 neighbour + 3 loop edges), rel_pose_thres 0 so that every candidate edge is accepted and
goes through the DPT heads and the bookkeeping (the most work a keyframe can cost).

(a) keyframes/s of `OnlineSLAM.step` over KEYFRAMES keyframes (host wall-clock around the synchronised run, a warm-up run first) with the
    optimiser every PGO_EVERY keyframes, and the per-stage breakdown of `get_time_dict` (device events).  Nobody has measured this loop
    before and no target is set: the reference's own loop needs pypose, cv2 and DBoW3 and cannot run where this one is measured.
(b) one `commit` per keyframe against the route it replaces: `keyframe_pipeline.NodeBook.add` (the scale and sqrt-mean reductions, one
    node at a time) plus the torch statements for the mean confidence, the best node, the Sim(3) products (`pgo.sim3_mul`) and the edge
    appends, writing the same arrays (compared before timing).  Both replay the same recorded scheduler results of COMMIT_KEYFRAMES
    keyframes from an empty graph, alternating, `reps` runs each, host wall-clock around the synchronised replay (the replaced route is
    bound by its launches, which device events around single kernels would not show).  With --parent-lib the replaced route's library
    calls (sta_estimate_scale, sta_mat_to_se3, sta_sim3_op: kernels this build shares with its parent) run on that build.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
import flow_cases as F                                                         # noqa: E402
from vista_slam_amd import _lib, formats, graph, loop, pgo, weights as W       # noqa: E402
from vista_slam_amd.keyframe_pipeline import EdgeRecord, NodeBook              # noqa: E402
from vista_slam_amd.slam import OnlineSLAM                                     # noqa: E402
from vista_slam_amd.slam_scheduler import regress_views                        # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend                            # noqa: E402

args = sys.argv[1:]
parent_lib = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
nums = [int(v) for v in args if v.isdigit()]
reps = nums[0] if nums else 20
KEYFRAMES, PGO_EVERY, COMMIT_KEYFRAMES, NB, LP = 40, 20, 12, 3, 3
DIST_MIN, NMS = 10, 5

m = STAFrontend(W.FULL, "cuda:0").load_procedural(seed=43)
shared = m if parent_lib is None else STAFrontend(W.TINY, "cuda:0", lib=_lib.load_other(parent_lib)).load_procedural(seed=43)


def full_tree(k, depth, seed):
    rng = np.random.RandomState(seed)
    inner = sum(k ** d for d in range(depth))
    n = inner + k ** depth
    idx = np.arange(n)
    return loop.Vocabulary.from_arrays(rng.randint(0, 256, (n, 32)).astype(np.uint8), np.where(idx < inner, idx * k + 1, 0),
                                       np.where(idx < inner, k, 0), np.where(idx >= inner, idx - inner, -1), 0.25 + 3.0 * rng.rand(k ** depth))


def frames_of(H, Wd, n):
    """a pan over a blob panorama and back: frame t and frame n - 1 - t see the same place"""
    pano = F.blob_frame(H + 6, Wd * 4, seed=3, n_blobs=1200)
    half, out = n // 2, []
    for t in range(n):
        step, y0, dx = (t, 0, 0) if t < half else (n - 1 - t, 3, 1)
        x0 = int(round(step * (Wd * 3 - 1) / (half - 1) * 0.9)) + dx
        g = torch.from_numpy(np.ascontiguousarray(pano[y0:y0 + H, x0:x0 + Wd])).cuda()
        out.append({"rgb": (g.float() / 127.5 - 1.0)[None].expand(1, 3, -1, -1).contiguous(), "gray": g, "view_name": str(t)})
    return out


class Replaced:
    """The state `PoseGraph` keeps, written the way the parent could: NodeBook.add for the reductions, torch statements for the rest.
    No host read anywhere (the best node is a torch.where on device tables), so the comparison is launches against launches."""

    def __init__(self, fe, plan_):
        dev, p = fe.device, plan_
        self.fe, self.p = fe, p
        self.poses = torch.empty(p.max_nodes, 8, device=dev, dtype=torch.float64)
        self.edges = torch.empty(p.max_edges, 2, device=dev, dtype=torch.int64)
        self.edge_poses = torch.empty(p.max_edges, 8, device=dev, dtype=torch.float64)
        self.edge_confs = torch.empty(p.max_edges, 7, device=dev, dtype=torch.float64)
        self.depth = torch.empty(p.max_nodes, p.H, p.W, device=dev)
        self.conf = torch.empty(p.max_nodes, p.H, p.W, device=dev)
        self.intri = torch.empty(p.max_nodes, 3, 3, device=dev)
        self.mean_conf = torch.empty(p.max_nodes, device=dev, dtype=torch.float64)
        self.best_node = torch.empty(p.max_views, device=dev, dtype=torch.int32)
        self.best_conf = torch.empty(p.max_views, device=dev, dtype=torch.float64)
        self.identity = torch.tensor([0, 0, 0, 0, 0, 0, 1, 1], device=dev, dtype=torch.float64)
        self.two = torch.full((6,), 2.0, device=dev, dtype=torch.float64)
        self.reset()

    def reset(self):
        self.poses.copy_(self.identity.expand_as(self.poses))
        self.edge_poses.copy_(self.identity.expand_as(self.edge_poses))
        self.edges.fill_(-1); self.edge_confs.fill_(1.0); self.best_node.fill_(-1); self.best_conf.fill_(-100.0)
        self.book, self.first, self.nn, self.ne = NodeBook(self.fe), {}, 0, 0

    def _edge(self, a, b, T, w):
        self.edges[self.ne, 0] = a; self.edges[self.ne, 1] = b
        self.edge_poses[self.ne] = T
        self.edge_confs[self.ne] = w
        self.ne += 1

    def commit(self, i, js, results):
        fe = self.fe
        for j, r in zip(js, results):
            if not r.accepted:
                continue
            rec = EdgeRecord(i, j, r)
            self.book.add(rec)                                            # the two reductions, one node at a time (and the first node's clones)
            se3 = formats.mat_to_se3(fe, r.pose[None])[0].double()
            sim3_ij = torch.cat([se3, self.identity[7:]])
            nodes, i_new = [], i not in self.first
            for side, v in enumerate((i, j)):
                n = self.nn
                self.depth[n].copy_(r.depths[side]); self.conf[n].copy_(r.confs[side]); self.intri[n].copy_(r.intri)
                mean = r.confs[side].double().mean()
                self.mean_conf[n] = mean
                better = mean > self.best_conf[v]
                self.best_node[v] = torch.where(better, torch.full_like(self.best_node[v], n), self.best_node[v])
                self.best_conf[v] = torch.where(better, mean, self.best_conf[v])
                if v in self.first:
                    S = torch.cat([self.identity[:7], rec.scales[side].double().reshape(1)])
                    self._edge(n, self.first[v], S, torch.cat([self.two, rec.scale_confs[side].double().reshape(1)]))
                    self.poses[n] = pgo.sim3_mul(fe, self.poses[self.first[v]][None], S[None])[0]
                else:
                    self.first[v] = n
                nodes.append(n)
                self.nn += 1
            if i_new:
                self.poses[nodes[0]] = pgo.sim3_mul(fe, self.poses[nodes[1]][None], sim3_ij[None])[0]
            self._edge(nodes[0], nodes[1], sim3_ij, float(r.rel_pose_conf))


def edge_list(i):
    far = max(0, i - NB)
    return list(range(far, i)) + [j for j in range(far) if i - j > 4][:LP]


def stats(t):
    t = np.asarray(t)
    return f"median {np.median(t):9.1f} us   min {t.min():9.1f}   max {t.max():9.1f}"


print(f"{torch.cuda.get_device_name(0)}; full-size model, procedural weights; replaced route's library calls on {'this build' if parent_lib is None else parent_lib}")
voc = full_tree(10, 4, 5).bind(m)
for H, Wd in ((224, 224), (384, 512)):
    frames = frames_of(H, Wd, KEYFRAMES)
    plan_ = graph.plan(400, NB, LP, H, Wd)
    print(f"{H} x {Wd}: graph.plan(400, {NB}, {LP}): {plan_.max_nodes} nodes, {plan_.max_edges} edges, state {plan_.state_bytes / 1e9:.2f} GB "
          f"(map pool {plan_.pool_bytes / 1e9:.2f} GB), export buffers {plan_.export_bytes / 1e9:.2f} GB")
    # ---- (a) the whole loop
    slam = OnlineSLAM(None, voc, max_view_num=400, neighbor_edge_num=NB, loop_edge_num=LP, loop_dist_min=DIST_MIN, loop_nms=NMS, loop_cand_thresh_neighbor=NB,
                      rel_pose_thres=0.0, pgo_every=PGO_EVERY, frontend=m)
    walls = []
    for run in range(3):                                                   # the first run is the warm-up
        slam.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in frames:
            slam.step(f)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        t = slam.get_time_dict()
    g = slam.pose_graph
    info = slam.last_pgo_info
    print(f"  OnlineSLAM.step, {KEYFRAMES} keyframes, optimiser every {PGO_EVERY}: {KEYFRAMES / walls[1]:.1f} and {KEYFRAMES / walls[2]:.1f} keyframes/s "
          f"(two timed runs; warm-up run {KEYFRAMES / walls[0]:.1f}); {g.num_nodes} nodes, {g.num_edges} edges")
    print("  stages of the last run (device events, ms per keyframe): " + "  ".join(f"{k} {v * 1e3 / KEYFRAMES:.3f}" for k, v in t.items()))
    print(f"  last optimisation: status {info['status']}, {len(info['f'])} trials" + (f", cost {info['f'][0]:.4g} -> {min(info['f_new']):.4g}" if info["f"] else ""))
    no_pgo = sum(v for k, v in t.items() if k not in ("pgo", "total"))
    print(f"  without the optimiser: {no_pgo * 1e3 / KEYFRAMES:.3f} ms of device time per keyframe = {KEYFRAMES / no_pgo:.1f} keyframes/s")
    # ---- (b) commit against the route it replaces
    feats = slam.enc_features
    rec = []
    for i in range(1, COMMIT_KEYFRAMES + 1):
        js = edge_list(i)
        rec.append((i, js, regress_views(m, feats[i], [feats[j] for j in js], [i - j == 1 for j in js], 0.0, H, Wd)))
    del slam
    torch.cuda.empty_cache()
    small = graph.plan(COMMIT_KEYFRAMES + 1, NB, LP, H, Wd)
    new, old = graph.PoseGraph(m, small), Replaced(shared, small)

    def replay(route):
        route.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, js, rs in rec:
            route.commit(i, js, rs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / len(rec)
    replay(new); replay(old)
    n, E = new.num_nodes, new.num_edges
    assert (old.nn, old.ne) == (n, E)
    diffs = {k: float((getattr(new, k)[:c].double() - getattr(old, k)[:c].double()).abs().max()) for k, c in
             (("poses", n), ("edge_poses", E), ("edge_confs", E), ("mean_conf", n), ("depth", n), ("conf", n))}
    same = torch.equal(new.edges[:E], old.edges[:E]) and torch.equal(new.best_node, old.best_node)
    print(f"  {len(rec)} keyframes, {sum(len(js) for _, js, _ in rec)} accepted edges -> {n} nodes, {E} edges; index arrays equal: {same}; max |difference| "
          + " ".join(f"{k} {v:.1e}" for k, v in diffs.items()) + "  (fp32 reductions on the replaced route)")
    tn, to = [], []
    for _ in range(reps):
        tn.append(replay(new)); to.append(replay(old))
    print(f"  per keyframe, host wall-clock around the synchronised replay, {reps} alternating runs:")
    print(f"    PoseGraph.commit (2 launches)                        {stats(tn)}")
    print(f"    NodeBook.add + torch statements                      {stats(to)}")
    del new, old, rec
    torch.cuda.empty_cache()
