"""`OnlineSLAM` of vista_slam/slam.py on the GPU, with its constructor, attributes and methods, and `run_sequence`, the frame loop of
run.py:153-245 without rerun.  A caller needs

    from vista_slam_amd.slam import OnlineSLAM
    slam = OnlineSLAM(ckpt, vocab, ...)
    slam.step(value)
    ...
    slam.save_data_all(out)

and neither pypose, cv2 nor DBoW3.  Every stage is one of this package's device stages: the keyframe gate (`flow.FlowTracker`), the
encoder, the loop detector (`loop.LoopDetector`), ONE batched scheduler call per keyframe (`slam_scheduler.regress_views`), ONE
`graph.PoseGraph.commit`, and `pgo.optimize` on the graph's own arrays.  Stated differences from the reference: the pose-graph state
and its sums are float64 (fp32 there); the loop candidates are asked for BEFORE the neighbour edges are regressed (they do not depend
on them, slam.py:269), so that all <= neighbor_edge_num + loop_edge_num edges go through one scheduler call, and the bookkeeping keeps
the reference's order, neighbours first; every node's maps and the input images stay on the device; views of an accepted edge with
i - j > neighbor_edge_num enter `loop_related_views` whether `verbose` is set or not (slam.py:199-203 adds them under `verbose` only);
`time_dict` is measured with device events read at `get_time_dict`, and its `graph_construction` is the bookkeeping alone (there it is
a host clock around regress + bookkeeping, from which `get_time_dict` subtracts the decoder).  Single stream: the three-stream schedule
of `keyframe_pipeline` is not used here.  Out of scope: rerun, `run_live.py`, the PNG of `save_pointmap`.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import formats, geo, graph
from .flow import FlowTracker
from .loop import LoopDetector
from .slam_scheduler import EdgeResult, regress_views
from .sta_frontend import STAFrontend

STAGES = ("prepare_data", "encoder", "decoder", "lc", "pgo", "graph_construction")


class View(dict):
    """`munch.Munch` as `get_view` uses it: a dict whose keys are attributes too"""
    __getattr__ = dict.__getitem__


class OnlineSLAM:
    def __init__(self, ckpt_path: Optional[str], vocab_path, verbose: bool = False, max_view_num: int = 400, neighbor_edge_num: int = 3,
                 loop_edge_num: int = 3, loop_dist_min: int = 40, loop_nms: int = 40, loop_cand_thresh_neighbor: int = 5, conf_thres: float = 4.2,
                 rel_pose_thres: float = 0.75, flow_thres: float = 5.0, pgo_every: int = 500, live_mode: bool = False, *,
                 frontend: Optional[STAFrontend] = None, pgo_kwargs: Optional[dict] = None):
        """The reference's signature (slam.py:21-27).  frontend: a built `STAFrontend` in place of ckpt_path; vocab_path: a DBoW3 text
        vocabulary or a `loop.Vocabulary`; pgo_kwargs: keyword arguments of `pgo.optimize`.  The pose graph's arrays are allocated at
        the first frame, whose size they take (`graph.plan` reports the bytes)."""
        self.verbose = verbose
        self.max_view_num = max_view_num
        self.neighbor_edge_num = neighbor_edge_num
        self.loop_edge_num = loop_edge_num
        if neighbor_edge_num + loop_edge_num > graph.MAX_CALL_EDGES:
            raise ValueError(f"{neighbor_edge_num} neighbour and {loop_edge_num} loop edges are more than {graph.MAX_CALL_EDGES} per keyframe")
        graph.plan(max_view_num, neighbor_edge_num, loop_edge_num, 16, 16)               # every refusal that does not depend on the frame size, now
        self.conf_thres = conf_thres
        self.rel_pose_thres = rel_pose_thres
        self.frontend = frontend if frontend is not None else self.load_frontend(ckpt_path)
        self.device = self.frontend.device
        self.pose_graph: Optional[graph.PoseGraph] = None
        self.enc_features: List[torch.Tensor] = []
        self.enc_pos: List[torch.Tensor] = []
        self.img_shapes: list = []
        self.imgs: List[torch.Tensor] = []
        self.view_names: list = []
        self.lc_detector = LoopDetector(self.frontend, vocab_path, loop_dist_min, loop_nms, loop_cand_thresh_neighbor)
        self.view_num = 0
        self.pgo_every = pgo_every
        self.flow_tracker = FlowTracker(self.frontend, flow_thres)
        self.live_mode = live_mode
        self.pgo_window_size = 2 * pgo_every
        self.pgo_kwargs = dict(pgo_kwargs or {})
        self.last_pgo_info = None
        self.last_edges = None
        self._loop_related_views = set()
        self._reset_time()

    # ------------------------------------------------------------------------------------------------------------ state
    @property
    def loop_related_views(self):
        return self.pose_graph.loop_related_views if self.pose_graph is not None else self._loop_related_views

    def _reset_time(self):
        self.time_dict = {k: 0.0 for k in STAGES}
        self._spans: Dict[str, list] = {k: [] for k in STAGES}

    def reset(self):
        """slam.py:76-93 (and the loop detector's database, which the reference's reset leaves behind)"""
        self.enc_features, self.enc_pos, self.img_shapes, self.imgs, self.view_names = [], [], [], [], []
        self.view_num = 0
        if self.pose_graph is not None:
            self.pose_graph.reset()
        self.flow_tracker.reset()
        self.lc_detector.reset()
        self._reset_time()

    def load_frontend(self, ckpt_path: str) -> STAFrontend:
        """slam.py:95-106"""
        frontend = STAFrontend()
        checkpoint = torch.load(ckpt_path, map_location="cpu", weights_only=False)
        frontend.load_state_dict(checkpoint["model"], strict=True)
        del checkpoint
        frontend.eval()
        return frontend

    def _mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _span(self, stage: str, start):
        self._spans[stage].append((start, self._mark()))

    def _graph_for(self, H: int, W: int) -> graph.PoseGraph:
        g = self.pose_graph
        if g is None:
            g = self.pose_graph = graph.PoseGraph(self.frontend, graph.plan(self.max_view_num, self.neighbor_edge_num, self.loop_edge_num, H, W))
        elif (g.plan.H, g.plan.W) != (H, W):
            raise ValueError(f"a frame of {H} x {W} in a graph of {g.plan.H} x {g.plan.W} maps")
        return g

    def _frame_size(self, i: int):
        H, W = (int(v) for v in self.imgs[i].shape[-2:])
        return H, W

    # ------------------------------------------------------------------------------------------------------------ the loop
    def pose_graph_optimize(self):
        """slam.py:108-140: the nodes of the last `pgo_window_size` views and `loop_related_views`"""
        g = self.pose_graph
        if g is None or g.num_edges == 0:
            return
        if self.verbose:
            print(f"Pose graph optimization (at keyframe {self.view_num}) ...")
        self.last_pgo_info = g.optimize(self.view_num, self.pgo_window_size, return_info=True, **self.pgo_kwargs)

    def add_view(self, image, image_shape, view_name):
        """slam.py:142-151; the image stays on the device"""
        image = image if image.dim() == 4 else image[None]
        enc_feat, enc_pos = self.frontend._encode_image(image, image_shape, normalize=False)
        self.enc_features.append(enc_feat)
        self.enc_pos.append(enc_pos)
        self.img_shapes.append(image_shape)
        self.imgs.append(image.squeeze(0).detach().to(self.device, torch.float32).clone())
        self.view_names.append(view_name)
        self.view_num += 1
        assert len(self.enc_features) == len(self.enc_pos) == len(self.img_shapes) == len(self.imgs) == len(self.view_names) == self.view_num

    def _regress(self, i: int, js: Sequence[int]) -> List[EdgeResult]:
        H, W = self._frame_size(i)
        t0 = self._mark()
        res = regress_views(self.frontend, self.enc_features[i], [self.enc_features[j] for j in js], [i - j == 1 for j in js],
                            float(self.rel_pose_thres), H, W)
        self._span("decoder", t0)
        return res

    def _commit(self, i: int, js: Sequence[int], results: Sequence[EdgeResult]):
        H, W = self._frame_size(i)
        t0 = self._mark()
        out = self._graph_for(H, W).commit(i, js, results)
        self._span("graph_construction", t0)
        if self.verbose:
            for j, r in zip(js, results):
                what = "Rejecting edge" if not r.accepted else "Adding loop closure edge" if i - j > self.neighbor_edge_num else "Adding edge"
                print(f"{what} (view {i} [{self.view_names[i]}] -- view {j} [{self.view_names[j]}]) with conf {r.rel_pose_conf:.3f}")
        return out

    def regress_two_views(self, i: int, j: int):
        """slam.py:153-189 -> (se3_ij [1,7], rel_pose_conf_ij [1], confs [2,H,W], intri [3,3], depths [2,H,W]), the last three None for a
        rejected edge"""
        r = self._regress(i, [j])[0]
        se3 = formats.mat_to_se3(self.frontend, r.pose[None])
        conf = torch.tensor([r.rel_pose_conf], dtype=torch.float32, device=self.device)
        return se3, conf, r.confs, r.intri, r.depths

    def connect_view_i_j(self, i: int, j: int) -> bool:
        """slam.py:191-241 for one edge (`step` does all of a keyframe's edges in one call of each stage)"""
        assert i > j, f"i should be larger than j, but got i={i}, j={j}"
        res = self._regress(i, [j])
        return self._commit(i, [j], res)[0] is not None

    def step(self, value, force_pgo: bool = False, log_intermediate_results: bool = False, output_folder=None) -> bool:
        """slam.py:244-297.  value: {'rgb': [1,3,H,W] or [3,H,W] in [-1,1], 'shape': [[H,W]], 'gray': what `LoopDetector.detect_loop`
        takes, 'view_name'}.  -> True iff the pose graph was optimised."""
        t0 = self._mark()
        image, image_shape, img_gray, view_name = value["rgb"], value.get("shape"), value["gray"], value.get("view_name")
        i = self.view_num
        if image_shape is None:
            image_shape = torch.tensor([list(image.shape[-2:])])
        self._graph_for(int(image.shape[-2]), int(image.shape[-1]))
        self._span("prepare_data", t0)

        t0 = self._mark()
        self.add_view(image, image_shape, view_name)
        self._span("encoder", t0)

        t0 = self._mark()
        farthest_neighbor = max(0, i - self.neighbor_edge_num)
        loop_candi_list = self.lc_detector.detect_loop(img_gray, farthest_neighbor)
        self._span("lc", t0)

        js = list(range(farthest_neighbor, i)) + [int(j_sim[0]) for j_sim in loop_candi_list[:self.loop_edge_num]]
        self.last_edges = (i, js, self._regress(i, js) if js else [])      # what the scheduler returned for this keyframe, in edge order
        if js:
            self._commit(i, js, self.last_edges[2])

        if self.view_num % self.pgo_every == 0 or force_pgo:
            if log_intermediate_results:
                self.save_data_all(f"{output_folder}", save_view_graph=False, traj_name_postfix=f"{self.view_num - 1}", save_poses=True, save_images=False,
                                   save_scales=True, save_depths=False, save_intrinsics=False, save_confs=False, save_ply=False)
            t0 = self._mark()
            self.pose_graph_optimize()
            self._span("pgo", t0)
            return True
        return False

    # ------------------------------------------------------------------------------------------------------------ readers
    def get_view(self, v: int, filter_outlier: bool = True, return_pose: bool = True, return_depth: bool = True, return_intri: bool = True) -> View:
        """slam.py:299-326 -> host tensors: pose [4,4], depth [H,W] (scaled, outliers zeroed), intri [3,3]"""
        ex = self.pose_graph.export(conf_thres=self.conf_thres, filter_outlier=filter_outlier, scaled=True, view_num=self.view_num)
        view = View()
        if return_pose:
            view["pose"] = ex.poses[v].cpu()
        if return_depth:
            view["depth"] = ex.depths[v].cpu()
        if return_intri:
            view["intri"] = ex.intrinsics[v].cpu()
        return view

    def get_view_graph(self) -> Dict[int, List[int]]:
        """slam.py:328-336"""
        g = self.pose_graph
        return {v: [g.node_to_connected_view[u] for u in g.view_to_node[v]] for v in range(self.view_num)}

    def save_data_all(self, output_folder, save_view_graph=True, traj_name_postfix=None, save_poses=True, save_images=True, save_scales=True,
                      save_depths=True, save_intrinsics=True, save_confs=True, save_ply=True, gt_poses=None, gt_depths=None, gt_intrinsics=None):
        """slam.py:338-421: the gather is one launch (`PoseGraph.export`), the files are `formats.save_data_all`'s"""
        ex = self.pose_graph.export(view_num=self.view_num)
        formats.save_data_all(self.frontend, output_folder, poses=ex.poses, scales=ex.scales, depths=ex.depths, confs=ex.confs, intrinsics=ex.intrinsics,
                              imgs=torch.stack(self.imgs, dim=0), conf_thres=self.conf_thres, view_graph=self.get_view_graph() if save_view_graph else None,
                              loop_min_dist=self.lc_detector.loop_dist_min, view_names=self.view_names, save_view_graph=save_view_graph,
                              traj_name_postfix=traj_name_postfix, save_poses=save_poses, save_images=save_images, save_scales=save_scales,
                              save_depths=save_depths, save_intrinsics=save_intrinsics, save_confs=save_confs, save_ply=save_ply, gt_poses=gt_poses,
                              gt_depths=gt_depths, gt_intrinsics=gt_intrinsics)

    def get_pointmap_vis(self, v: int):
        """slam.py:423-432 -> (uint8 [H,W,3] image of the normalised local point map, the point map itself)"""
        view = self.get_view(v, filter_outlier=False, return_pose=False, return_depth=True, return_intri=True)
        pcl = geo.compute_local_pointclouds(self.frontend, view.depth.unsqueeze(0), view.intri).squeeze(0).cpu().numpy()
        min_vals = pcl.min(axis=(0, 1), keepdims=True)
        max_vals = pcl.max(axis=(0, 1), keepdims=True)
        normalized = (pcl - min_vals) / (max_vals - min_vals + 1e-8)
        return (normalized * 255).astype(np.uint8), pcl

    def save_pointmap(self, v: int, output_folder):
        """slam.py:434-440 without the PNG (cv2 is not a dependency)"""
        os.makedirs(output_folder, exist_ok=True)
        _img, pcl = self.get_pointmap_vis(v)
        np.save(f"{output_folder}/pointmap_cam_{v}.npy", pcl)

    def get_time_dict(self) -> Dict[str, float]:
        """Seconds per stage and their total, from device events: reading them waits for the work recorded so far."""
        for stage, spans in self._spans.items():
            for start, end in spans:
                end.synchronize()
                self.time_dict[stage] += start.elapsed_time(end) * 1e-3
            spans.clear()
        time_dict = self.time_dict.copy()
        time_dict["total"] = sum(time_dict.values())
        return time_dict


def run_sequence(slam: OnlineSLAM, frames: Sequence[dict], keyframe_detection: str = "flow", stride: int = 1, max_view_num: Optional[int] = None) -> dict:
    """The frame loop of run.py:153-245 without rerun.  frames: a sequence of the dicts `preprocess.process_image` produces ('rgb'
    [3,H,W] in [-1,1], 'gray', optionally 'img_name').  keyframe_detection: "flow" (the gate), "stride", or "flow_stride" (the gate, and a
    restart by stride after `slam.reset()` once more than max_view_num keyframes were taken).  The last frame forces the optimisation.
    -> {'keyframes': frame indices, 'restarted': bool, 'is_optimized': bool}"""
    if keyframe_detection not in ("flow", "stride", "flow_stride"):
        raise ValueError(f'keyframe_detection is "flow", "stride" or "flow_stride" (got {keyframe_detection!r})')
    cap = slam.max_view_num if max_view_num is None else int(max_view_num)
    last = len(frames)

    def stride_indices():
        idx = list(range(1, last, stride))
        if len(idx) > cap:
            idx = [int(v) for v in torch.linspace(0, last - 1, steps=cap).long()]
        return idx
    using_stride = keyframe_detection == "stride"
    stride_idxes = stride_indices() if using_stride else []
    first, is_optimized, restarted, keyframes, t = True, False, False, [], 0
    while t < last:
        data = frames[t]
        if using_stride:
            is_keyframe = t in stride_idxes
        else:
            is_keyframe = slam.flow_tracker.compute_disparity(data["gray"], visualize=False)
        if not is_keyframe:
            if t == last - 1 and not is_optimized:
                slam.pose_graph_optimize()
                is_optimized = True
            t += 1
            continue
        rgb = data["rgb"]
        value = {"rgb": rgb if rgb.dim() == 4 else rgb[None], "shape": torch.tensor([list(rgb.shape[-2:])]), "gray": data["gray"],
                 "view_name": data.get("img_name", str(t))}
        is_optimized = slam.step(value, force_pgo=(t == last - 1))
        keyframes.append(t)
        if first:
            first = False
            t += 1
            continue
        if slam.view_num > cap:
            if keyframe_detection == "flow_stride" and not using_stride:
                stride_idxes = stride_indices()
                using_stride, first, restarted, keyframes, t = True, True, True, [], 0
                slam.reset()
                continue
            slam.pose_graph_optimize()
            is_optimized = True
            break
        t += 1
    return {"keyframes": keyframes, "restarted": restarted, "is_optimized": is_optimized}
