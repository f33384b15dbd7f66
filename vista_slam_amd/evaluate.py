"""Score a run: the surface of the reference's `vista_slam/eval/` (eval_traj.py, eval_recon.py) without evo, Open3D or pykdtree.

Trajectory half (`align_traj`, `ape_translation`, `full_traj_eval`): Umeyama's Sim(3) alignment of the camera positions and the
translation APE.  A trajectory is at most a few thousand poses: this half has no hot path and runs on the host in numpy float64.

Reconstruction half (`eval_recon`, `eval_recon_from_saved_data`): world clouds, voxel down-sampling, point-to-point ICP and the clipped
chamfer distance, all on the device (formats.world_pointcloud, formats.voxel_downsample, vista_slam_amd.cloud).

Mesh half (`eval_mesh`, `mesh_depth_l1`): the protocol of the 7-Scenes and Replica evaluations of dense SLAM systems - points drawn
uniformly by area from the estimated and the ground-truth surface (vista_slam_amd.surface), nearest neighbours both ways
(vista_slam_amd.cloud), accuracy, completion, completion ratio and F-score; and the L1 difference of the two meshes' depth maps
(render.mesh_depth, or meshdist.ray_depth with method="rays").  By default samples are scored against samples;
`eval_mesh(mode="surface")` scores them against the other mesh itself, with the exact point-to-triangle distances of
vista_slam_amd.meshdist.  `pointmap_range_error` casts a ray from each view's camera centre through each of its predicted world points
and reads off, with meshdist's exact first hit, where along that ray the surface is.

What this is not: a comparison against evo, Open3D or pykdtree (none is available; ICP's loop and the alignment are restated from
their published definitions, tests/cloud_cases.py holds the numpy restatement they are tested against); no plots.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import cloud, formats


def _host(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    if isinstance(a, (list, tuple)):
        return np.stack([_host(v) for v in a], axis=0)
    return np.asarray(a)


def umeyama(x, y):
    """Sim(3) (R, t, c) minimising sum |y_i - (c R x_i + t)|^2 (Umeyama 1991, evo's `umeyama_alignment` with scale):
    cov = sum (y - mu_y)(x - mu_x)^T / n = U D V^T, S = diag(1, 1, sign(det U det V)), R = U S V^T, c = trace(D S) / var_x,
    t = mu_y - c R mu_x."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    mx, my = x.mean(axis=0), y.mean(axis=0)
    xc, yc = x - mx, y - my
    var_x = (xc * xc).sum() / n
    U, D, Vt = np.linalg.svd(yc.T @ xc / n)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    c = np.trace(np.diag(D) @ S) / var_x
    return R, my - c * (R @ mx), c


def align_traj(traj_est_all, traj_ref_all):
    """eval_traj.py:4-28.  Poses whose reference entry sums to NaN or Inf are dropped; the estimate is aligned to the reference with
    scale: aligned pose i = (R R_i, c R t_i + t).  -> r_a [3,3], t_a [3], s, est_aligned [n,4,4], ref [n,4,4] (float64 numpy)."""
    est_all, ref_all = _host(traj_est_all).astype(np.float64), _host(traj_ref_all).astype(np.float64)
    keep = [i for i in range(len(ref_all)) if np.isfinite(ref_all[i].sum())]
    if len(keep) < 3:
        raise ValueError(f"align_traj needs at least 3 poses with a finite reference (got {len(keep)})")
    est, ref = est_all[keep], ref_all[keep]
    r_a, t_a, s = umeyama(est[:, :3, 3], ref[:, :3, 3])
    aligned = est.copy()
    aligned[:, :3, :3] = r_a @ est[:, :3, :3]
    aligned[:, :3, 3] = s * (est[:, :3, 3] @ r_a.T) + t_a
    return r_a, t_a, float(s), aligned, ref


def ape_translation(est_aligned, ref):
    """evo's APE on PoseRelation.translation_part: the statistics of e_i = ||t_est_i - t_ref_i||."""
    e = np.linalg.norm(_host(est_aligned)[:, :3, 3].astype(np.float64) - _host(ref)[:, :3, 3].astype(np.float64), axis=1)
    return {"rmse": float(np.sqrt(np.mean(e * e))), "mean": float(np.mean(e)), "median": float(np.median(e)), "std": float(np.std(e)),
            "min": float(np.min(e)), "max": float(np.max(e)), "sse": float(np.sum(e * e))}


def full_traj_eval(traj_est, traj_ref, plot_parent_dir=None, plot_name=None):
    """eval_traj.py:62-75 without the plot (matplotlib and evo are absent; the two plot arguments are accepted and ignored).
    -> traj_est (aligned), traj_ref, r_a, t_a, s, ape_statistics."""
    r_a, t_a, s, est, ref = align_traj(traj_est, traj_ref)
    return est, ref, r_a, t_a, s, ape_translation(est, ref)


def eval_recon(frontend, gt_depths, gt_poses, gt_intri, est_depths, est_poses, est_intris, est_masks, rel_R, rel_t, rel_s, *,
               voxel_size: float = 0.05, max_corr: float = 0.1, max_error: float = 0.5, return_stages: bool = False):
    """eval_recon.py:108-178 on the device.
      1. world clouds through formats.world_pointcloud: gt keeps pixels with gt_depth > 0, est keeps est_mask & gt_mask (the masks
         go in as the confidence plane with threshold 0.5, scales of 1)
      2. est <- s R est + t
      3. both through formats.voxel_downsample(voxel_size)
      4. cloud.icp of the down-sampled est onto an index of the down-sampled gt (cell = max_corr, init = I)
      5. est <- T est, written as fp32 first, so that both chamfer directions see the same points (a stated difference: the
         reference keeps float64 points)
      6. cloud.chamfer(gt, est, max_error)
    -> rmse_acc, rmse_comp, chamfer_dist, gt_points, est_points (device tensors) [, the stages as a dict]."""
    dev = frontend.device
    gt_depths = torch.as_tensor(gt_depths).to(dev, torch.float32)
    N, H, W = gt_depths.shape
    est_depths = torch.as_tensor(est_depths).to(dev, torch.float32)
    est_masks = torch.as_tensor(est_masks).to(dev)
    gt_poses, est_poses = torch.as_tensor(gt_poses).to(dev, torch.float32), torch.as_tensor(est_poses).to(dev, torch.float32)
    if not (len(est_depths) == len(est_masks) == len(est_poses) == len(gt_poses) == N):
        raise ValueError("eval_recon: the view counts differ")
    gt_K = torch.as_tensor(gt_intri).to(dev, torch.float32)
    if gt_K.dim() == 2:
        gt_K = gt_K[None].expand(N, 3, 3)
    est_K = torch.as_tensor(est_intris).to(dev, torch.float32)
    if est_K.dim() == 2:
        est_K = est_K[None].expand(N, 3, 3)
    ones = torch.ones(N, device=dev)
    gt_mask = gt_depths > 0
    both = (est_masks.reshape(N, H, W) > 0) & gt_mask
    gt_pts, _ = formats.world_pointcloud(frontend, gt_depths, ones, gt_K, gt_poses, gt_mask.float(), None, 0.5)
    est_raw, _ = formats.world_pointcloud(frontend, est_depths, ones, est_K, est_poses, both.float(), None, 0.5)
    if gt_pts.shape[0] == 0 or est_raw.shape[0] == 0:
        raise ValueError("eval_recon: an empty cloud")
    sR = float(rel_s) * np.asarray(_host(rel_R), dtype=np.float64).reshape(3, 3)
    rel = np.concatenate([sR, np.asarray(_host(rel_t), dtype=np.float64).reshape(3, 1)], axis=1)
    est_pts = cloud.transform(est_raw, rel)
    est_down, _ = formats.voxel_downsample(frontend, est_pts, voxel_size=voxel_size)
    gt_down, _ = formats.voxel_downsample(frontend, gt_pts, voxel_size=voxel_size)
    reg = cloud.icp(est_down, cloud.NNIndex.build(gt_down, max_corr), max_corr)
    est_final = cloud.transform(est_pts, reg.T)
    ch = cloud.chamfer(gt_pts, est_final, max_error)
    out = (ch.rmse_1, ch.rmse_2, ch.chamfer, gt_pts, est_final)
    if return_stages:
        out += (dict(est_raw=est_raw, rel=rel, est_pts=est_pts, est_down=est_down, gt_down=gt_down, icp=reg),)
    return out


class MeshScore(NamedTuple):
    accuracy: float                # mean of min(d, max_error), estimate -> ground truth
    completion: float              # the same mean, ground truth -> estimate
    completion_ratio: float        # share of the ground-truth samples with d <= threshold
    precision: float               # share of the estimate's samples with d <= threshold
    fscore: float                  # 2 precision completion_ratio / (precision + completion_ratio), 0 when both are 0
    chamfer: float                 # (accuracy + completion) / 2
    est_points: torch.Tensor       # [n,3] f32, after T
    gt_points: torch.Tensor        # [n,3] f32 (the cloud itself when gt is a cloud)
    n_precise: int                 # the integer counts behind the two ratios
    n_complete: int
    T: Optional[np.ndarray] = None # [4,4] f64: the transform the estimate was scored under when refine= was given (None otherwise)


def eval_mesh(frontend, est_mesh, gt, *, n_samples: int = 200000, threshold: float = 0.05, max_error: float = 0.5, T=None, seed: int = 0,
              mode: str = "samples", refine: Optional[str] = None, refine_max_corr: Optional[float] = None,
              refine_min_cos: Optional[float] = None) -> MeshScore:
    """Score a mesh against a ground truth, samples against samples (mode="samples", the default).  gt: a `tsdf.Mesh`, the path of a PLY of `tsdf.write_mesh_ply`, or an
    [M,3] cloud (taken as it is, not sampled).
      1. n_samples points by area from the estimate with `seed`, from the ground-truth mesh with seed + 1 (surface.sample_surface)
      2. the estimate's samples moved by T ([3,4] or [4,4]; None = identity, not applied) through cloud.transform
      3. both directions of clipped nearest-neighbour distances from cloud.chamfer(gt, est, max_error, return_distances=True)
      4. means, counts of d <= threshold and the F-score, summed on the device in float64
    The clipped distance is cloud.chamfer's: sqrt(min(d^2, max_error^2)), and max_error for a sample without a neighbour within max_error
    or that is not finite (a mesh without area gives NaN samples: every one of them scores max_error).
    threshold > max_error is refused (every distance is clipped at max_error, so no sample could pass).
    mode="surface": the same samples with the same seeds (est_points and gt_points are those of the default mode), scored against the
    SURFACE: the estimate's samples against the ground-truth mesh, the ground truth's samples against the estimate's mesh (its vertices
    moved by T through cloud.transform, once), both as sqrt(min(d2, max_error^2)) of meshdist's exact point-to-triangle query with
    radius = max_error.  Scoring samples against samples has a floor of about one sample spacing even for identical surfaces; this has
    none.  When gt is a cloud there is no ground-truth surface: completion is the cloud against the estimate's mesh, accuracy stays the
    nearest-neighbour distance from the estimate's samples to the cloud, as in the default mode.
    refine="plane" | "point" (gt a mesh; refused for a cloud): before scoring, meshdist.icp registers the estimate's samples (as sampled,
    not yet moved) against the ground truth's SURFACE, starting at T, with max_corr = refine_max_corr (default max_error); with
    refine_min_cos the samples' face normals must agree with the matched triangle's to that cosine.  The refined transform replaces T in
    both modes and is returned in the last field; a score without it carries the residual misalignment of whatever fixed T in every
    number.  Without refine= nothing changes: the last field is None."""
    from . import surface, tsdf
    if not float(threshold) <= float(max_error):
        raise ValueError(f"eval_mesh: threshold must be <= max_error (got {threshold}, {max_error})")
    if mode not in ("samples", "surface"):
        raise ValueError(f"eval_mesh: mode must be 'samples' or 'surface' (got {mode!r})")
    if refine not in (None, "point", "plane"):
        raise ValueError(f"eval_mesh: refine must be None, 'point' or 'plane' (got {refine!r})")
    dev = getattr(frontend, "device", frontend)
    est_m = tsdf.Mesh(*[None if a is None else torch.as_tensor(a).to(dev) for a in est_mesh])
    if isinstance(gt, (str, os.PathLike)):
        gt = tsdf.mesh_from_ply(gt, dev)
    if refine is not None and not isinstance(gt, tsdf.Mesh):
        raise ValueError("eval_mesh: refine= registers against the ground truth's surface: gt must be a mesh, not a cloud")
    sampled = surface.sample_surface(est_m, n_samples, seed=seed, normals=refine is not None and refine_min_cos is not None)
    est = sampled.points
    gt_m = None
    if isinstance(gt, tsdf.Mesh):
        gt_m = tsdf.Mesh(*[None if a is None else torch.as_tensor(a).to(dev) for a in gt])
    T_used = None
    if refine is not None:
        from . import meshdist
        gt_index = meshdist.TriIndex.build(SimpleNamespace(vertices=gt_m.vertices, triangles=gt_m.triangles))
        reg = meshdist.icp(est, gt_index, float(max_error if refine_max_corr is None else refine_max_corr),
                           init=None if T is None else np.asarray(_host(T), dtype=np.float64), mode=refine,
                           normals=sampled.normals if refine_min_cos is not None else None, min_cos=refine_min_cos)
        T = T_used = reg.T
    if T is not None:
        est = cloud.transform(est, np.asarray(_host(T), dtype=np.float64)[:3])
    if gt_m is not None:
        gt_pts = surface.sample_surface(gt_m, n_samples, seed=int(seed) + 1).points
    else:
        gt_pts = torch.as_tensor(gt).to(dev, torch.float32).reshape(-1, 3).contiguous()
    if mode == "samples":
        ch = cloud.chamfer(gt_pts, est, max_error, return_distances=True)
        d_est, d_gt = ch.dist_1, ch.dist_2              # est -> gt, gt -> est
    else:
        from . import meshdist
        r2 = float(max_error) * float(max_error)

        def to_surface(points, verts, tris):
            d2, = meshdist.TriIndex.build(SimpleNamespace(vertices=verts, triangles=tris)).query(points, float(max_error), want=("d2",))
            return torch.sqrt(torch.clamp(d2, max=r2))
        est_v = est_m.vertices.to(torch.float32).contiguous()
        if T is not None:
            est_v = cloud.transform(est_v, np.asarray(_host(T), dtype=np.float64)[:3])
        d_gt = to_surface(gt_pts, est_v, est_m.triangles)
        if gt_m is not None:
            d_est = to_surface(est, gt_m.vertices, gt_m.triangles)
        else:
            d_est = cloud.chamfer(gt_pts, est, max_error, return_distances=True).dist_1
    thr = float(threshold)

    def score(d):
        n = len(d)
        return (float(d.sum().item()) / n if n else float("nan")), int((d <= thr).sum().item()), n
    acc, n_precise, n_est = score(d_est)
    comp, n_complete, n_gt = score(d_gt)
    precision = n_precise / n_est if n_est else float("nan")
    ratio = n_complete / n_gt if n_gt else float("nan")
    f = 2.0 * precision * ratio / (precision + ratio) if precision + ratio > 0 else (0.0 if precision + ratio == 0 else float("nan"))
    return MeshScore(acc, comp, ratio, precision, f, (acc + comp) / 2.0, est, gt_pts, n_precise, n_complete, T_used)


def mesh_depth_l1(frontend, est_mesh, gt_mesh, cameras, H: int, W: int, method: str = "raster"):
    """(mean |depth_est - depth_gt| over the pixels of `cameras` (render.Camera) that both meshes cover, the number of those pixels),
    through render.mesh_depth; NaN when there is no such pixel.  Plumbing: the triangle pass does the work.
    method="rays": the same over meshdist.ray_depth - the exact first hit along each pixel's ray instead of the rasteriser's vertices
    snapped to 1/256 pixel; one index per mesh, built once."""
    from . import render
    if method not in ("raster", "rays"):
        raise ValueError(f"mesh_depth_l1: method must be 'raster' or 'rays' (got {method!r})")
    if method == "rays":
        from . import meshdist
        dev = getattr(frontend, "device", frontend)
        index = [meshdist.TriIndex.build(SimpleNamespace(vertices=torch.as_tensor(m.vertices).to(dev), triangles=m.triangles)) for m in (est_mesh, gt_mesh)]
        depth = lambda which, mesh, cam: meshdist.ray_depth(index[which], cam, H, W)
    else:
        depth = lambda which, mesh, cam: render.mesh_depth(frontend, mesh, cam, H, W)
    total, count = 0.0, 0
    for cam in cameras:
        de, dg = depth(0, est_mesh, cam), depth(1, gt_mesh, cam)
        both = torch.isfinite(de) & torch.isfinite(dg)
        total += float((de.to(torch.float64) - dg.to(torch.float64)).abs()[both].sum().item())
        count += int(both.sum().item())
    return (total / count if count else float("nan")), count


class RangeError(NamedTuple):
    abs_mean: float                # mean of |t - 1| |d| over the rays that hit: the range error along the ray, in world units
    abs_median: float              # its lower median (torch.median's convention)
    rel_mean: float                # mean of |t - 1|: the same relative to the predicted range
    rel_median: float
    n_hit: int                     # valid rays that hit the mesh
    n_miss: int                    # valid rays that did not (or whose point is not finite, or lies at the centre)


def pointmap_range_error(frontend, mesh_or_index, centres, points, valid=None) -> RangeError:
    """The range error of predicted pointmaps against a mesh: from each view's camera centre (centres [V,3], world) a ray through each of
    its predicted world points (points [V,...,3]): o = the centre, d = float32(point - centre), so the prediction sits at t = 1 and the
    surface is where meshdist's first hit says, at t; the error along the ray is |t - 1| |d|.  valid [V,...] bool: the points that count
    (None = all).  mesh_or_index: a `tsdf.Mesh` or a `meshdist.TriIndex` of it.  The sums are float64 device reductions and the medians
    come from a device sort; ONE readback.  NaN statistics when no ray hits."""
    from . import meshdist
    dev = getattr(frontend, "device", frontend)
    index = mesh_or_index if isinstance(mesh_or_index, meshdist.TriIndex) else meshdist.TriIndex.build(
        SimpleNamespace(vertices=torch.as_tensor(mesh_or_index.vertices).to(dev), triangles=mesh_or_index.triangles))
    dev = index.device
    c = torch.as_tensor(_host(centres) if isinstance(centres, (list, tuple)) else centres).to(dev, torch.float32).reshape(-1, 3)
    p = torch.as_tensor(_host(points) if isinstance(points, (list, tuple)) else points).to(dev, torch.float32)
    if p.shape[-1] != 3 or p.shape[0] != len(c):
        raise ValueError(f"pointmap_range_error: points must be [V, ..., 3] for {len(c)} centres (got {tuple(p.shape)})")
    V = len(c)
    p = p.reshape(V, -1, 3)
    o = c[:, None, :].expand_as(p).reshape(-1, 3)
    d = (p.to(torch.float64) - c[:, None, :].to(torch.float64)).to(torch.float32).reshape(-1, 3)
    ok = torch.ones(len(d), dtype=torch.bool, device=dev) if valid is None else torch.as_tensor(valid).to(dev).reshape(-1).bool()
    if len(ok) != len(d):
        raise ValueError(f"pointmap_range_error: valid must have one entry per point ({len(d)}; got {len(ok)})")
    t, = index.cast(o, d, 0.0, float("inf"), want=("t",))
    hit = ok & torch.isfinite(t)
    rel = (t - 1.0).abs()
    dd = d.to(torch.float64)
    ab = rel * torch.sqrt((dd * dd).sum(dim=1))
    n_hit = hit.sum()
    mid = torch.clamp((n_hit - 1) // 2, min=0)
    inf = torch.full_like(rel, float("inf"))

    def stats(x):
        x = torch.where(hit, x, inf)
        return torch.where(hit, x, torch.zeros_like(x)).sum() / n_hit, torch.sort(x).values[mid]
    am, amed = stats(ab)
    rm, rmed = stats(rel)
    out = torch.stack([am, amed, rm, rmed, n_hit.to(torch.float64), (ok & ~hit).sum().to(torch.float64)]).cpu().tolist()          # the one readback
    nan = float("nan")
    n = int(out[4])
    return RangeError(*(out[:4] if n else [nan] * 4), n, int(out[5]))


def load_data(output_folder, load_view_graph=True, load_gt_depths=True, load_gt_poses=True, load_gt_intrinsic=True, load_unscaled_depths=True,
              load_scales=True, load_intrinsics=True, load_confs=True, load_poses=True):
    """eval_recon.py:7-35: what formats.save_data_all wrote, as a plain namespace (no munch)."""
    data = {}
    j = lambda name: os.path.join(output_folder, name)
    if load_view_graph:
        z = np.load(j("view_graph.npz"), allow_pickle=True)
        data["view_graph"] = z["view_graph"].item()
        data["loop_min_dist"] = z["loop_min_dist"].item()
        data["view_names"] = z["view_names"].tolist()
    if load_gt_depths:
        data["gt_depths"] = np.load(j("gt_depths.npy"))
    if load_gt_poses:
        data["gt_poses"] = np.load(j("gt_poses.npy"))
    if load_gt_intrinsic:
        data["gt_intrinsic"] = np.load(j("gt_intrinsics.npy"))
    if load_unscaled_depths:
        data["unscaled_depths"] = np.load(j("depths.npy"))
    if load_scales:
        data["scales"] = np.load(j("scales.npy"))[..., None]          # [N, 1, 1]
    if load_intrinsics:
        data["intrinsics"] = np.load(j("intrinsics.npy"))
    if load_confs:
        z = np.load(j("confs.npz"))
        data["confs"] = z["confs"]
        data["conf_thres"] = z["thres"].item()
    if load_poses:
        data["poses"] = np.load(j("trajectory.npy"))
    return SimpleNamespace(**data)


def eval_recon_from_saved_data(frontend, output_folder, rel_est_gt=None, **kwargs):
    """eval_recon.py:181-206.  rel_est_gt: None (align_traj of the saved poses) or [R, t, s]."""
    d = load_data(output_folder, load_view_graph=False)
    est_depths = (d.unscaled_depths * d.scales).astype(np.float32)
    est_masks = (d.confs > d.conf_thres).astype(np.float32)
    if rel_est_gt is not None:
        rel_R, rel_t, rel_s = rel_est_gt
    else:
        rel_R, rel_t, rel_s, _, _ = align_traj(d.poses, d.gt_poses)
    return eval_recon(frontend, d.gt_depths.astype(np.float32), d.gt_poses.astype(np.float32), d.gt_intrinsic, est_depths,
                      d.poses.astype(np.float32), d.intrinsics.astype(np.float32), est_masks, rel_R, rel_t, rel_s, **kwargs)


def eval_slam(slam, gt_poses, gt_depths=None, gt_intrinsic=None):
    """The metrics of a run held by an `OnlineSLAM`: -> dict(ape = the APE statistics, r_a, t_a, s) and, with the ground-truth
    depth maps and intrinsics, rmse_acc, rmse_comp and chamfer."""
    ex = slam.pose_graph.export(view_num=slam.view_num)
    est, ref, r_a, t_a, s, stats = full_traj_eval(ex.poses, gt_poses)
    out = {"ape": stats, "r_a": r_a, "t_a": t_a, "s": s}
    if gt_depths is not None:
        if gt_intrinsic is None:
            raise ValueError("eval_slam: gt_depths needs gt_intrinsic")
        N = ex.depths.shape[0]
        acc, comp, ch, _, _ = eval_recon(slam.frontend, gt_depths, gt_poses, gt_intrinsic, ex.depths * ex.scales.reshape(N, 1, 1), ex.poses,
                                         ex.intrinsics, ex.confs > slam.conf_thres, r_a, t_a, s)
        out.update(rmse_acc=acc, rmse_comp=comp, chamfer=ch)
    return out
