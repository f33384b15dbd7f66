"""Output step: the files `OnlineSLAM.save_data_all` writes (vista_slam/slam.py:338-421)
and the pose conversion of `regress_two_views` (slam.py:166), behind the same names, keys, dtypes and shapes, so
`eval/eval_recon.load_data` (vista_slam/eval/eval_recon.py:7-35) and `eval/eval_traj` read them unchanged.

Files: `trajectory[_postfix].npy [N,4,4]`, `scales[_postfix].npy [N,1]`, `images.npy [N,H,W,3]` in [0,1],
`depths.npy [N,H,W]` (unscaled), `confs.npz {confs [N,H,W], thres}`, `intrinsics.npy [N,3,3]`,
`view_graph.npz {view_graph (pickled dict), loop_min_dist, view_names}`, `pointcloud.ply`, `gt_*.npy`.
The only arithmetic (world point cloud, mat -> SE3) runs in libsta_mi355.so; the rest is formatting.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .sta_frontend import STAFrontend, _stream_ptr

PLY_RECORD = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
assert PLY_RECORD.itemsize == 27


def _dev(frontend, t, shape=None):
    t = torch.as_tensor(t).to(frontend.device, torch.float32).contiguous()
    if shape is not None:
        assert tuple(t.shape) == tuple(shape), f"expected shape {tuple(shape)}, got {tuple(t.shape)}"
    return t


def mat_to_se3(frontend: STAFrontend, pose: torch.Tensor) -> torch.Tensor:
    """pp.mat2SE3(pose).data (slam.py:166): [B,4,4] -> [B,7] = (tx,ty,tz,qx,qy,qz,qw)."""
    p = _dev(frontend, pose).reshape(-1, 4, 4)
    out = torch.empty(p.shape[0], 7, device=frontend.device, dtype=torch.float32)
    _lib.check(frontend.lib.sta_mat_to_se3(frontend._h, p.data_ptr(), p.shape[0], out.data_ptr(), frontend._stream()))
    return out


MAX_VOXEL_EXTENT = 1 << 21     # voxels per axis: three 21-bit fields make the 63-bit sort key
MAX_VOXEL_POINTS = (1 << 30) - 1


class VoxelPlan(NamedTuple):
    """What `sta_voxel_downsample` derives from the bounds of the kept points (`voxel_plan`)."""
    origin: Tuple[float, float, float]        # the grid's corner o
    index_min: Tuple[int, int, int]           # per axis (x, y, z): floor((bound - o) / voxel_size)
    index_max: Tuple[int, int, int]
    extent: Tuple[int, int, int]              # index_max - index_min + 1
    bits: Tuple[int, int, int]                # key bits per axis = bit length of extent - 1
    key_bits: int                             # their sum, <= 63
    passes: int                               # 8-bit sort passes = ceil(key_bits / 8); the call runs one more when it dropped
    #                                           non-finite points and key_bits is a multiple of 8 (their all-ones key needs a spare bit)


def voxel_plan(bounds_min, bounds_max, voxel_size, origin=None) -> VoxelPlan:
    """Host only: the grid of a `voxel_downsample` call whose finite points have the per-axis bounds `bounds_min` / `bounds_max`
    (fp32 values).  origin=None: o = double(min) - voxel_size * 0.5 (the rule Open3D documents for VoxelDownSample, restated from
    memory).  Raises ValueError with the message the library gives for a bad voxel_size, an index outside int32 and a grid wider
    than 2^21 voxels on an axis."""
    vs = float(voxel_size)
    if not (np.isfinite(vs) and vs > 0.0):
        raise ValueError("voxel_size must be finite and > 0 (got %g)" % vs)
    mn = np.asarray(bounds_min, dtype=np.float32).astype(np.float64).reshape(3)
    mx = np.asarray(bounds_max, dtype=np.float32).astype(np.float64).reshape(3)
    if not (np.isfinite(mn).all() and np.isfinite(mx).all() and (mn <= mx).all()):
        raise ValueError(f"bounds must be finite with min <= max (got {mn.tolist()} .. {mx.tolist()})")
    if origin is None:
        o = mn - vs * 0.5
    else:
        o = np.asarray(origin, dtype=np.float64).reshape(3)
        if not np.isfinite(o).all():
            raise ValueError("origin must be finite")
    lo, hi = np.floor((mn - o) / vs), np.floor((mx - o) / vs)
    for a in range(3):
        if not (lo[a] >= -2147483648.0 and hi[a] <= 2147483647.0):
            raise ValueError("voxel index outside int32 on axis %d: [%.17g, %.17g] at voxel_size %g" % (a, lo[a], hi[a], vs))
    ilo, ihi = [int(v) for v in lo], [int(v) for v in hi]
    ext = [ihi[a] - ilo[a] + 1 for a in range(3)]
    if max(ext) > MAX_VOXEL_EXTENT:
        raise ValueError("voxel grid too wide: %d x %d x %d voxels at voxel_size %g (at most %d per axis)"
                         % (ext[0], ext[1], ext[2], vs, MAX_VOXEL_EXTENT))
    bits = [(e - 1).bit_length() for e in ext]
    return VoxelPlan(tuple(float(v) for v in o), tuple(ilo), tuple(ihi), tuple(ext), tuple(bits), sum(bits), (sum(bits) + 7) // 8)


def voxel_downsample(frontend: STAFrontend, points, colors=None, *, voxel_size, origin=None, min_points: int = 1,
                     return_counts: bool = False, return_index: bool = False, return_inverse: bool = False,
                     want_records: bool = False):
    """The cloud fused on a voxel grid (sta_voxel_downsample; the contract is in include/sta_mi355.h): one row per occupied voxel
    with at least `min_points` points, in ascending (iz, iy, ix) order, holding the fp64 mean of its points and colours.

    points [M,3], colors [M,3] or None -> (points [V,3] fp32, colors [V,3] fp32 or None [, counts [V] int32] [, index [V,3] int32]
    [, inverse [M] int32, -1 for a dropped or filtered point] [, records [V] PLY_RECORD numpy array]), device tensors trimmed to
    V rows.  Points with a non-finite coordinate are dropped.  origin (three floats) fixes the grid's corner, so that two calls
    share one grid; by default the corner is min - voxel_size / 2.  ValueError for bad arguments and for a grid the library
    refuses (`voxel_plan` gives the same answer on the host)."""
    vs = float(voxel_size)
    if not (np.isfinite(vs) and vs > 0.0):
        raise ValueError("voxel_size must be finite and > 0 (got %g)" % vs)
    if int(min_points) < 1:
        raise ValueError(f"min_points must be >= 1 (got {int(min_points)})")
    pts = _dev(frontend, points)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [M, 3] (got {tuple(pts.shape)})")
    M = pts.shape[0]
    if M > MAX_VOXEL_POINTS:
        raise ValueError(f"voxel_downsample takes fewer than 2^30 points (got {M})")
    col = _dev(frontend, colors, (M, 3)) if colors is not None else None
    org = None
    if origin is not None:
        org = (C.c_double * 3)(*[float(v) for v in origin])
        if not all(np.isfinite(v) for v in org):
            raise ValueError("origin must be finite")
    dev = frontend.device
    out_p = torch.empty(M, 3, device=dev, dtype=torch.float32)
    out_c = torch.empty(M, 3, device=dev, dtype=torch.float32) if col is not None else None
    out_n = torch.empty(M, device=dev, dtype=torch.int32) if return_counts else None
    out_i = torch.empty(M, 3, device=dev, dtype=torch.int32) if return_index else None
    out_v = torch.empty(M, device=dev, dtype=torch.int32) if return_inverse else None
    rec = torch.empty(M * 27, device=dev, dtype=torch.uint8) if want_records else None
    cnt = (C.c_int64 * 2)(0, 0)

    def ptr(t):
        return t.data_ptr() if t is not None and t.numel() else None
    try:
        _lib.check(frontend.lib.sta_voxel_downsample(frontend._h, ptr(pts), ptr(col), M, vs, org, int(min_points), ptr(out_p), ptr(out_c),
                                                     ptr(out_n), ptr(out_i), ptr(out_v), ptr(rec), cnt, frontend._stream()))
    except _lib.StaError as e:
        if str(e).startswith(("voxel grid too wide", "voxel index outside int32")):
            raise ValueError(str(e)) from None
        raise
    V = cnt[0]
    res = [out_p[:V], out_c[:V] if out_c is not None else None]
    if return_counts:
        res.append(out_n[:V])
    if return_index:
        res.append(out_i[:V])
    if return_inverse:
        res.append(out_v)
    if want_records:
        res.append(np.frombuffer(rec[:V * 27].cpu().numpy().tobytes(), dtype=PLY_RECORD))
    return tuple(res)


def world_pointcloud(frontend: STAFrontend, depths, scales, intrinsics, poses, confs, imgs, conf_thres: float,
                     want_records: bool = False, counts=None, min_views: int = 0, voxel_size=None, voxel_origin=None,
                     min_points: int = 1, outlier=None):
    """slam.py:396-408 -> (points [M,3] fp32, colors [M,3] fp32 [, records [M] PLY_RECORD numpy array]).

    outlier: ("statistical", nb, ratio, radius) or ("radius", nb, radius) - the cloud, after the voxel step if there is one, without
    the points that vista_slam_amd.cloud.remove_statistical_outlier / remove_radius_outlier removes (the floaters); rows stay in order.

    counts [N,H,W] (geo.view_consistency_check) with min_views > 0: a pixel is kept iff conf > conf_thres AND counts >= min_views
    (the confidence of the other pixels is lowered to -inf on a copy before the same library call).  voxel_size: the cloud goes
    through one `voxel_downsample` call (voxel_origin, min_points as there) before it is returned: one row per occupied voxel.
    The defaults leave the output unchanged."""
    depths = _dev(frontend, depths)
    N, H, W = depths.shape
    scales = _dev(frontend, scales).reshape(N)
    K = _dev(frontend, intrinsics, (N, 3, 3))
    poses = _dev(frontend, poses, (N, 4, 4))
    confs = _dev(frontend, confs, (N, H, W))
    if counts is not None and min_views > 0:
        counts = torch.as_tensor(counts).to(frontend.device)
        assert tuple(counts.shape) == (N, H, W), f"expected counts of shape {(N, H, W)}, got {tuple(counts.shape)}"
        confs = torch.where(counts >= min_views, confs, torch.full_like(confs, float("-inf")))
    imgs = _dev(frontend, imgs, (N, 3, H, W)) if imgs is not None else None
    cap = N * H * W
    pts = torch.empty(cap, 3, device=frontend.device, dtype=torch.float32)
    col = torch.empty(cap, 3, device=frontend.device, dtype=torch.float32)
    rec = torch.empty(cap * 27, device=frontend.device, dtype=torch.uint8) if want_records and voxel_size is None else None
    cnt = C.c_int64(0)
    _lib.check(frontend.lib.sta_world_pointcloud(frontend._h, depths.data_ptr(), scales.data_ptr(), K.data_ptr(),
                                                 poses.data_ptr(), confs.data_ptr(),
                                                 imgs.data_ptr() if imgs is not None else None, N, H, W, float(conf_thres),
                                                 pts.data_ptr(), col.data_ptr(), rec.data_ptr() if rec is not None else None,
                                                 C.byref(cnt), frontend._stream()))
    M = cnt.value
    if voxel_size is not None:
        res = voxel_downsample(frontend, pts[:M], col[:M], voxel_size=voxel_size, origin=voxel_origin, min_points=min_points,
                               want_records=want_records)
    elif want_records:
        res = (pts[:M], col[:M], np.frombuffer(rec[:M * 27].cpu().numpy().tobytes(), dtype=PLY_RECORD))
    else:
        res = (pts[:M], col[:M])
    if outlier is not None and res[0].shape[0] > 0:
        from . import cloud
        kept, _mask = cloud.filter_outliers(res[0], outlier)
        res = (res[0][kept], res[1][kept]) + ((res[2][kept.cpu().numpy()],) if want_records else ())
    return res


def write_ply(path: str, records: np.ndarray):
    """Binary little-endian PLY of a coloured cloud with double coordinates - the layout Open3D's
    `write_point_cloud` produces for slam.py:405-408 (readable by `o3d.io.read_point_cloud`)."""
    assert records.dtype == PLY_RECORD
    header = ("ply\nformat binary_little_endian 1.0\ncomment Created by vista_slam_amd (Open3D layout)\n"
              f"element vertex {len(records)}\nproperty double x\nproperty double y\nproperty double z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(records.tobytes())


def read_ply(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        n = None
        while True:
            line = f.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                n = int(line.split()[-1])
            if line == "end_header":
                break
        return np.frombuffer(f.read(n * 27), dtype=PLY_RECORD)


def save_data_all(frontend: STAFrontend, output_folder: str, *, poses, scales, depths, confs, intrinsics, imgs,
                  conf_thres: float, view_graph: Optional[Dict[int, List[int]]] = None, loop_min_dist=None,
                  view_names: Optional[Sequence[str]] = None, save_view_graph=True, traj_name_postfix=None,
                  save_poses=True, save_images=True, save_scales=True, save_depths=True, save_intrinsics=True,
                  save_confs=True, save_ply=True, gt_poses=None, gt_depths=None, gt_intrinsics=None,
                  counts=None, min_views: int = 0, ply_voxel_size=None, ply_outlier=None, mesh_min_triangles=None, mesh_simplify_cell=None,
                  mesh_voxel_size=None):
    """Same switches and files as OnlineSLAM.save_data_all (slam.py:338-421).  poses [N,4,4] (rotation + translation
    of the best node's Sim3), scales [N,1], depths / confs [N,H,W], intrinsics [N,3,3], imgs [N,3,H,W] in [-1,1].
    counts / min_views: pointcloud.ply keeps only pixels that at least min_views neighbouring views agree with
    (world_pointcloud); ply_voxel_size: pointcloud.ply holds the cloud fused on a voxel grid of that size, one vertex per occupied
    voxel (voxel_downsample); every other file is unaffected.  mesh_voxel_size: additionally mesh.ply, the TSDF fusion of the same views at
    that voxel size (vista_slam_amd.tsdf.fuse, read back with tsdf.read_mesh_ply); without it every file is byte for byte what it was.
    mesh_min_triangles: that mesh without its connected components of fewer triangles (vista_slam_amd.surface.clean_mesh) - the floaters;
    without it mesh.ply is byte for byte what it was.  mesh_simplify_cell: that mesh, after the cleaning, simplified by vertex clustering on
    cells of that size (vista_slam_amd.simplify.simplify_mesh, quadric placement); without it mesh.ply is byte for byte what it was.
    ply_outlier: ("statistical", nb, ratio, radius) or ("radius", nb, radius) - pointcloud.ply, after the voxel step, without the points
    that filter of vista_slam_amd.cloud removes (world_pointcloud's `outlier`); without it every file is byte for byte what it was."""
    os.makedirs(output_folder, exist_ok=True)

    def host(t):
        return torch.as_tensor(t).detach().cpu().numpy()
    if save_view_graph:
        np.savez(f"{output_folder}/view_graph.npz", view_graph=view_graph, loop_min_dist=loop_min_dist,
                 view_names=list(view_names) if view_names is not None else None)
    post = f"_{traj_name_postfix}" if traj_name_postfix is not None else ""
    if save_poses:
        np.save(f"{output_folder}/trajectory{post}.npy", host(poses))
    if save_scales:
        np.save(f"{output_folder}/scales{post}.npy", host(scales))
    if save_images:
        images = (torch.as_tensor(imgs).detach().cpu().float().permute(0, 2, 3, 1) + 1.0) / 2.0
        np.save(f"{output_folder}/images.npy", images.numpy())
    if save_depths:
        np.save(f"{output_folder}/depths.npy", host(depths))
    if save_confs:
        np.savez(f"{output_folder}/confs.npz", confs=host(confs), thres=conf_thres)
    if save_intrinsics:
        np.save(f"{output_folder}/intrinsics.npy", host(intrinsics))
    if save_ply:
        _, _, records = world_pointcloud(frontend, depths, scales, intrinsics, poses, confs, imgs, conf_thres, want_records=True,
                                         counts=counts, min_views=min_views, voxel_size=ply_voxel_size, outlier=ply_outlier)
        write_ply(f"{output_folder}/pointcloud.ply", records)
    if mesh_voxel_size is not None:
        from . import tsdf
        mesh = tsdf.fuse(frontend, depths=depths, scales=scales, intrinsics=intrinsics, poses=poses, confs=confs, imgs=imgs, conf_thres=conf_thres,
                         counts=counts, min_views=min_views, voxel_size=mesh_voxel_size)
        if mesh_min_triangles is not None:
            from . import surface
            mesh = surface.clean_mesh(mesh, min_triangles=mesh_min_triangles)
        if mesh_simplify_cell is not None:
            from . import simplify
            mesh = simplify.simplify_mesh(mesh, mesh_simplify_cell)
        tsdf.write_mesh_ply(f"{output_folder}/mesh.ply", mesh)
    if gt_poses is not None:
        np.save(f"{output_folder}/gt_poses.npy", np.array(gt_poses).astype(np.float32))
    if gt_depths is not None:
        np.save(f"{output_folder}/gt_depths.npy", np.array(gt_depths).astype(np.float32))
    if gt_intrinsics is not None:
        np.save(f"{output_folder}/gt_intrinsics.npy", gt_intrinsics)
