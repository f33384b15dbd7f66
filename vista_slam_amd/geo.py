"""Geometric consistency of depth maps: the reference's `view_consistency_check` and
`compute_symmetric_geo_valid_mask` (vista_slam/utils/slam_utils.py:269-419) behind the same names and argument order, with the
frontend in front.  All arithmetic runs in libsta_mi355.so (csrc/geo.h): one launch sequence per call, no host round trip.

Row f6 serves the rest of slam_utils.py: `compute_geo_valid_mask_batched` (:193-266, the general two-view check with one quantile
threshold over the batch), `compute_local_pointclouds` (:82-121) and `depth_from_pointcloud_dot_batched` (:124-165).

Where the reference's code and docstring disagree the code is the definition: the vote looks +-4 views away (`window=4`), divides
by the unclamped third coordinate, and lets a point behind a neighbour agree when it samples the zero padding.
"""
from __future__ import annotations

import torch

from . import _lib
from .sta_frontend import STAFrontend


def _dev(frontend, t, shape=None):
    t = torch.as_tensor(t).to(frontend.device, torch.float32).contiguous()
    if shape is not None:
        assert tuple(t.shape) == tuple(shape), f"expected shape {tuple(shape)}, got {tuple(t.shape)}"
    return t


def view_consistency_check(frontend: STAFrontend, depth, intrinsics, poses, threshold: float = 0.05, window: int = 4) -> torch.Tensor:
    """slam_utils.py:346-419: depth [n,H,W], intrinsics [n,3,3], poses [n,4,4] camera-to-world -> count_map [n,H,W] int32, the
    number of views j in [i-window, i+window] \\ {i} whose depth, sampled bilinearly at the reprojection of pixel (i, y, x),
    lies within `threshold` of the reprojected depth."""
    depth = _dev(frontend, depth)
    assert depth.dim() == 3, "depth must be [n,H,W]"
    n, H, W = depth.shape
    K = _dev(frontend, intrinsics, (n, 3, 3))
    poses = _dev(frontend, poses, (n, 4, 4))
    out = torch.empty(n, H, W, device=frontend.device, dtype=torch.int32)
    _lib.check(frontend.lib.sta_view_consistency(frontend._h, depth.data_ptr(), K.data_ptr(), poses.data_ptr(), n, H, W,
                                                 float(threshold), int(window), out.data_ptr(), frontend._stream()))
    return out


def symmetric_geo_valid_masks(frontend: STAFrontend, depths, K, poses, return_thres: bool = False, k_on_transposed: bool = False):
    """`compute_symmetric_geo_valid_mask` for P edges in one call, in the layout of a scheduler result (`regress_views`):
    depths [P,2,H,W], K [P,3,3] (shared by the pair), poses [P,4,4] (pose_ij: view 0 -> view 1) -> masks [P,2,H,W] bool
    (and the thresholds [P,2] = 2 * median error per direction, 1e10 for a direction with no pixel inside the other view).

    k_on_transposed: for portrait frames (H > W) of the scheduler, whose K is the one the reference computes on the TRANSPOSED
    views its head wrapper returns: the masks are computed on contiguous copies of those views and returned in image orientation."""
    depths = _dev(frontend, depths)
    assert depths.dim() == 4 and depths.shape[1] == 2, "depths must be [P,2,H,W]"
    P = depths.shape[0]
    K = _dev(frontend, K, (P, 3, 3))
    poses = _dev(frontend, poses, (P, 4, 4))
    transposed = bool(k_on_transposed) and depths.shape[2] > depths.shape[3]
    if transposed:
        depths = depths.transpose(2, 3).contiguous()
    H, W = depths.shape[2:]
    mask = torch.empty(P, 2, H, W, device=frontend.device, dtype=torch.uint8)
    thres = torch.empty(P, 2, device=frontend.device, dtype=torch.float32) if return_thres else None
    _lib.check(frontend.lib.sta_symmetric_geo_mask(frontend._h, depths.data_ptr(), K.data_ptr(), poses.data_ptr(), P, H, W,
                                                   mask.data_ptr(), thres.data_ptr() if thres is not None else None,
                                                   frontend._stream()))
    mask = mask.bool()
    if transposed:
        mask = mask.transpose(2, 3).contiguous()
    return (mask, thres) if return_thres else mask


def compute_symmetric_geo_valid_mask(frontend: STAFrontend, depths, intri, relative_pose) -> torch.Tensor:
    """slam_utils.py:269-343: depths [2,H,W], intri [3,3], relative_pose [4,4] (cam 1 -> cam 2) -> [2,H,W] bool, the forward
    and the backward valid-pixel mask."""
    depths = torch.as_tensor(depths)
    assert depths.dim() == 3 and depths.shape[0] == 2, "depths must be [2,H,W]"
    return symmetric_geo_valid_masks(frontend, depths[None], torch.as_tensor(intri)[None], torch.as_tensor(relative_pose)[None])[0]


def geo_valid_masks(frontend: STAFrontend, depth1, depth2, K1, K2, T1, T2, error_thres_rel: float, return_thres: bool = False):
    """`compute_geo_valid_mask_batched` without its host round trip: depth1, depth2 [B,H,W], K1, K2 [B,3,3], T1, T2 [B,4,4]
    (camera-to-world) -> mask [B,H,W] bool = pixel of view 1 lands inside view 2 && |z2 - depth2 there| < torch.quantile(such errors
    of the WHOLE batch, error_thres_rel).  return_thres: also the threshold (0-dim fp32) and the number of valid pixels (0-dim
    int32) as device tensors; with no valid pixel they are NaN and 0 and the mask is all False (nothing is raised here)."""
    depth1 = _dev(frontend, depth1)
    assert depth1.dim() == 3, "depth1 must be [B,H,W]"
    B, H, W = depth1.shape
    depth2 = _dev(frontend, depth2, (B, H, W))
    K1, K2 = _dev(frontend, K1, (B, 3, 3)), _dev(frontend, K2, (B, 3, 3))
    T1, T2 = _dev(frontend, T1, (B, 4, 4)), _dev(frontend, T2, (B, 4, 4))
    mask = torch.empty(B, H, W, device=frontend.device, dtype=torch.uint8)
    thres = torch.empty((), device=frontend.device, dtype=torch.float32) if return_thres else None
    count = torch.empty((), device=frontend.device, dtype=torch.int32) if return_thres else None
    _lib.check(frontend.lib.sta_geo_valid_mask(frontend._h, depth1.data_ptr(), depth2.data_ptr(), K1.data_ptr(), K2.data_ptr(),
                                               T1.data_ptr(), T2.data_ptr(), B, H, W, float(error_thres_rel), mask.data_ptr(),
                                               thres.data_ptr() if return_thres else None,
                                               count.data_ptr() if return_thres else None, frontend._stream()))
    mask = mask.bool()
    return (mask, thres, count) if return_thres else mask


def compute_geo_valid_mask_batched(frontend: STAFrontend, depth1, depth2, K1, K2, T1, T2, error_thres_rel) -> torch.Tensor:
    """slam_utils.py:193-266 -> [B,H,W] bool.  Like the reference (whose boolean indexing synchronises, and whose quantile raises
    on an empty input) this reads the number of valid pixels and raises RuntimeError when there is none."""
    mask, _thres, count = geo_valid_masks(frontend, depth1, depth2, K1, K2, T1, T2, error_thres_rel, return_thres=True)
    if int(count.item()) == 0:
        raise RuntimeError("quantile() input tensor must be non-empty: no pixel of view 1 lands inside view 2")
    return mask


def _intrinsics(frontend, intrinsics, n):
    K = torch.as_tensor(intrinsics)
    if K.dim() not in (2, 3):
        raise ValueError(f"Unsupported intrinsics shape: {tuple(K.shape)}")
    return _dev(frontend, K, (3, 3) if K.dim() == 2 else (n, 3, 3)), int(K.dim() == 3)


def compute_local_pointclouds(frontend: STAFrontend, depths, intrinsics) -> torch.Tensor:
    """slam_utils.py:82-121: depths [N,H,W], intrinsics [3,3] or [N,3,3] -> [N,H,W,3] = K^-1 [x, y, 1] * depth."""
    depths = _dev(frontend, depths)
    assert depths.dim() == 3, "depths must be [N,H,W]"
    N, H, W = depths.shape
    K, batched = _intrinsics(frontend, intrinsics, N)
    out = torch.empty(N, H, W, 3, device=frontend.device, dtype=torch.float32)
    _lib.check(frontend.lib.sta_local_pointclouds(frontend._h, depths.data_ptr(), K.data_ptr(), batched, N, H, W, out.data_ptr(),
                                                  frontend._stream()))
    return out


def depth_from_pointcloud_dot_batched(frontend: STAFrontend, pointclouds, intrinsics) -> torch.Tensor:
    """slam_utils.py:124-165: pointclouds [B,H,W,3], intrinsics [3,3] or [B,3,3] -> [B,H,W], each point's dot product with the
    unit ray of its pixel."""
    pts = _dev(frontend, pointclouds)
    assert pts.dim() == 4 and pts.shape[3] == 3, "pointclouds must be [B,H,W,3]"
    B, H, W, _ = pts.shape
    K, batched = _intrinsics(frontend, intrinsics, B)
    out = torch.empty(B, H, W, device=frontend.device, dtype=torch.float32)
    _lib.check(frontend.lib.sta_ray_depth(frontend._h, pts.data_ptr(), K.data_ptr(), batched, B, H, W, out.data_ptr(),
                                          frontend._stream()))
    return out
