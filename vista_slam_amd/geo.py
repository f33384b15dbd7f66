"""Geometric consistency of depth maps: the reference's `view_consistency_check` and
`compute_symmetric_geo_valid_mask` (vista_slam/utils/slam_utils.py:269-419) behind the same names and argument order, with the
frontend in front.  All arithmetic runs in libsta_mi355.so (csrc/geo.h): one launch sequence per call, no host round trip.

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
