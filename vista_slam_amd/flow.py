"""The keyframe gate on the GPU: Shi-Tomasi corners on the last keyframe, tracked into the current frame with pyramidal
Lucas-Kanade - what `vista_slam/flow_tracker.py` does per incoming frame with two OpenCV calls on the CPU.  With it a frame goes
camera -> `preprocess.process_image` -> gate -> `encode` without touching the host, apart from the one small readback the caller
branches on.

    slam.flow_tracker = flow.FlowTracker(slam.frontend, flow_thres)

The contract restates OpenCV's documented algorithms in integer and float64 terms and is written out in include/sta_mi355.h; the
yardstick is the numpy restatement tests/flow_cases.py.  It is not cv2, and keyframe decisions can differ from OpenCV's at the
margin.  Kernels: csrc/flow.h.  `plan` holds every size and refusal and needs no GPU; the three device calls (`sta_flow_pyramid`,
`sta_flow_corners`, `sta_flow_track`) take the caller's buffers: the library allocates nothing, copies nothing to the host and never
synchronises.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .sta_frontend import STAFrontend

MAX_FRAMES = 32
MAX_PIXELS = 1 << 21
WIN, MAX_LEVEL, MAX_ITER, EPS, MIN_EIG = 21, 3, 30, 0.01, 1e-4
MAX_CORNERS, QUALITY, MIN_DISTANCE, BLOCK_SIZE = 1000, 0.01, 8, 7


class Plan(NamedTuple):
    """The sizes of the gate at one frame size: `sizes[l]` = (H_l, W_l) and `offsets[l]` = byte offset of level l in a pyramid buffer
    of `pyramid_bytes`; `workspace_bytes` = the scratch `good_features` needs."""
    H: int
    W: int
    B: int
    win: int
    max_level: int
    max_corners: int
    levels: int
    sizes: Tuple[Tuple[int, int], ...]
    offsets: Tuple[int, ...]
    pyramid_bytes: int
    workspace_bytes: int


def plan(H: int, W: int, B: int = 1, win: int = WIN, max_level: int = MAX_LEVEL, max_corners: int = MAX_CORNERS) -> Plan:
    """Every size and refusal of the gate, on the host (`sta_flow_plan`; no GPU).  ValueError, with the numbers in the message, for
    H or W below 8, H * W above 2^21, B outside [1, 32], win even or outside [3, 21], max_level outside [0, 3], max_corners < 1."""
    out = (C.c_int64 * 16)()
    lib = _lib.load()
    if lib.sta_flow_plan(int(H), int(W), int(B), int(win), int(max_level), int(max_corners), out) != 0:
        raise ValueError((lib.sta_last_error() or b"sta_flow_plan failed").decode())
    n = int(out[0])
    return Plan(int(H), int(W), int(B), int(win), int(max_level), int(max_corners), n,
                tuple((int(out[1 + l]), int(out[5 + l])) for l in range(n)), tuple(int(out[9 + l]) for l in range(n)),
                int(out[13]), int(out[14]))


class Pyramid:
    """B pyramids in one uint8 device buffer [B, pyramid_bytes]; `level(l, b)` is a [H_l, W_l] view."""

    def __init__(self, plan_: Plan, buf: torch.Tensor):
        self.plan, self.buf = plan_, buf

    @property
    def B(self) -> int:
        return self.buf.shape[0]

    def level(self, l: int, b: int = 0) -> torch.Tensor:
        (h, w), o = self.plan.sizes[l], self.plan.offsets[l]
        return self.buf[b, o:o + h * w].view(h, w)

    def frame(self, b: int) -> "Pyramid":
        return Pyramid(self.plan._replace(B=1), self.buf[b:b + 1])


def _on_device(frontend: STAFrontend, t: torch.Tensor) -> bool:
    dev = frontend.device
    return t.device.type == dev.type and (dev.index is None or t.device.index == dev.index)


def _frames(frontend: STAFrontend, gray) -> torch.Tensor:
    """-> contiguous device tensor [B, H, W], uint8 or float32, of: a numpy / torch uint8 [H,W]; float32 [H,W] or [1,H,W]
    (`process_image(...)['gray']`); a [B,H,W] uint8 stack; or a list of such frames of one size."""
    if isinstance(gray, (list, tuple)):
        parts = [_frames(frontend, g) for g in gray]
        if not parts:
            raise ValueError(f"1 .. {MAX_FRAMES} frames per call (got 0)")
        if any(p.shape[0] != 1 or p.shape != parts[0].shape or p.dtype != parts[0].dtype for p in parts):
            raise ValueError("the frames of one call share a size and a dtype: " + ", ".join(f"{p.dtype} {tuple(p.shape[1:])}" for p in parts))
        return torch.cat(parts, 0)
    if isinstance(gray, np.ndarray):
        gray = torch.from_numpy(np.ascontiguousarray(gray))
    if not isinstance(gray, torch.Tensor) or gray.dtype not in (torch.uint8, torch.float32) or gray.dim() not in (2, 3):
        raise ValueError(f"a grey frame is uint8 [H,W] or float32 [H,W] / [1,H,W] (got {getattr(gray, 'dtype', type(gray).__name__)} "
                         f"{tuple(getattr(gray, 'shape', ()))})")
    if gray.dim() == 2:
        gray = gray.unsqueeze(0)
    if not _on_device(frontend, gray):
        gray = gray.to(frontend.device)
    return gray.contiguous()


def pyramid(frontend: STAFrontend, gray, win: int = WIN, max_level: int = MAX_LEVEL) -> Pyramid:
    """The pyramids of 1 .. 32 frames of one size (see `_frames` for what a frame may be) in one call."""
    src = _frames(frontend, gray)
    B, H, W = src.shape
    p = plan(H, W, B, win, max_level)
    buf = torch.empty(B, p.pyramid_bytes, device=frontend.device, dtype=torch.uint8)
    _lib.check(frontend.lib.sta_flow_pyramid(frontend._h, src.data_ptr(), 0 if src.dtype == torch.uint8 else 1, H, W, B, p.win, p.max_level,
                                             buf.data_ptr(), frontend._stream()))
    pyr = Pyramid(p, buf)
    pyr._keep = src              # the launches read the frames after this returns
    return pyr


def _level0(frontend: STAFrontend, image) -> Tuple[torch.Tensor, object]:
    if isinstance(image, Pyramid):
        return image.level(0, 0), image
    pyr = pyramid(frontend, image, WIN, 0)
    if pyr.B != 1:
        raise ValueError(f"good_features takes one frame (got {pyr.B})")
    return pyr.level(0, 0), pyr


def good_features(frontend: STAFrontend, image, max_corners: int = MAX_CORNERS, quality: float = QUALITY, min_distance: int = MIN_DISTANCE,
                  block_size: int = BLOCK_SIZE, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """image: one frame or a `Pyramid` (its level 0 is used).  -> (corners [max_corners, 2] float32 (x, y) in rank order, n [1] int32),
    both on the device: rows >= n are not written, and n is not read here.  workspace: a uint8 device tensor of at least
    `plan(H, W).workspace_bytes` to reuse between calls."""
    img, keep = _level0(frontend, image)
    H, W = img.shape
    p = plan(H, W, 1, WIN, 0, max_corners)
    if workspace is None:
        workspace = torch.empty(p.workspace_bytes, device=frontend.device, dtype=torch.uint8)
    corners = torch.empty(p.max_corners, 2, device=frontend.device, dtype=torch.float32)
    n = torch.empty(1, device=frontend.device, dtype=torch.int32)
    _lib.check(frontend.lib.sta_flow_corners(frontend._h, img.data_ptr(), H, W, p.max_corners, float(quality), int(min_distance), int(block_size),
                                             workspace.data_ptr(), workspace.numel(), corners.data_ptr(), n.data_ptr(), frontend._stream()))
    corners._keep = (keep, workspace)
    return corners, n


def track(frontend: STAFrontend, prev: Pyramid, nxt: Pyramid, pts: torch.Tensor, n: Optional[torch.Tensor] = None, max_iter: int = MAX_ITER,
          eps: float = EPS, min_eig: float = MIN_EIG) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The points pts [cap, 2] float32 (device) of the frame behind `prev` into each of the B frames behind `nxt`; n = a device int32
    count (`good_features`' second result) or None for all cap rows.  -> (next_pts [B, cap, 2] float32, status [B, cap] uint8,
    stats [B, 3] float64 = n, n_good, sum of the displacements), all on the device."""
    if prev.plan.sizes != nxt.plan.sizes or prev.plan.win != nxt.plan.win:
        raise ValueError(f"the two pyramids differ: {prev.plan.sizes} at win {prev.plan.win}, {nxt.plan.sizes} at win {nxt.plan.win}")
    if not isinstance(pts, torch.Tensor) or pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 2 or not pts.is_contiguous() \
            or not _on_device(frontend, pts):
        raise ValueError("pts is a contiguous float32 [n, 2] tensor on the frontend's device")
    if n is not None and (n.dtype != torch.int32 or n.numel() != 1 or not _on_device(frontend, n)):
        raise ValueError("n is one int32 on the frontend's device")
    p, B, cap, dev = prev.plan, nxt.B, pts.shape[0], frontend.device
    plan(p.H, p.W, B, p.win, p.max_level)
    out = torch.empty(B, cap, 2, device=dev, dtype=torch.float32)
    status = torch.empty(B, cap, device=dev, dtype=torch.uint8)
    stats = torch.empty(B, 3, device=dev, dtype=torch.float64)
    _lib.check(frontend.lib.sta_flow_track(frontend._h, prev.buf.data_ptr(), nxt.buf.data_ptr(), p.H, p.W, B, p.win, p.max_level,
                                           pts.data_ptr() if cap else None, None if n is None else n.data_ptr(), cap, int(max_iter),
                                           float(eps), float(min_eig), out.data_ptr() if cap else None, status.data_ptr() if cap else None,
                                           stats.data_ptr(), frontend._stream()))
    stats._keep = (prev, nxt, pts, n)
    return out, status, stats


class FlowTracker:
    """`vista_slam.flow_tracker.FlowTracker` on the GPU, with its surface: `reset()`, `initialize_keyframe(image)`,
    `compute_disparity(image, visualize=False) -> bool`.  An image is the numpy uint8 [H,W] the reference hands over, a device uint8
    tensor, or `process_image(...)['gray']`.  The keyframe's pyramid and corners stay on the device; on a keyframe the current frame's
    pyramid becomes the keyframe's and is not rebuilt.  Every `compute_disparity` after the first reads three doubles back once; the
    mean displacement is float64 (float32 in the reference)."""

    def __init__(self, frontend: STAFrontend, min_disparity: float):
        self.frontend = frontend
        self.min_disparity = float(min_disparity)
        self._ws = None
        self.reset()

    def reset(self):
        self.kf_pyr = None
        self.kf_pts = None
        self.kf_n = None
        self.last = None                    # (n_pts, n_good, sum) of the most recent tracked call

    def _set_keyframe(self, pyr: Pyramid):
        p = plan(pyr.plan.H, pyr.plan.W)
        if self._ws is None or self._ws.numel() < p.workspace_bytes:
            self._ws = torch.empty(p.workspace_bytes, device=self.frontend.device, dtype=torch.uint8)
        self.kf_pyr = pyr
        self.kf_pts, self.kf_n = good_features(self.frontend, pyr, workspace=self._ws)

    def initialize_keyframe(self, image):
        self._set_keyframe(pyramid(self.frontend, image))

    def compute_disparity(self, image, visualize: bool = False) -> bool:
        if visualize:
            raise NotImplementedError("visualize=True draws with OpenCV on the host; the GPU gate has no drawing path")
        if self.kf_pyr is None:
            self.initialize_keyframe(image)
            return True
        cur = pyramid(self.frontend, image)
        if cur.plan.sizes != self.kf_pyr.plan.sizes:
            raise ValueError(f"frame of {cur.plan.H} x {cur.plan.W} after a keyframe of {self.kf_pyr.plan.H} x {self.kf_pyr.plan.W}")
        _, _, stats = track(self.frontend, self.kf_pyr, cur, self.kf_pts, self.kf_n)
        n_pts, n_good, total = stats[0].tolist()                      # THE readback of the call
        self.last = (int(n_pts), int(n_good), total)
        if n_pts < 10 or n_good < 10 or total / n_good > self.min_disparity:
            self._set_keyframe(cur)
            return True
        return False

    def disparities(self, images) -> List[Tuple[int, float]]:
        """Track the keyframe's corners into up to 32 frames in one call, without changing state: (n_good, mean displacement) per
        frame (mean = nan without a tracked point).  Offline callers scan ahead for the next keyframe with it."""
        if self.kf_pyr is None:
            raise RuntimeError("disparities() needs a keyframe: call initialize_keyframe or compute_disparity first")
        cur = pyramid(self.frontend, images)
        _, _, stats = track(self.frontend, self.kf_pyr, cur, self.kf_pts, self.kf_n)
        return [(int(g), t / g if g else float("nan")) for _, g, t in stats.tolist()]
