"""Look at a map without a display: a headless z-buffer rasteriser for points and line segments on the GPU, and what the reference's
scripts/video.py and scripts/vis_slam_results.py draw with it - the coloured cloud, camera frusta, the trajectory, the view graph.

The rasteriser is libsta_raster.so (include/sta_raster.h holds the contract, tests/render_cases.py restates it in numpy): every fragment
is a 64-bit key (depth bits, then colour or id) merged with an integer atomic minimum, so an image is defined bit for bit whatever
order the hardware runs the points in.  The same key buffer gives the colour image, a depth map of the fused map from any pose, and an
id image (which point is visible at each pixel).  Cameras and the line geometry are host float64 numpy: they have no hot path.

Triangles come from a library of their own, libsta_mesh.so (include/sta_mesh.h, restated in tests/mesh_cases.py): `Canvas.mesh` draws an
indexed mesh - a `tsdf.Mesh` - into the same key buffer with exact integer coverage on a 1/256-pixel grid, a near-plane clip and
perspective-correct depth and colour, so the mesh, the cloud and the lines occlude each other in any issue order; `render_mesh`,
`mesh_depth` and `render_folder(mesh=)` sit on it.

Not here: Open3D, rerun, a live window; text; round or anti-aliased points (footprints are squares, smoothing is box supersampling); GL's
diamond-exit line rule (the DDA of the header instead); for triangles: far-plane and 2-D polygon clipping (a per-fragment far test and a
drop beyond 2^28 sub-pixels instead), smooth shading (one two-sided light factor per face), textures, transparency.  DESIGN.md section 9.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import struct
import zlib
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_DIM = 8192
MAX_SIZE = 8
MIN_NEAR, MAX_FAR = 1e-30, 1e30
# scripts/video.py:46-48, as bytes
CAMERA_COLOR = (153, 204, 255)
CUR_CAMERA_COLOR = (19, 80, 27)
NEIGHBOR_EDGE_COLOR = (0, 0, 255)
LOOP_EDGE_COLOR = (255, 128, 0)
TRAJECTORY_COLOR = (220, 30, 30)
MESH_COLOR = (200, 200, 200)
MESH_MODES = {"shaded": 1, "color": 1, "normal": 2, "id": 0}          # -> STA_MESH_PAYLOAD_*
MESH_CULL = {"none": 0, "back": 1, "front": 2}
MESH_COUNTERS = ("seen", "bad", "behind", "clipped", "too_large", "degenerate", "culled", "off_canvas")
FRUSTUM_LINES = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1))


class Plan(NamedTuple):
    key_bytes: int
    Hs: int
    Ws: int


def plan(H: int, W: int, ssaa: int = 1) -> Plan:
    """Host only, no library needed: what sta_raster_plan reports (tests compare the two) and its refusals as ValueError."""
    H, W, ssaa = int(H), int(W), int(ssaa)
    if H < 1 or W < 1:
        raise ValueError(f"raster_plan: H and W must be >= 1 (got {H} x {W})")
    if ssaa not in (1, 2, 4):
        raise ValueError(f"raster_plan: ssaa must be 1, 2 or 4 (got {ssaa})")
    if H * ssaa > MAX_DIM or W * ssaa > MAX_DIM:
        raise ValueError(f"raster_plan: {H} x {W} at ssaa {ssaa} is a key buffer of {H * ssaa} x {W * ssaa}, at most {MAX_DIM} per axis")
    return Plan(H * ssaa * W * ssaa * 8, H * ssaa, W * ssaa)


def _value_error(e: _lib.StaError):
    return ValueError(str(e)) if str(e).startswith(("raster_", "mesh_")) else e


def _host(a, dtype=np.float64):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=dtype)


def _normalise(v):
    n = np.linalg.norm(v)
    if not n > 0:
        raise ValueError(f"a zero-length direction: {v}")
    return v / n


class Camera:
    """A pinhole camera: K (fx, fy, cx, cy in output pixels; a pixel's centre is at its integer coordinate) and a world-to-camera matrix,
    x right, y down, z forward.  Host float64."""

    def __init__(self, K, w2c, near: float = 1e-3, far: float = 1e4):
        K = _host(K)
        self.K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) if K.shape == (3, 3) else K.reshape(4).copy()
        w2c = _host(w2c)
        if w2c.shape == (4, 4):
            w2c = w2c[:3]
        if w2c.shape != (3, 4):
            raise ValueError(f"w2c must be 3x4 or 4x4 (got {w2c.shape})")
        self.w2c = w2c.copy()
        self.near, self.far = float(near), float(far)

    @staticmethod
    def look_at(eye, target, up, fx: float, fy: float, H: int, W: int, near: float = 1e-3, far: float = 1e4) -> "Camera":
        """The camera at `eye` whose axis goes through `target` and in whose image the world direction `up` points up; the principal
        point is the canvas centre ((W - 1) / 2, (H - 1) / 2)."""
        eye, target, up = _host(eye).reshape(3), _host(target).reshape(3), _host(up).reshape(3)
        z = _normalise(target - eye)
        x = _normalise(np.cross(z, up))                # to the right when y points down
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        return Camera([fx, fy, (W - 1) / 2.0, (H - 1) / 2.0], np.concatenate([R, (-R @ eye)[:, None]], axis=1), near, far)

    @staticmethod
    def from_pose(c2w, K, offset=None, near: float = 1e-3, far: float = 1e4) -> "Camera":
        """The camera of a camera-to-world pose; offset (4x4): `pose_offset @ extrinsic` of scripts/video.py:120-131, a view from behind."""
        w2c = np.linalg.inv(_host(c2w).reshape(4, 4))
        if offset is not None:
            w2c = _host(offset).reshape(4, 4) @ w2c
        return Camera(K, w2c, near, far)

    @staticmethod
    def fit(points_or_poses, H: int, W: int, direction: str = "topdown", fov_deg: float = 60.0, margin: float = 1.15) -> "Camera":
        """A camera that sees a set of points [N,3] or of camera-to-world poses [N,4,4] (their centres).  The world is the first camera's
        frame (y down, z forward): "topdown" looks along +y with +z up in the image, "oblique" looks forward and 45 degrees down."""
        p = _host(points_or_poses)
        p = p.reshape(-1, 4, 4)[:, :3, 3] if p.ndim == 3 or p.shape[-1] == 4 else p.reshape(-1, 3)
        p = p[np.isfinite(p).all(axis=1)]
        if len(p) == 0:
            raise ValueError("Camera.fit: no finite point")
        lo, hi = p.min(axis=0), p.max(axis=0)
        centre = (lo + hi) / 2.0
        radius = max(float(np.linalg.norm(hi - lo)) / 2.0, 1e-3)
        if direction == "topdown":
            d, up = np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
        elif direction == "oblique":
            d, up = _normalise(np.array([0.0, 1.0, 1.0])), np.array([0.0, -1.0, 0.0])
        else:
            raise ValueError(f'direction must be "topdown" or "oblique" (got {direction!r})')
        half = np.deg2rad(fov_deg) / 2.0
        f = 0.5 * min(H, W) / np.tan(half)
        dist = margin * radius / np.sin(half)
        return Camera.look_at(centre - d * dist, centre, up, f, f, H, W, near=max(1e-3, dist * 1e-3), far=(dist + radius) * 4.0)

    def _args(self):
        return (C.c_double * 12)(*self.w2c.reshape(12).tolist()), (C.c_double * 4)(*self.K.tolist()), self.near, self.far


# ------------------------------------------------------------------------------------------ line geometry (host, float64 -> float32)
def camera_segments(poses, intrinsics, size, scale: float) -> np.ndarray:
    """[N*8,2,3] float32: per camera the eight segments of Open3D's create_camera_visualization as scripts/video.py keeps them (lines[:8]):
    the centre to the four corners of a `size` = (width_px, height_px) image at depth `scale`, and the rectangle."""
    poses = _host(poses).reshape(-1, 4, 4)
    Ks = np.broadcast_to(_host(intrinsics), (len(poses), 3, 3))
    w, h = float(size[0]), float(size[1])
    corners = np.array([[0, 0, 1], [w, 0, 1], [w, h, 1], [0, h, 1]], dtype=np.float64)
    out = np.zeros((len(poses), 8, 2, 3))
    for n, (c2w, K) in enumerate(zip(poses, Ks)):
        local = np.concatenate([np.zeros((1, 3)), (np.linalg.inv(K) @ corners.T).T * float(scale)])
        world = local @ c2w[:3, :3].T + c2w[:3, 3]
        for e, (i, j) in enumerate(FRUSTUM_LINES):
            out[n, e, 0], out[n, e, 1] = world[i], world[j]
    return out.reshape(-1, 2, 3).astype(np.float32)


def trajectory_segments(poses) -> np.ndarray:
    c = _host(poses).reshape(-1, 4, 4)[:, :3, 3]
    return np.stack([c[:-1], c[1:]], axis=1).astype(np.float32)


def view_graph_segments(view_graph: Dict[int, Sequence[int]], poses, loop_min_dist: int, upto: Optional[int] = None):
    """scripts/video.py:162-188 for every view v (< upto): an edge to each neighbour nv <= v; orange when |v - nv| >= loop_min_dist, else
    blue.  -> (segments [S,2,3] float32, colours [S,3] uint8)"""
    c = _host(poses).reshape(-1, 4, 4)[:, :3, 3]
    segs, cols = [], []
    for v in sorted(view_graph):
        if upto is not None and v >= upto:
            continue
        for nv in view_graph[v]:
            if nv > v:
                continue
            segs.append(np.stack([c[v], c[nv]]))
            cols.append(LOOP_EDGE_COLOR if abs(v - nv) >= loop_min_dist else NEIGHBOR_EDGE_COLOR)
    return np.asarray(segs, dtype=np.float32).reshape(-1, 2, 3), np.asarray(cols, dtype=np.uint8).reshape(-1, 3)


# ------------------------------------------------------------------------------------------ the canvas
class Canvas:
    """A key buffer on the device and the calls that draw into it.  The buffer and the counters are allocated once, here; `clear` and
    the drawing methods allocate nothing when they are given contiguous device tensors of the entry point's dtype (anything else - a host
    array, another dtype - is converted first, which allocates and, for host data, waits for the copy); `image`, `depth` and `ids` each
    allocate the tensor they return.  Every call is enqueued on the current stream of the canvas's device."""

    def __init__(self, device, H: int, W: int, ssaa: int = 1):
        self.plan = plan(H, W, ssaa)
        self.H, self.W, self.ssaa = int(H), int(W), int(ssaa)
        self.device = torch.device(device)
        self.lib = _lib.load_raster()
        self.keys = torch.empty(self.plan.Hs, self.plan.Ws, dtype=torch.int64, device=self.device)      # uint64 bit patterns
        self._counters = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._mesh_counters = torch.zeros(len(MESH_COUNTERS), dtype=torch.int64, device=self.device)
        self._mesh_work = None                     # the triangle pass's list of large pieces: grown on demand, kept
        self.clear()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc):
        try:
            _lib.check_raster(rc)
        except _lib.StaError as e:
            raise _value_error(e) from None

    def _dev(self, a, dtype, tail):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        t = t.to(self.device, dtype).contiguous()
        if tuple(t.shape[1:]) != tail:
            raise ValueError(f"expected a tensor of shape [n, {', '.join(map(str, tail))}] (got {tuple(t.shape)})")
        return t

    def clear(self):
        self._counters.zero_()
        self._mesh_counters.zero_()
        self._check(self.lib.sta_raster_clear(self.keys.data_ptr(), self.H, self.W, self.ssaa, self._stream()))
        return self

    def points(self, camera: Camera, points, colors=None, point_size: int = 1, id_base: int = 0):
        """points [M,3]; colors None (the payload is the point's id, id_base + i), [M,3] uint8, or [M,3] floating point in [0, 1]."""
        pts = self._dev(points, torch.float32, (3,))
        kind, col = 0, None
        if colors is not None:
            is_u8 = (colors.dtype == torch.uint8) if isinstance(colors, torch.Tensor) else (np.asarray(colors).dtype == np.uint8)
            kind = 1 if is_u8 else 2
            col = self._dev(colors, torch.uint8 if is_u8 else torch.float32, (3,))
            if len(col) != len(pts):
                raise ValueError(f"{len(pts)} points but {len(col)} colours")
        T, K, near, far = camera._args()
        self._check(self.lib.sta_raster_points(self.keys.data_ptr(), self.H, self.W, self.ssaa, pts.data_ptr(), col.data_ptr() if col is not None else None,
                                               kind, int(id_base), len(pts), T, K, near, far, int(point_size), self._counters.data_ptr(), self._stream()))
        return self

    def lines(self, camera: Camera, segments, colors, line_width: int = 1):
        """segments [S,2,3] world coordinates; colors [S,3] uint8, or one colour (3 values) for all."""
        segs = self._dev(segments, torch.float32, (2, 3))
        if not isinstance(colors, torch.Tensor) and np.asarray(colors).ndim == 1:
            colors = np.tile(np.asarray(colors, dtype=np.uint8), (len(segs), 1))
        col = self._dev(colors, torch.uint8, (3,))
        if len(col) != len(segs):
            raise ValueError(f"{len(segs)} segments but {len(col)} colours")
        T, K, near, far = camera._args()
        self._check(self.lib.sta_raster_lines(self.keys.data_ptr(), self.H, self.W, self.ssaa, segs.data_ptr(), col.data_ptr(), len(segs), T, K, near, far,
                                              int(line_width), self._stream()))
        return self

    def mesh(self, camera: Camera, mesh_or_verts, triangles=None, colors=None, mode: str = "shaded", cull: str = "none", ambient: float = 0.3,
             color=MESH_COLOR, id_base: int = 0):
        """A `tsdf.Mesh` (its colours are used unless `colors` is given), or vertices [nv,3] with triangles [nt,3] int32 and optional
        colours [nv,3] floating point in [0, 1].  mode "color": the vertex colours, perspective-correct (without colours: `color`, three
        bytes, everywhere); "shaded": the same times a two-sided light factor per face, ambient + (1 - ambient) |cos|, with the light at
        the camera's centre; "normal": the face normal as a colour; "id": id_base + the triangle's index (`ids()`).  cull "back" does not
        draw the faces seen from behind (a top-down camera then looks into a room through its ceiling), "front" the others."""
        if mode not in MESH_MODES:
            raise ValueError(f"mode must be one of {sorted(MESH_MODES)} (got {mode!r})")
        if cull not in MESH_CULL:
            raise ValueError(f"cull must be one of {sorted(MESH_CULL)} (got {cull!r})")
        if triangles is None:
            verts, triangles, colors = mesh_or_verts.vertices, mesh_or_verts.triangles, (mesh_or_verts.colors if colors is None else colors)
        else:
            verts = mesh_or_verts
        verts, tris = self._dev(verts, torch.float32, (3,)), self._dev(triangles, torch.int32, (3,))
        kind = MESH_MODES[mode]
        col = uni = light = None
        if kind == 1:
            if colors is not None:
                col = self._dev(colors, torch.float32, (3,))
                if len(col) != len(verts):
                    raise ValueError(f"{len(verts)} vertices but {len(col)} colours")
            else:
                uni = (C.c_double * 3)(*[int(v) / 255.0 for v in color])
            if mode == "shaded":
                R, t = camera.w2c[:, :3], camera.w2c[:, 3]
                eye = -np.linalg.solve(R, t)                                   # the camera's centre, host float64
                light = (C.c_double * 4)(*eye.tolist(), float(ambient))
        lib = _lib.load_mesh()
        sizes = (C.c_int64 * 2)()
        self._check_mesh(lib.sta_mesh_plan(len(tris), len(verts), sizes))
        if self._mesh_work is None or self._mesh_work.numel() < sizes[0]:
            self._mesh_work = torch.empty(int(sizes[0]), dtype=torch.uint8, device=self.device)
        T, K, near, far = camera._args()
        self._check_mesh(lib.sta_mesh_triangles(self.keys.data_ptr(), self.H, self.W, self.ssaa, verts.data_ptr(), len(verts), tris.data_ptr(), len(tris),
                                                col.data_ptr() if col is not None else None, uni, light, kind, MESH_CULL[cull], int(id_base), T, K, near, far,
                                                self._mesh_counters.data_ptr(), self._mesh_work.data_ptr(), self._mesh_work.numel(), self._stream()))
        return self

    def _check_mesh(self, rc):
        try:
            _lib.check_mesh(rc)
        except _lib.StaError as e:
            raise _value_error(e) from None

    def mesh_counters(self) -> Dict[str, int]:
        """Of the triangles drawn since the last clear, the eight of include/sta_mesh.h (one readback, which waits for the stream)."""
        return dict(zip(MESH_COUNTERS, self._mesh_counters.cpu().tolist()))

    def cameras(self, camera: Camera, poses, intrinsics, size, scale: float = 0.1, color=CAMERA_COLOR, line_width: int = 1):
        """A frustum per camera-to-world pose: `camera_segments`."""
        return self.lines(camera, camera_segments(poses, intrinsics, size, scale), color, line_width)

    def trajectory(self, camera: Camera, poses, color=TRAJECTORY_COLOR, line_width: int = 1):
        return self.lines(camera, trajectory_segments(poses), color, line_width)

    def view_graph(self, camera: Camera, view_graph, poses, loop_min_dist: int, upto: Optional[int] = None, line_width: int = 1):
        """Blue neighbour edges, orange loop edges: `view_graph_segments`."""
        segs, cols = view_graph_segments(view_graph, poses, loop_min_dist, upto)
        return self.lines(camera, segs, cols, line_width)

    def _resolve(self, background, rgba=None, depth=None, ids=None):
        bg = (C.c_uint8 * 4)(*[int(v) for v in background])
        self._check(self.lib.sta_raster_resolve(self.keys.data_ptr(), self.H, self.W, self.ssaa, bg, rgba.data_ptr() if rgba is not None else None,
                                                depth.data_ptr() if depth is not None else None, ids.data_ptr() if ids is not None else None,
                                                self._stream()))

    def image(self, background=(255, 255, 255, 255)) -> torch.Tensor:
        """uint8 [H,W,4] r, g, b, a.  background (0, 0, 0, 0) is the transparent screenshot of scripts/vis_slam_results.py."""
        out = torch.empty(self.H, self.W, 4, dtype=torch.uint8, device=self.device)
        self._resolve(background, rgba=out)
        return out

    def depth(self) -> torch.Tensor:
        """float32 [H,W]: the z of the nearest fragment, +inf where nothing was drawn."""
        out = torch.empty(self.H, self.W, dtype=torch.float32, device=self.device)
        self._resolve((0, 0, 0, 0), depth=out)
        return out

    def ids(self) -> torch.Tensor:
        """int32 [H,W]: the payload of the nearest fragment (the point's id when it was drawn with colors=None) as the library's uint32 bit
        pattern, so -1 where nothing was drawn; ids above 2^31 - 1 read as `ids.to(torch.int64) & 0xFFFFFFFF`."""
        out = torch.empty(self.H, self.W, dtype=torch.int32, device=self.device)
        self._resolve((0, 0, 0, 0), ids=out)
        return out

    def counters(self) -> Dict[str, int]:
        """Of the points drawn since the last clear (one readback, which waits for the stream)."""
        c = self._counters.cpu().tolist()
        return {"seen": c[0], "non_finite": c[1], "near_far": c[2], "off_canvas": c[3]}


# ------------------------------------------------------------------------------------------ maps
def render_map(frontend, camera: Camera, *, depths, scales, intrinsics, poses, confs, imgs, conf_thres: float, H: int = 480, W: int = 720,
               ssaa: int = 1, point_size: int = 1, color_divisor: float = 1.0, canvas: Optional[Canvas] = None, clear: bool = True) -> Canvas:
    """`formats.world_pointcloud` of exactly the arguments `PoseGraph.export` returns (plus the images), then `Canvas.points`.  imgs None:
    the id image instead (colors=None).  color_divisor 1.5 is scripts/video.py:113 (the colours are multiplied by float32(1 / divisor)).  -> the canvas (a new one unless given)."""
    from . import formats
    pts, col = formats.world_pointcloud(frontend, depths, scales, intrinsics, poses, confs, imgs, conf_thres)
    cv = canvas if canvas is not None else Canvas(frontend.device, H, W, ssaa)
    if canvas is not None and clear:
        cv.clear()
    if imgs is None:
        col = None
    elif color_divisor != 1.0:
        col = col * (1.0 / float(color_divisor))          # one float32 multiplication by float32(1 / divisor)
    return cv.points(camera, pts, col, point_size)


def render_mesh(frontend, camera: Camera, mesh, *, H: int = 480, W: int = 720, ssaa: int = 1, mode: str = "shaded", cull: str = "none",
                background=(255, 255, 255, 255), poses=None, intrinsics=None, size=None, view_graph=None, loop_min_dist: int = 0, camera_scale: float = 0.1,
                ambient: float = 0.3, color=MESH_COLOR, line_width: int = 1, canvas: Optional[Canvas] = None) -> torch.Tensor:
    """A `tsdf.Mesh` as an image uint8 [H,W,4].  poses [N,4,4] camera-to-world: the trajectory is drawn over the mesh; with intrinsics and
    size = (width_px, height_px) a frustum per pose as well; with view_graph (and loop_min_dist) its edges - all with the line calls, so
    the mesh occludes them.  frontend: anything with a `.device`, or a device."""
    dev = getattr(frontend, "device", frontend)
    cv = canvas.clear() if canvas is not None else Canvas(dev, H, W, ssaa)
    cv.mesh(camera, mesh, mode=mode, cull=cull, ambient=ambient, color=color)
    if poses is not None:
        poses = _host(poses).reshape(-1, 4, 4)
        if intrinsics is not None and size is not None:
            cv.cameras(camera, poses, _host(intrinsics), size, camera_scale, CAMERA_COLOR, line_width)
        if len(poses) > 1:
            cv.trajectory(camera, poses, TRAJECTORY_COLOR, line_width)
        if view_graph is not None:
            cv.view_graph(camera, view_graph, poses, loop_min_dist, line_width=line_width)
    return cv.image(background)


def mesh_depth(frontend, mesh, camera: Camera, H: int, W: int) -> torch.Tensor:
    """The depth map of a `tsdf.Mesh` from a pose: float32 [H,W], the z of the nearest surface through each pixel's centre, +inf where
    there is none."""
    dev = getattr(frontend, "device", frontend)
    return Canvas(dev, H, W, 1).mesh(camera, mesh, mode="id").depth()


def render_slam(slam, camera: Optional[Camera] = None, H: int = 480, W: int = 720, ssaa: int = 1, point_size: int = 1, direction: str = "topdown",
                draw_cameras: bool = True, draw_graph: bool = True, camera_scale: float = 0.1, background=(255, 255, 255, 255)) -> torch.Tensor:
    """The map of a live OnlineSLAM as an image uint8 [H,W,4]: the cloud, a frustum per keyframe, the view-graph edges.  camera None:
    `Camera.fit` on the trajectory."""
    n = slam.view_num
    ex = slam.pose_graph.export(view_num=n)
    poses = ex.poses.cpu().numpy().astype(np.float64)
    if camera is None:
        camera = Camera.fit(poses, H, W, direction)
    cv = render_map(slam.frontend, camera, depths=ex.depths, scales=ex.scales, intrinsics=ex.intrinsics, poses=ex.poses, confs=ex.confs,
                    imgs=torch.stack(slam.imgs[:n], dim=0), conf_thres=slam.conf_thres, H=H, W=W, ssaa=ssaa, point_size=point_size)
    if draw_cameras:
        h, w = ex.depths.shape[1:]
        cv.cameras(camera, poses, ex.intrinsics.cpu().numpy(), (w, h), camera_scale)
    if draw_graph:
        cv.view_graph(camera, slam.get_view_graph(), poses, slam.lc_detector.loop_dist_min)
    return cv.image(background)


def follow_offset() -> np.ndarray:
    """The pose offset of the "follow" mode: the camera 5 behind and 0.3 below the current view's, pitched 20 degrees (the non-topdown
    branch of scripts/video.py:20-23, with the rotation in degrees as its comment intends)."""
    a = np.deg2rad(20.0)
    off = np.eye(4)
    off[:3, :3] = [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]
    off[:3, 3] = [0, 0.3, 5]
    return off


def folder_frames(folder: str):
    """The snapshots of a save_data_all folder as scripts/video.py:51-72, 230-238 walks them: -> (N, pose_and_scale_for(v)) where view v is
    drawn with the first trajectory_{i}.npy / scales_{i}.npy whose i >= v, and with trajectory.npy / scales.npy after the last."""
    idx = sorted(int(os.path.basename(p).split("_")[-1].split(".")[0]) for p in glob.glob(os.path.join(folder, "scales_*.npy")))
    final = (np.load(os.path.join(folder, "trajectory.npy")), np.load(os.path.join(folder, "scales.npy")))
    cache = {}

    def at(v):
        later = [i for i in idx if i >= v]
        if not later:
            return final
        i = later[0]
        if i not in cache:
            cache[i] = (np.load(os.path.join(folder, f"trajectory_{i}.npy")), np.load(os.path.join(folder, f"scales_{i}.npy")))
        return cache[i]
    return len(final[0]), at


def render_folder(frontend, folder: str, out_folder: str, mode: str = "topdown", H: int = 480, W: int = 720, ssaa: int = 1, point_size: int = 1,
                  camera: Optional[Camera] = None, camera_scale: float = 0.1, background=(255, 255, 255, 255), mesh=None, mesh_mode: str = "shaded",
                  mesh_cull: str = "none") -> List[str]:
    """What scripts/video.py does with a save_data_all folder: one PNG per view v, {v:04d}.png, of the views 0 .. v under the poses and
    scales of the snapshot current at v - the cloud (colours divided by 1.5), a small frustum per earlier view, the current view's frustum
    ten times larger in dark green, the view-graph edges.  mode "topdown": one fixed camera (`camera`, or Camera.fit on the final
    trajectory); "follow": behind the current view (`follow_offset`).  Not drawn: the extra {v:04d}_pgo.png frames and the previous-view
    frustum of the reference.  mesh: a `tsdf.Mesh`, or the path of a mesh.ply of `tsdf.write_mesh_ply` - every frame then draws the
    whole mesh (mesh_mode, mesh_cull of `Canvas.mesh`) in place of the cloud.  -> the paths written."""
    if mode not in ("topdown", "follow"):
        raise ValueError(f'mode must be "topdown" or "follow" (got {mode!r})')
    N, at = folder_frames(folder)
    depths = np.load(os.path.join(folder, "depths.npy"))
    images = np.load(os.path.join(folder, "images.npy"))                              # [N,H,W,3] in [0, 1]
    intrinsics = np.load(os.path.join(folder, "intrinsics.npy"))
    cz = np.load(os.path.join(folder, "confs.npz"), allow_pickle=True)
    confs, thres = cz["confs"], float(cz["thres"])
    gz = np.load(os.path.join(folder, "view_graph.npz"), allow_pickle=True)
    graph, loop_min_dist = gz["view_graph"].item(), int(gz["loop_min_dist"].item())
    dev = frontend.device
    depths_d, confs_d, K_d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (depths, confs, intrinsics)]
    imgs_d = (torch.from_numpy(images).to(dev).permute(0, 3, 1, 2) * 2.0 - 1.0).contiguous()
    size = (depths.shape[2], depths.shape[1])
    K_out = [0.5 * min(H, W) / np.tan(np.deg2rad(30.0))] * 2 + [(W - 1) / 2.0, (H - 1) / 2.0]
    if mode == "topdown" and camera is None:
        camera = Camera.fit(np.load(os.path.join(folder, "trajectory.npy")), H, W, "topdown")
    os.makedirs(out_folder, exist_ok=True)
    cv = Canvas(dev, H, W, ssaa)
    if isinstance(mesh, (str, os.PathLike)):
        from . import tsdf
        mesh = tsdf.mesh_from_ply(mesh, dev)
    paths = []
    for v in range(N):
        traj, scales = at(v)
        cam = camera if mode == "topdown" else Camera.from_pose(traj[v], K_out, follow_offset())
        if mesh is not None:
            cv.clear().mesh(cam, mesh, mode=mesh_mode, cull=mesh_cull)
        else:
            render_map(frontend, cam, depths=depths_d[:v + 1], scales=torch.from_numpy(scales[:v + 1]).to(dev), intrinsics=K_d[:v + 1],
                       poses=torch.from_numpy(traj[:v + 1]).to(dev), confs=confs_d[:v + 1], imgs=imgs_d[:v + 1], conf_thres=thres,
                       point_size=point_size, color_divisor=1.5, canvas=cv)
        if v > 0:
            cv.cameras(cam, traj[:v], intrinsics[:v], size, camera_scale, CAMERA_COLOR)
        cv.cameras(cam, traj[v:v + 1], intrinsics[v:v + 1], size, 10.0 * camera_scale, CUR_CAMERA_COLOR)
        cv.view_graph(cam, graph, traj, loop_min_dist, upto=v + 1)
        paths.append(os.path.join(out_folder, f"{v:04d}.png"))
        write_png(paths[-1], cv.image(background))
    return paths


# ------------------------------------------------------------------------------------------ PNG
def write_png(path: str, rgba) -> None:
    """An 8-bit RGBA (or RGB, [H,W,3]) PNG with the standard library alone: zlib and struct."""
    if isinstance(rgba, torch.Tensor):
        rgba = rgba.detach().cpu().numpy()
    a = np.ascontiguousarray(rgba)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"write_png takes uint8 [H,W,3] or [H,W,4] (got {a.dtype} {a.shape})")
    h, w, ch = a.shape
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), a.reshape(h, w * ch)], axis=1).tobytes()        # filter 0 in front of every row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6 if ch == 4 else 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """The inverse of `write_png` for the files it writes (8-bit RGB / RGBA, filter 0, not interlaced)."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, "bad CRC"
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype = head[:4]
    assert depth == 8 and ctype in (2, 6) and head[6] == 0, "write_png's subset only"
    ch = 4 if ctype == 6 else 3
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert (rows[:, 0] == 0).all(), "write_png's subset only (filter 0)"
    return rows[:, 1:].reshape(h, w, ch).copy()
