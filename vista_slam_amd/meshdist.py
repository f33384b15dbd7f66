"""Exact point-to-triangle distances on the GPU: how far is this point from that mesh.

The library is libsta_dist.so (include/sta_dist.h holds the contract, tests/dist_cases.py restates it in numpy): the triangles sorted along
a Morton curve with the stable radix sort, an implicit bounding-volume hierarchy of fan-out 8 over the sorted order, refitted with one
launch per level, and one lane per query that walks it without a stack.  The closest point is Ericson's seven-region rule in float64 in a
written order, clamped into the triangle's own box - which makes a node's box distance a lower bound without any margin, so the answer IS
the brute-force minimum, lowest triangle index among equals, bit for bit.

    idx = meshdist.TriIndex.build(mesh)                       # a tsdf.Mesh
    d2, tri, point = idx.query(points, radius=0.5)            # float64 [Q], int32 [Q], float32 [Q,3]; +inf, -1, NaN where nothing is within radius
    d2, tri, point = meshdist.point_to_mesh(points, mesh)     # both in one call, radius = +inf

Rays against the same index are libsta_ray.so (include/sta_ray.h holds the contract, tests/ray_cases.py restates it): one lane per ray
walks the index that TriIndex.build wrote - slab intervals of the boxes widened by one float32 step, Woop-Benthin-Wald's sheared triangle
test in float64 in a written order, the hit clamped into the slab interval of the triangle's own box - which makes a node's entry
parameter a lower bound without any margin, so the answer IS the brute-force first hit, lowest triangle index among equals, bit for bit.
A ray is o + t d with d as given, not normalised: t is in units of |d|.

    t, tri, bary = idx.cast(origins, dirs)                    # float64 [R], int32 [R], float32 [R,3]; +inf, -1, NaN where nothing is hit
    hidden = idx.occluded(origins, dirs, 0.0, 1.0)            # uint8 [R]: is there a triangle on the segment o .. o + d
    depth = meshdist.ray_depth(idx, camera, H, W)             # float32 [H,W] along the pixel rays of a render.Camera: t IS the depth
    seen = meshdist.visible(idx, a, b)                        # bool [R]: nothing between a and b

What it is not: no signed distance and no crossing parity (a hit on a shared edge is accepted by both neighbours by design), no all-hits
list, no point-to-plane ICP against the mesh.  Not compared with Open3D's RaycastingScene or trimesh's closest_point (neither is
available).  DESIGN.md section 9.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Sequence

import torch

from . import _lib

FANOUT = 8
MAX_LEVELS = 9
KEY_BITS = 21
PLAN_SIZES = 2
COUNTERS = ("valid", "bad_index", "non_finite", "no_area", "status", "reserved_5", "reserved_6", "reserved_7")
STATUS_BOUND = 1
WANT = ("d2", "tri", "point")
RAY_WANT = ("t", "tri", "bary")
RAY_PLAN_SIZES = 1
RAY_STATUS_BOUND = 1


class Plan(NamedTuple):
    index_bytes: int
    build_work_bytes: int


def _check(rc):
    try:
        _lib.check_dist(rc)
    except _lib.StaError as e:
        raise (ValueError(str(e)) if str(e).startswith("tri_") else e) from None


def _check_ray(rc):
    try:
        _lib.check_ray(rc)
    except _lib.StaError as e:
        raise (ValueError(str(e)) if str(e).startswith("ray_") else e) from None


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def plan(nt: int, Q: int = 1) -> Plan:
    """Host only (no GPU): the byte counts of sta_tri_plan, its refusals as ValueError."""
    out = (C.c_int64 * PLAN_SIZES)()
    _check(_lib.load_dist().sta_tri_plan(int(nt), int(Q), out))
    return Plan(*[int(v) for v in out])


def ray_plan(nt: int, R: int = 1) -> int:
    """Host only (no GPU): the number of nodes of the index of nt triangles from sta_ray_plan, its refusals as ValueError.  A cast takes
    no workspace."""
    out = (C.c_int64 * RAY_PLAN_SIZES)()
    _check_ray(_lib.load_ray().sta_ray_plan(int(nt), int(R), out))
    return int(out[0])


def ray_check(nt: int, R: int, t_min: float = 0.0, t_max: float = math.inf, occluded: bool = False) -> None:
    """Host only (no GPU): the refusals of sta_ray_cast (occluded: sta_ray_occluded) for these numbers as ValueError, in the library's
    own words.  The entry point is called without buffers: it checks the numbers first and launches nothing."""
    lib = _lib.load_ray()
    one = (C.c_uint8 * 1)()
    if occluded:
        rc = lib.sta_ray_occluded(None, None, None, None, int(nt), None, None, int(R), float(t_min), float(t_max), C.addressof(one), None, None)
    else:
        rc = lib.sta_ray_cast(None, None, None, None, int(nt), None, None, int(R), float(t_min), float(t_max), None, None, None, None, None)
    try:
        _check_ray(rc)
    except ValueError as e:
        if not str(e).endswith(": null argument"):
            raise


def level_counts(nt: int):
    """The node counts of the implicit tree, level 0 first: ceil(nt / 8), then ceil of an eighth until a level has one node."""
    counts = [(int(nt) + FANOUT - 1) // FANOUT]
    while counts[-1] > 1:
        counts.append((counts[-1] + FANOUT - 1) // FANOUT)
    return counts


def _points(points, device) -> torch.Tensor:
    t = torch.as_tensor(points).to(device, torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"points must be [Q, 3] (got {tuple(t.shape)})")
    return t


def _rays(origins, dirs, device):
    """(origins, dirs) as contiguous float32 [R,3] on `device` (None: where they are); origins [3] is broadcast"""
    d = torch.as_tensor(dirs)
    o = torch.as_tensor(origins)
    if d.dim() != 2 or d.shape[1] != 3:
        raise ValueError(f"dirs must be [R, 3] (got {tuple(d.shape)})")
    if tuple(o.shape) not in ((3,), (1, 3), (len(d), 3)):
        raise ValueError(f"origins must be [R, 3] or [3] for {len(d)} rays (got {tuple(o.shape)})")
    if device is not None:
        o, d = o.to(device), d.to(device)
    o, d = o.to(torch.float32), d.to(torch.float32)
    return o.reshape(-1, 3).expand(len(d), 3).contiguous(), d.contiguous()


class TriIndex:
    """The index of one mesh: the sorted triangles, their sources, the boxes of every level and the counters, all in one device buffer
    that this object owns.  `counters` [8] int32 stays on the device (valid, bad-index, non-finite, no-area triangles, the status bit
    that a traversal reaching its bound would set, three zeros); `tri`, `src` and `level_boxes` are views into the buffer."""

    def __init__(self, buf, host, nv):
        self._buf, self._host, self.nv = buf, host, nv
        self.nt, self.levels = int(host.nt), int(host.levels)
        self.level_offset = [int(v) for v in host.level_offset]
        base = buf.data_ptr()

        def view(ptr, count, dtype, size):
            o = int(ptr) - base
            return buf[o:o + count * size].view(dtype)
        self.tri = view(host.tri, self.nt * 9, torch.float32, 4).view(self.nt, 9)
        self.src = view(host.src, self.nt, torch.int32, 4)
        self.boxes = view(host.boxes, self.level_offset[self.levels] * 6, torch.float32, 4).view(-1, 6)
        self.counters = view(host.counters, 8, torch.int32, 4)
        self._ray_status = None

    @staticmethod
    def build(mesh) -> "TriIndex":
        """Build the index of a `tsdf.Mesh` (or any object with .vertices [nv,3] and .triangles [nt,3]) on the device of its vertices.
        Does not wait for the stream."""
        verts = torch.as_tensor(mesh.vertices)
        if not verts.is_cuda:
            verts = verts.to("cuda:0")
        verts = verts.to(torch.float32).contiguous()
        tris = torch.as_tensor(mesh.triangles).to(verts.device, torch.int32).contiguous()
        if verts.dim() != 2 or verts.shape[1] != 3 or tris.dim() != 2 or tris.shape[1] != 3:
            raise ValueError(f"a mesh is vertices [nv,3] and triangles [nt,3] (got {tuple(verts.shape)}, {tuple(tris.shape)})")
        dev, nv, nt = verts.device, len(verts), len(tris)
        p = plan(nt, 1)
        if not 1 <= nv < 1 << 31:
            raise ValueError(f"tri_build: nv must be in [1, 2^31) (got {nv})")
        buf = torch.empty(p.index_bytes, dtype=torch.uint8, device=dev)
        work = torch.empty(p.build_work_bytes, dtype=torch.uint8, device=dev)
        counters = torch.empty(8, dtype=torch.int32, device=dev)
        host = _lib.StaTriIndex()
        with torch.cuda.device(dev):
            _check(_lib.load_dist().sta_tri_build(verts.data_ptr(), nv, tris.data_ptr(), nt, buf.data_ptr(), buf.numel(), work.data_ptr(), work.numel(),
                                                  C.addressof(host), counters.data_ptr(), _stream(dev)))
        return TriIndex(buf, host, nv)

    @property
    def device(self):
        return self._buf.device

    def level_boxes(self, level: int) -> torch.Tensor:
        """[count, 6] float32 lo xyz, hi xyz of one level (0 = the leaves)."""
        return self.boxes[self.level_offset[level]:self.level_offset[level + 1]]

    def query(self, points, radius: float = math.inf, want: Sequence[str] = WANT):
        """The nearest point of the mesh for every row of points [Q,3]: a tuple in the order of `want`, out of d2 [Q] float64 (squared
        distance), tri [Q] int32 (input triangle index) and point [Q,3] float32; +inf, -1 and NaN where no valid triangle lies within
        `radius` (inclusive; +inf allowed) or the query is not finite.  Device tensors; does not wait for the stream."""
        want = tuple(want)
        if not want or any(w not in WANT for w in want):
            raise ValueError(f"want must name some of {WANT} (got {want})")
        q = _points(points, self.device)
        Q, dev = len(q), self.device
        out = {"d2": None, "tri": None, "point": None}
        if "d2" in want:
            out["d2"] = torch.empty(Q, dtype=torch.float64, device=dev)
        if "tri" in want:
            out["tri"] = torch.empty(Q, dtype=torch.int32, device=dev)
        if "point" in want:
            out["point"] = torch.empty(Q, 3, dtype=torch.float32, device=dev)
        ptr = lambda t: None if t is None or not t.numel() else t.data_ptr()
        with torch.cuda.device(dev):
            _check(_lib.load_dist().sta_tri_query(C.addressof(self._host), ptr(q), Q, float(radius), ptr(out["d2"]), ptr(out["tri"]), ptr(out["point"]),
                                                  _stream(dev)))
        return tuple(out[w] for w in want)


    @property
    def ray_status(self) -> torch.Tensor:
        """[1] int32 on the device: the status word of this index's ray calls, 0 unless a traversal reached its bound (RAY_STATUS_BOUND)."""
        if self._ray_status is None:
            self._ray_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._ray_status

    def _ray_call(self, name, origins, dirs, t_min, t_max, outs):
        o, d = _rays(origins, dirs, self.device)
        ptr = lambda t: None if t is None or not t.numel() else t.data_ptr()
        with torch.cuda.device(self.device):
            _check_ray(getattr(_lib.load_ray(), name)(ptr(self.tri), ptr(self.src), ptr(self.boxes), ptr(self.counters), self.nt, ptr(o), ptr(d), len(d),
                                                      float(t_min), float(t_max), *[ptr(t) for t in outs], self.ray_status.data_ptr(), _stream(self.device)))

    def cast(self, origins, dirs, t_min: float = 0.0, t_max: float = math.inf, want: Sequence[str] = RAY_WANT):
        """The first hit of the rays origins + t dirs (dirs [R,3] as given, NOT normalised: t is in units of |d|; origins [R,3] or [3]) with
        t in [t_min, t_max], both inclusive: a tuple in the order of `want`, out of t [R] float64, tri [R] int32 (input triangle index) and
        bary [R,3] float32 (the weights of the triangle's corners); +inf, -1 and NaN where no valid triangle is hit or the ray is not
        finite or has d = 0.  Device tensors; does not wait for the stream."""
        want = tuple(want)
        if not want or any(w not in RAY_WANT for w in want):
            raise ValueError(f"want must name some of {RAY_WANT} (got {want})")
        R, dev = len(torch.as_tensor(dirs)), self.device
        out = {"t": None, "tri": None, "bary": None}
        if "t" in want:
            out["t"] = torch.empty(R, dtype=torch.float64, device=dev)
        if "tri" in want:
            out["tri"] = torch.empty(R, dtype=torch.int32, device=dev)
        if "bary" in want:
            out["bary"] = torch.empty(R, 3, dtype=torch.float32, device=dev)
        self._ray_call("sta_ray_cast", origins, dirs, t_min, t_max, (out["t"], out["tri"], out["bary"]))
        return tuple(out[w] for w in want)

    def occluded(self, origins, dirs, t_min: float = 0.0, t_max: float = math.inf) -> torch.Tensor:
        """uint8 [R]: 1 where some valid triangle is hit with t in [t_min, t_max], i.e. where `cast` with the same arguments returns a
        triangle; the traversal leaves at the first one it meets.  A device tensor; does not wait for the stream."""
        occ = torch.empty(len(torch.as_tensor(dirs)), dtype=torch.uint8, device=self.device)
        self._ray_call("sta_ray_occluded", origins, dirs, t_min, t_max, (occ,))
        return occ


def point_to_mesh(points, mesh, radius: float = math.inf):
    """(d2, tri, point) of `TriIndex.build(mesh).query(points, radius)`."""
    return TriIndex.build(mesh).query(points, radius)


def ray_cast(origins, dirs, mesh, t_min: float = 0.0, t_max: float = math.inf):
    """(t, tri, bary) of `TriIndex.build(mesh).cast(origins, dirs, t_min, t_max)`."""
    return TriIndex.build(mesh).cast(origins, dirs, t_min, t_max)


def camera_rays(camera, H: int, W: int):
    """float32 (origins [3], dirs [H*W,3]) on the host: the rays through the pixel centres of a `render.Camera`, row-major (pixel (row v,
    column u) is ray v * W + u).  d has camera-space z = 1 - ((u - cx) / fx, (v - cy) / fy, 1) turned into the world - so the t of a hit
    IS the depth `render.mesh_depth` speaks of.  Computed in float64 and rounded once."""
    import numpy as np
    fx, fy, cx, cy = [float(v) for v in camera.K]
    Rm, tv = np.asarray(camera.w2c, dtype=np.float64)[:, :3], np.asarray(camera.w2c, dtype=np.float64)[:, 3]
    u, v = np.meshgrid(np.arange(int(W), dtype=np.float64), np.arange(int(H), dtype=np.float64))
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1).reshape(-1, 3)
    return torch.from_numpy((-Rm.T @ tv).astype(np.float32)), torch.from_numpy((dc @ Rm).astype(np.float32))


def ray_depth(index: TriIndex, camera, H: int, W: int) -> torch.Tensor:
    """The depth map of the indexed mesh from a `render.Camera` by rays: float32 [H,W], the depth of the first surface along each pixel's
    ray between the camera's near and far planes, +inf where there is none.  Unlike the rasteriser it snaps nothing to a sub-pixel grid;
    any other set of rays (a pointmap, a distorted model, a lidar pattern) goes through `cast` the same way."""
    o, d = camera_rays(camera, H, W)
    t, = index.cast(o, d, camera.near, camera.far, want=("t",))
    return t.to(torch.float32).view(int(H), int(W))


def visible(index: TriIndex, a, b, eps: float = 1e-6) -> torch.Tensor:
    """bool [R]: no valid triangle on the segments a -> b between the parameters eps and 1 - eps (a, b [R,3], or one of them [3]): line of
    sight against the surface.  A device tensor; does not wait for the stream."""
    dev = index.device
    a, b = torch.as_tensor(a).to(dev, torch.float32), torch.as_tensor(b).to(dev, torch.float32)
    d = (b.reshape(-1, 3).to(torch.float64) - a.reshape(-1, 3).to(torch.float64)).to(torch.float32)
    return index.occluded(a, d, float(eps), 1.0 - float(eps)) == 0
