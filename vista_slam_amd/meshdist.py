"""Exact point-to-triangle distances on the GPU: how far is this point from that mesh.

The library is libsta_dist.so (include/sta_dist.h holds the contract, tests/dist_cases.py restates it in numpy): the triangles sorted along
a Morton curve with the stable radix sort, an implicit bounding-volume hierarchy of fan-out 8 over the sorted order, refitted with one
launch per level, and one lane per query that walks it without a stack.  The closest point is Ericson's seven-region rule in float64 in a
written order, clamped into the triangle's own box - which makes a node's box distance a lower bound without any margin, so the answer IS
the brute-force minimum, lowest triangle index among equals, bit for bit.

    idx = meshdist.TriIndex.build(mesh)                       # a tsdf.Mesh
    d2, tri, point = idx.query(points, radius=0.5)            # float64 [Q], int32 [Q], float32 [Q,3]; +inf, -1, NaN where nothing is within radius
    d2, tri, point = meshdist.point_to_mesh(points, mesh)     # both in one call, radius = +inf

What it is not: no signed distance, no ray casting, no point-to-plane ICP against the mesh.  Not compared with Open3D's RaycastingScene or
trimesh's closest_point (neither is available).  DESIGN.md section 9.
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


class Plan(NamedTuple):
    index_bytes: int
    build_work_bytes: int


def _check(rc):
    try:
        _lib.check_dist(rc)
    except _lib.StaError as e:
        raise (ValueError(str(e)) if str(e).startswith("tri_") else e) from None


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def plan(nt: int, Q: int = 1) -> Plan:
    """Host only (no GPU): the byte counts of sta_tri_plan, its refusals as ValueError."""
    out = (C.c_int64 * PLAN_SIZES)()
    _check(_lib.load_dist().sta_tri_plan(int(nt), int(Q), out))
    return Plan(*[int(v) for v in out])


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


def point_to_mesh(points, mesh, radius: float = math.inf):
    """(d2, tri, point) of `TriIndex.build(mesh).query(points, radius)`."""
    return TriIndex.build(mesh).query(points, radius)
