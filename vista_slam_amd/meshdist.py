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

Registration against the same index is libsta_reg.so (include/sta_reg.h holds the contract, tests/reg_cases.py restates it): one pass
moves every point by T in float64 (the moved point is not rounded), finds its exact nearest triangle as `query` does, and folds the sums
of a point-to-point step (the record of cloud.kabsch) and of a point-to-plane step (g = sum J r, H = sum J J^T about a pivot) into one
record of 64 doubles, without floating-point atomics.  `icp` is cloud.icp's loop on it: one pass and one 512-byte readback per
evaluation, the source is never rewritten.

    rec = meshdist.RegRecord.from_array(idx.register_pass(points, T, radius=0.2)[0].cpu().numpy())
    reg = meshdist.icp(points, idx, max_corr=0.2, mode="plane")     # a cloud.ICPResult; mode="point": Kabsch on the closest points

What it is not: no signed distance and no crossing parity (a hit on a shared edge is accepted by both neighbours by design), no all-hits
list.  The ICP has no robust kernel and no scale estimate, it is not point-to-plane against a CLOUD with estimated normals, and it is not
Open3D's registration_icp, which is not available to compare with.  Not compared with Open3D's RaycastingScene or trimesh's
closest_point either.  DESIGN.md section 9.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Sequence

import numpy as np
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
REG_WANT = ("record", "d2", "tri", "point", "resid")
REG_PLAN_SIZES = 2
REG_RECORD = 64
REG_STATUS_BOUND = 1


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


def _check_reg(rc):
    try:
        _lib.check_reg(rc)
    except _lib.StaError as e:
        raise (ValueError(str(e)) if str(e).startswith("reg_") else e) from None


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


class RegPlan(NamedTuple):
    nodes: int
    work_bytes: int


def reg_plan(nt: int, Q: int = 1) -> RegPlan:
    """Host only (no GPU): the number of nodes of the index of nt triangles and the bytes of the workspace of one pass over Q points
    (the partial rows of the record) from sta_reg_plan, its refusals as ValueError."""
    out = (C.c_int64 * REG_PLAN_SIZES)()
    _check_reg(_lib.load_reg().sta_reg_plan(int(nt), int(Q), out))
    return RegPlan(*[int(v) for v in out])


def reg_check(nt: int, Q: int, radius: float = math.inf, min_cos: float = -1.0) -> None:
    """Host only (no GPU): the refusals of sta_reg_pass for these numbers as ValueError, in the library's own words.  The entry point is
    called without buffers: it checks the numbers first and launches nothing."""
    rc = _lib.load_reg().sta_reg_pass(None, None, None, None, int(nt), None, None, int(Q), None, None, float(radius), float(min_cos), None, None, None,
                                      None, None, None, 0, None, None)
    try:
        _check_reg(rc)
    except ValueError as e:
        if not str(e).endswith(": null argument"):
            raise


class RegRecord(NamedTuple):
    """The record of one registration pass (sta_reg_pass's record_out) on the host.  The first eight fields are cloud.Record's."""
    finite: int
    matched: int
    sum_d2: float
    sum_clipped: float
    sum_q: np.ndarray          # [3]   sum of the moved points over the matched ones
    sum_p: np.ndarray          # [3]   sum of their closest points (float64)
    sum_qp: np.ndarray         # [3,3] sum of q' c^T
    non_finite: int
    rejected: int              # found a triangle, failed the normal check
    sum_r2: float              # sum of the squared plane residuals
    sum_abs_r: float
    g: np.ndarray              # [6]   sum J r, (rotation, translation)
    H: np.ndarray              # [6,6] sum J J^T, symmetric

    @staticmethod
    def from_array(r) -> "RegRecord":
        r = np.asarray(r, dtype=np.float64).reshape(REG_RECORD)
        H = np.zeros((6, 6))
        H[np.triu_indices(6)] = r[29:50]
        H = H + np.triu(H, 1).T
        return RegRecord(int(r[0]), int(r[1]), float(r[2]), float(r[3]), r[4:7].copy(), r[7:10].copy(), r[10:19].reshape(3, 3).copy(), int(r[19]),
                         int(r[20]), float(r[21]), float(r[22]), r[23:29].copy(), H)


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
        self._reg_status = None

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

    @property
    def reg_status(self) -> torch.Tensor:
        """[1] int32 on the device: the status word of this index's registration passes, 0 unless a traversal reached its bound
        (REG_STATUS_BOUND)."""
        if self._reg_status is None:
            self._reg_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._reg_status

    def register_pass(self, points, T=None, radius: float = math.inf, normals=None, min_cos=None, pivot=None, want: Sequence[str] = ("record",)):
        """One sta_reg_pass over points [Q,3]: every point moved by T ([3,4] or [4,4] float64; None = identity) in float64, its exact
        nearest triangle within `radius` (inclusive; +inf allowed), the plane residual and the Jacobian row about `pivot` ([3]; None = 0).
        normals [Q,3] with min_cos (None with normals: 0): a match whose moved normal makes a cosine below min_cos with the triangle's is
        rejected after the search.  A tuple in the order of `want`, out of record [64] float64 (`RegRecord.from_array` on the host),
        d2 [Q] float64, tri [Q] int32, point [Q,3] float32 (as `query`) and resid [Q] float64 (the signed plane residual, NaN without a
        triangle).  Device tensors; does not wait for the stream."""
        want = tuple(want)
        if not want or any(w not in REG_WANT for w in want):
            raise ValueError(f"want must name some of {REG_WANT} (got {want})")
        if normals is None and min_cos is not None:
            raise ValueError("register_pass: min_cos needs normals")
        q = _points(points, self.device)
        Q, dev = len(q), self.device
        nrm = None
        if normals is not None:
            nrm = _points(normals, dev)
            if len(nrm) != Q:
                raise ValueError(f"normals must be [{Q}, 3] (got {tuple(nrm.shape)})")
        kinds = {"record": ((REG_RECORD,), torch.float64), "d2": ((Q,), torch.float64), "tri": ((Q,), torch.int32), "point": ((Q, 3), torch.float32),
                 "resid": ((Q,), torch.float64)}
        out = {k: (torch.empty(*kinds[k][0], dtype=kinds[k][1], device=dev) if k in want else None) for k in REG_WANT}
        work, wb = None, 0
        if out["record"] is not None:
            wb = reg_plan(self.nt, max(Q, 1)).work_bytes
            work = torch.empty(wb, dtype=torch.uint8, device=dev)
        Tm = None if T is None else (C.c_double * 12)(*_matrix34(T).reshape(12).tolist())
        pv = None if pivot is None else (C.c_double * 3)(*np.asarray(pivot, dtype=np.float64).reshape(3).tolist())
        ptr = lambda t: None if t is None or not t.numel() else t.data_ptr()
        with torch.cuda.device(dev):
            _check_reg(_lib.load_reg().sta_reg_pass(ptr(self.tri), ptr(self.src), ptr(self.boxes), ptr(self.counters), self.nt, ptr(q), ptr(nrm), Q, Tm, pv,
                                                    float(radius), 0.0 if min_cos is None else float(min_cos), ptr(out["d2"]), ptr(out["tri"]),
                                                    ptr(out["point"]), ptr(out["resid"]), ptr(out["record"]), ptr(work), wb, self.reg_status.data_ptr(),
                                                    _stream(dev)))
        return tuple(out[w] for w in want)


def _matrix34(T) -> np.ndarray:
    m = np.asarray(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, dtype=np.float64)
    if m.shape == (4, 4):
        m = m[:3]
    if m.shape != (3, 4):
        raise ValueError(f"T must be 3x4 or 4x4 (got {m.shape})")
    return np.ascontiguousarray(m)


def exp_so3(w) -> np.ndarray:
    """Rodrigues: Exp(w) = I + (sin t / t) K + ((1 - cos t) / t^2) K^2 with t = |w|, K = [w]x; the series' first terms below t = 1e-8."""
    w = np.asarray(w, dtype=np.float64).reshape(3)
    t = float(np.sqrt(w @ w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    a, b = (1.0 - t * t / 6.0, 0.5 - t * t / 24.0) if t < 1e-8 else (math.sin(t) / t, (1.0 - math.cos(t)) / (t * t))
    return np.eye(3) + a * K + b * (K @ K)


def plane_step(record, pivot, sv_ratio: float = 1e-9) -> np.ndarray:
    """The point-to-plane update of one record (host float64): solve H delta = -g for delta = (omega, v) through eigh(H); an
    eigen-direction whose eigenvalue is not above sv_ratio times the largest is left at 0 (a single wall moves the scan along its normal
    and about the two in-plane axes only).  -> the 3x4 update x -> Exp(omega)(x - pivot) + pivot + v."""
    rec = record if isinstance(record, RegRecord) else RegRecord.from_array(record)
    pivot = np.zeros(3) if pivot is None else np.asarray(pivot, dtype=np.float64).reshape(3)
    lam, V = np.linalg.eigh(rec.H)
    keep = lam > float(sv_ratio) * lam[-1] if lam[-1] > 0.0 else np.zeros(6, bool)
    coef = np.where(keep, (V.T @ -rec.g) / np.where(keep, lam, 1.0), 0.0)
    delta = V @ coef
    R = exp_so3(delta[:3])
    return np.concatenate([R, (pivot - R @ pivot + delta[3:])[:, None]], axis=1)


def _reg_evaluate(index, src, nrm, max_corr, min_cos, T, pivot):
    rec, = index.register_pass(src, T, max_corr, nrm, min_cos if nrm is not None else None, pivot)
    rec = RegRecord.from_array(rec.cpu().numpy())          # the 512-byte readback (which waits for the stream)
    fitness = rec.matched / (rec.finite + rec.non_finite)
    rmse = float(np.sqrt(rec.sum_d2 / rec.matched)) if rec.matched else 0.0
    return rec, fitness, rmse


def icp(source, index: TriIndex, max_corr: float, init=None, mode: str = "plane", normals=None, min_cos=None, max_iter: int = 30,
        rel_fitness: float = 1e-6, rel_rmse: float = 1e-6):
    """ICP of `source` [Q,3] onto the SURFACE of `index`: cloud.icp's loop and stopping rule on TriIndex.register_pass.

      1. evaluate at T = init: fitness = matched / Q, inlier_rmse = sqrt(sum d2 / matched) - the distance to the closest point, in both
         modes, so that the two are comparable
      2. repeat T <- step o T and evaluate again; stop when |d fitness| < rel_fitness and |d rmse| < rel_rmse, or after max_iter updates.
         mode="point": step = cloud.kabsch(record) on the closest points.  mode="plane": step = plane_step(record, pivot) with
         pivot = T . (the float64 mean of the finite source points, read once before the loop), which keeps H well conditioned.

    Each evaluation is one pass under T and one 512-byte readback; the source is never rewritten, T is composed on the host in float64.
    normals [Q,3] (of the source, in its own frame) with min_cos reject matches whose normals disagree.  Fewer than 6 matches in plane
    mode, 3 in point mode, end the loop with status "too_few_matches".  -> cloud.ICPResult.  No robust kernel, no scale estimate; not
    Open3D's registration_icp (not available to compare with)."""
    from . import cloud
    if mode not in ("plane", "point"):
        raise ValueError(f"icp: mode must be 'plane' or 'point' (got {mode!r})")
    src = _points(source, index.device)
    nrm = None if normals is None else _points(normals, index.device)
    if nrm is not None and min_cos is None:
        min_cos = 0.0
    need = 6 if mode == "plane" else 3
    T = np.eye(4)[:3] if init is None else _matrix34(init).copy()
    centre = np.zeros(3)
    if mode == "plane":
        fin = torch.isfinite(src).all(dim=1)
        if bool(fin.any()):
            centre = src[fin].to(torch.float64).mean(dim=0).cpu().numpy()
    pivot_of = lambda T: T[:, :3] @ centre + T[:, 3]
    rec, fitness, rmse = _reg_evaluate(index, src, nrm, max_corr, min_cos, T, pivot_of(T))
    status, it = "max_iter", 0
    while it < int(max_iter):
        if rec.matched < need:
            status = "too_few_matches"
            break
        step = plane_step(rec, pivot_of(T)) if mode == "plane" else cloud.kabsch(cloud.Record(*rec[:8]))
        T = cloud.compose(step, T)
        it += 1
        rec, f2, r2 = _reg_evaluate(index, src, nrm, max_corr, min_cos, T, pivot_of(T))
        done = abs(f2 - fitness) < rel_fitness and abs(r2 - rmse) < rel_rmse
        fitness, rmse = f2, r2
        if done:
            status = "converged"
            break
    if rec.matched < need and status == "max_iter":
        status = "too_few_matches"
    return cloud.ICPResult(np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]], axis=0), fitness, rmse, it, status)


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
