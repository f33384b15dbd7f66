"""Nearest neighbours between point clouds on the GPU, and what the reference's reconstruction metric builds on them
(vista_slam/eval/eval_recon.py): point-to-point ICP and the clipped chamfer distance.

The search is libsta_cloud.so (include/sta_cloud.h holds the contract, tests/cloud_cases.py restates it in numpy): an exact
nearest neighbour within a radius on a uniform grid, with a 24-double record of the sums that ICP and chamfer need, so an
ICP iteration is one kernel pass over the source cloud and one 192-byte readback.  The 3x3 algebra (`kabsch`) runs on the host in
numpy float64: it has no hot path.

Not here: Open3D, pykdtree (neither is available to compare against); point-to-plane ICP, normals, robust kernels.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_POINTS = (1 << 30) - 1
MAX_RINGS = 32
RECORD = 24
# Default cell of `chamfer` as a fraction of max_error, chosen from the three tables of tools/cloud_bench.py (profiles/r25_cloud.txt),
# one query pass at radius 0.5, fractions 1/4, 1/8, 1/16, 1/32:
#   2 M x 2 M, every query matched after ring 1           9.44    3.78    3.12    6.12 ms
#   20 M x 20 M, likewise                                  805     223    79.3    50.2 ms
#   2 M x 2 M, 5 % of the queries beyond the radius       20.5    61.2     386    2825 ms   (an unmatched query walks every ring)
# The rule: the fraction whose worst ratio to the best fraction of a table is smallest - 16, 4.4, 18.8, 138 - which is 1/8.  A cloud
# with many unmatched queries is served better by a larger cell, a very dense one by a smaller.  Correctness does not depend on it.
CHAMFER_CELL_FRACTION = 1.0 / 8.0


class Plan(NamedTuple):
    index_bytes: int
    build_bytes: int
    query_bytes: int


class Record(NamedTuple):
    """The record of one query pass (sta_nn_query's record_out) on the host."""
    finite: int
    matched: int
    sum_d2: float
    sum_clipped: float
    sum_q: np.ndarray          # [3]   sum of the transformed queries over matched pairs
    sum_p: np.ndarray          # [3]   sum of their reference points
    sum_qp: np.ndarray         # [3,3] sum of q' p^T
    non_finite: int

    @staticmethod
    def from_array(r) -> "Record":
        r = np.asarray(r, dtype=np.float64).reshape(RECORD)
        return Record(int(r[0]), int(r[1]), float(r[2]), float(r[3]), r[4:7].copy(), r[7:10].copy(), r[10:19].reshape(3, 3).copy(), int(r[19]))


def _align(n):
    return (int(n) + 255) & ~255


def plan(M: int, Q: int) -> Plan:
    """Host only, no library needed: the byte counts sta_nn_plan reports (tests compare the two) and its refusals as ValueError."""
    M, Q = int(M), int(Q)
    if not 1 <= M <= MAX_POINTS:
        raise ValueError(f"nn_plan: M must be in [1, 2^30) (got {M})")
    if not 1 <= Q <= MAX_POINTS:
        raise ValueError(f"nn_plan: Q must be in [1, 2^30) (got {Q})")
    nb256, nbs = (M + 255) // 256, (M + 1023) // 1024
    index = _align(8 * M) + _align(4 * (M + 2)) + _align(12 * M) + _align(4 * M)
    build = (_align(1024 * 32) + _align(32) + _align(64) + 2 * _align(8 * M) + _align(4 * M) + _align(1024 * nbs) + _align(1024)
             + _align(4 * nb256) + _align(8 * (nb256 + 1)))
    query = _align(min((Q + 255) // 256, 2048) * RECORD * 8)
    return Plan(index, build, query)


def check_radius(radius: float, cell: float) -> float:
    r = float(radius)
    if not (np.isfinite(r) and r >= 0.0):
        raise ValueError("nn_query: radius must be finite and >= 0 (got %g)" % r)
    if r > MAX_RINGS * float(cell):
        raise ValueError("nn_query: radius %.17g is more than %d cells of %.17g" % (r, MAX_RINGS, float(cell)))
    return r


def _points(points, device=None) -> torch.Tensor:
    t = torch.as_tensor(points)
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda:0")
    t = t.to(device, torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"points must be [M, 3] (got {tuple(t.shape)})")
    return t


def _matrix(T):
    if T is None:
        return None
    m = np.asarray(T, dtype=np.float64)
    if m.shape == (4, 4):
        m = m[:3]
    if m.shape != (3, 4):
        raise ValueError(f"T must be 3x4 or 4x4 (got {m.shape})")
    return (C.c_double * 12)(*m.reshape(12).tolist())


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _value_error(e: _lib.StaError):
    if str(e).startswith(("nn_build:", "nn_query:", "nn_plan:")):
        return ValueError(str(e))
    return e


class NNIndex:
    """A uniform-grid index over a reference cloud (sta_nn_build).  It owns its device buffer; queries allocate their outputs."""

    def __init__(self, buf, info, device):
        self._buf, self.info, self.device = buf, info, device
        self.M, self.finite, self.cells, self.cell = int(info.M), int(info.n_finite), int(info.C), float(info.cell)
        self.lo, self.extent = tuple(int(v) for v in info.lo), tuple(int(v) for v in info.ext)

    @classmethod
    def build(cls, points, cell: float) -> "NNIndex":
        """points [M,3] (fp32 on the device; anything else is converted), cell > 0.  Synchronises the current stream once.
        ValueError for a grid the library refuses (more than 2^21 cells on an axis, a cell index beyond +-2^21)."""
        pts = _points(points)
        cell = float(cell)
        if not (np.isfinite(cell) and cell > 0.0):
            raise ValueError("nn_build: cell must be finite and > 0 (got %g)" % cell)
        M = pts.shape[0]
        p = plan(M, 1)
        lib = _lib.load_cloud()
        with torch.cuda.device(pts.device):
            buf = torch.empty(p.index_bytes, device=pts.device, dtype=torch.uint8)
            work = torch.empty(p.build_bytes, device=pts.device, dtype=torch.uint8)
            info = _lib.StaNNIndex()
            try:
                _lib.check_cloud(lib.sta_nn_build(pts.data_ptr(), M, cell, buf.data_ptr(), p.index_bytes, work.data_ptr(), p.build_bytes,
                                                  C.byref(info), _stream(pts.device)))
            except _lib.StaError as e:
                raise _value_error(e) from None
        return cls(buf, info, pts.device)

    def query(self, points, radius: float, T=None, want: Sequence[str] = ("d2", "idx", "record")):
        """The exact nearest reference point within `radius` of every T-transformed query -> dict of device tensors:
        "d2" [Q] float64 (+inf: none), "idx" [Q] int32 (-1: none), "record" [24] float64 (`Record.from_array` on the host).
        Asynchronous on the current stream."""
        unknown = set(want) - {"d2", "idx", "record"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        qry = _points(points, self.device)
        r = check_radius(radius, self.cell)
        Q = qry.shape[0]
        qb = plan(1, Q).query_bytes
        lib = _lib.load_cloud()
        dev = self.device
        out = {}
        with torch.cuda.device(dev):
            if "d2" in want:
                out["d2"] = torch.empty(Q, device=dev, dtype=torch.float64)
            if "idx" in want:
                out["idx"] = torch.empty(Q, device=dev, dtype=torch.int32)
            work = None
            if "record" in want:
                out["record"] = torch.empty(RECORD, device=dev, dtype=torch.float64)
                work = torch.empty(qb, device=dev, dtype=torch.uint8)

            def ptr(k):
                return out[k].data_ptr() if k in out else None
            try:
                _lib.check_cloud(lib.sta_nn_query(C.byref(self.info), qry.data_ptr(), Q, _matrix(T), r, ptr("d2"), ptr("idx"), ptr("record"),
                                                  work.data_ptr() if work is not None else None, qb, _stream(dev)))
            except _lib.StaError as e:
                raise _value_error(e) from None
        return out


def transform(points, T) -> torch.Tensor:
    """float(T p) of every point (sta_cloud_transform): fp64 arithmetic, one rounding to fp32.  -> a new [M,3] device tensor."""
    pts = _points(points)
    out = torch.empty_like(pts)
    with torch.cuda.device(pts.device):
        _lib.check_cloud(_lib.load_cloud().sta_cloud_transform(pts.data_ptr() if pts.numel() else None, pts.shape[0], _matrix(T),
                                                               out.data_ptr() if out.numel() else None, _stream(pts.device)))
    return out


def kabsch(record) -> np.ndarray:
    """The rigid 3x4 update that moves the matched queries onto their reference points in the least-squares sense, from a record
    (host numpy float64).  H = sum q'p^T - (sum q')(sum p)^T / n; U S V^T = svd(H); R = V diag(1, 1, det(V U^T)) U^T;
    t = mean_p - R mean_q."""
    rec = record if isinstance(record, Record) else Record.from_array(record)
    n = float(rec.matched)
    H = rec.sum_qp - np.outer(rec.sum_q, rec.sum_p) / n
    U, _S, Vt = np.linalg.svd(H)
    V = Vt.T
    d = np.linalg.det(V @ U.T)
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    t = rec.sum_p / n - R @ (rec.sum_q / n)
    return np.concatenate([R, t[:, None]], axis=1)


def compose(A, B) -> np.ndarray:
    """A o B for 3x4 matrices (apply B first)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return np.concatenate([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]], axis=1)


class ICPResult(NamedTuple):
    T: np.ndarray              # [4,4] float64
    fitness: float
    inlier_rmse: float
    iterations: int
    status: str                # "converged" | "max_iter" | "too_few_matches"


def _evaluate(index, source, max_corr, T):
    rec = Record.from_array(index.query(source, max_corr, T=T, want=("record",))["record"].cpu().numpy())      # the 192-byte readback
    Q = rec.finite + rec.non_finite
    fitness = rec.matched / Q
    rmse = float(np.sqrt(rec.sum_d2 / rec.matched)) if rec.matched else 0.0
    return rec, fitness, rmse


def icp(source, index: NNIndex, max_corr: float, init=None, max_iter: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6) -> ICPResult:
    """Point-to-point ICP of `source` onto the cloud of `index`, after Open3D's registration_icp with
    TransformationEstimationPointToPoint().  Open3D's loop is restated from memory: Open3D was not available to compare against.

      1. evaluate at T = init: fitness = matched / Q, inlier_rmse = sqrt(sum d2 / matched)
      2. repeat T <- kabsch(record) o T and evaluate again; stop when |d fitness| < rel_fitness and |d rmse| < rel_rmse, or after
         max_iter updates.

    Each evaluation is one sta_nn_query under T and one 192-byte readback (which waits for the stream).  A stated difference:
    Open3D transforms the source cloud in place every iteration; here it is never rewritten, T is composed on the host in
    float64.  Fewer than 3 matches end the loop with status "too_few_matches"."""
    src = _points(source, index.device)
    T = np.eye(4)[:3] if init is None else np.asarray(init, dtype=np.float64)[:3].copy()
    rec, fitness, rmse = _evaluate(index, src, max_corr, T)
    status, it = "max_iter", 0
    while it < int(max_iter):
        if rec.matched < 3:
            status = "too_few_matches"
            break
        T = compose(kabsch(rec), T)
        it += 1
        rec, f2, r2 = _evaluate(index, src, max_corr, T)
        done = abs(f2 - fitness) < rel_fitness and abs(r2 - rmse) < rel_rmse
        fitness, rmse = f2, r2
        if done:
            status = "converged"
            break
    if rec.matched < 3 and status == "max_iter":
        status = "too_few_matches"
    return ICPResult(np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]], axis=0), fitness, rmse, it, status)


class Chamfer(NamedTuple):
    chamfer: float
    rmse_1: float              # est -> ref (accuracy)
    rmse_2: float              # ref -> est (completeness)
    dist_1: Optional[torch.Tensor]
    dist_2: Optional[torch.Tensor]


def chamfer(ref_points, est_points, max_error: float, cell: Optional[float] = None, return_distances: bool = False) -> Chamfer:
    """chamfer_distance_RMSE of eval_recon.py:89-105: two indices, two queries at radius = max_error;
    rmse_1 = sqrt(sum min(d2, max_error^2) / finite) for est -> ref, rmse_2 for ref -> est, chamfer = 0.5 rmse_1 + 0.5 rmse_2
    (clip(dist, 0, max_error) = sqrt(min(d2, max_error^2))).  return_distances: the clipped distances per point [float64]."""
    ref, est = _points(ref_points), _points(est_points)
    est = est.to(ref.device)
    cell = float(max_error) * CHAMFER_CELL_FRACTION if cell is None else float(cell)
    want = ("record", "d2") if return_distances else ("record",)
    out = []
    for a, b in ((ref, est), (est, ref)):
        res = NNIndex.build(a, cell).query(b, max_error, want=want)
        out.append(res)
    recs = [Record.from_array(r["record"].cpu().numpy()) for r in out]
    rm = [float(np.sqrt(r.sum_clipped / r.finite)) if r.finite else float("nan") for r in recs]
    dist = [None, None]
    if return_distances:
        r2 = float(max_error) * float(max_error)
        dist = [torch.sqrt(torch.clamp(r["d2"], max=r2)) for r in out]
    return Chamfer(0.5 * rm[0] + 0.5 * rm[1], rm[0], rm[1], dist[0], dist[1])
