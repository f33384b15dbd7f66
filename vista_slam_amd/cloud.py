"""Nearest neighbours between point clouds on the GPU, and what the reference's reconstruction metric builds on them
(vista_slam/eval/eval_recon.py): point-to-point ICP and the clipped chamfer distance.

The search is libsta_cloud.so (include/sta_cloud.h holds the contract, tests/cloud_cases.py restates it in numpy): an exact
nearest neighbour within a radius on a uniform grid, with a 24-double record of the sums that ICP and chamfer need, so an
ICP iteration is one kernel pass over the source cloud and one 192-byte readback.  The 3x3 algebra (`kabsch`) runs on the host in
numpy float64: it has no hot path.

Neighbourhoods are libsta_knn.so (include/sta_knn.h, restated by tests/knn_cases.py), which reads the same index: `NNIndex.knn` gives the
k nearest reference points of every query in (d2, index) order, `knn_moments` their mean distance, covariance normal and surface
variation, and on those sit `estimate_normals`, `remove_statistical_outlier` and `remove_radius_outlier` - what a user of pointcloud.ply
does next.  Their stated differences from Open3D stand above `knn_plan`.

Not here: Open3D, pykdtree (neither is available to compare against); point-to-plane ICP between clouds, tangent-plane normal
propagation, robust kernels.
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
    if str(e).startswith(("nn_build:", "nn_query:", "nn_plan:", "knn_plan:", "knn_query:", "knn_moments:")):
        return ValueError(str(e))
    return e


class NNIndex:
    """A uniform-grid index over a reference cloud (sta_nn_build).  It owns its device buffer; queries allocate their outputs."""

    def __init__(self, buf, info, device):
        self._buf, self.info, self.device = buf, info, device
        self.M, self.finite, self.cells, self.cell = int(info.M), int(info.n_finite), int(info.C), float(info.cell)
        self.lo, self.extent = tuple(int(v) for v in info.lo), tuple(int(v) for v in info.ext)
        self.knn_status = None          # one device int32 of `knn`, made by its first call

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

    @property
    def sorted_idx(self) -> torch.Tensor:
        """[M] int32, a view of the index buffer: the original index of every sorted position - a permutation of [0, M) in which the
        points of a cell are neighbours.  As `order` of `knn` for the cloud against itself it makes a wave's queries share cells."""
        off = int(self.info.sorted_idx) - self._buf.data_ptr()
        return self._buf[off:off + 4 * self.M].view(torch.int32)

    def knn(self, points, k: int, radius: float, exclude_self: bool = False, self_base: int = 0, order=None,
            want: Sequence[str] = ("d2", "idx", "count")):
        """The k nearest reference points within `radius` of every query under the order (d2, reference index) - sta_knn_query of
        include/sta_knn.h, the raw call -> dict of device tensors: "d2" [Q,k] float64 ascending (+inf: unused slot), "idx" [Q,k] int32
        (-1), "count" [Q] int32.  exclude_self: query i skips reference point self_base + i (the cloud against itself, whole or a chunk
        that starts at row self_base).  order: a device permutation [Q] int32 that says which queries share a wave, never a bit of the
        output.  `knn_status` (one device int32, zero unless the index or `order` was no valid one) is not read here.
        Asynchronous on the current stream."""
        unknown = set(want) - {"d2", "idx", "count"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        qry = _points(points, self.device)
        Q = qry.shape[0]
        k = int(k)
        r = knn_check(self.M, Q, k, radius, self.cell)
        dev = self.device
        if order is not None:
            order = torch.as_tensor(order).to(dev, torch.int32).contiguous()
            if tuple(order.shape) != (Q,):
                raise ValueError(f"order must be [{Q}] (got {tuple(order.shape)})")
        out = {}
        with torch.cuda.device(dev):
            if self.knn_status is None:
                self.knn_status = torch.zeros(1, device=dev, dtype=torch.int32)
            if "d2" in want:
                out["d2"] = torch.empty(Q, k, device=dev, dtype=torch.float64)
            if "idx" in want:
                out["idx"] = torch.empty(Q, k, device=dev, dtype=torch.int32)
            if "count" in want:
                out["count"] = torch.empty(Q, device=dev, dtype=torch.int32)

            def ptr(key):
                return out[key].data_ptr() if key in out else None
            try:
                _lib.check_knn(_lib.load_knn().sta_knn_query(C.byref(self.info), qry.data_ptr(), Q, order.data_ptr() if order is not None else None,
                                                             int(self_base) if exclude_self else -1, k, r, ptr("d2"), ptr("idx"), ptr("count"),
                                                             self.knn_status.data_ptr(), _stream(dev)))
            except _lib.StaError as e:
                raise _value_error(e) from None
        return out


# ---------------------------------------------------------------------------------------------------------
# Neighbourhoods: libsta_knn.so (include/sta_knn.h holds the contract, tests/knn_cases.py restates it in numpy).
#
# Stated differences from Open3D's remove_statistical_outlier / remove_radius_outlier / estimate_normals, which were not available to
# compare against and are restated from memory:
#   - `radius` is mandatory: the grid needs a bound (at most 32 cells), and a sparse neighbourhood uses fewer than k points;
#   - in the two filters a point is not its own neighbour (self is excluded), so nb_neighbors / nb_points count OTHER points;
#   - the statistical filter uses the SAMPLE standard deviation (n - 1);
#   - normals are oriented towards a viewpoint, per point or one for all, or by the sign of their largest component: there is no
#     consistent-tangent-plane propagation.
KNN_MAX_K = 64
KNN_RECORD = 8
KNN_MIN_COUNT = 3
KNN_STATUS_BOUND, KNN_STATUS_ORDER = 1, 2
# Lists of a wrapper beyond this many bytes (12 per neighbour slot) are taken in query chunks.  The chunk is a function of k alone
# (`knn_chunk_rows`), so what a wrapper returns is a function of its inputs alone.
KNN_LIST_BYTES = 256 << 20
# Default cell of the wrappers as a fraction of the radius.  NOBODY HAS MEASURED THIS: tools/knn_bench.py times radius, radius / 2 and
# radius / 4, and the default changes only on that evidence.
KNN_CELL_FRACTION = 0.5


class KnnPlan(NamedTuple):
    d2_bytes: int
    idx_bytes: int
    work_bytes: int


def knn_plan(M: int, Q: int, k: int) -> KnnPlan:
    """Host only, no library needed: the byte counts sta_knn_plan reports (tests compare the two) and its refusals as ValueError."""
    M, Q, k = int(M), int(Q), int(k)
    if not 1 <= M <= MAX_POINTS:
        raise ValueError(f"knn_plan: M must be in [1, 2^30) (got {M})")
    if not 1 <= Q <= MAX_POINTS:
        raise ValueError(f"knn_plan: Q must be in [1, 2^30) (got {Q})")
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn_plan: k must be in [1, {KNN_MAX_K}] (got {k})")
    return KnnPlan(8 * Q * k, 4 * Q * k, _align(min((Q + 255) // 256, 2048) * KNN_RECORD * 8))


def knn_check(M: int, Q: int, k: int, radius=None, cell=None, min_count=None) -> Optional[float]:
    """Host only: every refusal of sta_knn_query (radius, cell given) and sta_knn_moments (min_count given) as ValueError, with the
    library's words.  -> the radius as a float."""
    for name, v in (("M", M), ("Q", Q)):
        if not 1 <= int(v) <= MAX_POINTS:
            raise ValueError(f"knn: {name} must be in [1, 2^30) (got {int(v)})")
    if not 1 <= int(k) <= KNN_MAX_K:
        raise ValueError(f"knn: k must be in [1, {KNN_MAX_K}] (got {int(k)})")
    if min_count is not None and int(min_count) < KNN_MIN_COUNT:
        raise ValueError(f"knn_moments: min_count must be at least {KNN_MIN_COUNT} (got {int(min_count)})")
    if radius is None:
        return None
    r = float(radius)
    if not (np.isfinite(r) and r >= 0.0):
        raise ValueError("knn_query: radius must be finite and >= 0 (got %g)" % r)
    if cell is not None and r > MAX_RINGS * float(cell):
        raise ValueError("knn_query: radius %.17g is more than %d cells of %.17g" % (r, MAX_RINGS, float(cell)))
    return r


def knn_chunk_rows(k: int) -> int:
    """Queries per chunk of a wrapper: the most whose lists fit KNN_LIST_BYTES, a multiple of 256."""
    return max(256, (KNN_LIST_BYTES // (12 * int(k))) & ~255)


def _viewpoint(viewpoint, device) -> torch.Tensor:
    """one camera centre -> three float64 on the host (a Python list keeps its doubles); per-point centres -> [Q,3] fp32 on the device"""
    if not isinstance(viewpoint, torch.Tensor):
        viewpoint = torch.from_numpy(np.array(viewpoint, dtype=np.float64 if np.ndim(viewpoint) == 1 else np.float32))
    if viewpoint.dim() == 1:
        if viewpoint.numel() != 3:
            raise ValueError(f"viewpoint must be [3] or [Q, 3] (got {tuple(viewpoint.shape)})")
        return viewpoint.to("cpu", torch.float64)
    return _points(viewpoint, device)


def knn_moments(ref, lists, points=None, viewpoint=None, min_count: int = KNN_MIN_COUNT,
                want: Sequence[str] = ("normal", "curv", "mean_dist", "record")):
    """The moments of the neighbourhoods in `lists` (a dict of `NNIndex.knn` with "d2", "idx", "count") - sta_knn_moments, the raw
    call -> dict of device tensors: "normal" [Q,3] float32, "curv" [Q] float64, "mean_dist" [Q] float64, "record" [8] float64.
    ref [M,3]: the reference cloud in its original order.  points [Q,3]: the queries, needed with a viewpoint.  viewpoint: None (the
    largest component of a normal is positive), three numbers (one camera centre) or [Q,3] (each point's own).  Asynchronous."""
    unknown = set(want) - {"normal", "curv", "mean_dist", "record"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    ref = _points(ref)
    dev = ref.device
    idx, count = lists["idx"], lists["count"]
    d2 = lists.get("d2")
    Q, k = idx.shape
    knn_check(ref.shape[0], Q, k, min_count=min_count)
    if d2 is None and ("mean_dist" in want or "record" in want):
        raise ValueError("knn_moments: mean_dist and record need the d2 list")
    view, view_host, qry = None, None, None
    if viewpoint is not None:
        if points is None:
            raise ValueError("knn_moments: a viewpoint needs the query points")
        qry = _points(points, dev)
        view = _viewpoint(viewpoint, dev)
        if view.dim() == 1:
            view, view_host = None, (C.c_double * 3)(*view.tolist())
        elif view.shape[0] != Q:
            raise ValueError(f"viewpoint must be [3] or [{Q}, 3] (got {tuple(view.shape)})")
    out = {}
    with torch.cuda.device(dev):
        if "normal" in want:
            out["normal"] = torch.empty(Q, 3, device=dev, dtype=torch.float32)
        if "curv" in want:
            out["curv"] = torch.empty(Q, device=dev, dtype=torch.float64)
        if "mean_dist" in want:
            out["mean_dist"] = torch.empty(Q, device=dev, dtype=torch.float64)
        work, wb = None, 0
        if "record" in want:
            out["record"] = torch.empty(KNN_RECORD, device=dev, dtype=torch.float64)
            wb = knn_plan(1, Q, k).work_bytes
            work = torch.empty(wb, device=dev, dtype=torch.uint8)

        def ptr(t):
            return t.data_ptr() if t is not None else None
        _lib.check_knn(_lib.load_knn().sta_knn_moments(ref.data_ptr(), ref.shape[0], ptr(qry), Q, ptr(d2), idx.data_ptr(), count.data_ptr(), k, ptr(view),
                                                       view_host, int(min_count), ptr(out.get("normal")), ptr(out.get("curv")), ptr(out.get("mean_dist")),
                                                       ptr(out.get("record")), ptr(work), wb, _stream(dev)))
    return out


def _neighbourhoods(points, k, radius, index, cell, exclude_self, viewpoint, min_count, want):
    """The cloud against itself, whole or in the chunks of `knn_chunk_rows`: -> (dict of the wanted moments and "count", each over
    all M points; "record" is the sum of the chunks' records in chunk order, added on the device)."""
    pts = _points(points)
    M = pts.shape[0]
    knn_check(M, M, k, radius, min_count=min_count)
    if index is None:
        index = NNIndex.build(pts, float(radius) * KNN_CELL_FRACTION if cell is None else float(cell))
    elif index.M != M:
        raise ValueError(f"the index holds {index.M} points, the cloud {M}")
    view = _viewpoint(viewpoint, pts.device) if viewpoint is not None else None
    if view is not None and view.dim() == 2 and view.shape[0] != M:
        raise ValueError(f"viewpoint must be [3] or [{M}, 3] (got {tuple(view.shape)})")
    rows = knn_chunk_rows(k)
    sidx = index.sorted_idx
    lists_want = ("d2", "idx", "count") if ("mean_dist" in want or "record" in want) else ("idx", "count")
    if not want:
        lists_want = ("count",)

    def moments(lists, qry, v):
        o = knn_moments(pts, lists, qry, v, min_count, want) if want else {}
        o["count"] = lists["count"]
        return o
    if M <= rows:
        return moments(index.knn(pts, k, radius, exclude_self=exclude_self, order=sidx, want=lists_want), pts, view)
    rank = torch.empty(M, device=pts.device, dtype=torch.int64)
    rank[sidx.long()] = torch.arange(M, device=pts.device)          # where every point stands in the sorted order
    parts = []
    for s in range(0, M, rows):
        e = min(s + rows, M)
        order = torch.argsort(rank[s:e]).to(torch.int32)
        lists = index.knn(pts[s:e], k, radius, exclude_self=exclude_self, self_base=s, order=order, want=lists_want)
        parts.append(moments(lists, pts[s:e], view[s:e] if (view is not None and view.dim() == 2) else view))
    out = {key: torch.cat([p[key] for p in parts]) for key in parts[0] if key != "record"}
    if "record" in want:
        rec = parts[0]["record"].clone()
        for p in parts[1:]:
            rec = rec + p["record"]
        out["record"] = rec
    return out


def estimate_normals(points, k: int = 30, *, radius: float, viewpoint=None, index: Optional[NNIndex] = None, cell: Optional[float] = None,
                     min_count: int = KNN_MIN_COUNT, return_curvature: bool = False):
    """Normals of a cloud from the covariance of each point's k nearest points within `radius` (the point itself is one of them), after
    Open3D's estimate_normals with a hybrid search, restated from memory -> [M,3] float32 on the device [, curvature [M] float64 =
    l0 / (l0 + l1 + l2), the surface variation].  The normal is the eigenvector of the smallest eigenvalue (8 Jacobi sweeps in
    float64), NaN where fewer than min_count points are in reach.  viewpoint: None (the component of largest magnitude is made
    positive), [3] (one camera centre) or [M,3] (each point's own, which a SLAM cloud knows): the normal points to it.  There is no
    consistent-tangent-plane orientation.  index: an NNIndex over the same points; otherwise one is built with `cell`
    (default radius * KNN_CELL_FRACTION), which synchronises the stream once."""
    out = _neighbourhoods(points, k, radius, index, cell, False, viewpoint, min_count, ("normal", "curv") if return_curvature else ("normal",))
    return (out["normal"], out["curv"]) if return_curvature else out["normal"]


def _kept(mask):
    return torch.nonzero(mask).reshape(-1), mask


def remove_statistical_outlier(points, nb_neighbors: int = 20, std_ratio: float = 2.0, *, radius: float, index: Optional[NNIndex] = None,
                               cell: Optional[float] = None):
    """Open3D's remove_statistical_outlier, restated from memory -> (kept indices [int64, ascending], mask [M] bool), on the device.
    Every point's mean distance to its nb_neighbors nearest OTHER points within `radius` (fewer where the neighbourhood is sparse);
    over the points with at least one neighbour mean = r1 / r0 and the SAMPLE deviation std = sqrt(max(0, (r2 - r0*mean*mean) / (r0 - 1)))
    (0 for r0 <= 1), on the host in float64 from the record's one 64-byte readback (which waits for the stream); a point is kept iff
    its mean distance <= mean + std_ratio * std.  A point with no neighbour in the radius is removed."""
    out = _neighbourhoods(points, nb_neighbors, radius, index, cell, True, None, KNN_MIN_COUNT, ("mean_dist", "record"))
    r = out["record"].cpu().numpy()
    r0, r1, r2 = float(r[0]), float(r[1]), float(r[2])
    mean = r1 / r0 if r0 > 0 else 0.0
    std = float(np.sqrt(max(0.0, (r2 - r0 * mean * mean) / (r0 - 1.0)))) if r0 > 1 else 0.0
    return _kept(out["mean_dist"] <= mean + float(std_ratio) * std)          # (+inf, a point without neighbours, is above every threshold)


def remove_radius_outlier(points, nb_points: int, radius: float, *, index: Optional[NNIndex] = None, cell: Optional[float] = None):
    """Open3D's remove_radius_outlier, restated from memory -> (kept indices [int64, ascending], mask [M] bool), on the device: a point
    is kept iff at least nb_points OTHER points lie within `radius` (inclusive) - a k-NN query with k = nb_points whose list is full."""
    out = _neighbourhoods(points, nb_points, radius, index, cell, True, None, KNN_MIN_COUNT, ())
    return _kept(out["count"] >= int(nb_points))


def filter_outliers(points, outlier):
    """`outlier` = ("statistical", nb, ratio, radius) or ("radius", nb, radius) -> (kept indices, mask) of the filter it names."""
    kind = outlier[0]
    if kind == "statistical" and len(outlier) == 4:
        return remove_statistical_outlier(points, int(outlier[1]), float(outlier[2]), radius=float(outlier[3]))
    if kind == "radius" and len(outlier) == 3:
        return remove_radius_outlier(points, int(outlier[1]), float(outlier[2]))
    raise ValueError(f'outlier must be ("statistical", nb, ratio, radius) or ("radius", nb, radius) (got {outlier!r})')


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
