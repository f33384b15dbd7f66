"""The contract of sta_voxel_downsample (include/sta_mi355.h) restated in numpy, a brute force of the same contract in plain Python,
the case table of tests/test_voxel_gpu.py and its builders.  Nothing here touches the GPU or the library.

The restatement: float64 index arithmetic floor((double(p) - o) / voxel_size), integer keys (iz, iy, ix) packed relative to the
grid's corner, argsort(kind="stable"), np.add.at in sorted order (= ascending input index inside a voxel), mean = float64 sum /
count rounded once to float32.  Open3D orders its rows by a hash map and was not available to compare against, so this file is the
yardstick."""
import math

import numpy as np

F32 = np.float32
MAX_EXTENT = 1 << 21
TILE = 1024            # keys per workgroup of a sort pass (csrc/voxel.h VOX_TILE)
LONG = 1024            # rows of more points are reduced by a workgroup instead of a wave (VOX_LONG)


def grid_of(pts, voxel_size, origin=None):
    """(finite mask, o [3] float64) of a call, o = None when no point is kept."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    finite = np.isfinite(pts).all(axis=1)
    if not finite.any():
        return finite, None
    if origin is not None:
        return finite, np.asarray(origin, np.float64)
    mn = pts[finite].min(axis=0)                      # float32, exact
    return finite, mn.astype(np.float64) - float(voxel_size) * 0.5


def expected(pts, col=None, *, voxel_size, origin=None, min_points=1):
    """dict(points, colors, counts, index, inverse, V, n_dropped, key_bits); ValueError for a grid the library refuses."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    M = len(pts)
    vs = float(voxel_size)
    finite, o = grid_of(pts, vs, origin)
    out = {"n_dropped": int(M - finite.sum()), "inverse": np.full(M, -1, np.int32), "key_bits": 0}
    empty = {"points": np.zeros((0, 3), F32), "colors": np.zeros((0, 3), F32), "counts": np.zeros(0, np.int32),
             "index": np.zeros((0, 3), np.int32), "V": 0}
    if o is None:
        return {**out, **empty}
    kept = np.flatnonzero(finite)
    P = pts[kept].astype(np.float64)
    I = np.floor((P - o) / vs)
    lo, hi = I.min(axis=0), I.max(axis=0)
    assert lo.min() >= -2.0 ** 31 and hi.max() < 2.0 ** 31
    I = I.astype(np.int64)
    lo = lo.astype(np.int64)
    ext = (hi.astype(np.int64) - lo + 1).tolist()
    if max(ext) > MAX_EXTENT:
        raise ValueError("voxel grid too wide: %d x %d x %d voxels at voxel_size %g (at most %d per axis)" % (*ext, vs, MAX_EXTENT))
    nx, ny, nz = [int(e - 1).bit_length() for e in ext]
    R = I - lo
    key = (R[:, 2] << (nx + ny)) | (R[:, 1] << nx) | R[:, 0]                 # < 2^63: fits int64
    order = np.argsort(key, kind="stable")
    sk = key[order]
    head = np.ones(len(sk), bool)
    head[1:] = sk[1:] != sk[:-1]
    seg = np.cumsum(head) - 1                                               # voxel of every sorted position
    U = int(seg[-1]) + 1
    counts = np.bincount(seg, minlength=U).astype(np.int64)
    sums = np.zeros((U, 3), np.float64)
    np.add.at(sums, seg, P[order])
    csum = np.zeros((U, 3), np.float64)
    if col is not None:
        np.add.at(csum, seg, np.asarray(col, F32).reshape(-1, 3)[kept][order].astype(np.float64))
    keep = counts >= int(min_points)
    row = np.where(keep, np.cumsum(keep) - 1, -1)
    first = np.flatnonzero(head)
    out["inverse"][kept[order]] = row[seg].astype(np.int32)
    out["key_bits"] = nx + ny + nz
    n = counts[keep].astype(np.float64)[:, None]
    return {**out, "points": (sums[keep] / n).astype(F32), "colors": (csum[keep] / n).astype(F32),
            "counts": counts[keep].astype(np.int32), "index": I[order][first][keep].astype(np.int32), "V": int(keep.sum())}


def brute_force(pts, col=None, *, voxel_size, origin=None, min_points=1):
    """The same contract with a dict of lists and Python floats, point by point (small inputs)."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    vs = float(voxel_size)
    kept = [i for i in range(len(pts)) if all(math.isfinite(float(v)) for v in pts[i])]
    inverse = [-1] * len(pts)
    if not kept:
        return {"points": [], "colors": [], "counts": [], "index": [], "inverse": inverse, "V": 0, "n_dropped": len(pts)}
    if origin is None:
        o = [float(min(pts[i][a] for i in kept)) - vs * 0.5 for a in range(3)]
    else:
        o = [float(v) for v in origin]
    cells = {}
    for i in kept:                                                          # ascending input index
        ix, iy, iz = (math.floor((float(pts[i][a]) - o[a]) / vs) for a in range(3))
        cells.setdefault((iz, iy, ix), []).append(i)
    res = {"points": [], "colors": [], "counts": [], "index": [], "inverse": inverse, "n_dropped": len(pts) - len(kept)}
    for cell in sorted(cells):
        members = cells[cell]
        if len(members) < min_points:
            continue
        s, c = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for i in members:
            for a in range(3):
                s[a] += float(pts[i][a])
                if col is not None:
                    c[a] += float(col[i][a])
        for i in members:
            inverse[i] = len(res["counts"])
        res["points"].append([F32(v / len(members)) for v in s])
        res["colors"].append([F32(v / len(members)) for v in c])
        res["counts"].append(len(members))
        res["index"].append([cell[2], cell[1], cell[0]])
    res["V"] = len(res["counts"])
    return res


# ------------------------------------------------------------------------------------------ builders
def lattice(rng, M, lo=-64.0, hi=64.0):
    """Coordinates that are multiples of 2^-6 in [lo, hi) within [-64, 64): every float64 sum of up to 2^20 of them is exact."""
    return (rng.integers(int(lo * 64), int(hi * 64), size=(M, 3)) / 64.0).astype(F32)


def lattice_colors(rng, M):
    return (rng.integers(0, 257, size=(M, 3)) / 256.0).astype(F32)


def by_index(rng, idx, frac=(0.0, 0.25)):
    """Points of given voxel indices on the unit grid whose corner is (-0.5, -0.5, -0.5): index + a dyadic fraction below 0.5.  The
    first point is the corner voxel's (0, 0, 0) exactly, so that the default origin is that corner."""
    idx = np.asarray(idx, np.int64)
    p = idx.astype(np.float64) + rng.choice(np.asarray(frac), size=idx.shape)
    p[0] = 0.0
    assert (idx[0] == 0).all()
    out = p.astype(F32)
    assert np.array_equal(out.astype(np.float64), p)                        # representable: the case is what it says it is
    return out


def width_case(rng, ext, M=3000):
    """Random voxels of a grid of ext = (ex, ey, ez) voxels with both extreme corners present: key width = sum of bit_length(e - 1)."""
    idx = np.stack([rng.integers(0, e, size=M) for e in ext], axis=1)
    idx[0] = 0
    idx[1] = [e - 1 for e in ext]
    return by_index(rng, idx)


def segments(rng, lengths):
    """One voxel per entry of `lengths` along x on the unit grid, voxel j holding lengths[j] points; shuffled input order."""
    idx = np.zeros((sum(lengths), 3), np.int64)
    idx[:, 0] = np.repeat(np.arange(len(lengths)), lengths)
    perm = np.concatenate([[0], 1 + rng.permutation(len(idx) - 1)])
    return by_index(rng, idx[perm], frac=(0.0, 0.25, 0.125, 0.375))


def poison(pts, where, rng):
    """NaN / +inf / -inf in one coordinate of the points at `where`."""
    pts = pts.copy()
    bad = [np.nan, np.inf, -np.inf]
    for n, i in enumerate(where):
        pts[i, int(rng.integers(0, 3))] = bad[n % 3]
    return pts


def _case(pts, col, voxel_size, origin=None, min_points=1, exact=True):
    return {"pts": pts, "col": col, "voxel_size": voxel_size, "origin": origin, "min_points": min_points, "exact": exact}


def _sized(M):
    def make(rng):
        return _case(lattice(rng, M, -2.0, 2.0), lattice_colors(rng, M), 0.5)
    return make


def _hostile_normal(rng):
    M = 200000
    return _case((rng.standard_normal((M, 3)) * 3).astype(F32), rng.random((M, 3)).astype(F32), 0.05, exact=False)


def _hostile_one_voxel(rng):
    M = 37000
    return _case((rng.random((M, 3)) * 0.1 + 100).astype(F32), rng.random((M, 3)).astype(F32), 1.0, exact=False)


def _nan_positions(M):
    return sorted({0, M - 1, 255, 256, 257, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE} & set(range(M)))


# name -> builder(rng) -> case dict.  `exact`: every float64 sum of the case is exact, the means are compared with array_equal.
CASES = {
    # size boundaries: one point, the wave, the workgroup, more than 1024 workgroups of 256 (the single-block scan's per > 1 path) and
    # more than 256 sort tiles (the histogram scan's second chunk)
    **{f"m{M}": _sized(M) for M in (1, 63, 64, 65, 255, 256, 257)},
    "m300000": lambda rng: _case(lattice(rng, 300000, -8.0, 8.0), lattice_colors(rng, 300000), 0.25),
    "m300000_27bit": lambda rng: _case(lattice(rng, 300000), lattice_colors(rng, 300000), 0.25),
    # segment shapes
    "one_voxel_300000": lambda rng: _case(lattice(rng, 300000, 0.0, 0.5), lattice_colors(rng, 300000), 1.0),
    "all_distinct": lambda rng: _case(by_index(rng, np.stack(np.unravel_index(np.concatenate([[0], 1 + rng.permutation(4999)]), (10, 20, 25)), 1)),
                                      lattice_colors(rng, 5000), 1.0),
    "alternating_1_1000": lambda rng: _case(segments(rng, [1, 1000] * 20), lattice_colors(rng, 20020), 1.0),
    "long_row_threshold": lambda rng: _case(segments(rng, [LONG - 1, LONG, LONG + 1, 1, 2 * LONG + 1, 64, 65]), lattice_colors(rng, 5 * LONG + 132), 1.0),
    # key widths: pass skipping and the packing edge
    "width_1": lambda rng: _case(width_case(rng, (2, 1, 1)), None, 1.0),
    "width_8": lambda rng: _case(width_case(rng, (8, 8, 4)), None, 1.0),
    "width_9": lambda rng: _case(width_case(rng, (8, 8, 8)), None, 1.0),
    "width_16": lambda rng: _case(width_case(rng, (64, 32, 32)), None, 1.0),
    "width_17": lambda rng: _case(width_case(rng, (64, 64, 32)), None, 1.0),
    "width_63": lambda rng: _case(width_case(rng, (MAX_EXTENT, MAX_EXTENT, MAX_EXTENT)), None, 1.0),
    "extent_2p21_on_y": lambda rng: _case(width_case(rng, (4, MAX_EXTENT, 4)), None, 1.0),
    # a key that fills its digits AND dropped points: the extra pass that keeps the all-ones key behind every voxel
    "width_8_nan": lambda rng: _case(poison(width_case(rng, (8, 8, 4)), _nan_positions(3000)[1:], rng), None, 1.0),
    "width_16_nan": lambda rng: _case(poison(width_case(rng, (64, 32, 32)), _nan_positions(3000)[1:], rng), None, 1.0),
    "one_voxel_nan": lambda rng: _case(poison(lattice(rng, 3000, 0.0, 0.5), _nan_positions(3000), rng), lattice_colors(rng, 3000), 1.0),
    # grid placement
    "faces_default": lambda rng: _case(lattice(rng, 4000, -1.0, 1.0), lattice_colors(rng, 4000), 0.25),
    "faces_origin": lambda rng: _case(lattice(rng, 4000, -1.0, 1.0), lattice_colors(rng, 4000), 0.25, origin=(0.0, 0.0, 0.0)),
    "negative": lambda rng: _case(lattice(rng, 4000, -64.0, -60.0), lattice_colors(rng, 4000), 0.5),
    "origin_negative_index": lambda rng: _case(lattice(rng, 4000, -4.0, 4.0), lattice_colors(rng, 4000), 0.5, origin=(10.0, 20.0, 30.0)),
    # non-finite points
    "nan_scatter": lambda rng: _case(poison(lattice(rng, 2100, -2.0, 2.0), _nan_positions(2100), rng), lattice_colors(rng, 2100), 0.5),
    "all_nonfinite": lambda rng: _case(poison(lattice(rng, 300, -2.0, 2.0), range(300), rng), lattice_colors(rng, 300), 0.5),
    # min_points
    "min_points_2": lambda rng: _case(lattice(rng, 2000, -2.0, 2.0), lattice_colors(rng, 2000), 0.5, min_points=2),
    "min_points_5": lambda rng: _case(lattice(rng, 2000, -2.0, 2.0), lattice_colors(rng, 2000), 0.5, min_points=5),
    "min_points_filters_all": lambda rng: _case(lattice(rng, 2000, -2.0, 2.0), lattice_colors(rng, 2000), 0.5, min_points=2001),
    "no_colors": lambda rng: _case(lattice(rng, 2000, -2.0, 2.0), None, 0.5),
    # hostile floats: the sums round, the means are within one float32 step of any order of summation
    "hostile_normal": _hostile_normal,
    "hostile_one_voxel": _hostile_one_voxel,
}
SMALL = ("m1", "m63", "m64", "m65", "m257", "width_1", "width_9", "faces_default", "faces_origin", "negative", "origin_negative_index",
         "nan_scatter", "all_nonfinite", "min_points_2", "min_points_5", "min_points_filters_all", "no_colors")
TOO_WIDE = (MAX_EXTENT + 1, 4, 4)


def build(name):
    return CASES[name](np.random.default_rng(1700 + sorted(CASES).index(name)))


def too_wide(rng=None):
    """Extent 2^21 + 1 on x: refused."""
    return width_case(rng or np.random.default_rng(1699), TOO_WIDE)


_expected = {}


def expected_of(name):
    """The restatement's answer for a case, computed once and shared (read only)."""
    if name not in _expected:
        c = build(name)
        _expected[name] = (c, expected(c["pts"], c["col"], voxel_size=c["voxel_size"], origin=c["origin"], min_points=c["min_points"]))
    return _expected[name]


def wall_scene():
    """Six views of 48 x 64 looking down +z at a rippled wall 4 m away, stepping 1.5 m along x - except view 1, which stands 0.1 m
    from view 0 and sees the same part of the wall.  -> depths, scales, K, poses, confs, imgs (float32) and a confidence threshold."""
    rng = np.random.default_rng(1777)
    N, H, W = 6, 48, 64
    y, x = np.mgrid[0:H, 0:W]
    K = np.zeros((N, 3, 3), F32)
    K[:, 0, 0] = K[:, 1, 1] = 60.0
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W / 2, H / 2, 1.0
    poses = np.tile(np.eye(4, dtype=F32), (N, 1, 1))
    poses[:, 0, 3] = [0.0, 0.1, 1.5, 3.0, 4.5, 6.0]
    depths = np.stack([4.0 + 0.05 * np.sin(0.3 * x + n) * np.cos(0.2 * y) for n in range(N)]).astype(F32)
    scales = (1.0 + 0.01 * rng.standard_normal(N)).astype(F32)
    confs = (1.0 + rng.random((N, H, W))).astype(F32)
    imgs = (rng.random((N, 3, H, W)) * 2 - 1).astype(F32)
    return depths, scales, K, poses, confs, imgs, 1.2
