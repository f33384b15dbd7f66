"""Quantile geometry masks, local point clouds and ray depths: numpy restatements of the reference's
`compute_geo_valid_mask_batched`, `compute_local_pointclouds` and `depth_from_pointcloud_dot_batched`
(vista_slam/utils/slam_utils.py:82-266), statement by statement, usable at fp32 and fp64; a restatement of `torch.quantile`
(linear interpolation) that is bit-exact at fp32; the cases of the `tests/golden/geo_q_*.npz` / `geo_ray_*.npz` fixtures
(tools/gen_golden_geo_q.py); and the rules those fixtures are checked by.

The mask is a thresholded decision, so "equal" carries f5's measured band over (tests/geo_cases.py): `dev_uv` / `dev_err` = the
largest distance between the fp32 and the fp64 evaluation of a warped coordinate / an error, `band = BAND_FACTOR * dev`; a pixel
may fall either way only where its fp64 uv lies within `band_uv` of an INTEGER (the target is the truncated coordinate) or its fp64
error within `band_err + 2 |thres32 - thres64|` of the threshold.  The threshold itself may move by `thr_tol = 2 band_err +
spread`, `spread` = how far the fp64 threshold moves when every uv-border pixel is counted as valid, or every one dropped.
"""
import os
from fractions import Fraction

import numpy as np

import geo_cases as G

MAX_SPREAD_REL = 1e-3          # spread <= 1e-3 x thres


# ----------------------------------------------------------------------------------------------------------------------
# torch.quantile(x, q), interpolation='linear'
def _fma32(x, y, z):
    """fp32 fused multiply-add: x * y + z rounded ONCE (exact rational arithmetic, then the nearest fp32, ties to even)."""
    x, y, z = np.float32(x), np.float32(y), np.float32(z)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float32(np.float64(x) * np.float64(y) + np.float64(z))
    exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
    with np.errstate(over="ignore"):
        best = np.float32(float(exact))                                        # rounded twice: at most one step off
    if not np.isfinite(best):
        return best
    for cand in (np.nextafter(best, np.float32(-np.inf)), np.nextafter(best, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        dc, db = abs(Fraction(float(cand)) - exact), abs(Fraction(float(best)) - exact)
        if dc < db or (dc == db and int(cand.view(np.uint32)) % 2 == 0 and int(best.view(np.uint32)) % 2 == 1):
            best = cand
    return best


def quantile_np(values, q, dtype=np.float32):
    """torch.quantile(values.flatten(), q) with the default linear interpolation.  At fp32 it repeats ATen's arithmetic:
    rank = fp32(q) * fp32(n - 1); lo = floor, hi = ceil, w = rank - lo; lerp(a, b, w) = w < 0.5 ? fma(w, b - a, a)
    : fma(-(b - a), 1 - w, b) - ONE rounding per branch (the unfused a + w * (b - a) differs from torch in the last bit on about
    one case in a hundred).  A NaN among the values gives NaN; an empty input raises like torch."""
    v = np.sort(np.asarray(values, dtype).reshape(-1))
    n = v.size
    if n == 0:
        raise RuntimeError("quantile() input tensor must be non-empty")
    if np.isnan(v).any():
        return dtype(np.nan)
    if dtype == np.float64:
        rank = float(q) * (n - 1)
        lo, hi = int(np.floor(rank)), int(np.ceil(rank))
        w = rank - lo
        a, b = v[lo], v[hi]
        return np.float64(a + w * (b - a) if w < 0.5 else b - (b - a) * (1 - w))
    f = np.float32
    rank = f(f(q) * f(n - 1))
    lo, hi = np.floor(rank), np.ceil(rank)
    w = f(rank - lo)
    a, b = v[int(lo)], v[int(hi)]
    with np.errstate(invalid="ignore", over="ignore"):
        d = f(b - a)
        return _fma32(w, d, a) if w < f(0.5) else _fma32(-d, f(f(1) - w), b)


# ----------------------------------------------------------------------------------------------------------------------
# compute_geo_valid_mask_batched (slam_utils.py:193-266)
def q_parts(depth1, depth2, K1, K2, T1, T2, q, dtype=np.float32):
    """-> dict(uv [B,2,HW] = (u2, v2), z2 [B,HW], err [B,HW], valid [B,HW] bool, count, thres, mask [B,H,W] bool).
    No valid pixel: thres = NaN and mask all False (the reference raises there; the callers decide)."""
    d1 = np.asarray(depth1, dtype); d2 = np.asarray(depth2, dtype)
    K1 = np.asarray(K1, dtype); K2 = np.asarray(K2, dtype); T1 = np.asarray(T1, dtype); T2 = np.asarray(T2, dtype)
    B, H, W = d1.shape
    uu, vv = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    uu = uu.astype(dtype); vv = vv.astype(dtype)
    uvs, z2s, errs, valids = [], [], [], []
    for b in range(B):
        z = d1[b]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            x = (uu - K1[b, 0, 2]) * z / K1[b, 0, 0]
            y = (vv - K1[b, 1, 2]) * z / K1[b, 1, 1]
            cam1 = np.stack([x, y, z, np.ones_like(z)], 0).reshape(4, -1)
            world = (T1[b] @ cam1)[:3]
            world_h = np.concatenate([world, np.ones_like(world[:1])], 0)
            cam2 = (np.linalg.inv(T2[b]) @ world_h)[:3]
            x2, y2, z2 = cam2
            u2 = K2[b, 0, 0] * x2 / z2 + K2[b, 0, 2]
            v2 = K2[b, 1, 1] * y2 / z2 + K2[b, 1, 2]
            tu, tv = np.trunc(u2), np.trunc(v2)                                # .int(): toward zero
            ok = np.isfinite(u2) & np.isfinite(v2) & (np.abs(u2) < 2.0 ** 31) & (np.abs(v2) < 2.0 ** 31)   # else INT_MIN: invalid
            valid = ok & (tv >= 0) & (tv < H) & (tu >= 0) & (tu < W)
            xi = np.where(valid, tu, 0).astype(np.int64); yi = np.where(valid, tv, 0).astype(np.int64)
            err = np.abs(z2 - d2[b][yi, xi])
        uvs.append(np.stack([u2, v2])); z2s.append(z2); errs.append(err); valids.append(valid)
    uv, z2, err, valid = np.stack(uvs), np.stack(z2s), np.stack(errs), np.stack(valids)
    count = int(valid.sum())
    thres = quantile_np(err[valid], q, dtype) if count else dtype(np.nan)
    with np.errstate(invalid="ignore"):
        mask = valid & (err < thres)
    return dict(uv=uv, z2=z2, err=err, valid=valid, count=count, thres=thres, mask=mask.reshape(B, H, W))


def q_deviation(p32, p64, H, W):
    """-> dev_uv (where |uv64| < 4 max(H, W)), dev_err (over pixels both evaluations send to the same target)."""
    with np.errstate(invalid="ignore"):
        near = np.isfinite(p64["uv"]).all(1) & (np.abs(p64["uv"]) < 4 * max(H, W)).all(1) & np.isfinite(p32["uv"]).all(1)
        dev_uv = float(np.abs(p32["uv"].astype(np.float64) - p64["uv"]).max(1)[near].max()) if near.any() else 0.0
        same = p32["valid"] & p64["valid"] & (np.trunc(p32["uv"]) == np.trunc(p64["uv"])).all(1)
        de = np.abs(p32["err"].astype(np.float64) - p64["err"])[same]
        de = de[np.isfinite(de)]
        dev_err = float(de.max()) if de.size else 0.0
    return dev_uv, dev_err


def q_uv_border(p64, band_uv):
    """[B,HW] bool: the fp64 uv lies within band_uv of an integer in either coordinate."""
    with np.errstate(invalid="ignore"):
        return (np.abs(p64["uv"] - np.rint(p64["uv"])) < band_uv).any(1)


def q_border(p64, thres32, band_uv, band_err):
    """border [B,H,W] bool: uv border, or |err - thres| < band_err + 2 |thres32 - thres64| on a valid pixel."""
    B, H, W = p64["mask"].shape
    with np.errstate(invalid="ignore"):
        tol = band_err + 2.0 * abs(float(thres32) - float(p64["thres"]))
        edge = p64["valid"] & (np.abs(p64["err"] - p64["thres"]) < tol)
    return (q_uv_border(p64, band_uv) | edge).reshape(B, H, W)


def q_spread(p64, depth2, q, band_uv):
    """How far the fp64 threshold moves when every uv-border pixel is dropped, or every one is counted as valid (a border pixel
    that is invalid but within band_uv of the frame then reads the nearest pixel of the frame)."""
    d2 = np.asarray(depth2, np.float64)
    B, H, W = d2.shape
    if p64["count"] == 0 or not np.isfinite(p64["thres"]):
        return 0.0
    uvb = q_uv_border(p64, band_uv)
    u, v = p64["uv"][:, 0], p64["uv"][:, 1]
    with np.errstate(invalid="ignore"):
        close = uvb & ~p64["valid"] & (u > -1 - band_uv) & (u < W + band_uv) & (v > -1 - band_uv) & (v < H + band_uv)
    extra = []
    for b in range(B):
        xi = np.clip(np.trunc(u[b][close[b]]), 0, W - 1).astype(np.int64); yi = np.clip(np.trunc(v[b][close[b]]), 0, H - 1).astype(np.int64)
        extra.append(np.abs(p64["z2"][b][close[b]] - d2[b][yi, xi]))
    t_all = quantile_np(np.concatenate([p64["err"][p64["valid"]]] + extra), q, np.float64)
    kept = p64["err"][p64["valid"] & ~uvb]
    t_drop = quantile_np(kept, q, np.float64) if kept.size else np.float64(np.nan)
    return float(max(abs(t_all - p64["thres"]), abs(t_drop - p64["thres"])))


def check_q_masks(mask, mask_ref, border):
    """masks equal wherever border == 0 -> the number of pixels outside the rule."""
    return G.check_masks(mask, mask_ref, border)


def thres_within(thres, thres_ref, tol):
    """|thres - thres_ref| <= tol, or both NaN."""
    a, b = float(thres), float(thres_ref)
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


# ----------------------------------------------------------------------------------------------------------------------
# compute_local_pointclouds / depth_from_pointcloud_dot_batched (slam_utils.py:82-165)
def _pix(H, W, dtype):
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([xs, ys, np.ones_like(xs)], -1).astype(dtype).reshape(-1, 3)           # [HW,3]


def local_points_np(depths, intrinsics, dtype=np.float32):
    """-> [N,H,W,3]; intrinsics [3,3] or [N,3,3]."""
    d = np.asarray(depths, dtype); K = np.asarray(intrinsics, dtype)
    N, H, W = d.shape
    Ki = np.linalg.inv(K)
    rays = _pix(H, W, dtype) @ np.swapaxes(Ki, -1, -2)                          # [HW,3] or [N,HW,3]
    rays = np.broadcast_to(rays.reshape((-1, H, W, 3)), (N, H, W, 3))
    return rays * d[..., None]


def ray_depth_np(points, intrinsics, dtype=np.float32):
    """-> [B,H,W]: the dot product of each point with the unit ray of its pixel."""
    p = np.asarray(points, dtype); K = np.asarray(intrinsics, dtype)
    B, H, W, _ = p.shape
    rays = _pix(H, W, dtype) @ np.swapaxes(np.linalg.inv(K), -1, -2)
    rays = np.broadcast_to(rays.reshape((-1, H, W, 3)), (B, H, W, 3))
    unit = rays / np.linalg.norm(rays, axis=-1, keepdims=True)
    return (p * unit).sum(-1)


def pc_distance(pc, pc64):
    """[N,H,W]: |pc - pc64|_inf / |pc64|_2 per pixel."""
    pc64 = np.asarray(pc64, np.float64)
    return np.abs(np.asarray(pc, np.float64) - pc64).max(-1) / np.linalg.norm(pc64, axis=-1)


def rd_distance(rd, rd64):
    rd64 = np.asarray(rd64, np.float64)
    return np.abs(np.asarray(rd, np.float64) - rd64) / np.abs(rd64)


# ----------------------------------------------------------------------------------------------------------------------
# cases: scenes are geo_cases.scene(n, H, W, seed=11), whose focal length grows per view, so K1 != K2.  No view is paired with
# itself: its errors are rounding noise, the quantile falls into the gap and a quarter of the pixels come out undecided.
Q_SEED = 11
Q_CASES = {         # name -> H, W, scene views, pairs (view 1, view 2), q, NaN at depth2[b, y, x] or None
    "geo_q_40x56_b3": (40, 56, 6, [(0, 2), (1, 3), (5, 2)], 0.8, None),
    "geo_q_72x40_b2_portrait": (72, 40, 6, [(0, 1), (4, 2)], 0.5, None),
    "geo_q_40x56_b4_q037": (40, 56, 7, [(0, 3), (6, 2), (2, 4), (1, 2)], 0.37, None),      # some points behind camera 2
    "geo_q_224_b3": (224, 224, 5, [(0, 2), (3, 1), (4, 0)], 0.9, None),
    "geo_q_40x56_b1_max": (40, 56, 6, [(0, 2)], 1.0, None),
    "geo_q_40x56_b2_min": (40, 56, 6, [(0, 2), (3, 4)], 0.0, None),                        # thres = the smallest error: all False
    "geo_q_40x56_b2_nan": (40, 56, 6, [(0, 2), (1, 3)], 0.8, (0, 20, 28)),                 # thres = NaN: all False
}
ALL_FALSE = ("geo_q_40x56_b2_min", "geo_q_40x56_b2_nan")
RAY_CASES = {       # name -> n, H, W
    "geo_ray_40x56_n4": (4, 40, 56),
    "geo_ray_72x40_n3_portrait": (3, 72, 40),
}


# the exact construction: torch.quantile itself is the reference
def exact_depths(B, H, W, s, seed, dup=True):
    """depth1 = code * 2^-s, code < 2^18, with duplicated values: under identity K and T and depth2 = 0 every pixel maps onto
    itself exactly and the errors ARE depth1."""
    rng = np.random.default_rng(seed)
    code = rng.integers(1, 2 ** 18, size=(B, H, W))
    if dup and code.size > 3:
        flat = code.reshape(-1)
        flat[rng.integers(0, flat.size, size=flat.size // 3)] = flat[rng.integers(0, flat.size, size=flat.size // 3)]
    return (code * 2.0 ** -s).astype(np.float32)


EXACT_SHAPES = [(1, 1, 1), (1, 1, 2), (2, 5, 7), (3, 24, 40), (1, 40, 56)]
EXACT_QS = [0, 0.1, 0.37, 0.5, 0.8, 0.9, 0.999, 1]


def q_case_inputs(name):
    """-> depth1, depth2 [B,H,W], K1, K2 [B,3,3], T1, T2 [B,4,4] fp32, q.  (The NaN of a `_nan` case is NOT applied here: the depths
    are stored as integer codes; load_q_case and the generator apply it.)"""
    H, W, n, pairs, q, _nan = Q_CASES[name]
    depth, Ks, Ts = G.scene(n, H, W, seed=Q_SEED)
    a = [p[0] for p in pairs]; b = [p[1] for p in pairs]
    return depth[a].copy(), depth[b].copy(), Ks[a].copy(), Ks[b].copy(), Ts[a].copy(), Ts[b].copy(), q


def apply_nan(name, depth2):
    nan_at = Q_CASES[name][5]
    if nan_at is not None:
        depth2 = depth2.copy(); depth2[nan_at] = np.nan
    return depth2


def load_q_case(name, golden_dir):
    with np.load(os.path.join(golden_dir, f"{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    g["depth1"] = G.depth_decode(g.pop("depth1_code"))
    g["depth2"] = apply_nan(name, G.depth_decode(g.pop("depth2_code")))
    shape = g["depth1"].shape
    g["mask"] = G.unpack_bits(g["mask"], shape); g["border"] = G.unpack_bits(g["border"], shape)
    g["uv_border"] = G.unpack_bits(g["uv_border"], shape)
    return g


def load_ray_case(name, golden_dir):
    with np.load(os.path.join(golden_dir, f"{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    g["depth"] = G.depth_decode(g.pop("depth_code"))
    return g
