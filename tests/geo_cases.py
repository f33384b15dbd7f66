"""Geometric consistency: numpy restatements of the reference's `view_consistency_check` and
`compute_symmetric_geo_valid_mask` (vista_slam/utils/slam_utils.py:269-419), statement by statement, usable at fp32 and fp64;
the procedural scenes of the `tests/golden/geo_*.npz` fixtures; and the comparison rules those fixtures are checked by.

Both outputs are thresholded decisions, so "equal" is defined with a measured band (tools/gen_golden_geo.py):
`dev` = the largest distance between the fp32 and the fp64 evaluation of an error, `band = BAND_FACTOR * dev`; a pixel may fall
either way only where its fp64 error lies within `band` of the threshold (or its warped uv within `band_uv` of a rounding boundary).
"""
import numpy as np

BAND_FACTOR = 8.0
MAX_BORDERLINE = 0.02          # at most 2 % of a fixture's pixels may be undecided
MIN_MASK_SHARE = 0.05          # each mask value covers at least 5 % of a mask fixture
VOTE_THRESHOLD = 0.05


# ----------------------------------------------------------------------------------------------------------------------
# view_consistency_check
def _grid_sample_bilinear(img, ix, iy):
    """F.grid_sample(mode='bilinear', padding_mode='zeros') at unnormalised coordinates: a corner outside the frame adds nothing."""
    H, W = img.shape
    with np.errstate(invalid="ignore", over="ignore"):
        x0 = np.floor(ix); y0 = np.floor(iy)
        x1 = x0 + 1; y1 = y0 + 1
        out = np.zeros_like(ix)
        for xs, ys, wgt in ((x0, y0, (x1 - ix) * (y1 - iy)), (x1, y0, (ix - x0) * (y1 - iy)),
                            (x0, y1, (x1 - ix) * (iy - y0)), (x1, y1, (ix - x0) * (iy - y0))):
            inb = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
            xi = np.where(inb, xs, 0).astype(np.int64); yi = np.where(inb, ys, 0).astype(np.int64)
            out = out + np.where(inb, img[yi, xi] * wgt, 0).astype(ix.dtype)
    return out


def vote_errors(depth, intrinsics, poses, window=4, dtype=np.float32):
    """-> err [n, 2*window, H, W] (`dtype`): |sampled - z| of view i's pixels in neighbour slot s (j = i-window+s, the slot of
    j = i removed); +inf where the neighbour does not exist (it never agrees)."""
    depth = np.asarray(depth, dtype); Ks = np.asarray(intrinsics, dtype); Ts = np.asarray(poses, dtype)
    n, H, W = depth.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1).astype(dtype)
    err = np.full((n, max(2 * window, 1), H, W), np.inf, dtype)
    one = dtype(1)
    for i in range(n):
        cam = (np.linalg.inv(Ks[i]) @ pix) * depth[i].reshape(1, -1)
        world = (Ts[i] @ np.concatenate([cam, np.ones_like(cam[:1])], 0))[:3].T               # [HW,3]
        world_h = np.concatenate([world, np.ones_like(world[:, :1])], 1)
        for j in range(max(0, i - window), min(n, i + window + 1)):
            if j == i:
                continue
            cam_j = (world_h @ np.linalg.inv(Ts[j]).T)[:, :3]
            z = np.maximum(cam_j[:, 2], dtype(1e-6))
            z = np.where(np.isnan(cam_j[:, 2]), cam_j[:, 2], z)
            uvw = cam_j @ Ks[j].T
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                u = uvw[:, 0] / uvw[:, 2]; v = uvw[:, 1] / uvw[:, 2]
                # the reference normalises to [-1, 1] and grid_sample (align_corners=True) maps back
                if W > 1:
                    u = ((u / dtype(W - 1)) * dtype(2) - one + one) / dtype(2) * dtype(W - 1)
                if H > 1:
                    v = ((v / dtype(H - 1)) * dtype(2) - one + one) / dtype(2) * dtype(H - 1)
                sampled = _grid_sample_bilinear(depth[j], u, v)
                e = np.abs(sampled - z)
            s = j - (i - window)
            err[i, s - (1 if j > i else 0)] = e.reshape(H, W)
    return err


def vote_count(err, threshold):
    with np.errstate(invalid="ignore"):
        return (err < np.asarray(threshold, err.dtype)).sum(1).astype(np.int32)


def view_consistency_np(depth, intrinsics, poses, threshold=VOTE_THRESHOLD, window=4, dtype=np.float32):
    if window == 0:
        return np.zeros(np.asarray(depth).shape, np.int32)
    return vote_count(vote_errors(depth, intrinsics, poses, window, dtype), threshold)


def vote_borderline(err64, threshold, band):
    """nb [n,H,W]: the number of neighbours whose fp64 error lies within `band` of the threshold."""
    with np.errstate(invalid="ignore"):
        return (np.abs(err64 - threshold) < band).sum(1).astype(np.int32)


def check_votes(count, count_ref, nb):
    """|count - count_ref| <= nb at EVERY pixel -> the number of pixels outside the rule."""
    return int((np.abs(np.asarray(count, np.int64) - np.asarray(count_ref, np.int64)) > np.asarray(nb, np.int64)).sum())


# ----------------------------------------------------------------------------------------------------------------------
# compute_symmetric_geo_valid_mask
def sym_parts(depths, intri, relative_pose, dtype=np.float32):
    """-> dict(uv [2,2,HW], err [2,HW] (NaN-free only where valid), valid [2,HW] bool, thres [2], mask [2,H,W] bool)."""
    depths = np.asarray(depths, dtype); K = np.asarray(intri, dtype); T12 = np.asarray(relative_pose, dtype)
    _, H, W = depths.shape
    Kinv = np.linalg.inv(K)
    u, v = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    uv1 = np.stack([u, v, np.ones_like(u)], 0).reshape(3, -1).astype(dtype)
    T21 = np.linalg.inv(T12)
    res = dict(uv=[], err=[], valid=[], thres=[], mask=[])
    for d, (src, tgt, T) in enumerate(((depths[0], depths[1], T12), (depths[1], depths[0], T21))):
        cam = (Kinv @ uv1) * src.reshape(1, -1)
        pts = (T @ np.concatenate([cam, np.ones_like(cam[:1])], 0))[:3]
        proj = K @ pts
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            uv = proj[:2] / (proj[2:] + dtype(1e-8))
            r = np.round(uv)                                   # half to even, like torch.round
            valid = (r[0] >= 0) & (r[0] < W) & (r[1] >= 0) & (r[1] < H)
            xi = np.where(valid, r[0], 0).astype(np.int64); yi = np.where(valid, r[1], 0).astype(np.int64)
            err = np.abs(tgt[yi, xi] - pts[2])
        ve = err[valid]
        if ve.size == 0:
            thres = dtype(1e10)
        elif np.isnan(ve).any():
            thres = dtype(np.nan)
        else:
            thres = dtype(2) * np.sort(ve)[(ve.size - 1) // 2]          # torch.median: the lower middle element
        with np.errstate(invalid="ignore"):
            mask = valid & (err < thres)
        res["uv"].append(uv); res["err"].append(err); res["valid"].append(valid); res["thres"].append(thres)
        res["mask"].append(mask.reshape(H, W))
    return {k: np.stack(vv) for k, vv in res.items()}


def sym_border(p64, thres32, band_uv, band_err):
    """border [2,H,W] bool from the fp64 parts: uv within band_uv of a rounding boundary (.5) in either coordinate, or
    |err - thres| < band_err + 2 |thres32 - thres64| on a valid pixel."""
    _, H, W = p64["mask"].shape
    with np.errstate(invalid="ignore"):
        frac = p64["uv"] - np.floor(p64["uv"])
        near = (np.abs(frac - 0.5) < band_uv).any(1)
        tol = band_err + 2.0 * np.abs(np.asarray(thres32, np.float64) - p64["thres"].astype(np.float64))
        edge = p64["valid"] & (np.abs(p64["err"] - p64["thres"][:, None]) < tol[:, None])
    return (near | edge).reshape(2, H, W)


def check_masks(mask, mask_ref, border):
    """masks equal wherever border == 0 -> the number of pixels outside the rule."""
    return int(((np.asarray(mask, bool) != np.asarray(mask_ref, bool)) & ~np.asarray(border, bool)).sum())


# ----------------------------------------------------------------------------------------------------------------------
# the procedural scene: a camera that yaws 0.06 rad and moves (0.08, ~0, 0.05) per view through the box room
# [-2,2] x [-1.5,1.5] x [-1,4]; depth = the camera-frame z at which each pixel's z = 1 ray leaves the room (float64, rounded to
# fp32); focal length 0.9 W, growing `f_growth` per view; a smooth per-view ripple and 4 % outlier pixels on top, so
# that neighbouring views agree on most pixels, disagree on some, and the vote takes every value.  Depths lie on a grid of
# DEPTH_STEP = 2^-11 m (a sensor's half millimetre), so a fixture stores them exactly as small integers (depth_code below).
DEPTH_STEP = 2.0 ** -11
ROOM_LO = np.array([-2.0, -1.5, -1.0])
ROOM_HI = np.array([2.0, 1.5, 4.0])


def scene(n, H, W, seed=0, f_growth=0.01, first_view=0):
    """-> depth [n,H,W] fp32, K [n,3,3] fp32, poses [n,4,4] fp32 (camera-to-world)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = np.zeros((n, H, W), np.float32); Ks = np.zeros((n, 3, 3), np.float32); Ts = np.zeros((n, 4, 4), np.float32)
    for q in range(n):
        i = q + first_view
        f = 0.9 * W * (1.0 + f_growth) ** i
        K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
        a = 0.06 * i
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c = np.array([-0.5 + 0.08 * i, 0.01 * np.sin(i), 0.05 * i])
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = c
        K32 = K.astype(np.float32).astype(np.float64); T32 = T.astype(np.float32).astype(np.float64)   # the depth is true for the fp32 inputs
        x = (xs - K32[0, 2]) / K32[0, 0]; y = (ys - K32[1, 2]) / K32[1, 1]
        D = np.einsum("rc,chw->rhw", T32[:3, :3], np.stack([x, y, np.ones_like(x)], 0))
        with np.errstate(divide="ignore"):
            t_exit = np.where(D > 0, (ROOM_HI[:, None, None] - T32[:3, 3, None, None]) / D,
                              (ROOM_LO[:, None, None] - T32[:3, 3, None, None]) / D)
        d = np.nanmin(np.where(D == 0, np.inf, t_exit), 0)
        d = d + 0.03 * np.sin(6 * x + i) * np.cos(5 * y - i / 2.0)
        out = rng.random((H, W)) < 0.04
        d = np.where(out, d * (1 + 0.3 * rng.standard_normal((H, W))), d)
        depth[q] = (np.round(d / DEPTH_STEP) * DEPTH_STEP).astype(np.float32); Ks[q] = K.astype(np.float32); Ts[q] = T.astype(np.float32)
    return depth, Ks, Ts


def scene_pair(depth, Ks, Ts, a, b):
    """Views a, b of a scene as one edge: depths [2,H,W], the shared K (view a's), rel_pose = T_b^-1 T_a (cam a -> cam b) fp32."""
    rel = np.linalg.inv(Ts[b].astype(np.float64)) @ Ts[a].astype(np.float64)
    return np.stack([depth[a], depth[b]]), Ks[a].copy(), rel.astype(np.float32)


def empty_direction_pair(H, W, seed=0):
    """An edge whose direction 0 has NO valid pixel (the 1e10 path): view 0 is 0.5 m deep and the pose moves it 3 m sideways, so
    every pixel projects far outside view 1; view 1 is ~50 m deep and lands inside view 0 almost unmoved."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f = 0.9 * W
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]], np.float32)
    d0 = 0.5 + 0.05 * np.sin(xs / 7.0) * np.cos(ys / 5.0)
    d1 = 50.0 * (1 + 0.4 * np.sin(xs / 9.0 + 1) * np.cos(ys / 6.0))
    d1 = np.where(rng.random((H, W)) < 0.15, d1 * 4.0, d1)
    rel = np.eye(4, dtype=np.float32); rel[0, 3] = 3.0
    return (np.round(np.stack([d0, d1]) / DEPTH_STEP) * DEPTH_STEP).astype(np.float32), K, rel


VOTE_CASES = {      # name -> n, H, W
    "geo_vote_48x64_n6": (6, 48, 64),                  # n < 2 window + 1
    "geo_vote_64x80_n12": (12, 64, 80),
    "geo_vote_80x48_n9_portrait": (9, 80, 48),
    "geo_vote_224_n10": (10, 224, 224),
}
SYM_CASES = {       # name -> H, W, scene views, edges (a, b) | "empty"
    "geo_sym_48x64_p3": (48, 64, 6, [(0, 2), (1, 3), (2, 5)]),
    "geo_sym_224_p2": (224, 224, 4, [(0, 2), (3, 1)]),
    "geo_sym_48x64_empty": (48, 64, 3, [(0, 2), "empty"]),
}


def sym_case_inputs(name):
    """-> depths [P,2,H,W], K [P,3,3], rel_pose [P,4,4] fp32 of a mask case (shared intrinsics: f_growth = 0)."""
    H, W, n, edges = SYM_CASES[name]
    depth, Ks, Ts = scene(n, H, W, seed=7, f_growth=0.0)
    ds, ks, rs = [], [], []
    for e in edges:
        d, k, r = empty_direction_pair(H, W) if e == "empty" else scene_pair(depth, Ks, Ts, *e)
        ds.append(d); ks.append(k); rs.append(r)
    return np.stack(ds), np.stack(ks), np.stack(rs)


def depth_code(depth):
    """fp32 depths on the DEPTH_STEP grid -> int32 codes, differenced along a row (small numbers compress well); exact."""
    code = np.round(np.asarray(depth, np.float64) / DEPTH_STEP).astype(np.int64)
    assert np.array_equal((code * DEPTH_STEP).astype(np.float32), depth) and np.abs(code).max() < 2 ** 24
    return np.diff(code, axis=-1, prepend=0).astype(np.int32)


def depth_decode(code):
    return (np.cumsum(code.astype(np.int64), axis=-1) * DEPTH_STEP).astype(np.float32)


def load_case(name, golden_dir):
    """A geo_* fixture as a dict, depths decoded to fp32 and bit maps unpacked."""
    import os
    with np.load(os.path.join(golden_dir, f"{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    key = "depth" if name in VOTE_CASES else "depths"
    g[key] = depth_decode(g.pop("depth_code"))
    if name in SYM_CASES:
        shape = g["depths"].shape
        g["mask"] = unpack_bits(g["mask"], shape); g["border"] = unpack_bits(g["border"], shape)
    return g


def pack_bits(a):
    return np.packbits(np.asarray(a, bool).reshape(-1))


def unpack_bits(p, shape):
    return np.unpackbits(p)[:int(np.prod(shape))].reshape(shape).astype(bool)
