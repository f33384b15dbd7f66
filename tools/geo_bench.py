"""Geometric consistency (sta_view_consistency / sta_symmetric_geo_mask) against a torch restatement of the reference's loops
(slam_utils.py:269-419: a Python double loop of small launches with a torch.inverse per view pair; two median() calls behind
boolean-mask compactions) on the same GPU, in the same process, alternating; and row f6 (sta_geo_valid_mask,
sta_local_pointclouds, sta_ray_depth) against a torch restatement of slam_utils.py:82-266 (batched tensor statements, one
boolean-mask compaction and one torch.quantile - a full sort - per call).

    python tools/geo_bench.py [reps]          # default 20 repetitions per case and side, medians

Votes: n = 64 and 400 views of 224x224 and n = 64 of 384x512, window 4.  Masks: P = 5 edges at both sizes (the torch side runs
the reference's single-edge function P times, as slam.py would).  f6: B = 5 and 16 at 224x224, B = 8 at 384x512, q = 0.8.  Prints microseconds per call, votes/s (pixel-neighbour pairs)
or mask pixels/s, the bytes touched over time (depth in, result out, and the gathers, which mostly hit L2), and whether the two
sides agree.  Times are host wall-clock around a synchronised call: what a caller waits for, launch overhead included - that
overhead IS the reference's cost at this scale."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
import torch.nn.functional as F                            # noqa: E402
import geo_cases as G                                      # noqa: E402
from vista_slam_amd import geo, weights as W               # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)


def torch_votes(depth, Ks, Ts, thr=0.05, window=4):
    n, H, W_ = depth.shape
    dev = depth.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W_, device=dev), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], 0).float().reshape(3, -1)
    out = torch.zeros(n, H, W_, dtype=torch.int32, device=dev)
    for i in range(n):
        cam = (torch.inverse(Ks[i]) @ pix) * depth[i].reshape(1, -1)
        world = (Ts[i] @ torch.cat([cam, torch.ones_like(cam[:1])], 0))[:3].T
        world_h = torch.cat([world, torch.ones_like(world[:, :1])], 1)
        votes = torch.zeros(H * W_, device=dev)
        for j in range(max(0, i - window), min(n, i + window + 1)):
            if j == i:
                continue
            cam_j = (world_h @ torch.inverse(Ts[j]).T)[:, :3]
            z = cam_j[:, 2].clamp(min=1e-6)
            uvw = cam_j @ Ks[j].T
            uv = (uvw[:, :2] / uvw[:, 2:]).reshape(1, H, W_, 2).clone()
            uv[..., 0] = uv[..., 0] / (W_ - 1) * 2 - 1
            uv[..., 1] = uv[..., 1] / (H - 1) * 2 - 1
            s = F.grid_sample(depth[j][None, None], uv, mode="bilinear", align_corners=True).reshape(-1)
            votes += ((s - z).abs() < thr).int()
        out[i] = votes.reshape(H, W_)
    return out


def torch_mask(depths, K, T12):
    _, H, W_ = depths.shape
    dev = depths.device
    u, v = torch.meshgrid(torch.arange(W_, device=dev), torch.arange(H, device=dev), indexing="xy")
    uv1 = torch.stack([u, v, torch.ones_like(u)], 0).float().reshape(3, -1)
    Kinv = torch.inverse(K)
    masks = []
    for src, tgt, T in ((depths[0], depths[1], T12), (depths[1], depths[0], torch.inverse(T12))):
        cam = (Kinv @ uv1) * src.reshape(1, -1)
        pts = (T @ torch.cat([cam, torch.ones_like(cam[:1])], 0))[:3]
        proj = K @ pts
        r = (proj[:2] / (proj[2:] + 1e-8)).round().long()
        valid = (r[0] >= 0) & (r[0] < W_) & (r[1] >= 0) & (r[1] < H)
        idx = r[:, valid]
        err = (tgt[idx[1], idx[0]] - pts[2][valid]).abs()
        thres = 2 * err.median() if err.numel() > 0 else 1e10
        mk = torch.zeros(H * W_, dtype=torch.bool, device=dev)
        mk[valid] = err < thres
        masks.append(mk.reshape(H, W_))
    return torch.stack(masks)


def torch_q_mask(depth1, depth2, K1, K2, T1, T2, q):
    """slam_utils.py:193-266, statement by statement."""
    B, H, W_ = depth1.shape
    dev = depth1.device
    uu, vv = torch.meshgrid(torch.arange(W_, device=dev), torch.arange(H, device=dev), indexing="xy")
    uv = torch.stack([uu, vv], dim=-1).float()[None].expand(B, H, W_, 2)
    z = depth1
    fx, fy, cx, cy = (K1[:, a, b][:, None, None] for a, b in ((0, 0), (1, 1), (0, 2), (1, 2)))
    x = (uv[..., 0] - cx) * z / fx
    y = (uv[..., 1] - cy) * z / fy
    pts1 = torch.cat([torch.stack([x, y, z], dim=-1), torch.ones_like(z)[..., None]], dim=-1).view(B, -1, 4).transpose(1, 2)
    world = (T1 @ pts1).transpose(1, 2)[..., :3]
    world_h = torch.cat([world, torch.ones_like(world[..., :1])], dim=-1).transpose(1, 2)
    cam2 = (torch.inverse(T2) @ world_h).transpose(1, 2)[..., :3]
    x2, y2, z2 = cam2[..., 0], cam2[..., 1], cam2[..., 2]
    u2 = K2[:, 0, 0][:, None] * x2 / z2 + K2[:, 0, 2][:, None]
    v2 = K2[:, 1, 1][:, None] * y2 / z2 + K2[:, 1, 2][:, None]
    uv2 = torch.stack([v2, u2], dim=-1).int()
    valid = (uv2[..., 0] >= 0) & (uv2[..., 0] < H) & (uv2[..., 1] >= 0) & (uv2[..., 1] < W_)
    uv2[~valid] = 0
    bi = torch.arange(B, device=dev).view(B, 1).expand(B, H * W_)
    error = (z2 - depth2[bi, uv2[..., 0], uv2[..., 1]]).abs()
    thres = torch.quantile(error[valid], q)
    return ((error < thres) & valid).view(B, H, W_)


def _rays(K, n, H, W_):
    dev = K.device
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W_, device=dev), indexing="ij")
    pix = torch.stack((x, y, torch.ones_like(x)), dim=-1).float().reshape(-1, 3)
    return torch.bmm(torch.inverse(K), pix.T.unsqueeze(0).expand(n, 3, H * W_)).permute(0, 2, 1).reshape(n, H, W_, 3)


def torch_points(depths, K):
    """slam_utils.py:82-121 (batched intrinsics)."""
    n, H, W_ = depths.shape
    return _rays(K, n, H, W_) * depths[..., None]


def torch_ray_depth(pts, K):
    """slam_utils.py:124-165 (batched intrinsics)."""
    n, H, W_, _ = pts.shape
    rays = _rays(K, n, H, W_)
    return torch.sum(pts * (rays / torch.norm(rays, dim=-1, keepdim=True)), dim=-1)


def views(n, H, W_):
    """n views of the fixtures' room: 8 distinct ones walked back and forth, so that neighbours stay neighbours."""
    d, K, T = G.scene(8, H, W_, seed=11)
    idx = [k % 14 if k % 14 < 8 else 14 - k % 14 for k in range(n)]
    return (torch.from_numpy(a[idx]).cuda() for a in (d, K, T))


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, r


def run(tag, ours, ref, work, unit, nbytes, same):
    for f in (ours, ref):
        f()
    t = {"hip": [], "torch": []}
    for _ in range(reps):
        us, a = clock(ours); t["hip"].append(us)
        us, b = clock(ref); t["torch"].append(us)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"{tag:34s} hip {med['hip']:10.1f} us (min {min(t['hip']):9.1f})  torch {med['torch']:12.1f} us (min {min(t['torch']):11.1f})  "
          f"torch / hip {med['torch'] / med['hip']:8.1f}   hip: {work / med['hip']:8.1f} M{unit}/s, {nbytes / med['hip'] / 1e3:7.2f} GB/s touched; "
          f"{same(a, b)}", flush=True)


print(f"medians of {reps} alternating repetitions, host wall-clock around one synchronised call, {torch.cuda.get_device_name(0)}")
for n, H, W_ in ((64, 224, 224), (400, 224, 224), (64, 384, 512)):
    d, K, T = views(n, H, W_)
    pairs = sum(min(n, i + 5) - max(0, i - 4) - 1 for i in range(n)) * H * W_
    run(f"votes n={n} {H}x{W_} window 4", lambda: geo.view_consistency_check(m, d, K, T), lambda: torch_votes(d, K, T), pairs, "votes",
        n * H * W_ * 8 + pairs * 16,                        # depth in, count out, four 4-byte gathers per vote (L2)
        lambda a, b: f"differs from torch at {int((a != b).sum())} of {a.numel()} pixels")
for H, W_ in ((224, 224), (384, 512)):
    P = 5
    dv, Kv, Tv = (t.cpu().numpy() for t in views(P + 2, H, W_))
    edges = [G.scene_pair(dv, np.repeat(Kv[:1], P + 2, 0), Tv, p, p + 2) for p in range(P)]
    d, K, T = (torch.from_numpy(np.stack([e[q] for e in edges])).cuda() for q in range(3))
    run(f"masks P={P} {H}x{W_}", lambda: geo.symmetric_geo_valid_masks(m, d, K, T),
        lambda: torch.stack([torch_mask(d[p], K[p], T[p]) for p in range(P)]), 2 * P * H * W_, "px",
        2 * P * H * W_ * 33,                                # depth 4 + gather 4 + err out 4, 3 radix passes x 4, err in 4 + mask out 1
        lambda a, b: f"differs from torch at {int((a != b).sum())} of {a.numel()} pixels")

# f6.  Pairs (view k, view k + 1) of the walked room (never a view with itself); bytes: depth1 4 + gather 4 + err out 4, 3 radix reads x 4, err in 4 + mask out 1 = 29 B
# per mask pixel; 16 B per point (depth in, 3 floats out); 16 B per ray depth (3 floats in, 1 out).
for B, H, W_ in ((5, 224, 224), (16, 224, 224), (8, 384, 512)):
    d, K, T = views(B + 1, H, W_)
    a = tuple(t.contiguous() for t in (d[:B], d[1:], K[:B], K[1:], T[:B], T[1:]))
    px = B * H * W_
    run(f"quantile masks B={B} {H}x{W_} q=0.8", lambda: geo.geo_valid_masks(m, *a, 0.8), lambda: torch_q_mask(*a, 0.8), px, "px", px * 29,
        lambda x, y: f"differs from torch at {int((x != y).sum())} of {x.numel()} pixels")
    pts = geo.compute_local_pointclouds(m, d[:B], K[:B])
    run(f"local points N={B} {H}x{W_}", lambda: geo.compute_local_pointclouds(m, d[:B], K[:B]), lambda: torch_points(d[:B], K[:B]), px, "px", px * 16,
        lambda x, y: f"max distance from torch {float(((x - y).abs().amax(-1) / y.norm(dim=-1)).max()):.2e} of the point's norm")
    run(f"ray depths B={B} {H}x{W_}", lambda: geo.depth_from_pointcloud_dot_batched(m, pts, K[:B]), lambda: torch_ray_depth(pts, K[:B]), px, "px", px * 16,
        lambda x, y: f"max distance from torch {float(((x - y).abs() / y.abs()).max()):.2e} relative")
