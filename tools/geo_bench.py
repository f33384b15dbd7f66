"""Geometric consistency (sta_view_consistency / sta_symmetric_geo_mask) against a torch restatement of the reference's loops
(slam_utils.py:269-419: a Python double loop of small launches with a torch.inverse per view pair; two median() calls behind
boolean-mask compactions) on the same GPU, in the same process, alternating.

    python tools/geo_bench.py [reps]          # default 20 repetitions per case and side, medians

Votes: n = 64 and 400 views of 224x224 and n = 64 of 384x512, window 4.  Masks: P = 5 edges at both sizes (the torch side runs
the reference's single-edge function P times, as slam.py would).  Prints microseconds per call, votes/s (pixel-neighbour pairs)
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
