"""libsta_reg.so on one GPU: one fused registration pass next to the composition it replaces, a whole ICP in both modes from a known
offset, and evaluate.eval_mesh(refine="plane").

    python tools/reg_bench.py [runs]      # default 20 runs per measurement; medians between device events

Scene: the mesh of tools/tsdf_bench.py's procedural 16 x 12 x 4 m room fused from 40 views of 224 x 224 at voxel_size 0.05 (about 1 M
vertices and 2 M triangles); the queries are surface samples of it under a small known motion.  The composition: cloud.transform (which
rounds the moved point to float32, so its matches are not bit for bit the pass's) + TriIndex.query + the same 50 sums in torch float64
on the device.  The two are timed alternating.  Nobody measured any of this before and no target is set: the numbers are reported, not
asserted."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                              # noqa: E402
import torch                                                                    # noqa: E402
from vista_slam_amd import cloud, evaluate, meshdist, surface, tsdf             # noqa: E402

runs = next((int(v) for v in sys.argv[1:] if v.isdigit()), 20)
VOXEL, H0, W0 = 0.05, 224, 224
SIZE = (16.0, 12.0, 4.0)
dev = torch.device("cuda:0")
RADIUS = 0.2


def room_views(V, seed):
    """tools/tsdf_bench.py's: V cameras on an ellipse at mid height, looking outwards and slightly ahead along the loop"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.arange(V, dtype=torch.float64) * (2 * np.pi / V)
    pos = torch.stack([8.0 + 4.0 * torch.cos(a), 6.0 + 3.0 * torch.sin(a), torch.full_like(a, 2.0) + 0.5 * torch.sin(3 * a)], 1)
    yaw = a + 0.6
    fwd = torch.stack([torch.cos(yaw), torch.sin(yaw), torch.zeros_like(a)], 1)
    down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).expand(V, 3)
    right = torch.linalg.cross(down, fwd)
    poses = torch.eye(4, dtype=torch.float64).repeat(V, 1, 1)
    poses[:, :3, 0], poses[:, :3, 1], poses[:, :3, 2], poses[:, :3, 3] = right, down, fwd, pos
    poses = poses.float()
    K = torch.tensor([[112.0, 0, 111.5], [0, 112.0, 111.5], [0, 0, 1]]).repeat(V, 1, 1)
    P = poses.double().to(dev)
    iy, ix = torch.meshgrid(torch.arange(H0, dtype=torch.float64, device=dev), torch.arange(W0, dtype=torch.float64, device=dev), indexing="ij")
    dc = torch.stack([(ix - 111.5) / 112.0, (iy - 111.5) / 112.0, torch.ones_like(ix)], -1)
    depths = torch.empty(V, H0, W0, device=dev)
    size = torch.tensor(SIZE, dtype=torch.float64, device=dev)
    for v in range(V):
        dw = dc @ P[v, :3, :3].T
        t = torch.where(dw > 0, (size - P[v, :3, 3]) / dw, torch.where(dw < 0, -P[v, :3, 3] / dw, torch.full_like(dw, float("inf")))).min(-1).values
        depths[v] = t.float()
    depths += 0.01 * torch.randn(V, H0, W0, device=dev, generator=g)
    imgs = torch.rand(V, 3, H0, W0, device=dev, generator=g) * 2 - 1
    return tsdf.views(depths, torch.ones(V), K, poses, torch.ones(V, H0, W0, device=dev), imgs, conf_thres=0.5, device=dev), poses


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def motion(angle, shift, centre):
    """`angle` rad about (1, 2, 3) through `centre`, then `shift` along (2, -1, 2) / 3"""
    R = meshdist.exp_so3(angle * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))
    return np.concatenate([R, (centre - R @ centre + shift * np.array([2.0, -1.0, 2.0]) / 3.0)[:, None]], axis=1)


def composition(idx, q, T, pivot, r2):
    """what one had before the pass: move and round the cloud, query it, reduce the same 50 sums in torch float64 -> [64]"""
    tri9 = idx.tri
    moved = cloud.transform(q, T)
    d2, tri, point = idx.query(moved, RADIUS)
    hit = tri >= 0
    qd, c = moved.double(), point.double()
    # the input index -> the sorted position, for the corners (the pass keeps the position; here the inverse of src is one scatter)
    pos = torch.empty(idx.nt, dtype=torch.int64, device=dev)
    pos[idx.src.long()] = torch.arange(idx.nt, device=dev)
    P = tri9[pos[tri.clamp(min=0).long()]].double().view(-1, 3, 3)
    n = torch.linalg.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nhat = n / n.norm(dim=1, keepdim=True)
    r = ((qd - c) * nhat).sum(dim=1)
    x = qd - torch.as_tensor(pivot, device=dev)
    J = torch.cat([torch.linalg.cross(x, nhat), nhat], dim=1)
    w = hit.double()
    z = lambda t: torch.where(hit.view(-1, *[1] * (t.dim() - 1)), t, torch.zeros_like(t))
    fin = torch.isfinite(qd).all(dim=1)
    out = torch.zeros(64, dtype=torch.float64, device=dev)
    out[0], out[1], out[2] = fin.sum(), w.sum(), z(d2).sum()
    out[3] = torch.where(hit, d2, torch.full_like(d2, r2))[fin].sum()
    out[4:7], out[7:10], out[10:19] = z(qd).sum(0), z(c).sum(0), (z(qd)[:, :, None] * z(c)[:, None, :]).sum(0).reshape(9)
    out[19] = (~fin).sum()
    out[21], out[22] = z(r * r).sum(), z(r.abs()).sum()
    Jz = z(J)
    out[23:29] = (Jz * z(r)[:, None]).sum(0)
    iu = torch.triu_indices(6, 6, device=dev)
    out[29:50] = (Jz.T @ Jz)[iu[0], iu[1]]
    return out


print(f"{torch.cuda.get_device_name(0)}; medians of {runs} runs between device events", flush=True)
views, poses = room_views(40, 2740)
mesh = tsdf.TSDFVolume(dev, VOXEL).allocate(views).integrate(views).mesh()
nv, nt = len(mesh.vertices), len(mesh.triangles)
idx = meshdist.TriIndex.build(mesh)
print(f"the room of tools/tsdf_bench.py, 40 views of {H0} x {W0}, voxel {VOXEL}: {nv} vertices, {nt} triangles; fan-out {meshdist.FANOUT}, {idx.levels} levels, "
      f"{meshdist.reg_plan(nt).nodes} nodes; counters {idx.counters.tolist()}", flush=True)
centre = np.array([8.0, 6.0, 2.0])
M = motion(0.01, 0.05, centre)          # the known offset: 0.01 rad about the room's centre (0.1 m at its walls) and 0.05 m
Minv = np.concatenate([M[:, :3].T, (-M[:, :3].T @ M[:, 3])[:, None]], axis=1)

for n in (200_000, 2_000_000):
    s = surface.sample_surface(mesh, n, seed=1, normals=True)
    q = cloud.transform(s.points, M)
    pivot = M[:, :3] @ centre + M[:, 3]
    fused, comp = [], []
    for k in range(runs + 1):                      # alternating; the first pair warms up
        a = once(lambda: idx.register_pass(q, Minv, RADIUS, pivot=pivot))
        b = once(lambda: composition(idx, q, Minv, pivot, RADIUS * RADIUS))
        if k:
            fused.append(a)
            comp.append(b)
    rec = idx.register_pass(q, Minv, RADIUS, pivot=pivot)[0].cpu().numpy()
    ref = composition(idx, q, Minv, pivot, RADIUS * RADIUS).cpu().numpy()
    geo = [k for k in range(50) if k not in (2, 3) and not 21 <= k <= 28]          # the sums that hold neither d2 nor the residual r
    each = np.abs(rec - ref)[geo] / np.maximum(np.abs(rec[geo]), 1e-300)
    rel, worst = float(each.max()), geo[int(each.argmax())]
    all_ms = float(np.median([once(lambda: idx.register_pass(q, Minv, RADIUS, pivot=pivot, want=meshdist.REG_WANT)) for _ in range(runs)]))
    nrm_ms = float(np.median([once(lambda: idx.register_pass(q, Minv, RADIUS, s.normals, 0.5, pivot)) for _ in range(runs)]))
    query_ms = float(np.median([once(lambda: idx.query(q, RADIUS)) for _ in range(runs)]))
    print(f"{n} samples, radius {RADIUS}: one fused pass (record only) {float(np.median(fused)):.3f} ms; the composition (cloud.transform + TriIndex.query + 50 torch "
          f"float64 sums) {float(np.median(comp)):.3f} ms (alternating); the pass with every per-query output {all_ms:.3f} ms, with normals and min_cos 0.5 "
          f"{nrm_ms:.3f} ms; TriIndex.query alone {query_ms:.3f} ms; matched {int(rec[1])} of {int(rec[0])}, by the composition {int(ref[1])}; largest relative "
          f"difference of the 40 sums without d2 and the residual {rel:.2e} (entry {worst}: {rec[worst]:.6e} fused, {ref[worst]:.6e} composed; the median of the 40 {float(np.median(each)):.2e}); sqrt(sum d2 / matched) {np.sqrt(rec[2] / rec[1]):.3e} fused, {np.sqrt(ref[2] / ref[1]):.3e} composed; sqrt(sum r^2 / matched) {np.sqrt(rec[21] / rec[1]):.3e} fused, "
          f"{np.sqrt(ref[21] / ref[1]):.3e} composed (the composition rounds the moved point to float32: here the distance IS that rounding); status "
          f"{int(idx.reg_status)}", flush=True)

s = surface.sample_surface(mesh, 200_000, seed=1, normals=True)
q = cloud.transform(s.points, M)
for mode in ("plane", "point"):
    ms = float(np.median([once(lambda: meshdist.icp(q, idx, RADIUS, mode=mode)) for _ in range(5)]))
    r = meshdist.icp(q, idx, RADIUS, mode=mode)
    err = np.abs(cloud.compose(r.T[:3], M) - np.eye(4)[:3]).max()
    print(f"icp(mode={mode!r}) of 200000 samples from the known offset (0.01 rad, 0.05 m), max_corr {RADIUS}, with its readbacks: {ms:.2f} ms (5 runs); "
          f"{r.iterations} iterations, {r.status}, fitness {r.fitness:.5f}, inlier rmse {r.inlier_rmse:.3e}, |T o M - I| {err:.2e}", flush=True)

moved = tsdf.Mesh(cloud.transform(mesh.vertices, M), None, mesh.triangles)
for refine in (None, "plane"):
    ms = float(np.median([once(lambda: evaluate.eval_mesh(dev, moved, mesh, n_samples=200000, mode="surface", refine=refine, refine_max_corr=RADIUS)) for _ in range(5)]))
    r = evaluate.eval_mesh(dev, moved, mesh, n_samples=200000, mode="surface", refine=refine, refine_max_corr=RADIUS)
    print(f"eval_mesh(the room moved by the offset, the room, n_samples=200000, mode='surface', refine={refine!r}), with its readbacks: {ms:.2f} ms (5 runs); accuracy "
          f"{r.accuracy:.3e} completion {r.completion:.3e} f-score {r.fscore:.4f}"
          + ("" if r.T is None else f", |T o M - I| {np.abs(cloud.compose(r.T[:3], M) - np.eye(4)[:3]).max():.2e}"), flush=True)
