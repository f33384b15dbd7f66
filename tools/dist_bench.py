"""libsta_dist.so on one GPU: the build of the triangle index, query passes of surface samples of a simplified copy against the original
mesh, the same answer from a chunked float64 torch brute force, and evaluate.eval_mesh in both modes.

    python tools/dist_bench.py [runs]      # default 20 runs per measurement; medians between device events

Scene: the mesh of tools/tsdf_bench.py's procedural 16 x 12 x 4 m room fused from 40 views of 224 x 224 at voxel_size 0.05 (about 1 M
vertices and 2 M triangles).  Queries: area-uniform samples (surface.sample_surface) of simplify.simplify_mesh(mesh, 4 voxels), 200 000 and
2 M of them, at radius 0.5 and +inf, as they are and with 5 % of them moved 5 m away (beyond the radius: unmatched at 0.5, a long walk at
+inf).  The torch brute force evaluates the header's closest point for every (query, triangle) pair in float64, 64 queries at a time, on
the first 200 000 triangles and 20 000 queries, takes the smallest d2 and the lowest index among equals; every tri must be equal.  The
split of the build into sort, refit and the rest comes from a kernel trace of this tool, not from the tool itself."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                              # noqa: E402
import torch                                                                    # noqa: E402
from vista_slam_amd import evaluate, meshdist, simplify, surface, tsdf         # noqa: E402

runs = next((int(v) for v in sys.argv[1:] if v.isdigit()), 20)
VOXEL, H0, W0 = 0.05, 224, 224
SIZE = (16.0, 12.0, 4.0)
dev = torch.device("cuda:0")


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
    return tsdf.views(depths, torch.ones(V), K, poses, torch.ones(V, H0, W0, device=dev), imgs, conf_thres=0.5, device=dev)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, n=None):
    fn()
    return float(np.median([once(fn) for _ in range(runs if n is None else n)]))


def torch_closest_d2(q, a, b, c):
    """d2 [Q, T] float64 of include/sta_dist.h: q [Q,1,3], a, b, c [1,T,3] float64; one torch operation per written step"""
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    ab, ac, ap = b - a, c - a, q - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = q - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = q - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    denom = 1.0 / ((va + vb) + vc)
    p = (a + ab * (vb * denom)[..., None]) + ac * (vc * denom)[..., None]
    for cond, val in (((va <= 0) & (e1 >= 0) & (e2 >= 0), b + (c - b) * (e1 / (e1 + e2))[..., None]),
                      ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * (d2 / (d2 - d6))[..., None]),
                      ((d6 >= 0) & (d5 <= d6), c.expand_as(p)),
                      ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * (d1 / (d1 - d3))[..., None]),
                      ((d3 >= 0) & (d4 <= d3), b.expand_as(p)),
                      ((d1 <= 0) & (d2 <= 0), a.expand_as(p))):
        p = torch.where(cond[..., None], val, p)
    lo, hi = torch.minimum(torch.minimum(a, b), c), torch.maximum(torch.maximum(a, b), c)
    p = torch.where(p >= lo, p, lo.expand_as(p))
    p = torch.where(p <= hi, p, hi.expand_as(p))
    d = q - p
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def torch_brute(verts, tris, q, chunk=64):
    P = verts.to(torch.float64)[tris.long()]
    a, b, c = P[None, :, 0], P[None, :, 1], P[None, :, 2]
    ids = torch.arange(len(tris), device=dev)
    big = torch.full((), len(tris), device=dev)
    d2o, trio = torch.empty(len(q), dtype=torch.float64, device=dev), torch.empty(len(q), dtype=torch.int64, device=dev)
    for s in range(0, len(q), chunk):
        dd = torch_closest_d2(q[s:s + chunk].to(torch.float64)[:, None, :], a, b, c)
        m = dd.min(dim=1).values
        d2o[s:s + chunk] = m
        trio[s:s + chunk] = torch.where(dd == m[:, None], ids[None, :], big).min(dim=1).values
    return d2o, trio.to(torch.int32)


print(f"{torch.cuda.get_device_name(0)}; medians of {runs} runs between device events", flush=True)
v = room_views(40, 2740)
mesh = tsdf.TSDFVolume(dev, VOXEL).allocate(v).integrate(v).mesh()
nv, nt = len(mesh.vertices), len(mesh.triangles)
p = meshdist.plan(nt, 2_000_000)
idx = meshdist.TriIndex.build(mesh)
cnt = idx.counters.tolist()
print(f"the room of tools/tsdf_bench.py, 40 views of {H0} x {W0}, voxel {VOXEL}: {nv} vertices, {nt} triangles; fan-out {meshdist.FANOUT}, {idx.levels} levels, "
      f"{idx.level_offset[idx.levels]} nodes, index {p.index_bytes / 2 ** 20:.1f} MiB, build workspace {p.build_work_bytes / 2 ** 20:.1f} MiB; counters {cnt}", flush=True)
print(f"TriIndex.build (with its allocations, no readback): {median_ms(lambda: meshdist.TriIndex.build(mesh)):.3f} ms", flush=True)

small = simplify.simplify_mesh(mesh, 4 * VOXEL)
for n in (200_000, 2_000_000):
    q = surface.sample_surface(small, n, seed=1).points
    far = q.clone()
    far[::20] += 5.0
    for name, pts in (("all near the surface", q), ("5 % moved 5 m away", far)):
        for radius in (0.5, float("inf")):
            ms = median_ms(lambda: idx.query(pts, radius))
            tri = idx.query(pts, radius, want=("tri",))[0]
            print(f"query of {n} samples of the 4-voxel simplified mesh, {name}, radius {radius}: {ms:.3f} ms ({int((tri >= 0).sum())} matched); "
                  f"status {int(idx.counters[4])}", flush=True)
    ms = median_ms(lambda: idx.query(q, 0.5, want=("d2",)))
    print(f"    the same {n} near queries at radius 0.5, d2 only: {ms:.3f} ms", flush=True)

# the brute force, on a size torch can hold
sub = tsdf.Mesh(mesh.vertices, None, mesh.triangles[:200_000].contiguous())
sub_idx = meshdist.TriIndex.build(sub)
qs = surface.sample_surface(small, 20_000, seed=2).points
t_nat, t_torch = [], []
for _ in range(3):                                  # alternating; three runs: the brute force takes seconds
    t_nat.append(once(lambda: meshdist.TriIndex.build(sub).query(qs)))
    t_torch.append(once(lambda: torch_brute(sub.vertices, sub.triangles, qs)))
d2n, trin, _pt = sub_idx.query(qs)
d2t, trit = torch_brute(sub.vertices, sub.triangles, qs)
print(f"20 000 queries against the first 200 000 triangles, radius +inf: build + query {float(np.median(t_nat)):.3f} ms, torch float64 brute force in chunks of 64 "
      f"queries {float(np.median(t_torch)):.1f} ms (3 runs each, alternating); tri {'all equal' if torch.equal(trin, trit) else 'DIFFER: ' + str(int((trin != trit).sum()))}, "
      f"d2 {'all equal' if torch.equal(d2n, d2t) else 'differ in ' + str(int((d2n != d2t).sum()))}", flush=True)

# eval_mesh in both modes, next to the table of tools/simplify_bench.py
for k in (2, 4, 8):
    s = simplify.simplify_mesh(mesh, k * VOXEL)
    for mode in ("samples", "surface"):
        r = evaluate.eval_mesh(dev, s, mesh, n_samples=200000, mode=mode)
        ms = median_ms(lambda: evaluate.eval_mesh(dev, s, mesh, n_samples=200000, mode=mode), 5)
        print(f"eval_mesh(simplified at {k} voxels ({len(s.triangles)} triangles), original, n_samples=200000, threshold 0.05, mode={mode!r}): accuracy {r.accuracy:.5f} "
              f"completion {r.completion:.5f} precision {r.precision:.4f} completion ratio {r.completion_ratio:.4f} F {r.fscore:.4f}; {ms:.1f} ms (median of 5, "
              f"with its readbacks)", flush=True)
r = evaluate.eval_mesh(dev, mesh, mesh, n_samples=200000, mode="samples")
s = evaluate.eval_mesh(dev, mesh, mesh, n_samples=200000, mode="surface")
print(f"the original against itself: samples mode accuracy {r.accuracy:.5f} completion {r.completion:.5f} F {r.fscore:.4f}; surface mode accuracy {s.accuracy:.3e} "
      f"completion {s.completion:.3e} F {s.fscore:.4f}", flush=True)
