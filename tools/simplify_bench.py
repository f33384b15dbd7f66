"""libsta_simp.so on one GPU: the three stages of simplify.simplify_mesh next to a torch composition of the same integer result, the sizes
that come out, how far the simplified mesh is from the original (evaluate.eval_mesh, both placements) and what a render_mesh frame
of it costs.

    python tools/simplify_bench.py [runs]      # default 20 runs per measurement; medians between device events, the two sides alternating

Scene: the mesh of tools/tsdf_bench.py's procedural 16 x 12 x 4 m room fused from 40 views of 224 x 224 at voxel_size 0.05 (about 1 M
vertices and 2 M triangles); cells of 2, 4 and 8 voxel sizes.  The torch composition: float64 cell indices packed into an int64 key,
`torch.unique(return_inverse=True)` for the ranks, `index_add_` for the float64 means, a sort of the sorted cluster triples packed into two
int64 keys and `unique_consecutive` for the distinct triples - the mean placement only, no first-of-a-set survivor, no quadrics.  The tool
says which integer results are identical: vcell and the number of cells must be, and the number of distinct triples must be the number
of output triangles."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                   # noqa: E402
import torch                                                         # noqa: E402
from vista_slam_amd import evaluate, render, simplify, tsdf         # noqa: E402

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


def alternating(f, g):
    """medians of `runs` runs of each, f and g taking turns"""
    f(); g()
    tf, tg = [], []
    for _ in range(runs):
        tf.append(once(f))
        tg.append(once(g))
    return float(np.median(tf)), float(np.median(tg))


def torch_simplify(mesh, cell):
    """-> (vcell, number of cells, mean positions per cell, mean colours per cell, number of distinct cluster triples); every vertex of the
    room is finite and in range, every triangle valid"""
    p = mesh.vertices.to(torch.float64)
    i = torch.floor(p / cell).to(torch.int64) + (1 << 20)
    key = (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0]
    uniq, inv = torch.unique(key, return_inverse=True)
    n = len(uniq)
    cnt = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, inv, torch.ones(len(p), dtype=torch.float64, device=dev))
    pos = torch.zeros(n, 3, dtype=torch.float64, device=dev).index_add_(0, inv, p) / cnt[:, None]
    col = torch.zeros(n, 3, dtype=torch.float64, device=dev).index_add_(0, inv, mesh.colors.to(torch.float64)) / cnt[:, None]
    c = inv[mesh.triangles.to(torch.int64)]
    c = c[(c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])]
    s = c.sort(dim=1).values
    hi, lo = (s[:, 0] << 31) | s[:, 1], s[:, 2]
    order = torch.argsort(lo, stable=True)
    order = order[torch.argsort(hi[order], stable=True)]
    pairs = torch.stack([hi[order], lo[order]], 1)
    distinct = torch.unique_consecutive(pairs, dim=0)
    return inv.to(torch.int32), n, pos.float(), col.float(), len(distinct)


def native(mesh, cell, placement):
    cl = simplify.cluster_triangles(mesh, cell)
    return cl, simplify.place_vertices(mesh, cl, cell, placement=placement)


def frame_ms(mesh):
    """a whole render_mesh frame up to the image on the host, 720 x 480 at ssaa 1, top-down: host wall-clock, mean of 5"""
    H, Wd = 480, 720
    cam = render.Camera.look_at([8.0, 6.0, 16.0], [8.0, 6.0, 0.0], [0.0, 1.0, 0.0], 0.75 * H, 0.75 * H, H, Wd, near=0.05, far=100.0)
    cvs = render.Canvas(dev, H, Wd, 1)
    fn = lambda: render.render_mesh(dev, cam, mesh, H=H, W=Wd, ssaa=1, canvas=cvs).cpu()
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        fn()
    return (time.perf_counter() - t0) * 1e3 / 5


print(f"{torch.cuda.get_device_name(0)}; medians of {runs} runs between device events, the native calls and the torch composition alternating", flush=True)
v = room_views(40, 2740)
mesh = tsdf.TSDFVolume(dev, VOXEL).allocate(v).integrate(v).mesh()
nv, nt = len(mesh.vertices), len(mesh.triangles)
print(f"the room of tools/tsdf_bench.py, 40 views of {H0} x {W0}, voxel {VOXEL}: {nv} vertices, {nt} triangles; a render_mesh frame (720x480, ssaa 1, top-down, "
      f"up to the image on the host) of it: {frame_ms(mesh):.2f} ms", flush=True)

for k in (2, 4, 8):
    cell = k * VOXEL
    small, maps = simplify.simplify_mesh(mesh, cell, return_maps=True)
    c = maps.counters
    ref = torch_simplify(mesh, cell)
    cl, (mv, mc) = native(mesh, cell, "mean")
    same_cells = torch.equal(cl.vcell, ref[0]) and c.cells == ref[1]
    used = cl.cell_out >= 0
    same_mean = torch.equal(mv[:c.vertices], ref[2][used[:ref[1]]]) and torch.equal(mc[:c.vertices], ref[3][used[:ref[1]]])
    t_q, t_torch = alternating(lambda: native(mesh, cell, "quadric"), lambda: torch_simplify(mesh, cell))
    t_m, _ = alternating(lambda: native(mesh, cell, "mean"), lambda: None)
    t_stage = [float(np.median([once(f) for _ in range(runs)])) for f in (lambda: simplify.cells(mesh, cell), lambda: simplify.cluster_triangles(mesh, cell))]
    t_all = float(np.median([once(lambda: simplify.simplify_mesh(mesh, cell)) for _ in range(runs)]))
    print(f"cell {cell:.2f} ({k} voxels): {c.vertices} vertices, {c.triangles} triangles ({100.0 * c.triangles / nt:.2f} % of the input); {c.cells} cells, "
          f"{c.collapsed} collapsed, {c.duplicates} duplicates, {c.dropped_vertices} dropped, {c.invalid_triangles} invalid, {c.fallbacks} fallbacks to the mean "
          f"({100.0 * c.fallbacks / max(c.vertices, 1):.2f} % of the vertices)", flush=True)
    print(f"    three stages, quadric (with their workspace and output allocations, no readback): {t_q:.3f} ms; mean placement: {t_m:.3f} ms; cells alone "
          f"{t_stage[0]:.3f} ms, cells + triangles {t_stage[1]:.3f} ms; simplify_mesh with its one readback {t_all:.3f} ms; torch unique + index_add_ + sort + "
          f"unique_consecutive (mean placement only): {t_torch:.3f} ms", flush=True)
    print(f"    vcell and the cell count {'identical' if same_cells else 'DIFFER'}; distinct triples {ref[4]} {'==' if ref[4] == c.triangles else '!='} output triangles "
          f"{c.triangles}; mean positions and colours {'identical' if same_mean else 'not identical'} to index_add_'s", flush=True)
    for placement in ("quadric", "mean"):
        s = small if placement == "quadric" else simplify.simplify_mesh(mesh, cell, placement="mean")
        r = evaluate.eval_mesh(dev, s, mesh, n_samples=200000)
        print(f"    eval_mesh({placement}, original, n_samples=200000, threshold 0.05): accuracy {r.accuracy:.5f} completion {r.completion:.5f} precision "
              f"{r.precision:.4f} completion ratio {r.completion_ratio:.4f} F {r.fscore:.4f}", flush=True)
    print(f"    a render_mesh frame of the simplified mesh: {frame_ms(small):.2f} ms", flush=True)
