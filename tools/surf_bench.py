"""sta_surf_components, sta_surf_weights, sta_surf_sample, a whole clean_mesh and a whole eval_mesh on one GPU, each next to a torch
composition of the same result on the same GPU.

    python tools/surf_bench.py [runs]          # default 20 runs per measurement; medians between device events, the two sides alternating

Scene: the mesh of tools/tsdf_bench.py's procedural 16 x 12 x 4 m room fused from 40 views of 224 x 224 at voxel_size 0.05 (about 1 M
vertices and 2 M triangles).  The torch compositions: for the labels, `scatter_reduce_(amin)` over the triangles' corners plus one pointer
jump per round, until nothing changes (one host readback per round); for the sampler, the weights, `cumsum` in float64 and
`searchsorted` on the same stratified positions.  The tool says which results are identical: the labels and counts must be; cumsum's
order is not the header's, so the prefixes need not be - the largest relative difference, the share of samples whose triangle index
agrees and the share whose point has the same bits are printed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                   # noqa: E402
import torch                                                         # noqa: E402
from vista_slam_amd import _lib, evaluate, surface, tsdf            # noqa: E402

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


def torch_components(tris, nv):
    """(vlabel, tlabel, tcount) of include/sta_surf.h with torch alone; the triangles are all valid here.  -> also the number of rounds"""
    t = tris.to(torch.int64)
    lab = torch.arange(nv, device=dev)
    rounds = 0
    while True:
        m = lab[t].amin(dim=1)
        new = lab.clone()
        for k in range(3):
            new.scatter_reduce_(0, t[:, k], m, "amin")
        new = torch.minimum(new, new[new])
        rounds += 1
        if torch.equal(new, lab):
            break
        lab = new
    named = torch.zeros(nv, dtype=torch.bool, device=dev)
    named[t.reshape(-1)] = True
    tlabel = lab[t[:, 0]]
    return torch.where(named, lab, -1).to(torch.int32), tlabel.to(torch.int32), torch.bincount(tlabel, minlength=nv).to(torch.int32), rounds


def _lsr(z, s):
    return (z >> s) & ((1 << (64 - s)) - 1)            # a logical shift of an int64


def _wrap(c):
    return c - (1 << 64) if c >= 1 << 63 else c


def torch_units(seed, ns):
    """splitmix64 in wrapping int64 -> u [ns,3] float64"""
    k = torch.arange(ns, dtype=torch.int64, device=dev)
    out = []
    for j in range(3):
        z = _wrap(seed) + (3 * k + (j + 1)) * _wrap(0x9E3779B97F4A7C15)
        z = (z ^ _lsr(z, 30)) * _wrap(0xBF58476D1CE4E5B9)
        z = (z ^ _lsr(z, 27)) * _wrap(0x94D049BB133111EB)
        z = z ^ _lsr(z, 31)
        out.append(_lsr(z, 11).to(torch.float64) * 2.0 ** -53)
    return torch.stack(out, 1)


def torch_prefix(verts, tris):
    """-> (cumsum of |(B - A) x (C - A)| in float64, A, B, C)"""
    V = verts.to(torch.float64)
    t = tris.to(torch.int64)
    A, B, Cc = V[t[:, 0]], V[t[:, 1]], V[t[:, 2]]
    w = torch.linalg.cross(B - A, Cc - A).norm(dim=1)
    return torch.cumsum(torch.where(torch.isfinite(w), w, 0.0), 0), A, B, Cc


def torch_sample(verts, tris, ns, seed=0):
    P, A, B, Cc = torch_prefix(verts, tris)
    u = torch_units(seed, ns)
    x = (torch.arange(ns, dtype=torch.float64, device=dev) + u[:, 0]) / ns * P[-1]
    pick = torch.searchsorted(P, x, right=True).clamp_(max=len(P) - 1)
    r = u[:, 1].sqrt()
    b0, b1, b2 = (1 - r)[:, None], (r * (1 - u[:, 2]))[:, None], (r * u[:, 2])[:, None]
    return (b0 * A[pick] + b1 * B[pick] + b2 * Cc[pick]).float(), pick.to(torch.int32)


print(f"{torch.cuda.get_device_name(0)}; medians of {runs} runs between device events, the native call and the torch composition alternating", flush=True)
v = room_views(40, 2740)
mesh = tsdf.TSDFVolume(dev, VOXEL).allocate(v).integrate(v).mesh()
nv, nt = len(mesh.vertices), len(mesh.triangles)
print(f"the room of tools/tsdf_bench.py, 40 views of {H0} x {W0}, voxel {VOXEL}: {nv} vertices, {nt} triangles", flush=True)

# components
got = surface.components(mesh, return_status=True)
ref = torch_components(mesh.triangles, nv)
same = all(torch.equal(a, b) for a, b in zip(got[:3], ref[:3]))
sizes = got[2][got[2] > 0]
t_native, t_torch = alternating(lambda: surface.components(mesh), lambda: torch_components(mesh.triangles, nv))
print(f"sta_surf_components (with its workspace and output allocations): {t_native:.3f} ms; torch scatter_reduce_(amin) + jump, {ref[3]} rounds with a readback each: "
      f"{t_torch:.3f} ms; vlabel, tlabel and tcount {'identical' if same else 'DIFFER'}; status {int(got[3].item())}; {len(sizes)} components, the largest of "
      f"{int(sizes.max())} triangles, {int((sizes < 100).sum())} of fewer than 100", flush=True)

# weights
t_w, t_wt = alternating(lambda: surface.weights(mesh), lambda: torch_prefix(mesh.vertices, mesh.triangles))
P, total = surface.weights(mesh)
Pt = torch_prefix(mesh.vertices, mesh.triangles)[0]
print(f"sta_surf_weights ({(nt + 1023) // 1024} chunks): {t_w:.3f} ms; torch cross + norm + cumsum in float64: {t_wt:.3f} ms; the prefixes are "
      f"{'identical' if torch.equal(P, Pt) else 'not identical'} (largest relative difference {float(((P - Pt).abs() / Pt).max()):.2e}); area {float(total) / 2:.3f} m^2",
      flush=True)

# samples
for ns in (200000, 2000000):
    s = surface.sample_surface(mesh, ns)
    pts, pick = torch_sample(mesh.vertices, mesh.triangles, ns)
    agree = float((s.triangles == pick).double().mean())
    same_pts = float((s.points == pts).all(dim=1).double().mean())
    pts_out, tri_out = torch.empty(ns, 3, device=dev), torch.empty(ns, dtype=torch.int32, device=dev)
    lib = _lib.load_surf()
    st = torch.cuda.current_stream().cuda_stream
    t_s, t_st = alternating(lambda: _lib.check_surf(lib.sta_surf_sample(mesh.vertices.data_ptr(), nv, mesh.triangles.data_ptr(), nt, P.data_ptr(), total.data_ptr(), None, ns, 0,
                                                                        pts_out.data_ptr(), tri_out.data_ptr(), None, None, st)),
                            lambda: torch_sample(mesh.vertices, mesh.triangles, ns))
    t_all = float(np.median([once(lambda: surface.sample_surface(mesh, ns)) for _ in range(runs)]))
    print(f"sta_surf_sample, {ns} samples: {t_s:.3f} ms (sample_surface with the weights and allocations: {t_all:.3f} ms); torch weights + cumsum + searchsorted + "
          f"generator: {t_st:.3f} ms; the same triangle for {100 * agree:.4f} % of the samples, the same point bits for {100 * same_pts:.4f} %", flush=True)

# whole calls
t_clean = float(np.median([once(lambda: surface.clean_mesh(mesh, min_triangles=100)) for _ in range(runs)]))
clean = surface.clean_mesh(mesh, min_triangles=100)
print(f"clean_mesh(min_triangles=100), with the status readback and cull_mesh: {t_clean:.3f} ms; {len(clean.vertices)} vertices and {len(clean.triangles)} triangles stay",
      flush=True)
t_eval = float(np.median([once(lambda: evaluate.eval_mesh(dev, clean, mesh, n_samples=200000)) for _ in range(runs)]))
r = evaluate.eval_mesh(dev, clean, mesh, n_samples=200000)
print(f"eval_mesh(cleaned, uncleaned, n_samples=200000), with its readbacks: {t_eval:.3f} ms; accuracy {r.accuracy:.5f} completion {r.completion:.5f} "
      f"completion ratio {r.completion_ratio:.4f} precision {r.precision:.4f} F {r.fscore:.4f}", flush=True)
