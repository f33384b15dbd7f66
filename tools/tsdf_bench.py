"""The three stages of a TSDF fusion (vista_slam_amd.tsdf: sta_tsdf_blocks, sta_tsdf_integrate, sta_tsdf_mesh) between device events, and
next to the integration, alternating on the same GPU, a torch composition that produces the same tsdf / weight arrays: a float64
projection of all lattice points per view, then gather and where.

    python tools/tsdf_bench.py [reps] [torch_reps]      # default 20 runs per stage (medians), 5 of the torch composition

Scene: the procedural 16 x 12 x 4 m room of tools/voxel_bench.py, seen by 40 and 400 views of 224 x 224 from a loop inside it (depth =
z of the first wall along the pixel's ray + 1 cm of noise), voxel_size 0.05, trunc 0.15.  Printed: the medians, the block, vertex and
triangle counts, the bytes of the volume, and for the integration the float64 operations the header names and the bytes it must move,
over the kernel's time (the ceilings are in profiles/r27_tsdf.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
from vista_slam_amd import tsdf                            # noqa: E402

nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
reps = nums[0] if nums else 20
torch_reps = nums[1] if len(nums) > 1 else 5
VOXEL, H, W = 0.05, 224, 224
SIZE = (16.0, 12.0, 4.0)
dev = torch.device("cuda:0")


def room_views(V, seed):
    """V cameras on an ellipse at mid height, looking outwards and slightly ahead along the loop; K = 112 px focal length (90 degrees)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.arange(V, dtype=torch.float64) * (2 * np.pi / V)
    pos = torch.stack([8.0 + 4.0 * torch.cos(a), 6.0 + 3.0 * torch.sin(a), torch.full_like(a, 2.0) + 0.5 * torch.sin(3 * a)], 1)
    yaw = a + 0.6
    fwd = torch.stack([torch.cos(yaw), torch.sin(yaw), torch.zeros_like(a)], 1)             # camera z
    down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).expand(V, 3)                 # camera y
    right = torch.linalg.cross(down, fwd)                                                   # camera x
    poses = torch.eye(4, dtype=torch.float64).repeat(V, 1, 1)
    poses[:, :3, 0], poses[:, :3, 1], poses[:, :3, 2], poses[:, :3, 3] = right, down, fwd, pos
    poses = poses.float()
    K = torch.tensor([[112.0, 0, 111.5], [0, 112.0, 111.5], [0, 0, 1]]).repeat(V, 1, 1)
    P = poses.double().to(dev)
    iy, ix = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    dc = torch.stack([(ix - 111.5) / 112.0, (iy - 111.5) / 112.0, torch.ones_like(ix)], -1)
    depths = torch.empty(V, H, W, device=dev)
    size = torch.tensor(SIZE, dtype=torch.float64, device=dev)
    for v in range(V):
        dw = dc @ P[v, :3, :3].T
        t = torch.where(dw > 0, (size - P[v, :3, 3]) / dw, torch.where(dw < 0, -P[v, :3, 3] / dw, torch.full_like(dw, float("inf")))).min(-1).values
        depths[v] = t.float()
    depths += 0.01 * torch.randn(V, H, W, device=dev, generator=g)
    imgs = torch.rand(V, 3, H, W, device=dev, generator=g) * 2 - 1
    return tsdf.views(depths, torch.ones(V), K, poses, torch.ones(V, H, W, device=dev), imgs, conf_thres=0.5, device=dev)


def torch_integrate(vol, v):
    """tsdf / weight of sta_tsdf_integrate over all views from a cleared volume, in torch: one float64 operation per step, as written"""
    k = vol.keys
    b = torch.stack([(k & 0x1FFFFF), ((k >> 21) & 0x1FFFFF), ((k >> 42) & 0x1FFFFF)], 1) - (1 << 20)
    l = torch.arange(512, device=dev)
    i = (8 * b[:, None, :] + torch.stack([l & 7, (l >> 3) & 7, l >> 6], 1)[None]).double().reshape(-1, 3)
    x, y, z = (i[:, a] * VOXEL for a in range(3))
    n = x.numel()
    ts, wt = torch.ones(n, device=dev), torch.zeros(n, device=dev)
    trunc = torch.full((), vol.trunc, dtype=torch.float64, device=dev)
    Ts, Ks = v.w2c.cpu().tolist(), v.K.cpu().tolist()
    stats = torch.zeros(3, dtype=torch.int64, device=dev)
    for q in range(v.depths.shape[0]):
        T, K = Ts[q], Ks[q]
        pcz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11]
        pcx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]
        pcy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7]
        px, py = torch.floor(K[0] * (pcx / pcz) + K[2] + 0.5), torch.floor(K[1] * (pcy / pcz) + K[3] + 0.5)
        front = pcz > 0
        inside = front & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        pix = torch.where(inside, py * W + px, torch.zeros_like(px)).long()
        D = v.depths[q].reshape(-1).gather(0, pix).double() * float(v.scales[q])
        ob = v.obs[q].reshape(-1).gather(0, pix)
        sdf = D - pcz
        take = inside & (ob > 0) & torch.isfinite(D) & (D > 0) & ~(sdf < -trunc)
        d = torch.minimum(sdf / trunc, torch.ones_like(sdf))
        w, Wo = ob.double(), wt.double()
        den = Wo + w
        ts = torch.where(take, ((Wo * ts.double() + w * d) / den).float(), ts)
        wt = torch.where(take, torch.clamp(den, max=vol.max_weight).float(), wt)
        stats += torch.stack([front.sum(), inside.sum(), take.sum()])
    return ts.reshape(-1, 512), wt.reshape(-1, 512), stats.tolist()


def events(fn, n):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out, r


def line(name, ms):
    return f"    {name:10s} median {float(np.median(ms)):9.3f} ms   min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs)"


print(f"{torch.cuda.get_device_name(0)}; medians of {reps} runs between device events; torch composition {torch_reps} runs, alternating with the kernel")
for V in (40, 400):
    v = room_views(V, 2700 + V)
    vol = tsdf.TSDFVolume(dev, VOXEL)
    vol.allocate(v)                                         # warm-up of every stage
    vol.integrate(v)
    m = vol.mesh()
    t_blocks, _ = events(lambda: vol.allocate(v), reps)
    t_int, _ = events(lambda: vol.clear().integrate(v), reps)
    t_clear, _ = events(lambda: vol.clear(), reps)
    vol.clear().integrate(v)
    t_mesh, m = events(lambda: vol.mesh(), reps)
    t_torch, t_hip = [], []
    for _ in range(torch_reps):
        ms, ref = events(lambda: torch_integrate(vol, v), 1); t_torch += ms
        ms, _ = events(lambda: vol.clear().integrate(v), 1); t_hip += ms
    same = torch.equal(ref[0], vol.tsdf) and torch.equal(ref[1], vol.weight)
    nb, pts = vol.n_blocks, vol.n_blocks * 512
    front, inside, fused = ref[2]
    # the float64 operations the header names: 6 for pc_z of every (point, view); 22 more in front of the camera (pc_x, pc_y, two divisions,
    # u, v, two + 0.5, two floors); 1 (D) + 1 (sdf) for a pixel on the image; 2 (d) + 5 per fused value (tsdf and three colours) + 2 (weight)
    flop = 6 * pts * V + 22 * front + 2 * inside + 24 * fused
    # bytes it must move: the volume read and written once (tsdf, weight, rgb), 8 B of depth and obs per pixel lookup, 12 B of colour per fused value
    byts = pts * 20 * 2 + 8 * inside + 12 * fused
    k_ms = float(np.median(t_int)) - float(np.median(t_clear))
    print(f"{V} views of {H} x {W}, voxel {VOXEL}: {nb} blocks ({pts} lattice points, volume {vol.nbytes() / 1e6:.1f} MB), {vol.n_observed} observed pixels, "
          f"{vol.n_dropped} dropped; mesh {len(m.vertices)} vertices, {len(m.triangles)} triangles", flush=True)
    print(line("blocks", t_blocks)); print(line("clear", t_clear)); print(line("clear+integ", t_int)); print(line("mesh", t_mesh))
    print(line("torch integ", t_torch)); print(line("hip (altern.)", t_hip))
    print(f"    torch / hip {float(np.median(t_torch)) / float(np.median(t_hip)):7.1f}; tsdf and weight {'identical' if same else 'DIFFER'}")
    print(f"    integrate alone {k_ms:.3f} ms: {pts * V / 1e6:.0f} M (point, view) pairs, {front / 1e6:.0f} M in front, {inside / 1e6:.0f} M on an image, "
          f"{fused / 1e6:.0f} M fused; {flop / 1e9:.2f} G float64 operations = {flop / k_ms / 1e9:.2f} TFLOP/s, {byts / 1e6:.0f} MB = {byts / k_ms / 1e9:.3f} TB/s", flush=True)
    del v, vol, m, ref
    torch.cuda.empty_cache()
