"""libsta_ray.so on one GPU: depth maps by rays next to the rasteriser's, occlusion of random segments, first hits with rays that point
away, and the same answer from a chunked float64 torch brute force.

    python tools/ray_bench.py [runs]      # default 20 runs per measurement; medians between device events

Scene: the mesh of tools/tsdf_bench.py's procedural 16 x 12 x 4 m room fused from 40 views of 224 x 224 at voxel_size 0.05 (about 1 M
vertices and 2 M triangles), and the top-down and follow cameras of tools/mesh_bench.py.  Per camera and canvas: TriIndex.cast of the
pixel rays (already on the device; t only), meshdist.ray_depth as a whole (host rays, upload, cast), render.mesh_depth as a whole, the
share of pixels where both name the same triangle and the largest relative depth difference among those - reported, not asserted: the
rasteriser snaps vertices to 1/256 pixel.  The torch brute force evaluates the header's rules 2 to 5 for every (ray, triangle) pair in
float64, 32 rays at a time, on the first 200 000 triangles and 20 000 rays; every t and tri must be equal.  The traversal variant
(children in the order of the ray's signs, -DRY_SIGN_ORDER=1) is built next to the library into tools/probes/bin and timed alternating
with it on the same rays, its outputs compared bit for bit; `--build-only` builds it and stops (no GPU)."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                              # noqa: E402
import torch                                                                    # noqa: E402
from vista_slam_amd import _lib, build, meshdist, render, surface, tsdf        # noqa: E402

runs = next((int(v) for v in sys.argv[1:] if v.isdigit()), 20)
VOXEL, H0, W0 = 0.05, 224, 224
SIZE = (16.0, 12.0, 4.0)
dev = torch.device("cuda:0")
INF = float("inf")
BIN = os.path.join(ROOT, "tools", "probes", "bin")


def variant(name, flags):
    """libsta_ray.so with a traversal macro, built once per source content"""
    os.makedirs(BIN, exist_ok=True)
    out, tag = os.path.join(BIN, f"libsta_ray_{name}.so"), build.source_hash(build.RAY_DEPS) + " ".join(flags)
    if not (os.path.exists(out) and os.path.exists(out + ".srchash") and open(out + ".srchash").read() == tag):
        cmd = [build.hipcc_path()] + build.BASE_FLAGS + flags + ["-o", out, os.path.join(build.CSRC, "sta_ray.hip")]
        print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=build.CSRC)
        with open(out + ".srchash", "w") as f:
            f.write(tag)
    lib = C.CDLL(out)
    for fn, (res, args) in _lib.RAY_SIGNATURES.items():
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = res, args
    return lib


sign_lib = variant("sign", ["-DRY_SIGN_ORDER=1"])
if "--build-only" in sys.argv:
    sys.exit(0)


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


def median_ms(fn, n=None):
    fn()
    return float(np.median([once(fn) for _ in range(runs if n is None else n)]))


def cameras(H, Wd, pose):
    """tools/mesh_bench.py's: looking in through the ceiling, and 2 m behind a view inside the room"""
    top = render.Camera.look_at([8.0, 6.0, 16.0], [8.0, 6.0, 0.0], [0.0, 1.0, 0.0], 0.75 * H, 0.75 * H, H, Wd, near=0.05, far=100.0)
    K_out = [0.5 * min(H, Wd) / np.tan(np.deg2rad(30.0))] * 2 + [(Wd - 1) / 2.0, (H - 1) / 2.0]
    off = render.follow_offset()
    off[:3, 3] = [0, 0.3, 2.0]
    return (("topdown", top), ("follow", render.Camera.from_pose(pose, K_out, off, near=0.05, far=100.0)))


def torch_brute(tri9, src, n_valid, o, d, t_min, t_max, chunk=32):
    """rules 2 to 5 of include/sta_ray.h for every pair, one torch float64 operation per written step -> (t [R] f64, tri [R] i32)"""
    P = tri9[:n_valid].view(-1, 3, 3)
    lo32, hi32 = P.min(dim=1).values, P.max(dim=1).values
    ninf, pinf = torch.tensor(-INF, device=dev), torch.tensor(INF, device=dev)
    lo, hi = torch.nextafter(lo32, ninf).double()[None], torch.nextafter(hi32, pinf).double()[None]          # [1,T,3]
    A, B, Cc = P[None, :, 0].double(), P[None, :, 1].double(), P[None, :, 2].double()
    ids = src[:n_valid].long()[None]
    big = torch.full((), 1 << 40, device=dev)
    to, trio = torch.empty(len(o), dtype=torch.float64, device=dev), torch.empty(len(o), dtype=torch.int64, device=dev)
    for s in range(0, len(o), chunk):
        oo, dd = o[s:s + chunk].double()[:, None, :], d[s:s + chunk].double()[:, None, :]          # [r,1,3]
        enter = torch.full((oo.shape[0], P.shape[0]), float(t_min), dtype=torch.float64, device=dev)
        exit_ = torch.full_like(enter, float(t_max))
        ok = torch.ones_like(enter, dtype=torch.bool)
        for k in range(3):
            dk, ok_ = dd[..., k], oo[..., k]
            nz, inv = dk != 0, 1.0 / dk
            near, far = torch.where(dk > 0, lo[..., k], hi[..., k]), torch.where(dk > 0, hi[..., k], lo[..., k])
            tn, tf = (near - ok_) * inv, (far - ok_) * inv
            enter = torch.where(nz & (tn > enter), tn, enter)
            exit_ = torch.where(nz & (tf < exit_), tf, exit_)
            ok = ok & (nz | ((lo[..., k] <= ok_) & (ok_ <= hi[..., k])))
        ok = ok & (enter <= exit_)
        kz = d[s:s + chunk].abs().argmax(dim=1)          # the first maximum
        pick = lambda x, k: torch.gather(x.expand(len(kz), -1, 3), 2, k[:, None, None].expand(-1, x.shape[1], 1))[..., 0]
        dz = pick(dd, kz)
        Sx, Sy, Sz = pick(dd, (kz + 1) % 3) / dz, pick(dd, (kz + 2) % 3) / dz, 1.0 / dz

        def sheared(V):
            q = V - oo
            c = pick(q, kz)
            return pick(q, (kz + 1) % 3) - Sx * c, pick(q, (kz + 2) % 3) - Sy * c, Sz * c
        Ax, Ay, Az = sheared(A)
        Bx, By, Bz = sheared(B)
        Cx, Cy, Cz = sheared(Cc)
        U, V_, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        det = (U + V_) + W
        t = ((U * Az + V_ * Bz) + W * Cz) / det
        q = ok & (((U >= 0) & (V_ >= 0) & (W >= 0)) | ((U <= 0) & (V_ <= 0) & (W <= 0))) & (det != 0) & (t >= t_min) & (t <= t_max)
        tc = torch.where(t >= enter, t, enter)
        tc = torch.where(tc <= exit_, tc, exit_)
        key = torch.where(q, tc, torch.full_like(tc, INF))
        m = key.min(dim=1).values
        best = torch.where(q & (tc == m[:, None]), ids, big).min(dim=1).values
        hit = q.any(dim=1)
        to[s:s + chunk] = torch.where(hit, m, torch.full_like(m, INF))
        trio[s:s + chunk] = torch.where(hit, best, torch.full_like(best, -1))
    return to, trio.to(torch.int32)


def cast_through(lib, index, o, d, t_min, t_max, out):
    """sta_ray_cast of `lib` on the index's buffers into out = (t, tri, bary); o and d are [R,3] float32 rows, as meshdist._rays makes them"""
    assert o.shape == d.shape == (len(d), 3) and o.dtype == d.dtype == torch.float32 and o.is_contiguous() and d.is_contiguous() and o.is_cuda and d.is_cuda
    assert all(x.is_contiguous() and len(x) == len(d) for x in out)
    rc = lib.sta_ray_cast(index.tri.data_ptr(), index.src.data_ptr(), index.boxes.data_ptr(), index.counters.data_ptr(), index.nt, o.data_ptr(), d.data_ptr(), len(d),
                          float(t_min), float(t_max), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), index.ray_status.data_ptr(),
                          torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.sta_ray_last_error()


def order_ab(what, index, o, d, t_min, t_max):
    """index order (the library) against sign order (the variant), alternating, on the same rays and output buffers of their own"""
    prod = _lib.load_ray()
    o, d = meshdist._rays(o, d, dev)          # a single origin [3] becomes one row per ray: the C entry point reads org[3 i .. 3 i + 2]
    n = len(d)
    outs = [(torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, 3, device=dev)) for _ in range(2)]
    ms = ([], [])
    for k in range(runs + 1):
        for which, lib in enumerate((prod, sign_lib)):
            t_ms = once(lambda: cast_through(lib, index, o, d, t_min, t_max, outs[which]))
            if k:
                ms[which].append(t_ms)
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*outs))
    print(f"    children in index order {float(np.median(ms[0])):.3f} ms, in the order of the ray's signs {float(np.median(ms[1])):.3f} ms ({what}; alternating, "
          f"medians of {runs}; outputs {'bit-identical' if same else 'DIFFER'})", flush=True)


print(f"{torch.cuda.get_device_name(0)}; medians of {runs} runs between device events", flush=True)
views, poses = room_views(40, 2740)
mesh = tsdf.TSDFVolume(dev, VOXEL).allocate(views).integrate(views).mesh()
nv, nt = len(mesh.vertices), len(mesh.triangles)
idx = meshdist.TriIndex.build(mesh)
print(f"the room of tools/tsdf_bench.py, 40 views of {H0} x {W0}, voxel {VOXEL}: {nv} vertices, {nt} triangles; fan-out {meshdist.FANOUT}, {idx.levels} levels, "
      f"{meshdist.ray_plan(nt)} nodes; counters {idx.counters.tolist()}", flush=True)

pose = poses[5].double().numpy()
for (Wd, H) in ((720, 480), (1920, 1080)):
    for name, cam in cameras(H, Wd, pose):
        o, d = [a.to(dev) for a in meshdist.camera_rays(cam, H, Wd)]
        cast_ms = median_ms(lambda: idx.cast(o, d, cam.near, cam.far, want=("t",)))
        all_ms = median_ms(lambda: idx.cast(o, d, cam.near, cam.far))
        whole_ms = median_ms(lambda: meshdist.ray_depth(idx, cam, H, Wd), 5)
        raster_ms = median_ms(lambda: render.mesh_depth(dev, mesh, cam, H, Wd))
        t, tri = idx.cast(o, d, cam.near, cam.far, want=("t", "tri"))
        cv = render.Canvas(dev, H, Wd, 1).mesh(cam, mesh, mode="id")
        rd, rid = cv.depth().reshape(-1), cv.ids().reshape(-1)
        both = (tri >= 0) & (rid >= 0)
        same = both & (tri == rid)
        rel = ((t.float() - rd).abs() / rd)[same]
        print(f"{Wd}x{H} {name}: cast of {H * Wd} pixel rays, t only {cast_ms:.3f} ms, t + tri + bary {all_ms:.3f} ms; ray_depth as a whole (host rays, upload) "
              f"{whole_ms:.2f} ms; render.mesh_depth as a whole {raster_ms:.3f} ms; hit by rays {int((tri >= 0).sum())}, by the rasteriser {int((rid >= 0).sum())}, "
              f"by both {int(both.sum())}, the same triangle on {int(same.sum())} ({100.0 * int(same.sum()) / max(int(both.sum()), 1):.2f} % of both), largest "
              f"relative depth difference among those {float(rel.max()) if len(rel) else float('nan'):.3e}; status {int(idx.ray_status)}", flush=True)
        order_ab(f"the {H * Wd} pixel rays", idx, o, d, cam.near, cam.far)

# segments between surface samples; rays from surface samples, 5 % pointing away from the room
n = 2_000_000
a = surface.sample_surface(mesh, n, seed=1).points
b = surface.sample_surface(mesh, n, seed=2).points
seg = (b - a).contiguous()
ms = median_ms(lambda: idx.occluded(a, seg, 1e-6, 1.0 - 1e-6))
occ = idx.occluded(a, seg, 1e-6, 1.0 - 1e-6)
print(f"occluded for {n} segments between surface samples, t in [1e-6, 1 - 1e-6]: {ms:.3f} ms ({int(occ.sum())} occluded); status {int(idx.ray_status)}", flush=True)
ms = median_ms(lambda: idx.cast(a, seg, 1e-6, 1.0 - 1e-6))
print(f"    cast of the same segments (first hit, t + tri + bary): {ms:.3f} ms", flush=True)
centre = torch.tensor([8.0, 6.0, 2.0], device=dev)
g = torch.Generator(device="cuda").manual_seed(7)
org = (centre + (torch.rand(n, 3, device=dev, generator=g) - 0.5) * torch.tensor([12.0, 8.0, 2.0], device=dev)).contiguous()
dirs = torch.randn(n, 3, device=dev, generator=g)
org[::20] = centre + torch.tensor([0.0, 0.0, 30.0], device=dev)          # 5 %: above the room, pointing up and away
dirs[::20, 2] = dirs[::20, 2].abs() + 0.1
ms = median_ms(lambda: idx.cast(org, dirs))
tri = idx.cast(org, dirs, want=("tri",))[0]
print(f"cast of {n} random rays from inside the room, t_max = +inf, 5 % of them outside and pointing away: {ms:.3f} ms ({int((tri >= 0).sum())} hit); "
      f"status {int(idx.ray_status)}", flush=True)
ms = median_ms(lambda: idx.cast(org, dirs, want=("t",)))
print(f"    the same, t only: {ms:.3f} ms", flush=True)
order_ab("the same 2 M rays", idx, org, dirs, 0.0, INF)
order_ab("the 2 M segments", idx, a, seg, 1e-6, 1.0 - 1e-6)

# the brute force, on a size torch can hold
sub = tsdf.Mesh(mesh.vertices, None, mesh.triangles[:200_000].contiguous())
sub_idx = meshdist.TriIndex.build(sub)
ro, rd_ = org[:20_000].contiguous(), dirs[:20_000].contiguous()
n_valid = int(sub_idx.counters[0])
t_nat, t_torch = [], []
for _ in range(3):                                  # alternating; three runs: the brute force takes seconds
    t_nat.append(once(lambda: meshdist.TriIndex.build(sub).cast(ro, rd_)))
    t_torch.append(once(lambda: torch_brute(sub_idx.tri, sub_idx.src, n_valid, ro, rd_, 0.0, INF)))
tn, trin, _b = sub_idx.cast(ro, rd_)
tt, trit = torch_brute(sub_idx.tri, sub_idx.src, n_valid, ro, rd_, 0.0, INF)
print(f"20 000 rays against the first 200 000 triangles, t_max +inf: build + cast {float(np.median(t_nat)):.3f} ms, torch float64 brute force in chunks of 32 rays "
      f"{float(np.median(t_torch)):.1f} ms (3 runs each, alternating); {int((trin >= 0).sum())} hit; tri {'all equal' if torch.equal(trin, trit) else 'DIFFER: ' + str(int((trin != trit).sum()))}, "
      f"t {'all equal' if torch.equal(tn, tt) else 'differ in ' + str(int((tn != tt).sum()))}", flush=True)
