"""sta_mesh_triangles, sta_mesh_vertex_normals and a whole render_mesh frame on one GPU.

    python tools/mesh_bench.py [runs] [--threshold]          # default 20 runs per configuration; medians between device events

Scene: the mesh of tools/tsdf_bench.py's procedural 16 x 12 x 4 m room fused from 40 views of 224 x 224 at voxel_size 0.05 (about 1 M
vertices and 2 M triangles); canvases 720 x 480 and 1920 x 1080, ssaa 1 and 2; a top-down camera above the room with the back faces
culled (it looks in through the ceiling) and a follow camera inside it.  Per configuration: clear + sta_mesh_triangles per payload kind,
the share of the drawn pieces that take the large path, the fragments and the atomics the early-out load lets through (a measurement build of the
same translation unit with MS_COUNT_ATOMICS, built into tools/probes/bin/, never shipped), and sta_raster_points on the same vertices as
the yardstick.  --threshold: the table of the small / large threshold (measurement builds with -DMS_SMALL_MAX=n)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
from vista_slam_amd import _lib, build, render, tsdf      # noqa: E402

runs = next((int(v) for v in sys.argv[1:] if v.isdigit()), 20)
BIN = os.path.join(ROOT, "tools", "probes", "bin")
VOXEL, H0, W0 = 0.05, 224, 224
SIZE = (16.0, 12.0, 4.0)
dev = torch.device("cuda:0")


def variant(name, flags):
    """libsta_mesh.so with measurement macros, built once per source content"""
    os.makedirs(BIN, exist_ok=True)
    out, tag = os.path.join(BIN, f"libsta_mesh_{name}.so"), build.source_hash(build.MESH_DEPS) + " ".join(flags)
    if not (os.path.exists(out) and os.path.exists(out + ".srchash") and open(out + ".srchash").read() == tag):
        cmd = [build.hipcc_path()] + build.BASE_FLAGS + flags + ["-o", out, os.path.join(build.CSRC, "sta_mesh.hip")]
        print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=build.CSRC)
        with open(out + ".srchash", "w") as f:
            f.write(tag)
    lib = C.CDLL(out)
    for fn, (res, args) in _lib.MESH_SIGNATURES.items():
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = res, args
    return lib


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


def events(fn, n=None):
    out = []
    for _ in range(runs if n is None else n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def check(lib, rc):
    if rc != 0:
        raise RuntimeError(lib.sta_mesh_last_error().decode())


def tri_call(lib, cv, cam, mesh, work, kind, cull, counters=None, lit=True):
    T, K, near, far = cam._args()
    eye = -np.linalg.solve(cam.w2c[:, :3], cam.w2c[:, 3])
    light = (C.c_double * 4)(*eye.tolist(), 0.3) if kind == 1 and lit else None
    col = mesh.colors.data_ptr() if kind == 1 else None

    def call():
        cv.clear()
        check(lib, lib.sta_mesh_triangles(cv.keys.data_ptr(), cv.H, cv.W, cv.ssaa, mesh.vertices.data_ptr(), len(mesh.vertices), mesh.triangles.data_ptr(),
                                          len(mesh.triangles), col, None, light, kind, cull, 0, T, K, near, far, counters.data_ptr() if counters is not None else None,
                                          work.data_ptr(), work.numel(), cv._stream()))
    return call


def points_call(cv, cam, mesh):
    """clear + sta_raster_points on the mesh's vertices with their float32 colours, through the C ABI like the triangle calls"""
    rl = _lib.load_raster()
    T, K, near, far = cam._args()

    def call():
        cv.clear()
        _lib.check_raster(rl.sta_raster_points(cv.keys.data_ptr(), cv.H, cv.W, cv.ssaa, mesh.vertices.data_ptr(), mesh.colors.data_ptr(), 2, 0, len(mesh.vertices),
                                               T, K, near, far, 1, None, cv._stream()))
    return call


print(f"{torch.cuda.get_device_name(0)}; medians of {runs} runs between device events", flush=True)
v, poses = room_views(40, 2740)
vol = tsdf.TSDFVolume(dev, VOXEL).allocate(v).integrate(v)
mesh = vol.mesh()
nv, nt = len(mesh.vertices), len(mesh.triangles)
print(f"the room of tools/tsdf_bench.py, 40 views of {H0} x {W0}, voxel {VOXEL}: {nv} vertices, {nt} triangles", flush=True)
prod = _lib.load_mesh()
count = variant("count", ["-DMS_COUNT_ATOMICS"])
sizes = (C.c_int64 * 2)()
check(prod, prod.sta_mesh_plan(nt, nv, sizes))
work = torch.empty(int(sizes[0]), dtype=torch.uint8, device=dev)
pose = poses[5].double().numpy()


def cameras(H, Wd):
    top = render.Camera.look_at([8.0, 6.0, 16.0], [8.0, 6.0, 0.0], [0.0, 1.0, 0.0], 0.75 * H, 0.75 * H, H, Wd, near=0.05, far=100.0)
    K_out = [0.5 * min(H, Wd) / np.tan(np.deg2rad(30.0))] * 2 + [(Wd - 1) / 2.0, (H - 1) / 2.0]
    off = render.follow_offset()
    off[:3, 3] = [0, 0.3, 2.0]                              # 2 m behind the view (5 m would be outside the room)
    follow = render.Camera.from_pose(pose, K_out, off, near=0.05, far=100.0)
    return (("topdown", top, 1), ("follow", follow, 0))


print(f"{'canvas':>10s} ssaa camera   |   id ms  color ms  shaded ms  normal ms | points ms (the {nv} vertices) | large of drawn pieces share | fragments   atomics issued  skipped | clear ms")
for (Wd, H) in ((720, 480), (1920, 1080)):
    for s in (1, 2):
        cv = render.Canvas(dev, H, Wd, s)
        for name, cam, cull in cameras(H, Wd):
            t = {}
            for label, kind, lit in (("id", 0, False), ("color", 1, False), ("shaded", 1, True), ("normal", 2, False)):
                f = tri_call(prod, cv, cam, mesh, work, kind, cull, lit=lit)
                f()
                t[label] = events(f)
            large = int(work[:4].view(torch.int32).item())            # the list's counter after the last call (a readback of the tool, not of the library)
            cnt = torch.zeros(11, dtype=torch.int64, device=dev)
            tri_call(count, cv, cam, mesh, work, 1, cull, cnt)()
            c = cnt.cpu().tolist()
            drawn = c[10]                                             # the pieces that reach the draw, counted by the measurement build
            f = points_call(cv, cam, mesh)
            f()
            t_pts = events(f)
            clear = events(cv.clear)
            print(f"{Wd:5d}x{H:<4d} {s:4d} {name:8s} | {t['id']:7.3f} {t['color']:9.3f} {t['shaded']:10.3f} {t['normal']:10.3f} | {t_pts:9.3f} | "
                  f"{large:8d} of {drawn:8d} {100.0 * large / max(drawn, 1):6.2f}% | {c[8]:9d} {c[9]:16d} {100.0 * (1 - c[9] / max(c[8], 1)):7.2f}% | {clear:.3f}"
                  f"   counters {c[:8]}", flush=True)
        del cv

if "--threshold" in sys.argv:
    print("the small / large threshold (MS_SMALL_MAX, pixels of the clamped box a setup lane draws itself): clear + shaded triangles, ms")
    rows, ref, equal = {}, {}, True
    for n in (64, 0, 16, 256, 1024, 1 << 30):
        lib = prod if n == 64 else variant(f"small{n}", [f"-DMS_SMALL_MAX={n}"])
        for (Wd, H, s) in ((720, 480, 1), (1920, 1080, 2)):
            cv = render.Canvas(dev, H, Wd, s)
            for name, cam, cull in cameras(H, Wd):
                f = tri_call(lib, cv, cam, mesh, work, 1, cull)
                f()
                rows.setdefault(n, []).append((f"{Wd}x{H} ssaa {s} {name}", events(f)))
                if n == 64:
                    ref[(Wd, s, name)] = cv.keys.clone()
                else:
                    equal = equal and torch.equal(ref[(Wd, s, name)], cv.keys)            # the threshold is no part of the contract: the same keys
            del cv
    rows = {n: rows[n] for n in (0, 16, 64, 256, 1024, 1 << 30)}
    heads = [k for k, _ in rows[64]]
    print(f"{'MS_SMALL_MAX':>12s} | " + " | ".join(f"{h:>24s}" for h in heads))
    for n, r in rows.items():
        print(f"{('all large' if n == 0 else 'all small' if n == 1 << 30 else str(n)):>12s} | " + " | ".join(f"{ms:24.3f}" for _, ms in r), flush=True)
    print(f"the keys of every threshold {'equal' if equal else 'DIFFER from'} the product's (64)", flush=True)

# vertex normals against sta_tsdf_mesh of the same volume
tsdf.vertex_normals(mesh)
t_n = events(lambda: tsdf.vertex_normals(mesh))
t_m = events(lambda: vol.mesh())
print(f"sta_mesh_vertex_normals ({nv} vertices, {3 * nt} pairs, {2 if nv < 65536 else 4} sort passes; with its workspace allocation): {t_n:.3f} ms; "
      f"sta_tsdf_mesh of the same volume (two calls: count, then emit): {t_m:.3f} ms", flush=True)

# a whole render_mesh frame with its PNG: host wall-clock
with tempfile.TemporaryDirectory() as tmp:
    for (Wd, H, s) in ((720, 480, 1), (720, 480, 2), (1920, 1080, 2)):
        name, cam, cull = cameras(H, Wd)[1]
        cvs = render.Canvas(dev, H, Wd, s)
        frame = lambda: render.write_png(os.path.join(tmp, "f.png"), render.render_mesh(dev, cam, mesh, H=H, W=Wd, ssaa=s, poses=poses.numpy(), canvas=cvs))
        image = lambda: render.render_mesh(dev, cam, mesh, H=H, W=Wd, ssaa=s, poses=poses.numpy(), canvas=cvs).cpu()
        out = []
        for fn in (frame, image):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            out.append((time.perf_counter() - t0) * 1e3 / 5)
        print(f"render_mesh (shaded, trajectory) + write_png, {Wd}x{H} at ssaa {s}, follow camera: {out[0]:.2f} ms per frame, host wall-clock "
              f"({os.path.getsize(os.path.join(tmp, 'f.png')) / 1024:.0f} KiB), of which {out[1]:.2f} ms up to the image on the host (the rest is zlib)", flush=True)
