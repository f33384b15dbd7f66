"""sta_raster_points, sta_raster_resolve and a whole render_folder frame on one GPU, against the torch composition that yields the same
image on the same GPU, in the same process, alternating: float64 projection, int64 keys, scatter_reduce_(amin) per footprint pixel, decode.

    python tools/render_bench.py [runs]           # default 20 runs per configuration and side; medians between device events

Scene: 2 M and 20 M points (40 and 400 views of 224 x 224) on the walls of the procedural 16 x 12 x 4 m room of tools/voxel_bench.py, seen
from a corner at eye height; canvases 720 x 480 and 1920 x 1080, ssaa 1 and 2, point_size 1 and 3.  The keys of both sides must be equal.

Three measurement builds of the same translation unit (csrc/raster.h: RS_NO_EARLY_OUT, RS_NO_WRITE, RS_COUNT_ATOMICS; built into
tools/probes/bin/, never shipped) separate what the pass costs: every atomic issued, no key traffic at all, and the count of footprint
pixels and of the atomics the early-out load lets through."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
from vista_slam_amd import _lib, build, formats, render, weights as W           # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

runs = next((int(v) for v in sys.argv[1:] if v.isdigit()), 20)
BIN = os.path.join(ROOT, "tools", "probes", "bin")
VARIANTS = {"noearly": "-DRS_NO_EARLY_OUT", "nowrite": "-DRS_NO_WRITE", "count": "-DRS_COUNT_ATOMICS"}


def variant(name):
    """libsta_raster.so with one measurement macro, built once per source content"""
    os.makedirs(BIN, exist_ok=True)
    out, tag = os.path.join(BIN, f"libsta_raster_{name}.so"), build.source_hash(build.RASTER_DEPS) + VARIANTS[name]
    if not (os.path.exists(out) and os.path.exists(out + ".srchash") and open(out + ".srchash").read() == tag):
        cmd = [build.hipcc_path()] + build.BASE_FLAGS + [VARIANTS[name], "-o", out, os.path.join(build.CSRC, "sta_raster.hip")]
        print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=build.CSRC)
        with open(out + ".srchash", "w") as f:
            f.write(tag)
    lib = C.CDLL(out)
    for fn, (res, args) in _lib.RASTER_SIGNATURES.items():
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = res, args
    return lib


def room(M, seed):
    """tools/voxel_bench.py's: M points on the six faces of a 16 x 12 x 4 m box with 1 cm of normal noise; colours uniform (uint8 here)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    size = torch.tensor([16.0, 12.0, 4.0], device="cuda")
    p = torch.rand(M, 3, device="cuda", generator=g) * size
    face = torch.randint(0, 6, (M,), device="cuda", generator=g)
    axis, side = face // 2, (face % 2).float()
    p.scatter_(1, axis[:, None], (side * size[axis])[:, None])
    p += 0.01 * torch.randn(M, 3, device="cuda", generator=g)
    return p.contiguous(), torch.randint(0, 256, (M, 3), device="cuda", generator=g, dtype=torch.uint8)


def torch_points(pts, col, cam, Hs, Ws, s, p):
    """the keys of sta_raster_points as int64, empty = -1"""
    T, K = torch.from_numpy(cam.w2c).cuda(), cam.K
    x, y, z = pts.double().unbind(1)
    pc = [((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)]
    ok = torch.isfinite(pc[0]) & torch.isfinite(pc[1]) & torch.isfinite(pc[2]) & (pc[2] >= cam.near) & (pc[2] <= cam.far)
    us = (K[0] * (pc[0] / pc[2]) + K[2]) * float(s) + (s - 1) * 0.5
    vs = (K[1] * (pc[1] / pc[2]) + K[3]) * float(s) + (s - 1) * 0.5
    fx, fy = torch.floor(us + 0.5), torch.floor(vs + 0.5)
    lo, hi = (p - 1) // 2, p // 2
    ok &= (fx + hi >= 0) & (fx - lo <= Ws - 1) & (fy + hi >= 0) & (fy - lo <= Hs - 1)
    c = col.long()
    key = (pc[2].float().view(torch.int32).long() << 32) | (c[:, 0] << 24) | (c[:, 1] << 16) | (c[:, 2] << 8) | 255
    ix, iy, key = fx[ok].long(), fy[ok].long(), key[ok]
    big = torch.iinfo(torch.int64).max
    keys = torch.full((Hs * Ws,), big, dtype=torch.int64, device="cuda")
    for dy in range(-lo, hi + 1):
        for dx in range(-lo, hi + 1):
            xx, yy = ix + dx, iy + dy
            on = (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
            keys.scatter_reduce_(0, (yy[on] * Ws + xx[on]), key[on], "amin")
    return torch.where(keys == big, torch.full_like(keys, -1), keys).view(Hs, Ws)


def torch_resolve(keys, s, bg):
    Hs, Ws = keys.shape
    H, Wd = Hs // s, Ws // s
    b = keys.view(H, s, Wd, s).permute(0, 2, 1, 3).reshape(H, Wd, s * s)
    empty = b == -1
    chans = [(b >> 24) & 255, (b >> 16) & 255, (b >> 8) & 255, (b & 255) if s == 1 else torch.full_like(b, 255)]
    rgba = torch.stack([(torch.where(empty, torch.full_like(b, bg[c]), chans[c]).sum(dim=2) + s * s // 2) // (s * s) for c in range(4)], dim=-1).to(torch.uint8)
    best = torch.where(empty, torch.full_like(b, torch.iinfo(torch.int64).max), b).amin(dim=2)
    depth = torch.where(empty.all(dim=2), torch.full((H, Wd), float("inf"), device="cuda"), (best >> 32).to(torch.int32).view(torch.float32))
    return rgba, depth


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def alternate(ours, ref):
    for f in (ours, ref):
        f()
    t = {"hip": [], "torch": []}
    a = b = None
    for _ in range(runs):
        ms, a = device_ms(ours); t["hip"].append(ms)
        ms, b = device_ms(ref); t["torch"].append(ms)
    return float(np.median(t["hip"])), float(np.median(t["torch"])), a, b


def points_call(lib, cv, cam, pts, col, p, counters=None):
    T, K, near, far = cam._args()
    def call():
        _lib_check(lib, lib.sta_raster_clear(cv.keys.data_ptr(), cv.H, cv.W, cv.ssaa, cv._stream()))
        _lib_check(lib, lib.sta_raster_points(cv.keys.data_ptr(), cv.H, cv.W, cv.ssaa, pts.data_ptr(), col.data_ptr(), 1, 0, len(pts), T, K, near, far, p,
                                              counters.data_ptr() if counters is not None else None, cv._stream()))
        return cv.keys
    return call


def _lib_check(lib, rc):
    if rc != 0:
        raise RuntimeError(lib.sta_raster_last_error().decode())


print(f"{torch.cuda.get_device_name(0)}; medians of {runs} runs between device events, alternating with the torch composition; clear + points per run")
prod = _lib.load_raster()
libs = {k: variant(k) for k in VARIANTS}
bg = (255, 255, 255, 255)
print(f"{'points':>9s} {'canvas':>10s} ssaa size |   hip ms  torch ms  torch/hip | every atomic  no key traffic | fragments   atomics issued  skipped | "
      f"Gfrag/s  Gatomic/s (every atomic)  GB/s of 15 B/point")
for M in (2_000_000, 20_000_000):
    pts, col = room(M, 2600 + M // 1_000_000)
    for (Wd, H) in ((720, 480), (1920, 1080)):
        cam = render.Camera.look_at([0.5, 0.5, 1.6], [12.0, 9.0, 1.8], [0.0, 0.0, 1.0], 0.6 * Wd, 0.6 * Wd, H, Wd, near=0.05, far=100.0)
        for s in (1, 2):
            cv = render.Canvas("cuda:0", H, Wd, s)
            for p in (1, 3):
                hip, tor, a, b = alternate(points_call(prod, cv, cam, pts, col, p), lambda: torch_points(pts, col, cam, H * s, Wd * s, s, p))
                same = torch.equal(a, b)
                every = float(np.median([device_ms(points_call(libs["noearly"], cv, cam, pts, col, p))[0] for _ in range(runs)]))
                nokey = float(np.median([device_ms(points_call(libs["nowrite"], cv, cam, pts, col, p))[0] for _ in range(runs)]))
                cnt = torch.zeros(6, dtype=torch.int64, device="cuda")
                points_call(libs["count"], cv, cam, pts, col, p, cnt)()
                frag, issued = cnt[4].item(), cnt[5].item()
                clear = float(np.median([device_ms(cv.clear)[0] for _ in range(runs)]))
                print(f"{M:9d} {Wd:5d}x{H:<4d} {s:4d} {p:4d} | {hip:8.3f} {tor:9.2f} {tor / hip:10.1f} | {every:12.3f} {nokey:14.3f} | {frag:9d} {issued:16d} "
                      f"{100.0 * (1 - issued / max(frag, 1)):7.2f}% | {frag / (hip - clear) / 1e6:7.2f} {frag / (every - clear) / 1e6:10.2f} "
                      f"{15.0 * M / (hip - clear) / 1e6:18.1f}   keys {'equal' if same else 'DIFFER'} (clear alone {clear:.3f} ms)", flush=True)
            # resolve of the last image
            rgba = torch.empty(H, Wd, 4, dtype=torch.uint8, device="cuda")
            depth = torch.empty(H, Wd, dtype=torch.float32, device="cuda")
            hip, tor, _a, (trgba, tdepth) = alternate(lambda: cv._resolve(bg, rgba=rgba, depth=depth), lambda: torch_resolve(cv.keys, s, bg))
            print(f"{'resolve':>9s} {Wd:5d}x{H:<4d} {s:4d}      | {hip:8.3f} {tor:9.2f} {tor / hip:10.1f} | rgba and depth "
                  f"{'equal' if torch.equal(rgba, trgba) and torch.equal(depth, tdepth) else 'DIFFER'}", flush=True)
            del cv
    del pts, col
    torch.cuda.empty_cache()

# a whole render_folder frame: 6 views of 224 x 224 in a saved folder, 720 x 480 output, host wall-clock per frame (cloud, lines, resolve, PNG)
import render_cases as RC                                  # noqa: E402
m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
run = RC.room_run(N=6, H=224, W=224)
with tempfile.TemporaryDirectory() as tmp:
    formats.save_data_all(m, tmp, poses=run["poses"], scales=run["scales"], depths=run["depths"], confs=run["confs"], intrinsics=run["intrinsics"],
                          imgs=torch.from_numpy(run["imgs"]), conf_thres=0.0, view_graph={i: [j for j in (i - 1, i + 1) if 0 <= j < 6] for i in range(6)},
                          loop_min_dist=4, view_names=[str(i) for i in range(6)], save_ply=False)
    for s in (1, 2):
        render.render_folder(m, tmp, os.path.join(tmp, "warm"), H=480, W=720, ssaa=s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths = render.render_folder(m, tmp, os.path.join(tmp, f"out{s}"), H=480, W=720, ssaa=s)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        size = sum(os.path.getsize(p) for p in paths) / len(paths)
        print(f"render_folder, 6 views of 224x224 (up to {6 * 224 * 224} points), 720x480 at ssaa {s}: {ms / len(paths):.2f} ms per frame, host wall-clock with the PNG "
              f"({size / 1024:.0f} KiB per file)", flush=True)
