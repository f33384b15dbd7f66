"""libsta_knn.so on one GPU (vista_slam_amd.cloud: NNIndex.knn, knn_moments, estimate_normals, remove_statistical_outlier): medians of
`runs` calls between device events, on the procedural room of tools/voxel_bench.py (16 x 12 x 4 m, 1 cm of noise).

    python tools/knn_bench.py [runs] [small]      # default 20 runs; `small` leaves the 2 M cloud out

  1. knn of the cloud against itself (self excluded) at radius 0.1, cell = radius / 2: k = 8 / 16 / 30 / 64 for 200 000 and 2 M points,
     with `order` = the grid's sorted_idx and without;
  2. the three cell choices radius, radius / 2 and radius / 4 at k = 16 and 30 (the default of the wrappers, KNN_CELL_FRACTION, changes
     only on this evidence);
  3. knn_moments on the lists of k = 16 and 30 (normal, curvature, mean distance and record in one pass);
  4. a whole estimate_normals(k = 30) and a whole remove_statistical_outlier(nb 20), index build and readback included (host wall-clock
     around a synchronised call: what a caller waits for);
  5. the torch composition for the same lists - chunked float64 cdist-by-hand (the library's own d2 formula) and topk over
     (d2, index) - at 100 000 x 100 000, k = 16, alternating with the library call, with every index compared.
Reported, not asserted."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
from vista_slam_amd import cloud                           # noqa: E402

nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
RUNS = nums[0] if nums else 20
SMALL = "small" in sys.argv[1:]
RADIUS = 0.1


def room(M, seed):
    """M points on the six faces of a 16 x 12 x 4 m box, uniform per face with 1 cm of normal noise (tools/voxel_bench.py)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    size = torch.tensor([16.0, 12.0, 4.0], device="cuda")
    p = torch.rand(M, 3, device="cuda", generator=g) * size
    face = torch.randint(0, 6, (M,), device="cuda", generator=g)
    axis, side = face // 2, (face % 2).float()
    p.scatter_(1, axis[:, None], (side * size[axis])[:, None])
    p += 0.01 * torch.randn(M, 3, device="cuda", generator=g)
    return p.contiguous()


def events(fn, runs=None):
    """median and spread in ms of `runs` calls between device events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs or RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(max(ts) - min(ts))


def wall(fn, runs=None):
    fn()
    ts = []
    for _ in range(runs or RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(max(ts) - min(ts))


def torch_knn(ref, qry, k, radius, chunk=2048):
    """the same lists from torch: d2 by the library's formula in float64, the k smallest (d2, index) by a stable sort"""
    R = ref.double()
    out_i = torch.empty(len(qry), k, dtype=torch.int32, device=ref.device)
    r2 = radius * radius
    for s in range(0, len(qry), chunk):
        q = qry[s:s + chunk].double()
        dx, dy, dz = q[:, None, 0] - R[None, :, 0], q[:, None, 1] - R[None, :, 1], q[:, None, 2] - R[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = torch.where(d2 <= r2, d2, torch.full_like(d2, float("inf")))
        v, i = torch.sort(d2, dim=1, stable=True)
        out_i[s:s + chunk] = torch.where(torch.isfinite(v[:, :k]), i[:, :k], torch.full_like(i[:, :k], -1)).int()
    return out_i


print(f"{torch.cuda.get_device_name(0)}; medians of {RUNS} runs between device events unless said; radius {RADIUS}", flush=True)
for M in (200_000,) if SMALL else (200_000, 2_000_000):
    pts = room(M, 1700 + M // 100_000)
    print(f"--- {M} points against themselves", flush=True)
    for frac in (1.0, 0.5, 0.25):
        t0 = time.perf_counter()
        index = cloud.NNIndex.build(pts, RADIUS * frac)
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        ks = (8, 16, 30, 64) if frac == 0.5 else (16, 30)
        for k in ks:
            lists = index.knn(pts, k, RADIUS, exclude_self=True, order=index.sorted_idx)
            full = float((lists["count"] == k).float().mean())
            row = f"cell radius*{frac:<4} ({index.cells} cells, build {build_ms:7.2f} ms wall) k {k:2d}: "
            ms, sp = events(lambda: index.knn(pts, k, RADIUS, exclude_self=True, order=index.sorted_idx))
            row += f"ordered {ms:9.3f} ms (spread {sp:.3f})"
            if frac == 0.5:
                ms, sp = events(lambda: index.knn(pts, k, RADIUS, exclude_self=True))
                row += f", input order {ms:9.3f} ms (spread {sp:.3f})"
            print(row + f"; {100 * full:.1f} % of the lists full, mean count {float(lists['count'].float().mean()):.1f}", flush=True)
            if frac == 0.5 and k in (16, 30):
                ms, sp = events(lambda: cloud.knn_moments(pts, lists, pts, [8.0, 6.0, 2.0]))
                print(f"    knn_moments on those lists, one viewpoint, all four outputs: {ms:9.3f} ms (spread {sp:.3f})", flush=True)
            del lists
        del index
        torch.cuda.empty_cache()
    ms, sp = wall(lambda: cloud.estimate_normals(pts, 30, radius=RADIUS, viewpoint=[8.0, 6.0, 2.0]), max(3, RUNS // 4))
    print(f"whole estimate_normals(k 30), index build included, host wall-clock: {ms:9.2f} ms (spread {sp:.2f})", flush=True)
    ms, sp = wall(lambda: cloud.remove_statistical_outlier(pts, 20, 2.0, radius=RADIUS), max(3, RUNS // 4))
    kept, _mask = cloud.remove_statistical_outlier(pts, 20, 2.0, radius=RADIUS)
    print(f"whole remove_statistical_outlier(nb 20, ratio 2), build and readback included, host wall-clock: {ms:9.2f} ms (spread {sp:.2f}); "
          f"{M - len(kept)} of {M} points removed", flush=True)
    del pts
    torch.cuda.empty_cache()

M = 100_000
pts = room(M, 99)
index = cloud.NNIndex.build(pts, RADIUS * cloud.KNN_CELL_FRACTION)
ours = lambda: index.knn(pts, 16, RADIUS, order=index.sorted_idx)["idx"]      # noqa: E731
ref = lambda: torch_knn(pts, pts, 16, RADIUS)                                  # noqa: E731
a, b = ours(), ref()
t = {"hip": [], "torch": []}
for _ in range(max(3, RUNS // 4)):
    for key, f in (("hip", ours), ("torch", ref)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        t[key].append((time.perf_counter() - t0) * 1e3)
print(f"--- {M} x {M}, k 16, alternating, host wall-clock: library {float(np.median(t['hip'])):.3f} ms, torch composition (chunked float64 distances + stable sort) "
      f"{float(np.median(t['torch'])):.1f} ms; {int((a != b).sum())} of {a.numel()} indices differ", flush=True)
