"""One sta_voxel_downsample call (vista_slam_amd.formats.voxel_downsample) against the torch composition that yields the same rows, on
the same GPU, in the same process, alternating: key arithmetic in float64, torch.unique(..., return_inverse, return_counts),
index_add_ in float64 for points and colours, a divide.

    python tools/voxel_bench.py [reps]            # default 5 alternating repetitions per size and side
    python tools/voxel_bench.py trace [calls]     # only the library calls, `calls` times per size after two warm-up calls: the target
                                                  # of a kernel trace (rocprofv3 --kernel-trace -d DIR -o t -- ...; python
                                                  # tools/rocpd_stats.py --by-grid DIR/*/*.db: one row per size and kernel)

Sizes: 2 M and 20 M points (40 and 400 views of 224 x 224) scattered with 1 cm of noise over the walls, floor and ceiling of a
procedural 16 x 12 x 4 m room, voxel_size 0.05.  Times are host wall-clock around a synchronised call: what a caller waits for.  The
sort's traffic per pass is printed for the record: 8 B read by the histogram, 12 B read and 12 B written by the scatter, per point."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
from vista_slam_amd import formats, weights as W           # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
reps = nums[0] if nums else 5
VOXEL = 0.05
m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)


def room(M, seed):
    """M points on the six faces of a 16 x 12 x 4 m box, uniform per face with 1 cm of normal noise; colours uniform."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    size = torch.tensor([16.0, 12.0, 4.0], device="cuda")
    p = torch.rand(M, 3, device="cuda", generator=g) * size
    face = torch.randint(0, 6, (M,), device="cuda", generator=g)
    axis, side = face // 2, (face % 2).float()
    p.scatter_(1, axis[:, None], (side * size[axis])[:, None])
    p += 0.01 * torch.randn(M, 3, device="cuda", generator=g)
    return p.contiguous(), torch.rand(M, 3, device="cuda", generator=g)


def torch_voxel(pts, col):
    P = pts.double()
    o = pts.min(dim=0).values.double() - VOXEL * 0.5
    I = torch.floor((P - o) / torch.full((), VOXEL, dtype=torch.float64, device=pts.device)).long()      # a tensor divisor: a true division (a
    #                                            Python scalar is multiplied by its reciprocal, which moves points that sit next to a voxel face)
    lo = I.min(dim=0).values
    R = I - lo
    nx, ny, _nz = [int(e).bit_length() for e in R.max(dim=0).values.tolist()]
    key = (R[:, 2] << (nx + ny)) | (R[:, 1] << nx) | R[:, 0]
    _uk, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    n = cnt.double()[:, None]
    ps = torch.zeros(len(cnt), 3, dtype=torch.float64, device=pts.device).index_add_(0, inv, P)
    cs = torch.zeros(len(cnt), 3, dtype=torch.float64, device=pts.device).index_add_(0, inv, col.double())
    return (ps / n).float(), (cs / n).float(), cnt.int(), inv.int()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


print(f"{torch.cuda.get_device_name(0)}; " + (f"{reps} library calls per size after two warm-up calls" if trace else
                                              f"{reps} alternating repetitions, host wall-clock around one synchronised call"))
for M in (2_000_000, 20_000_000):
    pts, col = room(M, 1700 + M // 1_000_000)
    ours = lambda: formats.voxel_downsample(m, pts, col, voxel_size=VOXEL, return_counts=True, return_inverse=True)      # noqa: E731
    ref = lambda: torch_voxel(pts, col)                                                                                    # noqa: E731
    if trace:
        for _ in range(2 + reps):
            ours()
        torch.cuda.synchronize()
        continue
    for f in (ours, ref):
        f()
    t = {"hip": [], "torch": []}
    for _ in range(reps):
        ms, a = clock(ours); t["hip"].append(ms)
        ms, b = clock(ref); t["torch"].append(ms)
    same = torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    if not same:
        print(f"    {int((a[3] != b[3]).sum())} of {M} inverse entries and {int((a[2] != b[2]).sum())} of {len(a[2])} counts differ", flush=True)
    step = (a[0] - b[0]).abs().max().item()
    mn, mx = pts.min(dim=0).values.cpu().numpy(), pts.max(dim=0).values.cpu().numpy()
    plan = formats.voxel_plan(mn, mx, VOXEL)
    cnt = a[2]
    print(f"{M:9d} points -> {len(cnt):8d} voxels of 1 .. {int(cnt.max())} points (median {int(cnt.median())}), key {plan.key_bits} bits, {plan.passes} passes, "
          f"{24 * M * plan.passes / 1e6:.0f} MB scattered + {8 * M * plan.passes / 1e6:.0f} MB histogrammed", flush=True)
    for k in ("hip", "torch"):
        v = t[k]
        print(f"    {k:5s} {' '.join(f'{x:8.2f}' for x in v)} ms   median {float(np.median(v)):8.2f}  spread {max(v) - min(v):6.2f}", flush=True)
    print(f"    torch / hip {float(np.median(t['torch'])) / float(np.median(t['hip'])):6.2f}; counts and inverse {'identical' if same else 'DIFFER'}, "
          f"largest |mean - mean| {step:.3g}", flush=True)
    del pts, col, a, b
    torch.cuda.empty_cache()
