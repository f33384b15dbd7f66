"""The keyframe gate (vista_slam_amd.flow) timed on the GPU: the three library calls on their own (device events around one call:
pyramid of one frame, corners, track of 1000 points into one frame and into 32), the whole `FlowTracker.compute_disparity` call
including its readback (host wall-clock), and - alongside - `encode_u8hwc` of the same frame with the full-size model, the step the
gate decides on.

    python tools/flow_bench.py [reps]             # default 20 repetitions per row after 3 warm-up calls
    python tools/flow_bench.py trace [calls]      # only pyramid + corners + track (1000 points, one frame), `calls` times per size: the
                                                  # target of a kernel trace (rocprofv3 --kernel-trace -d DIR -o t -- ...; python
                                                  # tools/rocpd_stats.py --by-grid DIR/*/*.db: one row per size and kernel)

Sizes: 224 x 224 and 384 x 512, a procedural blob texture (tests/flow_cases.py) moved by (1.25, -0.5) px; the 1000 tracked points are
uniform positions inside the frame.  There is no earlier implementation of the gate on this hardware to compare a time against: the
numpy restatement is a yardstick for results, not a baseline."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
import flow_cases as F                                     # noqa: E402
from vista_slam_amd import flow, weights as W              # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
reps = nums[0] if nums else 20
m = STAFrontend(W.FULL, "cuda:0").load_procedural(seed=43)


def events(fn):
    """median, min, max of `reps` device-event times of one call, microseconds"""
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return float(np.median(t)), min(t), max(t)


def wall(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), min(t), max(t)


def row(name, r):
    print(f"    {name:46s} median {r[0]:9.1f} us   min {r[1]:9.1f}   max {r[2]:9.1f}", flush=True)


print(f"{torch.cuda.get_device_name(0)}; {reps} repetitions per row after 3 warm-up calls")
for H, Wd in ((224, 224), (384, 512)):
    a, b = F.blob_frame(H, Wd, n_blobs=400), F.blob_frame(H, Wd, (1.25, -0.5), n_blobs=400)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    gray = (db.float() / 255.0)[None].contiguous()
    u8 = torch.from_numpy(np.ascontiguousarray(np.stack([a, a, a], -1))).cuda()
    p = flow.plan(H, Wd)
    ws = torch.empty(p.workspace_bytes, device="cuda", dtype=torch.uint8)
    pa, pb = flow.pyramid(m, da), flow.pyramid(m, db)
    p32 = flow.pyramid(m, [db] * 32)
    pts = torch.from_numpy(np.random.RandomState(5).uniform([0, 0], [Wd, H], (1000, 2)).astype(np.float32)).cuda()
    _, n = flow.good_features(m, pa, workspace=ws)
    print(f"{H} x {Wd}: {p.levels} levels, pyramid {p.pyramid_bytes} B, corner workspace {p.workspace_bytes} B, {int(n.item())} corners on the texture")
    if trace:
        for _ in range(reps):
            flow.good_features(m, flow.pyramid(m, da), workspace=ws)
            flow.track(m, pa, pb, pts)
        torch.cuda.synchronize()
        continue
    print("  device events around one library call:")
    row("pyramid, uint8 frame", events(lambda: flow.pyramid(m, da)))
    row("pyramid, float32 frame", events(lambda: flow.pyramid(m, gray)))
    row("corners (1000, 0.01, 8, 7)", events(lambda: flow.good_features(m, pa, workspace=ws)))
    row("track, 1000 points into 1 frame", events(lambda: flow.track(m, pa, pb, pts)))
    row("track, 1000 points into 32 frames", events(lambda: flow.track(m, pa, p32, pts)))
    print("  host wall-clock around one synchronised call:")
    tr = flow.FlowTracker(m, 1e9)
    tr.compute_disparity(da)
    row(f"compute_disparity, no keyframe ({int(tr.kf_n.item())} corners)", wall(lambda: tr.compute_disparity(gray)))
    tk = flow.FlowTracker(m, -1.0)                         # every frame is a keyframe
    tk.compute_disparity(da)
    row("compute_disparity, keyframe (corners again)", wall(lambda: tk.compute_disparity(gray)))
    row("encode_u8hwc of the frame (full-size model)", wall(lambda: m.encode_u8hwc(u8[None])))
    del pa, pb, p32, ws
    torch.cuda.empty_cache()
