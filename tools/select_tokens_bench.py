"""One sta_select_patches call (vista_slam_amd.select) against the torch composition a caller writes today for the same result, on the
same GPU, in the same process, alternating: per entry reshape / sum pooling, a compare and `nonzero` (min_score) or a stable
descending sort cut at k and sorted back (top_k), the (y, x) list, and min / max for the window.

    python tools/select_tokens_bench.py [reps]            # default 30 repetitions per case and side, medians
    python tools/select_tokens_bench.py trace [calls]     # only the library calls, `calls` times per case after two warm-up calls:
                                                          # the target of a kernel trace (rocprofv3 --kernel-trace -d DIR -o t -- ...;
                                                          # python tools/rocpd_stats.py --by-grid DIR/*/*.db: one row per case and kernel)

Cases: 10 bool masks of 224x224 (min_score 128); 16 float32 maps of 384x512 in the fixed-point sum mode, top_k = half the patches
(the largest case: 12.6 MB read); 32 uint8 maps of mixed sizes (min_score 128).  Times are host wall-clock around a synchronised call:
what a caller waits for, launch overhead included.  Both library kernels are latency-bound; the bytes/s is printed next to the time
for the record, not as a target."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
import select_cases as S                                   # noqa: E402
from vista_slam_amd import select, weights as W            # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
reps = nums[0] if nums else (10 if trace else 30)
m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
MIXED = [(224, 224), (384, 512), (512, 384), (160, 224), (16, 1040), (272, 240), (48, 64), (288, 512)]


def torch_select(maps, min_score=None, top_k=None):
    """-> per entry (scores [hp, wp] int32, index [n] int64, pos [n, 2] int64, window [4] int64), all on the device."""
    out = []
    for b, x in enumerate(maps):
        H, W_ = x.shape
        hp, wp = H // 16, W_ // 16
        if x.dtype == torch.float32:
            v = torch.where(x > 0, x, torch.zeros((), device=x.device)).clamp(max=32767.0)
            px = torch.round(v * 256.0).to(torch.int64)
        else:
            px = (x != 0).to(torch.int32)
        score = px.view(hp, 16, wp, 16).sum(dim=(1, 3)).to(torch.int32)
        flat = score.view(-1)
        if top_k is None:
            idx = torch.nonzero(flat >= min_score).squeeze(1)
        else:
            idx = torch.sort(torch.sort(flat, descending=True, stable=True).indices[:top_k[b]]).values
        y, xx = torch.div(idx, wp, rounding_mode="floor"), idx % wp
        if idx.numel():
            win = torch.stack([y.min(), xx.min(), y.max() - y.min() + 1, xx.max() - xx.min() + 1])
        else:
            win = torch.zeros(4, dtype=torch.int64, device=x.device)
        out.append((score, idx, torch.stack([y, xx], 1), win))
    return out


def agree(sel, ref):
    bad = 0
    for b, (score, idx, pos, win) in enumerate(ref):
        bad += int(not torch.equal(sel.scores[b], score)) + int(not torch.equal(sel.index[b], idx)) + int(not torch.equal(sel.pos[b], pos))
        bad += int(list(sel.windows[b]) != win.tolist())
    return f"{'identical to' if bad == 0 else f'DIFFERS ({bad} tensors) from'} the torch composition"


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, r


def cases():
    masks = [torch.from_numpy(S.random_mask(224, 224, 200 + b).astype(np.bool_)).cuda() for b in range(10)]
    yield "10 bool masks 224x224, min_score 128", masks, dict(min_score=128)
    confs = [torch.from_numpy(S.hostile_float(384, 512, 300 + b)).cuda() for b in range(16)]
    yield "16 float32 maps 384x512, sum mode, top_k 384", confs, dict(top_k=[384] * 16)
    mixed = [torch.from_numpy(S.random_mask(*MIXED[b % len(MIXED)], seed=400 + b)).cuda() for b in range(32)]
    yield "32 uint8 maps of mixed sizes, min_score 128", mixed, dict(min_score=128)


print(f"{torch.cuda.get_device_name(0)}; " + (f"{reps} library calls per case after two warm-up calls" if trace else
                                              f"medians of {reps} alternating repetitions, host wall-clock around one synchronised call"))
for tag, maps, kw in cases():
    nbytes = sum(x.numel() * x.element_size() for x in maps)
    patches = sum(x.numel() // 256 for x in maps)
    nbytes += patches * (4 + 4 + 8 + 16)                   # scores out and in, index and pos out
    ours = lambda: select.select_tokens_from_maps(m, maps, **kw)         # noqa: E731
    ref = lambda: torch_select(maps, **kw)                               # noqa: E731
    if trace:
        for _ in range(2 + reps):
            ours()
        torch.cuda.synchronize()
        print(f"{tag}: grid of patch_score_kernel = ({min((max(x.numel() // 256 for x in maps) + 15) // 16, 256)}, {len(maps)}), of patch_select_kernel = ({len(maps)})")
        continue
    for f in (ours, ref):
        f()
    t = {"hip": [], "torch": []}
    for _ in range(reps):
        us, a = clock(ours); t["hip"].append(us)
        us, b = clock(ref); t["torch"].append(us)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"{tag:48s} {patches:6d} patches  hip {med['hip']:8.1f} us (min {min(t['hip']):8.1f})  torch {med['torch']:10.1f} us (min {min(t['torch']):10.1f})  "
          f"torch / hip {med['torch'] / med['hip']:7.1f}   hip: {nbytes / 1e6:6.2f} MB touched, {nbytes / med['hip'] / 1e3:7.2f} GB/s; {agree(a, b)}", flush=True)
