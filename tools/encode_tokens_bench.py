"""The encoder on token subsets (encode_tokens, C ABI sta_encode_tokens) next to the whole-frame encoder (sta_encode) on the SAME
images, alternating on one device.  N = all tokens in grid order computes what sta_encode computes, through the positions table
(gather by the table, identity rotation in the QKV epilogues + one rope_tokens_kernel<., false> launch per layer): that ratio is the
price of the table route.  The other N are random selections per batch entry: each ratio is what a caller who needs that many tokens
pays of a whole-frame call.

    python tools/encode_tokens_bench.py [H W [B [precision [N ...]]]]        # default 384 512 8 f16x3h 768 576 384 192
    python tools/encode_tokens_bench.py H W B precision N trace [calls]
        only encode_tokens with that N, `calls` times after two warm-up calls: the target of a kernel trace
        (rocprofv3 --kernel-trace --stats -- python tools/encode_tokens_bench.py 384 512 8 f16x3h 384 trace)

Prints ms per call (median of 7 rounds of 10 calls each, device events) and the ratios to sta_encode."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
from vista_slam_amd import weights as W                    # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

a = [v for v in sys.argv[1:] if v != "trace"]
trace = "trace" in sys.argv[1:]
H, Wd = (int(a[0]), int(a[1])) if len(a) >= 2 else (384, 512)
B = int(a[2]) if len(a) > 2 else 8
prec = a[3] if len(a) > 3 else "f16x3h"
total = (H // 16) * (Wd // 16)
m = STAFrontend(W.FULL, "cuda:0", precision=prec).load_procedural()
img = torch.from_numpy(W.synth_images(B, H, Wd, seed=43, tag=0)).cuda()


def selection(n):
    """All tokens: grid order; fewer: a random selection per batch entry, in random order."""
    if n == total:
        return torch.arange(total)[None].expand(B, -1).contiguous().cuda()
    return torch.from_numpy(np.stack([np.random.default_rng(1000 + b).permutation(total)[:n] for b in range(B)])).cuda()


if trace:
    n, calls = int(a[4]), int(a[5]) if len(a) > 5 else 20
    idx = selection(n)
    for _ in range(2 + calls):
        m.encode_tokens(img, index=idx)
    torch.cuda.synchronize()
    print(f"{2 + calls} calls of encode_tokens, {H}x{Wd}, B = {B}, N = {n} of {total}, {prec}, {W.FULL.enc_depth} encoder layers per call")
    sys.exit(0)

Ns = [int(v) for v in a[4:]] or [total, total * 3 // 4, total // 2, total // 4]
sel = {n: selection(n) for n in Ns}
calls = {"sta_encode": lambda: m._encode_image(img, None, normalize=False)}
for n in Ns:
    calls[f"sta_encode_tokens N = {n}"] = (lambda ix: (lambda: m.encode_tokens(img, index=ix)))(sel[n])
ref = calls["sta_encode"]()[0]
for k, f in calls.items():          # warm every variant (the first call of a shape allocates)
    f(); out = f()[0]
    if out.shape == ref.shape:
        print(f"{k:32s} rel-L2 vs sta_encode {float((out - ref).norm() / ref.norm()):.2e}")
torch.cuda.synchronize()
times = {k: [] for k in calls}
for rnd in range(7):
    for k, f in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            f()
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) / 10)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
for k, v in times.items():
    print(f"{k:32s} median {med[k]:8.3f} ms   (min {min(v):8.3f}, max {max(v):8.3f})   / sta_encode = {med[k] / med['sta_encode']:.3f}")
print(f"{H}x{Wd}, B = {B}, {prec}, {total} tokens per frame")
