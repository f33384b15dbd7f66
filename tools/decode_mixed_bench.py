"""The decoder on a view pair of different resolution (decode_stereo_mixed) against today's decoder (_decode_stereo) at the two equal
sizes, alternating on one device: the mixed call pushes the same number of rows through every row-wise kernel as the MEAN of the two
equal calls, and its attention does less (tools/attn_bench.py).

    python tools/decode_mixed_bench.py [Ha Wa Hb Wb [B [precision]]]        # default 384 512 224 224 8 f16x3h

Prints the three times (median of 7 rounds of 10 calls each, device events), the ratio mixed / mean of the equal sizes, and the
equal-grid pair through both routes (what the per-side QKV launches and the missing paired QKV launch cost on their own)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                               # noqa: E402
from vista_slam_amd import weights as W                    # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

a = sys.argv[1:]
Ha, Wa, Hb, Wb = (int(v) for v in a[:4]) if len(a) >= 4 else (384, 512, 224, 224)
B = int(a[4]) if len(a) > 4 else 8
prec = a[5] if len(a) > 5 else "f16x3h"
m = STAFrontend(W.FULL, "cuda:0", precision=prec).load_procedural()
layers = sorted({hk - 1 for hk in W.FULL.hooks[1:]})


def feats(H, Wd, tag):
    img = torch.from_numpy(W.synth_images(B, H, Wd, seed=43, tag=tag)).cuda()
    return m._encode_image(img, None, normalize=False)


fa, pa = feats(Ha, Wa, 0)
fb, pb = feats(Hb, Wb, 1)
fa2, _ = feats(Ha, Wa, 2)
fb2, _ = feats(Hb, Wb, 3)
calls = {
    "mixed": lambda: m.decode_stereo_mixed(fa, fb, pa, pb, layers=layers),
    f"equal {Ha}x{Wa}": lambda: m._decode_stereo(fa, fa2, pa, pa, layers=layers),
    f"equal {Hb}x{Wb}": lambda: m._decode_stereo(fb, fb2, pb, pb, layers=layers),
    f"equal {Ha}x{Wa} by the mixed route": lambda: m.decode_stereo_mixed(fa, fa2, pa, pa, layers=layers),
    f"equal {Hb}x{Wb} by the mixed route": lambda: m.decode_stereo_mixed(fb, fb2, pb, pb, layers=layers),
}
times = {k: [] for k in calls}
for k, f in calls.items():          # warm every shape
    f(); f()
torch.cuda.synchronize()
for rnd in range(7):
    for k, f in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            f()
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) / 10 * 1e3)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
for k, v in times.items():
    print(f"{k:40s} median {med[k]:9.1f} us   (min {min(v):9.1f}, max {max(v):9.1f})")
keys = list(calls)
mean_eq = 0.5 * (med[keys[1]] + med[keys[2]])
print(f"B = {B}, {prec}: mixed {med['mixed']:.1f} us / mean of the equal sizes {mean_eq:.1f} us = {med['mixed'] / mean_eq:.3f}")
print(f"mixed route / today's route on equal grids: {Ha}x{Wa} {med[keys[3]] / med[keys[1]]:.3f}, {Hb}x{Wb} {med[keys[4]] / med[keys[2]]:.3f}")
depth = W.FULL.dec_depth
print(f"launches per decoder layer: mixed route 6 QKV-epilogue GEMMs (qkv, projk|projv, projq: once per side) + 2 attention; today's route "
      f"2 or 3 (paired qkv + projk|projv, projq) + 2: {3 * depth} to {4 * depth} more dependent launches per call")
