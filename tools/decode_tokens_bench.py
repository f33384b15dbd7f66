"""The decoder on token subsets (decode_stereo_tokens, C ABI sta_decode_tokens) against the mixed-resolution decoder
(decode_stereo_mixed) on the SAME patch-grid inputs, alternating on one device: the two compute the same thing, the tokens route
through the positions table (identity rotation in the QKV epilogues + two rope_tokens_kernel launches per layer), so the ratio is the
price of the table route.  Third column: the same entry with the rotation done by per-buffer rope_planes_kernel launches (experiment
switch 3 of include/sta_mi355_debug.h: eight launches per layer) - what the entry would cost on the existing kernel.

    python tools/decode_tokens_bench.py [Ha Wa Hb Wb [B [precision]]]        # default 384 512 224 224 8 f16x3h
    python tools/decode_tokens_bench.py Ha Wa Hb Wb B precision trace=tokens|planes [calls]
        only that variant, `calls` times after two warm-up calls: the target of a kernel trace
        (rocprofv3 --kernel-trace --stats -- python tools/decode_tokens_bench.py 384 512 224 224 8 f16x3h trace=tokens)

Prints the three times (median of 7 rounds of 10 calls each, device events) and the ratios.  Needs the test-hooks library (the
experiment switch lives there)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                               # noqa: E402
from vista_slam_amd import _lib                            # noqa: E402
from vista_slam_amd import weights as W                    # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

a = [v for v in sys.argv[1:] if not v.startswith("trace=")]
trace = next((v.split("=", 1)[1] for v in sys.argv[1:] if v.startswith("trace=")), None)
Ha, Wa, Hb, Wb = (int(v) for v in a[:4]) if len(a) >= 4 else (384, 512, 224, 224)
B = int(a[4]) if len(a) > 4 else 8
prec = a[5] if len(a) > 5 else "f16x3h"
m = STAFrontend(W.FULL, "cuda:0", precision=prec, lib=_lib.load_test()).load_procedural()
layers = sorted({hk - 1 for hk in W.FULL.hooks[1:]})


def feats(H, Wd, tag):
    img = torch.from_numpy(W.synth_images(B, H, Wd, seed=43, tag=tag)).cuda()
    return m._encode_image(img, None, normalize=False)


def per_buffer(on):
    _lib.check(m.lib.sta_debug_set_option(m._h, 3, 1 if on else 0))


fa, pa = feats(Ha, Wa, 0)
fb, pb = feats(Hb, Wb, 1)


def tokens(planes):
    per_buffer(planes)
    out = m.decode_stereo_tokens(fa, fb, pa, pb, layers=layers)
    per_buffer(False)
    return out


if trace is not None:
    assert trace in ("tokens", "planes"), trace
    n = int(a[6]) if len(a) > 6 else 20
    for _ in range(2 + n):
        tokens(trace == "planes")
    torch.cuda.synchronize()
    print(f"{2 + n} calls of decode_stereo_tokens ({'per-buffer rope_planes_kernel' if trace == 'planes' else 'rope_tokens_kernel'}), "
          f"{Ha}x{Wa} vs {Hb}x{Wb}, B = {B}, {prec}, {W.FULL.dec_depth} decoder layers per call")
    sys.exit(0)

calls = {
    "mixed (sta_decode_mixed)": lambda: m.decode_stereo_mixed(fa, fb, pa, pb, layers=layers),
    "tokens (sta_decode_tokens)": lambda: tokens(False),
    "tokens, per-buffer rope_planes_kernel": lambda: tokens(True),
}
ref = calls["mixed (sta_decode_mixed)"]()
for k, f in calls.items():          # warm every variant; they compute the same thing
    f(); out = f()
    d = max(float((x - y).norm() / y.norm()) for o, r in zip(out, ref) for x, y in zip(o, r) if x is not None)
    print(f"{k:40s} rel-L2 vs the mixed route {d:.2e}")
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
        times[k].append(e0.elapsed_time(e1) / 10 * 1e3)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
for k, v in times.items():
    print(f"{k:40s} median {med[k]:9.1f} us   (min {min(v):9.1f}, max {max(v):9.1f})")
keys = list(calls)
print(f"{Ha}x{Wa} vs {Hb}x{Wb}, B = {B}, {prec}: tokens / mixed = {med[keys[1]] / med[keys[0]]:.3f} (the price of the table route); "
      f"per-buffer rotation / rope_tokens_kernel = {med[keys[2]] / med[keys[1]]:.3f}")
