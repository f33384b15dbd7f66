"""The attention kernel alone (sta_bench_attention) on the encoder / decoder shapes of the benchmark.
    python tools/attn_bench.py [precision]
Last block: the two-group launch (sta_bench_attention_mixed; the decoder on view pairs of different resolution) against the equal-grid
launches of the same token counts, alternating.  A cross-attention launch of B pairs N1 / N2 computes 2 B N1 N2 scores, the pair of
equal launches (2B sequences each) 2 B (N1^2 + N2^2): the figure to compare the mixed time with is the sum of the two equal times
scaled by N1 N2 / (N1^2 + N2^2)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from vista_slam_amd import weights as W, _lib
from vista_slam_amd import _lib as _hooks_lib; _hooks_lib.use_test_hooks()      # tools use the test-hooks build (include/sta_mi355_debug.h)
from vista_slam_amd.sta_frontend import STAFrontend
prec = sys.argv[1] if len(sys.argv) > 1 else "f16x3"
m = STAFrontend(W.TINY, "cuda:0", precision=prec).load_procedural()
st = torch.cuda.current_stream().cuda_stream
for name, S, heads, nq, nk, pose in (("enc 16x16 768", 16, 16, 768, 768, 0), ("dec 16x12 768+pose", 16, 12, 768, 768, 1),
                                     ("dec 16x12 769 (round 2)", 16, 12, 769, 769, 0), ("enc 224^2 B8", 16, 16, 196, 196, 0), ("enc 2x16 768", 2, 16, 768, 768, 0),
                                     ("SLAM enc 1x16 196", 1, 16, 196, 196, 0), ("SLAM dec 10x12 196+pose", 10, 12, 196, 196, 1),
                                     ("SLAM dec 10x12 197 (round 2)", 10, 12, 197, 197, 0), ("SLAM dec 2x12 196+pose", 2, 12, 196, 196, 1),
                                     ("B1 dec 2x12 768+pose", 2, 12, 768, 768, 1), ("B1 dec 2x12 769 (round 2)", 2, 12, 769, 769, 0),
                                     ("B2 dec 4x12 768+pose", 4, 12, 768, 768, 1), ("B2 dec 4x12 769 (round 2)", 4, 12, 769, 769, 0)):
    row = f"{name:24s}"
    gf = 4.0 * S * heads * (nq + pose) * (nk + pose) * 64 / 1e9
    for rep in range(2):
        ms = C.c_float()
        _lib.check(m.lib.sta_bench_attention(m._h, S, heads, nq, nk, pose, 20, 0, C.byref(ms), st))
        row += f"  {ms.value * 1e3:7.1f} us ({gf / ms.value:5.0f} TF)"
    print(row, flush=True)


def _mixed(S1, S2, heads, qa, ka, qb, kb, shift):
    ms = C.c_float()
    _lib.check(m.lib.sta_bench_attention_mixed(m._h, S1, S2, heads, qa, ka, qb, kb, shift, 20, C.byref(ms), st))
    return ms.value * 1e3


def _equal(S, heads, n):
    ms = C.c_float()
    _lib.check(m.lib.sta_bench_attention(m._h, S, heads, n, n, 1, 20, 0, C.byref(ms), st))
    return ms.value * 1e3


if hasattr(m.lib, "sta_bench_attention_mixed"):
    for B, n1, n2 in ((8, 768, 196), (1, 768, 196), (8, 196, 140), (1, 196, 140), (8, 256, 196)):
        cross, selfa, e1, e2 = [], [], [], []
        for rep in range(5):                     # alternating
            cross.append(_mixed(B, B, 12, n1, n2, n2, n1, B)); e1.append(_equal(2 * B, 12, n1))
            selfa.append(_mixed(B, B, 12, n1, n1, n2, n2, 0)); e2.append(_equal(2 * B, 12, n2))
        med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
        scale = n1 * n2 / (n1 * n1 + n2 * n2)
        target = (med(e1) + med(e2)) * scale
        print(f"mixed B={B} {n1}/{n2} x 12 heads: cross {med(cross):7.1f} us, self {med(selfa):7.1f} us | equal launches {n1}^2 {med(e1):7.1f} us + "
              f"{n2}^2 {med(e2):7.1f} us; scaled by {scale:.3f}: {target:7.1f} us -> cross / scaled {med(cross) / target:.2f}, "
              f"self / half the sum {med(selfa) / (0.5 * (med(e1) + med(e2))):.2f}", flush=True)
