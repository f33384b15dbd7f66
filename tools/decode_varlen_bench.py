"""sta_decode_varlen against what it replaces, through the C ABI with preallocated outputs (no shim, no allocation in the timed
loops), everything on ONE stream, full model.

Default workload: 384 x 512 frames, B = 8; side 1 whole frames of 768 tokens, side 2 random subsets of 768, 672, 576, 480, 384, 288,
192 and 96 tokens of another frame.  Features are random (the decoder's cost does not depend on their values); positions are the
tokens' grid positions.

    python tools/decode_varlen_bench.py [precision]                 # default f16x3h
    python tools/decode_varlen_bench.py precision trace=varlen|b1 [calls]
        only that variant, `calls` times after two warm-up calls: the target of a kernel trace
        (rocprofv3 --kernel-trace --stats -- python tools/decode_varlen_bench.py f16x3h trace=varlen)

Columns (median of 7 rounds of 10 repetitions, device events around each round):
    varlen             one sta_decode_varlen call on the eight entries
    8 x B=1 tokens     eight sta_decode_tokens calls at B = 1, back to back: the baseline - the only way to get the same answer before
    padded B=8 tokens  one sta_decode_tokens call with every entry at 768 / 768: what padding costs (it computes something else)
    varlen, equal      sta_decode_varlen with eight equal entries 768 / 768 against the padded call above: the equal-count overhead
"""
import ctypes as C
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
prec = a[0] if a else "f16x3h"
HP, WP = 24, 32
N = HP * WP
N2 = [768, 672, 576, 480, 384, 288, 192, 96]
B = len(N2)
cfg = W.FULL
m = STAFrontend(cfg, "cuda:0", precision=prec).load_procedural()
E, D, L = cfg.enc_embed_dim, cfg.dec_embed_dim, cfg.dec_depth + 1
layers = sorted({hk - 1 for hk in cfg.hooks[1:]})
gen = torch.Generator(device="cpu").manual_seed(43)
grid = torch.cartesian_prod(torch.arange(HP), torch.arange(WP)).to(torch.int64)

f1 = [torch.randn(N, E, generator=gen).cuda() for _ in range(B)]
p1 = [grid.clone().cuda() for _ in range(B)]
sel = [torch.randperm(N, generator=gen)[:n] for n in N2]
f2 = [torch.randn(n, E, generator=gen).cuda() for n in N2]
p2 = [grid[s].contiguous().cuda() for s in sel]
st = m._stream()


def outs(rows1, rows2):
    o1, o2 = (C.c_void_p * L)(), (C.c_void_p * L)()
    keep = []
    for i in layers:
        t1, t2 = torch.empty(rows1, D, device="cuda"), torch.empty(rows2, D, device="cuda")
        keep += [t1, t2]
        o1[i], o2[i] = t1.data_ptr(), t2.data_ptr()
    return o1, o2, keep


def varlen_call(fa, fb, pa, pb):
    F1, Q1, n1 = m.pack_varlen(fa, pa, E, m.device)
    F2, Q2, n2 = m.pack_varlen(fb, pb, E, m.device)
    o1, o2, keep = outs(sum(n1) + len(n1), sum(n2) + len(n2))
    c1, c2 = (C.c_int * len(n1))(*n1), (C.c_int * len(n2))(*n2)

    def run():
        _lib.check(m.lib.sta_decode_varlen(m._h, F1.data_ptr(), F2.data_ptr(), Q1.data_ptr(), Q2.data_ptr(), c1, c2, len(n1), WP - 1, o1, o2, st))
    run.keep = (F1, F2, Q1, Q2, keep)
    return run


def tokens_call(fa, fb, pa, pb):
    """One sta_decode_tokens call on stacked [b, n, .] inputs."""
    b, na, nb = fa.shape[0], fa.shape[1], fb.shape[1]
    o1, o2, keep = outs(b * (na + 1), b * (nb + 1))

    def run():
        _lib.check(m.lib.sta_decode_tokens(m._h, fa.data_ptr(), fb.data_ptr(), pa.data_ptr(), pb.data_ptr(), b, na, nb, WP - 1, o1, o2, st))
    run.keep = (fa, fb, pa, pb, keep)
    return run


varlen = varlen_call(f1, f2, p1, p2)
singles = [tokens_call(f1[b][None].contiguous(), f2[b][None].contiguous(), p1[b][None].contiguous(), p2[b][None].contiguous()) for b in range(B)]


def b1():
    for f in singles:
        f()


fpad = torch.randn(B, N, E, generator=gen).cuda()
padded = tokens_call(torch.stack(f1), fpad, torch.stack(p1), torch.stack(p1))
equal = varlen_call(f1, list(fpad), p1, p1)

if trace is not None:
    assert trace in ("varlen", "b1"), trace
    n = int(a[1]) if len(a) > 1 else 20
    for _ in range(2 + n):
        (varlen if trace == "varlen" else b1)()
    torch.cuda.synchronize()
    print(f"{2 + n} repetitions of {'one sta_decode_varlen call' if trace == 'varlen' else 'eight B = 1 sta_decode_tokens calls'}, "
          f"768 vs {N2}, {prec}, {cfg.dec_depth} decoder layers per call")
    sys.exit(0)

calls = {"varlen": varlen, "8 x B=1 tokens": b1, "padded B=8 tokens": padded, "varlen, equal": equal}
for f in calls.values():
    f(); f()
torch.cuda.synchronize()
# the two routes to the same answer agree
last = layers[-1]
v_last = varlen.keep[4][2 * layers.index(last)]
r0 = 0
worst = 0.0
for b in range(B):
    s_last = singles[b].keep[4][2 * layers.index(last)]
    worst = max(worst, float((v_last[r0:r0 + N + 1] - s_last).norm() / s_last.norm()))
    r0 += N + 1
print(f"varlen vs the eight B = 1 calls, side 1, last layer: worst rel-L2 {worst:.2e}")
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
    print(f"{k:20s} median {med[k]:9.1f} us   (min {min(v):9.1f}, max {max(v):9.1f})")
print(f"384x512, B = 8, side 1 768 tokens, side 2 {N2}, {prec}:")
print(f"  varlen / eight B = 1 calls   = {med['varlen'] / med['8 x B=1 tokens']:.3f}   (must be below 1.0)")
print(f"  varlen / padded B = 8 call   = {med['varlen'] / med['padded B=8 tokens']:.3f}   (context: padding computes something else)")
print(f"  equal counts: varlen / tokens = {med['varlen, equal'] / med['padded B=8 tokens']:.3f}   (the equal-count overhead)")
