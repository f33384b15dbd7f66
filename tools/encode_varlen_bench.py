"""sta_encode_varlen against what it replaces, through the C ABI with preallocated outputs (no shim, no allocation in the timed loops),
everything on ONE stream, full model.

Default workload: 384 x 512 frames, 16 entries: eight whole frames of 768 tokens and eight random subsets of 768, 672, 576, 480, 384,
288, 192 and 96 tokens (tools/decode_varlen_bench.py's N2) - the two sides of the B = 8 call that tool decodes.  Frames are the
procedural images; positions are the tokens' grid positions.

    python tools/encode_varlen_bench.py [precision] [parent=PATH]      # default f16x3h
        parent=PATH: a second build of the library (libsta_mi355.so of another commit); the grouped sta_encode_tokens calls are timed on
        it as well, in the same process and the same rounds
    python tools/encode_varlen_bench.py precision trace=varlen|per_seq|grouped [calls]
        only that variant, `calls` times after two warm-up calls: the target of a kernel trace
        (rocprofv3 --kernel-trace --stats -- python tools/encode_varlen_bench.py f16x3h trace=varlen)

Columns (median of 7 rounds of 5 repetitions, device events around each round):
    varlen             one sta_encode_varlen call on the sixteen entries (dense QKV GEMM + varlen finisher)
    varlen, per-seq    the same call under experiment switch 8: one fused-epilogue QKV GEMM per sequence + one rotation launch per layer
    grouped            the sta_encode_tokens calls forward_pairs_tokens(encode="grouped") issues for these entries: one call per distinct
                       (count, frame size) - here one at B = 9 (768 tokens) and seven at B = 1
    grouped (parent)   the same calls on the parent build
    tokens B=16, equal one sta_encode_tokens call on sixteen whole frames
    varlen, equal      sta_encode_varlen on the same sixteen whole frames: the equal-count overhead
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

a = [v for v in sys.argv[1:] if "=" not in v]
opts = dict(v.split("=", 1) for v in sys.argv[1:] if "=" in v)
trace, parent = opts.get("trace"), opts.get("parent")
prec = a[0] if a else "f16x3h"
H, WD = 384, 512
HP, WP = H // 16, WD // 16
N = HP * WP
COUNTS = [768] * 8 + [768, 672, 576, 480, 384, 288, 192, 96]
B = len(COUNTS)
cfg = W.FULL
E = cfg.enc_embed_dim
m = STAFrontend(cfg, "cuda:0", precision=prec, lib=_lib.load_test()).load_procedural()
gen = torch.Generator(device="cpu").manual_seed(43)
grid = torch.cartesian_prod(torch.arange(HP), torch.arange(WP)).to(torch.int64)
frames = torch.from_numpy(W.synth_images(B, H, WD, seed=43, tag=0)).cuda()
pos = [grid.clone() if n == N else grid[torch.randperm(N, generator=gen)[:n]].contiguous() for n in COUNTS]
st = m._stream()


def varlen_call(model, idx, poss):
    b = len(idx)
    q = torch.cat(poss).cuda().contiguous()
    n = [int(p.shape[0]) for p in poss]
    out = torch.empty(sum(n), E, device="cuda")
    ptrs = (C.c_void_p * b)(*[frames[i].data_ptr() for i in idx])
    hs, ws, cn = (C.c_int * b)(*[H] * b), (C.c_int * b)(*[WD] * b), (C.c_int * b)(*n)

    def run():
        _lib.check(model.lib.sta_encode_varlen(model._h, ptrs, hs, ws, q.data_ptr(), cn, b, out.data_ptr(), st))
    run.out, run.keep = out, (q,)
    return run


def tokens_call(model, idx, poss):
    """One sta_encode_tokens call on the stacked frames idx with [b, n, 2] positions."""
    b, n = len(idx), int(poss[0].shape[0])
    img = frames[idx].contiguous()
    q = torch.stack(poss).cuda().contiguous()
    out = torch.empty(b, n, E, device="cuda")

    def run():
        _lib.check(model.lib.sta_encode_tokens(model._h, img.data_ptr(), q.data_ptr(), b, H, WD, n, out.data_ptr(), st))
    run.out, run.keep, run.idx = out, (img, q), idx
    return run


def grouped_calls(model):
    groups = {}
    for i, n in enumerate(COUNTS):
        groups.setdefault(n, []).append(i)
    calls = [tokens_call(model, idx, [pos[i] for i in idx]) for idx in groups.values()]

    def run():
        for f in calls:
            f()
    run.calls = calls
    return run


def with_option(f, idx, value):
    def run():
        _lib.check(m.lib.sta_debug_set_option(m._h, idx, value))
        try:
            f()
        finally:
            _lib.check(m.lib.sta_debug_set_option(m._h, idx, 0))
    return run


varlen = varlen_call(m, list(range(B)), pos)
per_seq = with_option(varlen_call(m, list(range(B)), pos), 8, 1)
grouped = grouped_calls(m)

if trace is not None:
    target = {"varlen": varlen, "per_seq": per_seq, "grouped": grouped}[trace]
    n = int(a[1]) if len(a) > 1 else 10
    for _ in range(2 + n):
        target()
    torch.cuda.synchronize()
    print(f"{2 + n} repetitions of {trace}, counts {COUNTS}, {prec}, {cfg.enc_depth} encoder layers per call")
    sys.exit(0)

calls = {"varlen": varlen, "varlen, per-seq": per_seq, "grouped": grouped}
if parent:
    mp = STAFrontend(cfg, "cuda:0", precision=prec, lib=_lib.load_other(parent)).load_procedural()
    calls["grouped (parent)"] = grouped_calls(mp)
whole = [grid.clone()] * B
calls["tokens B=16, equal"] = tokens_call(m, list(range(B)), whole)
calls["varlen, equal"] = varlen_call(m, list(range(B)), whole)
for f in calls.values():
    f(); f()
torch.cuda.synchronize()
# the routes to the same answer agree
off = [0]
for n in COUNTS:
    off.append(off[-1] + n)
worst = 0.0
for c in grouped.calls:
    for j, i in enumerate(c.idx):
        got = varlen.out[off[i]:off[i + 1]]
        worst = max(worst, float((got - c.out[j]).norm() / c.out[j].norm()))
print(f"varlen vs the grouped calls: worst entry rel-L2 {worst:.2e}")
times = {k: [] for k in calls}
for rnd in range(7):
    for k, f in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            f()
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) / 5 * 1e3)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
for k, v in times.items():
    print(f"{k:20s} median {med[k]:9.1f} us   (min {min(v):9.1f}, max {max(v):9.1f})")
print(f"384x512, 16 entries {COUNTS}, {prec}:")
base = "grouped (parent)" if parent else "grouped"
print(f"  varlen / {base:17s}          = {med['varlen'] / med[base]:.3f}   (must be below 1.0)")
print(f"  varlen / varlen per-sequence QKV     = {med['varlen'] / med['varlen, per-seq']:.3f}")
print(f"  equal counts: varlen / tokens B = 16 = {med['varlen, equal'] / med['tokens B=16, equal']:.3f}   (the equal-count overhead)")
