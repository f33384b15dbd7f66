"""One sta_head_pts_varlen call over all window sides of a keyframe's edges against the per-entry sta_head_pts calls it replaces, full
model, one stream, through the shim.

    python tools/head_varlen_bench.py [precision] [--parent-lib PATH]        # default f16x3h

The three configurations of tools/regress_tokens_bench.py (k = 5, every edge accepted): per edge two sides; the head runs on every
WINDOW side (a whole frame is a window).  Hooks and features are random (the cost does not depend on their values).

    224x224, windows 8x10      4 whole-frame sides (14 x 14 patches) + 6 windows of 8 x 10
    384x512, windows 16x20     4 whole-frame sides (24 x 32) + 6 windows of 16 x 20
    384x512, pruned 50 %       4 whole-frame sides only (index-list sides have no maps)

Quantities (median of 21 single calls after 3 warm-up calls, device events around each call):
    (v) varlen      ONE head_pts_varlen call over all sides
    (e) per entry   what sta_regress_views_tokens runs without the switch: per edge ONE sta_head_pts call with n = 2 (the two sides
                    of these edges share a shape), five calls (pruned: two) - with --parent-lib also on that build's library
    (1) one shape   all sides of ONE shape (ten 8 x 10 / 16 x 20 windows): head_pts_varlen against ONE batched sta_head_pts call -
                    the equal-shape overhead of the varlen route
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                               # noqa: E402
from vista_slam_amd import _lib, weights as W              # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

args = [a for a in sys.argv[1:]]
parent = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    parent = args[i + 1]
    del args[i:i + 2]
prec = args[0] if args else "f16x3h"
WARM, REPS = 3, 21
cfg = W.FULL
E, D = cfg.enc_embed_dim, cfg.dec_embed_dim
models = {"this build": STAFrontend(cfg, "cuda:0", precision=prec).load_procedural()}
if parent:
    models["parent build"] = STAFrontend(cfg, "cuda:0", precision=prec, lib=_lib.load_other(parent)).load_procedural()
gen = torch.Generator(device="cpu").manual_seed(43)


def median_us(f):
    for _ in range(WARM):
        f()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    t.sort()
    return t[len(t) // 2], t[0], t[-1]


def sides(shapes):
    """Random inputs of a list of (h, w) sides: [(feat [n, E], [three hooks [n, D]])]."""
    return [(torch.randn(h * w, E, generator=gen).cuda(), [(0.5 * torch.randn(h * w, D, generator=gen)).cuda() for _ in range(3)]) for h, w in shapes]


def toks_of(m, group):
    """decout list of head_pts for a batch of same-shape sides."""
    toks = [None] * (cfg.dec_depth + 2)
    toks[cfg.hooks[0]] = torch.stack([f for f, _ in group])
    for j, hk in enumerate(cfg.hooks[1:]):
        toks[hk] = torch.stack([h[j] for _, h in group])
    return toks


def report(name, med):
    for key, (v, lo, hi) in med.items():
        print(f"  {key:34s} median {v:9.1f} us   (min {lo:9.1f}, max {hi:9.1f})")


CONFIGS = [("224x224, windows 8x10", (14, 14), (8, 10), 6), ("384x512, windows 16x20", (24, 32), (16, 20), 6), ("384x512, pruned 50 %", (24, 32), None, 0)]
for name, whole, win, nwin in CONFIGS:
    shapes = [whole] * 4 + ([win] * nwin if win else [])
    ent = sides(shapes)
    m = models["this build"]

    def varlen(m=m, ent=ent, shapes=shapes):
        return m.head_pts_varlen([f for f, _ in ent], [[h[j] for _, h in ent] for j in range(3)], shapes)

    def per_entry(m, ent=ent, shapes=shapes):
        out = []
        for e in range(0, len(ent), 2):          # one call per edge: its two sides share a shape
            out.append(m.head_pts(toks_of(m, ent[e:e + 2]), [[16 * shapes[e][0], 16 * shapes[e][1]]] * 2))
        return out
    a, b = varlen(), per_entry(m)
    torch.cuda.synchronize()
    worst = 0.0
    for e in range(len(ent)):
        want = b[e // 2]["pts3d"][e % 2]
        worst = max(worst, float((a[e]["pts3d"][0] - want).norm() / want.norm()))
    print(f"{name}, {len(ent)} sides, {prec}: varlen against per entry, points, worst rel-L2 {worst:.2e}")
    med = {"(v) varlen, one call": median_us(varlen)}
    for tag, mm in models.items():
        med[f"(e) per entry, {len(ent) // 2} calls, {tag}"] = median_us(lambda mm=mm: per_entry(mm))
    report(name, med)
    v = med["(v) varlen, one call"][0]
    for tag in models:
        print(f"  (v) / (e, {tag}) = {v / med[f'(e) per entry, {len(ent) // 2} calls, {tag}'][0]:.3f}")
    if win:
        same = sides([win] * 10)
        med = {"(1) varlen, ten sides of one shape": median_us(lambda: m.head_pts_varlen([f for f, _ in same], [[h[j] for _, h in same] for j in range(3)], [win] * 10)),
               "(1) ONE batched head_pts, n = 10": median_us(lambda: m.head_pts(toks_of(m, same), [[16 * win[0], 16 * win[1]]] * 10))}
        report(name, med)
        print(f"  equal-shape overhead: varlen / batched = {med['(1) varlen, ten sides of one shape'][0] / med['(1) ONE batched head_pts, n = 10'][0]:.3f}")
