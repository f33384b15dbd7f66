"""The keyframe scheduler on token subsets against what it replaces, full model, one stream, through the shim (every route waits on
the host for its pose confidences, as the SLAM loop does, so a call's device events bracket that wait too).

    python tools/regress_tokens_bench.py [precision]                 # default f16x3h

Per configuration a keyframe with k = 5 candidate edges, all frames of one size: two adjacent edges on whole frames and three loop
candidates on subsets.  The threshold is 0, so every edge is accepted and every window side pays for its DPT head.  Features are
random (the cost does not depend on their values).

    224x224, windows      loop candidates: an 8 x 10 window of the keyframe against an 8 x 10 window of the candidate
    384x512, windows      the same with 16 x 20 windows
    384x512, pruned       loop candidates: a random half of the tokens on both sides (index lists: no maps)

Quantities (median of 21 single calls after 3 warm-up calls, device events around each call):
    (a) tokens     one regress_views_tokens call (heads="entry": the DPT head once per edge)
    (a') varlen    the same call with heads="varlen": the window sides of all edges through one varlen head pass
    (b) split      the k regress_two_views_tokens_split sequences it replaces (decode_stereo_tokens, head_pose_s, a host read, head_pts)
    (c) whole      regress_views on the whole frames: what a caller without subsets pays (it computes something else)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                               # noqa: E402
from vista_slam_amd import weights as W                    # noqa: E402
from vista_slam_amd.keyframe_pipeline import regress_two_views_tokens_split        # noqa: E402
from vista_slam_amd.slam_scheduler import regress_views, regress_views_tokens      # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

prec = sys.argv[1] if len(sys.argv) > 1 else "f16x3h"
K, WARM, REPS = 5, 3, 21
cfg = W.FULL
m = STAFrontend(cfg, "cuda:0", precision=prec).load_procedural()
E = cfg.enc_embed_dim
gen = torch.Generator(device="cpu").manual_seed(43)


def config(H, Wd, kind, win):
    hp, wp = H // 16, Wd // 16
    N = hp * wp
    feats = [torch.randn(N, E, generator=gen).cuda() for _ in range(K + 1)]
    sel_i, sel_j = [None, None], [None, None]
    for e in range(2, K):
        if kind == "windows":
            h, w = win
            sel_i.append(((hp - h) // 2, (wp - w) // 2, h, w)); sel_j.append((e % (hp - h + 1), e % (wp - w + 1), h, w))
        else:
            sel_i.append(torch.randperm(N, generator=gen)[:N // 2]); sel_j.append(torch.randperm(N, generator=gen)[:N // 2])
    adjacent = [True, True] + [False] * (K - 2)
    size = (H, Wd)

    def tokens():
        return regress_views_tokens(m, feats[0], size, feats[1:], [size] * K, sel_i, sel_j, adjacent, 0.0)

    def split():
        return [regress_two_views_tokens_split(m, feats[0], size, feats[1 + e], size, sel_i[e], sel_j[e], adjacent[e], 0.0) for e in range(K)]

    def whole():
        return regress_views(m, feats[0], feats[1:], adjacent, 0.0, H, Wd)
    def tokens_varlen():
        return regress_views_tokens(m, feats[0], size, feats[1:], [size] * K, sel_i, sel_j, adjacent, 0.0, heads="varlen")
    return {"(a) tokens": tokens, "(a') varlen": tokens_varlen, "(b) split": split, "(c) whole": whole}


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


CONFIGS = [("224x224, windows 8x10", 224, 224, "windows", (8, 10)), ("384x512, windows 16x20", 384, 512, "windows", (16, 20)),
           ("384x512, pruned 50 %", 384, 512, "pruned", None)]
for name, H, Wd, kind, win in CONFIGS:
    calls = config(H, Wd, kind, win)
    a, b = calls["(a) tokens"](), calls["(b) split"]()
    torch.cuda.synchronize()
    worst = max(float((x.pose - y.pose).norm() / y.pose.norm()) for x, y in zip(a, b))
    med = {}
    print(f"{name}, k = {K}, {prec}: (a) against (b), pose, worst rel-L2 {worst:.2e}")
    for key, f in calls.items():
        med[key], lo, hi = median_us(f)
        print(f"  {key:12s} median {med[key]:9.1f} us   (min {lo:9.1f}, max {hi:9.1f})")
    print(f"  (a) / (b) = {med['(a) tokens'] / med['(b) split']:.3f}    (a) / (c) = {med['(a) tokens'] / med['(c) whole']:.3f}")
    av = med["(a') varlen"]
    print(f"  (a') / (b) = {av / med['(b) split']:.3f}    (a') / (c) = {av / med['(c) whole']:.3f}    (a') / (a) = {av / med['(a) tokens']:.3f}")
