"""Loop candidates (vista_slam_amd.loop) timed on the GPU: the three library calls on their own (device events around one call:
`sta_orb_extract` with the default parameters, `sta_bow_transform` through a procedural k = 10, L = 6 tree, `sta_bow_score` against a
database of 400 views), a whole `LoopDetector.detect_loop` call with its readback against 400 earlier views (host wall-clock), and -
alongside, for scale - `encode_u8hwc` of the same frame with the full-size model.

    python tools/loop_bench.py [reps]             # default 20 repetitions per row after 3 warm-up calls

Sizes: 224 x 224 and 384 x 512, a procedural blob texture (tests/flow_cases.py).  Nobody has measured these steps before and no target is
set: there is no earlier implementation of the detector on this hardware, and what the reference's CPU detector costs cannot be measured
where cv2 and DBoW3 are absent.  The numpy restatement is a yardstick for results, not a baseline."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
import flow_cases as F                                     # noqa: E402
from vista_slam_amd import loop, weights as W              # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
reps = nums[0] if nums else 20
VIEWS = 400
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
    print(f"    {name:52s} median {r[0]:9.1f} us   min {r[1]:9.1f}   max {r[2]:9.1f}", flush=True)


def full_tree(k, depth, seed):
    """a complete k-ary tree in breadth-first order (the children of node i are k i + 1 .. k i + k), random descriptors and weights"""
    rng = np.random.RandomState(seed)
    inner = sum(k ** d for d in range(depth))
    n = inner + k ** depth
    idx = np.arange(n)
    return loop.Vocabulary.from_arrays(rng.randint(0, 256, (n, 32)).astype(np.uint8), np.where(idx < inner, idx * k + 1, 0),
                                       np.where(idx < inner, k, 0), np.where(idx >= inner, idx - inner, -1), 0.25 + 3.0 * rng.rand(k ** depth))


voc = full_tree(10, 6, 5).bind(m)
print(f"{torch.cuda.get_device_name(0)}; {reps} repetitions per row after 3 warm-up calls; vocabulary k = 10, L = 6: {voc.n_nodes} nodes, {voc.n_words} words")
for H, Wd in ((224, 224), (384, 512)):
    frames = [F.blob_frame(H, Wd, (0.7 * k, 0.3 * k), n_blobs=400) for k in range(4)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    u8 = torch.from_numpy(np.ascontiguousarray(np.stack([frames[0]] * 3, -1))).cuda()
    ex = loop.Extractor(m)
    kp, resp, desc, n, p = ex.extract(dev[0])
    out = (kp, resp, desc, n)
    vec = voc.transform(desc, n)
    det = loop.LoopDetector(m, voc, 10, 5, 3, max_views=VIEWS + 8)
    for k in range(VIEWS):
        det.detect_loop(dev[k % 4], max(0, k - 3))
    print(f"{H} x {Wd}: {p.built} levels, workspace {p.workspace_bytes} B, {int(n.item())} keypoints, {int(vec.n.item())} words on the texture")
    print("  device events around one library call:")
    row("sta_orb_extract (500 features, 8 levels)", events(lambda: ex.extract(dev[0], out=out)))
    row("sta_bow_transform (k = 10, L = 6)", events(lambda: voc.transform_into(desc, n, vec.words, vec.counts, vec.vals, vec.n)))

    row(f"sta_bow_score against {VIEWS} views", events(lambda: det.score_views(0, VIEWS)))
    print("  host wall-clock around one synchronised call:")

    def detect():
        det.bow_feats = det.bow_feats[:VIEWS]                # always view number 400 against the 400 before it
        det.detect_loop(dev[1], VIEWS - 3)
    row(f"detect_loop with its readback, {VIEWS} earlier views", wall(detect))
    row("encode_u8hwc of the frame (full-size model)", wall(lambda: m.encode_u8hwc(u8[None])))
    del det, ex
    torch.cuda.empty_cache()
