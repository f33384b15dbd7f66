"""Fixtures `tests/golden/rvt_*.npz`: the REFERENCE's `regress_two_views` (vista_slam/slam.py:153-189) on per-edge TOKEN SUBSETS - what
`slam_scheduler.regress_views_tokens` answers for all candidate edges of a keyframe in one call.

TEST INFRASTRUCTURE, like tools/gen_golden_decv.py: needs the reference tree (oracle.ref_import), writes data only.  Weights and
images are procedural (vista_slam_amd.weights): the keyframe is synth_images(1, H, W, seed, tag 0), candidate e is tag 1 + e, every
frame encoded WHOLE by the reference's `_encode_image(normalize=False)` (what `add_view` caches, slam.py:142-151).  A selection slices
that encoding and its positions; edge e is then the body of `regress_two_views` statement by statement at B = 1 on the two slices:
`_decode_stereo`, `head_pose_s` on side i's pose token, the accept / reject test, `head_pts` per WINDOW side at (16 h, 16 w) (j
first), and `estimate_intrinsic_from_pts3d(shared_intrinsic=True)` where both sides are windows of one shape (the reference's
torch.cat exists for nothing else).

    python tools/gen_golden_rvt.py              # every case (the full-architecture one takes a few minutes on a CPU; the seed
                                                # search of rvt_tiny_k4_edges about twenty: it ends at seed 926)
    python tools/gen_golden_rvt.py tiny         # the tiny cases / any list of case names

Each fixture records, with <e> the edge and <t> in (i, j) the side,
    hw_i [2], hw_j [k, 2]            frame sizes;  adjacent [k];  thres;  accepted [k];  conf [k];  pose [k, 4, 4]
    win_<t> [k, 4]                   (y0, x0, h, w) of a window side (the whole frame is (0, 0, hp, wp)), zeros for an index list
    idx_<t>_e<e>                     the index list of an index-list side
    feat_i, feat_j_e<e>              the cached whole-frame encodings (tiny cases only; the consumer of a full case encodes itself)
    confs_<t>_e<e>, depths_<t>_e<e>  maps of a window side of an accepted edge, every sub-th pixel of both axes, with their L2 norms
                                     confs_l2_<t>_e<e> / depths_l2_<t>_e<e> over all pixels
    intri_e<e>                       the pair-shared K of an accepted edge whose sides are windows of one shape
    ref_noise                        rel-L2 between the reference's own fp32 and fp64 last decoder layer (worst edge and side),
                                     asserted <= 1e-4; a case takes the first seed from `seed_from` upward that holds its assertions
    alt_whole [k]                    rel-L2 between the edge's pose and the reference's pose for the same edge on the WHOLE frames: what a
                                     gather that ignored the selection would give.  Asserted >= 3e-3 for every edge with a proper subset.
The threshold of a case lies in the widest gap between the confidences it must separate (rvt_tiny_k4_edges: edge 0 below, edge 3
above; rvt_tiny_k3_win_sharp: a non-adjacent edge on either side; rvt_full_224_k3: below every edge, so every map is compared) and
the seed search runs until such a gap exists: procedural weights put the confidences of a keyframe within about 0.01 of each other,
so most seeds fail that test, which is why it comes first and is cheap.  Every |conf - thres| >= 1e-2 (asserted);
`check_mixtures` asserts over the three fixtures together that a non-adjacent edge is rejected, one is accepted, and accepted edges
cover window / window, window / index list and index list / index list.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vista_slam_amd import weights as W          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
REF_NOISE_MAX = 1e-4
ALT_WHOLE_MIN = 3e-3
THRES_MARGIN = 1e-2
torch.set_grad_enabled(False)


def _perm(n, k, seed):
    return np.random.default_rng(seed).permutation(n)[:k]


# A selection: None (whole frame) | (y0, x0, h, w) | index array.  edges: [(sel_i, (Hj, Wj), sel_j, adjacent)]
CASES = {
    # whole / whole accepted only by the adjacency exemption; window vs whole of another size (maps on both sides, no K); 17 permuted
    # indices vs a window (maps on side j only); one token vs 65 of 80 indices (no maps): every mixture of the sides in one call
    "rvt_tiny_k4_edges": dict(cfg="tiny", hw=(80, 96), seed_from=43, edges=[
        (None, (80, 96), None, True),
        ((1, 2, 2, 3), (48, 64), None, False),
        (_perm(30, 17, 1), (64, 80), (0, 1, 4, 4), False),
        (np.array([5]), (128, 160), _perm(80, 65, 2), False)], need=dict(below=[0], above=[3])),
    # three window-vs-window edges of equal shape (K defined), the tiny stress conditioning
    "rvt_tiny_k3_win_sharp": dict(cfg="tiny", hw=(80, 96), qk_gain=4.0, seed_from=43, edges=[
        ((1, 2, 2, 3), (80, 96), (2, 1, 2, 3), False),
        ((2, 0, 3, 5), (80, 96), (0, 1, 3, 5), False),
        ((0, 1, 4, 4), (64, 80), (0, 0, 4, 4), False)], need=dict(split=True)),
    "rvt_full_224_k3": dict(cfg="full", hw=(224, 224), sub=8, seed_from=43, edges=[
        (None, (224, 224), None, True),
        ((6, 4, 8, 10), (224, 224), None, False),
        (_perm(196, 140, 43), (224, 224), None, False)], need=dict(all=True)),
}


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def selection(sel, hp, wp):
    """-> (window [4] (zeros for an index list), idx [n] int64 into the row-major grid, map grid (h, w) or None)."""
    if sel is None:
        sel = (0, 0, hp, wp)
    if isinstance(sel, tuple):
        y0, x0, h, w = sel
        assert h >= 1 and w >= 1 and 0 <= y0 and y0 + h <= hp and 0 <= x0 and x0 + w <= wp
        idx = (np.arange(y0, y0 + h)[:, None] * wp + np.arange(x0, x0 + w)[None, :]).ravel().astype(np.int64)
        return np.array(sel, np.int64), idx, (h, w)
    idx = np.asarray(sel).astype(np.int64)
    assert idx.ndim == 1 and idx.size >= 1 and idx.min() >= 0 and idx.max() < hp * wp
    return np.zeros(4, np.int64), idx, None


def kind(win):
    return "win" if int(win[2]) * int(win[3]) else "idx"


def pick_threshold(conf, adjacent, need):
    """The midpoint of the widest gap that satisfies `need`: below / above = edges whose confidence must lie below / above the
    threshold, split = a non-adjacent edge on either side; all = every edge accepted on its confidence (2 x the margin below the
    lowest).  -> (thres, margin) or None."""
    if need.get("all"):
        return min(float(v) for v in conf) - 2 * THRES_MARGIN, 2 * THRES_MARGIN
    c = sorted(set(float(v) for v in conf))
    best = None
    for lo, hi in zip(c[:-1], c[1:]):
        t = 0.5 * (lo + hi)
        if any(conf[e] > t for e in need.get("below", [])) or any(conf[e] < t for e in need.get("above", [])):
            continue
        non = [conf[e] for e in range(len(conf)) if not adjacent[e]]
        if need.get("split") and not (min(non) < t < max(non)):
            continue
        if best is None or hi - lo > best[1]:
            best = (t, hi - lo)
    if best is None:
        return None
    return best[0], 0.5 * best[1]


def _grow_rope(model, top, dtype):
    # the reference's python RoPE indexes a reused cos / sin table with the call's minimum position as its origin: make the table
    # cover every position of the call, from 0, beforehand (the note in gen_golden_enct.encode_subset)
    model.rope(torch.zeros(1, 1, 2, 64, dtype=dtype), torch.tensor([[[0, 0], [top, top]]]))


def build_case(name, seed=None):
    """-> dict of arrays, the fixture of case `name`.  Needs the reference tree."""
    from oracle.ref_import import load_reference_model
    from oracle.gen_golden import _ref_slam_utils
    su = _ref_slam_utils()
    c = CASES[name]
    cfg = W.TINY if c["cfg"] == "tiny" else W.FULL
    qk_gain, sub = c.get("qk_gain", 1.0), c.get("sub", 1)
    Hi, Wi = c["hw"]
    k = len(c["edges"])
    adjacent = [e[3] for e in c["edges"]]
    threads = torch.get_num_threads()
    if c["cfg"] == "tiny":
        torch.set_num_threads(1)          # the tiny fixtures regenerate bit for bit (tests/test_regress_tokens_cpu.py): one summation order
    try:
        seeds = [seed] if seed is not None else [c["seed_from"] + i for i in range(c.get("seeds", 1024))]
        why = "no seed tried"
        sels = [(selection(sel_i, Hi // 16, Wi // 16), selection(sel_j, Hj // 16, Wj // 16)) for sel_i, (Hj, Wj), sel_j, _adj in c["edges"]]
        for sd_seed in seeds:
            sd = W.state_dict(cfg, seed=sd_seed, qk_gain=qk_gain)
            model = load_reference_model(cfg, sd)
            top = max([Hi, Wi] + [v for e in c["edges"] for v in e[1]]) // 16
            _grow_rope(model, top, torch.float32)

            def encode(H, W_, tag):
                img = torch.from_numpy(W.synth_images(1, H, W_, seed=sd_seed, tag=tag).copy())
                return model._encode_image(img, torch.tensor([[H, W_]]), normalize=False)

            fi, pi = encode(Hi, Wi, 0)
            frames_j = [encode(H, W_, 1 + e) for e, (_s, (H, W_), _t, _a) in enumerate(c["edges"])]
            edges = []
            for e, ((wi, ii, gi), (wj, ij, gj)) in enumerate(sels):
                fj, pj = frames_j[e]
                a = (fi[:, ii], pi[:, ii]); b = (fj[:, ij], pj[:, ij])
                d1, d2 = model._decode_stereo(a[0], b[0], a[1], b[1])
                pose = model.head_pose_s(d1[-1][:, 0, :])
                edges.append(dict(win=(wi, wj), idx=(ii, ij), grid=(gi, gj), feat=(a[0], b[0]), pos=(a[1], b[1]), dec=(d1, d2), pose=pose["pose"][0].numpy().copy(),
                                  conf=float(pose["conf"][0]), proper=len(ii) < fi.shape[1] or len(ij) < fj.shape[1]))
            conf = [ed["conf"] for ed in edges]
            picked = pick_threshold(conf, adjacent, c["need"])
            if picked is None or picked[1] < THRES_MARGIN:         # the cheap test first: most seeds end here
                why = f"no threshold with a margin of {THRES_MARGIN:g} separates the confidences as the case needs"
                print(f"[rvt] {name}: seed {sd_seed} conf {[round(v, 4) for v in conf]} refused: {why}", flush=True)
                continue
            model64 = load_reference_model(cfg, sd).double()
            _grow_rope(model64, top, torch.float64)
            noise = 0.0
            for e, ed in enumerate(edges):
                fj, pj = frames_j[e]
                e1, e2 = model64._decode_stereo(ed["feat"][0].double(), ed["feat"][1].double(), ed["pos"][0], ed["pos"][1])
                noise = max(noise, rel_l2(ed["dec"][0][-1].numpy(), e1[-1].numpy()), rel_l2(ed["dec"][1][-1].numpy(), e2[-1].numpy()))
                w1, _w2 = model._decode_stereo(fi, fj, pi, pj)            # the same edge on the whole frames
                ed["alt"] = rel_l2(ed["pose"][None], model.head_pose_s(w1[-1][:, 0, :])["pose"].numpy())
            del model64
            conf = [ed["conf"] for ed in edges]
            alts = ["%.1e" % ed["alt"] for ed in edges]
            print(f"[rvt] {name}: seed {sd_seed} ref_noise {noise:.2e} conf {[round(v, 4) for v in conf]} alt_whole {alts}", flush=True)
            if noise > REF_NOISE_MAX:
                why = f"ref_noise {noise:.2e} > {REF_NOISE_MAX:g}"
            elif any(ed["proper"] and ed["alt"] < ALT_WHOLE_MIN for ed in edges):
                why = "the selection of an edge moves its pose by less than alt_whole's bound"
            else:
                break
            print(f"[rvt] {name}: seed {sd_seed} refused: {why}", flush=True)
        else:
            raise AssertionError(f"{name}: no seed in {seeds} holds the assertions ({why})")
        thres = picked[0]
        res = {"hw_i": np.array([Hi, Wi], np.int64), "hw_j": np.array([e[1] for e in c["edges"]], np.int64),
               "adjacent": np.array(adjacent), "thres": np.float64(thres), "thres_margin": np.float64(picked[1]),
               "conf": np.array(conf, np.float32), "pose": np.stack([ed["pose"] for ed in edges]),
               "win_i": np.stack([ed["win"][0] for ed in edges]), "win_j": np.stack([ed["win"][1] for ed in edges]),
               "alt_whole": np.array([ed["alt"] for ed in edges]), "proper": np.array([ed["proper"] for ed in edges]),
               "ref_noise": np.float64(noise)}
        if c["cfg"] == "tiny":
            res["feat_i"] = fi[0].numpy().copy()
        acc = []
        for e, ed in enumerate(edges):
            if c["cfg"] == "tiny":
                res[f"feat_j_e{e}"] = frames_j[e][0][0].numpy().copy()
            for t, tag in enumerate("ij"):
                if ed["grid"][t] is None:
                    res[f"idx_{tag}_e{e}"] = ed["idx"][t]
            accepted = not (ed["conf"] < thres and not adjacent[e])           # slam.py:169
            acc.append(accepted)
            if not accepted:
                continue
            maps = [None, None]
            for t in (1, 0):                                                   # j first, like slam.py:179-180
                if ed["grid"][t] is not None:
                    ts = torch.tensor([[16 * ed["grid"][t][0], 16 * ed["grid"][t][1]]])
                    maps[t] = model.head_pts([ed["feat"][t]] + [x[:, 1:, :].float() for x in ed["dec"][t]], ts)
            for t, tag in enumerate("ij"):
                if maps[t] is None:
                    continue
                cf, dp = maps[t]["conf"][0], maps[t]["pts3d"][0, ..., 2]
                res[f"confs_{tag}_e{e}"] = cf.numpy()[::sub, ::sub].copy()
                res[f"depths_{tag}_e{e}"] = dp.numpy()[::sub, ::sub].copy()
                res[f"confs_l2_{tag}_e{e}"] = np.sqrt((cf.double().numpy() ** 2).sum())
                res[f"depths_l2_{tag}_e{e}"] = np.sqrt((dp.double().numpy() ** 2).sum())
            if maps[0] is not None and maps[1] is not None and ed["grid"][0] == ed["grid"][1]:
                pcls = torch.cat([maps[0]["pts3d"], maps[1]["pts3d"]], dim=0)         # [ij, ji] (slam.py:182)
                confs = torch.cat([maps[0]["conf"], maps[1]["conf"]], dim=0)
                res[f"intri_e{e}"] = su.estimate_intrinsic_from_pts3d(pcls, confs, shared_intrinsic=True).numpy()
        res["accepted"] = np.array(acc)
        meta = dict(k=k, sub=sub, seed=sd_seed, qk_gain=qk_gain)
        res["meta_keys"] = np.array(list(meta.keys())); res["meta_vals"] = np.array([float(v) for v in meta.values()], dtype=np.float64)
        print(f"[rvt] {name}: thres {thres:.4f} (margin {picked[1]:.3f}) accepted {acc}", flush=True)
        return res
    finally:
        torch.set_num_threads(threads)


def check_mixtures(fixtures):
    """The conditions on the three fixtures TAKEN TOGETHER (asserted here and in tests/test_regress_tokens_cpu.py): `fixtures` = dicts
    with adjacent / accepted / conf / thres / win_i / win_j."""
    rejected = accepted = False
    mixtures = set()
    for g in fixtures:
        for e in range(len(g["accepted"])):
            assert abs(float(g["conf"][e]) - float(g["thres"])) >= THRES_MARGIN, (e, float(g["conf"][e]), float(g["thres"]))
            if not g["adjacent"][e]:
                rejected |= not g["accepted"][e]
                accepted |= bool(g["accepted"][e])
            if g["accepted"][e]:
                mixtures.add(tuple(sorted((kind(g["win_i"][e]), kind(g["win_j"][e])))))
    assert rejected and accepted, "a non-adjacent edge rejected and a non-adjacent edge accepted"
    assert mixtures == {("win", "win"), ("idx", "win"), ("idx", "idx")}, mixtures


def write_case(name, out_dir=OUT):
    t0 = time.time()
    res = build_case(name)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"[rvt] {name}: {size / 1e6:.2f} MB in {time.time() - t0:.1f}s", flush=True)
    assert size <= (1 << 20), f"{path}: {size} bytes - raise sub (committed files stay below 1 MiB)"
    return path


if __name__ == "__main__":
    want = sys.argv[1:] or list(CASES)
    names = [n for n in CASES if n in want or CASES[n]["cfg"] in want]
    assert names, f"no case matches {want}; cases: {list(CASES)}"
    for n in names:
        write_case(n)
    have = [n for n in CASES if os.path.exists(os.path.join(OUT, f"{n}.npz"))]
    if len(have) == len(CASES):
        check_mixtures([dict(np.load(os.path.join(OUT, f"{n}.npz"))) for n in CASES])
        print("[rvt] mixtures, decisions and margins hold over the three fixtures", flush=True)
