"""Fixtures `tests/golden/decv_*.npz`: the REFERENCE model's `_decode_stereo` on batches whose ENTRIES have their own token counts.

TEST INFRASTRUCTURE, like tools/gen_golden_dect.py: needs the reference tree (oracle.ref_import), writes data only.  Batch entries of
`_decode_stereo` never interact, so the answer for entry b is the reference's call on that entry ALONE at B = 1 - that is what every
record below holds.  Weights and images are procedural (vista_slam_amd.weights): side t (0 = a, 1 = b) of entry b is the frame
synth_images(1, H, W, seed, tag 2 b + t), and its features are the reference's encoder on the selected tokens alone
(gen_golden_enct.encode_subset: patch_embed, gather, every block with the gathered positions) - what `forward_pairs_tokens` computes.

    python tools/gen_golden_decv.py              # every case (the full-architecture one takes a few minutes on a CPU)
    python tools/gen_golden_decv.py tiny         # the tiny cases / any list of case names

Each fixture records, with <t> in (a, b) = side (1, 2) and <b> the entry,
    n1 / n2                          [B] token counts of the two sides
    hw_a / hw_b                      [B, 2] frame sizes;  rect_a / rect_b [B, 2] the (h, w) of a side that is a row-major rectangle, else 0
    idx_<t>_e<b>, pos_<t>_e<b>       [n] token indices into the frame's row-major patch grid, [n, 2] the (y, x) positions fed
    feat_<t>_e<b>                    [n, E] the features fed (tiny cases only; the consumer of a full case encodes the subsets itself)
    dec1_hook<i>_e<b> / dec2_hook<i>_e<b>   the decoder list entries the heads read, pose row first, every tsub-th row ([::tsub])
    a_pose / a_pose_conf, b_*        [B, 4, 4] / [B] head_pose_s per side (the keys of dect_*)
    <t>_pts3d_e<b> / <t>_conf_e<b>   head_pts at the side's token shape (16 h, 16 w), every sub-th pixel of both axes, rectangles only
    ref_noise                        rel-L2 between the reference's own fp32 and fp64 last decoder layer (worst entry and side),
                                     asserted <= 1e-4; a case with `seed_from` takes the first seed from there upward that holds it
    alt_padded                       [B] rel-L2 between the last layer of entry b (both sides) and what the reference returns for it when
                                     every entry is ZERO-PADDED to the call's largest count per side (features 0, positions (0, 0)) and
                                     the batch is decoded unmasked: what a kernel that ignored the counts would compute.  Asserted
                                     >= 3e-3 (3 x the GPU parity bar) for every entry shorter than the maximum on either side.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vista_slam_amd import weights as W          # noqa: E402
from gen_golden_enct import encode_subset         # noqa: E402  (the reference's encoder on a token subset)

OUT = os.path.join(ROOT, "tests", "golden")
REF_NOISE_MAX = 1e-4
ALT_PADDED_MIN = 3e-3
torch.set_grad_enabled(False)


def _win(hp, wp, y0, x0, h, w):
    assert 0 <= y0 and y0 + h <= hp and 0 <= x0 and x0 + w <= wp
    return (np.arange(y0, y0 + h)[:, None] * wp + np.arange(x0, x0 + w)[None, :]).ravel()


def _perm(n, k, seed):
    return np.random.default_rng(seed).permutation(n)[:k]


# A side of an entry: ((H, W) of its frame, selection) with selection ("whole",) | ("win", (y0, x0, h, w)) | ("idx", index array).
# name -> cfg, Q/K gain, entries [(side a, side b)], token stride, pixel stride
CASES = {
    # counts (1, 64, 129, 12) / (65, 128, 63, 256): one token; the 64-key tile boundary from both sides on both sides; nq % 128 == 0
    # (pose blocks) next to nq % 128 != 0 (pose query in a spare row) in one launch; 256 keys = the last count that prefetches
    "decv_tiny_b4_edges": dict(cfg="tiny", tsub=3, sub=8, entries=[
        (((48, 64), ("idx", np.array([5]))), ((128, 160), ("idx", _perm(80, 65, 1)))),
        (((128, 128), ("idx", np.arange(63, -1, -1))), ((176, 192), ("idx", _perm(132, 128, 2)))),
        (((176, 192), ("idx", _perm(132, 129, 3))), ((128, 128), ("idx", np.delete(np.arange(64), 27)))),
        (((48, 64), ("whole",)), ((256, 256), ("whole",)))]),
    # windows 2 x 3, 3 x 5, 4 x 4 of a 5 x 6 grid against whole frames of 12, 30, 20 tokens: every side a rectangle (the DPT head is
    # compared), the tiny stress conditioning
    "decv_tiny_b3_win_sharp": dict(cfg="tiny", qk_gain=4.0, seed_from=43, entries=[
        (((80, 96), ("win", (1, 2, 2, 3))), ((48, 64), ("whole",))),
        (((80, 96), ("win", (2, 0, 3, 5))), ((80, 96), ("whole",))),
        (((80, 96), ("win", (0, 1, 4, 4))), ((64, 80), ("whole",)))]),
    # equal counts (12, 12) / (15, 15): the dect-style calls serve the same inputs
    "decv_tiny_b2_equal": dict(cfg="tiny", entries=[
        (((48, 64), ("whole",)), ((48, 80), ("whole",))),
        (((48, 64), ("whole",)), ((48, 80), ("whole",)))]),
    # full architecture, counts (196, 80) / (140, 196): a whole frame against a pruned set, a window against a whole frame
    "decv_full_224_b2": dict(cfg="full", tsub=11, sub=8, entries=[
        (((224, 224), ("whole",)), ((224, 224), ("idx", _perm(196, 140, 43)))),
        (((224, 224), ("win", (6, 4, 8, 10))), ((224, 224), ("whole",)))]),
}


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def side_selection(side):
    """-> ((H, W), idx [n] int64, rect (h, w) or None) of one side of one entry."""
    (H, W_), sel = side
    hp, wp = H // 16, W_ // 16
    if sel[0] == "whole":
        return (H, W_), np.arange(hp * wp, dtype=np.int64), (hp, wp)
    if sel[0] == "win":
        return (H, W_), _win(hp, wp, *sel[1]).astype(np.int64), (sel[1][2], sel[1][3])
    idx = np.asarray(sel[1]).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < hp * wp
    return (H, W_), idx, None


def counts(name):
    """([n1_b], [n2_b]) of a case, from the table alone."""
    e = CASES[name]["entries"]
    return [len(side_selection(a)[1]) for a, _ in e], [len(side_selection(b)[1]) for _, b in e]


def _grow_rope(model, top, dtype):
    # the reference's python RoPE indexes a reused cos / sin table with the call's minimum position as its origin: make the table
    # cover every position of the call, from 0, beforehand (the note in gen_golden_enct.encode_subset)
    model.rope(torch.zeros(1, 1, 2, 64, dtype=dtype), torch.tensor([[[0, 0], [top, top]]]))


def build_case(name, seed=None):
    """-> (dict of arrays, the fixture of case `name`).  Needs the reference tree."""
    from oracle.ref_import import load_reference_model
    c = CASES[name]
    cfg = W.TINY if c["cfg"] == "tiny" else W.FULL
    qk_gain, tsub, sub = c.get("qk_gain", 1.0), c.get("tsub", 1), c.get("sub", 1)
    sel = [(side_selection(a), side_selection(b)) for a, b in c["entries"]]
    B = len(sel)
    threads = torch.get_num_threads()
    if c["cfg"] == "tiny":
        torch.set_num_threads(1)          # the tiny fixtures regenerate bit for bit (tests/test_decode_varlen_cpu.py): one summation order
    try:
        seeds = [seed] if seed is not None else ([c["seed_from"] + i for i in range(8)] if "seed_from" in c else [43])
        for sd_seed in seeds:
            sd = W.state_dict(cfg, seed=sd_seed, qk_gain=qk_gain)
            model = load_reference_model(cfg, sd)
            model64 = load_reference_model(cfg, sd).double()
            feats, poss, decs, noise = [], [], [], 0.0
            for b, sides in enumerate(sel):
                fp = []
                for t, ((H, W_), idx, _rect) in enumerate(sides):
                    img = torch.from_numpy(W.synth_images(1, H, W_, seed=sd_seed, tag=2 * b + t).copy())
                    fp.append(encode_subset(model, img, H, W_, idx[None]))
                (fa, pa), (fb, pb) = fp
                top = int(max(pa.max(), pb.max()))
                _grow_rope(model, top, torch.float32)
                d1, d2 = model._decode_stereo(fa, fb, pa, pb)
                _grow_rope(model64, top, torch.float64)
                e1, e2 = model64._decode_stereo(fa.double(), fb.double(), pa, pb)
                noise = max(noise, rel_l2(d1[-1].numpy(), e1[-1].numpy()), rel_l2(d2[-1].numpy(), e2[-1].numpy()))
                feats.append((fa, fb)); poss.append((pa, pb)); decs.append((d1, d2))
            del model64
            print(f"[decv] {name}: seed {sd_seed} ref_noise {noise:.2e}", flush=True)
            if noise <= REF_NOISE_MAX:
                break
        assert noise <= REF_NOISE_MAX, f"{name}: the reference's own fp32-vs-fp64 distance {noise:.2e} exceeds {REF_NOISE_MAX:g}"
        n = [[f[t].shape[1] for f in feats] for t in range(2)]
        # what ignoring the counts would give: every entry zero-padded to the largest count of its side, one unmasked batch
        E = cfg.enc_embed_dim
        padf = [torch.zeros(B, max(n[t]), E) for t in range(2)]
        padp = [torch.zeros(B, max(n[t]), 2, dtype=poss[0][t].dtype) for t in range(2)]
        for b in range(B):
            for t in range(2):
                padf[t][b, :n[t][b]] = feats[b][t][0]
                padp[t][b, :n[t][b]] = poss[b][t][0]
        _grow_rope(model, int(max(padp[0].max(), padp[1].max())), torch.float32)
        q1, q2 = model._decode_stereo(padf[0], padf[1], padp[0], padp[1])
        last = cfg.hooks[-1] - 1
        alt = np.zeros(B)
        for b in range(B):
            got = np.concatenate([q1[last][b, :n[0][b] + 1].numpy(), q2[last][b, :n[1][b] + 1].numpy()])
            want = np.concatenate([decs[b][0][last][0].numpy(), decs[b][1][last][0].numpy()])
            alt[b] = rel_l2(got, want)
            short = n[0][b] < max(n[0]) or n[1][b] < max(n[1])
            print(f"[decv] {name}: entry {b} counts ({n[0][b]}, {n[1][b]}) alt_padded {alt[b]:.2e}{'' if short else ' (not padded)'}", flush=True)
            assert not short or alt[b] >= ALT_PADDED_MIN, f"{name}: entry {b}: padding moves the answer by {alt[b]:.2e} only - raise the Q/K gain or change the seed"
        res = {"n1": np.array(n[0], np.int64), "n2": np.array(n[1], np.int64),
               "hw_a": np.array([s[0][0] for s in sel], np.int64), "hw_b": np.array([s[1][0] for s in sel], np.int64),
               "rect_a": np.array([s[0][2] or (0, 0) for s in sel], np.int64), "rect_b": np.array([s[1][2] or (0, 0) for s in sel], np.int64)}
        poses = {"a": [], "b": []}
        for b in range(B):
            for t, tag in enumerate("ab"):
                (_hw, idx, rect), feat, pos, dec = sel[b][t], feats[b][t], poss[b][t], decs[b][t]
                res[f"idx_{tag}_e{b}"] = idx
                res[f"pos_{tag}_e{b}"] = pos[0].numpy().astype(np.int64)
                if c["cfg"] == "tiny":
                    res[f"feat_{tag}_e{b}"] = feat[0].numpy().copy()
                for hk in cfg.hooks[1:]:
                    res[f"dec{t + 1}_hook{hk - 1}_e{b}"] = dec[hk - 1][0].numpy()[::tsub].copy()
                poses[tag].append(model.head_pose_s(dec[-1][:, 0, :]))
                if rect is not None:
                    ts = torch.tensor([[16 * rect[0], 16 * rect[1]]])
                    pts = model.head_pts([feat] + [x[:, 1:, :].float() for x in dec], ts)
                    res[f"{tag}_pts3d_e{b}"] = pts["pts3d"].numpy()[0, ::sub, ::sub].copy()
                    res[f"{tag}_conf_e{b}"] = pts["conf"].numpy()[0, ::sub, ::sub].copy()
        for tag in "ab":
            res[f"{tag}_pose"] = np.concatenate([p["pose"].numpy() for p in poses[tag]]).copy()
            res[f"{tag}_pose_conf"] = np.concatenate([p["conf"].numpy() for p in poses[tag]]).copy()
        res["ref_noise"] = np.float64(noise)
        res["alt_padded"] = alt
        meta = dict(B=B, tsub=tsub, sub=sub, seed=sd_seed, qk_gain=qk_gain)
        res["meta_keys"] = np.array(list(meta.keys())); res["meta_vals"] = np.array([float(v) for v in meta.values()], dtype=np.float64)
        return res
    finally:
        torch.set_num_threads(threads)


def write_case(name, out_dir=OUT):
    t0 = time.time()
    res = build_case(name)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"[decv] {name}: {size / 1e6:.2f} MB in {time.time() - t0:.1f}s", flush=True)
    assert size <= (1 << 20), f"{path}: {size} bytes - raise tsub / sub (committed files stay below 1 MiB)"
    return path


if __name__ == "__main__":
    want = sys.argv[1:] or list(CASES)
    names = [n for n in CASES if n in want or CASES[n]["cfg"] in want]
    assert names, f"no case matches {want}; cases: {list(CASES)}"
    for n in names:
        write_case(n)
