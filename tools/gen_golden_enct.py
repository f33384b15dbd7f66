"""Fixtures `tests/golden/enct_*.npz`: the REFERENCE model's encoder on TOKEN SUBSETS - `patch_embed`, a gather of the patch
embeddings and their positions by an index array, then every encoder Block on the gathered tokens with the gathered positions
(sta_model.py:163-174; Block / XFormer_Attention take any token count and rotate q / k by the positions they are handed,
sta_blocks.py:129-148,166-169).

TEST INFRASTRUCTURE, like tools/gen_golden_dect.py: needs the reference tree (oracle.ref_import), writes data only.  Weights and
images are procedural (vista_slam_amd.weights): frame = synth_images(B, H, W, seed, tag 0); the pair case's second frame has tag 1.

    python tools/gen_golden_enct.py              # every case (the full-architecture ones take a minute or two each on a CPU)
    python tools/gen_golden_enct.py tiny         # the tiny cases / any list of case names

Each fixture records (the pair case: every key below with the suffix _a / _b, one per side)
    idx          [B, N] token indices into the frame (row-major patch grid): the selection
    pos          [B, N, 2] the gathered (y, x) grid positions: what names the patch and rotates q / k
    enc_feat     the encoder blocks on the subset, no final norm, every tsub-th token row ([:, ::tsub]; tiny cases: all rows)
    alt_enum     the same call with the positions replaced by the enumeration (0, t): what a route that ignored the positions
                 would rotate by.  Differs from enc_feat (except for ONE token: softmax over one key is 1 whatever the rotation)
    slice_full   the same rows of the WHOLE-frame encoding: what a route that encoded the frame and sliced would return.  Differs
                 from enc_feat except where all tokens are selected (attention is permutation-equivariant).  Left out where the
                 case says so (no_slice).
    ref_noise    rel-L2 between the reference's own fp32 and fp64 result (pair case: the largest of both encodings and both last
                 decoder layers), asserted <= 1e-4; a case with `seed_from` takes the first seed from there upward that holds it.
The pair case additionally records what `dect_*` records, computed from the two subset encodings: dec1_hook<i> / dec2_hook<i>,
a_pose / a_pose_conf, b_*, and <side>_pts3d / <side>_conf for a side that is a row-major rectangle.
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
torch.set_grad_enabled(False)


def _win(hp, wp, y0, x0, h, w):
    """Row-major token indices of the h x w window at (y0, x0) of an hp x wp grid."""
    assert 0 <= y0 and y0 + h <= hp and 0 <= x0 and x0 + w <= wp
    return (np.arange(y0, y0 + h)[:, None] * wp + np.arange(x0, x0 + w)[None, :]).ravel()


def _perm(n, k, seed):
    return lambda b: np.random.default_rng(seed + b).permutation(n)[:k]


# A selection: ("win", [(y0, x0, h, w) per batch entry]) | ("idx", f(b) -> index array).
# name -> cfg, frame (H, W), B, Q/K gain, selection, token stride
CASES = {
    # 4 x 5 grid, a 2 x 3 window at another place per entry: per-entry positions, N = 6
    "enct_tiny_win_b2": dict(cfg="tiny", hw=(64, 80), B=2, sel=("win", [(1, 2, 2, 3), (2, 0, 2, 3)])),
    # 7 of 12 tokens in arbitrary order, different per entry: no grid at all
    "enct_tiny_pruned_b2": dict(cfg="tiny", hw=(48, 64), B=2, sel=("idx", _perm(12, 7, 100))),
    # ONE token per entry (5 and 10), the tiny stress conditioning: N = 1, M = 2 rows
    "enct_tiny_one_sharp": dict(cfg="tiny", hw=(48, 64), B=2, qk_gain=4.0, seed_from=43, sel=("idx", lambda b: np.array([5, 10][b:b + 1]))),
    # all 64 tokens reversed: N = npad exactly, and the one case where the subset IS the (permuted) whole-frame encoding
    "enct_tiny_64_rev": dict(cfg="tiny", hw=(128, 128), B=1, sel=("idx", lambda b: np.arange(63, -1, -1))),
    # 128 of 132 permuted: N = npad with a next head and a next sequence; one full query block, two full key tiles
    "enct_tiny_128_of_132_b2": dict(cfg="tiny", hw=(176, 192), B=2, sel=("idx", _perm(132, 128, 200))),
    # 65 of 80 permuted: a one-key tail tile
    "enct_tiny_65_of_80": dict(cfg="tiny", hw=(160, 128), B=1, sel=("idx", _perm(80, 65, 300))),
    # 129 of 132 in grid order: a one-row second query block
    "enct_tiny_129_of_132": dict(cfg="tiny", hw=(176, 192), B=1, sel=("idx", lambda b: np.sort(np.random.default_rng(400).permutation(132)[:129]))),
    # full architecture: a prime count in permuted order, default conditioning and the gain-3 stress conditioning
    "enct_full_224_pruned_b1": dict(cfg="full", hw=(224, 224), B=1, sel=("idx", _perm(196, 131, 43)), tsub=7),
    "enct_full_224_pruned_sharp": dict(cfg="full", hw=(224, 224), B=1, qk_gain=3.0, seed_from=43, sel=("idx", _perm(196, 131, 43)), tsub=7),
    # the headline grid (24 x 32): 192 of 768, several query blocks and key tiles; the whole-frame slice is left out
    "enct_full_384x512_192": dict(cfg="full", hw=(384, 512), B=1, sel=("idx", _perm(768, 192, 500)), tsub=8, no_slice=True),
    # the pair: 9 of 20 pruned against the 2 x 3 window at (1, 1) of a 3 x 4 grid: encode the subsets, decode them, both heads
    "enct_tiny_pair_pruned_vs_win_b2": dict(cfg="tiny", hw=(64, 80), hw_b=(48, 64), B=2, sel=("idx", _perm(20, 9, 600)),
                                            sel_b=("win", [(1, 1, 2, 3), (1, 1, 2, 3)])),
}


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def selection(sel, B, hp, wp):
    """-> (idx [B, N] int64, rect (h, w) or None)."""
    if sel[0] == "win":
        wins = sel[1]
        assert len(wins) == B and len({(w[2], w[3]) for w in wins}) == 1
        return np.stack([_win(hp, wp, *w) for w in wins]).astype(np.int64), (wins[0][2], wins[0][3])
    return np.stack([np.asarray(sel[1](b)) for b in range(B)]).astype(np.int64), None


def enumeration(B, N):
    return np.stack([np.zeros((B, N), np.int64), np.broadcast_to(np.arange(N), (B, N))], -1)


def encode_subset(model, img, H, W_, idx, pos_override=None):
    """The reference computation: patch_embed, gather rows of x and pos, every encoder block.  -> (feat [B, N, E], pos [B, N, 2])."""
    B = img.shape[0]
    x, pos = model.patch_embed(img, true_shape=torch.tensor([[H, W_]] * B))
    ix = torch.from_numpy(idx)
    x = torch.gather(x, 1, ix[:, :, None].expand(-1, -1, x.shape[2])).contiguous()
    pos = torch.gather(pos, 1, ix[:, :, None].expand(-1, -1, 2)).contiguous()
    rot = pos if pos_override is None else torch.from_numpy(pos_override)
    # The reference's python RoPE keeps ONE cos / sin table per dtype and indexes a reused table with the CALL's minimum position as
    # its origin (pos_embed.py:135-159).  Reused consistently that is a uniform shift of q and k - harmless, RoPE is relative - but a
    # subset whose smallest y or x is not 0 can have the table rebuilt between the rotation of q and the rotation of k of the first
    # layer, and then rotates the two by different origins: a result that depends on what the module ran before.  The fixture pins
    # the rotation the code intends (sta_blocks.py:134-137): make the table cover every position of the call, from 0, beforehand.
    top = int(rot.max())
    model.rope(torch.zeros(1, 1, 2, 64, dtype=x.dtype), torch.tensor([[[0, 0], [top, top]]]))
    for blk in model.enc_blocks:
        x = blk(x, rot)
    return x, pos


def build_side(model, model64, img, H, W_, idx, tsub, no_slice):
    """One frame's records -> (dict without suffix, feat, pos, noise)."""
    B, N = idx.shape
    feat, pos = encode_subset(model, img, H, W_, idx)
    f64, _ = encode_subset(model64, img.double(), H, W_, idx)
    noise = rel_l2(feat.numpy(), f64.numpy())
    alt, _ = encode_subset(model, img, H, W_, idx, enumeration(B, N))
    res = {"idx": idx, "pos": pos.numpy().astype(np.int64), "enc_feat": feat.numpy()[:, ::tsub].copy(), "alt_enum": alt.numpy()[:, ::tsub].copy()}
    if not no_slice:
        full, _ = model._encode_image(img, torch.tensor([[H, W_]] * B), normalize=False)
        ix = torch.from_numpy(idx)
        res["slice_full"] = torch.gather(full, 1, ix[:, :, None].expand(-1, -1, full.shape[2])).numpy()[:, ::tsub].copy()
    return res, feat, pos, noise


def build_case(name, seed=None):
    """-> (dict of arrays, the fixture of case `name`).  Needs the reference tree."""
    from oracle.ref_import import load_reference_model
    c = CASES[name]
    cfg = W.TINY if c["cfg"] == "tiny" else W.FULL
    (H, W_), B = c["hw"], c["B"]
    qk_gain, tsub, no_slice, pair = c.get("qk_gain", 1.0), c.get("tsub", 1), c.get("no_slice", False), "sel_b" in c
    idx, rect = selection(c["sel"], B, H // 16, W_ // 16)
    threads = torch.get_num_threads()
    if c["cfg"] == "tiny":
        torch.set_num_threads(1)          # the tiny fixtures regenerate bit for bit (tests/test_encode_tokens_cpu.py): one summation order
    try:
        seeds = [seed] if seed is not None else ([c["seed_from"] + i for i in range(8)] if "seed_from" in c else [43])
        for sd_seed in seeds:
            sd = W.state_dict(cfg, seed=sd_seed, qk_gain=qk_gain)
            model = load_reference_model(cfg, sd)
            model64 = load_reference_model(cfg, sd).double()
            img = torch.from_numpy(W.synth_images(B, H, W_, seed=sd_seed, tag=0).copy())
            ra, fa, pa, noise = build_side(model, model64, img, H, W_, idx, tsub, no_slice)
            if pair:
                Hb, Wb = c["hw_b"]
                idx_b, rect_b = selection(c["sel_b"], B, Hb // 16, Wb // 16)
                img_b = torch.from_numpy(W.synth_images(B, Hb, Wb, seed=sd_seed, tag=1).copy())
                rb, fb, pb, noise_b = build_side(model, model64, img_b, Hb, Wb, idx_b, tsub, no_slice)
                d1, d2 = model._decode_stereo(fa, fb, pa, pb)
                e1, e2 = model64._decode_stereo(fa.double(), fb.double(), pa, pb)
                noise = max(noise, noise_b, rel_l2(d1[-1].numpy(), e1[-1].numpy()), rel_l2(d2[-1].numpy(), e2[-1].numpy()))
            del model64
            print(f"[enct] {name}: seed {sd_seed} ref_noise {noise:.2e}", flush=True)
            if noise <= REF_NOISE_MAX:
                break
        assert noise <= REF_NOISE_MAX, f"{name}: the reference's own fp32-vs-fp64 distance {noise:.2e} exceeds {REF_NOISE_MAX:g}"
        meta = dict(H=H, W=W_, B=B, tsub=tsub, sub=1, seed=sd_seed, qk_gain=qk_gain, rect_h=rect[0] if rect else 0, rect_w=rect[1] if rect else 0)
        if not pair:
            res = dict(ra)
            print(f"[enct] {name}: positions matter {rel_l2(res['alt_enum'], res['enc_feat']):.2e}"
                  + ("" if no_slice else f", subset vs slice of the frame {rel_l2(res['slice_full'], res['enc_feat']):.2e}"), flush=True)
        else:
            res = {f"{k}_a": v for k, v in ra.items()}
            res.update({f"{k}_b": v for k, v in rb.items()})
            for tag in "ab":
                print(f"[enct] {name}: side {tag}: positions matter {rel_l2(res[f'alt_enum_{tag}'], res[f'enc_feat_{tag}']):.2e}, "
                      f"subset vs slice of the frame {rel_l2(res[f'slice_full_{tag}'], res[f'enc_feat_{tag}']):.2e}", flush=True)
            for hk in cfg.hooks[1:]:
                res[f"dec1_hook{hk - 1}"] = d1[hk - 1].numpy()[:, ::tsub].copy()
                res[f"dec2_hook{hk - 1}"] = d2[hk - 1].numpy()[:, ::tsub].copy()
            for tag, feat, dec, rc in (("a", fa, d1, rect), ("b", fb, d2, rect_b)):
                pose = model.head_pose_s(dec[-1][:, 0, :])
                res[f"{tag}_pose"] = pose["pose"].numpy().copy()
                res[f"{tag}_pose_conf"] = pose["conf"].numpy().copy()
                if rc is not None:
                    ts = torch.tensor([[16 * rc[0], 16 * rc[1]]] * B)
                    pts = model.head_pts([feat] + [t[:, 1:, :].float() for t in dec], ts)
                    res[f"{tag}_pts3d"] = pts["pts3d"].numpy().copy()
                    res[f"{tag}_conf"] = pts["conf"].numpy().copy()
            meta.update(Hb=Hb, Wb=Wb, rect_bh=rect_b[0] if rect_b else 0, rect_bw=rect_b[1] if rect_b else 0)
        res["ref_noise"] = np.float64(noise)
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
    print(f"[enct] {name}: {size / 1e6:.2f} MB in {time.time() - t0:.1f}s", flush=True)
    assert size <= (1 << 20), f"{path}: {size} bytes - raise tsub (committed files stay below 1 MiB)"
    return path


if __name__ == "__main__":
    sel = sys.argv[1:] or list(CASES)
    names = [n for n in CASES if n in sel or CASES[n]["cfg"] in sel]
    assert names, f"no case matches {sel}; cases: {list(CASES)}"
    for n in names:
        write_case(n)
