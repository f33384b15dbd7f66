"""Fixtures `tests/golden/dect_*.npz`: the REFERENCE model's `_decode_stereo` on TOKEN SUBSETS - caller positions together with
unequal token counts (a rectangular window of one view against the whole other view, a pruned token set, one token).

TEST INFRASTRUCTURE, like tools/gen_golden_decn.py: needs the reference tree (oracle.ref_import), writes data only.  Weights and
images are procedural (vista_slam_amd.weights): frame a = synth_images(B, Ha, Wa, seed, tag 0), frame b = synth_images(B, Hb, Wb,
seed, tag 1).  Both frames are encoded WHOLE; a side is then a gather of its frame's tokens and positions by an index array.

    python tools/gen_golden_dect.py              # every case (the full-architecture ones take a minute or two each on a CPU)
    python tools/gen_golden_dect.py tiny         # the tiny cases / any list of case names

Each fixture records
    idx_a / idx_b                  [B, Nx] token indices into the side's frame (row-major patch grid): the selection
    pos_a / pos_b                  [B, Nx, 2] the (y, x) positions actually fed (the gathered grid positions + the case's offset)
    enc_feat_a / enc_feat_b        encoder features of the WHOLE frames (tiny cases only; the consumer of a full case encodes the
                                   procedural pair itself)
    dec1_hook<i> / dec2_hook<i>    _decode_stereo on the subsets: the decoder list entries the heads read, pose row included, every
                                   tsub-th token row ([:, ::tsub]: row 0 = the pose token is always in)
    swap_dec1_last / swap_dec2_last   _decode_stereo with the sides exchanged: swap_dec1_last == dec2_hook<last> and swap_dec2_last ==
                                   dec1_hook<last> BIT FOR BIT
    a_pose / a_pose_conf, b_*      head_pose_s per side
    a_pts3d / a_conf, b_*          head_pts at the side's token shape (16 h, 16 w), every sub-th pixel of both axes - only for a side
                                   that is a rectangle in row-major order (a window or the whole frame)
    alt_dec1_last                  the same call with side 1's positions made zero-based, i.e. what a route that ignored the
                                   caller's positions would rotate by: the window's own grid (positions minus the window origin) for
                                   a rectangle, the enumeration (0, t) for a set without a grid.  It must differ from dec1_hook<last>.
    ref_noise                      rel-L2 between the reference's own fp32 and fp64 last decoder layer (the larger of the two sides),
                                   asserted <= 1e-4; a case with `seed_from` takes the first seed from there upward that holds it.
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


def _pruned_7_of_12(b):
    return np.random.default_rng(100 + b).permutation(12)[:7]


# A side: ("whole",) | ("win", [(y0, x0, h, w) per batch entry]) | ("idx", f(b) -> index array [, (dy, dx) added to the positions]).
# name -> cfg, frames (Ha, Wa) / (Hb, Wb), B, Q/K gain, the two sides, token stride, pixel stride
CASES = {
    # 4 x 5 grid, 2 x 3 windows at another place per entry (N1 = 6) against 12 tokens: side 2's table offset with N1 != N2 and B > 1
    "dect_tiny_win_vs_full_b2": dict(cfg="tiny", a=(64, 80), b=(48, 64), B=2, sa=("win", [(1, 2, 2, 3), (2, 0, 2, 3)]), sb=("whole",)),
    # the same windows against 7 of the 12 tokens in arbitrary order, different per entry: no grid on either side
    "dect_tiny_win_vs_pruned_b2": dict(cfg="tiny", a=(64, 80), b=(48, 64), B=2, sa=("win", [(1, 2, 2, 3), (2, 0, 2, 3)]),
                                       sb=("idx", _pruned_7_of_12)),
    # ONE token at its grid position + 30 (pos_max beyond any grid: the RoPE table grows) against 12, the tiny stress conditioning
    "dect_tiny_one_vs_full_sharp": dict(cfg="tiny", a=(48, 64), b=(48, 64), B=2, qk_gain=4.0, seed_from=43,
                                        sa=("idx", lambda b: np.array([5, 10][b:b + 1]), (30, 30)), sb=("whole",)),
    # 64 tokens reversed against 63 (token 27 dropped): 65 and 64 rows with the pose token - the two sides of the npad boundary
    "dect_tiny_63_vs_64": dict(cfg="tiny", a=(128, 128), b=(128, 128), B=1, sa=("idx", lambda b: np.arange(63, -1, -1)),
                               sb=("idx", lambda b: np.delete(np.arange(64), 27))),
    # full architecture: an 8 x 10 window at (6, 4) of the 14 x 14 grid against 196 tokens; its point map is 128 x 160
    "dect_full_224_win_vs_full_sharp": dict(cfg="full", a=(224, 224), b=(224, 224), B=1, qk_gain=3.0, seed_from=43,
                                            sa=("win", [(6, 4, 8, 10)]), sb=("whole",), tsub=7, sub=8),
    # a prime count in permuted order against all tokens reversed, default conditioning
    "dect_full_224_pruned_b1": dict(cfg="full", a=(224, 224), b=(224, 224), B=1,
                                    sa=("idx", lambda b: np.random.default_rng(43).permutation(196)[:131]),
                                    sb=("idx", lambda b: np.arange(195, -1, -1)), tsub=7, sub=8),
}


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def side_selection(side, B, hp, wp):
    """-> (idx [B, K] int64, offset (dy, dx), rect (h, w) or None) of one side of a case."""
    if side[0] == "whole":
        return np.broadcast_to(np.arange(hp * wp), (B, hp * wp)).astype(np.int64).copy(), (0, 0), (hp, wp)
    if side[0] == "win":
        wins = side[1]
        assert len(wins) == B and len({(w[2], w[3]) for w in wins}) == 1
        return np.stack([_win(hp, wp, *w) for w in wins]).astype(np.int64), (0, 0), (wins[0][2], wins[0][3])
    idx = np.stack([np.asarray(side[1](b)) for b in range(B)]).astype(np.int64)
    return idx, (side[2] if len(side) > 2 else (0, 0)), None


def zero_based(pos, rect):
    """Side 1's positions as a route that ignored the caller's would make them (alt_dec1_last)."""
    if rect is not None:
        return pos - pos.min(axis=1, keepdims=True)
    B, K, _ = pos.shape
    return np.stack([np.zeros((B, K), np.int64), np.broadcast_to(np.arange(K), (B, K))], -1)


def build_case(name, seed=None):
    """-> (dict of arrays, the fixture of case `name`).  Needs the reference tree."""
    from oracle.ref_import import load_reference_model
    c = CASES[name]
    cfg = W.TINY if c["cfg"] == "tiny" else W.FULL
    (Ha, Wa), (Hb, Wb), B = c["a"], c["b"], c["B"]
    qk_gain, tsub, sub = c.get("qk_gain", 1.0), c.get("tsub", 1), c.get("sub", 1)
    ia, off_a, rect_a = side_selection(c["sa"], B, Ha // 16, Wa // 16)
    ib, off_b, rect_b = side_selection(c["sb"], B, Hb // 16, Wb // 16)
    threads = torch.get_num_threads()
    if c["cfg"] == "tiny":
        torch.set_num_threads(1)          # the tiny fixtures regenerate bit for bit (tests/test_decode_tokens_cpu.py): one summation order
    try:
        seeds = [seed] if seed is not None else ([c["seed_from"] + i for i in range(8)] if "seed_from" in c else [43])
        for sd_seed in seeds:
            sd = W.state_dict(cfg, seed=sd_seed, qk_gain=qk_gain)
            model = load_reference_model(cfg, sd)
            img_a = torch.from_numpy(W.synth_images(B, Ha, Wa, seed=sd_seed, tag=0).copy())
            img_b = torch.from_numpy(W.synth_images(B, Hb, Wb, seed=sd_seed, tag=1).copy())
            Fa, Pa = model._encode_image(img_a, torch.tensor([[Ha, Wa]] * B), normalize=False)
            Fb, Pb = model._encode_image(img_b, torch.tensor([[Hb, Wb]] * B), normalize=False)

            def take(F, P, idx, off):
                ix = torch.from_numpy(idx)
                f = torch.gather(F, 1, ix[:, :, None].expand(-1, -1, F.shape[2])).contiguous()
                p = torch.gather(P, 1, ix[:, :, None].expand(-1, -1, 2)) + torch.tensor(off)
                return f, p.contiguous()
            fa, pa = take(Fa, Pa, ia, off_a)
            fb, pb = take(Fb, Pb, ib, off_b)
            d1, d2 = model._decode_stereo(fa, fb, pa, pb)
            model64 = load_reference_model(cfg, sd).double()
            e1, e2 = model64._decode_stereo(fa.double(), fb.double(), pa, pb)
            noise = max(rel_l2(d1[-1].numpy(), e1[-1].numpy()), rel_l2(d2[-1].numpy(), e2[-1].numpy()))
            del model64, e1, e2
            print(f"[dect] {name}: seed {sd_seed} ref_noise {noise:.2e}", flush=True)
            if noise <= REF_NOISE_MAX:
                break
        assert noise <= REF_NOISE_MAX, f"{name}: the reference's own fp32-vs-fp64 distance {noise:.2e} exceeds {REF_NOISE_MAX:g}"
        s1, s2 = model._decode_stereo(fb, fa, pb, pa)
        alt1, _ = model._decode_stereo(fa, fb, torch.from_numpy(zero_based(pa.numpy(), rect_a)), pb)
        res = {"idx_a": ia, "idx_b": ib, "pos_a": pa.numpy().astype(np.int64), "pos_b": pb.numpy().astype(np.int64)}
        if tsub == 1:
            res["enc_feat_a"] = Fa.numpy(); res["enc_feat_b"] = Fb.numpy()
        last = cfg.hooks[-1] - 1
        for hk in cfg.hooks[1:]:
            res[f"dec1_hook{hk - 1}"] = d1[hk - 1].numpy()[:, ::tsub].copy()
            res[f"dec2_hook{hk - 1}"] = d2[hk - 1].numpy()[:, ::tsub].copy()
        res["swap_dec1_last"] = s1[last].numpy()[:, ::tsub].copy()
        res["swap_dec2_last"] = s2[last].numpy()[:, ::tsub].copy()
        res["alt_dec1_last"] = alt1[last].numpy()[:, ::tsub].copy()
        print(f"[dect] {name}: positions matter {rel_l2(alt1[last].numpy(), d1[last].numpy()):.2e}", flush=True)
        for tag, feat, dec, rect in (("a", fa, d1, rect_a), ("b", fb, d2, rect_b)):
            pose = model.head_pose_s(dec[-1][:, 0, :])
            res[f"{tag}_pose"] = pose["pose"].numpy().copy()
            res[f"{tag}_pose_conf"] = pose["conf"].numpy().copy()
            if rect is not None:
                ts = torch.tensor([[16 * rect[0], 16 * rect[1]]] * B)
                pts = model.head_pts([feat] + [t[:, 1:, :].float() for t in dec], ts)
                res[f"{tag}_pts3d"] = pts["pts3d"].numpy()[:, ::sub, ::sub].copy()
                res[f"{tag}_conf"] = pts["conf"].numpy()[:, ::sub, ::sub].copy()
        res["ref_noise"] = np.float64(noise)
        meta = dict(Ha=Ha, Wa=Wa, Hb=Hb, Wb=Wb, B=B, tsub=tsub, sub=sub, seed=sd_seed, qk_gain=qk_gain,
                    rect_ah=rect_a[0] if rect_a else 0, rect_aw=rect_a[1] if rect_a else 0,
                    rect_bh=rect_b[0] if rect_b else 0, rect_bw=rect_b[1] if rect_b else 0)
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
    print(f"[dect] {name}: {size / 1e6:.2f} MB in {time.time() - t0:.1f}s", flush=True)
    assert size <= (1 << 20), f"{path}: {size} bytes - raise tsub / sub (committed files stay below 1 MiB)"
    return path


if __name__ == "__main__":
    sel = sys.argv[1:] or list(CASES)
    names = [n for n in CASES if n in sel or CASES[n]["cfg"] in sel]
    assert names, f"no case matches {sel}; cases: {list(CASES)}"
    for n in names:
        write_case(n)
