"""Fixtures `tests/golden/encv_*.npz`: the REFERENCE model's encoder on batches whose ENTRIES differ in token count and frame size.

TEST INFRASTRUCTURE, like tools/gen_golden_decv.py: needs the reference tree (oracle.ref_import), writes data only.  Batch entries of
the encoder never interact (attention is per sample), so the answer for entry b is the reference's computation on that entry ALONE
at B = 1 (gen_golden_enct.encode_subset: patch_embed, gather, every Block with the gathered positions) - that is what every record
below holds.  Weights and images are procedural (vista_slam_amd.weights): entry b is the frame synth_images(1, H, W, seed, tag b).

    python tools/gen_golden_encv.py              # every case (the full-architecture ones take a few minutes on a CPU)
    python tools/gen_golden_encv.py tiny         # the tiny cases / any list of case names

Each fixture records, with <b> the entry,
    n                 [B] token counts;  hw [B, 2] frame sizes
    idx_e<b>          [n] token indices into the entry's own row-major patch grid: the selection
    pos_e<b>          [n, 2] the gathered (y, x) grid positions: what names the patch and rotates q / k
    enc_feat_e<b>     the encoder blocks on the subset, no final norm, every tsub-th token row ([::tsub]; tiny cases: all rows)
    alt_enum_e<b>     the same call with the positions replaced by the enumeration (0, t), every (tsub * asub)-th row: what a route that
                      ignored the positions would rotate by.  Differs from enc_feat except for an entry of ONE token
    ref_noise         rel-L2 between the reference's own fp32 and fp64 result over the worst entry, asserted <= 1e-4; a case with
                      `seed_from` takes the first seed from there upward that holds it
    alt_padded        [B] rel-L2 between entry b and what the reference returns for it when its patch embeddings are ZERO-PADDED to
                      the call's largest count (embeddings 0, positions (0, 0)) and encoded unmasked: what a kernel that ignored
                      the counts would compute.  Asserted >= 3e-3 (3 x the GPU parity bar) for every entry shorter than the maximum.
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
from gen_golden_enct import encode_subset, enumeration         # noqa: E402  (the reference's encoder on a token subset)
import gen_golden_decv as DECV                    # noqa: E402  (the table of decv_tiny_b4_edges, side_selection)

OUT = os.path.join(ROOT, "tests", "golden")
REF_NOISE_MAX = 1e-4
ALT_PADDED_MIN = 3e-3
torch.set_grad_enabled(False)

_EDGES = [side for pair in DECV.CASES["decv_tiny_b4_edges"]["entries"] for side in pair]      # counts 1, 65, 64, 128, 129, 63, 12, 256

# An entry: ((H, W) of its frame, selection) with selection ("whole",) | ("win", (y0, x0, h, w)) | ("idx", index array).
# name -> cfg, Q/K gain, entries, token stride of enc_feat, extra stride of alt_enum
CASES = {
    # one token; the 64-key tile boundary from both sides; a one-row second query block; exact multiples of 64 (n == npad of a call
    # on the entry alone); 256 keys = the last count that prefetches; frames 48x64 .. 256x256
    "encv_tiny_b8_edges": dict(cfg="tiny", entries=_EDGES),
    "encv_tiny_b8_edges_sharp": dict(cfg="tiny", qk_gain=4.0, seed_from=43, entries=_EDGES),
    # equal counts and frames: one sta_encode_tokens call at B = 3 serves the same inputs
    "encv_tiny_b3_equal": dict(cfg="tiny", entries=[((48, 64), ("whole",))] * 3),
    # full architecture: a whole frame, a prime count in permuted order, a window, one token
    "encv_full_224_b4": dict(cfg="full", tsub=3, asub=2, entries=[
        ((224, 224), ("whole",)), ((224, 224), ("idx", DECV._perm(196, 131, 43))),
        ((224, 224), ("win", (6, 4, 8, 10))), ((224, 224), ("idx", np.array([97])))]),
    # two frame sizes in one call, the gain-3 stress conditioning
    "encv_full_mixed_frames_sharp": dict(cfg="full", qk_gain=3.0, seed_from=43, tsub=3, asub=2, entries=[
        ((224, 224), ("idx", DECV._perm(196, 140, 43))), ((384, 512), ("idx", DECV._perm(768, 192, 500)))]),
}


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def counts(name):
    """[n_b] of a case, from the table alone."""
    return [len(DECV.side_selection(e)[1]) for e in CASES[name]["entries"]]


def encode_padded(model, img, H, W_, idx, nmax):
    """Entry's gathered patch embeddings zero-padded to nmax tokens at position (0, 0), every Block unmasked -> its first n rows."""
    x, pos = model.patch_embed(img, true_shape=torch.tensor([[H, W_]]))
    ix = torch.from_numpy(idx)
    n = ix.shape[1]
    xp = torch.zeros(1, nmax, x.shape[2], dtype=x.dtype)
    pp = torch.zeros(1, nmax, 2, dtype=pos.dtype)
    xp[:, :n] = torch.gather(x, 1, ix[:, :, None].expand(-1, -1, x.shape[2]))
    pp[:, :n] = torch.gather(pos, 1, ix[:, :, None].expand(-1, -1, 2))
    top = int(pp.max())
    model.rope(torch.zeros(1, 1, 2, 64, dtype=x.dtype), torch.tensor([[[0, 0], [top, top]]]))      # see gen_golden_enct.encode_subset
    for blk in model.enc_blocks:
        xp = blk(xp, pp)
    return xp[:, :n]


def build_case(name, seed=None):
    """-> (dict of arrays, the fixture of case `name`).  Needs the reference tree."""
    from oracle.ref_import import load_reference_model
    c = CASES[name]
    cfg = W.TINY if c["cfg"] == "tiny" else W.FULL
    qk_gain, tsub, asub = c.get("qk_gain", 1.0), c.get("tsub", 1), c.get("asub", 1)
    sel = [DECV.side_selection(e) for e in c["entries"]]
    B = len(sel)
    nmax = max(len(s[1]) for s in sel)
    threads = torch.get_num_threads()
    if c["cfg"] == "tiny":
        torch.set_num_threads(1)          # the tiny fixtures regenerate bit for bit (tests/test_encode_varlen_cpu.py): one summation order
    try:
        seeds = [seed] if seed is not None else ([c["seed_from"] + i for i in range(8)] if "seed_from" in c else [43])
        for sd_seed in seeds:
            sd = W.state_dict(cfg, seed=sd_seed, qk_gain=qk_gain)
            model = load_reference_model(cfg, sd)
            model64 = load_reference_model(cfg, sd).double()
            imgs, feats, poss, noise = [], [], [], 0.0
            for b, ((H, W_), idx, _rect) in enumerate(sel):
                img = torch.from_numpy(W.synth_images(1, H, W_, seed=sd_seed, tag=b).copy())
                f, p = encode_subset(model, img, H, W_, idx[None])
                f64, _ = encode_subset(model64, img.double(), H, W_, idx[None])
                noise = max(noise, rel_l2(f.numpy(), f64.numpy()))
                imgs.append(img); feats.append(f); poss.append(p)
            del model64
            print(f"[encv] {name}: seed {sd_seed} ref_noise {noise:.2e}", flush=True)
            if noise <= REF_NOISE_MAX:
                break
        assert noise <= REF_NOISE_MAX, f"{name}: the reference's own fp32-vs-fp64 distance {noise:.2e} exceeds {REF_NOISE_MAX:g}"
        res = {"n": np.array([len(s[1]) for s in sel], np.int64), "hw": np.array([s[0] for s in sel], np.int64)}
        alt_padded = np.zeros(B)
        for b, ((H, W_), idx, _rect) in enumerate(sel):
            n = len(idx)
            alt, _ = encode_subset(model, imgs[b], H, W_, idx[None], enumeration(1, n))
            res[f"idx_e{b}"] = idx
            res[f"pos_e{b}"] = poss[b][0].numpy().astype(np.int64)
            res[f"enc_feat_e{b}"] = feats[b][0].numpy()[::tsub].copy()
            res[f"alt_enum_e{b}"] = alt[0].numpy()[::tsub * asub].copy()
            moved = rel_l2(res[f"alt_enum_e{b}"], res[f"enc_feat_e{b}"][::asub])
            if n < nmax:
                alt_padded[b] = rel_l2(encode_padded(model, imgs[b], H, W_, idx[None], nmax)[0].numpy(), feats[b][0].numpy())
            print(f"[encv] {name}: entry {b} frame {H}x{W_} count {n}: positions matter {moved:.2e}, alt_padded {alt_padded[b]:.2e}"
                  f"{'' if n < nmax else ' (not padded)'}", flush=True)
            assert n == nmax or alt_padded[b] >= ALT_PADDED_MIN, f"{name}: entry {b}: padding moves the answer by {alt_padded[b]:.2e} only - change the seed or the selection"
        res["ref_noise"] = np.float64(noise)
        res["alt_padded"] = alt_padded
        meta = dict(B=B, tsub=tsub, asub=asub, seed=sd_seed, qk_gain=qk_gain)
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
    print(f"[encv] {name}: {size / 1e6:.2f} MB in {time.time() - t0:.1f}s", flush=True)
    assert size <= (1 << 20), f"{path}: {size} bytes - raise tsub / asub (committed files stay below 1 MiB)"
    return path


if __name__ == "__main__":
    want = sys.argv[1:] or list(CASES)
    names = [n for n in CASES if n in want or CASES[n]["cfg"] in want]
    assert names, f"no case matches {want}; cases: {list(CASES)}"
    for n in names:
        write_case(n)
