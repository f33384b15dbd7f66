"""Fixtures `tests/golden/decn_*.npz`: the REFERENCE model on view pairs of DIFFERENT resolution (N1 != N2 patch tokens).

TEST INFRASTRUCTURE, like oracle/gen_golden.py: needs the reference tree (oracle.ref_import), writes data only.  Weights and images
are procedural (vista_slam_amd.weights): side a = synth_images(B, Ha, Wa, seed, tag 0), side b = synth_images(B, Hb, Wb, seed, tag 1).

    python tools/gen_golden_decn.py              # every case (the full-architecture ones take a minute or two each on a CPU)
    python tools/gen_golden_decn.py tiny         # the tiny cases / any list of case names

Each fixture records
    enc_feat_a / enc_feat_b        encoder features (tiny cases only; the consumer of a full case encodes the procedural pair itself)
    dec1_hook<i> / dec2_hook<i>    _decode_stereo(a, b): the decoder list entries the heads read, pose row included, every
                                   tsub-th token row ([:, ::tsub]: row 0 = the pose token is always in)
    a_* / b_*                      pts3d / conf of head_pts (every sub-th pixel of both axes, [:, ::sub, ::sub]; a portrait side as
                                   the reference returns it: transposed) and pose / pose_conf of head_pose_s, per side
    swap_dec1_last / swap_dec2_last   _decode_stereo(b, a): its last list entry per side.  The reference treats the two sides alike,
                                   so swap_dec1_last == dec2_hook<last> and swap_dec2_last == dec1_hook<last> BIT FOR BIT
    ref_noise                      rel-L2 between the reference's own fp32 and fp64 last decoder layer (the larger of the two sides):
                                   how well the answer is defined.  Asserted <= 1e-4 (a tenth of the project's parity bar); a case with
                                   `seed_from` takes the first seed from there upward that holds it.
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

# name -> cfg, (Ha, Wa), (Hb, Wb), B, Q/K gain, token stride, pixel stride
CASES = {
    "decn_tiny_48x64_vs_48x80_b2": dict(cfg="tiny", a=(48, 64), b=(48, 80), B=2),                        # 12 / 15 tokens, batch > 1
    "decn_tiny_64x48_vs_32x32": dict(cfg="tiny", a=(64, 48), b=(32, 32), B=1),                           # portrait 12 / 4: a very short side
    "decn_tiny_48x80_vs_32x48_sharp": dict(cfg="tiny", a=(48, 80), b=(32, 48), B=1, qk_gain=4.0, seed_from=43),   # 15 / 6, the tiny stress conditioning
    "decn_full_224_vs_224x160_b1": dict(cfg="full", a=(224, 224), b=(224, 160), B=1, tsub=5, sub=8),     # 196 / 140: both spare-row pose, 4 vs 3 key tiles
    "decn_full_256_vs_224_b1": dict(cfg="full", a=(256, 256), b=(224, 224), B=1, tsub=7, sub=8),         # 256 / 196: side workgroups vs spare row
    "decn_full_384x512_vs_224_b1": dict(cfg="full", a=(384, 512), b=(224, 224), B=1, tsub=13, sub=16),   # 768 / 196: 12 vs 4 key tiles
}


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def build_case(name, seed=None):
    """-> (dict of arrays, the fixture of case `name`).  Needs the reference tree."""
    from oracle.ref_import import load_reference_model
    c = CASES[name]
    cfg = W.TINY if c["cfg"] == "tiny" else W.FULL
    (Ha, Wa), (Hb, Wb), B = c["a"], c["b"], c["B"]
    qk_gain, tsub, sub = c.get("qk_gain", 1.0), c.get("tsub", 1), c.get("sub", 1)
    threads = torch.get_num_threads()
    if c["cfg"] == "tiny":
        torch.set_num_threads(1)          # the tiny fixtures regenerate bit for bit (tests/test_decode_mixed_cpu.py): one summation order
    try:
        seeds = [seed] if seed is not None else ([c["seed_from"] + i for i in range(8)] if "seed_from" in c else [43])
        for sd_seed in seeds:
            sd = W.state_dict(cfg, seed=sd_seed, qk_gain=qk_gain)
            model = load_reference_model(cfg, sd)
            img_a = torch.from_numpy(W.synth_images(B, Ha, Wa, seed=sd_seed, tag=0).copy())
            img_b = torch.from_numpy(W.synth_images(B, Hb, Wb, seed=sd_seed, tag=1).copy())
            ts_a, ts_b = torch.tensor([[Ha, Wa]] * B), torch.tensor([[Hb, Wb]] * B)
            fa, pa = model._encode_image(img_a, ts_a, normalize=False)
            fb, pb = model._encode_image(img_b, ts_b, normalize=False)
            d1, d2 = model._decode_stereo(fa, fb, pa, pb)
            model64 = load_reference_model(cfg, sd).double()
            e1, e2 = model64._decode_stereo(fa.double(), fb.double(), pa, pb)
            noise = max(rel_l2(d1[-1].numpy(), e1[-1].numpy()), rel_l2(d2[-1].numpy(), e2[-1].numpy()))
            del model64, e1, e2
            print(f"[decn] {name}: seed {sd_seed} ref_noise {noise:.2e}", flush=True)
            if noise <= REF_NOISE_MAX:
                break
        assert noise <= REF_NOISE_MAX, f"{name}: the reference's own fp32-vs-fp64 distance {noise:.2e} exceeds {REF_NOISE_MAX:g}"
        s1, s2 = model._decode_stereo(fb, fa, pb, pa)
        res = {}
        if tsub == 1:
            res["enc_feat_a"] = fa.numpy(); res["enc_feat_b"] = fb.numpy()
        last = cfg.hooks[-1] - 1
        for hk in cfg.hooks[1:]:
            res[f"dec1_hook{hk - 1}"] = d1[hk - 1].numpy()[:, ::tsub].copy()
            res[f"dec2_hook{hk - 1}"] = d2[hk - 1].numpy()[:, ::tsub].copy()
        res["swap_dec1_last"] = s1[last].numpy()[:, ::tsub].copy()
        res["swap_dec2_last"] = s2[last].numpy()[:, ::tsub].copy()
        for tag, feat, dec, ts in (("a", fa, d1, ts_a), ("b", fb, d2, ts_b)):
            pts = model.head_pts([feat] + [t[:, 1:, :].float() for t in dec], ts)
            pose = model.head_pose_s(dec[-1][:, 0, :])
            res[f"{tag}_pts3d"] = pts["pts3d"].numpy()[:, ::sub, ::sub].copy()
            res[f"{tag}_conf"] = pts["conf"].numpy()[:, ::sub, ::sub].copy()
            res[f"{tag}_pose"] = pose["pose"].numpy().copy()
            res[f"{tag}_pose_conf"] = pose["conf"].numpy().copy()
        res["ref_noise"] = np.float64(noise)
        meta = dict(Ha=Ha, Wa=Wa, Hb=Hb, Wb=Wb, B=B, tsub=tsub, sub=sub, seed=sd_seed, qk_gain=qk_gain)
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
    print(f"[decn] {name}: {size / 1e6:.2f} MB in {time.time() - t0:.1f}s", flush=True)
    assert size <= (1 << 20), f"{path}: {size} bytes - raise tsub / sub (committed files stay below 1 MiB)"
    return path


if __name__ == "__main__":
    sel = sys.argv[1:] or list(CASES)
    names = [n for n in CASES if n in sel or CASES[n]["cfg"] in sel]
    assert names, f"no case matches {sel}; cases: {list(CASES)}"
    for n in names:
        write_case(n)
