"""Fixture `tests/golden/dptv_tiny_b4_edges.npz`: the REFERENCE model's `head_pts` on eight rectangular sides of DIFFERENT shape - what
one `sta_head_pts_varlen` call must return for each of them.

TEST INFRASTRUCTURE, like tools/gen_golden_decv.py, whose format and machinery this is (a `decv_*` record of four pairs: the
reference's encoder on each window, `_decode_stereo` on each pair alone at B = 1, `head_pts` on each side alone at its own
(16 h, 16 w)): needs the reference tree (oracle.ref_import), writes data only.

    python tools/gen_golden_dptv.py

The eight sides, in the pack order of `forward_pairs_tokens(heads="varlen")` (side a of the four entries, then side b):

    a: 1x1   every level degenerates, a bilinear from one pixel      b: 2x8   the second of the two adjacent 2x8 entries
       1x9   one patch row; 36 and 144 columns cross 32-column tiles     3x5   odd in both axes
       5x1   h > w, odd h: the 2 x 3 -> 5 crop of refinenet4             4x4   square
       2x8   the first of the two adjacent 2x8 entries                   6x10  the largest side, a whole frame

Besides the `decv_*` keys it records
    alt_stacked      rel-L2 between the reference's POINTS for the two adjacent 2x8 sides and what it returns when the two are fed as ONE
                     4x8 image - what a kernel without per-entry borders computes.  Asserted >= 3e-3 (3 x the GPU parity bar).
    alt_stacked_conf the same for the confidence (recorded, not asserted: the confidence moves far less).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_decv as D          # noqa: E402
from vista_slam_amd import weights as W          # noqa: E402

NAME = "dptv_tiny_b4_edges"
ALT_STACKED_MIN = 3e-3
FRAME = (96, 160)          # a 6 x 10 patch grid
# (y0, x0, h, w) of each window in the frame's patch grid
CASE = dict(cfg="tiny", qk_gain=4.0, seed_from=43, entries=[
    ((FRAME, ("win", (2, 3, 1, 1))), (FRAME, ("win", (3, 1, 2, 8)))),
    ((FRAME, ("win", (4, 0, 1, 9))), (FRAME, ("win", (1, 4, 3, 5)))),
    ((FRAME, ("win", (0, 7, 5, 1))), (FRAME, ("win", (2, 5, 4, 4)))),
    ((FRAME, ("win", (0, 2, 2, 8))), (FRAME, ("whole",)))])
SHAPES = ([(1, 1), (1, 9), (5, 1), (2, 8)], [(2, 8), (3, 5), (4, 4), (6, 10)])
torch.set_grad_enabled(False)


def build():
    """-> dict of arrays.  Needs the reference tree."""
    from oracle.ref_import import load_reference_model
    D.CASES[NAME] = CASE
    try:
        res = D.build_case(NAME)
    finally:
        del D.CASES[NAME]
    assert [tuple(r) for r in res["rect_a"].tolist()] == SHAPES[0] and [tuple(r) for r in res["rect_b"].tolist()] == SHAPES[1]
    meta = dict(zip(res["meta_keys"].tolist(), res["meta_vals"].tolist()))
    cfg = W.TINY
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        model = load_reference_model(cfg, W.state_dict(cfg, seed=int(meta["seed"]), qk_gain=float(meta["qk_gain"])))
        # the two adjacent 2x8 sides (a of entry 3, b of entry 0) as ONE 4x8 image
        feat = torch.from_numpy(np.concatenate([res["feat_a_e3"], res["feat_b_e0"]]))[None]
        hooks = [torch.from_numpy(np.concatenate([res[f"dec1_hook{hk - 1}_e3"][1:], res[f"dec2_hook{hk - 1}_e0"][1:]]))[None] for hk in cfg.hooks[1:]]
        toks = [None] * (cfg.dec_depth + 2)
        toks[cfg.hooks[0]] = feat
        for hk, t in zip(cfg.hooks[1:], hooks):
            toks[hk] = t
        st = model.head_pts(toks, torch.tensor([[64, 128]]))
        want_p = np.concatenate([res["a_pts3d_e3"], res["b_pts3d_e0"]])
        want_c = np.concatenate([res["a_conf_e3"], res["b_conf_e0"]])
        sub = int(meta["sub"])
        assert 32 % sub == 0
        res["alt_stacked"] = np.float64(D.rel_l2(st["pts3d"].numpy()[0, ::sub, ::sub], want_p))
        res["alt_stacked_conf"] = np.float64(D.rel_l2(st["conf"].numpy()[0, ::sub, ::sub], want_c))
    finally:
        torch.set_num_threads(threads)
    print(f"[dptv] {NAME}: alt_stacked {float(res['alt_stacked']):.3e} (points), {float(res['alt_stacked_conf']):.3e} (confidence)", flush=True)
    assert res["alt_stacked"] >= ALT_STACKED_MIN, f"stacking the two 2x8 sides moves the points by {float(res['alt_stacked']):.2e} only"
    return res


if __name__ == "__main__":
    r = build()
    path = os.path.join(D.OUT, NAME + ".npz")
    np.savez_compressed(path, **r)
    size = os.path.getsize(path)
    print(f"[dptv] {path}: {size / 1e6:.2f} MB")
    assert size <= (1 << 20), size
