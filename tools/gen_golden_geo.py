"""Fixtures `tests/golden/geo_*.npz`: the REFERENCE's `view_consistency_check` and `compute_symmetric_geo_valid_mask`
(vista_slam/utils/slam_utils.py:269-419) in fp32 on the CPU, on the procedural scenes of tests/geo_cases.py.

TEST INFRASTRUCTURE, like tools/gen_golden_decn.py: needs the reference tree (oracle.ref_import.REF_ROOT), writes data only.

    python tools/gen_golden_geo.py               # every case
    python tools/gen_golden_geo.py geo_sym_224_p2

Both outputs are thresholded decisions, so every fixture carries the MEASURED distance between the fp32 and the fp64 evaluation
of the formulas and the band derived from it (tests/geo_cases.py: BAND_FACTOR = 8), and the map of pixels that lie inside it:
  geo_vote_*: depth_code (the fp32 depths, exactly: geo_cases.depth_code), K, poses (fp32 inputs), threshold, window; count
              (reference, int8), count64 (fp64 restatement, int8); dev = max |err32 - err64| over every (pixel, neighbour),
              band = 8 dev; nb [n,H,W] int8 = neighbours whose fp64 |err - threshold| < band.
              Rule: |count - count_ref| <= nb at every pixel.
  geo_sym_*:  depth_code of depths [P,2,H,W], K [P,3,3], rel_pose [P,4,4]; mask (reference, packed bits); thres [P,2] (the fp32
              restatement's: the reference does not return its thresholds), thres64; dev_uv, dev_err (over pixels that round to
              the same target), band_uv, band_err; border (packed bits) = uv within band_uv of a rounding boundary, or
              |err - thres| < band_err + 2 |thres32 - thres64| on a valid pixel.
              Rule: masks equal wherever border == 0; thresholds within 2 band_err of the recorded ones.
Asserted here (and again on the committed files by tests/test_geo_cpu.py): at most 2 % of a fixture's pixels are undecided; the
reference's own fp32 output obeys the rule against the fp64 restatement (this validates band and restatement - if it fails,
change the scene, not the cap); every vote value 0 .. min(2 window, n - 1) occurs; each mask value covers >= 5 % of a fixture.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geo_cases as G          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)


def ref_slam_utils():
    """The reference's slam_utils module (colorama stubbed: terminal colours only)."""
    from oracle.ref_import import REF_ROOT
    if "colorama" not in sys.modules:
        col = types.ModuleType("colorama")

        class _Any:
            def __getattr__(self, _name):
                return ""
        col.Fore = _Any(); col.Style = _Any()
        sys.modules["colorama"] = col
    spec = importlib.util.spec_from_file_location("ref_slam_utils", os.path.join(REF_ROOT, "vista_slam", "utils", "slam_utils.py"))
    su = importlib.util.module_from_spec(spec); spec.loader.exec_module(su)
    return su


def build_vote(name, su):
    n, H, W = G.VOTE_CASES[name]
    window, thr = 4, G.VOTE_THRESHOLD
    depth, K, T = G.scene(n, H, W, seed=11)
    ref = su.view_consistency_check(torch.from_numpy(depth), torch.from_numpy(K), torch.from_numpy(T), threshold=thr).numpy()
    e32 = G.vote_errors(depth, K, T, window, np.float32)
    e64 = G.vote_errors(depth, K, T, window, np.float64)
    fin = np.isfinite(e64)
    with np.errstate(invalid="ignore"):                    # (inf - inf in the slots of absent neighbours)
        dev = float(np.abs(e32.astype(np.float64) - e64)[fin].max())
    band = G.BAND_FACTOR * dev
    nb = G.vote_borderline(e64, thr, band)
    c32, c64 = G.vote_count(e32, thr), G.vote_count(e64, thr)
    share = float((nb > 0).mean())
    out_ref, out_32 = G.check_votes(ref, c64, nb), G.check_votes(c32, c64, nb)
    vals = sorted(set(np.unique(ref).tolist()))
    print(f"[geo] {name}: dev {dev:.2e} band {band:.2e} borderline {100 * share:.2f} % reference outside the rule {out_ref} "
          f"(differs from fp64 at {int((ref != c64).sum())}) restatement32 outside {out_32} "
          f"(differs from the reference at {int((c32 != ref).sum())}) votes {vals}", flush=True)
    assert share <= G.MAX_BORDERLINE, f"{name}: {share:.4f} of the pixels are undecided"
    assert out_ref == 0 and out_32 == 0, f"{name}: the reference / the fp32 restatement leaves the band: change the scene"
    assert vals == list(range(min(2 * window, n - 1) + 1)), f"{name}: vote values {vals}"
    return dict(depth_code=G.depth_code(depth), K=K, poses=T, threshold=np.float64(thr), window=np.int64(window), count=ref.astype(np.int8),
                count64=c64.astype(np.int8), nb=nb.astype(np.int8), dev=np.float64(dev), band=np.float64(band))


def build_sym(name, su):
    depths, K, rel = G.sym_case_inputs(name)
    P, _, H, W = depths.shape
    masks, thres, thres64, borders = [], [], [], []
    dev_uv = dev_err = 0.0
    parts = []
    for p in range(P):
        m = su.compute_symmetric_geo_valid_mask(torch.from_numpy(depths[p]), torch.from_numpy(K[p]), torch.from_numpy(rel[p])).numpy()
        p32, p64 = G.sym_parts(depths[p], K[p], rel[p], np.float32), G.sym_parts(depths[p], K[p], rel[p], np.float64)
        near = np.isfinite(p64["uv"]).all(1) & (np.abs(p64["uv"]) < 4 * max(H, W)).all(1)      # uv far outside the frame decides nothing
        if near.any():
            dev_uv = max(dev_uv, float(np.abs(p32["uv"].astype(np.float64) - p64["uv"]).max(1)[near].max()))
        same = p32["valid"] & p64["valid"] & (np.round(p32["uv"]) == np.round(p64["uv"])).all(1)
        if same.any():
            dev_err = max(dev_err, float(np.abs(p32["err"].astype(np.float64) - p64["err"])[same].max()))
        masks.append(m); parts.append((p32, p64))
    band_uv, band_err = G.BAND_FACTOR * dev_uv, G.BAND_FACTOR * dev_err
    out_ref = out_32 = 0
    for p in range(P):
        p32, p64 = parts[p]
        border = G.sym_border(p64, p32["thres"], band_uv, band_err)
        out_ref += G.check_masks(masks[p], p64["mask"], border)
        out_32 += G.check_masks(p32["mask"], p64["mask"], border) + G.check_masks(p32["mask"], masks[p], border)
        with np.errstate(invalid="ignore"):
            assert (np.abs(p32["thres"].astype(np.float64) - p64["thres"]) <= 2 * band_err).all(), (name, p32["thres"], p64["thres"])
        borders.append(border); thres.append(p32["thres"]); thres64.append(p64["thres"])
    masks, borders = np.stack(masks), np.stack(borders)
    share, true_share = float(borders.mean()), float(masks.mean())
    print(f"[geo] {name}: dev_uv {dev_uv:.2e} dev_err {dev_err:.2e} border {100 * share:.2f} % reference outside the rule {out_ref} "
          f"restatement32 outside {out_32} True on {100 * true_share:.0f} % thres {np.stack(thres).round(4).tolist()}", flush=True)
    assert share <= G.MAX_BORDERLINE, f"{name}: {share:.4f} of the pixels are undecided"
    assert out_ref == 0 and out_32 == 0, f"{name}: the reference / the fp32 restatement leaves the band: change the scene"
    assert G.MIN_MASK_SHARE <= true_share <= 1 - G.MIN_MASK_SHARE, f"{name}: True on {true_share:.3f}"
    return dict(depth_code=G.depth_code(depths), K=K, rel_pose=rel, mask=G.pack_bits(masks), thres=np.stack(thres).astype(np.float32),
                thres64=np.stack(thres64).astype(np.float64), border=G.pack_bits(borders), dev_uv=np.float64(dev_uv),
                dev_err=np.float64(dev_err), band_uv=np.float64(band_uv), band_err=np.float64(band_err))


def write_case(name, su, out_dir=OUT):
    res = build_vote(name, su) if name in G.VOTE_CASES else build_sym(name, su)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"[geo] {name}: {size / 1e6:.2f} MB", flush=True)
    assert size <= (1 << 20), f"{path}: {size} bytes (committed files stay below 1 MiB)"
    return path


if __name__ == "__main__":
    cases = list(G.VOTE_CASES) + list(G.SYM_CASES)
    sel = sys.argv[1:] or cases
    assert all(s in cases for s in sel), f"cases: {cases}"
    su = ref_slam_utils()
    for nm in sel:
        write_case(nm, su)
