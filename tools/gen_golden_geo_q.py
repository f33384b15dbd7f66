"""Fixtures `tests/golden/geo_q_*.npz` and `geo_ray_*.npz`: the REFERENCE's `compute_geo_valid_mask_batched`,
`compute_local_pointclouds` and `depth_from_pointcloud_dot_batched` (vista_slam/utils/slam_utils.py:82-266) in fp32 on the CPU,
on the procedural scenes of tests/geo_cases.py (seed 11: the focal length grows per view, so K1 != K2).

TEST INFRASTRUCTURE, like tools/gen_golden_geo.py: needs the reference tree (oracle.ref_import.REF_ROOT), writes data only.

    python tools/gen_golden_geo_q.py                     # every case
    python tools/gen_golden_geo_q.py geo_q_224_b3
    python tools/gen_golden_geo_q.py --check             # regenerate in memory and compare with the committed files, array by array

  geo_q_*:   depth1_code, depth2_code (the fp32 depths, exactly: geo_cases.depth_code; a `_nan` case's NaN is applied by the
             loader), K1, K2, T1, T2, q; mask (reference, packed bits); thres (the fp32 restatement's = torch.quantile of the
             restatement's errors: the reference does not return its threshold), thres64, count, count64 (valid pixels);
             dev_uv, dev_err, band_uv, band_err (tests/geo_cases.py: BAND_FACTOR = 8); uv_border, border (packed bits); spread,
             thr_tol = 2 band_err + spread; min_z2.
             Rule: masks equal wherever border == 0; threshold within thr_tol of `thres`; count within the number of uv-border
             pixels of `count`.
  geo_ray_*: depth_code, K [n,3,3] (the shared form uses K[0]); pc_b, pc_s, rd_b, rd_s (reference, fp32; batched / shared K; the
             ray depths are taken of the reference's own fp32 point clouds); pc64_b, pc64_s, rd64_b, rd64_s (fp64 restatement on
             the same inputs); dev_pc = max |pc32 - pc64|_inf / |pc64|_2, dev_rd = max |rd32 - rd64| / |rd64|.
             Rule: within 8 x dev of the fp64 value at every pixel, same normalisation.
Asserted here (and again on the committed files by tests/test_geo_q_cpu.py): at most 2 % of a mask fixture is undecided; the
reference's own output and the fp32 restatement have 0 pixels outside the rule against fp64; spread <= 1e-3 x thres; each mask
value covers >= 5 % (the `_min` and `_nan` cases are all False by construction).  If one fails, change the scene, not the cap.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import geo_cases as G          # noqa: E402
import geo_q_cases as Q        # noqa: E402
from gen_golden_geo import ref_slam_utils          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)


def build_q(name, su):
    H, W = Q.Q_CASES[name][:2]
    d1, d2c, K1, K2, T1, T2, q = Q.q_case_inputs(name)
    d2 = Q.apply_nan(name, d2c)
    t = torch.from_numpy
    ref = su.compute_geo_valid_mask_batched(t(d1), t(d2), t(K1), t(K2), t(T1), t(T2), q).numpy()
    p32, p64 = Q.q_parts(d1, d2, K1, K2, T1, T2, q, np.float32), Q.q_parts(d1, d2, K1, K2, T1, T2, q, np.float64)
    dev_uv, dev_err = Q.q_deviation(p32, p64, H, W)
    band_uv, band_err = G.BAND_FACTOR * dev_uv, G.BAND_FACTOR * dev_err
    uvb = Q.q_uv_border(p64, band_uv).reshape(ref.shape)
    border = Q.q_border(p64, p32["thres"], band_uv, band_err)
    spread = Q.q_spread(p64, d2, q, band_uv)
    thr_tol = 2 * band_err + spread
    out_ref = Q.check_q_masks(ref, p64["mask"], border)
    out_32 = Q.check_q_masks(p32["mask"], p64["mask"], border) + Q.check_q_masks(p32["mask"], ref, border)
    share, true_share = float(border.mean()), float(ref.mean())
    print(f"[geo_q] {name}: valid {p32['count']} / {ref.size} (fp64 {p64['count']}) thres {float(p32['thres']):.6g} (fp64 {float(p64['thres']):.6g}) "
          f"dev_uv {dev_uv:.2e} dev_err {dev_err:.2e} uv-border {int(uvb.sum())} border {100 * share:.2f} % spread {spread:.2e} thr_tol {thr_tol:.2e} "
          f"reference outside the rule {out_ref} restatement32 outside {out_32} (differs from the reference at "
          f"{int((p32['mask'] != ref).sum())}) True on {100 * true_share:.0f} % min z2 {np.nanmin(p64['z2']):.3f}", flush=True)
    assert share <= G.MAX_BORDERLINE, f"{name}: {share:.4f} of the pixels are undecided"
    assert out_ref == 0 and out_32 == 0, f"{name}: the reference / the fp32 restatement leaves the band: change the scene"
    assert Q.thres_within(p32["thres"], p64["thres"], thr_tol), (name, p32["thres"], p64["thres"])
    assert abs(p32["count"] - p64["count"]) <= int(uvb.sum())
    if np.isfinite(p64["thres"]):
        assert spread <= Q.MAX_SPREAD_REL * float(p64["thres"]), f"{name}: spread {spread:.3e} vs thres {float(p64['thres']):.3e}"
    if name in Q.ALL_FALSE:
        assert not ref.any()
    else:
        assert G.MIN_MASK_SHARE <= true_share <= 1 - G.MIN_MASK_SHARE, f"{name}: True on {true_share:.3f}"
    return dict(depth1_code=G.depth_code(d1), depth2_code=G.depth_code(d2c), K1=K1, K2=K2, T1=T1, T2=T2, q=np.float64(q),
                mask=G.pack_bits(ref), thres=np.float32(p32["thres"]), thres64=np.float64(p64["thres"]), count=np.int64(p32["count"]),
                count64=np.int64(p64["count"]), dev_uv=np.float64(dev_uv), dev_err=np.float64(dev_err), band_uv=np.float64(band_uv),
                band_err=np.float64(band_err), uv_border=G.pack_bits(uvb), border=G.pack_bits(border), spread=np.float64(spread),
                thr_tol=np.float64(thr_tol), min_z2=np.float64(np.nanmin(p64["z2"])))


def build_ray(name, su):
    n, H, W = Q.RAY_CASES[name]
    depth, K, _T = G.scene(n, H, W, seed=Q.Q_SEED)
    t = torch.from_numpy
    res = dict(depth_code=G.depth_code(depth), K=K)
    dev_pc = dev_rd = 0.0
    for tag, Kf in (("b", K), ("s", K[0])):
        pc = su.compute_local_pointclouds(t(depth), t(Kf)).numpy()
        rd = su.depth_from_pointcloud_dot_batched(t(pc), t(Kf)).numpy()
        pc64, rd64 = Q.local_points_np(depth, Kf, np.float64), Q.ray_depth_np(pc, Kf, np.float64)
        dev_pc = max(dev_pc, float(Q.pc_distance(pc, pc64).max()))
        dev_rd = max(dev_rd, float(Q.rd_distance(rd, rd64).max()))
        res.update({f"pc_{tag}": pc, f"rd_{tag}": rd, f"pc64_{tag}": pc64, f"rd64_{tag}": rd64})
    print(f"[geo_q] {name}: dev_pc {dev_pc:.2e} dev_rd {dev_rd:.2e} -> bounds {G.BAND_FACTOR * dev_pc:.2e} / {G.BAND_FACTOR * dev_rd:.2e}", flush=True)
    assert 0 < dev_pc < 1e-6 and 0 < dev_rd < 1e-6
    res.update(dev_pc=np.float64(dev_pc), dev_rd=np.float64(dev_rd))
    return res


def build_case(name, su):
    return build_q(name, su) if name in Q.Q_CASES else build_ray(name, su)


def write_case(name, su, out_dir=OUT):
    res = build_case(name, su)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"[geo_q] {name}: {size / 1e6:.2f} MB", flush=True)
    assert size <= (1 << 20), f"{path}: {size} bytes (committed files stay below 1 MiB)"
    return path


def check_case(name, su, out_dir=OUT):
    res = build_case(name, su)
    with np.load(os.path.join(out_dir, f"{name}.npz")) as z:
        assert sorted(z.files) == sorted(res), (name, sorted(z.files), sorted(res))
        for k in z.files:
            a, b = np.asarray(res[k]), z[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name}: {k} differs from the committed file"
    print(f"[geo_q] {name}: identical to the committed file", flush=True)


if __name__ == "__main__":
    cases = list(Q.Q_CASES) + list(Q.RAY_CASES)
    args = sys.argv[1:]
    check = "--check" in args
    sel = [a for a in args if a != "--check"] or cases
    assert all(s in cases for s in sel), f"cases: {cases}"
    su = ref_slam_utils()
    for nm in sel:
        (check_case if check else write_case)(nm, su)
