"""CPU: the case tables and float64 references of tests/row_cases.py and tests/post_cases.py.

  * every float64 reference reproduces the reference-generated fixtures (ops.npz LayerNorm / SVD / postprocess, post.npz, fmt.npz) at
    the bar tests/test_oracle_golden.py holds the oracle to;
  * every condition a case table states holds: the expected launch plan, the conditioning bounds, the exact-class representability,
    the Shepperd branch coverage;
  * the fp32 oracle (oracle/sta_oracle.py) alone stays within a quarter of each derived bound - a bound the plain fp32 restatement of
    the formula could not meet would be a wrong derivation, not a finding about a kernel.
tests/test_row_gpu.py and tests/test_post_gpu.py run the kernels on the same tables."""
import ctypes as C
import os

import numpy as np
import pytest

import post_cases as PC
import row_cases as RC
from helpers import load_golden, max_rel
from oracle import sta_oracle as O

PREC = {"f16": 1, "f16x3": 3}
PLANE_BAR = {"f16x3": 1e-5, "f16": 3e-3}          # fp32 class; test_gpu_kernels.TOL["f16"]
FIELDS = ("family", "bm", "bn", "m_tail", "tiles_m", "tiles_n", "ksplit", "slab_ks")


@pytest.fixture(scope="module")
def ops():
    return load_golden("ops")[0]


# ------------------------------------------------------------------------------------------ references vs fixtures
def test_layernorm64_reproduces_fixture(ops):
    assert max_rel(RC.layernorm64(ops["ln_x"], ops["ln_w"], ops["ln_b"], 1e-6), ops["ln_out"]) < 2e-6


def test_svd_rotation64_reproduces_fixture(ops):
    r = np.stack([PC.svd_rotation64(m) for m in ops["svd_in"]])
    assert np.abs(r - ops["svd_out"]).max() < 5e-6
    assert np.allclose(np.linalg.det(r), 1.0, atol=1e-12)


def test_postprocess64_reproduces_fixture(ops):
    pre = ops["post_in"][0].transpose(1, 2, 0)                       # [h,w,4]
    pts, conf = PC.postprocess64(pre)
    assert max_rel(pts, ops["post_pts"][0]) < 2e-6 and max_rel(conf, ops["post_conf"][0]) < 2e-6
    assert np.all(pts[0, 0] == 0)


def test_post_sta_references_reproduce_fixture():
    g = load_golden("post")[0]
    K1, cm = PC.intr_ref(g["pts"], g["conf"], 1)
    K0, _ = PC.intr_ref(g["pts"], g["conf"], 0)
    assert max_rel(K1, g["K_shared"]) < 2e-6 and max_rel(K0, g["K_per"]) < 2e-6
    assert max_rel(cm, g["conf_mean"]) < 2e-6
    s = PC.scale_ref(g["pts"][0, ..., 2].reshape(-1), g["pts"][1, ..., 2].reshape(-1), g["conf"][0].reshape(-1), g["conf"][1].reshape(-1))
    assert abs(float(s) - float(g["scale"])) < 2e-6 * abs(float(g["scale"]))


def test_cloud_and_se3_references_reproduce_fixture():
    g = load_golden("fmt")[0]
    world, _mag = PC.cloud_ref64(g["depths"], g["scales"].reshape(-1), g["intrinsics"], g["poses"])
    keep = g["confs"] > float(g["thres"])
    assert int(keep.sum()) == len(g["points"])
    assert max_rel(world[keep], g["points"]) < 1e-5
    col = PC.color_of(g["imgs"]).transpose(0, 2, 3, 1)[keep]
    assert np.abs(col - g["colors"]).max() < 1e-6
    se3, _raw, _br = PC.shepperd64(g["poses"])
    q = g["quat_xyzw"] * np.sign(g["quat_xyzw"][:, 3:4])
    assert np.abs(se3[:, 3:] - q).max() < 2e-6 and np.array_equal(se3[:, :3].astype(np.float32), g["poses"][:, :3, 3])


# ------------------------------------------------------------------------------------------ residual GEMM + LayerNorm
@pytest.fixture(scope="module")
def lib():
    from vista_slam_amd import _lib
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libsta_mi355_test.so not built here (python -m vista_slam_amd.build)")
    return _lib.load_test()


def host_plan(lib, c, prec):
    out = (C.c_int * 8)()
    assert lib.sta_debug_gemm_plan(0, RC.EPI_F32R, c["M"], c["N"], c["K"], PREC[prec], 0, 0, 0, out) == 0, lib.sta_last_error()
    return dict(zip(FIELDS, out))


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("c", RC.RESID_CASES, ids=RC.case_id)
def test_resid_case_plans(lib, c, prec):
    """Each case runs the path its table entry says: K slices to resid_ln_kernel (slab_ks > 1) below the small-grid predicate, the
    in-place GEMM on a throughput family + ln_kernel above it."""
    p = host_plan(lib, c, prec)
    assert (p["slab_ks"] > 1) == c["slab"], p
    if c["slab"]:
        assert p["family"] == 6 and p["ksplit"] == p["slab_ks"] and p["slab_ks"] * c["M"] * c["N"] <= 4 << 20, p
    else:
        assert p["family"] != 6 and p["ksplit"] == 1, p
    if (c["M"], c["N"], c["K"]) == (5, 64, 256):
        assert p["slab_ks"] == 2, p                  # "two slices"


def test_resid_table_covers_what_it_claims():
    shapes = {(c["M"], c["N"], c["K"]) for c in RC.RESID_CASES}
    assert shapes == {(5, 64, 256), (196, 768, 768), (392, 768, 3072), (197, 1024, 1024), (129, 192, 512), (2400, 768, 768), (6200, 768, 768)}
    assert [c["M"] for c in RC.RESID_CASES if not c["slab"]] == [6200]       # one shape runs the in-place GEMM + ln_kernel
    for c in RC.RESID_CASES:
        assert c["N"] % 4 == 0 and c["N"] <= 1024 and c["K"] % 32 == 0


@pytest.mark.parametrize("c", RC.RESID_CASES, ids=RC.case_id)
def test_resid_exact_class_is_representable(c):
    """Every partial sum of the integer class is an integer of magnitude <= 2048: fp16 holds it, so fp32 accumulation in ANY order
    and any number of slices gives the same integer."""
    A, W, b, x = RC.resid_inputs(c, "int")
    for a in (A, W, b, x):
        assert np.array_equal(a, np.rint(a)) and np.array_equal(a.astype(np.float16).astype(np.float32), a)
    assert RC.int_partial_bound(A, W, b, x) <= 2048
    ref = RC.resid_ref64(A, W, b, x)
    assert np.array_equal(ref, np.rint(ref)) and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    assert len(np.unique(ref)) > 100             # not a degenerate result


@pytest.mark.parametrize("c", RC.RESID_CASES, ids=RC.case_id)
def test_resid_affine_sets_are_far_apart(c):
    """Set 2's expected planes differ from set 1's by more than 100 x the loosest bar in EVERY row: swapped gains cannot pass."""
    A, W, b, x = RC.resid_inputs(c, "gauss")
    g1, b1, g2, b2 = RC.affine_sets(c["N"])
    sep = RC.set_separation(RC.resid_ref64(A, W, b, x), g1, b1, g2, b2)
    assert sep.min() > 100 * max(PLANE_BAR.values()), sep.min()
    # ... and so does set 2 evaluated with set 1's GAINS only
    x2 = RC.resid_ref64(A, W, b, x)
    assert RC.row_rel_l2(RC.layernorm64(x2, g1, b2), RC.layernorm64(x2, g2, b2)).min() > 100 * max(PLANE_BAR.values())


def test_layernorm_oracle_within_a_quarter_of_the_plane_bar():
    """The fp32 oracle on the residual class's rows: per row within a quarter of the fp32-class bar."""
    c = RC.RESID_CASES[0]
    A, W, b, x = RC.resid_inputs(c, "gauss")
    x2 = RC.resid_ref64(A, W, b, x).astype(np.float32)
    g1, b1, _g2, _b2 = RC.affine_sets(c["N"])
    e = RC.row_rel_l2(O.layernorm(x2, g1, b1, 1e-6), RC.layernorm64(x2, g1, b1))
    assert e.max() < 0.25 * PLANE_BAR["f16x3"], e.max()


def test_layernorm_row_kinds():
    for M in RC.LN_M:
        for Cd in RC.LN_C:
            assert Cd % 4 == 0 and Cd <= 1024
            x, g, b = RC.ln_inputs(M, Cd, "constant")
            assert np.all(x == x[:, :1]) and len(np.unique(x[:, 0])) == M
            ref = RC.layernorm64(x, g, b)
            assert np.array_equal(ref, np.broadcast_to(b.astype(np.float64), ref.shape))          # the reference itself returns the bias
            x, _g, _b = RC.ln_inputs(M, Cd, "offset")
            assert np.all(np.abs(x.astype(np.float64).mean(1)) > 3e3 * x.astype(np.float64).std(1))
            x, _g, _b = RC.ln_inputs(M, Cd, "outlier")
            assert np.all((x == 1e3).sum(1) == 1)
    assert {m % 4 for m in RC.LN_M} == {0, 1, 2, 3} and min(RC.LN_M) == 1
    assert any(c < 256 for c in RC.LN_C) and {252, 256, 260, 1020, 1024} <= set(RC.LN_C)


# ------------------------------------------------------------------------------------------ head_final
@pytest.mark.parametrize("npix", PC.HEAD_NPIX)
def test_head_final_inputs(npix):
    feat, w4, bias = PC.head_final_inputs(npix)
    assert feat.min() >= 1 and np.array_equal(feat.astype(np.float16).astype(np.float32), feat) and np.array_equal(feat, np.rint(feat))
    # every lane of the 16-lane butterfly (8 channels each) carries weight for every output
    assert np.all(np.abs(w4).reshape(4, 16, 8).sum(-1) > 0)
    assert float((np.abs(feat.astype(np.float64)) @ np.abs(w4.astype(np.float64)).T + np.abs(bias.astype(np.float64))).max()) < 2048      # any partial sum
    pre = PC.head_final_pre64(feat, w4, bias)
    assert np.array_equal(pre[:, :3], np.rint(pre[:, :3]))                 # x, y, z exact integers
    assert np.all(pre[0, :3] == 0)
    d = np.sqrt((pre[:, :3] ** 2).sum(-1))
    assert d.max() < 80                                                    # expm1 stays inside fp32
    if npix > 1:
        assert 8 < d[1] < 12
    pts, conf = PC.postprocess64(pre)
    assert np.all(pts[0] == 0) and np.isfinite(pts).all() and np.isfinite(conf).all()
    # the fp32 oracle within a quarter of the tightest bar (5 x TOL["f16x3"] = 1e-4), per pixel
    opts, oconf = O.postprocess(pre.astype(np.float32).T.reshape(1, 4, 1, npix))
    assert PC.pixel_rel(opts.reshape(npix, 3), pts).max() < 0.25e-4
    assert PC.pixel_rel(oconf.reshape(npix, 1), conf.reshape(npix, 1)).max() < 0.25e-4


# ------------------------------------------------------------------------------------------ nearest rotation
@pytest.fixture(scope="module")
def svd_tab():
    return PC.svd_table()


def test_svd_table_conditions(svd_tab):
    mats, kinds = svd_tab
    assert len(mats) == max(PC.SVD_B) and mats.dtype == np.float32
    rnd = mats[kinds == "random"]
    dets = np.linalg.det(PC.row_normalize64(rnd))
    assert abs(int((dets < 0).sum()) - len(rnd) / 2) <= 1
    for m, k in zip(mats, kinds):
        S = np.linalg.svd(PC.row_normalize64(m), compute_uv=False)
        if k in ("random", "rot", "rep+", "rep-"):
            gap, s2 = PC.svd_gap(m)
            assert s2 >= 1e-3 and gap >= PC.SVD_GAP, (k, S)
            # the bound the comparison rests on: row perturbation 3 x 2^-24 over the gap, under a quarter of 1e-5
            assert 3 * 2.0 ** -24 / gap < 0.25e-5
        if k in ("rep+", "rep-"):
            assert abs(S[0] - S[1]) < 1e-6 * S[0] and S[2] < 0.6 * S[1], S
        if k == "rot":
            assert abs(S[0] - S[2]) < 1e-6 * S[0], S
        if k == "rank2":
            assert S[2] < 1e-15 and S[1] > 0.1, S
            a, b = PC.svd_rotation64(m, 1), PC.svd_rotation64(m, -1)
            assert np.abs(a - b).max() > 0.1
        if k == "rank1":
            assert S[1] < 1e-6 and S[0] > 0.5, S
        if k == "zero":
            assert S[0] == 0
    for k in ("rot", "rep+", "rep-", "rank2", "rank1", "zero", "random"):
        assert (kinds == k).any(), k
    assert kinds[0] == "rot"                       # B = 1 runs a regular case


def test_svd_oracle_within_a_quarter_of_the_bar(svd_tab):
    mats, kinds = svd_tab
    reg = np.isin(kinds, ("random", "rot", "rep+", "rep-"))
    ref = np.stack([PC.svd_rotation64(m) for m in mats[reg]])
    got = O.svd_orthogonalize(mats[reg])
    assert np.abs(got - ref).max() < 0.25e-5, np.abs(got - ref).max()


# ------------------------------------------------------------------------------------------ mat_to_se3
def test_se3_table_branch_coverage():
    pose = PC.se3_table()
    assert len(pose) == max(PC.SE3_B)
    se3, raw, br = PC.shepperd64(pose)
    for b in range(4):
        assert (br == b).sum() >= 3, (b, np.bincount(br, minlength=4))
        assert ((br == b) & (raw < 0)).sum() >= (0 if b == 0 else 1)       # (the trace branch has qw = s / 4 > 0)
    assert (raw < 0).sum() >= 3
    # the kernel's fp32 comparisons pick the same branch as the float64 definition on every case
    assert [PC.shepperd_branch(P[:3, :3], np.float32) for P in pose] == br.tolist()
    tr = pose[:, 0, 0].astype(np.float64) + pose[:, 1, 1] + pose[:, 2, 2]
    assert (tr == 0).sum() >= 3                                            # the cyclic permutations: trace exactly 0
    assert ((pose[:, 0, 0] == pose[:, 1, 1]) & (tr <= 0)).sum() >= 2       # ties m00 == m11 below the trace branch
    assert (np.abs(raw) < 1e-3).sum() >= 8                                 # rotations by pi and pi - 1e-3
    assert np.abs(np.linalg.norm(se3[:, 3:], axis=1) - 1).max() < 1e-12 and se3[:, 6].min() >= 0
    # the quaternion reproduces R (to the rounding of the fp32 entries it was computed from)
    assert np.abs(PC.quat_to_rot(se3[:, 3:]) - pose[:, :3, :3]).max() < 0.5e-6
    # the oracle is the same definition
    assert np.abs(O.mat_to_se3(pose) - se3).max() < 1e-12


# ------------------------------------------------------------------------------------------ world point cloud
def test_cloud_geometry_table():
    want = {(1, 5, 7): (1, 1), (3, 9, 29): (4, 1), (3, 300, 301): (1059, 2), (2, 513, 512): (2052, 3)}
    for g in PC.CLOUD_GEOMS:
        assert PC.cloud_blocks(g) == want[g], (g, PC.cloud_blocks(g))
    assert (1 * 5 * 7) < 64 and (3 * 9 * 29) % 256 != 0 and 9 * 29 % 64 != 0


@pytest.mark.parametrize("geom", PC.CLOUD_GEOMS[:3], ids=str)
def test_cloud_patterns(geom):
    n = geom[0] * geom[1] * geom[2]
    for pat in PC.CLOUD_PATTERNS:
        conf, keep = PC.cloud_conf(geom, pat)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(conf > np.float32(PC.CLOUD_THRES), keep), pat
        want = {"all": n, "none": 0, "first": 1, "last": 1}.get(pat)
        if want is not None:
            assert int(keep.sum()) == want
        else:
            assert 0.25 * n < keep.sum() < 0.75 * n
    assert (PC.cloud_conf(geom, "at_thres")[0] == np.float32(PC.CLOUD_THRES)).sum() > 0.1 * n
    assert np.isnan(PC.cloud_conf(geom, "nan")[0]).sum() > 0.1 * n
    assert PC.cloud_conf(geom, "first")[1].reshape(-1)[0] and PC.cloud_conf(geom, "last")[1].reshape(-1)[-1]


@pytest.mark.parametrize("geom", PC.CLOUD_GEOMS[:3], ids=str)
def test_cloud_exact_class_is_exact_in_fp32(geom):
    depths, scales, K, poses, imgs = PC.cloud_inputs(geom, "exact")
    world, _mag = PC.cloud_ref64(depths, scales, K, poses)
    assert np.array_equal(world.astype(np.float32).astype(np.float64), world)
    conf, keep = PC.cloud_conf(geom, "random")
    pts, _col = O.world_pointcloud(depths, scales, K, poses, conf, imgs, PC.CLOUD_THRES)
    assert len(pts) == keep.sum() and np.array_equal(pts.astype(np.float64), world[keep])       # the fp32 oracle equals float64
    for n in range(geom[0]):
        assert np.array_equal(np.abs(poses[n, :3, :3]).sum(0), np.ones(3)) and np.array_equal(np.abs(poses[n, :3, :3]).sum(1), np.ones(3))
        assert K[n, 0, 1] == 0 and np.log2(K[n, 0, 0]) % 1 == 0 and np.log2(K[n, 1, 1]) % 1 == 0 and K[n, 0, 2] % 1 == 0 and K[n, 1, 2] % 1 == 0


@pytest.mark.parametrize("geom", PC.CLOUD_GEOMS[:3], ids=str)
def test_cloud_general_bound_holds_for_the_fp32_oracle(geom):
    """|fp32 - float64| <= 32 x 2^-24 x mag per coordinate: the fp32 oracle (LU inverse, einsum) fits a QUARTER of it."""
    depths, scales, K, poses, imgs = PC.cloud_inputs(geom, "general")
    world, mag = PC.cloud_ref64(depths, scales, K, poses)
    assert np.all(K[:, 0, 1] != 0) and np.all(K[:, 1, 0] == 0) and np.all(mag >= np.abs(world) * (1 - 1e-12))
    conf, keep = PC.cloud_conf(geom, "all")
    pts, col = O.world_pointcloud(depths, scales, K, poses, conf, imgs, PC.CLOUD_THRES)
    ratio = np.abs(pts.astype(np.float64) - world[keep]) / (PC.CLOUD_BOUND * mag[keep])
    assert ratio.max() < 0.25, ratio.max()
    assert np.array_equal(col, PC.color_of(imgs).transpose(0, 2, 3, 1)[keep])


def test_color_ties():
    t = PC.color_ties()
    prod = (np.clip(PC.color_of(t), np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.float32)
    half = prod[(prod % 1) == 0.5]
    assert len(half) >= 16 and {int(v) % 2 for v in half} == {0, 1}          # exact .5 ties above even AND odd integers
    b = PC.color_byte(PC.color_of(t))
    assert np.array_equal(b[(prod % 1) == 0.5] % 2, np.zeros(len(half), np.uint8))       # round half to even
    assert t.min() < -1 and t.max() > 1 and 0 in b and 255 in b
    imgs = PC.cloud_inputs((1, 5, 7), "general")[4]
    assert len(t) <= imgs.size and np.array_equal(imgs.reshape(-1)[:len(t)], t)      # the smallest geometry holds them all


# ------------------------------------------------------------------------------------------ intrinsics / scale
def test_intrinsics_shape_table():
    for B, H, W, nblk in PC.INTR_SHAPES:
        assert PC.intr_nblk(H, W) == nblk, (H, W)
    assert 3 * 683 == 2048 + 1 and (513 * 1024 + 2047) // 2048 > 256
    for s in PC.INTR_SHARED:
        assert s < 2 or 6 % s == 0
    assert 1 % 2 != 0                                  # B = 1 with shared = 2 is the refused call


@pytest.mark.parametrize("B,H,W,nblk", PC.INTR_SHAPES)
def test_intrinsics_inputs_are_well_conditioned(B, H, W, nblk):
    pts, conf = PC.intr_inputs(B, H, W)
    terms = PC.intr_terms(pts, conf)
    for shared in (PC.INTR_SHARED if B == 6 else (0,)):
        for idx in PC.intr_groups(B, shared):
            for t in terms[:4]:
                assert PC.conditioning(t[idx]) <= PC.COND_MAX, (shared, idx, PC.conditioning(t[idx]))
    for b in range(B):
        assert PC.conditioning(terms[4][b]) <= PC.COND_MAX
    if H * W >= 100:
        X, Z = pts[..., 0], pts[..., 2]
        assert ((Z == 0) & (X == 0)).any() and ((Z == 0) & (X != 0)).any() and (Z < 0).any()
        for v in (0.0, 1e-7, -1.0):
            assert (conf == np.float32(v)).any()


def test_intrinsics_summation_orders_and_oracle_agree_to_the_ulp():
    B, H, W = 6, 257, 512
    pts, conf = PC.intr_inputs(B, H, W)
    for shared in (0, 1):
        K, cm = PC.intr_ref(pts, conf, shared, "forward")
        for order in ("reverse", "blocks"):
            K2, cm2 = PC.intr_ref(pts, conf, shared, order)
            assert np.array_equal(K, K2) and np.array_equal(cm, cm2), (shared, order)
        assert np.array_equal(O.estimate_intrinsic_from_pts3d(pts, conf, bool(shared)), K), shared


@pytest.mark.parametrize("n", PC.SCALE_N)
def test_scale_inputs(n):
    Di, Dj, ci, cj = PC.scale_inputs(n)
    num, den = PC.scale_terms(Di, Dj, ci, cj)
    assert PC.conditioning(num) <= PC.COND_MAX and PC.conditioning(den) <= PC.COND_MAX
    assert ((ci * cj) < 1e-6).any()
    s = PC.scale_ref(Di, Dj, ci, cj)
    assert PC.ulp_diff(s, PC.scale_ref(Di, Dj, ci, cj, reverse=True)) == 0
    assert PC.ulp_diff(s, O.estimate_scale_with_depth_and_confidence(Di, Dj, ci, cj)) == 0
    assert (n > 1024) == (n in (1025, 50179))          # the sizes at which a thread takes a second trip


def test_pack_table():
    assert [h * w for h, w in PC.PACK_HW] == [1, 255, 257, 1008, 1100000]
    trips = [PC.pack_trips(h, w) for h, w in PC.PACK_HW]
    assert max(trips[:4]) <= 8 and trips[4] > 8, trips              # only the last shape is past the grid cap
