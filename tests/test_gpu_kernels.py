"""GPU: each hand-written HIP kernel (called through the C ABI debug entry points) against a plain
fp32 reference of the same op.  Tolerances: f16x3 (2-term split, the default) must be fp32-class
(1e-5); f16 (single product == TF32-class mantissa) 2e-3."""
import pytest

pytestmark = pytest.mark.gpu

# head_mx: the DPT head's arithmetic in the default policy (correction products as one block-scaled fp8 MFMA, ~1e-5 per GEMM),
# for the kernels the head is made of
TOL = {"f16x3": 2e-5, "f16": 3e-3, "head_mx": 6e-5, "mlp_mx": 6e-5}
PRECS = ["f16x3", "f16"]
HEAD_PRECS = ["f16x3", "f16", "head_mx"]


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    return gpu_checks


def small_grid(M, N):
    """The small-grid predicate (sta_launch.inc: small_grid_m), restated."""
    return M <= 640 or ((M + 191) // 192) * ((N + 127) // 128) < 192


def small_shape_family(M, N, variant=0):
    """The tile family a shape BELOW the small-grid predicate runs (sta_launch.inc: gemm_plan): the small-grid family 6 whatever
    family 2 / 3 / 4 is forced - a forced family never displaces it -, the register-staged 128x128 kernel (1) where N is no
    multiple of 64, the halo-tiled convolution (8) only where that is forced."""
    assert small_grid(M, N), (M, N)
    return 8 if variant == 8 else (6 if N % 64 == 0 else 1)


@pytest.mark.parametrize("prec", HEAD_PRECS)
@pytest.mark.parametrize("kw", [dict(), dict(resid=True), dict(M=520, N=384, K=1024), dict(act=1, via_f16=1),
                                dict(act=2, via_f16=1), dict(M=1, N=96, K=32), dict(M=129, N=129, K=64),
                                # forced 256-row and 192-row families on SMALL shapes: below the small-grid predicate a forced family never
                                # displaces family 6, so these run 128x64 tiles (asserted below) - M tails and every epilogue of that
                                # family.  The forced families themselves run in test_gemm_tail_rows (dense) and test_conv_exact.py
                                dict(M=700, N=512, K=256, variant=2), dict(M=300, N=384, K=96, variant=2, resid=True),
                                dict(M=513, N=256, K=1024, variant=2, act=1, via_f16=1), dict(M=5, N=128, K=32, variant=2, act=2, via_f16=1),
                                dict(M=700, N=512, K=256, variant=3), dict(M=385, N=384, K=96, variant=3, resid=True),
                                dict(M=193, N=128, K=64, variant=3, act=1, via_f16=1),
                                # ... and ABOVE the predicate (6200 rows x 768 columns: 33 x 6 = 198 tiles of 192x128), where the forced
                                # families do run (fam: asserted): the plane epilogue + ReLU of the head's 1x1 convolutions, in the
                                # f16mx arithmetic too, on 256x256 / 192x256 / 192x128, the automatic choice, and the fp32 + residual one (GELU on these
                                # families: test_gemm_tail_rows)
                                dict(M=6200, N=768, K=256, variant=2, act=2, via_f16=1, fam=2), dict(M=6200, N=768, K=256, variant=3, act=2, via_f16=1, fam=3),
                                dict(M=6200, N=768, K=256, variant=4, act=2, via_f16=1, fam=5), dict(M=6200, N=768, K=256, via_f16=1, fam=5),
                                dict(M=6200, N=768, K=256, variant=3, resid=True, fam=3)])
def test_gemm(G, prec, kw):
    kw = dict(kw)
    fam = kw.pop("fam", None)
    r = G.check_gemm(prec, **kw)
    if fam is None:
        fam = small_shape_family(kw.get("M", 300), kw.get("N", 200), kw.get("variant", 0))
    else:
        assert not small_grid(kw["M"], kw["N"]), kw
    assert r["plan"]["family"] == fam, r
    assert r["nan"] == 0, r
    assert r["rel_l2"] < TOL[prec], r


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kw", [dict(), dict(hp=14, wp=14, pose_tok=0, S=1), dict(hp=3, wp=5, pose_tok=1, S=3),
                                dict(hp=14, wp=14, pose_tok=1, S=2, variant=2), dict(hp=5, wp=7, pose_tok=0, S=3, Cdim=256, K=256, variant=2),
                                dict(hp=14, wp=14, pose_tok=1, S=2, variant=3),
                                # throughput tile (192x128: >= 192 tiles), token rows 32-aligned: the V^T LDS-transpose path; with a pose
                                # token in front (t0 = 32k + 1: unaligned) its fallback
                                dict(hp=24, wp=32, pose_tok=0, S=4, K=64, Cdim=512), dict(hp=24, wp=32, pose_tok=1, S=4, K=64, Cdim=512)])
def test_qkv_rope(G, prec, kw):
    r = G.check_qkv_rope(prec, **kw)
    assert r["q"] < TOL[prec] and r["k"] < TOL[prec] and r["v"] < TOL[prec], r
    assert r["vpad_abs"] == 0.0, "V^T padding must stay zero (0 * garbage = NaN otherwise)"


@pytest.mark.parametrize("kw", [dict(), dict(resid=True), dict(M=520, N=384, K=1024), dict(M=520, N=384, K=1024, resid=True), dict(act=1, via_f16=1),
                                dict(M=129, N=128, K=64, resid=True), dict(M=700, N=512, K=256, variant=3), dict(M=385, N=384, K=96, variant=3, resid=True),
                                dict(M=700, N=512, K=256, variant=2, resid=True), dict(M=193, N=128, K=64, variant=3, act=1, via_f16=1),
                                dict(M=3000, N=1024, K=512, resid=True), dict(M=2400, N=768, K=3072, resid=True), dict(M=3000, N=512, K=256, act=1, via_f16=1)])
def test_gemm_mlp_f16mx(G, kw):
    """Precision f16x3m (round 6): mlp.fc2 in the f16mx arithmetic - fp32 and in-place-residual epilogues on f16mx rows / weights on
    the small-grid, 192x128 and 192x256 families - and mlp.fc1's GELU epilogue writing the f16mx rows (LDS-staged and edge tiles)."""
    r = G.check_gemm("mlp_mx", **kw)
    assert r["rel_l2"] < TOL["mlp_mx"], r


def _assert_tail(r, fam, tail, tol):
    """The GEMM ran on tile family `fam` with the pose rows on the skinny tail blocks (m_tail == tail; tail=0: the case says the
    rows sit in the main tiles), and both the whole matrix and the tail rows alone meet the bar."""
    p = r["plan"]
    assert (p["family"], p["m_tail"]) == (fam, tail), r
    assert (p["tiles_m"] - 1) * p["bm"] < r["M"] - p["m_tail"] <= p["tiles_m"] * p["bm"], r
    if p["m_tail"]:
        assert (r["M"] - p["m_tail"]) % p["bm"] == 0, r
    assert r["rel_l2"] < tol and r["rel_l2_tail"] < tol, r


def _tail(G, prec, fam, tail=16, **kw):
    r = G.check_gemm_tail(prec, tail=tail, **kw)
    bm = 256 if kw.get("variant") == 2 else 192
    r["M"] = kw["M"] if "M" in kw else kw.get("tiles_m", 12) * bm + tail
    return r


# mlp.fc2 under f16x3m: gemm2_tail<MX> on 192x128 and 192x256 (fragments straight from global memory).  Forced family 2 has no
# f16mx fp32-epilogue kernel and runs 192x256: with 8 x 256 patch rows (no whole count of 192-row tiles) the pose rows must stay
# in the main tiles, with 16 x 192 = 12 x 256 they go to the tail blocks.  Last: the product's own decision for the decoder's
# mlp.fc2 at B = 10 @512x512 (20480 patch rows + 20 pose rows, K = 3072, in place): 256x256 by the cost model, 192x256 in f16mx.
@pytest.mark.parametrize("kw", [dict(fam=5, resid=True), dict(fam=3, variant=3, N=768, K=1024, tiles_m=40, resid=True),
                                dict(fam=5, tail=1), dict(fam=5, tail=32, resid=True), dict(fam=5, variant=4, N=768, tiles_m=40, tail=20),
                                dict(fam=3, variant=2, tiles_m=12, resid=True), dict(fam=3, variant=2, tiles_m=8, resid=True, expect_tail=0),
                                dict(fam=3, M=20480 + 20, tail=20, N=768, K=3072, resid=True, expect_tail=0)])
def test_gemm_tail_rows_mlp_f16mx(G, kw):
    """The pose-token tail blocks of mlp.fc2 in the f16mx arithmetic (gemm2_tail<MX>: fragments straight from global memory)."""
    kw = dict(kw)
    fam, expect = kw.pop("fam"), kw.pop("expect_tail", None)
    r = _tail(G, "mlp_mx", fam, **kw)
    _assert_tail(r, fam, kw.get("tail", 16) if expect is None else expect, TOL["mlp_mx"])


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("kw", [dict(fam=5), dict(fam=5, resid=True), dict(fam=5, act=1, via_f16=1),
                                dict(fam=3, variant=3, N=768, K=1024, tiles_m=40, resid=True),
                                dict(fam=2, variant=2, N=4096, K=128, tiles_m=6, act=1, via_f16=1),
                                dict(fam=2, variant=2, N=768, K=256, tiles_m=30, tail=32, resid=True),
                                dict(fam=5, variant=4, N=768, K=256, tiles_m=40, tail=20, resid=True),
                                dict(fam=5, tail=1), dict(fam=5, tail=32, resid=True)])
def test_gemm_tail_rows(G, prec, kw):
    """Skinny tail blocks (the decoder's pose-token rows) on every family / epilogue the decoder uses them with; every case is
    above the small-grid predicate, so the tail blocks really run (the plan says so)."""
    kw = dict(kw)
    fam = kw.pop("fam")
    r = _tail(G, prec, fam, **kw)
    _assert_tail(r, fam, kw.get("tail", 16), TOL[prec])


# plan: (family, m_tail) - small grids run 128x64 tiles with the pose rows in the main tiles; 24 x 32 tokens x 4 sequences at
# C = 512 is past the small-grid predicate: 192x128 tiles, the 4 pose rows on tail blocks (V^T LDS-transpose path)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kw", [dict(plan=(6, 0)), dict(hp=14, wp=14, S=2, plan=(6, 0)), dict(hp=14, wp=14, S=2, variant=3, plan=(6, 0)),
                                dict(hp=24, wp=32, S=4, K=64, plan=(6, 0)), dict(hp=24, wp=32, S=4, K=64, Cdim=512, plan=(5, 4))])
def test_qkv_rope_decoder_rows(G, prec, kw):
    kw = dict(kw)
    plan = kw.pop("plan")
    r = G.check_qkv_rope_decoder_rows(prec, **kw)
    assert r["q"] < TOL[prec] and r["k"] < TOL[prec] and r["v"] < TOL[prec], r
    assert r["q_pose"] < TOL[prec] and r["k_pose"] < TOL[prec] and r["v_pose"] < TOL[prec], r
    assert r["vpad_abs"] == 0.0, r
    assert (r["plan"]["family"], r["plan"]["m_tail"]) == plan, r


# The decoder's paired launch (gemm_qkv_pair): attn.qkv + cross_attn.projk|projv.  24 x 32 tokens, S = 4: both halves past the
# small-grid predicate, one launch (family 7), the 4 pose rows on tail blocks; S = 16 @14x14: 3136 patch rows are no whole
# count of 192-row tiles - still one launch, the pose rows in the main tiles; S = 2 @24x32: below the predicate, two launches
# (the last one: projk|projv on the small-grid family); precision f16: never paired (two 192x128 launches with tails).
PAIR_CASES = [(dict(S=4), "f16x3", (7, 4)), (dict(S=4), "f16x3h", (7, 4)), (dict(S=16, hp=14, wp=14), "f16x3", (7, 0)),
              (dict(S=16, hp=14, wp=14), "f16x3h", (7, 0)), (dict(S=2), "f16x3", (6, 0)), (dict(S=2), "f16x3h", (6, 0)),
              (dict(S=4), "f16", (5, 4)), (dict(S=4, ints=True), "f16x3", (7, 4)), (dict(S=4, ints=True), "f16", (5, 4))]


@pytest.mark.parametrize("kw,prec,plan", PAIR_CASES)
def test_qkv_pair(G, kw, prec, plan):
    r = G.check_qkv_pair(prec, **kw)
    assert (r["plan"]["family"], r["plan"]["m_tail"]) == plan, r
    tol = TOL["f16x3" if prec == "f16x3h" else prec]       # f16x3h: the transformer's GEMMs run f16x3
    for name in ("q_a", "k_a", "v_a", "k_b", "v_b"):
        assert r[name] < tol and r[name + "_pose"] < tol, (name, r)
    assert r["v_a_pad_abs"] == 0.0 and r["v_b_pad_abs"] == 0.0, "V^T padding must stay zero"
    if kw.get("ints"):
        assert r["v_exact_bad"] == 0, r


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kw", [dict(), dict(kv_shift=1), dict(n=768, S=2, heads=1, sharp=3.0), dict(n=12, sharp=6.0), dict(n=64),
                                dict(n=129, sharp=10.0, S=3, heads=1, kv_shift=2), dict(n=128, S=3), dict(n=127, sharp=3.0), dict(n=256, S=1, heads=3),
                                dict(n=255, S=1, heads=1)])
def test_attention_pose_token(G, prec, kw):
    r = G.check_attention_pose(prec, **kw)
    assert r["nan"] == 0, r
    assert r["rel_l2"] < TOL[prec] and r["rel_l2_pose"] < TOL[prec], r


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kw", [dict(), dict(kv_shift=1), dict(nq=70, nk=130, sharp=6.0),
                                dict(S=1, heads=1, nq=769, nk=769, sharp=3.0), dict(nq=1, nk=1), dict(nq=64, nk=64),
                                dict(nq=65, nk=129, sharp=10.0)])
def test_attention(G, prec, kw):
    r = G.check_attention(prec, **kw)
    assert r["nan"] == 0, r
    assert r["rel_l2"] < TOL[prec], r


def _conv_pixels(kw):
    s = kw.get("stride", 1)
    return kw.get("n", 2) * ((kw.get("H", 7) - 1) // s + 1) * ((kw.get("W_", 5) - 1) // s + 1)


@pytest.mark.parametrize("prec", HEAD_PRECS)
@pytest.mark.parametrize("kw", [dict(), dict(stride=2), dict(stride=2, H=6, W_=8),
                                dict(relu_in=1, act=2, resid=True, Cin=96, Co=256, H=9, W_=12), dict(H=1, W_=1),
                                # forced families 2 / 3 at <= 874 pixels: below the small-grid predicate, so these run family 6 (asserted
                                # below).  The implicit-GEMM loader on families 2 / 3 / 5 runs in test_conv_exact.py (tests/conv_cases.py)
                                dict(relu_in=1, act=2, resid=True, Cin=96, Co=256, H=19, W_=23, variant=2),
                                dict(Cin=64, Co=128, H=17, W_=9, variant=2), dict(stride=2, Cin=32, Co=256, H=15, W_=14, variant=2),
                                dict(relu_in=1, act=2, resid=True, Cin=96, Co=256, H=19, W_=23, variant=3), dict(Cin=64, Co=128, H=17, W_=9, variant=3),
                                # tiny grids with a long K loop: split-K partial sums + splitk_finish_kernel (SLAM-scale DPT levels)
                                dict(Cin=128, Co=64, H=6, W_=6), dict(relu_in=1, act=2, resid=True, Cin=256, Co=256, H=7, W_=7, n=3),
                                dict(stride=2, Cin=768, Co=256, H=14, W_=14, n=1)])
def test_conv3x3(G, prec, kw):
    r = G.check_conv3(prec, **kw)
    assert r["plan"]["family"] == small_shape_family(_conv_pixels(kw), kw.get("Co", 48), kw.get("variant", 0)), r
    assert r["plan"]["ksplit"] > 1 or kw.get("Cin", 32) < 128, r          # the three long-K cases do split K
    assert r["nan"] == 0, r
    assert r["rel_l2"] < TOL[prec], r


@pytest.mark.parametrize("prec", HEAD_PRECS)
@pytest.mark.parametrize("kw", [dict(Cin=32, Co=128, H=9, W_=40), dict(Cin=96, Co=256, H=19, W_=23, relu_in=1, act=2, resid=True),
                                dict(Cin=64, Co=128, H=8, W_=32, n=3), dict(Cin=128, Co=256, H=17, W_=64, n=1, relu_in=1),
                                dict(Cin=256, Co=128, H=3, W_=97, act=2), dict(Cin=32, Co=256, H=1, W_=1), dict(Cin=64, Co=128, H=30, W_=33, resid=True)])
def test_conv3x3_halo_tiles(G, prec, kw):
    """conv3h.h (forced with tile family 8): pixel tiles of 8 x 32 outputs, halo in LDS, image borders / ragged tiles /
    several channel blocks (double-buffered halo) / ReLU on fragments / residual planes."""
    r = G.check_conv3(prec, variant=8, **kw)
    assert (r["plan"]["family"], r["plan"]["bn"]) == (8, kw["Co"]), r
    assert r["nan"] == 0, r
    assert r["rel_l2"] < TOL[prec], r


@pytest.mark.parametrize("prec", HEAD_PRECS)
# (the first two variant=2 cases: 30 .. 198 input pixels, below the small-grid predicate - family 6 like the others, asserted below.
#  Above it - 2 x 55 x 56 = 6160 pixels x N = 4 x 192: 33 x 6 = 198 tiles of 192x128, the tiles span image rows and both images -
#  the scatter epilogue runs on the automatic choice and on the forced 256x256 / 192x256 / 192x128 tiles; k = 4 at Cdim = 96 as in
#  act_postprocess[0])
@pytest.mark.parametrize("kw", [dict(), dict(Cdim=192, k=2), dict(Cdim=192, k=2, variant=2), dict(Cdim=96, k=4, variant=2, H=9, W_=11),
                                dict(H=55, W_=56, Cdim=192, k=2, fam=5), dict(H=55, W_=56, Cdim=192, k=2, variant=2, fam=2),
                                dict(H=55, W_=56, Cdim=192, k=2, variant=3, fam=3), dict(H=55, W_=56, Cdim=192, k=2, variant=4, fam=5),
                                dict(H=37, W_=41, Cdim=96, k=4, variant=2, fam=2), dict(H=37, W_=41, Cdim=96, k=4, variant=3, fam=3)])
def test_convt(G, prec, kw):
    kw = dict(kw)
    fam = kw.pop("fam", None)
    r = G.check_convt(prec, **kw)
    M, N = kw.get("n", 2) * kw.get("H", 3) * kw.get("W_", 5), kw.get("k", 4) ** 2 * kw.get("Cdim", 96)
    if fam is None:
        fam = small_shape_family(M, N, kw.get("variant", 0))
    else:
        assert not small_grid(M, N) and M % 192 and M % 256 and (kw["H"] * kw["W_"]) % 192, kw
    assert r["plan"]["family"] == fam, r
    assert r["nan"] == 0, r
    assert r["rel_l2"] < TOL[prec], r


# the product's shapes: 256 channels between the refinenets, the cropped output of refinenet4 (odd sizes: 7 x 9 -> 13 x 17 of
# 14 x 18), 128 channels in front of head.2; 16 images of 64 (65) rows = 512 (528) groups of four output rows: where run_up2
# (sta_launch.inc) gives the split precisions four rows per workgroup (the last group of 129 rows partly filled) and precision f16
# one, and every precision one under experiment switch 7
@pytest.mark.parametrize("prec", HEAD_PRECS)
@pytest.mark.parametrize("kw", [dict(), dict(H=2, W_=3, crop=(3, 5)), dict(H=1, W_=1),
                                dict(Cdim=256, H=12, W_=16), dict(Cdim=256, H=7, W_=9, crop=(13, 17)), dict(Cdim=128, H=24, W_=20),
                                dict(Cdim=128, n=16, H=64, W_=10), dict(Cdim=256, n=16, H=65, W_=5, crop=(129, 9)),
                                dict(Cdim=128, n=16, H=64, W_=10, one_row=1)])
def test_up2(G, prec, kw):
    r = G.check_up2(prec, **kw)
    assert r["nan"] == 0, r
    assert r["rel_l2"] < TOL[prec], r
    # every border class under the whole-tensor bar: a rounding error that is iid over the elements has the same expected rel-L2 on
    # a class as on the whole
    assert r["worst"][1] < TOL[prec], r


@pytest.mark.parametrize("prec", HEAD_PRECS)
def test_up2_of_one_pixel_is_exact(G, prec):
    """x2 with align_corners has the weights j (H - 1) / (2 H - 1): odd denominators, so integer inputs give no dyadic results in
    general - except for a 1 x 1 image, whose four outputs ARE the input (integers an fp16 holds)."""
    r = G.check_up2(prec, n=3, H=1, W_=1, Cdim=64, ints=True)
    assert r["nan"] == 0 and r["exact_bad"] == 0, r


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", [128, 768, 1024])
def test_layernorm(G, prec, C):
    r = G.check_layernorm(prec, Cdim=C)
    assert r["f32"] < 1e-5, r
    assert r["planes"] < TOL[prec], r


@pytest.mark.parametrize("prec", HEAD_PRECS)
def test_reference_op_goldens(G, prec):
    """Vectors produced by the reference's own modules (RoPE2D, svd_orthogonalize, postprocess...)."""
    r = G.check_ops_golden(prec)
    assert r["rope2d"] < 1e-5 and r["rope2d_roundtrip"] < 1e-5, r
    assert r["rope2d_f16"] < 2e-3 and r["rope2d_f64"] < 1e-5, r        # fp16 storage: one ulp of the stored half
    assert r["layernorm"] < 1e-5, r
    assert r["svd_orth"] < 1e-5, r
    assert r["bilinear"] < TOL[prec], r
    assert r["post_pts"] < TOL[prec] * 5 and r["post_conf"] < TOL[prec] * 5, r


# Rows of the launch layer's dispatch table (sta_launch.inc: TileFamily x has_kernel) that no other kernel test launches, at the
# smallest shapes that reach them, each with the plan of the launch asserted.
# GELU and RoPE are no integer functions, so these rows keep the file's bars:
#   * GELU on 192x256 (forced 3) and on the register-staged kernel (forced 1) above the small-grid predicate, and on the 4-WAVE form
#     of the small-grid family: 641 rows x 5632 columns = 4 x 44 = 176 tiles of 192x128 (small grid), 6 x 88 = 528 workgroups of
#     128x64 (more than the 256 up to which the 8-wave form runs);
#   * the RoPE epilogue on the register-staged kernel (forced 1, the throughput shape of test_qkv_rope).
@pytest.mark.parametrize("prec,kw,fam", [(p, kw, fam) for p in PRECS for kw, fam in (
    (dict(M=6200, N=768, K=64, variant=3, act=1, via_f16=1), 3), (dict(M=6200, N=768, K=64, variant=1, act=1, via_f16=1), 1))] +
    [("f16x3", dict(M=641, N=5632, K=64, act=1, via_f16=1), 6)])
def test_gemm_dispatch_rows_gelu(G, prec, kw, fam):
    r = G.check_gemm(prec, **kw)
    assert (r["plan"]["family"], r["plan"]["ksplit"]) == (fam, 1), r
    assert fam != 6 or r["plan"]["tiles_m"] * r["plan"]["tiles_n"] > 256, r
    assert r["nan"] == 0, r
    assert r["rel_l2"] < TOL[prec], r


@pytest.mark.parametrize("prec", PRECS)
def test_qkv_rope_dispatch_row_register_staged(G, prec):
    r = G.check_qkv_rope(prec, hp=24, wp=32, pose_tok=0, S=4, K=64, Cdim=512, variant=1)
    assert (r["plan"]["family"], r["plan"]["ksplit"], r["plan"]["m_tail"]) == (1, 1, 0), r
    assert r["nan"] == 0, r
    assert r["q"] < TOL[prec] and r["k"] < TOL[prec] and r["v"] < TOL[prec], r
    assert r["vpad_abs"] == 0.0, r


# The transposed-convolution scatter is an integer function: exact, on integers as in test_dpt_varlen_kernels.py (inputs in [-3, 3],
# weights +-1, bias in [-32, 32]: |sum| <= 3 C + 32 <= 704, exact in every arithmetic), the output NaN before the launch.
#   * the register-staged kernel (forced 1) above the small-grid predicate: 2 x 55 x 56 = 6160 pixels x 4 x 192 columns;
#   * the 4-wave form of the small-grid family, split and f16mx operands: 2 x 16 x 20 = 640 pixels x 16 x 224 columns = 5 x 56 = 280
#     workgroups of 128x64, too many for K slices.
@pytest.mark.parametrize("prec,kw,fam", [("f16x3", dict(H=55, W_=56, Cdim=192, k=2, variant=1), 1), ("f16", dict(H=55, W_=56, Cdim=192, k=2, variant=1), 1),
                                         ("f16x3", dict(H=16, W_=20, Cdim=224, k=4), 6), ("head_mx", dict(H=16, W_=20, Cdim=224, k=4), 6)])
def test_convt_dispatch_rows_integer_exact(G, prec, kw, fam):
    import numpy as np
    import torch
    from vista_slam_amd import _lib
    n, H, W_, Cd, k, variant = 2, kw["H"], kw["W_"], kw["Cdim"], kw["k"], kw.get("variant", 0)
    rng = np.random.default_rng(11 + k)
    w = (rng.integers(0, 2, size=(Cd, Cd, k, k)) * 2 - 1).astype(np.float32)            # ConvTranspose2d layout [Cin, Cout, k, k]
    b = rng.integers(-32, 33, size=Cd).astype(np.float32)
    x = rng.integers(-3, 4, size=(n, H, W_, Cd)).astype(np.float32)
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double(),
                                                torch.from_numpy(b).double(), stride=k).permute(0, 2, 3, 1).numpy()
    assert np.abs(want).max() <= 3 * Cd + 32 < 2048
    m, lib, h = G.kernel_handle(prec, variant)
    out = torch.full((n, H * k, W_ * k, Cd), float("nan"), device=G.DEV)
    xd, wd, bd = G.dev(x), G.dev(w), G.dev(b)
    try:
        _lib.check(lib.sta_debug_convt(h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), n, H, W_, Cd, k, out.data_ptr(), G.st()))
        torch.cuda.synchronize()
        plan = G.last_plan(lib, h)
    finally:
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    assert (plan["family"], plan["ksplit"], plan["m_tail"]) == (fam, 1, 0), plan
    assert fam != 6 or plan["tiles_m"] * plan["tiles_n"] > 256, plan
    got = out.cpu().numpy().astype(np.float64)
    bad = np.argwhere(~(got == want))
    assert len(bad) == 0, f"{len(bad)} wrong elements ({int(np.isnan(got).sum())} NaN), first (image, y, x, channel) {bad[:4].tolist()}"
