"""The GPU case matrix of tests/test_conv_exact.py as plain data (no torch, no numpy), so that the host-only coverage test
(tests/test_conv_plan.py) can import it.

A CLASS names the code path a 3x3 convolution launch of the DPT head runs (sta_launch.inc: gemm_plan / launch_gemm):

    (family, tile columns, epilogue, K steps, stride, split-K)

    family      2 / 3 / 5: implicit GEMM (A_CONV3 loader of gemm2.h) on 256x256 / 192x256 / 192x128 tiles of FLATTENED pixels, which
                cross image rows and image boundaries; 6: the same loader on 128x64 tiles (small grids); 8: the halo-tiled kernel
                (conv3h.h: 8 x 32 pixels of one image)
    columns     bn of the plan (family 8: 128 = two taps per K step, the fused tail's tile; 256 = one tap per step)
    epilogue    "plain", "relu" (ReLU on the input AND the output: resConfUnit.conv1), "r1" / "r2" (one / two residual planes),
                "head" (EPI_HEAD: the fused DPT tail)
    K steps     family 8 on 128 columns pairs the 9 Cin / 32 taps: "even", or "odd" (a last step of one tap); "-" elsewhere
    stride      1 | 2
    split-K     1: the small-grid family splits K into fp32 slabs and splitk_finish_kernel applies the epilogue

The arithmetic (f16x3, f16, f16mx = "head_mx") is the seventh coordinate; every case runs in all three.

A case: (id, n, H, W, Cin, Co, stride, relu_in, act, residuals, forced variant, class).  The class is what the case CLAIMS: the GPU
tests assert family, tile and K slices against the plan of the launch (sta_debug_last_gemm_plan), tests/test_conv_plan.py against
sta_debug_conv_plan.  Families 2 / 3 / 5 are forced (variant 2 / 3 / 4) at 2 x 100 x 97 = 19400 pixels x 256 channels: above the
small-grid predicate (M <= 640 or ceil(M / 192) ceil(N / 128) < 192), below which a forced family never displaces family 6;
19400 and 100 x 97 = 9700 are multiples of neither 192 nor 256, so tiles end inside image rows and span the two images.
"""

FIELDS = ("family", "bm", "bn", "m_tail", "tiles_m", "tiles_n", "ksplit", "slab_ks")
PLAIN, RELU, R1, R2 = (0, 0, 0), (1, 2, 0), (0, 0, 1), (0, 0, 2)
EPI_NAME = {PLAIN: "plain", RELU: "relu", R1: "r1", R2: "r2", (0, 2, 0): "relu_out"}


def out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def small_grid(M, N):
    """The small-grid predicate (sta_launch.inc: small_grid_m), restated."""
    return M <= 640 or ((M + 191) // 192) * ((N + 127) // 128) < 192


def conv_class(plan, Cin, stride, epi):
    """plan: dict of FIELDS -> the class tuple.  epi: a name of EPI_NAME or "head"."""
    fam, bn = plan["family"], plan["bn"]
    ksteps = ("odd" if (9 * (Cin // 32)) % 2 else "even") if fam == 8 and bn == 128 else "-"
    return (fam, bn, epi, ksteps, stride, 1 if plan["ksplit"] > 1 else 0)


def _c(cid, n, H, W, Cin, Co, stride, epi, variant, fam, bn, ksteps="-", splitk=0):
    return (cid, n, H, W, Cin, Co, stride, epi[0], epi[1], epi[2], variant, (fam, bn, EPI_NAME[epi], ksteps, stride, splitk))


CASES = [
    # ---- implicit GEMM on the throughput tiles: 2 x 100 x 97 pixels, Cout = 256
    _c("g2_plain_c32", 2, 100, 97, 32, 256, 1, PLAIN, 2, 2, 256),
    _c("g2_relu_c64", 2, 100, 97, 64, 256, 1, RELU, 2, 2, 256),
    _c("g2_r1_c32", 2, 100, 97, 32, 256, 1, R1, 2, 2, 256),
    _c("g2_r2_c96", 2, 100, 97, 96, 256, 1, R2, 2, 2, 256),
    _c("g3_plain_c96", 2, 100, 97, 96, 256, 1, PLAIN, 3, 3, 256),
    _c("g3_relu_c32", 2, 100, 97, 32, 256, 1, RELU, 3, 3, 256),
    _c("g3_r1_c64", 2, 100, 97, 64, 256, 1, R1, 3, 3, 256),
    _c("g3_r2_c32", 2, 100, 97, 32, 256, 1, R2, 3, 3, 256),
    _c("g5_plain_c64", 2, 100, 97, 64, 256, 1, PLAIN, 4, 5, 128),
    _c("g5_relu_c96", 2, 100, 97, 96, 256, 1, RELU, 4, 5, 128),
    _c("g5_r1_c32", 2, 100, 97, 32, 256, 1, R1, 4, 5, 128),
    _c("g5_r2_c64", 2, 100, 97, 64, 256, 1, R2, 4, 5, 128),
    # the product's own K loop on these families: Cin = 256 (K = 2304, the length pick_family keys on)
    _c("g2_relu_c256", 2, 100, 97, 256, 256, 1, RELU, 2, 2, 256),
    _c("g3_r1_c256", 2, 100, 97, 256, 256, 1, R1, 3, 3, 256),
    _c("g5_r2_c256", 2, 100, 97, 256, 256, 1, R2, 4, 5, 128),
    # stride 2 on 192x128, even and odd input sizes (both -> 100 x 97 outputs)
    _c("g5_s2_even", 2, 200, 194, 32, 256, 2, PLAIN, 4, 5, 128),
    _c("g5_s2_odd", 2, 199, 193, 32, 256, 2, PLAIN, 4, 5, 128),
    # Cout = 128 (head.0's width) needs 36673 pixels: 5 x 89 x 83 = 36935
    _c("g5_co128", 5, 89, 83, 32, 128, 1, PLAIN, 4, 5, 128),
    # ---- small grids (family 6), with and without K slices; stride 2 (act_postprocess[3] is Cin = Co = 768)
    _c("s6_plain", 2, 7, 5, 32, 64, 1, PLAIN, 0, 6, 64),
    _c("s6_one_pixel", 2, 1, 1, 64, 128, 1, R1, 0, 6, 64),
    _c("s6_one_row", 3, 1, 37, 96, 256, 1, RELU, 0, 6, 64),
    _c("s6_sk_relu", 3, 7, 7, 256, 256, 1, RELU, 0, 6, 64, splitk=1),
    _c("s6_sk_r1", 2, 9, 12, 128, 256, 1, R1, 0, 6, 64, splitk=1),
    _c("s6_sk_r2", 2, 14, 14, 256, 256, 1, R2, 0, 6, 64, splitk=1),
    _c("s6_sk_plain_c768", 2, 7, 7, 768, 256, 1, PLAIN, 0, 6, 64, splitk=1),
    _c("s6_sk_s2_even", 1, 14, 14, 768, 768, 2, PLAIN, 0, 6, 64, splitk=1),
    _c("s6_sk_s2_odd", 2, 13, 15, 768, 768, 2, PLAIN, 0, 6, 64, splitk=1),
    _c("s6_s2_odd_even", 2, 7, 10, 32, 64, 2, PLAIN, 0, 6, 64),
    _c("s6_r2", 2, 9, 11, 64, 128, 1, R2, 0, 6, 64),
    _c("s6_forced2", 2, 19, 23, 96, 256, 1, R1, 2, 6, 64),            # a forced family never displaces the small-grid one
    # the 4-WAVE form of family 6 (every case above runs at most 256 workgroups, i.e. the 8-wave form in the split arithmetics):
    # 2 x 130 x 130 = 33800 pixels at Cout = 64 are 177 tiles of 192x128 - a small grid - and 265 workgroups of 128x64, too many
    # for K slices (tests/test_conv_plan.py asserts the count)
    _c("s6_four_waves", 2, 130, 130, 32, 64, 1, R1, 0, 6, 64),
    # ---- halo-tiled kernel (family 8, forced): W % 32 in {0, 1, 16, 31}, H % 8 != 0, every tap count parity
    # 256 columns: one tap per K step
    _c("h256_plain_w32", 2, 9, 32, 32, 256, 1, PLAIN, 8, 8, 256),
    _c("h256_relu_w33", 2, 11, 33, 96, 256, 1, RELU, 8, 8, 256),
    _c("h256_r1_w48", 3, 13, 48, 64, 256, 1, R1, 8, 8, 256),
    _c("h256_r2_w63", 2, 5, 63, 256, 256, 1, R2, 8, 8, 256),
    # 128 columns: two taps per K step
    _c("h128_plain_c32", 2, 9, 33, 32, 128, 1, PLAIN, 8, 8, 128, "odd"),
    _c("h128_relu_c96", 2, 13, 63, 96, 128, 1, RELU, 8, 8, 128, "odd"),
    _c("h128_r1_c64", 3, 11, 48, 64, 128, 1, R1, 8, 8, 128, "even"),
    _c("h128_plain_c256", 2, 9, 64, 256, 128, 1, PLAIN, 8, 8, 128, "even"),
    _c("h128_r2_c128", 2, 17, 31, 128, 128, 1, R2, 8, 8, 128, "even"),
    _c("h128_one_pixel", 2, 1, 1, 32, 128, 1, PLAIN, 8, 8, 128, "odd"),
    _c("h256_one_row", 2, 1, 70, 64, 256, 1, RELU, 8, 8, 256),
]

# the arithmetics of tests/gpu_checks.py: kernel_handle
ARITHMETICS = ("f16x3", "f16", "head_mx")
# (test arithmetic) -> (precision id of sta_debug_conv_plan, mx): the plan each launch must report
PLAN_ARGS = {"f16x3": (3, 0), "f16": (1, 0), "head_mx": (5, 1)}

# ---- the fused DPT tail (sta_debug_conv3_head): (id, n, H, W, forced variant, scale of head.4's weights, class)
# halo form: forced family 8 at any size; implicit GEMM on 192x128: variant 9 ("automatic without the halo kernel") above the
# small-grid predicate, i.e. from 36673 pixels on.  Every case runs with nA in TAIL_SPLITS(n).
HEAD_CASES = [
    ("t8_w48", 3, 13, 48, 8, 1.0, (8, 128, "head", "even", 1, 0)),
    ("t8_w33_tiny_w4", 2, 9, 33, 8, 1e-5, (8, 128, "head", "even", 1, 0)),
    ("t8_w64", 2, 11, 64, 8, 1.0, (8, 128, "head", "even", 1, 0)),
    ("t8_w31_tiny_w4", 2, 5, 31, 8, 1e-5, (8, 128, "head", "even", 1, 0)),
    ("t5_w80", 6, 80, 80, 9, 1.0, (5, 128, "head", "-", 1, 0)),
    ("t5_w64_tiny_w4", 10, 61, 64, 9, 1e-5, (5, 128, "head", "-", 1, 0)),
]


def tail_splits(n):
    """nA: the split between the two output pairs on an image boundary at both ends and next to both ends."""
    return sorted({0, 1, n - 1, n})


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def covered_classes():
    return {c[11] for c in CASES} | {c[6] for c in HEAD_CASES}


# ---- what the product launches: the 3x3 convolutions of dpt_impl (sta_forward.inc) on n images of H x W
def product_convs(n, H, W):
    """-> [(name, images, Hin, Win, Cin, Co, stride, epilogue name)] in launch order; head.2 is the fused tail when conv3_head_ok
    (the caller decides: "head" here, "relu_out" for the unfused path)."""
    hp, wp = H // 16, W // 16
    h3, w3 = (hp - 1) // 2 + 1, (wp - 1) // 2 + 1
    Hs, Ws, Cs = (4 * hp, 2 * hp, hp, h3), (4 * wp, 2 * wp, wp, w3), (96, 192, 384, 768)
    L = [("act_postprocess3.1", n, hp, wp, 768, 768, 2, "plain")]
    for k in (3, 2, 1, 0):
        L.append((f"layer_rn{k}", n, Hs[k], Ws[k], Cs[k], 256, 1, "plain"))
        if k < 3:
            L.append((f"refinenet{k}.rcu1.conv1", n, Hs[k], Ws[k], 256, 256, 1, "relu"))
    for k in (3, 2, 1, 0):
        if k < 3:
            L.append((f"refinenet{k}.rcu1.conv2", n, Hs[k], Ws[k], 256, 256, 1, "r2"))
        L.append((f"refinenet{k}.rcu2.conv1", n, Hs[k], Ws[k], 256, 256, 1, "relu"))
        L.append((f"refinenet{k}.rcu2.conv2", n, Hs[k], Ws[k], 256, 256, 1, "r1"))
    L.append(("head.0", n, H // 2, W // 2, 256, 128, 1, "plain"))
    L.append(("head.2", n, H, W, 128, 128, 1, "head"))
    return L


PRODUCT_BATCHES = (1, 2, 4, 8)                       # pairs: the head runs on 2 B images
PRODUCT_SIZES = ((224, 224), (384, 512), (512, 384))
PRODUCT_PRECISIONS = {"f16x3": (3, 0), "f16x3h": (5, 1), "f16x3m": (6, 1)}     # -> (precision id, f16mx in the head)
