"""GPU: the DPT head's 3x3 convolutions (gemm2.h A_CONV3, conv3h.h) and the fused tail (EPI_HEAD), exactly and per pixel class.

The cases are tests/conv_cases.py (one table; tests/test_conv_plan.py proves on the host that it holds every class a product launch
can reach).  Every test asserts the class its launch RAN under (sta_debug_last_gemm_plan: family, tile, K slices) and nan == 0: the
debug entries poison the output planes / the four tail outputs, so an element that was never stored is a NaN.

1. tap selection (bit exact; f16x3, f16, f16mx): integer inputs that carry their own address (plane 4j = y, 4j + 1 = x, 4j + 2 = image,
   4j + 3 = group j) and one-hot weights - output channel co selects one (tap, input channel), every (tap, 32-channel input block)
   pair used.  The output must EQUAL the shifted input plane, 0 outside the image.  A failure names the output pixel, the channel,
   the source pixel expected and the value found, which decodes to the pixel actually read.  With an input ReLU every second group of
   planes is offset by -40, so the ReLU clamps there.
2. integer sums (bit exact): small integer inputs, weights (+-1, at most 512 per output channel), bias and residuals; every exact
   output is an integer of magnitude <= 2048 by construction (asserted in int64 before the launch).  fp16 holds every operand and
   result, fp32 every partial sum: all three arithmetics must return the integer itself.
3. Gaussian inputs against a float64 reference of the same convolution: rel-L2 of the whole tensor under the bars of
   test_gpu_kernels.py and of each class - four corners, each border, interior, the ragged last tile column / row (or the last
   tile of the flattened pixels), first and last row of every image after the first, every 32-channel output block.
4. the fused tail through sta_debug_conv3_head, halo form (forced family 8) and implicit GEMM on 192x128 (variant 9), the split nA
   between the two output pairs at 0, 1, n - 1, n, head.4 at ordinary and at 1e-5 scale: pts and conf per pixel class against
   float64, and an exact case - one-hot head.2, integer head.4, the four pre-activations known integers in [-3, 3] - compared with
   the float64 activations of those integers in ulps of the fp32 result.

Bounds of 3 and 4 = 4 x the worst class of a numpy model of the documented arithmetic (helpers.conv_model / tail_model: f16x3 =
operands as fp16 hi + lo, three products, fp32 accumulation, hi + lo output; f16 = single fp16 roundings) run on the CPU on the
same inputs against the same float64 reference; the factor 4 covers the summation order of the MFMAs and of the K slices.  Model
figures (worst class over all cases, the case and class that set it); test_conv_plan.py::test_class_bounds_come_from_the_model
recomputes them:

    group   arithmetic   model worst class   case, class                              bound (4 x)
    conv    f16x3        4.195e-07           s6_sk_s2_even, channels_480_511          1.68e-06
    conv    f16          3.934e-04           h128_plain_c256, corner_bl               1.57e-03
    pts     f16x3        1.402e-06           t8_w64, corner_br                        5.61e-06
    pts     f16          7.791e-04           t8_w64, corner_br                        3.12e-03
    conf    f16x3        1.394e-07           t8_w48, image1_last_row                  5.58e-07
    conf    f16          8.482e-05           t8_w48, corner_tr                        3.39e-04

f16mx ("head_mx") has no model here (the fp8 correction's error depends on block scales): every class of 3 and
every pts / conf class of 4 uses the whole-tensor bar of test_gpu_kernels.py, 6e-5 - an iid error has the same expected rel-L2 on a
class as on the whole.  This bound is NOT model-derived.

Exact tail, the ulp counts: d = sqrtf(x^2 + y^2 + z^2) is a correctly rounded square root of an exact integer (0.5 ulp), which
expm1(d) / d sees with sensitivity d / (1 - e^-d) - 1 <= 3.74 at d <= sqrt(22) (x in [-1, 3], y in [-3, 1], z in [-2, 2]): 1.87 ulp;
expm1f 1 ulp, the division 0.5 ulp (2.5 when not correctly rounded), the product with x 0.5 ulp: at most 5.87, asserted as 6.
conf = 1 + expf(c): expf 1 ulp, the sum 0.5 ulp: asserted as 2.

Measured on the MI355X (worst class over all cases): conv 5.5e-7 (f16x3), 3.9e-4 (f16), 2.2e-5 (f16mx); tail pts 1.8e-6 / 7.8e-4 /
1.5e-5, conf 1.5e-7 / 8.5e-5 / 3.5e-6; exact tail 2.6 ulp (pts), 0.4 ulp (conf).
"""
import pytest

import conv_cases as CC

pytestmark = pytest.mark.gpu

# (group, arithmetic) -> (model worst class, case that sets it); the bound is 4 x the figure
MODEL = {("conv", "f16x3"): (4.195e-07, "s6_sk_s2_even"),
         ("conv", "f16"): (3.934e-04, "h128_plain_c256"),
         ("pts", "f16x3"): (1.402e-06, "t8_w64"),
         ("pts", "f16"): (7.791e-04, "t8_w64"),
         ("conf", "f16x3"): (1.394e-07, "t8_w48"),
         ("conf", "f16"): (8.482e-05, "t8_w48")}
GLOBAL_TOL = {"f16x3": 2e-5, "f16": 3e-3, "head_mx": 6e-5}          # the whole-tensor bounds of test_gpu_kernels.py
PTS_ULPS, CONF_ULPS = 6.0, 2.0


def class_bound(group, prec):
    return 4.0 * MODEL[(group, prec)][0]


def model_conv_worst(case, prec):
    """(class, error) of the model's worst class on the Gaussian inputs of test_gaussian_classes."""
    import helpers as HP
    cid, n, H, W, Cin, Co, stride, relu_in, act, nres, variant, cls = case
    x, w, b, res = HP.conv_gaussian_inputs(n, H, W, Cin, Co, stride, nres, 32)
    Ho, Wo = CC.out_size(H, W, stride)
    masks = HP.conv_pixel_classes(n, Ho, Wo, cls[0], {2: 256, 3: 192, 5: 192, 6: 128, 8: 256}[cls[0]])
    errs = HP.class_errors(HP.conv_model(x, w, b, stride, relu_in, act, res, prec), HP.conv_ref64(x, w, b, stride, relu_in, act, res), masks)
    return HP.worst_class(errs)


def model_tail_worst(hcase, prec):
    import helpers as HP
    cid, n, H, W, variant, w4scale, cls = hcase
    ins = HP.tail_gaussian_inputs(n, H, W, w4scale)
    (mp, mc), (rp, rc) = HP.tail_model(*ins, prec), HP.tail_ref64(*ins)
    masks = HP.conv_pixel_classes(n, H, W, cls[0], 256 if cls[0] == 8 else 192)
    return {"pts": HP.worst_class(HP.class_errors(mp, rp, masks, channel_blocks=False)),
            "conf": HP.worst_class(HP.class_errors(mc[..., None], rc[..., None], masks, channel_blocks=False))}


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    return gpu_checks


IDS = [c[0] for c in CC.CASES]
HEAD_IDS = [c[0] for c in CC.HEAD_CASES]


@pytest.mark.parametrize("prec", CC.ARITHMETICS)
@pytest.mark.parametrize("case", CC.CASES, ids=IDS)
def test_tap_selection_is_bit_exact(G, prec, case):
    r = G.check_conv_selection(prec, case)
    print(case[0], prec, {k: r[k] for k in ("class", "nan", "wrong")})
    assert r["class"] == case[11], r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong elements ({r['nan']} NaN); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec", CC.ARITHMETICS)
@pytest.mark.parametrize("case", CC.CASES, ids=IDS)
def test_integer_sums_are_bit_exact(G, prec, case):
    r = G.check_conv_integers(prec, case)
    print(case[0], prec, {k: r[k] for k in ("class", "nan", "wrong", "max_abs")})
    assert r["class"] == case[11], r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong elements ({r['nan']} NaN); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec", CC.ARITHMETICS)
@pytest.mark.parametrize("case", CC.CASES, ids=IDS)
def test_gaussian_classes(G, prec, case):
    r = G.check_conv_classes(prec, case)
    bound = GLOBAL_TOL["head_mx"] if prec == "head_mx" else class_bound("conv", prec)
    print(case[0], prec, r["class"], "rel_l2", r["rel_l2"], "worst", r["worst"], "bound", bound)
    assert r["class"] == case[11], r["class"]
    assert r["nan"] == 0, r
    assert r["rel_l2"] < GLOBAL_TOL[prec], r
    assert r["worst"][1] < bound, (r["worst"], bound, r["errs"])


def _tail_bounds(prec):
    """(pts bound, conf bound) of the fused-tail classes (module docstring)."""
    if prec == "head_mx":
        return GLOBAL_TOL["head_mx"], GLOBAL_TOL["head_mx"]
    return class_bound("pts", prec), class_bound("conf", prec)


@pytest.mark.parametrize("prec", CC.ARITHMETICS)
@pytest.mark.parametrize("hcase", CC.HEAD_CASES, ids=HEAD_IDS)
def test_fused_tail_classes(G, prec, hcase):
    for nA in CC.tail_splits(hcase[1]):
        r = G.check_tail_classes(prec, hcase, nA)
        bp, bc = _tail_bounds(prec)
        print(hcase[0], prec, "nA", nA, r, "bounds", bp, bc)
        assert r["class"] == hcase[6], r["class"]
        assert r["nan"] == 0, (nA, r)
        assert r["worst_pts"][1] < bp, f"nA = {nA}: pts, worst class {r['worst_pts']} against {bp}"
        assert r["worst_conf"][1] < bc, f"nA = {nA}: conf, worst class {r['worst_conf']} against {bc}"


@pytest.mark.parametrize("prec", CC.ARITHMETICS)
@pytest.mark.parametrize("hcase", CC.HEAD_CASES, ids=HEAD_IDS)
def test_fused_tail_on_known_integers(G, prec, hcase):
    for nA in CC.tail_splits(hcase[1]):
        r = G.check_tail_exact(prec, hcase, nA)
        print(hcase[0], prec, "nA", nA, r)
        assert r["class"] == hcase[6], r["class"]
        assert r["nan"] == 0, (nA, r)
        assert r["pts_ulp"] <= PTS_ULPS, (nA, r["pts_ulp"], r["pts_worst"])
        assert r["conf_ulp"] <= CONF_ULPS, (nA, r["conf_ulp"], r["conf_worst"])
