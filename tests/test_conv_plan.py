"""CPU: the launch plans of the DPT head's 3x3 convolutions, and what the case table of tests/conv_cases.py covers.

sta_debug_conv_plan (test-hooks build; sta_launch.inc: gemm_plan with the implicit-GEMM loader and the image geometry, so that the
halo-tiled family 8 is a candidate) needs the built library but no GPU.
  * every case of the table plans the class it claims, in each of the three arithmetics it runs in;
  * the table holds what it was built to hold (tiles that span image rows and images, ragged halo tiles, every tap-count parity,
    stride 2 on even and odd sizes, every epilogue, one-pixel and one-row images);
  * every class a product launch can reach - the convolutions of dpt_impl for 1, 2, 4, 8 pairs at 224x224, 384x512, 512x384 in the
    three split precisions - is represented by at least one case;
  * the bounds of tests/test_conv_exact.py are 4 x the figures of the numpy model of the arithmetic (helpers.conv_model /
    tail_model), recomputed here on the cases that set them.
"""
import ctypes as C
import os

import pytest

import conv_cases as CC

EPI_F16, EPI_HEAD = 1, 6


def _load_lib():
    from vista_slam_amd import _lib
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libsta_mi355_test.so not built here (python -m vista_slam_amd.build)")
    return _lib.load_test()


@pytest.fixture(scope="module")
def lib():
    return _load_lib()


def plan(lib, epi, M, N, K, prec, mx, forced, stride, Ho, Wo, head_gemm=0):
    out = (C.c_int * 8)()
    rc = lib.sta_debug_conv_plan(epi, M, N, K, prec, mx, forced, stride, Ho, Wo, head_gemm, out)
    assert rc == 0, (epi, M, N, K, prec, mx, forced, stride, Ho, Wo, lib.sta_last_error())
    return dict(zip(CC.FIELDS, out))


def test_every_case_plans_the_class_it_names(lib):
    for cid, n, H, W, Cin, Co, stride, relu_in, act, nres, variant, cls in CC.CASES:
        Ho, Wo = CC.out_size(H, W, stride)
        for arith, (prec, mx) in CC.PLAN_ARGS.items():
            p = plan(lib, EPI_F16, n * Ho * Wo, Co, 9 * Cin, prec, mx, variant, stride, Ho, Wo)
            assert CC.conv_class(p, Cin, stride, CC.EPI_NAME[(relu_in, act, nres)]) == cls, (cid, arith, p)
            assert (p["tiles_n"] - 1) * p["bn"] < Co <= p["tiles_n"] * p["bn"], (cid, p)
    for cid, n, H, W, variant, w4scale, cls in CC.HEAD_CASES:
        assert variant == 8 or not CC.small_grid(n * H * W, 128), (cid, "conv3_head_ok would be false: the unfused path")
        for arith, (prec, mx) in CC.PLAN_ARGS.items():
            p = plan(lib, EPI_HEAD, n * H * W, 128, 9 * 128, prec, mx, variant, 1, H, W)
            assert CC.conv_class(p, 128, 1, "head") == cls, (cid, arith, p)


def test_forced_families_need_a_shape_above_the_small_grid_predicate(lib):
    """What the convolution cases of test_gpu_kernels.py ran into: below the predicate a forced family 2 / 3 / 4 runs family 6."""
    for forced in (2, 3, 4):
        assert plan(lib, EPI_F16, 2 * 19 * 23, 256, 9 * 96, 3, 0, forced, 1, 19, 23)["family"] == 6
        assert plan(lib, EPI_F16, 2 * 100 * 97, 256, 9 * 96, 3, 0, forced, 1, 100, 97)["family"] == {2: 2, 3: 3, 4: 5}[forced]
    assert plan(lib, EPI_F16, 2 * 19 * 23, 256, 9 * 96, 3, 0, 8, 1, 19, 23)["family"] == 8     # only the halo form is really forced


def test_table_reaches_both_wave_forms_of_the_small_grid_family(lib):
    """Family 6 runs on 8 waves up to 256 workgroups (K slices included) and on 4 waves beyond (sta_launch.inc: gemm_plan, FAM6 /
    FAM6_LONE; plain f16 has the 4-wave form only): the table holds unsplit cases on both sides of that count."""
    wgs = {}
    for cid, n, H, W, Cin, Co, stride, relu_in, act, nres, variant, cls in CC.CASES:
        if cls[0] != 6:
            continue
        Ho, Wo = CC.out_size(H, W, stride)
        for arith, (prec, mx) in CC.PLAN_ARGS.items():
            p = plan(lib, EPI_F16, n * Ho * Wo, Co, 9 * Cin, prec, mx, variant, stride, Ho, Wo)
            wgs[(cid, arith)] = p["tiles_m"] * p["tiles_n"] * p["ksplit"]
    for arith in CC.PLAN_ARGS:
        assert wgs[("s6_four_waves", arith)] == 265, wgs
        assert any(w <= 256 for (cid, a), w in wgs.items() if a == arith and cid != "s6_four_waves"), wgs
    assert all(w <= 256 for (cid, a), w in wgs.items() if cid != "s6_four_waves"), wgs


def test_conv_plan_sweep_invariants(lib):
    """gemm_plan on the convolution loader over host-only shapes (the dense sweep is tests/test_gemm_plan.py): every plan names a
    kernel that exists (the call fails otherwise), tiles the output exactly, keeps the small-grid family under forced 2 / 3 / 4,
    runs the halo form only where it is legal, never under variant 9, and always where it is forced and legal."""
    tile = {1: (128, 128), 2: (256, 256), 3: (192, 256), 5: (192, 128), 6: (128, 64)}
    count = 0
    for arith, (prec, mx) in CC.PLAN_ARGS.items():
        for Co in (64, 128, 256, 768):
            for Cin in (32, 96, 256, 768):
                for stride in (1, 2):
                    for n, H, W in ((1, 1, 1), (2, 7, 5), (3, 14, 14), (2, 28, 28), (2, 100, 97), (6, 80, 80), (16, 112, 112), (4, 192, 256)):
                        Ho, Wo = CC.out_size(H, W, stride)
                        M = n * Ho * Wo
                        for forced in (0, 2, 3, 4, 8, 9):
                            p = plan(lib, EPI_F16, M, Co, 9 * Cin, prec, mx, forced, stride, Ho, Wo)
                            q = (arith, Co, Cin, stride, n, H, W, forced, p)
                            fam = p["family"]
                            legal8 = stride == 1 and Co in (128, 256)
                            if fam == 8:
                                assert legal8 and forced != 9 and forced not in (2, 3, 4), q
                                assert (p["bm"], p["bn"]) == (256, Co) and p["tiles_m"] == n * ((Ho + 7) // 8) * ((Wo + 31) // 32), q
                            else:
                                assert (p["bm"], p["bn"]) == tile[fam] and (p["tiles_m"] - 1) * p["bm"] < M <= p["tiles_m"] * p["bm"], q
                            assert (p["tiles_n"] - 1) * p["bn"] < Co <= p["tiles_n"] * p["bn"] and p["m_tail"] == 0, q
                            if forced == 8 and legal8:
                                assert fam == 8, q
                            elif CC.small_grid(M, Co):
                                assert fam == 6, q
                            elif forced in (2, 3) and Co % 256 == 0:
                                assert fam == forced, q
                            elif forced in (2, 3, 4) and Co % 128 == 0:
                                assert fam == 5, q
                            if fam != 6:
                                assert p["ksplit"] == 1 and p["slab_ks"] == 0, q
                            count += 1
    assert count > 4000


def test_table_holds_the_edges_it_was_built_for():
    by_fam = {}
    for c in CC.CASES:
        by_fam.setdefault(c[11][0], []).append(c)
    for fam, bm in ((2, 256), (3, 192), (5, 192)):
        assert by_fam[fam], fam
        for cid, n, H, W, Cin, Co, stride, *_ in by_fam[fam]:
            Ho, Wo = CC.out_size(H, W, stride)
            M = n * Ho * Wo
            assert not CC.small_grid(M, Co), cid
            assert n >= 2 and M % 192 and M % 256 and (Ho * Wo) % bm, (cid, "tiles must end inside image rows and span images")
        assert {c[11][2] for c in by_fam[fam]} >= {"plain", "relu", "r1", "r2"}, fam
        assert {c[4] for c in by_fam[fam]} >= {32, 256}, fam                                    # Cin = 256: the product's K loop
    assert {(c[2] % 2, c[3] % 2) for c in by_fam[5] if c[6] == 2} >= {(0, 0), (1, 1)}          # stride 2, even and odd sizes
    assert {(c[2] % 2, c[3] % 2) for c in by_fam[6] if c[6] == 2} >= {(0, 0), (1, 1)}
    assert any(c[4] == 768 and c[5] == 768 and c[6] == 2 for c in by_fam[6])                    # act_postprocess[3]
    assert {c[11][5] for c in by_fam[6]} == {0, 1}                                              # with and without K slices
    for bn in (128, 256):
        h = [c for c in by_fam[8] if c[11][1] == bn]
        assert {c[3] % 32 for c in h} >= {0, 1, 16, 31}, bn
        assert {c[11][2] for c in h} >= {"plain", "relu", "r1", "r2"}, bn
        assert sum(1 for c in h if c[2] % 8) >= 4, bn
    assert {c[4] for c in by_fam[8] if c[11][1] == 128} >= {32, 64, 96, 256}                    # 9, 18, 27, 72 taps, two per K step
    assert {c[11][3] for c in by_fam[8] if c[11][1] == 128} == {"odd", "even"}
    assert any(c[2] == 1 and c[3] == 1 for c in CC.CASES) and any(c[2] == 1 and c[3] > 32 for c in CC.CASES)
    assert {c[3] % 32 for c in CC.HEAD_CASES if c[4] == 8} >= {0, 16} and {c[3] % 32 for c in CC.HEAD_CASES if c[4] == 9} >= {0, 16}
    assert {c[5] for c in CC.HEAD_CASES} == {1.0, 1e-5}


def product_classes(lib):
    """{class: first (launch, pairs, size, precision) that reaches it} over the convolutions of dpt_impl."""
    reached = {}
    for B in CC.PRODUCT_BATCHES:
        for H, W in CC.PRODUCT_SIZES:
            for pname, (prec, mx) in CC.PRODUCT_PRECISIONS.items():
                for name, n, Hi, Wi, Cin, Co, stride, epi in CC.product_convs(2 * B, H, W):
                    Ho, Wo = CC.out_size(Hi, Wi, stride)
                    M = n * Ho * Wo
                    if epi == "head" and CC.small_grid(M, Co):      # conv3_head_ok: the unfused path, conv + ReLU to planes
                        epi = "relu_out"
                    p = plan(lib, EPI_HEAD if epi == "head" else EPI_F16, M, Co, 9 * Cin, prec, mx, 0, stride, Ho, Wo)
                    reached.setdefault(CC.conv_class(p, Cin, stride, epi), (name, B, (H, W), pname))
    return reached


def test_every_class_the_product_reaches_has_a_case(lib):
    reached = product_classes(lib)
    assert len(reached) >= 26, reached                # today: 26 classes (6 on families 2 / 3, 4 on 5, 10 on 6, 6 on 8)
    missing = {c: w for c, w in reached.items() if c not in CC.covered_classes()}
    assert not missing, f"classes a product launch runs that no case of tests/conv_cases.py covers: {missing}"
    # the fused tail: the halo form on the product path; its implicit-GEMM form (what forced variant 9 runs in HEAD_CASES) only
    # under experiment switch 0, from 2^21 pixels on
    assert {c[0] for c in reached if c[2] == "head"} == {8}, reached
    M = 16 * 512 * 384
    assert plan(lib, EPI_HEAD, M, 128, 9 * 128, 5, 1, 0, 1, 512, 384, head_gemm=0)["family"] == 8
    assert plan(lib, EPI_HEAD, M, 128, 9 * 128, 5, 1, 0, 1, 512, 384, head_gemm=1)["family"] == 5


def test_class_bounds_come_from_the_model():
    """The figures in the tables of test_conv_exact.py are the numpy model's worst class on the named case (within a factor of 2: the
    model's own fp32 summation order depends on the convolution library underneath)."""
    import helpers as HP
    import test_conv_exact as TE
    for (group, prec), (figure, cid) in TE.MODEL.items():
        if group == "conv":
            cid_, n, H, W, Cin, Co, stride, relu_in, act, nres, variant, cls = CC.case_by_id(cid)
            got = TE.model_conv_worst(CC.case_by_id(cid), prec)[1]
        else:
            hcase = next(c for c in CC.HEAD_CASES if c[0] == cid)
            got = TE.model_tail_worst(hcase, prec)[group][1]
        assert 0.5 * figure < got < 2.0 * figure, (group, prec, cid, got, figure)
        assert TE.class_bound(group, prec) == 4.0 * figure
