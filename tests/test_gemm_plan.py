"""CPU: the launch plan of the dense GEMMs over thousands of host-only shapes.

launch_gemm runs exactly the plan of gemm_plan (sta_launch.inc; exported by the test-hooks build as sta_debug_gemm_plan, and the
paired QKV launch's decision as sta_debug_qkv_pair_plan) - so this needs the built library but no GPU.  Every plan must
  * name a kernel that exists (the f16mx and RoPE forms exist on some tile families only),
  * tile exactly: the main tiles cover rows [0, M_all - m_tail) and the skinny tail blocks the m_tail rows after them, so no row
    is computed twice (an in-place residual GEMM would add it twice) and none is left out,
  * keep the decoder's pose-token tail only where the family has tail blocks for that epilogue and arithmetic, and keep it
    wherever the rule admits it,
  * never let a forced family displace the small-grid one,
and the paired launch is chosen only where both halves pass the small-grid predicate and neither half is f16mx.
"""
import itertools
import os

import pytest

A_DENSE = 0
EPI = {"f32": 0, "f16": 1, "qkv": 2, "gelu": 4, "f32r": 5}
PREC = {"f16": 1, "f16x3": 3, "f16x3h": 5, "f16x3m": 6}
TILE = {1: (128, 128), 2: (256, 256), 3: (192, 256), 5: (192, 128), 6: (128, 64)}
FIELDS = ("family", "bm", "bn", "m_tail", "tiles_m", "tiles_n", "ksplit", "slab_ks")

NS = (128, 256, 384, 512, 768, 1024, 1536, 2304, 3072, 4096)
KS = (256, 1024, 3072)
# patch rows around multiples of 192, 256 and 768, on both sides of the small-grid predicate (M <= 640 or < 192 tiles of 192x128)
MS = sorted({b * k + d for b in (192, 256, 768) for k in (2, 8, 12, 27) for d in (0, 64)} | {640, 20480})
TAILS = (0, 1, 2, 16, 20, 32)
FORCED = (0, 1, 2, 3, 4, 9)


def _load_lib():
    from vista_slam_amd import _lib
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libsta_mi355_test.so not built here (python -m vista_slam_amd.build)")
    return _lib.load_test()


@pytest.fixture(scope="module")
def lib():
    return _load_lib()


def plan(lib, epi, M_all, N, K, prec, mx=0, tail=0, forced=0):
    import ctypes as C
    out = (C.c_int * 8)()
    rc = lib.sta_debug_gemm_plan(A_DENSE, EPI[epi], M_all, N, K, PREC[prec], mx, tail, forced, out)
    assert rc == 0, (epi, M_all, N, K, prec, mx, tail, forced, lib.sta_last_error())
    return dict(zip(FIELDS, out))


def pair_plan(lib, M_all, Na, Nb, K, prec, mx_a=0, mx_b=0, tail=0, forced=0):
    import ctypes as C
    out = (C.c_int * 2)()
    assert lib.sta_debug_qkv_pair_plan(PREC[prec], M_all, Na, Nb, K, mx_a, mx_b, tail, forced, out) == 0
    return bool(out[0]), out[1]


def small_grid(M, N):
    """The small-grid predicate (sta_launch.inc: small_grid_m), restated."""
    return M <= 640 or ((M + 191) // 192) * ((N + 127) // 128) < 192


def has_tail(family, epi, mx):
    """Which gemm2 instantiations carry tail blocks (gemm2.h: gemm2_has_tail), restated."""
    return family in (2, 3, 5) and (epi in ("f32", "f32r") or (epi in ("gelu", "qkv") and not mx))


def has_kernel(family, epi, mx):
    """The instantiated (family, epilogue, arithmetic) combinations of launch_gemm's dense branches."""
    if mx and epi not in ("f32", "f32r", "f16"):
        return False
    if family == 1:
        return not mx
    if family == 2:
        return epi != "qkv" and (not mx or epi == "f16")
    if family == 3:
        return epi != "qkv"
    return family in (5, 6)


def mx_forms(prec, epi):
    """The values of GemmParams::mx the product can pass (use_mx: mlp.fc2 under f16x3m; the DPT head's plane-epilogue
    convolutions under f16x3h / f16x3m)."""
    if prec == "f16x3m" and epi in ("f32", "f32r"):
        return (0, 1)
    if prec in ("f16x3h", "f16x3m") and epi == "f16":
        return (0, 1)
    return (0,)


def sweep(lib):
    for prec, epi in itertools.product(PREC, EPI):
        for mx, N, K, M, tail, forced in itertools.product(mx_forms(prec, epi), NS, KS, MS, TAILS, FORCED):
            q = dict(epi=epi, M_all=M + tail, N=N, K=K, prec=prec, mx=mx, tail=tail, forced=forced)
            yield q, plan(lib, **q)


def check_plan(q, p):
    epi, M_all, N, mx, tail, forced = q["epi"], q["M_all"], q["N"], q["mx"], q["tail"], q["forced"]
    fam = p["family"]
    assert has_kernel(fam, epi, mx), "plan names a kernel that does not exist"
    assert (p["bm"], p["bn"]) == TILE[fam]
    bm = p["bm"]
    rows = M_all - p["m_tail"]
    assert (p["tiles_m"] - 1) * bm < rows <= p["tiles_m"] * bm, "main tiles do not cover exactly [0, M_all - m_tail)"
    assert (p["tiles_n"] - 1) * p["bn"] < N <= p["tiles_n"] * p["bn"]
    if p["m_tail"]:
        assert has_tail(fam, epi, mx), "row tail on a family without tail blocks for this epilogue"
        assert p["m_tail"] == tail
        assert rows % bm == 0, "main tiles overlap the tail rows"
        assert p["ksplit"] == 1
    else:
        # the tail is dropped only where the rule does not admit it or the final family cannot tile it
        admitted = 0 < tail <= 32 and N % 128 == 0 and forced != 1 and not small_grid(M_all - tail, N) and (not mx or epi in ("f32", "f32r"))
        assert not (admitted and has_tail(fam, epi, mx) and (M_all - tail) % bm == 0), "admissible row tail dropped"
    if forced == 1:
        assert fam == (5 if mx else 1)
    if fam == 6 or p["ksplit"] > 1:
        assert p["m_tail"] == 0
    if fam != 6:
        assert p["ksplit"] == 1 and p["slab_ks"] == 0
    if small_grid(M_all, N) and N % 64 == 0 and forced != 1:
        assert fam == 6, "a forced family displaced the small-grid one"


def test_sweep_invariants(lib):
    n = 0
    auto = {}
    for q, p in sweep(lib):
        try:
            check_plan(q, p)
        except AssertionError as e:
            raise AssertionError(f"{q} -> {p}: {e}") from None
        key = tuple(q[k] for k in ("prec", "epi", "M_all", "N", "K", "mx", "tail"))
        if q["forced"] == 0:
            auto[key] = p
        elif q["forced"] in (2, 3, 4, 9) and auto[key]["family"] == 6:
            assert p["family"] == 6, f"{q} -> {p}: a forced family displaced the small-grid one"
        if q["forced"] == 9:      # automatic without the halo convolution: the same plan on a dense GEMM
            assert p == auto[key], q
        n += 1
    assert n > 100000


def test_split_precisions_plan_alike(lib):
    """Outside the f16mx arithmetic the three split precisions run the same plans (the precision enters only as split / mx)."""
    for epi, N, K, M, tail, forced in itertools.product(EPI, NS, KS, MS[::2], TAILS, FORCED):
        ps = [plan(lib, epi, M + tail, N, K, prec, 0, tail, forced) for prec in ("f16x3", "f16x3h", "f16x3m")]
        assert ps[0] == ps[1] == ps[2], (epi, N, K, M, tail, forced, ps)


# The regressions: the f16mx remap of family 2 (no fp32-epilogue 256x256 f16mx kernel) ran AFTER the row-tail check, which
# therefore kept a tail that tiles by 256 rows for a launch that tiles by 192 - the last main tile then covered the pose rows
# that the tail blocks also computed (x += A W^T twice, or a race).
def test_regression_mx_remap_before_row_tail_decoder_fc2(lib):
    """The decoder's mlp.fc2 at B = 10 @512x512 (M = 20480 + 20 pose rows, N = 768, K = 3072, in-place residual) under f16x3m."""
    assert lib.sta_debug_pick_family(A_DENSE, EPI["f32r"], 20480, 768, 3072, 1, 0, 0, 0) == 2     # the cost model's 256x256 ...
    p = plan(lib, "f32r", 20480 + 20, 768, 3072, "f16x3m", mx=1, tail=20)
    check_plan(dict(epi="f32r", M_all=20500, N=768, mx=1, tail=20, forced=0), p)
    assert (p["family"], p["bm"]) == (3, 192) and 20480 % 192 != 0     # ... runs 192x256 in the f16mx arithmetic
    assert p["m_tail"] == 0 and p["tiles_m"] == (20500 + 191) // 192, p


@pytest.mark.parametrize("epi", ["f32r", "f32"])
def test_regression_forced_256_rows_under_f16x3m(lib, epi):
    """Forced family 2 under f16x3m at M = 8 x 256 + 16, N = 2304: runs 192x256, where 2048 patch rows are no whole tile count."""
    p = plan(lib, epi, 8 * 256 + 16, 2304, 256, "f16x3m", mx=1, tail=16, forced=2)
    check_plan(dict(epi=epi, M_all=2064, N=2304, mx=1, tail=16, forced=2), p)
    assert (p["family"], p["m_tail"], p["tiles_m"]) == (3, 0, 11), p
    # without f16mx the same request runs 256x256 and keeps its tail
    p = plan(lib, epi, 8 * 256 + 16, 2304, 256, "f16x3m", mx=0, tail=16, forced=2)
    assert (p["family"], p["m_tail"], p["tiles_m"]) == (2, 16, 8), p


def test_pair_plan_sweep(lib):
    n = 0
    for prec, C, K, M, tail, forced in itertools.product(PREC, (512, 768, 1024), (256, 768, 1024), MS, TAILS, FORCED):
        Na, Nb, M_all = 3 * C, 2 * C, M + tail
        for mx_a, mx_b in ((0, 0), (1, 0), (0, 1)):
            one, m_tail = pair_plan(lib, M_all, Na, Nb, K, prec, mx_a, mx_b, tail, forced)
            want = prec != "f16" and not mx_a and not mx_b and forced in (0, 9) and not small_grid(M_all, Na) and not small_grid(M_all, Nb)
            assert one == want, (prec, C, K, M_all, tail, forced, mx_a, mx_b)
            if m_tail:
                assert one and m_tail == tail and (M_all - tail) % 192 == 0
                assert not small_grid(M_all - tail, Na) and not small_grid(M_all - tail, Nb)
            elif one and 0 < tail <= 32:
                assert (M_all - tail) % 192 != 0 or small_grid(M_all - tail, Na) or small_grid(M_all - tail, Nb), "admissible pair tail dropped"
            n += 1
    assert n > 10000
