"""GPU: the varlen forms of the DPT head's geometry-decoding kernels (sta_head_pts_varlen), one launch over entries of different size,
exactly and per pixel.

Every launch packs its entries entry-major and is compared, entry by entry, with the operation on THAT ENTRY ALONE: a tap, a
bilinear tap or a scatter that crosses into a neighbouring entry, or stops short of the entry's own border, changes the result.

1. 3x3 convolutions (gemm2.h A_CONV3 loader, varlen form) on the integer inputs of tests/test_conv_exact.py (helpers.
   conv_integer_inputs: every exact output is an integer of magnitude <= 2048 by construction, so f16x3 and the f16mx arithmetic must
   return the integer itself): the forced implicit-GEMM families 2 / 3 / 5, the forced halo-tiled family 8 on 128 and 256 columns
   (entries 9x32, 9x33, 7x16, 1x31, 1x1 and 17x5 in one launch), the small-grid family 6 with and without K slices,
   stride 2 on odd and even sizes in one launch, every epilogue of conv_cases.EPI_NAME.  The family, tile and K slices the launch ran
   under are asserted against its plan.
2. the fused tail (EPI_HEAD: implicit GEMM on 192x128 tiles, and the halo form under forced family 8) on Gaussian inputs against
   float64, per entry, under the bounds of test_conv_exact.py.
3. ConvTranspose (EPI_CONVT scatter), k = 2 and k = 4, on integers (|sum| <= 3 C + 32 <= 608: exact in every arithmetic).
4. the bilinear x2: Hi = 1, Wi = 1, the crop Hc = 2 Hi - 1, an entry of 64 rows next to one of 3 - against float64
   (torch.nn.functional.interpolate, align_corners) under the whole-tensor bar of test_gpu_kernels.py, entry by entry (Gaussian
   inputs: one foreign tap moves an entry by O(1)).

The debug entries poison the output planes (a pixel never stored is a NaN) and return the 4096 guard bytes that lie right behind the
output planes: they must come back as the 0xA5 they were filled with.

Families 2 / 3 / 5: the entries 100x97, 57x61, 1x1 and 3x200 hold 13778 pixels, below the small-grid predicate (M <= 640 or
ceil(M / 192) ceil(N / 128) < 192: 18241 pixels at 256 columns), under which a forced family never displaces family 6; a second
100x97 entry behind them makes it 23478, so that the launch really runs on the forced tiles (asserted).  23478, and the offsets 9700,
13177, 13178 and 13778, are multiples of neither 192 nor 256: tiles end inside rows and span entries.
"""
import ctypes as C

import numpy as np
import pytest

import conv_cases as CC

pytestmark = pytest.mark.gpu

ARITH = ("f16x3", "head_mx")                  # the varlen forms exist for the split precisions (plain f16 is refused)
GLOBAL_TOL = {"f16x3": 2e-5, "head_mx": 6e-5}          # the whole-tensor bounds of test_gpu_kernels.py
TAIL_BOUND = {"f16x3": (5.61e-06, 5.58e-07), "head_mx": (6e-5, 6e-5)}       # pts, conf: the class bounds of test_conv_exact.py

BIG = [(100, 97), (57, 61), (1, 1), (3, 200), (100, 97)]
SMALL = [(7, 5), (1, 1), (3, 9), (5, 2), (1, 13)]
STRIDE2 = [(14, 14), (13, 15), (1, 1), (7, 10), (2, 3), (1, 8)]
HALO = [(9, 32), (9, 33), (7, 16), (1, 31), (1, 1), (17, 5)]          # family 8: W % 32 in {0, 1, 16, 31, 5}, H % 8 != 0, one pixel
EPIS = [CC.PLAIN, CC.RELU, CC.R1, CC.R2, (0, 2, 0)]

# (id, entries, Cin, Co, stride, epilogue, forced variant, (family, bn, split-K))
CONV_CASES = (
    [(f"g{v}_{CC.EPI_NAME[e]}", BIG, 32 if i % 2 == 0 else 64, 256, 1, e, v, (f, bn, 0))
     for v, f, bn in ((2, 2, 256), (3, 3, 256), (4, 5, 128)) for i, e in enumerate(EPIS)] +
    [(f"s6_{CC.EPI_NAME[e]}", SMALL, 32, 64, 1, e, 0, (6, 64, 0)) for e in EPIS] +
    [(f"s6_sk_{CC.EPI_NAME[e]}", SMALL, 256, 256, 1, e, 0, (6, 64, 1)) for e in EPIS] +
    [(f"h{co}_{CC.EPI_NAME[e]}", HALO, 32 if i % 2 == 0 else 96, co, 1, e, 8, (8, co, 0)) for co in (128, 256) for i, e in enumerate(EPIS)] +
    [("s6_s2", STRIDE2, 32, 64, 2, CC.PLAIN, 0, (6, 64, 0)),
     ("s6_sk_s2_c768", STRIDE2, 768, 768, 2, CC.PLAIN, 0, (6, 64, 1)),
     ("g5_s2", [(200, 194), (199, 193), (1, 1), (7, 10)], 32, 256, 2, CC.PLAIN, 4, (5, 128, 0))])


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    return gpu_checks


def iarr(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def guard_ok(g):
    return bool((g.cpu().numpy() == 0xA5).all())


def conv_vl_launch(G, prec, case, xs, w, b, ress):
    """One sta_debug_conv3x3_varlen launch on per-entry NHWC inputs -> (per-entry outputs, plan, guard intact)."""
    import torch
    from vista_slam_amd import _lib
    cid, ents, Cin, Co, stride, (relu_in, act, nres), variant, cls = case
    m, lib, h = G.kernel_handle(prec, variant)
    outs = [CC.out_size(H, W, stride) for H, W in ents]
    pout = sum(a * c for a, c in outs)
    x = G.dev(np.concatenate([t.reshape(-1, Cin) for t in xs]))
    rd = [G.dev(np.concatenate([r[k].reshape(-1, Co) for r in ress])) for k in range(nres)]
    wd, bd = G.dev(w), G.dev(b)
    out = torch.full((pout, Co), float("nan"), device=G.DEV)
    guard = torch.zeros(4096, dtype=torch.uint8, device=G.DEV)
    m.range_report(reset=True)
    try:
        _lib.check(lib.sta_debug_conv3x3_varlen(h, x.data_ptr(), wd.data_ptr(), bd.data_ptr(), len(ents), iarr([e[0] for e in ents]),
                                                iarr([e[1] for e in ents]), Cin, Co, stride, relu_in, act,
                                                rd[0].data_ptr() if nres > 0 else None, rd[1].data_ptr() if nres > 1 else None,
                                                out.data_ptr(), guard.data_ptr(), G.st()))
        torch.cuda.synchronize()
        plan = G.last_plan(lib, h)
    finally:
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    assert tuple(m.range_report(reset=True)) == (0, 0)
    o = out.cpu().numpy()
    per, at = [], 0
    for a, c in outs:
        per.append(o[at:at + a * c].reshape(1, a, c, Co))
        at += a * c
    return per, plan, guard_ok(guard)


@pytest.mark.parametrize("prec", ARITH)
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_varlen_integer_sums_are_bit_exact_per_entry(G, prec, case):
    import helpers as HP
    cid, ents, Cin, Co, stride, (relu_in, act, nres), variant, cls = case
    _, w, b, _ = HP.conv_integer_inputs(1, 1, 1, Cin, Co, stride, nres, 31)
    xs, ress, wants = [], [], []
    for i, (H, W) in enumerate(ents):
        x, _, _, res = HP.conv_integer_inputs(1, H, W, Cin, Co, stride, nres, 100 + i)       # (|x| <= 3 with THESE weights: the bound of the helper holds)
        ref = HP.conv_ref64(x, w, b, stride, relu_in, act, res)
        want = np.rint(ref).astype(np.int64)
        assert np.array_equal(want.astype(np.float64), ref) and np.abs(want).max() <= 2048
        xs.append(x); ress.append(res); wants.append(want)
    got, plan, guard = conv_vl_launch(G, prec, case, xs, w, b, ress)
    print(cid, prec, plan)
    assert (plan["family"], plan["bn"], 1 if plan["ksplit"] > 1 else 0) == cls, plan
    for i, (g, want) in enumerate(zip(got, wants)):
        bad = np.argwhere(~(g.astype(np.float64) == want))
        first = "; ".join(f"(y {y}, x {x}) channel {co}: want {want[0, y, x, co]}, got {g[0, y, x, co]:g}" for _, y, x, co in bad[:4])
        assert len(bad) == 0, f"entry {i} ({ents[i][0]} x {ents[i][1]}): {len(bad)} wrong elements ({int(np.isnan(g).sum())} NaN); {first}"
    assert guard, "the guard block behind the output planes was written"


@pytest.mark.parametrize("prec", ARITH)
def test_conv_varlen_tap_selection_names_the_pixel_read(G, prec):
    """One-hot weights on inputs that carry their own address (y, x, ENTRY, group): the output must equal the shifted planes of the
    entry itself, 0 outside it - a failure decodes to the entry and pixel actually read."""
    import helpers as HP
    case = ("sel", SMALL + [(9, 33)], 32, 64, 1, CC.PLAIN, 0, (6, 64, 0))
    ents = case[1]
    xs, wants = [], []
    for i, (H, W) in enumerate(ents):
        x, w, tap, ci = HP.conv_selection_inputs(1, H, W, 32, 64, 0)
        x[..., 2::4] = float(i)                                   # the "image" planes carry the entry
        xs.append(x); wants.append(HP.conv_selection_expected(x, tap, ci, 1, 0))
    got, plan, guard = conv_vl_launch(G, prec, case, xs, w, np.zeros(64, np.float32), [[] for _ in ents])
    for i, (g, want) in enumerate(zip(got, wants)):
        wrong, first = HP.conv_selection_report(g, want, tap, ci, 1)
        assert wrong == 0, f"entry {i}: {wrong} wrong elements; {first}"
    assert guard


@pytest.mark.parametrize("prec", ARITH)
@pytest.mark.parametrize("variant", [0, 8])
def test_fused_tail_varlen_per_entry(G, prec, variant):
    """conv3_head on packed pixels (EPI_HEAD).  Automatic: implicit GEMM on 192x128 tiles, 40398 pixels, above the small-grid predicate;
    forced 8: the halo form on the entries of the family-8 convolution cases."""
    import torch
    import helpers as HP
    from vista_slam_amd import _lib
    ents = [(200, 150), (97, 101), (1, 1), (3, 200)] if variant == 0 else HALO
    ins = [HP.tail_gaussian_inputs(1, H, W, 1.0, seed=41) for H, W in ents]
    x = np.concatenate([HP.tail_gaussian_inputs(1, H, W, 1.0, seed=50 + i)[0].reshape(-1, 128) for i, (H, W) in enumerate(ents)])
    w2, b2, w4, b4 = ins[0][1:]
    m, lib, h = G.kernel_handle(prec, variant)
    npix = x.shape[0]
    pts = torch.full((npix, 3), float("nan"), device=G.DEV)
    conf = torch.full((npix,), float("nan"), device=G.DEV)
    d = [G.dev(t) for t in (x, w2, b2, w4, b4)]
    m.range_report(reset=True)
    try:
        _lib.check(lib.sta_debug_conv3_head_varlen(h, *[t.data_ptr() for t in d], len(ents), iarr([e[0] for e in ents]), iarr([e[1] for e in ents]),
                                                   pts.data_ptr(), conf.data_ptr(), G.st()))
        torch.cuda.synchronize()
        plan = G.last_plan(lib, h)
    finally:
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    assert tuple(m.range_report(reset=True)) == (0, 0)
    assert (plan["family"], plan["bn"]) == ((5, 128) if variant == 0 else (8, 128)), plan
    p, c = pts.cpu().numpy(), conf.cpu().numpy()
    at = 0
    for i, (H, W) in enumerate(ents):
        xe = x[at:at + H * W].reshape(1, H, W, 128)
        rp, rc = HP.tail_ref64(xe, w2, b2, w4, b4)
        ep, ec = HP.rel_l2(p[at:at + H * W].reshape(1, H, W, 3), rp), HP.rel_l2(c[at:at + H * W].reshape(1, H, W), rc)
        print("tail", prec, ents[i], ep, ec)
        assert not np.isnan(p[at:at + H * W]).any() and not np.isnan(c[at:at + H * W]).any()
        assert ep < TAIL_BOUND[prec][0] and ec < TAIL_BOUND[prec][1], (i, ep, ec)
        at += H * W


@pytest.mark.parametrize("prec", ARITH)
@pytest.mark.parametrize("k,Cd", [(2, 192), (4, 96)])
def test_convt_varlen_integers_are_bit_exact_per_entry(G, prec, k, Cd):
    import torch
    from vista_slam_amd import _lib
    ents = [(3, 5), (1, 1), (7, 2), (1, 9), (6, 10), (2, 8), (2, 8)]
    rng = np.random.default_rng(7 + k)
    w = (rng.integers(0, 2, size=(Cd, Cd, k, k)) * 2 - 1).astype(np.float32)            # ConvTranspose2d layout [Cin, Cout, k, k]
    b = rng.integers(-32, 33, size=Cd).astype(np.float32)
    xs = [rng.integers(-3, 4, size=(H, W, Cd)).astype(np.float32) for H, W in ents]
    m, lib, h = G.kernel_handle(prec, 0)
    pout = sum(H * W * k * k for H, W in ents)
    out = torch.full((pout, Cd), float("nan"), device=G.DEV)
    guard = torch.zeros(4096, dtype=torch.uint8, device=G.DEV)
    xd, wd, bd = G.dev(np.concatenate([x.reshape(-1, Cd) for x in xs])), G.dev(w), G.dev(b)
    m.range_report(reset=True)
    _lib.check(lib.sta_debug_convt_varlen(h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), len(ents), iarr([e[0] for e in ents]),
                                          iarr([e[1] for e in ents]), Cd, k, out.data_ptr(), guard.data_ptr(), G.st()))
    torch.cuda.synchronize()
    assert tuple(m.range_report(reset=True)) == (0, 0)
    o = out.cpu().numpy()
    at = 0
    for i, ((H, W), x) in enumerate(zip(ents, xs)):
        want = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).double().permute(2, 0, 1)[None], torch.from_numpy(w).double(),
                                                    torch.from_numpy(b).double(), stride=k)[0].permute(1, 2, 0).numpy()
        g = o[at:at + H * W * k * k].reshape(H * k, W * k, Cd)
        bad = np.argwhere(~(g.astype(np.float64) == want))
        assert len(bad) == 0, f"entry {i} ({H} x {W}): {len(bad)} wrong elements ({int(np.isnan(g).sum())} NaN), first {bad[:3].tolist()}"
        at += H * W * k * k
    assert guard_ok(guard), "the guard block behind the output planes was written"


UP2 = [  # (Hi, Wi, Hc, Wc)
    (1, 1, 2, 2), (1, 1, 1, 1), (1, 9, 2, 18), (5, 1, 10, 2), (3, 2, 5, 3), (64, 5, 128, 10), (3, 7, 6, 14), (4, 4, 7, 8), (2, 8, 4, 16), (2, 8, 4, 16)]


@pytest.mark.parametrize("prec", ARITH)
def test_up2_varlen_per_entry(G, prec):
    import torch
    from vista_slam_amd import _lib
    Cd = 64
    rng = np.random.default_rng(5)
    xs = [rng.standard_normal((Hi, Wi, Cd)).astype(np.float32) for Hi, Wi, _, _ in UP2]
    m, lib, h = G.kernel_handle(prec, 0)
    pout = sum(e[2] * e[3] for e in UP2)
    out = torch.full((pout, Cd), float("nan"), device=G.DEV)
    guard = torch.zeros(4096, dtype=torch.uint8, device=G.DEV)
    xd = G.dev(np.concatenate([x.reshape(-1, Cd) for x in xs]))
    m.range_report(reset=True)
    _lib.check(lib.sta_debug_up2_varlen(h, xd.data_ptr(), len(UP2), iarr([e[0] for e in UP2]), iarr([e[1] for e in UP2]), Cd,
                                        iarr([e[2] for e in UP2]), iarr([e[3] for e in UP2]), out.data_ptr(), guard.data_ptr(), G.st()))
    torch.cuda.synchronize()
    assert tuple(m.range_report(reset=True)) == (0, 0)
    o = out.cpu().numpy()
    at = 0
    for i, ((Hi, Wi, Hc, Wc), x) in enumerate(zip(UP2, xs)):
        g = o[at:at + Hc * Wc].reshape(Hc, Wc, Cd)
        at += Hc * Wc
        ref = torch.nn.functional.interpolate(torch.from_numpy(x).double().permute(2, 0, 1)[None], scale_factor=2, mode="bilinear",
                                              align_corners=True)[0].permute(1, 2, 0).numpy()[:Hc, :Wc]
        assert not np.isnan(g).any(), f"entry {i}: {int(np.isnan(g).sum())} elements never stored"
        import helpers as HP
        err = HP.rel_l2(g, ref)
        print("up2", prec, UP2[i], err)
        assert err < GLOBAL_TOL[prec], (i, err)
    assert guard_ok(guard), "the guard block behind the output planes was written"
    m.range_report(reset=True)


def test_range_report_counts_a_hot_value_of_one_entry(G):
    """A value above 65504 in ONE entry of a varlen launch raises the fp16 counter, as tests/test_range_gpu.py expects of the writers
    (epilogue_tile's plane epilogue through the varlen conv), and the value is stored saturated; every other pixel is untouched."""
    import torch
    from vista_slam_amd import _lib
    m, lib, h = G.kernel_handle("f16x3", 0)
    ents = [(3, 4), (2, 5), (1, 1)]
    Cin, Co = 32, 64
    w = np.zeros((Co, Cin, 3, 3), np.float32)
    w[np.arange(Co), np.arange(Co) % Cin, 1, 1] = 2.0                    # out[co] = 2 x in[co % 32] (centre tap)
    xs = [np.ones((H, W, Cin), np.float32) for H, W in ents]
    xs[1][1, 3, 7] = 40000.0                                             # 2 x 40000 = 80000 > 65504
    x = G.dev(np.concatenate([t.reshape(-1, Cin) for t in xs]))
    out = torch.zeros(sum(a * b for a, b in ents), Co, device=G.DEV)
    wd, bd = G.dev(w), G.dev(np.zeros(Co, np.float32))
    _, rng = G.with_range(m, lambda: _lib.check(lib.sta_debug_conv3x3_varlen(
        h, x.data_ptr(), wd.data_ptr(), bd.data_ptr(), 3, iarr([e[0] for e in ents]), iarr([e[1] for e in ents]), Cin, Co, 1, 0, 0, None, None,
        out.data_ptr(), None, G.st())))
    print("[range] varlen conv <- 40000 x 2:", rng)
    assert rng[0] > 0 and rng[1] == 0, rng
    o = out.cpu().numpy()
    hot = 12 + 1 * 5 + 3                                                  # entry 1 starts at pixel 12; its pixel (1, 3)
    assert o[hot, 7] == 65504.0 and o[hot, 39] == 65504.0, o[hot, [7, 39]]          # the planes saturate
    o[hot, [7, 39]] = 2.0
    assert (o == 2.0).all()
    m.range_report(reset=True)
