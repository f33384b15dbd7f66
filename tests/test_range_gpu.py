"""GPU: the range report (sta_range_report) and the saturation of every fp16 plane writer, at the exact thresholds.

The product claim (README.md): planes saturate at +-65504 instead of producing inf; leaving the fp16 range - or a
NaN - is reported, never silent.  tests/range_cases.py lists every writer (tests/test_range_inventory.py proves on the host that the
list is complete); this file drives each one through the kernel-level entries of include/sta_mi355_debug.h or the product API.

The recipe.  All operands are integers an fp16 holds, so the expected output is exact in every arithmetic (f16x3, f16, f16mx =
"head_mx").  The operands themselves stay inside BOTH ranges (|a| <= 32752 < 57344, |w| <= 2 < 28), so the input converters
(rows_to_planes_kernel, repack_weight_kernel), which report too, stay silent and an event can only come from the writer under test.
One output element, the HOT element, is built as a * w + d (range_cases.HOT): 57344, 57345, 65504, 65505, -65505.  Each launch asserts
  report   which of the two counters is non-zero (the event count depends on how many lanes flush and is not a contract);
  value    the hot element reads back as clamp(v, +-65504), exactly (f16: its nearest fp16); never inf / NaN;
  others   every other element equals the exact integer result AND differs from the same launch without the hot element's "+ d"
           by exactly what the reference differs by (0 outside the bias column): saturating one element disturbs nothing else.

Where an entry cannot do what a recipe would need, the test says so:
  sta_debug_gemm ignores `resid` under via_f16, so the residual planes of the plane epilogue are driven through the 3x3 convolutions;
  the pose token's table row is position -1, a rotation by -1 rad at frequency 0, not the identity: the exact boundary case of the
  rotation kernels and of qkv_finish_kernel uses position 0, and the pose row is one more overflow case;
  sta_debug_up2 converts its input with rows_to_planes_kernel, which counts an fp8 event per group of four values above 57344 itself:
  the bilinear kernel's own flush shows as MORE fp8 events than the input has groups of four.
"""
import ctypes as C

import numpy as np
import pytest

import conv_cases as CC
import range_cases as RC
import row_cases as ROWS

pytestmark = pytest.mark.gpu

F16_MAX = float(RC.F16_MAX)
PLANE_BAR = {"f16x3": 1e-5, "f16": 3e-3, "head_mx": 1e-5}    # tests/test_row_gpu.py: the bars of test_layernorm_rows (LayerNorm planes are f16x3 planes under "head_mx")
PREC_ID = {"f16x3": (3, 0), "f16": (1, 0), "head_mx": (5, 1)}      # -> (precision id, mx) of sta_debug_gemm_plan


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    return gpu_checks


def expected_class(v, mx_out):
    return RC.HOT[v][2 if mx_out else 1]


class_of = RC.class_of            # the rule behind range_cases.HOT, for values that are not in the table (the launches without the + d)


def stored(v, prec):
    """What the planes hold for the exact result v: the clamp (f16x3, f16mx: hi + lo is exact for these integers), its nearest fp16 (f16)."""
    c = float(np.clip(v, -F16_MAX, F16_MAX))
    return float(np.float16(c)) if prec == "f16" else c


def check_launch(tag, prec, got, ref, hot, rng, want_class, cold=None, ref_cold=None):
    """got / ref: the launch and its exact float64 result (unclamped); hot: tuple of index tuples of the hot elements."""
    print(f"[range] {tag} {prec}: report {rng}, expected class {want_class}, hot got {[float(got[i]) for i in hot]} exact {[float(ref[i]) for i in hot]}")
    assert np.isfinite(got).all(), (tag, "inf / NaN in a plane", np.argwhere(~np.isfinite(got))[:4].tolist())
    if rng is not None:                                      # (None: the launch helper asserted the class itself)
        assert RC.range_class(rng) == tuple(want_class), (tag, prec, "report", rng, "expected class", want_class)
    mask = np.zeros(got.shape, bool)
    for i in hot:
        assert float(got[i]) == stored(ref[i], prec), (tag, prec, i, float(got[i]), "expected", stored(ref[i], prec))
        mask[i] = True
    bad = np.argwhere((got.astype(np.float64) != ref) & ~mask)
    assert len(bad) == 0, (tag, prec, "elements beside the hot one", len(bad), bad[:4].tolist())
    if cold is not None:
        d = (got.astype(np.float64) - cold.astype(np.float64)) != (ref - ref_cold)
        assert not (d & ~mask).any(), (tag, prec, "saturating the hot element disturbed others", np.argwhere(d & ~mask)[:4].tolist())


# ------------------------------------------------------------------------------------------ dense GEMM, plane epilogue
def gemm_operands(M, N, K, r, c, v, with_d=True, seed=5, wide=False):
    """A [M, K], W [N, K], bias [N] and the exact result.  K column 0 carries the hot product alone (A[r, 0] = a, W[c, 0] = w), row r
    and column c are zero elsewhere, the bias of column c is d.  Everything else: integers in [-3, 3] x [-2, 2] (wide=False) or
    {-1, 0, 1} (long K: every sum stays below 2048)."""
    (a, w, d), _, _ = RC.HOT[v]
    rs = np.random.default_rng(seed + M + 3 * N + 7 * K)
    lim = (1, 1) if wide else (3, 2)
    A = rs.integers(-lim[0], lim[0] + 1, size=(M, K)).astype(np.float32)
    Wt = rs.integers(-lim[1], lim[1] + 1, size=(N, K)).astype(np.float32)
    b = rs.integers(-4, 5, size=N).astype(np.float32)
    A[:, 0] = 0; Wt[:, 0] = 0; A[r, :] = 0; Wt[c, :] = 0
    A[r, 0] = a; Wt[c, 0] = w
    b[c] = d if with_d else 0
    ref = (A @ Wt.T + b).astype(np.float64)               # exact in fp32: integers, every partial sum below 2^24
    rest = np.abs(ref); rest[r, c] = 0
    assert rest.max() <= 2048 and ref[r, c] == a * w + (d if with_d else 0)
    return A, Wt, b, ref


def run_gemm_thresholds(G, prec, M, N, K, act, places, variant=0, want_family=None, want_split=None, values=None, wide=False):
    mx_out = prec == "head_mx" and N % 64 == 0
    for (r, c) in places:
        cold = {}
        for v in values or RC.HOT:
            if act == 2 and v < 0:
                continue                                        # behind a ReLU the negative side does not exist
            A, Wt, b, ref = gemm_operands(M, N, K, r, c, v, wide=wide)
            if act == 2:
                ref = np.maximum(ref, 0)
            got, rng, plan = G.range_gemm(prec, A, Wt, b, act=act, variant=variant)
            if want_family is not None:
                assert plan["family"] == want_family, plan
            if want_split is not None:
                assert (plan["ksplit"] > 1) == want_split, plan
            base = RC.HOT[v][0][:2]
            if base not in cold:
                Ac, Wc, bc, rc = gemm_operands(M, N, K, r, c, v, with_d=False, wide=wide)
                oc, rng_c, _ = G.range_gemm(prec, Ac, Wc, bc, act=act, variant=variant)
                cold[base] = (oc, np.maximum(rc, 0) if act == 2 else rc)
            check_launch(f"gemm {M}x{N}x{K} act {act} variant {variant} hot ({r}, {c}) = {v}", prec, got, ref, ((r, c),), rng,
                         expected_class(v, mx_out), *cold[base])


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("prec,N", [(p, n) for n in (128, 80) for p in RC.ARITHMETICS if n % 64 == 0 or p != "head_mx"])
def test_plane_epilogue_thresholds(G, prec, N, act):
    """epilogue_tile<EPI_F16> through sta_debug_gemm(via_f16 = 1), M = 72 = two interior 32-row sub-tiles + 8 ragged rows, K = 64.
    N = 128: the small-grid family (128 x 64 tiles, LDS-staged interior sub-tiles in f16x3); N = 80: the 128 x 128 kernel of gemm.h with
    a column-ragged sub-tile (f16x3 / f16 only: an f16mx GEMM needs N % 64 == 0).  Hot element at the first element, the last element
    of the last interior sub-tile, inside a row-ragged sub-tile, and at (M - 1, N - 1)."""
    M = 72
    places = [(0, 0), (63, 127 if N == 128 else 63), (68, 40), (M - 1, N - 1)]
    run_gemm_thresholds(G, prec, M, N, 64, act, places, want_family=6 if N == 128 else 1, want_split=False)


def smallest_split_k(lib, prec, M, N):
    pid, mx = PREC_ID[prec]
    out = (C.c_int * 8)()
    for K in range(64, 4097, 32):
        assert lib.sta_debug_gemm_plan(0, 1, M, N, K, pid, mx, 0, 0, out) == 0
        if out[6] > 1:
            return K
    raise AssertionError("no K up to 4096 splits")


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_splitk_finish_thresholds(G, prec, act):
    """The same entry at the smallest K whose plan has K slices at M = 72: the tiles store fp32 slabs and splitk_finish_kernel applies
    bias / activation, saturates and reports (per group of four columns)."""
    m, lib, h = G.kernel_handle(prec)
    M, N = 72, 128
    K = smallest_split_k(lib, prec, M, N)
    print(f"[range] split-K from K = {K}")
    run_gemm_thresholds(G, prec, M, N, K, act, [(0, 0), (M - 1, N - 1), (68, 41)], want_family=6, want_split=True, wide=True)


@pytest.mark.parametrize("variant", [2, 3, 4])
@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_forced_family_thresholds(G, prec, variant):
    """The throughput families (forced; 256 x 256, 192 x 256, 192 x 128 tiles) at 19400 x 256, K = 64 - past the small-grid predicate.
    Hot element in the first tile, in the last row of the ragged last tile, and in the last column."""
    M, N = 19400, 256
    places = [(0, 0), (M - 1, 100), (300, N - 1)]
    run_gemm_thresholds(G, prec, M, N, 64, 0, places, variant=variant, want_family={2: 2, 3: 3, 4: 5}[variant], want_split=False)


# ------------------------------------------------------------------------------------------ ConvTranspose scatter
@pytest.mark.parametrize("k,Cd", [(2, 192), (4, 96)])
@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_convt_scatter_thresholds(G, prec, k, Cd):
    """epilogue_tile<EPI_CONVT> through sta_debug_convt, n = 2, H = 3, W = 5: hot element at sub-pixel (k - 1, k - 1) of the last input
    pixel and at (0, 0) of the first.  Input channel 0 carries the hot product alone."""
    n, H, W_ = 2, 3, 5
    co = 37
    for (img, y, x, dy, dx) in [(n - 1, H - 1, W_ - 1, k - 1, k - 1), (0, 0, 0, 0, 0)]:
        cold = {}
        for v in RC.HOT:
            def make(with_d):
                (a, w, d), _, _ = RC.HOT[v]
                rs = np.random.default_rng(17 + k)
                xx = rs.integers(-3, 4, size=(n, H, W_, Cd)).astype(np.float32)
                ww = rs.integers(-1, 2, size=(Cd, Cd, k, k)).astype(np.float32)          # [Ci, Co, k, k]
                b = rs.integers(-4, 5, size=Cd).astype(np.float32)
                xx[..., 0] = 0; ww[0] = 0; xx[img, y, x, :] = 0
                xx[img, y, x, 0] = a; ww[0, co, dy, dx] = w
                b[co] = d if with_d else 0
                ref = np.einsum("nyxi,iodv->nydxvo", xx.astype(np.float64), ww.astype(np.float64)).reshape(n, H * k, W_ * k, Cd) + b.astype(np.float64)
                return xx, ww, b, ref
            xx, ww, b, ref = make(True)
            got, rng, plan = G.range_convt(prec, xx, ww, b, k)
            base = RC.HOT[v][0][:2]
            if base not in cold:
                xc, wc, bc, rc = make(False)
                cold[base] = (G.range_convt(prec, xc, wc, bc, k)[0], rc)
            hot = (img, y * k + dy, x * k + dx, co)
            check_launch(f"convt k {k} C {Cd} hot {hot} = {v}", prec, got, ref, (hot,), rng, expected_class(v, prec == "head_mx"), *cold[base])


# ------------------------------------------------------------------------------------------ 3x3 convolutions
CONV_IDS = ["s6_plain", "s6_sk_r1", "g2_r1_c32", "g3_r2_c32", "g5_s2_odd", "h128_r2_c128", "h256_plain_w32"]
_conv_base = {}


def conv_base(case):
    """Integer inputs of the case with input channel 0 and output channel `co` cleared, and their exact result: computed once."""
    import helpers as HP
    cid, n, H, W_, Cin, Co, stride, relu_in, act, nres, variant, cls = case
    if cid not in _conv_base:
        _conv_base.clear()
        x, w, b, res = HP.conv_integer_inputs(n, H, W_, Cin, Co, stride, nres, 33)
        co = Co - 3
        x[..., 0] = 0; w[:, 0] = 0; w[co] = 0; b[co] = 0
        for r in res:
            r[..., co] = 0                                    # the hot element's residual is set per launch (first plane only)
        _conv_base[cid] = (x, w, b, res, co, HP.conv_ref64(x, w, b, stride, relu_in, act, res))
    return _conv_base[cid]


@pytest.mark.parametrize("prec", RC.ARITHMETICS)
@pytest.mark.parametrize("cid", CONV_IDS)
def test_conv3_thresholds(G, prec, cid):
    """One case per (family, split-K) class of tests/conv_cases.py, through conv_launch(expect_range = ...): a one-hot centre tap on one
    (Cin, Co) pair makes one output element hot - at a corner pixel of the first image and at the last pixel of the last.  With
    residual planes the hot value is conv 32752 x 1 + residual 32752 (+ bias): the threshold sits BEHIND the residual add."""
    case = CC.case_by_id(cid)
    _cid, n, H, W_, Cin, Co, stride, relu_in, act, nres, variant, cls = case
    assert relu_in == 0 and act == 0
    x0, w0, b0, res0, co, ref0 = conv_base(case)
    Ho, Wo = CC.out_size(H, W_, stride)
    places = [(0, 0, 0), (n - 1, Ho - 1, Wo - 1)]
    for (img, yo, xo) in places:
        cold = {}
        for v in RC.HOT:
            (a, w_, d), _, _ = RC.HOT[v]

            def make(with_d):
                x, w, b = x0.copy(), w0.copy(), b0.copy()
                res = [r.copy() for r in res0]
                x[img, yo * stride, xo * stride, 0] = a
                w[co, 0, 1, 1] = 1 if nres else w_
                ref = ref0.copy()
                if nres:
                    ref[img, yo, xo, co] += a - res[0][img, yo, xo, co]
                    res[0][img, yo, xo, co] = a
                ref[img, yo, xo, co] += a * w[co, 0, 1, 1]
                if with_d:
                    b[co] = d
                    ref[..., co] += d
                return x, w, b, res, ref
            x, w, b, res, ref = make(True)
            want = expected_class(v, prec == "head_mx")
            got, ran = G.conv_launch(prec, case, x, w, b, res, expect_range=want)
            assert ran == cls, ran
            base = RC.HOT[v][0][:2]
            if base not in cold:
                xc, wc, bc, rc, refc = make(False)
                cold[base] = (G.conv_launch(prec, case, xc, wc, bc, rc, expect_range=class_of(v - d, prec == "head_mx"))[0], refc)
            check_launch(f"conv {cid} hot ({img}, {yo}, {xo}, {co}) = {v}", prec, got, ref, ((img, yo, xo, co),), None, want, *cold[base])


# ------------------------------------------------------------------------------------------ fused DPT tail
TAIL_CASE = next(c for c in CC.HEAD_CASES if c[0] == "t8_w33_tiny_w4")      # the smallest with an interior AND a ragged 8 x 32 pixel tile


def tail_inputs(hcase, pix, v):
    """tail_exact_inputs with head.2 channels c and c2 rebuilt: at pixel pix channel c is the hot value v = a w + d (d through a second
    reserved input channel, so that no other pixel changes), channel c2 is clamp(v) built the same way, both 0 elsewhere; head.4 reads
    them with +2^-5 and -2^-5, so their contributions cancel exactly IF channel c was clamped (65505 -> 65504) and are off by 2^-5
    per output (some 1e-2 of the result) if it was not.  The four pre-activations stay the integers of tail_exact_inputs' kind."""
    import gpu_checks as GC
    import helpers as HP
    cid, n, H, W_, variant, w4scale, cls = hcase
    (x, w2, b2, w4, b4), _pre = GC.tail_exact_inputs(hcase)
    x, w2, w4 = x.copy(), w2.copy(), w4.copy()
    free = [ch for ch in range(128) if not w4[:, ch].any()]
    c, c2 = free[0], free[1]
    ci = (5, 6, 70, 71)                                       # reserved input channels: hot a, hot d, companion a, companion d
    x[..., ci] = 0
    w2[:, ci, :, :] = 0
    w2[c] = 0; w2[c2] = 0
    (a, w_, d), _, _ = RC.HOT[v]
    vc = int(np.clip(v, -RC.F16_MAX, RC.F16_MAX))
    (a2, w2_, d2), _, _ = RC.HOT[vc]
    img, y, xx = pix
    x[img, y, xx, ci[0]] = a; x[img, y, xx, ci[1]] = d
    x[img, y, xx, ci[2]] = a2; x[img, y, xx, ci[3]] = d2
    w2[c, ci[0], 1, 1] = w_; w2[c, ci[1], 1, 1] = 1
    w2[c2, ci[2], 1, 1] = w2_; w2[c2, ci[3], 1, 1] = 1
    w4[:, c] = 2.0 ** -5; w4[:, c2] = -(2.0 ** -5)
    y2 = np.minimum(HP.conv_ref64(x, w2, b2, 1, 0, 2), F16_MAX)                  # head.2 + ReLU as the planes carry it: clamped
    pre = y2 @ w4.astype(np.float64).T + b4.astype(np.float64)
    assert np.array_equal(pre, np.rint(pre)) and np.abs(pre).max() <= 3 and y2[img, y, xx, c] == vc and y2[img, y, xx, c2] == vc
    return (x, w2, b2, w4, b4), pre


@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_fused_tail_saturates_head2(G, prec):
    """head_epilogue_t (halo form, forced family 8): head.2's ReLU output hot at one pixel and channel, in an interior tile and in a
    ragged one.  It reports on counter 0 only (its planes are fp16 hi / lo in every arithmetic), and points / confidence of the hot
    pixel equal the float64 activations of head.4 on the CLAMPED head.2 output within the ulp bounds of
    test_conv_exact.test_fused_tail_on_known_integers (6 / 2 ulp of the fp32 result).  Every other pixel: bit-identical to the launch
    without the + 1."""
    import helpers as HP
    from test_conv_exact import PTS_ULPS, CONF_ULPS
    cid, n, H, W_, variant, w4scale, cls = TAIL_CASE
    nA = 1

    def ulps(got, ref):
        return np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    for pix in [(0, 3, 7), (n - 1, H - 1, W_ - 1)]:           # interior tile (rows 0..7, x 0..31); ragged in rows and columns
        cold = {}
        for v in (57344, 57345, 65504, 65505):
            ins, pre = tail_inputs(TAIL_CASE, pix, v)
            want = (1, 0) if v > RC.F16_MAX else (0, 0)
            pts, conf, ran = G.tail_launch(prec, TAIL_CASE, nA, *ins, expect_range=want)
            assert ran == cls, ran
            rp, rc = HP.tail_activations64(pre)
            up, uc = ulps(pts, rp), ulps(conf, rc)
            print(f"[range] tail {prec} hot pixel {pix} = {v}: pts {up[pix].max():.2f} ulp, conf {uc[pix]:.2f} ulp; all pixels {up.max():.2f} / {uc.max():.2f}")
            assert np.isfinite(pts).all() and np.isfinite(conf).all()
            assert up[pix].max() <= PTS_ULPS and uc[pix] <= CONF_ULPS, (pix, v, pts[pix], rp[pix], conf[pix], rc[pix])
            assert up.max() <= PTS_ULPS and uc.max() <= CONF_ULPS
            base = v - RC.HOT[v][0][2]
            if base not in cold:
                ci, _ = tail_inputs(TAIL_CASE, pix, base)
                cold[base] = G.tail_launch(prec, TAIL_CASE, nA, *ci)[:2]
            other = np.ones(conf.shape, bool); other[pix] = False
            assert np.array_equal(pts[other].view(np.uint32), cold[base][0][other].view(np.uint32)), (pix, v)
            assert np.array_equal(conf[other].view(np.uint32), cold[base][1][other].view(np.uint32)), (pix, v)


# ------------------------------------------------------------------------------------------ QKV
QKV = dict(S=2, hp=3, wp=4, Cdim=128)


def qkv_inputs(K, v):
    """x in the decoder's row order [S*ntok patch rows | S pose rows], W [3C, K], bias: integers in {-1, 0, 1}; K columns 0 .. 5 carry
    the hot products alone (a w and d 1, two columns per hot element): three hot elements - Q at (sequence 1, token 0), K at (sequence 0, token 0), both at grid
    position (0, 0), where the rotation is the identity, and V on the pose row of sequence 1: the last, partly filled group of four rows."""
    S, ntok, Cd = QKV["S"], QKV["hp"] * QKV["wp"], QKV["Cdim"]
    M = S * ntok + S
    rs = np.random.default_rng(23 + K)
    x = rs.integers(-1, 2, size=(M, K)).astype(np.float32)
    Wt = rs.integers(-1, 2, size=(3 * Cd, K)).astype(np.float32)
    b = rs.integers(-2, 3, size=3 * Cd).astype(np.float32)
    x[:, :6] = 0; Wt[:, :6] = 0
    hots = [(ntok, 0 * Cd + 64 + 5), (0, 1 * Cd + 3), (M - 1, 2 * Cd + Cd - 1)]
    a, w, d = v if isinstance(v, tuple) else RC.HOT[v][0]
    for r, c in hots:
        x[r, :] = 0; Wt[c, :] = 0; b[c] = 0
    for i, (r, c) in enumerate(hots):                        # its own two K columns each: no hot row meets another's hot column
        x[r, 2 * i] = a; x[r, 2 * i + 1] = d
        Wt[c, 2 * i] = w; Wt[c, 2 * i + 1] = 1
    # where the three land: q[s, head, t, dcol], k[...], vt[s, head, dcol, t]
    where = [("q", (1, 1, 0, 5)), ("k", (0, 0, 0, 3)), ("v", (1, 1, 63, ntok))]
    return x, Wt, b, where


def run_qkv(G, prec, K, want_split, values):
    S, ntok = QKV["S"], QKV["hp"] * QKV["wp"]
    cold = {}
    for v in values:
        (a, w, d), want, _ = RC.HOT[v]
        x, Wt, b, where = qkv_inputs(K, v)
        q, k, vt, rng, plan = G.range_qkv_rope(prec, x, Wt, b, S, ntok, QKV["Cdim"], QKV["wp"])
        assert (plan["ksplit"] > 1) == want_split, plan
        if (a, w) not in cold:
            xc, Wc, bc, _ = qkv_inputs(K, (a, w, 0))
            cold[(a, w)] = G.range_qkv_rope(prec, xc, Wc, bc, S, ntok, QKV["Cdim"], QKV["wp"])[:3]
        got = {"q": q, "k": k, "v": vt}
        print(f"[range] qkv K {K} {prec} hot {v}: report {rng}, stored {[float(got[n][i]) for n, i in where]}")
        if want_split:
            assert RC.range_class(rng) == want, (v, rng, want)
        for name, idx in where:
            assert float(got[name][idx]) == stored(v, prec), (name, idx, float(got[name][idx]), stored(v, prec))
        for name, cg in zip(("q", "k", "v"), cold[(a, w)]):
            g = got[name].copy(); cc = cg.copy()
            for nm, idx in where:
                if nm == name:
                    g[idx] = cc[idx] = 0
            live = ~np.isnan(cc) if name != "v" else np.ones(cc.shape, bool)
            assert np.isfinite(g[live]).all(), name
            assert np.array_equal(g[live].view(np.uint32), cc[live].view(np.uint32)), (name, v, "other elements changed")


@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_qkv_finish_thresholds(G, prec):
    """qkv_finish_kernel: sta_debug_qkv_rope at K = 512, whose plan splits K (asserted from the launch's plan record)."""
    run_qkv(G, prec, 512, True, list(RC.HOT))


@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_exempt_qkv_epilogue_saturates(G, prec):
    """epilogue_qkv_tile (K = 128: no K slices) never flushes - q / k / v are linear maps of LayerNorm outputs -; it still saturates:
    the value only, the counters are not asserted either way."""
    run_qkv(G, prec, 128, False, [65505, -65505])


# ------------------------------------------------------------------------------------------ the rotation kernels
POS_MAX = 40
INV = 100.0 ** (-np.arange(16, dtype=np.float64) / 16.0)


def rotate64(rows, pos):
    """rows [R, 64] float64, pos [R, 2] (y, x) -> the 2-D rotation of every row (pairs (d, d + 16) of each 32-wide half)."""
    out = rows.copy()
    for xy in range(2):
        ang = pos[:, xy, None].astype(np.float64) * INV[None]
        c, s = np.cos(ang), np.sin(ang)
        v0, v1 = rows[:, xy * 32:xy * 32 + 16], rows[:, xy * 32 + 16:xy * 32 + 32]
        out[:, xy * 32:xy * 32 + 16] = v0 * c - v1 * s
        out[:, xy * 32 + 16:xy * 32 + 32] = v1 * c + v0 * s
    return out


ROPE_ENTRIES = {
    # entry -> (kwargs of gpu_checks.range_rope, tokens per sequence, pose row?, guard block?)
    "tokens_one_launch": ("tokens", dict(S1=1, S2=1, heads=2, na=63, nb=64, which=0), [63, 64], True, False),
    "planes_per_buffer": ("tokens", dict(S1=1, S2=1, heads=2, na=63, nb=64, which=1), [63, 64], True, False),
    "encoder_tokens": ("enc", dict(S=2, heads=2, ntok=63), [63, 63], False, True),
    "encoder_tokens_64": ("enc", dict(S=2, heads=2, ntok=64), [64, 64], False, True),
    "varlen": ("varlen", dict(S=2, heads=2, n=[64, 13]), [64, 13], True, True),
}
# (v0, v1) at frequency 0, the position of the token (None: the pose row, position -1), exact?, the two results the fp64 rotation gives
ROPE_HOT = {
    "overflow": ((60000.0, 60000.0), 1, (1, 0)),          # r1 = 60000 (cos 1 + sin 1) = 82908 -> +65504
    "negative": ((-60000.0, -60000.0), 1, (1, 0)),        # -> -65504
    "boundary": ((65504.0, 65504.0), 0, (0, 0)),          # position 0: cos = 1, sin = 0 exactly: comes back as it went in
    "pose_row": ((60000.0, 60000.0), None, (1, 0)),       # position -1: r0 = 60000 (cos 1 + sin 1) -> +65504
}


@pytest.mark.parametrize("prec", RC.ARITHMETICS)
@pytest.mark.parametrize("entry", list(ROPE_ENTRIES))
def test_rope_kernels_saturate(G, entry, prec):
    """rope_tokens_kernel (decoder and encoder forms), rope_planes_kernel, rope_varlen_kernel: the only writers where operands inside
    the range leave it through the op itself.  One hot pair per launch, in the last token of the last sequence or in the first token
    of the second one, y half or x half.  Every other live element against the float64 rotation within the bounds of
    test_decode_tokens_gpu.test_rope_tokens_kernel_alone ((POS_MAX + 2) 2^-21 (|v0| + |v1|); f16 adds its output rounding, 2^-11 of the
    result); rows no token owns come back bit for bit.  (Q / K are f16x3 planes under "head_mx" too: that arithmetic differs only
    inside the DPT head, so its run repeats f16x3 on the handle the head tests use.)"""
    kind, kw, counts, has_pose, guard = ROPE_ENTRIES[entry]
    heads = kw["heads"]
    S = len(counts)
    npad = (max(counts) + (1 if has_pose else 0) + 63) // 64 * 64
    nblk = S * heads + (1 if guard else 0)
    rs = np.random.default_rng(3 + len(entry))
    base = (rs.integers(-1024, 1025, size=(nblk, npad, 64)) * 2.0 ** -8).astype(np.float32)
    pos = [rs.integers(0, POS_MAX + 1, size=(nt, 2)).astype(np.int32) for nt in counts]
    for name, ((v0, v1), hp_, want) in ROPE_HOT.items():
        if hp_ is None and not has_pose:
            continue
        for (s, hd, xp) in [(S - 1, heads - 1, 1), (1, 0, 0)]:
            t = counts[s] if hp_ is None else (counts[s] - 1 if (s, hd, xp) == (S - 1, heads - 1, 1) else 0)
            buf = base.copy()
            p = [q.copy() for q in pos]
            if hp_ is not None:
                p[s][t, xp] = hp_
            blk = s * heads + hd
            buf[blk, t, xp * 32] = v0; buf[blk, t, xp * 32 + 16] = v1
            (got,), rng = G.range_rope(prec, kind, [buf.reshape((S, heads, npad, 64) if kind == "tokens" else buf.shape)],
                                       np.concatenate([q.ravel() for q in p]), POS_MAX, **kw)
            got = got.reshape(nblk, npad, 64)
            ref = buf.astype(np.float64)
            live = np.zeros(buf.shape, bool)
            for ss in range(S):
                nrow = counts[ss] + (1 if has_pose else 0)
                pp = np.concatenate([p[ss], [[-1, -1]]], 0) if has_pose else p[ss]
                for h_ in range(heads):
                    ref[ss * heads + h_, :nrow] = rotate64(buf[ss * heads + h_, :nrow].astype(np.float64), pp)
                    live[ss * heads + h_, :nrow] = True
            a = np.abs(buf.astype(np.float64)).reshape(nblk, npad, 2, 2, 16)
            bound = (POS_MAX + 2) * 2.0 ** -21 * np.broadcast_to((a[..., 0, :] + a[..., 1, :])[..., None, :], a.shape).reshape(buf.shape)
            clamped = np.clip(ref, -F16_MAX, F16_MAX)
            if prec == "f16":
                bound = bound + 2.0 ** -11 * np.abs(clamped)
            hot = np.abs(ref) > F16_MAX
            tag = f"rope {entry} {prec} {name} at (sequence {s}, head {hd}, token {t}, half {xp})"
            print(f"[range] {tag}: report {rng}, pair -> {got[blk, t, xp * 32]}, {got[blk, t, xp * 32 + 16]}")
            assert np.isfinite(got).all(), tag
            assert RC.range_class(rng) == want, (tag, rng, want)
            assert hot.sum() == (1 if want[0] else 0), (tag, int(hot.sum()))
            assert np.array_equal(got[hot].astype(np.float64), clamped[hot]), (tag, got[hot], clamped[hot])
            if name == "boundary":
                assert got[blk, t, xp * 32] == v0 and got[blk, t, xp * 32 + 16] == v1, tag
            err = np.abs(got.astype(np.float64) - clamped)
            assert (err <= bound)[live & ~hot].all(), (tag, np.argwhere((err > bound) & live & ~hot)[:4].tolist())
            assert np.array_equal(got[~live].view(np.uint32), buf[~live].view(np.uint32)), (tag, "rows no token owns were written")


# ------------------------------------------------------------------------------------------ first writers: the INPUT leaves the range
BAD = {"65505": 65505.0, "+inf": np.inf, "-inf": -np.inf, "nan": np.nan}


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_input_converters_report_bad_values(G, prec, bad):
    """rows_to_planes_kernel (row-major form: q / k of sta_debug_attention and the buffers of sta_debug_rope_tokens; blocked and f16mx
    forms: sta_debug_up2) and pack_vt_kernel (v of sta_debug_attention): one element out of range or not finite - at the last valid
    key / row, column 63 - is reported on counter 0 (a NaN too: the running maximum is kept on the bit pattern) and stored as +-65504
    (the documented clamp turns a NaN into -65504: for a NaN only the report is asserted).  The stored value is read back where an
    entry returns it unchanged: pack_vt_kernel through a one-key attention (the output is v), the row-major form through a buffer row
    the rotation does not touch, the blocked and f16mx forms through the bilinear of a 1 x 1 image.  q / k of sta_debug_attention
    reach the output only through the softmax, which cannot tell 65504 from more: they are the same row-major form of the same kernel
    as the rotation buffers, and only their report is asserted."""
    val = BAD[bad]
    sat = None if bad == "nan" else float(np.clip(val, -F16_MAX, F16_MAX))
    rs = np.random.default_rng(41)
    S, heads, nq, nk = 1, 2, 5, 65
    q0 = np.zeros((S, heads, nq, 64), np.float32)
    k0 = rs.integers(-2, 3, size=(S, heads, nk, 64)).astype(np.float32)
    v0 = rs.integers(-8, 9, size=(S, heads, nk, 64)).astype(np.float32)
    out, rng = G.range_attention(prec, q0, k0, v0)
    assert rng == (0, 0), rng
    for which in "qkv":
        q, k, v = q0.copy(), k0.copy(), v0.copy()
        {"q": q, "k": k, "v": v}[which][S - 1, heads - 1, -1, 63] = val
        out, rng = G.range_attention(prec, q, k, v)
        print(f"[range] attention {prec} {which} <- {bad}: report {rng}")
        assert rng[0] > 0 and rng[1] == 0, (which, bad, rng)
        assert np.isfinite(out).all(), (which, bad)
    # pack_vt_kernel's stored value: one key, q = 0 -> the output IS v
    if sat is not None:
        v1 = v0[:, :, :1].copy(); v1[S - 1, heads - 1, 0, 63] = val
        out, rng = G.range_attention(prec, q0, k0[:, :, :1].copy(), v1)
        assert rng[0] > 0, rng
        assert out[S - 1, :, (heads - 1) * 64 + 63].tolist() == [sat] * nq, (bad, out[S - 1, :, (heads - 1) * 64 + 63])
    # rows_to_planes_kernel, row-major form: a row the rotation does not touch comes back as the planes hold it
    S1 = S2 = 1
    na, nb = 6, 12
    npad = 64
    buf = (rs.integers(-1024, 1025, size=(S1 + S2, 2, npad, 64)) * 2.0 ** -8).astype(np.float32)
    buf[-1, -1, npad - 1, 63] = val
    pos = rs.integers(0, POS_MAX + 1, size=((S1 * na + S2 * nb) * 2)).astype(np.int32)
    (got,), rng = G.range_rope(prec, "tokens", [buf], pos, POS_MAX, S1=S1, S2=S2, heads=2, na=na, nb=nb, which=0)
    print(f"[range] row-major rows_to_planes {prec} <- {bad}: report {rng}, stored {got[-1, -1, npad - 1, 63]}")
    assert rng[0] > 0 and rng[1] == 0, rng
    assert np.isfinite(got).all()
    if sat is not None:
        assert got[-1, -1, npad - 1, 63] == sat
    # blocked planes (f16x3 / f16) and f16mx rows (head_mx): the bilinear's input
    n, H, W_, Cd = 1, 3, 5, 64
    x = rs.integers(-8, 9, size=(n, H, W_, Cd)).astype(np.float32)
    out, rng = G.range_up2(prec, x, 2 * H, 2 * W_)
    assert rng == (0, 0), rng
    x[n - 1, H - 1, W_ - 1, Cd - 1] = val
    out, rng = G.range_up2(prec, x, 2 * H, 2 * W_)
    print(f"[range] blocked rows_to_planes {prec} <- {bad}: report {rng}")
    assert np.isfinite(out).all()
    assert rng[0] > 0 and (rng[1] > 0) == (prec == "head_mx"), rng
    # ... and the value those two forms store: a 1 x 1 image has interpolation ratios 0, every weight is exactly 1 or 0, so all four
    # output pixels ARE the stored plane value (f16mx rows: hi + lo8 2^-11 = 65504 + 0)
    x1 = rs.integers(-8, 9, size=(1, 1, 1, Cd)).astype(np.float32)
    x1[0, 0, 0, Cd - 1] = val
    out, rng = G.range_up2(prec, x1, 2, 2)
    print(f"[range] blocked rows_to_planes {prec} <- {bad}, 1 x 1 image: report {rng}, stored {out[0, :, :, Cd - 1].ravel()}")
    assert rng[0] > 0 and (rng[1] > 0) == (prec == "head_mx"), rng
    assert np.isfinite(out).all()
    assert np.array_equal(out[..., :Cd - 1], np.broadcast_to(x1[..., :Cd - 1], out[..., :Cd - 1].shape))
    if sat is not None:
        assert (out[0, :, :, Cd - 1] == sat).all(), (bad, out[0, :, :, Cd - 1])


@pytest.mark.parametrize("Hc", [2, 4, 6])
@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_bilinear_reports_its_own_rows(G, prec, Hc):
    """bilinear_up2_kernel is a convex combination and cannot overflow by itself.  An image of 65000 everywhere (inside the fp16 range,
    past the e5m2 one) gives (0, 0) on planes and fp8 events on f16mx rows - from the kernel's own flush, which sits in front of an
    early return: the input conversion counts at most one event per four values, the kernel one more per eight output values.
    H = 3: Hc = 4 is one full group of four output rows, Hc = 2 one partly filled group, Hc = 6 both."""
    n, H, W_, Cd = 1, 3, 5, 16
    x = np.full((n, H, W_, Cd), 65000.0, np.float32)
    out, rng = G.range_up2(prec, x, Hc, 2 * W_)
    print(f"[range] up2 {prec} Hc {Hc}: report {rng}")
    assert np.isfinite(out).all() and np.abs(out - 65000.0).max() <= (32.0 if prec == "f16" else 0.05), np.abs(out - 65000.0).max()
    if prec == "head_mx":
        assert rng[0] == 0 and rng[1] > x.size // 4, (rng, x.size // 4)
    else:
        assert rng == (0, 0), rng


@pytest.mark.parametrize("prec", ["f16x3", "f16", "f16x3h"])
def test_patch_gather_reports_a_pixel_out_of_range(G, prec):
    """(Product API: the precisions are the product's; "f16x3h" is the policy whose DPT head runs the "head_mx" arithmetic - the gathers
    themselves write f16x3 planes in it.)
    patch_gather_kernel (_encode_image) and patch_gather_tokens_kernel (encode_tokens) on the tiny model: one pixel of 1e5 in the last
    gathered patch.  The planes then hold 65504, exactly what they hold for a pixel of 65504 - so everything behind the gather is the
    same in both runs and the gather's event is the DIFFERENCE of the two reports."""
    import torch
    from vista_slam_amd import weights as W
    m = G.model("tiny", precision=prec)
    H, W_ = 48, 64
    img = W.synth_images(1, H, W_, seed=43, tag=0).copy()
    ts = torch.tensor([[H, W_]])
    index = torch.tensor([[0, 5, (H // 16) * (W_ // 16) - 1]])
    rep = {}
    for name, val in (("cold", 65504.0), ("hot", 1e5)):
        im = img.copy(); im[0, 2, H - 1, W_ - 1] = val
        d = G.dev(im)
        _, rep[name, "frame"] = G.with_range(m, lambda: m._encode_image(d, ts, normalize=False))
        _, rep[name, "tokens"] = G.with_range(m, lambda: m.encode_tokens(d, index=index))
    print(f"[range] patch gather {prec}: {rep}")
    for form in ("frame", "tokens"):
        assert rep["hot", form][0] > rep["cold", form][0], (form, rep)
        assert rep["hot", form][1] == rep["cold", form][1], (form, rep)


@pytest.mark.parametrize("prec", ["f16x3", "f16", "f16x3h"])
def test_patch_gather_u8_is_silent(G, prec):
    """The uint8 forms normalise into [-1, 1] and cannot overflow: an all-255 image leaves both counters at 0.  Precisions as in
    test_patch_gather_reports_a_pixel_out_of_range."""
    import torch
    m = G.model("tiny", precision=prec)
    H, W_ = 48, 64
    img = torch.full((1, H, W_, 3), 255, dtype=torch.uint8)
    index = torch.tensor([[0, 5, (H // 16) * (W_ // 16) - 1]])
    _, r1 = G.with_range(m, lambda: m.encode_u8hwc(img))
    _, r2 = G.with_range(m, lambda: m.encode_tokens_u8hwc(img, index=index))
    assert r1 == (0, 0) and r2 == (0, 0), (r1, r2)


@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_weight_repack_thresholds(G, prec):
    """repack_weight_kernel: one weight past the fp16 range -> counter 0 (every arithmetic packs the f16x3 planes); under f16mx one weight
    of 29 (29 x 16 = 464 > 448: the e4m3 byte saturates) -> counter 1, 28 -> nothing.  The weight meets a zero column of A."""
    M, N, K = 72, 128, 64
    for wv, want in ((28.0, (0, 0)), (-28.0, (0, 0)), (29.0, (0, 1 if prec == "head_mx" else 0)), (-29.0, (0, 1 if prec == "head_mx" else 0)),
                     (65504.0, (0, 1 if prec == "head_mx" else 0)), (65505.0, (1, 1 if prec == "head_mx" else 0))):
        A, Wt, b, ref = gemm_operands(M, N, K, 3, 7, 57344)
        A[:, 9] = 0
        Wt[N - 1, 9] = wv
        got, rng, plan = G.range_gemm(prec, A, Wt, b)
        ref = A.astype(np.float64) @ np.where(np.abs(Wt) > 100, 0, Wt).astype(np.float64).T + b.astype(np.float64)
        print(f"[range] repack {prec} weight {wv}: report {rng}")
        assert RC.range_class(rng) == want, (wv, rng, want)
        assert np.array_equal(got.astype(np.float64), ref), wv


# ------------------------------------------------------------------------------------------ LayerNorm: the row statistics
LN_BAD = {"nan": [np.nan], "+inf": [np.inf], "pair_1e20": [1e20, -1e20], "finite_3e18": [3e18, -3e18]}


def ln_rows(M, Cd, kind, at_end):
    x, g, b = ROWS.ln_inputs(M, Cd, "random")
    vals = LN_BAD[kind]
    cols = range(Cd - len(vals), Cd) if at_end else range(len(vals))
    for c, v in zip(cols, vals):
        x[M - 1, c] = v
    return x, g, b


@pytest.mark.parametrize("kind", list(LN_BAD))
@pytest.mark.parametrize("Cd", [768, 1024])
@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_layernorm_row_statistics(G, prec, Cd, kind):
    """ln_kernel (sta_debug_layernorm) and resid_ln_kernel (the slab path of sta_debug_gemm_resid_ln) do not watch values: they count a
    row whose statistics are not finite, or whose variance overflowed fp32 (rstd == 0: the row would silently become pure bias).
    M = 6: the last block of ln_kernel holds two rows, the bad one is the last.  NaN, +inf, or a pair +-1e20 at column 0 (the pivot) or at
    the row's end -> counter 0; a finite row of +-3e18 (variance 2 x 9e36 / C: finite in fp32) -> nothing.  Every other row keeps the
    float64 bounds of test_row_gpu.test_layernorm_rows."""
    M = 6
    want = (0, 0) if kind == "finite_3e18" else (1, 0)
    for at_end in (False, True):
        x, g, b = ln_rows(M, Cd, kind, at_end)
        o32, op, rng = G.range_layernorm(prec, x, g, b, ROWS.EPS)
        ref = ROWS.layernorm64(x[:M - 1], g, b)
        e32 = max(ROWS.worst(ROWS.row_rel_l2(o32[:M - 1], ref))[1], ROWS.worst(ROWS.row_max_rel(o32[:M - 1], ref))[1])
        ep = max(ROWS.worst(ROWS.row_rel_l2(op[:M - 1], ref))[1], ROWS.worst(ROWS.row_max_rel(op[:M - 1], ref))[1])
        print(f"[range] ln_kernel {prec} C {Cd} {kind} at_end {at_end}: report {rng}, other rows fp32 {e32:.2e} planes {ep:.2e}")
        assert RC.range_class(rng) == want, (rng, want)
        assert e32 < 1e-5 and ep < PLANE_BAR[prec], (e32, ep)
        if kind == "finite_3e18":
            assert np.isfinite(op).all() and np.isfinite(o32).all()
        # resid_ln_kernel: x' = x + A W^T + bias with the bad row in x; the K slices reach it through the slab
        K = 256
        rs = np.random.default_rng(9 + Cd)
        A = (rs.standard_normal((M, K)) * 1.3).astype(np.float32)
        Wt = (rs.standard_normal((Cd, K)) * 0.1).astype(np.float32)
        bias = rs.standard_normal(Cd).astype(np.float32)
        x2, o1, rng, plan = G.range_resid_ln(prec, A, Wt, bias, x, g, b, ROWS.EPS)
        assert plan["slab_ks"] > 1, plan                    # resid_ln_kernel ran
        ref = ROWS.layernorm64(x2[:M - 1], g, b)            # of the x' the GPU returned, as test_resid_ln does
        ep = max(ROWS.worst(ROWS.row_rel_l2(o1[:M - 1], ref))[1], ROWS.worst(ROWS.row_max_rel(o1[:M - 1], ref))[1])
        print(f"[range] resid_ln_kernel {prec} C {Cd} {kind} at_end {at_end}: report {rng}, other rows planes {ep:.2e}, plan {plan}")
        assert RC.range_class(rng) == want, (rng, want)
        assert ep < PLANE_BAR[prec], ep


# ------------------------------------------------------------------------------------------ exempt writers: the value only
@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_exempt_layernorm_planes_saturate(G, prec):
    """ln_store4 never flushes (a normalised row times the gains cannot leave the range).  It still saturates: gain 0 and bias 65505 make
    the affine output 65505 exactly; the planes hold 65504, the fp32 copy 65505."""
    M, Cd = 3, 8
    x = np.tile(np.array([1, -1, 1, -1, 2, -2, 2, -2], np.float32), (M, 1))
    g = np.ones(Cd, np.float32); b = np.zeros(Cd, np.float32)
    g[0] = 0; b[0] = 65505.0
    g[5] = 0; b[5] = -65505.0
    o32, op, rng = G.range_layernorm(prec, x, g, b, ROWS.EPS)
    print(f"[range] ln_store4 {prec}: report {rng} (not asserted), planes {op[:, 0]}, {op[:, 5]}")
    assert np.isfinite(op).all()
    assert (op[:, 0] == F16_MAX).all() and (op[:, 5] == -F16_MAX).all(), (op[:, 0], op[:, 5])
    assert (o32[:, 0] == 65505.0).all() and (o32[:, 5] == -65505.0).all()


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
def test_exempt_gelu_epilogue_saturates(G, prec):
    """mlp.fc1's epilogue (EPI_GELU: sta_debug_gemm(act = 1, via_f16 = 1) from M = 641 on) never flushes; gelu(65505) = 65505 in fp32 and
    the planes hold 65504.  Hot element in an interior sub-tile and at (M - 1, N - 1) of the ragged last tile.  The value only.
    f16x3 and f16: there is no GELU epilogue on the DPT head's f16mx rows (sta_debug_gemm_plan refuses epilogue 4 with mx for "head_mx");
    the f16mx form of this epilogue belongs to precision f16x3m and writes through the same split_mx1 the plane epilogue tests pin."""
    M, N, K = 648, 128, 64
    for (r, c) in [(0, 0), (M - 1, N - 1)]:
        A, Wt, b, ref = gemm_operands(M, N, K, r, c, 65505)
        got, rng, plan = G.range_gemm(prec, A, Wt, b, act=1)
        print(f"[range] gelu epilogue {prec} hot ({r}, {c}): report {rng} (not asserted), stored {got[r, c]}")
        assert np.isfinite(got).all()
        assert got[r, c] == F16_MAX, got[r, c]


@pytest.mark.parametrize("pose", [False, True])
@pytest.mark.parametrize("prec", RC.ARITHMETICS)
def test_attention_output_of_saturated_v(G, prec, pose):
    """The attention output (attn_body: never flushes; attn_pose_query: flushes per element) is a convex combination of V rows that
    pack_vt_kernel already clamped.  q = 0 makes it the exact mean over the keys: with V = 65504 in column 63 of every key the output
    is 65504 and NOTHING is reported - by either writer; with one key at 65505 the converter reports and the output is the mean of
    the clamped values."""
    S, heads = 1, 2
    nk = nq = 129 if pose else 4          # pose: n = 128 patch tokens, so the pose query is served by the pose blocks (attn_pose_query)
    rs = np.random.default_rng(77)
    q = np.zeros((S, heads, nq, 64), np.float32)
    k = rs.integers(-2, 3, size=(S, heads, nk, 64)).astype(np.float32)
    v = rs.integers(-8, 9, size=(S, heads, nk, 64)).astype(np.float32) * 4
    v[..., 63] = F16_MAX
    out, rng = G.range_attention(prec, q, k, v, pose=pose)
    col = out.reshape(-1, heads * 64)
    print(f"[range] attention pose {pose} {prec}: V = 65504 -> report {rng}, column 63 {col[:, 63]}")
    assert np.isfinite(out).all()
    assert rng == (0, 0), rng
    if pose:      # 129 keys: the mean's division is exact only where the kernel divides (the pose rows); the patch rows multiply by 1 / 129
        assert (col[-S:, 63] == F16_MAX).all() and (col[-S:, 127] == F16_MAX).all(), (col[-S:, 63], col[-S:, 127])
        assert (np.abs(col[:, [63, 127]] - F16_MAX) <= F16_MAX * 2.0 ** -22).all() and (col <= F16_MAX).all()
    else:
        assert (col[:, 63] == F16_MAX).all() and (col[:, 127] == F16_MAX).all()
        assert np.array_equal(col[:, :63].astype(np.float64), np.broadcast_to(v[0, 0, :, :63].astype(np.float64).mean(0), col[:, :63].shape))
    v[0, heads - 1, nk - 1, 63] = 65505.0
    out, rng = G.range_attention(prec, q, k, v, pose=pose)
    col = out.reshape(-1, heads * 64)
    assert rng[0] > 0 and rng[1] == 0, rng
    assert (np.abs(col[:, 127] - F16_MAX) <= (F16_MAX * 2.0 ** -22 if pose else 0)).all() and (col <= F16_MAX).all(), col[:, 127]
