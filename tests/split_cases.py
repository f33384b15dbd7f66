"""Operands that give the split arithmetics ONE right answer (numpy only; tests/test_split_exact_cpu.py checks every claim made here
on the host, tests/test_split_exact_gpu.py runs the kernels on them).

An operand element is x = hi + lo with hi in {-3, 0, 3} and lo = q 2^-12, q in {-3 .. 3} \\ {0} (q = 0 where hi = 0).  3 sits in the
middle of a binade, so fp16 splits x into exactly (hi, lo): restated_split, asserted for every builder.  A product of two such
operands in the f16x3 arithmetic is hi hi' + hi lo' + lo hi' - in units of 2^-12: 4096 hi hi' + hi q' + q hi', at most TERM = 9 x 4096
+ 18 per k.  Whenever (non-zeros per weight row) x TERM + 4096 x (|bias| + |residuals|) < 2^24 (assert_window: an upper bound of the
sum of the magnitudes of all addends of every output element), every product and every partial sum IN ANY ORDER is a multiple of 2^-12
inside one 24-bit window: exact in fp32.  The result is then I + J 2^-12 with

    I = sum hi hi'        J = T1 + T2,   T1 = sum hi q',   T2 = sum q hi'        (integers)

computed here by float64 matrix products of integer-valued arrays (every partial sum below 2^53: the same integers int64 gives, on
BLAS).  The three arithmetics:

    f16x3            I + J 2^-12
    f16mx            the same: the fp8 copies of these values are exact (fp8_images), both correction products come to 3 q 2^-12
    f16              I: lo is ignored, not half-applied

and the stores: fp32 (as is); an fp16 hi + lo pair (exact while |y| < 2048: store_pair asserts it); one fp16 (f16: an integer below
2048); an f16mx row, whose second byte is e5m2(lo 2^11) - a DOCUMENTED rounding of the stored lo to three significant bits
(sta_common.h: split_mx4), restated in store_mx, so that the f16mx plane outputs have one right answer too.

Three wrong results that the tests must tell from the right one (sensitivity): the hi-only value I, the full product I + J 2^-12 +
L 2^-24 (L = sum q q': a lo lo term applied), and the value with the lo rows of one operand rolled by 16 (T2 of the GEMMs rolled by 16
rows, T1 of the convolutions by 16 output channels: a lo fragment fed to the neighbouring 16-row sub-block)."""
import numpy as np

UNIT = 2.0 ** -12
TERM = 9 * 4096 + 18              # |hi hi'| + |hi lo'| + |lo hi'| of one k at its largest, in units of 2^-12
WINDOW = 1 << 24
GEMM_NNZ, CONV_NNZ = 448, 400     # non-zeros per weight row where K is longer (448 x TERM = 2^23.98, 400 x TERM = 2^23.81)


# ---------------------------------------------------------------------------------------------------- operands and their split
def parts(rng, shape, zeros=True):
    """-> (hi, q) int16: hi in {-3, 0, 3} (zeros=False: {-3, 3}), q in +-{1, 2, 3}, 0 where hi = 0."""
    hi = 3 * (rng.integers(-1, 2, size=shape) if zeros else rng.integers(0, 2, size=shape) * 2 - 1)
    q = rng.integers(1, 4, size=shape) * (rng.integers(0, 2, size=shape) * 2 - 1)
    return hi.astype(np.int16), np.where(hi == 0, 0, q).astype(np.int16)


def thin_rows(rng, hi, q, keep):
    """At most `keep` non-zeros in every row of the 2-D (hi, q)."""
    rows, K = hi.shape
    if K <= keep:
        return hi, q
    mask = np.zeros((rows, K), bool)
    np.put_along_axis(mask, np.argsort(rng.random((rows, K)), axis=1)[:, :keep], True, 1)
    return hi * mask, q * mask


def residual_parts(rng, shape, lim=33):
    """A residual: hi = 3 r, |r| <= lim (a multiple of 3 is never a power of two, so both fp16 neighbours of hi are at least 2^-9 = 8 x
    2^-12 away and |lo| <= 3 x 2^-12 stays below half an ulp), q as in parts."""
    hi = 3 * rng.integers(-lim, lim + 1, size=shape)
    q = rng.integers(1, 4, size=shape) * (rng.integers(0, 2, size=shape) * 2 - 1)
    return hi.astype(np.int16), np.where(hi == 0, 0, q).astype(np.int16)


def value(p):
    """(hi, q) -> the float32 operand hi + q 2^-12 (exact: 14 bits)."""
    hi, q = p
    x = hi.astype(np.float64) + q.astype(np.float64) * UNIT
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return x.astype(np.float32)


def restated_split(x):
    """The split as the kernels do it: hi = fp16(x), lo = fp16(x - hi).  -> (hi, lo) float32."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    lo = (x - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def split_is(x, p):
    """Does fp16 split x into exactly (hi, q 2^-12)?"""
    hi, lo = restated_split(x)
    return bool(np.array_equal(hi, p[0].astype(np.float32)) and np.array_equal(lo.astype(np.float64), p[1].astype(np.float64) * UNIT))


def assert_split(x, p, what=""):
    assert split_is(x, p), f"{what}: fp16 does not split this operand into (hi, q 2^-12)"


def assert_window(nnz, extra, what=""):
    """nnz: the largest count of non-zeros in a weight row (an upper bound of the k with a non-zero product in any output element);
    extra: the largest |bias| + sum of the largest |residual| (+ 1 for their lo).  int64."""
    total = np.int64(nnz) * np.int64(TERM) + np.int64(4096) * np.int64(extra)
    assert total < WINDOW, f"{what}: sum of magnitudes {int(total)} = 2^{np.log2(float(total)):.2f} units of 2^-12 does not fit 24 bits"
    return int(total)


def row_nnz(hi):
    return int((np.asarray(hi).reshape(hi.shape[0], -1) != 0).sum(1).max())


# ------------------------------------------------------------------------------------------------------------- fp8 and stores
def _round_f16_bits(x, drop):
    """x (values an fp16 holds) rounded to nearest even on the low `drop` bits of its fp16 significand."""
    h = np.asarray(x, np.float64).astype(np.float16)
    assert np.array_equal(h.astype(np.float64), np.asarray(x, np.float64)), "not an fp16 value"
    b = h.view(np.uint16).astype(np.uint32)
    half = (1 << (drop - 1)) - 1
    r = ((b + half + ((b >> drop) & 1)) >> drop) << drop
    return r.astype(np.uint16).view(np.float16).astype(np.float64)


def e5m2(x):
    """RNE to OCP e5m2 = the upper byte of an fp16 (normal range, no saturation: asserted)."""
    r = _round_f16_bits(x, 8)
    assert np.isfinite(r).all() and (np.abs(r) <= 57344).all()
    return r


def e4m3(x):
    """RNE to OCP e4m3 for 2^-6 <= |x| <= 448 or 0 (the normal range; asserted): three mantissa bits."""
    x = np.asarray(x, np.float64)
    nz = x != 0
    assert ((np.abs(x[nz]) >= 2.0 ** -6) & (np.abs(x[nz]) <= 448)).all()
    return _round_f16_bits(x, 7)


def fp8_images():
    """{name: (values, their fp8 image)} of every value the f16mx rows hold of these operands: activation bytes e5m2(hi), e5m2(lo
    2^11); weight bytes e4m3(lo 2^15), e4m3(hi 2^4) (sta_common.h)."""
    hi = np.array([-3.0, 0.0, 3.0])
    lo = np.array([q * UNIT for q in range(-3, 4)])
    return {"act_hi": (hi, e5m2(hi)), "act_lo": (lo * 2.0 ** 11, e5m2(lo * 2.0 ** 11)),
            "w_lo": (lo * 2.0 ** 15, e4m3(lo * 2.0 ** 15)), "w_hi": (hi * 2.0 ** 4, e4m3(hi * 2.0 ** 4))}


def store_pair(y, what=""):
    """An fp16 hi + lo pair holds a multiple of 2^-12 below 2048 exactly (hi: ulp <= 1, lo = y - hi: at most 11 bits)."""
    y = np.asarray(y, np.float64)
    assert np.abs(y).max() < 2048, f"{what}: |result| reaches {np.abs(y).max()}"
    hi, lo = restated_split(y.astype(np.float32))
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), y), what
    return y


def store_f16(y, what=""):
    y = np.asarray(y, np.float64)
    assert np.abs(y).max() < 2048 and np.array_equal(y, np.rint(y)), what
    return y


def store_mx(y, what=""):
    """An f16mx ACTIVATION row (sta_common.h: split_mx4 / load_mx_act): hi = fp16(y), second byte e5m2((y - hi) 2^11); its value is
    hi + byte 2^-11.  lo = y - hi is a multiple of 2^-12 of at most 11 bits, so fp32 holds it and the one rounding is the e5m2."""
    y = np.asarray(y, np.float64)
    assert np.abs(y).max() < 2048, f"{what}: |result| reaches {np.abs(y).max()}"
    hi = y.astype(np.float16).astype(np.float64)
    return hi + e5m2((y - hi) * 2.0 ** 11) * 2.0 ** -11


def store(y, prec, planes, what=""):
    """The value read back of the exact result y: fp32 (planes=False) or the planes of the arithmetic."""
    if not planes:
        assert np.array_equal(np.asarray(y, np.float64).astype(np.float32).astype(np.float64), y), what
        return np.asarray(y, np.float64)
    return {"f16": store_f16, "f16x3": store_pair, "mlp_mx": store_pair, "head_mx": store_mx}[prec](y, what)


def mm64(a, b):
    """a [M, K], b [N, K] integer-valued -> a b^T in float64 (exact: every partial sum is an integer below 2^53)."""
    return np.asarray(a, np.float64) @ np.asarray(b, np.float64).T


def differs(a, b):
    """Fraction of elements in which two expectations differ."""
    return float((np.asarray(a) != np.asarray(b)).mean())


# ------------------------------------------------------------------------------------------------------------------------ GEMM
def _param(test, name):
    """The value list of the parametrize mark `name` of a test function."""
    return next(list(m.args[1]) for m in test.pytestmark if m.name == "parametrize" and m.args[0] == name)


def gemm_cases():
    """[(precision, kw)]: every row of the exact tests of tests/test_gemm_mfma16.py, in the arithmetic it runs there."""
    import test_gemm_mfma16 as TG
    exact = _param(TG.test_gemm_integer_exact, "kw")
    rows = [(p, kw) for p in ("f16x3", "f16") for kw in exact]
    rows += [(p, kw) for p in ("f16x3", "f16") for kw in TG.TAIL_CASES] + [("mlp_mx", kw) for kw in TG.MX_TAIL_CASES]
    return rows + list(TG.DISPATCH_CASES)


def gemm_id(prec, kw):
    return f"{prec}-M{kw['M']}-N{kw['N']}-K{kw['K']}-v{kw['variant']}" + ("-resid" if kw.get("resid") else "") + ("-planes" if kw.get("via_f16") else "")


def gemm_operands(M, N, K, resid=False, seed=0):
    """A [M, K] and W [N, K] as (hi, q) parts, integer bias, a residual with a fractional part (the in-place epilogue adds fp32 to
    fp32).  K <= 256: dense {-3, 0, 3}; longer: W rows of exactly GEMM_NNZ non-zeros."""
    rng = np.random.default_rng(1000 + seed)
    A = parts(rng, (M, K))
    W = parts(rng, (N, K)) if K <= 256 else thin_rows(rng, *parts(rng, (N, K), zeros=False), GEMM_NNZ)
    b = rng.integers(-8, 9, size=N).astype(np.int16)
    R = (rng.integers(-8, 9, size=(M, N)).astype(np.int16), rng.integers(-3, 4, size=(M, N)).astype(np.int16)) if resid else None
    assert_window(row_nnz(W[0]), 8 + (9 if resid else 0), f"GEMM {M}x{N}x{K}")
    return {"A": A, "W": W, "b": b, "R": R}


def gemm_terms(ops, mm=mm64, lolo=False):
    """-> {"I", "T1", "T2" (, "L")}: integer-valued float64 [M, N]."""
    (ah, aq), (wh, wq) = ops["A"], ops["W"]
    t = {"I": mm(ah, wh), "T1": mm(ah, wq), "T2": mm(aq, wh)}
    if lolo:
        t["L"] = mm(aq, wq)
    return t


def gemm_expected(ops, t, prec, planes, wrong=None):
    """The one right answer of the arithmetic `prec` (wrong: "hi_only" | "lolo" | "rolled" - the three wrong ones, in the f16x3
    arithmetic), and the store of the epilogue."""
    tail = ops["b"].astype(np.float64)[None, :]
    if ops["R"] is not None:
        tail = tail + ops["R"][0].astype(np.float64) + ops["R"][1].astype(np.float64) * UNIT
    if prec == "f16" or wrong == "hi_only":
        y = t["I"] + tail
    elif wrong == "lolo":
        y = t["I"] + (t["T1"] + t["T2"]) * UNIT + t["L"] * UNIT * UNIT + tail
        return y                                  # (not storable: compared as a float64 statement)
    elif wrong == "rolled":
        y = t["I"] + (t["T1"] + np.roll(t["T2"], 16, axis=0)) * UNIT + tail
    else:
        y = t["I"] + (t["T1"] + t["T2"]) * UNIT + tail
    return store(y, prec if wrong is None else "f16x3", planes and wrong is None, "GEMM")


def linear_operands(seed, rows, N, K, prec, v_cols, mm=mm64):
    """A linear layer of the QKV checks: x [*rows, K] and W [N, K] as hi + q 2^-12 (W rows thinned where K > 256), integer bias in
    [-2, 2].  -> x, W, b float32 and the ONE right value of the columns v_cols (a slice: the un-rotated V columns, stored as an fp16
    hi + lo pair; prec f16: the hi-only value) [prod(rows), len(v_cols)] float64."""
    rng = np.random.default_rng(seed)
    x = parts(rng, tuple(rows) + (K,))
    w = parts(rng, (N, K)) if K <= 256 else thin_rows(rng, *parts(rng, (N, K), zeros=False), GEMM_NNZ)
    b = rng.integers(-2, 3, size=N).astype(np.int16)
    assert_window(row_nnz(w[0]), 2, "QKV")
    for name, p_ in (("x", x), ("W", w)):
        assert_split(value(p_), p_, name)
    ops = {"A": (x[0].reshape(-1, K), x[1].reshape(-1, K)), "W": (w[0][v_cols], w[1][v_cols]), "b": b[v_cols], "R": None}
    return value(x), value(w), b.astype(np.float32), gemm_expected(ops, gemm_terms(ops, mm), prec, True)


# ------------------------------------------------------------------------------------------ 3x3 convolutions and ConvTranspose
def conv_operands(case, seed=0):
    """x NHWC, w [Co, Cin, 3, 3] as (hi, q) parts; residual parts (residual_parts).  9 Cin <= CONV_NNZ: dense {-3, 0, 3} weights;
    longer: exactly CONV_NNZ non-zeros per output channel.  One-pixel images (effective K = Cin) get inputs without zeros.  The bias
    is left to conv_bias: it needs I."""
    cid, n, H, W, Cin, Co, stride, relu_in, act, nres, variant, cls = case
    rng = np.random.default_rng(2000 + seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = parts(rng, (n, H, W, Cin), zeros=H * W > 1)
    K = 9 * Cin
    wh, wq = parts(rng, (Co, K)) if K <= CONV_NNZ else thin_rows(rng, *parts(rng, (Co, K), zeros=False), CONV_NNZ)
    w = (wh.reshape(Co, Cin, 3, 3), wq.reshape(Co, Cin, 3, 3))
    res = [residual_parts(rng, (n, Ho, Wo, Co)) for _ in range(nres)]
    return {"x": x, "w": w, "res": res, "rng": rng, "relu_in": relu_in, "act": act}


def conv_relu_in(x):
    """The input ReLU of the kernels looks at the sign of hi: both parts of a negative element become 0."""
    hi, q = x
    return np.where(hi < 0, 0, hi), np.where(hi < 0, 0, q)


def conv_bias(ops, t):
    """Integer bias in [-32, 32]; in front of an output ReLU shifted per channel so that about 2 % of the channel's sums are clamped:
    the ReLU still clamps thousands of elements, and the expectation can differ from the wrong ones in more than 90 % of all."""
    Co = t["I"].shape[-1]
    b = ops["rng"].integers(-32, 33, size=Co).astype(np.float64)
    if ops["act"] == 2:
        b += np.ceil(-np.percentile(t["I"].reshape(-1, Co), 2, axis=0))
    return b


def conv_window(ops, b):
    extra = int(np.abs(b).max()) + sum(int(np.abs(r[0]).max()) + 1 for r in ops["res"])
    return assert_window(row_nnz(ops["w"][0]), extra, "conv")


def conv_expected(ops, t, b, prec, wrong=None):
    """t: {"I", "T1" = x_hi * w_q, "T2" = x_q * w_hi (, "L")} NHWC float64, of the input after its ReLU."""
    split = prec != "f16" and wrong != "hi_only"
    J = 0.0
    if split:
        J = ((np.roll(t["T1"], 16, axis=-1) if wrong == "rolled" else t["T1"]) + t["T2"]) * UNIT
        if wrong == "lolo":
            J = J + t["L"] * UNIT * UNIT
    y = t["I"] + J + b
    if ops["act"] == 2:
        y = np.maximum(y, 0.0)
    for rh, rq in ops["res"]:
        y = y + rh.astype(np.float64) + (rq.astype(np.float64) * UNIT if split else 0.0)
    if wrong == "lolo":
        return y
    return store(y, prec if wrong is None else "f16x3", wrong is None, "conv")


def convt_rows():
    """[(precision, kw, family)] of test_convt_dispatch_rows_integer_exact (tests/test_gpu_kernels.py)."""
    import test_gpu_kernels as TK
    return _param(TK.test_convt_dispatch_rows_integer_exact, "prec,kw,fam")


def convt_operands(H, W, C, k, n=2, seed=0):
    """x NHWC [n, H, W, C], w [Cin, Cout, k, k] (ConvTranspose2d layout) as parts, integer bias.  K = C <= 256: dense."""
    rng = np.random.default_rng(3000 + seed + k)
    x, w = parts(rng, (n, H, W, C)), parts(rng, (C, C, k, k))
    b = rng.integers(-32, 33, size=C).astype(np.float64)
    assert_window(C, 32, "ConvT")
    return {"x": x, "w": w, "b": b, "k": k}


def convt_terms(ops, mm=mm64, lolo=False):
    """Stride = kernel: every output pixel (y k + ky, x k + kx) is one matrix product row.  -> terms NHWC [n, k H, k W, C]."""
    (xh, xq), (wh, wq), k = ops["x"], ops["w"], ops["k"]
    n, H, W, C = xh.shape

    def f(a, w):
        y = mm(a.reshape(-1, C), w.transpose(2, 3, 1, 0).reshape(k * k * C, C))          # [pixels, (ky, kx, co)]
        return np.asarray(y).reshape(n, H, W, k, k, C).transpose(0, 1, 3, 2, 4, 5).reshape(n, H * k, W * k, C)
    t = {"I": f(xh, wh), "T1": f(xh, wq), "T2": f(xq, wh)}
    if lolo:
        t["L"] = f(xq, wq)
    return t


def convt_expected(ops, t, prec, wrong=None):
    o = {"x": ops["x"], "w": ops["w"], "res": [], "act": 0}
    return conv_expected(o, t, ops["b"], prec, wrong)


# ------------------------------------------------------------------------------------------------------------------- attention
def attn_v_with_lo(v, seed):
    """V of the selection test + lo: every column but the id columns 0..2 gets q 2^-12, q in +-{1, 2, 3}.  Any such value IS an fp16
    hi + lo pair (split_holds), whichever hi fp16 rounds to; with p exactly 1 the output planes must hold it."""
    rng = np.random.default_rng(4000 + seed)
    q = rng.integers(1, 4, size=v.shape) * (rng.integers(0, 2, size=v.shape) * 2 - 1)
    q[..., :3] = 0
    out = (v.astype(np.float64) + q * UNIT).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v.astype(np.float64) + q * UNIT)
    return out


def split_holds(x):
    """x = fp16 hi + fp16 lo exactly?"""
    hi, lo = restated_split(x)
    return bool(np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), np.asarray(x, np.float64)))


def attn_uniform_lo(v, seed):
    """V of the uniform test (integers 1024 +- 64, some 2048) + lo: a multiple of 2^-5 below half an ulp (0.25 under 1024), ONE SIGN
    PER COLUMN, so that the lo parts of any set of keys add up.  Short key rows: |lo| in {4 .. 7} x 2^-5; where the column sum in
    units of 2^-5 would leave the 24-bit window (more than 2^19 / 2048 = 256 keys), |lo| = 4 x 2^-5 = 2^-3 for every key, and the sums
    are multiples of 2^-3 below 2^21.  -> v float32, the unit of the sums."""
    rng = np.random.default_rng(5000 + seed)
    nkt = v.shape[2]
    short = nkt * 2048 < (1 << 19)
    mag = rng.integers(4, 8, size=v.shape) if short else np.full(v.shape, 4)
    sign = np.where(np.arange(v.shape[-1]) % 2 == 0, 1, -1)
    out = v.astype(np.float64) + mag * sign * 2.0 ** -5
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    unit = 2.0 ** -5 if short else 2.0 ** -3
    assert np.abs(out).sum(2).max() / unit < WINDOW
    return out.astype(np.float32), unit


# ---- (c) Q K^T decided by the correction products.  Keys come in pairs (selected, decoy) whose hi hi scores TIE at exactly 0 for
# every query that selects the pair; only the correction products put the decoy below.  Values: query code dims +-8192 (+ lo +-1
# in one pair of dims), keys +-2048 (+ lo +-0.25), dim 63 = -63 x 512 (query) x 32768 (key) = -63 x 2^24 cancels the 63 code
# products of 2^24.  Every product is a multiple of 2^11 and the magnitudes of all addends of a score sum to less than 2^31: 20 bits,
# exact in fp32 in any order.  One log2 unit of the softmax is 1 / (0.125 log2 e) = 5.55 in the raw score.
ATT_Q, ATT_K, ATT_QL, ATT_KL, ATT_Q63, ATT_K63 = 8192.0, 2048.0, 1.0, 0.25, -63.0 * 512.0, 32768.0
ATT_SCALE_LOG2E = 0.125 * 1.44269504088896340736
ATT_DECIDED_CASES = ("n588_shift", "n130_opt5", "n64_opt5", "n63", "n65", "n130", "n196", "n128", "q70_k130", "pose640", "pose128",
                     "pose588", "pose520", "pose12_opt5", "pose196_shift", "pose129", "pose100", "pose12")


def _key_pairs(rng, nkt, pose_key, pose_is_base):
    """All keys but at most one, in (selected, decoy) pairs: a quarter of every 64-key tile pairs up INSIDE the tile, the rest across
    the whole key row.  The pose key (decoder form) is the selected key of its pair or the decoy of it."""
    same, pool = [], []
    for t0 in range(0, nkt, 64):
        keys = rng.permutation(np.arange(t0, min(t0 + 64, nkt)))
        n_in = 2 * (len(keys) // 4)
        same += [(int(keys[i]), int(keys[i + 1])) for i in range(0, n_in, 2)]
        pool += [int(j) for j in keys[n_in:]]
    pool = rng.permutation(pool)
    pairs = same + [(int(pool[i]), int(pool[i + 1])) for i in range(0, len(pool) - 1, 2)]
    if pose_key is not None:
        pairs = [((d, b) if (b == pose_key) != pose_is_base and pose_key in (b, d) else (b, d)) for b, d in pairs]
    return pairs


def attn_decided_inputs(form, S, heads, nq, nk, seed=0):
    """-> dict: q, k, v float32 (token layout of helpers.py), their parts qh, ql, kh, kl float64, pi and dec [S, heads, nqt] (the key
    every query selects and its decoy), family [S, heads, nqt]: 0 - q_hi k_lo separates (the decoy has the selected key's hi and its
    own lo), 1 - q_lo k_hi separates (the decoy's hi moves 2048 from one dim to another where q_hi is equal and q_lo differs)."""
    rng = np.random.default_rng(6000 + seed)
    nqt, nkt = (nq, nk) if form == "plain" else (nq + 1, nk + 1)
    assert nkt >= 2
    qh, ql = np.zeros((S, heads, nqt, 64)), np.zeros((S, heads, nqt, 64))
    kh, kl = np.zeros((S, heads, nkt, 64)), np.zeros((S, heads, nkt, 64))
    pi, dec, family = (np.zeros((S, heads, nqt), np.int64) for _ in range(3))
    sigma = np.where(np.arange(32) % 2 == 0, 1.0, -1.0)
    for s in range(S):
        for h in range(heads):
            pairs = _key_pairs(rng, nkt, nk if form == "pose" else None, (s + h) % 2 == 0)
            kh[s, h, :, :63] = ATT_K * (rng.integers(0, 2, size=(nkt, 63)) * 2 - 1)           # (a key left without partner)
            code = rng.integers(0, 2, size=(len(pairs), 63)) * 2.0 - 1
            ab = []
            for i, (b, d) in enumerate(pairs):
                c = code[i]
                a1, a2 = [(x, y) for x in range(3) for y in range(x + 1, 3) if c[x] == c[y]][0]
                ab.append((a1, a2))
                kh[s, h, b, :63] = kh[s, h, d, :63] = ATT_K * c
                kl[s, h, b, 8:40] = ATT_KL * c[8:40] * sigma                                # sum q_hi k_lo = 0
                if i % 2 == 0:
                    kl[s, h, d, 8:40] = -ATT_KL * c[8:40] * sigma                           # its own lo: cancels too ...
                    kl[s, h, d, 40:48] = -ATT_KL * c[40:48]                                 # ... and 8 dims of -2048
                else:
                    kl[s, h, d, 8:40] = kl[s, h, b, 8:40]
                    kh[s, h, d, a1], kh[s, h, d, a2] = 2 * ATT_K * c[a1], 0.0
            order = rng.permutation(len(pairs))
            for t in range(nqt):
                i = int(order[t % len(pairs)])
                if form == "pose" and t == nq:
                    i = next((j for j, p in enumerate(pairs) if p[0] == nk), i)
                c, (a1, a2) = code[i], ab[i]
                pi[s, h, t], dec[s, h, t], family[s, h, t] = pairs[i][0], pairs[i][1], i % 2
                qh[s, h, t, :63] = ATT_Q * c
                ql[s, h, t, a1], ql[s, h, t, a2] = -ATT_QL * c[a1], ATT_QL * c[a2]
    qh[..., 63], kh[..., 63] = ATT_Q63, ATT_K63
    v = rng.integers(-1024, 1025, size=(S, heads, nkt, 64)).astype(np.float32)
    v[..., 0] = np.arange(S)[:, None, None]; v[..., 1] = np.arange(heads)[None, :, None]; v[..., 2] = np.arange(nkt)
    return {"q": (qh + ql).astype(np.float32), "k": (kh + kl).astype(np.float32), "v": attn_v_with_lo(v, seed),
            "qh": qh, "ql": ql, "kh": kh, "kl": kl, "pi": pi, "dec": dec, "family": family}


def attn_decided_assert(d):
    """Everything the test rests on, in float64 on the parts (integers and quarters: exact): the fp16 split, the selected score
    exactly 0, the decoy tied in hi hi and at least 160 log2 units below in the sum, every other key at least 160 below through hi hi
    alone, 24 bits.  -> (smallest margin of a decoy, of another key) in log2 units."""
    qh, ql, kh, kl, pi, dec = (d[n] for n in ("qh", "ql", "kh", "kl", "pi", "dec"))
    for x, hi, lo in ((d["q"], qh, ql), (d["k"], kh, kl)):
        h_, l_ = restated_split(x)
        assert np.array_equal(h_, hi) and np.array_equal(l_, lo), "fp16 does not split q / k into these parts"
    # every product a multiple of 2^11
    assert not (qh[..., :63] % 8192).any() and not (kh[..., :63] % 2048).any() and not kl[..., 63].any() and not ql[..., 63].any()
    assert not (ql % 1).any() and not ((kl * 4) % 1).any() and qh[0, 0, 0, 63] * kh[0, 0, 0, 63] % 2048 == 0
    kt = lambda a: a.transpose(0, 1, 3, 2)
    shh = qh @ kt(kh)
    sc = shh + qh @ kt(kl) + ql @ kt(kh)
    mag = np.abs(qh) @ kt(np.abs(kh)) + np.abs(qh) @ kt(np.abs(kl)) + np.abs(ql) @ kt(np.abs(kh))
    assert mag.max() / 2048 < WINDOW
    sel = np.take_along_axis(sc, pi[..., None], 3)[..., 0]
    assert not sel.any(), "the selected score must be exactly 0"
    assert not np.take_along_axis(shh, dec[..., None], 3).any(), "the decoy must tie in hi hi"
    m_dec = float((-np.take_along_axis(sc, dec[..., None], 3) * ATT_SCALE_LOG2E).min())
    rest = shh.copy()
    np.put_along_axis(rest, pi[..., None], -np.inf, 3)
    np.put_along_axis(rest, dec[..., None], -np.inf, 3)
    m_rest = float((-rest * ATT_SCALE_LOG2E).min()) if rest.shape[3] > 2 else np.inf
    both = sc.copy()
    np.put_along_axis(both, pi[..., None], -np.inf, 3)
    assert m_dec > 160 and m_rest > 160 and float((-both * ATT_SCALE_LOG2E).min()) > 160, (m_dec, m_rest)
    return m_dec, m_rest


def attn_decided_expected(d, prec):
    """f16x3: the selected V row, both parts.  f16: lo is ignored, the decoy TIES (p = 1 for both): the mean of the hi parts of the
    two rows, rounded to fp16 once (the sum of two fp16 values of at most 1024 and its half are exact in fp32)."""
    if prec != "f16":
        return np.take_along_axis(d["v"], d["pi"][..., None], 2)
    vh = d["v"].astype(np.float16).astype(np.float32)
    mean = (np.take_along_axis(vh, d["pi"][..., None], 2).astype(np.float64) + np.take_along_axis(vh, d["dec"][..., None], 2)) * 0.5
    assert np.array_equal(mean.astype(np.float32).astype(np.float64), mean)
    return mean.astype(np.float16).astype(np.float32)
