"""GPU: the correction products of the split arithmetics, exactly.

Every other bit-exact test of the suite feeds operands that one fp16 holds, so lo == 0 and the two correction products of every
GEMM, convolution and attention launch multiply by zero there.  The operands of tests/split_cases.py have both parts non-zero and
still ONE right answer in every arithmetic: hi in {-3, 0, 3}, lo = q 2^-12, every product and every partial sum in any order inside
one 24-bit window of multiples of 2^-12 (asserted before every launch), so that

    f16x3 and f16mx ("mlp_mx", "head_mx")     I + J 2^-12      (I = sum hi hi', J = sum hi q' + q hi')
    f16                                       I                (lo ignored, not half-applied)

and the comparison is equality.  The expectation is integer arithmetic on (hi, q), not helpers.conv_model / attn_model
(tests/test_split_exact_cpu.py shows that those return the same bits, and that the expectation differs from the hi-only value, from
the product with a lo lo term and from the one with the lo rows rolled by 16 in more than 90 % of the elements of every case).  A
failure names the first wrong element with the value found, the right one and the hi-only one.

1. GEMM: the case tables of tests/test_gemm_mfma16.py (every tile family, row tail, K split and epilogue) with their plan assertions.
2. QKV epilogues: the decoder-row launch with split operands, the un-rotated V columns exact in both parts (the paired launch:
   test_gpu_kernels.py::test_qkv_pair, whose `ints` rows now carry a lo part).  Q and K are rotated: they keep their bars.
3. 3x3 convolutions: every row of tests/conv_cases.py in all three arithmetics, input ReLU by the sign of hi, integer bias,
   residuals with a lo part; the ConvT rows of test_convt_dispatch_rows_integer_exact.
4. Attention: (a) the selection test with V = integer + lo: with p exactly 1 the output planes hold BOTH parts of the selected row -
   all rows of tests/attention_cases.py (V goes through pack_vt_kernel at 64-aligned and unaligned key counts), the two-group and the
   per-sequence forms; (b) the uniform test with a lo part of one sign per column (below);

   (c) Q K^T decided by the correction products (split_cases.attn_decided_inputs): the keys come in (selected, decoy) pairs that tie
   at exactly 0 in hi hi; q_hi k_lo (even pairs: the decoy has the selected key's hi and its own lo) or q_lo k_hi (odd pairs: the
   decoy's hi moves from one dimension to another where q_hi is equal and q_lo differs) alone put the decoy 738 log2 units or more
   below, every other key lies millions below through hi hi.  |q_hi| = 8192, |k_hi| = 2048, dimension 63 cancels the 63 code products;
   every product is a multiple of 2^11 under 2^31 (asserted in float64 with the rest before the launch).  The output must equal the
   selected V row, both parts; in f16 the decoy TIES and the output is the fp16 mean of the hi parts of the two rows.  Cases
   (split_cases.ATT_DECIDED_CASES): every tail kind of both schedules, all three pose modes, kv shifts; a quarter of every 64-key tile
   pairs up inside the tile, the other keys across tiles; the pose key is a selected key or a decoy.

Stores.  fp32 and fp16 hi + lo pairs hold the result exactly (|result| < 2048, asserted).  An f16mx OUTPUT row keeps e5m2(lo 2^11) in
its second byte (sta_common.h: split_mx4): a documented rounding of the stored lo to three significant bits, restated in
split_cases.store_mx - the head_mx plane outputs are compared with that value, again by equality.  It hides a single missing product
where |result| is large (the lo of a result near 100 is kept to 2^-8); a dropped or misplaced lo FRAGMENT moves J by hundreds of
units and is seen; the mlp_mx rows (fp32 epilogues) see every single product.

(b) in detail.  q = 0, V = 1024 +- 64 (2048 at three keys) + lo, lo a multiple of 2^-5 below half an ulp, one sign per column, so the
lo parts of any set of keys add up; the column sums stay exact in fp32 (split_cases.attn_uniform_lo: |lo| in {4 .. 7} x 2^-5 up to 255
keys, 4 x 2^-5 for all keys of longer rows).  The bound stays the one of test_attention_exact.py, 2^-20 max|V| = 2^-9 (f16: + half an
fp16 ulp of the mean, which is the mean of the hi parts).  What it catches: the mean of nk keys moves by (sum of the dropped lo) / nk,
at least 0.125 m / nk for m keys - the lo plane of one 64-key tile at every nk of the table (64 x 0.125 / 1026 = 2^-7), of one 16-key
fragment up to nk = 1024, of a single key up to nk = 64.

Not covered here, and why: P's own lo part needs a non-trivial p and has no exact answer (ramp and Gaussian bounds of
test_attention_exact.py); the rotated Q / K of the QKV epilogues (their bars); the fused tail passes through expm1 (ulp test of
test_conv_exact.py).

Measured on the MI355X: wrong == 0 in every case and arithmetic, f16mx included - the block-scaled fp8 MFMA accumulates these addends
exactly, which was derived (multiples of 3 x 2^-12 inside 24 bits) and not known before; the uniform test with lo parts: max |error|
2.4e-4 (n63, bound 2^-9 = 1.95e-3), 0 at n1024.
"""
import pytest

import attention_cases as AC
import attention_mixed_cases as AM
import attention_varlen_cases as AV
import conv_cases as CC
import split_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    return gpu_checks


@pytest.fixture(scope="module")
def GM():
    import gpu_checks_mixed
    return gpu_checks_mixed


@pytest.fixture(scope="module")
def GV():
    import gpu_checks_varlen
    return gpu_checks_varlen


# rows of one shape next to each other: the operands and their integer sums are computed once per shape
GEMM = sorted(SC.gemm_cases(), key=lambda c: SC.gemm_id("", c[1]))


@pytest.mark.parametrize("prec,kw", GEMM, ids=[SC.gemm_id(p, kw) for p, kw in GEMM])
def test_gemm_is_bit_exact(G, prec, kw):
    r = G.check_gemm_split(prec, **kw)
    print(SC.gemm_id(prec, kw), r["plan"], {k: r[k] for k in ("nan", "wrong")})
    assert r["wrong"] == 0, f"{r['wrong']} wrong elements ({r['nan']} NaN); {r['first']}"


# the decoder-row QKV launch (rows of test_gpu_kernels.py::test_qkv_rope_decoder_rows)
@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("kw", [dict(plan=(6, 0)), dict(hp=14, wp=14, S=2, plan=(6, 0)), dict(hp=24, wp=32, S=4, K=64, plan=(6, 0)),
                                dict(hp=24, wp=32, S=4, K=64, Cdim=512, plan=(5, 4))])
def test_qkv_decoder_rows_v_is_bit_exact(G, prec, kw):
    from test_gpu_kernels import TOL
    kw = dict(kw)
    plan = kw.pop("plan")
    r = G.check_qkv_rope_decoder_rows(prec, ints=True, **kw)
    print(prec, kw, r)
    assert (r["plan"]["family"], r["plan"]["m_tail"]) == plan, r
    assert r["v_exact_bad"] == 0, f"{r['v_exact_bad']} wrong V elements; {r['v_first']}"
    assert r["vpad_abs"] == 0.0, r
    assert r["q"] < TOL[prec] and r["k"] < TOL[prec] and r["q_pose"] < TOL[prec] and r["k_pose"] < TOL[prec], r


CONV_IDS = [c[0] for c in CC.CASES]


@pytest.mark.parametrize("prec", CC.ARITHMETICS)
@pytest.mark.parametrize("case", CC.CASES, ids=CONV_IDS)
def test_conv_is_bit_exact(G, prec, case):
    r = G.check_conv_split(prec, case)
    print(case[0], prec, {k: r[k] for k in ("class", "nan", "wrong", "max_abs")})
    assert r["class"] == case[11], r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong elements ({r['nan']} NaN); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec,kw,fam", SC.convt_rows())
def test_convt_is_bit_exact(G, prec, kw, fam):
    r = G.check_convt_split(prec, kw["H"], kw["W_"], kw["Cdim"], kw["k"], kw.get("variant", 0))
    plan = r["plan"]
    print(prec, kw, plan, {k: r[k] for k in ("nan", "wrong")})
    assert (plan["family"], plan["ksplit"], plan["m_tail"]) == (fam, 1, 0), plan
    assert fam != 6 or plan["tiles_m"] * plan["tiles_n"] > 256, plan
    assert r["wrong"] == 0, f"{r['wrong']} wrong elements ({r['nan']} NaN); {r['first']}"


ATT_IDS = [c[0] for c in AC.CASES]


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("case", AC.CASES, ids=ATT_IDS)
def test_attention_selection_returns_both_parts_of_v(G, prec, case):
    pose_sel = "patch" if ATT_IDS.index(case[0]) % 2 else "self"
    r = G.check_attention_selection(prec, case, pose_sel=pose_sel, v_lo=True)
    print(case[0], prec, pose_sel, {k: r[k] for k in ("class", "margin", "nan", "wrong")})
    assert r["class"] == case[8], r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong rows ({r['nan']} NaN elements); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec", AM.PRECISIONS)
@pytest.mark.parametrize("case", AM.CASES, ids=AM.IDS)
def test_mixed_attention_selection_returns_both_parts_of_v(GM, prec, case):
    pose_sel = "patch" if AM.IDS.index(case[0]) % 2 else "self"
    r = GM.check_selection(prec, case, pose_sel=pose_sel, v_lo=True)
    assert r["class"] == GM.claimed(case), r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong rows ({r['nan']} NaN elements); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec", AV.PRECISIONS)
@pytest.mark.parametrize("shift", AV.SHIFTS)
@pytest.mark.parametrize("case", AV.CASES, ids=AV.IDS)
def test_varlen_attention_selection_returns_both_parts_of_v(GV, prec, shift, case):
    pose_sel = "patch" if AV.IDS.index(case[0]) % 2 else "self"
    r = GV.check_selection(prec, case, shift, pose_sel=pose_sel, v_lo=True)
    assert r["class"] == GV.claimed(case), r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong rows ({r['nan']} NaN elements); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("case", AC.CASES, ids=ATT_IDS)
def test_attention_uniform_mean_includes_v_lo(G, prec, case):
    r = G.check_attention_uniform(prec, case, v_lo=True)
    bound = 2.0 ** -20 * r["vmax"] + (r["half_ulp16"] if prec == "f16" else 0.0)
    print(case[0], prec, r, "bound", bound)
    assert r["class"] == case[8], r["class"]
    assert r["nan"] == 0, r
    assert r["max_abs"] <= bound, (r, bound)


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("cid", SC.ATT_DECIDED_CASES)
def test_attention_scores_decided_by_the_correction_products(G, prec, cid):
    case = AC.case_by_id(cid)
    r = G.check_attention_decided(prec, case)
    print(cid, prec, {k: r[k] for k in ("class", "margin", "nan", "wrong")})
    assert r["class"] == case[8], r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong rows ({r['nan']} NaN elements); {r['first']}"
    assert r["nan"] == 0, r
