"""Host: every claim that tests/test_split_exact_gpu.py rests on (no GPU; tests/split_cases.py says what the operands are).

For every case of every table that the GPU tests run:
  * the restated fp16 split returns exactly (hi, q 2^-12) for every operand;
  * the sum of the magnitudes of all addends of an output element fits 24 bits in units of 2^-12 (assert_window inside the builders),
    and results stored as fp16 pairs stay below 2048 (store_pair / store_mx / store_f16 inside *_expected);
  * the float32 statements of the documented arithmetic - helpers.conv_model, helpers.attn_model, and a three-product float32 GEMM
    summed in a shuffled order - return the integer expectation bit for bit;
  * the tests can see what they are for: the expectation differs in at least 90 % of its elements from the hi-only result, from the
    full product with its lo lo term, and from the result with the lo rows of one operand rolled by 16;
  * the fp8 images of every value in the f16mx rows are exact;
  * the attention inputs whose scores the correction products decide are what split_cases.attn_decided_inputs says.
"""
import numpy as np
import pytest

import attention_cases as AC
import conv_cases as CC
import helpers as HP
import split_cases as SC

SEEN = 0.90


def _sensitive(want, hi_only, lolo, rolled, what):
    for name, other in (("hi-only", hi_only), ("with lo lo", lolo), ("lo rows rolled by 16", rolled)):
        f = SC.differs(want, other)
        assert f >= SEEN, f"{what}: the expectation differs from the {name} result in only {100 * f:.1f} % of its elements"


def test_fp8_images_are_exact():
    for name, (x, image) in SC.fp8_images().items():
        assert np.array_equal(x, image), (name, x, image)
    # the rounding restated here does round: 1.25 has three significant bits (e5m2 keeps two after the leading one -> tie to even),
    # 17 has five (e4m3 keeps four)
    assert SC.e5m2(np.array([1.25, 1.375, 0.5625]))[1] == 1.5 and SC.e5m2(np.array([1.125]))[0] == 1.0
    assert SC.e4m3(np.array([17.0]))[0] == 16.0 and SC.e4m3(np.array([19.0]))[0] == 20.0


def test_the_recipe_avoids_the_values_that_split_differently():
    """+-1 and +-2 with this lo do NOT split into (hi, lo) - the reason for hi = +-3; the check does see it."""
    for hi in (1, 2, -1, -2):
        p = (np.array([hi], np.int16), np.array([-3 * np.sign(hi)], np.int16))
        assert not SC.split_is(SC.value(p), p), hi
    assert not SC.split_holds(np.array([1.0 + 2.0 ** -12 + 2.0 ** -23], np.float32))


def test_store_mx_rounds_lo_to_e5m2():
    y = np.array([100.0 + 37 * SC.UNIT, 3.0 + 3 * SC.UNIT, -1027.0 - 1000 * SC.UNIT])
    got = SC.store_mx(y)
    # 100 + 37 x 2^-12: hi = 100, lo 2^11 = 18.5 -> e5m2 20 (three significant bits) -> 100 + 40 x 2^-12
    assert got[0] == 100.0 + 40 * SC.UNIT and got[1] == y[1] and got[2] == -1027.0 - 1024 * SC.UNIT


# ------------------------------------------------------------------------------------------------------------------------ GEMM
GEMM_SHAPES = sorted({(kw["M"], kw["N"], kw["K"], bool(kw.get("resid")), bool(kw.get("via_f16"))) for _p, kw in SC.gemm_cases()})


def _shuffled_f32_gemm(ops, rows, cols, rng):
    """The three product planes of the f16x3 arithmetic in float32, all 3 K addends of an element summed one after the other in a
    random order (np.cumsum in float32 is sequential)."""
    ah, al = SC.restated_split(SC.value(ops["A"])[rows])
    wh, wl = SC.restated_split(SC.value(ops["W"])[cols])
    prod = np.concatenate([ah[:, None, :] * wh[None], ah[:, None, :] * wl[None], al[:, None, :] * wh[None]], -1)
    return np.cumsum(prod[..., rng.permutation(prod.shape[-1])], axis=-1, dtype=np.float32)[..., -1].astype(np.float64)


@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=["M%d-N%d-K%d-resid%d-planes%d" % s for s in GEMM_SHAPES])
def test_gemm_cases(shape):
    M, N, K, resid, planes = shape
    ops = SC.gemm_operands(M, N, K, resid)               # (asserts the 24-bit window)
    for name in ("A", "W"):
        SC.assert_split(SC.value(ops[name]), ops[name], name)
    t = SC.gemm_terms(ops, HP.mm64, lolo=True)
    precs = [p for p, kw in SC.gemm_cases() if (kw["M"], kw["N"], kw["K"], bool(kw.get("resid")), bool(kw.get("via_f16"))) == shape]
    want = SC.gemm_expected(ops, t, "f16x3", planes)      # (asserts |result| < 2048 where it is stored as a pair)
    for p in precs:
        SC.gemm_expected(ops, t, p, planes)
    _sensitive(want, *(SC.gemm_expected(ops, t, "f16x3", planes, wrong=w) for w in ("hi_only", "lolo", "rolled")), f"GEMM {shape}")
    rng = np.random.default_rng(7)
    rows, cols = np.sort(rng.permutation(M)[:24]), np.sort(rng.permutation(N)[:24])
    sub = {"A": ops["A"], "W": ops["W"], "b": ops["b"] * 0, "R": None}
    assert np.array_equal(_shuffled_f32_gemm(sub, rows, cols, rng), (t["I"] + (t["T1"] + t["T2"]) * SC.UNIT)[np.ix_(rows, cols)])


# the QKV checks (gpu_checks.check_qkv_pair(ints=True): K = C = 768, 4 x 769 rows; check_qkv_rope_decoder_rows(ints=True): its rows)
@pytest.mark.parametrize("rows,N,K,v0", [((4, 769), 2304, 768, 1536), ((4, 769), 1536, 768, 768), ((2, 13), 384, 128, 256),
                                         ((2, 197), 384, 128, 256), ((4, 769), 384, 64, 256), ((4, 769), 1536, 64, 1024)])
def test_qkv_operands(rows, N, K, v0):
    for prec in ("f16x3", "f16"):
        x, w, b, want = SC.linear_operands(14, rows, N, K, prec, slice(v0, N), HP.mm64)       # (asserts split, window, |V| < 2048)
        assert want.shape == (rows[0] * rows[1], N - v0)
    hi_only = SC.linear_operands(14, rows, N, K, "f16", slice(v0, N), HP.mm64)[3]
    assert SC.differs(SC.linear_operands(14, rows, N, K, "f16x3", slice(v0, N), HP.mm64)[3], hi_only) >= SEEN


# ------------------------------------------------------------------------------------------------ convolutions and ConvTranspose
@pytest.mark.parametrize("case", CC.CASES, ids=[c[0] for c in CC.CASES])
def test_conv_cases(case):
    cid, n, H, W, Cin, Co, stride, relu_in, act, nres, variant, cls = case
    ops = SC.conv_operands(case, 33)
    for name, p in [("x", ops["x"]), ("w", ops["w"])] + [(f"residual {i}", r) for i, r in enumerate(ops["res"])]:
        SC.assert_split(SC.value(p), p, f"{cid} {name}")
    t = HP.split_conv_terms(ops, stride, lolo=True)
    b = SC.conv_bias(ops, t)
    SC.conv_window(ops, b)
    want = {p: SC.conv_expected(ops, t, b, p) for p in CC.ARITHMETICS}          # (asserts the 2048 bound of every store)
    assert np.array_equal(want["f16"], SC.conv_expected(ops, t, b, "f16x3", wrong="hi_only")) or nres
    _sensitive(want["f16x3"], *(SC.conv_expected(ops, t, b, "f16x3", wrong=w) for w in ("hi_only", "lolo", "rolled")), cid)
    if act == 2:
        assert 0.002 < (want["f16x3"] == 0).mean() < 0.08, "the output ReLU must still clamp, and only a few per cent"
    x, w, res = SC.value(ops["x"]), SC.value(ops["w"]), [SC.value(r) for r in ops["res"]]
    for p in ("f16x3", "f16"):
        model = HP.conv_model(x, w, b.astype(np.float32), stride, relu_in, act, res, p)
        assert np.array_equal(model, want[p]), f"{cid} {p}: helpers.conv_model differs in {(model != want[p]).sum()} elements"


@pytest.mark.parametrize("prec,kw,fam", SC.convt_rows())
def test_convt_cases(prec, kw, fam):
    ops = SC.convt_operands(kw["H"], kw["W_"], kw["Cdim"], kw["k"])
    for name in ("x", "w"):
        SC.assert_split(SC.value(ops[name]), ops[name], name)
    t = SC.convt_terms(ops, HP.mm64, lolo=True)
    want = SC.convt_expected(ops, t, prec)
    _sensitive(SC.convt_expected(ops, t, "f16x3"), *(SC.convt_expected(ops, t, "f16x3", wrong=w) for w in ("hi_only", "lolo", "rolled")), str(kw))
    assert want.shape == (2, kw["H"] * kw["k"], kw["W_"] * kw["k"], kw["Cdim"])
    # the scatter, restated with torch: the float64 ConvTranspose2d of the values, less its lo lo term
    import torch
    x, w = (torch.from_numpy(SC.value(ops[n_]).astype(np.float64)) for n_ in ("x", "w"))
    full = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), w, torch.from_numpy(ops["b"]), stride=kw["k"]).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(full, SC.convt_expected(ops, t, "f16x3", wrong="lolo"))


# ------------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("case", AC.CASES, ids=[c[0] for c in AC.CASES])
def test_attention_values(case):
    cid, form, S, heads, nq, nk, kv_shift, opt5, cls = case
    q, k, v, pi, margin = HP.attn_selection_inputs(form, S, heads, nq, nk, "self", 21)
    vl = SC.attn_v_with_lo(v, 21)
    assert SC.split_holds(vl)
    hi, lo = SC.restated_split(vl)
    assert (lo[..., 3:] != 0).mean() >= SEEN and np.array_equal(vl[..., :3], v[..., :3])
    u = HP.attn_uniform_inputs(form, S, heads, nq, nk, 22)[2]
    ul, unit = SC.attn_uniform_lo(u, 22)                 # (asserts that the column sums fit the 24-bit window)
    assert SC.split_is(ul, (u, np.rint((ul.astype(np.float64) - u) * 4096)))
    lo = ul.astype(np.float64) - u
    assert (np.abs(lo) >= 0.125).all() and (np.abs(lo) < 0.25).all() and np.array_equal(lo * 32, np.rint(lo * 32))
    assert (np.sign(lo) == np.sign(lo[0, 0, 0])).all(), "one sign per column"
    # leaving the lo plane of the last 64-key tile out moves the mean past the bound of the test
    m = min(64, ul.shape[2])
    assert np.abs(lo[:, :, -m:]).sum(2).min() / ul.shape[2] > 2.0 ** -20 * 2048


MODEL_CASES = ("n65", "q70_k130", "n130_opt5", "pose129", "pose12", "n1")


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("cid", MODEL_CASES)
def test_attn_model_returns_both_parts_of_the_selected_row(cid, prec):
    _cid, form, S, heads, nq, nk, kv_shift, opt5, cls = AC.case_by_id(cid)
    q, k, v, pi, margin = HP.attn_selection_inputs(form, S, heads, nq, nk, "self", 21)
    vl = SC.attn_v_with_lo(v, 21)
    idx = [(s - kv_shift) % S for s in range(S)]
    got = HP.attn_model(q, k[idx], vl[idx], kv_shift, prec)
    vw = vl.astype(np.float16).astype(np.float32) if prec == "f16" else vl
    assert np.array_equal(got, np.take_along_axis(vw, pi[..., None], 2).astype(np.float64))


@pytest.mark.parametrize("cid", SC.ATT_DECIDED_CASES)
def test_attention_decided_cases(cid):
    """(c): the split, the exact 0 of the selected score, the hi hi tie and the margins (attn_decided_assert); both kinds of pair in
    every case, pairs inside one 64-key tile and - where there are two tiles - across tiles; the pose key as selected key and as
    decoy; helpers.attn_model returns the expectation bit for bit (f16: the tie)."""
    _cid, form, S, heads, nq, nk, kv_shift, opt5, cls = AC.case_by_id(cid)
    d = SC.attn_decided_inputs(form, S, heads, nq, nk, 23)
    m_dec, m_rest = SC.attn_decided_assert(d)
    assert set(np.unique(d["family"])) == {0, 1}
    same = d["pi"] // 64 == d["dec"] // 64
    assert same.any() and (nk + (form == "pose") <= 64 or (~same).any())
    assert (d["ql"] != 0).any(-1).all() and ((d["kl"] != 0).any(-1).sum(-1) >= d["kl"].shape[2] - 1).all()         # (one key may be left without partner)
    if form == "pose":
        assert (d["pi"][..., :nq] == nk).any() and (d["dec"] == nk).any() and (d["pi"][..., nq] != nk).any()
    if nq <= 200:
        for p in AC.PRECISIONS:
            assert np.array_equal(HP.attn_model(d["q"], d["k"], d["v"], 0, p), SC.attn_decided_expected(d, p).astype(np.float64)), p
