"""GPU: the per-sequence attention kernel (csrc/attention.h: attn_varlen_kernel - the decoder's attention on batches whose entries
have their own token counts), exactly and per row: the methods of tests/test_attention_mixed_exact.py on the launches of
tests/attention_varlen_cases.py (tests/test_attention_varlen_plan.py proves on the host that the table holds every sequence class a
decoder call can reach).  Every launch has 3 to 8 sequences, each in a DIFFERENT class, and runs under kv_shift = 0 and S // 2.

Every test asserts the classes ALL sequences of its launch ran under (sta_debug_last_attn_varlen_plan) and nan == 0: the debug entry
poisons the output planes, the K padding and the dead Q rows.

a. selection (bit exact): every query - the pose queries too - selects one key with probability exactly 1, so the output must
   EQUAL that key's V row.  Forced selections include key 0, key nk - 1, the first and last key of every 64-key tile and the pose
   key at index nk; a kernel that takes a sequence's nk, tile count, tail stage or output row from its neighbour, or maps a
   workgroup to the wrong sequence, returns another key's row, and the message names it.
b. uniform (q = 0): the column mean of integer V over exactly nk + 1 keys, bound as in test_attention_exact.py.
c. running maximum (rise / fall / peak ramps) and d. Gaussian inputs: per-row rel-L2 against the float64 softmax.

Row bounds of c and d: 4 x the worst row of the numpy model (helpers.attn_model) on the same inputs over the cases of the group,
computed when the test runs (gpu_checks_varlen.model_worst_row); the whole-output bounds are test_attention_exact.GLOBAL_TOL.  No
constants of its own.
"""
import pytest

import attention_varlen_cases as AV
from test_attention_exact import GLOBAL_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def GV():
    import gpu_checks_varlen
    return gpu_checks_varlen


@pytest.mark.parametrize("prec", AV.PRECISIONS)
@pytest.mark.parametrize("shift", AV.SHIFTS)
@pytest.mark.parametrize("case", AV.CASES, ids=AV.IDS)
def test_selection_is_bit_exact(GV, prec, shift, case):
    pose_sel = "patch" if AV.IDS.index(case[0]) % 2 else "self"
    r = GV.check_selection(prec, case, shift, pose_sel=pose_sel)
    print(case[0], shift, prec, pose_sel, {k: r[k] for k in ("class", "margin", "nan", "wrong")})
    assert r["class"] == GV.claimed(case), r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong rows ({r['nan']} NaN elements); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec", AV.PRECISIONS)
@pytest.mark.parametrize("shift", AV.SHIFTS)
@pytest.mark.parametrize("case", AV.CASES, ids=AV.IDS)
def test_uniform_scores_give_the_column_mean(GV, prec, shift, case):
    r = GV.check_uniform(prec, case, shift)
    bound = 2.0 ** -20 * r["vmax"] + (r["half_ulp16"] if prec == "f16" else 0.0)
    print(case[0], shift, prec, r, "bound", bound)
    assert r["class"] == GV.claimed(case), r["class"]
    assert r["nan"] == 0, r
    assert r["max_abs"] <= bound, (r, bound)


@pytest.mark.parametrize("prec", AV.PRECISIONS)
@pytest.mark.parametrize("shift", AV.SHIFTS)
@pytest.mark.parametrize("pattern", AV.RAMP_PATTERNS)
@pytest.mark.parametrize("cid", AV.RAMP_CASES)
def test_running_maximum(GV, prec, shift, pattern, cid):
    case = AV.case_by_id(cid)
    bound = 4.0 * GV.model_worst_row("ramp", pattern, prec)
    r = GV.check_ramp(prec, case, shift, pattern)
    print(cid, shift, pattern, prec, r, "bound", bound)
    assert r["class"] == GV.claimed(case), r["class"]
    assert r["nan"] == 0, r
    assert r["worst_row"] < bound, (r, bound)


@pytest.mark.parametrize("prec", AV.PRECISIONS)
@pytest.mark.parametrize("shift", AV.SHIFTS)
@pytest.mark.parametrize("case", AV.CASES, ids=AV.IDS)
def test_gaussian_rows(GV, prec, shift, case):
    sharp = AV.sharp_of(case[0])
    bound = 4.0 * GV.model_worst_row("gauss", sharp, prec)
    r = GV.check_rows(prec, case, shift, sharp)
    print(case[0], shift, prec, "sharp", sharp, r, "bound", bound)
    assert r["class"] == GV.claimed(case), r["class"]
    assert r["nan"] == 0, r
    assert r["worst_row"] < bound, (r, bound)
    assert r["rel_l2"] < GLOBAL_TOL[prec], r
