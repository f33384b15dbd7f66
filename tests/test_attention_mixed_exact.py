"""GPU: the two-group attention kernel (csrc/attention.h: attn_mixed_kernel - the decoder's attention on view pairs of different
resolution), exactly and per row: the methods of tests/test_attention_exact.py on the cases of tests/attention_mixed_cases.py
(tests/test_attention_mixed_plan.py proves on the host that the table holds every group class a decoder launch can reach).

Every test asserts the classes BOTH groups of its launch ran under (sta_debug_last_attn_mixed_plan) and nan == 0: the debug entry
poisons the output planes, the K padding and the dead Q rows.

a. selection (bit exact): every query - the pose queries too - selects one key with probability exactly 1, so the output must
   EQUAL that key's V row.  Forced selections include key 0, key nk - 1, the first and last key of every 64-key tile and the pose
   key at index nk; with nq != nk in a group a kernel that reads the pose key at nq, takes a group's tile count or tail stage from
   the other group, or maps a workgroup to the wrong sequence returns another key's row, and the message names it.
b. uniform (q = 0): the column mean of integer V over exactly nk + 1 keys, bound as in test_attention_exact.py.
c. running maximum (rise / fall / peak ramps) and d. Gaussian inputs: per-row rel-L2 against the float64 softmax.

Row bounds of c and d: 4 x the worst row of the numpy model (helpers.attn_model) on the same inputs over the cases of the group,
computed when the test runs (gpu_checks_mixed.model_worst_row) - the rule of test_attention_exact.py evaluated for these shapes,
no constants of its own; the whole-output bounds are test_attention_exact.GLOBAL_TOL.
"""
import pytest

import attention_mixed_cases as AM
from test_attention_exact import GLOBAL_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def GM():
    import gpu_checks_mixed
    return gpu_checks_mixed


@pytest.mark.parametrize("prec", AM.PRECISIONS)
@pytest.mark.parametrize("case", AM.CASES, ids=AM.IDS)
def test_selection_is_bit_exact(GM, prec, case):
    pose_sel = "patch" if AM.IDS.index(case[0]) % 2 else "self"
    r = GM.check_selection(prec, case, pose_sel=pose_sel)
    print(case[0], prec, pose_sel, {k: r[k] for k in ("class", "margin", "nan", "wrong")})
    assert r["class"] == GM.claimed(case), r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong rows ({r['nan']} NaN elements); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec", AM.PRECISIONS)
@pytest.mark.parametrize("case", AM.CASES, ids=AM.IDS)
def test_uniform_scores_give_the_column_mean(GM, prec, case):
    r = GM.check_uniform(prec, case)
    bound = 2.0 ** -20 * r["vmax"] + (r["half_ulp16"] if prec == "f16" else 0.0)
    print(case[0], prec, r, "bound", bound)
    assert r["class"] == GM.claimed(case), r["class"]
    assert r["nan"] == 0, r
    assert r["max_abs"] <= bound, (r, bound)


@pytest.mark.parametrize("prec", AM.PRECISIONS)
@pytest.mark.parametrize("pattern", AM.RAMP_PATTERNS)
@pytest.mark.parametrize("cid", AM.RAMP_CASES)
def test_running_maximum(GM, prec, pattern, cid):
    case = AM.case_by_id(cid)
    bound = 4.0 * GM.model_worst_row("ramp", pattern, prec)
    r = GM.check_ramp(prec, case, pattern)
    print(cid, pattern, prec, r, "bound", bound)
    assert r["class"] == GM.claimed(case), r["class"]
    assert r["nan"] == 0, r
    assert r["worst_row"] < bound, (r, bound)


@pytest.mark.parametrize("prec", AM.PRECISIONS)
@pytest.mark.parametrize("case", AM.CASES, ids=AM.IDS)
def test_gaussian_rows(GM, prec, case):
    sharp = AM.sharp_of(case[0])
    bound = 4.0 * GM.model_worst_row("gauss", sharp, prec)
    r = GM.check_rows(prec, case, sharp)
    print(case[0], prec, "sharp", sharp, r, "bound", bound)
    assert r["class"] == GM.claimed(case), r["class"]
    assert r["nan"] == 0, r
    assert r["worst_row"] < bound, (r, bound)
    assert r["rel_l2"] < GLOBAL_TOL[prec], r
