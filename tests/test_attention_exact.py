"""GPU: every schedule of the attention kernel (csrc/attention.h), exactly and per row.

The cases are tests/attention_cases.py (one table; tests/test_attention_plan.py proves on the host that it holds every schedule
class a product launch can reach).  Every test asserts the schedule class its launch RAN under (sta_debug_last_attn_plan) and
nan == 0: the debug entry points poison the output planes, the K padding and the dead Q rows, so an element that was never stored
or a padded key that leaked is a NaN.

a. selection (bit exact, f16x3 and f16): every query selects one key with probability exactly 1 - integer operands, selected score
   exactly 0, every other one at least 160 log2 units below (asserted in float64 before the launch) - so the output must EQUAL the
   V row of the selected key.  V carries (sequence, head, key) in columns 0..2: a failure names the query, the key expected and
   the key returned.
b. uniform (q = 0): the output is the column mean of integer V over exactly nk (+ 1) keys.  The sums are exact in fp32; what is
   left is the rounding of 1 / l, of the product with it and of the hi + lo output split: |error| <= 2^-20 max|V| (f16x3).  The
   f16 form rounds its output to ONE fp16: half an fp16 ulp of the largest mean on top of that.  One key too many or too few
   moves the mean by about max|V| / (2 nk): hundreds of times the first bound, at 1025 keys still twice the second.
c. running maximum: score ramps that rise tile by tile (every tile rescales), fall tile by tile (the wave-uniform alpha == 1 skip
   on every tile after the first) or peak in the last tile / at the pose key, against the float64 softmax, worst row.
d. Gaussian inputs over the whole matrix: rel-L2 of every (sequence, query) row, the worst one asserted, and the whole-output
   figure under the bounds of test_gpu_kernels.py (2e-5 / 3e-3).

Bounds of c and d = 4 x the worst row of a numpy model of the documented arithmetic (helpers.attn_model: f16x3 = operands and P as
fp16 hi + lo, three products, fp32 accumulation, fp32 exp2 softmax; f16 = single fp16 roundings, fp32 row sum of the unrounded p)
run on the CPU on the same inputs against the same float64 reference; the factor 4 covers the summation order of the MFMAs and
the online rescaling, and the hardware exp2.  Model figures (worst row over the cases of the group, the case that sets it) and
bounds; test_attention_plan.py::test_row_bounds_come_from_the_model recomputes the model on those cases:

    group            precision   model worst row   case             bound (4 x)
    rise             f16x3       3.094e-05         n588             1.24e-04
    rise             f16         4.872e-04         n1024            1.95e-03
    fall             f16x3       4.773e-07         n1024            1.91e-06
    fall             f16         5.162e-04         n1024            2.06e-03
    peak             f16x3       3.872e-06         n588             1.55e-05
    peak             f16         4.852e-04         n1024            1.94e-03
    gauss sharp 1    f16x3       1.138e-06         q130_k1025       4.55e-06
    gauss sharp 1    f16         8.571e-04         pose768          3.43e-03
    gauss sharp 3    f16x3       3.262e-06         pose320          1.30e-05
    gauss sharp 3    f16         2.805e-03         n256             1.12e-02
    gauss sharp 6    f16x3       7.925e-06         pose588_shift    3.17e-05
    gauss sharp 6    f16         4.540e-03         pose588_shift    1.82e-02

(rise, f16x3: the scores reach 8 x 9 = 72, raw dot products 576 - fp32 accumulation of the three products at that magnitude is
what the model's 3e-5 is made of.)
"""
import pytest

import attention_cases as AC

pytestmark = pytest.mark.gpu

# (group, precision) -> (model worst row, case that sets it); the bound is 4 x the figure
MODEL = {("rise", "f16x3"): (3.094e-05, "n588"), ("rise", "f16"): (4.872e-04, "n1024"),
         ("fall", "f16x3"): (4.773e-07, "n1024"), ("fall", "f16"): (5.162e-04, "n1024"),
         ("peak", "f16x3"): (3.872e-06, "n588"), ("peak", "f16"): (4.852e-04, "n1024"),
         (1.0, "f16x3"): (1.138e-06, "q130_k1025"), (1.0, "f16"): (8.571e-04, "pose768"),
         (3.0, "f16x3"): (3.262e-06, "pose320"), (3.0, "f16"): (2.805e-03, "n256"),
         (6.0, "f16x3"): (7.925e-06, "pose588_shift"), (6.0, "f16"): (4.540e-03, "pose588_shift")}
GLOBAL_TOL = {"f16x3": 2e-5, "f16": 3e-3}          # the whole-output bounds of test_gpu_kernels.py


def row_bound(group, prec):
    return 4.0 * MODEL[(group, prec)][0]


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    return gpu_checks


IDS = [c[0] for c in AC.CASES]


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_selection_is_bit_exact(G, prec, case):
    pose_sel = "patch" if IDS.index(case[0]) % 2 else "self"
    r = G.check_attention_selection(prec, case, pose_sel=pose_sel)
    print(case[0], prec, pose_sel, {k: r[k] for k in ("class", "margin", "nan", "wrong")})
    assert r["class"] == case[8], r["class"]
    assert r["wrong"] == 0, f"{r['wrong']} wrong rows ({r['nan']} NaN elements); {r['first']}"
    assert r["nan"] == 0, r


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_uniform_scores_give_the_column_mean(G, prec, case):
    r = G.check_attention_uniform(prec, case)
    bound = 2.0 ** -20 * r["vmax"] + (r["half_ulp16"] if prec == "f16" else 0.0)
    print(case[0], prec, r, "bound", bound)
    assert r["class"] == case[8], r["class"]
    assert r["nan"] == 0, r
    assert r["max_abs"] <= bound, (r, bound)


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("pattern", AC.RAMP_PATTERNS)
@pytest.mark.parametrize("cid", AC.RAMP_CASES)
def test_running_maximum(G, prec, pattern, cid):
    case = AC.case_by_id(cid)
    r = G.check_attention_ramp(prec, case, pattern)
    print(cid, pattern, prec, r, "bound", row_bound(pattern, prec))
    assert r["class"] == case[8], r["class"]
    assert r["nan"] == 0, r
    assert r["worst_row"] < row_bound(pattern, prec), r


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_gaussian_rows(G, prec, case):
    sharp = AC.sharp_of(case[0])
    r = G.check_attention_rows(prec, case, sharp)
    print(case[0], prec, "sharp", sharp, r, "bound", row_bound(sharp, prec))
    assert r["class"] == case[8], r["class"]
    assert r["nan"] == 0, r
    assert r["worst_row"] < row_bound(sharp, prec), r
    assert r["rel_l2"] < GLOBAL_TOL[prec], r
