"""GPU checks of the two-group attention kernel (attn_mixed_kernel through sta_debug_attention_mixed), shared by
tests/test_attention_mixed_exact.py: one launch of a case of tests/attention_mixed_cases.py and the four kinds of check of
tests/test_attention_exact.py on it.  Inputs, the float64 reference and the numpy model are the ones of tests/helpers.py, per group
in the decoder ("pose") form; k / v of a sequence are the keys it reads (the debug entry stores them where kv_shift points)."""
import ctypes as C
import functools

import numpy as np
import torch

import attention_mixed_cases as AM
import gpu_checks as G
import helpers as HP
import split_cases as SC
from vista_slam_amd import _lib


def groups_of(case):
    """-> [(S, nq, nk)] of group a and b (group b dropped when S2 == 0)."""
    cid, S1, S2, heads, nq_a, nk_a, nq_b, nk_b = case[:8]
    return [(S1, nq_a, nk_a)] + ([(S2, nq_b, nk_b)] if S2 else [])


def mixed_launch(precision, case, inputs):
    """inputs: [(q, k, v)] per group (token layout of helpers.py, pose token last) -> ([output per token [S, heads, nq + 1, 64]] per
    group, [class of the group the launch ran under]).  The output buffer starts as NaN and the debug entry poisons the planes."""
    cid, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, kv_shift, opt5 = case[:10]
    m, lib, h = G.kernel_handle(precision)
    d = [[G.dev(x) for x in grp] for grp in inputs]
    ptr = [x.data_ptr() for grp in d for x in grp] + [None] * (3 * (2 - len(d)))
    rows = S1 * (nq_a + 1) + S2 * (nq_b + 1)
    out = torch.full((rows, heads * 64), float("nan"), device=G.DEV)
    _lib.check(lib.sta_debug_set_option(h, 5, opt5))
    try:
        _lib.check(lib.sta_debug_attention_mixed(h, *ptr, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, kv_shift, out.data_ptr(), G.st()))
        torch.cuda.synchronize()
        buf = (C.c_int * AM.PLAN_INTS)()
        _lib.check(lib.sta_debug_last_attn_mixed_plan(h, buf))
        plan = AM.plan_dict(buf)
    finally:
        _lib.check(lib.sta_debug_set_option(h, 5, 0))
    o = out.cpu().numpy()
    got, r0 = [], 0
    for g, (S, nq, nk) in enumerate(groups_of(case)):
        got.append(HP.attn_rows_to_tokens(o[r0:r0 + S * (nq + 1)], "pose", S, heads, nq))
        r0 += S * (nq + 1)
    return got, [AM.group_class(plan, g, grp[1]) for g, grp in enumerate(groups_of(case))]


def claimed(case):
    return [case[10], case[11]][:len(groups_of(case))]


def check_selection(precision, case, pose_sel="self", seed=21, v_lo=False):
    """Every query selects one key with probability exactly 1: the output must EQUAL V[pi(query)].  V columns 0..2 = (sequence of the
    whole launch, head, key): a failure names what was expected and what came back."""
    heads, S1 = case[3], case[1]
    inputs, pis, margin = [], [], np.inf
    for g, (S, nq, nk) in enumerate(groups_of(case)):
        q, k, v, pi, mg = HP.attn_selection_inputs("pose", S, heads, nq, nk, pose_sel, seed + g)
        v[..., 0] += g * S1
        if v_lo:        # V = integer + lo (split_cases.attn_v_with_lo): both parts of the selected row must come back (f16: its hi)
            v = SC.attn_v_with_lo(v, seed + g)
            assert SC.split_holds(v)
        inputs.append((q, k, v)); pis.append(pi); margin = min(margin, mg)
    assert margin > 160, (case[0], margin)
    got, ran = mixed_launch(precision, case, inputs)
    wrong, nan, first = 0, 0, []
    for g, (S, nq, nk) in enumerate(groups_of(case)):
        vw = inputs[g][2].astype(np.float16).astype(np.float32) if v_lo and precision == "f16" else inputs[g][2]
        want = np.take_along_axis(vw, pis[g][..., None], 2)
        bad = np.argwhere((got[g] != want).any(-1))
        wrong += len(bad); nan += int(np.isnan(got[g]).sum())
        for s, h, t in bad[:4]:
            r = got[g][s, h, t]
            who = "pose query" if t == nq else f"query {t}"
            first.append(f"(group {'ab'[g]}, sequence {s + g * S1}, head {h}, {who}): expected key {pis[g][s, h, t]} (pose key = {nk}), "
                         f"got columns 0..2 = (sequence {r[0]:g}, head {r[1]:g}, key {r[2]:g}), {int((r != want[s, h, t]).sum())} of 64 columns differ")
    return {"class": ran, "margin": margin, "nan": nan, "wrong": wrong, "first": "; ".join(first)}


def check_uniform(precision, case, seed=22):
    """q = 0: the output is the column mean of V over exactly nk + 1 keys of the group."""
    heads = case[3]
    inputs = [HP.attn_uniform_inputs("pose", S, heads, nq, nk, seed + g) for g, (S, nq, nk) in enumerate(groups_of(case))]
    got, ran = mixed_launch(precision, case, inputs)
    res = {"class": ran, "nan": 0, "max_abs": 0.0, "vmax": 0.0, "half_ulp16": 0.0}
    for g, (q, k, v) in enumerate(inputs):
        ref = np.broadcast_to(v.astype(np.float64).mean(2, keepdims=True), got[g].shape)
        err = np.abs(got[g] - ref)
        res["nan"] += int(np.isnan(got[g]).sum())
        res["max_abs"] = max(res["max_abs"], float(np.nanmax(err)) if not np.isnan(err).all() else float("nan"))
        res["vmax"] = max(res["vmax"], float(np.abs(v).max()))
        res["half_ulp16"] = max(res["half_ulp16"], float(2.0 ** (np.floor(np.log2(np.abs(ref).max())) - 11)))
    return res


def _inputs(case, kind, what, seed):
    heads = case[3]
    if kind == "ramp":
        return [HP.attn_ramp_inputs("pose", S, heads, nq, nk, what, seed + g) for g, (S, nq, nk) in enumerate(groups_of(case))]
    return [HP.attn_gaussian_inputs("pose", S, heads, nq, nk, what, seed + g) for g, (S, nq, nk) in enumerate(groups_of(case))]


def _rows(precision, case, inputs):
    got, ran = mixed_launch(precision, case, inputs)
    worst, num, den, nan = 0.0, 0.0, 0.0, 0
    for g, (q, k, v) in enumerate(inputs):
        ref = HP.attn_ref64(q, k, v, 0)
        rows, _ = HP.attn_row_errors(got[g], ref)
        nan += int(np.isnan(got[g]).sum())
        worst = max(worst, float(np.nanmax(rows)) if not np.isnan(rows).all() else float("nan"))
        num += float(((got[g].astype(np.float64) - ref) ** 2).sum()); den += float((ref ** 2).sum())
    return {"class": ran, "nan": nan, "worst_row": worst, "rel_l2": float(np.sqrt(num / max(den, 1e-300)))}


def check_ramp(precision, case, pattern, seed=101):
    return _rows(precision, case, _inputs(case, "ramp", pattern, seed))


def check_rows(precision, case, sharp, seed=100):
    return _rows(precision, case, _inputs(case, "gauss", sharp, seed))


@functools.lru_cache(maxsize=None)
def model_worst_row(kind, what, precision):
    """The numpy model of the documented arithmetic (helpers.attn_model) against the float64 reference on the SAME inputs the GPU
    checks use: its worst (sequence, query) row over every case of the group (kind "ramp": AM.RAMP_CASES under pattern `what`; kind
    "gauss": the cases whose sharpness is `what`).  The tests' row bounds are 4 x this figure - no constants of their own."""
    cases = [AM.case_by_id(c) for c in AM.RAMP_CASES] if kind == "ramp" else [c for c in AM.CASES if AM.sharp_of(c[0]) == what]
    worst = 0.0
    for case in cases:
        for q, k, v in _inputs(case, kind, what, 101 if kind == "ramp" else 100):
            rows, _ = HP.attn_row_errors(HP.attn_model(q, k, v, 0, precision), HP.attn_ref64(q, k, v, 0))
            worst = max(worst, float(rows.max()))
    return worst
