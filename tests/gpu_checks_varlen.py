"""GPU checks of the per-sequence attention kernel (attn_varlen_kernel through sta_debug_attn_varlen), shared by
tests/test_attention_varlen_exact.py: one launch of a case of tests/attention_varlen_cases.py and the four kinds of check of
tests/test_attention_exact.py on it.  Inputs, the float64 reference and the numpy model are the ones of tests/helpers.py, per
sequence (S = 1 arrays) in the decoder ("pose") form; k / v of a sequence are the keys it reads (the debug entry stores them where
kv_shift points)."""
import ctypes as C
import functools

import numpy as np
import torch

import attention_varlen_cases as AV
import gpu_checks as G
import helpers as HP
import split_cases as SC
from vista_slam_amd import _lib


def varlen_launch(precision, case, shift, inputs):
    """inputs: [(q, k, v)] per sequence ([1, heads, n + 1, 64], pose token last) -> ([output [1, heads, nq + 1, 64]] per sequence,
    [class the sequence ran under]).  The output buffer starts as NaN and the debug entry poisons the planes.  The guard block that
    the entry keeps directly behind the output planes (every byte 0x3C: fp16 1.05859375 in each plane) must come back bit for bit:
    asserted here, so in every test of the kernel."""
    cid, heads, opt5, seqs = case[:4]
    S = len(seqs)
    m, lib, h = G.kernel_handle(precision)
    q, k, v = (G.dev(np.concatenate([x[i].ravel() for x in inputs])) for i in range(3))
    nq, nk = [s[0] for s in seqs], [s[1] for s in seqs]
    rows = sum(n + 1 for n in nq)
    out = torch.full((rows + AV.GUARD_ROWS, heads * 64), float("nan"), device=G.DEV)
    _lib.check(lib.sta_debug_set_option(h, 5, opt5))
    try:
        _lib.check(lib.sta_debug_attn_varlen(h, q.data_ptr(), k.data_ptr(), v.data_ptr(), S, heads, (C.c_int * S)(*nq), (C.c_int * S)(*nk),
                                             AV.kv_shift(case, shift), out.data_ptr(), G.st()))
        torch.cuda.synchronize()
        buf = (C.c_int * AV.plan_ints(AV.MAX_SEQ))()
        _lib.check(lib.sta_debug_last_attn_varlen_plan(h, buf))
        plan = AV.plan_dict(buf)
    finally:
        _lib.check(lib.sta_debug_set_option(h, 5, 0))
    o = out.cpu().numpy()
    guard = np.float32(1.05859375 * (1 if precision == "f16" else 2))          # hi (+ lo) of the byte pattern 0x3C3C
    touched = np.argwhere(o[rows:].view(np.uint32) != guard.view(np.uint32))
    assert len(touched) == 0, f"{case[0]}: {len(touched)} elements of the guard block behind the output changed, first (row, column) {touched[0]}"
    got, r0 = [], 0
    for n in nq:
        got.append(HP.attn_rows_to_tokens(o[r0:r0 + n + 1], "pose", 1, heads, n))
        r0 += n + 1
    assert plan["S"] == S and plan["orows"] == rows
    return got, [AV.seq_class(plan, i, nq[i]) for i in range(S)]


def claimed(case):
    return list(case[4])


def check_selection(precision, case, shift, pose_sel="self", seed=21, v_lo=False):
    """Every query selects one key with probability exactly 1: the output must EQUAL V[pi(query)].  V columns 0..2 = (sequence of the
    launch, head, key): a failure names what was expected and what came back."""
    heads, seqs = case[1], case[3]
    inputs, pis, margin = [], [], np.inf
    for s, (nq, nk) in enumerate(seqs):
        q, k, v, pi, mg = HP.attn_selection_inputs("pose", 1, heads, nq, nk, pose_sel, seed + s)
        v[..., 0] += s
        if v_lo:        # V = integer + lo (split_cases.attn_v_with_lo): both parts of the selected row must come back (f16: its hi)
            v = SC.attn_v_with_lo(v, seed + s)
            assert SC.split_holds(v)
        inputs.append((q, k, v)); pis.append(pi); margin = min(margin, mg)
    assert margin > 160, (case[0], margin)
    got, ran = varlen_launch(precision, case, shift, inputs)
    wrong, nan, first = 0, 0, []
    for s, (nq, nk) in enumerate(seqs):
        vw = inputs[s][2].astype(np.float16).astype(np.float32) if v_lo and precision == "f16" else inputs[s][2]
        want = np.take_along_axis(vw, pis[s][..., None], 2)
        bad = np.argwhere((got[s] != want).any(-1))
        wrong += len(bad); nan += int(np.isnan(got[s]).sum())
        for _z, h, t in bad[:4]:
            r = got[s][0, h, t]
            who = "pose query" if t == nq else f"query {t}"
            first.append(f"(sequence {s}, head {h}, {who}): expected key {pis[s][0, h, t]} (pose key = {nk}), "
                         f"got columns 0..2 = (sequence {r[0]:g}, head {r[1]:g}, key {r[2]:g}), {int((r != want[0, h, t]).sum())} of 64 columns differ")
    return {"class": ran, "margin": margin, "nan": nan, "wrong": wrong, "first": "; ".join(first[:8])}


def check_uniform(precision, case, shift, seed=22):
    """q = 0: the output is the column mean of V over exactly nk + 1 keys of the sequence."""
    heads, seqs = case[1], case[3]
    inputs = [HP.attn_uniform_inputs("pose", 1, heads, nq, nk, seed + s) for s, (nq, nk) in enumerate(seqs)]
    got, ran = varlen_launch(precision, case, shift, inputs)
    res = {"class": ran, "nan": 0, "max_abs": 0.0, "vmax": 0.0, "half_ulp16": 0.0}
    for s, (q, k, v) in enumerate(inputs):
        ref = np.broadcast_to(v.astype(np.float64).mean(2, keepdims=True), got[s].shape)
        err = np.abs(got[s] - ref)
        res["nan"] += int(np.isnan(got[s]).sum())
        res["max_abs"] = max(res["max_abs"], float(np.nanmax(err)) if not np.isnan(err).all() else float("nan"))
        res["vmax"] = max(res["vmax"], float(np.abs(v).max()))
        res["half_ulp16"] = max(res["half_ulp16"], float(2.0 ** (np.floor(np.log2(np.abs(ref).max())) - 11)))
    return res


def _inputs(case, kind, what, seed):
    heads, seqs = case[1], case[3]
    if kind == "ramp":
        return [HP.attn_ramp_inputs("pose", 1, heads, nq, nk, what, seed + s) for s, (nq, nk) in enumerate(seqs)]
    return [HP.attn_gaussian_inputs("pose", 1, heads, nq, nk, what, seed + s) for s, (nq, nk) in enumerate(seqs)]


def _rows(precision, case, shift, inputs):
    got, ran = varlen_launch(precision, case, shift, inputs)
    worst, num, den, nan = 0.0, 0.0, 0.0, 0
    for s, (q, k, v) in enumerate(inputs):
        ref = HP.attn_ref64(q, k, v, 0)
        rows, _ = HP.attn_row_errors(got[s], ref)
        nan += int(np.isnan(got[s]).sum())
        worst = max(worst, float(np.nanmax(rows)) if not np.isnan(rows).all() else float("nan"))
        num += float(((got[s].astype(np.float64) - ref) ** 2).sum()); den += float((ref ** 2).sum())
    return {"class": ran, "nan": nan, "worst_row": worst, "rel_l2": float(np.sqrt(num / max(den, 1e-300)))}


def check_ramp(precision, case, shift, pattern, seed=101):
    return _rows(precision, case, shift, _inputs(case, "ramp", pattern, seed))


def check_rows(precision, case, shift, sharp, seed=100):
    return _rows(precision, case, shift, _inputs(case, "gauss", sharp, seed))


@functools.lru_cache(maxsize=None)
def model_worst_row(kind, what, precision):
    """The numpy model of the documented arithmetic (helpers.attn_model) against the float64 reference on the SAME inputs the GPU
    checks use: its worst (sequence, query) row over every case of the group (kind "ramp": AV.RAMP_CASES under pattern `what`; kind
    "gauss": the cases whose sharpness is `what`).  The tests' row bounds are 4 x this figure - no constants of their own."""
    cases = [AV.case_by_id(c) for c in AV.RAMP_CASES] if kind == "ramp" else [c for c in AV.CASES if AV.sharp_of(c[0]) == what]
    worst = 0.0
    for case in cases:
        for q, k, v in _inputs(case, kind, what, 101 if kind == "ramp" else 100):
            rows, _ = HP.attn_row_errors(HP.attn_model(q, k, v, 0, precision), HP.attn_ref64(q, k, v, 0))
            worst = max(worst, float(rows.max()))
    return worst
