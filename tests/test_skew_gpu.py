"""GPU: skewed-wave schedules.  Every other test here sees ONE interleaving of a workgroup's waves, the one the hardware picked in that
run; a missing or misplaced barrier between waves that share LDS (or global memory behind a barrier) passes such a test almost every
time.  This module runs cases that already exist, with the exact expectations they already have, on libsta_mi355_skew.so - the
test-hooks build whose kernels carry a skew point (csrc/sta_skew.h) behind every barrier, at kernel entry and in front of every
epilogue - and delays chosen waves at every point by far more than the kernel's longest barrier-to-barrier interval, so that a
delayed wave is certainly overtaken and a wave that runs ahead certainly meets data the others have not finished with.

Nothing is asserted here that is not asserted elsewhere: a case is a call of the existing test function (or check function) with
its frontend / check module on the skew library (gpu_checks.on_library).  What this module adds is the schedule and one assertion
of its own: the hit counter moved and the points that every wave of the kernel under test passes (MUST) were hit, i.e. the pattern
selected waves the kernel has and delayed them there (a pattern that selects none is a test bug).

Patterns over the NW waves of the kernel under test (4, 8, 12 or 16): each single wave slow; each single wave fast (all others slow);
even waves slow; odd waves slow; upper half slow; lower half slow.  Every (case, pattern) runs once; a test is one case under one
kind of pattern (the single slow waves of one half of the workgroup, the single fast ones, the four sets): at most 8 runs.

The delay: s_sleep 127 is 127 x 64 = 8128 clocks, 3.4 us at the 2.4 GHz peak clock and longer below it.  repeat_of gives, per group of
kernels, the number of such sleeps per point: ceil(4 x longest measured interval / 3.4 us), the intervals measured on the cases of
this file by tools/skew_intervals.py (profiles/r33_wave_skew.txt holds the table).

A skewed kernel has other registers and other code than the product's: this proves the SOURCE's synchronisation, not the product binary.
Kernels without a barrier have no skew point and are not here (bilinear_up2_kernel among them: its 1 x 1 case would count no hit).
"""
import pytest

import attention_cases as AC
import attention_mixed_cases as AM
import attention_varlen_cases as AV
import conv_cases as CC
import row_cases as RC
import split_cases as SC

pytestmark = pytest.mark.gpu

SLEEP_US = 8128 / 2400.0      # one s_sleep 127 at the peak clock: the shortest it can be
# group -> longest interval between two skew points of one wave in us, the largest over the group's cases and over the measuring
# runs (profiles/r33_wave_skew.txt); sleeps per point = ceil(4 x interval / SLEEP_US).  pgo: pgo_solve_kernel on the 1030-node graph
# (slam120, the largest system of tests/test_pgo_gpu.py that is solved to convergence there, is measured next to it).
INTERVAL_US = {
    "gemm": 101.76, "conv": 47.80, "halo": 7.12, "attention": 8.08, "rows": 33.64, "cloud": 124.00, "voxel": 51.40, "pgo": 113.36,
    "flow": 11.36, "orb": 5.56, "select": 2.08, "graph": 5.08,
}


def repeat_of(group):
    import math
    return max(1, math.ceil(4.0 * INTERVAL_US[group] / SLEEP_US))


def patterns(nw):
    """[(name, wave mask)] over a kernel of nw waves."""
    full, half = (1 << nw) - 1, nw // 2
    out = [(f"slow{w}", 1 << w) for w in range(nw)] + [(f"fast{w}", full ^ (1 << w)) for w in range(nw)]
    return out + [("even", 0x5555 & full), ("odd", 0xAAAA & full), ("upper", full ^ ((1 << half) - 1)), ("lower", (1 << half) - 1)]


class Ctx:
    """What a case may use: the check modules and one frontend on the skew library."""
    def __init__(self):
        import gpu_checks
        import gpu_checks_mixed
        import gpu_checks_varlen
        from vista_slam_amd import _lib
        from vista_slam_amd import weights as W
        from vista_slam_amd.sta_frontend import STAFrontend
        self.G, self.GM, self.GV = gpu_checks, gpu_checks_mixed, gpu_checks_varlen
        self.lib = _lib.load_skew()
        self.m = STAFrontend(W.TINY, "cuda:0", lib=self.lib).load_procedural(seed=43)


# ------------------------------------------------------------------------------------------ the cases: (id, waves, group, call)
def _gemm(prec, gid):
    kw = next(kw for p, kw in SC.gemm_cases() if SC.gemm_id(p, kw) == gid)

    def call(c):
        import test_split_exact_gpu as T
        T.test_gemm_is_bit_exact(c.G, prec, kw)
    return call


def _conv(cid, split=False):
    case = CC.case_by_id(cid)

    def call(c):
        import test_conv_exact as TC
        import test_split_exact_gpu as T
        (T.test_conv_is_bit_exact if split else TC.test_integer_sums_are_bit_exact)(c.G, "f16x3", case)
    return call


def _tail(hid):
    hcase = next(h for h in CC.HEAD_CASES if h[0] == hid)

    def call(c):
        import test_conv_exact as TC
        r = c.G.check_tail_exact("f16x3", hcase, 1)
        assert r["class"] == hcase[6] and r["nan"] == 0, r
        assert r["pts_ulp"] <= TC.PTS_ULPS and r["conf_ulp"] <= TC.CONF_ULPS, r
    return call


def _qkv_rows(**kw):
    def call(c):
        import test_split_exact_gpu as T
        T.test_qkv_decoder_rows_v_is_bit_exact(c.G, "f16x3", kw)
    return call


def _qkv_pair(c):
    r = c.G.check_qkv_pair("f16x3", ints=True)
    assert r["plan"]["family"] == 7, r["plan"]
    assert r["v_exact_bad"] == 0, f"{r['v_exact_bad']} wrong V elements; {r['v_first']}"
    assert r["v_a_pad_abs"] == 0.0 and r["v_b_pad_abs"] == 0.0, r


def _convt(row):
    prec, kw, fam = SC.convt_rows()[row]

    def call(c):
        import test_split_exact_gpu as T
        T.test_convt_is_bit_exact(c.G, prec, kw, fam)
    return call


def _gelu(c):
    from test_gpu_kernels import TOL
    r = c.G.check_gemm("f16x3", M=6200, N=768, K=64, variant=4, act=1, via_f16=1)
    assert r["plan"]["family"] == 5 and r["nan"] == 0 and r["rel_l2"] < TOL["f16x3"], r


def _attention(cid):
    case = AC.case_by_id(cid)

    def call(c):
        import test_split_exact_gpu as T
        T.test_attention_selection_returns_both_parts_of_v(c.G, "f16x3", case)
        T.test_attention_uniform_mean_includes_v_lo(c.G, "f16x3", case)
    return call


def _mixed(cid):
    case = AM.CASES[AM.IDS.index(cid)]

    def call(c):
        import test_split_exact_gpu as T
        T.test_mixed_attention_selection_returns_both_parts_of_v(c.GM, "f16x3", case)
    return call


def _varlen(cid):
    case = AV.CASES[AV.IDS.index(cid)]

    def call(c):
        import test_split_exact_gpu as T
        T.test_varlen_attention_selection_returns_both_parts_of_v(c.GV, "f16x3", AV.SHIFTS[0], case)
    return call


def _resid(c):
    import test_row_gpu as TR
    TR.test_resid_ln_exact_integers(c.G, "f16x3", next(x for x in RC.RESID_CASES if RC.case_id(x) == "196x768x768"))


def _pose(c):
    import test_post_gpu as TP
    TP.test_head_pose(c.G, 3, False)


def _cloud(c):
    import test_post_gpu as TP
    TP.test_world_pointcloud_exact(c.G, (2, 513, 512))          # 525312 pixels: 2052 blocks of cloud_count / cloud_emit over one cloud_scan


def _voxel(name):
    def call(c):
        import test_voxel_gpu as TV
        TV.test_case_against_the_restatement(c.m, name)
    return call


def _pgo_index(name):
    def call(c):
        import test_pgo_gpu as TG
        TG.test_index_equals_the_restatement(c.m, name)
    return call


def _pgo_solve(name):
    def call(c):
        import test_pgo_gpu as TG
        TG.test_solve_reaches_the_residual(c.m, name)
    return call


_SOLVE = {}
SOLVE_ITERS = 8
# x after SOLVE_ITERS PCG iterations against the float64 restatement's x after as many (pgo_cases.pcg), relative to 1 + max|row|: both run
# the same recurrence in float64 and differ in the order of their sums - block sums over at most 7 x 1030 terms (7e3 x 1.1e-16 = 8e-13
# on alpha and beta), carried through 8 iterations: 1e-9 leaves two to three orders of margin, and a p or d_e read before another
# thread wrote it is an error of order 1.  This holds where fixed nodes make the system definite: both graphs have some.  (With
# every node free the seven gauge directions are held by the damping alone, 1e-6 / radius, and an iterate carries the rounding of r
# divided by that: the all-free star40 of pgo_cases differs from the restatement by 4.7e-5 after 8 iterations with no wave delayed -
# so the star is solved here with leaf 0 fixed; the hub and its 40 edges are optimised.)
SOLVE_TOL = 1e-9


def _pgo_solve_capped(name):
    """sta_pgo_solve for SOLVE_ITERS iterations on a graph whose nodes and edges are spread over all 16 waves ("random 1030/2100":
    thread k owns node k and edge k, k + 1024 ...) or over one (star40, leaf 0 fixed), against the restatement stopped at the same
    iteration."""
    def call(c):
        import numpy as np
        import pgo_cases as P
        import test_pgo_gpu as TG
        if name not in _SOLVE:
            if name.startswith("random"):
                g, opt = TG._random(1030, 2100)
            else:
                g = P.get_graph(name)[0]
                opt = P.opt_mask(len(g["nodes"]), list(range(1, len(g["nodes"]))))
            lin = dict(P.linearize(g["nodes"], g["edges"], g["poses"], g["confs"], opt))
            _SOLVE[name] = (g, opt, lin) + P.pcg(lin, 1e4, rtol=1e-10, max_iter=SOLVE_ITERS)
        g, opt, lin, x_ref, st_ref = _SOLVE[name]
        d = TG.Dev(c.m, g, opt)
        d.index()
        d.linearize()
        x, stats = d.solve(1e4, 1e-10, SOLVE_ITERS)
        err = TG.rel(x, x_ref)
        print(f"[skew solve] {name}: iterations {stats[0]} (restatement {st_ref[0]}), status {int(stats[3])} ({st_ref[3]}), x against the restatement {err:.3e}")
        assert int(stats[0]) == st_ref[0] >= 1 and int(stats[3]) == st_ref[3], (stats, st_ref)
        assert err <= SOLVE_TOL, (err, SOLVE_TOL)
        assert not x[~opt].any()
        mdec = -2 * (x * lin["g"]).sum() - (x * P.hprod(lin, x)).sum()
        assert abs(stats[2] - mdec) <= 1e-9 * abs(mdec), (stats[2], mdec)
    return call


def _conv_varlen(cid):
    def call(c):
        import test_dpt_varlen_kernels as TD
        TD.test_conv_varlen_integer_sums_are_bit_exact_per_entry(c.G, "f16x3", next(x for x in TD.CONV_CASES if x[0] == cid))
    return call


def _tail_varlen(c):
    import test_dpt_varlen_kernels as TD
    TD.test_fused_tail_varlen_per_entry(c.G, "f16x3", 8)


def _corners(c):
    import test_flow_gpu as TF
    TF.test_corners_against_the_restatement(c.m, "across_1024")


def _orb(c):
    import test_loop_gpu as TL
    TL.test_orb_cut_with_ties_and_candidates_either_side_of_n(c.m)


def _select(name):
    def call(c):
        import test_select_gpu as TS
        TS.test_case_against_the_restatement(c.m, name)
    return call


def _graph(c):
    import test_graph_gpu as TGr
    TGr.test_commit_against_the_restatement(c.m, "k = 6", (48, 80))


CASES = [
    # ---- dense GEMM: every tile family, two-stage and ring loops, the row tail, K slices, plane / residual epilogues
    ("gemm_fam1_resid", 4, "gemm", _gemm("f16x3", "f16x3-M6145-N768-K64-v1-resid")),
    ("gemm_fam2_tail16", 16, "gemm", _gemm("f16x3", "f16x3-M6160-N768-K256-v2")),
    ("gemm_fam3_tail1", 12, "gemm", _gemm("f16x3", "f16x3-M6913-N768-K224-v3")),
    ("gemm_fam5_planes", 8, "gemm", _gemm("f16x3", "f16x3-M6900-N768-K64-v4-planes")),
    ("gemm_fam5_resid_tail16", 8, "gemm", _gemm("f16x3", "f16x3-M6928-N768-K192-v4-resid")),
    ("gemm_fam6_ring8_slices", 8, "gemm", _gemm("f16x3", "f16x3-M100-N256-K1024-v0")),
    ("gemm_fam6_ring4_planes", 4, "gemm", _gemm("f16x3", "f16x3-M513-N3328-K64-v0-planes")),
    ("gemm_fam6_ring8_resid", 8, "gemm", _gemm("f16x3", "f16x3-M513-N768-K128-v0-resid")),
    ("gemm_fam5_gelu", 8, "gemm", _gelu),
    ("qkv_fam5_tail4", 8, "gemm", _qkv_rows(hp=24, wp=32, S=4, K=64, Cdim=512, plan=(5, 4))),
    ("qkv_fam6", 8, "gemm", _qkv_rows(plan=(6, 0))),
    ("qkv_pair_fam7", 8, "gemm", _qkv_pair),
    ("convt_fam1", 4, "gemm", _convt(0)),
    ("convt_fam6_ring4", 4, "gemm", _convt(2)),
    ("resid_ln_slices", 4, "rows", _resid),
    # ---- implicit-GEMM convolutions (A_CONV3): the plane epilogue on every family, K slices + splitk_finish, the fused tail
    ("g5_plain_c64", 8, "conv", _conv("g5_plain_c64")),
    ("g5_relu_c96", 8, "conv", _conv("g5_relu_c96")),
    ("g5_r1_c32", 8, "conv", _conv("g5_r1_c32")),
    ("g5_r2_c64", 8, "conv", _conv("g5_r2_c64")),
    ("g2_plain_c32", 16, "conv", _conv("g2_plain_c32")),
    ("g3_plain_c96", 12, "conv", _conv("g3_plain_c96")),
    ("s6_sk_relu", 8, "conv", _conv("s6_sk_relu", split=True)),
    ("s6_four_waves", 4, "conv", _conv("s6_four_waves")),
    ("tail_fam5", 8, "conv", _tail("t5_w80")),
    # ---- the halo kernel (conv3h.h): several channel blocks (the halo is double buffered), ragged tiles, the fused tail
    ("h256_relu_w33", 16, "halo", _conv("h256_relu_w33")),
    ("h128_r1_c64", 16, "halo", _conv("h128_r1_c64")),
    ("tail_halo", 16, "halo", _tail("t8_w48")),
    ("h256_relu_varlen", 16, "halo", _conv_varlen("h256_relu")),
    ("tail_halo_varlen", 16, "halo", _tail_varlen),
    # ---- attention: double-buffered and 4-stage prefetch, pose modes 0 / 1 / 2, partly valid last tile; two-group and varlen forms
    ("att_n588", 4, "attention", _attention("n588")),
    ("att_q130_k1025", 4, "attention", _attention("q130_k1025")),
    ("att_n196", 4, "attention", _attention("n196")),
    ("att_n130", 4, "attention", _attention("n130")),
    ("att_pose640", 4, "attention", _attention("pose640")),
    ("att_pose128", 4, "attention", _attention("pose128")),
    ("att_pose588", 4, "attention", _attention("pose588")),
    ("att_pose196", 4, "attention", _attention("pose196")),
    ("att_mixed_pf", 4, "attention", _mixed("n196_140_self")),
    ("att_mixed_db", 4, "attention", _mixed("q255k260_q255k320")),
    ("att_varlen_pf", 4, "attention", _varlen("three")),
    ("att_varlen_db", 4, "attention", _varlen("db_opt5_b")),
    # ---- rows, scans, sorts and the one-workgroup kernels
    ("pose_final", 4, "rows", _pose),
    ("cloud_scan_2052_blocks", 16, "cloud", _cloud),
    ("voxel_m300000", 4, "voxel", _voxel("m300000")),
    ("voxel_long_rows", 16, "voxel", _voxel("long_row_threshold")),
    ("pgo_index_1030_2100", 16, "pgo", _pgo_index("random 1030/2100")),
    ("pgo_index_star40", 16, "pgo", _pgo_index("star40")),
    ("pgo_solve_1030_2100", 16, "pgo", _pgo_solve_capped("random 1030/2100")),
    ("pgo_solve_star40", 16, "pgo", _pgo_solve_capped("star40")),
    ("pgo_solve_triangle", 16, "pgo", _pgo_solve("triangle")),
    ("flow_corners_across_1024", 16, "flow", _corners),
    ("orb_tied_cut", 4, "orb", _orb),
    ("select_topk_ties", 4, "select", _select("topk_ties_per_entry_k")),
    ("select_grid_272x240", 4, "select", _select("grid_272x240_topk")),
    ("graph_commit_48x80", 4, "graph", _graph),
]

# The skew points EVERY wave of the kernel under test passes in a case (ids of csrc/*.h; a tuple = at least one of them): the run of every
# pattern must have hit them, so a pass says that the delayed waves were delayed in THAT kernel, at its entry, its barriers and
# its epilogue - not somewhere in a fill or a conversion next to it.  Read from the source: entry points and the barriers outside
# data-dependent branches.  Points no case reaches: 200 / 201 (head_epilogue: every EPI_HEAD kernel that exists has NT == 1 and runs
# head_epilogue_t), 212 / 213 (the ring's peel for 4 and 5 stages: family 6, the only ring, has 3).
_G1 = (104, 101, 102, 105)                         # gemm.h: gemm_kernel
_G2 = (208, 205, 206, 214)                         # gemm2.h, two stages: entry, first tile, K loop, epilogue
_G2T = _G2 + (215, 204)                            # ... with row-tail blocks (gemm2_tail)
_RING = (208, (209, 210, 211), 214)                # gemm2.h, ring: entry, a counted-wait barrier, epilogue
_HEAD_T = (202, 203)                               # head_epilogue_t
_ATT = (410, 406)                                  # attention.h: the output stage of every query block
_SOLVE_POINTS = (1114, 1116, 1107, 1108, 1109, 1111, 1112)
MUST = {
    "gemm_fam1_resid": _G1, "gemm_fam2_tail16": _G2T, "gemm_fam3_tail1": _G2T, "gemm_fam5_planes": _G2, "gemm_fam5_resid_tail16": _G2T,
    "gemm_fam6_ring8_slices": _RING, "gemm_fam6_ring4_planes": _RING + (207,), "gemm_fam6_ring8_resid": _RING, "gemm_fam5_gelu": _G2,
    "qkv_fam5_tail4": _G2T, "qkv_fam6": _RING, "qkv_pair_fam7": _G2, "convt_fam1": _G1, "convt_fam6_ring4": _RING,
    "resid_ln_slices": (510, 500, 501, 502),
    "g5_plain_c64": _G2, "g5_relu_c96": _G2, "g5_r1_c32": _G2, "g5_r2_c64": _G2, "g2_plain_c32": _G2, "g3_plain_c96": _G2,
    "s6_sk_relu": _RING, "s6_four_waves": _RING + (207,), "tail_fam5": _G2 + _HEAD_T,
    "h256_relu_w33": (304, 300, 301, 306), "h128_r1_c64": (304, 300, 301, 306), "tail_halo": (304, 300, 301, 306) + _HEAD_T,
    "h256_relu_varlen": (305, 302, 303, 307), "tail_halo_varlen": (305, 302, 303, 307) + _HEAD_T,
    "att_n588": (407,) + _ATT, "att_q130_k1025": (407,) + _ATT, "att_n196": (407,) + _ATT, "att_n130": (407,) + _ATT,
    "att_pose640": (407,) + _ATT, "att_pose128": (407,) + _ATT, "att_pose588": (407,) + _ATT, "att_pose196": (407,) + _ATT,
    "att_mixed_pf": (408,) + _ATT, "att_mixed_db": (408,) + _ATT, "att_varlen_pf": (409,) + _ATT, "att_varlen_db": (409,) + _ATT,
    "pose_final": (511, 503), "cloud_scan_2052_blocks": (515, 507, 508),
    "voxel_m300000": (716, 702, 703, 718, 706), "voxel_long_rows": (719, 712, 713),
    "pgo_index_1030_2100": (1113, 1100, 1101, 1102, 1105, 1106), "pgo_index_star40": (1113, 1100, 1101, 1102, 1105, 1106),
    "pgo_solve_1030_2100": _SOLVE_POINTS + (1110,), "pgo_solve_star40": _SOLVE_POINTS + (1110,), "pgo_solve_triangle": _SOLVE_POINTS + (1110,),
    "flow_corners_across_1024": (910, 904), "orb_tied_cut": (1010, 1000, 1012, 1003, 1004),
    "select_topk_ties": (609,), "select_grid_272x240": (609,), "graph_commit_48x80": (1201, 1200),
}
assert set(MUST) == {c[0] for c in CASES}


def missing_points(cid, seen):
    return [m for m in MUST[cid] if not (set(m) & seen if isinstance(m, tuple) else m in seen)]


# One test per (case, kind of pattern): "slow_lo" / "slow_hi" = each single wave of the lower / upper half slow, "fast_lo" / "fast_hi" = each
# of them fast, "sets" = even, odd, upper, lower.  (One test per pattern would be 1056 of them for the same 1056 runs; a failure names
# its pattern either way.)
KINDS = ("slow_lo", "slow_hi", "fast_lo", "fast_hi", "sets")


def patterns_of(nw, kind):
    pats = patterns(nw)
    if kind == "sets":
        return pats[2 * nw:]
    waves = range(nw // 2) if kind.endswith("lo") else range(nw // 2, nw)
    return [(n, m) for n, m in pats[:2 * nw] if n[:4] == kind[:4] and int(n[4:]) in waves]


ITEMS = [(cid, nw, group, call, kind) for cid, nw, group, call in CASES for kind in KINDS]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.G.drop_models()


def run_skewed(c, call, mask, repeat):
    """One run of `call` under the wave mask -> (skew points hit, largest interval of the measuring mode, the set of ids hit).  The
    configuration is cleared after the run and after a failed assertion of the call; after any other error (a device error among
    them) no further device call is made."""
    import ctypes as C
    from vista_slam_amd import _lib
    out = (C.c_ulonglong * 34)()

    def finish():
        _lib.check(c.lib.sta_debug_wave_skew_hits(out))
        _lib.check(c.lib.sta_debug_set_wave_skew(0, 0, 0, 0))
    _lib.check(c.lib.sta_debug_set_wave_skew(mask, 0xFFFFFFFF, 0xFFFFFFFF, repeat))
    try:
        with c.G.on_library(c.lib):
            call(c)
    except AssertionError:
        finish()
        raise
    finish()
    seen = {64 * w + b for w in range(32) for b in range(64) if (out[2 + w] >> b) & 1}
    return int(out[0]), int(out[1]), seen


@pytest.mark.parametrize("cid,nw,group,call,kind", ITEMS, ids=[f"{i[0]}-{i[4]}" for i in ITEMS])
def test_skewed_schedule(ctx, cid, nw, group, call, kind):
    pats = patterns_of(nw, kind)
    assert len(pats) == (4 if kind == "sets" else nw // 2)
    for pname, mask in pats:
        try:
            hits, _gap, seen = run_skewed(ctx, call, mask, repeat_of(group))
        except AssertionError as e:
            raise AssertionError(f"{cid} under pattern {pname} (wave mask {mask:#x}): {e}") from e
        assert hits > 0, f"{cid}: pattern {pname} (mask {mask:#x}) selected no wave of the launch: a test bug, not a pass"
        assert not missing_points(cid, seen), f"{cid}: pattern {pname} (mask {mask:#x}) did not reach the points {missing_points(cid, seen)} (hit: {sorted(seen)})"
