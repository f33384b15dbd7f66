"""GPU: the residual GEMM + LayerNorm pair (gemm_resid_ln through sta_debug_gemm_resid_ln: slab split-K residual GEMM +
resid_ln_kernel below the small-grid predicate, in-place GEMM + ln_kernel above it) and LayerNorm alone (sta_debug_layernorm,
sta_encoder_norm), per ROW against float64 references of the same values.  Cases and references: tests/row_cases.py (their
conditions are asserted on the CPU in tests/test_row_post_cpu.py).  Bars: the GEMM bar of test_gpu_kernels.TOL for x', fp32 class
(1e-5) for fp32 outputs and the f16x3 planes, TOL["f16"] for the f16 planes - the project's own."""
import ctypes as C

import numpy as np
import pytest
import torch

import row_cases as RC
from helpers import _split16, rel_l2
from test_gpu_kernels import TOL
from vista_slam_amd import _lib
from vista_slam_amd import weights as W

pytestmark = pytest.mark.gpu

PRECS = ["f16x3", "f16"]
PLANE_BAR = {"f16x3": 1e-5, "f16": TOL["f16"]}
PREC_ID = {"f16": 1, "f16x3": 3}
_cache = {}


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    return gpu_checks


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def resid_case(c, kind):
    """Inputs and the float64 x' of a case, computed once and shared (never modified)."""
    def make():
        A, Wt, b, x = RC.resid_inputs(c, kind)
        return A, Wt, b, x, RC.resid_ref64(A, Wt, b, x)
    return cached(("resid", RC.case_id(c), kind), make)


def host_plan(lib, c, prec):
    out = (C.c_int * 8)()
    _lib.check(lib.sta_debug_gemm_plan(0, RC.EPI_F32R, c["M"], c["N"], c["K"], PREC_ID[prec], 0, 0, 0, out))
    return dict(zip(("family", "bm", "bn", "m_tail", "tiles_m", "tiles_n", "ksplit", "slab_ks"), out))


def run_resid(G, prec, c, kind, sets):
    """-> x' [M,N], planes of set 1, planes of set 2 (numpy), the plan record of the launch, the affine sets."""
    m, lib, h = G.kernel_handle(prec)
    A, Wt, b, x, _ref = resid_case(c, kind)
    M, N, K = c["M"], c["N"], c["K"]
    aff = RC.affine_sets(N)
    Ad, Wd, bd, xd = G.dev(A), G.dev(Wt), G.dev(b), G.dev(x.copy())
    ad = [G.dev(a) for a in aff]
    o1 = torch.zeros(M, N, device=G.DEV); o2 = torch.zeros(M, N, device=G.DEV)
    p = [a.data_ptr() for a in ad]
    if sets == "add":
        p = [None] * 4
    elif sets == "one":
        p[2] = p[3] = None
    _lib.check(lib.sta_debug_gemm_resid_ln(h, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), xd.data_ptr(), M, N, K,
                                           p[0], p[1], p[2], p[3], RC.EPS, o1.data_ptr(), o2.data_ptr(), G.st()))
    torch.cuda.synchronize()
    plan = G.last_plan(lib, h)
    assert plan == host_plan(lib, c, prec), (plan, host_plan(lib, c, prec))       # the host-only plan entry describes the real launch
    return xd.cpu().numpy(), o1.cpu().numpy(), o2.cpu().numpy(), plan, aff


def check_planes(tag, got, x2, g, b, bar):
    ref = RC.layernorm64(x2, g, b)
    r, e = RC.worst(RC.row_rel_l2(got, ref))
    r2, e2 = RC.worst(RC.row_max_rel(got, ref))
    print(f"[resid_ln] {tag}: worst row rel-L2 {e:.3e} (row {r}), worst row max-rel {e2:.3e} (row {r2}), bar {bar:g}")
    assert e < bar and e2 < bar, (tag, r, e, r2, e2)


@pytest.mark.parametrize("sets", RC.RESID_SETS)
@pytest.mark.parametrize("c", RC.RESID_CASES, ids=RC.case_id)
@pytest.mark.parametrize("prec", PRECS)
def test_resid_ln(G, prec, c, sets):
    x2, o1, o2, plan, (g1, b1, g2, b2) = run_resid(G, prec, c, "gauss", sets)
    assert (plan["slab_ks"] > 1) == c["slab"], plan            # which kernel pair ran: from the launch plan record
    ref = resid_case(c, "gauss")[4]
    assert not np.isnan(x2).any()
    whole = rel_l2(x2, ref)
    r, e = RC.worst(RC.row_rel_l2(x2, ref))
    print(f"[resid_ln] {prec} {RC.case_id(c)} {sets} slab_ks {plan['slab_ks']}: x' rel-L2 {whole:.3e}, worst row {e:.3e} (row {r}), bar {TOL[prec]:g}")
    assert whole < TOL[prec] and e < TOL[prec], (whole, r, e)
    # each plane set against the float64 LayerNorm of the x' THE GPU RETURNED: GEMM error cannot mask LayerNorm error
    tag = f"{prec} {RC.case_id(c)} {sets}"
    if sets == "add":
        assert np.isnan(o1).all() and np.isnan(o2).all(), "add only: no plane may be written"
        return
    check_planes(tag + " set 1", o1, x2, g1, b1, PLANE_BAR[prec])
    if sets == "one":
        assert np.isnan(o2).all(), "one affine set: the second plane set must stay poisoned"
        return
    check_planes(tag + " set 2", o2, x2, g2, b2, PLANE_BAR[prec])
    sep = RC.set_separation(x2, g1, b1, g2, b2)
    assert sep.min() > 100 * PLANE_BAR[prec], sep.min()


@pytest.mark.parametrize("c", RC.RESID_CASES, ids=RC.case_id)
@pytest.mark.parametrize("prec", PRECS)
def test_resid_ln_exact_integers(G, prec, c):
    """Integer operands whose every partial sum fp16 holds: x' is the integer result bit for bit, whatever the slice count."""
    x2, o1, o2, plan, (g1, b1, g2, b2) = run_resid(G, prec, c, "int", "two")
    assert (plan["slab_ks"] > 1) == c["slab"], plan
    ref = resid_case(c, "int")[4].astype(np.float32)
    bad = np.argwhere(x2 != ref)
    assert len(bad) == 0, (plan, len(bad), bad[:4].tolist(), x2[tuple(bad[0])], ref[tuple(bad[0])])
    check_planes(f"{prec} {RC.case_id(c)} int set 1", o1, x2, g1, b1, PLANE_BAR[prec])
    check_planes(f"{prec} {RC.case_id(c)} int set 2", o2, x2, g2, b2, PLANE_BAR[prec])


def plane_value(y, prec):
    """What the fp16 planes carry for fp32 values y: hi + lo (f16x3) or the single fp16 rounding (f16)."""
    hi, lo = _split16(np.asarray(y, np.float32))
    return (hi + lo).astype(np.float32) if prec != "f16" else hi


@pytest.mark.parametrize("kind", RC.LN_KINDS)
@pytest.mark.parametrize("prec", PRECS)
def test_layernorm_rows(G, prec, kind):
    """sta_debug_layernorm (ln_kernel, one affine set, fp32 copy + planes) over M x C, every row on its own."""
    m, lib, h = G.kernel_handle(prec)
    worst32, worstp = (0.0, None), (0.0, None)
    for M in RC.LN_M:
        for Cd in RC.LN_C:
            x, g, b = RC.ln_inputs(M, Cd, kind)
            xd, gd, bd = G.dev(x), G.dev(g), G.dev(b)
            o32 = torch.zeros(M, Cd, device=G.DEV); op = torch.zeros(M, Cd, device=G.DEV)
            _lib.check(lib.sta_debug_layernorm(h, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), M, Cd, RC.EPS, o32.data_ptr(), op.data_ptr(), G.st()))
            torch.cuda.synchronize()
            o32, op = o32.cpu().numpy(), op.cpu().numpy()
            if kind == "constant":          # x - mean is exactly 0: the output IS the bias, and the planes its fp16 split
                assert np.array_equal(o32, np.broadcast_to(b, o32.shape)), (M, Cd, float(np.abs(o32 - b).max()))
                assert np.array_equal(op, np.broadcast_to(plane_value(b, prec), op.shape)), (M, Cd)
                continue
            ref = RC.layernorm64(x, g, b)
            e32 = max(RC.worst(RC.row_rel_l2(o32, ref))[1], RC.worst(RC.row_max_rel(o32, ref))[1])
            ep = max(RC.worst(RC.row_rel_l2(op, ref))[1], RC.worst(RC.row_max_rel(op, ref))[1])
            worst32 = max(worst32, (e32, (M, Cd))); worstp = max(worstp, (ep, (M, Cd)))
            assert e32 < 1e-5, (M, Cd, kind, e32)
            assert ep < PLANE_BAR[prec], (M, Cd, kind, ep)
    print(f"[layernorm] {prec} {kind}: worst row fp32 {worst32[0]:.3e} at (M, C) = {worst32[1]} (bar 1e-5), planes {worstp[0]:.3e} at {worstp[1]} (bar {PLANE_BAR[prec]:g})")


@pytest.mark.parametrize("kind", RC.LN_KINDS)
def test_encoder_norm_rows(G, kind):
    """sta_encoder_norm: the planes-less fp32 form of ln_kernel, at the model's width, with the model's own enc_norm."""
    m = G.model("tiny", precision="f16x3")
    sd = W.state_dict(W.TINY, seed=43)
    g, b = sd["enc_norm.weight"], sd["enc_norm.bias"]
    E = W.TINY.enc_embed_dim
    worst = 0.0
    for M in RC.LN_M:
        x, _g, _b = RC.ln_inputs(M, E, kind)
        xd = G.dev(x)
        out = torch.zeros(M, E, device=G.DEV)
        _lib.check(m.lib.sta_encoder_norm(m._h, xd.data_ptr(), M, out.data_ptr(), G.st()))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        if kind == "constant":
            assert np.array_equal(o, np.broadcast_to(b, o.shape)), (M, float(np.abs(o - b).max()))
            continue
        ref = RC.layernorm64(x, g, b, W.TINY.ln_eps)
        e = max(RC.worst(RC.row_rel_l2(o, ref))[1], RC.worst(RC.row_max_rel(o, ref))[1])
        worst = max(worst, e)
        assert e < 1e-5, (M, kind, e)
    print(f"[encoder_norm] {kind}: worst row {worst:.3e} (bar 1e-5)")
