"""GPU: no product call depends on what its stream's scratch context held before it (the workspace contract above StreamCtx in
vista_slam_amd/csrc/sta_api.hip), and none writes behind the peak its dry pass planned.

Every row of tests/workspace_cases.py, in every precision it has, in deterministic mode: the call runs twice on the scratch as the
previous calls left it - the two results must be bit-identical, the first is the reference - and then once behind each fill of the
WHOLE scratch (workspace, split-K scratch, slab scratch, side lane's scratch: sta_debug_workspace_fill) with 0x00, 0xFF (NaN as fp16
and fp32, -1 as int32), 0x3C (1.06 per fp16 plane) and 0x7B (61280 as fp16, 1.3e36 as fp32: shows 0 * stale and stale addends that a
small value hides).  Every output must equal the reference bit for bit, and the bytes of the workspace behind the planned peak
(+ 4096, the slack plan_and_run asks for) must still hold the fill (sta_debug_workspace_tail).  The split-phase scheduler rows fill
before `begin` only; between the phases the fill hook must refuse.

Transitions: largest - smallest - largest call of a family on one handle and stream; the small call must equal the same call as the
FIRST call of a fresh handle (what the goldens measure).

Default mode (atomic split-K allowed): the 0xFF fill only.  A case whose two untouched runs are bit-identical must stay bit-identical;
a case whose runs differ launches an atomic split-K at this shape and must stay finite and within rel-L2 1e-4 of the deterministic
result (the bound test_deterministic_mode_is_bit_reproducible_at_slam_scale holds between the two modes).  The class is printed."""
import numpy as np
import pytest

import workspace_cases as WC
from helpers import first_difference, snapshot

pytestmark = pytest.mark.gpu

_handles = {}


def handle(precision):
    """One frontend on the test-hooks library per precision, kept for the module."""
    import torch
    from vista_slam_amd import _lib
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    if precision not in _handles:
        prec = WC.DEFAULT_PRECISION if precision == "DEFAULT" else precision
        _handles[precision] = STAFrontend(W.TINY, "cuda:0", precision=prec, lib=_lib.load_test()).load_procedural(seed=43)
    torch.cuda.synchronize()
    return _handles[precision]


@pytest.fixture(scope="module", autouse=True)
def _drop_handles():
    yield
    import torch
    _handles.clear()
    torch.cuda.empty_cache()


def fresh_handle(precision):
    from vista_slam_amd import _lib
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    prec = WC.DEFAULT_PRECISION if precision == "DEFAULT" else precision
    return STAFrontend(W.TINY, "cuda:0", precision=prec, lib=_lib.load_test()).load_procedural(seed=43)


def reset_switches(m):
    from vista_slam_amd import _lib
    m.set_deterministic(False)
    m.set_side_lanes("auto")
    m.set_varlen_heads(False)
    _lib.check(m.lib.sta_debug_set_option(m._h, 8, 0))
    m.lib.sta_regress_views_abort(m._h, m._stream())


def tail_bytes(G, m):
    info = G.workspace_info(m)
    return info["ws_cap"] - (info["plan_peak"] + 4096), info


def ensure_tail(G, m, case, x):
    """The tail guard needs room behind the planned peak: a workspace that this very call sized has 12.5 % + 1 MiB of slack, one that
    sta_reserve sized exactly has none - then a larger call first (it grows the workspace), and the case again for its own plan."""
    tail, info = tail_bytes(G, m)
    if tail < WC.MIN_TAIL:
        big = WC.by_name("forward_pair_lanes")
        big.run(m, big.make(m))
        case.run(m, x)
        tail, info = tail_bytes(G, m)
    assert tail >= WC.MIN_TAIL, f"{case.name}: {tail} bytes behind the planned peak ({info})"
    return tail, info


def refuses_between(G, m, case):
    """-> the `between` callable of a split-phase row: the fill hook must refuse while phase B is pending, with a message."""
    def between():
        assert G.workspace_info(m)["pending"] == 1, case.name
        rc = G.workspace_fill_rc(m, 0xFF)
        msg = m.lib.sta_last_error().decode()
        assert rc == -1 and "pending" in msg, f"{case.name}: sta_debug_workspace_fill between the two phases returned {rc} ({msg!r})"
    return between


@pytest.mark.parametrize("name,precision", WC.runs(), ids=lambda v: str(v))
def test_outputs_do_not_depend_on_the_scratch(name, precision):
    import gpu_checks as G
    case = WC.by_name(name)
    m = handle(precision)
    between = refuses_between(G, m, case) if name in WC.SPLIT_PHASE else None
    try:
        m.set_deterministic(True)
        x = case.make(m)
        ref = snapshot(case.run(m, x, between))
        again = snapshot(case.run(m, x, between))
        diff = first_difference(again, ref)
        assert diff is None, f"{name} {precision}: two runs on the untouched scratch differ in deterministic mode - {diff}"
        tail, info = ensure_tail(G, m, case, x)
        failures = []
        for byte in WC.FILLS:
            G.workspace_fill(m, byte)
            got = snapshot(case.run(m, x, between))
            diff = first_difference(got, ref)
            if diff is not None:
                failures.append(f"fill 0x{byte:02X}: {diff}")
            n_bad, first = G.workspace_tail(m, byte)
            if n_bad:
                now = G.workspace_info(m)
                failures.append(f"fill 0x{byte:02X}: {n_bad} bytes behind the planned peak changed, first at workspace offset {first} "
                                f"(planned peak {now['plan_peak']}, capacity {now['ws_cap']})")
        print(f"[workspace] {name} {precision} ({case.shapes}): planned peak {info['plan_peak']}, capacity {info['ws_cap']}, tail {tail} bytes, "
              f"side lane scratch {info['side_skbuf']}; {len(ref)} outputs; {'bit-identical under all four fills, tail untouched' if not failures else failures}")
        assert not failures, f"{name} {precision}: " + " | ".join(failures)
    finally:
        reset_switches(m)


def rel_l2_all(got, ref):
    """(largest rel-L2 over the outputs, all finite) of two output lists, in float64."""
    worst, finite = 0.0, True
    for (name, a), (_n, b) in zip(got, ref):
        a64, b64 = a.double().cpu().numpy(), b.double().cpu().numpy()
        finite &= bool(np.isfinite(a64).all())
        den = float(np.sqrt((b64 ** 2).sum()))
        with np.errstate(invalid="ignore", over="ignore"):
            num = float(np.sqrt(((a64 - b64) ** 2).sum()))
        worst = max(worst, num / den if den > 0 else num)
    return worst, finite


@pytest.mark.parametrize("name,precision", WC.runs(), ids=lambda v: str(v))
def test_default_mode_does_not_depend_on_the_scratch(name, precision):
    import gpu_checks as G
    case = WC.by_name(name)
    m = handle(precision)
    between = refuses_between(G, m, case) if name in WC.SPLIT_PHASE else None
    try:
        m.set_deterministic(True)
        x = case.make(m)
        det = snapshot(case.run(m, x, between))
        m.set_deterministic(False)
        one = snapshot(case.run(m, x, between))
        two = snapshot(case.run(m, x, between))
        repeatable = first_difference(two, one) is None
        G.workspace_fill(m, 0xFF)
        got = snapshot(case.run(m, x, between))
        n_bad, first = G.workspace_tail(m, 0xFF)
        assert [(n, t.shape, t.dtype) for n, t in got] == [(n, t.shape, t.dtype) for n, t in det], f"{name} {precision}: outputs changed shape"
        err, finite = rel_l2_all(got, det)
        print(f"[workspace] default mode {name} {precision}: class {'bit-repeatable' if repeatable else 'atomic split-K'}; filled run against the "
              f"deterministic result: rel-L2 {err:.3e}, finite {finite}; bytes changed behind the planned peak {n_bad}")
        assert n_bad == 0, f"{name} {precision}: {n_bad} bytes behind the planned peak changed, first at workspace offset {first}"
        if repeatable:
            diff = first_difference(got, one)
            assert diff is None, f"{name} {precision}: default mode, fill 0xFF - {diff}"
        else:
            assert finite and err <= 1e-4, f"{name} {precision}: default mode, fill 0xFF: rel-L2 {err:.3e} against the deterministic result (bound 1e-4), finite {finite}"
    finally:
        reset_switches(m)


@pytest.mark.parametrize("precision", WC.PRECISIONS)
@pytest.mark.parametrize("family", WC.TRANSITION_FAMILIES)
def test_small_call_after_a_large_one_equals_the_first_call_of_a_fresh_handle(family, precision):
    import torch
    big, small = WC.family_extremes(family)
    assert precision not in big.no_prec and precision not in small.no_prec
    m = handle(precision)
    fresh = None
    try:
        m.set_deterministic(True)
        xb, xs = big.make(m), small.make(m)
        first_big = snapshot(big.run(m, xb))
        got = snapshot(small.run(m, xs))
        last_big = snapshot(big.run(m, xb))
        fresh = fresh_handle(precision)
        fresh.set_deterministic(True)
        want = snapshot(small.run(fresh, xs))              # the FIRST call of this handle: nothing has been in its scratch
        diff = first_difference(got, want)
        print(f"[workspace] transition {family} {precision}: {big.name} -> {small.name} -> {big.name}; {len(got)} outputs of the small call "
              f"{'equal the fresh handle first call' if diff is None else diff}")
        assert diff is None, f"{family} {precision}: {small.name} behind {big.name} differs from the first call of a fresh handle - {diff}"
        diff = first_difference(last_big, first_big)
        assert diff is None, f"{family} {precision}: {big.name} behind {small.name} differs from itself before it - {diff}"
    finally:
        reset_switches(m)
        if fresh is not None:
            torch.cuda.synchronize()
            fresh.__del__()                                # sta_destroy now, not at some later collection


def test_hooks_refuse_without_a_context_and_see_every_tail_byte():
    """The hooks themselves: no context before the first call on a stream (-1 with a message, from all three); after a call the info
    is that call's plan; a tail that holds another byte than the one asked for is reported whole, from its first byte."""
    import ctypes as C
    import torch
    import gpu_checks as G
    m = fresh_handle("f16x3")
    try:
        n_bad, first, out = C.c_int64(0), C.c_int64(0), (C.c_int64 * 8)()
        for rc in (G.workspace_fill_rc(m, 0), m.lib.sta_debug_workspace_info(m._h, m._stream(), out),
                   m.lib.sta_debug_workspace_tail(m._h, m._stream(), 0, C.byref(n_bad), C.byref(first))):
            assert rc == -1 and "no scratch context" in m.lib.sta_last_error().decode(), (rc, m.lib.sta_last_error())
        assert G.workspace_fill_rc(m, 256) == -1
        case = WC.by_name("encode")
        case.run(m, case.make(m))
        info = G.workspace_info(m)
        assert info["plan_peak"] > 0 and info["ws_cap"] >= info["plan_peak"] + 4096 + WC.MIN_TAIL and info["pending"] == 0, info
        assert info["skbuf"] == info["slab"] == 16 << 20 and info["side_skbuf"] in (0, 16 << 20), info
        assert m.workspace_bytes() == info["ws_cap"]
        G.workspace_fill(m, 0x3C)
        assert G.workspace_tail(m, 0x3C) == (0, -1)
        lo = info["plan_peak"] + 4096
        assert G.workspace_tail(m, 0x7B) == (info["ws_cap"] - lo, lo)
    finally:
        torch.cuda.synchronize()
        m.__del__()
