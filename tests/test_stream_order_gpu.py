"""GPU: every call is ordered by its stream alone, also while that stream and others have work pending ("Streams and concurrency" in
include/sta_mi355.h).  The method - one delayed call on a library-owned side stream, inputs that hold poison until the delay ends,
stale intermediates of a second input set in every scratch - and the matrix are in tests/stream_cases.py.  Deterministic mode, the
precisions DEFAULT and f16 (the two route structures).  Every row prints its delay, the host time of the call and its class:
"asynchronous" (the whole call was enqueued while its inputs held poison) or "waited" (allowed for the rows that name an entry of
stream_cases.SYNCS: there only the launches before the first wait are proven).

The hazard tests pend one call on s1 in the same way and then do what one of the four guards of the library exists for: a preprocess
frame of another source geometry (the handle-wide tables are uploaded again), a call with a larger position range (the RoPE table is
rebuilt), a larger call on the same stream (the workspace is re-allocated), a call on a ninth stream (the least recently used scratch
context changes hands).  Each asserts that the guard was passed (sta_alloc_stats counts the device synchronisations) and that the
pending call equals its reference bit for bit.  Crossed calls: A pending on s1, B on s2, for every row.

The harness proves itself on two rows made of torch alone: one launches on the default stream, one refreshes a module-level table with
a copy that is not ordered behind the pending stream.  Both must be reported."""
import time

import pytest

import stream_cases as SC
import workspace_cases as WC
from helpers import first_difference, snapshot

pytestmark = pytest.mark.gpu

_handles = {}
_refs = {}
_flip = [0]


def handle(precision):
    """One frontend on the test-hooks library per precision, kept for the module, with two of its pipeline streams: two that were
    measured to overlap with the null stream as well, so that a stray launch there does not sit behind the delay in one hardware queue."""
    import torch
    from vista_slam_amd import _lib
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    if precision not in _handles:
        prec = WC.DEFAULT_PRECISION if precision == "DEFAULT" else precision
        m = STAFrontend(W.TINY, "cuda:0", precision=prec, lib=_lib.load_test()).load_procedural(seed=43)
        _handles[precision] = (m, SC.side_streams(m, 2))
    torch.cuda.synchronize()
    return _handles[precision]


def fresh_handle(precision):
    from vista_slam_amd import _lib
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    prec = WC.DEFAULT_PRECISION if precision == "DEFAULT" else precision
    m = STAFrontend(W.TINY, "cuda:0", precision=prec, lib=_lib.load_test()).load_procedural(seed=43)
    m.set_deterministic(True)
    return m


def destroy(m):
    import torch
    torch.cuda.synchronize()
    m.__del__()                                # sta_destroy now, not at some later collection


@pytest.fixture(scope="module", autouse=True)
def _drop_handles():
    yield
    import torch
    torch.cuda.synchronize()
    _refs.clear()
    _handles.clear()
    torch.cuda.empty_cache()


def reset_switches(m):
    from vista_slam_amd import _lib
    m.set_deterministic(False)
    m.set_side_lanes("auto")
    m.set_varlen_heads(False)
    _lib.check(m.lib.sta_debug_set_option(m._h, 8, 0))
    for s in [None] + list(getattr(m, "_test_streams", ())):
        m.lib.sta_regress_views_abort(m._h, m._stream() if s is None else s.cuda_stream)


def refs(name, precision):
    """(A, B, ref_A, ref_B) of a row: computed once, shared by the row test and the crossed test, never changed (the harness restores
    the inputs it poisons)."""
    key = (name, precision)
    if key not in _refs:
        m, streams = handle(precision)
        _refs[key] = SC.references(SC.by_name(name), m, streams[0])
    return _refs[key]


def check_class(row, rep, what):
    allowed = SC.may_wait(row)
    if rep.waited and not allowed:
        pytest.fail(f"{what}: the call returned after the delay of {rep.delay_ms:.1f} ms had ended (host time of the same call on an idle stream {rep.host_ms:.2f} ms): either an "
                    f"entry documented as asynchronous waited for its stream, or the delay was too short")


@pytest.mark.parametrize("name,precision", SC.runs(), ids=lambda v: str(v))
def test_a_call_behind_pending_work_equals_its_reference(name, precision):
    row = SC.by_name(name)
    m, streams = handle(precision)
    m._test_streams = streams
    s = streams[_flip[0] % 2]
    _flip[0] += 1
    try:
        m.set_deterministic(True)
        xa, xb, ref_a, ref_b = refs(name, precision)
        rep = SC.delayed_call(row, m, s, xa, xb, ref_a, ref_b)
        print(f"[stream] {name} {precision} ({row.shapes}): {rep.line()}" + (f"; may wait: {SC.may_wait(row)}" if rep.waited else ""))
        check_class(row, rep, f"{name} {precision}")
        assert rep.diff is None, f"{name} {precision}: behind pending work on its stream the call differs from its reference - {rep.diff}"
    finally:
        reset_switches(m)


@pytest.mark.parametrize("name,precision", SC.runs(), ids=lambda v: str(v))
def test_crossed_calls_on_two_streams(name, precision):
    """A pending on s1 and B pending on s2, each behind its own delay with its inputs restored behind it."""
    import torch
    row = SC.by_name(name)
    m, (s1, s2) = handle(precision)
    m._test_streams = (s1, s2)
    try:
        m.set_deterministic(True)
        xa, xb, ref_a, ref_b = refs(name, precision)
        _, ha = SC.timed_run(row, m, s1, xa)                       # both contexts exist and hold these shapes
        _, hb = SC.timed_run(row, m, s2, xb)
        pa, pb = SC.poison_inputs(xa), SC.poison_inputs(xb)
        delay = SC.DELAY_FACTOR * max(ha + hb, 0.5)
        e1 = SC.pend(s1, pa, delay)
        e2 = SC.pend(s2, pb, delay)
        with torch.cuda.stream(s1):
            out_a = row.run(m, xa)
        with torch.cuda.stream(s2):
            out_b = row.run(m, xb)
        waited = e1.event.query() or e2.event.query()
        got_a, got_b = snapshot(out_a), snapshot(out_b)
        da, db = first_difference(got_a, ref_a), first_difference(got_b, ref_b)
        print(f"[stream] crossed {name} {precision}: host {ha:.2f} + {hb:.2f} ms, delay {delay:.1f} ms, class {'waited' if waited else 'asynchronous'}; "
              f"A {'bit-identical' if da is None else da}; B {'bit-identical' if db is None else db}")
        check_class(row, SC.Report(ha + hb, delay, waited, None), f"crossed {name} {precision}")
        assert da is None and db is None, f"crossed {name} {precision}: A on s1 - {da}; B on s2 - {db}"
    finally:
        reset_switches(m)


# ------------------------------------------------------------------------------------------ the four guards
def pend_row(row, m, s, xa, xb):
    """Warm the row on s with B (stale state), then poison A and pend the delay on s -> the pending record."""
    _, host_ms = SC.timed_run(row, m, s, xb)
    pairs = SC.poison_inputs(xa)
    return SC.pend(s, pairs, SC.DELAY_FACTOR * max(host_ms, 2.0))


def _rgb(Hs, Ws, seed, room=None):
    """a [Hs, Ws, 3] uint8 frame at the head of an allocation of `room` bytes"""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    buf = torch.zeros(max(room or 0, Hs * Ws * 3), dtype=torch.uint8, device="cuda")
    view = buf[:Hs * Ws * 3].view(Hs, Ws, 3)
    view.copy_(torch.from_numpy(rng.integers(0, 256, size=(Hs, Ws, 3), dtype=np.uint8)))
    return view


def preprocess_hazard(m, s1, s2, run):
    """Hazard form 1: frame A (100x140 -> 64x48) pending on s1, then a frame of another source geometry (120x160 -> 64x48) on s2, whose
    tables go into the same allocation.  run(m, frame) -> [(name, tensor)].  -> (first difference of A, of the second frame, the
    device synchronisations the second call made)."""
    import torch
    big = 120 * 160 * 3
    fa, fa2, fb = {"rgb": _rgb(100, 140, 7, big)}, {"rgb": _rgb(100, 140, 8, big)}, {"rgb": _rgb(120, 160, 9)}
    with torch.cuda.stream(s2):
        ref_b = snapshot(run(m, fb))                                # (the larger tables size the allocation)
    with torch.cuda.stream(s1):
        ref_a = snapshot(run(m, fa))
        ref_a2 = snapshot(run(m, fa2))
    assert first_difference(ref_a2, ref_a) is not None
    with torch.cuda.stream(s1):
        t0 = time.perf_counter()
        run(m, fa2)                                                 # A's geometry is the current one; stale state of another frame
        host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    pairs = SC.poison_inputs(fa)
    p = SC.pend(s1, pairs, SC.DELAY_FACTOR * max(host_ms, 2.0))
    with torch.cuda.stream(s1):
        out_a = run(m, fa)
    assert not p.event.query(), "the pending frame waited for its stream, or the delay was too short"
    syncs = m.alloc_stats()[1] if hasattr(m, "alloc_stats") else 0
    with torch.cuda.stream(s2):
        out_b = run(m, fb)
    syncs = (m.alloc_stats()[1] if hasattr(m, "alloc_stats") else 0) - syncs
    got_a, got_b = snapshot(out_a), snapshot(out_b)
    return first_difference(got_a, ref_a), first_difference(got_b, ref_b), syncs


def test_preprocess_tables_of_a_new_geometry_wait_for_pending_frames():
    """Checked once on a scratch build without the hipDeviceSynchronize of sta_preprocess_frame: the pending frame then reads the new
    geometry's tables at its own offsets - coefficient words as row bounds - and the run ends in HIP's 'an illegal memory access was
    encountered', not in a mere difference: a failure of this test for that reason is not to be repeated on a shared GPU."""
    row = SC.by_name("preprocess_frame")
    m, (s1, s2) = handle("DEFAULT")
    try:
        m.set_deterministic(True)
        da, db, syncs = preprocess_hazard(m, s1, s2, row.run)
        print(f"[stream] hazard 1, preprocess tables: device synchronisations of the second frame {syncs}; pending frame "
              f"{'bit-identical' if da is None else da}; second frame {'bit-identical' if db is None else db}")
        assert syncs >= 1, "the frame of another geometry did not pass the guard of sta_preprocess_frame"
        assert da is None, f"the frame pending on s1 while the tables were uploaded again - {da}"
        assert db is None, f"the frame of the new geometry on s2 - {db}"
    finally:
        reset_switches(m)


def _decode_pos(m, x, shift=0):
    """sta_decode_pos itself (the wrapper compares foreign positions with the grid on the host first), the first side's positions
    moved by `shift`"""
    return SC._run_decode_pos_abi(m, x, None, "p1_far" if shift else "p1", SC.DECODE_POS_MAX + shift)


ROPE_SHIFT = 40


@pytest.mark.parametrize("precision", SC.PRECISIONS)
def test_rope_table_growth_waits_for_pending_calls(precision):
    """A decode_pos call pending on s1 of a fresh handle (a small table), then one whose largest position exceeds the table on s2.
    (The table is freed before it is rebuilt, and hipFree waits for the device by itself: the runtime may hide a missing guard.)"""
    import torch
    case = WC.by_name("decode_pos")
    old, _ = handle(precision)
    old.set_deterministic(True)
    m = fresh_handle(precision)
    try:
        s1, s2 = m.pipeline_streams(2)

        def inputs(tag):
            x = case.make(old)                                      # (features from the module's handle: the same weights)
            if tag:
                x["fa"].mul_(1.125); x["fb"].mul_(1.125)
            assert int(max(x["p1"].max(), x["p2"].max())) <= SC.DECODE_POS_MAX
            x["p1_far"] = (x["p1"] + ROPE_SHIFT).contiguous()
            return x
        xa, xb = inputs(0), inputs(1)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):                                 # references from the module's handle: bit-identical across handles
            ref_a = snapshot(_decode_pos(old, xa))
            ref_far = snapshot(_decode_pos(old, xb, ROPE_SHIFT))
        run = lambda mm, x, between=None: _decode_pos(mm, x)
        with torch.cuda.stream(s2):
            _decode_pos(m, xb)                                      # s2's context and workspace exist: the guard left is the table's
        p = pend_row(SC.Row("decode_pos", (), None, run, ""), m, s1, xa, xb)
        with torch.cuda.stream(s1):
            out_a = _decode_pos(m, xa)
        assert not p.event.query(), "the pending call waited for its stream, or the delay was too short"
        syncs = m.alloc_stats()[1]
        with torch.cuda.stream(s2):
            out_far = _decode_pos(m, xb, ROPE_SHIFT)
        syncs = m.alloc_stats()[1] - syncs
        da, dfar = first_difference(snapshot(out_a), ref_a), first_difference(snapshot(out_far), ref_far)
        print(f"[stream] hazard 2, RoPE table growth {precision}: device synchronisations of the second call {syncs}; pending call "
              f"{'bit-identical' if da is None else da}; call with positions + {ROPE_SHIFT} {'bit-identical' if dfar is None else dfar}")
        assert syncs >= 1, "the call with larger positions did not pass the guard of ensure_rope"
        assert da is None, f"the call pending on s1 while the RoPE table was rebuilt - {da}"
        assert dfar is None, f"the call with the larger positions on s2 - {dfar}"
    finally:
        reset_switches(old)
        destroy(m)


@pytest.mark.parametrize("precision", SC.PRECISIONS)
def test_workspace_growth_waits_for_the_pending_call_on_the_same_stream(precision):
    """The smallest row of the forward_pair family pending on s1 of a fresh handle, then the largest row of the family on s1 as the
    first call of that shape.  (hipFree of the old workspace waits for the device by itself: the runtime may hide a missing guard.)"""
    import torch
    big, small = WC.family_extremes("pair")
    old, _ = handle(precision)
    old.set_deterministic(True)
    m = fresh_handle(precision)
    try:
        s1, _s2 = m.pipeline_streams(2)
        xa, xb, xbig = small.make(old), SC.default_b(small.make)(old), big.make(old)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            ref_a, ref_big = snapshot(small.run(old, xa)), snapshot(big.run(old, xbig))
        p = pend_row(small, m, s1, xa, xb)
        with torch.cuda.stream(s1):
            out_a = small.run(m, xa)
        assert not p.event.query(), "the pending call waited for its stream, or the delay was too short"
        before = m.workspace_bytes(), m.alloc_stats()[1]
        with torch.cuda.stream(s1):
            out_big = big.run(m, xbig)
        grown, syncs = m.workspace_bytes() - before[0], m.alloc_stats()[1] - before[1]
        da, dbig = first_difference(snapshot(out_a), ref_a), first_difference(snapshot(out_big), ref_big)
        print(f"[stream] hazard 3, workspace growth {precision}: {small.name} pending, then {big.name}: workspace + {grown} bytes, device "
              f"synchronisations {syncs}; pending call {'bit-identical' if da is None else da}; large call {'bit-identical' if dbig is None else dbig}")
        assert grown > 0 and syncs >= 1, "the large call did not re-allocate the stream's workspace"
        assert da is None, f"{small.name} pending on s1 while its workspace was re-allocated - {da}"
        assert dbig is None, f"{big.name} behind it - {dbig}"
    finally:
        reset_switches(old)
        destroy(m)


def context_hazard(m, ref_handle):
    """Hazard form 4 on a fresh handle `m`: calls on eight streams, each synchronised; a call pending on the first; calls on the other
    seven; then a call on a ninth stream, which takes over the least recently used context - the first stream's.  The first and the
    ninth are the library's pipeline streams, and the ninth waits for the event behind the delay: with the guard gone its call and
    the pending one would run at the same time on one scratch (a race: likely to show, not certain).
    -> (first difference of the pending call, of the ninth stream's call, device synchronisations of the ninth call, stream pointers)"""
    import torch
    row = SC.by_name("encode")
    xa, xb = row.make(ref_handle), SC.default_b(row.make)(ref_handle)
    torch.cuda.synchronize()
    ref_a, ref_b = snapshot(row.run(ref_handle, xa)), snapshot(row.run(ref_handle, xb))
    first, ninth = m.pipeline_streams(2)              # measured to overlap: these two do not share a hardware queue
    streams = [first] + [torch.cuda.Stream() for _ in range(7)] + [ninth]
    assert len(streams) <= SC.MAX_STREAMS
    for s in streams[:8]:
        with torch.cuda.stream(s):
            row.run(m, xb)
        s.synchronize()
    p = pend_row(row, m, streams[0], xa, xb)
    with torch.cuda.stream(streams[0]):
        out_a = row.run(m, xa)
    others = []
    for s in streams[1:8]:
        with torch.cuda.stream(s):
            others.append(row.run(m, xb))
    assert not p.event.query(), "the pending call waited for its stream, or the delay was too short"
    syncs = m.alloc_stats()[1]
    streams[8].wait_event(p.event)
    with torch.cuda.stream(streams[8]):
        out_9 = row.run(m, xb)
    syncs = m.alloc_stats()[1] - syncs
    got_a, got_9 = snapshot(out_a), snapshot(out_9)
    for o in others:
        d = first_difference(snapshot(o), ref_b)
        assert d is None, f"a call on one of the other seven streams - {d}"
    return first_difference(got_a, ref_a), first_difference(got_9, ref_b), syncs, {s.cuda_stream for s in streams}


@pytest.mark.parametrize("precision", SC.PRECISIONS)
def test_a_ninth_stream_takes_a_context_over_behind_its_pending_call(precision):
    """Checked once on a scratch build without the guard's line in stream_ctx (synchronisation and counter): the counter assertion
    failed, and the pending call differed from its reference in all 1536 elements at DEFAULT but stayed bit-identical at f16 - the
    value check is a race between two calls on one scratch, the counter check is what always fails."""
    old, _ = handle(precision)
    old.set_deterministic(True)
    m = fresh_handle(precision)
    try:
        da, d9, syncs, ptrs = context_hazard(m, old)
        print(f"[stream] hazard 4, context recycling {precision}: {len(ptrs)} streams, device synchronisations of the ninth stream's call {syncs}; "
              f"pending call {'bit-identical' if da is None else da}; ninth stream {'bit-identical' if d9 is None else d9}")
        assert len(ptrs) > 8, ptrs
        assert syncs >= 1, "the ninth stream did not take a context over"
        assert da is None, f"the call pending on the first stream while the ninth stream took its context over - {da}"
        assert d9 is None, f"the ninth stream's call - {d9}"
    finally:
        reset_switches(old)
        destroy(m)


# ------------------------------------------------------------------------------------------ the harness proves itself
class _Torch:
    """what the fake rows take for a frontend"""


def _mk_fake(seed):
    def make(m):
        import torch
        gen = torch.Generator(device="cuda").manual_seed(71 + seed)
        return {"x": torch.randn(1 << 16, device="cuda", generator=gen)}
    return make


def _run_wrong_stream(m, x, between=None):
    import torch
    with torch.cuda.stream(torch.cuda.default_stream()):          # the fault: not the caller's stream
        return [("y", x["x"] * 2)]


_TABLE = {}


def _run_table(m, frame, between=None):
    """A module-level device table per 'geometry' (the frame's first dimension), refreshed with a synchronous copy from host memory
    that is not ordered behind the caller's stream, then a launch on the caller's stream."""
    import torch
    n = frame["rgb"].shape[0]
    if _TABLE.get("key") != n:
        with torch.cuda.stream(torch.cuda.default_stream()):      # the fault: no wait for the frames that still read the old table
            if "tab" not in _TABLE:
                _TABLE["tab"] = torch.zeros(256, device="cuda")
            _TABLE["tab"].copy_(torch.arange(256, dtype=torch.float32) * n)
            torch.cuda.default_stream().synchronize()
        _TABLE["key"] = n
    return [("y", _TABLE["tab"][frame["rgb"].reshape(-1)[:4096].long()] + 1)]


def test_the_harness_reports_a_launch_on_the_wrong_stream():
    import torch
    row = SC.Row("wrong_stream", (), _mk_fake(0), _run_wrong_stream, "65536 floats", (), _mk_fake(1))
    m, (s1, _s2) = handle("DEFAULT")
    xa, xb, ref_a, ref_b = SC.references(row, _Torch(), s1)
    rep = SC.delayed_call(row, _Torch(), s1, xa, xb, ref_a, ref_b)
    torch.cuda.synchronize()
    print(f"[stream] fake row wrong_stream: {rep.line()}")
    assert not rep.waited and rep.diff is not None, \
        f"a launch on the default stream went unnoticed ({rep.line()}): the queue mapping of this machine hides stray launches"


def test_the_harness_reports_a_table_overwritten_under_a_pending_call():
    import torch
    m, (s1, s2) = handle("DEFAULT")
    _TABLE.clear()
    da, db, _ = preprocess_hazard(_Torch(), s1, s2, _run_table)
    torch.cuda.synchronize()
    print(f"[stream] fake row table_overwritten: pending call {'bit-identical' if da is None else da}; second call {'bit-identical' if db is None else db}")
    assert da is not None and db is None, \
        f"a table refreshed under a pending call went unnoticed (pending call: {da}; second call: {db}): the queue mapping of this machine hides it"
