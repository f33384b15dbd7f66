"""GPU: the keyframe scheduler on token subsets with the varlen DPT head (sta_set_varlen_heads; slam_scheduler.regress_views_tokens /
regress_views_tokens_finish with heads="varlen"): the window sides of ALL accepted edges go through one sta_head_pts_varlen pass that
writes straight into the scheduler's map layout.

On the three `rvt_*` fixtures, with the helpers and bars of tests/test_regress_tokens_gpu.py: decisions identical; maps, depths and K
within TOL = 1e-3 (rel-L2 and max norm) of the reference fixture; everything within ROUTE_TOL = 1e-4 of heads="entry"; ranges of
rejected edges unwritten; the begin / finish pair; a begin / abort leaves the switch usable; the keyword owns the switch for one call
and puts the handle's own setting back; a full-model call on a fresh handle with an edge rejected in front of accepted ones (the
begin-time plan has to hold the unfused tail).
"""
import ctypes as C

import numpy as np
import pytest

from test_decode_tokens_gpu import TOL, DEFAULT
from test_regress_tokens_gpu import TINY, FULL, CANARY, _setup, _inputs, _vs_fixture, _assert_bar, _err

pytestmark = pytest.mark.gpu

ROUTE_TOL = 1e-4


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    yield gpu_checks
    gpu_checks.drop_models()


def _route_errs(res, ref):
    """{name: error} of every map of every edge, route against route; decisions and the None pattern identical."""
    errs = {}
    assert len(res) == len(ref)
    for e, (a, b) in enumerate(zip(res, ref)):
        assert a.accepted == b.accepted and abs(a.rel_pose_conf - b.rel_pose_conf) < 1e-6
        errs[f"pose_e{e}"] = _err(a.pose.cpu().numpy(), b.pose.cpu().numpy())
        if not a.accepted:
            assert a.confs is None and a.pts3d is None
            continue
        assert (a.intri is None) == (b.intri is None)
        if a.intri is not None:
            errs[f"intri_e{e}"] = _err(a.intri.cpu().numpy(), b.intri.cpu().numpy())
        for t in range(2):
            assert (a.confs[t] is None) == (b.confs[t] is None)
            if a.confs[t] is None:
                continue
            assert a.confs[t].shape == b.confs[t].shape and a.pts3d[t].shape == b.pts3d[t].shape
            for key, x, y in (("confs", a.confs[t], b.confs[t]), ("depths", a.depths[t], b.depths[t]), ("pts", a.pts3d[t], b.pts3d[t])):
                errs[f"{key}_{t}_e{e}"] = _err(x.cpu().numpy(), y.cpu().numpy())
    return errs


def _check(G, case, prec):
    import torch
    from vista_slam_amd.slam_scheduler import regress_views_tokens, regress_views_tokens_begin, regress_views_tokens_finish
    g, meta, m = _setup(G, case, prec)
    a = _inputs(m, g, meta)
    m.range_report(reset=True)
    res = regress_views_tokens(m, *a, heads="varlen")
    torch.cuda.synchronize()
    _assert_bar(case, prec, "regress_views_tokens heads=varlen", _vs_fixture(res, g, meta))
    assert tuple(m.range_report(reset=True)) == (0, 0)
    ref = regress_views_tokens(m, *a)                     # the switch went back: this is the per-entry route
    with regress_views_tokens_begin(m, *a[:6], heads="varlen") as p:
        two = regress_views_tokens_finish(m, p, a[6], a[7])          # (None: what the begin was given)
    torch.cuda.synchronize()
    route = _route_errs(res, ref)
    worst = max(route, key=route.get)
    print(case, prec, "varlen vs entry: worst", worst, f"{route[worst]:.2e}")
    assert not {k: v for k, v in route.items() if not v < ROUTE_TOL}, route
    pair = _route_errs(two, res)
    assert not {k: v for k, v in pair.items() if not v < ROUTE_TOL}, pair
    return g, meta, m, a


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", TINY)
def test_varlen_heads_vs_reference_golden_and_entry_route(G, case, prec):
    _check(G, case, prec)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_varlen_heads_full_vs_reference_golden_and_entry_route(G, prec):
    _check(G, FULL, prec)
    G.drop_models()


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_every_edge_accepted(G, prec):
    """rvt_tiny_k4_edges with a threshold below every confidence: windows of several shapes, a same-shape pair (K) and index-list sides
    in one call - five window sides through one head pass, against the per-entry route."""
    import torch
    from vista_slam_amd.slam_scheduler import regress_views_tokens
    g, meta, m = _setup(G, "rvt_tiny_k4_edges", prec)
    a = list(_inputs(m, g, meta))
    a[7] = 0.0
    res = regress_views_tokens(m, *a, heads="varlen")
    ref = regress_views_tokens(m, *a, heads="entry")
    torch.cuda.synchronize()
    assert all(r.accepted for r in res)
    route = _route_errs(res, ref)
    worst = max(route, key=route.get)
    print("rvt_tiny_k4_edges", prec, "all accepted, varlen vs entry: worst", worst, f"{route[worst]:.2e}")
    assert not {k: v for k, v in route.items() if not v < ROUTE_TOL}, route


def test_rejected_ranges_stay_unwritten_and_abort_leaves_the_switch_usable(G):
    """The C entry on canary-filled buffers with the switch on: the ranges of a rejected edge stay canaries next to written ones, nothing
    behind the maps is touched.  Then a begin / abort with the switch on, and the handle serves both routes again."""
    import torch
    from vista_slam_amd import _lib
    from vista_slam_amd.slam_scheduler import _selection, _pack_side, regress_views_tokens, regress_views_tokens_begin
    g, meta, m = _setup(G, "rvt_tiny_k4_edges", "f16x3")
    feat_i, size_i, feats_j, sizes_j, sel_i, sel_j, adj, thres0 = _inputs(m, g, meta)
    k = len(feats_j)
    si = [_selection(s, size_i[0] // 16, size_i[1] // 16) for s in sel_i]
    sj = [_selection(s, sizes_j[e][0] // 16, sizes_j[e][1] // 16) for e, s in enumerate(sel_j)]
    win_i, cnt_i, idx_i = _pack_side(si, m.device)
    win_j, cnt_j, idx_j = _pack_side(sj, m.device)
    spans, pix = [], 0
    for e in range(k):
        n = sum(256 * w[2] * w[3] for w, ix in (si[e], sj[e]) if ix is None)
        spans.append((pix, n)); pix += n
    conf_g = [float(v) for v in g["conf"]]
    order = sorted(range(k), key=lambda e: conf_g[e])
    between = 0.5 * (conf_g[order[0]] + conf_g[order[1]])          # rejects exactly the edge of lowest confidence
    ptrs = (C.c_void_p * k)(*[f.data_ptr() for f in feats_j])
    Hj, Wj = (C.c_int * k)(*[s[0] for s in sizes_j]), (C.c_int * k)(*[s[1] for s in sizes_j])
    m.set_varlen_heads(True)
    try:
        for thres in (max(conf_g) + 0.01, between):
            pose = torch.empty(k, 4, 4, device="cuda")
            pts = torch.full((pix + 64, 3), CANARY, device="cuda")
            conf, depth = torch.full((pix + 64,), CANARY, device="cuda"), torch.full((pix + 64,), CANARY, device="cuda")
            K = torch.full((k, 3, 3), CANARY, device="cuda")
            pc, acc, kval, nacc = (C.c_float * k)(), (C.c_int * k)(), (C.c_int * k)(), C.c_int(-1)
            _lib.check(m.lib.sta_regress_views_tokens(m._h, feat_i.data_ptr(), size_i[0], size_i[1], ptrs, Hj, Wj, k, win_i, cnt_i, idx_i.data_ptr(),
                                                      win_j, cnt_j, idx_j.data_ptr(), bytes(bytearray(0 for _ in range(k))), thres, pose.data_ptr(),
                                                      pc, acc, C.byref(nacc), pts.data_ptr(), conf.data_ptr(), depth.data_ptr(), K.data_ptr(), kval, m._stream()))
            torch.cuda.synchronize()
            want = [not conf_g[e] < thres for e in range(k)]
            assert [bool(v) for v in acc] == want and nacc.value == sum(want), (thres, list(acc))
            for e, (p0, n) in enumerate(spans):
                for buf in (pts, conf, depth):
                    touched = bool((buf[p0:p0 + n] != CANARY).any()) if n else False
                    assert touched == (want[e] and n > 0), (thres, e)
                    if want[e] and n:
                        assert bool((buf[p0:p0 + n] != CANARY).all())
            assert all(bool((buf[pix:] == CANARY).all()) for buf in (pts, conf, depth))
        assert sum(want) == k - 1
        # begin / abort with the switch on
        p = regress_views_tokens_begin(m, feat_i, size_i, feats_j, sizes_j, sel_i, sel_j)
        p.close()
    finally:
        m.set_varlen_heads(False)
    a = (feat_i, size_i, feats_j, sizes_j, sel_i, sel_j, adj, thres0)
    res = regress_views_tokens(m, *a, heads="varlen")
    ref = regress_views_tokens(m, *a)
    torch.cuda.synchronize()
    assert [r.accepted for r in res] == [r.accepted for r in ref] == [bool(v) for v in g["accepted"]]
    with pytest.raises(ValueError, match="heads must be"):
        regress_views_tokens(m, *a, heads="both")
    assert m.lib.sta_set_varlen_heads(m._h, 2) == -1


def test_the_keyword_owns_the_switch_for_one_call_only(G):
    """The workspace is planned at begin time: a finish with heads="varlen" after a begin without it is refused with a message, and the
    stream serves the next call; a begin with it serves a finish of either kind.  A handle whose own setting is on keeps it across calls
    that name the other route, and heads=None follows it."""
    import torch
    from vista_slam_amd import _lib
    from vista_slam_amd.slam_scheduler import regress_views_tokens, regress_views_tokens_begin, regress_views_tokens_finish
    g, meta, m = _setup(G, "rvt_tiny_k3_win_sharp", "f16x3")
    a = _inputs(m, g, meta)
    ref = regress_views_tokens(m, *a, heads="entry")
    p = regress_views_tokens_begin(m, *a[:6])
    with pytest.raises(_lib.StaError, match="came after sta_regress_views_tokens_begin"):
        regress_views_tokens_finish(m, p, a[6], a[7], heads="varlen")
    with regress_views_tokens_begin(m, *a[:6], heads="varlen") as p:
        ent = regress_views_tokens_finish(m, p, a[6], a[7], heads="entry")
    torch.cuda.synchronize()
    assert not {k: v for k, v in _route_errs(ent, ref).items() if not v < ROUTE_TOL}          # the per-edge route, whatever was planned
    assert m.set_varlen_heads(True) is False
    try:
        via_handle = regress_views_tokens(m, *a)                     # None: the handle's setting
        regress_views_tokens(m, *a, heads="entry")
        assert m._varlen_heads is True                               # the keyword did not lose the caller's setting
        named = regress_views_tokens(m, *a, heads="varlen")
        torch.cuda.synchronize()
        assert not {k: v for k, v in _route_errs(via_handle, named).items() if not v < ROUTE_TOL}
    finally:
        assert m.set_varlen_heads(False) is True


@pytest.mark.parametrize("reject", [0, 1])
def test_full_model_fresh_handle_with_an_edge_rejected_in_front(G, reject):
    """Full model, a handle whose workspace no larger call has grown, k = 3 window edges of which one that is NOT the last is rejected:
    the accepted edges' outputs are then not packed (a gap, or a first offset above 0), the head runs its unfused tail, and the plan
    made at begin time - every edge accepted, packed outputs, fused tail - has to hold it.  Against the per-entry route; the rejected
    edge's range stays untouched."""
    import torch
    from vista_slam_amd.slam_scheduler import regress_views_tokens
    G.drop_models()
    m = G.model("full", 1.0, DEFAULT, seed=43)
    E = m.cfg.enc_embed_dim
    gen = torch.Generator().manual_seed(5)
    feats = [torch.randn(196, E, generator=gen).cuda() for _ in range(4)]
    size = (224, 224)
    sel_i = [(0, 0, 12, 14), (1, 0, 12, 14), (2, 0, 12, 14)]          # 168 patches a side: above the small-grid predicate, the plan fuses the tail
    sel_j = [(2, 0, 12, 14), (0, 0, 12, 14), (1, 0, 12, 14)]
    adjacent = [e != reject for e in range(3)]                        # a threshold above every confidence: only the adjacency exemption accepts
    args = (feats[0], size, feats[1:], [size] * 3, sel_i, sel_j, adjacent, 2.0)
    res = regress_views_tokens(m, *args, heads="varlen")             # the handle's FIRST call
    torch.cuda.synchronize()
    ref = regress_views_tokens(m, *args, heads="entry")
    torch.cuda.synchronize()
    assert [r.accepted for r in res] == adjacent == [r.accepted for r in ref]
    route = _route_errs(res, ref)
    worst = max(route, key=route.get)
    print("full model, edge", reject, "rejected, varlen vs entry: worst", worst, f"{route[worst]:.2e}")
    assert not {k: v for k, v in route.items() if not v < ROUTE_TOL}, route
    m.range_report(reset=True)
    G.drop_models()
