"""GPU: the keyframe scheduler on token subsets (sta_regress_views_tokens[_begin/_finish] through slam_scheduler.regress_views_tokens)
against the reference fixtures `rvt_*` (tools/gen_golden_rvt.py: every edge is the reference's `regress_two_views` at B = 1 on the two
sliced sides), against the routes it replaces, its two new kernels alone, and the two-phase protocol.

Bounds: the project's bar TOL = 1e-3 for everything compared with a reference fixture, rel-L2 AND max norm, as
test_keyframe_scheduler_f2_vs_reference_golden; |conf - golden| < 1e-4; decisions identical (every fixture keeps its confidences 1e-2
away from its threshold: tests/test_regress_tokens_cpu.py).  The gather and the pose head's row-table form are compared bit for bit:
the first copies fp32 rows, the second runs the instructions of pose_layer_kernel on another source pointer.
What makes passing mean something: `alt_whole` of every fixture - ignoring the selection moves the pose by 1.4e-2 .. 0.85.
"""
import ctypes as C

import numpy as np
import pytest

from test_decode_tokens_gpu import TOL, DEFAULT

pytestmark = pytest.mark.gpu

TINY = ["rvt_tiny_k4_edges", "rvt_tiny_k3_win_sharp"]
FULL = "rvt_full_224_k3"
CANARY = -12345.0


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    yield gpu_checks
    gpu_checks.drop_models()


def _err(got, want):
    from helpers import rel_l2, max_rel
    return max(rel_l2(got, want), max_rel(got, want))


# ------------------------------------------------------------------------------------------ the gather alone
def _w(y0, x0, h, w):
    return ("win", (y0, x0, h, w))


def _i(a):
    return ("idx", np.asarray(a, np.int64))


_rs = np.random.default_rng(7)
# name -> (E, [(frame id, (hp, wp), selection)] over S sequences: the first half is side i, the second side j)
GATHER = {
    # counts 1, 63, 64, 65 by index on a 9 x 8 grid; the whole frame, the grid's last row and its last column as windows
    "counts_and_edges_E64": (64, [(0, (9, 8), _i([71])), (0, (9, 8), _i(_rs.permutation(72)[:63])), (0, (9, 8), _w(0, 0, 9, 8)), (0, (9, 8), _w(8, 0, 1, 8)),
                                  (1, (9, 8), _i(_rs.permutation(72)[:64])), (1, (9, 8), _i(_rs.permutation(72)[:65])), (1, (9, 8), _w(0, 7, 9, 1)), (1, (9, 8), _w(8, 7, 1, 1))]),
    # repeats, a descending list, out-of-grid values (clamped to the grid's first / last cell), frames of two sizes in one launch
    "order_clamp_two_frames_E1024": (1024, [(0, (3, 4), _i([5, 5, 0, 5, 11, 11])), (0, (3, 4), _i(np.arange(11, -1, -1))), (0, (3, 4), _i([12, -1, 3, 1 << 40, -(1 << 40)])),
                                            (1, (5, 2), _w(1, 0, 3, 2)), (1, (5, 2), _i([9, 0])), (2, (2, 7), _w(0, 3, 2, 4))]),
    "k1_E1024": (1024, [(0, (4, 4), _w(1, 1, 2, 3)), (1, (2, 3), _i([4, 2, 2]))]),
    # k = 16: thirty-two sequences, every second one by index, every side-j frame of its own size
    "k16_E64": (64, [(0, (6, 5), _w(s % 3, s % 2, 2 + s % 3, 3) if s % 2 else _i(_rs.integers(0, 30, size=1 + 5 * s))) for s in range(16)] +
                    [(1 + s, (2 + s % 4, 3 + s % 5), _i(_rs.integers(0, (2 + s % 4) * (3 + s % 5), size=1 + 3 * s)) if s % 2 else _w(0, 0, 2 + s % 4, 3 + s % 5)) for s in range(16)]),
}


@pytest.mark.parametrize("name", list(GATHER))
def test_gather_tokens_kernel_alone(G, name):
    """Features bit-identical to torch.index_select of the source frame, the positions table = the gathered grid positions, the guard
    rows behind both outputs untouched."""
    import torch
    from vista_slam_amd import _lib
    E, seqs = GATHER[name]
    S = len(seqs)
    m, lib, h = G.kernel_handle("f16x3")
    rs = np.random.default_rng(3)
    frames = {}
    for fid, (hp, wp), _sel in seqs:
        if fid not in frames:
            frames[fid] = G.dev(rs.standard_normal((hp * wp, E)).astype(np.float32))
    win, cnt, lists, want_f, want_p = [], [], [[], []], [], []
    for s, (fid, (hp, wp), (kind, v)) in enumerate(seqs):
        if kind == "win":
            y0, x0, wh, ww = v
            cells = (np.arange(y0, y0 + wh)[:, None] * wp + np.arange(x0, x0 + ww)[None, :]).ravel()
            win += [y0, x0, wh, ww]; cnt.append(0)
        else:
            cells = np.clip(v, 0, hp * wp - 1)
            win += [0, 0, 0, 0]; cnt.append(len(v))
            lists[s // (S // 2)].append(v)
        want_f.append(torch.index_select(frames[fid], 0, torch.from_numpy(cells).cuda()))
        want_p.append(np.stack([cells // wp, cells % wp], -1).astype(np.int32))
    want_f, want_p = torch.cat(want_f), np.concatenate(want_p)
    M, guard = want_f.shape[0], 3
    idx = [G.dev(np.concatenate(l)) if l else None for l in lists]
    feat = torch.full((M + guard, E), CANARY, device="cuda", dtype=torch.float32)
    pos = torch.full((M + guard, 2), -7, device="cuda", dtype=torch.int32)
    srcs = (C.c_void_p * S)(*[frames[fid].data_ptr() for fid, _g, _s in seqs])
    _lib.check(lib.sta_debug_gather_tokens(h, srcs, (C.c_int * S)(*[g[0] for _f, g, _s in seqs]), (C.c_int * S)(*[g[1] for _f, g, _s in seqs]),
                                           (C.c_int * (4 * S))(*win), (C.c_int * S)(*cnt), None if idx[0] is None else idx[0].data_ptr(),
                                           None if idx[1] is None else idx[1].data_ptr(), S, E, feat.data_ptr(), pos.data_ptr(), G.st()))
    torch.cuda.synchronize()
    assert torch.equal(feat[:M].view(torch.int32), want_f.view(torch.int32)), np.argwhere((feat[:M] != want_f).any(1).cpu().numpy())[:4]
    assert np.array_equal(pos[:M].cpu().numpy(), want_p), np.argwhere((pos[:M].cpu().numpy() != want_p).any(1))[:4]
    assert bool((feat[M:] == CANARY).all()) and bool((pos[M:] == -7).all())


def test_gather_tokens_refusals(G):
    from vista_slam_amd import _lib  # noqa: F401
    import torch
    m, lib, h = G.kernel_handle("f16x3")
    f = torch.zeros(12, 64, device="cuda")
    out, pos = torch.zeros(64, 64, device="cuda"), torch.zeros(64, 2, device="cuda", dtype=torch.int32)
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    srcs = (C.c_void_p * 2)(f.data_ptr(), f.data_ptr())
    grid = ((C.c_int * 2)(3, 3), (C.c_int * 2)(4, 4))

    def call(win, cnt, ix=idx.data_ptr(), s=srcs):
        return lib.sta_debug_gather_tokens(h, s, grid[0], grid[1], (C.c_int * 8)(*win), (C.c_int * 2)(*cnt), ix, ix, 2, 64, out.data_ptr(), pos.data_ptr(), G.st())
    assert call([0, 0, 3, 4, 0, 0, 1, 1], [0, 0]) == 0
    for win, cnt, kw in (([0, 0, 4, 4, 0, 0, 1, 1], [0, 0], {}),          # a window that leaves the 3 x 4 grid
                         ([0, 2, 1, 3, 0, 0, 1, 1], [0, 0], {}),
                         ([-1, 0, 1, 1, 0, 0, 1, 1], [0, 0], {}),
                         ([0, 0, 0, 0, 0, 0, 1, 1], [0, 0], {}),          # an index list without a token
                         ([0, 0, 0, 0, 0, 0, 1, 1], [2, 0], {"ix": None}),          # an index list without an index array
                         ([0, 0, 1, 1, 0, 0, 1, 1], [0, 0], {"s": (C.c_void_p * 2)(f.data_ptr() + 4, f.data_ptr())})):          # misaligned features
        assert call(win, cnt, **kw) == -1 and len(lib.sta_last_error()) > 0, (win, cnt)


# ------------------------------------------------------------------------------------------ the pose head on a row table
@pytest.mark.parametrize("k", [1, 5, 16])
def test_pose_rows_bit_identical_to_head_pose_on_a_stacked_copy(G, k):
    import torch
    from vista_slam_amd import _lib
    m, lib, h = G.kernel_handle("f16x3")
    D = m.cfg.dec_embed_dim
    rs = np.random.default_rng(k)
    rows = np.sort(rs.permutation(400)[:k]).astype(np.int64)[::-1].copy() if k == 5 else np.cumsum(rs.integers(1, 70, size=k)).astype(np.int64)
    tok = G.dev(rs.standard_normal((int(rows.max()) + 1, D)).astype(np.float32))
    pose, conf = torch.empty(k, 4, 4, device="cuda"), torch.empty(k, device="cuda")
    _lib.check(lib.sta_debug_pose_rows(h, tok.data_ptr(), D, (C.c_int64 * k)(*rows.tolist()), k, pose.data_ptr(), conf.data_ptr(), G.st()))
    ref = m.head_pose_s(tok[torch.from_numpy(rows).cuda()].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(pose.view(torch.int32), ref["pose"].view(torch.int32)) and torch.equal(conf.view(torch.int32), ref["conf"].view(torch.int32))
    assert lib.sta_debug_pose_rows(h, tok.data_ptr(), D, (C.c_int64 * 17)(), 17, pose.data_ptr(), conf.data_ptr(), G.st()) == -1
    assert lib.sta_debug_pose_rows(h, tok.data_ptr(), D, (C.c_int64 * 1)(-1), 1, pose.data_ptr(), conf.data_ptr(), G.st()) == -1


# ------------------------------------------------------------------------------------------ reference goldens
def _setup(G, case, prec):
    from helpers import load_golden
    g, meta = load_golden(case)
    full = case == FULL
    if full:
        G.drop_models()
    m = G.model("full" if full else "tiny", float(meta["qk_gain"]), prec, seed=int(meta["seed"]))
    return g, meta, m


def _inputs(m, g, meta):
    """(feat_i, size_i, feats_j, sizes_j, sel_i, sel_j, adjacent, thres): the fixture's cached encodings (tiny) or our encoder on the
    procedural frames (full: the fixture holds no features); index lists alternately on the CPU and on the device."""
    import torch
    from vista_slam_amd import weights as W
    k, seed = int(meta["k"]), int(meta["seed"])
    size_i = tuple(int(v) for v in g["hw_i"])
    sizes_j = [tuple(int(v) for v in g["hw_j"][e]) for e in range(k)]

    def frame(e, size, key):
        if key in g:
            return torch.from_numpy(g[key]).cuda()
        img = torch.from_numpy(W.synth_images(1, size[0], size[1], seed=seed, tag=e)).cuda()
        return m._encode_image(img, None, normalize=False)[0][0]

    def sel(tag, e):
        if f"idx_{tag}_e{e}" in g:
            t = torch.from_numpy(g[f"idx_{tag}_e{e}"])
            return t.cuda() if e % 2 else t
        w = tuple(int(v) for v in g[f"win_{tag}"][e])
        size = size_i if tag == "i" else sizes_j[e]
        return None if w == (0, 0, size[0] // 16, size[1] // 16) and e % 2 == 0 else w          # the whole frame both ways
    feat_i = frame(0, size_i, "feat_i")
    feats_j = [frame(1 + e, sizes_j[e], f"feat_j_e{e}") for e in range(k)]
    return (feat_i, size_i, feats_j, sizes_j, [sel("i", e) for e in range(k)], [sel("j", e) for e in range(k)],
            [bool(a) for a in g["adjacent"]], float(g["thres"]))


def _vs_fixture(res, g, meta):
    """{name: error} over every edge: decisions identical, None exactly where the fixture has none; the bars are asserted by the caller."""
    k, sub = int(meta["k"]), int(meta["sub"])
    errs = {}
    assert len(res) == k
    for e, r in enumerate(res):
        assert abs(r.rel_pose_conf - float(g["conf"][e])) < 1e-4, (e, r.rel_pose_conf, float(g["conf"][e]))
        assert r.accepted == bool(g["accepted"][e]), (e, r.rel_pose_conf, float(g["thres"]))
        errs[f"pose_e{e}"] = _err(r.pose.cpu().numpy(), g["pose"][e])
        if not r.accepted:
            assert r.confs is None and r.intri is None and r.depths is None and r.pts3d is None
            continue
        assert (r.intri is not None) == (f"intri_e{e}" in g), e
        if r.intri is not None:
            errs[f"intri_e{e}"] = _err(r.intri.cpu().numpy(), g[f"intri_e{e}"])
            assert tuple(r.confs.shape[:1]) == (2,)
        for t, tag in enumerate("ij"):
            has = f"confs_{tag}_e{e}" in g
            assert (r.confs[t] is not None) == has == (r.depths[t] is not None) == (r.pts3d[t] is not None), (e, tag)
            if not has:
                continue
            for key, got in (("confs", r.confs[t]), ("depths", r.depths[t])):
                got = got.cpu().numpy()
                errs[f"{key}_{tag}_e{e}"] = _err(got[::sub, ::sub], g[f"{key}_{tag}_e{e}"])
                errs[f"{key}_l2_{tag}_e{e}"] = abs(np.sqrt((got.astype(np.float64) ** 2).sum()) / float(g[f"{key}_l2_{tag}_e{e}"]) - 1)
            assert np.array_equal(r.pts3d[t][..., 2].cpu().numpy(), r.depths[t].cpu().numpy())
    return errs


def _assert_bar(case, prec, route, errs):
    worst = max(errs, key=errs.get)
    print(case, prec, route, "worst", worst, f"{errs[worst]:.2e}", {k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", TINY)
def test_regress_views_tokens_vs_reference_golden(G, case, prec):
    import torch
    g, meta, m = _setup(G, case, prec)
    from vista_slam_amd.slam_scheduler import regress_views_tokens
    m.range_report(reset=True)
    res = regress_views_tokens(m, *_inputs(m, g, meta))
    torch.cuda.synchronize()
    _assert_bar(case, prec, "regress_views_tokens", _vs_fixture(res, g, meta))
    assert tuple(m.range_report(reset=True)) == (0, 0)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_regress_views_tokens_full_vs_reference_golden(G, prec):
    """Full architecture at 224 x 224: whole / whole (adjacent), an 8 x 10 window against the whole frame, 140 of 196 tokens against
    the whole frame.  The encodings are our encoder's, so its error is inside the figures."""
    import torch
    from vista_slam_amd.slam_scheduler import regress_views_tokens
    g, meta, m = _setup(G, FULL, prec)
    res = regress_views_tokens(m, *_inputs(m, g, meta))
    torch.cuda.synchronize()
    _assert_bar(FULL, prec, "regress_views_tokens", _vs_fixture(res, g, meta))
    G.drop_models()


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", TINY)
def test_split_route_vs_reference_golden(G, case, prec):
    """The k per-edge B = 1 sequences the call replaces (keyframe_pipeline.regress_two_views_tokens_split), held to the same goldens
    at the same bar."""
    import torch
    from vista_slam_amd.keyframe_pipeline import regress_two_views_tokens_split
    g, meta, m = _setup(G, case, prec)
    feat_i, size_i, feats_j, sizes_j, sel_i, sel_j, adjacent, thres = _inputs(m, g, meta)
    res = [regress_two_views_tokens_split(m, feat_i, size_i, feats_j[e], sizes_j[e], sel_i[e], sel_j[e], adjacent[e], thres) for e in range(len(feats_j))]
    torch.cuda.synchronize()
    _assert_bar(case, prec, "split", _vs_fixture(res, g, meta))


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_every_edge_accepted_against_the_split_route(G, prec):
    """rvt_tiny_k4_edges with a threshold below every confidence: the fixture's own threshold rejects edges 1 and 2, so here their maps -
    a window against a whole frame of another size (two shapes: two head calls, no K) and an index list against a window - are held
    to the per-edge B = 1 sequences at the same bar."""
    import torch
    from vista_slam_amd.keyframe_pipeline import regress_two_views_tokens_split
    from vista_slam_amd.slam_scheduler import regress_views_tokens
    g, meta, m = _setup(G, "rvt_tiny_k4_edges", prec)
    feat_i, size_i, feats_j, sizes_j, sel_i, sel_j, adjacent, _thres = _inputs(m, g, meta)
    res = regress_views_tokens(m, feat_i, size_i, feats_j, sizes_j, sel_i, sel_j, adjacent, 0.0)
    errs = {}
    for e, r in enumerate(res):
        s = regress_two_views_tokens_split(m, feat_i, size_i, feats_j[e], sizes_j[e], sel_i[e], sel_j[e], adjacent[e], 0.0)
        assert r.accepted and s.accepted and abs(r.rel_pose_conf - s.rel_pose_conf) < 1e-4
        errs[f"pose_e{e}"] = _err(r.pose.cpu().numpy(), s.pose.cpu().numpy())
        assert (r.intri is None) == (s.intri is None) == (e != 0)
        if e == 0:
            errs["intri_e0"] = _err(r.intri.cpu().numpy(), s.intri.cpu().numpy())
        for t in range(2):
            assert (r.confs[t] is None) == (s.confs[t] is None) == [[False, False], [False, False], [True, False], [True, True]][e][t]
            if r.confs[t] is not None:
                assert r.confs[t].shape == s.confs[t].shape
                errs[f"confs_{t}_e{e}"] = _err(r.confs[t].cpu().numpy(), s.confs[t].cpu().numpy())
                errs[f"depths_{t}_e{e}"] = _err(r.depths[t].cpu().numpy(), s.depths[t].cpu().numpy())
                errs[f"pts_{t}_e{e}"] = _err(r.pts3d[t].cpu().numpy(), s.pts3d[t].cpu().numpy())
    torch.cuda.synchronize()
    _assert_bar("rvt_tiny_k4_edges", prec, "all accepted vs split", errs)


@pytest.mark.parametrize("name", ["f2_tiny_48x64", "f2_tiny_80x48_portrait"])
@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_whole_frame_selections_vs_f2_golden(G, name, prec):
    """With the whole frame selected on every edge and equal frame sizes the call answers what regress_views answers: the f2 goldens
    at TOL, the same decisions, and for the portrait frames the transposed views and the K the reference derives from them."""
    import torch
    from helpers import load_golden, rel_l2, max_rel
    from vista_slam_amd import weights as W
    from vista_slam_amd.slam_scheduler import regress_views_tokens
    g, meta = load_golden(name)
    H, Wd, nview, sub = int(meta["H"]), int(meta["W"]), int(meta["nview"]), int(meta["sub"])
    m = G.model("tiny", 1.0, prec)
    imgs = torch.from_numpy(W.synth_images(nview, H, Wd, seed=int(meta["seed"]), tag=int(meta["tag"]))).cuda()
    feats = [m._encode_image(imgs[v:v + 1], None, normalize=False)[0] for v in range(nview)]
    i = nview - 1
    js = list(range(i))
    thres = float(g["thres"])
    whole = (0, 0, H // 16, Wd // 16)
    res = regress_views_tokens(m, feats[i], (H, Wd), [feats[j] for j in js], [(H, Wd)] * i, [None if j % 2 else whole for j in js], [None] * i,
                               [i - j == 1 for j in js], thres)
    torch.cuda.synchronize()
    acc = g["accepted"]
    for j, r in zip(js, res):
        assert abs(r.rel_pose_conf - float(g[f"conf_{j}"])) < 1e-4, (j, r.rel_pose_conf, float(g[f"conf_{j}"]))
        assert rel_l2(r.pose.cpu().numpy(), g[f"pose_{j}"]) < TOL
        assert r.accepted == bool(acc[j]), (j, r.rel_pose_conf, thres)
        if not r.accepted:
            assert r.confs is None and r.intri is None and r.depths is None
            continue
        confs, depths = r.confs.cpu().numpy(), r.depths.cpu().numpy()
        assert confs.shape == ((2, Wd, H) if H > Wd else (2, H, Wd))          # portrait: the transposed views
        assert rel_l2(confs[:, ::sub, ::sub], g[f"confs_{j}"]) < TOL and max_rel(confs[:, ::sub, ::sub], g[f"confs_{j}"]) < TOL
        assert rel_l2(depths[:, ::sub, ::sub], g[f"depths_{j}"]) < TOL and max_rel(depths[:, ::sub, ::sub], g[f"depths_{j}"]) < TOL
        assert abs(np.sqrt((confs.astype(np.float64) ** 2).sum()) / float(g[f"confs_l2_{j}"]) - 1) < TOL
        assert abs(np.sqrt((depths.astype(np.float64) ** 2).sum()) / float(g[f"depths_l2_{j}"]) - 1) < TOL
        assert max_rel(r.intri.cpu().numpy(), g[f"intri_{j}"]) < TOL
    assert res[-1].accepted and float(g[f"conf_{i - 1}"]) < thres      # accepted only through the adjacency exemption


# ------------------------------------------------------------------------------------------ the two-phase protocol
def _same(a, b):
    import torch
    assert a.accepted == b.accepted and a.rel_pose_conf == b.rel_pose_conf and torch.equal(a.pose, b.pose)
    if not a.accepted:
        return
    assert (a.intri is None) == (b.intri is None) and (a.intri is None or torch.equal(a.intri, b.intri))
    for t in range(2):
        assert (a.confs[t] is None) == (b.confs[t] is None)
        if a.confs[t] is not None:
            assert torch.equal(a.confs[t], b.confs[t]) and torch.equal(a.depths[t], b.depths[t]) and torch.equal(a.pts3d[t], b.pts3d[t])


def test_begin_finish_on_two_streams_equal_the_one_shot_calls(G):
    """Two keyframes in flight at once, each on its own stream, begun before either is finished: the results are those of the one-shot
    calls, bit for bit (deterministic summation orders)."""
    import torch
    from vista_slam_amd.slam_scheduler import regress_views_tokens, regress_views_tokens_begin, regress_views_tokens_finish
    cases = [_setup(G, c, "f16x3") for c in TINY]
    m = cases[0][2]
    args = []
    for g, meta, _m in cases:          # both fixtures on the weights of the first: only the routes are compared here
        args.append(_inputs(m, g, meta))
    m.set_deterministic(True)
    try:
        ref = [regress_views_tokens(m, *a) for a in args]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pend = []
        for s, a in zip(streams, args):
            with torch.cuda.stream(s):
                pend.append(regress_views_tokens_begin(m, *a[:6]))
        out = []
        for s, p, a in zip(streams, pend, args):
            with torch.cuda.stream(s), p:
                out.append(regress_views_tokens_finish(m, p, a[6], a[7]))
        torch.cuda.synchronize()
    finally:
        m.set_deterministic(False)
    for got, want in zip(out, ref):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            _same(a, b)


def test_rejected_ranges_and_index_sides_stay_untouched(G):
    """The C entry on canary-filled buffers.  (a) a threshold above every confidence, no adjacent edge: n_accepted == 0, nothing is
    written.  (b) the fixture's own decisions with edge 1 made non-viable by a threshold between: the ranges of a rejected edge stay
    canaries next to written ones, and the buffers hold nothing for index-list sides (their size is the window sides' alone)."""
    import torch
    from vista_slam_amd import _lib
    from vista_slam_amd.slam_scheduler import _selection, _pack_side
    g, meta, m = _setup(G, "rvt_tiny_k4_edges", "f16x3")
    feat_i, size_i, feats_j, sizes_j, sel_i, sel_j, _adj, _thres = _inputs(m, g, meta)
    k = len(feats_j)
    si = [_selection(s, size_i[0] // 16, size_i[1] // 16) for s in sel_i]
    sj = [_selection(s, sizes_j[e][0] // 16, sizes_j[e][1] // 16) for e, s in enumerate(sel_j)]
    win_i, cnt_i, idx_i = _pack_side(si, m.device)
    win_j, cnt_j, idx_j = _pack_side(sj, m.device)
    spans = []          # per edge: (first pixel, pixels) of its window sides in the map buffers
    pix = 0
    for e in range(k):
        n = sum(256 * w[2] * w[3] for w, ix in (si[e], sj[e]) if ix is None)
        spans.append((pix, n)); pix += n
    assert pix == 256 * (30 + 30 + 6 + 12 + 16)          # index-list sides occupy nothing
    conf_g = [float(v) for v in g["conf"]]
    ptrs = (C.c_void_p * k)(*[f.data_ptr() for f in feats_j])
    Hj, Wj = (C.c_int * k)(*[s[0] for s in sizes_j]), (C.c_int * k)(*[s[1] for s in sizes_j])
    order = sorted(range(k), key=lambda e: conf_g[e])
    between = 0.5 * (conf_g[order[0]] + conf_g[order[1]])          # rejects exactly the edge of lowest confidence
    for thres, adjacent in ((max(conf_g) + 0.01, [False] * k), (between, [False] * k)):
        pose = torch.empty(k, 4, 4, device="cuda")
        pts = torch.full((pix + 64, 3), CANARY, device="cuda")
        conf, depth = torch.full((pix + 64,), CANARY, device="cuda"), torch.full((pix + 64,), CANARY, device="cuda")
        K = torch.full((k, 3, 3), CANARY, device="cuda")
        pc, acc, kval, nacc = (C.c_float * k)(), (C.c_int * k)(), (C.c_int * k)(), C.c_int(-1)
        _lib.check(m.lib.sta_regress_views_tokens(m._h, feat_i.data_ptr(), size_i[0], size_i[1], ptrs, Hj, Wj, k, win_i, cnt_i, idx_i.data_ptr(),
                                                  win_j, cnt_j, idx_j.data_ptr(), bytes(bytearray(int(a) for a in adjacent)), thres, pose.data_ptr(),
                                                  pc, acc, C.byref(nacc), pts.data_ptr(), conf.data_ptr(), depth.data_ptr(), K.data_ptr(), kval, m._stream()))
        torch.cuda.synchronize()
        want = [not conf_g[e] < thres for e in range(k)]
        assert [bool(a) for a in acc] == want and nacc.value == sum(want), (thres, list(acc))
        assert list(kval) == [1 if want[0] and e == 0 else 0 for e in range(k)]          # only edge 0 has two windows of one shape
        assert bool((K[1:] == CANARY).all()) and bool((K[0] == CANARY).all()) != want[0]
        for e, (p0, n) in enumerate(spans):
            for buf in (pts, conf, depth):
                touched = bool((buf[p0:p0 + n] != CANARY).any()) if n else False
                assert touched == (want[e] and n > 0), (thres, e)
                if want[e] and n:
                    assert bool((buf[p0:p0 + n] != CANARY).all())
        assert all(bool((buf[pix:] == CANARY).all()) for buf in (pts, conf, depth))
    assert sum(want) == k - 1          # the second pass rejected one edge next to written ones


def test_protocol_refusals_and_recovery(G):
    """finish without begin; a begin of either kind while the other kind is pending; a finish of the wrong kind (the call stays
    pending); abort, then the stream serves both kinds again.  Every refusal is a host-side check."""
    import torch
    from vista_slam_amd import _lib
    from vista_slam_amd.slam_scheduler import (regress_views_begin, regress_views_finish, regress_views_tokens_begin,
                                               regress_views_tokens_finish, regress_views_tokens)
    g, meta, m = _setup(G, "rvt_tiny_k3_win_sharp", "f16x3")
    a = _inputs(m, g, meta)
    k = len(a[2])
    H, Wd = a[1]
    whole_j = [f for f, s in zip(a[2], a[3]) if s == (H, Wd)]
    stream = m._stream()
    pc, ai, nacc = (C.c_float * k)(), (C.c_int * k)(), C.c_int(0)
    buf = torch.empty(4 * k * 2 * H * Wd * 3, device="cuda")

    def c_finish_tokens():
        return m.lib.sta_regress_views_tokens_finish(m._h, b"\x00" * k, 0.5, pc, ai, C.byref(nacc), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ai, stream)

    def c_finish_frames():
        return m.lib.sta_regress_views_finish(m._h, b"\x00" * k, 0.5, pc, ai, C.byref(nacc), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), stream)
    assert c_finish_tokens() == -1 and b"no scheduler call was begun" in m.lib.sta_last_error()
    # an f2 call pending: the tokens begin refuses, the tokens finish refuses and leaves it pending, its own finish serves it
    p = regress_views_begin(m, a[0], whole_j, H, Wd)
    with pytest.raises(_lib.StaError, match="pending|not been finished"):
        regress_views_tokens_begin(m, *a[:6])
    assert c_finish_tokens() == -1 and b"sta_regress_views_finish" in m.lib.sta_last_error()
    assert len(regress_views_finish(m, p, [False] * len(whole_j), 0.0)) == len(whole_j)
    # a tokens call pending: the f2 begin refuses, the f2 finish refuses and leaves it pending, abort releases it
    p = regress_views_tokens_begin(m, *a[:6])
    with pytest.raises(_lib.StaError, match="pending|not been finished"):
        regress_views_begin(m, a[0], whole_j, H, Wd)
    with pytest.raises(_lib.StaError, match="pending|not been finished"):
        regress_views_tokens_begin(m, *a[:6])
    with pytest.raises(_lib.StaError, match="pending"):
        m.head_pose_s(torch.zeros(1, m.cfg.dec_embed_dim, device="cuda"))
    assert c_finish_frames() == -1 and b"sta_regress_views_tokens_finish" in m.lib.sta_last_error()
    p.close()
    p.close()                                            # idempotent
    assert c_finish_tokens() == -1 and b"no scheduler call was begun" in m.lib.sta_last_error()
    with pytest.raises(AssertionError, match="already finished or aborted"):
        regress_views_tokens_finish(m, p, a[6], a[7])
    # the stream serves both kinds again
    with regress_views_tokens_begin(m, *a[:6]) as p:
        res = regress_views_tokens_finish(m, p, a[6], a[7])
    ref = regress_views_tokens(m, *a)
    torch.cuda.synchronize()
    assert [r.accepted for r in res] == [r.accepted for r in ref] == [bool(v) for v in g["accepted"]]
    assert len(regress_views_finish(m, regress_views_begin(m, a[0], whole_j, H, Wd), [True] * len(whole_j), 0.5)) == len(whole_j)
    torch.cuda.synchronize()


def test_entry_refusals(G):
    """The shim's refusals (what encode_tokens refuses) and the C entry's: status -1 with a message, the handle serves a good call after."""
    import torch
    from vista_slam_amd import _lib
    from vista_slam_amd.slam_scheduler import regress_views_tokens
    g, meta, m = _setup(G, "rvt_tiny_k3_win_sharp", "f16x3")
    a = list(_inputs(m, g, meta))
    k = len(a[2])

    def with_sel(e, side, sel):
        b = list(a)
        b[4 + side] = list(b[4 + side]); b[4 + side][e] = sel
        return b
    with pytest.raises(ValueError, match="outside the 5 x 6"):
        regress_views_tokens(m, *with_sel(0, 0, torch.tensor([30])))
    with pytest.raises(ValueError, match="empty"):
        regress_views_tokens(m, *with_sel(1, 1, torch.zeros(0, dtype=torch.int64)))
    with pytest.raises(ValueError, match="leaves the 4 x 5"):
        regress_views_tokens(m, *with_sel(2, 1, (0, 0, 5, 5)))
    with pytest.raises(AssertionError, match="int64"):
        regress_views_tokens(m, *with_sel(0, 0, torch.tensor([1.0])))
    with pytest.raises(AssertionError, match="one frame size and one selection"):
        regress_views_tokens(m, a[0], a[1], a[2], a[3], a[4][:2], a[5], a[6], a[7])
    with pytest.raises(AssertionError, match="expected"):
        regress_views_tokens(m, a[0][:-1], *a[1:])
    with pytest.raises(AssertionError, match="1 .. 16"):
        regress_views_tokens(m, a[0], a[1], a[2] * 6, a[3] * 6, a[4] * 6, a[5] * 6, a[6] * 6, a[7])
    fi = a[0]
    ptrs = (C.c_void_p * k)(*[f.data_ptr() for f in a[2]])
    Hj, Wj = (C.c_int * k)(*[s[0] for s in a[3]]), (C.c_int * k)(*[s[1] for s in a[3]])
    win = (C.c_int * (4 * k))(*([0, 0, 1, 1] * k))
    cnt = (C.c_int * k)(*([1] * k))
    idx = torch.zeros(1 << 10, dtype=torch.int64, device="cuda")
    pose = torch.empty(k, 4, 4, device="cuda")

    def begin(feat=fi.data_ptr(), Hi=a[1][0], Wi=a[1][1], fj=ptrs, hj=Hj, wj=Wj, kk=k, wi=win, ci=cnt, ii=idx.data_ptr(), wjn=win, po=pose.data_ptr()):
        return m.lib.sta_regress_views_tokens_begin(m._h, feat, Hi, Wi, fj, hj, wj, kk, wi, ci, ii, wjn, cnt, idx.data_ptr(), po, m._stream())
    bad_win = (C.c_int * (4 * k))(*([0, 0, 1, 1] * (k - 1) + [4, 0, 2, 1]))
    idx_win = (C.c_int * (4 * k))(*([0, 0, 0, 0] * k))
    for kw in (dict(feat=None), dict(po=None), dict(wi=None), dict(fj=None), dict(kk=0), dict(kk=17), dict(Hi=a[1][0] + 8),
               dict(hj=(C.c_int * k)(*([40] * k))), dict(wi=bad_win), dict(wi=idx_win, ci=(C.c_int * k)(*([1] * (k - 1) + [0]))),
               dict(wi=idx_win, ci=(C.c_int * k)(*([1 << 30] * k))), dict(wi=idx_win, ii=None), dict(feat=fi.data_ptr() + 4),
               dict(fj=(C.c_void_p * k)(*([None] * k)))):
        assert begin(**kw) == -1 and len(m.lib.sta_last_error()) > 0, kw
    res = regress_views_tokens(m, *a)          # nothing is pending, the handle still serves a good call
    torch.cuda.synchronize()
    assert [r.accepted for r in res] == [bool(v) for v in g["accepted"]]
