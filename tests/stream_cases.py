"""The matrix and the harness of tests/test_stream_order_gpu.py: every call is ordered by ITS stream alone, also while that stream
has work pending ("Streams and concurrency" in include/sta_mi355.h).  Host-only importable: torch and the package are imported inside
the callables.  tests/test_stream_inventory.py holds the entry points named here against the declarations of the header that take a
`void* stream`, in both directions.

The method, one delayed call (`delayed_call`): for a row with inputs A = make(m), a second valid input set B = make_b(m) of the same
shapes and a library-owned side stream s
  1. run A on s, synchronise, snapshot: ref_A, bit level; the same for B; the two must differ in at least one output;
  2. run B once more on s and synchronise: the stream's workspace, every caller-owned workspace, every buffer the Python layer keeps
     and the allocator blocks the outputs will land in now hold B's intermediates;
  3. poison the device inputs of A in place (true copies are kept): NaN for floating point, 0xFF for uint8 and bool, 0 for every
     other integer tensor - values a kernel may legally read, so that even a failing run cannot fault.  Host values (Python numbers,
     lists, host tensors) are handed over by value at call time and are not poisoned;
  4. on s: the delay kernel D (torch.cuda._sleep, 4 x the host wall time step 2's call took, at least 1 ms), the inputs restored
     by copy_ from the true copies, an event e_in; e_in must still be pending; then run A on s with no host synchronisation of the
     test's own;
  5. e_in still pending when the call returns: everything was enqueued while the inputs held poison - the run is conclusive
     ("asynchronous").  Done: the call waited for its stream, which is allowed only for a row that names an entry of SYNCS
     ("waited").  For those rows only the launches before the first wait are proven; everything behind it runs on an idle stream;
  6. synchronise s, compare every output with ref_A bit for bit.
Any launch, memset or copy of the call that is not ordered behind s reads poison or B's stale intermediates, or has its output
overwritten later: the result differs from ref_A, always, not occasionally.

A row: name, entries (the C entry points the call goes through), make(m) -> inputs, run(m, inputs, between=None) -> [(output name,
tensor)], shapes (text), no_prec (precisions the entry refuses), make_b (None: the default B - floats x 1.125, uint8 255 - v, integers
unchanged), layer (callables of the Python layer the row goes through that SYNCS may name).  Inputs are nested dicts / lists /
tuples of tensors and host values; what sits under a key that starts with "_" belongs to the row (state objects, caller workspaces,
tables) and is neither poisoned nor changed for B."""
import functools
from typing import Callable, NamedTuple, Optional, Tuple

import workspace_cases as WC

PRECISIONS = ("DEFAULT", "f16")       # the two route structures
DELAY_FACTOR = 4.0
MIN_HOST_MS = 0.25                    # a call of a few microseconds still gets a delay that covers the harness's own enqueues
MAX_STREAMS = 12


class Row(NamedTuple):
    name: str
    entries: Tuple[str, ...]
    make: Callable
    run: Callable
    shapes: str
    no_prec: Tuple[str, ...] = ()
    make_b: Optional[Callable] = None
    layer: Tuple[str, ...] = ()


# Entry points (and callables of the Python layer) that are documented to wait for their stream: the sentence that says so.
SYNCS = {
    "sta_world_pointcloud": "include/sta_mi355.h, sta_reserve: 'sta_voxel_downsample (workspace per point count; it synchronises its stream twice like "
                            "sta_world_pointcloud does once)' - the count comes back in count_host",
    "sta_voxel_downsample": "include/sta_mi355.h, sta_reserve: 'sta_voxel_downsample (workspace per point count; it synchronises its stream twice ...)'",
    "sta_regress_views": "include/sta_mi355.h: the one-call scheduler reads the pose confidences back to decide the edges (pose_conf_host / slot_host are host arrays)",
    "sta_regress_views_finish": "include/sta_mi355.h: phase B starts with the readback of the pose confidences phase A left pending",
    "sta_regress_views_tokens": "include/sta_mi355.h: as sta_regress_views - accepted_host / k_valid_host are host arrays filled by the call",
    "sta_regress_views_tokens_finish": "include/sta_mi355.h: as sta_regress_views_finish",
    "sta_pgo_optimize": "include/sta_mi355.h: the LM loop decides every trial on the host (info rows, n_info, status_out are host memory)",
    "loop.LoopDetector.detect_loop": "loop.LoopDetector: 'detect_loop scores the new view against all earlier ones in one launch and reads back once'",
    "flow.FlowTracker.compute_disparity": "flow.FlowTracker: 'Every compute_disparity after the first reads three doubles back once'",
}
# ... and entry points that are asynchronous themselves (the *_abi rows hold that), whose WRAPPER in sta_frontend.py reads positions on
# the host before it calls: the sentence of the Python layer
_GRID = ("sta_frontend.STAFrontend._grid_from_pos: 'a foreign tensor is compared with the grid ONCE (two device syncs) and the verdict is cached' - the "
         "harness restores the positions in place, which makes them a new version of the tensor")
_SUBSET = ("sta_frontend.STAFrontend._subset_positions: 'checked on the host ... a selection in host memory is uploaded with a synchronous copy and one on "
           "the device is read back: either way the call waits for its stream before the entry point is called'")
WRAPPER_SYNCS = {
    "sta_decode": _GRID, "sta_decode_pos": _GRID, "sta_decode_mixed": _GRID, "sta_decode_tokens": _GRID,
    "sta_decode_varlen": "sta_frontend.STAFrontend.decode_stereo_varlen: the range of the packed positions is read back - '(one device sync)'",
    "sta_encode_tokens": _SUBSET, "sta_encode_tokens_u8hwc": _SUBSET, "sta_encode_varlen": _SUBSET, "sta_encode_varlen_u8hwc": _SUBSET,
}
SYNCS.update(WRAPPER_SYNCS)
# stream-taking entry points without a row
EXEMPT = {
    "sta_regress_views_abort": "launches nothing: it drops the pending flag of the stream's context (every split-phase row ends through it in reset_switches)",
}


# ------------------------------------------------------------------------------------------ inputs: walk, poison, B
def _walk(x, fn, path=""):
    """fn(path, tensor) for every torch tensor of the nested inputs, keys that start with "_" left out."""
    import torch
    if isinstance(x, torch.Tensor):
        fn(path, x)
    elif isinstance(x, dict):
        for k in x:
            if not str(k).startswith("_"):
                _walk(x[k], fn, f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _walk(v, fn, f"{path}[{i}]")


def device_inputs(x):
    """[(path, tensor)] of the device tensors of the inputs, each storage range once."""
    out, seen = [], set()

    def take(path, t):
        key = (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)
        if t.is_cuda and t.numel() and key not in seen:
            seen.add(key)
            out.append((path, t))
    _walk(x, take)
    return out


def poison_(t):
    import torch
    if t.is_floating_point():
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(0xFF)
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        t.fill_(0)


def default_b(make):
    """The default second input set: make(m) again with floats x 1.125, uint8 255 - v, everything else unchanged."""
    def make_b(m):
        import torch
        x = make(m)

        def change(_path, t):
            if t.is_floating_point():
                t.mul_(1.125)
            elif t.dtype == torch.uint8:
                t.copy_(255 - t)
        _walk(x, change)
        return x
    return make_b


def zero_alloc():
    """While it is open, torch.empty is torch.zeros: the rows of the wrappers whose outputs have rows the kernels leave unwritten by
    contract (behind a device-side count) compare whole buffers bit for bit.  The fills are enqueued on the current stream, like the
    call."""
    import contextlib
    import torch

    @contextlib.contextmanager
    def cm():
        real = torch.empty
        torch.empty = torch.zeros
        try:
            yield
        finally:
            torch.empty = real
    return cm()


def _up(a):
    import numpy as np
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------ post, rope, encoder_norm
def _mk_scale(seed):
    def make(m):
        import post_cases as PC
        return {"d": [_up(a) for a in PC.scale_inputs(65, seed=47 + seed)]}
    return make


def _run_scale(m, x, between=None):
    from vista_slam_amd import post
    return [("s", post.estimate_scale_with_depth_and_confidence(m, *x["d"]))]


def _mk_se3(seed):
    def make(m):
        import post_cases as PC
        return {"pose": _up(PC.se3_table(seed=31 + seed)[:65])}
    return make


def _run_se3(m, x, between=None):
    from vista_slam_amd import formats
    return [("se3", formats.mat_to_se3(m, x["pose"]))]


PACK_B, PACK_H, PACK_W = 3, 15, 17        # 255 pixels: not a multiple of anything


def _mk_pack(seed):
    def make(m):
        import torch
        gen = torch.Generator(device="cuda").manual_seed(59 + seed)
        one = lambda: {"pts3d_pred": torch.randn(PACK_B, PACK_H, PACK_W, 3, device="cuda", generator=gen),
                       "conf": torch.rand(PACK_B, PACK_H, PACK_W, device="cuda", generator=gen) + 1,
                       "relative_pose": torch.randn(PACK_B, 4, 4, device="cuda", generator=gen),
                       "relative_pose_conf": torch.rand(PACK_B, device="cuda", generator=gen)}
        return {"main": one(), "supp": one()}
    return make


def _run_pack(m, x, between=None):
    from vista_slam_amd import parallel
    return [("record", parallel.pack_compact(x["main"], x["supp"], model=m))]


ROPE_B, ROPE_N, ROPE_H, ROPE_D = 2, 13, 3, 64


def _mk_rope(seed):
    def make(m):
        import torch
        gen = torch.Generator(device="cuda").manual_seed(61 + seed)
        tok = torch.randn(ROPE_B, ROPE_N, ROPE_H, ROPE_D, device="cuda", generator=gen)
        pos = torch.randint(0, 14, (ROPE_B, ROPE_N, 2), device="cuda", generator=gen)
        return {"tok": tok, "tok16": tok.half(), "pos": pos}
    return make


def _run_rope(m, x, between=None):
    """both forms rotate in place: on copies made on the call's stream"""
    from vista_slam_amd import _lib
    from vista_slam_amd.sta_frontend import rope2d_inplace
    a, b = x["tok"].clone(), x["tok16"].clone()
    _lib.check(_lib.load().sta_rope2d_inplace(a.data_ptr(), a.stride(0), a.stride(1), x["pos"].data_ptr(), ROPE_B, ROPE_N, ROPE_H, ROPE_D, 100.0, 1.0,
                                              m._stream()))
    rope2d_inplace(b, x["pos"], 100.0, -1.0)
    return [("f32", a), ("f16", b)]


NORM_ROWS = 37


def _mk_norm(seed):
    def make(m):
        import torch
        gen = torch.Generator(device="cuda").manual_seed(67 + seed)
        return {"x": torch.randn(NORM_ROWS, m.cfg.enc_embed_dim, device="cuda", generator=gen)}
    return make


def _run_norm(m, x, between=None):
    import torch
    from vista_slam_amd import _lib
    out = torch.empty_like(x["x"])
    _lib.check(m.lib.sta_encoder_norm(m._h, x["x"].data_ptr(), NORM_ROWS, out.data_ptr(), m._stream()))
    return [("out", out)]


# ------------------------------------------------------------------------------------------ select
def _mk_select(aligned, seed):
    def make(m):
        import torch
        import select_cases as S
        if aligned:
            return {"maps": [_up(S.random_mask(48, 64, 40 + seed)), _up(S.random_mask(80, 48, 50 + seed))]}
        fl = S.hostile_float(48, 64, 61 + seed)
        buf = torch.zeros(48 * 64 + 4, dtype=torch.float32, device="cuda")
        view = buf[1:1 + 48 * 64].view(48, 64)          # 4 bytes into its storage: the element-wise path
        view.copy_(torch.from_numpy(fl))
        assert view.data_ptr() % 16 == 4
        return {"maps": [view]}
    return make


def _run_select(kw):
    def run(m, x, between=None):
        from vista_slam_amd import select
        with zero_alloc():
            sel = select.select_tokens_from_maps(m, x["maps"], **kw)
        return [("score", sel.score_slots), ("index", sel.index_slots), ("pos", sel.pos_slots), ("meta", sel._meta)]
    return run


# ------------------------------------------------------------------------------------------ flow
FLOW_H, FLOW_W = 45, 91


def _flow_frames(seed):
    import flow_cases as F
    return F.blob_frame(FLOW_H, FLOW_W, seed=7 + seed), F.blob_frame(FLOW_H, FLOW_W, (1.25, -0.5), seed=7 + seed)


def _mk_flow_pyramid(seed):
    def make(m):
        import numpy as np
        return {"gray": _up(np.stack(_flow_frames(seed)))}
    return make


def _run_flow_pyramid(m, x, between=None):
    from vista_slam_amd import flow
    with zero_alloc():
        pyr = flow.pyramid(m, x["gray"])
    return [("pyramid", pyr.buf)]


def _mk_flow_corners(seed):
    def make(m):
        import torch
        from vista_slam_amd import flow
        a, _b = _flow_frames(seed)
        p = flow.plan(FLOW_H, FLOW_W, 1, flow.WIN, 0, 64)
        return {"img": _up(a), "_ws": torch.zeros(p.workspace_bytes, device="cuda", dtype=torch.uint8)}
    return make


def _run_flow_corners(m, x, between=None):
    from vista_slam_amd import flow
    with zero_alloc():
        corners, n = flow.good_features(m, x["img"], max_corners=64, min_distance=4, workspace=x["_ws"])
    return [("corners", corners), ("n", n)]


def _mk_flow_track(seed):
    def make(m):
        import torch
        from vista_slam_amd import flow
        a, b = _flow_frames(seed)
        prev, nxt = flow.pyramid(m, _up(a)), flow.pyramid(m, _up(b))
        with zero_alloc():
            pts, n = flow.good_features(m, prev, max_corners=64, min_distance=4)
        torch.cuda.synchronize()
        return {"prev": prev.buf, "next": nxt.buf, "pts": pts, "n": n, "_prev": prev, "_next": nxt}
    return make


def _run_flow_track(m, x, between=None):
    from vista_slam_amd import flow
    with zero_alloc():
        out, status, stats = flow.track(m, x["_prev"], x["_next"], x["pts"], x["n"])
    return [("next_pts", out), ("status", status), ("stats", stats)]


def _mk_flow_tracker(seed):
    def make(m):
        import torch
        from vista_slam_amd import flow
        a, b = _flow_frames(seed)
        tr = flow.FlowTracker(m, 1e9)               # never a keyframe after the first: the step leaves the tracker as it was
        tr.initialize_keyframe(_up(a))
        torch.cuda.synchronize()
        return {"img": _up(b), "_tracker": tr}
    return make


def _run_flow_tracker(m, x, between=None):
    import torch
    tr = x["_tracker"]
    key = tr.compute_disparity(x["img"])
    assert not key
    return [("last", torch.tensor(list(tr.last), dtype=torch.float64))]


# ------------------------------------------------------------------------------------------ loop
ORB_KW = dict(nfeatures=20, nlevels=3, edge=22)
ORB_H, ORB_W = 70, 67


@functools.lru_cache(maxsize=None)
def _vocab_arrays():
    import loop_cases as L
    return L.vocab_arrays(L.make_vocab(10, 2, seed=5))


def _vocab(m):
    from vista_slam_amd import loop
    V = _vocab_arrays()
    return loop.Vocabulary.from_arrays(V.node_desc, V.child_first, V.child_count, V.word_of, V.word_weight).bind(m)


def _mk_orb(seed):
    def make(m):
        import flow_cases as F
        from vista_slam_amd import loop
        return {"img": _up(F.blob_frame(ORB_H, ORB_W, seed=7 + seed, n_blobs=30)), "_ex": loop.Extractor(m, **ORB_KW)}
    return make


def _run_orb(m, x, between=None):
    with zero_alloc():
        kp, resp, desc, n, _plan = x["_ex"].extract(x["img"])
    return [("kp", kp), ("resp", resp), ("desc", desc), ("n", n)]


def _mk_bow_transform(seed):
    def make(m):
        import loop_cases as L
        return {"desc": _up(L.random_desc(65, 3 + seed, _vocab_arrays())), "_voc": _vocab(m)}
    return make


def _run_bow_transform(m, x, between=None):
    with zero_alloc():
        v = x["_voc"].transform(x["desc"])
    return [("words", v.words), ("counts", v.counts), ("vals", v.vals), ("n", v.n)]


BOW_VIEWS, BOW_CAP = 3, 65


def _mk_bow_score(seed):
    def make(m):
        import loop_cases as L
        import torch
        voc, V = _vocab(m), _vocab_arrays()
        with zero_alloc():
            vs = [voc.transform(_up(L.random_desc(BOW_CAP, 10 * seed + 21 + i, V))) for i in range(BOW_VIEWS + 1)]
        torch.cuda.synchronize()
        q, db = vs[0], vs[1:]
        return {"q_words": q.words, "q_vals": q.vals, "q_n": q.n, "db_words": torch.stack([v.words for v in db]), "db_vals": torch.stack([v.vals for v in db]),
                "db_n": torch.cat([v.n for v in db]), "rows": torch.arange(BOW_VIEWS, device="cuda", dtype=torch.int32)}
    return make


def _run_bow_score(m, x, between=None):
    import torch
    from vista_slam_amd import _lib
    sim = torch.zeros(BOW_VIEWS, device="cuda", dtype=torch.float64)
    _lib.check(m.lib.sta_bow_score(m._h, x["q_words"].data_ptr(), x["q_vals"].data_ptr(), x["q_n"].data_ptr(), BOW_CAP, x["db_words"].data_ptr(),
                                   x["db_vals"].data_ptr(), x["db_n"].data_ptr(), BOW_VIEWS, BOW_CAP, x["rows"].data_ptr(), BOW_VIEWS, sim.data_ptr(),
                                   m._stream()))
    return [("sim", sim)]


def _mk_detect_loop(seed):
    def make(m):
        import flow_cases as F
        import torch
        from vista_slam_amd import loop
        det = loop.LoopDetector(m, _vocab(m), 1, 0, 1, nfeatures=100, nlevels=3, max_views=8)
        frames = [F.blob_frame(96, 128, (0.7 * k, 0.3 * k), seed=7 + seed, n_blobs=60) for k in range(4)]
        for f in frames[:3]:                        # the three-frame database
            det.compute_bow_feat(_up(f))
        torch.cuda.synchronize()
        return {"img": _up(frames[3]), "_det": det}
    return make


def _run_detect_loop(m, x, between=None):
    import torch
    det = x["_det"]
    n = len(det.bow_feats)
    try:
        cands = det.detect_loop(x["img"], n)
        sims = list(det.last)
    finally:
        del det.bow_feats[n:]                       # the database row is overwritten by the next run
    flat = [float(v) for c in cands for v in c]
    return [("similarities", torch.tensor(sims, dtype=torch.float64)), ("candidates", torch.tensor(flat, dtype=torch.float64))]


# ------------------------------------------------------------------------------------------ pgo
def _mk_sim3(seed):
    def make(m):
        import pgo_cases as P
        import torch
        a, b, xi = P.op_inputs(65, seed=7 + seed)
        return {"a": _up(a), "b": _up(b), "xi": _up(xi), "mask": (torch.arange(65, device="cuda") % 3 != 0).to(torch.uint8)}
    return make


def _run_sim3(m, x, between=None):
    from vista_slam_amd import pgo
    return [("mul", pgo.sim3_mul(m, x["a"], x["b"])), ("between", pgo.sim3_between(m, x["a"], x["b"])), ("log", pgo.sim3_log(m, x["a"])),
            ("exp", pgo.sim3_exp(m, x["xi"])), ("retract", pgo.sim3_retract(m, x["xi"], x["a"], x["mask"]))]


def _pgo_graph(m, seed):
    import pgo_cases as P
    from vista_slam_amd import pgo
    g = P.random_graph(65, 65, seed=5 + seed)
    G = pgo.Graph(m, 65, g["edges"], g["poses"], g["confs"], "all")
    return g, G


def _graph_inputs(G):
    return {"edges": G.edges, "poses": G.poses, "confs": G.confs, "opt": G.opt, "_G": G}


def _mk_pgo_index(seed):
    def make(m):
        _g, G = _pgo_graph(m, seed)
        return _graph_inputs(G)
    return make


def _run_pgo_index(m, x, between=None):
    with zero_alloc():
        off, inc, status = x["_G"].index()
    return [("off", off), ("inc", inc), ("status", status)]


def _mk_pgo_linearize(seed, solve=False):
    def make(m):
        import torch
        from vista_slam_amd import pgo
        g, G = _pgo_graph(m, seed)
        with zero_alloc():
            G.index()
            x = dict(_graph_inputs(G), X=_up(g["nodes"]), off=G.off, inc=G.inc, status=G.status)
            if solve:
                lin = pgo.linearize(G, x["X"])
                x.update(S=lin["S"], g=lin["g"], blocks=lin["blocks"], _lin=lin)
        torch.cuda.synchronize()
        return x
    return make


def _run_pgo_linearize(m, x, between=None):
    from vista_slam_amd import pgo
    with zero_alloc():
        o = pgo.linearize(x["_G"], x["X"])
    return [(k, o[k]) for k in sorted(o)]


def _run_pgo_solve(m, x, between=None):
    from vista_slam_amd import pgo
    with zero_alloc():
        d, stats = pgo.solve(x["_G"], x["_lin"])
    return [("d", d), ("stats", stats)]


def _mk_pgo_optimize(seed):
    def make(m):
        import pgo_cases as P
        g = P.slam_graph(12, seed=seed)
        return {"nodes": _up(g["nodes"]), "edges": _up(g["edges"]), "poses": _up(g["poses"]), "confs": _up(g["confs"])}
    return make


def _run_pgo_optimize(m, x, between=None):
    import pgo_cases as P
    from vista_slam_amd import pgo
    return [("nodes", pgo.optimize(m, x["nodes"], x["edges"], x["poses"], x["confs"], **P.LM_ARGS))]


# ------------------------------------------------------------------------------------------ graph
def _mk_graph(seed):
    def make(m):
        import graph_cases as GC
        import torch
        from vista_slam_amd import graph
        from vista_slam_amd.slam_scheduler import EdgeResult
        seq = GC.scripted("keyframe 2", 16, 16, seed=seed)          # keyframe 1, then one keyframe with two accepted edges
        tensors, dev_seq = [], []
        for i, js, edges in seq:
            rs = []
            for e in edges:
                t = [_up(e.pose), _up(e.confs), _up(e.intri), _up(e.depths)]
                tensors += t
                rs.append(EdgeResult(t[0], e.rel_pose_conf, True, t[1], t[2], t[3]))
            dev_seq.append((i, js, rs))
        g = graph.PoseGraph(m, graph.plan(8, 3, 3, 16, 16))
        torch.cuda.synchronize()
        return {"t": tensors, "_seq": dev_seq, "_g": g}
    return make


def _run_graph(m, x, between=None):
    g = x["_g"]
    g.reset()
    for i, js, rs in x["_seq"]:
        g.commit(i, js, rs)
    ex = g.export(conf_thres=1.0, filter_outlier=True, scaled=True)
    state = [(k, getattr(g, k)) for k in ("poses", "edges", "edge_poses", "edge_confs", "mean_conf", "first_node", "best_node", "best_conf")]
    n = g.num_nodes
    return state + [("depth", g.depth[:n]), ("conf", g.conf[:n]), ("intri", g.intri[:n]), ("partials", g.call_partials())] + \
        [(f"export.{k}", getattr(ex, k)) for k in ("poses", "scales", "depths", "confs", "intrinsics")]


# ------------------------------------------------------------------------------------------ the token routes through the C ABI itself
# The wrappers of these entries read positions on the host before they call (SYNCS): behind that wait the stream is idle and the
# launches prove nothing.  These rows hand the entry points device positions and host counts directly, so the whole call is enqueued
# under the delay.  Inputs: the workspace rows' own.
def _dec_outs(m, B, n1, n2, rows=None):
    """the dec_depth + 1 output tensors of both sides and their pointer arrays (rows: packed [rows, D] instead of [B, n + 1, D])"""
    import ctypes as C
    import torch
    L, D = m.cfg.dec_depth + 1, m.cfg.dec_embed_dim
    mk = (lambda n, r: torch.empty(r, D, device=m.device)) if rows else (lambda n, r: torch.empty(B, n + 1, D, device=m.device))
    o1, o2 = [mk(n1, rows and rows[0]) for _ in range(L)], [mk(n2, rows and rows[1]) for _ in range(L)]
    return o1, o2, (C.c_void_p * L)(*[t.data_ptr() for t in o1]), (C.c_void_p * L)(*[t.data_ptr() for t in o2])


def _run_decode_abi(m, x, between=None):
    from vista_slam_amd import _lib
    B, N, _E = x["fa"].shape
    o1, o2, a1, a2 = _dec_outs(m, B, N, N)
    _lib.check(m.lib.sta_decode(m._h, x["fa"].data_ptr(), x["fb"].data_ptr(), B, WC.H0 // 16, WC.W0 // 16, a1, a2, m._stream()))
    return WC._named("dec1", o1) + WC._named("dec2", o2)


DECODE_POS_MAX = 4            # _mk_decode_pos: the 2 x 3 grid shifted by (1, 2)


def _run_decode_pos_abi(m, x, between=None, p1="p1", pos_max=DECODE_POS_MAX):
    from vista_slam_amd import _lib
    B, N, _E = x["fa"].shape
    o1, o2, a1, a2 = _dec_outs(m, B, N, N)
    _lib.check(m.lib.sta_decode_pos(m._h, x["fa"].data_ptr(), x["fb"].data_ptr(), x[p1].data_ptr(), x["p2"].data_ptr(), B, N, pos_max, a1, a2, m._stream()))
    return WC._named("dec1", o1) + WC._named("dec2", o2)


def _run_decode_mixed_abi(m, x, between=None):
    from vista_slam_amd import _lib
    B, N1, _E = x["fa"].shape
    N2 = x["fb"].shape[1]
    o1, o2, a1, a2 = _dec_outs(m, B, N1, N2)
    _lib.check(m.lib.sta_decode_mixed(m._h, x["fa"].data_ptr(), x["fb"].data_ptr(), B, 2, 3, 2, 1, a1, a2, m._stream()))      # 32x48 against 32x16
    return WC._named("dec1", o1) + WC._named("dec2", o2)


def _run_decode_tokens_abi(m, x, between=None):
    from vista_slam_amd import _lib
    B, N1, _E = x["f1"].shape
    N2 = x["f2"].shape[1]
    o1, o2, a1, a2 = _dec_outs(m, B, N1, N2)
    _lib.check(m.lib.sta_decode_tokens(m._h, x["f1"].data_ptr(), x["f2"].data_ptr(), x["p1"].data_ptr(), x["p2"].data_ptr(), B, N1, N2, 2, a1, a2,
                                       m._stream()))
    return WC._named("dec1", o1) + WC._named("dec2", o2)


def _run_decode_varlen_abi(m, x, between=None):
    import ctypes as C
    import torch
    from vista_slam_amd import _lib
    B = len(x["f1"])
    n1, n2 = [int(f.shape[0]) for f in x["f1"]], [int(f.shape[0]) for f in x["f2"]]
    f1, f2, q1, q2 = (torch.cat(x[k], 0).contiguous() for k in ("f1", "f2", "q1", "q2"))          # (packed on the call's stream)
    o1, o2, a1, a2 = _dec_outs(m, B, 0, 0, rows=(sum(n1) + B, sum(n2) + B))
    _lib.check(m.lib.sta_decode_varlen(m._h, f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), (C.c_int * B)(*n1), (C.c_int * B)(*n2), B, 2,
                                       a1, a2, m._stream()))
    return WC._named("dec1", o1) + WC._named("dec2", o2)


def _mk_encode_tokens_abi(m):
    import torch
    x = WC._mk_encode_tokens(m)
    idx = x["index"].cuda()
    x["q"] = torch.stack([torch.div(idx, WC.W0 // 16, rounding_mode="floor"), idx % (WC.W0 // 16)], -1).contiguous()
    return x


def _run_encode_tokens_abi(m, x, between=None):
    import torch
    from vista_slam_amd import _lib
    B, N = x["q"].shape[:2]
    feat = torch.empty(B, N, m.cfg.enc_embed_dim, device=m.device)
    _lib.check(m.lib.sta_encode_tokens(m._h, x["img"].data_ptr(), x["q"].data_ptr(), B, WC.H0, WC.W0, N, feat.data_ptr(), m._stream()))
    u8 = torch.empty_like(feat)
    _lib.check(m.lib.sta_encode_tokens_u8hwc(m._h, x["u8"].data_ptr(), x["q"].data_ptr(), B, WC.H0, WC.W0, N, u8.data_ptr(), m._stream()))
    return [("feat", feat), ("feat_u8", u8)]


def _mk_encode_varlen_abi(m):
    import torch
    x = WC._mk_encode_varlen(m)
    qs = []
    for (h, w), ix in zip(WC.VARLEN_FRAMES, x["index"]):
        ix = ix.cuda()
        qs.append(torch.stack([torch.div(ix, w // 16, rounding_mode="floor"), ix % (w // 16)], -1))
    x["q"] = torch.cat(qs, 0).contiguous()
    return x


def _run_encode_varlen_abi(m, x, between=None):
    import ctypes as C
    import torch
    from vista_slam_amd import _lib
    B = len(WC.VARLEN_FRAMES)
    counts = [len(ix) for ix in WC.VARLEN_INDEX]
    Hs, Ws = (C.c_int * B)(*[h for h, _w in WC.VARLEN_FRAMES]), (C.c_int * B)(*[w for _h, w in WC.VARLEN_FRAMES])
    outs = []
    for key, entry in (("imgs", m.lib.sta_encode_varlen), ("u8", m.lib.sta_encode_varlen_u8hwc)):
        feat = torch.empty(sum(counts), m.cfg.enc_embed_dim, device=m.device)
        ptrs = (C.c_void_p * B)(*[f.data_ptr() for f in x[key]])
        _lib.check(entry(m._h, ptrs, Hs, Ws, x["q"].data_ptr(), (C.c_int * B)(*counts), B, feat.data_ptr(), m._stream()))
        outs.append(("feat_" + key, feat))
    return outs


ABI_ROWS = [
    Row("decode_abi", ("sta_decode",), WC._mk_decode, _run_decode_abi, "B 2, 6 tokens; the entry point itself"),
    Row("decode_pos_abi", ("sta_decode_pos",), WC._mk_decode_pos, _run_decode_pos_abi, "B 2, 6 tokens, shifted and reversed positions; the entry point itself"),
    Row("decode_mixed_abi", ("sta_decode_mixed",), WC._mk_decode_mixed, _run_decode_mixed_abi, "B 2, 6 against 2 tokens; the entry point itself"),
    Row("decode_tokens_abi", ("sta_decode_tokens",), WC._mk_decode_tokens, _run_decode_tokens_abi, "B 2, 5 against 2 tokens; the entry point itself"),
    Row("decode_varlen_abi", ("sta_decode_varlen",), WC._mk_decode_varlen, _run_decode_varlen_abi, "4|3, 6|2, 1|5 tokens; the entry point itself"),
    Row("encode_tokens_abi", ("sta_encode_tokens", "sta_encode_tokens_u8hwc"), _mk_encode_tokens_abi, _run_encode_tokens_abi,
        "B 2, 5 of 6 tokens, fp32 and uint8 HWC; the entry points themselves"),
    Row("encode_varlen_abi", ("sta_encode_varlen", "sta_encode_varlen_u8hwc"), _mk_encode_varlen_abi, _run_encode_varlen_abi,
        "4 / 6 / 1 tokens of 32x48, 48x32, 32x32, fp32 and uint8 HWC; the entry points themselves"),
]
WRAPPER_WAITS = {"decode_abi", "decode_pos_abi", "decode_mixed_abi", "decode_tokens_abi", "decode_varlen_abi", "encode_tokens_abi", "encode_varlen_abi"}


# ------------------------------------------------------------------------------------------ the matrix
def _seeded(name, entries, mk, run, shapes, no_prec=(), layer=()):
    return Row(name, entries, mk(0), run, shapes, no_prec, mk(1), layer)


ROWS = [Row(c.name, c.entries, c.make, c.run, c.shapes, c.no_prec, None) for c in WC.CASES] + [
    _seeded("estimate_scale", ("sta_estimate_scale",), _mk_scale, _run_scale, "65 pairs"),
    _seeded("mat_to_se3", ("sta_mat_to_se3",), _mk_se3, _run_se3, "65 poses"),
    _seeded("pack_compact", ("sta_pack_compact",), _mk_pack, _run_pack, "B 3, 15x17"),
    _seeded("rope2d_inplace", ("sta_rope2d_inplace", "sta_rope2d_inplace_dtype"), _mk_rope, _run_rope, "B 2, 13 tokens, 3 heads of 64; fp32 and fp16"),
    _seeded("encoder_norm", ("sta_encoder_norm",), _mk_norm, _run_norm, "37 rows"),
    _seeded("select_patches", ("sta_select_patches",), functools.partial(_mk_select, True), _run_select(dict(min_score=100, margin=1)),
            "uint8 48x64 and 80x48, min_score with margin"),
    _seeded("select_patches_unaligned", ("sta_select_patches",), functools.partial(_mk_select, False), _run_select(dict(top_k=4)),
            "float32 48x64 at +4 bytes, top_k"),
    _seeded("flow_pyramid", ("sta_flow_pyramid",), _mk_flow_pyramid, _run_flow_pyramid, "2 frames of 45x91"),
    _seeded("flow_corners", ("sta_flow_pyramid", "sta_flow_corners"), _mk_flow_corners, _run_flow_corners, "45x91, 64 corners, the row's workspace"),
    _seeded("flow_track", ("sta_flow_track",), _mk_flow_track, _run_flow_track, "45x91, device count"),
    _seeded("flow_tracker_step", ("sta_flow_pyramid", "sta_flow_track"), _mk_flow_tracker, _run_flow_tracker, "FlowTracker.compute_disparity, 45x91",
            layer=("flow.FlowTracker.compute_disparity",)),
    _seeded("orb_extract", ("sta_orb_extract",), _mk_orb, _run_orb, "70x67, 3 levels, 20 features"),
    _seeded("bow_transform", ("sta_bow_transform",), _mk_bow_transform, _run_bow_transform, "65 descriptors, 100 words"),
    _seeded("bow_score", ("sta_bow_score",), _mk_bow_score, _run_bow_score, "one vector against 3 views"),
    _seeded("detect_loop", ("sta_orb_extract", "sta_bow_transform", "sta_bow_score"), _mk_detect_loop, _run_detect_loop,
            "LoopDetector.detect_loop, 96x128, a three-frame database", layer=("loop.LoopDetector.detect_loop",)),
    _seeded("sim3_op", ("sta_sim3_op",), _mk_sim3, _run_sim3, "65 elements: mul, between, log, exp, masked retract"),
    _seeded("pgo_index", ("sta_pgo_index",), _mk_pgo_index, _run_pgo_index, "random 65 / 65"),
    _seeded("pgo_linearize", ("sta_pgo_linearize",), _mk_pgo_linearize, _run_pgo_linearize, "random 65 / 65"),
    _seeded("pgo_solve", ("sta_pgo_solve",), functools.partial(_mk_pgo_linearize, solve=True), _run_pgo_solve, "random 65 / 65"),
    _seeded("pgo_optimize", ("sta_pgo_optimize",), _mk_pgo_optimize, _run_pgo_optimize, "slam12", layer=("pgo.optimize",)),
    _seeded("graph", ("sta_graph_reset", "sta_graph_commit", "sta_graph_export"), _mk_graph, _run_graph,
            "keyframe 1, then one keyframe with two accepted edges, 16x16 maps; reset, commit x 2, export"),
] + ABI_ROWS


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    """The keys of SYNCS a row may wait through.  The *_abi rows call the entry points themselves: the waits of the wrappers
    (WRAPPER_SYNCS) are not theirs."""
    keys = SYNCS if row.name not in WRAPPER_WAITS else {k: v for k, v in SYNCS.items() if k not in WRAPPER_SYNCS}
    return [k for k in row.entries + row.layer if k in keys]


def runs():
    return [(r.name, p) for r in ROWS for p in PRECISIONS if p not in r.no_prec]


def second_inputs(row):
    return row.make_b if row.make_b is not None else default_b(row.make)


# ------------------------------------------------------------------------------------------ the harness
class Pending(NamedTuple):
    event: object
    delay_ms: float


_cycles_per_ms = []


def cycles_per_ms():
    """torch.cuda._sleep spins for a number of device clock ticks: ticks per millisecond, measured once with an event pair."""
    import torch
    if not _cycles_per_ms:
        torch.cuda._sleep(1_000_000)                   # (the first launch loads the kernel)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20_000_000
        a.record(); torch.cuda._sleep(n); b.record()
        torch.cuda.synchronize()
        _cycles_per_ms.append(n / max(a.elapsed_time(b), 1e-3))
    return _cycles_per_ms[0]


def overlaps_null_stream(s, ms=4.0):
    """Does work on the null stream run while s is busy?  The runtime maps streams onto a few hardware queues, and a stream that shares
    its queue with the null stream would HIDE a stray null-stream launch behind the delay: measured, not assumed."""
    import torch
    null = torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(ms * cycles_per_ms()))
        e_s = torch.cuda.Event()
        e_s.record(s)
    with torch.cuda.stream(null):
        torch.zeros(64, device="cuda").add_(1)
        e_n = torch.cuda.Event()
        e_n.record(null)
    e_n.synchronize()
    ok = not e_s.query()
    torch.cuda.synchronize()
    return ok


def side_streams(m, n=2):
    """n of the library's pipeline streams (non-blocking, measured to overlap pairwise) that also overlap with the null stream."""
    cands = m.pipeline_streams(4)
    cands = cands[:max(m.pipeline_streams_verified, 1)]
    good = [s for s in cands if overlaps_null_stream(s)]
    assert len(good) >= n, (f"only {len(good)} of the {len(cands)} verified pipeline streams overlap with the null stream: the queue mapping of this "
                            "process would hide stray launches")
    return good[:n]


def poison_inputs(x):
    """-> [(tensor, true copy)] of the device inputs, which now hold poison (device-synchronised)"""
    import torch
    pairs = [(t, t.clone()) for _p, t in device_inputs(x)]
    for t, _c in pairs:
        poison_(t)
    torch.cuda.synchronize()
    return pairs


def pend(s, pairs, delay_ms):
    """On stream s: the delay, the inputs restored behind it, an event behind that.  The event must still be pending."""
    import torch
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(delay_ms * cycles_per_ms()))
        for t, c in pairs:
            t.copy_(c)
        e = torch.cuda.Event()
        e.record(s)
    assert not e.query(), f"the delay of {delay_ms:.1f} ms ended before the inputs were restored behind it: the delay is too short"
    return Pending(e, delay_ms)


class Report(NamedTuple):
    host_ms: float                # host wall time of step 2's call, on an idle stream: an upper bound of the enqueue time
    delay_ms: float               # DELAY_FACTOR x that (x at least MIN_HOST_MS)
    waited: bool
    diff: Optional[str]           # first_difference against ref_A, None when bit-identical
    call_ms: float = 0.0          # host wall time of the delayed call itself

    def line(self):
        return (f"host {self.host_ms:.2f} ms, delay {self.delay_ms:.1f} ms, the delayed call returned after {self.call_ms:.2f} ms, "
                f"class {'waited' if self.waited else 'asynchronous'}; {'bit-identical to the reference' if self.diff is None else self.diff}")


def timed_run(row, m, s, x):
    """row.run on s from an idle stream, synchronised -> (outputs snapshot, host wall time of the call in ms)"""
    import time
    import torch
    from helpers import snapshot
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t0 = time.perf_counter()
        outs = row.run(m, x)
        ms = (time.perf_counter() - t0) * 1e3
    return snapshot(outs), ms


def references(row, m, s):
    """Steps 1: -> (A, B, ref_A, ref_B); ref_A and ref_B must differ."""
    import torch
    from helpers import first_difference
    with torch.cuda.stream(s):
        xa, xb = row.make(m), second_inputs(row)(m)
    torch.cuda.synchronize()
    ref_a, _ = timed_run(row, m, s, xa)
    ref_b, _ = timed_run(row, m, s, xb)
    assert first_difference(ref_b, ref_a) is not None, f"{row.name}: the second input set gives the outputs of the first: it proves nothing for this row"
    return xa, xb, ref_a, ref_b


def delayed_call(row, m, s, xa, xb, ref_a, ref_b, before_sync=None):
    """Steps 2 - 6 -> Report.  before_sync(pending): called behind the call, while the stream is still pending (the hazard tests)."""
    import time
    import torch
    from helpers import first_difference, snapshot
    got_b, host_ms = timed_run(row, m, s, xb)                      # 2: stale state
    diff = first_difference(got_b, ref_b)
    assert diff is None, f"{row.name}: the second input set does not reproduce its own reference - {diff}"
    pairs = poison_inputs(xa)                                      # 3
    delay_ms = DELAY_FACTOR * max(host_ms, MIN_HOST_MS)
    p = pend(s, pairs, delay_ms)                                   # 4
    with torch.cuda.stream(s):
        t0 = time.perf_counter()
        outs = row.run(m, xa)
        call_ms = (time.perf_counter() - t0) * 1e3
    waited = p.event.query()                                       # 5
    if before_sync is not None:
        before_sync(p)
    got = snapshot(outs)                                           # 6 (synchronises)
    return Report(host_ms, delay_ms, waited, first_difference(got, ref_a), call_ms)
