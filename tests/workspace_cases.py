"""The matrix of tests/test_workspace_gpu.py: one row per product entry point that runs on a stream's scratch context (StreamCtx in
vista_slam_amd/csrc/sta_api.hip: workspace, split-K scratch, slab scratch, the side lane's scratch).  Host-only importable: torch and
the package are imported inside the callables.  tests/test_workspace_inventory.py holds the set of entry points named here against
the call sites of plan_and_run( / cur_bump( in the sources, in both directions.

A row: name, entries (the C entry points the call goes through), family (enc / dec / pair / head / sched / rows), rank (size order
inside the family: the transition test runs largest - smallest - largest), make(m) -> inputs in CALLER memory (torch tensors,
host arrays), run(m, inputs, between=None) -> [(output name, tensor)], shapes (text), no_prec (precisions the entry refuses).
Tiny model, the smallest shapes at which the route has its special structure (32x48 frames = 2x3 tokens unless noted)."""
from typing import Callable, NamedTuple, Tuple

FILLS = (0x00, 0xFF, 0x3C, 0x7B)      # zeros; NaN as fp16 / fp32, -1 as int32; 1.06 per fp16 plane; 61280 as fp16, 1.3e36 as fp32
PRECISIONS = ("f16", "f16x3", "f16x3m", "DEFAULT")
DEFAULT_PRECISION = "f16x3h"          # what sta_default_config sets: the suite's DEFAULT
MIN_TAIL = 64 << 10                   # bytes of workspace behind the planned peak that the tail guard needs

# Every run() makes exactly ONE library call that takes the scratch: the planned peak the tail guard reads is that call's.
# Entry points of csrc/sta_rows.inc that take NO stream scratch and so have no row (the inventory test holds that they still do not):
NO_SCRATCH = {
    "sta_estimate_scale": "one launch on caller memory",
    "sta_pack_compact": "one launch on caller memory",
    "sta_select_patches": "two launches, the geometry travels in the kernel arguments",
    "sta_mat_to_se3": "one launch on caller memory",
    "sta_flow_pyramid": "caller-provided buffers (tests/test_flow_gpu.py runs them on filled memory)",
    "sta_flow_corners": "caller-provided workspace (tests/test_flow_gpu.py runs it on filled memory)",
    "sta_flow_track": "caller-provided buffers (tests/test_flow_gpu.py runs them on filled memory)",
}
# product entry points that reach plan_and_run without ever launching on the scratch: named here with the reason
EXEMPT = {
    "sta_reserve": "runs the planning pass of other entry points (reserve_only) and allocates; launches nothing",
}


class Case(NamedTuple):
    name: str
    entries: Tuple[str, ...]
    family: str
    rank: int
    make: Callable
    run: Callable
    shapes: str
    no_prec: Tuple[str, ...] = ()


H0, W0 = 32, 48          # 2 x 3 patches


def _imgs(n, H, W, tag=0):
    import torch
    from vista_slam_amd import weights as Wt
    return torch.from_numpy(Wt.synth_images(n, H, W, seed=43, tag=tag)).cuda()


def _imgs_u8(n, H, W, tag=0):
    import torch
    from vista_slam_amd import weights as Wt
    return torch.from_numpy(Wt.synth_images_u8(n, H, W, seed=43, tag=tag)).cuda()


def _named(prefix, lists):
    """[(name, tensor)] of nested lists of tensors / None."""
    out = []

    def walk(p, v):
        if v is None:
            return
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{p}[{i}]", x)
        elif isinstance(v, dict):
            for k in sorted(v):
                walk(f"{p}.{k}", v[k])
        else:
            out.append((p, v))
    walk(prefix, lists)
    return out


def _feats(m, B=2, H=H0, W=W0, tag=0):
    """Encoder features + grid positions of B synthetic frames: decoder / head / scheduler inputs, in caller memory."""
    f, p = m._encode_image(_imgs(B, H, W, tag), None, normalize=False)
    return f.clone(), p


# ------------------------------------------------------------------------------------------ encoder routes
def _mk_encode(m):
    return {"img": _imgs(2, H0, W0)}


def _run_encode(m, x, between=None):
    return [("feat", m._encode_image(x["img"], None, normalize=False)[0])]


def _mk_encode_u8(m):
    return {"img": _imgs_u8(2, H0, W0)}


def _run_encode_u8(m, x, between=None):
    return [("feat", m.encode_u8hwc(x["img"])[0])]


def _tok_index():
    import torch
    return torch.tensor([[0, 1, 2, 4, 5], [5, 3, 2, 1, 0]], dtype=torch.int64)      # 5 of 6 tokens, each entry its own


def _mk_encode_tokens(m):
    return {"img": _imgs(2, H0, W0), "u8": _imgs_u8(2, H0, W0), "index": _tok_index()}


def _run_encode_tokens(m, x, between=None):
    return [("feat", m.encode_tokens(x["img"], index=x["index"])[0])]


def _run_encode_tokens_u8(m, x, between=None):
    return [("feat", m.encode_tokens_u8hwc(x["u8"], index=x["index"])[0])]


VARLEN_FRAMES = ((32, 48), (48, 32), (32, 32))          # three frame sizes
VARLEN_INDEX = ((0, 2, 3, 5), (5, 4, 3, 2, 1, 0), (3,))   # 4 / 6 / 1 tokens


def _mk_encode_varlen(m):
    import torch
    return {"imgs": [_imgs(1, h, w, tag=b)[0] for b, (h, w) in enumerate(VARLEN_FRAMES)],
            "u8": [_imgs_u8(1, h, w, tag=b)[0] for b, (h, w) in enumerate(VARLEN_FRAMES)],
            "index": [torch.tensor(ix, dtype=torch.int64) for ix in VARLEN_INDEX]}


def _with_option(m, idx, value, fn):
    from vista_slam_amd import _lib
    _lib.check(m.lib.sta_debug_set_option(m._h, idx, value))
    try:
        return fn()
    finally:
        _lib.check(m.lib.sta_debug_set_option(m._h, idx, 0))


def _run_encode_varlen(opt8, u8=False):
    def run(m, x, between=None):
        call = (lambda: m.encode_tokens_varlen_u8hwc(x["u8"], index=x["index"])) if u8 else (lambda: m.encode_tokens_varlen(x["imgs"], index=x["index"]))
        feats, _pos = _with_option(m, 8, opt8, call)
        return _named("feat", list(feats))
    return run


# ------------------------------------------------------------------------------------------ decoder routes
def _mk_decode(m):
    fa, pa = _feats(m, 2, tag=0)
    fb, pb = _feats(m, 2, tag=1)
    return {"fa": fa, "fb": fb, "pa": pa, "pb": pb}


def _run_decode(m, x, between=None):
    d1, d2 = m._decode_stereo(x["fa"], x["fb"], x["pa"], x["pb"])
    return _named("dec1", d1) + _named("dec2", d2)


def _mk_decode_pos(m):
    x = _mk_decode(m)
    x["p1"] = (x["pa"].clone() + x["pa"].new_tensor([1, 2])).contiguous()      # shifted
    x["p2"] = x["pb"].clone().flip(1).contiguous()                             # reversed
    return x


def _run_decode_pos(m, x, between=None):
    d1, d2 = m._decode_stereo(x["fa"], x["fb"], x["p1"], x["p2"])
    return _named("dec1", d1) + _named("dec2", d2)


def _mk_decode_mixed(m):
    fa, pa = _feats(m, 2, H0, W0, tag=0)              # 6 tokens
    fb, pb = m._encode_image(_imgs(2, 32, 16, 1), None, normalize=False)      # 2 tokens
    return {"fa": fa, "fb": fb.clone(), "pa": pa, "pb": pb}


def _run_decode_mixed(m, x, between=None):
    d1, d2 = m.decode_stereo_mixed(x["fa"], x["fb"], x["pa"], x["pb"])
    return _named("dec1", d1) + _named("dec2", d2)


def _mk_decode_tokens(m):
    x = _mk_decode(m)
    f1, p1 = m.select_tokens(x["fa"], x["pa"], [0, 1, 2, 4, 5])               # 5 against 2
    f2, p2 = m.select_tokens(x["fb"], x["pb"], [3, 1])
    return {"f1": f1, "p1": p1, "f2": f2, "p2": p2}


def _run_decode_tokens(m, x, between=None):
    d1, d2 = m.decode_stereo_tokens(x["f1"], x["f2"], x["p1"], x["p2"])
    return _named("dec1", d1) + _named("dec2", d2)


DECV_COUNTS = ((4, 3), (6, 2), (1, 5))


def _mk_decode_varlen(m):
    import torch
    fa, pa = _feats(m, 3, tag=0)
    fb, pb = _feats(m, 3, tag=1)
    pick = lambda n, b: torch.tensor([(5 * b + 1 + 5 * i) % 6 for i in range(n)], device=fa.device)      # n distinct tokens of 6 (5 is coprime to 6)
    f1, q1, f2, q2 = [], [], [], []
    for b, (n1, n2) in enumerate(DECV_COUNTS):
        i1, i2 = pick(n1, b), pick(n2, b + 1)
        f1.append(fa[b][i1].contiguous()); q1.append(pa[b][i1].contiguous())
        f2.append(fb[b][i2].contiguous()); q2.append(pb[b][i2].contiguous())
    return {"f1": f1, "q1": q1, "f2": f2, "q2": q2}


def _run_decode_varlen(m, x, between=None):
    d1, d2 = m.decode_stereo_varlen(x["f1"], x["f2"], x["q1"], x["q2"])
    return _named("dec1", d1) + _named("dec2", d2)


# ------------------------------------------------------------------------------------------ forward_pair
def _mk_pair(B, H, W):
    def make(m):
        return {"a": _imgs(B, H, W, 0), "b": _imgs(B, H, W, 1), "a8": _imgs_u8(B, H, W, 0), "b8": _imgs_u8(B, H, W, 1)}
    return make


def _run_pair(lanes="auto", u8=False):
    def run(m, x, between=None):
        m.set_side_lanes(lanes)
        try:
            main, supp = m.forward_pair_u8hwc(x["a8"], x["b8"]) if u8 else m.forward_pair(x["a"], x["b"])
        finally:
            m.set_side_lanes("auto")
        return _named("main", main) + _named("supp", supp)
    return run


# ------------------------------------------------------------------------------------------ heads
def _mk_heads(m):
    x = _mk_decode(m)
    d1, _d2 = m._decode_stereo(x["fa"], x["fb"], x["pa"], x["pb"])
    return {"fa": x["fa"], "dec": [t.clone() for t in d1]}


def _run_head_pose(m, x, between=None):
    return _named("pose", m.head_pose_s(x["dec"][-1][:, 0, :]))


def _run_head_pts(m, x, between=None):
    return _named("pts", m.head_pts([x["fa"]] + [t[:, 1:, :] for t in x["dec"]], [[H0, W0]] * x["fa"].shape[0]))


HEADV_RECTS = ((2, 3), (1, 2), (2, 1))       # a whole 2 x 3 frame, a 1 x 2 window, a portrait 2 x 1 window


def _run_head_pts_varlen(m, x, between=None):
    hooks = m.cfg.hooks
    src = (0, 1, 1)                           # batch entry the rows of each rectangle are taken from
    feats = [x["fa"][b][:h * w].contiguous() for b, (h, w) in zip(src, HEADV_RECTS)]
    hk = [[x["dec"][i - 1][b][1:1 + h * w].contiguous() for b, (h, w) in zip(src, HEADV_RECTS)] for i in hooks[1:]]
    return _named("head", m.head_pts_varlen(feats, hk, HEADV_RECTS))


# ------------------------------------------------------------------------------------------ schedulers
def _edge_outputs(res):
    import torch
    out = []
    for e, r in enumerate(res):
        out += [(f"edge{e}.pose", r.pose), (f"edge{e}.rel_pose_conf", torch.tensor([r.rel_pose_conf])), (f"edge{e}.accepted", torch.tensor([int(r.accepted)]))]
        out += _named(f"edge{e}.confs", r.confs) + _named(f"edge{e}.intri", r.intri) + _named(f"edge{e}.depths", r.depths) + _named(f"edge{e}.pts3d", r.pts3d)
    return out


def _mk_sched(m):
    f, _p = _feats(m, 3, tag=0)
    return {"fi": f[0:1].contiguous(), "fj": [f[1:2].contiguous(), f[2:3].contiguous()], "adjacent": [True, False]}


RV_THRES = 0.0       # every edge is accepted: phase B runs both heads


def _run_rv_split(m, x, between=None):
    from vista_slam_amd import slam_scheduler as S
    p = S.regress_views_begin(m, x["fi"], x["fj"], H0, W0)
    try:
        if between is not None:
            between()
        return _edge_outputs(S.regress_views_finish(m, p, x["adjacent"], RV_THRES))
    finally:
        p.close()


def _run_rv(m, x, between=None):
    """sta_regress_views itself (the one-call form), on the buffers the split wrappers allocate."""
    import ctypes as C
    import torch
    from vista_slam_amd import _lib
    from vista_slam_amd.slam_scheduler import EdgeResult
    k, dev = len(x["fj"]), m.device
    pose = torch.empty(k, 4, 4, device=dev)
    pts, conf = torch.empty(k, 2, H0, W0, 3, device=dev), torch.empty(k, 2, H0, W0, device=dev)
    K, depth = torch.empty(k, 3, 3, device=dev), torch.empty(k, 2, H0, W0, device=dev)
    pconf, slot, nacc = (C.c_float * k)(), (C.c_int * k)(), C.c_int(0)
    ptrs = (C.c_void_p * k)(*[f.data_ptr() for f in x["fj"]])
    adj = bytes(bytearray(1 if a else 0 for a in x["adjacent"]))
    _lib.check(m.lib.sta_regress_views(m._h, x["fi"].data_ptr(), ptrs, k, adj, RV_THRES, H0, W0, pose.data_ptr(), pconf, slot, C.byref(nacc),
                                       pts.data_ptr(), conf.data_ptr(), K.data_ptr(), depth.data_ptr(), m._stream()))
    res = [EdgeResult(pose[e], float(pconf[e]), False) if slot[e] < 0 else
           EdgeResult(pose[e], float(pconf[e]), True, conf[slot[e]], K[slot[e]], depth[slot[e]], pts[slot[e]]) for e in range(k)]
    return _edge_outputs(res)


def _mk_sched_tokens(m):
    import torch
    x = _mk_sched(m)
    x["sel_i"] = [(0, 1, 2, 2), (0, 0, 1, 3)]                                       # window sides
    x["sel_j"] = [torch.tensor([4, 0, 5], dtype=torch.int64), (1, 0, 1, 2)]         # an index-list side, a window side
    return x


def _run_rvt_split(heads):
    def run(m, x, between=None):
        from vista_slam_amd import slam_scheduler as S
        p = S.regress_views_tokens_begin(m, x["fi"], (H0, W0), x["fj"], [(H0, W0)] * 2, x["sel_i"], x["sel_j"], heads=heads)
        try:
            if between is not None:
                between()
            return _edge_outputs(S.regress_views_tokens_finish(m, p, x["adjacent"], RV_THRES))
        finally:
            p.close()
    return run


def _run_rvt(heads):
    """sta_regress_views_tokens itself (the one-call form), packed as the split wrappers pack it."""
    def run(m, x, between=None):
        import ctypes as C
        import torch
        from vista_slam_amd import _lib
        from vista_slam_amd import slam_scheduler as S
        k, dev, hp, wp = 2, m.device, H0 // 16, W0 // 16
        si = [S._selection(s, hp, wp) for s in x["sel_i"]]
        sj = [S._selection(s, hp, wp) for s in x["sel_j"]]
        win_i, cnt_i, idx_i = S._pack_side(si, dev)
        win_j, cnt_j, idx_j = S._pack_side(sj, dev)
        pix = sum(256 * w[2] * w[3] for e in range(k) for w, ix in (si[e], sj[e]) if ix is None)
        pose, Kk = torch.empty(k, 4, 4, device=dev), torch.empty(k, 3, 3, device=dev)
        # (zeros: the ranges of index-list sides and of rejected edges stay unwritten by contract)
        pts, conf, depth = torch.zeros(pix, 3, device=dev), torch.zeros(pix, device=dev), torch.zeros(pix, device=dev)
        pconf, acc, kval, nacc = (C.c_float * k)(), (C.c_int * k)(), (C.c_int * k)(), C.c_int(0)
        ptrs = (C.c_void_p * k)(*[f.data_ptr() for f in x["fj"]])
        HW = (C.c_int * k)(*[H0] * k), (C.c_int * k)(*[W0] * k)
        adj = bytes(bytearray(1 if a else 0 for a in x["adjacent"]))
        prev = m.set_varlen_heads(heads == "varlen")
        try:
            _lib.check(m.lib.sta_regress_views_tokens(m._h, x["fi"].data_ptr(), H0, W0, ptrs, HW[0], HW[1], k, win_i, cnt_i,
                                                      None if idx_i is None else idx_i.data_ptr(), win_j, cnt_j, None if idx_j is None else idx_j.data_ptr(),
                                                      adj, RV_THRES, pose.data_ptr(), pconf, acc, C.byref(nacc), pts.data_ptr(), conf.data_ptr(),
                                                      depth.data_ptr(), Kk.data_ptr(), kval, m._stream()))
        finally:
            m.set_varlen_heads(prev)
        return [("pose", pose), ("pose_conf", torch.tensor(list(pconf))), ("accepted", torch.tensor(list(acc))), ("k_valid", torch.tensor(list(kval))),
                ("pts", pts), ("conf", conf), ("depth", depth)] + [(f"K[{e}]", Kk[e]) for e in range(k) if kval[e]]
    return run


# ------------------------------------------------------------------------------------------ sta_rows.inc
def _mk_preprocess(m):
    import numpy as np
    import torch
    rng = np.random.default_rng(7)
    return {"rgb": torch.from_numpy(rng.integers(0, 256, size=(100, 140, 3), dtype=np.uint8)).cuda()}


def _run_preprocess(m, x, between=None):
    from vista_slam_amd.preprocess import process_image
    return _named("frame", process_image(m, x["rgb"], (64, 48)))


def _mk_intrinsics(m):
    import numpy as np
    import torch
    rng = np.random.default_rng(9)
    B, H, W = 2, 24, 40
    v, u = np.mgrid[0:H, 0:W]
    z = 2.0 + rng.random((B, H, W))
    pts = np.stack([(u - W / 2) / 30.0 * z, (v - H / 2) / 30.0 * z, z], -1).astype(np.float32)
    return {"pts": torch.from_numpy(pts).cuda(), "conf": torch.from_numpy((1.0 + rng.random((B, H, W))).astype(np.float32)).cuda()}


def _run_intrinsics(shared):
    def run(m, x, between=None):
        from vista_slam_amd import post
        return _named("K_depth_confmean", list(post.pair_reductions(m, x["pts"], x["conf"], shared)))
    return run


def _mk_cloud(m):
    import torch
    import voxel_cases as V
    depths, scales, K, poses, confs, imgs, thres = V.wall_scene()
    return {"args": [torch.from_numpy(a).cuda() for a in (depths, scales, K, poses, confs, imgs)], "thres": thres}


def _run_cloud(m, x, between=None):
    from vista_slam_amd import formats
    return _named("cloud", list(formats.world_pointcloud(m, *x["args"], x["thres"])))


def _mk_voxel(m):
    import torch
    import voxel_cases as V
    c = V.build("min_points_2")
    return {"pts": torch.from_numpy(c["pts"]).cuda(), "col": torch.from_numpy(c["col"]).cuda(), "voxel_size": c["voxel_size"]}


def _run_voxel(m, x, between=None):
    from vista_slam_amd import formats
    return _named("voxel", list(formats.voxel_downsample(m, x["pts"], x["col"], voxel_size=x["voxel_size"], min_points=2, return_counts=True,
                                                         return_index=True, return_inverse=True)))


def _mk_votes(m):
    import torch
    import geo_cases as G
    return {"a": [torch.from_numpy(a).cuda() for a in G.scene(3, 48, 64, seed=5)]}


def _run_votes(m, x, between=None):
    from vista_slam_amd import geo
    return [("count", geo.view_consistency_check(m, *x["a"], window=4))]


def _mk_sym(m):
    import torch
    import geo_cases as G
    return {"a": [torch.from_numpy(a).cuda() for a in G.sym_case_inputs("geo_sym_48x64_p3")]}


def _run_sym(m, x, between=None):
    from vista_slam_amd import geo
    return _named("sym", list(geo.symmetric_geo_valid_masks(m, *x["a"], return_thres=True)))


def _mk_quantile(m):
    import torch
    import geo_q_cases as Q
    a = Q.q_case_inputs("geo_q_40x56_b3")
    return {"a": [torch.from_numpy(t).cuda() for t in a[:6]], "q": float(a[6])}


def _run_quantile(m, x, between=None):
    from vista_slam_amd import geo
    return _named("q", list(geo.geo_valid_masks(m, *x["a"], x["q"], return_thres=True)))


def _mk_ray(m):
    import torch
    import geo_cases as G
    from vista_slam_amd import geo
    depth, Ks, _Ts = G.scene(3, 40, 56, seed=11)
    x = {"depth": torch.from_numpy(depth).cuda(), "K": torch.from_numpy(Ks).cuda()}
    x["pc"] = geo.compute_local_pointclouds(m, x["depth"], x["K"]).clone()
    return x


def _run_local_points(shared):
    def run(m, x, between=None):
        from vista_slam_amd import geo
        return [("points", geo.compute_local_pointclouds(m, x["depth"], x["K"][0] if shared else x["K"]))]
    return run


def _run_ray_depth(shared):
    def run(m, x, between=None):
        from vista_slam_amd import geo
        return [("ray_depth", geo.depth_from_pointcloud_dot_batched(m, x["pc"], x["K"][0] if shared else x["K"]))]
    return run


CASES = [
    Case("encode", ("sta_encode",), "enc", 3, _mk_encode, _run_encode, "B 2, 32x48"),
    Case("encode_u8hwc", ("sta_encode_u8hwc",), "enc", 3, _mk_encode_u8, _run_encode_u8, "B 2, 32x48 uint8 HWC"),
    Case("encode_tokens", ("sta_encode_tokens",), "enc", 2, _mk_encode_tokens, _run_encode_tokens, "B 2, 5 of 6 tokens"),
    Case("encode_tokens_u8hwc", ("sta_encode_tokens_u8hwc",), "enc", 2, _mk_encode_tokens, _run_encode_tokens_u8, "B 2, 5 of 6 tokens, uint8 HWC"),
    Case("encode_varlen", ("sta_encode_varlen",), "enc", 4, _mk_encode_varlen, _run_encode_varlen(0), "4 / 6 / 1 tokens of 32x48, 48x32, 32x32"),
    Case("encode_varlen_opt8", ("sta_encode_varlen",), "enc", 4, _mk_encode_varlen, _run_encode_varlen(1), "the same, experiment switch 8 on"),
    Case("encode_varlen_u8hwc", ("sta_encode_varlen_u8hwc",), "enc", 4, _mk_encode_varlen, _run_encode_varlen(0, True), "the same, uint8 HWC"),
    Case("decode", ("sta_decode",), "dec", 4, _mk_decode, _run_decode, "B 2, 6 tokens"),
    Case("decode_pos", ("sta_decode_pos",), "dec", 4, _mk_decode_pos, _run_decode_pos, "B 2, 6 tokens, shifted and reversed positions"),
    Case("decode_mixed", ("sta_decode_mixed",), "dec", 2, _mk_decode_mixed, _run_decode_mixed, "B 2, 6 against 2 tokens"),
    Case("decode_tokens", ("sta_decode_tokens",), "dec", 1, _mk_decode_tokens, _run_decode_tokens, "B 2, 5 against 2 tokens"),
    Case("decode_varlen", ("sta_decode_varlen",), "dec", 5, _mk_decode_varlen, _run_decode_varlen, "4|3, 6|2, 1|5 tokens"),
    Case("forward_pair", ("sta_forward_pair",), "pair", 1, _mk_pair(1, 32, 48), _run_pair(), "B 1, 32x48"),
    Case("forward_pair_u8hwc", ("sta_forward_pair_u8hwc",), "pair", 1, _mk_pair(1, 32, 48), _run_pair(u8=True), "B 1, 32x48 uint8 HWC"),
    Case("forward_pair_lanes", ("sta_forward_pair",), "pair", 2, _mk_pair(2, 64, 96), _run_pair("on"), "B 2, 64x96, side lanes on"),
    Case("head_pose", ("sta_head_pose",), "head", 1, _mk_heads, _run_head_pose, "B 2"),
    Case("head_pts", ("sta_head_pts",), "head", 3, _mk_heads, _run_head_pts, "B 2, 32x48"),
    Case("head_pts_varlen", ("sta_head_pts_varlen",), "head", 2, _mk_heads, _run_head_pts_varlen, "2x3, 1x2, 2x1 patches", ("f16",)),
    Case("regress_views", ("sta_regress_views",), "sched", 4, _mk_sched, _run_rv, "2 edges, 32x48"),
    Case("regress_views_split", ("sta_regress_views_begin", "sta_regress_views_finish"), "sched", 4, _mk_sched, _run_rv_split, "2 edges, 32x48, split phases"),
    Case("regress_views_tokens", ("sta_regress_views_tokens",), "sched", 1, _mk_sched_tokens, _run_rvt("entry"), "2 edges: window | index list, window | window"),
    Case("regress_views_tokens_varlen", ("sta_regress_views_tokens",), "sched", 2, _mk_sched_tokens, _run_rvt("varlen"), "the same, varlen heads", ("f16",)),
    Case("regress_views_tokens_split", ("sta_regress_views_tokens_begin", "sta_regress_views_tokens_finish"), "sched", 1, _mk_sched_tokens,
         _run_rvt_split("entry"), "the same, split phases"),
    Case("preprocess_frame", ("sta_preprocess_frame",), "rows", 1, _mk_preprocess, _run_preprocess, "100x140 -> 64x48"),
    Case("estimate_intrinsics", ("sta_estimate_intrinsics",), "rows", 1, _mk_intrinsics, _run_intrinsics(False), "B 2, 24x40, K per view"),
    Case("estimate_intrinsics_shared", ("sta_estimate_intrinsics",), "rows", 1, _mk_intrinsics, _run_intrinsics(True), "B 2, 24x40, one K for the pair"),
    Case("world_pointcloud", ("sta_world_pointcloud",), "rows", 1, _mk_cloud, _run_cloud, "6 views of 48x64"),
    Case("voxel_downsample", ("sta_voxel_downsample",), "rows", 1, _mk_voxel, _run_voxel, "voxel_cases min_points_2"),
    Case("view_consistency", ("sta_view_consistency",), "rows", 1, _mk_votes, _run_votes, "3 views of 48x64, window 4"),
    Case("symmetric_geo_mask", ("sta_symmetric_geo_mask",), "rows", 1, _mk_sym, _run_sym, "3 pairs of 48x64"),
    Case("geo_valid_mask", ("sta_geo_valid_mask",), "rows", 1, _mk_quantile, _run_quantile, "3 pairs of 40x56, q 0.8"),
    Case("local_pointclouds", ("sta_local_pointclouds",), "rows", 1, _mk_ray, _run_local_points(False), "3 views of 40x56, K per view"),
    Case("local_pointclouds_shared", ("sta_local_pointclouds",), "rows", 1, _mk_ray, _run_local_points(True), "3 views of 40x56, one K"),
    Case("ray_depth", ("sta_ray_depth",), "rows", 1, _mk_ray, _run_ray_depth(False), "3 views of 40x56, K per view"),
    Case("ray_depth_shared", ("sta_ray_depth",), "rows", 1, _mk_ray, _run_ray_depth(True), "3 views of 40x56, one K"),
]
SPLIT_PHASE = ("regress_views_split", "regress_views_tokens_split")      # the fill hook must refuse between their two phases
TRANSITION_FAMILIES = ("enc", "dec", "pair", "sched")


def by_name(name):
    return next(c for c in CASES if c.name == name)


def named_entries():
    return {e for c in CASES for e in c.entries}


def runs():
    """(case name, precision) of every run of the matrix."""
    return [(c.name, p) for c in CASES for p in PRECISIONS if p not in c.no_prec]


def family_extremes(family):
    """(largest, smallest) case of a family by rank; ties go to the first row."""
    rows = [c for c in CASES if c.family == family]
    return max(rows, key=lambda c: c.rank), min(rows, key=lambda c: c.rank)
