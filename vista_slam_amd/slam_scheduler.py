"""Keyframe scheduler behind the reference's `regress_two_views` contract.

`OnlineSLAM.step` (vista_slam/slam.py:263-277) connects a new keyframe i to its <= neighbor_edge_num previous views
and <= loop_edge_num loop candidates by calling `regress_two_views(i, j)` (slam.py:153-189) once per edge: a B=1
decode, the pose head, an early return for low-confidence non-adjacent edges, then two DPT heads, the shared
intrinsics and the depths.  `regress_views` does the same for all candidate edges in one native call
(`sta_regress_views`, include/sta_mi355.h): one batched decode, pose heads first, one D2H read of the k
confidences, DPT + reductions only for the accepted edges.  `regress_views_tokens` is the same contract with a SELECTION per
edge and side (the whole frame, a window of patches, an index list) and a frame size per candidate
(`sta_regress_views_tokens`): one varlen decode of the k sliced pairs.  All arithmetic runs in libsta_mi355.so.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .sta_frontend import STAFrontend, _stream_ptr


class EdgeResult:
    """What `regress_two_views` returns for one edge (slam.py:170,189): the relative pose (4x4; the reference converts
    it with pp.mat2SE3, see `formats.mat_to_se3`), its confidence, and - for accepted edges - confs [2,H,W],
    intri [3,3], depths [2,H,W] (+ the full point maps, which the reference discards after the reductions)."""
    __slots__ = ("pose", "rel_pose_conf", "accepted", "confs", "intri", "depths", "pts3d")

    def __init__(self, pose, rel_pose_conf, accepted, confs=None, intri=None, depths=None, pts3d=None):
        self.pose, self.rel_pose_conf, self.accepted = pose, rel_pose_conf, accepted
        self.confs, self.intri, self.depths, self.pts3d = confs, intri, depths, pts3d

    def as_reference_tuple(self):
        """(pose_ij 4x4, rel_pose_conf_ij, confs, intri, depths) with None for rejected edges (slam.py:170)."""
        return self.pose, self.rel_pose_conf, self.confs, self.intri, self.depths


class PendingEdges:
    """A scheduler call between its two phases (sta_regress_views_begin / _finish): the output tensors, the inputs kept
    alive, and the stream the call lives on.  While it is open its stream's scratch context inside the library is reserved;
    `regress_views_finish` closes it, and so does `close()` / leaving a `with` block (an exception between the phases must not
    leave the stream unusable: sta_regress_views_abort).  Close it EXPLICITLY: `__del__` is only a best-effort fallback and acts
    only on the thread that created the object - the abort may block in hipEventSynchronize and the handle is not thread-safe,
    so a garbage collection that happens to run on another thread must not enter the library."""
    __slots__ = ("k", "H", "W", "stream", "pose", "pts", "conf", "K", "depth", "_keep", "_frontend", "_open", "_tid", "maps", "heads")

    def close(self):
        """Abort the call if it is still pending (idempotent)."""
        if getattr(self, "_open", False):
            self._open = False
            fe = self._frontend
            if getattr(fe, "_h", None):
                fe.lib.sta_regress_views_abort(fe._h, self.stream)

    def __enter__(self):
        return self

    def __exit__(self, *_exc):
        self.close()
        return False

    def __del__(self):
        try:
            if getattr(self, "_tid", None) == threading.get_ident():
                self.close()
        except Exception:
            pass


def regress_views_begin(frontend: STAFrontend, enc_feat_i: torch.Tensor, enc_feats_j: Sequence[torch.Tensor], H: int, W: int) -> PendingEdges:
    """Phase 1 of `regress_views` on the CURRENT stream: gather + batched decode + pose heads, no host synchronisation.
    Until `regress_views_finish` no other frontend call may run on this stream (calls on other streams are fine)."""
    k = len(enc_feats_j)
    assert 1 <= k <= 16
    frontend._check_hw(H, W)
    dev = frontend.device
    N, E = (H // 16) * (W // 16), frontend.cfg.enc_embed_dim
    fi = enc_feat_i.to(dev, torch.float32).contiguous()
    fj = [f.to(dev, torch.float32).contiguous() for f in enc_feats_j]
    for f in [fi] + fj:
        assert f.numel() == N * E, f"encoder feature has {f.numel()} elements, expected {N}x{E}"
    ptrs = (C.c_void_p * k)(*[f.data_ptr() for f in fj])
    p = PendingEdges()
    p.k, p.H, p.W, p.stream = k, H, W, frontend._stream()
    p.pose = torch.empty(k, 4, 4, device=dev, dtype=torch.float32)
    p.pts = torch.empty(k, 2, H, W, 3, device=dev, dtype=torch.float32)
    p.conf = torch.empty(k, 2, H, W, device=dev, dtype=torch.float32)
    p.K = torch.empty(k, 3, 3, device=dev, dtype=torch.float32)
    p.depth = torch.empty(k, 2, H, W, device=dev, dtype=torch.float32)
    p._keep = (fi, fj)
    p._frontend, p._open, p._tid = frontend, False, threading.get_ident()
    _lib.check(frontend.lib.sta_regress_views_begin(frontend._h, fi.data_ptr(), ptrs, k, H, W, p.pose.data_ptr(), p.stream))
    p._open = True
    return p


def regress_views_finish(frontend: STAFrontend, p: PendingEdges, adjacent: Sequence[bool], rel_pose_thres: float) -> List[EdgeResult]:
    """Phase 2: waits for the k pose confidences, accepts / rejects (slam.py:169), enqueues the DPT heads + reductions of the
    accepted edges on the stream `regress_views_begin` ran on."""
    k, H, W = p.k, p.H, p.W
    assert k == len(adjacent)
    adj = bytes(bytearray(1 if a else 0 for a in adjacent))
    pconf = (C.c_float * k)()
    slot = (C.c_int * k)()
    nacc = C.c_int(0)
    assert p._open, "this scheduler call was already finished or aborted"
    p._open = False
    rc = frontend.lib.sta_regress_views_finish(frontend._h, adj, float(rel_pose_thres), pconf, slot, C.byref(nacc),
                                               p.pts.data_ptr(), p.conf.data_ptr(), p.K.data_ptr(), p.depth.data_ptr(), p.stream)
    if rc != 0:
        # a failure BEFORE the C side cleared its pending flag (an argument check, a context lookup) would leave the stream
        # reserved until sta_destroy: abort unconditionally - idempotent, 0 when nothing is pending - and keep the first error
        msg = frontend.lib.sta_last_error()
        frontend.lib.sta_regress_views_abort(frontend._h, p.stream)
        raise _lib.StaError(msg.decode() if isinstance(msg, bytes) else str(msg))
    pts, conf, depth = p.pts, p.conf, p.depth
    if H > W:     # portrait: the reference sees transposed views of the same memory (utils/misc.py:60-61,81)
        pts, conf, depth = pts.swapaxes(2, 3), conf.swapaxes(2, 3), depth.swapaxes(2, 3)
    out = []
    for e in range(k):
        s = slot[e]
        if s < 0:
            out.append(EdgeResult(p.pose[e], float(pconf[e]), False))
        else:
            out.append(EdgeResult(p.pose[e], float(pconf[e]), True, conf[s], p.K[s], depth[s], pts[s]))
    return out


def regress_views(frontend: STAFrontend, enc_feat_i: torch.Tensor, enc_feats_j: Sequence[torch.Tensor],
                  adjacent: Sequence[bool], rel_pose_thres: float, H: int, W: int) -> List[EdgeResult]:
    """Edges (i, j_e), e < k, of one keyframe.  enc_feat_i / enc_feats_j[e]: [1,N,1024] encoder features as cached
    by `add_view` (slam.py:142-151).  adjacent[e] = (i - j_e == 1).  Synchronises once, on the k pose confidences."""
    assert len(enc_feats_j) == len(adjacent)
    return regress_views_finish(frontend, regress_views_begin(frontend, enc_feat_i, enc_feats_j, H, W), adjacent, rel_pose_thres)


# ------------------------------------------------------------------------------------------ the scheduler on token subsets
def _selection(sel, hp: int, wp: int):
    """One side's selection on a frame of hp x wp patches -> ((y0, x0, h, w), None) for a window (None = the whole frame) or
    ((0, 0, 0, 0), index tensor) for an index list.  Refuses what `encode_tokens` refuses."""
    if sel is None:
        return (0, 0, hp, wp), None
    if isinstance(sel, (tuple, list)) and not isinstance(sel, torch.Tensor):
        assert len(sel) == 4, f"a window is (y0, x0, h, w) in patches (got {sel!r})"
        y0, x0, h, w = (int(v) for v in sel)
        if h < 1 or w < 1:
            raise ValueError(f"empty window {(y0, x0, h, w)}")
        if y0 < 0 or x0 < 0 or y0 + h > hp or x0 + w > wp:
            raise ValueError(f"window {(y0, x0, h, w)} leaves the {hp} x {wp} patch grid")
        return (y0, x0, h, w), None
    index = torch.as_tensor(sel)
    assert index.dtype == torch.int64, f"index must be int64 (got {index.dtype})"
    assert index.dim() == 1, f"index must be [n] (got {tuple(index.shape)})"
    if index.numel() < 1:
        raise ValueError("empty selection: an index list has at least one token")
    lo, hi = int(index.min()), int(index.max())
    if lo < 0 or hi >= hp * wp:
        raise ValueError(f"token index outside the {hp} x {wp} patch grid (range [{lo}, {hi}])")
    return (0, 0, 0, 0), index


def _pack_side(sels, dev):
    """[(window, index)] over the k edges of one side -> (int[k][4] windows, int[k] counts, packed device int64 indices or None)."""
    k = len(sels)
    win = (C.c_int * (4 * k))(*[v for w, _ in sels for v in w])
    cnt = (C.c_int * k)(*[0 if ix is None else int(ix.numel()) for _, ix in sels])
    lists = [ix.to(dev) for _, ix in sels if ix is not None]
    return win, cnt, (torch.cat(lists).contiguous() if lists else None)


def _heads_on(frontend: STAFrontend, heads):
    """heads keyword -> the switch value for one call: None = whatever `set_varlen_heads` left on the handle."""
    if heads is None:
        return getattr(frontend, "_varlen_heads", False)
    if heads not in ("entry", "varlen"):
        raise ValueError(f'heads must be "entry" or "varlen" (got {heads!r})')
    return heads == "varlen"


def regress_views_tokens_begin(frontend: STAFrontend, enc_feat_i: torch.Tensor, size_i: Tuple[int, int], enc_feats_j: Sequence[torch.Tensor],
                               sizes_j: Sequence[Tuple[int, int]], sel_i: Sequence, sel_j: Sequence, heads: str | None = None) -> PendingEdges:
    """Phase 1 of `regress_views_tokens` on the CURRENT stream: slice + varlen decode + pose heads, no host synchronisation (index
    lists given on the CPU are checked there and copied).  Until `regress_views_tokens_finish` no other frontend call may run on this
    stream.  The returned `PendingEdges` closes like the one of `regress_views_begin`.  heads: "entry" | "varlen" | None (the handle's
    `set_varlen_heads` setting) - the call's workspace is planned HERE, so a finish with heads="varlen" needs a begin with it; the
    handle's own setting is put back before this returns."""
    on = _heads_on(frontend, heads)
    k = len(enc_feats_j)
    assert 1 <= k <= 16, f"1 .. 16 candidate edges per keyframe (got {k})"
    assert len(sizes_j) == k and len(sel_i) == k and len(sel_j) == k, "one frame size and one selection per side for every edge"
    dev, E = frontend.device, frontend.cfg.enc_embed_dim
    Hi, Wi = (int(v) for v in size_i)
    frontend._check_hw(Hi, Wi)
    fi = enc_feat_i.to(dev, torch.float32).contiguous()
    assert fi.numel() == (Hi // 16) * (Wi // 16) * E, f"encoder feature of view i has {fi.numel()} elements, expected {(Hi // 16) * (Wi // 16)}x{E}"
    fj, Hj, Wj, si, sj = [], [], [], [], []
    for e in range(k):
        H, W = (int(v) for v in sizes_j[e])
        frontend._check_hw(H, W)
        f = enc_feats_j[e].to(dev, torch.float32).contiguous()
        assert f.numel() == (H // 16) * (W // 16) * E, f"encoder feature of candidate {e} has {f.numel()} elements, expected {(H // 16) * (W // 16)}x{E}"
        fj.append(f); Hj.append(H); Wj.append(W)
        si.append(_selection(sel_i[e], Hi // 16, Wi // 16))
        sj.append(_selection(sel_j[e], H // 16, W // 16))
    win_i, cnt_i, idx_i = _pack_side(si, dev)
    win_j, cnt_j, idx_j = _pack_side(sj, dev)
    # the maps of the window sides of all k edges, (edge, side) order: [(offset in pixels, 16 h, 16 w) or None] per edge and side
    maps, pix = [], 0
    for e in range(k):
        row = []
        for w, ix in (si[e], sj[e]):
            row.append(None if ix is not None else (pix, 16 * w[2], 16 * w[3]))
            pix += 0 if ix is not None else 256 * w[2] * w[3]
        maps.append(row)
    p = PendingEdges()
    p.k, p.H, p.W, p.stream, p.maps = k, Hi, Wi, frontend._stream(), maps
    p.pose = torch.empty(k, 4, 4, device=dev, dtype=torch.float32)
    p.pts = torch.empty(max(pix, 1), 3, device=dev, dtype=torch.float32)
    p.conf = torch.empty(max(pix, 1), device=dev, dtype=torch.float32)
    p.depth = torch.empty(max(pix, 1), device=dev, dtype=torch.float32)
    p.K = torch.empty(k, 3, 3, device=dev, dtype=torch.float32)
    p._keep = (fi, fj, idx_i, idx_j)
    p._frontend, p._open, p._tid = frontend, False, threading.get_ident()
    ptrs = (C.c_void_p * k)(*[f.data_ptr() for f in fj])
    p.heads = "varlen" if on else "entry"
    prev = frontend.set_varlen_heads(on)
    try:
        _lib.check(frontend.lib.sta_regress_views_tokens_begin(
            frontend._h, fi.data_ptr(), Hi, Wi, ptrs, (C.c_int * k)(*Hj), (C.c_int * k)(*Wj), k,
            win_i, cnt_i, None if idx_i is None else idx_i.data_ptr(), win_j, cnt_j, None if idx_j is None else idx_j.data_ptr(),
            p.pose.data_ptr(), p.stream))
    finally:
        frontend.set_varlen_heads(prev)
    p._open = True
    return p


def regress_views_tokens_finish(frontend: STAFrontend, p: PendingEdges, adjacent: Sequence[bool], rel_pose_thres: float,
                                heads: str | None = None) -> List[EdgeResult]:
    """Phase 2: waits for the k pose confidences, accepts / rejects (slam.py:169), enqueues the DPT heads of the accepted edges' window
    sides and their reductions.  Per edge an `EdgeResult` whose confs / depths / pts3d are 2-LISTS [side i, side j] with None for an
    index-list side ([16 h, 16 w] maps; a window with h > w comes as the transposed view the reference's head wrapper returns).  An
    edge whose two sides are windows of one (h, w) additionally gets what `regress_views` returns: confs / depths / pts3d are the
    stacked [2, ..] tensors (indexing [0] / [1] gives the sides) and intri the pair-shared K - `estimate_intrinsic_from_pts3d` of
    those two maps, so its principal point is the centre of the WINDOW's image, not of the frame.  Every other edge has intri None.
    heads="entry": the DPT head once per accepted edge and window side; heads="varlen": the window sides of ALL accepted edges through
    one varlen head pass - same decisions, same layout, ranges of rejected edges unwritten; None (default): what the begin was given.
    "varlen" needs a begin with heads="varlen" (the workspace is planned there; the library refuses otherwise); "entry" is served after
    either.  The handle's own `set_varlen_heads` setting is put back before this returns."""
    on = (p.heads == "varlen") if heads is None else _heads_on(frontend, heads)
    k = p.k
    assert k == len(adjacent)
    adj = bytes(bytearray(1 if a else 0 for a in adjacent))
    pconf, acc, kval, nacc = (C.c_float * k)(), (C.c_int * k)(), (C.c_int * k)(), C.c_int(0)
    assert p._open, "this scheduler call was already finished or aborted"
    p._open = False
    prev = frontend.set_varlen_heads(on)
    try:
        rc = frontend.lib.sta_regress_views_tokens_finish(frontend._h, adj, float(rel_pose_thres), pconf, acc, C.byref(nacc),
                                                          p.pts.data_ptr(), p.conf.data_ptr(), p.depth.data_ptr(), p.K.data_ptr(), kval, p.stream)
    finally:
        frontend.set_varlen_heads(prev)
    if rc != 0:
        msg = frontend.lib.sta_last_error()
        frontend.lib.sta_regress_views_abort(frontend._h, p.stream)
        raise _lib.StaError(msg.decode() if isinstance(msg, bytes) else str(msg))
    out = []
    for e in range(k):
        if not acc[e]:
            out.append(EdgeResult(p.pose[e], float(pconf[e]), False))
            continue
        mi, mj = p.maps[e]
        if kval[e]:      # two windows of one shape: the reference's stacked tensors
            off, H, W = mi
            pts, conf, depth = p.pts[off:off + 2 * H * W].view(2, H, W, 3), p.conf[off:off + 2 * H * W].view(2, H, W), p.depth[off:off + 2 * H * W].view(2, H, W)
            if H > W:
                pts, conf, depth = pts.swapaxes(1, 2), conf.swapaxes(1, 2), depth.swapaxes(1, 2)
            out.append(EdgeResult(p.pose[e], float(pconf[e]), True, conf, p.K[e], depth, pts))
            continue
        confs, depths, ptss = [None, None], [None, None], [None, None]
        for side, m in enumerate((mi, mj)):
            if m is None:
                continue
            off, H, W = m
            pts, conf, depth = p.pts[off:off + H * W].view(H, W, 3), p.conf[off:off + H * W].view(H, W), p.depth[off:off + H * W].view(H, W)
            if H > W:
                pts, conf, depth = pts.swapaxes(0, 1), conf.swapaxes(0, 1), depth.swapaxes(0, 1)
            confs[side], depths[side], ptss[side] = conf, depth, pts
        out.append(EdgeResult(p.pose[e], float(pconf[e]), True, confs, None, depths, ptss))
    return out


def regress_views_tokens(frontend: STAFrontend, enc_feat_i: torch.Tensor, size_i: Tuple[int, int], enc_feats_j: Sequence[torch.Tensor],
                         sizes_j: Sequence[Tuple[int, int]], sel_i: Sequence, sel_j: Sequence, adjacent: Sequence[bool],
                         rel_pose_thres: float, heads: str | None = None) -> List[EdgeResult]:
    """Edges (i, j_e), e < k <= 16, of one keyframe on TOKEN SUBSETS.  enc_feat_i: keyframe i's cached whole-frame encoding at size_i
    = (H, W); enc_feats_j[e] / sizes_j[e]: candidate e's, each with its own frame size.  sel_i[e] / sel_j[e] select the tokens of the
    two sides of edge e: None (the whole frame), a 4-tuple (y0, x0, h, w) (a window, in patches of that frame's grid, row-major) or
    an int64 tensor [n >= 1] of indices into the frame's row-major patch grid (any order, repeats allowed).  Selecting slices the
    cached encoding (`select_tokens` / `window_tokens`, the encode="frame" meaning); the positions are the tokens' (y, x) in their
    own frame.  Edge e is `regress_two_views` (slam.py:153-189) at B = 1 on the two slices; see `regress_views_tokens_finish` for
    the result and for `heads`.  ValueError: indices outside the grid, an empty selection, a window outside its grid, an unknown `heads`;
    AssertionError: dtype / shape."""
    assert len(enc_feats_j) == len(adjacent)
    _heads_on(frontend, heads)
    return regress_views_tokens_finish(frontend, regress_views_tokens_begin(frontend, enc_feat_i, size_i, enc_feats_j, sizes_j, sel_i, sel_j, heads=heads),
                                       adjacent, rel_pose_thres)
