"""Token selections from per-pixel maps: the producer of what the token routes take (`encode_tokens_varlen(index=...)`,
`decode_stereo_varlen(pos1=...)`, `regress_views_tokens(sel_i=..., sel_j=...)`).  B <= 32 maps, each of its own frame size - the
bool masks of `geo.geo_valid_masks` / `geo.symmetric_geo_valid_masks`, `geo.view_consistency_check`'s votes, the DPT head's
confidences, a caller's own segmentation - are pooled over the 16x16 patches to integer scores, a rule selects patches per entry,
and the selection comes out as ascending index lists, (y, x) lists, counts and bounding windows.  One C call
(`sta_select_patches`, csrc/select.h: two launches), no allocation by the library, no host synchronisation in the call.

The contract is integer arithmetic and written out in include/sta_mi355.h; `plan` holds every argument check and needs no GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from .sta_frontend import STAFrontend

MAX_ENTRIES = 32
MAX_PATCHES = 8192
MAX_MARGIN = 8
_DTYPES = {"bool": 0, "uint8": 0, "float32": 1}


class Plan(NamedTuple):
    """The arguments of one `sta_select_patches` call, checked: off[b] = first patch of entry b in every packed output."""
    B: int
    H: Tuple[int, ...]
    W: Tuple[int, ...]
    grids: Tuple[Tuple[int, int], ...]
    off: Tuple[int, ...]              # B + 1 values; off[B] = all patches
    dtype: int                        # 0 uint8 / bool bytes, 1 float32
    mode: int                         # 0 count, 1 fixed-point sum
    thres: float
    invert: int
    rule: int                         # 0 min_score, 1 top_k
    min_score: int
    top_k: Optional[Tuple[int, ...]]
    margin: int


def _dtype_name(dtype) -> str:
    return str(dtype).replace("torch.", "")


def plan(shapes: Sequence[Sequence[int]], dtype, *, thres=None, invert: bool = False, min_score: Optional[int] = None, top_k=None,
         margin: int = 0, addresses: Optional[Sequence[int]] = None) -> Plan:
    """Every check of a selection call, on the host: shapes = one (H, W) per map, dtype = the maps' common dtype (a torch dtype or its
    name), the rest as `select_tokens_from_maps`; addresses (optional) = the maps' base addresses.  -> `Plan`, or ValueError for what
    the C entry refuses: B outside [1, 32]; H or W below 16 or no multiple of 16; more than 8192 patches in an entry; the fixed-point
    sum (float32 without thres) with invert; top_k with a margin or outside [1, N_b]; min_score < 0; margin outside [0, 8]; a
    float32 map that is not 4-byte aligned - and for neither or both of min_score and top_k, or a thres on a byte map."""
    name = _dtype_name(dtype)
    if name not in _DTYPES:
        raise ValueError(f"maps must be bool, uint8 or float32 (got {name})")
    code = _DTYPES[name]
    B = len(shapes)
    if not 1 <= B <= MAX_ENTRIES:
        raise ValueError(f"1 .. {MAX_ENTRIES} maps per call (got {B})")
    if code == 0 and thres is not None:
        raise ValueError(f"thres applies to float32 maps; a {name} map counts its non-zero bytes")
    mode = 1 if (code == 1 and thres is None) else 0
    if mode == 1 and invert:
        raise ValueError("invert is refused with the fixed-point sum (a float32 map without thres)")
    if (min_score is None) == (top_k is None):
        raise ValueError("give exactly one of min_score and top_k")
    margin = int(margin)
    if not 0 <= margin <= MAX_MARGIN:
        raise ValueError(f"margin must lie in [0, {MAX_MARGIN}] (got {margin})")
    if min_score is not None and int(min_score) < 0:
        raise ValueError(f"min_score must be >= 0 (got {int(min_score)})")
    if top_k is not None and margin != 0:
        raise ValueError(f"margin is refused with top_k: the count would stop being known on the host (got margin = {margin})")
    Hs, Ws, grids, off = [], [], [], [0]
    for b, hw in enumerate(shapes):
        if len(hw) != 2:
            raise ValueError(f"entry {b}: a map is [H, W] (got shape {tuple(hw)})")
        H, W = int(hw[0]), int(hw[1])
        if H < 16 or W < 16 or H % 16 or W % 16:
            raise ValueError(f"entry {b}: H and W must be multiples of 16, at least 16 (got {H} x {W})")
        n = (H // 16) * (W // 16)
        if n > MAX_PATCHES:
            raise ValueError(f"entry {b}: {H} x {W} is {n} patches, above the limit of {MAX_PATCHES} per entry")
        Hs.append(H); Ws.append(W); grids.append((H // 16, W // 16)); off.append(off[-1] + n)
    ks = None
    if top_k is not None:
        ks = [int(top_k)] * B if isinstance(top_k, int) else [int(k) for k in top_k]
        if len(ks) != B:
            raise ValueError(f"top_k is one int or one int per map: {B} maps, {len(ks)} values")
        for b, k in enumerate(ks):
            n = off[b + 1] - off[b]
            if not 1 <= k <= n:
                raise ValueError(f"entry {b}: top_k must lie in [1, {n}] (got {k})")
    if addresses is not None:
        if len(addresses) != B:
            raise ValueError(f"one address per map: {B} maps, {len(addresses)} addresses")
        for b, a in enumerate(addresses):
            if code == 1 and int(a) % 4:
                raise ValueError(f"entry {b}: a float32 map must be 4-byte aligned")
    return Plan(B, tuple(Hs), tuple(Ws), tuple(grids), tuple(off), code, mode, float("nan") if thres is None else float(thres),
                int(bool(invert)), 0 if top_k is None else 1, 0 if min_score is None else int(min_score),
                None if ks is None else tuple(ks), margin)


def _map_list(frontend: STAFrontend, maps) -> List[torch.Tensor]:
    if isinstance(maps, torch.Tensor):
        if maps.dim() != 3:
            raise ValueError(f"maps must be a list of [H, W] tensors or one [B, H, W] tensor (got {maps.dtype} {tuple(maps.shape)})")
        maps = list(maps.unbind(0))
    maps = list(maps)
    for b, m in enumerate(maps):
        what = f"entry {b}: {getattr(m, 'dtype', type(m).__name__)} {tuple(getattr(m, 'shape', ()))}"
        if not isinstance(m, torch.Tensor) or m.dim() != 2:
            raise ValueError(f"a map is a [H, W] tensor ({what})")
        if _dtype_name(m.dtype) not in _DTYPES:
            raise ValueError(f"maps must be bool, uint8 or float32 ({what})")
        if m.dtype != maps[0].dtype:
            raise ValueError(f"all maps of one call share a dtype: entry 0 is {maps[0].dtype} ({what})")
        dev = frontend.device
        if m.device.type != dev.type or (dev.index is not None and m.device.index != dev.index):
            raise ValueError(f"maps live on the frontend's device {frontend.device} ({what} on {m.device})")
        if not m.is_contiguous():
            raise ValueError(f"maps must be contiguous ({what}, strides {tuple(m.stride())})")
    return maps


class Selections:
    """The result of `select_tokens_from_maps`.  Raw device tensors: `score_slots` int32 [sum N], `index_slots` int64 [sum N],
    `pos_slots` int64 [sum N, 2], `n_sel` int32 [B], `window` int32 [B, 4] (slot b starts at `plan.off[b]`; -1 behind the selected
    patches).  Per-entry views: `scores` ([hp_b, wp_b] int32), `index` ([n_b] int64, ascending), `pos` ([n_b, 2] int64 (y, x));
    host values: `counts` (n_b), `windows` ((y0, x0, h, w) in patches, (0, 0, 0, 0) for an empty selection).  Under top_k the
    counts are the arguments: `index` and `pos` read nothing from the device.  Otherwise the first access of counts / windows /
    index / pos copies the 5 B ints once and synchronises the stream; nothing more is ever read."""

    def __init__(self, plan_: Plan, score, index, pos, meta, stream):
        self.plan = plan_
        self.score_slots, self.index_slots, self.pos_slots = score, index, pos
        B = plan_.B
        self._meta = meta
        self.n_sel, self.window = meta[:B], meta[B:].view(B, 4)
        self._host = None
        self._stream = stream

    def _read(self):
        if self._host is None:
            self._host = self._meta.cpu().tolist()        # ONE copy of 5 B ints (synchronises)
        return self._host

    @property
    def scores(self) -> List[torch.Tensor]:
        off, grids = self.plan.off, self.plan.grids
        return [self.score_slots[off[b]:off[b + 1]].view(*grids[b]) for b in range(self.plan.B)]

    @property
    def counts(self) -> List[int]:
        if self.plan.top_k is not None:
            return list(self.plan.top_k)
        return self._read()[:self.plan.B]

    @property
    def windows(self) -> List[Tuple[int, int, int, int]]:
        B = self.plan.B
        w = self._read()[B:]
        return [tuple(w[4 * b:4 * b + 4]) for b in range(B)]

    @property
    def index(self) -> List[torch.Tensor]:
        off = self.plan.off
        return [self.index_slots[off[b]:off[b] + n] for b, n in enumerate(self.counts)]

    @property
    def pos(self) -> List[torch.Tensor]:
        off = self.plan.off
        return [self.pos_slots[off[b]:off[b] + n] for b, n in enumerate(self.counts)]


def select_tokens_from_maps(frontend: STAFrontend, maps, *, thres=None, invert: bool = False, min_score: Optional[int] = None, top_k=None,
                            margin: int = 0) -> Selections:
    """maps: a list of [H_b, W_b] device tensors or one [B, H, W] tensor - bool, uint8 or float32, contiguous, B <= 32, H_b and W_b
    multiples of 16, at most 8192 patches per entry.  Patch score (int32, over the patch's 256 pixels): bool / uint8 - the number of
    non-zero bytes; float32 with thres - the number of pixels with v > thres (strict; false for NaN); invert negates the pixel
    predicate; float32 without thres - the fixed-point sum of rint(clamp(v, 0, 32767) * 256) (NaN counts 0; invert refused).
    Exactly one rule: min_score = s (patch selected iff score >= s), optionally dilated by margin <= 8 patches (Chebyshev, inside
    the entry's grid); or top_k = k (one int or one per entry): exactly k patches, the largest scores, the lower index first among
    equals.  -> `Selections`.  The call never synchronises and the library allocates nothing."""
    maps = _map_list(frontend, maps)
    if not maps:
        raise ValueError(f"1 .. {MAX_ENTRIES} maps per call (got 0)")
    addresses = [m.data_ptr() for m in maps]
    p = plan([m.shape for m in maps], maps[0].dtype, thres=thres, invert=invert, min_score=min_score, top_k=top_k, margin=margin,
             addresses=addresses)
    B, total, dev = p.B, p.off[-1], frontend.device
    score = torch.empty(total, device=dev, dtype=torch.int32)
    index = torch.empty(total, device=dev, dtype=torch.int64)
    pos = torch.empty(total, 2, device=dev, dtype=torch.int64)
    meta = torch.empty(5 * B, device=dev, dtype=torch.int32)          # n_sel [B] then window [B, 4]: one buffer, one copy
    ptrs = (C.c_void_p * B)(*addresses)
    ks = None if p.top_k is None else (C.c_int * B)(*p.top_k)
    stream = frontend._stream()
    _lib.check(frontend.lib.sta_select_patches(frontend._h, ptrs, (C.c_int * B)(*p.H), (C.c_int * B)(*p.W), B, p.dtype, p.mode,
                                               0.0 if thres is None else p.thres, p.invert, p.rule, p.min_score, ks, p.margin,
                                               score.data_ptr(), index.data_ptr(), pos.data_ptr(), meta.data_ptr(),
                                               meta.data_ptr() + 4 * B, stream))
    sel = Selections(p, score, index, pos, meta, stream)
    sel._keep = maps          # the launches read the maps after this returns
    return sel


def patch_scores(frontend: STAFrontend, maps, thres=None, invert: bool = False) -> List[torch.Tensor]:
    """The pooling alone: one [hp_b, wp_b] int32 view per map (the scores `select_tokens_from_maps` ranks; same arguments)."""
    return select_tokens_from_maps(frontend, maps, thres=thres, invert=invert, min_score=0).scores
