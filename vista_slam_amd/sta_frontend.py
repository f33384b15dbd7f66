"""`STAFrontend`: the reference's Python call surface over the MI355X C-ABI library.

Mirrors `SymmetricTwoViewAssociation` (vista_slam/sta_model/sta_model.py) as consumed by
`OnlineSLAM` (vista_slam/slam.py:95-106,144,162,165,179-180): constructor with the reference
defaults, `load_state_dict(strict=True)`, `.to()`, `.eval()`, `.parameters()`, and the four split
entry points `_encode_image`, `_decode_stereo`, `head_pose_s`, `head_pts`, plus the monolithic
`forward(views, loop_num)` (sta_model.py:247-291) and a batched `forward_pair(img_a, img_b)`.

torch is used ONLY for device memory and streams (tensor allocation, `.data_ptr()`,
`torch.cuda.current_stream()`); every FLOP runs in libsta_mi355.so.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Sequence

import numpy as np
import torch

from . import _lib
from . import weights as W


def _stream_ptr(device=None) -> int:
    """Raw HIP stream torch is currently enqueueing on FOR `device` (not for whatever torch's current device happens
    to be: a frontend on cuda:1 used while torch's current device is cuda:0 must get cuda:1's stream)."""
    return torch.cuda.current_stream(device).cuda_stream


class STAFrontend:
    def __init__(self, cfg: W.STAConfig = W.FULL, device: str | torch.device = "cuda:0",
                 precision: str = "f16x3h", img_size=(224, 224), lib=None):
        """`lib`: tests / tools only - another build of the library (`_lib.load_test()`: the test-hooks build with the
        kernel-level entry points of include/sta_mi355_debug.h); the product path never passes it."""
        self.lib = lib if lib is not None else _lib.load()
        if not torch.cuda.is_available():
            raise _lib.StaError("STAFrontend needs a ROCm GPU (MI355X / gfx950); there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.StaError("STAFrontend only runs on a cuda(=ROCm) device")
        self.img_size = img_size
        self.dec_depth = cfg.dec_depth
        self.dec_embed_dim = cfg.dec_embed_dim
        self.enc_embed_dim = cfg.enc_embed_dim
        self.patch_size = cfg.patch_size
        self.training = False
        c = _lib.StaConfig(cfg.patch_size, cfg.enc_embed_dim, cfg.enc_depth, cfg.enc_num_heads,
                           cfg.dec_embed_dim, cfg.dec_depth, cfg.dec_num_heads, cfg.mlp_ratio,
                           cfg.rope_base, cfg.ln_eps, _lib.PRECISIONS[precision])
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else 0
        _lib.check(self.lib.sta_create(C.byref(c), idx, C.byref(h)))
        self._h = h
        self._finalized = False
        self._pos_cache: Dict[tuple, torch.Tensor] = {}
        self._pos_verified: Dict[tuple, tuple] = {}       # foreign positions tensors already compared with the patch grid (_grid_from_pos)
        self.precision = precision

    # ------------------------------------------------------------------ nn.Module-like surface
    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self.lib.sta_destroy(h)
            except Exception:
                pass
            self._h = None

    def to(self, device):
        """nn.Module.to for the only move that makes sense here: the device the handle was created on.  Weights and
        workspace live inside libsta_mi355.so on that GPU; another index (or the CPU) raises instead of silently staying put."""
        d = torch.device(device)
        if d.type != "cuda":
            raise _lib.StaError("STAFrontend lives on the GPU it was created on; there is no CPU path")
        idx = d.index if d.index is not None else torch.cuda.current_device()
        mine = self.device.index if self.device.index is not None else 0
        if idx != mine:
            raise _lib.StaError(f"STAFrontend was created on cuda:{mine}; construct it with device='cuda:{idx}' instead of .to()")
        return self

    def _stream(self) -> int:
        return _stream_ptr(self.device)

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("inference-only frontend (training is out of scope)")
        return self

    def parameters(self) -> Iterable[torch.Tensor]:
        """Shape-only views (meta tensors) so `sum(p.numel() ...)` (slam.py:46) works."""
        seen = set()
        for name, shape, _k, _f in W.schema(self.cfg):
            src = W._alias_of(name)
            if src in seen:
                continue
            seen.add(src)
            yield torch.empty(shape, device="meta")

    def set_precision(self, precision: str):
        _lib.check(self.lib.sta_set_precision(self._h, _lib.PRECISIONS[precision]))
        self.precision = precision

    def range_report(self, reset: bool = True):
        """(fp16 saturations, fp8 correction-byte saturations) counted by the plane writers in THIS handle's calls since the last reset
        (sta_range_report): non-zero fp16 saturations = the forward left the range the fp16 planes can carry."""
        c = (C.c_ulonglong * 2)()
        _lib.check(self.lib.sta_range_report(self._h, c, int(reset)))
        return int(c[0]), int(c[1])

    def set_deterministic(self, on: bool = True):
        """Bit-reproducible results (no split-K fp32 atomics at SLAM scale; include/sta_mi355.h)."""
        _lib.check(self.lib.sta_set_deterministic(self._h, int(on)))

    def set_varlen_heads(self, on: bool):
        """How `regress_views_tokens[_finish]` runs the DPT head (include/sta_mi355.h, sta_set_varlen_heads): False (default) once per
        accepted edge and window side, True the window sides of all accepted edges in one varlen pass.  Read at finish time; the
        workspace for the varlen pass is planned at begin time, so it has to be on at begin as well.  Returns the previous setting."""
        prev = getattr(self, "_varlen_heads", False)
        _lib.check(self.lib.sta_set_varlen_heads(self._h, 1 if on else 0))
        self._varlen_heads = bool(on)
        return prev

    def set_side_lanes(self, mode: str = "auto"):
        """The library's internal side streams (include/sta_mi355.h, sta_set_side_lanes): "auto" (default: on unless the
        application overlaps calls on several streams itself), "off", "on".  Results are bit-identical in all three."""
        _lib.check(self.lib.sta_set_side_lanes(self._h, {"auto": -1, "off": 0, "on": 1}[mode]))

    def pipeline_streams(self, n: int = 3):
        """n library-owned streams measured to overlap pairwise (sta_pipeline_streams), as torch stream objects - the lanes of
        `keyframe_pipeline.replay(schedule="pipelined")`.  `self.pipeline_streams_verified` = how many of them are verified
        mutually concurrent."""
        ptrs = (C.c_void_p * n)()
        nv = C.c_int(0)
        _lib.check(self.lib.sta_pipeline_streams(self._h, n, ptrs, C.byref(nv)))
        self.pipeline_streams_verified = int(nv.value)
        return [torch.cuda.ExternalStream(int(ptrs[i]), device=self.device) for i in range(n)]

    def reserve(self, B: int, H: int, W: int, max_edges: int = 0, streams: Sequence["torch.cuda.Stream | None"] | None = None):
        """Allocate NOW everything calls of at most these sizes will need on `streams` (default: the current stream): scratch
        contexts, workspaces, side lanes, the scheduler's pinned buffer, the RoPE table (sta_reserve, include/sta_mi355.h).
        Afterwards such calls neither allocate nor synchronise the device (`alloc_stats()` stays put)."""
        sts = [self._stream()] if streams is None else [s.cuda_stream if s is not None else None for s in streams]
        arr = (C.c_void_p * len(sts))(*sts)
        _lib.check(self.lib.sta_reserve(self._h, B, H, W, max_edges, arr, len(sts)))
        return self

    def alloc_stats(self):
        """(allocations / frees / stream and event creations, device-wide synchronisations) the compute entry points of this handle
        have made since it was created (sta_alloc_stats)."""
        o = (C.c_int64 * 2)()
        _lib.check(self.lib.sta_alloc_stats(self._h, o))
        return int(o[0]), int(o[1])

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state: Dict[str, "torch.Tensor | np.ndarray"], strict: bool = True):
        if not strict:
            raise NotImplementedError("only strict=True is supported (slam.py:100)")
        for name, t in state.items():
            self._load_one(name, t)
        _lib.check(self.lib.sta_finalize_weights(self._h))   # raises on missing keys
        self._finalized = True
        return self

    def _load_one(self, name: str, t):
        if isinstance(t, torch.Tensor):
            t = t.detach().to("cpu", torch.float32).contiguous().numpy()
        a = np.ascontiguousarray(t, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        _lib.check(self.lib.sta_load_tensor(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim, 0))

    def load_procedural(self, seed: int = 43, qk_gain: float = 1.0, outlier: int = 0):
        """Stream the deterministic procedural weights (vista_slam_amd.weights) into the library."""
        for name, a in W.generate(self.cfg, seed=seed, qk_gain=qk_gain, reuse_buffer=True, outlier=outlier):
            self._load_one(name, a)
        _lib.check(self.lib.sta_finalize_weights(self._h))
        self._finalized = True
        return self

    # ------------------------------------------------------------------ helpers
    def _positions(self, B: int, hp: int, wp: int) -> torch.Tensor:
        """(y,x) patch positions, int64 [B,N,2] (PositionGetter, sta_blocks.py:241-247)."""
        key = (hp, wp)
        if key not in self._pos_cache:
            y = torch.arange(hp, device=self.device)
            x = torch.arange(wp, device=self.device)
            self._pos_cache[key] = torch.cartesian_prod(y, x)
        t = self._pos_cache[key].view(1, hp * wp, 2).expand(B, -1, 2).clone()
        # provenance: this tensor IS the patch grid (checked without a device sync in _grid_from_pos) - as long as nobody wrote
        # to it since: the tag carries the tensor's version counter, an in-place edit (pos.add_(1), copy_) invalidates it
        t._sta_grid = (hp, wp, t._version)
        return t

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        if t.device != self.device:
            t = t.to(self.device)
        if t.dtype != torch.float32:
            t = t.float()
        return t

    @staticmethod
    def _check_hw(H: int, W_: int, P: int = 16):
        assert H % P == 0, f"Input image height ({H}) is not a multiple of patch size ({P})."
        assert W_ % P == 0, f"Input image width ({W_}) is not a multiple of patch size ({P})."

    # ------------------------------------------------------------------ split entry points
    def _encode_image(self, image: torch.Tensor, true_shape=None, normalize: bool = True):
        image = self._f32(image).contiguous()
        B, Cc, H, W_ = image.shape
        assert Cc == 3
        self._check_hw(H, W_, self.patch_size)
        hp, wp = H // 16, W_ // 16
        feat = torch.empty(B, hp * wp, self.cfg.enc_embed_dim, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.sta_encode(self._h, image.data_ptr(), B, H, W_, feat.data_ptr(), self._stream()))
        if normalize:   # the reference's default argument (sta_model.py:163,172-173); forward / SLAM pass False
            _lib.check(self.lib.sta_encoder_norm(self._h, feat.data_ptr(), B * hp * wp, feat.data_ptr(), self._stream()))
        return feat, self._positions(B, hp, wp)

    def _grid_from_pos(self, pos: torch.Tensor, N: int):
        """Classify a positions tensor: (hp, wp, None) when it IS the (y, x) patch grid of an hp x wp frame - RoPE is then evaluated on
        the grid inside the QKV epilogues (sta_decode) -, (None, None, pos_max) for any other positions - the reference rotates q / k
        by whatever it is handed (sta_blocks.py:134-137,196-199), served by sta_decode_pos, which looks every row's position up in a
        table.  Tensors this frontend produced (what slam.py:144 stores and feeds back at :162) carry a provenance tag and cost
        nothing; a foreign tensor is compared with the grid ONCE (two device syncs) and the verdict is cached."""
        g = getattr(pos, "_sta_grid", None)
        if g is not None and g[0] * g[1] == N and tuple(pos.shape[1:]) == (N, 2) and g[2] == pos._version:
            return g[0], g[1], None
        assert pos.dim() == 3 and tuple(pos.shape[1:]) == (N, 2), f"positions must be [B, {N}, 2] (got {tuple(pos.shape)})"
        # a foreign tensor (the tag does not survive .to() / .clone() / indexing / a save-load round trip) is verified ONCE: the
        # verdict is cached by (storage address, version counter, shape), so the device syncs below are paid per tensor, not
        # per _decode_stereo call - the zero-edit SLAM path feeds the same cached positions back for every edge of a keyframe
        key = (pos.data_ptr(), pos._version, tuple(pos.shape), str(pos.device))
        hit = self._pos_verified.get(key)
        if hit is not None:
            return hit[0], hit[1], hit[2]
        assert not pos.dtype.is_floating_point, "positions are integer (y, x) coordinates (PositionGetter, sta_blocks.py:241-247)"
        mx = pos[0].max(dim=0).values.tolist()
        hp, wp = int(mx[0]) + 1, int(mx[1]) + 1
        ok = hp * wp == N and bool(torch.equal(pos.to(self.device, torch.int64), self._positions(pos.shape[0], hp, wp)))
        if ok:
            verdict = (hp, wp, None)
        else:
            lo, hi = int(pos.min()), int(pos.max())
            if lo < -1:
                raise ValueError(f"positions below -1 ({lo}) are not served (-1 is the pose token's position; the reference's python RoPE "
                                 "indexes its cos / sin tables with the position)")
            verdict = (None, None, max(hi, 0))
        if len(self._pos_verified) >= 4096:
            self._pos_verified.clear()
        # (the entry holds a reference to the tensor: its address cannot be handed to another tensor while the entry lives)
        self._pos_verified[key] = verdict + (pos,)
        return verdict

    def _decode_stereo(self, feat1: torch.Tensor, feat2: torch.Tensor, pose1: torch.Tensor, pose2: torch.Tensor,
                       layers: Sequence[int] | None = None):
        """Returns two lists of dec_depth+1 tensors [B, N+1, D] like the reference.  `layers`
        (extension) restricts which list entries are materialised (others are None)."""
        feat1 = self._f32(feat1).contiguous()
        feat2 = self._f32(feat2).contiguous()
        B, N, E = feat1.shape
        # The module code would accept two views with different token counts (cross-attention takes any memory length,
        # sta_blocks.py:193-205); the pipeline never produces them (one process_image resolution, sta_model.py:257-262), and
        # here both sides run as ONE batch of 2B sequences over the shared decoder weights: not served
        assert feat2.shape[1] == N and feat2.shape[0] == B, \
            f"both views must have the same token grid (got {tuple(feat1.shape)} and {tuple(feat2.shape)})"
        assert feat2.shape == feat1.shape and E == self.cfg.enc_embed_dim
        g1, g2 = self._grid_from_pos(pose1, N), self._grid_from_pos(pose2, N)
        assert pose1.shape[0] == B and pose2.shape[0] == B, "one positions row per batch entry"
        on_grid = g1[2] is None and g2[2] is None and g1[:2] == g2[:2]
        L = self.cfg.dec_depth + 1
        want = range(L) if layers is None else layers
        D = self.cfg.dec_embed_dim
        out1: List[torch.Tensor | None] = [None] * L
        out2: List[torch.Tensor | None] = [None] * L
        p1 = (C.c_void_p * L)()
        p2 = (C.c_void_p * L)()
        for i in want:
            out1[i] = torch.empty(B, N + 1, D, device=self.device, dtype=torch.float32)
            out2[i] = torch.empty(B, N + 1, D, device=self.device, dtype=torch.float32)
            p1[i] = out1[i].data_ptr()
            p2[i] = out2[i].data_ptr()
        if on_grid:
            _lib.check(self.lib.sta_decode(self._h, feat1.data_ptr(), feat2.data_ptr(), B, g1[0], g1[1], p1, p2, self._stream()))
        else:       # any other positions (a window of a larger grid, a permuted order, two different grids of equal token count)
            q1 = pose1.to(self.device, torch.int64).contiguous()
            q2 = pose2.to(self.device, torch.int64).contiguous()
            pos_max = max(g[2] if g[2] is not None else max(g[0], g[1]) - 1 for g in (g1, g2))
            _lib.check(self.lib.sta_decode_pos(self._h, feat1.data_ptr(), feat2.data_ptr(), q1.data_ptr(), q2.data_ptr(),
                                               B, N, pos_max, p1, p2, self._stream()))
        return out1, out2

    def decode_stereo_mixed(self, feat1: torch.Tensor, feat2: torch.Tensor, pos1: torch.Tensor, pos2: torch.Tensor,
                            layers: Sequence[int] | None = None):
        """`_decode_stereo` for two views with DIFFERENT token counts (a landscape and a portrait frame, two cameras, a loop
        candidate kept at a lower resolution): feat1 [B, N1, E], feat2 [B, N2, E] -> two lists of dec_depth+1 tensors
        [B, N1+1, D] / [B, N2+1, D] like the reference's module code returns for such a pair (cross attention takes any memory
        length, sta_blocks.py:193-205).  Positions must be each side's own patch grid (what `_encode_image` returns).  Equal
        counts are accepted and take the same route (sta_decode_mixed), so the two routes can be compared."""
        feat1 = self._f32(feat1).contiguous()
        feat2 = self._f32(feat2).contiguous()
        B, N1, E = feat1.shape
        N2 = feat2.shape[1]
        assert feat2.shape[0] == B and feat2.shape[2] == E and E == self.cfg.enc_embed_dim, \
            f"both views need the same batch and feature width (got {tuple(feat1.shape)} and {tuple(feat2.shape)})"
        assert pos1.shape[0] == B and pos2.shape[0] == B, "one positions row per batch entry"
        g1, g2 = self._grid_from_pos(pos1, N1), self._grid_from_pos(pos2, N2)
        if g1[2] is not None or g2[2] is not None:
            raise NotImplementedError("decode_stereo_mixed serves patch-grid positions only: foreign positions (a window of a larger "
                                      "grid, a permuted order) are served for equal token counts by _decode_stereo and for any "
                                      "token counts by decode_stereo_tokens")
        L = self.cfg.dec_depth + 1
        want = range(L) if layers is None else layers
        D = self.cfg.dec_embed_dim
        out1: List[torch.Tensor | None] = [None] * L
        out2: List[torch.Tensor | None] = [None] * L
        p1 = (C.c_void_p * L)()
        p2 = (C.c_void_p * L)()
        for i in want:
            out1[i] = torch.empty(B, N1 + 1, D, device=self.device, dtype=torch.float32)
            out2[i] = torch.empty(B, N2 + 1, D, device=self.device, dtype=torch.float32)
            p1[i] = out1[i].data_ptr()
            p2[i] = out2[i].data_ptr()
        _lib.check(self.lib.sta_decode_mixed(self._h, feat1.data_ptr(), feat2.data_ptr(), B, g1[0], g1[1], g2[0], g2[1],
                                             p1, p2, self._stream()))
        return out1, out2

    def forward_pair_mixed(self, img_a: torch.Tensor, img_b: torch.Tensor):
        """`forward_pair` for two images of different shape [B,3,Ha,Wa] / [B,3,Hb,Wb]: each is encoded at its own shape, the pair
        is decoded by `decode_stereo_mixed`, and both heads run per side at that side's shape.  Returns (main, support) dicts with
        pts3d_pred, conf, relative_pose, relative_pose_conf; a portrait side's per-pixel outputs are transposed views, like
        everywhere else."""
        img_a, img_b = self._f32(img_a).contiguous(), self._f32(img_b).contiguous()
        assert img_a.shape[0] == img_b.shape[0], "both views need the same batch"
        hooks = self.cfg.hooks
        layers = sorted({hk - 1 for hk in hooks[1:]})
        feats = [self._encode_image(im, None, normalize=False) for im in (img_a, img_b)]
        d1, d2 = self.decode_stereo_mixed(feats[0][0], feats[1][0], feats[0][1], feats[1][1], layers=layers)
        res = []
        for im, (feat, _pos), dec in zip((img_a, img_b), feats, (d1, d2)):
            B, _c, H, W_ = im.shape
            toks = [feat] + [None if t is None else t[:, 1:, :] for t in dec]
            pts = self.head_pts(toks, [[H, W_]] * B)
            pose = self.head_pose_s(dec[-1][:, 0, :])
            res.append({"pts3d_pred": pts["pts3d"], "conf": pts["conf"], "relative_pose": pose["pose"], "relative_pose_conf": pose["conf"]})
        return res[0], res[1]

    def decode_stereo_tokens(self, feat1: torch.Tensor, feat2: torch.Tensor, pos1: torch.Tensor, pos2: torch.Tensor,
                             layers: Sequence[int] | None = None):
        """`_decode_stereo` on TOKEN SUBSETS: feat1 [B, N1, E] with positions pos1 [B, N1, 2], feat2 [B, N2, E] with pos2
        [B, N2, 2] - any token counts (down to 1, equal or not) with any integer (y, x) positions >= -1, each batch entry its own:
        a rectangular window of one view against the whole other view, a pruned token set (see `window_tokens`, `select_tokens`).
        Returns two lists of dec_depth+1 tensors [B, N1+1, D] / [B, N2+1, D] like the reference's module code returns for such
        inputs (every attention rotates q / k by the positions it is handed, sta_blocks.py:134-137,196-199).  Always takes the
        sta_decode_tokens route, also for inputs the other entries serve, so the routes can be compared."""
        feat1 = self._f32(feat1).contiguous()
        feat2 = self._f32(feat2).contiguous()
        assert feat1.dim() == 3 and feat2.dim() == 3, "features are [B, N, E]"
        B, N1, E = feat1.shape
        N2 = feat2.shape[1]
        assert feat2.shape[0] == B and feat2.shape[2] == E and E == self.cfg.enc_embed_dim, \
            f"both views need the same batch and feature width (got {tuple(feat1.shape)} and {tuple(feat2.shape)})"
        assert N1 >= 1 and N2 >= 1, "every side needs at least one token"
        assert pos1.shape[0] == B and pos2.shape[0] == B, "one positions row per batch entry"
        g1, g2 = self._grid_from_pos(pos1, N1), self._grid_from_pos(pos2, N2)
        pos_max = max(g[2] if g[2] is not None else max(g[0], g[1]) - 1 for g in (g1, g2))
        q1 = pos1.to(self.device, torch.int64).contiguous()
        q2 = pos2.to(self.device, torch.int64).contiguous()
        L = self.cfg.dec_depth + 1
        want = range(L) if layers is None else layers
        D = self.cfg.dec_embed_dim
        out1: List[torch.Tensor | None] = [None] * L
        out2: List[torch.Tensor | None] = [None] * L
        p1 = (C.c_void_p * L)()
        p2 = (C.c_void_p * L)()
        for i in want:
            out1[i] = torch.empty(B, N1 + 1, D, device=self.device, dtype=torch.float32)
            out2[i] = torch.empty(B, N2 + 1, D, device=self.device, dtype=torch.float32)
            p1[i] = out1[i].data_ptr()
            p2[i] = out2[i].data_ptr()
        _lib.check(self.lib.sta_decode_tokens(self._h, feat1.data_ptr(), feat2.data_ptr(), q1.data_ptr(), q2.data_ptr(),
                                              B, N1, N2, pos_max, p1, p2, self._stream()))
        return out1, out2

    @staticmethod
    def select_tokens(feat: torch.Tensor, pos: torch.Tensor, index):
        """Gather a token subset: feat [B, N, E], pos [B, N, 2], index [K] (the same tokens of every batch entry) or [B, K] ->
        (feat [B, K, E], pos [B, K, 2]) in the order of `index` - the inputs of `decode_stereo_tokens`."""
        index = torch.as_tensor(index, dtype=torch.int64, device=feat.device)
        B, N, E = feat.shape
        assert tuple(pos.shape) == (B, N, 2), f"positions must be [{B}, {N}, 2] (got {tuple(pos.shape)})"
        if index.dim() == 1:
            index = index[None].expand(B, -1)
        assert index.dim() == 2 and index.shape[0] == B and index.shape[1] >= 1, f"index must be [K] or [{B}, K] (got {tuple(index.shape)})"
        assert int(index.min()) >= 0 and int(index.max()) < N, "token index out of range"
        f = torch.gather(feat, 1, index[:, :, None].expand(-1, -1, E))
        p = torch.gather(pos.to(feat.device), 1, index[:, :, None].expand(-1, -1, 2))
        return f.contiguous(), p.contiguous()

    @staticmethod
    def window_tokens(feat: torch.Tensor, pos: torch.Tensor, grid, window):
        """The tokens of a rectangular window of an encoded frame, row-major: feat [B, hp*wp, E], pos [B, hp*wp, 2] on the patch
        grid `grid` = (hp, wp); `window` = (y0, x0, h, w) in patches, one tuple for all batch entries or one per entry (all of one
        size h x w).  -> (feat [B, h*w, E], pos [B, h*w, 2])."""
        hp, wp = int(grid[0]), int(grid[1])
        B = feat.shape[0]
        assert feat.shape[1] == hp * wp, f"{feat.shape[1]} tokens are not a {hp} x {wp} grid"
        return STAFrontend.select_tokens(feat, pos, STAFrontend.window_index((hp, wp), window, B))

    @staticmethod
    def window_index(grid, window, B: int) -> torch.Tensor:
        """Row-major token indices [B, h*w] (int64, CPU) of a rectangular window of the patch grid `grid` = (hp, wp); `window` as in
        `window_tokens` - the `index` argument of `encode_tokens`."""
        hp, wp = int(grid[0]), int(grid[1])
        wins = [tuple(int(v) for v in window)] * B if not isinstance(window[0], (tuple, list)) else [tuple(int(v) for v in w) for w in window]
        assert len(wins) == B and len({w[2:] for w in wins}) == 1, "one window per batch entry, all of one size"
        rows = []
        for y0, x0, h, w in wins:
            assert h >= 1 and w >= 1 and 0 <= y0 and y0 + h <= hp and 0 <= x0 and x0 + w <= wp, f"window {(y0, x0, h, w)} leaves the {hp} x {wp} grid"
            rows.append(((torch.arange(y0, y0 + h)[:, None] * wp) + torch.arange(x0, x0 + w)[None, :]).reshape(-1))
        return torch.stack(rows)

    def forward_pair_window(self, img_a: torch.Tensor, img_b: torch.Tensor, window_a=None, window_b=None, encode: str = "frame"):
        """`forward_pair` with one or both views restricted to a rectangular window of patches (a region of interest, the
        overlapping part of a loop candidate): both frames [B,3,Ha,Wa] / [B,3,Hb,Wb] are encoded WHOLE, `window_a` / `window_b`
        = (y0, x0, h, w) in patches (or one per batch entry; None = the whole frame) select the tokens that enter the decoder
        (`decode_stereo_tokens`, with their true grid positions), and both heads run per side at that side's token shape
        (16 h, 16 w).  Returns (main, support) dicts like `forward_pair_mixed`.  A window's outputs are what the reference computes
        for those tokens: the decoder attends to the selected tokens only and the DPT head sees the window as an image of its own,
        so they are NOT a crop of the full-frame outputs.
        `encode`: "frame" (default) as above - a window's tokens are a slice of the whole frame's encoding, they have attended to the
        rest of the frame; "window": a windowed side is encoded from its window's patches alone (`encode_tokens`, the reference's
        encoder on those tokens with their frame positions) and pays for those tokens only."""
        if encode not in ("frame", "window"):
            raise ValueError(f'encode must be "frame" or "window" (got {encode!r})')
        img_a, img_b = self._f32(img_a).contiguous(), self._f32(img_b).contiguous()
        assert img_a.shape[0] == img_b.shape[0], "both views need the same batch"
        hooks = self.cfg.hooks
        layers = sorted({hk - 1 for hk in hooks[1:]})
        sides = []
        for im, win in ((img_a, window_a), (img_b, window_b)):
            B, _c, H, W_ = im.shape
            shape = (H, W_)
            if win is not None and encode == "window":
                feat, pos = self.encode_tokens(im, index=self.window_index((H // 16, W_ // 16), win, B))
            else:
                feat, pos = self._encode_image(im, None, normalize=False)
            if win is not None:
                if encode == "frame":
                    feat, pos = self.window_tokens(feat, pos, (H // 16, W_ // 16), win)
                w0 = win if not isinstance(win[0], (tuple, list)) else win[0]
                shape = (16 * int(w0[2]), 16 * int(w0[3]))
            sides.append((feat, pos, shape))
        d1, d2 = self.decode_stereo_tokens(sides[0][0], sides[1][0], sides[0][1], sides[1][1], layers=layers)
        res = []
        for (feat, _pos, (H, W_)), dec in zip(sides, (d1, d2)):
            toks = [feat] + [None if t is None else t[:, 1:, :] for t in dec]
            pts = self.head_pts(toks, [[H, W_]] * feat.shape[0])
            pose = self.head_pose_s(dec[-1][:, 0, :])
            res.append({"pts3d_pred": pts["pts3d"], "conf": pts["conf"], "relative_pose": pose["pose"], "relative_pose_conf": pose["conf"]})
        return res[0], res[1]

    def head_pose_s(self, pose_token: torch.Tensor):
        tok = self._f32(pose_token)
        B, D = tok.shape
        assert D == self.cfg.dec_embed_dim
        if tok.stride(1) != 1:
            tok = tok.contiguous()
        pose = torch.empty(B, 4, 4, device=self.device, dtype=torch.float32)
        conf = torch.empty(B, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.sta_head_pose(self._h, tok.data_ptr(), B, tok.stride(0) if B > 1 else D,
                                          pose.data_ptr(), conf.data_ptr(), self._stream()))
        return {"pose": pose, "conf": conf}

    def _rows(self, t: torch.Tensor, N: int, Cdim: int) -> torch.Tensor:
        t = self._f32(t)
        assert t.shape[1] == N and t.shape[2] == Cdim, f"bad token tensor shape {tuple(t.shape)}"
        if t.stride(2) != 1 or t.stride(1) != Cdim:
            t = t.contiguous()
        return t

    def head_pts(self, decout: Sequence[torch.Tensor], true_shape):
        """decout = [enc_feat] + [tok[:,1:,:] for tok in dec_list] (14 entries for depth 12);
        only the hooks [0, d/2+1, 3d/4+1, d+1] are read (dpt_head.py:112)."""
        ts = true_shape
        if isinstance(ts, torch.Tensor):
            assert bool((ts[0:1] == ts).all()), "true_shape must be all identical"
            H, W_ = int(ts[0, 0]), int(ts[0, 1])
        else:
            H, W_ = int(ts[0][0]), int(ts[0][1])
        self._check_hw(H, W_)
        hooks = self.cfg.hooks
        N = (H // 16) * (W_ // 16)
        enc = self._rows(decout[hooks[0]], N, self.cfg.enc_embed_dim)
        hk = [self._rows(decout[i], N, self.cfg.dec_embed_dim) for i in hooks[1:]]
        B = enc.shape[0]
        pts = torch.empty(B, H, W_, 3, device=self.device, dtype=torch.float32)
        conf = torch.empty(B, H, W_, device=self.device, dtype=torch.float32)

        def bs(t):
            return t.stride(0) if B > 1 else t.shape[1] * t.shape[2]
        _lib.check(self.lib.sta_head_pts(self._h, enc.data_ptr(), bs(enc), hk[0].data_ptr(), bs(hk[0]),
                                         hk[1].data_ptr(), bs(hk[1]), hk[2].data_ptr(), bs(hk[2]),
                                         B, H, W_, pts.data_ptr(), conf.data_ptr(), self._stream()))
        if H > W_:      # portrait: the reference's head wrapper returns transposed views (utils/misc.py:60-61,81)
            pts, conf = pts.swapaxes(1, 2), conf.swapaxes(1, 2)
        return {"pts3d": pts, "conf": conf}

    def _row_table(self, rows: Sequence[torch.Tensor], Cdim: int):
        """Per-entry row blocks [n_b, Cdim] -> (base tensor, first row of every entry in it).  In place where the entries are dense-row
        views of ONE buffer whose offsets are whole rows (the packed outputs of the varlen calls); else one packed copy."""
        ts = [self._f32(t) for t in rows]
        for t in ts:
            assert t.dim() == 2 and t.shape[1] == Cdim, f"bad token tensor shape {tuple(t.shape)}"
        store = ts[0].untyped_storage().data_ptr()
        base = min(t.data_ptr() for t in ts)
        if all(t.untyped_storage().data_ptr() == store and t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) == Cdim) and
               (t.data_ptr() - base) % (Cdim * 4) == 0 for t in ts) and base % 16 == 0:
            return ts, base, [(t.data_ptr() - base) // (Cdim * 4) for t in ts]
        buf = torch.cat([t.reshape(-1, Cdim) for t in ts]).contiguous()
        offs, acc = [], 0
        for t in ts:
            offs.append(acc)
            acc += int(t.shape[0])
        return buf, buf.data_ptr(), offs

    def head_pts_varlen(self, feats: Sequence[torch.Tensor], hooks: Sequence[Sequence[torch.Tensor]], rects: Sequence[Sequence[int]],
                        out_pix: Sequence[int] | None = None, out: tuple | None = None):
        """`head_pts` for B <= 32 entries whose patch rectangles differ, in ONE sta_head_pts_varlen call.  feats[b] [h_b w_b, E]: the
        encoder features of entry b; hooks: three lists (decoder hooks d/2, 3d/4, d - dpt_head.py:112) of B tensors [h_b w_b, D], pose
        row already skipped; rects[b] = (h_b, w_b) patches, row-major.  Views into one packed buffer (what `encode_tokens_varlen` /
        `decode_stereo_varlen` return) are read in place through row tables; anything else is packed first.  Returns a list of B dicts
        {"pts3d": [1, 16 h, 16 w, 3], "conf": [1, 16 h, 16 w]} - per entry exactly what `head_pts` returns for it alone, the transposed
        views for h > w included (utils/misc.py:48-61).  out_pix / out = (pts [P, 3], conf [P]): the entries' pixel offsets in caller
        buffers (default: a fresh packed pair)."""
        B = len(feats)
        assert 1 <= B <= 32, f"1 .. 32 entries per call (got {B})"
        assert len(hooks) == 3 and all(len(hk) == B for hk in hooks) and len(rects) == B, "three hook lists and one rectangle per entry"
        E, D = self.cfg.enc_embed_dim, self.cfg.dec_embed_dim
        hp = [int(r[0]) for r in rects]
        wp = [int(r[1]) for r in rects]
        for b in range(B):
            assert feats[b].shape[0] == hp[b] * wp[b] and all(hk[b].shape[0] == hp[b] * wp[b] for hk in hooks), \
                f"entry {b}: {hp[b]} x {wp[b]} patches need {hp[b] * wp[b]} rows"
        keep_e, enc_ptr, enc_row = self._row_table(feats, E)
        tabs = [self._row_table(hk, D) for hk in hooks]
        if any(t[2] != tabs[0][2] for t in tabs):          # the three hooks share ONE row table: pack them alike
            tabs = []
            for hk in hooks:
                buf = torch.cat([self._f32(t).reshape(-1, D) for t in hk]).contiguous()
                tabs.append((buf, buf.data_ptr(), [sum(hp[i] * wp[i] for i in range(b)) for b in range(B)]))
        npix = [256 * hp[b] * wp[b] for b in range(B)]
        if out is None:
            assert out_pix is None, "out_pix names offsets in caller buffers: pass out=(pts, conf)"
            pts = torch.empty(sum(npix), 3, device=self.device, dtype=torch.float32)
            conf = torch.empty(sum(npix), device=self.device, dtype=torch.float32)
        else:
            pts, conf = out
            assert pts.dtype == torch.float32 and conf.dtype == torch.float32 and pts.is_contiguous() and conf.is_contiguous()
        offs = [sum(npix[:b]) for b in range(B)] if out_pix is None else [int(o) for o in out_pix]
        for b in range(B):
            assert 0 <= offs[b] and offs[b] + npix[b] <= conf.numel() and (offs[b] + npix[b]) * 3 <= pts.numel(), f"entry {b}: output range"
        I64, I32 = C.c_int64 * B, C.c_int * B
        _lib.check(self.lib.sta_head_pts_varlen(self._h, enc_ptr, I64(*enc_row), tabs[0][1], tabs[1][1], tabs[2][1], I64(*tabs[0][2]),
                                                I32(*hp), I32(*wp), B, pts.data_ptr(), conf.data_ptr(),
                                                None if out_pix is None else I64(*offs), self._stream()))
        del keep_e
        res = []
        pf, cf = pts.view(-1, 3), conf.view(-1)
        for b in range(B):
            H, W_ = 16 * hp[b], 16 * wp[b]
            p = pf[offs[b]:offs[b] + npix[b]].view(1, H, W_, 3)
            c = cf[offs[b]:offs[b] + npix[b]].view(1, H, W_)
            if H > W_:
                p, c = p.swapaxes(1, 2), c.swapaxes(1, 2)
            res.append({"pts3d": p, "conf": c})
        return res

    # ------------------------------------------------------------------ monolithic paths
    @staticmethod
    def _landscape_views(outs, H: int, W_: int):
        """Portrait frames: per-pixel outputs as transposed views [B,W,H,..] of the image-orientation buffers, exactly what
        `transpose_to_landscape(head)` returns in the reference (utils/misc.py:60-61,81)."""
        if H > W_:
            for o in outs:
                o["pts3d_pred"] = o["pts3d_pred"].swapaxes(1, 2)
                o["conf"] = o["conf"].swapaxes(1, 2)
        return outs[0], outs[1]

    def forward_pair(self, img_a: torch.Tensor, img_b: torch.Tensor):
        """Batched two-view forward == forward({'main_view':a,'neighbor_views':[b],'loop_views':[]}).
        Returns (main, support) dicts with pts3d_pred, conf, relative_pose, relative_pose_conf."""
        img_a = self._f32(img_a).contiguous()
        img_b = self._f32(img_b).contiguous()
        assert img_a.shape == img_b.shape
        B, Cc, H, W_ = img_a.shape
        assert Cc == 3
        self._check_hw(H, W_)
        outs = []
        arrs = [(C.c_void_p * 2)() for _ in range(4)]
        for k in range(2):
            o = {"pts3d_pred": torch.empty(B, H, W_, 3, device=self.device, dtype=torch.float32),
                 "conf": torch.empty(B, H, W_, device=self.device, dtype=torch.float32),
                 "relative_pose": torch.empty(B, 4, 4, device=self.device, dtype=torch.float32),
                 "relative_pose_conf": torch.empty(B, device=self.device, dtype=torch.float32)}
            outs.append(o)
            for a, key in zip(arrs, ("pts3d_pred", "conf", "relative_pose", "relative_pose_conf")):
                a[k] = o[key].data_ptr()
        _lib.check(self.lib.sta_forward_pair(self._h, img_a.data_ptr(), img_b.data_ptr(), B, H, W_,
                                             arrs[0], arrs[1], arrs[2], arrs[3], self._stream()))
        return self._landscape_views(outs, H, W_)

    def encode_u8hwc(self, image_u8: torch.Tensor):
        """Extension: encode uint8 HWC camera frames [B,H,W,3] directly; the reference
        ImgNorm (x/255-0.5)/0.5 is fused into the patch gather (bit-identical to `_encode_image` on the
        normalised NCHW tensor)."""
        assert image_u8.dtype == torch.uint8 and image_u8.dim() == 4 and image_u8.shape[-1] == 3
        img = image_u8.to(self.device).contiguous()
        B, H, W_, _ = img.shape
        self._check_hw(H, W_, self.patch_size)
        hp, wp = H // 16, W_ // 16
        feat = torch.empty(B, hp * wp, self.cfg.enc_embed_dim, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.sta_encode_u8hwc(self._h, img.data_ptr(), B, H, W_, feat.data_ptr(), self._stream()))
        return feat, self._positions(B, hp, wp)

    # ------------------------------------------------------------------ the encoder on token subsets
    def _subset_positions(self, B: int, hp: int, wp: int, pos, index) -> torch.Tensor:
        """The one of `pos` [B, N, 2] / `index` [B, N] that was given -> device int64 [B, N, 2] (y, x) positions, checked on the host:
        a selection in host memory is uploaded with a synchronous copy and one on the device is read back: either way the call waits
        for its stream before the entry point is called (the entry points themselves never do)."""
        if (pos is None) == (index is None):
            raise ValueError("give exactly one of pos ([B, N, 2] (y, x) patch positions) and index ([B, N] into the row-major patch grid)")
        if index is not None:
            index = torch.as_tensor(index)
            assert index.dtype == torch.int64, f"index must be int64 (got {index.dtype})"
            assert index.dim() == 2 and index.shape[0] == B and index.shape[1] >= 1, f"index must be [{B}, N >= 1] (got {tuple(index.shape)})"
            lo, hi = int(index.min()), int(index.max())
            if lo < 0 or hi >= hp * wp:
                raise ValueError(f"token index outside the {hp} x {wp} patch grid (range [{lo}, {hi}])")
            index = index.to(self.device)
            return torch.stack([torch.div(index, wp, rounding_mode="floor"), index % wp], -1).contiguous()
        pos = torch.as_tensor(pos)
        assert pos.dtype == torch.int64, f"positions must be int64 (y, x) patch coordinates (got {pos.dtype})"
        assert pos.dim() == 3 and pos.shape[0] == B and pos.shape[1] >= 1 and pos.shape[2] == 2, f"positions must be [{B}, N >= 1, 2] (got {tuple(pos.shape)})"
        lo = pos.reshape(-1, 2).min(dim=0).values.tolist()
        hi = pos.reshape(-1, 2).max(dim=0).values.tolist()
        if lo[0] < 0 or lo[1] < 0 or hi[0] >= hp or hi[1] >= wp:
            raise ValueError(f"positions outside the {hp} x {wp} patch grid (y in [{lo[0]}, {hi[0]}], x in [{lo[1]}, {hi[1]}])")
        return pos.to(self.device).contiguous()

    def encode_tokens(self, image: torch.Tensor, pos=None, index=None):
        """`_encode_image(normalize=False)` on a TOKEN SUBSET: image [B,3,H,W]; exactly one of `pos` ([B, N, 2] int64 (y, x) patch
        positions, CPU or device) and `index` ([B, N] int64 into the row-major patch grid) selects the N tokens of every batch entry -
        each entry its own, any order, repeats allowed.  A position names the patch that is gathered AND the RoPE position of the
        token.  -> (feat [B, N, E], pos [B, N, 2] on the device): what the reference's encoder computes for those tokens alone
        (patch_embed, gather, every Block with the gathered positions) - NOT a slice of the frame's encoding; only B*N rows are
        computed.  The positions keep the frame's coordinates and go on to `decode_stereo_tokens` as they are."""
        image = self._f32(image).contiguous()
        assert image.dim() == 4 and image.shape[1] == 3, f"image must be [B, 3, H, W] (got {tuple(image.shape)})"
        B, _c, H, W_ = image.shape
        self._check_hw(H, W_, self.patch_size)
        q = self._subset_positions(B, H // 16, W_ // 16, pos, index)
        N = q.shape[1]
        feat = torch.empty(B, N, self.cfg.enc_embed_dim, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.sta_encode_tokens(self._h, image.data_ptr(), q.data_ptr(), B, H, W_, N, feat.data_ptr(), self._stream()))
        return feat, q

    def encode_tokens_u8hwc(self, image_u8: torch.Tensor, pos=None, index=None):
        """`encode_tokens` on uint8 HWC camera frames [B,H,W,3] with the fused ImgNorm of `encode_u8hwc`: bit-identical to
        `encode_tokens` on the normalised NCHW tensor."""
        assert image_u8.dtype == torch.uint8 and image_u8.dim() == 4 and image_u8.shape[-1] == 3
        img = image_u8.to(self.device).contiguous()
        B, H, W_, _ = img.shape
        self._check_hw(H, W_, self.patch_size)
        q = self._subset_positions(B, H // 16, W_ // 16, pos, index)
        N = q.shape[1]
        feat = torch.empty(B, N, self.cfg.enc_embed_dim, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.sta_encode_tokens_u8hwc(self._h, img.data_ptr(), q.data_ptr(), B, H, W_, N, feat.data_ptr(), self._stream()))
        return feat, q

    @staticmethod
    def _rectangle_of(pos: torch.Tensor):
        """(h, w) when every batch entry of pos [B, N, 2] is a row-major h x w rectangle of patches (anywhere, all of one size), else None."""
        p = pos.cpu()
        B, N, _ = p.shape
        h, w = int(p[0, -1, 0] - p[0, 0, 0]) + 1, int(p[0, -1, 1] - p[0, 0, 1]) + 1
        if h < 1 or w < 1 or h * w != N:
            return None
        rect = torch.cartesian_prod(torch.arange(h), torch.arange(w)).view(1, N, 2)
        return (h, w) if bool(torch.equal(p - p[:, :1, :], rect.expand(B, -1, -1))) else None

    def forward_pair_tokens(self, img_a: torch.Tensor, img_b: torch.Tensor, pos_a: torch.Tensor, pos_b: torch.Tensor):
        """`forward_pair` on token subsets of both views, encoder included: `encode_tokens` on each frame with its positions
        ([B, Na, 2] / [B, Nb, 2]), `decode_stereo_tokens` on the two subsets, the pose head on both sides.  Returns (main, support)
        dicts like `forward_pair_window`.  The DPT head runs at a side's token shape (16 h, 16 w) only where that side is a row-major
        h x w rectangle of patches in every batch entry; any other side has None for pts3d_pred / conf."""
        img_a, img_b = self._f32(img_a).contiguous(), self._f32(img_b).contiguous()
        assert img_a.shape[0] == img_b.shape[0], "both views need the same batch"
        hooks = self.cfg.hooks
        layers = sorted({hk - 1 for hk in hooks[1:]})
        sides = [self.encode_tokens(im, pos=p) for im, p in ((img_a, pos_a), (img_b, pos_b))]
        d1, d2 = self.decode_stereo_tokens(sides[0][0], sides[1][0], sides[0][1], sides[1][1], layers=layers)
        res = []
        for (feat, pos), dec in zip(sides, (d1, d2)):
            rect = self._rectangle_of(pos)
            pts = {"pts3d": None, "conf": None}
            if rect is not None:
                toks = [feat] + [None if t is None else t[:, 1:, :] for t in dec]
                pts = self.head_pts(toks, [[16 * rect[0], 16 * rect[1]]] * feat.shape[0])
            pose = self.head_pose_s(dec[-1][:, 0, :])
            res.append({"pts3d_pred": pts["pts3d"], "conf": pts["conf"], "relative_pose": pose["pose"], "relative_pose_conf": pose["conf"]})
        return res[0], res[1]

    # ------------------------------------------------------------------ one token count per batch entry
    @staticmethod
    def pack_varlen(feats: Sequence[torch.Tensor], poss: Sequence[torch.Tensor], E: int, device=None):
        """One side of a varlen call: lists of [n_b, E] features and [n_b, 2] integer (y, x) positions, one pair per entry ->
        (feat [sum n, E] float32, pos [sum n, 2] int64, counts [B]) packed entry-major.  Entry b's tokens are rows
        [sum(counts[:b]), sum(counts[:b + 1])) of both."""
        assert len(feats) == len(poss) and len(feats) >= 1, "one positions tensor per features tensor, at least one entry"
        counts = []
        for b, (f, q) in enumerate(zip(feats, poss)):
            assert f.dim() == 2 and f.shape[1] == E, f"entry {b}: features must be [n, {E}] (got {tuple(f.shape)})"
            assert f.shape[0] >= 1, f"entry {b}: every side needs at least one token"
            assert tuple(q.shape) == (f.shape[0], 2), f"entry {b}: positions must be [{f.shape[0]}, 2] (got {tuple(q.shape)})"
            assert not q.dtype.is_floating_point, "positions are integer (y, x) coordinates (PositionGetter, sta_blocks.py:241-247)"
            counts.append(int(f.shape[0]))
        dev = feats[0].device if device is None else device
        feat = torch.cat([f.to(dev, torch.float32) for f in feats], 0).contiguous()
        pos = torch.cat([q.to(dev, torch.int64) for q in poss], 0).contiguous()
        return feat, pos, counts

    @staticmethod
    def varlen_offsets(counts: Sequence[int]):
        """First row of every entry in a packed decoder output [sum(n) + B, D] (entry b: counts[b] + 1 rows, pose token first),
        and the total: (offsets [B], rows)."""
        offs, r = [], 0
        for n in counts:
            offs.append(r)
            r += int(n) + 1
        return offs, r

    def _encode_varlen(self, frames: List[torch.Tensor], sizes: List[tuple], entry, pos, index):
        """The shared part of `encode_tokens_varlen[_u8hwc]`: per-entry selection checks, then ONE C call over the packed positions."""
        B = len(frames)
        sel = pos if pos is not None else index
        if (pos is None) == (index is None):
            raise ValueError("give exactly one of pos (a list of [n, 2] (y, x) patch positions) and index (a list of [n] indices into each entry's row-major patch grid)")
        if len(sel) != B:
            raise ValueError(f"one selection per frame: {B} frames, {len(sel)} selections")
        if not 1 <= B <= 32:
            raise ValueError(f"1 .. 32 entries per call (got {B})")
        qs = []
        for b, (H, W_) in enumerate(sizes):
            self._check_hw(H, W_, self.patch_size)
            one = torch.as_tensor(sel[b])
            if one.dim() == (2 if pos is not None else 1) and one.shape[0] == 0:
                raise ValueError(f"entry {b}: a token subset has at least one token")
            try:          # the rules and refusals of encode_tokens, on this entry alone in its OWN grid
                qs.append(self._subset_positions(1, H // 16, W_ // 16, one[None] if pos is not None else None, one[None] if index is not None else None)[0])
            except (ValueError, AssertionError) as err:
                raise type(err)(f"entry {b}: {err}") from None
        counts = [int(q.shape[0]) for q in qs]
        q = torch.cat(qs, 0).contiguous()
        feat = torch.empty(sum(counts), self.cfg.enc_embed_dim, device=self.device, dtype=torch.float32)
        ptrs = (C.c_void_p * B)(*[f.data_ptr() for f in frames])
        Hs, Ws = (C.c_int * B)(*[hw[0] for hw in sizes]), (C.c_int * B)(*[hw[1] for hw in sizes])
        _lib.check(entry(self._h, ptrs, Hs, Ws, q.data_ptr(), (C.c_int * B)(*counts), B, feat.data_ptr(), self._stream()))
        offs = [0]
        for n in counts:
            offs.append(offs[-1] + n)
        return [feat[offs[b]:offs[b + 1]] for b in range(B)], [q[offs[b]:offs[b + 1]] for b in range(B)]

    def encode_tokens_varlen(self, images: Sequence[torch.Tensor], pos=None, index=None):
        """`encode_tokens` for B <= 32 entries that differ in token count AND frame size, in ONE call: images[b] [3, H_b, W_b]; exactly
        one of `pos` (a list of [n_b, 2] int64 (y, x) patch positions) and `index` (a list of [n_b] int64 indices into entry b's own
        row-major patch grid), selected and refused per entry exactly as `encode_tokens` does.  Entry b is what `encode_tokens` returns
        for it alone at B = 1; nothing is padded, no token attends to another entry's.  -> (feats, poss): lists of per-entry views
        [n_b, E] / [n_b, 2] into one packed buffer each - what `decode_stereo_varlen` takes."""
        frames = []
        for b, im in enumerate(images):
            im = self._f32(im).contiguous()
            assert im.dim() == 3 and im.shape[0] == 3, f"entry {b}: a frame is [3, H, W] (got {tuple(im.shape)})"
            frames.append(im)
        return self._encode_varlen(frames, [(int(f.shape[1]), int(f.shape[2])) for f in frames], self.lib.sta_encode_varlen, pos, index)

    def encode_tokens_varlen_u8hwc(self, images_u8: Sequence[torch.Tensor], pos=None, index=None):
        """`encode_tokens_varlen` on uint8 HWC camera frames [H_b, W_b, 3] with the fused ImgNorm of `encode_u8hwc`: bit-identical to
        `encode_tokens_varlen` on the normalised [3, H_b, W_b] tensors."""
        frames = []
        for b, im in enumerate(images_u8):
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[-1] == 3, f"entry {b}: a camera frame is uint8 [H, W, 3] (got {im.dtype} {tuple(im.shape)})"
            frames.append(im.to(self.device).contiguous())
        return self._encode_varlen(frames, [(int(f.shape[0]), int(f.shape[1])) for f in frames], self.lib.sta_encode_varlen_u8hwc, pos, index)

    def decode_stereo_varlen(self, feats1: Sequence[torch.Tensor], feats2: Sequence[torch.Tensor], pos1: Sequence[torch.Tensor],
                             pos2: Sequence[torch.Tensor], layers: Sequence[int] | None = None):
        """`_decode_stereo` on a batch whose entries have their OWN token counts: feats1[b] [n1_b, E] with positions pos1[b]
        [n1_b, 2], feats2[b] [n2_b, E] with pos2[b] [n2_b, 2] - lists over the B <= 16 entries.  Entry b of the result is what the
        reference returns for that entry alone at B = 1 (batch entries never interact); nothing is padded.  Returns two lists over
        the dec_depth+1 layers; each element is None (layer not in `layers`) or a list of B views [n_b + 1, D] (pose token first)
        into one packed buffer.  One sta_decode_varlen call."""
        B = len(feats1)
        assert len(feats2) == B and len(pos1) == B and len(pos2) == B, "both views need the same number of entries"
        assert 1 <= B <= 16, f"1 .. 16 entries per call (got {B})"
        E, D = self.cfg.enc_embed_dim, self.cfg.dec_embed_dim
        f1, q1, n1 = self.pack_varlen(feats1, pos1, E, self.device)
        f2, q2, n2 = self.pack_varlen(feats2, pos2, E, self.device)
        lo, hi = torch.stack(torch.aminmax(torch.cat([q1, q2]))).tolist()          # (one device sync)
        if lo < -1:
            raise ValueError(f"positions below -1 ({lo}) are not served (-1 is the pose token's position; the reference's python RoPE "
                             "indexes its cos / sin tables with the position)")
        L = self.cfg.dec_depth + 1
        want = range(L) if layers is None else layers
        out1: List[List[torch.Tensor] | None] = [None] * L
        out2: List[List[torch.Tensor] | None] = [None] * L
        p1 = (C.c_void_p * L)()
        p2 = (C.c_void_p * L)()
        (o1, r1), (o2, r2) = self.varlen_offsets(n1), self.varlen_offsets(n2)
        for i in want:
            both = torch.empty(r1 + r2, D, device=self.device, dtype=torch.float32)      # one buffer per layer: `head_pts_varlen` reads both sides in place
            b1, b2 = both[:r1], both[r1:]
            p1[i], p2[i] = b1.data_ptr(), b2.data_ptr()
            out1[i] = [b1[o:o + n + 1] for o, n in zip(o1, n1)]
            out2[i] = [b2[o:o + n + 1] for o, n in zip(o2, n2)]
        _lib.check(self.lib.sta_decode_varlen(self._h, f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(),
                                              (C.c_int * B)(*n1), (C.c_int * B)(*n2), B, max(hi, 0), p1, p2, self._stream()))
        return out1, out2

    def forward_pairs_tokens(self, imgs_a: Sequence[torch.Tensor], imgs_b: Sequence[torch.Tensor], pos_a: Sequence[torch.Tensor],
                             pos_b: Sequence[torch.Tensor], encode: str = "grouped", heads: str = "entry"):
        """`forward_pair_tokens` for B pairs whose token subsets differ in size: imgs_a[b] [3, H, W] (any frame size per entry) with
        pos_a[b] [n, 2] int64 (y, x) patch positions, the same for side b.  Encoder: encode="grouped" (default): `encode_tokens`,
        entries of equal count and frame size sharing one call; encode="varlen": all 2B frames through `encode_tokens_varlen` - one
        call where 2B <= 32, else one per side.  Decoder: ONE `decode_stereo_varlen` call; pose head: once over all 2B pose rows; DPT
        head, where a side is a row-major rectangle of patches: heads="entry" (default): `head_pts` per entry and side; heads="varlen":
        every rectangular side of both sides through ONE `head_pts_varlen` call (chunks of 32).  Returns (main, support): two lists of B dicts
        with pts3d_pred / conf ([16 h, 16 w, 3] / [16 h, 16 w], or None), relative_pose [4, 4], relative_pose_conf []."""
        B = len(imgs_a)
        assert len(imgs_b) == B and len(pos_a) == B and len(pos_b) == B and B >= 1, "one frame and one positions tensor per entry and side"
        if encode not in ("grouped", "varlen"):
            raise ValueError(f'encode must be "grouped" or "varlen" (got {encode!r})')
        if heads not in ("entry", "varlen"):
            raise ValueError(f'heads must be "entry" or "varlen" (got {heads!r})')
        hooks = self.cfg.hooks
        layers = sorted({hk - 1 for hk in hooks[1:]})
        sides = []
        if encode == "varlen":
            for imgs in (imgs_a, imgs_b):
                for b, im in enumerate(imgs):
                    assert im.dim() == 3 and im.shape[0] == 3, f"entry {b}: a frame is [3, H, W] (got {tuple(im.shape)})"
            if 2 * B <= 32:
                f, q = self.encode_tokens_varlen(list(imgs_a) + list(imgs_b), pos=list(pos_a) + list(pos_b))
                sides = [(f[:B], q[:B]), (f[B:], q[B:])]
            else:
                sides = [self.encode_tokens_varlen(list(imgs), pos=list(poss)) for imgs, poss in ((imgs_a, pos_a), (imgs_b, pos_b))]
        for imgs, poss in ((imgs_a, pos_a), (imgs_b, pos_b)) if encode == "grouped" else ():
            groups: Dict[tuple, List[int]] = {}
            for b, (im, q) in enumerate(zip(imgs, poss)):
                assert im.dim() == 3 and im.shape[0] == 3, f"entry {b}: a frame is [3, H, W] (got {tuple(im.shape)})"
                groups.setdefault((int(q.shape[0]), int(im.shape[1]), int(im.shape[2])), []).append(b)
            feats: List[torch.Tensor | None] = [None] * B
            qs: List[torch.Tensor | None] = [None] * B
            for members in groups.values():
                f, q = self.encode_tokens(torch.stack([self._f32(imgs[b]) for b in members]),
                                          pos=torch.stack([torch.as_tensor(poss[b]).cpu() for b in members]))
                for j, b in enumerate(members):
                    feats[b], qs[b] = f[j], q[j]
            sides.append((feats, qs))
        d1, d2 = self.decode_stereo_varlen(sides[0][0], sides[1][0], sides[0][1], sides[1][1], layers=layers)
        pose = self.head_pose_s(torch.stack([t[0] for d in (d1, d2) for t in d[-1]]))
        res = []
        vl = {}
        if heads == "varlen":
            ent = [(k, b, self._rectangle_of(qs[b][None]), feats[b], [dec[hk - 1][b][1:, :] for hk in hooks[1:]])
                   for k, ((feats, qs), dec) in enumerate(zip(sides, (d1, d2))) for b in range(B)]
            ent = [e for e in ent if e[2] is not None]
            for c0 in range(0, len(ent), 32):
                part = ent[c0:c0 + 32]
                got = self.head_pts_varlen([e[3] for e in part], [[e[4][j] for e in part] for j in range(3)], [e[2] for e in part])
                for e, g in zip(part, got):
                    vl[(e[0], e[1])] = {key: v[0] for key, v in g.items()}
        for k, ((feats, qs), dec) in enumerate(zip(sides, (d1, d2))):
            outs = []
            for b in range(B):
                rect = self._rectangle_of(qs[b][None]) if heads == "entry" else None
                pts = vl.get((k, b), {"pts3d": None, "conf": None})
                if rect is not None:
                    toks = [feats[b][None]] + [None if t is None else t[b][None, 1:, :] for t in dec]
                    pts = self.head_pts(toks, [[16 * rect[0], 16 * rect[1]]])
                    pts = {key: v[0] for key, v in pts.items()}
                outs.append({"pts3d_pred": pts["pts3d"], "conf": pts["conf"], "relative_pose": pose["pose"][k * B + b],
                             "relative_pose_conf": pose["conf"][k * B + b]})
            res.append(outs)
        return res[0], res[1]

    def forward_pair_u8hwc(self, img_a: torch.Tensor, img_b: torch.Tensor):
        """`forward_pair` on uint8 HWC frames [B,H,W,3]."""
        assert img_a.dtype == torch.uint8 and img_b.dtype == torch.uint8 and img_a.shape == img_b.shape
        a, b = img_a.to(self.device).contiguous(), img_b.to(self.device).contiguous()
        B, H, W_, Cc = a.shape
        assert Cc == 3
        self._check_hw(H, W_)
        outs = []
        arrs = [(C.c_void_p * 2)() for _ in range(4)]
        for k in range(2):
            o = {"pts3d_pred": torch.empty(B, H, W_, 3, device=self.device, dtype=torch.float32),
                 "conf": torch.empty(B, H, W_, device=self.device, dtype=torch.float32),
                 "relative_pose": torch.empty(B, 4, 4, device=self.device, dtype=torch.float32),
                 "relative_pose_conf": torch.empty(B, device=self.device, dtype=torch.float32)}
            outs.append(o)
            for arr, key in zip(arrs, ("pts3d_pred", "conf", "relative_pose", "relative_pose_conf")):
                arr[k] = o[key].data_ptr()
        _lib.check(self.lib.sta_forward_pair_u8hwc(self._h, a.data_ptr(), b.data_ptr(), B, H, W_,
                                                   arrs[0], arrs[1], arrs[2], arrs[3], self._stream()))
        return self._landscape_views(outs, H, W_)

    def forward(self, views: dict, loop_num: int = 0):
        """sta_model.py:247-291.  The main view is encoded ONCE (:257); the k support views are encoded, decoded against
        it and run through the heads as ONE batch of k pairs (the reference loops over them; pairs are independent, so the
        results are the same to rounding)."""
        main_view = views["main_view"]
        support = list(views["neighbor_views"]) + list(views["loop_views"])   # eval: all loop views (sta_model.py:252-255)
        main_res, supp_res = [], []
        if not support:
            return {"main_views": main_res, "support_views": supp_res}
        img_m = self._f32(main_view["img"])
        B, _c, H, W_ = img_m.shape
        k = len(support)
        feat_m, pos_m = self._encode_image(img_m, None, normalize=False)
        img_s = torch.cat([self._f32(v["img"]) for v in support], 0)             # [k*B, 3, H, W], support-major
        assert img_s.shape[0] == k * B and img_s.shape[1:] == img_m.shape[1:], "support views must match the main view's shape"
        feat_s, pos_s = self._encode_image(img_s, None, normalize=False)
        feat_mk, pos_mk = feat_m.repeat(k, 1, 1), self._positions(k * B, H // 16, W_ // 16)
        hooks = self.cfg.hooks                      # decoder list indices hooks[i] - 1 (dpt_head.py:112)
        layers = sorted({hk - 1 for hk in hooks[1:]})
        d1, d2 = self._decode_stereo(feat_mk, feat_s, pos_mk, pos_s, layers=layers)
        ts = [[H, W_]] * (k * B)
        for res, feat, dec in ((main_res, feat_mk, d1), (supp_res, feat_s, d2)):
            toks = [feat] + [None if t is None else t[:, 1:, :] for t in dec]
            pts = self.head_pts(toks, ts)
            pose = self.head_pose_s(dec[-1][:, 0, :])
            for j in range(k):
                sl = slice(j * B, (j + 1) * B)
                res.append({"pts3d_pred": pts["pts3d"][sl], "conf": pts["conf"][sl],
                            "relative_pose": pose["pose"][sl], "relative_pose_conf": pose["conf"][sl]})
        return {"main_views": main_res, "support_views": supp_res}

    __call__ = forward

    # ------------------------------------------------------------------ introspection
    def flops_per_pair(self, H: int, W_: int) -> float:
        return float(self.lib.sta_flops_per_pair(self._h, H, W_))

    def enable_stage_timing(self, on: bool = True):
        _lib.check(self.lib.sta_enable_stage_timing(self._h, int(on)))

    def stage_ms(self):
        ms = (C.c_float * 4)()
        _lib.check(self.lib.sta_get_stage_ms(self._h, ms))
        return dict(zip(("encode", "decode", "pose", "dpt"), [float(x) for x in ms]))

    def kernel_timing(self, on: bool = True):
        _lib.check(self.lib.sta_kernel_timing(self._h, int(on)))

    def kernel_timing_read(self, tile_family: int = 0):
        n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        _lib.check(self.lib.sta_kernel_timing_read(self._h, tile_family, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return int(n.value), float(ms.value), float(fl.value), float(by.value)

    def kernel_timing_records(self, cap: int = 16384):
        """Per-launch records since kernel_timing(2): list of (M, N, K, epilogue, a_mode, mx, family, ms)."""
        sh = (C.c_int * (6 * cap))(); ms = (C.c_float * cap)(); var = (C.c_int * cap)(); n = C.c_int()
        _lib.check(self.lib.sta_kernel_timing_dump_shapes(self._h, cap, sh, ms, var, C.byref(n)))
        return [tuple(sh[6 * i + q] for q in range(6)) + (var[i], float(ms[i])) for i in range(n.value)]

    def bench_gemm(self, M: int, N: int, K: int, iters: int = 20, tile: int = 0, ablation: int = 0) -> float:
        """tools/ only: needs the test-hooks build (`STAFrontend(..., lib=_lib.load_test())`); the product library does not export it."""
        ms = C.c_float()
        _lib.check(self.lib.sta_bench_gemm(self._h, M, N, K, iters, tile, ablation, C.byref(ms), self._stream()))
        return float(ms.value)

    def workspace_bytes(self) -> int:
        return int(self.lib.sta_workspace_bytes(self._h))


def rope2d_inplace(tokens: torch.Tensor, positions: torch.Tensor, base: float, fwd: float = 1.0):
    """curope.rope_2d drop-in (pos_embed/curope/curope.cpp:49-65): tokens (B,N,H,D) fp16 / fp32 / fp64 CUDA view (the dtypes
    kernels.cu:101 dispatches on) with stride(3)==1 and stride(2)==D, positions (B,N,2) int64 contiguous; rotates in place."""
    lib = _lib.load()
    assert tokens.dim() == 4, "tokens must have 4 dimensions"
    assert positions.dim() == 3, "positions must have 3 dimensions"
    assert tokens.size(0) == positions.size(0), "batch size differs between tokens & positions"
    assert tokens.size(1) == positions.size(1), "seq_length differs between tokens & positions"
    assert positions.size(2) == 2, "positions.shape[2] must be equal to 2"
    assert tokens.is_cuda and positions.is_cuda, "tokens and positions must be on the GPU"
    dt = {torch.float32: 0, torch.float16: 1, torch.float64: 2}.get(tokens.dtype)
    assert dt is not None, f"rope_2d: unsupported token dtype {tokens.dtype}"       # (AT_DISPATCH_FLOATING_TYPES_AND_HALF)
    assert positions.dtype == torch.int64
    B, N, Hh, D = tokens.shape
    assert tokens.stride(3) == 1 and tokens.stride(2) == D, "tokens are not contiguous"
    assert positions.is_contiguous(), "positions are not contiguous"
    assert D % 4 == 0, "token dim must be multiple of 4"
    _lib.check(lib.sta_rope2d_inplace_dtype(tokens.data_ptr(), dt, tokens.stride(0), tokens.stride(1), positions.data_ptr(),
                                            B, N, Hh, D, float(base), float(fwd), _stream_ptr(tokens.device)))
    return tokens
