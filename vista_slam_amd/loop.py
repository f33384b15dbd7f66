"""Loop candidates on the GPU: ORB keypoints and descriptors, a bag-of-words vector from a vocabulary tree and its L1 scores against
the earlier keyframes - what `vista_slam/loop_detector.py` does per keyframe with cv2.ORB_create().detectAndCompute, DBoW3 and Python
loops on the CPU.  With it a keyframe's grey frame goes from `preprocess.process_image` to its loop candidates without touching the
host, apart from the one readback the caller branches on.

    slam.lc_detector = loop.LoopDetector(slam.frontend, cfg.vocab_path, loop_dist_min, loop_nms, loop_cand_thresh_neighbor)

The contract restates the documented algorithms in integer and float64 terms and is written out in include/sta_mi355.h; the yardstick
is the numpy restatement tests/loop_cases.py.  It is not cv2 and not DBoW3: the stated differences are in the header and in DESIGN.md
section 9.  In particular OpenCV's learned 256-pair comparison table is not part of this package: `pattern=None` is the seeded
procedural table `default_pattern()`, and a caller who wants the words of a vocabulary trained on cv2's ORB (ORBvoc.txt) passes that
table as `pattern=`.  Kernels: csrc/loop.h.  `plan` holds every size and refusal and needs no GPU; the three device calls
(`sta_orb_extract`, `sta_bow_transform`, `sta_bow_score`) take the caller's buffers: the library allocates nothing, copies nothing to
the host and never synchronises.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, flow
from .sta_frontend import STAFrontend

MAX_LEVELS, MAX_FEATURES, MAX_K, MAX_DEPTH = 8, 4096, 64, 10
NFEATURES, NLEVELS, FAST_THRESHOLD, EDGE = 500, 8, 20, 31
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)

_TRIG = None


def trig_table() -> np.ndarray:
    """int32 [720, 2] = rint(2^30 (cos, sin)(j * 0.5 degrees)): the only trigonometry of the contract, computed here once with numpy
    and handed to the library (and to the restatement) as data."""
    global _TRIG
    if _TRIG is None:
        ang = np.deg2rad(np.arange(720, dtype=np.float64) * 0.5)
        _TRIG = np.ascontiguousarray(np.rint(np.stack([np.cos(ang), np.sin(ang)], 1) * float(1 << 30)).astype(np.int32))
        _TRIG.setflags(write=False)
    return _TRIG


def default_pattern(seed: int = 12345) -> np.ndarray:
    """The procedural comparison table, int8 [256, 4] rows (x1, y1, x2, y2) in [-13, 13]: a 31-bit linear congruential generator
    x <- (1103515245 x + 12345) mod 2^31 from `seed`, a coordinate = ((x >> 16) mod 27) - 13 of each next x; a row whose two points
    coincide is drawn again."""
    x = int(seed) & 0x7FFFFFFF
    rows = []
    while len(rows) < 256:
        r = []
        for _ in range(4):
            x = (1103515245 * x + 12345) & 0x7FFFFFFF
            r.append(((x >> 16) % 27) - 13)
        if (r[0], r[1]) != (r[2], r[3]):
            rows.append(r)
    return np.array(rows, np.int8)


def check_pattern(pattern) -> np.ndarray:
    p = np.asarray(pattern)
    if p.shape != (256, 4) or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"pattern is an integer [256, 4] table of (x1, y1, x2, y2) (got {p.dtype} {p.shape})")
    if np.abs(p.astype(np.int64)).max() > 13:
        raise ValueError(f"every pattern value must lie in [-13, 13] (got {int(p.min())} .. {int(p.max())}): a rotated point must stay "
                         f"inside the edge of 22 pixels")
    return np.ascontiguousarray(p.astype(np.int8))


class Plan(NamedTuple):
    """The sizes of the extraction at one frame size: `sizes[l]` = (H_l, W_l) and `nfeat[l]` for all nlevels; the first `built` levels
    exist, `offsets[l]` = byte offset of a built level in a plane of `plane_bytes`; `rows` = the rows of the outputs;
    `workspace_bytes` / `bow_workspace_bytes` = the scratch of `sta_orb_extract` / of `sta_bow_transform` on `rows` descriptors."""
    H: int
    W: int
    nfeatures: int
    nlevels: int
    fast_threshold: int
    edge: int
    built: int
    sizes: Tuple[Tuple[int, int], ...]
    nfeat: Tuple[int, ...]
    offsets: Tuple[int, ...]
    plane_bytes: int
    workspace_bytes: int
    rows: int
    bow_workspace_bytes: int


def plan(H: int, W: int, nfeatures: int = NFEATURES, nlevels: int = NLEVELS, fast_threshold: int = FAST_THRESHOLD, edge: int = EDGE) -> Plan:
    """Every size and refusal of the extraction, on the host (`sta_orb_plan`; no GPU).  ValueError, with the numbers in the message, for
    nlevels outside [1, 8], nfeatures outside [1, 4096], edge outside [22, 64], fast_threshold outside [1, 254], H or W <= 2 edge,
    H * W above 2^21."""
    out = (C.c_int64 * 40)()
    lib = _lib.load()
    if lib.sta_orb_plan(int(H), int(W), int(nfeatures), int(nlevels), int(fast_threshold), int(edge), out) != 0:
        raise ValueError((lib.sta_last_error() or b"sta_orb_plan failed").decode())
    n, built = int(out[0]), int(out[1])
    return Plan(int(H), int(W), int(nfeatures), n, int(fast_threshold), int(edge), built,
                tuple((int(out[2 + l]), int(out[10 + l])) for l in range(n)), tuple(int(out[18 + l]) for l in range(n)),
                tuple(int(out[26 + l]) for l in range(built)), int(out[34]), int(out[35]), int(out[36]), int(out[37]))


def _dev(frontend: STAFrontend, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(frontend.device)     # (a copy: the cached tables are read-only)


class Extractor:
    """The device side of `orb` at fixed parameters: the trig and pattern tables and one workspace, kept between calls."""

    def __init__(self, frontend: STAFrontend, nfeatures: int = NFEATURES, nlevels: int = NLEVELS, fast_threshold: int = FAST_THRESHOLD,
                 edge: int = EDGE, pattern=None):
        self.frontend = frontend
        self.params = (int(nfeatures), int(nlevels), int(fast_threshold), int(edge))
        self.pattern = check_pattern(default_pattern() if pattern is None else pattern)
        self._trig = _dev(frontend, trig_table())
        self._pattern = _dev(frontend, self.pattern)
        self._ws = None

    def plan(self, H: int, W: int) -> Plan:
        return plan(H, W, *self.params)

    def extract(self, image, out=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, Plan]:
        """-> (kp int32 [rows,4], resp int64 [rows], desc uint8 [rows,32], n int32 [1], plan), all on the device; rows >= n are not
        written and n is not read here."""
        fe = self.frontend
        src = flow._frames(fe, image)
        if src.shape[0] != 1:
            raise ValueError(f"orb takes one frame (got {src.shape[0]})")
        _, H, W = src.shape
        p = self.plan(H, W)
        if self._ws is None or self._ws.numel() < p.workspace_bytes:
            self._ws = torch.empty(p.workspace_bytes, device=fe.device, dtype=torch.uint8)
        if out is None:
            out = (torch.empty(p.rows, 4, device=fe.device, dtype=torch.int32), torch.empty(p.rows, device=fe.device, dtype=torch.int64),
                   torch.empty(p.rows, 32, device=fe.device, dtype=torch.uint8), torch.empty(1, device=fe.device, dtype=torch.int32))
        kp, resp, desc, n = out
        _lib.check(fe.lib.sta_orb_extract(fe._h, src.data_ptr(), 0 if src.dtype == torch.uint8 else 1, H, W, *self.params, self._trig.data_ptr(),
                                          self._pattern.data_ptr(), self._ws.data_ptr(), self._ws.numel(), kp.data_ptr(), resp.data_ptr(),
                                          desc.data_ptr(), n.data_ptr(), fe._stream()))
        # (nothing is held back for the launches: they run on torch's current stream, so the allocator's reuse of `src` is ordered behind them)
        return kp, resp, desc, n, p


def orb(frontend: STAFrontend, image, nfeatures: int = NFEATURES, nlevels: int = NLEVELS, fast_threshold: int = FAST_THRESHOLD, edge: int = EDGE,
        pattern=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One frame (see `flow._frames` for what a frame may be) -> device tensors kp int32 [n,4] = (x, y, level, angle bin) in the level's
    own pixels, resp int64 [n], desc uint8 [n,32], level-major and by response within a level.  Reads n back once to cut the rows.  A
    utility: every call builds an `Extractor` (uploads the two tables, allocates the workspace); a caller with many frames keeps one
    `Extractor` and calls `extract`."""
    kp, resp, desc, n, _ = Extractor(frontend, nfeatures, nlevels, fast_threshold, edge, pattern).extract(image)
    k = int(n.item())
    return kp[:k], resp[:k], desc[:k]


class BowVector:
    """A bag-of-words vector on the device: `words` / `counts` / `vals` hold `n` (int32 [1], device) entries, the words ascending."""

    def __init__(self, words: torch.Tensor, counts: torch.Tensor, vals: torch.Tensor, n: torch.Tensor):
        self.words, self.counts, self.vals, self.n = words, counts, vals, n

    def numpy(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        k = int(self.n.item())
        return self.words[:k].cpu().numpy(), self.counts[:k].cpu().numpy(), self.vals[:k].cpu().numpy()


class Vocabulary:
    """A DBoW-style vocabulary tree as five arrays (include/sta_mi355.h): node 0 is the root, siblings are contiguous and keep file
    order, children follow their parent.  L1 scoring and TF-IDF weighting only."""

    def __init__(self, node_desc, child_first, child_count, word_of, word_weight, k: int, L: int):
        self.node_desc, self.child_first, self.child_count, self.word_of, self.word_weight = node_desc, child_first, child_count, word_of, word_weight
        self.k, self.L = int(k), int(L)
        self.frontend = None
        self._dev = None

    @property
    def n_nodes(self) -> int:
        return len(self.child_first)

    @property
    def n_words(self) -> int:
        return len(self.word_weight)

    @classmethod
    def from_arrays(cls, node_desc, child_first, child_count, word_of, word_weight) -> "Vocabulary":
        nd = np.ascontiguousarray(node_desc, np.uint8)
        cf, cc, wo = (np.ascontiguousarray(a, np.int32) for a in (child_first, child_count, word_of))
        ww = np.ascontiguousarray(word_weight, np.float64)
        n = len(cf)
        if n < 1 or nd.shape != (n, 32) or cc.shape != (n,) or wo.shape != (n,) or ww.ndim != 1:
            raise ValueError(f"a vocabulary is node_desc [n,32], child_first / child_count / word_of [n], word_weight [n_words] with n >= 1 "
                             f"(got {nd.shape}, {cf.shape}, {cc.shape}, {wo.shape}, {ww.shape})")
        if cc.min() < 0 or cc.max() > MAX_K:
            raise ValueError(f"a node has 0 .. {MAX_K} children (got {int(cc.min())} .. {int(cc.max())})")
        inner = np.flatnonzero(cc > 0)
        if inner.size and ((cf[inner] <= inner).any() or (cf[inner].astype(np.int64) + cc[inner] > n).any()):
            raise ValueError("children follow their parent and lie inside the arrays: child_first > the node's index, child_first + child_count <= n")
        if (wo[inner] != -1).any():
            raise ValueError("word_of is -1 for an inner node")
        leaves = np.flatnonzero(cc == 0)
        lw = wo[leaves]
        if ((lw < -1) | (lw >= len(ww))).any():
            raise ValueError(f"word_of of a leaf lies in [-1, {len(ww)})")
        depth = np.zeros(n, np.int64)
        for i in inner:                                  # ascending: a parent comes before its children
            depth[cf[i]:cf[i] + cc[i]] = depth[i] + 1
        if depth.max() > MAX_DEPTH:
            raise ValueError(f"the tree is {int(depth.max())} deep, above the limit of {MAX_DEPTH}")
        if not np.isfinite(ww).all():
            raise ValueError("word weights must be finite")
        return cls(nd, cf, cc, wo, ww, int(cc.max()) if n > 1 else 0, int(depth.max()))

    @classmethod
    def load(cls, path, frontend: Optional[STAFrontend] = None) -> "Vocabulary":
        """An .npz of the five arrays, or the text format of ORBvoc.txt: the first line `k L scoring weighting`, every further line
        `parent is_leaf b0 ... b31 weight`; node ids run from 1 in file order (0 is the root), word ids follow leaf order."""
        path = str(path)
        if path.endswith(".npz"):
            with np.load(path) as z:
                v = cls.from_arrays(z["node_desc"], z["child_first"], z["child_count"], z["word_of"], z["word_weight"])
            return v.bind(frontend) if frontend is not None else v
        with open(path) as f:
            head = f.readline().split()
            if len(head) != 4:
                raise ValueError(f"{path}: the first line is `k L scoring weighting` (got {len(head)} fields)")
            k, L, scoring, weighting = (int(t) for t in head)
            if scoring != 0 or weighting != 0:
                raise ValueError(f"{path}: only L1 scoring (0) with TF-IDF weighting (0) is supported (got scoring {scoring}, weighting {weighting})")
            if not (1 <= k <= MAX_K and 0 <= L <= MAX_DEPTH):
                raise ValueError(f"{path}: k must lie in [1, {MAX_K}] and L in [0, {MAX_DEPTH}] (got k = {k}, L = {L})")
            rows = [ln.split() for ln in f if ln.strip()]
        n = len(rows) + 1
        if any(len(r) != 35 for r in rows):
            bad = next(i for i, r in enumerate(rows) if len(r) != 35)
            raise ValueError(f"{path}: line {bad + 2} has {len(rows[bad])} fields, a node line has 35")
        parent = np.array([int(r[0]) for r in rows], np.int64)
        leaf = np.array([int(r[1]) != 0 for r in rows], bool)
        desc = np.array([[int(t) for t in r[2:34]] for r in rows], np.int64).reshape(-1, 32)
        weight = np.array([float(r[34]) for r in rows], np.float64)
        if rows and (parent.min() < 0 or (parent >= np.arange(1, n)).any() or desc.min() < 0 or desc.max() > 255):
            raise ValueError(f"{path}: a node's parent comes before it and descriptor bytes lie in [0, 255]")
        kids: List[List[int]] = [[] for _ in range(n)]
        for i, p in enumerate(parent):
            kids[p].append(i + 1)
        order = [0]
        for node in order:                               # breadth first: siblings contiguous, in file order, behind their parent
            order.extend(kids[node])
        new = np.empty(n, np.int64)
        new[order] = np.arange(n)
        node_desc = np.zeros((n, 32), np.uint8)
        child_first, child_count, word_of = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
        words = 0
        word_weight = []
        for i in range(1, n):
            node_desc[new[i]] = desc[i - 1]
            if leaf[i - 1]:
                if kids[i]:
                    raise ValueError(f"{path}: node {i} is marked a leaf and has children")
                word_of[new[i]] = words
                word_weight.append(weight[i - 1])
                words += 1
        for i in range(n):
            if kids[i]:
                child_first[new[i]], child_count[new[i]] = new[kids[i][0]], len(kids[i])
        v = cls.from_arrays(node_desc, child_first, child_count, word_of, np.array(word_weight, np.float64))
        v.k, v.L = k, L
        return v.bind(frontend) if frontend is not None else v

    def save(self, path):
        np.savez(str(path), node_desc=self.node_desc, child_first=self.child_first, child_count=self.child_count, word_of=self.word_of,
                 word_weight=self.word_weight)

    def bind(self, frontend: STAFrontend) -> "Vocabulary":
        """Upload the arrays to the frontend's device; `transform` and `score` run there."""
        if self.frontend is not frontend:
            self.frontend = frontend
            ww = self.word_weight if self.n_words else np.zeros(1, np.float64)          # (a device pointer to hand over)
            self._dev = tuple(_dev(frontend, a) for a in (self.node_desc, self.child_first, self.child_count, self.word_of, ww))
            self._ws = None
        return self

    def _need(self) -> STAFrontend:
        if self.frontend is None:
            raise RuntimeError("the vocabulary is not on a device: call bind(frontend) first")
        return self.frontend

    def transform_into(self, desc: torch.Tensor, n: Optional[torch.Tensor], words: torch.Tensor, counts: torch.Tensor, vals: torch.Tensor,
                       n_words: torch.Tensor):
        """`sta_bow_transform` into the caller's tensors (each of desc.shape[0] entries); nothing is allocated once the workspace exists."""
        fe = self._need()
        cap = desc.shape[0]
        if self._ws is None or self._ws.numel() < 4 * cap:
            self._ws = torch.empty(4 * cap, device=fe.device, dtype=torch.uint8)
        d = self._dev
        _lib.check(fe.lib.sta_bow_transform(fe._h, desc.data_ptr(), None if n is None else n.data_ptr(), cap, d[0].data_ptr(), d[1].data_ptr(),
                                            d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), self.n_nodes, self.n_words, self._ws.data_ptr(),
                                            self._ws.numel(), words.data_ptr(), counts.data_ptr(), vals.data_ptr(), n_words.data_ptr(), fe._stream()))

    def transform(self, desc, n: Optional[torch.Tensor] = None) -> BowVector:
        """desc uint8 [n,32] (numpy or device; at least one row) -> its BowVector; n = a device int32 count of the rows that hold descriptors."""
        fe = self._need()
        if isinstance(desc, np.ndarray):
            desc = torch.from_numpy(np.ascontiguousarray(desc))
        if desc.dtype != torch.uint8 or desc.dim() != 2 or desc.shape[1] != 32 or desc.shape[0] < 1:
            raise ValueError(f"descriptors are uint8 [n,32] with n >= 1 (got {desc.dtype} {tuple(desc.shape)})")
        desc = desc.to(fe.device).contiguous()
        cap = desc.shape[0]
        v = BowVector(torch.empty(cap, device=fe.device, dtype=torch.int32), torch.empty(cap, device=fe.device, dtype=torch.int32),
                      torch.empty(cap, device=fe.device, dtype=torch.float64), torch.empty(1, device=fe.device, dtype=torch.int32))
        self.transform_into(desc, n, v.words, v.counts, v.vals, v.n)
        return v

    def score(self, a: BowVector, b: BowVector) -> float:
        """DBoW's L1 score of two vectors of any two capacities (`sta_bow_score` with `b` as a database of one row; reads one double
        back).  Symmetric in its arguments up to the summation order."""
        fe = self._need()
        sim = torch.empty(1, device=fe.device, dtype=torch.float64)
        row = torch.zeros(1, device=fe.device, dtype=torch.int32)
        _lib.check(fe.lib.sta_bow_score(fe._h, a.words.data_ptr(), a.vals.data_ptr(), a.n.data_ptr(), a.words.shape[0], b.words.data_ptr(),
                                        b.vals.data_ptr(), b.n.data_ptr(), 1, b.words.shape[0], row.data_ptr(), 1, sim.data_ptr(), fe._stream()))
        return float(sim.item())


def candidates(present: Sequence[bool], sim: Sequence[float], i: int, farthest_neighbor: int, loop_dist_min: int, loop_nms: int,
               loop_cand_thresh_neighbor: int) -> List[Tuple[int, float]]:
    """Lines 26-48 of the reference's detect_loop on the host, statement for statement: present[j] = view j has a BoW vector
    (j <= i), sim[j] = its score against view i (j < i)."""
    loop_farthest_neighbor = max(0, i - loop_cand_thresh_neighbor)
    neighbor_sims = []
    for j in range(loop_farthest_neighbor, i):
        if not present[i] or not present[j]:
            continue
        neighbor_sims.append(sim[j])
    sim_thresh = 1.0 if len(neighbor_sims) == 0 else min(neighbor_sims)
    last_edge = farthest_neighbor
    out = []
    for j in reversed(range(0, farthest_neighbor)):
        if last_edge - j > loop_nms and i - j > loop_dist_min:
            if not present[i] or not present[j]:
                continue
            similarity = sim[j]
            if similarity > sim_thresh:
                out.append((j, similarity))
                last_edge = j
    return sorted(out, key=lambda x: x[1], reverse=True)


class LoopDetector:
    """`vista_slam.loop_detector.LoopDetector` on the GPU, with its surface: the attributes `loop_dist_min`, `loop_nms`,
    `loop_cand_thresh_neighbor`, `bow_feats`; `compute_bow_feat(image)`, `detect_loop(image, farthest_neighbor)`; and `reset()`.  An image
    is the numpy uint8 [H,W] the reference hands over, a device uint8 tensor, or `process_image(...)['gray']`.  The vectors of all views
    live in one device database [max_views, rows] (doubled, outside the device calls, when it is full); `detect_loop` scores the new view
    against all earlier ones in one launch and reads back once: the i similarities and the view's descriptor count."""

    def __init__(self, frontend: STAFrontend, vocab, loop_dist_min: int, loop_nms: int, loop_cand_thresh_neighbor: int, *,
                 nfeatures: int = NFEATURES, nlevels: int = NLEVELS, fast_threshold: int = FAST_THRESHOLD, edge: int = EDGE, pattern=None,
                 max_views: int = 512):
        self.frontend = frontend
        self.vocab = (vocab if isinstance(vocab, Vocabulary) else Vocabulary.load(vocab)).bind(frontend)
        self.loop_dist_min, self.loop_nms, self.loop_cand_thresh_neighbor = loop_dist_min, loop_nms, loop_cand_thresh_neighbor
        self.extractor = Extractor(frontend, nfeatures, nlevels, fast_threshold, edge, pattern)
        if max_views < 1:
            raise ValueError(f"max_views must be positive (got {max_views})")
        self.max_views = int(max_views)
        self._db, self._size = None, None
        self.reset()

    def reset(self):
        self.bow_feats: List[Optional[BowVector]] = []
        self.last = None                    # (sim_thresh inputs) of the most recent detect_loop: the similarities read back

    def _alloc(self, rows: int, views: int):
        dev = self.frontend.device
        return {"words": torch.empty(views, rows, device=dev, dtype=torch.int32), "counts": torch.empty(views, rows, device=dev, dtype=torch.int32),
                "vals": torch.empty(views, rows, device=dev, dtype=torch.float64), "n": torch.zeros(views, device=dev, dtype=torch.int32),
                "ndesc": torch.zeros(views, device=dev, dtype=torch.int32), "sim": torch.empty(views + 1, device=dev, dtype=torch.float64),
                "rows": torch.arange(views, device=dev, dtype=torch.int32),
                "kp": torch.empty(rows, 4, device=dev, dtype=torch.int32), "resp": torch.empty(rows, device=dev, dtype=torch.int64),
                "desc": torch.empty(rows, 32, device=dev, dtype=torch.uint8)}

    def _room(self, rows: int, i: int, size: Tuple[int, int]):
        """The database with a row for view i (allocation and growth happen here, outside the device calls).  The first view after a
        `reset()` sets the frame size; a view of another size is refused (its words would come from another set of levels)."""
        if i == 0:
            self._size = size
        if size != self._size:
            raise ValueError(f"a frame of {size[0]} x {size[1]} after frames of {self._size[0]} x {self._size[1]}: reset() before changing the frame size")
        if self._db is None or self._db["words"].shape[1] != rows:
            self._db = self._alloc(rows, self.max_views)
        db = self._db
        if i >= db["n"].shape[0]:
            big = self._alloc(rows, 2 * db["n"].shape[0])
            for key in ("words", "counts", "vals", "n", "ndesc"):
                big[key][:db[key].shape[0]].copy_(db[key])
            self._db = db = big
            self.max_views = db["n"].shape[0]
        return db

    def _append(self, image) -> int:
        """ORB and the BoW transform of one view into database row i = len(bow_feats); nothing is read back."""
        i = len(self.bow_feats)
        src = flow._frames(self.frontend, image)
        p = self.extractor.plan(src.shape[1], src.shape[2])
        db = self._room(p.rows, i, (int(src.shape[1]), int(src.shape[2])))
        n = db["ndesc"][i:i + 1]
        self.extractor.extract(src, out=(db["kp"], db["resp"], db["desc"], n))
        self.vocab.transform_into(db["desc"], n, db["words"][i], db["counts"][i], db["vals"][i], db["n"][i:i + 1])
        return i

    def _vector(self, i: int) -> BowVector:
        db = self._db
        return BowVector(db["words"][i], db["counts"][i], db["vals"][i], db["n"][i:i + 1])

    def compute_bow_feat(self, image) -> Optional[BowVector]:
        i = self._append(image)
        n_desc = int(self._db["ndesc"][i].item())                    # the readback of this call: None iff the frame has no descriptor
        self.bow_feats.append(self._vector(i) if n_desc > 0 else None)
        return self.bow_feats[i]

    def score_views(self, i: int, m: int) -> torch.Tensor:
        """One `sta_bow_score` launch: view i of the database against its views 0 .. m - 1 -> their similarities, float64 [m] on the
        device (a view of the detector's own buffer: the next call overwrites it).  Nothing is read back."""
        fe, db = self.frontend, self._db
        if db is None or not (0 <= i < db["n"].shape[0] and 0 <= m <= db["n"].shape[0]):
            raise ValueError(f"view {i} against the first {m} views of a database of {0 if db is None else db['n'].shape[0]} rows")
        q, cap = self._vector(i), db["words"].shape[1]
        _lib.check(fe.lib.sta_bow_score(fe._h, q.words.data_ptr(), q.vals.data_ptr(), q.n.data_ptr(), cap, db["words"].data_ptr(), db["vals"].data_ptr(),
                                        db["n"].data_ptr(), db["n"].shape[0], cap, db["rows"].data_ptr(), m, db["sim"].data_ptr(), fe._stream()))
        return db["sim"][:m]

    def detect_loop(self, image, farthest_neighbor: int) -> List[Tuple[int, float]]:
        i = self._append(image)
        db = self._db
        q = self._vector(i)
        self.score_views(i, i)
        db["sim"][i:i + 1].copy_(db["ndesc"][i:i + 1])                # the descriptor count rides along (exact in float64)
        host = db["sim"][:i + 1].tolist()                             # THE readback of the call
        self.bow_feats.append(q if host[i] > 0 else None)
        self.last = host[:i]
        return candidates([f is not None for f in self.bow_feats], host, i, farthest_neighbor, self.loop_dist_min, self.loop_nms,
                          self.loop_cand_thresh_neighbor)
