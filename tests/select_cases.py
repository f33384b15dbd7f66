"""Token selections from per-pixel maps (sta_select_patches, include/sta_mi355.h): the numpy restatement of the contract (`pool`,
`select`) and the case inventory shared by tests/test_select_cpu.py (the restatement against a brute-force double loop) and
tests/test_select_gpu.py (the kernels against the restatement, `array_equal` everywhere).

The contract is integer arithmetic, so the restatement IS the definition: no fixture, no tolerance.
  score   uint8 / bool: non-zero bytes of the 16x16 patch (zero bytes with invert); float32 with thres: pixels with v > thres
          (strict, false for NaN on either side; invert negates the predicate); float32 without thres: sum of
          rint(clamp(v, 0, 32767) * 256), half to even, NaN / -inf / negatives -> 0, +inf -> 32767
  rule    min_score = s: score >= s, then dilated by `margin` patches (Chebyshev, inside the entry's grid);
          top_k = k: the k largest scores, the lower patch index first among equals
  output  packed per entry at off_b = sum of N_a, a < b: score, index (ascending, -1 tail), pos ((y, x), -1 tail), n_sel, window
          ((y0, x0, h, w) of the bounding rectangle, zeros when empty)
"""
import numpy as np

SCORE_MAX = 256 * 8388352          # 2 147 418 112 < 2^31: every pixel of a patch at the clamp
PIXEL_MAX = 8388352                # rint(32767 * 256)


def pool(m, thres=None, invert=False):
    """One map [H, W] (bool, uint8 or float32) -> its [H/16, W/16] int32 patch scores."""
    m = np.asarray(m)
    H, W = m.shape
    assert H % 16 == 0 and W % 16 == 0 and H >= 16 and W >= 16
    if m.dtype == np.float32 and thres is None:
        assert not invert
        with np.errstate(invalid="ignore"):
            v = np.where(m > 0, m, np.float32(0)).astype(np.float32)          # NaN, -inf, negatives -> 0
            v = np.minimum(v, np.float32(32767))
        px = np.rint(v * np.float32(256)).astype(np.int64)                     # exact product, half to even
    elif m.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            px = m > np.float32(thres)
        px = (~px if invert else px).astype(np.int64)
    else:
        assert m.dtype in (np.uint8, np.bool_) and thres is None
        px = ((m == 0) if invert else (m != 0)).astype(np.int64)
    s = px.reshape(H // 16, 16, W // 16, 16).sum(axis=(1, 3))
    assert s.min() >= 0 and s.max() <= SCORE_MAX
    return s.astype(np.int32)


def dilate(flag, r):
    """Chebyshev dilation of a bool grid by r patches, inside the grid."""
    hp, wp = flag.shape
    out = np.zeros_like(flag)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if abs(dy) >= hp or abs(dx) >= wp:          # the shift leaves the grid
                continue
            ys, yd = (slice(0, hp - dy), slice(dy, hp)) if dy >= 0 else (slice(-dy, hp), slice(0, hp + dy))
            xs, xd = (slice(0, wp - dx), slice(dx, wp)) if dx >= 0 else (slice(-dx, wp), slice(0, wp + dx))
            out[yd, xd] |= flag[ys, xs]
    return out


def select(scores, min_score=None, top_k=None, margin=0):
    """scores: one [hp_b, wp_b] int32 grid per entry -> dict of the packed outputs of one call."""
    assert (min_score is None) != (top_k is None)
    B = len(scores)
    ks = None if top_k is None else ([int(top_k)] * B if np.isscalar(top_k) else [int(k) for k in top_k])
    total = sum(s.size for s in scores)
    out = {"score": np.concatenate([s.reshape(-1) for s in scores]).astype(np.int32),
           "index": np.full(total, -1, np.int64), "pos": np.full((total, 2), -1, np.int64),
           "n_sel": np.zeros(B, np.int32), "window": np.zeros((B, 4), np.int32), "off": np.zeros(B + 1, np.int64)}
    off = 0
    for b, s in enumerate(scores):
        hp, wp = s.shape
        if ks is None:
            flag = s >= min_score
            if margin:
                flag = dilate(flag, margin)
            idx = np.flatnonzero(flag.reshape(-1))
        else:
            assert margin == 0 and 1 <= ks[b] <= s.size
            order = np.argsort(-s.reshape(-1).astype(np.int64), kind="stable")      # stable: the lower index first among equals
            idx = np.sort(order[:ks[b]])
        n = idx.size
        out["index"][off:off + n] = idx
        out["pos"][off:off + n, 0] = idx // wp
        out["pos"][off:off + n, 1] = idx % wp
        out["n_sel"][b] = n
        if n:
            y, x = idx // wp, idx % wp
            out["window"][b] = (y.min(), x.min(), y.max() - y.min() + 1, x.max() - x.min() + 1)
        off += s.size
        out["off"][b + 1] = off
    return out


def expected(maps, thres=None, invert=False, min_score=None, top_k=None, margin=0):
    return select([pool(m, thres, invert) for m in maps], min_score=min_score, top_k=top_k, margin=margin)


# ----------------------------------------------------------------------------------------------------------------------
# builders: maps with chosen scores
def mask_from_scores(s, rng=None, value=1):
    """uint8 map whose patch (y, x) has exactly s[y, x] non-zero pixels (the first ones row-major, or random ones with rng)."""
    s = np.asarray(s)
    hp, wp = s.shape
    m = np.zeros((hp, 16, wp, 16), np.uint8)
    for y in range(hp):
        for x in range(wp):
            px = np.zeros(256, np.uint8)
            where = np.arange(256) if rng is None else rng.permutation(256)
            px[where[:int(s[y, x])]] = value
            m[y, :, x, :] = px.reshape(16, 16)
    return m.reshape(hp * 16, wp * 16)


def float_from_scores(s):
    """float32 map whose fixed-point patch sum is exactly s[y, x] <= SCORE_MAX: pixels at the clamp, then one with the rest / 256."""
    s = np.asarray(s, np.int64)
    hp, wp = s.shape
    m = np.zeros((hp, 16, wp, 16), np.float32)
    for y in range(hp):
        for x in range(wp):
            full, rest = divmod(int(s[y, x]), PIXEL_MAX)
            px = np.zeros(256, np.float32)
            px[:full] = 32767.0
            if rest:
                px[full] = np.float32(rest) / np.float32(256)          # exact: rest < 2^24
            m[y, :, x, :] = px.reshape(16, 16)
    return m.reshape(hp * 16, wp * 16)


def random_mask(H, W, seed):
    """uint8 0/1 map with a density of its own per patch, a few patches empty and a few full."""
    rng = np.random.default_rng(seed)
    hp, wp = H // 16, W // 16
    dens = rng.choice([0.0, 0.05, 0.3, 0.5, 0.7, 1.0], size=(hp, wp))
    return (rng.random((H, W)) < np.kron(dens, np.ones((16, 16)))).astype(np.uint8)


def hostile_float(H, W, seed):
    """float32 map with NaN, +-inf, negatives, values above 32767 and values at k / 512 (the ties of the fixed-point rounding)."""
    rng = np.random.default_rng(seed)
    m = (rng.random((H, W)) * 4 - 1).astype(np.float32)
    kind = rng.integers(0, 16, size=(H, W))
    m[kind == 0] = np.nan
    m[kind == 1] = np.inf
    m[kind == 2] = -np.inf
    m[kind == 3] = 40000.0
    m[kind == 4] = 32767.0
    ties = (rng.integers(0, 4096, size=(H, W)).astype(np.float32) * 2 + 1) / np.float32(512)       # odd / 512: exactly half way
    m[kind >= 12] = ties[kind >= 12]
    return m


def threshold_float(H, W, thres, seed):
    """float32 map with pixels exactly at thres, one ulp above and below it, NaN and +-inf."""
    rng = np.random.default_rng(seed)
    t = np.float32(thres)
    vals = np.array([t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf)), np.nan, np.inf, -np.inf,
                     t + 1, t - 1], np.float32)
    return vals[rng.integers(0, len(vals), size=(H, W))]


# ----------------------------------------------------------------------------------------------------------------------
# the inventory: name -> () -> (maps, keyword arguments)
GRIDS = [(16, 16), (16, 1024), (16, 1040), (16, 1008), (256, 256), (272, 240), (16, 4112), (48, 64), (80, 48), (1024, 2048)]
#          1 patch   64          65          63          256         255         257         12        15        8192
SMALL_GRIDS = GRIDS[:-1]


def _tie_scores(n, group, high):
    """A 1 x n score row: `high` patches at 200, the tie group at 100, every other patch at 50."""
    s = np.full((1, n), 50, np.int64)
    s[0, list(group)] = 100
    s[0, list(high)] = 200
    return s


def _corners(hp, wp):
    s = np.zeros((hp, wp), np.int64)
    s[0, 0] = s[0, wp - 1] = s[hp - 1, 0] = s[hp - 1, wp - 1] = 256
    return s


def _corner_pixels():
    maps = []
    for cy, cx in ((0, 0), (0, 15), (15, 0), (15, 15)):
        m = np.zeros((32, 48), np.uint8)
        m[16 + cy, 32 + cx] = 7          # patch (1, 2), one pixel in its corner
        maps.append(m)
    return maps


def _levels():
    s = np.array([[256, 0, 1, 255], [0, 256, 256, 1], [2, 0, 0, 256]], np.int64)
    return mask_from_scores(s, np.random.default_rng(5))


def _leak():
    full_last = mask_from_scores(np.array([[0, 0, 0, 0], [0, 0, 0, 0], [256, 256, 256, 256]]))
    full_first = mask_from_scores(np.array([[256, 256, 256, 256], [0, 0, 0, 0], [0, 0, 0, 0]]))
    empty = np.zeros((48, 64), np.uint8)
    return [full_last, empty, full_first, empty, full_last, full_first]


def _b32():
    return [random_mask(*GRIDS[i % len(GRIDS)], seed=100 + i) for i in range(32)]


def _radix(kind):
    p = np.arange(64, dtype=np.int64)
    if kind == "top":
        s = ((p * 37) % 128) << 24
    elif kind == "low":
        s = 0x12345600 + (p * 37) % 256
    else:
        s = np.zeros(64, np.int64)
        s[41] = SCORE_MAX
    return float_from_scores(s.reshape(1, 64))


CASES = {}
for _H, _W in GRIDS:
    _n = (_H // 16) * (_W // 16)
    CASES[f"grid_{_H}x{_W}_min"] = (lambda H=_H, W=_W: ([random_mask(H, W, H + W)], dict(min_score=100)))
    CASES[f"grid_{_H}x{_W}_margin"] = (lambda H=_H, W=_W: ([random_mask(H, W, H + W)], dict(min_score=256, margin=1)))
    CASES[f"grid_{_H}x{_W}_topk"] = (lambda H=_H, W=_W, n=_n: ([random_mask(H, W, H + W + 1)], dict(top_k=max(1, n // 2))))
CASES.update({
    "b32_mixed_min": lambda: (_b32(), dict(min_score=77, margin=2)),
    "b32_mixed_topk": lambda: (_b32(), dict(top_k=[1 + (7 * i) % ((GRIDS[i % len(GRIDS)][0] // 16) * (GRIDS[i % len(GRIDS)][1] // 16)) for i in range(32)])),
    "leak_min": lambda: (_leak(), dict(min_score=256)),
    "leak_margin1": lambda: (_leak(), dict(min_score=256, margin=1)),
    "leak_margin8": lambda: (_leak(), dict(min_score=256, margin=8)),
    "bytes_0_1_2_255": lambda: ([np.array([0, 1, 2, 255], np.uint8)[np.random.default_rng(3).integers(0, 4, size=(48, 64))]], dict(min_score=190)),
    "bytes_0_1_2_255_invert": lambda: ([np.array([0, 1, 2, 255], np.uint8)[np.random.default_rng(3).integers(0, 4, size=(48, 64))]], dict(min_score=66, invert=True)),
    "bool_invert": lambda: ([random_mask(80, 48, 9).astype(np.bool_)], dict(min_score=128, invert=True)),
    "corner_pixels": lambda: (_corner_pixels(), dict(min_score=1)),
    "thres_edges": lambda: ([threshold_float(48, 64, 0.5, 11), threshold_float(80, 48, 0.5, 12)], dict(thres=0.5, min_score=96)),
    "thres_edges_invert": lambda: ([threshold_float(48, 64, 0.5, 11)], dict(thres=0.5, invert=True, min_score=160)),
    "thres_nan": lambda: ([threshold_float(48, 64, 0.5, 13)], dict(thres=float("nan"), min_score=1)),
    "thres_nan_invert": lambda: ([threshold_float(48, 64, 0.5, 13)], dict(thres=float("nan"), invert=True, min_score=256)),
    "thres_topk": lambda: ([threshold_float(272, 240, -3.0, 14)], dict(thres=-3.0, top_k=100)),
    "sum_hostile_topk": lambda: ([hostile_float(48, 64, 21), hostile_float(272, 240, 22)], dict(top_k=[6, 127])),
    "sum_hostile_384x512": lambda: ([hostile_float(384, 512, 7)], dict(top_k=384)),          # the map of the CPU summation-order test
    "sum_hostile_min": lambda: ([hostile_float(80, 48, 23)], dict(min_score=400000000, margin=1)),
    "min_score_0": lambda: ([_levels()], dict(min_score=0)),
    "min_score_1": lambda: ([_levels()], dict(min_score=1)),
    "min_score_256": lambda: ([_levels()], dict(min_score=256)),
    "min_score_257": lambda: ([_levels(), _levels()], dict(min_score=257)),
    "topk_1": lambda: ([random_mask(48, 64, 31)], dict(top_k=1)),
    "topk_all": lambda: ([random_mask(48, 64, 31)], dict(top_k=12)),
    "topk_all_equal": lambda: ([np.ones((16, 4112), np.uint8), np.full((256, 256), 255, np.uint8)], dict(top_k=[200, 65])),
    "topk_radix_top_byte": lambda: ([_radix("top")], dict(top_k=20)),
    "topk_radix_low_byte": lambda: ([_radix("low")], dict(top_k=33)),
    "topk_radix_single_max": lambda: ([_radix("one"), _radix("one")], dict(top_k=[1, 3])),
})
for _r in (1, 4, 8):
    CASES[f"margin{_r}_corners"] = (lambda r=_r: ([mask_from_scores(_corners(17, 15)), mask_from_scores(_corners(3, 4)), mask_from_scores(_corners(1, 65))],
                                                   dict(min_score=256, margin=r)))
# tie groups at the k-th value that straddle patch 63 | 64 (a wave) and 255 | 256 (a chunk); three patches score higher, so the
# quota q = k - 3 ends before, at and behind the boundary
TIE_ROWS = {"wave": (range(60, 68), (0, 100, 256)), "chunk": (range(252, 260), (0, 100, 300))}
for _name, (_group, _high) in TIE_ROWS.items():
    for _q in (2, 4, 6):
        CASES[f"topk_tie_{_name}_q{_q}"] = (lambda g=_group, h=_high, q=_q: ([mask_from_scores(_tie_scores(514, g, h))], dict(top_k=3 + q)))
CASES["topk_ties_per_entry_k"] = lambda: ([mask_from_scores(_tie_scores(514, g, h)) for g, h in TIE_ROWS.values() for _ in range(3)],
                                          dict(top_k=[5, 7, 9, 5, 7, 9]))

LARGE = {n for n in CASES if "1024x2048" in n or n.startswith("b32")}      # millions of pixels: the CPU brute force pools these per patch, not per pixel

OUTPUTS = ("score", "index", "pos", "n_sel", "window")


def build(name):
    maps, kw = CASES[name]()
    return maps, kw
