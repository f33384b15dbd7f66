"""Host only: the numpy restatement of the selection contract (tests/select_cases.py) against an independent brute force on every
inventory case; the fixed-point score under two summation orders; and the argument checks of `vista_slam_amd.select.plan`.  These
pass without the kernels - the proof of the kernels is tests/test_select_gpu.py."""
import math

import numpy as np
import pytest

import select_cases as S


# ----------------------------------------------------------------------------------------------------------------------
# brute force: plain Python loops, no reshape, no sort of arrays
def _pixel(v, kind, thres, invert):
    if kind == "byte":
        return int((v == 0) if invert else (v != 0))
    if kind == "thres":
        hit = (not math.isnan(v)) and (not math.isnan(thres)) and v > thres
        return int(hit != invert)
    if math.isnan(v) or v <= 0:
        c = 0.0
    else:
        c = min(v, 32767.0)
    x = c * 256.0                               # exact in double too
    f = math.floor(x)
    if x - f > 0.5 or (x - f == 0.5 and f % 2 == 1):
        f += 1
    return int(f)


def brute_pool(m, thres, invert, per_pixel=True):
    H, W = m.shape
    kind = "byte" if m.dtype != np.float32 else ("sum" if thres is None else "thres")
    t = None if thres is None else float(np.float32(thres))
    rows = m.astype(np.float64).tolist() if (m.dtype == np.float32 and per_pixel) else (m.astype(np.int64).tolist() if per_pixel else None)
    out = [[0] * (W // 16) for _ in range(H // 16)]
    for py in range(H // 16):
        for px in range(W // 16):
            if per_pixel:
                s = 0
                for y in range(16 * py, 16 * py + 16):
                    row = rows[y]
                    for x in range(16 * px, 16 * px + 16):
                        s += _pixel(row[x], kind, t, invert)
            else:                               # the large cases are byte maps: count per patch
                assert kind == "byte"
                blk = m[16 * py:16 * py + 16, 16 * px:16 * px + 16]
                s = int(np.count_nonzero(blk == 0) if invert else np.count_nonzero(blk))
            out[py][px] = s
    return out


def brute_select(grid, min_score, k, margin):
    hp, wp = len(grid), len(grid[0])
    if k is None:
        chosen = set()
        for y in range(hp):
            for x in range(wp):
                if grid[y][x] >= min_score:
                    for yy in range(y - margin, y + margin + 1):
                        for xx in range(x - margin, x + margin + 1):
                            if 0 <= yy < hp and 0 <= xx < wp:
                                chosen.add(yy * wp + xx)
        idx = sorted(chosen)
    else:
        flat = [grid[y][x] for y in range(hp) for x in range(wp)]
        idx = sorted(sorted(range(hp * wp), key=lambda p: (-flat[p], p))[:k])
    win = (0, 0, 0, 0)
    if idx:
        ys, xs = [p // wp for p in idx], [p % wp for p in idx]
        win = (min(ys), min(xs), max(ys) - min(ys) + 1, max(xs) - min(xs) + 1)
    return idx, win


@pytest.mark.parametrize("name", list(S.CASES))
def test_restatement_against_brute_force(name):
    maps, kw = S.build(name)
    exp = S.expected(maps, **kw)
    B = len(maps)
    ks = kw.get("top_k")
    ks = None if ks is None else ([ks] * B if isinstance(ks, int) else list(ks))
    off = 0
    for b, m in enumerate(maps):
        grid = brute_pool(m, kw.get("thres"), kw.get("invert", False), per_pixel=name not in S.LARGE)
        hp, wp = len(grid), len(grid[0])
        n = hp * wp
        assert int(exp["off"][b]) == off                                        # slot offsets
        assert exp["score"][off:off + n].tolist() == [v for row in grid for v in row]
        idx, win = brute_select(grid, kw.get("min_score"), None if ks is None else ks[b], kw.get("margin", 0))
        assert int(exp["n_sel"][b]) == len(idx) and (ks is None or len(idx) == ks[b])
        assert exp["index"][off:off + len(idx)].tolist() == idx                 # ascending order, tie rule, margin
        assert exp["pos"][off:off + len(idx)].tolist() == [[p // wp, p % wp] for p in idx]
        assert (exp["index"][off + len(idx):off + n] == -1).all() and (exp["pos"][off + len(idx):off + n] == -1).all()      # -1 tails
        assert tuple(exp["window"][b].tolist()) == win
        off += n
    assert exp["index"].shape == (off,) and exp["pos"].shape == (off, 2)


def test_inventory_covers_what_it_claims():
    """The constructions do what their names say: tie groups straddle the boundaries with the quota on either side, the radix
    cases decide in one pass each, an empty selection and a full one exist."""
    for tag, (group, high) in S.TIE_ROWS.items():
        edge = 64 if tag == "wave" else 256
        assert min(group) < edge <= max(group)
        for q in (2, 4, 6):
            maps, kw = S.build(f"topk_tie_{tag}_q{q}")
            exp = S.expected(maps, **kw)
            got = exp["index"][:kw["top_k"]].tolist()
            assert got == sorted(list(high) + list(group)[:q])
        assert list(group)[1] < edge - 1 and list(group)[3] == edge - 1 and list(group)[5] > edge
    top = S.pool(S.build("topk_radix_top_byte")[0][0]).reshape(-1).astype(np.int64)
    assert ((top & 0xFFFFFF) == 0).all() and len(set((top >> 24).tolist())) > 32
    low = S.pool(S.build("topk_radix_low_byte")[0][0]).reshape(-1).astype(np.int64)
    assert len(set((low >> 8).tolist())) == 1 and len(set((low & 255).tolist())) > 32
    one = S.pool(S.build("topk_radix_single_max")[0][0]).reshape(-1)
    assert int(one.max()) == S.SCORE_MAX == 2147418112 and int((one > 0).sum()) == 1
    empty = S.expected(*S.build("min_score_257")[:1], min_score=257)
    assert (empty["n_sel"] == 0).all() and (empty["window"] == 0).all() and (empty["index"] == -1).all()
    full = S.expected(*S.build("min_score_0")[:1], min_score=0)
    assert full["n_sel"].tolist() == [12] and full["index"].tolist() == list(range(12))
    sizes = sorted((H // 16) * (W // 16) for H, W in S.GRIDS)
    assert sizes == [1, 12, 15, 63, 64, 65, 255, 256, 257, 8192]


def test_fixed_point_score_does_not_depend_on_summation_order():
    m = S.hostile_float(384, 512, 7)
    assert np.isnan(m).any() and np.isposinf(m).any() and np.isneginf(m).any() and (m < 0).any() and (m > 32767).any()
    frac = m[np.isfinite(m) & (m > 0) & (m < 32767)] * np.float32(512)
    assert ((frac == np.rint(frac)) & (frac % 2 == 1)).sum() > 1000          # pixels at odd / 512: the rounding ties
    a = S.pool(m)
    with np.errstate(invalid="ignore"):
        v = np.minimum(np.where(m > 0, m, np.float32(0)), np.float32(32767)).astype(np.float32)
    t = np.rint(v * np.float32(256)).astype(np.int64).reshape(24, 16, 32, 16)
    b = np.zeros((24, 32), np.int64)
    for r in reversed(range(16)):                # rows last to first, columns last to first
        for c in reversed(range(16)):
            b += t[:, r, :, c]
    assert np.array_equal(a, b.astype(np.int32))
    assert a.dtype == np.int32 and int(a.max()) <= S.SCORE_MAX


def test_half_to_even_at_the_ties():
    m = np.zeros((16, 16), np.float32)
    m[0, :4] = np.array([1, 3, 5, 7], np.float32) / np.float32(512)          # 0.5, 1.5, 2.5, 3.5 -> 0, 2, 2, 4
    assert int(S.pool(m)[0, 0]) == 8


# ----------------------------------------------------------------------------------------------------------------------
# select.plan: the refusals of the C entry, on the host
def _plan(*a, **k):
    from vista_slam_amd import select
    return select.plan(*a, **k)


def test_plan_offsets_for_mixed_frame_sizes():
    p = _plan([(48, 64), (16, 16), (272, 240), (1024, 2048)], "uint8", min_score=1, margin=3)
    assert p.off == (0, 12, 13, 268, 8460) and p.grids == ((3, 4), (1, 1), (17, 15), (64, 128))
    assert (p.dtype, p.mode, p.rule, p.min_score, p.margin, p.top_k) == (0, 0, 0, 1, 3, None)
    p = _plan([(48, 64), (80, 48)], "float32", top_k=5)
    assert (p.dtype, p.mode, p.rule, p.top_k) == (1, 1, 1, (5, 5))
    p = _plan([(48, 64)], "torch.float32", thres=0.25, invert=True, top_k=[12])
    assert (p.dtype, p.mode, p.invert, p.thres) == (1, 0, 1, 0.25)
    assert _plan([(48, 64)], "bool", invert=True, min_score=0).dtype == 0


@pytest.mark.parametrize("shapes,dtype,kw,text", [
    ([], "uint8", dict(min_score=1), "1 .. 32 maps"),
    ([(16, 16)] * 33, "uint8", dict(min_score=1), "1 .. 32 maps"),
    ([(0, 16)], "uint8", dict(min_score=1), "multiples of 16"),
    ([(16, 24)], "uint8", dict(min_score=1), "multiples of 16"),
    ([(40, 16)], "uint8", dict(min_score=1), "multiples of 16"),
    ([(16, 16), (16, 8208 * 16)], "uint8", dict(min_score=1), "8208 patches"),
    ([(1040, 2048)], "uint8", dict(min_score=1), "above the limit of 8192"),
    ([(16, 16)], "float32", dict(min_score=1, invert=True), "invert is refused"),
    ([(16, 16)], "uint8", dict(min_score=1, thres=0.5), "thres applies to float32"),
    ([(16, 16)], "int32", dict(min_score=1), "bool, uint8 or float32"),
    ([(48, 64)], "uint8", dict(top_k=3, margin=1), "margin is refused with top_k"),
    ([(48, 64)], "uint8", dict(top_k=0), "top_k must lie in [1, 12]"),
    ([(48, 64), (16, 16)], "uint8", dict(top_k=[12, 2]), "entry 1: top_k must lie in [1, 1]"),
    ([(48, 64), (16, 16)], "uint8", dict(top_k=[12]), "one int per map"),
    ([(48, 64)], "uint8", dict(min_score=-1), "min_score must be >= 0"),
    ([(48, 64)], "uint8", dict(min_score=1, margin=9), "margin must lie in [0, 8]"),
    ([(48, 64)], "uint8", dict(min_score=1, margin=-1), "margin must lie in [0, 8]"),
    ([(48, 64)], "uint8", dict(), "exactly one of min_score and top_k"),
    ([(48, 64)], "uint8", dict(min_score=1, top_k=1), "exactly one of min_score and top_k"),
    ([(48, 64)], "float32", dict(min_score=1, addresses=[4098]), "4-byte aligned"),
    ([(48, 64, 3)], "uint8", dict(min_score=1), "a map is [H, W]"),
])
def test_plan_refuses(shapes, dtype, kw, text):
    with pytest.raises(ValueError) as e:
        _plan(shapes, dtype, **kw)
    assert text in str(e.value), str(e.value)


def test_plan_accepts_an_unaligned_byte_map():
    assert _plan([(48, 64)], "bool", min_score=1, addresses=[4097]).B == 1
