"""CPU: the yardstick of the keyframe gate checks itself, and `flow.plan` (host only).  1. the numpy restatement (tests/flow_cases.py)
against a deliberately naive second statement of the same contract - per-pixel Python loops, a dict for the suppression - on three
tiny frames, everything with array_equal.  2. the restatement really is Lucas-Kanade: corners of a procedural blob texture tracked
into the same texture sampled at shifted coordinates land on the true shift.  3. the sizes, offsets and refusals of `flow.plan`."""
import numpy as np
import pytest

import flow_cases as F

TINY = [(12, 16, 1), (17, 23, 2), (24, 32, 3)]


def _pair(H, W, seed):
    return F.blob_frame(H, W, seed=seed, n_blobs=14), F.blob_frame(H, W, (0.6, -0.3), seed=seed, n_blobs=14)


@pytest.mark.parametrize("H,W,seed", TINY)
def test_restatement_against_the_naive_statement(H, W, seed):
    a, b = _pair(H, W, seed)
    for win, max_level in ((5, 2), (5, 0), (21, 3)):
        p1, p2 = F.pyramid(a, win, max_level), F.naive_pyramid(a, win, max_level)
        assert len(p1) == len(p2) == len(F.level_sizes(H, W, win, max_level))
        assert all(np.array_equal(x, y) for x, y in zip(p1, p2)), (win, max_level)
    assert len(F.pyramid(a, 5, 2)) > 1                                   # the tiny frames do have levels at a small window
    fl = a.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(F.naive_pyramid(fl, 5, 2)[1], F.pyramid(fl, 5, 2)[1])
    n_corners = []
    for kw in (dict(), dict(min_distance=3, block_size=3), dict(max_corners=3, min_distance=2, block_size=5), dict(min_distance=1, quality=0.2)):
        c1, c2 = F.good_features(a, **kw), F.naive_good_features(a, **kw)
        assert c1.dtype == c2.dtype == np.float32 and np.array_equal(c1, c2), (kw, c1, c2)
        n_corners.append(len(c1))
    assert n_corners[1] >= 2 and n_corners[2] == 3, n_corners
    flat = np.full((H, W), 77, np.uint8)
    assert len(F.good_features(flat)) == 0 and len(F.naive_good_features(flat)) == 0
    pts = np.concatenate([F.good_features(a, min_distance=3, block_size=3)[:4],
                          np.array([[0, 0], [W - 1, H - 1], [3.3, 4.7], [-9.0, 2.0], [W + 2.5, 1.0]], np.float32)])
    seen = set()
    for win, max_level in ((5, 2), (7, 1)):
        r1 = F.track(a, b, pts, win=win, max_level=max_level)
        r2 = F.naive_track(a, b, pts, win=win, max_level=max_level)
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]), (win, r1, r2)
        seen |= set(r1[1].tolist())
    assert seen == {0, 1}                                                # both outcomes are exercised


@pytest.mark.parametrize("H,W", [(96, 128), (224, 224)])
@pytest.mark.parametrize("shift", [(1.25, -0.5), (5.5, 3.25)])
def test_restatement_is_lucas_kanade(H, W, shift):
    a, b = F.blob_frame(H, W), F.blob_frame(H, W, shift)
    pts = F.good_features(a)
    assert len(pts) >= 40
    nxt, st = F.track(a, b, pts)
    good = st == 1
    err = np.hypot(nxt[good, 0] - pts[good, 0] - shift[0], nxt[good, 1] - pts[good, 1] - shift[1])
    print(f"[flow] {H}x{W} shift {shift}: {int(good.sum())} of {len(pts)} tracked, median error {np.median(err):.4f} px, worst {err.max():.3f} px")
    assert F.LK_MEDIAN_BOUND < 0.25
    assert np.median(err) < F.LK_MEDIAN_BOUND, np.median(err)
    assert good.sum() >= 0.9 * len(pts), (int(good.sum()), len(pts))
    n, n_good, total = F.disparity(pts, nxt, st)
    assert n == len(pts) and n_good == good.sum() and abs(total / n_good - np.hypot(*shift)) < 0.5


def test_zero_shift_returns_the_points():
    a = F.blob_frame(48, 64)
    pts = np.concatenate([F.good_features(a), np.array([[10.25, 20.5], [0.0, 0.0]], np.float32)])
    nxt, st = F.track(a, a, pts)
    ok = st == 1
    assert ok.sum() >= len(pts) - 2 and np.array_equal(nxt[ok], pts[ok])


def test_plan_levels_offsets_and_bytes():
    from vista_slam_amd import flow
    want = {(224, 224): [(224, 224), (112, 112), (56, 56), (28, 28)], (96, 128): [(96, 128), (48, 64), (24, 32)],
            (48, 64): [(48, 64), (24, 32)], (40, 56): [(40, 56)], (45, 91): [(45, 91), (23, 46)]}
    for (H, W), sizes in want.items():
        p = flow.plan(H, W)
        assert list(p.sizes) == sizes == F.level_sizes(H, W) and p.levels == len(sizes), (H, W, p)
        off = 0
        for (h, w), o in zip(p.sizes, p.offsets):
            assert o == off and o % 256 == 0, (H, W, p.offsets)
            off += -(-h * w // 256) * 256
        assert p.pyramid_bytes == off
        # two key arrays, R, the rank map, two payload arrays: 32 bytes per pixel; the sort's histogram (1 KiB per tile of 1024
        # keys), its digit totals (1 KiB) and the counters; nine arrays, each rounded up to 256 bytes
        N, tiles = H * W, -(-H * W // 1024)
        assert 32 * N + 1024 * tiles + 1024 + 16 <= p.workspace_bytes <= 32 * N + 1024 * tiles + 1024 + 9 * 256, (H, W, p.workspace_bytes)
    assert flow.plan(224, 224, max_level=1).levels == 2 and flow.plan(224, 224, win=5).levels == 4
    assert flow.plan(24, 32, win=5, max_level=2).sizes == ((24, 32), (12, 16), (6, 8))
    assert flow.plan(1024, 2048, B=32).levels == 4


@pytest.mark.parametrize("kw,needles", [
    (dict(H=7, W=64), ["7 x 64", "at least 8"]),
    (dict(H=64, W=5), ["64 x 5", "at least 8"]),
    (dict(H=2048, W=1025), ["2048 x 1025", "2099200", "2097152"]),
    (dict(H=64, W=64, B=33), ["B = 33", "32"]),
    (dict(H=64, W=64, B=0), ["B = 0"]),
    (dict(H=64, W=64, win=20), ["win", "20"]),
    (dict(H=64, W=64, win=23), ["win", "23"]),
    (dict(H=64, W=64, max_level=4), ["max_level", "4"]),
    (dict(H=64, W=64, max_corners=0), ["max_corners", "got 0"]),
])
def test_plan_refusals_name_the_numbers(kw, needles):
    from vista_slam_amd import flow
    with pytest.raises(ValueError) as e:
        flow.plan(**kw)
    for s in needles:
        assert s in str(e.value), (s, str(e.value))
