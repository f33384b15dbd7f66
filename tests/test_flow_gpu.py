"""GPU: the keyframe gate (csrc/flow.h: sta_flow_pyramid / sta_flow_corners / sta_flow_track, vista_slam_amd.flow) against the numpy
restatement of its contract (tests/flow_cases.py), through the C ABI with guard regions behind every output and through the Python
layer.  Every comparison is array_equal; the exception is the sum of the displacements, a float64 sum of at most 1000 terms whose
order differs from numpy's, compared at rel 1e-12.  The shapes are the smallest at which the kernels can go wrong: odd sizes whose
halvings are odd, a frame of one level, 8x8 (the halo reflects more than a tile), candidate counts either side of a sort tile and of
the suppression workgroup (both 1024), long tie chains, n either side of a wave, 32 frames in one launch."""
import ctypes as C

import numpy as np
import pytest

import flow_cases as F

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64               # bytes / rows behind every output


@pytest.fixture(scope="module")
def m():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    fe = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield fe
    del fe


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(nbytes):
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


def run_pyramid(m, frames, win=21, max_level=3):
    """frames [B, H, W] uint8 or float32 (numpy) -> per frame the list of levels, after asserting that the bytes between the levels,
    behind the last one and behind the last pyramid still hold the fill pattern."""
    import torch
    from vista_slam_amd import _lib, flow
    frames = np.ascontiguousarray(frames)
    B, H, W = frames.shape
    p = flow.plan(H, W, B, win, max_level)
    src = _up(frames)
    buf = _filled(B * p.pyramid_bytes + GUARD)
    _lib.check(m.lib.sta_flow_pyramid(m._h, src.data_ptr(), 0 if frames.dtype == np.uint8 else 1, H, W, B, win, max_level, buf.data_ptr(), m._stream()))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    touched = np.ones(len(raw), bool)
    out = []
    for b in range(B):
        lv = []
        for (h, w), o in zip(p.sizes, p.offsets):
            s = b * p.pyramid_bytes + o
            lv.append(raw[s:s + h * w].reshape(h, w).copy())
            touched[s:s + h * w] = False
        out.append(lv)
    assert (raw[touched] == FILL).all(), "bytes outside the levels were written"
    return out, src, buf, p


def run_corners(m, img, max_corners=1000, quality=0.01, min_distance=8, block_size=7):
    """-> corners [n, 2] float32 through the C ABI; rows at or past n, and the words behind n, must still hold the pattern"""
    import torch
    from vista_slam_amd import _lib, flow
    H, W = img.shape
    p = flow.plan(H, W, 1, 21, 0, max_corners)
    src = _up(img)
    ws = _filled(p.workspace_bytes + GUARD)
    corners = _filled((max_corners + GUARD) * 8)
    n = _filled(4 + GUARD)
    _lib.check(m.lib.sta_flow_corners(m._h, src.data_ptr(), H, W, max_corners, quality, min_distance, block_size, ws.data_ptr(), p.workspace_bytes,
                                      corners.data_ptr(), n.data_ptr(), m._stream()))
    torch.cuda.synchronize()
    nraw, craw = n.cpu().numpy(), corners.cpu().numpy()
    count = int(nraw[:4].view(np.int32)[0])
    assert 0 <= count <= max_corners, count
    assert (nraw[4:] == FILL).all() and (craw[count * 8:] == FILL).all(), "rows at or past n were written"
    assert (ws.cpu().numpy()[p.workspace_bytes:] == FILL).all(), "bytes behind the workspace were written"
    return craw[:count * 8].view(np.float32).reshape(count, 2).copy()


def run_track(m, prev, nxts, pts, n_dev=None, cap=None, **kw):
    """prev [H, W], nxts [B, H, W] uint8, pts [n, 2] -> (next_pts [B, n, 2], status [B, n], stats [B, 3]) through the C ABI and the
    pyramids of `flow.pyramid`; cap > n with a device count n_dev exercises the rows that must stay untouched."""
    import torch
    from vista_slam_amd import _lib, flow
    nxts = np.ascontiguousarray(nxts)
    B, H, W = nxts.shape
    win, max_level = kw.get("win", 21), kw.get("max_level", 3)
    pp, pn = flow.pyramid(m, prev, win, max_level), flow.pyramid(m, nxts, win, max_level)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    cap = n if cap is None else cap
    rows = np.zeros((cap, 2), np.float32)
    rows[:n] = pts
    pd = _up(rows) if cap else None
    nd = _up(np.array([n_dev], np.int32)) if n_dev is not None else None
    out, status, stats = _filled((B * cap + GUARD) * 8), _filled(B * cap + GUARD), _filled((B * 3 + GUARD) * 8)
    _lib.check(m.lib.sta_flow_track(m._h, pp.buf.data_ptr(), pn.buf.data_ptr(), H, W, B, win, max_level, pd.data_ptr() if cap else None,
                                    nd.data_ptr() if nd is not None else None, cap, kw.get("max_iter", 30), kw.get("eps", 0.01),
                                    kw.get("min_eig", 1e-4), out.data_ptr(), status.data_ptr(), stats.data_ptr(), m._stream()))
    torch.cuda.synchronize()
    o, s, t = out.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy()
    assert (o[B * cap * 8:] == FILL).all() and (s[B * cap:] == FILL).all() and (t[B * 24:] == FILL).all(), "bytes behind an output were written"
    o = o[:B * cap * 8].view(np.float32).reshape(B, cap, 2)
    s = s[:B * cap].reshape(B, cap)
    if n < cap:
        assert (o[:, n:].view(np.uint8) == FILL).all() and (s[:, n:] == FILL).all(), "rows at or past n were written"
    return o[:, :n].copy(), s[:, :n].copy(), t[:B * 24].view(np.float64).reshape(B, 3).copy()


def check_track(got, prev, nxts, pts, what, ref=None, **kw):
    """against the restatement (ref = its precomputed (next_pts, status) per frame, when a caller shares one)"""
    o, s, t = got
    for b in range(len(nxts)):
        e_o, e_s = ref[b] if ref is not None else F.track(prev, nxts[b], pts, **kw)
        bad = np.flatnonzero((o[b] != e_o).any(axis=1) | (s[b] != e_s))
        assert bad.size == 0, (f"{what} frame {b}: {bad.size} of {len(pts)} points differ, first {bad[:4].tolist()}: got "
                               f"{o[b][bad[:4]].tolist()} {s[b][bad[:4]].tolist()}, expected {e_o[bad[:4]].tolist()} {e_s[bad[:4]].tolist()}")
        n, good, total = F.disparity(pts, e_o, e_s)
        assert t[b, 0] == n and t[b, 1] == good, (what, b, t[b].tolist(), n, good)
        assert abs(t[b, 2] - total) <= 1e-12 * abs(total), (what, b, t[b, 2], total)


# ------------------------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("H,W,levels", [(224, 224, 4), (45, 91, 2), (40, 56, 1), (8, 8, 1), (96, 128, 3)])
def test_pyramid_against_the_restatement(m, H, W, levels):
    frames = np.stack([F.noise_frame(H, W, 5), F.blob_frame(H, W, n_blobs=30)])
    got, *_ = run_pyramid(m, frames)
    for b in range(2):
        exp = F.pyramid(frames[b])
        assert len(exp) == len(got[b]) == levels
        for l, (g, e) in enumerate(zip(got[b], exp)):
            assert np.array_equal(g, e), (H, W, b, l, int((g != e).sum()))


def test_pyramid_small_window_reaches_tiny_levels(m):
    """win = 5 lets 24x32 halve twice (6x8: a level smaller than a tile's halo) and 45x91 three times"""
    for H, W in ((24, 32), (45, 91)):
        frames = F.noise_frame(H, W, 6)[None]
        got, *_ = run_pyramid(m, frames, win=5, max_level=3)
        exp = F.pyramid(frames[0], 5, 3)
        assert len(exp) == len(got[0]) >= 3
        assert all(np.array_equal(g, e) for g, e in zip(got[0], exp))


def test_pyramid_float_route(m):
    """fp32 frames convert as uint8(trunc(fp32 * 255.0f)): every k / 255, random values (truncated, not rounded), a random frame, and
    the same pyramid as the uint8 route gives for the converted frame"""
    rng = np.random.RandomState(9)
    ramp = np.zeros((16, 32), np.float32)
    ramp.reshape(-1)[:256] = np.arange(256, dtype=np.float32) / np.float32(255.0)
    ramp.reshape(-1)[256:] = rng.uniform(0, 1, 256).astype(np.float32)
    for fl in (ramp, rng.uniform(0, 1, (45, 91)).astype(np.float32)):
        u8 = F.to_u8(fl)
        a, *_ = run_pyramid(m, fl[None])
        b, *_ = run_pyramid(m, u8[None])
        exp = F.pyramid(fl)
        assert np.array_equal(a[0][0], u8)
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a[0], b[0], exp))
    tail = ramp.reshape(-1)[256:]
    assert (F.to_u8(ramp).reshape(-1)[256:] != np.rint(tail * 255.0)).any()        # truncation, not rounding, is what the ramp checks


# ------------------------------------------------------------------------------------------------------------ corners
def _corner_cases():
    checker = F.checker_frame(64, 64)
    return {
        "blobs": (F.blob_frame(96, 128), {}),
        "noise": (F.noise_frame(96, 128, 3), {}),
        "noise_all_kept": (F.noise_frame(96, 128, 3), dict(min_distance=1)),
        "checker_ties": (checker, {}),
        "checker_truncated": (checker, dict(max_corners=16, min_distance=3)),
        "constant": (np.full((40, 56), 9, np.uint8), {}),
        "odd_block5": (F.noise_frame(45, 91, 4), dict(block_size=5, min_distance=5, quality=0.05)),
        "tiny_block3": (F.noise_frame(8, 8, 8), dict(block_size=3, min_distance=2)),
        "across_1024": (F.noise_frame(128, 160, 12), dict(min_distance=1, max_corners=4000)),
        "large": (F.noise_frame(384, 512, 13), {}),
    }


@pytest.mark.parametrize("name", list(_corner_cases()))
def test_corners_against_the_restatement(m, name):
    img, kw = _corner_cases()[name]
    info = {}
    exp = F.good_features(img, info=info, **kw)
    got = run_corners(m, img, **kw)
    print(f"[flow] {name}: {info['n_candidates']} candidates of {info['n_distinct']} distinct responses -> {len(exp)} corners")
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"{name}: {bad.size} of {len(exp)} corners differ, first at {bad[:4].tolist()}: got {got[bad[:4]].tolist()}, expected {exp[bad[:4]].tolist()}"
    if name == "constant":
        assert len(exp) == 0
    if name == "checker_ties":
        assert info["n_candidates"] > 1000 and info["n_distinct"] < 16           # the tie order and long chains are exercised
    if name == "checker_truncated":
        assert len(exp) == 16
    if name == "across_1024":
        assert info["n_candidates"] > 1024 and len(exp) == info["n_candidates"]
    if name == "large":
        assert info["n_candidates"] > 4096 and len(exp) == 1000


# ------------------------------------------------------------------------------------------------------------ track
@pytest.mark.parametrize("H,W", [(48, 64), (96, 128), (224, 224), (45, 91)])
def test_track_blob_pairs(m, H, W):
    a = F.blob_frame(H, W)
    pts = F.good_features(a)
    shifts = [(1.25, -0.5), (5.5, 3.25)]
    nxts = np.stack([F.blob_frame(H, W, s) for s in shifts])
    check_track(run_track(m, a, nxts, pts), a, nxts, pts, f"{H}x{W}")


def test_track_caller_points(m):
    H, W = 96, 128
    a = F.blob_frame(H, W).copy()
    a[30:66, 40:80] = 131                                       # a constant patch: the eigenvalue test rejects a point on it
    pts = np.array([[20.25, 30.5], [77.125, 12.875], [100.5, 80.0], [0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1],
                    [-12.5, 40.0], [W + 11.0, 20.0], [50.0, -30.0], [60.0, 48.0], [59.5, 47.25], [3.0, 90.0], [124.0, 50.5]], np.float32)
    nxts = []
    for s in ((1.25, -0.5), (20.0, 0.0), (0.0, 0.0)):
        b = F.blob_frame(H, W, s).copy()
        y0, x0 = 30 + int(s[1]), 40 + int(s[0])
        b[y0:y0 + 36, x0:x0 + 40] = 131
        nxts.append(b)
    nxts = np.stack(nxts)
    ref = [F.track(a, b, pts) for b in nxts]
    st = ref[0][1]
    assert st[9] == 0 and st[10] == 0 and st[:3].all(), st.tolist()          # window outside the frame; constant patch; tracked
    assert 0 < ref[1][1].sum() < len(pts), ref[1][1].tolist()                # the 20 px shift loses some points and keeps others
    check_track(run_track(m, a, nxts, pts), a, nxts, pts, "caller points", ref=ref)


@pytest.fixture(scope="module")
def many_points():
    H, W = 48, 64
    a, b = F.blob_frame(H, W), F.blob_frame(H, W, (1.25, -0.5))
    pts = np.random.RandomState(21).uniform([-4, -4], [W + 4, H + 4], (1000, 2)).astype(np.float32)
    return a, b, pts, F.track(a, b, pts)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_track_point_counts(m, many_points, n):
    a, b, pts, (e_o, e_s) = many_points
    ref = [(e_o[:n], e_s[:n])]
    check_track(run_track(m, a, b[None], pts[:n]), a, b[None], pts[:n], f"n = {n}", ref=ref)
    if n in (1, 65):                                                          # the count from the device, capacity above it
        check_track(run_track(m, a, b[None], pts[:n], n_dev=n, cap=n + 70), a, b[None], pts[:n], f"n_dev = {n}", ref=ref)
    if n == 64:                                                               # a device count above the capacity is cut to it
        check_track(run_track(m, a, b[None], pts[:n], n_dev=5000), a, b[None], pts[:n], "n_dev above cap", ref=ref)


@pytest.mark.parametrize("B", [1, 3, 32])
def test_track_frames_in_one_launch(m, B):
    H, W = 48, 64
    a = F.blob_frame(H, W)
    pts = F.good_features(a)[:24]
    nxts = np.stack([F.blob_frame(H, W, (0.35 * k, -0.2 * k)) for k in range(B)])
    got = run_track(m, a, nxts, pts)
    check_track(got, a, nxts, pts, f"B = {B}")
    if B > 1:
        assert not np.array_equal(got[0][0], got[0][B - 1])


def test_track_zero_shift_is_exact(m):
    a = F.blob_frame(96, 128)
    pts = np.concatenate([F.good_features(a), np.array([[10.25, 20.5], [64.0, 48.0]], np.float32)])
    o, s, t = run_track(m, a, a[None], pts)
    e_o, e_s = F.track(a, a, pts)
    assert np.array_equal(o[0], e_o) and np.array_equal(s[0], e_s)
    ok = s[0] == 1
    assert ok.sum() >= len(pts) - 2 and np.array_equal(o[0][ok], pts[ok]) and t[0, 2] == 0.0


def test_track_small_window(m):
    """win = 7 (two pixels per lane, lanes without a pixel) and two iterations only"""
    H, W = 45, 91
    a, b = F.blob_frame(H, W), F.blob_frame(H, W, (1.25, -0.5))
    pts = F.good_features(a, min_distance=4)[:40]
    kw = dict(win=7, max_level=2, max_iter=2)
    check_track(run_track(m, a, b[None], pts, **kw), a, b[None], pts, "win 7", **kw)


# ------------------------------------------------------------------------------------------------------------ FlowTracker
def _rgb_sequence():
    """13 frames for process_image: drift, a jump at frame 8, and a blank frame at 5 (a keyframe without corners: the next call
    re-initialises)"""
    shifts, s = [], 0.0
    for t in range(12):
        s += 18.0 if t == 8 else 0.6
        shifts.append((s, 0.4 * s))
    frames = [F.blob_frame(212, 276, sh, seed=11, n_blobs=150) for sh in shifts]
    frames.insert(5, np.full((212, 276), 128, np.uint8))
    return [np.ascontiguousarray(np.stack([f, f, f], axis=-1)) for f in frames]


def test_flow_tracker_replay(m):
    import torch
    from vista_slam_amd import flow
    from vista_slam_amd.preprocess import process_image
    grays = [process_image(m, rgb, (128, 96))["gray"] for rgb in _rgb_sequence()]
    assert tuple(grays[0].shape) == (1, 96, 128) and grays[0].dtype == torch.float32
    u8 = [F.to_u8(g.cpu().numpy()) for g in grays]
    thres = 1.0
    ref = F.RefTracker(thres)
    want = [ref.compute_disparity(f) for f in u8]
    why = [r[1] for r in ref.log]
    print("[flow] replay:", " ".join(f"{w}:{r[2]}/{r[3]}" for w, r in zip(why, ref.log)))
    assert why[0] == "first" and {"moved", "still", "reinit"} <= set(why), why        # every branch of the reference is taken
    routes = {"numpy": u8, "device": [torch.from_numpy(f).cuda() for f in u8], "process_image": grays}
    torch.cuda.synchronize()
    before = m.alloc_stats()
    for name, frames in routes.items():
        tr = flow.FlowTracker(m, thres)
        got, last = [], []
        for f in frames:
            got.append(tr.compute_disparity(f))
            last.append(tr.last)
        assert got == want, (name, got, want)
        for t, (l, r) in enumerate(zip(last[1:], ref.log[1:]), 1):
            assert l[0] == r[2] and l[1] == r[3], (name, t, l, r)
            assert abs(l[2] - r[4]) <= 1e-12 * abs(r[4]), (name, t, l, r)
        routes[name] = last
        with pytest.raises(NotImplementedError):
            tr.compute_disparity(frames[0], visualize=True)
    assert routes["numpy"] == routes["device"] == routes["process_image"]          # bit for bit, the sums included
    assert m.alloc_stats() == before


def test_disparities_equals_the_per_frame_calls(m):
    import torch
    from vista_slam_amd import flow
    H, W = 96, 128
    frames = [F.blob_frame(H, W, (0.4 * k, 0.1 * k)) for k in range(7)]
    tr = flow.FlowTracker(m, 1e9)                                               # never a keyframe after the first
    assert tr.compute_disparity(frames[0]) is True
    kf = tr.kf_pts.clone()
    torch.cuda.synchronize()
    before = m.alloc_stats()
    batch = tr.disparities(frames[1:])
    assert torch.equal(tr.kf_pts, kf) and tr.last is None                       # no state changed
    for f, (n_good, mean) in zip(frames[1:], batch):
        assert tr.compute_disparity(f) is False
        assert tr.last[1] == n_good and tr.last[2] / tr.last[1] == mean
    pts = F.good_features(frames[0])
    assert int(tr.kf_n.item()) == len(pts) and np.array_equal(tr.kf_pts[:len(pts)].cpu().numpy(), pts)
    for f, (n_good, mean) in zip(frames[1:3], batch):
        _, good, total = F.disparity(pts, *F.track(frames[0], f, pts))
        assert good == n_good and abs(mean - total / good) <= 1e-12 * mean
    with pytest.raises(ValueError):
        tr.disparities([frames[0]] * 33)
    assert m.alloc_stats() == before


def test_python_layer_returns_device_tensors(m):
    from vista_slam_amd import flow
    a, b = F.blob_frame(45, 91), F.blob_frame(45, 91, (1.25, -0.5))
    pa, pb = flow.pyramid(m, a), flow.pyramid(m, [a, b])
    assert pb.B == 2 and all(np.array_equal(pa.level(l).cpu().numpy(), e) for l, e in enumerate(F.pyramid(a)))
    assert np.array_equal(pb.level(1, 1).cpu().numpy(), F.pyramid(b)[1])
    pts, n = flow.good_features(m, pa)
    exp = F.good_features(a)
    assert pts.is_cuda and n.is_cuda and int(n.item()) == len(exp) and np.array_equal(pts[:len(exp)].cpu().numpy(), exp)
    out, status, stats = flow.track(m, pa, pb, pts, n)
    e_o, e_s = F.track(a, b, exp)
    assert out.is_cuda and tuple(out.shape) == (2, 1000, 2) and tuple(stats.shape) == (2, 3)
    assert np.array_equal(out[1, :len(exp)].cpu().numpy(), e_o) and np.array_equal(status[1, :len(exp)].cpu().numpy(), e_s)
    assert np.array_equal(out[0, :len(exp)].cpu().numpy(), exp)
