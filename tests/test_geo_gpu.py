"""GPU: sta_view_consistency / sta_symmetric_geo_mask (csrc/geo.h) through vista_slam_amd.geo against the reference's recorded
output (tests/golden/geo_*.npz) by the rule the fixtures carry (tests/geo_cases.py): votes may differ from the reference by at
most nb (the neighbours whose fp64 error lies within the measured band of the threshold) at EVERY pixel, masks are equal wherever
border == 0, thresholds lie within 2 band_err.  Every figure is printed before it is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import geo_cases as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def m():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    fe = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield fe
    del fe


def _spot_votes(depth, K, T, window, thr):
    """The fixture rule computed on the spot: fp32 / fp64 restatement counts and nb from the measured band."""
    e32, e64 = G.vote_errors(depth, K, T, window, np.float32), G.vote_errors(depth, K, T, window, np.float64)
    with np.errstate(invalid="ignore"):
        dev = float(np.abs(e32.astype(np.float64) - e64)[np.isfinite(e64)].max())
    nb = G.vote_borderline(e64, thr, G.BAND_FACTOR * dev)
    return G.vote_count(e32, thr), G.vote_count(e64, thr), nb


@pytest.mark.parametrize("name", list(G.VOTE_CASES))
def test_votes_against_the_reference_fixture(m, name):
    from vista_slam_amd import geo
    g = G.load_case(name, GOLDEN)
    got = geo.view_consistency_check(m, g["depth"], g["K"], g["poses"], threshold=float(g["threshold"]), window=int(g["window"]))
    assert got.dtype.is_floating_point is False and got.element_size() == 4 and tuple(got.shape) == g["depth"].shape
    got = got.cpu().numpy()
    ref, c64, nb = g["count"].astype(np.int32), g["count64"].astype(np.int32), g["nb"].astype(np.int32)
    out_ref, out_64 = G.check_votes(got, ref, nb), G.check_votes(got, c64, nb)
    print(f"[geo] {name}: band {float(g['band']):.2e} borderline pixels {int((nb > 0).sum())} of {nb.size}; differs from the reference "
          f"at {int((got != ref).sum())} pixels, outside the rule {out_ref}; from fp64 at {int((got != c64).sum())}, outside {out_64}")
    assert out_ref == 0 and out_64 == 0
    assert np.array_equal(got[nb == 0], ref[nb == 0])                      # exact wherever no neighbour is borderline


@pytest.mark.parametrize("name", list(G.SYM_CASES))
def test_masks_against_the_reference_fixture(m, name):
    from vista_slam_amd import geo
    g = G.load_case(name, GOLDEN)
    mask, thres = geo.symmetric_geo_valid_masks(m, g["depths"], g["K"], g["rel_pose"], return_thres=True)
    assert mask.dtype.is_floating_point is False and mask.element_size() == 1 and tuple(mask.shape) == g["depths"].shape
    mask, thres = mask.cpu().numpy(), thres.cpu().numpy()
    outside = G.check_masks(mask, g["mask"], g["border"])
    dthres = np.abs(thres.astype(np.float64) - g["thres"].astype(np.float64))
    print(f"[geo] {name}: band_uv {float(g['band_uv']):.2e} band_err {float(g['band_err']):.2e} border pixels {int(g['border'].sum())} of "
          f"{g['border'].size}; differs from the reference at {int((mask != g['mask']).sum())} pixels, outside the rule {outside}; "
          f"thresholds {thres.tolist()} vs {g['thres'].tolist()}, max distance {dthres.max():.3e}")
    assert outside == 0
    assert (dthres <= 2 * float(g["band_err"])).all()
    # the single-edge entry point (the reference's signature) gives the same edge
    one = geo.compute_symmetric_geo_valid_mask(m, g["depths"][0], g["K"][0], g["rel_pose"][0])
    assert tuple(one.shape) == g["depths"].shape[1:] and np.array_equal(one.cpu().numpy(), mask[0])


def test_identical_views_count_their_neighbours(m):
    """n identical views, identity poses: every neighbour reprojects a pixel onto itself and agrees, so
    count == min(i, w) + min(n-1-i, w) at every pixel with finite positive depth; n = 1 -> all zero."""
    from vista_slam_amd import geo
    rng = np.random.default_rng(3)
    H, W, n = 40, 56, 11
    clean = (1.0 + 3.0 * rng.random((H, W))).astype(np.float32)
    bad = clean.copy()
    bad[5, 7] = np.nan; bad[6, 18] = np.inf; bad[17, 9] = -1.0; bad[28, 30] = 0.0   # must not fault; what they vote is not pinned
    # ... nor what their eight neighbours vote: uv = (x, y) up to rounding, so a bilinear tap may touch the pixel next door
    good = np.isfinite(bad) & (bad > 0)
    far = good.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            far &= np.roll(np.roll(good, dy, 0), dx, 1)
    K = np.array([[50.0, 0, W / 2.0], [0, 50.0, H / 2.0], [0, 0, 1]], np.float32)
    Ks, Ts = np.stack([K] * n), np.stack([np.eye(4, dtype=np.float32)] * n)
    for d, ok in ((clean, np.ones((H, W), bool)), (bad, far)):
        depth = np.stack([d] * n)
        for w in (4, 1, 2, 0, 20):
            got = geo.view_consistency_check(m, depth, Ks, Ts, window=w).cpu().numpy()
            assert got.min() >= 0 and got.max() <= min(2 * w, n - 1)
            for i in range(n):
                want = min(i, w) + min(n - 1 - i, w)
                assert (got[i][ok] == want).all(), (w, i, want, np.unique(got[i][ok]))
    depth = np.stack([clean] * n)
    one = geo.view_consistency_check(m, depth[:1], Ks[:1], Ts[:1]).cpu().numpy()
    assert one.shape == (1, H, W) and (one == 0).all()


@pytest.mark.parametrize("n,window", [(2, 4), (7, 1), (7, 2)])
def test_votes_against_the_restatement(m, n, window):
    """n = 2 and the windows the fixtures do not hold, against the numpy restatement by the rule computed on the spot."""
    from vista_slam_amd import geo
    depth, K, T = G.scene(n, 48, 64, seed=5)
    c32, c64, nb = _spot_votes(depth, K, T, window, G.VOTE_THRESHOLD)
    got = geo.view_consistency_check(m, depth, K, T, window=window).cpu().numpy()
    out_32, out_64 = G.check_votes(got, c32, nb), G.check_votes(got, c64, nb)
    print(f"[geo] n={n} window={window}: borderline pixels {int((nb > 0).sum())} of {nb.size}, differs from the fp32 restatement at "
          f"{int((got != c32).sum())}, outside the rule {out_32} / {out_64}; values {np.unique(got).tolist()}")
    assert (nb > 0).mean() <= G.MAX_BORDERLINE and out_32 == 0 and out_64 == 0
    assert got.max() == min(2 * window, n - 1) and got.min() == 0


def test_batched_edges_equal_single_edges_and_runs_repeat(m):
    from vista_slam_amd import geo
    import torch
    g = G.load_case("geo_sym_48x64_p3", GOLDEN)
    d, K, T = (torch.from_numpy(g[k]).cuda() for k in ("depths", "K", "rel_pose"))
    mask, thres = geo.symmetric_geo_valid_masks(m, d, K, T, return_thres=True)
    for p in range(3):
        m1, t1 = geo.symmetric_geo_valid_masks(m, d[p:p + 1], K[p:p + 1], T[p:p + 1], return_thres=True)
        assert torch.equal(m1[0], mask[p]) and torch.equal(t1[0], thres[p])
    mask2, thres2 = geo.symmetric_geo_valid_masks(m, d, K, T, return_thres=True)
    assert torch.equal(mask, mask2) and torch.equal(thres, thres2)
    v = G.load_case("geo_vote_64x80_n12", GOLDEN)
    a = geo.view_consistency_check(m, v["depth"], v["K"], v["poses"])
    b = geo.view_consistency_check(m, v["depth"], v["K"], v["poses"])
    assert torch.equal(a, b)


def test_portrait_shim_works_on_the_transposed_views(m):
    """k_on_transposed (H > W): the masks of the transposed views, returned in image orientation."""
    from vista_slam_amd import geo
    import torch
    depths, K, rel = G.sym_case_inputs("geo_sym_48x64_p3")                     # [P,2,48,64]: the views the reference works on
    img = torch.from_numpy(depths).transpose(2, 3).contiguous()                # [P,2,64,48]: the portrait frames in image orientation
    want = geo.symmetric_geo_valid_masks(m, depths, K, rel)
    got = geo.symmetric_geo_valid_masks(m, img, K, rel, k_on_transposed=True)
    assert tuple(got.shape) == (3, 2, 64, 48) and torch.equal(got.transpose(2, 3), want)


def test_mask_of_a_scheduler_result(m):
    """depth, K and pose straight from the device buffers of a real sta_regress_views call on the tiny model: the mask equals the
    fp32 restatement outside a border computed on the spot (the fixtures' rule, band = 8 x the measured fp32-fp64 distance)."""
    import torch
    from vista_slam_amd import geo, weights as W
    from vista_slam_amd.slam_scheduler import regress_views
    H, Wd = 48, 64
    imgs = torch.from_numpy(W.synth_images(4, H, Wd, seed=43, tag=31)).cuda()
    feats = [m._encode_image(imgs[v:v + 1], None, normalize=False)[0] for v in range(4)]
    edges = [e for e in regress_views(m, feats[3], feats[:3], [False, False, True], -1.0, H, Wd) if e.accepted]
    assert len(edges) == 3
    depths, K, pose = torch.stack([e.depths for e in edges]), torch.stack([e.intri for e in edges]), torch.stack([e.pose for e in edges])
    mask, thres = geo.symmetric_geo_valid_masks(m, depths, K, pose, return_thres=True)
    mask, thres = mask.cpu().numpy(), thres.cpu().numpy()
    dn, Kn, Tn = depths.cpu().numpy(), K.cpu().numpy(), pose.cpu().numpy()
    for p in range(3):
        p32, p64 = G.sym_parts(dn[p], Kn[p], Tn[p], np.float32), G.sym_parts(dn[p], Kn[p], Tn[p], np.float64)
        with np.errstate(invalid="ignore"):
            near = np.isfinite(p64["uv"]).all(1) & (np.abs(p64["uv"]) < 4 * max(H, Wd)).all(1)
            dev_uv = float(np.abs(p32["uv"].astype(np.float64) - p64["uv"]).max(1)[near].max()) if near.any() else 0.0
            same = p32["valid"] & p64["valid"] & (np.round(p32["uv"]) == np.round(p64["uv"])).all(1)
            dev_err = float(np.abs(p32["err"].astype(np.float64) - p64["err"])[same].max()) if same.any() else 0.0
        border = G.sym_border(p64, p32["thres"], G.BAND_FACTOR * dev_uv, G.BAND_FACTOR * dev_err)
        outside = G.check_masks(mask[p], p32["mask"], border)
        dth = np.abs(thres[p].astype(np.float64) - p32["thres"].astype(np.float64))
        print(f"[geo] scheduler edge {p}: dev_uv {dev_uv:.2e} dev_err {dev_err:.2e} border {int(border.sum())} of {border.size} valid "
              f"{p32['valid'].mean(1).tolist()} True {mask[p].mean((1, 2)).tolist()} differs {int((mask[p] != p32['mask']).sum())} outside the rule "
              f"{outside}; thresholds {thres[p].tolist()} vs {p32['thres'].tolist()}")
        assert border.mean() <= G.MAX_BORDERLINE
        assert outside == 0
        with np.errstate(invalid="ignore"):
            assert ((dth <= 2 * G.BAND_FACTOR * dev_err) | (thres[p] == p32["thres"])).all()


def test_second_call_of_a_shape_allocates_nothing(m):
    from vista_slam_amd import geo
    v = G.load_case("geo_vote_224_n10", GOLDEN)
    s = G.load_case("geo_sym_224_p2", GOLDEN)
    geo.view_consistency_check(m, v["depth"], v["K"], v["poses"])
    geo.symmetric_geo_valid_masks(m, s["depths"], s["K"], s["rel_pose"], return_thres=True)
    a0 = m.alloc_stats()
    geo.view_consistency_check(m, v["depth"], v["K"], v["poses"])
    assert m.alloc_stats() == a0
    geo.symmetric_geo_valid_masks(m, s["depths"], s["K"], s["rel_pose"], return_thres=True)
    assert m.alloc_stats() == a0


def test_pointcloud_keeps_the_pixels_enough_views_agree_on(m):
    """world_pointcloud(..., counts, min_views=3) returns exactly the rows of the unfiltered cloud whose pixel has count >= 3, in
    order; with the defaults the records are byte-identical to the call without the new arguments."""
    import torch
    from vista_slam_amd import formats as F, geo
    v = G.load_case("geo_vote_48x64_n6", GOLDEN)
    n, H, W = v["depth"].shape
    rng = np.random.default_rng(9)
    conf = (1.0 + 2.0 * rng.random((n, H, W))).astype(np.float32)
    imgs = (2.0 * rng.random((n, 3, H, W)) - 1.0).astype(np.float32)
    scales = np.ones(n, np.float32)
    thr = 1.8
    counts = geo.view_consistency_check(m, v["depth"], v["K"], v["poses"])
    args = (m, v["depth"], scales, v["K"], v["poses"], conf, imgs, thr)
    pts, col, rec = F.world_pointcloud(*args, want_records=True)
    pts_d, col_d, rec_d = F.world_pointcloud(*args, want_records=True, counts=None, min_views=0)
    assert rec.tobytes() == rec_d.tobytes() and torch.equal(pts, pts_d) and torch.equal(col, col_d)
    pts_0, _, rec_0 = F.world_pointcloud(*args, want_records=True, counts=counts, min_views=0)
    assert rec.tobytes() == rec_0.tobytes() and torch.equal(pts, pts_0)
    pts_f, col_f, rec_f = F.world_pointcloud(*args, want_records=True, counts=counts, min_views=3)
    keep = conf.reshape(-1) > np.float32(thr)
    sel = counts.cpu().numpy().reshape(-1)[keep] >= 3
    assert 0 < sel.sum() < keep.sum() == len(pts)
    sel_t = torch.from_numpy(sel).to(pts.device)
    assert torch.equal(pts_f, pts[sel_t]) and torch.equal(col_f, col[sel_t]) and rec_f.tobytes() == rec[sel].tobytes()


def test_argument_errors_return_a_status_and_a_message(m):
    import torch
    from vista_slam_amd import _lib
    lib, h, st = m.lib, m._h, m._stream()
    d = torch.ones(2, 2, 8, 8, device="cuda"); K = torch.eye(3, device="cuda").repeat(2, 1, 1).contiguous()
    T = torch.eye(4, device="cuda").repeat(2, 1, 1).contiguous()
    cnt = torch.full((2, 8, 8), -7, device="cuda", dtype=torch.int32); msk = torch.full((1, 2, 8, 8), 9, device="cuda", dtype=torch.uint8)
    a0 = m.alloc_stats()
    p = lambda t: t.data_ptr()

    def fails(rc, match):
        assert rc < 0
        msg = lib.sta_last_error().decode()
        assert match in msg, msg
    fails(lib.sta_view_consistency(h, p(d), p(K), p(T), 0, 8, 8, 0.05, 4, p(cnt), st), "bad size")
    fails(lib.sta_view_consistency(h, p(d), p(K), p(T), 2, 8, 8, 0.05, -1, p(cnt), st), "window")
    fails(lib.sta_view_consistency(h, p(d), p(K), p(T), 2, 8, 8, 0.05, 4, None, st), "null")
    fails(lib.sta_view_consistency(h, None, p(K), p(T), 2, 8, 8, 0.05, 4, p(cnt), st), "null")
    fails(lib.sta_symmetric_geo_mask(h, p(d), p(K), p(T), 0, 8, 8, p(msk), None, st), "bad size")
    fails(lib.sta_symmetric_geo_mask(h, p(d), p(K), p(T), 1, 8, 0, p(msk), None, st), "bad size")
    fails(lib.sta_symmetric_geo_mask(h, p(d), p(K), p(T), 1, 8, 8, None, None, st), "null")
    torch.cuda.synchronize()
    assert m.alloc_stats() == a0 and (cnt == -7).all() and (msk == 9).all()      # nothing was launched
    with pytest.raises(_lib.StaError):
        from vista_slam_amd import geo
        geo.view_consistency_check(m, d[0], K, T, window=-1)
