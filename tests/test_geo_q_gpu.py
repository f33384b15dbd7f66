"""GPU: sta_geo_valid_mask / sta_local_pointclouds / sta_ray_depth (csrc/geo.h) through vista_slam_amd.geo against the reference's
recorded output (tests/golden/geo_q_*.npz, geo_ray_*.npz) by the rules the fixtures carry (tests/geo_q_cases.py): masks equal
wherever border == 0, the threshold within thr_tol, the count within the number of uv-border pixels; points and ray depths within
8 x the reference's own fp32-fp64 distance.  The threshold itself is pinned bit for bit against torch.quantile on a construction
whose errors are exact.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest

import geo_cases as G
import geo_q_cases as Q

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def m():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    fe = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield fe
    del fe


def _args(g):
    return g["depth1"], g["depth2"], g["K1"], g["K2"], g["T1"], g["T2"], float(g["q"])


def _identity(B):
    return np.stack([np.eye(3, dtype=np.float32)] * B), np.stack([np.eye(4, dtype=np.float32)] * B)


@pytest.mark.parametrize("name", list(Q.Q_CASES))
def test_masks_against_the_reference_fixture(m, name):
    from vista_slam_amd import geo
    g = Q.load_q_case(name, GOLDEN)
    mask, thres, count = geo.geo_valid_masks(m, *_args(g), return_thres=True)
    assert mask.dtype.is_floating_point is False and mask.element_size() == 1 and tuple(mask.shape) == g["depth1"].shape
    assert thres.dim() == 0 and count.dim() == 0 and thres.is_cuda and count.is_cuda
    mask, thres, count = mask.cpu().numpy(), float(thres), int(count)
    outside = Q.check_q_masks(mask, g["mask"], g["border"])
    nuv = int(g["uv_border"].sum())
    print(f"[geo_q] {name}: band_uv {float(g['band_uv']):.2e} band_err {float(g['band_err']):.2e} border pixels {int(g['border'].sum())} of "
          f"{g['border'].size} (uv {nuv}); differs from the reference at {int((mask != g['mask']).sum())} pixels, outside the rule {outside}; "
          f"threshold {thres!r} vs {float(g['thres'])!r}, distance {abs(thres - float(g['thres'])):.3e}, thr_tol {float(g['thr_tol']):.3e}; "
          f"count {count} vs {int(g['count'])}")
    assert outside == 0
    assert Q.thres_within(thres, g["thres"], float(g["thr_tol"]))
    assert abs(count - int(g["count"])) <= nuv
    # the function that carries the reference's name gives the same mask
    one = geo.compute_geo_valid_mask_batched(m, *_args(g))
    assert one.dtype.is_floating_point is False and one.element_size() == 1 and np.array_equal(one.cpu().numpy(), mask)


@pytest.mark.parametrize("name", list(Q.RAY_CASES))
def test_points_and_ray_depths_against_the_reference_fixture(m, name):
    from vista_slam_amd import geo
    g = Q.load_ray_case(name, GOLDEN)
    n, H, W = Q.RAY_CASES[name]
    bound_pc, bound_rd = G.BAND_FACTOR * float(g["dev_pc"]), G.BAND_FACTOR * float(g["dev_rd"])
    got = {}
    for tag, Kf in (("b", g["K"]), ("s", g["K"][0])):
        pc = geo.compute_local_pointclouds(m, g["depth"], Kf)
        rd = geo.depth_from_pointcloud_dot_batched(m, g[f"pc_{tag}"], Kf)
        assert tuple(pc.shape) == (n, H, W, 3) and tuple(rd.shape) == (n, H, W) and pc.element_size() == rd.element_size() == 4
        got[tag] = pc.cpu().numpy()
        dpc, drd = Q.pc_distance(got[tag], g[f"pc64_{tag}"]), Q.rd_distance(rd.cpu().numpy(), g[f"rd64_{tag}"])
        print(f"[geo_q] {name} ({'batched' if tag == 'b' else 'shared'} K): points {dpc.max():.3e} of the point's norm (bound {bound_pc:.3e}, "
              f"reference {float(g['dev_pc']):.3e}); ray depths {drd.max():.3e} relative (bound {bound_rd:.3e}, reference {float(g['dev_rd']):.3e})")
        assert dpc.max() <= bound_pc and drd.max() <= bound_rd
    # the shared and the batched form give the same values where the matrix is the same
    assert np.array_equal(got["b"][0], got["s"][0])


@pytest.mark.parametrize("B,H,W", Q.EXACT_SHAPES)
def test_threshold_is_torch_quantile_bit_for_bit(m, B, H, W):
    """Identity K and T, depth2 = 0, depth1 = code * 2^-s: every pixel maps onto itself, all are valid, the errors ARE depth1.
    Catches a wrong rank, a wrong lerp branch, the lower element in place of the interpolation and a per-image threshold."""
    import torch
    from vista_slam_amd import geo
    K, T = _identity(B)
    bad = []
    for s in (3, 11):
        d1 = Q.exact_depths(B, H, W, s, seed=100 + Q.EXACT_SHAPES.index((B, H, W)))
        assert np.unique(d1).size < d1.size or d1.size <= 3                     # duplicated values
        dt = torch.from_numpy(d1)
        for q in Q.EXACT_QS:
            want = torch.quantile(dt.flatten(), q)
            mask, thres, count = geo.geo_valid_masks(m, d1, np.zeros_like(d1), K, K, T, T, q, return_thres=True)
            thres = thres.cpu()
            same = thres.numpy().tobytes() == want.numpy().tobytes()
            ok_mask = torch.equal(mask.cpu(), dt < want)
            print(f"[geo_q] exact B={B} {H}x{W} s={s} q={q}: thres {float(thres)!r} torch {float(want)!r} {'same bits' if same else 'DIFFERENT'}; "
                  f"count {int(count)} of {d1.size}; mask {'equal' if ok_mask else 'DIFFERENT'}")
            if not (same and ok_mask and int(count) == d1.size):
                bad.append((s, q))
    assert not bad, bad


def test_one_threshold_per_batch(m):
    """A B = 2 call differs from two B = 1 calls, and its threshold is that of the concatenated errors."""
    import torch
    from vista_slam_amd import geo
    g = Q.load_q_case("geo_q_40x56_b3", GOLDEN)
    a = [torch.from_numpy(x).cuda() for x in _args(g)[:6]]
    q = float(g["q"])
    both, t_both, c_both = geo.geo_valid_masks(m, *[x[:2] for x in a], q, return_thres=True)
    single = [geo.geo_valid_masks(m, *[x[b:b + 1] for x in a], q, return_thres=True) for b in range(2)]
    t_single = [float(s[1]) for s in single]
    p32 = Q.q_parts(*[x[:2].cpu().numpy() for x in a], q, np.float32)
    p64 = Q.q_parts(*[x[:2].cpu().numpy() for x in a], q, np.float64)
    tol = float(g["thr_tol"])
    print(f"[geo_q] one threshold per batch: B=2 {float(t_both)!r}, B=1 {t_single}, restatement of the concatenated errors "
          f"{float(p32['thres'])!r} (fp64 {float(p64['thres'])!r}), tolerance {tol:.3e}; counts {int(c_both)} = {int(single[0][2])} + {int(single[1][2])}")
    assert int(c_both) == int(single[0][2]) + int(single[1][2])
    assert abs(float(t_both) - float(p32["thres"])) <= tol
    assert min(abs(float(t_both) - t) for t in t_single) > 2 * tol             # not a per-image threshold: further than rounding reaches
    assert not torch.equal(both, torch.cat([single[0][0], single[1][0]]))
    # exact form: the errors are the depths
    K, T = _identity(2)
    d1 = Q.exact_depths(2, 24, 40, 11, seed=7); d1[1] *= 4.0
    z = np.zeros_like(d1)
    _, t2, _ = geo.geo_valid_masks(m, d1, z, K, K, T, T, 0.5, return_thres=True)
    t1 = [geo.geo_valid_masks(m, d1[b:b + 1], z[:1], K[:1], K[:1], T[:1], T[:1], 0.5, return_thres=True)[1] for b in range(2)]
    want = torch.quantile(torch.from_numpy(d1).flatten(), 0.5)
    assert t2.cpu().numpy().tobytes() == want.numpy().tobytes()
    assert all(t.cpu().numpy().tobytes() == torch.quantile(torch.from_numpy(d1[b]).flatten(), 0.5).numpy().tobytes() for b, t in enumerate(t1))
    assert float(t1[0]) != float(t2) != float(t1[1])


def test_swapped_arguments_change_the_result(m):
    from vista_slam_amd import geo
    g = Q.load_q_case("geo_q_40x56_b3", GOLDEN)
    d1, d2, K1, K2, T1, T2, q = _args(g)
    base, t0, _ = geo.geo_valid_masks(m, d1, d2, K1, K2, T1, T2, q, return_thres=True)
    ks, t_k, _ = geo.geo_valid_masks(m, d1, d2, K2, K1, T1, T2, q, return_thres=True)
    ts, t_t, _ = geo.geo_valid_masks(m, d1, d2, K1, K2, T2, T1, q, return_thres=True)
    nk, nt = int((ks != base).sum()), int((ts != base).sum())
    print(f"[geo_q] swapped K1/K2: {nk} pixels differ, threshold {float(t_k)!r} vs {float(t0)!r}; swapped T1/T2: {nt} pixels differ, "
          f"threshold {float(t_t)!r}; border pixels {int(g['border'].sum())}")
    assert Q.check_q_masks(base.cpu().numpy(), g["mask"], g["border"]) == 0
    assert Q.check_q_masks(ks.cpu().numpy(), g["mask"], g["border"]) > 0 and Q.check_q_masks(ts.cpu().numpy(), g["mask"], g["border"]) > 0
    assert abs(float(t_k) - float(t0)) > float(g["thr_tol"]) and abs(float(t_t) - float(t0)) > float(g["thr_tol"])


def test_no_valid_pixel(m):
    """The C call: count 0, NaN, an all-zero mask, no host round trip; the reference-named function raises like torch.quantile."""
    import torch
    from vista_slam_amd import geo
    B, H, W = 2, 9, 13
    K, T = _identity(B)
    T1 = T.copy(); T1[:, 0, 3] = 1000.0                                         # every pixel lands far outside view 2
    d = np.ones((B, H, W), np.float32)
    mask, thres, count = geo.geo_valid_masks(m, d, d, K, K, T1, T, 0.8, return_thres=True)
    print(f"[geo_q] no valid pixel: count {int(count)} thres {float(thres)!r} mask sum {int(mask.sum())}")
    assert int(count) == 0 and torch.isnan(thres) and not mask.any()
    with pytest.raises(RuntimeError):
        geo.compute_geo_valid_mask_batched(m, d, d, K, K, T1, T, 0.8)


def test_argument_errors_and_hostile_depths(m):
    import torch
    from vista_slam_amd import _lib, geo
    lib, h, st = m.lib, m._h, m._stream()
    d = torch.ones(2, 8, 8, device="cuda"); K = torch.eye(3, device="cuda").repeat(2, 1, 1).contiguous()
    T = torch.eye(4, device="cuda").repeat(2, 1, 1).contiguous()
    msk = torch.full((2, 8, 8), 9, device="cuda", dtype=torch.uint8)
    thr = torch.full((1,), -7.0, device="cuda"); cnt = torch.full((1,), -7, device="cuda", dtype=torch.int32)
    pc = torch.full((2, 8, 8, 3), -7.0, device="cuda"); rd = torch.full((2, 8, 8), -7.0, device="cuda")
    a0 = m.alloc_stats()
    p = lambda t: t.data_ptr()

    def fails(rc, match):
        assert rc < 0
        msg = lib.sta_last_error().decode()
        assert match in msg, msg
    mask_call = lambda B, H, W, q, out=msk: lib.sta_geo_valid_mask(h, p(d), p(d), p(K), p(K), p(T), p(T), B, H, W, q, p(out) if out is not None else None, p(thr), p(cnt), st)
    fails(mask_call(2, 8, 8, 1.5), "q must lie in [0, 1]")
    fails(mask_call(2, 8, 8, -0.01), "q must lie in [0, 1]")
    fails(mask_call(2, 8, 8, float("nan")), "q must lie in [0, 1]")
    fails(mask_call(4001, 4000, 1, 0.5), "16 000 000")                          # B*H*W = 16 004 000: refused before anything is read
    fails(mask_call(2, 4000, 4000, 0.5), "16 000 000")
    fails(mask_call(0, 8, 8, 0.5), "bad size")
    fails(mask_call(2, 8, 8, 0.5, None), "null")
    fails(lib.sta_local_pointclouds(h, p(d), p(K), 2, 2, 8, 8, p(pc), st), "k_batched")
    fails(lib.sta_local_pointclouds(h, p(d), p(K), 1, 0, 8, 8, p(pc), st), "bad size")
    fails(lib.sta_local_pointclouds(h, None, p(K), 1, 2, 8, 8, p(pc), st), "null")
    fails(lib.sta_ray_depth(h, p(pc), p(K), 1, 2, 8, 0, p(rd), st), "bad size")
    fails(lib.sta_ray_depth(h, p(pc), p(K), 1, 2, 8, 8, None, st), "null")
    torch.cuda.synchronize()
    assert m.alloc_stats() == a0                                                  # nothing was launched
    assert (msk == 9).all() and (thr == -7).all() and (cnt == -7).all() and (pc == -7).all() and (rd == -7).all()
    with pytest.raises(_lib.StaError):
        geo.geo_valid_masks(m, d, d, K, K, T, T, 1.5)
    with pytest.raises(ValueError):
        geo.compute_local_pointclouds(m, d, K[None])
    # depths NaN, inf, 0 and negative do not fault; what they decide is not pinned
    rng = np.random.default_rng(3)
    g = Q.load_q_case("geo_q_40x56_b3", GOLDEN)
    d1, d2, K1, K2, T1, T2, q = _args(g)
    d1, d2 = d1.copy(), d2.copy()
    for arr in (d1, d2):
        for val in (np.nan, np.inf, -np.inf, 0.0, -1.5, 3e38, 1e-30):
            idx = tuple(rng.integers(0, s, size=12) for s in arr.shape)
            arr[idx] = val
    mask, thres, count = geo.geo_valid_masks(m, d1, d2, K1, K2, T1, T2, q, return_thres=True)
    torch.cuda.synchronize()
    print(f"[geo_q] hostile depths: count {int(count)} thres {float(thres)!r} True {int(mask.sum())}")
    assert 0 <= int(count) <= d1.size and int(mask.sum()) <= int(count)
    pcs = geo.compute_local_pointclouds(m, d1, K1)
    geo.depth_from_pointcloud_dot_batched(m, pcs, K1)
    torch.cuda.synchronize()


def test_second_call_of_a_shape_allocates_nothing_and_repeats_bit_identically(m):
    import torch
    from vista_slam_amd import geo
    g = Q.load_q_case("geo_q_224_b3", GOLDEN)
    r = Q.load_ray_case("geo_ray_40x56_n4", GOLDEN)
    a = [torch.from_numpy(x).cuda() for x in _args(g)[:6]]
    q = float(g["q"])
    dr, Kr, pr = (torch.from_numpy(r[k]).cuda() for k in ("depth", "K", "pc_b"))
    first = geo.geo_valid_masks(m, *a, q, return_thres=True)
    pc1, rd1 = geo.compute_local_pointclouds(m, dr, Kr), geo.depth_from_pointcloud_dot_batched(m, pr, Kr)
    a0 = m.alloc_stats()
    second = geo.geo_valid_masks(m, *a, q, return_thres=True)
    assert m.alloc_stats() == a0
    pc2, rd2 = geo.compute_local_pointclouds(m, dr, Kr), geo.depth_from_pointcloud_dot_batched(m, pr, Kr)
    assert m.alloc_stats() == a0
    assert all(torch.equal(x, y) for x, y in zip(first, second)) and torch.equal(pc1, pc2) and torch.equal(rd1, rd2)
    # a smaller batch in between leaves nothing behind in the shared state
    geo.geo_valid_masks(m, *[x[:1] for x in a], 0.3)
    third = geo.geo_valid_masks(m, *a, q, return_thres=True)
    assert m.alloc_stats() == a0 and all(torch.equal(x, y) for x, y in zip(first, third))


def test_round_trip_points_to_ray_depths(m):
    """depth_from_pointcloud_dot_batched(compute_local_pointclouds(d, K), K) = d |K^-1 [x, y, 1]|, within the geo_ray bound."""
    from vista_slam_amd import geo
    for name in Q.RAY_CASES:
        g = Q.load_ray_case(name, GOLDEN)
        n, H, W = Q.RAY_CASES[name]
        bound = G.BAND_FACTOR * float(g["dev_rd"])
        for Kf in (g["K"], g["K"][0]):
            rd = geo.depth_from_pointcloud_dot_batched(m, geo.compute_local_pointclouds(m, g["depth"], Kf), Kf).cpu().numpy()
            K64 = np.broadcast_to(np.asarray(Kf, np.float64), (n, 3, 3))
            rays = Q.local_points_np(np.ones((n, H, W)), K64, np.float64)
            want = g["depth"].astype(np.float64) * np.linalg.norm(rays, axis=-1)
            dist = Q.rd_distance(rd, want)
            print(f"[geo_q] round trip {name} K{list(np.shape(Kf))}: {dist.max():.3e} relative, bound {bound:.3e}")
            assert dist.max() <= bound
