"""CPU: the quantile-mask and ray fixtures (tests/golden/geo_q_*.npz, geo_ray_*.npz, tools/gen_golden_geo_q.py) meet the conditions
they were generated under, the numpy restatements of tests/geo_q_cases.py reproduce the reference's recorded output by the
fixtures' own rule, the quantile restatement equals torch.quantile bit for bit, the reference's quirks hold as unit cases, and the
C ABI declares the three entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import geo_cases as G
import geo_q_cases as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", list(Q.Q_CASES))
def test_mask_fixture_conditions_and_restatement(name):
    g = Q.load_q_case(name, GOLDEN)
    H, W, _n, pairs, q, _nan = Q.Q_CASES[name]
    d1, d2 = g["depth1"], g["depth2"]
    assert d1.shape == d2.shape == (len(pairs), H, W) and d1.dtype == np.float32 and float(g["q"]) == q
    d1s, d2s, K1, K2, T1, T2, _q = Q.q_case_inputs(name)                        # the fixture holds the case's scene
    assert np.array_equal(d1, d1s) and np.array_equal(d2, Q.apply_nan(name, d2s), equal_nan=True)
    for k, v in (("K1", K1), ("K2", K2), ("T1", T1), ("T2", T2)):
        assert np.array_equal(g[k], v) and g[k].dtype == np.float32
    assert not np.array_equal(K1, K2)
    band_uv, band_err = float(g["band_uv"]), float(g["band_err"])
    assert band_uv == G.BAND_FACTOR * float(g["dev_uv"]) and band_err == G.BAND_FACTOR * float(g["dev_err"])
    assert 0 < band_uv < 0.01 and 0 < band_err < 1e-4
    assert float(g["thr_tol"]) == 2 * band_err + float(g["spread"])
    mask, border = g["mask"], g["border"]
    assert border.mean() <= G.MAX_BORDERLINE
    if name in Q.ALL_FALSE:
        assert not mask.any()
    else:
        assert G.MIN_MASK_SHARE <= mask.mean() <= 1 - G.MIN_MASK_SHARE
    p32, p64 = Q.q_parts(d1, d2, K1, K2, T1, T2, q, np.float32), Q.q_parts(d1, d2, K1, K2, T1, T2, q, np.float64)
    # what is stored follows from the restatements
    assert np.array_equal(Q.q_uv_border(p64, band_uv).reshape(mask.shape), g["uv_border"])
    assert np.array_equal(Q.q_border(p64, g["thres"], band_uv, band_err), border)
    assert Q.q_spread(p64, d2, q, band_uv) == float(g["spread"])
    assert np.array_equal(p32["thres"], g["thres"], equal_nan=True) and np.array_equal(p64["thres"], g["thres64"], equal_nan=True)
    assert p32["count"] == int(g["count"]) and p64["count"] == int(g["count64"])
    dev_uv, dev_err = Q.q_deviation(p32, p64, H, W)
    assert dev_uv <= band_uv and dev_err <= band_err
    # the conditions
    if np.isfinite(g["thres64"]):
        assert float(g["spread"]) <= Q.MAX_SPREAD_REL * float(g["thres64"])
    else:
        assert name.endswith("_nan") and np.isnan(g["thres"])
    assert Q.check_q_masks(mask, p64["mask"], border) == 0                     # the reference against fp64
    assert Q.check_q_masks(p32["mask"], mask, border) == 0                     # the fp32 restatement against the reference
    assert Q.check_q_masks(p32["mask"], p64["mask"], border) == 0
    assert Q.thres_within(g["thres"], g["thres64"], float(g["thr_tol"]))
    assert abs(int(g["count"]) - int(g["count64"])) <= int(g["uv_border"].sum())
    if name.endswith("q037") or name.endswith("224_b3"):
        assert float(g["min_z2"]) < 0                                          # points behind camera 2 take part


@pytest.mark.parametrize("name", list(Q.RAY_CASES))
def test_ray_fixture_conditions_and_restatement(name):
    g = Q.load_ray_case(name, GOLDEN)
    n, H, W = Q.RAY_CASES[name]
    depth, K = g["depth"], g["K"]
    assert depth.shape == (n, H, W) and K.shape == (n, 3, 3)
    dev_pc, dev_rd = float(g["dev_pc"]), float(g["dev_rd"])
    assert 0 < dev_pc < 1e-6 and 0 < dev_rd < 1e-6
    worst_pc = worst_rd = 0.0
    for tag, Kf in (("b", K), ("s", K[0])):
        pc, rd, pc64, rd64 = g[f"pc_{tag}"], g[f"rd_{tag}"], g[f"pc64_{tag}"], g[f"rd64_{tag}"]
        assert pc.shape == (n, H, W, 3) and rd.shape == (n, H, W) and pc.dtype == rd.dtype == np.float32
        assert np.array_equal(Q.local_points_np(depth, Kf, np.float64), pc64) and np.array_equal(Q.ray_depth_np(pc, Kf, np.float64), rd64)
        worst_pc = max(worst_pc, float(Q.pc_distance(pc, pc64).max())); worst_rd = max(worst_rd, float(Q.rd_distance(rd, rd64).max()))
        # the fp32 restatement obeys the rule
        assert Q.pc_distance(Q.local_points_np(depth, Kf, np.float32), pc64).max() <= G.BAND_FACTOR * dev_pc
        assert Q.rd_distance(Q.ray_depth_np(pc, Kf, np.float32), rd64).max() <= G.BAND_FACTOR * dev_rd
    assert worst_pc == dev_pc and worst_rd == dev_rd
    # the shared and the batched form agree on view 0, whose K is the shared one
    assert np.array_equal(g["pc64_b"][0], g["pc64_s"][0])


def test_quantile_restatement_equals_torch_bit_for_bit():
    import torch
    n_cases = 0
    for si, (B, H, W) in enumerate(Q.EXACT_SHAPES):
        for s in (3, 11):
            d = Q.exact_depths(B, H, W, s, seed=100 + si)
            for q in Q.EXACT_QS:
                want = torch.quantile(torch.from_numpy(d).flatten(), q).numpy()
                got = Q.quantile_np(d, q, np.float32)
                assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (B, H, W, s, q, got, want)
                n_cases += 1
    assert n_cases == 80
    # free-form values too (rounding in every step), and NaN / empty
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 1000, 4481):
        v = rng.standard_normal(n).astype(np.float32) ** 2
        for q in Q.EXACT_QS + [0.25, 0.6180339]:
            assert Q.quantile_np(v, q).tobytes() == torch.quantile(torch.from_numpy(v), q).numpy().tobytes(), (n, q)
    v[3] = np.nan
    assert np.isnan(Q.quantile_np(v, 0.5)) and torch.isnan(torch.quantile(torch.from_numpy(v), 0.5))
    with pytest.raises(RuntimeError):
        Q.quantile_np(np.zeros(0, np.float32), 0.5)
    with pytest.raises(RuntimeError):
        torch.quantile(torch.zeros(0), 0.5)


def test_exact_construction_maps_every_pixel_onto_itself():
    """The GPU test's construction, through the restatement: all pixels valid, err == depth1, thres == torch.quantile(depth1)."""
    import torch
    B, H, W = 2, 5, 7
    d1 = Q.exact_depths(B, H, W, 11, seed=1)
    K = np.stack([np.eye(3, dtype=np.float32)] * B); T = np.stack([np.eye(4, dtype=np.float32)] * B)
    p = Q.q_parts(d1, np.zeros_like(d1), K, K, T, T, 0.37, np.float32)
    assert p["valid"].all() and np.array_equal(p["err"].reshape(B, H, W), d1)
    want = torch.quantile(torch.from_numpy(d1).flatten(), 0.37).numpy()
    assert p["thres"].tobytes() == want.tobytes() and np.array_equal(p["mask"], d1 < want)


def _flat_pair(H=4, W=8, d=1.0):
    K = np.eye(3, dtype=np.float32)[None].copy()
    return np.full((1, H, W), d, np.float32), K, np.eye(4, dtype=np.float32)[None].copy()


def test_target_pixel_is_truncated_toward_zero():
    """u2 = x + t / d: with t = -0.5 column 0 lands at u2 = -0.5, which int() sends to column 0 (valid); round-to-nearest or floor
    would not.  With t = +0.5 every column reads itself, where rounding would read the next one."""
    H, W = 4, 8
    d1, K, T1 = _flat_pair(H, W)
    d2 = np.tile(np.arange(W, dtype=np.float32)[None, None], (1, H, 1)) + 1.0           # the target depth tells which column was read
    for tx in (-0.5, 0.5):
        T = T1.copy(); T[0, 0, 3] = tx
        p = Q.q_parts(d1, d2, K, K, T, np.eye(4, dtype=np.float32)[None], 1.0, np.float32)
        cols = np.trunc(np.arange(W) + tx)
        assert p["valid"].all()
        assert np.array_equal(p["err"].reshape(H, W)[0], np.abs(1.0 - (cols + 1.0)))
    T = T1.copy(); T[0, 0, 3] = -1.0                                             # u2 = -1 exactly: int() = -1, invalid
    p = Q.q_parts(d1, d2, K, K, T, np.eye(4, dtype=np.float32)[None], 1.0, np.float32)
    assert not p["valid"].reshape(H, W)[:, 0].any() and p["valid"].reshape(H, W)[:, 1:].all()


def test_points_behind_camera_two_project_and_count():
    """z2 < 0 divides like any other z2: (x2, y2, z2) and (-x2, -y2, -z2) land on the same pixel."""
    H, W = 4, 8
    d1, _K, _T = _flat_pair(H, W)
    K = np.array([[[2.0, 0, 4.0], [0, 2.0, 2.0], [0, 0, 1]]], np.float32)
    T2 = np.eye(4, dtype=np.float32)[None].copy(); T2[0, 2, 3] = 3.0             # camera 2 stands 3 m ahead of the points at z = 1
    p = Q.q_parts(d1, np.zeros_like(d1), K, K, np.eye(4, dtype=np.float32)[None], T2, 0.5, np.float32)
    assert (p["z2"] == -2.0).all() and p["valid"].any() and p["count"] == int(p["valid"].sum()) > 0
    assert (p["err"][p["valid"]] == 2.0).all()


def test_non_finite_and_huge_coordinates_are_invalid_and_nan_errors_clear_the_mask():
    H, W = 4, 8
    d1, K, T = _flat_pair(H, W)
    d1[0, 1, 2] = np.inf; d1[0, 2, 3] = np.nan; d1[0, 3, 4] = 0.0                # u2 = x + 3e9 / d: z = 0 divides to +-inf / NaN
    T1 = T.copy(); T1[0, 0, 3] = 0.25
    p = Q.q_parts(d1, np.ones_like(d1), K, K, T1, T, 0.5, np.float32)
    v = p["valid"].reshape(H, W)
    assert not v[2, 3] and not v[3, 4]
    big = T.copy(); big[0, 0, 3] = 3e9
    assert not Q.q_parts(np.ones_like(d1), np.ones_like(d1), K, K, big, T, 0.5, np.float32)["valid"].any()
    d2 = np.ones((1, H, W), np.float32); d2[0, 1, 1] = np.nan
    p = Q.q_parts(np.ones_like(d1), d2, K, K, T, T, 0.5, np.float32)
    assert p["valid"].all() and np.isnan(p["thres"]) and not p["mask"].any()


def test_one_threshold_for_the_whole_batch_and_strict_less_than():
    d1 = np.stack([np.full((2, 2), 1.0, np.float32), np.full((2, 2), 3.0, np.float32)])
    K = np.stack([np.eye(3, dtype=np.float32)] * 2); T = np.stack([np.eye(4, dtype=np.float32)] * 2)
    p = Q.q_parts(d1, np.zeros_like(d1), K, K, T, T, 0.5, np.float32)
    assert p["thres"] == 2.0 and p["mask"][0].all() and not p["mask"][1].any()  # per image it would be 1.0 and 3.0: nothing below
    p = Q.q_parts(d1, np.zeros_like(d1), K, K, T, T, 1.0, np.float32)
    assert p["thres"] == 3.0 and p["mask"][0].all() and not p["mask"][1].any()  # err < thres is strict


def test_only_four_entries_of_each_intrinsics_matrix_are_read():
    d1, d2, K1, K2, T1, T2, q = Q.q_case_inputs("geo_q_40x56_b3")
    a = Q.q_parts(d1, d2, K1, K2, T1, T2, q, np.float32)
    K1b, K2b = K1.copy(), K2.copy()
    for K in (K1b, K2b):
        K[:, 0, 1] = 7.0; K[:, 1, 0] = -3.0; K[:, 2] = (5.0, 6.0, 9.0)
    b = Q.q_parts(d1, d2, K1b, K2b, T1, T2, q, np.float32)
    assert np.array_equal(a["mask"], b["mask"]) and a["thres"] == b["thres"]


def test_signatures_hold_the_three_prototypes():
    from vista_slam_amd import _lib
    _vp, _i, _f = C.c_void_p, C.c_int, C.c_float
    assert _lib.SIGNATURES["sta_geo_valid_mask"] == (_i, [_vp] * 7 + [_i, _i, _i, _f, _vp, _vp, _vp, _vp])
    assert _lib.SIGNATURES["sta_local_pointclouds"] == (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp])
    assert _lib.SIGNATURES["sta_ray_depth"] == (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp])
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "sta_mi355.h")).read()
    for name in ("sta_geo_valid_mask", "sta_local_pointclouds", "sta_ray_depth"):
        assert f"STA_API int {name}(" in hdr


def test_python_entry_points_keep_the_reference_argument_order():
    import inspect
    from vista_slam_amd import geo
    assert list(inspect.signature(geo.compute_geo_valid_mask_batched).parameters) == \
        ["frontend", "depth1", "depth2", "K1", "K2", "T1", "T2", "error_thres_rel"]
    assert list(inspect.signature(geo.compute_local_pointclouds).parameters) == ["frontend", "depths", "intrinsics"]
    assert list(inspect.signature(geo.depth_from_pointcloud_dot_batched).parameters) == ["frontend", "pointclouds", "intrinsics"]
    p = inspect.signature(geo.geo_valid_masks).parameters
    assert list(p)[:8] == ["frontend", "depth1", "depth2", "K1", "K2", "T1", "T2", "error_thres_rel"] and p["return_thres"].default is False
