"""CPU: the geometric-consistency fixtures (tests/golden/geo_*.npz, tools/gen_golden_geo.py) meet the conditions they were
generated under, the numpy restatements of tests/geo_cases.py reproduce the reference's recorded output by the fixtures' own
rule, the reference's quirks hold as unit cases, and the C ABI declares the two entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import geo_cases as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return G.load_case(name, GOLDEN)


@pytest.mark.parametrize("name", list(G.VOTE_CASES))
def test_vote_fixture_conditions_and_restatement(name):
    g = load(name)
    n, H, W = G.VOTE_CASES[name]
    window, thr = int(g["window"]), float(g["threshold"])
    assert g["depth"].shape == (n, H, W) and g["depth"].dtype == np.float32 and window == 4 and thr == G.VOTE_THRESHOLD
    depth, K, T = g["depth"], g["K"], g["poses"]
    assert K.shape == (n, 3, 3) and T.shape == (n, 4, 4) and K.dtype == T.dtype == np.float32
    assert float(g["band"]) == G.BAND_FACTOR * float(g["dev"]) and 0 < float(g["band"]) < 0.1 * thr
    nb, ref = g["nb"].astype(np.int32), g["count"].astype(np.int32)
    assert (nb > 0).mean() <= G.MAX_BORDERLINE
    assert sorted(np.unique(ref).tolist()) == list(range(min(2 * window, n - 1) + 1))
    # band and nb as stored follow from the fp64 restatement; the reference's fp32 output and the fp32 restatement obey the rule
    e64 = G.vote_errors(depth, K, T, window, np.float64)
    assert np.array_equal(G.vote_borderline(e64, thr, float(g["band"])), nb)
    c64 = G.vote_count(e64, thr)
    assert np.array_equal(c64, g["count64"].astype(np.int32))
    assert G.check_votes(ref, c64, nb) == 0
    e32 = G.vote_errors(depth, K, T, window, np.float32)
    with np.errstate(invalid="ignore"):                                        # (inf - inf in the slots of absent neighbours)
        assert np.abs(e32.astype(np.float64) - e64)[np.isfinite(e64)].max() <= float(g["band"])
    c32 = G.vote_count(e32, thr)
    assert G.check_votes(c32, ref, nb) == 0 and G.check_votes(c32, c64, nb) == 0


@pytest.mark.parametrize("name", list(G.SYM_CASES))
def test_mask_fixture_conditions_and_restatement(name):
    g = load(name)
    depths, K, rel = g["depths"], g["K"], g["rel_pose"]
    P, _, H, W = depths.shape
    assert (H, W) == G.SYM_CASES[name][:2] and P == len(G.SYM_CASES[name][3]) and depths.dtype == np.float32
    mask, border = g["mask"], g["border"]
    assert float(g["band_uv"]) == G.BAND_FACTOR * float(g["dev_uv"]) and float(g["band_err"]) == G.BAND_FACTOR * float(g["dev_err"])
    assert 0 < float(g["band_uv"]) < 0.01 and 0 < float(g["band_err"]) < 1e-3
    assert border.mean() <= G.MAX_BORDERLINE
    assert G.MIN_MASK_SHARE <= mask.mean() <= 1 - G.MIN_MASK_SHARE
    for p in range(P):
        p32, p64 = G.sym_parts(depths[p], K[p], rel[p], np.float32), G.sym_parts(depths[p], K[p], rel[p], np.float64)
        assert np.array_equal(G.sym_border(p64, g["thres"][p], float(g["band_uv"]), float(g["band_err"])), border[p])
        assert G.check_masks(mask[p], p64["mask"], border[p]) == 0             # the reference against fp64
        assert G.check_masks(p32["mask"], mask[p], border[p]) == 0             # the fp32 restatement against the reference
        assert np.abs(p32["thres"].astype(np.float64) - g["thres"][p]).max() <= 2 * float(g["band_err"])
        assert np.abs(g["thres"][p].astype(np.float64) - g["thres64"][p]).max() <= 2 * float(g["band_err"])
    if name.endswith("empty"):
        assert g["thres"][1, 0] == np.float32(1e10) and not mask[1, 0].any() and mask[1, 1].any()


def _two_views(H=6, W=8, d=2.0):
    K = np.array([[8.0, 0, W / 2.0], [0, 8.0, H / 2.0], [0, 0, 1]], np.float32)
    return np.full((H, W), d, np.float32), K


def test_window_is_four_views_not_two():
    """slam_utils.py:384: range(max(0, i-4), min(n, i+5)) - the docstring's +-2 is not what runs."""
    d, K = _two_views()
    n = 9
    depth, Ks, Ts = np.stack([d] * n), np.stack([K] * n), np.stack([np.eye(4, dtype=np.float32)] * n)
    c = G.view_consistency_np(depth, Ks, Ts)
    assert (c[4] == 8).all() and (c[0] == 4).all() and (c[8] == 4).all() and (c[2] == 6).all()
    assert (G.view_consistency_np(depth, Ks, Ts, window=2)[4] == 4).all()


def test_point_behind_a_neighbour_outside_its_frame_agrees():
    """z is clamped to 1e-6 and uv divides by the UNCLAMPED coordinate: a point behind view j lands outside the frame, samples the
    zero padding, and |0 - 1e-6| < threshold: it AGREES (depth_proj > 0 is always true)."""
    d, K = _two_views()
    T1 = np.eye(4, dtype=np.float32); T1[2, 3] = 5.0                         # view 1 stands 5 m ahead: view 0's points (z = 2) lie behind it
    T1[0, 3] = 40.0                                                            # ... and far to the side: uv outside the frame
    depth, Ks, Ts = np.stack([d, d]), np.stack([K, K]), np.stack([np.eye(4, dtype=np.float32), T1])
    e = G.vote_errors(depth, Ks, Ts, 4, np.float32)
    assert np.allclose(e[0, 4], 1e-6, rtol=1e-3) and (G.vote_count(e, 0.05)[0] == 1).all()
    assert (G.vote_count(e, 1e-6)[0] == 0).all()                               # strict <: not with threshold <= 1e-6


def test_round_half_to_even_at_an_exact_half():
    """uv = 2.5 rounds to 2, 3.5 to 4 (torch.round); the error is read at the rounded pixel."""
    H, W = 4, 8
    K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]], np.float32)          # uv = (x + tx / d, y)
    d0 = np.ones((H, W), np.float32)
    d1 = np.tile(np.arange(W, dtype=np.float32)[None], (H, 1)) + 1.0           # target depth tells which column was read
    rel = np.eye(4, dtype=np.float32); rel[0, 3] = 0.5                         # u = x + 0.5 exactly (1e-8 vanishes next to 1)
    p = G.sym_parts(np.stack([d0, d1]), K, rel, np.float32)
    assert np.array_equal(p["uv"][0, 0].reshape(H, W)[0], np.arange(W, dtype=np.float32) + 0.5)
    cols = np.round(np.arange(W) + 0.5)                                        # 0, 2, 2, 4, 4, 6, 6, 8
    assert cols.tolist() == [0, 2, 2, 4, 4, 6, 6, 8]
    err = p["err"][0].reshape(H, W)[0]
    assert np.array_equal(err[:7], np.abs(cols[:7] + 1.0 - 1.0)) and not p["valid"][0].reshape(H, W)[0, 7]


def test_lower_median_for_an_even_count():
    """torch.median of an even number of elements is the LOWER middle one: 4 valid errors 0, 1, 2, 3 -> median 1, thres 2."""
    H, W = 1, 4
    K = np.eye(3, dtype=np.float32)
    d0 = np.ones((H, W), np.float32)
    d1 = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
    p = G.sym_parts(np.stack([d0, d1]), K, np.eye(4, dtype=np.float32), np.float32)
    assert p["valid"][0].all() and p["thres"][0] == 2.0
    assert p["mask"][0].reshape(-1).tolist() == [True, True, False, False]   # err < 2: 0 and 1 only (strict)


def test_empty_direction_is_1e10_and_all_false():
    depths, K, rel = G.empty_direction_pair(48, 64)
    for dt in (np.float32, np.float64):
        p = G.sym_parts(depths, K, rel, dt)
        assert not p["valid"][0].any() and p["thres"][0] == dt(1e10) and not p["mask"][0].any()
        assert p["valid"][1].mean() > 0.9 and 0.5 < p["mask"][1].mean() < 0.95


def test_nan_among_the_valid_errors_makes_the_direction_false():
    d, K = _two_views()
    d1 = d.copy(); d1[2, 3] = np.nan
    p = G.sym_parts(np.stack([d, d1]), K, np.eye(4, dtype=np.float32), np.float32)
    assert np.isnan(p["thres"][0]) and not p["mask"][0].any()


def test_signatures_hold_the_two_prototypes():
    from vista_slam_amd import _lib
    _vp, _i, _f = C.c_void_p, C.c_int, C.c_float
    assert _lib.SIGNATURES["sta_view_consistency"] == (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _vp])
    assert _lib.SIGNATURES["sta_symmetric_geo_mask"] == (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp])
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "sta_mi355.h")).read()
    assert "STA_API int sta_view_consistency(" in hdr and "STA_API int sta_symmetric_geo_mask(" in hdr


def test_python_entry_points_exist_and_defaults_are_the_reference():
    import inspect
    from vista_slam_amd import formats, geo
    sig = inspect.signature(geo.view_consistency_check)
    assert list(sig.parameters)[:4] == ["frontend", "depth", "intrinsics", "poses"]
    assert sig.parameters["threshold"].default == 0.05 and sig.parameters["window"].default == 4
    assert list(inspect.signature(geo.compute_symmetric_geo_valid_mask).parameters) == ["frontend", "depths", "intri", "relative_pose"]
    assert inspect.signature(geo.symmetric_geo_valid_masks).parameters["return_thres"].default is False
    for fn in (formats.world_pointcloud, formats.save_data_all):
        p = inspect.signature(fn).parameters
        assert p["counts"].default is None and p["min_views"].default == 0
