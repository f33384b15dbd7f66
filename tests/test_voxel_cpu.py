"""CPU: the numpy restatement of sta_voxel_downsample's contract (tests/voxel_cases.py) against a dict-of-lists brute force in plain
Python, and formats.voxel_plan - the host-side half of the call: grid corner, index ranges, key widths, sort passes, refusals."""
import ctypes as C
import inspect

import numpy as np
import pytest

import voxel_cases as V


@pytest.mark.parametrize("name", V.SMALL)
def test_restatement_matches_brute_force(name):
    """Keys, row order, counts, means (bit for bit: both add in ascending input order), indices, inverse, dropped count."""
    c, exp = V.expected_of(name)
    bf = V.brute_force(c["pts"], c["col"], voxel_size=c["voxel_size"], origin=c["origin"], min_points=c["min_points"])
    assert exp["V"] == bf["V"] and exp["n_dropped"] == bf["n_dropped"]
    assert exp["counts"].tolist() == bf["counts"]
    assert exp["index"].tolist() == bf["index"]
    assert exp["inverse"].tolist() == bf["inverse"]
    assert np.array_equal(exp["points"], np.array(bf["points"], np.float32).reshape(-1, 3))
    assert np.array_equal(exp["colors"], np.array(bf["colors"], np.float32).reshape(-1, 3))
    # rows ascend in (iz, iy, ix)
    idx = exp["index"].astype(np.int64)
    if len(idx) > 1:
        a, b = idx[:-1, ::-1], idx[1:, ::-1]
        assert all(tuple(x) < tuple(y) for x, y in zip(a.tolist(), b.tolist()))


def test_inverse_rows_hold_their_points():
    c, exp = V.expected_of("min_points_2")
    inv = exp["inverse"]
    assert (inv >= -1).all() and inv.max() == exp["V"] - 1
    assert np.array_equal(np.bincount(inv[inv >= 0], minlength=exp["V"]), exp["counts"])
    assert (inv == -1).sum() == len(inv) - exp["counts"].sum()


@pytest.mark.parametrize("name,bits,passes", [("width_1", 1, 1), ("width_8", 8, 1), ("width_9", 9, 2), ("width_16", 16, 2), ("width_17", 17, 3),
                                               ("width_63", 63, 8), ("extent_2p21_on_y", 25, 4), ("one_voxel_300000", 0, 0)])
def test_voxel_plan_widths_and_passes(name, bits, passes):
    from vista_slam_amd import formats
    c, exp = V.expected_of(name)
    p = formats.voxel_plan(c["pts"].min(axis=0), c["pts"].max(axis=0), c["voxel_size"], c["origin"])
    assert p.key_bits == bits == exp["key_bits"] and p.passes == passes and sum(p.bits) == bits
    assert p.extent == tuple(hi - lo + 1 for lo, hi in zip(p.index_min, p.index_max))
    assert all(b == (e - 1).bit_length() for b, e in zip(p.bits, p.extent))
    assert p.index_min == tuple(exp["index"].min(axis=0).tolist()) and p.index_max == tuple(exp["index"].max(axis=0).tolist())
    _, o = V.grid_of(c["pts"], c["voxel_size"], c["origin"])
    assert p.origin == tuple(o.tolist())


def test_voxel_plan_origin_and_negative_indices():
    from vista_slam_amd import formats
    c, exp = V.expected_of("origin_negative_index")
    p = formats.voxel_plan(c["pts"].min(axis=0), c["pts"].max(axis=0), c["voxel_size"], c["origin"])
    assert p.origin == (10.0, 20.0, 30.0) and max(p.index_max) < 0
    assert p.index_min == tuple(exp["index"].min(axis=0).tolist())
    # the default corner is min - voxel_size / 2: the smallest point sits in the middle of voxel 0
    q = formats.voxel_plan([1.0, 2.0, 3.0], [1.0, 2.0, 3.0], 0.5)
    assert q.origin == (0.75, 1.75, 2.75) and q.index_min == q.index_max == (0, 0, 0) and q.key_bits == 0 and q.passes == 0


def test_voxel_plan_refusals():
    from vista_slam_amd import formats
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size must be finite and > 0"):
            formats.voxel_plan([0, 0, 0], [1, 1, 1], bad)
    with pytest.raises(ValueError, match="bounds must be finite"):
        formats.voxel_plan([0, 0, 0], [1, float("inf"), 1], 0.5)
    with pytest.raises(ValueError, match="bounds must be finite"):
        formats.voxel_plan([0, 2, 0], [1, 1, 1], 0.5)
    with pytest.raises(ValueError, match="origin must be finite"):
        formats.voxel_plan([0, 0, 0], [1, 1, 1], 0.5, origin=(0.0, float("nan"), 0.0))
    # extent 2^21 is accepted, 2^21 + 1 refused with the extents in the message - the restatement words it the same way
    formats.voxel_plan([0, 0, 0], [float(V.MAX_EXTENT - 1), 1, 1], 1.0)
    pts = V.too_wide()
    with pytest.raises(ValueError) as lib_msg:
        formats.voxel_plan(pts.min(axis=0), pts.max(axis=0), 1.0)
    with pytest.raises(ValueError) as ref_msg:
        V.expected(pts, voxel_size=1.0)
    assert str(lib_msg.value) == str(ref_msg.value) == "voxel grid too wide: 2097153 x 4 x 4 voxels at voxel_size 1 (at most 2097152 per axis)"
    with pytest.raises(ValueError, match="voxel index outside int32 on axis 1"):
        formats.voxel_plan([0, 0, 0], [1, 1, 1], 1e-3, origin=(0.0, -1e9, 0.0))


def test_entry_points_and_defaults():
    from vista_slam_amd import _lib, formats
    p = inspect.signature(formats.voxel_downsample).parameters
    assert list(p)[:3] == ["frontend", "points", "colors"] and p["colors"].default is None
    assert p["voxel_size"].kind is inspect.Parameter.KEYWORD_ONLY and p["origin"].default is None and p["min_points"].default == 1
    assert all(p[k].default is False for k in ("return_counts", "return_index", "return_inverse", "want_records"))
    w = inspect.signature(formats.world_pointcloud).parameters
    assert w["voxel_size"].default is None and w["voxel_origin"].default is None and w["min_points"].default == 1
    assert inspect.signature(formats.save_data_all).parameters["ply_voxel_size"].default is None
    _vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
    assert _lib.SIGNATURES["sta_voxel_downsample"] == (_i, [_vp, _vp, _vp, _i64, C.c_double, C.POINTER(C.c_double), _i, _vp, _vp, _vp, _vp, _vp,
                                                             _vp, C.POINTER(_i64), _vp])
