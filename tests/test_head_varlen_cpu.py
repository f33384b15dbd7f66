"""CPU: the fixture `dptv_tiny_b4_edges` (tools/gen_golden_dptv.py: the REFERENCE's head_pts on eight rectangular sides of different
shape, each alone) and the parts of sta_head_pts_varlen that need no device.

  * the fixture exists, stays below the committed-file limit, holds the eight shapes in the pack order the generator documents (the
    two 2x8 sides adjacent) and full-size maps for every side;
  * the borders matter: `alt_stacked` - the reference on the two adjacent 2x8 sides fed as ONE 4x8 image - is >= 3e-3 (3 x the GPU
    parity bar) away from the recorded points.  Recorded: 0.230 on the points, 2.3e-3 on the confidence (not the witness);
  * it regenerates bit for bit where the reference tree is present;
  * the host-only plan (sta_debug_dpt_varlen_plan): for lists of shapes that include the fixture's, every level's offsets are the
    prefix sums of its entries' pixels, sizes follow (ceil(h/2), ceil(w/2)), (h, w), (2h, 2w), (4h, 4w), (8h, 8w), (16h, 16w), and the
    tile map of the halo-tiled convolution - tile -> (entry, y0, x0), decoded by vl_tile, the function the kernel decodes its block
    index with - is a bijection onto the 8 x 32 tiles of the entries, entry-major and row-major;
  * sta_head_pts_varlen is part of the product ABI, declared in the header, and refuses a null handle without touching a device.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from helpers import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_dptv as GEN          # noqa: E402  (the case table only: the reference is imported inside build)

NAME = "dptv_tiny_b4_edges"
SHAPES_A, SHAPES_B = [(1, 1), (1, 9), (5, 1), (2, 8)], [(2, 8), (3, 5), (4, 4), (6, 10)]
ALT_STACKED_MIN = 3e-3


def test_fixture_holds_the_eight_sides():
    path = os.path.join(ROOT, "tests", "golden", NAME + ".npz")
    assert os.path.exists(path) and os.path.getsize(path) <= (1 << 20)
    g, meta = load_golden(NAME)
    assert int(meta["B"]) == 4 and int(meta["sub"]) == 1 and int(meta["tsub"]) == 1
    assert [tuple(r) for r in g["rect_a"].tolist()] == SHAPES_A == GEN.SHAPES[0]
    assert [tuple(r) for r in g["rect_b"].tolist()] == SHAPES_B == GEN.SHAPES[1]
    assert SHAPES_A[-1] == SHAPES_B[0] == (2, 8)          # adjacent in the pack order: side a of the entries, then side b
    assert 0 < float(g["ref_noise"]) <= 1e-4
    for tag, shapes in (("a", SHAPES_A), ("b", SHAPES_B)):
        for b, (h, w) in enumerate(shapes):
            assert g[f"feat_{tag}_e{b}"].shape[0] == h * w == int(g["n1" if tag == "a" else "n2"][b])
            view = (16 * w, 16 * h) if h > w else (16 * h, 16 * w)          # h > w: the reference wrapper's transposed view (utils/misc.py:48-61)
            assert g[f"{tag}_pts3d_e{b}"].shape == view + (3,) and g[f"{tag}_conf_e{b}"].shape == view
            assert np.isfinite(g[f"{tag}_pts3d_e{b}"]).all() and (g[f"{tag}_conf_e{b}"] > 1.0).all()


def test_the_borders_matter():
    g, _ = load_golden(NAME)
    print("alt_stacked", float(g["alt_stacked"]), "confidence", float(g["alt_stacked_conf"]))
    assert float(g["alt_stacked"]) >= ALT_STACKED_MIN


def test_fixture_regenerates_bit_for_bit():
    from oracle import ref_import
    if not os.path.isdir(ref_import.REF_ROOT):
        pytest.skip("reference tree not present (fixtures are regenerated where it is)")
    g, meta = load_golden(NAME)
    res = GEN.build()
    for k in g:
        assert np.array_equal(np.asarray(res[k]), g[k]), k
    assert set(res) - {"meta_keys", "meta_vals"} == set(g)
    assert float(res["alt_stacked"]) >= ALT_STACKED_MIN


SHAPE_LISTS = [SHAPES_A + SHAPES_B, [(1, 1)], [(6, 10)] * 3, [(5, 1), (1, 1), (1, 9), (8, 10), (3, 5)] * 6 + [(2, 8), (2, 8)],
               [(16, 20)] * 10, [(7, 3), (1, 2), (2, 1)]]


@pytest.mark.parametrize("shapes", SHAPE_LISTS, ids=[f"B{len(s)}" for s in SHAPE_LISTS])
def test_level_plan_offsets_and_sizes(shapes):
    from vista_slam_amd import _lib
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libsta_mi355_test.so not built here (python -m vista_slam_amd.build)")
    lib = _lib.load_test()
    B = len(shapes)
    off = (C.c_longlong * (6 * (B + 1)))()
    hw = (C.c_int * (6 * B * 2))()
    hp, wp = (C.c_int * B)(*[s[0] for s in shapes]), (C.c_int * B)(*[s[1] for s in shapes])
    nt = (C.c_int * 6)()
    _lib.check(lib.sta_debug_dpt_varlen_plan(B, hp, wp, off, hw, nt, None, 0))          # the counts alone
    cap = sum(nt)
    tiles = (C.c_int * (3 * cap))()
    _lib.check(lib.sta_debug_dpt_varlen_plan(B, hp, wp, off, hw, nt, tiles, cap))
    assert lib.sta_debug_dpt_varlen_plan(B, hp, wp, off, hw, nt, tiles, cap - 1) == -1
    off = np.array(off[:]).reshape(6, B + 1)
    hw = np.array(hw[:]).reshape(6, B, 2)
    tiles = np.array(tiles[:]).reshape(cap, 3)
    at = 0
    for k in range(6):
        # the tile map of level k: exactly the tiles (b, 8 i, 32 j) of every entry, each once, entry-major and row-major inside an entry
        want = [(b, 8 * i, 32 * j) for b in range(B) for i in range(-(-int(hw[k, b, 0]) // 8)) for j in range(-(-int(hw[k, b, 1]) // 32))]
        got = [tuple(int(v) for v in t) for t in tiles[at:at + nt[k]]]
        assert nt[k] == len(want) and got == want, (k, nt[k], len(want))
        assert len(set(got)) == len(got)
        at += nt[k]
        for b, (h, w) in enumerate(shapes):
            want = (-(-h // 2), -(-w // 2)) if k == 0 else (h << (k - 1), w << (k - 1))
            assert tuple(hw[k, b]) == want, (k, b)
        sizes = hw[k, :, 0].astype(np.int64) * hw[k, :, 1]
        assert off[k, 0] == 0 and np.array_equal(off[k, 1:], np.cumsum(sizes)), k          # prefix sums: no gap, no overlap
    assert at == cap
    assert lib.sta_debug_dpt_varlen_plan(33, None, None, None, None, None, None, 0) == -1


def test_entry_is_in_the_product_abi_and_refuses_a_null_handle():
    from vista_slam_amd import _lib
    assert "sta_head_pts_varlen" in _lib.SIGNATURES and "sta_head_pts_varlen" not in _lib.TEST_SIGNATURES
    for hook in ("sta_debug_conv3x3_varlen", "sta_debug_conv3_head_varlen", "sta_debug_convt_varlen", "sta_debug_up2_varlen", "sta_debug_dpt_varlen_plan"):
        assert hook in _lib.TEST_SIGNATURES and hook not in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsta_mi355.so not built here (python -m vista_slam_amd.build)")
    lib = _lib.load()
    one64, one = (C.c_int64 * 1)(0), (C.c_int * 1)(1)
    assert lib.sta_head_pts_varlen(None, None, one64, None, None, None, one64, one, one, 1, None, None, None, None) == -1
    assert b"null handle" in lib.sta_last_error()
    with open(os.path.join(ROOT, "include", "sta_mi355.h")) as f:
        assert "STA_API int sta_head_pts_varlen(" in f.read()


def test_heads_switch_refuses_unknown_values():
    """forward_pairs_tokens(heads=...) and the scheduler's keyword refuse an unknown value before they touch a device: called here on
    an object that has no handle at all."""
    import inspect
    from vista_slam_amd import slam_scheduler
    from vista_slam_amd.sta_frontend import STAFrontend
    assert inspect.signature(STAFrontend.forward_pairs_tokens).parameters["heads"].default == "entry"
    bare = object.__new__(STAFrontend)
    with pytest.raises(ValueError, match="heads must be"):
        bare.forward_pairs_tokens([None], [None], [None], [None], heads="both")
    with pytest.raises(ValueError, match="heads must be"):
        slam_scheduler.regress_views_tokens(bare, None, (32, 32), [], [], [], [], [], 0.5, heads="both")
