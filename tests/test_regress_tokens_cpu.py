"""CPU: the `rvt_*` fixtures - the REFERENCE's `regress_two_views` on per-edge token subsets (tools/gen_golden_rvt.py) -, the parts of
sta_regress_views_tokens that need no device, and the shim's host-side refusals.

  * the fixtures exist, stay below the committed-file limit and are self-consistent: selections as the case table says, map shapes,
    None exactly where an index-list side or a rejected edge has no maps, K exactly on accepted window / window edges of one shape,
    ref_noise <= 1e-4;
  * the selections matter: `alt_whole` - the reference's pose for the same edge on the whole frames - is >= 3e-3 (3 x the GPU parity
    bar) away from the recorded pose for every edge with a proper subset, so a gather that ignored the selection fails the GPU test;
  * the decisions are safe: every |conf - thres| >= 1e-2, 100 x the confidence bound of the GPU test; over the three fixtures a
    non-adjacent edge is rejected, one is accepted, and accepted edges cover window / window, window / index list and index list /
    index list (gen_golden_rvt.check_mixtures);
  * the tiny fixtures regenerate bit for bit at their recorded seed where the reference tree is present;
  * the three entries are product ABI, the two hooks test ABI only, a null handle is refused without a device;
  * `slam_scheduler._selection` refuses what `encode_tokens` refuses.
"""
import os
import sys

import numpy as np
import pytest

from helpers import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_rvt as GEN          # noqa: E402  (the case table only: the reference is imported inside build_case)

NAMES = ["rvt_tiny_k4_edges", "rvt_tiny_k3_win_sharp", "rvt_full_224_k3"]
TINY = NAMES[:2]
# (tokens side i, tokens side j) per edge
COUNTS = {"rvt_tiny_k4_edges": [(30, 30), (6, 12), (17, 16), (1, 65)], "rvt_tiny_k3_win_sharp": [(6, 6), (15, 15), (16, 16)],
          "rvt_full_224_k3": [(196, 196), (80, 196), (140, 196)]}


def test_the_three_fixtures_exist():
    assert NAMES == list(GEN.CASES)
    for n in NAMES:
        path = os.path.join(ROOT, "tests", "golden", n + ".npz")
        assert os.path.exists(path) and os.path.getsize(path) <= (1 << 20), n


@pytest.mark.parametrize("name", NAMES)
def test_fixture_invariants(name):
    from vista_slam_amd import weights as W
    g, meta = load_golden(name)
    c = GEN.CASES[name]
    cfg = W.TINY if c["cfg"] == "tiny" else W.FULL
    k, sub = int(meta["k"]), int(meta["sub"])
    assert k == len(c["edges"]) == len(COUNTS[name]) and float(meta["qk_gain"]) == c.get("qk_gain", 1.0)
    assert g["hw_i"].tolist() == list(c["hw"]) and g["hw_j"].tolist() == [list(e[1]) for e in c["edges"]]
    assert g["adjacent"].tolist() == [e[3] for e in c["edges"]]
    assert g["pose"].shape == (k, 4, 4) and g["conf"].shape == (k,) and g["accepted"].shape == (k,)
    assert 0 < float(g["ref_noise"]) <= 1e-4, float(g["ref_noise"])
    thres = float(g["thres"])
    print(name, "seed", int(meta["seed"]), "thres", thres, "conf", g["conf"].tolist(), "accepted", g["accepted"].tolist(),
          "alt_whole", g["alt_whole"].tolist(), "ref_noise", float(g["ref_noise"]))
    Hi, Wi = c["hw"]
    for e, (sel_i, (Hj, Wj), sel_j, adj) in enumerate(c["edges"]):
        assert abs(float(g["conf"][e]) - thres) >= 1e-2, (e, float(g["conf"][e]), thres)
        assert bool(g["accepted"][e]) == (not (float(g["conf"][e]) < thres and not adj))          # slam.py:169
        grids = []
        for tag, sel, (H, W_) in (("i", sel_i, (Hi, Wi)), ("j", sel_j, (Hj, Wj))):
            win, idx, grid = GEN.selection(sel, H // 16, W_ // 16)
            assert g[f"win_{tag}"][e].tolist() == win.tolist()
            assert (f"idx_{tag}_e{e}" in g) == (grid is None)
            if grid is None:
                assert np.array_equal(g[f"idx_{tag}_e{e}"], idx) and g[f"idx_{tag}_e{e}"].dtype == np.int64
            assert len(idx) == COUNTS[name][e][0 if tag == "i" else 1]
            grids.append(grid)
            has = grid is not None and bool(g["accepted"][e])          # maps: window sides of accepted edges, nothing else
            for key in ("confs", "depths", "confs_l2", "depths_l2"):
                assert (f"{key}_{tag}_e{e}" in g) == has, (key, tag, e)
            if has:
                shape = (len(range(0, 16 * grid[0], sub)), len(range(0, 16 * grid[1], sub)))
                assert g[f"confs_{tag}_e{e}"].shape == shape and g[f"depths_{tag}_e{e}"].shape == shape
        assert (f"intri_e{e}" in g) == (bool(g["accepted"][e]) and grids[0] is not None and grids[0] == grids[1]), e
        if f"intri_e{e}" in g:          # the principal point is the centre of the WINDOW's image
            assert g[f"intri_e{e}"][0, 2] == 8 * grids[0][1] and g[f"intri_e{e}"][1, 2] == 8 * grids[0][0]
        proper = COUNTS[name][e] != ((Hi // 16) * (Wi // 16), (Hj // 16) * (Wj // 16))
        assert bool(g["proper"][e]) == proper
        if proper:
            assert g["alt_whole"][e] >= 3e-3, (e, g["alt_whole"][e])
        else:
            assert g["alt_whole"][e] <= 1e-5          # nothing was left out: the reference against itself
        assert (f"feat_j_e{e}" in g) == (c["cfg"] == "tiny")
        if c["cfg"] == "tiny":
            assert g[f"feat_j_e{e}"].shape == ((Hj // 16) * (Wj // 16), cfg.enc_embed_dim)
    if name == "rvt_tiny_k4_edges":          # edge 0 is accepted only through the adjacency exemption
        assert g["accepted"][0] and float(g["conf"][0]) < thres


def test_decisions_and_mixtures_over_the_three_fixtures():
    GEN.check_mixtures([load_golden(n)[0] for n in NAMES])


@pytest.mark.parametrize("name", TINY)
def test_tiny_fixtures_regenerate_bit_for_bit(name):
    """At the recorded seed (the search for it runs over many seeds: tools/gen_golden_rvt.py)."""
    from oracle import ref_import
    if not os.path.isdir(ref_import.REF_ROOT):
        pytest.skip("reference tree not present (fixtures are regenerated where it is)")
    g, meta = load_golden(name)
    res = GEN.build_case(name, seed=int(meta["seed"]))
    for k in g:
        assert np.array_equal(np.asarray(res[k]), g[k]), k
    assert set(res) - {"meta_keys", "meta_vals"} == set(g)


def test_entries_are_in_the_product_abi_and_refuse_a_null_handle():
    import ctypes as C
    from vista_slam_amd import _lib
    entries = ("sta_regress_views_tokens", "sta_regress_views_tokens_begin", "sta_regress_views_tokens_finish")
    with open(os.path.join(ROOT, "include", "sta_mi355.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "include", "sta_mi355_debug.h")) as f:
        debug_header = f.read()
    for name in entries:
        assert name in _lib.SIGNATURES and name not in _lib.TEST_SIGNATURES
        assert f"STA_API int {name}(" in header and f"{name}(" not in debug_header
    for hook in ("sta_debug_gather_tokens", "sta_debug_pose_rows"):
        assert hook in _lib.TEST_SIGNATURES and hook not in _lib.SIGNATURES
        assert f"STA_API int {hook}(" in debug_header and f"{hook}(" not in header
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsta_mi355.so not built here (python -m vista_slam_amd.build)")
    lib = _lib.load()
    one, win = (C.c_int * 1)(16), (C.c_int * 4)(0, 0, 1, 1)
    fj = (C.c_void_p * 1)()
    host_f, host_i = (C.c_float * 1)(), (C.c_int * 1)()
    assert lib.sta_regress_views_tokens_begin(None, None, 16, 16, fj, one, one, 1, win, one, None, win, one, None, None, None) == -1
    assert b"null handle" in lib.sta_last_error()
    assert lib.sta_regress_views_tokens_finish(None, b"\x00", 0.5, host_f, host_i, host_i, None, None, None, None, host_i, None) == -1
    assert b"null handle" in lib.sta_last_error()
    assert lib.sta_regress_views_tokens(None, None, 16, 16, fj, one, one, 1, win, one, None, win, one, None, b"\x00", 0.5,
                                        None, host_f, host_i, host_i, None, None, None, None, host_i, None) == -1
    assert b"null handle" in lib.sta_last_error()


def test_selection_refusals():
    import torch
    from vista_slam_amd.slam_scheduler import _selection
    assert _selection(None, 5, 6) == ((0, 0, 5, 6), None)
    assert _selection((1, 2, 2, 3), 5, 6) == ((1, 2, 2, 3), None)
    assert _selection([4, 5, 1, 1], 5, 6) == ((4, 5, 1, 1), None)          # the grid's last cell
    win, idx = _selection(torch.tensor([29, 0, 0, 7]), 5, 6)          # any order, repeats
    assert win == (0, 0, 0, 0) and idx.tolist() == [29, 0, 0, 7]
    for bad in ((1, 2, 5, 3), (0, 4, 1, 3), (-1, 0, 1, 1)):
        with pytest.raises(ValueError, match="leaves the 5 x 6"):
            _selection(bad, 5, 6)
    with pytest.raises(ValueError, match="empty"):
        _selection((0, 0, 0, 3), 5, 6)
    with pytest.raises(ValueError, match="empty"):
        _selection(torch.zeros(0, dtype=torch.int64), 5, 6)
    with pytest.raises(ValueError, match="outside the 5 x 6"):
        _selection(torch.tensor([0, 30]), 5, 6)
    with pytest.raises(ValueError, match="outside the 5 x 6"):
        _selection(torch.tensor([-1]), 5, 6)
    with pytest.raises(AssertionError, match="int64"):
        _selection(torch.tensor([0, 1], dtype=torch.int32), 5, 6)
    with pytest.raises(AssertionError, match=r"\[n\]"):
        _selection(torch.zeros(2, 2, dtype=torch.int64), 5, 6)
    with pytest.raises(AssertionError, match="window is"):
        _selection((0, 0, 1), 5, 6)
