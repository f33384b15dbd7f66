"""Host only: the numpy restatement of include/sta_mesh.h (tests/mesh_cases.py) against a naive scalar per-pixel statement of the same
rule, and the invariants a watertight rasteriser owes a closed mesh - on tsdf_cases.sphere_volume()'s mesh (1064 vertices, 2124
triangles, closed): seen from outside every pixel is covered by as many front faces as back faces, seen from inside every pixel by
exactly one face.  A gap or a pixel drawn twice along a shared edge, a shared vertex, a cut edge or the diagonal of a cut quad breaks
them."""
import numpy as np
import pytest

import mesh_cases as MC
import render_cases as RC
import tsdf_cases as TC


def test_the_sphere_mesh_is_what_the_invariants_assume():
    v, t, _ = MC.sphere_mesh()
    rep = TC.mesh_report(v, t)
    assert (rep["V"], rep["F"], rep["closed"], rep["euler"]) == (1064, 2124, True, 2)
    assert rep["volume"] > 0                                 # normals outwards


@pytest.mark.parametrize("name", ["shared_edge", "sliver", "near_plane", "off_canvas", "too_large", "coincident", "far"])
def test_restatement_equals_the_naive_statement(name):
    """ids only (the naive statement has no colours): the id ops of the case, each on its own canvas"""
    case = MC.CASES[name]()
    n = 0
    for kind, a in case["ops"]:
        if kind != "triangles" or a.get("kind", MC.ID) != MC.ID:
            continue
        s = case["ssaa"]
        keys = RC.new_keys(case["H"], case["W"], s)
        MC.triangles(keys, s, **a)
        naive = MC.naive_triangles(keys.shape[0], keys.shape[1], s, a["verts"], a["tris"], a["T"], a["K"], a.get("near", 1e-3), a.get("far", 1e4),
                                   a.get("cull", 0), a.get("id_base", 0))
        assert np.array_equal(keys, naive), name
        n += 1
    assert n


def test_naive_statement_on_a_rotated_sphere_view():
    v, t, _ = MC.sphere_mesh()
    c = MC.outside_cam(9, 12, 7.0, MC.OBLIQUE_EYE)
    for cull in (0, 1, 2):
        keys = RC.new_keys(9, 12, 1)
        MC.triangles(keys, 1, v, t, cull=cull, **c)
        assert np.array_equal(keys, MC.naive_triangles(9, 12, 1, v, t, c["T"], c["K"], c["near"], c["far"], cull)), cull


@pytest.mark.parametrize("name", ["sphere_inside_lit_cull1", "sphere_outside_id_cull2", "too_large", "bad_index_nan", "off_canvas", "sliver", "near_plane"])
def test_the_array_prefilter_counts_what_the_scalar_rules_count(name):
    case = MC.CASES[name]()
    for kind, a in case["ops"]:
        out = []
        for pre in (True, False):
            keys = RC.new_keys(case["H"], case["W"], case["ssaa"])
            out.append((keys, MC.triangles(keys, case["ssaa"], prefilter=pre, **a)))
        assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tolist() == out[1][1].tolist(), name


def test_shared_edges_through_pixel_centres_are_drawn_once():
    case, exp = MC.expected_of("shared_edge")
    a = case["ops"][0][1]
    cov = (np.zeros((12, 13), int), np.zeros((12, 13), int))
    MC.triangles(RC.new_keys(12, 13, 1), 1, cover=cov, **a)
    total = cov[0] + cov[1]
    assert total.max() == 1
    assert total[2:8, 2:8].all() and total[2, 2] == 1              # the square (2..8)^2, half-open by the top-left rule: its top and left edges are in
    ids = exp["ids"]
    assert ids[2, 2] == 0 and ids[5, 5] == 0 and ids[5, 4] == 1    # the vertex on a centre and the diagonal go to the triangle for which the edge is a left edge
    assert (ids[8, 2:8] == 2).all() and (ids[3:8, 8] == 3).all()   # the square's bottom and right edges are the top / left edges of the triangles beyond
    assert ids[8, 8] == ids[2, 8] == 0xFFFFFFFF and total[8, 8] == 0        # the corners (8, 8) and (8, 2) are on a top or left edge of none of the four


@pytest.mark.parametrize("name", list(MC.OUTSIDE))
def test_outside_every_pixel_has_as_many_front_as_back_faces(name):
    """At EVERY pixel the number of covering front faces equals the number of back faces, from both eyes and on both grids.  That both are
    0 or 1 on the 1/256 grid is asserted from the axial eye only: the marching-tetrahedra mesh of the sphere is not convex (its facets fold
    slightly along the lattice), so from the oblique eye a ray near the silhouette can enter and leave the surface twice and a pixel there
    has two front and two back faces - the counts still agree, and 2 is the most either eye reaches."""
    H, W, f, sub = MC.OUTSIDE[name]
    v, t, _ = MC.sphere_mesh()
    for eye, at_most in ((MC.OUTSIDE_EYE, 1), (MC.OBLIQUE_EYE, 2)):
        for grid in sorted({sub, 256}):
            cov = (np.zeros((H, W), int), np.zeros((H, W), int))
            cnt = MC.triangles(RC.new_keys(H, W, 1), 1, v, t, cover=cov, sub=grid, **MC.outside_cam(H, W, f, eye))
            assert cnt[MC.SEEN] == 2124 and cnt[MC.BAD] == cnt[MC.BEHIND] == cnt[MC.CLIPPED] == cnt[MC.TOO_LARGE] == 0
            assert np.array_equal(cov[0], cov[1]), (name, grid)
            assert cov[0].any() and cov[0].max() <= at_most
            if grid == 256 and at_most == 1:
                assert set(np.unique(cov[0])) == {0, 1} and set(np.unique(cov[1])) == {0, 1}


@pytest.mark.parametrize("near", MC.INSIDE_NEARS)
def test_inside_every_pixel_is_covered_exactly_once(near):
    """The issue names no eye direction, so the camera is mesh_cases.inside_cam's; its numbers are pinned as literals in
    mesh_cases.INSIDE_EXPECTED: the eight counters per `near` (122 / 119 / 121 triangles cut, 650 / 548 / 537 behind, 924 / 1023 / 1035
    off the canvas) and the largest |snapped coordinate| among the cut pieces, which grows as `near` shrinks (2^15.0, 2^18.4, 2^24.1) and
    stays below the 2^28 drop."""
    v, t, _ = MC.sphere_mesh()
    H, W = 24, 32
    assert abs(np.linalg.norm(MC.INSIDE_EYE - MC.SPHERE_CENTRE) - 3.0) < 1e-12
    cov = (np.zeros((H, W), int), np.zeros((H, W), int))
    keys = RC.new_keys(H, W, 1)
    st = {}
    cnt = MC.triangles(keys, 1, v, t, cover=cov, stats=st, **MC.inside_cam(near))
    assert (cov[1] == 1).sum() == 768 == H * W, "every one of the 768 pixels by exactly one back face"
    assert (cov[0] == 0).all(), "and by no front face"
    assert (keys != RC.EMPTY).all()
    print(f"near {near}: counters {cnt.tolist()}, largest |snapped coordinate| of a cut piece {st['max_cut_snap']}")
    want_cnt, want_snap = MC.INSIDE_EXPECTED[near]
    assert cnt.tolist() == want_cnt
    assert st["max_cut_snap"] == want_snap and want_snap < MC.MAX_SNAP
    assert MC.INSIDE_EXPECTED == {0.5: ([2124, 0, 650, 122, 0, 0, 0, 924], 33690), 0.05: ([2124, 0, 548, 119, 0, 0, 0, 1023], 352143),
                                  0.001: ([2124, 0, 537, 121, 0, 0, 0, 1035], 17675909)}


def test_seen_from_outside_the_sphere_is_all_front_facing():
    """the facing rule of the header: normals into free space are front faces from free space"""
    v, t, _ = MC.sphere_mesh()
    H, W = 24, 32
    c = MC.outside_cam(H, W, 20.0)
    front, back, both = [RC.new_keys(H, W, 1) for _ in range(3)]
    cf = MC.triangles(front, 1, v, t, cull=MC.CULL_BACK, **c)
    cb = MC.triangles(back, 1, v, t, cull=MC.CULL_FRONT, **c)
    MC.triangles(both, 1, v, t, **c)
    assert np.array_equal(front, both) and cf[MC.CULLED] > 0 and cb[MC.CULLED] > 0
    assert ((back == RC.EMPTY) == (both == RC.EMPTY)).all() and (back[both != RC.EMPTY] > both[both != RC.EMPTY]).all()


def test_depth_of_a_slanted_plane_is_exact_at_the_vertices_and_monotone():
    case, exp = MC.expected_of("far")
    d = exp["depth"]
    assert d[0, 0] == 1.0 and np.isinf(d[11, 13])
    seen = np.isfinite(d)
    assert seen.any() and d[seen].max() <= 2.5 and (np.diff(d[0][np.isfinite(d[0])]) > 0).all()


def test_vertex_normals_of_the_restatement():
    v, t, _ = MC.sphere_mesh()
    err = MC.sphere_normal_error()
    print(f"largest angle to the analytic normal: {err:.4f} rad (bound {MC.SPHERE_NORMAL_BOUND:.4f})")
    assert err <= MC.SPHERE_NORMAL_BOUND
    assert MC.SPHERE_NORMAL_BOUND == MC.SPHERE_NORMAL_ERROR * MC.SPHERE_NORMAL_MARGIN and MC.SPHERE_NORMAL_MARGIN == 2.0
    n = MC.vertex_normals(v, t)
    assert np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=1e-6)
    ov, ot = MC.odd_mesh()
    on = MC.vertex_normals(ov, ot)
    assert (on[4] == 0).all() and (on[5] == 0).all() and (on[6] == 0).all()           # isolated; only in a zero-area triangle
    assert np.allclose(on[0].astype(np.float64), np.array([1.0, 0.0, 0.0]) * 0 + on[0]) and np.linalg.norm(on[0]) > 0.99
    fv, ft = MC.fan_mesh()
    assert len(ft) == 40 and np.linalg.norm(MC.vertex_normals(fv, ft)[0]) > 0.99


def test_plan_restated():
    assert MC.plan(0, 0) == (256, 1024)
    assert MC.plan(1, 3) == (512, 3072)
    assert MC.plan(2 ** 31 - 1, 5)[1] == -1
    for args, text in (((-1, 3), r"nt must be in \[0, 2\^31\) \(got -1\)"), ((1, 2 ** 31), r"nv must be in \[0, 2\^31\) \(got 2147483648\)")):
        with pytest.raises(ValueError, match=text):
            MC.plan(*args)


def test_write_mesh_ply_with_normals(tmp_path):
    """host tensors suffice: the file with normals has Open3D's property order, and without the keyword it is byte for byte the old file"""
    import torch
    from vista_slam_amd import tsdf
    v, t, col = MC.sphere_mesh()
    mesh = tsdf.Mesh(torch.from_numpy(v.copy()), torch.from_numpy(col.copy()), torch.from_numpy(t.copy()))
    n = MC.vertex_normals(v, t)
    a, b, c = [str(tmp_path / f) for f in ("plain.ply", "normals.ply", "none.ply")]
    tsdf.write_mesh_ply(a, mesh)
    tsdf.write_mesh_ply(b, mesh, normals=torch.from_numpy(n))
    tsdf.write_mesh_ply(c, mesh, normals=None)
    assert open(a, "rb").read() == open(c, "rb").read()
    head = open(b, "rb").read(600).split(b"end_header\n")[0].decode().splitlines()
    props = [ln.split()[-1] for ln in head if ln.startswith("property") and "list" not in ln]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    rec, tris = tsdf.read_mesh_ply(b)
    assert np.array_equal(tris, t) and np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1), n.astype(np.float64))
    rec0, tris0 = tsdf.read_mesh_ply(a)
    assert rec0.dtype.names == ("x", "y", "z", "red", "green", "blue") and np.array_equal(rec0["x"], rec["x"]) and np.array_equal(rec0["red"], rec["red"])


def test_cull_mesh_reindexes_in_ascending_order():
    import torch
    from vista_slam_amd import tsdf
    v = torch.arange(18, dtype=torch.float32).reshape(6, 3)
    t = torch.tensor([[0, 1, 2], [3, 4, 5], [5, 1, 3]], dtype=torch.int32)
    m = tsdf.cull_mesh(tsdf.Mesh(v, v / 18, t), [False, False, True])
    assert m.vertices.tolist() == v[[1, 3, 5]].tolist() and m.triangles.tolist() == [[2, 0, 1]] and m.colors.tolist() == (v / 18)[[1, 3, 5]].tolist()
    m = tsdf.cull_mesh(tsdf.Mesh(v, None, t), torch.tensor([True, True, True]))
    assert m.vertices.shape == (6, 3) and m.triangles.tolist() == t.tolist() and m.colors is None
