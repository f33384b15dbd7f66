"""Host only: the numpy restatement of include/sta_tsdf.h (tests/tsdf_cases.py) against a naive scalar second statement - one pixel, one
lattice point and one tetrahedron at a time, written from the header alone -, the generated case table against the library's, the
invariants of the mesh of an analytic sphere, the host-side refusals and the PLY files."""
import inspect
import math
import os

import numpy as np
import pytest

import tsdf_cases as TC


# ------------------------------------------------------------------------------------------ the naive statement
def _f(x):
    return float(np.float64(x))


def naive_observed(v, q, iy, ix, depth_max):
    ob, D = float(v["obs"][q, iy, ix]), _f(v["depths"][q, iy, ix]) * _f(v["scales"][q])
    return (ob > 0) and math.isfinite(D) and 0 < D <= depth_max, D


def naive_blocks(v, vs, trunc, origin, depth_max):
    o = [0.0, 0.0, 0.0] if origin is None else [float(x) for x in origin]
    V, H, W = v["depths"].shape
    keys, n_obs, n_drop = set(), 0, 0
    for q in range(V):
        fx, fy, cx, cy = (float(x) for x in v["K"][q])
        T = [float(x) for x in v["c2w"][q]]
        for iy in range(H):
            for ix in range(W):
                ok, D = naive_observed(v, q, iy, ix, depth_max)
                if not ok:
                    continue
                n_obs += 1
                l = [(ix - cx) / fx * D, (iy - cy) / fy * D, D]
                P = [((T[4 * r] * l[0] + T[4 * r + 1] * l[1]) + T[4 * r + 2] * l[2]) + T[4 * r + 3] for r in range(3)]
                idx, bad = [], False
                for a in range(3):
                    pair = []
                    for c in (P[a] - trunc, P[a] + trunc):
                        f = (c - o[a]) / vs
                        if not math.isfinite(f) or not (-8388608.0 <= math.floor(f) < 8388608.0):
                            bad = True
                        else:
                            pair.append(math.floor(f) >> 3)
                    idx.append(pair)
                if bad:
                    n_drop += 1
                    continue
                for bx in idx[0]:
                    for by in idx[1]:
                        for bz in idx[2]:
                            keys.add(((bz + TC.BIAS) << 42) | ((by + TC.BIAS) << 21) | (bx + TC.BIAS))
    return np.array(sorted(keys), dtype=np.uint64), n_obs, n_drop


def naive_integrate(keys, tsdf, weight, rgb, v, v0, v1, vs, trunc, origin, depth_max, max_weight):
    o = [0.0, 0.0, 0.0] if origin is None else [float(x) for x in origin]
    tsdf, weight, rgb = tsdf.copy(), weight.copy(), rgb.copy()
    V, H, W = v["depths"].shape
    for r, key in enumerate(int(k) for k in keys):
        b = [(key & TC.FIELD) - TC.BIAS, ((key >> 21) & TC.FIELD) - TC.BIAS, (key >> 42) - TC.BIAS]
        for l in range(512):
            i = [8 * b[0] + (l & 7), 8 * b[1] + ((l >> 3) & 7), 8 * b[2] + (l >> 6)]
            x, y, z = (o[a] + float(i[a]) * vs for a in range(3))
            for q in range(v0, v1):
                T = [float(t) for t in v["w2c"][q]]
                fx, fy, cx, cy = (float(t) for t in v["K"][q])
                pcx, pcy, pcz = (((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3] for a in range(3))
                if not pcz > 0:
                    continue
                px, py = math.floor(fx * (pcx / pcz) + cx + 0.5), math.floor(fy * (pcy / pcz) + cy + 0.5)
                if not (0 <= px <= W - 1 and 0 <= py <= H - 1):
                    continue
                ok, D = naive_observed(v, q, py, px, depth_max)
                if not ok:
                    continue
                sdf = D - pcz
                if sdf < -trunc:
                    continue
                d, w, Wo = min(sdf / trunc, 1.0), _f(v["obs"][q, py, px]), _f(weight[r, l])
                tsdf[r, l] = np.float32((Wo * _f(tsdf[r, l]) + w * d) / (Wo + w))
                for ch in range(3):
                    c = (_f(v["imgs"][q, ch, py, px]) + 1.0) * 0.5
                    rgb[r, l, ch] = np.float32((Wo * _f(rgb[r, l, ch]) + w * c) / (Wo + w))
                weight[r, l] = np.float32(min(Wo + w, max_weight))
    return tsdf, weight, rgb


def naive_table():
    """the header's rule once more, with tuples"""
    T = {}
    for t, p in enumerate(TC.PERMS):
        e = [tuple(int(a == k) for a in range(3)) for k in range(3)]
        add = lambda u, w: tuple(a + b for a, b in zip(u, w))                  # noqa: E731
        cv = [(0, 0, 0), e[p[0]], add(e[p[0]], e[p[1]]), (1, 1, 1)]
        for m in range(16):
            ins, outs = [k for k in range(4) if m >> k & 1], [k for k in range(4) if not m >> k & 1]
            if not ins or not outs:
                T[t, m] = []
                continue
            if len(ins) == 1:
                tris = [[(ins[0], outs[0]), (ins[0], outs[1]), (ins[0], outs[2])]]
            elif len(ins) == 3:
                tris = [[(ins[0], outs[0]), (ins[1], outs[0]), (ins[2], outs[0])]]
            else:
                tris = [[(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1])], [(ins[0], outs[0]), (ins[1], outs[1]), (ins[1], outs[0])]]
            direction = [len(ins) * sum(cv[k][a] for k in outs) - len(outs) * sum(cv[k][a] for k in ins) for a in range(3)]
            res = []
            for tri in tris:
                P = [add(cv[i], cv[j]) for i, j in tri]
                u, w = [P[1][a] - P[0][a] for a in range(3)], [P[2][a] - P[0][a] for a in range(3)]
                n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
                s = sum(n[a] * direction[a] for a in range(3))
                assert s != 0
                res.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
            T[t, m] = (res, cv)
    return T


def naive_mesh(keys, tsdf, weight, rgb, vs, origin, min_weight):
    """one tetrahedron at a time; vertices found by walking the triangles, then put in the header's order"""
    o = [0.0, 0.0, 0.0] if origin is None else [float(x) for x in origin]
    table = naive_table()
    rank = {int(k): r for r, k in enumerate(keys)}

    def point(i):
        """-> (rank, local index) of the lattice point i, or None"""
        b = [c >> 3 for c in i]
        if any(not -TC.BIAS <= c < TC.BIAS for c in b):
            return None
        r = rank.get(((b[2] + TC.BIAS) << 42) | ((b[1] + TC.BIAS) << 21) | (b[0] + TC.BIAS))
        return None if r is None else (r, ((i[2] & 7) * 8 + (i[1] & 7)) * 8 + (i[0] & 7))

    def state(i):
        p = point(i)
        if p is None or not _f(weight[p]) >= min_weight:
            return 0
        return 2 if tsdf[p] < 0 else 1
    tris, used = [], {}
    for r, key in enumerate(int(k) for k in keys):
        b = [(key & TC.FIELD) - TC.BIAS, ((key >> 21) & TC.FIELD) - TC.BIAS, (key >> 42) - TC.BIAS]
        for l in range(512):
            c = (8 * b[0] + (l & 7), 8 * b[1] + ((l >> 3) & 7), 8 * b[2] + (l >> 6))
            if state(c) == 0:
                continue
            for t in range(6):
                cv = table[t, 1][1]
                corners = [tuple(c[a] + cv[k][a] for a in range(3)) for k in range(4)]
                st = [state(x) for x in corners]
                if 0 in st:
                    continue
                m = sum((s == 2) << k for k, s in enumerate(st))
                if m in (0, 15):
                    continue
                for tri in table[t, m][0]:
                    ids = []
                    for i, j in tri:
                        lo, hi = min(i, j), max(i, j)
                        d = tuple(corners[hi][a] - corners[lo][a] for a in range(3))
                        vk = point(corners[lo]) + (d[0] + 2 * d[1] + 4 * d[2] - 1,)
                        used[vk] = (corners[lo], corners[hi], d)
                        ids.append(vk)
                    tris.append(ids)
    order = {vk: n for n, vk in enumerate(sorted(used))}
    verts, cols = np.zeros((len(order), 3), np.float32), np.zeros((len(order), 3), np.float32)
    for vk, n in order.items():
        a, bb, d = used[vk]
        pa, pb = point(a), point(bb)
        da, db = _f(tsdf[pa]), _f(tsdf[pb])
        with np.errstate(all="ignore"):
            t = float(np.float64(da) / np.float64(da - db))
        verts[n] = [np.float32(o[k] + (float(a[k]) + (t if d[k] else 0.0)) * vs) for k in range(3)]
        if rgb is not None:
            cols[n] = [np.float32(_f(rgb[pa][ch]) + t * (_f(rgb[pb][ch]) - _f(rgb[pa][ch]))) for ch in range(3)]
    return verts, cols if rgb is not None else None, np.array([[order[x] for x in tri] for tri in tris], dtype=np.int32).reshape(-1, 3)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ tests
def test_the_table_is_the_librarys_and_the_naive_one():
    from vista_slam_amd import build, tsdf
    build.build_lib()
    T = TC.make_table()
    assert T.shape == (6, 16, TC.TABLE_ROW) and T.dtype == np.int8
    assert np.array_equal(tsdf.case_table(), T)
    naive = naive_table()
    for t in range(6):
        for m in range(16):
            tris = naive[t, m][0] if naive[t, m] else []
            assert T[t, m, 0] == len(tris)
            assert T[t, m, 1:1 + 3 * len(tris)].tolist() == [4 * i + j for tri in tris for i, j in tri]
            assert (T[t, m, 1 + 3 * len(tris):] == -1).all()
    assert [T[t, m, 0] for t in range(1) for m in range(16)] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def test_blocks_equal_the_naive_statement():
    for v, kw in ((TC.room_views(9, 13, 4), dict(vs=0.125, trunc=0.375, origin=None, depth_max=np.inf)),
                  (TC.room_views(9, 13, 4), dict(vs=0.25, trunc=1.0, origin=(0.0625, 0.5, -0.25), depth_max=2.5))):
        a = TC.blocks(v, kw["vs"], kw["trunc"], kw["origin"], kw["depth_max"])
        b = naive_blocks(v, kw["vs"], kw["trunc"], kw["origin"], kw["depth_max"])
        assert _same(a[0], b[0]) and a[1:] == b[1:] and a[1] > 0 and len(a[0]) > 8
    d = np.array([[np.nan, np.inf, 0.0, -1.0, 3.5, 1e30, 2.25]], np.float32)
    v = TC.flat_views(d, K=(4.0, 8.0, 3.0, 0.0))
    a, b = TC.blocks(v, 0.25, 0.75), naive_blocks(v, 0.25, 0.75, None, np.inf)
    assert _same(a[0], b[0]) and a[1:] == b[1:] == (3, 1)


def test_integrate_equals_the_naive_statement():
    v = TC.room_views(9, 13, 4)
    keys = TC.blocks(v, 0.25, 0.75)[0][::3][:12]                 # a dozen blocks: the naive statement is slow
    t0, w0, c0 = TC.cleared(len(keys))
    st = {}
    a = TC.integrate(keys, t0, w0, c0, v, 0, 4, 0.25, 0.75, None, 3.0, 0.5, stats=st)
    b = naive_integrate(keys, t0, w0, c0, v, 0, 4, 0.25, 0.75, None, 3.0, 0.5)
    assert all(_same(x, y) for x, y in zip(a, b)) and st["fused"] > 100 and st["clamped"] > 0 and st["unobserved"] > 0
    # a flat wall at depth 1 seen from the origin on dyadic lattices: every tie and every boundary of the header is hit exactly
    box = TC.full_keys((-1, -1, -1), (2, 2, 2))
    d = np.full((4, 4), 1.0, np.float32)
    d[3, 3] = np.nan
    fv = TC.flat_views(d, K=(4.0, 4.0, 1.5, 1.5), repeat=2)
    st2 = {}
    a2 = TC.integrate(box, *TC.cleared(27), fv, 0, 2, 0.25, 0.75, stats=st2)
    b2 = naive_integrate(box, *TC.cleared(27), fv, 0, 2, 0.25, 0.75, None, np.inf, 64.0)
    assert all(_same(x, y) for x, y in zip(a2, b2))
    for k in ("behind", "outside", "border", "tie", "unobserved", "far_behind", "at_minus_trunc", "at_plus_trunc", "fused"):
        assert st2[k] > 0, (k, st2)
    assert (t0 == 1).all() and (w0 == 0).all()                   # the inputs are left as they are
    half = TC.integrate(keys, *TC.integrate(keys, t0, w0, c0, v, 0, 2, 0.25, 0.75, None, 3.0, 0.5), v, 2, 4, 0.25, 0.75, None, 3.0, 0.5)
    assert all(_same(x, y) for x, y in zip(a, half))


def test_mesh_equals_the_naive_statement_and_reaches_every_case():
    keys, t, w, rgb = TC.random_volume(3, lo=(0, 0, 0), hi=(2, 1, 1))
    a = TC.mesh(keys, t, w, rgb, 0.125, (1.0, 2.0, -3.0), 1.0)
    b = naive_mesh(keys, t, w, rgb, 0.125, (1.0, 2.0, -3.0), 1.0)
    assert all(_same(x, y) for x, y in zip(a, b)) and len(a[2]) > 500
    keys, t, w = TC.sphere_volume(drop=(0, 1, 0), lo=(0, 0, 0), hi=(1, 2, 1))
    assert all(_same(x, y) for x, y in zip(TC.mesh(keys, t, w)[::2], naive_mesh(keys, t, w, None, 1.0, None, 1.0)[::2]))
    # all 6 x 14 (tetrahedron, case) pairs occur in the random volume
    keys, t, w, rgb = TC.random_volume(3)
    _lo, state, _val, _sk = TC._dense(keys, t, w, 1.0)
    seen = set()
    Z, Y, X = state.shape
    for tt in range(6):
        cv = TC.tet_corners(tt)
        S = [state[cv[k, 2]:Z - 1 + cv[k, 2], cv[k, 1]:Y - 1 + cv[k, 1], cv[k, 0]:X - 1 + cv[k, 0]] for k in range(4)]
        known = (S[0] > 0) & (S[1] > 0) & (S[2] > 0) & (S[3] > 0)
        case = sum((S[k] == 2).astype(int) << k for k in range(4))
        seen |= {(tt, int(m)) for m in np.unique(case[known])}
    assert {(tt, m) for tt in range(6) for m in range(1, 15)} <= seen


def test_the_sphere_is_a_closed_manifold():
    keys, t, w = TC.sphere_volume()
    assert len(keys) == 27
    verts, _c, tris = TC.mesh(keys, t, w)
    rep = TC.mesh_report(verts, tris)
    full = 4.0 / 3.0 * math.pi * 4.4 ** 3
    print(f"[tsdf cpu] sphere r = 4.4: {rep}, analytic volume {full:.1f}, deficit {1 - rep['volume'] / full:.4f}")
    assert (rep["V"], rep["F"]) == (1064, 2124)
    assert rep["directed_once"] and rep["closed"] and rep["euler"] == 2 and rep["unreferenced"] == 0
    assert 0 < rep["volume"] <= full and 1 - rep["volume"] / full <= TC.SPHERE_MAX_VOLUME_DEFICIT
    r = np.sqrt(((verts.astype(np.float64) - np.array([3.5, 4.25, 2.75])) ** 2).sum(1))
    assert r.max() <= 4.4 + 1e-5 and r.min() >= 4.4 - 0.085 * 1.5       # on chords of the sphere: never outside, a sag inside
    # the lattice is translation invariant: the same sphere moved by one block is the same mesh moved
    k2, t2, w2 = TC.sphere_volume(centre=(11.5, 4.25, 2.75), lo=(0, -1, -1), hi=(3, 2, 2))
    v2, _c, tr2 = TC.mesh(k2, t2, w2)
    # (coordinates below 16 are rounded to float32 once on either side: half an ulp of 2^-20 each)
    assert np.array_equal(tr2, tris) and np.abs(v2.astype(np.float64) - (verts.astype(np.float64) + [8, 0, 0])).max() <= 2.0 ** -20


def test_the_fused_room_lies_on_the_analytic_surface():
    v, (keys, t, w, c, verts, cols, tris) = TC.room_expected()
    d = TC.room_distance(verts)
    rep = TC.mesh_report(verts, tris)
    print(f"[tsdf cpu] room 24x32, 5 views, voxel 1/8: {len(keys)} blocks, {len(verts)} vertices, {len(tris)} triangles, "
          f"distance max {d.max():.4f} mean {d.mean():.4f}")
    assert len(tris) > 10000 and rep["directed_once"] and rep["unreferenced"] == 0
    assert d.max() <= TC.ROOM_MAX_VERTEX_DISTANCE
    assert cols.min() >= 0 and cols.max() <= 1


def test_views_restate_the_python_layer():
    from vista_slam_amd import tsdf
    s = TC.room_scene(9, 13, 4)
    e = TC.views_of(s["depths"], s["scales"], s["intrinsics"], s["poses"], s["confs"], s["imgs"], s["conf_thres"])
    g = tsdf.views(s["depths"], s["scales"], s["intrinsics"], s["poses"], s["confs"], s["imgs"], conf_thres=s["conf_thres"], device="cpu")
    for k in ("depths", "scales", "K", "c2w", "w2c", "obs", "imgs"):
        assert _same(getattr(g, k).numpy(), e[k]), k
    counts = (np.arange(4 * 9 * 13).reshape(4, 9, 13) % 3).astype(np.int32)
    e = TC.views_of(s["depths"], s["scales"], s["intrinsics"], s["poses"], s["confs"], None, 1.0, counts, 2)
    g = tsdf.views(s["depths"], s["scales"], s["intrinsics"], s["poses"], s["confs"], conf_thres=1.0, counts=counts, min_views=2, device="cpu")
    assert _same(g.obs.numpy(), e["obs"]) and g.imgs is None and 0 < e["obs"].sum() < (s["confs"] > 1.0).sum()
    K = s["intrinsics"].copy()
    K[1, 0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        tsdf.views(s["depths"], s["scales"], K, s["poses"], s["confs"], conf_thres=1.0, device="cpu")
    K = s["intrinsics"].copy()
    K[2, 2, 2] = 2.0
    with pytest.raises(ValueError, match="last row"):
        tsdf.views(s["depths"], s["scales"], K, s["poses"], s["confs"], conf_thres=1.0, device="cpu")


def test_plan_and_its_refusals():
    from vista_slam_amd import tsdf
    p = tsdf.plan(4, 9, 13, 0.125, None, 100, 1000, 2000)
    assert p.key_slots == 8 * 4 * 9 * 13 and p.keys_bytes == 800 and p.tsdf_bytes == 100 * 2048 and p.rgb_bytes == 100 * 6144
    assert p.verts_bytes == 12000 and p.tris_bytes == 24000 and p.blocks_work_bytes >= 24 * p.key_slots and p.mesh_work_bytes >= 100 * 512 * 3
    for kw, word in ((dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=float("nan")), "voxel_size"), (dict(trunc=-1.0), "trunc"),
                     (dict(trunc=float("inf")), "trunc"), (dict(trunc=0.51), "more than 4 voxels"), (dict(max_blocks=1 << 24), "16777216"),
                     (dict(max_blocks=0), "max_blocks"), (dict(V=1 << 14, H=1 << 7, W=1 << 7), "below 2.28"), (dict(H=0), "H and W"), (dict(W=0), "H and W"),
                     (dict(max_vertices=1 << 31), "max_vertices")):
        a = dict(V=4, H=9, W=13, voxel_size=0.125, trunc=None, max_blocks=100, max_vertices=0, max_triangles=0)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            tsdf.plan(**a)
    tsdf.plan(1, 1, 1, 0.125, 0.5)                                        # trunc == 4 voxels is allowed
    tsdf.plan((1 << 28) - 1, 1, 1, 0.125)
    with pytest.raises(ValueError):
        tsdf.TSDFVolume("cpu", voxel_size=-1.0)
    with pytest.raises(ValueError, match="origin"):
        tsdf.TSDFVolume("cpu", voxel_size=0.1, origin=(0, float("nan"), 0))
    vol = tsdf.TSDFVolume("cpu", voxel_size=0.1)
    assert vol.trunc == 3.0 * 0.1 and vol.max_weight == 64.0 and vol.depth_max == float("inf") and vol.n_blocks == 0


def test_mesh_ply_round_trip(tmp_path):
    import torch
    from vista_slam_amd import formats, tsdf
    keys, t, w, rgb = TC.random_volume(7, lo=(0, 0, 0), hi=(1, 1, 1))
    verts, cols, tris = TC.mesh(keys, t, w, rgb, 0.5)
    path = str(tmp_path / "m.ply")
    tsdf.write_mesh_ply(path, tsdf.Mesh(torch.from_numpy(verts), torch.from_numpy(cols), torch.from_numpy(tris)))
    rec, got = tsdf.read_mesh_ply(path)
    assert rec.dtype == formats.PLY_RECORD and np.array_equal(got, tris)
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), verts.astype(np.float64))
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), np.rint(np.clip(cols, 0, 1) * np.float32(255)).astype(np.uint8))
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode()
    assert "format binary_little_endian 1.0" in head and f"element vertex {len(verts)}" in head and f"element face {len(tris)}" in head
    assert "property list uchar int vertex_indices" in head
    assert os.path.getsize(path) == len(head) + len("end_header\n") + 27 * len(verts) + 13 * len(tris)
    assert np.array_equal(formats.read_ply(path), rec)                  # the vertex block is a pointcloud.ply's
    tsdf.write_mesh_ply(path, tsdf.Mesh(torch.from_numpy(verts), None, torch.from_numpy(tris)))
    assert (tsdf.read_mesh_ply(path)[0]["red"] == 255).all()


def test_save_data_all_keeps_its_signature():
    from vista_slam_amd import formats
    p = inspect.signature(formats.save_data_all).parameters
    assert p["mesh_voxel_size"].default is None and list(p)[-1] == "mesh_voxel_size"



@pytest.mark.parametrize("t", range(6))
def test_table_normals_point_into_free_space(t):
    """every triangle of the library's table, placed on the edge midpoints of its tetrahedron, has its normal on the side of the outside
    corners and never degenerates"""
    from vista_slam_amd import tsdf
    T, cv = tsdf.case_table(), TC.tet_corners(t).astype(np.float64)
    for m in range(1, 15):
        ins, outs = [k for k in range(4) if m >> k & 1], [k for k in range(4) if not m >> k & 1]
        for r in range(T[t, m, 0]):
            codes = T[t, m, 1 + 3 * r:4 + 3 * r]
            assert all((c >> 2) in ins and (c & 3) in outs for c in codes)
            P = [(cv[c >> 2] + cv[c & 3]) * 0.5 for c in codes]
            n = np.cross(P[1] - P[0], P[2] - P[0])
            assert np.dot(n, cv[outs].mean(0) - cv[ins].mean(0)) > 0
