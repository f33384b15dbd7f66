"""GPU: libsta_tsdf.so (csrc/tsdf.h) against the numpy restatement of its contract (tests/tsdf_cases.py), through the C ABI into
pattern-filled buffers with guard regions behind every one, and vista_slam_amd.tsdf on top of it.  Every comparison is array_equal.  The
scenes are the smallest that cross wave tails and block faces; the restatement's branch counters say which branches a case reaches."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import tsdf_cases as TC

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256              # bytes behind every buffer
VS, TRUNC = 0.25, 0.75


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(nbytes, content=None):
    import torch
    buf = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    if content is not None:
        buf[:nbytes] = _up(np.ascontiguousarray(content).view(np.uint8).reshape(-1))
    return buf


def _tail_untouched(buf, nbytes, what):
    raw = buf[nbytes:].cpu().numpy()
    assert (raw == FILL).all(), f"{what}: bytes past its {nbytes} were written"


def _take(buf, nbytes, dtype, shape):
    return buf[:nbytes].cpu().numpy().view(dtype).reshape(shape)


def _lib():
    from vista_slam_amd import _lib as L
    return L, L.load_tsdf()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _org(origin):
    return None if origin is None else (C.c_double * 3)(*[float(x) for x in origin])


def _plan(lib, V, H, W, vs, trunc, mb, mv=0, mt=0):
    sizes = (C.c_int64 * TC.PLAN_SIZES)()
    assert lib.sta_tsdf_plan(V, H, W, vs, trunc, mb, mv, mt, sizes) == 0, lib.sta_tsdf_last_error()
    return list(sizes)


def _dev_views(v):
    return {k: (_up(a) if a is not None else None) for k, a in v.items()}


def raw_blocks(v, vs=VS, trunc=TRUNC, origin=None, depth_max=np.inf, max_blocks=4096):
    """-> (rc, keys_out as written [max_blocks] uint64, counts)"""
    import torch
    L, lib = _lib()
    V, H, W = v["depths"].shape
    sizes = _plan(lib, V, H, W, vs, trunc, max_blocks)
    assert sizes[7] == 8 * V * H * W and sizes[1] == 8 * max_blocks
    d = _dev_views(v)
    keys, work = _guarded(sizes[1]), _guarded(sizes[0])
    cnt = (C.c_int64 * 3)(-1, -1, -1)
    rc = lib.sta_tsdf_blocks(d["depths"].data_ptr(), d["scales"].data_ptr(), d["K"].data_ptr(), d["c2w"].data_ptr(), d["obs"].data_ptr(), V, H, W, vs, trunc,
                             _org(origin), depth_max, keys.data_ptr(), max_blocks, work.data_ptr(), sizes[0], cnt, _stream())
    torch.cuda.synchronize()
    _tail_untouched(keys, sizes[1], "keys_out")
    _tail_untouched(work, sizes[0], "work")
    return rc, _take(keys, sizes[1], np.uint64, (max_blocks,)), list(cnt)


def raw_integrate(keys, t, w, rgb, v, v0, v1, vs=VS, trunc=TRUNC, origin=None, depth_max=np.inf, max_weight=64.0, imgs=True):
    import torch
    L, lib = _lib()
    V, H, W = v["depths"].shape
    nb = len(keys)
    d = _dev_views(v)
    kb, tb, wb = _guarded(nb * 8, keys), _guarded(nb * 2048, t), _guarded(nb * 2048, w)
    cb = _guarded(nb * 6144, rgb) if rgb is not None else None
    im = d["imgs"] if imgs else None
    L.check_tsdf(lib.sta_tsdf_integrate(kb.data_ptr(), nb, tb.data_ptr(), wb.data_ptr(), cb.data_ptr() if cb is not None else None, d["depths"].data_ptr(),
                                        d["scales"].data_ptr(), d["K"].data_ptr(), d["w2c"].data_ptr(), d["obs"].data_ptr(),
                                        im.data_ptr() if im is not None else None, V, H, W, v0, v1, vs, trunc, _org(origin), depth_max, max_weight, _stream()))
    torch.cuda.synchronize()
    for buf, n, what in ((kb, nb * 8, "keys"), (tb, nb * 2048, "tsdf"), (wb, nb * 2048, "weight")) + (((cb, nb * 6144, "rgb"),) if cb is not None else ()):
        _tail_untouched(buf, n, what)
    assert np.array_equal(_take(kb, nb * 8, np.uint64, (nb,)), keys)
    return (_take(tb, nb * 2048, np.float32, (nb, 512)), _take(wb, nb * 2048, np.float32, (nb, 512)),
            _take(cb, nb * 6144, np.float32, (nb, 512, 3)) if cb is not None else None)


def raw_clear(nb, colour=True):
    import torch
    L, lib = _lib()
    tb, wb, cb = _guarded(nb * 2048), _guarded(nb * 2048), _guarded(nb * 6144) if colour else None
    L.check_tsdf(lib.sta_tsdf_clear(tb.data_ptr(), wb.data_ptr(), cb.data_ptr() if colour else None, nb, _stream()))
    torch.cuda.synchronize()
    for buf, n in ((tb, nb * 2048), (wb, nb * 2048)) + (((cb, nb * 6144),) if colour else ()):
        _tail_untouched(buf, n, "clear")
    return (_take(tb, nb * 2048, np.float32, (nb, 512)), _take(wb, nb * 2048, np.float32, (nb, 512)),
            _take(cb, nb * 6144, np.float32, (nb, 512, 3)) if colour else None)


def raw_mesh(keys, t, w, rgb=None, vs=1.0, origin=None, min_weight=1.0, max_v=None, max_t=None, count_only=False):
    """-> (rc, counts, verts, cols, tris): the three buffers whole, as the call left them (max_v / max_t rows)"""
    import torch
    L, lib = _lib()
    nb = len(keys)
    exp_v, _c, exp_t = TC.mesh(keys, t, w, rgb, vs, origin, min_weight)
    max_v = len(exp_v) if max_v is None else max_v
    max_t = len(exp_t) if max_t is None else max_t
    sizes = _plan(lib, 1, 1, 1, 1.0, 1.0, max(nb, 1), max_v, max_t)
    assert sizes[5] == 12 * max_v and sizes[6] == 12 * max_t
    kb, tb, wb = _up(keys.view(np.int64)), _up(t), _up(w)
    cb = _up(rgb) if rgb is not None else None
    vb, ob, qb, work = _guarded(sizes[5]), _guarded(sizes[5]), _guarded(sizes[6]), _guarded(sizes[4])
    cnt = (C.c_int64 * 2)(-1, -1)
    rc = lib.sta_tsdf_mesh(kb.data_ptr(), nb, tb.data_ptr(), wb.data_ptr(), cb.data_ptr() if cb is not None else None, vs, _org(origin), min_weight,
                           None if count_only else vb.data_ptr(), None if count_only or rgb is None else ob.data_ptr(), None if count_only else qb.data_ptr(),
                           max_v, max_t, work.data_ptr(), sizes[4], cnt, _stream())
    torch.cuda.synchronize()
    for buf, n, what in ((vb, sizes[5], "verts_out"), (ob, sizes[5], "cols_out"), (qb, sizes[6], "tris_out"), (work, sizes[4], "work")):
        _tail_untouched(buf, n, what)
    return (rc, list(cnt), _take(vb, sizes[5], np.float32, (max_v, 3)), _take(ob, sizes[5], np.float32, (max_v, 3)), _take(qb, sizes[6], np.int32, (max_t, 3)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same(got, exp, what):
    assert got.shape == exp.shape, f"{what}: shape {got.shape} against {exp.shape}"
    bad = np.argwhere(_bits(got) != _bits(exp))
    assert not len(bad), f"{what}: {len(bad)} of {got.size} differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} against {exp[tuple(bad[0])]!r}"


# ------------------------------------------------------------------------------------------ blocks
def _mixed_views():
    """5 x 7 depths from a camera at a negative position: finite, NaN, inf, 0, negative, beyond depth_max = 3, too far for the key's
    fields; obs 0 and NaN.  D = 1.25 puts P_z + trunc = -0.5 + 1.25 + 0.75 on a voxel face and D = 1.75 on the block face z = 2."""
    d = np.full((5, 7), 1.25, np.float32)
    d[0, :] = [np.nan, np.inf, 0.0, -1.0, 3.5, 1e30, 1.75]
    d[1, :3] = [0.5, 2.75, 3.0]
    conf = np.ones((5, 7), np.float32)
    conf[2, 1], conf[2, 2] = 0.0, np.nan
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (-3.0, -1.125, -0.5)
    return TC.flat_views(d, obs=conf, K=(4.0, 8.0, 3.0, 2.0), pose=pose)


def _one_pixel():
    return TC.flat_views([[1.0]], K=(1.0, 1.0, 0.0, 0.0))


BLOCK_CASES = {
    "one_pixel": (_one_pixel, {}),
    "mixed": (_mixed_views, {"depth_max": 3.0}),
    "mixed_far": (_mixed_views, {"depth_max": np.inf}),
    "mixed_origin": (_mixed_views, {"depth_max": 3.0, "origin": (0.125, -0.25, 1.0)}),
    "room_9x13": (lambda: TC.room_views(9, 13, 4), {"vs": 0.125, "trunc": 0.375}),
    "room_24x32": (lambda: TC.room_views(24, 32, 5), {"vs": 0.125, "trunc": 0.375}),
}


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_blocks_equal_the_restatement(name):
    make, kw = BLOCK_CASES[name]
    v = make()
    vs, trunc = kw.get("vs", VS), kw.get("trunc", TRUNC)
    exp, n_obs, n_drop = TC.blocks(v, vs, trunc, kw.get("origin"), kw.get("depth_max", np.inf))
    rc, keys, cnt = raw_blocks(v, vs, trunc, kw.get("origin"), kw.get("depth_max", np.inf))
    print(f"[tsdf blocks] {name}: nb {cnt[0]}, observed {cnt[1]}, dropped {cnt[2]}")
    assert rc == 0 and cnt == [len(exp), n_obs, n_drop], (rc, cnt, len(exp), n_obs, n_drop)
    same(keys[:len(exp)], exp, "keys")
    assert (keys[len(exp):] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), "keys past nb were written"
    assert (np.diff(exp.astype(np.int64)) > 0).all()
    if name == "one_pixel":
        assert cnt[:2] == [4, 1]                     # P = (0, 0, 1), trunc 0.75: x and y reach the blocks -1 and 0, z (voxels 1 and 7) only block 0
    if name.startswith("mixed"):
        # of 35 pixels: NaN, inf, 0, -1 and the two obs (0, NaN) never count; 3.5 and 1e30 only without the depth limit, and 1e30 is dropped
        assert (n_obs, n_drop) == ((29, 1) if name == "mixed_far" else (27, 0))
        assert (TC.block_coords(exp) < 0).any()


def test_blocks_reach_a_block_face_exactly():
    """the case table above is only worth its name if a corner lies exactly on a block face"""
    v = _mixed_views()
    ok, D = TC.observed(v, 3.0)
    pz = v["c2w"][0, 11] + D[ok]
    assert ((((pz + TRUNC) / VS) % 8) == 0).any() and ((((pz + TRUNC) / VS) % 1) == 0).any()


def test_more_blocks_than_max_blocks_is_refused_and_writes_nothing_past_them():
    v = _mixed_views()
    exp, n_obs, n_drop = TC.blocks(v, VS, TRUNC, None, 3.0)
    assert len(exp) > 3
    rc, keys, cnt = raw_blocks(v, VS, TRUNC, None, 3.0, max_blocks=3)
    L, lib = _lib()
    assert rc != 0 and cnt == [len(exp), n_obs, n_drop]
    assert str(len(exp)) in lib.sta_tsdf_last_error().decode() and "max_blocks" in lib.sta_tsdf_last_error().decode()
    same(keys, exp[:3], "the first max_blocks keys")


def test_clear():
    t, w, c = raw_clear(3)
    assert (t == 1).all() and (w == 0).all() and (c == 0).all()
    t, w, c = raw_clear(2, colour=False)
    assert (t == 1).all() and (w == 0).all() and c is None


# ------------------------------------------------------------------------------------------ integrate
BOX = TC.full_keys((-1, -1, -1), (2, 2, 2))          # 27 blocks around the origin: z from -2 to 3.75 at voxel 0.25


def _flat(repeat=1, **kw):
    d = np.full((4, 4), 1.0, np.float32)
    d[3, 3] = np.nan
    return TC.flat_views(d, K=(4.0, 4.0, 1.5, 1.5), repeat=repeat, **kw)


def _narrow():
    """a 3 x 3 image under a long focal length: the frustum is a thin pyramid that leaves most of the 27 blocks out and clips others"""
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.875, 0.875, -1.0)
    return TC.flat_views(np.full((3, 3), 2.0, np.float32), K=(16.0, 16.0, 1.0, 1.0), pose=pose, repeat=2)


def _check_integrate(v, keys, v0, v1, stats=None, colour=True, imgs=True, **kw):
    t0, w0, c0 = TC.cleared(len(keys), colour)
    vv = dict(v) if imgs else {**v, "imgs": None}
    exp = TC.integrate(keys, t0, w0, c0, vv, v0, v1, kw.get("vs", VS), kw.get("trunc", TRUNC), kw.get("origin"), kw.get("depth_max", np.inf),
                       kw.get("max_weight", 64.0), stats=stats)
    got = raw_integrate(keys, t0, w0, c0, v, v0, v1, kw.get("vs", VS), kw.get("trunc", TRUNC), kw.get("origin"), kw.get("depth_max", np.inf),
                        kw.get("max_weight", 64.0), imgs=imgs)
    for g, e, what in zip(got, exp, ("tsdf", "weight", "rgb")):
        if e is not None:
            same(g, e, what)
    return got


def test_integrate_a_flat_view_reaches_every_branch():
    st = {}
    _check_integrate(_flat(), BOX, 0, 1, st)
    print(f"[tsdf integrate] flat: {st}")
    for k in ("behind", "outside", "border", "tie", "unobserved", "far_behind", "at_minus_trunc", "at_plus_trunc", "fused"):
        assert st[k] > 0, (k, st)


def test_integrate_clamps_the_weight_of_a_repeated_view():
    st = {}
    t, w, c = _check_integrate(_flat(repeat=5), BOX, 0, 5, st, max_weight=3.0)
    assert st["clamped"] > 0 and w.max() == 3.0


def test_integrate_in_two_calls_gives_the_bits_of_one():
    v, (keys, t, w, c, _v, _c, _t) = TC.room_expected(9, 13, 4)
    t0, w0, c0 = TC.cleared(len(keys))
    a = raw_integrate(keys, t0, w0, c0, v, 0, 2, 0.125, 0.375)
    b = raw_integrate(keys, a[0], a[1], a[2], v, 2, 4, 0.125, 0.375)
    one = raw_integrate(keys, t0, w0, c0, v, 0, 4, 0.125, 0.375)
    for g, h, e, what in zip(b, one, (t, w, c), ("tsdf", "weight", "rgb")):
        same(g, h, what + " [0,2)+[2,4) against [0,4)")
        same(h, e, what)
    assert (w > 0).any() and not np.array_equal(a[0], b[0])


def test_integrate_under_a_narrow_frustum_culling_changes_nothing():
    st = {}
    _check_integrate(_narrow(), BOX, 0, 2, st)
    print(f"[tsdf integrate] narrow: {st}")
    assert st["fused"] > 0 and st["outside"] > 20 * st["fused"]
    # blocks of which exactly one corner region is inside the image: some but not all of their points project into it
    v = _narrow()
    li = TC.lattice_index(BOX).astype(np.float64) * VS
    pc = li - np.array([0.875, 0.875, -1.0])
    with np.errstate(all="ignore"):
        px, py = np.floor(16 * pc[..., 0] / pc[..., 2] + 1.5), np.floor(16 * pc[..., 1] / pc[..., 2] + 1.5)
    ins = ((pc[..., 2] > 0) & (px >= 0) & (px <= 2) & (py >= 0) & (py <= 2)).sum(1)
    assert ((ins > 0) & (ins < 64)).any() and (ins == 0).any()


def test_integrate_without_images_and_without_a_colour_volume():
    t, w, c = _check_integrate(_flat(), BOX, 0, 1, imgs=False)
    assert (c == 0).all() and (w > 0).any()
    _check_integrate(_flat(), BOX, 0, 1, colour=False)


def test_integrate_with_an_origin_and_a_depth_limit():
    st = {}
    _check_integrate(TC.room_views(9, 13, 4), TC.blocks(TC.room_views(9, 13, 4), 0.125, 0.375, (0.0625, 0.5, -0.25), 2.5)[0], 0, 4, st, vs=0.125, trunc=0.375,
                     origin=(0.0625, 0.5, -0.25), depth_max=2.5)
    assert st["fused"] > 0 and st["unobserved"] > 0


# ------------------------------------------------------------------------------------------ mesh
def _check_mesh(keys, t, w, rgb=None, **kw):
    exp_v, exp_c, exp_t = TC.mesh(keys, t, w, rgb, kw.get("vs", 1.0), kw.get("origin"), kw.get("min_weight", 1.0))
    rc, cnt, gv, gc, gt = raw_mesh(keys, t, w, rgb, **kw)
    assert rc == 0 and cnt == [len(exp_v), len(exp_t)], (rc, cnt, len(exp_v), len(exp_t))
    same(gv, exp_v, "verts")
    same(gt, exp_t, "tris")
    if rgb is not None:
        same(gc, exp_c, "cols")
    else:
        assert (gc.view(np.uint8) == FILL).all()
    return gv, gt


def test_mesh_of_a_sphere_is_closed():
    keys, t, w = TC.sphere_volume()
    verts, tris = _check_mesh(keys, t, w)
    rep = TC.mesh_report(verts, tris)
    print(f"[tsdf mesh] sphere: {rep}")
    full = 4.0 / 3.0 * np.pi * 4.4 ** 3
    assert rep["closed"] and rep["euler"] == 2 and rep["unreferenced"] == 0 and (1 - TC.SPHERE_MAX_VOLUME_DEFICIT) * full <= rep["volume"] <= full
    assert (rep["V"], rep["F"]) == (1064, 2124)


def test_mesh_with_a_missing_block_is_open_there():
    keys, t, w = TC.sphere_volume(drop=(0, 1, 0))
    verts, tris = _check_mesh(keys, t, w, vs=0.5, origin=(0.25, -1.0, 3.0))
    rep = TC.mesh_report(verts, tris)
    assert len(tris) and rep["directed_once"] and not rep["closed"] and rep["unreferenced"] == 0


@pytest.mark.parametrize("min_weight", [1.0, 2.5])
def test_mesh_of_a_random_volume_with_zeros_unknowns_and_colours(min_weight):
    keys, t, w, rgb = TC.random_volume(3)
    assert (t == 0).any() and (w < 1).any()
    _check_mesh(keys, t, w, rgb, vs=0.125, origin=(1.0, 2.0, -3.0), min_weight=min_weight)
    _check_mesh(keys, t, w, None, min_weight=min_weight)


def test_mesh_of_a_lone_block():
    keys, t, w = TC.sphere_volume(radius=2.6, centre=(3.5, 3.25, 3.75), lo=(0, 0, 0), hi=(1, 1, 1))
    verts, tris = _check_mesh(keys, t, w)
    assert TC.mesh_report(verts, tris)["closed"]
    keys, t, w = TC.sphere_volume(lo=(0, 0, 0), hi=(1, 1, 1))          # the sphere leaves through the block's faces
    verts, tris = _check_mesh(keys, t, w)
    assert len(tris) and not TC.mesh_report(verts, tris)["closed"]


def test_mesh_of_nothing_known_is_empty():
    keys, t, w = TC.sphere_volume(lo=(0, 0, 0), hi=(1, 1, 1))
    rc, cnt, gv, gc, gt = raw_mesh(keys, t, np.full_like(w, 0.5), max_v=4, max_t=4)
    assert rc == 0 and cnt == [0, 0] and (gv.view(np.uint8) == FILL).all() and (gt.view(np.uint8) == FILL).all()


def test_mesh_counts_only_and_refuses_a_short_buffer():
    L, lib = _lib()
    keys, t, w, rgb = TC.random_volume(5)
    exp_v, _c, exp_t = TC.mesh(keys, t, w, rgb)
    rc, cnt, gv, gc, gt = raw_mesh(keys, t, w, rgb, count_only=True)
    assert rc == 0 and cnt == [len(exp_v), len(exp_t)]
    assert all((b.view(np.uint8) == FILL).all() for b in (gv, gc, gt))
    for mv, mt in ((len(exp_v) - 1, len(exp_t)), (len(exp_v), len(exp_t) - 1)):
        rc, cnt, gv, gc, gt = raw_mesh(keys, t, w, rgb, max_v=mv, max_t=mt)
        msg = lib.sta_tsdf_last_error().decode()
        assert rc != 0 and cnt == [len(exp_v), len(exp_t)] and str(len(exp_v)) in msg and str(len(exp_t)) in msg, (rc, cnt, msg)
        assert all((b.view(np.uint8) == FILL).all() for b in (gv, gc, gt)), "a refused call wrote to its outputs"


# ------------------------------------------------------------------------------------------ end to end
def test_fuse_equals_the_restatement_twice():
    import torch
    from vista_slam_amd import tsdf
    s = TC.room_scene()
    v, (keys, t, w, c, verts, cols, tris) = TC.room_expected()
    m, vol = tsdf.fuse("cuda:0", **s, voxel_size=0.125, return_volume=True)
    torch.cuda.synchronize()
    same(vol.keys.cpu().numpy().view(np.uint64), keys, "keys")
    for g, e, what in ((vol.tsdf, t, "tsdf"), (vol.weight, w, "weight"), (vol.rgb, c, "rgb"), (m.vertices, verts, "verts"), (m.colors, cols, "cols"),
                       (m.triangles, tris, "tris")):
        same(g.cpu().numpy(), e, what)
    assert vol.n_observed == TC.blocks(v, 0.125, 0.375)[1] and vol.n_dropped == 0
    d = TC.room_distance(m.vertices.cpu().numpy())
    print(f"[tsdf fuse] room: {vol.n_blocks} blocks, {len(verts)} vertices, {len(tris)} triangles, distance max {d.max():.4f} mean {d.mean():.4f}")
    assert len(tris) > 10000 and d.max() <= TC.ROOM_MAX_VERTEX_DISTANCE
    m2 = tsdf.fuse("cuda:0", **s, voxel_size=0.125)
    assert torch.equal(m2.vertices, m.vertices) and torch.equal(m2.colors, m.colors) and torch.equal(m2.triangles, m.triangles)
    # a second capacity round of allocate gives the same volume
    small = tsdf.TSDFVolume("cuda:0", 0.125)
    old, tsdf.FIRST_MAX_BLOCKS = tsdf.FIRST_MAX_BLOCKS, 16
    try:
        small.allocate(tsdf.views(s["depths"], s["scales"], s["intrinsics"], s["poses"], s["confs"], s["imgs"], conf_thres=s["conf_thres"]))
    finally:
        tsdf.FIRST_MAX_BLOCKS = old
    assert torch.equal(small.keys, vol.keys)


def test_save_data_all_writes_a_mesh_and_leaves_the_other_files_alone(tmp_path):
    from vista_slam_amd import formats, tsdf
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    s = TC.room_scene(9, 13, 4)
    kw = dict(poses=s["poses"], scales=s["scales"], depths=s["depths"], confs=s["confs"], intrinsics=s["intrinsics"], imgs=s["imgs"], conf_thres=s["conf_thres"],
              view_graph={0: [1]}, loop_min_dist=3, view_names=["a", "b", "c", "d"])
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    formats.save_data_all(m, a, **kw)
    formats.save_data_all(m, b, **kw, mesh_voxel_size=0.125)
    assert sorted(os.listdir(b)) == sorted(os.listdir(a) + ["mesh.ply"])
    for f in os.listdir(a):
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
    rec, tris = tsdf.read_mesh_ply(os.path.join(b, "mesh.ply"))
    _v, (keys, t, w, c, verts, cols, etris) = TC.room_expected(9, 13, 4)
    same(tris, etris, "tris")
    same(np.stack([rec["x"], rec["y"], rec["z"]], 1), verts.astype(np.float64), "vertices")
    same(np.stack([rec["red"], rec["green"], rec["blue"]], 1), np.rint(np.clip(cols, 0, 1) * np.float32(255)).astype(np.uint8), "colours")
