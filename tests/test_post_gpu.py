"""GPU: the scalar kernels behind the transformer, each against a float64 reference of the same operation on the same fp32 inputs:
the DPT tail's head_final_kernel and the pose head (sta_debug_head_final, sta_debug_svd_orthogonalize, sta_head_pose), and the output
step through the public ABI (sta_world_pointcloud, sta_estimate_intrinsics, sta_estimate_scale, sta_mat_to_se3, sta_pack_compact).
Cases, references and the derivation of every bound: tests/post_cases.py (conditions asserted on the CPU in
tests/test_row_post_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import post_cases as PC
from helpers import load_golden, rel_l2
from test_gpu_kernels import HEAD_PRECS, TOL
from vista_slam_amd import _lib
from vista_slam_amd import weights as W

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-3          # test_gpu_parity.TOL: the bar of every pose comparison there
FILL = 0xA5              # byte pattern of output buffers before a call: a finite, recognisable value in every type
_cache = {}


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    return gpu_checks


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def filled(G, nbytes):
    return torch.full((max(int(nbytes), 4),), FILL, dtype=torch.uint8, device=G.DEV)


def untouched(buf, first_byte=0):
    return bool((buf[first_byte:] == FILL).all())


def product(G):
    """The PRODUCT library on the tiny model: the output step is public ABI."""
    m = G.model("tiny", precision="f16x3")
    return m, m.lib, m._h


# ------------------------------------------------------------------------------------------ B: head_final, nearest rotation, pose head
@pytest.mark.parametrize("npix", PC.HEAD_NPIX)
@pytest.mark.parametrize("prec", HEAD_PRECS)
def test_head_final(G, prec, npix):
    """Dense w4: all 16 lanes of the butterfly contribute.  x, y, z, c are exact integers (+ one fp32 bias), so what is compared is
    the butterfly and the activations, per pixel, at the bar of check_ops_golden (5 x TOL)."""
    m, lib, h = G.kernel_handle(prec)
    feat, w4, bias = PC.head_final_inputs(npix)
    fd, wd, bd = G.dev(feat), G.dev(w4), G.dev(bias)
    pts = torch.full((npix, 3), float("nan"), device=G.DEV); conf = torch.full((npix,), float("nan"), device=G.DEV)
    _lib.check(lib.sta_debug_head_final(h, fd.data_ptr(), wd.data_ptr(), bd.data_ptr(), npix, pts.data_ptr(), conf.data_ptr(), G.st()))
    torch.cuda.synchronize()
    pts, conf = pts.cpu().numpy(), conf.cpu().numpy()
    rp, rc = PC.postprocess64(PC.head_final_pre64(feat, w4, bias))
    assert np.all(pts[0] == 0), pts[0]                           # xyz = 0: the clamp, not 0 / 0
    ep, ec = PC.pixel_rel(pts, rp), PC.pixel_rel(conf.reshape(-1, 1), rc.reshape(-1, 1))
    print(f"[head_final] {prec} npix {npix}: worst pixel pts {np.nanmax(ep):.3e} conf {np.nanmax(ec):.3e}, bar {5 * TOL[prec]:g}")
    assert not np.isnan(pts).any() and not np.isnan(conf).any()
    assert ep.max() < 5 * TOL[prec], (int(ep.argmax()), ep.max(), pts[ep.argmax()], rp[ep.argmax()])
    assert ec.max() < 5 * TOL[prec], (int(ec.argmax()), ec.max())


def run_svd(G, mats):
    m, lib, h = G.kernel_handle("f16x3")
    B = len(mats)
    md = G.dev(mats)
    r = torch.full((B + 1, 3, 3), 7.0, device=G.DEV)             # one guard matrix behind the last
    _lib.check(lib.sta_debug_svd_orthogonalize(h, md.data_ptr(), r.data_ptr(), B, G.st()))
    torch.cuda.synchronize()
    r = r.cpu().numpy()
    assert np.all(r[B] == 7.0), "wrote past the last matrix"
    return r[:B]


@pytest.mark.parametrize("B", PC.SVD_B)
def test_svd_orthogonalize(G, B):
    mats, kinds = cached("svd", PC.svd_table)
    mats, kinds = mats[:B], kinds[:B]
    r = run_svd(G, mats)
    worst = 0.0
    for i, (mt, k) in enumerate(zip(mats, kinds)):
        if k in ("random", "rot", "rep+", "rep-"):
            e = float(np.abs(r[i] - PC.svd_rotation64(mt)).max())
            worst = max(worst, e)
            assert e < 1e-5, (i, k, e)
        elif k == "rank2":        # sigma3 = 0: the third singular pair is free up to its sign
            e = min(float(np.abs(r[i] - PC.svd_rotation64(mt, s)).max()) for s in (1, -1))
            assert e < 1e-5, (i, k, e)
    # every output - rank 1 and the zero matrix included - is a rotation
    assert np.isfinite(r).all(), np.argwhere(~np.isfinite(r).all((1, 2))).ravel().tolist()
    orth, det = PC.rotation_defects(r)
    print(f"[svd] B {B}: worst regular |R - R64| {worst:.3e} (bar 1e-5), worst |R R^T - I| {orth.max():.3e}, |det - 1| {det.max():.3e}")
    assert orth.max() < 1e-5 and det.max() < 1e-5, (int(orth.argmax()), kinds[orth.argmax()], orth.max(), det.max())


def test_svd_rank2_and_up_bit_identical_to_recorded_run(G):
    """nearest_rotation completes the frame for rank <= 1 inputs (they gave NaN poses); every input of rank >= 2 returns the bits it
    returned before that change (tests/golden/nearest_rotation_r13.npz: the library one commit earlier on the same table)."""
    mats, kinds = cached("svd", PC.svd_table)
    g = load_golden("nearest_rotation_r13")[0]
    assert np.array_equal(g["m"], mats), "the recorded table is not tests/post_cases.svd_table()"
    r = run_svd(G, mats)
    keep = ~np.isin(kinds, ("rank1", "zero"))
    assert (kinds[keep] == "random").sum() == 257 - 16
    assert np.array_equal(r[keep].view(np.uint32), g["r"][keep].view(np.uint32)), np.argwhere((r != g["r"]).any((1, 2)) & keep).ravel().tolist()
    assert np.isnan(g["r"][~keep]).any()              # what the recorded run returned where the rank is <= 1


@pytest.mark.parametrize("wide", [False, True], ids=["stride_D", "stride_3D+4"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_head_pose(G, B, wide):
    m, lib, h = product(G)
    sd = W.state_dict(W.TINY, seed=43)
    D = W.TINY.dec_embed_dim
    rng = np.random.default_rng(53 + B)
    tok = rng.standard_normal((B, D)).astype(np.float32)
    stride = 3 * D + 4 if wide else D
    buf = np.full((B, stride), np.nan, np.float32); buf[:, :D] = tok
    bd = G.dev(buf)
    pose = torch.full((B, 4, 4), float("nan"), device=G.DEV); conf = torch.full((B,), float("nan"), device=G.DEV)
    _lib.check(lib.sta_head_pose(h, bd.data_ptr(), B, stride, pose.data_ptr(), conf.data_ptr(), G.st()))
    torch.cuda.synchronize()
    from oracle import sta_oracle as O
    rp, rc = O.head_pose(W.TINY, sd, tok)
    pose, conf = pose.cpu().numpy(), conf.cpu().numpy()
    per = [rel_l2(pose[b], rp[b]) for b in range(B)]
    print(f"[head_pose] B {B} stride {stride}: pose rel-L2 {rel_l2(pose, rp):.3e}, worst sample {max(per):.3e}, conf {rel_l2(conf, rc):.3e}, bar {POSE_TOL:g}")
    assert rel_l2(pose, rp) < POSE_TOL and max(per) < POSE_TOL and rel_l2(conf, rc) < POSE_TOL, per
    assert np.array_equal(pose[:, 3], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (B, 4)))


# ------------------------------------------------------------------------------------------ C: world point cloud
def cloud_case(G, geom, klass):
    def make():
        depths, scales, K, poses, imgs = PC.cloud_inputs(geom, klass)
        world, mag = PC.cloud_ref64(depths, scales, K, poses)
        col = PC.color_of(imgs).transpose(0, 2, 3, 1)
        dev = tuple(G.dev(a) for a in (depths, scales, K, poses, imgs))
        return dev, world, mag, np.ascontiguousarray(col)
    return cached(("cloud", geom, klass), make)


def run_cloud(G, geom, klass, pattern, want=("pts", "col", "rec"), with_imgs=True):
    m, lib, h = product(G)
    (dd, sd, Kd, Pd, imd), world, mag, col = cloud_case(G, geom, klass)
    conf, keep = PC.cloud_conf(geom, pattern)
    cd = G.dev(conf)
    N, H, Wd = geom
    cap = N * H * Wd + 8
    bufs = {"pts": filled(G, cap * 12), "col": filled(G, cap * 12), "rec": filled(G, cap * 27)}
    count = C.c_int64(-1)
    ptr = {k: (bufs[k].data_ptr() if k in want else None) for k in bufs}
    _lib.check(lib.sta_world_pointcloud(h, dd.data_ptr(), sd.data_ptr(), Kd.data_ptr(), Pd.data_ptr(), cd.data_ptr(),
                                        imd.data_ptr() if with_imgs else None, N, H, Wd, PC.CLOUD_THRES,
                                        ptr["pts"], ptr["col"], ptr["rec"], C.byref(count), G.st()))
    torch.cuda.synchronize()
    M = int(keep.sum())
    assert count.value == M, (count.value, M)
    out = {}
    for k, row in (("pts", 12), ("col", 12), ("rec", 27)):
        assert untouched(bufs[k], M * row if k in want else 0), f"{k}: bytes at or past row {M} were written" if k in want else f"{k} was not requested"
        raw = bufs[k][:M * row].cpu().numpy()
        out[k] = raw.view(np.float32).reshape(M, 3) if row == 12 else raw.reshape(M, 27)
    return out, keep, world[keep], mag[keep], (col[keep] if with_imgs else np.zeros((M, 3), np.float32))


def check_points(pts, world, mag, klass, tag):
    if len(pts) == 0:
        return 0.0
    if klass == "exact":
        bad = np.argwhere(pts.astype(np.float64) != world)         # values, not bytes: -0.0 == 0.0
        assert len(bad) == 0, (tag, len(bad), bad[:3].tolist())
        return 0.0
    ratio = np.abs(pts.astype(np.float64) - world) / (PC.CLOUD_BOUND * mag)
    assert ratio.max() <= 1.0, (tag, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    return float(ratio.max())


def check_cloud(out, want, world, mag, col, klass, tag):
    worst = 0.0
    if "pts" in want:
        worst = check_points(out["pts"], world, mag, klass, tag)      # kept set and order: a point of another pixel is metres off
    if "col" in want:
        assert np.array_equal(out["col"], col), tag
    if "rec" in want:
        xyz, rgb = PC.ply_record_fields(out["rec"])
        if "pts" in want:
            assert np.array_equal(xyz, out["pts"].astype(np.float64)), tag         # bytes 0..23: the float64 of the returned fp32 point
        assert np.array_equal(xyz, xyz.astype(np.float32).astype(np.float64)), tag
        worst = max(worst, check_points(xyz.astype(np.float32), world, mag, klass, tag))
        assert np.array_equal(rgb, PC.color_byte(col)), tag
    return worst


@pytest.mark.parametrize("pattern", PC.CLOUD_PATTERNS)
@pytest.mark.parametrize("geom", PC.CLOUD_GEOMS, ids=str)
def test_world_pointcloud_general(G, geom, pattern):
    want = ("pts", "col", "rec")
    out, keep, world, mag, col = run_cloud(G, geom, "general", pattern, want)
    worst = check_cloud(out, want, world, mag, col, "general", (geom, pattern))
    nblk, per = PC.cloud_blocks(geom)
    print(f"[cloud] {geom} {pattern}: {int(keep.sum())} of {keep.size} kept, {nblk} blocks, {per} per scan thread, worst |err| / (32 x 2^-24 x mag) {worst:.3f} (bar 1)")


@pytest.mark.parametrize("geom", PC.CLOUD_GEOMS, ids=str)
def test_world_pointcloud_exact(G, geom):
    """Power-of-two focal lengths, integer principal points, dyadic depths, signed-permutation poses: fp32 is exact, so are we."""
    want = ("pts", "col", "rec")
    out, keep, world, mag, col = run_cloud(G, geom, "exact", "random", want)
    check_cloud(out, want, world, mag, col, "exact", geom)
    print(f"[cloud] {geom} exact class: {int(keep.sum())} of {keep.size} kept, all equal")


@pytest.mark.parametrize("with_imgs", [True, False], ids=["imgs", "no_imgs"])
@pytest.mark.parametrize("want", [("pts",), ("col",), ("rec",), ("pts", "rec")], ids="+".join)
def test_world_pointcloud_outputs_alone(G, want, with_imgs):
    """Each output requested alone (the others NULL and untouched); imgs == NULL gives colour 0."""
    for geom in PC.CLOUD_GEOMS[:3]:
        out, keep, world, mag, col = run_cloud(G, geom, "general", "random", want, with_imgs)
        check_cloud(out, want, world, mag, col, "general", (geom, want, with_imgs))
    out, keep, world, mag, col = run_cloud(G, PC.CLOUD_GEOMS[1], "general", "none", want, with_imgs)
    assert keep.sum() == 0                       # (run_cloud: a count of 0 leaves every byte of every buffer as it was)


# ------------------------------------------------------------------------------------------ C: intrinsics, scale
def intr_case(G, B, H, Wd):
    def make():
        pts, conf = PC.intr_inputs(B, H, Wd)
        return pts, conf, G.dev(pts), G.dev(conf)
    return cached(("intr", B, H, Wd), make)


# every group size that divides B (B = 1 with groups of 2: test_estimate_intrinsics_refuses_bad_groups)
INTR_RUNS = [(B, H, Wd, nblk, s) for B, H, Wd, nblk in PC.INTR_SHAPES for s in PC.INTR_SHARED if s < 2 or B % s == 0]


@pytest.mark.parametrize("B,H,Wd,nblk,shared", INTR_RUNS, ids=lambda v: str(v))
def test_estimate_intrinsics(G, B, H, Wd, nblk, shared):
    m, lib, h = product(G)
    pts, conf, pd, cd = intr_case(G, B, H, Wd)
    Kref, cmref = PC.intr_ref(pts, conf, shared)
    Kref = Kref.reshape(-1, 3, 3)
    ng = len(Kref)
    worst = 0
    for outs in (True, False):
        Kb = filled(G, B * 36 + 36); db = filled(G, B * H * Wd * 4); mb = filled(G, B * 4 + 4)
        _lib.check(lib.sta_estimate_intrinsics(h, pd.data_ptr(), cd.data_ptr(), B, H, Wd, shared, Kb.data_ptr(),
                                               db.data_ptr() if outs else None, mb.data_ptr() if outs else None, G.st()))
        torch.cuda.synchronize()
        K = Kb[:ng * 36].cpu().numpy().view(np.float32).reshape(ng, 3, 3)
        assert untouched(Kb, ng * 36), "K written past its groups"
        mask = np.zeros((3, 3), bool); mask[0, 0] = mask[1, 1] = True
        assert np.array_equal(K[:, ~mask], Kref[:, ~mask]), (K, Kref)                 # principal point, zeros, 1: exact
        u = PC.ulp_diff(K[:, mask], Kref[:, mask])
        worst = max(worst, int(u.max()))
        assert u.max() <= 1, (shared, K[:, mask], Kref[:, mask])
        if outs:
            depth = db.cpu().numpy().view(np.uint32).reshape(B, H, Wd)
            assert np.array_equal(depth, pts[..., 2].view(np.uint32)), "depth is not Z bit for bit"
            cm = mb[:B * 4].cpu().numpy().view(np.float32)
            assert untouched(mb, B * 4)
            um = PC.ulp_diff(cm, cmref)
            worst = max(worst, int(um.max()))
            assert um.max() <= 1, (cm, cmref)
        else:
            assert untouched(db) and untouched(mb)
    print(f"[intrinsics] B {B} {H}x{Wd} nblk {nblk} shared {shared}: worst {worst} ulp (bar 1)")


def test_estimate_intrinsics_refuses_bad_groups(G):
    m, lib, h = product(G)
    pts, conf, pd, cd = intr_case(G, 1, 513, 1024)
    Kb = filled(G, 72)
    assert lib.sta_estimate_intrinsics(h, pd.data_ptr(), cd.data_ptr(), 1, 513, 1024, 2, Kb.data_ptr(), None, None, G.st()) != 0
    torch.cuda.synchronize()
    assert untouched(Kb)


@pytest.mark.parametrize("n", PC.SCALE_N)
def test_estimate_scale(G, n):
    m, lib, h = product(G)
    Di, Dj, ci, cj = PC.scale_inputs(n)
    d = [G.dev(a) for a in (Di, Dj, ci, cj)]
    out = filled(G, 8)
    _lib.check(lib.sta_estimate_scale(h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, out.data_ptr(), G.st()))
    torch.cuda.synchronize()
    s = out[:4].cpu().numpy().view(np.float32)[0]
    ref = PC.scale_ref(Di, Dj, ci, cj)
    u = int(PC.ulp_diff(s, ref))
    print(f"[scale] n {n}: {s!r} vs {ref!r}, {u} ulp (bar 1)")
    assert u <= 1 and untouched(out, 4)


# ------------------------------------------------------------------------------------------ C: mat_to_se3, pack_compact
@pytest.mark.parametrize("B", PC.SE3_B)
def test_mat_to_se3(G, B):
    m, lib, h = product(G)
    pose = cached("se3", PC.se3_table)[:B]
    pd = G.dev(pose)
    out = filled(G, B * 28 + 28)
    _lib.check(lib.sta_mat_to_se3(h, pd.data_ptr(), B, out.data_ptr(), G.st()))
    torch.cuda.synchronize()
    assert untouched(out, B * 28)
    se3 = out[:B * 28].cpu().numpy().view(np.float32).reshape(B, 7)
    ref, raw, _br = PC.shepperd64(pose)
    assert np.array_equal(se3[:, :3].view(np.uint32), pose[:, :3, 3].view(np.uint32)), "translation is not copied bit for bit"
    q = se3[:, 3:].astype(np.float64)
    e = np.abs(q - ref[:, 3:]).max(1)
    flip = np.abs(q + ref[:, 3:]).max(1)
    e = np.where(np.abs(raw) < 1e-6, np.minimum(e, flip), e)          # qw ~ 0: q and -q are the same rotation and both have qw >= 0
    nrm = np.abs(np.linalg.norm(q, axis=1) - 1)
    rr = np.abs(PC.quat_to_rot(q) - pose[:, :3, :3]).max((1, 2))
    print(f"[mat_to_se3] B {B}: worst |q - q64| {e.max():.3e}, | |q| - 1 | {nrm.max():.3e}, |R(q) - R| {rr.max():.3e} (bars 2e-6)")
    assert e.max() < 2e-6, (int(e.argmax()), e.max())
    assert nrm.max() < 2e-6 and np.all(se3[:, 6] >= 0)
    assert rr.max() < 2e-6, (int(rr.argmax()), rr.max())


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("H,Wd", PC.PACK_HW)
@pytest.mark.parametrize("B", PC.PACK_B)
def test_pack_compact(G, B, H, Wd, pad):
    """Pure data movement: the record is compared ON THE DEVICE with the same slices gathered by torch, bit for bit."""
    m, lib, h = product(G)
    hw = H * Wd
    gen = torch.Generator(device=G.DEV).manual_seed(59 + B + hw)
    pts = [torch.randn(B, hw, 3, device=G.DEV, generator=gen) for _ in range(2)]
    conf = [torch.rand(B, hw, device=G.DEV, generator=gen) + 1 for _ in range(2)]
    pose = [torch.randn(B, 16, device=G.DEV, generator=gen) for _ in range(2)]
    pc = [torch.rand(B, device=G.DEV, generator=gen) for _ in range(2)]
    width = 2 * (17 + 2 * hw)
    stride = width + pad
    out = torch.full((B, stride), -7.25, device=G.DEV)
    arr = lambda ts: (C.c_void_p * 2)(ts[0].data_ptr(), ts[1].data_ptr())
    _lib.check(lib.sta_pack_compact(h, arr(pts), arr(conf), arr(pose), arr(pc), B, H, Wd, out.data_ptr(), stride, G.st()))
    torch.cuda.synchronize()
    want = torch.cat([torch.cat([pose[v], pc[v][:, None], pts[v][:, :, 2], conf[v]], 1) for v in range(2)], 1)
    assert want.shape == (B, width)
    assert torch.equal(out[:, :width].view(torch.int32), want.view(torch.int32))
    assert bool((out[:, width:] == -7.25).all()), "padding written"
