"""GPU: the decoder on TOKEN SUBSETS - caller positions together with unequal token counts (sta_decode_tokens through
STAFrontend.decode_stereo_tokens / forward_pair_window) - against the reference fixtures `dect_*` (tools/gen_golden_dect.py), the new
route against the two existing ones where they overlap, and the rotation kernel alone (sta_debug_rope_tokens).

Bounds: the project's bar TOL = 1e-3 of tests/test_gpu_parity.py for everything compared with a reference fixture (rel-L2 AND max
norm, range report (0, 0)); 0.1 x bar = 1e-4 for route-vs-route and swap comparisons, by the argument of tests/test_decode_mixed_gpu.py:
every route is measured well inside half of that against the reference, so two of them are inside it of each other.

The kernel alone, on inputs k * 2^-8 (|k| <= 1024: exact in an fp16 plane) and positions in [-1, 40]:
  (a) against rope_planes_kernel (the per-buffer kernel of sta_decode_pos) on the same planes: expected identical; asserted
      |diff| <= 2^-20 max(|v0|, |v1|) per rotated pair (v0, v1 the pair's inputs) - one fp32 rounding of one product, should the
      compiler contract the two kernels differently, plus one step of the lo plane.
  (b) against an fp64 rotation by the exact angles pos * 100^(-f/16): |err| <= (pos_max + 2) 2^-21 (|v0| + |v1|) per element - the
      host table's fp32 angle is off by <= 2 ulp of an angle <= pos_max, cosf / sinf by 1 ulp, the hi + lo split adds 2^-21.  A
      position off by one at the LOWEST frequency moves the result by 1.3e-2 |v|: a thousand times the bound.
  (c) rows (ntok, npad) of every sequence of every buffer come back bit for bit, for both groups.

Measured (MI355X; worst over the cases of each class, f16x3h / f16x3; DESIGN.md section 3 keeps the table):
    hook layers vs golden 1.4e-5 / 1.4e-5 (the gain-3 window; <= 5.0e-6 at gain 1)     points 5.4e-5 / 9.6e-6
    confidence 1.1e-6 / 3.6e-7     pose 1.3e-5     pose confidence 2.4e-7     swap 0.0 (bit-identical)
    tokens route vs sta_decode_pos route 5.6e-7, vs sta_decode_mixed route 5.6e-7
    kernel: (a) 0.34 of the bound (not bit-identical: the two kernels' products are contracted differently), (b) 0.053 of the bound
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-3                  # tests/test_gpu_parity.py
ROUTE_TOL = 0.1 * TOL
DEFAULT = "f16x3h"
CASES = ["dect_tiny_win_vs_full_b2", "dect_tiny_win_vs_pruned_b2", "dect_tiny_one_vs_full_sharp", "dect_tiny_63_vs_64",
         "dect_full_224_win_vs_full_sharp", "dect_full_224_pruned_b1"]
WINDOWS = {"dect_tiny_win_vs_full_b2": [(1, 2, 2, 3), (2, 0, 2, 3)], "dect_full_224_win_vs_full_sharp": (6, 4, 8, 10)}   # side a of the cases forward_pair_window serves


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    yield gpu_checks
    gpu_checks.drop_models()


def _setup(G, case, prec):
    import torch
    from helpers import load_golden
    from vista_slam_amd import weights as W
    g, meta = load_golden(case)
    full = case.startswith("dect_full")
    if full:
        G.drop_models()
    cfg = W.FULL if full else W.TINY
    seed = int(meta["seed"])
    m = G.model("full" if full else "tiny", float(meta["qk_gain"]), prec, seed=seed)
    B = int(meta["B"])
    shp = ((int(meta["Ha"]), int(meta["Wa"])), (int(meta["Hb"]), int(meta["Wb"])))
    imgs = [torch.from_numpy(W.synth_images(B, H, Wd, seed=seed, tag=t)).cuda() for t, (H, Wd) in enumerate(shp)]
    return g, meta, cfg, m, imgs, shp


def _subsets(m, g, imgs):
    """Whole-frame encoder features (tiny: the reference's own, after checking ours against them) -> the two sides' tokens and the
    positions the fixture fed."""
    import torch
    from helpers import rel_l2
    Fa, Pa = m._encode_image(imgs[0], None, normalize=False)
    Fb, Pb = m._encode_image(imgs[1], None, normalize=False)
    if "enc_feat_a" in g:
        assert rel_l2(Fa.cpu().numpy(), g["enc_feat_a"]) < TOL and rel_l2(Fb.cpu().numpy(), g["enc_feat_b"]) < TOL
        Fa, Fb = torch.from_numpy(g["enc_feat_a"]).cuda(), torch.from_numpy(g["enc_feat_b"]).cuda()
    fa, _ = m.select_tokens(Fa, Pa, torch.from_numpy(g["idx_a"]))
    fb, _ = m.select_tokens(Fb, Pb, torch.from_numpy(g["idx_b"]).cuda())
    return fa, fb, torch.from_numpy(g["pos_a"]), torch.from_numpy(g["pos_b"]).cuda()      # one on the CPU, one on the device


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", CASES)
def test_decode_stereo_tokens_vs_reference_golden(G, case, prec):
    """Every hook layer of both sides (pose row included), rel-L2 and max norm; the swap decode(b, a) against decode(a, b) at
    0.1 x bar; `layers` restricts what is materialised; the heads on every side that is a rectangle."""
    import torch
    from helpers import rel_l2, max_rel
    g, meta, cfg, m, imgs, shp = _setup(G, case, prec)
    m.range_report(reset=True)
    tsub, sub = int(meta["tsub"]), int(meta["sub"])
    fa, fb, pa, pb = _subsets(m, g, imgs)
    assert fa.shape[1] != fb.shape[1]
    d1, d2 = m.decode_stereo_tokens(fa, fb, pa, pb)
    s1, s2 = m.decode_stereo_tokens(fb, fa, pb, pa)
    torch.cuda.synchronize()
    assert all(t is not None and t.shape[1] == fa.shape[1] + 1 for t in d1) and all(t.shape[1] == fb.shape[1] + 1 for t in d2)
    errs = {}
    for hk in cfg.hooks[1:]:
        for side, d in (("dec1", d1), ("dec2", d2)):
            got, want = d[hk - 1].cpu().numpy()[:, ::tsub], g[f"{side}_hook{hk - 1}"]
            errs[f"{side}_hook{hk - 1}"] = max(rel_l2(got, want), max_rel(got, want))
    last = cfg.hooks[-1] - 1
    swap = max(max(rel_l2(a.cpu().numpy(), b.cpu().numpy()), max_rel(a.cpu().numpy(), b.cpu().numpy()))
               for a, b in ((s1[last], d2[last]), (s2[last], d1[last]), (s1[0], d2[0]), (s2[cfg.hooks[1] - 1], d1[cfg.hooks[1] - 1])))
    for tag, feat, dec in (("a", fa, d1), ("b", fb, d2)):
        pose = m.head_pose_s(dec[-1][:, 0, :])
        errs[f"{tag}_pose"] = max(rel_l2(pose["pose"].cpu().numpy(), g[f"{tag}_pose"]), max_rel(pose["pose"].cpu().numpy(), g[f"{tag}_pose"]))
        errs[f"{tag}_pose_conf"] = max_rel(pose["conf"].cpu().numpy(), g[f"{tag}_pose_conf"])
        h, w = int(meta[f"rect_{tag}h"]), int(meta[f"rect_{tag}w"])
        if h:
            pts = m.head_pts([feat] + [t[:, 1:, :] for t in dec], [[16 * h, 16 * w]] * feat.shape[0])
            for key in ("pts3d", "conf"):
                got, want = pts[key].cpu().numpy()[:, ::sub, ::sub], g[f"{tag}_{key}"]
                errs[f"{tag}_{key}"] = max(rel_l2(got, want), max_rel(got, want))
    rng = tuple(m.range_report(reset=True))
    print(case, prec, {k: f"{v:.2e}" for k, v in errs.items()}, "swap", swap, "ref_noise", float(g["ref_noise"]), "range", rng)
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    assert swap <= ROUTE_TOL, swap
    assert rng == (0, 0), rng
    e1, e2 = m.decode_stereo_tokens(fa, fb, pa, pb, layers=[last])
    assert [t is not None for t in e1] == [i == last for i in range(len(e1))] == [t is not None for t in e2]
    assert torch.equal(e1[last], d1[last]) and torch.equal(e2[last], d2[last])


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", list(WINDOWS))
def test_forward_pair_window_vs_reference_golden(G, case, prec):
    """Encode both frames whole, slice the window, decode the subsets, both heads per side at the side's token shape: points,
    confidence, pose, pose confidence."""
    import torch
    from helpers import rel_l2, max_rel
    g, meta, cfg, m, imgs, shp = _setup(G, case, prec)
    m.range_report(reset=True)
    sub = int(meta["sub"])
    res = m.forward_pair_window(imgs[0], imgs[1], window_a=WINDOWS[case])
    torch.cuda.synchronize()
    errs = {}
    for tag, r in zip("ab", res):
        h, w = int(meta[f"rect_{tag}h"]), int(meta[f"rect_{tag}w"])
        pts, conf = r["pts3d_pred"].cpu().numpy(), r["conf"].cpu().numpy()
        assert pts.shape == (pts.shape[0], 16 * h, 16 * w, 3), pts.shape
        for key, got, want in (("pts3d", pts[:, ::sub, ::sub], g[f"{tag}_pts3d"]), ("conf", conf[:, ::sub, ::sub], g[f"{tag}_conf"]),
                               ("pose", r["relative_pose"].cpu().numpy(), g[f"{tag}_pose"]),
                               ("pose_conf", r["relative_pose_conf"].cpu().numpy(), g[f"{tag}_pose_conf"])):
            errs[f"{tag}_{key}"] = max(rel_l2(got, want), max_rel(got, want))
    rng = tuple(m.range_report(reset=True))
    print(case, prec, {k: f"{v:.2e}" for k, v in errs.items()}, "range", rng)
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    assert rng == (0, 0), rng


def _route_diff(cfg, new, old):
    from helpers import rel_l2, max_rel
    worst = 0.0
    for hk in cfg.hooks[1:]:
        for n, o in zip(new, old):
            a, b = n[hk - 1].cpu().numpy(), o[hk - 1].cpu().numpy()
            worst = max(worst, rel_l2(a, b), max_rel(a, b))
    return worst


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_equal_counts_foreign_positions_vs_decode_pos_route(G, prec):
    """Equal counts with foreign positions (the decpos_tiny_48x64_b2 inputs): sta_decode_tokens against sta_decode_pos."""
    import torch
    from helpers import load_golden
    from vista_slam_amd import weights as W
    g, meta = load_golden("decpos_tiny_48x64_b2")
    m = G.model("tiny", float(meta["qk_gain"]), prec, seed=int(meta["seed"]))
    m.range_report(reset=True)
    fa, fb = torch.from_numpy(g["enc_feat_a"]).cuda(), torch.from_numpy(g["enc_feat_b"]).cuda()
    for tag in ("shift", "flip", "regrid"):
        qa, qb = torch.from_numpy(g[f"{tag}_pos_a"]).cuda(), torch.from_numpy(g[f"{tag}_pos_b"]).cuda()
        old = m._decode_stereo(fa, fb, qa, qb)
        new = m.decode_stereo_tokens(fa, fb, qa, qb)
        torch.cuda.synchronize()
        d = _route_diff(W.TINY, new, old)
        print("decpos_tiny_48x64_b2", tag, prec, "tokens route vs decode_pos route", d)
        assert d <= ROUTE_TOL, (tag, d)
    assert tuple(m.range_report(reset=True)) == (0, 0)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_unequal_counts_grid_positions_vs_mixed_route(G, prec):
    """Unequal counts with patch-grid positions (the decn_tiny_48x64_vs_48x80_b2 inputs): sta_decode_tokens against sta_decode_mixed."""
    import torch
    from helpers import load_golden
    from vista_slam_amd import weights as W
    g, meta = load_golden("decn_tiny_48x64_vs_48x80_b2")
    m = G.model("tiny", float(meta["qk_gain"]), prec, seed=int(meta["seed"]))
    m.range_report(reset=True)
    fa, fb = torch.from_numpy(g["enc_feat_a"]).cuda(), torch.from_numpy(g["enc_feat_b"]).cuda()
    B = fa.shape[0]
    pa, pb = m._positions(B, 3, 4), m._positions(B, 3, 5)
    old = m.decode_stereo_mixed(fa, fb, pa, pb)
    new = m.decode_stereo_tokens(fa, fb, pa, pb)
    torch.cuda.synchronize()
    d = _route_diff(W.TINY, new, old)
    print("decn_tiny_48x64_vs_48x80_b2", prec, "tokens route vs mixed route", d)
    assert d <= ROUTE_TOL, d
    assert tuple(m.range_report(reset=True)) == (0, 0)


# ------------------------------------------------------------------------------------------ the rotation kernel alone
ROPE_SHAPES = [(2, 2, 2, 6, 12), (1, 1, 2, 1, 12), (1, 1, 2, 63, 64), (2, 1, 3, 67, 13)]      # (S1, S2, heads, ntok_a, ntok_b)
POS_MAX = 40


def _rope_inputs(S1, S2, heads, na, nb, nbuf, seed):
    rs = np.random.default_rng(seed)
    npad = (max(na, nb) + 1 + 63) // 64 * 64
    bufs = [(rs.integers(-1024, 1025, size=(S1 + S2, heads, npad, 64)) * 2.0 ** -8).astype(np.float32) for _ in range(nbuf)]
    pos = [rs.integers(-1, POS_MAX + 1, size=(S, n, 2)).astype(np.int32) for S, n in ((S1, na), (S2, nb))]
    return bufs, pos, npad


def _rope_run(G, prec, bufs, pos, S1, S2, heads, na, nb, which):
    import torch
    from vista_slam_amd import _lib
    m, lib, h = G.kernel_handle(prec)
    dev = [G.dev(b) for b in bufs]
    table = G.dev(np.concatenate([pos[0].ravel(), pos[1].ravel()]))
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in dev])
    _lib.check(lib.sta_debug_rope_tokens(h, ptrs, len(dev), S1, S2, heads, na, nb, table.data_ptr(), POS_MAX, which, G.st()))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev]


def _rope_ref64(buf, pos, S1, heads, na, nb):
    """fp64 rotation of the live rows; rows past the pose token are copied."""
    out = buf.astype(np.float64)
    inv = 100.0 ** (-np.arange(16, dtype=np.float64) / 16.0)
    for s in range(buf.shape[0]):
        n = na if s < S1 else nb
        p = np.concatenate([(pos[0][s] if s < S1 else pos[1][s - S1]).astype(np.float64), [[-1.0, -1.0]]], 0)      # [n + 1, 2], pose token last
        for xy in range(2):
            ang = p[:, xy, None] * inv[None, :]                                  # [n + 1, 16]
            c, sn = np.cos(ang)[None], np.sin(ang)[None]
            v0 = buf[s, :, :n + 1, xy * 32:xy * 32 + 16].astype(np.float64)
            v1 = buf[s, :, :n + 1, xy * 32 + 16:xy * 32 + 32].astype(np.float64)
            out[s, :, :n + 1, xy * 32:xy * 32 + 16] = v0 * c - v1 * sn
            out[s, :, :n + 1, xy * 32 + 16:xy * 32 + 32] = v1 * c + v0 * sn
    return out


def _pair_mag(buf, fn):
    """fn(|v0|, |v1|) of every rotation pair (d, d + 16), broadcast back to both elements of the pair: [S, heads, npad, 64]."""
    a = np.abs(buf.astype(np.float64)).reshape(buf.shape[:3] + (2, 2, 16))
    mag = fn(a[..., 0, :], a[..., 1, :])
    return np.broadcast_to(mag[..., None, :], a.shape).reshape(buf.shape)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("nbuf", [1, 3])
@pytest.mark.parametrize("shape", ROPE_SHAPES)
def test_rope_tokens_kernel_alone(G, shape, nbuf, prec):
    S1, S2, heads, na, nb = shape
    bufs, pos, npad = _rope_inputs(S1, S2, heads, na, nb, nbuf, seed=7 + na)
    new = _rope_run(G, prec, bufs, pos, S1, S2, heads, na, nb, 0)
    old = _rope_run(G, prec, bufs, pos, S1, S2, heads, na, nb, 1)
    worst_a = worst_b = 0.0
    for b in range(nbuf):
        live = np.zeros(bufs[b].shape, bool)
        live[:S1, :, :na + 1] = True
        live[S1:, :, :nb + 1] = True
        # (c) dead rows: bit for bit what went in, by both kernels
        assert np.array_equal(new[b][~live].view(np.uint32), bufs[b][~live].view(np.uint32)), ("dead rows written", b)
        assert np.array_equal(old[b][~live].view(np.uint32), bufs[b][~live].view(np.uint32)), ("dead rows written (per-buffer kernel)", b)
        assert np.isfinite(new[b]).all()
        # (a) against the per-buffer kernel
        bound_a = 2.0 ** -20 * _pair_mag(bufs[b], np.maximum)
        diff = np.abs(new[b].astype(np.float64) - old[b].astype(np.float64))
        worst_a = max(worst_a, float((diff / np.maximum(bound_a, 1e-300))[live].max()))
        assert (diff <= bound_a)[live].all(), ("vs rope_planes_kernel", b, np.argwhere((diff > bound_a) & live)[:4])
        # (b) against the fp64 rotation
        ref = _rope_ref64(bufs[b], pos, S1, heads, na, nb)
        bound_b = (POS_MAX + 2) * 2.0 ** -21 * _pair_mag(bufs[b], np.add)
        err = np.abs(new[b].astype(np.float64) - ref)
        worst_b = max(worst_b, float((err / np.maximum(bound_b, 1e-300))[live & (bound_b > 0)].max()))
        assert (err <= bound_b)[live].all(), ("vs fp64 rotation", b, np.argwhere((err > bound_b) & live)[:4])
        assert not np.array_equal(new[b][live], bufs[b][live])          # it did rotate
    print(shape, nbuf, prec, "new vs per-buffer kernel, fraction of bound", worst_a, "new vs fp64, fraction of bound", worst_b)


# ------------------------------------------------------------------------------------------ refusals
def test_tokens_route_refusals(G):
    """The shim refuses float positions, positions below -1 and a batch mismatch; the C entry bad arguments with status -1 and a
    message; the existing refusals of decode_stereo_mixed and _decode_stereo are still raised."""
    import torch
    from vista_slam_amd import weights as W
    m = G.model("tiny", 1.0, DEFAULT)
    imgs = torch.from_numpy(W.synth_images(2, 48, 64, seed=43, tag=0)).cuda(), torch.from_numpy(W.synth_images(2, 48, 80, seed=43, tag=1)).cuda()
    Fa, Pa = m._encode_image(imgs[0], None, normalize=False)
    Fb, Pb = m._encode_image(imgs[1], None, normalize=False)
    fa, pa = m.window_tokens(Fa, Pa, (3, 4), (1, 1, 2, 2))
    assert fa.shape == (2, 4, W.TINY.enc_embed_dim) and pa[0].tolist() == [[1, 1], [1, 2], [2, 1], [2, 2]]
    f2, p2 = m.select_tokens(Fb, Pb, [14, 0, 7])
    assert f2.shape[1] == 3 and p2[1].tolist() == [[2, 4], [0, 0], [1, 2]] and torch.equal(f2[:, 1], Fb[:, 0])
    d1, d2 = m.decode_stereo_tokens(fa, f2, pa, p2)                 # what the refusals below are variations of
    assert d1[-1].shape[1] == 5 and d2[-1].shape[1] == 4
    with pytest.raises(AssertionError, match="integer"):
        m.decode_stereo_tokens(fa, f2, pa.float(), p2)
    with pytest.raises(ValueError, match="below -1"):
        m.decode_stereo_tokens(fa, f2, pa - 3, p2)
    with pytest.raises(AssertionError, match="same batch"):
        m.decode_stereo_tokens(fa, f2[:1], pa, p2[:1])
    with pytest.raises(AssertionError, match="one positions row per batch entry"):
        m.decode_stereo_tokens(fa, f2, pa[:1], p2)
    with pytest.raises(AssertionError, match="leaves the"):
        m.window_tokens(Fa, Pa, (3, 4), (2, 2, 2, 3))
    L = m.cfg.dec_depth + 1
    nul = (C.c_void_p * L)()
    q1, q2 = pa.contiguous(), p2.contiguous()
    for args in ((fa.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), 2, 0, 3, 4),          # N1 = 0
                 (None, f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), 2, 4, 3, 4),                   # null features
                 (fa.data_ptr(), f2.data_ptr(), q1.data_ptr(), None, 2, 4, 3, 4),                   # null positions
                 (fa.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), 2, 4, 3, 1 << 20)):   # pos_max out of range
        rc = m.lib.sta_decode_tokens(m._h, *args, nul, nul, m._stream())
        assert rc == -1 and len(m.lib.sta_last_error()) > 0, (args[4:], rc)
    with pytest.raises(NotImplementedError, match="patch-grid positions only"):
        m.decode_stereo_mixed(Fa, Fb, Pa + 2, Pb)
    with pytest.raises(AssertionError, match="same token grid"):
        m._decode_stereo(Fa, Fb, Pa, Pb)
