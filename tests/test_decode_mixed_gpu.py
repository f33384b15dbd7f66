"""GPU: the decoder on view pairs of different resolution (sta_decode_mixed through STAFrontend.decode_stereo_mixed /
forward_pair_mixed) against the reference fixtures `decn_*` (tools/gen_golden_decn.py), and the new route against today's route on
equal grids.

Bounds: the project's bar TOL = 1e-3 of tests/test_gpu_parity.py for everything compared with a reference fixture (rel-L2 AND max
norm, range report (0, 0)); 0.1 x bar = 1e-4 for route-vs-route and swap comparisons - the two routes differ only in tile choice
and summation order, README / DESIGN put today's route at <= 3.7e-5 of the reference on the two equal-grid configurations used
here, so two routes that both hold that are <= 7.4e-5 apart by the triangle inequality.

Measured (MI355X; worst over the cases of each class, f16x3h / f16x3; DESIGN.md section 3 keeps the table):
    hook layers vs golden 8.9e-6 / 8.9e-6 (the gain-4 pair; 1.3e-6 .. 5.4e-6 at gain 1)     points 5.2e-5 / 1.9e-5
    confidence 1.4e-6 / 3.6e-7     pose 8.0e-5 / 8.0e-5 (gain 4; <= 1.8e-5 at gain 1)     pose confidence 6.0e-7
    swap 0.0 (bit-identical)     equal grids, new route vs today's: tiny_48x64_b2 0.0, full_224_b1 7.1e-7
    (new route alone vs golden: 2.3e-6 / 4.7e-6 - below 3.7e-5, so the route bound stays at 1e-4)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-3                  # tests/test_gpu_parity.py
ROUTE_TOL = 0.1 * TOL
DEFAULT = "f16x3h"
CASES = ["decn_tiny_48x64_vs_48x80_b2", "decn_tiny_64x48_vs_32x32", "decn_tiny_48x80_vs_32x48_sharp",
         "decn_full_224_vs_224x160_b1", "decn_full_256_vs_224_b1", "decn_full_384x512_vs_224_b1"]


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
    full = "_full_" in case
    if full:
        G.drop_models()
    cfg = W.FULL if full else W.TINY
    seed = int(meta["seed"])
    m = G.model("full" if full else "tiny", float(meta["qk_gain"]), prec, seed=seed)
    B = int(meta["B"])
    shp = ((int(meta["Ha"]), int(meta["Wa"])), (int(meta["Hb"]), int(meta["Wb"])))
    imgs = [torch.from_numpy(W.synth_images(B, H, Wd, seed=seed, tag=t)).cuda() for t, (H, Wd) in enumerate(shp)]
    return g, meta, cfg, m, imgs, shp


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", CASES)
def test_decode_stereo_mixed_vs_reference_golden(G, case, prec):
    """Every hook layer of both sides (pose row included), rel-L2 and max norm; tiny: the decoder alone on the reference's own
    encoder features; the swap decode(b, a) against decode(a, b) at 0.1 x bar."""
    import torch
    from helpers import rel_l2, max_rel
    g, meta, cfg, m, imgs, shp = _setup(G, case, prec)
    m.range_report(reset=True)
    tsub = int(meta["tsub"])
    fa, pa = m._encode_image(imgs[0], None, normalize=False)
    fb, pb = m._encode_image(imgs[1], None, normalize=False)
    if "enc_feat_a" in g:
        assert rel_l2(fa.cpu().numpy(), g["enc_feat_a"]) < TOL and rel_l2(fb.cpu().numpy(), g["enc_feat_b"]) < TOL
        fa, fb = torch.from_numpy(g["enc_feat_a"]).cuda(), torch.from_numpy(g["enc_feat_b"]).cuda()
    assert fa.shape[1] != fb.shape[1]
    d1, d2 = m.decode_stereo_mixed(fa, fb, pa, pb)
    s1, s2 = m.decode_stereo_mixed(fb, fa, pb, pa)
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
    rng = tuple(m.range_report(reset=True))
    print(case, prec, "worst vs golden", max(errs.values()), "swap", swap, "ref_noise", float(g["ref_noise"]), "range", rng)
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    assert swap <= ROUTE_TOL, swap
    assert rng == (0, 0), rng
    # `layers` restricts what is materialised, as in _decode_stereo
    e1, e2 = m.decode_stereo_mixed(fa, fb, pa, pb, layers=[last])
    assert [t is not None for t in e1] == [i == last for i in range(len(e1))]
    assert torch.equal(e1[last], d1[last]) and torch.equal(e2[last], d2[last])


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", CASES)
def test_forward_pair_mixed_vs_reference_golden(G, case, prec):
    """Encode each image at its own shape, decode the pair, both heads per side: points, confidence, pose, pose confidence."""
    import torch
    from helpers import rel_l2, max_rel
    g, meta, cfg, m, imgs, shp = _setup(G, case, prec)
    m.range_report(reset=True)
    sub = int(meta["sub"])
    res = m.forward_pair_mixed(imgs[0], imgs[1])
    torch.cuda.synchronize()
    errs = {}
    for tag, r, (H, Wd) in zip("ab", res, shp):
        pts, conf = r["pts3d_pred"].cpu().numpy(), r["conf"].cpu().numpy()
        B = pts.shape[0]
        assert pts.shape == ((B, Wd, H, 3) if H > Wd else (B, H, Wd, 3)), pts.shape          # a portrait side: transposed views
        for key, got, want in (("pts3d", pts[:, ::sub, ::sub], g[f"{tag}_pts3d"]), ("conf", conf[:, ::sub, ::sub], g[f"{tag}_conf"]),
                               ("pose", r["relative_pose"].cpu().numpy(), g[f"{tag}_pose"]),
                               ("pose_conf", r["relative_pose_conf"].cpu().numpy(), g[f"{tag}_pose_conf"])):
            errs[f"{tag}_{key}"] = max(rel_l2(got, want), max_rel(got, want))
    rng = tuple(m.range_report(reset=True))
    print(case, prec, {k: f"{v:.2e}" for k, v in errs.items()}, "range", rng)
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    assert rng == (0, 0), rng


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", ["tiny_48x64_b2", "full_224_b1"])
def test_equal_grids_new_route_vs_todays_route(G, case, prec):
    """With EQUAL grids decode_stereo_mixed and _decode_stereo compute the same thing by two routes (per-side QKV launches and the
    two-group attention launch against one batch of 2B sequences): both within the bar of the reference golden, and their direct
    difference below 0.1 x bar."""
    import torch
    from helpers import load_golden, rel_l2, max_rel
    from vista_slam_amd import weights as W
    g, meta = load_golden(case)
    full = case.startswith("full")
    if full:
        G.drop_models()
    cfg = W.FULL if full else W.TINY
    m = G.model("full" if full else "tiny", 1.0, prec, seed=43)
    H, Wd, B, sub = int(meta["H"]), int(meta["W"]), int(meta["B"]), int(meta["sub"])
    tsub = max(1, sub)
    imgs = torch.from_numpy(W.synth_images(2 * B, H, Wd, seed=43, tag=0)).cuda()
    fa, pa = m._encode_image(imgs[:B], None, normalize=False)
    fb, pb = m._encode_image(imgs[B:], None, normalize=False)
    m.range_report(reset=True)
    o1, o2 = m._decode_stereo(fa, fb, pa, pb)
    n1, n2 = m.decode_stereo_mixed(fa, fb, pa, pb)
    torch.cuda.synchronize()
    old_g, new_g, direct = 0.0, 0.0, 0.0
    for hk in cfg.hooks[1:]:
        for side, o, n in (("dec1", o1, n1), ("dec2", o2, n2)):
            want = g[f"{side}_hook{hk - 1}"]
            a, b = o[hk - 1].cpu().numpy(), n[hk - 1].cpu().numpy()
            old_g = max(old_g, rel_l2(a[:, ::tsub], want), max_rel(a[:, ::tsub], want))
            new_g = max(new_g, rel_l2(b[:, ::tsub], want), max_rel(b[:, ::tsub], want))
            direct = max(direct, rel_l2(b, a), max_rel(b, a))
    rng = tuple(m.range_report(reset=True))
    print(case, prec, "today's route vs golden", old_g, "new route vs golden", new_g, "new vs today's", direct, "range", rng)
    assert old_g <= TOL and new_g <= TOL, (old_g, new_g)
    assert direct <= ROUTE_TOL, direct
    assert rng == (0, 0), rng


def test_mixed_route_refuses_what_it_does_not_serve(G):
    """Foreign positions with the mixed entry are refused with a message; the equal-grid entries keep refusing unequal counts."""
    import torch
    from vista_slam_amd import weights as W
    m = G.model("tiny", 1.0, DEFAULT)
    imgs = torch.from_numpy(W.synth_images(1, 48, 64, seed=43, tag=0)).cuda(), torch.from_numpy(W.synth_images(1, 48, 80, seed=43, tag=1)).cuda()
    fa, pa = m._encode_image(imgs[0], None, normalize=False)
    fb, pb = m._encode_image(imgs[1], None, normalize=False)
    with pytest.raises(NotImplementedError, match="patch-grid positions only"):
        m.decode_stereo_mixed(fa, fb, pa + 2, pb)
    with pytest.raises(AssertionError, match="same token grid"):
        m._decode_stereo(fa, fb, pa, pb)
