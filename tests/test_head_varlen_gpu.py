"""GPU: the DPT head on batches whose entries differ in patch rectangle (sta_head_pts_varlen through STAFrontend.head_pts_varlen and
forward_pairs_tokens(heads="varlen")) against the reference fixtures, against the per-entry route, and its independence of
neighbours.

Inputs: the fixture's own encoder features, and the decoder hooks of OUR decode_stereo_varlen on them (the route the head is part of:
the packed decoder output, a pose row in front of each entry, is read in place through the row tables).

Bounds: TOL = 1e-3 (rel-L2 and max norm), the project's bar, for everything compared with a reference fixture, with the range report
(0, 0); ROUTE_TOL = 1e-4 for the varlen call against `head_pts` on every entry alone.  What makes passing mean something:
`alt_stacked` of dptv_tiny_b4_edges (tests/test_head_varlen_cpu.py) - feeding the two adjacent 2x8 sides as one 4x8 image moves the
points by 0.23, two hundred times the bar - and the exact tests: permuting the entries and replacing every OTHER entry's inputs leave an
entry bit-identical, which no halo, bilinear tap or tile that crossed an entry border would.

Tile families: automatic, forced 2, forced 4 (the 192x128 tiles) and forced 8 (the halo-tiled kernel's varlen form, fused tail
included); the register-staged family 1 has no varlen form, and forcing it is refused with a message (asserted here).

Measured on the MI355X (worst entry): see the table in DESIGN.md section 3.
"""
import ctypes as C

import numpy as np
import pytest

from test_decode_tokens_gpu import TOL, DEFAULT

pytestmark = pytest.mark.gpu

ROUTE_TOL = 1e-4
CASES = ["dptv_tiny_b4_edges", "decv_tiny_b3_win_sharp"]
VARIANTS = [0, 2, 4, 8]


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    yield gpu_checks
    gpu_checks.drop_models()


def _err(got, want):
    from helpers import rel_l2, max_rel
    return max(rel_l2(got, want), max_rel(got, want))


_cache = {}


def _entries(G, case, prec):
    """-> (m, g, meta, [(tag, b, (h, w), feat [n, E], [three hooks [n, D]])]) in pack order: side a of every entry, then side b.
    hooks=True frontend: the forced families need the test-hooks library."""
    import torch
    from helpers import load_golden
    g, meta = load_golden(case)
    m = G.model("tiny", float(meta["qk_gain"]), prec, seed=int(meta["seed"]), hooks=True)
    G.set_variant(m, 0)
    key = (case, prec)
    if key not in _cache:
        _cache.clear()
        B = int(meta["B"])
        fa = [torch.from_numpy(g[f"feat_a_e{b}"]).cuda() for b in range(B)]
        fb = [torch.from_numpy(g[f"feat_b_e{b}"]).cuda() for b in range(B)]
        pa = [torch.from_numpy(g[f"pos_a_e{b}"]) for b in range(B)]
        pb = [torch.from_numpy(g[f"pos_b_e{b}"]) for b in range(B)]
        d1, d2 = m.decode_stereo_varlen(fa, fb, pa, pb, layers=sorted({hk - 1 for hk in m.cfg.hooks[1:]}))
        torch.cuda.synchronize()
        ents = []
        for tag, feats, d in (("a", fa, d1), ("b", fb, d2)):
            for b in range(B):
                h, w = (int(v) for v in g[f"rect_{tag}"][b])
                assert h > 0
                ents.append((tag, b, (h, w), feats[b], [d[hk - 1][b][1:, :] for hk in m.cfg.hooks[1:]]))
        _cache[key] = ents
    return m, g, meta, _cache[key]


def _run(m, ents, **kw):
    import torch
    out = m.head_pts_varlen([e[3] for e in ents], [[e[4][j] for e in ents] for j in range(3)], [e[2] for e in ents], **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", CASES)
def test_head_pts_varlen_vs_reference_golden_and_per_entry_route(G, case, prec, variant):
    """Every side of the fixture in ONE call: points and confidence against the reference's head_pts on that side alone (TOL, range
    report (0, 0)), and against OUR head_pts on it alone (ROUTE_TOL); shapes and the transposed views for h > w as head_pts returns."""
    import torch
    m, g, meta, ents = _entries(G, case, prec)
    sub = int(meta["sub"])
    m.range_report(reset=True)
    G.set_variant(m, variant)
    try:
        got = _run(m, ents)
        rng = tuple(m.range_report(reset=True))
        errs, route = {}, {}
        for (tag, b, (h, w), feat, hooks), o in zip(ents, got):
            toks = [None] * (m.cfg.dec_depth + 2)
            toks[m.cfg.hooks[0]] = feat[None]
            for hk, t in zip(m.cfg.hooks[1:], hooks):
                toks[hk] = t[None]
            one = m.head_pts(toks, [[16 * h, 16 * w]])
            torch.cuda.synchronize()
            for key in ("pts3d", "conf"):
                assert o[key].shape == one[key].shape and o[key].stride()[1:] == one[key].stride()[1:], (tag, b, key, o[key].shape, one[key].shape)
                # (h > w: the fixture records the reference wrapper's transposed view, which is what head_pts_varlen returns)
                errs[f"{tag}_{key}_e{b}"] = _err(o[key].cpu().numpy()[0, ::sub, ::sub], g[f"{tag}_{key}_e{b}"])
                route[f"{tag}_{key}_e{b}"] = _err(o[key].cpu().numpy(), one[key].cpu().numpy())
    finally:
        G.set_variant(m, 0)
    worst, rworst = max(errs, key=errs.get), max(route, key=route.get)
    print(case, prec, "variant", variant, "vs fixture", worst, f"{errs[worst]:.2e}", "vs head_pts per entry", rworst, f"{route[rworst]:.2e}", "range", rng)
    assert not {k: v for k, v in errs.items() if not v < TOL}, errs
    assert not {k: v for k, v in route.items() if not v < ROUTE_TOL}, route
    assert rng == (0, 0), rng


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_permuting_the_entries_is_bit_identical(G, prec):
    """The multiset of shapes is the same, so every launch has the same plan: an entry's result does not depend on its place."""
    import torch
    m, g, meta, ents = _entries(G, "dptv_tiny_b4_edges", prec)
    base = _run(m, ents)
    for perm in ((3, 0, 7, 1, 6, 2, 5, 4), (7, 6, 5, 4, 3, 2, 1, 0)):
        got = _run(m, [ents[i] for i in perm])
        for j, i in enumerate(perm):
            for key in ("pts3d", "conf"):
                assert torch.equal(got[j][key], base[i][key]), (perm, j, i, key)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_an_entry_does_not_see_its_neighbours(G, prec):
    """Replacing the inputs of every OTHER entry (same shapes: the same plans) leaves an entry bit-identical - the exact test of halo,
    tap and tile isolation.  The replacement is large (x 3, sign flipped) so that a single foreign tap would show."""
    import torch
    m, g, meta, ents = _entries(G, "dptv_tiny_b4_edges", prec)
    base = _run(m, ents)
    for keep in range(len(ents)):
        other = [e if i == keep else (e[0], e[1], e[2], -3.0 * e[3].flip(0), [-3.0 * t.flip(0) for t in e[4]]) for i, e in enumerate(ents)]
        got = _run(m, other)
        for key in ("pts3d", "conf"):
            assert torch.equal(got[keep][key], base[keep][key]), (keep, ents[keep][2], key)
            assert not torch.equal(got[(keep + 1) % len(ents)][key], base[(keep + 1) % len(ents)][key])          # (the replacement did change the others)
    m.range_report(reset=True)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_row_tables_and_output_offsets(G, prec):
    """In place through enc_row / hook_row on the packed decoder layout == the same inputs copied out contiguously, bit for bit;
    out_pix with gaps (and in another order) writes the same values and leaves the gaps' guard pattern untouched."""
    import torch
    m, g, meta, ents = _entries(G, "dptv_tiny_b4_edges", prec)
    # the hooks of one side are views of ONE packed buffer, a pose row in front of each entry: read in place
    tabs = m._row_table([e[4][0] for e in ents], m.cfg.dec_embed_dim)
    assert isinstance(tabs[0], list) and tabs[2][0] == 0 and tabs[2][1] == ents[0][2][0] * ents[0][2][1] + 1, tabs[2]
    base = _run(m, ents)
    copied = [(e[0], e[1], e[2], e[3].clone(), [t.clone() for t in e[4]]) for e in ents]
    got = _run(m, copied)
    for a, b in zip(base, got):
        assert torch.equal(a["pts3d"], b["pts3d"]) and torch.equal(a["conf"], b["conf"])
    npix = [256 * e[2][0] * e[2][1] for e in ents]
    gap = 37
    order = [5, 0, 3, 7, 1, 2, 6, 4]                   # where each entry goes: a permutation, gaps between the ranges
    offs, at = [0] * len(ents), gap
    for i in order:
        offs[i] = at
        at += npix[i] + gap
    pts = torch.full((at, 3), -7.5, device="cuda")
    conf = torch.full((at,), -7.5, device="cuda")
    got = _run(m, ents, out_pix=offs, out=(pts, conf))
    mask = torch.ones(at, dtype=torch.bool, device="cuda")
    for i, o in enumerate(got):
        assert o["pts3d"].data_ptr() == pts.data_ptr() + 12 * offs[i]
        assert torch.equal(o["pts3d"], base[i]["pts3d"]) and torch.equal(o["conf"], base[i]["conf"]), i
        mask[offs[i]:offs[i] + npix[i]] = False
    assert int(mask.sum()) == gap * (len(ents) + 1)
    assert bool((pts[mask] == -7.5).all()) and bool((conf[mask] == -7.5).all()), "a gap between the entries' output ranges was written"


def test_refusals(G):
    """Every refusal of the call, each with its message."""
    import torch
    from vista_slam_amd import _lib
    m, g, meta, ents = _entries(G, "dptv_tiny_b4_edges", DEFAULT)
    E, D = m.cfg.enc_embed_dim, m.cfg.dec_embed_dim
    enc = torch.zeros(64, E, device="cuda")
    hk = [torch.zeros(64, D, device="cuda") for _ in range(3)]
    pts, conf = torch.zeros(64 * 256, 3, device="cuda"), torch.zeros(64 * 256, device="cuda")
    I64, I32 = (C.c_int64 * 2), (C.c_int * 2)

    def call(enc_p=None, rows=(0, 4), hp=(2, 2), wp=(2, 3), B=2, pts_p=None, hooks=None, hp_arr=True, big=None):
        hooks = hooks or [t.data_ptr() for t in hk]
        if big:
            n = big
            return m.lib.sta_head_pts_varlen(m._h, enc.data_ptr(), (C.c_int64 * n)(*([0] * n)), *hooks, (C.c_int64 * n)(*([0] * n)),
                                             (C.c_int * n)(*([1] * n)), (C.c_int * n)(*([1] * n)), n, pts.data_ptr(), conf.data_ptr(), None, G.st())
        return m.lib.sta_head_pts_varlen(m._h, enc.data_ptr() if enc_p is None else enc_p, I64(*rows), *hooks, I64(*rows),
                                         I32(*hp) if hp_arr else None, I32(*wp), B, pts.data_ptr() if pts_p is None else pts_p, conf.data_ptr(), None, G.st())

    def refused(rc, text):
        assert rc == -1
        msg = m.lib.sta_last_error().decode()
        assert text in msg, (text, msg)

    assert call() == 0
    refused(call(enc_p=0), "null device pointer")
    refused(call(pts_p=0), "null device pointer")
    refused(call(hooks=[hk[0].data_ptr(), 0, hk[2].data_ptr()]), "null device pointer")
    refused(call(hp_arr=False), "null host array")
    refused(call(B=0), "takes 1 .. 32 entries")
    refused(call(big=33), "takes 1 .. 32 entries")
    refused(call(hp=(2, 0)), "at least one row and one column")
    refused(call(wp=(-1, 3)), "at least one row and one column")
    refused(call(hp=(1 << 15, 2), wp=(1 << 15, 3)), "too many rows")          # 2^30 patches: 2^32 pixels at 2x already
    refused(call(enc_p=enc.data_ptr() + 4), "misaligned features")
    refused(call(hooks=[hk[0].data_ptr(), hk[1].data_ptr() + 8, hk[2].data_ptr()]), "misaligned features")
    m.set_precision("f16")
    try:
        refused(call(), "no precision-f16 form")
    finally:
        m.set_precision(DEFAULT)
    # the register-staged family has no varlen form: forcing it is refused, not ignored
    G.set_variant(m, 1)
    try:
        refused(call(), "has no varlen form")
    finally:
        G.set_variant(m, 0)
    torch.cuda.synchronize()
    m.range_report(reset=True)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", ["decv_tiny_b3_win_sharp", "dptv_tiny_b4_edges", "decv_full_224_b2"])
def test_forward_pairs_tokens_with_the_varlen_head(G, case, prec):
    """forward_pairs_tokens(heads="varlen"): every rectangular side of both sides through one head call - against the fixture at the
    bars of the existing test (TOL), and at most ROUTE_TOL from heads="entry"."""
    import torch
    from helpers import load_golden
    from vista_slam_amd import weights as W
    g, meta = load_golden(case)
    full = case == "decv_full_224_b2"
    if full:
        G.drop_models()
        _cache.clear()
    m = G.model("full" if full else "tiny", float(meta["qk_gain"]), prec, seed=int(meta["seed"]))
    B, seed, sub = int(meta["B"]), int(meta["seed"]), int(meta["sub"])
    imgs = [[torch.from_numpy(W.synth_images(1, int(g[f"hw_{tag}"][b][0]), int(g[f"hw_{tag}"][b][1]), seed=seed, tag=2 * b + t))[0].cuda()
             for b in range(B)] for t, tag in enumerate("ab")]
    pos = [[torch.from_numpy(g[f"pos_{tag}_e{b}"]) for b in range(B)] for tag in "ab"]
    m.range_report(reset=True)
    res = {hd: m.forward_pairs_tokens(imgs[0], imgs[1], pos[0], pos[1], encode="varlen", heads=hd) for hd in ("entry", "varlen")}
    torch.cuda.synchronize()
    rng = tuple(m.range_report(reset=True))
    errs, route = {}, {}
    for t, tag in enumerate("ab"):
        for b in range(B):
            h, w = (int(v) for v in g[f"rect_{tag}"][b])
            ov, oe = res["varlen"][t][b], res["entry"][t][b]
            assert _err(ov["relative_pose"].cpu().numpy(), oe["relative_pose"].cpu().numpy()) < ROUTE_TOL
            if not h:
                assert ov["pts3d_pred"] is None and ov["conf"] is None and oe["pts3d_pred"] is None
                continue
            for key, gk in (("pts3d_pred", "pts3d"), ("conf", "conf")):
                assert ov[key].shape == oe[key].shape, (tag, b, key)
                errs[f"{tag}_{gk}_e{b}"] = _err(ov[key].cpu().numpy()[::sub, ::sub], g[f"{tag}_{gk}_e{b}"])
                route[f"{tag}_{gk}_e{b}"] = _err(ov[key].cpu().numpy(), oe[key].cpu().numpy())
    worst, rworst = max(errs, key=errs.get), max(route, key=route.get)
    print(case, prec, "vs fixture", worst, f"{errs[worst]:.2e}", "varlen vs entry", rworst, f"{route[rworst]:.2e}", "range", rng)
    assert not {k: v for k, v in errs.items() if not v < TOL}, errs
    assert not {k: v for k, v in route.items() if not v < ROUTE_TOL}, route
    assert rng == (0, 0), rng
    if full:
        G.drop_models()
