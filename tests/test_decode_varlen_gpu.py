"""GPU: the decoder on batches whose ENTRIES have their own token counts (sta_decode_varlen through STAFrontend.decode_stereo_varlen /
forward_pairs_tokens) against the reference fixtures `decv_*` (tools/gen_golden_decv.py: every entry is the reference's
`_decode_stereo` on that entry alone at B = 1), the new route against sta_decode_tokens, and the rotation kernel's varlen form alone
(sta_debug_rope_varlen).

Bounds, as tests/test_decode_tokens_gpu.py: the project's bar TOL = 1e-3 for everything compared with a reference fixture (rel-L2
AND max norm, range report (0, 0)); ROUTE_TOL = 0.1 x TOL route against route, for the swap and for permuted entries.  What makes
passing mean something: `alt_padded` of every fixture (tests/test_decode_varlen_cpu.py) - zero-padding an entry to the call's largest
count moves its answer by 0.2 .. 1.1, two hundred times the bar -, and the neighbour classes of decv_tiny_b4_edges (both pose modes,
64-key tile boundaries from both sides, one token, the last count that prefetches, all in one launch).

The rotation kernel alone, on inputs k * 2^-8 (|k| <= 1024: exact in an fp16 plane) and positions in [-1, 40]: against the fp64
rotation at the bound (b) of tests/test_decode_tokens_gpu.py, (pos_max + 2) 2^-21 (|v0| + |v1|) per element; rows past a sequence's
pose token and the guard block behind the buffers come back bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from test_decode_tokens_gpu import TOL, ROUTE_TOL, DEFAULT, POS_MAX, _pair_mag

pytestmark = pytest.mark.gpu

TINY = ["decv_tiny_b4_edges", "decv_tiny_b3_win_sharp", "decv_tiny_b2_equal"]
FULL = "decv_full_224_b2"


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    yield gpu_checks
    gpu_checks.drop_models()


def _err(got, want):
    from helpers import rel_l2, max_rel
    return max(rel_l2(got, want), max_rel(got, want))


def _setup(G, case, prec):
    from helpers import load_golden
    g, meta = load_golden(case)
    full = case == FULL
    if full:
        G.drop_models()
    m = G.model("full" if full else "tiny", float(meta["qk_gain"]), prec, seed=int(meta["seed"]))
    return g, meta, m


def _inputs(m, g, meta):
    """Per entry features and positions of both sides: the fixture's own features (tiny), or our encoder on the recorded subsets
    of the procedural frames (full: the fixture holds no features)."""
    import torch
    from vista_slam_amd import weights as W
    B, seed = int(meta["B"]), int(meta["seed"])
    sides = []
    for t, tag in enumerate("ab"):
        feats, poss = [], []
        for b in range(B):
            pos = torch.from_numpy(g[f"pos_{tag}_e{b}"])
            if f"feat_{tag}_e{b}" in g:
                f = torch.from_numpy(g[f"feat_{tag}_e{b}"]).cuda()
            else:
                H, Wd = (int(v) for v in g[f"hw_{tag}"][b])
                img = torch.from_numpy(W.synth_images(1, H, Wd, seed=seed, tag=2 * b + t)).cuda()
                f = m.encode_tokens(img, pos=pos[None])[0][0]
            feats.append(f)
            poss.append(pos if (b + t) % 2 else pos.cuda())          # some on the CPU, some on the device
        sides.append((feats, poss))
    return sides


def _vs_fixture(m, g, meta, sides, d1, d2, with_heads=True):
    """{name: error} of every hook layer of every entry of both sides, the pose head over all pose rows, the DPT head per rectangle."""
    import torch
    cfg, B, tsub, sub = m.cfg, int(meta["B"]), int(meta["tsub"]), int(meta["sub"])
    errs = {}
    for hk in cfg.hooks[1:]:
        for t, d in enumerate((d1, d2)):
            for b in range(B):
                want = g[f"dec{t + 1}_hook{hk - 1}_e{b}"]
                got = d[hk - 1][b].cpu().numpy()
                assert got.shape[0] == int(g["n1" if t == 0 else "n2"][b]) + 1
                errs[f"dec{t + 1}_hook{hk - 1}_e{b}"] = _err(got[::tsub], want)
    if not with_heads:
        return errs
    for t, (tag, d) in enumerate(zip("ab", (d1, d2))):
        pose = m.head_pose_s(torch.stack([x[0] for x in d[-1]]))
        errs[f"{tag}_pose"] = _err(pose["pose"].cpu().numpy(), g[f"{tag}_pose"])
        errs[f"{tag}_pose_conf"] = _err(pose["conf"].cpu().numpy(), g[f"{tag}_pose_conf"])
        for b in range(B):
            h, w = (int(v) for v in g[f"rect_{tag}"][b])
            assert (f"{tag}_pts3d_e{b}" in g) == (h > 0)
            if h:
                toks = [sides[t][0][b][None]] + [None if x is None else x[b][None, 1:, :] for x in d]
                pts = m.head_pts(toks, [[16 * h, 16 * w]])
                for key in ("pts3d", "conf"):
                    errs[f"{tag}_{key}_e{b}"] = _err(pts[key].cpu().numpy()[0, ::sub, ::sub], g[f"{tag}_{key}_e{b}"])
    return errs


def _check_case(G, case, prec):
    import torch
    g, meta, m = _setup(G, case, prec)
    m.range_report(reset=True)
    sides = _inputs(m, g, meta)
    d1, d2 = m.decode_stereo_varlen(sides[0][0], sides[1][0], sides[0][1], sides[1][1])
    torch.cuda.synchronize()
    assert all(x is not None and len(x) == int(meta["B"]) for x in d1 + d2)
    errs = _vs_fixture(m, g, meta, sides, d1, d2)
    rng = tuple(m.range_report(reset=True))
    worst = max(errs, key=errs.get)
    print(case, prec, "worst", worst, f"{errs[worst]:.2e}", {k: f"{v:.2e}" for k, v in errs.items() if "hook" not in k},
          "ref_noise", float(g["ref_noise"]), "range", rng)
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad
    assert rng == (0, 0), rng
    return g, meta, m, sides, d1, d2


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", TINY)
def test_decode_stereo_varlen_vs_reference_golden(G, case, prec):
    """Every hook layer of every entry of both sides (pose row included), pose and pose confidence over all pose rows, points and
    confidence of every rectangular side; `layers=` restricts what is materialised."""
    import torch
    g, meta, m, sides, d1, d2 = _check_case(G, case, prec)
    last = m.cfg.hooks[-1] - 1
    e1, e2 = m.decode_stereo_varlen(sides[0][0], sides[1][0], sides[0][1], sides[1][1], layers=[last])
    assert [x is not None for x in e1] == [i == last for i in range(len(e1))] == [x is not None for x in e2]
    for b in range(int(meta["B"])):
        assert torch.equal(e1[last][b], d1[last][b]) and torch.equal(e2[last][b], d2[last][b])
    # the views of one layer share one packed buffer, entry after entry
    base = e1[last][0].data_ptr()
    assert [x.data_ptr() - base for x in e1[last]] == [4 * m.cfg.dec_embed_dim * o for o in m.varlen_offsets(g["n1"].tolist())[0]]


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_decode_stereo_varlen_full_vs_reference_golden(G, prec):
    """Full architecture, counts (196, 80) / (140, 196): a whole frame against a pruned set and a window against a whole frame in one
    call.  The features are our encoder's on the recorded subsets (sta_encode_tokens), so its error is inside the figures."""
    _check_case(G, FULL, prec)


def _layers_diff(cfg, got, want):
    """Worst error over the hook layers of lists of per-entry tensors (both sides)."""
    return max(_err(a.cpu().numpy(), b.cpu().numpy()) for hk in cfg.hooks[1:] for a, b in zip(got[hk - 1], want[hk - 1]))


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", TINY)
def test_every_entry_against_a_b1_tokens_call(G, case, prec):
    """Entry b of the varlen call against sta_decode_tokens at B = 1 on the same inputs, every hook layer of both sides; and the swap
    decode(b, a) against decode(a, b).  Measured: the swap is bit-identical (0.0) in both precisions."""
    import torch
    g, meta, m = _setup(G, case, prec)
    sides = _inputs(m, g, meta)
    (fa, pa), (fb, pb) = sides
    d1, d2 = m.decode_stereo_varlen(fa, fb, pa, pb)
    s1, s2 = m.decode_stereo_varlen(fb, fa, pb, pa)
    worst = 0.0
    for b in range(int(meta["B"])):
        o1, o2 = m.decode_stereo_tokens(fa[b][None], fb[b][None], pa[b][None], pb[b][None])
        torch.cuda.synchronize()
        for hk in m.cfg.hooks[1:]:
            worst = max(worst, _err(d1[hk - 1][b].cpu().numpy(), o1[hk - 1][0].cpu().numpy()), _err(d2[hk - 1][b].cpu().numpy(), o2[hk - 1][0].cpu().numpy()))
    swap = max(_layers_diff(m.cfg, s1, d2), _layers_diff(m.cfg, s2, d1))
    print(case, prec, "varlen vs B = 1 tokens calls", worst, "swap", swap)
    assert worst < ROUTE_TOL, worst
    assert swap < ROUTE_TOL, swap
    assert tuple(m.range_report(reset=True)) == (0, 0)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_equal_counts_against_one_b2_tokens_call(G, prec):
    """decv_tiny_b2_equal, counts (12, 12) / (15, 15): one varlen call against ONE B = 2 sta_decode_tokens call."""
    import torch
    g, meta, m = _setup(G, "decv_tiny_b2_equal", prec)
    (fa, pa), (fb, pb) = _inputs(m, g, meta)
    d1, d2 = m.decode_stereo_varlen(fa, fb, pa, pb)
    o1, o2 = m.decode_stereo_tokens(torch.stack(fa), torch.stack(fb), torch.stack([p.cuda() for p in pa]), torch.stack([p.cuda() for p in pb]))
    torch.cuda.synchronize()
    worst = max(_err(torch.stack(d[hk - 1]).cpu().numpy(), o[hk - 1].cpu().numpy()) for hk in m.cfg.hooks[1:] for d, o in ((d1, o1), (d2, o2)))
    print("decv_tiny_b2_equal", prec, "varlen vs one B = 2 tokens call", worst)
    assert worst < ROUTE_TOL, worst


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_permuting_the_entries_permutes_the_outputs(G, prec):
    """decv_tiny_b4_edges in the orders (2, 0, 3, 1) and (3, 2, 1, 0), and entry 2 alone with entry 0 twice: an entry's result does
    not depend on its neighbours or on its place in the batch."""
    import torch
    g, meta, m = _setup(G, "decv_tiny_b4_edges", prec)
    (fa, pa), (fb, pb) = _inputs(m, g, meta)
    d1, d2 = m.decode_stereo_varlen(fa, fb, pa, pb)
    worst = 0.0
    for perm in ((2, 0, 3, 1), (3, 2, 1, 0), (0, 2, 0)):
        def pick(x):
            return [x[i] for i in perm]
        q1, q2 = m.decode_stereo_varlen(pick(fa), pick(fb), pick(pa), pick(pb))
        torch.cuda.synchronize()
        for hk in m.cfg.hooks[1:]:
            for j, i in enumerate(perm):
                worst = max(worst, _err(q1[hk - 1][j].cpu().numpy(), d1[hk - 1][i].cpu().numpy()), _err(q2[hk - 1][j].cpu().numpy(), d2[hk - 1][i].cpu().numpy()))
    print("decv_tiny_b4_edges", prec, "permuted entries", worst)
    assert worst < ROUTE_TOL, worst


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_forward_pairs_tokens_vs_reference_golden(G, prec):
    """decv_tiny_b3_win_sharp end to end: encode_tokens per entry (three different windows of one frame size against three frame
    sizes), one varlen decode, the pose head over all six pose rows, the DPT head per entry and side (every side is a rectangle)."""
    import torch
    from vista_slam_amd import weights as W
    case = "decv_tiny_b3_win_sharp"
    g, meta, m = _setup(G, case, prec)
    m.range_report(reset=True)
    B, seed, sub = int(meta["B"]), int(meta["seed"]), int(meta["sub"])
    imgs = [[torch.from_numpy(W.synth_images(1, int(g[f"hw_{tag}"][b][0]), int(g[f"hw_{tag}"][b][1]), seed=seed, tag=2 * b + t))[0].cuda()
             for b in range(B)] for t, tag in enumerate("ab")]
    pos = [[torch.from_numpy(g[f"pos_{tag}_e{b}"]) for b in range(B)] for tag in "ab"]
    res = m.forward_pairs_tokens(imgs[0], imgs[1], pos[0], pos[1])
    torch.cuda.synchronize()
    errs = {}
    for tag, side in zip("ab", res):
        assert len(side) == B
        for b, r in enumerate(side):
            h, w = (int(v) for v in g[f"rect_{tag}"][b])
            assert tuple(r["pts3d_pred"].shape) == (16 * h, 16 * w, 3) and tuple(r["conf"].shape) == (16 * h, 16 * w)
            errs[f"{tag}_pts3d_e{b}"] = _err(r["pts3d_pred"].cpu().numpy()[::sub, ::sub], g[f"{tag}_pts3d_e{b}"])
            errs[f"{tag}_conf_e{b}"] = _err(r["conf"].cpu().numpy()[::sub, ::sub], g[f"{tag}_conf_e{b}"])
            errs[f"{tag}_pose_e{b}"] = _err(r["relative_pose"].cpu().numpy(), g[f"{tag}_pose"][b])
            errs[f"{tag}_pose_conf_e{b}"] = _err(r["relative_pose_conf"].cpu().numpy(), g[f"{tag}_pose_conf"][b])
    rng = tuple(m.range_report(reset=True))
    print(case, prec, {k: f"{v:.2e}" for k, v in errs.items()}, "range", rng)
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad
    assert rng == (0, 0), rng


# ------------------------------------------------------------------------------------------ the rotation kernel alone
ROPE_COUNTS = [(2, [6, 12, 1]), (2, [63, 64, 1, 65]), (3, [67, 13]), (1, [1]), (2, [129, 5, 64, 127, 2, 200])]      # (heads, tokens per sequence)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("nbuf", [1, 3])
@pytest.mark.parametrize("shape", ROPE_COUNTS, ids=[f"h{h}_" + "_".join(map(str, n)) for h, n in ROPE_COUNTS])
def test_rope_varlen_kernel_alone(G, shape, nbuf, prec):
    import torch
    from vista_slam_amd import _lib
    heads, n = shape
    S = len(n)
    rs = np.random.default_rng(11 + sum(n))
    npad = (max(n) + 1 + 63) // 64 * 64
    bufs = [(rs.integers(-1024, 1025, size=(S * heads + 1, npad, 64)) * 2.0 ** -8).astype(np.float32) for _ in range(nbuf)]
    pos = [rs.integers(-1, POS_MAX + 1, size=(k, 2)).astype(np.int32) for k in n]
    m, lib, h = G.kernel_handle(prec)
    dev = [G.dev(b) for b in bufs]
    table = G.dev(np.concatenate([p.ravel() for p in pos]))
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in dev])
    _lib.check(lib.sta_debug_rope_varlen(h, ptrs, nbuf, S, heads, (C.c_int * S)(*n), table.data_ptr(), POS_MAX, G.st()))
    torch.cuda.synchronize()
    new = [t.cpu().numpy() for t in dev]
    inv = 100.0 ** (-np.arange(16, dtype=np.float64) / 16.0)
    worst = 0.0
    for b in range(nbuf):
        live = np.zeros(bufs[b].shape, bool)
        ref = bufs[b].astype(np.float64)
        for s in range(S):
            rows = slice(s * heads, (s + 1) * heads)
            live[rows, :n[s] + 1] = True
            p = np.concatenate([pos[s].astype(np.float64), [[-1.0, -1.0]]], 0)
            for xy in range(2):
                ang = p[:, xy, None] * inv[None, :]
                c, sn = np.cos(ang)[None], np.sin(ang)[None]
                v0 = bufs[b][rows, :n[s] + 1, xy * 32:xy * 32 + 16].astype(np.float64)
                v1 = bufs[b][rows, :n[s] + 1, xy * 32 + 16:xy * 32 + 32].astype(np.float64)
                ref[rows, :n[s] + 1, xy * 32:xy * 32 + 16] = v0 * c - v1 * sn
                ref[rows, :n[s] + 1, xy * 32 + 16:xy * 32 + 32] = v1 * c + v0 * sn
        assert not live[S * heads].any()          # the guard block
        # rows past a sequence's pose token and the guard block: bit for bit what went in
        assert np.array_equal(new[b][~live].view(np.uint32), bufs[b][~live].view(np.uint32)), ("dead rows written", b, np.argwhere((new[b] != bufs[b]) & ~live)[:4])
        assert np.isfinite(new[b]).all()
        bound = (POS_MAX + 2) * 2.0 ** -21 * _pair_mag(bufs[b][None], np.add)[0]
        err = np.abs(new[b].astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300))[live & (bound > 0)].max()))
        assert (err <= bound)[live].all(), ("vs fp64 rotation", b, np.argwhere((err > bound) & live)[:4])
        assert not np.array_equal(new[b][live], bufs[b][live])          # it did rotate
    print(shape, nbuf, prec, "vs fp64, fraction of bound", worst)


# ------------------------------------------------------------------------------------------ refusals
def test_varlen_refusals(G):
    """The shim refuses float positions, positions below -1, mismatched lists and more than 16 entries; the C entry bad arguments
    with status -1 and a message."""
    import torch
    g, meta, m = _setup(G, "decv_tiny_b2_equal", DEFAULT)
    (fa, pa), (fb, pb) = _inputs(m, g, meta)
    with pytest.raises(AssertionError, match="integer"):
        m.decode_stereo_varlen(fa, fb, [p.float() for p in pa], pb)
    with pytest.raises(ValueError, match="below -1"):
        m.decode_stereo_varlen(fa, fb, [p - 3 for p in pa], pb)
    with pytest.raises(AssertionError, match="same number of entries"):
        m.decode_stereo_varlen(fa, fb[:1], pa, pb[:1])
    with pytest.raises(AssertionError, match="1 .. 16 entries"):
        m.decode_stereo_varlen(fa * 9, fb * 9, pa * 9, pb * 9)
    with pytest.raises(AssertionError, match="positions must be"):
        m.decode_stereo_varlen(fa, fb, [pa[0][:5], pa[1]], pb)
    f1, q1, n1 = m.pack_varlen(fa, pa, m.cfg.enc_embed_dim, m.device)
    f2, q2, n2 = m.pack_varlen(fb, pb, m.cfg.enc_embed_dim, m.device)
    L = m.cfg.dec_depth + 1
    nul = (C.c_void_p * L)()
    ok1, ok2 = (C.c_int * 2)(*n1), (C.c_int * 2)(*n2)
    zero = (C.c_int * 2)(n1[0], 0)
    big = (C.c_int * 2)(2 ** 30, 2 ** 30)
    for args in ((None, f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), ok1, ok2, 2, 4),                     # null features
                 (f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), None, ok1, ok2, 2, 4),                     # null positions
                 (f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), None, ok2, 2, 4),           # null counts
                 (f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), zero, ok2, 2, 4),           # a count below 1
                 (f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), ok1, ok2, 0, 4),            # B out of range
                 (f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), ok1, ok2, 17, 4),
                 (f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), ok1, ok2, 2, 1 << 20),      # pos_max out of range
                 (f1.data_ptr(), f2.data_ptr(), q1.data_ptr(), q2.data_ptr(), big, ok2, 2, 4)):           # 2^31 or more decoder rows
        rc = m.lib.sta_decode_varlen(m._h, *args, nul, nul, m._stream())
        assert rc == -1 and len(m.lib.sta_last_error()) > 0, (args[6:], rc)
    d1, _ = m.decode_stereo_varlen(fa, fb, pa, pb, layers=[0])          # the handle still serves a good call
    torch.cuda.synchronize()
    assert d1[0][1].shape == (13, m.cfg.dec_embed_dim)
