"""GPU: the encoder on batches whose ENTRIES differ in token count and frame size (sta_encode_varlen[_u8hwc] through
STAFrontend.encode_tokens_varlen / encode_tokens_varlen_u8hwc / forward_pairs_tokens(encode="varlen")) - against the reference
fixtures `encv_*` (tools/gen_golden_encv.py: every entry is the reference on that entry alone at B = 1), route against route, exactness,
refusals, and its three new launches alone: the QKV finisher (sta_debug_qkv_finish_varlen), the encoder form of the per-sequence
attention (sta_debug_attn_encv) and the varlen gather (sta_debug_patch_gather_varlen).

Bounds are those of tests/test_encode_tokens_gpu.py: TOL = 1e-3 against a reference fixture (rel-L2 AND max norm, per entry, range
report (0, 0)); ROUTE_TOL = 0.1 x TOL route against route.  What makes passing mean something: `alt_padded` of every fixture
(tests/test_encode_varlen_cpu.py) - encoding an entry zero-padded to the call's largest count moves it by 0.088 .. 1.24 - and the counts
of encv_tiny_b8_edges (1, 65, 64, 128, 129, 63, 12, 256: packed rows start at multiples of neither 4, 8 nor 32; tile tails of 1 and 63).

The finisher alone, heads = 3, slab and bias k * 2^-8 in the q | k columns (their sum is exact in fp32 and as hi + lo), Gaussian floats in
the v columns, every output element poisoned with a sentinel on entry:
  (i)   V^T equals the hi / lo split of float32(slab + bias) bit for bit - there is no other arithmetic on that path;
  (ii)  Q / K against a float64 rotation by the exact angles at the bound of test_rope_rotation_of_buffers_without_a_pose_row,
        (POS_MAX + 2) 2^-21 (|v0| + |v1|) per element;
  (iii) rows [n_s, npad) of Q / K, columns [n_s, npad) of V^T and the guard block behind each buffer keep the sentinel bit for bit;
  (iv)  one value above 65504 raises counter 0 and is stored saturated.

The encoder form of the attention alone, heads = 2: the selection / uniform / Gaussian methods of tests/test_attention_varlen_exact.py
(its helpers, its bounds: the uniform bound 2^-20 max|V|, row bound 4 x the numpy model's worst row on the same inputs, whole-output
bound test_attention_exact.GLOBAL_TOL) on launches that mix the counts 1, 63, 64, 65, 128, 129, 256, 257: n_s == npad (a pose-key read
would hit the next head's row 0 - K rows and dead Q rows are poisoned), a one-row second query block, a one-key tail tile, the last
count that prefetches next to one that does not.  With nq == nk every selection map is a permutation: every key is selected by some
query - key 0, key n_s - 1, the first and last key of every tile.  Every test asserts the classes of all sequences and nan == 0.

Measured (MI355X; f16x3h / f16x3 alike unless noted; DESIGN.md section 3 keeps the table):
    worst entry vs golden 1.5e-6 (tiny), 9.4e-6 (tiny, gain 4), 3.9e-6 (full), 1.1e-5 (full, gain 3); range report (0, 0) everywhere
    entry vs encode_tokens alone 2.6e-7, vs the per-sequence-QKV route 2.6e-7, reversed entries 0.0; b3_equal vs one B = 3 call 2.2e-7
    u8hwc vs fp32 frames and repeated calls: bit-identical
    forward_pairs_tokens(encode="varlen") on decv_*: points 5.8e-5 / 5.2e-5, pose 3.9e-4 (gain 4); vs encode="grouped" 5.8e-5 / 2.6e-5
    finisher: V^T bit-identical, sentinel intact, Q / K <= 0.17 of the bound; attention: selection exact, worst Gaussian row 1.1e-6
    against a bound of 7.6e-6 (sharpness 3); gather: bit-identical to the equal-count form
"""
import ctypes as C

import numpy as np
import pytest

from test_attention_exact import GLOBAL_TOL
from test_encode_tokens_gpu import TOL, ROUTE_TOL, DEFAULT, POS_MAX, SENTINEL, _pair_sum

pytestmark = pytest.mark.gpu

PRECS = [DEFAULT, "f16x3"]
CASES = ["encv_tiny_b8_edges", "encv_tiny_b8_edges_sharp", "encv_tiny_b3_equal", "encv_full_224_b4", "encv_full_mixed_frames_sharp"]
EDGES = "encv_tiny_b8_edges"
DECV = ["decv_tiny_b4_edges", "decv_tiny_b3_win_sharp", "decv_tiny_b2_equal", "decv_full_224_b2"]


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    yield gpu_checks
    gpu_checks.drop_models()


def _err(got, want):
    from helpers import rel_l2, max_rel
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    want = want.cpu().numpy() if hasattr(want, "cpu") else want
    return max(rel_l2(got, want), max_rel(got, want))


def _setup(G, case, prec, hooks=False):
    from helpers import load_golden
    g, meta = load_golden(case)
    full = "_full_" in case
    if full:
        G.drop_models()
    m = G.model("full" if full else "tiny", float(meta["qk_gain"]), prec, seed=int(meta["seed"]), hooks=hooks)
    return g, meta, m


def _frames(g, meta, u8=False):
    """Entry b's frame: synth_images(1, H_b, W_b, seed, tag b) [3, H, W] (u8: the uint8 HWC frame whose ImgNorm is exactly that)."""
    import torch
    from vista_slam_amd import weights as W
    seed = int(meta["seed"])
    f = W.synth_images_u8 if u8 else W.synth_images
    return [torch.from_numpy(f(1, int(h), int(w), seed=seed, tag=b))[0].cuda() for b, (h, w) in enumerate(g["hw"])]


def _selection(g, B, key="pos"):
    import torch
    return [torch.from_numpy(g[f"{key}_e{b}"]) for b in range(B)]


# ------------------------------------------------------------------------------------------ against the reference fixtures
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CASES)
def test_encode_tokens_varlen_vs_reference_golden(G, case, prec):
    """Every entry of every fixture, given as positions (some on the CPU, some on the device) and as indices: rel-L2 and max norm per
    entry, so a wrong entry is named."""
    import torch
    g, meta, m = _setup(G, case, prec)
    B, tsub = int(meta["B"]), int(meta["tsub"])
    imgs = _frames(g, meta)
    pos = [p if b % 2 else p.cuda() for b, p in enumerate(_selection(g, B))]
    m.range_report(reset=True)
    feats, poss = m.encode_tokens_varlen(imgs, pos=pos)
    feats_i, poss_i = m.encode_tokens_varlen(imgs, index=_selection(g, B, "idx"))
    torch.cuda.synchronize()
    rng = tuple(m.range_report(reset=True))
    assert len(feats) == len(poss) == B
    errs = {}
    for b in range(B):
        n = int(g["n"][b])
        assert feats[b].shape == (n, m.cfg.enc_embed_dim) and poss[b].dtype == torch.int64 and poss[b].is_cuda
        assert np.array_equal(poss[b].cpu().numpy(), g[f"pos_e{b}"]) and np.array_equal(poss_i[b].cpu().numpy(), g[f"pos_e{b}"])
        assert torch.equal(feats[b], feats_i[b])
        errs[f"e{b}"] = _err(feats[b][::tsub], g[f"enc_feat_e{b}"])
    # the views share one packed buffer, entry after entry: what decode_stereo_varlen's packing expects
    base, offs = feats[0].data_ptr(), np.concatenate([[0], np.cumsum(g["n"])[:-1]])
    assert [f.data_ptr() - base for f in feats] == [4 * m.cfg.enc_embed_dim * int(o) for o in offs]
    print(case, prec, {k: f"{v:.2e}" for k, v in errs.items()}, "ref_noise", float(g["ref_noise"]), "range", rng)
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    assert rng == (0, 0), rng


# ------------------------------------------------------------------------------------------ route against route
@pytest.mark.parametrize("prec", PRECS)
def test_every_entry_against_the_other_routes(G, prec):
    """encv_tiny_b8_edges: entry b of the one call against (a) encode_tokens on entry b alone, (b) the per-sequence-QKV route
    (experiment switch 8: S fused-epilogue GEMMs + one no-pose rotation launch per layer), (c) a call with the entries reversed."""
    import torch
    from vista_slam_amd import _lib
    g, meta, m = _setup(G, EDGES, prec, hooks=True)
    B = int(meta["B"])
    imgs, pos = _frames(g, meta), _selection(g, B)
    m.range_report(reset=True)
    feats, _ = m.encode_tokens_varlen(imgs, pos=pos)
    _lib.check(m.lib.sta_debug_set_option(m._h, 8, 1))
    try:
        per_seq, _ = m.encode_tokens_varlen(imgs, pos=pos)
    finally:
        _lib.check(m.lib.sta_debug_set_option(m._h, 8, 0))
    rev, _ = m.encode_tokens_varlen(imgs[::-1], pos=pos[::-1])
    torch.cuda.synchronize()
    worst = {"alone": 0.0, "per_seq_qkv": 0.0, "reversed": 0.0}
    for b in range(B):
        alone, _ = m.encode_tokens(imgs[b][None], pos=pos[b][None])
        d = {"alone": _err(feats[b], alone[0]), "per_seq_qkv": _err(feats[b], per_seq[b]), "reversed": _err(feats[b], rev[B - 1 - b])}
        print(EDGES, prec, "entry", b, int(g["n"][b]), {k: f"{v:.2e}" for k, v in d.items()})
        for k in d:
            assert d[k] <= ROUTE_TOL, (b, k, d[k])
            worst[k] = max(worst[k], d[k])
    print(EDGES, prec, "worst", worst)
    assert tuple(m.range_report(reset=True)) == (0, 0)


@pytest.mark.parametrize("prec", PRECS)
def test_equal_entries_against_one_b3_tokens_call(G, prec):
    import torch
    g, meta, m = _setup(G, "encv_tiny_b3_equal", prec)
    imgs, pos = _frames(g, meta), _selection(g, 3)
    feats, _ = m.encode_tokens_varlen(imgs, pos=pos)
    one, _ = m.encode_tokens(torch.stack(imgs), pos=torch.stack(pos))
    torch.cuda.synchronize()
    d = _err(torch.stack(feats), one)
    print("encv_tiny_b3_equal", prec, "varlen vs one B = 3 tokens call", d)
    assert d <= ROUTE_TOL, d


# ------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("prec", PRECS)
def test_u8hwc_route_and_repeat_are_bit_identical(G, prec):
    import torch
    g, meta, m = _setup(G, EDGES, prec)
    B = int(meta["B"])
    pos = _selection(g, B)
    a, pa = m.encode_tokens_varlen(_frames(g, meta), pos=pos)
    b, pb = m.encode_tokens_varlen_u8hwc(_frames(g, meta, u8=True), pos=pos)
    c, _ = m.encode_tokens_varlen(_frames(g, meta), index=_selection(g, B, "idx"))
    d, _ = m.encode_tokens_varlen_u8hwc(_frames(g, meta, u8=True), pos=[p.cuda() for p in pos])
    torch.cuda.synchronize()
    for e in range(B):
        assert torch.equal(pa[e], pb[e])
        assert torch.equal(a[e], b[e]), (e, float((a[e] - b[e]).abs().max()))
        assert torch.equal(a[e], c[e]) and torch.equal(b[e], d[e]), e
        assert bool(torch.isfinite(a[e]).all()) and float(a[e].abs().max()) > 0


# ------------------------------------------------------------------------------------------ the pair route
def _pair_inputs(g, meta):
    import torch
    from vista_slam_amd import weights as W
    B, seed = int(meta["B"]), int(meta["seed"])
    imgs = [[torch.from_numpy(W.synth_images(1, int(g[f"hw_{tag}"][b][0]), int(g[f"hw_{tag}"][b][1]), seed=seed, tag=2 * b + t))[0].cuda()
             for b in range(B)] for t, tag in enumerate("ab")]
    pos = [[torch.from_numpy(g[f"pos_{tag}_e{b}"]) for b in range(B)] for tag in "ab"]
    return imgs, pos


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", DECV)
def test_forward_pairs_tokens_encode_varlen(G, case, prec):
    """forward_pairs_tokens(encode="varlen") on every decv_* fixture - all 2B frames in ONE encoder call - at the bounds
    tests/test_decode_varlen_gpu.py applies to the default route (pose, pose confidence, points and confidence of every rectangular
    side: TOL, range (0, 0)), and against encode="grouped" within ROUTE_TOL."""
    import torch
    g, meta, m = _setup(G, case, prec)
    B, sub = int(meta["B"]), int(meta["sub"])
    imgs, pos = _pair_inputs(g, meta)
    m.range_report(reset=True)
    res = m.forward_pairs_tokens(imgs[0], imgs[1], pos[0], pos[1], encode="varlen")
    torch.cuda.synchronize()
    rng = tuple(m.range_report(reset=True))
    old = m.forward_pairs_tokens(imgs[0], imgs[1], pos[0], pos[1])
    old2 = m.forward_pairs_tokens(imgs[0], imgs[1], pos[0], pos[1], encode="grouped")
    torch.cuda.synchronize()
    errs, route = {}, 0.0
    for tag, side, oside, o2side in zip("ab", res, old, old2):
        assert len(side) == B
        for b, (r, o, o2) in enumerate(zip(side, oside, o2side)):
            h, w = (int(v) for v in g[f"rect_{tag}"][b])
            assert (r["pts3d_pred"] is None) == (o["pts3d_pred"] is None) and (h == 0 or r["pts3d_pred"] is not None)      # (a lone token is a 1 x 1 rectangle the fixture does not record)
            if h:
                assert tuple(r["pts3d_pred"].shape) == (16 * h, 16 * w, 3) and tuple(r["conf"].shape) == (16 * h, 16 * w)
                errs[f"{tag}_pts3d_e{b}"] = _err(r["pts3d_pred"].cpu().numpy()[::sub, ::sub], g[f"{tag}_pts3d_e{b}"])
                errs[f"{tag}_conf_e{b}"] = _err(r["conf"].cpu().numpy()[::sub, ::sub], g[f"{tag}_conf_e{b}"])
            errs[f"{tag}_pose_e{b}"] = _err(r["relative_pose"], g[f"{tag}_pose"][b])
            errs[f"{tag}_pose_conf_e{b}"] = _err(r["relative_pose_conf"], g[f"{tag}_pose_conf"][b])
            for k in r:
                if r[k] is not None:
                    route = max(route, _err(r[k], o[k]))
                    assert torch.equal(o[k], o2[k]), (tag, b, k)          # the default IS the grouped route
    print(case, prec, {k: f"{v:.2e}" for k, v in errs.items()}, "varlen vs grouped", f"{route:.2e}", "range", rng)
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad
    assert route <= ROUTE_TOL, route
    assert rng == (0, 0), rng
    with pytest.raises(ValueError, match="encode must be"):
        m.forward_pairs_tokens(imgs[0], imgs[1], pos[0], pos[1], encode="padded")


# ------------------------------------------------------------------------------------------ refusals
def test_encode_varlen_refusals(G):
    """The shim refuses, before any launch: a count of 0, 33 entries, a frame size that is no multiple of 16, positions outside an
    entry's OWN grid (valid in its neighbour's larger one), mismatched list lengths, both or neither of pos / index; the C entry bad
    arguments with status -1 and a message.  A refused call leaves the handle as it was."""
    import torch
    g, meta, m = _setup(G, EDGES, DEFAULT)
    imgs, pos = _frames(g, meta)[5:8], _selection(g, 8)[5:8]          # frames 128x128 (8 x 8), 48x64 (3 x 4), 256x256 (16 x 16)
    feats, _ = m.encode_tokens_varlen(imgs, pos=pos)
    with pytest.raises(ValueError, match="entry 1: a token subset has at least one token"):
        m.encode_tokens_varlen(imgs, pos=[pos[0], pos[1][:0], pos[2]])
    with pytest.raises(ValueError, match="1 .. 32 entries"):
        m.encode_tokens_varlen([imgs[1]] * 33, pos=[pos[1]] * 33)
    with pytest.raises(AssertionError, match="multiple of patch size"):
        m.encode_tokens_varlen([imgs[0], imgs[1][:, :40], imgs[2]], pos=pos)
    bad = pos[1].clone(); bad[3] = torch.tensor([2, 7])               # (2, 7) lies in entry 0's 8 x 8 grid and in entry 2's, not in the 3 x 4 one
    with pytest.raises(ValueError, match="entry 1: positions outside the 3 x 4 patch grid"):
        m.encode_tokens_varlen(imgs, pos=[pos[0], bad, pos[2]])
    with pytest.raises(ValueError, match="entry 1: token index outside the 3 x 4 patch grid"):
        m.encode_tokens_varlen(imgs, index=[torch.arange(5), torch.tensor([0, 12]), torch.arange(5)])
    with pytest.raises(ValueError, match="one selection per frame"):
        m.encode_tokens_varlen(imgs, pos=pos[:2])
    with pytest.raises(ValueError, match="exactly one of pos"):
        m.encode_tokens_varlen(imgs)
    with pytest.raises(ValueError, match="exactly one of pos"):
        m.encode_tokens_varlen(imgs, pos=pos, index=pos)
    with pytest.raises(AssertionError, match="entry 0: positions must be int64"):
        m.encode_tokens_varlen(imgs, pos=[pos[0].float(), pos[1], pos[2]])
    with pytest.raises(AssertionError, match=r"a frame is \[3, H, W\]"):
        m.encode_tokens_varlen([imgs[0][None], imgs[1], imgs[2]], pos=pos)
    with pytest.raises(AssertionError, match="camera frame is uint8"):
        m.encode_tokens_varlen_u8hwc(imgs, pos=pos)
    q = torch.cat([p.cuda() for p in pos]).contiguous()
    out = torch.empty(q.shape[0], m.cfg.enc_embed_dim, device="cuda")
    n = [int(p.shape[0]) for p in pos]
    P, I = C.c_void_p * 3, C.c_int * 3
    ok = dict(imgs=P(*[x.data_ptr() for x in imgs]), H=I(128, 48, 256), W=I(128, 64, 256), pos=q.data_ptr(), n=I(*n), B=3, out=out.data_ptr())
    for change, what in ((dict(imgs=None), "null"), (dict(H=None), "null"), (dict(n=None), "null"), (dict(pos=None), "null device pointer"),
                         (dict(out=None), "null device pointer"), (dict(imgs=P(imgs[0].data_ptr(), None, imgs[2].data_ptr())), "frame of entry 1"),
                         (dict(n=I(n[0], 0, n[2])), "at least one token"), (dict(B=0), "out of range"), (dict(B=33), "out of range"),
                         (dict(H=I(128, 40, 256)), "multiple of patch size"), (dict(W=I(128, 64, 250)), "multiple of patch size"),
                         (dict(n=I(2 ** 30, 2 ** 30, 1)), "too many encoder rows")):
        a = dict(ok, **change)
        for entry in (m.lib.sta_encode_varlen, m.lib.sta_encode_varlen_u8hwc):
            rc = entry(m._h, a["imgs"], a["H"], a["W"], a["pos"], a["n"], a["B"], a["out"], m._stream())
            msg = m.lib.sta_last_error().decode()
            assert rc == -1 and what in msg, (change, rc, msg)
    again, _ = m.encode_tokens_varlen(imgs, pos=pos)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(again, feats))


# ------------------------------------------------------------------------------------------ the finisher alone
FIN_HEADS = 3
FIN_COUNTS = [[1, 65, 64, 7], [63, 128, 129, 1], [256, 12, 64], [5, 64, 1, 130, 63, 2]]


def _finish_run(G, prec, n, slab, bias, pos):
    import torch
    from vista_slam_amd import _lib
    S, npad = len(n), (max(n) + 63) // 64 * 64
    m, lib, h = G.kernel_handle(prec)
    shape_qk, shape_vt = (S * FIN_HEADS + 1, npad, 64), (S * FIN_HEADS + 1, 64, npad)          # the last block is the guard
    q, k, vt = (torch.full(s, float(SENTINEL), device="cuda") for s in (shape_qk, shape_qk, shape_vt))
    d_slab, d_bias, d_pos = G.dev(slab), None if bias is None else G.dev(bias), G.dev(pos.ravel())
    m.range_report(reset=True)
    _lib.check(lib.sta_debug_qkv_finish_varlen(h, d_slab.data_ptr(), None if d_bias is None else d_bias.data_ptr(), d_pos.data_ptr(),
                                               S, FIN_HEADS, (C.c_int * S)(*n), POS_MAX, q.data_ptr(), k.data_ptr(), vt.data_ptr(), G.st()))
    torch.cuda.synchronize()
    return q.cpu().numpy(), k.cpu().numpy(), vt.cpu().numpy(), tuple(m.range_report(reset=True)), npad


def _finish_inputs(n, seed):
    rs = np.random.default_rng(seed)
    M, E = sum(n), FIN_HEADS * 64
    slab = np.empty((M, 3 * E), np.float32)
    slab[:, :2 * E] = rs.integers(-1024, 1025, size=(M, 2 * E)) * 2.0 ** -8
    slab[:, 2 * E:] = rs.standard_normal((M, E)) * 3.0
    bias = np.empty(3 * E, np.float32)
    bias[:2 * E] = rs.integers(-1024, 1025, size=2 * E) * 2.0 ** -8
    bias[2 * E:] = rs.standard_normal(E)
    pos = rs.integers(0, POS_MAX + 1, size=(M, 2)).astype(np.int32)
    return slab, bias, pos


def _split(x):
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32) + lo.astype(np.float32)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("n", FIN_COUNTS, ids=["_".join(map(str, c)) for c in FIN_COUNTS])
def test_qkv_finisher_alone(G, n, with_bias, prec):
    S, E = len(n), FIN_HEADS * 64
    slab, bias, pos = _finish_inputs(n, 17 + sum(n))
    q, k, vt, rng, npad = _finish_run(G, prec, n, slab, bias if with_bias else None, pos)
    x = (slab + bias[None]).astype(np.float32) if with_bias else slab
    tok0 = np.concatenate([[0], np.cumsum(n)])
    sent = np.float32(SENTINEL).view(np.uint32)
    inv = 100.0 ** (-np.arange(16, dtype=np.float64) / 16.0)
    worst = 0.0
    for name, got, c0 in (("q", q, 0), ("k", k, E)):
        live = np.zeros(got.shape, bool)
        ref = np.zeros(got.shape, np.float64)
        src = np.zeros(got.shape, np.float32)
        for s in range(S):
            rows = slice(s * FIN_HEADS, (s + 1) * FIN_HEADS)
            live[rows, :n[s]] = True
            v = x[tok0[s]:tok0[s + 1], c0:c0 + E].reshape(n[s], FIN_HEADS, 64).transpose(1, 0, 2)          # [heads, n_s, 64]
            src[rows, :n[s]] = v
            for xy in range(2):
                ang = pos[tok0[s]:tok0[s + 1], xy, None].astype(np.float64) * inv[None, :]
                c, sn = np.cos(ang)[None], np.sin(ang)[None]
                v0, v1 = v[..., xy * 32:xy * 32 + 16].astype(np.float64), v[..., xy * 32 + 16:xy * 32 + 32].astype(np.float64)
                ref[rows, :n[s], xy * 32:xy * 32 + 16] = v0 * c - v1 * sn
                ref[rows, :n[s], xy * 32 + 16:xy * 32 + 32] = v1 * c + v0 * sn
        assert not live[S * FIN_HEADS].any()
        # (iii) rows [n_s, npad) of every (sequence, head) and the guard block: the sentinel, bit for bit
        assert (got[~live].view(np.uint32) == sent).all(), (name, "dead rows or the guard written", np.argwhere((got != SENTINEL) & ~live)[:4])
        assert np.isfinite(got).all()
        # (ii) against the fp64 rotation
        bound = (POS_MAX + 2) * 2.0 ** -21 * _pair_sum(src)
        err = np.abs(got.astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300))[live & (bound > 0)].max()))
        assert (err <= bound)[live].all(), (name, "vs fp64 rotation", np.argwhere((err > bound) & live)[:4])
        assert (got[live] != SENTINEL).any()
    # (i) V^T: the split of float32(slab + bias), bit for bit; (iii) columns [n_s, npad) and the guard keep the sentinel
    want = np.full(vt.shape, SENTINEL, np.float32)
    for s in range(S):
        v = x[tok0[s]:tok0[s + 1], 2 * E:].reshape(n[s], FIN_HEADS, 64).transpose(1, 2, 0)                 # [heads, 64, n_s]
        want[s * FIN_HEADS:(s + 1) * FIN_HEADS, :, :n[s]] = _split(v)
    assert np.array_equal(vt.view(np.uint32), want.view(np.uint32)), ("V^T", np.argwhere(vt.view(np.uint32) != want.view(np.uint32))[:4])
    print(n, with_bias, prec, "npad", npad, "Q / K vs fp64, fraction of bound", worst, "range", rng)
    assert rng == (0, 0), rng


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("where", ["q", "v"])
def test_qkv_finisher_reports_and_saturates(G, where, prec):
    """(iv) one value above 65504: counter 0, and the stored value is the saturated one."""
    n, E = [65, 3], FIN_HEADS * 64
    slab, _bias, pos = _finish_inputs(n, 5)
    pos[:] = 0                                                         # angle 0: Q stores the value itself
    row, head, d = 64, 1, 37                                           # the one-token tail tile of sequence 0
    slab[row, (0 if where == "q" else 2 * E) + head * 64 + d] = 70000.0
    q, k, vt, rng, _npad = _finish_run(G, prec, n, slab, None, pos)
    got = q[head, row, d] if where == "q" else vt[head, d, row]
    print(where, prec, "stored", got, "range", rng)
    assert got == np.float32(65504.0), got
    assert rng[0] >= 1 and rng[1] == 0, rng
    assert np.isfinite(q).all() and np.isfinite(k).all() and np.isfinite(vt).all()


# ------------------------------------------------------------------------------------------ the encoder form of the attention alone
ATT_HEADS = 2
# (id, switch 5, counts, the class of every sequence: (LDS stages, pose mode, prefetch, tail stage, nfull parity, last query block))
ATT_CASES = [
    ("all8_prefetch", 0, [1, 63, 64, 65, 128, 129, 256, 257],
     [(4, 0, 1, "pf0", "0", "ragged"), (4, 0, 1, "pf0", "0", "ragged"), (4, 0, 1, "none", "odd", "ragged"), (4, 0, 1, "pf1", "odd", "ragged"),
      (4, 0, 1, "none", "even", "full"), (4, 0, 1, "pf2", "even", "ragged"), (4, 0, 1, "none", "even", "full"), (4, 0, 0, "s0", "even", "ragged")]),
    ("n_equals_npad", 0, [256, 64, 128],
     [(4, 0, 1, "none", "even", "full"), (4, 0, 1, "none", "odd", "ragged"), (4, 0, 1, "none", "even", "full")]),
    ("double_buffered", 1, [257, 64, 1, 129, 65],
     [(2, 0, 0, "s0", "even", "ragged"), (2, 0, 0, "none", "odd", "ragged"), (2, 0, 0, "s0", "0", "ragged"), (2, 0, 0, "s0", "even", "ragged"),
      (2, 0, 0, "s1", "odd", "ragged")]),
]
ATT_IDS = [c[0] for c in ATT_CASES]


def _attn_launch(G, prec, case, inputs):
    """inputs: [(q, k, v)] per sequence [1, heads, n, 64] -> ([output [1, heads, n, 64]] per sequence, [class it ran under]).  The guard
    block behind the output planes must come back bit for bit."""
    import torch
    import attention_varlen_cases as AV
    import helpers as HP
    from vista_slam_amd import _lib
    _cid, opt5, n, _cls = case
    S, rows = len(n), sum(n)
    m, lib, h = G.kernel_handle(prec)
    q, k, v = (G.dev(np.concatenate([x[i].ravel() for x in inputs])) for i in range(3))
    out = torch.full((rows + AV.GUARD_ROWS, ATT_HEADS * 64), float("nan"), device="cuda")
    _lib.check(lib.sta_debug_set_option(h, 5, opt5))
    try:
        _lib.check(lib.sta_debug_attn_encv(h, q.data_ptr(), k.data_ptr(), v.data_ptr(), S, ATT_HEADS, (C.c_int * S)(*n), out.data_ptr(), G.st()))
        torch.cuda.synchronize()
        buf = (C.c_int * AV.plan_ints(AV.MAX_SEQ))()
        _lib.check(lib.sta_debug_last_attn_encv_plan(h, buf))
        plan = AV.plan_dict(buf)
    finally:
        _lib.check(lib.sta_debug_set_option(h, 5, 0))
    o = out.cpu().numpy()
    guard = np.float32(1.05859375 * 2)                                 # hi + lo of the byte pattern 0x3C3C
    touched = np.argwhere(o[rows:].view(np.uint32) != guard.view(np.uint32))
    assert len(touched) == 0, f"{case[0]}: {len(touched)} elements of the guard block behind the output changed, first (row, column) {touched[0]}"
    got, r0 = [], 0
    for c in n:
        got.append(HP.attn_rows_to_tokens(o[r0:r0 + c], "plain", 1, ATT_HEADS, c))
        r0 += c
    assert plan["S"] == S and plan["orows"] == rows and plan["pose_blocks"] == 0
    return got, [AV.seq_class(plan, i, n[i]) for i in range(S)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", ATT_CASES, ids=ATT_IDS)
def test_encoder_attention_selection_is_bit_exact(G, case, prec):
    import helpers as HP
    n = case[2]
    inputs, pis, margin = [], [], np.inf
    for s, c in enumerate(n):
        q, k, v, pi, mg = HP.attn_selection_inputs("plain", 1, ATT_HEADS, c, c, "self", 21 + s)
        v[..., 0] += s
        assert sorted(pi[0, 0].tolist()) == list(range(c))             # a permutation: key 0, key n - 1, both ends of every tile are selected
        inputs.append((q, k, v)); pis.append(pi); margin = min(margin, mg)
    assert margin > 160, margin
    got, ran = _attn_launch(G, prec, case, inputs)
    wrong, nan, first = 0, 0, []
    for s, c in enumerate(n):
        want = np.take_along_axis(inputs[s][2], pis[s][..., None], 2)
        bad = np.argwhere((got[s] != want).any(-1))
        wrong += len(bad); nan += int(np.isnan(got[s]).sum())
        for _z, h, t in bad[:4]:
            r = got[s][0, h, t]
            first.append(f"(sequence {s}, head {h}, query {t}): expected key {pis[s][0, h, t]}, got columns 0..2 = (sequence {r[0]:g}, head {r[1]:g}, key {r[2]:g})")
    print(case[0], prec, {"class": ran, "margin": margin, "nan": nan, "wrong": wrong})
    assert ran == case[3], ran
    assert wrong == 0, f"{wrong} wrong rows ({nan} NaN elements); {'; '.join(first[:8])}"
    assert nan == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", ATT_CASES, ids=ATT_IDS)
def test_encoder_attention_uniform_scores_give_the_column_mean(G, case, prec):
    import helpers as HP
    n = case[2]
    inputs = [HP.attn_uniform_inputs("plain", 1, ATT_HEADS, c, c, 22 + s) for s, c in enumerate(n)]
    got, ran = _attn_launch(G, prec, case, inputs)
    nan, max_abs, vmax = 0, 0.0, 0.0
    for s, (q, k, v) in enumerate(inputs):
        ref = np.broadcast_to(v.astype(np.float64).mean(2, keepdims=True), got[s].shape)
        nan += int(np.isnan(got[s]).sum())
        max_abs = max(max_abs, float(np.abs(got[s] - ref).max()))
        vmax = max(vmax, float(np.abs(v).max()))
    bound = 2.0 ** -20 * vmax
    print(case[0], prec, {"class": ran, "nan": nan, "max_abs": max_abs}, "bound", bound)
    assert ran == case[3], ran
    assert nan == 0
    assert max_abs <= bound, (max_abs, bound)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("sharp", [1.0, 3.0])
@pytest.mark.parametrize("case", ATT_CASES, ids=ATT_IDS)
def test_encoder_attention_gaussian_rows(G, case, sharp, prec):
    import helpers as HP
    n = case[2]
    inputs = [HP.attn_gaussian_inputs("plain", 1, ATT_HEADS, c, c, sharp, 100 + s) for s, c in enumerate(n)]
    model = 0.0
    for q, k, v in inputs:
        rows, _ = HP.attn_row_errors(HP.attn_model(q, k, v, 0, "f16x3"), HP.attn_ref64(q, k, v, 0))
        model = max(model, float(rows.max()))
    bound = 4.0 * model
    got, ran = _attn_launch(G, prec, case, inputs)
    worst, num, den, nan = 0.0, 0.0, 0.0, 0
    for s, (q, k, v) in enumerate(inputs):
        ref = HP.attn_ref64(q, k, v, 0)
        rows, _ = HP.attn_row_errors(got[s], ref)
        nan += int(np.isnan(got[s]).sum())
        worst = max(worst, float(np.nanmax(rows)))
        num += float(((got[s].astype(np.float64) - ref) ** 2).sum()); den += float((ref ** 2).sum())
    rel = float(np.sqrt(num / max(den, 1e-300)))
    print(case[0], sharp, prec, {"class": ran, "nan": nan, "worst_row": worst, "rel_l2": rel}, "bound", bound)
    assert ran == case[3], ran
    assert nan == 0
    assert worst < bound, (worst, bound)
    assert rel < GLOBAL_TOL["f16x3"], rel


# ------------------------------------------------------------------------------------------ the gather alone
def _gather_run(G, prec, frames, u8, sizes, pos, n, which):
    import torch
    from vista_slam_amd import _lib
    B = len(n)
    m, lib, h = G.kernel_handle(prec)
    out = torch.full((sum(n), 768), float("nan"), device="cuda")
    m.range_report(reset=True)
    d_pos = G.dev(pos)
    _lib.check(lib.sta_debug_patch_gather_varlen(h, (C.c_void_p * B)(*[f.data_ptr() for f in frames]), int(u8), (C.c_int * B)(*[s[0] for s in sizes]),
                                                 (C.c_int * B)(*[s[1] for s in sizes]), d_pos.data_ptr(), (C.c_int * B)(*n), B, which, out.data_ptr(), G.st()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tuple(m.range_report(reset=True))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8hwc"])
def test_varlen_gather_alone(G, u8, prec):
    """Three entries of different frame sizes, with repeats and a reversed order: one launch of the varlen form against the equal-count
    form of the same kernel entry by entry, bit for bit; both forms agree with the patch pixels themselves."""
    import torch
    from vista_slam_amd import weights as W
    sizes = [(48, 64), (128, 160), (32, 16)]
    idx = [np.array([11, 0, 5, 5, 5, 7, 0]), np.arange(80)[::-1].copy(), np.array([1, 0, 1])]
    n = [len(i) for i in idx]
    pos = np.concatenate([np.stack([i // (w // 16), i % (w // 16)], -1) for i, (_h, w) in zip(idx, sizes)]).astype(np.int32)
    f32 = [W.synth_images(1, h, w, seed=43, tag=b)[0] for b, (h, w) in enumerate(sizes)]
    frames = [torch.from_numpy(W.synth_images_u8(1, h, w, seed=43, tag=b)[0] if u8 else f32[b]).cuda() for b, (h, w) in enumerate(sizes)]
    one, rng1 = _gather_run(G, prec, frames, u8, sizes, pos, n, 0)
    per, rng2 = _gather_run(G, prec, frames, u8, sizes, pos, n, 1)
    assert np.isfinite(one).all()
    assert np.array_equal(one.view(np.uint32), per.view(np.uint32)), np.argwhere(one != per)[:4]
    r = 0
    for b, (h, w) in enumerate(sizes):
        for (y, x) in pos[r:r + n[b]]:
            want = f32[b][:, 16 * y:16 * y + 16, 16 * x:16 * x + 16].reshape(768)          # K order (c, ky, kx)
            assert np.abs(one[r] - want).max() <= 2.0 ** -20, (b, y, x)                    # |pixel| <= 1: hi + lo is within 2^-22 of it
            r += 1
    assert rng1 == (0, 0) and rng2 == (0, 0)


@pytest.mark.parametrize("prec", PRECS)
def test_varlen_gather_reports_an_out_of_range_pixel(G, prec):
    import torch
    from vista_slam_amd import weights as W
    sizes = [(48, 64), (32, 32)]
    f32 = [W.synth_images(1, h, w, seed=43, tag=b)[0].copy() for b, (h, w) in enumerate(sizes)]
    f32[1][2, 16 + 3, 16 + 9] = 1.0e5                                  # patch (1, 1) of entry 1, channel 2
    pos = np.array([[0, 0], [2, 3], [1, 1], [0, 1]], np.int32)
    frames = [torch.from_numpy(x).cuda() for x in f32]
    out, rng = _gather_run(G, prec, frames, False, sizes, pos, [2, 2], 0)
    assert out[2, 2 * 256 + 3 * 16 + 9] == np.float32(65504.0), out[2, 2 * 256 + 3 * 16 + 9]
    assert rng[0] >= 1 and rng[1] == 0, rng
    clean, rng = _gather_run(G, prec, frames, False, sizes, np.array([[0, 0], [2, 3], [1, 0], [0, 1]], np.int32), [2, 2], 0)
    assert rng == (0, 0) and np.abs(clean).max() <= 1.0          # the pixel is not selected: not read, not reported
