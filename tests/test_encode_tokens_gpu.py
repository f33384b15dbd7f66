"""GPU: the encoder on TOKEN SUBSETS (sta_encode_tokens[_u8hwc] through STAFrontend.encode_tokens / encode_tokens_u8hwc /
forward_pair_tokens / forward_pair_window(encode="window")) - against the reference fixtures `enct_*` (tools/gen_golden_enct.py),
the new route against the whole-frame encoder where the two must agree, exactness, refusals, and the rotation launch alone
(sta_debug_rope_enc_tokens).

Bounds: the project's bar TOL = 1e-3 of tests/test_gpu_parity.py for everything compared with a reference fixture (rel-L2 AND max
norm, range report (0, 0)); ROUTE_TOL = 0.1 x bar = 1e-4 for route-vs-route comparisons, by the argument of
tests/test_decode_mixed_gpu.py: every route is measured well inside half of that against the reference, so two of them are inside it
of each other.  The fixtures cannot be met by a route that ignores the positions or that encodes the frame and slices: both are
> 3e-3 away (tests/test_encode_tokens_cpu.py).

Route against route:
  (a) all tokens in row-major order == _encode_image (48x64 tiny, 224 x 224 full);
  (b) a permuted selection == the same selection in grid order with its rows permuted (attention is permutation-equivariant);
  (c) a window == _encode_image of the cropped image: the patch embedding is local and RoPE is relative, so a translated token set
      encodes identically (CPU oracle: 1.9e-7 window vs crop, <= 3e-6 under a (3, 5) shift at gain 3);
  (d) forward_pair_window(encode="window") == forward_pair_tokens on the window's positions.

The rotation launch alone, on inputs k * 2^-8 (|k| <= 1024: exact in an fp16 plane), positions in [0, 40], S = 2, heads = 2, buffers
[S*heads][npad][64] with npad = roundup(N, 64) - NO pose row - and one guard block of npad x 64 behind them:
  (i)  against an fp64 rotation by the exact angles: |err| <= (pos_max + 2) 2^-21 (|v0| + |v1|) per element, the bound derived in
       tests/test_decode_tokens_gpu.py;
  (ii) every row >= N of every (sequence, head) and the whole guard come back bit for bit.  The decoder's pose-row form of the same
       kernel (ntok + 1 rows per (sequence, head)) breaks (ii) exactly where N is a multiple of 64 - row 0 of the next head, and the
       guard after the last one; the test runs that form too (inside the guarded allocation: nothing faults) and asserts that it is
       caught there.

Measured (MI355X; worst over the cases of each class, f16x3h / f16x3; DESIGN.md section 3 keeps the table):
    encoder features vs golden 1.05e-5 (the gain-3 full case; 3.9e-6 / 3.6e-6 at gain 1 full, <= 1.5e-6 tiny), both precisions alike
    pair: hook layers 2.3e-6     pose 5.6e-6     pose confidence 0.0     points 3.4e-5 / 1.8e-6     confidence 6.6e-7 / 1.2e-7
    (a) all tokens vs _encode_image 2.7e-7 (tiny), 9.3e-7 (full)     (b) permuted 2.2e-7     (c) window vs crop 2.8e-7 (tiny), 3.0e-6 (full, gain 3)
    (d) forward_pair_window(encode="window") vs forward_pair_tokens 3.0e-5 / 1.0e-6 (side b: sta_encode against the table route, through the heads)
    u8hwc vs fp32 route and repeated calls: bit-identical     range report (0, 0) everywhere
    rotation: (i) 0.055 of the bound (0.036 at N = 1), (ii) holds for N in {1, 63, 64, 65, 128}; the pose-row form is caught at every N
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-3                  # tests/test_gpu_parity.py
ROUTE_TOL = 0.1 * TOL
DEFAULT = "f16x3h"
PAIR = "enct_tiny_pair_pruned_vs_win_b2"
CASES = ["enct_tiny_win_b2", "enct_tiny_pruned_b2", "enct_tiny_one_sharp", "enct_tiny_64_rev", "enct_tiny_128_of_132_b2",
         "enct_tiny_65_of_80", "enct_tiny_129_of_132", "enct_full_224_pruned_b1", "enct_full_384x512_192", "enct_full_224_pruned_sharp"]


@pytest.fixture(scope="module")
def G():
    import gpu_checks
    yield gpu_checks
    gpu_checks.drop_models()


def _err(got, want):
    from helpers import rel_l2, max_rel
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return max(rel_l2(got, want), max_rel(got, want))


def _model(G, full, gain, prec, seed=43):
    return G.model("full" if full else "tiny", gain, prec, seed=seed)


def _images(B, H, W_, seed=43, tag=0):
    import torch
    from vista_slam_amd import weights as W
    return torch.from_numpy(W.synth_images(B, H, W_, seed=seed, tag=tag)).cuda()


def _grid_index(B, n):
    import torch
    return torch.arange(n)[None].expand(B, -1).contiguous()


# ------------------------------------------------------------------------------------------ against the reference fixtures
@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("case", CASES)
def test_encode_tokens_vs_reference_golden(G, case, prec):
    """encode_tokens on the fixture's selection, given as positions (on the CPU) and as indices (on the device): rel-L2 and max norm."""
    import torch
    from helpers import load_golden
    g, meta = load_golden(case)
    m = _model(G, case.startswith("enct_full"), float(meta["qk_gain"]), prec, seed=int(meta["seed"]))
    B, H, W_, tsub = int(meta["B"]), int(meta["H"]), int(meta["W"]), int(meta["tsub"])
    img = _images(B, H, W_, seed=int(meta["seed"]))
    m.range_report(reset=True)
    feat, pos = m.encode_tokens(img, pos=torch.from_numpy(g["pos"]))
    feat_i, pos_i = m.encode_tokens(img, index=torch.from_numpy(g["idx"]).cuda())
    torch.cuda.synchronize()
    rng = tuple(m.range_report(reset=True))
    assert feat.shape == (B, g["idx"].shape[1], m.cfg.enc_embed_dim) and pos.dtype == torch.int64 and pos.is_cuda
    assert np.array_equal(pos.cpu().numpy(), g["pos"]) and np.array_equal(pos_i.cpu().numpy(), g["pos"])
    assert torch.equal(feat, feat_i)
    e = _err(feat[:, ::tsub], g["enc_feat"])
    print(case, prec, f"enc_feat {e:.2e}", "ref_noise", float(g["ref_noise"]), "range", rng)
    assert e <= TOL, e
    assert rng == (0, 0), rng


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_forward_pair_tokens_vs_reference_golden(G, prec):
    """The pair: encode both subsets, decode them (hook layers, pose row included), pose heads on both sides, points and confidence
    on the rectangular side; forward_pair_tokens returns the same heads and None for the points of the side without a grid."""
    import torch
    from helpers import load_golden
    g, meta = load_golden(PAIR)
    m = _model(G, False, float(meta["qk_gain"]), prec, seed=int(meta["seed"]))
    cfg, B, seed = m.cfg, int(meta["B"]), int(meta["seed"])
    img_a, img_b = _images(B, int(meta["H"]), int(meta["W"]), seed, 0), _images(B, int(meta["Hb"]), int(meta["Wb"]), seed, 1)
    pa, pb = torch.from_numpy(g["pos_a"]), torch.from_numpy(g["pos_b"]).cuda()
    m.range_report(reset=True)
    fa, qa = m.encode_tokens(img_a, pos=pa)
    fb, qb = m.encode_tokens(img_b, pos=pb)
    d1, d2 = m.decode_stereo_tokens(fa, fb, qa, qb)
    main, supp = m.forward_pair_tokens(img_a, img_b, pa, pb)
    torch.cuda.synchronize()
    errs = {"enc_feat_a": _err(fa, g["enc_feat_a"]), "enc_feat_b": _err(fb, g["enc_feat_b"])}
    for hk in cfg.hooks[1:]:
        errs[f"dec1_hook{hk - 1}"] = _err(d1[hk - 1], g[f"dec1_hook{hk - 1}"])
        errs[f"dec2_hook{hk - 1}"] = _err(d2[hk - 1], g[f"dec2_hook{hk - 1}"])
    for tag, r in (("a", main), ("b", supp)):
        errs[f"{tag}_pose"] = _err(r["relative_pose"], g[f"{tag}_pose"])
        errs[f"{tag}_pose_conf"] = _err(r["relative_pose_conf"], g[f"{tag}_pose_conf"])
    assert main["pts3d_pred"] is None and main["conf"] is None                  # 9 of 20 pruned: no rectangle, no DPT head
    assert supp["pts3d_pred"].shape == (B, 32, 48, 3)
    errs["b_pts3d"] = _err(supp["pts3d_pred"], g["b_pts3d"])
    errs["b_conf"] = _err(supp["conf"], g["b_conf"])
    rng = tuple(m.range_report(reset=True))
    print(PAIR, prec, {k: f"{v:.2e}" for k, v in errs.items()}, "ref_noise", float(g["ref_noise"]), "range", rng)
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    assert rng == (0, 0), rng


# ------------------------------------------------------------------------------------------ route against route
@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("shape", [("tiny", 2, 48, 64), ("full", 1, 224, 224)])
def test_all_tokens_in_grid_order_vs_encode_image(G, shape, prec):
    """(a) every token, row-major: the identity-table + rotate route against the whole-frame encoder."""
    import torch
    name, B, H, W_ = shape
    m = _model(G, name == "full", 1.0, prec)
    img = _images(B, H, W_, tag=3)
    m.range_report(reset=True)
    want, pos_w = m._encode_image(img, None, normalize=False)
    got, pos_g = m.encode_tokens(img, index=_grid_index(B, (H // 16) * (W_ // 16)))
    torch.cuda.synchronize()
    d = _err(got, want.cpu().numpy())
    print(shape, prec, "all tokens vs _encode_image", d)
    assert torch.equal(pos_g, pos_w)
    assert d <= ROUTE_TOL, d
    assert tuple(m.range_report(reset=True)) == (0, 0)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_permuted_selection_vs_permuted_rows(G, prec):
    """(b) 13 of 20 tokens in a random order per entry against the same tokens in grid order, rows permuted afterwards."""
    import torch
    m = _model(G, False, 1.0, prec)
    B, H, W_ = 2, 64, 80
    img = _images(B, H, W_, tag=4)
    rs = np.random.default_rng(5)
    perm = np.stack([rs.permutation(20)[:13] for _ in range(B)])
    order = np.argsort(perm, axis=1)                                  # perm[b][order[b]] is sorted
    sorted_idx = np.take_along_axis(perm, order, 1)
    got, _ = m.encode_tokens(img, index=torch.from_numpy(perm))
    base, _ = m.encode_tokens(img, index=torch.from_numpy(sorted_idx))
    torch.cuda.synchronize()
    inv = np.argsort(order, axis=1)                                   # row of perm[b][j] inside the sorted selection
    want = np.take_along_axis(base.cpu().numpy(), inv[:, :, None], 1)
    d = _err(got, want)
    print(prec, "permuted selection vs permuted rows", d)
    assert not np.array_equal(perm, sorted_idx)
    assert d <= ROUTE_TOL, d


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("shape", [("tiny", 1.0, 2, 64, 80, (1, 2, 2, 3)), ("full", 3.0, 1, 224, 224, (6, 4, 8, 10))])
def test_window_vs_encode_image_of_the_crop(G, shape, prec):
    """(c) a window of the frame, with its frame positions, against the cropped image encoded as a frame of its own."""
    import torch
    name, gain, B, H, W_, (y0, x0, h, w) = shape
    m = _model(G, name == "full", gain, prec)
    img = _images(B, H, W_, tag=6)
    crop = img[:, :, 16 * y0:16 * (y0 + h), 16 * x0:16 * (x0 + w)].contiguous()
    m.range_report(reset=True)
    want, _ = m._encode_image(crop, None, normalize=False)
    got, pos = m.encode_tokens(img, index=m.window_index((H // 16, W_ // 16), (y0, x0, h, w), B))
    torch.cuda.synchronize()
    assert pos[0, 0].tolist() == [y0, x0] and pos[0, -1].tolist() == [y0 + h - 1, x0 + w - 1]
    d = _err(got, want.cpu().numpy())
    print(shape, prec, "window vs crop", d)
    assert d <= ROUTE_TOL, d
    assert tuple(m.range_report(reset=True)) == (0, 0)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_forward_pair_window_encode_window_vs_forward_pair_tokens(G, prec):
    """(d) forward_pair_window(encode="window") against forward_pair_tokens on the windows' positions; the default encode="frame" is a
    different computation (the window's tokens have seen the whole frame) and stays what it was."""
    import torch
    m = _model(G, False, 1.0, prec)
    B = 2
    img_a, img_b = _images(B, 64, 80, tag=0), _images(B, 48, 64, tag=1)
    wins = [(1, 2, 2, 3), (2, 0, 2, 3)]
    ia = m.window_index((4, 5), wins, B)
    pa = torch.stack([ia // 5, ia % 5], -1)
    pb = m._positions(B, 3, 4)
    new = m.forward_pair_window(img_a, img_b, window_a=wins, encode="window")
    ref = m.forward_pair_tokens(img_a, img_b, pa, pb)
    old = m.forward_pair_window(img_a, img_b, window_a=wins)
    old2 = m.forward_pair_window(img_a, img_b, window_a=wins, encode="frame")
    torch.cuda.synchronize()
    worst = 0.0
    for a, b in zip(new, ref):
        for k in ("pts3d_pred", "conf", "relative_pose", "relative_pose_conf"):
            assert a[k].shape == b[k].shape
            worst = max(worst, _err(a[k], b[k].cpu().numpy()))
    print(prec, "forward_pair_window(encode=window) vs forward_pair_tokens", worst)
    assert worst <= ROUTE_TOL, worst
    assert new[0]["pts3d_pred"].shape == (B, 32, 48, 3) and new[1]["pts3d_pred"].shape == (B, 48, 64, 3)
    assert all(torch.equal(old[s][k], old2[s][k]) for s in range(2) for k in old[s])
    assert _err(new[0]["pts3d_pred"], old[0]["pts3d_pred"].cpu().numpy()) > 3 * TOL          # encoding the window alone IS another result
    with pytest.raises(ValueError, match="encode must be"):
        m.forward_pair_window(img_a, img_b, window_a=wins, encode="crop")


# ------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
def test_u8hwc_route_and_repeat_are_bit_identical(G, prec):
    import torch
    from vista_slam_amd import weights as W
    m = _model(G, False, 1.0, prec)
    B, H, W_ = 2, 64, 80
    f32 = _images(B, H, W_, tag=5)
    u8 = torch.from_numpy(W.synth_images_u8(B, H, W_, seed=43, tag=5)).cuda()
    idx = torch.from_numpy(np.stack([np.random.default_rng(9 + b).permutation(20)[:11] for b in range(B)]))
    a, pa = m.encode_tokens(f32, index=idx)
    b, pb = m.encode_tokens_u8hwc(u8, index=idx)
    c, _ = m.encode_tokens(f32, pos=pa)
    d, _ = m.encode_tokens_u8hwc(u8, pos=pb.cpu())
    torch.cuda.synchronize()
    assert torch.equal(pa, pb)
    assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(a, c) and torch.equal(b, d)
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ------------------------------------------------------------------------------------------ refusals
def test_encode_tokens_refusals(G):
    """The shim: positions outside the grid or negative, both or neither of pos / index, a wrong dtype or shape; the C entry: N = 0,
    H not a multiple of 16, null pointers - status -1 with a message."""
    import torch
    m = _model(G, False, 1.0, DEFAULT)
    B, H, W_ = 2, 48, 64
    img = _images(B, H, W_)
    pos = m._positions(B, 3, 4)[:, :5].contiguous()
    feat, q = m.encode_tokens(img, pos=pos)                         # what the refusals below are variations of
    assert feat.shape == (B, 5, m.cfg.enc_embed_dim)
    bad = pos.clone(); bad[1, 2, 1] = 4
    with pytest.raises(ValueError, match="outside the 3 x 4 patch grid"):
        m.encode_tokens(img, pos=bad)
    bad = pos.clone(); bad[0, 0, 0] = 3
    with pytest.raises(ValueError, match="outside the 3 x 4 patch grid"):
        m.encode_tokens(img, pos=bad)
    with pytest.raises(ValueError, match="outside the 3 x 4 patch grid"):
        m.encode_tokens(img, pos=pos - 1)
    with pytest.raises(ValueError, match="outside the 3 x 4 patch grid"):
        m.encode_tokens(img, index=torch.tensor([[0, 12], [1, 2]]))
    with pytest.raises(ValueError, match="outside the 3 x 4 patch grid"):
        m.encode_tokens_u8hwc(torch.zeros(B, H, W_, 3, dtype=torch.uint8), index=torch.tensor([[0, -1], [1, 2]]))
    with pytest.raises(ValueError, match="exactly one of pos"):
        m.encode_tokens(img)
    with pytest.raises(ValueError, match="exactly one of pos"):
        m.encode_tokens(img, pos=pos, index=_grid_index(B, 5))
    with pytest.raises(AssertionError, match="positions must be int64"):
        m.encode_tokens(img, pos=pos.float())
    with pytest.raises(AssertionError, match="positions must be int64"):
        m.encode_tokens(img, pos=pos.int())
    with pytest.raises(AssertionError, match="index must be int64"):
        m.encode_tokens(img, index=_grid_index(B, 5).int())
    with pytest.raises(AssertionError, match=r"positions must be \[2, N >= 1, 2\]"):
        m.encode_tokens(img, pos=pos[:1])
    with pytest.raises(AssertionError, match=r"positions must be \[2, N >= 1, 2\]"):
        m.encode_tokens(img, pos=pos[:, :, :1])
    with pytest.raises(AssertionError, match=r"positions must be \[2, N >= 1, 2\]"):
        m.encode_tokens(img, pos=pos[:, :0])
    with pytest.raises(AssertionError, match=r"index must be \[2, N >= 1\]"):
        m.encode_tokens(img, index=torch.arange(5))
    with pytest.raises(AssertionError, match="multiple of patch size"):
        m.encode_tokens(img[:, :, :40], pos=pos)
    q = q.contiguous()
    out = torch.empty_like(feat)
    u8 = torch.zeros(B, H, W_, 3, dtype=torch.uint8, device="cuda")
    for entry, image, args, what in (
            (m.lib.sta_encode_tokens, img.data_ptr(), (q.data_ptr(), B, H, W_, 0, out.data_ptr()), "at least one token"),          # N = 0
            (m.lib.sta_encode_tokens, img.data_ptr(), (q.data_ptr(), B, 40, W_, 5, out.data_ptr()), "multiple of patch size"),     # H % 16
            (m.lib.sta_encode_tokens, img.data_ptr(), (None, B, H, W_, 5, out.data_ptr()), "null device pointer"),
            (m.lib.sta_encode_tokens, None, (q.data_ptr(), B, H, W_, 5, out.data_ptr()), "null device pointer"),
            (m.lib.sta_encode_tokens_u8hwc, u8.data_ptr(), (q.data_ptr(), B, H, W_, 0, out.data_ptr()), "at least one token"),
            (m.lib.sta_encode_tokens_u8hwc, u8.data_ptr(), (q.data_ptr(), B, H, 40, 5, out.data_ptr()), "multiple of patch size")):
        rc = entry(m._h, image, *args, m._stream())
        msg = m.lib.sta_last_error().decode()
        assert rc == -1 and what in msg, (args[1:5], rc, msg)
    again, _ = m.encode_tokens(img, pos=pos)                        # a refused call leaves the handle as it was
    assert torch.equal(again, feat)


# ------------------------------------------------------------------------------------------ the rotation launch alone
POS_MAX = 40
ROPE_N = [1, 63, 64, 65, 128]
SENTINEL = np.float32(-777.25)       # k * 2^-8 with |k| > 1024 * 2^8: not a value of the live rows, exact as hi + lo


def _rope_enc_inputs(S, heads, n, nbuf, seed):
    rs = np.random.default_rng(seed)
    npad = (n + 63) // 64 * 64
    bufs = []
    for _ in range(nbuf):
        b = np.full((S * heads + 1, npad, 64), SENTINEL, np.float32)             # the last block is the guard
        b[:S * heads] = rs.integers(-1024, 1025, size=(S * heads, npad, 64)) * 2.0 ** -8
        bufs.append(b)
    pos = rs.integers(0, POS_MAX + 1, size=(S, n, 2)).astype(np.int32)
    return bufs, pos, npad


def _rope_enc_run(G, prec, bufs, pos, S, heads, n, pose):
    import torch
    from vista_slam_amd import _lib
    m, lib, h = G.kernel_handle(prec)
    dev = [G.dev(b) for b in bufs]
    table = G.dev(pos.ravel())
    ptrs = (C.c_void_p * 2)(*([t.data_ptr() for t in dev] + [None] * (2 - len(dev))))
    _lib.check(lib.sta_debug_rope_enc_tokens(h, ptrs, len(dev), S, heads, n, table.data_ptr(), POS_MAX, pose, G.st()))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev]


def _rope_enc_ref64(buf, pos, S, heads, n):
    """fp64 rotation of rows [0, n) of every (sequence, head); everything else is copied."""
    out = buf.astype(np.float64)
    inv = 100.0 ** (-np.arange(16, dtype=np.float64) / 16.0)
    live = out[:S * heads].reshape(S, heads, buf.shape[1], 64)          # a view: writes land in `out`
    src = buf[:S * heads].reshape(S, heads, buf.shape[1], 64).astype(np.float64)
    for xy in range(2):
        ang = pos[:, :, xy, None].astype(np.float64) * inv[None, None, :]               # [S, n, 16]
        c, sn = np.cos(ang)[:, None], np.sin(ang)[:, None]
        v0, v1 = src[:, :, :n, xy * 32:xy * 32 + 16], src[:, :, :n, xy * 32 + 16:xy * 32 + 32]
        live[:, :, :n, xy * 32:xy * 32 + 16] = v0 * c - v1 * sn
        live[:, :, :n, xy * 32 + 16:xy * 32 + 32] = v1 * c + v0 * sn
    return out


def _pair_sum(buf):
    """|v0| + |v1| of every rotation pair (d, d + 16), broadcast back to both elements of the pair."""
    a = np.abs(buf.astype(np.float64)).reshape(buf.shape[:2] + (2, 2, 16))
    s = a[..., 0, :] + a[..., 1, :]
    return np.broadcast_to(s[..., None, :], a.shape).reshape(buf.shape)


@pytest.mark.parametrize("prec", [DEFAULT, "f16x3"])
@pytest.mark.parametrize("n", ROPE_N)
def test_rope_rotation_of_buffers_without_a_pose_row(G, n, prec):
    S, heads, nbuf = 2, 2, 2
    bufs, pos, npad = _rope_enc_inputs(S, heads, n, nbuf, seed=11 + n)
    new = _rope_enc_run(G, prec, bufs, pos, S, heads, n, 0)
    worst = 0.0
    live = np.zeros(bufs[0].shape, bool)
    live[:S * heads, :n] = True
    for b in range(nbuf):
        # (ii) rows >= n of every (sequence, head) and the guard: bit for bit what went in
        assert np.array_equal(new[b][~live].view(np.uint32), bufs[b][~live].view(np.uint32)), ("dead rows or the guard written", b, np.argwhere((new[b] != bufs[b]) & ~live)[:4])
        assert np.isfinite(new[b]).all()
        # (i) against the fp64 rotation
        ref = _rope_enc_ref64(bufs[b], pos, S, heads, n)
        bound = (POS_MAX + 2) * 2.0 ** -21 * _pair_sum(bufs[b])
        err = np.abs(new[b].astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300))[live & (bound > 0)].max()))
        assert (err <= bound)[live].all(), ("vs fp64 rotation", b, np.argwhere((err > bound) & live)[:4])
        assert not np.array_equal(new[b][live], bufs[b][live])          # it did rotate
    print(n, prec, "no-pose rotation vs fp64, fraction of bound", worst)
    # the decoder's pose-row form on the same buffers: (ii) catches it exactly where row n is another block's row 0
    old = _rope_enc_run(G, prec, bufs, pos, S, heads, n, 1)
    broken = [not np.array_equal(old[b][~live].view(np.uint32), bufs[b][~live].view(np.uint32)) for b in range(nbuf)]
    assert all(broken), "the pose-row form rotates row n: (ii) must see it"
    if n % 64 == 0:
        for b in range(nbuf):
            assert not np.array_equal(old[b][S * heads], bufs[b][S * heads]), "pose-row form: the guard block's row 0"
