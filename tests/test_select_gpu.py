"""GPU: sta_select_patches (csrc/select.h) through vista_slam_amd.select against the numpy restatement of its contract
(tests/select_cases.py).  The contract is integer arithmetic, so every assertion is array_equal: scores, ascending index lists,
(y, x) lists, -1 tails, counts, windows, slot offsets.  The shapes are the smallest at which the kernels can go wrong: one patch, the
wave boundary (63 / 64 / 65 patches), the chunk boundary (255 / 256 / 257), portrait, the 8192-patch limit, 32 mixed entries."""
import ctypes as C

import numpy as np
import pytest

import select_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    fe = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield fe
    del fe


def _up(maps):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in maps]


def _raw(sel):
    return {"score": sel.score_slots.cpu().numpy(), "index": sel.index_slots.cpu().numpy(), "pos": sel.pos_slots.cpu().numpy(),
            "n_sel": sel.n_sel.cpu().numpy(), "window": sel.window.cpu().numpy()}


def _check(sel, exp, what=""):
    got = _raw(sel)
    for key in S.OUTPUTS:
        assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape, (what, key, got[key].dtype, got[key].shape)
        if not np.array_equal(got[key], exp[key]):
            bad = np.flatnonzero((got[key] != exp[key]).reshape(-1))
            raise AssertionError(f"{what}: {key} differs at {bad.size} of {got[key].size} places, first {bad[:8].tolist()}: "
                                 f"got {got[key].reshape(-1)[bad[:8]].tolist()}, expected {exp[key].reshape(-1)[bad[:8]].tolist()}")
    return got


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_against_the_restatement(m, name):
    from vista_slam_amd import select
    maps, kw = S.build(name)
    exp = S.expected(maps, **kw)
    sel = select.select_tokens_from_maps(m, _up(maps), **kw)
    _check(sel, exp, name)
    # the per-entry views are the slots cut at the counts
    off, B = exp["off"], len(maps)
    assert sel.counts == exp["n_sel"].tolist() and [list(w) for w in sel.windows] == exp["window"].tolist()
    for b in range(B):
        n = int(exp["n_sel"][b])
        assert np.array_equal(sel.index[b].cpu().numpy(), exp["index"][off[b]:off[b] + n])
        assert np.array_equal(sel.pos[b].cpu().numpy(), exp["pos"][off[b]:off[b] + n])
        assert np.array_equal(sel.scores[b].cpu().numpy(), S.pool(maps[b], kw.get("thres"), kw.get("invert", False)))


def test_one_stacked_tensor_and_patch_scores(m):
    """maps as one [B, H, W] tensor; patch_scores alone; bool maps."""
    import torch
    from vista_slam_amd import select
    maps = [S.random_mask(48, 64, 40 + b).astype(np.bool_) for b in range(3)]
    stack = torch.from_numpy(np.stack(maps)).cuda()
    _check(select.select_tokens_from_maps(m, stack, min_score=90, margin=1), S.expected(maps, min_score=90, margin=1), "stacked bool")
    for got, x in zip(select.patch_scores(m, stack, invert=True), maps):
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), S.pool(x, invert=True))
    f = [S.threshold_float(80, 48, 0.5, 50)]
    assert np.array_equal(select.patch_scores(m, _up(f), thres=0.5)[0].cpu().numpy(), S.pool(f[0], thres=0.5))
    assert np.array_equal(select.patch_scores(m, _up(f))[0].cpu().numpy(), S.pool(f[0]))


@pytest.mark.parametrize("H,W", [(48, 64), (16, 1040), (272, 240)])
def test_unaligned_maps_take_the_elementwise_path(m, H, W):
    """A bool view whose storage offset is 1 byte, and a float32 view 4 bytes into its storage: the same data as the aligned maps."""
    import torch
    from vista_slam_amd import select
    mask = S.random_mask(H, W, 60)
    buf = torch.zeros(H * W + 16, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + H * W].view(H, W)
    view.copy_(torch.from_numpy(mask))
    bview = view.view(torch.bool)
    assert bview.data_ptr() % 16 == 1 and bview.is_contiguous()
    exp = S.expected([mask], min_score=100, margin=1)
    _check(select.select_tokens_from_maps(m, [bview], min_score=100, margin=1), exp, "bool at +1")
    _check(select.select_tokens_from_maps(m, _up([mask.astype(np.bool_)]), min_score=100, margin=1), exp, "bool aligned")
    fl = S.hostile_float(H, W, 61)
    fbuf = torch.zeros(H * W + 4, dtype=torch.float32, device="cuda")
    fview = fbuf[1:1 + H * W].view(H, W)
    fview.copy_(torch.from_numpy(fl))
    assert fview.data_ptr() % 16 == 4
    for kw in (dict(top_k=max(1, (H // 16) * (W // 16) // 3)), dict(thres=0.25, min_score=60), dict(thres=0.25, invert=True, min_score=60)):
        exp = S.expected([fl], **kw)
        _check(select.select_tokens_from_maps(m, [fview], **kw), exp, f"float at +4 {kw}")
        _check(select.select_tokens_from_maps(m, _up([fl]), **kw), exp, f"float aligned {kw}")


def test_no_allocation_no_synchronisation_and_a_repeat_is_identical(m):
    """alloc_stats() before the FIRST call of a set of shapes equals the value after it; under top_k the views need no device read;
    under min_score the first access reads the 5 B ints once; a repeat is bit-identical."""
    import torch
    from vista_slam_amd import select
    maps = [S.random_mask(96, 112, 70), S.random_mask(32, 208, 71), S.random_mask(1024, 2048, 72)]
    dev = _up(maps)
    torch.cuda.synchronize()
    before = m.alloc_stats()
    a = select.select_tokens_from_maps(m, dev, min_score=120, margin=2)
    b = select.select_tokens_from_maps(m, dev, top_k=[5, 26, 4000])
    assert m.alloc_stats() == before
    assert a._host is None and b._host is None
    assert [int(t.numel()) for t in b.index] == [5, 26, 4000] and [tuple(t.shape) for t in b.pos] == [(5, 2), (26, 2), (4000, 2)]
    assert b._host is None                                   # top_k: the counts are the arguments
    first = a.counts
    host = a._host
    assert host is not None and len(host) == 5 * 3
    _ = a.windows, a.index, a.pos
    assert a._host is host                                   # ONE read
    ra, rb = _check(a, S.expected(maps, min_score=120, margin=2), "min"), _check(b, S.expected(maps, top_k=[5, 26, 4000]), "topk")
    assert first == ra["n_sel"].tolist()
    a2 = _raw(select.select_tokens_from_maps(m, dev, min_score=120, margin=2))
    b2 = _raw(select.select_tokens_from_maps(m, dev, top_k=[5, 26, 4000]))
    for key in S.OUTPUTS:
        assert np.array_equal(ra[key], a2[key]) and np.array_equal(rb[key], b2[key])
    assert m.alloc_stats() == before


def test_outputs_of_other_slots_are_untouched(m):
    """Nothing is written outside [0, sum N): the call on a sub-range of larger buffers leaves the guard words alone."""
    import torch
    maps = _up([S.random_mask(48, 64, 80), S.random_mask(16, 1040, 81)])
    total, B, G = 12 + 65, 2, 64
    score = torch.full((total + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    index = torch.full((total + 2 * G,), 0x5A5A5A5A5A, dtype=torch.int64, device="cuda")
    pos = torch.full((total + 2 * G, 2), 0x5A5A5A5A5A, dtype=torch.int64, device="cuda")
    meta = torch.full((5 * B + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in maps])
    from vista_slam_amd import _lib
    _lib.check(m.lib.sta_select_patches(m._h, ptrs, (C.c_int * B)(48, 16), (C.c_int * B)(64, 1040), B, 0, 0, 0.0, 0, 0, 100, None, 1,
                                        score[G:].data_ptr(), index[G:].data_ptr(), pos[G:].data_ptr(), meta[G:].data_ptr(),
                                        meta[G + B:].data_ptr(), m._stream()))
    torch.cuda.synchronize()
    exp = S.expected([t.cpu().numpy() for t in maps], min_score=100, margin=1)
    assert np.array_equal(score[G:G + total].cpu().numpy(), exp["score"]) and np.array_equal(index[G:G + total].cpu().numpy(), exp["index"])
    assert np.array_equal(pos[G:G + total].cpu().numpy(), exp["pos"])
    assert np.array_equal(meta[G:G + B].cpu().numpy(), exp["n_sel"]) and np.array_equal(meta[G + B:G + 5 * B].cpu().numpy().reshape(B, 4), exp["window"])
    for t, v in ((score, 0x5A5A5A5A), (index, 0x5A5A5A5A5A), (pos, 0x5A5A5A5A5A)):
        assert bool((t[:G] == v).all()) and bool((t[G + total:] == v).all())
    assert bool((meta[:G] == 0x5A5A5A5A).all()) and bool((meta[G + 5 * B:] == 0x5A5A5A5A).all())


# ----------------------------------------------------------------------------------------------------------------------
# refusals
def _c_entry(m, H, W, dtype=0, mode=0, invert=0, rule=0, min_score=1, top_k=None, margin=0, ptr_shift=0, null=None, B=None):
    """The C entry itself with small real buffers; a refused call launches nothing, so the sizes named in H / W are never touched."""
    import torch
    B = len(H) if B is None else B
    n = max(len(H), 1)
    maps = [torch.zeros(16, 16, dtype=torch.float32 if dtype == 1 else torch.uint8, device="cuda") for _ in range(n)]
    out = {k: torch.zeros(64, dtype=t, device="cuda") for k, t in (("score", torch.int32), ("index", torch.int64), ("pos", torch.int64),
                                                                    ("n_sel", torch.int32), ("window", torch.int32))}
    a = {k: v.data_ptr() for k, v in out.items()}
    if null in a:
        a[null] = None
    ptrs = (C.c_void_p * n)(*[t.data_ptr() + ptr_shift for t in maps])
    ks = None if top_k is None else (C.c_int * n)(*top_k)
    return m.lib.sta_select_patches(m._h, None if null == "maps" else ptrs, None if null == "H" else (C.c_int * n)(*H),
                                    None if null == "W" else (C.c_int * n)(*W), B, dtype, mode, 0.0, invert, rule, min_score, ks, margin,
                                    a["score"], a["index"], a["pos"], a["n_sel"], a["window"], m._stream())


@pytest.mark.parametrize("kw,text", [
    (dict(H=[16], W=[16], null="maps"), "null argument"),
    (dict(H=[16], W=[16], null="H"), "null argument"),
    (dict(H=[16], W=[16], null="score"), "null argument"),
    (dict(H=[16], W=[16], null="index"), "null argument"),
    (dict(H=[16], W=[16], null="pos"), "null argument"),
    (dict(H=[16], W=[16], null="n_sel"), "null argument"),
    (dict(H=[16], W=[16], null="window"), "null argument"),
    (dict(H=[16], W=[16], rule=1, top_k=None), "null argument"),
    (dict(H=[16], W=[16], B=0), "1 .. 32 maps"),
    (dict(H=[16] * 33, W=[16] * 33), "1 .. 32 maps"),
    (dict(H=[0], W=[16]), "multiples of 16"),
    (dict(H=[16], W=[24]), "multiples of 16"),
    (dict(H=[16, 16], W=[16, 8208 * 16]), "entry 1: 16 x 131328 is 8208 patches"),
    (dict(H=[16], W=[16], dtype=0, mode=1), "float32 maps only"),
    (dict(H=[16], W=[16], dtype=1, mode=1, invert=1), "invert is refused"),
    (dict(H=[48], W=[64], rule=1, top_k=[3], margin=1), "margin is refused with top_k"),
    (dict(H=[48], W=[64], rule=1, top_k=[0]), "top_k must lie in [1, 12]"),
    (dict(H=[48, 16], W=[64, 16], rule=1, top_k=[12, 2]), "entry 1: top_k must lie in [1, 1]"),
    (dict(H=[48], W=[64], min_score=-1), "min_score must be >= 0"),
    (dict(H=[48], W=[64], margin=9), "margin must lie in [0, 8]"),
    (dict(H=[48], W=[64], margin=-1), "margin must lie in [0, 8]"),
    (dict(H=[16], W=[16], dtype=1, ptr_shift=2), "4-byte aligned"),
])
def test_c_entry_refuses_with_a_message(m, kw, text):
    from vista_slam_amd import _lib
    rc = _c_entry(m, **kw)
    assert rc == -1
    with pytest.raises(_lib.StaError) as e:
        _lib.check(rc)
    assert text in str(e.value), str(e.value)


def test_shim_refuses_before_the_library(m):
    import torch
    from vista_slam_amd import select
    good = _up([S.random_mask(48, 64, 1)])[0]
    with pytest.raises(ValueError, match="8208 patches"):
        select.select_tokens_from_maps(m, [torch.zeros(16, 8208 * 16, dtype=torch.uint8, device="cuda")], min_score=1)
    with pytest.raises(ValueError, match=r"torch.int32 \(48, 64\)"):
        select.select_tokens_from_maps(m, [good.to(torch.int32)], min_score=1)
    with pytest.raises(ValueError, match=r"torch.uint8 \(3, 48, 64\)"):
        select.select_tokens_from_maps(m, [good[None].expand(3, -1, -1)], min_score=1)
    with pytest.raises(ValueError, match="contiguous"):
        select.select_tokens_from_maps(m, [good[:, ::2][:, :16]], min_score=1)
    with pytest.raises(ValueError, match="share a dtype"):
        select.select_tokens_from_maps(m, [good, good.float()], min_score=1)
    with pytest.raises(ValueError, match="device"):
        select.select_tokens_from_maps(m, [good.cpu()], min_score=1)
    with pytest.raises(ValueError, match="exactly one of min_score and top_k"):
        select.select_tokens_from_maps(m, [good])
    with pytest.raises(ValueError, match="margin is refused with top_k"):
        select.select_tokens_from_maps(m, [good], top_k=2, margin=1)
    # after the refusals the handle still serves a good call
    _check(select.select_tokens_from_maps(m, [good], top_k=2), S.expected([good.cpu().numpy()], top_k=2), "after refusals")


# ----------------------------------------------------------------------------------------------------------------------
# end to end on the tiny model: the selections go unchanged into the token routes
SIZES = [(48, 64), (80, 48), (32, 48)]


def _frames():
    import torch
    from vista_slam_amd import weights as W
    return [torch.from_numpy(W.synth_images(1, H, Wd, seed=7 + i, tag=i))[0].cuda() for i, (H, Wd) in enumerate(SIZES)]


def _host_lists(exp):
    import torch
    off = exp["off"]
    idx = [torch.from_numpy(exp["index"][off[b]:off[b] + int(n)].copy()) for b, n in enumerate(exp["n_sel"])]
    pos = [torch.from_numpy(exp["pos"][off[b]:off[b] + int(n)].copy()) for b, n in enumerate(exp["n_sel"])]
    return idx, pos


def test_mask_selection_through_encode_and_decode_varlen(m):
    """A mask selection over three frames of different size -> encode_tokens_varlen(index=sel.index) -> decode_stereo_varlen against
    a top_k selection of the same frames: bit-identical to the same calls fed the restatement's lists built on the host."""
    import torch
    from vista_slam_amd import select
    imgs = _frames()
    masks = [S.random_mask(H, Wd, 90 + i) for i, (H, Wd) in enumerate(SIZES)]
    confs = [S.hostile_float(H, Wd, 95 + i) for i, (H, Wd) in enumerate(SIZES)]
    exp1, exp2 = S.expected(masks, min_score=100, margin=1), S.expected(confs, top_k=[5, 7, 3])
    assert (exp1["n_sel"] >= 1).all()
    sel1 = select.select_tokens_from_maps(m, _up(masks), min_score=100, margin=1)
    sel2 = select.select_tokens_from_maps(m, _up(confs), top_k=[5, 7, 3])
    (idx1, pos1), (idx2, pos2) = _host_lists(exp1), _host_lists(exp2)
    m.set_deterministic(True)
    try:
        f1, q1 = m.encode_tokens_varlen(imgs, index=sel1.index)
        f2, q2 = m.encode_tokens_varlen(imgs, index=sel2.index)
        h1, hq1 = m.encode_tokens_varlen(imgs, index=idx1)
        h2, hq2 = m.encode_tokens_varlen(imgs, index=idx2)
        d1, d2 = m.decode_stereo_varlen(f1, f2, sel1.pos, sel2.pos)
        e1, e2 = m.decode_stereo_varlen(h1, h2, pos1, pos2)
        torch.cuda.synchronize()
    finally:
        m.set_deterministic(False)
    for b in range(3):
        assert torch.equal(f1[b], h1[b]) and torch.equal(f2[b], h2[b]) and torch.equal(q1[b], hq1[b]) and torch.equal(q2[b], hq2[b])
        assert torch.equal(q1[b].cpu(), pos1[b]) and tuple(f1[b].shape) == (int(exp1["n_sel"][b]), m.cfg.enc_embed_dim)
        assert torch.equal(d1[-1][b], e1[-1][b]) and torch.equal(d2[-1][b], e2[-1][b])
        assert bool(torch.isfinite(d1[-1][b]).all())


def test_topk_selection_and_windows_through_regress_views_tokens(m):
    """A top_k selection gives index lists for two sides and `windows` for the two sides that get maps from the DPT head:
    bit-identical to the call fed the restatement's lists and tuples."""
    import torch
    from vista_slam_amd import select
    from vista_slam_amd.slam_scheduler import regress_views_tokens
    imgs = _frames()
    feats = [m._encode_image(im[None], None, normalize=False)[0] for im in imgs]
    confs = [S.hostile_float(H, Wd, 97 + i) for i, (H, Wd) in enumerate(SIZES)]
    ks = [6, 8, 4]
    exp = S.expected(confs, top_k=ks)
    sel = select.select_tokens_from_maps(m, _up(confs), top_k=ks)
    idx, _pos = _host_lists(exp)
    wins = [tuple(int(v) for v in w) for w in exp["window"]]
    assert sel.windows == wins and all(w[2] >= 1 and w[3] >= 1 for w in wins)

    def run(ix, wn):
        return regress_views_tokens(m, feats[0], SIZES[0], [feats[1], feats[2]], [SIZES[1], SIZES[2]], [ix[0], wn[0]], [wn[1], ix[2]],
                                    [True, True], 0.0)
    m.set_deterministic(True)
    try:
        got, want = run(sel.index, sel.windows), run(idx, wins)
        torch.cuda.synchronize()
    finally:
        m.set_deterministic(False)
    for e, (a, b) in enumerate(zip(got, want)):
        assert a.accepted and b.accepted and a.rel_pose_conf == b.rel_pose_conf and torch.equal(a.pose, b.pose)
        side = 1 if e == 0 else 0              # edge 0: side j is the window; edge 1: side i
        assert a.confs[1 - side] is None and a.confs[side] is not None
        h, w = (wins[1] if e == 0 else wins[0])[2:]
        assert sorted(a.confs[side].shape) == sorted((16 * h, 16 * w))
        assert torch.equal(a.confs[side], b.confs[side]) and torch.equal(a.pts3d[side], b.pts3d[side]) and torch.equal(a.depths[side], b.depths[side])
