"""GPU: loop candidates (csrc/loop.h: sta_orb_extract / sta_bow_transform / sta_bow_score, vista_slam_amd.loop) against the numpy
restatement of their contract (tests/loop_cases.py), through the C ABI with guard regions behind every output and through the Python
layer.  Every comparison is array_equal - level images, blurred levels, keypoints, responses, descriptors, words, counts; the
exceptions are the BoW values and the similarities: float64 sums of at most 4096 terms in [0, 1] whose order differs from numpy's,
which costs at most about 4096 * 1.1e-16 = 5e-13, compared at 1e-12 absolute.  The shapes are the smallest at which the kernels can go
wrong: frames a few pixels wider than twice the edge, sizes that are no multiple of the 16-pixel tile, pyramids whose upper levels are
not built, candidate counts either side of n_l and of the first cut with ties at the cut, all-tie frames, an empty frame, descriptor
counts either side of a wave, trees whose fan-out fills a wave, database sizes 1 / 5 / 400 with empty rows, a query longer than a
database row.  The checkerboard does NOT produce tied comparisons under this contract: its X-corners have no arc of 9, so it has no FAST
corner at level 0 (and untied survivors on the resampled levels) and is only compared with the restatement; the frame in which every NMS
comparison ties is `loop_cases.dot_frame` (2x2 dots: four corners of one score each), asserted on the restatement and on the GPU."""
import numpy as np
import pytest

import flow_cases as F
import loop_cases as L

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64               # bytes / rows behind every output
TRIG = L.trig_table()
PATTERN = L.default_pattern()


@pytest.fixture(scope="module")
def m():
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    fe = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    yield fe
    del fe


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(nbytes):
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


def run_orb(m, frame, nfeatures=500, nlevels=8, fast_threshold=20, edge=31, pattern=PATTERN):
    """-> (kp [n,4], resp [n], desc [n,32], levels, blurred levels) through the C ABI; the rows at or past n, the bytes behind n and
    behind the workspace, and the gaps between the levels of the two promised planes must still hold the fill pattern."""
    import torch
    from vista_slam_amd import _lib, loop
    frame = np.ascontiguousarray(frame)
    H, W = frame.shape
    p = loop.plan(H, W, nfeatures, nlevels, fast_threshold, edge)
    src, trig, pat = _up(frame), _up(TRIG), _up(pattern)
    ws = _filled(p.workspace_bytes + GUARD)
    kp, resp, desc, n = _filled((p.rows + GUARD) * 16), _filled((p.rows + GUARD) * 8), _filled((p.rows + GUARD) * 32), _filled(4 + GUARD)
    _lib.check(m.lib.sta_orb_extract(m._h, src.data_ptr(), 0 if frame.dtype == np.uint8 else 1, H, W, nfeatures, nlevels, fast_threshold, edge,
                                     trig.data_ptr(), pat.data_ptr(), ws.data_ptr(), p.workspace_bytes, kp.data_ptr(), resp.data_ptr(),
                                     desc.data_ptr(), n.data_ptr(), m._stream()))
    torch.cuda.synchronize()
    nraw, kraw, rraw, draw, wraw = (t.cpu().numpy() for t in (n, kp, resp, desc, ws))
    count = int(nraw[:4].view(np.int32)[0])
    assert 0 <= count <= p.rows, count
    assert (nraw[4:] == FILL).all() and (kraw[count * 16:] == FILL).all() and (rraw[count * 8:] == FILL).all() and (draw[count * 32:] == FILL).all(), \
        "rows at or past n were written"
    assert (wraw[p.workspace_bytes:] == FILL).all(), "bytes behind the workspace were written"
    planes = []
    for base in (0, p.plane_bytes):
        plane, gaps, lv = wraw[base:base + p.plane_bytes], np.ones(p.plane_bytes, bool), []
        for (h, w), o in zip(p.sizes, p.offsets):
            lv.append(plane[o:o + h * w].reshape(h, w).copy())
            gaps[o:o + h * w] = False
        assert (plane[gaps] == FILL).all(), "bytes between the levels were written"
        planes.append(lv)
    return (kraw[:count * 16].view(np.int32).reshape(count, 4).copy(), rraw[:count * 8].view(np.int64).copy(),
            draw[:count * 32].reshape(count, 32).copy(), planes[0], planes[1])


def check_orb(got, frame, what, **kw):
    """against the restatement; -> its info"""
    info = {}
    e_kp, e_resp, e_desc = L.extract(frame, pattern=kw.pop("pattern", PATTERN), trig=TRIG, info=info, **kw)
    kp, resp, desc, lv, bl = got
    assert len(lv) == len(info["levels"]), (what, len(lv), len(info["levels"]))
    for l, (g, e) in enumerate(zip(lv, info["levels"])):
        assert np.array_equal(g, e), (what, "level", l, int((g != e).sum()))
    for l, (g, e) in enumerate(zip(bl, info["blurred"])):
        assert np.array_equal(g, e), (what, "blurred level", l, int((g != e).sum()))
    assert len(kp) == len(e_kp), (what, len(kp), len(e_kp), info["cuts"])
    bad = np.flatnonzero((kp != e_kp).any(1) | (resp != e_resp) | (desc != e_desc).any(1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(kp)} rows differ, first {bad[:3].tolist()}: got {kp[bad[:3]].tolist()} {resp[bad[:3]].tolist()}, "
                           f"expected {e_kp[bad[:3]].tolist()} {e_resp[bad[:3]].tolist()}")
    return info


# ------------------------------------------------------------------------------------------------------------ ORB
ORB_CASES = [
    ("blobs 70x67, 3 levels", lambda: F.blob_frame(70, 67, n_blobs=30), dict(nfeatures=20, nlevels=3, edge=22)),
    ("noise 45x47, one level, a 1x3 interior", lambda: F.noise_frame(45, 47, 1), dict(nfeatures=2, nlevels=1, edge=22)),
    ("noise 70x67, 8 levels asked", lambda: F.noise_frame(70, 67, 2), dict(nfeatures=12, nlevels=8, edge=22)),
    ("noise 96x128 float32, 3 levels", lambda: (F.noise_frame(96, 128, 3) / np.float32(255.0)).astype(np.float32), dict(nfeatures=60, nlevels=3)),
    ("blobs 96x128, 8 levels asked", lambda: F.blob_frame(96, 128, n_blobs=60), dict(nfeatures=100, nlevels=8)),
    ("checkerboard 96x128, 3 levels", lambda: F.checker_frame(96, 128), dict(nlevels=3)),
    ("blobs 224x224, 8 levels", lambda: F.blob_frame(224, 224), dict()),
    ("noise 224x224, 8 levels, threshold 35", lambda: F.noise_frame(224, 224, 6), dict(fast_threshold=35)),
]


@pytest.mark.parametrize("what,make,kw", ORB_CASES, ids=[c[0] for c in ORB_CASES])
def test_orb_against_the_restatement(m, what, make, kw):
    frame = make()
    info = check_orb(run_orb(m, frame, **kw), frame, what, **kw)
    if "8 levels asked" in what:
        assert len(info["levels"]) < 8                                              # some levels are not built
    print(f"[loop] {what}: (survivors, kept, cut, at the cut) per level {info['cuts']}")


def test_orb_cut_with_ties_and_candidates_either_side_of_n(m):
    frame, kw = F.noise_frame(96, 128, 2), dict(nfeatures=80, nlevels=3)
    info = check_orb(run_orb(m, frame, **kw), frame, "noise 96x128, tied cut", **kw)
    surv, kept, cut, at_cut = info["cuts"][0]
    assert cut is not None and kept > 2 * info["nfeat"][0] and at_cut >= 2          # the cut is active and its ties extend it
    assert kept > info["nfeat"][0] and info["cuts"][2][1] < info["nfeat"][2]        # more candidates than n_0, fewer than n_2


def test_orb_all_ties_and_the_empty_frame(m):
    dots = L.dot_frame(96, 128)
    sc = L.fast_scores(dots, 20)
    assert (sc[31:-31, 31:-31] > 0).sum() >= 100 and len(L.survivors(sc, 31)[0]) == 0   # corners, every NMS comparison a tie
    got = run_orb(m, dots, nlevels=1)
    assert len(got[0]) == 0
    check_orb(got, dots, "dots", nlevels=1)
    const = L.constant_frame(96, 128)
    got = run_orb(m, const)
    assert len(got[0]) == 0
    check_orb(got, const, "constant")


def test_orb_orientations_over_the_circle(m):
    frame, centres, _ = L.disc_frame(16, 22)
    kw = dict(nfeatures=2000, nlevels=1)
    e_kp, _, _ = L.extract(frame, pattern=PATTERN, trig=TRIG, **kw)
    at = {(int(y), int(x)): int(b) for x, y, _, b in e_kp}
    assert len(set(e_kp[:, 3].tolist())) >= 300                                     # the condition is on the inputs: the restatement's bins
    assert [at.get(centres[i]) for i in (0, 88, 176, 264)] == [0, 90, 180, 270]    # the four axis discs hit their bins exactly
    check_orb(run_orb(m, frame, **kw), frame, "discs", **kw)


def test_orb_refusals_and_pattern(m):
    from vista_slam_amd import _lib, loop
    frame = F.blob_frame(70, 67, n_blobs=30)
    other = L.default_pattern(seed=99)
    kw = dict(nfeatures=20, nlevels=2, edge=22)
    check_orb(run_orb(m, frame, pattern=other, **kw), frame, "another table", pattern=other, **kw)
    p = loop.plan(70, 67, 20, 2, 20, 22)
    src, trig, pat, ws = _up(frame), _up(TRIG), _up(PATTERN), _filled(p.workspace_bytes)
    out = [_filled(p.rows * 16), _filled(p.rows * 8), _filled(p.rows * 32), _filled(4)]
    args = lambda **o: (m._h, src.data_ptr(), 0, 70, 67, 20, 2, 20, o.get("edge", 22), trig.data_ptr(), pat.data_ptr(), ws.data_ptr(),
                        o.get("bytes", p.workspace_bytes), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), m._stream())
    assert m.lib.sta_orb_extract(*args(bytes=p.workspace_bytes - 1)) == -1 and b"workspace" in m.lib.sta_last_error()
    assert m.lib.sta_orb_extract(*args(edge=21)) == -1 and b"edge" in m.lib.sta_last_error()
    assert m.lib.sta_orb_extract(*args()) == 0
    import torch
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="14"):
        bad = PATTERN.copy()
        bad[0, 0] = 14
        loop.orb(m, frame, pattern=bad, **kw)


# ------------------------------------------------------------------------------------------------------------ bag of words
def run_transform(m, V, desc, n_dev=None, cap=None):
    """-> (words, counts, vals) through the C ABI; cap > n with a device count exercises the rows that must not be read"""
    import torch
    from vista_slam_amd import _lib
    n = len(desc)
    cap = n if cap is None else cap
    rows = np.full((cap, 32), 0x5A, np.uint8)
    rows[:n] = desc
    d, nd = _up(rows), (_up(np.array([n_dev], np.int32)) if n_dev is not None else None)
    arrays = [_up(a) for a in (V.node_desc, V.child_first, V.child_count, V.word_of, V.word_weight if len(V.word_weight) else np.zeros(1))]
    ws = _filled(4 * cap + GUARD)
    words, counts, vals, nw = _filled((cap + GUARD) * 4), _filled((cap + GUARD) * 4), _filled((cap + GUARD) * 8), _filled(4 + GUARD)
    _lib.check(m.lib.sta_bow_transform(m._h, d.data_ptr(), nd.data_ptr() if nd is not None else None, cap, *(a.data_ptr() for a in arrays),
                                       len(V.child_first), len(V.word_weight), ws.data_ptr(), 4 * cap, words.data_ptr(), counts.data_ptr(),
                                       vals.data_ptr(), nw.data_ptr(), m._stream()))
    torch.cuda.synchronize()
    w, c, v, k, wsr = (t.cpu().numpy() for t in (words, counts, vals, nw, ws))
    cnt = int(k[:4].view(np.int32)[0])
    assert 0 <= cnt <= cap, cnt
    assert (k[4:] == FILL).all() and (w[cnt * 4:] == FILL).all() and (c[cnt * 4:] == FILL).all() and (v[cnt * 8:] == FILL).all(), \
        "entries at or past n_words were written"
    assert (wsr[4 * cap:] == FILL).all(), "bytes behind the workspace were written"
    return w[:cnt * 4].view(np.int32).copy(), c[:cnt * 4].view(np.int32).copy(), v[:cnt * 8].view(np.float64).copy()


def check_transform(got, exp, what):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (what, len(got[0]), len(exp[0]))
    assert len(got[2]) == len(exp[2]) and (len(exp[2]) == 0 or np.abs(got[2] - exp[2]).max() <= 1e-12), what


VOCABS = {
    "k2 L1": (2, 1, {}), "k10 L3 duplicated siblings": (10, 3, dict(dup_siblings=True)), "k64 L2": (64, 2, {}),
    "unbalanced k4 L4": (4, 4, dict(unbalanced=True)), "zero-weight words": (5, 3, dict(zero_words=0.3)), "all weights zero": (3, 2, dict(zero_words=1.0)),
}
_vocab_cache = {}


def vocab(name):
    if name not in _vocab_cache:
        k, L_, kw = VOCABS[name]
        _vocab_cache[name] = L.vocab_arrays(L.make_vocab(k, L_, seed=len(name), **kw))
    return _vocab_cache[name]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 500])
def test_bow_transform_descriptor_counts(m, n):
    V = vocab("k10 L3 duplicated siblings")
    desc = L.random_desc(n, n, V)
    if n >= 63:
        desc[5] = V.node_desc[V.child_first[0]]                                     # exactly the duplicated pair's descriptor: distance 0 twice
    exp = L.transform(desc, V)
    check_transform(run_transform(m, V, desc), exp, n)
    check_transform(run_transform(m, V, desc, n_dev=n, cap=n + 7), exp, (n, "device count"))
    check_transform(run_transform(m, V, desc, n_dev=n + 100, cap=n), exp, (n, "device count above the capacity"))


@pytest.mark.parametrize("name", list(VOCABS))
def test_bow_transform_vocabularies(m, name):
    V = vocab(name)
    desc = L.random_desc(65, 3, V)
    exp = L.transform(desc, V)
    assert (len(exp[0]) == 0) == (name == "all weights zero")                       # an empty vector is a result
    if name == "zero-weight words":
        assert 0 < exp[1].sum() < 65                                                # some descriptors fall on dropped words
    check_transform(run_transform(m, V, desc), exp, name)
    check_transform(run_transform(m, V, desc, n_dev=0, cap=65), L.transform(desc[:0], V), (name, "no descriptor"))


def make_database(rows, cap, n_words, seed, empty=()):
    """rows synthetic vectors: sorted distinct words and positive L1-normalised values -> (words [rows,cap], vals [rows,cap], n [rows])"""
    rng = np.random.RandomState(seed)
    words, vals, n = np.full((rows, cap), -7, np.int32), np.full((rows, cap), np.nan), np.zeros(rows, np.int32)
    for r in range(rows):
        if r in empty:
            continue
        k = int(rng.randint(1, cap + 1))
        words[r, :k] = np.sort(rng.choice(n_words, k, replace=False))
        v = rng.rand(k) + 0.01
        vals[r, :k] = v / v.sum()
        n[r] = k
    return words, vals, n


def run_score(m, q, db, rows):
    import torch
    from vista_slam_amd import _lib
    cap = db[0].shape[1]
    q_cap = len(q[0]) + 5                                                           # the query's capacity is its own: above or below the rows'
    qw, qv = np.full(q_cap, -3, np.int32), np.full(q_cap, np.nan)
    qw[:len(q[0])], qv[:len(q[0])] = q[0], q[1]
    t = [_up(a) for a in (qw, qv, np.array([len(q[0])], np.int32), db[0], db[1], db[2], np.asarray(rows, np.int32))]
    sim = _filled((len(rows) + GUARD) * 8)
    _lib.check(m.lib.sta_bow_score(m._h, *(a.data_ptr() for a in t[:3]), q_cap, *(a.data_ptr() for a in t[3:6]), db[0].shape[0], cap, t[6].data_ptr(),
                                   len(rows), sim.data_ptr(), m._stream()))
    torch.cuda.synchronize()
    raw = sim.cpu().numpy()
    assert (raw[len(rows) * 8:] == FILL).all(), "bytes behind sim were written"
    return raw[:len(rows) * 8].view(np.float64).copy()


@pytest.mark.parametrize("views,empty", [(1, ()), (5, (2,)), (400, (0, 17, 399))])
def test_bow_score_database(m, views, empty):
    cap = 96
    db = make_database(views, cap, 300, views, empty)
    src = views - 1 if views - 1 not in empty else 1
    q = (db[0][src, :db[2][src]].copy(), db[1][src, :db[2][src]].copy())
    rows = list(range(views)) + [src, 0]                                            # any rows, in any order, repeats allowed
    got = run_score(m, q, db, rows)
    exp = np.array([L.score(q, (db[0][r, :db[2][r]], db[1][r, :db[2][r]])) for r in rows])
    assert np.abs(got - exp).max() <= 1e-12, (views, float(np.abs(got - exp).max()))
    assert abs(got[src] - 1.0) <= 1e-12                                             # identical vectors
    assert all(got[r] == 0.0 for r in empty)                                        # an empty row shares no word
    assert np.array_equal(got, run_score(m, q, db, rows))                           # two runs are bit-identical
    # a query of 200 words against rows of at most 96: every common word counts, those behind position 96 of the query included
    rng = np.random.RandomState(views)
    long_q = (np.sort(rng.choice(300, 200, replace=False)).astype(np.int32), np.full(200, 1.0 / 200))
    exp = np.array([L.score(long_q, (db[0][r, :db[2][r]], db[1][r, :db[2][r]])) for r in rows])
    full = [r for r in range(views) if db[2][r] > 0]
    assert any(np.intersect1d(long_q[0][cap:], db[0][r, :db[2][r]]).size >= 3 for r in full)    # common words past the rows' capacity
    assert np.abs(run_score(m, long_q, db, rows) - exp).max() <= 1e-12
    # a vector of words the database does not hold scores exactly 0 against every row; so does the empty query
    far = (np.arange(300, 300 + 10, dtype=np.int32), np.full(10, 0.1))
    assert (run_score(m, far, db, rows) == 0.0).all()
    assert (run_score(m, (np.zeros(0, np.int32), np.zeros(0)), db, rows) == 0.0).all()


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_returns_device_tensors(m, tmp_path):
    import torch
    from vista_slam_amd import loop
    frame = F.blob_frame(96, 128, n_blobs=60)
    kw = dict(nfeatures=100, nlevels=3)
    e_kp, e_resp, e_desc = L.extract(frame, pattern=PATTERN, trig=TRIG, **kw)
    as_f32 = (frame / np.float32(255.0)).astype(np.float32)                        # trunc(fp32(g / 255) * 255) need not give g back
    f_kp, f_resp, f_desc = L.extract(as_f32, pattern=PATTERN, trig=TRIG, **kw)
    for img, exp in ((torch.from_numpy(as_f32)[None].cuda(), (f_kp, f_resp, f_desc)), (frame, (e_kp, e_resp, e_desc)),
                     (torch.from_numpy(frame).cuda(), (e_kp, e_resp, e_desc))):
        kp, resp, desc = loop.orb(m, img, **kw)
        assert kp.is_cuda and kp.dtype == torch.int32 and resp.dtype == torch.int64 and desc.dtype == torch.uint8
        assert all(np.array_equal(g.cpu().numpy(), e) for g, e in zip((kp, resp, desc), exp))
    rows = L.make_vocab(10, 3, seed=5)
    L.write_vocab(tmp_path / "voc.txt", rows, 10, 3)
    V = L.vocab_arrays(rows)
    voc = loop.Vocabulary.load(tmp_path / "voc.txt", m)
    a, b = voc.transform(desc), voc.transform(L.random_desc(40, 8, V))
    ea, eb = L.transform(e_desc, V), L.transform(L.random_desc(40, 8, V), V)
    check_transform(a.numpy(), ea, "Vocabulary.transform")
    assert abs(voc.score(a, b) - L.score((ea[0], ea[2]), (eb[0], eb[2]))) <= 1e-12 and abs(voc.score(a, a) - 1.0) <= 1e-12
    det = loop.LoopDetector(m, voc, 10, 5, 3, **kw)
    assert det.compute_bow_feat(L.constant_frame(96, 128)) is None and det.bow_feats == [None]       # no descriptor: None, as the reference
    v = det.compute_bow_feat(frame)
    check_transform(v.numpy(), ea, "compute_bow_feat")
    assert det.detect_loop(frame, 0) == [] and len(det.bow_feats) == 3 and abs(det.last[1] - 1.0) <= 1e-12 and det.last[0] == 0.0
    det.reset()
    assert det.bow_feats == [] and (det.loop_dist_min, det.loop_nms, det.loop_cand_thresh_neighbor) == (10, 5, 3)


def test_vocabulary_score_on_vectors_of_different_capacity(m):
    """`score(a, b)` with more words in a than b has room for, in both argument orders, against the restatement."""
    from vista_slam_amd import loop
    V = L.vocab_arrays(L.make_vocab(10, 2, seed=5))                                 # 100 words: the two vectors share many
    voc = loop.Vocabulary.from_arrays(V.node_desc, V.child_first, V.child_count, V.word_of, V.word_weight).bind(m)
    da, db_ = L.random_desc(500, 21, V), L.random_desc(40, 22, V)
    ea, eb = L.transform(da, V), L.transform(db_, V)
    common = np.intersect1d(ea[0], eb[0])
    assert len(ea[0]) > 40 >= len(eb[0]) and len(common) >= 10                      # n_a > cap_b, several common words ...
    assert np.isin(common, ea[0][40:]).sum() >= 3                                   # ... some of them behind position cap_b of a
    a, b = voc.transform(da), voc.transform(db_)
    assert a.words.shape[0] == 500 and b.words.shape[0] == 40
    exp = L.score((ea[0], ea[2]), (eb[0], eb[2]))
    assert 0.0 < exp < 1.0
    assert abs(voc.score(a, b) - exp) <= 1e-12 and abs(voc.score(b, a) - exp) <= 1e-12


def test_detector_refuses_another_frame_size_until_reset(m):
    from vista_slam_amd import loop
    V = L.vocab_arrays(L.make_vocab(10, 2, seed=5))
    voc = loop.Vocabulary.from_arrays(V.node_desc, V.child_first, V.child_count, V.word_of, V.word_weight)
    det = loop.LoopDetector(m, voc, 10, 5, 3, nfeatures=100, nlevels=3)
    det.detect_loop(F.blob_frame(96, 128, n_blobs=60), 0)
    with pytest.raises(ValueError, match="96 x 160 after frames of 96 x 128"):
        det.detect_loop(F.blob_frame(96, 160, n_blobs=60), 0)
    assert len(det.bow_feats) == 1                                                  # the refused frame left no view behind
    det.reset()
    assert det.detect_loop(F.blob_frame(96, 160, n_blobs=60), 0) == [] and len(det.bow_feats) == 1


# ------------------------------------------------------------------------------------------------------------ end to end
def test_detect_loop_on_a_sequence_that_returns(m):
    """60 frames pan away and come back; the candidate lists equal the restatement's.  The restatement's own numbers are checked first:
    no similarity sits within 1e-9 of its threshold (the two sides may differ by 1e-12), some frame has several candidates, some view is
    skipped by the NMS window alone.  The database starts smaller than the sequence, so it grows on the way; no device call allocates
    or synchronises."""
    import torch
    from vista_slam_amd import loop
    dist_min, nms, nb = 10, 5, 3
    kw = dict(nfeatures=300, nlevels=3, edge=22)
    V = L.vocab_arrays(L.make_vocab(10, 2, seed=5))                                 # 100 words: neighbouring frames always share some
    seq = L.loop_sequence()
    feats, exp, margins, skips = [], [], [], 0
    for i, f in enumerate(seq):
        d = L.extract(f, pattern=PATTERN, trig=TRIG, **kw)[2]
        feats.append(None if len(d) == 0 else L.transform(d, V))
        present = [x is not None for x in feats]
        sim = [L.score((feats[i][0], feats[i][2]), (feats[j][0], feats[j][2])) if present[i] and present[j] else 0.0 for j in range(i)]
        far = max(0, i - nb)
        exp.append(L.reference_detect_loop(list(feats), lambda a, b: L.score((a[0], a[2]), (b[0], b[2])), dist_min, nms, nb, far))
        mg, sk = L.detect_loop_margins(present, sim, i, far, dist_min, nms, nb)
        margins.append(mg)
        skips += sk
    assert min(margins) > 1e-9, min(margins)
    assert any(len(c) >= 2 for c in exp) and skips >= 1, (skips, [len(c) for c in exp])
    voc = loop.Vocabulary.from_arrays(V.node_desc, V.child_first, V.child_count, V.word_of, V.word_weight)
    det = loop.LoopDetector(m, voc, dist_min, nms, nb, max_views=32, **kw)
    det.detect_loop(seq[0], 0)                                                      # workspaces exist from here on
    det.reset()
    torch.cuda.synchronize()
    before = m.alloc_stats()
    got = [det.detect_loop(torch.from_numpy(f).cuda() if i % 2 else f, max(0, i - nb)) for i, f in enumerate(seq)]
    assert m.alloc_stats() == before
    assert det.max_views == 64 and len(det.bow_feats) == 60
    for i, (g, e) in enumerate(zip(got, exp)):
        assert [j for j, _ in g] == [j for j, _ in e], (i, g, e)
        assert all(abs(a[1] - b[1]) <= 1e-12 for a, b in zip(g, e)), (i, g, e)
    print("[loop] sequence:", " ".join(f"{i}:{[j for j, _ in c]}" for i, c in enumerate(exp) if c))
