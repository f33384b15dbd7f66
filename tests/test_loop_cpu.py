"""Host only: the loop-candidate contract (include/sta_mi355.h: sta_orb_extract / sta_bow_transform / sta_bow_score) - the numpy
restatement tests/loop_cases.py against its naive second statement, sta_orb_plan's values and refusals through the built library, the
vocabulary loader, the tables of the contract, the angle-bin rule, and detect_loop's host logic against a literal transcription of
the reference's lines."""
import ctypes as C

import numpy as np
import pytest

import flow_cases as F
import loop_cases as L


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("name,frame,kw", [
    ("blobs 70x67", F.blob_frame(70, 67, n_blobs=30), dict(edge=22, nlevels=3, nfeatures=20)),
    ("noise 70x67, cut active", F.noise_frame(70, 67, 2), dict(edge=22, nlevels=3, nfeatures=12)),
    ("noise 45x47, a 1x3 interior", F.noise_frame(45, 47, 1), dict(edge=22, nlevels=1, nfeatures=2)),
    ("dots 70x67, all ties", L.dot_frame(70, 67), dict(edge=22, nlevels=1, nfeatures=50)),
    ("float32 frame", (F.noise_frame(70, 67, 4) / np.float32(255.0)).astype(np.float32), dict(edge=22, nlevels=2, nfeatures=30)),
])
def test_restatement_equals_the_naive_statement(name, frame, kw):
    got, exp = L.extract(frame, **kw), L.naive_extract(frame, **kw)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.uint8
    assert _same(got, exp), (name, len(got[0]), len(exp[0]))


def test_restatement_frames_do_what_they_are_for():
    info = {}
    kp, _, _ = L.extract(F.noise_frame(70, 67, 2), edge=22, nlevels=3, nfeatures=12, info=info)
    assert len(kp) > 0 and info["cuts"][0][2] is not None                          # the naive comparison above saw an active cut
    sc = L.fast_scores(L.dot_frame(70, 67), 20)
    assert (sc[22:-22, 22:-22] > 0).sum() >= 16 and len(L.survivors(sc, 22)[0]) == 0   # corners, every one tied with a neighbour


@pytest.mark.parametrize("k,L_,kw,n", [(2, 1, {}, 9), (10, 3, dict(dup_siblings=True), 65), (4, 4, dict(unbalanced=True), 64),
                                       (5, 2, dict(zero_words=0.3), 63), (3, 2, dict(zero_words=1.0), 20)])
def test_bow_restatement_equals_the_naive_statement(k, L_, kw, n):
    V = L.vocab_arrays(L.make_vocab(k, L_, seed=k + L_, **kw))
    a, b = L.random_desc(n, 1, V), L.random_desc(n + 3, 2, V)
    ta, tb = L.transform(a, V), L.transform(b, V)
    na, nb = L.naive_transform(a, V), L.naive_transform(b, V)
    for t, nv in ((ta, na), (tb, nb)):
        assert t[0].tolist() == nv[0] and t[1].tolist() == nv[1]
        assert np.allclose(t[2], nv[2], rtol=0, atol=1e-15) and (len(nv[0]) == 0 or abs(t[2].sum() - 1.0) < 1e-12)
    if kw.get("zero_words") == 1.0:
        assert len(ta[0]) == 0
    assert abs(L.score((ta[0], ta[2]), (tb[0], tb[2])) - L.naive_score((na[0], na[2]), (nb[0], nb[2]))) <= 1e-15
    if len(ta[0]):
        assert abs(L.score((ta[0], ta[2]), (ta[0], ta[2])) - 1.0) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ plan
def test_plan_pins_the_size_tables():
    from vista_slam_amd import loop
    p = loop.plan(224, 224)
    assert [w for _, w in p.sizes] == [224, 187, 156, 130, 108, 90, 75, 63] and all(h == w for h, w in p.sizes)
    assert p.nfeat == (109, 90, 75, 63, 52, 44, 36, 31) and sum(p.nfeat) == 500 == p.rows and p.built == 8
    q = loop.plan(384, 512)
    assert q.sizes == ((384, 512), (320, 427), (267, 356), (222, 296), (185, 247), (154, 206), (129, 171), (107, 143)) and q.built == 8
    assert q.nfeat == p.nfeat
    for H, W, nf, nl, e in [(224, 224, 500, 8, 31), (384, 512, 500, 8, 31), (70, 67, 20, 3, 22), (45, 47, 2, 1, 22), (96, 128, 60, 8, 31),
                            (100, 1000, 4096, 8, 22), (224, 224, 7, 8, 31), (224, 224, 1, 8, 31)]:
        p = loop.plan(H, W, nf, nl, 20, e)
        sizes = L.level_sizes(H, W, nl)
        assert list(p.sizes) == sizes and list(p.nfeat) == L.level_features(nf, nl) and p.built == L.built_levels(sizes, e), (H, W, nf, nl, e)
        assert p.rows == max(nf, sum(p.nfeat))
        # the built levels lie one behind the other in a plane, 256-byte aligned
        end = 0
        for (h, w), o in zip(p.sizes, p.offsets):
            assert o == end and o % 256 == 0
            end += (h * w + 255) // 256 * 256
        assert p.plane_bytes == end and p.workspace_bytes >= 4 * end and p.bow_workspace_bytes >= 4 * p.rows
    assert loop.plan(96, 128, 60, 8, 20, 31).built == 3                            # 67 x 89, then 56 x 74 <= 62: not built
    assert loop.plan(224, 224, 7, 8).rows == 8                                     # the one rounding that overshoots nfeatures


@pytest.mark.parametrize("args,word", [
    ((224, 224, 500, 0, 20, 31), "nlevels"), ((224, 224, 500, 9, 20, 31), "nlevels"), ((224, 224, 0, 8, 20, 31), "nfeatures"),
    ((224, 224, 4097, 8, 20, 31), "nfeatures"), ((224, 224, 500, 8, 20, 21), "edge"), ((224, 224, 500, 8, 20, 65), "edge"),
    ((224, 224, 500, 8, 0, 31), "fast_threshold"), ((224, 224, 500, 8, 255, 31), "fast_threshold"), ((62, 224, 500, 8, 20, 31), "62 x 224"),
    ((224, 44, 500, 8, 20, 22), "224 x 44"), ((2048, 1025, 500, 8, 20, 31), "pixels")])
def test_plan_refuses_with_the_numbers(args, word):
    from vista_slam_amd import _lib, loop
    with pytest.raises(ValueError, match=word):
        loop.plan(*args)
    assert _lib.load().sta_orb_plan(*args, (C.c_int64 * 40)()) == -1
    assert loop.plan(63, 63, 1, 1, 1, 31).built == 1 and loop.plan(1024, 2048, 4096, 8, 254, 64).built == 8      # the limits themselves pass


def test_ctypes_table_mirrors_the_header():
    from vista_slam_amd import _lib
    _vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
    assert _lib.SIGNATURES["sta_orb_plan"] == (_i, [_i] * 6 + [C.POINTER(_i64)])
    assert _lib.SIGNATURES["sta_orb_extract"] == (_i, [_vp, _vp] + [_i] * 7 + [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp])
    assert _lib.SIGNATURES["sta_bow_transform"] == (_i, [_vp, _vp, _vp, _i] + [_vp] * 5 + [_i, _i, _vp, _i64] + [_vp] * 5)
    assert _lib.SIGNATURES["sta_bow_score"] == (_i, [_vp] * 4 + [_i] + [_vp] * 3 + [_i, _i, _vp, _i, _vp, _vp])


# ------------------------------------------------------------------------------------------------------------ tables
def test_tables_of_the_contract():
    from vista_slam_amd import loop
    assert L.umax_construction() == L.UMAX == loop.UMAX
    assert np.array_equal(loop.trig_table(), L.trig_table()) and loop.trig_table().dtype == np.int32 and loop.trig_table().shape == (720, 2)
    assert loop.trig_table()[0].tolist() == [1 << 30, 0] and loop.trig_table()[180].tolist() == [0, 1 << 30]
    p = loop.default_pattern()
    assert np.array_equal(p, L.default_pattern()) and p.dtype == np.int8 and p.shape == (256, 4) and np.abs(p).max() <= 13
    assert ((p[:, 0] != p[:, 2]) | (p[:, 1] != p[:, 3])).all() and len({tuple(r) for r in p.tolist()}) > 250
    bad = p.copy()
    bad[7, 2] = 14
    with pytest.raises(ValueError, match="14"):
        loop.check_pattern(bad)
    with pytest.raises(ValueError):
        loop.check_pattern(p[:255])
    # a rotated point stays within 19 of the keypoint for every bin: with edge >= 22 no read leaves the level
    rx, ry = L.rotate(np.array([[13, 13, -13, 13]] * 256, np.int8), np.arange(360), L.trig_table())
    assert max(np.abs(rx).max(), np.abs(ry).max()) <= 19


def test_bin_rule_gives_exactly_one_bin():
    trig = L.trig_table()
    rng = np.random.RandomState(5)
    vecs = rng.randint(-(1 << 22), 1 << 22, (100000, 2)).tolist() + rng.randint(-20, 21, (2000, 2)).tolist()
    t = trig.astype(np.int64)
    k = np.arange(360)
    lo, hi = t[(2 * k - 1) % 720], t[2 * k + 1]
    v = np.array([p for p in vecs if p != [0, 0]], np.int64)
    ok = (lo[None, :, 0] * v[:, None, 1] - lo[None, :, 1] * v[:, None, 0] >= 0) & (hi[None, :, 0] * v[:, None, 1] - hi[None, :, 1] * v[:, None, 0] < 0)
    assert (ok.sum(1) == 1).all()
    deg = np.rad2deg(np.arctan2(v[:, 1].astype(np.float64), v[:, 0].astype(np.float64))) % 360.0
    diff = np.abs((ok.argmax(1) - deg + 180.0) % 360.0 - 180.0)
    assert diff.max() <= 0.5 + 1e-6                                                 # the bin is the nearest whole degree
    for m, want in [((5, 0), 0), ((0, 5), 90), ((-5, 0), 180), ((0, -5), 270), ((3, 3), 45), ((-3, 3), 135), ((-3, -3), 225), ((3, -3), 315),
                    ((1 << 22, 0), 0), ((0, -(1 << 22)), 270)]:
        assert L.angle_bin(m[0], m[1], trig) == (want, 1), m
    assert L.angle_bin(0, 0, trig) == (0, 0)


# ------------------------------------------------------------------------------------------------------------ vocabulary
def _check_loaded(v, rows):
    e = L.vocab_arrays(rows)
    assert np.array_equal(v.node_desc, e.node_desc) and np.array_equal(v.child_first, e.child_first) and np.array_equal(v.child_count, e.child_count)
    assert np.array_equal(v.word_of, e.word_of) and np.array_equal(v.word_weight, e.word_weight)
    assert v.node_desc.dtype == np.uint8 and v.child_first.dtype == np.int32 and v.word_weight.dtype == np.float64


def test_vocabulary_loader_round_trip(tmp_path):
    from vista_slam_amd import loop
    for name, k, L_, kw in [("balanced", 3, 3, {}), ("unbalanced", 4, 4, dict(unbalanced=True)), ("k64", 64, 1, {}), ("zeros", 5, 2, dict(zero_words=0.3))]:
        rows = L.make_vocab(k, L_, seed=9, **kw)
        L.write_vocab(tmp_path / f"{name}.txt", rows, k, L_)
        v = loop.Vocabulary.load(tmp_path / f"{name}.txt")
        _check_loaded(v, rows)
        assert (v.k, v.L) == (k, L_) and v.n_nodes == len(rows) + 1 and v.n_words == sum(r[1] for r in rows)
        v.save(tmp_path / f"{name}.npz")
        _check_loaded(loop.Vocabulary.load(tmp_path / f"{name}.npz"), rows)
        leaves = np.flatnonzero(v.child_count == 0)
        if name == "unbalanced":                                                    # leaves at more than one depth
            depth = np.zeros(v.n_nodes, int)
            for i in np.flatnonzero(v.child_count > 0):
                depth[v.child_first[i]:v.child_first[i] + v.child_count[i]] = depth[i] + 1
            assert len(set(depth[leaves].tolist())) > 1
    rows = L.make_vocab(2, 2, seed=1)
    for scoring, weighting in [(1, 0), (0, 1), (3, 2)]:
        L.write_vocab(tmp_path / "other.txt", rows, 2, 2, scoring, weighting)
        with pytest.raises(ValueError, match=f"scoring {scoring}, weighting {weighting}"):
            loop.Vocabulary.load(tmp_path / "other.txt")
    e = L.vocab_arrays(rows)
    for field, value in [("child_first", 0), ("child_count", 65)]:
        arrays = {f: getattr(e, f).copy() for f in ("node_desc", "child_first", "child_count", "word_of", "word_weight")}
        arrays[field][0] = value
        with pytest.raises(ValueError):
            loop.Vocabulary.from_arrays(**arrays)
    with pytest.raises(RuntimeError, match="bind"):
        loop.Vocabulary.from_arrays(e.node_desc, e.child_first, e.child_count, e.word_of, e.word_weight).transform(np.zeros((1, 32), np.uint8))


# ------------------------------------------------------------------------------------------------------------ detect_loop's host logic
def test_candidates_equal_the_reference_lines():
    from vista_slam_amd import loop
    rng = np.random.RandomState(2)
    cases = 0
    for trial in range(300):
        i = int(rng.randint(0, 40))
        sim = np.round(rng.rand(i), 1 if trial % 2 else 6).tolist()                 # one decimal: many ties in similarity
        feats = [None if rng.rand() < 0.15 else j for j in range(i + 1)]            # a view's vector stands for its index
        if trial % 7 == 0:
            feats[i] = None
        dist_min, nms, nb = int(rng.randint(0, 12)), int(rng.randint(0, 8)), int(rng.randint(0, 5))
        for far in {0, max(0, i - 3), i, int(rng.randint(0, i + 1))}:
            exp = L.reference_detect_loop(feats, lambda a, b: sim[b], dist_min, nms, nb, far)
            got = loop.candidates([f is not None for f in feats], sim, i, far, dist_min, nms, nb)
            assert got == exp, (trial, i, far, got, exp)
            cases += len(exp) > 1
    assert cases > 50
    # hand-made: ties in similarity keep the scan order (stable sort), a None view is skipped, the comparison is strict
    sim = [0.5, 0.9, 0.5, 0.5, 0.2, 0.7, 0.2, 0.2]
    assert loop.candidates([True] * 9, sim, 8, 6, 1, 0, 3) == [(1, 0.9), (5, 0.7), (3, 0.5), (2, 0.5), (0, 0.5)]
    assert loop.candidates([True] * 9, sim, 8, 6, 1, 1, 3) == [(1, 0.9), (3, 0.5)]                # 5, 2 and 0 sit inside the window
    assert loop.candidates([True, False] + [True] * 7, sim, 8, 6, 1, 0, 3) == [(5, 0.7), (3, 0.5), (2, 0.5), (0, 0.5)]
    assert loop.candidates([True] * 9, [0.2] * 8, 8, 6, 1, 0, 3) == []             # equal to the threshold is not above it
    assert loop.candidates([True] * 8 + [False], sim, 8, 6, 1, 0, 3) == []
    assert loop.candidates([True] * 9, sim, 8, 6, 1, 0, 0) == []                   # no neighbour: the threshold is 1.0
    assert L.detect_loop_margins([True] * 9, sim, 8, 6, 1, 1, 3)[1] == 3           # views 5, 2 and 0 fall to the NMS window alone
