"""Host only: tests/dist_cases.py, the numpy restatement of include/sta_dist.h, held against a second, independent statement - the closest
point as the best of the plane projection (when it falls inside the triangle) and the three segment projections, in numpy.longdouble -,
against the geometry of a sphere, and against the property the search rests on: on hostile floats the computed bound of every node is <=
the computed d2 of every triangle below it.  Plus `meshdist.plan` (sizes and refusals need no GPU) and the key and order restatements."""
import numpy as np
import pytest

import dist_cases as D
import surf_cases as SF

LD = np.longdouble


# ------------------------------------------------------------------------------------------ the second statement
def _segment(q, a, b):
    ab = b - a
    t = np.clip(((q - a) * ab).sum(-1) / (ab * ab).sum(-1), 0, 1)
    d = q - (a + ab * t[..., None])
    return np.sqrt((d * d).sum(-1))


def second_statement(q, a, b, c):
    """distance [n] from q [n,3] to the triangles (a, b, c) [n,3] in longdouble, not one line of it shared with dist_cases.closest"""
    q, a, b, c = (np.asarray(x, dtype=np.float32).astype(LD) for x in (q, a, b, c))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    h = ((q - a) * n).sum(-1) / nn
    p = q - n * h[..., None]                      # the projection into the plane
    inside = np.ones(len(q), dtype=bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, p - u) * n).sum(-1) >= 0
    best = np.minimum(np.minimum(_segment(q, a, b), _segment(q, b, c)), _segment(q, c, a))
    plane = np.abs(h) * np.sqrt(nn)
    return np.where(inside, np.minimum(plane, best), best)


def _pairs():
    """(q, a, b, c) [n,3] float32: the region queries on one triangle, the lattice queries on every lattice triangle, and 4000 random
    pairs over six decades of scale"""
    out = []
    v, t = D.one_triangle()
    q = D.regions()
    out.append((q,) + tuple(np.repeat(v[t[:, k]], len(q), axis=0) for k in range(3)))
    v, t = D.lattice()
    q = D.lattice_queries()
    qi, ti = np.meshgrid(np.arange(len(q)), np.arange(len(t)), indexing="ij")
    out.append((q[qi.ravel()],) + tuple(v[t[ti.ravel(), k]] for k in range(3)))
    r = np.random.default_rng(12)
    s = 10.0 ** r.integers(-3, 4, (4000, 1))
    out.append(tuple((r.standard_normal((4000, 3)) * s).astype(np.float32) for _ in range(4)))
    return [np.concatenate([o[k] for o in out]) for k in range(4)]


def test_the_restatement_agrees_with_projections_in_extended_precision():
    q, a, b, c = _pairs()
    _c, d2 = D.closest(q, a, b, c)
    ref = second_statement(q, a, b, c)
    scale = np.max(np.abs(np.concatenate([q, a, b, c], axis=1)), axis=1).astype(LD)
    err = float(np.max(np.abs(np.sqrt(d2.astype(LD)) - ref) / scale))
    print(f"[dist cpu] {len(q)} pairs: largest |restatement - longdouble statement| / scale = {err:.3e} "
          f"(recorded {D.SECOND_STATEMENT_MEASURED:.1e}, asserted x {D.SECOND_STATEMENT_FACTOR})")
    assert err <= D.SECOND_STATEMENT_FACTOR * D.SECOND_STATEMENT_MEASURED


def test_the_seven_regions_give_the_answers_known_by_hand():
    v, t = D.one_triangle()
    idx = D.Index(v, t)
    q = np.array([[1, 1, 3], [-1, -1, 0], [5, -1, 0], [-1, 5, 0], [2, -1, 0], [-1, 2, 0], [3, 3, 0], [6, -2, 1], [0.5, 0.25, -2]], dtype=np.float32)
    want = np.array([[1, 1, 0], [0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0], [4, 0, 0], [0.5, 0.25, 0]], dtype=np.float32)
    d2, tri, pt = D.brute(idx, q)
    assert np.array_equal(pt, want) and np.array_equal(tri, np.zeros(len(q), dtype=np.int32))
    assert np.array_equal(d2, ((q.astype(np.float64) - want) ** 2).sum(axis=1))
    # radius: inclusive, and one float64 step below is not enough
    assert D.brute(idx, q[:1], 3.0)[1][0] == 0 and D.brute(idx, q[:1], np.nextafter(3.0, 0.0))[1][0] == -1
    far = D.brute(idx, q[:1], np.nextafter(3.0, 0.0))
    assert far[0][0] == np.inf and np.isnan(far[2]).all()


def test_a_query_at_a_sphere_lies_between_its_inner_and_outer_radius():
    v, t, _ = SF.sphere()
    r_in, r_out = SF.sphere_radii()
    centre = np.asarray(SF.MC.SPHERE_CENTRE, dtype=np.float64)
    idx = D.Index(v, t)
    assert idx.n_valid == len(t)
    r = np.random.default_rng(3)
    dirs = r.standard_normal((40, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    for f in (0.0, 0.3, 0.9, 1.2, 2.0, 10.0):
        rho_nominal = f * r_out if f > 1 else f * r_in
        q = (centre + dirs * rho_nominal).astype(np.float32)
        rho = np.linalg.norm(q.astype(np.float64) - centre, axis=1)          # the radius of the rounded query
        d = np.sqrt(D.brute(idx, q)[0])
        lo, hi = np.minimum(np.abs(rho - r_out), np.abs(rho - r_in)), np.maximum(np.abs(rho - r_out), np.abs(rho - r_in))
        slack = 1e-12 * (rho + r_out)
        assert (d >= lo - slack).all() and (d <= hi + slack).all(), (f, float((lo - d).max()), float((d - hi).max()))


# ------------------------------------------------------------------------------------------ the property the search rests on
@pytest.mark.parametrize("case", ["hostile", "near_1e6", "lattice_with_bad", "same_centre"])
def test_every_nodes_bound_is_at_most_the_d2_of_every_triangle_below_it(case):
    if case == "hostile":
        (v, t), q = D.hostile_soup(), D.hostile_queries()
    elif case == "near_1e6":
        (v, t), q = D.soup(300, 2, 1.0, 0.2, 1.0e6), D.soup_queries(200, 3, 1.0, 1.0e6)
    elif case == "lattice_with_bad":
        (v, t), q = D.with_bad(*D.lattice()), D.lattice_queries()
    else:
        (v, t), q = D.same_centre(), D.soup_queries(200, 5, 8.0, -4.0)
    idx = D.Index(v, t)
    P = idx.tri[:idx.n_valid].reshape(-1, 3, 3)
    c, dd = D.closest(q[:, None, :], P[None, :, 0], P[None, :, 1], P[None, :, 2])          # [Q, n_valid]
    assert not np.isnan(dd).any()
    lo, hi = P.min(axis=1).astype(np.float64), P.max(axis=1).astype(np.float64)
    assert ((c >= lo[None]) & (c <= hi[None])).all(), "the clamped point lies inside the triangle's box exactly"
    pos = np.arange(idx.n_valid)
    for level, boxes in enumerate(idx.boxes):
        node = pos // D.FANOUT ** (level + 1)
        b = D.bound(boxes[None, :, :], q[:, None, :])                                  # [Q, count]
        assert (b[:, node] <= dd).all(), (case, level)
        empty = boxes[:, 0] > boxes[:, 3]
        assert np.array_equal(empty, ~np.isin(np.arange(len(boxes)), node))
        assert np.isposinf(b[:, empty]).all()
    assert len(idx.boxes[-1]) == 1 and len(idx.boxes) == len(D.level_counts(idx.nt))


# ------------------------------------------------------------------------------------------ key, order, plan
def test_the_key_is_the_bit_interleave_and_the_order_is_stable():
    r = np.random.default_rng(7)
    g = r.integers(0, 1 << 21, (50, 3))
    k = D.spread(g[:, 0]) | (D.spread(g[:, 1]) << np.uint64(1)) | (D.spread(g[:, 2]) << np.uint64(2))
    for row, key in zip(g, k):
        want = 0
        for b in range(21):
            for a in range(3):
                want |= ((int(row[a]) >> b) & 1) << (3 * b + a)
        assert int(key) == want
    v, t = D.with_bad(*D.reversed_duplicated(*D.lattice()))
    idx = D.Index(v, t)
    assert sorted(idx.src.tolist()) == list(range(len(t)))
    ks = idx.key[idx.src]
    assert (np.diff(ks.astype(np.float64)) >= 0).all() and (ks[:idx.n_valid] < D.INVALID_KEY).all() and (ks[idx.n_valid:] == D.INVALID_KEY).all()
    same = ks[1:] == ks[:-1]
    assert same.any() and (np.diff(idx.src)[same] > 0).all()
    assert idx.counters[:4].sum() == len(t) and np.isnan(idx.tri[idx.n_valid:]).all()
    # a planar mesh: U == L on z, so the z bits of every key are 0
    assert not (idx.key[idx.cls == D.VALID] & D.spread(np.uint64((1 << 21) - 1)) << np.uint64(2)).any()


def test_plan_gives_the_restated_sizes_and_refusals_without_a_gpu():
    from vista_slam_amd import meshdist
    F = D.FANOUT
    for nt in (1, F - 1, F, F + 1, F * F, F * F + 1, F ** 3 + 1, 1023, 1024, 1025, 2_000_000, (1 << 27) - 1):
        assert tuple(meshdist.plan(nt, 5)) == D.plan(nt, 5), nt
        assert meshdist.level_counts(nt) == D.level_counts(nt) and len(D.level_counts(nt)) <= D.MAX_LEVELS
    assert D.level_counts(F ** 3 + 1) == [F * F + 1, F + 1, 2, 1] and D.level_counts(1) == [1]
    for args in ((0, 1), (-3, 1), (1 << 27, 1), (5, 0), (5, 1 << 30)):
        with pytest.raises(ValueError) as mine:
            D.plan(*args)
        with pytest.raises(ValueError) as theirs:
            meshdist.plan(*args)
        assert str(mine.value) == str(theirs.value) and str(args[0] if "nt" in str(mine.value) else args[1]) in str(mine.value)
    assert (meshdist.FANOUT, meshdist.MAX_LEVELS, meshdist.KEY_BITS, meshdist.COUNTERS) == (D.FANOUT, D.MAX_LEVELS, D.KEY_BITS, D.COUNTERS)
