"""Host only: the numpy restatement of include/sta_surf.h (tests/surf_cases.py) held against second statements - the components against
a plain breadth-first search and against scipy's connected_components, the generator against its known answers and Python integers, the
prefix against a plain loop, the sampler against the properties the header promises (a non-decreasing prefix, no triangle of weight 0
chosen, the stratification bound, barycentric weights >= 0, samples between the mesh's own inner and outer radius) - and the arithmetic
of evaluate.eval_mesh on restated samples."""
import collections

import numpy as np
import pytest

import mesh_cases as MC
import surf_cases as SF


def _bfs(tris, nv):
    """(vlabel, tlabel, tcount) by a breadth-first search over vertex adjacency lists"""
    ok = SF.valid(tris, nv)
    adj = collections.defaultdict(set)
    named = set()
    for a, b, c in tris[ok].tolist():
        named.update((a, b, c))
        for x, y in ((a, b), (a, c), (b, c)):
            if x != y:
                adj[x].add(y)
                adj[y].add(x)
    vlabel = np.full(nv, -1, dtype=np.int32)
    for s in sorted(named):                  # ascending: the first vertex that reaches a component is its smallest
        if vlabel[s] >= 0:
            continue
        vlabel[s] = s
        queue = collections.deque([s])
        while queue:
            x = queue.popleft()
            for y in adj[x]:
                if vlabel[y] < 0:
                    vlabel[y] = s
                    queue.append(y)
    tlabel = np.where(ok, vlabel[np.clip(tris[:, 0], 0, max(nv - 1, 0))] if nv else -1, -1).astype(np.int32)
    tcount = np.zeros(nv, dtype=np.int32)
    for r in tlabel[ok].tolist():
        tcount[r] += 1
    return vlabel, tlabel, tcount


@pytest.mark.parametrize("name", list(SF.COMPONENT_CASES))
def test_components_equal_a_breadth_first_search(name):
    tris, nv = SF.COMPONENT_CASES[name]()
    got, want = SF.components(tris, nv), _bfs(tris, nv)
    for g, w, what in zip(got, want, ("vlabel", "tlabel", "tcount")):
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, what)
    vlabel, tlabel, tcount = got
    assert tcount.sum() == SF.valid(tris, nv).sum() and np.all((tcount > 0) <= (vlabel == np.arange(nv)))
    assert np.all(vlabel <= np.arange(nv))


@pytest.mark.parametrize("name", ["odd", "three_spheres", "strip_65536", "fan_4096", "soup", "islands"])
def test_components_equal_scipy(name):
    from scipy import sparse
    from scipy.sparse.csgraph import connected_components
    tris, nv = SF.COMPONENT_CASES[name]()
    tv = tris[SF.valid(tris, nv)]
    rows = np.concatenate([tv[:, 0], tv[:, 0], tv[:, 1]])
    cols = np.concatenate([tv[:, 1], tv[:, 2], tv[:, 2]])
    _n, lab = connected_components(sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv)), directed=False)
    smallest = np.full(lab.max() + 1, nv, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(nv))
    named = np.zeros(nv, dtype=bool)
    named[tv.reshape(-1)] = True
    assert np.array_equal(SF.components(tris, nv)[0], np.where(named, smallest[lab], -1))


def test_the_expected_shapes_of_the_component_cases():
    v, t = SF.three_spheres()
    vlabel, tlabel, tcount = SF.components(t, len(v))
    roots = np.nonzero(tcount)[0]
    assert len(roots) == 3 and tcount[roots].tolist() == [2124] * 3 and (vlabel >= 0).all()
    for tris, nv in (SF.strip(), SF.fan()):
        vlabel, tlabel, tcount = SF.components(tris, nv)
        assert (vlabel == 0).all() and (tlabel == 0).all() and tcount[0] == len(tris)
    tris, nv = SF.soup()
    vlabel, _tlabel, tcount = SF.components(tris, nv)
    assert np.count_nonzero(tcount) == 1 and 100 < (vlabel < 0).sum() < 400          # one giant component; e^-4.5 of the vertices are not named
    tris, nv = SF.islands()
    tcount = SF.components(tris, nv)[2]
    assert 2000 < np.count_nonzero(tcount) < 8000 and len(np.unique(tcount)) > 8       # many components, many sizes
    tris, nv = SF.odd()
    vlabel, tlabel, tcount = SF.components(tris, nv)
    assert vlabel.tolist() == [0, 0, 0, 3, 3, 5, -1, -1, 8, 8, 8, 3, 3, -1]
    assert tlabel.tolist() == [0, 0, 0, 3, 5, -1, -1, -1, 8, 8, 3, -1] and tcount.tolist() == [3, 0, 0, 2, 0, 1, 0, 0, 2, 0, 0, 0, 0, 0]
    # the order of the triangles does not matter
    p = np.random.default_rng(1).permutation(len(t))
    a, b = SF.components(t, len(v)), SF.components(t[p], len(v))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1][p], b[1])


def test_clean_keep_and_its_ties():
    tlabel = np.array([0, 0, 4, 4, 7, -1, 9, 9, 9], np.int32)
    tcount = np.zeros(12, np.int32)
    tcount[[0, 4, 7, 9]] = 2, 2, 1, 3
    assert SF.clean_keep(tlabel, tcount, min_triangles=2).tolist() == [True, True, True, True, False, False, True, True, True]
    assert SF.clean_keep(tlabel, tcount, keep_largest=2).tolist() == [True, True, False, False, False, False, True, True, True]      # 0 wins the tie with 4
    assert SF.clean_keep(tlabel, tcount, min_triangles=3, keep_largest=2).tolist() == [False] * 6 + [True] * 3
    assert not SF.clean_keep(tlabel, tcount, keep_largest=0).any()


def test_the_generator():
    for i, z in SF.KNOWN_ANSWERS.items():
        assert SF.mix_int(0, i) == z and int(SF.mix(0, np.array([i]))[0]) == z
    i = np.array([0, 1, 2, 3, 2 ** 31, 2 ** 33 + 7, 3 * (2 ** 31 - 1)], dtype=np.uint64)
    for seed in SF.SEEDS + (2 ** 64 - 1,):
        assert [int(z) for z in SF.mix(seed, i)] == [SF.mix_int(seed, int(k)) for k in i]
    u = SF.units(SF.SEEDS[1], 100001)
    assert u.shape == (100001, 3) and u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.005
    assert u[1, 0] == float(SF.mix_int(SF.SEEDS[1], 4) >> 11) * 2.0 ** -53


def test_the_plan():
    assert SF.plan(0, 0, 0) == (0, 0, 0) and SF.plan(1, 1, 1) == (256, 512, 0) and SF.plan(1025, 65, 9) == (512, 512, 0)
    assert SF.plan(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == (2 ** 33, 2 * 8 * 2 ** 21, 0)
    for args in ((-1, 0, 0), (0, 2 ** 31, 0), (0, 0, -5)):
        with pytest.raises(ValueError, match=r"must be in \[0, 2\^31\)"):
            SF.plan(*args)


@pytest.fixture(scope="module")
def sphere_samples():
    v, t, col = SF.sphere()
    return SF.sample(v, t, 100001, seed=0, colors=col, normals=True)


@pytest.fixture(scope="module")
def hostile_samples():
    v, t = SF.hostile()
    return SF.sample(v, t, 50000, seed=SF.SEEDS[1])


def test_the_prefix_is_the_loops_and_never_decreases(sphere_samples, hostile_samples):
    for s in (sphere_samples, hostile_samples):
        P, total = SF.prefix_loop(s["w"])
        assert np.array_equal(P, s["P"]) and total == s["total"] == s["P"][-1]
        assert np.all(np.diff(s["P"]) >= 0) and np.all(s["w"] >= 0) and np.isfinite(s["total"])
        rise = np.diff(np.concatenate([[0.0], s["P"]])) > 0
        assert np.all(s["w"][rise] > 0)                       # P[t] > P[t - 1] implies w_t > 0
    w = hostile_samples["w"]
    assert len(w) == 3073 and (w == 0).sum() >= 200 and np.log10(w[w > 0].max() / w[w > 0].min()) > 16
    for nt in SF.PREFIX_SIZES:
        w = SF.tri_weights(*SF.prefix_mesh(nt))
        P, total = SF.prefix(w)
        Pl, tl = SF.prefix_loop(w)
        assert np.array_equal(P, Pl) and total == tl and (w == 0).sum() >= (nt > 100)
    assert SF.prefix(np.zeros(0))[1] == 0.0 and len(SF.prefix(np.zeros(0))[0]) == 0


def test_no_triangle_of_weight_zero_is_chosen_and_the_strata_hold(sphere_samples, hostile_samples):
    for s, ns in ((sphere_samples, 100001), (hostile_samples, 50000)):
        t, w = s["tri"], s["w"]
        assert t.shape == (ns,) and t.min() >= 0 and np.all(w[t] > 0) and np.all(np.diff(t) >= 0)
        count = np.bincount(t, minlength=len(w))
        worst = np.abs(count - ns * w / s["total"]).max()
        print(f"[surf strata] ns = {ns}: the largest |count_t - ns w_t / total| is {worst:.3f}")
        assert worst < 2.0
        assert np.all(s["b"] >= 0) and np.all(s["b"] <= 1) and np.abs(s["b"].sum(axis=1) - 1).max() < 1e-15


def test_sphere_samples_lie_between_the_meshs_own_radii(sphere_samples):
    lo, hi = SF.sphere_radii()
    assert 0.9 * MC.SPHERE_RADIUS < lo < hi < 1.1 * MC.SPHERE_RADIUS
    d = np.linalg.norm(sphere_samples["points"].astype(np.float64) - MC.SPHERE_CENTRE, axis=1)
    slack = 8 * np.spacing(np.float32(8.0))                   # the float32 rounding of a sample's three coordinates
    assert lo - slack <= d.min() and d.max() <= hi + slack
    v, t, col = SF.sphere()
    n = sphere_samples["normals"].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    out = (sphere_samples["points"].astype(np.float64) - MC.SPHERE_CENTRE) / d[:, None]
    assert (n * out).sum(axis=1).min() > 0.8                  # the mesh's normals point outwards
    c = sphere_samples["colors"]
    assert c.min() >= 0 and c.max() <= 1 and np.abs(c - np.clip((sphere_samples["points"] - MC.SPHERE_CENTRE) / (2 * MC.SPHERE_RADIUS) + 0.5, 0, 1)).max() < 1e-5


def test_degenerate_and_kept_samples():
    v, t = SF.flat_mesh()
    s = SF.sample(v, t, 7, normals=True)
    assert s["total"] == 0 and (s["tri"] == -1).all() and np.isnan(s["points"]).all() and np.isnan(s["normals"]).all()
    assert SF.sample(v, t, 0)["points"].shape == (0, 3)
    v, t, _ = SF.sphere()
    keep = np.arange(len(t)) % 3 == 0
    s = SF.sample(v, t, 4096, seed=7, keep=keep)
    assert keep[s["tri"]].all() and len(np.unique(s["tri"])) > 600


def test_eval_mesh_arithmetic_on_restated_samples():
    """A mesh against itself with the same seed scores 0 exactly.  Against itself shifted by a dyadic d along x every sample has a partner
    at exactly |d|, so accuracy and completion are at most |d|: the mesh is moved to x in [16, 32), where every float32 is a multiple of
    2^-19 and adding 2^-5 is exact."""
    v, t, _ = SF.sphere()
    v = v + np.array([20.0, 0.0, 0.0], dtype=np.float32)
    S = SF.sample(v, t, 2000, seed=0)["points"]
    same = SF.eval_points(S, S)
    assert same["accuracy"] == 0.0 and same["completion"] == 0.0 and same["chamfer"] == 0.0
    assert same["precision"] == same["completion_ratio"] == same["fscore"] == 1.0 and same["n_precise"] == same["n_complete"] == 2000
    for d in (2.0 ** -5, 2.0 ** -3):
        E = S + np.array([d, 0.0, 0.0], dtype=np.float32)
        assert S[:, 0].min() >= 16 and E[:, 0].max() < 32 and np.all(E[:, 0].astype(np.float64) - S[:, 0].astype(np.float64) == d)
        r = SF.eval_points(E, S, threshold=0.05, max_error=0.5)
        assert 0 < r["accuracy"] <= d and 0 < r["completion"] <= d and r["chamfer"] == (r["accuracy"] + r["completion"]) / 2
        if d <= 0.05:
            assert r["n_precise"] == r["n_complete"] == 2000 and r["fscore"] == 1.0
        else:
            assert r["n_precise"] < 2000 and 0 < r["fscore"] < 1
    far = SF.eval_points(S + np.float32(4.0), S, threshold=0.05, max_error=0.5)
    assert far["accuracy"] <= 0.5 and far["n_precise"] < 2000
