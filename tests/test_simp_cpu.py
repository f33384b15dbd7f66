"""Host only: the numpy restatement of include/sta_simp.h (tests/simp_cases.py) against a second, naive statement - Python dicts and sets
for cells, collapse and duplicates, numpy.linalg.eigh for the eigen-decomposition, numpy.linalg.lstsq on the crease and the corner -, the
properties the header promises, and the plan and its refusals against the library's own messages."""
import ctypes as C
import math

import numpy as np
import pytest

import simp_cases as SP

f64 = np.float64


# ------------------------------------------------------------------------------------------ the naive statement
def naive_integers(v, t, cell, origin):
    o = [0.0, 0.0, 0.0] if origin is None else [float(x) for x in origin]
    nv = len(v)
    where = {}
    dropped = 0
    for i, p in enumerate(v.astype(f64).tolist()):
        if not all(math.isfinite(x) for x in p):
            dropped += 1
            continue
        idx = tuple(math.floor((p[k] - o[k]) / cell) for k in range(3))
        if not all(-SP.BIAS <= x < SP.BIAS for x in idx):
            dropped += 1
            continue
        where[i] = idx
    ranked = sorted(set(where.values()), key=lambda c: (c[2], c[1], c[0]))
    rank = {c: r for r, c in enumerate(ranked)}
    vcell = np.array([rank[where[i]] if i in where else -1 for i in range(nv)], np.int32).reshape(nv)
    seen, out, src = set(), [], []
    invalid = collapsed = duplicates = 0
    for ti, tri in enumerate(t.tolist()):
        if not all(0 <= i < nv and i in where for i in tri):
            invalid += 1
            continue
        c = [int(vcell[i]) for i in tri]
        if len(set(c)) < 3:
            collapsed += 1
            continue
        if frozenset(c) in seen:
            duplicates += 1
            continue
        seen.add(frozenset(c))
        k = c.index(min(c))
        out.append((c[k], c[(k + 1) % 3], c[(k + 2) % 3]))
        src.append(ti)
    used = sorted({c for tri in out for c in tri})
    new = {c: i for i, c in enumerate(used)}
    return {"vcell": vcell, "ranked": ranked, "tris": np.array([[new[c] for c in tri] for tri in out], np.int32).reshape(-1, 3), "src": np.array(src, np.int32),
            "used": used, "vmap": np.array([new.get(int(c), -1) if c >= 0 else -1 for c in vcell], np.int32).reshape(nv),
            "counters": (len(ranked), len(used), len(out), dropped, invalid, collapsed, duplicates)}


def naive_positions(v, t, cell, origin, nav, sv_ratio=1e-3):
    """per used cell: (mean, position by numpy.linalg.eigh with the header's threshold and acceptance rules, fell back, the cell's pairs)"""
    o = np.zeros(3) if origin is None else np.asarray(origin, f64)
    p = v.astype(f64)
    vcell = nav["vcell"]
    valid = np.array([all(0 <= i < len(v) and vcell[i] >= 0 for i in tri) for tri in t.tolist()], bool).reshape(len(t))
    rows = []
    for c in nav["used"]:
        m = p[vcell == c].mean(axis=0)
        tl = [t[ti] for ti in np.nonzero(valid)[0] for j in range(3) if vcell[t[ti, j]] == c]
        Q, g = np.zeros((3, 3)), np.zeros(3)
        for ia, ib, ic in tl:
            n = np.cross(p[ib] - p[ia], p[ic] - p[ia])
            if np.isfinite(n).all():
                Q += np.outer(n, n)
                g += n * (n @ (m - p[ia]))
        l, E = np.linalg.eigh(Q)
        lmax = l.max()
        y = sum((E[:, i] * ((E[:, i] @ g) / l[i]) for i in range(3) if l[i] > sv_ratio * lmax), np.zeros(3))
        x = m - y
        idx = np.array(nav["ranked"][c], f64)
        ok = lmax > 0 and np.isfinite(x).all() and (o + idx * cell <= x).all() and (x <= o + (idx + 1) * cell).all()
        rows.append((m, x if ok else m, not ok, tl))
    return rows


# ------------------------------------------------------------------------------------------ restatement against the naive statement
@pytest.mark.parametrize("name", list(SP.CASES))
def test_the_integer_stages_equal_the_naive_statement(name):
    v, _col, t, cell, origin = SP.CASES[name]()
    want = naive_integers(v, t, cell, origin)
    got = SP.expected(name, SP.PLACE_MEAN)
    n_v, n_t = want["counters"][1], want["counters"][2]
    assert got["counters"][:7] == want["counters"]
    assert np.array_equal(got["vcell"], want["vcell"]) and np.array_equal(got["vmap"], want["vmap"])
    assert np.array_equal(got["tris_out"][:n_t], want["tris"]) and np.array_equal(got["tri_src"][:n_t], want["src"])
    assert (got["tris_out"][n_t:] == -1).all() and (got["tri_src"][n_t:] == -1).all()
    cell_out = np.full(len(v), -1, np.int32)
    cell_out[want["used"]] = np.arange(n_v)
    assert np.array_equal(got["cell_out"], cell_out)


def test_the_cases_hold_what_they_promise():
    for name in SP.CASES:
        v, col, t, _cell, _origin = SP.CASES[name]()
        assert v.dtype == np.float32 and t.dtype == np.int32 and col.shape == v.shape, name
    v, _col, t, cell, _o = SP.hostile()
    assert len(t) == 4101 and len(v) == 1501 and len(t) % 64 and len(t) % 256 and len(t) > 4 * 1024
    c = dict(zip(SP.COUNTERS, SP.expected("hostile")["counters"]))
    assert all(c[k] > 0 for k in SP.COUNTERS), c
    assert not np.isfinite(v).all() and (t < 0).any() and (t >= len(v)).any()
    kept, idx = SP.cell_indices(v, cell)
    assert (idx < 0).any() and kept[10] and not kept[9] and not kept[11] and not kept[8]
    assert ((v[kept].astype(f64) / cell) % 1 == 0).any(), "a vertex exactly on a cell face"
    vc = SP.expected("hostile")["vcell"]
    assert 15 not in t and vc[15] == vc[20] and SP.expected("hostile")["vmap"][15] >= 0, "an unused vertex in a used cell"
    assert dict(zip(SP.COUNTERS, SP.expected("one_cell")["counters"]))["cells"] == 1 and SP.expected("one_cell")["counters"][1:3] == (0, 0)
    assert SP.expected("empty")["counters"] == (0,) * 8
    assert len(SP.crease()[2]) == 3200 and len(SP.sphere()[2]) == 2124


@pytest.mark.parametrize("name", SP.PLACE_CASES)
def test_the_jacobi_placement_against_eigh(name):
    v, _col, t, cell, origin = SP.CASES[name]()
    nav = naive_integers(v, t, cell, origin)
    rows = naive_positions(v, t, cell, origin, nav)
    got = SP.expected(name, SP.PLACE_QUADRIC)
    mean = SP.expected(name, SP.PLACE_MEAN)
    fell = np.array([r[2] for r in rows], bool)
    # A vertex alone in its cell and exactly on a cell face (the dyadic coordinates of `hostile`) has the exact answer x = m ON the face:
    # whether the rounding of g (1e-13 against eigenvalues of 1e3) leaves x inside is decided differently by the two statements, and
    # either way the position is m to 1e-16.  So the flags are reported and the positions - after the fallback - are what is compared.
    differ = int((got["fell"] != fell).sum())
    assert differ == 0 or name == "hostile", differ
    diff = max((np.abs(got["x64"][i] - r[1]).max() for i, r in enumerate(rows)), default=0.0)
    diff_mean = max((np.abs(mean["x64"][i] - r[0]).max() for i, r in enumerate(rows)), default=0.0)
    print(f"[simp] {name}: {len(rows)} cells, {int(fell.sum())} fallbacks ({differ} decided differently), Jacobi against eigh {diff:.3e} (bound {SP.JACOBI_VS_EIGH_BOUND:.3e}), "
          f"sequential mean against numpy's {diff_mean:.3e}")
    assert diff <= SP.JACOBI_VS_EIGH_BOUND and diff_mean <= SP.JACOBI_VS_EIGH_BOUND
    assert np.array_equal(mean["x64"], got["mean64"]) and mean["fallbacks"] == 0


def test_jacobi_diagonalises():
    r = np.random.default_rng(3)
    for _ in range(200):
        n = r.standard_normal((r.integers(1, 6), 3)) * 10.0 ** r.integers(-3, 4)
        Q = n.T @ n
        l, V = SP.jacobi(Q[0, 0], Q[0, 1], Q[0, 2], Q[1, 1], Q[1, 2], Q[2, 2])
        V = np.array(V)
        scale = np.abs(Q).max()
        assert np.abs(V.T @ V - np.eye(3)).max() < 1e-14
        assert np.abs(V @ np.diag(l) @ V.T - Q).max() <= 1e-14 * scale
        assert np.abs(np.sort(l) - np.linalg.eigvalsh(Q)).max() <= 1e-14 * scale
    assert SP.jacobi(2.0, 0.0, 0.0, 3.0, 0.0, 1.0) == ([2.0, 3.0, 1.0], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])      # nothing to rotate
    l, _V = SP.jacobi(1.0, 1e-300, 0.0, 1e300, 0.0, 0.0)          # theta * theta overflows: t = 0, the matrix stays
    assert l == [1.0, 1e300, 0.0]


# ------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("name", list(SP.CASES))
def test_properties(name):
    v, _col, t, cell, origin = SP.CASES[name]()
    for placement in (SP.PLACE_MEAN, SP.PLACE_QUADRIC):
        e = SP.expected(name, placement)
        c = dict(zip(SP.COUNTERS, e["counters"]))
        tri, src = e["tris_out"][:c["triangles"]], e["tri_src"][:c["triangles"]]
        assert ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])).all()
        assert len({frozenset(r) for r in tri.tolist()}) == len(tri)
        assert (tri[:, 0] < tri[:, 1]).all() and (tri[:, 0] < tri[:, 2]).all() and tri.min(initial=0) >= 0 and tri.max(initial=-1) < c["vertices"]
        assert (np.diff(src) > 0).all()
        assert len(t) == c["triangles"] + c["invalid_triangles"] + c["collapsed"] + c["duplicates"]
        assert c["vertices"] <= c["cells"] <= len(v) - c["dropped_vertices"]
        assert sorted(set(tri.reshape(-1).tolist())) == list(range(c["vertices"])), "every output vertex is named"
        # every output vertex inside its cell's closed cube, in float64, before the rounding
        kept, idx = SP.cell_indices(v, cell, origin)
        o = np.zeros(3) if origin is None else np.asarray(origin, f64)
        first = {int(e["vmap"][i]): i for i in range(len(v) - 1, -1, -1) if e["vmap"][i] >= 0}
        for row in range(c["vertices"]):
            i3 = idx[first[row]].astype(f64)
            assert (o + i3 * cell <= e["x64"][row]).all() and (e["x64"][row] <= o + (i3 + 1) * cell).all(), (name, placement, row)
        assert c["fallbacks"] == int(e["fell"].sum()) and (placement == SP.PLACE_QUADRIC or c["fallbacks"] == 0)


def test_identity_returns_the_input_mesh():
    v, col, t, _cell, _origin = SP.identity()
    e = SP.expected("identity", SP.PLACE_MEAN)
    vmap = e["vmap"]
    assert sorted(vmap.tolist()) == list(range(len(v))) and e["counters"] == (len(v), len(v), len(t), 0, 0, 0, 0, 0)
    assert np.array_equal(e["verts"][vmap], v) and np.array_equal(e["colors"][vmap], col)
    assert np.array_equal(e["tri_src"], np.arange(len(t)))
    mapped = vmap[t]
    k = mapped.argmin(axis=1)
    assert np.array_equal(e["tris_out"], np.stack([mapped[np.arange(len(t)), (k + j) % 3] for j in range(3)], axis=1))


@pytest.mark.parametrize("name", ("hostile", "sphere_2"))
def test_permuting_the_triangles(name):
    """New triangle k = old triangle perm[k].  Cells, vcell, cell_out, vmap, every counter, and the positions and colours of the mean
    placement do not change.  The output triangles are the same SET of unordered cluster triples; the one exception is which member of a
    set of duplicates represents it: the member with the lowest NEW index, in its own winding and rotation, at its place in the ascending
    order of the new indices.  (The quadric sums run in the new order, so quadric positions may move by rounding: not compared here.)"""
    v, col, t, cell, origin = SP.CASES[name]()
    perm = np.random.default_rng(1).permutation(len(t))
    a = SP.expected(name, SP.PLACE_MEAN)
    b = SP.simplify(v, col, t[perm], cell, origin, SP.PLACE_MEAN)
    for k in ("vcell", "cell_out", "vmap", "verts", "colors"):
        assert np.array_equal(a[k], b[k]), k
    assert a["counters"] == b["counters"]
    n = a["counters"][2]
    sets = lambda tri: sorted(tuple(sorted(r)) for r in tri.tolist())
    assert sets(a["tris_out"][:n]) == sets(b["tris_out"][:n])
    valid, collapsed, c = SP.triples(t, len(v), a["vcell"])
    new_index = np.argsort(perm)                                   # old triangle -> new index
    lowest = {}
    for old in np.nonzero(valid & ~collapsed)[0]:
        key = frozenset(c[old].tolist())
        lowest[key] = min(lowest.get(key, len(t)), int(new_index[old]))
    assert sorted(lowest.values()) == b["tri_src"][:n].tolist()
    for j in range(n):
        old = perm[b["tri_src"][j]]
        cc = a["cell_out"][c[old]]
        k = int(cc.argmin())
        assert b["tris_out"][j].tolist() == [cc[k], cc[(k + 1) % 3], cc[(k + 2) % 3]]


# ------------------------------------------------------------------------------------------ the crease and the corner
def _lstsq_point(p, tl, m):
    """the point nearest to m on the planes of the cell's triangles: min-norm least squares of n . (x - m) = n . (A - m), unit normals"""
    N, b = [], []
    for ia, ib, ic in tl:
        n = np.cross(p[ib] - p[ia], p[ic] - p[ia])
        n = n / np.linalg.norm(n)
        N.append(n)
        b.append(n @ (p[ia] - m))
    return m + np.linalg.lstsq(np.array(N), np.array(b), rcond=1e-9)[0]


def test_the_quadric_puts_the_vertex_on_the_crease_and_the_mean_does_not():
    v, _col, t, cell, origin = SP.crease()
    nav = naive_integers(v, t, cell, origin)
    rows = naive_positions(v, t, cell, origin, nav)
    quad, mean = SP.expected("crease", SP.PLACE_QUADRIC), SP.expected("crease", SP.PLACE_MEAN)
    assert quad["fallbacks"] == 0
    planes = SP.crease_planes()
    straddling = [i for i, c in enumerate(nav["used"]) if nav["ranked"][c][0] == math.floor(SP.CREASE_RIDGE / cell)]
    assert len(straddling) == 11, len(straddling)         # the rows y = 0 .. 10 in cells of 1
    worst_plane = worst_lstsq = 0.0
    least_mean = math.inf
    p = v.astype(f64)
    for i in straddling:
        x, m = quad["x64"][i], mean["x64"][i]
        off = [abs(n @ x - d) / np.linalg.norm(n) for n, d in planes]
        worst_plane = max(worst_plane, max(off))
        worst_lstsq = max(worst_lstsq, np.abs(x - _lstsq_point(p, rows[i][3], rows[i][0])).max())
        least_mean = min(least_mean, max(abs(n @ m - d) / np.linalg.norm(n) for n, d in planes))
        assert abs(x[0] - SP.CREASE_RIDGE) <= SP.LSTSQ_BOUND and abs(x[2] - SP.CREASE_Z0) <= SP.LSTSQ_BOUND
        assert abs(x[1] - m[1]) <= SP.LSTSQ_BOUND, "along the crease the vertex stays at the mean"
    print(f"[simp] crease: {len(straddling)} straddling cells, quadric off the planes by {worst_plane:.3e}, off the lstsq point by {worst_lstsq:.3e} "
          f"(bound {SP.LSTSQ_BOUND:.3e}); the mean is off a plane by at least {least_mean:.4f} (derived bound {SP.CREASE_MEAN_OFF:.4f}, cell {cell})")
    assert worst_plane <= SP.LSTSQ_BOUND and worst_lstsq <= SP.LSTSQ_BOUND
    assert least_mean > SP.CREASE_MEAN_OFF > 0.1 * cell
    # away from the crease every triangle of a cell lies in one plane: the vertex stays on it
    for i, c in enumerate(nav["used"]):
        if i not in straddling:
            side = planes[0] if nav["ranked"][c][0] < math.floor(SP.CREASE_RIDGE / cell) else planes[1]
            assert abs(side[0] @ quad["x64"][i] - side[1]) <= SP.LSTSQ_BOUND


def test_the_quadric_puts_the_vertex_on_the_corner():
    v, _col, t, cell, origin = SP.corner()
    nav = naive_integers(v, t, cell, origin)
    rows = naive_positions(v, t, cell, origin, nav)
    quad = SP.expected("corner", SP.PLACE_QUADRIC)
    i = nav["used"].index(nav["ranked"].index((2, 2, 2)))
    x = quad["x64"][i]
    off = np.abs(x - np.array(SP.CORNER)).max()
    off_lstsq = np.abs(x - _lstsq_point(v.astype(f64), rows[i][3], rows[i][0])).max()
    off_mean = np.abs(SP.expected("corner", SP.PLACE_MEAN)["x64"][i] - np.array(SP.CORNER)).max()
    print(f"[simp] corner: quadric off the corner by {off:.3e}, off the lstsq point by {off_lstsq:.3e} (bound {SP.LSTSQ_BOUND:.3e}); the mean by {off_mean:.4f}")
    assert off <= SP.LSTSQ_BOUND and off_lstsq <= SP.LSTSQ_BOUND and off_mean > 0.1 and not quad["fell"][i]


# ------------------------------------------------------------------------------------------ the plan and the refusals
PLANS = ((0, 0), (1, 3), (2124, 1064), (1023, 7), (1024, 256), (1025, 257), (10 ** 6, 2 * 10 ** 6), ((2 ** 31 - 1) // 3, 2 ** 31 - 1))
BAD_PLANS = ((-1, 3), (2 ** 31 // 3 + 1, 3), (2 ** 31, 3), (3, -1), (3, 2 ** 31))


def test_the_plan_is_the_restatements():
    from vista_slam_amd import _lib, build, simplify
    build.build_lib()
    lib = _lib.load_simp()
    out = (C.c_int64 * 3)()
    for nt, nv in PLANS:
        assert lib.sta_simp_plan(nt, nv, out) == 0 and tuple(out) == SP.plan(nt, nv) == tuple(simplify.plan(nt, nv)), (nt, nv)
    for nt, nv in BAD_PLANS:
        assert lib.sta_simp_plan(nt, nv, out) == -1
        with pytest.raises(ValueError) as e:
            SP.plan(nt, nv)
        assert str(e.value) == lib.sta_simp_last_error().decode()
        with pytest.raises(ValueError) as e2:
            simplify.plan(nt, nv)
        assert str(e2.value) == str(e.value)
    assert lib.sta_simp_plan(1, 1, None) == -1 and lib.sta_simp_last_error() == b"simp_plan: null argument"
