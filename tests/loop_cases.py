"""The loop-candidate contract of include/sta_mi355.h (sta_orb_extract / sta_bow_transform / sta_bow_score) restated in numpy, a
naive second statement of it (per-pixel FAST by the definition, per-pixel Harris and moments, a looped tree walk, dict-based BoW), a
literal transcription of the reference's detect_loop, procedural frames and a procedural vocabulary writer.  Host only: numpy and
flow_cases (frame conversion, blobs, noise, checkerboard).  The trig table and the default comparison table are data of the contract;
`default_pattern` restates the generator of vista_slam_amd/loop.py, the trig table is handed in by the caller (the same array the
library gets).
"""
import numpy as np

import flow_cases as F

RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
TAPS = np.array([18, 33, 49, 56, 49, 33, 18], np.int64)


def trig_table():
    ang = np.deg2rad(np.arange(720, dtype=np.float64) * 0.5)
    return np.rint(np.stack([np.cos(ang), np.sin(ang)], 1) * float(1 << 30)).astype(np.int32)


def default_pattern(seed=12345):
    x = seed & 0x7FFFFFFF
    rows = []
    while len(rows) < 256:
        r = []
        for _ in range(4):
            x = (1103515245 * x + 12345) & 0x7FFFFFFF
            r.append(((x >> 16) % 27) - 13)
        if (r[0], r[1]) != (r[2], r[3]):
            rows.append(r)
    return np.array(rows, np.int8)


def umax_construction(half=15):
    """OpenCV's table for a patch of 31: rounded circle half-widths up to 45 degrees, mirrored beyond so the patch is symmetric."""
    umax = [0] * (half + 2)
    vmax = int(np.floor(half * np.sqrt(2.0) / 2 + 1))
    vmin = int(np.ceil(half * np.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        umax[v] = int(np.rint(np.sqrt(float(half * half - v * v))))
    v0 = 0
    for v in range(half, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return tuple(umax[:half + 1])


# ------------------------------------------------------------------------------------------------------------ sizes
def level_sizes(H, W, nlevels):
    s, out = np.float64(1.0), []
    for _ in range(nlevels):
        out.append((int(np.rint(np.float64(H) / s)), int(np.rint(np.float64(W) / s))))
        s = s * np.float64(1.2)
    return out


def level_features(nfeatures, nlevels):
    f = np.float64(1.0) / np.float64(1.2)
    fp = np.float64(1.0)
    for _ in range(nlevels):
        fp = fp * f
    nd = (np.float64(nfeatures) * (np.float64(1.0) - f)) / (np.float64(1.0) - fp)
    out = []
    for _ in range(nlevels - 1):
        out.append(int(np.rint(nd)))
        nd = nd * f
    out.append(max(nfeatures - sum(out), 0))
    return out


def built_levels(sizes, edge):
    n = 0
    for h, w in sizes:
        if h <= 2 * edge or w <= 2 * edge:
            break
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------ images
def _taps(n_dst, n_src):
    x = np.arange(n_dst, dtype=np.float64)
    r = np.float64(n_src) / np.float64(n_dst)
    f = (x + 0.5) * r - 0.5
    fl = np.floor(f)
    a = f - fl
    s = fl.astype(np.int64)
    lo, hi = s < 0, s >= n_src - 1
    s[lo], a[lo] = 0, 0.0
    s[hi], a[hi] = n_src - 1, 0.0
    c1 = np.rint(a * 2048.0).astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), 2048 - c1, c1


def resize(src, Hd, Wd):
    Hs, Ws = src.shape
    y0, y1, cy0, cy1 = _taps(Hd, Hs)
    x0, x1, cx0, cx1 = _taps(Wd, Ws)
    p = src.astype(np.int64)
    top = cx0[None] * p[y0][:, x0] + cx1[None] * p[y0][:, x1]
    bot = cx0[None] * p[y1][:, x0] + cx1[None] * p[y1][:, x1]
    return ((cy0[:, None] * top + cy1[:, None] * bot + (1 << 21)) >> 22).astype(np.uint8)


def levels(gray, nlevels, edge):
    img = F.to_u8(gray)
    sizes = level_sizes(*img.shape, nlevels)
    out = [img]
    for l in range(1, built_levels(sizes, edge)):
        out.append(resize(out[-1], *sizes[l]))
    return out


def blur(img):
    p = np.pad(img.astype(np.int64), 3, mode="reflect")              # numpy's "reflect" is reflect-101
    H, W = img.shape
    rows = sum(TAPS[b] * p[:, b:b + W] for b in range(7))
    s = sum(TAPS[a] * rows[a:a + H] for a in range(7))
    return ((s + (1 << 15)) >> 16).astype(np.uint8)


def fast_scores(img, thr):
    """score map [H, W]: 0 within 3 of the border and for a non-corner"""
    H, W = img.shape
    p = img.astype(np.int64)
    c = p[3:H - 3, 3:W - 3]
    d = np.stack([c - p[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for dx, dy in RING])
    A = np.full(c.shape, -256, np.int64)
    B = np.full(c.shape, -256, np.int64)
    for s0 in range(16):
        arc = d[[(s0 + j) & 15 for j in range(9)]]
        A = np.maximum(A, arc.min(0))
        B = np.maximum(B, (-arc).min(0))
    sc = np.maximum(A, B) - 1
    out = np.zeros((H, W), np.int64)
    out[3:H - 3, 3:W - 3] = np.where(sc >= thr, sc, 0)
    return out


def survivors(score, edge):
    """(ys, xs, scores) of the corners strictly above their 8 neighbours, inside the edge, in pixel order"""
    H, W = score.shape
    c = score[edge:H - edge, edge:W - edge]
    top = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                top &= score[edge + dy:H - edge + dy, edge + dx:W - edge + dx] < c
    ys, xs = np.nonzero(top)
    return ys + edge, xs + edge, c[top]


def first_cut(scores, n_l):
    """mask of the survivors that stay: all of them, or - above 2 n_l - those at or above the score of the 2 n_l-th largest"""
    if n_l == 0:
        return np.zeros(len(scores), bool)
    if len(scores) <= 2 * n_l:
        return np.ones(len(scores), bool)
    return scores >= np.sort(scores)[::-1][2 * n_l - 1]


def harris(img, ys, xs):
    p = img.astype(np.int64)
    H, W = p.shape
    ix = np.zeros((H, W), np.int64)
    iy = np.zeros((H, W), np.int64)
    ix[1:-1, 1:-1] = 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[:-2, 2:] - p[:-2, :-2]) + (p[2:, 2:] - p[2:, :-2])
    iy[1:-1, 1:-1] = 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, :-2] - p[:-2, :-2]) + (p[2:, 2:] - p[:-2, 2:])
    a = np.zeros(len(ys), np.int64)
    b = np.zeros(len(ys), np.int64)
    c = np.zeros(len(ys), np.int64)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            gx, gy = ix[ys + dy, xs + dx], iy[ys + dy, xs + dx]
            a += gx * gx
            b += gy * gy
            c += gx * gy
    return 25 * (a * b - c * c) - (a + b) * (a + b)


def angle_bin(m10, m01, trig):
    """the smallest k with cross(d_k, m) >= 0 > cross(d_(k+1), m); 0 for m = 0 or when no k qualifies.  -> (bin, number of such k)"""
    if m10 == 0 and m01 == 0:
        return 0, 0
    t = trig.astype(np.int64)
    k = np.arange(360)
    lo, hi = t[(2 * k - 1) % 720], t[2 * k + 1]
    ok = (lo[:, 0] * m01 - lo[:, 1] * m10 >= 0) & (hi[:, 0] * m01 - hi[:, 1] * m10 < 0)
    hits = np.flatnonzero(ok)
    return (int(hits[0]) if hits.size else 0), int(hits.size)


_MASK = np.array([[abs(u) <= UMAX[abs(v)] for u in range(-15, 16)] for v in range(-15, 16)])
_U = np.arange(-15, 16, dtype=np.int64)[None, :] * _MASK
_V = np.arange(-15, 16, dtype=np.int64)[:, None] * _MASK


def orientations(img, ys, xs, trig):
    p = img.astype(np.int64)
    out = np.zeros(len(ys), np.int64)
    for i, (y, x) in enumerate(zip(ys, xs)):
        patch = p[y - 15:y + 16, x - 15:x + 16]
        out[i] = angle_bin(int((_U * patch).sum()), int((_V * patch).sum()), trig)[0]
    return out


def rotate(pattern, bins, trig):
    """-> rx, ry int64 [n, 256, 2] (point 1, point 2)"""
    t = trig.astype(np.int64)[2 * bins]                               # [n, 2]
    C, S = t[:, 0][:, None, None], t[:, 1][:, None, None]
    pt = pattern.astype(np.int64).reshape(1, 256, 2, 2)
    x, y = pt[..., 0], pt[..., 1]
    return (x * C - y * S + (1 << 29)) >> 30, (x * S + y * C + (1 << 29)) >> 30


def descriptors(blurred, ys, xs, bins, pattern, trig):
    if len(ys) == 0:
        return np.zeros((0, 32), np.uint8)
    rx, ry = rotate(pattern, bins, trig)
    v = blurred[ys[:, None, None] + ry, xs[:, None, None] + rx].astype(np.int64)
    bits = (v[..., 0] < v[..., 1]).astype(np.uint8)                   # [n, 256]
    return np.packbits(bits, axis=1, bitorder="little")


def extract(gray, nfeatures=500, nlevels=8, fast_threshold=20, edge=31, pattern=None, trig=None, info=None):
    """-> kp int32 [n,4] (x, y, level, bin), resp int64 [n], desc uint8 [n,32]; info (a dict) receives the levels, the blurred levels and,
    per built level, (survivors, kept by the first cut, cut score or None, survivors exactly at the cut score)."""
    pattern = default_pattern() if pattern is None else pattern
    trig = trig_table() if trig is None else trig
    lv = levels(gray, nlevels, edge)
    nfeat = level_features(nfeatures, nlevels)
    kps, resps, descs, cuts, blurs = [], [], [], [], []
    for l, img in enumerate(lv):
        ys, xs, sc = survivors(fast_scores(img, fast_threshold), edge)
        keep = first_cut(sc, nfeat[l])
        cut = int(sc[keep].min()) if (nfeat[l] and len(sc) > 2 * nfeat[l]) else None
        cuts.append((len(sc), int(keep.sum()), cut, int((sc == cut).sum()) if cut is not None else 0))
        ys, xs = ys[keep], xs[keep]
        R = harris(img, ys, xs)
        order = np.lexsort((ys * img.shape[1] + xs, -R))[:nfeat[l]]
        ys, xs, R = ys[order], xs[order], R[order]
        bins = orientations(img, ys, xs, trig)
        b = blur(img)
        blurs.append(b)
        kps.append(np.stack([xs, ys, np.full(len(ys), l), bins], 1).astype(np.int32).reshape(-1, 4))
        resps.append(R.astype(np.int64))
        descs.append(descriptors(b, ys, xs, bins, pattern, trig))
    if info is not None:
        info.update(levels=lv, blurred=blurs, cuts=cuts, nfeat=nfeat)
    return np.concatenate(kps), np.concatenate(resps), np.concatenate(descs)


# ------------------------------------------------------------------------------------------------------------ the naive statement
def naive_extract(gray, nfeatures=500, nlevels=8, fast_threshold=20, edge=31, pattern=None, trig=None):
    """The same contract with Python loops and integers, pixel by pixel: slow, for small frames."""
    pattern = (default_pattern() if pattern is None else pattern).tolist()
    trig = (trig_table() if trig is None else trig).tolist()
    img0 = F.to_u8(gray).tolist()
    H0, W0 = len(img0), len(img0[0])
    sizes, s = [], 1.0
    for _ in range(nlevels):
        sizes.append((int(np.rint(H0 / s)), int(np.rint(W0 / s))))
        s = s * 1.2
    nfeat = level_features(nfeatures, nlevels)
    rows, img = [], img0
    for l, (H, W) in enumerate(sizes):
        if H <= 2 * edge or W <= 2 * edge:
            break
        if l > 0:
            prev, (Hp, Wp) = img, sizes[l - 1]

            def tap(x, nd, ns):
                f = (x + 0.5) * (float(ns) / float(nd)) - 0.5
                sx = int(np.floor(f))
                a = f - np.floor(f)
                if sx < 0:
                    sx, a = 0, 0.0
                elif sx >= ns - 1:
                    sx, a = ns - 1, 0.0
                c1 = int(np.rint(a * 2048.0))
                return sx, min(sx + 1, ns - 1), 2048 - c1, c1
            img = []
            for y in range(H):
                y0, y1, cy0, cy1 = tap(y, H, Hp)
                row = []
                for x in range(W):
                    x0, x1, cx0, cx1 = tap(x, W, Wp)
                    v = cy0 * cx0 * prev[y0][x0] + cy0 * cx1 * prev[y0][x1] + cy1 * cx0 * prev[y1][x0] + cy1 * cx1 * prev[y1][x1]
                    row.append((v + (1 << 21)) >> 22)
                img.append(row)
        memo = {}

        def score(y, x):
            if (y, x) not in memo:
                sc = 0
                if 3 <= x < W - 3 and 3 <= y < H - 3:
                    p = img[y][x]
                    ring = [img[y + dy][x + dx] for dx, dy in RING]
                    A = max(min(p - ring[(s0 + j) % 16] for j in range(9)) for s0 in range(16))
                    B = max(min(ring[(s0 + j) % 16] - p for j in range(9)) for s0 in range(16))
                    sc = max(A, B) - 1
                    sc = sc if sc >= fast_threshold else 0
                memo[(y, x)] = sc
            return memo[(y, x)]
        surv = []
        for y in range(edge, H - edge):
            for x in range(edge, W - edge):
                sc = score(y, x)
                if sc > 0 and all(score(y + dy, x + dx) < sc for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy):
                    surv.append((y, x, sc))
        n_l = nfeat[l]
        if n_l == 0:
            surv = []
        elif len(surv) > 2 * n_l:
            cut = sorted((sc for _, _, sc in surv), reverse=True)[2 * n_l - 1]
            surv = [t for t in surv if t[2] >= cut]
        cand = []
        for y, x, _ in surv:
            a = b = c = 0
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    yy, xx = y + dy, x + dx
                    gx = 2 * (img[yy][xx + 1] - img[yy][xx - 1]) + (img[yy - 1][xx + 1] - img[yy - 1][xx - 1]) + (img[yy + 1][xx + 1] - img[yy + 1][xx - 1])
                    gy = 2 * (img[yy + 1][xx] - img[yy - 1][xx]) + (img[yy + 1][xx - 1] - img[yy - 1][xx - 1]) + (img[yy + 1][xx + 1] - img[yy - 1][xx + 1])
                    a += gx * gx
                    b += gy * gy
                    c += gx * gy
            cand.append((-(25 * (a * b - c * c) - (a + b) ** 2), y * W + x))
        cand.sort()
        blurred = None
        for negR, pix in cand[:n_l]:
            y, x = divmod(pix, W)
            m10 = m01 = 0
            for v in range(-15, 16):
                for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1):
                    m10 += u * img[y + v][x + u]
                    m01 += v * img[y + v][x + u]
            b = 0
            if m10 or m01:
                for k in range(360):
                    d0, d1 = trig[(2 * k - 1) % 720], trig[2 * k + 1]
                    if d0[0] * m01 - d0[1] * m10 >= 0 and d1[0] * m01 - d1[1] * m10 < 0:
                        b = k
                        break
            if blurred is None:
                blurred = {}

            def B(yy, xx):
                if (yy, xx) not in blurred:
                    s_ = 0
                    for i in range(7):
                        for j in range(7):
                            s_ += int(TAPS[i]) * int(TAPS[j]) * img[int(F.reflect(yy + i - 3, H))][int(F.reflect(xx + j - 3, W))]
                    blurred[(yy, xx)] = (s_ + (1 << 15)) >> 16
                return blurred[(yy, xx)]
            C, S = trig[2 * b]
            d = [0] * 32
            for i, (x1, y1, x2, y2) in enumerate(pattern):
                ax, ay = (x1 * C - y1 * S + (1 << 29)) >> 30, (x1 * S + y1 * C + (1 << 29)) >> 30
                bx, by = (x2 * C - y2 * S + (1 << 29)) >> 30, (x2 * S + y2 * C + (1 << 29)) >> 30
                if B(y + ay, x + ax) < B(y + by, x + bx):
                    d[i // 8] |= 1 << (i % 8)
            rows.append(([x, y, l, b], -negR, d))
    return (np.array([r[0] for r in rows], np.int32).reshape(-1, 4), np.array([r[1] for r in rows], np.int64),
            np.array([r[2] for r in rows], np.uint8).reshape(-1, 32))


# ------------------------------------------------------------------------------------------------------------ bag of words
class Vocab:
    """the five arrays of the contract (numpy), as vista_slam_amd.loop.Vocabulary holds them"""

    def __init__(self, node_desc, child_first, child_count, word_of, word_weight):
        self.node_desc, self.child_first, self.child_count, self.word_of, self.word_weight = node_desc, child_first, child_count, word_of, word_weight


def transform(desc, V):
    """-> words int32 [m] ascending, counts int32 [m], vals float64 [m] (L1-normalised)"""
    n = len(desc)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    bits = np.unpackbits(np.asarray(desc, np.uint8), axis=1).astype(np.int16)
    nbits = np.unpackbits(V.node_desc, axis=1).astype(np.int16)
    node = np.zeros(n, np.int64)
    while True:
        active = np.flatnonzero(V.child_count[node] > 0)
        if active.size == 0:
            break
        for u in np.unique(node[active]):
            sel = active[node[active] == u]
            cf, cc = int(V.child_first[u]), int(V.child_count[u])
            d = (bits[sel][:, None, :] != nbits[cf:cf + cc][None]).sum(2)
            node[sel] = cf + d.argmin(1)                             # argmin: the first among equals
    w = V.word_of[node].astype(np.int64)
    keep = w >= 0
    keep[keep] = V.word_weight[w[keep]] > 0
    words, counts = np.unique(w[keep], return_counts=True)
    vals = counts.astype(np.float64) * V.word_weight[words]
    if len(vals):
        vals = vals / vals.sum()
    return words.astype(np.int32), counts.astype(np.int32), vals


def score(a, b):
    """a, b = (words, vals): DBoW's L1 score"""
    _, ia, ib = np.intersect1d(a[0], b[0], assume_unique=True, return_indices=True)
    va, vb = a[1][ia], b[1][ib]
    return float(-0.5 * np.sum(np.abs(va - vb) - np.abs(va) - np.abs(vb)))


def naive_transform(desc, V):
    """a looped walk on Python integers and a dict"""
    nd = [int.from_bytes(bytes(r.tolist()), "little") for r in V.node_desc]
    bag = {}
    for r in np.asarray(desc, np.uint8):
        q, node = int.from_bytes(bytes(r.tolist()), "little"), 0
        while V.child_count[node] > 0:
            best, best_d = None, None
            for c in range(int(V.child_first[node]), int(V.child_first[node]) + int(V.child_count[node])):
                dist = bin(q ^ nd[c]).count("1")
                if best is None or dist < best_d:
                    best, best_d = c, dist
            node = best
        w = int(V.word_of[node])
        if w >= 0 and V.word_weight[w] > 0:
            bag[w] = bag.get(w, 0) + 1
    words = sorted(bag)
    vals = [bag[w] * float(V.word_weight[w]) for w in words]
    norm = sum(vals)
    return words, [bag[w] for w in words], [v / norm for v in vals]


def naive_score(a, b):
    db = dict(zip(b[0], b[1]))
    s = 0.0
    for w, v in zip(a[0], a[1]):
        if w in db:
            s += abs(v - db[w]) - abs(v) - abs(db[w])
    return -0.5 * s


def make_vocab(k, L, seed=0, dup_siblings=False, unbalanced=False, zero_words=0.0):
    """A procedural tree as the text-format rows [(parent, is_leaf, bytes[32], weight)] in file order (node ids from 1).  dup_siblings:
    the first two children of every node share a descriptor (first-among-equals decides); unbalanced: every third inner node below
    the root is a leaf instead; zero_words: that fraction of the words gets weight 0 (1.0: all of them)."""
    rng = np.random.RandomState(seed)
    rows, frontier = [], [(0, 0)]                                     # (node id, depth)
    while frontier:
        node, depth = frontier.pop(0)
        for c in range(k):
            d = rng.randint(0, 256, 32)
            if dup_siblings and c == 1:
                d = rows[-1][2]
            leaf = depth + 1 == L or (unbalanced and depth >= 1 and (len(rows) % 3) == 0) or (unbalanced and depth == 0 and c == 0)
            rows.append([node, int(leaf), d, 0.0])
            if not leaf:
                frontier.append((len(rows), depth + 1))
    leaves = [r for r in rows if r[1]]
    for i, r in enumerate(leaves):
        r[3] = float(np.round(0.25 + 3.0 * rng.rand(), 6))
    if zero_words:
        for i in rng.permutation(len(leaves))[:max(1, int(round(zero_words * len(leaves))))]:
            leaves[i][3] = 0.0
    return rows


def write_vocab(path, rows, k, L, scoring=0, weighting=0):
    with open(path, "w") as f:
        f.write(f"{k} {L} {scoring} {weighting}\n")
        for parent, leaf, d, w in rows:
            f.write(f"{parent} {leaf} " + " ".join(str(int(b)) for b in d) + f" {w!r}\n")


def vocab_arrays(rows):
    """the text rows -> Vocab, by the loader's rule restated: breadth-first renumbering (siblings contiguous in file order behind their
    parent), word ids in leaf order of the file"""
    n = len(rows) + 1
    kids = [[] for _ in range(n)]
    for i, r in enumerate(rows):
        kids[r[0]].append(i + 1)
    order = [0]
    for node in order:
        order.extend(kids[node])
    new = {old: i for i, old in enumerate(order)}
    node_desc = np.zeros((n, 32), np.uint8)
    cf, cc, wo = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    weights = []
    for i, r in enumerate(rows, 1):
        node_desc[new[i]] = r[2]
        if r[1]:
            wo[new[i]] = len(weights)
            weights.append(r[3])
    for i in range(n):
        if kids[i]:
            cf[new[i]], cc[new[i]] = new[kids[i][0]], len(kids[i])
    return Vocab(node_desc, cf, cc, wo, np.array(weights, np.float64))


def random_desc(n, seed, V=None, near=0.5):
    """n descriptors: random bytes, or - with a vocabulary - about `near` of them a node's descriptor with a few bits flipped"""
    rng = np.random.RandomState(seed)
    d = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    if V is not None:
        for i in np.flatnonzero(rng.rand(n) < near):
            d[i] = V.node_desc[rng.randint(1, len(V.node_desc))]
            d[i, rng.randint(0, 32)] ^= np.uint8(1 << rng.randint(0, 8))
    return d


# ------------------------------------------------------------------------------------------------------------ detect_loop
def reference_detect_loop(bow_feats, score_fn, loop_dist_min, loop_nms, loop_cand_thresh_neighbor, farthest_neighbor):
    """vista_slam/loop_detector.py:25-50 transcribed: bow_feats ends with the new view's vector (or None)"""
    i = len(bow_feats) - 1
    loop_farthest_neighbor = max(0, i - loop_cand_thresh_neighbor)
    bow_feat_i = bow_feats[i]
    neighbor_sims = []
    for j in range(loop_farthest_neighbor, i):
        if bow_feat_i is None or bow_feats[j] is None:
            continue
        similarity = score_fn(bow_feat_i, bow_feats[j])
        neighbor_sims.append(similarity)
    sim_thresh = 1.0 if len(neighbor_sims) == 0 else min(neighbor_sims)
    last_egde = farthest_neighbor
    loop_candi_list = []
    for j in reversed(range(0, farthest_neighbor)):
        if last_egde - j > loop_nms and i - j > loop_dist_min:
            if bow_feat_i is None or bow_feats[j] is None:
                continue
            similarity = score_fn(bow_feat_i, bow_feats[j])
            if similarity > sim_thresh:
                loop_candi_list.append((j, similarity))
                last_egde = j
    loop_candi_list = sorted(loop_candi_list, key=lambda x: x[1], reverse=True)
    return loop_candi_list


# ------------------------------------------------------------------------------------------------------------ frames
def constant_frame(H, W, v=128):
    return np.full((H, W), v, np.uint8)


def dot_frame(H, W, pitch=8):
    """2x2 bright dots on a dark ground: the four pixels of a dot are corners of one score, so every comparison among them ties"""
    img = np.full((H, W), 40, np.uint8)
    for y in range(3, H - 4, pitch):
        for x in range(3, W - 4, pitch):
            img[y:y + 2, x:x + 2] = 220
    return img


def disc_frame(rows, cols, cell=32, margin=16):
    """rows x cols cells, each a disc around a bright centre pixel whose brightness ramps along its own direction (cell i: i * 360 /
    (rows cols) degrees) under a radial window - mirror-symmetric about that direction, so the four axis directions give m01 = 0 or
    m10 = 0 exactly; a margin keeps the outer centres inside the default edge of 31.  -> (frame, centres [(y, x)], directions in degrees)"""
    n = rows * cols
    img = np.full((rows * cell + 2 * margin, cols * cell + 2 * margin), 120, np.uint8)
    v, u = np.mgrid[-15:16, -15:16].astype(np.float64)
    win = np.clip(1.0 - (u * u + v * v) / 225.0, 0.0, None)
    centres, degs = [], []
    for i in range(n):
        deg = i * 360.0 / n
        c, s = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}.get(deg, (np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))))
        patch = np.rint(120.0 + 4.0 * (u * c + v * s) * win)
        cy, cx = margin + (i // cols) * cell + 16, margin + (i % cols) * cell + 16
        img[cy - 15:cy + 16, cx - 15:cx + 16] = patch.astype(np.uint8)
        img[cy, cx] = 255
        centres.append((cy, cx))
        degs.append(deg)
    return img, centres, degs


def loop_sequence(n=60, H=96, W=128, seed=3):
    """A camera that pans over a wide blob panorama and comes back to where it started, three rows lower and a pixel to the side: frame t
    and frame n - 1 - t see the same place, and no two frames are the same picture."""
    pano = F.blob_frame(H + 6, W * 4, seed=seed, n_blobs=240)
    half = n // 2
    out = []
    for t in range(n):
        step, y0, dx = (t, 0, 0) if t < half else (n - 1 - t, 3, 1)
        x0 = int(round(step * (W * 3 - 1) / (half - 1) * 0.9)) + dx
        out.append(np.ascontiguousarray(pano[y0:y0 + H, x0:x0 + W]))
    return out


def detect_loop_margins(present, sim, i, farthest_neighbor, loop_dist_min, loop_nms, loop_cand_thresh_neighbor):
    """What the numbers of one detect_loop call look like: (the smallest |similarity - sim_thresh| over the comparisons made, the
    number of views that passed the distance test and the threshold and were skipped by the NMS window alone)."""
    sims = [sim[j] for j in range(max(0, i - loop_cand_thresh_neighbor), i) if present[i] and present[j]]
    thresh = 1.0 if not sims else min(sims)
    margin, skips, last_edge = np.inf, 0, farthest_neighbor
    for j in reversed(range(0, farthest_neighbor)):
        if not (i - j > loop_dist_min) or not present[i] or not present[j]:
            continue
        if last_edge - j > loop_nms:
            margin = min(margin, abs(sim[j] - thresh))
            if sim[j] > thresh:
                last_edge = j
        elif sim[j] > thresh:
            skips += 1
    return margin, skips
