"""The contract of the keyframe gate (sta_flow_pyramid / sta_flow_corners / sta_flow_track, include/sta_mi355.h) restated in numpy,
a deliberately naive second statement of the same contract in per-pixel Python loops, and the frame builders of tests/test_flow_*.py.
Nothing here touches the GPU or the library.

The restatement follows OpenCV's documented algorithms (pyrDown, goodFeaturesToTrack with the minimal-eigenvalue response,
calcOpticalFlowPyrLK) in integer and float64 terms; it is NOT cv2, which was not available to compare against, so this file is the
yardstick.  Every float64 operation is one Python float operation in the order written (no fused multiply-add)."""
import math

import numpy as np

F32 = np.float32
W_BITS = 14
FS = 2.0 ** -20
KERNEL5 = (1, 4, 6, 4, 1)
MAX_PIXELS = 1 << 21
MAX_FRAMES = 32

# Test 2 of tests/test_flow_cpu.py (the restatement really is Lucas-Kanade): medians of |tracked - true shift| measured with
# blob_frame(seed=7) below: 96x128 shift (1.25, -0.5) 0.0097 px (46 of 47 points tracked), shift (5.5, 3.25) 0.0096 px (45 of 47);
# 224x224 0.0092 px (198 of 198) and 0.0116 px (192 of 198).  The bound is 3x the worst of them (the factor covers another seed,
# not another algorithm); a median above 0.25 px would mean that the restatement is not Lucas-Kanade.
LK_MEDIAN_BOUND = 3 * 0.0116


# ------------------------------------------------------------------------------------------------------------ input and extension
def to_u8(gray):
    """uint8 [H, W] of a frame: uint8 as it is; float32 in [0, 1] as the reference converts it, uint8(trunc(float32(g) * 255.0f))."""
    g = np.asarray(gray)
    g = g.reshape(g.shape[-2:])
    if g.dtype == np.uint8:
        return np.ascontiguousarray(g)
    assert g.dtype == np.float32, g.dtype
    return np.ascontiguousarray((g * F32(255.0)).astype(np.int32).astype(np.uint8))


def reflect(i, n):
    """periodic reflect-101 of integer indices into [0, n)"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = 2 * (n - 1)
    i = np.mod(i, m)
    return np.where(i >= n, m - i, i)


def ext(img, ys, xs):
    """img at the extended rows ys x columns xs -> int64 [len(ys), len(xs)]"""
    H, W = img.shape
    return img[reflect(ys, H)[:, None], reflect(xs, W)[None, :]].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ pyramid
def pyr_down(img):
    H, W = img.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    P = ext(img, np.arange(-2, 2 * H2 + 1), np.arange(-2, 2 * W2 + 1))
    acc = np.zeros((H2, W2), np.int64)
    for a in range(5):
        for b in range(5):
            acc += KERNEL5[a] * KERNEL5[b] * P[a:a + 2 * H2:2, b:b + 2 * W2:2]
    return ((acc + 128) >> 8).astype(np.uint8)


def pyramid(gray, win=21, max_level=3):
    """[level 0 .. level L] uint8; a level is added while l < max_level and both of its dimensions exceed win"""
    levels = [to_u8(gray)]
    while len(levels) - 1 < max_level:
        H, W = levels[-1].shape
        if not ((H + 1) // 2 > win and (W + 1) // 2 > win):
            break
        levels.append(pyr_down(levels[-1]))
    return levels


def level_sizes(H, W, win=21, max_level=3):
    out = [(H, W)]
    while len(out) - 1 < max_level:
        h, w = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if not (h > win and w > win):
            break
        out.append((h, w))
    return out


# ------------------------------------------------------------------------------------------------------------ corners
def isqrt(v):
    v = np.asarray(v, np.int64)
    s = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    s = s - (s * s > v)
    s = s + ((s + 1) * (s + 1) <= v)
    return s


def response(img, block_size=7):
    """(R int64 [H, W]) the integer minimal-eigenvalue response: Sobel 3x3, block_size^2 box sums of the products, isqrt"""
    H, W = img.shape
    P = ext(img, np.arange(-1, H + 1), np.arange(-1, W + 1))
    gx = (P[:-2, 2:] - P[:-2, :-2]) + 2 * (P[1:-1, 2:] - P[1:-1, :-2]) + (P[2:, 2:] - P[2:, :-2])
    gy = (P[2:, :-2] - P[:-2, :-2]) + 2 * (P[2:, 1:-1] - P[:-2, 1:-1]) + (P[2:, 2:] - P[:-2, 2:])
    r = block_size // 2
    sums = []
    for m in (gx * gx, gx * gy, gy * gy):
        E = ext(m, np.arange(-r, H + r), np.arange(-r, W + r))
        s = np.zeros((H, W), np.int64)
        for dy in range(block_size):
            for dx in range(block_size):
                s += E[dy:dy + H, dx:dx + W]
        sums.append(s)
    a, b, c = sums
    return (a + c) - isqrt((a - c) * (a - c) + 4 * b * b)


def candidates(R, quality=0.01):
    """flat pixel indices of the candidates in rank order (R descending, the lower index first), and Rmax"""
    H, W = R.shape
    rmax = int(R.max())
    pad = np.full((H + 2, W + 2), np.iinfo(np.int64).min, np.int64)
    pad[1:-1, 1:-1] = R
    nb = np.max([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)
    ok = (R > 0) & (R.astype(np.float64) >= quality * float(rmax)) & (R == nb)
    idx = np.flatnonzero(ok.reshape(-1))
    order = np.lexsort((idx, -R.reshape(-1)[idx]))
    return idx[order], rmax


def good_features(gray, max_corners=1000, quality=0.01, min_distance=8, block_size=7, info=None):
    """-> [n, 2] float32 (x, y) in rank order.  info (a dict) receives n_candidates and the responses' distinct count."""
    img = to_u8(gray)
    H, W = img.shape
    R = response(img, block_size)
    cand, _ = candidates(R, quality)
    if info is not None:
        info["n_candidates"] = len(cand)
        info["n_distinct"] = len(np.unique(R.reshape(-1)[cand]))
    ax, ay = np.zeros(max_corners, np.int64), np.zeros(max_corners, np.int64)
    n = 0
    md2 = min_distance * min_distance
    for p in cand.tolist():
        y, x = divmod(p, W)
        if n and ((ax[:n] - x) ** 2 + (ay[:n] - y) ** 2 < md2).any():
            continue
        ax[n], ay[n] = x, y
        n += 1
        if n == max_corners:
            break
    return np.stack([ax[:n], ay[:n]], axis=1).astype(F32)


# ------------------------------------------------------------------------------------------------------------ tracking
def scharr(img):
    H, W = img.shape
    P = ext(img, np.arange(-1, H + 1), np.arange(-1, W + 1))
    ix = 3 * (P[:-2, 2:] - P[:-2, :-2]) + 10 * (P[1:-1, 2:] - P[1:-1, :-2]) + 3 * (P[2:, 2:] - P[2:, :-2])
    iy = 3 * (P[2:, :-2] - P[:-2, :-2]) + 10 * (P[2:, 1:-1] - P[:-2, 1:-1]) + 3 * (P[2:, 2:] - P[:-2, 2:])
    return ix, iy


def weights(a, b):
    w00 = int(np.rint((1.0 - a) * (1.0 - b) * 16384.0))
    w01 = int(np.rint(a * (1.0 - b) * 16384.0))
    w10 = int(np.rint((1.0 - a) * b * 16384.0))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _interp(P, w, shift):
    s = w[0] * P[:-1, :-1] + w[1] * P[:-1, 1:] + w[2] * P[1:, :-1] + w[3] * P[1:, 1:]
    return (s + (1 << (shift - 1))) >> shift


class _Level:
    """one pyramid level padded for the window reads: the image by its extension, the gradients by zeros"""

    def __init__(self, prev, nxt, win):
        self.H, self.W = prev.shape
        self.pad = pad = win + 2
        ys, xs = np.arange(-pad, self.H + pad), np.arange(-pad, self.W + pad)
        self.I, self.J = ext(prev, ys, xs), ext(nxt, ys, xs)
        ix, iy = scharr(prev)
        self.ix = np.zeros_like(self.I)
        self.iy = np.zeros_like(self.I)
        self.ix[pad:-pad, pad:-pad] = ix
        self.iy[pad:-pad, pad:-pad] = iy

    def patch(self, arr, x, y, win):
        p = self.pad
        return arr[y + p:y + p + win + 1, x + p:x + p + win + 1]


def track(prev, nxt, pts, win=21, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4):
    """prev, nxt: frames (or pyramids as lists); pts [n, 2] float32 -> (next_pts [n, 2] float32, status [n] uint8)"""
    pp = prev if isinstance(prev, list) else pyramid(prev, win, max_level)
    pn = nxt if isinstance(nxt, list) else pyramid(nxt, win, max_level)
    assert [a.shape for a in pp] == [a.shape for a in pn]
    pts = np.asarray(pts, F32).reshape(-1, 2)
    L = len(pp) - 1
    lv = [_Level(a, b, win) for a, b in zip(pp, pn)]
    half = float((win - 1) // 2)
    out = np.zeros((len(pts), 2), F32)
    status = np.ones(len(pts), np.uint8)
    for i in range(len(pts)):
        x, y = float(pts[i, 0]), float(pts[i, 1])
        qx = qy = 0.0
        for l in range(L, -1, -1):
            v = lv[l]
            sc = 2.0 ** -l
            px, py = x * sc - half, y * sc - half
            if l == L:
                qx, qy = x * sc, y * sc
            else:
                qx, qy = 2.0 * qx, 2.0 * qy
            fx, fy = math.floor(px), math.floor(py)
            if fx < -win or fx >= v.W or fy < -win or fy >= v.H:
                if l == 0:
                    status[i] = 0
                continue
            w = weights(px - fx, py - fy)
            I = _interp(v.patch(v.I, fx, fy, win), w, W_BITS - 5)
            Ix = _interp(v.patch(v.ix, fx, fy, win), w, W_BITS)
            Iy = _interp(v.patch(v.iy, fx, fy, win), w, W_BITS)
            A11, A12, A22 = FS * float((Ix * Ix).sum()), FS * float((Ix * Iy).sum()), FS * float((Iy * Iy).sum())
            D = A11 * A22 - A12 * A12
            e = (A11 + A22 - math.sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / float(2 * win * win)
            if e < min_eig or D < 2.0 ** -23:
                if l == 0:
                    status[i] = 0
                continue
            qx, qy = qx - half, qy - half
            pdx = pdy = 0.0
            for j in range(max_iter):
                gx, gy = math.floor(qx), math.floor(qy)
                if gx < -win or gx >= v.W or gy < -win or gy >= v.H:
                    if l == 0:
                        status[i] = 0
                    break
                J = _interp(v.patch(v.J, gx, gy, win), weights(qx - gx, qy - gy), W_BITS - 5)
                diff = J - I
                b1, b2 = FS * float((diff * Ix).sum()), FS * float((diff * Iy).sum())
                dx, dy = (A12 * b2 - A22 * b1) / D, (A12 * b1 - A11 * b2) / D
                qx, qy = qx + dx, qy + dy
                if dx * dx + dy * dy <= eps * eps:
                    break
                if j > 0 and abs(dx + pdx) < 0.01 and abs(dy + pdy) < 0.01:
                    qx, qy = qx - dx * 0.5, qy - dy * 0.5
                    break
                pdx, pdy = dx, dy
            qx, qy = qx + half, qy + half
        out[i, 0], out[i, 1] = qx, qy
    return out, status


def disparity(pts, nxt_pts, status):
    """(n_pts, n_good, sum of the float64 displacements of the tracked points)"""
    good = np.asarray(status) == 1
    d = np.asarray(nxt_pts, F32)[good].astype(np.float64) - np.asarray(pts, F32)[good].astype(np.float64)
    return len(pts), int(good.sum()), float(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).sum())


class RefTracker:
    """vista_slam/flow_tracker.py's FlowTracker on the restatement: the branches of compute_disparity, the mean in float64"""

    def __init__(self, min_disparity, **kw):
        self.min_disparity = float(min_disparity)
        self.kw = kw
        self.reset()

    def reset(self):
        self.kf = self.kf_pts = None
        self.log = []                        # per call: (decision, why, n_pts, n_good, sum)

    def initialize_keyframe(self, image):
        self.kf = pyramid(image)
        self.kf_pts = good_features(self.kf[0], **self.kw)

    def compute_disparity(self, image):
        if self.kf is None:
            self.initialize_keyframe(image)
            self.log.append((True, "first", 0, 0, 0.0))
            return True
        cur = pyramid(image)
        n = len(self.kf_pts)
        nxt, st = track(self.kf, cur, self.kf_pts)
        _, good, total = disparity(self.kf_pts, nxt, st)
        if n < 10 or good < 10:
            why, key = "reinit", True
        else:
            key = total / good > self.min_disparity
            why = "moved" if key else "still"
        if key:
            self.kf = cur
            self.kf_pts = good_features(cur[0], **self.kw)
        self.log.append((key, why, n, good, total))
        return key


# ------------------------------------------------------------------------------------------------------------ the naive statement
def _reflect1(i, n):
    if n == 1:
        return 0
    m = 2 * (n - 1)
    i = ((i % m) + m) % m
    return m - i if i >= n else i


def _at(img, y, x):
    H, W = len(img), len(img[0])
    return int(img[_reflect1(y, H)][_reflect1(x, W)])


def naive_pyramid(gray, win=21, max_level=3):
    levels = [to_u8(gray).tolist()]
    while len(levels) - 1 < max_level:
        src = levels[-1]
        H, W = len(src), len(src[0])
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        if H2 <= win or W2 <= win:
            break
        dst = [[0] * W2 for _ in range(H2)]
        for y in range(H2):
            for x in range(W2):
                s = 0
                for a in range(5):
                    for b in range(5):
                        s += KERNEL5[a] * KERNEL5[b] * _at(src, 2 * y + a - 2, 2 * x + b - 2)
                dst[y][x] = (s + 128) >> 8
        levels.append(dst)
    return [np.array(lv, np.uint8) for lv in levels]


def naive_good_features(gray, max_corners=1000, quality=0.01, min_distance=8, block_size=7):
    img = to_u8(gray).tolist()
    H, W = len(img), len(img[0])
    gx = [[0] * W for _ in range(H)]
    gy = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            gx[y][x] = sum(k * (_at(img, y + d, x + 1) - _at(img, y + d, x - 1)) for d, k in ((-1, 1), (0, 2), (1, 1)))
            gy[y][x] = sum(k * (_at(img, y + 1, x + d) - _at(img, y - 1, x + d)) for d, k in ((-1, 1), (0, 2), (1, 1)))
    r = block_size // 2
    R = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            a = b = c = 0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yy, xx = _reflect1(y + dy, H), _reflect1(x + dx, W)
                    a += gx[yy][xx] * gx[yy][xx]
                    b += gx[yy][xx] * gy[yy][xx]
                    c += gy[yy][xx] * gy[yy][xx]
            R[y][x] = (a + c) - math.isqrt((a - c) * (a - c) + 4 * b * b)
    rmax = max(max(row) for row in R)
    cand = []
    for y in range(H):
        for x in range(W):
            v = R[y][x]
            if v <= 0 or float(v) < quality * float(rmax):
                continue
            if all(R[yy][xx] <= v for yy in range(max(0, y - 1), min(H, y + 2)) for xx in range(max(0, x - 1), min(W, x + 2))):
                cand.append((-v, y * W + x))
    cand.sort()
    taken = {}
    out = []
    reach = min_distance - 1
    for _, p in cand:
        y, x = divmod(p, W)
        clash = False
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                if dx * dx + dy * dy < min_distance * min_distance and (y + dy, x + dx) in taken:
                    clash = True
        if clash:
            continue
        taken[(y, x)] = len(out)
        out.append((x, y))
        if len(out) == max_corners:
            break
    return np.array(out, F32).reshape(-1, 2)


def _descale(s, k):
    return (s + (1 << (k - 1))) >> k


def naive_track(prev, nxt, pts, win=21, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4):
    pp = [a.tolist() for a in naive_pyramid(prev, win, max_level)]
    pn = [a.tolist() for a in naive_pyramid(nxt, win, max_level)]
    pts = np.asarray(pts, F32).reshape(-1, 2)
    L = len(pp) - 1
    half = float((win - 1) // 2)

    def grad(img, y, x):
        H, W = len(img), len(img[0])
        if not (0 <= y < H and 0 <= x < W):
            return 0, 0
        ix = sum(k * (_at(img, y + d, x + 1) - _at(img, y + d, x - 1)) for d, k in ((-1, 3), (0, 10), (1, 3)))
        iy = sum(k * (_at(img, y + 1, x + d) - _at(img, y - 1, x + d)) for d, k in ((-1, 3), (0, 10), (1, 3)))
        return ix, iy

    def bil(f, y, x, w, k):
        return _descale(w[0] * f(y, x) + w[1] * f(y, x + 1) + w[2] * f(y + 1, x) + w[3] * f(y + 1, x + 1), k)

    out = np.zeros((len(pts), 2), F32)
    status = np.ones(len(pts), np.uint8)
    for i in range(len(pts)):
        x, y = float(pts[i, 0]), float(pts[i, 1])
        qx = qy = 0.0
        for l in range(L, -1, -1):
            A, B = pp[l], pn[l]
            H, W = len(A), len(A[0])
            sc = 1.0 / (1 << l)
            px, py = x * sc - half, y * sc - half
            qx, qy = (x * sc, y * sc) if l == L else (2.0 * qx, 2.0 * qy)
            fx, fy = math.floor(px), math.floor(py)
            if fx < -win or fx >= W or fy < -win or fy >= H:
                status[i] = 0 if l == 0 else status[i]
                continue
            w = weights(px - fx, py - fy)
            T = []
            s11 = s12 = s22 = 0
            for wy in range(win):
                for wx in range(win):
                    yy, xx = fy + wy, fx + wx
                    iv = bil(lambda a, b: _at(A, a, b), yy, xx, w, W_BITS - 5)
                    ixv = bil(lambda a, b: grad(A, a, b)[0], yy, xx, w, W_BITS)
                    iyv = bil(lambda a, b: grad(A, a, b)[1], yy, xx, w, W_BITS)
                    T.append((iv, ixv, iyv))
                    s11 += ixv * ixv
                    s12 += ixv * iyv
                    s22 += iyv * iyv
            A11, A12, A22 = FS * float(s11), FS * float(s12), FS * float(s22)
            D = A11 * A22 - A12 * A12
            e = (A11 + A22 - math.sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / float(2 * win * win)
            if e < min_eig or D < 2.0 ** -23:
                status[i] = 0 if l == 0 else status[i]
                continue
            qx, qy = qx - half, qy - half
            pdx = pdy = 0.0
            for j in range(max_iter):
                gx, gy = math.floor(qx), math.floor(qy)
                if gx < -win or gx >= W or gy < -win or gy >= H:
                    status[i] = 0 if l == 0 else status[i]
                    break
                wq = weights(qx - gx, qy - gy)
                s1 = s2 = 0
                for wy in range(win):
                    for wx in range(win):
                        jv = bil(lambda a, b: _at(B, a, b), gy + wy, gx + wx, wq, W_BITS - 5)
                        iv, ixv, iyv = T[wy * win + wx]
                        s1 += (jv - iv) * ixv
                        s2 += (jv - iv) * iyv
                b1, b2 = FS * float(s1), FS * float(s2)
                dx, dy = (A12 * b2 - A22 * b1) / D, (A12 * b1 - A11 * b2) / D
                qx, qy = qx + dx, qy + dy
                if dx * dx + dy * dy <= eps * eps:
                    break
                if j > 0 and abs(dx + pdx) < 0.01 and abs(dy + pdy) < 0.01:
                    qx, qy = qx - dx * 0.5, qy - dy * 0.5
                    break
                pdx, pdy = dx, dy
            qx, qy = qx + half, qy + half
        out[i, 0], out[i, 1] = qx, qy
    return out, status


# ------------------------------------------------------------------------------------------------------------ frames
def blob_frame(H, W, shift=(0.0, 0.0), seed=7, n_blobs=None):
    """A procedural texture of Gaussian blobs sampled at (x - shift_x, y - shift_y) and quantised to uint8: the content of
    blob_frame(shift=s) is the content of blob_frame() moved by s.  Aperiodic, so a large shift has no alias to lock onto."""
    rng = np.random.RandomState(seed)
    n = n_blobs or max(24, H * W // 160)
    cx, cy = rng.uniform(-12, W + 12, n), rng.uniform(-12, H + 12, n)
    sg = rng.uniform(1.6, 4.5, n)
    amp = rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    xs, ys = xs - shift[0], ys - shift[1]
    v = np.zeros((H, W))
    for k in range(n):
        v += amp[k] * np.exp(-((xs - cx[k]) ** 2 + (ys - cy[k]) ** 2) / (2.0 * sg[k] ** 2))
    return np.clip(np.rint(127.5 + 70.0 * v), 0, 255).astype(np.uint8)


def noise_frame(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (H, W)).astype(np.uint8)


def checker_frame(H, W, square=4, lo=40, hi=210):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.where(((ys // square) + (xs // square)) % 2 == 0, lo, hi).astype(np.uint8)


def sequence(H=96, W=128, seed=11):
    """12 frames: a slow drift of 0.3 px per frame, then a jump of 9 px at frame 8, then drift again"""
    shifts, s = [], 0.0
    for t in range(12):
        s += 9.0 if t == 8 else 0.3
        shifts.append((s, 0.4 * s))
    return [blob_frame(H, W, sh, seed) for sh in shifts]
