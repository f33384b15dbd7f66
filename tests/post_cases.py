"""Case tables and plain float64 references of the scalar kernels behind the transformer: the DPT tail's head_final_kernel, the pose
head's nearest_rotation, and the output step of the public ABI (sta_world_pointcloud, sta_estimate_intrinsics, sta_estimate_scale,
sta_mat_to_se3, sta_pack_compact).  Importable without a GPU (tests/test_row_post_cpu.py runs every condition stated here on the
CPU and pins each reference to the reference-generated fixtures); tests/test_post_gpu.py runs the kernels."""
import numpy as np

F32 = np.float32
ULP24 = 2.0 ** -24


def ulp_diff(a, b):
    """Distance of two float32 values in units in the last place (same sign assumed)."""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------ head_final_kernel
HEAD_NPIX = (1, 3, 4, 5, 63, 64, 65, 4099)


def head_final_inputs(npix, seed=23):
    """feat [npix,128] positive integers in {1, 2} (pixel 1: one entry 7), w4 [4,128] DENSE with entries in {-1, 0, 1}, bias [4].
    Every lane of the 16-lane butterfly holds non-zero weights of every output.  Every product and partial sum is an integer below
    2^11, so x, y, z, c are exact in any precision and any summation order; the three xyz biases are the integers that put pixel 0
    at xyz = 0 exactly, and pixel 1 (npix > 1) differs from pixel 0 in one feature by 6, which puts it at |xyz| = 6 sqrt(3) = 10.4."""
    rng = np.random.default_rng(seed)
    w4 = rng.integers(-1, 2, size=(4, 128)).astype(F32)
    j = 5
    w4[:3, j] = (1, -1, 1)
    f0 = rng.integers(1, 3, size=128).astype(F32)
    feat = rng.integers(1, 3, size=(npix, 128)).astype(F32)
    feat[0] = f0
    if npix > 1:
        feat[1] = f0
        feat[1, j] += 6
    bias = np.empty(4, F32)
    bias[:3] = -(w4[:3].astype(np.float64) @ f0.astype(np.float64))
    bias[3] = F32(rng.standard_normal() - float(w4[3].astype(np.float64) @ f0.astype(np.float64)))
    return feat, w4, bias


def head_final_pre64(feat, w4, bias):
    return feat.astype(np.float64) @ w4.astype(np.float64).T + bias.astype(np.float64)


def postprocess64(pre):
    """pre [..., 4] (x, y, z, c) -> pts = xyz / max(|xyz|, 1e-8) expm1(|xyz|), conf = 1 + exp(c)   (postprocess.py:10-62)."""
    pre = np.asarray(pre, np.float64)
    xyz = pre[..., :3]
    d = np.sqrt((xyz ** 2).sum(-1, keepdims=True))
    return xyz * (np.expm1(d) / np.maximum(d, 1e-8)), 1.0 + np.exp(pre[..., 3])


def pixel_rel(got, ref):
    """Per pixel |got - ref| / |ref| over the last axis ([npix,3] -> [npix]); 0 where both are exactly 0."""
    got = np.asarray(got, np.float64).reshape(len(got), -1); ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    num = np.sqrt(((got - ref) ** 2).sum(-1)); den = np.sqrt((ref ** 2).sum(-1))
    out = num / np.maximum(den, 1e-300)
    out[(num == 0) & (den == 0)] = 0.0
    return out


# ------------------------------------------------------------------------------------------ nearest_rotation
SVD_B = (1, 63, 64, 65, 257)
SVD_GAP = 0.1          # sigma2 + sign(det) sigma3 of the ROW-NORMALISED matrix, see svd_table


def rot_axis_angle(axis, ang):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def row_normalize64(m):
    """F.normalize(m, dim=-1) (pose_head.py:41) in float64 of the float32 values."""
    m = np.asarray(m, np.float64)
    return m / np.maximum(np.sqrt((m ** 2).sum(-1, keepdims=True)), 1e-12)


def svd_rotation64(m, s3=None):
    """svd_orthogonalize (pose_head.py:38-57) in float64: rows normalised, M = U S V^T, R = U diag(1, 1, det(U V^T)) V^T - the
    rotation nearest to M.  s3 = +-1 forces the third sign (the two candidates of an exactly singular input)."""
    M = row_normalize64(m)
    U, S, Vt = np.linalg.svd(M)
    d = np.linalg.det(U @ Vt) if s3 is None else s3
    return U @ np.diag([1.0, 1.0, np.sign(d)]) @ Vt


def svd_gap(m):
    """sigma2 + sign(det) sigma3 of the row-normalised matrix: the reciprocal condition number of its nearest rotation."""
    M = row_normalize64(m)
    S = np.linalg.svd(M, compute_uv=False)
    return float(S[1] + np.sign(np.linalg.det(M)) * S[2]), float(S[1])


def svd_table(seed=29):
    """257 float32 3x3 inputs and their kinds.  The first 16 entries are the special cases, the rest random.
      regular (compared with svd_rotation64 at 1e-5):
        "rot"     a scaled rotation (three equal singular values)
        "rep+" / "rep-"  Q1 diag(2, 2, +-1) Q2^T with the third column of Q1 = (1, 1, 1) / sqrt(3): its rows have equal norms, so the
                  row normalisation keeps the repeated pair of singular values
        "random"  Gaussian matrices, every second one with its first row negated until the determinants alternate in sign, kept when
                  sigma2 >= 1e-3 AND sigma2 + sign(det) sigma3 >= SVD_GAP.  The second clause is the conditioning of the comparison
                  itself: the kernel normalises the rows in fp32, the reference in fp64 - a relative row perturbation of <= 3 x 2^-24 =
                  1.8e-7 -, and the nearest rotation moves by at most that over the gap: 1.8e-7 / 0.1 = 1.8e-6, under a quarter of 1e-5.
      "rank2": exactly singular after the normalisation, sigma3 = 0 (two identical rows, a zero row, a zero column): the output must
               be one of svd_rotation64(m, +1), svd_rotation64(m, -1)
      "rank1" (identical / opposite rows, one non-zero row) and "zero": any rotation."""
    rng = np.random.default_rng(seed)
    mats, kinds = [], []

    def add(m, k):
        mats.append(np.asarray(m, np.float64).astype(F32)); kinds.append(k)

    q3 = np.full(3, 1 / np.sqrt(3))
    q1 = np.cross(q3, [1.0, 0.0, 0.0]); q1 /= np.linalg.norm(q1)
    Q1 = np.stack([q1, np.cross(q3, q1), q3], 1)
    add(1.7 * random_rotation(rng), "rot")
    add(Q1 @ np.diag([2.0, 2.0, 1.0]) @ random_rotation(rng).T, "rep+")
    add(Q1 @ np.diag([2.0, 2.0, -1.0]) @ random_rotation(rng).T, "rep-")
    a, b = rng.standard_normal(3), rng.standard_normal(3)
    add(np.stack([a, b, a]), "rank2")
    add(np.stack([a, np.zeros(3), b]), "rank2")
    m = rng.standard_normal((3, 3)); m[:, 1] = 0
    add(m, "rank2")
    add(np.stack([a, a, a]), "rank1")
    add(np.stack([a, -a, 2 * a]), "rank1")
    add(np.stack([np.zeros(3), b, np.zeros(3)]), "rank1")
    add(np.stack([[1.0, 0, 0]] * 3), "rank1")
    add(np.zeros((3, 3)), "zero")
    add(0.3 * random_rotation(rng), "rot")
    add(np.eye(3), "rot")
    add(Q1 @ np.diag([2.0, 2.0, -1.0]) @ random_rotation(rng).T * 0.2, "rep-")
    add(Q1 @ np.diag([2.0, 2.0, 1.0]) @ random_rotation(rng).T * 5, "rep+")
    add(np.stack([b, b, -b]), "rank1")
    assert len(mats) == 16
    want_neg = False
    while len(mats) < 257:
        m = (rng.standard_normal((3, 3)) * rng.choice([0.01, 1.0, 30.0])).astype(F32)
        if (np.linalg.det(m.astype(np.float64)) < 0) != want_neg:
            m[0] = -m[0]
        gap, s2 = svd_gap(m)
        if s2 >= 1e-3 and gap >= SVD_GAP:
            mats.append(m); kinds.append("random")
            want_neg = not want_neg
    return np.stack(mats), np.array(kinds)


def rotation_defects(r):
    """-> (max |R R^T - I|, max |det - 1|) per matrix."""
    r = np.asarray(r, np.float64)
    return np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max((1, 2)), np.abs(np.linalg.det(r) - 1.0)


# ------------------------------------------------------------------------------------------ mat_to_se3
SE3_B = (1, 63, 64, 65, 130)


def shepperd_branch(R, dtype):
    """The branch mat_to_se3_kernel takes, with the comparisons evaluated in `dtype`: 0 trace > 0, 1 m00 largest, 2 m11, 3 m22."""
    m = np.asarray(R, dtype)
    tr = dtype(dtype(m[0, 0] + m[1, 1]) + m[2, 2])
    if tr > 0:
        return 0
    if m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        return 1
    return 2 if m[1, 1] > m[2, 2] else 3


def shepperd64(pose):
    """pp.mat2SE3 by definition in float64 of the float32 entries: -> (se3 [B,7] = (t, qx, qy, qz, qw) with qw >= 0, the raw qw before
    the sign flip [B], branch [B])."""
    pose = np.asarray(pose, np.float64).reshape(-1, 4, 4)
    out = np.zeros((len(pose), 7)); raw = np.zeros(len(pose)); br = np.zeros(len(pose), np.int64)
    for i, P in enumerate(pose):
        m = P[:3, :3]
        b = shepperd_branch(m, np.float64)
        if b == 0:
            s = np.sqrt(np.trace(m) + 1.0) * 2; q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
        elif b == 1:
            s = np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2; q = [0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
        elif b == 2:
            s = np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2; q = [(m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
        else:
            s = np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2; q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s, (m[1, 0] - m[0, 1]) / s]
        q = np.array(q) / np.linalg.norm(q)
        raw[i] = q[3]; br[i] = b
        out[i, :3] = P[:3, 3]; out[i, 3:] = q * (-1.0 if q[3] < 0 else 1.0)
    return out, raw, br


def quat_to_rot(q):
    """(qx, qy, qz, qw) [B,4] -> rotation matrices [B,3,3] in float64."""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def se3_table(seed=31):
    """130 float32 poses [130,4,4].  Rotations: by pi and by pi - 1e-3 about x, y, z and (1, 1, 1) / sqrt(3) (both senses of the
    latter angle: the raw qw has both signs); the three cyclic permutation matrices and their squares (trace exactly 0); rotations about
    (1, 1, 0) / sqrt(2) by pi and 2.5 (m00 == m11 to the bit: the strict comparisons fall through to the m22 branch / the trace
    branch); the rest random.  Translations: random, with -0.0, a subnormal and 1e30 among them (copied bit for bit)."""
    rng = np.random.default_rng(seed)
    rots = []
    axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
    for ax in axes:
        rots.append(rot_axis_angle(ax, np.pi))
        rots.append(rot_axis_angle(ax, np.pi - 1e-3))
        rots.append(rot_axis_angle(ax, -(np.pi - 1e-3)))
    cyc = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)
    rots += [cyc, cyc @ cyc, cyc.T]
    rots += [rot_axis_angle((1, 1, 0), np.pi), rot_axis_angle((1, 1, 0), 2.5), rot_axis_angle((1, 1, 0), -3.0),
             rot_axis_angle((0, 1, 1), np.pi), rot_axis_angle((1, 0, 1), np.pi)]
    # the m00-largest / m11-largest / m22-largest branches with a raw qw of both signs: angle near pi about a tilted axis
    for ax in [(3, 1, 0.5), (1, 3, 0.5), (0.5, 1, 3)]:
        for ang in (3.0, -3.0, 2.9, -2.9):
            rots.append(rot_axis_angle(ax, ang))
    while len(rots) < 130:
        rots.append(random_rotation(rng))
    pose = np.zeros((130, 4, 4), F32)
    pose[:, :3, :3] = np.stack(rots).astype(F32)
    pose[:, 3, 3] = 1
    t = (rng.standard_normal((130, 3)) * 10).astype(F32)
    t[0, 0] = F32(-0.0); t[1, 1] = F32(1e-40); t[2, 2] = F32(1e30); t[3] = 0
    pose[:, :3, 3] = t
    return pose


# ------------------------------------------------------------------------------------------ sta_world_pointcloud
CLOUD_GEOMS = [(1, 5, 7), (3, 9, 29), (3, 300, 301), (2, 513, 512)]
CLOUD_PATTERNS = ("all", "none", "first", "last", "random", "at_thres", "nan")
CLOUD_THRES = 1.5


def cloud_blocks(geom):
    """(blocks of 256 pixels, count blocks per thread of the single-block scan)."""
    n = geom[0] * geom[1] * geom[2]
    nblk = (n + 255) // 256
    return nblk, (nblk + 1023) // 1024


def cloud_conf(geom, pattern, seed=37):
    """Confidences [N,H,W] float32 and the keep mask they must produce under conf > CLOUD_THRES."""
    N, H, W = geom
    rng = np.random.default_rng(seed + N * H * W + CLOUD_PATTERNS.index(pattern))
    total = N * H * W
    keep = np.zeros(total, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern in ("random", "at_thres", "nan"):
        keep = rng.random(total) < 0.5
    conf = np.where(keep, CLOUD_THRES + 0.25 + rng.random(total), CLOUD_THRES - 0.25 - rng.random(total)).astype(F32)
    if pattern == "at_thres":                  # every second dropped pixel sits exactly AT the threshold: strict >
        drop = np.nonzero(~keep)[0]
        conf[drop[::2]] = F32(CLOUD_THRES)
    if pattern == "nan":                       # every second dropped pixel is NaN: NaN > thres is false
        drop = np.nonzero(~keep)[0]
        conf[drop[::2]] = np.nan
    return conf.reshape(N, H, W), keep.reshape(N, H, W)


def cloud_inputs(geom, klass, seed=41):
    """depths [N,H,W], scales [N], K [N,3,3], poses [N,4,4], imgs [N,3,H,W] float32.
    klass "exact": focal lengths powers of two, integer principal points, no skew, depth x scale dyadic (depth = k / 16, k < 256;
    scale a power of two), poses signed permutations with integer translations: every intermediate of the formula has at most
    10 + 8 + 5 = 23 significant bits, so fp32 evaluates it exactly in any association.
    klass "general": upper-triangular K with skew, random rigid poses, depths in [0.5, 8), scales in [0.5, 2).
    Images: uniform in [-1.5, 1.5] (values outside [-1, 1] clip), and every value of `color_ties` somewhere."""
    N, H, W = geom
    rng = np.random.default_rng(seed + N * H * W + (klass == "exact"))
    K = np.zeros((N, 3, 3), F32); K[:, 2, 2] = 1
    poses = np.zeros((N, 4, 4), F32); poses[:, 3, 3] = 1
    if klass == "exact":
        depths = (rng.integers(1, 256, size=(N, H, W)) / 16.0).astype(F32)
        scales = np.array([0.5, 2.0, 1.0, 4.0][:N], F32)
        for n in range(N):
            K[n, 0, 0] = (256.0, 512.0, 128.0)[n % 3]; K[n, 1, 1] = (512.0, 256.0, 128.0)[n % 3]
            K[n, 0, 2] = W // 2 + n; K[n, 1, 2] = H // 2 - n
            perm = rng.permutation(3)
            poses[n, np.arange(3), perm] = rng.choice([-1.0, 1.0], 3)
            poses[n, :3, 3] = rng.integers(-16, 17, 3)
    else:
        depths = (0.5 + 7.5 * rng.random((N, H, W))).astype(F32)
        scales = (0.5 + 1.5 * rng.random(N)).astype(F32)
        for n in range(N):
            f = 0.8 * max(H, W) + 50
            K[n, 0, 0] = f * (1 + 0.1 * rng.random()); K[n, 1, 1] = f * (1 + 0.1 * rng.random())
            K[n, 0, 1] = 3.0 * rng.standard_normal()
            K[n, 0, 2] = W / 2 + rng.standard_normal(); K[n, 1, 2] = H / 2 + rng.standard_normal()
            poses[n, :3, :3] = random_rotation(rng)
            poses[n, :3, 3] = rng.standard_normal(3) * 5
    imgs = (rng.random((N, 3, H, W)) * 3 - 1.5).astype(F32)
    ties = color_ties()
    flat = imgs.reshape(-1)
    flat[:len(ties)] = ties[:flat.size]
    return depths, scales, K, poses, imgs


def color_of(img):
    """(img + 1) / 2 in float32, operation by operation as the kernel (and slam.py:404) evaluates it."""
    return ((np.asarray(img, F32) + F32(1.0)) / F32(2.0)).astype(F32)


def color_byte(c):
    """rint(clip(c, 0, 1) * 255): one fp32 product, round half to even."""
    return np.rint((np.clip(np.asarray(c, F32), F32(0), F32(1)) * F32(255.0)).astype(F32)).astype(np.uint8)


def color_ties():
    """Image values whose colour times 255 is EXACTLY k + 0.5 in fp32 (found by search, both parities of k), and the values that
    clip: below -1, above 1, the ends themselves."""
    out = []
    for k in range(255):
        for img in np.nextafter(F32(2 * (k + 0.5) / 255 - 1), F32([-4, 4])).tolist() + [2 * (k + 0.5) / 255 - 1]:
            p = (np.clip(color_of(F32(img)), F32(0), F32(1)) * F32(255.0)).astype(F32)
            if float(p) == k + 0.5:
                out.append(img)
                break
    return np.array(out[:48] + [-1.0, 1.0, -1.25, 1.5, -3.0], F32)          # (the smallest geometry has 105 image values)


def _abs_adjugate_inverse(K):
    """|K^-1| term magnitudes [N,3,3]: the adjugate formula of the kernel with every product taken in absolute value, over |det|."""
    K = np.asarray(K, np.float64)
    a, b, c, d, e, f, g, h, k = (np.abs(K[:, i, j]) for i in range(3) for j in range(3))
    adj = np.stack([np.stack([e * k + f * h, b * k + c * h, b * f + c * e], -1),
                    np.stack([d * k + f * g, a * k + c * g, a * f + c * d], -1),
                    np.stack([d * h + e * g, a * h + b * g, a * e + b * d], -1)], 1)
    return adj / np.abs(np.linalg.det(K))[:, None, None]


def cloud_ref64(depths, scales, K, poses):
    """world [N,H,W,3] in float64 of the float32 inputs (slam.py:396-408, slam_utils.py:82-121), and `mag` [N,H,W,3]: per
    coordinate the sum of the absolute values of every term that enters it - the size its ~20 fp32 roundings are relative to
    (products of K^-1's adjugate, the three terms of each local coordinate, depth x scale, the four terms of the pose row)."""
    N, H, W = depths.shape
    K64, P = np.asarray(K, np.float64), np.asarray(poses, np.float64)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([x, y, np.ones_like(x)], -1)                                   # [H,W,3]
    z = np.asarray(depths, np.float64) * np.asarray(scales, np.float64).reshape(N, 1, 1)
    Kinv = np.linalg.inv(K64)
    local = np.einsum("nij,hwj->nhwi", Kinv, pix) * z[..., None]
    world = np.einsum("nij,nhwj->nhwi", P[:, :3, :3], local) + P[:, None, None, :3, 3]
    mloc = np.einsum("nij,hwj->nhwi", _abs_adjugate_inverse(K64), pix) * np.abs(z)[..., None]
    mag = np.einsum("nij,nhwj->nhwi", np.abs(P[:, :3, :3]), mloc) + np.abs(P[:, None, None, :3, 3])
    return world, mag


CLOUD_BOUND = 32 * ULP24          # x mag, per coordinate


def ply_record_fields(rec):
    """uint8 [M,27] -> (float64 [M,3], uint8 [M,3])."""
    rec = np.ascontiguousarray(rec)
    return rec[:, :24].copy().view("<f8").reshape(-1, 3), rec[:, 24:]


# ------------------------------------------------------------------------------------------ sta_estimate_intrinsics / _scale
# (B, H, W, blocks per image of the partial kernel: ceil(H W / 2048) capped at 256)
INTR_SHAPES = [(6, 1, 1, 1), (6, 3, 683, 2), (6, 257, 512, 65), (1, 513, 1024, 256)]
INTR_SHARED = (0, 1, 2, 3)
COND_MAX = 1e3


def intr_nblk(H, W):
    return max(1, min(256, (H * W + 2047) // 2048))


def intr_inputs(B, H, W, seed=43):
    """pts [B,H,W,3], conf [B,H,W] float32: a pinhole camera (focal 0.9 max(H, W) + 20, principal point (W/2, H/2)) looking at depths
    in [1, 5) with 2 % noise on X / Z and Y / Z; confidences in [0.5, 3).  From 100 pixels on, 1 % of the pixels get Z = 0 (half of
    them with X = Y = 0: 0 / 0; the other half X / 0), 1 % Z < 0 (point mirrored through the centre: X / Z unchanged), and 1 % each a
    confidence of 0, 1e-7 and -1 (all below the 1e-6 clamp)."""
    rng = np.random.default_rng(seed + B * H * W)
    f = 0.9 * max(H, W) + 20
    v, u = np.meshgrid(np.arange(H) - H / 2.0, np.arange(W) - W / 2.0, indexing="ij")
    Z = 1 + 4 * rng.random((B, H, W))
    X = (u / f * (1 + 0.02 * rng.standard_normal((B, H, W)))) * Z
    Y = (v / f * (1 + 0.02 * rng.standard_normal((B, H, W)))) * Z
    conf = 0.5 + 2.5 * rng.random((B, H, W))
    if H * W >= 100:
        r = rng.random((B, H, W))
        z0 = r < 0.01
        Z[z0] = 0.0
        both = z0 & (rng.random((B, H, W)) < 0.5)
        X[both] = 0.0; Y[both] = 0.0
        neg = (r >= 0.01) & (r < 0.02)
        X[neg] *= -1; Y[neg] *= -1; Z[neg] *= -1
        conf[(r >= 0.02) & (r < 0.03)] = 0.0
        conf[(r >= 0.03) & (r < 0.04)] = 1e-7
        conf[(r >= 0.04) & (r < 0.05)] = -1.0
    return np.stack([X, Y, Z], -1).astype(F32), conf.astype(F32)


def intr_terms(pts, conf):
    """The fp32 products the kernel sums, [B, H*W] each: fx numerator / denominator, fy numerator / denominator (w = max(conf, 1e-6),
    xz = X / Z with non-finite -> 0, (w * xz) * u and (w * xz) * xz evaluated left to right in fp32), and the UNCLAMPED confidences."""
    pts = np.asarray(pts, F32); conf = np.asarray(conf, F32)
    B, H, W, _ = pts.shape
    v, u = np.meshgrid(np.arange(H, dtype=F32) - F32(H / 2.0), np.arange(W, dtype=F32) - F32(W / 2.0), indexing="ij")
    u = u.reshape(1, -1).astype(F32); v = v.reshape(1, -1).astype(F32)
    X, Y, Z = (pts[..., k].reshape(B, -1) for k in range(3))
    w = np.maximum(conf.reshape(B, -1), F32(1e-6))
    with np.errstate(divide="ignore", invalid="ignore"):
        xz = (X / Z).astype(F32); yz = (Y / Z).astype(F32)
    xz = np.where(np.isfinite(xz), xz, F32(0)); yz = np.where(np.isfinite(yz), yz, F32(0))
    wx = (w * xz).astype(F32); wy = (w * yz).astype(F32)
    return (wx * u).astype(F32), (wx * xz).astype(F32), (wy * v).astype(F32), (wy * yz).astype(F32), conf.reshape(B, -1)


def intr_groups(B, shared):
    """Image groups one K is estimated over: shared 0 -> one per image, 1 -> all, g >= 2 -> consecutive groups of g."""
    g = 1 if shared == 0 else (B if shared == 1 else shared)
    assert B % g == 0
    return [list(range(i, i + g)) for i in range(0, B, g)]


def intr_ref(pts, conf, shared, order="forward"):
    """K [groups,3,3] (shared 1: [3,3]) and conf_mean [B] float32 from the fp32 terms summed in float64.  order: "forward" numpy's
    pairwise sum, "reverse" the same over the reversed terms, "blocks" 2048-element blocks summed first (the kernel's shape)."""
    B, H, W, _ = np.asarray(pts).shape
    terms = intr_terms(pts, conf)

    def tot(t, idx):
        a = t[idx].astype(np.float64).reshape(-1)
        if order == "reverse":
            a = a[::-1]
        if order == "blocks":
            pad = (-len(a)) % 2048
            return float(np.concatenate([a, np.zeros(pad)]).reshape(-1, 2048).sum(1).sum())
        return float(a.sum())

    groups = intr_groups(B, shared)
    K = np.zeros((len(groups), 3, 3), F32)
    for gi, idx in enumerate(groups):
        K[gi, 0, 0] = F32(tot(terms[0], idx) / tot(terms[1], idx))
        K[gi, 1, 1] = F32(tot(terms[2], idx) / tot(terms[3], idx))
        K[gi, 0, 2] = F32(W / 2.0); K[gi, 1, 2] = F32(H / 2.0); K[gi, 2, 2] = 1
    cm = np.array([F32(tot(terms[4], [b]) / (float(H) * W)) for b in range(B)], F32)
    return (K[0] if shared == 1 else K), cm


def conditioning(terms):
    """sum |t| / |sum t| of a set of terms (float64)."""
    t = np.asarray(terms, np.float64).reshape(-1)
    return float(np.abs(t).sum() / max(abs(t.sum()), 1e-300))


SCALE_N = (1, 63, 64, 65, 1023, 1024, 1025, 50176 + 3)


def scale_inputs(n, seed=47):
    """Di, Dj (depths in [1, 5), Dj = 1.3 Di with 5 % noise), ci, cj (confidences in [0.2, 2); every 16th pair has a product below the
    1e-6 clamp)."""
    rng = np.random.default_rng(seed + n)
    Di = 1 + 4 * rng.random(n)
    Dj = 1.3 * Di * (1 + 0.05 * rng.standard_normal(n))
    ci = 0.2 + 1.8 * rng.random(n); cj = 0.2 + 1.8 * rng.random(n)
    ci[::16] = 1e-4; cj[::16] = 1e-4
    return tuple(a.astype(F32) for a in (Di, Dj, ci, cj))


def scale_terms(Di, Dj, ci, cj):
    w = np.maximum((ci * cj).astype(F32), F32(1e-6))
    wd = (w * Di).astype(F32)
    return (wd * Dj).astype(F32), (wd * Di).astype(F32)


def scale_ref(Di, Dj, ci, cj, reverse=False):
    num, den = scale_terms(Di, Dj, ci, cj)
    s = slice(None, None, -1) if reverse else slice(None)
    return F32(num.astype(np.float64)[s].sum() / den.astype(np.float64)[s].sum())


# ------------------------------------------------------------------------------------------ sta_pack_compact
PACK_B = (1, 3)
PACK_HW = [(1, 1), (15, 17), (1, 257), (28, 36), (1000, 1100)]          # H*W = 1, 255, 257, 1008, 1100000
PACK_GX_CAP = 1024


def pack_trips(H, W):
    """Trips of the copy loop of the first thread: 2 H W elements over min(ceil(2 H W / 2048), 1024) blocks of 256 threads - at most
    8 while the grid is below its cap."""
    n = 2 * H * W
    gx = max(1, min(PACK_GX_CAP, (n + 2047) // 2048))
    return (n + gx * 256 - 1) // (gx * 256)
