"""Case tables and plain float64 references of the row kernels: the residual GEMM + LayerNorm pair (gemm_resid_ln: the slab
split-K residual GEMM and resid_ln_kernel, or the in-place GEMM and ln_kernel) and LayerNorm alone (sta_debug_layernorm,
sta_encoder_norm).  Importable without a GPU (tests/test_row_post_cpu.py runs every condition stated here on the CPU);
tests/test_row_gpu.py runs the kernels."""
import numpy as np

# ------------------------------------------------------------------------------------------ residual GEMM + LayerNorm
# (M, N, K) -> does the launch plan hand its K slices to resid_ln_kernel (slab_ks > 1)?  The expectation is a statement about the
# CASE, asserted against sta_debug_gemm_plan (epilogue 5... the in-place fp32 one) on the CPU and against the last-plan record on
# the GPU; the rule itself lives in sta_launch.inc only.
RESID_CASES = [
    # two slices; M < 128; 16 of the 256 threads of resid_ln_kernel hold columns
    dict(M=5, N=64, K=256, slab=True),
    # SLAM-scale attn.proj / mlp.fc2 (224 x 224, one and two views)
    dict(M=196, N=768, K=768, slab=True),
    dict(M=392, N=768, K=3072, slab=True),
    # the widest legal row (every thread of resid_ln_kernel holds columns), M odd
    dict(M=197, N=1024, K=1024, slab=True),
    # crosses a 128-row tile
    dict(M=129, N=192, K=512, slab=True),
    # the largest SLAM-scale batch: 13 x 6 = 78 tiles of 192 x 128 is still BELOW the small-grid predicate (< 192 tiles), and the 228
    # tiles of 128 x 64 take two slices - the last shape on the slab path, 19 row tiles
    dict(M=2400, N=768, K=768, slab=True),
    # above the predicate (33 x 6 = 198 tiles): the in-place GEMM on a throughput family, then plain ln_kernel with two affine sets
    dict(M=6200, N=768, K=768, slab=False),
]
RESID_SETS = ("one", "two", "add")          # one affine set, two, add only (no planes written)
EPS = 1e-6
EPI_F32 = 0                                 # sta_launch.inc: the epilogue gemm_resid_ln launches below the predicate (in place, with a slab)
EPI_F32R = 5                                # ... and above it (gemm_f32: the specialised in-place residual epilogue)


def case_id(c):
    return f"{c['M']}x{c['N']}x{c['K']}"


def resid_inputs(c, kind, seed=7):
    """-> A [M,K], W [N,K], bias [N], x [M,N] float32.  kind "gauss": the distributions of check_gemm (tests/gpu_checks.py).
    kind "int": small integers whose every partial sum is an integer of magnitude <= 3 x 512 + 32 + 100 = 1668 < 2048 BY
    CONSTRUCTION (A in [-3, 3], every row of W has min(K, 512) entries of +-1, the rest 0, bias in [-32, 32], x in [-100, 100]):
    fp16 holds every operand and every partial sum, so the result is the same integer whatever the slice count or summation order."""
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.default_rng(seed + M + 3 * N + 5 * K)
    if kind == "gauss":
        A = (rng.standard_normal((M, K)) * 1.3).astype(np.float32)
        W = (rng.standard_normal((N, K)) * 0.1).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32)
        x = rng.standard_normal((M, N)).astype(np.float32)
        return A, W, b, x
    assert kind == "int"
    A = rng.integers(-3, 4, size=(M, K)).astype(np.float32)
    W = (rng.integers(0, 2, size=(N, K)) * 2 - 1).astype(np.float32)
    if K > 512:
        keep = np.argsort(rng.random((N, K)), axis=1)[:, :512]
        mask = np.zeros((N, K), bool)
        np.put_along_axis(mask, keep, True, 1)
        W = W * mask
    b = rng.integers(-32, 33, size=N).astype(np.float32)
    x = rng.integers(-100, 101, size=(M, N)).astype(np.float32)
    return A, W.astype(np.float32), b, x


def int_partial_bound(A, W, b, x):
    """The largest magnitude ANY partial sum of x + b + sum_k A W can reach: sum of the absolute values of the terms."""
    return float((np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64)) + np.abs(x.astype(np.float64))).max())


def resid_ref64(A, W, b, x):
    return x.astype(np.float64) + A.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)


def affine_sets(N, seed=11):
    """Two affine sets (g1, b1, g2, b2) float32 [N] whose LayerNorm outputs differ in EVERY row by far more than any bar:
    independent Gaussian gains and biases (asserted per case by set_separation)."""
    rng = np.random.default_rng(seed + N)
    return tuple(rng.standard_normal(N).astype(np.float32) for _ in range(4))


def layernorm64(x, g, b, eps=EPS):
    """nn.LayerNorm (biased variance, eps inside the square root) in float64 of the given values."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    var = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def row_rel_l2(got, ref):
    """rel-L2 of every row, [M]; a NaN in a row makes its error NaN."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    return np.sqrt(((got - ref) ** 2).sum(-1) / np.maximum((ref ** 2).sum(-1), 1e-300))


def row_max_rel(got, ref):
    """max |got - ref| / max |ref| of every row, [M]."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    return np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-300)


def worst(v):
    """-> (index, value) of the worst entry; NaN wins."""
    v = np.where(np.isnan(v), np.inf, np.asarray(v, np.float64))
    i = int(np.argmax(v))
    return i, float(v[i])


def set_separation(x2, g1, b1, g2, b2, eps=EPS):
    """Per row: rel-L2 distance of set 2's expected planes from set 1's."""
    return row_rel_l2(layernorm64(x2, g2, b2, eps), layernorm64(x2, g1, b1, eps))


# ------------------------------------------------------------------------------------------ LayerNorm alone
LN_M = (1, 2, 3, 4, 5, 37)
LN_C = (4, 8, 96, 252, 256, 260, 1020, 1024)
LN_KINDS = ("random", "constant", "offset", "outlier")


def ln_inputs(M, C, kind, seed=19):
    """x [M,C], g [C], b [C] float32.  random: the rows of test_layernorm (3 N(0,1) + 0.7); constant: every row one value (a
    different one per row, none a power of two), the output must be the bias; offset: mean 1e4, unit spread; outlier: N(0,1)
    with one entry of 1e3 at a different column per row."""
    rng = np.random.default_rng(seed + 1000 * M + C + 7 * LN_KINDS.index(kind))
    g = rng.standard_normal(C).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    if kind == "random":
        x = rng.standard_normal((M, C)) * 3 + 0.7
    elif kind == "constant":
        x = np.repeat(0.7 + 1.3 * np.arange(M)[:, None] + rng.random((M, 1)), C, 1)
    elif kind == "offset":
        x = 1e4 + rng.standard_normal((M, C))
    else:
        x = rng.standard_normal((M, C))
        x[np.arange(M), (np.arange(M) * 37 + 3) % C] = 1e3
    return x.astype(np.float32), g, b
