"""The f16x3 / f16 main loop of gemm2_body on 16x16x32 MFMAs (round 7).

(a) GPU: small-integer operands, so that every product and every partial sum is exact in fp32 whatever the summation order -
    the result must equal the integer product EXACTLY.  Any row / column mis-placement of the 16x16 sub-blocks, of the A-row
    permutation or of the permlane16 exchange that rebuilds the 32x32 accumulator layout shows up as a wrong integer.
(b) CPU: the hot gemm2_kernel symbols of the built code object issue v_mfma_f32_16x16x32_f16 (their skinny tail blocks keep
    32x32x16), use no scratch and stay within the VGPR budget of their occupancy (two 192x128 workgroups or one 16-wave
    256x256 workgroup per CU: 128; 12 waves: 168)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

A_DENSE, EPI_F32 = 0, 0


def _int_gemm(precision, M, N, K, variant, resid=False, via_f16=0, seed=0, tail=0, plan=None, wg_over=None):
    """tail: the last `tail` rows are pose-token rows (tail hint).  The output starts as NaN - an element no block writes fails -
    or, with resid, as the residual itself (the in-place form x += A W^T: a row that two blocks add shows up as a wrong integer).
    plan: the (family, m_tail) the launch must have run under; wg_over: its grid must have MORE main workgroups than this.
    Long K: operands in {-1, 0, 1} keep every sum exact."""
    import torch
    import gpu_checks as G
    from vista_slam_amd import _lib
    m, lib, h = G.kernel_handle(precision, variant)
    rng = np.random.default_rng(seed)
    lim = 3 if K <= 256 else 1
    A = rng.integers(-lim, lim + 1, size=(M, K)).astype(np.float32)
    Wt = rng.integers(-lim, lim + 1, size=(N, K)).astype(np.float32)
    b = rng.integers(-8, 9, size=N).astype(np.float32)
    R = rng.integers(-8, 9, size=(M, N)).astype(np.float32) if resid else None
    ref = A.astype(np.float64) @ Wt.astype(np.float64).T + b.astype(np.float64)      # (integers: exact in float64)
    if resid:
        ref = ref + R.astype(np.float64)
    assert np.abs(ref).max() < 2 ** 11      # exact in fp32 and, for the plane epilogue, in the fp16 hi plane
    Ad, Wd, bd = G.dev(A), G.dev(Wt), G.dev(b)
    out = G.dev(R) if resid else torch.full((M, N), float("nan"), device=G.DEV)
    _lib.check(lib.sta_debug_set_tail_hint(h, tail))
    try:
        _lib.check(lib.sta_debug_gemm(h, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), M, N, K, 0, via_f16,
                                      out.data_ptr() if resid else None, out.data_ptr(), G.st()))
        torch.cuda.synchronize()
        got_plan = G.last_plan(lib, h)
    finally:
        _lib.check(lib.sta_debug_set_tail_hint(h, 0))
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    if plan is not None:
        assert (got_plan["family"], got_plan["m_tail"]) == plan, got_plan
    if wg_over is not None:
        assert got_plan["tiles_m"] * got_plan["tiles_n"] * got_plan["ksplit"] > wg_over, got_plan
    got = out.cpu().numpy().astype(np.float64)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{len(bad)} wrong elements, first (row, col) {bad[:4].tolist()}: got {got[tuple(bad[0])]} want {ref[tuple(bad[0])]}"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("kw", [
    # forced families (variant 2: 256x256 / 16 waves, 3: 192x256 / 12 waves, 4: 192x128 / 8 waves) apply above the small-grid
    # predicate (M > 640 and >= 192 tiles of 192x128): 6145 = 32 x 192 + 1 = 24 x 256 + 1, 6337 = 33 x 192 + 1 = 24 x 256 + 193,
    # 6900 = 35 x 192 + 180 = 26 x 256 + 244; fp32 and in-place-residual epilogues
    dict(M=6145, N=768, K=256, variant=2), dict(M=6900, N=768, K=224, variant=2, resid=True),
    dict(M=6337, N=768, K=256, variant=3), dict(M=6900, N=768, K=160, variant=3, resid=True),
    dict(M=6145, N=768, K=256, variant=4), dict(M=6337, N=768, K=192, variant=4, resid=True), dict(M=6900, N=768, K=96, variant=4),
    # the LDS-staged fp16-plane epilogue (integers below 2^11 are exact in the hi plane)
    dict(M=6900, N=768, K=64, variant=4, via_f16=1),
    # small-grid 128x64 ring family (product selection; K = 1024 on 8 tiles is split in K), M tails 193 / 513 / 700
    dict(M=100, N=256, K=1024, variant=0), dict(M=64, N=128, K=96, variant=0, resid=True),
    dict(M=193, N=768, K=256, variant=0), dict(M=513, N=768, K=128, variant=0, resid=True), dict(M=700, N=768, K=96, variant=0),
])
def test_gemm_integer_exact(prec, kw):
    _int_gemm(prec, **kw)


# Pose-token row tails (GemmParams::m_tail) on the skinny tail blocks, exact: forced families 2 (256x256), 3 (192x256), 4 (192x128)
# and the automatic choice, fp32 and in-place-residual epilogues.  Under mlp_mx (precision f16x3m: mlp.fc2's f16mx arithmetic)
# forced family 2 runs 192x256: 25 x 256 patch rows are no whole count of 192-row tiles, so the pose rows must stay in the main
# tiles (before the row tail was checked against the remapped tile, the last main tile and the tail blocks both added them).
TAIL_CASES = [dict(M=24 * 256 + 16, N=768, K=256, variant=2, tail=16, plan=(2, 16)),
              dict(M=24 * 256 + 32, N=768, K=224, variant=2, tail=32, resid=True, plan=(2, 32)),
              dict(M=36 * 192 + 1, N=768, K=224, variant=3, tail=1, plan=(3, 1)),
              dict(M=36 * 192 + 20, N=768, K=160, variant=3, tail=20, resid=True, plan=(3, 20)),
              dict(M=36 * 192 + 16, N=768, K=192, variant=4, tail=16, resid=True, plan=(5, 16)),
              dict(M=36 * 192 + 16, N=768, K=3072, variant=0, tail=16, resid=True, plan=(5, 16)),
              dict(M=12 * 192 + 2, N=2304, K=1024, variant=0, tail=2, plan=(5, 2))]
MX_TAIL_CASES = [dict(M=36 * 192 + 16, N=768, K=1024, variant=3, tail=16, resid=True, plan=(3, 16)),
                 dict(M=36 * 192 + 1, N=768, K=256, variant=4, tail=1, plan=(5, 1)),
                 dict(M=12 * 192 + 32, N=2304, K=3072, variant=0, tail=32, resid=True, plan=(5, 32)),
                 dict(M=48 * 192 + 16, N=768, K=256, variant=2, tail=16, resid=True, plan=(3, 16)),
                 dict(M=25 * 256 + 16, N=768, K=256, variant=2, tail=16, resid=True, plan=(3, 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,kw", [(p, kw) for p in ("f16x3", "f16") for kw in TAIL_CASES] + [("mlp_mx", kw) for kw in MX_TAIL_CASES])
def test_gemm_tail_integer_exact(prec, kw):
    _int_gemm(prec, **kw)


# Rows of the launch layer's dispatch table (sta_launch.inc: TileFamily x has_kernel) that no other case of the kernel tests launches,
# at the smallest shapes that reach them, K = 2 GEMM_BK:
#   * the fp32 epilogue in the f16mx arithmetic on 192x256 (forced 3; 6145 = 32 x 192 + 1 rows: above the small-grid predicate);
#   * the plane epilogue on the 4-WAVE form of the small-grid family, split and f16mx operands: 513 rows x 3328 columns = 5 x 52 = 260
#     workgroups, more than the 256 up to which the 8-wave form runs (and too many tiles for K slices);
#   * the in-place residual epilogue on the register-staged 128x128 kernel (forced 1).
DISPATCH_CASES = [("mlp_mx", dict(M=6145, N=768, K=64, variant=3, plan=(3, 0))),
                  ("f16x3", dict(M=513, N=3328, K=64, variant=0, via_f16=1, plan=(6, 0), wg_over=256)),
                  ("head_mx", dict(M=513, N=3328, K=64, variant=0, via_f16=1, plan=(6, 0), wg_over=256)),
                  ("f16x3", dict(M=6145, N=768, K=64, variant=1, resid=True, plan=(1, 0))),
                  ("f16", dict(M=6145, N=768, K=64, variant=1, resid=True, plan=(1, 0)))]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,kw", DISPATCH_CASES)
def test_gemm_dispatch_rows_integer_exact(prec, kw):
    _int_gemm(prec, **kw)


def test_small_shapes_take_the_ring_family():
    """The variant-0 shapes of the exact test run on the small-grid family (pick_family -> 6); the forced shapes do not."""
    from vista_slam_amd import _lib
    lib = _lib.load_test()
    for M, N, K in ((100, 256, 1024), (64, 128, 96), (193, 768, 256), (513, 768, 128), (700, 768, 96)):
        assert lib.sta_debug_pick_family(A_DENSE, EPI_F32, M, N, K, 1, 1, 0, 0) == 6, (M, N, K)
    for M in (6145, 6337, 6900):
        assert lib.sta_debug_pick_family(A_DENSE, EPI_F32, M, 768, 256, 1, 1, 0, 0) != 6, M


# hot f16x3 main loops (split operands, dense A, no MX): symbol fragment -> VGPR cap
HOT = {"ILb1ELi0ELi0ELi192ELi128ELi2ELi4ELi0ELi2ELb0E": 128,     # fp32 epilogue, 192x128
       "ILb1ELi0ELi5ELi192ELi128ELi2ELi4ELi0ELi2ELb0E": 128,     # in-place residual (attn.proj class)
       "ILb1ELi0ELi4ELi192ELi128ELi2ELi4ELi0ELi2ELb0E": 128,     # GELU
       "ILb1ELi0ELi2ELi192ELi128ELi2ELi4ELi0ELi2ELb0E": 128,     # QKV / RoPE
       "ILb1ELi0ELi4ELi256ELi256ELi4ELi4ELi0ELi2ELb0E": 128,     # fc1, 256x256
       "ILb1ELi0ELi5ELi256ELi256ELi4ELi4ELi0ELi2ELb0E": 128,
       "ILb1ELi0ELi4ELi192ELi256ELi3ELi4ELi0ELi2ELb0E": 168,     # 192x256 / 12 waves
       "ILb1ELi0ELi5ELi192ELi256ELi3ELi4ELi0ELi2ELb0E": 168}     # fc2 / proj class


def test_hot_gemm_kernels_use_16x16x32_mfma():
    import kernel_resources as kr
    if not os.path.exists(kr.LIB):
        pytest.skip("libsta_mi355.so not built here (python -m vista_slam_amd.build)")
    if not os.path.exists(os.path.join(kr.LLVM, "llvm-objdump")):
        pytest.skip("ROCm LLVM tools (llvm-objdump) not installed on this box")
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(kr.code_object(kr.LIB))
        path = f.name
    try:
        dis = subprocess.run([os.path.join(kr.LLVM, "llvm-objdump"), "-d", path], capture_output=True, text=True).stdout
        notes = subprocess.run([os.path.join(kr.LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True).stdout
    finally:
        os.unlink(path)
    mfma, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
        if m:
            cur = m.group(1)
            mfma[cur] = set()
        elif cur is not None and "v_mfma" in ln:
            mfma[cur].add(ln.split()[0])
    meta = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        g = {k: re.search(r"\.%s:\s+(\S+)" % k, blk) for k in ("name", "vgpr_count", "private_segment_fixed_size", "vgpr_spill_count")}
        meta[g["name"].group(1)] = (int(blk.split()[0]), int(g["vgpr_count"].group(1)), int(g["private_segment_fixed_size"].group(1)),
                                    int(g["vgpr_spill_count"].group(1)))
    names = [n for n in mfma if n.startswith("_Z17gemm2_pair_kernel")] + \
            [n for n in mfma if n.startswith("_Z12gemm2_kernel") and any(f in n for f in HOT)]
    assert len(names) == len(HOT) + 1, sorted(names)
    for n in names:
        cap = 128 if n.startswith("_Z17") else next(c for f, c in HOT.items() if f in n)
        agpr, vgpr, scratch, spill = meta[n]
        assert "v_mfma_f32_16x16x32_f16" in mfma[n], (n, sorted(mfma[n]))
        assert scratch == 0 and spill == 0, (n, scratch, spill)
        assert agpr + vgpr <= cap, (n, vgpr, agpr, cap)
