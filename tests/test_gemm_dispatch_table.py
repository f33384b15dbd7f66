"""CPU: the tile-family table and the existence predicate of the launch layer (sta_launch.inc), held to two independent records.

launch_gemm dispatches by ONE table (struct TileFamily) and ONE predicate (gemm_has_kernel, exported by the test-hooks build as
sta_debug_gemm_has_kernel): gemm_plan asks it at run time, the dispatch asks it in `if constexpr`.  Needs the built libraries, no GPU.
  * the predicate agrees, over the whole cross product of its arguments, with the restatements the plan sweeps already use
    (tests/test_gemm_plan.py: has_kernel; tests/test_conv_plan.py: where the halo-tiled family is legal, the fused head's one shape);
  * the kernels the product library really holds are the table's: every admitted combination has its gemm2_kernel / conv3h_kernel /
    gemm_kernel symbol with exactly the table's template arguments, and every such symbol (main-loop ablation argument 0) belongs to an admitted
    combination or is the varlen (VlGeo) form of one.  The set of instantiated kernels cannot drift silently - each costs compile time.
Symbol NAMES only are read from the code object.
"""
import itertools
import os
import re
import subprocess
import sys
import tempfile

import pytest

import test_gemm_plan as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

A_DENSE, A_CONV3 = 0, 1
EPI_F32, EPI_F16, EPI_QKV, EPI_CONVT, EPI_GELU, EPI_F32R, EPI_HEAD = range(7)
DENSE_NAME = {v: k for k, v in TG.EPI.items()}           # the epilogues tests/test_gemm_plan.py sweeps, by id
FAMILIES = range(1, 9)
NS = (64, 128, 256, 384)
# The table, restated: family -> [(BM, BN, wave rows, wave columns, DMA stages)]; family 6 has its 4-wave and its 8-wave layout
# (the latter in the split arithmetics only), family 8 (conv3h_kernel: no stage argument) one tile per Cout.
TABLE = {2: [(256, 256, 4, 4, 2)], 3: [(192, 256, 3, 4, 2)], 5: [(192, 128, 2, 4, 2)], 6: [(128, 64, 2, 2, 3), (128, 64, 4, 2, 3)]}
HALO = {128: (256, 128, 4, 4), 256: (256, 256, 4, 4)}


def restated(amode, epi, family, mx, N, cstride):
    """Which combinations launch_gemm has a kernel for, from the restatements of the plan tests (the arithmetic enters as mx only:
    every admitted combination exists in the split precisions and in plain f16)."""
    if amode == A_DENSE:
        if epi in DENSE_NAME:
            return TG.has_kernel(family, DENSE_NAME[epi], mx)
        if epi == EPI_CONVT:                               # the head's transposed convolutions: every family, f16mx on the DMA ones
            return family in (2, 3, 5, 6) or (family == 1 and not mx)
        return False                                       # the fused head is a convolution epilogue
    if epi not in (EPI_F16, EPI_HEAD):                     # tests/test_conv_plan.py: the two convolution epilogues
        return False
    if family == 8:                                        # ... its legal8, and the fused head's single 128-channel tile
        return cstride == 1 and (N == 128 or (N == 256 and epi == EPI_F16))
    if epi == EPI_HEAD:
        return family == 5 and N == 128
    return family in (2, 3, 5, 6) or (family == 1 and not mx)


@pytest.fixture(scope="module")
def lib():
    return TG._load_lib()


def test_predicate_agrees_with_the_restatements(lib):
    n = 0
    for amode, epi, family, mx, split, N, cstride in itertools.product((A_DENSE, A_CONV3), range(7), FAMILIES, (0, 1), (0, 1), NS, (1, 2)):
        got = lib.sta_debug_gemm_has_kernel(amode, epi, family, mx, split, N, cstride)
        assert got == int(restated(amode, epi, family, bool(mx), N, cstride)), (amode, epi, family, mx, split, N, cstride, got)
        n += 1
    assert n == 2 * 7 * 8 * 2 * 2 * 4 * 2


def kernel_symbols():
    """The demangled gemm2_kernel<...> / conv3h_kernel<...> / gemm_kernel<...> (family 1) template argument lists of the product
    library's gfx950 code object."""
    import kernel_resources as kr
    if not os.path.exists(kr.LIB):
        pytest.skip("libsta_mi355.so not built here (python -m vista_slam_amd.build)")
    readelf = os.path.join(kr.LLVM, "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("ROCm LLVM tools (llvm-readelf) not installed on this box")
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(kr.code_object(kr.LIB))
        path = f.name
    try:
        syms = subprocess.run([readelf, "-s", "-W", "--demangle", path], capture_output=True, text=True, check=True).stdout
    finally:
        os.unlink(path)
    out = {"gemm2_kernel": set(), "conv3h_kernel": set(), "gemm_kernel": set()}
    for ln in syms.splitlines():
        m = re.search(r" FUNC .* void (gemm2_kernel|conv3h_kernel|gemm_kernel)<([^>]*)>\(", ln)
        if m:
            out[m.group(1)].add(tuple(a.strip() for a in m.group(2).split(",")))
    return out


def b(x):
    return "true" if x else "false"


def test_kernel_symbols_are_the_table(lib):
    syms = kernel_symbols()
    assert len(syms["gemm2_kernel"]) > 100 and len(syms["conv3h_kernel"]) >= 10, {k: len(v) for k, v in syms.items()}
    want1, want2, want3 = set(), set(), set()
    for amode, epi, family, mx, split, N in itertools.product((A_DENSE, A_CONV3), range(7), FAMILIES, (0, 1), (0, 1), NS):
        if not lib.sta_debug_gemm_has_kernel(amode, epi, family, mx, split, N, 1):
            continue
        S = bool(split or mx)                              # f16mx operands are split operands
        if family == 1:                                    # gemm_kernel<SPLIT, AMODE, EPI> (gemm.h): its 128x128 tile is no argument
            want1.add((b(S), str(amode), str(epi)))
            continue
        if family == 8:
            bm, bn, wms, wns = HALO[N]
            want3.add((b(S), str(epi), str(bm), str(bn), str(wms), str(wns), b(mx)))
            continue
        for bm, bn, wms, wns, nstg in TABLE[family]:
            if (wms, wns) == (4, 2) and not S:
                continue
            want2.add((b(S), str(amode), str(epi), str(bm), str(bn), str(wms), str(wns), "0", str(nstg), b(mx)))
    # the varlen forms (sta_head_pts_varlen): the geometry-decoding launches - convolutions and transposed convolutions - in the
    # split arithmetics
    varlen2 = {k + ("VlGeo",) for k in want2 if k[0] == "true" and (k[1] == str(A_CONV3) or k[2] == str(EPI_CONVT))}
    varlen3 = {k + ("VlGeo",) for k in want3 if k[0] == "true"}
    have2 = {k for k in syms["gemm2_kernel"] if k[7] == "0"}            # argument 7: the main-loop ablation (0 = product)
    assert want2 - have2 == set(), ("admitted combinations without a kernel", sorted(want2 - have2))
    assert have2 - want2 - varlen2 == set(), ("kernels no admitted combination launches", sorted(have2 - want2 - varlen2))
    assert varlen2 - have2 == set(), sorted(varlen2 - have2)
    assert syms["gemm_kernel"] == want1, ("family 1", sorted(want1 - syms["gemm_kernel"]), sorted(syms["gemm_kernel"] - want1))
    have3 = syms["conv3h_kernel"]
    assert want3 - have3 == set(), ("admitted halo combinations without a kernel", sorted(want3 - have3))
    assert have3 - want3 - varlen3 == set(), ("halo kernels no admitted combination launches", sorted(have3 - want3 - varlen3))
    assert varlen3 - have3 == set(), sorted(varlen3 - have3)
