"""CPU: the launch plan of the two-group attention kernel (attn_mixed_kernel) and its workgroup map, host only.

run_attn_mixed runs exactly the plan of attn_mixed_plan (sta_launch.inc; sta_debug_attn_mixed_plan), and the kernel maps its
workgroups by the arithmetic sta_debug_attn_mixed_block_map repeats on the host (attn_block_map over both groups' query blocks,
group a's logical ids first) - so this needs the built test library but no GPU.

  * SWEEP: every ordered pair of different patch grids up to 32 x 32 per side (354 token counts: 124 962 pairs), B = 1 .. 16,
    decoder self attention (nq == nk per group) and cross attention ((N1, N2) | (N2, N1)): per-group pose mode from the group's nq,
    tiles / tail / pose scratch from the group's nk, prefetch from the grid of the whole launch, LDS of the launch covers both
    groups.  The plan does not depend on the precision except for the LDS bytes: the sweep runs the f16x3 form, every 97th shape
    also the f16 form.
  * the workgroup map is a bijection onto (sequence, head, query block), covers every query of every sequence exactly once, and
    the blocks of one (sequence, head) stay on one XCD except where an XCD's contiguous range ends,
  * equal groups (and S2 == 0) reduce to attn_plan of the same shape, field by field,
  * COVERAGE: every group class (tests/attention_mixed_cases.py) the sweep reaches is the class of a case of the GPU matrix, in
    the same slot.  Zero uncovered, no allow-list.
  * code-object pins of attn_mixed_kernel: no scratch, no spills, >= 2 waves per SIMD, fp16 MFMAs only.
"""
import ctypes as C
import os

import pytest

import attention_cases as AC
import attention_mixed_cases as AM

LDS_PER_CU = 160 * 1024
MIN_LDS = 2 * 2 * 64 * 128
HEADS = 12                          # the decoder's


@pytest.fixture(scope="module")
def lib():
    from vista_slam_amd import _lib
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libsta_mi355_test.so not built here (python -m vista_slam_amd.build)")
    return _lib.load_test()


_buf = (C.c_int * AM.PLAN_INTS)()


def mplan(lib, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, split=1, no_prefetch=0):
    rc = lib.sta_debug_attn_mixed_plan(S1, S2, heads, nq_a, nk_a, nq_b, nk_b, split, no_prefetch, _buf)
    assert rc == 0, (S1, S2, heads, nq_a, nk_a, nq_b, nk_b, lib.sta_last_error())
    return AM.plan_dict(_buf)


def check_plan(p, S1, S2, heads, nq, nk, split, no_prefetch):
    try:
        _check_plan(p, S1, S2, heads, nq, nk, split, no_prefetch)
    except AssertionError as e:          # (the shape is attached here: building it for each of four million plans costs more than the checks)
        raise AssertionError(f"{e} at {(S1, S2, heads, nq, nk, split, no_prefetch, p)}") from e


def _check_plan(p, S1, S2, heads, nq, nk, split, no_prefetch):
    key = None
    grid = 0
    for g, Sg in ((0, S1), (1, S2)):
        a = p["g"][g]
        assert a["pose"] == (1 if nq[g] % 128 == 0 else 2), key                     # the group's own nq decides its pose mode
        nqe = nq[g] + (1 if a["pose"] == 2 else 0)
        assert a["qblocks"] == (nqe + 127) // 128, key
        assert a["pose_blocks"] == (Sg * heads if a["pose"] == 1 else 0), key
        assert a["ntiles"] == (nk[g] + 63) // 64 and a["nfull"] == nk[g] // 64, key    # the group's own nk decides its key loop
        assert a["pose_scratch"] == ((nk[g] + 1 + 63) // 64 * 64 + 8 + 256) * 4 <= MIN_LDS, key       # sized by nk, not nq
        grid += a["qblocks"] * heads * Sg + a["pose_blocks"]
    assert p["grid"] == grid and p["nwg_a"] == p["g"][0]["qblocks"] * heads * S1, key
    any_pf = 0
    for g in (0, 1):
        a = p["g"][g]
        want = int(nk[g] <= 256 and grid <= 256 and not no_prefetch)
        assert a["prefetch"] == want, key
        any_pf |= want
        assert not want or a["ntiles"] <= 4, key
        if nk[g] % 64 == 0:
            assert a["tail_stage"] == -1, key
        elif want:
            assert a["tail_stage"] == a["ntiles"] - 1 == a["nfull"], key
        else:
            assert a["tail_stage"] == (a["ntiles"] - 1) & 1, key
    # ONE LDS size for the launch: the larger need of the two groups
    assert p["stages"] == (4 if any_pf else 2), key
    assert p["lds_bytes"] == p["stages"] * (4 if split else 2) * 64 * 128, key
    assert MIN_LDS <= p["lds_bytes"] <= LDS_PER_CU, key
    assert not split or p["lds_bytes"] >= 4 * 64 * 128, key          # the query blocks stage their output tile in LDS (f16x3 form)


def decoder_shapes():
    """(B, nq, nk) of every two-group launch of decode_mixed_impl: ordered pairs of different token counts."""
    tokens = sorted({hp * wp for hp in range(1, 33) for wp in range(1, 33)})
    for B in range(1, 17):
        for n1 in tokens:
            for n2 in tokens:
                if n1 != n2:
                    yield B, (n1, n2), (n1, n2)          # self attention of both sides
                    yield B, (n1, n2), (n2, n1)          # cross attention of both directions


@pytest.fixture(scope="module")
def sweep(lib):
    """One pass over decoder_shapes(): every plan checked, -> {(slot, *class): first shape}."""
    reached, n = {}, 0
    for B, nq, nk in decoder_shapes():
        p = mplan(lib, B, B, HEADS, nq[0], nk[0], nq[1], nk[1])
        check_plan(p, B, B, HEADS, nq, nk, 1, 0)
        if n % 97 == 0:
            check_plan(mplan(lib, B, B, HEADS, nq[0], nk[0], nq[1], nk[1], 0, 0), B, B, HEADS, nq, nk, 0, 0)
            check_plan(mplan(lib, B, B, HEADS, nq[0], nk[0], nq[1], nk[1], 1, 1), B, B, HEADS, nq, nk, 1, 1)
        for g in (0, 1):
            reached.setdefault((g,) + AM.group_class(p, g, nq[g]), (B, nq, nk))
        n += 1
    assert n == 16 * 2 * 354 * 353
    return reached


def test_plans_of_every_decoder_shape_are_consistent(sweep):
    assert len(sweep) >= 80              # the enumeration is alive (90 group classes today)


def test_every_decoder_group_class_is_in_the_gpu_matrix(sweep):
    covered = AM.covered_classes()
    uncovered = {c: eg for c, eg in sweep.items() if c not in covered}
    assert not uncovered, f"{len(uncovered)} group classes of decoder launches have no GPU case (class: first B, nq, nk): {uncovered}"


def test_case_table_claims_match_the_plan(lib):
    assert len(set(AM.IDS)) == len(AM.IDS)
    for cid, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, shift, opt5, cls_a, cls_b in AM.CASES:
        assert 0 <= shift < S1 + S2 and max(nq_a, nk_a, nq_b, nk_b) <= 1024, cid
        for split in (0, 1):
            p = mplan(lib, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, split, opt5)
            assert AM.group_class(p, 0, nq_a) == cls_a and AM.group_class(p, 1, nq_b) == cls_b, (cid, p)


def test_required_cases_are_in_the_matrix():
    have = {(c[4], c[5], c[6], c[7]) for c in AM.CASES}
    for n1, n2 in ((12, 15), (196, 140), (256, 196), (768, 196)):          # the decn_* fixtures' launches
        assert (n1, n1, n2, n2) in have or (n1, n2, n2, n1) in have, (n1, n2)
    assert (768, 196, 196, 768) in have and (196, 140, 140, 196) in have and (256, 196, 196, 256) in have
    assert any(c[8] != 0 for c in AM.CASES) and any(c[9] == 1 for c in AM.CASES)
    assert any(c[10][1] != c[11][1] for c in AM.CASES)                       # the two groups in different pose modes
    assert any(c[10][2] != c[11][2] for c in AM.CASES)                       # one group prefetches, the other runs double-buffered


def block_map(lib, S1, S2, heads, qa, qb):
    nwg = heads * (S1 * qa + S2 * qb)
    out = (C.c_int * (3 * nwg))()
    assert lib.sta_debug_attn_mixed_block_map(S1, S2, heads, qa, qb, out) == 0
    return [tuple(out[3 * b:3 * b + 3]) for b in range(nwg)]


def test_block_map_is_a_bijection_and_covers_every_query(lib):
    """Every (sequence, head, query block) of both groups exactly once; with the blocks' 128 rows every query of every sequence
    (pose mode 2: and its pose row) is owned by exactly one workgroup."""
    for S1, S2, heads in ((1, 1, 1), (1, 1, 12), (2, 2, 12), (3, 3, 5), (8, 8, 12), (16, 16, 12), (2, 0, 3), (1, 3, 2)):
        for nq_a, nq_b in ((12, 15), (196, 140), (256, 196), (768, 196), (196, 768), (1, 1024), (255, 128), (127, 129), (384, 383)):
            p = mplan(lib, S1, S2, heads, nq_a, nq_a, nq_b, nq_b)
            qa, qb = p["g"][0]["qblocks"], p["g"][1]["qblocks"]
            m = block_map(lib, S1, S2, heads, qa, qb if S2 else 0)
            want = {(s, h, q) for s in range(S1) for h in range(heads) for q in range(qa)} | \
                   {(S1 + s, h, q) for s in range(S2) for h in range(heads) for q in range(qb)}
            assert len(m) == len(want) and set(m) == want, (S1, S2, heads, nq_a, nq_b)
            assert len(m) + p["g"][0]["pose_blocks"] + p["g"][1]["pose_blocks"] == p["grid"]
            for s in range(S1 + S2):
                g = int(s >= S1)
                nq = (nq_a, nq_b)[g]
                nqe = nq + (1 if p["g"][g]["pose"] == 2 else 0)
                rows = sorted(q * 128 + r for (ss, h, q) in m if ss == s and h == 0 for r in range(128) if q * 128 + r < nqe)
                assert rows == list(range(nqe)), (S1, S2, heads, nq_a, nq_b, s)


def test_block_map_keeps_a_sequence_head_on_one_xcd(lib):
    """Workgroup b runs on XCD b % 8 and an XCD owns ONE contiguous range of logical ids: at most 7 (sequence, head) sets of query
    blocks are cut by a range boundary, every other one has all its blocks on one XCD (what attn_block_map is for)."""
    for S1, S2, heads, qa, qb in ((8, 8, 12, 6, 2), (1, 1, 12, 2, 2), (2, 2, 12, 2, 1), (3, 5, 7, 3, 4)):
        m = block_map(lib, S1, S2, heads, qa, qb)
        xcds = {}
        for b, (s, h, q) in enumerate(m):
            xcds.setdefault((s, h), set()).add(b % 8)
        assert sum(len(v) > 1 for v in xcds.values()) <= 7, (S1, S2, heads, qa, qb)


def test_equal_groups_reduce_to_attn_plan(lib):
    """S2 == 0, and two groups of the same (nq, nk = nq): the launch fields and both groups' fields are attn_plan's of that shape."""
    out = (C.c_int * len(AC.FIELDS))()
    for split in (0, 1):
        for no_prefetch in (0, 1):
            for heads in (2, 12):
                for n in (1, 12, 63, 64, 65, 128, 130, 196, 255, 256, 320, 383, 588, 640, 768, 1024):
                    for S1, S2 in ((1, 1), (2, 2), (8, 8), (3, 1), (2, 0), (11, 0)):
                        assert lib.sta_debug_attn_plan(S1 + S2, heads, n, n, 1, split, no_prefetch, out) == 0
                        one = dict(zip(AC.FIELDS, out))
                        p = mplan(lib, S1, S2, heads, n, n, n, n, split, no_prefetch)
                        key = (split, no_prefetch, heads, n, S1, S2, one, p)
                        assert (p["stages"], p["lds_bytes"], p["grid"]) == (one["stages"], one["lds_bytes"], one["grid"]), key
                        assert p["g"][0]["pose_blocks"] + p["g"][1]["pose_blocks"] == one["pose_blocks"], key
                        for g in ((0, 1) if S2 else (0,)):
                            for f in ("pose", "prefetch", "qblocks", "ntiles", "nfull", "tail_stage", "pose_scratch"):
                                assert p["g"][g][f] == one[f], (f, g) + key
                            assert AM.group_class(p, g, n)[1:] == AC.schedule_class(one, n), key


def test_mixed_plan_rejects_bad_shapes(lib):
    assert lib.sta_debug_attn_mixed_plan(0, 2, 2, 10, 10, 10, 10, 1, 0, _buf) != 0
    assert lib.sta_debug_attn_mixed_plan(2, 2, 2, 10, 10, 0, 10, 1, 0, _buf) != 0
    assert lib.sta_debug_attn_mixed_plan(1, 1, 1, 100, 8000, 100, 100, 1, 0, _buf) != 0        # pose-query scratch beyond the LDS allocation
    assert lib.sta_debug_attn_plan(2, 2, 100, 101, 1, 1, 0, (C.c_int * len(AC.FIELDS))()) != 0   # the one-group pose form still needs nq == nk


# ---------------------------------------------------------------------------------------------------------
# code-object pins of attn_mixed_kernel in the built PRODUCT library (as tests/test_attention_plan.py pins attn_kernel)
MIXED_MIN_WAVES = {"_Z17attn_mixed_kernelILb1EEv15AttnMixedParams": 2, "_Z17attn_mixed_kernelILb0EEv15AttnMixedParams": 2}


def test_attn_mixed_kernel_code_object():
    import re
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
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
        g = {k: re.search(r"\.%s:\s+(\S+)" % k, blk) for k in ("name", "vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
        meta[g["name"].group(1)] = (int(blk.split()[0]), int(g["vgpr_count"].group(1)), int(g["private_segment_fixed_size"].group(1)),
                                    int(g["vgpr_spill_count"].group(1)), int(g["sgpr_spill_count"].group(1)))
    for name, min_waves in MIXED_MIN_WAVES.items():
        assert name in meta and name in mfma, name
        agpr, vgpr, scratch, vspill, sspill = meta[name]
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        regs = (agpr + vgpr + 7) // 8 * 8
        assert min(8, 512 // regs) >= min_waves, (name, vgpr, agpr)
        assert mfma[name] and all(re.fullmatch(r"v_mfma_f32_\d+x\d+x\d+_f16", op) for op in mfma[name]), (name, sorted(mfma[name]))
