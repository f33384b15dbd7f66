"""CPU: the launch plan of the per-sequence attention kernel (attn_varlen_kernel) and its workgroup map, host only.

run_attn_varlen runs exactly the plan of attn_varlen_plan (sta_launch.inc; sta_debug_attn_varlen_plan), and the kernel maps its
workgroups by the arithmetic sta_debug_attn_varlen_block_map repeats on the host (attn_block_map, then the scan over the plan's first
logical ids) - so this needs the built test library but no GPU.

  * RULES: every plan of the sweep is checked against attn_plan's rules on each sequence's OWN numbers - pose mode from its nq, tiles /
    tail / pose scratch from its nk, prefetch from the grid of the whole launch, one LDS size that covers the hungriest sequence - and
    the table's first logical ids / pose blocks / output rows are the running sums in sequence order.
  * REACH: a sequence's class depends on its (nq, nk) and on the launch only through "grid <= 256" and "some sequence prefetches".
    `reachable_classes` enumerates, by those rules written out in Python, every class of every (nq, nk) in 1 .. 1024 under the four
    launch contexts (each of them exists at B <= 16 with 12 heads: a lone pair is at most 216 workgroups, 16 pairs are at least 384);
    the SWEEP runs real plans - decoder self and cross launches, B = 1, 2, 16, one entry running through every count against
    partners at the thresholds - and must reach exactly that set.
  * COVERAGE: every reachable class is the class of a sequence of the GPU matrix (tests/attention_varlen_cases.py).  Zero uncovered.
  * the workgroup map is a bijection onto (sequence, head, query block) and covers every query of every sequence exactly once,
  * equal sequences per side reduce to attn_mixed_plan field by field,
  * code-object pins of attn_varlen_kernel: no scratch, no spills, >= 2 waves per SIMD, fp16 MFMAs only.
"""
import ctypes as C
import os

import pytest

import attention_mixed_cases as AM
import attention_varlen_cases as AV

LDS_PER_CU = 160 * 1024
MIN_LDS = 2 * 2 * 64 * 128
HEADS = 12                          # the decoder's


@pytest.fixture(scope="module")
def lib():
    from vista_slam_amd import _lib
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libsta_mi355_test.so not built here (python -m vista_slam_amd.build)")
    return _lib.load_test()


_buf = (C.c_int * AV.plan_ints(AV.MAX_SEQ))()


def vplan(lib, heads, nq, nk, split=1, no_prefetch=0):
    S = len(nq)
    rc = lib.sta_debug_attn_varlen_plan(S, heads, (C.c_int * S)(*nq), (C.c_int * S)(*nk), split, no_prefetch, _buf)
    assert rc == 0, (heads, nq, nk, lib.sta_last_error())
    return AV.plan_dict(_buf)


def check_plan(p, heads, nq, nk, split, no_prefetch):
    key = (heads, nq, nk, split, no_prefetch)
    S = len(nq)
    assert p["S"] == S, key
    nwg = npose = orows = 0
    for i in range(S):
        a = p["s"][i]
        assert a["pose"] == (1 if nq[i] % 128 == 0 else 2), key                     # the sequence's own nq decides its pose mode
        nqe = nq[i] + (1 if a["pose"] == 2 else 0)
        assert a["qblocks"] == (nqe + 127) // 128, key
        assert a["pose_blocks"] == (heads if a["pose"] == 1 else 0), key
        assert a["ntiles"] == (nk[i] + 63) // 64 and a["nfull"] == nk[i] // 64, key    # its own nk decides its key loop
        assert a["pose_scratch"] == ((nk[i] + 1 + 63) // 64 * 64 + 8 + 256) * 4 <= MIN_LDS, key
        assert (a["blk0"], a["pose_blk0"], a["orow0"]) == (nwg, npose, orows), key
        nwg += a["qblocks"] * heads; npose += a["pose_blocks"]; orows += nq[i] + 1
    assert (p["nwg"], p["pose_blocks"], p["grid"], p["orows"]) == (nwg, npose, nwg + npose, orows), key
    any_pf = 0
    for i in range(S):
        a = p["s"][i]
        want = int(nk[i] <= 256 and p["grid"] <= 256 and not no_prefetch)
        assert a["prefetch"] == want, key
        any_pf |= want
        assert not want or a["ntiles"] <= 4, key
        if nk[i] % 64 == 0:
            assert a["tail_stage"] == -1, key
        elif want:
            assert a["tail_stage"] == a["ntiles"] - 1 == a["nfull"], key
        else:
            assert a["tail_stage"] == (a["ntiles"] - 1) & 1, key
    assert p["stages"] == (4 if any_pf else 2), key                     # ONE LDS size: the hungriest sequence's
    assert p["lds_bytes"] == p["stages"] * (4 if split else 2) * 64 * 128, key
    assert MIN_LDS <= p["lds_bytes"] <= LDS_PER_CU, key
    assert not split or p["lds_bytes"] >= 4 * 64 * 128, key          # the query blocks stage their output tile in LDS (f16x3 form)


def reachable_classes():
    """Every class of a sequence (nq, nk) in 1 .. 1024 under the four launch contexts, by the rules written out."""
    out = set()
    for nq in range(1, 1025):
        pose = 1 if nq % 128 == 0 else 2
        last = "full" if (nq + (pose == 2)) % 128 == 0 else "ragged"
        for nk in range(1, 1025):
            nfull, ntiles = nk // 64, (nk + 63) // 64
            kind = "0" if nfull == 0 else ("odd" if nfull & 1 else "even")
            # (stages, prefetch): grid > 256 or nobody prefetches | this sequence prefetches | another one does
            ctx = [(2, 0)] + ([(4, 1)] if nk <= 256 else [(4, 0)])
            for stages, pf in ctx:
                tail = "none" if nfull == ntiles else (f"pf{nfull}" if pf else f"s{nfull & 1}")
                out.add((stages, pose, pf, tail, kind, last))
    return out


PARTNERS = (1, 128, 255, 300)          # as nq: ragged, pose blocks, a full last block; as nk: prefetching or not
FILLERS = ((1, 1), (1024, 1024))


def decoder_launches():
    """(nq, nk) lists of decoder launches: entry 0 = (n, p) or (p, n), the other B - 1 entries one filler pair; self and cross."""
    for n in range(1, 1025):
        for p in PARTNERS:
            for n1, n2 in ((n, p), (p, n)):
                for B in (1, 2, 16):
                    for f1, f2 in (FILLERS if B > 1 else FILLERS[:1]):
                        side1, side2 = [n1] + [f1] * (B - 1), [n2] + [f2] * (B - 1)
                        yield side1 + side2, side1 + side2          # self attention of all sequences
                        yield side1 + side2, side2 + side1          # cross attention: every sequence reads the other side's entry


@pytest.fixture(scope="module")
def sweep(lib):
    reached, n = {}, 0
    for nq, nk in decoder_launches():
        p = vplan(lib, HEADS, nq, nk)
        check_plan(p, HEADS, nq, nk, 1, 0)
        if n % 97 == 0:
            check_plan(vplan(lib, HEADS, nq, nk, 0, 0), HEADS, nq, nk, 0, 0)
            check_plan(vplan(lib, HEADS, nq, nk, 1, 1), HEADS, nq, nk, 1, 1)
        for i in range(len(nq)):
            reached.setdefault(AV.seq_class(p, i, nq[i]), (nq, nk))
        n += 1
    assert n == 1024 * len(PARTNERS) * 2 * (1 + 2 * len(FILLERS)) * 2
    return reached


def test_the_sweep_reaches_every_class_a_decoder_call_can_reach(sweep):
    want = reachable_classes()
    assert len(want) == 45
    assert set(sweep) == want, (sorted(want - set(sweep)), sorted(set(sweep) - want))


def test_every_reachable_class_is_in_the_gpu_matrix(sweep):
    covered = AV.covered_classes()
    uncovered = {c: eg for c, eg in sweep.items() if c not in covered}
    assert not uncovered, f"{len(uncovered)} sequence classes of decoder launches have no GPU case (class: first nq, nk): {uncovered}"
    assert not reachable_classes() - covered


def test_case_table_claims_match_the_plan(lib):
    assert len(set(AV.IDS)) == len(AV.IDS)
    for cid, heads, opt5, seqs, classes in AV.CASES:
        assert 3 <= len(seqs) <= 8 and len(classes) == len(seqs), cid
        assert len(set(classes)) == len(classes), (cid, "every sequence of a launch is in a different class")
        nq, nk = [s[0] for s in seqs], [s[1] for s in seqs]
        assert max(nq + nk) <= 1024, cid
        for split in (0, 1):
            p = vplan(lib, heads, nq, nk, split, opt5)
            check_plan(p, heads, nq, nk, split, opt5)
            assert [AV.seq_class(p, i, nq[i]) for i in range(len(seqs))] == list(classes), (cid, p)
        for which in AV.SHIFTS:
            assert 0 <= AV.kv_shift((cid, heads, opt5, seqs), which) < len(seqs)


def test_required_launches_are_in_the_matrix(lib):
    cls = [c for case in AV.CASES for c in case[4]]
    assert {c[1] for c in cls} == {1, 2} and {c[2] for c in cls} == {0, 1}                       # both pose modes, both schedules
    assert {"none", "s0", "s1"} <= {c[3] for c in cls} and any(c[3].startswith("pf") for c in cls)
    grids = [vplan(lib, heads, [s[0] for s in seqs], [s[1] for s in seqs], 1, opt5) for _c, heads, opt5, seqs, _k in AV.CASES]
    big = [p for p in grids if p["grid"] > 256]
    assert big and all(p["stages"] == 2 for p in big)                       # a launch whose 2-stage LDS comes from its grid
    assert any(len({c[1] for c in case[4]}) == 2 for case in AV.CASES)      # both pose modes inside one launch
    assert any(len({c[2] for c in case[4]}) == 2 for case in AV.CASES)      # a double-buffered sequence next to a prefetching one


def block_map(lib, heads, nq, nk):
    S = len(nq)
    p = vplan(lib, heads, nq, nk)
    out = (C.c_int * (3 * p["nwg"]))()
    assert lib.sta_debug_attn_varlen_block_map(S, heads, (C.c_int * S)(*nq), (C.c_int * S)(*nk), out) == 0
    return p, [tuple(out[3 * b:3 * b + 3]) for b in range(p["nwg"])]


def test_block_map_is_a_bijection_and_covers_every_query(lib):
    """Every (sequence, head, query block) exactly once; with the blocks' 128 rows every query of every sequence (pose mode 2: and
    its pose row) is owned by exactly one workgroup; the pose blocks are one per head of every pose-mode-1 sequence."""
    shapes = [[1, 64, 129, 12, 65, 128, 63, 256], [196, 80, 140, 196], [768, 768, 672, 96], [128] * 6, [1, 1024, 255, 256, 257],
              [5], [384, 383, 385], list(range(1, 33)), [1024] * 32, [127, 128, 129] * 10]
    for heads in (1, 2, 12):
        for nq in shapes:
            p, m = block_map(lib, heads, nq, nq[::-1])
            want = {(s, h, q) for s in range(len(nq)) for h in range(heads) for q in range(p["s"][s]["qblocks"])}
            assert len(m) == len(want) and set(m) == want, (heads, nq)
            assert len(m) + sum(a["pose_blocks"] for a in p["s"]) == p["grid"]
            for s, n in enumerate(nq):
                nqe = n + (1 if p["s"][s]["pose"] == 2 else 0)
                rows = sorted(q * 128 + r for (ss, h, q) in m if ss == s and h == 0 for r in range(128) if q * 128 + r < nqe)
                assert rows == list(range(nqe)), (heads, nq, s)
            # the kernel's pose-block scan: block b belongs to the last sequence whose first pose block is <= b
            owners = [max(i for i in range(len(nq)) if p["s"][i]["pose_blk0"] <= b) for b in range(p["pose_blocks"])]
            assert owners == [s for s in range(len(nq)) for _ in range(p["s"][s]["pose_blocks"])], (heads, nq)
            assert all(p["s"][s]["pose"] == 1 for s in owners)


def test_equal_sequences_reduce_to_attn_mixed_plan(lib):
    """All sequences of a side equal: the launch fields and every sequence's fields are attn_mixed_plan's for its group."""
    out = (C.c_int * AM.PLAN_INTS)()
    for split in (0, 1):
        for no_prefetch in (0, 1):
            for heads in (2, 12):
                for B in (1, 2, 8, 16):
                    for n1, n2 in ((12, 15), (196, 140), (256, 196), (768, 196), (1, 1024), (128, 128), (255, 64), (65, 320), (384, 383)):
                        for cross in (0, 1):
                            nq = [n1] * B + [n2] * B
                            nk = nq[B:] + nq[:B] if cross else nq
                            assert lib.sta_debug_attn_mixed_plan(B, B, heads, nq[0], nk[0], nq[B], nk[B], split, no_prefetch, out) == 0
                            mp = AM.plan_dict(out)
                            p = vplan(lib, heads, nq, nk, split, no_prefetch)
                            key = (split, no_prefetch, heads, B, n1, n2, cross)
                            assert (p["stages"], p["lds_bytes"], p["grid"]) == (mp["stages"], mp["lds_bytes"], mp["grid"]), key
                            assert p["s"][B]["blk0"] == mp["nwg_a"], key
                            for g in (0, 1):
                                seqs = p["s"][g * B:(g + 1) * B]
                                assert sum(a["pose_blocks"] for a in seqs) == mp["g"][g]["pose_blocks"], key
                                for a in seqs:
                                    for f in ("pose", "prefetch", "qblocks", "ntiles", "nfull", "tail_stage", "pose_scratch"):
                                        assert a[f] == mp["g"][g][f], (f, g) + key
                                assert AV.seq_class(p, g * B, nq[g * B]) == AM.group_class(mp, g, nq[g * B]), key


def test_varlen_plan_rejects_bad_shapes(lib):
    one = (C.c_int * 1)(10)
    assert lib.sta_debug_attn_varlen_plan(0, 2, one, one, 1, 0, _buf) != 0
    assert lib.sta_debug_attn_varlen_plan(33, 2, (C.c_int * 33)(*[4] * 33), (C.c_int * 33)(*[4] * 33), 1, 0, _buf) != 0
    assert lib.sta_debug_attn_varlen_plan(2, 2, (C.c_int * 2)(10, 0), (C.c_int * 2)(10, 10), 1, 0, _buf) != 0
    assert lib.sta_debug_attn_varlen_plan(2, 2, (C.c_int * 2)(100, 100), (C.c_int * 2)(100, 8000), 1, 0, _buf) != 0      # pose-query scratch beyond the LDS allocation
    assert lib.sta_debug_attn_varlen_plan(1, 2, one, None, 1, 0, _buf) != 0


# ---------------------------------------------------------------------------------------------------------
# code-object pins of attn_varlen_kernel in the built PRODUCT library (as tests/test_attention_mixed_plan.py pins attn_mixed_kernel)
VARLEN_MIN_WAVES = {"_Z18attn_varlen_kernelILb1EEv16AttnVarlenParams": 2, "_Z18attn_varlen_kernelILb0EEv16AttnVarlenParams": 2}


def test_attn_varlen_kernel_code_object():
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
    for name, min_waves in VARLEN_MIN_WAVES.items():
        assert name in meta and name in mfma, name
        agpr, vgpr, scratch, vspill, sspill = meta[name]
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        regs = (agpr + vgpr + 7) // 8 * 8
        assert min(8, 512 // regs) >= min_waves, (name, vgpr, agpr)
        assert mfma[name] and all(re.fullmatch(r"v_mfma_f32_\d+x\d+x\d+_f16", op) for op in mfma[name]), (name, sorted(mfma[name]))
