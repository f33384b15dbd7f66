"""CPU: the launch plan of the attention kernel and its workgroup remap, host only.

run_attn runs exactly the plan of attn_plan (sta_launch.inc; exported by the test-hooks build as sta_debug_attn_plan), and
attn_kernel maps its workgroups through attn_block_map (attention.h; sta_debug_attn_block_map runs the same inline function on
the host) - so this needs the built test library but no GPU.

  * the block map is a permutation of [0, nwg) for every grid size from 1 to 4096 (grids that are no multiple of 8 included),
  * every plan is consistent with the kernel's own arithmetic (grid, pose mode, tiles, LDS, tail stage),
  * COVERAGE: every schedule class (tests/attention_cases.py) that a product launch can reach - H and W multiples of 16 up to 512,
    1 to 16 pairs, encoder / decoder self / decoder cross attention, both precisions - is the class of at least one case of the
    GPU matrix of tests/test_attention_exact.py.  No allow-list: zero uncovered classes.
"""
import ctypes as C
import os

import pytest

import attention_cases as AC

LDS_PER_CU = 160 * 1024
MIN_LDS = 2 * 2 * 64 * 128          # attn_smem_bytes<false>(): the smallest allocation a launch gets (f16, two stages)


@pytest.fixture(scope="module")
def lib():
    from vista_slam_amd import _lib
    if not os.path.exists(_lib.TEST_LIB_PATH):
        pytest.skip("libsta_mi355_test.so not built here (python -m vista_slam_amd.build)")
    return _lib.load_test()


def plan(lib, S, heads, nq, nk, pose, split, no_prefetch=0):
    out = (C.c_int * len(AC.FIELDS))()
    rc = lib.sta_debug_attn_plan(S, heads, nq, nk, pose, split, no_prefetch, out)
    assert rc == 0, (S, heads, nq, nk, pose, split, no_prefetch, lib.sta_last_error())
    return dict(zip(AC.FIELDS, out))


def test_block_map_is_a_permutation(lib):
    buf = (C.c_int * 4096)()
    for nwg in range(1, 4097):
        assert lib.sta_debug_attn_block_map(nwg, buf) == 0
        got = sorted(buf[:nwg])
        assert got == list(range(nwg)), f"nwg={nwg}: not a permutation (first ids {buf[:min(nwg, 16)]})"


def test_block_map_keeps_an_xcd_contiguous(lib):
    """Workgroup b runs on XCD b % 8: the ids of one XCD are one contiguous ascending range (what the remap is for)."""
    buf = (C.c_int * 300)()
    for nwg in (1, 7, 8, 9, 63, 144, 260, 288):
        assert lib.sta_debug_attn_block_map(nwg, buf) == 0
        for x in range(min(8, nwg)):
            ids = [buf[b] for b in range(x, nwg, 8)]
            assert ids == list(range(ids[0], ids[0] + len(ids))), (nwg, x, ids)


SWEEP_N = sorted(set(range(1, 70)) | {n + d for n in (128, 192, 256, 320, 384, 512, 576, 640, 768, 1024) for d in (-2, -1, 0, 1, 2)} |
                 {196, 375, 588, 1025})


def check_plan(p, S, heads, nq, nk, pose, split, no_prefetch):
    key = (S, heads, nq, nk, pose, split, no_prefetch, p)
    nqe = nq + (1 if p["pose"] == 2 else 0)
    assert p["pose"] == (0 if not pose else (1 if nq % 128 == 0 else 2)), key
    assert p["qblocks"] == (nqe + 127) // 128, key
    assert p["pose_blocks"] == (S * heads if p["pose"] == 1 else 0), key
    assert p["grid"] == p["qblocks"] * heads * S + p["pose_blocks"], key
    assert p["ntiles"] == (nk + 63) // 64 and p["nfull"] == nk // 64, key
    want_prefetch = int(nk <= 256 and p["grid"] <= 256 and not no_prefetch)
    assert p["prefetch"] == want_prefetch, key
    assert p["stages"] == (4 if want_prefetch else 2), key
    assert want_prefetch == 0 or p["ntiles"] <= p["stages"], key           # every tile of the prefetch schedule has its own stage
    assert p["lds_bytes"] == p["stages"] * (4 if split else 2) * 64 * 128, key
    assert MIN_LDS <= p["lds_bytes"] <= LDS_PER_CU, key
    # the query blocks stage their output tile in LDS: 4 waves x 64 rows x 128 B (f16x3 form)
    assert not split or p["lds_bytes"] >= 4 * 64 * 128, key
    if pose:
        npad = (nq + 1 + 63) // 64 * 64
        assert p["pose_scratch"] == (npad + 8 + 256) * 4 and p["pose_scratch"] <= MIN_LDS, key
    else:
        assert p["pose_scratch"] == 0, key
    if nk % 64 == 0:
        assert p["tail_stage"] == -1, key
    elif want_prefetch:
        assert p["tail_stage"] == p["ntiles"] - 1 == p["nfull"], key
    else:
        assert p["tail_stage"] == (p["ntiles"] - 1) & 1, key


def test_plans_are_consistent(lib):
    n = 0
    for split in (0, 1):
        for no_prefetch in (0, 1):
            for S, heads in ((1, 1), (2, 2), (2, 12), (2, 16), (9, 16), (10, 13), (10, 12), (11, 12), (32, 16), (32, 12)):
                for nk in SWEEP_N:
                    for pose in (0, 1):
                        for nq in ((nk,) if pose else (nk, 1, 130, 256)):
                            check_plan(plan(lib, S, heads, nq, nk, pose, split, no_prefetch), S, heads, nq, nk, pose, split, no_prefetch)
                            n += 1
    assert n > 10000


def test_plan_rejects_what_run_attn_rejects(lib):
    out = (C.c_int * len(AC.FIELDS))()
    assert lib.sta_debug_attn_plan(2, 2, 100, 101, 1, 1, 0, out) != 0          # pose form needs nq == nk
    assert lib.sta_debug_attn_plan(1, 1, 8000, 8000, 1, 1, 0, out) != 0        # pose-query scratch beyond the LDS allocation
    assert lib.sta_debug_attn_plan(0, 2, 100, 100, 0, 1, 0, out) != 0


def product_launches():
    """(S, heads, n, pose) of every attention launch of the product: n = (H / 16) x (W / 16) patch tokens, 2B sequences."""
    tokens = sorted({hp * wp for hp in range(1, 33) for wp in range(1, 33)})
    for n in tokens:
        for B in range(1, 17):
            yield 2 * B, 16, n, 0          # encoder self attention
            yield 2 * B, 12, n, 1          # decoder self and cross attention (same plan: kv_shift is no input of it)


def test_case_table_claims_match_the_plan(lib):
    ids = [c[0] for c in AC.CASES]
    assert len(set(ids)) == len(ids)
    for cid, form, S, heads, nq, nk, kv_shift, opt5, cls in AC.CASES:
        assert form in ("plain", "pose") and 0 <= kv_shift < S and max(nq, nk) <= 1025, cid
        assert form == "plain" or nq == nk, cid
        for split in (0, 1):
            p = plan(lib, S, heads, nq, nk, int(form == "pose"), split, opt5)
            assert AC.schedule_class(p, nq) == cls, (cid, p)


def test_every_product_schedule_class_is_in_the_gpu_matrix(lib):
    covered = AC.covered_classes()
    reached = {}
    for S, heads, n, pose in product_launches():
        for split in (0, 1):
            cls = (split,) + AC.schedule_class(plan(lib, S, heads, n, n, pose, split), n)
            reached.setdefault(cls, (S, heads, n, pose))
    assert len(reached) >= 40                       # the enumeration itself is alive (24 classes per precision today)
    uncovered = {c: eg for c, eg in reached.items() if c not in covered}
    assert not uncovered, f"{len(uncovered)} schedule classes of product launches have no GPU case (class: first S, heads, n, pose): {uncovered}"


def test_required_cases_are_in_the_matrix():
    """The shapes the matrix must hold whatever else changes."""
    have = {(form, S, heads, nq, nk, opt5) for _, form, S, heads, nq, nk, _, opt5, _ in AC.CASES}
    keys = {(form, nk) for form, _, _, _, nk, _ in have}
    for nk in (588, 375, 1, 63, 64, 65, 1024):
        assert ("plain", nk) in keys, nk
    for n in (196, 588, 640, 768):
        assert ("pose", n) in keys, n
    assert ("plain", 9, 16, 196, 196, 0) in have                       # 196 keys on a grid above 256 workgroups
    assert any(f == "plain" and nq == nk == 196 and o == 1 for f, _, _, nq, nk, o in have)      # ... and under option 5
    assert any(f == "plain" and nq != nk for f, _, _, nq, nk, _ in have)
    assert any(c[6] != 0 and c[2] >= 3 for c in AC.CASES)


# ---------------------------------------------------------------------------------------------------------
# the inputs and bounds of tests/test_attention_exact.py, on the CPU
def test_selection_inputs_select_exactly():
    """The selection construction on the CPU: margin above 160 log2 units, and both the float64 reference and the numpy model of
    the kernel's arithmetic return exactly the selected V rows (1025 keys, and a pose form with kv_shift)."""
    import numpy as np
    import helpers as H
    for form, S, heads, nq, nk, shift, sel in (("plain", 1, 2, 130, 1025, 0, "self"), ("pose", 3, 1, 196, 196, 1, "patch"),
                                               ("pose", 2, 1, 128, 128, 0, "self")):
        q, k, v, pi, margin = H.attn_selection_inputs(form, S, heads, nq, nk, sel, seed=21)
        assert margin > 160, margin
        nkt = k.shape[2]
        if nq == nk and form == "plain":
            assert all(sorted(pi[s, h].tolist()) == list(range(nk)) for s in range(S) for h in range(heads))
        elif form == "plain":
            forced = {0, nk - 1} | {t * 64 for t in range((nk + 63) // 64)} | {min(t * 64 + 63, nk - 1) for t in range((nk + 63) // 64)}
            assert all(forced <= set(pi[s, h].tolist()) for s in range(S) for h in range(heads))
        if form == "pose":
            assert ((pi[:, :, :nq] == nk).sum(-1) >= 1).all()                       # patch queries select the pose key
            assert ((pi[:, :, nq] == nk) if sel == "self" else (pi[:, :, nq] < nk)).all()
        assert pi.max() < nkt
        idx = [(s - shift) % S for s in range(S)]
        want = np.take_along_axis(v, pi[..., None], 2)
        assert np.abs(H.attn_ref64(q, k[idx], v[idx], shift) - want).max() < 1e-60        # (exp(-208) is not yet 0 in float64)
        for prec in AC.PRECISIONS:
            assert (H.attn_model(q, k[idx], v[idx], shift, prec) == want).all(), prec


def test_row_bounds_come_from_the_model():
    """The figures in the table of test_attention_exact.py are the numpy model's worst row on the named case (within a factor of 2:
    the model's own fp32 summation order depends on the BLAS underneath)."""
    import helpers as H
    import test_attention_exact as TE
    for (group, prec), (figure, cid) in TE.MODEL.items():
        _, form, S, heads, nq, nk, shift = AC.case_by_id(cid)[:7]
        if isinstance(group, str):
            assert cid in AC.RAMP_CASES
            q, k, v = H.attn_ramp_inputs(form, S, heads, nq, nk, group, seed=101)
        else:
            assert AC.sharp_of(cid) == group
            q, k, v = H.attn_gaussian_inputs(form, S, heads, nq, nk, group, seed=100)
        rows, _ = H.attn_row_errors(H.attn_model(q, k, v, shift, prec), H.attn_ref64(q, k, v, shift))
        assert 0.5 * figure < rows.max() < 2.0 * figure, (group, prec, cid, rows.max(), figure)
        assert TE.row_bound(group, prec) == 4.0 * figure


# ---------------------------------------------------------------------------------------------------------
# code-object pins of attn_kernel in the built PRODUCT library
# waves per SIMD implied by the unified register file (512 registers, allocated in blocks of 8): the parent commit's build has
# attn_kernel<true> at 214 VGPR + 0 AGPR and attn_kernel<false> at 189 + 0, i.e. 2 waves per SIMD each (launch bounds: 256, 2)
ATTN_MIN_WAVES = {"_Z11attn_kernelILb1EEv10AttnParams": 2, "_Z11attn_kernelILb0EEv10AttnParams": 2}


def test_attn_kernel_code_object():
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
    for name, min_waves in ATTN_MIN_WAVES.items():
        assert name in meta and name in mfma, name
        agpr, vgpr, scratch, vspill, sspill = meta[name]
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        regs = (agpr + vgpr + 7) // 8 * 8
        assert min(8, 512 // regs) >= min_waves, (name, vgpr, agpr)
        # fp16 MFMAs only (the shape is free to change: 32x32x16 today)
        assert mfma[name] and all(re.fullmatch(r"v_mfma_f32_\d+x\d+x\d+_f16", op) for op in mfma[name]), (name, sorted(mfma[name]))
