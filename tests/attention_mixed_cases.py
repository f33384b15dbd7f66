"""The GPU case matrix of tests/test_attention_mixed_exact.py as plain data (no torch, no numpy), so that the host-only coverage test
(tests/test_attention_mixed_plan.py) can import it.

The two-group launch (csrc/attention.h: attn_mixed_kernel; sta_launch.inc: attn_mixed_plan) serves the decoder on view pairs of
different resolution: group a = S1 sequences of nq_a queries over nk_a keys, group b = S2 sequences of nq_b over nk_b, every one
in the pose-token form (pose key at token index nk, pose query at token index nq of its group).

A workgroup of the launch runs the code path of ITS group: the groups share nothing but the LDS size of the launch (workgroups do
not communicate).  So the unit of coverage is the GROUP CLASS

    (slot, LDS stages of the launch, pose mode, prefetch, tail kind, nfull kind, last query block)

slot 0 / 1 = group a / b (the kernel selects the group's numbers by comparing the logical block id with group a's block count);
the other coordinates as in tests/attention_cases.py.  A double-buffered group inside a 4-stage launch (the other group prefetches)
is a class of its own.

A case: (id, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, kv_shift, option 5, class of group a, class of group b) with the classes
WITHOUT the slot.  The first rows are the decoder's own launches at the sizes of the decn_* fixtures (self attention: nq == nk per
group, kv_shift 0; cross attention: (nq, nk) = (N1, N2) | (N2, N1), kv_shift = S1) and two grids above 256 workgroups; the rest was
chosen so that every group class the decoder can reach (every pair of patch grids up to 32 x 32, 1 to 16 pairs) occurs in its
slot: general (nq, nk) per group and any kv_shift - the kernel does not know about sides.  option 5 = 1 forbids the prefetch
schedule (runs a small shape the way a large batch of it runs).
"""

PLAN_FIELDS = ("stages", "lds_bytes", "grid", "nwg_a")
GROUP_FIELDS = ("pose", "prefetch", "pose_blocks", "qblocks", "ntiles", "nfull", "tail_stage", "pose_scratch")
PLAN_INTS = len(PLAN_FIELDS) + 2 * len(GROUP_FIELDS)


def plan_dict(out):
    """The 20 ints of sta_debug_attn_mixed_plan / sta_debug_last_attn_mixed_plan -> {"stages", .., "g": [group a, group b]}."""
    out = list(out)
    d = dict(zip(PLAN_FIELDS, out[:4]))
    d["g"] = [dict(zip(GROUP_FIELDS, out[4 + 8 * i:12 + 8 * i])) for i in range(2)]
    return d


def group_class(plan, g, nq):
    """Class of group g (0 / 1) of a plan_dict, without the slot."""
    a = plan["g"][g]
    if a["tail_stage"] < 0:
        tail = "none"
    else:
        tail = ("pf%d" if a["prefetch"] else "s%d") % a["tail_stage"]
    nfull = "0" if a["nfull"] == 0 else ("odd" if a["nfull"] & 1 else "even")
    nqe = nq + (1 if a["pose"] == 2 else 0)
    return (plan["stages"], a["pose"], a["prefetch"], tail, nfull, "full" if nqe % 128 == 0 else "ragged")


CASES = [
    ('tiny12_15_self', 2, 2, 2, 12, 12, 15, 15, 0, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('tiny12_15_cross', 2, 2, 2, 12, 15, 15, 12, 2, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('tiny12_4_cross', 1, 1, 2, 12, 4, 4, 12, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('tiny15_6_cross', 1, 1, 2, 15, 6, 6, 15, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('n196_140_self', 1, 1, 12, 196, 196, 140, 140, 0, 0, (4, 2, 1, 'pf3', 'odd', 'ragged'), (4, 2, 1, 'pf2', 'even', 'ragged')),
    ('n196_140_cross', 1, 1, 12, 196, 140, 140, 196, 1, 0, (4, 2, 1, 'pf2', 'even', 'ragged'), (4, 2, 1, 'pf3', 'odd', 'ragged')),
    ('n256_196_self', 1, 1, 12, 256, 256, 196, 196, 0, 0, (4, 1, 1, 'none', 'even', 'full'), (4, 2, 1, 'pf3', 'odd', 'ragged')),
    ('n256_196_cross', 1, 1, 12, 256, 196, 196, 256, 1, 0, (4, 1, 1, 'pf3', 'odd', 'full'), (4, 2, 1, 'none', 'even', 'ragged')),
    ('n768_196_self', 1, 1, 2, 768, 768, 196, 196, 0, 0, (4, 1, 0, 'none', 'even', 'full'), (4, 2, 1, 'pf3', 'odd', 'ragged')),
    ('n768_196_cross', 2, 2, 1, 768, 196, 196, 768, 2, 0, (4, 1, 1, 'pf3', 'odd', 'full'), (4, 2, 0, 'none', 'even', 'ragged')),
    ('n196_768_cross', 1, 1, 2, 196, 768, 768, 196, 1, 0, (4, 2, 0, 'none', 'even', 'ragged'), (4, 1, 1, 'pf3', 'odd', 'full')),
    ('n768_196_cross_grid272', 8, 8, 2, 768, 196, 196, 768, 8, 0, (4, 1, 1, 'pf3', 'odd', 'full'), (4, 2, 0, 'none', 'even', 'ragged')),
    ('n196_140_self_grid290', 8, 8, 12, 196, 196, 140, 140, 0, 0, (2, 2, 0, 's1', 'odd', 'ragged'), (2, 2, 0, 's0', 'even', 'ragged')),
    ('q1k64_q1k64', 1, 1, 2, 1, 64, 1, 64, 1, 0, (4, 2, 1, 'none', 'odd', 'ragged'), (4, 2, 1, 'none', 'odd', 'ragged')),
    ('q1k65_q1k65', 1, 1, 2, 1, 65, 1, 65, 0, 0, (4, 2, 1, 'pf1', 'odd', 'ragged'), (4, 2, 1, 'pf1', 'odd', 'ragged')),
    ('q1k128_q128k1', 1, 1, 2, 1, 128, 128, 1, 0, 0, (4, 2, 1, 'none', 'even', 'ragged'), (4, 1, 1, 'pf0', '0', 'full')),
    ('q128k1_q128k64', 1, 1, 2, 128, 1, 128, 64, 0, 0, (4, 1, 1, 'pf0', '0', 'full'), (4, 1, 1, 'none', 'odd', 'full')),
    ('q128k64_q128k65', 1, 1, 2, 128, 64, 128, 65, 1, 0, (4, 1, 1, 'none', 'odd', 'full'), (4, 1, 1, 'pf1', 'odd', 'full')),
    ('q128k65_q128k128', 1, 1, 2, 128, 65, 128, 128, 0, 0, (4, 1, 1, 'pf1', 'odd', 'full'), (4, 1, 1, 'none', 'even', 'full')),
    ('q128k130_q128k130', 1, 1, 2, 128, 130, 128, 130, 0, 0, (4, 1, 1, 'pf2', 'even', 'full'), (4, 1, 1, 'pf2', 'even', 'full')),
    ('q255k1_q255k1', 1, 1, 2, 255, 1, 255, 1, 0, 0, (4, 2, 1, 'pf0', '0', 'full'), (4, 2, 1, 'pf0', '0', 'full')),
    ('q255k64_q255k64', 1, 1, 2, 255, 64, 255, 64, 1, 0, (4, 2, 1, 'none', 'odd', 'full'), (4, 2, 1, 'none', 'odd', 'full')),
    ('q255k65_q255k65', 1, 1, 2, 255, 65, 255, 65, 0, 0, (4, 2, 1, 'pf1', 'odd', 'full'), (4, 2, 1, 'pf1', 'odd', 'full')),
    ('q255k128_q255k128', 1, 1, 2, 255, 128, 255, 128, 1, 0, (4, 2, 1, 'none', 'even', 'full'), (4, 2, 1, 'none', 'even', 'full')),
    ('q255k130_q255k130', 1, 1, 2, 255, 130, 255, 130, 1, 0, (4, 2, 1, 'pf2', 'even', 'full'), (4, 2, 1, 'pf2', 'even', 'full')),
    ('q255k195_q255k195', 1, 1, 2, 255, 195, 255, 195, 0, 0, (4, 2, 1, 'pf3', 'odd', 'full'), (4, 2, 1, 'pf3', 'odd', 'full')),
    ('q1k260_q128k260', 1, 1, 2, 1, 260, 128, 260, 1, 0, (2, 2, 0, 's0', 'even', 'ragged'), (2, 1, 0, 's0', 'even', 'full')),
    ('q128k260_q255k260', 1, 1, 2, 128, 260, 255, 260, 0, 0, (2, 1, 0, 's0', 'even', 'full'), (2, 2, 0, 's0', 'even', 'full')),
    ('q1k320_q1k320', 1, 1, 2, 1, 320, 1, 320, 1, 0, (2, 2, 0, 'none', 'odd', 'ragged'), (2, 2, 0, 'none', 'odd', 'ragged')),
    ('q128k320_q128k320', 1, 1, 2, 128, 320, 128, 320, 0, 0, (2, 1, 0, 'none', 'odd', 'full'), (2, 1, 0, 'none', 'odd', 'full')),
    ('q255k260_q255k320', 1, 1, 2, 255, 260, 255, 320, 1, 0, (2, 2, 0, 's0', 'even', 'full'), (2, 2, 0, 'none', 'odd', 'full')),
    ('q128k322_q1k322', 1, 1, 2, 128, 322, 1, 322, 0, 0, (2, 1, 0, 's1', 'odd', 'full'), (2, 2, 0, 's1', 'odd', 'ragged')),
    ('q255k320_q128k322', 1, 1, 2, 255, 320, 128, 322, 1, 0, (2, 2, 0, 'none', 'odd', 'full'), (2, 1, 0, 's1', 'odd', 'full')),
    ('q255k322_q255k322', 1, 1, 2, 255, 322, 255, 322, 1, 0, (2, 2, 0, 's1', 'odd', 'full'), (2, 2, 0, 's1', 'odd', 'full')),
    ('q1k384_q1k384', 1, 1, 2, 1, 384, 1, 384, 1, 0, (2, 2, 0, 'none', 'even', 'ragged'), (2, 2, 0, 'none', 'even', 'ragged')),
    ('q128k384_q128k384', 1, 1, 2, 128, 384, 128, 384, 0, 0, (2, 1, 0, 'none', 'even', 'full'), (2, 1, 0, 'none', 'even', 'full')),
    ('q255k384_q255k384', 1, 1, 2, 255, 384, 255, 384, 1, 0, (2, 2, 0, 'none', 'even', 'full'), (2, 2, 0, 'none', 'even', 'full')),
    ('q1k1_q1k1_opt5', 1, 1, 2, 1, 1, 1, 1, 0, 1, (2, 2, 0, 's0', '0', 'ragged'), (2, 2, 0, 's0', '0', 'ragged')),
    ('q128k1_q128k1_opt5', 1, 1, 2, 128, 1, 128, 1, 1, 1, (2, 1, 0, 's0', '0', 'full'), (2, 1, 0, 's0', '0', 'full')),
    ('q255k1_q255k1_opt5', 1, 1, 2, 255, 1, 255, 1, 0, 1, (2, 2, 0, 's0', '0', 'full'), (2, 2, 0, 's0', '0', 'full')),
    ('q1k1_q1k260', 1, 1, 2, 1, 1, 1, 260, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 0, 's0', 'even', 'ragged')),
    ('q1k1_q128k260', 1, 1, 2, 1, 1, 128, 260, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 1, 0, 's0', 'even', 'full')),
    ('q1k1_q255k260', 1, 1, 2, 1, 1, 255, 260, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 0, 's0', 'even', 'full')),
    ('q1k260_q1k1', 1, 1, 2, 1, 260, 1, 1, 0, 0, (4, 2, 0, 's0', 'even', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q128k260_q1k1', 1, 1, 2, 128, 260, 1, 1, 1, 0, (4, 1, 0, 's0', 'even', 'full'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q255k260_q1k1', 1, 1, 2, 255, 260, 1, 1, 0, 0, (4, 2, 0, 's0', 'even', 'full'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q1k1_q1k320', 1, 1, 2, 1, 1, 1, 320, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 0, 'none', 'odd', 'ragged')),
    ('q1k1_q128k320', 1, 1, 2, 1, 1, 128, 320, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 1, 0, 'none', 'odd', 'full')),
    ('q1k1_q255k320', 1, 1, 2, 1, 1, 255, 320, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 0, 'none', 'odd', 'full')),
    ('q1k320_q1k1', 1, 1, 2, 1, 320, 1, 1, 0, 0, (4, 2, 0, 'none', 'odd', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q128k320_q1k1', 1, 1, 2, 128, 320, 1, 1, 1, 0, (4, 1, 0, 'none', 'odd', 'full'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q255k320_q1k1', 1, 1, 2, 255, 320, 1, 1, 0, 0, (4, 2, 0, 'none', 'odd', 'full'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q1k1_q1k322', 1, 1, 2, 1, 1, 1, 322, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 0, 's1', 'odd', 'ragged')),
    ('q1k1_q128k322', 1, 1, 2, 1, 1, 128, 322, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 1, 0, 's1', 'odd', 'full')),
    ('q1k1_q255k322', 1, 1, 2, 1, 1, 255, 322, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 0, 's1', 'odd', 'full')),
    ('q1k322_q1k1', 1, 1, 2, 1, 322, 1, 1, 0, 0, (4, 2, 0, 's1', 'odd', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q128k322_q1k1', 1, 1, 2, 128, 322, 1, 1, 1, 0, (4, 1, 0, 's1', 'odd', 'full'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q255k322_q1k1', 1, 1, 2, 255, 322, 1, 1, 0, 0, (4, 2, 0, 's1', 'odd', 'full'), (4, 2, 1, 'pf0', '0', 'ragged')),
    ('q1k1_q128k384', 1, 1, 2, 1, 1, 128, 384, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 1, 0, 'none', 'even', 'full')),
    ('q1k1_q255k384', 1, 1, 2, 1, 1, 255, 384, 1, 0, (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 0, 'none', 'even', 'full')),
    ('q255k384_q1k1', 1, 1, 2, 255, 384, 1, 1, 0, 0, (4, 2, 0, 'none', 'even', 'full'), (4, 2, 1, 'pf0', '0', 'ragged')),
]

PRECISIONS = ("f16x3", "f16")
IDS = [c[0] for c in CASES]


def covered_classes():
    """{(slot, *class)} of the table."""
    return {(0,) + c[10] for c in CASES} | {(1,) + c[11] for c in CASES}


# the running-maximum test (rise / fall / peak ramps): long and short loops, both schedules, both pose modes, different tile counts per group
RAMP_CASES = ("n196_140_cross", "n256_196_cross", "n768_196_self", "n768_196_cross", "n196_768_cross", "n768_196_cross_grid272")
RAMP_PATTERNS = ("rise", "fall", "peak")
SHARPS = (1.0, 3.0, 6.0)


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def sharp_of(cid):
    return SHARPS[IDS.index(cid) % len(SHARPS)]
