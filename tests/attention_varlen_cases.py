"""The GPU case matrix of tests/test_attention_varlen_exact.py as plain data (no torch, no numpy), so that the host-only coverage test
(tests/test_attention_varlen_plan.py) can import it.

The per-sequence launch (csrc/attention.h: attn_varlen_kernel; sta_launch.inc: attn_varlen_plan) serves sta_decode_varlen: S <= 32
sequences, sequence s with its own nq queries over its own nk keys, every one in the pose-token form (pose key at token index nk of
the key sequence, pose query at token index nq).  A workgroup finds its sequence by a scan of the launch's table and then runs the
code path of THAT sequence; sequences share nothing but the LDS size of the launch.  So the unit of coverage is the SEQUENCE CLASS

    (LDS stages of the launch, pose mode, prefetch, tail kind, nfull kind, last query block)

- tests/attention_mixed_cases.py's group class without the slot (a sequence's place in the table is not a code path: the scan is the
same loop for every place).  A double-buffered sequence inside a 4-stage launch (another sequence prefetches) is a class of its own.

A launch: (id, heads, option 5, [(nq, nk) per sequence], [class per sequence]).  EVERY sequence of a launch is in a different class,
so a kernel that takes a sequence's nk, tail stage, pose mode or output row from its neighbour runs the wrong code path on it.  Each
launch runs under kv_shift = 0 and kv_shift = S // 2.  option 5 = 1 forbids the prefetch schedule (runs small shapes the way a launch
of more than 256 workgroups runs them); `db_grid276` is such a launch for real (the 2-stage LDS because of its grid).
"""

LAUNCH_FIELDS = ("S", "stages", "lds_bytes", "grid", "nwg", "pose_blocks", "orows")
SEQ_FIELDS = ("pose", "prefetch", "pose_blocks", "qblocks", "ntiles", "nfull", "tail_stage", "pose_scratch", "blk0", "pose_blk0", "orow0")
MAX_SEQ = 32
GUARD_ROWS = 64             # sta_debug_attn_varlen returns this many rows of a guard block behind the output planes, every byte 0x3C


def plan_ints(S):
    return len(LAUNCH_FIELDS) + len(SEQ_FIELDS) * S


def plan_dict(out):
    """The ints of sta_debug_attn_varlen_plan / sta_debug_last_attn_varlen_plan -> {"S", "stages", .., "s": [per sequence]}."""
    out = list(out)
    d = dict(zip(LAUNCH_FIELDS, out[:7]))
    d["s"] = [dict(zip(SEQ_FIELDS, out[7 + 11 * i:18 + 11 * i])) for i in range(d["S"])]
    return d


def seq_class(plan, i, nq):
    """Class of sequence i of a plan_dict."""
    a = plan["s"][i]
    if a["tail_stage"] < 0:
        tail = "none"
    else:
        tail = ("pf%d" if a["prefetch"] else "s%d") % a["tail_stage"]
    nfull = "0" if a["nfull"] == 0 else ("odd" if a["nfull"] & 1 else "even")
    nqe = nq + (1 if a["pose"] == 2 else 0)
    return (plan["stages"], a["pose"], a["prefetch"], tail, nfull, "full" if nqe % 128 == 0 else "ragged")


CASES = [
    ('pf_q128', 2, 0, [(128, 64), (128, 128), (128, 1), (128, 65), (128, 130), (128, 195)],
     [(4, 1, 1, 'none', 'odd', 'full'), (4, 1, 1, 'none', 'even', 'full'), (4, 1, 1, 'pf0', '0', 'full'), (4, 1, 1, 'pf1', 'odd', 'full'), (4, 1, 1, 'pf2', 'even', 'full'), (4, 1, 1, 'pf3', 'odd', 'full')]),
    ('pf_q255', 2, 0, [(255, 64), (255, 128), (255, 1), (255, 65), (255, 130), (255, 195)],
     [(4, 2, 1, 'none', 'odd', 'full'), (4, 2, 1, 'none', 'even', 'full'), (4, 2, 1, 'pf0', '0', 'full'), (4, 2, 1, 'pf1', 'odd', 'full'), (4, 2, 1, 'pf2', 'even', 'full'), (4, 2, 1, 'pf3', 'odd', 'full')]),
    ('pf_ragged', 2, 0, [(1, 64), (12, 128), (5, 1), (63, 65), (129, 130), (200, 195)],
     [(4, 2, 1, 'none', 'odd', 'ragged'), (4, 2, 1, 'none', 'even', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged'), (4, 2, 1, 'pf1', 'odd', 'ragged'), (4, 2, 1, 'pf2', 'even', 'ragged'), (4, 2, 1, 'pf3', 'odd', 'ragged')]),
    ('db_in_pf_full', 2, 0, [(128, 320), (128, 384), (128, 260), (128, 322), (255, 320), (255, 384), (255, 260), (1, 1)],
     [(4, 1, 0, 'none', 'odd', 'full'), (4, 1, 0, 'none', 'even', 'full'), (4, 1, 0, 's0', 'even', 'full'), (4, 1, 0, 's1', 'odd', 'full'), (4, 2, 0, 'none', 'odd', 'full'), (4, 2, 0, 'none', 'even', 'full'), (4, 2, 0, 's0', 'even', 'full'), (4, 2, 1, 'pf0', '0', 'ragged')]),
    ('db_in_pf_ragged', 2, 0, [(255, 322), (1, 320), (12, 384), (5, 260), (63, 322), (128, 1)],
     [(4, 2, 0, 's1', 'odd', 'full'), (4, 2, 0, 'none', 'odd', 'ragged'), (4, 2, 0, 'none', 'even', 'ragged'), (4, 2, 0, 's0', 'even', 'ragged'), (4, 2, 0, 's1', 'odd', 'ragged'), (4, 1, 1, 'pf0', '0', 'full')]),
    ('db_opt5_a', 2, 1, [(128, 64), (128, 128), (128, 1), (128, 65), (128, 130), (255, 64), (255, 128), (255, 1)],
     [(2, 1, 0, 'none', 'odd', 'full'), (2, 1, 0, 'none', 'even', 'full'), (2, 1, 0, 's0', '0', 'full'), (2, 1, 0, 's1', 'odd', 'full'), (2, 1, 0, 's0', 'even', 'full'), (2, 2, 0, 'none', 'odd', 'full'), (2, 2, 0, 'none', 'even', 'full'), (2, 2, 0, 's0', '0', 'full')]),
    ('db_opt5_b', 2, 1, [(255, 65), (255, 130), (1, 64), (12, 128), (5, 1), (63, 65), (129, 130)],
     [(2, 2, 0, 's1', 'odd', 'full'), (2, 2, 0, 's0', 'even', 'full'), (2, 2, 0, 'none', 'odd', 'ragged'), (2, 2, 0, 'none', 'even', 'ragged'), (2, 2, 0, 's0', '0', 'ragged'), (2, 2, 0, 's1', 'odd', 'ragged'), (2, 2, 0, 's0', 'even', 'ragged')]),
    ('db_grid276', 12, 0, [(384, 64), (384, 128), (384, 1), (384, 65), (384, 130), (383, 322)],
     [(2, 1, 0, 'none', 'odd', 'full'), (2, 1, 0, 'none', 'even', 'full'), (2, 1, 0, 's0', '0', 'full'), (2, 1, 0, 's1', 'odd', 'full'), (2, 1, 0, 's0', 'even', 'full'), (2, 2, 0, 's1', 'odd', 'full')]),
    ('three', 2, 0, [(196, 140), (140, 196), (80, 80)],
     [(4, 2, 1, 'pf2', 'even', 'ragged'), (4, 2, 1, 'pf3', 'odd', 'ragged'), (4, 2, 1, 'pf1', 'odd', 'ragged')]),
    # the two classes that the launches above hold only with ONE query, which the selection test sends to the pose key: here with
    # enough queries to select every forced key (2 of 64 keys, 10 of 320) and the pose key besides
    ('ragged_small', 2, 0, [(9, 64), (17, 320), (3, 1)],
     [(4, 2, 1, 'none', 'odd', 'ragged'), (4, 2, 0, 'none', 'odd', 'ragged'), (4, 2, 1, 'pf0', '0', 'ragged')]),
]

PRECISIONS = ("f16x3", "f16")
IDS = [c[0] for c in CASES]
SHIFTS = ("shift0", "shift_half")


def kv_shift(case, which):
    return 0 if which == "shift0" else len(case[3]) // 2


def covered_classes():
    return {cls for c in CASES for cls in c[4]}


# the running-maximum test (rise / fall / peak ramps): long and short loops, both schedules, both pose modes, the large grid
RAMP_CASES = ("pf_ragged", "db_in_pf_full", "db_in_pf_ragged", "db_grid276")
RAMP_PATTERNS = ("rise", "fall", "peak")
SHARPS = (1.0, 3.0, 6.0)


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def sharp_of(cid):
    return SHARPS[IDS.index(cid) % len(SHARPS)]
