"""The GPU case matrix of tests/test_attention_exact.py as plain data (no torch, no numpy), so that the host-only coverage test
(tests/test_attention_plan.py) can import it.

A SCHEDULE CLASS names the code path of attn_kernel (csrc/attention.h) that a launch runs:

    (pose mode, prefetch, tail kind, nfull kind, last query block)

    pose mode   0 no pose token / 1 pose query on side workgroups (nq % 128 == 0) / 2 pose query in the last block's spare row
    prefetch    1: 4 LDS stages, every key tile requested up front / 0: the double-buffered loop
    tail kind   "none" (nk % 64 == 0), "s0" / "s1" (double-buffered: the LDS stage whose separately instantiated TAIL body runs),
                "pf0" .. "pf3" (prefetch: index of the partly valid tile)
    nfull kind  whole key tiles: "0", "odd", "even" (the peeled loop of the double-buffered schedule differs in all three)
    last block  "full" / "ragged": whether the last query block (pose mode 2: with its pose row) has dead rows

The precision (f16x3: attn_kernel<true>, f16: attn_kernel<false>) is the sixth coordinate; every case runs in both.

A case: (id, form, S, heads, nq, nk, kv_shift, option 5, class).  form "plain": sta_debug_attention; "pose": the decoder form
sta_debug_attention_pose with n = nq = nk patch tokens and the pose token last.  option 5 = 1 forbids the prefetch schedule
(sta_debug_set_option), i.e. runs a small shape the way a large batch of it runs.  The class is what the case CLAIMS: the GPU tests
assert it against the plan of the launch (sta_debug_last_attn_plan), the coverage test against sta_debug_attn_plan.
"""

FIELDS = ("pose", "prefetch", "stages", "lds_bytes", "grid", "pose_blocks", "qblocks", "ntiles", "nfull", "tail_stage", "pose_scratch")


def schedule_class(plan, nq):
    """plan: dict of FIELDS (sta_debug_attn_plan / sta_debug_last_attn_plan) -> the class tuple."""
    if plan["tail_stage"] < 0:
        tail = "none"
    else:
        tail = ("pf%d" if plan["prefetch"] else "s%d") % plan["tail_stage"]
    nfull = "0" if plan["nfull"] == 0 else ("odd" if plan["nfull"] & 1 else "even")
    nqe = nq + (1 if plan["pose"] == 2 else 0)
    return (plan["pose"], plan["prefetch"], tail, nfull, "full" if nqe % 128 == 0 else "ragged")


CASES = [
    # ---- no pose token (encoder; cross attention of a model without pose token has nq != nk)
    # double-buffered loop, tail tile in LDS stage 1: 448x336 = 588 tokens (10 tiles, tail at index 9), 375 keys (tail at 5),
    # 196 keys on a grid above 256 workgroups (224x224 at 5 or more pairs; tail at 3) and the same small shape under option 5
    ("n588", "plain", 2, 2, 588, 588, 0, 0, (0, 0, "s1", "odd", "ragged")),
    ("n588_shift", "plain", 3, 1, 588, 588, 1, 0, (0, 0, "s1", "odd", "ragged")),
    ("q100_k375", "plain", 2, 2, 100, 375, 0, 0, (0, 0, "s1", "odd", "ragged")),
    ("q128_k375", "plain", 1, 2, 128, 375, 0, 0, (0, 0, "s1", "odd", "full")),
    ("n196_grid288", "plain", 9, 16, 196, 196, 0, 0, (0, 0, "s1", "odd", "ragged")),
    ("n196_opt5", "plain", 3, 2, 196, 196, 2, 1, (0, 0, "s1", "odd", "ragged")),
    ("n65_opt5", "plain", 2, 2, 65, 65, 0, 1, (0, 0, "s1", "odd", "ragged")),
    # double-buffered, tail in stage 0: no whole tile at all (grid of 272 workgroups; option 5), an even count of whole tiles
    ("n63_grid272", "plain", 17, 16, 63, 63, 0, 0, (0, 0, "s0", "0", "ragged")),
    ("n1_opt5", "plain", 2, 2, 1, 1, 0, 1, (0, 0, "s0", "0", "ragged")),
    ("q130_k1025", "plain", 1, 2, 130, 1025, 0, 0, (0, 0, "s0", "even", "ragged")),
    ("n130_opt5", "plain", 2, 2, 130, 130, 1, 1, (0, 0, "s0", "even", "ragged")),
    # double-buffered, no tail: even / odd whole tiles
    ("n1024", "plain", 1, 1, 1024, 1024, 0, 0, (0, 0, "none", "even", "full")),
    ("n128_opt5", "plain", 2, 2, 128, 128, 0, 1, (0, 0, "none", "even", "full")),
    ("n320", "plain", 1, 2, 320, 320, 0, 0, (0, 0, "none", "odd", "ragged")),
    ("n64_opt5", "plain", 2, 2, 64, 64, 0, 1, (0, 0, "none", "odd", "ragged")),
    # prefetch schedule: 1 .. 4 tiles, tail at every index, no tail
    ("n1", "plain", 2, 2, 1, 1, 0, 0, (0, 1, "pf0", "0", "ragged")),
    ("n63", "plain", 2, 2, 63, 63, 0, 0, (0, 1, "pf0", "0", "ragged")),
    ("n65", "plain", 3, 2, 65, 65, 1, 0, (0, 1, "pf1", "odd", "ragged")),
    ("q300_k100", "plain", 2, 2, 300, 100, 0, 0, (0, 1, "pf1", "odd", "ragged")),
    ("q70_k130", "plain", 2, 2, 70, 130, 0, 0, (0, 1, "pf2", "even", "ragged")),
    ("n130", "plain", 2, 2, 130, 130, 0, 0, (0, 1, "pf2", "even", "ragged")),
    ("n196", "plain", 2, 2, 196, 196, 0, 0, (0, 1, "pf3", "odd", "ragged")),
    ("n64", "plain", 2, 2, 64, 64, 0, 0, (0, 1, "none", "odd", "ragged")),
    ("n192", "plain", 2, 1, 192, 192, 0, 0, (0, 1, "none", "odd", "ragged")),
    ("n128", "plain", 2, 2, 128, 128, 0, 0, (0, 1, "none", "even", "full")),
    ("n256", "plain", 3, 1, 256, 256, 2, 0, (0, 1, "none", "even", "full")),
    # ---- decoder forms (pose token last)
    # pose query on side workgroups (n % 128 == 0)
    ("pose640", "pose", 2, 2, 640, 640, 0, 0, (1, 0, "none", "even", "full")),
    ("pose768", "pose", 3, 1, 768, 768, 1, 0, (1, 0, "none", "even", "full")),
    ("pose128_opt5", "pose", 2, 2, 128, 128, 0, 1, (1, 0, "none", "even", "full")),
    ("pose128", "pose", 2, 2, 128, 128, 0, 0, (1, 1, "none", "even", "full")),
    ("pose256", "pose", 3, 2, 256, 256, 2, 0, (1, 1, "none", "even", "full")),
    # pose query in the last block's spare row, double-buffered
    ("pose588", "pose", 2, 2, 588, 588, 0, 0, (2, 0, "s1", "odd", "ragged")),
    ("pose588_shift", "pose", 3, 1, 588, 588, 2, 0, (2, 0, "s1", "odd", "ragged")),
    ("pose196_opt5", "pose", 2, 2, 196, 196, 1, 1, (2, 0, "s1", "odd", "ragged")),
    ("pose196_grid260", "pose", 10, 13, 196, 196, 5, 0, (2, 0, "s1", "odd", "ragged")),
    ("pose383", "pose", 1, 2, 383, 383, 0, 0, (2, 0, "s1", "odd", "full")),
    ("pose255_opt5", "pose", 2, 1, 255, 255, 0, 1, (2, 0, "s1", "odd", "full")),
    ("pose520", "pose", 1, 2, 520, 520, 0, 0, (2, 0, "s0", "even", "ragged")),
    ("pose130_opt5", "pose", 2, 2, 130, 130, 0, 1, (2, 0, "s0", "even", "ragged")),
    ("pose12_opt5", "pose", 2, 2, 12, 12, 0, 1, (2, 0, "s0", "0", "ragged")),
    ("pose320", "pose", 1, 2, 320, 320, 0, 0, (2, 0, "none", "odd", "ragged")),
    ("pose64_opt5", "pose", 2, 2, 64, 64, 0, 1, (2, 0, "none", "odd", "ragged")),
    # pose query in the spare row, prefetch schedule
    ("pose196", "pose", 2, 2, 196, 196, 0, 0, (2, 1, "pf3", "odd", "ragged")),
    ("pose196_shift", "pose", 4, 2, 196, 196, 2, 0, (2, 1, "pf3", "odd", "ragged")),
    ("pose255", "pose", 1, 1, 255, 255, 0, 0, (2, 1, "pf3", "odd", "full")),
    ("pose129", "pose", 3, 1, 129, 129, 2, 0, (2, 1, "pf2", "even", "ragged")),
    ("pose100", "pose", 2, 2, 100, 100, 0, 0, (2, 1, "pf1", "odd", "ragged")),
    ("pose12", "pose", 2, 2, 12, 12, 0, 0, (2, 1, "pf0", "0", "ragged")),
    ("pose64", "pose", 2, 2, 64, 64, 0, 0, (2, 1, "none", "odd", "ragged")),
    ("pose192", "pose", 2, 1, 192, 192, 0, 0, (2, 1, "none", "odd", "ragged")),
]

PRECISIONS = ("f16x3", "f16")


def covered_classes():
    """{(split, *class)}: every case runs in both precisions."""
    return {(split,) + c[8] for c in CASES for split in (1, 0)}


# the running-maximum test (rise / fall / peak score ramps) runs on these: every tail kind of both schedules, long loops, all pose modes
RAMP_CASES = ("n588", "q100_k375", "n196_grid288", "q130_k1025", "n1024", "n196", "n130", "pose588", "pose640", "pose196",
              "pose196_opt5", "pose520")
RAMP_PATTERNS = ("rise", "fall", "peak")
# the Gaussian test: q = sharp x N(0, 1), by position in CASES (as the kernel tests of test_gpu_kernels.py: 1, 3, 6)
SHARPS = (1.0, 3.0, 6.0)


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def sharp_of(cid):
    return SHARPS[[c[0] for c in CASES].index(cid) % len(SHARPS)]
