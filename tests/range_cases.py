"""The inventory of fp16 plane writers as plain data (no torch, no numpy): what tests/test_range_inventory.py checks against the
kernel sources on the host and what tests/test_range_gpu.py drives on the GPU.

A WRITER is a function or kernel of vista_slam_amd/csrc/*.h that declares a RangeAcc, hands the handle's range pointer to one of the
saturating converters (split_f16, to_f16_sat, split_mx4, store_mx1), or counts a range event itself (atomicAdd(p.range, ...)).
Keys are the enclosing function's name; "name[part]" classifies one part of a function that is both (the base name is what the
host test compares with the sources).

REPORTING: writer -> (counters it can raise, the tests of tests/test_range_gpu.py that drive it).  Counter 0 = a value left the
fp16 range (|x| > 65504) or was not finite; counter 1 = an fp8 correction byte of the f16mx arithmetic saturated (activation rows:
|x| > 57344, e5m2; weights: |w * 16| > 448, e4m3).
EXEMPT: writer -> the reason it never flushes, from the comment at the declaration.  Exempt writers still SATURATE; the GPU file
pins the stored value and leaves the counters alone.
"""

# the thresholds (sta_common.h): integers an fp16 holds, so every case is exact
F16_MAX = 65504
E5M2_MAX = 57344
E4M3_W_MAX = 28           # |w| * 2^4 <= 448

# hot value -> (how it is built: a, w, d with v = a * w + d), expected (counter 0, counter 1) class for plane outputs (f16x3 / f16)
# and for f16mx row outputs (head_mx); 1 = "> 0", 0 = "== 0"
HOT = {
    57344: ((28672, 2, 0), (0, 0), (0, 0)),
    57345: ((28672, 2, 1), (0, 0), (0, 1)),
    65504: ((32752, 2, 0), (0, 0), (0, 1)),
    65505: ((32752, 2, 1), (1, 0), (1, 1)),
    -65505: ((-32752, 2, -1), (1, 0), (1, 1)),
}

ARITHMETICS = ("f16x3", "f16", "head_mx")

REPORTING = {
    "epilogue_tile": ("0, 1", ("test_plane_epilogue_thresholds", "test_forced_family_thresholds", "test_convt_scatter_thresholds",
                               "test_conv3_thresholds")),
    "splitk_finish_kernel": ("0, 1", ("test_splitk_finish_thresholds", "test_conv3_thresholds")),
    "head_epilogue_t": ("0", ("test_fused_tail_saturates_head2",)),
    "qkv_finish_kernel": ("0", ("test_qkv_finish_thresholds",)),
    "rope_planes_kernel": ("0", ("test_rope_kernels_saturate",)),
    "rope_tokens_kernel": ("0", ("test_rope_kernels_saturate",)),
    "rope_varlen_kernel": ("0", ("test_rope_kernels_saturate",)),
    "bilinear_up2_kernel": ("0, 1", ("test_bilinear_reports_its_own_rows",)),
    "rows_to_planes_kernel": ("0, 1", ("test_input_converters_report_bad_values", "test_plane_epilogue_thresholds")),
    "pack_vt_kernel": ("0", ("test_input_converters_report_bad_values",)),
    "patch_gather_kernel": ("0", ("test_patch_gather_reports_a_pixel_out_of_range",)),
    "patch_gather_tokens_kernel": ("0", ("test_patch_gather_reports_a_pixel_out_of_range",)),
    "patch_gather_u8hwc_kernel": ("0", ("test_patch_gather_u8_is_silent",)),
    "patch_gather_tokens_u8hwc_kernel": ("0", ("test_patch_gather_u8_is_silent",)),
    "repack_weight_kernel": ("0, 1", ("test_weight_repack_thresholds",)),
    "ln_kernel": ("0", ("test_layernorm_row_statistics",)),
    "resid_ln_kernel": ("0", ("test_layernorm_row_statistics",)),
    # a convex combination of V rows that pack_vt_kernel / the QKV epilogue already clamped: it flushes, but nothing in range can
    # make it fire; the case pins the value it stores and that it stays silent on V = +-65504
    "attn_pose_query": ("0", ("test_attention_output_of_saturated_v",)),
}

EXEMPT = {
    "ln_store4": "a normalised row times the gains cannot leave the fp16 range; a non-finite row is counted by ln_kernel / "
                 "resid_ln_kernel from the row statistics",
    "epilogue_qkv_tile": "q / k / v are linear maps of LayerNorm outputs (bounded by sqrt(C) x the gains x the weights); the range "
                         "report covers the unnormalised tensors instead",
    "epilogue_tile[EPI_GELU]": "mlp.fc1's GELU tile is a function of a LayerNorm output and stays uncounted",
    "attn_body": "a convex combination of V rows stays inside V's range",
    "head_epilogue_t[rw]": "head.4's weight fragments: hw4 * hw4_scale is a power-of-two scaling into [0.5, 1), exact",
}

# the test of tests/test_range_gpu.py that pins the VALUE an exempt writer stores
EXEMPT_CASES = {
    "ln_store4": "test_exempt_layernorm_planes_saturate",
    "epilogue_qkv_tile": "test_exempt_qkv_epilogue_saturates",
    "epilogue_tile[EPI_GELU]": "test_exempt_gelu_epilogue_saturates",
    "attn_body": "test_attention_output_of_saturated_v",
    "head_epilogue_t[rw]": "test_fused_tail_saturates_head2",
}

# the definitions of the mechanism itself (sta_common.h): not writers
HELPERS = ("split_f16", "to_f16_sat", "split_mx4", "split_mx1", "store_mx1", "sat_f16_range", "flush")


def class_of(value, mx_out):
    """The rule behind HOT: (counter 0 raised, counter 1 raised) for an exact result `value` written to planes / to f16mx rows."""
    return (int(abs(value) > F16_MAX), int(bool(mx_out) and abs(value) > E5M2_MAX))


def range_class(rng):
    """(fp16 events, fp8 events) -> which counters are non-zero, as (0 | 1, 0 | 1): what the GPU tests pin (the event COUNT depends on
    how many lanes flush, which is not a contract)."""
    return tuple(int(c > 0) for c in rng)


def base(name):
    return name.split("[")[0]


def all_case_names():
    names = set(EXEMPT_CASES.values())
    for _, cases in REPORTING.values():
        names.update(cases)
    return names
