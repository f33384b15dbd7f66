"""ctypes binding of libsta_mi355.so (the C-ABI declared in include/sta_mi355.h).

There is NO fallback: if the HIP library is missing or fails to load, importing the product path
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)

Three builds of the same translation unit (vista_slam_amd/build.py; the third, `load_skew()` = libsta_mi355_skew.so, is the second with live
skew points behind every barrier, for tests/test_skew_gpu.py alone): `load()` = libsta_mi355.so, the product, which exports
include/sta_mi355.h and nothing else; `load_test()` = libsta_mi355_test.so (-DSTA_TEST_HOOKS), which additionally exports the
kernel-level test / micro-benchmark entry points of include/sta_mi355_debug.h.  Only tests/ and tools/ load the second one
(`STAFrontend(..., lib=_lib.load_test())`, or `_lib.use_test_hooks()` at the top of a tool).
"""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libsta_mi355.so")
TEST_LIB_PATH = os.path.join(PKG, "libsta_mi355_test.so")
SKEW_LIB_PATH = os.path.join(PKG, "libsta_mi355_skew.so")   # the test-hooks build with live skew points (csrc/sta_skew.h): `load_skew()`
CLOUD_LIB_PATH = os.path.join(PKG, "libsta_cloud.so")      # a second library with its own ABI (include/sta_cloud.h): `load_cloud()`
RASTER_LIB_PATH = os.path.join(PKG, "libsta_raster.so")    # a third one (include/sta_raster.h): `load_raster()`
TSDF_LIB_PATH = os.path.join(PKG, "libsta_tsdf.so")        # a fourth one (include/sta_tsdf.h): `load_tsdf()`
MESH_LIB_PATH = os.path.join(PKG, "libsta_mesh.so")        # a fifth one (include/sta_mesh.h): `load_mesh()`
SURF_LIB_PATH = os.path.join(PKG, "libsta_surf.so")        # a sixth one (include/sta_surf.h): `load_surf()`
SIMP_LIB_PATH = os.path.join(PKG, "libsta_simp.so")        # a seventh one (include/sta_simp.h): `load_simp()`
DIST_LIB_PATH = os.path.join(PKG, "libsta_dist.so")        # an eighth one (include/sta_dist.h): `load_dist()`
RAY_LIB_PATH = os.path.join(PKG, "libsta_ray.so")          # a ninth one (include/sta_ray.h): `load_ray()`
REG_LIB_PATH = os.path.join(PKG, "libsta_reg.so")          # a tenth one (include/sta_reg.h): `load_reg()`
KNN_LIB_PATH = os.path.join(PKG, "libsta_knn.so")          # an eleventh one (include/sta_knn.h): `load_knn()`

STA_PREC_F16 = 1
STA_PREC_F16X3 = 3
STA_PREC_F16X3H = 5
STA_PREC_F16X3M = 6
PRECISIONS = {"f16": STA_PREC_F16, "f16x3": STA_PREC_F16X3, "f16x3h": STA_PREC_F16X3H, "f16x3m": STA_PREC_F16X3M}


class StaConfig(C.Structure):
    _fields_ = [("patch_size", C.c_int32), ("enc_embed_dim", C.c_int32), ("enc_depth", C.c_int32),
                ("enc_num_heads", C.c_int32), ("dec_embed_dim", C.c_int32), ("dec_depth", C.c_int32),
                ("dec_num_heads", C.c_int32), ("mlp_ratio", C.c_int32), ("rope_base", C.c_float),
                ("ln_eps", C.c_float), ("precision", C.c_int32)]


class StaGraphState(C.Structure):
    """sta_graph_state of include/sta_mi355.h: the device arrays of one pose graph (vista_slam_amd/graph.py owns them)."""
    _fields_ = [("max_nodes", C.c_int32), ("max_edges", C.c_int32), ("max_views", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("chunks", C.c_int32), ("poses", C.c_void_p), ("edges", C.c_void_p), ("edge_poses", C.c_void_p), ("edge_confs", C.c_void_p),
                ("depth", C.c_void_p), ("conf", C.c_void_p), ("intri", C.c_void_p), ("mean_conf", C.c_void_p), ("first_node", C.c_void_p),
                ("best_node", C.c_void_p), ("best_conf", C.c_void_p), ("partials", C.c_void_p)]


class StaNNIndex(C.Structure):
    """sta_nn_index of include/sta_cloud.h: a host struct whose pointers point into the caller's device index buffer."""
    _fields_ = [("cell_key", C.c_void_p), ("cell_start", C.c_void_p), ("sorted_pts", C.c_void_p), ("sorted_idx", C.c_void_p),
                ("lo", C.c_int64 * 3), ("ext", C.c_int64 * 3), ("cell", C.c_double), ("M", C.c_int64), ("n_finite", C.c_int64), ("C", C.c_int64)]


_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
_fp = C.c_void_p   # device float* passed as integer address

# name -> (restype, argtypes); mirrors include/sta_mi355.h (the product ABI)
SIGNATURES = {
    "sta_default_config": (None, [C.POINTER(StaConfig)]),
    "sta_create": (_i, [C.POINTER(StaConfig), _i, C.POINTER(_vp)]),
    "sta_destroy": (_i, [_vp]),
    "sta_set_precision": (_i, [_vp, _i]),
    "sta_set_deterministic": (_i, [_vp, _i]),
    "sta_set_side_lanes": (_i, [_vp, _i]),
    "sta_set_varlen_heads": (_i, [_vp, _i]),
    "sta_pipeline_streams": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i)]),
    "sta_reserve": (_i, [_vp, _i, _i, _i, _i, C.POINTER(_vp), _i]),
    "sta_alloc_stats": (_i, [_vp, C.POINTER(_i64)]),
    "sta_num_expected_tensors": (_i, [_vp]),
    "sta_num_loaded_tensors": (_i, [_vp]),
    "sta_load_tensor": (_i, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i, _i]),
    "sta_finalize_weights": (_i, [_vp]),
    "sta_encode": (_i, [_vp, _fp, _i, _i, _i, _fp, _vp]),
    "sta_decode": (_i, [_vp, _fp, _fp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "sta_decode_mixed": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "sta_decode_pos": (_i, [_vp, _fp, _fp, _vp, _vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "sta_decode_tokens": (_i, [_vp, _fp, _fp, _vp, _vp, _i, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "sta_decode_varlen": (_i, [_vp, _fp, _fp, _vp, _vp, C.POINTER(_i), C.POINTER(_i), _i, _i, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "sta_head_pose": (_i, [_vp, _fp, _i, _i64, _fp, _fp, _vp]),
    "sta_head_pts_varlen": (_i, [_vp, _fp, C.POINTER(_i64), _fp, _fp, _fp, C.POINTER(_i64), C.POINTER(_i), C.POINTER(_i), _i, _fp, _fp,
                                 C.POINTER(_i64), _vp]),
    "sta_head_pts": (_i, [_vp, _fp, _i64, _fp, _i64, _fp, _i64, _fp, _i64, _i, _i, _i, _fp, _fp, _vp]),
    "sta_forward_pair": (_i, [_vp, _fp, _fp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                              C.POINTER(_vp), _vp]),
    "sta_encode_u8hwc": (_i, [_vp, _fp, _i, _i, _i, _fp, _vp]),
    "sta_encode_tokens": (_i, [_vp, _fp, _vp, _i, _i, _i, _i, _fp, _vp]),
    "sta_encode_tokens_u8hwc": (_i, [_vp, _fp, _vp, _i, _i, _i, _i, _fp, _vp]),
    "sta_encode_varlen": (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), _vp, C.POINTER(_i), _i, _fp, _vp]),
    "sta_encode_varlen_u8hwc": (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), _vp, C.POINTER(_i), _i, _fp, _vp]),
    "sta_encoder_norm": (_i, [_vp, _fp, C.c_int64, _fp, _vp]),
    "sta_forward_pair_u8hwc": (_i, [_vp, _fp, _fp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                    C.POINTER(_vp), _vp]),
    "sta_estimate_intrinsics": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _fp, _fp, _fp, _vp]),
    "sta_estimate_scale": (_i, [_vp, _fp, _fp, _fp, _fp, _i64, _fp, _vp]),
    "sta_preprocess_geometry": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "sta_preprocess_frame": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _fp, _fp, _fp, _vp]),
    "sta_world_pointcloud": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _f, _fp, _fp, _fp, C.POINTER(_i64), _vp]),
    "sta_voxel_downsample": (_i, [_vp, _fp, _fp, _i64, C.c_double, C.POINTER(C.c_double), _i, _fp, _fp, _fp, _fp, _fp, _fp,
                                  C.POINTER(_i64), _vp]),
    "sta_mat_to_se3": (_i, [_vp, _fp, _i, _fp, _vp]),
    "sta_view_consistency": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _f, _i, _fp, _vp]),
    "sta_symmetric_geo_mask": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _vp]),
    "sta_geo_valid_mask": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _f, _fp, _fp, _fp, _vp]),
    "sta_local_pointclouds": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _fp, _vp]),
    "sta_ray_depth": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _fp, _vp]),
    "sta_select_patches": (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), _i, _i, _i, _f, _i, _i, _i, C.POINTER(_i), _i,
                                _vp, _vp, _vp, _vp, _vp, _vp]),
    "sta_flow_plan": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_i64)]),
    "sta_flow_pyramid": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _fp, _vp]),
    "sta_flow_corners": (_i, [_vp, _fp, _i, _i, _i, C.c_double, _i, _i, _fp, _i64, _fp, _fp, _vp]),
    "sta_flow_track": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _i, _i, C.c_double, C.c_double, _fp, _fp, _fp, _vp]),
    "sta_orb_plan": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_i64)]),
    "sta_orb_extract": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _fp, _i64, _fp, _fp, _fp, _fp, _vp]),
    "sta_bow_transform": (_i, [_vp, _fp, _fp, _i, _fp, _fp, _fp, _fp, _fp, _i, _i, _fp, _i64, _fp, _fp, _fp, _fp, _vp]),
    "sta_bow_score": (_i, [_vp, _fp, _fp, _fp, _i, _fp, _fp, _fp, _i, _i, _fp, _i, _fp, _vp]),
    "sta_pgo_plan": (_i, [_i, _i, C.POINTER(_i64)]),
    "sta_sim3_op": (_i, [_vp, _i, _fp, _fp, _fp, _fp, _i64, _vp]),
    "sta_pgo_index": (_i, [_vp, _fp, _fp, _i, _i, _fp, _i64, _fp, _fp, _fp, _vp]),
    "sta_pgo_linearize": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
    "sta_pgo_solve": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, C.c_double, C.c_double, C.c_double, C.c_double, _i, _fp, _i64, _fp, _fp, _vp]),
    "sta_pgo_optimize": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, _i, C.c_double, C.c_double, C.c_double, _i, _i, C.c_double, _i, C.c_double, C.c_double,
                              C.c_double, C.c_double, C.c_double, _i, _fp, _i64, C.POINTER(C.c_double), _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "sta_graph_plan": (_i, [_i, _i, _i, _i, _i, C.POINTER(_i64)]),
    "sta_graph_reset": (_i, [_vp, C.POINTER(StaGraphState), _vp]),
    "sta_graph_commit": (_i, [_vp, C.POINTER(StaGraphState), _i, _i, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p,
                              C.POINTER(C.c_double), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), _vp]),
    "sta_graph_export": (_i, [_vp, C.POINTER(StaGraphState), _i, _i, _i, _f, _fp, _fp, _fp, _fp, _fp, _vp]),
    "sta_regress_views": (_i, [_vp, _fp, C.POINTER(_vp), _i, C.c_char_p, _f, _i, _i, _fp, C.POINTER(C.c_float),
                               C.POINTER(_i), C.POINTER(_i), _fp, _fp, _fp, _fp, _vp]),
    "sta_regress_views_begin": (_i, [_vp, _fp, C.POINTER(_vp), _i, _i, _i, _fp, _vp]),
    "sta_regress_views_finish": (_i, [_vp, C.c_char_p, _f, C.POINTER(C.c_float), C.POINTER(_i), C.POINTER(_i), _fp, _fp, _fp, _fp, _vp]),
    "sta_regress_views_abort": (_i, [_vp, _vp]),
    "sta_regress_views_tokens": (_i, [_vp, _fp, _i, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), _i,
                                      C.POINTER(_i), C.POINTER(_i), _vp, C.POINTER(_i), C.POINTER(_i), _vp, C.c_char_p, _f,
                                      _fp, C.POINTER(C.c_float), C.POINTER(_i), C.POINTER(_i), _fp, _fp, _fp, _fp, C.POINTER(_i), _vp]),
    "sta_regress_views_tokens_begin": (_i, [_vp, _fp, _i, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), _i,
                                            C.POINTER(_i), C.POINTER(_i), _vp, C.POINTER(_i), C.POINTER(_i), _vp, _fp, _vp]),
    "sta_regress_views_tokens_finish": (_i, [_vp, C.c_char_p, _f, C.POINTER(C.c_float), C.POINTER(_i), C.POINTER(_i),
                                             _fp, _fp, _fp, _fp, C.POINTER(_i), _vp]),
    "sta_pack_compact": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _i, _i, _i, _fp, _i64, _vp]),
    "sta_rope2d_inplace": (_i, [_fp, _i64, _i64, _vp, _i, _i, _i, _i, _f, _f, _vp]),
    "sta_rope2d_inplace_dtype": (_i, [_vp, _i, _i64, _i64, _vp, _i, _i, _i, _i, _f, _f, _vp]),
    "sta_flops_per_pair": (C.c_double, [_vp, _i, _i]),
    "sta_workspace_bytes": (_i64, [_vp]),
    "sta_weight_bytes": (_i64, [_vp]),
    "sta_enable_stage_timing": (_i, [_vp, _i]),
    "sta_get_stage_ms": (_i, [_vp, C.POINTER(_f)]),
    "sta_kernel_timing": (_i, [_vp, _i]),
    "sta_kernel_timing_read": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sta_kernel_clock_read": (_i, [_vp, C.POINTER(C.c_float)]),
    "sta_kernel_timing_filter": (_i, [_vp, _i, _i, _i, _i, _i]),
    "sta_kernel_timing_dump_shapes": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(C.c_float), C.POINTER(_i), C.POINTER(_i)]),
    "sta_range_report": (_i, [_vp, C.POINTER(C.c_ulonglong), _i]),
    "sta_last_error": (C.c_char_p, []),
    "sta_version": (C.c_char_p, []),
}

# include/sta_mi355_debug.h: kernel-level test / micro-benchmark entry points, exported by libsta_mi355_test.so only
TEST_SIGNATURES = {
    "sta_set_gemm_variant": (_i, [_vp, _i]),
    "sta_kernel_timing_dump": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(_i), C.POINTER(_i)]),
    "sta_kernel_stamps_dump": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(_i)]),
    "sta_bench_gemm_stamps": (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong), _i, _vp]),
    "sta_bench_gemm": (_i, [_vp, _i, _i, _i, _i, _i, _i, C.POINTER(_f), _vp]),
    "sta_bench_gemm_last_ghz": (C.c_float, []),
    "sta_bench_attention_mixed": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_f), _vp]),
    "sta_bench_attention": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_f), _vp]),
    "sta_debug_gemm": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _vp]),
    "sta_debug_qkv_rope": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _fp, _fp, _fp, _vp]),
    "sta_debug_attention": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _vp]),
    "sta_debug_attention_pose": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _fp, _vp]),
    "sta_debug_attention_mixed": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _fp, _vp]),
    "sta_debug_attn_mixed_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "sta_debug_last_attn_mixed_plan": (_i, [_vp, C.POINTER(_i)]),
    "sta_debug_attn_mixed_block_map": (_i, [_i, _i, _i, _i, _i, C.POINTER(_i)]),
    "sta_debug_attn_varlen": (_i, [_vp, _fp, _fp, _fp, _i, _i, C.POINTER(_i), C.POINTER(_i), _i, _fp, _vp]),
    "sta_debug_attn_varlen_plan": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i), _i, _i, C.POINTER(_i)]),
    "sta_debug_last_attn_varlen_plan": (_i, [_vp, C.POINTER(_i)]),
    "sta_debug_attn_varlen_block_map": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "sta_debug_attn_encv": (_i, [_vp, _fp, _fp, _fp, _i, _i, C.POINTER(_i), _fp, _vp]),
    "sta_debug_attn_encv_plan": (_i, [_i, _i, C.POINTER(_i), _i, _i, C.POINTER(_i)]),
    "sta_debug_last_attn_encv_plan": (_i, [_vp, C.POINTER(_i)]),
    "sta_debug_attn_encv_block_map": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "sta_debug_qkv_finish_varlen": (_i, [_vp, _fp, _fp, _vp, _i, _i, C.POINTER(_i), _i, _fp, _fp, _fp, _vp]),
    "sta_debug_patch_gather_varlen": (_i, [_vp, C.POINTER(_vp), _i, C.POINTER(_i), C.POINTER(_i), _vp, C.POINTER(_i), _i, _i, _fp, _vp]),
    "sta_debug_gather_tokens": (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp, _vp, _i, _i, _fp, _vp, _vp]),
    "sta_debug_pose_rows": (_i, [_vp, _fp, _i64, C.POINTER(_i64), _i, _fp, _fp, _vp]),
    "sta_debug_rope_varlen": (_i, [_vp, C.POINTER(_vp), _i, _i, _i, C.POINTER(_i), _vp, _i, _vp]),
    "sta_debug_rope_tokens": (_i, [_vp, C.POINTER(_vp), _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "sta_debug_rope_enc_tokens": (_i, [_vp, C.POINTER(_vp), _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "sta_debug_attn_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "sta_debug_last_attn_plan": (_i, [_vp, C.POINTER(_i)]),
    "sta_debug_attn_block_map": (_i, [_i, C.POINTER(_i)]),
    "sta_debug_set_tail_hint": (_i, [_vp, _i]),
    "sta_debug_set_option": (_i, [_vp, _i, _i]),
    "sta_debug_pick_family": (_i, [_i, _i, C.c_longlong, _i, _i, _i, _i, _i, _i]),
    "sta_debug_gemm_has_kernel": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "sta_debug_gemm_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "sta_debug_last_gemm_plan": (_i, [_vp, C.POINTER(_i)]),
    "sta_debug_qkv_pair_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "sta_debug_qkv_pair": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _vp]),
    "sta_debug_conv3x3": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _vp]),
    "sta_debug_conv3x3_r2": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _fp, _vp]),
    "sta_debug_conv3_head": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _vp]),
    "sta_debug_conv_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "sta_debug_convt": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _vp]),
    "sta_debug_up2": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _fp, _vp]),
    "sta_debug_layernorm": (_i, [_vp, _fp, _fp, _fp, _i, _i, _f, _fp, _fp, _vp]),
    "sta_debug_gemm_resid_ln": (_i, [_vp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _fp, _fp, _f, _fp, _fp, _vp]),
    "sta_debug_head_final": (_i, [_vp, _fp, _fp, _fp, _i64, _fp, _fp, _vp]),
    "sta_debug_svd_orthogonalize": (_i, [_vp, _fp, _fp, _i, _vp]),
    "sta_debug_conv3x3_varlen": (_i, [_vp, _fp, _fp, _fp, _i, C.POINTER(_i), C.POINTER(_i), _i, _i, _i, _i, _i, _fp, _fp, _fp, _vp, _vp]),
    "sta_debug_conv3_head_varlen": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, C.POINTER(_i), C.POINTER(_i), _fp, _fp, _vp]),
    "sta_debug_convt_varlen": (_i, [_vp, _fp, _fp, _fp, _i, C.POINTER(_i), C.POINTER(_i), _i, _i, _fp, _vp, _vp]),
    "sta_debug_up2_varlen": (_i, [_vp, _fp, _i, C.POINTER(_i), C.POINTER(_i), _i, C.POINTER(_i), C.POINTER(_i), _fp, _vp, _vp]),
    "sta_debug_dpt_varlen_plan": (_i, [_i, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_longlong), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i]),
    "sta_debug_workspace_fill": (_i, [_vp, _vp, _i]),
    "sta_debug_workspace_info": (_i, [_vp, _vp, C.POINTER(_i64)]),
    "sta_debug_workspace_tail": (_i, [_vp, _vp, _i, C.POINTER(_i64), C.POINTER(_i64)]),
}

# include/sta_mi355_skew.h (what include/sta_mi355_debug.h includes under STA_WAVE_SKEW): exported by libsta_mi355_skew.so alone
SKEW_SIGNATURES = {
    "sta_debug_set_wave_skew": (_i, [C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "sta_debug_wave_skew_hits": (_i, [C.POINTER(C.c_ulonglong)]),      # out[34]
}

# include/sta_cloud.h: libsta_cloud.so, handle-free; NOT part of SIGNATURES (which stays equal to include/sta_mi355.h)
CLOUD_SIGNATURES = {
    "sta_nn_plan": (_i, [_i64, _i64, C.POINTER(_i64)]),
    "sta_nn_build": (_i, [_fp, _i64, C.c_double, _vp, _i64, _vp, _i64, C.POINTER(StaNNIndex), _vp]),
    "sta_nn_query": (_i, [C.POINTER(StaNNIndex), _fp, _i64, C.POINTER(C.c_double), C.c_double, _fp, _fp, _fp, _vp, _i64, _vp]),
    "sta_cloud_transform": (_i, [_fp, _i64, C.POINTER(C.c_double), _fp, _vp]),
    "sta_cloud_last_error": (C.c_char_p, []),
}

# include/sta_raster.h: libsta_raster.so, handle-free; a table of its own like CLOUD_SIGNATURES
_dp = C.POINTER(C.c_double)
RASTER_SIGNATURES = {
    "sta_raster_plan": (_i, [_i, _i, _i, C.POINTER(_i64)]),
    "sta_raster_clear": (_i, [_vp, _i, _i, _i, _vp]),
    "sta_raster_points": (_i, [_vp, _i, _i, _i, _fp, _vp, _i, _i64, _i64, _dp, _dp, C.c_double, C.c_double, _i, _vp, _vp]),
    "sta_raster_lines": (_i, [_vp, _i, _i, _i, _fp, _vp, _i64, _dp, _dp, C.c_double, C.c_double, _i, _vp]),
    "sta_raster_resolve": (_i, [_vp, _i, _i, _i, C.POINTER(C.c_uint8), _vp, _vp, _vp, _vp]),
    "sta_raster_last_error": (C.c_char_p, []),
}

# include/sta_tsdf.h: libsta_tsdf.so, handle-free; a table of its own like the two above
_i64p = C.POINTER(_i64)
TSDF_SIGNATURES = {
    "sta_tsdf_plan": (_i, [_i64, _i, _i, C.c_double, C.c_double, _i64, _i64, _i64, _i64p]),
    "sta_tsdf_table": (_i, [C.POINTER(C.c_int8)]),
    "sta_tsdf_blocks": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, C.c_double, C.c_double, _dp, C.c_double, _vp, _i64, _vp, _i64, _i64p, _vp]),
    "sta_tsdf_clear": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "sta_tsdf_integrate": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i64, _i64, C.c_double, C.c_double, _dp, C.c_double,
                                C.c_double, _vp]),
    "sta_tsdf_mesh": (_i, [_vp, _i64, _vp, _vp, _vp, C.c_double, _dp, C.c_double, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64p, _vp]),
    "sta_tsdf_last_error": (C.c_char_p, []),
}

# include/sta_mesh.h: libsta_mesh.so, handle-free; a table of its own like the three above
MESH_SIGNATURES = {
    "sta_mesh_plan": (_i, [_i64, _i64, _i64p]),
    "sta_mesh_triangles": (_i, [_vp, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _dp, _dp, _i, _i, _i64, _dp, _dp, C.c_double, C.c_double, _vp, _vp, _i64, _vp]),
    "sta_mesh_vertex_normals": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "sta_mesh_last_error": (C.c_char_p, []),
}

# include/sta_surf.h: libsta_surf.so, handle-free; a table of its own like the four above
SURF_SIGNATURES = {
    "sta_surf_plan": (_i, [_i64, _i64, _i64, _i64p]),
    "sta_surf_components": (_i, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sta_surf_weights": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sta_surf_sample": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, C.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    "sta_surf_last_error": (C.c_char_p, []),
}
# include/sta_simp.h: libsta_simp.so, handle-free; a table of its own like the five above
_d = C.c_double
SIMP_SIGNATURES = {
    "sta_simp_plan": (_i, [_i64, _i64, _i64p]),
    "sta_simp_cells": (_i, [_vp, _i64, _d, _d, _d, _d, _vp, _vp, _vp, _i64, _vp]),
    "sta_simp_triangles": (_i, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sta_simp_place": (_i, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _d, _d, _d, _d, _i, _d, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sta_simp_last_error": (C.c_char_p, []),
}
# include/sta_dist.h: libsta_dist.so, handle-free; a table of its own like the six above (the host struct sta_tri_index goes as void*)
DIST_SIGNATURES = {
    "sta_tri_plan": (_i, [_i64, _i64, _i64p]),
    "sta_tri_build": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "sta_tri_query": (_i, [_vp, _vp, _i64, _d, _vp, _vp, _vp, _vp]),
    "sta_tri_last_error": (C.c_char_p, []),
}
# include/sta_ray.h: libsta_ray.so, handle-free; a table of its own like the seven above (the index of libsta_dist.so goes as four pointers)
RAY_SIGNATURES = {
    "sta_ray_plan": (_i, [_i64, _i64, _i64p]),
    "sta_ray_cast": (_i, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "sta_ray_occluded": (_i, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _d, _d, _vp, _vp, _vp]),
    "sta_ray_last_error": (C.c_char_p, []),
}
# include/sta_reg.h: libsta_reg.so, handle-free; a table of its own like the eight above (the index goes as four pointers, T_host and
# pivot_host as host doubles)
REG_SIGNATURES = {
    "sta_reg_plan": (_i, [_i64, _i64, _i64p]),
    "sta_reg_pass": (_i, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _dp, _dp, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "sta_reg_last_error": (C.c_char_p, []),
}
# include/sta_knn.h: libsta_knn.so, handle-free; a table of its own like the nine above (the index of libsta_cloud.so goes as the host
# struct StaNNIndex, which the header restates as sta_knn_grid; view_host as host doubles)
KNN_SIGNATURES = {
    "sta_knn_plan": (_i, [_i64, _i64, _i64, _i64p]),
    "sta_knn_query": (_i, [C.POINTER(StaNNIndex), _vp, _i64, _vp, _i64, _i64, _d, _vp, _vp, _vp, _vp, _vp]),
    "sta_knn_moments": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _dp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sta_knn_last_error": (C.c_char_p, []),
}


class StaTriIndex(C.Structure):
    """sta_tri_index of include/sta_dist.h: pointers into the caller's index buffer and the shape of the implicit tree."""
    _fields_ = [("tri", C.c_void_p), ("src", C.c_void_p), ("boxes", C.c_void_p), ("counters", C.c_void_p), ("nt", C.c_int64),
                ("levels", C.c_int32), ("reserved", C.c_int32), ("level_offset", C.c_int64 * 10)]


_lib = None
_test_lib = None
_skew_lib = None
_satellites = {}      # path -> the loaded handle-free library

class StaError(RuntimeError):
    pass


_last_called = None      # the library object of the most recent C call: sta_last_error() is per library (two builds may be loaded)


def _bind(lib, table, strict):
    def note(result, _func, _args):
        global _last_called
        _last_called = lib
        return result
    for name, (res, args) in table.items():
        fn = getattr(lib, name, None) if not strict else getattr(lib, name)    # strict: AttributeError if the .so does not export it
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
            if name != "sta_last_error":
                fn.errcheck = note


def load_other(path):
    """A SECOND build of the library next to the product one (tools/ab_inproc.py: same-process A/B of two builds).  Binds
    the symbols that build exports; never used by the product path."""
    import torch  # noqa: F401
    lib = C.CDLL(path)
    _bind(lib, SIGNATURES, strict=False)
    _bind(lib, TEST_SIGNATURES, strict=False)
    return lib


def _missing(path):
    return StaError(f"{path} not found: the MI355X STA frontend has no CPU fallback. "
                    "Build it with `python -m vista_slam_amd.build` (needs hipcc) or `__graft_entry__.build()`.")


def load():
    """Load libsta_mi355.so (the product library) and bind every symbol of include/sta_mi355.h; raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise _missing(LIB_PATH)
    # torch must be imported BEFORE the library: the ROCm wheel bundles its own libamdhip64 and the
    # process must end up with exactly one HIP runtime (loading /opt/rocm's first makes the second
    # initialisation fail with "no ROCm-capable device is detected").
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    _bind(lib, SIGNATURES, strict=True)
    _lib = lib
    return lib


def load_test():
    """Load libsta_mi355_test.so: the product ABI plus the kernel-level test / micro-benchmark entry points
    (include/sta_mi355_debug.h).  tests/ and tools/ only."""
    global _test_lib
    if _test_lib is not None:
        return _test_lib
    if not os.path.exists(TEST_LIB_PATH):
        raise _missing(TEST_LIB_PATH)
    import torch  # noqa: F401
    lib = C.CDLL(TEST_LIB_PATH)
    _bind(lib, SIGNATURES, strict=True)
    _bind(lib, TEST_SIGNATURES, strict=True)
    _test_lib = lib
    return lib


def load_skew():
    """Load libsta_mi355_skew.so: the test-hooks build whose kernels carry live skew points (csrc/sta_skew.h), plus the two
    sta_debug_*wave_skew* entry points.  tests/test_skew_gpu.py only; `STAFrontend(..., lib=_lib.load_skew())`."""
    global _skew_lib
    if _skew_lib is not None:
        return _skew_lib
    if not os.path.exists(SKEW_LIB_PATH):
        raise _missing(SKEW_LIB_PATH)
    import torch  # noqa: F401
    lib = C.CDLL(SKEW_LIB_PATH)
    _bind(lib, SIGNATURES, strict=True)
    _bind(lib, TEST_SIGNATURES, strict=True)
    _bind(lib, SKEW_SIGNATURES, strict=True)
    _skew_lib = lib
    return lib


def _load_satellite(path, table):
    """Load one handle-free library (once per path) and bind every symbol of its signature table; raises if it is absent (no fallback
    here either)."""
    lib = _satellites.get(path)
    if lib is not None:
        return lib
    if not os.path.exists(path):
        raise _missing(path)
    import torch  # noqa: F401      (one HIP runtime per process: see load())
    lib = C.CDLL(path)
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _satellites[path] = lib
    return lib


def _satellite(path, table, last_error):
    """(load_x, check_x) of one handle-free library.  Its errors are its own: check_x(rc) raises what its `last_error` function says."""
    def load_x():
        return _load_satellite(path, table)

    def check_x(rc):
        if rc != 0:
            raise StaError((getattr(load_x(), last_error)() or b"unknown error").decode())
    return load_x, check_x


load_cloud, check_cloud = _satellite(CLOUD_LIB_PATH, CLOUD_SIGNATURES, "sta_cloud_last_error")        # include/sta_cloud.h
load_raster, check_raster = _satellite(RASTER_LIB_PATH, RASTER_SIGNATURES, "sta_raster_last_error")    # include/sta_raster.h
load_tsdf, check_tsdf = _satellite(TSDF_LIB_PATH, TSDF_SIGNATURES, "sta_tsdf_last_error")              # include/sta_tsdf.h
load_mesh, check_mesh = _satellite(MESH_LIB_PATH, MESH_SIGNATURES, "sta_mesh_last_error")              # include/sta_mesh.h
load_surf, check_surf = _satellite(SURF_LIB_PATH, SURF_SIGNATURES, "sta_surf_last_error")              # include/sta_surf.h
load_simp, check_simp = _satellite(SIMP_LIB_PATH, SIMP_SIGNATURES, "sta_simp_last_error")              # include/sta_simp.h
load_dist, check_dist = _satellite(DIST_LIB_PATH, DIST_SIGNATURES, "sta_tri_last_error")               # include/sta_dist.h: its names are sta_tri_*
load_ray, check_ray = _satellite(RAY_LIB_PATH, RAY_SIGNATURES, "sta_ray_last_error")                   # include/sta_ray.h
load_reg, check_reg = _satellite(REG_LIB_PATH, REG_SIGNATURES, "sta_reg_last_error")                   # include/sta_reg.h
load_knn, check_knn = _satellite(KNN_LIB_PATH, KNN_SIGNATURES, "sta_knn_last_error")                   # include/sta_knn.h


def use_test_hooks():
    """tools/: make the test-hooks build THIS process's default library, so that every STAFrontend() created afterwards has the
    sta_debug_* / sta_bench_* entry points.  Never called by the product path."""
    global _lib
    _lib = load_test()
    return _lib


def check(rc):
    if rc != 0:
        lib = _last_called or _lib or _test_lib or load()
        msg = lib.sta_last_error()
        raise StaError((msg or b"unknown error").decode())
