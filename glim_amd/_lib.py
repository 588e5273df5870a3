"""ctypes loader for libglim_amd.so (the C-ABI shared library declared in include/glim_amd.h).

The product path fails loudly when the HIP extension is missing: there is NO CPU fallback anywhere in this package.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLIM_AMD_LIB") or os.path.join(_HERE, "libglim_amd.so")  # GLIM_AMD_LIB: profiling builds only
CSRC = os.path.join(_HERE, "csrc")

COMPACT_DOUBLES = 29
FACTOR_BINARY = 0x1
FACTOR_SURFACE_VALIDATION = 0x2

ERR = {
    0: "ok", -1: "invalid argument", -2: "HIP runtime error", -3: "no HIP device", -4: "voxel coordinate out of key range",
    -5: "invalid state for this call", -6: "unsupported", -7: "out of memory",
}


class Linearized6(C.Structure):
    _fields_ = [
        ("num_inliers", C.c_int64),
        ("error", C.c_double),
        ("H_tt", C.c_double * 36),
        ("H_ss", C.c_double * 36),
        ("H_ts", C.c_double * 36),
        ("b_t", C.c_double * 6),
        ("b_s", C.c_double * 6),
    ]


class CtLinearized(C.Structure):
    """glim_amd_ct_linearized: HessianFactor(X, Y, H_00, H_01, -b_0, H_11, -b_1, error) of the continuous-time GICP factor."""

    _fields_ = [
        ("num_inliers", C.c_int64),
        ("error", C.c_double),
        ("H_00", C.c_double * 36),
        ("H_01", C.c_double * 36),
        ("H_11", C.c_double * 36),
        ("b_0", C.c_double * 6),
        ("b_1", C.c_double * 6),
    ]


class PreprocessParams(C.Structure):
    """glim_amd_preprocess_params (include/glim_amd.h) == CloudPreprocessorParams (cloud_preprocessor.cpp:20-61)."""

    _fields_ = [
        ("distance_near_thresh", C.c_double),
        ("distance_far_thresh", C.c_double),
        ("use_random_grid_downsampling", C.c_int32),
        ("downsample_target", C.c_int32),
        ("downsample_resolution", C.c_double),
        ("downsample_rate", C.c_double),
        ("global_shutter", C.c_int32),
        ("enable_outlier_removal", C.c_int32),
        ("outlier_removal_k", C.c_int32),
        ("outlier_std_mul_factor", C.c_double),
        ("enable_cropbox_filter", C.c_int32),
        ("crop_bbox_frame_imu", C.c_int32),
        ("crop_bbox_min", C.c_double * 3),
        ("crop_bbox_max", C.c_double * 3),
        ("T_imu_lidar", C.c_double * 12),
        ("k_correspondences", C.c_int32),
        ("voxelgrid_block_size", C.c_int32),
        ("seed", C.c_uint64),
    ]


class GncParams(C.Structure):
    """glim_amd_gnc_params (include/glim_amd.h "GNC") == gtsam_points::GNCParams as manual_loop_close_modal.cpp:449-456 fills it."""

    _fields_ = [
        ("max_init_samples", C.c_int32),
        ("tuple_check", C.c_int32),
        ("tuple_thresh", C.c_double),
        ("max_num_tuples", C.c_int32),
        ("div_factor", C.c_double),
        ("max_iterations", C.c_int32),
        ("max_corr_dist", C.c_double),
        ("inlier_voxel_resolution", C.c_double),
        ("dof", C.c_int32),
        ("seed", C.c_uint64),
    ]


class GncInfo(C.Structure):
    _fields_ = [
        ("num_correspondences", C.c_int64),
        ("num_tuples", C.c_int64),
        ("list_length", C.c_int64),
        ("mu_final", C.c_double),
        ("weight_sum", C.c_double),
        ("cost", C.c_double),
    ]


class RansacParams(C.Structure):
    """glim_amd_ransac_params (include/glim_amd.h "RANSAC") == gtsam_points::RANSACParams as manual_loop_close_modal.cpp:435-441 fills it."""

    _fields_ = [
        ("max_iterations", C.c_int32),
        ("early_stop_inlier_rate", C.c_double),
        ("poly_error_thresh", C.c_double),
        ("inlier_voxel_resolution", C.c_double),
        ("dof", C.c_int32),
        ("seed", C.c_uint64),
    ]


class RegistrationResult(C.Structure):
    """glim_amd_registration_result"""

    _fields_ = [
        ("T_target_source", C.c_double * 12),
        ("inlier_rate", C.c_double),
        ("num_inliers", C.c_int64),
        ("best_iteration", C.c_int32),
        ("iterations_run", C.c_int32),
    ]


class LMParams(C.Structure):
    """glim_amd_lm_params (include/glim_amd.h "GICP fine registration")"""

    _fields_ = [
        ("lambda_initial", C.c_double),
        ("lambda_factor", C.c_double),
        ("lambda_upper_bound", C.c_double),
        ("lambda_lower_bound", C.c_double),
        ("relative_error_tol", C.c_double),
        ("absolute_error_tol", C.c_double),
        ("max_iterations", C.c_int32),
        ("max_trials", C.c_int32),
        ("error_scale", C.c_double),
    ]


class AlignResult(C.Structure):
    """glim_amd_align_result"""

    _fields_ = [
        ("T_target_source", C.c_double * 12),
        ("error", C.c_double),
        ("num_inliers", C.c_int64),
        ("iterations", C.c_int32),
        ("trials", C.c_int32),
        ("status", C.c_int32),
        ("reserved", C.c_int32),
        ("lam", C.c_double),
        ("compact", C.c_double * COMPACT_DOUBLES),
    ]


class AlignTraceEntry(C.Structure):
    """glim_amd_align_trace_entry (include/glim_amd_diag.h)"""

    _fields_ = [
        ("T_candidate", C.c_double * 12),
        ("lam", C.c_double),
        ("compact", C.c_double * COMPACT_DOUBLES),
        ("accepted", C.c_int32),
        ("status", C.c_int32),
    ]


class CtAlignTerms(C.Structure):
    """glim_amd_ct_align_terms (include/glim_amd.h "CT-GICP frame alignment")"""

    _fields_ = [
        ("T_location", C.c_double * 12),
        ("location_precision", C.c_double),
        ("T_between", C.c_double * 12),
        ("between_precision", C.c_double),
    ]


class CtAlignResult(C.Structure):
    """glim_amd_ct_align_result"""

    _fields_ = [
        ("X", C.c_double * 12),
        ("Y", C.c_double * 12),
        ("linearized", CtLinearized),
        ("cost", C.c_double),
        ("location_cost", C.c_double),
        ("between_cost", C.c_double),
        ("lam", C.c_double),
        ("iterations", C.c_int32),
        ("trials", C.c_int32),
        ("status", C.c_int32),
        ("reserved", C.c_int32),
    ]


class CtAlignTraceEntry(C.Structure):
    """glim_amd_ct_align_trace_entry (include/glim_amd_diag.h)"""

    _fields_ = [
        ("X", C.c_double * 12),
        ("Y", C.c_double * 12),
        ("lam", C.c_double),
        ("record", C.c_double * 92),
        ("cost", C.c_double),
        ("accepted", C.c_int32),
        ("status", C.c_int32),
    ]


BUNDLE_MAX_POSES, BUNDLE_MAX_FACTORS, BUNDLE_MAX_TERMS = 32, 1024, 1024  # GLIM_AMD_BUNDLE_MAX_* (include/glim_amd.h)
GRAPH_MAX_POSES, GRAPH_MAX_FACTORS, GRAPH_MAX_TERMS = 256, 32768, 1024  # GLIM_AMD_GRAPH_MAX_* (the global-graph optimisation)


class BundlePrior(C.Structure):
    """glim_amd_bundle_prior (include/glim_amd.h "Sub-map bundle optimisation")"""

    _fields_ = [("pose", C.c_int32), ("reserved", C.c_int32), ("T", C.c_double * 12), ("information", C.c_double * 36)]


class BundleBetween(C.Structure):
    """glim_amd_bundle_between"""

    _fields_ = [("pose_i", C.c_int32), ("pose_j", C.c_int32), ("T", C.c_double * 12), ("information", C.c_double * 36)]


class BundleResult(C.Structure):
    """glim_amd_bundle_result"""

    _fields_ = [
        ("cost", C.c_double),
        ("factor_cost", C.c_double),
        ("prior_cost", C.c_double),
        ("between_cost", C.c_double),
        ("num_inliers", C.c_int64),
        ("iterations", C.c_int32),
        ("trials", C.c_int32),
        ("status", C.c_int32),
        ("reserved", C.c_int32),
        ("lam", C.c_double),
    ]


class BundleTraceRound(C.Structure):
    """glim_amd_bundle_trace_round (include/glim_amd_diag.h)"""

    _fields_ = [("lam", C.c_double), ("cost", C.c_double), ("accepted", C.c_int32), ("status", C.c_int32)]


class GraphDamping(C.Structure):
    """glim_amd_graph_damping (include/glim_amd.h "Damping terms and Huber between terms")"""

    _fields_ = [("pose", C.c_int32), ("reserved", C.c_int32), ("diagonal", C.c_double * 6)]


class GraphTerms(C.Structure):
    """glim_amd_graph_terms"""

    _fields_ = [("dampings", C.POINTER(GraphDamping)), ("num_dampings", C.c_int32), ("reserved", C.c_int32), ("between_huber_width", C.POINTER(C.c_double))]


class NavVectorPrior(C.Structure):
    """glim_amd_nav_vector_prior (include/glim_amd.h "Graph optimisation with velocity and bias variables")"""

    _fields_ = [("node", C.c_int32), ("reserved", C.c_int32), ("value", C.c_double * 6), ("information", C.c_double * 36)]


class NavVectorBetween(C.Structure):
    """glim_amd_nav_vector_between"""

    _fields_ = [("node_i", C.c_int32), ("node_j", C.c_int32), ("measurement", C.c_double * 6), ("information", C.c_double * 36)]


class NavImuTerm(C.Structure):
    """glim_amd_nav_imu_term"""

    _fields_ = [("pose_i", C.c_int32), ("velocity_i", C.c_int32), ("pose_j", C.c_int32), ("velocity_j", C.c_int32), ("bias", C.c_int32), ("mode", C.c_int32),
                ("dt", C.c_double), ("gravity", C.c_double * 3), ("bias_hat", C.c_double * 6), ("delta", C.c_double * 9), ("H_bias", C.c_double * 54),
                ("information", C.c_double * 81)]


class NavTerms(C.Structure):
    """glim_amd_nav_terms"""

    _fields_ = [("kinds", C.POINTER(C.c_int32)), ("vector_priors", C.POINTER(NavVectorPrior)), ("vector_betweens", C.POINTER(NavVectorBetween)),
                ("imu_terms", C.POINTER(NavImuTerm)), ("num_vector_priors", C.c_int32), ("num_vector_betweens", C.c_int32), ("num_imu_terms", C.c_int32),
                ("reserved", C.c_int32)]


class NavResult(C.Structure):
    """glim_amd_nav_result"""

    _fields_ = [("cost", C.c_double), ("factor_cost", C.c_double), ("prior_cost", C.c_double), ("between_cost", C.c_double), ("vector_prior_cost", C.c_double),
                ("vector_between_cost", C.c_double), ("imu_cost", C.c_double), ("num_inliers", C.c_int64), ("iterations", C.c_int32), ("trials", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32), ("lam", C.c_double)]


NODE_POSE, NODE_BIAS, NODE_VELOCITY = 0, 1, 2  # GLIM_AMD_NODE_*
IMU_TANGENT, IMU_MANIFOLD = 0, 1               # GLIM_AMD_IMU_*


class BaParams(C.Structure):
    """glim_amd_ba_params (include/glim_amd.h "Plane / edge bundle-adjustment factors and ball selection")"""

    _fields_ = [("min_radius", C.c_double), ("max_radius", C.c_double), ("plane_eps", C.c_double)]


class BaStats(C.Structure):
    """glim_amd_ba_stats"""

    _fields_ = [("num_points", C.c_int64), ("sum", C.c_double * 3), ("sum_cross", C.c_double * 6), ("eigenvalues", C.c_double * 3)]


class BaRadiusResult(C.Structure):
    """glim_amd_ba_radius_result"""

    _fields_ = [("radius", C.c_double), ("num_points", C.c_int64), ("eigenvalues", C.c_double * 3), ("trials", C.c_int32), ("stop", C.c_int32)]


class BaTraceEntry(C.Structure):
    """glim_amd_ba_trace_entry (include/glim_amd_diag.h)"""

    _fields_ = [("radius", C.c_double), ("count", C.c_int64), ("eigenvalues", C.c_double * 3), ("decision", C.c_int32), ("reserved", C.c_int32)]


BA_MAX_FRAMES, BA_MAX_TRIALS, BA_MOMENT_DOUBLES, BA_DEGENERATE = 128, 10, 13, 0x1  # GLIM_AMD_BA_* (include/glim_amd.h)


class EditWindow(C.Structure):
    """glim_amd_edit_window (include/glim_amd.h "Map editing")"""

    _fields_ = [("center", C.c_double * 3), ("resolution", C.c_double), ("window", C.c_int32), ("reserved", C.c_int32)]


class EditOutlierParams(C.Structure):
    """glim_amd_edit_outlier_params"""

    _fields_ = [("radius_offset", C.c_double), ("stddev_thresh", C.c_double), ("num_neighbors", C.c_int32), ("reserved", C.c_int32)]


class EditRegionGrowingParams(C.Structure):
    """glim_amd_edit_region_growing_params"""

    _fields_ = [("distance_threshold", C.c_double), ("cos_angle_threshold", C.c_double), ("dilation_radius", C.c_double), ("use_normals", C.c_int32),
                ("max_hops", C.c_int32)]


class EditRegionResult(C.Structure):
    """glim_amd_edit_region_result"""

    _fields_ = [("count", C.c_int64), ("num_candidates", C.c_int64), ("seed", C.c_int32 * 2), ("rounds", C.c_int32), ("status", C.c_int32),
                ("seed_qq", C.c_double)]


class EditMinCutParams(C.Structure):
    """glim_amd_edit_min_cut_params"""

    _fields_ = [("distance_sigma", C.c_double), ("angle_sigma", C.c_double), ("foreground_mask_radius", C.c_double), ("background_mask_radius", C.c_double),
                ("foreground_weight", C.c_double), ("background_weight", C.c_double), ("k_neighbors", C.c_int32), ("use_normals", C.c_int32),
                ("max_rounds", C.c_int32), ("reserved", C.c_int32)]


class EditMinCutResult(C.Structure):
    """glim_amd_edit_min_cut_result"""

    _fields_ = [("count", C.c_int64), ("num_candidates", C.c_int64), ("num_edges", C.c_int64), ("num_foreground", C.c_int64), ("num_background", C.c_int64),
                ("flow", C.c_int64), ("rounds", C.c_int32), ("looks", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


EDIT_BOX, EDIT_SPHERE, EDIT_WINDOW, EDIT_WINDOW_BALL = 0, 1, 2, 3  # GLIM_AMD_EDIT_* (include/glim_amd.h)
EDIT_ROUNDS_PER_LOOK = 32
EDIT_OK, EDIT_EMPTY, EDIT_FEW_POINTS, EDIT_NO_SEED, EDIT_ROUND_LIMIT = 0, 1, 2, 3, 4
EDIT_CAP_SCALE, EDIT_MIN_CUT_MAX_ROUNDS = 65536, 65536


class GlimAmdError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: {ERR.get(code, 'unknown error')} ({code}){(' -- ' + detail) if detail else ''}")


def build(force=False):
    """Compile every HIP source for gfx950 with hipcc (glim_amd/csrc/Makefile) into glim_amd/libglim_amd.so."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("hipcc build did not produce " + LIB_PATH)
    return LIB_PATH


# every symbol include/glim_amd.h declares: name -> (restype, argtypes)
_vp, _i, _i32, _i64, _u32, _d, _sz = C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_double, C.c_size_t
_dp, _fp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_pp = C.POINTER(C.c_void_p)
SYMBOLS = {
    "glim_amd_version": (_i, []),
    "glim_amd_error_string": (C.c_char_p, [_i]),
    "glim_amd_last_hip_error": (C.c_char_p, []),
    "glim_amd_device_count": (_i, []),
    "glim_amd_ctx_create": (_i, [_i, _i, _vp, _pp]),
    "glim_amd_ctx_create_ex": (_i, [_i, _i, _vp, _i, _pp]),
    "glim_amd_ctx_destroy": (_i, [_vp]),
    "glim_amd_ctx_synchronize": (_i, [_vp]),
    "glim_amd_ctx_set_diag": (_i, [_vp, C.c_char_p]),
    "glim_amd_ctx_get_diag": (_i, [_vp, C.c_char_p, _sz]),
    "glim_amd_device_info": (_i, [_vp, C.c_char_p, _sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_i)]),
    "glim_amd_cloud_create": (_i, [_vp, _i64, _dp, _dp, _dp, _pp]),
    "glim_amd_cloud_create_f32": (_i, [_vp, _i64, _fp, _fp, _fp, _pp]),
    "glim_amd_cloud_create_deskewed": (_i, [_vp, _i64, _dp, _dp, _dp, _i32, _dp, _dp, _d, _dp, _dp, _i32, _pp]),
    "glim_amd_preprocess_default_params": (_i, [C.POINTER(PreprocessParams)]),
    "glim_amd_preprocess": (_i, [_vp, _i64, _dp, _dp, _dp, C.POINTER(PreprocessParams), _pp]),
    "glim_amd_cloud_download_frame": (_i, [_vp, _dp, _dp, _dp, _ip]),
    "glim_amd_factor_set_profile_fresh_samples": (_i, [_vp, _i32, _pp, _pp, C.POINTER(C.c_uint32), _dp, _i, _d, _fp]),
    "glim_amd_factor_set_trip_stats": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _i]),
    "glim_amd_multi_last_timing": (_i, [_vp, _fp, _fp]),
    "glim_amd_multi_last_breakdown": (_i, [_vp, _i32, _dp, _i32]),
    "glim_amd_debug_plan_stats": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _ip]),
    "glim_amd_debug_ctx_query_streams": (_i, [_vp, _ip]),
    "glim_amd_debug_pool_stats": (_i, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "glim_amd_debug_frame_stages": (_i, [_dp, _i32]),
    "glim_amd_multi_set_one_rank_collective": (_i, [_vp, _i32]),
    "glim_amd_multi_set_host_records": (_i, [_vp, _i32]),
    "glim_amd_factor_set_linearize_repeat": (_i, [_vp, _dp, _i, _i, _vp]),
    "glim_amd_multi_set_split": (_i, [_vp, _i32]),
    "glim_amd_multi_records": (_i, [_vp, _i64, _i64, _dp]),
    "glim_amd_voxelmap_set_lru_horizon": (_i, [_vp, _i32, _i32]),
    "glim_amd_cloud_create_exact": (_i, [_vp, _i64, _dp, _pp]),
    "glim_amd_frame_create": (_i, [_vp, _i64, _dp, _dp, _dp, _i32, _dp, _pp, _pp]),
    "glim_amd_shard_layout": (_i, [_lp, _i32, _i32, _lp, _lp, _ip, _lp]),
    "glim_amd_debug_resident_stop": (_i, [_i]),
    "glim_amd_debug_resident_stats": (_i, [_i, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _ip]),
    "glim_amd_debug_resident_post_stats": (_i, [_i, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "glim_amd_debug_deskew_table": (_i, [_i64, _dp, _dp, _i32, _dp, _dp, _d, _dp, _dp, _ip, _dp, _i32, _ip]),
    "glim_amd_cloud_deskew": (_i, [_vp, _dp, _i32, _dp, _dp, _d, _dp, _dp, _i32, _pp]),
    "glim_amd_cloud_save_compact": (_i, [_vp, C.c_char_p]),
    "glim_amd_cloud_load_compact": (_i, [_vp, C.c_char_p, _pp]),
    "glim_amd_nn_index_create": (_i, [_vp, _d, _pp]),
    "glim_amd_nn_index_destroy": (_i, [_vp]),
    "glim_amd_gicp_linearize": (_i, [_vp, _vp, _dp, _d, _u32, C.POINTER(Linearized6)]),
    "glim_amd_gicp_error": (_i, [_vp, _vp, _dp, _d, _dp, _lp]),
    "glim_amd_gicp_correspondences": (_i, [_vp, _vp, _dp, _d, _ip]),
    "glim_amd_ct_gicp_create": (_i, [_vp, _vp, _dp, _pp]),
    "glim_amd_ct_gicp_destroy": (_i, [_vp]),
    "glim_amd_ct_gicp_set_max_correspondence_distance": (_i, [_vp, _d]),
    "glim_amd_ct_gicp_linearize": (_i, [_vp, _dp, _dp, C.POINTER(CtLinearized)]),
    "glim_amd_ct_gicp_error": (_i, [_vp, _dp, _dp, _dp, _lp]),
    "glim_amd_ct_gicp_correspondences": (_i, [_vp, _dp, _dp, _ip]),
    "glim_amd_ct_gicp_deskewed_points": (_i, [_vp, _dp, _dp, _i32, _dp]),
    "glim_amd_ct_gicp_deskewed_cloud": (_i, [_vp, _dp, _dp, _i32, _pp]),
    "glim_amd_debug_ct_gicp_poses": (_i, [_vp, _dp, _dp, _ip, _i32, _dp, _dp, _dp, _dp, _ip]),
    "glim_amd_ivox_create": (_i, [_vp, _d, _pp]),
    "glim_amd_ivox_destroy": (_i, [_vp]),
    "glim_amd_ivox_set_insertion": (_i, [_vp, _d, _i32]),
    "glim_amd_ivox_set_lru": (_i, [_vp, _i32, _i32]),
    "glim_amd_ivox_set_neighbor_voxel_mode": (_i, [_vp, _i32]),
    "glim_amd_ivox_insert": (_i, [_vp, _vp, _dp]),
    "glim_amd_ivox_info": (_i, [_vp, _ip, _lp, _ip, _dp]),
    "glim_amd_ivox_download": (_i, [_vp, _ip, _ip, _fp, _fp]),
    "glim_amd_ivox_voxel_points": (_i, [_vp, _dp]),
    "glim_amd_ivox_gicp_linearize": (_i, [_vp, _vp, _dp, _d, _u32, C.POINTER(Linearized6)]),
    "glim_amd_ivox_gicp_error": (_i, [_vp, _vp, _dp, _d, _dp, _lp]),
    "glim_amd_ivox_gicp_correspondences": (_i, [_vp, _vp, _dp, _d, _lp]),
    "glim_amd_ivox_ct_factor_create": (_i, [_vp, _vp, _dp, _pp]),
    "glim_amd_debug_ivox_set_initial_capacity": (_i, [_vp, _i32]),
    "glim_amd_debug_ivox_capacity": (_i, [_vp, _ip, _ip]),
    "glim_amd_fpfh_estimate": (_i, [_vp, _d, _pp]),
    "glim_amd_fpfh_destroy": (_i, [_vp]),
    "glim_amd_fpfh_size": (_i, [_vp, _lp]),
    "glim_amd_fpfh_download": (_i, [_vp, _fp]),
    "glim_amd_fpfh_match": (_i, [_vp, _vp, _u32, _ip, _fp]),
    "glim_amd_fpfh_create": (_i, [_vp, _i64, _fp, _pp]),
    "glim_amd_ransac_default_params": (_i, [C.POINTER(RansacParams)]),
    "glim_amd_ransac_align": (_i, [_vp, _vp, _ip, C.POINTER(RansacParams), C.POINTER(RegistrationResult)]),
    "glim_amd_ransac_align_fpfh": (_i, [_vp, _vp, _vp, _vp, _u32, C.POINTER(RansacParams), C.POINTER(RegistrationResult)]),
    "glim_amd_ransac_debug_hypotheses": (_i, [_vp, _vp, _ip, C.POINTER(RansacParams), _i32, _i32, _ip, _ip, _dp, _ip, _ip, _ip]),
    "glim_amd_debug_ransac_max_lds_slots": (_i, [_i32]),
    "glim_amd_ransac_profile": (_i, [_vp, _vp, _ip, C.POINTER(RansacParams), _i, _fp, _fp, _fp, _ip, _ip]),
    "glim_amd_gnc_default_params": (_i, [C.POINTER(GncParams)]),
    "glim_amd_gnc_align": (_i, [_vp, _vp, _ip, C.POINTER(GncParams), C.POINTER(RegistrationResult), C.POINTER(GncInfo)]),
    "glim_amd_gnc_align_fpfh": (_i, [_vp, _vp, _vp, _vp, _u32, C.POINTER(GncParams), C.POINTER(RegistrationResult), C.POINTER(GncInfo)]),
    "glim_amd_gnc_debug_trace": (_i, [_vp, _vp, _ip, C.POINTER(GncParams), _i64, _ip, _lp, _dp, _dp, _dp, C.POINTER(RegistrationResult),
                                      C.POINTER(GncInfo)]),
    "glim_amd_gnc_profile": (_i, [_vp, _vp, _ip, C.POINTER(GncParams), _i, _fp, _fp, _fp, _fp, _fp]),
    "glim_amd_gicp_align_default_params": (_i, [C.POINTER(LMParams)]),
    "glim_amd_gicp_align_batch": (_i, [_pp, _pp, _dp, _dp, _i32, C.POINTER(LMParams), C.POINTER(AlignResult)]),
    "glim_amd_gicp_align_batch_incremental": (_i, [_pp, _pp, _dp, _dp, _i32, C.POINTER(LMParams), C.POINTER(AlignResult)]),
    "glim_amd_debug_gicp_align_trace": (_i, [_i32, _pp, _pp, _dp, _dp, _i32, C.POINTER(LMParams), C.POINTER(AlignResult), C.POINTER(AlignTraceEntry)]),
    "glim_amd_icp_linearize": (_i, [_vp, _vp, _dp, _d, _u32, C.POINTER(Linearized6)]),
    "glim_amd_icp_error": (_i, [_vp, _vp, _dp, _d, _u32, _dp, _lp]),
    "glim_amd_icp_align_default_params": (_i, [C.POINTER(LMParams)]),
    "glim_amd_icp_align_batch": (_i, [_pp, _pp, _dp, _dp, _u32, _i32, C.POINTER(LMParams), C.POINTER(AlignResult)]),
    "glim_amd_debug_icp_align_trace": (_i, [_pp, _pp, _dp, _dp, _u32, _i32, C.POINTER(LMParams), C.POINTER(AlignResult), C.POINTER(AlignTraceEntry), _i32]),
    "glim_amd_vgicp_align_default_params": (_i, [C.POINTER(LMParams)]),
    "glim_amd_vgicp_align_batch": (_i, [_pp, _pp, _dp, _u32, _i32, C.POINTER(LMParams), C.POINTER(AlignResult)]),
    "glim_amd_debug_vgicp_align_trace": (_i, [_pp, _pp, _dp, _u32, _i32, C.POINTER(LMParams), C.POINTER(AlignResult), C.POINTER(AlignTraceEntry)]),
    "glim_amd_keyframe_align_default_params": (_i, [C.POINTER(LMParams)]),
    "glim_amd_keyframe_align_batch": (_i, [_pp, _ip, _pp, _dp, _dp, C.POINTER(BundlePrior), _i32, _u32, _i32, C.POINTER(LMParams), C.POINTER(AlignResult), _dp]),
    "glim_amd_debug_keyframe_align_trace": (_i, [_pp, _ip, _pp, _dp, _dp, C.POINTER(BundlePrior), _i32, _u32, _i32, C.POINTER(LMParams), C.POINTER(AlignResult),
                                                 _dp, C.POINTER(AlignTraceEntry), _dp, _dp, _dp]),
    "glim_amd_ct_align_default_params": (_i, [C.POINTER(LMParams)]),
    "glim_amd_ct_align": (_i, [_vp, _dp, _dp, C.POINTER(CtAlignTerms), C.POINTER(LMParams), C.POINTER(CtAlignResult)]),
    "glim_amd_debug_ct_align_trace": (_i, [_vp, _dp, _dp, C.POINTER(CtAlignTerms), C.POINTER(LMParams), C.POINTER(CtAlignResult),
                                           C.POINTER(CtAlignTraceEntry)]),
    "glim_amd_debug_ct_align_poses": (_i, [_vp, _dp, _dp, _ip, _i32, _dp, _dp, _dp]),
    "glim_amd_bundle_align_default_params": (_i, [C.POINTER(LMParams)]),
    "glim_amd_bundle_align": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp, _i32,
                                   C.POINTER(LMParams), _dp, _dp, C.POINTER(BundleResult)]),
    "glim_amd_debug_bundle_align_trace": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp, _i32,
                                               C.POINTER(LMParams), _dp, _dp, C.POINTER(BundleResult), _i32, _dp, _dp, _dp,
                                               C.POINTER(BundleTraceRound)]),
    "glim_amd_graph_align_default_params": (_i, [C.POINTER(LMParams)]),
    "glim_amd_graph_align": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp, _i32,
                                  C.POINTER(LMParams), _dp, _dp, C.POINTER(BundleResult)]),
    "glim_amd_bundle_align_terms": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp, _i32,
                                         C.POINTER(LMParams), _dp, _dp, C.POINTER(BundleResult), C.POINTER(GraphTerms), _dp]),
    "glim_amd_graph_align_terms": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp, _i32,
                                        C.POINTER(LMParams), _dp, _dp, C.POINTER(BundleResult), C.POINTER(GraphTerms), _dp]),
    "glim_amd_debug_bundle_align_terms_trace": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp,
                                                     _i32, C.POINTER(LMParams), _dp, _dp, C.POINTER(BundleResult), C.POINTER(GraphTerms), _dp, _i32, _dp, _dp,
                                                     _dp, C.POINTER(BundleTraceRound)]),
    "glim_amd_debug_graph_align_terms_trace": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp,
                                                    _i32, C.POINTER(LMParams), _dp, _dp, C.POINTER(BundleResult), C.POINTER(GraphTerms), _dp, _i32, _dp, _dp,
                                                    _dp, C.POINTER(BundleTraceRound), _i32]),
    "glim_amd_debug_graph_align_trace": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp, _i32,
                                              C.POINTER(LMParams), _dp, _dp, C.POINTER(BundleResult), _i32, _dp, _dp, _dp,
                                              C.POINTER(BundleTraceRound), _i32]),
    "glim_amd_graph_align_nav": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp, _i32,
                                      C.POINTER(LMParams), _dp, _dp, C.POINTER(NavResult), C.POINTER(GraphTerms), _dp, C.POINTER(NavTerms)]),
    "glim_amd_debug_graph_align_nav_trace": (_i, [_vp, _pp, _pp, _ip, _ip, _i32, _u32, C.POINTER(BundlePrior), _i32, C.POINTER(BundleBetween), _i32, _dp,
                                                  _i32, C.POINTER(LMParams), _dp, _dp, C.POINTER(NavResult), C.POINTER(GraphTerms), _dp, C.POINTER(NavTerms),
                                                  _i32, _dp, _dp, _dp, C.POINTER(BundleTraceRound), _i32]),
    "glim_amd_debug_graph_solve": (_i, [_vp, _dp, _i32, C.c_double, _dp, C.POINTER(_i32)]),
    "glim_amd_ba_default_params": (_i, [C.POINTER(BaParams)]),
    "glim_amd_ba_ball_select": (_i, [_pp, _i32, _dp, _dp, _d, _i64, _ip, _lp]),
    "glim_amd_ba_ball_stats": (_i, [_pp, _i32, _dp, _dp, _d, C.POINTER(BaStats)]),
    "glim_amd_ba_auto_radius": (_i, [_pp, _i32, _dp, _dp, _d, C.POINTER(BaParams), C.POINTER(BaRadiusResult)]),
    "glim_amd_debug_ba_auto_radius_trace": (_i, [_pp, _i32, _dp, _dp, _d, C.POINTER(BaParams), C.POINTER(BaRadiusResult), C.POINTER(BaTraceEntry), _ip]),
    "glim_amd_debug_ba_eigen3": (_i, [_vp, _i32, _dp, _dp, _dp]),
    "glim_amd_debug_se3_eval": (_i, [_vp, _i32, _i32, _dp, _dp]),
    "glim_amd_ba_factor_create": (_i, [_vp, _i32, _i64, _dp, _ip, _i32, _pp]),
    "glim_amd_ba_factor_create_from_ball": (_i, [_pp, _i32, _dp, _dp, _d, _i32, _pp]),
    "glim_amd_ba_factor_info": (_i, [_vp, _ip, _lp, _ip, _ip, _dp]),
    "glim_amd_ba_factor_error": (_i, [_vp, _dp, _dp, C.POINTER(C.c_uint32)]),
    "glim_amd_ba_factor_linearize": (_i, [_vp, _dp, _dp, _dp, _dp, C.POINTER(C.c_uint32)]),
    "glim_amd_ba_factor_destroy": (_i, [_vp]),
    "glim_amd_edit_select": (_i, [_pp, _i32, _dp, _i32, C.POINTER(EditWindow), _d, _i64, _ip, _lp]),
    "glim_amd_edit_select_outliers": (_i, [_pp, _i32, _dp, C.POINTER(EditWindow), _d, C.POINTER(EditOutlierParams), _i64, _ip, _lp, _ip]),
    "glim_amd_edit_region_grow": (_i, [_pp, _i32, _dp, C.POINTER(EditWindow), C.POINTER(EditRegionGrowingParams), _i64, _ip, _ip,
                                       C.POINTER(EditRegionResult)]),
    "glim_amd_edit_remove_points": (_i, [_vp, _i64, _ip, _pp]),
    "glim_amd_edit_min_cut": (_i, [_pp, _i32, _dp, C.POINTER(EditWindow), C.POINTER(EditMinCutParams), _i64, _ip, C.POINTER(EditMinCutResult)]),
    "glim_amd_diag_edit_min_cut_graph": (_i, [_pp, _i32, _dp, C.POINTER(EditWindow), C.POINTER(EditMinCutParams), _i64, _ip, _ip, _ip, _i64, _ip, _ip,
                                              C.POINTER(EditMinCutResult)]),
    "glim_amd_diag_max_flow": (_i, [_vp, _i32, _i64, _ip, _ip, _ip, _ip, _i32, _ip, _lp, _ip, _ip, _ip]),
    "glim_amd_merge_frames":(_i, [_vp, _i32, _dp, C.POINTER(_dp), C.POINTER(_dp), _lp, _d, _i32, _i32, C.c_uint64, _pp]),
    "glim_amd_cloud_download_merged": (_i, [_vp, _dp, _dp]),
    "glim_amd_debug_sort_pairs": (_i, [_vp, _i64, _i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "glim_amd_debug_exclusive_scan": (_i, [_vp, _i64, _ip, _ip]),
    "glim_amd_cloud_random_sample": (_i, [_vp, _d, C.c_uint64, _pp]),
    "glim_amd_cloud_sample": (_i, [_vp, _i64, _ip, _pp]),
    "glim_amd_cloud_transform": (_i, [_vp, _dp, _pp]),
    "glim_amd_debug_select_smallest": (_i, [_vp, _i64, C.POINTER(C.c_uint32), _i64, _ip]),
    "glim_amd_cloud_destroy": (_i, [_vp]),
    "glim_amd_cloud_size": (_i, [_vp, _lp]),
    "glim_amd_cloud_memory_usage": (_i, [_vp, C.POINTER(_sz)]),
    "glim_amd_cloud_download": (_i, [_vp, _fp, _fp, _fp, _ip]),
    "glim_amd_cloud_find_neighbors": (_i, [_vp, _i, _ip]),
    "glim_amd_cloud_set_neighbors": (_i, [_vp, _i, _ip]),
    "glim_amd_cloud_estimate_covariances": (_i, [_vp, _i]),
    "glim_amd_voxelmap_create": (_i, [_vp, _d, _i, _i, _d, _pp]),
    "glim_amd_voxelmap_insert": (_i, [_vp, _vp]),
    "glim_amd_voxelmap_destroy": (_i, [_vp]),
    "glim_amd_voxelmap_info": (_i, [_vp, _ip, _ip, _dp, C.POINTER(_sz)]),
    "glim_amd_voxelmap_download": (_i, [_vp, _ip, _ip, _fp, _fp]),
    "glim_amd_factor_set_create": (_i, [_vp, _pp]),
    "glim_amd_factor_set_destroy": (_i, [_vp]),
    "glim_amd_factor_set_add": (_i, [_vp, _vp, _vp, _u32, _ip]),
    "glim_amd_factor_set_clear": (_i, [_vp]),
    "glim_amd_factor_set_size": (_i, [_vp, _ip]),
    "glim_amd_factor_set_linearize": (_i, [_vp, _dp, C.POINTER(Linearized6)]),
    "glim_amd_factor_set_error": (_i, [_vp, _dp, _dp, _dp, _lp]),
    "glim_amd_factor_set_correspondences": (_i, [_vp, _i32, _dp, _ip]),
    "glim_amd_factor_set_linearize_device_async": (_i, [_vp, _dp, _vp, _i64]),
    "glim_amd_expand_compact": (_i, [_dp, _dp, _u32, C.POINTER(Linearized6)]),
    "glim_amd_factor_set_profile": (_i, [_vp, _dp, _i, _fp, _fp]),
    "glim_amd_factor_set_profile_sync": (_i, [_vp, _dp, _i, _fp]),
    "glim_amd_factor_set_profile_lm": (_i, [_vp, _dp, _i, _fp, _fp]),
    "glim_amd_overlap": (_i, [_vp, _i32, _pp, _dp, _vp, _dp]),
    "glim_amd_overlap_batch": (_i, [_vp, _i32, _ip, _pp, _dp, _pp, _dp]),
    "glim_amd_overlap_profile": (_i, [_vp, _i32, _ip, _pp, _dp, _pp, _i, _fp]),
    "glim_amd_factor_set_profile_fresh": (_i, [_vp, _i32, _pp, _pp, C.POINTER(C.c_uint32), _dp, _i, _fp]),
    "glim_amd_multi_create": (_i, [_ip, _i32, _pp]),
    "glim_amd_multi_destroy": (_i, [_vp]),
    "glim_amd_multi_info": (_i, [_vp, _ip, _ip, _lp]),
    "glim_amd_multi_add_cloud": (_i, [_vp, _i64, _dp, _dp, _dp, _ip]),
    "glim_amd_multi_add_cloud_f32": (_i, [_vp, _i64, _fp, _fp, _fp, _ip]),
    "glim_amd_multi_cloud_estimate_covariances": (_i, [_vp, _i32, _i]),
    "glim_amd_multi_add_voxelmap": (_i, [_vp, _i32, _d, _ip]),
    "glim_amd_multi_set_factors": (_i, [_vp, _i64, _ip, _ip, C.POINTER(C.c_uint32)]),
    "glim_amd_multi_shard": (_i, [_vp, _lp]),
    "glim_amd_multi_linearize": (_i, [_vp, _dp, C.POINTER(Linearized6), _dp]),
    "glim_amd_multi_profile": (_i, [_vp, _dp, _i, _fp]),
    "glim_amd_shard_bounds": (_i, [_dp, _i64, _i32, _lp]),
    "glim_amd_debug_scratch_poke": (_i, [_vp, _i32, _u32]),
    "glim_amd_debug_resident_timeline": (_i, [_i, _i, _dp, _i32]),
    "glim_amd_cloud_profile_neighbors": (_i, [_vp, _i, _i, _fp, _fp]),
    "glim_amd_multi_set_gather_mode": (_i, [_vp, _i32]),
    "glim_amd_multi_wait_gather": (_i, [_vp]),
    "glim_amd_multi_gathered_device": (_i, [_vp, _i32, _pp, _lp]),
    "glim_amd_debug_multi_create_virtual": (_i, [_ip, _i32, _pp]),
    "glim_amd_debug_multi_inject_failure": (_i, [_vp, _i32, _i32]),
    "glim_amd_debug_multi_set_diag": (_i, [_vp, C.c_char_p]),
    "glim_amd_debug_multi_gathered_download": (_i, [_vp, _i32, _i64, _i64, _dp]),
}

_lib = None


def lib():
    """Load libglim_amd.so; raises (never falls back) when it is missing or lacks a declared symbol."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
                "or make -C glim_amd/csrc).  glim_amd has no CPU fallback."
            )
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared entry point
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code, where):
    if code != 0:
        detail = lib().glim_amd_last_hip_error().decode() if code == -2 else ""
        raise GlimAmdError(code, where, detail)
