"""ctypes mirror of include/dcreg.h (the C-ABI of libdcreg_hip.so).

Python is plumbing here: tests, bench.py and multi-GPU launch use this thin binding; the product is the
shared library.  There is no CPU fallback: creating a Context without a usable HIP device raises.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCREG_LIB") or os.path.join(_HERE, "lib", "libdcreg_hip.so")   # DCREG_LIB: an experiment variant (build.py)

# enum values of DCReg/include/utils.hpp:106-121
DETECTION = {"NONE_DETE": 0, "SCHUR_CONDITION_NUMBER": 1, "FULL_EVD_MIN_EIGENVALUE": 2,
             "EVD_SUB_CONDITION": 3, "FULL_SVD_CONDITION": 4}
HANDLING = {"NONE_HAND": 0, "STANDARD_REGULARIZATION": 1, "ADAPTIVE_REGULARIZATION": 2,
            "PRECONDITIONED_CG": 3, "SOLUTION_REMAPPING": 4, "TRUNCATED_SVD": 5}
# method-name dispatch of the YAML test_methods section (DCReg/config/icp.yaml:101-116)
METHODS = {
    "ME-SR": ("FULL_EVD_MIN_EIGENVALUE", "SOLUTION_REMAPPING"),
    "ME-TSVD": ("FULL_EVD_MIN_EIGENVALUE", "TRUNCATED_SVD"),
    "ME-TReg": ("FULL_EVD_MIN_EIGENVALUE", "STANDARD_REGULARIZATION"),
    "FCN-SR": ("FULL_SVD_CONDITION", "SOLUTION_REMAPPING"),
    "Ours": ("SCHUR_CONDITION_NUMBER", "PRECONDITIONED_CG"),
    "NONE": ("NONE_DETE", "NONE_HAND"),
}

OK, E_INVALID, E_NOMEM, E_DEVICE, E_STATE = 0, -1, -2, -3, -4
# DCREG_ROBUST_* of include/dcreg.h ("robust kernels": the second and third engine's rows)
ROBUST = {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3}
ROBUST_SCALE_RANGE = (1.0e-6, 1.0e6)


class LinParams(C.Structure):
    _fields_ = [("search_radius", C.c_double), ("max_plane_thickness_sq", C.c_double),
                ("min_normal_norm", C.c_double), ("weight_slope", C.c_double), ("weight_min", C.c_double),
                ("use_weight_derivative", C.c_int), ("k", C.c_int), ("parameterization", C.c_int), ("reserved_", C.c_int),
                ("euler_rpy", C.c_double * 3)]


class LinOut(C.Structure):
    _fields_ = [("H_upper", C.c_double * 21), ("g", C.c_double * 6), ("sum_r2", C.c_double),
                ("sum_b2", C.c_double), ("n_eff", C.c_int64), ("n_pt", C.c_int64)]


class LinDebug(C.Structure):
    _fields_ = [("nn_idx", C.POINTER(C.c_int32)), ("nn_d2", C.POINTER(C.c_float)),
                ("flag", C.POINTER(C.c_uint8)), ("normal", C.POINTER(C.c_double)),
                ("r", C.POINTER(C.c_double)), ("s", C.POINTER(C.c_double)), ("stats", C.POINTER(C.c_uint32)),
                ("stamps", C.POINTER(C.c_uint64))]


class NlinDebug(C.Structure):      # dcreg_nlin_debug: the per-point dump of dcreg_linearize_normals_debug
    _fields_ = [("nn_idx", C.POINTER(C.c_int32)), ("nn_d2", C.POINTER(C.c_float)), ("flag", C.POINTER(C.c_uint8)),
                ("normal", C.POINTER(C.c_double)), ("r", C.POINTER(C.c_double)), ("s", C.POINTER(C.c_double)),
                ("row", C.POINTER(C.c_double))]


class GlinDebug(C.Structure):      # dcreg_glin_debug: the per-point dump of dcreg_linearize_gicp_debug
    _fields_ = [("nn_idx", C.POINTER(C.c_int32)), ("nn_d2", C.POINTER(C.c_float)), ("flag", C.POINTER(C.c_uint8)),
                ("normal_map", C.POINTER(C.c_double)), ("normal_src", C.POINTER(C.c_double)), ("w", C.POINTER(C.c_double)),
                ("r", C.POINTER(C.c_double)), ("row", C.POINTER(C.c_double))]


class VlinDebug(C.Structure):      # dcreg_vlin_debug: the per-point dump of dcreg_linearize_voxels_debug
    _fields_ = [("voxel_idx", C.POINTER(C.c_int32)), ("flag", C.POINTER(C.c_uint8)), ("mean", C.POINTER(C.c_double)),
                ("cov", C.POINTER(C.c_double)), ("normal_src", C.POINTER(C.c_double)), ("w", C.POINTER(C.c_double)),
                ("r", C.POINTER(C.c_double)), ("row", C.POINTER(C.c_double))]


class VoxelMapParams(C.Structure):     # dcreg_voxel_map_params
    _fields_ = [("leaf", C.c_double), ("epsilon", C.c_double), ("min_points", C.c_int), ("reserved_", C.c_int)]


class VoxelMapInfo(C.Structure):       # dcreg_voxel_map_info
    _fields_ = [("n_points", C.c_int64), ("n_voxels", C.c_int64), ("n_small", C.c_int64), ("n_degenerate", C.c_int64), ("n_kept", C.c_int64)]


class VoxelsFollowInfo(C.Structure):   # dcreg_voxels_follow_info
    _fields_ = [("n_target", C.c_int64), ("n_touched", C.c_int64), ("n_refit", C.c_int64), ("n_carried", C.c_int64), ("n_kept", C.c_int64),
                ("followed", C.c_int), ("reserved_", C.c_int)]


class LaunchStats(C.Structure):
    _fields_ = [("launches", C.c_int64), ("poses", C.c_int64), ("points", C.c_int64), ("points_searched", C.c_int64),
                ("points_team", C.c_int64)]


class MethodStats(C.Structure):
    _fields_ = [("total_runs", C.c_int64), ("converged_runs", C.c_int64), ("success_rate", C.c_double),
                ("mean_trans_error", C.c_double), ("std_trans_error", C.c_double), ("min_trans_error", C.c_double), ("max_trans_error", C.c_double),
                ("mean_rot_error", C.c_double), ("std_rot_error", C.c_double), ("min_rot_error", C.c_double), ("max_rot_error", C.c_double),
                ("mean_time_ms", C.c_double), ("std_time_ms", C.c_double),
                ("mean_iterations", C.c_double), ("mean_rmse", C.c_double), ("mean_fitness", C.c_double),
                ("corr_num", C.c_int64), ("iterations_total", C.c_int64), ("ranks_seen", C.c_int), ("world", C.c_int)]


class IndexInfo(C.Structure):
    _fields_ = [("cell", C.c_double), ("origin", C.c_double * 3), ("dims", C.c_int32 * 3),
                ("n_cells", C.c_int64), ("n_target", C.c_int64), ("n_source", C.c_int64),
                ("max_ring", C.c_int32)]


class Config(C.Structure):
    _fields_ = [("search_radius", C.c_double), ("max_iterations", C.c_int),
                ("CONVERGENCE_THRESH_ROT", C.c_double), ("CONVERGENCE_THRESH_TRANS", C.c_double),
                ("DEGENERACY_THRES_COND", C.c_double), ("DEGENERACY_THRES_EIG", C.c_double),
                ("KAPPA_TARGET", C.c_double), ("PCG_TOLERANCE", C.c_double), ("PCG_MAX_ITER", C.c_int),
                ("STD_REG_GAMMA", C.c_double), ("ADAPTIVE_REG_ALPHA", C.c_double),
                ("use_weight_derivative", C.c_int), ("always_compute_schur", C.c_int),
                ("euler_exact_jacobian", C.c_int), ("reserved_cfg_", C.c_int),
                ("gt_matrix", C.c_double * 16)]


class Analysis(C.Structure):
    _fields_ = [("isDegenerate", C.c_int), ("degenerate_mask", C.c_int * 6),
                ("cond_schur_rot", C.c_double), ("cond_schur_trans", C.c_double),
                ("cond_diag_rot", C.c_double), ("cond_diag_trans", C.c_double),
                ("cond_full", C.c_double), ("cond_full_sub_rot", C.c_double),
                ("cond_full_sub_trans", C.c_double), ("eigenvalues_full", C.c_double * 6),
                ("eigenvectors_full", C.c_double * 36), ("singular_values", C.c_double * 6),
                ("lambda_schur_rot", C.c_double * 3), ("lambda_schur_trans", C.c_double * 3),
                ("lambda_sub_rot", C.c_double * 3), ("lambda_sub_trans", C.c_double * 3),
                ("schur_V_rot", C.c_double * 9), ("schur_V_trans", C.c_double * 9),
                ("aligned_V_rot", C.c_double * 9), ("aligned_V_trans", C.c_double * 9),
                ("rot_indices", C.c_int * 3), ("trans_indices", C.c_int * 3),
                ("P_preconditioner", C.c_double * 36), ("W_adaptive", C.c_double * 36),
                ("pcg_iterations", C.c_int)]


class IterLog(C.Structure):
    _fields_ = [("iter_count", C.c_int), ("effective_points", C.c_int64), ("corr_pt_count", C.c_int64),
                ("rmse", C.c_double), ("fitness", C.c_double), ("objective_value", C.c_double),
                ("gradient", C.c_double * 6), ("update_dx", C.c_double * 6),
                ("transform_matrix", C.c_double * 16), ("trans_error_vs_gt", C.c_double),
                ("rot_error_vs_gt", C.c_double), ("iter_time_ms", C.c_double),
                ("H_upper", C.c_double * 21), ("analysis", Analysis)]


class IcpResult(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("status", C.c_int),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("icp_cov", C.c_double * 36),
                ("time_ms", C.c_double)]


class TrialResult(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("status", C.c_int),
                ("time_ms", C.c_double), ("trans_error_m", C.c_double), ("rot_error_deg", C.c_double),
                ("final_rmse", C.c_double), ("final_fitness", C.c_double), ("corr_num", C.c_int64),
                ("final_transform", C.c_double * 16), ("H_upper", C.c_double * 21),
                ("degenerate_mask", C.c_int * 6)]


_STRUCTS = {"dcreg_lin_params": LinParams, "dcreg_lin_out": LinOut, "dcreg_lin_debug": LinDebug,
            "dcreg_index_info": IndexInfo, "dcreg_config": Config, "dcreg_analysis": Analysis,
            "dcreg_iter_log": IterLog, "dcreg_icp_result": IcpResult, "dcreg_trial_result": TrialResult,
            "dcreg_launch_stats": LaunchStats, "dcreg_method_stats": MethodStats, "dcreg_nlin_debug": NlinDebug,
            "dcreg_glin_debug": GlinDebug, "dcreg_vlin_debug": VlinDebug, "dcreg_voxel_map_params": VoxelMapParams,
            "dcreg_voxel_map_info": VoxelMapInfo, "dcreg_voxels_follow_info": VoxelsFollowInfo}
# (VoxelParams / VoxelInfo are defined below and join _STRUCTS there)

# every symbol include/dcreg.h and include/dcreg_debug.h declare
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_void_p)      # dcreg_reduce_fn

EXPORTS = [
    "dcreg_backend_create", "dcreg_backend_destroy", "dcreg_last_error", "dcreg_set_stream", "dcreg_set_option",
    "dcreg_set_target", "dcreg_set_target_device", "dcreg_set_source", "dcreg_set_source_device",
    "dcreg_target_insert", "dcreg_target_insert_device", "dcreg_target_insert_source", "dcreg_target_crop", "dcreg_target_get",
    "dcreg_debug_index_check",
    "dcreg_default_lin_params", "dcreg_linearize", "dcreg_linearize_batch", "dcreg_linearize_batch_begin",
    "dcreg_linearize_batch_end", "dcreg_linearize_batch_begin_warm", "dcreg_reserve_warm_states", "dcreg_reset_warm_state", "dcreg_hint_misalignment", "dcreg_linearize_debug", "dcreg_launch_stats_get", "dcreg_knn", "dcreg_kdtree_build", "dcreg_kdtree_info", "dcreg_knn_timed",
    "dcreg_linearize_gated_begin", "dcreg_linearize_gate_open", "dcreg_linearize_gate_abort",
    "dcreg_index_info_get", "dcreg_kernel_time", "dcreg_launch_series", "dcreg_launch_series_passes", "dcreg_launch_series_structure", "dcreg_team_pass_stamps", "dcreg_roi_info", "dcreg_default_config", "dcreg_analyze_degeneracy", "dcreg_analyze_degeneracy_two_part",
    "dcreg_solve_degenerate_system", "dcreg_unpack_hessian", "dcreg_boxplus", "dcreg_pose6d_to_matrix",
    "dcreg_pose_error", "dcreg_icp_run", "dcreg_icp_run_sharded", "dcreg_icp_run_many", "dcreg_icp_run_euler", "dcreg_icp_run_trials", "dcreg_icp_run_montecarlo", "dcreg_p2p_error", "dcreg_sizeof", "dcreg_version", "dcreg_trial_pose",
    "dcreg_set_host_threads", "dcreg_get_host_threads", "dcreg_comm_unique_id", "dcreg_comm_init", "dcreg_comm_destroy", "dcreg_comm_allgather_sum", "dcreg_icp_run_sharded_rccl",
    "dcreg_montecarlo_job", "dcreg_comm_allgather", "dcreg_comm_info", "dcreg_set_error_message",
    "dcreg_register_frames", "dcreg_frames_load", "dcreg_frames_reserve_states", "dcreg_frames_reset_state", "dcreg_frames_batch_begin",
    "dcreg_register_pairs", "dcreg_pairs_plan", "dcreg_pairs_sources_load", "dcreg_pairs_build", "dcreg_pairs_reserve_states",
    "dcreg_pairs_reset_state", "dcreg_pairs_batch_begin",
    "dcreg_voxel_downsample", "dcreg_voxel_downsample_device", "dcreg_set_source_voxel", "dcreg_set_source_voxel_device",
    "dcreg_set_target_voxel", "dcreg_set_target_voxel_device",
    "dcreg_deskew", "dcreg_deskew_device", "dcreg_set_source_deskew", "dcreg_set_source_deskew_device",
    "dcreg_deskew_path", "dcreg_deskew_path_device", "dcreg_set_source_deskew_path", "dcreg_set_source_deskew_path_device",
    "dcreg_default_place_params", "dcreg_place_descriptors", "dcreg_place_descriptors_device", "dcreg_places_reset", "dcreg_places_count",
    "dcreg_places_add", "dcreg_places_add_clouds", "dcreg_places_add_clouds_device", "dcreg_places_add_source", "dcreg_places_get",
    "dcreg_places_query", "dcreg_places_query_clouds", "dcreg_places_query_clouds_device", "dcreg_places_query_source",
    "dcreg_default_outlier_params", "dcreg_outlier_filter", "dcreg_outlier_filter_device", "dcreg_set_source_outliers",
    "dcreg_set_source_outliers_device", "dcreg_set_target_outliers", "dcreg_set_target_outliers_device", "dcreg_target_remove_outliers",
    "dcreg_keyframes_reset", "dcreg_keyframes_count", "dcreg_keyframes_sizes", "dcreg_keyframes_add_clouds", "dcreg_keyframes_add_clouds_device",
    "dcreg_keyframes_add_source", "dcreg_keyframes_get", "dcreg_keyframes_submaps", "dcreg_keyframes_submaps_device", "dcreg_set_target_keyframes",
    "dcreg_default_visibility_params", "dcreg_keyframes_range_images", "dcreg_keyframes_range_images_device", "dcreg_visibility_filter",
    "dcreg_visibility_filter_device", "dcreg_target_remove_dynamic",
    "dcreg_default_normal_params", "dcreg_normals", "dcreg_normals_device", "dcreg_target_normals", "dcreg_target_normals_device",
    "dcreg_target_normals_keep", "dcreg_target_normals_set", "dcreg_target_normals_set_device", "dcreg_target_normals_kept",
    "dcreg_target_normals_drop", "dcreg_linearize_normals", "dcreg_linearize_normals_debug", "dcreg_icp_run_normals",
    "dcreg_register_frames_normals", "dcreg_icp_run_trials_normals", "dcreg_normals_reserve_slots", "dcreg_normals_reset_slot",
    "dcreg_normals_batch_begin", "dcreg_normals_batch_end",
    "dcreg_target_normals_get", "dcreg_target_normals_get_device", "dcreg_target_normals_follow_info",
    "dcreg_source_normals_keep", "dcreg_source_normals_set", "dcreg_source_normals_set_device", "dcreg_source_normals_get",
    "dcreg_source_normals_get_device", "dcreg_source_normals_kept", "dcreg_source_normals_drop", "dcreg_linearize_gicp",
    "dcreg_linearize_gicp_debug", "dcreg_icp_run_gicp",
    "dcreg_normals_clouds", "dcreg_normals_clouds_device", "dcreg_frames_normals_keep", "dcreg_frames_normals_set", "dcreg_frames_normals_kept",
    "dcreg_gicp_batch_begin", "dcreg_gicp_batch_end", "dcreg_normal_params_check", "dcreg_register_frames_gicp", "dcreg_icp_run_trials_gicp",
    "dcreg_register_pairs_normals", "dcreg_register_pairs_gicp", "dcreg_pairs_plan_normals", "dcreg_pairs_normals_keep", "dcreg_pairs_normals_set",
    "dcreg_pairs_normals_get", "dcreg_pairs_normals_kept", "dcreg_pairs_sources_normals_keep", "dcreg_pairs_sources_normals_set",
    "dcreg_pairs_sources_normals_get", "dcreg_pairs_normals_reserve_slots", "dcreg_pairs_normals_batch_begin", "dcreg_pairs_gicp_batch_begin",
    "dcreg_default_voxel_map_params", "dcreg_target_voxels_keep", "dcreg_target_voxels_get", "dcreg_target_voxels_kept", "dcreg_target_voxels_drop",
    "dcreg_target_voxels_follow_info",
    "dcreg_linearize_voxels", "dcreg_linearize_voxels_debug", "dcreg_icp_run_voxels",
    "dcreg_voxels_batch_begin", "dcreg_voxels_batch_end", "dcreg_register_frames_voxels", "dcreg_icp_run_trials_voxels",
    "dcreg_register_pairs_voxels", "dcreg_pairs_plan_voxels", "dcreg_pairs_voxels_build", "dcreg_pairs_voxels_get", "dcreg_pairs_voxels_kept",
    "dcreg_voxel_map_params_check", "dcreg_pairs_voxels_box_check", "dcreg_pairs_voxels_batch_begin",
    "dcreg_default_fpfh_params", "dcreg_fpfh", "dcreg_fpfh_device", "dcreg_target_fpfh", "dcreg_target_fpfh_device", "dcreg_fpfh_debug_counts",
    "dcreg_feature_match", "dcreg_feature_match_device",
    "dcreg_default_fpfh_radius_params", "dcreg_fpfh_radius", "dcreg_fpfh_radius_device", "dcreg_target_fpfh_radius", "dcreg_target_fpfh_radius_device",
    "dcreg_fpfh_radius_debug_counts",
    "dcreg_default_align_params", "dcreg_align_correspondences", "dcreg_align_correspondences_device",
    "dcreg_default_consensus_params", "dcreg_consensus_correspondences", "dcreg_consensus_correspondences_device",
    "dcreg_default_verify_params", "dcreg_verify_poses", "dcreg_verify_poses_cloud", "dcreg_verify_poses_cloud_device",
]

_lib = None


def _frames_arg(frames, what):
    """frames as register_frames takes them -> (xyz [N, c] float32, offsets [n + 1] int64, n)"""
    if isinstance(frames, tuple):
        xyz, off = frames
        xyz = _points(xyz, what)
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
    else:
        parts = [_points(f, what) for f in frames]
        if len({f.shape[1] for f in parts}) > 1:
            raise ValueError("%s: every frame needs the same number of columns, got %s" % (what, sorted({f.shape[1] for f in parts})))
        off = np.zeros(len(parts) + 1, np.int64)
        off[1:] = np.cumsum([len(f) for f in parts])
        xyz = np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.float32))
    if len(off) < 1:
        raise ValueError("%s: offsets need at least one entry" % what)
    return xyz, off, len(off) - 1


def _pose_arg(T, what=None):
    """a 4 x 4 pose -> (R [9], t [3]); what: the wrapper that refuses anything but a finite 4 x 4 itself (None: reshaped, the C side checks)"""
    T = _f64(T)
    if what is None:
        T = T.reshape(4, 4)
    elif T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("%s: a finite 4 x 4 pose is expected" % what)
    return np.ascontiguousarray(T[:3, :3]).reshape(9), np.ascontiguousarray(T[:3, 3])


def _poses_arg(Ts):
    """[n, 4, 4] poses -> (R [n, 9], t [n, 3], n)"""
    Ts = _f64(Ts).reshape(-1, 4, 4)
    n = Ts.shape[0]
    return np.ascontiguousarray(Ts[:, :3, :3]).reshape(n, 9), np.ascontiguousarray(Ts[:, :3, 3]).reshape(n, 3), n


def _method(method, what=None):
    """a name of METHODS or a (detection, handling) pair -> the two C enums; what: the wrapper that refuses an unknown name itself"""
    if what is not None and isinstance(method, str) and method not in METHODS:
        raise ValueError("%s: unknown method %r" % (what, method))
    det, hand = METHODS[method] if isinstance(method, str) else method
    return DETECTION[det], HANDLING[hand]


# the per-point dumps of linearize_normals / linearize_gicp: (key, dtype, shape per point) of every array of the C struct
_DUMP_FILL = {"nn_idx": -1, "nn_d2": np.inf, "voxel_idx": -1}
_NLIN_DUMP = [("nn_idx", np.int32, ()), ("nn_d2", np.float32, ()), ("flag", np.uint8, ()), ("normal", np.float64, (3,)), ("r", np.float64, ()),
              ("s", np.float64, ()), ("row", np.float64, (8,))]
_GLIN_DUMP = [("nn_idx", np.int32, ()), ("nn_d2", np.float32, ()), ("flag", np.uint8, ()), ("normal_map", np.float64, (3,)),
              ("normal_src", np.float64, (3,)), ("w", np.float64, (3, 3)), ("r", np.float64, (3,)), ("row", np.float64, (3, 8))]


_VLIN_DUMP = [("voxel_idx", np.int32, ()), ("flag", np.uint8, ()), ("mean", np.float64, (3,)), ("cov", np.float64, (6,)),
              ("normal_src", np.float64, (3,)), ("w", np.float64, (3, 3)), ("r", np.float64, (3,)), ("row", np.float64, (3, 8))]


def _dump_arg(n, entries, struct):
    """-> ({key: array of n points}, the ctypes struct that points at them)"""
    keep = {k: np.full((n,) + shape, _DUMP_FILL.get(k, 0), dtype) for k, dtype, shape in entries}
    return keep, struct(**{k: keep[k].ctypes.data_as(t) for k, t in struct._fields_})


class MapUpdate(C.Structure):
    _fields_ = [("n_offered", C.c_int64), ("n_added", C.c_int64), ("n_removed", C.c_int64), ("n_target", C.c_int64), ("rebuilt", C.c_int),
                ("reserved_", C.c_int)]


class VoxelParams(C.Structure):
    _fields_ = [("leaf", C.c_double * 3), ("mode", C.c_int), ("min_points", C.c_int)]


class VoxelInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_finite", C.c_int64), ("n_voxels", C.c_int64), ("n_out", C.c_int64)]


_STRUCTS.update({"dcreg_voxel_params": VoxelParams, "dcreg_voxel_info": VoxelInfo})
VOXEL_MODES = {"centroid": 0, "first": 1}      # DCREG_VOXEL_CENTROID / DCREG_VOXEL_FIRST


def voxel_params(leaf, mode="centroid", min_points=1):
    """dcreg_voxel_params of a leaf (one edge for a cubic voxel, or three), a mode name and PCL's minimum points per voxel"""
    lf = np.asarray(leaf, dtype=np.float64).reshape(-1)
    if lf.size == 1:
        lf = np.repeat(lf, 3)
    if lf.size != 3:
        raise ValueError("voxel leaf: one edge or three are expected, got %d values" % lf.size)
    if not np.all(np.isfinite(lf)) or not np.all(lf > 0.0):
        raise ValueError("voxel leaf: finite edges > 0 are expected, got %s" % (lf.tolist(),))
    if mode not in VOXEL_MODES:
        raise ValueError("voxel mode: one of %s is expected, got %r" % (sorted(VOXEL_MODES), mode))
    p = VoxelParams()
    for a in range(3):
        p.leaf[a] = float(lf[a])
    p.mode = VOXEL_MODES[mode]
    p.min_points = int(min_points)
    return p


def _voxel_info_dict(i):
    return {"n_in": i.n_in, "n_finite": i.n_finite, "n_voxels": i.n_voxels, "n_out": i.n_out}


class TimeField(C.Structure):
    _fields_ = [("column", C.c_int), ("type", C.c_int), ("scale", C.c_double)]


class SweepMotion(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("t_begin", C.c_double), ("t_end", C.c_double), ("ref", C.c_double),
                ("span_from_data", C.c_int), ("reserved_", C.c_int)]


class DeskewInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_finite", C.c_int64), ("n_outside", C.c_int64), ("t_min", C.c_double), ("t_max", C.c_double)]


class SweepPath(C.Structure):
    _fields_ = [("first_knot", C.c_int64), ("n_knots", C.c_int), ("reserved_", C.c_int), ("t_ref", C.c_double), ("ext_R", C.c_double * 9),
                ("ext_t", C.c_double * 3)]


_STRUCTS.update({"dcreg_time_field": TimeField, "dcreg_sweep_motion": SweepMotion, "dcreg_deskew_info": DeskewInfo,
                 "dcreg_sweep_path": SweepPath})
_SWEEP_PATH_DTYPE = np.dtype([("first_knot", np.int64), ("n_knots", np.int32), ("reserved_", np.int32), ("t_ref", np.float64),
                              ("ext_R", np.float64, (3, 3)), ("ext_t", np.float64, 3)])
TIME_TYPES = {"f32": 0, "f64": 1, "u32": 2, "u64": 3}      # DCREG_TIME_F32 / _F64 / _U32 / _U64


def se3_exp(xi):
    """SE(3) exponential of xi = (w, v) as include/dcreg.h defines it (series through theta^4 below theta = 1e-3) -> 4x4"""
    xi = np.asarray(xi, np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-3:
        A, B, Cc = 1 - th2 / 6 + th2 * th2 / 120, 0.5 - th2 / 24 + th2 * th2 / 720, 1 / 6 - th2 / 120 + th2 * th2 / 5040
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    W2 = W @ W
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * W + B * W2
    T[:3, 3] = (np.eye(3) + B * W + Cc * W2) @ v
    return T


def se3_log(T):
    """inverse of se3_exp for rotations below pi (angle-axis of R, then v = V^-1 t) -> xi = (w, v)"""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.linalg.norm(s)
    th = np.arctan2(sn, 0.5 * (np.trace(R) - 1.0))
    th2 = th * th
    w = s * (1 + th2 / 6 + 7 * th2 * th2 / 360 if th < 1e-3 else th / sn)
    if th < 1e-3:
        D = 1 / 12 + th2 / 720 + th2 * th2 / 30240
    else:
        A, B = np.sin(th) / th, (1 - np.cos(th)) / th2
        D = (1 - A / (2 * B)) / th2
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.r_[w, (np.eye(3) - 0.5 * W + D * (W @ W)) @ t]


def constant_velocity_motion(T_prev, T_last, ratio=1.0):
    """the motion of the next sweep predicted from the last two registered poses (4x4, sensor -> map): Exp(ratio Log(T_prev^-1 T_last))"""
    d = np.linalg.inv(np.asarray(T_prev, np.float64).reshape(4, 4)) @ np.asarray(T_last, np.float64).reshape(4, 4)
    return se3_exp(float(ratio) * se3_log(d))


def _check_field(f, stride, what):
    if not isinstance(f, TimeField):
        raise ValueError("%s: a time_field is expected, got %r" % (what, type(f).__name__))
    if f.type not in TIME_TYPES.values():
        raise ValueError("%s: unknown time type %r" % (what, f.type))
    wide = f.type in (TIME_TYPES["f64"], TIME_TYPES["u64"])
    if f.column < 3 or (stride is not None and (f.column >= stride or (wide and f.column + 1 >= stride))):
        raise ValueError("%s: time column %d outside [3, %s)%s" % (what, f.column, stride, " (a 64-bit stamp takes two slots)" if wide else ""))
    if not (np.isfinite(f.scale) and f.scale > 0.0):
        raise ValueError("%s: time scale %r: finite and > 0 expected" % (what, f.scale))


def _check_motion(m, what):
    """the library's refusals of one motion, in plain Python (a call checks one per cloud: numpy's per-call overhead would dominate)"""
    if not isinstance(m, SweepMotion):
        raise ValueError("%s: a sweep_motion is expected, got %r" % (what, type(m).__name__))
    R, t = m.R[:], m.t[:]
    if not all(math.isfinite(v) for v in R + t):
        raise ValueError("%s: the motion is not finite" % what)
    det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6])
    if not det > 0.0 or any(not abs(R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j)) <= 1e-6 for i in range(3) for j in range(3)):
        raise ValueError("%s: R is not a rotation (|R^T R - I| > 1e-6 or det <= 0)" % what)
    sn = 0.5 * math.sqrt((R[7] - R[5]) ** 2 + (R[2] - R[6]) ** 2 + (R[3] - R[1]) ** 2)
    if not math.atan2(sn, 0.5 * (R[0] + R[4] + R[8] - 1.0)) < math.pi / 2:
        raise ValueError("%s: the motion rotates by pi/2 or more over the sweep" % what)
    if not m.span_from_data and not (np.isfinite(m.t_begin) and np.isfinite(m.t_end) and m.t_end >= m.t_begin):
        raise ValueError("%s: span [%r, %r] is not finite and ordered" % (what, m.t_begin, m.t_end))
    if not (0.0 <= m.ref <= 1.0):
        raise ValueError("%s: ref %r outside [0, 1]" % (what, m.ref))


def time_field(column, type="f32", scale=1.0):
    """dcreg_time_field: the stamp at float slot `column` (>= 3) of every record, of type "f32", "f64", "u32" or "u64" (the 64-bit types take
    two slots, little-endian), scale seconds per unit"""
    if type not in TIME_TYPES:
        raise ValueError("time type: one of %s is expected, got %r" % (sorted(TIME_TYPES), type))
    f = TimeField()
    f.column, f.type, f.scale = int(column), TIME_TYPES[type], float(scale)
    _check_field(f, None, "time_field")
    return f


def sweep_motion(R, t, span=None, ref=0.5):
    """dcreg_sweep_motion: (R 3x3, t 3) = the sensor pose at the end of the span in the frame of the pose at its start; span = (t_begin, t_end)
    in seconds, or None = the cloud's own minimum / maximum finite stamp; ref = the reference instant in [0, 1] of the span"""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError("sweep_motion: R 3x3 and t 3 are expected, got %s and %s" % (R.shape, t.shape))
    m = SweepMotion()
    m.R[:] = [float(v) for v in R.reshape(9)]
    m.t[:] = [float(v) for v in t]
    if span is None:
        m.span_from_data, m.t_begin, m.t_end = 1, 0.0, 0.0
    else:
        sp = np.asarray(span, np.float64).reshape(-1)
        if sp.shape != (2,):
            raise ValueError("sweep_motion: span = (t_begin, t_end) or None, got %r" % (span,))
        m.span_from_data, m.t_begin, m.t_end = 0, float(sp[0]), float(sp[1])
    m.ref = float(ref)
    _check_motion(m, "sweep_motion")
    return m


def _deskew_info_dict(i):
    return {"n_in": i.n_in, "n_finite": i.n_finite, "n_outside": i.n_outside, "t_min": i.t_min, "t_max": i.t_max}


def _motions(motions, n, what):
    ms = [motions] if isinstance(motions, SweepMotion) else list(motions)
    if len(ms) == 1 and n != 1:
        ms = ms * n
    if len(ms) != n:
        raise ValueError("%s: one motion per cloud is expected (%d clouds, %d motions)" % (what, n, len(ms)))
    for m in ms:
        _check_motion(m, what)
    arr = (SweepMotion * max(n, 1))()
    for k, m in enumerate(ms):
        arr[k] = m
    return arr


def _rotations_ok(R):
    """per matrix of R [m, 3, 3]: |R^T R - I| <= 1e-6 in every element and det > 0 (the library's is_rotation)"""
    G = np.einsum("mki,mkj->mij", R, R) - np.eye(3)
    with np.errstate(invalid="ignore"):
        return np.all(np.abs(G) <= 1e-6, axis=(1, 2)) & (np.linalg.det(R) > 0.0)


def _check_extrinsic(R, t, what):
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        raise ValueError("%s: the extrinsic is not finite" % what)
    if not np.all(_rotations_ok(R.reshape(-1, 3, 3))):
        raise ValueError("%s: the extrinsic's R is not a rotation (|R^T R - I| > 1e-6 or det <= 0)" % what)


def sweep_path(first_knot, n_knots, t_ref, extrinsic=None):
    """dcreg_sweep_path: the cloud's window [first_knot, first_knot + n_knots) of the call's knot table (n_knots >= 2), the reference instant
    t_ref in seconds (inside the window's stamps) and the pose of the sensor in the body frame (4x4, None = identity: the knots are the
    sensor's own poses)"""
    if int(n_knots) < 2 or int(first_knot) < 0:
        raise ValueError("sweep_path: a window of at least 2 knots from a knot >= 0 is expected, got %r knots from %r" % (n_knots, first_knot))
    if not np.isfinite(t_ref):
        raise ValueError("sweep_path: t_ref %r is not finite" % (t_ref,))
    E = np.eye(4) if extrinsic is None else np.asarray(extrinsic, np.float64)
    if E.shape != (4, 4):
        raise ValueError("sweep_path: a 4x4 extrinsic is expected, got %s" % (E.shape,))
    _check_extrinsic(E[:3, :3], E[:3, 3], "sweep_path")
    b = SweepPath()
    b.first_knot, b.n_knots, b.t_ref = int(first_knot), int(n_knots), float(t_ref)
    b.ext_R[:] = [float(v) for v in E[:3, :3].reshape(9)]
    b.ext_t[:] = [float(v) for v in E[:3, 3]]
    return b


def _knot_table(knot_stamps, knot_poses, what):
    """(stamps [K] float64, poses [K, 12] float64 = R row-major then t) of a knot table given as [K, 12] or [K, 4, 4] poses"""
    st = np.ascontiguousarray(knot_stamps, dtype=np.float64).reshape(-1)
    P = np.asarray(knot_poses, dtype=np.float64)
    if P.ndim == 3 and P.shape[1:] == (4, 4):
        P = np.concatenate([P[:, :3, :3].reshape(-1, 9), P[:, :3, 3]], axis=1)
    if P.ndim != 2 or P.shape[1] != 12 or len(P) != len(st):
        raise ValueError("%s: a knot table of K stamps and K poses ([K, 12] = R row-major then t, or [K, 4, 4]) is expected, got %s and %s"
                         % (what, st.shape, np.shape(knot_poses)))
    return st, np.ascontiguousarray(P)


def _paths(paths, n, st, P, what):
    """the library's refusals of a path call, over all blocks and all knots at once -> the array of blocks the call takes"""
    ps = [paths] if isinstance(paths, SweepPath) else list(paths)
    if len(ps) == 1 and n != 1:
        ps = ps * n
    if len(ps) != n:
        raise ValueError("%s: one path block per cloud is expected (%d clouds, %d blocks)" % (what, n, len(ps)))
    if any(not isinstance(b, SweepPath) for b in ps):
        raise ValueError("%s: sweep_path blocks are expected" % what)
    arr = (SweepPath * max(n, 1))(*ps)
    if n == 0:
        return arr
    b = np.frombuffer(arr, dtype=_SWEEP_PATH_DTYPE, count=n)
    K = len(st)
    first, nk = b["first_knot"], b["n_knots"].astype(np.int64)
    if np.any(nk < 2) or np.any(first < 0) or np.any(first + nk > K):
        raise ValueError("%s: every window must hold at least 2 knots inside the table of %d knots" % (what, K))
    _check_extrinsic(b["ext_R"], b["ext_t"], what)
    cover = np.zeros(K + 1, np.int64)                  # knots and segments (knot j to j + 1) inside some window
    np.add.at(cover, first, 1)
    np.add.at(cover, first + nk, -1)
    knots = np.cumsum(cover[:-1]) > 0
    cover[:] = 0
    np.add.at(cover, first, 1)
    np.add.at(cover, first + nk - 1, -1)
    segs = np.flatnonzero(np.cumsum(cover[:-1]) > 0)
    if not np.all(np.isfinite(P[knots])):
        raise ValueError("%s: a knot pose is not finite" % what)
    if not np.all(_rotations_ok(P[knots, :9].reshape(-1, 3, 3))):
        raise ValueError("%s: R of a knot is not a rotation (|R^T R - I| > 1e-6 or det <= 0)" % what)
    if not np.all(np.isfinite(st[knots])) or not np.all(st[segs + 1] > st[segs]):
        raise ValueError("%s: the stamps of a window's knots are not finite and strictly increasing" % what)
    D = np.einsum("mki,mkj->mij", P[segs, :9].reshape(-1, 3, 3), P[segs + 1, :9].reshape(-1, 3, 3))        # R_k^T R_k+1
    sn = 0.5 * np.sqrt((D[:, 2, 1] - D[:, 1, 2]) ** 2 + (D[:, 0, 2] - D[:, 2, 0]) ** 2 + (D[:, 1, 0] - D[:, 0, 1]) ** 2)
    if not np.all(np.arctan2(sn, 0.5 * (np.trace(D, axis1=1, axis2=2) - 1.0)) < np.pi / 2):
        raise ValueError("%s: a segment rotates by pi/2 or more" % what)
    with np.errstate(invalid="ignore"):
        if not np.all((b["t_ref"] >= st[first]) & (b["t_ref"] <= st[first + nk - 1])):
            raise ValueError("%s: t_ref must be finite and inside the stamps of its window's knots" % what)
    return arr


class PlaceParams(C.Structure):
    _fields_ = [("n_rings", C.c_int), ("n_sectors", C.c_int), ("max_range", C.c_double), ("min_range", C.c_double), ("z_offset", C.c_double)]


class PlaceInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_finite", C.c_int64), ("n_used", C.c_int64)]


_STRUCTS.update({"dcreg_place_params": PlaceParams, "dcreg_place_info": PlaceInfo})
PLACE_MAX_K = 64


def _check_place_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_place_params block"""
    if not isinstance(p, PlaceParams):
        raise ValueError("%s: place_params(...) is expected, got %s" % (what, type(p).__name__))
    if not 1 <= p.n_rings <= 64:
        raise ValueError("%s: n_rings in [1, 64] is expected, got %d" % (what, p.n_rings))
    if not 1 <= p.n_sectors <= 128:
        raise ValueError("%s: n_sectors in [1, 128] is expected, got %d" % (what, p.n_sectors))
    if not (np.isfinite(p.max_range) and p.max_range > 0.0):
        raise ValueError("%s: a finite max_range > 0 is expected, got %r" % (what, p.max_range))
    if not (np.isfinite(p.min_range) and 0.0 <= p.min_range < p.max_range):
        raise ValueError("%s: a finite min_range in [0, max_range) is expected, got %r" % (what, p.min_range))
    if not np.isfinite(p.z_offset):
        raise ValueError("%s: a finite z_offset is expected, got %r" % (what, p.z_offset))


def place_params(n_rings=20, n_sectors=60, max_range=80.0, min_range=0.0, z_offset=2.0):
    """dcreg_place_params: the Scan Context grid (rings x sectors out to max_range, nothing nearer than min_range) and the height offset"""
    p = PlaceParams()
    p.n_rings, p.n_sectors = int(n_rings), int(n_sectors)
    p.max_range, p.min_range, p.z_offset = float(max_range), float(min_range), float(z_offset)
    _check_place_params(p, "place_params")
    return p


def place_guess(shift, n_sectors):
    """the 4x4 start pose for registering a query (source) against the entry (target) a search returned with this shift:
    a rotation about z by 2 pi shift / n_sectors, no translation (include/dcreg.h)"""
    n_sectors = int(n_sectors)
    if not 1 <= n_sectors <= 128:
        raise ValueError("place_guess: n_sectors in [1, 128] is expected, got %d" % n_sectors)
    if not 0 <= int(shift) < n_sectors:
        raise ValueError("place_guess: a shift in [0, %d) is expected, got %d" % (n_sectors, int(shift)))
    a = 2.0 * np.pi * int(shift) / n_sectors
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return T


def _place_info_dict(i):
    return {"n_in": i.n_in, "n_finite": i.n_finite, "n_used": i.n_used}


def _descriptors(desc, bins, what):
    """[n, bins] float32 of finite values"""
    d = np.ascontiguousarray(desc, dtype=np.float32)
    if d.ndim == 3:
        d = d.reshape(d.shape[0], -1)
    if d.ndim == 1 and d.size == bins:
        d = d.reshape(1, bins)
    if d.ndim != 2 or d.shape[1] != bins:
        raise ValueError("%s: descriptors of %d floats each are expected, got shape %s" % (what, bins, np.shape(desc)))
    if not np.all(np.isfinite(d)):
        raise ValueError("%s: a descriptor holds a value that is not finite" % what)
    return d


def _check_range(first, last, k, what):
    if int(first) < 0 or int(first) > int(last):
        raise ValueError("%s: a range 0 <= first <= last is expected, got [%d, %d)" % (what, int(first), int(last)))
    if not 1 <= int(k) <= PLACE_MAX_K:
        raise ValueError("%s: k in [1, %d] is expected, got %d" % (what, PLACE_MAX_K, int(k)))


class OutlierParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("k", C.c_int), ("std_mul", C.c_double), ("search_radius", C.c_double), ("radius", C.c_double),
                ("min_neighbors", C.c_int), ("reserved_", C.c_int)]


class OutlierInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_finite", C.c_int64), ("n_sparse", C.c_int64), ("n_out", C.c_int64), ("mean", C.c_double),
                ("stddev", C.c_double), ("threshold", C.c_double)]


_STRUCTS.update({"dcreg_outlier_params": OutlierParams, "dcreg_outlier_info": OutlierInfo})
OUTLIER_MODES = {"statistical": 0, "radius": 1}      # DCREG_OUTLIER_STATISTICAL / DCREG_OUTLIER_RADIUS
OUTLIER_MAX_K = 32
OUTLIER_MAX_POINTS = 2 ** 31 - 1


def _check_outlier_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_outlier_params block"""
    if not isinstance(p, OutlierParams):
        raise ValueError("%s: outlier_params(...) is expected, got %s" % (what, type(p).__name__))
    if p.mode == OUTLIER_MODES["statistical"]:
        if not 1 <= p.k <= OUTLIER_MAX_K:
            raise ValueError("%s: k in [1, %d] is expected, got %d" % (what, OUTLIER_MAX_K, p.k))
        if not np.isfinite(p.std_mul):
            raise ValueError("%s: a finite std_mul is expected, got %r" % (what, p.std_mul))
        if not (np.isfinite(p.search_radius) and p.search_radius >= 0.0):
            raise ValueError("%s: a finite search_radius >= 0 is expected, got %r" % (what, p.search_radius))
    elif p.mode == OUTLIER_MODES["radius"]:
        if not (np.isfinite(p.radius) and p.radius > 0.0):
            raise ValueError("%s: a finite radius > 0 is expected, got %r" % (what, p.radius))
        if p.min_neighbors < 1:
            raise ValueError("%s: min_neighbors >= 1 is expected, got %d" % (what, p.min_neighbors))
    else:
        raise ValueError("%s: an outlier mode of %s is expected, got %d" % (what, sorted(OUTLIER_MODES.values()), p.mode))


def outlier_params(mode="statistical", k=8, std_mul=2.0, search_radius=0.0, radius=0.5, min_neighbors=3):
    """dcreg_outlier_params: "statistical" (PCL StatisticalOutlierRemoval: k = setMeanK, std_mul = setStddevMulThresh, search_radius > 0
    bounds the search) or "radius" (PCL RadiusOutlierRemoval: radius, min_neighbors); include/dcreg.h has the rules"""
    if mode not in OUTLIER_MODES:
        raise ValueError("outlier_params: a mode of %s is expected, got %r" % (sorted(OUTLIER_MODES), mode))
    p = OutlierParams()
    p.mode = OUTLIER_MODES[mode]
    p.k, p.min_neighbors = int(k), int(min_neighbors)
    p.std_mul, p.search_radius, p.radius = float(std_mul), float(search_radius), float(radius)
    _check_outlier_params(p, "outlier_params")
    return p


def _outlier_info_dict(i):
    return {"n_in": i.n_in, "n_finite": i.n_finite, "n_sparse": i.n_sparse, "n_out": i.n_out, "mean": i.mean, "stddev": i.stddev,
            "threshold": i.threshold}


def _check_device_cloud(n, stride, what):
    if int(n) < 0 or int(n) > OUTLIER_MAX_POINTS:
        raise ValueError("%s: 0 .. 2^31 - 1 points are expected, got %d" % (what, int(n)))
    if int(stride) < 3:
        raise ValueError("%s: a stride of at least 3 floats is expected, got %d" % (what, int(stride)))


class NormalParams(C.Structure):
    _fields_ = [("k", C.c_int), ("orient", C.c_int), ("search_radius", C.c_double), ("viewpoint", C.c_double * 3),
                ("reserved_", C.c_double * 2)]


class NormalInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_finite", C.c_int64), ("n_sparse", C.c_int64), ("n_out", C.c_int64)]


class NormalsFollowInfo(C.Structure):
    _fields_ = [("n_target", C.c_int64), ("n_refit", C.c_int64), ("n_carried", C.c_int64), ("followed", C.c_int), ("reserved_", C.c_int)]


_STRUCTS.update({"dcreg_normal_params": NormalParams, "dcreg_normal_info": NormalInfo, "dcreg_normals_follow_info": NormalsFollowInfo})
NORMAL_ORIENT = {"viewpoint": 0, "none": 1}      # DCREG_NORMAL_ORIENT_VIEWPOINT / DCREG_NORMAL_ORIENT_NONE
NORMAL_MIN_K, NORMAL_MAX_K = 3, 32


def _check_normal_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_normal_params block"""
    if not isinstance(p, NormalParams):
        raise ValueError("%s: normal_params(...) is expected, got %s" % (what, type(p).__name__))
    if not NORMAL_MIN_K <= p.k <= NORMAL_MAX_K:
        raise ValueError("%s: k in [%d, %d] is expected, got %d" % (what, NORMAL_MIN_K, NORMAL_MAX_K, p.k))
    if p.orient not in NORMAL_ORIENT.values():
        raise ValueError("%s: an orientation of %s is expected, got %d" % (what, sorted(NORMAL_ORIENT.values()), p.orient))
    if not (np.isfinite(p.search_radius) and p.search_radius >= 0.0):
        raise ValueError("%s: a finite search_radius >= 0 is expected, got %r" % (what, p.search_radius))
    if not all(np.isfinite(v) for v in p.viewpoint):
        raise ValueError("%s: a finite viewpoint is expected, got %r" % (what, list(p.viewpoint)))


def normal_params(k=5, search_radius=0.0, viewpoint=(0.0, 0.0, 0.0)):
    """dcreg_normal_params: k neighbours per point, the point itself among them (PCL NormalEstimation setKSearch; the reference's
    normal_nn), search_radius > 0 bounds the search, viewpoint = the side the normals point to (PCL setViewPoint), None = the solver's
    sign (DCREG_NORMAL_ORIENT_NONE); include/dcreg.h has the rule"""
    p = NormalParams()
    p.k = int(k)
    p.search_radius = float(search_radius)
    if viewpoint is None:
        p.orient = NORMAL_ORIENT["none"]
    else:
        v = np.asarray(viewpoint, np.float64).reshape(-1)
        if v.shape != (3,):
            raise ValueError("normal_params: a viewpoint of 3 values or None is expected, got %r" % (viewpoint,))
        p.orient = NORMAL_ORIENT["viewpoint"]
        p.viewpoint[0], p.viewpoint[1], p.viewpoint[2] = float(v[0]), float(v[1]), float(v[2])
    _check_normal_params(p, "normal_params")
    return p


class FpfhParams(C.Structure):
    _fields_ = [("k", C.c_int), ("reserved0_", C.c_int), ("search_radius", C.c_double), ("reserved_", C.c_double * 2)]


class FpfhInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_used", C.c_int64), ("n_empty", C.c_int64), ("n_out", C.c_int64)]


class MatchInfo(C.Structure):
    _fields_ = [("n_a_valid", C.c_int64), ("n_b_valid", C.c_int64), ("n_mutual", C.c_int64), ("reserved_", C.c_int64)]


_STRUCTS.update({"dcreg_fpfh_params": FpfhParams, "dcreg_fpfh_info": FpfhInfo, "dcreg_match_info": MatchInfo})
FPFH_DIM = 33                            # DCREG_FPFH_DIM
FPFH_MIN_K, FPFH_MAX_K = 3, 32
_normal_params = normal_params            # (Context.fpfh has an argument of that name)


def _check_fpfh_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_fpfh_params block"""
    if not isinstance(p, FpfhParams):
        raise ValueError("%s: fpfh_params(...) is expected, got %s" % (what, type(p).__name__))
    if not FPFH_MIN_K <= p.k <= FPFH_MAX_K:
        raise ValueError("%s: k in [%d, %d] is expected, got %d" % (what, FPFH_MIN_K, FPFH_MAX_K, p.k))
    if not (np.isfinite(p.search_radius) and p.search_radius >= 0.0):
        raise ValueError("%s: a finite search_radius >= 0 is expected, got %r" % (what, p.search_radius))


def fpfh_params(k=16, search_radius=0.0):
    """dcreg_fpfh_params: k neighbours per point, the point itself among them (PCL FPFHEstimation setKSearch); search_radius > 0 bounds
    the search (a point keeps the neighbours it has inside it); include/dcreg.h has the rule"""
    p = FpfhParams()
    p.k = int(k)
    p.search_radius = float(search_radius)
    _check_fpfh_params(p, "fpfh_params")
    return p


def _fpfh_info_dict(i):
    return {"n_in": i.n_in, "n_used": i.n_used, "n_empty": i.n_empty, "n_out": i.n_out}


class FpfhRadiusParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("max_neighbors", C.c_int), ("reserved0_", C.c_int), ("reserved_", C.c_double * 2)]


class FpfhRadiusInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_used", C.c_int64), ("n_empty", C.c_int64), ("n_crowded", C.c_int64), ("n_out", C.c_int64),
                ("m_max", C.c_int64), ("m_sum", C.c_int64), ("reserved_", C.c_int64)]


_STRUCTS.update({"dcreg_fpfh_radius_params": FpfhRadiusParams, "dcreg_fpfh_radius_info": FpfhRadiusInfo})
FPFH_MIN_CAP, FPFH_MAX_CAP = 2, 65535


def _check_fpfh_radius_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_fpfh_radius_params block"""
    if not isinstance(p, FpfhRadiusParams):
        raise ValueError("%s: fpfh_radius_params(...) is expected, got %s" % (what, type(p).__name__))
    with np.errstate(all="ignore"):
        r2 = np.float32(np.float64(p.radius) * np.float64(p.radius))
    if not (np.isfinite(p.radius) and p.radius > 0.0 and np.float32(0.0) < r2 < np.float32(3.0e38)):
        raise ValueError("%s: a finite radius > 0 whose square is a float in (0, 3.0e38) is expected, got %r" % (what, p.radius))
    if not FPFH_MIN_CAP <= p.max_neighbors <= FPFH_MAX_CAP:
        raise ValueError("%s: max_neighbors in [%d, %d] is expected, got %d" % (what, FPFH_MIN_CAP, FPFH_MAX_CAP, p.max_neighbors))


def fpfh_radius_params(radius=1.0, max_neighbors=65535):
    """dcreg_fpfh_radius_params: every used point within radius is a neighbour (PCL FPFHEstimation setRadiusSearch); a point with more
    than max_neighbors of them is crowded and gets no descriptor; include/dcreg.h has the rule"""
    p = FpfhRadiusParams()
    p.radius = float(radius)
    p.max_neighbors = int(max_neighbors)
    _check_fpfh_radius_params(p, "fpfh_radius_params")
    return p


def _fpfh_radius_info_dict(i):
    return {"n_in": i.n_in, "n_used": i.n_used, "n_empty": i.n_empty, "n_crowded": i.n_crowded, "n_out": i.n_out, "m_max": i.m_max,
            "m_sum": i.m_sum}


def _feature_rows(a, what):
    """descriptor rows as the C-ABI takes them: 2-D float32, the 33 values in the first columns, further columns skipped through the stride"""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.float32 or a.shape[1] < FPFH_DIM:
        raise ValueError("%s: a 2-D float32 array with at least %d columns is expected, got %s %s" % (what, FPFH_DIM, a.dtype, a.shape))
    if a.shape[0] > OUTLIER_MAX_POINTS:
        raise ValueError("%s: at most 2^31 - 1 rows are expected, got %d" % (what, a.shape[0]))
    return np.ascontiguousarray(a)


def _check_device_rows(n, stride, what):
    if int(n) < 0 or int(n) > OUTLIER_MAX_POINTS:
        raise ValueError("%s: 0 .. 2^31 - 1 rows are expected, got %d" % (what, int(n)))
    if int(stride) < FPFH_DIM:
        raise ValueError("%s: a stride of at least %d floats is expected, got %d" % (what, FPFH_DIM, int(stride)))


class AlignParams(C.Structure):
    _fields_ = [("n_hypotheses", C.c_int64), ("seed", C.c_uint64), ("inlier_distance", C.c_double), ("edge_similarity", C.c_double),
                ("n_best", C.c_int), ("refine_iterations", C.c_int), ("reserved_", C.c_double * 2)]


class AlignRecord(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("hypothesis", C.c_int64), ("pairs", C.c_int32 * 3), ("count", C.c_int32), ("cost", C.c_uint64),
                ("n_inliers", C.c_int32), ("refined", C.c_int32), ("rmse", C.c_double)]


class AlignInfo(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("n_used", C.c_int64), ("n_drawn", C.c_int64), ("n_degenerate", C.c_int64), ("n_rejected", C.c_int64),
                ("n_scored", C.c_int64), ("n_returned", C.c_int64), ("reserved_", C.c_int64)]


_STRUCTS.update({"dcreg_align_params": AlignParams, "dcreg_align_record": AlignRecord, "dcreg_align_info": AlignInfo})
ALIGN_MAX_HYPOTHESES, ALIGN_MAX_BEST, ALIGN_MAX_REFINE = 1 << 24, 32, 8


def _check_align_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_align_params block"""
    if not isinstance(p, AlignParams):
        raise ValueError("%s: align_params(...) is expected, got %s" % (what, type(p).__name__))
    if not 1 <= p.n_hypotheses <= ALIGN_MAX_HYPOTHESES:
        raise ValueError("%s: n_hypotheses in [1, 2^24] is expected, got %d" % (what, p.n_hypotheses))
    if not (np.isfinite(p.inlier_distance) and p.inlier_distance > 0.0):
        raise ValueError("%s: a finite inlier_distance > 0 is expected, got %r" % (what, p.inlier_distance))
    if not 0.0 <= p.edge_similarity < 1.0:
        raise ValueError("%s: an edge_similarity in [0, 1) is expected, got %r" % (what, p.edge_similarity))
    if not 1 <= p.n_best <= ALIGN_MAX_BEST:
        raise ValueError("%s: n_best in [1, %d] is expected, got %d" % (what, ALIGN_MAX_BEST, p.n_best))
    if not 0 <= p.refine_iterations <= ALIGN_MAX_REFINE:
        raise ValueError("%s: refine_iterations in [0, %d] is expected, got %d" % (what, ALIGN_MAX_REFINE, p.refine_iterations))


def align_params(n_hypotheses=100000, seed=0, inlier_distance=0.5, edge_similarity=0.9, n_best=1, refine_iterations=3):
    """dcreg_align_params: H seeded three-pair hypotheses, the inlier distance d in metres, the edge-length pre-rejection s (0 = none;
    a hypothesis is kept when the three edges of its triangles agree within the factor s), the number of records returned and the
    least-squares refinement steps of each; include/dcreg.h has the rule"""
    p = AlignParams()
    p.n_hypotheses = int(n_hypotheses)
    p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    p.inlier_distance = float(inlier_distance)
    p.edge_similarity = float(edge_similarity)
    p.n_best = int(n_best)
    p.refine_iterations = int(refine_iterations)
    _check_align_params(p, "align_params")
    return p


def _align_info_dict(i):
    return {k: getattr(i, k) for k in ("n_pairs", "n_used", "n_drawn", "n_degenerate", "n_rejected", "n_scored", "n_returned")}


def _align_records(recs, n):
    return [{"T": np.array(r.T, np.float64).reshape(4, 4), "hypothesis": r.hypothesis, "pairs": tuple(r.pairs), "count": r.count, "cost": r.cost,
             "n_inliers": r.n_inliers, "refined": r.refined, "rmse": r.rmse} for r in recs[:n]]


def _corr_index(a, what):
    a = np.asarray(a)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("%s: a 1-D integer index array is expected, got %s %s" % (what, a.dtype, a.shape))
    if a.size and (a.min() < -(2 ** 31) or a.max() > 2 ** 31 - 1):
        raise ValueError("%s: index values that fit an int32 are expected" % what)
    return np.ascontiguousarray(a, np.int32)


def correspondences_from_match(match, mutual_only=True, max_ratio=None):
    """The dict of Context.feature_match(a, b) as index pairs for align_correspondences: rows of a without a match (-1) are dropped, with
    mutual_only the rows whose match is not mutual, with max_ratio the rows whose ratio sqrt(d / d2) of the best to the second-best
    distance is above it (a row without a second-best passes).  Pure numpy.  -> (corr_a [m] int32, corr_b [m] int32)"""
    idx = np.asarray(match["idx"])
    keep = idx >= 0
    if mutual_only:
        if "mutual" not in match:
            raise ValueError("correspondences_from_match: mutual_only needs feature_match(..., want_mutual=True)")
        keep &= np.asarray(match["mutual"]) != 0
    if max_ratio is not None:
        if "d2" not in match:
            raise ValueError("correspondences_from_match: max_ratio needs feature_match(..., want_second=True)")
        d, d2 = np.asarray(match["d"], np.float64), np.asarray(match["d2"], np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            keep &= ~(np.sqrt(d / d2) > float(max_ratio))
    rows = np.flatnonzero(keep)
    return rows.astype(np.int32), idx[rows].astype(np.int32)


class ConsensusParams(C.Structure):
    _fields_ = [("compat_distance", C.c_double), ("min_length", C.c_double), ("inlier_distance", C.c_double), ("n_seeds", C.c_int),
                ("consensus_size", C.c_int), ("n_best", C.c_int), ("refine_iterations", C.c_int), ("reserved_", C.c_double * 2)]


class ConsensusRecord(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("seed", C.c_int32), ("seed_rank", C.c_int32), ("weight", C.c_int32), ("n_members", C.c_int32),
                ("count", C.c_int32), ("cost", C.c_uint64), ("n_inliers", C.c_int32), ("refined", C.c_int32), ("rmse", C.c_double)]


class ConsensusInfo(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("n_used", C.c_int64), ("n_edges", C.c_int64), ("max_degree", C.c_int64), ("n_seeds", C.c_int64),
                ("n_skipped", C.c_int64), ("n_scored", C.c_int64), ("n_returned", C.c_int64), ("reserved_", C.c_int64)]


_STRUCTS.update({"dcreg_consensus_params": ConsensusParams, "dcreg_consensus_record": ConsensusRecord, "dcreg_consensus_info": ConsensusInfo})
CONSENSUS_MAX_PAIRS, CONSENSUS_MAX_SEEDS, CONSENSUS_MAX_SET = 32768, 1024, 64


def _check_consensus_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_consensus_params block"""
    if not isinstance(p, ConsensusParams):
        raise ValueError("%s: consensus_params(...) is expected, got %s" % (what, type(p).__name__))
    if not (np.isfinite(p.compat_distance) and p.compat_distance > 0.0):
        raise ValueError("%s: a finite compat_distance > 0 is expected, got %r" % (what, p.compat_distance))
    if not (np.isfinite(p.min_length) and p.min_length >= 0.0):
        raise ValueError("%s: a finite min_length >= 0 is expected, got %r" % (what, p.min_length))
    if not (np.isfinite(p.inlier_distance) and p.inlier_distance > 0.0):
        raise ValueError("%s: a finite inlier_distance > 0 is expected, got %r" % (what, p.inlier_distance))
    if not 1 <= p.n_seeds <= CONSENSUS_MAX_SEEDS:
        raise ValueError("%s: n_seeds in [1, %d] is expected, got %d" % (what, CONSENSUS_MAX_SEEDS, p.n_seeds))
    if not 3 <= p.consensus_size <= CONSENSUS_MAX_SET:
        raise ValueError("%s: consensus_size in [3, %d] is expected, got %d" % (what, CONSENSUS_MAX_SET, p.consensus_size))
    if not 1 <= p.n_best <= ALIGN_MAX_BEST:
        raise ValueError("%s: n_best in [1, %d] is expected, got %d" % (what, ALIGN_MAX_BEST, p.n_best))
    if not 0 <= p.refine_iterations <= ALIGN_MAX_REFINE:
        raise ValueError("%s: refine_iterations in [0, %d] is expected, got %d" % (what, ALIGN_MAX_REFINE, p.refine_iterations))


def consensus_params(compat_distance=0.5, min_length=1.0, inlier_distance=0.5, n_seeds=64, consensus_size=16, n_best=1, refine_iterations=3):
    """dcreg_consensus_params: two pairs are compatible when their lengths on both sides are at least min_length and differ by at most
    compat_distance (metres); the n_seeds pairs of the largest second-order weight each gather a set of at most consensus_size members;
    the sets' poses are scored with the inlier distance d, the n_best best returned and refined; include/dcreg.h has the rule"""
    p = ConsensusParams()
    p.compat_distance = float(compat_distance)
    p.min_length = float(min_length)
    p.inlier_distance = float(inlier_distance)
    p.n_seeds = int(n_seeds)
    p.consensus_size = int(consensus_size)
    p.n_best = int(n_best)
    p.refine_iterations = int(refine_iterations)
    _check_consensus_params(p, "consensus_params")
    return p


def _consensus_info_dict(i):
    return {k: getattr(i, k) for k in ("n_pairs", "n_used", "n_edges", "max_degree", "n_seeds", "n_skipped", "n_scored", "n_returned")}


def _consensus_records(recs, n):
    return [{"T": np.array(r.T, np.float64).reshape(4, 4), "seed": r.seed, "seed_rank": r.seed_rank, "weight": r.weight, "n_members": r.n_members,
             "count": r.count, "cost": r.cost, "n_inliers": r.n_inliers, "refined": r.refined, "rmse": r.rmse} for r in recs[:n]]


class VerifyParams(C.Structure):
    _fields_ = [("inlier_distance", C.c_double), ("point_stride", C.c_int64), ("rank_by", C.c_int32), ("detail_pose", C.c_int32),
                ("reserved_", C.c_double * 2)]


class VerifyRecord(C.Structure):
    _fields_ = [("pose", C.c_int32), ("count", C.c_int32), ("cost", C.c_uint64), ("score", C.c_uint64), ("fitness", C.c_double),
                ("rmse", C.c_double)]


class VerifyInfo(C.Structure):
    _fields_ = [("n_poses", C.c_int64), ("n_points", C.c_int64), ("n_scored", C.c_int64), ("best_pose", C.c_int64), ("reserved_", C.c_int64 * 2)]


_STRUCTS.update({"dcreg_verify_params": VerifyParams, "dcreg_verify_record": VerifyRecord, "dcreg_verify_info": VerifyInfo})
VERIFY_MAX_POSES, VERIFY_RECORD_STRIDE = 65535, 22      # (22 doubles: the size of an align or consensus record, whose T leads it)


def _check_verify_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_verify_params block (detail_pose against the poses: _verify_poses)"""
    if not isinstance(p, VerifyParams):
        raise ValueError("%s: verify_params(...) is expected, got %s" % (what, type(p).__name__))
    if not (np.isfinite(p.inlier_distance) and p.inlier_distance > 0.0):
        raise ValueError("%s: a finite inlier_distance > 0 is expected, got %r" % (what, p.inlier_distance))
    if p.point_stride < 1:
        raise ValueError("%s: point_stride >= 1 is expected, got %d" % (what, p.point_stride))
    if p.rank_by not in (0, 1):
        raise ValueError("%s: rank_by 0 (count, cost) or 1 (score) is expected, got %d" % (what, p.rank_by))
    if p.detail_pose < -1:
        raise ValueError("%s: detail_pose -1 (none) or an input index is expected, got %d" % (what, p.detail_pose))


def verify_params(inlier_distance=0.5, point_stride=1, rank_by=0, detail_pose=-1):
    """dcreg_verify_params: the inlier distance d in metres (a point counts when a map point lies strictly inside it), every
    point_stride-th point of the cloud by original index, the ranking key - 0: (count descending, cost ascending), the align records'
    key; 1: the MSAC score ascending - and the input index of the pose whose inlier mask and neighbours are wanted (-1: none);
    include/dcreg.h has the rule"""
    p = VerifyParams()
    p.inlier_distance = float(inlier_distance)
    p.point_stride = int(point_stride)
    p.rank_by = int(rank_by)
    p.detail_pose = int(detail_pose)
    _check_verify_params(p, "verify_params")
    return p


def _verify_poses(Ts, p, what):
    """the poses of a verify call - [P, 4, 4], or a list of record dicts with a T - as a contiguous [P, 16] block, checked as the C-ABI
    checks them"""
    if isinstance(Ts, (list, tuple)) and len(Ts) and isinstance(Ts[0], dict):
        Ts = [r["T"] for r in Ts]
    Ts = np.ascontiguousarray(Ts, dtype=np.float64)
    if Ts.size == 0:
        Ts = Ts.reshape(0, 4, 4)
    if Ts.ndim != 3 or Ts.shape[1:] != (4, 4):
        raise ValueError("%s: poses of shape [P, 4, 4] are expected, got %s" % (what, (Ts.shape,)))
    n = Ts.shape[0]
    if n > VERIFY_MAX_POSES:
        raise ValueError("%s: at most %d poses are expected, got %d" % (what, VERIFY_MAX_POSES, n))
    if p.detail_pose >= n:
        raise ValueError("%s: detail_pose in [-1, %d] is expected, got %d" % (what, n - 1, p.detail_pose))
    top = Ts[:, :3, :]
    bad = np.flatnonzero(~np.isfinite(top).all(axis=(1, 2)))
    if len(bad):
        raise ValueError("%s: pose %d has a non-finite entry" % (what, bad[0]))
    bad = np.flatnonzero(~_rotations_ok(top[:, :, :3]))
    if len(bad):
        raise ValueError("%s: the rotation block of pose %d is not a rotation (|R^T R - I| > 1e-6 or det <= 0)" % (what, bad[0]))
    return Ts.reshape(n, 16), n


def _verify_info_dict(i):
    return {k: getattr(i, k) for k in ("n_poses", "n_points", "n_scored", "best_pose")}


def _verify_records(recs, n):
    return [{"pose": r.pose, "count": r.count, "cost": r.cost, "score": r.score, "fitness": r.fitness, "rmse": r.rmse} for r in recs[:n]]


def _check_voxel_map_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_voxel_map_params block"""
    if not isinstance(p, VoxelMapParams):
        raise ValueError("%s: voxel_map_params(...) is expected, got %s" % (what, type(p).__name__))
    if not (np.isfinite(p.leaf) and p.leaf > 0.0):
        raise ValueError("%s: a finite leaf > 0 is expected, got %r" % (what, p.leaf))
    if not 1.0e-6 <= p.epsilon <= 1.0:
        raise ValueError("%s: an epsilon in [1e-6, 1] is expected, got %r" % (what, p.epsilon))
    if p.min_points < 2:
        raise ValueError("%s: min_points >= 2 is expected, got %d" % (what, p.min_points))


def voxel_map_params(leaf=1.0, epsilon=1.0e-3, min_points=6):
    """dcreg_voxel_map_params: the voxel edge in metres, the floor of the normalised eigenvalues, and the points a voxel needs to be kept
    (include/dcreg.h has the rule)"""
    p = VoxelMapParams()
    p.leaf, p.epsilon, p.min_points, p.reserved_ = float(leaf), float(epsilon), int(min_points), 0
    _check_voxel_map_params(p, "voxel_map_params")
    return p


def _normal_info_dict(i):
    return {"n_in": i.n_in, "n_finite": i.n_finite, "n_sparse": i.n_sparse, "n_out": i.n_out}


KEYFRAME_MAX_POINTS = 2 ** 31 - 1      # member points of one gather (include/dcreg.h)


def _voxel_block(leaf, mode, min_points, what):
    """None (no voxel pass), a voxel_params(...) block, or the block of a leaf / mode / min_points"""
    if leaf is None:
        return None
    if isinstance(leaf, VoxelParams):
        p = leaf
        if not all(np.isfinite(p.leaf[a]) and p.leaf[a] > 0.0 for a in range(3)):
            raise ValueError("%s: voxel leaf: finite edges > 0 are expected, got %s" % (what, list(p.leaf)))
        if p.mode not in VOXEL_MODES.values():
            raise ValueError("%s: a voxel mode of %s is expected, got %d" % (what, sorted(VOXEL_MODES.values()), p.mode))
        return p
    if isinstance(leaf, (str, bytes, dict)) or isinstance(leaf, C.Structure):
        raise ValueError("%s: leaf: None, one edge, three edges or voxel_params(...) is expected, got %s" % (what, type(leaf).__name__))
    try:
        return voxel_params(leaf, mode, min_points)
    except (TypeError, ValueError) as e:
        raise ValueError("%s: %s" % (what, e)) from None


def _keyframe_id(i, what):
    if isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)):
        raise ValueError("%s: keyframe ids are integers, got %r" % (what, i))
    if int(i) < 0:
        raise ValueError("%s: keyframe ids are >= 0, got %d" % (what, int(i)))
    return int(i)


def _members(members, what):
    """(member_offsets [n + 1], ids [M], poses [M, 12]) of a list (one per submap) of lists of (keyframe id, T 4x4)"""
    if isinstance(members, (str, bytes)) or not hasattr(members, "__len__"):
        raise ValueError("%s: members: a list (one per submap) of lists of (id, T 4x4) is expected" % what)
    off, ids, poses = [0], [], []
    for g, sub in enumerate(members):
        if isinstance(sub, (str, bytes)) or not hasattr(sub, "__len__"):
            raise ValueError("%s: members[%d]: a list of (id, T 4x4) is expected" % (what, g))
        for m, item in enumerate(sub):
            if not isinstance(item, (tuple, list)) or len(item) != 2:
                raise ValueError("%s: members[%d][%d]: an (id, T 4x4) pair is expected" % (what, g, m))
            where = "%s: members[%d][%d]" % (what, g, m)
            ids.append(_keyframe_id(item[0], where))
            try:
                R, t = _pose_rt(item[1], where)
            except (TypeError, ValueError) as e:
                raise ValueError(str(e) if str(e).startswith(where) else "%s: a 4x4 pose is expected (%s)" % (where, e)) from None
            if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
                raise ValueError("%s: a finite pose is expected" % where)
            poses.append(np.concatenate([R, t]))
        off.append(len(ids))
    return (np.asarray(off, np.int64), np.asarray(ids, np.int64).reshape(-1),
            np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12)))


class VisibilityParams(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("elev_min", C.c_double), ("elev_max", C.c_double), ("min_range", C.c_double),
                ("max_range", C.c_double), ("margin_abs", C.c_double), ("margin_rel", C.c_double), ("window", C.c_int), ("min_votes", C.c_int),
                ("min_ratio", C.c_double)]


class VisibilityInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_finite", C.c_int64), ("n_observed", C.c_int64), ("n_flagged", C.c_int64), ("n_out", C.c_int64),
                ("n_members", C.c_int64)]


_STRUCTS.update({"dcreg_visibility_params": VisibilityParams, "dcreg_visibility_info": VisibilityInfo})
VISIBILITY_MAX_ROWS, VISIBILITY_MAX_COLS, VISIBILITY_MAX_WINDOW = 256, 4096, 3


def _check_visibility_params(p, what):
    """the refusals of include/dcreg.h for a dcreg_visibility_params block"""
    if not isinstance(p, VisibilityParams):
        raise ValueError("%s: visibility_params(...) is expected, got %s" % (what, type(p).__name__))
    if not (1 <= p.rows <= VISIBILITY_MAX_ROWS and 1 <= p.cols <= VISIBILITY_MAX_COLS):
        raise ValueError("%s: rows in [1, %d] and cols in [1, %d] are expected, got %d x %d"
                         % (what, VISIBILITY_MAX_ROWS, VISIBILITY_MAX_COLS, p.rows, p.cols))
    if not (np.isfinite(p.elev_min) and np.isfinite(p.elev_max) and -0.5 * np.pi <= p.elev_min < p.elev_max <= 0.5 * np.pi):
        raise ValueError("%s: elev_min < elev_max inside [-pi/2, pi/2] is expected, got %r, %r" % (what, p.elev_min, p.elev_max))
    if not (np.isfinite(p.min_range) and np.isfinite(p.max_range) and 0.0 <= p.min_range < p.max_range):
        raise ValueError("%s: a finite 0 <= min_range < max_range is expected, got %r, %r" % (what, p.min_range, p.max_range))
    if not (np.isfinite(p.margin_abs) and p.margin_abs >= 0.0):
        raise ValueError("%s: a finite margin_abs >= 0 is expected, got %r" % (what, p.margin_abs))
    if not (np.isfinite(p.margin_rel) and p.margin_rel >= 0.0):
        raise ValueError("%s: a finite margin_rel >= 0 is expected, got %r" % (what, p.margin_rel))
    if not 0 <= p.window <= VISIBILITY_MAX_WINDOW:
        raise ValueError("%s: a window in [0, %d] is expected, got %d" % (what, VISIBILITY_MAX_WINDOW, p.window))
    if p.min_votes < 1:
        raise ValueError("%s: min_votes >= 1 is expected, got %d" % (what, p.min_votes))
    if not 0.0 <= p.min_ratio <= 1.0:
        raise ValueError("%s: a min_ratio in [0, 1] is expected, got %r" % (what, p.min_ratio))


def visibility_params(rows=64, cols=1024, elev_min=-0.125 * np.pi, elev_max=0.125 * np.pi, min_range=0.5, max_range=80.0, margin_abs=0.2,
                      margin_rel=0.01, window=1, min_votes=2, min_ratio=0.0):
    """dcreg_visibility_params: the range image (rows x cols over the elevations [elev_min, elev_max] radians and the ranges
    [min_range, max_range) metres), the margins of the see-through test (range > r + margin_abs + margin_rel r), the pixel window whose
    minimum is compared, and the decision (through >= min_votes and through >= min_ratio x observed); include/dcreg.h has the rule"""
    for name, v in (("rows", rows), ("cols", cols), ("window", window), ("min_votes", min_votes)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("visibility_params: %s: an integer is expected, got %r" % (name, v))
    p = VisibilityParams()
    p.rows, p.cols, p.window, p.min_votes = int(rows), int(cols), int(window), int(min_votes)
    p.elev_min, p.elev_max, p.min_range, p.max_range = float(elev_min), float(elev_max), float(min_range), float(max_range)
    p.margin_abs, p.margin_rel, p.min_ratio = float(margin_abs), float(margin_rel), float(min_ratio)
    _check_visibility_params(p, "visibility_params")
    return p


def _visibility_info_dict(i):
    return {"n_in": i.n_in, "n_finite": i.n_finite, "n_observed": i.n_observed, "n_flagged": i.n_flagged, "n_out": i.n_out,
            "n_members": i.n_members}


def _keyframe_ids(ids, what):
    """[n] int64 of a sequence of keyframe ids, checked as a whole (no loop over the ids)"""
    a = np.asarray(ids)
    if a.dtype == object or a.ndim != 1 and a.size:
        raise ValueError("%s: keyframe ids: a 1-D sequence of integers is expected" % what)
    a = a.reshape(-1)
    if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("%s: keyframe ids are integers, got %s" % (what, a.dtype))
    a = np.ascontiguousarray(a, dtype=np.int64)
    if a.size and int(a.min()) < 0:
        raise ValueError("%s: keyframe ids are >= 0, got %d" % (what, int(a.min())))
    return a


def _vote_members(members, what):
    """(ids [M] int64, poses [M, 12] float64 = R row-major then t) of the members of a visibility call: an (ids [M], T [M, 4, 4]) pair of
    arrays, or a list of (keyframe id, T 4x4) as set_target_keyframes takes it.  Checked with numpy over all members at once."""
    if isinstance(members, (str, bytes)) or not hasattr(members, "__len__"):
        raise ValueError("%s: members: a list of (id, T 4x4) or an (ids [M], T [M, 4, 4]) pair is expected" % what)
    if isinstance(members, tuple) and len(members) == 2 and np.ndim(members[0]) == 1:
        ids, Ts = members
    elif len(members) == 0:
        ids, Ts = np.zeros(0, np.int64), np.zeros((0, 4, 4))
    else:
        try:
            ok = all(len(m) == 2 for m in members)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError("%s: members: a list of (id, T 4x4) or an (ids [M], T [M, 4, 4]) pair is expected" % what)
        ids, Ts = zip(*members)
    ids = _keyframe_ids(ids, "%s: members" % what)
    try:
        Ts = np.asarray(Ts, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: members: 4x4 poses are expected" % what) from None
    if Ts.shape != (len(ids), 4, 4):
        raise ValueError("%s: members: %d poses of shape 4x4 are expected, got shape %s" % (what, len(ids), Ts.shape))
    poses = np.ascontiguousarray(np.concatenate([Ts[:, :3, :3].reshape(-1, 9), Ts[:, :3, 3]], 1))
    if not np.all(np.isfinite(poses)):
        raise ValueError("%s: members: finite poses are expected (member %d)" % (what, int(np.argmin(np.isfinite(poses).all(1)))))
    return ids, poses


def _offsets(offsets, what):
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if len(off) < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
        raise ValueError("%s: offsets must start at 0 and not decrease" % what)
    return off


def _clouds(clouds, what):
    """(xyz [N, c] float32, offsets [n + 1] int64, was_list) of a list of [n_i, c] float32 arrays or an (xyz, offsets) pair"""
    if isinstance(clouds, tuple):
        if len(clouds) != 2:
            raise ValueError("%s: an (xyz, offsets) pair is expected" % what)
        xyz = _points(clouds[0], what)
        off = np.ascontiguousarray(clouds[1], dtype=np.int64).reshape(-1)
        if len(off) < 1 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != len(xyz):
            raise ValueError("%s: offsets must start at 0, not decrease and end at the number of points (%d)" % (what, len(xyz)))
        return xyz, off, False
    parts = [_points(f, what) for f in clouds]
    if len({f.shape[1] for f in parts}) > 1:
        raise ValueError("%s: every cloud needs the same number of columns, got %s" % (what, sorted({f.shape[1] for f in parts})))
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(f) for f in parts])
    xyz = np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.float32))
    return xyz, off, True


def _pose_rt(T, what):
    """(R row-major [9], t [3]) of a 4x4 pose"""
    T = np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("%s: a 4x4 pose is expected, got shape %s" % (what, T.shape))
    return np.ascontiguousarray(T[:3, :3]).reshape(9), np.ascontiguousarray(T[:3, 3])


def _update_dict(u):
    return {"n_offered": u.n_offered, "n_added": u.n_added, "n_removed": u.n_removed, "n_target": u.n_target, "rebuilt": u.rebuilt}


class DcregError(RuntimeError):
    pass


class CapacityError(DcregError):
    """a device output buffer is too small: nothing was written; out_offsets / info carry the sizes needed (the capacity protocol)"""
    def __init__(self, msg, out_offsets, info):
        super().__init__(msg)
        self.out_offsets, self.info = out_offsets, info


def load():
    """dlopen the in-tree HIP library.  Fails loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DcregError("libdcreg_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                         "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    vp = C.c_void_p
    L.dcreg_backend_create.restype = C.c_int
    L.dcreg_backend_create.argtypes = [C.POINTER(vp), C.c_int]
    L.dcreg_backend_destroy.restype = None
    L.dcreg_backend_destroy.argtypes = [vp]
    L.dcreg_last_error.restype = C.c_char_p
    L.dcreg_last_error.argtypes = [vp]
    L.dcreg_set_stream.argtypes = [vp, vp]
    L.dcreg_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    for name in ("dcreg_set_target", "dcreg_set_target_device"):
        getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_double]
    for name in ("dcreg_set_source", "dcreg_set_source_device"):
        getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64]
    L.dcreg_default_lin_params.argtypes = [C.POINTER(LinParams), C.c_double]
    L.dcreg_linearize.argtypes = [vp, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut)]
    L.dcreg_linearize_batch.argtypes = [vp, C.c_int, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut)]
    L.dcreg_linearize_batch_begin.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.POINTER(LinParams)]
    L.dcreg_linearize_batch_begin_warm.argtypes = [vp, C.c_int, C.c_int, dp, dp, ip, C.POINTER(LinParams)]
    L.dcreg_linearize_batch_end.argtypes = [vp, C.c_int, C.POINTER(LinOut)]
    L.dcreg_reserve_warm_states.argtypes = [vp, C.c_int64]
    L.dcreg_reset_warm_state.argtypes = [vp, C.c_int64]
    L.dcreg_hint_misalignment.argtypes = [vp, C.c_double]
    L.dcreg_launch_stats_get.argtypes = [vp, C.POINTER(LaunchStats), C.c_int]
    L.dcreg_linearize_gated_begin.argtypes = [vp, C.c_int, C.POINTER(LinParams)]
    L.dcreg_linearize_gate_open.argtypes = [vp, dp, dp]
    L.dcreg_linearize_gate_abort.argtypes = [vp]
    L.dcreg_linearize_debug.argtypes = [vp, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut), C.POINTER(LinDebug)]
    L.dcreg_knn.argtypes = [vp, fp, C.c_int64, C.c_int64, C.c_int, C.c_double, ip, fp]
    L.dcreg_kdtree_build.argtypes = [vp, C.c_int]
    L.dcreg_kdtree_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp]
    L.dcreg_knn_timed.argtypes = [vp, fp, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_int, C.c_int, ip, fp, dp]
    L.dcreg_index_info_get.argtypes = [vp, C.POINTER(IndexInfo)]
    L.dcreg_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64), C.c_int]
    L.dcreg_launch_series.argtypes = [vp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.c_int]
    if hasattr(L, "dcreg_launch_series_passes"):        # (absent from an older build loaded through DCREG_LIB for an A/B: scripts/ab_multi.sh)
        L.dcreg_launch_series_passes.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64]
    if hasattr(L, "dcreg_launch_series_structure"):
        L.dcreg_launch_series_structure.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64]
    if hasattr(L, "dcreg_team_pass_stamps"):
        L.dcreg_team_pass_stamps.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int64]
    L.dcreg_default_config.restype = None
    L.dcreg_default_config.argtypes = [C.POINTER(Config)]
    L.dcreg_analyze_degeneracy.argtypes = [dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(Analysis)]
    L.dcreg_analyze_degeneracy_two_part.argtypes = [dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(Analysis), C.POINTER(C.c_int)]
    L.dcreg_solve_degenerate_system.argtypes = [dp, dp, C.c_int, C.POINTER(Config), C.POINTER(Analysis), dp]
    L.dcreg_unpack_hessian.restype = None
    L.dcreg_unpack_hessian.argtypes = [dp, dp]
    L.dcreg_boxplus.restype = None
    L.dcreg_boxplus.argtypes = [dp, dp, dp, dp, dp]
    L.dcreg_pose6d_to_matrix.restype = None
    L.dcreg_pose6d_to_matrix.argtypes = [C.c_double] * 6 + [dp]
    L.dcreg_pose_error.restype = None
    L.dcreg_pose_error.argtypes = [dp, dp, dp, dp]
    L.dcreg_icp_run.argtypes = [vp, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(IterLog), C.c_int,
                                C.POINTER(IcpResult)]
    L.dcreg_icp_run_sharded.argtypes = [vp, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.c_int64, REDUCE_FN, vp,
                                        C.POINTER(IterLog), C.c_int, C.POINTER(IcpResult)]
    L.dcreg_comm_unique_id.argtypes = [vp]
    L.dcreg_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    L.dcreg_comm_destroy.argtypes = [vp]
    L.dcreg_comm_allgather_sum.argtypes = [vp, dp]
    L.dcreg_icp_run_sharded_rccl.argtypes = [vp, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.c_int64, C.POINTER(IterLog), C.c_int,
                                             C.POINTER(IcpResult)]
    L.dcreg_icp_run_many.argtypes = [C.c_int, C.POINTER(vp), dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(IcpResult)]
    L.dcreg_icp_run_euler.argtypes = [vp, dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(IterLog), C.c_int,
                                      C.POINTER(IcpResult), dp]
    L.dcreg_icp_run_trials.argtypes = [vp, C.c_int, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(TrialResult)]
    i64p = C.POINTER(C.c_int64)
    L.dcreg_register_frames.argtypes = [vp, C.c_int, fp, i64p, C.c_int64, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.c_int,
                                        C.POINTER(TrialResult)]
    L.dcreg_frames_load.argtypes = [vp, C.c_int, fp, i64p, C.c_int64]
    L.dcreg_register_pairs.argtypes = [vp, C.c_int, fp, i64p, fp, i64p, C.c_int64, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.c_int,
                                       C.POINTER(TrialResult)]
    L.dcreg_frames_reserve_states.argtypes = [vp, C.c_int64]
    L.dcreg_frames_reset_state.argtypes = [vp, C.c_int64]
    L.dcreg_frames_batch_begin.argtypes = [vp, C.c_int, C.c_int, dp, dp, ip, ip, C.POINTER(LinParams)]
    if hasattr(L, "dcreg_target_insert"):      # (absent from an older build loaded through DCREG_LIB for an A/B)
        L.dcreg_target_insert.argtypes = [vp, fp, C.c_int64, C.c_int64, dp, dp, C.c_double, C.POINTER(MapUpdate)]
        L.dcreg_target_insert_device.argtypes = [vp, vp, C.c_int64, C.c_int64, dp, dp, C.c_double, C.POINTER(MapUpdate)]
        L.dcreg_target_insert_source.argtypes = [vp, dp, dp, C.c_double, C.POINTER(MapUpdate)]
        L.dcreg_target_crop.argtypes = [vp, dp, dp, C.POINTER(MapUpdate)]
        L.dcreg_target_get.argtypes = [vp, fp, C.c_int64]
        L.dcreg_debug_index_check.argtypes = [vp, C.POINTER(C.c_int64)]
    L.dcreg_voxel_downsample.argtypes = [vp, C.c_int, vp, i64p, C.c_int64, C.POINTER(VoxelParams), vp, C.c_int64, i64p, C.POINTER(VoxelInfo)]
    L.dcreg_voxel_downsample_device.argtypes = L.dcreg_voxel_downsample.argtypes
    for name in ("dcreg_set_source_voxel", "dcreg_set_source_voxel_device"):
        getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, C.POINTER(VoxelParams), C.POINTER(VoxelInfo)]
    for name in ("dcreg_set_target_voxel", "dcreg_set_target_voxel_device"):
        getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, C.POINTER(VoxelParams), C.c_double, C.POINTER(VoxelInfo)]
    if hasattr(L, "dcreg_deskew"):             # (absent from an older build loaded through DCREG_LIB for an A/B)
        L.dcreg_deskew.argtypes = [vp, C.c_int, vp, i64p, C.c_int64, C.POINTER(TimeField), C.POINTER(SweepMotion), C.POINTER(VoxelParams), vp,
                                   C.c_int64, i64p, C.POINTER(DeskewInfo), C.POINTER(VoxelInfo)]
        L.dcreg_deskew_device.argtypes = L.dcreg_deskew.argtypes
        for name in ("dcreg_set_source_deskew", "dcreg_set_source_deskew_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, C.POINTER(TimeField), C.POINTER(SweepMotion), C.POINTER(VoxelParams),
                                         C.POINTER(DeskewInfo), C.POINTER(VoxelInfo)]
    if hasattr(L, "dcreg_deskew_path"):
        tail = [C.POINTER(TimeField), C.c_int64, dp, dp, C.POINTER(SweepPath), C.POINTER(VoxelParams)]
        L.dcreg_deskew_path.argtypes = [vp, C.c_int, vp, i64p, C.c_int64] + tail + [vp, C.c_int64, i64p, C.POINTER(DeskewInfo), C.POINTER(VoxelInfo)]
        L.dcreg_deskew_path_device.argtypes = L.dcreg_deskew_path.argtypes
        for name in ("dcreg_set_source_deskew_path", "dcreg_set_source_deskew_path_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64] + tail + [C.POINTER(DeskewInfo), C.POINTER(VoxelInfo)]
    if hasattr(L, "dcreg_places_reset"):       # (absent from an older build loaded through DCREG_LIB for an A/B)
        pp, pi = C.POINTER(PlaceParams), C.POINTER(PlaceInfo)
        res = [C.c_int64, C.c_int64, C.c_int, ip, ip, dp]           # first, last, k, idx, shift, dist
        L.dcreg_default_place_params.argtypes = [pp]
        for name in ("dcreg_place_descriptors", "dcreg_place_descriptors_device"):
            getattr(L, name).argtypes = [vp, C.c_int, vp, i64p, C.c_int64, pp, vp, pi]
        L.dcreg_places_reset.argtypes = [vp, pp]
        L.dcreg_places_count.restype = C.c_int64
        L.dcreg_places_count.argtypes = [vp]
        L.dcreg_places_add.argtypes = [vp, C.c_int64, fp]
        for name in ("dcreg_places_add_clouds", "dcreg_places_add_clouds_device"):
            getattr(L, name).argtypes = [vp, C.c_int, vp, i64p, C.c_int64, pi]
        L.dcreg_places_add_source.argtypes = [vp, pi]
        L.dcreg_places_get.argtypes = [vp, C.c_int64, C.c_int64, fp]
        L.dcreg_places_query.argtypes = [vp, C.c_int, fp] + res
        for name in ("dcreg_places_query_clouds", "dcreg_places_query_clouds_device"):
            getattr(L, name).argtypes = [vp, C.c_int, vp, i64p, C.c_int64] + res + [pi]
        L.dcreg_places_query_source.argtypes = [vp] + res + [pi]
    if hasattr(L, "dcreg_outlier_filter"):     # (absent from an older build loaded through DCREG_LIB for an A/B)
        op, oi, vpp, vi = C.POINTER(OutlierParams), C.POINTER(OutlierInfo), C.POINTER(VoxelParams), C.POINTER(VoxelInfo)
        L.dcreg_default_outlier_params.argtypes = [op]
        for name in ("dcreg_outlier_filter", "dcreg_outlier_filter_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, op, vp, C.c_int64, i64p, vp, vp, oi]
        for name in ("dcreg_set_source_outliers", "dcreg_set_source_outliers_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, vpp, op, vi, oi]
        for name in ("dcreg_set_target_outliers", "dcreg_set_target_outliers_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, vpp, op, C.c_double, vi, oi]
        L.dcreg_target_remove_outliers.argtypes = [vp, op, oi]
    if hasattr(L, "dcreg_keyframes_reset"):    # (absent from an older build loaded through DCREG_LIB for an A/B)
        vpp, vi = C.POINTER(VoxelParams), C.POINTER(VoxelInfo)
        L.dcreg_keyframes_reset.argtypes = [vp]
        L.dcreg_keyframes_count.argtypes = [vp]
        L.dcreg_keyframes_count.restype = C.c_int64
        L.dcreg_keyframes_sizes.argtypes = [vp, C.c_int64, C.c_int64, i64p]
        for name in ("dcreg_keyframes_add_clouds", "dcreg_keyframes_add_clouds_device"):
            getattr(L, name).argtypes = [vp, C.c_int, vp, i64p, C.c_int64, i64p]
        L.dcreg_keyframes_add_source.argtypes = [vp, i64p]
        L.dcreg_keyframes_get.argtypes = [vp, C.c_int64, vp, C.c_int64]
        for name in ("dcreg_keyframes_submaps", "dcreg_keyframes_submaps_device"):
            getattr(L, name).argtypes = [vp, C.c_int, i64p, i64p, dp, vpp, vp, C.c_int64, i64p, vi]
        L.dcreg_set_target_keyframes.argtypes = [vp, C.c_int64, i64p, dp, vpp, C.c_double, vi]
    if hasattr(L, "dcreg_visibility_filter"):  # (absent from an older build loaded through DCREG_LIB for an A/B)
        sp, si = C.POINTER(VisibilityParams), C.POINTER(VisibilityInfo)
        L.dcreg_default_visibility_params.argtypes = [sp]
        for name in ("dcreg_keyframes_range_images", "dcreg_keyframes_range_images_device"):
            getattr(L, name).argtypes = [vp, C.c_int64, i64p, sp, vp]
        for name in ("dcreg_visibility_filter", "dcreg_visibility_filter_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, i64p, dp, sp, vp, C.c_int64, i64p, vp, vp, vp, si]
        L.dcreg_target_remove_dynamic.argtypes = [vp, C.c_int64, i64p, dp, sp, si]
    if hasattr(L, "dcreg_normals"):            # (absent from an older build loaded through DCREG_LIB for an A/B)
        np_, ni = C.POINTER(NormalParams), C.POINTER(NormalInfo)
        L.dcreg_default_normal_params.argtypes = [np_]
        for name in ("dcreg_normals", "dcreg_normals_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, np_, vp, vp, vp, ni]
        for name in ("dcreg_target_normals", "dcreg_target_normals_device"):
            getattr(L, name).argtypes = [vp, np_, vp, vp, vp, C.c_int64, ni]
    if hasattr(L, "dcreg_linearize_normals"):  # (likewise)
        L.dcreg_target_normals_keep.argtypes = [vp, C.POINTER(NormalParams), C.POINTER(NormalInfo)]
        for name in ("dcreg_target_normals_set", "dcreg_target_normals_set_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64]
        L.dcreg_target_normals_kept.argtypes = [vp]
        L.dcreg_target_normals_drop.argtypes = [vp]
        L.dcreg_linearize_normals.argtypes = [vp, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut)]
        L.dcreg_linearize_normals_debug.argtypes = [vp, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut), C.POINTER(NlinDebug)]
        L.dcreg_icp_run_normals.argtypes = [vp, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(IterLog), C.c_int, C.POINTER(IcpResult)]
    if hasattr(L, "dcreg_register_frames_normals"):  # (likewise)
        L.dcreg_register_frames_normals.argtypes = L.dcreg_register_frames.argtypes
        L.dcreg_icp_run_trials_normals.argtypes = L.dcreg_icp_run_trials.argtypes
        L.dcreg_normals_reserve_slots.argtypes = [vp, C.c_int64, C.c_int]
        L.dcreg_normals_reset_slot.argtypes = [vp, C.c_int64]
        L.dcreg_normals_batch_begin.argtypes = [vp, C.c_int, C.c_int, dp, dp, ip, ip, C.POINTER(LinParams)]
        L.dcreg_normals_batch_end.argtypes = [vp, C.c_int, C.POINTER(LinOut)]
    if hasattr(L, "dcreg_target_normals_get"):  # (likewise)
        for name in ("dcreg_target_normals_get", "dcreg_target_normals_get_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64]
        L.dcreg_target_normals_follow_info.argtypes = [vp, C.POINTER(NormalsFollowInfo)]
    if hasattr(L, "dcreg_linearize_gicp"):  # (likewise)
        L.dcreg_source_normals_keep.argtypes = [vp, C.POINTER(NormalParams), C.POINTER(NormalInfo)]
        for name in ("dcreg_source_normals_set", "dcreg_source_normals_set_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64]
        for name in ("dcreg_source_normals_get", "dcreg_source_normals_get_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64]
        L.dcreg_source_normals_kept.argtypes = [vp]
        L.dcreg_source_normals_drop.argtypes = [vp]
        L.dcreg_linearize_gicp.argtypes = [vp, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut)]
        L.dcreg_linearize_gicp_debug.argtypes = [vp, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut), C.POINTER(GlinDebug)]
        L.dcreg_icp_run_gicp.argtypes = [vp, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(IterLog), C.c_int, C.POINTER(IcpResult)]
    if hasattr(L, "dcreg_linearize_voxels"):  # (likewise)
        L.dcreg_default_voxel_map_params.argtypes = [C.POINTER(VoxelMapParams)]
        L.dcreg_target_voxels_keep.argtypes = [vp, C.POINTER(VoxelMapParams), C.POINTER(VoxelMapInfo)]
        L.dcreg_target_voxels_get.argtypes = [vp, vp, vp, vp, vp, C.c_int64]
        L.dcreg_target_voxels_kept.argtypes = [vp]
        L.dcreg_target_voxels_drop.argtypes = [vp]
    if hasattr(L, "dcreg_target_voxels_follow_info"):  # (likewise)
        L.dcreg_target_voxels_follow_info.argtypes = [vp, C.POINTER(VoxelsFollowInfo)]
        L.dcreg_linearize_voxels.argtypes = [vp, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut)]
        L.dcreg_linearize_voxels_debug.argtypes = [vp, dp, dp, C.POINTER(LinParams), C.POINTER(LinOut), C.POINTER(VlinDebug)]
        L.dcreg_icp_run_voxels.argtypes = [vp, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.POINTER(IterLog), C.c_int, C.POINTER(IcpResult)]
    if hasattr(L, "dcreg_register_frames_gicp"):  # (likewise)
        np_, ni = C.POINTER(NormalParams), C.POINTER(NormalInfo)
        for name in ("dcreg_normals_clouds", "dcreg_normals_clouds_device"):
            getattr(L, name).argtypes = [vp, C.c_int, vp, i64p, C.c_int64, np_, vp, vp, ni]
        L.dcreg_frames_normals_keep.argtypes = [vp, np_, ni]
        L.dcreg_frames_normals_set.argtypes = [vp, vp, C.c_int64, C.c_int64]
        L.dcreg_frames_normals_kept.argtypes = [vp]
        L.dcreg_gicp_batch_begin.argtypes = L.dcreg_normals_batch_begin.argtypes
        L.dcreg_gicp_batch_end.argtypes = L.dcreg_normals_batch_end.argtypes
        L.dcreg_normal_params_check.argtypes = [vp, np_]
        L.dcreg_register_frames_gicp.argtypes = [vp, C.c_int, fp, i64p, C.c_int64, np_, dp, dp, C.c_int, C.c_int, C.POINTER(Config), C.c_int,
                                                 C.POINTER(TrialResult)]
        L.dcreg_icp_run_trials_gicp.argtypes = L.dcreg_icp_run_trials.argtypes
    if hasattr(L, "dcreg_register_frames_voxels"):  # (likewise)
        L.dcreg_voxels_batch_begin.argtypes = [vp, C.c_int, C.c_int, dp, dp, ip, C.POINTER(LinParams)]
        L.dcreg_voxels_batch_end.argtypes = L.dcreg_normals_batch_end.argtypes
        L.dcreg_register_frames_voxels.argtypes = L.dcreg_register_frames_gicp.argtypes
        L.dcreg_icp_run_trials_voxels.argtypes = L.dcreg_icp_run_trials.argtypes
    if hasattr(L, "dcreg_register_pairs_normals"):  # (likewise)
        np_, ni, cfgp, trp = C.POINTER(NormalParams), C.POINTER(NormalInfo), C.POINTER(Config), C.POINTER(TrialResult)
        L.dcreg_register_pairs_normals.argtypes = [vp, C.c_int, fp, i64p, fp, i64p, C.c_int64, np_, dp, dp, C.c_int, C.c_int, cfgp, C.c_int, trp]
        L.dcreg_register_pairs_gicp.argtypes = [vp, C.c_int, fp, i64p, fp, i64p, C.c_int64, np_, np_, dp, dp, C.c_int, C.c_int, cfgp, C.c_int, trp]
        L.dcreg_pairs_sources_load.argtypes = [vp, C.c_int, fp, i64p, C.c_int64]
        L.dcreg_pairs_build.argtypes = [vp, C.c_int, fp, i64p, C.c_int64, C.c_double]
        for name in ("dcreg_pairs_normals_keep", "dcreg_pairs_sources_normals_keep"):
            getattr(L, name).argtypes = [vp, np_, ni]
        for name in ("dcreg_pairs_normals_set", "dcreg_pairs_sources_normals_set"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64]
        for name in ("dcreg_pairs_normals_get", "dcreg_pairs_sources_normals_get"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64]
        L.dcreg_pairs_normals_kept.argtypes = [vp]
        L.dcreg_pairs_normals_reserve_slots.argtypes = [vp, C.c_int64]
        for name in ("dcreg_pairs_normals_batch_begin", "dcreg_pairs_gicp_batch_begin"):
            getattr(L, name).argtypes = [vp, C.c_int, C.c_int, dp, dp, ip, ip, ip, C.POINTER(LinParams)]
    if hasattr(L, "dcreg_register_pairs_voxels"):  # (likewise)
        vmp, np_ = C.POINTER(VoxelMapParams), C.POINTER(NormalParams)
        L.dcreg_register_pairs_voxels.argtypes = [vp, C.c_int, fp, i64p, fp, i64p, C.c_int64, vmp, np_, dp, dp, C.c_int, C.c_int, C.POINTER(Config),
                                                  C.c_int, C.POINTER(TrialResult)]
        L.dcreg_pairs_plan_voxels.argtypes = [vp, C.c_int, i64p, C.c_int64, ip, C.POINTER(C.c_int)]
        L.dcreg_pairs_voxels_build.argtypes = [vp, C.c_int, fp, i64p, C.c_int64, vmp, C.POINTER(VoxelMapInfo)]
        L.dcreg_pairs_voxels_get.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int64]
        L.dcreg_pairs_voxels_kept.argtypes = [vp, C.c_int]
        L.dcreg_voxel_map_params_check.argtypes = [vp, vmp]
        L.dcreg_pairs_voxels_box_check.argtypes = [vp, fp, fp, C.c_double, C.c_int]
        L.dcreg_pairs_voxels_batch_begin.argtypes = [vp, C.c_int, C.c_int, dp, dp, ip, ip, C.POINTER(LinParams)]
    if hasattr(L, "dcreg_fpfh"):  # (likewise)
        np_, fpp, fpi = C.POINTER(NormalParams), C.POINTER(FpfhParams), C.POINTER(FpfhInfo)
        L.dcreg_default_fpfh_params.argtypes = [fpp]
        for name in ("dcreg_fpfh", "dcreg_fpfh_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, np_, fpp, vp, vp, fpi]
        for name in ("dcreg_target_fpfh", "dcreg_target_fpfh_device"):
            getattr(L, name).argtypes = [vp, fpp, vp, C.c_int64, fpi]
        L.dcreg_fpfh_debug_counts.argtypes = [vp, vp, C.c_int64]
        for name in ("dcreg_feature_match", "dcreg_feature_match_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, C.POINTER(MatchInfo)]
    if hasattr(L, "dcreg_fpfh_radius"):  # (likewise)
        np_, frp, fri = C.POINTER(NormalParams), C.POINTER(FpfhRadiusParams), C.POINTER(FpfhRadiusInfo)
        L.dcreg_default_fpfh_radius_params.argtypes = [frp]
        for name in ("dcreg_fpfh_radius", "dcreg_fpfh_radius_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, np_, frp, vp, vp, fri]
        for name in ("dcreg_target_fpfh_radius", "dcreg_target_fpfh_radius_device"):
            getattr(L, name).argtypes = [vp, frp, vp, C.c_int64, fri]
        L.dcreg_fpfh_radius_debug_counts.argtypes = [vp, vp, C.c_int64]
    if hasattr(L, "dcreg_align_correspondences"):  # (likewise)
        L.dcreg_default_align_params.argtypes = [C.POINTER(AlignParams)]
        for name in ("dcreg_align_correspondences", "dcreg_align_correspondences_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, C.c_int64, C.POINTER(AlignParams),
                                         C.POINTER(AlignRecord), vp, C.POINTER(AlignInfo)]
    if hasattr(L, "dcreg_consensus_correspondences"):  # (likewise)
        L.dcreg_default_consensus_params.argtypes = [C.POINTER(ConsensusParams)]
        for name in ("dcreg_consensus_correspondences", "dcreg_consensus_correspondences_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, C.c_int64, C.POINTER(ConsensusParams),
                                         C.POINTER(ConsensusRecord), vp, vp, vp, vp, C.POINTER(ConsensusInfo)]
    if hasattr(L, "dcreg_verify_poses"):  # (likewise)
        vpp, vrp, vip = C.POINTER(VerifyParams), C.POINTER(VerifyRecord), C.POINTER(VerifyInfo)
        L.dcreg_default_verify_params.argtypes = [vpp]
        L.dcreg_verify_poses.argtypes = [vp, vp, C.c_int64, C.c_int64, vpp, vrp, vp, vp, vip]
        for name in ("dcreg_verify_poses_cloud", "dcreg_verify_poses_cloud_device"):
            getattr(L, name).argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, vpp, vrp, vp, vp, vip]
    L.dcreg_p2p_error.argtypes = [vp, dp, C.c_double, dp, dp, dp, C.POINTER(C.c_int64)]
    L.dcreg_trial_pose.argtypes = [dp, C.c_uint64, C.c_int64, C.c_double, C.c_double, dp, dp]
    L.dcreg_set_host_threads.argtypes = [C.c_int]
    L.dcreg_get_host_threads.argtypes = []
    L.dcreg_icp_run_montecarlo.argtypes = [vp, dp, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_int,
                                           C.POINTER(Config), C.c_int, C.POINTER(TrialResult)]
    L.dcreg_montecarlo_job.argtypes = [vp, dp, C.c_uint64, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(Config), C.c_int, dp,
                                       C.POINTER(MethodStats)]
    L.dcreg_comm_allgather.argtypes = [vp, dp, dp, C.c_int64]
    L.dcreg_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dcreg_set_error_message.restype = None
    L.dcreg_set_error_message.argtypes = [vp, C.c_char_p]
    L.dcreg_sizeof.restype = C.c_size_t
    L.dcreg_sizeof.argtypes = [C.c_char_p]
    L.dcreg_version.restype = C.c_char_p
    for name, st in _STRUCTS.items():
        if L.dcreg_sizeof(name.encode()) != C.sizeof(st):
            raise DcregError("struct layout mismatch for %s" % name)
    _lib = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if n is not None:
        a = a.reshape(n)
    return a


def _points(a, what):
    """a cloud as the C-ABI takes it: 2-D float32, x y z in the first three columns, any further columns skipped through stride_floats"""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.float32 or a.shape[1] < 3:
        raise ValueError("%s: a 2-D float32 array with at least 3 columns (x y z first) is expected, got %s %s" % (what, a.dtype, a.shape))
    return np.ascontiguousarray(a)


def default_config(**kw):
    cfg = Config()
    load().dcreg_default_config(C.byref(cfg))
    for k, v in kw.items():
        if k == "gt_matrix":
            cfg.gt_matrix = (C.c_double * 16)(*_f64(v, 16))
        else:
            if not hasattr(cfg, k):
                raise AttributeError(k)
            setattr(cfg, k, v)
    return cfg


def default_lin_params(search_radius=1.0, use_weight_derivative=0, euler_rpy=None, euler_exact=False):
    """euler_rpy = (roll, pitch, yaw): the Euler row of the second engine (R, t passed to linearize must be the pose6d_matrix of
    that pose) - DCREG_PARAM_EULER = as the reference writes it (icp_test_runner.cpp:2299-2346), euler_exact =
    DCREG_PARAM_EULER_EXACT, the exact roll / pitch / yaw derivative."""
    p = LinParams()
    load().dcreg_default_lin_params(C.byref(p), float(search_radius))
    p.use_weight_derivative = int(use_weight_derivative)
    if euler_rpy is not None:
        p.parameterization = 2 if euler_exact else 1
        p.euler_rpy[:] = [float(v) for v in euler_rpy]
    return p


def unpack_hessian(H_upper):
    H = np.empty(36)
    load().dcreg_unpack_hessian(_dp(_f64(H_upper, 21)), _dp(H))
    return H.reshape(6, 6)


def analyze_degeneracy(H, detection, handling, cfg):
    an = Analysis()
    rc = load().dcreg_analyze_degeneracy(_dp(_f64(H, 36)), DETECTION[detection], HANDLING[handling], C.byref(cfg), C.byref(an))
    if rc:
        raise DcregError("dcreg_analyze_degeneracy rc=%d" % rc)
    return an


def analyze_degeneracy_two_part(H, detection, handling, cfg):
    """the analysis as the pipelined engine takes it (dcreg_debug.h) -> (Analysis, owed mask)"""
    an, owed = Analysis(), C.c_int(0)
    rc = load().dcreg_analyze_degeneracy_two_part(_dp(_f64(H, 36)), DETECTION[detection], HANDLING[handling], C.byref(cfg), C.byref(an), C.byref(owed))
    if rc:
        raise DcregError("dcreg_analyze_degeneracy_two_part rc=%d" % rc)
    return an, owed.value


def solve_degenerate_system(H, g, handling, cfg, an):
    x = np.empty(6)
    rc = load().dcreg_solve_degenerate_system(_dp(_f64(H, 36)), _dp(_f64(g, 6)), HANDLING[handling], C.byref(cfg), C.byref(an), _dp(x))
    if rc:
        raise DcregError("dcreg_solve_degenerate_system rc=%d" % rc)
    return x


def boxplus(R, t, dx):
    Ro, to = np.empty(9), np.empty(3)
    load().dcreg_boxplus(_dp(_f64(R, 9)), _dp(_f64(t, 3)), _dp(_f64(dx, 6)), _dp(Ro), _dp(to))
    return Ro.reshape(3, 3), to


def pose6d_to_matrix(roll, pitch, yaw, x, y, z):
    T = np.empty(16)
    load().dcreg_pose6d_to_matrix(roll, pitch, yaw, x, y, z, _dp(T))
    return T.reshape(4, 4)


def pose_error(gt, T):
    a, b = C.c_double(), C.c_double()
    load().dcreg_pose_error(_dp(_f64(gt, 16)), _dp(_f64(T, 16)), C.byref(a), C.byref(b))
    return a.value, b.value


def trial_pose(base_xyzrpy, seed, k, trans_amp, rot_amp_rad):
    """dcreg_trial_pose: initial pose of Monte-Carlo trial k (k == 0: the base pose), 4x4."""
    T = np.empty(16)
    rc = load().dcreg_trial_pose(_dp(_f64(base_xyzrpy, 6)), int(seed), int(k), float(trans_amp), float(rot_amp_rad), _dp(T), None)
    if rc:
        raise DcregError("dcreg_trial_pose rc=%d" % rc)
    return T.reshape(4, 4)


def set_host_threads(n):
    """dcreg_set_host_threads: OpenMP threads of the batched engines' host steps (overrides a launcher's OMP_NUM_THREADS=1)."""
    if load().dcreg_set_host_threads(int(n)) != 0:
        raise DcregError("dcreg_set_host_threads(%d)" % n)
    return load().dcreg_get_host_threads()


def comm_unique_id():
    """dcreg_comm_unique_id: 128 opaque bytes identifying a new RCCL communicator (rank 0 calls it and shares the bytes)."""
    buf = (C.c_char * 128)()
    rc = load().dcreg_comm_unique_id(C.cast(buf, C.c_void_p))
    if rc:
        raise DcregError("dcreg_comm_unique_id rc=%d (RCCL unavailable?)" % rc)
    return bytes(buf.raw)


def icp_run_many(contexts, T0s, method, cfg):
    """dcreg_icp_run_many: independent scan pairs (one Context each) at once, one host thread per pair."""
    n = len(contexts)
    T0s = _f64(T0s).reshape(n, 4, 4)
    R0 = np.ascontiguousarray(T0s[:, :3, :3]).reshape(n, 9)
    t0 = np.ascontiguousarray(T0s[:, :3, 3]).reshape(n, 3)
    det, hand = METHODS[method] if isinstance(method, str) else method
    handles = (C.c_void_p * max(n, 1))(*[c._h for c in contexts])
    res = (IcpResult * max(n, 1))()
    rc = load().dcreg_icp_run_many(n, handles, _dp(R0), _dp(t0), DETECTION[det], HANDLING[hand], C.byref(cfg), res)
    if rc:
        raise DcregError("dcreg_icp_run_many rc=%d" % rc)
    return [res[i] for i in range(n)]


class Context:
    """One device context (one GPU, one stream).  Stands for ICPContext (utils.hpp:340-425)."""

    def __init__(self, device=0):
        self._L = load()
        self._h = C.c_void_p()
        self._n_frames = 0            # frames the last successful load put on the device
        self._voxels_neighbors = 1    # "voxels_neighbors" as set_option last set it: the size of linearize_voxels' dump
        rc = self._L.dcreg_backend_create(C.byref(self._h), int(device))
        if rc != OK:
            self._h = None
            raise DcregError("dcreg_backend_create(device=%d) failed with %d: no usable HIP device and no CPU fallback" % (device, rc))
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.dcreg_backend_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != OK:
            raise DcregError("%s failed (%d): %s" % (what, rc, self._L.dcreg_last_error(self._h).decode()))

    def set_stream(self, hip_stream_ptr):
        self._check(self._L.dcreg_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)), "dcreg_set_stream")

    def set_option(self, key, value):
        self._check(self._L.dcreg_set_option(self._h, key.encode(), float(value)), "dcreg_set_option")
        if key == "voxels_neighbors":
            self._voxels_neighbors = int(value)

    def set_robust(self, kernel, scale=None, gicp_scale=None):
        """The robust kernel of linearize_normals / linearize_gicp and of every form built on them (include/dcreg.h, "robust kernels"):
        kernel a name of ROBUST or its code; scale: "robust_scale" (second engine, metres), gicp_scale: "gicp_robust_scale" (third engine,
        whitened units) - None leaves a scale as it is.  Everything is checked before anything reaches the library."""
        if isinstance(kernel, str):
            if kernel not in ROBUST:
                raise ValueError("set_robust: kernel: one of %s is expected, got %r" % (sorted(ROBUST), kernel))
            code = ROBUST[kernel]
        else:
            if isinstance(kernel, bool) or not isinstance(kernel, (int, np.integer)) or int(kernel) not in ROBUST.values():
                raise ValueError("set_robust: kernel: a name or code of %s is expected, got %r" % (ROBUST, kernel))
            code = int(kernel)
        for name, v in (("scale", scale), ("gicp_scale", gicp_scale)):
            if v is None:
                continue
            try:
                ok = ROBUST_SCALE_RANGE[0] <= float(v) <= ROBUST_SCALE_RANGE[1]
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("set_robust: %s: a finite value in [%g, %g] is expected, got %r" % ((name,) + ROBUST_SCALE_RANGE + (v,)))
        self.set_option("robust_kernel", code)
        if scale is not None:
            self.set_option("robust_scale", float(scale))
        if gicp_scale is not None:
            self.set_option("gicp_robust_scale", float(gicp_scale))

    def set_target(self, xyz, search_radius):
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        n, stride = a.shape[0], a.shape[1]
        self._check(self._L.dcreg_set_target(self._h, a.ctypes.data, n, stride, float(search_radius)), "dcreg_set_target")

    def set_source(self, xyz):
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        self._check(self._L.dcreg_set_source(self._h, a.ctypes.data, a.shape[0], a.shape[1]), "dcreg_set_source")

    def set_target_device(self, dev_ptr, n, stride, search_radius):
        self._check(self._L.dcreg_set_target_device(self._h, C.c_void_p(dev_ptr), n, stride, float(search_radius)), "dcreg_set_target_device")

    def set_source_device(self, dev_ptr, n, stride):
        self._check(self._L.dcreg_set_source_device(self._h, C.c_void_p(dev_ptr), n, stride), "dcreg_set_source_device")

    def voxel_downsample(self, clouds, leaf, mode="centroid", min_points=1):
        """dcreg_voxel_downsample: one point per occupied voxel of every cloud (include/dcreg.h has the rules).  clouds = a list of [n_i, c]
        float32 arrays, or (xyz [N, c], offsets [n + 1]) as register_frames takes them (c >= 3 columns, x y z first); leaf = one edge (cubic
        voxels) or three; mode "centroid" or "first"; min_points as PCL's setMinimumPointsNumberPerVoxel.  -> (the output in the shape of
        the input: a list of [m_i, 3] float32 arrays, or (xyz [M, 3], offsets [n + 1]); dict n_in / n_finite / n_voxels / n_out)"""
        p = voxel_params(leaf, mode, min_points)
        xyz, off, was_list = _clouds(clouds, "voxel_downsample")
        n = len(off) - 1
        out = np.empty((max(int(off[-1]), 1), 3), np.float32)
        out_off = np.zeros(n + 1, np.int64)
        info = VoxelInfo()
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.dcreg_voxel_downsample(self._h, n, xyz.ctypes.data, off.ctypes.data_as(i64p), xyz.shape[1], C.byref(p), out.ctypes.data,
                                                   int(off[-1]), out_off.ctypes.data_as(i64p), C.byref(info)), "dcreg_voxel_downsample")
        out = out[:int(out_off[-1])]
        if was_list:
            return [out[out_off[k]:out_off[k + 1]] for k in range(n)], _voxel_info_dict(info)
        return (out, out_off), _voxel_info_dict(info)

    def voxel_downsample_device(self, dev_ptr, offsets, stride, dev_out_ptr, capacity, leaf, mode="centroid", min_points=1):
        """dcreg_voxel_downsample_device: clouds in device memory (dev_ptr, stride floats per point, offsets on the host), the output to
        the device buffer dev_out_ptr (3 floats per point, capacity points).  -> (out_offsets [n + 1], info dict)"""
        p = voxel_params(leaf, mode, min_points)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise ValueError("voxel_downsample_device: offsets must start at 0 and not decrease")
        n = len(off) - 1
        out_off = np.zeros(n + 1, np.int64)
        info = VoxelInfo()
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.dcreg_voxel_downsample_device(self._h, n, C.c_void_p(dev_ptr), off.ctypes.data_as(i64p), int(stride), C.byref(p),
                                                          C.c_void_p(dev_out_ptr), int(capacity), out_off.ctypes.data_as(i64p), C.byref(info)),
                    "dcreg_voxel_downsample_device")
        return out_off, _voxel_info_dict(info)

    def set_source_voxel(self, xyz, leaf, mode="centroid", min_points=1):
        """dcreg_set_source_voxel: the cloud voxelised on the device and kept as the source (bitwise set_source(voxel_downsample(xyz)))"""
        p = voxel_params(leaf, mode, min_points)
        a = _points(xyz, "set_source_voxel")
        info = VoxelInfo()
        self._check(self._L.dcreg_set_source_voxel(self._h, a.ctypes.data, a.shape[0], a.shape[1], C.byref(p), C.byref(info)), "dcreg_set_source_voxel")
        return _voxel_info_dict(info)

    def set_source_voxel_device(self, dev_ptr, n, stride, leaf, mode="centroid", min_points=1):
        p = voxel_params(leaf, mode, min_points)
        info = VoxelInfo()
        self._check(self._L.dcreg_set_source_voxel_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.byref(p), C.byref(info)),
                    "dcreg_set_source_voxel_device")
        return _voxel_info_dict(info)

    def set_target_voxel(self, xyz, search_radius, leaf, mode="centroid", min_points=1):
        """dcreg_set_target_voxel: the cloud voxelised on the device and kept as the map (bitwise set_target(voxel_downsample(xyz)))"""
        p = voxel_params(leaf, mode, min_points)
        a = _points(xyz, "set_target_voxel")
        info = VoxelInfo()
        self._check(self._L.dcreg_set_target_voxel(self._h, a.ctypes.data, a.shape[0], a.shape[1], C.byref(p), float(search_radius), C.byref(info)),
                    "dcreg_set_target_voxel")
        return _voxel_info_dict(info)

    def set_target_voxel_device(self, dev_ptr, n, stride, search_radius, leaf, mode="centroid", min_points=1):
        p = voxel_params(leaf, mode, min_points)
        info = VoxelInfo()
        self._check(self._L.dcreg_set_target_voxel_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.byref(p), float(search_radius),
                                                          C.byref(info)), "dcreg_set_target_voxel_device")
        return _voxel_info_dict(info)

    def deskew(self, clouds, field, motions, leaf=None, mode="centroid", min_points=1):
        """dcreg_deskew: every cloud moved into the sensor frame at its reference instant from per-point stamps (include/dcreg.h has the
        rules).  clouds as voxel_downsample takes them, records of at least field.column + 1 (+ 1 for 64-bit stamps) float32 columns; field =
        time_field(...); motions = one sweep_motion per cloud (or one for all); leaf = None: every point out, in input order, or a voxel
        leaf: the voxel pass of the deskewed clouds.  -> (output in the shape of the input, deskew info dict, voxel info dict or None)"""
        xyz, off, was_list = _clouds(clouds, "deskew")
        n = len(off) - 1
        _check_field(field, xyz.shape[1], "deskew")
        mots = _motions(motions, n, "deskew")
        p = voxel_params(leaf, mode, min_points) if leaf is not None else None
        out = np.empty((max(int(off[-1]), 1), 3), np.float32)
        out_off = np.zeros(n + 1, np.int64)
        info, vinfo = DeskewInfo(), VoxelInfo()
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.dcreg_deskew(self._h, n, xyz.ctypes.data, off.ctypes.data_as(i64p), xyz.shape[1], C.byref(field), mots,
                                         C.byref(p) if p is not None else None, out.ctypes.data, int(off[-1]), out_off.ctypes.data_as(i64p),
                                         C.byref(info), C.byref(vinfo)), "dcreg_deskew")
        out = out[:int(out_off[-1])]
        vd = _voxel_info_dict(vinfo) if p is not None else None
        if was_list:
            return [out[out_off[k]:out_off[k + 1]] for k in range(n)], _deskew_info_dict(info), vd
        return (out, out_off), _deskew_info_dict(info), vd

    def deskew_device(self, dev_ptr, offsets, stride, field, motions, dev_out_ptr, capacity, leaf=None, mode="centroid", min_points=1):
        """dcreg_deskew_device: records in device memory (dev_ptr, stride floats each, offsets on the host), the output to the device buffer
        dev_out_ptr (3 floats per point, capacity points).  -> (out_offsets [n + 1], deskew info dict, voxel info dict or None)"""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise ValueError("deskew_device: offsets must start at 0 and not decrease")
        n = len(off) - 1
        _check_field(field, int(stride), "deskew_device")
        mots = _motions(motions, n, "deskew_device")
        p = voxel_params(leaf, mode, min_points) if leaf is not None else None
        out_off = np.zeros(n + 1, np.int64)
        info, vinfo = DeskewInfo(), VoxelInfo()
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.dcreg_deskew_device(self._h, n, C.c_void_p(dev_ptr), off.ctypes.data_as(i64p), int(stride), C.byref(field), mots,
                                                C.byref(p) if p is not None else None, C.c_void_p(dev_out_ptr), int(capacity),
                                                out_off.ctypes.data_as(i64p), C.byref(info), C.byref(vinfo)), "dcreg_deskew_device")
        return out_off, _deskew_info_dict(info), (_voxel_info_dict(vinfo) if p is not None else None)

    def set_source_deskew(self, records, field, motion, leaf=None, mode="centroid", min_points=1):
        """dcreg_set_source_deskew: one sweep deskewed on the device and kept as the source (bitwise set_source / set_source_voxel of its
        deskew output).  -> (deskew info dict, voxel info dict or None)"""
        a = _points(records, "set_source_deskew")
        _check_field(field, a.shape[1], "set_source_deskew")
        m = _motions(motion, 1, "set_source_deskew")
        p = voxel_params(leaf, mode, min_points) if leaf is not None else None
        info, vinfo = DeskewInfo(), VoxelInfo()
        self._check(self._L.dcreg_set_source_deskew(self._h, a.ctypes.data, a.shape[0], a.shape[1], C.byref(field), m,
                                                    C.byref(p) if p is not None else None, C.byref(info), C.byref(vinfo)), "dcreg_set_source_deskew")
        return _deskew_info_dict(info), (_voxel_info_dict(vinfo) if p is not None else None)

    def set_source_deskew_device(self, dev_ptr, n, stride, field, motion, leaf=None, mode="centroid", min_points=1):
        _check_field(field, int(stride), "set_source_deskew_device")
        m = _motions(motion, 1, "set_source_deskew_device")
        p = voxel_params(leaf, mode, min_points) if leaf is not None else None
        info, vinfo = DeskewInfo(), VoxelInfo()
        self._check(self._L.dcreg_set_source_deskew_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.byref(field), m,
                                                           C.byref(p) if p is not None else None, C.byref(info), C.byref(vinfo)),
                    "dcreg_set_source_deskew_device")
        return _deskew_info_dict(info), (_voxel_info_dict(vinfo) if p is not None else None)

    def deskew_path(self, clouds, field, knot_stamps, knot_poses, paths, leaf=None, mode="centroid", min_points=1):
        """dcreg_deskew_path: deskew as above, the pose at a point's stamp read off a sampled trajectory through a sensor-to-body extrinsic
        (include/dcreg.h has the rule).  knot_stamps [K] seconds and knot_poses [K, 12] (R row-major then t) or [K, 4, 4]: the BODY's poses
        in any fixed frame; paths = one sweep_path per cloud (or one for all).  The output is each sweep in its sensor frame at its t_ref.
        -> as deskew"""
        xyz, off, was_list = _clouds(clouds, "deskew_path")
        n = len(off) - 1
        _check_field(field, xyz.shape[1], "deskew_path")
        st, P = _knot_table(knot_stamps, knot_poses, "deskew_path")
        blocks = _paths(paths, n, st, P, "deskew_path")
        p = voxel_params(leaf, mode, min_points) if leaf is not None else None
        out = np.empty((max(int(off[-1]), 1), 3), np.float32)
        out_off = np.zeros(n + 1, np.int64)
        info, vinfo = DeskewInfo(), VoxelInfo()
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.dcreg_deskew_path(self._h, n, xyz.ctypes.data, off.ctypes.data_as(i64p), xyz.shape[1], C.byref(field), len(st), _dp(st),
                                              _dp(P), blocks, C.byref(p) if p is not None else None, out.ctypes.data, int(off[-1]),
                                              out_off.ctypes.data_as(i64p), C.byref(info), C.byref(vinfo)), "dcreg_deskew_path")
        out = out[:int(out_off[-1])]
        vd = _voxel_info_dict(vinfo) if p is not None else None
        if was_list:
            return [out[out_off[k]:out_off[k + 1]] for k in range(n)], _deskew_info_dict(info), vd
        return (out, out_off), _deskew_info_dict(info), vd

    def deskew_path_device(self, dev_ptr, offsets, stride, field, knot_stamps, knot_poses, paths, dev_out_ptr, capacity, leaf=None,
                           mode="centroid", min_points=1):
        """dcreg_deskew_path_device: records and output in device memory as deskew_device takes them; the knot table and the blocks on the host.
        -> (out_offsets [n + 1], deskew info dict, voxel info dict or None)"""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
            raise ValueError("deskew_path_device: offsets must start at 0 and not decrease")
        n = len(off) - 1
        _check_field(field, int(stride), "deskew_path_device")
        st, P = _knot_table(knot_stamps, knot_poses, "deskew_path_device")
        blocks = _paths(paths, n, st, P, "deskew_path_device")
        p = voxel_params(leaf, mode, min_points) if leaf is not None else None
        out_off = np.zeros(n + 1, np.int64)
        info, vinfo = DeskewInfo(), VoxelInfo()
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.dcreg_deskew_path_device(self._h, n, C.c_void_p(dev_ptr), off.ctypes.data_as(i64p), int(stride), C.byref(field),
                                                     len(st), _dp(st), _dp(P), blocks, C.byref(p) if p is not None else None,
                                                     C.c_void_p(dev_out_ptr), int(capacity), out_off.ctypes.data_as(i64p), C.byref(info),
                                                     C.byref(vinfo)), "dcreg_deskew_path_device")
        return out_off, _deskew_info_dict(info), (_voxel_info_dict(vinfo) if p is not None else None)

    def set_source_deskew_path(self, records, field, knot_stamps, knot_poses, path, leaf=None, mode="centroid", min_points=1):
        """dcreg_set_source_deskew_path: one sweep deskewed along its path on the device and kept as the source (bitwise set_source /
        set_source_voxel of its deskew_path output).  -> (deskew info dict, voxel info dict or None)"""
        a = _points(records, "set_source_deskew_path")
        _check_field(field, a.shape[1], "set_source_deskew_path")
        st, P = _knot_table(knot_stamps, knot_poses, "set_source_deskew_path")
        block = _paths(path, 1, st, P, "set_source_deskew_path")
        p = voxel_params(leaf, mode, min_points) if leaf is not None else None
        info, vinfo = DeskewInfo(), VoxelInfo()
        self._check(self._L.dcreg_set_source_deskew_path(self._h, a.ctypes.data, a.shape[0], a.shape[1], C.byref(field), len(st), _dp(st), _dp(P),
                                                         block, C.byref(p) if p is not None else None, C.byref(info), C.byref(vinfo)),
                    "dcreg_set_source_deskew_path")
        return _deskew_info_dict(info), (_voxel_info_dict(vinfo) if p is not None else None)

    def set_source_deskew_path_device(self, dev_ptr, n, stride, field, knot_stamps, knot_poses, path, leaf=None, mode="centroid", min_points=1):
        _check_field(field, int(stride), "set_source_deskew_path_device")
        st, P = _knot_table(knot_stamps, knot_poses, "set_source_deskew_path_device")
        block = _paths(path, 1, st, P, "set_source_deskew_path_device")
        p = voxel_params(leaf, mode, min_points) if leaf is not None else None
        info, vinfo = DeskewInfo(), VoxelInfo()
        self._check(self._L.dcreg_set_source_deskew_path_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.byref(field), len(st), _dp(st),
                                                                _dp(P), block, C.byref(p) if p is not None else None, C.byref(info),
                                                                C.byref(vinfo)), "dcreg_set_source_deskew_path_device")
        return _deskew_info_dict(info), (_voxel_info_dict(vinfo) if p is not None else None)

    # ---- place recognition (include/dcreg.h has the rules)
    def place_descriptors(self, clouds, params=None):
        """dcreg_place_descriptors: the Scan Context descriptor of every cloud (clouds as voxel_downsample takes them); the database is
        not touched.  -> ([n, n_rings, n_sectors] float32, dict n_in / n_finite / n_used)"""
        p = params if params is not None else place_params()
        _check_place_params(p, "place_descriptors")
        xyz, off, _ = _clouds(clouds, "place_descriptors")
        n = len(off) - 1
        out = np.zeros((n, p.n_rings, p.n_sectors), np.float32)
        info = PlaceInfo()
        self._check(self._L.dcreg_place_descriptors(self._h, n, xyz.ctypes.data, off.ctypes.data_as(C.POINTER(C.c_int64)), xyz.shape[1], C.byref(p),
                                                    out.ctypes.data, C.byref(info)), "dcreg_place_descriptors")
        return out, _place_info_dict(info)

    def place_descriptors_device(self, dev_ptr, offsets, stride, dev_out_ptr, params=None):
        """dcreg_place_descriptors_device: clouds in device memory (dev_ptr, stride floats per point, offsets on the host), the descriptors
        to the device buffer dev_out_ptr (n * n_rings * n_sectors floats) -> info dict"""
        p = params if params is not None else place_params()
        _check_place_params(p, "place_descriptors_device")
        off = _offsets(offsets, "place_descriptors_device")
        if int(stride) < 3:
            raise ValueError("place_descriptors_device: a stride of at least 3 floats is expected, got %d" % int(stride))
        info = PlaceInfo()
        self._check(self._L.dcreg_place_descriptors_device(self._h, len(off) - 1, C.c_void_p(dev_ptr), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                           int(stride), C.byref(p), C.c_void_p(dev_out_ptr), C.byref(info)),
                    "dcreg_place_descriptors_device")
        return _place_info_dict(info)

    def places_reset(self, params=None):
        """dcreg_places_reset: an empty place database with these parameters (place_params(...); the defaults when None)"""
        p = params if params is not None else place_params()
        _check_place_params(p, "places_reset")
        self._check(self._L.dcreg_places_reset(self._h, C.byref(p)), "dcreg_places_reset")
        self._place_shape = (p.n_rings, p.n_sectors)

    def _places_shape(self, what):
        shape = getattr(self, "_place_shape", None)
        if shape is None:
            raise ValueError("%s: no place database (places_reset first)" % what)
        return shape

    def places_count(self):
        return int(self._L.dcreg_places_count(self._h))

    def places_add(self, desc):
        """dcreg_places_add: host descriptors ([n, n_rings, n_sectors] or [n, n_rings * n_sectors], finite) appended -> index of the first"""
        R, S = self._places_shape("places_add")
        d = _descriptors(desc, R * S, "places_add")
        at = self.places_count()
        self._check(self._L.dcreg_places_add(self._h, d.shape[0], d.ctypes.data_as(C.POINTER(C.c_float))), "dcreg_places_add")
        return at

    def places_add_clouds(self, clouds):
        """dcreg_places_add_clouds: the descriptors of the clouds computed and appended on the device -> (index of the first, info dict)"""
        self._places_shape("places_add_clouds")
        xyz, off, _ = _clouds(clouds, "places_add_clouds")
        info = PlaceInfo()
        at = self.places_count()
        self._check(self._L.dcreg_places_add_clouds(self._h, len(off) - 1, xyz.ctypes.data, off.ctypes.data_as(C.POINTER(C.c_int64)), xyz.shape[1],
                                                    C.byref(info)), "dcreg_places_add_clouds")
        return at, _place_info_dict(info)

    def places_add_clouds_device(self, dev_ptr, offsets, stride):
        self._places_shape("places_add_clouds_device")
        off = _offsets(offsets, "places_add_clouds_device")
        if int(stride) < 3:
            raise ValueError("places_add_clouds_device: a stride of at least 3 floats is expected, got %d" % int(stride))
        info = PlaceInfo()
        at = self.places_count()
        self._check(self._L.dcreg_places_add_clouds_device(self._h, len(off) - 1, C.c_void_p(dev_ptr), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                           int(stride), C.byref(info)), "dcreg_places_add_clouds_device")
        return at, _place_info_dict(info)

    def places_add_source(self):
        """dcreg_places_add_source: the descriptor of the current source appended -> (its index, info dict)"""
        self._places_shape("places_add_source")
        info = PlaceInfo()
        at = self.places_count()
        self._check(self._L.dcreg_places_add_source(self._h, C.byref(info)), "dcreg_places_add_source")
        return at, _place_info_dict(info)

    def places_get(self, first=0, n=None):
        """dcreg_places_get: entries [first, first + n) (to the end when n is None) -> [n, n_rings, n_sectors] float32"""
        R, S = self._places_shape("places_get")
        if int(first) < 0 or (n is not None and int(n) < 0):
            raise ValueError("places_get: first >= 0 and n >= 0 are expected, got %d and %s" % (int(first), n))
        if n is None:
            n = max(self.places_count() - int(first), 0)
        out = np.zeros((int(n), R, S), np.float32)
        self._check(self._L.dcreg_places_get(self._h, int(first), int(n), out.ctypes.data_as(C.POINTER(C.c_float))), "dcreg_places_get")
        return out

    def _place_results(self, n, k):
        return np.full((n, k), -1, np.int32), np.zeros((n, k), np.int32), np.full((n, k), np.inf, np.float64)

    def _place_range(self, first, last, k, what):
        if last is None:
            last = self.places_count()
        _check_range(first, last, k, what)
        return int(first), int(last), int(k)

    def places_query(self, desc, k=1, first=0, last=None):
        """dcreg_places_query: for every host descriptor the k entries of [first, last) (to the end when last is None) with the smallest
        distance, ordered by (distance, index) -> (idx [n, k] int32, shift [n, k] int32, dist [n, k] float64); unused slots -1, 0, inf"""
        R, S = self._places_shape("places_query")
        d = _descriptors(desc, R * S, "places_query")
        first, last, k = self._place_range(first, last, k, "places_query")
        idx, shift, dist = self._place_results(d.shape[0], k)
        ip = C.POINTER(C.c_int32)
        self._check(self._L.dcreg_places_query(self._h, d.shape[0], d.ctypes.data_as(C.POINTER(C.c_float)), first, last, k, idx.ctypes.data_as(ip),
                                               shift.ctypes.data_as(ip), _dp(dist)), "dcreg_places_query")
        return idx, shift, dist

    def places_query_clouds(self, clouds, k=1, first=0, last=None):
        """dcreg_places_query_clouds: one query per cloud, its descriptor computed on the device -> (idx, shift, dist, info dict)"""
        self._places_shape("places_query_clouds")
        xyz, off, _ = _clouds(clouds, "places_query_clouds")
        first, last, k = self._place_range(first, last, k, "places_query_clouds")
        n = len(off) - 1
        idx, shift, dist = self._place_results(n, k)
        info = PlaceInfo()
        ip = C.POINTER(C.c_int32)
        self._check(self._L.dcreg_places_query_clouds(self._h, n, xyz.ctypes.data, off.ctypes.data_as(C.POINTER(C.c_int64)), xyz.shape[1], first, last,
                                                      k, idx.ctypes.data_as(ip), shift.ctypes.data_as(ip), _dp(dist), C.byref(info)),
                    "dcreg_places_query_clouds")
        return idx, shift, dist, _place_info_dict(info)

    def places_query_clouds_device(self, dev_ptr, offsets, stride, k=1, first=0, last=None):
        self._places_shape("places_query_clouds_device")
        off = _offsets(offsets, "places_query_clouds_device")
        if int(stride) < 3:
            raise ValueError("places_query_clouds_device: a stride of at least 3 floats is expected, got %d" % int(stride))
        first, last, k = self._place_range(first, last, k, "places_query_clouds_device")
        n = len(off) - 1
        idx, shift, dist = self._place_results(n, k)
        info = PlaceInfo()
        ip = C.POINTER(C.c_int32)
        self._check(self._L.dcreg_places_query_clouds_device(self._h, n, C.c_void_p(dev_ptr), off.ctypes.data_as(C.POINTER(C.c_int64)), int(stride),
                                                             first, last, k, idx.ctypes.data_as(ip), shift.ctypes.data_as(ip), _dp(dist),
                                                             C.byref(info)), "dcreg_places_query_clouds_device")
        return idx, shift, dist, _place_info_dict(info)

    def places_query_source(self, k=1, first=0, last=None):
        """dcreg_places_query_source: the current source as the one query -> (idx [k], shift [k], dist [k], info dict)"""
        self._places_shape("places_query_source")
        first, last, k = self._place_range(first, last, k, "places_query_source")
        idx, shift, dist = self._place_results(1, k)
        info = PlaceInfo()
        ip = C.POINTER(C.c_int32)
        self._check(self._L.dcreg_places_query_source(self._h, first, last, k, idx.ctypes.data_as(ip), shift.ctypes.data_as(ip), _dp(dist),
                                                      C.byref(info)), "dcreg_places_query_source")
        return idx[0], shift[0], dist[0], _place_info_dict(info)

    def outlier_filter(self, xyz, params=None, want_mask=True, want_scores=True):
        """dcreg_outlier_filter: the points of one cloud ([n, c] float32, x y z first; non-finite points are dropped) that pass the
        statistical or radius filter of params (outlier_params(...); None = the defaults), in input order (include/dcreg.h has the
        rules).  -> (kept [m, 3] float32, keep mask [n] bool or None, scores [n] float32 or None, dict n_in / n_finite / n_sparse /
        n_out / mean / stddev / threshold)"""
        p = params if params is not None else outlier_params()
        _check_outlier_params(p, "outlier_filter")
        a = _points(xyz, "outlier_filter")
        n = a.shape[0]
        out = np.empty((max(n, 1), 3), np.float32)
        mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
        scores = np.full(max(n, 1), np.nan, np.float32) if want_scores else None
        n_out = C.c_int64(0)
        info = OutlierInfo()
        self._check(self._L.dcreg_outlier_filter(self._h, a.ctypes.data, n, a.shape[1], C.byref(p), out.ctypes.data, n, C.byref(n_out),
                                                 mask.ctypes.data if want_mask else None, scores.ctypes.data if want_scores else None,
                                                 C.byref(info)), "dcreg_outlier_filter")
        return (out[:n_out.value], mask[:n].astype(bool) if want_mask else None, scores[:n] if want_scores else None,
                _outlier_info_dict(info))

    def outlier_filter_device(self, dev_ptr, n, stride, dev_out_ptr, capacity, params=None, dev_mask_ptr=0, dev_scores_ptr=0):
        """dcreg_outlier_filter_device: the cloud in device memory, the kept points to dev_out_ptr (3 floats per point, capacity points),
        optionally the uint8 mask and the float scores to device buffers of n entries.  -> (n_out, info dict)"""
        p = params if params is not None else outlier_params()
        _check_outlier_params(p, "outlier_filter_device")
        _check_device_cloud(n, stride, "outlier_filter_device")
        if int(capacity) < 0:
            raise ValueError("outlier_filter_device: a capacity >= 0 is expected, got %d" % int(capacity))
        n_out = C.c_int64(0)
        info = OutlierInfo()
        self._check(self._L.dcreg_outlier_filter_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.byref(p), C.c_void_p(dev_out_ptr),
                                                        int(capacity), C.byref(n_out), C.c_void_p(dev_mask_ptr or None),
                                                        C.c_void_p(dev_scores_ptr or None), C.byref(info)), "dcreg_outlier_filter_device")
        return n_out.value, _outlier_info_dict(info)

    def _set_outliers(self, name, ptr, n, stride, params, leaf, mode, min_points, search_radius=None):
        p = params if params is not None else outlier_params()
        _check_outlier_params(p, name)
        v = voxel_params(leaf, mode, min_points) if leaf is not None else None
        _check_device_cloud(n, stride, name)
        vinfo, info = VoxelInfo(), OutlierInfo()
        args = [self._h, ptr, int(n), int(stride), C.byref(v) if v is not None else None, C.byref(p)]
        if search_radius is not None:
            args.append(float(search_radius))
        self._check(getattr(self._L, "dcreg_" + name)(*(args + [C.byref(vinfo), C.byref(info)])), "dcreg_" + name)
        return _outlier_info_dict(info), (_voxel_info_dict(vinfo) if v is not None else None)

    def set_source_outliers(self, xyz, params=None, leaf=None, mode="centroid", min_points=1):
        """dcreg_set_source_outliers: the cloud filtered on the device (leaf given: voxelised first) and kept as the source - bitwise
        set_source(outlier_filter(xyz)).  -> (outlier info dict, voxel info dict or None)"""
        a = _points(xyz, "set_source_outliers")
        return self._set_outliers("set_source_outliers", a.ctypes.data, a.shape[0], a.shape[1], params, leaf, mode, min_points)

    def set_source_outliers_device(self, dev_ptr, n, stride, params=None, leaf=None, mode="centroid", min_points=1):
        return self._set_outliers("set_source_outliers_device", C.c_void_p(dev_ptr), n, stride, params, leaf, mode, min_points)

    def set_target_outliers(self, xyz, search_radius, params=None, leaf=None, mode="centroid", min_points=1):
        """dcreg_set_target_outliers: the cloud filtered on the device (leaf given: voxelised first) and kept as the map - bitwise
        set_target(outlier_filter(xyz), search_radius).  -> (outlier info dict, voxel info dict or None)"""
        a = _points(xyz, "set_target_outliers")
        return self._set_outliers("set_target_outliers", a.ctypes.data, a.shape[0], a.shape[1], params, leaf, mode, min_points, search_radius)

    def set_target_outliers_device(self, dev_ptr, n, stride, search_radius, params=None, leaf=None, mode="centroid", min_points=1):
        return self._set_outliers("set_target_outliers_device", C.c_void_p(dev_ptr), n, stride, params, leaf, mode, min_points, search_radius)

    def remove_outliers(self, params=None):
        """dcreg_target_remove_outliers: the resident map cleaned in place (later calls are bitwise set_target of the cleaned cloud).
        -> dict n_in / n_finite / n_sparse / n_out / mean / stddev / threshold"""
        p = params if params is not None else outlier_params()
        _check_outlier_params(p, "remove_outliers")
        info = OutlierInfo()
        self._check(self._L.dcreg_target_remove_outliers(self._h, C.byref(p), C.byref(info)), "dcreg_target_remove_outliers")
        return _outlier_info_dict(info)

    @staticmethod
    def _normal_wants(want_normals, want_curvature, want_eigenvalues, what):
        if not (want_normals or want_curvature or want_eigenvalues):
            raise ValueError("%s: at least one of normals, curvature and eigenvalues is expected" % what)

    def normals(self, xyz, params=None, want_normals=True, want_curvature=True, want_eigenvalues=False):
        """dcreg_normals: per point of one cloud ([n, c] float32, x y z first) the normal of the plane through its k nearest points (itself
        among them), the surface variation and optionally the three eigenvalues of the neighbourhood's covariance, ascending (PCL
        NormalEstimation with setKSearch; include/dcreg.h has the rule).  Non-finite and sparse points get NaN.  params: normal_params(...),
        None = the defaults.  -> (normals [n, 3] float32 or None, curvature [n] float32 or None, eigenvalues [n, 3] float32 or None,
        dict n_in / n_finite / n_sparse / n_out)"""
        p = params if params is not None else normal_params()
        _check_normal_params(p, "normals")
        self._normal_wants(want_normals, want_curvature, want_eigenvalues, "normals")
        a = _points(xyz, "normals")
        n = a.shape[0]
        nrm = np.full((max(n, 1), 3), np.nan, np.float32) if want_normals else None
        cur = np.full(max(n, 1), np.nan, np.float32) if want_curvature else None
        eig = np.full((max(n, 1), 3), np.nan, np.float32) if want_eigenvalues else None
        info = NormalInfo()
        self._check(self._L.dcreg_normals(self._h, a.ctypes.data, n, a.shape[1], C.byref(p), nrm.ctypes.data if want_normals else None,
                                          cur.ctypes.data if want_curvature else None, eig.ctypes.data if want_eigenvalues else None,
                                          C.byref(info)), "dcreg_normals")
        return (nrm[:n] if want_normals else None, cur[:n] if want_curvature else None, eig[:n] if want_eigenvalues else None,
                _normal_info_dict(info))

    def normals_device(self, dev_ptr, n, stride, params=None, dev_normals_ptr=0, dev_curvature_ptr=0, dev_eigenvalues_ptr=0):
        """dcreg_normals_device: the cloud in device memory; the normals (3 n floats), curvature (n floats) and eigenvalues (3 n floats) to
        the device buffers given (0: not wanted).  -> info dict"""
        p = params if params is not None else normal_params()
        _check_normal_params(p, "normals_device")
        _check_device_cloud(n, stride, "normals_device")
        self._normal_wants(dev_normals_ptr, dev_curvature_ptr, dev_eigenvalues_ptr, "normals_device")
        info = NormalInfo()
        self._check(self._L.dcreg_normals_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.byref(p), C.c_void_p(dev_normals_ptr or None),
                                                 C.c_void_p(dev_curvature_ptr or None), C.c_void_p(dev_eigenvalues_ptr or None),
                                                 C.byref(info)), "dcreg_normals_device")
        return _normal_info_dict(info)

    def normals_clouds(self, clouds, params=None, want_normals=True, want_curvature=True):
        """dcreg_normals_clouds: normals() of many clouds in one call - a list of [n_i, c] float32 arrays or an (xyz, offsets) pair; every
        cloud is indexed on its own, all of them in one build and one launch, and every value is bitwise what normals() returns for the
        cloud alone.  -> (normals [N, 3] float32 or None, curvature [N] float32 or None, offsets [n + 1] int64, [info dict per cloud]);
        cloud s is rows offsets[s]:offsets[s + 1]"""
        p = params if params is not None else normal_params()
        _check_normal_params(p, "normals_clouds")
        self._normal_wants(want_normals, want_curvature, False, "normals_clouds")
        xyz, off, _ = _clouds(clouds, "normals_clouds")
        n_clouds, n = len(off) - 1, int(off[-1])
        if n > OUTLIER_MAX_POINTS:
            raise ValueError("normals_clouds: at most 2^31 - 1 points a call, got %d" % n)
        nrm = np.full((max(n, 1), 3), np.nan, np.float32) if want_normals else None
        cur = np.full(max(n, 1), np.nan, np.float32) if want_curvature else None
        infos = (NormalInfo * max(n_clouds, 1))()
        self._check(self._L.dcreg_normals_clouds(self._h, n_clouds, xyz.ctypes.data, off.ctypes.data_as(C.POINTER(C.c_int64)), xyz.shape[1], C.byref(p),
                                                 nrm.ctypes.data if want_normals else None, cur.ctypes.data if want_curvature else None, infos),
                    "dcreg_normals_clouds")
        return (nrm[:n] if want_normals else None, cur[:n] if want_curvature else None, off, [_normal_info_dict(infos[s]) for s in range(n_clouds)])

    def normals_clouds_device(self, dev_ptr, offsets, stride, params=None, dev_normals_ptr=0, dev_curvature_ptr=0):
        """dcreg_normals_clouds_device: the clouds back to back in device memory (offsets on the host); the normals (3 N floats) and the
        curvature (N floats) to the device buffers given (0: not wanted).  -> [info dict per cloud]"""
        p = params if params is not None else normal_params()
        _check_normal_params(p, "normals_clouds_device")
        off = _offsets(offsets, "normals_clouds_device")
        _check_device_cloud(int(off[-1]), stride, "normals_clouds_device")
        self._normal_wants(dev_normals_ptr, dev_curvature_ptr, False, "normals_clouds_device")
        n_clouds = len(off) - 1
        infos = (NormalInfo * max(n_clouds, 1))()
        self._check(self._L.dcreg_normals_clouds_device(self._h, n_clouds, C.c_void_p(dev_ptr), off.ctypes.data_as(C.POINTER(C.c_int64)), int(stride),
                                                        C.byref(p), C.c_void_p(dev_normals_ptr or None), C.c_void_p(dev_curvature_ptr or None), infos),
                    "dcreg_normals_clouds_device")
        return [_normal_info_dict(infos[s]) for s in range(n_clouds)]

    def target_normals(self, params=None, want_normals=True, want_curvature=True, want_eigenvalues=False):
        """dcreg_target_normals: the same for the resident map's points in index order (target_points()), searched through the map's own
        index - what ICPContext::setTargetCloud(target, normal_nn) keeps in targetNormals.  The map is untouched.
        -> (normals, curvature, eigenvalues, info dict) as normals()"""
        p = params if params is not None else normal_params()
        _check_normal_params(p, "target_normals")
        self._normal_wants(want_normals, want_curvature, want_eigenvalues, "target_normals")
        n = max(int(self.index_info().n_target), 0)
        nrm = np.full((max(n, 1), 3), np.nan, np.float32) if want_normals else None
        cur = np.full(max(n, 1), np.nan, np.float32) if want_curvature else None
        eig = np.full((max(n, 1), 3), np.nan, np.float32) if want_eigenvalues else None
        info = NormalInfo()
        self._check(self._L.dcreg_target_normals(self._h, C.byref(p), nrm.ctypes.data if want_normals else None,
                                                 cur.ctypes.data if want_curvature else None, eig.ctypes.data if want_eigenvalues else None,
                                                 n, C.byref(info)), "dcreg_target_normals")
        return (nrm[:n] if want_normals else None, cur[:n] if want_curvature else None, eig[:n] if want_eigenvalues else None,
                _normal_info_dict(info))

    # ---- FPFH descriptors and feature-space matching (include/dcreg.h: dcreg_fpfh .. dcreg_feature_match)
    def fpfh(self, cloud, normals=None, normal_params=None, params=None, want_normals=False):
        """dcreg_fpfh: per point of one cloud ([n, c] float32, x y z first) its FPFH descriptor, 33 floats - three histograms of 11 bins,
        each summing to 100 (PCL FPFHEstimation with setKSearch; include/dcreg.h has the rule).  normals: [n, c] float32, the normal in
        the first three columns; None = they are estimated first with normal_params (normal_params(...), None = its defaults) on the same
        index, and returned with want_normals.  A point without finite coordinates and a finite normal, and an EMPTY point, get NaN.
        params: fpfh_params(...), None = the defaults.  -> (fpfh [n, 33] float32, normals [n, 3] float32 or None, dict n_in / n_used /
        n_empty / n_out)"""
        p = params if params is not None else fpfh_params()
        _check_fpfh_params(p, "fpfh")
        a = _points(cloud, "fpfh")
        n = a.shape[0]
        nrm_in = npb = None
        if normals is not None:
            nrm_in = _points(normals, "fpfh")
            if nrm_in.shape[0] != n:
                raise ValueError("fpfh: one normal per point is expected, got %d normals for %d points" % (nrm_in.shape[0], n))
            if want_normals:
                raise ValueError("fpfh: want_normals returns the normals the call estimates; these were given")
        else:
            npb = normal_params if normal_params is not None else _normal_params()
            _check_normal_params(npb, "fpfh")
        out = np.full((max(n, 1), FPFH_DIM), np.nan, np.float32)
        nrm_out = np.full((max(n, 1), 3), np.nan, np.float32) if want_normals else None
        info = FpfhInfo()
        self._check(self._L.dcreg_fpfh(self._h, a.ctypes.data, n, a.shape[1], nrm_in.ctypes.data if nrm_in is not None else None,
                                       nrm_in.shape[1] if nrm_in is not None else 3, C.byref(npb) if npb is not None else None, C.byref(p),
                                       out.ctypes.data, nrm_out.ctypes.data if want_normals else None, C.byref(info)), "dcreg_fpfh")
        return out[:n], (nrm_out[:n] if want_normals else None), _fpfh_info_dict(info)

    def fpfh_device(self, dev_ptr, n, stride, dev_fpfh_ptr, dev_normals_ptr=0, normals_stride=3, normal_params=None, params=None,
                    dev_normals_out_ptr=0):
        """dcreg_fpfh_device: the cloud, the normals (0: estimated with normal_params) and the outputs (33 n floats; 3 n floats of
        estimated normals, 0: not wanted) in device memory.  -> info dict"""
        p = params if params is not None else fpfh_params()
        _check_fpfh_params(p, "fpfh_device")
        _check_device_cloud(n, stride, "fpfh_device")
        if not dev_fpfh_ptr:
            raise ValueError("fpfh_device: an output buffer is expected")
        npb = None
        if dev_normals_ptr:
            if int(normals_stride) < 3:
                raise ValueError("fpfh_device: a normals stride of at least 3 floats is expected, got %d" % int(normals_stride))
        else:
            npb = normal_params if normal_params is not None else _normal_params()
            _check_normal_params(npb, "fpfh_device")
        info = FpfhInfo()
        self._check(self._L.dcreg_fpfh_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.c_void_p(dev_normals_ptr or None), int(normals_stride),
                                              C.byref(npb) if npb is not None else None, C.byref(p), C.c_void_p(dev_fpfh_ptr),
                                              C.c_void_p(dev_normals_out_ptr or None), C.byref(info)), "dcreg_fpfh_device")
        return _fpfh_info_dict(info)

    def target_fpfh(self, params=None):
        """dcreg_target_fpfh: the descriptors of the resident map's points in index order (target_points()), from the kept normals
        (keep_target_normals / set_target_normals) through the map's own index.  -> (fpfh [n, 33] float32, info dict)"""
        p = params if params is not None else fpfh_params()
        _check_fpfh_params(p, "target_fpfh")
        n = max(int(self.index_info().n_target), 0)
        out = np.full((max(n, 1), FPFH_DIM), np.nan, np.float32)
        info = FpfhInfo()
        self._check(self._L.dcreg_target_fpfh(self._h, C.byref(p), out.ctypes.data, n, C.byref(info)), "dcreg_target_fpfh")
        return out[:n], _fpfh_info_dict(info)

    def fpfh_debug_counts(self, n):
        """dcreg_fpfh_debug_counts: the SPFH records behind the descriptor call just made, for its n input points
        -> (counts [n, 33] uint8, m [n] uint8, has_spfh [n] bool)"""
        raw = np.zeros((max(int(n), 1), 36), np.uint8)
        self._check(self._L.dcreg_fpfh_debug_counts(self._h, raw.ctypes.data, int(n)), "dcreg_fpfh_debug_counts")
        raw = raw[:n]
        return raw[:, :FPFH_DIM].copy(), raw[:, FPFH_DIM].copy(), raw[:, FPFH_DIM + 1] != 0

    # ---- FPFH over a radius support (include/dcreg.h: dcreg_fpfh_radius ..)
    def fpfh_radius(self, cloud, normals=None, normal_params=None, params=None, want_normals=False):
        """dcreg_fpfh_radius: fpfh() with every used point within params.radius as the support (PCL setRadiusSearch; include/dcreg.h has
        the rule).  params: fpfh_radius_params(...), None = the defaults.  -> (fpfh [n, 33] float32, normals [n, 3] float32 or None, dict
        n_in / n_used / n_empty / n_crowded / n_out / m_max / m_sum)"""
        p = params if params is not None else fpfh_radius_params()
        _check_fpfh_radius_params(p, "fpfh_radius")
        a = _points(cloud, "fpfh_radius")
        n = a.shape[0]
        nrm_in = npb = None
        if normals is not None:
            nrm_in = _points(normals, "fpfh_radius")
            if nrm_in.shape[0] != n:
                raise ValueError("fpfh_radius: one normal per point is expected, got %d normals for %d points" % (nrm_in.shape[0], n))
            if want_normals:
                raise ValueError("fpfh_radius: want_normals returns the normals the call estimates; these were given")
        else:
            npb = normal_params if normal_params is not None else _normal_params()
            _check_normal_params(npb, "fpfh_radius")
        out = np.full((max(n, 1), FPFH_DIM), np.nan, np.float32)
        nrm_out = np.full((max(n, 1), 3), np.nan, np.float32) if want_normals else None
        info = FpfhRadiusInfo()
        self._check(self._L.dcreg_fpfh_radius(self._h, a.ctypes.data, n, a.shape[1], nrm_in.ctypes.data if nrm_in is not None else None,
                                              nrm_in.shape[1] if nrm_in is not None else 3, C.byref(npb) if npb is not None else None,
                                              C.byref(p), out.ctypes.data, nrm_out.ctypes.data if want_normals else None, C.byref(info)),
                    "dcreg_fpfh_radius")
        return out[:n], (nrm_out[:n] if want_normals else None), _fpfh_radius_info_dict(info)

    def fpfh_radius_device(self, dev_ptr, n, stride, dev_fpfh_ptr, dev_normals_ptr=0, normals_stride=3, normal_params=None, params=None,
                           dev_normals_out_ptr=0):
        """dcreg_fpfh_radius_device: the arguments of fpfh_device with fpfh_radius_params(...).  -> info dict"""
        p = params if params is not None else fpfh_radius_params()
        _check_fpfh_radius_params(p, "fpfh_radius_device")
        _check_device_cloud(n, stride, "fpfh_radius_device")
        if not dev_fpfh_ptr:
            raise ValueError("fpfh_radius_device: an output buffer is expected")
        npb = None
        if dev_normals_ptr:
            if int(normals_stride) < 3:
                raise ValueError("fpfh_radius_device: a normals stride of at least 3 floats is expected, got %d" % int(normals_stride))
        else:
            npb = normal_params if normal_params is not None else _normal_params()
            _check_normal_params(npb, "fpfh_radius_device")
        info = FpfhRadiusInfo()
        self._check(self._L.dcreg_fpfh_radius_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.c_void_p(dev_normals_ptr or None),
                                                     int(normals_stride), C.byref(npb) if npb is not None else None, C.byref(p),
                                                     C.c_void_p(dev_fpfh_ptr), C.c_void_p(dev_normals_out_ptr or None), C.byref(info)),
                    "dcreg_fpfh_radius_device")
        return _fpfh_radius_info_dict(info)

    def target_fpfh_radius(self, params=None):
        """dcreg_target_fpfh_radius: target_fpfh() under the radius rule.  -> (fpfh [n, 33] float32, info dict)"""
        p = params if params is not None else fpfh_radius_params()
        _check_fpfh_radius_params(p, "target_fpfh_radius")
        n = max(int(self.index_info().n_target), 0)
        out = np.full((max(n, 1), FPFH_DIM), np.nan, np.float32)
        info = FpfhRadiusInfo()
        self._check(self._L.dcreg_target_fpfh_radius(self._h, C.byref(p), out.ctypes.data, n, C.byref(info)), "dcreg_target_fpfh_radius")
        return out[:n], _fpfh_radius_info_dict(info)

    def fpfh_radius_debug_counts(self, n):
        """dcreg_fpfh_radius_debug_counts: the SPFH records behind the radius descriptor call just made, for its n input points
        -> (counts [n, 33] uint32, m [n] uint32, has_spfh [n] bool)"""
        raw = np.zeros((max(int(n), 1), FPFH_DIM + 2), np.uint32)
        self._check(self._L.dcreg_fpfh_radius_debug_counts(self._h, raw.ctypes.data, int(n)), "dcreg_fpfh_radius_debug_counts")
        raw = raw[:n]
        return raw[:, :FPFH_DIM].copy(), raw[:, FPFH_DIM].copy(), raw[:, FPFH_DIM + 1] != 0

    def feature_match(self, a, b, want_second=True, want_mutual=True):
        """dcreg_feature_match: for every row of a ([n_a, c] float32, 33 values first) its nearest and second-nearest row of b in feature
        space, ranked by (squared distance in double, index); rows with a non-finite value are neither queries nor candidates.
        -> dict idx [n_a] int32 (-1: none), d [n_a] float64, idx2 / d2 (want_second), mutual [n_a] uint8 (want_mutual: b's best row of a
        is the query), n_a_valid, n_b_valid, n_mutual"""
        a = _feature_rows(a, "feature_match")
        b = _feature_rows(b, "feature_match")
        na = a.shape[0]
        idx = np.full(max(na, 1), -1, np.int32)
        d = np.full(max(na, 1), np.nan, np.float64)
        idx2 = np.full(max(na, 1), -1, np.int32) if want_second else None
        d2 = np.full(max(na, 1), np.nan, np.float64) if want_second else None
        mutual = np.zeros(max(na, 1), np.uint8) if want_mutual else None
        info = MatchInfo()
        self._check(self._L.dcreg_feature_match(self._h, a.ctypes.data, na, a.shape[1], b.ctypes.data, b.shape[0], b.shape[1], idx.ctypes.data,
                                                d.ctypes.data, idx2.ctypes.data if want_second else None, d2.ctypes.data if want_second else None,
                                                mutual.ctypes.data if want_mutual else None, C.byref(info)), "dcreg_feature_match")
        out = {"idx": idx[:na], "d": d[:na], "n_a_valid": info.n_a_valid, "n_b_valid": info.n_b_valid, "n_mutual": info.n_mutual}
        if want_second:
            out.update(idx2=idx2[:na], d2=d2[:na])
        if want_mutual:
            out["mutual"] = mutual[:na]
        return out

    def feature_match_device(self, dev_a, n_a, stride_a, dev_b, n_b, stride_b, dev_idx, dev_d, dev_idx2=0, dev_d2=0, dev_mutual=0):
        """dcreg_feature_match_device: both descriptor sets and the outputs (n_a int32 / float64 / bytes; 0: not wanted) in device memory
        -> dict n_a_valid / n_b_valid / n_mutual"""
        _check_device_rows(n_a, stride_a, "feature_match_device")
        _check_device_rows(n_b, stride_b, "feature_match_device")
        if not dev_idx or not dev_d:
            raise ValueError("feature_match_device: the index and distance outputs are expected")
        info = MatchInfo()
        self._check(self._L.dcreg_feature_match_device(self._h, C.c_void_p(dev_a or None), int(n_a), int(stride_a), C.c_void_p(dev_b or None), int(n_b),
                                                       int(stride_b), C.c_void_p(dev_idx), C.c_void_p(dev_d), C.c_void_p(dev_idx2 or None),
                                                       C.c_void_p(dev_d2 or None), C.c_void_p(dev_mutual or None), C.byref(info)),
                    "dcreg_feature_match_device")
        return {"n_a_valid": info.n_a_valid, "n_b_valid": info.n_b_valid, "n_mutual": info.n_mutual}

    # ---- a pose from correspondences (include/dcreg.h: dcreg_align_correspondences)
    def align_correspondences(self, a, b, corr_a, corr_b, params=None, want_mask=True):
        """dcreg_align_correspondences: the rigid pose q ~ R p + t that most of the point pairs (a[corr_a[m]], b[corr_b[m]]) agree on,
        by seeded RANSAC over three-pair hypotheses (include/dcreg.h has the rule).  a, b: [n, c] float32 clouds, x y z first; corr_a,
        corr_b: integer arrays of one length - a pair with an index out of range (feature_match's -1) or a non-finite point is skipped.
        params: align_params(...), None = the defaults.  -> dict records (best first, at most n_best dicts: T [4, 4] float64 - a start
        pose as icp_run* and icp_run_trials* take it -, hypothesis, pairs, count, cost, n_inliers, refined, rmse), mask ([m] uint8:
        the inliers of records[0]; None without want_mask) and info (n_pairs, n_used, n_drawn, n_degenerate, n_rejected, n_scored,
        n_returned)"""
        p = params if params is not None else align_params()
        _check_align_params(p, "align_correspondences")
        a = _points(a, "align_correspondences")
        b = _points(b, "align_correspondences")
        ca = _corr_index(corr_a, "align_correspondences")
        cb = _corr_index(corr_b, "align_correspondences")
        if ca.shape[0] != cb.shape[0]:
            raise ValueError("align_correspondences: index arrays of one length are expected, got %d and %d" % (ca.shape[0], cb.shape[0]))
        m = ca.shape[0]
        recs = (AlignRecord * p.n_best)()
        mask = np.zeros(max(m, 1), np.uint8) if want_mask else None
        info = AlignInfo()
        self._check(self._L.dcreg_align_correspondences(self._h, a.ctypes.data, a.shape[0], a.shape[1], b.ctypes.data, b.shape[0], b.shape[1],
                                                        ca.ctypes.data, cb.ctypes.data, m, C.byref(p), recs, mask.ctypes.data if want_mask else None,
                                                        C.byref(info)), "dcreg_align_correspondences")
        return {"records": _align_records(recs, info.n_returned), "mask": mask[:m] if want_mask else None, "info": _align_info_dict(info)}

    def align_correspondences_device(self, dev_a, n_a, stride_a, dev_b, n_b, stride_b, dev_corr_a, dev_corr_b, n_pairs, params=None, dev_mask=0):
        """dcreg_align_correspondences_device: both clouds, both int32 index arrays and the mask (n_pairs bytes; 0: not wanted) in device
        memory.  -> dict records / info, as align_correspondences"""
        p = params if params is not None else align_params()
        _check_align_params(p, "align_correspondences_device")
        _check_device_cloud(n_a, stride_a, "align_correspondences_device")
        _check_device_cloud(n_b, stride_b, "align_correspondences_device")
        if int(n_pairs) < 0 or int(n_pairs) > OUTLIER_MAX_POINTS:
            raise ValueError("align_correspondences_device: 0 .. 2^31 - 1 pairs are expected, got %d" % int(n_pairs))
        if int(n_pairs) > 0 and (not dev_corr_a or not dev_corr_b):
            raise ValueError("align_correspondences_device: both index arrays are expected")
        recs = (AlignRecord * p.n_best)()
        info = AlignInfo()
        self._check(self._L.dcreg_align_correspondences_device(self._h, C.c_void_p(dev_a or None), int(n_a), int(stride_a), C.c_void_p(dev_b or None),
                                                               int(n_b), int(stride_b), C.c_void_p(dev_corr_a or None), C.c_void_p(dev_corr_b or None),
                                                               int(n_pairs), C.byref(p), recs, C.c_void_p(dev_mask or None), C.byref(info)),
                    "dcreg_align_correspondences_device")
        return {"records": _align_records(recs, info.n_returned), "info": _align_info_dict(info)}

    # ---- a consensus pose from the correspondences' compatibility graph (include/dcreg.h: dcreg_consensus_correspondences)
    def consensus_correspondences(self, a, b, corr_a, corr_b, params=None, want_mask=True, want_members=False, want_weights=False):
        """dcreg_consensus_correspondences: the rigid pose q ~ R p + t of the largest length-preserving set among the point pairs
        (a[corr_a[m]], b[corr_b[m]]), for inlier shares of a per cent and below (include/dcreg.h has the rule).  Arguments as
        align_correspondences takes them, at most 32768 pairs; params: consensus_params(...), None = the defaults.  -> dict records (best
        first, at most n_best dicts: T [4, 4] float64, seed, seed_rank, weight, n_members, count, cost, n_inliers, refined, rmse), mask
        ([m] uint8: the inliers of records[0]; None without want_mask), info (n_pairs, n_used, n_edges, max_degree, n_seeds, n_skipped,
        n_scored, n_returned); with want_members: members [n_best, consensus_size] int32 (the correspondence numbers of each record's
        set, -1 padded); with want_weights: degree and weight [m] uint32 (0 at unused pairs) - the pairs with weight > 0 are a far
        cleaner input for align_correspondences"""
        p = params if params is not None else consensus_params()
        _check_consensus_params(p, "consensus_correspondences")
        a = _points(a, "consensus_correspondences")
        b = _points(b, "consensus_correspondences")
        ca = _corr_index(corr_a, "consensus_correspondences")
        cb = _corr_index(corr_b, "consensus_correspondences")
        if ca.shape[0] != cb.shape[0]:
            raise ValueError("consensus_correspondences: index arrays of one length are expected, got %d and %d" % (ca.shape[0], cb.shape[0]))
        m = ca.shape[0]
        if m > CONSENSUS_MAX_PAIRS:
            raise ValueError("consensus_correspondences: at most %d pairs are expected, got %d" % (CONSENSUS_MAX_PAIRS, m))
        recs = (ConsensusRecord * p.n_best)()
        mask = np.zeros(max(m, 1), np.uint8) if want_mask else None
        members = np.full((p.n_best, p.consensus_size), -1, np.int32) if want_members else None
        degree = np.zeros(max(m, 1), np.uint32) if want_weights else None
        weight = np.zeros(max(m, 1), np.uint32) if want_weights else None
        info = ConsensusInfo()
        ptr = lambda x: x.ctypes.data if x is not None else None
        self._check(self._L.dcreg_consensus_correspondences(self._h, a.ctypes.data, a.shape[0], a.shape[1], b.ctypes.data, b.shape[0], b.shape[1],
                                                            ca.ctypes.data, cb.ctypes.data, m, C.byref(p), recs, ptr(mask), ptr(members), ptr(degree),
                                                            ptr(weight), C.byref(info)), "dcreg_consensus_correspondences")
        out = {"records": _consensus_records(recs, info.n_returned), "mask": mask[:m] if want_mask else None, "info": _consensus_info_dict(info)}
        if want_members:
            out["members"] = members
        if want_weights:
            out["degree"], out["weight"] = degree[:m], weight[:m]
        return out

    def consensus_correspondences_device(self, dev_a, n_a, stride_a, dev_b, n_b, stride_b, dev_corr_a, dev_corr_b, n_pairs, params=None, dev_mask=0,
                                         dev_members=0, dev_degree=0, dev_weight=0):
        """dcreg_consensus_correspondences_device: both clouds, both int32 index arrays and the outputs wanted (0: not wanted) - the mask
        (n_pairs bytes), the members (n_best x consensus_size int32), degree and weight (n_pairs uint32 each) - in device memory.
        -> dict records / info, as consensus_correspondences"""
        p = params if params is not None else consensus_params()
        _check_consensus_params(p, "consensus_correspondences_device")
        _check_device_cloud(n_a, stride_a, "consensus_correspondences_device")
        _check_device_cloud(n_b, stride_b, "consensus_correspondences_device")
        if int(n_pairs) < 0 or int(n_pairs) > CONSENSUS_MAX_PAIRS:
            raise ValueError("consensus_correspondences_device: 0 .. %d pairs are expected, got %d" % (CONSENSUS_MAX_PAIRS, int(n_pairs)))
        if int(n_pairs) > 0 and (not dev_corr_a or not dev_corr_b):
            raise ValueError("consensus_correspondences_device: both index arrays are expected")
        recs = (ConsensusRecord * p.n_best)()
        info = ConsensusInfo()
        self._check(self._L.dcreg_consensus_correspondences_device(self._h, C.c_void_p(dev_a or None), int(n_a), int(stride_a), C.c_void_p(dev_b or None),
                                                                   int(n_b), int(stride_b), C.c_void_p(dev_corr_a or None),
                                                                   C.c_void_p(dev_corr_b or None), int(n_pairs), C.byref(p), recs,
                                                                   C.c_void_p(dev_mask or None), C.c_void_p(dev_members or None),
                                                                   C.c_void_p(dev_degree or None), C.c_void_p(dev_weight or None), C.byref(info)),
                    "dcreg_consensus_correspondences_device")
        return {"records": _consensus_records(recs, info.n_returned), "info": _consensus_info_dict(info)}

    # ---- candidate poses scored against the map (include/dcreg.h: dcreg_verify_poses)
    def verify_poses(self, Ts, params=None, cloud=None, want_detail=False):
        """dcreg_verify_poses / dcreg_verify_poses_cloud: P candidate poses of one cloud scored against the resident map in one launch -
        per pose the points with a map point strictly inside the inlier distance and an integer cost of their distances (include/dcreg.h
        has the rule).  Ts: [P, 4, 4] poses, or the record dicts of align_correspondences / consensus_correspondences (their T is
        taken); cloud: None = the resident source, else an [n, c] float32 cloud (x y z first, non-finite rows skipped) - the resident
        source is then neither read nor changed; params: verify_params(...), None = the defaults.  -> dict records (ALL poses, best
        first: pose - the input index -, count, cost, score, fitness, rmse), order (the ranked input indices: Ts[order[0]] is a start
        pose as icp_run* and icp_run_trials* take it), info (n_poses, n_points, n_scored, best_pose); with want_detail (params.detail_pose
        names the pose): mask [n] uint8 and nn [n] int32 in the cloud's original order"""
        p = params if params is not None else verify_params()
        _check_verify_params(p, "verify_poses")
        T16, n_poses = _verify_poses(Ts, p, "verify_poses")
        if want_detail and p.detail_pose < 0:
            raise ValueError("verify_poses: want_detail needs a detail_pose in the parameters, got %d" % p.detail_pose)
        pts = _points(cloud, "verify_poses") if cloud is not None else None
        recs = (VerifyRecord * max(n_poses, 1))()
        info = VerifyInfo()
        n = pts.shape[0] if pts is not None else (int(self.index_info().n_source) if want_detail else 0)
        mask = np.zeros(max(n, 1), np.uint8) if want_detail else None
        nn = np.full(max(n, 1), -1, np.int32) if want_detail else None
        ptr = lambda x: x.ctypes.data if x is not None else None
        tail = (T16.ctypes.data, n_poses, 16, C.byref(p), recs, ptr(mask), ptr(nn), C.byref(info))
        if pts is None:
            self._check(self._L.dcreg_verify_poses(self._h, *tail), "dcreg_verify_poses")
        else:
            self._check(self._L.dcreg_verify_poses_cloud(self._h, pts.ctypes.data, pts.shape[0], pts.shape[1], *tail), "dcreg_verify_poses_cloud")
        out = {"records": _verify_records(recs, info.n_poses), "info": _verify_info_dict(info)}
        out["order"] = [r["pose"] for r in out["records"]]
        if want_detail:
            out["mask"], out["nn"] = mask[:n], nn[:n]
        return out

    def verify_poses_device(self, dev_ptr, n, stride, Ts, params=None, dev_mask=0, dev_nn=0):
        """dcreg_verify_poses_cloud_device: the cloud (n rows of `stride` floats) and the detail outputs wanted (0: not wanted; n bytes
        / n int32, written for params.detail_pose) in device memory.  -> dict records / order / info, as verify_poses"""
        p = params if params is not None else verify_params()
        _check_verify_params(p, "verify_poses_device")
        _check_device_cloud(n, stride, "verify_poses_device")
        if int(n) > 0 and not dev_ptr:
            raise ValueError("verify_poses_device: a cloud pointer is expected")
        T16, n_poses = _verify_poses(Ts, p, "verify_poses_device")
        recs = (VerifyRecord * max(n_poses, 1))()
        info = VerifyInfo()
        self._check(self._L.dcreg_verify_poses_cloud_device(self._h, C.c_void_p(dev_ptr or None), int(n), int(stride), T16.ctypes.data, n_poses, 16,
                                                            C.byref(p), recs, C.c_void_p(dev_mask or None), C.c_void_p(dev_nn or None), C.byref(info)),
                    "dcreg_verify_poses_cloud_device")
        out = {"records": _verify_records(recs, info.n_poses), "info": _verify_info_dict(info)}
        out["order"] = [r["pose"] for r in out["records"]]
        return out

    # ---- kept normals and the second engine (include/dcreg.h: dcreg_target_normals_keep .. dcreg_icp_run_normals)
    def keep_target_normals(self, params=None):
        """dcreg_target_normals_keep: the map's normals, as target_normals(params) returns them, stay on the device for linearize_normals and
        icp_run_normals.  -> info dict"""
        p = params if params is not None else normal_params()
        _check_normal_params(p, "keep_target_normals")
        info = NormalInfo()
        self._check(self._L.dcreg_target_normals_keep(self._h, C.byref(p), C.byref(info)), "dcreg_target_normals_keep")
        return _normal_info_dict(info)

    def _set_kept_normals(self, which, normals, dev_ptr, n, stride):
        """set_target_normals / set_source_normals (which = "target" / "source")"""
        what, symbol = "set_%s_normals" % which, "dcreg_%s_normals_set" % which
        if (normals is None) == (not dev_ptr):
            raise ValueError("%s: either normals or dev_ptr is expected" % what)
        if normals is not None:
            a = _points(normals, what)
            self._check(getattr(self._L, symbol)(self._h, a.ctypes.data, a.shape[0], a.shape[1]), symbol)
            return
        if n is None or stride is None:
            raise ValueError("%s: n and stride are expected with dev_ptr" % what)
        _check_device_cloud(n, stride, what)
        self._check(getattr(self._L, symbol + "_device")(self._h, C.c_void_p(dev_ptr), int(n), int(stride)), symbol + "_device")

    def _kept_normals(self, which, dev_ptr, capacity):
        """kept_target_normals / kept_source_normals (which = "target" / "source")"""
        what, symbol = "kept_%s_normals" % which, "dcreg_%s_normals_get" % which
        if dev_ptr:
            if capacity is None or isinstance(capacity, bool) or int(capacity) != capacity or not 0 <= int(capacity) <= OUTLIER_MAX_POINTS:
                raise ValueError("%s: with dev_ptr a capacity of 0 .. 2^31 - 1 points is expected, got %r" % (what, capacity))
            self._check(getattr(self._L, symbol + "_device")(self._h, C.c_void_p(dev_ptr), int(capacity)), symbol + "_device")
            return None
        if capacity is not None:
            raise ValueError("%s: a capacity is expected with dev_ptr only" % what)
        n = max(int(getattr(self.index_info(), "n_" + which)), 0)
        out = np.full((max(n, 1), 4), np.nan, np.float32)
        self._check(getattr(self._L, symbol)(self._h, out.ctypes.data, n), symbol)
        return np.ascontiguousarray(out[:n, :3]), np.ascontiguousarray(out[:n, 3])

    def set_target_normals(self, normals=None, dev_ptr=0, n=None, stride=None):
        """dcreg_target_normals_set[_device]: the caller's normals, one per map point in index order (target_points()), kept as given.
        normals: [n, c >= 3] float32 on the host, or dev_ptr / n / stride for device memory.  A normal with a non-finite component
        means that the point has none."""
        self._set_kept_normals("target", normals, dev_ptr, n, stride)

    def target_normals_kept(self):
        return int(self._L.dcreg_target_normals_kept(self._h))

    def drop_target_normals(self):
        self._check(self._L.dcreg_target_normals_drop(self._h), "dcreg_target_normals_drop")

    def kept_target_normals(self, dev_ptr=0, capacity=None):
        """dcreg_target_normals_get[_device]: the kept normals as they stand, in index order (target_points()) - what a caller persists with
        a map, and what set_option("normals_follow", 1) keeps up to date through inserts and removals.
        -> (normals [n, 3] float32, curvature [n] float32); with dev_ptr: 4 floats per point (nx ny nz curvature) go to that device buffer
        of `capacity` points instead, -> None"""
        return self._kept_normals("target", dev_ptr, capacity)

    def normals_follow_info(self):
        """dcreg_target_normals_follow_info: what the last update that changed the map did to the kept normals -> dict n_target / n_refit /
        n_carried / followed (0 dropped or no update yet, 1 refitted incrementally, 2 recomputed in full)"""
        info = NormalsFollowInfo()
        self._check(self._L.dcreg_target_normals_follow_info(self._h, C.byref(info)), "dcreg_target_normals_follow_info")
        return {"n_target": int(info.n_target), "n_refit": int(info.n_refit), "n_carried": int(info.n_carried), "followed": int(info.followed)}

    @staticmethod
    def _nlin_params(params, what):
        params = params if params is not None else default_lin_params()
        if not isinstance(params, LinParams):
            raise ValueError("%s: a default_lin_params(...) block is expected" % what)
        if params.parameterization != 0:
            raise ValueError("%s: parameterization must be SO3 (0), got %d" % (what, params.parameterization))
        if not (np.isfinite(params.search_radius) and params.search_radius > 0.0):
            raise ValueError("%s: search_radius must be finite and > 0, got %r" % (what, params.search_radius))
        return params

    def _linearize_kept(self, symbol, what, T, params, debug, entries, struct):
        """linearize_normals / linearize_gicp: the plain call, or the debug form with every array of its dump"""
        params = self._nlin_params(params, what)
        R, t = _pose_arg(T, what)
        out = LinOut()
        if not debug:
            self._check(getattr(self._L, symbol)(self._h, _dp(R), _dp(t), C.byref(params), C.byref(out)), symbol)
            return self._out_dict(out)
        keep, dbg = _dump_arg(self.index_info().n_source, entries, struct)
        self._check(getattr(self._L, symbol + "_debug")(self._h, _dp(R), _dp(t), C.byref(params), C.byref(out), C.byref(dbg)), symbol + "_debug")
        d = self._out_dict(out)
        d.update(keep)
        return d

    def _run_logged(self, symbol, T0, method, cfg, log_capacity, what=None, extra=()):
        """the single runs: `symbol` from the pose T0 -> (result, the log records the run wrote); what: the wrapper checks pose and method
        itself (_pose_arg, _method); extra: the call's arguments between cfg and the log"""
        R0, t0 = _pose_arg(T0, what)
        det, hand = _method(method, what)
        cap = cfg.max_iterations if log_capacity is None else log_capacity
        logs = (IterLog * max(cap, 1))()
        res = IcpResult()
        self._check(getattr(self._L, symbol)(self._h, _dp(R0), _dp(t0), det, hand, C.byref(cfg), *extra, logs, cap, C.byref(res)), symbol)
        n = min(res.iterations, cap)
        if res.status == 1:
            n = min(res.iterations - 1, cap)
        return res, [logs[i] for i in range(max(n, 0))]

    def linearize_normals(self, T, params=None, debug=False):
        """dcreg_linearize_normals at the pose T (4 x 4): the 1-NN point-to-plane rows against the kept normals (include/dcreg.h has the
        rule) -> dict as linearize(); debug=True adds the per-point dump in source order: nn_idx, nn_d2, flag, normal [n, 3], r, s,
        row [n, 8]."""
        return self._linearize_kept("dcreg_linearize_normals", "linearize_normals", T, params, debug, _NLIN_DUMP, NlinDebug)

    def icp_run_normals(self, T0, method, cfg, log_capacity=None):
        """dcreg_icp_run_normals: icp_run's loop against the kept normals -> (result, logs)"""
        return self._run_logged("dcreg_icp_run_normals", T0, method, cfg, log_capacity, "icp_run_normals")

    # ---- kept source normals and the third engine (include/dcreg.h: dcreg_source_normals_keep .. dcreg_icp_run_gicp)
    def keep_source_normals(self, params=None):
        """dcreg_source_normals_keep: the source's own normals, as normals(source, params) returns them, stay on the device beside its
        points for linearize_gicp and icp_run_gicp.  -> info dict"""
        p = params if params is not None else normal_params()
        _check_normal_params(p, "keep_source_normals")
        info = NormalInfo()
        self._check(self._L.dcreg_source_normals_keep(self._h, C.byref(p), C.byref(info)), "dcreg_source_normals_keep")
        return _normal_info_dict(info)

    def set_source_normals(self, normals=None, dev_ptr=0, n=None, stride=None):
        """dcreg_source_normals_set[_device]: the caller's normals, one per source point in the order the source was given, kept as given.
        normals: [n, c >= 3] float32 on the host, or dev_ptr / n / stride for device memory.  A normal with a non-finite component
        means that the point has none."""
        self._set_kept_normals("source", normals, dev_ptr, n, stride)

    def source_normals_kept(self):
        return int(self._L.dcreg_source_normals_kept(self._h))

    def drop_source_normals(self):
        self._check(self._L.dcreg_source_normals_drop(self._h), "dcreg_source_normals_drop")

    def kept_source_normals(self, dev_ptr=0, capacity=None):
        """dcreg_source_normals_get[_device]: the kept source normals in the order the source was given
        -> (normals [n, 3] float32, curvature [n] float32); with dev_ptr: 4 floats per point (nx ny nz curvature) go to that device buffer
        of `capacity` points instead, -> None"""
        return self._kept_normals("source", dev_ptr, capacity)

    def linearize_gicp(self, T, params=None, debug=False):
        """dcreg_linearize_gicp at the pose T (4 x 4): three whitened point-to-plane rows per correspondence from the kept map normals and
        the kept source normals (include/dcreg.h has the rule; of params only search_radius is read) -> dict as linearize(); debug=True
        adds the per-point dump in source order: nn_idx, nn_d2, flag, normal_map [n, 3], normal_src [n, 3], w [n, 3, 3], r [n, 3],
        row [n, 3, 8]."""
        return self._linearize_kept("dcreg_linearize_gicp", "linearize_gicp", T, params, debug, _GLIN_DUMP, GlinDebug)

    def icp_run_gicp(self, T0, method, cfg, log_capacity=None):
        """dcreg_icp_run_gicp: icp_run_normals's loop around linearize_gicp -> (result, logs); a log's rmse is the RMS Mahalanobis distance
        per effective point"""
        return self._run_logged("dcreg_icp_run_gicp", T0, method, cfg, log_capacity, "icp_run_gicp")

    # ---- the kept voxel map and the fourth engine (include/dcreg.h: dcreg_target_voxels_keep .. dcreg_icp_run_voxels)
    def keep_target_voxels(self, params=None):
        """dcreg_target_voxels_keep: one Gaussian per voxel of the map (voxel_map_params(leaf, epsilon, min_points)) stays on the device
        for linearize_voxels and icp_run_voxels.  -> info dict n_points / n_voxels / n_small / n_degenerate / n_kept"""
        p = params if params is not None else voxel_map_params()
        _check_voxel_map_params(p, "keep_target_voxels")
        info = VoxelMapInfo()
        self._check(self._L.dcreg_target_voxels_keep(self._h, C.byref(p), C.byref(info)), "dcreg_target_voxels_keep")
        return {k: int(getattr(info, k)) for k, _ in VoxelMapInfo._fields_}

    def target_voxels_kept(self):
        """dcreg_target_voxels_kept: the number of kept voxels, 0 without a member"""
        return int(self._L.dcreg_target_voxels_kept(self._h))

    def voxels_follow_info(self):
        """dcreg_target_voxels_follow_info: what the last update that changed the map did to the kept voxel map (set_option("voxels_follow",
        1) makes inserts and removals refit it instead of dropping it) -> dict n_target / n_touched / n_refit / n_carried / n_kept /
        followed (0 not followed, 1 incremental, 2 the full keep)"""
        info = VoxelsFollowInfo()
        self._check(self._L.dcreg_target_voxels_follow_info(self._h, C.byref(info)), "dcreg_target_voxels_follow_info")
        return {k: int(getattr(info, k)) for k, _ in VoxelsFollowInfo._fields_ if k != "reserved_"}

    def drop_target_voxels(self):
        self._check(self._L.dcreg_target_voxels_drop(self._h), "dcreg_target_voxels_drop")

    def kept_target_voxels(self):
        """dcreg_target_voxels_get: the kept voxels in ascending (z, y, x) order -> dict coords [V, 3] int64 (absolute voxel coordinates),
        count [V] int32, mean [V, 3] float32, cov [V, 6] float32 (xx xy xz yy yz zz)"""
        n = self.target_voxels_kept()
        m = max(n, 1)
        coords, count = np.zeros((m, 3), np.int64), np.zeros(m, np.int32)
        mean, cov = np.zeros((m, 3), np.float32), np.zeros((m, 6), np.float32)
        self._check(self._L.dcreg_target_voxels_get(self._h, coords.ctypes.data, count.ctypes.data, mean.ctypes.data, cov.ctypes.data, n),
                    "dcreg_target_voxels_get")
        return {"coords": coords[:n], "count": count[:n], "mean": mean[:n], "cov": cov[:n]}

    @staticmethod
    def _vlin_params(params, what):
        params = params if params is not None else default_lin_params()
        if not isinstance(params, LinParams):
            raise ValueError("%s: a default_lin_params(...) block is expected" % what)
        if params.parameterization != 0:
            raise ValueError("%s: parameterization must be SO3 (0), got %d" % (what, params.parameterization))
        return params

    def linearize_voxels(self, T, params=None, debug=False):
        """dcreg_linearize_voxels at the pose T (4 x 4): three whitened rows per source point that falls into a kept voxel (include/dcreg.h
        has the rule; of params only the parameterization is read; set_option("voxels_source_cov", 1) adds the source's plane covariance;
        set_option("voxels_neighbors", S), S = 7 or 27, matches a point to the kept voxels of the stencil around its own, three rows each)
        -> dict as linearize(); debug=True adds the per-point dump in source order: voxel_idx, flag, mean [n, 3], cov [n, 6],
        normal_src [n, 3], w [n, 3, 3], r [n, 3], row [n, 3, 8].  With S > 1 every array but normal_src has an axis of length S - the
        correspondences in stencil order - behind the point axis: voxel_idx [n, S], ..., row [n, S, 3, 8].  S is the value this wrapper's
        set_option set last."""
        what, symbol = "linearize_voxels", "dcreg_linearize_voxels"
        params = self._vlin_params(params, what)
        R, t = _pose_arg(T, what)
        out = LinOut()
        if not debug:
            self._check(self._L.dcreg_linearize_voxels(self._h, _dp(R), _dp(t), C.byref(params), C.byref(out)), symbol)
            return self._out_dict(out)
        S = self._voxels_neighbors
        entries = [(k, dt, shape if S == 1 or k == "normal_src" else (S,) + shape) for k, dt, shape in _VLIN_DUMP]
        keep, dbg = _dump_arg(self.index_info().n_source, entries, VlinDebug)
        self._check(self._L.dcreg_linearize_voxels_debug(self._h, _dp(R), _dp(t), C.byref(params), C.byref(out), C.byref(dbg)), symbol + "_debug")
        d = self._out_dict(out)
        d.update(keep)
        return d

    def linearize_voxels_debug(self, T, params=None):
        """linearize_voxels(T, params, debug=True)"""
        return self.linearize_voxels(T, params, debug=True)

    def icp_run_voxels(self, T0, method, cfg, log_capacity=None):
        """dcreg_icp_run_voxels: icp_run_gicp's loop around linearize_voxels -> (result, logs); a log's rmse is the RMS Mahalanobis
        distance per effective point.  "voxels_neighbors" is read when the call starts, like "voxels_source_cov"."""
        return self._run_logged("dcreg_icp_run_voxels", T0, method, cfg, log_capacity, "icp_run_voxels")

    # ---- the fourth engine's many-frames form (include/dcreg.h: dcreg_register_frames_voxels, dcreg_icp_run_trials_voxels) and its device
    # seam (include/dcreg_debug.h: dcreg_voxels_batch_begin / _end)
    def register_frames_voxels(self, frames, T0s, method, cfg, frame_normals=None, slots=0):
        """dcreg_register_frames_voxels: register_frames with the fourth engine (keep_target_voxels first).  frame_normals =
        normal_params(...) is the rule every frame's own normals are estimated with when set_option("voxels_source_cov", 1) is on - it is
        required then - and is not read otherwise (None: a null pointer is passed).  Same arguments and records; each record is bitwise
        set_source(frame) [+ keep_source_normals(frame_normals)] + icp_run_voxels(T0), at the "voxels_neighbors" in force when the call starts."""
        if frame_normals is not None:
            _check_normal_params(frame_normals, "register_frames_voxels")
        return self._register_frames("dcreg_register_frames_voxels", frames, T0s, method, cfg, slots, "register_frames_voxels",
                                     extra_args=(None if frame_normals is None else C.byref(frame_normals),))

    def icp_run_trials_voxels(self, T0s, method, cfg):
        """dcreg_icp_run_trials_voxels: icp_run_trials with the fourth engine (kept voxels first, in mode 1 kept source normals too); each
        record is bitwise icp_run_voxels from its pose, at the "voxels_neighbors" in force when the call starts"""
        return self._run_trials("dcreg_icp_run_trials_voxels", T0s, method, cfg, "icp_run_trials_voxels")

    def voxels_batch_begin(self, Ts, frame_ids=None, params=None, slot=0):
        """dcreg_voxels_batch_begin: one launch over the poses Ts ([n, 4, 4]); pose i linearises frame frame_ids[i] of the loaded frames
        (None: the own source) against the kept voxels.  Nothing is kept between launches: there are no state_ids.  "voxels_neighbors" is
        read here, with the other options.  -> the number of poses, for voxels_batch_end"""
        params = self._vlin_params(params, "voxels_batch_begin")
        Rs, ts, n = _poses_arg(Ts)
        fids = None if frame_ids is None else np.ascontiguousarray(frame_ids, dtype=np.int32).reshape(n)
        self._check(self._L.dcreg_voxels_batch_begin(self._h, int(slot), n, _dp(Rs), _dp(ts),
                                                     None if fids is None else fids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(params)),
                    "dcreg_voxels_batch_begin")
        return n

    def voxels_batch_end(self, n_poses, slot=0):
        """dcreg_voxels_batch_end -> one dict per pose, as linearize_voxels returns"""
        return self._batch_end("dcreg_voxels_batch_end", n_poses, slot)

    def voxels_batch(self, Ts, frame_ids=None, params=None, slot=0):
        return self.voxels_batch_end(self.voxels_batch_begin(Ts, frame_ids, params, slot), slot)

    # ---- the keyframe store (include/dcreg.h: dcreg_keyframes_*): clouds kept on the device by index, submaps assembled from (id, pose) members
    def keyframes_reset(self):
        """dcreg_keyframes_reset: creates the store, or empties it"""
        self._check(self._L.dcreg_keyframes_reset(self._h), "dcreg_keyframes_reset")

    def keyframes_count(self):
        return int(self._L.dcreg_keyframes_count(self._h))

    def keyframes_sizes(self, first=0, n=None):
        """dcreg_keyframes_sizes: the points of the keyframes [first, first + n) (n = None: to the end) -> [n] int64"""
        first = _keyframe_id(first, "keyframes_sizes: first")
        if n is None:
            n = max(self.keyframes_count() - first, 0)
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or int(n) < 0:
            raise ValueError("keyframes_sizes: n: an integer >= 0 is expected, got %r" % (n,))
        out = np.zeros(max(int(n), 1), np.int64)
        self._check(self._L.dcreg_keyframes_sizes(self._h, first, int(n), out.ctypes.data_as(C.POINTER(C.c_int64))), "dcreg_keyframes_sizes")
        return out[:int(n)]

    def keyframes_add(self, clouds):
        """dcreg_keyframes_add_clouds: clouds = a list of [n_i, c] float32 arrays, or (xyz [N, c], offsets [n + 1]); every cloud becomes one
        keyframe, stored bit for bit in input order (non-finite coordinates are refused).  -> the first new id (the others follow)"""
        xyz, off, _ = _clouds(clouds, "keyframes_add")
        first = C.c_int64(-1)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.dcreg_keyframes_add_clouds(self._h, len(off) - 1, xyz.ctypes.data, off.ctypes.data_as(i64p), xyz.shape[1], C.byref(first)),
                    "dcreg_keyframes_add_clouds")
        return first.value

    def keyframes_add_device(self, dev_ptr, offsets, stride):
        """dcreg_keyframes_add_clouds_device: the clouds in device memory (stride floats per point, offsets on the host) -> the first new id"""
        off = _offsets(offsets, "keyframes_add_device")
        if int(stride) < 3:
            raise ValueError("keyframes_add_device: a stride of at least 3 floats is expected, got %d" % int(stride))
        first = C.c_int64(-1)
        self._check(self._L.dcreg_keyframes_add_clouds_device(self._h, len(off) - 1, C.c_void_p(dev_ptr), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                              int(stride), C.byref(first)), "dcreg_keyframes_add_clouds_device")
        return first.value

    def keyframes_add_source(self):
        """dcreg_keyframes_add_source: the current source, in its input order, becomes a keyframe (no second upload) -> its id"""
        i = C.c_int64(-1)
        self._check(self._L.dcreg_keyframes_add_source(self._h, C.byref(i)), "dcreg_keyframes_add_source")
        return i.value

    def keyframes_get(self, i):
        """dcreg_keyframes_get: the stored points of keyframe i -> [n, 3] float32"""
        i = _keyframe_id(i, "keyframes_get")
        n = int(self.keyframes_sizes(i, 1)[0])
        out = np.empty((max(n, 1), 3), np.float32)
        self._check(self._L.dcreg_keyframes_get(self._h, i, out.ctypes.data, n), "dcreg_keyframes_get")
        return out[:n]

    def _member_points(self, off, ids, what):
        """points per submap of checked member lists (the ids against the store's count)"""
        sizes = self.keyframes_sizes()
        if len(ids) and int(ids.max()) >= len(sizes):
            raise ValueError("%s: keyframe id %d is not inside the store's [0, %d)" % (what, int(ids.max()), len(sizes)))
        per = np.concatenate([[0], np.cumsum(sizes[ids])]).astype(np.int64)
        if int(per[-1]) >= KEYFRAME_MAX_POINTS:
            raise ValueError("%s: fewer than 2^31 - 1 member points are expected in one call, got %d" % (what, int(per[-1])))
        return per[off]

    def keyframe_submaps(self, members, leaf=None, mode="centroid", min_points=1):
        """dcreg_keyframes_submaps: members = a list (one per submap) of lists of (keyframe id, T 4x4); every member's stored points moved by
        its pose on the device, a submap = its members one after the other; leaf given (an edge, three, or voxel_params(...)): each submap
        through the voxel pass (include/dcreg.h has the rules).  -> (a list of [m, 3] float32 arrays, dict n_in / n_finite / n_voxels / n_out)"""
        v = _voxel_block(leaf, mode, min_points, "keyframe_submaps")
        off, ids, poses = _members(members, "keyframe_submaps")
        cap = int(self._member_points(off, ids, "keyframe_submaps")[-1])
        n = len(off) - 1
        out = np.empty((max(cap, 1), 3), np.float32)
        out_off = np.zeros(n + 1, np.int64)
        info = VoxelInfo()
        i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        self._check(self._L.dcreg_keyframes_submaps(self._h, n, off.ctypes.data_as(i64p), ids.ctypes.data_as(i64p), poses.ctypes.data_as(dp),
                                                    C.byref(v) if v is not None else None, out.ctypes.data, cap, out_off.ctypes.data_as(i64p),
                                                    C.byref(info)), "dcreg_keyframes_submaps")
        return [out[out_off[k]:out_off[k + 1]] for k in range(n)], _voxel_info_dict(info)

    def keyframe_submaps_device(self, members, dev_out_ptr, capacity, leaf=None, mode="centroid", min_points=1):
        """dcreg_keyframes_submaps_device: the output to the device buffer dev_out_ptr (3 floats per point, capacity points), written on the
        context's stream.  A capacity the output does not fit raises CapacityError with nothing written; its out_offsets / info carry the
        sizes needed (the member points in all, from keyframes_sizes, are always enough).  -> (out_offsets [n + 1], info dict)"""
        v = _voxel_block(leaf, mode, min_points, "keyframe_submaps_device")
        off, ids, poses = _members(members, "keyframe_submaps_device")
        if isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)) or int(capacity) < 0:
            raise ValueError("keyframe_submaps_device: a capacity >= 0 is expected, got %r" % (capacity,))
        n = len(off) - 1
        out_off = np.zeros(n + 1, np.int64)
        info = VoxelInfo()
        i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        rc = self._L.dcreg_keyframes_submaps_device(self._h, n, off.ctypes.data_as(i64p), ids.ctypes.data_as(i64p), poses.ctypes.data_as(dp),
                                                    C.byref(v) if v is not None else None, C.c_void_p(dev_out_ptr or None), int(capacity),
                                                    out_off.ctypes.data_as(i64p), C.byref(info))
        if rc != OK and int(out_off[-1]) > int(capacity):
            raise CapacityError("dcreg_keyframes_submaps_device: the output holds %d points, the capacity is %d" % (int(out_off[-1]), int(capacity)),
                                out_off, _voxel_info_dict(info))
        self._check(rc, "dcreg_keyframes_submaps_device")
        return out_off, _voxel_info_dict(info)

    def set_target_keyframes(self, members, search_radius, leaf=None, mode="centroid", min_points=1):
        """dcreg_set_target_keyframes: members = a list of (keyframe id, T 4x4); the map becomes bitwise set_target (leaf given:
        set_target_voxel) of keyframe_submaps([members], ...) - after a pose-graph update, or as a local map of the nearest keyframes; the
        points never leave the device.  -> dict n_in / n_finite / n_voxels / n_out"""
        v = _voxel_block(leaf, mode, min_points, "set_target_keyframes")
        off, ids, poses = _members([members], "set_target_keyframes")
        if len(ids) == 0:
            raise ValueError("set_target_keyframes: members: at least one (id, T 4x4) is expected")
        if not np.isfinite(float(search_radius)):
            raise ValueError("set_target_keyframes: a finite search_radius is expected, got %r" % (search_radius,))
        info = VoxelInfo()
        i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        self._check(self._L.dcreg_set_target_keyframes(self._h, len(ids), ids.ctypes.data_as(i64p), poses.ctypes.data_as(dp),
                                                       C.byref(v) if v is not None else None, float(search_radius), C.byref(info)),
                    "dcreg_set_target_keyframes")
        return _voxel_info_dict(info)

    # ---- moving objects (include/dcreg.h: visibility votes from keyframes): range images of stored keyframes, votes of (id, pose) members
    def _ids_in_store(self, ids, what):
        count = self.keyframes_count()
        if len(ids) and int(ids.max()) >= count:
            raise ValueError("%s: keyframe id %d is not inside the store's [0, %d)" % (what, int(ids.max()), count))

    def keyframe_range_images(self, ids, params=None):
        """dcreg_keyframes_range_images: the range images of the stored keyframes ids under params (visibility_params(...); None = the
        defaults) -> [n, rows, cols] float32, +inf where a pixel holds no point"""
        p = params if params is not None else visibility_params()
        _check_visibility_params(p, "keyframe_range_images")
        ids = _keyframe_ids(ids, "keyframe_range_images")
        self._ids_in_store(ids, "keyframe_range_images")
        out = np.empty((len(ids), p.rows, p.cols), np.float32)
        self._check(self._L.dcreg_keyframes_range_images(self._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p),
                                                         out.ctypes.data if len(ids) else None), "dcreg_keyframes_range_images")
        return out

    def keyframe_range_images_device(self, ids, dev_out_ptr, params=None):
        """dcreg_keyframes_range_images_device: the images to the device buffer dev_out_ptr (len(ids) x rows x cols floats)"""
        p = params if params is not None else visibility_params()
        _check_visibility_params(p, "keyframe_range_images_device")
        ids = _keyframe_ids(ids, "keyframe_range_images_device")
        self._ids_in_store(ids, "keyframe_range_images_device")
        self._check(self._L.dcreg_keyframes_range_images_device(self._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p),
                                                                C.c_void_p(dev_out_ptr or None)), "dcreg_keyframes_range_images_device")

    def visibility_filter(self, xyz, members, params=None, want_mask=True, want_counts=True):
        """dcreg_visibility_filter: the points of one cloud in the map frame ([n, c] float32, x y z first; non-finite points are dropped)
        that the members - a list of (keyframe id, T 4x4 sensor -> map), or an (ids [M], T [M, 4, 4]) pair - do not look through
        (include/dcreg.h has the rule), in input order.  -> (kept [m, 3] float32, keep mask [n] bool or None, through [n] int32 or None,
        observed [n] int32 or None, dict n_in / n_finite / n_observed / n_flagged / n_out / n_members)"""
        p = params if params is not None else visibility_params()
        _check_visibility_params(p, "visibility_filter")
        a = _points(xyz, "visibility_filter")
        ids, poses = _vote_members(members, "visibility_filter")
        self._ids_in_store(ids, "visibility_filter")
        n = a.shape[0]
        out = np.empty((max(n, 1), 3), np.float32)
        mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
        through = np.zeros(max(n, 1), np.int32) if want_counts else None
        observed = np.zeros(max(n, 1), np.int32) if want_counts else None
        n_out = C.c_int64(0)
        info = VisibilityInfo()
        self._check(self._L.dcreg_visibility_filter(self._h, a.ctypes.data, n, a.shape[1], len(ids), ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    _dp(poses), C.byref(p), out.ctypes.data, n, C.byref(n_out),
                                                    mask.ctypes.data if want_mask else None, through.ctypes.data if want_counts else None,
                                                    observed.ctypes.data if want_counts else None, C.byref(info)), "dcreg_visibility_filter")
        return (out[:n_out.value], mask[:n].astype(bool) if want_mask else None, through[:n] if want_counts else None,
                observed[:n] if want_counts else None, _visibility_info_dict(info))

    def visibility_filter_device(self, dev_ptr, n, stride, members, dev_out_ptr, capacity, params=None, dev_mask_ptr=0, dev_through_ptr=0,
                                 dev_observed_ptr=0):
        """dcreg_visibility_filter_device: the cloud in device memory, the kept points to dev_out_ptr (3 floats per point, capacity points),
        optionally the uint8 mask and the int32 counts to device buffers of n entries.  A capacity the output does not fit raises
        CapacityError with nothing written; its info carries the size needed.  -> (n_out, info dict)"""
        p = params if params is not None else visibility_params()
        _check_visibility_params(p, "visibility_filter_device")
        _check_device_cloud(n, stride, "visibility_filter_device")
        if isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)) or int(capacity) < 0:
            raise ValueError("visibility_filter_device: a capacity >= 0 is expected, got %r" % (capacity,))
        ids, poses = _vote_members(members, "visibility_filter_device")
        self._ids_in_store(ids, "visibility_filter_device")
        n_out = C.c_int64(-1)
        info = VisibilityInfo()
        rc = self._L.dcreg_visibility_filter_device(self._h, C.c_void_p(dev_ptr or None), int(n), int(stride), len(ids),
                                                    ids.ctypes.data_as(C.POINTER(C.c_int64)), _dp(poses), C.byref(p), C.c_void_p(dev_out_ptr or None),
                                                    int(capacity), C.byref(n_out), C.c_void_p(dev_mask_ptr or None),
                                                    C.c_void_p(dev_through_ptr or None), C.c_void_p(dev_observed_ptr or None), C.byref(info))
        if rc != OK and n_out.value > int(capacity):
            raise CapacityError("dcreg_visibility_filter_device: the output holds %d points, the capacity is %d" % (n_out.value, int(capacity)),
                                None, _visibility_info_dict(info))
        self._check(rc, "dcreg_visibility_filter_device")
        return n_out.value, _visibility_info_dict(info)

    def remove_dynamic(self, members, params=None):
        """dcreg_target_remove_dynamic: the points of the resident map that the members look through are removed in place (later calls are
        bitwise set_target of the survivors) - after a pose-graph update and set_target_keyframes, or every few keyframes on a local map.
        -> dict n_in / n_finite / n_observed / n_flagged / n_out / n_members"""
        p = params if params is not None else visibility_params()
        _check_visibility_params(p, "remove_dynamic")
        ids, poses = _vote_members(members, "remove_dynamic")
        self._ids_in_store(ids, "remove_dynamic")
        info = VisibilityInfo()
        self._check(self._L.dcreg_target_remove_dynamic(self._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int64)), _dp(poses), C.byref(p),
                                                        C.byref(info)), "dcreg_target_remove_dynamic")
        return _visibility_info_dict(info)

    def index_info(self):
        info = IndexInfo()
        self._L.dcreg_index_info_get(self._h, C.byref(info))
        return info

    @staticmethod
    def _out_dict(o):
        d = {"H_upper": np.array(o.H_upper[:]), "g": np.array(o.g[:]), "sum_r2": o.sum_r2, "sum_b2": o.sum_b2,
             "n_eff": o.n_eff, "n_pt": o.n_pt}
        d["H"] = unpack_hessian(d["H_upper"])
        return d

    def linearize(self, R, t, params=None, debug=False):
        params = params or default_lin_params()
        R, t = _f64(R, 9), _f64(t, 3)
        out = LinOut()
        if not debug:
            self._check(self._L.dcreg_linearize(self._h, _dp(R), _dp(t), C.byref(params), C.byref(out)), "dcreg_linearize")
            return self._out_dict(out)
        n = self.index_info().n_source
        keep = {"nn_idx": np.full((n, 5), -1, np.int32), "nn_d2": np.full((n, 5), np.inf, np.float32),
                "flag": np.zeros(n, np.uint8), "normal": np.zeros((n, 3)), "r": np.zeros(n), "s": np.zeros(n),
                "stats": np.zeros(n, np.uint32)}
        dbg = LinDebug(keep["nn_idx"].ctypes.data_as(C.POINTER(C.c_int32)), keep["nn_d2"].ctypes.data_as(C.POINTER(C.c_float)),
                       keep["flag"].ctypes.data_as(C.POINTER(C.c_uint8)), _dp(keep["normal"]), _dp(keep["r"]), _dp(keep["s"]),
                       keep["stats"].ctypes.data_as(C.POINTER(C.c_uint32)))
        self._check(self._L.dcreg_linearize_debug(self._h, _dp(R), _dp(t), C.byref(params), C.byref(out), C.byref(dbg)), "dcreg_linearize_debug")
        d = self._out_dict(out)
        d.update(keep)
        return d

    def linearize_stamped(self, R, t, params=None):
        """timing probe (dcreg_debug.h dcreg_lin_debug::stamps): a plain linearisation (certificates in use) whose waves record shader-clock
        stamps at their phase boundaries -> (sums dict, stamps [n_waves, 8] uint64: t_start, t_loaded, t_searched, t_fitted, t_row, t_reduced,
        lanes searched, lanes refitted; waves that skipped a phase leave its stamp 0)"""
        params = params or default_lin_params()
        R, t = _f64(R, 9), _f64(t, 3)
        out = LinOut()
        n = self.index_info().n_source
        nw = 4 * ((n + 255) // 256)
        st = np.zeros((nw, 8), np.uint64)
        dbg = LinDebug()
        dbg.stamps = st.ctypes.data_as(C.POINTER(C.c_uint64))
        self._check(self._L.dcreg_linearize_debug(self._h, _dp(R), _dp(t), C.byref(params), C.byref(out), C.byref(dbg)), "dcreg_linearize_debug")
        return self._out_dict(out), st

    def linearize_raw(self, R, t, params, out):
        """Hot-loop variant: caller-owned float64 arrays / structs, no allocation."""
        return self._L.dcreg_linearize(self._h, _dp(R), _dp(t), C.byref(params), C.byref(out))

    def linearize_batch(self, Rs, ts, params=None):
        params = params or default_lin_params()
        Rs = _f64(Rs).reshape(-1, 9)
        ts = _f64(ts).reshape(-1, 3)
        n = Rs.shape[0]
        outs = (LinOut * n)()
        self._check(self._L.dcreg_linearize_batch(self._h, n, _dp(Rs), _dp(ts), C.byref(params), outs), "dcreg_linearize_batch")
        return [self._out_dict(o) for o in outs]

    def reserve_warm_states(self, n_states):
        self._check(self._L.dcreg_reserve_warm_states(self._h, int(n_states)), "dcreg_reserve_warm_states")

    def hint_misalignment(self, metres):
        """Scheduling hint (never needed for correctness): expected distance of the source points from the map at the next poses."""
        self._check(self._L.dcreg_hint_misalignment(self._h, float(metres)), "dcreg_hint_misalignment")

    def reset_warm_state(self, state_id):
        self._check(self._L.dcreg_reset_warm_state(self._h, int(state_id)), "dcreg_reset_warm_state")

    def launch_stats(self, reset=False):
        """dcreg_launch_stats_get (dcreg_debug.h): how the linearisations since the last reset were carried out"""
        st = LaunchStats()
        self._check(self._L.dcreg_launch_stats_get(self._h, C.byref(st), int(reset)), "dcreg_launch_stats_get")
        return {k: int(getattr(st, k)) for k, _ in LaunchStats._fields_}

    def linearize_batch_warm(self, Rs, ts, state_ids, params=None, slot=0):
        """dcreg_linearize_batch_begin_warm + _end: pose i reads and updates warm-start state state_ids[i] (-1 = cold)."""
        params = params or default_lin_params()
        Rs = _f64(Rs).reshape(-1, 9)
        ts = _f64(ts).reshape(-1, 3)
        n = Rs.shape[0]
        ids = np.ascontiguousarray(state_ids, dtype=np.int32).reshape(n)
        outs = (LinOut * n)()
        self._check(self._L.dcreg_linearize_batch_begin_warm(self._h, slot, n, _dp(Rs), _dp(ts), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                             C.byref(params)), "dcreg_linearize_batch_begin_warm")
        self._check(self._L.dcreg_linearize_batch_end(self._h, slot, outs), "dcreg_linearize_batch_end")
        return [self._out_dict(o) for o in outs]

    # pipelined single-pose launches (what dcreg_icp_run does between two iterations)
    def linearize_begin(self, R, t, params=None, slot=0):
        params = params or default_lin_params()
        R = _f64(R).reshape(9); t = _f64(t).reshape(3)
        self._check(self._L.dcreg_linearize_batch_begin(self._h, slot, 1, _dp(R), _dp(t), C.byref(params)), "dcreg_linearize_batch_begin")

    def linearize_gated_begin(self, params=None, slot=0):
        """queue a linearisation whose pose arrives later (gate_open) or never (gate_abort)"""
        params = params or default_lin_params()
        self._check(self._L.dcreg_linearize_gated_begin(self._h, slot, C.byref(params)), "dcreg_linearize_gated_begin")

    def gate_open(self, R, t):
        R = _f64(R).reshape(9); t = _f64(t).reshape(3)
        self._check(self._L.dcreg_linearize_gate_open(self._h, _dp(R), _dp(t)), "dcreg_linearize_gate_open")

    def gate_abort(self):
        self._check(self._L.dcreg_linearize_gate_abort(self._h), "dcreg_linearize_gate_abort")

    def linearize_end(self, slot=0):
        out = (LinOut * 1)()
        self._check(self._L.dcreg_linearize_batch_end(self._h, slot, out), "dcreg_linearize_batch_end")
        return self._out_dict(out[0])

    def knn(self, q, k=5, max_radius=0.0):
        q = _points(q, "knn")
        idx = np.empty((q.shape[0], k), np.int32)
        d2 = np.empty((q.shape[0], k), np.float32)
        self._check(self._L.dcreg_knn(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], q.shape[1], k, float(max_radius),
                                      idx.ctypes.data_as(C.POINTER(C.c_int32)), d2.ctypes.data_as(C.POINTER(C.c_float))), "dcreg_knn")
        return idx, d2

    def kdtree_build(self, leaf_size=16):
        """kd-tree comparator over the current target (dcreg_debug.h); returns (depth, leaf_size, host build ms)"""
        self._check(self._L.dcreg_kdtree_build(self._h, int(leaf_size)), "dcreg_kdtree_build")
        d, l, ms = C.c_int32(), C.c_int32(), C.c_double()
        self._check(self._L.dcreg_kdtree_info(self._h, C.byref(d), C.byref(l), C.byref(ms)), "dcreg_kdtree_info")
        return d.value, l.value, ms.value

    def knn_timed(self, q, k=5, max_radius=0.0, index="grid", repeats=10):
        """exact k-NN on the grid or on the kd-tree comparator -> (idx, d2, kernel ms per launch)"""
        q = _points(q, "knn_timed")
        idx = np.empty((q.shape[0], k), np.int32)
        d2 = np.empty((q.shape[0], k), np.float32)
        ms = C.c_double()
        self._check(self._L.dcreg_knn_timed(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], q.shape[1], k, float(max_radius),
                                            {"grid": 0, "kdtree": 1, "grid_sweep": 2}[index], int(repeats), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                            d2.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ms)), "dcreg_knn_timed")
        return idx, d2, ms.value

    def launch_series(self, reset=True, cap=1 << 20):
        """dcreg_launch_series (dcreg_debug.h; option "record_launches"): per completed launch its HIP-event time (ms, -1 = untimed),
        points searched, points refitted and points linearised, which pass ran in front (dcreg_launch_series_passes: 0 / 1 / 2),
        whether the linearisation kernel ran in one-wave blocks and which kernels carried the launch out (dcreg_launch_series_structure:
        0 the linearisation kernel alone, 1 a pass and the kernel behind it, 2 the advance pass alone; its bit 2 comes back as "five":
        1 where the launch was a five-neighbour launch, option "search_five") -> dict of arrays"""
        lp = C.POINTER(C.c_int64)
        n = self._L.dcreg_launch_series(self._h, None, None, None, None, 0, 0)
        if n < 0:
            raise DcregError("dcreg_launch_series failed")
        n = min(n, cap)
        ms = np.empty(n, np.float64)
        se, rf, pt = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int64)
        adv = np.zeros(n, np.uint8)
        if hasattr(self._L, "dcreg_launch_series_passes"):
            self._L.dcreg_launch_series_passes(self._h, adv.ctypes.data_as(C.POINTER(C.c_uint8)), n)
        st = np.where((adv & 3) != 0, 1, 0).astype(np.uint8)      # (a build without the getter has the two-kernel form only)
        if hasattr(self._L, "dcreg_launch_series_structure"):
            self._L.dcreg_launch_series_structure(self._h, st.ctypes.data_as(C.POINTER(C.c_uint8)), n)
        self._L.dcreg_launch_series(self._h, _dp(ms), se.ctypes.data_as(lp), rf.ctypes.data_as(lp), pt.ctypes.data_as(lp), n, int(reset))
        return {"ms": ms, "searched": se, "refitted": rf, "points": pt, "advanced": adv & 3, "one_wave": (adv >> 2) & 1, "structure": st & 3, "five": (st >> 2) & 1}

    def team_pass_stamps(self):
        """dcreg_team_pass_stamps (option "team_stamps"): [n_blocks, 8] shader-clock words of the last launch that ran the small-frame pass"""
        n = self._L.dcreg_team_pass_stamps(self._h, None, 0)
        if n <= 0:
            return np.zeros((0, 8), np.uint64)
        st = np.zeros((n + 1, 8), np.uint64)          # the last row: outcome counts (served with slack, layers, wide, rows, list, OUT, no slack, refit)
        rc = self._L.dcreg_team_pass_stamps(self._h, st.ctypes.data_as(C.POINTER(C.c_uint64)), n + 1)
        if rc < 0:
            self._check(rc, "dcreg_team_pass_stamps")
        return st

    def roi_info(self):
        """dcreg_roi_info: the window index of a large map (dcreg_debug.h)"""
        v = (C.c_double * 11)()
        self._L.dcreg_roi_info.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._check(self._L.dcreg_roi_info(self._h, v), "dcreg_roi_info")
        return {"box_min": [v[0], v[1], v[2]], "box_max": [v[3], v[4], v[5]], "points": int(v[6]), "cell": v[7], "windows_built": int(v[8]),
                "active": bool(v[9]), "whole_map_capped": bool(v[10])}

    def kernel_time(self, reset=False):
        ms, n = C.c_double(), C.c_int64()
        self._L.dcreg_kernel_time(self._h, C.byref(ms), C.byref(n), int(reset))
        return ms.value, n.value

    def icp_run(self, T0, method, cfg, log_capacity=None):
        return self._run_logged("dcreg_icp_run", T0, method, cfg, log_capacity)

    def icp_run_sharded(self, T0, method, cfg, n_source_total, reduce_rows, log_capacity=None):
        """dcreg_icp_run_sharded: reduce_rows(numpy float64[32] view) must overwrite the row IN PLACE with the sum over
        all ranks in rank order (see dcreg_amd/pointshard.py)."""
        T0 = _f64(T0).reshape(4, 4)
        R0, t0 = np.ascontiguousarray(T0[:3, :3]).reshape(9), np.ascontiguousarray(T0[:3, 3])
        det, hand = METHODS[method] if isinstance(method, str) else method
        cap = cfg.max_iterations if log_capacity is None else log_capacity
        logs = (IterLog * max(cap, 1))()
        res = IcpResult()
        err = []

        def _cb(row_ptr, _user):
            try:
                reduce_rows(np.ctypeslib.as_array(row_ptr, shape=(32,)))
                return 0
            except Exception as e:          # never let an exception cross the C boundary
                err.append(e)
                return 1
        cb = REDUCE_FN(_cb)
        rc = self._L.dcreg_icp_run_sharded(self._h, _dp(R0), _dp(t0), DETECTION[det], HANDLING[hand], C.byref(cfg),
                                           int(n_source_total), cb, None, logs, cap, C.byref(res))
        if err:
            raise err[0]
        self._check(rc, "dcreg_icp_run_sharded")
        n = min(res.iterations, cap)
        if res.status == 1:
            n = min(res.iterations - 1, cap)
        return res, [logs[i] for i in range(max(n, 0))]

    def comm_init(self, id128, rank, world):
        """dcreg_comm_init: collective (every rank of the job calls it with the same 128 bytes from comm_unique_id())."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._check(self._L.dcreg_comm_init(self._h, C.cast(buf, C.c_void_p), int(rank), int(world)), "dcreg_comm_init")

    def comm_allgather_sum(self, row):
        row = _f64(row, 32).copy()
        self._check(self._L.dcreg_comm_allgather_sum(self._h, _dp(row)), "dcreg_comm_allgather_sum")
        return row

    def icp_run_sharded_rccl(self, T0, method, cfg, n_source_total, log_capacity=None):
        """dcreg_icp_run_sharded_rccl: point-sharded run, the per-iteration exchange is an RCCL all_gather inside the engine."""
        return self._run_logged("dcreg_icp_run_sharded_rccl", T0, method, cfg, log_capacity, extra=(int(n_source_total),))

    def icp_run_euler(self, pose6d, method, cfg, log_capacity=None):
        """Second engine (Pose6D state, LOAM Jacobian); pose6d = (roll, pitch, yaw, x, y, z).
        Returns (result, [IterLog...], final_pose6d)."""
        p0 = _f64(pose6d, 6)
        det, hand = METHODS[method] if isinstance(method, str) else method
        cap = cfg.max_iterations if log_capacity is None else log_capacity
        logs = (IterLog * max(cap, 1))()
        res = IcpResult()
        pf = np.zeros(6)
        self._check(self._L.dcreg_icp_run_euler(self._h, _dp(p0), DETECTION[det], HANDLING[hand], C.byref(cfg), logs, cap,
                                                C.byref(res), _dp(pf)), "dcreg_icp_run_euler")
        return res, [logs[i] for i in range(max(min(res.iterations, cap), 0))], pf

    def icp_run_montecarlo(self, base_xyzrpy, seed, first_trial, trial_stride, n_trials, trans_amp, rot_amp_rad, method, cfg, slots=0):
        """dcreg_icp_run_montecarlo: this rank's share of the Monte-Carlo experiment, poses generated and trials batched in C++."""
        det, hand = METHODS[method]
        res = (TrialResult * max(int(n_trials), 1))()
        self._check(self._L.dcreg_icp_run_montecarlo(self._h, _dp(_f64(base_xyzrpy, 6)), int(seed), int(first_trial), int(trial_stride), int(n_trials),
                                                     float(trans_amp), float(rot_amp_rad), DETECTION[det], HANDLING[hand], C.byref(cfg), int(slots), res),
                    "dcreg_icp_run_montecarlo")
        return [res[i] for i in range(int(n_trials))]

    def montecarlo_job(self, base_xyzrpy, seed, n_trials, trans_amp, rot_amp_rad, method, cfg, slots=0, want_records=True):
        """dcreg_montecarlo_job: the whole experiment as one C-ABI job over the ranks of this context's communicator (comm_init; none = one
        rank): shard, run, ONE ncclAllGather, statistics - on every rank.  -> (records [n_trials, 64] float64 or None, stats dict)"""
        det, hand = METHODS[method]
        n = int(n_trials)
        rec = np.zeros((max(n, 1), 64)) if want_records else None
        st = MethodStats()
        self._check(self._L.dcreg_montecarlo_job(self._h, _dp(_f64(base_xyzrpy, 6)), int(seed), n, float(trans_amp), float(rot_amp_rad), DETECTION[det],
                                                 HANDLING[hand], C.byref(cfg), int(slots), _dp(rec) if want_records else None, C.byref(st)),
                    "dcreg_montecarlo_job")
        return (rec[:n] if want_records else None), {k: getattr(st, k) for k, _ in MethodStats._fields_}

    def comm_allgather(self, row):
        """dcreg_comm_allgather: this rank's doubles -> [world, len(row)] on every rank"""
        rank, world = C.c_int(), C.c_int()
        self._L.dcreg_comm_info(self._h, C.byref(rank), C.byref(world))
        row = _f64(row).reshape(-1)
        out = np.zeros((world.value, len(row)))
        self._check(self._L.dcreg_comm_allgather(self._h, _dp(row), _dp(out), len(row)), "dcreg_comm_allgather")
        return out

    def _run_trials(self, symbol, T0s, method, cfg, what=None):
        """icp_run_trials and the other engines' forms: one record per pose; what: the wrapper refuses an unknown method name itself"""
        R0, t0, n = _poses_arg(T0s)
        det, hand = _method(method, what)
        res = (TrialResult * max(n, 1))()
        self._check(getattr(self._L, symbol)(self._h, n, _dp(R0), _dp(t0), det, hand, C.byref(cfg), res), symbol)
        return [res[i] for i in range(n)]

    def _register_frames(self, symbol, frames, T0s, method, cfg, slots, what, check_method=True, extra_args=()):
        """register_frames and the other engines' forms: one record per frame; extra_args: the call's arguments between the frames and the
        poses"""
        xyz, off, n = _frames_arg(frames, what)
        R0, t0, n_poses = _poses_arg(T0s)
        if n_poses != n:
            raise ValueError("one initial pose per frame: %d frames, %d poses" % (n, n_poses))
        det, hand = _method(method, what if check_method else None)
        res = (TrialResult * max(n, 1))()
        self._check(getattr(self._L, symbol)(self._h, n, xyz.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)), xyz.shape[1],
                                             *extra_args, _dp(R0), _dp(t0), det, hand, C.byref(cfg), int(slots), res), symbol)
        self._n_frames = n            # (the call loaded its frames: frames_normals_keep sizes its infos by it)
        return [res[i] for i in range(n)]

    def icp_run_trials(self, T0s, method, cfg):
        return self._run_trials("dcreg_icp_run_trials", T0s, method, cfg)

    def register_frames(self, frames, T0s, method, cfg, slots=0):
        """dcreg_register_frames: many frames against this context's map in one call.  frames = a list of [n_i, c] float32 arrays, or
        (xyz [N, c], offsets [n_frames + 1]) with frame f = xyz[offsets[f]:offsets[f + 1]] (c >= 3 columns, x y z first: an xyzi array is
        passed as it is, the rows c floats apart); T0s = one initial 4x4 pose per frame.  Returns one record per frame, as icp_run_trials does;
        each is bitwise set_source(frame) + icp_run(T0) on this context."""
        return self._register_frames("dcreg_register_frames", frames, T0s, method, cfg, slots, "register_frames", check_method=False)

    def register_frames_normals(self, frames, T0s, method, cfg, slots=0):
        """dcreg_register_frames_normals: register_frames with the second engine (the map's kept normals: keep_target_normals or
        set_target_normals first).  Same arguments and records; each record is bitwise set_source(frame) + icp_run_normals(T0)."""
        return self._register_frames("dcreg_register_frames_normals", frames, T0s, method, cfg, slots, "register_frames_normals")

    def icp_run_trials_normals(self, T0s, method, cfg):
        """dcreg_icp_run_trials_normals: icp_run_trials with the second engine; each record is bitwise icp_run_normals from its pose"""
        return self._run_trials("dcreg_icp_run_trials_normals", T0s, method, cfg, "icp_run_trials_normals")

    # ---- the device seam of the two calls above (include/dcreg_debug.h), for the tests
    def frames_load(self, frames):
        """dcreg_frames_load: the frames (as register_frames takes them) onto the device"""
        xyz, off, n = _frames_arg(frames, "frames_load")
        self._check(self._L.dcreg_frames_load(self._h, n, xyz.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)), xyz.shape[1]),
                    "dcreg_frames_load")
        self._n_frames = n            # (frames_normals_keep sizes its per-frame infos by the frames on the device)

    def normals_reserve_slots(self, n_slots, frames=True):
        self._check(self._L.dcreg_normals_reserve_slots(self._h, int(n_slots), 1 if frames else 0), "dcreg_normals_reserve_slots")

    def normals_reset_slot(self, slot_id):
        self._check(self._L.dcreg_normals_reset_slot(self._h, int(slot_id)), "dcreg_normals_reset_slot")

    def _batch_begin(self, symbol, what, Ts, state_ids, frame_ids, params, slot):
        """normals_batch_begin / gicp_batch_begin -> the number of poses"""
        params = self._nlin_params(params, what)
        Rs, ts, n = _poses_arg(Ts)
        i32p = C.POINTER(C.c_int32)
        ids = None if state_ids is None else np.ascontiguousarray(state_ids, dtype=np.int32).reshape(n)
        fids = None if frame_ids is None else np.ascontiguousarray(frame_ids, dtype=np.int32).reshape(n)
        self._check(getattr(self._L, symbol)(self._h, int(slot), n, _dp(Rs), _dp(ts), None if ids is None else ids.ctypes.data_as(i32p),
                                             None if fids is None else fids.ctypes.data_as(i32p), C.byref(params)), symbol)
        return n

    def _batch_end(self, symbol, n_poses, slot):
        """normals_batch_end / gicp_batch_end -> one dict per pose"""
        outs = (LinOut * max(int(n_poses), 1))()
        self._check(getattr(self._L, symbol)(self._h, int(slot), outs), symbol)
        return [self._out_dict(outs[i]) for i in range(int(n_poses))]

    def normals_batch_begin(self, Ts, state_ids=None, frame_ids=None, params=None, slot=0):
        """dcreg_normals_batch_begin: one launch over the poses Ts ([n, 4, 4]); pose i linearises frame frame_ids[i] of the loaded frames
        (None: the own source) with warm slot state_ids[i] (-1, or None: cold).  -> the number of poses, for normals_batch_end"""
        return self._batch_begin("dcreg_normals_batch_begin", "normals_batch_begin", Ts, state_ids, frame_ids, params, slot)

    def normals_batch_end(self, n_poses, slot=0):
        """dcreg_normals_batch_end -> one dict per pose, as linearize_normals returns"""
        return self._batch_end("dcreg_normals_batch_end", n_poses, slot)

    def normals_batch(self, Ts, state_ids=None, frame_ids=None, params=None, slot=0):
        return self.normals_batch_end(self.normals_batch_begin(Ts, state_ids, frame_ids, params, slot), slot)

    # ---- the third engine's many-frames form (include/dcreg.h: dcreg_register_frames_gicp, dcreg_icp_run_trials_gicp) and its device seam
    # (include/dcreg_debug.h: dcreg_frames_normals_*, dcreg_gicp_batch_begin / _end)
    def register_frames_gicp(self, frames, T0s, method, cfg, frame_normals=None, slots=0):
        """dcreg_register_frames_gicp: register_frames with the third engine (the map's kept normals first; every frame's own normals are
        estimated with frame_normals = normal_params(...), None = the defaults, all frames in one batched pass).  Same arguments and
        records; each record is bitwise set_source(frame) + keep_source_normals(frame_normals) + icp_run_gicp(T0)."""
        p = frame_normals if frame_normals is not None else normal_params()
        _check_normal_params(p, "register_frames_gicp")
        return self._register_frames("dcreg_register_frames_gicp", frames, T0s, method, cfg, slots, "register_frames_gicp", extra_args=(C.byref(p),))

    def icp_run_trials_gicp(self, T0s, method, cfg):
        """dcreg_icp_run_trials_gicp: icp_run_trials with the third engine (kept map normals and kept source normals first); each record is
        bitwise icp_run_gicp from its pose"""
        return self._run_trials("dcreg_icp_run_trials_gicp", T0s, method, cfg, "icp_run_trials_gicp")

    def frames_normals_keep(self, params=None):
        """dcreg_frames_normals_keep: the loaded frames' own normals, all frames in one batched pass, kept beside their points
        -> [info dict per frame]"""
        p = params if params is not None else normal_params()
        _check_normal_params(p, "frames_normals_keep")
        n = self._n_frames
        infos = (NormalInfo * max(n, 1))()
        self._check(self._L.dcreg_frames_normals_keep(self._h, C.byref(p), infos), "dcreg_frames_normals_keep")
        return [_normal_info_dict(infos[s]) for s in range(n)]

    def frames_normals_set(self, normals):
        """dcreg_frames_normals_set: the caller's normals ([N, c >= 3] float32, or a list with one array per frame) for all points of the
        load in its upload order, kept as given"""
        if isinstance(normals, (list, tuple)):
            parts = [_points(a, "frames_normals_set") for a in normals]
            if len({a.shape[1] for a in parts}) > 1:
                raise ValueError("frames_normals_set: every frame's normals need the same number of columns")
            a = np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.float32))
        else:
            a = _points(normals, "frames_normals_set")
        self._check(self._L.dcreg_frames_normals_set(self._h, a.ctypes.data, a.shape[0], a.shape[1]), "dcreg_frames_normals_set")

    def frames_normals_kept(self):
        return int(self._L.dcreg_frames_normals_kept(self._h))

    def gicp_batch_begin(self, Ts, state_ids=None, frame_ids=None, params=None, slot=0):
        """dcreg_gicp_batch_begin: normals_batch_begin for linearize_gicp - pose i linearises frame frame_ids[i] with its kept frame
        normals (None: the own source with its kept source normals).  -> the number of poses, for gicp_batch_end"""
        return self._batch_begin("dcreg_gicp_batch_begin", "gicp_batch_begin", Ts, state_ids, frame_ids, params, slot)

    def gicp_batch_end(self, n_poses, slot=0):
        """dcreg_gicp_batch_end -> one dict per pose, as linearize_gicp returns"""
        return self._batch_end("dcreg_gicp_batch_end", n_poses, slot)

    def gicp_batch(self, Ts, state_ids=None, frame_ids=None, params=None, slot=0):
        return self.gicp_batch_end(self.gicp_batch_begin(Ts, state_ids, frame_ids, params, slot), slot)

    @staticmethod
    def _pairs_args(sources, targets, T0s, what):
        """the argument checks of register_pairs and the other engines' forms -> (source points, source offsets, target points, target
        offsets, columns, R0 [n, 9], t0 [n, 3], n)"""
        if len(sources) != len(targets):
            raise ValueError("%s: one target per source: %d sources, %d targets" % (what, len(sources), len(targets)))
        src = [_points(f, what) for f in sources]
        tgt = [_points(f, what) for f in targets]
        widths = {f.shape[1] for f in src + tgt}
        if len(widths) > 1:
            raise ValueError("%s: every cloud needs the same number of columns, got %s" % (what, sorted(widths)))
        width = widths.pop() if widths else 3
        n = len(src)
        T0s = _f64(T0s).reshape(-1, 4, 4)
        if T0s.shape[0] != n:
            raise ValueError("one initial pose per pair: %d pairs, %d poses" % (n, T0s.shape[0]))

        def pack(parts):
            off = np.zeros(n + 1, np.int64)
            off[1:] = np.cumsum([len(f) for f in parts])
            xyz = np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0, width), np.float32))
            return xyz, off
        sxyz, soff = pack(src)
        txyz, toff = pack(tgt)
        R0 = np.ascontiguousarray(T0s[:, :3, :3]).reshape(n, 9)
        t0 = np.ascontiguousarray(T0s[:, :3, 3]).reshape(n, 3)
        return sxyz, soff, txyz, toff, width, R0, t0, n

    def _register_pairs(self, symbol, what, sources, targets, T0s, method, cfg, slots, extra_args=()):
        """register_pairs and the other engines' forms: one record per pair; extra_args: the call's arguments between the clouds and the
        poses"""
        sxyz, soff, txyz, toff, width, R0, t0, n = self._pairs_args(sources, targets, T0s, what)
        det, hand = METHODS[method] if isinstance(method, str) else method
        res = (TrialResult * max(n, 1))()
        fp = C.POINTER(C.c_float)
        i64p = C.POINTER(C.c_int64)
        self._check(getattr(self._L, symbol)(self._h, n, sxyz.ctypes.data_as(fp), soff.ctypes.data_as(i64p), txyz.ctypes.data_as(fp),
                                             toff.ctypes.data_as(i64p), width, *extra_args, _dp(R0), _dp(t0), DETECTION[det], HANDLING[hand],
                                             C.byref(cfg), int(slots), res), symbol)
        return [res[i] for i in range(n)]

    def register_pairs(self, sources, targets, T0s, method, cfg, slots=0):
        """dcreg_register_pairs: many scan pairs in one call, pair p = sources[p] registered against targets[p] from T0s[p].  sources and
        targets = lists of equal length of [n_i, c] float32 arrays (c >= 3 columns, x y z first, the same c for every cloud: the rows are
        passed c floats apart); T0s = one initial 4x4 pose per pair.  The targets are indexed for cfg.search_radius.  Needs no map on this
        context and leaves it as it was.  Returns one record per pair, as icp_run_trials does; each is bitwise set_target(target,
        cfg.search_radius) + set_source(source) + icp_run(T0) on a context with the same options."""
        return self._register_pairs("dcreg_register_pairs", "register_pairs", sources, targets, T0s, method, cfg, slots)

    def register_pairs_normals(self, sources, targets, T0s, method, cfg, target_normals=None, slots=0):
        """dcreg_register_pairs_normals: register_pairs with the second engine.  Every target's normals are estimated with target_normals
        = normal_params(...), None = the defaults, all targets of a build batch in one launch.  Same arguments and records; each record is
        bitwise set_target(target, cfg.search_radius) + keep_target_normals(target_normals) + set_source(source) + icp_run_normals(T0)."""
        tn = target_normals if target_normals is not None else normal_params()
        _check_normal_params(tn, "register_pairs_normals")
        return self._register_pairs("dcreg_register_pairs_normals", "register_pairs_normals", sources, targets, T0s, method, cfg, slots,
                                    extra_args=(C.byref(tn),))

    def register_pairs_gicp(self, sources, targets, T0s, method, cfg, target_normals=None, source_normals=None, slots=0):
        """dcreg_register_pairs_gicp: register_pairs with the third engine.  target_normals as register_pairs_normals takes it;
        source_normals: the rule of every source's own normals (None = the defaults), all sources in one batched pass.  Each record is
        bitwise set_target(target, cfg.search_radius) + keep_target_normals(target_normals) + set_source(source) +
        keep_source_normals(source_normals) + icp_run_gicp(T0)."""
        tn = target_normals if target_normals is not None else normal_params()
        sn = source_normals if source_normals is not None else normal_params()
        _check_normal_params(tn, "register_pairs_gicp")
        _check_normal_params(sn, "register_pairs_gicp")
        return self._register_pairs("dcreg_register_pairs_gicp", "register_pairs_gicp", sources, targets, T0s, method, cfg, slots,
                                    extra_args=(C.byref(tn), C.byref(sn)))

    # ---- the device seam of the two calls above (include/dcreg_debug.h), for the tests
    def pairs_sources_load(self, sources):
        """dcreg_pairs_sources_load: the pairs' sources (a list of [n_i, c] arrays) onto the device"""
        xyz, off, n = _frames_arg(sources, "pairs_sources_load")
        self._check(self._L.dcreg_pairs_sources_load(self._h, n, xyz.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     xyz.shape[1]), "dcreg_pairs_sources_load")
        self._n_pair_sources, self._n_pair_source_points = n, int(off[-1]) if n else 0

    def pairs_build(self, targets, search_radius):
        """dcreg_pairs_build: the targets of one build batch (a list of [n_i, c] arrays) indexed for search_radius"""
        xyz, off, n = _frames_arg(targets, "pairs_build")
        self._check(self._L.dcreg_pairs_build(self._h, n, xyz.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                              xyz.shape[1], float(search_radius)), "dcreg_pairs_build")
        self._n_pair_targets, self._n_pair_target_points = n, int(off[-1]) if n else 0

    def _pairs_keep(self, symbol, params, n):
        p = params if params is not None else normal_params()
        _check_normal_params(p, symbol[len("dcreg_"):])
        infos = (NormalInfo * max(n, 1))()
        self._check(getattr(self._L, symbol)(self._h, C.byref(p), infos), symbol)
        return [_normal_info_dict(infos[s]) for s in range(n)]

    def _pairs_set(self, symbol, normals):
        what = symbol[len("dcreg_"):]
        if isinstance(normals, (list, tuple)):
            parts = [_points(a, what) for a in normals]
            if len({a.shape[1] for a in parts}) > 1:
                raise ValueError("%s: every cloud's normals need the same number of columns" % what)
            a = np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.float32))
        else:
            a = _points(normals, what)
        self._check(getattr(self._L, symbol)(self._h, a.ctypes.data, a.shape[0], a.shape[1]), symbol)

    def _pairs_get(self, symbol, n):
        out = np.empty((max(n, 1), 4), np.float32)
        self._check(getattr(self._L, symbol)(self._h, out.ctypes.data, n), symbol)
        return out[:n]

    def pairs_normals_keep(self, params=None):
        """dcreg_pairs_normals_keep: the kept normals of the build batch's targets, one launch -> [info dict per target]"""
        return self._pairs_keep("dcreg_pairs_normals_keep", params, getattr(self, "_n_pair_targets", 0))

    def pairs_normals_set(self, normals):
        """dcreg_pairs_normals_set: the caller's normals ([N, c >= 3], or one array per target) for all points of the batch, as given"""
        self._pairs_set("dcreg_pairs_normals_set", normals)

    def pairs_normals_get(self):
        """dcreg_pairs_normals_get -> [N, 4] float32: normal and curvature of every point of the batch, target after target"""
        return self._pairs_get("dcreg_pairs_normals_get", getattr(self, "_n_pair_target_points", 0))

    def pairs_normals_kept(self):
        return int(self._L.dcreg_pairs_normals_kept(self._h))

    def pairs_sources_normals_keep(self, params=None):
        """dcreg_pairs_sources_normals_keep: the loaded pair sources' own normals, one batched pass -> [info dict per source]"""
        return self._pairs_keep("dcreg_pairs_sources_normals_keep", params, getattr(self, "_n_pair_sources", 0))

    def pairs_sources_normals_set(self, normals):
        self._pairs_set("dcreg_pairs_sources_normals_set", normals)

    def pairs_sources_normals_get(self):
        """dcreg_pairs_sources_normals_get -> [N, 4] float32 in the upload order of the load"""
        return self._pairs_get("dcreg_pairs_sources_normals_get", getattr(self, "_n_pair_source_points", 0))

    def pairs_normals_reserve_slots(self, n_slots):
        self._check(self._L.dcreg_pairs_normals_reserve_slots(self._h, int(n_slots)), "dcreg_pairs_normals_reserve_slots")

    def _pairs_batch_begin(self, symbol, Ts, source_ids, target_ids, state_ids, params, slot):
        params = self._nlin_params(params, symbol[len("dcreg_"):])
        Rs, ts, n = _poses_arg(Ts)
        i32p = C.POINTER(C.c_int32)
        ids = None if state_ids is None else np.ascontiguousarray(state_ids, dtype=np.int32).reshape(n)
        sids = np.ascontiguousarray(source_ids, dtype=np.int32).reshape(n)
        tids = np.ascontiguousarray(target_ids, dtype=np.int32).reshape(n)
        self._check(getattr(self._L, symbol)(self._h, int(slot), n, _dp(Rs), _dp(ts), None if ids is None else ids.ctypes.data_as(i32p),
                                             sids.ctypes.data_as(i32p), tids.ctypes.data_as(i32p), C.byref(params)), symbol)
        return n

    def pairs_normals_batch(self, Ts, source_ids, target_ids, state_ids=None, params=None, slot=0):
        """dcreg_pairs_normals_batch_begin + dcreg_normals_batch_end: pose i linearises pair source source_ids[i] against target
        target_ids[i] of the build batch and its kept normals -> one dict per pose, as linearize_normals returns"""
        n = self._pairs_batch_begin("dcreg_pairs_normals_batch_begin", Ts, source_ids, target_ids, state_ids, params, slot)
        return self.normals_batch_end(n, slot)

    def pairs_gicp_batch(self, Ts, source_ids, target_ids, state_ids=None, params=None, slot=0):
        """dcreg_pairs_gicp_batch_begin + dcreg_normals_batch_end: the same for linearize_gicp, with the sources' kept normals"""
        n = self._pairs_batch_begin("dcreg_pairs_gicp_batch_begin", Ts, source_ids, target_ids, state_ids, params, slot)
        return self.normals_batch_end(n, slot)

    # ---- the fourth engine's pairs form (include/dcreg.h: dcreg_register_pairs_voxels) and its device seam (include/dcreg_debug.h:
    # dcreg_pairs_voxels_build / _get / _kept, dcreg_pairs_voxels_batch_begin)
    def register_pairs_voxels(self, sources, targets, T0s, method, cfg, target_voxels=None, source_normals=None, slots=0):
        """dcreg_register_pairs_voxels: register_pairs with the fourth engine - a voxel map per target (target_voxels =
        voxel_map_params(...), None = the defaults) instead of an index.  source_normals = normal_params(...) is the rule every source's
        own normals are estimated with when set_option("voxels_source_cov", 1) is on - it is required then - and is not read otherwise
        (None: a null pointer is passed).  Each record is bitwise set_target(target, any radius) + keep_target_voxels(target_voxels) +
        set_source(source) [+ keep_source_normals(source_normals)] + icp_run_voxels(T0), at the "voxels_neighbors" in force when the call starts; a target that keeps no voxel gives status 3."""
        tv = target_voxels if target_voxels is not None else voxel_map_params()
        _check_voxel_map_params(tv, "register_pairs_voxels")
        if source_normals is not None:
            _check_normal_params(source_normals, "register_pairs_voxels")
        return self._register_pairs("dcreg_register_pairs_voxels", "register_pairs_voxels", sources, targets, T0s, method, cfg, slots,
                                    extra_args=(C.byref(tv), None if source_normals is None else C.byref(source_normals)))

    def pairs_voxels_build(self, targets, params=None):
        """dcreg_pairs_voxels_build: the targets of one build batch (a list of [n_i, c] arrays) uploaded, packed and every one's voxel map
        kept, all at once; no grid is built -> [info dict per target], as keep_target_voxels returns"""
        p = params if params is not None else voxel_map_params()
        _check_voxel_map_params(p, "pairs_voxels_build")
        xyz, off, n = _frames_arg(targets, "pairs_voxels_build")
        infos = (VoxelMapInfo * max(n, 1))()
        self._check(self._L.dcreg_pairs_voxels_build(self._h, n, xyz.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     xyz.shape[1], C.byref(p), infos), "dcreg_pairs_voxels_build")
        return [{k: int(getattr(infos[t], k)) for k, _ in VoxelMapInfo._fields_} for t in range(n)]

    def pairs_voxels_kept(self, t):
        """dcreg_pairs_voxels_kept: the kept voxels of target t of the pairs' voxel batch, 0 without a member"""
        return int(self._L.dcreg_pairs_voxels_kept(self._h, int(t)))

    def pairs_kept_voxels(self, t):
        """dcreg_pairs_voxels_get: target t's member of the pairs' voxel batch -> the dict kept_target_voxels returns"""
        n = self.pairs_voxels_kept(t)
        m = max(n, 1)
        coords, count = np.zeros((m, 3), np.int64), np.zeros(m, np.int32)
        mean, cov = np.zeros((m, 3), np.float32), np.zeros((m, 6), np.float32)
        self._check(self._L.dcreg_pairs_voxels_get(self._h, int(t), coords.ctypes.data, count.ctypes.data, mean.ctypes.data, cov.ctypes.data, n),
                    "dcreg_pairs_voxels_get")
        return {"coords": coords[:n], "count": count[:n], "mean": mean[:n], "cov": cov[:n]}

    def pairs_voxels_batch_begin(self, Ts, source_ids, target_ids, params=None, slot=0):
        """dcreg_pairs_voxels_batch_begin: one launch over the poses Ts; pose i linearises pair source source_ids[i] against the voxel map
        of target target_ids[i] of the batch; "voxels_neighbors" is read here, with the other options.  -> the number of poses, for
        voxels_batch_end"""
        params = self._vlin_params(params, "pairs_voxels_batch_begin")
        Rs, ts, n = _poses_arg(Ts)
        i32p = C.POINTER(C.c_int32)
        sids = np.ascontiguousarray(source_ids, dtype=np.int32).reshape(n)
        tids = np.ascontiguousarray(target_ids, dtype=np.int32).reshape(n)
        self._check(self._L.dcreg_pairs_voxels_batch_begin(self._h, int(slot), n, _dp(Rs), _dp(ts), sids.ctypes.data_as(i32p), tids.ctypes.data_as(i32p),
                                                           C.byref(params)), "dcreg_pairs_voxels_batch_begin")
        return n

    def pairs_voxels_batch(self, Ts, source_ids, target_ids, params=None, slot=0):
        """pairs_voxels_batch_begin + voxels_batch_end -> one dict per pose, as linearize_voxels returns"""
        return self.voxels_batch_end(self.pairs_voxels_batch_begin(Ts, source_ids, target_ids, params, slot), slot)

    def insert(self, xyz, T, min_spacing=0.0):
        """dcreg_target_insert: the points xyz (body frame) transformed by the 4x4 pose T appended to the map, except those with a map point
        closer than min_spacing (> 0) -> dict n_offered / n_added / n_removed / n_target / rebuilt"""
        a = _points(xyz, "insert")
        R, t = _pose_rt(T, "insert")
        u = MapUpdate()
        self._check(self._L.dcreg_target_insert(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], a.shape[1], _dp(R), _dp(t),
                                                float(min_spacing), C.byref(u)), "dcreg_target_insert")
        return _update_dict(u)

    def insert_device(self, dev_ptr, n, stride, T, min_spacing=0.0):
        R, t = _pose_rt(T, "insert_device")
        u = MapUpdate()
        self._check(self._L.dcreg_target_insert_device(self._h, C.c_void_p(dev_ptr), int(n), int(stride), _dp(R), _dp(t), float(min_spacing),
                                                       C.byref(u)), "dcreg_target_insert_device")
        return _update_dict(u)

    def insert_source(self, T, min_spacing=0.0):
        """dcreg_target_insert_source: the source of the last set_source, transformed by T (typically the registration's result), into the map"""
        R, t = _pose_rt(T, "insert_source")
        u = MapUpdate()
        self._check(self._L.dcreg_target_insert_source(self._h, _dp(R), _dp(t), float(min_spacing), C.byref(u)), "dcreg_target_insert_source")
        return _update_dict(u)

    def crop(self, lo, hi):
        """dcreg_target_crop: keep the map points inside the box lo .. hi (inclusive, per axis)"""
        lo = _f64(lo)
        hi = _f64(hi)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("crop: lo and hi are 3 coordinates each, got shapes %s and %s" % (lo.shape, hi.shape))
        u = MapUpdate()
        self._check(self._L.dcreg_target_crop(self._h, _dp(lo), _dp(hi), C.byref(u)), "dcreg_target_crop")
        return _update_dict(u)

    def target_points(self):
        """the map in index order, float32 [n, 3] (dcreg_target_get)"""
        n = self.index_info().n_target
        out = np.empty((max(n, 0), 3), np.float32)
        self._check(self._L.dcreg_target_get(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n), "dcreg_target_get")
        return out

    def index_check(self):
        """dcreg_debug_index_check: differing entries of sorted points, cell table, row words, gap field and owners against a full build
        of the current grid (all zero = exact)"""
        mm = (C.c_int64 * 5)()
        self._check(self._L.dcreg_debug_index_check(self._h, mm), "dcreg_debug_index_check")
        return dict(zip(("points", "table", "row_words", "gap", "owner"), [int(v) for v in mm]))

    def p2p_error(self, T, error_threshold):
        r, f, ch = C.c_double(), C.c_double(), C.c_double()
        v = C.c_int64()
        self._check(self._L.dcreg_p2p_error(self._h, _dp(_f64(T, 16)), float(error_threshold), C.byref(r), C.byref(f), C.byref(ch),
                                            C.byref(v)), "dcreg_p2p_error")
        return r.value, f.value, ch.value, v.value
