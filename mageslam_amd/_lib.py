"""ctypes binding of libmage_hot.so (the C-ABI in include/mage_hot.h).

The product path has no CPU fallback: if the HIP library is missing this module raises at
import, and every call that needs a GPU fails with MageError(MAGE_EDEVICE).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "_lib" / "libmage_hot.so"

MAGE_OK, MAGE_EINVAL, MAGE_EDEVICE, MAGE_ENOMEM, MAGE_EUNSUPPORTED, MAGE_ECAPACITY = range(6)
MAGE_TETHER_DISTANCE, MAGE_TETHER_ROTATION, MAGE_TETHER_TRANSFORM = range(3)
STATUS_NAMES = {0: "MAGE_OK", 1: "MAGE_EINVAL", 2: "MAGE_EDEVICE", 3: "MAGE_ENOMEM",
                4: "MAGE_EUNSUPPORTED", 5: "MAGE_ECAPACITY"}

# Every entry point declared in include/mage_hot.h (checked by tests/test_capi.py).
EXPORTS = [
    "mage_version", "mage_last_error", "mage_pool_trim", "mage_profile_enable", "mage_profile_filter", "mage_profile_reset",
    "mage_profile_report", "mage_orb_create", "mage_orb_destroy", "mage_orb_detect_and_compute",
    "mage_orb_detect_and_compute_batch_device", "mage_orb_status", "mage_orb_reset_status",
    "mage_orb_set_fast_gate", "mage_orb_fast_gate_stats",
    "mage_synth_frames_device", "mage_synth_scene_device", "mage_orb_fast_score_map",
    "mage_debug_fast_tile_plan",
    "mage_undistort_keypoints", "mage_undistort_keypoints_batch_device",
    "mage_undistorter_create", "mage_undistorter_destroy", "mage_undistorter_get_maps", "mage_undistort_image",
    "mage_undistort_image_batch_device", "mage_resize_linear_device", "mage_scale_for_camera_configuration",
    "mage_scale_image_for_camera_configuration_device", "mage_overlap_crop_source_in_target",
    "mage_hamming_distance", "mage_hamming_match", "mage_hamming_match_batch_device",
    "mage_radius_match", "mage_radius_match_batch_device", "mage_local_map_match",
    "mage_bow_create", "mage_bow_destroy", "mage_bow_train", "mage_bow_train_kmedoid", "mage_bow_get_tree", "mage_bow_find_leaves", "mage_bow_find_leaves_device",
    "mage_indexed_match", "mage_indexed_match_batch_device",
    "mage_ba_create", "mage_ba_destroy", "mage_ba_set_cameras", "mage_ba_fix_camera",
    "mage_ba_set_points", "mage_ba_set_observations", "mage_ba_set_lambda", "mage_ba_get_lambda",
    "mage_ba_set_tethers", "mage_ba_step", "mage_ba_get_poses", "mage_ba_get_points",
    "mage_ba_get_stats", "mage_ba_get_state_f64", "mage_ba_pose_batch", "mage_ba_pose_batch_device",
    "mage_track_sequence", "mage_track_sequence_device",
    "mage_new_map_points", "mage_new_map_points_host", "mage_new_map_points_batch_device",
    "mage_new_points_associate", "mage_new_points_associate_host", "mage_new_points_associate_batch_device",
    "mage_stereo_map_init", "mage_debug_stereo_init_host",
    "mage_stereo_init_triangulate", "mage_stereo_init_triangulate_batch_device", "mage_stereo_init_triangulate_host",
    "mage_mono_init_trace_bytes", "mage_mono_init_scratch_bytes",
    "mage_mono_init_two_view", "mage_mono_init_two_view_batch_device", "mage_mono_init_two_view_host",
    "mage_mono_init_third_scratch_bytes", "mage_mono_init_third_frame_batch_device", "mage_mono_init_third_frame",
    "mage_mono_init_third_frame_host",
    "mage_reloc_pnp_trace_bytes", "mage_reloc_pnp_scratch_bytes", "mage_reloc_pnp_batch_device", "mage_reloc_pnp",
    "mage_reloc_pnp_host", "mage_debug_reloc_pnp_update", "mage_debug_reloc_pnp_loop",
    "mage_reloc_guided_scratch_bytes", "mage_reloc_guided_batch_device", "mage_reloc_guided", "mage_reloc_guided_host",
    "mage_reloc_guided_choose_host", "mage_reloc_candidates_batch_device",
    "mage_bounding_plane_depths_host", "mage_bounding_plane_depths", "mage_bounding_plane_depths_batch_device",
    "mage_voi_settings_prepare", "mage_voi_teardrop_host", "mage_volume_of_interest_host", "mage_volume_of_interest",
    "mage_volume_of_interest_scratch_bytes", "mage_volume_of_interest_batch_device",
    "mage_map_points_refresh_host", "mage_map_points_refresh", "mage_map_points_refresh_batch_device",
    "mage_cheap_loop_closure_host", "mage_cheap_loop_closure", "mage_cheap_loop_closure_batch_device",
]


class MageError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class Calibration(C.Structure):
    """mage_calibration: CameraCalibration's linear intrinsics + OpenCV-ordered distortion."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("dist", C.c_float * 8), ("ndist", C.c_int32)]

    @classmethod
    def make(cls, fx, fy, cx, cy, dist=()):
        d = list(dist)
        if len(d) not in (0, 5, 8):
            raise ValueError("distortion: 0 (None), 5 (Poly3k) or 8 (Rational6k) coefficients")
        return cls(fx, fy, cx, cy, (C.c_float * 8)(*(d + [0.0] * (8 - len(d)))), len(d))


class CameraConfig(C.Structure):
    """mage_camera_config: MAGESlam::CameraConfiguration (Extrinsics M11..M44 row-major, Size) with
    its undistorted pinhole calibration."""
    _fields_ = [("extrinsics", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32)]

    @classmethod
    def make(cls, extrinsics, fx, fy, cx, cy, width, height):
        e = np.asarray(extrinsics, np.float32).reshape(16)
        return cls((C.c_float * 16)(*e.tolist()), fx, fy, cx, cy, width, height)


class KeyPoint(C.Structure):
    """cv::KeyPoint layout (28 B)."""

    _fields_ = [("x", C.c_float), ("y", C.c_float), ("size", C.c_float), ("angle", C.c_float),
                ("response", C.c_float), ("octave", C.c_int32), ("class_id", C.c_int32)]


class OrbSettingsC(C.Structure):
    _fields_ = [("gaussian_kernel_size", C.c_uint32), ("nfeatures", C.c_uint32),
                ("scale_factor", C.c_float), ("nlevels", C.c_uint32), ("patch_size", C.c_uint32),
                ("fast_threshold", C.c_uint32), ("use_orientation", C.c_int32),
                ("feature_factor", C.c_float), ("feature_strength", C.c_float),
                ("strong_response", C.c_int32), ("min_robust_factor", C.c_float),
                ("max_robust_factor", C.c_float), ("num_cells_x", C.c_int32),
                ("num_cells_y", C.c_int32)]


class TrackSettingsC(C.Structure):
    """mage_track_settings (include/mage_hot.h)."""
    _fields_ = [("search_radius", C.c_float), ("wider_search_radius", C.c_float),
                ("extra_wider_search_radius", C.c_float), ("small_match_ratio", C.c_double),
                ("min_matches", C.c_uint32), ("max_hamming", C.c_int32), ("min_hamming_difference", C.c_int32),
                ("initial_steps", C.c_uint32), ("initial_huber", C.c_float), ("initial_max_error", C.c_double),
                ("final_steps", C.c_uint32), ("final_huber", C.c_float), ("final_max_error", C.c_double),
                ("refinement_info", C.c_float), ("keyframe_ratio", C.c_double), ("keyframe_min", C.c_uint32),
                ("local_map_keyframes", C.c_uint32), ("match_search_radius", C.c_float),
                ("local_max_hamming", C.c_int32), ("local_min_hamming_difference", C.c_int32),
                ("min_view_cos", C.c_float), ("image_border", C.c_float), ("min_tracked", C.c_uint32),
                ("scale_factor", C.c_float), ("num_levels", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("local_ba", C.c_uint32), ("ba_huber", C.c_float), ("ba_huber_scale", C.c_float),
                ("ba_max_outlier_error", C.c_float), ("ba_steps_per_run", C.c_uint32),
                ("ba_low_connectivity_scale", C.c_float), ("ba_upper_connections", C.c_uint32),
                ("min_lambda", C.c_float), ("ba_free_keyframes", C.c_uint32),
                ("covis_min_threshold", C.c_uint32), ("covis_ba_step", C.c_uint32),
                ("ba_lower_connections", C.c_uint32), ("covis_max_steps", C.c_uint32),
                ("map_point_depth_noise", C.c_float)]


class NewPointsSettingsC(C.Structure):
    """mage_new_points_settings (include/mage_hot.h); struct_size is filled in by make()."""
    _fields_ = [("struct_size", C.c_uint32), ("max_epipolar_error", C.c_float),
                ("min_accepted_distance_ratio", C.c_float), ("min_parallax_degrees", C.c_float),
                ("pyramid_scale", C.c_float), ("num_levels", C.c_uint32), ("grid_width", C.c_uint32),
                ("grid_height", C.c_uint32), ("max_grid_count", C.c_uint32), ("image_width", C.c_uint32),
                ("image_height", C.c_uint32)]

    @classmethod
    def make(cls, **kw):
        return cls(struct_size=C.sizeof(cls), **kw)


class NewPointsAssocSettingsC(C.Structure):
    """mage_new_points_assoc_settings (include/mage_hot.h); struct_size is filled in by make()."""
    _fields_ = [("struct_size", C.c_uint32), ("search_radius", C.c_float), ("max_keyframe_angle_degrees", C.c_float),
                ("image_border", C.c_float), ("max_hamming_distance", C.c_int32), ("min_hamming_difference", C.c_int32)]

    @classmethod
    def make(cls, **kw):
        return cls(struct_size=C.sizeof(cls), **kw)


class StereoInitSettingsC(C.Structure):
    """mage_stereo_init_settings (include/mage_hot.h); struct_size is filled in by make()."""
    _fields_ = [("struct_size", C.c_uint32), ("min_init_map_points", C.c_uint32), ("min_feature_matches", C.c_uint32),
                ("max_outlier_error", C.c_float), ("max_epipolar_error", C.c_float),
                ("min_accepted_distance_ratio", C.c_float), ("initialization_tether_strength", C.c_float),
                ("max_pose_contribution_z", C.c_float), ("amount_ba_can_change_pose", C.c_float),
                ("max_depth_meters", C.c_float), ("max_hamming_distance", C.c_int32),
                ("min_hamming_difference", C.c_int32), ("ba_num_steps", C.c_uint32),
                ("ba_num_steps_per_run", C.c_uint32), ("ba_min_steps", C.c_uint32), ("ba_huber_width", C.c_float),
                ("ba_huber_width_scale", C.c_float), ("ba_max_outlier_error", C.c_float),
                ("ba_max_outlier_error_scale_factor", C.c_float), ("ba_min_mean_square_error", C.c_float),
                ("ba_distance_tether_weight", C.c_float), ("ba_low_connectivity_iterations_scale", C.c_float)]

    @classmethod
    def make(cls, **kw):
        return cls(struct_size=C.sizeof(cls), **kw)


class MonoInitSettingsC(C.Structure):
    """mage_mono_init_settings (include/mage_hot.h); struct_size is filled in by make()."""
    _fields_ = [("struct_size", C.c_uint32), ("fundamental_transfer_error_threshold", C.c_float),
                ("min_feature_matches", C.c_uint32), ("min_scoring_inliers", C.c_uint32),
                ("min_inlier_percentage", C.c_float), ("min_initial_map_points", C.c_uint32),
                ("min_map_points", C.c_uint32), ("min_third_frame_match_percentage", C.c_float),
                ("feature_covisibility_threshold", C.c_float), ("max_parallax_3d_distance", C.c_float),
                ("max_parallax_3d_median_distance", C.c_float), ("min_candidate_pose_disimilarity", C.c_float),
                ("max_pose_contribution_z", C.c_float), ("bundle_adjustment_g2o_steps", C.c_uint32),
                ("bundle_adjustment_huber_width", C.c_float), ("ransac_iterations_for_models", C.c_uint32),
                ("max_epipolar_error", C.c_float), ("max_outlier_error", C.c_float),
                ("amount_ba_can_change_pose", C.c_float),
                ("map_initialization_new_points_creation_min_distance", C.c_float),
                ("map_init_frame_interval_milliseconds", C.c_uint32),
                ("min_initialization_interval_milliseconds", C.c_uint32),
                ("max_initialization_interval_milliseconds", C.c_uint32), ("min_pixel_spread", C.c_float),
                ("final_ba_huber_width", C.c_float), ("final_ba_max_outlier_error", C.c_float),
                ("final_ba_max_outlier_error_scale_factor", C.c_float), ("final_ba_min_mean_square_error", C.c_float),
                ("final_ba_num_steps_per_run", C.c_uint32), ("final_ba_num_steps", C.c_uint32),
                ("extra_frame_max_outlier_error", C.c_float), ("extra_frame_bundle_adjustment_steps", C.c_uint32),
                ("extra_frame_huber_width", C.c_float), ("extra_frame_search_radius", C.c_float),
                ("five_point_max_hamming_distance", C.c_int32), ("five_point_min_hamming_difference", C.c_int32),
                ("extra_frame_max_hamming_distance", C.c_int32), ("extra_frame_min_hamming_difference", C.c_int32)]

    @classmethod
    def make(cls, **kw):
        return cls(struct_size=C.sizeof(cls), **kw)


class RelocSettingsC(C.Structure):
    """mage_reloc_settings (include/mage_hot.h); struct_size is filled in by make()."""
    _fields_ = [("struct_size", C.c_uint32), ("min_brute_force_correspondences", C.c_uint32),
                ("min_radius_match_correspondences", C.c_uint32), ("min_map_points", C.c_uint32),
                ("ransac_inliers_pct_required", C.c_float), ("bundle_adjust_inliers_pct_required", C.c_float),
                ("ransac_confidence", C.c_float), ("round_robin_iterations", C.c_uint32),
                ("ransac_iterations", C.c_uint32), ("bundle_adjust_iterations", C.c_uint32),
                ("search_radius", C.c_float), ("max_bundle_adjust_reprojection_error", C.c_float),
                ("max_bundle_pnp_reprojection_error", C.c_float), ("max_hamming_distance", C.c_int32),
                ("min_hamming_difference", C.c_int32)]

    @classmethod
    def make(cls, **kw):
        return cls(struct_size=C.sizeof(cls), **kw)


class BoundingDepthSettingsC(C.Structure):
    """mage_bounding_depth_settings (include/mage_hot.h); struct_size is filled in by make()."""
    _fields_ = [("struct_size", C.c_uint32), ("region_of_interest_min_x", C.c_float),
                ("region_of_interest_min_y", C.c_float), ("region_of_interest_max_x", C.c_float),
                ("region_of_interest_max_y", C.c_float), ("near_depth_softness", C.c_float),
                ("far_depth_softness", C.c_float)]

    @classmethod
    def make(cls, **kw):
        return cls(struct_size=C.sizeof(cls), **kw)


class VoiSettingsC(C.Structure):
    """mage_voi_settings (include/mage_hot.h); struct_size is filled in by make(), the derived constants by
    mage_voi_settings_prepare."""
    _fields_ = [("struct_size", C.c_uint32), ("threshold", C.c_float), ("iterations", C.c_int32),
                ("voxel_count_floor", C.c_int32), ("away_prominence", C.c_float), ("toward_prominence", C.c_float),
                ("side_prominence", C.c_float), ("kernel_angle_x_rads", C.c_float), ("kernel_angle_y_rads", C.c_float),
                ("kernel_pitch_rads", C.c_float), ("kernel_roll_rads", C.c_float), ("kernel_yaw_rads", C.c_float),
                ("kernel_depth_modifier", C.c_float), ("kernel_rotation", C.c_float * 9), ("tan_min_angle", C.c_float),
                ("tan_half_angle_x", C.c_float), ("tan_half_angle_y", C.c_float)]

    @classmethod
    def make(cls, **kw):
        return cls(struct_size=C.sizeof(cls), **kw)


class LoopClosureSettingsC(C.Structure):
    """mage_loop_closure_settings (include/mage_hot.h); struct_size is filled in by make()."""
    _fields_ = [("struct_size", C.c_uint32), ("max_map_points", C.c_uint32), ("min_keyframes", C.c_uint32),
                ("search_radius", C.c_float), ("min_view_degrees", C.c_float), ("image_border", C.c_float),
                ("width", C.c_uint32), ("height", C.c_uint32), ("num_levels", C.c_uint32), ("pyramid_scale", C.c_float),
                ("closure_max_hamming_distance", C.c_int32), ("closure_min_hamming_difference", C.c_int32),
                ("connect_max_hamming_distance", C.c_int32), ("connect_min_hamming_difference", C.c_int32)]

    @classmethod
    def make(cls, **kw):
        return cls(struct_size=C.sizeof(cls), **kw)


class _PointerArgs(C.Structure):
    """An argument block whose _POINTERS fields take anything ptr() takes; struct_size is filled in
    by make()."""
    _POINTERS = ()

    @classmethod
    def make(cls, **kw):
        for name in cls._POINTERS:
            if name in kw:
                kw[name] = ptr(kw[name])
        return cls(struct_size=C.sizeof(cls), **kw)


class LoopClosureProblemC(_PointerArgs):
    """mage_loop_closure_problem (include/mage_hot.h)."""
    _POINTERS = ("state", "obs", "ki_pos3", "ki_r9", "ki_intr4", "ki_kp", "ki_desc", "ki_point", "kf_id", "kf_pos3",
                 "kf_r9", "kf_intr4", "kf_kp", "kf_desc", "kf_point", "kf_start", "kf_mask", "sample_index", "closure",
                 "closure_verdict", "connect", "connect_verdict", "ki_mask", "kf_modified", "counts", "status")
    _fields_ = ([("struct_size", C.c_uint32), ("n_map", C.c_uint32), ("state", C.c_void_p), ("obs", C.c_void_p),
                 ("obs_pitch", C.c_int64), ("offset", C.c_uint32), ("n_keyframes", C.c_uint32), ("ki_id", C.c_int32),
                 ("n_ki", C.c_uint32)] + [(n, C.c_void_p) for n in _POINTERS[2:8]] +
                [("n_kf", C.c_uint32), ("reserved", C.c_uint32)] + [(n, C.c_void_p) for n in _POINTERS[8:]])


class LoopClosureBatchC(_PointerArgs):
    """mage_loop_closure_batch (include/mage_hot.h)."""
    _POINTERS = ("d_n_map", "d_state", "d_obs", "d_offset", "d_n_keyframes", "d_ki_id", "d_n_ki", "d_ki_pos3", "d_ki_r9",
                 "d_ki_intr4", "d_ki_kp", "d_ki_desc", "d_ki_point", "d_n_kf", "d_kf_id", "d_kf_pos3", "d_kf_r9",
                 "d_kf_intr4", "d_kf_kp", "d_kf_desc", "d_kf_point", "d_n_kf_kp", "d_kf_mask", "d_sample_index",
                 "d_closure", "d_closure_verdict", "d_connect", "d_connect_verdict", "d_ki_mask", "d_kf_modified",
                 "d_counts", "d_status")
    _fields_ = ([("struct_size", C.c_uint32), ("problems", C.c_uint32), ("kf_slots", C.c_uint32), ("reserved", C.c_uint32),
                 ("map_pitch", C.c_int64), ("obs_pitch", C.c_int64), ("ki_pitch", C.c_int64), ("kf_pitch", C.c_int64)] +
                [(n, C.c_void_p) for n in _POINTERS])


class StereoMapInitResultC(C.Structure):
    """mage_stereo_map_init_result (include/mage_hot.h)."""
    _fields_ = [("code", C.c_int32), ("crop", C.c_int32 * 4), ("n_masked", C.c_uint32), ("n_matches", C.c_uint32),
                ("n_verdicts", C.c_uint32), ("frame1_pos3", C.c_float * 3), ("frame1_r9", C.c_float * 9),
                ("n_points", C.c_uint32), ("n_ba_outliers", C.c_uint32), ("ba_runs", C.c_uint32)]


class BAStats(C.Structure):
    _fields_ = [("iterations", C.c_uint64), ("trials", C.c_uint64), ("rejected_trials", C.c_uint64),
                ("last_chi2", C.c_double), ("lambda_", C.c_double)]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DM_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"),
                     ("distance", "<f4")])
# mage_new_point (48 B)
NP_DTYPE = np.dtype([("position", "<f4", 3), ("mean_view_dir", "<f4", 3), ("d_min", "<f4"), ("d_max", "<f4"),
                     ("ki_index", "<u4"), ("kc_slot", "<u4"), ("kc_index", "<u4"), ("match_index", "<u4")])

# mage_stereo_point (28 B)
SP_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4"), ("position", "<f4", 3),
                     ("near_parallel", "<u4")])

# mage_mono_init_result (408 B)
MI_RESULT_DTYPE = np.dtype([("verdict", "<u4"), ("status", "<u4"), ("n_matches", "<u4"), ("n_points", "<u4"),
                            ("win_iteration", "<i4"), ("win_root", "<i4"), ("win_indices", "<i4", 5),
                            ("win_score", "<f4"), ("selected_pose", "<i4"), ("next_best_score", "<f4"),
                            ("pos3", "<f4", 6), ("r9", "<f4", 18), ("cand_pos3", "<f4", 12), ("cand_r9", "<f4", 36),
                            ("cand_score", "<f4", 4), ("cand_median", "<f4", 4), ("cand_count", "<u4", 4),
                            ("cand_flags", "<u4", 4)])

# mage_mono_init_third_result (128 B)
M3_RESULT_DTYPE = np.dtype([("verdict", "<u4"), ("status", "<u4"), ("n_points", "<u4"), ("n_behind", "<u4"),
                            ("n_matched", "<u4"), ("n_outliers", "<u4"), ("n_associated", "<u4"), ("mean_sq", "<f4"),
                            ("pos3", "<f4", 3), ("r9", "<f4", 9), ("opt_pos3", "<f4", 3), ("opt_r9", "<f4", 9)])

# mage_reloc_pnp_result (104 B)
RP_RESULT_DTYPE = np.dtype([("verdict", "<u4"), ("status", "<u4"), ("n_matches", "<u4"), ("n_inliers", "<u4"),
                            ("n_in_front", "<u4"), ("n_kept", "<u4"), ("win_iteration", "<i4"),
                            ("win_indices", "<i4", 5), ("iterations", "<u4"), ("iterations_run", "<u4"),
                            ("pos3", "<f4", 3), ("r9", "<f4", 9)])

# mage_reloc_guided_result (124 B)
RG_RESULT_DTYPE = np.dtype([("verdict", "<u4"), ("status", "<u4"), ("n_assoc", "<u4"), ("n_queries", "<u4"),
                            ("n_radius_matches", "<u4"), ("n_in_front", "<u4"), ("n_outliers", "<u4"),
                            ("pos3_first", "<f4", 3), ("r9_first", "<f4", 9), ("pos3", "<f4", 3), ("r9", "<f4", 9)])

# mage_reloc_frame_result (56 B)
RG_FRAME_DTYPE = np.dtype([("index", "<i4"), ("n_assoc", "<u4"), ("pos3", "<f4", 3), ("r9", "<f4", 9)])

# mage_projected_point (16 B) and mage_depth_result (20 B)
PP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("depth", "<f4"), ("id", "<i4")])
BD_RESULT_DTYPE = np.dtype([("near", "<f4"), ("far", "<f4"), ("n_valid", "<u4"), ("n_points", "<u4"), ("status", "<u4")])

# mage_voi_result (32 B) and mage_voi_level (60 B)
VOI_RESULT_DTYPE = np.dtype([("min", "<f4", 3), ("max", "<f4", 3), ("status", "<u4"), ("levels_done", "<u4")])
VOI_LEVEL_DTYPE = np.dtype([("side", "<f4"), ("dims", "<i4", 3), ("voxel_min", "<f4"), ("voxel_max", "<f4"),
                            ("threshold", "<f4"), ("box_min", "<f4", 3), ("box_max", "<f4", 3), ("n_voxels", "<u4"),
                            ("n_centroids", "<u4")])


class RelocGuidedArgsC(C.Structure):
    """mage_reloc_guided_args (include/mage_hot.h); struct_size is filled in by make(), pointers are
    given as anything ptr() takes."""
    _POINTERS = ("d_n_candidates", "d_intr4", "d_ba_intr4", "d_map_xyzi", "d_kf_kp", "d_kf_desc", "d_n_kf", "d_order",
                 "d_n_order", "d_kp", "d_desc", "d_n_kp", "d_pnp_result", "d_obs_start", "d_points3", "d_uv", "d_info",
                 "d_pos3", "d_r9", "d_query_kp", "d_query_pos", "d_query_desc", "d_query_ref", "d_n_queries",
                 "d_radius_matches", "d_n_radius", "d_assoc", "d_ba_obs_start", "d_ba_points3", "d_ba_uv", "d_ba_info",
                 "d_ba_outlier", "d_result", "d_frame_result", "d_qt7_first", "d_qt7", "d_scratch")
    _fields_ = ([("struct_size", C.c_uint32), ("frames", C.c_uint32), ("candidates_per_frame", C.c_uint32),
                 ("cap", C.c_uint32), ("pnp_cap", C.c_uint32), ("pose_max_hamming_distance", C.c_int32),
                 ("pose_min_hamming_difference", C.c_int32), ("kf_pitch", C.c_int64), ("kp_pitch", C.c_int64)] +
                [(name, C.c_void_p) for name in _POINTERS])

    @classmethod
    def make(cls, **kw):
        for name in cls._POINTERS:
            if name in kw:
                kw[name] = ptr(kw[name])
        return cls(struct_size=C.sizeof(cls), **kw)


class RelocCandidatesArgsC(C.Structure):
    """mage_reloc_candidates_args (include/mage_hot.h); as RelocGuidedArgsC."""
    _POINTERS = ("d_leaf_kf", "d_leaf", "d_mask_kf", "d_matches", "d_n_matches", "d_match_status", "d_pnp_result",
                 "d_inlier_idx", "d_obs_start", "d_points3", "d_uv", "d_info", "d_pos3", "d_r9", "d_pnp_scratch")
    _fields_ = [("struct_size", C.c_uint32), ("match_cap", C.c_uint32)] + [(name, C.c_void_p) for name in _POINTERS]

    @classmethod
    def make(cls, **kw):
        for name in cls._POINTERS:
            if name in kw:
                kw[name] = ptr(kw[name])
        return cls(struct_size=C.sizeof(cls), **kw)


# mage_new_point_assoc (16 B)
NA_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("keypoint", "<i4")])

# mage_map_point_obs (64 B), mage_map_point_state (40 B), mage_loop_closure_assoc (16 B)
MP_OBS_DTYPE = np.dtype([("desc", "u1", 32), ("centre", "<f4", 3), ("octave", "<i4"), ("keyframe_id", "<i4"),
                         ("reserved", "<u4", 3)])
MP_STATE_DTYPE = np.dtype([("pos", "<f4", 3), ("mvd", "<f4", 3), ("dmin", "<f4"), ("dmax", "<f4"), ("rep", "<i4"),
                           ("n_obs", "<i4")])
LC_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("keypoint", "<i4")])

_lib = None


def load() -> C.CDLL:
    """Load libmage_hot.so (raises ImportError if it has not been built)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m mageslam_amd.build`")
        lib = C.CDLL(str(LIB_PATH))
        _declare(lib)
        _lib = lib
    return _lib


def ptr(a):
    """Host pointer of a numpy array, or raw device pointer of a torch tensor / int."""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def check(status: int) -> None:
    if status != MAGE_OK:
        msg = load().mage_last_error().decode(errors="replace")
        raise MageError(status, msg)


def profile_report() -> dict:
    """{kernel: (launches, total_ms)} from the library's event timers."""
    out = {}
    for line in load().mage_profile_report().decode().splitlines():
        name, cnt, ms = line.split()
        out[name] = (int(cnt), float(ms))
    return out


def _declare(L: C.CDLL) -> None:
    vp, i32, u32, f32, i64, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float, C.c_int64, C.c_uint64
    st = C.c_int

    def sig(name, res, *args):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = list(args)

    sig("mage_version", C.c_char_p)
    sig("mage_last_error", C.c_char_p)
    sig("mage_pool_trim", C.c_uint64, i32)
    sig("mage_profile_enable", None, i32)
    sig("mage_profile_filter", None, C.c_char_p)
    sig("mage_profile_reset", None)
    sig("mage_profile_report", C.c_char_p)
    sig("mage_orb_create", st, vp, C.c_int, C.POINTER(vp))
    sig("mage_orb_destroy", st, vp)
    sig("mage_orb_detect_and_compute", st, vp, vp, i32, i32, i32, vp, vp, u32, C.POINTER(u32))
    sig("mage_orb_detect_and_compute_batch_device", st, vp, vp, u32, i32, i32, i32, i64, vp, vp, u32, vp, vp)
    sig("mage_orb_status", st, vp, vp)
    sig("mage_orb_reset_status", st, vp, vp)
    sig("mage_orb_set_fast_gate", st, vp, u32, i32, vp)
    sig("mage_orb_fast_gate_stats", st, vp, u32, C.POINTER(i32), C.POINTER(i32), C.POINTER(u32), vp)
    sig("mage_synth_frames_device", st, vp, u32, i32, i32, i64, u32, u64, vp)
    f64 = C.c_double
    sig("mage_synth_scene_device", st, vp, u32, i32, i32, i64, vp, f64, f64, f64, f64, f64, f64, i64, u64, vp)
    sig("mage_orb_fast_score_map", st, vp, i32, i32, i32, i32, vp, C.c_int)
    sig("mage_debug_fast_tile_plan", st, vp, i32, i32, i32, i32, i32, vp, vp, vp)
    sig("mage_undistort_keypoints", st, vp, vp, vp, u32, C.c_int)
    sig("mage_undistort_keypoints_batch_device", st, vp, vp, vp, i64, vp, u32, vp)
    sig("mage_undistorter_create", st, vp, i32, i32, C.c_int, C.POINTER(vp), vp)
    sig("mage_undistorter_destroy", st, vp)
    sig("mage_undistorter_get_maps", st, vp, vp, vp)
    sig("mage_undistort_image", st, vp, vp, i32, vp, i32)
    sig("mage_undistort_image_batch_device", st, vp, vp, i32, i64, vp, i32, i64, u32, vp)
    sig("mage_resize_linear_device", st, vp, i32, i32, i32, vp, i32, i32, i32, vp)
    sig("mage_scale_for_camera_configuration", st, vp, vp, f32, vp, C.POINTER(f32), vp, C.POINTER(i32))
    sig("mage_scale_image_for_camera_configuration_device", st, vp, vp, f32, vp, i32, vp, i32, i64, vp,
        C.POINTER(f32), C.POINTER(i32), vp)
    sig("mage_hamming_distance", i32, vp, vp)
    sig("mage_hamming_match", st, vp, u32, vp, vp, u32, vp, i32, i32, vp, u32, C.POINTER(u32))
    sig("mage_hamming_match_batch_device", st, vp, i64, vp, vp, i64, vp, u32, i32, i32, vp, u32, vp, vp)
    sig("mage_radius_match", st, vp, vp, vp, vp, u32, vp, vp, vp, u32, C.c_float, i32, i32, vp, u32, C.POINTER(u32))
    sig("mage_radius_match_batch_device", st, vp, vp, vp, i64, vp, vp, vp, i64, vp, u32, C.c_float, i32, i32, vp,
        vp, u32, vp, vp, vp)
    sig("mage_local_map_match", st, vp, vp, vp, vp, u32, vp, vp, u32, vp, C.c_float, i32, i32, vp, C.c_int)
    sig("mage_bow_create", st, vp, vp, vp, u32, C.c_int, C.POINTER(vp))
    sig("mage_bow_destroy", st, vp)
    sig("mage_bow_train", st, vp, u32, u32, u32, u32, C.c_int, C.POINTER(vp))
    sig("mage_bow_train_kmedoid", st, vp, u32, u32, u32, u32, C.c_int, C.POINTER(vp))
    sig("mage_bow_get_tree", st, vp, vp, vp, vp, u32, C.POINTER(u32))
    sig("mage_bow_find_leaves", st, vp, vp, u32, vp)
    sig("mage_bow_find_leaves_device", st, vp, vp, u32, vp, vp)
    sig("mage_indexed_match", st, vp, vp, u32, vp, vp, u32, vp, i32, i32, vp, u32, C.POINTER(u32))
    sig("mage_indexed_match_batch_device", st, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, u32, i32, i32, vp, u32,
        vp, vp, vp)
    sig("mage_ba_create", st, i32, C.c_int, C.POINTER(vp))
    sig("mage_ba_destroy", st, vp)
    sig("mage_ba_set_cameras", st, vp, u32, vp, vp, vp, vp)
    sig("mage_ba_fix_camera", st, vp, u32, i32)
    sig("mage_ba_set_points", st, vp, u32, vp)
    sig("mage_ba_set_observations", st, vp, u32, vp, vp, vp, vp)
    sig("mage_ba_set_lambda", st, vp, f32)
    sig("mage_ba_get_lambda", st, vp, C.POINTER(f32))
    sig("mage_ba_set_tethers", st, vp, u32, u32, vp, vp, vp, vp)
    sig("mage_ba_step", st, vp, vp, u32, f32, vp, u32, C.POINTER(u32), C.POINTER(f32))
    sig("mage_ba_get_poses", st, vp, vp, vp)
    sig("mage_ba_get_points", st, vp, vp)
    sig("mage_ba_get_state_f64", st, vp, vp, vp)
    sig("mage_ba_get_stats", st, vp, C.POINTER(BAStats))
    sig("mage_track_sequence", st, vp, vp, vp, u32, vp, vp, C.c_double, vp, vp, vp, vp, vp, C.c_int)
    sig("mage_track_sequence_device", st, vp, vp, u32, vp, u32, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp)
    sig("mage_ba_pose_batch", st, u32, vp, vp, vp, vp, vp, vp, vp, u32, f32, f32, vp, vp, vp, vp, vp, vp, C.c_int)
    sig("mage_ba_pose_batch_device", st, u32, vp, vp, vp, vp, vp, vp, vp, u32, f32, f32, vp, vp, vp, vp, vp, vp, vp)
    sig("mage_new_map_points", st, vp, vp, vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp,
        C.c_int)
    sig("mage_new_map_points_host", st, vp, vp, vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp,
        vp)
    sig("mage_new_map_points_batch_device", st, vp, u32, u32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp,
        vp, u32, vp, vp, u32, vp, vp, vp, vp)
    sig("mage_new_points_associate", st, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
        C.c_int)
    sig("mage_new_points_associate_host", st, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
        vp)
    sig("mage_new_points_associate_batch_device", st, vp, vp, u32, u32, vp, u32, vp, vp, i64, vp, vp, vp, vp, vp, vp,
        vp, vp, i64, vp, vp, vp, vp, vp, vp)
    sig("mage_stereo_init_triangulate_batch_device", st, vp, u32, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp,
        vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("mage_stereo_init_triangulate_host", st, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp, u32,
        vp, vp, vp, vp, vp, vp, vp)
    sig("mage_stereo_init_triangulate", st, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp,
        u32, vp, vp, vp, vp, vp, vp, vp, C.c_int)
    sig("mage_mono_init_trace_bytes", u64, u32)
    sig("mage_mono_init_scratch_bytes", u64, u32, u32, i64, i64, i32, i32)
    sig("mage_mono_init_two_view_batch_device", st, vp, u32, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, u32, vp, vp, vp,
        u32, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("mage_mono_init_two_view", st, vp, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp,
        vp, C.c_int)
    sig("mage_mono_init_two_view_host", st, vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp)
    sig("mage_mono_init_third_scratch_bytes", u64, u32, u32, vp)
    sig("mage_mono_init_third_frame_batch_device", st, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, i64, vp, vp, i64,
        vp, vp, vp, i64, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("mage_mono_init_third_frame", st, vp, vp, vp, vp, vp, u32, vp, vp, vp, u32, vp, u32, vp, vp, u32, u32, vp, vp,
        vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int)
    sig("mage_mono_init_third_frame_host", st, vp, vp, vp, vp, vp, u32, vp, vp, vp, u32, vp, u32, vp, vp, u32, u32, vp,
        vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("mage_reloc_pnp_trace_bytes", u64, u32)
    sig("mage_reloc_pnp_scratch_bytes", u64, u32, u32, u32, i32)
    sig("mage_reloc_pnp_batch_device", st, vp, u32, vp, vp, i64, vp, i64, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp,
        vp, vp, vp, vp, vp)
    sig("mage_reloc_pnp", st, vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, vp, C.c_int)
    sig("mage_reloc_pnp_host", st, vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, vp)
    sig("mage_debug_reloc_pnp_update", st, f64, u32, u32, vp)
    sig("mage_debug_reloc_pnp_loop", st, vp, vp, u32, u32, f64, i32, vp)
    sig("mage_reloc_guided_scratch_bytes", u64, u32, u32, u32)
    sig("mage_reloc_guided_batch_device", st, vp, vp, vp)
    sig("mage_reloc_guided", st, vp, i32, i32, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, u32, vp, u32,
        vp, vp, vp, vp, C.c_int)
    sig("mage_reloc_guided_host", st, vp, i32, vp, vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp,
        vp, u32, vp, vp, vp, vp, vp, vp, vp)
    sig("mage_reloc_guided_choose_host", st, vp, vp, u32, vp)
    sig("mage_reloc_candidates_batch_device", st, vp, vp, vp, vp)
    sig("mage_bounding_plane_depths_host", st, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, u32, u32, vp, vp)
    sig("mage_bounding_plane_depths", st, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, u32, u32, vp, vp, C.c_int)
    sig("mage_bounding_plane_depths_batch_device", st, vp, u32, vp, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, u32, vp, vp,
        vp)
    sig("mage_voi_settings_prepare", st, vp)
    sig("mage_voi_teardrop_host", st, vp, vp, vp, u32, vp, u32, vp)
    sig("mage_volume_of_interest_host", st, vp, vp, vp, vp, u32, vp, u32, vp, vp)
    sig("mage_volume_of_interest", st, vp, vp, vp, vp, u32, vp, u32, vp, vp, C.c_int)
    sig("mage_volume_of_interest_scratch_bytes", u64, u32, u32)
    sig("mage_volume_of_interest_batch_device", st, vp, u32, vp, i64, vp, vp, vp, u32, vp, vp, vp, vp, vp)
    sig("mage_map_points_refresh_host", st, vp, u32, vp, vp, i64, vp, vp)
    sig("mage_map_points_refresh", st, vp, u32, vp, vp, i64, vp, vp, C.c_int)
    sig("mage_map_points_refresh_batch_device", st, vp, u32, vp, vp, i64, vp, vp, vp, vp)
    sig("mage_cheap_loop_closure_host", st, vp, vp)
    sig("mage_cheap_loop_closure", st, vp, vp, C.c_int)
    sig("mage_cheap_loop_closure_batch_device", st, vp, vp, vp)
    sig("mage_overlap_crop_source_in_target", st, vp, vp, vp, f32, vp)
    sig("mage_stereo_map_init", st, vp, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, C.c_int)
    sig("mage_debug_stereo_init_host", st, vp, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp)
