"""ctypes binding of the gfx950 backend's C-ABI (include/rebvio_hip.h).

Plumbing only: this module loads `rebvio_amd/_build/librebvio_hip.so` and forwards calls. There is no CPU
fallback anywhere: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# REBVIO_HIP_LIB: another build of the same library (A/B measurements of compile-time variants); default = the in-tree build
LIB_PATH = os.environ.get("REBVIO_HIP_LIB") or os.path.join(_HERE, "_build", "librebvio_hip.so")

KEYLINE_DTYPE = np.dtype([
    ("pos", "<f4", (2,)), ("pos_img", "<f4", (2,)), ("match_pos_img", "<f4", (2,)), ("gradient", "<f4", (2,)),
    ("match_gradient", "<f4", (2,)), ("gradient_norm", "<f4"), ("match_gradient_norm", "<f4"), ("rho", "<f4"),
    ("sigma_rho", "<f4"), ("id", "<i4"), ("id_prev", "<i4"), ("id_next", "<i4"), ("match_id", "<i4"),
    ("match_id_forward", "<i4"), ("match_id_keyframe", "<i4"), ("matches", "<u4")])
assert KEYLINE_DTYPE.itemsize == 84

# rebvio_hip_cloud_point: one record of a map's point cloud
CLOUD_POINT_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("rho", "<f4"), ("sigma_rho", "<f4"), ("gradient_norm", "<f4"),
                              ("keyline", "<i4"), ("matches", "<u4")])
assert CLOUD_POINT_DTYPE.itemsize == 32

# rebvio_hip_kf_match: one keyframe-to-current correspondence (Map.keyframe_matches)
KF_MATCH_DTYPE = np.dtype([("kf_keyline", "<i4"), ("keyline", "<i4"), ("claimants", "<i4"), ("matches", "<u4"), ("rho", "<f4"),
                           ("sigma_rho", "<f4"), ("pos_img", "<f4", (2,))])
assert KF_MATCH_DTYPE.itemsize == 32

# rebvio_hip_chain_ref: one keyline's place in its edge chain (Map.edge_chains)
CHAIN_REF_DTYPE = np.dtype([("head", "<i4"), ("rank", "<i4"), ("length", "<i4"), ("flags", "<i4")])
assert CHAIN_REF_DTYPE.itemsize == 16

# rebvio_hip_polyline: one line of Map.edge_polylines; bit 0 of flags = closed
POLYLINE_DTYPE = np.dtype([("first_point", "<i4"), ("points", "<i4"), ("head", "<i4"), ("flags", "<i4")])
assert POLYLINE_DTYPE.itemsize == 16

# rebvio_hip_line_segment: one straight segment of Map.edge_segments; flags bit 0 = depth valid, bit 1 = unresolved
LINE_SEGMENT_DTYPE = np.dtype([("xyz0", "<f4", (3,)), ("xyz1", "<f4", (3,)), ("uv0", "<f4", (2,)), ("uv1", "<f4", (2,)), ("rho0", "<f4"),
                               ("rho1", "<f4"), ("sigma_rho0", "<f4"), ("sigma_rho1", "<f4"), ("max_dev2", "<f4"), ("chi2", "<f4"),
                               ("first_point", "<i4"), ("points", "<i4"), ("line", "<i4"), ("flags", "<i4")])
assert LINE_SEGMENT_DTYPE.itemsize == 80


class Params(C.Structure):
    _fields_ = [
        ("rows", C.c_int), ("cols", C.c_int), ("fm", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("keylines_ref", C.c_int), ("keylines_max", C.c_int),
        ("pos_neg_threshold", C.c_float), ("dog_threshold", C.c_float), ("threshold", C.c_float), ("gain", C.c_float),
        ("max_threshold", C.c_float), ("min_threshold", C.c_float),
        ("search_range", C.c_float), ("reweight_distance", C.c_float), ("match_treshold", C.c_float),
        ("min_match_threshold", C.c_uint), ("iterations", C.c_uint), ("global_min_matches_threshold", C.c_uint),
        ("pixel_uncertainty", C.c_float), ("quantile_cutoff", C.c_float), ("quantile_num_bins", C.c_int),
        ("reshape_q_abs", C.c_float),
        ("pixel_uncertainty_match", C.c_float), ("match_threshold_norm", C.c_float), ("match_threshold_angle", C.c_float),
        ("regularization_threshold", C.c_float),
        ("gyro_std_dev", C.c_float), ("gyro_bias_std_dev", C.c_float),
        ("device_id", C.c_int), ("map_pool", C.c_int)]


class PairOut(C.Structure):
    _fields_ = [
        ("Vg", C.c_float * 3), ("P_Vg", C.c_float * 9), ("F", C.c_float), ("Xv", C.c_float * 6), ("W_Xv", C.c_float * 36),
        ("Xgv", C.c_float * 6), ("V", C.c_float * 3), ("R", C.c_float * 9), ("P_V", C.c_float * 9),
        ("sigma_rho_min", C.c_float), ("ext_ok", C.c_int), ("klm_num", C.c_int), ("kf_matches", C.c_int),
        ("reg_num", C.c_int), ("lm_accept_mask", C.c_int), ("status", C.c_int)]


class PairMid(C.Structure):
    _fields_ = [("Vg", C.c_float * 3), ("P_Vg", C.c_float * 9), ("F", C.c_float), ("sigma_rho_min", C.c_float),
                ("lm_accept_mask", C.c_int), ("ext_ok", C.c_int), ("Xv", C.c_float * 6), ("W_Xv", C.c_float * 36),
                ("Xgv", C.c_float * 6), ("W_Xgv", C.c_float * 36), ("R", C.c_float * 9)]


class CloudFilter(C.Structure):
    _fields_ = [("min_matches", C.c_uint), ("max_rel_sigma", C.c_float), ("rho_min", C.c_float), ("rho_max", C.c_float)]


class CloudPose(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("scale", C.c_float)]


class PolylineOpts(C.Structure):
    """rebvio_hip_polyline_opts (Map.edge_polylines); defaults from default_polyline_opts"""
    _fields_ = [("filter", CloudFilter), ("min_chain_length", C.c_int), ("reserved", C.c_int)]


class SegmentOpts(C.Structure):
    """rebvio_hip_segment_opts (Map.edge_segments); defaults from default_segment_opts"""
    _fields_ = [("poly", PolylineOpts), ("tol", C.c_float), ("min_length", C.c_float), ("min_points", C.c_int), ("max_rounds", C.c_int)]


class SegmentCounts(C.Structure):
    """rebvio_hip_segment_counts: what Map.edge_segments found, whatever the cap let through"""
    _fields_ = [("segments_all", C.c_int), ("kept", C.c_int), ("depth_valid", C.c_int), ("unresolved", C.c_int),
                ("rounds_used", C.c_int), ("points", C.c_int), ("lines", C.c_int), ("reserved", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KfMatch(C.Structure):
    _fields_ = [("kf_keyline", C.c_int), ("keyline", C.c_int), ("claimants", C.c_int), ("matches", C.c_uint), ("rho", C.c_float),
                ("sigma_rho", C.c_float), ("pos_img", C.c_float * 2)]


class KfPoseOpts(C.Structure):
    """rebvio_hip_kf_pose_opts (Map.keyframe_pose); defaults from default_kf_pose_opts"""
    _fields_ = [("kf_filter", CloudFilter), ("huber_px", C.c_double), ("max_iter", C.c_int), ("min_used", C.c_int)]


class KfAlignOpts(C.Structure):
    """rebvio_hip_kf_align_opts (Map.keyframe_align); defaults from default_kf_align_opts"""
    _fields_ = [("kf_filter", CloudFilter), ("huber_px", C.c_double), ("min_cos", C.c_double), ("max_dist", C.c_int),
                ("max_iter", C.c_int), ("min_used", C.c_int)]


class KfFuseOpts(C.Structure):
    """rebvio_hip_kf_fuse_opts (KfSnapshot.fuse_depth); defaults from default_kf_fuse_opts"""
    _fields_ = [("kf_filter", CloudFilter), ("min_cos", C.c_double), ("pixel_sigma", C.c_double), ("gate_sigma", C.c_double),
                ("q_abs", C.c_double), ("max_dist", C.c_int), ("reserved", C.c_int)]


class KfFuse(C.Structure):
    """rebvio_hip_kf_fuse: the counts of one depth fusion; associated = fused + gated + flat"""
    _fields_ = [("candidates", C.c_int), ("associated", C.c_int), ("fused", C.c_int), ("gated", C.c_int), ("flat", C.c_int),
                ("clamped", C.c_int)]


DEPTH_U16, DEPTH_F32 = 0, 1  # REBVIO_HIP_DEPTH_*: uint16 counts of `unit` metres (0 = invalid) | float32 metres


class DepthPriorOpts(C.Structure):
    """rebvio_hip_depth_prior_opts (Map.fuse_depth_image); defaults from default_depth_prior_opts"""
    _fields_ = [("tap_px", C.c_double), ("jump_rel", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double),
                ("sigma_z0", C.c_double), ("sigma_z2", C.c_double), ("gate_sigma", C.c_double), ("q_abs", C.c_double),
                ("unit", C.c_double), ("reserved", C.c_int)]


class DepthPriorCounts(C.Structure):
    """rebvio_hip_depth_prior_counts: the counts of one depth-image fusion; sampled = fused + gated"""
    _fields_ = [("candidates", C.c_int), ("sampled", C.c_int), ("fused", C.c_int), ("gated", C.c_int), ("jumps", C.c_int),
                ("clamped", C.c_int)]

    def as_tuple(self):
        return (self.candidates, self.sampled, self.fused, self.gated, self.jumps, self.clamped)


class StereoPriorOpts(C.Structure):
    """rebvio_hip_stereo_prior_opts (Map.fuse_stereo); defaults from default_stereo_prior_opts, baseline has none"""
    _fields_ = [("baseline", C.c_double), ("d_min", C.c_double), ("d_max", C.c_double), ("min_ux", C.c_double), ("row_tol", C.c_int),
                ("sigma_px", C.c_double), ("gate_sigma", C.c_double), ("ambig_px", C.c_double), ("cos_min", C.c_double),
                ("norm_tol", C.c_double), ("q_abs", C.c_double), ("reserved", C.c_int)]


class StereoPriorCounts(C.Structure):
    """rebvio_hip_stereo_prior_counts: the counts of one stereo fusion"""
    _fields_ = [("candidates", C.c_int), ("usable", C.c_int), ("seen", C.c_int), ("fused", C.c_int), ("gated", C.c_int),
                ("ambiguous", C.c_int), ("clamped", C.c_int), ("reserved", C.c_int)]

    def as_tuple(self):
        return (self.candidates, self.usable, self.seen, self.fused, self.gated, self.ambiguous, self.clamped, self.reserved)


class PlaceMatch(C.Structure):
    """rebvio_hip_place_match: one result record of a place query"""
    _fields_ = [("distance", C.c_uint32), ("index", C.c_int32), ("tag", C.c_uint64)]

    def as_tuple(self):
        return (self.distance, self.index, self.tag)


PLACE_WORDS = 384
PLACE_TOPK_MAX = 16


class KfHandoverOpts(C.Structure):
    """rebvio_hip_kf_handover_opts (KfSnapshot.handover_depth); defaults from default_kf_handover_opts"""
    _fields_ = [("kf_filter", CloudFilter), ("min_cos", C.c_double), ("gate_sigma", C.c_double), ("q_abs", C.c_double),
                ("max_dist", C.c_int), ("reserved", C.c_int)]


class KfHandover(C.Structure):
    """rebvio_hip_kf_handover: the counts of one depth hand-over; claimed = adopted + kept + conflicts"""
    _fields_ = [("candidates", C.c_int), ("associated", C.c_int), ("out_of_range", C.c_int), ("claimed", C.c_int), ("adopted", C.c_int),
                ("kept", C.c_int), ("conflicts", C.c_int)]


class KfPose(C.Structure):
    """rebvio_hip_kf_pose: X_cur = R X_kf + t, the sums at that pose, and the counters"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("H", C.c_double * 36), ("g", C.c_double * 6), ("cost", C.c_double),
                ("candidates", C.c_int), ("used", C.c_int), ("iterations", C.c_int), ("status", C.c_int)]


KF_HYP_MAX = 64  # REBVIO_HIP_KF_HYP_MAX


class KfHypothesis(C.Structure):
    """rebvio_hip_kf_hypothesis: a snapshot's handle and a guess (Map.keyframe_align_many; kf_hypothesis builds one)"""
    _fields_ = [("snap", C.c_void_p), ("R0", C.c_double * 9), ("t0", C.c_double * 3)]


class KfHypResult(C.Structure):
    """rebvio_hip_kf_hyp_result: the pose of one hypothesis and its count of used terms with |e| <= huber_px"""
    _fields_ = [("pose", KfPose), ("inliers", C.c_int), ("reserved", C.c_int)]


# every symbol include/rebvio_hip.h declares: (restype, argtypes)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)
_vp = C.c_void_p
SIGNATURES = {
    "rebvio_hip_abi_version": (C.c_int, []),
    "rebvio_hip_last_error": (C.c_char_p, []),
    "rebvio_hip_default_params": (None, [C.POINTER(Params), C.c_int, C.c_int]),
    "rebvio_hip_create": (C.c_int, [C.POINTER(Params), C.POINTER(_vp)]),
    "rebvio_hip_destroy": (None, [_vp]),
    "rebvio_hip_scale_space": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _fp]),
    "rebvio_hip_detect": (C.c_int, [_vp, _fp, C.c_size_t, C.c_uint64, C.POINTER(_vp)]),
    "rebvio_hip_detect_u8_device": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    "rebvio_hip_detect_u8": (C.c_int, [_vp, _vp, C.c_size_t, C.c_uint64, C.POINTER(_vp)]),
    "rebvio_hip_set_undistort": (C.c_int, [_vp, _fp, _fp]),
    "rebvio_hip_front_end_u8": (C.c_int, [_vp, _vp, _fp]),
    "rebvio_hip_detect_px": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_uint64, C.POINTER(_vp)]),
    "rebvio_hip_detect_px_device": (C.c_int, [_vp, _vp, C.c_int, C.c_uint64, C.POINTER(_vp)]),
    "rebvio_hip_front_end_px": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _fp]),
    "rebvio_hip_set_detection_mask": (C.c_int, [_vp, _vp, C.c_size_t]),
    "rebvio_hip_detect_px_masked_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_uint64, C.POINTER(_vp)]),
    "rebvio_hip_detector_state": (C.c_int, [_vp, _fp, _fp, _ip]),
    "rebvio_hip_map_size": (C.c_int, [_vp]),
    "rebvio_hip_map_threshold": (C.c_float, [_vp]),
    "rebvio_hip_map_ts": (C.c_uint64, [_vp]),
    "rebvio_hip_map_download": (C.c_int, [_vp, _vp, _ip]),
    "rebvio_hip_render_edge_image": (C.c_int, [_vp, _vp, _vp]),
    "rebvio_hip_default_cloud_filter": (None, [C.POINTER(CloudFilter)]),
    "rebvio_hip_map_point_cloud": (C.c_int, [_vp, C.POINTER(CloudFilter), C.POINTER(CloudPose), _vp, C.c_int, _ip]),
    "rebvio_hip_map_point_cloud_async": (C.c_int, [_vp, _vp, C.POINTER(CloudFilter), C.POINTER(CloudPose), C.POINTER(_vp)]),
    "rebvio_hip_cloud_wait": (C.c_int, [_vp, C.POINTER(_vp), _ip, C.POINTER(_vp)]),
    "rebvio_hip_cloud_release": (None, [_vp]),
    "rebvio_hip_map_edge_chains": (C.c_int, [_vp, _vp, C.c_int, _ip, _ip, C.c_int, _ip, _ip]),
    "rebvio_hip_default_polyline_opts": (None, [C.POINTER(PolylineOpts)]),
    "rebvio_hip_map_edge_polylines": (C.c_int, [_vp, C.POINTER(PolylineOpts), C.POINTER(CloudPose), _vp, _ip, C.c_int, _vp, C.c_int, _ip,
                                                _ip]),
    "rebvio_hip_test_edge_chains_host": (C.c_int, [_ip, _ip, C.c_int, _vp, C.c_int, _ip, _ip, C.c_int, _ip, _ip]),
    "rebvio_hip_test_edge_polylines_host": (C.c_int, [C.c_float, _vp, C.c_int, C.POINTER(PolylineOpts), C.POINTER(CloudPose), _vp, _ip,
                                                      C.c_int, _vp, C.c_int, _ip, _ip]),
    "rebvio_hip_default_segment_opts": (None, [C.POINTER(SegmentOpts)]),
    "rebvio_hip_map_edge_segments": (C.c_int, [_vp, C.POINTER(SegmentOpts), C.POINTER(CloudPose), _vp, C.c_int, C.POINTER(SegmentCounts)]),
    "rebvio_hip_test_edge_segments_host": (C.c_int, [C.c_float, _vp, C.c_int, C.POINTER(SegmentOpts), C.POINTER(CloudPose), _vp, C.c_int,
                                                     C.POINTER(SegmentCounts)]),
    "rebvio_hip_map_mark_keyframe": (C.c_int, [_vp, _vp]),
    "rebvio_hip_map_keyframe_matches": (C.c_int, [_vp, C.c_int, C.POINTER(KfMatch), C.c_int, _ip]),
    "rebvio_hip_map_keyframe_snapshot": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "rebvio_hip_kf_snapshot_release": (None, [_vp]),
    "rebvio_hip_kf_snapshot_download": (C.c_int, [_vp, _fp, C.POINTER(C.c_uint), C.c_int, _ip]),
    "rebvio_hip_default_kf_pose_opts": (None, [C.POINTER(KfPoseOpts)]),
    "rebvio_hip_map_keyframe_pose": (C.c_int, [_vp, _vp, C.POINTER(KfPoseOpts), _dp, _dp, C.POINTER(KfPose)]),
    "rebvio_hip_kf_snapshot_add_normals": (C.c_int, [_vp, _vp]),
    "rebvio_hip_kf_snapshot_download_normals": (C.c_int, [_vp, _fp, C.c_int, _ip]),
    "rebvio_hip_default_kf_align_opts": (None, [_vp, C.POINTER(KfAlignOpts)]),
    "rebvio_hip_map_keyframe_align": (C.c_int, [_vp, _vp, C.POINTER(KfAlignOpts), _dp, _dp, C.POINTER(KfPose), _ip]),
    "rebvio_hip_test_kf_align_host": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, _fp, C.POINTER(C.c_uint), _fp,
                                                C.c_int, _fp, _fp, C.c_int, _ip, _ip, C.POINTER(KfAlignOpts), _dp, _dp,
                                                C.POINTER(KfPose), _ip]),
    "rebvio_hip_map_keyframe_align_many": (C.c_int, [_vp, C.POINTER(KfHypothesis), C.c_int, C.POINTER(KfAlignOpts),
                                                     C.POINTER(KfHypResult)]),
    "rebvio_hip_kf_align_best": (C.c_int, [C.POINTER(KfHypResult), C.c_int, C.c_int]),
    "rebvio_hip_kf_hypotheses_around": (C.c_int, [_vp, _dp, _dp, C.c_double, C.c_double, C.POINTER(KfHypothesis)]),
    "rebvio_hip_test_kf_align_many_host": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, _fp, C.POINTER(C.c_uint),
                                                     _fp, C.c_int, _fp, _fp, C.c_int, _ip, _ip, C.POINTER(KfAlignOpts), _dp, _dp, C.c_int,
                                                     C.POINTER(KfHypResult)]),
    "rebvio_hip_default_kf_fuse_opts": (None, [_vp, C.POINTER(KfFuseOpts)]),
    "rebvio_hip_kf_snapshot_fuse_depth": (C.c_int, [_vp, _vp, C.POINTER(KfFuseOpts), _dp, _dp, C.POINTER(KfFuse), _ip]),
    "rebvio_hip_test_kf_fuse_host": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, _fp, C.POINTER(C.c_uint), _fp,
                                               C.c_int, _fp, _fp, C.c_int, _ip, _ip, C.POINTER(KfFuseOpts), _dp, _dp,
                                               C.POINTER(KfFuse), _ip]),
    "rebvio_hip_default_kf_handover_opts": (None, [_vp, C.POINTER(KfHandoverOpts)]),
    "rebvio_hip_kf_snapshot_handover_depth": (C.c_int, [_vp, _vp, _vp, C.POINTER(KfHandoverOpts), _dp, _dp, C.POINTER(KfHandover), _ip]),
    "rebvio_hip_test_kf_handover_host": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, _fp, C.POINTER(C.c_uint), _fp,
                                                   C.c_int, _fp, _fp, C.c_int, _ip, _ip, _fp, C.POINTER(C.c_uint), C.c_int,
                                                   C.POINTER(KfHandoverOpts), _dp, _dp, C.POINTER(KfHandover), _ip]),
    "rebvio_hip_kf_snapshot_point_cloud": (C.c_int, [_vp, C.POINTER(CloudFilter), C.POINTER(CloudPose), _vp, C.c_int, _ip]),
    "rebvio_hip_kf_snapshot_point_cloud_async": (C.c_int, [_vp, C.POINTER(CloudFilter), C.POINTER(CloudPose), C.POINTER(_vp)]),
    "rebvio_hip_test_kf_cloud_host": (C.c_int, [C.c_float, _fp, C.POINTER(C.c_uint), C.c_int, C.POINTER(CloudFilter), C.POINTER(CloudPose),
                                                _vp, C.c_int, _ip]),
    "rebvio_hip_test_kf_pose_host": (C.c_int, [C.c_float, _fp, C.POINTER(C.c_uint), C.c_int, _fp, _fp, C.c_int, C.POINTER(KfMatch),
                                               C.c_int, C.POINTER(KfPoseOpts), _dp, _dp, C.POINTER(KfPose)]),
    "rebvio_hip_map_upload": (C.c_int, [_vp, _vp, C.c_int]),
    "rebvio_hip_map_release": (None, [_vp]),
    "rebvio_hip_build_distance_field": (C.c_int, [_vp, _vp]),
    "rebvio_hip_distance_field": (C.c_int, [_vp, _ip, _ip]),
    "rebvio_hip_map_distance_field": (C.c_int, [_vp, _ip, _ip]),
    "rebvio_hip_search_match": (C.c_int, [_vp, _vp, _vp, _fp, _fp, _fp, C.c_float, _ip]),
    "rebvio_hip_smooth": (C.c_int, [_vp, _fp, _ip, _fp]),
    "rebvio_hip_smooth_n": (C.c_int, [_vp, _fp, _ip, C.c_int, _fp]),
    "rebvio_hip_rotate": (C.c_int, [_vp, _vp, _fp]),
    "rebvio_hip_quantile": (C.c_int, [_vp, _vp, C.c_float, C.c_int, _fp]),
    "rebvio_hip_try_vel": (C.c_int, [_vp, _vp, _fp, C.c_float, _fp, _fp]),
    "rebvio_hip_minimize_vel": (C.c_int, [_vp, _vp, _fp, _fp, _fp, _ip, _fp]),
    "rebvio_hip_forward_match": (C.c_int, [_vp, _vp, _vp]),
    "rebvio_hip_ext_rot_vel": (C.c_int, [_vp, _fp, _fp, _fp, _fp, _ip]),
    "rebvio_hip_directed_match": (C.c_int, [_vp, _vp, _vp, _fp, _fp, _fp, C.c_float, _ip, _ip]),
    "rebvio_hip_regularize": (C.c_int, [_vp, _vp, _ip]),
    "rebvio_hip_update_inverse_depth": (C.c_int, [_vp, _fp]),
    "rebvio_hip_reset_state": (None, [_vp]),
    "rebvio_hip_get_gyro_state": (C.c_int, [_vp, _fp, _fp]),
    "rebvio_hip_set_gyro_state": (C.c_int, [_vp, _fp, _fp]),
    "rebvio_hip_track_pair": (C.c_int, [_vp, _vp, _vp, _fp, C.c_float, C.POINTER(PairOut)]),
    "rebvio_hip_track_pair_begin": (C.c_int, [_vp, _vp, _vp, _fp, C.c_float, C.POINTER(PairMid)]),
    "rebvio_hip_track_pair_finish": (C.c_int, [_vp, _vp, _vp, _fp, _fp, _fp, _fp, _ip, _ip, _ip, _ip]),
    "rebvio_hip_track_pair_finish_async": (C.c_int, [_vp, _vp, _vp, _fp, _fp, _fp, _fp, _fp]),
    "rebvio_hip_track_pair_result": (C.c_int, [_vp, _ip, _ip, _ip, _ip]),
    "rebvio_hip_track_pair_hint_next": (C.c_int, [_vp, _vp]),
    "rebvio_hip_push_frame_u8_device": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_push_frame_u8": (C.c_int, [_vp, _vp, C.c_size_t, C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_push_frame_px": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_push_frame_px_device": (C.c_int, [_vp, _vp, C.c_int, C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_push_frame_px_masked_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_push_frame_px_gyro_device": (C.c_int, [_vp, _vp, C.c_int, _vp, _fp, C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_push_frame_px_gyro": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _fp, C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_gyro_integrate": (None, [_fp, _fp, C.c_float]),
    "rebvio_hip_keyframe_next": (C.c_int, [_vp]),
    "rebvio_hip_next_record": (C.c_int, [_vp, C.POINTER(PairOut), _ip]),
    "rebvio_hip_pairs_started": (C.c_uint64, [_vp]),
    "rebvio_hip_flush": (C.c_int, [_vp]),
    "rebvio_hip_batch_create": (C.c_int, [C.POINTER(Params), C.c_int, C.POINTER(_vp)]),
    "rebvio_hip_batch_destroy": (None, [_vp]),
    "rebvio_hip_batch_lanes": (C.c_int, [_vp]),
    "rebvio_hip_batch_lane": (_vp, [_vp, C.c_int]),
    "rebvio_hip_batch_push_u8_device": (C.c_int, [_vp, C.POINTER(_vp), C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_batch_push_px_device": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_uint64, C.POINTER(PairOut), _ip]),
    "rebvio_hip_batch_push_px_masked_device": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_uint64, C.POINTER(PairOut),
                                                         _ip]),
    "rebvio_hip_batch_push_px_gyro_device": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.POINTER(_fp), C.c_uint64,
                                                       C.POINTER(PairOut), _ip]),
    "rebvio_hip_batch_next_records": (C.c_int, [_vp, C.POINTER(PairOut), _ip]),
    "rebvio_hip_batch_flush": (C.c_int, [_vp]),
    "rebvio_hip_test_glue": (C.c_int, [_vp, _fp, _fp, C.c_float, C.c_float, C.c_int, _fp, C.c_int, C.c_float, _fp, _fp, _fp,
                                      C.POINTER(PairOut), _fp, _fp, C.POINTER(PairOut), _fp, _fp]),
    "rebvio_hip_test_glue_set_next": (C.c_int, [_vp, _fp, C.c_int]),
    "rebvio_hip_test_forge_record_stamp": (C.c_int, [_vp]),
    "rebvio_hip_batch_test_forge_record_stamp": (C.c_int, [_vp]),
    "rebvio_hip_default_depth_prior_opts": (None, [C.POINTER(DepthPriorOpts)]),
    "rebvio_hip_map_fuse_depth_image": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.POINTER(DepthPriorOpts),
                                                  C.POINTER(DepthPriorCounts), _ip]),
    "rebvio_hip_map_fuse_depth_image_device": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.POINTER(DepthPriorOpts),
                                                         C.POINTER(DepthPriorCounts), _ip]),
    "rebvio_hip_map_fuse_depth_image_async": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, C.POINTER(DepthPriorOpts)]),
    "rebvio_hip_depth_prior_last_counts": (C.c_int, [_vp, C.POINTER(DepthPriorCounts)]),
    "rebvio_hip_test_depth_prior_host": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_size_t, C.c_int,
                                                   C.POINTER(DepthPriorOpts), C.POINTER(DepthPriorCounts), _ip]),
    "rebvio_hip_default_stereo_prior_opts": (None, [_vp, C.POINTER(StereoPriorOpts)]),
    "rebvio_hip_map_fuse_stereo": (C.c_int, [_vp, _vp, C.POINTER(StereoPriorOpts), C.POINTER(StereoPriorCounts), _ip, _ip]),
    "rebvio_hip_map_fuse_stereo_async": (C.c_int, [_vp, _vp, _vp, C.POINTER(StereoPriorOpts)]),
    "rebvio_hip_stereo_prior_last_counts": (C.c_int, [_vp, C.POINTER(StereoPriorCounts)]),
    "rebvio_hip_test_stereo_prior_host": (C.c_int, [C.c_int, C.c_int, C.c_float, _vp, C.c_int, _vp, C.c_int, _vp,
                                                    C.POINTER(StereoPriorOpts), C.POINTER(StereoPriorCounts), _ip, _ip]),
    "rebvio_hip_test_map_set_mask": (C.c_int, [_vp, _vp]),
    "rebvio_hip_map_place_signature": (C.c_int, [_vp, _vp, _ip]),
    "rebvio_hip_place_db_create": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "rebvio_hip_place_db_release": (None, [_vp]),
    "rebvio_hip_place_db_clear": (C.c_int, [_vp]),
    "rebvio_hip_place_db_size": (C.c_int, [_vp]),
    "rebvio_hip_place_db_add": (C.c_int, [_vp, _vp, C.c_uint64, _ip]),
    "rebvio_hip_place_db_add_signature": (C.c_int, [_vp, _vp, C.c_int, C.c_uint64, _ip]),
    "rebvio_hip_place_db_entry": (C.c_int, [_vp, C.c_int, _vp, _ip, C.POINTER(C.c_uint64)]),
    "rebvio_hip_place_db_query": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(PlaceMatch), _ip]),
    "rebvio_hip_place_db_query_signature": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(PlaceMatch), _ip]),
    "rebvio_hip_test_place_signature_host": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, _vp, _ip]),
    "rebvio_hip_test_place_query_host": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.POINTER(PlaceMatch), _ip]),
    "rebvio_hip_test_live_resources": (C.c_long, []),
    "rebvio_hip_test_handover_counters": (C.c_int, [_vp, C.POINTER(C.c_ulonglong)]),
    "rebvio_hip_profile_enable": (C.c_int, [_vp, C.c_int]),
    "rebvio_hip_profile_select": (C.c_int, [_vp, C.c_char_p]),
    "rebvio_hip_profile_reset": (C.c_int, [_vp]),
    "rebvio_hip_profile_read": (C.c_int, [_vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), _ip, C.c_int]),
    "rebvio_hip_device_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "rebvio_hip_device_free": (C.c_int, [_vp, _vp]),
    "rebvio_hip_device_upload": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
}


def build(verbose: bool = False) -> str:
    """Compile the backend for gfx950 with hipcc (rebvio_amd/csrc/Makefile)."""
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc")] + ([] if verbose else ["-s"]), check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP backend has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


# pixel formats of the *_px entries (REBVIO_HIP_PX_*) and their bytes per pixel
PX_GRAY8, PX_RGB8, PX_BGR8, PX_RGBA8, PX_BGRA8, PX_YUYV, PX_UYVY = range(7)
PX_BPP = (1, 3, 3, 4, 4, 2, 2)


def _px_frame(frame: np.ndarray, fmt: int, rows: int, cols: int):
    """(pointer, pitch_bytes) of a host frame of pixel format fmt: uint8 [H, W] (1 byte per pixel) or [H, W, bytes per pixel] with
    dense pixels; the row pitch is taken from the array (a padded view is passed as it is)."""
    assert frame.dtype == np.uint8 and 0 <= fmt < len(PX_BPP), (frame.dtype, fmt)
    bpp = PX_BPP[fmt]
    if frame.ndim == 2:
        assert bpp == 1 and frame.shape == (rows, cols) and frame.strides[1] == 1, (frame.shape, frame.strides)
    else:
        assert frame.shape == (rows, cols, bpp) and frame.strides[1:] == (bpp, 1), (frame.shape, frame.strides)
    return _vp(frame.ctypes.data), frame.strides[0]


def _dev_addr(a, nbytes: int, device: int, what: str, dtypes=("uint8",)) -> int:
    """Device address of a frame or detection mask: an int is taken as it is; a torch CUDA tensor is checked (dtype, size,
    contiguity, device) and torch's current stream on it is synchronised, because the library's streams are private and would
    not wait for the kernels that wrote it. The tensor must stay alive and unchanged as rebvio_hip.h says."""
    if isinstance(a, int) or isinstance(a, np.integer):
        return int(a)
    import torch
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"{what}: a device address or a torch tensor, not {type(a).__name__}")
    if str(a.dtype).replace("torch.", "") not in dtypes:
        raise TypeError(f"{what}: dtype {a.dtype}, expected one of {dtypes}")
    if not a.is_cuda or a.device.index != device:
        raise ValueError(f"{what}: tensor on {a.device}, the context runs on cuda:{device}")
    if not a.is_contiguous() or a.numel() * a.element_size() != nbytes:
        raise ValueError(f"{what}: a dense tensor of {nbytes} bytes expected, got shape {tuple(a.shape)} (contiguous: {a.is_contiguous()})")
    torch.cuda.current_stream(a.device).synchronize()
    return a.data_ptr()


def _mask_addr(m, rows: int, cols: int, device: int, what: str) -> int:
    if not (isinstance(m, int) or isinstance(m, np.integer)) and tuple(getattr(m, "shape", ())) != (rows, cols):
        raise ValueError(f"{what}: mask of shape {tuple(getattr(m, 'shape', ()))}, expected ({rows}, {cols})")
    return _dev_addr(m, rows * cols, device, what, ("uint8", "bool"))


class HipError(RuntimeError):
    pass


def _chk(rc):
    if rc != 0:
        raise HipError(f"rebvio_hip error {rc}: {lib().rebvio_hip_last_error().decode()}")


def _f(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(_fp)


def _gyro(R):
    """(keep-alive array, pointer) of a gyro rotation: 9 floats row-major (3x3 or flat), or (None, NULL) for None."""
    if R is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(R, np.float32).reshape(9))
    return a, a.ctypes.data_as(_fp)


def gyro_integrate(R, gyro, dt) -> np.ndarray:
    """R * exp(gyro * dt) as float32 [3, 3]: one gyro sample (rad/s, in the camera frame) added to a pre-integrated rotation
    (rebvio_hip_gyro_integrate; start from np.eye(3) at a frame, the result at the next frame is that frame's R_gyro)."""
    out = np.array(np.asarray(R, np.float32).reshape(9), np.float32)
    g, pg = _f(np.asarray(gyro, np.float32).reshape(3))
    lib().rebvio_hip_gyro_integrate(out.ctypes.data_as(_fp), pg, float(dt))
    return out.reshape(3, 3)


def test_live_resources() -> int:
    """Device buffers, pinned buffers, events and streams the library holds in this process (rebvio_hip_test_live_resources)."""
    return int(lib().rebvio_hip_test_live_resources())


def default_params(rows, cols, **over) -> Params:
    p = Params()
    lib().rebvio_hip_default_params(C.byref(p), rows, cols)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def default_cloud_filter(**over) -> CloudFilter:
    f = CloudFilter()
    lib().rebvio_hip_default_cloud_filter(C.byref(f))
    for k, v in over.items():
        setattr(f, k, v)
    return f


def _cloud_filter(f):
    """None (the library's default), a CloudFilter, or a dict of the fields to change from the default."""
    if f is None or isinstance(f, CloudFilter):
        return f
    return default_cloud_filter(**f)


def cloud_pose(R=None, t=None, scale=1.0) -> CloudPose:
    p = CloudPose()
    p.R[:] = [float(v) for v in np.asarray(np.eye(3) if R is None else R, np.float32).reshape(9)]
    p.t[:] = [float(v) for v in np.asarray(np.zeros(3) if t is None else t, np.float32).reshape(3)]
    p.scale = float(np.float32(scale))
    return p


def _cloud_pose(pose):
    """None (identity), a CloudPose, or (R, t, scale)."""
    if pose is None or isinstance(pose, CloudPose):
        return pose
    return cloud_pose(*pose)


def default_polyline_opts(**over) -> PolylineOpts:
    """The library's defaults (rebvio_hip_default_polyline_opts): the default cloud filter, min_chain_length 8; filter takes a
    CloudFilter or a dict of its fields to change."""
    o = PolylineOpts()
    lib().rebvio_hip_default_polyline_opts(C.byref(o))
    for k, v in over.items():
        if k == "filter" and not isinstance(v, CloudFilter):
            for fk, fv in v.items():
                setattr(o.filter, fk, fv)
        else:
            setattr(o, k, v)
    return o


def edge_chains_host(id_prev, id_next, cap_keylines=None, cap_chains=None):
    """Map.edge_chains on the host, from the two link arrays (rebvio_hip_test_edge_chains_host). Touches no device. Returns (refs
    CHAIN_REF_DTYPE, order int32, starts int32, n_keylines, n_chains), the arrays cut to what the caps let through."""
    idp = np.ascontiguousarray(id_prev, np.int32).reshape(-1)
    idn = np.ascontiguousarray(id_next, np.int32).reshape(-1)
    assert len(idp) == len(idn)
    n = len(idp)
    ck = n if cap_keylines is None else cap_keylines
    cc = n + 1 if cap_chains is None else cap_chains
    refs, order, starts = np.zeros(max(ck, 0), CHAIN_REF_DTYPE), np.zeros(max(ck, 0), np.int32), np.zeros(max(cc, 0), np.int32)
    nk, nc = C.c_int(), C.c_int()
    _chk(lib().rebvio_hip_test_edge_chains_host(idp.ctypes.data_as(_ip) if n else None, idn.ctypes.data_as(_ip) if n else None, n,
                                                refs.ctypes.data if len(refs) else None, ck, order.ctypes.data_as(_ip) if len(order) else None,
                                                starts.ctypes.data_as(_ip) if len(starts) else None, cc, C.byref(nk), C.byref(nc)))
    return refs[:min(nk.value, ck)], order[:min(nk.value, ck)], starts[:min(nc.value + 1, cc)], nk.value, nc.value


def _polylines_call(fn, head_args, n_hint, opts, pose, cap_points, cap_lines):
    cp = n_hint if cap_points is None else cap_points
    cl = n_hint if cap_lines is None else cap_lines
    pts, refs2 = np.zeros(max(cp, 0), CLOUD_POINT_DTYPE), np.zeros((max(cp, 0), 2), np.int32)
    lines = np.zeros(max(cl, 0), POLYLINE_DTYPE)
    npts, nl = C.c_int(), C.c_int()
    _chk(fn(*head_args, opts, _cloud_pose(pose), pts.ctypes.data if len(pts) else None, refs2.ctypes.data_as(_ip) if len(pts) else None, cp,
            lines.ctypes.data if len(lines) else None, cl, C.byref(npts), C.byref(nl)))
    return pts[:min(npts.value, cp)], refs2[:min(npts.value, cp)], lines[:min(nl.value, cl)], npts.value, nl.value


def edge_polylines_host(fm, keylines, opts=None, pose=None, cap_points=None, cap_lines=None):
    """Map.edge_polylines on the host, from a KEYLINE_DTYPE array (rebvio_hip_test_edge_polylines_host). Touches no device. Returns
    (points CLOUD_POINT_DTYPE, refs2 int32 [k, 2] = head, rank, lines POLYLINE_DTYPE, n_points, n_lines)."""
    kl = np.ascontiguousarray(keylines, KEYLINE_DTYPE)
    return _polylines_call(lib().rebvio_hip_test_edge_polylines_host, (float(fm), kl.ctypes.data if len(kl) else None, len(kl)), len(kl),
                           opts, pose, cap_points, cap_lines)


def default_segment_opts(**over) -> SegmentOpts:
    """The library's defaults (rebvio_hip_default_segment_opts): the polyline defaults, tol 1 px, min_length 4 px, min_points 8,
    max_rounds 16; poly takes a PolylineOpts or a dict for default_polyline_opts."""
    o = SegmentOpts()
    lib().rebvio_hip_default_segment_opts(C.byref(o))
    for k, v in over.items():
        setattr(o, k, default_polyline_opts(**v) if k == "poly" and not isinstance(v, PolylineOpts) else v)
    return o


def _segments_call(fn, head_args, n_hint, opts, pose, cap):
    cs = n_hint if cap is None else cap
    segs = np.zeros(max(cs, 0), LINE_SEGMENT_DTYPE)
    counts = SegmentCounts()
    _chk(fn(*head_args, opts, _cloud_pose(pose), segs.ctypes.data if len(segs) else None, cs, C.byref(counts)))
    return segs[:min(counts.kept, cs)], counts


def edge_segments_host(fm, keylines, opts=None, pose=None, cap=None):
    """Map.edge_segments on the host, from a KEYLINE_DTYPE array (rebvio_hip_test_edge_segments_host). Touches no device. Returns
    (segments LINE_SEGMENT_DTYPE, SegmentCounts)."""
    kl = np.ascontiguousarray(keylines, KEYLINE_DTYPE)
    return _segments_call(lib().rebvio_hip_test_edge_segments_host, (float(fm), kl.ctypes.data if len(kl) else None, len(kl)), len(kl), opts,
                          pose, cap)


def default_kf_pose_opts(**over) -> KfPoseOpts:
    """The library's defaults (rebvio_hip_default_kf_pose_opts); kf_filter takes a CloudFilter or a dict of its fields to change."""
    o = KfPoseOpts()
    lib().rebvio_hip_default_kf_pose_opts(C.byref(o))
    for k, v in over.items():
        if k == "kf_filter" and not isinstance(v, CloudFilter):
            for fk, fv in v.items():
                setattr(o.kf_filter, fk, fv)
        else:
            setattr(o, k, v)
    return o


def _guess(a, n):
    """(keep-alive array, pointer) of a pose guess: n doubles, or (None, NULL) for None."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(n))
    return a, a.ctypes.data_as(_dp)


def kf_pose_host(fm, prs4, kf_matches, cur_pos_img, cur_gradient, records, opts=None, R0=None, t0=None) -> KfPose:
    """The solve of Map.keyframe_pose on the host, from arrays (rebvio_hip_test_kf_pose_host): a snapshot's download, the current
    map's pos_img / gradient, KF_MATCH_DTYPE records. Touches no device; the terms are summed in record order."""
    prs4 = np.ascontiguousarray(prs4, np.float32).reshape(-1, 4)
    kf_matches = np.ascontiguousarray(kf_matches, np.uint32)
    q = np.ascontiguousarray(cur_pos_img, np.float32).reshape(-1, 2)
    g = np.ascontiguousarray(cur_gradient, np.float32).reshape(-1, 2)
    rec = np.ascontiguousarray(records, KF_MATCH_DTYPE)
    assert len(prs4) == len(kf_matches) and len(q) == len(g)
    (kR, pR), (kt, pt) = _guess(R0, 9), _guess(t0, 3)
    out = KfPose()
    up = C.POINTER(C.c_uint)
    _chk(lib().rebvio_hip_test_kf_pose_host(float(fm), prs4.ctypes.data_as(_fp) if len(prs4) else None,
                                            kf_matches.ctypes.data_as(up) if len(prs4) else None, len(prs4),
                                            q.ctypes.data_as(_fp) if len(q) else None, g.ctypes.data_as(_fp) if len(q) else None, len(q),
                                            rec.ctypes.data_as(C.POINTER(KfMatch)) if len(rec) else None, len(rec), opts, pR, pt,
                                            C.byref(out)))
    del kR, kt
    return out


def default_kf_align_opts(ctx=None, **over) -> KfAlignOpts:
    """The library's defaults (rebvio_hip_default_kf_align_opts): max_dist is ctx's search_range (40, the default one, without a
    context); kf_filter takes a CloudFilter or a dict of its fields to change."""
    o = KfAlignOpts()
    lib().rebvio_hip_default_kf_align_opts(ctx.h if ctx is not None else None, C.byref(o))
    for k, v in over.items():
        if k == "kf_filter" and not isinstance(v, CloudFilter):
            for fk, fv in v.items():
                setattr(o.kf_filter, fk, fv)
        else:
            setattr(o, k, v)
    return o


def kf_align_host(fm, cx, cy, rows, cols, search_range, prs4, kf_matches, normals, cur_pos, cur_unit, df_id, df_dist, opts=None, R0=None,
                  t0=None):
    """The solve of Map.keyframe_align on the host, from arrays (rebvio_hip_test_kf_align_host): the camera, a snapshot's download and
    normals (or None), the map's pos / unit and its distance field as Map.distance_field returns it. Touches no device; the terms
    are summed in index order. Returns (KfPose, assoc int32 [kf_size])."""
    prs4 = np.ascontiguousarray(prs4, np.float32).reshape(-1, 4)
    kf_matches = np.ascontiguousarray(kf_matches, np.uint32)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(cur_pos, np.float32).reshape(-1, 2)
    u = np.ascontiguousarray(cur_unit, np.float32).reshape(-1, 2)
    ids = np.ascontiguousarray(df_id, np.int32).reshape(-1)
    dists = np.ascontiguousarray(df_dist, np.int32).reshape(-1)
    assert len(prs4) == len(kf_matches) and len(q) == len(u) and (nrm is None or len(nrm) == len(prs4))
    assert len(ids) == len(dists) == int(rows) * int(cols)
    (kR, pR), (kt, pt) = _guess(R0, 9), _guess(t0, 3)
    out = KfPose()
    assoc = np.full(len(prs4), -1, np.int32)
    up = C.POINTER(C.c_uint)
    _chk(lib().rebvio_hip_test_kf_align_host(float(fm), float(cx), float(cy), int(rows), int(cols), int(search_range),
                                             prs4.ctypes.data_as(_fp) if len(prs4) else None,
                                             kf_matches.ctypes.data_as(up) if len(prs4) else None,
                                             nrm.ctypes.data_as(_fp) if nrm is not None and len(nrm) else None, len(prs4),
                                             q.ctypes.data_as(_fp) if len(q) else None, u.ctypes.data_as(_fp) if len(q) else None, len(q),
                                             ids.ctypes.data_as(_ip) if len(ids) else None, dists.ctypes.data_as(_ip) if len(ids) else None,
                                             opts, pR, pt, C.byref(out), assoc.ctypes.data_as(_ip) if len(assoc) else None))
    del kR, kt
    return out, assoc


def kf_hypothesis(snap, R0=None, t0=None) -> KfHypothesis:
    """One hypothesis for Map.keyframe_align_many: a KfSnapshot (or None, for the host helpers) and a guess (None: identity / zero)"""
    h = KfHypothesis()
    h.snap = snap.h if snap is not None else None
    h.R0[:] = (np.eye(3) if R0 is None else np.asarray(R0, np.float64)).reshape(9)
    h.t0[:] = np.zeros(3) if t0 is None else np.asarray(t0, np.float64).reshape(3)
    return h


def _hyp_array(items, ctype):
    arr = (ctype * len(items))()
    for k, x in enumerate(items):
        C.memmove(C.byref(arr, k * C.sizeof(ctype)), C.byref(x), C.sizeof(ctype))
    return arr


def kf_align_best(results, min_inliers=0) -> int:
    """Index of the best result (rebvio_hip_kf_align_best): status 0 and inliers >= min_inliers; the most inliers, then the smaller
    cost, then the lower index. -1: none qualifies."""
    results = list(results)
    arr = _hyp_array(results, KfHypResult)
    rc = lib().rebvio_hip_kf_align_best(arr if results else None, len(results), int(min_inliers))
    if rc < -1:
        _chk(rc)
    return rc


def kf_hypotheses_around(snap, R, t, rot_step, trans_step):
    """13 starts around the guess (R, t) for `snap` (rebvio_hip_kf_hypotheses_around): the guess itself, +- rot_step about x, y and z,
    +- trans_step along x, y and z. Returns a list of KfHypothesis; touches no device."""
    (kR, pR), (kt, pt) = _guess(R, 9), _guess(t, 3)
    out = (KfHypothesis * 13)()
    _chk(lib().rebvio_hip_kf_hypotheses_around(snap.h if snap is not None else None, pR, pt, float(rot_step), float(trans_step), out))
    del kR, kt
    return [KfHypothesis.from_buffer_copy(out[k]) for k in range(13)]


def kf_align_many_host(fm, cx, cy, rows, cols, search_range, prs4, kf_matches, normals, cur_pos, cur_unit, df_id, df_dist, R0s, t0s,
                       opts=None):
    """kf_align_host for n guesses against one snapshot's arrays (rebvio_hip_test_kf_align_many_host): R0s [n, 3, 3], t0s [n, 3].
    Returns a list of n KfHypResult - pose byte for byte kf_align_host's, inliers counted from the same terms. Touches no device."""
    prs4 = np.ascontiguousarray(prs4, np.float32).reshape(-1, 4)
    kf_matches = np.ascontiguousarray(kf_matches, np.uint32)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(cur_pos, np.float32).reshape(-1, 2)
    u = np.ascontiguousarray(cur_unit, np.float32).reshape(-1, 2)
    ids = np.ascontiguousarray(df_id, np.int32).reshape(-1)
    dists = np.ascontiguousarray(df_dist, np.int32).reshape(-1)
    Rs = np.ascontiguousarray(R0s, np.float64).reshape(-1, 9)
    ts = np.ascontiguousarray(t0s, np.float64).reshape(-1, 3)
    assert len(prs4) == len(kf_matches) and len(q) == len(u) and (nrm is None or len(nrm) == len(prs4)) and len(Rs) == len(ts)
    assert len(ids) == len(dists) == int(rows) * int(cols)
    n = len(Rs)
    out = (KfHypResult * max(n, 1))()
    up = C.POINTER(C.c_uint)
    _chk(lib().rebvio_hip_test_kf_align_many_host(float(fm), float(cx), float(cy), int(rows), int(cols), int(search_range),
                                                  prs4.ctypes.data_as(_fp) if len(prs4) else None,
                                                  kf_matches.ctypes.data_as(up) if len(prs4) else None,
                                                  nrm.ctypes.data_as(_fp) if nrm is not None and len(nrm) else None, len(prs4),
                                                  q.ctypes.data_as(_fp) if len(q) else None, u.ctypes.data_as(_fp) if len(q) else None,
                                                  len(q), ids.ctypes.data_as(_ip) if len(ids) else None,
                                                  dists.ctypes.data_as(_ip) if len(ids) else None, opts, Rs.ctypes.data_as(_dp),
                                                  ts.ctypes.data_as(_dp), n, out))
    return [KfHypResult.from_buffer_copy(out[k]) for k in range(n)]


def default_kf_fuse_opts(ctx=None, **over) -> KfFuseOpts:
    """The library's defaults (rebvio_hip_default_kf_fuse_opts): pixel_sigma is ctx's pixel_uncertainty and max_dist its search_range
    (1 and 40, the default ones, without a context); kf_filter takes a CloudFilter or a dict of its fields to change."""
    o = KfFuseOpts()
    lib().rebvio_hip_default_kf_fuse_opts(ctx.h if ctx is not None else None, C.byref(o))
    for k, v in over.items():
        if k == "kf_filter" and not isinstance(v, CloudFilter):
            for fk, fv in v.items():
                setattr(o.kf_filter, fk, fv)
        else:
            setattr(o, k, v)
    return o


def kf_fuse_host(fm, cx, cy, rows, cols, search_range, prs4, kf_matches, normals, cur_pos, cur_unit, df_id, df_dist, opts=None, R=None,
                 t=None):
    """KfSnapshot.fuse_depth on the host, from arrays (rebvio_hip_test_kf_fuse_host; the arrays of kf_align_host). Touches no device
    and leaves its inputs alone. Returns (KfFuse, new prs4 float32 [n, 4], new matches uint32 [n], assoc int32 [n])."""
    prs4 = np.array(prs4, np.float32).reshape(-1, 4)            # (copies: the hook updates them in place)
    kf_matches = np.array(kf_matches, np.uint32).reshape(-1)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(cur_pos, np.float32).reshape(-1, 2)
    u = np.ascontiguousarray(cur_unit, np.float32).reshape(-1, 2)
    ids = np.ascontiguousarray(df_id, np.int32).reshape(-1)
    dists = np.ascontiguousarray(df_dist, np.int32).reshape(-1)
    assert len(prs4) == len(kf_matches) and len(q) == len(u) and (nrm is None or len(nrm) == len(prs4))
    assert len(ids) == len(dists) == int(rows) * int(cols)
    (kR, pR), (kt, pt) = _guess(R, 9), _guess(t, 3)
    out = KfFuse()
    assoc = np.full(len(prs4), -2 ** 31, np.int32)
    up = C.POINTER(C.c_uint)
    _chk(lib().rebvio_hip_test_kf_fuse_host(float(fm), float(cx), float(cy), int(rows), int(cols), int(search_range),
                                            prs4.ctypes.data_as(_fp) if len(prs4) else None,
                                            kf_matches.ctypes.data_as(up) if len(prs4) else None,
                                            nrm.ctypes.data_as(_fp) if nrm is not None and len(nrm) else None, len(prs4),
                                            q.ctypes.data_as(_fp) if len(q) else None, u.ctypes.data_as(_fp) if len(q) else None, len(q),
                                            ids.ctypes.data_as(_ip) if len(ids) else None, dists.ctypes.data_as(_ip) if len(ids) else None,
                                            opts, pR, pt, C.byref(out), assoc.ctypes.data_as(_ip) if len(assoc) else None))
    del kR, kt
    return out, prs4, kf_matches, assoc


def default_depth_prior_opts(**over) -> DepthPriorOpts:
    """The library's defaults (rebvio_hip_default_depth_prior_opts), with the given fields changed."""
    o = DepthPriorOpts()
    lib().rebvio_hip_default_depth_prior_opts(C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _depth_image(depth, fmt, rows, cols):
    """(array kept alive, address, pitch in bytes, format) of a host depth image: uint16 or float32, [rows, cols], rows any number
    of bytes apart (a column slice of a wider array keeps its pitch); anything else is copied dense."""
    depth = np.asarray(depth)
    if fmt is None:
        fmt = DEPTH_U16 if depth.dtype == np.uint16 else DEPTH_F32
    dt = np.uint16 if fmt == DEPTH_U16 else np.float32
    if depth.dtype != dt or depth.ndim != 2 or depth.strides[1] != depth.itemsize or depth.strides[0] < cols * depth.itemsize:
        depth = np.ascontiguousarray(depth, dt)
    assert depth.shape == (rows, cols), (depth.shape, rows, cols)
    return depth, depth.ctypes.data, depth.strides[0], fmt


def depth_prior_host(rows, cols, keylines, depth, fmt=None, opts=None):
    """Map.fuse_depth_image on the host, from arrays (rebvio_hip_test_depth_prior_host). Touches no device and leaves its inputs
    alone. Returns (DepthPriorCounts, the updated KEYLINE_DTYPE copy, outcome int32 [n])."""
    kl = np.array(keylines, KEYLINE_DTYPE).reshape(-1)  # (a copy: the hook updates it in place)
    keep, addr, pitch, fmt = _depth_image(depth, fmt, rows, cols)
    out = DepthPriorCounts()
    outcome = np.zeros(len(kl), np.int32)
    _chk(lib().rebvio_hip_test_depth_prior_host(int(rows), int(cols), kl.ctypes.data if len(kl) else None, len(kl), addr, pitch, fmt,
                                                opts, C.byref(out), outcome.ctypes.data_as(_ip) if len(kl) else None))
    del keep
    return out, kl, outcome


def default_stereo_prior_opts(ctx=None, **over) -> StereoPriorOpts:
    """The library's defaults (rebvio_hip_default_stereo_prior_opts): cos_min and norm_tol are ctx's match_threshold_angle and
    match_threshold_norm (45 degrees and 1, the default ones, without a context). baseline has no default: give it."""
    o = StereoPriorOpts()
    lib().rebvio_hip_default_stereo_prior_opts(ctx.h if ctx is not None else None, C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


def stereo_prior_host(rows, cols, fm, left, right, right_mask, opts):
    """Map.fuse_stereo on the host, from arrays (rebvio_hip_test_stereo_prior_host). Touches no device and leaves its inputs alone.
    Returns (StereoPriorCounts, the updated KEYLINE_DTYPE copy of left, outcome int32 [n], winner int32 [n])."""
    kl = np.array(left, KEYLINE_DTYPE).reshape(-1)  # (a copy: the hook updates it in place)
    kr = np.ascontiguousarray(right, KEYLINE_DTYPE).reshape(-1)
    mask = np.ascontiguousarray(right_mask, np.int32).reshape(-1)
    assert mask.size == int(rows) * int(cols), (mask.size, rows, cols)
    out = StereoPriorCounts()
    outcome = np.zeros(len(kl), np.int32)
    winner = np.zeros(len(kl), np.int32)
    _chk(lib().rebvio_hip_test_stereo_prior_host(int(rows), int(cols), float(fm), kl.ctypes.data if len(kl) else None, len(kl),
                                                 kr.ctypes.data if len(kr) else None, len(kr), mask.ctypes.data if mask.size else None,
                                                 opts, C.byref(out), outcome.ctypes.data_as(_ip) if len(kl) else None,
                                                 winner.ctypes.data_as(_ip) if len(kl) else None))
    return out, kl, outcome, winner


def _place_sig(sig):
    sig = np.ascontiguousarray(sig, np.uint16).reshape(-1)
    assert sig.size == PLACE_WORDS, sig.shape
    return sig


def _place_matches(out, count):
    return [PlaceMatch(out[i].distance, out[i].index, out[i].tag) for i in range(count)]


def place_signature_host(rows, cols, keylines):
    """Map.place_signature on the host, from a KEYLINE_DTYPE array (rebvio_hip_test_place_signature_host). Touches no device.
    Returns (sig uint16 [384], counted)."""
    kl = np.ascontiguousarray(keylines, KEYLINE_DTYPE).reshape(-1)
    sig = np.zeros(PLACE_WORDS, np.uint16)
    n = C.c_int()
    _chk(lib().rebvio_hip_test_place_signature_host(int(rows), int(cols), kl.ctypes.data if len(kl) else None, len(kl), sig.ctypes.data,
                                                    C.byref(n)))
    return sig, n.value


def place_query_host(rows384, sig, k, exclude_last=0):
    """PlaceDb.query_signature on the host (rebvio_hip_test_place_query_host): rows384 uint16 [size, 384]. Touches no device. Returns
    the list of PlaceMatch (tag 0), nearest first."""
    rows384 = np.ascontiguousarray(rows384, np.uint16).reshape(-1, PLACE_WORDS)
    sig = _place_sig(sig)
    out = (PlaceMatch * PLACE_TOPK_MAX)()
    n = C.c_int()
    _chk(lib().rebvio_hip_test_place_query_host(rows384.ctypes.data if len(rows384) else None, len(rows384), sig.ctypes.data, int(k),
                                                int(exclude_last), out, C.byref(n)))
    return _place_matches(out, n.value)


class PlaceDb:
    """A device-resident database of place signatures (rebvio_hip_place_db_create; include/rebvio_hip.h is the definition):
    add() maps as keyframes are marked, query() with a later map, release() when done."""

    def __init__(self, h, cap):
        self.h, self.cap = h, cap

    def add(self, map, tag=0) -> int:
        """Queues the signature of `map` as the next row (rebvio_hip_place_db_add; no host wait). Returns its index."""
        i = C.c_int()
        _chk(lib().rebvio_hip_place_db_add(self.h, map.h if map is not None else None, int(tag), C.byref(i)))
        return i.value

    def add_signature(self, sig, counted=0, tag=0) -> int:
        """Uploads 384 words of the caller's as the next row (rebvio_hip_place_db_add_signature; synchronous). Returns its index."""
        sig = _place_sig(sig)
        i = C.c_int()
        _chk(lib().rebvio_hip_place_db_add_signature(self.h, sig.ctypes.data, int(counted), int(tag), C.byref(i)))
        return i.value

    def entry(self, index):
        """(sig uint16 [384], counted, tag) of one row (rebvio_hip_place_db_entry; waits for the stream)"""
        sig = np.zeros(PLACE_WORDS, np.uint16)
        n, tag = C.c_int(), C.c_uint64()
        _chk(lib().rebvio_hip_place_db_entry(self.h, int(index), sig.ctypes.data, C.byref(n), C.byref(tag)))
        return sig, n.value, tag.value

    def query(self, map, k=1, exclude_last=0):
        """The k entries nearest to the signature of `map` among all but the last exclude_last, nearest first, as a list of
        PlaceMatch (rebvio_hip_place_db_query)."""
        out = (PlaceMatch * PLACE_TOPK_MAX)()
        n = C.c_int()
        _chk(lib().rebvio_hip_place_db_query(self.h, map.h if map is not None else None, int(k), int(exclude_last), out, C.byref(n)))
        return _place_matches(out, n.value)

    def query_signature(self, sig, k=1, exclude_last=0):
        """The same from 384 words of the caller's (rebvio_hip_place_db_query_signature)"""
        sig = _place_sig(sig)
        out = (PlaceMatch * PLACE_TOPK_MAX)()
        n = C.c_int()
        _chk(lib().rebvio_hip_place_db_query_signature(self.h, sig.ctypes.data, int(k), int(exclude_last), out, C.byref(n)))
        return _place_matches(out, n.value)

    def clear(self):
        _chk(lib().rebvio_hip_place_db_clear(self.h))

    def size(self) -> int:
        n = lib().rebvio_hip_place_db_size(self.h)
        if n < 0:
            raise HipError(lib().rebvio_hip_last_error().decode())
        return n

    def release(self):
        if self.h:
            lib().rebvio_hip_place_db_release(self.h)  # safe after the context is closed too
            self.h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def default_kf_handover_opts(ctx=None, **over) -> KfHandoverOpts:
    """The library's defaults (rebvio_hip_default_kf_handover_opts): max_dist is ctx's search_range (40, the default one, without a
    context); kf_filter takes a CloudFilter or a dict of its fields to change."""
    o = KfHandoverOpts()
    lib().rebvio_hip_default_kf_handover_opts(ctx.h if ctx is not None else None, C.byref(o))
    for k, v in over.items():
        if k == "kf_filter" and not isinstance(v, CloudFilter):
            for fk, fv in v.items():
                setattr(o.kf_filter, fk, fv)
        else:
            setattr(o, k, v)
    return o


def kf_handover_host(fm, cx, cy, rows, cols, search_range, prs4, kf_matches, normals, cur_pos, cur_unit, df_id, df_dist, dst_prs4,
                     dst_matches, opts=None, R=None, t=None):
    """KfSnapshot.handover_depth on the host, from arrays (rebvio_hip_test_kf_handover_host; the arrays of kf_fuse_host for the outgoing
    snapshot, dst_prs4 / dst_matches for the successor). Touches no device and leaves its inputs alone. Returns (KfHandover, new
    dst_prs4 float32 [m, 4], new dst_matches uint32 [m], assoc int32 [n])."""
    prs4 = np.ascontiguousarray(prs4, np.float32).reshape(-1, 4)
    kf_matches = np.ascontiguousarray(kf_matches, np.uint32).reshape(-1)
    dst_prs4 = np.array(dst_prs4, np.float32).reshape(-1, 4)    # (copies: the hook updates them in place)
    dst_matches = np.array(dst_matches, np.uint32).reshape(-1)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(cur_pos, np.float32).reshape(-1, 2)
    u = np.ascontiguousarray(cur_unit, np.float32).reshape(-1, 2)
    ids = np.ascontiguousarray(df_id, np.int32).reshape(-1)
    dists = np.ascontiguousarray(df_dist, np.int32).reshape(-1)
    assert len(prs4) == len(kf_matches) and len(q) == len(u) and (nrm is None or len(nrm) == len(prs4))
    assert len(dst_prs4) == len(dst_matches) and len(ids) == len(dists) == int(rows) * int(cols)
    (kR, pR), (kt, pt) = _guess(R, 9), _guess(t, 3)
    out = KfHandover()
    assoc = np.full(len(prs4), -2 ** 31, np.int32)
    up = C.POINTER(C.c_uint)
    _chk(lib().rebvio_hip_test_kf_handover_host(float(fm), float(cx), float(cy), int(rows), int(cols), int(search_range),
                                                prs4.ctypes.data_as(_fp) if len(prs4) else None,
                                                kf_matches.ctypes.data_as(up) if len(prs4) else None,
                                                nrm.ctypes.data_as(_fp) if nrm is not None and len(nrm) else None, len(prs4),
                                                q.ctypes.data_as(_fp) if len(q) else None, u.ctypes.data_as(_fp) if len(q) else None, len(q),
                                                ids.ctypes.data_as(_ip) if len(ids) else None, dists.ctypes.data_as(_ip) if len(ids) else None,
                                                dst_prs4.ctypes.data_as(_fp) if len(dst_prs4) else None,
                                                dst_matches.ctypes.data_as(up) if len(dst_prs4) else None, len(dst_prs4),
                                                opts, pR, pt, C.byref(out), assoc.ctypes.data_as(_ip) if len(assoc) else None))
    del kR, kt
    return out, dst_prs4, dst_matches, assoc


def kf_cloud_host(fm, prs4, kf_matches, filter=None, pose=None, cap=None, return_count=False):
    """KfSnapshot.point_cloud on the host, from arrays (rebvio_hip_test_kf_cloud_host): prs4 float32 [n, 4] and matches uint32 [n] as
    KfSnapshot.download returns them. Touches no device. Returns the CLOUD_POINT_DTYPE array (and the count with return_count)."""
    prs4 = np.ascontiguousarray(prs4, np.float32).reshape(-1, 4)
    kf_matches = np.ascontiguousarray(kf_matches, np.uint32).reshape(-1)
    assert len(prs4) == len(kf_matches)
    if cap is None:
        cap = len(prs4)
    out = np.zeros(cap, CLOUD_POINT_DTYPE)
    n = C.c_int()
    _chk(lib().rebvio_hip_test_kf_cloud_host(float(fm), prs4.ctypes.data_as(_fp) if len(prs4) else None,
                                             kf_matches.ctypes.data_as(C.POINTER(C.c_uint)) if len(prs4) else None, len(prs4),
                                             _cloud_filter(filter), _cloud_pose(pose), out.ctypes.data if cap else None, cap, C.byref(n)))
    out = out[:min(n.value, cap)]
    return (out, n.value) if return_count else out


class KfSnapshot:
    """A keyframe as it was when marked (rebvio_hip_map_keyframe_snapshot): download() its keylines, release() when done."""

    def __init__(self, h):
        self.h = h

    def download(self):
        """(prs4 float32 [n, 4] = pos_img.x, pos_img.y, rho, sigma_rho; matches uint32 [n]) of the keyframe's n keylines"""
        n = C.c_int()
        _chk(lib().rebvio_hip_kf_snapshot_download(self.h, None, None, 0, C.byref(n)))
        prs, mt = np.zeros((n.value, 4), np.float32), np.zeros(n.value, np.uint32)
        if n.value:
            _chk(lib().rebvio_hip_kf_snapshot_download(self.h, prs.ctypes.data_as(_fp), mt.ctypes.data_as(C.POINTER(C.c_uint)), n.value,
                                                       C.byref(n)))
        return prs, mt

    def add_normals(self, map):
        """Keeps gradient / gradient_norm of `map`'s keylines next to the snapshot (rebvio_hip_kf_snapshot_add_normals; queued on the
        track stream, returns at once): the gradient test of Map.keyframe_align. `map` is the map the snapshot was taken from, where
        it was taken."""
        _chk(lib().rebvio_hip_kf_snapshot_add_normals(self.h, map.h))

    def normals(self):
        """float32 [n, 2]: the normals add_normals kept (error -7 when none were added)"""
        n = C.c_int()
        _chk(lib().rebvio_hip_kf_snapshot_download_normals(self.h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 2), np.float32)
        if n.value:
            _chk(lib().rebvio_hip_kf_snapshot_download_normals(self.h, out.ctypes.data_as(_fp), n.value, C.byref(n)))
        return out

    def fuse_depth(self, map, R, t, opts=None, want_assoc=False):
        """Folds `map`, seen from the pose X_cur = R X_kf + t (e.g. Map.keyframe_align's), into this snapshot's rho / sigma_rho: one
        scalar Kalman update per associated keyline (rebvio_hip_kf_snapshot_fuse_depth; synchronous). opts: a KfFuseOpts or None
        for the defaults. Returns the KfFuse counts; want_assoc: also the int32 array with, per keyframe keyline, the owner i when
        fused, -1 - i when gated or flat, INT_MIN when not associated. Fusing one map twice counts its pixels twice."""
        (kR, pR), (kt, pt) = _guess(R, 9), _guess(t, 3)
        out = KfFuse()
        assoc = None
        if want_assoc:
            n = C.c_int()
            _chk(lib().rebvio_hip_kf_snapshot_download(self.h, None, None, 0, C.byref(n)))
            assoc = np.full(n.value, -2 ** 31, np.int32)
        _chk(lib().rebvio_hip_kf_snapshot_fuse_depth(self.h, map.h, opts, pR, pt, C.byref(out),
                                                     assoc.ctypes.data_as(_ip) if want_assoc and len(assoc) else None))
        del kR, kt
        return (out, assoc) if want_assoc else out

    def handover_depth(self, src, map, R, t, opts=None, want_assoc=False):
        """Takes over the refined depths of `src`, the outgoing keyframe's snapshot, where they are better than this snapshot's own
        (rebvio_hip_kf_snapshot_handover_depth; synchronous). This snapshot must have been taken from `map`; (R, t) is the pose
        X_cur = R X_kf + t of src against map (e.g. Map.keyframe_align's). src is only read; the two estimates of a slot are never
        combined. opts: a KfHandoverOpts or None for the defaults. Returns the KfHandover counts; want_assoc: also the int32 array
        with, per src keyline, the slot i when it won an adopted slot, -1 - i for any other associated keyline, INT_MIN when not
        associated."""
        (kR, pR), (kt, pt) = _guess(R, 9), _guess(t, 3)
        out = KfHandover()
        assoc = None
        if want_assoc:
            n = C.c_int()
            _chk(lib().rebvio_hip_kf_snapshot_download(src.h, None, None, 0, C.byref(n)))
            assoc = np.full(n.value, -2 ** 31, np.int32)
        _chk(lib().rebvio_hip_kf_snapshot_handover_depth(self.h, src.h if src is not None else None, map.h if map is not None else None, opts,
                                                         pR, pt, C.byref(out), assoc.ctypes.data_as(_ip) if want_assoc and len(assoc) else None))
        del kR, kt
        return (out, assoc) if want_assoc else out

    def point_cloud(self, filter=None, pose=None, cap=None, return_count=False):
        """The snapshot's depth-bearing keylines - as marked, or as fuse_depth has refined them - as a CLOUD_POINT_DTYPE array
        (rebvio_hip_kf_snapshot_point_cloud; synchronous; filter / pose as Map.point_cloud, pose None = the keyframe's own frame in
        keyframe depth units). `keyline` indexes download() / normals(); gradient_norm is 0. cap: at most this many records (default:
        the snapshot's size); return_count: also the number of keylines that passed, which may exceed cap."""
        n = C.c_int()
        if cap is None:
            _chk(lib().rebvio_hip_kf_snapshot_download(self.h, None, None, 0, C.byref(n)))
            cap = n.value
        out = np.zeros(cap, CLOUD_POINT_DTYPE)
        _chk(lib().rebvio_hip_kf_snapshot_point_cloud(self.h, _cloud_filter(filter), _cloud_pose(pose), out.ctypes.data if cap else None,
                                                      cap, C.byref(n)))
        out = out[:min(n.value, cap)]
        return (out, n.value) if return_count else out

    def point_cloud_async(self, filter=None, pose=None) -> "Cloud":
        """Queues the extraction on the track stream and returns at once (rebvio_hip_kf_snapshot_point_cloud_async; allowed between
        track_pair_finish_async(k) and track_pair_begin(k+1)). The Cloud is the kind Context.point_cloud_async returns."""
        h = _vp()
        _chk(lib().rebvio_hip_kf_snapshot_point_cloud_async(self.h, _cloud_filter(filter), _cloud_pose(pose), C.byref(h)))
        return Cloud(h)

    def release(self):
        if self.h:
            lib().rebvio_hip_kf_snapshot_release(self.h)  # safe after the context is closed too
            self.h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Cloud:
    """A queued point cloud (rebvio_hip_map_point_cloud_async): wait() for the records, release() when done with them."""

    def __init__(self, h):
        self.h = h
        self.device_points = None

    def wait(self, copy=True) -> np.ndarray:
        """The records as a CLOUD_POINT_DTYPE array: a copy, or with copy=False a view of the library's buffer that is valid until
        release(). device_points then holds the device address of the same records."""
        pts, dev, n = _vp(), _vp(), C.c_int()
        _chk(lib().rebvio_hip_cloud_wait(self.h, C.byref(pts), C.byref(n), C.byref(dev)))
        self.device_points = dev.value
        if n.value == 0:
            return np.zeros(0, CLOUD_POINT_DTYPE)
        buf = (C.c_char * (n.value * CLOUD_POINT_DTYPE.itemsize)).from_address(pts.value)
        a = np.frombuffer(buf, CLOUD_POINT_DTYPE)
        return a.copy() if copy else a

    def release(self):
        if self.h:
            lib().rebvio_hip_cloud_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Map:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def release(self):
        if self.h:
            lib().rebvio_hip_map_release(self.h)  # safe after the context is closed too: the library drops the husk
            self.h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def size(self):
        n = lib().rebvio_hip_map_size(self.h)
        if n < 0:
            raise HipError(lib().rebvio_hip_last_error().decode())
        return n

    @property
    def threshold(self):
        return lib().rebvio_hip_map_threshold(self.h)

    def render_edge_image(self, gray_u8=None) -> np.ndarray:
        rows, cols = self.ctx.rows, self.ctx.cols
        out = np.empty((rows, cols, 3), np.uint8)
        g = None
        if gray_u8 is not None:
            gray_u8 = np.ascontiguousarray(gray_u8, np.uint8)
            assert gray_u8.shape == (rows, cols)
            g = gray_u8.ctypes.data_as(_vp)
        _chk(lib().rebvio_hip_render_edge_image(self.h, g, out.ctypes.data_as(_vp)))
        return out

    def keylines(self) -> np.ndarray:
        out = np.zeros(self.size(), KEYLINE_DTYPE)
        _chk(lib().rebvio_hip_map_download(self.h, out.ctypes.data if out.size else None, None))
        return out

    def mask(self) -> np.ndarray:
        out = np.empty((self.ctx.rows, self.ctx.cols), np.int32)
        _chk(lib().rebvio_hip_map_download(self.h, None, out.ctypes.data_as(_ip)))
        return out

    def distance_field(self):
        """The field built from THIS map (DistanceField::operator[] for all cells)."""
        ids = np.empty((self.ctx.rows, self.ctx.cols), np.int32)
        dist = np.empty((self.ctx.rows, self.ctx.cols), np.int32)
        _chk(lib().rebvio_hip_map_distance_field(self.h, ids.ctypes.data_as(_ip), dist.ctypes.data_as(_ip)))
        return ids, dist

    def search_match(self, query_keyline, vel, Rvel, Rback, max_radius=40.0) -> int:
        """EdgeMap::searchMatch: this map is searched for a match of `query_keyline` (one KEYLINE_DTYPE record)."""
        q = np.ascontiguousarray(np.asarray(query_keyline, KEYLINE_DTYPE).reshape(1))
        vel, pv = _f(vel)
        Rvel, prv = _f(np.asarray(Rvel).reshape(9))
        Rback, prb = _f(np.asarray(Rback).reshape(9))
        out = C.c_int(-2)
        _chk(lib().rebvio_hip_search_match(self.ctx.h, self.h, q.ctypes.data, pv, prv, prb, max_radius, C.byref(out)))
        return out.value

    def point_cloud(self, filter=None, pose=None, cap=None, return_count=False):
        """The map's depth-bearing keylines as a CLOUD_POINT_DTYPE array (rebvio_hip_map_point_cloud; filter / pose: see
        _cloud_filter / _cloud_pose). cap: at most this many records (default: the map's size); return_count: also the number of
        keylines that passed, which may exceed cap."""
        if cap is None:
            cap = self.size()
        out = np.zeros(cap, CLOUD_POINT_DTYPE)
        n = C.c_int()
        _chk(lib().rebvio_hip_map_point_cloud(self.h, _cloud_filter(filter), _cloud_pose(pose), out.ctypes.data if cap else None,
                                              cap, C.byref(n)))
        out = out[:min(n.value, cap)]
        return (out, n.value) if return_count else out

    def edge_chains(self, cap_keylines=None, cap_chains=None):
        """Every keyline's edge chain and the chain table (rebvio_hip_map_edge_chains; include/rebvio_hip.h is the definition).
        Returns (refs CHAIN_REF_DTYPE, order int32, starts int32, n_keylines, n_chains); the caps (default: everything) cut the
        arrays, never the counts."""
        n = self.ctx.p.keylines_max
        ck = n if cap_keylines is None else cap_keylines
        cc = n + 1 if cap_chains is None else cap_chains
        refs, order, starts = np.zeros(max(ck, 0), CHAIN_REF_DTYPE), np.zeros(max(ck, 0), np.int32), np.zeros(max(cc, 0), np.int32)
        nk, nc = C.c_int(), C.c_int()
        _chk(lib().rebvio_hip_map_edge_chains(self.h, refs.ctypes.data if len(refs) else None, ck,
                                              order.ctypes.data_as(_ip) if len(order) else None,
                                              starts.ctypes.data_as(_ip) if len(starts) else None, cc, C.byref(nk), C.byref(nc)))
        return refs[:min(nk.value, ck)], order[:min(nk.value, ck)], starts[:min(nc.value + 1, cc)], nk.value, nc.value

    def edge_polylines(self, opts=None, pose=None, cap_points=None, cap_lines=None):
        """The map's edge chains as ordered 3D polylines (rebvio_hip_map_edge_polylines). opts: a PolylineOpts or None for the
        defaults; pose: see _cloud_pose. Returns (points CLOUD_POINT_DTYPE in slot order, refs2 int32 [k, 2] = head, rank per point,
        lines POLYLINE_DTYPE, n_points, n_lines); the caps (default: everything) cut the arrays, never the counts."""
        return _polylines_call(lib().rebvio_hip_map_edge_polylines, (self.h,), self.ctx.p.keylines_max, opts, pose, cap_points, cap_lines)

    def edge_segments(self, opts=None, pose=None, cap=None):
        """The map's polylines split into straight 3D segments with fitted end depths (rebvio_hip_map_edge_segments). opts: a
        SegmentOpts or None for the defaults; pose: None (identity), a CloudPose, or (R, t, scale). Returns (segments
        LINE_SEGMENT_DTYPE, SegmentCounts); the cap (default: everything) cuts the array, never the counts."""
        return _segments_call(lib().rebvio_hip_map_edge_segments, (self.h,), self.ctx.p.keylines_max, opts, pose, cap)

    def mark_keyframe(self):
        """Makes this map the keyframe: match_id_keyframe[i] = i for every keyline (rebvio_hip_map_mark_keyframe; queued on the track
        stream, returns at once). Mark a map after it has been a pair's new map and before it serves as an old map."""
        _chk(lib().rebvio_hip_map_mark_keyframe(self.ctx.h, self.h))

    def keyframe_matches(self, kf_size: int, cap=None, return_count=False):
        """The keyframe-to-current correspondences of this map as a KF_MATCH_DTYPE array, one record per keyline of the keyframe
        (indices 0..kf_size-1) that a keyline of this map still continues, in ascending kf_keyline (rebvio_hip_map_keyframe_matches).
        cap: at most this many records (default: kf_size); return_count: also the number of such keyframe keylines, which may
        exceed cap."""
        if cap is None:
            cap = max(0, int(kf_size))
        out = np.zeros(cap, KF_MATCH_DTYPE)
        n = C.c_int()
        _chk(lib().rebvio_hip_map_keyframe_matches(self.h, kf_size, out.ctypes.data_as(C.POINTER(KfMatch)) if cap else None, cap,
                                                   C.byref(n)))
        out = out[:min(n.value, cap)]
        return (out, n.value) if return_count else out

    def keyframe_snapshot(self) -> KfSnapshot:
        """Keeps this map's keylines as they are now, in its own camera frame (rebvio_hip_map_keyframe_snapshot; queued on the track
        stream, returns at once). Take it where the map is marked: after it has been a pair's new map, before it is an old one."""
        h = _vp()
        _chk(lib().rebvio_hip_map_keyframe_snapshot(self.ctx.h, self.h, C.byref(h)))
        return KfSnapshot(h)

    def keyframe_pose(self, snap: KfSnapshot, opts=None, R0=None, t0=None) -> KfPose:
        """Pose of this map relative to the keyframe `snap` was taken from, X_cur = R X_kf + t, estimated on the device from the
        keyframe correspondences (rebvio_hip_map_keyframe_pose). opts: a KfPoseOpts or None for the defaults; R0 / t0: the guess
        (None: identity / zero), e.g. the previous result."""
        (kR, pR), (kt, pt) = _guess(R0, 9), _guess(t0, 3)
        out = KfPose()
        _chk(lib().rebvio_hip_map_keyframe_pose(self.h, snap.h, opts, pR, pt, C.byref(out)))
        del kR, kt
        return out

    def keyframe_align(self, snap: KfSnapshot, opts=None, R0=None, t0=None, want_assoc=False):
        """Aligns the keyframe `snap` to this map through this map's distance field, X_cur = R X_kf + t
        (rebvio_hip_map_keyframe_align): no correspondence chain is needed, any detected map of the snapshot's context will do.
        opts: a KfAlignOpts or None for the defaults; R0 / t0: the guess (None: identity / zero). want_assoc: also the int32 array of
        the keyline of this map every keyframe keyline was associated with at the returned pose (-1: none)."""
        (kR, pR), (kt, pt) = _guess(R0, 9), _guess(t0, 3)
        out = KfPose()
        assoc = None
        if want_assoc:
            n = C.c_int()
            _chk(lib().rebvio_hip_kf_snapshot_download(snap.h, None, None, 0, C.byref(n)))
            assoc = np.full(n.value, -1, np.int32)
        _chk(lib().rebvio_hip_map_keyframe_align(self.h, snap.h, opts, pR, pt, C.byref(out),
                                                 assoc.ctypes.data_as(_ip) if want_assoc and len(assoc) else None))
        del kR, kt
        return (out, assoc) if want_assoc else out

    def keyframe_align_many(self, hyps, opts=None):
        """Aligns every hypothesis of `hyps` (KfHypothesis: kf_hypothesis(snap, R0, t0), kf_hypotheses_around) to this map in one set
        of launches (rebvio_hip_map_keyframe_align_many). Returns a list of KfHypResult whose pose is bit for bit keyframe_align's for
        the same snapshot, guess and options; there are no associations - run keyframe_align on the winner (kf_align_best) for them.
        The snapshots behind the hypotheses must be kept alive by the caller."""
        hyps = list(hyps)
        arr = _hyp_array(hyps, KfHypothesis)
        out = (KfHypResult * max(len(hyps), 1))()
        _chk(lib().rebvio_hip_map_keyframe_align_many(self.h, arr if hyps else None, len(hyps), opts, out))
        return [KfHypResult.from_buffer_copy(out[k]) for k in range(len(hyps))]

    def fuse_depth_image(self, depth, fmt=None, opts=None, device=False, queued=False, pitch=None, want_outcome=False):
        """Folds a registered depth image into this map's (rho, sigma_rho), one Kalman update per keyline (rebvio_hip_map_fuse_depth_image*;
        include/rebvio_hip.h is the definition and says where in a stream it belongs). depth: a host array [rows, cols], uint16
        (DEPTH_U16, counts of opts.unit metres) or float32 (DEPTH_F32, metres) - or, with device=True or queued=True, a device address
        (fmt is then required; pitch in bytes, default dense). Returns the DepthPriorCounts, with want_outcome also the int32 outcome
        word per keyline; queued=True returns None at once: Context.depth_prior_last_counts fetches the counts."""
        if device or queued:
            assert fmt is not None, "a device image needs its format"
            addr, pb = _vp(int(depth)), int(pitch or 0)
            if queued:
                _chk(lib().rebvio_hip_map_fuse_depth_image_async(self.ctx.h, self.h, addr, pb, fmt, opts))
                return None
            entry, keep = lib().rebvio_hip_map_fuse_depth_image_device, None
        else:
            keep, addr, pb, fmt = _depth_image(depth, fmt, self.ctx.rows, self.ctx.cols)
            entry = lib().rebvio_hip_map_fuse_depth_image
        out = DepthPriorCounts()
        outcome = np.zeros(self.ctx.p.keylines_max, np.int32) if want_outcome else None
        _chk(entry(self.h, addr, pb, fmt, opts, C.byref(out), outcome.ctypes.data_as(_ip) if want_outcome else None))
        del keep
        return (out, outcome[:out.candidates]) if want_outcome else out

    def set_mask(self, mask: np.ndarray):
        """Test hook: overwrite the dense mask (rebvio_hip_test_map_set_mask), for a right map planted by hand."""
        mask = np.ascontiguousarray(mask, np.int32)
        assert mask.size == self.ctx.rows * self.ctx.cols, mask.shape
        _chk(lib().rebvio_hip_test_map_set_mask(self.h, mask.ctypes.data))

    def fuse_stereo(self, right, opts, queued=False, want_outcome=False):
        """Folds the disparities found in `right`, the edge map of the rectified right image of the same instant (a Map of this
        context or of another one on the same device), into this map's (rho, sigma_rho) (rebvio_hip_map_fuse_stereo*;
        include/rebvio_hip.h is the definition and says where in a stream it belongs). Returns the StereoPriorCounts, with
        want_outcome also the int32 outcome and winner words per keyline; queued=True returns None at once:
        Context.stereo_prior_last_counts fetches the counts, and `right` stays unreleased until then."""
        rh = right.h if right is not None else None
        if queued:
            _chk(lib().rebvio_hip_map_fuse_stereo_async(self.ctx.h, self.h, rh, opts))
            return None
        out = StereoPriorCounts()
        kmax = self.ctx.p.keylines_max
        outcome = np.zeros(kmax, np.int32) if want_outcome else None
        winner = np.zeros(kmax, np.int32) if want_outcome else None
        _chk(lib().rebvio_hip_map_fuse_stereo(self.h, rh, opts, C.byref(out), outcome.ctypes.data_as(_ip) if want_outcome else None,
                                              winner.ctypes.data_as(_ip) if want_outcome else None))
        return (out, outcome[:out.candidates], winner[:out.candidates]) if want_outcome else out

    def place_signature(self):
        """(sig uint16 [384], counted): this map's edge signature, 8 x 6 image cells x 8 orientation bins over the keylines it holds
        now (rebvio_hip_map_place_signature; synchronous). Take it where the map is marked, as the snapshot."""
        sig = np.zeros(PLACE_WORDS, np.uint16)
        n = C.c_int()
        _chk(lib().rebvio_hip_map_place_signature(self.h, sig.ctypes.data, C.byref(n)))
        return sig, n.value

    def upload(self, kl: np.ndarray):
        kl = np.ascontiguousarray(kl, KEYLINE_DTYPE)
        _chk(lib().rebvio_hip_map_upload(self.h, kl.ctypes.data if kl.size else None, len(kl)))


class Context:
    def __init__(self, params: Params, _handle=None):
        self.p = params
        self.rows, self.cols = params.rows, params.cols
        self._owned = _handle is None
        if _handle is None:
            h = _vp()
            _chk(lib().rebvio_hip_create(C.byref(params), C.byref(h)))
        else:
            h = _vp(_handle)
        self.h = h
        self._dev_bufs = []

    def close(self):
        if getattr(self, "h", None):
            for b in self._dev_bufs:
                lib().rebvio_hip_device_free(self.h, b)
            self._dev_bufs = []
            if self._owned:
                lib().rebvio_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # detection
    def scale_space(self, img):
        img, pi = _f(img)
        outs = [np.empty((self.rows, self.cols), np.float32) for _ in range(4)]
        _chk(lib().rebvio_hip_scale_space(self.h, pi, *[o.ctypes.data_as(_fp) for o in outs]))
        return dict(scale0=outs[0], scale1=outs[1], dog=outs[2], mag=outs[3])

    def smooth(self, img, widths):
        """FastGaussian::smooth with the given box widths (three for the reference's own filters, any count for its general n)."""
        img, pi = _f(img)
        n = len(widths)
        w = (C.c_int * n)(*[int(v) for v in widths])
        out = np.empty((self.rows, self.cols), np.float32)
        if n == 3:
            _chk(lib().rebvio_hip_smooth(self.h, pi, w, out.ctypes.data_as(_fp)))
        else:
            _chk(lib().rebvio_hip_smooth_n(self.h, pi, w, n, out.ctypes.data_as(_fp)))
        return out

    def detect(self, img, ts_us=0) -> Map:
        img, pi = _f(img)
        assert img.shape == (self.rows, self.cols)
        h = _vp()
        _chk(lib().rebvio_hip_detect(self.h, pi, 0, ts_us, C.byref(h)))
        return Map(self, h)

    def detect_u8(self, frame_u8, ts_us=0) -> Map:
        return self.detect(frame_u8.astype(np.float32) * np.float32(3.0), ts_us)

    def detect_u8_host(self, frame_u8, ts_us=0) -> Map:
        """u8 host frame through the device front end (x3, undistort when a lens model is set)."""
        frame_u8 = np.ascontiguousarray(frame_u8, np.uint8)
        assert frame_u8.shape == (self.rows, self.cols)
        h = _vp()
        _chk(lib().rebvio_hip_detect_u8(self.h, frame_u8.ctypes.data_as(_vp), 0, ts_us, C.byref(h)))
        return Map(self, h)

    def set_undistort(self, fx, fy, cx, cy, dist):
        k, pk = _f(np.array([fx, fy, cx, cy], np.float32))
        d, pd = _f(np.array(dist, np.float32))
        assert d.size == 5
        _chk(lib().rebvio_hip_set_undistort(self.h, pk, pd))

    def front_end_u8(self, frame_u8) -> np.ndarray:
        frame_u8 = np.ascontiguousarray(frame_u8, np.uint8)
        assert frame_u8.shape == (self.rows, self.cols)
        out = np.empty((self.rows, self.cols), np.float32)
        _chk(lib().rebvio_hip_front_end_u8(self.h, frame_u8.ctypes.data_as(_vp), out.ctypes.data_as(_fp)))
        return out

    def detect_px(self, frame: np.ndarray, fmt: int, ts_us=0) -> Map:
        """Host frame of pixel format fmt (PX_*, see _px_frame) through the device front end."""
        ptr, pitch = _px_frame(frame, fmt, self.rows, self.cols)
        h = _vp()
        _chk(lib().rebvio_hip_detect_px(self.h, ptr, pitch, fmt, ts_us, C.byref(h)))
        return Map(self, h)

    def detect_px_device(self, dev_addr: int, fmt: int, ts_us=0) -> Map:
        h = _vp()
        _chk(lib().rebvio_hip_detect_px_device(self.h, _vp(dev_addr), fmt, ts_us, C.byref(h)))
        return Map(self, h)

    def set_detection_mask(self, mask):
        """Static detection mask (rebvio_hip_set_detection_mask): a 2-D array of shape (rows, cols), any dtype, non-zero = "keylines
        may come from here"; None clears it. Applies from the next frame on."""
        if mask is None:
            _chk(lib().rebvio_hip_set_detection_mask(self.h, None, 0))
            return
        if hasattr(mask, "detach"):  # a torch tensor, wherever it lives
            mask = mask.detach().cpu().numpy()
        mask = np.asarray(mask)
        if mask.shape != (self.rows, self.cols):
            raise ValueError(f"set_detection_mask: shape {mask.shape}, expected ({self.rows}, {self.cols})")
        m = np.ascontiguousarray(mask != 0, np.uint8)
        _chk(lib().rebvio_hip_set_detection_mask(self.h, _vp(m.ctypes.data), self.cols))

    def _frame_addr(self, frame, fmt: int) -> int:
        return _dev_addr(frame, self.rows * self.cols * PX_BPP[fmt] if 0 <= fmt < len(PX_BPP) else 0, self.p.device_id, "frame")

    def detect_px_masked_device(self, frame, fmt: int, mask, ts_us=0) -> Map:
        """detect_px_device with a per-frame detection mask; frame and mask: device addresses or torch CUDA tensors (uint8 frame,
        uint8 / bool (rows, cols) mask)."""
        fa = self._frame_addr(frame, fmt)
        ma = _mask_addr(mask, self.rows, self.cols, self.p.device_id, "detect_px_masked_device")
        h = _vp()
        _chk(lib().rebvio_hip_detect_px_masked_device(self.h, _vp(fa), fmt, _vp(ma), ts_us, C.byref(h)))
        return Map(self, h)

    def front_end_px(self, frame: np.ndarray, fmt: int) -> np.ndarray:
        ptr, pitch = _px_frame(frame, fmt, self.rows, self.cols)
        out = np.empty((self.rows, self.cols), np.float32)
        _chk(lib().rebvio_hip_front_end_px(self.h, ptr, pitch, fmt, out.ctypes.data_as(_fp)))
        return out

    def upload_frames(self, frames_u8: np.ndarray) -> int:
        """Stage u8 frames in HBM; returns the device address of frame 0."""
        frames_u8 = np.ascontiguousarray(frames_u8, np.uint8)
        d = _vp()
        _chk(lib().rebvio_hip_device_alloc(self.h, frames_u8.nbytes, C.byref(d)))
        _chk(lib().rebvio_hip_device_upload(self.h, d, frames_u8.ctypes.data, frames_u8.nbytes))
        self._dev_bufs.append(d)
        return d.value

    def upload_bytes(self, arr: np.ndarray) -> int:
        """Stage any array's bytes in HBM (e.g. depth images for Map.fuse_depth_image); returns the device address."""
        arr = np.ascontiguousarray(arr)
        return self.upload_frames(arr.view(np.uint8).reshape(-1))

    def depth_prior_last_counts(self) -> DepthPriorCounts:
        """The counts of the context's most recent depth-image fusion, queued ones included; waits for them
        (rebvio_hip_depth_prior_last_counts). All zero before the first."""
        out = DepthPriorCounts()
        _chk(lib().rebvio_hip_depth_prior_last_counts(self.h, C.byref(out)))
        return out

    def stereo_prior_last_counts(self) -> StereoPriorCounts:
        """The counts of the context's most recent stereo fusion, queued ones included; waits for them
        (rebvio_hip_stereo_prior_last_counts). All zero before the first."""
        out = StereoPriorCounts()
        _chk(lib().rebvio_hip_stereo_prior_last_counts(self.h, C.byref(out)))
        return out

    def place_db(self, cap: int) -> PlaceDb:
        """A place database of `cap` rows (1..65536) on this context's device (rebvio_hip_place_db_create)"""
        h = _vp()
        _chk(lib().rebvio_hip_place_db_create(self.h, int(cap), C.byref(h)))
        return PlaceDb(h, int(cap))

    def detect_u8_device(self, dev_addr: int, ts_us=0) -> Map:
        h = _vp()
        _chk(lib().rebvio_hip_detect_u8_device(self.h, _vp(dev_addr), ts_us, C.byref(h)))
        return Map(self, h)

    def detector_state(self):
        t, a, n = C.c_float(), C.c_float(), C.c_int()
        _chk(lib().rebvio_hip_detector_state(self.h, C.byref(t), C.byref(a), C.byref(n)))
        return t.value, a.value, n.value

    # tracking
    def build_distance_field(self, m: Map):
        _chk(lib().rebvio_hip_build_distance_field(self.h, m.h))

    def distance_field(self):
        ids = np.empty((self.rows, self.cols), np.int32)
        dist = np.empty((self.rows, self.cols), np.int32)
        _chk(lib().rebvio_hip_distance_field(self.h, ids.ctypes.data_as(_ip), dist.ctypes.data_as(_ip)))
        return ids, dist

    def rotate(self, m: Map, R):
        R, pr = _f(np.asarray(R).reshape(9))
        _chk(lib().rebvio_hip_rotate(self.h, m.h, pr))

    def quantile(self, m: Map, pct=0.9, bins=100):
        out = C.c_float()
        _chk(lib().rebvio_hip_quantile(self.h, m.h, pct, bins, C.byref(out)))
        return out.value

    def try_vel(self, m: Map, vel, sigma_rho_min, residuals):
        vel, pv = _f(vel)
        assert residuals.dtype == np.float32 and residuals.flags.c_contiguous
        out = np.zeros(10, np.float32)
        _chk(lib().rebvio_hip_try_vel(self.h, m.h, pv, sigma_rho_min, residuals.ctypes.data_as(_fp), out.ctypes.data_as(_fp)))
        J = np.array([[out[1], out[4], out[5]], [out[4], out[2], out[6]], [out[5], out[6], out[3]]], np.float32)
        return float(out[0]), J, out[7:10].copy()

    def minimize_vel(self, m: Map, vel0=(0, 0, 0)):
        vel = np.array(vel0, np.float32)
        Rvel = np.zeros(9, np.float32)
        F, srm, mask = C.c_float(), C.c_float(), C.c_int()
        _chk(lib().rebvio_hip_minimize_vel(self.h, m.h, vel.ctypes.data_as(_fp), Rvel.ctypes.data_as(_fp), C.byref(F),
                                           C.byref(mask), C.byref(srm)))
        return dict(F=F.value, vel=vel, Rvel=Rvel.reshape(3, 3), accept_mask=mask.value, sigma_rho_min=srm.value)

    def forward_match(self, old: Map, new: Map):
        _chk(lib().rebvio_hip_forward_match(self.h, old.h, new.h))

    def ext_rot_vel(self, vel):
        vel, pv = _f(vel)
        Wx = np.zeros(36, np.float32)
        JtF = np.zeros(6, np.float32)
        X = np.zeros(6, np.float32)
        ok = C.c_int()
        _chk(lib().rebvio_hip_ext_rot_vel(self.h, pv, Wx.ctypes.data_as(_fp), JtF.ctypes.data_as(_fp), X.ctypes.data_as(_fp),
                                          C.byref(ok)))
        return dict(ok=ok.value, Wx=Wx.reshape(6, 6), X=X, JtF=JtF)

    def directed_match(self, new: Map, old: Map, vel, Rvel, Rback, max_radius=40.0):
        vel, pv = _f(vel)
        Rvel, prv = _f(np.asarray(Rvel).reshape(9))
        Rback, prb = _f(np.asarray(Rback).reshape(9))
        n, kf = C.c_int(), C.c_int()
        _chk(lib().rebvio_hip_directed_match(self.h, new.h, old.h, pv, prv, prb, max_radius, C.byref(n), C.byref(kf)))
        return n.value, kf.value

    def regularize(self, m: Map):
        n = C.c_int()
        _chk(lib().rebvio_hip_regularize(self.h, m.h, C.byref(n)))
        return n.value

    def update_inverse_depth(self, vel):
        vel, pv = _f(vel)
        _chk(lib().rebvio_hip_update_inverse_depth(self.h, pv))

    def reset_state(self):
        lib().rebvio_hip_reset_state(self.h)

    def gyro_state(self):
        """(Bg[3], W_Bg[3, 3]) of the pair glue's gyro-bias filter (types/imu.hpp:180-182)."""
        bg = np.zeros(3, np.float32)
        w = np.zeros(9, np.float32)
        _chk(lib().rebvio_hip_get_gyro_state(self.h, bg.ctypes.data_as(_fp), w.ctypes.data_as(_fp)))
        return bg, w.reshape(3, 3)

    def set_gyro_state(self, bg, w_bg):
        bg, pb = _f(np.asarray(bg).reshape(3))
        w, pw = _f(np.asarray(w_bg).reshape(9))
        _chk(lib().rebvio_hip_set_gyro_state(self.h, pb, pw))

    def track_pair(self, old: Map, new: Map, R_prior=None, frame_dt=0.05) -> PairOut:
        out = PairOut()
        pr = None
        if R_prior is not None:
            R_prior, pr = _f(np.asarray(R_prior).reshape(9))
        _chk(lib().rebvio_hip_track_pair(self.h, old.h, new.h, pr, frame_dt, C.byref(out)))
        return out

    # the pair step in two halves (what rebvio::Rebvio drives, with the host's inertial fusion in between)
    def track_pair_begin(self, old: Map, new: Map, R_prior=None, frame_dt=0.05) -> PairMid:
        mid = PairMid()
        pr = None
        if R_prior is not None:
            R_prior, pr = _f(np.asarray(R_prior).reshape(9))
        _chk(lib().rebvio_hip_track_pair_begin(self.h, old.h, new.h, pr, frame_dt, C.byref(mid)))
        return mid

    def track_pair_finish_async(self, old: Map, new: Map, V, P_V, Rgva, R_second, R_prior_next=None):
        V, pv = _f(V)
        P_V, ppv = _f(np.asarray(P_V).reshape(9))
        Rgva, prg = _f(np.asarray(Rgva).reshape(9))
        R_second, pr2 = _f(np.asarray(R_second).reshape(9))
        prn = None
        if R_prior_next is not None:
            R_prior_next, prn = _f(np.asarray(R_prior_next).reshape(9))
        _chk(lib().rebvio_hip_track_pair_finish_async(self.h, old.h, new.h, pv, ppv, prg, pr2, prn))

    def track_pair_result(self):
        """(klm_num, kf_matches, reg_num, status) of the pair whose _finish_async came last but one / last."""
        v = [C.c_int() for _ in range(4)]
        _chk(lib().rebvio_hip_track_pair_result(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def point_cloud_async(self, m: Map, filter=None, pose=None) -> Cloud:
        """Queues the extraction of m's point cloud on the track stream and returns at once (allowed between
        track_pair_finish_async(k) and track_pair_begin(k+1))."""
        h = _vp()
        _chk(lib().rebvio_hip_map_point_cloud_async(self.h, m.h, _cloud_filter(filter), _cloud_pose(pose), C.byref(h)))
        return Cloud(h)

    def track_pair_hint_next(self, next_new: Map):
        _chk(lib().rebvio_hip_track_pair_hint_next(self.h, next_new.h))

    def push_frame_u8_device(self, dev_addr: int, ts_us: int):
        out = PairOut()
        n = C.c_int()
        _chk(lib().rebvio_hip_push_frame_u8_device(self.h, _vp(dev_addr), ts_us, C.byref(out), C.byref(n)))
        return out, n.value

    def push_frame_u8(self, frame_u8: np.ndarray, ts_us: int):
        """Streaming push of a MONO8 frame in host memory (rows x cols, C-contiguous rows; a row pitch is taken from the array)."""
        assert frame_u8.dtype == np.uint8 and frame_u8.shape == (self.rows, self.cols) and frame_u8.strides[1] == 1
        out = PairOut()
        n = C.c_int()
        _chk(lib().rebvio_hip_push_frame_u8(self.h, _vp(frame_u8.ctypes.data), frame_u8.strides[0], ts_us, C.byref(out), C.byref(n)))
        return out, n.value

    def push_frame_px(self, frame: np.ndarray, fmt: int, ts_us: int):
        """Streaming push of a host frame of pixel format fmt (PX_*, see _px_frame)."""
        ptr, pitch = _px_frame(frame, fmt, self.rows, self.cols)
        out = PairOut()
        n = C.c_int()
        _chk(lib().rebvio_hip_push_frame_px(self.h, ptr, pitch, fmt, ts_us, C.byref(out), C.byref(n)))
        return out, n.value

    def push_frame_px_device(self, dev_addr: int, fmt: int, ts_us: int):
        out = PairOut()
        n = C.c_int()
        _chk(lib().rebvio_hip_push_frame_px_device(self.h, _vp(dev_addr), fmt, ts_us, C.byref(out), C.byref(n)))
        return out, n.value

    def push_frame_px_masked_device(self, frame, fmt: int, mask, ts_us: int):
        """push_frame_px_device with a per-frame detection mask (device addresses or torch CUDA tensors, see detect_px_masked_device)."""
        fa = self._frame_addr(frame, fmt)
        ma = _mask_addr(mask, self.rows, self.cols, self.p.device_id, "push_frame_px_masked_device")
        out = PairOut()
        n = C.c_int()
        _chk(lib().rebvio_hip_push_frame_px_masked_device(self.h, _vp(fa), fmt, _vp(ma), ts_us, C.byref(out), C.byref(n)))
        return out, n.value

    def push_frame_px_gyro_device(self, frame, fmt: int, R_gyro=None, mask=None, ts_us: int = 0):
        """push_frame_px_device with the gyro rotation over the interval from the previously pushed frame to this one (3x3 or 9
        floats, row-major; None: identity) and an optional per-frame detection mask; frame / mask: device addresses or torch CUDA
        tensors. The pair that ends at this frame equals track_pair(..., R_prior=R_gyro)."""
        fa = self._frame_addr(frame, fmt)
        ma = None if mask is None else _vp(_mask_addr(mask, self.rows, self.cols, self.p.device_id, "push_frame_px_gyro_device"))
        _keep, pr = _gyro(R_gyro)
        out = PairOut()
        n = C.c_int()
        _chk(lib().rebvio_hip_push_frame_px_gyro_device(self.h, _vp(fa), fmt, ma, pr, ts_us, C.byref(out), C.byref(n)))
        return out, n.value

    def push_frame_px_gyro(self, frame: np.ndarray, fmt: int, R_gyro, ts_us: int):
        """push_frame_px (host frame of pixel format fmt) with a gyro rotation (see push_frame_px_gyro_device)."""
        ptr, pitch = _px_frame(frame, fmt, self.rows, self.cols)
        _keep, pr = _gyro(R_gyro)
        out = PairOut()
        n = C.c_int()
        _chk(lib().rebvio_hip_push_frame_px_gyro(self.h, ptr, pitch, fmt, pr, ts_us, C.byref(out), C.byref(n)))
        return out, n.value

    def test_glue(self, vel, JtJ6, F, sigma_rho_min, accept_mask, xrv, n_new, frame_dt, Bg, W_Bg, R_prior):
        """The pair glue on the device and on the host from the same inputs: ((out, state[22], second[44 words]) per side)."""
        vel, pv = _f(vel)
        JtJ6, pj = _f(JtJ6)
        xrv, px = _f(np.asarray(xrv, np.float32).reshape(-1))
        Bg, pb = _f(Bg)
        W_Bg, pw = _f(np.asarray(W_Bg).reshape(9))
        R_prior, pr = _f(np.asarray(R_prior).reshape(9))
        res = []
        outs = [PairOut(), PairOut()]
        sts = [np.zeros(22, np.float32) for _ in range(2)]
        sec = [np.zeros(44, np.float32) for _ in range(2)]
        _chk(lib().rebvio_hip_test_glue(self.h, pv, pj, F, sigma_rho_min, accept_mask, px, n_new, frame_dt, pb, pw, pr,
                                        C.byref(outs[0]), sts[0].ctypes.data_as(_fp), sec[0].ctypes.data_as(_fp),
                                        C.byref(outs[1]), sts[1].ctypes.data_as(_fp), sec[1].ctypes.data_as(_fp)))
        for i in range(2):
            res.append((outs[i], sts[i], sec[i]))
        return res

    def test_glue_set_next(self, R_next=None, has_next=True):
        """The next pair's gyro rotation (None: identity) and whether it is known, for the test_glue calls that follow."""
        _keep, pr = _gyro(R_next)
        _chk(lib().rebvio_hip_test_glue_set_next(self.h, pr, 1 if has_next else 0))

    def pairs_started(self) -> int:
        """Frame pairs the streaming driver has queued on the device so far."""
        return int(lib().rebvio_hip_pairs_started(self.h))

    def handover_counters(self) -> dict:
        """The streaming driver's hand-over counters since the context was created (rebvio_hip_test_handover_counters): per stream
        ("track", "scan", "keyline") a dict of waits "queued", waits "skipped" and "events" recorded, and "reuse_fallbacks"."""
        v = (C.c_ulonglong * 10)()
        _chk(lib().rebvio_hip_test_handover_counters(self.h, v))
        d = {s: dict(queued=int(v[3 * i]), skipped=int(v[3 * i + 1]), events=int(v[3 * i + 2]))
             for i, s in enumerate(("track", "scan", "keyline"))}
        d["reuse_fallbacks"] = int(v[9])
        return d

    def keyframe_next(self):
        """The next frame pushed becomes a keyframe (rebvio_hip_keyframe_next): its map is marked between the pair that ends at it
        and the pair that starts from it."""
        _chk(lib().rebvio_hip_keyframe_next(self.h))

    def next_record(self):
        """The oldest complete pair record not handed out yet, or None."""
        out = PairOut()
        n = C.c_int()
        k = lib().rebvio_hip_next_record(self.h, C.byref(out), C.byref(n))
        if k < 0:
            _chk(k)
        return (out, n.value) if k == 1 else None

    def flush(self):
        """Finishes every pair in flight; returns the records that were still waiting to be handed out, oldest first."""
        _chk(lib().rebvio_hip_flush(self.h))
        rest = []
        while True:
            r = self.next_record()
            if r is None:
                return rest
            rest.append(r)

    # profiling
    def profile(self, on: bool, only: str | None = None, stride: int = 1):
        lib().rebvio_hip_profile_select(self.h, (only or "").encode())
        lib().rebvio_hip_profile_enable(self.h, (max(1, stride) if on else 0))

    def profile_reset(self):
        lib().rebvio_hip_profile_reset(self.h)

    def profile_read(self):
        cap = 128
        names = C.create_string_buffer(16384)
        avg = (C.c_double * cap)()
        calls = (C.c_int * cap)()
        k = lib().rebvio_hip_profile_read(self.h, names, 16384, avg, calls, cap)
        ns = names.value.decode().split("\n")
        return {ns[i]: (avg[i], calls[i]) for i in range(k)}


class Batch:
    """`lanes` camera streams of one GPU advanced in lock-step (rebvio_hip_batch_*)."""

    def __init__(self, params: Params, lanes: int):
        self.p, self.B = params, lanes
        h = _vp()
        _chk(lib().rebvio_hip_batch_create(C.byref(params), lanes, C.byref(h)))
        self.h = h
        self.lanes = [Context(params, _handle=lib().rebvio_hip_batch_lane(h, l)) for l in range(lanes)]
        self._frames = (_vp * lanes)()
        self._masks = (_vp * lanes)()
        self._out = (PairOut * lanes)()
        self._n = (C.c_int * lanes)()

    def push_u8_device(self, dev_addrs, ts_us: int):
        for l, a in enumerate(dev_addrs):
            self._frames[l] = int(a)
        _chk(lib().rebvio_hip_batch_push_u8_device(self.h, self._frames, ts_us, self._out, self._n))
        return self._out, self._n

    def push_px_device(self, dev_addrs, fmt: int, ts_us: int):
        for l, a in enumerate(dev_addrs):
            self._frames[l] = int(a)
        _chk(lib().rebvio_hip_batch_push_px_device(self.h, self._frames, fmt, ts_us, self._out, self._n))
        return self._out, self._n

    def push_px_masked_device(self, frames, fmt: int, masks, ts_us: int):
        """push_px_device with a per-frame detection mask per lane: masks[l] is a device address, a torch CUDA tensor or None (no
        per-frame mask for lane l); frames[l] a device address or a torch CUDA tensor."""
        rows, cols, dev = self.p.rows, self.p.cols, self.p.device_id
        for l in range(self.B):
            self._frames[l] = self.lanes[l]._frame_addr(frames[l], fmt)
            self._masks[l] = None if masks[l] is None else _mask_addr(masks[l], rows, cols, dev, "batch push_px_masked_device")
        _chk(lib().rebvio_hip_batch_push_px_masked_device(self.h, self._frames, fmt, self._masks, ts_us, self._out, self._n))
        return self._out, self._n

    def push_px_gyro_device(self, frames, fmt: int, R_gyros, masks=None, ts_us: int = 0):
        """push_px_device with a gyro rotation per lane (R_gyros: None, or one entry per lane, each 3x3 / 9 floats or None for
        the identity) and optional per-frame masks (as push_px_masked_device)."""
        rows, cols, dev = self.p.rows, self.p.cols, self.p.device_id
        keep = []
        rot = None
        if R_gyros is not None:
            rot = (_fp * self.B)()
            for l in range(self.B):
                a, ptr = _gyro(R_gyros[l])
                keep.append(a)
                if ptr is not None:
                    rot[l] = ptr
        for l in range(self.B):
            self._frames[l] = self.lanes[l]._frame_addr(frames[l], fmt)
            if masks is not None:
                self._masks[l] = None if masks[l] is None else _mask_addr(masks[l], rows, cols, dev, "batch push_px_gyro_device")
        _chk(lib().rebvio_hip_batch_push_px_gyro_device(self.h, self._frames, fmt, self._masks if masks is not None else None, rot, ts_us,
                                                        self._out, self._n))
        return self._out, self._n

    def flush(self):
        """Finishes every step in flight; returns the steps' records that were still waiting, oldest first, as
        (list of PairOut per lane, list of keyline counts per lane)."""
        _chk(lib().rebvio_hip_batch_flush(self.h))
        rest = []
        while True:
            out = (PairOut * self.B)()
            n = (C.c_int * self.B)()
            k = lib().rebvio_hip_batch_next_records(self.h, out, n)
            if k < 0:
                _chk(k)
            if k != 1:
                return rest
            rest.append((list(out), list(n)))

    def close(self):
        if getattr(self, "h", None):
            for c in self.lanes:
                c.close()  # frees the frames staged through the lane; the lane itself belongs to the batch
            lib().rebvio_hip_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
