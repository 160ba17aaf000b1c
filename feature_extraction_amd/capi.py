"""ctypes binding of include/fx.h (libfx_hip.so).

Plumbing for tests/ and bench.py only: the product is the C-ABI library and the C++ host
classes above it (csrc/fx_node.hpp).  Loading fails loudly when the library is missing —
there is no Python/CPU fallback for the hot path.
"""
import contextlib
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfx_hip.so")

FX_DESC_BINS = 1980
FX_DESC_RF = 9
FX_DESC_FLOATS = 1989
FX_FEATURE_RECORD_BYTES = 7984
FX_OK = 0
FX_ERR_NO_DEVICE = 2
FX_ERR_INVALID_ARG, FX_ERR_TOO_LARGE = 1, 5
FX_IN_DEVICE, FX_OUT_HOST, FX_OUT_DEBUG, FX_OUT_CLOUDS = 1, 2, 4, 8
FX_OUT_DESC_CSR = 0x10  # with FX_OUT_HOST: the descriptor rows come back as the context's CSR block (fx_get_descriptors_csr)
FX_FLAG_RING_OVERFLOW, FX_FLAG_CAND_OVERFLOW, FX_FLAG_KP_OVERFLOW, FX_FLAG_NBR_OVERFLOW = 0x1, 0x2, 0x4, 0x8
FX_FLAG_NAMES = {0x1: "RING_OVERFLOW", 0x2: "CAND_OVERFLOW", 0x4: "KP_OVERFLOW", 0x8: "NBR_OVERFLOW",
                 0x10: "TOTAL_KP_OVERFLOW", 0x20: "KPC_OVERFLOW"}
FX_N_STAGES = 9
STAGE_NAMES = ("k_prep", "k_bucket", "k_rings_runs", "k_rings_large", "k_merge", "k_gather", "k_desc_group", "k_desc_mid",
               "k_desc_rare")
# stages that are one kernel launch (eligible as the roofline line's dominant kernel: their HIP-event span is that kernel)
SINGLE_LAUNCH_STAGES = ("k_prep", "k_bucket", "k_rings_runs", "k_gather", "k_desc_group")
# kernels launched inside each timed stage (rocprofv3 / PMC rows are per kernel name)
STAGE_KERNELS = {"k_prep": ("k_prep", "k_front", "k_front_ab"),  # (k_front: stages 0-4 of scans that fit its LDS tables, in one launch)
                 "k_bucket": ("k_bucket", "k_bucket_many"),  # (k_bucket_many: sensors of more than 24 rings)
                 "k_rings_large": ("k_rings_runs2", "k_rings_large"),  # (k_rings_runs2: sensors of more than 16 rings)
                 "k_merge": ("k_merge_small", "k_merge_big", "k_merge_huge", "k_front_redo", "k_slow"),
                 "k_desc_group": ("k_desc",),  # (every descriptor tier but the dense tier's own kernels, in one launch)
                 "k_desc_mid": (),  # (the slot brackets nothing since k_desc took its rows)
                 "k_gather": ("k_gather", "k_rng_ord"),  # (k_rng_ord only when several workgroups share a scan: small batches)
                 "k_desc_rare": ("k_dense_sort", "k_dense_density", "k_dense_finish")}


class FxParams(C.Structure):
    _fields_ = [("cloud_leveling", C.c_int32),
                ("x_min", C.c_double), ("x_max", C.c_double),
                ("y_min", C.c_double), ("y_max", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double),
                ("cluster_tolerance", C.c_double),
                ("cluster_min_count", C.c_int32), ("cluster_max_count", C.c_int32),
                ("cluster_radius_threshold", C.c_double),
                ("number_detection_channels", C.c_int32),
                ("estimate_descriptors", C.c_int32),
                ("descriptor_radius", C.c_double),
                ("n_rings", C.c_int32), ("el0_deg", C.c_double), ("el_step_deg", C.c_double),
                ("secondary_max", C.c_int32)]


class FxLimits(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in
                ("max_batch", "max_points", "max_ring_points", "max_ring_candidates", "max_candidates",
                 "max_keypoints", "max_neighbors", "max_total_keypoints", "max_kpc_points", "max_dense_points", "max_overflow_points")]


class FxScanDesc(C.Structure):
    _fields_ = [("points", C.c_void_p), ("n_points", C.c_uint32), ("stride_bytes", C.c_uint32),
                ("roll", C.c_double), ("pitch", C.c_double)]


_U32P, _F32P, _I32P = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_int32)


class FxBatchView(C.Structure):
    _fields_ = [("batch", C.c_uint32), ("max_points", C.c_uint32), ("max_keypoints", C.c_uint32),
                ("max_candidates", C.c_uint32), ("max_kpc_points", C.c_uint32), ("total_keypoints", C.c_uint32),
                ("d_n_keypoints", C.c_void_p), ("d_kp_offset", C.c_void_p), ("d_keypoints", C.c_void_p),
                ("d_descriptors", C.c_void_p), ("d_flags", C.c_void_p), ("d_n_filtered", C.c_void_p),
                ("d_filtered", C.c_void_p), ("d_n_kpc", C.c_void_p), ("d_kpc", C.c_void_p),
                ("h_n_keypoints", _U32P), ("h_kp_offset", _U32P), ("h_keypoints", _F32P),
                ("h_descriptors", _F32P), ("h_flags", _U32P), ("h_n_filtered", _U32P), ("h_filtered", _F32P),
                ("h_n_kpc", _U32P), ("h_kpc", _F32P),
                ("h_n_candidates", _U32P), ("h_candidates", _F32P), ("h_cand_size", _U32P),
                ("h_cand_keypoint", _I32P), ("h_kpc_cand", _U32P), ("h_kp_size", _U32P),
                ("h_kp_neighbors", _U32P)]


class FxPc2Layout(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in
                ("point_step", "offset_x", "offset_y", "offset_z", "offset_intensity", "is_bigendian")]


class FxDescriptorCsrView(C.Structure):
    _fields_ = [("rows", C.c_uint32), ("nnz", C.c_uint32), ("h_row_ptr", _U32P), ("h_col", _U32P), ("h_val", _F32P),
                ("d_row_ptr", C.c_void_p), ("d_col", C.c_void_p), ("d_val", C.c_void_p)]


class FxMatchPair(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("q_row0", "q_rows", "t_row0", "t_rows")]


class FxMatchOptions(C.Structure):
    _fields_ = [("azimuth_shifts", C.c_uint32), ("max_dist2", C.c_float), ("max_ratio", C.c_float), ("mutual", C.c_uint32)]


class FxMatch(C.Structure):
    _fields_ = [("train_row", C.c_int32), ("shift", C.c_uint32), ("dist2", C.c_float), ("second_row", C.c_int32),
                ("dist2_second", C.c_float), ("flags", C.c_uint32), ("pair", C.c_uint32), ("reserved", C.c_uint32)]


FX_MATCH_ACCEPTED, FX_MATCH_MUTUAL = 0x1, 0x2
FX_MATCH_NO_PAIR = 0xffffffff
FX_MATCH_SECTOR = 165  # bins of one azimuth sector: a rotation by s sectors shifts the bin index by 165 s
# fx_match as a numpy record (match_records)
MATCH_DTYPE = np.dtype([("train_row", "<i4"), ("shift", "<u4"), ("dist2", "<f4"), ("second_row", "<i4"), ("dist2_second", "<f4"),
                        ("flags", "<u4"), ("pair", "<u4"), ("reserved", "<u4")])


class FxRegisterOptions(C.Structure):
    _fields_ = [("inlier_dist", C.c_float), ("min_baseline", C.c_float), ("hyp_corr", C.c_uint32), ("min_inliers", C.c_uint32),
                ("require_flags", C.c_uint32)]


class FxRegistration(C.Structure):
    _fields_ = [("c", C.c_double), ("s", C.c_double), ("tx", C.c_double), ("ty", C.c_double), ("tz", C.c_double), ("rms", C.c_float),
                ("n_corr", C.c_uint32), ("n_inliers", C.c_uint32), ("flags", C.c_uint32), ("hyp_a", C.c_uint32), ("hyp_b", C.c_uint32)]


FX_REG_VALID, FX_REG_TRUNCATED, FX_REG_NO_HYPOTHESIS = 0x1, 0x2, 0x4
FX_REG_MAX_CORR = 1024
FX_REG_NO_ROW = 0xffffffff
# fx_registration as a numpy record (register_records)
REG_DTYPE = np.dtype([("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("tz", "<f8"), ("rms", "<f4"), ("n_corr", "<u4"),
                      ("n_inliers", "<u4"), ("flags", "<u4"), ("hyp_a", "<u4"), ("hyp_b", "<u4")])
REG_DEFAULTS = dict(inlier_dist=0.30, min_baseline=2.0, hyp_corr=64, min_inliers=3, require_flags=FX_MATCH_ACCEPTED)


class FxPose(C.Structure):
    _fields_ = [("c", C.c_double), ("s", C.c_double), ("tx", C.c_double), ("ty", C.c_double), ("tz", C.c_double),
                ("segment", C.c_uint32), ("flags", C.c_uint32)]


class FxLandmark(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double), ("rms_xy", C.c_float), ("n_obs", C.c_uint32), ("obs0", C.c_uint32),
                ("first_row", C.c_uint32), ("first_scan", C.c_uint32), ("last_scan", C.c_uint32)]


class FxTrackHeader(C.Structure):
    _fields_ = [("scans", C.c_uint32), ("rows", C.c_uint32), ("n_landmarks", C.c_uint32), ("n_obs", C.c_uint32),
                ("n_conflicts", C.c_uint32), ("n_gaps", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class FxTrackOptions(C.Structure):
    _fields_ = [("min_obs", C.c_uint32), ("reserved", C.c_uint32)]


FX_POSE_GAP, FX_POSE_NO_SCAN = 0x1, 0x2
FX_TRACK_NO_ROW = 0xffffffff
# fx_pose / fx_landmark as numpy records (track_records)
POSE_DTYPE = np.dtype([("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("tz", "<f8"), ("segment", "<u4"), ("flags", "<u4")])
LANDMARK_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("rms_xy", "<f4"), ("n_obs", "<u4"), ("obs0", "<u4"),
                           ("first_row", "<u4"), ("first_scan", "<u4"), ("last_scan", "<u4")])
TRACK_HEADER_FIELDS = ("scans", "rows", "n_landmarks", "n_obs", "n_conflicts", "n_gaps")


class FxMapLandmark(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double), ("rms_xy", C.c_float), ("n_obs", C.c_uint32),
                ("first_scan", C.c_uint32), ("last_scan", C.c_uint32), ("segment", C.c_uint32), ("flags", C.c_uint32)]


class FxMapHeader(C.Structure):
    _fields_ = [("n_landmarks", C.c_uint32), ("n_needed", C.c_uint32), ("n_obs", C.c_uint32), ("scans", C.c_uint32),
                ("batches", C.c_uint32), ("segments", C.c_uint32), ("flags", C.c_uint32), ("carry_rows", C.c_uint32),
                ("last_joined", C.c_uint32), ("last_new", C.c_uint32), ("last_pose", FxPose)]


FX_MAP_OVERLAP = 0x1
FX_MAP_FULL, FX_MAP_OVERLAP_MISMATCH, FX_MAP_TRACK_TRUNCATED = 0x1, 0x2, 0x4
FX_MAP_LM_CONTINUED = 0x1
FX_MAP_LM_ABSORBED, FX_MAP_LM_MERGED = 0x2, 0x4  # fx_map_merge: merged into another landmark (see the alias table) / has absorbed one
# fx_map_landmark as numpy records, and the header's counts (map_records)
MAP_LANDMARK_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("rms_xy", "<f4"), ("n_obs", "<u4"), ("first_scan", "<u4"),
                               ("last_scan", "<u4"), ("segment", "<u4"), ("flags", "<u4")])
MAP_HEADER_FIELDS = ("n_landmarks", "n_needed", "n_obs", "scans", "batches", "segments", "flags", "carry_rows", "last_joined", "last_new")


class FxMapMergeOptions(C.Structure):
    _fields_ = [("merge_dist", C.c_float), ("max_gap_scans", C.c_uint32)]


class FxMapMergeResult(C.Structure):
    _fields_ = [("proposals", C.c_uint32), ("merged", C.c_uint32), ("live", C.c_uint32), ("reserved", C.c_uint32)]


MAP_MERGE_RESULT_FIELDS = ("proposals", "merged", "live", "reserved")


class FxMapCompactOptions(C.Structure):
    _fields_ = [("min_obs", C.c_uint32), ("min_age_scans", C.c_uint32)]


class FxMapCompactResult(C.Structure):
    _fields_ = [("before", C.c_uint32), ("kept", C.c_uint32), ("dropped_absorbed", C.c_uint32), ("dropped_live", C.c_uint32)]


MAP_COMPACT_RESULT_FIELDS = ("before", "kept", "dropped_absorbed", "dropped_live")
# the snapshot of a map (include/fx.h fx_map_export_host; map_snapshot_pack is the layout's statement in Python)
FX_MAP_SNAPSHOT_MAGIC, FX_MAP_SNAPSHOT_FORMAT, FX_MAP_SNAPSHOT_HEADER_BYTES, FX_MAP_ACC = 0x504D5846, 1, 64, 8


class FxMapAppendResult(C.Structure):
    _fields_ = [("id_base", C.c_uint32), ("scan_base", C.c_uint32), ("segment_base", C.c_uint32), ("appended", C.c_uint32),
                ("flags", C.c_uint32), ("carry_rows", C.c_uint32), ("reserved", C.c_uint32 * 2)]


FX_APPEND_APPLIED, FX_APPEND_CARRY_DROPPED, FX_APPEND_EMPTY, FX_APPEND_OVERFLOWED, FX_APPEND_NO_ROOM, FX_APPEND_TOO_LONG = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
# fx_map_append_result as a numpy record (append_records)
APPEND_DTYPE = np.dtype([("id_base", "<u4"), ("scan_base", "<u4"), ("segment_base", "<u4"), ("appended", "<u4"), ("flags", "<u4"),
                         ("carry_rows", "<u4"), ("reserved", "<u4", (2,))])


class FxLocalizeOptions(C.Structure):
    _fields_ = [("search_dist", C.c_float), ("inlier_dist", C.c_float), ("min_baseline", C.c_float), ("hyp_corr", C.c_uint32),
                ("min_inliers", C.c_uint32), ("min_landmark_obs", C.c_uint32), ("segment", C.c_uint32), ("reserved", C.c_uint32)]


class FxLocalization(C.Structure):
    _fields_ = [("pose", FxPose), ("dc", C.c_double), ("ds", C.c_double), ("dtx", C.c_double), ("dty", C.c_double), ("dtz", C.c_double),
                ("rms", C.c_float), ("n_corr", C.c_uint32), ("n_inliers", C.c_uint32), ("flags", C.c_uint32), ("hyp_a", C.c_uint32),
                ("hyp_b", C.c_uint32)]


FX_LOC_MAX_CORR = 1024
FX_LOC_ANY_SEGMENT, FX_LOC_LAST_SEGMENT = 0xffffffff, 0xfffffffe
FX_LOC_VALID, FX_LOC_TRUNCATED, FX_LOC_NO_HYPOTHESIS, FX_LOC_BAD_PRIOR, FX_LOC_NO_SCAN = 0x1, 0x2, 0x4, 0x8, 0x10
FX_LOC_NO_ROW = 0xffffffff
# fx_localization as numpy records (localize_records); "pose" is a POSE_DTYPE record
LOC_DTYPE = np.dtype([("pose", POSE_DTYPE), ("dc", "<f8"), ("ds", "<f8"), ("dtx", "<f8"), ("dty", "<f8"), ("dtz", "<f8"), ("rms", "<f4"),
                      ("n_corr", "<u4"), ("n_inliers", "<u4"), ("flags", "<u4"), ("hyp_a", "<u4"), ("hyp_b", "<u4")])
LOC_DEFAULTS = dict(search_dist=2.0, inlier_dist=0.30, min_baseline=2.0, hyp_corr=64, min_inliers=3, min_landmark_obs=2,
                    segment=FX_LOC_LAST_SEGMENT)


class FxMapObserveOptions(C.Structure):
    _fields_ = [("gate_dist", C.c_float), ("require_flags", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32)]


class FxMapObserveResult(C.Structure):
    _fields_ = [("scans_used", C.c_uint32), ("proposed", C.c_uint32), ("added", C.c_uint32), ("duplicates", C.c_uint32), ("gated", C.c_uint32),
                ("stale", C.c_uint32), ("landmarks_touched", C.c_uint32), ("reserved", C.c_uint32)]


FX_MAP_LM_OBSERVED = 0x8  # fx_map_observe: the landmark gained at least one observation through it
FX_OBS_APPLY, FX_OBS_DRY_RUN = 0, 1
MAP_OBSERVE_RESULT_FIELDS = ("scans_used", "proposed", "added", "duplicates", "gated", "stale", "landmarks_touched", "reserved")
OBS_DEFAULTS = dict(gate_dist=0.30, require_flags=FX_LOC_VALID, mode=FX_OBS_APPLY)


class FxMapExpectOptions(C.Structure):
    _fields_ = [("x_min", C.c_float), ("x_max", C.c_float), ("y_min", C.c_float), ("y_max", C.c_float), ("min_range", C.c_float),
                ("max_range", C.c_float), ("shadow_width", C.c_float), ("require_flags", C.c_uint32), ("min_landmark_obs", C.c_uint32),
                ("segment", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32)]


class FxMapExpectResult(C.Structure):
    _fields_ = [("scans_used", C.c_uint32), ("in_range", C.c_uint32), ("in_box", C.c_uint32), ("shadowed", C.c_uint32), ("expected", C.c_uint32),
                ("seen", C.c_uint32), ("stale", C.c_uint32), ("landmarks_expected", C.c_uint32)]


class FxMapRetireOptions(C.Structure):
    _fields_ = [("min_expected", C.c_uint32), ("seen_num", C.c_uint32), ("seen_den", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class FxMapRetireResult(C.Structure):
    _fields_ = [("before", C.c_uint32), ("kept", C.c_uint32), ("dropped_absorbed", C.c_uint32), ("retired", C.c_uint32), ("retired_obs", C.c_uint32),
                ("protected_by_carry", C.c_uint32), ("reserved", C.c_uint32 * 2)]


FX_EXPECT_WRITE, FX_EXPECT_ADD = 0, 1
FX_RETIRE_APPLY, FX_RETIRE_DRY_RUN = 0, 1
MAP_EXPECT_RESULT_FIELDS = ("scans_used", "in_range", "in_box", "shadowed", "expected", "seen", "stale", "landmarks_expected")
MAP_RETIRE_RESULT_FIELDS = ("before", "kept", "dropped_absorbed", "retired", "retired_obs", "protected_by_carry")
EXPECT_DEFAULTS = dict(x_min=1.0, x_max=74.0, y_min=-29.0, y_max=29.0, min_range=2.0, max_range=60.0, shadow_width=0.5,
                       require_flags=FX_LOC_VALID, min_landmark_obs=2, segment=FX_LOC_ANY_SEGMENT, mode=FX_EXPECT_WRITE)
RETIRE_DEFAULTS = dict(min_expected=16, seen_num=1, seen_den=8, mode=FX_RETIRE_APPLY)


class FxMapDiscoverOptions(C.Structure):
    _fields_ = [("known_dist", C.c_float), ("join_dist", C.c_float), ("min_obs", C.c_uint32), ("require_flags", C.c_uint32),
                ("segment", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class FxMapDiscoverResult(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("scans_used", "unmatched", "known", "free_rows", "leaders", "orphans", "duplicates", "weak", "added",
                                          "lost", "created", "not_stored", "first_id", "refused")] + [("reserved", C.c_uint32 * 2)]


FX_MAP_LM_DISCOVERED = 0x10  # fx_map_discover: the landmark was created by it
FX_DISC_APPLY, FX_DISC_DRY_RUN = 0, 1
MAP_DISCOVER_RESULT_FIELDS = ("scans_used", "unmatched", "known", "free_rows", "leaders", "orphans", "duplicates", "weak", "added", "lost",
                              "created", "not_stored", "first_id", "refused")
DISCOVER_DEFAULTS = dict(known_dist=1.0, join_dist=0.30, min_obs=3, require_flags=FX_LOC_VALID, segment=FX_LOC_LAST_SEGMENT, mode=FX_DISC_APPLY)


class FxRelocalizeOptions(C.Structure):
    _fields_ = [("inlier_dist", C.c_float), ("pair_tol", C.c_float), ("min_baseline", C.c_float), ("max_baseline", C.c_float),
                ("max_seeds", C.c_uint32), ("min_inliers", C.c_uint32), ("min_margin", C.c_uint32), ("min_landmark_obs", C.c_uint32),
                ("segment", C.c_uint32), ("reserved", C.c_uint32)]


class FxRelocalization(C.Structure):
    _fields_ = [("pose", FxPose), ("n_hyp", C.c_uint64), ("n_kp", C.c_uint32), ("n_seeds", C.c_uint32), ("score", C.c_uint32),
                ("runner_up", C.c_uint32), ("flags", C.c_uint32), ("seed_a", C.c_uint32), ("seed_b", C.c_uint32), ("lm_a", C.c_uint32),
                ("lm_b", C.c_uint32), ("reserved", C.c_uint32)]


FX_RELOC_MAX_KP = 64
FX_RELOC_VALID, FX_RELOC_TRUNCATED, FX_RELOC_NO_HYPOTHESIS, FX_RELOC_AMBIGUOUS, FX_RELOC_NO_SCAN = 0x1, 0x2, 0x4, 0x8, 0x10
FX_RELOC_NONE = 0xffffffff
# fx_relocalization as numpy records (relocalize_records); "pose" is a POSE_DTYPE record
RELOC_DTYPE = np.dtype([("pose", POSE_DTYPE), ("n_hyp", "<u8"), ("n_kp", "<u4"), ("n_seeds", "<u4"), ("score", "<u4"), ("runner_up", "<u4"),
                        ("flags", "<u4"), ("seed_a", "<u4"), ("seed_b", "<u4"), ("lm_a", "<u4"), ("lm_b", "<u4"), ("reserved", "<u4")])
RELOC_DEFAULTS = dict(inlier_dist=0.30, pair_tol=0.30, min_baseline=2.0, max_baseline=60.0, max_seeds=16, min_inliers=4, min_margin=1,
                      min_landmark_obs=2, segment=FX_LOC_ANY_SEGMENT)


class FxMapJoinOptions(C.Structure):
    _fields_ = [("search_dist", C.c_float), ("inlier_dist", C.c_float), ("min_baseline", C.c_float), ("hyp_corr", C.c_uint32),
                ("min_inliers", C.c_uint32), ("min_landmark_obs", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32)]


class FxMapJoinResult(C.Structure):
    _fields_ = [("c", C.c_double), ("s", C.c_double), ("tx", C.c_double), ("ty", C.c_double), ("tz", C.c_double), ("dc", C.c_double),
                ("ds", C.c_double), ("dtx", C.c_double), ("dty", C.c_double), ("dtz", C.c_double), ("rms", C.c_float), ("n_src", C.c_uint32),
                ("n_corr", C.c_uint32), ("n_inliers", C.c_uint32), ("flags", C.c_uint32), ("moved", C.c_uint32), ("label", C.c_uint32),
                ("segments", C.c_uint32), ("hyp_a", C.c_uint32), ("hyp_b", C.c_uint32)]


FX_JOIN_MAX_CORR = 1024
FX_JOIN_FIT, FX_JOIN_GIVEN, FX_JOIN_DRY_RUN = 0, 1, 2
FX_JOIN_APPLIED, FX_JOIN_TRUNCATED, FX_JOIN_NO_HYPOTHESIS, FX_JOIN_BAD_PRIOR, FX_JOIN_BAD_SEGMENT, FX_JOIN_FITTED = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
FX_JOIN_NONE = 0xffffffff
# fx_map_join_result as a numpy record (join_records)
JOIN_DTYPE = np.dtype([("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("tz", "<f8"), ("dc", "<f8"), ("ds", "<f8"), ("dtx", "<f8"),
                       ("dty", "<f8"), ("dtz", "<f8"), ("rms", "<f4"), ("n_src", "<u4"), ("n_corr", "<u4"), ("n_inliers", "<u4"), ("flags", "<u4"),
                       ("moved", "<u4"), ("label", "<u4"), ("segments", "<u4"), ("hyp_a", "<u4"), ("hyp_b", "<u4")])
JOIN_DEFAULTS = dict(search_dist=2.0, inlier_dist=0.30, min_baseline=2.0, hyp_corr=64, min_inliers=3, min_landmark_obs=2, mode=FX_JOIN_FIT)


class FxMapLoopOptions(C.Structure):
    _fields_ = [("search_dist", C.c_float), ("inlier_dist", C.c_float), ("min_baseline", C.c_float), ("hyp_corr", C.c_uint32),
                ("min_inliers", C.c_uint32), ("min_landmark_obs", C.c_uint32), ("segment", C.c_uint32), ("min_loop_scans", C.c_uint32),
                ("recent_scans", C.c_uint32), ("mode", C.c_uint32), ("loop_first_scan", C.c_uint32), ("loop_last_scan", C.c_uint32),
                ("pivot_x", C.c_double), ("pivot_y", C.c_double), ("reserved", C.c_uint32)]


class FxMapLoopResult(C.Structure):
    _fields_ = [("c", C.c_double), ("s", C.c_double), ("tx", C.c_double), ("ty", C.c_double), ("tz", C.c_double), ("dc", C.c_double),
                ("ds", C.c_double), ("dtx", C.c_double), ("dty", C.c_double), ("dtz", C.c_double), ("px", C.c_double), ("py", C.c_double),
                ("rms", C.c_float), ("n_query", C.c_uint32), ("n_corr", C.c_uint32), ("n_inliers", C.c_uint32), ("flags", C.c_uint32),
                ("moved", C.c_uint32), ("loop_first_scan", C.c_uint32), ("loop_last_scan", C.c_uint32), ("segment", C.c_uint32),
                ("hyp_a", C.c_uint32), ("hyp_b", C.c_uint32), ("reserved", C.c_uint32)]


FX_LOOP_MAX_CORR = 1024
FX_LOOP_FIT, FX_LOOP_GIVEN, FX_LOOP_DRY_RUN = 0, 1, 2
(FX_LOOP_APPLIED, FX_LOOP_TRUNCATED, FX_LOOP_NO_HYPOTHESIS, FX_LOOP_BAD_PRIOR, FX_LOOP_BAD_SEGMENT, FX_LOOP_FITTED,
 FX_LOOP_TOO_FAR) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
FX_LOOP_NONE = 0xffffffff
# fx_map_loop_result as a numpy record (loop_records)
LOOP_DTYPE = np.dtype([("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("tz", "<f8"), ("dc", "<f8"), ("ds", "<f8"), ("dtx", "<f8"),
                       ("dty", "<f8"), ("dtz", "<f8"), ("px", "<f8"), ("py", "<f8"), ("rms", "<f4"), ("n_query", "<u4"), ("n_corr", "<u4"),
                       ("n_inliers", "<u4"), ("flags", "<u4"), ("moved", "<u4"), ("loop_first_scan", "<u4"), ("loop_last_scan", "<u4"),
                       ("segment", "<u4"), ("hyp_a", "<u4"), ("hyp_b", "<u4"), ("reserved", "<u4")])
LOOP_DEFAULTS = dict(search_dist=2.0, inlier_dist=0.30, min_baseline=2.0, hyp_corr=64, min_inliers=3, min_landmark_obs=2,
                     segment=FX_LOC_LAST_SEGMENT, min_loop_scans=256, recent_scans=32, mode=FX_LOOP_FIT, loop_first_scan=0, loop_last_scan=0,
                     pivot_x=0.0, pivot_y=0.0)


class FxMapFindLoopOptions(C.Structure):
    _fields_ = [("inlier_dist", C.c_float), ("pair_tol", C.c_float), ("min_baseline", C.c_float), ("max_baseline", C.c_float),
                ("max_seeds", C.c_uint32), ("min_inliers", C.c_uint32), ("min_margin", C.c_uint32), ("min_landmark_obs", C.c_uint32),
                ("segment", C.c_uint32), ("target_segment", C.c_uint32), ("min_loop_scans", C.c_uint32), ("recent_scans", C.c_uint32),
                ("reserved", C.c_uint32)]


class FxMapLoopCandidate(C.Structure):
    _fields_ = [("c", C.c_double), ("s", C.c_double), ("tx", C.c_double), ("ty", C.c_double), ("tz", C.c_double), ("wc", C.c_double),
                ("ws", C.c_double), ("wtx", C.c_double), ("wty", C.c_double), ("wtz", C.c_double), ("n_hyp", C.c_uint64),
                ("n_query", C.c_uint32), ("n_targets", C.c_uint32), ("n_seeds", C.c_uint32), ("score", C.c_uint32), ("runner_up", C.c_uint32),
                ("flags", C.c_uint32), ("seed_a", C.c_uint32), ("seed_b", C.c_uint32), ("lm_a", C.c_uint32), ("lm_b", C.c_uint32),
                ("segment", C.c_uint32), ("target_segment", C.c_uint32)]


FX_FIND_MAX_QUERY = 64
FX_FIND_SAME_SEGMENT = 0xfffffffd
FX_FIND_VALID, FX_FIND_TRUNCATED, FX_FIND_NO_HYPOTHESIS, FX_FIND_AMBIGUOUS, FX_FIND_BAD_SEGMENT = 0x1, 0x2, 0x4, 0x8, 0x10
FX_FIND_NONE = 0xffffffff
FX_FIND_NAN_BITS = 0x7ff8000000000000  # c, s, tx, ty, tz of a result that is not FX_FIND_VALID
# fx_map_loop_candidate as a numpy record (find_loop_records)
FIND_DTYPE = np.dtype([("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("tz", "<f8"), ("wc", "<f8"), ("ws", "<f8"), ("wtx", "<f8"),
                       ("wty", "<f8"), ("wtz", "<f8"), ("n_hyp", "<u8"), ("n_query", "<u4"), ("n_targets", "<u4"), ("n_seeds", "<u4"),
                       ("score", "<u4"), ("runner_up", "<u4"), ("flags", "<u4"), ("seed_a", "<u4"), ("seed_b", "<u4"), ("lm_a", "<u4"),
                       ("lm_b", "<u4"), ("segment", "<u4"), ("target_segment", "<u4")])
FIND_DEFAULTS = dict(inlier_dist=0.30, pair_tol=0.30, min_baseline=2.0, max_baseline=60.0, max_seeds=16, min_inliers=4, min_margin=1,
                     min_landmark_obs=2, segment=FX_LOC_LAST_SEGMENT, target_segment=FX_FIND_SAME_SEGMENT, min_loop_scans=256, recent_scans=32)


class FxSpliceSource(C.Structure):
    _fields_ = [("kp_block_device", C.c_void_p), ("max_scans", C.c_uint32), ("max_total_keypoints", C.c_uint32),
                ("csr_block_device", C.c_void_p), ("max_rows", C.c_uint32), ("capacity", C.c_uint32), ("scan0", C.c_uint32), ("n_scans", C.c_uint32)]


FX_SPLICE_LAST_SCAN = 0xffffffff  # scan0: the source's last scan, read on the device


class FxDeskewOptions(C.Structure):
    _fields_ = [("start_turn", C.c_double), ("ref_fraction", C.c_double), ("sweep_fraction", C.c_double), ("direction", C.c_int32),
                ("source", C.c_uint32), ("require_flags", C.c_uint32), ("reserved", C.c_uint32)]


class FxDeskewScan(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("motion", C.c_uint32), ("rows_moved", C.c_uint32), ("max_shift", C.c_float)]


FX_DESKEW_LINKS, FX_DESKEW_PER_SCAN = 0, 1
FX_DESKEW_MOVED, FX_DESKEW_NEXT_LINK, FX_DESKEW_NO_MOTION, FX_DESKEW_NO_SCAN = 0x1, 0x2, 0x4, 0x8
FX_DESKEW_NO_RECORD = 0xffffffff
# include/fx.h FX_DESKEW_TURN_K restated (tests/test_deskew_reference.py holds the two together)
DESKEW_TURN_K = (0.15915173357526405, -0.052943764423474274, 0.030823588143917297, -0.01856560178002491, 0.008407119202664756,
                 -0.001873333241134883)
# fx_deskew_scan as a numpy record (deskew_records)
DESKEW_DTYPE = np.dtype([("flags", "<u4"), ("motion", "<u4"), ("rows_moved", "<u4"), ("max_shift", "<f4")])
DESKEW_DEFAULTS = dict(start_turn=0.5, ref_fraction=1.0, sweep_fraction=1.0, direction=-1, source=FX_DESKEW_LINKS, require_flags=0x1)


class FxFollowOptions(C.Structure):
    _fields_ = [("loc", FxLocalizeOptions), ("chain_scans", C.c_uint32), ("require_flags", C.c_uint32), ("max_lost", C.c_uint32),
                ("reserved", C.c_uint32)]


class FxFollowScan(C.Structure):
    _fields_ = [("prior", FxPose), ("flags", C.c_uint32), ("motion", C.c_uint32), ("streak", C.c_uint32), ("reserved", C.c_uint32)]


FX_FOLLOW_START, FX_FOLLOW_LINK, FX_FOLLOW_COASTED, FX_FOLLOW_HELD, FX_FOLLOW_LOST = 0x1, 0x2, 0x4, 0x8, 0x10
FX_FOLLOW_NO_MOTION = 0xffffffff
# fx_follow_scan as a numpy record (follow_records); "prior" is a POSE_DTYPE record
FOLLOW_DTYPE = np.dtype([("prior", POSE_DTYPE), ("flags", "<u4"), ("motion", "<u4"), ("streak", "<u4"), ("reserved", "<u4")])
# the fields of fx_follow_options: fx_localize_options's (segment: every segment) and the chain's own
FOLLOW_DEFAULTS = dict(LOC_DEFAULTS, segment=FX_LOC_ANY_SEGMENT, chain_scans=0, require_flags=FX_REG_VALID, max_lost=5)


class FxTestGatherInfo(C.Structure):  # (the header's FX_TEST_HOOKS section)
    _fields_ = [("batch", C.c_uint32), ("rows", C.c_uint32), ("near_words", C.c_uint32), ("list_cap", C.c_uint32), ("ovf_cap", C.c_uint32),
                ("ovf_stored", C.c_uint32), ("dense_min", C.c_uint32), ("max_dense_rows", C.c_uint32),
                ("r2_support", C.c_float), ("r2_search", C.c_float), ("box_margin", C.c_float),
                ("n_list", C.c_uint32), ("n_wave", C.c_uint32), ("n_group", C.c_uint32 * 3), ("n_dense", C.c_uint32)]


_GATHER_OUT = ("near_bits", "s_cnt", "s_pts", "ovf_cnt", "ovf_pts", "ovf_kp", "row_map", "row_kp", "row_class", "row_xa", "list_desc",
               "wave_desc", "group_desc", "dense_rows")


class FxTestGatherOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _GATHER_OUT]


class FxTimings(C.Structure):
    _fields_ = [("ms", C.c_float * FX_N_STAGES), ("total_ms", C.c_float), ("k_prep_exec_ms", C.c_float)]


class FxStageBytes(C.Structure):
    _fields_ = [("read", C.c_double * FX_N_STAGES), ("written", C.c_double * FX_N_STAGES)]


class FxSynthCfg(C.Structure):
    _fields_ = [("n_rings", C.c_uint32), ("n_az", C.c_uint32), ("el0_deg", C.c_double), ("el_step_deg", C.c_double),
                ("n_poles", C.c_uint32), ("pole_radius", C.c_double), ("pole_height", C.c_double),
                ("x_lo", C.c_double), ("x_hi", C.c_double), ("y_lo", C.c_double), ("y_hi", C.c_double),
                ("sensor_height", C.c_double), ("wall_radius", C.c_double), ("seed", C.c_uint64)]


# every symbol include/fx.h declares (tests/test_capi_symbols.py checks the list against the header)
FX_HEADER_VERSION = (0 << 16) | 7  # the include/fx.h these ctypes structures mirror
EXPORTS = ("fx_version", "fx_check_abi", "fx_status_str", "fx_last_error", "fx_params_default", "fx_params_launch",
           "fx_limits_default", "fx_limits_sparse", "fx_create", "fx_destroy", "fx_set_stream", "fx_get_stream", "fx_set_graph_batch", "fx_set_batches_in_flight", "fx_set_profiling", "fx_set_profiling_stages", "fx_get_timings",
           "fx_get_stage_bytes", "fx_get_limits", "fx_process_batch", "fx_synchronize", "fx_pack_features", "fx_pack_keypoint_records", "fx_keypoint_block_bytes", "fx_pack_keypoint_block",
           "fx_descriptor_csr_bytes", "fx_pack_descriptors_csr", "fx_get_descriptors_csr", "fx_set_descriptor_csr_capacity",
           "fx_match_options_default", "fx_match_descriptors_csr", "fx_register_options_default", "fx_register_matches",
           "fx_track_options_default", "fx_track_landmarks",
           "fx_map_create", "fx_map_destroy", "fx_map_reset", "fx_map_update", "fx_map_get", "fx_map_read_header", "fx_map_read_landmarks",
           "fx_map_merge_options_default", "fx_map_merge", "fx_map_get_alias", "fx_map_read_alias",
           "fx_localize_options_default", "fx_map_localize", "fx_relocalize_options_default", "fx_map_relocalize",
           "fx_map_observe_options_default", "fx_map_observe",
           "fx_map_expect_options_default", "fx_map_expect_options_from_params", "fx_map_expect",
           "fx_map_retire_options_default", "fx_map_retire",
           "fx_map_discover_options_default", "fx_map_discover",
           "fx_map_compact_options_default", "fx_map_compact", "fx_map_export_host", "fx_map_import_host", "fx_map_snapshot_check",
           "fx_map_append", "fx_map_append_host",
           "fx_map_join_options_default", "fx_map_join_segments",
           "fx_map_loop_options_default", "fx_map_close_loop", "fx_map_loop_correct_poses",
           "fx_map_find_loop_options_default", "fx_map_find_loop", "fx_splice_blocks",
           "fx_deskew_options_default", "fx_deskew_keypoint_block", "fx_follow_options_default", "fx_map_follow",
           "fx_rotation_from_roll_pitch", "fx_sc3d_tables", "fx_sc3d_xaxis", "fx_synth_cfg_vlp16",
           "fx_synth_scan", "fx_unpack_pointcloud2", "fx_pack_pointxyzi")
# the header's FX_TEST_HOOKS section: exported by lib/libfx_hip_test.so only
TEST_EXPORTS = ("fx_test_sort_replay", "fx_test_sort_replay_ranked", "fx_test_sort_replay_lists", "fx_test_sort_replay_device",
                "fx_test_cc_order_device", "fx_test_elevation_device", "fx_test_within_device", "fx_test_gather_state")

_lib = None
_libs = {}
# lib/libfx_hip_test.so: the same sources compiled with -DFX_TEST_HOOKS (environment hooks that push work through the rarely
# used tiers and kernels: FX_FRONT, FX_FRONT_FORCE, FX_MERGE_BIG_CAP, ...).  The product library has none of them.
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libfx_hip_test.so")


class test_hooks:
    """Context manager: inside it load() (and so Context, params, ...) uses the test build of the library."""

    def __enter__(self):
        global _lib, LIB_PATH
        self._saved = (_lib, LIB_PATH)
        LIB_PATH = TEST_LIB_PATH
        _lib = _libs.get(LIB_PATH)
        try:
            return load()
        except BaseException:  # (a missing / mismatched test library must not leave the process pointing at it)
            _lib, LIB_PATH = self._saved
            raise

    def __exit__(self, *exc):
        global _lib, LIB_PATH
        _lib, LIB_PATH = self._saved
        return False


def load_test():
    """The test build of the library (FX_TEST_HOOKS: the fx_test_* entry points and the environment hooks) without making it
    the process's default."""
    with test_hooks() as lib:
        return lib


def load():
    """Load libfx_hip.so; raises (never falls back) if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if LIB_PATH in _libs:
        _lib = _libs[LIB_PATH]
        return _lib
    try:
        # When torch is going to be used in the same process (tests, bench.py) it must be imported
        # before libfx_hip.so is loaded: both link libamdhip64 and the process must end up with ONE HIP
        # runtime; with the other order the second runtime to initialise finds no device.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The hot path has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.fx_version.restype = C.c_uint32
    # the ABI guard before anything else: these structures must be the library's (include/fx.h fx_check_abi)
    lib.fx_last_error.restype = C.c_char_p
    lib.fx_check_abi.argtypes = [C.c_uint32, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
    if lib.fx_check_abi(FX_HEADER_VERSION, C.sizeof(FxParams), C.sizeof(FxLimits), C.sizeof(FxScanDesc), C.sizeof(FxBatchView)) != FX_OK:
        raise RuntimeError(f"{LIB_PATH}: {lib.fx_last_error().decode()}")
    lib.fx_status_str.restype = C.c_char_p
    lib.fx_status_str.argtypes = [C.c_int]
    lib.fx_last_error.restype = C.c_char_p
    lib.fx_params_default.argtypes = [C.POINTER(FxParams)]
    lib.fx_params_launch.argtypes = [C.POINTER(FxParams)]
    lib.fx_limits_default.argtypes = [C.POINTER(FxLimits), C.c_uint32, C.c_uint32]
    lib.fx_limits_sparse.argtypes = [C.POINTER(FxLimits), C.c_uint32, C.c_uint32]
    lib.fx_create.argtypes = [C.POINTER(FxParams), C.POINTER(FxLimits), C.c_int, C.POINTER(C.c_void_p)]
    lib.fx_create.restype = C.c_int
    lib.fx_destroy.argtypes = [C.c_void_p]
    lib.fx_destroy.restype = None
    lib.fx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.fx_set_profiling.argtypes = [C.c_void_p, C.c_int]
    lib.fx_set_profiling_stages.argtypes = [C.c_void_p, C.c_uint32]
    lib.fx_set_graph_batch.argtypes = [C.c_void_p, C.c_uint32]
    lib.fx_set_batches_in_flight.argtypes = [C.c_void_p, C.c_uint32]
    lib.fx_get_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.fx_get_stream.restype = C.c_int
    lib.fx_get_timings.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(FxTimings)]
    lib.fx_get_limits.argtypes = [C.c_void_p, C.POINTER(FxLimits)]
    lib.fx_get_stage_bytes.argtypes = [C.c_void_p, C.POINTER(FxStageBytes)]
    lib.fx_process_batch.argtypes = [C.c_void_p, C.POINTER(FxScanDesc), C.c_uint32, C.c_uint32,
                                     C.POINTER(FxBatchView)]
    lib.fx_process_batch.restype = C.c_int
    lib.fx_synchronize.argtypes = [C.c_void_p]
    lib.fx_pack_features.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.fx_pack_keypoint_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.fx_keypoint_block_bytes.argtypes = [C.c_uint32, C.c_uint32]
    lib.fx_keypoint_block_bytes.restype = C.c_size_t
    lib.fx_pack_keypoint_block.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.fx_descriptor_csr_bytes.argtypes = [C.c_uint32, C.c_uint32]
    lib.fx_descriptor_csr_bytes.restype = C.c_size_t
    lib.fx_pack_descriptors_csr.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.fx_get_descriptors_csr.argtypes = [C.c_void_p, C.POINTER(FxDescriptorCsrView)]
    lib.fx_set_descriptor_csr_capacity.argtypes = [C.c_void_p, C.c_uint32]
    lib.fx_match_options_default.argtypes = [C.POINTER(FxMatchOptions)]
    lib.fx_match_options_default.restype = None
    lib.fx_match_descriptors_csr.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                             C.POINTER(FxMatchPair), C.c_uint32, C.POINTER(FxMatchOptions), C.c_void_p]
    lib.fx_register_options_default.argtypes = [C.POINTER(FxRegisterOptions)]
    lib.fx_register_options_default.restype = None
    lib.fx_register_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.c_uint32, C.POINTER(FxMatchPair), C.c_uint32, C.POINTER(FxRegisterOptions), C.c_void_p, C.c_void_p]
    lib.fx_track_options_default.argtypes = [C.POINTER(FxTrackOptions)]
    lib.fx_track_options_default.restype = None
    lib.fx_track_landmarks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                       C.POINTER(FxPose), C.POINTER(FxTrackOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.c_void_p]
    lib.fx_map_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.fx_map_destroy.argtypes = [C.c_void_p]
    lib.fx_map_destroy.restype = None
    lib.fx_map_reset.argtypes = [C.c_void_p, C.c_void_p]
    lib.fx_map_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.fx_map_get.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.fx_map_read_header.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FxMapHeader)]
    lib.fx_map_read_landmarks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.fx_map_merge_options_default.argtypes = [C.POINTER(FxMapMergeOptions)]
    lib.fx_map_merge_options_default.restype = None
    lib.fx_map_merge.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FxMapMergeOptions), C.c_void_p]
    lib.fx_map_get_alias.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.fx_map_read_alias.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.fx_localize_options_default.argtypes = [C.POINTER(FxLocalizeOptions)]
    lib.fx_localize_options_default.restype = None
    lib.fx_map_localize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.POINTER(FxLocalizeOptions), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fx_relocalize_options_default.argtypes = [C.POINTER(FxRelocalizeOptions)]
    lib.fx_relocalize_options_default.restype = None
    lib.fx_map_relocalize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.POINTER(FxRelocalizeOptions), C.c_void_p, C.c_void_p]
    lib.fx_map_observe_options_default.argtypes = [C.POINTER(FxMapObserveOptions)]
    lib.fx_map_observe_options_default.restype = None
    lib.fx_map_observe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                   C.POINTER(FxMapObserveOptions), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fx_map_expect_options_default.argtypes = [C.POINTER(FxMapExpectOptions)]
    lib.fx_map_expect_options_default.restype = None
    lib.fx_map_expect_options_from_params.argtypes = [C.POINTER(FxParams), C.c_float, C.POINTER(FxMapExpectOptions)]
    lib.fx_map_expect_options_from_params.restype = None
    lib.fx_map_expect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                  C.POINTER(FxMapExpectOptions), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fx_map_retire_options_default.argtypes = [C.POINTER(FxMapRetireOptions)]
    lib.fx_map_retire_options_default.restype = None
    lib.fx_map_retire.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FxMapRetireOptions), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fx_map_discover_options_default.argtypes = [C.POINTER(FxMapDiscoverOptions)]
    lib.fx_map_discover_options_default.restype = None
    lib.fx_map_discover.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                    C.POINTER(FxMapDiscoverOptions), C.c_void_p, C.c_void_p]
    lib.fx_map_compact_options_default.argtypes = [C.POINTER(FxMapCompactOptions)]
    lib.fx_map_compact_options_default.restype = None
    lib.fx_map_compact.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FxMapCompactOptions), C.c_void_p, C.c_void_p]
    lib.fx_map_export_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fx_map_import_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fx_map_snapshot_check.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32]
    lib.fx_map_append.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fx_map_append_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.fx_map_join_options_default.argtypes = [C.POINTER(FxMapJoinOptions)]
    lib.fx_map_join_options_default.restype = None
    lib.fx_map_join_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(FxPose), C.c_void_p, C.POINTER(FxMapJoinOptions),
                                         C.c_void_p, C.c_void_p]
    lib.fx_map_loop_options_default.argtypes = [C.POINTER(FxMapLoopOptions)]
    lib.fx_map_loop_options_default.restype = None
    lib.fx_map_close_loop.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FxPose), C.c_void_p, C.POINTER(FxMapLoopOptions), C.c_void_p, C.c_void_p]
    lib.fx_map_loop_correct_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.fx_map_find_loop_options_default.argtypes = [C.POINTER(FxMapFindLoopOptions)]
    lib.fx_map_find_loop_options_default.restype = None
    lib.fx_map_find_loop.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FxMapFindLoopOptions), C.c_void_p, C.c_void_p]
    lib.fx_splice_blocks.argtypes = [C.c_void_p, C.POINTER(FxSpliceSource), C.POINTER(FxSpliceSource), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                     C.c_uint32, C.c_uint32]
    lib.fx_deskew_options_default.argtypes = [C.POINTER(FxDeskewOptions)]
    lib.fx_deskew_options_default.restype = None
    lib.fx_deskew_keypoint_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                             C.POINTER(FxDeskewOptions), C.c_void_p]
    lib.fx_follow_options_default.argtypes = [C.POINTER(FxFollowOptions)]
    lib.fx_follow_options_default.restype = None
    lib.fx_map_follow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                  C.POINTER(FxFollowOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fx_rotation_from_roll_pitch.argtypes = [C.c_double, C.c_double, _F32P]
    lib.fx_rotation_from_roll_pitch.restype = None
    lib.fx_sc3d_tables.argtypes = [C.c_double, _F32P, _F32P, _F32P, _F32P]
    lib.fx_sc3d_tables.restype = None
    lib.fx_sc3d_xaxis.argtypes = [C.c_uint32, _F32P]
    lib.fx_sc3d_xaxis.restype = None
    lib.fx_synth_cfg_vlp16.argtypes = [C.POINTER(FxSynthCfg), C.c_uint64]
    lib.fx_synth_cfg_vlp16.restype = None
    lib.fx_synth_scan.argtypes = [C.POINTER(FxSynthCfg), _F32P, C.c_uint32]
    lib.fx_synth_scan.restype = C.c_uint32
    lib.fx_unpack_pointcloud2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(FxPc2Layout), C.c_void_p]
    lib.fx_pack_pointxyzi.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, _U32P]
    if hasattr(lib, "fx_test_sort_replay"):  # the test build (-DFX_TEST_HOOKS)
        lib.fx_test_sort_replay.argtypes = [_U32P, C.c_uint32, _U32P]
        lib.fx_test_sort_replay.restype = None
        lib.fx_test_sort_replay_ranked.argtypes = [_U32P, C.c_uint32, _U32P]
        lib.fx_test_sort_replay_ranked.restype = None
        lib.fx_test_sort_replay_lists.argtypes = [_U32P, C.c_uint32, _U32P]
        lib.fx_test_sort_replay_lists.restype = None
        lib.fx_test_sort_replay_device.argtypes = [C.c_int, _U32P, C.c_uint32, C.c_uint32, _U32P]
        lib.fx_test_cc_order_device.argtypes = [C.c_int, _U32P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _U32P, C.c_uint32, C.c_int,
                                                _U32P, _U32P, _U32P, _U32P]
        lib.fx_test_elevation_device.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.fx_test_within_device.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        lib.fx_test_gather_state.argtypes = [C.c_void_p, C.POINTER(FxTestGatherInfo), C.POINTER(FxTestGatherOut)]
    _lib = lib
    _libs[LIB_PATH] = lib
    return lib


class FxError(RuntimeError):
    pass


def check(status):
    if status != FX_OK:
        lib = load()
        raise FxError(f"fx status {status} ({lib.fx_status_str(status).decode()}): {lib.fx_last_error().decode()}")


def params(preset="default", **overrides):
    """fx_params for a named preset: 'default' (ref: node.cpp:9-34) or 'launch'
    (ref: launch/keypoint_playback.launch:17-33), with keyword overrides."""
    lib = load()
    p = FxParams()
    {"default": lib.fx_params_default, "launch": lib.fx_params_launch}[preset](C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def limits(max_batch, max_points, sparse=False, **overrides):
    """fx_limits_default (or, sparse=True, fx_limits_sparse: small dense-tier pools, for VLP-16-class workloads) with overrides."""
    lib = load()
    l = FxLimits()
    (lib.fx_limits_sparse if sparse else lib.fx_limits_default)(C.byref(l), max_batch, max_points)
    for k, v in overrides.items():
        if not hasattr(l, k):
            raise AttributeError(k)
        setattr(l, k, v)
    return l


def synth_cfg(seed, **overrides):
    lib = load()
    c = FxSynthCfg()
    lib.fx_synth_cfg_vlp16(C.byref(c), seed)
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def synth_scan(cfg):
    """One synthetic scan as an [N,4] float32 array (x, y, z, 0), firing order."""
    lib = load()
    n = cfg.n_rings * cfg.n_az
    out = np.zeros((n, 4), np.float32)
    got = lib.fx_synth_scan(C.byref(cfg), out.ctypes.data_as(_F32P), n)
    assert got == n
    return out


# ---- descriptors as compressed rows (CSR; include/fx.h fx_descriptor_csr_bytes)
def csr_layout(max_rows, capacity):
    """Byte offsets (row_ptr, col, val, end) of the sections of a CSR block: header 16 B, row_ptr u32[max_rows + 1], col u32[capacity],
    val f32[capacity], each rounded up to 16 bytes."""
    rp = 16
    col = rp + 4 * ((max_rows + 1 + 3) // 4 * 4)
    val = col + 4 * ((capacity + 3) // 4 * 4)
    return rp, col, val, val + 4 * ((capacity + 3) // 4 * 4)


def csr_from_dense(rows):
    """The storage rule, stated in numpy: every word of the [n, 1989] float32 rows whose bit pattern is non-zero (-0.0 and NaN
    included), row by row, columns increasing.  Returns (row_ptr u32[n + 1], col u32[nnz], val f32[nnz])."""
    bits = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, FX_DESC_FLOATS).view(np.uint32)
    nz = bits != 0
    row_ptr = np.zeros(len(bits) + 1, np.uint32)
    np.cumsum(nz.sum(axis=1), out=row_ptr[1:])
    r, c = np.nonzero(nz)
    return row_ptr, c.astype(np.uint32), bits[r, c].view(np.float32)


def dense_from_csr(row_ptr, col, val, n_rows=None):
    """[n, 1989] float32 rows from (row_ptr, col, val): zeros everywhere else, the stored words bit for bit.  n_rows (default
    len(row_ptr) - 1) reads row_ptr[:n_rows + 1]; col / val are indexed from row_ptr[0]."""
    row_ptr = np.asarray(row_ptr).astype(np.int64)
    n = len(row_ptr) - 1 if n_rows is None else int(n_rows)
    out = np.zeros((n, FX_DESC_FLOATS), np.uint32)
    lo, hi = int(row_ptr[0]), int(row_ptr[n])
    r = np.repeat(np.arange(n), np.diff(row_ptr[:n + 1]))
    out[r, np.asarray(col)[lo:hi].astype(np.int64)] = np.ascontiguousarray(np.asarray(val)[lo:hi], dtype=np.float32).view(np.uint32)
    return out.view(np.float32)


def csr_parse(block, max_rows, capacity):
    """A CSR block (bytes / uint8 array, as fx_pack_descriptors_csr writes it) as a dict: the header words and the stored
    row_ptr[:min(rows, max_rows) + 1], col[:nnz_stored], val[:nnz_stored]."""
    b = np.frombuffer(bytes(block), np.uint8) if not isinstance(block, np.ndarray) else np.ascontiguousarray(block).view(np.uint8)
    rp, col, val, _ = csr_layout(max_rows, capacity)
    rows, nnz_stored, nnz_needed, rows_stored = (int(x) for x in b[:16].view(np.uint32))
    n = min(rows, max_rows)
    return {"rows": rows, "nnz_stored": nnz_stored, "nnz_needed": nnz_needed, "rows_stored": rows_stored,
            "row_ptr": b[rp:rp + 4 * (n + 1)].view(np.uint32).copy(), "row_ptr_all": b[rp:rp + 4 * (max_rows + 1)].view(np.uint32).copy(),
            "col": b[col:col + 4 * nnz_stored].view(np.uint32).copy(), "val": b[val:val + 4 * nnz_stored].view(np.float32).copy()}


# ---- matching descriptor rows across azimuth shifts (include/fx.h fx_match_descriptors_csr)
def pairs_consecutive(kp_offset):
    """Scan b + 1's rows as query against scan b's as train, for the scans of one batch: [(q_row0, q_rows, t_row0, t_rows)]."""
    off = [int(x) for x in kp_offset]
    return [(off[b + 1], off[b + 2] - off[b + 1], off[b], off[b + 1] - off[b]) for b in range(len(off) - 2)]


def match_epsilon(d2, nq2, nt2):
    """The error bound of a reported dist2 (include/fx.h): 2^-23 d2 + 2^-40 (|q|^2 + |t|^2) + 2^-150, the last term half the
    smallest fp32 subnormal (the one rounding to fp32)."""
    return 2.0 ** -23 * d2 + 2.0 ** -40 * (nq2 + nt2) + 2.0 ** -150


def match_records(out):
    """A host copy of fx_match_descriptors_csr's output (a torch int32 tensor [n, 8], or any array of n * 32 bytes) as a
    structured numpy array of MATCH_DTYPE records."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(MATCH_DTYPE).copy()


def match_reference(rows_q, rows_t, pairs, shifts=12, max_dist2=np.inf, max_ratio=1.0, mutual=False):
    """The matching rule of include/fx.h stated in numpy on dense [n, 1989] float32 rows.  d2(q, t, s) = sum over the 1980 bins of
    (q[c] - t[(c + 165 s) mod 1980])^2, formed directly in float64 term by term (no |q|^2 + |t|^2 - 2 q.t): where q[c] is 0 the
    term is t^2, summed as such.  Returns a dict: "rec" (MATCH_DTYPE [n_q], what the library writes), "d2" (per pair the float64
    array [q rows, t rows, shifts], NaN for rows that hold a non-finite word), "nq2" / "nt2" (|row|^2 of the bins, float64) and "ranges"
    (per pair the clipped (q0, q1, t0, t1))."""
    rows_q = np.ascontiguousarray(rows_q, dtype=np.float32).reshape(-1, FX_DESC_FLOATS)
    rows_t = np.ascontiguousarray(rows_t, dtype=np.float32).reshape(-1, FX_DESC_FLOATS)
    nq, nt, B = len(rows_q), len(rows_t), FX_DESC_BINS
    Q, T = rows_q[:, :B].astype(np.float64), rows_t[:, :B].astype(np.float64)
    q_nan, t_nan = (~np.isfinite(rows_q)).any(axis=1), (~np.isfinite(rows_t)).any(axis=1)  # (any stored word, rf included)
    rec = np.zeros(nq, MATCH_DTYPE)
    rec["train_row"] = rec["second_row"] = -1
    rec["dist2"] = rec["dist2_second"] = np.inf
    rec["pair"] = FX_MATCH_NO_PAIR
    ratio2 = np.float32(max_ratio) * np.float32(max_ratio)
    seen = np.zeros(nq, bool)
    d2s, ranges = [], []
    for p, (q0, qn, t0, tn) in enumerate(pairs):
        q1, t1 = min(q0 + qn, nq), min(t0 + tn, nt)
        q0, t0 = min(q0, q1), min(t0, t1)
        if seen[q0:q1].any():
            raise ValueError("query ranges of the pairs overlap")
        seen[q0:q1] = True
        ranges.append((q0, q1, t0, t1))
        d2 = np.full((q1 - q0, t1 - t0, shifts), np.nan)
        qi, ti = np.flatnonzero(~q_nan[q0:q1]), np.flatnonzero(~t_nan[t0:t1])
        if len(qi) and len(ti):
            Qp, Tp = Q[q0:q1][qi], T[t0:t1][ti]
            zero = (Qp == 0).astype(np.float64)
            for s in range(shifts):
                Ts = np.roll(Tp, -FX_MATCH_SECTOR * s, axis=1)  # Ts[c] = t[(c + 165 s) mod 1980]
                part = (Ts * Ts) @ zero.T  # [t, q]: the terms where q[c] is 0, each t^2
                for k in range(len(qi)):
                    c = np.flatnonzero(Qp[k])
                    part[:, k] += ((Qp[k, c][None, :] - Ts[:, c]) ** 2).sum(axis=1)
                d2[np.ix_(qi, ti, [s])] = part.T[:, :, None]
        d2s.append(d2)
        rec["pair"][q0:q1] = p
        f32 = d2.astype(np.float32)  # (one rounding, as the library's; comparisons are on the fp32 values)
        best_t = np.full((q1 - q0, t1 - t0), np.inf, np.float32)  # per train row: min over shifts, the lowest shift on ties
        best_s = np.zeros((q1 - q0, t1 - t0), np.uint32)
        valid = ~np.isnan(d2[:, :, 0]) if d2.size else np.zeros(d2.shape[:2], bool)
        if d2.size:
            f = np.where(np.isnan(f32), np.float32(np.inf), f32)
            best_s = f.argmin(axis=2).astype(np.uint32)
            best_t = f.min(axis=2)
        for i in range(q1 - q0):
            cand = np.flatnonzero(valid[i])
            if not len(cand):
                continue
            order = cand[np.lexsort((cand, best_t[i, cand]))]  # by (dist2, train row)
            r = rec[q0 + i:q0 + i + 1]
            j = order[0]
            r["train_row"], r["shift"], r["dist2"] = t0 + j, best_s[i, j], best_t[i, j]
            if len(order) > 1:
                r["second_row"], r["dist2_second"] = t0 + order[1], best_t[i, order[1]]
            ok = bool(r["dist2"][0] <= np.float32(max_dist2))
            if ok and np.float32(max_ratio) < 1:
                with np.errstate(invalid="ignore"):
                    ok = bool(r["dist2"][0] <= ratio2 * r["dist2_second"][0])
            r["flags"] = FX_MATCH_ACCEPTED if ok else 0
        if mutual:
            for j in range(t1 - t0):
                cand = np.flatnonzero(valid[:, j])
                if len(cand):
                    i = cand[np.lexsort((cand, best_t[cand, j]))][0]
                    if rec["train_row"][q0 + i] == t0 + j:
                        rec["flags"][q0 + i] |= FX_MATCH_MUTUAL
    return {"rec": rec, "d2": d2s, "ranges": ranges, "nq2": (Q * Q).sum(axis=1), "nt2": (T * T).sum(axis=1)}


# ---- scan-to-scan rigid motion from the matches (include/fx.h fx_register_matches)
class KeypointBlockLayout(tuple):
    """(k0, n_rows) of a compact keypoint block — the first float4 row of the keypoint area and the rows of the whole block —, which
    also carries f0, the first u32 word of the flags section."""

    def __new__(cls, f0, k0, n_rows):
        self = super().__new__(cls, (k0, n_rows))
        self.f0, self.k0, self.n_rows = f0, k0, n_rows
        return self


def keypoint_block_layout(max_scans, max_total):
    """The sections of a compact keypoint block (fx_pack_keypoint_block), the Python statement of csrc/fx_device.h's kp_block_*: as
    u32 words, the header is [0, 4), kp_offset (padded to whole rows) [4, f0) and the flags [f0, 4 * k0); as float4 rows, the
    keypoints are [k0, n_rows).  Unpacks as (k0, n_rows); .f0 is an attribute."""
    f0 = 4 + 4 * ((max_scans + 1 + 3) // 4)
    k0 = f0 // 4 + (max_scans + 3) // 4
    return KeypointBlockLayout(f0, k0, k0 + max_total)


def keypoint_block_parse(block, max_scans, max_total):
    """A keypoint block (bytes / array, as fx_pack_keypoint_block writes it) as a dict: the header words, kp_offset[scans + 1],
    flags[scans] and "rows", the [keypoints stored, 4] float32 (x, y, z, elevation) rows of the keypoint area."""
    b = np.frombuffer(bytes(block), np.uint8) if not isinstance(block, np.ndarray) else np.ascontiguousarray(block).view(np.uint8).reshape(-1)
    lay = keypoint_block_layout(max_scans, max_total)
    f0, k0, n_rows = lay.f0, lay.k0, lay.n_rows
    assert len(b) >= 16 * n_rows, (len(b), max_scans, max_total)
    u = b[:16 * n_rows].view(np.uint32)
    scans, stored, flags_or, mt = (int(x) for x in u[:4])
    stored = min(stored, max_total)
    nb = min(scans, max_scans)
    return {"scans": scans, "keypoints": stored, "flags_or": flags_or, "max_total": mt, "kp_offset": u[4:4 + nb + 1].copy(),
            "flags": u[f0:f0 + nb].copy(), "rows": b[16 * k0:16 * (k0 + stored)].view(np.float32).reshape(-1, 4).copy()}


def keypoint_block_from_rows(rows, max_scans=1, max_total=None):
    """The keypoint block of one scan holding these [n, 3 or 4] rows (what fx_pack_keypoint_block would write for a batch of one
    such scan), as a uint8 array; for tests and for registering keypoints that did not come from a batch.  Returns (block,
    max_scans, max_total)."""
    rows = np.asarray(rows, np.float32).reshape(len(rows), -1)
    n = len(rows)
    max_total = n if max_total is None else int(max_total)
    assert n <= max_total and max_scans >= 1
    lay = keypoint_block_layout(max_scans, max_total)
    f0, k0, n_rows = lay.f0, lay.k0, lay.n_rows
    blk = np.zeros((n_rows, 4), np.float32)
    u = blk.view(np.uint32).reshape(-1)
    u[:4] = (1, n, 0, max_total)
    u[5:f0] = n  # kp_offset[0] = 0, every later entry the total
    blk[k0:k0 + n, :rows.shape[1]] = rows[:, :4]
    return blk.view(np.uint8).reshape(-1), max_scans, max_total


def register_records(out):
    """A host copy of fx_register_matches's output (a torch tensor, or any array of n * 64 bytes) as a structured numpy array of
    REG_DTYPE records."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(REG_DTYPE).copy()


def register_yaw(rec):
    """atan2(s, c) of REG_DTYPE records: the rotation about z in radians (a host convenience, not a device output)."""
    return np.arctan2(rec["s"], rec["c"])


def _register_fit(P, idx, c, s):
    """The refit of include/fx.h over the correspondences idx (ascending) of P = [(qx, qy, tx, ty)] as Python floats: sequential
    sums, (c, s) kept when the centred sums vanish.  Returns (c, s, tx, ty)."""
    sqx = sqy = stx = sty = 0.0
    for i in idx:
        qx, qy, tx, ty = P[i]
        sqx += qx
        sqy += qy
        stx += tx
        sty += ty
    n = float(len(idx))
    qcx, qcy, tcx, tcy = sqx / n, sqy / n, stx / n, sty / n
    sdot = scrs = 0.0
    for i in idx:
        qx, qy, tx, ty = P[i]
        ux, uy, vx, vy = qx - qcx, qy - qcy, tx - tcx, ty - tcy
        sdot += (ux * vx + uy * vy)
        scrs += (ux * vy - uy * vx)
    nrm = math.sqrt(sdot * sdot + scrs * scrs)
    if nrm > 0.0:
        c, s = sdot / nrm, scrs / nrm
    return c, s, tcx - (c * qcx - s * qcy), tcy - (s * qcx + c * qcy)


def _register_r2(P, i, c, s, tx, ty):
    qx, qy, t_x, t_y = P[i]
    rx, ry = ((c * qx - s * qy) + tx) - t_x, ((s * qx + c * qy) + ty) - t_y
    return rx * rx + ry * ry


def register_reference(q_kp_rows, t_kp_rows, match_records, pairs, inlier_dist=0.30, min_baseline=2.0, hyp_corr=64, min_inliers=3,
                       require_flags=FX_MATCH_ACCEPTED):
    """The definition of fx_register_matches (include/fx.h) in numpy.  q_kp_rows / t_kp_rows: the [stored, >= 3] float32 keypoint
    rows of the two blocks (keypoint_block_parse(...)["rows"]); match_records: MATCH_DTYPE [q_max_rows], taken as given (from
    the GPU or from match_reference); pairs: [(q_row0, q_rows, t_row0, t_rows)].  The hypothesis stage runs in np.float32, one
    ufunc an operation (no contraction); the refit in Python floats in the stated order.  Returns {"rec": REG_DTYPE [n_pairs],
    "inlier": uint32 [q_max_rows], "corr": per pair the query rows of its correspondences}."""
    f32 = np.float32
    kq = np.ascontiguousarray(q_kp_rows, dtype=f32).reshape(len(q_kp_rows), -1)[:, :3]
    kt = np.ascontiguousarray(t_kp_rows, dtype=f32).reshape(len(t_kp_rows), -1)[:, :3]
    m = np.asarray(match_records)
    n_rows = len(m)
    rec = np.zeros(len(pairs), REG_DTYPE)
    inlier = np.zeros(n_rows, np.uint32)
    corrs = []
    idist, mb = f32(inlier_dist), f32(min_baseline)
    if not (np.isfinite(idist) and idist > 0 and np.isfinite(mb) and mb > 0 and 2 <= hyp_corr <= 128 and min_inliers >= 2):
        raise ValueError("options outside what fx_register_matches accepts")
    with np.errstate(all="ignore"):  # (a min_baseline whose square leaves float32's range: 0 or +inf, as on the device)
        mb2, gate, id2 = mb * mb, f32(2) * idist, idist * idist
    id2d = float(idist) * float(idist)
    seen = np.zeros(n_rows, bool)
    for p, (q0, qn, _t0, _tn) in enumerate(pairs):
        q1 = min(q0 + qn, n_rows)
        q0 = min(q0, q1)
        if seen[q0:q1].any():
            raise ValueError("query ranges of the pairs overlap")
        seen[q0:q1] = True
        i = np.arange(q0, min(q1, len(kq)), dtype=np.int64)
        mi = m[i]
        tr = mi["train_row"].astype(np.int64)
        ok = (mi["pair"] == p) & (tr >= 0) & (tr < len(kt)) & ((mi["flags"] & np.uint32(require_flags)) == np.uint32(require_flags))
        i, tr = i[ok], tr[ok]
        fin = np.isfinite(kq[i]).all(axis=1) & np.isfinite(kt[tr]).all(axis=1)
        i, tr = i[fin], tr[fin]
        r = rec[p:p + 1]
        flags = FX_REG_TRUNCATED if len(i) > FX_REG_MAX_CORR else 0
        i, tr = i[:FX_REG_MAX_CORR], tr[:FX_REG_MAX_CORR]
        n = len(i)
        corrs.append(i.astype(np.uint32))
        r["n_corr"] = n
        P32 = np.concatenate([kq[i][:, :2], kt[tr][:, :2]], axis=1) if n else np.zeros((0, 4), f32)  # (qx, qy, tx, ty)
        H = min(n, int(hyp_corr))
        best_count, best = 0, None
        if H >= 2:
            d2b = m["dist2"][i].view(np.uint32)
            pool = np.lexsort((i, d2b))[:H]  # by (dist2 bits, query row)
            a, b = np.triu_indices(H, 1)     # lexicographic (a, b), a < b
            A, B = P32[pool[a]], P32[pool[b]]
            with np.errstate(all="ignore"):
                dqx, dqy, dtx, dty = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1], B[:, 2] - A[:, 2], B[:, 3] - A[:, 3]
                lq2, lt2 = dqx * dqx + dqy * dqy, dtx * dtx + dty * dty
                keep = (lq2 >= mb2) & (lt2 >= mb2)
                keep &= ~(np.abs(np.sqrt(lq2) - np.sqrt(lt2)) > gate)
                dot, crs = dqx * dtx + dqy * dty, dqx * dty - dqy * dtx
                nrm = np.sqrt(dot * dot + crs * crs)
                keep &= nrm > 0
                c, s = dot / nrm, crs / nrm
                mqx, mqy, mtx, mty = (A[:, 0] + B[:, 0]) * f32(0.5), (A[:, 1] + B[:, 1]) * f32(0.5), (A[:, 2] + B[:, 2]) * f32(0.5), (A[:, 3] + B[:, 3]) * f32(0.5)
                tx, ty = mtx - (c * mqx - s * mqy), mty - (s * mqx + c * mqy)
                ks = np.flatnonzero(keep)
                counts = np.zeros(len(a), np.int64)
                for lo in range(0, len(ks), 512):  # (chunks: [samples, n] float32 temporaries)
                    k = ks[lo:lo + 512]
                    ck, sk, txk, tyk = c[k, None], s[k, None], tx[k, None], ty[k, None]
                    qx, qy, t_x, t_y = P32[None, :, 0], P32[None, :, 1], P32[None, :, 2], P32[None, :, 3]
                    rx, ry = ((ck * qx - sk * qy) + txk) - t_x, ((sk * qx + ck * qy) + tyk) - t_y
                    agree = rx * rx + ry * ry <= id2
                    counts[k] = agree.sum(axis=1)
                    assert rx.dtype == f32
            counts[counts < 2] = 0  # (a sample with fewer than 2 agreeing is no hypothesis)
            if counts.any():
                w = int(np.argmax(counts))  # (the first maximum: the lowest (a, b))
                best_count, best = int(counts[w]), w
                with np.errstate(all="ignore"):
                    rx = ((c[w] * P32[:, 0] - s[w] * P32[:, 1]) + tx[w]) - P32[:, 2]
                    ry = ((s[w] * P32[:, 0] + c[w] * P32[:, 1]) + ty[w]) - P32[:, 3]
                    I0 = [int(x) for x in np.flatnonzero(rx * rx + ry * ry <= id2)]
                assert len(I0) == best_count
        if best is None:
            r["c"], r["rms"], r["flags"], r["hyp_a"], r["hyp_b"] = 1.0, np.inf, flags | FX_REG_NO_HYPOTHESIS, FX_REG_NO_ROW, FX_REG_NO_ROW
            continue
        P = [tuple(float(x) for x in row) for row in P32]
        Z = [(float(kq[i[k], 2]), float(kt[tr[k], 2])) for k in range(n)]
        fit = _register_fit(P, I0, float(c[best]), float(s[best]))
        final = I0
        I1 = [k for k in range(n) if _register_r2(P, k, *fit) <= id2d]
        if len(I1) >= 2:
            fit = _register_fit(P, I1, fit[0], fit[1])
            final = I1
        sz = sr = 0.0
        for k in final:
            sz += (Z[k][1] - Z[k][0])
            sr += _register_r2(P, k, *fit)
        nf = float(len(final))
        r["c"], r["s"], r["tx"], r["ty"] = fit
        r["tz"] = sz / nf
        r["rms"] = np.float32(math.sqrt(sr / nf))
        r["n_inliers"] = len(final)
        r["flags"] = flags | (FX_REG_VALID if len(final) >= min_inliers else 0)
        r["hyp_a"], r["hyp_b"] = i[pool[a[best]]], i[pool[b[best]]]
        inlier[i[final]] = 1
    return {"rec": rec, "inlier": inlier, "corr": corrs}


# ---- poses and landmark tracks of one batch of consecutive scans (include/fx.h fx_track_landmarks)
def track_records(poses, landmark_of_row, obs_row, landmarks, header):
    """Host copies of fx_track_landmarks's five outputs (torch tensors, or arrays of the same bytes) as a dict: "poses" (POSE_DTYPE
    [n_scans]), "landmark_of_row" (int32 [q_max_rows]), "obs_row" (uint32 [q_max_rows]), "landmarks" (LANDMARK_DTYPE, the
    min(n_landmarks, max_landmarks) records written) and "header" (a dict of the six counts)."""
    def host(x):
        if hasattr(x, "detach"):
            x = x.detach().cpu().numpy()
        return np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    h = host(header).view(np.uint32)
    hdr = {k: int(h[i]) for i, k in enumerate(TRACK_HEADER_FIELDS)}
    lm = host(landmarks)
    lm = lm[:len(lm) // LANDMARK_DTYPE.itemsize * LANDMARK_DTYPE.itemsize].view(LANDMARK_DTYPE)
    return {"poses": host(poses).view(POSE_DTYPE).copy(), "landmark_of_row": host(landmark_of_row).view(np.int32).copy(),
            "obs_row": host(obs_row).view(np.uint32).copy(), "landmarks": lm[:min(hdr["n_landmarks"], len(lm))].copy(), "header": hdr}


def track_reference(kp_offset, kp_rows, match_records, inlier, reg_records, n_scans, init_pose=None, min_obs=2):
    """The definition of fx_track_landmarks (include/fx.h) in numpy and Python floats.  kp_offset: the block's kp_offset[scans + 1]
    and kp_rows its [stored, >= 3] float32 keypoint rows (keypoint_block_parse(...)["kp_offset"] / ["rows"], the rows already
    cut to min(stored, max_total_keypoints)); match_records (MATCH_DTYPE) and inlier, [q_max_rows] each, and reg_records
    (REG_DTYPE [>= n_scans - 1]) taken as given; init_pose: (c, s, tx, ty, tz) or None.  Returns what track_records returns
    (every landmark: no capacity), plus "parent" (int64 [q_max_rows], the kept parent of each row or -1)."""
    off = [int(x) for x in kp_offset]
    kp = np.ascontiguousarray(kp_rows, dtype=np.float32)
    kp = kp.reshape(len(kp), -1)[:, :3] if kp.size else np.zeros((0, 3), np.float32)
    m, inl, reg = np.asarray(match_records), np.asarray(inlier).astype(np.int64) & 0xffffffff, np.asarray(reg_records)
    R = len(m)
    n_scans, min_obs = int(n_scans), int(min_obs)
    if n_scans < 1 or min_obs < 1 or len(inl) != R:
        raise ValueError("arguments outside what fx_track_landmarks accepts")
    init = (1.0, 0.0, 0.0, 0.0, 0.0) if init_pose is None else tuple(float(v) for v in init_pose)
    if not all(math.isfinite(v) for v in init):
        raise ValueError("init_pose must be finite")
    S = min(n_scans, len(off) - 1)
    rows = min(len(kp), R)
    # good links and the pose fold
    good = [bool(reg["flags"][p] & FX_REG_VALID) and all(math.isfinite(float(reg[f][p])) for f in ("c", "s", "tx", "ty", "tz")) for p in range(S - 1)]
    poses = np.zeros(n_scans, POSE_DTYPE)
    pc, ps, ptx, pty, ptz = init
    seg = 0
    for b in range(n_scans):
        flags = 0
        if b >= S:
            flags = FX_POSE_NO_SCAN
        elif b >= 1 and good[b - 1]:
            rc, rs, rtx, rty, rtz = (float(reg[f][b - 1]) for f in ("c", "s", "tx", "ty", "tz"))
            pc, ps, ptx, pty, ptz = pc * rc - ps * rs, ps * rc + pc * rs, (pc * rtx - ps * rty) + ptx, (ps * rtx + pc * rty) + pty, ptz + rtz
        elif b >= 1:
            seg, flags = seg + 1, FX_POSE_GAP
        poses[b] = (pc, ps, ptx, pty, ptz, seg, flags)
    # the scan of every row
    scan = np.full(R, -1, np.int64)
    for b in range(S):
        scan[off[b]:min(off[b + 1], rows)] = b
    finite = np.isfinite(kp).all(axis=1)
    # proposals; a parent keeps its proposer of lowest row
    parent = np.full(R, -1, np.int64)
    child = {}
    proposers = 0
    for r in range(R):
        b = int(scan[r])
        if b < 1 or inl[r] != 1 or int(m["pair"][r]) != b - 1 or not good[b - 1]:
            continue
        t = int(m["train_row"][r])
        if not (off[b - 1] <= t < off[b] and t < rows and finite[r] and finite[t]):
            continue
        proposers += 1
        if t not in child:  # (rows ascend: the first proposer is the lowest)
            child[t] = r
            parent[r] = t
    # tracks: chains from every row without a kept parent, in ascending first row
    landmark_of_row = np.full(R, -1, np.int32)
    obs_row = np.full(R, FX_TRACK_NO_ROW, np.uint32)
    lms = []
    n_obs = 0
    for r in range(R):
        if scan[r] < 0 or parent[r] >= 0:
            continue
        chain = [r]
        while chain[-1] in child:
            chain.append(child[chain[-1]])
        if len(chain) < min_obs:
            continue
        landmark_of_row[chain] = len(lms)
        obs_row[n_obs:n_obs + len(chain)] = chain
        w = []
        for q in chain:
            c, s, tx, ty, tz = (float(poses[f][scan[q]]) for f in ("c", "s", "tx", "ty", "tz"))
            x, y, z = (float(v) for v in kp[q])
            w.append(((c * x - s * y) + tx, (s * x + c * y) + ty, z + tz))
        sx = sy = sz = 0.0
        for wx, wy, wz in w:
            sx += wx
            sy += wy
            sz += wz
        n = float(len(chain))
        mx, my, mz = sx / n, sy / n, sz / n
        acc = 0.0
        for wx, wy, _ in w:
            dx, dy = wx - mx, wy - my
            acc += (dx * dx + dy * dy)
        lms.append((mx, my, mz, np.float32(math.sqrt(acc / n)), len(chain), n_obs, r, int(scan[r]), int(scan[chain[-1]])))
        n_obs += len(chain)
    hdr = {"scans": S, "rows": rows, "n_landmarks": len(lms), "n_obs": n_obs, "n_conflicts": proposers - len(child),
           "n_gaps": sum(1 for g in good if not g)}
    return {"poses": poses, "landmark_of_row": landmark_of_row, "obs_row": obs_row, "landmarks": np.array(lms, LANDMARK_DTYPE),
            "header": hdr, "parent": parent}


# ---- the persistent landmark map: tracks carried across overlapping batches (include/fx.h fx_map_update)
def map_state(max_landmarks, max_carry_rows):
    """The state of a fresh map as map_reference keeps it: plain Python (a header dict, lists, one uint32 array)."""
    hdr = {k: 0 for k in MAP_HEADER_FIELDS}
    hdr["last_pose"] = (1.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    return {"max_landmarks": int(max_landmarks), "max_carry_rows": int(max_carry_rows), "header": hdr, "landmarks": [], "acc": [],
            "carry": [], "carry_kp": np.zeros((0, 4), np.uint32)}


def map_state_records(state):
    """A map_reference state as Map.records() returns the device's: {"header": the counts and last_pose (a 7-tuple),
    "landmarks": MAP_LANDMARK_DTYPE [n_landmarks]}."""
    lm = np.zeros(len(state["landmarks"]), MAP_LANDMARK_DTYPE)
    for i, r in enumerate(state["landmarks"]):
        lm[i] = tuple(r[f] for f in MAP_LANDMARK_DTYPE.names)
    return {"header": dict(state["header"]), "landmarks": lm}


def _map_record_from_sums(rec, acc):
    """include/fx.h fx_map_update's "Records" clause: the public x, y, z and rms_xy of a landmark from its sums and its n_obs."""
    dn = float(rec["n_obs"])
    mx, my = acc[5] / dn, acc[6] / dn
    var = acc[7] / dn - (mx * mx + my * my)
    rec["x"], rec["y"], rec["z"] = acc[0] / dn, acc[1] / dn, acc[2] / dn
    rec["rms_xy"] = np.float32(math.sqrt(var if var > 0.0 else 0.0))


def map_reference(state, kp_offset, kp_rows, track, overlap=False, track_max_landmarks=None):
    """The definition of fx_map_update (include/fx.h) in numpy and Python floats, one batch at a time.  state: map_state(...) or
    what an earlier call returned (it is not modified); kp_offset / kp_rows: the block's kp_offset[scans + 1] and its [stored, 4]
    float32 rows (all four words: the overlap is a comparison of bit patterns); track: what track_records / track_reference
    returned for the batch ("poses", "landmark_of_row", "obs_row", "landmarks", "header"); overlap: FX_MAP_OVERLAP;
    track_max_landmarks: the max_landmarks the track was run with (default: every landmark it needed).
    Returns (the new state, map_id_of_row int32 [q_max_rows])."""
    import copy
    st = copy.deepcopy(state)
    H, cap, max_carry = st["header"], st["max_landmarks"], st["max_carry_rows"]
    off = [int(x) for x in kp_offset]
    kp = np.ascontiguousarray(kp_rows, dtype=np.float32)
    kp = kp.reshape(len(kp), 4) if kp.size else np.zeros((0, 4), np.float32)
    words = kp.view(np.uint32)
    lor, obs_row, poses, lms, th = (track[k] for k in ("landmark_of_row", "obs_row", "poses", "landmarks", "header"))
    R = len(lor)
    S, rows = min(int(th["scans"]), len(off) - 1), min(int(th["rows"]), len(kp), R)
    max_l = len(lms) if track_max_landmarks is None else min(int(track_max_landmarks), len(lms))
    L = min(int(th["n_landmarks"]), max_l)
    ids = np.full(R, -1, np.int32)
    H["batches"] += 1
    H["last_joined"] = H["last_new"] = 0
    if S == 0:
        return st, ids

    def lo(b):
        return min(off[b], rows)

    def hi(b):
        return max(min(off[b + 1], rows), lo(b))
    n0 = hi(0) - lo(0)
    accepted = bool(overlap) and H["scans"] > 0 and H["carry_rows"] == n0 and np.array_equal(words[lo(0):hi(0)], st["carry_kp"][:n0])
    scan_base = H["scans"] - 1 if accepted else H["scans"]
    seg_base = H["segments"] - 1 if accepted else H["segments"]
    id_of_lm, n_new, n_joined, added = [], 0, 0, 0
    pose = [tuple(float(poses[f][b]) for f in ("c", "s", "tx", "ty", "tz")) for b in range(S)]  # (Python floats: IEEE doubles)
    xyz, obs = kp[:rows, :3].astype(np.float64).tolist(), np.asarray(obs_row).tolist()
    lm_words = [np.asarray(lms[f][:L]).tolist() for f in ("first_scan", "n_obs", "obs0", "first_row")]
    for i in range(L):
        fs, n, o, fr = (col[i] for col in lm_words)
        g = -1
        if accepted and fs == 0 and 0 <= fr - lo(0) < H["carry_rows"]:
            g = st["carry"][fr - lo(0)]
        if g >= 0:
            n_joined += 1
            lid = g
        else:
            lid = H["n_needed"] + n_new
            n_new += 1
        if lid >= cap:
            id_of_lm.append(-1)
            continue
        id_of_lm.append(lid)
        if g >= 0:
            acc, rec, start = st["acc"][lid], st["landmarks"][lid], 1
            rec["flags"] |= FX_MAP_LM_CONTINUED
        else:
            acc, start = [0.0] * 8, 0
            rec = {"n_obs": 0, "first_scan": scan_base + fs, "segment": seg_base + int(poses["segment"][fs]), "flags": 0}
            assert lid == len(st["landmarks"])
            st["acc"].append(acc), st["landmarks"].append(rec)
        for k in range(start, n):
            c, s, tx, ty, tz = pose[fs + k]
            x, y, z = xyz[obs[o + k]]
            wx, wy, wz = (c * x - s * y) + tx, (s * x + c * y) + ty, z + tz
            if g < 0 and k == 0:
                acc[3], acc[4] = wx, wy
            dx, dy = wx - acc[3], wy - acc[4]
            acc[0] += wx
            acc[1] += wy
            acc[2] += wz
            acc[5] += dx
            acc[6] += dy
            acc[7] += (dx * dx + dy * dy)
        rec["n_obs"] += n - start
        added += n - start
        _map_record_from_sums(rec, acc)
        rec["last_scan"] = scan_base + fs + n - 1
    of_row = np.asarray(lor[:rows]).astype(np.int64)
    has = (of_row >= 0) & (of_row < L)
    ids[:rows][has] = np.array(id_of_lm, np.int32)[of_row[has]]
    l_s, h_s = lo(S - 1), hi(S - 1)
    if h_s - l_s <= max_carry:
        keep = S == 1 and accepted
        st["carry"] = [int(ids[l_s + j]) if ids[l_s + j] >= 0 else (st["carry"][j] if keep else -1) for j in range(h_s - l_s)]
        st["carry_kp"], H["carry_rows"] = words[l_s:h_s].copy(), h_s - l_s
    else:
        st["carry"], st["carry_kp"], H["carry_rows"] = [], np.zeros((0, 4), np.uint32), 0
    H["last_new"], H["last_joined"] = n_new, n_joined
    H["n_needed"] += n_new
    H["n_landmarks"] = min(H["n_needed"], cap)
    H["n_obs"] += added
    H["scans"] = scan_base + S
    H["segments"] = seg_base + int(poses["segment"][S - 1]) + 1
    H["last_pose"] = tuple(poses[S - 1].tolist())
    if H["n_needed"] > cap:
        H["flags"] |= FX_MAP_FULL
    if overlap and not accepted:
        H["flags"] |= FX_MAP_OVERLAP_MISMATCH
    if int(th["n_landmarks"]) > max_l:
        H["flags"] |= FX_MAP_TRACK_TRUNCATED
    return st, ids


def map_merge_reference(state, merge_dist=0.30, max_gap_scans=64):
    """The definition of fx_map_merge (include/fx.h) in Python floats over a map_reference state: ONE call, one round.  The state
    is not modified; state["alias"] (missing or short: -1) is kept in the new state, one entry a stored landmark.  Every pair of
    landmarks is looked at (for every h, all g at once as numpy columns): nothing here knows of a grid.
    Returns (the new state, {"proposals", "merged", "live", "reserved"})."""
    import struct
    st = dict(state, header=dict(state["header"]), landmarks=[dict(r) for r in state["landmarks"]], acc=[list(a) for a in state["acc"]],
              carry=list(state["carry"]), carry_kp=state["carry_kp"].copy())
    lms, accs = st["landmarks"], st["acc"]
    N = min(int(st["header"]["n_landmarks"]), len(lms))
    alias = [int(a) for a in st.get("alias", [])][:N]
    alias += [-1] * (N - len(alias))
    md = float(np.float32(merge_dist))
    md2, gap = md * md, int(max_gap_scans)
    if not (math.isfinite(md) and md > 0.0) or gap < 1:
        raise ValueError("merge_dist must be finite and positive, max_gap_scans at least 1")

    def takes_part(i):
        return alias[i] == -1 and lms[i]["n_obs"] >= 1 and math.isfinite(lms[i]["x"]) and math.isfinite(lms[i]["y"])
    part = np.array([takes_part(i) for i in range(N)], bool)
    x, y = (np.array([float(r[f]) for r in lms[:N]], np.float64) for f in ("x", "y"))
    first, last, seg = (np.array([int(r[f]) for r in lms[:N]], np.int64) for f in ("first_scan", "last_scan", "segment"))
    last_p = np.where(part, last, np.int64(1) << 40)  # (a landmark that takes no part precedes nothing)
    first_l = first.tolist()
    bits = lambda d: struct.unpack("<Q", struct.pack("<d", d))[0]
    # proposals: the most recent predecessor, then the nearest (d2 as the bit pattern of a non-negative double), then the lowest id
    prop = {}
    with np.errstate(over="ignore", invalid="ignore"):
        for h in np.flatnonzero(part).tolist():
            cand = np.flatnonzero((last_p < first_l[h]) & (last_p >= first_l[h] - gap) & (seg == seg[h]))
            cand = cand[cand != h]
            if not len(cand):
                continue
            dx, dy = x[cand] - x[h], y[cand] - y[h]
            d2 = dx * dx + dy * dy
            near = d2 <= md2
            best = None
            for g, d in zip(cand[near].tolist(), d2[near].tolist()):
                key = (-int(last[g]), bits(d), g)
                if best is None or key < best:
                    best = key
            if best is not None:
                prop[h] = best[2]
    # acceptance: a g keeps its proposer of lowest (first_scan, id)
    keeps = {}
    for h, g in prop.items():
        key = (int(first[h]) << 32) | h
        if g not in keeps or key < keeps[g]:
            keeps[g] = key
    succ = {g: k & 0xffffffff for g, k in keeps.items()}
    pred = {h: g for g, h in succ.items()}
    absorbed = {}
    for r in sorted(g for g in succ if g not in pred):
        R, A = lms[r], accs[r]
        m = succ[r]
        while m is not None:
            M, B = lms[m], accs[m]
            nm = float(M["n_obs"])
            ex, ey = B[3] - A[3], B[4] - A[4]
            A[0] += B[0]
            A[1] += B[1]
            A[2] += B[2]
            A[7] += ((B[7] + 2.0 * (ex * B[5] + ey * B[6])) + nm * (ex * ex + ey * ey))
            A[5] += (B[5] + nm * ex)
            A[6] += (B[6] + nm * ey)
            R["n_obs"] += M["n_obs"]
            R["last_scan"] = M["last_scan"]
            R["flags"] |= FX_MAP_LM_MERGED | (M["flags"] & FX_MAP_LM_CONTINUED)
            M["flags"] |= FX_MAP_LM_ABSORBED
            alias[m] = absorbed[m] = r
            m = succ.get(m)
        _map_record_from_sums(R, A)
    alias = [absorbed.get(a, a) for a in alias]
    st["carry"] = [alias[c] if 0 <= c < N and alias[c] >= 0 else c for c in st["carry"]]
    st["alias"] = alias
    live = sum(1 for i in range(N) if takes_part(i))
    return st, {"proposals": len(prop), "merged": len(succ), "live": live, "reserved": 0}


# ---- the map compacted, and its whole state as one block of bytes (include/fx.h fx_map_compact, fx_map_export_host)
def map_compact_reference(state, min_obs=1, min_age_scans=64):
    """The definition of fx_map_compact (include/fx.h) in plain loops over a map_reference / map_merge_reference state, which is
    not modified; a state without "alias" has every landmark live.  Returns (the new state, remap int32 [max_landmarks], {"before",
    "kept", "dropped_absorbed", "dropped_live"})."""
    return _map_compact(state, min_obs, min_age_scans)[:3]


def _map_compact(state, min_obs, min_age_scans, condemned=None):
    """fx_map_compact's clauses, which fx_map_retire runs too: condemned(i) (None: no rule) says whether the counters condemn the live
    landmark i; one that no carry word holds is then not kept.  Returns map_compact_reference's three and {"new_id": per old id, -1
    dropped, "retired": the old ids retired, "protected": those the carry held, "retired_obs"}."""
    min_obs, min_age = int(min_obs), int(min_age_scans) & 0xffffffff
    if min_obs < 1:
        raise ValueError("min_obs must be at least 1")
    H = dict(state["header"])
    lms, accs = state["landmarks"], state["acc"]
    N = min(int(H["n_landmarks"]), len(lms))
    alias = [int(a) for a in state.get("alias", [])][:N]
    alias += [-1] * (N - len(alias))

    def root(i):
        return alias[i] if 0 <= alias[i] < N else i
    carry = [int(c) for c in state["carry"]]
    carried = set(root(c) for c in carry[:int(H["carry_rows"])] if 0 <= c < N)
    new_id, K, absorbed, lost_obs = [-1] * N, 0, 0, 0
    retired, protected, retired_obs = [], [], 0
    for i in range(N):
        if alias[i] != -1:
            absorbed += 1
            continue
        age = ((int(H["scans"]) - 1) - int(lms[i]["last_scan"])) & 0xffffffff
        if condemned is not None and condemned(i):
            (protected if i in carried else retired).append(i)
        if retired and retired[-1] == i:
            lost_obs += int(lms[i]["n_obs"])
            retired_obs = (retired_obs + int(lms[i]["n_obs"])) & 0xffffffff
        elif int(lms[i]["n_obs"]) >= min_obs or age < min_age or i in carried:
            new_id[i] = K
            K += 1
        else:
            lost_obs += int(lms[i]["n_obs"])
    st = dict(state, header=H, landmarks=[dict(lms[i]) for i in range(N) if new_id[i] >= 0],
              acc=[list(accs[i]) for i in range(N) if new_id[i] >= 0], alias=[-1] * K, carry_kp=state["carry_kp"].copy())
    st["carry"] = [(new_id[root(c)] if c < N else -1) if c >= 0 else c for c in carry]
    H["n_landmarks"] = H["n_needed"] = K
    H["n_obs"] = (int(H["n_obs"]) - lost_obs) & 0xffffffff
    remap = np.full(int(state["max_landmarks"]), -1, np.int32)
    for i in range(N):
        remap[i] = new_id[root(i)]
    return (st, remap, {"before": N, "kept": K, "dropped_absorbed": absorbed, "dropped_live": N - K - absorbed},
            {"new_id": new_id, "retired": retired, "protected": protected, "retired_obs": retired_obs})


def map_retire_reference(state, expected, seen, min_expected=16, seen_num=1, seen_den=8, dry_run=False):
    """The definition of fx_map_retire (include/fx.h) over a map_reference / ... state, which is not modified: the rule on the
    counters in Python integers (no width to overflow), then map_compact_reference's own clauses with min_obs = 1 (_map_compact: the
    same code).  expected / seen: uint32 [max_landmarks].  Returns (the new state (the old one's content with dry_run), remap int32
    [max_landmarks], retired_of_landmark uint8 [max_landmarks], {"before", "kept", "dropped_absorbed", "retired", "retired_obs",
    "protected_by_carry"}, the new expected, the new seen (copies of the old with dry_run))."""
    min_expected, num, den = int(min_expected), int(seen_num), int(seen_den)
    if not (min_expected >= 1 and 1 <= num <= den):
        raise ValueError("arguments outside what fx_map_retire accepts")
    cap = int(state["max_landmarks"])
    e, sn = (np.asarray(a).astype(np.uint32).reshape(-1) for a in (expected, seen))
    if len(e) != cap or len(sn) != cap:
        raise ValueError("the counter arrays have max_landmarks words")

    def condemned(i):
        return int(e[i]) >= min_expected and int(sn[i]) * den < int(e[i]) * num
    st, remap, res, more = _map_compact(state, 1, 64, condemned)
    mask = np.zeros(cap, np.uint8)
    mask[more["retired"]] = 1
    new_e, new_s = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    for i, k in enumerate(more["new_id"]):
        if k >= 0:
            new_e[k], new_s[k] = e[i], sn[i]
    out = {"before": res["before"], "kept": res["kept"], "dropped_absorbed": res["dropped_absorbed"], "retired": len(more["retired"]),
           "retired_obs": more["retired_obs"], "protected_by_carry": len(more["protected"])}
    if dry_run:
        return state, remap, mask, out, e.copy(), sn.copy()
    return st, remap, mask, out, new_e, new_s


# ---- one map appended to another (include/fx.h fx_map_append)
def append_records(out):
    """The 32 bytes fx_map_append wrote (a device tensor, or an array) as one APPEND_DTYPE record."""
    a = out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:APPEND_DTYPE.itemsize].view(APPEND_DTYPE)[0]


def map_append_reference(dst_state, src_state):
    """The definition of fx_map_append and fx_map_append_host (include/fx.h) in plain loops over two map_reference /
    map_merge_reference / ... states; neither is modified.  Returns (dst's new state, {"id_base", "scan_base", "segment_base",
    "appended", "flags", "carry_rows", "reserved"})."""
    D, S = dst_state["header"], src_state["header"]
    cap, max_carry = int(dst_state["max_landmarks"]), int(dst_state["max_carry_rows"])
    N, M, r = min(int(D["n_landmarks"]), cap), int(S["n_landmarks"]), int(S["carry_rows"])
    Sd, Gd = int(D["scans"]), int(D["segments"])
    top, flags = 0xffffffff, 0
    if int(S["scans"]) == 0:
        flags |= FX_APPEND_EMPTY
    if int(D["n_needed"]) > int(D["n_landmarks"]) or int(S["n_needed"]) > int(S["n_landmarks"]):
        flags |= FX_APPEND_OVERFLOWED
    if N + M > cap:
        flags |= FX_APPEND_NO_ROOM
    if any(int(D[k]) + int(S[k]) > top for k in ("scans", "segments", "batches", "n_obs")):
        flags |= FX_APPEND_TOO_LONG
    res = {"id_base": N, "scan_base": Sd, "segment_base": Gd, "appended": 0, "flags": flags, "carry_rows": int(D["carry_rows"]), "reserved": 0}
    st = dict(dst_state, header=dict(D), landmarks=[dict(R) for R in dst_state["landmarks"]], acc=[list(a) for a in dst_state["acc"]],
              carry=[int(c) for c in dst_state["carry"]], carry_kp=dst_state["carry_kp"].copy())
    alias = [int(a) for a in dst_state.get("alias", [])][:N]
    st["alias"] = alias + [-1] * (N - len(alias))
    if flags:
        return st, res
    src_alias = [int(a) for a in src_state.get("alias", [])][:M]
    src_alias += [-1] * (M - len(src_alias))
    for i in range(M):
        R = dict(src_state["landmarks"][i])
        R["first_scan"] = int(R["first_scan"]) + Sd
        R["last_scan"] = int(R["last_scan"]) + Sd
        R["segment"] = int(R["segment"]) + Gd
        st["landmarks"].append(R), st["acc"].append(list(src_state["acc"][i]))
        st["alias"].append(src_alias[i] + N if src_alias[i] >= 0 else -1)
    H = st["header"]
    if r <= max_carry:
        st["carry"] = [int(c) + N if int(c) >= 0 else -1 for c in list(src_state["carry"])[:r]]
        st["carry_kp"], H["carry_rows"] = np.array(src_state["carry_kp"][:r], np.uint32).reshape(r, 4), r
        flags = FX_APPEND_APPLIED
    else:
        st["carry"], st["carry_kp"], H["carry_rows"] = [], np.zeros((0, 4), np.uint32), 0
        flags = FX_APPEND_APPLIED | FX_APPEND_CARRY_DROPPED
    H["n_landmarks"] = H["n_needed"] = N + M
    for k in ("n_obs", "scans", "batches", "segments"):
        H[k] = int(D[k]) + int(S[k])
    H["flags"] = int(D["flags"]) | int(S["flags"])
    H["last_joined"], H["last_new"], H["last_pose"] = int(S["last_joined"]), int(S["last_new"]), tuple(S["last_pose"])
    res.update(appended=M, flags=flags, carry_rows=H["carry_rows"])
    return st, res


def _pad16(b):
    return b + b"\0" * (-len(b) % 16)


def map_snapshot_pack(state):
    """A map_reference / map_merge_reference / map_compact_reference state as the bytes fx_map_export_host writes for a device map in
    that state (include/fx.h, "The snapshot"): the layout's one statement in Python."""
    import struct
    H = state["header"]
    n, r = int(H["n_landmarks"]), int(H["carry_rows"])
    lms, accs, carry = state["landmarks"], state["acc"], [int(c) for c in state["carry"]]
    if len(lms) != n or len(accs) != n or len(carry) != r or len(state["carry_kp"]) != r:
        raise ValueError(f"the state holds {len(lms)} landmarks and {len(carry)} carry rows, its header says {n} and {r}")
    alias = [int(a) for a in state.get("alias", [])][:n]
    alias += [-1] * (n - len(alias))
    p = H["last_pose"]
    hdr = struct.pack("<10I", *(int(H[k]) & 0xffffffff for k in MAP_HEADER_FIELDS)) + struct.pack("<5d2I", *(float(v) for v in p[:5]), int(p[5]), int(p[6]))
    rec = np.zeros(n, MAP_LANDMARK_DTYPE)
    for i, R in enumerate(lms):
        rec[i] = tuple(R[f] for f in MAP_LANDMARK_DTYPE.names)
    body = [_pad16(hdr), rec.tobytes(), np.array(accs, "<f8").reshape(n, FX_MAP_ACC).tobytes(), _pad16(np.array(alias, "<i4").tobytes()),
            _pad16(np.array(carry, "<i4").tobytes()), np.ascontiguousarray(state["carry_kp"], "<u4").reshape(r, 4).tobytes()]
    total = FX_MAP_SNAPSHOT_HEADER_BYTES + sum(len(b) for b in body)
    head = struct.pack("<10IQ", FX_MAP_SNAPSHOT_MAGIC, FX_MAP_SNAPSHOT_FORMAT, FX_HEADER_VERSION, FX_MAP_SNAPSHOT_HEADER_BYTES, n, r,
                       C.sizeof(FxMapHeader), C.sizeof(FxMapLandmark), FX_MAP_ACC, 0, total)
    return head + b"\0" * (FX_MAP_SNAPSHOT_HEADER_BYTES - len(head)) + b"".join(body)


def map_snapshot_parse(data, max_landmarks=None, max_carry_rows=None):
    """The bytes of a snapshot as a map_reference state ("alias" included); max_landmarks / max_carry_rows: the capacities the
    state is to have (default: what the snapshot holds).  Raises ValueError on a block the layout does not describe (the content
    checks are fx_map_snapshot_check's)."""
    import struct
    data = bytes(data)
    if len(data) < FX_MAP_SNAPSHOT_HEADER_BYTES:
        raise ValueError("shorter than the block header")
    w = struct.unpack_from("<10IQ", data)
    if w[0] != FX_MAP_SNAPSHOT_MAGIC or w[1] != FX_MAP_SNAPSHOT_FORMAT or (w[3], w[6], w[7], w[8]) != (64, 88, 48, FX_MAP_ACC):
        raise ValueError(f"not a format-1 map snapshot: {w}")
    n, r = w[4], w[5]
    up = lambda b: (b + 15) & ~15
    o_rec = 64 + up(88)
    o_acc = o_rec + 48 * n
    o_alias = o_acc + 64 * n
    o_carry = o_alias + up(4 * n)
    o_kp = o_carry + up(4 * r)
    if w[10] != len(data) or len(data) != o_kp + 16 * r:
        raise ValueError(f"total bytes {w[10]}, {len(data)} given, the sections sum to {o_kp + 16 * r}")
    h = struct.unpack_from("<10I5d2I", data, 64)
    hdr = dict(zip(MAP_HEADER_FIELDS, h[:10]))
    hdr["last_pose"] = tuple(h[10:])
    rec = np.frombuffer(data, MAP_LANDMARK_DTYPE, n, o_rec)
    lms = [{f: (np.float32(R[f]) if f == "rms_xy" else float(R[f]) if f in "xyz" else int(R[f])) for f in MAP_LANDMARK_DTYPE.names} for R in rec]
    acc = np.frombuffer(data, "<f8", n * FX_MAP_ACC, o_acc).reshape(n, FX_MAP_ACC).tolist()
    return {"max_landmarks": n if max_landmarks is None else int(max_landmarks), "max_carry_rows": r if max_carry_rows is None else int(max_carry_rows),
            "header": hdr, "landmarks": lms, "acc": acc, "alias": np.frombuffer(data, "<i4", n, o_alias).tolist(),
            "carry": np.frombuffer(data, "<i4", r, o_carry).tolist(), "carry_kp": np.frombuffer(data, "<u4", 4 * r, o_kp).reshape(r, 4).copy()}


# ---- scans localised against the map under a prior pose (include/fx.h fx_map_localize)
def localize_records(out):
    """A host copy of fx_map_localize's records (a torch tensor, or any array of n * 112 bytes) as LOC_DTYPE records."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(LOC_DTYPE).copy()


def _map_consensus(P64, d2_bits, names, tz, qz, hyp_corr, mb2, gate, id2):
    """The hypothesis stage and the refit of fx_map_localize (include/fx.h), which fx_map_join_segments shares, in numpy float64
    over the n correspondences P64 [n, 4] = (qx, qy, tx, ty): d2_bits their association distances as uint64, names what the pool's
    ties and hyp_a / hyp_b go by (rows, landmark ids: ascending), tz and qz the targets' and the points' z.  mb2, gate, id2: the
    gates as float64.  Call it under np.errstate(all="ignore").  Returns None without a hypothesis, else {"fit": (dc, ds, dtx,
    dty), "dtz", "rms": float32, "final": the final inlier set (indices), "hyp": the names of the winning sample}."""
    f64 = np.float64
    n = len(P64)
    H = min(n, int(hyp_corr))
    best = None
    if H >= 2:
        pool = np.lexsort((names, d2_bits))[:H]  # by (d2 bits, name)
        a, c_ = np.triu_indices(H, 1)            # lexicographic (a, b), a < b
        A, B = P64[pool[a]], P64[pool[c_]]
        dqx, dqy, dtx, dty = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1], B[:, 2] - A[:, 2], B[:, 3] - A[:, 3]
        lq2, lt2 = dqx * dqx + dqy * dqy, dtx * dtx + dty * dty
        keep = (lq2 >= mb2) & (lt2 >= mb2)
        keep &= ~(np.abs(np.sqrt(lq2) - np.sqrt(lt2)) > gate)
        dot, crs = dqx * dtx + dqy * dty, dqx * dty - dqy * dtx
        nrm = np.sqrt(dot * dot + crs * crs)
        keep &= nrm > 0
        c, s = dot / nrm, crs / nrm
        half = f64(0.5)
        mqx, mqy, mtx, mty = (A[:, 0] + B[:, 0]) * half, (A[:, 1] + B[:, 1]) * half, (A[:, 2] + B[:, 2]) * half, (A[:, 3] + B[:, 3]) * half
        tx, ty = mtx - (c * mqx - s * mqy), mty - (s * mqx + c * mqy)
        ks = np.flatnonzero(keep)
        counts = np.zeros(len(a), np.int64)
        for lo_ in range(0, len(ks), 512):  # (chunks: [samples, n] temporaries)
            k = ks[lo_:lo_ + 512]
            ck, sk, txk, tyk = c[k, None], s[k, None], tx[k, None], ty[k, None]
            qx, qy, t_x, t_y = P64[None, :, 0], P64[None, :, 1], P64[None, :, 2], P64[None, :, 3]
            rx, ry = ((ck * qx - sk * qy) + txk) - t_x, ((sk * qx + ck * qy) + tyk) - t_y
            counts[k] = (rx * rx + ry * ry <= id2).sum(axis=1)
        counts[counts < 2] = 0  # (a sample with fewer than 2 agreeing is no hypothesis)
        if counts.any():
            best = int(np.argmax(counts))  # (the first maximum: the lowest (a, b))
            rx = ((c[best] * P64[:, 0] - s[best] * P64[:, 1]) + tx[best]) - P64[:, 2]
            ry = ((s[best] * P64[:, 0] + c[best] * P64[:, 1]) + ty[best]) - P64[:, 3]
            I0 = [int(v) for v in np.flatnonzero(rx * rx + ry * ry <= id2)]
            assert len(I0) == int(counts[best])
    if best is None:
        return None
    Pl = [tuple(float(v) for v in row) for row in P64]  # (Python floats: IEEE doubles, the register's refit as it is)
    fit = _register_fit(Pl, I0, float(c[best]), float(s[best]))
    final = I0
    I1 = [k for k in range(n) if _register_r2(Pl, k, *fit) <= float(id2)]
    if len(I1) >= 2:
        fit = _register_fit(Pl, I1, fit[0], fit[1])
        final = I1
    sz = sr = 0.0
    for k in final:
        sz += (float(tz[k]) - float(qz[k]))
        sr += _register_r2(Pl, k, *fit)
    nf = float(len(final))
    return {"fit": fit, "dtz": sz / nf, "rms": np.float32(math.sqrt(sr / nf)), "final": final,
            "hyp": (int(names[pool[a[best]]]), int(names[pool[c_[best]]]))}


def map_localize_reference(state, kp_offset, kp_rows, prior_poses, n_scans, q_max_rows=None, search_dist=2.0, inlier_dist=0.30,
                           min_baseline=2.0, hyp_corr=64, min_inliers=3, min_landmark_obs=2, segment=FX_LOC_LAST_SEGMENT):
    """The definition of fx_map_localize (include/fx.h) in numpy float64 over a map_reference / map_merge_reference state (which is
    only read).  kp_offset / kp_rows: the block's kp_offset[scans + 1] and its [stored, >= 3] float32 rows, already cut to
    min(stored, max_total_keypoints); prior_poses: POSE_DTYPE [>= n_scans]; q_max_rows: the length of the row arrays (default: the
    block's rows).  Every (row, landmark) pair is looked at: nothing here knows of a grid.  One ufunc an operation, so nothing is
    contracted.  Returns {"rec": LOC_DTYPE [n_scans], "map_id_of_row", "nearest_of_row": int32 [q_max_rows], "corr": per scan
    the rows of its correspondences}."""
    f64 = np.float64
    off = [int(x) for x in kp_offset]
    kp = np.ascontiguousarray(kp_rows, dtype=np.float32)
    kp = kp.reshape(len(kp), -1)[:, :3] if kp.size else np.zeros((0, 3), np.float32)
    n_scans = int(n_scans)
    R = len(kp) if q_max_rows is None else int(q_max_rows)
    sd32, id32, mb32 = np.float32(search_dist), np.float32(inlier_dist), np.float32(min_baseline)
    if not (n_scans >= 1 and all(np.isfinite(v) and v > 0 for v in (sd32, id32, mb32)) and 2 <= hyp_corr <= 128 and min_inliers >= 2 and
            min_landmark_obs >= 1):
        raise ValueError("arguments outside what fx_map_localize accepts")
    sd, idd, mbd = f64(sd32), f64(id32), f64(mb32)
    sd2, mb2, gate, id2 = sd * sd, mbd * mbd, f64(2.0) * idd, idd * idd
    prior = np.asarray(prior_poses)[:n_scans]
    S, rows = min(n_scans, len(off) - 1), min(len(kp), R)
    # the eligible landmarks
    lms = state["landmarks"]
    N = min(int(state["header"]["n_landmarks"]), len(lms))
    alias = [int(a) for a in state.get("alias", [])][:N]
    alias += [-1] * (N - len(alias))
    lx, ly, lz = (np.array([float(r[f]) for r in lms[:N]], f64) for f in ("x", "y", "z"))
    want = int(segment) & 0xffffffff
    if want == FX_LOC_LAST_SEGMENT:
        want = int(state["header"]["segments"]) - 1  # (-1 in a map of no segment: nothing is eligible)
    elig = np.array([alias[g] == -1 and int(lms[g]["n_obs"]) >= min_landmark_obs and (want == FX_LOC_ANY_SEGMENT or int(lms[g]["segment"]) == want)
                     for g in range(N)], bool)
    if N:
        elig &= np.isfinite(lx) & np.isfinite(ly) & np.isfinite(lz)
    ids = np.flatnonzero(elig)
    rec = np.zeros(n_scans, LOC_DTYPE)
    rec["pose"] = prior
    rec["dc"], rec["rms"], rec["hyp_a"], rec["hyp_b"] = 1.0, np.inf, FX_LOC_NO_ROW, FX_LOC_NO_ROW
    nearest, map_id = np.full(R, -1, np.int32), np.full(R, -1, np.int32)
    d2_of = np.zeros(R, np.uint64)
    W = np.zeros((R, 3), f64)
    corrs = []
    with np.errstate(all="ignore"):
        for b in range(n_scans):
            P = prior[b]
            if b >= S:
                rec["flags"][b] = FX_LOC_NO_SCAN
                corrs.append(np.zeros(0, np.uint32))
                continue
            pc, ps, ptx, pty, ptz = (f64(P[f]) for f in ("c", "s", "tx", "ty", "tz"))
            if not all(np.isfinite(v) for v in (pc, ps, ptx, pty, ptz)):
                rec["flags"][b] = FX_LOC_BAD_PRIOR
                corrs.append(np.zeros(0, np.uint32))
                continue
            lo = min(off[b], rows)
            hi = max(min(off[b + 1], rows), lo)
            r = np.arange(lo, hi)
            x, y, z = (kp[lo:hi, k].astype(f64) for k in range(3))
            wx, wy, wz = (pc * x - ps * y) + ptx, (ps * x + pc * y) + pty, z + ptz
            W[lo:hi] = np.stack([wx, wy, wz], axis=1)
            fin = np.isfinite(kp[lo:hi]).all(axis=1)
            if len(ids) and len(r):
                dx, dy = lx[ids][None, :] - wx[:, None], ly[ids][None, :] - wy[:, None]
                d2 = dx * dx + dy * dy
                key = np.where(d2 <= sd2, d2, np.inf).view(np.uint64)  # (the bits of +inf are above those of any distance in reach)
                j = np.argmin(key, axis=1)  # (the first minimum: ids ascend, so ties go to the lowest id)
                hit = fin & (d2[np.arange(len(r)), j] <= sd2)
                nearest[lo:hi][hit] = ids[j[hit]]
                d2_of[lo:hi][hit] = d2[np.arange(len(r)), j].view(np.uint64)[hit]
            i = r[nearest[lo:hi] >= 0]
            flags = FX_LOC_TRUNCATED if len(i) > FX_LOC_MAX_CORR else 0
            i = i[:FX_LOC_MAX_CORR]
            n = len(i)
            corrs.append(i.astype(np.uint32))
            rec["n_corr"][b] = n
            g = nearest[i]
            P64 = np.stack([W[i, 0], W[i, 1], lx[g], ly[g]], axis=1) if n else np.zeros((0, 4), f64)  # (qx, qy, tx, ty)
            fitd = _map_consensus(P64, d2_of[i], i, lz[g], W[i, 2], hyp_corr, mb2, gate, id2)
            if fitd is None:
                rec["flags"][b] = flags | FX_LOC_NO_HYPOTHESIS
                continue
            (dc, ds, dtx_, dty_), dtz, final = fitd["fit"], fitd["dtz"], fitd["final"]
            rec["dc"][b], rec["ds"][b], rec["dtx"][b], rec["dty"][b], rec["dtz"][b] = dc, ds, dtx_, dty_, dtz
            rec["rms"][b] = fitd["rms"]
            rec["n_inliers"][b] = len(final)
            valid = len(final) >= min_inliers
            rec["flags"][b] = flags | (FX_LOC_VALID if valid else 0)
            rec["hyp_a"][b], rec["hyp_b"][b] = fitd["hyp"]
            if valid:
                qc, qs, qtx, qty, qtz = (float(v) for v in (pc, ps, ptx, pty, ptz))
                rec["pose"]["c"][b], rec["pose"]["s"][b] = dc * qc - ds * qs, ds * qc + dc * qs
                rec["pose"]["tx"][b], rec["pose"]["ty"][b] = (dc * qtx - ds * qty) + dtx_, (ds * qtx + dc * qty) + dty_
                rec["pose"]["tz"][b] = qtz + dtz
            map_id[i[final]] = g[final]
    return {"rec": rec, "map_id_of_row": map_id, "nearest_of_row": nearest, "corr": corrs}


# ---- chains of scans followed through the map (include/fx.h fx_map_follow)
def follow_records(out):
    """A host copy of fx_map_follow's per-scan records (a torch tensor, or any array of n * 64 bytes) as FOLLOW_DTYPE records."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(FOLLOW_DTYPE).copy()


_POSE5 = ("c", "s", "tx", "ty", "tz")


def map_follow_reference(state, kp_offset, kp_rows, links, start_poses, n_scans, q_max_rows=None, **options):
    """The definition of fx_map_follow (include/fx.h): the chain in Python floats around map_localize_reference called one scan at
    a time (every other scan of such a call has a prior that is not finite and is left out).  The prior is the track's good-link
    composition as track_reference writes it; nothing of the localise is restated.  state, kp_offset, kp_rows, q_max_rows: as in
    map_localize_reference; links: REG_DTYPE [>= n_scans - 1] (may be None where none is read); start_poses: POSE_DTYPE
    [>= n_chains]; options: the fields of fx_follow_options (FOLLOW_DEFAULTS).  Returns {"rec": LOC_DTYPE [n_scans], "follow":
    FOLLOW_DTYPE [n_scans], "poses": POSE_DTYPE [n_scans], "map_id_of_row", "nearest_of_row": int32 [q_max_rows]}."""
    bad = set(options) - set(FOLLOW_DEFAULTS)
    if bad:
        raise TypeError(f"unknown follow options {sorted(bad)}")
    o = dict(FOLLOW_DEFAULTS, **options)
    loc = {k: o[k] for k in LOC_DEFAULTS}
    n_scans, chain, require, max_lost = int(n_scans), int(o["chain_scans"]), int(o["require_flags"]), int(o["max_lost"])
    if n_scans < 1 or chain < 0 or max_lost < 1 or require & ~(FX_REG_VALID | FX_REG_TRUNCATED | FX_REG_NO_HYPOTHESIS):
        raise ValueError("arguments outside what fx_map_follow accepts")
    L = chain if 0 < chain < n_scans else n_scans
    n_chains = -(-n_scans // L)
    if links is None and L > 1:
        raise ValueError("links may be None only when every chain is one scan")
    starts = np.asarray(start_poses)[:n_chains]
    off = [int(x) for x in kp_offset]
    kp = np.ascontiguousarray(kp_rows, dtype=np.float32)
    R = len(kp) if q_max_rows is None else int(q_max_rows)
    S, rows = min(n_scans, len(off) - 1), min(len(kp), R)
    usable = lambda p: (int(links["flags"][p]) & require) == require and all(math.isfinite(float(links[f][p])) for f in _POSE5)
    rec, fol = np.zeros(n_scans, LOC_DTYPE), np.zeros(n_scans, FOLLOW_DTYPE)
    map_id, nearest = np.full(R, -1, np.int32), np.full(R, -1, np.int32)
    for j in range(n_chains):
        last, streak = None, 0
        for b in range(j * L, min((j + 1) * L, n_scans)):
            P = np.zeros(1, POSE_DTYPE)
            flags, motion = FX_FOLLOW_START, FX_FOLLOW_NO_MOTION
            if b == j * L:
                P[0] = starts[j]
            else:
                P[0] = rec["pose"][b - 1]  # p*
                flags = FX_FOLLOW_HELD
                own = usable(b - 1)
                if own:
                    last = b - 1
                pc, ps, ptx, pty, ptz = (float(P[f][0]) for f in _POSE5)
                if last is not None and b < S and all(math.isfinite(v) for v in (pc, ps, ptx, pty, ptz)):
                    rc, rs, rtx, rty, rtz = (float(links[f][last]) for f in _POSE5)
                    new = (pc * rc - ps * rs, ps * rc + pc * rs, (pc * rtx - ps * rty) + ptx, (ps * rtx + pc * rty) + pty, ptz + rtz)  # (track_reference's fold)
                    if all(math.isfinite(v) for v in new):
                        P[0] = new + (int(starts["segment"][j]), 0)
                        flags, motion = (FX_FOLLOW_LINK if own else FX_FOLLOW_COASTED), last
            pri = np.zeros(n_scans, POSE_DTYPE)
            for f in _POSE5:
                pri[f] = np.nan
            pri[b] = P[0]
            one = map_localize_reference(state, off, kp, pri, n_scans, q_max_rows=R, **loc)
            rec[b] = one["rec"][b]
            if b < S:
                lo = min(off[b], rows)
                hi = max(min(off[b + 1], rows), lo)
                map_id[lo:hi], nearest[lo:hi] = one["map_id_of_row"][lo:hi], one["nearest_of_row"][lo:hi]
            streak = 0 if int(rec["flags"][b]) & FX_LOC_VALID else streak + 1
            fol["prior"][b] = P[0]
            fol["flags"][b], fol["motion"][b], fol["streak"][b] = flags | (FX_FOLLOW_LOST if streak >= max_lost else 0), motion, streak
    return {"rec": rec, "follow": fol, "poses": rec["pose"].copy(), "map_id_of_row": map_id, "nearest_of_row": nearest}


# ---- localised scans folded into the map (include/fx.h fx_map_observe)
def observe_records(out):
    """The 32 bytes fx_map_observe wrote (a device tensor, or an array) as a dict of MAP_OBSERVE_RESULT_FIELDS."""
    a = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
    w = np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:32].view("<u4")
    return dict(zip(MAP_OBSERVE_RESULT_FIELDS, (int(v) for v in w)))


def map_observe_reference(state, kp_offset, kp_rows, loc_records, map_id_of_row, n_scans, q_max_rows=None, gate_dist=0.30,
                          require_flags=FX_LOC_VALID, dry_run=False):
    """The definition of fx_map_observe (include/fx.h) in numpy float64 over a map_reference / map_merge_reference / ... state, which
    is not modified.  kp_offset / kp_rows: the block's kp_offset[scans + 1] and its [stored, >= 3] float32 rows, already cut to
    min(stored, max_total_keypoints); loc_records: LOC_DTYPE [>= n_scans]; map_id_of_row: int32 [>= q_max_rows]; q_max_rows: the
    length of the row arrays (default: the block's rows).  Every (row, row) pair of a scan is looked at and every clause is a mask
    over all rows: nothing here knows of counts, cursors or a sort.  One ufunc an operation, so nothing is contracted.
    Returns (the new state (the old one's content with dry_run), {"scans_used", "proposed", "added", "duplicates", "gated", "stale",
    "landmarks_touched", "reserved"}, gained_of_landmark uint32 [max_landmarks], observed_id_of_row int32 [q_max_rows])."""
    f64 = np.float64
    off = [int(x) for x in kp_offset]
    kp = np.ascontiguousarray(kp_rows, dtype=np.float32)
    kp = kp.reshape(len(kp), -1)[:, :3] if kp.size else np.zeros((0, 3), np.float32)
    n_scans = int(n_scans)
    R = len(kp) if q_max_rows is None else int(q_max_rows)
    gd32, req = np.float32(gate_dist), int(require_flags) & 0xffffffff
    known = FX_LOC_VALID | FX_LOC_TRUNCATED | FX_LOC_NO_HYPOTHESIS | FX_LOC_BAD_PRIOR | FX_LOC_NO_SCAN
    if not (n_scans >= 1 and np.isfinite(gd32) and gd32 > 0 and not req & ~known):
        raise ValueError("arguments outside what fx_map_observe accepts")
    gd = f64(gd32)
    gd2 = gd * gd
    st = dict(state, header=dict(state["header"]), landmarks=[dict(r) for r in state["landmarks"]], acc=[list(a) for a in state["acc"]],
              carry=list(state["carry"]), carry_kp=state["carry_kp"].copy())
    if "alias" in state:
        st["alias"] = list(state["alias"])
    lms, accs = st["landmarks"], st["acc"]
    N = min(int(st["header"]["n_landmarks"]), len(lms), int(st["max_landmarks"]))
    alias = np.array([int(a) for a in state.get("alias", [])][:N] + [-1] * max(0, N - len(state.get("alias", []))), np.int64)
    lx, ly, lz = (np.array([float(r[f]) for r in lms[:N]], f64) for f in ("x", "y", "z"))
    ln = np.array([int(r["n_obs"]) for r in lms[:N]], np.int64)
    loc = np.asarray(loc_records)[:n_scans]
    S, rows = min(n_scans, len(off) - 1), min(len(kp), R)
    ids = np.asarray(map_id_of_row)[:rows].astype(np.int64)
    # the scan of every row, -1: a non-row; the used scans
    scan = np.full(rows, -1, np.int64)
    for b in range(S):
        lo = min(off[b], rows)
        scan[lo:max(min(off[b + 1], rows), lo)] = b
    P = loc["pose"][:S]
    used = np.array([(int(loc["flags"][b]) & req) == req and all(np.isfinite(f64(P[f][b])) for f in ("c", "s", "tx", "ty", "tz")) for b in range(S)], bool)
    with np.errstate(all="ignore"):
        sc = np.where(scan >= 0, scan, 0)
        in_used = (scan >= 0) & (used[sc] if S else np.zeros(rows, bool))
        proposes = in_used & np.isfinite(kp[:rows]).all(axis=1) & (ids >= 0) & (ids < N)
        idc = np.where(proposes, ids, 0)
        via = alias[idc] if N else np.zeros(rows, np.int64)
        g = np.where(via >= 0, via, idc)
        gc = np.where(g < N, g, 0)
        if N:
            live = (g < N) & (alias[gc] == -1) & (ln[gc] >= 1) & np.isfinite(lx[gc]) & np.isfinite(ly[gc]) & np.isfinite(lz[gc])
        else:
            live = np.zeros(rows, bool)
        stale = proposes & ~live
        # the world points under the scans' poses, the gate against the records as they are
        x, y, z = (kp[:rows, k].astype(f64) for k in range(3))
        pc, ps, ptx, pty, ptz = ((P[f][sc].astype(f64) if S else np.zeros(rows, f64)) for f in ("c", "s", "tx", "ty", "tz"))
        wx, wy, wz = (pc * x - ps * y) + ptx, (ps * x + pc * y) + pty, z + ptz
        if N:
            dx, dy = lx[gc] - wx, ly[gc] - wy
        else:
            dx = dy = np.zeros(rows, f64)
        d2 = dx * dx + dy * dy
        passes = proposes & live & (d2 <= gd2)
        gated = proposes & live & ~passes
    # one observation a scan a landmark: a passing proposal is kept unless another of its scan and its landmark is lower in (d2 bits, row)
    bits = np.ascontiguousarray(d2).view(np.uint64)
    kept = passes.copy()
    r_all = np.arange(rows)
    for b in np.unique(scan[passes]).tolist():
        i = np.flatnonzero(passes & (scan == b))
        same = g[i][:, None] == g[i][None, :]
        lower = (bits[i][None, :] < bits[i][:, None]) | ((bits[i][None, :] == bits[i][:, None]) & (r_all[i][None, :] < r_all[i][:, None]))
        kept[i] = ~(same & lower).any(axis=1)
    observed = np.full(R, -1, np.int32)
    observed[:rows][kept] = g[kept]
    gained = np.zeros(int(st["max_landmarks"]), np.uint32)
    touched = 0
    W = np.stack([wx, wy, wz], axis=1).tolist() if rows else []
    for t in sorted(set(g[kept].tolist())):
        mine = np.flatnonzero(kept & (g == t)).tolist()  # (ascending row)
        gained[t] = len(mine)
        touched += 1
        if dry_run:
            continue
        acc, rec = accs[t], lms[t]
        for r in mine:
            ox, oy, oz = W[r]
            ddx, ddy = ox - acc[3], oy - acc[4]
            acc[0] += ox
            acc[1] += oy
            acc[2] += oz
            acc[5] += ddx
            acc[6] += ddy
            acc[7] += (ddx * ddx + ddy * ddy)
        rec["n_obs"] += len(mine)
        _map_record_from_sums(rec, acc)
        rec["flags"] |= FX_MAP_LM_OBSERVED
    added = int(kept.sum())
    if not dry_run:
        st["header"]["n_obs"] = (int(st["header"]["n_obs"]) + added) & 0xffffffff
    res = {"scans_used": int(used.sum()), "proposed": int(proposes.sum()), "added": added, "duplicates": int(passes.sum()) - added,
           "gated": int(gated.sum()), "stale": int(stale.sum()), "landmarks_touched": touched, "reserved": 0}
    return st, res, gained, observed


# ---- negative evidence: how often a landmark should have been seen and how often it was (include/fx.h fx_map_expect)
def expect_records(out):
    """The 32 bytes fx_map_expect wrote (a device tensor, or an array) as a dict of MAP_EXPECT_RESULT_FIELDS."""
    a = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
    w = np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:32].view("<u4")
    return dict(zip(MAP_EXPECT_RESULT_FIELDS, (int(v) for v in w)))


def retire_records(out):
    """The 32 bytes fx_map_retire wrote (a device tensor, or an array) as a dict of MAP_RETIRE_RESULT_FIELDS; the reserved words must be 0."""
    a = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
    w = np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:32].view("<u4")
    if w[6] or w[7]:
        raise ValueError("fx_map_retire_result.reserved is not 0")
    return dict(zip(MAP_RETIRE_RESULT_FIELDS, (int(v) for v in w[:6])))


def map_expect_reference(state, kp_offset, kp_rows, loc_records, map_id_of_row, n_scans, q_max_rows=None, expected=None, seen=None, **opts):
    """The definition of fx_map_expect (include/fx.h) in numpy float64 over a map_reference / ... state, which is only read.  The
    arguments are map_observe_reference's; opts: the fields of fx_map_expect_options (EXPECT_DEFAULTS).  expected / seen: the arrays
    an FX_EXPECT_ADD call adds to (uint32 [max_landmarks]; not modified).  Every (used scan, eligible landmark) pair and every (pair,
    row) triple is looked at: nothing here knows of a grid, a cell or a bucket.  One ufunc an operation, so nothing is contracted.
    Returns ({"scans_used", "in_range", "in_box", "shadowed", "expected", "seen", "stale", "landmarks_expected"}, expected_of_landmark,
    seen_of_landmark uint32 [max_landmarks])."""
    f64 = np.float64
    bad = set(opts) - set(EXPECT_DEFAULTS)
    if bad:
        raise TypeError(f"unknown expect options {sorted(bad)}")
    o = dict(EXPECT_DEFAULTS, **opts)
    off = [int(x) for x in kp_offset]
    kp = np.ascontiguousarray(kp_rows, dtype=np.float32)
    kp = kp.reshape(len(kp), -1)[:, :3] if kp.size else np.zeros((0, 3), np.float32)
    n_scans = int(n_scans)
    R = len(kp) if q_max_rows is None else int(q_max_rows)
    x_min, x_max, y_min, y_max, r_lo, r_hi, sw = (np.float32(o[k]) for k in ("x_min", "x_max", "y_min", "y_max", "min_range", "max_range", "shadow_width"))
    req, min_obs, segment, mode = (int(o[k]) & 0xffffffff for k in ("require_flags", "min_landmark_obs", "segment", "mode"))
    known = FX_LOC_VALID | FX_LOC_TRUNCATED | FX_LOC_NO_HYPOTHESIS | FX_LOC_BAD_PRIOR | FX_LOC_NO_SCAN
    if not (n_scans >= 1 and x_min <= x_max and y_min <= y_max and np.isfinite(r_lo) and r_lo >= 0 and np.isfinite(r_hi) and r_hi > 0 and
            r_hi >= r_lo and np.isfinite(sw) and sw >= 0 and not req & ~known and min_obs >= 1 and mode <= 1):
        raise ValueError("arguments outside what fx_map_expect accepts")
    bx0, bx1, by0, by1 = f64(x_min), f64(x_max), f64(y_min), f64(y_max)
    lo2, hi2, w2 = f64(r_lo) * f64(r_lo), f64(r_hi) * f64(r_hi), f64(sw) * f64(sw)
    lms, H = state["landmarks"], state["header"]
    cap = int(state["max_landmarks"])
    N = min(int(H["n_landmarks"]), len(lms), cap)
    alias = np.array([int(a) for a in state.get("alias", [])][:N] + [-1] * max(0, N - len(state.get("alias", []))), np.int64)
    X, Y, Z = (np.array([float(r[f]) for r in lms[:N]], f64) for f in ("x", "y", "z"))
    ln = np.array([int(r["n_obs"]) for r in lms[:N]], np.int64)
    lseg = np.array([int(r["segment"]) for r in lms[:N]], np.int64)
    if segment == FX_LOC_ANY_SEGMENT:
        seg_ok = np.ones(N, bool)
    elif segment == FX_LOC_LAST_SEGMENT:
        seg_ok = (lseg == int(H["segments"]) - 1) if int(H["segments"]) else np.zeros(N, bool)
    else:
        seg_ok = lseg == segment
    eligible = (alias == -1) & (ln >= min_obs) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & seg_ok
    loc = np.asarray(loc_records)[:n_scans]
    S, rows = min(n_scans, len(off) - 1), min(len(kp), R)
    ids = np.asarray(map_id_of_row)[:rows].astype(np.int64)
    P = loc["pose"][:S]
    used = [(int(loc["flags"][b]) & req) == req and all(np.isfinite(f64(P[f][b])) for f in ("c", "s", "tx", "ty", "tz")) for b in range(S)]
    cnt_e, cnt_s = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    res = {k: 0 for k in MAP_EXPECT_RESULT_FIELDS}
    G = np.flatnonzero(eligible)
    with np.errstate(all="ignore"):
        for b in range(S):
            if not used[b]:
                continue
            res["scans_used"] += 1
            q_lo = min(off[b], rows)
            q_hi = max(min(off[b + 1], rows), q_lo)
            k = kp[q_lo:q_hi]
            fin = np.isfinite(k).all(axis=1)
            idb = ids[q_lo:q_hi]
            proposes = fin & (idb >= 0) & (idb < N)
            idc = np.where(proposes, idb, 0)
            via = alias[idc] if N else np.zeros(len(idc), np.int64)
            tgt = np.where(via >= 0, via, idc)
            ok = proposes & (tgt < N) & (eligible[np.where(tgt < N, tgt, 0)] if N else False)
            res["stale"] += int((proposes & ~ok).sum())
            name = np.where(ok, tgt, -1)  # the landmark a row names, -1: none
            c, s, tx, ty = (f64(P[f][b]) for f in ("c", "s", "tx", "ty"))
            dx, dy = X[G] - tx, Y[G] - ty
            d2 = (dx * dx) + (dy * dy)
            lx, ly = (c * dx) + (s * dy), (c * dy) - (s * dx)
            l2 = (lx * lx) + (ly * ly)
            in_range = (lo2 <= d2) & (d2 <= hi2)
            in_box = (bx0 <= lx) & (lx <= bx1) & (by0 <= ly) & (ly <= by1)
            names_g = name[None, :] == G[:, None]  # [landmark, row]
            seen_g = in_range & names_g.any(axis=1)
            kx, ky = k[:, 0].astype(f64), k[:, 1].astype(f64)
            k2 = (kx * kx) + (ky * ky)
            along = (kx[None, :] * lx[:, None]) + (ky[None, :] * ly[:, None])
            crs = (kx[None, :] * ly[:, None]) - (ky[None, :] * lx[:, None])
            shadow = fin[None, :] & ~names_g & (k2[None, :] < l2[:, None]) & (along > 0) & ((crs * crs) <= (w2 * l2)[:, None])
            shadowed = shadow.any(axis=1) if sw > 0 else np.zeros(len(G), bool)
            exp_g = in_range & (seen_g | (in_box & ~shadowed))
            res["in_range"] += int(in_range.sum())
            res["in_box"] += int((in_range & in_box).sum())
            res["shadowed"] += int((in_range & in_box & ~seen_g & shadowed).sum())
            res["expected"] += int(exp_g.sum())
            res["seen"] += int(seen_g.sum())
            cnt_e[G[exp_g]] += 1
            cnt_s[G[seen_g]] += 1
    res["landmarks_expected"] = int((cnt_e > 0).sum())
    if mode == FX_EXPECT_ADD:
        base_e, base_s = (np.asarray(a).astype(np.int64).reshape(-1) for a in (expected, seen))
        if len(base_e) != cap or len(base_s) != cap:
            raise ValueError("the counter arrays have max_landmarks words")
        cnt_e, cnt_s = (base_e + cnt_e) & 0xffffffff, (base_s + cnt_s) & 0xffffffff
    return res, cnt_e.astype(np.uint32), cnt_s.astype(np.uint32)


# ---- new poles learnt from the unexplained rows of localised scans (include/fx.h fx_map_discover)
def discover_records(out):
    """The 64 bytes fx_map_discover wrote (a device tensor, or an array) as a dict of MAP_DISCOVER_RESULT_FIELDS; the reserved words must be 0."""
    a = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
    w = np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:64].view("<u4")
    if w[14] or w[15]:
        raise ValueError("fx_map_discover_result.reserved is not 0")
    return dict(zip(MAP_DISCOVER_RESULT_FIELDS, (int(v) for v in w[:14])))


def map_discover_reference(state, kp_offset, kp_rows, loc_records, map_id_of_row, n_scans, q_max_rows=None, dry_run=False, **opts):
    """The definition of fx_map_discover (include/fx.h) in numpy float64 over a map_reference / ... state, which is not modified.  The
    arguments are map_observe_reference's; opts: the fields of fx_map_discover_options (DISCOVER_DEFAULTS) but mode, which is dry_run.
    Every (row, landmark) pair and every (free row, free row) pair is looked at and every clause is a mask over all of them: nothing
    here knows of a grid, a prefix or a list.  One ufunc an operation, so nothing is contracted.
    Returns (the new state (the old one's content with dry_run, or when the call is refused), a dict of MAP_DISCOVER_RESULT_FIELDS,
    new_id_of_row int32 [q_max_rows])."""
    f64 = np.float64
    bad = set(opts) - (set(DISCOVER_DEFAULTS) - {"mode"})
    if bad:
        raise TypeError(f"unknown discover options {sorted(bad)}")
    o = dict(DISCOVER_DEFAULTS, **opts)
    off = [int(x) for x in kp_offset]
    kp = np.ascontiguousarray(kp_rows, dtype=np.float32)
    kp = kp.reshape(len(kp), -1)[:, :3] if kp.size else np.zeros((0, 3), np.float32)
    n_scans = int(n_scans)
    R = len(kp) if q_max_rows is None else int(q_max_rows)
    kd32, jd32 = np.float32(o["known_dist"]), np.float32(o["join_dist"])
    min_obs, req, segment = (int(o[k]) & 0xffffffff for k in ("min_obs", "require_flags", "segment"))
    flags_known = FX_LOC_VALID | FX_LOC_TRUNCATED | FX_LOC_NO_HYPOTHESIS | FX_LOC_BAD_PRIOR | FX_LOC_NO_SCAN
    if not (n_scans >= 1 and np.isfinite(kd32) and kd32 > 0 and np.isfinite(jd32) and jd32 > 0 and f64(kd32) >= f64(2.0) * f64(jd32) and
            min_obs >= 1 and not req & ~flags_known and segment != FX_LOC_ANY_SEGMENT):
        raise ValueError("arguments outside what fx_map_discover accepts")
    kd2, jd2 = f64(kd32) * f64(kd32), f64(jd32) * f64(jd32)
    st = dict(state, header=dict(state["header"]), landmarks=[dict(r) for r in state["landmarks"]], acc=[list(a) for a in state["acc"]],
              carry=list(state["carry"]), carry_kp=state["carry_kp"].copy())
    if "alias" in state:
        st["alias"] = list(state["alias"])
    H, lms, cap = st["header"], st["landmarks"], int(st["max_landmarks"])
    first_id = int(H["n_needed"])
    res = dict({k: 0 for k in MAP_DISCOVER_RESULT_FIELDS}, first_id=first_id)
    new_id = np.full(R, -1, np.int32)
    seg = int(H["segments"]) - 1 if segment == FX_LOC_LAST_SEGMENT else segment
    if seg < 0 or seg >= int(H["segments"]):
        res["refused"] = 1
        return st, res, new_id
    N = min(int(H["n_landmarks"]), len(lms), cap)
    alias = np.array([int(a) for a in state.get("alias", [])][:N] + [-1] * max(0, N - len(state.get("alias", []))), np.int64)
    lx, ly = (np.array([float(r[f]) for r in lms[:N]], f64) for f in ("x", "y"))
    ln, lseg = (np.array([int(r[f]) for r in lms[:N]], np.int64) for f in ("n_obs", "segment"))
    loc = np.asarray(loc_records)[:n_scans]
    S, rows = min(n_scans, len(off) - 1), min(len(kp), R)
    ids = np.asarray(map_id_of_row)[:rows].astype(np.int64)
    scan = np.full(rows, -1, np.int64)  # the scan of every row, -1: a non-row
    for b in range(S):
        lo = min(off[b], rows)
        scan[lo:max(min(off[b + 1], rows), lo)] = b
    P = loc["pose"][:S]
    used = np.array([(int(loc["flags"][b]) & req) == req and all(np.isfinite(f64(P[f][b])) for f in ("c", "s", "tx", "ty", "tz")) for b in range(S)], bool)
    with np.errstate(all="ignore"):
        sc = np.where(scan >= 0, scan, 0)
        in_used = (scan >= 0) & (used[sc] if S else np.zeros(rows, bool))
        x, y, z = (kp[:rows, k].astype(f64) for k in range(3))
        pc, ps, ptx, pty, ptz = ((P[f][sc].astype(f64) if S else np.zeros(rows, f64)) for f in ("c", "s", "tx", "ty", "tz"))
        wx, wy, wz = (pc * x - ps * y) + ptx, (ps * x + pc * y) + pty, z + ptz
        unmatched = in_used & np.isfinite(kp[:rows]).all(axis=1) & (ids < 0) & np.isfinite(wx) & np.isfinite(wy) & np.isfinite(wz)
        # known: some live landmark of the segment within kd
        live = np.flatnonzero((alias == -1) & (ln >= 1) & np.isfinite(lx) & np.isfinite(ly) & (lseg == seg))
        U = np.flatnonzero(unmatched)
        dx, dy = lx[live][None, :] - wx[U][:, None], ly[live][None, :] - wy[U][:, None]
        known = ((dx * dx + dy * dy) <= kd2).any(axis=1)
        F = U[~known]  # the free rows, ascending
        n = len(F)
        # every pair of free rows: [r, r'] is the d2 of r' from r
        dx, dy = wx[F][None, :] - wx[F][:, None], wy[F][None, :] - wy[F][:, None]
        d2 = dx * dx + dy * dy
        near = d2 <= jd2
    bits = np.ascontiguousarray(d2).view(np.uint64).reshape(n, n)
    idx = np.arange(n)
    leader = ~(near & (idx[None, :] < idx[:, None])).any(axis=1)
    # attachment: the leader within jd of lowest (d2 bits, leader row); argmin takes the first of equals, which is the lowest row
    cand = near & leader[None, :]
    attached = cand.any(axis=1)
    att = np.where(attached, np.where(cand, bits, np.uint64(0xffffffffffffffff)).argmin(axis=1) if n else idx, -1)
    abits = bits[idx, np.where(attached, att, 0)] if n else np.zeros(0, np.uint64)
    # one observation a scan a leader: the lowest (d2 bits, row)
    fscan = scan[F]
    same = attached[:, None] & attached[None, :] & (att[:, None] == att[None, :]) & (fscan[:, None] == fscan[None, :])
    lower = (abits[None, :] < abits[:, None]) | ((abits[None, :] == abits[:, None]) & (idx[None, :] < idx[:, None]))
    kept = attached & ~(same & lower).any(axis=1)
    support = np.array([int((kept & (att == l)).sum()) for l in range(n)], np.int64)
    confirmed = [l for l in range(n) if leader[l] and support[l] >= min_obs]
    res.update(scans_used=int(used.sum()), unmatched=len(U), known=int(known.sum()), free_rows=n, leaders=int(leader.sum()),
               orphans=int((~attached).sum()), duplicates=int((attached & ~kept).sum()),
               weak=int(sum(support[l] for l in range(n) if leader[l] and support[l] < min_obs)))
    scan_now = int(H["scans"]) - 1 if int(H["scans"]) else 0
    W = np.stack([wx, wy, wz], axis=1).tolist() if rows else []
    for i, l in enumerate(confirmed):
        lid = first_id + i
        mine = np.flatnonzero(kept & (att == l)).tolist()  # (ascending row; the first is the leader)
        if lid >= cap:
            res["not_stored"] += 1
            res["lost"] += len(mine)
            continue
        res["created"] += 1
        res["added"] += len(mine)
        new_id[F[mine]] = lid
        if dry_run:
            continue
        acc = [0.0] * 8
        acc[3], acc[4] = W[F[mine[0]]][0], W[F[mine[0]]][1]
        for j in mine:
            ox, oy, oz = W[F[j]]
            ddx, ddy = ox - acc[3], oy - acc[4]
            acc[0] += ox
            acc[1] += oy
            acc[2] += oz
            acc[5] += ddx
            acc[6] += ddy
            acc[7] += (ddx * ddx + ddy * ddy)
        rec = {"n_obs": len(mine), "first_scan": scan_now, "last_scan": scan_now, "segment": seg, "flags": FX_MAP_LM_DISCOVERED}
        _map_record_from_sums(rec, acc)
        assert lid == len(lms), "a stored id is the next landmark"
        lms.append(rec), st["acc"].append(acc)
        if "alias" in st:
            st["alias"] = (st["alias"][:lid] + [-1] * lid)[:lid] + [-1]
    if not dry_run:
        H["n_needed"] = (first_id + len(confirmed)) & 0xffffffff
        H["n_landmarks"] = min(H["n_needed"], cap)
        H["n_obs"] = (int(H["n_obs"]) + res["added"]) & 0xffffffff
        if res["not_stored"]:
            H["flags"] |= FX_MAP_FULL
    return st, res, new_id


# ---- two segments of the map made one (include/fx.h fx_map_join_segments)
def join_records(out):
    """A host copy of fx_map_join_segments's result (a torch tensor, or any array of 120 bytes) as a JOIN_DTYPE record array [1]."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(JOIN_DTYPE).copy()


def map_join_reference(state, src, dst, prior=None, **opts):
    """The definition of fx_map_join_segments (include/fx.h) in numpy float64 and Python floats over a map_reference /
    map_merge_reference state, which is not modified.  prior: (c, s, tx, ty, tz) or None, the identity (a prior that is not finite is
    the device refusal FX_JOIN_BAD_PRIOR: what a prior_device gives); opts: the fields of fx_map_join_options (JOIN_DEFAULTS).
    Every (query, target) pair is looked at: nothing here knows of a grid.  Returns (the new state, the result: a JOIN_DTYPE
    record, match_of_landmark int32 [max_landmarks])."""
    f64 = np.float64
    bad = set(opts) - set(JOIN_DEFAULTS)
    if bad:
        raise TypeError(f"unknown join options {sorted(bad)}")
    o = dict(JOIN_DEFAULTS, **opts)
    src, dst, mode = int(src), int(dst), int(o["mode"])
    sd32, id32, mb32 = np.float32(o["search_dist"]), np.float32(o["inlier_dist"]), np.float32(o["min_baseline"])
    if src == dst or not (all(np.isfinite(v) and v > 0 for v in (sd32, id32, mb32)) and 2 <= o["hyp_corr"] <= 128 and o["min_inliers"] >= 2 and
                          o["min_landmark_obs"] >= 1 and 0 <= mode <= 2):
        raise ValueError("arguments outside what fx_map_join_segments accepts")
    sd, idd, mbd = f64(sd32), f64(id32), f64(mb32)
    sd2, mb2, gate, id2 = sd * sd, mbd * mbd, f64(2.0) * idd, idd * idd
    st = dict(state, header=dict(state["header"]), landmarks=[dict(r) for r in state["landmarks"]], acc=[list(a) for a in state["acc"]],
              carry=list(state["carry"]), carry_kp=state["carry_kp"].copy())
    H, lms, accs = st["header"], st["landmarks"], st["acc"]
    N, SEG = min(int(H["n_landmarks"]), len(lms)), int(H["segments"])
    alias = [int(a) for a in st.get("alias", [])][:N]
    alias += [-1] * (N - len(alias))
    st["alias"] = alias
    P = tuple(float(v) for v in (prior if prior is not None else (1.0, 0.0, 0.0, 0.0, 0.0)))[:5]
    res = np.zeros(1, JOIN_DTYPE)[0]
    res["c"], res["s"], res["tx"], res["ty"], res["tz"] = P
    res["dc"], res["rms"], res["label"], res["hyp_a"], res["hyp_b"], res["segments"] = 1.0, np.inf, FX_JOIN_NONE, FX_JOIN_NONE, FX_JOIN_NONE, SEG
    match = np.full(int(st["max_landmarks"]), -1, np.int32)
    refuse = (FX_JOIN_BAD_SEGMENT if src >= SEG or dst >= SEG else 0) | (0 if all(math.isfinite(v) for v in P) else FX_JOIN_BAD_PRIOR)
    if refuse:
        res["flags"] = refuse
        return st, res, match
    pc, ps, ptx, pty, ptz = P
    T, flags = P, 0
    if mode != FX_JOIN_GIVEN:
        seg = np.array([int(r["segment"]) for r in lms[:N]], np.int64)
        lx, ly, lz = (np.array([float(r[f]) for r in lms[:N]], f64) for f in ("x", "y", "z"))
        elig = np.array([alias[g] == -1 and int(lms[g]["n_obs"]) >= o["min_landmark_obs"] for g in range(N)], bool)
        if N:
            elig &= np.isfinite(lx) & np.isfinite(ly) & np.isfinite(lz)
        q, t = np.flatnonzero(elig & (seg == src)), np.flatnonzero(elig & (seg == dst))
        res["n_src"] = len(q)
        with np.errstate(all="ignore"):
            cc, ss, tx_, ty_, tz_ = (f64(v) for v in P)
            wx, wy, wz = (cc * lx[q] - ss * ly[q]) + tx_, (ss * lx[q] + cc * ly[q]) + ty_, lz[q] + tz_
            near, d2_of = np.full(len(q), -1, np.int64), np.zeros(len(q), np.uint64)
            if len(q) and len(t):
                for lo in range(0, len(q), 256):  # (chunks: [queries, targets] temporaries)
                    hi = min(lo + 256, len(q))
                    dx, dy = lx[t][None, :] - wx[lo:hi, None], ly[t][None, :] - wy[lo:hi, None]
                    d2 = dx * dx + dy * dy
                    key = np.where(d2 <= sd2, d2, np.inf).view(np.uint64)  # (the bits of +inf are above those of any distance in reach)
                    j = np.argmin(key, axis=1)  # (the first minimum: ids ascend, so ties go to the lowest id)
                    dj = d2[np.arange(hi - lo), j]
                    hit = dj <= sd2
                    near[lo:hi][hit] = t[j[hit]]
                    d2_of[lo:hi][hit] = dj.view(np.uint64)[hit]
            k = np.flatnonzero(near >= 0)
            flags = FX_JOIN_TRUNCATED if len(k) > FX_JOIN_MAX_CORR else 0
            k = k[:FX_JOIN_MAX_CORR]
            n = len(k)
            res["n_corr"] = n
            g = near[k]
            P64 = np.stack([wx[k], wy[k], lx[g], ly[g]], axis=1) if n else np.zeros((0, 4), f64)
            fitd = _map_consensus(P64, d2_of[k], q[k], lz[g], wz[k], o["hyp_corr"], mb2, gate, id2)
        if fitd is None:
            flags |= FX_JOIN_NO_HYPOTHESIS
        else:
            (dc, ds, dtx, dty), dtz, final = fitd["fit"], fitd["dtz"], fitd["final"]
            res["dc"], res["ds"], res["dtx"], res["dty"], res["dtz"], res["rms"] = dc, ds, dtx, dty, dtz, fitd["rms"]
            res["n_inliers"] = len(final)
            res["hyp_a"], res["hyp_b"] = fitd["hyp"]
            match[q[k[final]]] = g[final]
            if len(final) >= o["min_inliers"]:
                flags |= FX_JOIN_FITTED
                T = (dc * pc - ds * ps, ds * pc + dc * ps, (dc * ptx - ds * pty) + dtx, (ds * ptx + dc * pty) + dty, ptz + dtz)
    res["c"], res["s"], res["tx"], res["ty"], res["tz"] = T
    applied = mode == FX_JOIN_GIVEN or (mode == FX_JOIN_FIT and bool(flags & FX_JOIN_FITTED))
    if applied:
        flags |= FX_JOIN_APPLIED
        c, s, tx, ty, tz = T
        lo, hi = min(src, dst), max(src, dst)
        moved = 0
        for i in range(N):
            R, A = lms[i], accs[i]
            if int(R["segment"]) == src:
                moved += 1
                n = float(R["n_obs"])
                sx, sy, sz = (c * A[0] - s * A[1]) + n * tx, (s * A[0] + c * A[1]) + n * ty, A[2] + n * tz
                ax, ay = (c * A[3] - s * A[4]) + tx, (s * A[3] + c * A[4]) + ty
                dx, dy = c * A[5] - s * A[6], s * A[5] + c * A[6]
                A[:7] = [sx, sy, sz, ax, ay, dx, dy]
                if int(R["n_obs"]):
                    _map_record_from_sums(R, A)
            sg = int(R["segment"])
            R["segment"] = hi - 1 if sg == lo else (sg - 1 if sg > lo else sg)
        if SEG - 1 == src:
            lc, ls, ltx, lty, ltz = (float(v) for v in H["last_pose"][:5])
            H["last_pose"] = (c * lc - s * ls, s * lc + c * ls, (c * ltx - s * lty) + tx, (s * ltx + c * lty) + ty, ltz + tz) + tuple(H["last_pose"][5:])
        H["segments"] = SEG - 1
        res["moved"], res["label"], res["segments"] = moved, hi - 1, SEG - 1
    res["flags"] = flags
    return st, res, match


# ---- a loop closed in the map (include/fx.h fx_map_close_loop, fx_map_loop_correct_poses)
def loop_records(out):
    """A host copy of fx_map_close_loop's result (a torch tensor, or any array of 144 bytes) as a LOOP_DTYPE record array [1]."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(LOOP_DTYPE).copy()


def _loop_weight(t2, s0, s1):
    """include/fx.h "Weight of a global scan interval": t2 = first_scan + last_scan as an integer."""
    t2, a, b = int(t2), 2 * int(s0), 2 * int(s1)
    if t2 <= a:
        return 0.0
    if t2 >= b:
        return 1.0
    return float(t2 - a) / float(b - a)


def _loop_transform(T, px, py, alpha):
    """include/fx.h "Interpolated transform": T_alpha of T = (c, s, tx, ty, tz) about the pivot, Python floats in the clause's order."""
    c, s, tx, ty, tz = T
    if alpha == 1.0:
        return T
    cu, su = (1.0 - alpha) + alpha * c, alpha * s
    nrm = math.sqrt(cu * cu + su * su)
    ca, sa = cu / nrm, su / nrm
    gx, gy = (c * px - s * py) + tx, (s * px + c * py) + ty
    hx, hy = px + alpha * (gx - px), py + alpha * (gy - py)
    return (ca, sa, hx - (ca * px - sa * py), hy - (sa * px + ca * py), alpha * tz)


def _rigid_compose(p, r):
    """p o r by fx_map_localize's Pose clause."""
    return (p[0] * r[0] - p[1] * r[1], p[1] * r[0] + p[0] * r[1], (p[0] * r[2] - p[1] * r[3]) + p[2], (p[1] * r[2] + p[0] * r[3]) + p[3], r[4] + p[4])


def map_loop_reference(state, prior=None, **opts):
    """The definition of fx_map_close_loop (include/fx.h) in numpy float64 and Python floats over a map_reference /
    map_merge_reference state, which is not modified.  prior: (c, s, tx, ty, tz) or None, the identity (a prior that is not finite is
    the device refusal FX_LOOP_BAD_PRIOR: what a prior_device gives); opts: the fields of fx_map_loop_options (LOOP_DEFAULTS).
    Every (query, target) pair is looked at: nothing here knows of a grid.  Returns (the new state, the result: a LOOP_DTYPE
    record, match_of_landmark int32 [max_landmarks])."""
    f64 = np.float64
    bad = set(opts) - set(LOOP_DEFAULTS)
    if bad:
        raise TypeError(f"unknown loop options {sorted(bad)}")
    o = dict(LOOP_DEFAULTS, **opts)
    mode, want = int(o["mode"]), int(o["segment"])
    sd32, id32, mb32 = np.float32(o["search_dist"]), np.float32(o["inlier_dist"]), np.float32(o["min_baseline"])
    if not (all(np.isfinite(v) and v > 0 for v in (sd32, id32, mb32)) and 2 <= o["hyp_corr"] <= 128 and o["min_inliers"] >= 2 and
            o["min_landmark_obs"] >= 1 and 0 <= mode <= 2 and 0 <= o["recent_scans"] < o["min_loop_scans"] and want != FX_LOC_ANY_SEGMENT):
        raise ValueError("arguments outside what fx_map_close_loop accepts")
    if mode == FX_LOOP_GIVEN and not (0 <= o["loop_first_scan"] < o["loop_last_scan"] and math.isfinite(o["pivot_x"]) and math.isfinite(o["pivot_y"])):
        raise ValueError("FX_LOOP_GIVEN needs loop_first_scan < loop_last_scan and a finite pivot")
    sd, idd, mbd = f64(sd32), f64(id32), f64(mb32)
    sd2, mb2, gate, id2 = sd * sd, mbd * mbd, f64(2.0) * idd, idd * idd
    st = dict(state, header=dict(state["header"]), landmarks=[dict(r) for r in state["landmarks"]], acc=[list(a) for a in state["acc"]],
              carry=list(state["carry"]), carry_kp=state["carry_kp"].copy())
    H, lms, accs = st["header"], st["landmarks"], st["acc"]
    N, SEG, scans = min(int(H["n_landmarks"]), len(lms)), int(H["segments"]), int(H["scans"])
    last = scans - 1
    alias = [int(a) for a in st.get("alias", [])][:N]
    alias += [-1] * (N - len(alias))
    st["alias"] = alias
    seg_id = want if want != FX_LOC_LAST_SEGMENT else (SEG - 1 if SEG else FX_LOOP_NONE)
    P = tuple(float(v) for v in (prior if prior is not None else (1.0, 0.0, 0.0, 0.0, 0.0)))[:5]
    res = np.zeros(1, LOOP_DTYPE)[0]
    res["c"], res["s"], res["tx"], res["ty"], res["tz"] = P
    res["dc"], res["rms"], res["segment"] = 1.0, np.inf, seg_id
    res["loop_first_scan"] = res["loop_last_scan"] = res["hyp_a"] = res["hyp_b"] = FX_LOOP_NONE
    match = np.full(int(st["max_landmarks"]), -1, np.int32)
    refuse = (FX_LOOP_BAD_SEGMENT if seg_id >= SEG or scans == 0 else 0) | (0 if all(math.isfinite(v) for v in P) else FX_LOOP_BAD_PRIOR)
    if refuse:
        res["flags"] = refuse
        return st, res, match
    pc, ps, ptx, pty, ptz = P
    T, flags, ready = P, 0, False  # ready: T, the bounds and the pivot are set
    s0 = s1 = FX_LOOP_NONE
    px = py = 0.0
    if mode == FX_LOOP_GIVEN:
        s0, s1, px, py, ready = int(o["loop_first_scan"]), int(o["loop_last_scan"]), float(o["pivot_x"]), float(o["pivot_y"]), True
    else:
        seg = np.array([int(r["segment"]) for r in lms[:N]], np.int64)
        first, last_of = (np.array([int(r[f]) for r in lms[:N]], np.int64) for f in ("first_scan", "last_scan"))
        lx, ly, lz = (np.array([float(r[f]) for r in lms[:N]], f64) for f in ("x", "y", "z"))
        elig = np.array([alias[g] == -1 and int(lms[g]["n_obs"]) >= o["min_landmark_obs"] for g in range(N)], bool)
        if N:
            elig &= np.isfinite(lx) & np.isfinite(ly) & np.isfinite(lz) & (seg == seg_id)
        q = np.flatnonzero(elig & (first + int(o["recent_scans"]) >= last))
        t = np.flatnonzero(elig & (last_of + int(o["min_loop_scans"]) <= last))
        res["n_query"] = len(q)
        with np.errstate(all="ignore"):
            cc, ss, tx_, ty_, tz_ = (f64(v) for v in P)
            wx, wy, wz = (cc * lx[q] - ss * ly[q]) + tx_, (ss * lx[q] + cc * ly[q]) + ty_, lz[q] + tz_
            near, d2_of = np.full(len(q), -1, np.int64), np.zeros(len(q), np.uint64)
            if len(q) and len(t):
                for lo in range(0, len(q), 256):  # (chunks: [queries, targets] temporaries)
                    hi = min(lo + 256, len(q))
                    dx, dy = lx[t][None, :] - wx[lo:hi, None], ly[t][None, :] - wy[lo:hi, None]
                    d2 = dx * dx + dy * dy
                    key = np.where(d2 <= sd2, d2, np.inf).view(np.uint64)  # (the bits of +inf are above those of any distance in reach)
                    j = np.argmin(key, axis=1)  # (the first minimum: ids ascend, so ties go to the lowest id)
                    dj = d2[np.arange(hi - lo), j]
                    hit = dj <= sd2
                    near[lo:hi][hit] = t[j[hit]]
                    d2_of[lo:hi][hit] = dj.view(np.uint64)[hit]
            k = np.flatnonzero(near >= 0)
            flags = FX_LOOP_TRUNCATED if len(k) > FX_LOOP_MAX_CORR else 0
            k = k[:FX_LOOP_MAX_CORR]
            n = len(k)
            res["n_corr"] = n
            g = near[k]
            P64 = np.stack([wx[k], wy[k], lx[g], ly[g]], axis=1) if n else np.zeros((0, 4), f64)
            fitd = _map_consensus(P64, d2_of[k], q[k], lz[g], wz[k], o["hyp_corr"], mb2, gate, id2)
        if fitd is None:
            flags |= FX_LOOP_NO_HYPOTHESIS
        else:
            (dc, ds, dtx, dty), dtz, final = fitd["fit"], fitd["dtz"], fitd["final"]
            res["dc"], res["ds"], res["dtx"], res["dty"], res["dtz"], res["rms"] = dc, ds, dtx, dty, dtz, fitd["rms"]
            res["n_inliers"] = len(final)
            res["hyp_a"], res["hyp_b"] = fitd["hyp"]
            qi, gi = q[k[final]], g[final]
            match[qi] = gi
            if len(final) >= o["min_inliers"]:
                flags |= FX_LOOP_FITTED
                ready = True
                T = (dc * pc - ds * ps, ds * pc + dc * ps, (dc * ptx - ds * pty) + dtx, (ds * ptx + dc * pty) + dty, ptz + dtz)
                s0, s1 = int(last_of[gi].max()), int(first[qi].min())
                sx = sy = 0.0
                for i in qi.tolist():  # (ascending id)
                    sx += float(lx[i])
                    sy += float(ly[i])
                px, py = sx / float(len(final)), sy / float(len(final))
    res["c"], res["s"], res["tx"], res["ty"], res["tz"] = T
    res["loop_first_scan"], res["loop_last_scan"], res["px"], res["py"] = s0, s1, px, py
    applied = False
    if ready:
        if not T[0] > 0.0:
            flags |= FX_LOOP_TOO_FAR
        else:
            applied = mode != FX_LOOP_DRY_RUN
    if applied:
        flags |= FX_LOOP_APPLIED
        moved = 0
        for i in range(N):
            R, A = lms[i], accs[i]
            if int(R["segment"]) != seg_id:
                continue
            alpha = _loop_weight(int(R["first_scan"]) + int(R["last_scan"]), s0, s1)
            if not alpha > 0.0:
                continue
            moved += 1
            c, s, tx, ty, tz = _loop_transform(T, px, py, alpha)
            n = float(R["n_obs"])
            sx, sy, sz = (c * A[0] - s * A[1]) + n * tx, (s * A[0] + c * A[1]) + n * ty, A[2] + n * tz
            ax, ay = (c * A[3] - s * A[4]) + tx, (s * A[3] + c * A[4]) + ty
            dx, dy = c * A[5] - s * A[6], s * A[5] + c * A[6]
            A[:7] = [sx, sy, sz, ax, ay, dx, dy]
            if int(R["n_obs"]):
                _map_record_from_sums(R, A)
        if SEG - 1 == seg_id:
            alpha = _loop_weight(2 * last, s0, s1)
            if alpha > 0.0:
                lp = tuple(float(v) for v in H["last_pose"][:5])
                H["last_pose"] = _rigid_compose(_loop_transform(T, px, py, alpha), lp) + tuple(H["last_pose"][5:])
        res["moved"] = moved
    res["flags"] = flags
    return st, res, match


def loop_correct_poses_reference(result, poses, first_global_scan):
    """The definition of fx_map_loop_correct_poses (include/fx.h): result a LOOP_DTYPE record, poses POSE_DTYPE records of the global
    scans first_global_scan, first_global_scan + 1, ...  Returns the corrected copy."""
    out = np.array(poses, POSE_DTYPE).copy()
    if not int(result["flags"]) & FX_LOOP_APPLIED:
        return out
    T = tuple(float(result[k]) for k in ("c", "s", "tx", "ty", "tz"))
    px, py, s0, s1 = float(result["px"]), float(result["py"]), int(result["loop_first_scan"]), int(result["loop_last_scan"])
    for b in range(len(out)):
        alpha = _loop_weight(2 * (int(first_global_scan) + b), s0, s1)
        if alpha > 0.0:
            new = _rigid_compose(_loop_transform(T, px, py, alpha), tuple(float(out[k][b]) for k in ("c", "s", "tx", "ty", "tz")))
            out["c"][b], out["s"][b], out["tx"][b], out["ty"][b], out["tz"][b] = new
    return out


# ---- a scan's pose in the map without a prior (include/fx.h fx_map_relocalize)
def relocalize_records(out):
    """A host copy of fx_map_relocalize's records (a torch tensor, or any array of n * 96 bytes) as RELOC_DTYPE records."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(RELOC_DTYPE).copy()


def _constellation_search(x, y, z, ex, ey, ez, id2, ptd, mb2, xb2, g2, max_seeds):
    """The seed, hypothesis, score, winner, rival and tz clauses fx_map_relocalize and fx_map_find_loop share (include/fx.h), in
    numpy float64: x, y, z the points (a scan's used keypoints, a loop's queries), ex, ey, ez the landmarks they may be laid on, in
    ascending id.  Every (seed, g, h) and every (point, landmark) pair is looked at.  One ufunc an operation, so nothing is
    contracted; call it under np.errstate(all="ignore").  Returns {"n_seeds", "hyp": (s, g, h, score) arrays in (s, g, h) order with
    g, h as positions in ex, "win": None or a dict: T = (c, s, tx, ty), tz, score, runner, ka, kb (the winning seed's points), g, h,
    hit (bool a point: scored) and j (a point's landmark, a position in ex)}."""
    f64 = np.float64
    half = f64(0.5)
    n_kp, E = len(x), len(ex)

    def landed(wx, wy):
        """[..., E] -> does the image land on a landmark; chunked over the leading axis"""
        out = np.zeros(wx.shape, bool)
        if not E:
            return out
        step = max(1, (1 << 22) // max(1, wx.shape[1] * E))
        for lo_ in range(0, wx.shape[0], step):
            dx, dy = ex[None, None, :] - wx[lo_:lo_ + step, :, None], ey[None, None, :] - wy[lo_:lo_ + step, :, None]
            out[lo_:lo_ + step] = (dx * dx + dy * dy <= id2).any(axis=2)
        return out

    # seeds
    a, c_ = np.triu_indices(n_kp, 1)  # lexicographic (a, b), a < b
    dx, dy = x[c_] - x[a], y[c_] - y[a]
    d2 = dx * dx + dy * dy
    cand = np.flatnonzero((mb2 <= d2) & (d2 <= xb2))
    order = cand[np.lexsort((cand, ~d2[cand].view(np.uint64)))]  # descending d2 bits, then ascending (a, b)
    seeds = order[:int(max_seeds)]
    # hypotheses: (s, g, h) in ascending order, g and h as positions in ex
    parts = []
    for s_rank, k in enumerate(seeds):
        if E < 2:
            break
        xa, ya, xb_, yb_ = x[a[k]], y[a[k]], x[c_[k]], y[c_[k]]
        dqx, dqy = xb_ - xa, yb_ - ya
        dtx, dty = ex[None, :] - ex[:, None], ey[None, :] - ey[:, None]  # [g, h]: B.z - A.z
        lq2, lt2 = dqx * dqx + dqy * dqy, dtx * dtx + dty * dty
        keep = (lq2 >= mb2) & (lt2 >= mb2)
        keep &= ~(np.abs(np.sqrt(lq2) - np.sqrt(lt2)) > ptd)
        keep &= ~np.eye(E, dtype=bool)
        gi, hi_ = np.nonzero(keep)  # (row-major: ascending (g, h))
        dtx, dty = dtx[gi, hi_], dty[gi, hi_]
        dot, crs = dqx * dtx + dqy * dty, dqx * dty - dqy * dtx
        nrm = np.sqrt(dot * dot + crs * crs)
        ok = nrm > 0
        gi, hi_, dot, crs, nrm = gi[ok], hi_[ok], dot[ok], crs[ok], nrm[ok]
        c, s = dot / nrm, crs / nrm
        mqx, mqy = (xa + xb_) * half, (ya + yb_) * half
        mtx, mty = (ex[gi] + ex[hi_]) * half, (ey[gi] + ey[hi_]) * half
        tx, ty = mtx - (c * mqx - s * mqy), mty - (s * mqx + c * mqy)
        wx = (c[:, None] * x[None, :] - s[:, None] * y[None, :]) + tx[:, None]
        wy = (s[:, None] * x[None, :] + c[:, None] * y[None, :]) + ty[:, None]
        score = landed(wx, wy).sum(axis=1)
        parts.append((np.full(len(gi), s_rank), gi, hi_, score, c, s, tx, ty))
    if parts:
        hs, hg, hh, hscore, hc, hsn, htx, hty = (np.concatenate([p[k] for p in parts]) for k in range(8))
    else:
        hs = hg = hh = hscore = np.zeros(0, np.int64)
        hc = hsn = htx = hty = np.zeros(0, f64)
    out = {"n_seeds": len(seeds), "hyp": (hs, hg, hh, hscore), "win": None}
    if not len(hs) or hscore.max() < 2:
        return out
    w = int(np.argmax(hscore))  # (the first maximum: the lowest (s, g, h))
    wc, ws, wtx, wty = hc[w], hsn[w], htx[w], hty[w]
    # rivals: the winner's seed points under every hypothesis against under the winner
    ka, kb = a[seeds[hs[w]]], c_[seeds[hs[w]]]
    rival = np.zeros(len(hs), bool)
    for q in (ka, kb):
        ux, uy = (hc * x[q] - hsn * y[q]) + htx, (hsn * x[q] + hc * y[q]) + hty
        vx, vy = (wc * x[q] - ws * y[q]) + wtx, (ws * x[q] + wc * y[q]) + wty
        rx, ry = ux - vx, uy - vy
        rival |= rx * rx + ry * ry > g2
    runner = int(hscore[rival].max()) if rival.any() else 0
    # the landmark of every point under the winner: lowest (d2 bits, id) in reach
    wx, wy = (wc * x - ws * y) + wtx, (ws * x + wc * y) + wty
    dx, dy = ex[None, :] - wx[:, None], ey[None, :] - wy[:, None]
    d2 = dx * dx + dy * dy
    key = np.where(d2 <= id2, d2, np.inf).view(np.uint64)
    j = np.argmin(key, axis=1)  # (the first minimum: ids ascend)
    hit = d2[np.arange(n_kp), j] <= id2
    score = int(hit.sum())
    assert score == int(hscore[w])
    sz = 0.0
    for k in np.flatnonzero(hit):
        sz += (float(ez[j[k]]) - float(z[k]))
    out["win"] = dict(T=(wc, ws, wtx, wty), tz=sz / float(score), score=score, runner=runner, ka=int(ka), kb=int(kb), g=int(hg[w]), h=int(hh[w]),
                      hit=hit, j=j)
    return out


def map_relocalize_reference(state, kp_offset, kp_rows, n_scans, q_max_rows=None, inlier_dist=0.30, pair_tol=0.30, min_baseline=2.0,
                             max_baseline=60.0, max_seeds=16, min_inliers=4, min_margin=1, min_landmark_obs=2, segment=FX_LOC_ANY_SEGMENT):
    """The definition of fx_map_relocalize (include/fx.h) in numpy float64 over a map_reference / map_merge_reference state (which is
    only read).  kp_offset / kp_rows / q_max_rows as in map_localize_reference.  Every (seed, g, h) and every (keypoint, landmark)
    pair is looked at: nothing here knows of a grid.  One ufunc an operation, so nothing is contracted.  Returns {"rec": RELOC_DTYPE
    [n_scans], "map_id_of_row": int32 [q_max_rows], "hyp": per scan the hypotheses as a dict of arrays s, g, h, score in
    (s, g, h) order}."""
    f64 = np.float64
    off = [int(x) for x in kp_offset]
    kp = np.ascontiguousarray(kp_rows, dtype=np.float32)
    kp = kp.reshape(len(kp), -1)[:, :3] if kp.size else np.zeros((0, 3), np.float32)
    n_scans = int(n_scans)
    R = len(kp) if q_max_rows is None else int(q_max_rows)
    id32, pt32, mb32, xb32 = np.float32(inlier_dist), np.float32(pair_tol), np.float32(min_baseline), np.float32(max_baseline)
    if not (n_scans >= 1 and all(np.isfinite(v) and v > 0 for v in (id32, pt32, mb32)) and np.isfinite(xb32) and xb32 >= mb32 and
            1 <= max_seeds <= FX_RELOC_MAX_KP and min_inliers >= 3 and min_margin >= 1 and min_landmark_obs >= 1):
        raise ValueError("arguments outside what fx_map_relocalize accepts")
    idd, ptd, mbd, xbd = f64(id32), f64(pt32), f64(mb32), f64(xb32)
    id2, mb2, xb2 = idd * idd, mbd * mbd, xbd * xbd
    two = f64(2.0) * idd
    g2 = two * two
    S, rows = min(n_scans, len(off) - 1), min(len(kp), R)
    # the eligible landmarks (fx_map_localize's clause)
    lms = state["landmarks"]
    N = min(int(state["header"]["n_landmarks"]), len(lms))
    alias = [int(a) for a in state.get("alias", [])][:N]
    alias += [-1] * (N - len(alias))
    lx, ly, lz = (np.array([float(r[f]) for r in lms[:N]], f64) for f in ("x", "y", "z"))
    want = int(segment) & 0xffffffff
    if want == FX_LOC_LAST_SEGMENT:
        want = int(state["header"]["segments"]) - 1  # (-1 in a map of no segment: nothing is eligible)
    elig = np.array([alias[g] == -1 and int(lms[g]["n_obs"]) >= min_landmark_obs and (want == FX_LOC_ANY_SEGMENT or int(lms[g]["segment"]) == want)
                     for g in range(N)], bool)
    if N:
        elig &= np.isfinite(lx) & np.isfinite(ly) & np.isfinite(lz)
    ids = np.flatnonzero(elig)
    ex, ey, ez = lx[ids], ly[ids], lz[ids]
    rec = np.zeros(n_scans, RELOC_DTYPE)
    rec["pose"]["c"] = 1.0
    for f in ("seed_a", "seed_b", "lm_a", "lm_b"):
        rec[f] = FX_RELOC_NONE
    map_id = np.full(R, -1, np.int32)
    hyps = []
    with np.errstate(all="ignore"):
        for b in range(n_scans):
            empty = {k: np.zeros(0, np.int64) for k in ("s", "g", "h", "score")}
            if b >= S:
                rec["flags"][b] = FX_RELOC_NO_SCAN
                hyps.append(empty)
                continue
            lo = min(off[b], rows)
            hi = max(min(off[b + 1], rows), lo)
            fin = np.flatnonzero(np.isfinite(kp[lo:hi]).all(axis=1)) + lo
            flags = FX_RELOC_TRUNCATED if len(fin) > FX_RELOC_MAX_KP else 0
            used = fin[:FX_RELOC_MAX_KP]
            n_kp = len(used)
            x, y, z = (kp[used, k].astype(f64) for k in range(3))
            rec["n_kp"][b] = n_kp
            found = _constellation_search(x, y, z, ex, ey, ez, id2, ptd, mb2, xb2, g2, max_seeds)
            rec["n_seeds"][b] = found["n_seeds"]
            hs, hg, hh, hscore = found["hyp"]
            rec["n_hyp"][b] = len(hs)
            hyps.append({"s": hs, "g": ids[hg] if len(hg) else hg, "h": ids[hh] if len(hh) else hh, "score": hscore})
            W = found["win"]
            if W is None:
                rec["flags"][b] = flags | FX_RELOC_NO_HYPOTHESIS
                continue
            score, runner, hit, j = W["score"], W["runner"], W["hit"], W["j"]
            P = rec["pose"]
            P["c"][b], P["s"][b], P["tx"][b], P["ty"][b] = W["T"]
            P["tz"][b] = W["tz"]
            P["segment"][b] = int(lms[int(ids[W["g"]])]["segment"])
            rec["score"][b], rec["runner_up"][b] = score, runner
            rec["seed_a"][b], rec["seed_b"][b] = used[W["ka"]], used[W["kb"]]
            rec["lm_a"][b], rec["lm_b"][b] = ids[W["g"]], ids[W["h"]]
            if score >= min_inliers:
                flags |= FX_RELOC_VALID if score - runner >= min_margin else FX_RELOC_AMBIGUOUS
            rec["flags"][b] = flags
            if flags & FX_RELOC_VALID:
                map_id[used[hit]] = ids[j[hit]]
    return {"rec": rec, "map_id_of_row": map_id, "hyp": hyps}


def find_loop_records(out):
    """A host copy of fx_map_find_loop's result (a torch tensor, or any array of 136 bytes) as a FIND_DTYPE record."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(FIND_DTYPE).copy()[0]


def map_find_loop_reference(state, **options):
    """The definition of fx_map_find_loop (include/fx.h) in numpy float64 over a map_reference / map_merge_reference state (which is
    only read); options: the fields of fx_map_find_loop_options (FIND_DEFAULTS).  Every (seed, g, h) and every (query, target)
    pair is looked at: nothing here knows of a grid.  Returns {"rec": a FIND_DTYPE record, "match_of_landmark": int32
    [max_landmarks], "hyp": the hypotheses as a dict of arrays s, g, h, score in (s, g, h) order, g and h landmark ids}."""
    f64 = np.float64
    bad = set(options) - set(FIND_DEFAULTS)
    if bad:
        raise TypeError(f"unknown find-loop options {sorted(bad)}")
    o = dict(FIND_DEFAULTS, **options)
    id32, pt32, mb32, xb32 = (np.float32(o[k]) for k in ("inlier_dist", "pair_tol", "min_baseline", "max_baseline"))
    want_q, want_t = int(o["segment"]) & 0xffffffff, int(o["target_segment"]) & 0xffffffff
    same = want_t == FX_FIND_SAME_SEGMENT
    if not (all(np.isfinite(v) and v > 0 for v in (id32, pt32, mb32)) and np.isfinite(xb32) and xb32 >= mb32 and
            1 <= o["max_seeds"] <= FX_FIND_MAX_QUERY and o["min_inliers"] >= 3 and o["min_margin"] >= 1 and o["min_landmark_obs"] >= 1 and
            FX_LOC_ANY_SEGMENT not in (want_q, want_t) and (not same or 0 <= o["recent_scans"] < o["min_loop_scans"])):
        raise ValueError("arguments outside what fx_map_find_loop accepts")
    idd, ptd, mbd, xbd = f64(id32), f64(pt32), f64(mb32), f64(xb32)
    id2, mb2, xb2 = idd * idd, mbd * mbd, xbd * xbd
    two = f64(2.0) * idd
    g2 = two * two
    H, lms = state["header"], state["landmarks"]
    N, SEG, scans = min(int(H["n_landmarks"]), len(lms)), int(H["segments"]), int(H["scans"])
    last = scans - 1
    last_seg = SEG - 1 if SEG else FX_FIND_NONE
    qseg = last_seg if want_q == FX_LOC_LAST_SEGMENT else want_q
    tseg = qseg if same else (last_seg if want_t == FX_LOC_LAST_SEGMENT else want_t)
    rec = np.zeros(1, FIND_DTYPE)[0]
    nan = np.array([FX_FIND_NAN_BITS], np.uint64).view(f64)[0]
    for f in ("c", "s", "tx", "ty", "tz"):
        rec[f] = nan
    rec["wc"] = 1.0
    for f in ("seed_a", "seed_b", "lm_a", "lm_b"):
        rec[f] = FX_FIND_NONE
    rec["segment"], rec["target_segment"] = qseg, tseg
    match = np.full(int(state["max_landmarks"]), -1, np.int32)
    empty = {k: np.zeros(0, np.int64) for k in ("s", "g", "h", "score")}
    if qseg >= SEG or tseg >= SEG or scans == 0 or (not same and tseg == qseg):
        rec["flags"] = FX_FIND_BAD_SEGMENT
        return {"rec": rec, "match_of_landmark": match, "hyp": empty}
    alias = [int(a) for a in state.get("alias", [])][:N]
    alias += [-1] * (N - len(alias))
    lx, ly, lz = (np.array([float(r[f]) for r in lms[:N]], f64) for f in ("x", "y", "z"))
    seg = np.array([int(r["segment"]) for r in lms[:N]], np.int64)
    first, last_of = (np.array([int(r[f]) for r in lms[:N]], np.int64) for f in ("first_scan", "last_scan"))
    elig = np.array([alias[g] == -1 and int(lms[g]["n_obs"]) >= o["min_landmark_obs"] for g in range(N)], bool)
    if N:
        elig &= np.isfinite(lx) & np.isfinite(ly) & np.isfinite(lz)
    is_t = elig & (seg == tseg)
    if same:
        is_t &= last_of + int(o["min_loop_scans"]) <= last
    ids = np.flatnonzero(is_t)
    cand = np.flatnonzero(elig & (seg == qseg) & (first + int(o["recent_scans"]) >= last) & ~is_t)[::-1]  # descending id
    flags = FX_FIND_TRUNCATED if len(cand) > FX_FIND_MAX_QUERY else 0
    used = cand[:FX_FIND_MAX_QUERY]
    rec["n_query"], rec["n_targets"] = len(used), len(ids)
    with np.errstate(all="ignore"):
        found = _constellation_search(lx[used], ly[used], lz[used], lx[ids], ly[ids], lz[ids], id2, ptd, mb2, xb2, g2, o["max_seeds"])
    rec["n_seeds"] = found["n_seeds"]
    hs, hg, hh, hscore = found["hyp"]
    rec["n_hyp"] = len(hs)
    hyp = {"s": hs, "g": ids[hg] if len(hg) else hg, "h": ids[hh] if len(hh) else hh, "score": hscore}
    W = found["win"]
    if W is None:
        rec["flags"] = flags | FX_FIND_NO_HYPOTHESIS
        return {"rec": rec, "match_of_landmark": match, "hyp": hyp}
    score, runner = W["score"], W["runner"]
    rec["wc"], rec["ws"], rec["wtx"], rec["wty"] = W["T"]
    rec["wtz"] = W["tz"]
    rec["score"], rec["runner_up"] = score, runner
    rec["seed_a"], rec["seed_b"] = used[W["ka"]], used[W["kb"]]
    rec["lm_a"], rec["lm_b"] = ids[W["g"]], ids[W["h"]]
    if score >= o["min_inliers"]:
        flags |= FX_FIND_VALID if score - runner >= o["min_margin"] else FX_FIND_AMBIGUOUS
    rec["flags"] = flags
    if flags & FX_FIND_VALID:
        for f in ("c", "s", "tx", "ty", "tz"):
            rec[f] = rec["w" + f]
        match[used[W["hit"]]] = ids[W["j"][W["hit"]]]
    return {"rec": rec, "match_of_landmark": match, "hyp": hyp}


# ---- one block pair from scans of two (include/fx.h fx_splice_blocks)
def _splice_scans(src):
    """The selected scans of a source ((kp block bytes, max_scans, max_total), (CSR block bytes, max_rows, capacity) or None, scan0,
    n_scans): a list of (flag word, [(keypoint row as 4 words, its CSR entries (col, val bits) or None: the row does not exist)])."""
    (kb, max_scans, max_total), csr, scan0, n_scans = src
    u = np.ascontiguousarray(kb).view(np.uint8).reshape(-1).view(np.uint32)
    lay = keypoint_block_layout(max_scans, max_total)
    S, K = min(int(u[0]), max_scans), min(int(u[1]), max_total)
    off, flags, rows = u[4:5 + max_scans], u[lay.f0:lay.f0 + max_scans], u[4 * lay.k0:4 * lay.n_rows].reshape(-1, 4)
    if csr is not None:
        cb, max_rows, cap = csr
        c = np.ascontiguousarray(cb).view(np.uint8).reshape(-1)
        o_rp, o_col, o_val, _ = csr_layout(max_rows, cap)
        exists, rp = min(int(c[:16].view(np.uint32)[3]), max_rows), c[o_rp:o_col].view(np.uint32)
        col, val = c[o_col:o_val].view(np.uint32), c[o_val:].view(np.uint32)
    if scan0 == FX_SPLICE_LAST_SCAN:
        scan0, n_scans = (S - 1, n_scans) if S else (0, 0)
    out = []
    for i in range(min(scan0, S), min(scan0 + n_scans, S)):
        lo, hi = min(int(off[i]), K), min(int(off[i + 1]), K)
        out.append((int(flags[i]), [(rows[r].copy(), None if csr is None or r >= exists else (col[rp[r]:rp[r + 1]].copy(), val[rp[r]:rp[r + 1]].copy()))
                                    for r in range(lo, max(lo, hi))]))
    return out


def splice_reference(a, b, dst_kp, dst_csr=None):
    """The definition of fx_splice_blocks in plain loops: a and b are sources as _splice_scans reads them, dst_kp the destination's
    (max_scans, max_total_keypoints), dst_csr its (max_rows, capacity) or None.  The virtual batch's scans are built row by row; the
    two packs' rules are then stated on them.  Returns (the keypoint block as uint8, None or the CSR block's defined words as a dict:
    "header" u32[4], "row_ptr" u32[max_rows + 1], "col" u32[nnz_stored], "val" u32[nnz_stored], the val words as bits)."""
    scans = _splice_scans(a) + _splice_scans(b)
    max_scans, max_total = dst_kp
    lay = keypoint_block_layout(max_scans, max_total)
    blk = np.zeros(4 * lay.n_rows, np.uint32)
    voff = np.concatenate([[0], np.cumsum([len(rows) for _, rows in scans], dtype=np.int64)]).astype(np.int64)
    n, nb = len(scans), min(len(scans), max_scans)
    clip = np.minimum(voff, max_total)
    blk[4:lay.f0] = clip[np.minimum(np.arange(lay.f0 - 4), nb)]
    for i in range(nb):
        o0, o1 = int(clip[i]), int(clip[i + 1])
        blk[lay.f0 + i] = scans[i][0] | (0x4 if o1 - o0 < len(scans[i][1]) else 0)  # FX_FLAG_KP_OVERFLOW
        for k in range(o1 - o0):
            blk[4 * (lay.k0 + o0 + k):4 * (lay.k0 + o0 + k) + 4] = scans[i][1][k][0]
    blk[:4] = (nb, clip[nb], np.bitwise_or.reduce(blk[lay.f0:lay.f0 + nb], initial=0) | (0x4 if n > max_scans else 0), max_total)
    if dst_csr is None:
        return blk.view(np.uint8), None
    max_rows, cap = dst_csr
    virt = [entries for _, rows in scans for _, entries in rows]
    row_ptr, cols, vals, stored = [0], [], [], 0
    for v, e in enumerate(virt):
        if e is None or v >= max_rows or row_ptr[-1] + len(e[0]) > cap:
            break
        row_ptr.append(row_ptr[-1] + len(e[0])), cols.append(e[0]), vals.append(e[1])
        stored += 1
    nnz = row_ptr[-1]
    needed = sum(len(e[0]) for e in virt if e is not None) & 0xffffffff
    row_ptr = np.array(row_ptr + [nnz] * (max_rows - stored), np.uint32)
    return blk.view(np.uint8), {"header": np.array([len(virt), nnz, needed, stored], np.uint32), "row_ptr": row_ptr,
                                "col": np.concatenate(cols + [np.zeros(0, np.uint32)]).astype(np.uint32),
                                "val": np.concatenate(vals + [np.zeros(0, np.uint32)]).astype(np.uint32)}


def splice_kp_offset(off_a, off_b, a=(FX_SPLICE_LAST_SCAN, 1), b=(0, 0xffffffff)):
    """The kp_offset of the block fx_splice_blocks builds from scans a = (scan0, n_scans) of the batch with h_kp_offset off_a and scans
    b of the batch with off_b (neither block cut), for pairs_consecutive."""
    n = [np.diff(np.asarray(o, np.int64))[(max(len(o) - 2, 0) if s == FX_SPLICE_LAST_SCAN else s):][:c] for o, (s, c) in ((off_a, a), (off_b, b))]
    return np.concatenate([[0], np.cumsum(np.concatenate(n))]).astype(np.uint32)


# ---- keypoints de-skewed for the sensor's motion during a sweep (include/fx.h fx_deskew_keypoint_block)
def deskew_records(out):
    """A host copy of fx_deskew_keypoint_block's records (a torch tensor, or any array of n * 16 bytes) as a structured numpy array
    of DESKEW_DTYPE records."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1).view(DESKEW_DTYPE).copy()


def deskew_turn(x, y):
    """include/fx.h "Turn of a row": atan2(y, x) in turns through the odd polynomial DESKEW_TURN_K, Python floats in the clause's
    order."""
    k = DESKEW_TURN_K
    ax, ay = abs(x), abs(y)
    hi, lo = (ay, ax) if ay > ax else (ax, ay)
    if not hi > 0.0:
        return 0.0
    a = lo / hi
    t = a * a
    g = a * (k[0] + t * (k[1] + t * (k[2] + t * (k[3] + t * (k[4] + t * k[5])))))
    q = 0.25 - g if ay > ax else g
    h = 0.5 - q if x < 0.0 else q
    return -h if y < 0.0 else h


def deskew_share(x, y, start_turn=0.5, ref_fraction=1.0, sweep_fraction=1.0, direction=-1):
    """include/fx.h "Sweep fraction": (phi, a) of a row at (x, y), Python floats."""
    u = float(direction) * (deskew_turn(x, y) - start_turn)
    phi = u - float(math.floor(u))
    if phi >= 1.0:
        phi = 0.0
    return phi, (phi - ref_fraction) * sweep_fraction


def _deskew_usable(m, p, require_flags):
    """include/fx.h "Usable motion" of record p."""
    r = m[p]
    finite = all(math.isfinite(float(r[f])) for f in ("c", "s", "tx", "ty", "tz"))
    return (int(r["flags"]) & require_flags) == require_flags and finite and float(r["c"]) > 0.0


def deskew_reference(block, max_scans, max_total, motions, n_scans, **opts):
    """The definition of fx_deskew_keypoint_block (include/fx.h) in numpy and Python floats.  block: the source keypoint block's
    bytes, laid out for (max_scans, max_total); motions: REG_DTYPE records ([>= n_scans - 1] with FX_DESKEW_LINKS, [>= n_scans]
    with FX_DESKEW_PER_SCAN; may be None where none is read); opts: the fields of fx_deskew_options (DESKEW_DEFAULTS).  Returns
    (the destination block as uint8, DESKEW_DTYPE [n_scans])."""
    bad = set(opts) - set(DESKEW_DEFAULTS)
    if bad:
        raise TypeError(f"unknown deskew options {sorted(bad)}")
    o = dict(DESKEW_DEFAULTS, **opts)
    start, ref, sweep = float(o["start_turn"]), float(o["ref_fraction"]), float(o["sweep_fraction"])
    direction, source, require = int(o["direction"]), int(o["source"]), int(o["require_flags"]) & 0xffffffff
    n_scans = int(n_scans)
    if not (1 <= n_scans <= max_scans and math.isfinite(start) and 0.0 <= ref <= 1.0 and 0.0 < sweep <= 1.0 and direction in (1, -1) and
            source in (FX_DESKEW_LINKS, FX_DESKEW_PER_SCAN)):
        raise ValueError("arguments outside what fx_deskew_keypoint_block accepts")
    lay = keypoint_block_layout(max_scans, max_total)
    src = np.ascontiguousarray(block).view(np.uint8).reshape(-1)[:16 * lay.n_rows]
    assert len(src) == 16 * lay.n_rows, (len(src), max_scans, max_total)
    dst = src.copy()
    u = src.view(np.uint32)
    S, rows = min(n_scans, int(u[0]), max_scans), min(int(u[1]), max_total)
    off = [int(x) for x in u[4:5 + max_scans]]
    kp = src[16 * lay.k0:].view(np.float32).reshape(-1, 4)
    out_kp = dst[16 * lay.k0:].view(np.float32).reshape(-1, 4)
    m = None if motions is None else np.asarray(motions)
    rec = np.zeros(n_scans, DESKEW_DTYPE)
    rec["flags"], rec["motion"] = FX_DESKEW_NO_SCAN, FX_DESKEW_NO_RECORD
    # the motion of every scan
    for b in range(S):
        flags, p = FX_DESKEW_NO_MOTION, FX_DESKEW_NO_RECORD
        if source == FX_DESKEW_PER_SCAN:
            if _deskew_usable(m, b, require):
                flags, p = FX_DESKEW_MOVED, b
        elif b >= 1 and _deskew_usable(m, b - 1, require):
            flags, p = FX_DESKEW_MOVED, b - 1
        elif b + 1 < S and _deskew_usable(m, b, require):
            flags, p = FX_DESKEW_MOVED | FX_DESKEW_NEXT_LINK, b
        rec["flags"][b], rec["motion"][b] = flags, p
    # the scan of every row (fx_track_landmarks's scan(r))
    scan = np.full(max_total, -1, np.int64)
    for b in range(S):
        scan[off[b]:min(off[b + 1], rows)] = b
    shift_bits = np.zeros(n_scans, np.uint32)
    for r in range(rows):
        b = int(scan[r])
        if b < 0 or not rec["flags"][b] & FX_DESKEW_MOVED or not np.isfinite(kp[r, :3]).all():
            continue
        x, y, z = (float(v) for v in kp[r, :3])
        _, a = deskew_share(x, y, start, ref, sweep, direction)
        w = abs(a)
        if w == 0.0:
            continue
        c, s, tx, ty, tz = (float(m[f][rec["motion"][b]]) for f in ("c", "s", "tx", "ty", "tz"))
        G = (c, s, tx, ty, tz) if a > 0.0 else (c, -s, -(c * tx + s * ty), (s * tx - c * ty), -tz)
        ca, sa, txa, tya, tza = _loop_transform(G, 0.0, 0.0, w)
        with np.errstate(all="ignore"):
            new = np.array([(ca * x - sa * y) + txa, (sa * x + ca * y) + tya, z + tza], np.float64).astype(np.float32)
            out_kp[r, :3] = new
            dx, dy = float(new[0]) - x, float(new[1]) - y
            sh = np.float32(math.sqrt(dx * dx + dy * dy))
        rec["rows_moved"][b] += 1
        shift_bits[b] = max(int(shift_bits[b]), int(sh.view(np.uint32)))
    rec["max_shift"] = shift_bits.view(np.float32)
    return dst, rec


@contextlib.contextmanager
def _on_stream(stream_ptr, dev):
    """The stream hand-over of every wrapper that enqueues on a context's stream: that stream (stream_ptr, a hipStream_t as an
    integer) waits for what the caller's current stream on dev has queued, the body enqueues, and the caller's current stream
    waits for it.  Nothing waits on the host; when the body raises, nothing was enqueued and nobody waits."""
    import torch
    cur = torch.cuda.current_stream(dev)
    ext = torch.cuda.ExternalStream(stream_ptr, device=dev)
    ext.wait_stream(cur)
    yield
    cur.wait_stream(ext)


def _options(struct, defaults, what, opts):
    """An options structure of include/fx.h from its *_DEFAULTS and the caller's **opts, field by field: a float field takes
    float(value), a uint32 field the value's low 32 bits, `reserved` stays 0."""
    bad = set(opts) - set(defaults)
    if bad:
        raise TypeError(f"unknown {what} options {sorted(bad)}")
    o = dict(defaults, **opts)
    opt = struct()
    for name, ctype in struct._fields_:
        if name != "reserved":
            setattr(opt, name, float(o[name]) if ctype in (C.c_float, C.c_double) else int(o[name]) & 0xffffffff)
    return opt


def _out_tensor(t, shape, dtype, dev, error, typed=False):
    """An output tensor the caller may give: None allocates `shape` of `dtype` on dev, False passes NULL (None is returned), a
    tensor is used when it is contiguous, on dev and of the same bytes (typed: of the same dtype and shape), else ValueError(error)."""
    import torch
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t is False:
        return None
    fits = (t.dtype == dtype and tuple(t.shape) == tuple(shape)) if typed else t.numel() * t.element_size() == math.prod(shape) * dtype.itemsize
    if t.device != dev or not t.is_contiguous() or not fits:
        raise ValueError(error)
    return t


def _ptr(t):
    """The device address of an optional tensor as ctypes takes it: NULL for None."""
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _np(ptr, shape, dtype):
    n = int(np.prod(shape))
    if n == 0 or not ptr:
        return np.zeros(shape, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).reshape(shape).copy()


class Map:
    """Owner of an fx_map: the persistent landmark map of one context (include/fx.h fx_map_create).  Close it before its context."""

    def __init__(self, ctx, max_landmarks, max_carry_rows):
        self.ctx, self.lib = ctx, ctx.lib
        self.max_landmarks, self.max_carry_rows = int(max_landmarks), int(max_carry_rows)
        self.handle = C.c_void_p()
        check(self.lib.fx_map_create(ctx.handle, self.max_landmarks, self.max_carry_rows, C.byref(self.handle)))

    def close(self):
        if self.handle:
            self.lib.fx_map_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """fx_map_reset: enqueues the state of a fresh map."""
        check(self.lib.fx_map_reset(self.ctx.handle, self.handle))

    def _result_and_match(self, dtype, result, match):
        """The two outputs of join_segments, close_loop and find_loop: a record of `dtype` as float64 words and match_of_landmark."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        error = f"outputs must be contiguous tensors of {dtype.itemsize} and {self.max_landmarks} * 4 bytes on {dev}"
        return (_out_tensor(result, (dtype.itemsize // 8,), torch.float64, dev, error),
                _out_tensor(match, (self.max_landmarks,), torch.int32, dev, error))

    @staticmethod
    def _prior(prior, prior_device):
        """The prior of join_segments and close_loop as the library takes it: (byref of an fx_pose or None, a device address or None)."""
        pose = C.byref(FxPose(*(float(v) for v in tuple(prior)[:5]), 0, 0)) if prior is not None else None
        return pose, prior_device.data_ptr() if hasattr(prior_device, "data_ptr") else prior_device

    def update(self, kp, track_out, overlap=True, row_ids=None):
        """fx_map_update: kp is the keypoint block as (device tensor, max_scans, max_total_keypoints) and track_out the five device
        tensors Context.track_landmarks returned for it.  overlap: FX_MAP_OVERLAP (this batch's scan 0 is the last scan of the
        batch before).  Returns map_id_of_row, a device torch.int32 tensor [q_max_rows]; `row_ids` reuses one, row_ids=False passes
        NULL (None is returned).  Stream-correct like Context.track_landmarks; never waits for the stream."""
        import torch
        kb, scans, total = kp
        poses, lor, obs, lms, hdr = track_out
        dev = torch.device("cuda", self.ctx.device)
        n_rows, max_landmarks = int(lor.shape[0]), int(lms.shape[0])
        row_ids = _out_tensor(row_ids, (n_rows,), torch.int32, dev, f"row_ids must be a contiguous torch.int32 tensor [{n_rows}] on {dev}", typed=True)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_update(self.ctx.handle, self.handle, C.c_void_p(kb.data_ptr()), int(scans), int(total), C.c_void_p(poses.data_ptr()),
                                         C.c_void_p(lor.data_ptr()), C.c_void_p(obs.data_ptr()), n_rows, C.c_void_p(lms.data_ptr()), max_landmarks,
                                         C.c_void_p(hdr.data_ptr()), FX_MAP_OVERLAP if overlap else 0, _ptr(row_ids)))
        return row_ids

    def merge(self, merge_dist=0.30, max_gap_scans=64, result=None):
        """fx_map_merge: one round of spatial re-association of the fragments of one pole (include/fx.h).  Returns the
        fx_map_merge_result as a device torch.int32 tensor [4] (proposals, merged, live, 0); `result` reuses one, result=False
        passes NULL (None is returned).  Stream-correct like update(); never waits for the stream."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        result = _out_tensor(result, (4,), torch.int32, dev, f"result must be a contiguous torch.int32 tensor [4] on {dev}", typed=True)
        opt = FxMapMergeOptions(float(merge_dist), int(max_gap_scans))
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_merge(self.ctx.handle, self.handle, C.byref(opt), _ptr(result)))
        return result

    def localize(self, kp, prior_poses, n_scans, q_max_rows=None, out=None, nearest=None, **opts):
        """fx_map_localize: the scans of the keypoint block kp = (device tensor, max_scans, max_total_keypoints) against this map
        under prior_poses, a device tensor of n_scans fx_pose records (the first output of Context.track_landmarks, or the "pose"
        bytes of an earlier round).  opts: the fields of fx_localize_options (LOC_DEFAULTS).  Returns (records, map_id_of_row,
        nearest_of_row): device tensors of n_scans * 112 bytes (localize_records reads them) and torch.int32 [q_max_rows] each;
        out = (records, map_id_of_row) reuses two, nearest=False passes NULL (None is returned), a tensor reuses it.
        Stream-correct like update(); never waits for the stream."""
        import torch
        kb, scans, total = kp
        dev = torch.device("cuda", self.ctx.device)
        n_scans = int(n_scans)
        n_rows = int(total) if q_max_rows is None else int(q_max_rows)
        opt = _options(FxLocalizeOptions, LOC_DEFAULTS, "localize", opts)
        error = f"outputs must be contiguous tensors of {n_scans} * 112 and {n_rows} * 4 bytes on {dev}"
        recs, ids = (None, None) if out is None else out
        recs = _out_tensor(recs, (n_scans, LOC_DTYPE.itemsize // 8), torch.float64, dev, error)
        ids = _out_tensor(ids, (n_rows,), torch.int32, dev, error)
        nearest = _out_tensor(nearest, (n_rows,), torch.int32, dev, error)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_localize(self.ctx.handle, self.handle, C.c_void_p(kb.data_ptr()), int(scans), int(total),
                                           C.c_void_p(prior_poses.data_ptr()), n_scans, n_rows, C.byref(opt), C.c_void_p(recs.data_ptr()),
                                           C.c_void_p(ids.data_ptr() if n_rows else None), _ptr(nearest if n_rows else None)))
        return recs, ids, nearest

    def follow(self, kp, links, start_poses, n_scans, q_max_rows=None, out=None, poses=None, nearest=None, **opts):
        """fx_map_follow: chains of the consecutive scans of the keypoint block kp = (device tensor, max_scans,
        max_total_keypoints) followed through this map.  links: a device tensor of the register's n_scans - 1 link records (None
        where every chain is one scan); start_poses: a device tensor that begins with the n_chains fx_pose records, or a view into
        one (records[last] of the batch before: a record begins with its pose), or a device address; it is read on the device.
        opts: the fields of fx_follow_options (FOLLOW_DEFAULTS).  Returns (records, follow, poses, map_id_of_row, nearest_of_row):
        device tensors of n_scans * 112, n_scans * 64 and n_scans * 48 bytes (localize_records, follow_records and a POSE_DTYPE
        view read them) and torch.int32 [q_max_rows] each; out = (records, follow, map_id_of_row) reuses three, poses=False and
        nearest=False pass NULL (None is returned), a tensor reuses it.  Stream-correct like update(); never waits for the stream."""
        import torch
        kb, scans, total = kp
        dev = torch.device("cuda", self.ctx.device)
        n_scans = int(n_scans)
        n_rows = int(total) if q_max_rows is None else int(q_max_rows)
        bad = set(opts) - set(FOLLOW_DEFAULTS)
        if bad:
            raise TypeError(f"unknown follow options {sorted(bad)}")
        o = dict(FOLLOW_DEFAULTS, **opts)
        opt = FxFollowOptions()
        opt.loc = _options(FxLocalizeOptions, {k: o[k] for k in LOC_DEFAULTS}, "follow", {})
        opt.chain_scans, opt.require_flags, opt.max_lost = (int(o[k]) & 0xffffffff for k in ("chain_scans", "require_flags", "max_lost"))
        error = f"outputs must be contiguous tensors of {n_scans} * 112, {n_scans} * 64, {n_scans} * 48 and {n_rows} * 4 bytes on {dev}"
        recs, fol, ids = (None, None, None) if out is None else out
        recs = _out_tensor(recs, (n_scans, LOC_DTYPE.itemsize // 8), torch.float64, dev, error)
        fol = _out_tensor(fol, (n_scans, FOLLOW_DTYPE.itemsize // 8), torch.float64, dev, error)
        poses = _out_tensor(poses, (n_scans, POSE_DTYPE.itemsize // 8), torch.float64, dev, error)
        ids = _out_tensor(ids, (n_rows,), torch.int32, dev, error)
        nearest = _out_tensor(nearest, (n_rows,), torch.int32, dev, error)
        starts = start_poses.data_ptr() if hasattr(start_poses, "data_ptr") else int(start_poses)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_follow(self.ctx.handle, self.handle, C.c_void_p(kb.data_ptr()), int(scans), int(total), _ptr(links),
                                         C.c_void_p(starts), n_scans, n_rows, C.byref(opt), C.c_void_p(recs.data_ptr()), C.c_void_p(fol.data_ptr()),
                                         _ptr(poses), C.c_void_p(ids.data_ptr() if n_rows else None), _ptr(nearest if n_rows else None)))
        return recs, fol, poses, ids, nearest

    def observe(self, kp, loc, n_scans, map_id_of_row, q_max_rows=None, out=None, gained=None, observed=None, **opts):
        """fx_map_observe: the inlier rows of localised scans folded into the landmarks they were matched to (include/fx.h).  kp is
        the keypoint block the localise was given, as (device tensor, max_scans, max_total_keypoints); loc and map_id_of_row are the
        first two tensors localize() returned, read in place on the device.  opts: the fields of fx_map_observe_options
        (OBS_DEFAULTS).  Returns (result, gained_of_landmark, observed_id_of_row): device torch.int32 tensors [8] (observe_records
        reads it), [max_landmarks] and [q_max_rows]; out / gained / observed reuse one, False passes NULL (None is returned in its
        place).  Stream-correct like update(); never waits for the stream."""
        import torch
        kb, scans, total = kp
        dev = torch.device("cuda", self.ctx.device)
        n_scans = int(n_scans)
        n_rows = int(total) if q_max_rows is None else int(q_max_rows)
        opt = _options(FxMapObserveOptions, OBS_DEFAULTS, "observe", opts)
        error = f"outputs must be contiguous torch.int32 tensors [8], [{self.max_landmarks}] and [{n_rows}] on {dev}"
        out = _out_tensor(out, (8,), torch.int32, dev, error, typed=True)
        gained = _out_tensor(gained, (self.max_landmarks,), torch.int32, dev, error, typed=True)
        observed = _out_tensor(observed, (n_rows,), torch.int32, dev, error, typed=True)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_observe(self.ctx.handle, self.handle, C.c_void_p(kb.data_ptr()), int(scans), int(total), C.c_void_p(loc.data_ptr()),
                                          n_scans, C.c_void_p(map_id_of_row.data_ptr() if n_rows else None), n_rows, C.byref(opt), _ptr(out),
                                          _ptr(gained), _ptr(observed if n_rows else None)))
        return out, gained, observed

    def relocalize(self, kp, n_scans, q_max_rows=None, out=None, **opts):
        """fx_map_relocalize: the pose of the scans of the keypoint block kp = (device tensor, max_scans, max_total_keypoints) in this
        map, without a prior.  opts: the fields of fx_relocalize_options (RELOC_DEFAULTS).  Returns (records, map_id_of_row): device
        tensors of n_scans * 96 bytes (relocalize_records reads them; the first 48 bytes of a record are the fx_pose localize() takes
        as a prior) and torch.int32 [q_max_rows]; out = (records, map_id_of_row) reuses two.  Stream-correct like update(); never
        waits for the stream."""
        import torch
        kb, scans, total = kp
        dev = torch.device("cuda", self.ctx.device)
        n_scans = int(n_scans)
        n_rows = int(total) if q_max_rows is None else int(q_max_rows)
        opt = _options(FxRelocalizeOptions, RELOC_DEFAULTS, "relocalize", opts)
        if out is None:
            out = (torch.empty((n_scans, RELOC_DTYPE.itemsize // 8), dtype=torch.float64, device=dev), torch.empty((n_rows,), dtype=torch.int32, device=dev))
        recs, ids = out
        for t, size in ((recs, n_scans * RELOC_DTYPE.itemsize), (ids, n_rows * 4)):
            if t.device != dev or not t.is_contiguous() or t.numel() * t.element_size() != size:
                raise ValueError(f"outputs must be contiguous tensors of {n_scans} * 96 and {n_rows} * 4 bytes on {dev}")
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_relocalize(self.ctx.handle, self.handle, C.c_void_p(kb.data_ptr()), int(scans), int(total), n_scans, n_rows,
                                             C.byref(opt), C.c_void_p(recs.data_ptr()), C.c_void_p(ids.data_ptr() if n_rows else None)))
        return recs, ids

    def compact(self, min_obs=1, min_age_scans=64, remap=None, result=None):
        """fx_map_compact: the absorbed and the let-go landmarks taken out, the others renumbered in order (include/fx.h).  Returns
        (remap, result): device torch.int32 tensors [max_landmarks] (old id -> new id, -1: gone) and [4] (before, kept,
        dropped_absorbed, dropped_live); a tensor given reuses it, False passes NULL (None is returned in its place).
        Stream-correct like merge(); never waits for the stream."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        remap, result = (_out_tensor(t, (n,), torch.int32, dev, f"{name} must be a contiguous torch.int32 tensor [{n}] on {dev}", typed=True)
                         for t, n, name in ((remap, self.max_landmarks, "remap"), (result, 4, "result")))
        opt = FxMapCompactOptions(int(min_obs), int(min_age_scans))
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_compact(self.ctx.handle, self.handle, C.byref(opt), _ptr(remap), _ptr(result)))
        return remap, result

    def expect(self, kp, loc, n_scans, map_id_of_row, q_max_rows=None, out=None, expected=None, seen=None, **opts):
        """fx_map_expect: per landmark, how many of the localised scans should have seen it and how many did (include/fx.h).  kp, loc,
        n_scans, map_id_of_row and q_max_rows are observe()'s.  opts: the fields of fx_map_expect_options (EXPECT_DEFAULTS).
        expected / seen: device torch.int32 tensors [max_landmarks] to write (mode FX_EXPECT_WRITE) or to add to (FX_EXPECT_ADD: give
        them); None allocates them, zeroed.  Returns (result, expected, seen): result a device torch.int32 tensor [8] (expect_records
        reads it); out reuses one, False passes NULL.  Stream-correct like update(); never waits for the stream."""
        import torch
        kb, scans, total = kp
        dev = torch.device("cuda", self.ctx.device)
        n_rows = int(total) if q_max_rows is None else int(q_max_rows)
        opt = _options(FxMapExpectOptions, EXPECT_DEFAULTS, "expect", opts)
        error = f"outputs must be contiguous torch.int32 tensors [8], [{self.max_landmarks}] and [{self.max_landmarks}] on {dev}"
        out = _out_tensor(out, (8,), torch.int32, dev, error, typed=True)
        expected, seen = (torch.zeros(self.max_landmarks, dtype=torch.int32, device=dev) if t is None else
                          _out_tensor(t, (self.max_landmarks,), torch.int32, dev, error, typed=True) for t in (expected, seen))
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_expect(self.ctx.handle, self.handle, C.c_void_p(kb.data_ptr()), int(scans), int(total), C.c_void_p(loc.data_ptr()),
                                         int(n_scans), C.c_void_p(map_id_of_row.data_ptr() if n_rows else None), n_rows, C.byref(opt), _ptr(out),
                                         _ptr(expected), _ptr(seen)))
        return out, expected, seen

    def discover(self, kp, loc, n_scans, map_id_of_row, q_max_rows=None, out=None, new_id=None, **opts):
        """fx_map_discover: the unexplained rows of localised scans that fall on one spot in min_obs scans of this call made landmarks
        (include/fx.h).  kp, loc, n_scans, map_id_of_row and q_max_rows are observe()'s.  opts: the fields of
        fx_map_discover_options (DISCOVER_DEFAULTS).  Returns (result, new_id_of_row): device torch.int32 tensors [16]
        (discover_records reads it) and [q_max_rows]; out / new_id reuse one, False passes NULL (None is returned in its place).
        Stream-correct like update(); never waits for the stream."""
        import torch
        kb, scans, total = kp
        dev = torch.device("cuda", self.ctx.device)
        n_rows = int(total) if q_max_rows is None else int(q_max_rows)
        opt = _options(FxMapDiscoverOptions, DISCOVER_DEFAULTS, "discover", opts)
        error = f"outputs must be contiguous torch.int32 tensors [16] and [{n_rows}] on {dev}"
        out = _out_tensor(out, (16,), torch.int32, dev, error, typed=True)
        new_id = _out_tensor(new_id, (n_rows,), torch.int32, dev, error, typed=True)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_discover(self.ctx.handle, self.handle, C.c_void_p(kb.data_ptr()), int(scans), int(total), C.c_void_p(loc.data_ptr()),
                                           int(n_scans), C.c_void_p(map_id_of_row.data_ptr() if n_rows else None), n_rows, C.byref(opt), _ptr(out),
                                           _ptr(new_id if n_rows else None)))
        return out, new_id

    def retire(self, expected, seen, remap=None, retired=None, result=None, **opts):
        """fx_map_retire: the landmarks that expect()'s counters condemn taken out, the others renumbered as compact() does, the
        counters renumbered with them (include/fx.h).  expected / seen: the device torch.int32 tensors [max_landmarks] that
        expect() accumulated.  opts: the fields of fx_map_retire_options (RETIRE_DEFAULTS).  Returns (remap, retired, result): device
        tensors torch.int32 [max_landmarks], torch.uint8 [max_landmarks] (1: a retired old id) and torch.int32 [8] (retire_records
        reads it); a tensor given reuses it, False passes NULL (None is returned in its place).  Never waits for the stream."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        n = self.max_landmarks
        opt = _options(FxMapRetireOptions, RETIRE_DEFAULTS, "retire", opts)
        for t in (expected, seen):
            _out_tensor(t, (n,), torch.int32, dev, f"the counters must be contiguous torch.int32 tensors [{n}] on {dev}", typed=True)
        remap = _out_tensor(remap, (n,), torch.int32, dev, f"remap must be a contiguous torch.int32 tensor [{n}] on {dev}", typed=True)
        retired = _out_tensor(retired, (n,), torch.uint8, dev, f"retired must be a contiguous torch.uint8 tensor [{n}] on {dev}", typed=True)
        result = _out_tensor(result, (8,), torch.int32, dev, f"result must be a contiguous torch.int32 tensor [8] on {dev}", typed=True)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_retire(self.ctx.handle, self.handle, _ptr(expected), _ptr(seen), C.byref(opt), _ptr(remap), _ptr(retired),
                                         _ptr(result)))
        return remap, retired, result

    def join_segments(self, src, dst, prior=None, prior_device=None, result=None, match=None, **opts):
        """fx_map_join_segments: the landmarks of segment src brought into segment dst's frame, the two segments made one
        (include/fx.h).  prior: (c, s, tx, ty, tz) on the host, or prior_device: a device address (an int) or a tensor of five
        doubles (a view of an fx_localization's dc), or neither: the identity.  opts: the fields of fx_map_join_options
        (JOIN_DEFAULTS).  Returns (result, match_of_landmark): device tensors of 120 bytes (join_records reads it) and
        torch.int32 [max_landmarks]; a tensor given reuses it, False passes NULL (None is returned in its place).  Stream-correct
        like merge(); never waits for the stream."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        opt = _options(FxMapJoinOptions, JOIN_DEFAULTS, "join", opts)
        result, match = self._result_and_match(JOIN_DTYPE, result, match)
        pose, prior_device = self._prior(prior, prior_device)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_join_segments(self.ctx.handle, self.handle, int(src) & 0xffffffff, int(dst) & 0xffffffff,
                                                pose, C.c_void_p(prior_device), C.byref(opt), _ptr(result), _ptr(match)))
        return result, match

    def close_loop(self, prior=None, prior_device=None, result=None, match=None, **opts):
        """fx_map_close_loop: the recent landmarks of a segment brought onto its old ones, the correction spread over the scans of
        the loop (include/fx.h).  prior: (c, s, tx, ty, tz) on the host, or prior_device: a device address (an int) or a tensor of
        five doubles (a view of an fx_localization's dc), or neither: the identity.  opts: the fields of fx_map_loop_options
        (LOOP_DEFAULTS).  Returns (result, match_of_landmark): device tensors of 144 bytes (loop_records reads it) and torch.int32
        [max_landmarks]; a tensor given reuses it, False passes NULL (None is returned in its place).  Stream-correct like
        merge(); never waits for the stream."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        opt = _options(FxMapLoopOptions, LOOP_DEFAULTS, "loop", opts)
        result, match = self._result_and_match(LOOP_DTYPE, result, match)
        pose, prior_device = self._prior(prior, prior_device)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_close_loop(self.ctx.handle, self.handle, pose, C.c_void_p(prior_device), C.byref(opt), _ptr(result), _ptr(match)))
        return result, match

    def find_loop(self, result=None, match=None, **opts):
        """fx_map_find_loop: the transform that lays the recent landmarks of a segment on its old ones (or on another segment's,
        target_segment), found without a prior (include/fx.h).  opts: the fields of fx_map_find_loop_options (FIND_DEFAULTS).
        Returns (result, match_of_landmark): device tensors of 136 bytes (find_loop_records reads it; its first five doubles are
        what close_loop and join_segments take as prior_device) and torch.int32 [max_landmarks]; a tensor given reuses it, match =
        False passes NULL (None is returned in its place).  Stream-correct like merge(); never waits for the stream."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        opt = _options(FxMapFindLoopOptions, FIND_DEFAULTS, "find-loop", opts)
        result, match = self._result_and_match(FIND_DTYPE, result, match)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_find_loop(self.ctx.handle, self.handle, C.byref(opt), C.c_void_p(result.data_ptr()), _ptr(match)))
        return result, match

    def loop_correct_poses(self, result, poses, first_global_scan, n_poses=None):
        """fx_map_loop_correct_poses: poses (a device tensor of fx_pose records, 48 bytes each: those of the global scans
        first_global_scan, first_global_scan + 1, ...) brought up to date in place by close_loop's result (its device tensor).
        Stream-correct like merge(); never waits for the stream."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        have = poses.numel() * poses.element_size() // POSE_DTYPE.itemsize
        n = have if n_poses is None else int(n_poses)
        if poses.device != dev or result.device != dev or not poses.is_contiguous() or n > have or result.numel() * result.element_size() != LOOP_DTYPE.itemsize:
            raise ValueError(f"the result must hold {LOOP_DTYPE.itemsize} bytes and poses {n} contiguous fx_pose records on {dev}")
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_loop_correct_poses(self.ctx.handle, C.c_void_p(result.data_ptr()), C.c_void_p(poses.data_ptr()),
                                                     int(first_global_scan) & 0xffffffff, n))
        return poses

    def export_state(self):
        """fx_map_export_host (waits for the stream): the map's whole state as the bytes of one snapshot."""
        n = C.c_size_t()
        check(self.lib.fx_map_export_host(self.ctx.handle, self.handle, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        check(self.lib.fx_map_export_host(self.ctx.handle, self.handle, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def import_state(self, data):
        """fx_map_import_host: the snapshot `data` (bytes) becomes this map's state, in stream order; a block the check refuses
        raises FxError and leaves the map as it was."""
        data = bytes(data)
        check(self.lib.fx_map_import_host(self.ctx.handle, self.handle, data, len(data)))

    def _append_result(self, result):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        return dev, _out_tensor(result, (8,), torch.int32, dev, f"result must be a contiguous torch.int32 tensor [8] on {dev}", typed=True)

    def append(self, src, result=None):
        """fx_map_append: the Map `src` (of the same context; it is only read) appended behind this map's landmarks (include/fx.h).
        Returns the fx_map_append_result as a device torch.int32 tensor [8] (append_records reads it); `result` reuses one,
        result=False passes NULL (None is returned).  Stream-correct like merge(); never waits for the stream."""
        dev, result = self._append_result(result)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_append(self.ctx.handle, self.handle, src.handle, _ptr(result)))
        return result

    def append_state(self, data, result=None):
        """fx_map_append_host: the snapshot `data` (bytes: export_state() of a map of any context or device) appended behind this
        map's landmarks; a block the check refuses raises FxError and leaves the map as it was.  Returns what append() returns."""
        data = bytes(data)
        dev, result = self._append_result(result)
        with _on_stream(self.ctx.stream_ptr(), dev):
            check(self.lib.fx_map_append_host(self.ctx.handle, self.handle, data, len(data), _ptr(result)))
        return result

    def alias(self, first=0, count=None):
        """fx_map_read_alias (waits for the stream): alias[first, first + count) as int32, -1 for a live landmark, else the id of
        the live landmark that absorbed it; count defaults to the rest of max_landmarks."""
        count = self.max_landmarks - first if count is None else int(count)
        out = np.zeros(count, np.int32)
        check(self.lib.fx_map_read_alias(self.ctx.handle, self.handle, int(first), count, C.c_void_p(out.ctypes.data)))
        return out

    def alias_device_pointer(self):
        """fx_map_get_alias: the device address of the alias table, int32 [max_landmarks]."""
        a = C.c_void_p()
        check(self.lib.fx_map_get_alias(self.handle, C.byref(a)))
        return a.value

    def device_pointers(self):
        """fx_map_get: the device addresses of (the fx_map_header, the fx_map_landmark records)."""
        h, l = C.c_void_p(), C.c_void_p()
        check(self.lib.fx_map_get(self.handle, C.byref(h), C.byref(l)))
        return h.value, l.value

    def header(self):
        """fx_map_read_header (waits for the stream): the counts and last_pose, a 7-tuple (c, s, tx, ty, tz, segment, flags)."""
        h = FxMapHeader()
        check(self.lib.fx_map_read_header(self.ctx.handle, self.handle, C.byref(h)))
        out = {k: int(getattr(h, k)) for k in MAP_HEADER_FIELDS}
        p = h.last_pose
        out["last_pose"] = (p.c, p.s, p.tx, p.ty, p.tz, int(p.segment), int(p.flags))
        return out

    def landmarks(self, first=0, count=None):
        """fx_map_read_landmarks (waits for the stream): records [first, first + count) as MAP_LANDMARK_DTYPE; count defaults to the
        rest of max_landmarks."""
        count = self.max_landmarks - first if count is None else int(count)
        out = np.zeros(count, MAP_LANDMARK_DTYPE)
        check(self.lib.fx_map_read_landmarks(self.ctx.handle, self.handle, int(first), count, C.c_void_p(out.ctypes.data)))
        return out

    def records(self):
        """{"header": header(), "landmarks": the n_landmarks records stored} (waits for the stream)."""
        h = self.header()
        return {"header": h, "landmarks": self.landmarks(0, h["n_landmarks"])}


class Context:
    """Thin owner of an fx_ctx."""

    def __init__(self, p, lim, device=0):
        self.lib = load()
        self.device = device
        self.params, self.limits = p, lim
        self.handle = C.c_void_p()
        check(self.lib.fx_create(C.byref(p), C.byref(lim), device, C.byref(self.handle)))
        got = FxLimits()
        check(self.lib.fx_get_limits(self.handle, C.byref(got)))
        self.limits = got

    def close(self):
        if self.handle:
            self.lib.fx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        check(self.lib.fx_set_stream(self.handle, C.c_void_p(stream_ptr)))

    def stream_ptr(self):
        """The hipStream_t the context launches on, as an integer (torch.cuda.ExternalStream(ptr) wraps it)."""
        p = C.c_void_p()
        check(self.lib.fx_get_stream(self.handle, C.byref(p)))
        return p.value or 0

    def set_batches_in_flight(self, n):
        """Launch-policy hint: how many contexts the caller keeps busy on this device at a time (results never depend on it)."""
        check(self.lib.fx_set_batches_in_flight(self.handle, int(n)))

    def set_graph_batch(self, max_batch):
        check(self.lib.fx_set_graph_batch(self.handle, int(max_batch)))

    def set_profiling(self, depth, stages=None):
        """depth > 0: keep HIP-event timings of the last `depth` batches; stages: names to time (default all)."""
        check(self.lib.fx_set_profiling(self.handle, int(depth)))
        mask = 0xffffffff if stages is None else sum(1 << STAGE_NAMES.index(n) for n in stages)
        check(self.lib.fx_set_profiling_stages(self.handle, mask))

    def timings(self, back=0):
        """Per-kernel device ms (HIP events on the launch stream) of the batch `back` calls ago."""
        t = FxTimings()
        check(self.lib.fx_get_timings(self.handle, back, C.byref(t)))
        self.last_k_prep_exec_ms = t.k_prep_exec_ms
        return {STAGE_NAMES[i]: t.ms[i] for i in range(FX_N_STAGES)}, t.total_ms

    def front_active(self):
        """True when the last batch went through the fused front kernel (k_front: stages 0-4 in one launch)."""
        self.lib.fx_debug_front.argtypes = [C.c_void_p]
        self.lib.fx_debug_front.restype = C.c_int
        return bool(self.lib.fx_debug_front(self.handle))

    def stage_bytes(self):
        """Algorithmic bytes (read, written) per stage of the last batch: {stage: (read, written)}."""
        sb = FxStageBytes()
        check(self.lib.fx_get_stage_bytes(self.handle, C.byref(sb)))
        return {STAGE_NAMES[i]: (sb.read[i], sb.written[i]) for i in range(FX_N_STAGES)}

    def pack_keypoint_records(self, dst_device_ptr, rec_keypoints):
        check(self.lib.fx_pack_keypoint_records(self.handle, C.c_void_p(dst_device_ptr), rec_keypoints))

    def pack_keypoint_block(self, dst_device_ptr, max_scans, max_total_keypoints):
        """The last batch's keypoints as one compact block (fx_pack_keypoint_block; layout: sharding.unpack_block)."""
        check(self.lib.fx_pack_keypoint_block(self.handle, C.c_void_p(dst_device_ptr), int(max_scans), int(max_total_keypoints)))

    def synchronize(self):
        check(self.lib.fx_synchronize(self.handle))

    def gather_state(self):
        """fx_test_gather_state (the test build only): what the support gather of the last batch left on the device, as numpy
        copies — near_bits [B, near_words], s_cnt [rows], s_pts [rows, list_cap, 4] (float32; word 3 holds the point's index as
        bits), ovf_cnt [B], ovf_pts [B, ovf_stored, 4], ovf_kp [B, ovf_stored], row_map [rows, 2], row_kp [rows, 4], row_class
        [rows], row_xa [rows, 2], the work lists list_desc, wave_desc, group_desc (a list of three), dense_rows cut to their
        counters — and the reported constants (r2_support, r2_search, box_margin as np.float32; list_cap, ovf_cap, dense_min,
        near_words, batch, rows; n_list, n_wave, n_group, n_dense)."""
        info = FxTestGatherInfo()
        check(self.lib.fx_test_gather_state(self.handle, C.byref(info), None))
        B, rows, S = info.batch, info.rows, info.ovf_stored
        n_group = [int(v) for v in info.n_group]
        shapes = {"near_bits": ((B, info.near_words), np.uint32), "s_cnt": ((rows,), np.uint32), "s_pts": ((rows, info.list_cap, 4), np.float32),
                  "ovf_cnt": ((B,), np.uint32), "ovf_pts": ((B, S, 4), np.float32), "ovf_kp": ((B, S), np.uint32),
                  "row_map": ((rows, 2), np.uint32), "row_kp": ((rows, 4), np.float32), "row_class": ((rows,), np.uint8),
                  "row_xa": ((rows, 2), np.float32), "list_desc": ((min(info.n_list, rows),), np.uint32),
                  "wave_desc": ((min(info.n_wave, rows),), np.uint32), "group_desc": ((3, rows), np.uint32),
                  "dense_rows": ((min(info.n_dense, info.max_dense_rows),), np.uint32)}
        st = {k: np.zeros(sh, dt) for k, (sh, dt) in shapes.items()}
        out = FxTestGatherOut(**{k: st[k].ctypes.data if st[k].size else None for k in _GATHER_OUT})
        check(self.lib.fx_test_gather_state(self.handle, C.byref(info), C.byref(out)))
        st["group_desc"] = [st["group_desc"][g, :min(n_group[g], rows)].copy() for g in range(3)]
        for k in ("r2_support", "r2_search", "box_margin"):
            st[k] = np.float32(getattr(info, k))
        for k in ("batch", "rows", "near_words", "list_cap", "ovf_cap", "dense_min", "max_dense_rows", "n_list", "n_wave", "n_dense"):
            st[k] = int(getattr(info, k))
        st["n_group"] = n_group
        return st

    def set_descriptor_csr_capacity(self, entries):
        """Initial entries of the context's CSR block (0: max_total_keypoints * 128); it grows when a batch needs more."""
        check(self.lib.fx_set_descriptor_csr_capacity(self.handle, int(entries)))

    def pack_descriptors_csr(self, dst_device_ptr, max_rows, capacity):
        """fx_pack_descriptors_csr: the last batch's descriptor rows as a CSR block at dst (enqueued on the context's stream)."""
        check(self.lib.fx_pack_descriptors_csr(self.handle, C.c_void_p(dst_device_ptr), int(max_rows), int(capacity)))

    def descriptors_csr_host(self):
        """The last FX_OUT_DESC_CSR batch's rows (fx_get_descriptors_csr) as numpy copies: (row_ptr, col, val)."""
        v = FxDescriptorCsrView()
        check(self.lib.fx_get_descriptors_csr(self.handle, C.byref(v)))
        return (_np(v.h_row_ptr, (v.rows + 1,), np.uint32), _np(v.h_col, (v.nnz,), np.uint32), _np(v.h_val, (v.nnz,), np.float32))

    def descriptors_csr(self, buf=None, max_rows=None, capacity=None):
        """The last batch's descriptor rows packed on the GPU (fx_pack_descriptors_csr) into `buf` — a device torch.uint8 tensor of
        fx_descriptor_csr_bytes(max_rows, capacity) bytes, allocated here when None — and returned as a torch.sparse_csr_tensor of
        shape (min(rows, max_rows), 1989) whose int32 row_ptr / col and float32 values are views of `buf`, plus the header
        {rows, nnz_stored, nnz_needed, rows_stored}.  max_rows defaults to max_total_keypoints.  Without `buf` and `capacity`
        the block starts at 128 entries a row and is allocated again at nnz_needed when the rows need more (nothing is cut);
        a block the caller sizes may come back cut (rows_stored < rows: the leading rows_stored rows only).
        Stream-correct: the pack runs on the context's stream after the work the caller's current stream has queued, and the
        caller's current stream waits for it."""
        import torch
        max_rows = self.limits.max_total_keypoints if max_rows is None else int(max_rows)
        grow = buf is None and capacity is None
        capacity = max_rows * 128 if capacity is None else int(capacity)
        dev = torch.device("cuda", self.device)
        while True:
            nbytes = int(self.lib.fx_descriptor_csr_bytes(max_rows, capacity))
            if buf is None:
                buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            elif buf.dtype != torch.uint8 or buf.device != dev or buf.numel() < nbytes or not buf.is_contiguous() or buf.data_ptr() % 16:
                raise ValueError(f"buf must be a contiguous, 16-byte aligned torch.uint8 tensor of >= {nbytes} bytes on {dev}")
            # (the pack comes after the buffer's allocation / the caller's last use of it, and the caller's stream waits for the pack,
            #  so the buffer's later reuse on it comes after; no record_stream: the allocator would record events on the context's
            #  stream when the tensor dies, after fx_destroy perhaps)
            with _on_stream(self.stream_ptr(), dev):
                self.pack_descriptors_csr(buf.data_ptr(), max_rows, capacity)
            h = buf[:16].view(torch.int32).cpu().tolist()
            if not (grow and h[3] < min(h[0], max_rows)):
                break
            buf, capacity = None, h[2]  # (nnz_needed: every row; the dense rows are intact until the next batch)
        hdr = {"rows": h[0], "nnz_stored": h[1], "nnz_needed": h[2], "rows_stored": h[3]}
        rp, col, val, _ = csr_layout(max_rows, capacity)
        n, nnz = min(h[0], max_rows), h[1]
        t = torch.sparse_csr_tensor(buf[rp:rp + 4 * (n + 1)].view(torch.int32), buf[col:col + 4 * nnz].view(torch.int32),
                                    buf[val:val + 4 * nnz].view(torch.float32), size=(n, FX_DESC_FLOATS))
        return t, hdr

    def match_descriptors(self, q, t, pairs, out=None, shifts=12, max_dist2=float("inf"), max_ratio=1.0, mutual=False):
        """fx_match_descriptors_csr: q and t are CSR blocks as (torch.uint8 device buffer, max_rows, capacity) — what
        descriptors_csr(buf, max_rows, capacity) filled; the same block twice matches scans inside one batch —, pairs a list of
        (q_row0, q_rows, t_row0, t_rows) (pairs_consecutive).  Returns a device torch.int32 tensor [q_max_rows, 8], one fx_match
        record a query row (match_records views a host copy as named fields); `out` reuses a tensor of that shape.
        Stream-correct like descriptors_csr: the match runs on the context's stream after what the caller's current stream has
        queued, and the caller's current stream waits for it."""
        import torch
        (qb, q_rows, q_cap), (tb, t_rows, t_cap) = q, t
        dev = torch.device("cuda", self.device)
        for b, r, cap in ((qb, q_rows, q_cap), (tb, t_rows, t_cap)):
            nbytes = int(self.lib.fx_descriptor_csr_bytes(int(r), int(cap)))
            if b.dtype != torch.uint8 or b.device != dev or b.numel() < nbytes or not b.is_contiguous() or b.data_ptr() % 16:
                raise ValueError(f"a block must be a contiguous, 16-byte aligned torch.uint8 tensor of >= {nbytes} bytes on {dev}")
        if out is None:
            out = torch.empty((int(q_rows), 8), dtype=torch.int32, device=dev)
        elif out.dtype != torch.int32 or out.device != dev or tuple(out.shape) != (int(q_rows), 8) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous torch.int32 tensor [{int(q_rows)}, 8] on {dev}")
        arr = (FxMatchPair * max(len(pairs), 1))()
        for i, pr in enumerate(pairs):
            arr[i].q_row0, arr[i].q_rows, arr[i].t_row0, arr[i].t_rows = (int(x) for x in pr)
        opt = FxMatchOptions()
        self.lib.fx_match_options_default(C.byref(opt))
        opt.azimuth_shifts, opt.max_dist2, opt.max_ratio, opt.mutual = int(shifts), float(max_dist2), float(max_ratio), int(bool(mutual))
        with _on_stream(self.stream_ptr(), dev):
            check(self.lib.fx_match_descriptors_csr(self.handle, C.c_void_p(qb.data_ptr()), int(q_rows), int(q_cap), C.c_void_p(tb.data_ptr()),
                                                    int(t_rows), int(t_cap), arr, len(pairs), C.byref(opt), C.c_void_p(out.data_ptr())))
        return out

    def register_matches(self, q_kp, t_kp, matches, pairs, out=None, inliers=None, **opts):
        """fx_register_matches: q_kp and t_kp are keypoint blocks as (device tensor, max_scans, max_total_keypoints) — what
        pack_keypoint_block filled —, matches the device torch.int32 tensor [q_max_rows, 8] match_descriptors returned for the
        same `pairs`.  opts: inlier_dist, min_baseline, hyp_corr, min_inliers, require_flags (fx_register_options).  Returns
        (out, inliers): a device torch.float64 tensor [n_pairs, 8] holding one 64-byte fx_registration a pair (register_records
        views a host copy as named fields) and a device torch.int32 tensor [q_max_rows] of inlier words; `out` / `inliers` reuse
        tensors of those shapes, inliers=False passes NULL (no inlier words; None is returned for them).
        Stream-correct like match_descriptors."""
        import torch
        (qb, q_scans, q_total), (tb, t_scans, t_total) = q_kp, t_kp
        dev = torch.device("cuda", self.device)
        for b, sc, tot in ((qb, q_scans, q_total), (tb, t_scans, t_total)):
            nbytes = int(self.lib.fx_keypoint_block_bytes(int(sc), int(tot)))
            if b.device != dev or b.numel() * b.element_size() < nbytes or not b.is_contiguous() or b.data_ptr() % 16:
                raise ValueError(f"a keypoint block must be a contiguous, 16-byte aligned tensor of >= {nbytes} bytes on {dev}")
        if matches.dtype != torch.int32 or matches.device != dev or matches.dim() != 2 or matches.shape[1] != 8 or not matches.is_contiguous():
            raise ValueError(f"matches must be a contiguous torch.int32 tensor [q_max_rows, 8] on {dev}")
        n_rows, n_pairs = int(matches.shape[0]), len(pairs)
        if out is None:
            out = torch.empty((n_pairs, 8), dtype=torch.float64, device=dev)
        elif out.dtype != torch.float64 or out.device != dev or tuple(out.shape) != (n_pairs, 8) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous torch.float64 tensor [{n_pairs}, 8] on {dev}")
        inliers = _out_tensor(inliers, (n_rows,), torch.int32, dev, f"inliers must be a contiguous torch.int32 tensor [{n_rows}] on {dev}", typed=True)
        arr = (FxMatchPair * max(n_pairs, 1))()
        for i, pr in enumerate(pairs):
            arr[i].q_row0, arr[i].q_rows, arr[i].t_row0, arr[i].t_rows = (int(x) for x in pr)
        opt = FxRegisterOptions()
        self.lib.fx_register_options_default(C.byref(opt))
        for k, v in opts.items():
            if k not in REG_DEFAULTS:
                raise TypeError(f"unknown option {k!r}")
            setattr(opt, k, float(v) if k in ("inlier_dist", "min_baseline") else int(v))
        with _on_stream(self.stream_ptr(), dev):
            check(self.lib.fx_register_matches(self.handle, C.c_void_p(qb.data_ptr()), int(q_scans), int(q_total), C.c_void_p(tb.data_ptr()),
                                               int(t_scans), int(t_total), C.c_void_p(matches.data_ptr()), n_rows, arr, n_pairs, C.byref(opt),
                                               C.c_void_p(out.data_ptr()), _ptr(inliers)))
        return out, inliers

    def track_landmarks(self, kp, matches, inliers, reg, n_scans, init_pose=None, min_obs=2, max_landmarks=None, out=None):
        """fx_track_landmarks: kp is the keypoint block as (device tensor, max_scans, max_total_keypoints), matches / inliers / reg the
        device tensors match_descriptors and register_matches returned for pairs_consecutive of that block's scans.  init_pose:
        (c, s, tx, ty, tz) or None; max_landmarks defaults to q_max_rows.  Returns the device tensors (poses float64 [n_scans, 6],
        landmark_of_row int32 [q_max_rows], obs_row int32 [q_max_rows], landmarks float64 [max_landmarks, 6], header int32 [8]);
        `out` reuses a tuple of such tensors.  track_records views host copies of them as named fields.
        Stream-correct like register_matches."""
        import torch
        kb, scans, total = kp
        dev = torch.device("cuda", self.device)
        nbytes = int(self.lib.fx_keypoint_block_bytes(int(scans), int(total)))
        if kb.device != dev or kb.numel() * kb.element_size() < nbytes or not kb.is_contiguous() or kb.data_ptr() % 16:
            raise ValueError(f"the keypoint block must be a contiguous, 16-byte aligned tensor of >= {nbytes} bytes on {dev}")
        if matches.dtype != torch.int32 or matches.device != dev or matches.dim() != 2 or matches.shape[1] != 8 or not matches.is_contiguous():
            raise ValueError(f"matches must be a contiguous torch.int32 tensor [q_max_rows, 8] on {dev}")
        n_rows, n_scans = int(matches.shape[0]), int(n_scans)
        if inliers.dtype != torch.int32 or inliers.device != dev or tuple(inliers.shape) != (n_rows,) or not inliers.is_contiguous():
            raise ValueError(f"inliers must be a contiguous torch.int32 tensor [{n_rows}] on {dev}")
        if reg.dtype != torch.float64 or reg.device != dev or reg.dim() != 2 or reg.shape[1] != 8 or reg.shape[0] < n_scans - 1 or not reg.is_contiguous():
            raise ValueError(f"reg must be a contiguous torch.float64 tensor [>= {n_scans - 1}, 8] on {dev}")
        max_landmarks = n_rows if max_landmarks is None else int(max_landmarks)
        shapes = (((max(n_scans, 0), 6), torch.float64), ((n_rows,), torch.int32), ((n_rows,), torch.int32), ((max_landmarks, 6), torch.float64),
                  ((8,), torch.int32))
        if out is None:
            out = tuple(torch.empty(sh, dtype=dt, device=dev) for sh, dt in shapes)
        for t, (sh, dt) in zip(out, shapes):
            if t.dtype != dt or t.device != dev or tuple(t.shape) != sh or not t.is_contiguous():
                raise ValueError(f"out must hold contiguous tensors of {shapes} on {dev}")
        poses, lor, obs, lms, hdr = out
        ip = None
        if init_pose is not None:
            ip = FxPose(*(float(v) for v in init_pose), 0, 0)
        opt = FxTrackOptions()
        self.lib.fx_track_options_default(C.byref(opt))
        opt.min_obs = int(min_obs)
        with _on_stream(self.stream_ptr(), dev):
            check(self.lib.fx_track_landmarks(self.handle, C.c_void_p(kb.data_ptr()), int(scans), int(total), C.c_void_p(matches.data_ptr()),
                                              C.c_void_p(inliers.data_ptr()), n_rows, C.c_void_p(reg.data_ptr()), n_scans,
                                              C.byref(ip) if ip is not None else None, C.byref(opt), C.c_void_p(poses.data_ptr()),
                                              C.c_void_p(lor.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(lms.data_ptr()), max_landmarks,
                                              C.c_void_p(hdr.data_ptr())))
        return out

    def splice_blocks(self, a, b, dst_kp, dst_csr=None):
        """fx_splice_blocks: a and b are sources as ((kp tensor, max_scans, max_total_keypoints), (CSR tensor, max_rows, capacity) or
        None, scan0, n_scans) — scan0 may be FX_SPLICE_LAST_SCAN, n_scans 0xffffffff —, dst_kp the destination keypoint block as
        (device tensor, max_scans, max_total_keypoints) and dst_csr its CSR block as (torch.uint8 device tensor, max_rows, capacity) or
        None: keypoints only.  The destination is what the two packs would write for a batch of a's selected scans, then b's
        (include/fx.h).  Returns (dst_kp, dst_csr).  Stream-correct like match_descriptors; never waits for the stream."""
        import torch
        dev = torch.device("cuda", self.device)

        def fits(t, nbytes):
            if t.device != dev or t.numel() * t.element_size() < nbytes or not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError(f"a block must be a contiguous, 16-byte aligned tensor of >= {nbytes} bytes on {dev}")
            return t.data_ptr()
        src = []
        for (kb, scans, total), csr, scan0, n_scans in (a, b):
            s = FxSpliceSource(fits(kb, int(self.lib.fx_keypoint_block_bytes(int(scans), int(total)))), int(scans), int(total), None, 0, 0,
                               int(scan0) & 0xffffffff, int(n_scans) & 0xffffffff)
            if csr is not None:
                s.csr_block_device, s.max_rows, s.capacity = fits(csr[0], int(self.lib.fx_descriptor_csr_bytes(int(csr[1]), int(csr[2])))), int(csr[1]), int(csr[2])
            src.append(s)
        kp_ptr = fits(dst_kp[0], int(self.lib.fx_keypoint_block_bytes(int(dst_kp[1]), int(dst_kp[2]))))
        csr_ptr, rows, cap = (fits(dst_csr[0], int(self.lib.fx_descriptor_csr_bytes(int(dst_csr[1]), int(dst_csr[2])))), int(dst_csr[1]), int(dst_csr[2])) if dst_csr is not None else (None, 0, 0)
        with _on_stream(self.stream_ptr(), dev):
            check(self.lib.fx_splice_blocks(self.handle, C.byref(src[0]), C.byref(src[1]), C.c_void_p(kp_ptr), int(dst_kp[1]), int(dst_kp[2]),
                                            C.c_void_p(csr_ptr), rows, cap))
        return dst_kp, dst_csr

    def deskew_keypoint_block(self, kp, motions, n_scans, dst=None, out=None, **opts):
        """fx_deskew_keypoint_block: kp is the source keypoint block as (device tensor, max_scans, max_total_keypoints), motions the
        device torch.float64 tensor [n, 8] of fx_registration records register_matches returned for pairs_consecutive
        (FX_DESKEW_LINKS, n >= n_scans - 1; None with n_scans == 1) or one record a scan (FX_DESKEW_PER_SCAN, n >= n_scans).  dst: the
        destination block's tensor (None allocates one; kp's own tensor: in place); out: a device torch.int32 tensor [n_scans, 4] to
        reuse.  opts: the fields of fx_deskew_options (DESKEW_DEFAULTS).  Returns ((dst, max_scans, max_total_keypoints), out);
        deskew_records views a host copy of `out` as named fields.  Stream-correct like match_descriptors; never waits for the
        stream."""
        import torch
        kb, scans, total = kp
        dev = torch.device("cuda", self.device)
        nbytes, n_scans = int(self.lib.fx_keypoint_block_bytes(int(scans), int(total))), int(n_scans)
        if dst is None:
            dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for b in (kb, dst):
            if b.device != dev or b.numel() * b.element_size() < nbytes or not b.is_contiguous() or b.data_ptr() % 16:
                raise ValueError(f"a keypoint block must be a contiguous, 16-byte aligned tensor of >= {nbytes} bytes on {dev}")
        opt = _options(FxDeskewOptions, DESKEW_DEFAULTS, "deskew", opts)
        opt.direction = int(dict(DESKEW_DEFAULTS, **opts)["direction"])
        need = n_scans if opt.source == FX_DESKEW_PER_SCAN else n_scans - 1
        if motions is not None and (motions.dtype != torch.float64 or motions.device != dev or motions.dim() != 2 or motions.shape[1] != 8 or
                                    motions.shape[0] < need or not motions.is_contiguous()):
            raise ValueError(f"motions must be a contiguous torch.float64 tensor [>= {need}, 8] on {dev}")
        out = _out_tensor(out, (max(n_scans, 0), 4), torch.int32, dev, f"out must be a contiguous torch.int32 tensor [{n_scans}, 4] on {dev}", typed=True)
        with _on_stream(self.stream_ptr(), dev):
            check(self.lib.fx_deskew_keypoint_block(self.handle, C.c_void_p(kb.data_ptr()), C.c_void_p(dst.data_ptr()), int(scans), int(total),
                                                    _ptr(motions), n_scans, C.byref(opt), C.c_void_p(out.data_ptr())))
        return (dst, int(scans), int(total)), out

    def map_create(self, max_landmarks, max_carry_rows):
        """fx_map_create: a persistent landmark map owned by this context (Map.update after every track_landmarks)."""
        return Map(self, max_landmarks, max_carry_rows)

    def make_descs(self, ptrs, counts, stride_bytes=16, roll=0.0, pitch=0.0):
        n = len(ptrs)
        arr = (FxScanDesc * n)()
        for i in range(n):
            arr[i].points = ptrs[i]
            arr[i].n_points = int(counts[i])
            arr[i].stride_bytes = stride_bytes
            arr[i].roll = roll[i] if np.ndim(roll) else roll
            arr[i].pitch = pitch[i] if np.ndim(pitch) else pitch
        return arr

    def process_raw(self, descs, batch, flags):
        view = FxBatchView()
        check(self.lib.fx_process_batch(self.handle, descs, batch, flags, C.byref(view)))
        return view

    def process_host(self, scans, roll=0.0, pitch=0.0, debug=True, descriptors="dense"):
        """scans: list of [N,4] (or [N,8]) float32 arrays on the host.  Returns a list of dicts.  descriptors="csr": the rows come
        back through FX_OUT_DESC_CSR and every dict carries desc_csr = (row_ptr, col, val) of its own rows (row_ptr from 0)
        instead of the dense "descriptors"."""
        if descriptors not in ("dense", "csr"):
            raise ValueError(f"descriptors must be 'dense' or 'csr', not {descriptors!r}")
        scans = [np.ascontiguousarray(s, dtype=np.float32) for s in scans]
        stride = scans[0].shape[1] * 4 if scans else 16
        descs = self.make_descs([s.ctypes.data for s in scans], [s.shape[0] for s in scans], stride, roll, pitch)
        flags = FX_OUT_HOST | FX_OUT_CLOUDS | (FX_OUT_DEBUG if debug else 0) | (FX_OUT_DESC_CSR if descriptors == "csr" else 0)
        v = self.process_raw(descs, len(scans), flags)
        out = self.unpack(v, debug)
        if descriptors == "csr":
            rp, col, val = self.descriptors_csr_host()
            off = _np(v.h_kp_offset, (v.batch + 1,), np.uint32)
            for b, d in enumerate(out):
                del d["descriptors"]
                o0, o1 = min(int(off[b]), v.total_keypoints), min(int(off[b]) + d["n_keypoints"], v.total_keypoints)
                if o1 >= len(rp):  # (estimate_descriptors = 0: no rows)
                    o0 = o1 = 0
                d["rows"] = o1 - o0
                lo, hi = int(rp[o0]), int(rp[o1])
                d["desc_csr"] = (rp[o0:o1 + 1] - rp[o0], col[lo:hi], val[lo:hi])
        return out

    def unpack(self, v, debug=True):
        B = v.batch
        L = self.limits
        n_kp = _np(v.h_n_keypoints, (B,), np.uint32)
        off = _np(v.h_kp_offset, (B + 1,), np.uint32)
        flags = _np(v.h_flags, (B,), np.uint32)
        n_f = _np(v.h_n_filtered, (B,), np.uint32)
        n_kpc = _np(v.h_n_kpc, (B,), np.uint32)
        kp = _np(v.h_keypoints, (B, L.max_keypoints, 4), np.float32)
        desc = _np(v.h_descriptors, (v.total_keypoints, FX_DESC_FLOATS), np.float32)
        out = []
        if debug:
            n_c = _np(v.h_n_candidates, (B,), np.uint32)
        for b in range(B):
            # rows: the scan's descriptor rows the pool holds — its leading ones; n_keypoints unless FX_FLAG_TOTAL_KP_OVERFLOW
            # (include/fx.h "Cuts").  0 without descriptors.
            held = len(desc) if self.params.estimate_descriptors else 0
            r0, r1 = min(int(off[b]), held), min(int(off[b]) + int(n_kp[b]), held)
            d = {"flags": int(flags[b]), "n_keypoints": int(n_kp[b]), "keypoints": kp[b, :n_kp[b]], "rows": r1 - r0,
                 "descriptors": desc[r0:r1] if held else np.zeros((0, FX_DESC_FLOATS), np.float32)}
            if v.h_filtered:
                base = C.cast(v.h_filtered, C.c_void_p).value + b * L.max_points * 16
                d["filtered"] = _np(C.cast(base, _F32P), (int(n_f[b]), 4), np.float32)
                base = C.cast(v.h_kpc, C.c_void_p).value + b * L.max_kpc_points * 16
                d["kpc"] = _np(C.cast(base, _F32P), (int(n_kpc[b]), 4), np.float32)
            if debug:
                def row(ptr, width, dtype, n, comps=1):
                    base = C.cast(ptr, C.c_void_p).value + b * width * 4 * comps
                    return _np(C.cast(base, type(ptr)), (n, comps) if comps > 1 else (n,), dtype)
                nc = int(n_c[b])
                d["candidates"] = row(v.h_candidates, L.max_candidates, np.float32, nc, 4)
                d["cand_size"] = row(v.h_cand_size, L.max_candidates, np.uint32, nc)
                d["cand_keypoint"] = row(v.h_cand_keypoint, L.max_candidates, np.int32, nc)
                d["kpc_cand"] = row(v.h_kpc_cand, L.max_kpc_points, np.uint32, int(n_kpc[b]))
                d["kp_size"] = row(v.h_kp_size, L.max_keypoints, np.uint32, int(n_kp[b]))
                d["kp_neighbors"] = row(v.h_kp_neighbors, L.max_keypoints, np.uint32, int(n_kp[b]))
            out.append(d)
        return out
