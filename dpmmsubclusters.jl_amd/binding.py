"""ctypes binding of include/dpmm_hip.h and its companions dpmm_hip_master.h / dpmm_hip_debug.h.  No fallback: if libdpmmhip.so is missing or no
gfx950 device is usable, construction raises -- nothing here computes on the CPU."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PRIOR_NIW, PRIOR_MULT = 0, 1
MAX_CLUSTERS = 1024

_c_i64p = ctypes.POINTER(ctypes.c_int64)
_c_f32p = ctypes.POINTER(ctypes.c_float)
_c_f64p = ctypes.POINTER(ctypes.c_double)

# every symbol the three worker headers declare: (name, restype, argtypes)
ABI = [
    ("dpmm_abi_version", ctypes.c_int, []),
    ("dpmm_create", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64]),
    ("dpmm_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_last_error", ctypes.c_char_p, [ctypes.c_void_p]),
    ("dpmm_upload_points", ctypes.c_int, [ctypes.c_void_p, _c_f32p, ctypes.c_int64]),
    ("dpmm_upload_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    ("dpmm_upload_points_npy", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    ("dpmm_upload_points_csc", ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i64p, _c_f32p, ctypes.c_int]),
    ("dpmm_init_labels", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]),
    ("dpmm_set_labels", ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i64p]),
    ("dpmm_get_labels", ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i64p]),
    ("dpmm_set_params_niw", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p]),
    ("dpmm_set_params_niw_chol", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p]),
    ("dpmm_set_params_mult", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f32p, _c_f32p, _c_f32p]),
    ("dpmm_set_num_clusters", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_num_clusters", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_numa_node", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_niw_master_setup", ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_step_stats_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]),
    ("dpmm_step_master_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    ("dpmm_suffstats_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_niw_master_posterior", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("dpmm_niw_master_draw", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_niw_master_pairs_ahead", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_niw_master_pairs", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("dpmm_niw_master_put_rows", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_niw_master_rows", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    ("dpmm_niw_master_draws", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_debug_niw_draw_inputs", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_mult_master_setup", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_mult_master_draw", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_mult_master_draws", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    ("dpmm_mult_master_put_rows", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_mult_master_pairs_ahead", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_mult_master_marginals", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int)]),
    ("dpmm_mult_master_rows_on_demand", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_mult_master_rows_wait", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_sweep", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int]),
    ("dpmm_packed_stride", ctypes.c_int64, [ctypes.c_void_p]),
    ("dpmm_suffstats_packed_device", ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int, ctypes.c_void_p]),
    ("dpmm_suffstats_packed", ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int, _c_f64p]),
    ("dpmm_unpack_suffstats", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f64p, _c_f64p, _c_f64p, _c_f64p]),
    ("dpmm_split", ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i64p, ctypes.c_int, ctypes.c_uint32]),
    ("dpmm_merge", ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_i64p, ctypes.c_int]),
    ("dpmm_remove_empty", ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int]),
    ("dpmm_reset_sublabels", ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int, ctypes.c_uint32]),
    ("dpmm_set_predictive_niw", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p]),
    ("dpmm_set_predictive_mult", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f32p, _c_f32p]),
    ("dpmm_predict", ctypes.c_int, [ctypes.c_void_p, _c_f32p]),
    ("dpmm_predict_points", ctypes.c_int, [ctypes.c_void_p, _c_i64p, _c_f32p]),
    ("dpmm_set_ground_truth", ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int]),
    ("dpmm_contingency", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_i64p]),
    ("dpmm_bin_counts", ctypes.c_int, [ctypes.c_void_p, _c_i64p]),
    ("dpmm_smart_project", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _c_f64p, _c_f64p, _c_f64p, _c_i64p]),
    ("dpmm_smart_kmeans_iter", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _c_f64p]),
    ("dpmm_smart_assign", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_double]),
    ("dpmm_debug_loglik", ctypes.c_int, [ctypes.c_void_p, _c_f32p]),
    ("dpmm_sync", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_stream", ctypes.c_void_p, [ctypes.c_void_p]),
    ("dpmm_last_sweep_parts_ms", ctypes.c_int, [ctypes.c_void_p, _c_f32p]),
    ("dpmm_last_kernel_ms", ctypes.c_int, [ctypes.c_void_p, _c_f32p, _c_f32p]),
    ("dpmm_debug_counters", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]),
    ("dpmm_debug_sort_tables", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_debug_set_prelaunch_hook", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_init_labels_from", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32]),
    ("dpmm_set_option", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]),
    ("dpmm_params_staging", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int] + [ctypes.POINTER(ctypes.c_void_p)] * 6),
    ("dpmm_commit_params", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_suffstats_host", ctypes.c_int, [ctypes.c_void_p, _c_i64p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("dpmm_step_stats", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    ("dpmm_debug_subloglik", ctypes.c_int, [ctypes.c_void_p, _c_f32p]),
    ("dpmm_debug_ref_bracket", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, _c_f32p, _c_f32p]),
    ("dpmm_debug_pair_ball", ctypes.c_int, [ctypes.c_void_p, _c_f32p, _c_f32p]),
    ("dpmm_debug_pair_ball_sn2", ctypes.c_int, [ctypes.c_void_p, _c_f32p]),
    ("dpmm_debug_norm_cert_points", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8)]),
    ("dpmm_debug_bracket_big", ctypes.c_int, [ctypes.c_void_p, _c_f32p, ctypes.POINTER(ctypes.c_uint32)]),
    ("dpmm_debug_mult_draws_ahead", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]),
    ("dpmm_last_sweep_work", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("dpmm_comm_use_library", ctypes.c_int, [ctypes.c_char_p]),
    ("dpmm_comm_unique_id", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_comm_init", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    ("dpmm_comm_init_host", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_comm_info", ctypes.c_int, [ctypes.c_void_p, _c_i64p]),
    ("dpmm_last_comm_ms", ctypes.c_int, [ctypes.c_void_p, _c_f32p, _c_f32p]),
    ("dpmm_comm_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_comm_allgather_host", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
]

# include/dpmm_hip_tensor.h: caller-owned device memory in and out (additive; bound next to ABI)
ABI_TENSOR = [
    ("dpmm_upload_points_strided_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    ("dpmm_get_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    ("dpmm_get_labels_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_set_labels_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("dpmm_predict_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
]
# include/dpmm_hip_project.h: wide points projected to the ctx's dimension while they are read (additive)
_c_f64p_in = ctypes.POINTER(ctypes.c_double)
ABI_PROJECT = [
    ("dpmm_set_projection", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f64p_in, _c_f64p_in]),
    ("dpmm_upload_points_projected_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64]),
    ("dpmm_upload_points_projected", ctypes.c_int, [ctypes.c_void_p, _c_f32p, ctypes.c_int64]),
]
MAX_DIM_PROJECT_IN = 4096      # DPMM_MAX_DIM_PROJECT_IN
DT_F16, DT_BF16, DT_F32, DT_F64, DT_U8, DT_I16, DT_I32, DT_I64 = range(8)      # DPMM_DT_* (include/dpmm_hip_tensor.h)


class ScoreOut(ctypes.Structure):
    """dpmm_score_out (include/dpmm_hip_score.h): host or device addresses, 0 / None = not asked for."""
    _fields_ = [("labels", ctypes.c_void_p), ("logdens", ctypes.c_void_p), ("m", ctypes.c_int), ("top_idx", ctypes.c_void_p),
                ("top_prob", ctypes.c_void_p), ("probs", ctypes.c_void_p)]


# include/dpmm_hip_score.h: scoring new points (additive; bound next to ABI)
ABI_SCORE = [
    ("dpmm_score_points", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ScoreOut)]),
    ("dpmm_score_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ScoreOut)]),
]


class RankOut(ctypes.Structure):
    """dpmm_rank_out (include/dpmm_hip_rank.h): host or device addresses, 0 / None = not asked for."""
    _fields_ = [("typ_idx", ctypes.c_void_p), ("typ_score", ctypes.c_void_p), ("fringe_idx", ctypes.c_void_p), ("fringe_score", ctypes.c_void_p),
                ("count", ctypes.c_void_p), ("skipped", ctypes.c_void_p)]


# include/dpmm_hip_rank.h: exemplars, the m most and least typical points of every cluster (additive; bound next to ABI)
ABI_RANK = [
    ("dpmm_rank_begin", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    ("dpmm_rank_accumulate", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]),
    ("dpmm_rank_read", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RankOut)]),
    ("dpmm_rank_read_device", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RankOut)]),
]
RANK_MAX_M = 64                        # DPMM_RANK_MAX_M
RANK_TYPICAL, RANK_FRINGE = 1, 2       # DPMM_RANK_TYPICAL, DPMM_RANK_FRINGE


class OverlapOut(ctypes.Structure):
    """dpmm_overlap_out (include/dpmm_hip_overlap.h): host addresses, 0 / None = not asked for."""
    _fields_ = [("overlap", ctypes.c_void_p), ("mass", ctypes.c_void_p), ("count", ctypes.c_void_p), ("skipped", ctypes.c_void_p)]


# include/dpmm_hip_overlap.h: the posterior overlap of the clusters, sum_i p_ik p_ij (additive; bound next to ABI)
ABI_OVERLAP = [
    ("dpmm_overlap_begin", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_overlap_accumulate", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    ("dpmm_overlap_read", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(OverlapOut)]),
]
OVERLAP_PARTIAL_BLOCKS = 512           # DPMM_OVERLAP_PARTIAL_BLOCKS


class BatchStatsOut(ctypes.Structure):
    """dpmm_batchstats_out (include/dpmm_hip_batchstats.h): host addresses, 0 / None = not asked for."""
    _fields_ = [("N", ctypes.c_void_p), ("sums", ctypes.c_void_p), ("S", ctypes.c_void_p), ("count", ctypes.c_void_p), ("skipped", ctypes.c_void_p),
                ("incomplete", ctypes.c_void_p), ("held_out", ctypes.c_void_p)]


# include/dpmm_hip_batchstats.h: per-cluster sufficient statistics of a batch under the served model (additive; bound next to ABI)
ABI_BATCHSTATS = [
    ("dpmm_batchstats_begin", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float]),
    ("dpmm_batchstats_accumulate", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    ("dpmm_batchstats_read", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(BatchStatsOut)]),
]
BATCHSTATS_HARD, BATCHSTATS_SOFT = 0, 1    # DPMM_BATCHSTATS_HARD, DPMM_BATCHSTATS_SOFT
BATCHSTATS_PARTIAL_BLOCKS = 2048           # DPMM_BATCHSTATS_PARTIAL_BLOCKS


class CountStatsOut(ctypes.Structure):
    """dpmm_countstats_out (include/dpmm_hip_countstats.h): host addresses, 0 / None = not asked for."""
    _fields_ = [("N", ctypes.c_void_p), ("sums", ctypes.c_void_p), ("count", ctypes.c_void_p), ("skipped", ctypes.c_void_p),
                ("incomplete", ctypes.c_void_p), ("held_out", ctypes.c_void_p)]


# include/dpmm_hip_countstats.h: per-cluster count statistics of a batch under the served Multinomial model (additive; bound next to ABI)
ABI_COUNTSTATS = [
    ("dpmm_countstats_begin", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float]),
    ("dpmm_countstats_accumulate", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    ("dpmm_countstats_read", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CountStatsOut)]),
]
COUNTSTATS_PARTIAL_BYTES = 64 << 20        # DPMM_COUNTSTATS_PARTIAL_BYTES


class TypicalityOut(ctypes.Structure):
    """dpmm_typicality_out (include/dpmm_hip_typicality.h): host or device addresses (the two counters always host), 0 / None = not asked for."""
    _fields_ = [("labels", ctypes.c_void_p), ("mahalanobis", ctypes.c_void_p), ("tail", ctypes.c_void_p), ("skipped", ctypes.c_void_p),
                ("incomplete", ctypes.c_void_p)]


# include/dpmm_hip_typicality.h: calibrated outlier scores, the tail of a point's Mahalanobis distance under its own cluster (additive; bound next to ABI)
ABI_TYPICALITY = [
    ("dpmm_typicality_points", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(TypicalityOut)]),
    ("dpmm_typicality_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(TypicalityOut)]),
    ("dpmm_batchstats_set_min_tail", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float]),
]


class ExplainOut(ctypes.Structure):
    """dpmm_explain_out (include/dpmm_hip_explain.h): host or device addresses (the two counters always host), 0 / None = not asked for;
    top (0: all D features in order) and ld, the entries between two points' rows."""
    _fields_ = [("labels", ctypes.c_void_p), ("mahalanobis", ctypes.c_void_p), ("tail", ctypes.c_void_p), ("skipped", ctypes.c_void_p),
                ("incomplete", ctypes.c_void_p), ("residual", ctypes.c_void_p), ("zscore", ctypes.c_void_p), ("feature_tail", ctypes.c_void_p),
                ("features", ctypes.c_void_p), ("top", ctypes.c_int32), ("ld", ctypes.c_int64)]


# include/dpmm_hip_explain.h: per-feature conditional residuals, z-scores and tails of a point under its own cluster (additive; bound next to ABI)
ABI_EXPLAIN = [
    ("dpmm_explain_points", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ExplainOut)]),
    ("dpmm_explain_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ExplainOut)]),
]
EXPLAIN_MAX_TOP = 16                   # DPMM_EXPLAIN_MAX_TOP


class ExplainGroupsOut(ctypes.Structure):
    """dpmm_explain_groups_out (include/dpmm_hip_explain_groups.h): host or device addresses (the two counters always host), 0 / None = not
    asked for; ld, the entries between two points' rows."""
    _fields_ = [("labels", ctypes.c_void_p), ("mahalanobis", ctypes.c_void_p), ("tail", ctypes.c_void_p), ("skipped", ctypes.c_void_p),
                ("incomplete", ctypes.c_void_p), ("group_mahalanobis", ctypes.c_void_p), ("group_tail", ctypes.c_void_p), ("ld", ctypes.c_int64)]


# include/dpmm_hip_explain_groups.h: the conditional distance and tail of every group of features of a point (additive; bound next to ABI)
ABI_EXPLAIN_GROUPS = [
    ("dpmm_set_explain_groups", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_i64p, ctypes.POINTER(ctypes.c_int32), _c_f64p]),
    ("dpmm_explain_groups_points", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ExplainGroupsOut)]),
    ("dpmm_explain_groups_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ExplainGroupsOut)]),
]
EXPLAIN_MAX_GROUPS = 64                # DPMM_EXPLAIN_MAX_GROUPS


class HoldoutOut(ctypes.Structure):
    """dpmm_holdout_out (include/dpmm_hip_holdout.h): host addresses, 0 / None = not asked for."""
    _fields_ = [("total", ctypes.c_void_p), ("stored", ctypes.c_void_p), ("skipped", ctypes.c_void_p), ("incomplete", ctypes.c_void_p),
                ("scored", ctypes.c_void_p)]


# include/dpmm_hip_holdout.h: the held-out points of a batch, compacted on the GPU into the caller's device memory (additive; bound next to ABI)
ABI_HOLDOUT = [
    ("dpmm_holdout_begin", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_int64]),
    ("dpmm_holdout_accumulate", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]),
    ("dpmm_holdout_read", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HoldoutOut)]),
]


class CountHoldoutDst(ctypes.Structure):
    """dpmm_countholdout_dst (include/dpmm_hip_countholdout.h): device addresses -- points (dense stores) or colptr / rowval / val (sparse
    store), index -- and the two caps."""
    _fields_ = [("points", ctypes.c_void_p), ("colptr", ctypes.c_void_p), ("rowval", ctypes.c_void_p), ("val", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("cap", ctypes.c_int64), ("entry_cap", ctypes.c_int64)]


class CountHoldoutOut(ctypes.Structure):
    """dpmm_countholdout_out (include/dpmm_hip_countholdout.h): host addresses, 0 / None = not asked for."""
    _fields_ = [("total", ctypes.c_void_p), ("total_entries", ctypes.c_void_p), ("stored", ctypes.c_void_p), ("stored_entries", ctypes.c_void_p),
                ("skipped", ctypes.c_void_p), ("incomplete", ctypes.c_void_p), ("scored", ctypes.c_void_p)]


# include/dpmm_hip_countholdout.h: the floor per count and the held-out points of a batch of count data, compacted on the GPU (additive; bound next to ABI)
ABI_COUNTHOLDOUT = [
    ("dpmm_countstats_set_per_count", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float]),
    ("dpmm_countholdout_begin", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.POINTER(CountHoldoutDst)]),
    ("dpmm_countholdout_accumulate", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]),
    ("dpmm_countholdout_read", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CountHoldoutOut)]),
]
# include/dpmm_hip_trace.h: label samples kept on the GPU, their pairwise contingency tables and the per-point confidence (additive)
ABI_TRACE = [
    ("dpmm_trace_open", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("dpmm_trace_close", ctypes.c_int, [ctypes.c_void_p]),
    ("dpmm_trace_record", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    ("dpmm_trace_tables", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, _c_i64p]),
    ("dpmm_trace_confidence", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, _c_f32p, _c_f32p, ctypes.c_void_p]),
    ("dpmm_trace_read", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_i64p, ctypes.c_void_p]),
]
TRACE_MAX_SLOTS = 4096                 # DPMM_TRACE_MAX_SLOTS
# include/dpmm_hip_csc.h: sparse points out of caller-owned device memory (additive; bound next to ABI)
ABI_CSC = [
    ("dpmm_upload_points_csc_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                     ctypes.c_int64, ctypes.c_int]),
]


class SampleRequest(ctypes.Structure):
    """dpmm_sample_request (include/dpmm_hip_sample.h)."""
    _fields_ = [("i0", ctypes.c_int64), ("n", ctypes.c_int64), ("cluster_start", _c_i64p), ("seed", ctypes.c_uint64), ("trials", ctypes.c_int64),
                ("x", ctypes.c_void_p), ("ld", ctypes.c_int64), ("labels", ctypes.c_void_p), ("colptr", ctypes.c_void_p), ("nnz0", ctypes.c_int64),
                ("rowval", ctypes.c_void_p), ("nzval", ctypes.c_void_p), ("nnz_extent", ctypes.c_int64), ("nnz_out", _c_i64p)]


# include/dpmm_hip_sample.h: drawing points from a fitted model (additive; bound next to ABI)
ABI_SAMPLE = [
    ("dpmm_set_sampler_niw", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f32p, _c_f32p, _c_f32p]),
    ("dpmm_set_sampler_mult", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)]),
    ("dpmm_sample_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SampleRequest)]),
]
SAMPLE_MAX_TRIALS_SPARSE = 4096        # DPMM_SAMPLE_MAX_TRIALS_SPARSE
SAMPLE_MAX_TRIALS_DENSE = 1 << 24      # DPMM_SAMPLE_MAX_TRIALS_DENSE
OPT_SCORE_TABLE_MB = 32      # DPMM_OPT_SCORE_TABLE_MB
SCORE_MAX_TOP = 16           # DPMM_SCORE_MAX_TOP
# include/dpmm_hip_missing.h: points with missing (NaN) features, marginalised and imputed (additive; bound next to ABI)
ABI_MISSING = [
    ("dpmm_score_missing_counts", ctypes.c_int, [ctypes.c_void_p, _c_i64p]),
    ("dpmm_impute_points", ctypes.c_int, [ctypes.c_void_p, _c_f32p, ctypes.c_int64]),
    ("dpmm_impute_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
]
OPT_SCORE_MISSING = 33       # DPMM_OPT_SCORE_MISSING
SCORE_MAX_MISSING = 16       # DPMM_SCORE_MAX_MISSING
OPT_TYPICALITY_GAPS = 35     # DPMM_OPT_TYPICALITY_GAPS (include/dpmm_hip_typicality.h): typicality / explain marginalise a point's gaps
# include/dpmm_hip_impute.h: draws of the missing features from the fitted mixture (additive; bound next to ABI)
_IMPUTE_DRAW_TAIL = [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
ABI_IMPUTE = [
    ("dpmm_impute_draw_points", ctypes.c_int, [ctypes.c_void_p, _c_f32p] + _IMPUTE_DRAW_TAIL),
    ("dpmm_impute_draw_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + _IMPUTE_DRAW_TAIL),
]
IMPUTE_MAX_DRAWS = 1 << 26   # DPMM_IMPUTE_MAX_DRAWS
# include/dpmm_hip_regress.h: mixture regression, the given features to the targets (additive; bound next to ABI)
ABI_REGRESS = [
    ("dpmm_set_regression", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f64p, _c_f64p, _c_f64p, _c_f64p]),
    ("dpmm_regress_points", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _c_i64p]),
    ("dpmm_regress_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _c_i64p]),
]
REGRESS_MAX_TARGETS = 256    # DPMM_REGRESS_MAX_TARGETS
# include/dpmm_hip_regress_draw.h: draws of the targets from their conditional law (additive; bound next to ABI)
_REGRESS_DRAW_TAIL = _IMPUTE_DRAW_TAIL + [_c_i64p]
ABI_REGRESS_DRAW = [
    ("dpmm_set_regression_factor", ctypes.c_int, [ctypes.c_void_p, _c_f64p]),
    ("dpmm_regress_draw_points", ctypes.c_int, [ctypes.c_void_p, _c_f32p] + _REGRESS_DRAW_TAIL),
    ("dpmm_regress_draw_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + _REGRESS_DRAW_TAIL),
]
REGRESS_MAX_DRAWS = 1 << 26  # DPMM_REGRESS_MAX_DRAWS
# include/dpmm_hip_regress_cdf.h: conditional CDF and quantiles of the targets (additive; bound next to ABI)
ABI_REGRESS_CDF = [
    ("dpmm_regress_cdf_points", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _c_i64p]),
    ("dpmm_regress_cdf_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _c_i64p]),
    ("dpmm_set_regression_levels", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_f64p, _c_f64p]),
    ("dpmm_regress_quantile_points", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _c_i64p]),
    ("dpmm_regress_quantile_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _c_i64p]),
]
REGRESS_MAX_LEVELS = 16      # DPMM_REGRESS_MAX_LEVELS
# include/dpmm_hip_recommend.h: the m unseen features of largest next-count probability (Multinomial; additive; bound next to ABI)
_RECOMMEND_ARGS = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _c_i64p]
ABI_RECOMMEND = [
    ("dpmm_set_recommend", ctypes.c_int, [ctypes.c_void_p, _c_f64p]),
    ("dpmm_recommend_points", ctypes.c_int, _RECOMMEND_ARGS),
    ("dpmm_recommend_points_device", ctypes.c_int, _RECOMMEND_ARGS),
]
RECOMMEND_MAX_TOP = SCORE_MAX_TOP      # DPMM_RECOMMEND_MAX_TOP


class CountExplainOut(ctypes.Structure):
    """dpmm_count_explain_out (include/dpmm_hip_count_explain.h): host or device addresses (the two counters always host), 0 / None = not
    asked for; ld, the entries between two points' rows."""
    _fields_ = [("top", ctypes.c_int), ("side", ctypes.c_int), ("ld", ctypes.c_int64), ("features", ctypes.c_void_p), ("count", ctypes.c_void_p),
                ("expected", ctypes.c_void_p), ("residual", ctypes.c_void_p), ("feature_tail", ctypes.c_void_p), ("labels", ctypes.c_void_p),
                ("total", ctypes.c_void_p), ("skipped", ctypes.c_void_p), ("incomplete", ctypes.c_void_p)]


# include/dpmm_hip_count_explain.h: the features that put a count point out, with exact binomial tails (Multinomial; additive; bound next to ABI)
ABI_COUNT_EXPLAIN = [
    ("dpmm_set_count_explain", ctypes.c_int, [ctypes.c_void_p, _c_f64p, _c_f64p, ctypes.POINTER(ctypes.c_int32)]),
    ("dpmm_count_explain_points", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CountExplainOut)]),
    ("dpmm_count_explain_points_device", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CountExplainOut)]),
]
COUNT_EXPLAIN_MAX_TOP = SCORE_MAX_TOP      # DPMM_COUNT_EXPLAIN_MAX_TOP
COUNT_EXPLAIN_SIDES = {"both": 0, "over": 1, "under": 2}      # DPMM_COUNT_EXPLAIN_BOTH / _OVER / _UNDER

HOST_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int)   # dpmm_host_allreduce_fn

# dpmm_set_option keys (include/dpmm_hip.h)
MASTER_NSCALARS = 8          # DPMM_MASTER_NSCALARS
OPT_SCREEN_MARGIN, OPT_TAIL_SCREEN, OPT_PRESCREEN, OPT_ORDERED_SWEEP, OPT_MULT_FORCE_F32, OPT_STATS_ITEMS, OPT_STATS_GROUPS, OPT_TRACE_SLOW, OPT_LOGLIK_REF_CONST, OPT_WAVE_PRIO, OPT_MULT_NO_U8, OPT_SWEEP_GRID, OPT_SWEEP_QUEUE_ROUNDS, OPT_BALL_SCREEN, OPT_KERNEL_TIMING, OPT_STATS_DERIVE, OPT_NOISE_AHEAD, OPT_REF_BRACKET, OPT_SORT_TILE, OPT_ONE_COLLECTIVE, OPT_BF16_SCREENS, OPT_COMM_TIMEOUT_MS, OPT_DIRECTION_SCREEN, _OPT_RESERVED_24, OPT_MULT_DRAWS_AHEAD, OPT_B3_SUBLABELS, OPT_LEAN_TILES, OPT_MASTER_POLL, OPT_CHAIN_FUSION, OPT_LEAN_DIRECTION, OPT_PAIR_BALL = range(1, 32)
OPT_LEAN_NORM_CERT = 34      # DPMM_OPT_LEAN_NORM_CERT: 0 off | 1 (default) tight sn2 block where it pays | 2 always tight | 3 as 2, the neighbours keep sn (for A/B)
PB_MAXK = 256                # PB_MAXK (csrc/dpmm_kernels.h): the most clusters the pair-ball table, and with it the norm certificate, takes


class DpmmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libdpmmhip error {code}: {msg}")
        self.code = code


def lib_path():
    return os.path.join(_HERE, "lib", "libdpmmhip.so")


def locked_make(args, lock_dir):
    """Run `make` under an exclusive file lock: the ranks of a fresh multi-process launch all reach the lazy build at once and
    must not write the same .so concurrently."""
    import fcntl
    os.makedirs(lock_dir, exist_ok=True)
    with open(os.path.join(lock_dir, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            subprocess.check_call(args)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)


def build_library(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    if force:
        args.append("-B")
    locked_make(args, os.path.join(_HERE, "lib"))
    return lib_path()


_LIB = None


def _floor(v):
    """A floor as the C calls take it: (in use?, its value), None for a floor that is not in use."""
    return (0, 0.0) if v is None else (1, float(v))


def _device_addresses(*dst):
    """The device addresses (integers) of caller-owned destinations: torch tensors on the worker's GPU, addresses, or None (0)."""
    for a in dst:
        if hasattr(a, "data_ptr"):
            import torch
            torch.cuda.current_stream(a.device).synchronize()      # nothing queued on torch's stream still uses this memory
            break
    return [(a.data_ptr() if a.numel() else 0) if hasattr(a, "data_ptr") else int(a or 0) for a in dst]


ABI_VERSION = 3      # DPMM_ABI_VERSION of include/dpmm_hip.h this file is written against


def load_library():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            try:   # fresh checkout: compile for gfx950 (hipcc cross-compiles without a GPU); never falls back to CPU code
                build_library()
            except Exception as e:
                raise FileNotFoundError(f"{p} not built and building it failed ({e}): run __graft_entry__.build() "
                                        "(there is no CPU fallback)") from e
        # PyTorch ships its own libamdhip64 under the same SONAME.  Whichever copy is mapped first serves BOTH users; if
        # this library pulled in the system copy first, a later `import torch` (multi-GPU runs use torch.distributed)
        # would find no GPUs.  Mapping torch's copy first keeps one consistent HIP runtime in the process.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover  (torch is optional for single-GPU use)
            pass
        lib = ctypes.CDLL(p)
        for name, res, args in ABI + ABI_TENSOR + ABI_SCORE + ABI_RANK + ABI_OVERLAP + ABI_BATCHSTATS + ABI_COUNTSTATS + ABI_TYPICALITY + ABI_EXPLAIN + ABI_EXPLAIN_GROUPS + ABI_HOLDOUT + ABI_COUNTHOLDOUT + ABI_TRACE + ABI_MISSING + ABI_IMPUTE + ABI_REGRESS + ABI_REGRESS_DRAW + ABI_REGRESS_CDF + ABI_RECOMMEND + ABI_COUNT_EXPLAIN + ABI_CSC + ABI_SAMPLE + ABI_PROJECT:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.dpmm_abi_version() != ABI_VERSION:      # (dpmm_last_sweep_work fills 16 words since version 3: an older library would be handed too long a buffer, a newer one may overflow ours)
            raise ImportError(f"{p}: DPMM_ABI_VERSION {lib.dpmm_abi_version()}, this binding is written for {ABI_VERSION} (include/dpmm_hip.h)")
        _LIB = lib
    return _LIB


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


class Worker:
    """One shard of the points on one GPU: the stand-in for one reference worker process
    (the functions a worker runs on its `localpart`s, src/local_clusters_actions.jl)."""

    def __init__(self, prior, D, n_local, first_index=0, device=0, seed=0, timing=True):
        """timing: record HIP events around the sweep / statistics / all-reduces (last_kernel_ms, last_comm_ms).  On by default for
        this binding (tests, benches, scripts read them); the library's own default -- and what fit / dp_parallel use -- is off:
        each event costs ~5 us between two kernels."""
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        self.prior, self.D, self.n, self.first_index, self.device = prior, int(D), int(n_local), int(first_index), device
        rc = self._lib.dpmm_create(ctypes.byref(self._h), prior, D, n_local, first_index, device, ctypes.c_uint64(seed))
        if rc != 0:
            raise DpmmError(rc, self._lib.dpmm_last_error(None).decode())
        self.K = 0
        self.packed_stride = int(self._lib.dpmm_packed_stride(self._h))
        self.timing = bool(timing)
        if timing:
            self._chk(self._lib.dpmm_set_option(self._h, OPT_KERNEL_TIMING, 7.0))

    def _chk(self, rc):
        if rc != 0:
            err = DpmmError(rc, self._lib.dpmm_last_error(self._h).decode())
            cause = getattr(self, "_comm_error", None)          # an exception inside the host all-reduce callback (comm_init_host)
            if cause is not None:
                self._comm_error = None
                raise err from cause
            raise err

    @property
    def K(self):
        """Number of clusters the ctx currently knows (the native engine changes it through the C ABI directly)."""
        h = getattr(self, "_h", None)
        return int(self._lib.dpmm_num_clusters(h)) if h is not None and h.value else 0

    @K.setter
    def K(self, value):
        pass

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            try:
                early = self.debug_counters()[0]
            except Exception:
                early = 0
            if early:
                import sys
                print("dpmm worker: %d event wait(s) returned before the posterior records had reached host memory "
                      "(waited out; results unaffected)" % early, file=sys.stderr, flush=True)
            self._lib.dpmm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data
    def upload_points(self, X):
        """X: (n_local, ld) float32 C-contiguous, row i = point i (== Julia's D x n column-major)."""
        X = _f32(X)
        assert X.ndim == 2 and X.shape[0] == self.n and X.shape[1] >= self.D
        self._chk(self._lib.dpmm_upload_points(self._h, _p(X, _c_f32p), X.shape[1]))

    def upload_points_npy(self, rows, nan_to_zero=True):
        """rows: (n_local, >= D) array of a Samples x Dimensions .npy file (Float32 or Float64, C-contiguous; a
        read-only memory map is fine).  Float32 conversion and NaN -> 0 (utils.jl:9-13) happen on the device."""
        rows = np.asarray(rows)
        if rows.dtype not in (np.float32, np.float64):
            rows = rows.astype(np.float32)
        if not rows.flags.c_contiguous:
            rows = np.ascontiguousarray(rows)
        assert rows.ndim == 2 and rows.shape[0] == self.n and rows.shape[1] >= self.D
        self._chk(self._lib.dpmm_upload_points_npy(self._h, ctypes.c_void_p(rows.ctypes.data), int(rows.dtype == np.float64),
                                                   rows.shape[1], int(bool(nan_to_zero))))

    def upload_points_csc(self, colptr, rowval, nzval, index_base=0):
        """The shard as compressed sparse columns, one column per point (Multinomial): colptr (n_local + 1,), rowval / nzval the entries
        [colptr[i] - colptr[0], colptr[i+1] - colptr[0]) of point i; canonical (rows strictly increasing inside a column)."""
        colptr, rowval, nzval = _i64(colptr), _i64(rowval), _f32(nzval)
        assert colptr.ndim == 1 and colptr.size == self.n + 1 and rowval.size == nzval.size
        assert colptr.size == 0 or rowval.size >= colptr[-1] - colptr[0]
        self._chk(self._lib.dpmm_upload_points_csc(self._h, _p(colptr, _c_i64p), _p(rowval, _c_i64p), _p(nzval, _c_f32p), int(index_base)))

    def upload_points_device(self, ptr, ldx):
        self._chk(self._lib.dpmm_upload_points_device(self._h, ctypes.c_void_p(ptr), ldx))

    # ---- caller-owned device memory (include/dpmm_hip_tensor.h); pointers are plain integers (tensor.data_ptr())
    def upload_points_strided_device(self, ptr, dtype, stride_point, stride_feature, nan_to_zero=False):
        """Element (point i, feature d) at ptr + (i * stride_point + d * stride_feature) elements of the DT_* type `dtype`, device memory."""
        self._chk(self._lib.dpmm_upload_points_strided_device(self._h, ctypes.c_void_p(ptr), int(dtype), int(stride_point), int(stride_feature),
                                                              int(bool(nan_to_zero))))

    def upload_points_tensor(self, desc, lo, hi):
        """The points [lo, hi) of a device tensor described by host/tensors.py: no copy, no slicing on the host -- the shard starts
        lo * stride_point elements into the tensor's storage."""
        assert hi - lo == self.n and desc.D == self.D
        self.results_device = desc.torch_device            # labels and predictions follow the input (get_labels_tensor, _predict_points)
        self.upload_points_strided_device(desc.shard_ptr(lo), desc.dtype, desc.stride_point, desc.stride_feature, False)

    # ---- sparse points in caller-owned device memory (include/dpmm_hip_csc.h)
    def upload_points_csc_device(self, colptr_ptr, index_dtype, rowval_ptr, nzval_ptr, value_dtype, nnz_extent, index_base=0):
        """The shard as compressed sparse columns in device memory: colptr_ptr addresses the shard's first of n + 1 offsets (DT_I32 or
        DT_I64, as rowval), ABSOLUTE into rowval / nzval (`nnz_extent` entries of the DT_* type `value_dtype` behind nzval_ptr)."""
        self._chk(self._lib.dpmm_upload_points_csc_device(self._h, ctypes.c_void_p(colptr_ptr or None), int(index_dtype), ctypes.c_void_p(rowval_ptr or None),
                                                          ctypes.c_void_p(nzval_ptr or None), int(value_dtype), int(nnz_extent), int(index_base)))

    def upload_points_csc_tensor(self, desc, lo, hi):
        """The columns [lo, hi) of a sparse_csc tensor in device memory described by host/sparse.py (DeviceCSC): its offsets from `lo` on,
        the same two entry arrays -- no copy and no slicing on the host."""
        assert hi - lo == self.n and desc.D == self.D
        self.results_device = desc.torch_device            # labels and predictions follow the input, as for a dense tensor
        self.upload_points_csc_device(desc.colptr_ptr(lo), desc.index_dtype, desc.rowval_ptr, desc.nzval_ptr, desc.value_dtype, desc.nnz_extent, 0)

    # ---- projection (include/dpmm_hip_project.h): points wider than D, projected while they are read
    def set_projection(self, W, mu=None):
        """W: (D_in, D) Float64, mu: (D_in,) or None.  Afterwards the projected uploads read D_in-wide points: y = (x - mu)' W."""
        W = np.ascontiguousarray(W, dtype=np.float64)
        assert W.ndim == 2 and W.shape[1] == self.D
        mu = None if mu is None else np.ascontiguousarray(mu, dtype=np.float64)
        assert mu is None or mu.shape == (W.shape[0],)
        self._chk(self._lib.dpmm_set_projection(self._h, int(W.shape[0]), _p(W, _c_f64p_in), _p(mu, _c_f64p_in)))
        self.D_in = int(W.shape[0])

    def clear_projection(self):
        self._chk(self._lib.dpmm_set_projection(self._h, 0, None, None))
        self.D_in = 0

    def upload_points_projected(self, X):
        """X: (n_local, ld >= D_in) float32 C-contiguous host rows, row i = point i."""
        X = _f32(X)
        assert X.ndim == 2 and X.shape[0] == self.n
        self._chk(self._lib.dpmm_upload_points_projected(self._h, _p(X, _c_f32p), X.shape[1]))

    def upload_points_projected_strided_device(self, ptr, dtype, stride_point, stride_feature):
        self._chk(self._lib.dpmm_upload_points_projected_device(self._h, ctypes.c_void_p(ptr), int(dtype), int(stride_point), int(stride_feature)))

    def upload_points_projected_tensor(self, desc, lo, hi):
        """The points [lo, hi) of a D_in-wide device tensor described by host/tensors.py, projected on the way in."""
        assert hi - lo == self.n and desc.D == getattr(self, "D_in", 0)
        self.results_device = desc.torch_device
        self.upload_points_projected_strided_device(desc.shard_ptr(lo), desc.dtype, desc.stride_point, desc.stride_feature)

    def get_points_device(self, ptr, ld_out):
        self._chk(self._lib.dpmm_get_points_device(self._h, ctypes.c_void_p(ptr), int(ld_out)))

    def get_labels_device(self, labels_ptr, sub_ptr):
        self._chk(self._lib.dpmm_get_labels_device(self._h, ctypes.c_void_p(labels_ptr or None), ctypes.c_void_p(sub_ptr or None)))

    def set_labels_device(self, labels_ptr, sub_ptr):
        self._chk(self._lib.dpmm_set_labels_device(self._h, ctypes.c_void_p(labels_ptr or None), ctypes.c_void_p(sub_ptr or None)))

    def predict_points_device(self, labels_ptr, probs_ptr):
        self._chk(self._lib.dpmm_predict_points_device(self._h, ctypes.c_void_p(labels_ptr), ctypes.c_void_p(probs_ptr or None)))

    def get_labels_tensor(self, device):
        """(labels, sub_labels) as int64 tensors on `device` (this worker's GPU), written there by the library."""
        import torch
        lab = torch.empty(self.n, dtype=torch.int64, device=device); sub = torch.empty(self.n, dtype=torch.int64, device=device)
        torch.cuda.current_stream(device).synchronize()
        self.get_labels_device(lab.data_ptr(), sub.data_ptr())
        return lab, sub

    def init_labels(self, init_clusters, epoch):
        self._chk(self._lib.dpmm_init_labels(self._h, init_clusters, epoch))

    def set_labels(self, labels=None, sub=None):
        labels = _i64(labels) if labels is not None else None
        sub = _i64(sub) if sub is not None else None
        self._chk(self._lib.dpmm_set_labels(self._h, _p(labels, _c_i64p), _p(sub, _c_i64p)))

    def get_labels(self):
        lab = np.empty(self.n, np.int64); sub = np.empty(self.n, np.int64)
        self._chk(self._lib.dpmm_get_labels(self._h, _p(lab, _c_i64p), _p(sub, _c_i64p)))
        return lab, sub

    # ---- parameters
    def set_params_niw(self, mu, inv_sigma, logdet, lr_weights, weights):
        K = len(weights)
        mu, inv_sigma, logdet, lr_weights, weights = map(_f32, (mu, inv_sigma, logdet, lr_weights, weights))
        assert mu.shape == (3 * K, self.D) and inv_sigma.size == 3 * K * self.D * self.D and logdet.shape == (3 * K,) and lr_weights.shape == (K, 2)
        self._chk(self._lib.dpmm_set_params_niw(self._h, K, _p(mu, _c_f32p), _p(inv_sigma, _c_f32p), _p(logdet, _c_f32p), _p(lr_weights, _c_f32p), _p(weights, _c_f32p)))
        self.K = K

    def set_params_niw_chol(self, mu, R, logdet, lr_weights, weights):
        K = len(weights)
        mu, R, logdet, lr_weights, weights = map(_f32, (mu, R, logdet, lr_weights, weights))
        assert mu.shape == (3 * K, self.D) and R.size == 3 * K * self.D * self.D and logdet.shape == (3 * K,) and lr_weights.shape == (K, 2)
        self._chk(self._lib.dpmm_set_params_niw_chol(self._h, K, _p(mu, _c_f32p), _p(R, _c_f32p), _p(logdet, _c_f32p), _p(lr_weights, _c_f32p), _p(weights, _c_f32p)))
        self.K = K

    def set_params_mult(self, logp, lr_weights, weights):
        K = len(weights)
        logp, lr_weights, weights = map(_f32, (logp, lr_weights, weights))
        assert logp.shape == (3 * K, self.D) and lr_weights.shape == (K, 2)
        self._chk(self._lib.dpmm_set_params_mult(self._h, K, _p(logp, _c_f32p), _p(lr_weights, _c_f32p), _p(weights, _c_f32p)))
        self.K = K

    def set_num_clusters(self, K):
        self._chk(self._lib.dpmm_set_num_clusters(self._h, int(K)))
        self.K = int(K)

    # ---- the hot path
    def sweep(self, epoch, final=False):
        self._chk(self._lib.dpmm_sweep(self._h, epoch, int(bool(final))))

    def suffstats_packed(self, cluster_idx=None):
        out = np.empty((2 * self.K, self.packed_stride), np.float64)
        idx = _i64(cluster_idx) if cluster_idx is not None else None
        self._chk(self._lib.dpmm_suffstats_packed(self._h, _p(idx, _c_i64p), 0 if idx is None else len(idx), _p(out, _c_f64p)))
        return out

    def suffstats_packed_device(self, dev_ptr, cluster_idx=None):
        idx = _i64(cluster_idx) if cluster_idx is not None else None
        self._chk(self._lib.dpmm_suffstats_packed_device(self._h, _p(idx, _c_i64p), 0 if idx is None else len(idx), ctypes.c_void_p(dev_ptr)))

    def unpack(self, packed, K=None):
        K = self.K if K is None else K
        packed = np.ascontiguousarray(packed, np.float64)
        N = np.empty((K, 3)); s = np.empty((K, 3, self.D))
        S = np.empty((K, 3, self.D, self.D)) if self.prior == PRIOR_NIW else None
        self._chk(self._lib.dpmm_unpack_suffstats(self._h, K, _p(packed, _c_f64p), _p(N, _c_f64p), _p(s, _c_f64p), _p(S, _c_f64p)))
        return (N, s, S) if S is not None else (N, s)

    def suffstats(self, cluster_idx=None):
        return self.unpack(self.suffstats_packed(cluster_idx))

    # ---- relabel
    def split(self, idx, new_idx, epoch):
        idx, new_idx = _i64(idx), _i64(new_idx)
        self._chk(self._lib.dpmm_split(self._h, _p(idx, _c_i64p), _p(new_idx, _c_i64p), len(idx), epoch))

    def merge(self, idx, new_idx):
        idx, new_idx = _i64(idx), _i64(new_idx)
        self._chk(self._lib.dpmm_merge(self._h, _p(idx, _c_i64p), _p(new_idx, _c_i64p), len(idx)))

    def remove_empty(self, pts_count):
        pc = _i64(pts_count)
        self._chk(self._lib.dpmm_remove_empty(self._h, _p(pc, _c_i64p), len(pc)))

    def reset_sublabels(self, idx, epoch):
        if idx is None:
            self._chk(self._lib.dpmm_reset_sublabels(self._h, None, 0, epoch))
        else:
            idx = _i64(idx)
            self._chk(self._lib.dpmm_reset_sublabels(self._h, _p(idx, _c_i64p), len(idx), epoch))

    # ---- prediction (posterior predictive table)
    def predict_table_niw(self, m, R, logdet, df, weights, points=False):
        self.set_predictive_niw(m, R, logdet, df, weights)
        return self._predict_table(len(weights), points)

    def predict_table_mult(self, logp, weights, points=False):
        self.set_predictive_mult(logp, weights)
        return self._predict_table(len(weights), points)

    def _predict_table(self, K, points):
        self.K = K
        if points:
            return self._predict_points(K)
        out = np.empty((K, self.n), np.float32)
        self._chk(self._lib.dpmm_predict(self._h, _p(out, _c_f32p)))
        return out

    supports_predict_points = True

    def _predict_points(self, K):
        dev = getattr(self, "results_device", None)
        if dev is not None:                  # the points came from a device tensor: the (n, K) table stays on that device
            import torch
            lab = torch.empty(self.n, dtype=torch.int64, device=dev); probs = torch.empty((self.n, K), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            self.predict_points_device(lab.data_ptr(), probs.data_ptr())
            return lab, probs
        lab = np.empty(self.n, np.int64); probs = np.empty((self.n, K), np.float32)
        self._chk(self._lib.dpmm_predict_points(self._h, _p(lab, _c_i64p), _p(probs, _c_f32p)))
        return lab, probs

    # ---- scoring (include/dpmm_hip_score.h)
    def set_predictive_niw(self, m, R, logdet, df, weights):
        """dpmm_set_predictive_niw alone: the parameters stay in force for every later predict / score call."""
        K = len(weights)
        m, R, logdet, df, weights = map(_f32, (m, R, logdet, df, weights))
        assert m.shape == (K, self.D) and R.size == K * self.D * self.D
        self._chk(self._lib.dpmm_set_predictive_niw(self._h, K, _p(m, _c_f32p), _p(R, _c_f32p), _p(logdet, _c_f32p), _p(df, _c_f32p), _p(weights, _c_f32p)))

    def set_predictive_mult(self, logp, weights):
        K = len(weights)
        logp, weights = _f32(logp), _f32(weights)
        assert logp.shape == (K, self.D)
        self._chk(self._lib.dpmm_set_predictive_mult(self._h, K, _p(logp, _c_f32p), _p(weights, _c_f32p)))

    # ---- drawing points (include/dpmm_hip_sample.h)
    def set_sampler_niw(self, m, A, df):
        """dpmm_set_sampler_niw: m (K, D), A (K, D, D) upper triangular, df (K,)."""
        m, A, df = map(_f32, (m, A, df))
        K = len(df)
        assert m.shape == (K, self.D) and A.size == K * self.D * self.D
        self._chk(self._lib.dpmm_set_sampler_niw(self._h, K, _p(m, _c_f32p), _p(A, _c_f32p), _p(df, _c_f32p)))

    def set_sampler_mult(self, thr, alias):
        """dpmm_set_sampler_mult: the alias tables, thr (K, D) uint32 and alias (K, D) int32."""
        thr, alias = np.ascontiguousarray(thr, np.uint32), np.ascontiguousarray(alias, np.int32)
        assert thr.ndim == 2 and thr.shape == alias.shape and thr.shape[1] == self.D
        self._chk(self._lib.dpmm_set_sampler_mult(self._h, thr.shape[0], _p(thr, ctypes.POINTER(ctypes.c_uint32)), _p(alias, ctypes.POINTER(ctypes.c_int32))))

    def sample_points_raw(self, i0, n, cluster_start, seed, trials=0, x=0, ld=0, labels=0, colptr=0, nnz0=0, rowval=0, nzval=0, nnz_extent=0):
        """dpmm_sample_points_device on plain device addresses (integers; 0 = not asked for); returns the entries counted by a sparse
        first call, else None."""
        cs = _i64(cluster_start)
        nnz = ctypes.c_int64(0)
        first = bool(colptr) and not (rowval or nzval)
        req = SampleRequest(int(i0), int(n), _p(cs, _c_i64p), ctypes.c_uint64(int(seed)), int(trials), x or None, int(ld), labels or None, colptr or None,
                            int(nnz0), rowval or None, nzval or None, int(nnz_extent), ctypes.pointer(nnz) if first else None)
        self._chk(self._lib.dpmm_sample_points_device(self._h, ctypes.byref(req)))
        return int(nnz.value) if first else None

    # ---- the point calls (`*_into`): one marshaller for the storage their callers make
    def _marshal(self, call, arrays):
        """What every `*_into` method does with its arrays.  call: the C entry's base name; arrays: (name, array or None, dtype name,
        per_point) each -- numpy arrays (host variant) or torch tensors on this worker's GPU (device variant), never both, C-contiguous, of
        that dtype and, if per_point, with n as the leading extent.  Synchronises the tensors' current stream once.  Returns (fn, ptr, dev):
        `call` or `call_device`, ptr[name] the address of every array listed -- None for None and for an empty one: every entry returns at
        n_local == 0 before it reads through a pointer (csrc/dpmm_api.cpp), and with points a null it needs is its own DPMM_EINVAL -- and
        whether it is the device variant."""
        dev, first, ptr = False, None, {}
        for name, a, dt, per in arrays:             # (one pass: this runs once per slab of every served batch)
            ptr[name] = None
            if a is None:
                continue
            tensor = hasattr(a, "data_ptr")
            if first is None:
                dev, first = tensor, a
            assert tensor == dev, call + ": numpy arrays or tensors, not both"
            if dev:
                import torch
                assert a.is_contiguous() and a.dtype == getattr(torch, dt) and (not per or a.shape[0] == self.n), name
                if a.numel():
                    ptr[name] = a.data_ptr()
            else:
                assert a.flags.c_contiguous and a.dtype == dt and (not per or a.shape[0] == self.n), name
                if a.size:
                    ptr[name] = a.ctypes.data
        if dev:
            torch.cuda.current_stream(first.device).synchronize()
        return getattr(self._lib, call + ("_device" if dev else "")), ptr, dev

    _SCORE_OUTS = dict(labels="int64", logdens="float32", top_idx="int64", top_prob="float32", probs="float32")
    _EXPLAIN_OUTS = dict(labels="int64", mahalanobis="float32", tail="float32", residual="float32", zscore="float32", feature_tail="float32",
                         features="int32")

    def score_points_raw(self, device, labels=0, logdens=0, m=0, top_idx=0, top_prob=0, probs=0):
        """dpmm_score_points[_device] on plain addresses (integers; 0 = not asked for)."""
        out = ScoreOut(labels or None, logdens or None, int(m), top_idx or None, top_prob or None, probs or None)
        fn = self._lib.dpmm_score_points_device if device else self._lib.dpmm_score_points
        self._chk(fn(self._h, ctypes.byref(out)))

    def score_points_into(self, outs, m=0):
        """dpmm_score_points[_device] into storage the caller made: `outs` maps `labels` / `logdens` / `top_idx` / `top_prob` / `probs` to
        contiguous numpy arrays (host variant) or torch tensors on this worker's GPU (device variant) with n rows each."""
        _, ptr, dev = self._marshal("dpmm_score_points", [(name, a, self._SCORE_OUTS[name], True) for name, a in outs.items()])
        self.score_points_raw(dev, m=int(m), **ptr)

    def score_points(self, labels=False, logdens=False, m=0, top_idx=None, top_prob=None, probs=False, device=None):
        """The outputs asked for, of the ctx's n points: a dict with `labels` (n,) int64, `logdens` (n,) float32, `top_idx` (n, m) int64,
        `top_prob` (n, m) float32, `probs` (n, K) float32.  m > 0 asks for both top_* unless one is switched off with False.
        device: a torch device -- the results are tensors there, written by the library; None: numpy arrays."""
        n, K, m = self.n, self.K, int(m)
        spec = [("labels", labels, (n,), "int64"), ("logdens", logdens, (n,), "float32"), ("top_idx", m > 0 and top_idx is not False, (n, m), "int64"),
                ("top_prob", m > 0 and top_prob is not False, (n, m), "float32"), ("probs", probs, (n, K), "float32")]
        if device is not None:
            import torch
            res = {name: torch.empty(shape, dtype=getattr(torch, dt), device=device) for name, want, shape, dt in spec if want}
        else:
            res = {name: np.empty(shape, dt) for name, want, shape, dt in spec if want}
        if not res:
            raise ValueError("score_points: no output asked for")
        if n > 0:
            self.score_points_into(res, m=m)
        return res

    # ---- calibrated outlier scores (include/dpmm_hip_typicality.h)
    def typicality_points_raw(self, device, labels=0, mahalanobis=0, tail=0, skipped=0, incomplete=0):
        """dpmm_typicality_points[_device] on plain addresses (integers; 0 = not asked for); skipped, incomplete: host addresses."""
        out = TypicalityOut(labels or None, mahalanobis or None, tail or None, skipped or None, incomplete or None)
        fn = self._lib.dpmm_typicality_points_device if device else self._lib.dpmm_typicality_points
        self._chk(fn(self._h, ctypes.byref(out)))

    def typicality_points_into(self, outs):
        """dpmm_typicality_points[_device] into storage the caller made: `outs` maps `labels` / `mahalanobis` / `tail` to contiguous numpy
        arrays (host variant) or torch tensors on this worker's GPU (device variant) with n entries each; returns (skipped, incomplete)."""
        _, ptr, dev = self._marshal("dpmm_typicality_points", [(name, a, self._EXPLAIN_OUTS[name], True) for name, a in outs.items()])
        cnt = np.zeros(2, np.int64)
        self.typicality_points_raw(dev, skipped=cnt.ctypes.data, incomplete=cnt.ctypes.data + 8, **ptr)
        return int(cnt[0]), int(cnt[1])

    # ---- per-feature explanations (include/dpmm_hip_explain.h)
    def explain_points_raw(self, device, top=0, ld=0, labels=0, mahalanobis=0, tail=0, skipped=0, incomplete=0, residual=0, zscore=0, feature_tail=0,
                           features=0):
        """dpmm_explain_points[_device] on plain addresses (integers; 0 = not asked for); skipped, incomplete: host addresses."""
        out = ExplainOut(labels or None, mahalanobis or None, tail or None, skipped or None, incomplete or None, residual or None, zscore or None,
                         feature_tail or None, features or None, int(top), int(ld))
        fn = self._lib.dpmm_explain_points_device if device else self._lib.dpmm_explain_points
        self._chk(fn(self._h, ctypes.byref(out)))

    def explain_points_into(self, outs, top=0):
        """dpmm_explain_points[_device] into storage the caller made: `outs` maps `labels` / `mahalanobis` / `tail` (n entries each) and
        `residual` / `zscore` / `feature_tail` / `features` ((n, ld) each, one ld for all, features int32 and only with top > 0) to contiguous
        numpy arrays (host variant) or torch tensors on this worker's GPU (device variant); returns (skipped, incomplete)."""
        ld = 0
        for name in ("residual", "zscore", "feature_tail", "features"):
            if name in outs:
                assert len(outs[name].shape) == 2 and ld in (0, outs[name].shape[1]), name
                ld = int(outs[name].shape[1])
        _, ptr, dev = self._marshal("dpmm_explain_points", [(name, a, self._EXPLAIN_OUTS[name], True) for name, a in outs.items()])
        cnt = np.zeros(2, np.int64)
        self.explain_points_raw(dev, top=top, ld=ld, skipped=cnt.ctypes.data, incomplete=cnt.ctypes.data + 8, **ptr)
        return int(cnt[0]), int(cnt[1])

    # ---- explanations by groups of features (include/dpmm_hip_explain_groups.h)
    _EXPLAIN_GROUPS_OUTS = dict(labels="int64", mahalanobis="float32", tail="float32", group_mahalanobis="float32", group_tail="float32")

    def set_explain_groups(self, groups, W):
        """dpmm_set_explain_groups: `groups`, a sequence of sequences of 0-based feature indices (increasing inside a group), and W, the
        Float64 rows of the lower triangles of the factors L^-1 packed per cluster and group as the header says (what
        host/condition.py's `group_factors` returns), for the predictive parameters in force."""
        sizes = [len(g) for g in groups]
        offsets = _i64(np.concatenate([[0], np.cumsum(sizes)]))
        features = np.ascontiguousarray(np.concatenate([np.asarray(g, np.int64).ravel() for g in groups]) if sizes else np.zeros(0), np.int32)
        W = np.ascontiguousarray(W, np.float64).ravel()
        assert W.size == self.K * sum(s * (s + 1) // 2 for s in sizes), "set_explain_groups: W holds K sum s (s + 1) / 2 values"
        self._chk(self._lib.dpmm_set_explain_groups(self._h, len(sizes), _p(offsets, _c_i64p), _p(features, ctypes.POINTER(ctypes.c_int32)), _p(W, _c_f64p)))

    def explain_groups_points_raw(self, device, ld=0, labels=0, mahalanobis=0, tail=0, skipped=0, incomplete=0, group_mahalanobis=0, group_tail=0):
        """dpmm_explain_groups_points[_device] on plain addresses (integers; 0 = not asked for); skipped, incomplete: host addresses."""
        out = ExplainGroupsOut(labels or None, mahalanobis or None, tail or None, skipped or None, incomplete or None, group_mahalanobis or None,
                               group_tail or None, int(ld))
        fn = self._lib.dpmm_explain_groups_points_device if device else self._lib.dpmm_explain_groups_points
        self._chk(fn(self._h, ctypes.byref(out)))

    def explain_groups_points_into(self, outs):
        """dpmm_explain_groups_points[_device] into storage the caller made: `outs` maps `labels` / `mahalanobis` / `tail` (n entries each)
        and `group_mahalanobis` / `group_tail` ((n, ld >= G) each, one ld for both) to contiguous numpy arrays (host variant) or torch
        tensors on this worker's GPU (device variant); returns (skipped, incomplete)."""
        ld = 0
        for name in ("group_mahalanobis", "group_tail"):
            if name in outs:
                assert len(outs[name].shape) == 2 and ld in (0, outs[name].shape[1]), name
                ld = int(outs[name].shape[1])
        _, ptr, dev = self._marshal("dpmm_explain_groups_points", [(name, a, self._EXPLAIN_GROUPS_OUTS[name], True) for name, a in outs.items()])
        cnt = np.zeros(2, np.int64)
        self.explain_groups_points_raw(dev, ld=ld, skipped=cnt.ctypes.data, incomplete=cnt.ctypes.data + 8, **ptr)
        return int(cnt[0]), int(cnt[1])

    # ---- missing features (include/dpmm_hip_missing.h)
    def score_missing_counts(self):
        """dpmm_score_missing_counts: (marginalised, over the cap) among the points the last score / rank / impute call evaluated."""
        out = np.zeros(2, np.int64)
        self._chk(self._lib.dpmm_score_missing_counts(self._h, _p(out, _c_i64p)))
        return int(out[0]), int(out[1])

    def impute_points_into(self, out):
        """dpmm_impute_points[_device] into storage the caller made: a C-contiguous (n, ld >= D) float32 numpy array (host variant) or
        torch tensor on this worker's GPU (device variant)."""
        assert len(out.shape) == 2 and out.shape[1] >= self.D
        fn, p, _ = self._marshal("dpmm_impute_points", [("out", out, "float32", True)])
        self._chk(fn(self._h, ctypes.cast(p["out"], fn.argtypes[1]), int(out.shape[1])))

    # ---- draws of the missing features (include/dpmm_hip_impute.h)
    def impute_draws_into(self, out, seed, i0, draw0=0, comp=None):
        """dpmm_impute_draw_points[_device] into storage the caller made: out (n, ndraws, w >= D) float32, C-contiguous -- the draws of a
        point side by side: ld = ndraws * w, draw_stride = w -- a numpy array (host variant) or a torch tensor on this worker's GPU (device
        variant); the draws are draw0 .. draw0 + ndraws - 1 of the points with global indices i0 .. i0 + n - 1.  comp: None or an
        (ndraws, n) int32 array / tensor of the same kind for the drawn clusters (0-based, -1 off the marginalised points)."""
        nd, w = int(out.shape[1]), int(out.shape[2])
        assert nd >= 1 and w >= self.D and (comp is None or tuple(comp.shape) == (nd, self.n))
        fn, p, _ = self._marshal("dpmm_impute_draw_points", [("out", out, "float32", True), ("comp", comp, "int32", False)])
        dest = ctypes.cast(p["out"], fn.argtypes[1])
        self._chk(fn(self._h, dest, nd * w, w, p["comp"], ctypes.c_uint64(int(seed)), int(i0), int(draw0), nd))

    # ---- mixture regression (include/dpmm_hip_regress.h)
    def set_regression(self, B, c, V, h):
        """dpmm_set_regression: the tables B (K, D_t, D), c (K, D_t), V (K, D_t), h (K,) in Float64 for the predictive parameters in force."""
        B, c, V, h = (np.ascontiguousarray(a, np.float64) for a in (B, c, V, h))
        K, Dt = c.shape
        assert B.shape == (K, Dt, self.D) and V.shape == (K, Dt) and h.shape == (K,)
        self._chk(self._lib.dpmm_set_regression(self._h, int(Dt), _p(B, _c_f64p), _p(c, _c_f64p), _p(V, _c_f64p), _p(h, _c_f64p)))
        self._regress_Dt = int(Dt)

    def regress_points_into(self, mean, std=None, labels=None):
        """dpmm_regress_points[_device] into storage the caller made: mean and std C-contiguous (n, ld >= D_t) float32, labels (n,) int64
        -- numpy arrays (host variant) or torch tensors on this worker's GPU (device variant); std and labels may be None.  Returns the
        number of points that took no part."""
        assert std is None or tuple(std.shape) == tuple(mean.shape)
        fn, p, _ = self._marshal("dpmm_regress_points",
                                 [("mean", mean, "float32", True), ("std", std, "float32", True), ("labels", labels, "int64", True)])
        skipped = np.zeros(1, np.int64)
        self._chk(fn(self._h, p["mean"], p["std"], int(mean.shape[1]), p["labels"], _p(skipped, _c_i64p)))
        return int(skipped[0])

    # ---- next-count probabilities (include/dpmm_hip_recommend.h)
    def set_recommend(self, theta):
        """dpmm_set_recommend: theta (K, D) in Float64, the clusters' next-count probabilities, for the predictive parameters in force."""
        theta = np.ascontiguousarray(theta, np.float64)
        assert theta.shape == (self.K, self.D), "set_recommend: theta (K, D)"
        self._chk(self._lib.dpmm_set_recommend(self._h, _p(theta, _c_f64p)))

    def recommend_points_into(self, views, m, exclude_seen=True):
        """dpmm_recommend_points[_device] into storage the caller made: `views` maps `features` (n, ld >= m) int32, `prob` (n, ld) float32
        and, if asked for, `labels` (n,) int64 to C-contiguous numpy arrays (host variant) or torch tensors on this worker's GPU (device
        variant).  Returns the number of points that took no part."""
        features, prob, labels = views["features"], views["prob"], views.get("labels")
        assert len(features.shape) == 2 and tuple(prob.shape) == tuple(features.shape)
        fn, p, _ = self._marshal("dpmm_recommend_points",
                                 [("features", features, "int32", True), ("prob", prob, "float32", True), ("labels", labels, "int64", True)])
        skipped = np.zeros(1, np.int64)
        self._chk(fn(self._h, int(m), 1 if exclude_seen else 0, p["features"], p["prob"], int(features.shape[1]), p["labels"],
                     _p(skipped, _c_i64p)))
        return int(skipped[0])

    # ---- the features that put a count point out (include/dpmm_hip_count_explain.h)
    def set_count_explain(self, log_theta, log1m_theta, order):
        """dpmm_set_count_explain: log theta and log1p(-theta), (K, D) Float64 each, and order (K, D) int32, every cluster's features with
        log1p(-theta) non-decreasing, ties to the lower index -- for the predictive parameters in force."""
        lth, l1m = np.ascontiguousarray(log_theta, np.float64), np.ascontiguousarray(log1m_theta, np.float64)
        order = np.ascontiguousarray(order, np.int32)
        assert lth.shape == l1m.shape == order.shape == (self.K, self.D), "set_count_explain: three (K, D) tables"
        self._chk(self._lib.dpmm_set_count_explain(self._h, _p(lth, _c_f64p), _p(l1m, _c_f64p), _p(order, ctypes.POINTER(ctypes.c_int32))))

    _COUNT_EXPLAIN_OUTS = dict(features="int32", count="float32", expected="float32", residual="float32", feature_tail="float32", labels="int64",
                               total="float64")

    def count_explain_points_into(self, views, top, side="both"):
        """dpmm_count_explain_points[_device] into storage the caller made: `views` maps `features` (n, ld >= top) int32 and `count`,
        `expected`, `residual`, `feature_tail` (n, ld) float32 -- one ld for the five -- and, if asked for, `labels` (n,) int64 and `total`
        (n,) float64 to C-contiguous numpy arrays (host variant) or torch tensors on this worker's GPU (device variant).  Returns
        (skipped, incomplete)."""
        ld = int(views["features"].shape[1])
        for name in ("features", "count", "expected", "residual", "feature_tail"):
            assert len(views[name].shape) == 2 and int(views[name].shape[1]) == ld, name
        fn, p, _ = self._marshal("dpmm_count_explain_points", [(name, views.get(name), dt, True) for name, dt in self._COUNT_EXPLAIN_OUTS.items()])
        cnt = np.zeros(2, np.int64)
        out = CountExplainOut(int(top), COUNT_EXPLAIN_SIDES[side], ld, p["features"], p["count"], p["expected"], p["residual"], p["feature_tail"], p["labels"],
                              p["total"], cnt.ctypes.data, cnt.ctypes.data + 8)
        self._chk(fn(self._h, ctypes.byref(out)))
        return int(cnt[0]), int(cnt[1])

    # ---- draws of the targets (include/dpmm_hip_regress_draw.h)
    def set_regression_factor(self, W):
        """dpmm_set_regression_factor: W (K, D_t, D_t) Float64, upper triangular with W W' = (A_MM)^-1, for the tables of set_regression
        in force."""
        W = np.ascontiguousarray(W, np.float64)
        Dt = getattr(self, "_regress_Dt", None)
        assert Dt is not None and W.shape == (self.K, Dt, Dt), "set_regression_factor: set_regression first, W (K, D_t, D_t)"
        self._chk(self._lib.dpmm_set_regression_factor(self._h, _p(W, _c_f64p)))

    def regress_draw_points_into(self, out, seed, i0, draw0=0, comp=None):
        """dpmm_regress_draw_points[_device] into storage the caller made: out (n, ndraws, w >= D_t) float32, C-contiguous -- the draws of
        a point side by side: ld = ndraws * w, draw_stride = w -- a numpy array (host variant) or a torch tensor on this worker's GPU (device
        variant); the draws are draw0 .. draw0 + ndraws - 1 of the points with global indices i0 .. i0 + n - 1.  comp: None or an
        (ndraws, n) int32 array / tensor of the same kind for the drawn clusters (0-based, -1: the point took no part).  Returns the number
        of points that took no part."""
        nd, w = int(out.shape[1]), int(out.shape[2])
        assert nd >= 1 and w >= self._regress_Dt and (comp is None or tuple(comp.shape) == (nd, self.n))
        fn, p, _ = self._marshal("dpmm_regress_draw_points", [("out", out, "float32", True), ("comp", comp, "int32", False)])
        skipped = np.zeros(1, np.int64)
        dest = ctypes.cast(p["out"], fn.argtypes[1])
        self._chk(fn(self._h, dest, nd * w, w, p["comp"], ctypes.c_uint64(int(seed)), int(i0), int(draw0), nd, _p(skipped, _c_i64p)))
        return int(skipped[0])

    # ---- conditional CDF and quantiles of the targets (include/dpmm_hip_regress_cdf.h)
    def regress_cdf_points_into(self, y, cdf, sf=None, labels=None):
        """dpmm_regress_cdf_points[_device] into storage the caller made: y, cdf and sf C-contiguous (n, ld >= D_t) float32, labels (n,) int64
        -- numpy arrays (host variant) or torch tensors on this worker's GPU (device variant); sf and labels may be None.  Returns the
        number of points that took no part."""
        assert sf is None or tuple(sf.shape) == tuple(cdf.shape)
        fn, p, _ = self._marshal("dpmm_regress_cdf_points", [("y", y, "float32", True), ("cdf", cdf, "float32", True), ("sf", sf, "float32", True),
                                                             ("labels", labels, "int64", True)])
        skipped = np.zeros(1, np.int64)
        self._chk(fn(self._h, p["y"], int(y.shape[1]), p["cdf"], p["sf"], int(cdf.shape[1]), p["labels"], _p(skipped, _c_i64p)))
        return int(skipped[0])

    def set_regression_levels(self, levels, z):
        """dpmm_set_regression_levels: L strictly increasing levels inside (0, 1) and z (K, L) Float64, z[k, q] the level's quantile of
        t_{df_k + D}, for the tables of set_regression in force."""
        levels, z = np.ascontiguousarray(levels, np.float64), np.ascontiguousarray(z, np.float64)
        assert levels.ndim == 1 and z.shape == (self.K, len(levels)), "set_regression_levels: levels (L,), z (K, L)"
        self._chk(self._lib.dpmm_set_regression_levels(self._h, len(levels), _p(levels, _c_f64p), _p(z, _c_f64p)))
        self._regress_L = len(levels)

    def regress_quantile_points_into(self, out, labels=None):
        """dpmm_regress_quantile_points[_device] into storage the caller made: out (n, L, ld >= D_t) float32 C-contiguous, labels (n,) int64
        or None -- numpy arrays or torch tensors on this worker's GPU.  Returns the number of points that took no part."""
        assert int(out.shape[1]) == self._regress_L
        fn, p, _ = self._marshal("dpmm_regress_quantile_points", [("out", out, "float32", True), ("labels", labels, "int64", True)])
        skipped = np.zeros(1, np.int64)
        self._chk(fn(self._h, p["out"], int(out.shape[2]), p["labels"], _p(skipped, _c_i64p)))
        return int(skipped[0])

    # ---- exemplars (include/dpmm_hip_rank.h)
    def rank_begin(self, m, which=RANK_TYPICAL | RANK_FRINGE):
        """dpmm_rank_begin: a new ranking of width m over the lists in `which` (RANK_TYPICAL | RANK_FRINGE)."""
        self._chk(self._lib.dpmm_rank_begin(self._h, int(m), int(which)))
        self._rank_shape = (self.K, int(m))

    def rank_accumulate(self, index_base, n_valid):
        """dpmm_rank_accumulate: ranks the points 0..n_valid-1 of the current upload as global indices index_base + i."""
        self._chk(self._lib.dpmm_rank_accumulate(self._h, int(index_base), int(n_valid)))

    def rank_read_raw(self, device, typ_idx=0, typ_score=0, fringe_idx=0, fringe_score=0, count=0, skipped=0):
        """dpmm_rank_read[_device] on plain addresses (integers; 0 = not asked for)."""
        out = RankOut(typ_idx or None, typ_score or None, fringe_idx or None, fringe_score or None, count or None, skipped or None)
        fn = self._lib.dpmm_rank_read_device if device else self._lib.dpmm_rank_read
        self._chk(fn(self._h, ctypes.byref(out)))

    def rank_read(self, device=None):
        """The lists as they stand: a dict with `typ_idx`, `fringe_idx` (K, m) int64 (0-based global indices, -1 = unused slot),
        `typ_score`, `fringe_score` (K, m) float32 (NaN = unused slot), `count` (K,) int64 and `skipped` (1,) int64.
        device: a torch device -- the results are tensors there, written by the library; None: numpy arrays."""
        shape = getattr(self, "_rank_shape", None)
        if shape is None:
            self.rank_read_raw(False)          # (DPMM_ESTATE: no dpmm_rank_begin yet)
            raise RuntimeError("rank_read needs rank_begin first")
        K = shape[0]
        spec = [("typ_idx", shape, "int64"), ("typ_score", shape, "float32"), ("fringe_idx", shape, "int64"), ("fringe_score", shape, "float32"),
                ("count", (K,), "int64"), ("skipped", (1,), "int64")]
        if device is not None:
            import torch
            res = {name: torch.empty(sh, dtype=getattr(torch, dt), device=device) for name, sh, dt in spec}
            torch.cuda.current_stream(res["count"].device).synchronize()
            self.rank_read_raw(True, **{k: v.data_ptr() for k, v in res.items()})
        else:
            res = {name: np.empty(sh, dt) for name, sh, dt in spec}
            self.rank_read_raw(False, **{k: v.ctypes.data for k, v in res.items()})
        return res

    # ---- cluster overlap (include/dpmm_hip_overlap.h)
    def overlap_begin(self):
        """dpmm_overlap_begin: a new accumulation of the overlap matrix, the masses, count and skipped."""
        self._chk(self._lib.dpmm_overlap_begin(self._h))
        self._overlap_K = self.K

    def overlap_accumulate(self, n_valid):
        """dpmm_overlap_accumulate: adds the points 0..n_valid-1 of the current upload."""
        self._chk(self._lib.dpmm_overlap_accumulate(self._h, int(n_valid)))

    def overlap_read_raw(self, overlap=0, mass=0, count=0, skipped=0):
        """dpmm_overlap_read on plain host addresses (integers; 0 = not asked for)."""
        out = OverlapOut(overlap or None, mass or None, count or None, skipped or None)
        self._chk(self._lib.dpmm_overlap_read(self._h, ctypes.byref(out)))

    def overlap_read(self):
        """The sums as they stand: a dict of numpy arrays, `overlap` (K, K) float64 (symmetric bit for bit), `mass` (K,) float64,
        `count` (K,) int64 and `skipped` (1,) int64."""
        K = getattr(self, "_overlap_K", None)
        if K is None:
            self.overlap_read_raw()            # (DPMM_ESTATE: no dpmm_overlap_begin yet)
            raise RuntimeError("overlap_read needs overlap_begin first")
        res = dict(overlap=np.empty((K, K), np.float64), mass=np.empty(K, np.float64), count=np.empty(K, np.int64), skipped=np.empty(1, np.int64))
        self.overlap_read_raw(**{k: v.ctypes.data for k, v in res.items()})
        return res

    # ---- batch statistics (include/dpmm_hip_batchstats.h)
    def batchstats_begin(self, mode=BATCHSTATS_HARD, min_logdens=None):
        """dpmm_batchstats_begin: a new accumulation of N, sums, S and the counters with the weights of `mode`; min_logdens: None, or the
        floor below which a point is held out."""
        self._chk(self._lib.dpmm_batchstats_begin(self._h, int(mode), *_floor(min_logdens)))
        self._batchstats_K = self.K

    def batchstats_set_min_tail(self, min_tail=None):
        """dpmm_batchstats_set_min_tail (include/dpmm_hip_typicality.h), between batchstats_begin and the first batchstats_accumulate:
        min_tail in (0, 1], the tail below which a complete point is held out, or None for no such floor."""
        self._chk(self._lib.dpmm_batchstats_set_min_tail(self._h, *_floor(min_tail)))

    def batchstats_accumulate(self, n_valid):
        """dpmm_batchstats_accumulate: adds the points 0..n_valid-1 of the current upload."""
        self._chk(self._lib.dpmm_batchstats_accumulate(self._h, int(n_valid)))

    def batchstats_read_raw(self, N=0, sums=0, S=0, count=0, skipped=0, incomplete=0, held_out=0):
        """dpmm_batchstats_read on plain host addresses (integers; 0 = not asked for)."""
        out = BatchStatsOut(N or None, sums or None, S or None, count or None, skipped or None, incomplete or None, held_out or None)
        self._chk(self._lib.dpmm_batchstats_read(self._h, ctypes.byref(out)))

    def batchstats_read(self):
        """The sums as they stand: a dict of numpy arrays, `N` (K,), `sums` (K, D), `S` (K, D, D) float64 (S[k] symmetric bit for bit),
        `count` (K,) int64 and `skipped`, `incomplete`, `held_out` (1,) int64."""
        return self._stats_read("batchstats", dict(N=(), sums=(self.D,), S=(self.D, self.D)))

    def _stats_read(self, family, sums):
        """batchstats_read / countstats_read: `sums` names the family's float64 arrays and the shape of one cluster's part of each."""
        K = getattr(self, f"_{family}_K", None)
        raw = getattr(self, family + "_read_raw")
        if K is None:
            raw()                              # (DPMM_ESTATE: no dpmm_*_begin yet)
            raise RuntimeError(f"{family}_read needs {family}_begin first")
        res = {k: np.empty((K,) + per, np.float64) for k, per in sums.items()}
        res.update(count=np.empty(K, np.int64), skipped=np.empty(1, np.int64), incomplete=np.empty(1, np.int64), held_out=np.empty(1, np.int64))
        raw(**{k: v.ctypes.data for k, v in res.items()})
        return res

    # ---- held-out points (include/dpmm_hip_holdout.h)
    def holdout_begin(self, dst_points, dst_index, cap, min_logdens=None, min_tail=None):
        """dpmm_holdout_begin: a new collection of the points below the floor min_logdens and / or the tail floor min_tail (None: not in
        use) into dst_points [cap][D] float32 and dst_index [cap] int64 -- device addresses (integers) or torch tensors on this worker's
        GPU, which the caller keeps alive until holdout_read."""
        addr = [ctypes.c_void_p(a) for a in _device_addresses(dst_points, dst_index)]
        self._chk(self._lib.dpmm_holdout_begin(self._h, *_floor(min_logdens), *_floor(min_tail), addr[0], addr[1], int(cap)))

    def holdout_accumulate(self, lo, n_valid):
        """dpmm_holdout_accumulate: classifies the points 0..n_valid-1 of the current upload, global indices lo + i, and appends the
        held-out ones."""
        self._chk(self._lib.dpmm_holdout_accumulate(self._h, int(lo), int(n_valid)))

    def holdout_read(self):
        """The counters as they stand, after the stream has been waited for: a dict of ints `total`, `stored`, `skipped`, `incomplete`, `scored`."""
        cnt = np.zeros(5, np.int64)
        out = HoldoutOut(*[cnt[j:].ctypes.data for j in range(5)])
        self._chk(self._lib.dpmm_holdout_read(self._h, ctypes.byref(out)))
        return dict(zip(("total", "stored", "skipped", "incomplete", "scored"), (int(v) for v in cnt)))

    # ---- count statistics of the Multinomial prior (include/dpmm_hip_countstats.h)
    def countstats_begin(self, mode=BATCHSTATS_HARD, min_logdens=None):
        """dpmm_countstats_begin: a new accumulation of N, sums and the counters with the weights of `mode`; min_logdens: None, or the
        floor below which a point is held out."""
        self._chk(self._lib.dpmm_countstats_begin(self._h, int(mode), *_floor(min_logdens)))
        self._countstats_K = self.K

    def countstats_accumulate(self, n_valid):
        """dpmm_countstats_accumulate: adds the points 0..n_valid-1 of the current upload, whichever store they are in."""
        self._chk(self._lib.dpmm_countstats_accumulate(self._h, int(n_valid)))

    def countstats_read_raw(self, N=0, sums=0, count=0, skipped=0, incomplete=0, held_out=0):
        """dpmm_countstats_read on plain host addresses (integers; 0 = not asked for)."""
        out = CountStatsOut(N or None, sums or None, count or None, skipped or None, incomplete or None, held_out or None)
        self._chk(self._lib.dpmm_countstats_read(self._h, ctypes.byref(out)))

    def countstats_read(self):
        """The sums as they stand: a dict of numpy arrays, `N` (K,), `sums` (K, D) float64, `count` (K,) int64 and `skipped`,
        `incomplete`, `held_out` (1,) int64."""
        return self._stats_read("countstats", dict(N=(), sums=(self.D,)))

    # ---- the floor per count and the held-out points of count data (include/dpmm_hip_countholdout.h)
    def countstats_set_per_count(self, min_logdens_per_count):
        """dpmm_countstats_set_per_count: the accumulation just begun also holds out the complete points whose log-density per count lies
        below `min_logdens_per_count` (None: switched off); between countstats_begin and the first countstats_accumulate."""
        self._chk(self._lib.dpmm_countstats_set_per_count(self._h, *_floor(min_logdens_per_count)))

    def countholdout_begin(self, dst, min_logdens=None, min_logdens_per_count=None):
        """dpmm_countholdout_begin: a new collection of the points below the floor min_logdens and / or the floor per count (None: not in
        use).  dst: None (count only) or a dict -- `cap`, `index` and either `points` [cap][D] float32 (dense stores) or `colptr` [cap + 1]
        int64, `rowval` [entry_cap] int32, `val` [entry_cap] float32 and `entry_cap` (sparse store) -- of device addresses (integers) or
        torch tensors on this worker's GPU, which the caller keeps alive until countholdout_read."""
        dst = dict(dst or {})
        addr = _device_addresses(*[dst.get(k) for k in ("points", "colptr", "rowval", "val", "index")])
        d = CountHoldoutDst(*[a or None for a in addr], int(dst.get("cap", 0)), int(dst.get("entry_cap", 0)))
        self._chk(self._lib.dpmm_countholdout_begin(self._h, *_floor(min_logdens), *_floor(min_logdens_per_count), ctypes.byref(d)))

    def countholdout_accumulate(self, lo, n_valid):
        """dpmm_countholdout_accumulate: classifies the points 0..n_valid-1 of the current upload, global indices lo + i, and appends the
        held-out ones from whichever store is live."""
        self._chk(self._lib.dpmm_countholdout_accumulate(self._h, int(lo), int(n_valid)))

    def countholdout_read(self):
        """The counters as they stand, after the stream has been waited for: a dict of ints `total`, `total_entries`, `stored`,
        `stored_entries`, `skipped`, `incomplete`, `scored`."""
        cnt = np.zeros(7, np.int64)
        out = CountHoldoutOut(*[cnt[j:].ctypes.data for j in range(7)])
        self._chk(self._lib.dpmm_countholdout_read(self._h, ctypes.byref(out)))
        return dict(zip(("total", "total_entries", "stored", "stored_entries", "skipped", "incomplete", "scored"), (int(v) for v in cnt)))

    # ---- label trace (include/dpmm_hip_trace.h)
    def trace_open(self, slots):
        """dpmm_trace_open: room for `slots` labellings of the shard (16-bit cluster ids) on the GPU; an open trace is replaced."""
        self._chk(self._lib.dpmm_trace_open(self._h, int(slots)))
        self._trace_K = {}

    def trace_close(self):
        self._chk(self._lib.dpmm_trace_close(self._h))
        self._trace_K = {}

    def trace_record(self, slot, K):
        """dpmm_trace_record: the labels in force into `slot`, with K clusters; returns without waiting for the GPU."""
        self._chk(self._lib.dpmm_trace_record(self._h, int(slot), int(K)))
        self._trace_K[int(slot)] = int(K)

    def trace_tables(self, pairs):
        """dpmm_trace_tables: for every (s, t) of `pairs` the (K[s], K[t]) int64 contingency table of the two recorded labellings of this
        shard, a list in the order of `pairs`."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        known = getattr(self, "_trace_K", {})
        shapes = [(known.get(int(s), 0), known.get(int(t), 0)) for s, t in pairs]
        counts = np.zeros(max(1, sum(a * b for a, b in shapes)), np.int64)
        self._chk(self._lib.dpmm_trace_tables(self._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(pairs), _p(counts, _c_i64p)))
        out, off = [], 0
        for a, b in shapes:
            out.append(counts[off:off + a * b].reshape(a, b))
            off += a * b
        return out

    def trace_confidence(self, anchor, slots, ratio, device=None):
        """dpmm_trace_confidence: per local point the mean over `slots` of ratio[j][z_anchor, z_slots[j]], Float32 (n,).  ratio: one
        (K[anchor], K[s]) table per listed slot.  device: a torch device -- the result is a tensor there; None: a numpy array."""
        slots = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        flat = np.concatenate([_f32(r).ravel() for r in ratio]) if len(ratio) else np.zeros(0, np.float32)
        known = getattr(self, "_trace_K", {})
        assert len(ratio) == len(slots) and flat.size == sum(known.get(int(anchor), 0) * known.get(int(s), 0) for s in slots)
        flat = _f32(flat) if flat.size else np.zeros(1, np.float32)
        sp = slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if device is not None:
            import torch
            out = torch.empty(self.n, dtype=torch.float32, device=device)
            torch.cuda.current_stream(out.device).synchronize()
            if self.n:                 # (an empty tensor has no address to hand over)
                self._chk(self._lib.dpmm_trace_confidence(self._h, int(anchor), sp, len(slots), _p(flat, _c_f32p), None, ctypes.c_void_p(out.data_ptr())))
            return out
        out = np.empty(self.n, np.float32)
        self._chk(self._lib.dpmm_trace_confidence(self._h, int(anchor), sp, len(slots), _p(flat, _c_f32p), _p(out, _c_f32p), None))
        return out

    def trace_read(self, slot, device=None):
        """dpmm_trace_read: the labels of `slot`, 1-based int64 (n,): a tensor on `device`, or a numpy array."""
        if device is not None:
            import torch
            out = torch.empty(self.n, dtype=torch.int64, device=device)
            torch.cuda.current_stream(out.device).synchronize()
            if self.n:
                self._chk(self._lib.dpmm_trace_read(self._h, int(slot), None, ctypes.c_void_p(out.data_ptr())))
            return out
        out = np.empty(self.n, np.int64)
        self._chk(self._lib.dpmm_trace_read(self._h, int(slot), _p(out, _c_i64p), None))
        return out

    # ---- on-device evaluation
    def set_ground_truth(self, gt):
        """gt: integer ids of this shard's points (any integers; remapped to 0..n_gt-1 by the caller)."""
        gt = _i64(gt)
        self.n_gt = int(gt.max()) + 1 if len(gt) else 1
        self._chk(self._lib.dpmm_set_ground_truth(self._h, _p(gt, _c_i64p), self.n_gt))

    def set_ground_truth_range(self, gt, n_gt):
        gt = _i64(gt)
        self.n_gt = int(n_gt)
        self._chk(self._lib.dpmm_set_ground_truth(self._h, _p(gt, _c_i64p), self.n_gt))

    def contingency(self, K=None):
        K = self.K if K is None else K
        out = np.zeros((K, self.n_gt), np.int64)
        self._chk(self._lib.dpmm_contingency(self._h, K, _p(out, _c_i64p)))
        return out

    def bin_counts(self):
        """(K, 2) Int64: points per (cluster, sub-cluster) of this shard -- the N of the l / r statistics."""
        out = np.zeros((self.K, 2), np.int64)
        self._chk(self._lib.dpmm_bin_counts(self._h, _p(out, _c_i64p)))
        return out

    # ---- smart splits (worker halves of smart_cluster_init!)
    def smart_project(self, cluster, v, mu):
        """Projections t = v.(x - mu) of the points of `cluster` (1-based), in arbitrary order (Float64)."""
        v = np.ascontiguousarray(v, np.float64); mu = np.ascontiguousarray(mu, np.float64)
        assert v.shape == (self.D,) and mu.shape == (self.D,)
        vals = np.empty(max(self.n, 1), np.float64)
        cnt = np.zeros(1, np.int64)
        self._chk(self._lib.dpmm_smart_project(self._h, int(cluster), _p(v, _c_f64p), _p(mu, _c_f64p), _p(vals, _c_f64p), _p(cnt, _c_i64p)))
        return vals[:int(cnt[0])]

    def smart_kmeans_iter(self, cluster, m_lo, m_hi):
        out = np.zeros(4, np.float64)
        self._chk(self._lib.dpmm_smart_kmeans_iter(self._h, int(cluster), float(m_lo), float(m_hi), _p(out, _c_f64p)))
        return out

    def smart_assign(self, cluster, m_lo, m_hi):
        self._chk(self._lib.dpmm_smart_assign(self._h, int(cluster), float(m_lo), float(m_hi)))

    # ---- options / collective
    def set_option(self, option, value):
        self._chk(self._lib.dpmm_set_option(self._h, int(option), float(value)))

    def _use_torch_rccl(self):
        """One RCCL per process: when torch is importable, bind the library to torch's own librccl.so."""
        try:
            import torch
            cand = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
            if os.path.exists(cand):
                self._lib.dpmm_comm_use_library(cand.encode())
        except ImportError:
            pass

    def comm_unique_id(self):
        self._use_torch_rccl()
        buf = ctypes.create_string_buffer(128)
        rc = self._lib.dpmm_comm_unique_id(buf)
        if rc != 0:
            raise DpmmError(rc, self._lib.dpmm_last_error(None).decode())
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        self._use_torch_rccl()
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._lib.dpmm_comm_init(self._h, buf, int(rank), int(world)))

    def comm_init_host(self, rank, world, allreduce):
        """dpmm_comm_init_host: `allreduce(arr)` sums a 1-D numpy array (float64 or int64, a VIEW of the library's pinned staging)
        over the ranks IN PLACE.  The statistics calls then return rows summed over the ranks, as with comm_init."""
        def cb(_, buf, count, is_f64):
            try:
                t = ctypes.c_double if is_f64 else ctypes.c_int64
                allreduce(np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(t)), shape=(int(count),)))
                return 0
            except Exception as e:  # noqa: BLE001 -- must not unwind through the C frames; the library reports DPMM_ECOMM
                self._comm_error = e
                return 1
        self._host_cb = HOST_ALLREDUCE_FN(cb)       # keep the trampoline alive as long as the context
        self._chk(self._lib.dpmm_comm_init_host(self._h, int(rank), int(world), ctypes.cast(self._host_cb, ctypes.c_void_p), None))

    def comm_info(self):
        out = np.zeros(8, np.int64)
        self._chk(self._lib.dpmm_comm_info(self._h, _p(out, _c_i64p)))
        return dict(world=int(out[0]), rank=int(out[1]), transport={0: "none", 1: "rccl", 2: "host"}[int(out[2])],
                    counts_bytes=int(out[3]), rows_bytes=int(out[4]), allreduces=int(out[5]), one_collective=bool(out[7]))

    def last_comm_ms(self):
        """(occupancy all-reduce ms, packed-row all-reduce ms) of the last statistics pass (HIP events on the ctx stream)."""
        a = ctypes.c_float(); b = ctypes.c_float()
        self._chk(self._lib.dpmm_last_comm_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def numa_node(self):
        """dpmm_numa_node: NUMA node of the host this context's GPU is attached to (-1: unknown)."""
        return int(self._lib.dpmm_numa_node(self._h))

    # ---- the master's dense maths on the device (NIW)
    def master_setup(self, kappa, nu, m, psi):
        m = np.ascontiguousarray(m, np.float64); psi = np.ascontiguousarray(psi, np.float64)
        self._chk(self._lib.dpmm_niw_master_setup(self._h, float(kappa), float(nu), m.ctypes.data, psi.ctypes.data))

    def step_stats_device(self, reset_epoch):
        bad = ctypes.c_void_p()
        self._chk(self._lib.dpmm_step_stats_device(self._h, int(reset_epoch), ctypes.byref(bad)))
        return np.ctypeslib.as_array(ctypes.cast(bad, ctypes.POINTER(ctypes.c_uint8)), shape=(self.K,)).copy()

    def suffstats_device(self, cluster_idx=None):
        idx = None if cluster_idx is None else np.ascontiguousarray(cluster_idx, np.int64)
        self._chk(self._lib.dpmm_suffstats_device(self._h, None if idx is None else idx.ctypes.data, 0 if idx is None else len(idx)))

    def master_posterior(self, clusters, slots):
        """dpmm_niw_master_posterior: (n, 3, 8) float64 {N, kappa', nu', log det(nu' psi'), log Gamma_D(nu' / 2), 3 spare} for the listed clusters (1-based)."""
        slots = np.ascontiguousarray(slots, np.int32)
        cl = None if clusters is None else np.ascontiguousarray(clusters, np.int64)
        out = ctypes.c_void_p()
        self._chk(self._lib.dpmm_niw_master_posterior(self._h, None if cl is None else cl.ctypes.data, slots.ctypes.data, len(slots), ctypes.byref(out)))
        return np.ctypeslib.as_array(ctypes.cast(out, _c_f64p), shape=(len(slots), 3, MASTER_NSCALARS)).copy()

    def master_draw(self, epoch, slot_of_cluster, lr_weights, weights):
        sl = np.ascontiguousarray(slot_of_cluster, np.int32)
        lr = np.ascontiguousarray(lr_weights, np.float32); w = np.ascontiguousarray(weights, np.float32)
        self._chk(self._lib.dpmm_niw_master_draw(self._h, int(epoch), len(sl), sl.ctypes.data, lr.ctypes.data, w.ctypes.data))

    def master_pairs(self, slots_i, slots_j):
        """dpmm_niw_master_pairs: (n, 8) float64 {N, kappa', nu', log det(nu' psi'), log Gamma_D(nu' / 2), 3 spare} of the pooled statistics of the slot pairs."""
        a = np.ascontiguousarray(slots_i, np.int32); b = np.ascontiguousarray(slots_j, np.int32)
        out = ctypes.c_void_p()
        self._chk(self._lib.dpmm_niw_master_pairs(self._h, a.ctypes.data, b.ctypes.data, len(a), ctypes.byref(out)))
        return np.ctypeslib.as_array(ctypes.cast(out, _c_f64p), shape=(len(a), MASTER_NSCALARS)).copy()

    def master_pairs_ahead(self, slots_i, slots_j):
        """dpmm_niw_master_pairs_ahead: the pairs the next step_master_device computes behind its posteriors."""
        a = np.ascontiguousarray(slots_i, np.int32); b = np.ascontiguousarray(slots_j, np.int32)
        self._chk(self._lib.dpmm_niw_master_pairs_ahead(self._h, a.ctypes.data, b.ctypes.data, len(a)))

    def step_master_device(self, reset_epoch, slots, draw_epoch=0):
        """dpmm_step_master_device: statistics + all posteriors in one call -> (bad flags (K,), scalars (K, 3, 8))."""
        sl = np.ascontiguousarray(slots, np.int32)
        bad = ctypes.c_void_p(); out = ctypes.c_void_p()
        self._chk(self._lib.dpmm_step_master_device(self._h, int(reset_epoch), sl.ctypes.data, int(draw_epoch), ctypes.byref(bad), ctypes.byref(out)))
        return (np.ctypeslib.as_array(ctypes.cast(bad, ctypes.POINTER(ctypes.c_uint8)), shape=(self.K,)).copy(),
                np.ctypeslib.as_array(ctypes.cast(out, _c_f64p), shape=(len(sl), 3, MASTER_NSCALARS)).copy())

    def master_rows(self, slots):
        sl = np.ascontiguousarray(slots, np.int32)
        out = np.empty((len(sl), 2, self.packed_stride), np.float64)
        self._chk(self._lib.dpmm_niw_master_rows(self._h, sl.ctypes.data, len(sl), out.ctypes.data))
        return out

    def master_draws(self, K):
        mu = np.empty((3 * K, self.D), np.float32); R = np.empty((3 * K, self.D, self.D), np.float32); ld = np.empty(3 * K, np.float32)
        self._chk(self._lib.dpmm_niw_master_draws(self._h, int(K), mu.ctypes.data, R.ctypes.data, ld.ctypes.data))
        return mu, R, ld

    # ---- the Multinomial master's draws on the device
    def mult_master_setup(self, alpha, alpha_outlier=None):
        a = np.ascontiguousarray(alpha, np.float32); b = None if alpha_outlier is None else np.ascontiguousarray(alpha_outlier, np.float32)
        self._chk(self._lib.dpmm_mult_master_setup(self._h, a.ctypes.data, None if b is None else b.ctypes.data))

    def mult_master_draw(self, epoch, lr_weights, weights, outlier_first=False):
        lr = np.ascontiguousarray(lr_weights, np.float32); w = np.ascontiguousarray(weights, np.float32)
        self._chk(self._lib.dpmm_mult_master_draw(self._h, int(epoch), len(w), int(bool(outlier_first)), lr.ctypes.data, w.ctypes.data))

    def mult_master_draws(self, K):
        out = np.empty((3 * K, self.D), np.float32)
        self._chk(self._lib.dpmm_mult_master_draws(self._h, int(K), out.ctypes.data))
        return out

    def mult_master_pairs_ahead(self, ki, kj, outlier_first=False):
        a = np.ascontiguousarray(ki, np.int32); b = np.ascontiguousarray(kj, np.int32)
        self._chk(self._lib.dpmm_mult_master_pairs_ahead(self._h, int(bool(outlier_first)), a.ctypes.data, b.ctypes.data, len(a)))

    def mult_master_marginals(self, K):
        """-> (N [3K], log-marginals [3K], pooled log-marginals of the pairs asked for ahead)"""
        pn, pl, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
        self._chk(self._lib.dpmm_mult_master_marginals(self._h, int(K), ctypes.byref(pn), ctypes.byref(pl), ctypes.byref(n)))
        nl = np.ctypeslib.as_array(ctypes.cast(pn, ctypes.POINTER(ctypes.c_double)), shape=(3 * K, 2)).copy()
        pairs = np.ctypeslib.as_array(ctypes.cast(pl, ctypes.POINTER(ctypes.c_double)), shape=(max(n.value, 1),)).copy()[:n.value]
        return nl[:, 0], nl[:, 1], pairs

    def mult_master_put_rows(self, rows):
        r = np.ascontiguousarray(rows, np.float64)
        self._chk(self._lib.dpmm_mult_master_put_rows(self._h, r.ctypes.data, r.shape[0] // 2))

    def debug_draw_inputs(self, epoch, slot_of_cluster):
        """dpmm_debug_niw_draw_inputs: (A (3K, D, D) Bartlett factors, xi (3K, D)) the device draw of `epoch` consumes."""
        sl = np.ascontiguousarray(slot_of_cluster, np.int32)
        K = len(sl)
        A = np.empty((3 * K, self.D, self.D), np.float64); xi = np.empty((3 * K, self.D), np.float64)
        self._chk(self._lib.dpmm_debug_niw_draw_inputs(self._h, int(epoch), K, sl.ctypes.data, A.ctypes.data, xi.ctypes.data))
        return A, xi

    def step_stats(self, reset_epoch):
        """dpmm_step_stats: (packed (2K, stride) float64, bad (K,) uint8) -- copies of the ctx's pinned output."""
        pk, bad = ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(self._lib.dpmm_step_stats(self._h, int(reset_epoch), ctypes.byref(pk), ctypes.byref(bad)))
        packed = np.ctypeslib.as_array(ctypes.cast(pk, _c_f64p), shape=(2 * self.K, self.packed_stride)).copy()
        flags = np.ctypeslib.as_array(ctypes.cast(bad, ctypes.POINTER(ctypes.c_uint8)), shape=(self.K,)).copy()
        return packed, flags

    def init_labels_from(self, init_clusters, first_label, epoch):
        self._chk(self._lib.dpmm_init_labels_from(self._h, int(init_clusters), int(first_label), int(epoch)))

    def last_sweep_work(self):
        """dict of the executed-work counters of the NIW sweeps since the previous call, PER LAUNCH (dpmm_last_sweep_work returns their
        totals and the number of launches, and clears them): after every sweep = that sweep's; after a timed loop = its average."""
        out = (ctypes.c_uint64 * 16)()
        self._chk(self._lib.dpmm_last_sweep_work(self._h, out))
        v = [int(x) for x in out]
        n = max(1, v[7])
        sp = 8 * ((self.K + 15) // 16)      # bf16 matrix instructions of one direction screen: two per 16 clusters and point group
        # executed_flops: Float32 matrix work only (= SQ_INSTS_VALU_MFMA_MOPS_F32 x 512); the bf16 work (brackets, screens) beside it
        dirs, b3 = v[15] & 0xFFFFFFFF, v[15] >> 32      # direction screens | bf16 three-plane sub-cluster evaluations (144 bf16 matrix instructions + 4 Float32 row sums each)
        tops, cheap = v[13] & 0xFFFFFFFF, v[13] >> 32  # bf16 top screens | tiles the lean kernel settled by the norm certificate (no bracket)
        bf16 = v[8] * v[9] + v[11] * v[12] + tops * v[14] + dirs * sp + b3 * 144
        return dict(wave_tiles=v[0] / n, full_evals=v[1] / n, screens16=v[2] / n, tail_pairs=v[3] / n, mfma_per_full=v[4], mfma_per_screen=v[5],
                    flops_per_mfma=v[6], executed_flops=(v[1] * v[4] + v[2] * v[5] + 4 * b3) * v[6] / n, launches=v[7],
                    brackets=v[8] / n, bf16_mfma_per_bracket=v[9], bf16_bottom_screens=v[11] / n, bf16_top_screens=tops / n,
                    direction_screens=dirs / n, b3_evals=b3 / n, norm_cert_tiles=cheap / n,
                    bf16_mfma=bf16 / n, bf16_flops=bf16 * v[10] / n)

    # ---- diagnostics
    def debug_subloglik(self):
        """(2K, n) float32: row 2k+s = log-likelihood under sub-cluster s of cluster k + log lr_weights[k][s]."""
        out = np.empty((2 * self.K, self.n), np.float32)
        self._chk(self._lib.dpmm_debug_subloglik(self._h, _p(out, _c_f32p)))
        return out

    def debug_ref_bracket(self, cluster, c_override=0.0):
        """(q_hi, q): per point, the reference bracket's upper end and the Float32 quadratic form of `cluster` (1-based); include/dpmm_hip_debug.h."""
        qhi = np.empty(self.n, np.float32); q = np.empty(self.n, np.float32)
        self._chk(self._lib.dpmm_debug_ref_bracket(self._h, int(cluster), ctypes.c_float(c_override), _p(qhi, _c_f32p), _p(q, _c_f32p)))
        return qhi, q

    def debug_pair_ball(self):
        """(pd (K, K), sn (K,)): the pair-ball table of the parameters on the device; include/dpmm_hip_debug.h."""
        pd = np.empty((self.K, self.K), np.float32); sn = np.empty(self.K, np.float32)
        self._chk(self._lib.dpmm_debug_pair_ball(self._h, _p(pd, _c_f32p), _p(sn, _c_f32p)))
        return pd, sn

    def debug_pair_ball_sn2(self):
        """sn2 (K,): the pair-ball table's tighter norm bounds (DPMM_OPT_LEAN_NORM_CERT); include/dpmm_hip_debug.h."""
        sn2 = np.empty(self.K, np.float32)
        self._chk(self._lib.dpmm_debug_pair_ball_sn2(self._h, _p(sn2, _c_f32p)))
        return sn2

    def debug_norm_cert_points(self, enable=True, read=True):
        """bool (n,): the points whose tile the lean kernel's norm certificate settled in the sweeps since the record was last cleared (read=False, or
        the record was off: None); then the record is cleared and stays on (enable) or is freed; include/dpmm_hip_debug.h."""
        out = np.zeros(self.n, np.uint8) if read else None
        self._chk(self._lib.dpmm_debug_norm_cert_points(self._h, int(bool(enable)), _p(out, ctypes.POINTER(ctypes.c_uint8)) if read else None))
        return None if out is None else out.astype(bool)

    def debug_bracket_big(self):
        """(aref (n,), tile_flags (ceil(n / 128),)): what the D > 64 sweep reads from the bracket launch in front of it; include/dpmm_hip_debug.h."""
        aref = np.empty(self.n, np.float32); fl = np.empty((self.n + 127) // 128, np.uint32)
        self._chk(self._lib.dpmm_debug_bracket_big(self._h, _p(aref, _c_f32p), fl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return aref, fl

    def debug_mult_draws_ahead(self):
        """dpmm_mult_master_draw calls that took the draws launched ahead by dpmm_step_stats; include/dpmm_hip_debug.h."""
        v = ctypes.c_longlong(0)
        self._chk(self._lib.dpmm_debug_mult_draws_ahead(self._h, ctypes.byref(v)))
        return int(v.value)

    def debug_loglik(self):
        out = np.empty((self.K, self.n), np.float32)
        self._chk(self._lib.dpmm_debug_loglik(self._h, _p(out, _c_f32p)))
        return out

    def sync(self):
        self._chk(self._lib.dpmm_sync(self._h))

    @property
    def stream(self):
        return self._lib.dpmm_stream(self._h)

    def set_timing(self, on):
        """on: False / True (sweep + statistics + all-reduce events) or a bit mask 1 (sweep kernel) | 2 (statistics) | 4 (all-reduces)."""
        mask = 7 if on is True else int(on)      # (bit 3 = 8: the three parts of a D <= 64 sweep, last_sweep_parts_ms)
        self.timing = mask != 0
        self.set_option(OPT_KERNEL_TIMING, float(mask))

    def last_sweep_parts_ms(self):
        """(lean, labels, sub-labels) milliseconds of the last sweep's three launches (timing bits 0 and 3; zeros otherwise)."""
        out = np.zeros(3, np.float32)
        self._chk(self._lib.dpmm_last_sweep_parts_ms(self._h, _p(out, _c_f32p)))
        return [float(v) for v in out]

    def last_kernel_ms(self):
        if not self.timing:
            raise RuntimeError("kernel timing is off for this Worker (timing=False / set_timing(False)): no events were recorded")
        a = ctypes.c_float(); b = ctypes.c_float()
        self._chk(self._lib.dpmm_last_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def debug_sort_tables(self):
        """The counting sort of the last statistics pass (dpmm_debug_sort_tables): (perm[:perm_total] int32 point indices grouped by
        bin = 2 (label - 1) + (sub - 1), bin_total (2K,), bin_start (2K + 1,))."""
        perm = np.empty(max(self.n, 1), np.int32); tot = np.empty(2 * self.K, np.int32); start = np.empty(2 * self.K + 1, np.int32)
        ptot = np.zeros(1, np.int32)
        self._chk(self._lib.dpmm_debug_sort_tables(self._h, perm.ctypes.data, tot.ctypes.data, start.ctypes.data, ptot.ctypes.data))
        return perm[:int(ptot[0])].copy(), tot, start

    def debug_counters(self):
        """Health counters of the worker (include/dpmm_hip.h dpmm_debug_counters): [0] = event waits that returned early."""
        out = (ctypes.c_int64 * 4)()
        self._chk(self._lib.dpmm_debug_counters(self._h, out, 4))
        return list(out)
