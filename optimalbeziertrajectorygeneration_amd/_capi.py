"""ctypes binding of libobtg_hip.so (include/obtg.h).

This is the ONLY compute path of the package: there is no CPU fallback.  Importing
works without a GPU (so that host logic can be tested), but creating a `Context`
raises `RuntimeError` when the library is missing or no gfx950 device is usable.
"""
import ctypes as C
import os
import threading
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OBTG_LIB") or os.path.join(HERE, "libobtg_hip.so")   # OBTG_LIB: experimental builds (tools/build_variant.sh)

OK = 0
ST_OK, ST_MD_CAP, ST_MAXITER, ST_CYCLE = 0, 1, 2, 3
MD_OK, MD_NODE_CAP, MD_DEPTH_CAP, MD_GJK_CAP = 0, 1, 2, 3
PROX_WITHIN, PROX_REACH = 0, 1     # the kinds of a proximity item (obtg_ctx_set_proximity): the minimum / the maximum of g
K_TEMPORAL_SEP, K_SPEED, K_ANG_RATE, K_GJK, K_MIN_DIST, K_FD_BATCH, K_BERN, K_PAIR_SWEEP, K_JAC, K_COUNT = range(10)
K_ARC_LENGTH, K_END = 9, 10      # ids added after ABI revision 7 was cut: OBTG_K_COUNT stays what that revision's callers sized arrays by

_lib = None

_vp = C.c_void_p
_i = C.c_int
_d = C.c_double

# name -> (restype, argtypes); mirrors include/obtg.h one to one
_SIGNATURES = {
    "obtg_strerror": (C.c_char_p, [_i]),
    "obtg_last_error": (C.c_char_p, [_vp]),
    "obtg_abi_version": (_i, []),
    "obtg_source_hash": (C.c_char_p, [C.c_char_p]),
    "obtg_libm_pow_matches": (_i, []),
    "obtg_fast_kernels": (_i, [_i, _i]),
    "obtg_device_count": (_i, []),
    "obtg_abi_symbols": (_vp, []),
    "obtg_host_alloc": (_i, [C.c_size_t, C.POINTER(_vp)]),
    "obtg_host_free": (_i, [_vp]),
    "obtg_ctx_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _vp, _i]),
    "obtg_ctx_destroy": (None, [_vp]),
    "obtg_ctx_set_stream": (_i, [_vp, _vp]),
    "obtg_ctx_use_own_stream": (_i, [_vp]),
    "obtg_ctx_set_deg_elev": (_i, [_vp, _i]),
    "obtg_ctx_set_ang_rate_order": (_i, [_vp, _i]),
    "obtg_ctx_ang_rate_order_in_effect": (_i, [_vp]),
    "obtg_ctx_set_second_speed_bound": (_i, [_vp, _d, _i, _vp]),
    "obtg_constraint_sweep_fd_structured_dev": (_i, [_vp, _vp, _i, _d, _vp, _i, _d, _vp, _d, _i, _d, _vp, _vp, _i, _i, _vp, _vp,
                                                     _vp, _vp, _vp, _vp]),
    "obtg_constraint_sweep_fd_structured_rows_dev": (_i, [_vp, _vp, _i, _d, _i, _vp, _i, _d, _vp, _d, _i, _d, _vp, _vp, _i, _i, _vp,
                                                          _vp, _vp, _vp, _vp, _vp]),
    "obtg_one_vs_many_min": (_i, [_vp, _vp, _i, _vp, _i, _d, _vp]),
    "obtg_one_vs_many_min_dev": (_i, [_vp, _vp, _i, _vp, _i, _d, _vp]),
    "obtg_one_vs_many_min_spans": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _d, _d, _vp]),
    "obtg_one_vs_many_min_spans_dev": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _d, _d, _vp]),
    "obtg_sync": (_i, [_vp]),
    "obtg_len_temporal_sep": (_i, [_vp]),
    "obtg_len_speed": (_i, [_vp]),
    "obtg_len_ang_rate": (_i, [_vp]),
    "obtg_num_pairs": (_i, [_vp]),
    "obtg_temporal_sep": (_i, [_vp, _vp, _i, _d, _vp]),
    "obtg_speed": (_i, [_vp, _vp, _vp, _i, _d, _i, _vp]),
    "obtg_ang_rate": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_temporal_sep_min": (_i, [_vp, _vp, _i, _d, _vp]),
    "obtg_temporal_sep_active": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp]),
    "obtg_temporal_sep_active_dev": (_i, [_vp, _vp, _i, _d, _i, _i, _i, _vp, _vp]),
    "obtg_temporal_sep_min_gather_dev": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_temporal_sep_fd_min_rows_dev": (_i, [_vp, _vp, _i, _d, _i, _i, _d, _vp]),
    "obtg_comm_unique_id": (_i, [_vp]),
    "obtg_comm_create": (_i, [C.POINTER(_vp), _i, _i, _vp, _i]),
    "obtg_comm_destroy": (None, [_vp]),
    "obtg_comm_size": (_i, [_vp]),
    "obtg_comm_rank": (_i, [_vp]),
    "obtg_comm_last_error": (C.c_char_p, [_vp]),
    "obtg_comm_all_gather_dev": (_i, [_vp, _vp, _vp, _vp, C.c_size_t]),
    "obtg_pair_block": (_i, [_vp, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "obtg_unpack_pair_blocks_dev": (_i, [_vp, _vp, _i, _i, _vp]),
    "obtg_temporal_sep_min_range": (_i, [_vp, _vp, _i, _d, _i, _i, _vp]),
    "obtg_temporal_sep_fd": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _d, _vp]),
    "obtg_temporal_sep_fd_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _d, _vp]),
    "obtg_temporal_sep_dev": (_i, [_vp, _vp, _i, _d, _i, _i, _vp]),
    "obtg_temporal_sep_min_dev": (_i, [_vp, _vp, _i, _d, _i, _i, _vp]),
    "obtg_speed_dev": (_i, [_vp, _vp, _vp, _i, _d, _i, _vp]),
    "obtg_ang_rate_dev": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_dynamics_dev": (_i, [_vp, _vp, _vp, _i, _d, _i, _d, _vp, _vp]),
    "obtg_fd_batch_dev": (_i, [_vp, _vp, _i, _d, _i, _vp]),
    "obtg_fd_view_begin": (_i, [_vp, _vp, _i, _d, _i]),
    "obtg_fd_view_begin_rows": (_i, [_vp, _vp, _i, _d, _i, _i]),
    "obtg_fd_view_end": (_i, [_vp]),
    "obtg_fd_forms_on_the_fly": (_i, [_vp]),
    "obtg_pair_sweep_fd_dev": (_i, [_vp, _vp, _i, _d, _i, _d, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_dynamics_fd_dev": (_i, [_vp, _vp, _i, _d, _vp, _i, _d, _i, _d, _vp, _vp]),
    "obtg_gjk_pairs": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "obtg_ctx_set_polygons": (_i, [_vp, _vp, _i, _vp, _i]),
    "obtg_ctx_set_hull_pairs": (_i, [_vp, _vp, _vp, _i]),
    "obtg_ctx_set_fd_dedup": (_i, [_vp, _i]),
    "obtg_ctx_set_fd_view_structured": (_i, [_vp, _i]),
    "obtg_ctx_set_gjk_history": (_i, [_vp, _i]),
    "obtg_sweep_shape": (_i, [_vp, _i, _i, _i, _vp]),
    "obtg_pair_sweep_dev": (_i, [_vp, _vp, _i, _d, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_gjk_swarm_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_constraint_sweep_dev": (_i, [_vp, _vp, _vp, _i, _d, _vp, _d, _i, _d, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_gjk_swarm": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_min_dist": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _d, _i, _i, _i, _i, _vp, _vp, _vp]),
    "obtg_min_dist_mixed": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _d, _i, _i, _i, _i, _vp, _vp, _vp]),
    "obtg_min_dist_robust": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_min_dist2poly": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _d, _i, _i, _i, _i, _vp, _vp, _vp]),
    "obtg_min_dist2poly_robust": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_gjk_true_pairs": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_coll_check": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _d, _i, _i, _i, _vp, _vp, _vp]),
    "obtg_coll_check2poly": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "obtg_bern_extrema": (_i, [_vp, _vp, _i, _i, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_bern_extrema_dev": (_i, [_vp, _vp, _i, _i, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_temporal_sep_true_min": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_temporal_sep_true_min_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_temporal_sep_true_min_jac": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp]),
    "obtg_temporal_sep_true_min_jac_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp]),
    "obtg_speed_true_min": (_i, [_vp, _vp, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_speed_true_min_dev": (_i, [_vp, _vp, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_speed_true_min_jac": (_i, [_vp, _vp, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_speed_true_min_jac_dev": (_i, [_vp, _vp, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_ang_rate_poly": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_ang_rate_poly_dev": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_ang_rate_true_min": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_ang_rate_true_min_dev": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_ang_rate_true_min_jac": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_ang_rate_true_min_jac_dev": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_curvature_poly": (_i, [_vp, _vp, _i, _vp]),
    "obtg_curvature_poly_dev": (_i, [_vp, _vp, _i, _vp]),
    "obtg_curvature_true_min": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_curvature_true_min_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_curvature_true_min_jac": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp]),
    "obtg_curvature_true_min_jac_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp]),
    "obtg_bern_curvature": (_i, [_vp, _vp, _i, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_bern_curvature_dev": (_i, [_vp, _vp, _i, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_space_curvature_poly": (_i, [_vp, _vp, _i, _vp]),
    "obtg_space_curvature_poly_dev": (_i, [_vp, _vp, _i, _vp]),
    "obtg_space_curvature_true_min": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_space_curvature_true_min_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_space_curvature_true_min_jac": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp]),
    "obtg_space_curvature_true_min_jac_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp]),
    "obtg_bern_space_curvature": (_i, [_vp, _vp, _i, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_bern_space_curvature_dev": (_i, [_vp, _vp, _i, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_bern_elev": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "obtg_bern_diff": (_i, [_vp, _vp, _i, _i, _d, _vp]),
    "obtg_bern_mul": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "obtg_bern_normsq": (_i, [_vp, _vp, _i, _i, _vp]),
    "obtg_bern_split": (_i, [_vp, _vp, _i, _i, _d, _vp, _vp]),
    "obtg_bern_restrict": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "obtg_bern_eval": (_i, [_vp, _vp, _i, _i, _vp, _i, _d, _d, _vp]),
    "obtg_euclidean_obj": (_i, [_vp, _vp, _i, _vp]),
    "obtg_accel_obj": (_i, [_vp, _vp, _vp, _i, _vp]),
    "obtg_jerk_obj": (_i, [_vp, _vp, _vp, _i, _vp]),
    "obtg_bern_arc_length": (_i, [_vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_bern_arc_length_dev": (_i, [_vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_arc_length_obj": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_arc_length_obj_dev": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_temporal_sep_jac": (_i, [_vp, _vp, _i, _vp]),
    "obtg_temporal_sep_jac_dev": (_i, [_vp, _vp, _i, _vp]),
    "obtg_accel": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_accel_dev": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_accel_true_min": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_accel_true_min_dev": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_accel_true_min_jac": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_accel_true_min_jac_dev": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_ctx_set_proximity": (_i, [_vp, _vp, _vp, _vp, _i, _i]),
    "obtg_len_proximity": (_i, [_vp]),
    "obtg_proximity_poly": (_i, [_vp, _vp, _i, _vp]),
    "obtg_proximity_poly_dev": (_i, [_vp, _vp, _i, _vp]),
    "obtg_proximity_true": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_proximity_true_dev": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_proximity_true_jac": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_proximity_true_jac_dev": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_ctx_set_keep_in": (_i, [_vp, _vp, _i, _vp, _i]),
    "obtg_len_keep_in": (_i, [_vp]),
    "obtg_keep_in": (_i, [_vp, _vp, _i, _vp]),
    "obtg_keep_in_dev": (_i, [_vp, _vp, _i, _vp]),
    "obtg_keep_in_true_min": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_keep_in_true_min_dev": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_keep_in_true_min_jac": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp, _vp]),
    "obtg_keep_in_true_min_jac_dev": (_i, [_vp, _vp, _i, _d, _i, _vp, _vp, _vp, _vp]),
    "obtg_ctx_set_keep_out": (_i, [_vp, _vp, _vp, _i, _vp, _i]),
    "obtg_len_keep_out": (_i, [_vp]),
    "obtg_keep_out_true_min": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_keep_out_true_min_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_keep_out_true_min_jac": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_keep_out_true_min_jac_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_bern_keep_out": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_bern_keep_out_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_ctx_set_keep_out_motion": (_i, [_vp, _vp, _vp, _vp, _i]),
    "obtg_keep_out_moving_true_min": (_i, [_vp, _vp, _vp, _i, _d, _d, _i] + [_vp] * 8),
    "obtg_keep_out_moving_true_min_dev": (_i, [_vp, _vp, _vp, _i, _d, _d, _i] + [_vp] * 8),
    "obtg_keep_out_moving_true_min_jac": (_i, [_vp, _vp, _vp, _i, _d, _d, _i] + [_vp] * 10),
    "obtg_keep_out_moving_true_min_jac_dev": (_i, [_vp, _vp, _vp, _i, _d, _d, _i] + [_vp] * 10),
    "obtg_bern_keep_out_moving": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _d, _i, _vp, _vp, _vp]),
    "obtg_bern_keep_out_moving_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _d, _i, _vp, _vp, _vp]),
    "obtg_keep_out_features": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "obtg_keep_out_euclid_true_min": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_keep_out_euclid_true_min_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_keep_out_euclid_true_min_jac": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_keep_out_euclid_true_min_jac_dev": (_i, [_vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "obtg_bern_keep_out_euclid": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_bern_keep_out_euclid_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _d, _i, _vp, _vp, _vp]),
    "obtg_ctx_set_pair_keep_out": (_i, [_vp, _vp, _i]),
    "obtg_len_pair_keep_out": (_i, [_vp]),
    "obtg_pair_keep_out_true_min": (_i, [_vp, _vp, _i, _d, _d, _i] + [_vp] * 8),
    "obtg_pair_keep_out_true_min_dev": (_i, [_vp, _vp, _i, _d, _d, _i] + [_vp] * 8),
    "obtg_pair_keep_out_true_min_jac": (_i, [_vp, _vp, _i, _d, _d, _i] + [_vp] * 9),
    "obtg_pair_keep_out_true_min_jac_dev": (_i, [_vp, _vp, _i, _d, _d, _i] + [_vp] * 9),
    "obtg_pair_keep_out_euclid_true_min": (_i, [_vp, _vp, _i, _d, _d, _i] + [_vp] * 8),
    "obtg_pair_keep_out_euclid_true_min_dev": (_i, [_vp, _vp, _i, _d, _d, _i] + [_vp] * 8),
    "obtg_pair_keep_out_euclid_true_min_jac": (_i, [_vp, _vp, _i, _d, _d, _i] + [_vp] * 9),
    "obtg_pair_keep_out_euclid_true_min_jac_dev": (_i, [_vp, _vp, _i, _d, _d, _i] + [_vp] * 9),
    "obtg_jerk": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_jerk_dev": (_i, [_vp, _vp, _vp, _i, _d, _vp]),
    "obtg_jerk_true_min": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_jerk_true_min_dev": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp]),
    "obtg_jerk_true_min_jac": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_jerk_true_min_jac_dev": (_i, [_vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "obtg_speed_jac": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "obtg_speed_jac_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "obtg_ang_rate_jac": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "obtg_ang_rate_jac_dev": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "obtg_euclidean_grad": (_i, [_vp, _vp, _i, _vp]),
    "obtg_deriv_energy_grad": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "obtg_set_profiling": (_i, [_vp, _i]),
    "obtg_set_profile_period": (_i, [_vp, _i]),
    "obtg_kernel_stats": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(C.c_longlong)]),
    "obtg_reset_kernel_stats": (_i, [_vp]),
    "obtg_kernel_name": (C.c_char_p, [_i]),
}


def abi_symbol_names():
    """The symbols include/obtg.h declares (used by the CPU-side load test)."""
    return sorted(_SIGNATURES)


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so
    (soname libamdhip64.so.7, the same soname /opt/rocm's carries).  If libobtg_hip.so pulled in
    the system copy and torch later loaded its bundled copy, the process would hold two HIP
    runtimes and the second would see no GPU.  Loading torch's copy first (by path, without
    importing torch) makes both libobtg_hip.so (NEEDED libamdhip64.so.7, matched by soname) and
    a later `import torch` (same file) share it.  Without torch installed the system runtime
    is used."""
    if os.environ.get("OBTG_USE_SYSTEM_HIP") == "1":
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return None
    try:
        return C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError:
        return None


_hip_runtime = None


def load():
    """dlopen the in-tree library; loud failure when it has not been built."""
    global _lib, _hip_runtime
    if _lib is not None:
        return _lib
    _hip_runtime = _preload_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libobtg_hip.so is missing (%s). Build it with "
            "`python -m optimalbeziertrajectorygeneration_amd.build`; there is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here == ABI drift between header and library
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def device_count():
    return load().obtg_device_count()


def abi_version():
    return load().obtg_abi_version()


def source_hash(unit="all"):
    """obtg_source_hash: which sources the loaded library was built from (16 hex digits; None for an unknown unit name)."""
    h = load().obtg_source_hash(unit.encode() if unit is not None else None)
    return h.decode() if h is not None else None


def libm_pow_matches():
    """obtg_libm_pow_matches: does this host's pow(x, 2.0) round as the device's restatement of glibc 2.35's does."""
    return bool(load().obtg_libm_pow_matches())


def fast_kernels(dim, deg):
    """obtg_fast_kernels: bit 0 separation / speed rows, bit 1 angular rate + one-launch steps, bit 2 the DEG_ELEV > 0 forms."""
    return load().obtg_fast_kernels(int(dim), int(deg))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def keep_out_features(H, d=None):
    """obtg_keep_out_features: the host geometry of the Euclidean keep-out rows for ONE obstacle, the faces H[F][d+1].  Needs no
    device.  dict(Hn[F][d+1] -- the normalised faces --, idx[n][3] -- the features' faces, -1 padded --, ginv[n][6] -- their
    inverse Gram matrices --, n, rc): rc is OBTG_ERR_UNSUPPORTED with more than 128 features (n the count found, 128 stored)."""
    H = np.ascontiguousarray(H, np.float64)
    if d is None:
        d = H.shape[-1] - 1
    H = H.reshape(-1, d + 1)
    Hn, idx, ginv, n = np.empty_like(H), np.full((128, 3), -1, np.int32), np.zeros((128, 6)), C.c_int(0)
    rc = load().obtg_keep_out_features(_ptr(H), H.shape[0], int(d), _ptr(Hn), _ptr(idx), _ptr(ginv), C.byref(n))
    k = min(max(n.value, 0), 128)
    return dict(Hn=Hn, idx=idx[:k], ginv=ginv[:k], n=n.value, rc=rc)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# -- arguments of the batched pair searches (Context.gjk_pairs .. coll_check2poly), as the C ABI takes them
def _curves_arg(curves):
    """curves[n_curves][3][K] -> (array, n_curves, K)"""
    curves = _f64(curves)
    n_curves, _, K = curves.shape
    return curves, n_curves, K


def _polys_arg(pts, off):
    """-> (pts[n_pts][3], off[n_poly + 1])"""
    return _f64(pts).reshape(-1, 3), _i32(off)


def _pairs_arg(pair_a, pair_b):
    """-> (pair_a, pair_b, n_pairs)"""
    pa, pb = _i32(pair_a), _i32(pair_b)
    return pa, pb, pa.shape[0]


def _search_out(n, width, zeroed=False):
    """Outputs of a curve search over n pairs: res[n][width] (res[n] for width 1), info[n][4], status[n]."""
    shape = n if width == 1 else (n, width)
    return np.zeros(shape) if zeroed else np.empty(shape), np.zeros((n, 4), np.int32), np.zeros(n, np.int32)


def _prefer_torch_rccl():
    """One RCCL per process, as for the HIP runtime: PyTorch bundles a librccl.so; when it is there and the caller has not
    chosen a file, comm.cpp is told to open that one (OBTG_RCCL_LIB) so that obtg_comm_* and torch.distributed share it."""
    if os.environ.get("OBTG_RCCL_LIB"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "librccl.so")
        if os.path.exists(cand):
            os.environ["OBTG_RCCL_LIB"] = cand


class Comm(object):
    """obtg_comm: this process's membership of a group of n_ranks processes, one per GPU (RCCL).  Rank 0 creates the id
    (`Comm.unique_id()`, 128 bytes) and hands it to the others by any means; every rank then constructs its Comm --
    collectively."""

    @staticmethod
    def unique_id():
        _prefer_torch_rccl()
        buf = (C.c_ubyte * 128)()
        rc = load().obtg_comm_unique_id(buf)
        if rc:
            raise ObtgError("obtg_comm_unique_id: %s" % load().obtg_strerror(rc).decode(), rc)
        return bytes(buf)

    def __init__(self, n_ranks, rank, unique_id, device=0):
        _prefer_torch_rccl()
        self._lib = load()
        self._h = _vp()
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        rc = self._lib.obtg_comm_create(C.byref(self._h), int(n_ranks), int(rank), buf, int(device))
        if rc:
            raise ObtgError("obtg_comm_create: %s" % self._lib.obtg_strerror(rc).decode(), rc)
        self.n_ranks, self.rank = int(n_ranks), int(rank)

    def all_gather_dev(self, ctx, d_send, d_recv, bytes_per_rank):
        rc = self._lib.obtg_comm_all_gather_dev(self._h, ctx._h, _vp(d_send), _vp(d_recv), int(bytes_per_rank))
        if rc:
            raise ObtgError("obtg_comm_all_gather_dev: %s (%s)" % (self._lib.obtg_strerror(rc).decode(),
                                                                     (self._lib.obtg_comm_last_error(self._h) or b"").decode()), rc)

    def close(self):
        if self._h:
            self._lib.obtg_comm_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObtgError(RuntimeError):
    """A non-zero return of the C ABI; `.code` is the OBTG_ERR_* value (-5: the shape has no kernel of that kind)."""

    def __init__(self, msg, code=None):
        RuntimeError.__init__(self, msg)
        self.code = code


ERR_UNSUPPORTED = -5


class _PinnedPool(object):
    """Page-locked host blocks for the large result arrays of the host-buffer entry points.

    The device writes such an array by DMA at PCIe rate; a pageable NumPy array would be staged chunk by chunk
    (include/obtg.h, obtg_host_alloc).  Blocks are recycled: pinning costs milliseconds per 100 MB, an SLSQP
    driver asks for the same shapes on every iteration.  An array keeps its block alive through its buffer
    object; when the last view dies the block returns to the pool.  At most `cap` bytes stay cached -- 1 GiB by
    default (two Jacobian-sized result arrays of the 64-vehicle configuration), OBTG_PINNED_CACHE_MB overrides it --
    and `trim()` (module function `pinned_trim`) hands every cached block back to the driver."""

    MIN_BYTES = 1 << 20

    def __init__(self, cap=None):
        if cap is None:
            cap = int(os.environ.get("OBTG_PINNED_CACHE_MB", "1024")) << 20
        self.cap, self.cached, self.free = cap, 0, {}
        self._lock = threading.RLock()       # callers on several threads; re-entrant: a finaliser may run inside empty()

    def trim(self, keep_bytes=0):
        """Free cached blocks (largest first) until at most keep_bytes stay cached; returns the bytes released."""
        released = 0
        with self._lock:
            for size in sorted(self.free, reverse=True):
                blocks = self.free[size]
                while blocks and self.cached > keep_bytes:
                    ptr = blocks.pop()
                    self.cached -= size
                    released += size
                    if _lib is not None:
                        _lib.obtg_host_free(_vp(ptr))
            for size in [k for k, v in self.free.items() if not v]:
                del self.free[size]
        return released

    def _release(self, size, ptr):
        with self._lock:
            if self.cached + size <= self.cap:
                self.free.setdefault(size, []).append(ptr)
                self.cached += size
                return
        if _lib is not None:
            _lib.obtg_host_free(_vp(ptr))

    def empty(self, shape, dtype=np.float64):
        dtype = np.dtype(dtype)
        count = int(np.prod(shape))
        nbytes = count * dtype.itemsize
        if nbytes < self.MIN_BYTES:
            return np.empty(shape, dtype)
        size = 1 << (nbytes - 1).bit_length()
        if size > (1 << 28):                      # above 256 MB: 64 MB granularity instead of powers of two
            size = -(-nbytes // (64 << 20)) * (64 << 20)
        ptr = None
        with self._lock:
            blocks = self.free.get(size)
            if blocks:
                ptr = blocks.pop()
                self.cached -= size
        if ptr is None:
            h = _vp()
            if load().obtg_host_alloc(size, C.byref(h)) != OK or not h.value:
                return np.empty(shape, dtype)     # no pinned memory left: a pageable array still works (staged)
            ptr = h.value
        buf = (C.c_char * nbytes).from_address(ptr)
        weakref.finalize(buf, self._release, size, ptr)
        return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


_pinned = _PinnedPool()


def pinned_trim(keep_bytes=0):
    """Release the page-locked blocks the result-array pool has cached (all of them by default)."""
    return _pinned.trim(keep_bytes)


def pinned_empty(shape, dtype=np.float64):
    """An uninitialised array in page-locked host memory (falls back to np.empty for small sizes)."""
    return _pinned.empty(shape, dtype)


def torch_stream():
    """HIP handle of torch's current stream, for Context.set_stream (0 for torch's default stream, which IS the null
    stream: obtg_ctx_set_stream takes the handle as given, so the library's launches are ordered with torch's own)."""
    import torch
    return torch.cuda.current_stream().cuda_stream


class Context(object):
    """One problem shape on one MI355X: wraps obtg_ctx."""

    def __init__(self, n_veh, dim, deg, deg_elev=0, point_obs=None, device=0):
        self._lib = load()
        self._h = _vp()
        if self._lib.obtg_device_count() <= 0:
            raise ObtgError("no usable gfx950 (MI355X) device: the HIP path is the only compute path")
        obs = None
        n_obs = 0
        if point_obs is not None and len(point_obs) > 0:
            obs = _f64(point_obs).reshape(-1, dim)
            n_obs = obs.shape[0]
        rc = self._lib.obtg_ctx_create(C.byref(self._h), n_veh, dim, deg, deg_elev, n_obs, _ptr(obs), device)
        if rc != OK:
            self._h = _vp()
            raise ObtgError("obtg_ctx_create: " + self._lib.obtg_strerror(rc).decode())
        self.n_veh, self.dim, self.deg, self.deg_elev, self.n_obs = n_veh, dim, deg, deg_elev, n_obs
        self.device = device
        self.n_poly = 0
        self.n_hull_pairs = None      # no hull pair list registered yet
        self.keep_in_items = 0        # (vehicle, face) items of the keep-in region; 0: none set
        self._keep_in_key = None      # the bytes of the tables set_keep_in last sent
        self.keep_out_items = 0       # (vehicle, obstacle) items of the keep-out tables; 0: none set
        self._keep_out_key = None     # the bytes of the tables set_keep_out last sent
        self._keep_out_motion_key = None     # the bytes of the motion set_keep_out_motion last sent; None: none set
        self._pair_keep_out_key = None       # the bytes of the separation region set_pair_keep_out last sent; None: none set
        self.proximity_items = 0      # items of the proximity rows; 0: none set
        self._proximity_key = None    # the bytes of the tables set_proximity last sent

    # -- plumbing
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.obtg_ctx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != OK:
            msg = self._lib.obtg_strerror(rc).decode()
            extra = self._lib.obtg_last_error(self._h)
            if extra:
                msg += " (" + extra.decode() + ")"
            raise ObtgError("%s: %s" % (what, msg), rc)

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr):
        """Every later call goes to this HIP stream, the handle as given: 0 / None = the null stream, i.e. torch's default
        stream (torch.cuda.current_stream().cuda_stream is the right argument whichever stream is current)."""
        self._check(self._lib.obtg_ctx_set_stream(self._h, _vp(stream_ptr or None)), "obtg_ctx_set_stream")

    def use_own_stream(self):
        """Back to the context's private stream (created non-blocking: not ordered with the null stream)."""
        self._check(self._lib.obtg_ctx_use_own_stream(self._h), "obtg_ctx_use_own_stream")

    def set_deg_elev(self, R):
        self._check(self._lib.obtg_ctx_set_deg_elev(self._h, int(R)), "obtg_ctx_set_deg_elev")
        self.deg_elev = int(R)

    def set_ang_rate_order(self, elevate_first):
        """DEG_ELEV > 0: False / 0 (default) = products at degree 4n, then elevation by 4R; True / 1 = the reference's
        order of operations; 2 = the default order plus a double-double recompute of near-stop vehicles' rows
        (include/obtg.h obtg_ctx_set_ang_rate_order)."""
        self._check(self._lib.obtg_ctx_set_ang_rate_order(self._h, int(elevate_first)), "obtg_ctx_set_ang_rate_order")

    def ang_rate_order_in_effect(self):
        """0 / 1 / 2 = the order of operations the angular rate of this shape really runs in (a request for 'exact' or
        'fast' holds only where those kernels exist: include/obtg.h obtg_ctx_ang_rate_order_in_effect)."""
        rc = self._lib.obtg_ctx_ang_rate_order_in_effect(self._h)
        if rc < 0:
            self._check(rc, "obtg_ctx_ang_rate_order_in_effect")
        return rc

    def sync(self):
        self._check(self._lib.obtg_sync(self._h), "obtg_sync")

    @property
    def len_temporal_sep(self):
        return self._lib.obtg_len_temporal_sep(self._h)

    @property
    def len_speed(self):
        return self._lib.obtg_len_speed(self._h)

    @property
    def len_ang_rate(self):
        return self._lib.obtg_len_ang_rate(self._h)

    @property
    def num_pairs(self):
        return self._lib.obtg_num_pairs(self._h)

    def _rows(self, Y):
        Y = _f64(Y)
        per = self.n_veh * self.dim * (self.deg + 1)
        if Y.size % per != 0 or Y.size == 0:
            raise ValueError("Y must hold B x (%d x %d) doubles, got %s" % (self.n_veh * self.dim, self.deg + 1, Y.shape))
        return Y, Y.size // per

    def _tf(self, tf, B):
        return _f64(np.broadcast_to(np.asarray(tf, dtype=np.float64), (B,)))

    # -- host-buffer sweeps
    def temporal_sep(self, Y, max_sep):
        Y, B = self._rows(Y)
        out = pinned_empty((B, self.len_temporal_sep))
        self._check(self._lib.obtg_temporal_sep(self._h, _ptr(Y), B, float(max_sep), _ptr(out)), "obtg_temporal_sep")
        return out

    def temporal_sep_min(self, Y, max_sep, pair_begin=0, pair_count=None):
        """Per pair the smallest of its elevated separation control points minus max_sep^2 (obtg_temporal_sep_min_range):
        [B][pair_count].  A pair whose full row (temporal_sep) has a NaN or +-inf element is NaN, not the minimum of the
        finite rest (include/obtg.h, "Non-finite control points in the REDUCED separation forms")."""
        Y, B = self._rows(Y)
        if pair_count is None:
            pair_count = self.num_pairs - pair_begin
        out = pinned_empty((B, pair_count))
        self._check(self._lib.obtg_temporal_sep_min_range(self._h, _ptr(Y), B, float(max_sep), int(pair_begin),
                                                          int(pair_count), _ptr(out)), "obtg_temporal_sep_min_range")
        return out

    def temporal_sep_active(self, Y, max_sep, k, with_index=False):
        """Per pair its k smallest elevated separation control points, in control-point order (obtg_temporal_sep_active): [B][P * k]
        (and, with_index, the int32 control-point indices of the same shape).  A pair whose full row has a NaN or +-inf
        element: k NaNs with the indices 0 .. k-1 (always indices one can gather with; k = 1 is temporal_sep_min, NaN for NaN)."""
        Y, B = self._rows(Y)
        out = pinned_empty((B, self.num_pairs * int(k)))
        idx = np.empty((B, self.num_pairs * int(k)), np.int32) if with_index else None
        self._check(self._lib.obtg_temporal_sep_active(self._h, _ptr(Y), B, float(max_sep), int(k), _ptr(out), _ptr(idx)),
                    "obtg_temporal_sep_active")
        return (out, idx) if with_index else out

    def _true_min(self, name, items, Y, tf, lead, eps_rel, max_nodes, *blocks):
        """The allocation, the call and the dict of the true-minimum host calls, `items` values per row (an int, or the
        trailing shape of a row's values): obtg_<family>(Y[, tf], B, *lead, eps_rel, max_nodes, val, t_star, status[, jac[,
        jac_tf]]); blocks names the last two."""
        Y, B = self._rows(Y)
        ops = [Y] if tf is None else [Y, self._tf(tf, B)]
        shape = (B,) + (tuple(items) if isinstance(items, tuple) else (items,))
        r = dict(val=pinned_empty(shape), t_star=np.empty(shape), status=np.zeros(shape, np.int32))
        if "jac" in blocks:
            r["jac"] = pinned_empty(shape + (self.dim, self.deg + 1))
        if "jac_tf" in blocks:
            r["jac_tf"] = np.empty(shape)
        self._check(getattr(self._lib, name)(self._h, *[_ptr(a) for a in ops], B, *lead, float(eps_rel), int(max_nodes),
                                             *[_ptr(a) for a in r.values()]), name)
        return r

    def temporal_sep_true_min(self, Y, max_sep, eps_rel=1e-9, max_nodes=100000):
        """Per pair the true minimum over t in [0, 1] of the squared-separation polynomial minus max_sep^2
        (obtg_temporal_sep_true_min; DEG_ELEV does not enter): dict(val[B][P], t_star[B][P] -- where it is taken --,
        status[B][P] as MD_*).  val - (the search's lower bound) <= eps_rel x the pair's largest coefficient."""
        return self._true_min("obtg_temporal_sep_true_min", self.num_pairs, Y, None, (float(max_sep),), eps_rel, max_nodes)

    def _true_min_dev(self, name, ops, B, lead, eps_rel, max_nodes, d_out, d_t_star, d_status, *d_blocks):
        """The device-pointer form of the same calls: obtg_<family>_dev(*ops, B, *lead, eps_rel, max_nodes, d_out, d_t_star,
        d_status[, d_jac[, d_jac_tf]]) -- ops: dY[, d_tf]; d_blocks: the last two, in the ABI's order."""
        self._check(getattr(self._lib, name)(self._h, *[_vp(p) for p in ops], int(B), *lead, float(eps_rel), int(max_nodes),
                                             *[_vp(p) for p in (d_out, d_t_star, d_status) + d_blocks]), name)

    def _vehicle_rows(self, name, Y, tf, lead, shape):
        """The allocation and the call of the per-vehicle host row calls: obtg_<family>(Y, tf, B, *lead, out[B] + shape)."""
        Y, B = self._rows(Y)
        tf = self._tf(tf, B)
        out = pinned_empty((B,) + shape)
        self._check(getattr(self._lib, name)(self._h, _ptr(Y), _ptr(tf), B, *lead, _ptr(out)), name)
        return out

    def temporal_sep_true_min_dev(self, dY, B, max_sep, d_out, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_temporal_sep_true_min_dev", (dY,), B, (float(max_sep),), eps_rel, max_nodes, d_out, d_t_star, d_status)

    def temporal_sep_true_min_jac(self, Y, max_sep, eps_rel=1e-9, max_nodes=100000):
        """temporal_sep_true_min with its envelope Jacobian (obtg_temporal_sep_true_min_jac): dict(val, t_star, status -- the
        bits of temporal_sep_true_min --, jac[B][P][dim][deg+1]: d/d(control points of the pair's first object) of the pair's
        polynomial at t_star; the second object's block is the negation, an obstacle has no variable)."""
        return self._true_min("obtg_temporal_sep_true_min_jac", self.num_pairs, Y, None, (float(max_sep),), eps_rel, max_nodes, "jac")

    def temporal_sep_true_min_jac_dev(self, dY, B, max_sep, d_out, d_jac, d_t_star=None, d_status=None, eps_rel=1e-9,
                                      max_nodes=100000):
        self._true_min_dev("obtg_temporal_sep_true_min_jac_dev", (dY,), B, (float(max_sep),), eps_rel, max_nodes, d_out, d_t_star,
                           d_status, d_jac)

    def bern_extrema(self, c, want_max=False, eps_rel=1e-9, eps_abs=0.0, max_nodes=100000):
        """True minimum (want_max: maximum) over [0, 1] of every row of Bernstein coefficients c[M][K], K <= 64
        (obtg_bern_extrema): dict(val, t_star, bound, nodes, status) with bound <= min p <= val and, where status is MD_OK,
        val - bound <= max(eps_abs, eps_rel * max |c_k|)."""
        c = _f64(c)
        if c.ndim == 1:
            c = c[None]
        M, K = c.shape
        val, t_star, bound = np.empty(M), np.empty(M), np.empty(M)
        nodes, status = np.zeros(M, np.int32), np.zeros(M, np.int32)
        self._check(self._lib.obtg_bern_extrema(self._h, _ptr(c), M, K, int(bool(want_max)), float(eps_rel), float(eps_abs),
                                                int(max_nodes), _ptr(val), _ptr(t_star), _ptr(bound), _ptr(nodes), _ptr(status)),
                    "obtg_bern_extrema")
        return dict(val=val, t_star=t_star, bound=bound, nodes=nodes, status=status)

    def bern_extrema_dev(self, d_c, M, K, d_val, d_t_star=None, d_bound=None, d_nodes=None, d_status=None, want_max=False,
                         eps_rel=1e-9, eps_abs=0.0, max_nodes=100000):
        self._check(self._lib.obtg_bern_extrema_dev(self._h, _vp(d_c), int(M), int(K), int(bool(want_max)), float(eps_rel),
                                                    float(eps_abs), int(max_nodes), _vp(d_val), _vp(d_t_star), _vp(d_bound),
                                                    _vp(d_nodes), _vp(d_status)), "obtg_bern_extrema_dev")

    def temporal_sep_active_dev(self, dY, B, max_sep, k, d_out_val, d_out_idx=None, pair_begin=0, pair_count=None):
        if pair_count is None:
            pair_count = self.num_pairs - pair_begin
        self._check(self._lib.obtg_temporal_sep_active_dev(self._h, _vp(dY), B, float(max_sep), int(k), pair_begin, pair_count,
                                                           _vp(d_out_val), _vp(d_out_idx)), "obtg_temporal_sep_active_dev")

    def temporal_sep_fd_min_rows_dev(self, dY0, n_fixed_cols, h, row_begin, n_rows, max_sep, d_out):
        """Per finite-difference row only the minima of the pairs its vehicle touches: d_out[n_rows][n_obj - 1]
        (obtg_temporal_sep_fd_min_rows_dev).  NaN for a pair with a non-finite element, as temporal_sep_min_dev inside the view."""
        self._check(self._lib.obtg_temporal_sep_fd_min_rows_dev(self._h, _vp(dY0), int(n_fixed_cols), float(h), int(row_begin),
                                                                int(n_rows), float(max_sep), _vp(d_out)),
                    "obtg_temporal_sep_fd_min_rows_dev")

    # ---- pair partition + collective behind the C ABI (include/obtg.h obtg_comm_*)
    def pair_block(self, n_ranks, rank):
        b, c = _i(0), _i(0)
        self._check(self._lib.obtg_pair_block(self._h, int(n_ranks), int(rank), C.byref(b), C.byref(c)), "obtg_pair_block")
        return b.value, c.value

    def unpack_pair_blocks_dev(self, d_blocks, B, n_ranks, d_rows):
        self._check(self._lib.obtg_unpack_pair_blocks_dev(self._h, _vp(d_blocks), int(B), int(n_ranks), _vp(d_rows)),
                    "obtg_unpack_pair_blocks_dev")

    def temporal_sep_min_gather_dev(self, comm, dY, B, max_sep, d_min_all):
        """This rank's block of the per-pair minima + ONE RCCL all-gather on the context's stream: d_min_all[B][P] on every
        rank (obtg_temporal_sep_min_gather_dev)."""
        rc = self._lib.obtg_temporal_sep_min_gather_dev(self._h, comm._h, _vp(dY), int(B), float(max_sep), _vp(d_min_all))
        if rc:
            raise ObtgError("obtg_temporal_sep_min_gather_dev: %s (%s)" % (self._lib.obtg_strerror(rc).decode(),
                            (self._lib.obtg_comm_last_error(comm._h) or self._lib.obtg_last_error(self._h) or b"").decode()), rc)

    def speed(self, Y, tf, bound, is_max):
        return self._vehicle_rows("obtg_speed", Y, tf, (float(bound), int(bool(is_max))), (self.len_speed,))

    def speed_true_min(self, Y, tf, bound, is_max, eps_rel=1e-9, max_nodes=100000):
        """Per vehicle the true minimum over t in [0, 1] of the speed row's polynomial sign (d/2)|v'|^2 + offset -- the polynomial
        speed(Y, tf, bound, is_max) holds the control points of (obtg_speed_true_min; DEG_ELEV does not enter):
        dict(val[B][N], t_star[B][N], status[B][N] as MD_*)."""
        return self._true_min("obtg_speed_true_min", self.n_veh, Y, tf, (float(bound), int(bool(is_max))), eps_rel, max_nodes)

    def speed_true_min_dev(self, dY, d_tf, B, bound, is_max, d_out, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_speed_true_min_dev", (dY, d_tf), B, (float(bound), int(bool(is_max))), eps_rel, max_nodes, d_out,
                           d_t_star, d_status)

    def speed_true_min_jac(self, Y, tf, bound, is_max, eps_rel=1e-9, max_nodes=100000):
        """speed_true_min with its envelope Jacobian (obtg_speed_true_min_jac): dict(val, t_star, status -- the bits of
        speed_true_min --, jac[B][N][dim][deg+1]: d/d(the vehicle's own control points) of its polynomial at t_star,
        jac_tf[B][N]: d/dtf at fixed control points)."""
        return self._true_min("obtg_speed_true_min_jac", self.n_veh, Y, tf, (float(bound), int(bool(is_max))), eps_rel, max_nodes,
                              "jac", "jac_tf")

    def speed_true_min_jac_dev(self, dY, d_tf, B, bound, is_max, d_out, d_jac, d_jac_tf=None, d_t_star=None, d_status=None,
                               eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_speed_true_min_jac_dev", (dY, d_tf), B, (float(bound), int(bool(is_max))), eps_rel, max_nodes,
                           d_out, d_t_star, d_status, d_jac, d_jac_tf)

    def accel(self, Y, tf, bound):
        """The acceleration-bound rows (obtg_accel): [B][N * (2 deg + DEG_ELEV + 1)] control points of
        bound**2 - (d/2)|c''|^2, c'' = diff().diff() of the vehicle's curve on a span of tf."""
        return self._vehicle_rows("obtg_accel", Y, tf, (float(bound),), (self.len_speed,))

    def accel_dev(self, dY, d_tf, B, bound, d_out):
        self._check(self._lib.obtg_accel_dev(self._h, _vp(dY), _vp(d_tf), int(B), float(bound), _vp(d_out)), "obtg_accel_dev")

    def accel_true_min(self, Y, tf, bound, eps_rel=1e-9, max_nodes=100000):
        """Per vehicle the true minimum over t in [0, 1] of bound**2 - (d/2)|c''|^2 -- the polynomial accel(Y, tf, bound) holds
        the control points of (obtg_accel_true_min; DEG_ELEV does not enter): dict(val[B][N], t_star[B][N], status[B][N])."""
        return self._true_min("obtg_accel_true_min", self.n_veh, Y, tf, (float(bound),), eps_rel, max_nodes)

    def accel_true_min_dev(self, dY, d_tf, B, bound, d_out, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_accel_true_min_dev", (dY, d_tf), B, (float(bound),), eps_rel, max_nodes, d_out, d_t_star, d_status)

    def accel_true_min_jac(self, Y, tf, bound, eps_rel=1e-9, max_nodes=100000):
        """accel_true_min with its envelope Jacobian (obtg_accel_true_min_jac): dict(val, t_star, status -- the bits of
        accel_true_min --, jac[B][N][dim][deg+1]: d/d(the vehicle's own control points) of its polynomial at t_star,
        jac_tf[B][N]: d/dtf at fixed control points)."""
        return self._true_min("obtg_accel_true_min_jac", self.n_veh, Y, tf, (float(bound),), eps_rel, max_nodes, "jac", "jac_tf")

    def accel_true_min_jac_dev(self, dY, d_tf, B, bound, d_out, d_jac, d_jac_tf=None, d_t_star=None, d_status=None,
                               eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_accel_true_min_jac_dev", (dY, d_tf), B, (float(bound),), eps_rel, max_nodes, d_out, d_t_star,
                           d_status, d_jac, d_jac_tf)

    # -- keep-in regions (include/obtg.h "keep-in regions"): region = (H[F][dim+1], VF[P][2]); every call below takes it as its
    # optional `region` operand -- sent to the context only when its bytes differ from what the context holds -- or, with None,
    # works on the region set_keep_in left there
    def set_keep_in(self, H, VF):
        """obtg_ctx_set_keep_in: F half-spaces a . p <= b as rows (a, b) of H and the (vehicle, face) items VF; an empty VF
        clears the region."""
        VF = _i32(VF).reshape(-1, 2)
        H = _f64(H).reshape(-1, self.dim + 1)
        self._check(self._lib.obtg_ctx_set_keep_in(self._h, _ptr(H), H.shape[0], _ptr(VF), VF.shape[0]), "obtg_ctx_set_keep_in")
        self.keep_in_items = VF.shape[0]
        self._keep_in_key = (H.tobytes(), VF.tobytes())

    def _keep_in(self, region):
        if region is not None:
            H, VF = _f64(region[0]), _i32(region[1])
            if self._keep_in_key != (H.tobytes(), VF.tobytes()):
                self.set_keep_in(H, VF)
        return self.keep_in_items          # (0: no region -- the library's call answers OBTG_ERR_ARG)

    @property
    def len_keep_in(self):
        return self._lib.obtg_len_keep_in(self._h)

    def keep_in(self, Y, region=None):
        """The keep-in rows (obtg_keep_in): [B][P * (deg + DEG_ELEV + 1)] control points of b_f - a_f . c_v per (vehicle,
        face) item -- exact linear constraints on the control points."""
        self._keep_in(region)
        Y, B = self._rows(Y)
        out = pinned_empty((B, self.len_keep_in))
        self._check(self._lib.obtg_keep_in(self._h, _ptr(Y), B, _ptr(out)), "obtg_keep_in")
        return out

    def keep_in_dev(self, dY, B, d_out):
        self._check(self._lib.obtg_keep_in_dev(self._h, _vp(dY), int(B), _vp(d_out)), "obtg_keep_in_dev")

    def keep_in_true_min(self, Y, region=None, eps_rel=1e-9, max_nodes=100000):
        """Per item the true margin, the minimum over t in [0, 1] of b_f - a_f . c_v(t) (obtg_keep_in_true_min; DEG_ELEV does
        not enter): dict(val[B][P], t_star[B][P], status[B][P])."""
        return self._true_min("obtg_keep_in_true_min", self._keep_in(region), Y, None, (), eps_rel, max_nodes)

    def keep_in_true_min_dev(self, dY, B, d_out, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_keep_in_true_min_dev", (dY,), B, (), eps_rel, max_nodes, d_out, d_t_star, d_status)

    def keep_in_true_min_jac(self, Y, region=None, eps_rel=1e-9, max_nodes=100000):
        """keep_in_true_min with its envelope Jacobian (obtg_keep_in_true_min_jac): dict(val, t_star, status -- the bits of
        keep_in_true_min --, jac[B][P][dim][deg+1] = -a_f[c] B_i(t_star): d/d(the item's own vehicle's control points))."""
        return self._true_min("obtg_keep_in_true_min_jac", self._keep_in(region), Y, None, (), eps_rel, max_nodes, "jac")

    def keep_in_true_min_jac_dev(self, dY, B, d_out, d_jac, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_keep_in_true_min_jac_dev", (dY,), B, (), eps_rel, max_nodes, d_out, d_t_star, d_status, d_jac)

    # -- keep-out obstacles (include/obtg.h "keep-out obstacles"): obstacles = (H[F][dim+1], obs_off[O+1], VO[P][2]); every call
    # below takes them as its optional `obstacles` operand -- sent to the context only when their bytes differ from what the
    # context holds -- or, with None, works on the tables set_keep_out left there
    # -- proximity rows ("come close", "stay close": DESIGN.md 4.28).  The same shape as keep-in's: `tables` is (items[P][3],
    # params[P][3], points[Q][dim]) to set first when it differs from what the context holds, or None: the call works on the
    # tables set_proximity left there
    def set_proximity(self, items, params, points=None):
        """obtg_ctx_set_proximity: items (a, b, kind) -- vehicle a against vehicle b < n_veh or point b - n_veh of `points`, kind
        PROX_WITHIN (the minimum of g over the window) or PROX_REACH (the maximum) -- and params (rho, tau0, tau1), the Euclidean
        radius and the window of the normalised parameter; an empty list clears the tables."""
        items = np.ascontiguousarray(np.asarray(items, dtype=np.int32).reshape(-1, 3))
        params = _f64(np.asarray(params, dtype=np.float64).reshape(-1, 3))
        points = _f64(np.zeros((0, self.dim)) if points is None else np.asarray(points, dtype=np.float64).reshape(-1, self.dim))
        if items.shape[0] != params.shape[0]:
            raise ValueError("proximity items and params must have one row per item, got %d and %d" % (items.shape[0], params.shape[0]))
        self._check(self._lib.obtg_ctx_set_proximity(self._h, _ptr(items), _ptr(params), _ptr(points) if points.size else None,
                                                     items.shape[0], points.shape[0]), "obtg_ctx_set_proximity")
        self.proximity_items = items.shape[0]
        self._proximity_key = (items.tobytes(), params.tobytes(), points.tobytes())

    def _proximity(self, tables):
        if tables is not None:
            items, params, points = tables
            items = np.ascontiguousarray(np.asarray(items, dtype=np.int32).reshape(-1, 3))
            params = _f64(np.asarray(params, dtype=np.float64).reshape(-1, 3))
            points = _f64(np.asarray(points, dtype=np.float64).reshape(-1, self.dim))
            if self._proximity_key != (items.tobytes(), params.tobytes(), points.tobytes()):
                self.set_proximity(items, params, points)
        return self.proximity_items        # (0: no items -- the library's call answers OBTG_ERR_ARG)

    @property
    def len_proximity(self):
        return self._lib.obtg_len_proximity(self._h)

    def proximity_poly(self, Y, tables=None):
        """g's Bernstein coefficients per item (obtg_proximity_poly): [B][P][2 deg + 1], g = (dim/2)(rho^2 - |c_a - c_b|^2) on the
        item's window, un-negated for both kinds."""
        P = self._proximity(tables)
        Y, B = self._rows(Y)
        out = pinned_empty((B, P, 2 * self.deg + 1))
        self._check(self._lib.obtg_proximity_poly(self._h, _ptr(Y), B, _ptr(out)), "obtg_proximity_poly")
        return out

    def proximity_poly_dev(self, dY, B, d_out):
        self._check(self._lib.obtg_proximity_poly_dev(self._h, _vp(dY), int(B), _vp(d_out)), "obtg_proximity_poly_dev")

    def _proximity_true(self, name, Y, tables, eps_rel, max_nodes, jac):
        P = self._proximity(tables)
        Y, B = self._rows(Y)
        r = dict(val=pinned_empty((B, P)), t_star=np.empty((B, P)), bound=np.empty((B, P)), nodes=np.zeros((B, P), np.int32),
                 status=np.zeros((B, P), np.int32))
        if jac:
            r["jac"] = pinned_empty((B, P, self.dim, self.deg + 1))
        self._check(getattr(self._lib, name)(self._h, _ptr(Y), B, float(eps_rel), int(max_nodes), *[_ptr(a) for a in r.values()]), name)
        return r

    def proximity_true(self, Y, tables=None, eps_rel=1e-9, max_nodes=100000):
        """Per item the certified extremum of g over its window (obtg_proximity_true): dict(val[B][P] -- the value attained at
        t_star[B][P], the curve's parameter --, bound[B][P] closing the bracket on the other side, nodes[B][P], status[B][P] as
        MD_*).  A `within` row is the minimum (>= 0: the pair never leaves range), a `reach` row the maximum (>= 0: it comes
        within rho at some time)."""
        return self._proximity_true("obtg_proximity_true", Y, tables, eps_rel, max_nodes, False)

    def proximity_true_jac(self, Y, tables=None, eps_rel=1e-9, max_nodes=100000):
        """proximity_true with its envelope Jacobian (obtg_proximity_true_jac): the same outputs with the same bits, and
        jac[B][P][dim][deg+1] = -dim B_i(t_star) (c_a - c_b)(t_star): d/d(a's control points); a second vehicle's block is the
        negation, a point has none."""
        return self._proximity_true("obtg_proximity_true_jac", Y, tables, eps_rel, max_nodes, True)

    def proximity_true_dev(self, dY, B, d_val, d_t_star=None, d_bound=None, d_nodes=None, d_status=None, d_jac=None, eps_rel=1e-9,
                           max_nodes=100000):
        """The device-pointer form (obtg_proximity_true_dev; with d_jac: obtg_proximity_true_jac_dev)."""
        name = "obtg_proximity_true_jac_dev" if d_jac is not None else "obtg_proximity_true_dev"
        tail = (d_jac,) if d_jac is not None else ()
        self._check(getattr(self._lib, name)(self._h, _vp(dY), int(B), float(eps_rel), int(max_nodes),
                                             *[_vp(p) for p in (d_val, d_t_star, d_bound, d_nodes, d_status) + tail]), name)

    def set_keep_out(self, H, obs_off, VO):
        """obtg_ctx_set_keep_out: the faces a . p <= b of every obstacle as rows (a, b) of H, obstacle o owning rows
        obs_off[o] .. obs_off[o+1]-1, and the (vehicle, obstacle) items VO; an empty VO clears the tables."""
        VO = _i32(VO).reshape(-1, 2)
        H = _f64(H).reshape(-1, self.dim + 1)
        obs_off = _i32(obs_off).reshape(-1)
        self._check(self._lib.obtg_ctx_set_keep_out(self._h, _ptr(H), _ptr(obs_off), max(obs_off.shape[0] - 1, 0), _ptr(VO),
                                                    VO.shape[0]), "obtg_ctx_set_keep_out")
        self.keep_out_items = VO.shape[0]
        self._keep_out_key = (H.tobytes(), obs_off.tobytes(), VO.tobytes())
        self._keep_out_motion_key = None       # (the library clears the motion with the tables)

    def _keep_out(self, obstacles):
        if obstacles is not None:
            H, off, VO = _f64(obstacles[0]), _i32(obstacles[1]), _i32(obstacles[2])
            if self._keep_out_key != (H.tobytes(), off.tobytes(), VO.tobytes()):
                self.set_keep_out(H, off, VO)
        return self.keep_out_items         # (0: no tables -- the library's call answers OBTG_ERR_ARG)

    @property
    def len_keep_out(self):
        return self._lib.obtg_len_keep_out(self._h)

    def _keep_out_call(self, name, P, Y, margin, eps_rel, max_nodes, jac, tf=None, euclid=False, rel=False):
        """The one host caller of the keep-out family: P items per row; tf: the moving forms' spans (they return jac_tf beside
        jac); euclid: faces[.][3] and dir[.][dim] in the place of face[.][2] and lam; rel: the forms that return the relative
        control points.  The dict's order is the order of the library's arguments."""
        Y, B = self._rows(Y)
        lead = (_ptr(Y),)
        if tf is not None:
            tf = np.ascontiguousarray(np.broadcast_to(_f64(tf).reshape(-1), (B,)))
            lead += (_ptr(tf),)
        block = (B, P, self.dim, self.deg + 1)
        r = dict(val=pinned_empty((B, P)), t_star=np.empty((B, P)))
        if euclid:
            r.update(faces=np.zeros((B, P, 3), np.int32), dir=np.empty((B, P, self.dim)))
        else:
            r.update(face=np.zeros((B, P, 2), np.int32), lam=np.empty((B, P)))
        r.update(bound=np.empty((B, P)), nodes=np.zeros((B, P), np.int32), status=np.zeros((B, P), np.int32))
        if rel:
            r["rel"] = np.empty(block)
        if jac:
            r["jac"] = pinned_empty(block)
            if tf is not None:
                r["jac_tf"] = np.empty((B, P))
        self._check(getattr(self._lib, name)(self._h, *lead, B, float(margin), float(eps_rel), int(max_nodes),
                                             *[_ptr(a) for a in r.values()]), name)
        return r

    def _keep_out_call_dev(self, name, lead, B, margin, eps_rel, max_nodes, outs):
        self._check(getattr(self._lib, name)(self._h, *[_vp(q) for q in lead], int(B), float(margin), float(eps_rel), int(max_nodes),
                                             *[_vp(q) for q in outs]), name)

    def _bern_keep_out(self, name, c, H, eps_rel, max_nodes, moving=False, Q=None, r=None):
        """The one caller of the free-curve forms; moving: Q is the obstacle's offset curve, r[M] or None the curves' ratios."""
        c = _f64(c)
        if c.ndim == 2:
            c = c[None]
        M, dim, K = c.shape
        H = _f64(H).reshape(-1, dim + 1)
        motion = ()
        if moving:
            Q = _f64(Q).reshape(dim, -1)
            if r is not None:
                r = np.ascontiguousarray(np.broadcast_to(_f64(r).reshape(-1), (M,)))
            motion = (_ptr(Q), Q.shape[1], None if r is None else _ptr(r))
        out = dict(val=np.empty(M), t_star=np.empty(M), status=np.zeros(M, np.int32))
        self._check(getattr(self._lib, name)(self._h, _ptr(c), M, dim, K, _ptr(H), H.shape[0], *motion, float(eps_rel), int(max_nodes),
                                             *[_ptr(a) for a in out.values()]), name)
        return out

    def _bern_keep_out_dev(self, name, d_c, M, dim, K, H, eps_rel, max_nodes, d_val, d_t_star, d_status, moving=False, Q=None, d_r=None):
        H = _f64(H).reshape(-1, int(dim) + 1)
        motion = ()
        if moving:
            Q = _f64(Q).reshape(int(dim), -1)
            motion = (_ptr(Q), Q.shape[1], _vp(d_r))
        self._check(getattr(self._lib, name)(self._h, _vp(d_c), int(M), int(dim), int(K), _ptr(H), H.shape[0], *motion, float(eps_rel),
                                             int(max_nodes), _vp(d_val), _vp(d_t_star), _vp(d_status)), name)

    def keep_out_true_min(self, Y, obstacles=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """Per (vehicle, obstacle) item the clearance row: the minimum over t in [0, 1] of the largest a_f . c_v(t) - b_f over
        the obstacle's faces, minus margin (obtg_keep_out_true_min): dict(val[B][P], t_star[B][P], face[B][P][2] -- the
        active faces as indices into H, the second -1 without one --, lam[B][P] -- the first face's weight --, bound[B][P] --
        the certified lower bound --, nodes[B][P], status[B][P])."""
        return self._keep_out_call("obtg_keep_out_true_min", self._keep_out(obstacles), Y, margin, eps_rel, max_nodes, False)

    def keep_out_true_min_jac(self, Y, obstacles=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """keep_out_true_min with its envelope Jacobian (obtg_keep_out_true_min_jac): the same dict, bit for bit, and
        jac[B][P][dim][deg+1] = (lam a_f1[c] + (1 - lam) a_f2[c]) B_i(t_star): d/d(the item's own vehicle's control points)."""
        return self._keep_out_call("obtg_keep_out_true_min_jac", self._keep_out(obstacles), Y, margin, eps_rel, max_nodes, True)

    def keep_out_true_min_dev(self, dY, B, d_out, d_t_star=None, d_face=None, d_lam=None, d_bound=None, d_nodes=None, d_status=None,
                              margin=0.0, eps_rel=1e-9, max_nodes=100000):
        self._keep_out_call_dev("obtg_keep_out_true_min_dev", (dY,), B, margin, eps_rel, max_nodes,
                                (d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status))

    def keep_out_true_min_jac_dev(self, dY, B, d_out, d_jac, d_t_star=None, d_face=None, d_lam=None, d_bound=None, d_nodes=None,
                                  d_status=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        self._keep_out_call_dev("obtg_keep_out_true_min_jac_dev", (dY,), B, margin, eps_rel, max_nodes,
                                (d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, d_jac))

    def bern_keep_out(self, c, H, eps_rel=1e-9, max_nodes=100000):
        """The clearance of free curves c[M][dim][K] (dim 2 or 3, 2 <= K <= 32, whatever the context's shape is) from ONE
        convex obstacle, the faces H[F][dim+1] (obtg_bern_keep_out): dict(val[M], t_star[M], status[M])."""
        return self._bern_keep_out("obtg_bern_keep_out", c, H, eps_rel, max_nodes)

    def bern_keep_out_dev(self, d_c, M, dim, K, H, d_val, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._bern_keep_out_dev("obtg_bern_keep_out_dev", d_c, M, dim, K, H, eps_rel, max_nodes, d_val, d_t_star, d_status)

    # -- the Euclidean metric (include/obtg.h "Euclidean keep-out clearance"): the same tables, the signed Euclidean distance
    def keep_out_euclid_true_min(self, Y, obstacles=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """Per (vehicle, obstacle) item the Euclidean clearance row: the minimum over t in [0, 1] of the signed Euclidean
        distance from c_v(t) to the obstacle, minus margin (obtg_keep_out_euclid_true_min): dict(val[B][P], t_star[B][P],
        faces[B][P][3] -- the active set as indices into H, -1 padded --, dir[B][P][dim] -- the unit direction at t_star --,
        bound[B][P], nodes[B][P], status[B][P])."""
        return self._keep_out_call("obtg_keep_out_euclid_true_min", self._keep_out(obstacles),
                                   Y, margin, eps_rel, max_nodes, False, euclid=True)

    def keep_out_euclid_true_min_jac(self, Y, obstacles=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """keep_out_euclid_true_min with its envelope Jacobian (obtg_keep_out_euclid_true_min_jac): the same dict, bit for bit,
        and jac[B][P][dim][deg+1] = dir[c] B_i(t_star): d/d(the item's own vehicle's control points)."""
        return self._keep_out_call("obtg_keep_out_euclid_true_min_jac", self._keep_out(obstacles),
                                   Y, margin, eps_rel, max_nodes, True, euclid=True)

    def keep_out_euclid_true_min_dev(self, dY, B, d_out, d_t_star=None, d_faces=None, d_dir=None, d_bound=None, d_nodes=None,
                                     d_status=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        self._keep_out_call_dev("obtg_keep_out_euclid_true_min_dev", (dY,), B, margin, eps_rel, max_nodes,
                                (d_out, d_t_star, d_faces, d_dir, d_bound, d_nodes, d_status))

    def keep_out_euclid_true_min_jac_dev(self, dY, B, d_out, d_jac, d_t_star=None, d_faces=None, d_dir=None, d_bound=None, d_nodes=None,
                                         d_status=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        self._keep_out_call_dev("obtg_keep_out_euclid_true_min_jac_dev", (dY,), B, margin, eps_rel, max_nodes,
                                (d_out, d_t_star, d_faces, d_dir, d_bound, d_nodes, d_status, d_jac))

    def bern_keep_out_euclid(self, c, H, eps_rel=1e-9, max_nodes=100000):
        """The Euclidean clearance of free curves c[M][dim][K] from ONE convex obstacle, the raw faces H[F][dim+1]
        (obtg_bern_keep_out_euclid): dict(val[M], t_star[M], status[M])."""
        return self._bern_keep_out("obtg_bern_keep_out_euclid", c, H, eps_rel, max_nodes)

    def bern_keep_out_euclid_dev(self, d_c, M, dim, K, H, d_val, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._bern_keep_out_dev("obtg_bern_keep_out_euclid_dev", d_c, M, dim, K, H, eps_rel, max_nodes, d_val, d_t_star, d_status)

    # -- moving keep-out obstacles (include/obtg.h "moving keep-out obstacles"): motion = (Q, q_off[O+1], T[O]) -- Q the
    # obstacles' [dim][m_o+1] control-point blocks one after the other, flat; q_off in control points, an empty run for an
    # obstacle that stands still -- sent like `obstacles`, only when its bytes differ from what the context holds
    def set_keep_out_motion(self, Q, q_off, T):
        """obtg_ctx_set_keep_out_motion: the offset curves of the keep-out tables' obstacles; an empty q_off clears them."""
        Q, q_off, T = _f64(Q).reshape(-1), _i32(q_off).reshape(-1), _f64(T).reshape(-1)
        self._check(self._lib.obtg_ctx_set_keep_out_motion(self._h, _ptr(Q), _ptr(q_off), _ptr(T), max(q_off.shape[0] - 1, 0)),
                    "obtg_ctx_set_keep_out_motion")
        self._keep_out_motion_key = (Q.tobytes(), q_off.tobytes(), T.tobytes()) if q_off.shape[0] > 1 else None

    def _keep_out_motion(self, obstacles, motion):
        P = self._keep_out(obstacles)
        if motion is not None:
            Q, q_off, T = _f64(motion[0]).reshape(-1), _i32(motion[1]).reshape(-1), _f64(motion[2]).reshape(-1)
            if self._keep_out_motion_key != (Q.tobytes(), q_off.tobytes(), T.tobytes()):
                self.set_keep_out_motion(Q, q_off, T)
        return P

    def keep_out_moving_true_min(self, Y, tf, obstacles=None, motion=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """keep_out_true_min against obstacles that translate along Bezier offsets (obtg_keep_out_moving_true_min): per
        (vehicle, obstacle) item the static row of the relative curve c_v(s) - q_o(s tf), tf[B] the rows' spans.  The dict of
        keep_out_true_min and rel[B][P][dim][deg+1], the relative control points the search ran on."""
        return self._keep_out_call("obtg_keep_out_moving_true_min", self._keep_out_motion(obstacles, motion), Y, margin, eps_rel, max_nodes,
                                   False, tf=_f64(tf), rel=True)

    def keep_out_moving_true_min_jac(self, Y, tf, obstacles=None, motion=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """keep_out_moving_true_min with its envelope Jacobian (obtg_keep_out_moving_true_min_jac): the same dict, bit for bit,
        jac[B][P][dim][deg+1] (d/d the item's own vehicle's control points) and jac_tf[B][P], the explicit d/dtf."""
        return self._keep_out_call("obtg_keep_out_moving_true_min_jac", self._keep_out_motion(obstacles, motion), Y, margin, eps_rel,
                                   max_nodes, True, tf=_f64(tf), rel=True)

    def keep_out_moving_true_min_dev(self, dY, d_tf, B, d_out, d_t_star=None, d_face=None, d_lam=None, d_bound=None, d_nodes=None,
                                     d_status=None, d_rel=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        self._keep_out_call_dev("obtg_keep_out_moving_true_min_dev", (dY, d_tf), B, margin, eps_rel, max_nodes,
                                (d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, d_rel))

    def keep_out_moving_true_min_jac_dev(self, dY, d_tf, B, d_out, d_jac, d_jac_tf, d_t_star=None, d_face=None, d_lam=None, d_bound=None,
                                         d_nodes=None, d_status=None, d_rel=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        self._keep_out_call_dev("obtg_keep_out_moving_true_min_jac_dev", (dY, d_tf), B, margin, eps_rel, max_nodes,
                                (d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, d_rel, d_jac, d_jac_tf))

    def bern_keep_out_moving(self, c, H, Q, r=None, eps_rel=1e-9, max_nodes=100000):
        """The clearance of free curves c[M][dim][K] from ONE convex obstacle H[F][dim+1] that moves by the offset curve
        Q[dim][Km], Km <= K; r[M]: the part [0, r] of the motion's parameter each curve spans (None: 1)
        (obtg_bern_keep_out_moving): dict(val[M], t_star[M], status[M])."""
        return self._bern_keep_out("obtg_bern_keep_out_moving", c, H, eps_rel, max_nodes, moving=True, Q=Q, r=r)

    def bern_keep_out_moving_dev(self, d_c, M, dim, K, H, Q, d_val, d_r=None, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._bern_keep_out_dev("obtg_bern_keep_out_moving_dev", d_c, M, dim, K, H, eps_rel, max_nodes, d_val, d_t_star, d_status,
                                moving=True, Q=Q, d_r=d_r)

    # -- polytopic vehicle-to-vehicle separation (include/obtg.h): ONE region H[F][dim+1] around the origin, the pairs i < j in
    # the order of np.triu_indices(N, 1); `region` as `obstacles` above: sent only when its bytes differ, None: what is set
    def set_pair_keep_out(self, H):
        """obtg_ctx_set_pair_keep_out: the separation region's faces a . d <= b (every b > 0) as rows (a, b); an empty H clears."""
        H = _f64(H).reshape(-1, self.dim + 1)
        self._pair_keep_out_key = None
        self._check(self._lib.obtg_ctx_set_pair_keep_out(self._h, _ptr(H), H.shape[0]), "obtg_ctx_set_pair_keep_out")
        self._pair_keep_out_key = H.tobytes() if H.shape[0] else None

    def _pair_keep_out(self, region):
        if region is not None:
            H = _f64(region)
            if self._pair_keep_out_key != H.tobytes():
                self.set_pair_keep_out(H)
        return self.len_pair_keep_out

    @property
    def len_pair_keep_out(self):
        return self._lib.obtg_len_pair_keep_out(self._h)

    def _pair_items(self, region):
        self._pair_keep_out(region)
        return self.n_veh * (self.n_veh - 1) // 2    # (no region: the library's call answers OBTG_ERR_ARG)

    def pair_keep_out_true_min(self, Y, region=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """Per vehicle pair i < j the separation row: the minimum over t in [0, 1] of the largest a_f . (c_i - c_j)(t) - b_f over
        the region's faces, minus margin (obtg_pair_keep_out_true_min): the dict of keep_out_true_min over the P = N (N - 1) / 2
        pairs and rel[B][P][dim][deg+1], the relative control points the search ran on."""
        return self._keep_out_call("obtg_pair_keep_out_true_min", self._pair_items(region),
                                   Y, margin, eps_rel, max_nodes, False, euclid=False, rel=True)

    def pair_keep_out_true_min_jac(self, Y, region=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """pair_keep_out_true_min with its envelope Jacobian (obtg_pair_keep_out_true_min_jac): the same dict, bit for bit, and
        jac[B][P][dim][deg+1], the block of the pair's FIRST vehicle; the second vehicle's is its exact negation."""
        return self._keep_out_call("obtg_pair_keep_out_true_min_jac", self._pair_items(region),
                                   Y, margin, eps_rel, max_nodes, True, euclid=False, rel=True)

    def pair_keep_out_euclid_true_min(self, Y, region=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """pair_keep_out_true_min under the Euclidean metric (obtg_pair_keep_out_euclid_true_min): the dict of
        keep_out_euclid_true_min (faces[B][P][3], dir[B][P][dim]) and rel."""
        return self._keep_out_call("obtg_pair_keep_out_euclid_true_min", self._pair_items(region),
                                   Y, margin, eps_rel, max_nodes, False, euclid=True, rel=True)

    def pair_keep_out_euclid_true_min_jac(self, Y, region=None, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """pair_keep_out_euclid_true_min with jac[B][P][dim][deg+1] = dir[c] B_i(t_star), the first vehicle's block."""
        return self._keep_out_call("obtg_pair_keep_out_euclid_true_min_jac", self._pair_items(region),
                                   Y, margin, eps_rel, max_nodes, True, euclid=True, rel=True)

    def pair_keep_out_true_min_dev(self, dY, B, d_out, d_t_star=None, d_face=None, d_lam=None, d_bound=None, d_nodes=None, d_status=None,
                                   d_rel=None, d_jac=None, euclid=False, margin=0.0, eps_rel=1e-9, max_nodes=100000):
        """The four _dev calls in one: euclid picks the metric (d_face, d_lam are then faces[.][3], dir[.][dim]), d_jac the _jac
        form."""
        name = "obtg_pair_keep_out_%strue_min%s_dev" % ("euclid_" if euclid else "", "" if d_jac is None else "_jac")
        ptrs = [d_out, d_t_star, d_face, d_lam, d_bound, d_nodes, d_status, d_rel] + ([] if d_jac is None else [d_jac])
        self._keep_out_call_dev(name, (dY,), B, margin, eps_rel, max_nodes, ptrs)

    def jerk(self, Y, tf, bound):
        """The jerk-bound rows (obtg_jerk): [B][N * (2 deg + DEG_ELEV + 1)] control points of
        bound**2 - (d/2)|c'''|^2, c''' = diff().diff().diff() of the vehicle's curve on a span of tf."""
        return self._vehicle_rows("obtg_jerk", Y, tf, (float(bound),), (self.len_speed,))

    def jerk_dev(self, dY, d_tf, B, bound, d_out):
        self._check(self._lib.obtg_jerk_dev(self._h, _vp(dY), _vp(d_tf), int(B), float(bound), _vp(d_out)), "obtg_jerk_dev")

    def jerk_true_min(self, Y, tf, bound, eps_rel=1e-9, max_nodes=100000):
        """Per vehicle the true minimum over t in [0, 1] of bound**2 - (d/2)|c'''|^2 -- the polynomial jerk(Y, tf, bound) holds
        the control points of (obtg_jerk_true_min; DEG_ELEV does not enter): dict(val[B][N], t_star[B][N], status[B][N])."""
        return self._true_min("obtg_jerk_true_min", self.n_veh, Y, tf, (float(bound),), eps_rel, max_nodes)

    def jerk_true_min_dev(self, dY, d_tf, B, bound, d_out, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_jerk_true_min_dev", (dY, d_tf), B, (float(bound),), eps_rel, max_nodes, d_out, d_t_star, d_status)

    def jerk_true_min_jac(self, Y, tf, bound, eps_rel=1e-9, max_nodes=100000):
        """jerk_true_min with its envelope Jacobian (obtg_jerk_true_min_jac): dict(val, t_star, status -- the bits of
        jerk_true_min --, jac[B][N][dim][deg+1]: d/d(the vehicle's own control points) of its polynomial at t_star,
        jac_tf[B][N]: d/dtf at fixed control points)."""
        return self._true_min("obtg_jerk_true_min_jac", self.n_veh, Y, tf, (float(bound),), eps_rel, max_nodes, "jac", "jac_tf")

    def jerk_true_min_jac_dev(self, dY, d_tf, B, bound, d_out, d_jac, d_jac_tf=None, d_t_star=None, d_status=None,
                               eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_jerk_true_min_jac_dev", (dY, d_tf), B, (float(bound),), eps_rel, max_nodes, d_out, d_t_star,
                           d_status, d_jac, d_jac_tf)

    def ang_rate_poly(self, Y, tf, max_rate):
        """The true angular-rate rows' polynomials (obtg_ang_rate_poly; dim 2): [B][N][2][2 deg + 1] Bernstein coefficients of
        p_+ = max_rate den - num (side 0) and p_- = max_rate den + num (side 1), den = x'^2 + y'^2, num = y'' x' - x'' y' --
        in units of max_rate * speed^2, not ang_rate's maxAngRate^2 - omega^2."""
        return self._vehicle_rows("obtg_ang_rate_poly", Y, tf, (float(max_rate),), (self.n_veh, 2, 2 * self.deg + 1))

    def ang_rate_poly_dev(self, dY, d_tf, B, max_rate, d_out):
        self._check(self._lib.obtg_ang_rate_poly_dev(self._h, _vp(dY), _vp(d_tf), int(B), float(max_rate), _vp(d_out)),
                    "obtg_ang_rate_poly_dev")

    def ang_rate_true_min(self, Y, tf, max_rate, eps_rel=1e-9, max_nodes=100000):
        """Per vehicle and side the true minimum over t in [0, 1] of ang_rate_poly's polynomial (obtg_ang_rate_true_min;
        DEG_ELEV does not enter): dict(val[B][N][2], t_star[B][N][2], status[B][N][2] as MD_*); |angular rate| <= max_rate
        on the whole trajectory iff both values of the vehicle are >= 0."""
        return self._true_min("obtg_ang_rate_true_min", (self.n_veh, 2), Y, tf, (float(max_rate),), eps_rel, max_nodes)

    def ang_rate_true_min_dev(self, dY, d_tf, B, max_rate, d_out, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_ang_rate_true_min_dev", (dY, d_tf), B, (float(max_rate),), eps_rel, max_nodes, d_out, d_t_star,
                           d_status)

    def ang_rate_true_min_jac(self, Y, tf, max_rate, eps_rel=1e-9, max_nodes=100000):
        """ang_rate_true_min with its envelope Jacobian (obtg_ang_rate_true_min_jac): dict(val, t_star, status -- the bits of
        ang_rate_true_min --, jac[B][N][2][2][deg+1]: d/d(the vehicle's own control points) of the side's polynomial at
        t_star, jac_tf[B][N][2]: d/dtf at fixed control points)."""
        return self._true_min("obtg_ang_rate_true_min_jac", (self.n_veh, 2), Y, tf, (float(max_rate),), eps_rel, max_nodes,
                              "jac", "jac_tf")

    def ang_rate_true_min_jac_dev(self, dY, d_tf, B, max_rate, d_out, d_jac, d_jac_tf=None, d_t_star=None, d_status=None,
                                  eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_ang_rate_true_min_jac_dev", (dY, d_tf), B, (float(max_rate),), eps_rel, max_nodes, d_out, d_t_star,
                           d_status, d_jac, d_jac_tf)

    def curvature_poly(self, Y):
        """The curvature rows' polynomials (obtg_curvature_poly; dim 2): [B][N][2][2 deg + 1], the Bernstein coefficients of
        num = y'' x' - x'' y' and then of den = x'^2 + y'^2 on a span of 1; kappa = num / den^(3/2)."""
        Y, B = self._rows(Y)
        out = pinned_empty((B, self.n_veh, 2, 2 * self.deg + 1))
        self._check(self._lib.obtg_curvature_poly(self._h, _ptr(Y), B, _ptr(out)), "obtg_curvature_poly")
        return out

    def curvature_poly_dev(self, dY, B, d_out):
        self._check(self._lib.obtg_curvature_poly_dev(self._h, _vp(dY), int(B), _vp(d_out)), "obtg_curvature_poly_dev")

    def curvature_true_min(self, Y, max_curv, eps_rel=1e-9, max_nodes=100000):
        """Per vehicle and side max_curv - max over t in [0, 1] of max(0, +-kappa) (obtg_curvature_true_min; no time span
        enters): dict(val[B][N][2], t_star[B][N][2], status[B][N][2] as MD_*); |kappa| <= max_curv on the whole path iff both
        values of the vehicle are >= 0."""
        return self._true_min("obtg_curvature_true_min", (self.n_veh, 2), Y, None, (float(max_curv),), eps_rel, max_nodes)

    def curvature_true_min_dev(self, dY, B, max_curv, d_out, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_curvature_true_min_dev", (dY,), B, (float(max_curv),), eps_rel, max_nodes, d_out, d_t_star, d_status)

    def curvature_true_min_jac(self, Y, max_curv, eps_rel=1e-9, max_nodes=100000):
        """curvature_true_min with its envelope Jacobian (obtg_curvature_true_min_jac): dict(val, t_star, status -- the bits of
        curvature_true_min --, jac[B][N][2][2][deg+1]: d/d(the vehicle's own control points) of the row at t_star; zero where
        the row is max_curv itself).  The rows do not depend on tf."""
        return self._true_min("obtg_curvature_true_min_jac", (self.n_veh, 2), Y, None, (float(max_curv),), eps_rel, max_nodes, "jac")

    def curvature_true_min_jac_dev(self, dY, B, max_curv, d_out, d_jac, d_t_star=None, d_status=None, eps_rel=1e-9,
                                   max_nodes=100000):
        self._true_min_dev("obtg_curvature_true_min_jac_dev", (dY,), B, (float(max_curv),), eps_rel, max_nodes, d_out, d_t_star,
                           d_status, d_jac)

    def bern_curvature(self, c, eps_rel=1e-9, max_nodes=100000):
        """The curvature range of free planar curves c[M][2][K], 2 <= K <= 32 control points (obtg_bern_curvature):
        dict(k_min[M], t_min[M], k_max[M], t_max[M], status[M][2] -- side 0: k_max, side 1: k_min)."""
        c = _f64(c)
        if c.ndim == 2:
            c = c[None]
        M, two, K = c.shape
        if two != 2:
            raise ValueError("bern_curvature needs planar curves [M][2][K], got shape %r" % (c.shape,))
        r = dict(k_min=np.empty(M), t_min=np.empty(M), k_max=np.empty(M), t_max=np.empty(M), status=np.zeros((M, 2), np.int32))
        self._check(self._lib.obtg_bern_curvature(self._h, _ptr(c), M, K, float(eps_rel), int(max_nodes),
                                                  *[_ptr(a) for a in r.values()]), "obtg_bern_curvature")
        return r

    def bern_curvature_dev(self, d_c, M, K, d_k_min, d_t_min, d_k_max, d_t_max, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._check(self._lib.obtg_bern_curvature_dev(self._h, _vp(d_c), int(M), int(K), float(eps_rel), int(max_nodes), _vp(d_k_min),
                                                      _vp(d_t_min), _vp(d_k_max), _vp(d_t_max), _vp(d_status)), "obtg_bern_curvature_dev")

    def space_curvature_poly(self, Y):
        """The space-curvature rows' polynomials (obtg_space_curvature_poly; dim 3): [B][N][4][2 deg + 1], the Bernstein
        coefficients of the three components of w = c' x c'' and then of den = |c'|^2 on a span of 1;
        kappa = |w| / den^(3/2)."""
        Y, B = self._rows(Y)
        out = pinned_empty((B, self.n_veh, 4, 2 * self.deg + 1))
        self._check(self._lib.obtg_space_curvature_poly(self._h, _ptr(Y), B, _ptr(out)), "obtg_space_curvature_poly")
        return out

    def space_curvature_poly_dev(self, dY, B, d_out):
        self._check(self._lib.obtg_space_curvature_poly_dev(self._h, _vp(dY), int(B), _vp(d_out)), "obtg_space_curvature_poly_dev")

    def space_curvature_true_min(self, Y, max_curv, eps_rel=1e-9, max_nodes=100000):
        """Per vehicle max_curv - max over t in [0, 1] of kappa (obtg_space_curvature_true_min; dim 3; no time span enters):
        dict(val[B][N], t_star[B][N], status[B][N] as MD_*); kappa <= max_curv on the whole path iff the value is >= 0."""
        return self._true_min("obtg_space_curvature_true_min", self.n_veh, Y, None, (float(max_curv),), eps_rel, max_nodes)

    def space_curvature_true_min_dev(self, dY, B, max_curv, d_out, d_t_star=None, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._true_min_dev("obtg_space_curvature_true_min_dev", (dY,), B, (float(max_curv),), eps_rel, max_nodes, d_out, d_t_star,
                           d_status)

    def space_curvature_true_min_jac(self, Y, max_curv, eps_rel=1e-9, max_nodes=100000):
        """space_curvature_true_min with its envelope Jacobian (obtg_space_curvature_true_min_jac): dict(val, t_star, status --
        the bits of space_curvature_true_min --, jac[B][N][3][deg+1]: d/d(the vehicle's own control points) of the row at
        t_star; zero where the row is max_curv itself).  The rows do not depend on tf."""
        return self._true_min("obtg_space_curvature_true_min_jac", self.n_veh, Y, None, (float(max_curv),), eps_rel, max_nodes, "jac")

    def space_curvature_true_min_jac_dev(self, dY, B, max_curv, d_out, d_jac, d_t_star=None, d_status=None, eps_rel=1e-9,
                                         max_nodes=100000):
        self._true_min_dev("obtg_space_curvature_true_min_jac_dev", (dY,), B, (float(max_curv),), eps_rel, max_nodes, d_out,
                           d_t_star, d_status, d_jac)

    def bern_space_curvature(self, c, eps_rel=1e-9, max_nodes=100000):
        """The largest curvature of free space curves c[M][3][K], 2 <= K <= 32 control points (obtg_bern_space_curvature):
        dict(k_max[M], t_max[M], status[M])."""
        c = _f64(c)
        if c.ndim == 2:
            c = c[None]
        M, three, K = c.shape
        if three != 3:
            raise ValueError("bern_space_curvature needs space curves [M][3][K], got shape %r" % (c.shape,))
        r = dict(k_max=np.empty(M), t_max=np.empty(M), status=np.zeros(M, np.int32))
        self._check(self._lib.obtg_bern_space_curvature(self._h, _ptr(c), M, K, float(eps_rel), int(max_nodes),
                                                        *[_ptr(a) for a in r.values()]), "obtg_bern_space_curvature")
        return r

    def bern_space_curvature_dev(self, d_c, M, K, d_k_max, d_t_max, d_status=None, eps_rel=1e-9, max_nodes=100000):
        self._check(self._lib.obtg_bern_space_curvature_dev(self._h, _vp(d_c), int(M), int(K), float(eps_rel), int(max_nodes),
                                                            _vp(d_k_max), _vp(d_t_max), _vp(d_status)), "obtg_bern_space_curvature_dev")

    def ang_rate(self, Y, tf, max_rate):
        return self._vehicle_rows("obtg_ang_rate", Y, tf, (float(max_rate),), (self.len_ang_rate,))

    def euclidean_obj(self, Y):
        Y, B = self._rows(Y)
        out = np.empty(B)
        self._check(self._lib.obtg_euclidean_obj(self._h, _ptr(Y), B, _ptr(out)), "obtg_euclidean_obj")
        return out

    def deriv_energy_obj(self, Y, tf, order):
        """order 2: _minAccelObjective, order 3: _minJerkObjective (optimization.py:503-539)."""
        Y, B = self._rows(Y)
        tf = self._tf(tf, B)
        out = np.empty(B)
        fn = {2: self._lib.obtg_accel_obj, 3: self._lib.obtg_jerk_obj}[int(order)]
        self._check(fn(self._h, _ptr(Y), _ptr(tf), B, _ptr(out)), "obtg_accel/jerk_obj")
        return out

    def accel_obj(self, Y, tf):
        return self.deriv_energy_obj(Y, tf, 2)

    # -- true arc length (include/obtg.h obtg_bern_arc_length / obtg_arc_length_obj)
    def bern_arc_length(self, c, eps_rel=1e-12, max_nodes=100000, grad=False):
        """The length of every curve of c[M][d][K] (one curve: [d][K]; degree 1 .. 31, d <= 3), by adaptive 8-point Gauss-Legendre
        bisection (obtg_bern_arc_length): dict(len[M], err[M], nodes[M], status[M] as MD_*) and, with grad, grad[M][d][K], the
        derivative of len with respect to the control points.  Where status is MD_OK err <= eps_rel x the length of the
        control polygon; an eps_rel below the kernel's floor (include/obtg.h) is raised to it."""
        c = _f64(c)
        if c.ndim == 2:
            c = c[None]
        M, d, K = c.shape
        r = dict(len=np.empty(M), err=np.empty(M), nodes=np.zeros(M, np.int32), status=np.zeros(M, np.int32))
        if grad:
            r["grad"] = np.empty((M, d, K))
        self._check(self._lib.obtg_bern_arc_length(self._h, _ptr(c), M, d, K, float(eps_rel), int(max_nodes), _ptr(r["len"]),
                                                   _ptr(r["err"]), _ptr(r["nodes"]), _ptr(r["status"]), _ptr(r.get("grad"))),
                    "obtg_bern_arc_length")
        return r

    def bern_arc_length_dev(self, d_c, M, d, K, d_len, d_err=None, d_nodes=None, d_status=None, d_grad=None, eps_rel=1e-12,
                            max_nodes=100000):
        self._check(self._lib.obtg_bern_arc_length_dev(self._h, _vp(d_c), int(M), int(d), int(K), float(eps_rel), int(max_nodes),
                                                       _vp(d_len), _vp(d_err), _vp(d_nodes), _vp(d_status), _vp(d_grad)),
                    "obtg_bern_arc_length_dev")

    def arc_length_obj(self, Y, eps_rel=1e-12, max_nodes=100000, grad=False):
        """Per row of Y the summed true lengths of its vehicles' curves (obtg_arc_length_obj): dict(val[B], status[B]: the worst
        MD_* among the row's vehicles) and, with grad, grad[B][N d][n+1] in euclidean_grad's layout."""
        Y, B = self._rows(Y)
        r = dict(val=np.empty(B), status=np.zeros(B, np.int32))
        if grad:
            r["grad"] = np.empty((B, self.n_veh * self.dim, self.deg + 1))
        self._check(self._lib.obtg_arc_length_obj(self._h, _ptr(Y), B, float(eps_rel), int(max_nodes), _ptr(r["val"]),
                                                  _ptr(r["status"]), _ptr(r.get("grad"))), "obtg_arc_length_obj")
        return r

    def arc_length_obj_dev(self, dY, B, d_out, d_status=None, d_grad=None, eps_rel=1e-12, max_nodes=100000):
        self._check(self._lib.obtg_arc_length_obj_dev(self._h, _vp(dY), int(B), float(eps_rel), int(max_nodes), _vp(d_out),
                                                      _vp(d_status), _vp(d_grad)), "obtg_arc_length_obj_dev")

    # -- exact derivatives (include/obtg.h obtg_*_jac / *_grad): blocks per pair / vehicle, [..][d][deg + 1] per vehicle
    def temporal_sep_jac(self, Y):
        """d(temporal_sep rows)/d(first object's control points): [B][P][2n+R+1][d][n+1] (the second object's: the negation)."""
        Y, B = self._rows(Y)
        L, nc = 2 * self.deg + self.deg_elev + 1, self.deg + 1
        out = np.empty((B, self.num_pairs, L, self.dim, nc))
        self._check(self._lib.obtg_temporal_sep_jac(self._h, _ptr(Y), B, _ptr(out)), "obtg_temporal_sep_jac")
        return out

    def temporal_sep_jac_dev(self, dY, B, d_out):
        self._check(self._lib.obtg_temporal_sep_jac_dev(self._h, _vp(dY), int(B), _vp(d_out)), "obtg_temporal_sep_jac_dev")

    def speed_jac(self, Y, tf, is_max):
        """(d rows / d own control points [B][N][2n+R+1][d][n+1], d rows / d tf [B][N][2n+R+1]) of speed(Y, tf, bound, is_max)."""
        Y, B = self._rows(Y)
        tf = self._tf(tf, B)
        L, nc = 2 * self.deg + self.deg_elev + 1, self.deg + 1
        out, out_tf = np.empty((B, self.n_veh, L, self.dim, nc)), np.empty((B, self.n_veh, L))
        self._check(self._lib.obtg_speed_jac(self._h, _ptr(Y), _ptr(tf), B, int(bool(is_max)), _ptr(out), _ptr(out_tf)),
                    "obtg_speed_jac")
        return out, out_tf

    def speed_jac_dev(self, dY, d_tf, B, is_max, d_out, d_out_tf=None):
        self._check(self._lib.obtg_speed_jac_dev(self._h, _vp(dY), _vp(d_tf), int(B), int(bool(is_max)), _vp(d_out),
                                                 _vp(d_out_tf)), "obtg_speed_jac_dev")

    def ang_rate_jac(self, Y, tf):
        """(d rows / d own control points [B][N][4(n+R)+1][2][n+1], d rows / d tf [B][N][4(n+R)+1]) of ang_rate; rows whose
        value is not finite: NaN."""
        Y, B = self._rows(Y)
        tf = self._tf(tf, B)
        La, nc = 4 * (self.deg + self.deg_elev) + 1, self.deg + 1
        out, out_tf = np.empty((B, self.n_veh, La, 2, nc)), np.empty((B, self.n_veh, La))
        self._check(self._lib.obtg_ang_rate_jac(self._h, _ptr(Y), _ptr(tf), B, _ptr(out), _ptr(out_tf)), "obtg_ang_rate_jac")
        return out, out_tf

    def ang_rate_jac_dev(self, dY, d_tf, B, d_out, d_out_tf=None):
        self._check(self._lib.obtg_ang_rate_jac_dev(self._h, _vp(dY), _vp(d_tf), int(B), _vp(d_out), _vp(d_out_tf)),
                    "obtg_ang_rate_jac_dev")

    def euclidean_grad(self, Y):
        """Gradient of euclidean_obj: [B][N d][n+1]."""
        Y, B = self._rows(Y)
        out = np.empty((B, self.n_veh * self.dim, self.deg + 1))
        self._check(self._lib.obtg_euclidean_grad(self._h, _ptr(Y), B, _ptr(out)), "obtg_euclidean_grad")
        return out

    def deriv_energy_grad(self, Y, tf, order):
        """Gradient of deriv_energy_obj (order 2 accel, 3 jerk): ([B][N d][n+1], d/dtf [B])."""
        Y, B = self._rows(Y)
        tf = self._tf(tf, B)
        out, out_tf = np.empty((B, self.n_veh * self.dim, self.deg + 1)), np.empty(B)
        self._check(self._lib.obtg_deriv_energy_grad(self._h, _ptr(Y), _ptr(tf), B, int(order), _ptr(out), _ptr(out_tf)),
                    "obtg_deriv_energy_grad")
        return out, out_tf

    # -- device-pointer sweeps (pointers are plain ints, e.g. torch.Tensor.data_ptr())
    def temporal_sep_dev(self, dY, B, max_sep, d_out, pair_begin=0, pair_count=None):
        if pair_count is None:
            pair_count = self.num_pairs - pair_begin
        self._check(self._lib.obtg_temporal_sep_dev(self._h, _vp(dY), B, float(max_sep), pair_begin, pair_count,
                                                    _vp(d_out)), "obtg_temporal_sep_dev")

    def temporal_sep_min_dev(self, dY, B, max_sep, d_out, pair_begin=0, pair_count=None):
        if pair_count is None:
            pair_count = self.num_pairs - pair_begin
        self._check(self._lib.obtg_temporal_sep_min_dev(self._h, _vp(dY), B, float(max_sep), pair_begin, pair_count,
                                                        _vp(d_out)), "obtg_temporal_sep_min_dev")

    def speed_dev(self, dY, d_tf, B, bound, is_max, d_out):
        self._check(self._lib.obtg_speed_dev(self._h, _vp(dY), _vp(d_tf), B, float(bound), int(bool(is_max)),
                                             _vp(d_out)), "obtg_speed_dev")

    def ang_rate_dev(self, dY, d_tf, B, max_rate, d_out):
        self._check(self._lib.obtg_ang_rate_dev(self._h, _vp(dY), _vp(d_tf), B, float(max_rate), _vp(d_out)),
                    "obtg_ang_rate_dev")

    def dynamics_dev(self, dY, d_tf, B, speed_bound, speed_is_max, max_rate, d_out_speed, d_out_ang):
        self._check(self._lib.obtg_dynamics_dev(self._h, _vp(dY), _vp(d_tf), B, float(speed_bound),
                                                int(bool(speed_is_max)), float(max_rate), _vp(d_out_speed),
                                                _vp(d_out_ang)), "obtg_dynamics_dev")

    def fd_batch_dev(self, dY0, n_fixed_cols, h, B, dY):
        self._check(self._lib.obtg_fd_batch_dev(self._h, _vp(dY0), int(n_fixed_cols), float(h), B, _vp(dY)),
                    "obtg_fd_batch_dev")

    def one_vs_many_min(self, one, many, max_sep):
        """Examples/SequentialSwarm.py:43-70: one[B][dim][deg+1] (or [dim][deg+1]) against many[K][dim][deg+1] ->
        out[B][K], the per-pair minimum of the elevated squared-distance control points minus max_sep^2
        (include/obtg.h obtg_one_vs_many_min).  NaN for a pair whose elevated control points are not all finite -- what the
        reference's `.cpts.min()` returns."""
        nc = self.deg + 1
        one = np.ascontiguousarray(one, dtype=np.float64).reshape(-1, self.dim, nc)
        many = np.ascontiguousarray(many, dtype=np.float64).reshape(-1, self.dim, nc)
        B, K = one.shape[0], many.shape[0]
        out = np.empty((B, K))
        self._check(self._lib.obtg_one_vs_many_min(self._h, _ptr(one), B, _ptr(many), K, float(max_sep), _ptr(out)),
                    "obtg_one_vs_many_min")
        return out

    def one_vs_many_min_dev(self, d_one, B, d_many, K, max_sep, d_out):
        self._check(self._lib.obtg_one_vs_many_min_dev(self._h, _vp(d_one), int(B), _vp(d_many), int(K), float(max_sep),
                                                       _vp(d_out)), "obtg_one_vs_many_min_dev")

    def one_vs_many_min_spans(self, one, one_span, many, many_span, max_sep, no_overlap=np.inf):
        """one_vs_many_min for curves on different time spans (include/obtg.h obtg_one_vs_many_min_spans; the reference's
        Bezier.sub with _temporalAlignment, bezier.py:347-374, 903-941): one_span[B][2], many_span[K][2] = (t0, tf) per
        curve; every pair is cut down to its overlap first.  -> out[B][K]; pairs whose spans do not overlap (the
        reference's None, touching spans included) hold `no_overlap`, whatever their control points hold; an overlapping pair
        whose cut curves give a non-finite control point holds NaN."""
        nc = self.deg + 1
        one = np.ascontiguousarray(one, dtype=np.float64).reshape(-1, self.dim, nc)
        many = np.ascontiguousarray(many, dtype=np.float64).reshape(-1, self.dim, nc)
        B, K = one.shape[0], many.shape[0]
        so, sm = _f64(one_span).reshape(B, 2), _f64(many_span).reshape(K, 2)
        out = np.empty((B, K))
        self._check(self._lib.obtg_one_vs_many_min_spans(self._h, _ptr(one), _ptr(so), B, _ptr(many), _ptr(sm), K, float(max_sep),
                                                         float(no_overlap), _ptr(out)), "obtg_one_vs_many_min_spans")
        return out

    def one_vs_many_min_spans_dev(self, d_one, one_span, B, d_many, many_span, K, max_sep, d_out, no_overlap=np.inf):
        """d_one, d_many, d_out: device pointers; one_span[B][2], many_span[K][2]: host arrays."""
        so, sm = _f64(one_span).reshape(int(B), 2), _f64(many_span).reshape(int(K), 2)
        self._check(self._lib.obtg_one_vs_many_min_spans_dev(self._h, _vp(d_one), _ptr(so), int(B), _vp(d_many), _ptr(sm), int(K),
                                                             float(max_sep), float(no_overlap), _vp(d_out)),
                    "obtg_one_vs_many_min_spans_dev")

    def set_second_speed_bound(self, bound, is_max, d_out2):
        """Both speed bounds from one dynamics pass (include/obtg.h obtg_ctx_set_second_speed_bound): while d_out2 (a
        device pointer, [B][N*(2n+R+1)]) is set, dynamics_dev / constraint_sweep_dev also write this bound's rows.
        d_out2 = None switches it off."""
        self._check(self._lib.obtg_ctx_set_second_speed_bound(self._h, float(bound), int(bool(is_max)),
                                                               _vp(d_out2) if d_out2 else None),
                    "obtg_ctx_set_second_speed_bound")

    def fd_view_begin(self, dY0, n_fixed_cols, h, B, row_begin=0):
        """Open a virtual finite-difference batch over the ONE device row dY0 (include/obtg.h obtg_fd_view_begin): until
        fd_view_end the `_dev` sweeps take dY = None.  row_begin > 0: the view is rows row_begin .. row_begin + B - 1 of
        the batch (obtg_fd_view_begin_rows: one rank's share of a row-sharded iteration)."""
        if row_begin:
            self._check(self._lib.obtg_fd_view_begin_rows(self._h, _vp(dY0), int(n_fixed_cols), float(h), int(row_begin), int(B)),
                        "obtg_fd_view_begin_rows")
        else:
            self._check(self._lib.obtg_fd_view_begin(self._h, _vp(dY0), int(n_fixed_cols), float(h), int(B)), "obtg_fd_view_begin")

    def fd_view_end(self):
        self._check(self._lib.obtg_fd_view_end(self._h), "obtg_fd_view_end")

    def fd_forms_on_the_fly(self):
        """(pair sweep, dynamics): does the _fd_dev form build the finite-difference rows while staging them?"""
        m = self._lib.obtg_fd_forms_on_the_fly(self._h)
        return bool(m & 1), bool(m & 2)

    def pair_sweep_fd_dev(self, dY0, n_fixed_cols, h, B, max_sep, d_out_sep, d_flag, d_p1, d_p2, d_dist, d_nsup=None,
                          d_status=None, max_iter=128, md_cap=4096):
        """obtg_pair_sweep_dev on the virtual FD batch of ONE row dY0 (include/obtg.h obtg_pair_sweep_fd_dev)."""
        self._need_hull_pairs("pair_sweep_fd_dev")
        self._check(self._lib.obtg_pair_sweep_fd_dev(self._h, _vp(dY0), int(n_fixed_cols), float(h), B, float(max_sep),
                                                     _vp(d_out_sep), max_iter, md_cap, _vp(d_flag), _vp(d_p1), _vp(d_p2),
                                                     _vp(d_dist), _vp(d_nsup) if d_nsup else None,
                                                     _vp(d_status) if d_status else None), "obtg_pair_sweep_fd_dev")

    def dynamics_fd_dev(self, dY0, n_fixed_cols, h, d_tf, B, speed_bound, speed_is_max, max_rate, d_out_speed, d_out_ang):
        self._check(self._lib.obtg_dynamics_fd_dev(self._h, _vp(dY0), int(n_fixed_cols), float(h), _vp(d_tf), B,
                                                   float(speed_bound), int(bool(speed_is_max)), float(max_rate),
                                                   _vp(d_out_speed), _vp(d_out_ang)), "obtg_dynamics_fd_dev")

    # -- GJK
    def gjk_pairs(self, pts, off, pair_a, pair_b, max_iter=128, md_cap=4096, trace_cap=0):
        pts, off = _polys_arg(pts, off)
        pa, pb, n = _pairs_arg(pair_a, pair_b)
        flag = np.zeros(n, np.int32)
        nsup = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        p1 = np.empty((n, 3))
        p2 = np.empty((n, 3))
        dist = np.empty(n)
        trace = np.zeros((n, trace_cap, 2), np.int16) if trace_cap else None
        self._check(self._lib.obtg_gjk_pairs(self._h, _ptr(pts), pts.shape[0], _ptr(off), off.shape[0] - 1,
                                             _ptr(pa), _ptr(pb), n, max_iter, md_cap, _ptr(flag), _ptr(p1),
                                             _ptr(p2), _ptr(dist), _ptr(trace), trace_cap, _ptr(nsup),
                                             _ptr(status)), "obtg_gjk_pairs")
        return dict(flag=flag, c1=p1, c2=p2, dist=dist, trace=trace, n_support=nsup, status=status)

    def set_polygons(self, pts, off):
        if pts is None or len(off) <= 1:
            self._check(self._lib.obtg_ctx_set_polygons(self._h, None, 0, None, 0), "obtg_ctx_set_polygons")
            self.n_poly = 0
            self.n_hull_pairs = None      # object ids changed meaning: the library dropped the pair list too
            return
        pts = _f64(pts).reshape(-1, 3)
        off = _i32(off)
        self._check(self._lib.obtg_ctx_set_polygons(self._h, _ptr(pts), pts.shape[0], _ptr(off), off.shape[0] - 1),
                    "obtg_ctx_set_polygons")
        self.n_poly = off.shape[0] - 1
        self.n_hull_pairs = None

    def _need_hull_pairs(self, what):
        if self.n_hull_pairs is None:
            raise ObtgError("%s: no hull pair list registered -- call set_hull_pairs() (again) after set_polygons()" % what)

    def set_hull_pairs(self, pair_a, pair_b):
        pa, pb = _i32(pair_a), _i32(pair_b)
        self._check(self._lib.obtg_ctx_set_hull_pairs(self._h, _ptr(pa), _ptr(pb), pa.shape[0]),
                    "obtg_ctx_set_hull_pairs")
        self.n_hull_pairs = pa.shape[0]

    def set_fd_dedup(self, on):
        self._check(self._lib.obtg_ctx_set_fd_dedup(self._h, int(bool(on))), "obtg_ctx_set_fd_dedup")

    def set_fd_view_structured(self, on):
        """Structured routing of constraint_sweep_dev(None, ...) inside a view (on by default; OBTG_FD_VIEW_STRUCTURED=0 in
        the environment makes new contexts start with it off).  Same bits either way."""
        self._check(self._lib.obtg_ctx_set_fd_view_structured(self._h, int(bool(on))), "obtg_ctx_set_fd_view_structured")

    def set_gjk_history(self, on):
        self._check(self._lib.obtg_ctx_set_gjk_history(self._h, int(bool(on))), "obtg_ctx_set_gjk_history")

    SWEEP_FORMS = ("two_launches", "one_launch", "tiled", "general", "dedup")

    def sweep_shape(self, B, which=1, want_dyn=False):
        """Which form and grid the hull-pair sweep of B rows takes now (obtg_sweep_shape; launches nothing).  which = 0:
        gjk_swarm[_dev]; which = 1: pair_sweep_dev, with want_dyn constraint_sweep_dev with every family wanted."""
        self._need_hull_pairs("sweep_shape")
        out = (C.c_int * 8)()
        self._check(self._lib.obtg_sweep_shape(self._h, int(B), int(which), int(bool(want_dyn)), C.cast(out, _vp)), "obtg_sweep_shape")
        return dict(form=self.SWEEP_FORMS[out[0]], wgs=out[1], passes=out[2], chunk=out[3], tile_height=out[4],
                    refill_min=out[5], hist_shift=out[6], fold_dyn=bool(out[7]))

    def gjk_swarm(self, Y, max_iter=128, md_cap=4096):
        self._need_hull_pairs("gjk_swarm")
        Y, B = self._rows(Y)
        n = self.n_hull_pairs
        flag, nsup, status = (pinned_empty((B, n), np.int32) for _ in range(3))
        p1, p2, dist = pinned_empty((B, n, 3)), pinned_empty((B, n, 3)), pinned_empty((B, n))
        for a, v in ((flag, 0), (nsup, 0), (status, 0), (p1, np.nan), (p2, np.nan), (dist, np.nan)):
            a.fill(v)
        self._check(self._lib.obtg_gjk_swarm(self._h, _ptr(Y), B, max_iter, md_cap, _ptr(flag), _ptr(p1), _ptr(p2),
                                             _ptr(dist), _ptr(nsup), _ptr(status)), "obtg_gjk_swarm")
        return dict(flag=flag, c1=p1, c2=p2, dist=dist, n_support=nsup, status=status)

    def gjk_swarm_dev(self, dY, B, d_flag, d_p1, d_p2, d_dist, d_nsup=None, d_status=None, max_iter=128,
                      md_cap=4096):
        self._need_hull_pairs("gjk_swarm_dev")
        self._check(self._lib.obtg_gjk_swarm_dev(self._h, _vp(dY), B, max_iter, md_cap, _vp(d_flag), _vp(d_p1),
                                                 _vp(d_p2), _vp(d_dist), _vp(d_nsup), _vp(d_status)),
                    "obtg_gjk_swarm_dev")

    # -- minDist
    def pair_sweep_dev(self, dY, B, max_sep, d_out_sep, d_flag, d_p1, d_p2, d_dist, d_nsup=None, d_status=None,
                       max_iter=128, md_cap=4096):
        """temporal separation + gjkNew hull sweep of the same rows in one launch (obtg_pair_sweep_dev)."""
        self._need_hull_pairs("pair_sweep_dev")
        self._check(self._lib.obtg_pair_sweep_dev(self._h, _vp(dY), B, float(max_sep), _vp(d_out_sep), max_iter,
                                                  md_cap, _vp(d_flag), _vp(d_p1), _vp(d_p2), _vp(d_dist),
                                                  _vp(d_nsup) if d_nsup else None,
                                                  _vp(d_status) if d_status else None), "obtg_pair_sweep_dev")

    def constraint_sweep_dev(self, dY, d_tf, B, max_sep, d_out_sep, speed_bound, speed_is_max, max_rate, d_out_speed,
                             d_out_ang, d_flag, d_p1, d_p2, d_dist, d_nsup=None, d_status=None, max_iter=128, md_cap=4096):
        """Every constraint family of the batch in one call (obtg_constraint_sweep_dev)."""
        self._need_hull_pairs("constraint_sweep_dev")
        self._check(self._lib.obtg_constraint_sweep_dev(self._h, _vp(dY), _vp(d_tf), B, float(max_sep), _vp(d_out_sep),
                                                        float(speed_bound), int(bool(speed_is_max)), float(max_rate),
                                                        _vp(d_out_speed), _vp(d_out_ang), max_iter, md_cap, _vp(d_flag),
                                                        _vp(d_p1), _vp(d_p2), _vp(d_dist), _vp(d_nsup) if d_nsup else None,
                                                        _vp(d_status) if d_status else None), "obtg_constraint_sweep_dev")

    def constraint_sweep_fd_structured_dev(self, dY0, n_fixed_cols, h, d_tf, B, max_sep, d_out_sep, speed_bound, speed_is_max,
                                           max_rate, d_out_speed, d_out_ang, d_flag, d_p1, d_p2, d_dist, d_nsup=None,
                                           d_status=None, max_iter=128, md_cap=4096, row_begin=0):
        """The FD step as one launch that evaluates row 0 in full and per row only what its vehicle touches
        (obtg_constraint_sweep_fd_structured_dev); raises for shapes it does not cover (OBTG_ERR_UNSUPPORTED).
        row_begin > 0: the B rows [row_begin, row_begin + B) of the batch (obtg_constraint_sweep_fd_structured_rows_dev):
        d_tf and the outputs hold those B rows."""
        self._need_hull_pairs("constraint_sweep_fd_structured_dev")
        self._check(self._lib.obtg_constraint_sweep_fd_structured_rows_dev(
            self._h, _vp(dY0), int(n_fixed_cols), float(h), int(row_begin), _vp(d_tf), int(B), float(max_sep), _vp(d_out_sep),
            float(speed_bound), int(bool(speed_is_max)), float(max_rate), _vp(d_out_speed), _vp(d_out_ang), max_iter, md_cap,
            _vp(d_flag), _vp(d_p1), _vp(d_p2), _vp(d_dist), _vp(d_nsup) if d_nsup else None,
            _vp(d_status) if d_status else None), "obtg_constraint_sweep_fd_structured_rows_dev")

    def _curve_search(self, name, curves, polys, pairs, params, width, zeroed=False, info_keys=("gjk_calls", "depth")):
        """One of the six curve searches of the C ABI, which all take (curves, [polygons,] pair lists, the call's own scalars,
        res, info, status).  polys: (pts, off) or None; pairs: (first, second); width: doubles of res per pair."""
        curves, n_curves, K = _curves_arg(curves)
        args = [self._h, _ptr(curves), n_curves, K]
        if polys is not None:
            pts, off = _polys_arg(*polys)
            args += [_ptr(pts), pts.shape[0], _ptr(off), off.shape[0] - 1]
        pa, pb, n = _pairs_arg(*pairs)
        res, info, status = _search_out(n, width, zeroed)
        self._check(getattr(self._lib, name)(*args, _ptr(pa), _ptr(pb), n, *params, _ptr(res), _ptr(info), _ptr(status)), name)
        return {"res": res, "nodes": info[:, 0], info_keys[0]: info[:, 1], info_keys[1]: info[:, 2], "status": status}

    def min_dist(self, curves, pair_a, pair_b, eps=1e-9, max_iter=128, md_cap=4096, max_depth=64,
                 max_nodes=200000):
        """curves[n][3][K] (2-D curves: pass a zero z row)."""
        return self._curve_search("obtg_min_dist", curves, None, (pair_a, pair_b),
                                  (float(eps), max_iter, md_cap, max_depth, max_nodes), 3)

    def min_dist_mixed(self, curves, pair_a, pair_b, eps=1e-9, max_iter=128, md_cap=4096, max_depth=64,
                       max_nodes=200000):
        """`min_dist` on curves of different degree (obtg_min_dist_mixed): curves is a list of [3][K_i] arrays, 2 <= K_i <= 32
        (2-D curves: pass a zero z row).  The same dict as min_dist."""
        rows = [_f64(c).reshape(3, -1) for c in curves]
        off = _i32(np.concatenate(([0], np.cumsum([r.shape[1] for r in rows]))))
        cpts = _f64(np.concatenate([r.ravel() for r in rows]))
        pa, pb, n = _pairs_arg(pair_a, pair_b)
        res, info, status = _search_out(n, 3)
        self._check(self._lib.obtg_min_dist_mixed(self._h, _ptr(cpts), _ptr(off), len(rows), _ptr(pa), _ptr(pb), n, float(eps),
                                                  max_iter, md_cap, max_depth, max_nodes, _ptr(res), _ptr(info), _ptr(status)),
                    "obtg_min_dist_mixed")
        return {"res": res, "nodes": info[:, 0], "gjk_calls": info[:, 1], "depth": info[:, 2], "status": status}

    def min_dist_robust(self, curves, pair_a, pair_b, eps=1e-9, max_nodes=200000):
        """Robust branch & bound (obtg_min_dist_robust): true minimum within relative eps when status == MD_OK."""
        return self._curve_search("obtg_min_dist_robust", curves, None, (pair_a, pair_b), (float(eps), int(max_nodes)), 3,
                                  info_keys=("levels", "frontier"))

    def min_dist2poly(self, curves, pts, off, pair_curve, pair_poly, eps=1e-6, max_iter=128, md_cap=4096,
                      max_depth=64, max_nodes=200000):
        return self._curve_search("obtg_min_dist2poly", curves, (pts, off), (pair_curve, pair_poly),
                                  (float(eps), max_iter, md_cap, max_depth, max_nodes), 5)

    def min_dist2poly_robust(self, curves, pts, off, pair_curve, pair_poly, eps=1e-9, max_nodes=200000):
        """Robust curve <-> polygon distance (obtg_min_dist2poly_robust): true minimum within relative eps when MD_OK."""
        return self._curve_search("obtg_min_dist2poly_robust", curves, (pts, off), (pair_curve, pair_poly),
                                  (float(eps), int(max_nodes)), 5, info_keys=("levels", "frontier"))

    def coll_check(self, curves, pair_a, pair_b, eps=1e-9, max_iter=128, md_cap=4096, max_nodes=200000):
        """_collCheckBez2Bez (bezier.py:1561-1614) on every pair (obtg_coll_check): res[n] is the reference's return value --
        1 (no collision), -1 (its cnt > 100), 0.0 or the smallest end-point distance met -- where status is MD_OK (0 beside any
        other status).  curves[n_curves][3][K], K <= 16."""
        return self._curve_search("obtg_coll_check", curves, None, (pair_a, pair_b),
                                  (float(eps), int(max_iter), int(md_cap), int(max_nodes)), 1, zeroed=True)

    def coll_check2poly(self, curves, pts, off, pair_curve, pair_poly, max_iter=128, md_cap=4096, max_nodes=200000):
        """_collCheckBez2Poly (bezier.py:1617-1651) on every (curve, polygon) pair (obtg_coll_check2poly): res[n] is 1 (no
        collision) or 0 where status is MD_OK.  Polygons as in min_dist2poly, at most 16 vertices each; K <= 16."""
        return self._curve_search("obtg_coll_check2poly", curves, (pts, off), (pair_curve, pair_poly),
                                  (int(max_iter), int(md_cap), int(max_nodes)), 1, zeroed=True)

    def gjk_true_pairs(self, pts, off, pair_a, pair_b, eps=1e-10, max_iter=64):
        """True hull distances (obtg_gjk_true_pairs; not gjkNew).  status 0: converged with the certificate
        dist - lower <= eps * dist; 1: iteration cap; 2: stalled at rounding level before the certificate closed -- dist is
        then still a distance between hull points and `lower` a proven lower bound: check `lower` (or status)."""
        pts, off = _polys_arg(pts, off)
        pa, pb, n = _pairs_arg(pair_a, pair_b)
        flag, iters, status = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        p1, p2, dist, lower = np.empty((n, 3)), np.empty((n, 3)), np.empty(n), np.empty(n)
        self._check(self._lib.obtg_gjk_true_pairs(self._h, _ptr(pts), pts.shape[0], _ptr(off), off.shape[0] - 1, _ptr(pa), _ptr(pb),
                                                  n, float(eps), int(max_iter), _ptr(flag), _ptr(p1), _ptr(p2), _ptr(dist),
                                                  _ptr(lower), _ptr(iters), _ptr(status)), "obtg_gjk_true_pairs")
        return dict(flag=flag, c1=p1, c2=p2, dist=dist, lower=lower, iters=iters, status=status)

    # -- single-curve algebra
    def bern_elev(self, cpts, R):
        a = np.atleast_2d(_f64(cpts))
        rows, nc = a.shape
        out = np.empty((rows, nc + R))
        self._check(self._lib.obtg_bern_elev(self._h, _ptr(a), rows, nc - 1, int(R), _ptr(out)), "obtg_bern_elev")
        return out

    def bern_diff(self, cpts, T):
        a = np.atleast_2d(_f64(cpts))
        rows, nc = a.shape
        out = np.empty((rows, nc))
        self._check(self._lib.obtg_bern_diff(self._h, _ptr(a), rows, nc - 1, float(T), _ptr(out)), "obtg_bern_diff")
        return out

    def bern_mul(self, a, b):
        a = np.atleast_2d(_f64(a))
        b = np.atleast_2d(_f64(b))
        rows, mc = a.shape
        nc = b.shape[1]
        out = np.empty((rows, mc + nc - 1))
        self._check(self._lib.obtg_bern_mul(self._h, _ptr(a), _ptr(b), rows, mc - 1, nc - 1, _ptr(out)),
                    "obtg_bern_mul")
        return out

    def bern_normsq(self, x):
        x = np.atleast_2d(_f64(x))
        d, nc = x.shape
        out = np.empty((1, 2 * nc - 1))
        self._check(self._lib.obtg_bern_normsq(self._h, _ptr(x), d, nc - 1, _ptr(out)), "obtg_bern_normsq")
        return out

    def bern_split(self, cpts, z):
        """de Casteljau split of every row at parameter z in [0, 1] -> (left, right), each rows x (n+1)."""
        a = np.atleast_2d(_f64(cpts))
        rows, nc = a.shape
        left, right = np.empty((rows, nc)), np.empty((rows, nc))
        self._check(self._lib.obtg_bern_split(self._h, _ptr(a), rows, nc - 1, float(z), _ptr(left), _ptr(right)),
                    "obtg_bern_split")
        return left, right

    def bern_restrict(self, cpts, span, target):
        """Every row of cpts, a curve on span[r] = (t0, tf), cut down to target[r] = (a, e) within it (one span / target for
        all rows, or one per row) in the reference's _temporalAlignment order -> rows x (n+1) (obtg_bern_restrict)."""
        a = np.atleast_2d(_f64(cpts))
        rows, nc = a.shape
        span = np.ascontiguousarray(np.broadcast_to(_f64(span).reshape(-1, 2), (rows, 2)))
        target = np.ascontiguousarray(np.broadcast_to(_f64(target).reshape(-1, 2), (rows, 2)))
        out = np.empty((rows, nc))
        self._check(self._lib.obtg_bern_restrict(self._h, _ptr(a), rows, nc - 1, _ptr(span), _ptr(target), _ptr(out)),
                    "obtg_bern_restrict")
        return out

    def bern_eval(self, cpts, tau, t0, tf):
        """Every row of control points at every tau (obtg_bern_eval: de Casteljau per sample) -> rows x len(tau)."""
        a = np.atleast_2d(_f64(cpts))
        tau = np.atleast_1d(_f64(tau)).reshape(-1)
        rows, nc = a.shape
        out = np.empty((rows, tau.size))
        self._check(self._lib.obtg_bern_eval(self._h, _ptr(a), rows, nc - 1, _ptr(tau), tau.size, float(t0), float(tf), _ptr(out)),
                    "obtg_bern_eval")
        return out

    # -- instrumentation
    def temporal_sep_fd(self, Y0, pert_row, pert_col, pert_val, max_sep):
        """Structured finite differences: -> blk[n_pert][n_obj-1][2n+R+1] (include/obtg.h obtg_temporal_sep_fd)."""
        Y0 = _f64(Y0).reshape(self.n_veh * self.dim, self.deg + 1)
        pr = np.ascontiguousarray(pert_row, dtype=np.int32)
        pc = np.ascontiguousarray(pert_col, dtype=np.int32)
        pv = _f64(pert_val)
        n = pr.shape[0]
        out = pinned_empty((n, max(self.n_veh + self.n_obs - 1, 0), 2 * self.deg + self.deg_elev + 1))
        self._check(self._lib.obtg_temporal_sep_fd(self._h, _ptr(Y0), n, _ptr(pr), _ptr(pc), _ptr(pv),
                                                   float(max_sep), _ptr(out)), "obtg_temporal_sep_fd")
        return out

    def temporal_sep_fd_dev(self, dY0, n_pert, d_row, d_col, d_val, max_sep, d_out):
        self._check(self._lib.obtg_temporal_sep_fd_dev(self._h, _vp(dY0), int(n_pert), _vp(d_row), _vp(d_col),
                                                       _vp(d_val), float(max_sep), _vp(d_out)),
                    "obtg_temporal_sep_fd_dev")

    def set_profiling(self, on, only=None):
        """on: events around every kernel launch; only='gjk' (a kernel name): around that kernel alone."""
        mode = int(bool(on))
        if on and only is not None:
            names = [self._lib.obtg_kernel_name(k).decode() for k in range(K_END)]
            mode = 0x100 | names.index(only)
        self._check(self._lib.obtg_set_profiling(self._h, mode), "obtg_set_profiling")

    def set_profile_period(self, every):
        self._check(self._lib.obtg_set_profile_period(self._h, int(every)), "obtg_set_profile_period")

    def reset_kernel_stats(self):
        self._check(self._lib.obtg_reset_kernel_stats(self._h), "obtg_reset_kernel_stats")

    def kernel_stats(self):
        out = {}
        for k in range(K_END):
            ms = _d(0)
            n = C.c_longlong(0)
            self._check(self._lib.obtg_kernel_stats(self._h, k, C.byref(ms), C.byref(n)), "obtg_kernel_stats")
            out[self._lib.obtg_kernel_name(k).decode()] = (ms.value, n.value)
        return out


_scratch_ctx = None


def scratch_context():
    """A shape-agnostic context for the calls that do not depend on the problem shape
    (gjkNew on raw point sets, minDist, single-curve Bernstein algebra)."""
    global _scratch_ctx
    if _scratch_ctx is None:
        _scratch_ctx = Context(1, 2, 1, 0, device=default_device())
    return _scratch_ctx


def default_device():
    """The GPU of this process when nothing names one: OBTG_DEVICE, else the launcher's LOCAL_RANK (one process per GPU),
    wrapped to the devices present (a rehearsal of several ranks on one card), else 0."""
    n = max(load().obtg_device_count(), 1)
    for key in ("OBTG_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(key)
        if v is not None and v.strip().lstrip("-").isdigit():
            return int(v) % n
    return 0
