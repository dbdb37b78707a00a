"""ctypes loader of libpr_amd.so (the C ABI of include/place_recognition.h).

There is no fallback: if the shared library is missing this raises, and every entry point of the library
itself fails with PR_EHIP when no gfx950 device is usable.
"""
from __future__ import annotations

import ctypes as C
import os

PR_OK, PR_EINVAL, PR_ENOMEM, PR_EHIP, PR_EIO, PR_ENAN = 0, -1, -2, -3, -4, -5
TYPE_SC, TYPE_M2DP, TYPE_DELIGHT, TYPE_GIST, TYPE_BOW = 0, 1, 2, 3, 4
SC_ARITH_F16X2, SC_ARITH_F32, SC_ARITH_F16 = 0, 1, 2
NAN_EXCLUDE, NAN_FAIL = 0, 1
WARN_NAN_ROWS, WARN_M2DP_SVD, WARN_F16_FALLBACK, WARN_ORDER_RESOLVED, WARN_ORDER_UNRESOLVED = 1, 2, 4, 8, 16
WARN_BOW_TRUNCATED = 32
WARN_BOW_ROWS = 64     # a non-conforming BoW query row answered -1 / NaN (pr_bow_match_topk_dev)
ROLE_QUERY, ROLE_DB = 0, 1
F64, F32 = 0, 1
U8 = 2              # 8-bit images (pr_gist_generate*)
HOST, DEVICE = 0, 1
ICP_CONVERGED, ICP_MAX_ITER, ICP_TOO_FEW, ICP_DEGENERATE, ICP_NO_PAIR = 0, 1, 2, 3, 4     # pr_icp_stats.status
ICP_SEARCH_BRUTE, ICP_SEARCH_GRID = 0, 1            # pr_set_icp_search's mode
POSE_SC, POSE_M2DP, POSE_DELIGHT = 0, 1, 2          # pr_relative_pose*'s type
WINDOW_OVERFLOW, WINDOW_ORDER_GLOBAL = 1, 2         # info[3] of a pr_window push
MAP_OVERFLOW, MAP_DROPPED = 1, 2                    # info[3] of a pr_map append
ONLINE_OVERFLOW = 1                                 # info[3] of a pr_online append
ONLINE_NB = 512                                     # most workgroups of a pr_online match's rows kernel (online.hpp)
ONLINESET_FUSED, ONLINESET_DELIGHT = 0, 1             # pr_onlineset_create's kind
ONLINESET_NB_FUSED, ONLINESET_NB_DELIGHT = 512, 64  # most workgroups of a pr_onlineset match's rows kernel (onlineset.hpp): 1 / 16 entries each per stride
POSEGRAPH_OVERFLOW = 1                              # info[3] of a pr_posegraph add
POSEGRAPH_MAX_K = 128                               # most slots of one pr_posegraph add
WORLDMAP_OVERFLOW, WORLDMAP_SKIPPED, WORLDMAP_RANGE, WORLDMAP_TABLE = 1, 2, 4, 8   # flags of a pr_worldmap fuse (state[1], info[3])
MAPLOC_SKIPPED, MAPLOC_RANGE, MAPLOC_DUPLICATE, MAPLOC_TABLE = 1, 2, 4, 8           # flags of a pr_maploc index (info[2])
MAPGROW_ORDER, MAPGROW_STALE, MAPGROW_FULL = 16, 32, 64            # refusals of a pr_mapgrow extend (info[3]), beside the WORLDMAP_* bits
GATE_SRC_OVERFLOW, GATE_UNSETTLED = 1, 2           # flags of a pr_gate run (info[3])
SEQ_MAX_L, SEQ_MAX_V, SEQ_MAX_STEP, SEQ_MAX_K = 32, 16, 64, 32   # limits of a sequence-matching step table and call (PR_SEQ_*)
SEQMATCH_MAX_K = 128                                # most slots of one pr_seqmatch push
TRAJ_ALIGN_NONE, TRAJ_ALIGN_FIRST, TRAJ_ALIGN_SE3, TRAJ_ALIGN_SIM3 = 0, 1, 2, 3   # pr_trajeval_params.align
TRAJ_GT_W2C, TRAJ_GT_C2W, TRAJ_GT_POSITIONS = 0, 1, 2                         # pr_trajeval_params.gt_kind
TRAJ_FEW, TRAJ_DEGENERATE, TRAJ_NO_SCALE = 1, 2, 4                            # flags of a pr_trajeval alignment (ate[19])
PROXIMITY_QRANGE_CLAMPED = 1                                                   # flags of a pr_proximity search (info[3])
SUBMAP_TRUNCATED, SUBMAP_NO_CENTER, SUBMAP_OVERFLOW = 1, 2, 4                  # flags of a pr_submap slot (out_rows[p][1], OR-ed in info[3])
TRAJ_ATE_STATS, TRAJ_RPE_STATS, TRAJ_SEG_STATS, TRAJ_CLO_STATS = 24, 8, 4, 8   # doubles of one statistics row of a pr_trajeval run
SESSION_OVERFLOW, SESSION_REUSED, SESSION_LOG_OVERFLOW = 1, 2, 4                # flags of a pr_session begin (info[3]) and align (info[7])
SESSION_ALIGNED, SESSION_NO_TARGET, SESSION_NO_CANDIDATE, SESSION_WEAK, SESSION_NONFINITE = 0, 1, 2, 3, 4   # status of a pr_session align (info[0])
SNAPSHOT_MAP, SNAPSHOT_ONLINE, SNAPSHOT_ONLINESET, SNAPSHOT_GRAPH, SNAPSHOT_SESSION = 1, 2, 3, 4, 5   # section kinds of a pr_snapshot blob
SNAPSHOT_OVERFLOW, SNAPSHOT_BAD_MAGIC, SNAPSHOT_BAD_VERSION, SNAPSHOT_TRUNCATED, SNAPSHOT_MISSING = 1, 2, 4, 8, 16   # flags of a pr_snapshot pack / unpack (info[2])
SNAPSHOT_CAPACITY, SNAPSHOT_CHECKSUM, SNAPSHOT_OFFSETS, SNAPSHOT_SESSIONS = 32, 64, 128, 256
REGINFO_OFF, REGINFO_NONFINITE, REGINFO_TOO_FEW, REGINFO_SINGULAR, REGINFO_WEAK_ROT, REGINFO_WEAK_TRANS = 1, 2, 4, 8, 16, 32   # stat[3] of a pr_reginfo call

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PR_AMD_LIB") or os.path.join(_HERE, "libpr_amd.so")   # PR_AMD_LIB: experiment builds only

# every symbol include/place_recognition.h declares: (name, restype, argtypes)
_vp, _i32, _dbl = C.c_void_p, C.c_int32, C.c_double
SYMBOLS = {
    "pr_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "pr_create_on_stream": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "pr_set_nan_policy": (C.c_int, [_vp, C.c_int]),
    "pr_get_nan_policy": (C.c_int, [_vp]),
    "pr_set_exact_statistics": (C.c_int, [_vp, C.c_int]),
    "pr_take_warnings": (C.c_int, [_vp]),
    "pr_set_sc_binary": (C.c_int, [_vp, C.c_int]),
    "pr_sc_binary_state": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pr_set_kernel_timing": (C.c_int, [_vp, C.c_int]),
    "pr_last_distance_timing": (C.c_int, [_vp, _vp]),
    "pr_match_topk_f64": (C.c_int, [_vp, C.c_int, _vp, _i32, _vp, _i32, _i32, _dbl, _i32, _vp, _vp]),
    "pr_match_topk_fused_f64": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, _vp, _vp]),
    "pr_rerank_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, _i32, _vp,
                                _vp, _i32, _vp, _vp]),
    "pr_rerank_partial_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, _i32,
                                        _vp, _vp, _i32, _vp]),
    "pr_rerank_width": (C.c_int, [_vp, _i32]),
    "pr_f16_margin_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _dbl, _i32, _vp, _i32, _vp, _vp, _vp]),
    "pr_rerank_finish_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _dbl, _vp, _vp]),
    "pr_order_resolve_async_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _i32, _i32, _i32, _i32, _dbl, _i32, _vp, _vp]),
    "pr_order_resolve_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _i32, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp]),
    "pr_order_flagged_count": (C.c_int, [_vp, _i32, _vp]),
    "pr_order_exact_moments_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "pr_order_exact_select_dev": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, C.c_int, C.c_int, _i32, _i32, _vp]),
    "pr_order_exact_merge_dev": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_widen_scores_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "pr_merge_topk_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "pr_align_pairs_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "pr_delight_align_pairs_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "pr_match_align": (C.c_int, [_vp, C.c_int, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "pr_match_align_fused": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "pr_sc_relative_pose": (C.c_int, [_vp, _vp, _vp, _i32, _vp]),
    "pr_group_create": (C.c_int, [_vp, _i32, C.POINTER(_vp)]),
    "pr_group_destroy": (None, [_vp]),
    "pr_group_last_error": (C.c_char_p, [_vp]),
    "pr_group_size": (_i32, [_vp]),
    "pr_group_uses_rccl": (C.c_int, [_vp]),
    "pr_group_rccl_ranks": (_i32, [_vp]),
    "pr_group_last_flagged": (_i32, [_vp]),
    "pr_group_set_exact_statistics": (C.c_int, [_vp, C.c_int]),
    "pr_group_set_timing": (C.c_int, [_vp, C.c_int]),
    "pr_group_last_timing": (C.c_int, [_vp, _vp, _i32]),
    "pr_group_set_database": (C.c_int, [_vp, C.c_int, _vp, _i32]),
    "pr_group_set_database_growable": (C.c_int, [_vp, C.c_int, _vp, _i32, _i32]),
    "pr_group_append_database": (C.c_int, [_vp, _vp, _i32]),
    "pr_group_database_rows": (_i32, [_vp]),
    "pr_group_take_warnings": (C.c_int, [_vp]),
    "pr_group_match_topk": (C.c_int, [_vp, _vp, _i32, _i32, _dbl, _i32, _vp, _vp]),
    "pr_destroy": (None, [_vp]),
    "pr_last_error": (C.c_char_p, [_vp]),
    "pr_version": (C.c_char_p, []),
    "pr_set_sc_arith": (C.c_int, [_vp, C.c_int]),
    "pr_get_sc_arith": (C.c_int, [_vp]),
    "pr_sync": (C.c_int, [_vp]),
    "pr_stream": (_vp, [_vp]),
    "pr_sc_generate": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _dbl, _vp]),
    "pr_m2dp_generate": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _dbl, _vp]),
    "pr_m2dp_svd_rows": (C.c_int, [_vp, _vp, _i32, _vp]),
    "pr_delight_generate": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp]),
    "pr_gist_signature_size": (C.c_int, [_i32, _i32, _vp]),
    "pr_gist_generate": (C.c_int, [_vp, _vp, C.c_int, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_gist_generate_dev": (C.c_int, [_vp, _vp, C.c_int, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_bow_vocab_load": (C.c_int, [C.c_char_p, C.POINTER(_vp)]),
    "pr_bow_vocab_save_bin": (C.c_int, [_vp, C.c_char_p]),
    "pr_bow_vocab_create": (C.c_int, [_i32, _i32, _i32, _i32, C.c_int64, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "pr_bow_vocab_info": (C.c_int, [_vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pr_bow_vocab_export": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "pr_bow_vocab_destroy": (None, [_vp]),
    "pr_bow_generate": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "pr_bow_generate_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, _i32, _i32, _vp, _vp, _vp]),
    "pr_delight_distance": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp]),
    "pr_gist_distance": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "pr_bow_distance": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "pr_match_topk_fused": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, _vp, _vp]),
    "pr_fuse_select2_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _dbl, _i32, _vp, _vp]),
    "pr_fuse_select2_f64_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp]),
    "pr_fuse_select_f64_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp]),
    "pr_match_topk_cols": (C.c_int, [_vp, C.c_int, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_bow_db_create": (C.c_int, [_vp, _i32, _i32, _i32, C.c_int64, C.POINTER(_vp)]),
    "pr_bow_db_destroy": (None, [_vp, _vp]),
    "pr_bow_db_set": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32]),
    "pr_bow_db_append": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32]),
    "pr_bow_db_count": (_i32, [_vp]),
    "pr_bow_match_topk_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_bow_match_topk_f64": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_bow_distance_f64": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "pr_gist_db_create": (C.c_int, [_vp, _i32, _i32, C.POINTER(_vp)]),
    "pr_gist_db_destroy": (None, [_vp, _vp]),
    "pr_gist_db_set": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32]),
    "pr_gist_db_append": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32]),
    "pr_gist_db_count": (_i32, [_vp]),
    "pr_gist_db_bytes": (C.c_int64, [_vp]),
    "pr_gist_db_set_exact": (None, [_vp, C.c_int]),
    "pr_gist_match_topk_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_gist_flagged_count": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "pr_gist_match_topk_f64": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_gist_distance_f64": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "pr_delight_db_create": (C.c_int, [_vp, _i32, C.POINTER(_vp)]),
    "pr_delight_db_destroy": (None, [_vp, _vp]),
    "pr_delight_db_set": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32]),
    "pr_delight_db_append": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32]),
    "pr_delight_db_count": (_i32, [_vp]),
    "pr_delight_db_bytes": (C.c_int64, [_vp]),
    "pr_delight_db_set_exact": (None, [_vp, C.c_int]),
    "pr_delight_match_topk_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pr_delight_flagged_count": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "pr_delight_match_topk_f64": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "pr_delight_distance_f64": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp]),
    "pr_delight_generate_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp]),
    "pr_sc_distance": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp]),
    "pr_m2dp_distance": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp]),
    "pr_match_topk": (C.c_int, [_vp, C.c_int, _vp, _i32, _vp, _i32, _i32, _dbl, _i32, _vp, _vp]),
    "pr_sigset_create": (C.c_int, [_vp, C.c_int, C.c_int, _i32, C.POINTER(_vp)]),
    "pr_sigset_destroy": (None, [_vp, _vp]),
    "pr_sigset_pack": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _i32]),
    "pr_sigset_count": (_i32, [_vp]),
    "pr_sigset_reserve": (C.c_int, [_vp, _vp]),
    "pr_sigset_append": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _i32]),
    "pr_sigset_image": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t), C.POINTER(_i32)]),
    "pr_distances_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "pr_row_moments_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "pr_moments_select_f64_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp]),
    "pr_select_fallback_rows": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "pr_fuse_select_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _dbl, _i32, _vp, _vp]),
    "pr_sc_generate_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _dbl, _vp]),
    "pr_m2dp_generate_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _dbl, _vp]),
    "pr_cloud_frames_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp]),
    "pr_sc_generate_frames_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _dbl, _vp, C.c_int, _vp]),
    "pr_m2dp_generate_frames_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _dbl, _vp, C.c_int, _vp]),
    "pr_delight_generate_frames_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "pr_generate_clouds": (C.c_int, [_vp, C.c_int, _vp, _dbl, _vp]),
    "pr_clouds_dev_xyz": (_vp, [_vp]),
    "pr_clouds_dev_inten": (_vp, [_vp]),
    "pr_clouds_dev_offs": (_vp, [_vp]),
    "pr_clouds_dev_frames": (_vp, [_vp]),
    "pr_pts_preprocess": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, _dbl, C.c_int, C.c_int, C.POINTER(_vp)]),
    "pr_pts_preprocess_gpu": (C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_char_p, _dbl, C.c_int, C.c_int, C.POINTER(_vp)]),
    "pr_hash_order": (C.c_int, [_vp, _i32, _vp]),
    "pr_window_create": (C.c_int, [_vp, _dbl, C.c_int, _i32, _i32, _i32, C.POINTER(_vp)]),
    "pr_window_destroy": (None, [_vp]),
    "pr_window_reset": (C.c_int, [_vp]),
    "pr_window_count": (C.c_int, [_vp, C.POINTER(_i32)]),
    "pr_window_push_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "pr_window_push": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, C.POINTER(_i32), _vp, _vp]),
    "pr_clouds_avg_ms": (C.c_double, [_vp]),
    "pr_clouds_avg_pts": (C.c_double, [_vp]),
    "pr_clouds_count": (C.c_int64, [_vp]),
    "pr_clouds_offs": (C.POINTER(C.c_int64), [_vp]),
    "pr_clouds_xyz": (C.POINTER(C.c_double), [_vp]),
    "pr_clouds_inten": (C.POINTER(C.c_float), [_vp]),
    "pr_clouds_ids": (C.POINTER(C.c_int32), [_vp]),
    "pr_clouds_free": (None, [_vp]),
    "pr_write_signatures": (C.c_int, [C.c_char_p, _vp, C.c_int64, C.c_int64]),
    "pr_read_signatures": (C.c_int, [C.c_char_p, C.POINTER(_vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pr_free": (None, [_vp]),
    "pr_write_signatures_bin": (C.c_int, [C.c_char_p, _vp, C.c_int64, C.c_int64, C.c_int]),
    "pr_read_signatures_bin": (C.c_int, [C.c_char_p, C.POINTER(_vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pr_write_poses": (C.c_int, [C.c_char_p, _vp, _vp, C.c_int64]),
    "pr_write_points": (C.c_int, [C.c_char_p, _vp, _vp, _vp, C.c_int64]),
    "pr_precision_recall": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, C.POINTER(_dbl), C.POINTER(_dbl), _vp,
                                      C.POINTER(_i32)]),
    "pr_ground_truth_pairs_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _vp]),
    "pr_precision_recall_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _vp, _vp]),
    "pr_trapz_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp]),
    "pr_ground_truth_pairs": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _vp]),
    "pr_precision_recall_gpu": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, C.POINTER(_dbl), C.POINTER(_dbl), _vp,
                                          C.POINTER(_i32), _vp, C.POINTER(_i32), _vp, _vp]),
    "pr_eval_tile_rows": (_i32, []),
    "pr_set_eval_path": (C.c_int, [_vp, C.c_int, C.c_int]),
    "pr_icp_nn_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "pr_icp_pairs_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _dbl, _dbl, _dbl, _i32, _vp, _vp]),
    "pr_icp_nn": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "pr_icp_pairs": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _dbl, _dbl, _dbl, _i32, _vp, _vp]),
    "pr_icp_tile_rows": (_i32, []),
    "pr_set_icp_path": (C.c_int, [_vp, C.c_int]),
    "pr_set_icp_search": (C.c_int, [_vp, C.c_int]),
    "pr_get_icp_search": (C.c_int, [_vp]),
    "pr_icp_nn_radius_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _dbl, _vp, _vp, _vp]),
    "pr_icp_nn_radius": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _dbl, _vp, _vp, _vp]),
    "pr_relative_pose": (C.c_int, [C.c_int, _vp, _vp, _vp, _i32, _vp]),
    "pr_relative_pose_dev": (C.c_int, [_vp, C.c_int, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "pr_verify_select_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp]),
    "pr_verify_pairs_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32,
                                      _i32, _dbl, _dbl, _dbl, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp]),
    "pr_map_create": (C.c_int, [_vp, _vp, _i32, C.c_int64, _i32, _i32, C.POINTER(_vp)]),
    "pr_map_destroy": (None, [_vp]),
    "pr_map_reset": (C.c_int, [_vp]),
    "pr_map_count": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(C.c_int64), C.POINTER(_i32)]),
    "pr_map_append_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_int64, _vp]),
    "pr_map_append": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "pr_map_verify_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _dbl, _dbl, _dbl, _i32, _dbl,
                                    _dbl, _vp, _vp, _vp, _vp]),
    "pr_online_create": (C.c_int, [_vp, C.c_int, _vp, _i32, _i32, C.POINTER(_vp)]),
    "pr_online_destroy": (None, [_vp]),
    "pr_online_reset": (C.c_int, [_vp]),
    "pr_online_count": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "pr_online_match_dev": (C.c_int, [_vp, _vp, _vp, _i32, _dbl, _i32, _vp, _vp, _vp]),
    "pr_online_append_dev": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pr_online_append": (C.c_int, [_vp, _vp, _vp]),
    "pr_onlineset_create": (C.c_int, [_vp, C.c_int, _vp, _i32, _i32, C.POINTER(_vp)]),
    "pr_onlineset_destroy": (None, [_vp]),
    "pr_onlineset_reset": (C.c_int, [_vp]),
    "pr_onlineset_count": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "pr_onlineset_match_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _dbl, _i32, _vp, _vp, _vp]),
    "pr_onlineset_append_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_onlineset_append": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "pr_posegraph_create": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(_vp)]),
    "pr_posegraph_destroy": (None, [_vp]),
    "pr_posegraph_reset": (C.c_int, [_vp]),
    "pr_posegraph_count": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "pr_posegraph_add_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _dbl, _dbl, _vp]),
    "pr_posegraph_add": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _dbl, _dbl, _vp]),
    "pr_posegraphw_add_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "pr_posegraphw_add": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "pr_posegraph_relax_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_worldmap_create": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.POINTER(_vp)]),
    "pr_worldmap_destroy": (None, [_vp]),
    "pr_worldmap_scratch_bytes": (C.c_int64, [_i32, C.c_int64]),
    "pr_worldmap_count": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(_i32)]),
    "pr_worldmap_fuse_dev": (C.c_int, [_vp, _vp, _vp, _dbl, _i32, _i32, _vp]),
    "pr_worldmap_fuse": (C.c_int, [_vp, _vp, _vp, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_maploc_create": (C.c_int, [_vp, _vp, C.c_int64, _dbl, _i32, _i32, C.POINTER(_vp)]),
    "pr_maploc_destroy": (None, [_vp]),
    "pr_maploc_scratch_bytes": (C.c_int64, [C.c_int64, _i32, _i32]),
    "pr_maploc_count": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(_i32)]),
    "pr_maploc_index_dev": (C.c_int, [_vp, _vp]),
    "pr_maploc_seed_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "pr_maploc_nn_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _dbl, _vp, _vp, _vp]),
    "pr_maploc_refine_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _dbl, _dbl, _dbl, _i32, _vp, _vp]),
    "pr_maploc_index": (C.c_int, [_vp, _vp]),
    "pr_maploc_nn": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _dbl, _vp, _vp, _vp]),
    "pr_maploc_refine": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _dbl, _dbl, _dbl, _i32, _vp, _vp]),
    "pr_mapplane_create": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "pr_mapplane_destroy": (None, [_vp]),
    "pr_mapplane_scratch_bytes": (C.c_int64, [_i32, _i32]),
    "pr_mapplane_normals_dev": (C.c_int, [_vp, _dbl, _i32, _dbl, _vp, _vp]),
    "pr_mapplane_refine_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _dbl, _dbl, _dbl, _i32, _vp, _vp, _vp, _vp]),
    "pr_mapplane_normals": (C.c_int, [_vp, _dbl, _i32, _dbl, _vp, _vp]),
    "pr_mapplane_refine": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _dbl, _dbl, _dbl, _i32, _vp, _vp, _vp, _vp]),
    "pr_reginfo_create": (C.c_int, [_vp, _i32, _i32, C.POINTER(_vp)]),
    "pr_reginfo_destroy": (None, [_vp]),
    "pr_reginfo_scratch_bytes": (C.c_int64, [_i32, _i32]),
    "pr_reginfo_point_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_reginfo_plane_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _dbl, _i32, _dbl, _dbl, _dbl,
                                       _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_reginfo_point": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_reginfo_plane": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _dbl, _i32, _dbl, _dbl, _dbl,
                                   _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_mapgrow_create": (C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    "pr_mapgrow_destroy": (None, [_vp]),
    "pr_mapgrow_scratch_bytes": (C.c_int64, [_i32]),
    "pr_mapgrow_sync_dev": (C.c_int, [_vp, _vp]),
    "pr_mapgrow_extend_dev": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pr_mapgrow_normals_dev": (C.c_int, [_vp, _dbl, _i32, _dbl, _vp, _vp]),
    "pr_mapgrow_extend": (C.c_int, [_vp, _vp, _i32, _vp]),
    "pr_mapgrow_normals": (C.c_int, [_vp, _dbl, _i32, _dbl, _vp, _vp]),
    "pr_mapgrow_count": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(C.c_int64), C.POINTER(_i32)]),
    "pr_gate_create": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "pr_gate_run_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_gate_run": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_gate_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "pr_gate_destroy": (None, [_vp]),
    "pr_seq_select_dev": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _vp]),
    "pr_seq_tile": (None, [C.POINTER(_i32), C.POINTER(_i32)]),
    "pr_match_topk_seq_f64": (C.c_int, [_vp, C.c_int, _vp, _i32, _vp, _i32, _i32, _dbl, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "pr_seqmatch_create": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, C.POINTER(_vp)]),
    "pr_seqmatch_push_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "pr_seqmatch_push": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "pr_seqmatch_reset": (C.c_int, [_vp]),
    "pr_seqmatch_read": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pr_seqmatch_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32]),
    "pr_seqmatch_destroy": (None, [_vp]),
    "pr_host_last_error": (C.c_char_p, []),
    "pr_trajeval_create": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "pr_trajeval_run_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_trajeval_run": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_trajeval_scratch_bytes": (C.c_size_t, [_vp]),
    "pr_trajeval_destroy": (None, [_vp]),
    "pr_proximity_create": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(_vp)]),
    "pr_proximity_destroy": (None, [_vp]),
    "pr_proximity_scratch_bytes": (C.c_int64, [_i32, _i32, _i32]),
    "pr_proximity_tile": (None, [C.POINTER(_i32), C.POINTER(_i32)]),
    "pr_proximity_search_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_proximity_search": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_posegraphb_add_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _i32, _vp]),
    "pr_posegraphb_add": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _i32, _vp]),
    "pr_submap_create": (C.c_int, [_vp, _i32, _i32, C.c_int64, _i32, _i32, C.POINTER(_vp)]),
    "pr_submap_destroy": (None, [_vp]),
    "pr_submap_scratch_bytes": (C.c_int64, [_i32, _i32]),
    "pr_submap_build_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "pr_submap_build": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "pr_session_create": (C.c_int, [_vp, _vp, _i32, _i32, _i32, C.POINTER(_vp)]),
    "pr_session_destroy": (None, [_vp]),
    "pr_session_reset": (C.c_int, [_vp]),
    "pr_session_count": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "pr_session_scratch_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "pr_session_begin_dev": (C.c_int, [_vp, _vp, _vp]),
    "pr_session_begin": (C.c_int, [_vp, _vp, _vp]),
    "pr_session_align_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_session_align": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_session_relax_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_snapshot_create": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "pr_snapshot_destroy": (None, [_vp]),
    "pr_snapshot_bound": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "pr_snapshot_desc_bound": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "pr_snapshot_pack_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "pr_snapshot_unpack_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "pr_snapshot_save": (C.c_int, [_vp, C.c_char_p]),
    "pr_snapshot_load": (C.c_int, [_vp, C.c_char_p, _vp]),
}



class MapBuffers(C.Structure):
    """pr_map_buffers: the seven caller-owned device buffers of a pr_map."""
    _fields_ = [(n, _vp) for n in ("xyz", "inten", "offs", "frames", "poses", "ids", "state")]


class OnlineBuffers(C.Structure):
    """pr_online_buffers: the two caller-owned device buffers of a pr_online."""
    _fields_ = [(n, _vp) for n in ("sig", "state")]


class OnlineSetBuffers(C.Structure):
    """pr_onlineset_buffers: the caller-owned device buffers of a pr_onlineset (the parts its kind does not have are NULL)."""
    _fields_ = [(n, _vp) for n in ("sc", "m2dp", "delight", "state")]


class PoseGraphBuffers(C.Structure):
    """pr_posegraph_buffers: the four caller-owned device buffers of a pr_posegraph."""
    _fields_ = [(n, _vp) for n in ("edge_ij", "edge_Z", "edge_w", "state")]


class WorldMapBuffers(C.Structure):
    """pr_worldmap_buffers: the six caller-owned device buffers of a pr_worldmap."""
    _fields_ = [(n, _vp) for n in ("xyz", "inten", "src", "row", "count", "state")]


class PoseGraphParams(C.Structure):
    """pr_posegraph_params: the budgets and weights of one pr_posegraph_relax_dev (filled by position: `lambda` is no Python name)."""
    _fields_ = [("outer", _i32), ("inner", _i32), ("lambda", _dbl), ("w_odo_rot", _dbl), ("w_odo_trans", _dbl)]


class GateParams(C.Structure):
    """pr_gate_params: what a pr_gate fixes at create."""
    _fields_ = [("max_gap", _i32), ("min_support", _i32), ("rounds", _i32)]


class TrajEvalParams(C.Structure):
    """pr_trajeval_params: what a pr_trajeval fixes at create."""
    _fields_ = [(n, _i32) for n in ("node_capacity", "batch", "align", "gt_kind", "n_deltas", "n_lengths", "step", "edge_capacity")] + \
               [("rot_thr", _dbl), ("trans_thr", _dbl)]


class ProximityParams(C.Structure):
    """pr_proximity_params: the rule's numbers of one pr_proximity search."""
    _fields_ = [(n, _dbl) for n in ("radius", "growth", "radius_max", "cos_min")] + [(n, _i32) for n in ("min_gap", "stride", "k", "known_window")]


class SubmapParams(C.Structure):
    """pr_submap_params: the rule's numbers of one pr_submap build."""
    _fields_ = [(n, _i32) for n in ("half_window", "past_only", "avoid_gap", "max_pts")]


class SessionBuffers(C.Structure):
    """pr_session_buffers: the two caller-owned device buffers of a pr_session."""
    _fields_ = [(n, _vp) for n in ("start", "state")]


class SessionAlignParams(C.Structure):
    """pr_session_align_params: the rule's numbers of one pr_session align."""
    _fields_ = [("session", _i32), ("min_inliers", _i32), ("rot_c_max", _dbl), ("trans2_max", _dbl)]


class SnapshotDesc(C.Structure):
    """pr_snapshot_desc: pointers to the buffer records of the parts a pr_snapshot covers (NULL: not covered) and their create capacities."""
    _fields_ = [("map", _vp), ("keyframe_capacity", _i32), ("max_cloud_points", _i32), ("point_capacity", C.c_int64),
                ("online", _vp * 2), ("online_type", _i32 * 2), ("online_capacity", _i32 * 2),
                ("onlineset", _vp), ("onlineset_kind", _i32), ("onlineset_capacity", _i32),
                ("graph", _vp * 2), ("edge_capacity", _i32 * 2), ("sessions", _vp), ("session_capacity", _i32), ("reserved", _i32)]


class TrajEvalOut(C.Structure):
    """pr_trajeval_out: the nine output arrays of a pr_trajeval run (device pointers for run_dev, host pointers for run)."""
    _fields_ = [(n, _vp) for n in ("ate", "rpe", "seg", "clo", "err", "seg_end", "edge_err", "centres", "prefix")]


_lib = None
HIP_RUNTIME = "system"      # which libamdhip64 this process ended up on (_one_hip_runtime)


class PRError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libpr_amd error {code}: {msg}")
        self.code = code


def _one_hip_runtime():
    """A process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so.7 (same SONAME as /opt/rocm's, which
    libpr_amd.so is linked against): whichever copy is loaded first serves both, and torch does not find its GPUs on the other one
    ("No HIP GPUs are available" when libpr_amd.so came first).  So when torch is installed but not imported yet, its copy is loaded
    here - without importing torch - and both end up on it whatever the import order.  This is a process-wide choice made on behalf of a
    caller who may never import torch: PR_AMD_SYSTEM_HIP=1 keeps /opt/rocm's (the runtime the kernels were built against), HIP_RUNTIME
    records which one was taken, PR_AMD_VERBOSE=1 prints it."""
    import importlib.util
    import sys
    global HIP_RUNTIME
    if "torch" in sys.modules:
        HIP_RUNTIME = "torch's (torch was imported first)"
        return
    if os.environ.get("PR_AMD_SYSTEM_HIP"):
        HIP_RUNTIME = "system (PR_AMD_SYSTEM_HIP)"
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    for d in (spec.submodule_search_locations or []) if spec else []:
        p = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)
            HIP_RUNTIME = p
            if os.environ.get("PR_AMD_VERBOSE"):
                print(f"so_dso_place_recognition_amd: HIP runtime {p} (torch's copy, so that a later `import torch` finds its GPUs; "
                      "PR_AMD_SYSTEM_HIP=1 keeps /opt/rocm's)", file=sys.stderr)
            return


def load() -> C.CDLL:
    """Loads libpr_amd.so and binds every declared symbol (raises if the library or a symbol is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not found: build it with `make -C so_dso_place_recognition_amd/csrc` "
                      "(or __graft_entry__.build()); there is no CPU fallback")
    _one_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(ctx, rc: int):
    if rc != PR_OK:
        msg = load().pr_last_error(ctx)
        raise PRError(rc, msg.decode() if msg else "")
