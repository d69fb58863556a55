"""ctypes loader for csrc/libumereg.so -- the C ABI declared in include/umereg.h and include/umereg_*.h: the signature table
of every header (TABLES), the loader that types them all, and the one way into an entry that returns a status (`call`, or
`checked` where the caller holds the device guard itself or the entry is host-only).

There is no fallback of any kind: if the shared object is missing or a symbol is absent the
import of the ops fails loudly, and on a box with a GPU every op raises if the library reports
an error.
"""
import ctypes
import os

# torch must come first: PyTorch-ROCm bundles its own libamdhip64.so; loading it before
# libumereg.so makes our DT_NEEDED libamdhip64.so.7 resolve to THAT runtime, so torch's streams
# and device pointers are valid inside our kernels.  (Loaded the other way round the process
# holds two HIP runtimes and ours sees no device.)
import torch  # noqa: F401

from ._build import LIB_PATH

c_void_p, c_int, c_float, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
c_double, c_int64 = ctypes.c_double, ctypes.c_int64

# name -> (restype, argtypes); mirrors include/umereg.h one to one
SIGNATURES = {
    "umereg_abi_version": (c_int, []),
    "umereg_build_source_hash": (ctypes.c_char_p, []),
    "umereg_last_error": (ctypes.c_char_p, []),
    "umereg_device_count": (c_int, [ctypes.c_char_p, c_size_t]),
    "umereg_streams_run_side_by_side": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "umereg_ball_query_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_ball_query_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                      c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_ball_query_ex_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                         c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_ume_moments_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_ume_moments_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_pack_points_f32": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_size_t, c_void_p]),
    "umereg_ume_moments_packed_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                              c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "umereg_ume_keypoint_order": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "umereg_ume_dist_q_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "umereg_ume_dist_q_f16x2": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "umereg_ume_match_f16x2": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_void_p]),
    "umereg_ume_match_q_scratch_bytes": (c_size_t, [c_int, c_int]),
    "umereg_ume_match_q_f16r": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                        c_void_p]),
    "umereg_ume_match_reset_f16": (c_int, [c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "umereg_ume_match_coarse_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "umereg_ume_match_refine_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                            c_void_p]),
    "umereg_ume_match_f16r": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_void_p]),
    "umereg_qbasis_bytes": (c_size_t, [c_int, c_int]),
    "umereg_ume_orthobasis_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "umereg_ume_cdist_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "umereg_ume_cdist_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_ume_match_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "umereg_ume_match_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_size_t, c_void_p]),
    "umereg_pair_match_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_pair_match_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_match_prob_f32": (c_int, [c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "umereg_ume_svdvals_f32": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "umereg_icp_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_icp_point_to_point_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double, c_double,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_point_to_point_dev_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double, c_double,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_state_bytes": (c_size_t, []),
    "umereg_icp_enqueue_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double, c_double, c_int, c_int,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_state_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "umereg_host_choice_round": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "umereg_host_choice_check": (c_int, [c_void_p, c_int, c_void_p]),
    "umereg_host_choice_mt19937": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "umereg_pair_match_graph_create": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "umereg_pair_match_graph_launch": (c_int, [c_void_p, c_void_p]),
    "umereg_pair_match_graph_destroy": (c_int, [c_void_p]),
    "umereg_pair_match_graph_launch_ex": (c_int, [c_void_p, c_void_p, c_void_p]),
    "umereg_pair_match_graph_launch_from": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "umereg_pair_match_graph_solve": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    # per-call matcher options (umereg_match_opts*; None = defaults)
    "umereg_ume_match_q_scratch_bytes_ex": (c_size_t, [c_int, c_int, c_void_p]),
    "umereg_ume_match_q_f16r_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                           c_void_p, c_void_p]),
    "umereg_ume_match_coarse_f16_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "umereg_ume_match_refine_f16_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                               c_void_p, c_void_p]),
    "umereg_ume_match_workspace_bytes_ex": (c_size_t, [c_int, c_int, c_int, c_void_p]),
    "umereg_ume_match_f16r_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p, c_void_p]),
    "umereg_pair_match_workspace_bytes_ex": (c_size_t, [c_int, c_int, c_void_p]),
    "umereg_pair_match_ex_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "umereg_pair_match_graph_create_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "umereg_pair_match_ragged_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                             c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                             c_void_p]),
    "umereg_pair_match_graph_create_cap": (c_int, [c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "umereg_pair_match_graph_launch_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                                      c_int, c_void_p, c_void_p]),
    "umereg_voxel_first_index_workspace_bytes": (c_size_t, [c_int]),
    "umereg_voxel_first_index_f32": (c_int, [c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_host_permutation_mt19937": (c_int, [c_void_p, c_void_p, ctypes.c_int64, ctypes.c_int64, c_void_p, c_void_p]),
    "umereg_rtume_solve_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p]),
    "umereg_hypothesis_gates_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "umereg_knn_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_knn_points_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_void_p]),
    "umereg_nn1_pair_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_nn1_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_feature_spatial_var_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                               c_size_t, c_void_p]),
    "umereg_corr_weighted_features_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_corr_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "umereg_corr_scores_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                       c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_corr_workspace_bytes_ex": (c_size_t, [c_int, c_int, c_int, c_int]),
    "umereg_corr_scores_ex_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                          c_float, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_rre_deg_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "umereg_corr_scores_profile_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                               c_float, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "umereg_corr_select_best_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
}

_FEATNET = {
    "umereg_featnet_params_count": (c_size_t, []),
    "umereg_featnet_layer_info": (c_int, [c_int, c_void_p]),
    "umereg_featnet_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_featnet_buffer": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p]),
    "umereg_featnet_build_maps": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_featnet_forward_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                           c_void_p]),
}

_FEATNET_F16 = {
    "umereg_featnet_forward_f16": _FEATNET["umereg_featnet_forward_f32"],
    "umereg_sparse_conv_f16": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p, c_int, c_int, c_void_p]),
}

_SPARSE_CONV = {
    "umereg_sparse_conv_f32": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "umereg_sparse_conv1_f32": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "umereg_sparse_conv_repack_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "umereg_sparse_conv_wgrad_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "umereg_sparse_conv_wgrad_segments": (c_int, [c_int, c_int, c_int]),
    "umereg_sparse_conv_wgrad_f32": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int,
                                             c_void_p, c_void_p, c_size_t, c_void_p]),
}

_SPARSE_CONV_F16 = {
    "umereg_sparse_conv_wgrad_f16": _SPARSE_CONV["umereg_sparse_conv_wgrad_f32"],
}

# the arguments of the union engine's entries + int f16
_SPARSE_CONV_PAIRS = {
    "umereg_featnet_forward_pairs": (c_int, _FEATNET["umereg_featnet_forward_f32"][1] + [c_int]),
    "umereg_sparse_conv_pairs": (c_int, _SPARSE_CONV["umereg_sparse_conv_f32"][1] + [c_int]),
}

_BN_ACT = {
    "umereg_bn_act_scratch_bytes": (c_size_t, [c_int, c_int]),
    "umereg_bn_act_forward_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int, c_int, c_double, c_double, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]),
    "umereg_bn_act_backward_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                           c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                           c_void_p]),
    "umereg_grad_scale_scratch_bytes": (c_size_t, [c_size_t]),
    "umereg_grad_scale_f32": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

_UME_GRAD = {
    "umereg_ume_moments_bwd_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "umereg_ume_moments_bwd_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                           c_void_p, c_size_t, c_void_p]),
    "umereg_ume_cdist_bwd_scratch_bytes": (c_size_t, [c_int, c_int]),
    "umereg_ume_cdist_bwd_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                         c_void_p]),
}

_RTUME_GRAD = {
    "umereg_rtume_solve_bwd_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
}

_GT_MATCHES = {
    "umereg_gt_matches_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "umereg_gt_matches_one_side_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_double, c_void_p, c_void_p, c_void_p,
                                               c_size_t, c_void_p]),
    "umereg_gt_matches_mutual_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_double, c_void_p, c_void_p,
                                             c_void_p, c_size_t, c_void_p]),
}

_COLLATE = {
    "umereg_collate_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "umereg_collate_element": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                       c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

_ASSIGN = {
    "umereg_assign_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "umereg_linear_sum_assignment": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_size_t, c_void_p]),
}

_SCAN_PREP = {
    "umereg_scan_prep_workspace_bytes": (c_size_t, [c_int64]),
    "umereg_scan_prep_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

_INFONCE_COMMON = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float]
_INFONCE = {
    "umereg_infonce_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "umereg_infonce_fwd_f32": (c_int, _INFONCE_COMMON + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_infonce_bwd_f32": (c_int, _INFONCE_COMMON + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

_GT_KEYPOINTS = {
    "umereg_gt_keypoints_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_gt_candidates": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_gt_select_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_gt_ball_any_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p, c_void_p]),
}

_ICP_PLANE = {
    "umereg_normals_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_estimate_normals_f32": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_plane_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_icp_point_to_plane_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double, c_double,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_point_to_plane_dev_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double,
                                                  c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_plane_enqueue_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double, c_double,
                                             c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
}

_ICP_GICP = {
    "umereg_icp_plane_to_plane_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_icp_plane_to_plane_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double,
                                              c_double, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_plane_to_plane_dev_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int,
                                                  c_double, c_double, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_size_t, c_void_p]),
    "umereg_icp_plane_to_plane_enqueue_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int,
                                                      c_double, c_double, c_float, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                                      c_void_p]),
}

# header under include/ -> {name: (restype, argtypes)}: each table mirrors its header one to one, and one .so exports them all
TABLES = {
    "umereg.h": SIGNATURES,
    "umereg_featnet.h": _FEATNET,
    "umereg_featnet_f16.h": _FEATNET_F16,
    "umereg_sparse_conv.h": _SPARSE_CONV,
    "umereg_sparse_conv_f16.h": _SPARSE_CONV_F16,
    "umereg_sparse_conv_pairs.h": _SPARSE_CONV_PAIRS,
    "umereg_bn_act.h": _BN_ACT,
    "umereg_ume_grad.h": _UME_GRAD,
    "umereg_rtume_grad.h": _RTUME_GRAD,
    "umereg_gt_matches.h": _GT_MATCHES,
    "umereg_collate.h": _COLLATE,
    "umereg_assign.h": _ASSIGN,
    "umereg_scan_prep.h": _SCAN_PREP,
    "umereg_infonce.h": _INFONCE,
    "umereg_gt_keypoints.h": _GT_KEYPOINTS,
    "umereg_icp_plane.h": _ICP_PLANE,
    "umereg_icp_gicp.h": _ICP_GICP,
}

ABI_VERSION = 2


class MatchOpts(ctypes.Structure):
    """umereg_match_opts (include/umereg.h): per-call options of the filter + refine matcher."""
    _fields_ = [("variant", ctypes.c_int32), ("splits", ctypes.c_int32), ("share_mask", ctypes.c_int64),
                ("force_exhaustive", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def __init__(self, variant=0, splits=0, share_mask=-1, force_exhaustive=0):
        super().__init__(int(variant), int(splits), int(share_mask), int(force_exhaustive), 0)

    def key(self):
        return (self.variant, self.splits, self.share_mask, self.force_exhaustive)


def opts_ptr(opts):
    """ctypes argument for a `const umereg_match_opts*` parameter (None -> NULL = the defaults)."""
    return None if opts is None else ctypes.addressof(opts)


_lib = None
_typed = []     # the signature tables typed on _lib so far (the tables themselves: they are module constants)


class NativeLibraryError(RuntimeError):
    pass


class NativeCallError(RuntimeError):
    """A status-returning entry reported `code`; the message carries the entry's name and the library's last error."""

    def __init__(self, what, code, msg):
        super().__init__(f"{what} failed (code {code}): {msg}")
        self.code = code


def _set_types(lib, signatures):
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args


def load():
    """Load (once) and type every symbol of every table of TABLES.  Raises NativeLibraryError when the .so is absent (build it
    with `python -c "import __graft_entry__ as g; g.build()"`) or lacks a symbol, which the message names."""
    global _lib, _typed
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run __graft_entry__.build()); umeregrobust_amd has no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for table in TABLES.values():
        _set_types(lib, table)
    if lib.umereg_abi_version() != ABI_VERSION:
        raise NativeLibraryError(f"ABI version mismatch: {lib.umereg_abi_version()} != {ABI_VERSION}")
    _lib, _typed = lib, list(TABLES.values())
    return lib


def load_typed(signatures):
    """load(), with the entry points of a table from outside the package typed: `signatures` is a table like SIGNATURES, typed once
    per loaded library.  Raises NativeLibraryError when the library is absent or lacks one of the symbols."""
    lib = load()
    if not any(t is signatures for t in _typed):
        _set_types(lib, signatures)
        _typed.append(signatures)
    return lib


def check(rc, what):
    if rc != 0:
        raise NativeCallError(what, rc, load().umereg_last_error().decode("utf-8", "replace"))


def checked(fn, *args):
    """Call a status-returning entry; a non-zero status raises, named by the entry itself.  No device guard and no stream query:
    for a caller that holds the guard over several calls, for the explicit-stream hot path and for host-only entries."""
    rc = fn(*args)
    if rc:
        check(rc, fn.__name__)


def call(dev, fn, *args):
    """`checked` with `dev` the current device for the duration of the call: the way into every entry that launches kernels."""
    with torch.cuda.device(dev):
        checked(fn, *args)


def stream_ptr(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def on_gpu(who, *tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: expected torch tensors, got {type(t).__name__}")
        if t.device.type != "cuda":
            raise RuntimeError(f"{who}: CPU tensors given; umeregrobust_amd has no CPU fallback (move the input to the GPU)")


def rows(t, who, what):
    """`t` as the row-major kernels read it: f32 [rows, channels] on the GPU, unit channel stride, rows 16-byte aligned"""
    if t.device.type != "cuda":
        raise RuntimeError(f"{who}: {what} on the CPU; umeregrobust_amd has no CPU fallback (move the input to the GPU)")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"{who}: {what} must be f32 [rows, channels], got {t.dtype} {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.contiguous()
    return t
