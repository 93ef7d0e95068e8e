"""ctypes binding of csrc/libpit_hip.so (C ABI declared in include/pit_hip.h).

There is no fallback: if the library is missing or a symbol is absent this raises, and
every op in this package goes through it.  torch is imported first so that the HIP
runtime already loaded by PyTorch-ROCm is the one the library binds to."""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIT_LIB_PATH") or os.path.join(_HERE, "csrc", "libpit_hip.so")   # (override: diagnostic builds, tools/)

_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_long
_F = ctypes.c_float
_LL = ctypes.c_longlong
_D = ctypes.c_double

class MlpParamsJob(ctypes.Structure):
    """pit_mlp_params_job of include/pit_hip.h (the argument list of pit_mlp_bwd_params)."""
    _fields_ = [("x", _P), ("ldx", _L), ("rows", _I), ("n0", _I), ("n1", _I), ("n2", _I), ("h", _P), ("out_gelu", _I),
                ("d_y", _P), ("ld_dy", _L), ("d_w1", _P), ("d_b1", _P), ("d_w2", _P), ("d_b2", _P),
                ("accumulate", _I), ("scratch", _P), ("math_mode", _I)]


class BlockWeightsJob(ctypes.Structure):
    """pit_block_weights_job of include/pit_hip.h (the argument list of pit_block_weights)."""
    _fields_ = [("mesh", _P), ("n_pts", _I), ("space_dim", _I), ("metric", _I), ("period", _F),
                ("n_layers", _I), ("heads", _P), ("head_is_scale", _I), ("n_head", _I),
                ("e", _P), ("q", _P), ("inv", _P), ("rowstat", _P), ("scale_out", _P)]


class SlabPlan(ctypes.Structure):
    """pit_slab_plan of include/pit_hip.h (the static per-slab plan of a masked cross-attention layer on a fixed mesh pair)."""
    _fields_ = [("n_out", _I), ("n_in", _I), ("cap", _I), ("n_slabs", _I), ("umax", _I), ("stats", _P), ("rank_w", _F),
                ("idx", _P), ("cnt", _P), ("m", _P), ("slot", _P), ("keys", _P), ("nkeys", _P), ("rows", _I),
                ("grid_w", _I), ("grid_h", _I), ("patch_w", _I), ("patch_h", _I)]       # (all 0: consecutive rows)


class DecoderWeightsJob(ctypes.Structure):
    """pit_decoder_weights_job of include/pit_hip.h (the argument list of pit_decoder_weights)."""
    _fields_ = [("plan", _P), ("head", _P), ("head_is_scale", _I), ("n_head", _I), ("max_union", _I), ("max_count", _I),
                ("pw", _P), ("qw", _P), ("scale_out", _P), ("w1", _P), ("w1f", _P), ("dim", _I)]


# The argument groups that recur in the layer entries beside the main mesh path (ragged, distance matrix, candidate lists), in
# the header's order: their types here, their values in the *_args builders below SIGNATURES.
_VALUES = [_P, _I, _L, _L]                 # values, dim, ld_values, values_bstride
_VALUES_B = [_P, _I, _I, _L, _L]           # values, batch, dim, ld_values, values_bstride
_HEAD = [_P, _I, _I]                       # head, n_head, head_is_scale
_HEAD_BWD = _HEAD + [_P]                   # ..., scale
_STATS = [_P, _F, _I]                      # stats, rank_w, masked
_STATS_RAGGED = [_P, _P, _I]               # (rank_w per sample, on the device)
_STATS_BWD = [_P, _I]                      # rowstat, masked
_OUT = [_P, _L, _L, _I, _I, _P, _P]        # out, ld_out, out_bstride, out_col0, copy_inputs, rowstat, scale_out
_DOUT = [_P, _L, _L, _I]                   # d_out, ld_dout, dout_bstride, out_col0
_DVALUES = [_P, _L, _L, _I]                # d_values, ld_dvalues, dvalues_bstride, add_residual
_DHEAD = [_P, _I, _P]                      # d_head, accumulate_head, workspace
_SAVED_OUT = [_P, _L, _L]                  # out, ld_out, out_bstride (the forward's result, read by d(m) / d(sqd))
_TAIL = [_I, _P]                           # math_mode, stream
_RAGGED = [_P, _P, _I, _I, _I, _I, _P, _P]                  # mesh_out, mesh_in, mesh_batch, n_out, n_in, space_dim, len_out, len_in
_RAGGED_STRIDED = _RAGGED[:6] + [_L, _L] + _RAGGED[6:]      # ..., out_stride, in_stride, len_out, len_in
_RAGGED_LISTS = [_P, _P, _I]                                # nbr_idx, nbr_cnt, nbr_cap
_MAT = [_P, _L, _L, _I, _I]                                 # m, ld_m, m_bstride, n_out, n_in
_LIST = [_P, _P, _L, _L, _I, _I, _I]                        # idx, sqd, ld, bstride, cap, n_out, n_in
_FWD_RAGGED = _VALUES + _HEAD + _STATS_RAGGED + _OUT + _RAGGED_LISTS + _TAIL
_BWD_RAGGED = _VALUES + _HEAD_BWD + _STATS_BWD + _DOUT + _DVALUES + _DHEAD + _RAGGED_LISTS + [_P, _P] + _TAIL      # ..., rev_ptr, rev_row
_FWD_DIST = _VALUES_B + _HEAD + _STATS + _OUT + _TAIL
_BWD_DIST = _VALUES_B + _HEAD_BWD + _STATS_BWD + _DOUT + _DVALUES + _DHEAD

# name -> argtypes, mirrors include/pit_hip.h one to one
SIGNATURES = {
    "pit_version": [],
    "pit_error_string": [_I],
    "pit_head_scale": [_P, _I, _P, _P],
    "pit_select_fwd": [_P, _P, _I, _I, _I, _I, _I, _F, _I, _I, _P, _P],
    "pit_select_wide_fwd": [_P, _P, _I, _I, _I, _I, _I, _F, _I, _I, _P, _P],
    "pit_plan_fwd": [_P, _P, _I, _I, _I, _I, _I, _F, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P],
    "pit_lists_transpose": [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P],
    "pit_neighbors_fwd": [_P, _P, _I, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _P, _P],
    "pit_posatt_fwd": [_P, _P, _I, _I, _I, _I, _I, _F,
                       _P, _I, _I, _L, _L,
                       _P, _I, _I,
                       _P, _F, _I, _I,
                       _P, _L, _L, _I, _I,
                       _P, _P, _P, _P, _I, _I, _I, _P],
    "pit_posatt_fwd_job": [_P, _P, _I, _I, _I, _I, _I, _F,
                           _P, _I, _I, _L, _L,
                           _P, _I, _I,
                           _P, _F, _I, _I,
                           _P, _L, _L, _I, _I,
                           _P, _P, _P, _P, _I, _I, _I, _P, _P],
    "pit_posatt_bwd": [_P, _P, _I, _I, _I, _I, _I, _F,
                       _P, _I, _I, _L, _L,
                       _P, _I, _I, _P,
                       _P, _I,
                       _P, _L, _L, _I,
                       _P, _L, _L, _I,
                       _P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _P],
    "pit_posatt_dmesh": [_P, _P, _I, _I, _I, _I, _I, _F,
                         _P, _I, _I, _L, _L,
                         _P, _I, _I, _P,
                         _P, _I,
                         _P, _L, _L, _I,
                         _P, _P, _I, _I, _P, _P,
                         _P, _P, _I, _P, _P],
    "pit_posatt_dmesh_workspace": [_I, _I, _I, _I, _I, _I],
    "pit_posatt_dhead_finish": [_I, _P, _P, _P, _P, _P, _P, _P, _P],
    "pit_block_supported": [_I, _I, _I, _I],
    "pit_block_weights": [_P, _I, _I, _I, _F, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P],
    "pit_block_fwd": [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _L, _I, _P],
    "pit_slab_plan_build": [_P, _P, _I, _I, _I, _I, _F, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P],
    "pit_decoder_union_slots": [_P, _I],
    "pit_slab_plan_build_patch": [_P, _P, _I, _I, _I, _I, _F, _P, _P, _I, _I, _I, _I, _I, _P, _F, _P, _P, _P, _P, _P, _P],
    "pit_fold_supported": [_I, _I, _I, _I, _I],
    "pit_fold_weights": [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "pit_fold_att_fwd": [_P, _P, _L, _L, _I, _I, _I, _P, _P, _L, _L, _I, _I, _P],
    "pit_fold_att_bwd": [_P, _P, _L, _L, _I, _I, _I, _P, _P, _P, _L, _L, _P, _L, _L, _P, _P, _P, _P, _I, _I, _P],
    "pit_thin_tail_scratch_floats": [],
    "pit_thin_tail_fwd": [_P, _L, _I, _I, _I, _P, _P, _P, _P, _L, _I, _P],
    "pit_thin_tail_bwd": [_P, _L, _I, _I, _I, _P, _P, _P, _L, _P, _L, _P, _P, _P, _P, _I, _P],
    "pit_satt_supported": [_I, _I, _I, _I, _I],
    "pit_satt_fwd": [_P, _I, _I, _I, _I, _F, _P, _L, _L, _I, _I, _P, _I, _I, _P, _P, _L, _L, _I, _I, _P, _P, _P, _I, _P],
    "pit_satt_bwd": [_P, _I, _I, _I, _I, _F, _I, _I, _P, _I, _P, _P, _P, _P, _L, _L, _I, _P, _L, _L, _I, _P, _P, _I, _P, _P],
    "pit_satt_tiles_elems": [_I],
    "pit_mlp_chain_supported": [_I, _I, _I, _I],
    "pit_mlp_chain_fwd": [_P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P],
    "pit_mlp_chain_bwd": [_I, _I, _I, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P, _I, _I, _P],
    "pit_cast_bf16_multi": [_I, _P, _P, _P, _P],
    "pit_linear_fwd": [_P, _L, _I, _I, _I, _P, _P, _P, _L, _I, _P],
    "pit_linear_bwd": [_P, _L, _I, _I, _I, _P, _P, _L, _P, _L, _P, _I, _I, _P],
    "pit_edge_supported": [_I, _I, _I, _I],
    "pit_decoder_weights": [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P],
    "pit_decoder_fwd": [_P, _P, _L, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _L,
                        _P, _P, _P, _I, _P, _I, _P],
    "pit_decoder_bwd": [_P, _P, _L, _L, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _L, _P, _P, _L, _P,
                        _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P],
    "pit_union_att_supported": [_I, _I, _I, _I],
    "pit_union_att_fwd": [_P, _P, _L, _L, _I, _I, _I, _P, _P, _L, _L, _I, _I, _P],
    "pit_union_att_bwd": [_P, _P, _L, _L, _I, _I, _I, _P, _P, _P, _L, _L, _I, _P, _L, _L, _P, _I, _P],
    "pit_encoder_fwd": [_P, _P, _I, _I, _P, _L, _L, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P,
                        _P, _P, _P, _P, _P, _L, _P, _P, _P, _L, _P, _P, _P],
    "pit_encoder_bwd": [_P, _P, _I, _I, _P, _L, _L, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P],
    "pit_posatt_pre_supported": [_I, _I, _I, _I],
    "pit_posatt_pre_fwd": [_P, _P, _I, _I, _I, _I, _P, _L, _L, _P, _L, _L, _I, _I, _I, _P],
    "pit_posatt_pre_bwd": [_P, _P, _P, _I, _I, _I, _I, _P, _L, _L, _P, _L, _L, _I, _P, _L, _L, _I, _P, _I, _P],
    "pit_block_bwd": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _L, _P, _P, _L, _P, _P, _I, _P],
    "pit_mlp_bf16_io_supported": [_I, _I, _I, _I, _I],
    "pit_mlp_fwd": [_P, _L, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _L, _I, _P],
    "pit_mlp_bwd": [_P, _L, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _L,
                    _P, _L, _P, _P, _P, _P, _I, _P, _I, _P],
    "pit_mlp_bwd_data": [_I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _L, _P, _L, _P, _I, _P],
    "pit_mlp_bwd_params": [_P, _L, _I, _I, _I, _I, _P, _I, _P, _L, _P, _P, _P, _P, _I, _P, _I, _P],
    "pit_mlp_bwd_params_ordered": [_P, _L, _I, _I, _I, _I, _P, _I, _P, _L, _P, _P, _P, _P, _I, _P, _P, _P],
    "pit_mlp_bwd_params_ordered_workspace": [_I, _I, _I, _I],
    "pit_mlp_bwd_params_ordered_mfma": [_P, _L, _I, _I, _I, _I, _P, _I, _P, _L, _P, _P, _P, _P, _I, _P, _P, _P],
    "pit_mlp_bwd_params_ordered_mfma_workspace": [_I, _I, _I, _I],
    "pit_lists_sort_ranges": [_P, _P, _I, _I, _L, _P, _P],
    "pit_posatt_overflow_dv_ordered": [_P, _P, _I, _I, _I, _I, _I, _F, _I, _I, _P, _I, _I, _P, _P,
                                       _P, _L, _L, _I, _P, _L, _L, _P, _I, _I, _P],
    "pit_mlp_bwd_params_deferrable": [_I, _I, _I, _I, _I, _L],
    "pit_rel_lp_loss_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P],
    "pit_rel_lp_loss_fwd_grad": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P],
    "pit_rel_lp_loss_fwd_grad_ordered": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P],
    "pit_rel_lp_loss_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "pit_plan_ragged_fwd": [_P, _P, _I, _I, _I, _I, _P, _P, _F, _I, _P, _P, _I, _P, _P, _P],
    "pit_posatt_ragged_fwd": _RAGGED + _FWD_RAGGED,
    "pit_posatt_ragged_bwd": _RAGGED + _BWD_RAGGED,
    "pit_plan_ragged_strided_fwd": [_P, _P, _I, _I, _I, _I, _L, _L, _P, _P, _F, _I, _P, _P, _I, _P, _P, _P],
    "pit_posatt_ragged_strided_fwd": _RAGGED_STRIDED + _FWD_RAGGED,
    "pit_posatt_ragged_strided_bwd": _RAGGED_STRIDED + _BWD_RAGGED,
    "pit_rel_lp_loss_ragged_fwd": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "pit_rel_lp_loss_ragged_bwd": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P],
    "pit_rel_lp_loss_ragged_fwd_grad": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _L, _P],
    "pit_rel_max_norm_ragged": [_P, _P, _P, _I, _I, _I, _P, _P],
    "pit_distmat_select_fwd": [_P, _L, _L, _I, _I, _I, _I, _I, _P, _P],
    "pit_distmat_fwd": _MAT + _FWD_DIST,
    "pit_distmat_bwd_workspace": [_I, _I, _I],
    "pit_distmat_bwd": _MAT + _BWD_DIST + [_P] + _SAVED_OUT + [_P] + _TAIL,                 # ..., d_m, out ..., a_workspace
    "pit_distlist_select_fwd": [_P, _P, _L, _L, _I, _I, _I, _I, _I, _I, _P, _P],
    "pit_distlist_fwd": _LIST + _FWD_DIST,
    "pit_distlist_bwd_workspace": [_I, _I, _I, _I],
    "pit_distlist_bwd": _LIST + _BWD_DIST + [_P] + _SAVED_OUT + [_P] * 5 + _TAIL,            # ..., d_sqd, out ..., the transposed index, dv_workspace
    "pit_rel_max_norm": [_P, _P, _I, _I, _I, _P, _P, _P],
    "pit_eval_metrics_workspace": [_I, _I, _I],
    "pit_eval_metrics": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _L, _P, _L, _L, _I, _P, _P],
    "pit_batch_feed": [_P, _P, _P, _I, _L, _I, _I, _I, _I, _I, _P, _LL, _P, _P, _P, _P],
    "pit_batch_feed_points": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P, _LL, _P, _P, _P,
                              _P],
    "pit_fps": [_P, _I, _I, _I, _L, _P, _P, _I, _I, _P, _P, _P, _P],
    "pit_fps_large_workspace": [_I, _I, _I],
    "pit_fps_large": [_P, _I, _I, _I, _L, _P, _P, _I, _I, _P, _P, _P, _I, _P, _P],
    "pit_knn_box": [_P, _P, _I, _I, _I, _I, _L, _L, _P, _I, _P, _P, _P, _P],
    "pit_knn_rows": [_P, _L, _L, _I, _I, _I, _I, _P, _P, _P, _P],
    "pit_knn_last_form": [],
    "pit_instance_norm_fwd": [_P, _L, _L, _I, _I, _I, _F, _P, _P, _P],
    "pit_instance_norm_bwd": [_P, _P, _P, _I, _I, _I, _P, _P],
    "pit_adam_step": [_P, _P, _P, _P, _L, _P, _F, _F, _I, _F, _F, _F, _F, _I, _P, _P],
    "pit_adam_guard_parts": [_L],
    "pit_adam_step_guarded": [_P, _P, _P, _P, _L, _P, _P, _F, _F, _I, _I, _D, _F, _F, _F, _F, _I, _D, _I, _P, _P, _P, _P, _P],
    "pit_adam_step_averaged": [_P, _P, _P, _P, _L, _P, _P, _F, _F, _I, _I, _D, _F, _F, _F, _F, _I, _D, _I, _P, _P, _P, _P,
                               _P, _P, _I, _D, _I, _LL, _P],
    "pit_exchange_words": [_P, _P, _L, _P],
    "pit_debug_mfma_tile": [_P, _P, _P, _P],
    "pit_debug_rider_counts": [_P, _I, _I],
    "pit_debug_gemm_counts": [_P, _I, _I],
    "pit_debug_att_counts": [_P, _I, _I],
    "pit_block_fwd_set_form": [_I],
    "pit_block_fwd_last_rows": [],
    "pit_block_bwd_last_riders": [_P, _I],
}

LONG_RETURN = {"pit_satt_tiles_elems", "pit_posatt_dmesh_workspace", "pit_mlp_bwd_params_ordered_workspace",
               "pit_mlp_bwd_params_ordered_mfma_workspace", "pit_distmat_bwd_workspace", "pit_distlist_bwd_workspace",
               "pit_eval_metrics_workspace", "pit_fps_large_workspace"}
# entries added to an ABI version after its first release (PIT_HAS_* in the header): a library of the same version built before
# them lacks the symbols
ADDED_LATER = {"pit_distlist_select_fwd", "pit_distlist_fwd", "pit_distlist_bwd_workspace", "pit_distlist_bwd",
               "pit_rel_lp_loss_ragged_fwd_grad", "pit_rel_max_norm_ragged",       # PIT_HAS_DISTLIST, PIT_HAS_RAGGED_STEP
               "pit_block_fwd_set_form", "pit_block_fwd_last_rows",                # PIT_HAS_BLOCK_ROWS8
               "pit_block_bwd_last_riders",                                        # PIT_HAS_RIDER_TAIL
               "pit_debug_att_counts",                                             # PIT_HAS_ATT_COUNTS
               "pit_eval_metrics_workspace", "pit_eval_metrics",                   # PIT_HAS_EVAL_METRICS
               "pit_batch_feed",                                                   # PIT_HAS_BATCH_FEED
               "pit_adam_guard_parts", "pit_adam_step_guarded",                    # PIT_HAS_GUARDED_ADAM
               "pit_adam_step_averaged", "pit_exchange_words",                     # PIT_HAS_AVERAGED_ADAM
               "pit_fps",                                                          # PIT_HAS_FPS
               "pit_batch_feed_points",                                            # PIT_HAS_FEED_POINTS
               "pit_fps_large_workspace", "pit_fps_large",                         # PIT_HAS_FPS_LARGE
               "pit_knn_box", "pit_knn_rows", "pit_knn_last_form"}                 # PIT_HAS_KNN
FPS_MAX_POINTS = 16384   # PIT_FPS_MAX_POINTS
FPS_MAX_POINTS_WIDE = 4096       # PIT_FPS_MAX_POINTS_WIDE (space_dim 4..8)
FPS_LARGE_MAX_POINTS = 4194304   # PIT_FPS_LARGE_MAX_POINTS (every space_dim)
FPS_LARGE_MAX_SAMPLES = 16384    # PIT_FPS_LARGE_MAX_SAMPLES
KNN_MAX_K = 2048         # PIT_KNN_MAX_K
KNN_REG_MAX_KEYS = 1024  # PIT_KNN_REG_MAX_KEYS
GUARD_MAX_PARTS = 256    # PIT_GUARD_MAX_PARTS
GUARD_STATE_DOUBLES = 10         # PIT_GUARD_STATE_DOUBLES
FEED_MAX_FIELDS = 8      # PIT_FEED_MAX_FIELDS
FEED_MAX_ROW_BYTES = 1 << 30     # PIT_FEED_MAX_ROW_BYTES
FEED_WHOLE_ROW, FEED_POINTS_G0, FEED_POINTS_G1 = 0, 1, 2         # PIT_FEED_WHOLE_ROW, PIT_FEED_POINTS_G0, PIT_FEED_POINTS_G1
EVAL_STATE_DOUBLES = 8   # PIT_EVAL_STATE_DOUBLES
EVAL_MAX_PARTS = 64      # PIT_EVAL_MAX_PARTS
DISTLIST_CHUNK = 512   # PIT_DISTLIST_CHUNK


def distlist_chunk_slots(n_out: int, cap: int) -> int:
    """PIT_DISTLIST_CHUNK_SLOTS of include/pit_hip.h."""
    return int(n_out) * int(cap) // (DISTLIST_CHUNK // 2) + 1
ABI_VERSION = 31       # PIT_ABI_VERSION of include/pit_hip.h this binding was written against

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m position_induced_transformer_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for the PiT hot path.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            try:
                fn = getattr(handle, name)   # AttributeError if the ABI lost a symbol
            except AttributeError:
                if name not in ADDED_LATER:
                    raise
                raise RuntimeError(f"{LIB_PATH} was built before {name} joined PIT_ABI_VERSION {ABI_VERSION}: "
                                   "rebuild it (python -m position_induced_transformer_amd.build)") from None
            fn.argtypes = argtypes
            fn.restype = ctypes.c_char_p if name == "pit_error_string" else (_L if name in LONG_RETURN else _I)
        got = handle.pit_version()           # the default library and a PIT_LIB_PATH override alike
        if got != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} implements PIT_ABI_VERSION {got}, this package binds version {ABI_VERSION}: "
                               "rebuild it (python -m position_induced_transformer_amd.build)")
        _lib = handle
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().pit_error_string(code)
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else '?'}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


# ---- the values of the argument groups above (t: a (batch, points, channels) tensor whose rows are contiguous) --------------------
def values_args(t, with_batch: bool) -> tuple:
    b, _, d = t.shape
    return (t.data_ptr(),) + ((b, d) if with_batch else (d,)) + (t.stride(1), t.stride(0))


def head_args(head, n_head: int, is_scale: bool, *scale) -> tuple:
    """_HEAD; with the forward's scale_out as ``scale``: _HEAD_BWD."""
    return (head.data_ptr(), n_head, 1 if is_scale else 0) + tuple(c.data_ptr() for c in scale)


def out_args(out, d: int, concat: bool, rowstat, scale_out) -> tuple:
    return (out.data_ptr(), out.stride(1), out.stride(0), d if concat else 0, 1 if concat else 0, rowstat.data_ptr(), scale_out.data_ptr())


def dout_args(d_out, d: int, concat: bool) -> tuple:
    return (d_out.data_ptr(), d_out.stride(1), d_out.stride(0), d if concat else 0)


def dvalues_args(d_values, j: int, d: int, concat: bool) -> tuple:
    return (ptr(d_values), d, j * d, 1 if concat else 0)


def dhead_args(d_head, workspace) -> tuple:
    return (ptr(d_head), 0, ptr(workspace))


def saved_out_args(out) -> tuple:
    return (None, 0, 0) if out is None else (out.data_ptr(), out.stride(1), out.stride(0))
