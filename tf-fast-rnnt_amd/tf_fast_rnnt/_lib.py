"""ctypes binding of libftr_hip.so (the C ABI declared in include/ftr.h).

This is the Python side of the drop-in boundary: the reference loads its op library with
``tf.load_op_library`` (tf_fast_rnnt/python/tf_fast_rnnt/__init__.py:38-40); here the same native
entry points are plain C symbols taking device pointers, so any framework that can hand out a
device pointer and a stream (torch here; TensorFlow-ROCm through the shim in INTEGRATION.md) can
call them.  There is deliberately no CPU fallback: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FTR_LIB_PATH") or os.path.join(_HERE, "libftr_hip.so")   # override: diagnostic builds only
_lib = None

_c_fp = ctypes.c_void_p   # const float* (device)
_c_ip = ctypes.c_void_p   # const int32_t* (device)
_c_st = ctypes.c_void_p   # hipStream_t
_c_hi = ctypes.POINTER(ctypes.c_int32)   # const int32_t* (HOST array, read at launch time)
_i = ctypes.c_int
_f = ctypes.c_float

_SIGNATURES = {
    "ftr_abi_version": (ctypes.c_int, []),
    "ftr_package_version": (ctypes.c_char_p, []),
    "ftr_last_error": (ctypes.c_char_p, []),
    "ftr_mutual_information_workspace_floats": (ctypes.c_size_t, [_i, _i, _i]),
    "ftr_mutual_information_handoff_floats": (ctypes.c_size_t, [_i, _i, _i]),
    "ftr_mutual_information_fwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_bwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_fwd_ws_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, ctypes.c_size_t, _i, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_bwd_ws_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, ctypes.c_size_t, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_bwd_loss_ws_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, ctypes.c_size_t, _i, _c_fp, _c_fp, _c_fp, _i, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_workspace_init": (_i, [_c_fp, ctypes.c_size_t, _i, _i, _i, _c_st]),
    "ftr_mutual_information_status": (_i, [_c_fp, ctypes.c_size_t, _i, _i, _i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong), _c_st]),
    "ftr_mutual_information_viterbi_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "ftr_mutual_information_viterbi_f32": (_i, [_c_fp, _c_fp, _c_ip, ctypes.c_void_p, ctypes.c_size_t, _c_fp, _c_ip, _i, _i, _i, _i, _c_st]),
    "ftr_cummin_i32": (_i, [_c_ip, _c_ip, _i, _i, _c_st]),
    "ftr_prune_ranges_i32": (_i, [_c_fp, _c_fp, _c_ip, _c_ip, _c_ip, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int), _c_st]),
    "ftr_do_pruning_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_do_pruning_bwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_do_pruning_bwd_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "ftr_do_pruning_bwd_ws_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _i, _i, _i, _i, _i, ctypes.c_void_p, ctypes.c_size_t, _c_st]),
    "ftr_pruned_logprobs_fwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_logprobs_bwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_negated_reduce_f32": (_i, [_c_fp, _i, _i, _c_fp, _c_st]),
    "ftr_pruned_logprobs_bwd_scaled_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_bwd_w_scaled_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_bwd_am_scaled_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_fp, _c_ip, _c_ip, _i, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_rowmax_exp_f32": (_i, [_c_fp, _c_fp, _c_fp, ctypes.c_longlong, _i, _c_st]),
    "ftr_rowmax_exp_pair_f32": (_i, [_c_fp, _c_fp, _c_fp, ctypes.c_longlong, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _i, _c_st]),
    "ftr_rowmax_exp_sum_f32": (_i, [_c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _i, _c_st]),
    "ftr_smoothed_logprobs_fwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_ip, _i, _f, _f, _f, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_bwd_w_f32": (_i, [_c_fp, _c_fp, _c_fp, _c_ip, _f, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_bwd_am_f32": (_i, [_c_fp, _c_fp, _c_fp, _c_fp, _c_ip, _c_ip, _i, _f, _c_fp, _c_fp, _f, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_bwd_lm_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _i, _f, _c_fp, _c_fp, _c_fp, _c_fp, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_fwd_pen_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_ip, _i, ctypes.c_double, _f, _f, _f, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_bwd_w_scaled_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_ip, _f, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_bwd_am_scaled_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_fp, _c_ip, _c_ip, _i, _f, _c_fp, _c_fp, _f, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_rowmax_exp_dot_f32": (_i, [_c_fp, _c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_longlong, _i, _c_st]),
    "ftr_rowdot_f32": (_i, [_c_fp, _c_fp, _c_fp, ctypes.c_longlong, _i, _c_st]),
    "ftr_colsum_weighted_workspace_floats": (ctypes.c_size_t, [ctypes.c_longlong, _i]),
    "ftr_colsum_weighted_f32": (_i, [_c_fp, _c_fp, _c_fp, _c_fp, ctypes.c_size_t, ctypes.c_longlong, _i, _c_st]),
    "ftr_simple_logprobs_fused_supported": (_i, [_i]),
    "ftr_simple_logprobs_fused_bwd_supported": (_i, [_i, _i]),
    "ftr_normalizer_gemm_f32": (_i, [_i, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_normalizer_gemm_set_choice": (_i, [_i, _i, _i, _i, _i, _i]),
    "ftr_normalizer_gemm_choice": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]),
    "ftr_simple_logprobs_fused_fwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _c_fp, _c_ip, _i, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_fused_fwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_ip, _i, ctypes.c_double, _f, _f, _f, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_fused_bwd_am_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_fp, _c_fp, _c_ip, _c_ip, _i, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_fused_bwd_am_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_fp, _c_fp, _c_ip, _c_ip, _i, _f, _f, _c_fp, _c_fp, _f, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_band_supported": (_i, [_i, _i, _i]),
    "ftr_band_ranges_check_i32": (_i, [_c_ip, _c_ip, _c_ip, _i, _i, _i, _c_st]),
    "ftr_pruned_band_fwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_band_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_ip, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_band_workspace_floats": (ctypes.c_size_t, [_i, _i, _i, _i]),
    "ftr_mutual_information_band_ws_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_ip, _c_fp, ctypes.c_size_t, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_band_bwd_scaled_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_hat_pruned_logprobs_fwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_hat_pruned_logprobs_bwd_scaled_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_hat_pruned_band_fwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_hat_pruned_band_bwd_scaled_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_multiblank_workspace_floats": (ctypes.c_size_t, [_i, _i, _i]),
    "ftr_mutual_information_multiblank_fwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_hi, _i, _c_fp, ctypes.c_size_t, _c_fp, _i, _i, _i, _c_st]),
    "ftr_mutual_information_multiblank_bwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_hi, _i, _c_fp, ctypes.c_size_t, _c_fp, _c_fp, _c_fp, _i, _i, _i, _c_st]),
    "ftr_multiblank_pruned_logprobs_fwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _c_hi, _i, ctypes.c_double, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_multiblank_pruned_logprobs_bwd_scaled_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _c_hi, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_mutual_information_tdt_workspace_floats": (ctypes.c_size_t, [_i, _i, _i]),
    "ftr_mutual_information_tdt_fwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_hi, _i, _c_hi, _i, _c_fp, ctypes.c_size_t, _c_fp, _i, _i, _i, _c_st]),
    "ftr_mutual_information_tdt_bwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_hi, _i, _c_hi, _i, _c_fp, ctypes.c_size_t, _c_fp, _c_fp, _c_fp, _i, _i, _i, _c_st]),
    "ftr_mutual_information_viterbi_tdt_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "ftr_mutual_information_viterbi_tdt_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_hi, _i, _c_hi, _i, ctypes.c_void_p, ctypes.c_size_t, _c_fp, _c_ip, _c_ip, _c_ip, _i, _i, _i, _c_st]),
    "ftr_tdt_pruned_logprobs_fwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _i, ctypes.c_double, ctypes.c_double, _c_fp, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_tdt_pruned_logprobs_bwd_scaled_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _i, ctypes.c_double, ctypes.c_double, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_fwd_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _c_ip, _i, ctypes.c_double, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_bwd_w_f32": (_i, [_c_fp, _c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_bwd_am_f32": (_i, [_c_fp, _c_fp, _c_fp, _c_fp, _c_ip, _c_ip, _i, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_bwd_lm_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_fp, _c_fp, _i, _c_fp, _i, _i, _i, _c_st]),
    "ftr_selftest": (_i, [ctypes.c_void_p, _c_st]),
}
# include/ftr_lowp.h, 16-bit joiner logits: (logits, kind = FTR_DTYPE_*, ...the _f32 twin's arguments..., flags = FTR_PRUNED_HAT, stream)
_LOWP_SIGNATURES = {
    "ftr_pruned_logprobs_fwd_dt": (_i, [_c_fp, _i, _c_ip, _c_ip, _c_ip, _i, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_logprobs_bwd_scaled_dt": (_i, [_c_fp, _i, _c_ip, _c_ip, _c_ip, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_band_fwd_dt": (_i, [_c_fp, _i, _c_ip, _c_ip, _c_ip, _i, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_band_bwd_scaled_dt": (_i, [_c_fp, _i, _c_ip, _c_ip, _c_ip, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _i, _i, _c_st]),
}
# include/ftr_prune_sum.h, the prune gather fused with the joiner's first addition: (am, lm, kind = FTR_DTYPE_*, ranges, out, ...)
# and its backward (g_out, kind, ranges, d_am, d_lm, ..., workspace, workspace_bytes, stream)
_PRUNE_SUM_SIGNATURES = {
    "ftr_do_pruning_sum_dt": (_i, [_c_fp, _c_fp, _i, _c_ip, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_do_pruning_sum_bwd_ws_dt": (_i, [_c_fp, _i, _c_ip, _c_fp, _c_fp, _i, _i, _i, _i, _i, ctypes.c_void_p, ctypes.c_size_t, _c_st]),
}
# include/ftr_joiner_act.h, that sum with tanh / relu behind it: (am, lm, kind, act = FTR_ACT_*, ranges, out, ...) and its backward
# (g_out, out, kind, act, ranges, d_am, d_lm, ..., workspace, workspace_bytes, stream)
_JOINER_ACT_SIGNATURES = {
    "ftr_pruned_joiner_act_dt": (_i, [_c_fp, _c_fp, _i, _i, _c_ip, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_joiner_act_bwd_ws_dt": (_i, [_c_fp, _c_fp, _i, _i, _c_ip, _c_fp, _c_fp, _i, _i, _i, _i, _i, ctypes.c_void_p, ctypes.c_size_t, _c_st]),
}
# include/ftr_kd.h, knowledge distillation on the pruned band: (logits, kind, teacher_logits, teacher_kind, symbols, ranges,
# boundary, termination_symbol, temperature, mode = FTR_KD_*, ...)
_KD_SIGNATURES = {
    "ftr_pruned_kd_fwd_dt": (_i, [_c_fp, _i, _c_fp, _i, _c_ip, _c_ip, _c_ip, _i, _f, _i, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_kd_bwd_scaled_dt": (_i, [_c_fp, _i, _c_fp, _i, _c_ip, _c_ip, _c_ip, _i, _f, _i, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_kd_reduce_f32": (_i, [_c_fp, _i, _i, _c_fp, _c_st]),
}
# include/ftr_kd_fact.h, its factored forms (HAT, TDT, node weights): the two lists above with (factorization = FTR_KD_FACT_*,
# n_dur, dur_weight, node_weights) in front of the stream
_KD_FACT_SIGNATURES = {
    "ftr_pruned_kd_fact_fwd_dt": (_i, _KD_SIGNATURES["ftr_pruned_kd_fwd_dt"][1][:-1] + [_i, _i, _f, _c_fp, _c_st]),
    "ftr_pruned_kd_fact_bwd_scaled_dt": (_i, _KD_SIGNATURES["ftr_pruned_kd_bwd_scaled_dt"][1][:-1] + [_i, _i, _f, _c_fp, _c_st]),
}
# include/ftr_kd_loss.h, the transducer loss on the band and that distillation loss in one pass: the head of the kd entries, then
# (delay_penalty, modified, lse, px_band, py_band, node_loss, saved, utt_loss, ...) forward and (lse, gx_band, gy_band, the loss's
# scale triple, saved, the kd scale triple, glogits, ...) backward
_KD_LOSS_SIGNATURES = {
    "ftr_pruned_band_kd_fwd_dt": (_i, [_c_fp, _i, _c_fp, _i, _c_ip, _c_ip, _c_ip, _i, _f, _i, ctypes.c_double, _i, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_band_kd_bwd_scaled_dt": (_i, [_c_fp, _i, _c_fp, _i, _c_ip, _c_ip, _c_ip, _i, _f, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _c_st]),
}
# include/ftr_kd_loss_fact.h, that pass with HAT rows and node weights: the two lists above with (factorization, node_weights) in
# front of the stream; the node occupancies (gx_band, gy_band, ranges, boundary, occ, B, T, S, r, stream) and the weighted
# utterance sums (node_loss, node_weights, utt_loss, B, T, r, stream)
_KD_LOSS_FACT_SIGNATURES = {
    "ftr_pruned_band_kd_fact_fwd_dt": (_i, _KD_LOSS_SIGNATURES["ftr_pruned_band_kd_fwd_dt"][1][:-1] + [_i, _c_fp, _c_st]),
    "ftr_pruned_band_kd_fact_bwd_scaled_dt": (_i, _KD_LOSS_SIGNATURES["ftr_pruned_band_kd_bwd_scaled_dt"][1][:-1] + [_i, _c_fp, _c_st]),
    "ftr_band_node_occupancy_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_ip, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_kd_weighted_utt_sum_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _i, _i, _c_st]),
}
# include/ftr_kd_topk.h, that distillation loss from a stored top-K teacher on the teacher's own band: (logits, kind, teacher_values,
# teacher_kind, teacher_indices, ranges, teacher_ranges, boundary, teacher_rest, node_weights, temperature, ...) and (..., B, T, S, C,
# r, r_t, K, stream)
_KD_TOPK_SIGNATURES = {
    "ftr_pruned_kd_topk_fwd_dt": (_i, [_c_fp, _i, _c_fp, _i, _c_ip, _c_ip, _c_ip, _c_ip, _c_fp, _c_fp, _f, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _i, _i, _c_st]),
    "ftr_pruned_kd_topk_bwd_scaled_dt": (_i, [_c_fp, _i, _c_fp, _i, _c_ip, _c_ip, _c_ip, _c_ip, _c_fp, _c_fp, _f, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _i, _i, _c_st]),
}
# include/ftr_fused.h, the fused d am kernel with W as an operand: the arguments of ftr_*_logprobs_fused_bwd_am_f32 with W in place
# of prod (and no combined scale: W carries it)
_FUSED_SIGNATURES = {
    "ftr_simple_logprobs_fused_bwd_am_w_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_fp, _c_fp, _c_ip, _c_ip, _i, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_fused_bwd_am_w_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_fp, _c_fp, _c_ip, _c_ip, _i, _f, _c_fp, _c_fp, _f, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_fused_bwd_am_w_columns": (_i, [_i, _i, _i]),
}
# include/ftr_live.h, the builder's backward on the live part of the lattice: the _scaled W entries with `live` [B,S+1,2] (int32)
# behind rsy, and the W-operand d am entries with `live` behind W
_LIVE_SIGNATURES = {
    "ftr_simple_logprobs_bwd_w_live_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_ip, _c_fp, _c_fp, _c_fp, _c_ip, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_bwd_w_live_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_ip, _f, _c_fp, _c_fp, _c_fp, _c_ip, _i, _i, _i, _i, _c_st]),
    "ftr_simple_logprobs_fused_bwd_am_live_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_ip, _c_fp, _c_fp, _c_ip, _c_ip, _i, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_smoothed_logprobs_fused_bwd_am_live_f32": (_i, [_c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _c_ip, _c_fp, _c_fp, _c_ip, _c_ip, _i, _f, _c_fp, _c_fp, _f, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
}
# include/ftr_band_tdt.h, the TDT loss on the pruned band itself: the workspace and domain queries, the recursion on
# band-shaped operands, and the band-shaped twins of the two ftr_tdt_pruned_logprobs_* builders
_BAND_TDT_SIGNATURES = {
    "ftr_mutual_information_band_tdt_workspace_floats": (ctypes.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "ftr_mutual_information_band_tdt_supported": (_i, [_i, _i, _i, _i, _i]),
    "ftr_mutual_information_band_tdt_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_ip, _c_hi, _i, _c_hi, _i, _c_fp, ctypes.c_size_t, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_tdt_pruned_band_fwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _i, ctypes.c_double, ctypes.c_double, _c_fp, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_tdt_pruned_band_bwd_scaled_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _i, ctypes.c_double, ctypes.c_double, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _c_st]),
}
# include/ftr_tdt_mix.h, the TDT loss mixed with the ordinary loss on the token head (omega): the two builders that also write
# the ordinary operands, band shaped and lattice shaped, and the two gradient entries that take both sets of occupancies
_TDT_MIX_FWD = [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _i, ctypes.c_double, _i, ctypes.c_double, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]
_TDT_MIX_BWD = [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _i, ctypes.c_double, ctypes.c_double, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _f, _c_fp, _i, _i, _i, _i, _i, _c_st]
_TDT_MIX_SIGNATURES = {
    "ftr_tdt_mix_pruned_band_fwd_f32": (_i, _TDT_MIX_FWD),
    "ftr_tdt_mix_pruned_logprobs_fwd_f32": (_i, _TDT_MIX_FWD),
    "ftr_tdt_mix_pruned_band_bwd_scaled_f32": (_i, _TDT_MIX_BWD),
    "ftr_tdt_mix_pruned_logprobs_bwd_scaled_f32": (_i, _TDT_MIX_BWD),
}
# include/ftr_band_multiblank.h, the multi-blank loss on the pruned band itself: the workspace and domain queries, the
# recursion on band-shaped operands, and the band-shaped twins of the two ftr_multiblank_pruned_logprobs_* builders
_BAND_MULTIBLANK_SIGNATURES = {
    "ftr_mutual_information_band_multiblank_workspace_floats": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "ftr_mutual_information_band_multiblank_supported": (_i, [_i, _i, _i, _i]),
    "ftr_mutual_information_band_multiblank_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_ip, _c_hi, _i, _c_fp, ctypes.c_size_t, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _c_st]),
    "ftr_multiblank_pruned_band_fwd_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _c_hi, _i, ctypes.c_double, ctypes.c_double, _c_fp, _c_fp, _c_fp, _i, _i, _i, _i, _i, _c_st]),
    "ftr_multiblank_pruned_band_bwd_scaled_f32": (_i, [_c_fp, _c_ip, _c_ip, _c_ip, _i, _c_hi, _c_hi, _i, _c_fp, _c_fp, _c_fp, _c_fp, _i, _f, _c_fp, _i, _i, _i, _i, _i, _c_st]),
}
# include/ftr_band_viterbi.h, best-path alignment on the pruned band itself: the domain and workspace queries and the entry
_BAND_VITERBI_SIGNATURES = {
    "ftr_mutual_information_band_viterbi_supported": (_i, [_i, _i, _i, _i, _i]),
    "ftr_mutual_information_band_viterbi_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "ftr_mutual_information_band_viterbi_f32": (_i, [_c_fp, _c_fp, _c_ip, _c_ip, _c_hi, _i, _c_hi, _i, ctypes.c_void_p, ctypes.c_size_t, _c_fp, _c_ip, _c_ip, _c_ip, _i, _i, _i, _i, _c_st]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)            # the symbols of include/ftr.h
LOWP_SYMBOLS = tuple(_LOWP_SIGNATURES)           # those of include/ftr_lowp.h
PRUNE_SUM_SYMBOLS = tuple(_PRUNE_SUM_SIGNATURES) # those of include/ftr_prune_sum.h
JOINER_ACT_SYMBOLS = tuple(_JOINER_ACT_SIGNATURES)   # those of include/ftr_joiner_act.h
KD_SYMBOLS = tuple(_KD_SIGNATURES)               # those of include/ftr_kd.h
KD_FACT_SYMBOLS = tuple(_KD_FACT_SIGNATURES)     # those of include/ftr_kd_fact.h
KD_LOSS_SYMBOLS = tuple(_KD_LOSS_SIGNATURES)     # those of include/ftr_kd_loss.h
KD_LOSS_FACT_SYMBOLS = tuple(_KD_LOSS_FACT_SIGNATURES)   # those of include/ftr_kd_loss_fact.h
KD_TOPK_SYMBOLS = tuple(_KD_TOPK_SIGNATURES)     # those of include/ftr_kd_topk.h
FUSED_SYMBOLS = tuple(_FUSED_SIGNATURES)         # those of include/ftr_fused.h
LIVE_SYMBOLS = tuple(_LIVE_SIGNATURES)           # those of include/ftr_live.h
BAND_TDT_SYMBOLS = tuple(_BAND_TDT_SIGNATURES)   # those of include/ftr_band_tdt.h
TDT_MIX_SYMBOLS = tuple(_TDT_MIX_SIGNATURES)     # those of include/ftr_tdt_mix.h
BAND_MULTIBLANK_SYMBOLS = tuple(_BAND_MULTIBLANK_SIGNATURES)   # those of include/ftr_band_multiblank.h
BAND_VITERBI_SYMBOLS = tuple(_BAND_VITERBI_SIGNATURES)   # those of include/ftr_band_viterbi.h
band_tdt_recursions = 0   # how many times the band-native TDT recursion has been launched from Python (tests read it)
band_multiblank_recursions = 0   # ... and the band-native multi-blank recursion, likewise
FTR_KD_FULL, FTR_KD_COLLAPSED = 0, 1             # include/ftr_kd.h: the `mode` of the kd entry points
FTR_KD_FACT_SOFTMAX, FTR_KD_FACT_HAT, FTR_KD_FACT_TDT = 0, 1, 2   # include/ftr_kd_fact.h: the `factorization` of its entry points
FTR_KD_FACT_MAX_DUR = 5
FTR_KD_TOPK_MAX_K = 64                           # include/ftr_kd_topk.h: the most stored columns per teacher row
FTR_MI_WS_CLEAN = 1   # include/ftr.h
FTR_DTYPE_F32, FTR_DTYPE_BF16, FTR_DTYPE_FP16 = 0, 1, 2   # include/ftr_lowp.h: the `kind` of the _dt entry points
FTR_ACT_TANH, FTR_ACT_RELU = 1, 2                          # include/ftr_joiner_act.h: the `act` of its entry points
FTR_PRUNED_HAT = 1    # include/ftr_lowp.h: their `flags` bit
FTR_TDT_MIX_TDT, FTR_TDT_MIX_RNNT = 1, 2                   # include/ftr_tdt_mix.h: the `parts` bits of its builders


def lib() -> ctypes.CDLL:
    """Loads libftr_hip.so once; raises ImportError (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C tf-fast-rnnt_amd/csrc).  tf_fast_rnnt has no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in {**_SIGNATURES, **_LOWP_SIGNATURES, **_PRUNE_SUM_SIGNATURES, **_JOINER_ACT_SIGNATURES, **_KD_SIGNATURES, **_KD_FACT_SIGNATURES, **_KD_LOSS_SIGNATURES, **_KD_LOSS_FACT_SIGNATURES, **_KD_TOPK_SIGNATURES, **_FUSED_SIGNATURES, **_LIVE_SIGNATURES,
                                            **_BAND_TDT_SIGNATURES, **_TDT_MIX_SIGNATURES, **_BAND_MULTIBLANK_SIGNATURES, **_BAND_VITERBI_SIGNATURES}.items():
            fn = getattr(handle, name)   # AttributeError here = header/library mismatch
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


class FtrError(RuntimeError):
    """A native entry point returned an FTR_ERR_* code (the reference raises tf.errors.Internal,
    tf_fast_rnnt_op.cc:114-116)."""


def check(rc: int, what: str) -> None:
    if rc != 1:
        msg = lib().ftr_last_error().decode("utf-8", "replace")
        raise FtrError(f"{what} failed with code {rc}: {msg}")


# Optional per-call hook used by bench.py: when set, every native call is bracketed by two HIP events
# recorded on the stream the kernels are launched on, keyed by the C symbol name.
_profile_hook = None


def set_profile_hook(hook) -> None:
    """hook(name) must return a context manager (or None to disable)."""
    global _profile_hook
    _profile_hook = hook


def call(name: str, *args) -> None:
    """Invoke a status-returning entry point of the C ABI and raise FtrError unless it returns 1."""
    fn = getattr(lib(), name)
    if _profile_hook is None:
        rc = fn(*args)
    else:
        with _profile_hook(name):
            rc = fn(*args)
    check(rc, name)
