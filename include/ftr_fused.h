/* include/ftr_fused.h -- the fused d am kernel with W as an operand (MI355X addition): entry points of the product library
 * libftr_hip.so on top of ftr.h, whose conventions (return codes, ftr_last_error(), the opaque stream, asynchrony, the scale
 * arguments of the _scaled forms) they share.  A header of its own, so that ftr.h stays as it is, symbol for symbol;
 * ftr_abi_version() is unchanged by it. */
#ifndef FTR_FUSED_H_
#define FTR_FUSED_H_
#include "ftr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ftr_*_logprobs_fused_bwd_am_f32 (ftr.h) with W as an operand: W [B,S+1,T] is what ftr_*_logprobs_bwd_w_scaled_f32 (or ftr_*_logprobs_bwd_w_f32)
 * wrote for the SAME gpx, gpy, scale arguments and combined scale -- the caller has it anyway, for the kind-1 matmul towards
 * lm -- and is staged as it is instead of being formed again from g_px, g_py and prod.  gpx / gpy and the scale arguments are
 * still read: by the scatter by symbol, the blank column and R.  The column tiling (128 or 256 columns per workgroup) is
 * chosen from (B, T, C) and the device's CU count so that the tile list fills the last round of workgroup slots;
 * ftr_simple_logprobs_fused_bwd_am_w_columns reports it, FTR_FUSED_BWD_CT=128|256 in the environment forces one.  Results
 * do not depend on the launch (fixed reduction order, no atomics). */
int ftr_simple_logprobs_fused_bwd_am_w_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                           float scale_mul, const float* W, const float* lm_probs, const float* am_probs,
                                           const int32_t* symbols, const int32_t* boundary, int termination_symbol,
                                           float* d_am, int B, int T, int S, int C, int modified, void* stream);
int ftr_smoothed_logprobs_fused_bwd_am_w_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                             float scale_mul, const float* W, const float* lm_probs,
                                             const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                                             int termination_symbol, float direct_scale, const float* unigram,
                                             const float* am_dot, float am_only_scale, float* R, float* d_am, int B, int T,
                                             int S, int C, int modified, void* stream);
int ftr_simple_logprobs_fused_bwd_am_w_columns(int B, int T, int C);

#ifdef __cplusplus
}
#endif
#endif  /* FTR_FUSED_H_ */
