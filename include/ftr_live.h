/* include/ftr_live.h -- the simple / smoothed builder's backward on the LIVE part of the lattice (MI355X addition): entry
 * points of the product library libftr_hip.so on top of ftr.h and ftr_fused.h, whose conventions (return codes,
 * ftr_last_error(), the opaque stream, asynchrony, the scale arguments) they share.  A header of its own, so that ftr.h and
 * ftr_fused.h stay as they are, symbol for symbol; ftr_abi_version() is unchanged by it.
 *
 * The occupancies g_px, g_py underflow to exact zeros away from the paths that carry probability, and W with them.  The W
 * kernel reports, per lattice row (b, s), the half-open frame interval [tlo, thi) outside which x = g_px' * scale,
 * y = g_py * scale and W are ALL exactly zero (of either sign; a NaN is never zero); the fused d am kernel walks, for its 64
 * frames, only the 16-row chunks between the first and the last row whose interval reaches them.  What it leaves out are
 * additions of exact zeros: d am and R compare equal, element for element, with the entries of ftr_fused.h. */
#ifndef FTR_LIVE_H_
#define FTR_LIVE_H_
#include "ftr_fused.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ftr_simple_logprobs_bwd_w_scaled_f32 / ftr_smoothed_logprobs_bwd_w_scaled_f32 (ftr.h) that also write
 * live [B,S+1,2] (int32): live[b,s] = (tlo, thi), and (T, 0) for a row without a live cell.  Rows and frames outside an
 * utterance's boundary are dead by themselves (their occupancies are zero).  FTR_BWD_LIVE=dense in the environment makes
 * every interval (0, T): the readers of the table then walk every block (A/B measurements, tests). */
int ftr_simple_logprobs_bwd_w_live_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                       float scale_mul, const float* prod, const int32_t* boundary, float* W, float* rsx,
                                       float* rsy, int32_t* live, int B, int T, int S, int modified, void* stream);
int ftr_smoothed_logprobs_bwd_w_live_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                         float scale_mul, const float* prod, const int32_t* boundary, float combined_scale,
                                         float* W, float* rsx, float* rsy, int32_t* live, int B, int T, int S, int modified,
                                         void* stream);

/* ftr_*_logprobs_fused_bwd_am_w_f32 (ftr_fused.h) with `live` behind W: the table written together with that W, for the SAME
 * gpx, gpy and scale arguments.  Same domain (T % 4 == 0, C % 4 == 0), same column tiling, same results. */
int ftr_simple_logprobs_fused_bwd_am_live_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                              float scale_mul, const float* W, const int32_t* live, const float* lm_probs,
                                              const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                                              int termination_symbol, float* d_am, int B, int T, int S, int C, int modified,
                                              void* stream);
int ftr_smoothed_logprobs_fused_bwd_am_live_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                                float scale_mul, const float* W, const int32_t* live, const float* lm_probs,
                                                const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                                                int termination_symbol, float direct_scale, const float* unigram,
                                                const float* am_dot, float am_only_scale, float* R, float* d_am, int B, int T,
                                                int S, int C, int modified, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* FTR_LIVE_H_ */
