/* include/ftr_band_multiblank.h -- the multi-blank transducer loss on the pruned band itself (MI355X addition): entry
 * points of the product library libftr_hip.so on top of ftr.h, whose conventions (return codes, ftr_last_error(), the
 * opaque stream, asynchrony, host duration arrays read at launch time) they share.  A header of its own, so that ftr.h,
 * ftr_lowp.h, ftr_kd.h, ftr_fused.h and ftr_band_tdt.h stay as they are, symbol for symbol; ftr_abi_version() is unchanged
 * by it. */
#ifndef FTR_BAND_MULTIBLANK_H_
#define FTR_BAND_MULTIBLANK_H_
#include "ftr.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Band-shaped operands.  ranges [B,T,r] must be a band (ranges[b,t,k] = ranges[b,t,0] + k, ranges[b,t,0] non-decreasing
 * over the frames of the boundary rectangle; ftr_band_ranges_check_i32) with r <= 15.  px_band [B,T,r] and py_band
 * [B,D,T,r], float32: element (b,t,k) / (b,j,t,k) belongs to lattice cell (s,t), s = ranges[b,t,0] + k, and is what
 * ftr_multiblank_pruned_logprobs_fwd_f32 puts at px[b,s,t] / py[b,j,s,t] (its -inf rules included: px at s = S, at column
 * t_end and for a symbol that is a big-blank id, py where t + d_j > t_end).  No array of size S * T exists on this route.
 *
 * ftr_mutual_information_band_multiblank_f32: the recursion of ftr_mutual_information_multiblank_fwd_f32 / _bwd_f32 on
 *   those operands,
 *     p[s,t] = logadd(p[s-1,t] + px[s-1,t], logadd_j p[s,t-d_j] + py_j[s,t-d_j]),  p[s_begin,t_begin] = 0
 *   durations d_0 < ... < d_{D-1} in 1..32 (1 <= D <= 8; they need not contain 1), a host array.  A move exists iff its
 *   source is a band cell of a frame t_begin <= t < t_end inside the boundary rectangle and its destination is such a
 *   cell or the end cell (s_end, t_end); the frames a blank skips need not be in the band.  Writes ans [B] =
 *   p[s_end,t_end] (computed in float64, rounded once; -inf when no path exists) and, unless gx_band and gy_band are both
 *   NULL, the occupancies gx_band [B,T,r] / gy_band [B,D,T,r] = exp(p(source) + operand + q(destination) - ans), every
 *   element written (0 where the move does not exist, all 0 without a path): they equal px_grad / py_grad of
 *   ftr_mutual_information_multiblank_bwd_f32 (ans_grad = ones) at the band cells.  A band start that decreases inside the
 *   rectangle gives ans = NaN and zero occupancies, as ftr_mutual_information_band_f32 answers it.  The workspace holds
 *   ftr_mutual_information_band_multiblank_workspace_floats(B,T,S,r,D) floats, 8-byte aligned, of the order
 *   B (S+T) lanes (D+1); its contents before the call do not matter.  Launches only: no memset or memcpy, no host
 *   synchronisation -- capturable in a hipGraph; the same bits on every run.
 * ftr_mutual_information_band_multiblank_supported(T,S,r,D): 1 where the recursion entry accepts these sizes (r <= 15,
 *   T >= 1, S >= 0, 1 <= D <= 8, slot indices within 32 bits), else 0 (then the workspace query returns 0).
 * ftr_multiblank_pruned_band_fwd_f32: the builder ftr_multiblank_pruned_logprobs_fwd_f32 with band-shaped outputs: lse
 *   [B,T,r] and px_band / py_band, bit-identical to its lattices at the band cells; big_blank_ids (D - 1 values) and
 *   durations (D values, durations[0] = 1) as there.
 * ftr_multiblank_pruned_band_bwd_scaled_f32: ftr_multiblank_pruned_logprobs_bwd_scaled_f32 fed from band-shaped
 *   occupancies, the same arithmetic and the same `scale` semantics; every element of glogits [B,T,r,C] is written.
 * Validation, in this order: for the recursion D (FTR_ERR_UNSUPPORTED outside 1..8); the duration list (and for the
 *   builders the big-blank ids, termination_symbol and sigma, as their lattice twins); sizes (FTR_ERR_INVALID_ARG); for the
 *   recursion r (FTR_ERR_UNSUPPORTED); scale_stride; B == 0 returns FTR_OK; the workspace size; the pointers (boundary may
 *   be NULL; symbols may be NULL when S == 0); the workspace alignment; the device.
 */
size_t ftr_mutual_information_band_multiblank_workspace_floats(int B, int T, int S, int r, int D);
int ftr_mutual_information_band_multiblank_supported(int T, int S, int r, int D);
int ftr_mutual_information_band_multiblank_f32(const float* px_band, const float* py_band, const int32_t* ranges,
                                               const int32_t* boundary, const int32_t* durations, int D, float* workspace,
                                               size_t workspace_floats, float* ans, float* gx_band, float* gy_band, int B,
                                               int T, int S, int r, void* stream);
int ftr_multiblank_pruned_band_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                       const int32_t* boundary, int termination_symbol, const int32_t* big_blank_ids,
                                       const int32_t* durations, int D, double sigma, double delay_penalty, float* lse,
                                       float* px_band, float* py_band, int B, int T, int S, int C, int r, void* stream);
int ftr_multiblank_pruned_band_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                              const int32_t* boundary, int termination_symbol, const int32_t* big_blank_ids,
                                              const int32_t* durations, int D, const float* lse, const float* gx_band,
                                              const float* gy_band, const float* scale, int scale_stride, float scale_mul,
                                              float* glogits, int B, int T, int S, int C, int r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_BAND_MULTIBLANK_H_ */
