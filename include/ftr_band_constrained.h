/* include/ftr_band_constrained.h -- the constrained transducer type on the pruned band itself (MI355X addition): entry
 * points of the product library libftr_hip.so on top of ftr.h and ftr_lowp.h, whose conventions (return codes,
 * ftr_last_error(), the opaque stream, asynchrony, the FTR_DTYPE_* codes and the FTR_PRUNED_HAT flag bit) they share.  A
 * header of its own, so that ftr.h, ftr_lowp.h and the other headers stay as they are, symbol for symbol;
 * ftr_abi_version() is unchanged by it. */
#ifndef FTR_BAND_CONSTRAINED_H_
#define FTR_BAND_CONSTRAINED_H_
#include "ftr_lowp.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * The constrained type (rnnt_type = "constrained") is the modified type with a blank forced behind every symbol:
 * px_c[s,t] = px'[s,t] + py[s+1,t], where px' / py are the modified type's log-probs.  On a band (ranges[b,t,k] =
 * ranges[b,t,0] + k, ranges[b,t,0] non-decreasing over the frames of the boundary rectangle, r <= 15) row s+1 of frame t is
 * slot k+1 of the same frame, so the operands of the band recursion (ftr_mutual_information_band_ws_f32, modified = 1)
 * are formed frame by frame and no array of size S * T exists.
 *
 * ftr_pruned_band_constrained_fwd_dt: one launch, one workgroup per frame (b,t), one wave per band row k.  logits
 *   [B,T,r,C] of element type `kind` are read once.  Writes, for every (b,t,k), float32:
 *     lse[b,t,k]      logsumexp of the row (HAT: over the non-blank columns)
 *     py_band[b,t,k]  x[blank] - lse (HAT: log sigmoid(x[blank])), -inf where s = ranges[b,t,0] + k is outside 0..S
 *     px_band[b,t,k]  (x[sym_s] - lse) + py_band[b,t,k+1] (HAT: x[sym_s] - lse - softplus(x[blank]) in the first term),
 *                     -inf where s is outside 0..S-1, where k + 1 == r, and for HAT where sym_s is the blank; then, with
 *                     delay_penalty > 0, plus (float)(((t_end - 1) / 2 - t) * delay_penalty), the offset in float64
 *   which is, element for element, what the lattice composition of the constrained type puts at cell (s,t).  Frames outside
 *   [t_begin, t_end) are not read: there lse = 0 and px_band = py_band = -inf (the recursion never looks at them).
 * ftr_pruned_band_constrained_bwd_scaled_dt: one launch.  From the occupancies gx_band / gy_band [B,T,r] of the recursion
 *   on those operands, row (b,t,k) of glogits [B,T,r,C] is
 *     -(X + Y) softmax(x) + X 1[c == sym_s] + Y 1[c == blank],
 *     X = gx_band[b,t,k] (0 where px_band was forced to -inf),
 *     Y = gy_band[b,t,k] + gx_band[b,t,k-1] (the second term for k >= 1 and where that px_band element was not forced)
 *   (HAT: X (1[c == sym_s] - exp(x[c] - lse)) off the blank column, Y sigmoid(-x[blank]) - X sigmoid(x[blank]) on it), both
 *   multiplied by (scale ? scale[b * scale_stride] : 1) * scale_mul; computed in float32, rounded once into `kind`.  Every
 *   element of glogits is written (zeros in the frames outside [t_begin, t_end), which are not read).
 * Both: a 16-bit tensor stands for its exact float32 up-conversion; rows are read four elements at a time when
 *   C % 4 == 0 and a 16-bit base is 8-byte aligned, the forward keeps the row in registers while C <= 2048; any other C or
 *   base takes the element-by-element form with the same outputs.  Launches only: no memset, no memcpy, no host
 *   synchronisation -- capturable in a hipGraph; the same bits on every run.
 * Validation, in this order: `kind` and `flags` (FTR_ERR_INVALID_ARG); sizes, HAT's C >= 2, termination_symbol
 *   (FTR_ERR_INVALID_ARG); r > 15 (FTR_ERR_UNSUPPORTED); scale_stride; B == 0 returns FTR_OK; the pointers (boundary may be
 *   NULL, symbols may be NULL when S == 0, scale may be NULL); the device.
 */
int ftr_pruned_band_constrained_fwd_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                                       const int32_t* boundary, int termination_symbol, double delay_penalty, float* lse,
                                       float* px_band, float* py_band, int B, int T, int S, int C, int r, int flags,
                                       void* stream);
int ftr_pruned_band_constrained_bwd_scaled_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                                              const int32_t* boundary, int termination_symbol, const float* lse,
                                              const float* gx_band, const float* gy_band, const float* scale,
                                              int scale_stride, float scale_mul, void* glogits, int B, int T, int S, int C,
                                              int r, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_BAND_CONSTRAINED_H_ */
