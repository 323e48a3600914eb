/* include/ftr_lowp.h -- 16-bit joiner logits (MI355X addition): entry points of the product library libftr_hip.so on top
 * of everything in ftr.h, whose conventions (return codes, ftr_last_error(), the opaque stream, asynchrony) they share.
 * They are kept out of ftr.h so that ftr.h stays the float32 drop-in surface, symbol for symbol; ftr_abi_version() is
 * unchanged by them. */
#ifndef FTR_LOWP_H_
#define FTR_LOWP_H_
#include "ftr.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * The four logits-reading operations of ftr.h, with the element type of `logits`
 * and `glogits` given by `kind` (an FTR_DTYPE_* code) and the HAT normalisation selected by bit FTR_PRUNED_HAT of `flags`
 * (any other bit set: FTR_ERR_INVALID_ARG); apart from these two arguments each takes the argument list of its _f32 form and
 * validates it the same way, after `kind`.  An unknown `kind` returns FTR_ERR_INVALID_ARG before anything else is looked at.
 *   ftr_pruned_logprobs_fwd_dt         = ftr_pruned_logprobs_fwd_f32        / ftr_hat_pruned_logprobs_fwd_f32
 *   ftr_pruned_logprobs_bwd_scaled_dt  = ftr_pruned_logprobs_bwd_scaled_f32 / ftr_hat_pruned_logprobs_bwd_scaled_f32
 *   ftr_pruned_band_fwd_dt             = ftr_pruned_band_fwd_f32            / ftr_hat_pruned_band_fwd_f32
 *   ftr_pruned_band_bwd_scaled_dt      = ftr_pruned_band_bwd_scaled_f32     / ftr_hat_pruned_band_bwd_scaled_f32
 * A 16-bit tensor stands for its exact float32 up-conversion: lse, px / py (or their band forms) and every intermediate
 * are float32, computed as the _f32 entry points compute them; glogits is computed in float32 and rounded once, to
 * nearest-even, when it is stored in the element type (NaN stays NaN, -inf stays -inf).  With FTR_DTYPE_F32 the calls are
 * the _f32 entry points.  Rows are contiguous (C elements); a 16-bit tensor may start at any element, but is read and
 * written four elements at a time only when C % 4 == 0 and its base address is 8-byte aligned (else element by element).
 */
#define FTR_DTYPE_F32 0  /* float */
#define FTR_DTYPE_BF16 1 /* bfloat16: the upper 16 bits of a float */
#define FTR_DTYPE_FP16 2 /* IEEE binary16 */
#define FTR_PRUNED_HAT 1 /* flags bit: the ftr_hat_* normalisation (needs C >= 2) */
int ftr_pruned_logprobs_fwd_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                               const int32_t* boundary, int termination_symbol, double delay_penalty, float* lse,
                               float* px, float* py, int B, int T, int S, int C, int r, int modified, int flags,
                               void* stream);
int ftr_pruned_logprobs_bwd_scaled_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                                      const int32_t* boundary, int termination_symbol, const float* lse,
                                      const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                      float scale_mul, void* glogits, int B, int T, int S, int C, int r, int modified,
                                      int flags, void* stream);
int ftr_pruned_band_fwd_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                           const int32_t* boundary, int termination_symbol, double delay_penalty, float* lse,
                           float* px_band, float* py_band, int B, int T, int S, int C, int r, int modified, int flags,
                           void* stream);
int ftr_pruned_band_bwd_scaled_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                                  const int32_t* boundary, int termination_symbol, const float* lse,
                                  const float* gx_band, const float* gy_band, const float* scale, int scale_stride,
                                  float scale_mul, void* glogits, int B, int T, int S, int C, int r, int modified,
                                  int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_LOWP_H_ */
