/* include/ftr_kd_loss.h -- the transducer loss on the pruned band and the distillation loss of ftr_kd.h in one pass over
 * the student's joiner logits (MI355X addition): entry points of the product library libftr_hip.so on top of ftr_kd.h,
 * whose conventions (element type codes, modes, validity of a node, return codes, ftr_last_error(), the opaque stream,
 * asynchrony) they share.  A header of its own, so that ftr.h and the other headers stay as they are, symbol for symbol;
 * ftr_abi_version() is unchanged by it. */
#ifndef FTR_KD_LOSS_H_
#define FTR_KD_LOSS_H_
#include "ftr_kd.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * A distillation step evaluates ftr_pruned_band_fwd_dt / ftr_pruned_band_bwd_scaled_dt (ftr_lowp.h; the ordinary row, no
 * FTR_PRUNED_HAT) and ftr_pruned_kd_fwd_dt / ftr_pruned_kd_bwd_scaled_dt (ftr_kd.h) on the same student `logits` [B,T,r,C].
 * These two entries do the work of each pair in one pass over the rows.
 *
 * ftr_pruned_band_kd_fwd_dt writes, all float32,
 *   node_loss, saved, utt_loss: what ftr_pruned_kd_fwd_dt writes, bit for bit;
 *   lse [B,T,r]: logsumexp of the student row over its C columns (temperature 1), formed from the registers that hold the
 *     row for the distillation sums, by the arithmetic of ftr_pruned_band_fwd_dt's own logsumexp pass.  It is written for
 *     every node the band recursion looks at: frames t_begin <= t < t_end with 0 <= ranges[b,t,k] <= S -- the valid nodes,
 *     and the rows of those frames outside [s_begin, s_end], whose STUDENT row is read for this alone (the recursion's shift
 *     constants are means over all band entries of those frames).  Everywhere else lse = 0 and neither row is read;
 *   px_band, py_band [B,T,r]: what ftr_pruned_band_fwd_dt writes given that lse (`modified`, `delay_penalty` as there).
 *   With them ftr_mutual_information_band_ws_f32 returns the scores and occupancies of the composition, bit for bit.
 *   Three launches: the row kernel, the band gather, the utterance sums.  (A student that may be read four elements at a time
 *   next to a teacher that may not: four, the logsumexp then being ftr_pruned_band_fwd_dt's own pass over all rows.)
 *
 * ftr_pruned_band_kd_bwd_scaled_dt writes glogits [B,T,r,C] (element type `kind`), every element, in one launch:
 *   g[c] = a_b (-(gx + gy) exp(x[c] - lse) + 1[c == symbols[b,s]] gx + 1[c == termination_symbol] gy)
 *          + k_b (d node_loss / d x[c])
 *   a_b = (loss_scale ? loss_scale[b * loss_scale_stride] : 1) * loss_scale_mul, k_b likewise from the kd_ triple;
 *   gx = gx_band[b,t,k] where s < S, else 0; gy = gy_band[b,t,k]: the occupancies ftr_mutual_information_band_ws_f32
 *   returned, under the masks of ftr_pruned_band_bwd_scaled_dt.  The second term is the row of
 *   ftr_pruned_kd_bwd_scaled_dt.  The row is computed in float32 and rounded once.  An invalid node (ftr_kd.h) gets zeros
 *   and is not read: its occupancies are zero too.
 *   A part whose multiplier (loss_scale_mul, kd_scale_mul) is 0 is absent: nothing of it is read -- lse, gx_band and
 *   gy_band, or saved and teacher_logits -- and those pointers may be NULL; the row is then the other entry's row, bit
 *   for bit.
 *
 * Validation, in the order of ftr_kd.h: an unknown kind / teacher_kind / mode, or a temperature that is not finite and
 * > 0, returns FTR_ERR_INVALID_ARG before anything else is looked at; then the two multipliers, which must be finite
 * (backward); sizes; termination_symbol; the two scale strides (backward); B == 0 returns FTR_OK; then the pointers of
 * the parts that are present (boundary may be NULL; symbols may be NULL when S == 0) and the device.  Launches only: no
 * memset or memcpy, no host synchronisation, no workspace -- capturable in a hipGraph.
 */
int ftr_pruned_band_kd_fwd_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                              const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int termination_symbol,
                              float temperature, int mode, double delay_penalty, int modified, float* lse, float* px_band,
                              float* py_band, float* node_loss, float* saved, float* utt_loss, int B, int T, int S, int C,
                              int r, void* stream);
int ftr_pruned_band_kd_bwd_scaled_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                     const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                     int termination_symbol, float temperature, int mode, const float* lse,
                                     const float* gx_band, const float* gy_band, const float* loss_scale,
                                     int loss_scale_stride, float loss_scale_mul, const float* saved, const float* kd_scale,
                                     int kd_scale_stride, float kd_scale_mul, void* glogits, int B, int T, int S, int C,
                                     int r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_KD_LOSS_H_ */
