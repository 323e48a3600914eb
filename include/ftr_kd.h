/* include/ftr_kd.h -- knowledge distillation on the pruned band (MI355X addition): entry points of the product library
 * libftr_hip.so on top of ftr_lowp.h, whose element type codes (FTR_DTYPE_*) and conventions (return codes,
 * ftr_last_error(), the opaque stream, asynchrony) they share.  A header of its own, so that ftr.h and ftr_lowp.h stay as
 * they are, symbol for symbol; ftr_abi_version() is unchanged by it. */
#ifndef FTR_KD_H_
#define FTR_KD_H_
#include "ftr_lowp.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Student `logits` and `teacher_logits` are both [B,T,r,C], rows contiguous, evaluated on the same `ranges` [B,T,r]; their
 * element types `kind` and `teacher_kind` (FTR_DTYPE_* codes) are independent, and a 16-bit tensor stands for its exact
 * float32 up-conversion.  Node (b,t,k) with s = ranges[b,t,k] is VALID iff t_begin <= t < t_end and s_begin <= s <= s_end,
 * boundary[b] = (s_begin, t_begin, s_end, t_end), NULL = (0, 0, S, T).  The logits rows of an invalid node are never read
 * (they may hold NaN or inf); it adds 0 to the loss and gets an all-zero gradient row.
 *   mode FTR_KD_FULL       node loss = KL(p || q) = sum_c p_c (log p_c - log q_c), p = softmax(teacher row / temperature),
 *                          q = softmax(student row / temperature) over the C columns
 *   mode FTR_KD_COLLAPSED  the same KL over three classes: blank (column termination_symbol), the correct next symbol
 *                          (column symbols[b,s], present only when s < s_end and that column is not the blank) and the
 *                          rest, whose mass is summed over the other columns (a masked logsumexp, never 1 - ...)
 * Terms of teacher mass 0 are 0.  There is no temperature^2 factor.  A NaN in a valid row makes the loss of its utterance
 * NaN; a student logit at -inf where the teacher has mass makes it +inf.
 *
 * ftr_pruned_kd_fwd_dt writes, all float32:
 *   node_loss [B,T,r]; saved: 2 (full) or 4 (collapsed) planes of [B,T,r] -- logsumexp(student row / temperature),
 *   logsumexp(teacher row / temperature), and in collapsed mode the same two over the rest columns -- which is all the
 *   backward needs; utt_loss [B], the sum of the utterance's node losses in a fixed order (bit-identical from run to run).
 * ftr_pruned_kd_bwd_scaled_dt writes glogits [B,T,r,C] (element type `kind`) = d loss / d logits, every row of utterance b
 *   multiplied by (scale ? scale[b * scale_stride] : 1) * scale_mul, computed in float32 and rounded once to nearest-even;
 *   every element is written (zeros for invalid nodes), so the buffer need not be initialised.  No teacher gradient exists.
 * ftr_pruned_kd_reduce_f32: reduction 0: out[b] = utt_loss[b]; 1: out[0] = mean; 2: out[0] = sum (the fixed summation
 *   tree of ftr_negated_reduce_f32, without the negation).
 * Validation: an unknown kind / teacher_kind / mode, or a temperature that is not finite and > 0, returns
 * FTR_ERR_INVALID_ARG before anything else is looked at; then sizes, termination_symbol, scale_stride; B == 0 returns
 * FTR_OK; then the pointers (boundary may be NULL; symbols may be NULL when S == 0) and the device.  Launches only: no
 * memset or memcpy, no host synchronisation, no workspace -- capturable in a hipGraph.
 */
#define FTR_KD_FULL 0
#define FTR_KD_COLLAPSED 1
int ftr_pruned_kd_fwd_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                         const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int termination_symbol,
                         float temperature, int mode, float* node_loss, float* saved, float* utt_loss, int B, int T, int S,
                         int C, int r, void* stream);
int ftr_pruned_kd_bwd_scaled_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                int termination_symbol, float temperature, int mode, const float* saved,
                                const float* scale, int scale_stride, float scale_mul, void* glogits, int B, int T, int S,
                                int C, int r, void* stream);
int ftr_pruned_kd_reduce_f32(const float* utt_loss, int B, int reduction, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_KD_H_ */
