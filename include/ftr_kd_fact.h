/* include/ftr_kd_fact.h -- factored knowledge distillation on the pruned band (MI355X addition): entry points of the product
 * library libftr_hip.so on top of ftr_kd.h, whose conventions (element type codes, modes, validity of a node, return codes,
 * ftr_last_error(), the opaque stream, asynchrony) they share.  A header of its own, so that ftr.h, ftr_lowp.h and ftr_kd.h
 * stay as they are, symbol for symbol; ftr_abi_version() is unchanged by it. */
#ifndef FTR_KD_FACT_H_
#define FTR_KD_FACT_H_
#include "ftr_kd.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * The two entries take the argument lists of ftr_pruned_kd_fwd_dt / ftr_pruned_kd_bwd_scaled_dt, where the last dimension
 * `C` of both tensors is the full row width, plus (in front of `stream`)
 *   factorization   how a joiner row is a distribution (below)
 *   n_dur           the number of duration columns at the end of the row: 1 .. 5 for FTR_KD_FACT_TDT, 0 otherwise
 *   dur_weight      FTR_KD_FACT_TDT: the multiplier of the duration head's KL, finite and >= 0 (ignored otherwise)
 *   node_weights    NULL, or float32 [B,T,r]: the node's loss and gradient row are multiplied by w[b,t,k].  A weight of
 *                   exactly 0 makes the node INVALID in the sense of ftr_kd.h (rows never read, loss 0, zero gradient row);
 *                   the weight is read before any logits load.  A NaN weight on a valid node makes its loss NaN.
 * With a = student row / temperature, b = teacher row / temperature, Bk = termination_symbol, sym = the symbol column of
 * ftr_kd.h (absent when s >= s_end or when it is the blank), tau = temperature:
 *   FTR_KD_FACT_SOFTMAX  the loss of ftr_kd.h.  With node_weights == NULL the very kernels of ftr_pruned_kd_* run: the
 *                        results are theirs bit for bit.
 *   FTR_KD_FACT_HAT      (C >= 2) qb = sigmoid(a_Bk), u = softmax(a) over c != Bk; pb, v likewise from b.
 *       FTR_KD_FULL       KL(Bern(pb) || Bern(qb)) + (1 - pb) sum_{c != Bk} v_c (log v_c - log u_c)
 *       FTR_KD_COLLAPSED  the KL over three classes of masses pb, (1 - pb) v_sym, (1 - pb) rho, rho = exp(R - L) with R
 *                         the logsumexp over the columns that are neither Bk nor sym and L the one over c != Bk
 *                         (= KL(Bern) + (1 - pb) KL over {sym, rest} of the non-blank softmax)
 *       d/dx_Bk = (qb - pb) / tau in both modes.  Log-sigmoids are -softplus(-+ .), never log(sigmoid(.)).
 *   FTR_KD_FACT_TDT      the first C - n_dur columns are the token head, the last n_dur the duration head; needs
 *                        termination_symbol < C - n_dur.  Node loss = KL_tok + dur_weight KL_dur, KL_tok the loss of
 *                        ftr_kd.h (either mode) over the token columns, KL_dur always the full KL of the two duration
 *                        softmaxes.  dur_weight == 0: the duration columns get exact zeros.
 * Saved planes, float32 [B,T,r] each, in this order (student before teacher in each pair); 0 everywhere for an invalid node:
 *   factorization  mode        planes
 *   SOFTMAX        FULL        2: logsumexp(a), logsumexp(b)
 *   SOFTMAX        COLLAPSED   4: + the same over the rest columns
 *   HAT            FULL        2: logsumexp over c != Bk of a, of b
 *   HAT            COLLAPSED   4: + the same over the rest columns
 *   TDT            FULL        4: logsumexp over the token columns of a, of b; the same over the duration columns
 *   TDT            COLLAPSED   6: the token pair, the rest pair, the duration pair
 * node_loss, utt_loss, glogits (all C columns of every row are written), scale and ftr_pruned_kd_reduce_f32: as in ftr_kd.h.
 * Validation: an unknown kind / teacher_kind / mode / factorization, a temperature that is not finite and > 0, a dur_weight
 * that is not finite and >= 0 (TDT), or an n_dur that does not fit the factorization (or is not below C) returns
 * FTR_ERR_INVALID_ARG before anything else is looked at; then the order of ftr_kd.h, where HAT with C < 2 is refused with
 * the sizes and TDT checks termination_symbol against C - n_dur.  node_weights may be NULL.  Launches only: no memset or
 * memcpy, no host synchronisation, no workspace -- capturable in a hipGraph.
 */
#define FTR_KD_FACT_SOFTMAX 0
#define FTR_KD_FACT_HAT 1
#define FTR_KD_FACT_TDT 2
#define FTR_KD_FACT_MAX_DUR 5
int ftr_pruned_kd_fact_fwd_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                              const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                              int termination_symbol, float temperature, int mode, float* node_loss, float* saved,
                              float* utt_loss, int B, int T, int S, int C, int r, int factorization, int n_dur,
                              float dur_weight, const float* node_weights, void* stream);
int ftr_pruned_kd_fact_bwd_scaled_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                     const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                     int termination_symbol, float temperature, int mode, const float* saved,
                                     const float* scale, int scale_stride, float scale_mul, void* glogits, int B, int T,
                                     int S, int C, int r, int factorization, int n_dur, float dur_weight,
                                     const float* node_weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_KD_FACT_H_ */
