/* include/ftr_kd_loss_fact.h -- the transducer loss on the pruned band and the factored distillation loss of ftr_kd_fact.h in
 * one pass over the student's joiner logits: HAT rows, node weights, and the student's own node occupancies as weights
 * (MI355X addition).  Entry points of the product library libftr_hip.so on top of ftr_kd_fact.h, whose conventions (element
 * type codes, modes, factorizations, validity of a node, return codes, ftr_last_error(), the opaque stream, asynchrony) they
 * share.  A header of its own, so that every other header stays as it is, symbol for symbol; ftr_abi_version() is unchanged
 * by it. */
#ifndef FTR_KD_LOSS_FACT_H_
#define FTR_KD_LOSS_FACT_H_
#include "ftr_kd_fact.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * The first two entries take the argument lists of the two entries of ftr_kd_loss.h plus, in front of `stream`,
 *   factorization   FTR_KD_FACT_SOFTMAX: the ordinary row, the transducer loss is that of the ordinary band builder;
 *                   FTR_KD_FACT_HAT (C >= 2): the HAT row, the transducer loss is that of the band builder with
 *                   FTR_PRUNED_HAT.  FTR_KD_FACT_TDT is refused with FTR_ERR_INVALID_ARG: its transducer gradient needs the
 *                   occupancies of every duration, and its builders are float32 only.
 *   node_weights    NULL, or float32 [B,T,r], the weights of ftr_kd_fact.h: they multiply the node's distillation loss (as
 *                   its last factor) and the distillation part of its gradient row.  A weight of exactly 0 takes the node
 *                   out of the DISTILLATION: its teacher row and saved planes are never read, its node loss is 0.  The
 *                   transducer loss does not know the weights: such a node's student row is still read for `lse`, and its
 *                   gradient row is the transducer part alone.
 * With FTR_KD_FACT_SOFTMAX and node_weights == NULL the very kernels of ftr_kd_loss.h run, bit for bit.
 *
 * Forward.  node_loss, saved: what the forward entry of ftr_kd_fact.h writes for the same factorization, mode and weights
 * (n_dur = 0), bit for bit.  lse [B,T,r]: the normaliser of the transducer loss at temperature 1 -- the logsumexp over all C
 * columns, or for HAT over the columns c != termination_symbol -- by the arithmetic of the band builder's own pass, written
 * for the rows ftr_kd_loss.h names.  px_band, py_band: what the band builder writes given that lse (HAT: its HAT form).
 * utt_loss may be NULL: no utterance-sum launch is made then (the caller weights node_loss afterwards, see below).
 *
 * Backward.  glogits [B,T,r,C], every element, one launch:
 *   g[c] = a_b (transducer row) + k_b w (d node_loss / d x[c])
 * with the transducer row of ftr_kd_loss.h, or for HAT
 *   gx (1[c == symbols[b,s]] - exp(x[c] - lse)) for c != termination_symbol,
 *   gy sigmoid(-x[c]) - gx sigmoid(x[c]) at c == termination_symbol      (gx = 0 where the symbol is the termination symbol),
 * and the second term the row of the backward entry of ftr_kd_fact.h.  Computed in float32, rounded once.  A part whose
 * multiplier is 0 is absent and nothing of it is read; the row is then the single entry's row, bit for bit.
 *
 * Weights that are the student's own occupancies:
 *   ftr_band_node_occupancy_f32  occ[b,t,k] = gx + gy from the gx_band / gy_band the band recursion returned: the
 *     probability that an alignment passes through lattice node (ranges[b,t,k], t); gx only where s < S.  Exact zeros for
 *     a node outside the boundary rectangle or outside the lattice.
 *   ftr_pruned_kd_weighted_utt_sum_f32  utt_loss[b] = sum over the T * r nodes of node_weights * node_loss (0 where the
 *     weight is 0), in the summation tree of the forward entries' own utterance sums: the utt_loss a forward entry would
 *     have written had it been given these weights.
 * The forward runs without weights and utt_loss == NULL, the band recursion follows, then these two; the backward takes
 * occ as node_weights.
 *
 * Validation, in the order of ftr_kd_loss.h and ftr_kd_fact.h: an unknown kind / teacher_kind / mode, a temperature that is
 * not finite and > 0, an unknown factorization or FTR_KD_FACT_TDT: FTR_ERR_INVALID_ARG before anything else is looked at;
 * then the two multipliers, which must be finite (backward); sizes (HAT with C < 2 is refused with them);
 * termination_symbol; the two scale strides (backward); B == 0 returns FTR_OK; then the pointers of the parts that are
 * present (boundary, node_weights and, forward, utt_loss may be NULL; symbols may be NULL when S == 0) and the device.
 * The two small entries: sizes (B >= 0, T >= 1, S >= 0, r >= 1), B == 0 returns FTR_OK, the pointers (boundary may be
 * NULL), the device.  Launches only: no memset or memcpy, no host synchronisation, no workspace -- capturable in a hipGraph.
 */
int ftr_pruned_band_kd_fact_fwd_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                   const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                   int termination_symbol, float temperature, int mode, double delay_penalty, int modified,
                                   float* lse, float* px_band, float* py_band, float* node_loss, float* saved, float* utt_loss,
                                   int B, int T, int S, int C, int r, int factorization, const float* node_weights,
                                   void* stream);
int ftr_pruned_band_kd_fact_bwd_scaled_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                          const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                          int termination_symbol, float temperature, int mode, const float* lse,
                                          const float* gx_band, const float* gy_band, const float* loss_scale,
                                          int loss_scale_stride, float loss_scale_mul, const float* saved,
                                          const float* kd_scale, int kd_scale_stride, float kd_scale_mul, void* glogits, int B,
                                          int T, int S, int C, int r, int factorization, const float* node_weights,
                                          void* stream);
int ftr_band_node_occupancy_f32(const float* gx_band, const float* gy_band, const int32_t* ranges, const int32_t* boundary,
                                float* occ, int B, int T, int S, int r, void* stream);
int ftr_pruned_kd_weighted_utt_sum_f32(const float* node_loss, const float* node_weights, float* utt_loss, int B, int T,
                                       int r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_KD_LOSS_FACT_H_ */
