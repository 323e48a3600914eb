/* include/ftr_path.h -- the log-probability of one given alignment under the pruned joiner, and its gradient (MI355X
 * addition): entry points of the product library libftr_hip.so on top of ftr_lowp.h, whose conventions (return codes,
 * ftr_last_error(), the opaque stream, asynchrony, the FTR_DTYPE_* codes and the FTR_PRUNED_HAT flag bit) they share.  A
 * header of its own, so that every other header stays as it is, symbol for symbol; ftr_abi_version() is unchanged by it. */
#ifndef FTR_PATH_H_
#define FTR_PATH_H_
#include "ftr_lowp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* `flags` of the two entries: FTR_PRUNED_HAT (ftr_lowp.h) and this bit, the modified transducer type */
#define FTR_PATH_MODIFIED 2

/*
 * logits [B,T,r,C] of element type `kind` (a 16-bit tensor stands for its exact float32 up-conversion; a 16-bit base may be
 * aligned to 2 bytes only), symbols [B,S], ranges [B,T,r] (ANY ranges: node (s,t) is the FIRST slot k with ranges[b,t,k] ==
 * s), boundary [B,4] = (s_begin, t_begin, s_end, t_end) or NULL (clamped into [0,S] x [0,T] as everywhere), frames [B,S]:
 * frames[b,s] is the frame that emits symbols[b,s]; entries outside [s_begin, s_end) are ignored.
 *
 * The path of utterance b has one SYMBOL ARC per row s in [s_begin, s_end), at node (s, frames[b,s]), and BLANK ARCS:
 *   regular type   one for every frame t in [t_begin, t_end), at row s(t) = s_begin + #{s : frames[b,s] <= t}; frames must be
 *                  non-decreasing
 *   modified type  (FTR_PATH_MODIFIED) one for every frame that emits no symbol, at s(t) = s_begin + #{s : frames[b,s] < t};
 *                  frames must be strictly increasing
 * An arc's log-probability comes from its node's row x, target column c = min(max(symbols[b,s],0),C-1) for a symbol arc and
 * termination_symbol for a blank arc: x[c] - logsumexp(x); with FTR_PRUNED_HAT log sigmoid(x[blank]) for a blank arc and
 * log sigmoid(-x[blank]) + x[c] - logsumexp over the non-blank columns for a symbol arc (a symbol that is the blank: -inf).
 *
 * ftr_pruned_path_logprob_fwd_dt: two launches.  One wave per arc writes arc_lp [B,S+T] and arc_lse [B,2,S+T] (float32; arc
 *   a < S is the symbol arc of row a, arc S + t the blank arc of frame t; arc_lse[b,0,a] is the maximum m of the row and
 *   arc_lse[b,1,a] = log sum exp(x - m), HAT: both over the non-blank columns -- the row's logsumexp in two parts, so that the
 *   gradient entry forms exp((x - m) - log sum) as accurately as the element is large; an arc that does not exist -- outside
 *   the rectangle, an emitting frame of the modified type, an inverted rectangle -- has 0 everywhere and reads nothing; a HAT
 *   blank arc has 0 in arc_lse and reads x[blank] alone).  One wave per utterance then writes logprob[b], the sum of
 *   arc_lp[b,:] in a fixed order.  logprob[b] is exactly -inf when the path is not a path: a frame outside [t_begin, t_end),
 *   frames not monotone as the type requires, or a node absent from ranges; such an arc has arc_lp = -inf and reads no
 *   logits, and every index is checked before it is used.
 * ftr_pruned_path_logprob_bwd_dt: one launch, one wave per row of glogits [B,T,r,C] (element type `kind`; every element is
 *   written).  The row of a node that carries an arc of the path gets logprob_grad[b] * (1[c == target] - exp(x[c] -
 *   logsumexp)) (HAT: sigmoid(-x[blank]) resp. -sigmoid(x[blank]) times logprob_grad[b] in the blank column, the softmax term
 *   over the non-blank columns for symbol arcs only), computed in float32 and rounded once.  Every other row, and every row
 *   of an utterance with logprob[b] == -inf or logprob_grad[b] == 0, is exactly zero and its logits are NOT read.
 * Both: rows are read four elements at a time when C % 4 == 0 and a 16-bit base is 8-byte aligned, the forward keeps the row
 *   in registers while C <= 2048; any other C or base takes the element-by-element form with the same outputs.  Launches
 *   only: no memset, no memcpy, no host synchronisation -- capturable in a hipGraph; the same bits on every run.
 * Validation, in this order: `kind` and `flags` (FTR_ERR_INVALID_ARG, before anything else is looked at); sizes (B >= 0,
 *   T >= 1, S >= 0, C >= 1, r >= 1), HAT's C >= 2, termination_symbol; B == 0 returns FTR_OK; the pointers (boundary may be
 *   NULL; symbols and frames may be NULL when S == 0); the device.  More than 2^31 - 1 rows or arcs are refused.
 */
int ftr_pruned_path_logprob_fwd_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                                   const int32_t* boundary, const int32_t* frames, int termination_symbol, float* arc_lp,
                                   float* arc_lse, float* logprob, int B, int T, int S, int C, int r, int flags, void* stream);
int ftr_pruned_path_logprob_bwd_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                                   const int32_t* boundary, const int32_t* frames, int termination_symbol,
                                   const float* arc_lse, const float* logprob, const float* logprob_grad, void* glogits, int B,
                                   int T, int S, int C, int r, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_PATH_H_ */
