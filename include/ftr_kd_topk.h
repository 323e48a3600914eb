/* include/ftr_kd_topk.h -- knowledge distillation on the pruned band from a stored top-K teacher (MI355X addition): entry
 * points of the product library libftr_hip.so on top of ftr_lowp.h, whose element type codes (FTR_DTYPE_*) and conventions
 * (return codes, ftr_last_error(), the opaque stream, asynchrony) they share.  A header of its own, so that every other
 * header stays as it is, symbol for symbol; ftr_abi_version() is unchanged by it. */
#ifndef FTR_KD_TOPK_H_
#define FTR_KD_TOPK_H_
#include "ftr_lowp.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * The student `logits` are [B,T,r,C] (element type `kind`), rows contiguous, on `ranges` [B,T,r].  The teacher is a cache
 * made on the teacher's OWN band of r_t rows per frame:
 *   teacher_values  [B,T,r_t,K], element type `teacher_kind` (independent of `kind`; a 16-bit tensor stands for its exact
 *                   float32 up-conversion): the raw teacher logits at the stored columns
 *   teacher_indices [B,T,r_t,K] int32: those columns.  Each is clamped into [0,C) before use, so no value can send a kernel
 *                   out of bounds.  I = the set of a row's (clamped) indices.  A row is padded to K entries with value
 *                   -inf; an index may repeat a real entry's only with value -inf
 *   teacher_ranges  [B,T,r_t] int32, or NULL = `ranges` (then r_t must equal r).  Only teacher_ranges[b,t,0] is read: the
 *                   rows of a frame are taken to be consecutive
 *   teacher_rest    [B,T,r_t] float32, or NULL = -inf everywhere: logsumexp over c not in I of teacher_row[c] / temperature,
 *                   the unnormalised mass of the columns that were not stored, at the temperature of the call.  NULL is the
 *                   renormalised top-K form
 *   node_weights    [B,T,r] float32, or NULL: the node's loss and gradient row are multiplied by w[b,t,k]
 * Node (b,t,k) with s = ranges[b,t,k] is DISTILLED iff t_begin <= t < t_end and s_begin <= s <= s_end (boundary[b] =
 * (s_begin, t_begin, s_end, t_end), clamped into [0,S] x [0,T]; NULL = (0, 0, S, T)), its weight is not exactly 0 (a NaN
 * weight is not 0: the node's loss becomes NaN), and k' = s - teacher_ranges[b,t,0] satisfies 0 <= k' < r_t; its teacher
 * row is (b,t,k').  All of this is decided before any logits load.  Any other node adds 0, gets an all-zero gradient row,
 * and neither its student row nor any teacher row is read for it.  S enters through the boundary alone; a caller that
 * does not know it passes INT_MAX.
 * For a distilled node, a = student row / temperature, v = values / temperature, R = rest:
 *   L = logaddexp(logsumexp_k v_k, R); p_k = exp(v_k - L); p_R = exp(R - L)
 *   Ls = logsumexp_c a_c; Rs = logsumexp over c not in I of a_c (a masked logsumexp with its own maximum, never log(1 - ...))
 *   node loss = w (sum_k xlogy(p_k, p_k / q_k) + xlogy(p_R, p_R / q_R)), log q_k = a[idx_k] - Ls, log q_R = Rs - Ls
 *   d loss / d x_c = (w / temperature) (exp(a_c - Ls) - pt_c), pt_c = p_k for c = idx_k, p_R exp(a_c - Rs) for c not in I
 *   (0 when p_R = 0)
 * Terms of teacher mass 0 are 0.  There is no temperature^2 factor.  A stored column of teacher mass where the student has
 * -inf makes the loss +inf.
 *
 * ftr_pruned_kd_topk_fwd_dt writes, all float32: node_loss [B,T,r]; saved, 3 planes of [B,T,r]: Ls, Rs, L (0 for a node
 *   that is not distilled); utt_loss [B], the sum of the utterance's node losses in a fixed order (bit-identical from run to
 *   run).  The batch reduction is the reduce entry of ftr_kd.h.
 * ftr_pruned_kd_topk_bwd_scaled_dt writes glogits [B,T,r,C] (element type `kind`) = d loss / d logits, every row of
 *   utterance b multiplied by (scale ? scale[b * scale_stride] : 1) * scale_mul, computed in float32 and rounded once to
 *   nearest-even; every element is written (zeros for nodes that are not distilled).  No teacher gradient exists.
 * Validation, in this order: (1) an unknown kind / teacher_kind, or a temperature that is not finite and > 0, returns
 * FTR_ERR_INVALID_ARG before anything else is looked at; (2) sizes: B >= 0, T >= 1, S >= 0, C >= 1, r >= 1, r_t >= 1,
 * 1 <= K <= FTR_KD_TOPK_MAX_K, and r_t == r when teacher_ranges is NULL; (3) scale_stride (backward); B == 0 returns
 * FTR_OK; (4) the pointers (boundary, teacher_ranges, teacher_rest, node_weights and scale may be NULL); (5) the device.
 * Launches only: no memset or memcpy, no host synchronisation, no workspace -- capturable in a hipGraph.
 */
#define FTR_KD_TOPK_MAX_K 64
int ftr_pruned_kd_topk_fwd_dt(const void* logits, int kind, const void* teacher_values, int teacher_kind,
                              const int32_t* teacher_indices, const int32_t* ranges, const int32_t* teacher_ranges,
                              const int32_t* boundary, const float* teacher_rest, const float* node_weights,
                              float temperature, float* node_loss, float* saved, float* utt_loss, int B, int T, int S,
                              int C, int r, int r_t, int K, void* stream);
int ftr_pruned_kd_topk_bwd_scaled_dt(const void* logits, int kind, const void* teacher_values, int teacher_kind,
                                     const int32_t* teacher_indices, const int32_t* ranges, const int32_t* teacher_ranges,
                                     const int32_t* boundary, const float* teacher_rest, const float* node_weights,
                                     float temperature, const float* saved, const float* scale, int scale_stride,
                                     float scale_mul, void* glogits, int B, int T, int S, int C, int r, int r_t, int K,
                                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_KD_TOPK_H_ */
