/* The top-K teacher cache in one pass (MI355X addition): the entry point of the product library libftr_hip.so that WRITES
 * what the stored-teacher distillation entries read, on top of ftr_lowp.h, whose element type codes (FTR_DTYPE_*) and
 * conventions (return codes, ftr_last_error(), the opaque stream, asynchrony) it shares.  A header of its own, so that every
 * other header stays as it is, symbol for symbol; ftr_abi_version() is unchanged by it. */
#ifndef FTR_KD_TOPK_TEACHER_H_
#define FTR_KD_TOPK_TEACHER_H_
#include "ftr_lowp.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * `logits` are `rows` contiguous rows of C elements (element type `kind`; a 16-bit tensor stands for its exact float32
 * up-conversion; a 16-bit base may be aligned to 2 bytes only): the teacher's joiner output on the teacher's own band.
 * Of every row the entry writes
 *   values  [rows,K], element type `kind`: the K selected elements themselves, bit for bit
 *   indices [rows,K] int32: their columns, distinct, in [0,C)
 *   rest    [rows] float32, or NULL = not wanted: logsumexp over the columns c NOT selected of row[c] / temperature, in
 *           float32 against its own maximum (never log(1 - ...)): exactly -inf when K == C or every such element is -inf,
 *           NaN when one of them is NaN (a row of more than K NaNs), else +inf when one of them is +inf
 * Selection and order are total, so the cache is the same bits from run to run.  Elements are taken in descending order of
 * their value compared as float32, where -0.0 and +0.0 are equal, every NaN is larger than +inf and equal to every other
 * NaN, and among equal elements the lower column comes first.  Slot j of a row holds element j of that order.
 * `boundary` [B,4] int32 or NULL: with it the rows are those of a [B,T,r,C] tensor (rows == B T r) and boundary[b] =
 * (s_begin, t_begin, s_end, t_end), of which t_begin and t_end are read, clamped into [0,T].  The rows of a frame t < t_begin
 * or t >= t_end are NEVER READ and get the filler values = 0, indices[j] = j, rest = 0.  Without it B, T and r are ignored.
 * Validation, in this order: (1) an unknown kind returns FTR_ERR_INVALID_ARG before anything else is looked at; (2) C >= 1 and
 * 1 <= K <= min(C, FTR_KD_TOPK_MAX_K); (3) a temperature that is not finite and > 0 (also when rest is NULL); (4) sizes:
 * rows >= 0, and with a boundary B >= 0, T >= 1, r >= 1, rows == B T r; rows == 0 returns FTR_OK; (5) the pointers
 * (boundary and rest may be NULL); (6) the device.  More than 2^31 - 1 rows are refused.
 * Launches only: no memset or memcpy, no host synchronisation, no workspace -- capturable in a hipGraph.
 */
#ifndef FTR_KD_TOPK_MAX_K
#define FTR_KD_TOPK_MAX_K 64
#endif
int ftr_kd_teacher_topk_dt(const void* logits, int kind, const int32_t* boundary, void* values, int32_t* indices, float* rest,
                           float temperature, int B, int T, int r, long long rows, int C, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_KD_TOPK_TEACHER_H_ */
