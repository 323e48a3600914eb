/* include/ftr_prune_sum.h -- the prune gather fused with the joiner's first addition (MI355X addition): entry points of the
 * product library libftr_hip.so on top of ftr_lowp.h, whose element type codes (FTR_DTYPE_*) and conventions (return
 * codes, ftr_last_error(), the opaque stream, asynchrony) they share.  They are kept out of ftr.h and ftr_lowp.h, which
 * stay as they are symbol for symbol; ftr_abi_version() is unchanged by them. */
#ifndef FTR_PRUNE_SUM_H_
#define FTR_PRUNE_SUM_H_
#include "ftr_lowp.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * out[b,t,k,:] = am[b,t,:] + lm[b, ranges[b,t,k], :]: what a joiner computes first from the two results of
 * ftr_do_pruning_f32, without the gathered [B,T,r,C] tensor in between.  am [B,T,C], lm [B,S1,C] and out [B,T,r,C] have
 * the element type `kind` (an FTR_DTYPE_* code); rows of `ranges` [B,T,r] outside [0, S1 - 1] are clamped into it, as
 * ftr_do_pruning_f32 clamps them.  A 16-bit tensor stands for its exact float32 up-conversion: one float32 addition and
 * one rounding to nearest-even per element (NaN and +-inf as in IEEE arithmetic).
 *
 * The backward: given g_out [B,T,r,C] in the element type,
 *   d_am[b,t,:] = sum_k g_out[b,t,k,:]
 *   d_lm[b,s,:] = sum over (t,k) with ranges[b,t,k] == s of g_out[b,t,k,:]      (rows outside [0, S1 - 1] contribute nothing)
 * both accumulated in float32 in the summation order of ftr_do_pruning_bwd_ws_f32 called with g_am_pruned == g_lm_pruned ==
 * float(g_out), and rounded once into the element type.  With FTR_DTYPE_F32 it is that call.  No atomics: two runs give
 * the same bits.  `workspace`: ftr_do_pruning_bwd_workspace_bytes(B, T, S1, C, r) bytes, 16-byte aligned, for every
 * element type (the partial rows in it are float32).
 *
 * An unknown `kind` returns FTR_ERR_INVALID_ARG before anything else is looked at; the other checks are those of
 * ftr_do_pruning_f32 / ftr_do_pruning_bwd_ws_f32, with their replies.  Rows are contiguous (C elements); a 16-bit tensor
 * may start at any element, but is read and written four elements at a time only when C % 4 == 0 and its base address is
 * 8-byte aligned (else element by element; the backward then sums in increasing (t,k) order, which is the order of
 * ftr_do_pruning_bwd_ws_f32 at C % 4 != 0).  Both calls enqueue kernels only: they can be captured into a hipGraph.
 */
int ftr_do_pruning_sum_dt(const void* am, const void* lm, int kind, const int32_t* ranges, void* out, int B, int T, int S1,
                          int C, int r, void* stream);
int ftr_do_pruning_sum_bwd_ws_dt(const void* g_out, int kind, const int32_t* ranges, void* d_am, void* d_lm, int B, int T,
                                 int S1, int C, int r, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_PRUNE_SUM_H_ */
