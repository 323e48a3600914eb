/* include/ftr_joiner_act.h -- the pruned joiner's input with its activation fused in (MI355X addition): entry points of the
 * product library libftr_hip.so on top of ftr_lowp.h, whose element type codes (FTR_DTYPE_*) and conventions (return
 * codes, ftr_last_error(), the opaque stream, asynchrony) they share.  They are kept out of the other headers, which stay
 * as they are symbol for symbol; ftr_abi_version() is unchanged by them. */
#ifndef FTR_JOINER_ACT_H_
#define FTR_JOINER_ACT_H_
#include "ftr_lowp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* activation codes (`act`) */
#define FTR_ACT_TANH 1
#define FTR_ACT_RELU 2

/*
 * out[b,t,k,:] = act(am[b,t,:] + lm[b, ranges[b,t,k], :]): the tensor a joiner hands to its output layer, without the
 * gathered rows or the sum in memory.  am [B,T,C], lm [B,S1,C] and out [B,T,r,C] have the element type `kind` (an
 * FTR_DTYPE_* code); rows of `ranges` [B,T,r] outside [0, S1 - 1] are clamped into it, as ftr_do_pruning_f32 clamps them.
 * A 16-bit tensor stands for its exact float32 up-conversion: z is one float32 addition, act(z) is computed in float32
 * and rounded once, to nearest-even, into the element type.
 *   FTR_ACT_RELU: z < 0 ? 0 : z (a NaN stays a NaN).
 *   FTR_ACT_TANH: NaN -> NaN, +-inf -> +-1, 0 -> 0, |out| <= 1 for every input; before the final rounding the float32
 *                 value is within a few float32 ulps of tanh(z) relative to the result, for tiny |z| too.
 *
 * The backward: given g_out [B,T,r,C] and the forward's `out`, both in the element type,
 *   dz = g_out * (1 - out * out)   (tanh; three separately rounded float32 operations)
 *   dz = out <= 0 ? 0 : g_out      (relu; a NaN in `out` passes g_out)
 *   d_am[b,t,:] = sum_k dz[b,t,k,:]
 *   d_lm[b,s,:] = sum over (t,k) with ranges[b,t,k] == s of dz[b,t,k,:]      (rows outside [0, S1 - 1] contribute nothing)
 * both accumulated in float32 in the summation order of ftr_do_pruning_bwd_ws_f32 called with the float32 tensor dz as
 * both gradients, and rounded once into the element type.  dz itself is never stored.  No atomics: two runs give the
 * same bits.  `workspace`: ftr_do_pruning_bwd_workspace_bytes(B, T, S1, C, r) bytes, 16-byte aligned, for every element
 * type (the partial rows in it are float32).
 *
 * An unknown `kind` returns FTR_ERR_INVALID_ARG before anything else is looked at, an unknown `act` next; the other
 * checks are those of ftr_do_pruning_f32 / ftr_do_pruning_bwd_ws_f32, with their replies (`out` of the backward is one of
 * the pointers checked).  Rows are contiguous (C elements); a 16-bit tensor may start at any element, but is read and
 * written four elements at a time only when C % 4 == 0 and its base address is 8-byte aligned (else element by element;
 * the backward then sums in increasing (t,k) order, which is the order of ftr_do_pruning_bwd_ws_f32 at C % 4 != 0).
 * Both calls enqueue kernels only: they can be captured into a hipGraph.
 */
int ftr_pruned_joiner_act_dt(const void* am, const void* lm, int kind, int act, const int32_t* ranges, void* out,
                             int B, int T, int S1, int C, int r, void* stream);
int ftr_pruned_joiner_act_bwd_ws_dt(const void* g_out, const void* out, int kind, int act, const int32_t* ranges,
                                    void* d_am, void* d_lm, int B, int T, int S1, int C, int r,
                                    void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_JOINER_ACT_H_ */
