/* include/ftr_band_viterbi.h -- best-path (Viterbi) alignment on the pruned band itself (MI355X addition): entry points
 * of the product library libftr_hip.so on top of ftr.h, whose conventions (return codes, ftr_last_error(), the opaque
 * stream, asynchrony, host duration arrays read at launch time) they share.  A header of its own, so that ftr.h and the
 * other headers stay as they are, symbol for symbol; ftr_abi_version() is unchanged by it. */
#ifndef FTR_BAND_VITERBI_H_
#define FTR_BAND_VITERBI_H_
#include "ftr.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * ftr_mutual_information_band_viterbi_f32: the alignment of ftr_mutual_information_viterbi_tdt_f32 on the band-shaped
 * operands of ftr_mutual_information_band_tdt_f32 (ftr_band_tdt.h).  No array of size S * T exists on this route.
 *
 * Operands.  px_band [B,N,T,r] and py_band [B,Ny,T,r], float32: element (b,i,t,k) belongs to lattice cell (s,t),
 *   s = ranges[b,t,0] + k, and is the value of move i out of that cell.  ranges [B,T,r] must be a band (ranges[b,t,k] =
 *   ranges[b,t,0] + k, ranges[b,t,0] non-decreasing over the frames of the boundary rectangle) with r <= 15.  boundary
 *   [B,4] rows (s_begin, t_begin, s_end, t_end), clamped into the lattice, or NULL.  token_durations e_0 < ... < e_{N-1}
 *   in 0..16 and blank_durations d_0 < ... < d_{Ny-1} in 1..32 (they need not contain 1) are host arrays; N >= 1,
 *   Ny >= 1, N + Ny <= 9: the domain of the lattice entry, not the narrower one of the band loss.
 * Cells and moves.  The cells are the band cells of the frames t_begin <= t < t_end inside the rectangle, and the end
 *   cell (s_end, t_end).  A token move i leads from (s,t) to (s+1, t+e_i), a blank move j to (s, t+d_j); a move exists
 *   iff its source and its destination are cells (the frames it skips need not be in the band).  Frames >= t_end are
 *   never read.
 * Values.  Moves m = 0 .. M-1 are the token moves in list order, then the blank moves in list order.  For every cell
 *   but (s_begin,t_begin)
 *       cand[m] = p[src_m] + op_m[src_m]      one float32 add; -inf for a move that does not exist
 *       best = cand[M-1]; move = M-1
 *       for m = M-2 .. 0:  take = isnan(cand[m]) || cand[m] >= best;  if (take) best = cand[m], move = m
 *       p[cell] = best
 *   with p[s_begin,t_begin] = 0 and score = p[s_end,t_end]: a NaN propagates, a tie goes to the lowest-index move.  One
 *   add per move and ordered selects; no float64, no exp, no log.
 * Outputs.  score [B] float32; frames [B,S], durations [B,S], blank_steps [B,T], int32, with the meaning they have in
 *   ftr_mutual_information_viterbi_tdt_f32: frames[b,s] the source frame of the token move the best path takes out of
 *   row s and durations[b,s] its duration, -1 on rows outside [s_begin,s_end); blank_steps[b,t] the duration of the
 *   blank the path takes out of frame t, 0 on the other frames of [t_begin,t_end) and -1 outside.  All three are -1
 *   throughout for an utterance whose score is -inf (no path) or NaN, and for an inverted rectangle, whose score is 0.  A
 *   band start that decreases inside the rectangle gives score NaN and -1 throughout.  Every element of every output is
 *   written by the launch; nothing needs clearing beforehand.  Should the backtrace meet a decision that is no move of
 *   its walk (believed unreachable with a finite score), frames, durations and blank_steps of that utterance are -1
 *   throughout.
 * Relation to the lattice route.  Where the operands obey the builders' -inf rules (as everything that
 *   ftr_pruned_band_fwd_f32 / _dt, ftr_tdt_pruned_band_fwd_f32 and ftr_multiblank_pruned_band_fwd_f32 write does), all
 *   four outputs equal, bit for bit, those of ftr_mutual_information_viterbi_tdt_f32 on the band scattered into lattices
 *   of -inf: a lattice cell outside the band has only -inf operands leading out of it, so every candidate is the same
 *   float, and the select order is the same.  With moves (0) / (1) score and frames also equal
 *   ftr_mutual_information_viterbi_f32.  One deviation: on the lattice a NaN also travels through cells outside the band
 *   (NaN + -inf); here it travels along moves that exist and along no other.  Bit equality with the lattice route is
 *   promised for rectangles without NaN.
 * Workspace.  ftr_mutual_information_band_viterbi_workspace_bytes(B,T,S,r,N,Ny) bytes, 8-byte aligned: with
 *   steps = S + T + 1 rounded up to a multiple of 4 and lanes = 8 (r <= 7) or 16,
 *   B * ((steps + 4) * lanes * (N + Ny + 1) * 4 + steps * lanes / 2); its contents before the call do not matter.
 *   Launches only (one): no memset or memcpy, no atomics, no host synchronisation -- capturable in a hipGraph; the same
 *   bits on every run.
 * ftr_mutual_information_band_viterbi_supported(T,S,r,N,Ny): 1 where the entry accepts these sizes, else 0 (then the
 *   workspace query returns 0).
 * Validation, in this order: the duration lists; sizes (FTR_ERR_INVALID_ARG); r and the move counts
 *   (FTR_ERR_UNSUPPORTED); B == 0 returns FTR_OK; the workspace size; the pointers (boundary may be NULL; frames and
 *   durations may be NULL only when S == 0); the workspace alignment; the device.
 */
int ftr_mutual_information_band_viterbi_supported(int T, int S, int r, int N, int Ny);
size_t ftr_mutual_information_band_viterbi_workspace_bytes(int B, int T, int S, int r, int N, int Ny);
int ftr_mutual_information_band_viterbi_f32(const float* px_band, const float* py_band, const int32_t* ranges,
                                            const int32_t* boundary, const int32_t* token_durations, int N,
                                            const int32_t* blank_durations, int Ny, void* workspace, size_t workspace_bytes,
                                            float* score, int32_t* frames, int32_t* durations, int32_t* blank_steps, int B,
                                            int T, int S, int r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_BAND_VITERBI_H_ */
