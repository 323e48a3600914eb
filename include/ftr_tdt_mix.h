/* include/ftr_tdt_mix.h -- the TDT loss mixed with the ordinary transducer loss on the token head of the same joiner rows
 * (NeMo's `omega`; MI355X addition): entry points of the product library libftr_hip.so on top of ftr_band_tdt.h, whose
 * conventions (return codes, ftr_last_error(), the opaque stream, asynchrony, host duration arrays read at launch time) they
 * share.  A header of its own, so that ftr.h and the other headers stay as they are, symbol for symbol; ftr_abi_version()
 * is unchanged by it. */
#ifndef FTR_TDT_MIX_H_
#define FTR_TDT_MIX_H_
#include "ftr_band_tdt.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * The mixed loss of an utterance is L = (1 - omega) L_tdt + omega L_rnnt.  L_tdt is the TDT loss of the builders of ftr.h /
 * ftr_band_tdt.h; L_rnnt is the ordinary loss (regular type) whose operands are px0 = tok[sym] and py0 = tok[blank],
 * tok = log_softmax(row[:C]) of the same row: sigma is not applied to them, the delay penalty is (by source frame).  Their
 * normaliser is lse_tok, so one pass over the logits serves both, and the gradient of both w.r.t. a row is one pass too.
 *
 * `parts`: bit 1 (FTR_TDT_MIX_TDT) the TDT planes px / py are written, bit 2 (FTR_TDT_MIX_RNNT) the ordinary planes
 *   px0 / py0; 1..3.  The planes of an absent part are not touched and may be NULL.  lse_tok and lse_dur are always written.
 * ftr_tdt_mix_pruned_band_fwd_f32: ftr_tdt_pruned_band_fwd_f32 that also writes px0_band / py0_band [B,T,r], the values
 *   ftr_pruned_band_fwd_f32 (modified = 0) writes for logits[..., :C] given the same log-sum-exp.
 * ftr_tdt_mix_pruned_logprobs_fwd_f32: ftr_tdt_pruned_logprobs_fwd_f32 that also writes px0 [B,S,T+1] / py0 [B,S+1,T], the
 *   values of ftr_pruned_logprobs_fwd_f32 (modified = 0) likewise.
 * ftr_tdt_mix_pruned_band_bwd_scaled_f32: the gradient of the mix w.r.t. logits from the band-shaped occupancies of both
 *   recursions.  With up[b] = scale ? scale[b * scale_stride] : 1, w1 = up[b] * mul_tdt and w2 = up[b] * mul_rnnt (a caller
 *   passes mul_tdt = (1 - omega) m, mul_rnnt = omega m), GX / GY / gd[n] the TDT totals of
 *   ftr_tdt_pruned_band_bwd_scaled_f32 at scale w1 and gx0 / gy0 the ordinary occupancies of the row's cell under the masks of
 *   ftr_pruned_band_bwd_scaled_f32 (modified = 0), X = GX + w2 gx0 and Y = GY + w2 gy0:
 *       g_tok[c] = -softmax_tok[c] (X + Y) + 1[c == sym] X + 1[c == blank] Y
 *       g_dur[n] = -softmax_dur[n] (GX + GY) + gd[n]
 *   Every element of glogits [B,T,r,C+N] is written.  A part whose multiplier is 0 is not read (its planes may be NULL);
 *   with mul_tdt == 0 the duration columns are exact zeros.
 * ftr_tdt_mix_pruned_logprobs_bwd_scaled_f32: the same from full-size occupancies gpx [B,N,S,T+1], gpy [B,Ny,S+1,T],
 *   gpx0 [B,S,T+1], gpy0 [B,S+1,T].
 * All four launch only: no memset or memcpy, no host synchronisation -- capturable in a hipGraph.
 * Validation, in the order of their twins with the new arguments after sigma: the duration list, sigma, termination_symbol;
 *   `parts` (forward) or the two multipliers, which must be finite (backward); sizes; s_range (forward) or scale_stride
 *   (backward); B == 0 returns FTR_OK; the pointers of the parts that are present (boundary may be NULL; symbols and the
 *   lattice-shaped px / px0 / gpx / gpx0 may be NULL when S == 0); the device.
 */
#define FTR_TDT_MIX_TDT 1
#define FTR_TDT_MIX_RNNT 2

int ftr_tdt_mix_pruned_band_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                    const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                    double sigma, int parts, double delay_penalty, float* lse_tok, float* lse_dur,
                                    float* px_band, float* py_band, float* px0_band, float* py0_band, int B, int T, int S,
                                    int C, int r, void* stream);
int ftr_tdt_mix_pruned_logprobs_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                        const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                        double sigma, int parts, double delay_penalty, float* lse_tok, float* lse_dur,
                                        float* px, float* py, float* px0, float* py0, int B, int T, int S, int C, int r,
                                        void* stream);
int ftr_tdt_mix_pruned_band_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                           const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                           double sigma, double delay_penalty, const float* lse_tok, const float* lse_dur,
                                           const float* gx_band, const float* gy_band, const float* gx0_band,
                                           const float* gy0_band, const float* scale, int scale_stride, float mul_tdt,
                                           float mul_rnnt, float* glogits, int B, int T, int S, int C, int r, void* stream);
int ftr_tdt_mix_pruned_logprobs_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                               const int32_t* boundary, int termination_symbol, const int32_t* durations,
                                               int N, double sigma, double delay_penalty, const float* lse_tok,
                                               const float* lse_dur, const float* gpx, const float* gpy, const float* gpx0,
                                               const float* gpy0, const float* scale, int scale_stride, float mul_tdt,
                                               float mul_rnnt, float* glogits, int B, int T, int S, int C, int r,
                                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FTR_TDT_MIX_H_ */
