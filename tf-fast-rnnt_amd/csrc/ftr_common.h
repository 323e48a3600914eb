// csrc/ftr_common.h -- shared by every translation unit of libftr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/ftr_kd_fact.h"  // and, through it, ftr_kd.h, ftr_lowp.h and ftr.h
#include "../../include/ftr_kd_loss.h"
#include "../../include/ftr_kd_loss_fact.h"
#include "../../include/ftr_kd_topk.h"
#include "../../include/ftr_prune_sum.h"
#include "../../include/ftr_joiner_act.h"
#include "../../include/ftr_fused.h"
#include "../../include/ftr_band_tdt.h"
#include "../../include/ftr_tdt_mix.h"
#include "../../include/ftr_band_multiblank.h"
#include "../../include/ftr_band_viterbi.h"

namespace ftr {

// error text of the last failing call on this thread (ftr_last_error()).
void set_error(const char* fmt, ...);
void clear_error();

// Checks the launch that was just enqueued (no sync: hipGetLastError only reports launch-time errors).
inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return FTR_ERR_LAUNCH;
  }
  return FTR_OK;
}

// Element counts and offsets of the [B,T,s_range,C]-shaped tensors are size_t everywhere; the number of their ROWS (B*T*s_range,
// and the B*T frames of the prune gather) stays 32-bit: grid sizes are unsigned, and the kernels derive int b / t from a row.
inline int require_rows_32bit(const char* what, size_t rows) {
  if (rows > 0x7fffffffull) {
    set_error("%s: %zu rows (B*T*s_range) exceed the 2^31 - 1 that the launch grids index", what, rows);
    return FTR_ERR_INVALID_ARG;
  }
  return FTR_OK;
}

// Zero fill / device copy of 32-bit words as KERNELS.  Not hipMemsetAsync / hipMemcpyAsync: a memset node captured into a
// hipGraph writes the right value on the first replay only on this ROCm (scripts/graph_memset_probe.py: garbage from the
// second replay on), and every launch of this library must be capturable -- the recursion's hand-off region is cleared by
// such a node whenever the caller does not vouch for a clean workspace.
__global__ void zero_words_kernel(uint32_t* __restrict__ p, size_t n);
__global__ void copy_words_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, size_t n);
inline int zero_words(void* p, size_t n_words, hipStream_t st, const char* what) {
  if (n_words == 0) return FTR_OK;
  const size_t blocks = (n_words + 4 * 256 - 1) / (4 * 256);
  hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, static_cast<uint32_t*>(p), n_words);
  return check_launch(what);
}
inline int copy_words(void* dst, const void* src, size_t n_words, hipStream_t st, const char* what) {
  if (n_words == 0) return FTR_OK;
  const size_t blocks = (n_words + 255) / 256;
  hipLaunchKernelGGL(copy_words_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, static_cast<uint32_t*>(dst),
                     static_cast<const uint32_t*>(src), n_words);
  return check_launch(what);
}

// A "minus infinity" that stays finite under the additions of the recursion, so the dependent chain
// needs no NaN guard: anything <= NEG_THRESH is reported as -inf when it leaves a kernel.
constexpr float kNeg = -1.0e30f;
constexpr float kNegThresh = -1.0e29f;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// 16-byte vector with 4-byte alignment: lattice rows have odd lengths (T+1), so row starts are only
// dword aligned; amdhsa runs in unaligned-access mode and these lower to global_load/store_dwordx4.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ---- element types of the joiner logits and of their gradient (the FTR_DTYPE_* codes of ftr_lowp.h): float, or 16 bits of
// storage.  A 16-bit value is up-converted on load (exact), every kernel computes in float32 as before, and a store
// rounds once, to nearest-even (NaN stays NaN, -inf stays -inf, overflow goes to inf, fp16 subnormals are kept).  Plain C++
// conversions: the compiler picks v_cvt_f32_f16 / v_cvt_f16_f32 and the bf16 forms of gfx950.
struct bf16_t { uint16_t bits; };
struct fp16_t { uint16_t bits; };
// four 16-bit elements, one 8-byte access.  Naturally aligned: the launchers take the vector path of a 16-bit tensor only when
// its base is 8-byte aligned and C % 4 == 0 (every row then is), since a contiguous 16-bit view may start at an odd element
typedef uint16_t h4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float elem_to_float(float v) { return v; }
__device__ __forceinline__ float elem_to_float(bf16_t v) { return (float)__builtin_bit_cast(__bf16, v.bits); }
__device__ __forceinline__ float elem_to_float(fp16_t v) { return (float)__builtin_bit_cast(_Float16, v.bits); }
template <typename E> __device__ __forceinline__ E elem_from_float(float v);
template <> __device__ __forceinline__ float elem_from_float<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t elem_from_float<bf16_t>(float v) { return bf16_t{__builtin_bit_cast(uint16_t, (__bf16)v)}; }
template <> __device__ __forceinline__ fp16_t elem_from_float<fp16_t>(float v) { return fp16_t{__builtin_bit_cast(uint16_t, (_Float16)v)}; }

// elements 4i .. 4i+3 of a row as floats, and back (float rows: the f4u access above, any dword-aligned row)
__device__ __forceinline__ f4 load4(const float* row, int i) { return reinterpret_cast<const f4u*>(row)[i]; }
__device__ __forceinline__ void store4(float* row, int i, f4 v) { reinterpret_cast<f4u*>(row)[i] = v; }
template <typename E>
__device__ __forceinline__ f4 load4(const E* row, int i) {
  const h4 h = reinterpret_cast<const h4*>(row)[i];
  f4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = elem_to_float(E{h[e]});
  return v;
}
template <typename E>
__device__ __forceinline__ void store4(E* row, int i, f4 v) {
  h4 h;
#pragma unroll
  for (int e = 0; e < 4; ++e) h[e] = elem_from_float<E>(v[e]).bits;
  reinterpret_cast<h4*>(row)[i] = h;
}
// store4 as a non-temporal store: for streams far beyond any cache that the kernel does not read again
__device__ __forceinline__ void store4_nt(float* row, int i, f4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f4u*>(row) + i); }
template <typename E>
__device__ __forceinline__ void store4_nt(E* row, int i, f4 v) {
  h4 h;
#pragma unroll
  for (int e = 0; e < 4; ++e) h[e] = elem_from_float<E>(v[e]).bits;
  __builtin_nontemporal_store(h, reinterpret_cast<h4*>(row) + i);
}

// Per-utterance factor applied to incoming lattice gradients on the fly: (p ? p[b * stride] : 1) * mul.
// stride 0 = one scalar for the whole batch (reduction "sum"/"mean"), mul carries the sign and the 1/B of "mean".
struct Scale {
  const float* p; int stride; float mul;
  __device__ __forceinline__ float at(int b) const { return (p ? p[(size_t)b * stride] : 1.0f) * mul; }
};
inline Scale scale_none() { return Scale{nullptr, 0, 1.0f}; }

// Wave64 reductions on the VALU (DPP row shifts + row broadcasts, result read from lane 63) instead of six LDS
// round trips (ds_bpermute): the row kernels do two of these per 2-4 KB row.  Every lane gets the result.
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ float dpp_take(float identity, float src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity), __builtin_bit_cast(int, src),
                                                               CTRL, ROW_MASK, BANK_MASK, false));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dpp_take<0x111, 0xf, 0xf>(0.0f, v);   // row_shr:1
  v += dpp_take<0x112, 0xf, 0xf>(0.0f, v);   // row_shr:2
  v += dpp_take<0x114, 0xf, 0xe>(0.0f, v);   // row_shr:4
  v += dpp_take<0x118, 0xf, 0xc>(0.0f, v);   // row_shr:8  -> lane 15 of every row holds the row's sum
  v += dpp_take<0x142, 0xa, 0xf>(0.0f, v);   // row_bcast:15 into rows 1 and 3
  v += dpp_take<0x143, 0xc, 0xf>(0.0f, v);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  constexpr float ninf = -__builtin_inff();
  v = fmaxf(v, dpp_take<0x111, 0xf, 0xf>(ninf, v));
  v = fmaxf(v, dpp_take<0x112, 0xf, 0xf>(ninf, v));
  v = fmaxf(v, dpp_take<0x114, 0xf, 0xe>(ninf, v));
  v = fmaxf(v, dpp_take<0x118, 0xf, 0xc>(ninf, v));
  v = fmaxf(v, dpp_take<0x142, 0xa, 0xf>(ninf, v));
  v = fmaxf(v, dpp_take<0x143, 0xc, 0xf>(ninf, v));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ int wave_max_int_dpp(int v) {   // the same ladder on integers (identity: the smallest int)
  constexpr int lo = -2147483647 - 1;
  v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x111, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x112, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x114, 0xf, 0xe, false));
  v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x118, 0xf, 0xc, false));
  v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x142, 0xa, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x143, 0xc, 0xf, false));
  return __builtin_amdgcn_readlane(v, 63);
}

// ---- per-utterance shift of the recursion's operands (mi_wave_bidir.hip, mi_band.hip)
// The recursion is invariant under px -> px - cx, py -> py - cy with constants per utterance: every complete path takes
// the same number of px steps (s_end - s_begin) and of py steps (t_end - t_begin; modified: minus the px steps), so both
// incoming terms of every cell move together -- split ratios, occupancies and gradients are unchanged and `ans` moves
// by a known amount, which the cut reduction adds back.  What the shift buys is float32 accuracy: unshifted, p(s,t)
// reaches -5e3 .. -1e5 (log2 units) on a long lattice, one ulp there is 5e-4 .. 8e-3, and the split ratio is formed from
// the DIFFERENCE of two such numbers (the reference's own arithmetic has the same defect: term1 / term2 at
// mutual_information_cuda.cu:642-660 subtract them in the backward pass).  With cx, cy chosen so that a path along the
// rectangle's diagonal gains nothing on average -- cx = mean(px) - ln f, cy = mean(py) - ln(1 - f), f = the fraction of
// px steps -- p stays within tens to hundreds along the paths that carry the occupancy.  The means are estimates (a
// fixed sample, or the band itself): any finite constants are exact in exact arithmetic.
struct Shift { float cx2, cy2; };   // log2 domain
__device__ __forceinline__ bool shift_sample_ok(float v) { return v > -1.0e4f && v < 1.0e4f; }   // not -inf / NaN / a huge stand-in for -inf
template <bool MOD>
__device__ __forceinline__ Shift shift_from_sums(float sumx, float nx, float sumy, float ny, int Sn, int Tn) {
  const float steps = MOD ? (float)(Tn - 1) : (float)(Sn - 1 + Tn - 1);
  float f = steps > 0.0f ? (float)(Sn - 1) / steps : 0.5f;
  f = fminf(fmaxf(f, 1.0e-3f), 1.0f - 1.0e-3f);
  const float mx = nx > 0.0f ? sumx / nx : 0.0f, my = ny > 0.0f ? sumy / ny : 0.0f;
  Shift s;
  s.cx2 = mx * kLog2e - __builtin_amdgcn_logf(f);
  s.cy2 = my * kLog2e - __builtin_amdgcn_logf(1.0f - f);
  return s;
}
// what the shifts took out of `ans` (log2 units): px steps * cx2 + py steps * cy2 of any complete path
template <bool MOD>
__device__ __forceinline__ double shift_total(const Shift s, int Sn, int Tn) {
  const int nx = Sn - 1, ny = MOD ? (Tn - 1) - (Sn - 1) : (Tn - 1);
  return (double)nx * (double)s.cx2 + (double)ny * (double)s.cy2;
}

struct Bound { int sb, tb, se, te; };
__device__ __forceinline__ Bound load_boundary(const int32_t* __restrict__ boundary, int b, int S, int T) {
  Bound r;
  if (boundary) {
    // clamped into the lattice: a malformed row then behaves like its intersection with [0,S] x [0,T] instead of
    // sending a kernel out of bounds (the reference only asserts shapes, mutual_information_cuda.cu:773-785)
    r.sb = max(boundary[4 * b + 0], 0); r.tb = max(boundary[4 * b + 1], 0);
    r.se = min(boundary[4 * b + 2], S); r.te = min(boundary[4 * b + 3], T);
  } else { r.sb = 0; r.tb = 0; r.se = S; r.te = T; }
  return r;
}

// HAT normalisation of one joiner row (pruned_logprobs.hip, mi_band.hip)
// softplus(v) = log(1 + e^v), with relative accuracy in both tails (log1pf, never logf(1 + ...))
__device__ __forceinline__ float softplus(float v) { return fmaxf(v, 0.0f) + log1pf(expf(-fabsf(v))); }
// HAT log-probs of one row from its blank logit xb, the symbol's logit xs and Z: *vy = log sigmoid(xb),
// *vx = xs - Z - softplus(xb), -inf for a symbol that is the blank
__device__ __forceinline__ void hat_logprobs(float xb, float xs, float Z, bool sym_is_blank, float* vx, float* vy) {
  *vy = -softplus(-xb);
  *vx = sym_is_blank ? -INFINITY : (xs - Z) - softplus(xb);
}
// sigmoid(xb) and sigmoid(-xb), each accurate in its small tail
__device__ __forceinline__ void hat_sigmoids(float xb, float* sp, float* sn) {
  const float e = expf(-fabsf(xb)), big = 1.0f / (1.0f + e), small = e / (1.0f + e);
  *sp = xb >= 0.0f ? big : small;
  *sn = xb >= 0.0f ? small : big;
}

}  // namespace ftr

// launchers implemented in the kernel files (all return FTR_OK / FTR_ERR_*), called from capi.hip
namespace ftr {
int mi_plain_fwd(const float* px, const float* py, const int32_t* boundary, float* p, float* ans, int B, int S, int T, int modified, hipStream_t st);
int mi_plain_bwd(const float* px, const float* py, const int32_t* boundary, const float* p, float* p_grad, float* px_grad, float* py_grad, float* ans_grad, int overwrite, int B, int S, int T, int modified, hipStream_t st);
int mi_bidir_fwd(const float* px, const float* py, const int32_t* boundary, float* ws, size_t ws_floats, int flags, float* ans, int B, int S, int T, int modified, hipStream_t st);
int mi_bidir_bwd(const int32_t* boundary, const float* ws, size_t ws_floats, int flags, float* px_grad, float* py_grad, float* ans_grad, int overwrite, int B, int S, int T, int modified, hipStream_t st, const float* ans = nullptr, float* loss_out = nullptr, int loss_code = 0);
int mi_bidir_ws_init(float* ws, size_t ws_floats, int B, int S, int T, hipStream_t st);
int mi_bidir_status(const float* ws, size_t ws_floats, int B, int S, int T, int* status_host, long long* dirty_host, hipStream_t st);
size_t mi_bidir_workspace_floats(int B, int S, int T);
size_t mi_bidir_handoff_floats(int B, int S, int T);
size_t mi_viterbi_workspace_bytes(int B, int S, int T);
int mi_viterbi(const float* px, const float* py, const int32_t* boundary, void* ws, size_t ws_bytes, float* score, int32_t* frames, int B, int S, int T, int modified, hipStream_t st);
size_t mi_multiblank_workspace_floats(int B, int S, int T);
int mi_multiblank_fwd(const float* px, const float* py, const int32_t* boundary, const int32_t* durations, int D, float* ws, size_t ws_floats, float* ans, int B, int S, int T, hipStream_t st);
int mi_multiblank_bwd(const float* px, const float* py, const int32_t* boundary, const int32_t* durations, int D, float* ws, size_t ws_floats, const float* ans_grad, float* px_grad, float* py_grad, int B, int S, int T, hipStream_t st);
// multi-blank twins of pruned_logprobs_fwd / _bwd (regular type): big_ids[D-1] and durations[D] are host arrays
int multiblank_logprobs_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* big_ids, const int32_t* durations, int D, double sigma, double delay_penalty, float* lse, float* px, float* py, int B, int T, int S, int C, int r, hipStream_t st);
int multiblank_logprobs_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* big_ids, const int32_t* durations, int D, const float* lse, const float* gpx, const float* gpy, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st);
// TDT (token-and-duration transducer): csrc/mi_tdt.hip and csrc/tdt_logprobs.hip; the duration lists are host arrays
size_t mi_tdt_workspace_floats(int B, int S, int T);
int mi_tdt_fwd(const float* px, const float* py, const int32_t* boundary, const int32_t* token_durations, int Dx, const int32_t* blank_durations, int Dy, float* ws, size_t ws_floats, float* ans, int B, int S, int T, hipStream_t st);
int mi_tdt_bwd(const float* px, const float* py, const int32_t* boundary, const int32_t* token_durations, int Dx, const int32_t* blank_durations, int Dy, float* ws, size_t ws_floats, const float* ans_grad, float* px_grad, float* py_grad, int B, int S, int T, hipStream_t st);
int tdt_logprobs_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* durations, int N, double sigma, double delay_penalty, float* lse_tok, float* lse_dur, float* px, float* py, int B, int T, int S, int C, int r, hipStream_t st);
int tdt_logprobs_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* durations, int N, const float* lse_tok, const float* lse_dur, const float* gpx, const float* gpy, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st);
// TDT on the pruned band (include/ftr_band_tdt.h): csrc/mi_band_tdt.hip and the band-shaped builders of csrc/tdt_logprobs.hip
// which move lists an entry point of the band chain admits: up to max_tok token and max_blk blank moves, durations up to
// max_dur (a token of duration e reaches e + 1 steps back, a blank of duration d reaches d)
struct BandMoveDomain { int max_tok, max_blk, max_dur; };
constexpr BandMoveDomain kBandTdtDomain{5, 5, 16};          // include/ftr_band_tdt.h
constexpr BandMoveDomain kBandMultiblankDomain{1, 8, 32};   // include/ftr_band_multiblank.h: one token move of duration 0
int mi_band_tdt_supported(int T, int S, int r, int N, int Ny, BandMoveDomain dom);
size_t mi_band_tdt_workspace_floats(int B, int T, int S, int r, int N, int Ny, BandMoveDomain dom);
int mi_band_tdt(const float* pxb, const float* pyb, const int32_t* ranges, const int32_t* boundary, const int32_t* token_durations, int N, const int32_t* blank_durations, int Ny, float* ws, size_t ws_floats, float* ans, float* gxb, float* gyb, int B, int T, int S, int r, BandMoveDomain dom, const char* what, hipStream_t st);
int tdt_band_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* durations, int N, double sigma, double delay_penalty, float* lse_tok, float* lse_dur, float* pxb, float* pyb, int B, int T, int S, int C, int r, hipStream_t st);
int tdt_band_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* durations, int N, const float* lse_tok, const float* lse_dur, const float* gxb, const float* gyb, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st);
// the omega mix of the TDT and the ordinary loss (include/ftr_tdt_mix.h): the <MIX> instantiations of csrc/tdt_logprobs.hip;
// band != 0: band-shaped planes, else the lattices; parts: bit 1 the TDT planes, bit 2 the ordinary ones
int tdt_mix_fwd(int band, const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* durations, int N, double sigma, int parts, double delay_penalty, float* lse_tok, float* lse_dur, float* px, float* py, float* px0, float* py0, int B, int T, int S, int C, int r, hipStream_t st);
int tdt_mix_bwd(int band, const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* durations, int N, const float* lse_tok, const float* lse_dur, const float* gpx, const float* gpy, const float* gpx0, const float* gpy0, Scale scale, Scale scale0, float* glogits, int B, int T, int S, int C, int r, hipStream_t st);
// multi-blank on the pruned band (include/ftr_band_multiblank.h): the chain of csrc/mi_band_tdt.hip in its multi-blank
// domain and the band-shaped builders of csrc/pruned_logprobs.hip
int mi_band_multiblank(const float* pxb, const float* pyb, const int32_t* ranges, const int32_t* boundary, const int32_t* durations, int D, float* ws, size_t ws_floats, float* ans, float* gxb, float* gyb, int B, int T, int S, int r, hipStream_t st);
int multiblank_band_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* big_ids, const int32_t* durations, int D, double sigma, double delay_penalty, float* lse, float* pxb, float* pyb, int B, int T, int S, int C, int r, hipStream_t st);
int multiblank_band_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const int32_t* big_ids, const int32_t* durations, int D, const float* lse, const float* gxb, const float* gyb, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st);
// best-path alignment over the TDT / multi-blank lattice: csrc/mi_viterbi_tdt.hip; the duration lists are host arrays
size_t mi_viterbi_tdt_workspace_bytes(int B, int S, int T);
int mi_viterbi_tdt(const float* px, const float* py, const int32_t* boundary, const int32_t* token_durations, int Dx, const int32_t* blank_durations, int Dy, void* ws, size_t ws_bytes, float* score, int32_t* frames, int32_t* durations, int32_t* blank_steps, int B, int S, int T, hipStream_t st);
// best-path alignment on the pruned band (include/ftr_band_viterbi.h): csrc/mi_band_viterbi.hip; the duration lists are host arrays
int mi_band_viterbi_supported(int T, int S, int r, int N, int Ny);
size_t mi_band_viterbi_workspace_bytes(int B, int T, int S, int r, int N, int Ny);
int mi_band_viterbi(const float* pxb, const float* pyb, const int32_t* ranges, const int32_t* boundary, const int32_t* token_durations, int N, const int32_t* blank_durations, int Ny, void* ws, size_t ws_bytes, float* score, int32_t* frames, int32_t* durations, int32_t* blank_steps, int B, int T, int S, int r, hipStream_t st);
int cummin_i32(const int32_t* in, int32_t* out, int rows, int cols, hipStream_t st);
int prune_ranges(const float* px_grad, const float* py_grad, const int32_t* boundary, int32_t* ranges, int32_t* s_begin, int B, int S, int T, int T1, int r, hipStream_t st);
int do_pruning(const float* am, const float* lm, const int32_t* ranges, float* am_p, float* lm_p, int B, int T, int S1, int C, int r, hipStream_t st);
size_t do_pruning_bwd_workspace_bytes(int B, int T, int S1, int C, int r);
int do_pruning_bwd_ws(const float* g_am_p, const float* g_lm_p, const int32_t* ranges, float* d_am, float* d_lm, int B, int T, int S1, int C, int r, void* ws, size_t ws_bytes, hipStream_t st);
int do_pruning_bwd(const float* g_am_p, const float* g_lm_p, const int32_t* ranges, float* d_am, float* d_lm, int B, int T, int S1, int C, int r, hipStream_t st);
// the gather fused with the joiner's addition (include/ftr_prune_sum.h); dtype: the element type of am / lm / out and of g / d_am / d_lm.
// do_pruning_sum_bwd_ws takes the routes of do_pruning_bwd_ws with one g for both inputs, and its workspace: float32 through the
// do_pruning_bwd_* kernels themselves, a 16-bit type through gather_sum_bwd_* with no activation (prune.hip)
int do_pruning_sum(const void* am, const void* lm, int dtype, const int32_t* ranges, void* out, int B, int T, int S1, int C, int r, hipStream_t st);
int do_pruning_sum_bwd_ws(const void* g, int dtype, const int32_t* ranges, void* d_am, void* d_lm, int B, int T, int S1, int C, int r, void* ws, size_t ws_bytes, hipStream_t st);
// the same with an activation behind the addition (include/ftr_joiner_act.h); act: FTR_ACT_*, validated by the caller.  The backward
// forms dz from g and the forward's out as it loads them; routes and workspace of do_pruning_bwd_ws.  The same kernel family as the
// sum (gather_sum_kernel, gather_sum_bwd_*), instantiated with the activation
int pruned_joiner_act(const void* am, const void* lm, int dtype, int act, const int32_t* ranges, void* out, int B, int T, int S1, int C, int r, hipStream_t st);
int pruned_joiner_act_bwd_ws(const void* g, const void* out, int dtype, int act, const int32_t* ranges, void* d_am, void* d_lm, int B, int T, int S1, int C, int r, void* ws, size_t ws_bytes, hipStream_t st);
// hat != 0: the HAT normalisation (lse = non-blank normaliser Z, see pruned_logprobs.hip); hat == 0: the ordinary kernels
// dtype: the element type of logits / glogits (FTR_DTYPE_*, validated by the caller: dtype_ok)
int pruned_logprobs_fwd(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, double delay_penalty, float* lse, float* px, float* py, int B, int T, int S, int C, int r, int modified, int hat, hipStream_t st);
int pruned_logprobs_bwd(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const float* lse, const float* gpx, const float* gpy, Scale scale, void* glogits, int B, int T, int S, int C, int r, int modified, int hat, hipStream_t st);
int simple_rowmax_exp(const float* x, float* probs, float* rowmax, float* rowsum, const float* dotvec, float* dot, size_t rows, int C, hipStream_t st);
int simple_rowmax_exp_pair(const float* x1, float* probs1, float* rowmax1, size_t rows1, const float* x2, float* probs2, float* rowmax2, size_t rows2, int C, hipStream_t st);
int simple_rowdot(const float* x, const float* v, float* dot, size_t rows, int C, hipStream_t st);
size_t simple_colsum_workspace_floats(size_t rows, int C);
int simple_colsum_weighted(const float* x, const float* w, float* out, float* ws, size_t ws_floats, size_t rows, int C, hipStream_t st);
int simple_logprobs_fwd(const float* am, const float* lm, const int32_t* symbols, const float* prod, const float* am_max, const float* lm_max, const int32_t* boundary, int blank, double delay_penalty, const float* lmonly_norm, const float* amonly_norm, const float* ulog, float cs, float ls, float as, float* px, float* py, int B, int T, int S, int C, int modified, hipStream_t st);
int simple_logprobs_bwd_w(const float* gpx, const float* gpy, Scale scale, const float* prod, const int32_t* boundary, float* W, float* rsx, float* rsy, float cs, int B, int T, int S, int modified, hipStream_t st, int32_t* live = nullptr);   // live [B,S+1,2]: the rows' live frame intervals
int bwd_live_dense();   // FTR_BWD_LIVE=dense: the W kernel reports every interval as [0, T)
int simple_logprobs_bwd_am(const float* gpx, const float* gpy, Scale scale, const float* damp, const float* am_probs, const int32_t* symbols, const int32_t* boundary, int blank, float kdir, const float* uvec, const float* amdot, float as, float* Rout, float* d_am, int B, int T, int S, int C, int modified, hipStream_t st);
int simple_logprobs_bwd_lm(const float* dlmp, const float* lm_probs, const int32_t* symbols, const float* rsx, const float* rsy, int blank, float kdir, const float* arow, const float* invsum, const float* gu, float* d_lm, int B, int S, int C, hipStream_t st);
int simple_fused_supported(int C);
int simple_fused_bwd_supported(int T, int C);
int normalizer_gemm(int kind, const float* x, const float* y, float* out, int B, int T, int S1, int C, hipStream_t st);
int normalizer_gemm_choice(int kind, int B, int T, int S1, int C, int* solution, float* us, float* us_default, int* candidates);
int normalizer_gemm_set_choice(int kind, int B, int T, int S1, int C, int solution);
int simple_fused_fwd(const float* am, const float* lm, const int32_t* symbols, const float* am_probs, const float* lm_probs, const float* am_max, const float* lm_max, const int32_t* boundary, int blank, double delay_penalty, const float* lmonly_norm, const float* amonly_norm, const float* ulog, float cs, float ls, float as, float* px, float* py, float* prod_out, int B, int T, int S, int C, int modified, hipStream_t st);
int simple_fused_bwd_am(const float* gpx, const float* gpy, Scale scale, const float* prod, const float* lm_probs, const float* am_probs, const int32_t* symbols, const int32_t* boundary, int blank, float cs, float kdir, const float* uvec, const float* amdot, float as, float* Rout, float* d_am, int B, int T, int S, int C, int modified, hipStream_t st);
int simple_fused_bwd_columns(int B, int T, int C);   // columns per workgroup (128 | 256) the W-operand kernel takes for a shape
int simple_fused_bwd_am_w(const float* gpx, const float* gpy, Scale scale, const float* W, const float* lm_probs, const float* am_probs, const int32_t* symbols, const int32_t* boundary, int blank, float kdir, const float* uvec, const float* amdot, float as, float* Rout, float* d_am, int B, int T, int S, int C, int modified, hipStream_t st, const int32_t* live = nullptr);   // live: what simple_logprobs_bwd_w wrote next to W
int negated_reduce(const float* ans, int B, int reduction, float* out, hipStream_t st, float sign = -1.0f);   // sign = +1: the plain reduction
// knowledge distillation on the pruned band: csrc/pruned_kd.hip (collapsed != 0: the three-class form; hat != 0: the HAT rows; n_dur: duration columns at the end of a row of width W; weights [B,T,r] or NULL; saved: 2 + 2 collapsed + 2 with n_dur > 0 planes of [B,T,r]; hat = n_dur = 0 and weights = NULL: the plain form)
int pruned_kd_fwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed, int hat, int n_dur, float dur_weight, const float* weights, float* node, float* saved, float* utt, int B, int T, int S, int W, int r, hipStream_t st);
int pruned_kd_bwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed, int hat, int n_dur, float dur_weight, const float* weights, const float* saved, Scale scale, void* glogits, int B, int T, int S, int W, int r, hipStream_t st);
// the same pass carrying the transducer loss on the band (include/ftr_kd_loss.h; plain form): the forward also writes lse and the band operands, the backward adds the band gradient; a Scale with mul == 0: that part is not read
int pruned_band_kd_fact_fwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed, double delay_penalty, int modified, float* lse, float* pxb, float* pyb, float* node, float* saved, float* utt, int B, int T, int S, int W, int r, int hat, const float* weights, hipStream_t st);
int pruned_band_kd_fact_bwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed, const float* lse, const float* gxb, const float* gyb, Scale scale, const float* saved, Scale kd_scale, void* glogits, int B, int T, int S, int W, int r, int hat, const float* weights, hipStream_t st);
int pruned_kd_weighted_utt_sum(const float* node, const float* weights, float* utt, int B, int per, hipStream_t st);   // utt[b] = sum of w * node in kd_utt_sum's tree
int band_node_occupancy(const float* gxb, const float* gyb, const int32_t* ranges, const int32_t* boundary, float* occ, int B, int T, int S, int r, hipStream_t st);
int kd_utt_sum(const float* node, float* utt, int B, int per, hipStream_t st);   // utt[b] = the sum of utterance b's `per` node losses, a fixed summation tree
// the same loss from a stored top-K teacher on the teacher's own band: csrc/pruned_kd_topk.hip (include/ftr_kd_topk.h; tranges NULL: the student's ranges; rest, weights: NULL or [B,T,r_t] / [B,T,r]; saved: 3 planes of [B,T,r])
int pruned_kd_topk_fwd(const void* logits, int dtype, const void* tvalues, int teacher_dtype, const int32_t* tindices, const int32_t* ranges, const int32_t* tranges, const int32_t* boundary, const float* rest, const float* weights, float temperature, float* node, float* saved, float* utt, int B, int T, int S, int C, int r, int rt, int K, hipStream_t st);
int pruned_kd_topk_bwd(const void* logits, int dtype, const void* tvalues, int teacher_dtype, const int32_t* tindices, const int32_t* ranges, const int32_t* tranges, const int32_t* boundary, const float* rest, const float* weights, float temperature, const float* saved, Scale scale, void* glogits, int B, int T, int S, int C, int r, int rt, int K, hipStream_t st);
int lse_rows(const float* logits, float* lse, size_t rows, int C, int blank, int hat, hipStream_t st);
int lse_rows_dtype(const void* logits, int dtype, float* lse, size_t rows, int C, int blank, int hat, hipStream_t st);
int mi_band_supported(int T, int S, int r);
int band_ranges_check(const int32_t* ranges, const int32_t* boundary, int* flags, int B, int T, int r, hipStream_t st);
int band_gather(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, const float* lse, int blank, double delay_penalty, float* pxb, float* pyb, int B, int T, int S, int C, int r, int modified, int hat, hipStream_t st);
size_t mi_band_workspace_floats(int B, int T, int S, int r);
int mi_band_seg_supported(int T, int S, int r);
size_t mi_band_seg_workspace_floats(int B, int T, int S, int r);
int mi_band_seg(const float* pxb, const float* pyb, const int32_t* ranges, const int32_t* boundary, float* ws, size_t ws_floats, float* ans, float* gxb, float* gyb, int B, int T, int S, int r, int modified, hipStream_t st);
int mi_band(const float* pxb, const float* pyb, const int32_t* ranges, const int32_t* boundary, float* ws, size_t ws_floats, float* ans, float* gxb, float* gyb, int B, int T, int S, int r, int modified, hipStream_t st);
int band_grad_banded(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, const float* lse, const float* gxb, const float* gyb, Scale scale, void* glogits, int B, int T, int S, int C, int r, int modified, int hat, hipStream_t st);
int selftest(hipStream_t st, int* result_dev);
int debug_stamps(unsigned long long* out16);
int debug_trace(unsigned long long* out, int n);
}
