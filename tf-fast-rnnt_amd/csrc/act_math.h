// csrc/act_math.h -- the activations fused behind the joiner's addition (include/ftr_joiner_act.h): y = act(z)
// in float32 for the forward, dz = g * act'(y) from the stored y for the backward.  Device only, plain C++.
#pragma once
#include "ftr_common.h"

namespace ftr {

// tanh(z) in float32, branch-free: both arms are computed and one is selected, so a wave never diverges on its data.
//   |z| <  0.625: z + z s P(s), s = z^2, P of degree 5 fitted to (tanh(z)/z - 1)/s on [0, 0.625^2] with weight s (flat
//                 relative error in y): exact for tiny z (s underflows to 0 and y = z), relative error about 1.2 * 2^-24.
//   |z| >= 0.625: 1 - 2 / (e + 1), e = 2^(|z| * 2 log2 e).  y >= 0.55 there, so the subtraction cancels at most one
//                 bit.  What is left is e's relative error times 2 e / ((e + 1)^2 y) <= 0.62, so everything else is
//                 made small: the rounding of the exponent's product is recovered with one fma and applied to e to first
//                 order, e + 1 is kept as an exact pair (d, dl), and the hardware reciprocal is corrected by one Newton
//                 step against that pair.  |z| is clamped at 10 (tanh(10) rounds to 1), which keeps the Newton step away
//                 from inf * 0.
// Over 2^25 arguments (uniform in [-3, 3] and log-spaced from 1e-30 to 12) the largest error after the final rounding is
// 2.27 * 2^-24 |tanh z| on MI355X, the math library's tanhf: 2.46; without the three corrections it is 2.90.
// Results: NaN -> NaN, +-inf -> +-1, 0 -> 0 with its sign, and |y| <= 1 for every input (w >= 0 below).
__device__ __forceinline__ float act_tanh(float z) {
  const float a = __builtin_fabsf(z);
  const float s = z * z;
  float p = 0x1.18dc90p-9f;
  p = __builtin_fmaf(p, s, -0x1.0bf26ep-7f);
  p = __builtin_fmaf(p, s, 0x1.638a80p-6f);
  p = __builtin_fmaf(p, s, -0x1.b9ee70p-5f);
  p = __builtin_fmaf(p, s, 0x1.111066p-3f);
  p = __builtin_fmaf(p, s, -0x1.555554p-2f);
  const float ys = __builtin_fmaf(z, s * p, z);

  constexpr float K = 2.0f * kLog2e;                                       // 2 log2(e), rounded
  constexpr float Klo = (float)(2.0 * 1.4426950408889634074 - (double)K);  // what the rounding dropped
  const float ac = __builtin_fminf(a, 10.0f);                              // drops a NaN; the select at the end restores it
  const float m = ac * K;
  const float lo = __builtin_fmaf(ac, Klo, __builtin_fmaf(ac, K, -m));     // |z| 2 log2 e - m
  float e = __builtin_amdgcn_exp2f(m);                                     // v_exp_f32; m in [1.8, 28.9]: no scaling needed
  e = __builtin_fmaf(e * kLn2, lo, e);
  const float d = e + 1.0f;
  const float dl = 1.0f - (d - e);                                         // e >= 1: d + dl = e + 1 exactly
  float w = __builtin_amdgcn_rcpf(d);
  const float r = __builtin_fmaf(-dl, w, __builtin_fmaf(-d, w, 1.0f));     // 1 - (d + dl) w
  w = __builtin_fmaf(w, r, w);
  const float yl = __builtin_copysignf(__builtin_fmaf(-2.0f, w, 1.0f), z);
  return a >= 0.625f ? yl : ys;                                            // a NaN takes the polynomial arm, which keeps it
}

// NaN stays NaN (z < 0 is false for it), as torch.relu
__device__ __forceinline__ float act_relu(float z) { return z < 0.0f ? 0.0f : z; }

// no activation: what the gather-sum kernels of prune.hip are instantiated with for the plain sum (include/ftr_prune_sum.h).
// Internal to csrc, not an FTR_ACT_* code: the entries of capi.hip go on refusing everything but tanh and relu.
constexpr int ACT_NONE = 0;
static_assert(ACT_NONE != FTR_ACT_TANH && ACT_NONE != FTR_ACT_RELU, "ACT_NONE must not be a public activation code");

template <int ACT>
__device__ __forceinline__ float act_fwd(float z) {
  if constexpr (ACT == ACT_NONE) return z;
  else return ACT == FTR_ACT_TANH ? act_tanh(z) : act_relu(z);
}
template <int ACT>
__device__ __forceinline__ f4 act_fwd4(f4 z) {
  f4 y;
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = act_fwd<ACT>(z[e]);
  return y;
}

// dz = g act'(y).  tanh: three separately rounded float32 operations (never an fma); relu: torch's rule, a NaN y passes g;
// none: g, whatever y is
template <int ACT>
__device__ __forceinline__ float act_dz(float g, float y) {
  if (ACT == ACT_NONE) return g;
  if (ACT == FTR_ACT_TANH) return __fmul_rn(g, __fsub_rn(1.0f, __fmul_rn(y, y)));
  return y <= 0.0f ? 0.0f : g;
}
template <int ACT>
__device__ __forceinline__ f4 act_dz4(f4 g, f4 y) {
  f4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = act_dz<ACT>(g[e], y[e]);
  return v;
}

}  // namespace ftr
