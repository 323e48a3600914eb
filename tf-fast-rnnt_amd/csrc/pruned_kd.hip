// csrc/pruned_kd.hip -- knowledge distillation on the pruned band (MI355X addition, no reference counterpart), gfx950.
// Student and teacher joiner logits x, y [B,T,r,C] on the same `ranges`; per valid node (b,t,k) the loss is KL(p || q) with
// p = softmax(y / tau), q = softmax(x / tau) over the C columns ("full"), or over three classes -- blank, the correct next
// symbol, everything else -- ("collapsed", Panchapagesan et al., ICASSP 2021).  No tau^2 factor.
//   kd_fwd_reg_kernel  one wave per row, both rows held in registers (C % 4 == 0, C <= 256 * NQ), every load issued
//                      before the first use, one pass: as lse_rows_reg_kernel of pruned_logprobs.hip, twice the registers
//   kd_fwd_kernel      any C: two passes over the row (the second hits L1/L2), four elements at a time or one by one
//   kd_utt_sum_kernel  node losses -> per-utterance loss, one block per utterance, fixed summation tree
//   kd_bwd_kernel      one streaming pass: d loss / d x from x, y and the normalisers the forward saved (no reduction)
// A node is valid iff t_begin <= t < t_end and s_begin <= ranges[b,t,k] <= s_end; validity is decided from ranges and
// boundary BEFORE any logits load, an invalid row is never read (padding frames of a joiner hold garbage), its node loss
// and normalisers are 0 and its gradient row is written as zeros.
// Saved normalisers, float32 planes of [B,T,r]: 0 = logsumexp(x / tau), 1 = logsumexp(y / tau), and in collapsed mode
// 2, 3 = the same over the "rest" columns only (a masked logsumexp with its own maximum, never log(1 - ...)).
// Element types of x and y are independent (float, bf16_t, fp16_t); a row is read four elements at a time only when BOTH
// tensors pass rows_vec4.  All arithmetic is float32; the gradient row is rounded once when it is stored in x's type.
#include "ftr_common.h"
#include "launch.h"

namespace ftr {
namespace {

__device__ __forceinline__ float wave_max(float v) { return wave_max_dpp(v); }
__device__ __forceinline__ float wave_sum(float v) { return wave_sum_dpp(v); }

// what a wave knows about its row before it touches the logits: is the node valid, whose utterance is it, and (collapsed)
// the columns of the blank class k0 and of the symbol class k1 (-1: the node has no symbol class)
struct KdRow { bool valid; int b, k0, k1; };

template <bool COLL>
__device__ __forceinline__ KdRow kd_row(size_t row, const int32_t* __restrict__ symbols, const int32_t* __restrict__ ranges,
                                        const int32_t* __restrict__ boundary, int blank, int T, int S, int C, int r) {
  KdRow g;
  const unsigned bt = (unsigned)row / (unsigned)r;   // rows < 2^31 (require_rows_32bit): 32-bit divisions, a tenth of the 64-bit ones
  g.b = (int)(bt / (unsigned)T);
  const int t = (int)(bt - (unsigned)g.b * (unsigned)T);
  const int s = ranges[row];
  const Bound bd = load_boundary(boundary, g.b, S, T);   // clamped into the lattice: s < se implies s < S below
  g.valid = t >= bd.tb && t < bd.te && s >= bd.sb && s <= bd.se;
  g.k0 = blank;
  g.k1 = -1;
  if (COLL && g.valid && s < bd.se) {
    const int c = min(max(symbols[(size_t)g.b * S + s], 0), C - 1);   // symbol kept in bounds, as the pruned builders do
    if (c != blank) g.k1 = c;
  }
  return g;
}

// x log(x / y) with the xlogy convention: a class of teacher mass 0 adds nothing, whatever the student says; NaN stays NaN
__device__ __forceinline__ float kd_term(float p, float logp_minus_logq) { return p == 0.0f ? 0.0f : p * logp_minus_logq; }

__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));   // a NaN among a, b, c comes out of the sum
}

template <bool COLL>
__device__ __forceinline__ void kd_store(float* __restrict__ node, float* __restrict__ saved, size_t rows, size_t row,
                                         float loss, float Ls, float Lt, float Rs, float Rt) {
  node[row] = loss;
  saved[row] = Ls;
  saved[rows + row] = Lt;
  if (COLL) {
    saved[2 * rows + row] = Rs;
    saved[3 * rows + row] = Rt;
  }
}

// The end of a forward row, from the wave-reduced sums.  ms, mt: the maxima the sums were taken against; ss, st: sums of
// exp(. - max); full: over all columns, kl = sum exp(y - mt) (y - x); collapsed: over the rest columns, and xb, xs, yb,
// ys are the blank and symbol logits (xs = ys = -inf without a symbol class).  Everything is already divided by tau.
template <bool COLL>
__device__ __forceinline__ void kd_finish(float* __restrict__ node, float* __restrict__ saved, size_t rows, size_t row,
                                          float ms, float ss, float mt, float st, float kl, float xb, float xs, float yb,
                                          float ys) {
  if (!COLL) {
    const float Ls = ms + __logf(ss), Lt = mt + __logf(st);
    kd_store<false>(node, saved, rows, row, kl / st - (Lt - Ls), Ls, Lt, 0.0f, 0.0f);
  } else {
    const float Rs = ms + __logf(ss), Rt = mt + __logf(st);   // no rest column at all: -inf + log 0 = -inf
    const float Ls = lse3(Rs, xb, xs), Lt = lse3(Rt, yb, ys);
    const float lpb = yb - Lt, lps = ys - Lt, lpr = Rt - Lt;
    // the hardware exp / log, as in the sums: this tail runs once per row, and with the library forms it took longer than the row
    const float loss = kd_term(__expf(lpb), lpb - (xb - Ls)) + kd_term(__expf(lps), lps - (xs - Ls)) + kd_term(__expf(lpr), lpr - (Rs - Ls));
    kd_store<true>(node, saved, rows, row, loss, Ls, Lt, Rs, Rt);
  }
}

// a maximum to subtract that is never -inf (a row, or a rest class, of -inf only: exp(-inf - 0) = 0, not exp(NaN))
__device__ __forceinline__ float kd_safe_max(float m) { return m == -INFINITY ? 0.0f : m; }

template <typename ES, typename ET, int NQ, bool COLL>
__global__ __launch_bounds__(256) void kd_fwd_reg_kernel(const ES* __restrict__ x, const ET* __restrict__ y,
                                                         const int32_t* __restrict__ symbols, const int32_t* __restrict__ ranges,
                                                         const int32_t* __restrict__ boundary, int blank, float inv_tau,
                                                         float* __restrict__ node, float* __restrict__ saved, size_t rows,
                                                         int T, int S, int C, int r) {
  const int lane = threadIdx.x & 63;
  const size_t rowi = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (rowi >= rows) return;
  const size_t row = rows - 1 - rowi;   // last rows first: the tail of a tensor that was just written is what the cache still holds
  const KdRow g = kd_row<COLL>(row, symbols, ranges, boundary, blank, T, S, C, r);
  if (!g.valid) {
    if (lane == 0) kd_store<COLL>(node, saved, rows, row, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const int n4 = C >> 2;
  const f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const ES* xr = x + row * C;
  const ET* yr = y + row * C;
  f4 v[NQ], w[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    v[q] = (i < n4) ? load4(xr, i) : ninf;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    w[q] = (i < n4) ? load4(yr, i) : ninf;
  }
  float xb = -INFINITY, xs = -INFINITY, yb = -INFINITY, ys = -INFINITY;
  if (COLL) {   // the class logits, by every lane from the same address: lines this wave is fetching anyway
    xb = elem_to_float(xr[g.k0]) * inv_tau;
    yb = elem_to_float(yr[g.k0]) * inv_tau;
    if (g.k1 >= 0) {
      xs = elem_to_float(xr[g.k1]) * inv_tau;
      ys = elem_to_float(yr[g.k1]) * inv_tau;
    }
  }
  float ms = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * (lane + 64 * q) + e;
      const bool cls = COLL && (c == g.k0 || c == g.k1);   // collapsed: the sums run over the rest columns
      v[q][e] = cls ? -INFINITY : v[q][e] * inv_tau;
      w[q][e] = cls ? -INFINITY : w[q][e] * inv_tau;
    }
    ms = fmaxf(fmaxf(ms, fmaxf(v[q][0], v[q][1])), fmaxf(v[q][2], v[q][3]));
    mt = fmaxf(fmaxf(mt, fmaxf(w[q][0], w[q][1])), fmaxf(w[q][2], w[q][3]));
  }
  ms = kd_safe_max(wave_max(ms));
  mt = kd_safe_max(wave_max(mt));
  float ss = 0.0f, st = 0.0f, kl = 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // lanes past the row hold -inf: exp gives 0 and the kl term is skipped
      ss += __expf(v[q][e] - ms);
      const float p = __expf(w[q][e] - mt);
      st += p;
      if (!COLL) kl += kd_term(p, w[q][e] - v[q][e]);
    }
  }
  ss = wave_sum(ss);
  st = wave_sum(st);
  if (!COLL) kl = wave_sum(kl);
  if (lane == 0) kd_finish<COLL>(node, saved, rows, row, ms, ss, mt, st, kl, xb, xs, yb, ys);
}

// any C, one wave per row, two passes (the second hits L1/L2: a row is a few KB)
template <typename ES, typename ET, bool VEC, bool COLL>
__global__ void kd_fwd_kernel(const ES* __restrict__ x, const ET* __restrict__ y, const int32_t* __restrict__ symbols,
                              const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary, int blank,
                              float inv_tau, float* __restrict__ node, float* __restrict__ saved, size_t rows, int T, int S,
                              int C, int r) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const KdRow g = kd_row<COLL>(row, symbols, ranges, boundary, blank, T, S, C, r);
  if (!g.valid) {
    if (lane == 0) kd_store<COLL>(node, saved, rows, row, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const ES* xr = x + row * C;
  const ET* yr = y + row * C;
  float xb = -INFINITY, xs = -INFINITY, yb = -INFINITY, ys = -INFINITY;
  if (COLL) {
    xb = elem_to_float(xr[g.k0]) * inv_tau;
    yb = elem_to_float(yr[g.k0]) * inv_tau;
    if (g.k1 >= 0) {
      xs = elem_to_float(xr[g.k1]) * inv_tau;
      ys = elem_to_float(yr[g.k1]) * inv_tau;
    }
  }
  float ms = -INFINITY, mt = -INFINITY, ss = 0.0f, st = 0.0f, kl = 0.0f;
  if (VEC) {
    const int n4 = C >> 2;
    for (int i = lane; i < n4; i += 64) {
      const f4 v = load4(xr, i), w = load4(yr, i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * i + e;
        const bool cls = COLL && (c == g.k0 || c == g.k1);
        ms = fmaxf(ms, cls ? -INFINITY : v[e] * inv_tau);
        mt = fmaxf(mt, cls ? -INFINITY : w[e] * inv_tau);
      }
    }
    ms = kd_safe_max(wave_max(ms));
    mt = kd_safe_max(wave_max(mt));
    for (int i = lane; i < n4; i += 64) {
      const f4 v = load4(xr, i), w = load4(yr, i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * i + e;
        const bool cls = COLL && (c == g.k0 || c == g.k1);
        const float a = cls ? -INFINITY : v[e] * inv_tau, b = cls ? -INFINITY : w[e] * inv_tau;
        ss += __expf(a - ms);
        const float p = __expf(b - mt);
        st += p;
        if (!COLL) kl += kd_term(p, b - a);
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      const bool cls = COLL && (c == g.k0 || c == g.k1);
      ms = fmaxf(ms, cls ? -INFINITY : elem_to_float(xr[c]) * inv_tau);
      mt = fmaxf(mt, cls ? -INFINITY : elem_to_float(yr[c]) * inv_tau);
    }
    ms = kd_safe_max(wave_max(ms));
    mt = kd_safe_max(wave_max(mt));
    for (int c = lane; c < C; c += 64) {
      const bool cls = COLL && (c == g.k0 || c == g.k1);
      const float a = cls ? -INFINITY : elem_to_float(xr[c]) * inv_tau, b = cls ? -INFINITY : elem_to_float(yr[c]) * inv_tau;
      ss += __expf(a - ms);
      const float p = __expf(b - mt);
      st += p;
      if (!COLL) kl += kd_term(p, b - a);
    }
  }
  ss = wave_sum(ss);
  st = wave_sum(st);
  if (!COLL) kl = wave_sum(kl);
  if (lane == 0) kd_finish<COLL>(node, saved, rows, row, ms, ss, mt, st, kl, xb, xs, yb, ys);
}

// utt[b] = sum of the T * r node losses of utterance b: one block per utterance, a fixed summation tree (deterministic)
__global__ __launch_bounds__(256) void kd_utt_sum_kernel(const float* __restrict__ node, float* __restrict__ utt, int per) {
  __shared__ float red[4];
  const float* p = node + (size_t)blockIdx.x * per;
  float s = 0.0f;
  for (int i = threadIdx.x; i < per; i += 256) s += p[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) utt[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// d loss / d x[c] of one element, a = x[c] / tau.  k = upstream gradient / tau.
//   full:      k (q_c - p_c)
//   collapsed: k (Q_j - P_j) w_c for c in class j, Q / P the student's / teacher's class masses and w_c the share of column
//              c in its class: 1 for the blank and the symbol, exp(a - Rs) for a rest column (q_c = Q_rest exp(a - Rs))
// Either way a student that equals the teacher gets exact zeros: both sides of every difference are computed alike.
struct KdGrad {
  float k, Ls, Lt, Rs, db, ds, dr;
  int k0, k1;
  template <bool COLL>
  __device__ __forceinline__ float at(int c, float a, float b) const {
    if (!COLL) return k * (__expf(a - Ls) - __expf(b - Lt));
    return k * (c == k0 ? db : c == k1 ? ds : (dr == 0.0f ? 0.0f : dr * __expf(a - Rs)));
  }
};

template <typename ES, typename ET, bool VEC, bool COLL>
__global__ void kd_bwd_kernel(const ES* __restrict__ x, const ET* __restrict__ y, const int32_t* __restrict__ symbols,
                              const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary, int blank,
                              float inv_tau, const float* __restrict__ saved, const Scale scale, ES* __restrict__ gx,
                              size_t rows, int T, int S, int C, int r) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const KdRow g = kd_row<COLL>(row, symbols, ranges, boundary, blank, T, S, C, r);
  ES* gr = gx + row * C;
  if (!g.valid) {   // zeros, without a look at the logits
    if (VEC) {
      const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int i = lane; i < (C >> 2); i += 64) store4(gr, i, zero);
    } else {
      for (int c = lane; c < C; c += 64) gr[c] = elem_from_float<ES>(0.0f);
    }
    return;
  }
  const ES* xr = x + row * C;
  const ET* yr = y + row * C;
  KdGrad d;
  d.k = scale.at(g.b) * inv_tau;
  d.Ls = saved[row];
  d.Lt = saved[rows + row];
  d.Rs = 0.0f; d.db = 0.0f; d.ds = 0.0f; d.dr = 0.0f;
  d.k0 = g.k0; d.k1 = g.k1;
  if (COLL) {   // the teacher enters through its three class masses only: two of its logits and Rt, not its row
    d.Rs = saved[2 * rows + row];
    d.db = __expf(elem_to_float(xr[g.k0]) * inv_tau - d.Ls) - __expf(elem_to_float(yr[g.k0]) * inv_tau - d.Lt);
    if (g.k1 >= 0) d.ds = __expf(elem_to_float(xr[g.k1]) * inv_tau - d.Ls) - __expf(elem_to_float(yr[g.k1]) * inv_tau - d.Lt);
    d.dr = __expf(d.Rs - d.Ls) - __expf(saved[3 * rows + row] - d.Lt);
  }
  if (VEC) {
    const int n4 = C >> 2;
    for (int i = lane; i < n4; i += 64) {
      const f4 v = load4(xr, i);
      f4 w = {0.0f, 0.0f, 0.0f, 0.0f};
      if (!COLL) w = load4(yr, i);
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = d.at<COLL>(4 * i + e, v[e] * inv_tau, w[e] * inv_tau);
      store4(gr, i, o);
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      const float b = COLL ? 0.0f : elem_to_float(yr[c]) * inv_tau;
      gr[c] = elem_from_float<ES>(d.at<COLL>(c, elem_to_float(xr[c]) * inv_tau, b));
    }
  }
}

// both element types -> one call of f(elem_tag<ES>, elem_tag<ET>)
template <typename F>
inline auto dispatch_dtype2(int dtype, int teacher_dtype, F&& f) {
  return dispatch_dtype(dtype, [&](auto s) { return dispatch_dtype(teacher_dtype, [&](auto t) { return f(s, t); }); });
}

}  // namespace

int pruned_kd_fwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols,
                  const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed,
                  float* node, float* saved, float* utt, int B, int T, int S, int C, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("pruned_kd_fwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  const float inv_tau = 1.0f / temperature;
  dispatch_dtype2(dtype, teacher_dtype, [&](auto stag, auto ttag) {
    using ES = typename decltype(stag)::type;
    using ET = typename decltype(ttag)::type;
    const ES* x = static_cast<const ES*>(logits);
    const ET* y = static_cast<const ET*>(teacher);
    const bool vec4 = rows_vec4<ES>(C, x) && rows_vec4<ET>(C, y);
    dispatch(collapsed != 0, [&](auto coll) {
      constexpr bool COLL = decltype(coll)::value;
      if (vec4 && C <= 2048)   // both rows fit the registers of a wave: 1, 2, 4 or 8 quads of elements per lane and tensor
        dispatch_among<1, 2, 4, 8>(C <= 256 ? 1 : C <= 512 ? 2 : C <= 1024 ? 4 : 8, [&](auto n) {
          hipLaunchKernelGGL((kd_fwd_reg_kernel<ES, ET, decltype(n)::value, COLL>), dim3(blocks), dim3(64 * wpb), 0, st, x, y, symbols,
                             ranges, boundary, blank, inv_tau, node, saved, rows, T, S, C, r);
        });
      else
        dispatch(vec4, [&](auto vec) {
          hipLaunchKernelGGL((kd_fwd_kernel<ES, ET, decltype(vec)::value, COLL>), dim3(blocks), dim3(64 * wpb), 0, st, x, y, symbols,
                             ranges, boundary, blank, inv_tau, node, saved, rows, T, S, C, r);
        });
    });
  });
  { const int rc = check_launch("pruned_kd_fwd"); if (rc != FTR_OK) return rc; }
  hipLaunchKernelGGL(kd_utt_sum_kernel, dim3(B), dim3(256), 0, st, node, utt, T * r);
  return check_launch("pruned_kd_utt_sum");
}

int pruned_kd_bwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols,
                  const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed,
                  const float* saved, Scale scale, void* glogits, int B, int T, int S, int C, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("pruned_kd_bwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  const float inv_tau = 1.0f / temperature;
  dispatch_dtype2(dtype, teacher_dtype, [&](auto stag, auto ttag) {
    using ES = typename decltype(stag)::type;
    using ET = typename decltype(ttag)::type;
    const ES* x = static_cast<const ES*>(logits);
    const ET* y = static_cast<const ET*>(teacher);
    dispatch(rows_vec4<ES>(C, x, glogits) && rows_vec4<ET>(C, y), [&](auto vec) {
      dispatch(collapsed != 0, [&](auto coll) {
        hipLaunchKernelGGL((kd_bwd_kernel<ES, ET, decltype(vec)::value, decltype(coll)::value>), dim3(blocks), dim3(64 * wpb), 0, st, x, y,
                           symbols, ranges, boundary, blank, inv_tau, saved, scale, static_cast<ES*>(glogits), rows, T, S, C, r);
      });
    });
  });
  return check_launch("pruned_kd_bwd");
}

// kd_utt_sum_kernel for the factored forms of pruned_kd_fact.hip: the same kernel, the same summation tree
int pruned_kd_utt_sum(const float* node, float* utt, int B, int per, hipStream_t st) {
  hipLaunchKernelGGL(kd_utt_sum_kernel, dim3(B), dim3(256), 0, st, node, utt, per);
  return check_launch("pruned_kd_utt_sum");
}

}  // namespace ftr
