// csrc/tdt_logprobs.hip -- pruned joiner log-probs of the token-and-duration transducer (TDT), forward and backward
// (MI355X addition, regular type only).  A joiner row has C + N columns: C token logits (the termination symbol among
// them) and N duration logits, the two heads normalised independently:
//     tok = log_softmax(row[:C]) - sigma,   dur = log_softmax(row[C:])
//   tdt_lse_kernel         the two log-sum-exps of every (b,t,k) row, one wave per row, 16-byte loads when (C+N) % 4 == 0
//   tdt_to_lattice_kernel  px [B,N,S,T+1]: px[b,i,s,t] = tok[sym] + dur[i], the move (s,t) -> (s+1, t+e_i); -inf where
//                          t + e_i > t_end, at column t_end and outside the band; the delay penalty added by source frame
//                          py [B,Ny,S+1,T]: py[b,j,s,t] = tok[blank] + dur[index of d_j], the move (s,t) -> (s, t+d_j), d_j
//                          the positive durations; -inf where t + d_j > t_end and outside the band
//   tdt_grad_kernel        one wave per row of glogits; GX = sum_i gx_i, GY = sum_j gy_j:
//                          g_tok[c] = -softmax_tok[c] (GX + GY) + 1[c == sym] GX + 1[c == blank] GY
//                          g_dur[n] = -softmax_dur[n] (GX + GY) + gx_n + gy_j(n)        (no gy term for duration 0)
// Kernels of their own, in the manner of the mb_* kernels of pruned_logprobs.hip, whose instantiations stay as they are.
// The band-shaped twins (include/ftr_band_tdt.h; the operands and occupancies of mi_band_tdt.hip, [B,N|Ny,T,r]):
//   tdt_to_band_kernel     px_band / py_band: the values tdt_to_lattice_kernel puts at lattice cell (ranges[b,t,0] + k, t),
//                          by the same arithmetic, one thread per band row and no lattice write
//   tdt_grad_kernel<.,true> the same gradient kernel reading gx_band / gy_band at the row itself
#include "ftr_common.h"
#include "launch.h"

namespace ftr {
namespace {

constexpr int TDT_MAXN = 5;

// e[n]: the durations; first = index of the first positive one (0 or 1), so blank move j uses duration column first + j
struct TdtCols { int e[TDT_MAXN]; int N; int first; };

template <bool VEC>
__global__ void tdt_lse_kernel(const float* __restrict__ logits, float* __restrict__ lse_tok, float* __restrict__ lse_dur,
                               size_t rows, int C, int N) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int W = C + N;
  const float* x = logits + row * W;
  float m = -INFINITY, s = 0.0f;
  if (VEC) {
    const f4u* x4 = reinterpret_cast<const f4u*>(x);
    const int n4 = (C + 3) >> 2;                      // the quads that hold a token column (W % 4 == 0: all inside the row)
    for (int i = lane; i < n4; i += 64) {
      const f4 v = x4[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) m = fmaxf(m, 4 * i + e < C ? v[e] : -INFINITY);
    }
    m = wave_max_dpp(m);
    for (int i = lane; i < n4; i += 64) {             // second pass hits L1/L2: a row is 2-8 KB
      const f4 v = x4[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) s += 4 * i + e < C ? __expf(v[e] - m) : 0.0f;
    }
  } else {
    for (int i = lane; i < C; i += 64) m = fmaxf(m, x[i]);
    m = wave_max_dpp(m);
    for (int i = lane; i < C; i += 64) s += __expf(x[i] - m);
  }
  s = wave_sum_dpp(s);
  if (lane == 0) {
    lse_tok[row] = m + __logf(s);
    float md = -INFINITY, sd = 0.0f;
    for (int n = 0; n < N; ++n) md = fmaxf(md, x[C + n]);
    for (int n = 0; n < N; ++n) sd += __expf(x[C + n] - md);
    lse_dur[row] = md + __logf(sd);
  }
}

// grid: (ceil((T+1)/256), S+1, B); thread <-> (b, s, t).  Writes py[b,:,s,t] (t < T) and px[b,:,s,t] (s < S, t <= T).
__global__ void tdt_to_lattice_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                                      const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                      const float* __restrict__ lse_tok, const float* __restrict__ lse_dur, int blank,
                                      const TdtCols tc, float sigma, double delay_penalty, float* __restrict__ px,
                                      float* __restrict__ py, int T, int S, int C, int r) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y, b = blockIdx.z;
  if (t > T) return;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const int W = C + tc.N, Ny = tc.N - tc.first;
  bool inband = false;
  float tokx = -INFINITY, toky = -INFINITY;
  float dur[TDT_MAXN];
#pragma unroll
  for (int n = 0; n < TDT_MAXN; ++n) dur[n] = -INFINITY;
  if (t < T) {
    const size_t bt = (size_t)b * T + t;
    const int s0 = ranges[bt * r];
    int k = s - s0;
    if (k < 0) k += S + 1;
    if (k < r) {
      inband = true;
      const size_t row = bt * r + k;
      const float* x = logits + row * W;
      const float l = lse_tok[row] + sigma, ld = lse_dur[row];
      toky = x[blank] - l;
      if (s < S) tokx = x[min(max(symbols[(size_t)b * S + s], 0), C - 1)] - l;
#pragma unroll
      for (int n = 0; n < TDT_MAXN; ++n)
        if (n < tc.N) dur[n] = x[C + n] - ld;
    }
#pragma unroll
    for (int n = 0; n < TDT_MAXN; ++n) {
      const int jj = n - tc.first;
      if (n < tc.N && jj >= 0)
        py[(((size_t)b * Ny + jj) * (S + 1) + s) * T + t] = (inband && t + tc.e[n] <= te) ? toky + dur[n] : -INFINITY;
    }
  }
  if (s < S) {
    double pen = 0.0;
    if (delay_penalty > 0.0) pen = (((double)te - 1.0) / 2.0 - (double)t) * delay_penalty;
#pragma unroll
    for (int n = 0; n < TDT_MAXN; ++n) {
      if (n < tc.N) {
        float vx = (inband && t != te && t + tc.e[n] <= te) ? tokx + dur[n] : -INFINITY;
        if (delay_penalty > 0.0) vx += (float)pen;
        px[(((size_t)b * tc.N + n) * S + s) * (T + 1) + t] = vx;
      }
    }
  }
}

// one thread per band row (b,t,k) <-> lattice cell (s,t), s = (ranges[b,t,0] + k) mod (S+1) as the lattice kernel's roll
__global__ void tdt_to_band_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                                   const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                   const float* __restrict__ lse_tok, const float* __restrict__ lse_dur, int blank,
                                   const TdtCols tc, float sigma, double delay_penalty, float* __restrict__ pxb,
                                   float* __restrict__ pyb, size_t rows, int T, int S, int C, int r) {
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const size_t bt = row / r;
  const int k = (int)(row - bt * r);
  const int b = (int)(bt / T);
  const int t = (int)(bt - (size_t)b * T);
  int s = ranges[bt * r] + k;
  if (s > S) s -= S + 1;
  const bool sok = s >= 0 && s <= S;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const int W = C + tc.N, Ny = tc.N - tc.first;
  const float* x = logits + row * W;
  const float l = lse_tok[row] + sigma, ld = lse_dur[row];
  const float toky = x[blank] - l;
  float tokx = -INFINITY;
  if (sok && s < S) tokx = x[min(max(symbols[(size_t)b * S + s], 0), C - 1)] - l;
  double pen = 0.0;
  if (delay_penalty > 0.0) pen = (((double)te - 1.0) / 2.0 - (double)t) * delay_penalty;
#pragma unroll
  for (int n = 0; n < TDT_MAXN; ++n) {
    if (n < tc.N) {
      const float dur = x[C + n] - ld;
      const size_t at = (((size_t)b * tc.N + n) * T + t) * r + k;
      float vx = (sok && s < S && t != te && t + tc.e[n] <= te) ? tokx + dur : -INFINITY;
      if (delay_penalty > 0.0) vx += (float)pen;
      pxb[at] = vx;
      const int jj = n - tc.first;
      if (jj >= 0) pyb[(((size_t)b * Ny + jj) * T + t) * r + k] = (sok && t + tc.e[n] <= te) ? toky + dur : -INFINITY;
    }
  }
}

template <bool VEC, bool BAND>
__global__ void tdt_grad_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                                const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                const float* __restrict__ lse_tok, const float* __restrict__ lse_dur,
                                const float* __restrict__ gpx, const float* __restrict__ gpy, const Scale scale, int blank,
                                const TdtCols tc, float* __restrict__ glogits, size_t rows, int T, int S, int C, int r) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int T1 = T + 1;
  const int W = C + tc.N, Ny = tc.N - tc.first;
  const size_t bt = row / r;
  const int k = (int)(row - bt * r);
  const int b = (int)(bt / T);
  const int t = (int)(bt - (size_t)b * T);
  const int s0 = ranges[bt * r];
  int s = s0 + k;                        // inverse of the roll: band slot k <-> lattice row (s0 + k) mod (S+1)
  if (s > S) s -= S + 1;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const float sc = scale.at(b);
  const bool sok = s >= 0 && s <= S;     // ranges are caller data: a row outside the lattice gets no gradient
  int sym = -1;
  if (sok && s < S) sym = min(max(symbols[(size_t)b * S + s], 0), C - 1);   // the column the forward read
  float gd[TDT_MAXN];                    // what duration column n takes directly: gx_n + gy_j(n)
  float GX = 0.0f, GY = 0.0f;
#pragma unroll
  for (int n = 0; n < TDT_MAXN; ++n) {
    float gx = 0.0f, gy = 0.0f;
    if (n < tc.N && sok && t + tc.e[n] <= te) {     // the cells that are -inf whatever the row holds get no gradient
      if (BAND) {                                   // gpx / gpy are [B,N,T,r] / [B,Ny,T,r]: the row's own element of each plane
        if (s < S && t != te) gx = gpx[(((size_t)b * tc.N + n) * T + t) * r + k] * sc;
        if (n >= tc.first) gy = gpy[(((size_t)b * Ny + (n - tc.first)) * T + t) * r + k] * sc;
      } else {
        if (s < S && t != te) gx = gpx[(((size_t)b * tc.N + n) * S + s) * T1 + t] * sc;
        if (n >= tc.first) gy = gpy[(((size_t)b * Ny + (n - tc.first)) * (S + 1) + s) * T + t] * sc;
      }
    }
    gd[n] = gx + gy;
    GX += gx;
    GY += gy;
  }
  const float tot = GX + GY;
  const float l = lse_tok[row], ld = lse_dur[row];
  const float* x = logits + row * W;
  float* g = glogits + row * W;
  auto column = [&](int c, float v) -> float {
    if (c < C) {
      float val = -tot * __expf(v - l);
      if (c == sym) val += GX;
      if (c == blank) val += GY;
      return val;
    }
    float val = -tot * __expf(v - ld);
#pragma unroll
    for (int n = 0; n < TDT_MAXN; ++n) val += (c - C == n) ? gd[n] : 0.0f;
    return val;
  };
  if (VEC) {
    const f4u* x4 = reinterpret_cast<const f4u*>(x);
    f4u* g4 = reinterpret_cast<f4u*>(g);
    const int n4 = W >> 2;
    for (int i = lane; i < n4; i += 64) {
      const f4 v = x4[i];
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = column(4 * i + e, v[e]);
      g4[i] = o;
    }
  } else {
    for (int c = lane; c < W; c += 64) g[c] = column(c, x[c]);
  }
}

TdtCols tdt_cols(const int32_t* durations, int N) {
  TdtCols tc;
  for (int n = 0; n < TDT_MAXN; ++n) tc.e[n] = n < N ? durations[n] : 0;
  tc.N = N;
  tc.first = durations[0] == 0 ? 1 : 0;
  return tc;
}
}  // namespace

int tdt_logprobs_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                     const int32_t* durations, int N, double sigma, double delay_penalty, float* lse_tok, float* lse_dur,
                     float* px, float* py, int B, int T, int S, int C, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("tdt_logprobs_fwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  dispatch(((C + N) & 3) == 0, [&](auto vec) {
    hipLaunchKernelGGL((tdt_lse_kernel<decltype(vec)::value>), dim3(blocks), dim3(64 * wpb), 0, st, logits, lse_tok, lse_dur, rows, C, N);
  });
  int rc = check_launch("tdt_lse");
  if (rc != FTR_OK) return rc;
  const int threads = 256;
  const dim3 grid((T + 1 + threads - 1) / threads, S + 1, B);
  hipLaunchKernelGGL(tdt_to_lattice_kernel, grid, dim3(threads), 0, st, logits, symbols, ranges, boundary, lse_tok, lse_dur,
                     blank, tdt_cols(durations, N), (float)sigma, delay_penalty, px, py, T, S, C, r);
  return check_launch("tdt_to_lattice");
}

int tdt_logprobs_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                     const int32_t* durations, int N, const float* lse_tok, const float* lse_dur, const float* gpx,
                     const float* gpy, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("tdt_logprobs_bwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  const TdtCols tc = tdt_cols(durations, N);
  dispatch(((C + N) & 3) == 0, [&](auto vec) {
    hipLaunchKernelGGL((tdt_grad_kernel<decltype(vec)::value, false>), dim3(blocks), dim3(64 * wpb), 0, st, logits, symbols, ranges, boundary,
                       lse_tok, lse_dur, gpx, gpy, scale, blank, tc, glogits, rows, T, S, C, r);
  });
  return check_launch("tdt_grad");
}

int tdt_band_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                 const int32_t* durations, int N, double sigma, double delay_penalty, float* lse_tok, float* lse_dur,
                 float* pxb, float* pyb, int B, int T, int S, int C, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("tdt_pruned_band_fwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  dispatch(((C + N) & 3) == 0, [&](auto vec) {
    hipLaunchKernelGGL((tdt_lse_kernel<decltype(vec)::value>), dim3(blocks), dim3(64 * wpb), 0, st, logits, lse_tok, lse_dur, rows, C, N);
  });
  int rc = check_launch("tdt_lse");
  if (rc != FTR_OK) return rc;
  hipLaunchKernelGGL(tdt_to_band_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, logits, symbols, ranges, boundary,
                     lse_tok, lse_dur, blank, tdt_cols(durations, N), (float)sigma, delay_penalty, pxb, pyb, rows, T, S, C, r);
  return check_launch("tdt_to_band");
}

int tdt_band_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                 const int32_t* durations, int N, const float* lse_tok, const float* lse_dur, const float* gxb,
                 const float* gyb, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("tdt_pruned_band_bwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  const TdtCols tc = tdt_cols(durations, N);
  dispatch(((C + N) & 3) == 0, [&](auto vec) {
    hipLaunchKernelGGL((tdt_grad_kernel<decltype(vec)::value, true>), dim3(blocks), dim3(64 * wpb), 0, st, logits, symbols, ranges, boundary,
                       lse_tok, lse_dur, gxb, gyb, scale, blank, tc, glogits, rows, T, S, C, r);
  });
  return check_launch("tdt_band_grad");
}

}  // namespace ftr
