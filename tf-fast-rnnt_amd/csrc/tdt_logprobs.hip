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
// MIX (include/ftr_tdt_mix.h): the ordinary transducer loss on the token head of the same rows, for the omega mix
//     L = (1 - omega) L_tdt + omega L_rnnt.  The <MIX = true> builders also write px0 / py0, the operands of the regular
//     type (tok[sym] / tok[blank] with tok = log_softmax(row[:C]), no sigma; what band_gather_kernel of mi_band.hip and
//     band_to_lattice_kernel of pruned_logprobs.hip write for the token columns), and `parts` says which of the two sets of
//     planes a launch writes; the <MIX = true> gradient kernel adds the ordinary occupancies gx0 / gy0 with a multiplier of
//     their own, X = w1 GX + w2 gx0, Y = w1 GY + w2 gy0:
//                          g_tok[c] = -softmax_tok[c] (X + Y) + 1[c == sym] X + 1[c == blank] Y
//                          g_dur[n] = w1 (-softmax_dur[n] (GX + GY) + gd[n])
//     The mix arguments travel as a trailing parameter pack that is empty for MIX = false, so those instantiations keep the
//     parameter list and the code they had.
#include "ftr_common.h"
#include "launch.h"

namespace ftr {
namespace {

constexpr int TDT_MAXN = 5;

// e[n]: the durations; first = index of the first positive one (0 or 1), so blank move j uses duration column first + j
struct TdtCols { int e[TDT_MAXN]; int N; int first; };

constexpr int TDT_PART_TDT = 1, TDT_PART_RNNT = 2;   // the `parts` bits of include/ftr_tdt_mix.h
// what the MIX builders take on top: the ordinary operands (band shaped [B,T,r], or px0 [B,S,T+1] / py0 [B,S+1,T])
struct TdtMixOut { float* px0; float* py0; int parts; };
// ... and the MIX gradient kernel: the ordinary occupancies in those shapes and their multiplier; `tdt` / `rnnt`: is the
// part there at all (a part with a zero multiplier is never read: its planes may be NULL)
struct TdtMixIn { const float* gx0; const float* gy0; Scale scale0; bool tdt, rnnt; };
template <typename A> __device__ __forceinline__ const A& tdt_mix_arg(const A& a) { return a; }

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
template <bool MIX, typename... M>
__global__ void tdt_to_lattice_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                                      const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                      const float* __restrict__ lse_tok, const float* __restrict__ lse_dur, int blank,
                                      const TdtCols tc, float sigma, double delay_penalty, float* __restrict__ px,
                                      float* __restrict__ py, int T, int S, int C, int r, const M... mix) {
  static_assert(sizeof...(M) == (MIX ? 1 : 0), "one TdtMixOut when MIX, else nothing");
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y, b = blockIdx.z;
  if (t > T) return;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const int W = C + tc.N, Ny = tc.N - tc.first;
  bool inband = false;
  bool tdt = true;                       // are the TDT planes written?
  if constexpr (MIX) tdt = (tdt_mix_arg(mix...).parts & TDT_PART_TDT) != 0;
  float tokx = -INFINITY, toky = -INFINITY;
  float tokx0 = -INFINITY, toky0 = -INFINITY;   // MIX: the same two columns without sigma
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
      const float l0 = lse_tok[row];
      const float l = l0 + sigma, ld = lse_dur[row];
      const float xb = x[blank];
      toky = xb - l;
      if (MIX) toky0 = xb - l0;
      if (s < S) {
        const float xs = x[min(max(symbols[(size_t)b * S + s], 0), C - 1)];
        tokx = xs - l;
        if (MIX) tokx0 = xs - l0;
      }
#pragma unroll
      for (int n = 0; n < TDT_MAXN; ++n)
        if (n < tc.N) dur[n] = x[C + n] - ld;
    }
    if (tdt) {
#pragma unroll
      for (int n = 0; n < TDT_MAXN; ++n) {
        const int jj = n - tc.first;
        if (n < tc.N && jj >= 0)
          py[(((size_t)b * Ny + jj) * (S + 1) + s) * T + t] = (inband && t + tc.e[n] <= te) ? toky + dur[n] : -INFINITY;
      }
    }
    if constexpr (MIX) {
      const TdtMixOut& mo = tdt_mix_arg(mix...);
      if (mo.parts & TDT_PART_RNNT) mo.py0[((size_t)b * (S + 1) + s) * T + t] = toky0;
    }
  }
  if (s < S) {
    double pen = 0.0;
    if (delay_penalty > 0.0) pen = (((double)te - 1.0) / 2.0 - (double)t) * delay_penalty;
    if (tdt) {
#pragma unroll
      for (int n = 0; n < TDT_MAXN; ++n) {
        if (n < tc.N) {
          float vx = (inband && t != te && t + tc.e[n] <= te) ? tokx + dur[n] : -INFINITY;
          if (delay_penalty > 0.0) vx += (float)pen;
          px[(((size_t)b * tc.N + n) * S + s) * (T + 1) + t] = vx;
        }
      }
    }
    if constexpr (MIX) {
      const TdtMixOut& mo = tdt_mix_arg(mix...);
      if (mo.parts & TDT_PART_RNNT) {    // band_to_lattice_kernel<float, false, false>: -inf at column t_end, the penalty by source frame
        float vx0 = t != te ? tokx0 : -INFINITY;
        if (delay_penalty > 0.0) vx0 += (float)pen;
        mo.px0[((size_t)b * S + s) * (T + 1) + t] = vx0;
      }
    }
  }
}

// one thread per band row (b,t,k) <-> lattice cell (s,t), s = (ranges[b,t,0] + k) mod (S+1) as the lattice kernel's roll
template <bool MIX, typename... M>
__global__ void tdt_to_band_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                                   const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                   const float* __restrict__ lse_tok, const float* __restrict__ lse_dur, int blank,
                                   const TdtCols tc, float sigma, double delay_penalty, float* __restrict__ pxb,
                                   float* __restrict__ pyb, size_t rows, int T, int S, int C, int r, const M... mix) {
  static_assert(sizeof...(M) == (MIX ? 1 : 0), "one TdtMixOut when MIX, else nothing");
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const size_t bt = row / r;
  const int k = (int)(row - bt * r);
  const int b = (int)(bt / T);
  const int t = (int)(bt - (size_t)b * T);
  int s = ranges[bt * r] + k;
  const bool sok0 = s >= 0 && s <= S;    // MIX: the ordinary band operands do not roll (band_gather_kernel of mi_band.hip)
  if (s > S) s -= S + 1;
  const bool sok = s >= 0 && s <= S;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const int W = C + tc.N, Ny = tc.N - tc.first;
  const float* x = logits + row * W;
  const float l0 = lse_tok[row];
  const float l = l0 + sigma, ld = lse_dur[row];
  const float xb = x[blank];
  const float toky = xb - l;
  float tokx = -INFINITY, xs = 0.0f;
  if (sok && s < S) {
    xs = x[min(max(symbols[(size_t)b * S + s], 0), C - 1)];
    tokx = xs - l;
  }
  double pen = 0.0;
  if (delay_penalty > 0.0) pen = (((double)te - 1.0) / 2.0 - (double)t) * delay_penalty;
  bool tdt = true;                       // are the TDT planes written?
  if constexpr (MIX) {
    const TdtMixOut& mo = tdt_mix_arg(mix...);
    tdt = (mo.parts & TDT_PART_TDT) != 0;
    if (mo.parts & TDT_PART_RNNT) {
      float vx0 = -INFINITY, vy0 = -INFINITY;
      if (sok0) {
        vy0 = xb - l0;
        if (s < S) {
          vx0 = t != te ? xs - l0 : -INFINITY;
          if (delay_penalty > 0.0) vx0 += (float)pen;
        }
      }
      mo.px0[row] = vx0;
      mo.py0[row] = vy0;
    }
  }
  if (!tdt) return;
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

template <bool VEC, bool BAND, bool MIX, typename... M>
__global__ void tdt_grad_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                                const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                const float* __restrict__ lse_tok, const float* __restrict__ lse_dur,
                                const float* __restrict__ gpx, const float* __restrict__ gpy, const Scale scale, int blank,
                                const TdtCols tc, float* __restrict__ glogits, size_t rows, int T, int S, int C, int r,
                                const M... mix) {
  static_assert(sizeof...(M) == (MIX ? 1 : 0), "one TdtMixIn when MIX, else nothing");
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
  const float sc = scale.at(b);          // MIX: w1 = (1 - omega) * upstream
  const bool sok = s >= 0 && s <= S;     // ranges are caller data: a row outside the lattice gets no gradient
  int sym = -1;
  if (sok && s < S) sym = min(max(symbols[(size_t)b * S + s], 0), C - 1);   // the column the forward read
  bool tdt = true;                       // MIX: are there TDT occupancies at all?  (w1 == 0: the planes are not read)
  if constexpr (MIX) tdt = tdt_mix_arg(mix...).tdt;
  float gd[TDT_MAXN];                    // what duration column n takes directly: gx_n + gy_j(n)
  float GX = 0.0f, GY = 0.0f;
#pragma unroll
  for (int n = 0; n < TDT_MAXN; ++n) {
    float gx = 0.0f, gy = 0.0f;
    if (tdt && n < tc.N && sok && t + tc.e[n] <= te) {     // the cells that are -inf whatever the row holds get no gradient
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
  const float tot = GX + GY;             // what the duration head takes
  float X = GX, Y = GY;                  // what the token head takes at the symbol / at blank
  if constexpr (MIX) {
    const TdtMixIn& mi = tdt_mix_arg(mix...);
    if (mi.rnnt) {                       // the ordinary occupancies of the row's cell, w2 = omega * upstream
      const float w2 = mi.scale0.at(b);
      if (BAND) {                        // [B,T,r], no roll: the masks of band_grad_banded_kernel (mi_band.hip), regular type
        if (s0 + k <= S && sok) {
          if (s < S && t != te) X += mi.gx0[row] * w2;
          Y += mi.gy0[row] * w2;
        }
      } else if (sok) {                  // gx0 [B,S,T+1] / gy0 [B,S+1,T]: the masks of band_grad_kernel<MOD = false>
        if (s < S && t != te) X += mi.gx0[((size_t)b * S + s) * T1 + t] * w2;
        Y += mi.gy0[((size_t)b * (S + 1) + s) * T + t] * w2;
      }
    }
  }
  const float tott = MIX ? X + Y : tot;
  const float l = lse_tok[row], ld = lse_dur[row];
  const float* x = logits + row * W;
  float* g = glogits + row * W;
  auto column = [&](int c, float v) -> float {
    if (c < C) {
      float val = -tott * __expf(v - l);
      if (c == sym) val += X;
      if (c == blank) val += Y;
      return val;
    }
    if (MIX && !tdt) return 0.0f;        // omega == 1: exact zeros, whatever the duration logits hold
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

// The builders' two launches.  band: band-shaped px / py (tdt_to_band_kernel), else the lattices; mo: the MIX instantiation
// with these ordinary planes, nullptr: the kernel as it is without them.
int tdt_fwd_launch(bool band, const char* what, const float* logits, const int32_t* symbols, const int32_t* ranges,
                   const int32_t* boundary, int blank, const int32_t* durations, int N, double sigma, double delay_penalty,
                   float* lse_tok, float* lse_dur, float* px, float* py, const TdtMixOut* mo, int B, int T, int S, int C, int r,
                   hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit(what, rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  dispatch(((C + N) & 3) == 0, [&](auto vec) {
    hipLaunchKernelGGL((tdt_lse_kernel<decltype(vec)::value>), dim3(blocks), dim3(64 * wpb), 0, st, logits, lse_tok, lse_dur, rows, C, N);
  });
  int rc = check_launch("tdt_lse");
  if (rc != FTR_OK) return rc;
  const TdtCols tc = tdt_cols(durations, N);
  if (band) {
    const dim3 grid((unsigned)((rows + 255) / 256)), block(256);
    if (mo)
      hipLaunchKernelGGL((tdt_to_band_kernel<true, TdtMixOut>), grid, block, 0, st, logits, symbols, ranges, boundary, lse_tok, lse_dur,
                         blank, tc, (float)sigma, delay_penalty, px, py, rows, T, S, C, r, *mo);
    else
      hipLaunchKernelGGL((tdt_to_band_kernel<false>), grid, block, 0, st, logits, symbols, ranges, boundary, lse_tok, lse_dur, blank,
                         tc, (float)sigma, delay_penalty, px, py, rows, T, S, C, r);
    return check_launch("tdt_to_band");
  }
  const int threads = 256;
  const dim3 grid((T + 1 + threads - 1) / threads, S + 1, B);
  if (mo)
    hipLaunchKernelGGL((tdt_to_lattice_kernel<true, TdtMixOut>), grid, dim3(threads), 0, st, logits, symbols, ranges, boundary, lse_tok,
                       lse_dur, blank, tc, (float)sigma, delay_penalty, px, py, T, S, C, r, *mo);
  else
    hipLaunchKernelGGL((tdt_to_lattice_kernel<false>), grid, dim3(threads), 0, st, logits, symbols, ranges, boundary, lse_tok, lse_dur,
                       blank, tc, (float)sigma, delay_penalty, px, py, T, S, C, r);
  return check_launch("tdt_to_lattice");
}

// The gradient launch.  band: band-shaped occupancies; mi: the MIX instantiation, nullptr: the kernel as it is without it.
int tdt_bwd_launch(bool band, const char* what, const float* logits, const int32_t* symbols, const int32_t* ranges,
                   const int32_t* boundary, int blank, const int32_t* durations, int N, const float* lse_tok, const float* lse_dur,
                   const float* gpx, const float* gpy, Scale scale, const TdtMixIn* mi, float* glogits, int B, int T, int S, int C,
                   int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit(what, rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const dim3 grid((unsigned)((rows + wpb - 1) / wpb)), block(64 * wpb);
  const TdtCols tc = tdt_cols(durations, N);
  dispatch(((C + N) & 3) == 0, [&](auto vec) {
    dispatch(band, [&](auto bnd) {
      constexpr bool V = decltype(vec)::value, BD = decltype(bnd)::value;
      if (mi)
        hipLaunchKernelGGL((tdt_grad_kernel<V, BD, true, TdtMixIn>), grid, block, 0, st, logits, symbols, ranges, boundary, lse_tok,
                           lse_dur, gpx, gpy, scale, blank, tc, glogits, rows, T, S, C, r, *mi);
      else
        hipLaunchKernelGGL((tdt_grad_kernel<V, BD, false>), grid, block, 0, st, logits, symbols, ranges, boundary, lse_tok, lse_dur,
                           gpx, gpy, scale, blank, tc, glogits, rows, T, S, C, r);
    });
  });
  return check_launch(band ? "tdt_band_grad" : "tdt_grad");
}
}  // namespace

int tdt_logprobs_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                     const int32_t* durations, int N, double sigma, double delay_penalty, float* lse_tok, float* lse_dur,
                     float* px, float* py, int B, int T, int S, int C, int r, hipStream_t st) {
  return tdt_fwd_launch(false, "tdt_logprobs_fwd", logits, symbols, ranges, boundary, blank, durations, N, sigma, delay_penalty,
                        lse_tok, lse_dur, px, py, nullptr, B, T, S, C, r, st);
}

int tdt_logprobs_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                     const int32_t* durations, int N, const float* lse_tok, const float* lse_dur, const float* gpx,
                     const float* gpy, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st) {
  return tdt_bwd_launch(false, "tdt_logprobs_bwd", logits, symbols, ranges, boundary, blank, durations, N, lse_tok, lse_dur, gpx,
                        gpy, scale, nullptr, glogits, B, T, S, C, r, st);
}

int tdt_band_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                 const int32_t* durations, int N, double sigma, double delay_penalty, float* lse_tok, float* lse_dur,
                 float* pxb, float* pyb, int B, int T, int S, int C, int r, hipStream_t st) {
  return tdt_fwd_launch(true, "tdt_pruned_band_fwd", logits, symbols, ranges, boundary, blank, durations, N, sigma, delay_penalty,
                        lse_tok, lse_dur, pxb, pyb, nullptr, B, T, S, C, r, st);
}

int tdt_band_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                 const int32_t* durations, int N, const float* lse_tok, const float* lse_dur, const float* gxb,
                 const float* gyb, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st) {
  return tdt_bwd_launch(true, "tdt_pruned_band_bwd", logits, symbols, ranges, boundary, blank, durations, N, lse_tok, lse_dur, gxb,
                        gyb, scale, nullptr, glogits, B, T, S, C, r, st);
}

// include/ftr_tdt_mix.h.  band: the band-shaped planes, else the lattices; parts: TDT_PART_* bits, which planes are written
int tdt_mix_fwd(int band, const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                const int32_t* durations, int N, double sigma, int parts, double delay_penalty, float* lse_tok, float* lse_dur,
                float* px, float* py, float* px0, float* py0, int B, int T, int S, int C, int r, hipStream_t st) {
  const TdtMixOut mo{px0, py0, parts};
  return tdt_fwd_launch(band != 0, band ? "tdt_mix_pruned_band_fwd" : "tdt_mix_pruned_logprobs_fwd", logits, symbols, ranges, boundary,
                        blank, durations, N, sigma, delay_penalty, lse_tok, lse_dur, px, py, &mo, B, T, S, C, r, st);
}

// scale: w1 = (1 - omega) * upstream, scale0: w2 = omega * upstream; a multiplier of zero: that part's occupancies are not read
int tdt_mix_bwd(int band, const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                const int32_t* durations, int N, const float* lse_tok, const float* lse_dur, const float* gpx, const float* gpy,
                const float* gpx0, const float* gpy0, Scale scale, Scale scale0, float* glogits, int B, int T, int S, int C, int r,
                hipStream_t st) {
  const TdtMixIn mi{gpx0, gpy0, scale0, scale.mul != 0.0f, scale0.mul != 0.0f};
  return tdt_bwd_launch(band != 0, band ? "tdt_mix_pruned_band_bwd" : "tdt_mix_pruned_logprobs_bwd", logits, symbols, ranges, boundary,
                        blank, durations, N, lse_tok, lse_dur, gpx, gpy, scale, &mi, glogits, B, T, S, C, r, st);
}

}  // namespace ftr
