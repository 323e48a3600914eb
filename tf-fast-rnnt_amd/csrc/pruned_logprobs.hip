// csrc/pruned_logprobs.hip -- pruned joiner log-probs, forward and backward, gfx950.
// Replaces get_rnnt_logprobs_pruned (+ _roll_by_shifts, fix_for_boundary and the delay-penalty block)
// of /root/reference/tf_fast_rnnt/python/tf_fast_rnnt/rnnt_loss.py:853-1020, 814-851, 28-61, 1097-1114
// and what TensorFlow autodiff replays for them in the backward pass.
//   lse_rows_kernel        :942  reduce_logsumexp over C, one wave per (b,t,k) row, 16-byte loads
//   band_to_lattice_kernel :943-1016 gathers + pad + roll + transpose + fix_for_boundary, one thread per
//                          lattice cell, coalesced along t: px/py are written exactly once, complete
//   band_grad_kernel       gradient w.r.t. logits: -(gx+gy) softmax + gx 1[sym] + gy 1[blank]
// HAT (hybrid autoregressive transducer, MI355X addition): each kernel has a `bool HAT` twin that normalises the row
// differently -- lse holds Z = logsumexp over the non-blank columns, py = log sigmoid(x[blank]),
// px = x[sym] - Z - softplus(x[blank]) (-inf when sym == blank); the HAT = false instantiations are the ordinary kernels.
// 16-bit logits: the four kernels above also take an element type E (float, bf16_t, fp16_t of ftr_common.h).  A 16-bit
// row is read four elements (8 bytes) per lane where C % 4 == 0 and the tensor's base is 8-byte aligned, element by element
// otherwise; values are up-converted on load, lse / px / py and all arithmetic stay float32, and the gradient row is rounded
// once (nearest-even) when it is stored in E.  The float instantiations are the kernels as they were.  The multi-blank
// kernels below are float only.
#include "ftr_common.h"
#include "launch.h"

namespace ftr {
namespace {

__device__ __forceinline__ float wave_max(float v) { return wave_max_dpp(v); }
__device__ __forceinline__ float wave_sum(float v) { return wave_sum_dpp(v); }

// logsumexp of each row, the row held in registers (C % 4 == 0, C <= 256 * NQ): one wave per row, one 16-byte load per lane
// and quad, all issued before the first is used, a single pass over the data, one short-lived wave per row and as many waves
// as the chip holds.  (Rounds 1 - 2 ran this as 2048 persistent blocks, two rows per pass, the next pass's loads in flight
// while one is reduced: 73 us at c3 = 4.4 TB/s; scripts/probes/stream_probe.hip measures the plain form below at 55 us =
// 5.8 TB/s on the same tensor -- a flat read reaches 6.7 -- and 205 against 250 us at c4.  The memory system likes many short
// waves better than few clever ones.)
// HAT: the blank column is masked to -inf before the max and the sum (lse = Z, the non-blank normaliser).
// E: the element type of `logits` (float, bf16_t, fp16_t): a 16-bit row is one 8-byte load per lane and quad instead of a
// 16-byte one, up-converted into the same float registers, so the same NQ keeps the same C <= 2048 register-resident.
template <typename E, int NQ, bool HAT>
__global__ __launch_bounds__(256) void lse_rows_reg_kernel(const E* __restrict__ logits, float* __restrict__ lse,
                                                           size_t rows, int C, int blank) {
  const int lane = threadIdx.x & 63;
  // LAST ROWS FIRST.  The joiner has just written `logits` front to back, 320 MB at c3 against 256 MB of memory-side cache:
  // what is still in the cache is the tail.  Walking front to back misses the cache on the head AND pushes the dirty tail out
  // before it is read; walking back to front reads the tail from the cache: 75 -> 53 us inside the c3 step (the kernel alone,
  // on a tensor at rest, takes 55 us either way).
  const size_t rowi = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (rowi >= rows) return;
  const size_t row = rows - 1 - rowi;
  const int n4 = C >> 2;
  const f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const E* x = logits + row * C;
  f4 v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    v[q] = (i < n4) ? load4(x, i) : ninf;
    if (HAT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[q][e] = (4 * i + e == blank) ? -INFINITY : v[q][e];
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) m = fmaxf(fmaxf(m, fmaxf(v[q][0], v[q][1])), fmaxf(v[q][2], v[q][3]));
  m = wave_max(m);
  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (lane + 64 * q < n4)   // same per-lane order as the two-pass kernel
      sum += __expf(v[q][0] - m) + __expf(v[q][1] - m) + __expf(v[q][2] - m) + __expf(v[q][3] - m);
  }
  sum = wave_sum(sum);
  if (lane == 0) lse[row] = m + __logf(sum);
}

// logsumexp of each row of length C; rows = B*T*r.  One wave per row (any C).
template <typename E, bool VEC, bool HAT>
__global__ void lse_rows_kernel(const E* __restrict__ logits, float* __restrict__ lse, size_t rows, int C, int blank) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const E* x = logits + row * C;
  float m = -INFINITY;
  if (VEC) {
    const int n4 = C >> 2;
    for (int i = lane; i < n4; i += 64) {
      f4 v = load4(x, i);
      if (HAT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (4 * i + e == blank) ? -INFINITY : v[e];
      }
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    m = wave_max(m);
    float s = 0.0f;
    for (int i = lane; i < n4; i += 64) {  // second pass hits L1/L2: a row is 2-4 KB
      f4 v = load4(x, i);
      if (HAT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (4 * i + e == blank) ? -INFINITY : v[e];
      }
      s += __expf(v[0] - m) + __expf(v[1] - m) + __expf(v[2] - m) + __expf(v[3] - m);
    }
    s = wave_sum(s);
    if (lane == 0) lse[row] = m + __logf(s);
  } else {
    for (int i = lane; i < C; i += 64) m = fmaxf(m, (HAT && i == blank) ? -INFINITY : elem_to_float(x[i]));
    m = wave_max(m);
    float s = 0.0f;
    for (int i = lane; i < C; i += 64) s += __expf(((HAT && i == blank) ? -INFINITY : elem_to_float(x[i])) - m);
    s = wave_sum(s);
    if (lane == 0) lse[row] = m + __logf(s);
  }
}

// grid: (ceil((T+1)/256), S+1, B); thread <-> (b, s, t).  Writes py[b,s,t] (t < T) and px[b,s,t] (s < S, t < T1).
template <typename E, bool MOD, bool HAT>
__global__ void band_to_lattice_kernel(const E* __restrict__ logits, const int32_t* __restrict__ symbols,
                                       const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                       const float* __restrict__ lse, int blank, double delay_penalty,
                                       float* __restrict__ px, float* __restrict__ py, int T, int S, int C, int r) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y, b = blockIdx.z;
  const int T1 = MOD ? T : T + 1;
  if (t >= T1 && t >= T) return;
  const int te = boundary ? boundary[4 * b + 3] : T;
  float vx = -INFINITY, vy = -INFINITY;
  if (t < T) {
    const size_t bt = (size_t)b * T + t;
    const int s0 = ranges[bt * r];
    int k = s - s0;                     // _roll_by_shifts: out[s] = padded[(s - s0) mod (S+1)]  (:849)
    if (k < 0) k += S + 1;
    if (k < r) {
      const size_t row = bt * r + k;
      const float l = lse[row];
      if (HAT) {
        const float xb = elem_to_float(logits[row * C + blank]);
        int c = blank;
        if (s < S) c = min(max(symbols[(size_t)b * S + s], 0), C - 1);
        float hx, hy;
        hat_logprobs(xb, elem_to_float(logits[row * C + c]), l, c == blank, &hx, &hy);
        vy = hy;
        if (s < S) vx = hx;
      } else {
        vy = elem_to_float(logits[row * C + blank]) - l;                       // :995-996
        if (s < S) vx = elem_to_float(logits[row * C + min(max(symbols[(size_t)b * S + s], 0), C - 1)]) - l;   // :961-965 (symbol kept in bounds)
      }
    }
  }
  if (t < T) py[((size_t)b * (S + 1) + s) * T + t] = vy;
  if (s < S && t < T1) {
    if (!MOD && t == te) vx = -INFINITY;                      // fix_for_boundary (:1015-1016), px[:,:,T] (:984-993)
    if (delay_penalty > 0.0) {                                // :1097-1114, float64 then cast
      const double offset = ((double)te - 1.0) / 2.0;
      vx += (float)((offset - (double)t) * delay_penalty);
    }
    px[((size_t)b * S + s) * T1 + t] = vx;
  }
}

// one wave per (b,t,k) row of glogits.
// HAT: g[c] = gx (1[c == sym] - exp(x[c] - Z)) for c != blank, g[blank] = gy sigmoid(-x[blank]) - gx sigmoid(x[blank]).
// E: the element type of logits and glogits; the row is computed in float32 and rounded once when it is stored.
template <typename E, bool MOD, bool VEC, bool HAT>
__global__ void band_grad_kernel(const E* __restrict__ logits, const int32_t* __restrict__ symbols,
                                 const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                 const float* __restrict__ lse, const float* __restrict__ gpx,
                                 const float* __restrict__ gpy, const Scale scale, int blank,
                                 E* __restrict__ glogits, size_t rows, int T, int S, int C, int r) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int T1 = MOD ? T : T + 1;
  const size_t bt = row / r;
  const int k = (int)(row - bt * r);
  const int b = (int)(bt / T);
  const int t = (int)(bt - (size_t)b * T);
  const int s0 = ranges[bt * r];
  int s = s0 + k;                        // inverse of the roll: band slot k <-> lattice row (s0 + k) mod (S+1)
  if (s > S) s -= S + 1;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const float sc = scale.at(b);
  float gx = 0.0f;
  int sym = blank;
  const bool sok = s >= 0 && s <= S;     // ranges are caller data: a row outside the lattice gets no gradient
  if (sok && s < S) {
    sym = symbols[(size_t)b * S + s];
    if (MOD || t != te) gx = gpx[((size_t)b * S + s) * T1 + t] * sc;   // overwritten cells get no gradient
  }
  const float gy = sok ? gpy[((size_t)b * (S + 1) + s) * T + t] * sc : 0.0f;
  float tot = gx + gy;
  const float l = lse[row];
  if (HAT) {   // after the row's loads are issued, so none of them waits for the symbol
    sym = min(max(sym, 0), C - 1);       // the column the forward read
    if (sym == blank) gx = 0.0f;         // px is -inf there
    tot = gx;
  }
  const E* x = logits + row * C;
  E* g = glogits + row * C;
  if (VEC) {
    const int n4 = C >> 2;
    for (int i = lane; i < n4; i += 64) {
      const f4 v = load4(x, i);
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * i + e;
        float val = -tot * __expf(v[e] - l);
        if (c == sym) val += gx;
        if (c == blank) {
          if (HAT) {    // sigmoid(x[blank]) once per row, by the lane that holds the blank column
            float sp, sn;
            hat_sigmoids(v[e], &sp, &sn);
            val = gy * sn - gx * sp;
          } else {
            val += gy;
          }
        }
        o[e] = val;
      }
      store4(g, i, o);
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      const float xc = elem_to_float(x[c]);
      float val = -tot * __expf(xc - l);
      if (c == sym) val += gx;
      if (c == blank) {
        if (HAT) {
          float sp, sn;
          hat_sigmoids(xc, &sp, &sn);
          val = gy * sn - gx * sp;
        } else {
          val += gy;
        }
      }
      g[c] = elem_from_float<E>(val);
    }
  }
}

// loss tail (rnnt_loss.py:333,544-546,1124-1126,1487-1489): out = -ans (reduction 0), -mean (1) or -sum (2) over the
// batch, one block, fixed summation tree (deterministic).  sign = -1 is that tail; sign = +1 reduces per-utterance values
// that already are a loss (pruned_kd.hip).  sign * v with sign = -1 is -v, bit for bit.
__global__ __launch_bounds__(256) void negated_reduce_kernel(const float* __restrict__ ans, int B, int reduction,
                                                             float* __restrict__ out, float sign) {
  __shared__ float red[4];
  if (reduction == 0) {
    for (int b = threadIdx.x; b < B; b += 256) out[b] = sign * ans[b];
    return;
  }
  float s = 0.0f;
  for (int b = threadIdx.x; b < B; b += 256) s += ans[b];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = (red[0] + red[1]) + (red[2] + red[3]);
    out[0] = sign * ((reduction == 1) ? t / (float)B : t);
  }
}
}  // namespace

int negated_reduce(const float* ans, int B, int reduction, float* out, hipStream_t st, float sign) {
  hipLaunchKernelGGL(negated_reduce_kernel, dim3(1), dim3(256), 0, st, ans, B, reduction, out, sign);
  return check_launch("negated_reduce");
}

// logsumexp over the last axis of [rows, C] (rnnt_loss.py:942): picks the register-resident kernel where it fits
// (hat: over the non-blank columns only, the normaliser Z of the HAT factorisation)
namespace {
template <typename E>
int lse_rows_of(const E* logits, float* lse, size_t rows, int C, int blank, int hat, hipStream_t st) {
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("lse_rows", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  dispatch(hat != 0, [&](auto h) {
    constexpr bool HAT = decltype(h)::value;
    const bool vec4 = rows_vec4<E>(C, logits);
    if (vec4 && C <= 2048)   // the row fits the registers of a wave: 1, 2, 4 or 8 quads of elements per lane
      dispatch_among<1, 2, 4, 8>(C <= 256 ? 1 : C <= 512 ? 2 : C <= 1024 ? 4 : 8, [&](auto n) {
        hipLaunchKernelGGL((lse_rows_reg_kernel<E, decltype(n)::value, HAT>), dim3(blocks), dim3(64 * wpb), 0, st, logits, lse, rows, C, blank);
      });
    else
      dispatch(vec4, [&](auto vec) {
        hipLaunchKernelGGL((lse_rows_kernel<E, decltype(vec)::value, HAT>), dim3(blocks), dim3(64 * wpb), 0, st, logits, lse, rows, C, blank);
      });
  });
  return check_launch("lse_rows");
}
}  // namespace

int lse_rows(const float* logits, float* lse, size_t rows, int C, int blank, int hat, hipStream_t st) {
  return lse_rows_of(logits, lse, rows, C, blank, hat, st);
}
int lse_rows_dtype(const void* logits, int dtype, float* lse, size_t rows, int C, int blank, int hat, hipStream_t st) {
  return dispatch_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    return lse_rows_of(static_cast<const E*>(logits), lse, rows, C, blank, hat, st);
  });
}

int pruned_logprobs_fwd(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges,
                        const int32_t* boundary, int blank, double delay_penalty, float* lse, float* px,
                        float* py, int B, int T, int S, int C, int r, int modified, int hat, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("pruned_logprobs_fwd", rows); if (rc32 != FTR_OK) return rc32; }
  int rc = lse_rows_dtype(logits, dtype, lse, rows, C, blank, hat, st);
  if (rc != FTR_OK) return rc;
  const int threads = 256;
  const dim3 grid((T + 1 + threads - 1) / threads, S + 1, B);
  dispatch_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    dispatch(modified != 0, [&](auto mod) {
      dispatch(hat != 0, [&](auto h) {
        hipLaunchKernelGGL((band_to_lattice_kernel<E, decltype(mod)::value, decltype(h)::value>), grid, dim3(threads), 0, st,
                           static_cast<const E*>(logits), symbols, ranges, boundary, lse, blank, delay_penalty, px, py, T, S, C, r);
      });
    });
  });
  return check_launch("band_to_lattice");
}

int pruned_logprobs_bwd(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges,
                        const int32_t* boundary, int blank, const float* lse, const float* gpx,
                        const float* gpy, Scale scale, void* glogits, int B, int T, int S, int C,
                        int r, int modified, int hat, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("pruned_logprobs_bwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  dispatch_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    dispatch(modified != 0, [&](auto mod) {
      dispatch(rows_vec4<E>(C, logits, glogits), [&](auto vec) {
        dispatch(hat != 0, [&](auto h) {
          hipLaunchKernelGGL((band_grad_kernel<E, decltype(mod)::value, decltype(vec)::value, decltype(h)::value>), dim3(blocks), dim3(64 * wpb), 0, st,
                             static_cast<const E*>(logits), symbols, ranges, boundary, lse, gpx, gpy, scale, blank, static_cast<E*>(glogits), rows, T, S, C, r);
        });
      });
    });
  });
  return check_launch("band_grad");
}

// ---- multi-blank twins (MI355X addition, regular type only): D blank columns per row, blank j advancing d[j] frames.
// The row is normalised by the ordinary softmax over all C columns (lse_rows, unchanged); `sigma` is subtracted from
// every log-probability.  py has D planes [B,D,S+1,T]; py[b,j,s,t] = -inf where t + d[j] > t_end.  A symbol that is a
// big blank gets px = -inf and no gradient.  Kernels of their own, so the ordinary instantiations above stay as they are.
// The band-shaped twins (include/ftr_band_multiblank.h; the operands and occupancies of mi_band_tdt.hip's multi-blank
// entry, px_band [B,T,r] and py_band [B,D,T,r]): mb_to_band_kernel writes what mb_to_lattice_kernel puts at lattice cell
// (ranges[b,t,0] + k, t), by the same arithmetic, one thread per band row and no lattice write; mb_grad_kernel<., true>
// is the same gradient kernel reading gx_band / gy_band at the row itself.
namespace {

struct MbCols { int id[8]; int d[8]; int D; };   // id[0] = the standard blank, d[0] = 1

__device__ __forceinline__ bool mb_is_big_blank(const MbCols& mc, int c) {
  bool hit = false;
  for (int j = 1; j < mc.D; ++j) hit |= (c == mc.id[j]);
  return hit;
}

// grid: (ceil((T+1)/256), S+1, B); thread <-> (b, s, t).  Writes py[b,:,s,t] (t < T) and px[b,s,t] (s < S, t <= T).
__global__ void mb_to_lattice_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                                     const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                     const float* __restrict__ lse, const MbCols mc, float sigma, double delay_penalty,
                                     float* __restrict__ px, float* __restrict__ py, int T, int S, int C, int r) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y, b = blockIdx.z;
  if (t > T) return;
  const int te = boundary ? boundary[4 * b + 3] : T;
  float vx = -INFINITY;
  bool inband = false;
  size_t row = 0;
  float l = 0.0f;
  if (t < T) {
    const size_t bt = (size_t)b * T + t;
    const int s0 = ranges[bt * r];
    int k = s - s0;
    if (k < 0) k += S + 1;
    if (k < r) {
      inband = true;
      row = bt * r + k;
      l = lse[row] + sigma;
      if (s < S) {
        const int c = min(max(symbols[(size_t)b * S + s], 0), C - 1);
        if (!mb_is_big_blank(mc, c)) vx = logits[row * C + c] - l;
      }
    }
    for (int j = 0; j < mc.D; ++j) {
      float vy = -INFINITY;
      if (inband && t + mc.d[j] <= te) vy = logits[row * C + mc.id[j]] - l;
      py[(((size_t)b * mc.D + j) * (S + 1) + s) * T + t] = vy;
    }
  }
  if (s < S) {
    if (t == te) vx = -INFINITY;
    if (delay_penalty > 0.0) {
      const double offset = ((double)te - 1.0) / 2.0;
      vx += (float)((offset - (double)t) * delay_penalty);
    }
    px[((size_t)b * S + s) * (T + 1) + t] = vx;
  }
}

// one thread per band row (b,t,k) <-> lattice cell (s,t), s = (ranges[b,t,0] + k) mod (S+1) as the lattice kernel's roll.
// Every element of px_band [B,T,r] and py_band [B,D,T,r] is written.
__global__ void mb_to_band_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                                  const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                  const float* __restrict__ lse, const MbCols mc, float sigma, double delay_penalty,
                                  float* __restrict__ pxb, float* __restrict__ pyb, size_t rows, int T, int S, int C, int r) {
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
  const float l = lse[row] + sigma;
  float vx = -INFINITY;
  if (sok && s < S) {
    const int c = min(max(symbols[(size_t)b * S + s], 0), C - 1);
    if (!mb_is_big_blank(mc, c)) vx = logits[row * C + c] - l;
  }
  if (t == te) vx = -INFINITY;
  if (delay_penalty > 0.0) {
    const double offset = ((double)te - 1.0) / 2.0;
    vx += (float)((offset - (double)t) * delay_penalty);
  }
  pxb[row] = vx;
  for (int j = 0; j < mc.D; ++j) {
    float vy = -INFINITY;
    if (sok && t + mc.d[j] <= te) vy = logits[row * C + mc.id[j]] - l;
    pyb[(((size_t)b * mc.D + j) * T + t) * r + k] = vy;
  }
}

// one wave per (b,t,k) row of glogits, as band_grad_kernel: g[c] = -softmax(x)[c] (gx + sum_j gy_j) + 1[c == sym] gx
// + sum_j 1[c == id_j] gy_j; each blank column takes its term in the lane that holds the column.  BAND: gpx / gpy are
// the band-shaped occupancies [B,T,r] / [B,D,T,r], the row's own element of each plane, else the full-size lattices.
template <bool VEC, bool BAND>
__global__ void mb_grad_kernel(const float* __restrict__ logits, const int32_t* __restrict__ symbols,
                               const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                               const float* __restrict__ lse, const float* __restrict__ gpx,
                               const float* __restrict__ gpy, const Scale scale, const MbCols mc,
                               float* __restrict__ glogits, size_t rows, int T, int S, int C, int r) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int T1 = T + 1;
  const size_t bt = row / r;
  const int k = (int)(row - bt * r);
  const int b = (int)(bt / T);
  const int t = (int)(bt - (size_t)b * T);
  const int s0 = ranges[bt * r];
  int s = s0 + k;
  if (s > S) s -= S + 1;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const float sc = scale.at(b);
  float gx = 0.0f;
  int sym = -1;
  const bool sok = s >= 0 && s <= S;
  if (sok && s < S) {
    sym = min(max(symbols[(size_t)b * S + s], 0), C - 1);   // the column the forward read
    if (t != te && !mb_is_big_blank(mc, sym)) gx = gpx[BAND ? row : ((size_t)b * S + s) * T1 + t] * sc;
  }
  float gy[8];
  float tot = gx;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    gy[j] = 0.0f;
    if (j < mc.D && sok && t + mc.d[j] <= te)
      gy[j] = gpy[BAND ? (((size_t)b * mc.D + j) * T + t) * r + k : (((size_t)b * mc.D + j) * (S + 1) + s) * T + t] * sc;
    tot += gy[j];
  }
  const float l = lse[row];
  const float* x = logits + row * C;
  float* g = glogits + row * C;
  if (VEC) {
    const f4u* x4 = reinterpret_cast<const f4u*>(x);
    f4u* g4 = reinterpret_cast<f4u*>(g);
    const int n4 = C >> 2;
    for (int i = lane; i < n4; i += 64) {
      const f4 v = x4[i];
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = -tot * __expf(v[e] - l);
        if (4 * i + e == sym) o[e] += gx;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < mc.D && (mc.id[j] >> 2) == i) {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += ((mc.id[j] & 3) == e) ? gy[j] : 0.0f;
        }
      }
      g4[i] = o;
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      float val = -tot * __expf(x[c] - l);
      if (c == sym) val += gx;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < mc.D && c == mc.id[j]) val += gy[j];
      g[c] = val;
    }
  }
}

MbCols mb_cols(int blank, const int32_t* big_ids, const int32_t* durations, int D) {
  MbCols mc;
  for (int j = 0; j < 8; ++j) {
    mc.id[j] = j == 0 ? blank : (j < D ? big_ids[j - 1] : -1);
    mc.d[j] = j < D ? durations[j] : 1;
  }
  mc.D = D;
  return mc;
}
}  // namespace

int multiblank_logprobs_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                            int blank, const int32_t* big_ids, const int32_t* durations, int D, double sigma,
                            double delay_penalty, float* lse, float* px, float* py, int B, int T, int S, int C, int r,
                            hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("multiblank_logprobs_fwd", rows); if (rc32 != FTR_OK) return rc32; }
  int rc = lse_rows(logits, lse, rows, C, blank, 0, st);
  if (rc != FTR_OK) return rc;
  const int threads = 256;
  const dim3 grid((T + 1 + threads - 1) / threads, S + 1, B);
  hipLaunchKernelGGL(mb_to_lattice_kernel, grid, dim3(threads), 0, st, logits, symbols, ranges, boundary, lse,
                     mb_cols(blank, big_ids, durations, D), (float)sigma, delay_penalty, px, py, T, S, C, r);
  return check_launch("multiblank_to_lattice");
}

int multiblank_logprobs_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                            int blank, const int32_t* big_ids, const int32_t* durations, int D, const float* lse,
                            const float* gpx, const float* gpy, Scale scale, float* glogits, int B, int T, int S, int C,
                            int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("multiblank_logprobs_bwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  const MbCols mc = mb_cols(blank, big_ids, durations, D);
  dispatch((C & 3) == 0, [&](auto vec) {
    hipLaunchKernelGGL((mb_grad_kernel<decltype(vec)::value, false>), dim3(blocks), dim3(64 * wpb), 0, st, logits, symbols, ranges, boundary, lse,
                       gpx, gpy, scale, mc, glogits, rows, T, S, C, r);
  });
  return check_launch("multiblank_grad");
}

int multiblank_band_fwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                        const int32_t* big_ids, const int32_t* durations, int D, double sigma, double delay_penalty, float* lse,
                        float* pxb, float* pyb, int B, int T, int S, int C, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("multiblank_pruned_band_fwd", rows); if (rc32 != FTR_OK) return rc32; }
  int rc = lse_rows(logits, lse, rows, C, blank, 0, st);
  if (rc != FTR_OK) return rc;
  hipLaunchKernelGGL(mb_to_band_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, logits, symbols, ranges, boundary,
                     lse, mb_cols(blank, big_ids, durations, D), (float)sigma, delay_penalty, pxb, pyb, rows, T, S, C, r);
  return check_launch("multiblank_to_band");
}

int multiblank_band_bwd(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank,
                        const int32_t* big_ids, const int32_t* durations, int D, const float* lse, const float* gxb,
                        const float* gyb, Scale scale, float* glogits, int B, int T, int S, int C, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("multiblank_pruned_band_bwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  const MbCols mc = mb_cols(blank, big_ids, durations, D);
  dispatch((C & 3) == 0, [&](auto vec) {
    hipLaunchKernelGGL((mb_grad_kernel<decltype(vec)::value, true>), dim3(blocks), dim3(64 * wpb), 0, st, logits, symbols, ranges, boundary, lse,
                       gxb, gyb, scale, mc, glogits, rows, T, S, C, r);
  });
  return check_launch("multiblank_band_grad");
}

}  // namespace ftr
