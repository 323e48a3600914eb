// csrc/pruned_constrained.hip -- the constrained transducer type on the pruned band (include/ftr_band_constrained.h), gfx950.
//
// rnnt_type = "constrained" is the modified type with a blank forced behind every symbol: px_c[s,t] = px'[s,t] + py[s+1,t].
// On a band, lattice row s+1 of frame t is band slot k+1 of the SAME frame, so the operand needs nothing but a neighbour
// exchange among the r rows of one frame:
//
//   constr_frame_kernel   one workgroup per frame (b,t), r waves, wave k <-> band row k.  Each wave reads its joiner row once
//                         (into registers while C % 4 == 0 and C <= 2048, as lse_rows_reg_kernel of pruned_logprobs.hip
//                         does: 16-byte loads for float32, 8-byte loads for 16 bits), forms the row's normaliser and its two
//                         log-probs tok_x = log p(sym_s), tok_y = log p(blank), publishes tok_y and the row's validity in
//                         LDS (two words per row), crosses ONE barrier, and wave k writes lse, py_band = tok_y(k) and
//                         px_band = tok_x(k) + tok_y(k+1) (+ the delay penalty, after the sum).  One launch and one read of
//                         the logits where the ordinary band builder takes two of each (lse_rows + band_gather).
//   constr_grad_kernel    one wave per row (b,t,k), last rows first (see band_grad_banded_kernel, mi_band.hip): the symbol
//                         column takes X = gx_band[k], the blank column Y = gy_band[k] + gx_band[k-1] -- the forced blank of
//                         the symbol move that starts one row below lands in THIS row -- and the softmax term -(X + Y).
//
// -inf rules (what the lattice composition puts at cell (s,t), s = ranges[b,t,0] + k): py_band is -inf for s outside 0..S;
// px_band is -inf for s outside 0..S-1, for k + 1 == r (row s+1 is outside the band, its py is -inf on the lattice) and, HAT,
// for a symbol that is the blank.  Frames outside [t_begin, t_end) are not read: lse = 0, px_band = py_band = -inf, a zero
// gradient row (the band recursion never looks at them and gives them zero occupancies).
// HAT and the element type E of logits / glogits: as in pruned_logprobs.hip (lse holds Z, the helpers of ftr_common.h; 16-bit
// values are up-converted on load, all arithmetic is float32, the gradient row is rounded once when it is stored).
#include "ftr_common.h"
#include "launch.h"

namespace ftr {
namespace {

constexpr int kConstrMaxRows = 15;   // band rows per frame = waves per workgroup: the domain of the band recursion

// column c of a register-resident row (quad i = lane + 64 q holds columns 4 i .. 4 i + 3), for a wave-uniform c
template <int NQ>
__device__ __forceinline__ float row_pick(const f4 (&v)[NQ], int lane, int c) {
  float cand = 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) cand = (4 * (lane + 64 * q) + e == c) ? v[q][e] : cand;
  }
  return __shfl(cand, (c >> 2) & 63);
}

// grid: one workgroup per frame; block: 64 r threads.  NQ >= 1: the row in NQ quads of registers per lane (C % 4 == 0,
// C <= 256 NQ, rows readable four elements at a time); NQ == 0: the general form, element by element in two passes.
template <typename E, int NQ, bool HAT>
__global__ __launch_bounds__(64 * kConstrMaxRows) void constr_frame_kernel(
    const E* __restrict__ logits, const int32_t* __restrict__ symbols, const int32_t* __restrict__ ranges,
    const int32_t* __restrict__ boundary, int blank, double delay_penalty, float* __restrict__ lse, float* __restrict__ pxb,
    float* __restrict__ pyb, size_t frames, int T, int S, int C, int r) {
  __shared__ float s_ty[16];
  __shared__ int s_ok[16];
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  const size_t bt = frames - 1 - blockIdx.x;   // last frames first: the joiner has just written the tail (lse_rows_reg_kernel)
  const int b = (int)(bt / T);
  const int t = (int)(bt - (size_t)b * T);
  const int tb = boundary ? max(boundary[4 * b + 1], 0) : 0;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const size_t row = bt * r + k;
  if (t < tb || t >= te) {   // the whole workgroup: nothing is read, no barrier is reached
    if (lane == 0) { lse[row] = 0.0f; pxb[row] = -INFINITY; pyb[row] = -INFINITY; }
    return;
  }
  const E* x = logits + row * C;
  float m = -INFINITY, sum = 0.0f, xb, xs;
  int s, sym = blank;
  bool sok;
  if constexpr (NQ > 0) {
    const int n4 = C >> 2;
    const f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    f4 v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = lane + 64 * q;
      v[q] = (i < n4) ? load4(x, i) : ninf;
    }
    s = ranges[bt * r] + k;   // after the row's loads are issued, so none of them waits for the symbol
    sok = s >= 0 && s <= S;
    if (sok && s < S) sym = min(max(symbols[(size_t)b * S + s], 0), C - 1);
    xb = row_pick<NQ>(v, lane, blank);
    xs = row_pick<NQ>(v, lane, sym);
    if (HAT) {   // Z: the blank column leaves the max and the sum
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q][e] = (4 * (lane + 64 * q) + e == blank) ? -INFINITY : v[q][e];
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) m = fmaxf(fmaxf(m, fmaxf(v[q][0], v[q][1])), fmaxf(v[q][2], v[q][3]));
    m = wave_max_dpp(m);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (lane + 64 * q < n4)   // the per-lane order of lse_rows_reg_kernel
        sum += __expf(v[q][0] - m) + __expf(v[q][1] - m) + __expf(v[q][2] - m) + __expf(v[q][3] - m);
    }
  } else {
    for (int i = lane; i < C; i += 64) m = fmaxf(m, (HAT && i == blank) ? -INFINITY : elem_to_float(x[i]));
    m = wave_max_dpp(m);
    for (int i = lane; i < C; i += 64) sum += __expf(((HAT && i == blank) ? -INFINITY : elem_to_float(x[i])) - m);   // L1 / L2
    s = ranges[bt * r] + k;
    sok = s >= 0 && s <= S;
    if (sok && s < S) sym = min(max(symbols[(size_t)b * S + s], 0), C - 1);
    xb = elem_to_float(x[blank]);
    xs = elem_to_float(x[sym]);
  }
  sum = wave_sum_dpp(sum);
  const float l = m + __logf(sum);
  float tx, ty;
  if (HAT) {
    hat_logprobs(xb, xs, l, sym == blank, &tx, &ty);
  } else {
    ty = xb - l;
    tx = xs - l;
  }
  if (!sok) ty = -INFINITY;
  if (lane == 0) { s_ty[k] = ty; s_ok[k] = sok ? 1 : 0; }
  __syncthreads();
  if (lane == 0) {
    float vx = -INFINITY;
    if (sok && s < S && k + 1 < r && s_ok[k + 1]) {
      vx = tx + s_ty[k + 1];
      if (delay_penalty > 0.0) vx += (float)((((double)te - 1.0) / 2.0 - (double)t) * delay_penalty);   // after the sum
    }
    lse[row] = l;
    pyb[row] = ty;
    pxb[row] = vx;
  }
}

// one wave per (b,t,k) row of glogits
template <typename E, bool VEC, bool HAT>
__global__ void constr_grad_kernel(const E* __restrict__ logits, const int32_t* __restrict__ symbols,
                                   const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                   const float* __restrict__ lse, const float* __restrict__ gxb,
                                   const float* __restrict__ gyb, const Scale scale, int blank, E* __restrict__ glogits,
                                   size_t rows, int T, int S, int C, int r) {
  const int lane = threadIdx.x & 63;
  const size_t rowi = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (rowi >= rows) return;
  const size_t row = rows - 1 - rowi;
  const size_t bt = row / r;
  const int k = (int)(row - bt * r);
  const int b = (int)(bt / T);
  const int t = (int)(bt - (size_t)b * T);
  const int tb = boundary ? max(boundary[4 * b + 1], 0) : 0;
  const int te = boundary ? boundary[4 * b + 3] : T;
  const int n4 = C >> 2;
  E* g = glogits + row * C;
  if (t < tb || t >= te) {   // a frame the forward did not read: zeros
    if (VEC) {
      const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int i = lane; i < n4; i += 64) store4(g, i, zero);
    } else {
      for (int c = lane; c < C; c += 64) g[c] = elem_from_float<E>(0.0f);
    }
    return;
  }
  const int s = ranges[bt * r] + k;
  const float sc = scale.at(b);
  const bool sok = s >= 0 && s <= S;
  float X = 0.0f;
  int sym = blank;
  if (sok && s < S) {
    sym = min(max(symbols[(size_t)b * S + s], 0), C - 1);   // the column the forward read
    if (k + 1 < r) X = gxb[row] * sc;                       // k + 1 == r: px_band was forced to -inf
  }
  float Y = sok ? gyb[row] * sc : 0.0f;
  if (sok && k >= 1 && s >= 1) {   // px_band[b,t,k-1] = tok_x(k-1) + tok_y(k): its blank factor is this row's
    const bool forced = HAT && min(max(symbols[(size_t)b * S + s - 1], 0), C - 1) == blank;
    if (!forced) Y += gxb[row - 1] * sc;
  }
  float tot = X + Y;
  const float l = lse[row];
  if (HAT) {
    if (sym == blank) X = 0.0f;   // px is -inf there
    tot = X;
  }
  const E* x = logits + row * C;
  if (VEC) {
    for (int i = lane; i < n4; i += 64) {
      const f4 v = load4(x, i);
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * i + e;
        float val = -tot * __expf(v[e] - l);
        if (c == sym) val += X;
        if (c == blank) {
          if (HAT) {
            float sp, sn;
            hat_sigmoids(v[e], &sp, &sn);
            val = Y * sn - X * sp;
          } else {
            val += Y;
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
      if (c == sym) val += X;
      if (c == blank) {
        if (HAT) {
          float sp, sn;
          hat_sigmoids(xc, &sp, &sn);
          val = Y * sn - X * sp;
        } else {
          val += Y;
        }
      }
      g[c] = elem_from_float<E>(val);
    }
  }
}

}  // namespace

int band_constrained_fwd(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                         int blank, double delay_penalty, float* lse, float* pxb, float* pyb, int B, int T, int S, int C, int r,
                         int hat, hipStream_t st) {
  const size_t frames = (size_t)B * T;
  if (frames == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("pruned_band_constrained_fwd", frames * r); if (rc32 != FTR_OK) return rc32; }
  dispatch_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    const E* x = static_cast<const E*>(logits);
    dispatch(hat != 0, [&](auto h) {
      constexpr bool HAT = decltype(h)::value;
      const bool reg = rows_vec4<E>(C, logits) && C <= 2048;   // 1, 2, 4 or 8 quads of elements per lane; else the general form
      dispatch_among<1, 2, 4, 8, 0>(!reg ? 0 : C <= 256 ? 1 : C <= 512 ? 2 : C <= 1024 ? 4 : 8, [&](auto n) {
        hipLaunchKernelGGL((constr_frame_kernel<E, decltype(n)::value, HAT>), dim3((unsigned)frames), dim3(64 * r), 0, st, x, symbols,
                           ranges, boundary, blank, delay_penalty, lse, pxb, pyb, frames, T, S, C, r);
      });
    });
  });
  return check_launch("band_constrained_frame");
}

int band_constrained_bwd(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                         int blank, const float* lse, const float* gxb, const float* gyb, Scale scale, void* glogits, int B, int T,
                         int S, int C, int r, int hat, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("pruned_band_constrained_bwd", rows); if (rc32 != FTR_OK) return rc32; }
  const int wpb = 4;
  const unsigned blocks = (unsigned)((rows + wpb - 1) / wpb);
  dispatch_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    dispatch(rows_vec4<E>(C, logits, glogits), [&](auto vec) {
      dispatch(hat != 0, [&](auto h) {
        hipLaunchKernelGGL((constr_grad_kernel<E, decltype(vec)::value, decltype(h)::value>), dim3(blocks), dim3(64 * wpb), 0, st,
                           static_cast<const E*>(logits), symbols, ranges, boundary, lse, gxb, gyb, scale, blank,
                           static_cast<E*>(glogits), rows, T, S, C, r);
      });
    });
  });
  return check_launch("band_constrained_grad");
}

}  // namespace ftr
