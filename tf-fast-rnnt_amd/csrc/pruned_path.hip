// csrc/pruned_path.hip -- the log-probability of ONE given alignment under the pruned joiner, and its gradient
// (include/ftr_path.h; MI355X addition, no reference counterpart), gfx950.
// A path through utterance b's rectangle [s_begin, s_end] x [t_begin, t_end) is given by frames[b,s], the frame that emits
// symbols[b,s].  It takes one symbol arc per row and one blank arc per frame (modified: per frame that emits nothing), so of
// the T * s_range joiner rows of the utterance it touches S + T at the most.  The work is split by ARC, not by row:
//   path_arc_kernel   one wave per arc (b,a): a < S the symbol arc of row a, at node (a, frames[a]); a >= S the blank arc of
//                     frame t = a - S, at node (s(t), t), s(t) = s_begin + #{s : frames[s] <= t} (modified: < t), found by
//                     a binary search in the utterance's frames.  The wave index is wave-uniform for the compiler too, so
//                     the chain boundary -> frames -> ranges -> row address runs on the scalar unit.  The node's slot is
//                     the first k with ranges[b,t,k] == s: the lanes compare s_range slots at once, one ballot.  Then the
//                     row is read ONCE into registers (C % 4 == 0, C <= 256 * NQ; load4, every load issued before the first
//                     use) and reduced with the DPP ladders; arc_lp[b,a] and the two parts of the row's logsumexp are written.  A HAT blank arc
//                     needs x[blank] alone and reads nothing else.  An arc outside the rectangle writes 0 and reads no
//                     logits; an arc that is not an arc of a path (frame outside [t_begin, t_end), frames out of order, node
//                     absent from ranges, HAT symbol == blank) writes -inf and reads no logits.
//   path_arc_gen_kernel  any C and any alignment: the same arcs, the row re-read element by element (L1/L2 after the first
//                     sweep), every lane summing the columns the register form gives it in its order: the same bits.
//   path_sum_kernel   one wave per utterance: lane l adds arcs l, l + 64, ... in order, then the DPP ladder -- a fixed tree,
//                     no atomic, no fence.  One -inf arc makes the sum -inf.
//   path_grad_kernel  one wave per row (b,t,k) of glogits.  Whether node (ranges[b,t,k], t) carries an arc is decided from the
//                     two neighbours frames[s-1], frames[s] (for sorted frames the same verdict as the forward's binary
//                     search; unsorted frames have logprob = -inf and no gradient at all) and "k is the first slot with
//                     this s".  At most one arc leaves a node.  No arc, logprob == -inf or an upstream gradient of exactly
//                     0: the row is NOT read and zeros are stored.  Else one pass, g = up (1[c == target] - exp((x - m) - ls))
//                     with m, ls from arc_lse, in float32, rounded once into E.
#include "ftr_common.h"
#include "launch.h"

namespace ftr {
namespace {

constexpr int PA_WPB = 4;       // waves (arcs, rows) per block, as the sibling row kernels
constexpr int PA_REG_C = 2048;  // the longest register-resident row: 8 quads per lane

struct PathShape { int T, S, C, r, blank, modified; };

// lo + #{s in [lo, hi) : f[s] <= t} (strict: < t) for sorted f; for any f the result stays in [lo, hi] and no index leaves
// [lo, hi)
__device__ __forceinline__ int count_upto(const int32_t* __restrict__ f, int lo, int hi, int t, bool strict) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int v = f[mid];
    if (strict ? v < t : v <= t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the first slot k of a frame's ranges rg[0 .. r) with rg[k] == s, or -1: 64 slots per ballot
__device__ __forceinline__ int first_slot(const int32_t* __restrict__ rg, int r, int s, int lane) {
  for (int k0 = 0; k0 < r; k0 += 64) {
    const int k = k0 + lane;
    const unsigned long long hit = __ballot(k < r && rg[k] == s);
    if (hit) return k0 + (int)__builtin_ctzll(hit);
  }
  return -1;
}

// what arc (b,a) is: kind 0 = no arc here (writes 0), -1 = not an arc of a path (writes -inf), 1 = read `row`, column `tgt`
struct Arc { int kind; size_t row; int tgt; bool is_blank; };

template <bool HAT>
__device__ __forceinline__ Arc resolve_arc(const int32_t* __restrict__ symbols, const int32_t* __restrict__ ranges,
                                           const int32_t* __restrict__ boundary, const int32_t* __restrict__ frames, int b, int a,
                                           int lane, const PathShape g) {
  Arc arc = {0, 0, g.blank, a >= g.S};
  const Bound bd = load_boundary(boundary, b, g.S, g.T);
  if (bd.se < bd.sb || bd.te < bd.tb) return arc;   // an inverted rectangle has no arcs
  const int32_t* fb = frames + (size_t)b * g.S;     // S == 0: never dereferenced
  int s, t;
  if (!arc.is_blank) {
    s = a;
    if (s < bd.sb || s >= bd.se) return arc;
    t = fb[s];
    arc.kind = -1;
    if (t < bd.tb || t >= bd.te) return arc;
    if (s > bd.sb) {
      const int left = fb[s - 1];
      if (g.modified ? left >= t : left > t) return arc;
    }
    arc.tgt = min(max(symbols[(size_t)b * g.S + s], 0), g.C - 1);   // the column the builders read
    if (HAT && arc.tgt == g.blank) return arc;                      // HAT gives a symbol that is the blank no mass
  } else {
    t = a - g.S;
    if (t < bd.tb || t >= bd.te) return arc;
    s = count_upto(fb, bd.sb, bd.se, t, g.modified != 0);
    if (g.modified && s < bd.se && fb[s] == t) return arc;          // modified: an emitting frame has no blank arc
    arc.kind = -1;
  }
  const size_t bt = (size_t)b * g.T + t;
  const int k = first_slot(ranges + bt * g.r, g.r, s, lane);
  if (k < 0) return arc;
  arc.kind = 1;
  arc.row = bt * g.r + k;
  return arc;
}

// arc (b,a) of this wave; false past the last arc
__device__ __forceinline__ bool wave_arc(unsigned arcs, int per, int* b, int* a) {
  const unsigned idx = blockIdx.x * PA_WPB + (unsigned)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (idx >= arcs) return false;
  *b = (int)(idx / (unsigned)per);
  *a = (int)(idx - (unsigned)*b * (unsigned)per);
  return true;
}

// What an arc leaves behind: arc_lp[b,a], and in arc_lse [B,2,S+T] the row's maximum m (plane 0) and ls = log sum exp(x - m)
// (plane 1; HAT: both over the non-blank columns).  The logsumexp is m + ls; it is kept in two parts because the gradient
// needs exp(x - lse) to 2^-24 of ITSELF: (x - m) - ls is as accurate as the element is likely, m + ls rounded once is not
__device__ __forceinline__ void store_arc(float* __restrict__ arc_lp, float* __restrict__ arc_lse, int b, int a, int per, float lp,
                                          float m, float ls) {
  arc_lp[(size_t)b * per + a] = lp;
  arc_lse[(size_t)b * 2 * per + a] = m;
  arc_lse[((size_t)b * 2 + 1) * per + a] = ls;
}
// the arc's log-prob from its row's m and ls, x[tgt] and x[blank]
template <bool HAT>
__device__ __forceinline__ float arc_logprob(float xt, float xb, float m, float ls) {
  const float v = (xt - m) - ls;
  return HAT ? v - softplus(xb) : v;   // HAT: log sigmoid(-x[blank]) + x[sym] - Z
}

template <typename E, int NQ, bool HAT>
__global__ __launch_bounds__(64 * PA_WPB) void path_arc_kernel(const E* __restrict__ logits, const int32_t* __restrict__ symbols,
                                                               const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                                               const int32_t* __restrict__ frames, float* __restrict__ arc_lp,
                                                               float* __restrict__ arc_lse, unsigned arcs, const PathShape g) {
  const int lane = threadIdx.x & 63;
  int b, a;
  const int per = g.S + g.T;
  if (!wave_arc(arcs, per, &b, &a)) return;
  const Arc arc = resolve_arc<HAT>(symbols, ranges, boundary, frames, b, a, lane, g);
  if (arc.kind != 1) {
    if (lane == 0) store_arc(arc_lp, arc_lse, b, a, per, arc.kind < 0 ? -INFINITY : 0.0f, 0.0f, 0.0f);
    return;
  }
  const E* xr = logits + arc.row * g.C;
  if (HAT && arc.is_blank) {   // log sigmoid(x[blank]): one element of the row
    if (lane == 0) store_arc(arc_lp, arc_lse, b, a, per, -softplus(-elem_to_float(xr[g.blank])), 0.0f, 0.0f);
    return;
  }
  const int n4 = g.C >> 2;
  const f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  f4 v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    v[q] = (i < n4) ? load4(xr, i) : ninf;
  }
  const float xt = elem_to_float(xr[arc.tgt]);            // the line is on its way with the row
  const float xb = HAT ? elem_to_float(xr[g.blank]) : 0.0f;
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (HAT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[q][e] = (4 * (lane + 64 * q) + e == g.blank) ? -INFINITY : v[q][e];
    }
    m = fmaxf(fmaxf(m, fmaxf(v[q][0], v[q][1])), fmaxf(v[q][2], v[q][3]));
  }
  m = wave_max_dpp(m);
  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (lane + 64 * q < n4) {   // element by element: the order of path_arc_gen_kernel
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += __expf(v[q][e] - m);
    }
  }
  sum = wave_sum_dpp(sum);
  if (lane == 0) {
    const float ls = __logf(sum);
    store_arc(arc_lp, arc_lse, b, a, per, arc_logprob<HAT>(xt, xb, m, ls), m, ls);
  }
}

template <typename E, bool HAT>
__global__ __launch_bounds__(64 * PA_WPB) void path_arc_gen_kernel(const E* __restrict__ logits, const int32_t* __restrict__ symbols,
                                                                   const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                                                   const int32_t* __restrict__ frames, float* __restrict__ arc_lp,
                                                                   float* __restrict__ arc_lse, unsigned arcs, const PathShape g) {
  const int lane = threadIdx.x & 63;
  int b, a;
  const int per = g.S + g.T;
  if (!wave_arc(arcs, per, &b, &a)) return;
  const Arc arc = resolve_arc<HAT>(symbols, ranges, boundary, frames, b, a, lane, g);
  if (arc.kind != 1) {
    if (lane == 0) store_arc(arc_lp, arc_lse, b, a, per, arc.kind < 0 ? -INFINITY : 0.0f, 0.0f, 0.0f);
    return;
  }
  const E* xr = logits + arc.row * g.C;
  if (HAT && arc.is_blank) {
    if (lane == 0) store_arc(arc_lp, arc_lse, b, a, per, -softplus(-elem_to_float(xr[g.blank])), 0.0f, 0.0f);
    return;
  }
  const float xt = elem_to_float(xr[arc.tgt]);
  const float xb = HAT ? elem_to_float(xr[g.blank]) : 0.0f;
  float m = -INFINITY;
  for (int c = lane; c < g.C; c += 64) m = fmaxf(m, (HAT && c == g.blank) ? -INFINITY : elem_to_float(xr[c]));
  m = wave_max_dpp(m);
  float sum = 0.0f;
  for (int c0 = 4 * lane; c0 < g.C; c0 += 256) {   // the columns path_arc_kernel gives this lane, in its order
    for (int c = c0; c < min(c0 + 4, g.C); ++c) sum += __expf(((HAT && c == g.blank) ? -INFINITY : elem_to_float(xr[c])) - m);
  }
  sum = wave_sum_dpp(sum);
  if (lane == 0) {
    const float ls = __logf(sum);
    store_arc(arc_lp, arc_lse, b, a, per, arc_logprob<HAT>(xt, xb, m, ls), m, ls);
  }
}

__global__ __launch_bounds__(64 * PA_WPB) void path_sum_kernel(const float* __restrict__ arc_lp, float* __restrict__ logprob, int B,
                                                               int per) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * PA_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= B) return;
  const float* v = arc_lp + (size_t)b * per;
  float s = 0.0f;
  for (int i = lane; i < per; i += 64) s += v[i];
  s = wave_sum_dpp(s);
  if (lane == 0) logprob[b] = s;
}

template <typename E, bool VEC, bool HAT>
__global__ __launch_bounds__(64 * PA_WPB) void path_grad_kernel(const E* __restrict__ logits, const int32_t* __restrict__ symbols,
                                                                const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                                                const int32_t* __restrict__ frames, const float* __restrict__ arc_lse,
                                                                const float* __restrict__ logprob, const float* __restrict__ upstream,
                                                                E* __restrict__ glogits, unsigned rows, const PathShape g) {
  const int lane = threadIdx.x & 63;
  const unsigned row = blockIdx.x * PA_WPB + (unsigned)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;
  const unsigned bt = row / (unsigned)g.r;
  const int k = (int)(row - bt * (unsigned)g.r);
  const int b = (int)(bt / (unsigned)g.T);
  const int t = (int)(bt - (unsigned)b * (unsigned)g.T);
  const int s = ranges[row];
  const Bound bd = load_boundary(boundary, b, g.S, g.T);
  // which arc leaves node (s,t), if any: 1 the symbol arc of row s, 2 the blank arc of frame t
  int kind = 0;
  if (bd.sb <= bd.se && t >= bd.tb && t < bd.te && s >= bd.sb && s <= bd.se) {
    const int32_t* fb = frames + (size_t)b * g.S;
    const int big = 0x7fffffff;
    const int here = s < bd.se ? fb[s] : big;                // the frame that leaves row s
    const int left = s > bd.sb ? fb[s - 1] : -big - 1;       // the frame that entered it
    if (here == t) kind = 1;
    else if (here > t && (g.modified ? left < t : left <= t)) kind = 2;
  }
  float up = 0.0f;
  if (kind != 0 && first_slot(ranges + (size_t)bt * g.r, g.r, s, lane) == k && logprob[b] != -INFINITY) up = upstream[b];
  const size_t off = (size_t)row * g.C;
  E* gr = glogits + off;
  const int n4 = g.C >> 2;
  if (up == 0.0f) {   // the row is not read
    if (VEC) {
      const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int i = lane; i < n4; i += 64) store4(gr, i, zero);
    } else {
      for (int c = lane; c < g.C; c += 64) gr[c] = elem_from_float<E>(0.0f);
    }
    return;
  }
  const E* xr = logits + off;
  const int tgt = kind == 1 ? min(max(symbols[(size_t)b * g.S + s], 0), g.C - 1) : g.blank;
  const int per = g.S + g.T, a = kind == 1 ? s : g.S + t;
  const float m = arc_lse[(size_t)b * 2 * per + a], ls = arc_lse[((size_t)b * 2 + 1) * per + a];
  // gb: HAT's blank column; its softmax term runs over the non-blank columns of a symbol arc only
  float gb = 0.0f;
  if (HAT) {
    float sp, sn;
    hat_sigmoids(elem_to_float(xr[g.blank]), &sp, &sn);
    gb = kind == 1 ? -up * sp : up * sn;
  }
  const bool blank_only = HAT && kind == 2;   // a HAT blank arc: x[blank] was all it needed, the rest of the row is zeros
  auto grad_of = [&](int c, float x) -> float {
    if (HAT && c == g.blank) return gb;
    if (blank_only) return 0.0f;
    return up * ((c == tgt ? 1.0f : 0.0f) - __expf((x - m) - ls));
  };
  if (VEC) {
    const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = lane; i < n4; i += 64) {
      const f4 v = blank_only ? zero : load4(xr, i);
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = grad_of(4 * i + e, v[e]);
      store4(gr, i, o);
    }
  } else {
    for (int c = lane; c < g.C; c += 64) gr[c] = elem_from_float<E>(grad_of(c, blank_only ? 0.0f : elem_to_float(xr[c])));
  }
}

}  // namespace

int pruned_path_fwd(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                    const int32_t* frames, int blank, float* arc_lp, float* arc_lse, float* logprob, int B, int T, int S, int C,
                    int r, int modified, int hat, hipStream_t st) {
  const char* name = "pruned_path_logprob_fwd";
  const size_t arcs = (size_t)B * ((size_t)S + T);
  if (B == 0) return FTR_OK;
  { const int rc = require_rows_32bit(name, (size_t)B * T * r); if (rc != FTR_OK) return rc; }
  { const int rc = require_rows_32bit(name, arcs); if (rc != FTR_OK) return rc; }
  const PathShape g = {T, S, C, r, blank, modified};
  const unsigned blocks = (unsigned)((arcs + PA_WPB - 1) / PA_WPB);
  dispatch_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    const E* x = static_cast<const E*>(logits);
    dispatch(hat != 0, [&](auto h) {
      constexpr bool HAT = decltype(h)::value;
      if (rows_vec4<E>(C, x) && C <= PA_REG_C)   // the row fits the registers of a wave: 1, 2, 4 or 8 quads per lane
        dispatch_among<1, 2, 4, 8>(C <= 256 ? 1 : C <= 512 ? 2 : C <= 1024 ? 4 : 8, [&](auto n) {
          hipLaunchKernelGGL((path_arc_kernel<E, decltype(n)::value, HAT>), dim3(blocks), dim3(64 * PA_WPB), 0, st, x, symbols, ranges,
                             boundary, frames, arc_lp, arc_lse, (unsigned)arcs, g);
        });
      else
        hipLaunchKernelGGL((path_arc_gen_kernel<E, HAT>), dim3(blocks), dim3(64 * PA_WPB), 0, st, x, symbols, ranges, boundary, frames,
                           arc_lp, arc_lse, (unsigned)arcs, g);
    });
  });
  { const int rc = check_launch(name); if (rc != FTR_OK) return rc; }
  hipLaunchKernelGGL(path_sum_kernel, dim3((B + PA_WPB - 1) / PA_WPB), dim3(64 * PA_WPB), 0, st, arc_lp, logprob, B, S + T);
  return check_launch("pruned_path_logprob_sum");
}

int pruned_path_bwd(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                    const int32_t* frames, int blank, const float* arc_lse, const float* logprob, const float* upstream,
                    void* glogits, int B, int T, int S, int C, int r, int modified, int hat, hipStream_t st) {
  const char* name = "pruned_path_logprob_bwd";
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc = require_rows_32bit(name, rows); if (rc != FTR_OK) return rc; }
  const PathShape g = {T, S, C, r, blank, modified};
  const unsigned blocks = (unsigned)((rows + PA_WPB - 1) / PA_WPB);
  dispatch_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    const E* x = static_cast<const E*>(logits);
    E* gl = static_cast<E*>(glogits);
    dispatch(hat != 0, [&](auto h) {
      dispatch(rows_vec4<E>(C, x, gl), [&](auto vec) {
        hipLaunchKernelGGL((path_grad_kernel<E, decltype(vec)::value, decltype(h)::value>), dim3(blocks), dim3(64 * PA_WPB), 0, st, x,
                           symbols, ranges, boundary, frames, arc_lse, logprob, upstream, gl, (unsigned)rows, g);
      });
    });
  });
  return check_launch(name);
}

}  // namespace ftr
