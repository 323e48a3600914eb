// csrc/kd_common.h -- what the distillation kernels on the pruned band share (gfx950): pruned_kd.hip (a dense teacher) and
// pruned_kd_topk.hip (a stored top-K teacher) state none of this themselves.  The node a row belongs to and whether it is
// looked at at all, the two guards of the row arithmetic, the zero gradient row, the dispatch over both element types, and
// the opening of the host functions.
#pragma once
#include "ftr_common.h"
#include "launch.h"

namespace ftr {

// x log(x / y) with the xlogy convention: a class of teacher mass 0 adds nothing, whatever the student says; NaN stays NaN
__device__ __forceinline__ float kd_term(float p, float logp_minus_logq) { return p == 0.0f ? 0.0f : p * logp_minus_logq; }

// a maximum to subtract that is never -inf (a row, or a rest class, of -inf only: exp(-inf - 0) = 0, not exp(NaN))
__device__ __forceinline__ float kd_safe_max(float m) { return m == -INFINITY ? 0.0f : m; }

// what a wave knows about its row before it touches the logits: the node (b, t, s = ranges[b,t,k]), the utterance's
// rectangle, whether the node lies inside it (geo), its weight (1 without weights), and `valid`: geo and the weight is not 0
struct KdNode { int b, t, s; Bound bd; bool geo, valid; float w; };
__device__ __forceinline__ KdNode kd_node(size_t row, const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                          const float* __restrict__ weights, int T, int S, int r) {
  KdNode n;
  const unsigned bt = (unsigned)row / (unsigned)r;   // rows < 2^31 (require_rows_32bit): 32-bit divisions, a tenth of the 64-bit ones
  n.b = (int)(bt / (unsigned)T);
  n.t = (int)(bt - (unsigned)n.b * (unsigned)T);
  n.s = ranges[row];
  n.bd = load_boundary(boundary, n.b, S, T);   // clamped into the lattice: s < se implies s < S
  n.geo = n.t >= n.bd.tb && n.t < n.bd.te && n.s >= n.bd.sb && n.s <= n.bd.se;
  n.valid = n.geo;
  n.w = 1.0f;
  if (weights) {
    n.w = weights[row];
    n.valid = n.valid && n.w != 0.0f;   // a NaN weight compares unequal: the node stays valid and its loss becomes NaN
  }
  return n;
}

// a gradient row of zeros, four at a time or one by one: written without a look at the logits
template <typename ES, bool VEC>
__device__ __forceinline__ void kd_zero_row(ES* __restrict__ gr, int lane, int W) {
  if (VEC) {
    const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = lane; i < (W >> 2); i += 64) store4(gr, i, zero);
  } else {
    for (int c = lane; c < W; c += 64) gr[c] = elem_from_float<ES>(0.0f);
  }
}

// both element types -> one call of f(elem_tag<ES>, elem_tag<ET>)
template <typename F>
inline auto dispatch_dtype2(int dtype, int teacher_dtype, F&& f) {
  return dispatch_dtype(dtype, [&](auto s) { return dispatch_dtype(teacher_dtype, [&](auto t) { return f(s, t); }); });
}

// The opening of every host function: rows = B T r; nothing to do without rows (done, rc = FTR_OK); the 32-bit limit of the
// row index (done, rc = its error); else the grid of one wave per row, KD_WPB rows per block, and 1 / tau.
constexpr int KD_WPB = 4;
struct KdLaunch { size_t rows; int rc; bool done; unsigned blocks; float inv_tau; };
inline KdLaunch kd_launch(const char* name, int B, int T, int r, float temperature) {
  KdLaunch k;
  k.rows = (size_t)B * T * r;
  k.rc = k.rows == 0 ? FTR_OK : require_rows_32bit(name, k.rows);
  k.done = k.rows == 0 || k.rc != FTR_OK;
  k.blocks = (unsigned)((k.rows + KD_WPB - 1) / KD_WPB);
  k.inv_tau = 1.0f / temperature;
  return k;
}

}  // namespace ftr
