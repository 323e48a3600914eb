// csrc/mi_band_tdt_common.h -- what the chains over the band's duration lattice share (gfx950): the move list, which cells
// the walk visits, and the scatter of the operands into wavefront order.  mi_band_tdt.hip (the float64 log-add chain of the
// TDT and multi-blank losses) and mi_band_viterbi.hip (the float32 select chain of the alignment) state none of this
// themselves; the geometry underneath is mi_band_common.h's.
#pragma once
#include "mi_band_common.h"

namespace ftr {

constexpr int kTdtThreads = 256;
constexpr int kTdtMaxMoves = 10;   // TDT: N <= 5 token moves and Ny <= 5 blank moves; multi-blank: 1 + 8
constexpr int kTdtMaxDep = 64;     // ring steps the static LDS holds (a duration of 32 needs all of them)
constexpr int TCH = 4;             // steps per operand fetch

// moves 0 .. Dx-1 are the token moves (px_band planes), Dx .. M-1 the blank moves (py_band planes)
struct BandMoves { int dur[kTdtMaxMoves]; int Dx, M; };

inline BandMoves make_band_moves(const int32_t* tok, int N, const int32_t* blk, int Ny) {
  BandMoves mv;
  for (int m = 0; m < kTdtMaxMoves; ++m) mv.dur[m] = m < N ? tok[m] : (m < N + Ny ? blk[m - N] : 1);
  mv.Dx = N; mv.M = N + Ny;
  return mv;
}
// the power of two above the largest step offset of a move (a token of duration e reads e + 1 steps back)
inline int ring_depth_for(int far) {
  int dep = 2;
  while (dep <= far) dep *= 2;
  return dep;
}
inline int band_tdt_ring_depth(const int32_t* tok, int N, const int32_t* blk, int Ny) {
  return ring_depth_for((tok[N - 1] + 1 > blk[Ny - 1]) ? tok[N - 1] + 1 : blk[Ny - 1]);
}

// is (s,t) a cell of the walk?  (rg: the utterance's ranges)
template <int LANES>
__device__ __forceinline__ bool tdt_cell(const BandGeom<false, LANES>& g, const int32_t* __restrict__ rg, int s, int t) {
  if (s < g.sb || s > g.se || t < g.tb || t > g.te) return false;
  if (t == g.te) return s == g.se;
  return g.in_band(s, t, rg[(size_t)t * g.r]);
}
// operand of move m at the frame cell (s,t)
template <int LANES>
__device__ __forceinline__ float tdt_operand(const BandGeom<false, LANES>& g, const int32_t* __restrict__ rg, const float* __restrict__ pxu,
                                             const float* __restrict__ pyu, size_t plane, int Dx, int m, int s, int t) {
  const float* src = m < Dx ? pxu + (size_t)m * plane : pyu + (size_t)(m - Dx) * plane;
  return src[(size_t)t * g.r + (s - rg[(size_t)t * g.r])];
}

// the one precondition of the wavefront order, on the ranges themselves: does the band start decrease inside the
// rectangle?  Workgroup-wide (a barrier).
__device__ __forceinline__ bool tdt_band_start_decreases(const int32_t* rg, int tb, int te, int r, int tid) {
  int bad = 0;
  for (int t = tb + 1 + tid; t < te; t += kTdtThreads) bad |= (rg[(size_t)t * r] < rg[(size_t)(t - 1) * r]);
  return __syncthreads_or(bad) != 0;
}

// The cells of the walk, enumerated: i < (te - tb) * r are the band rows of the frames tb <= t < te, i = (te - tb) * r is
// the end cell.  False for a band row outside the rectangle's rows.
__device__ __forceinline__ bool tdt_nth_cell(const int32_t* rg, int sb, int tb, int se, int te, int r, int i, int& s, int& t) {
  if (i == (te - tb) * r) { s = se; t = te; }
  else { t = tb + i / r; s = rg[(size_t)t * r] + (i - (t - tb) * r); }
  return s >= sb && s <= se;
}

// The scatter of one cell (s,t) of the walk into wavefront order: its M operands go to O[step][move][lane] -- chain A: the
// moves INTO the cell at step dgA, chain B: those OUT of it at step dgB -- -inf where the move does not exist; the origin
// (chain B: the end cell) gets 0 as its first blank operand, which the 0 seeded in the ring leads from.  The caller fills O
// with -inf first and enumerates the cells with tdt_cell_of.
template <int LANES, int M>
__device__ __forceinline__ void tdt_scatter_cell(const BandGeom<false, LANES>& g, const int32_t* __restrict__ rg, const float* __restrict__ pxu,
                                                 const float* __restrict__ pyu, size_t plane, const BandMoves& mv, bool isB, float* O, int s, int t) {
  const int Dx = mv.Dx;
  const float NEGF = -__builtin_inff();
  const int slot = isB ? (g.dgB(s, t) * M) * LANES + g.laneB(s) : (g.dgA(s, t) * M) * LANES + g.laneA(s);
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int ds = m < Dx ? 1 : 0, d = mv.dur[m];
    float v = NEGF;
    if (isB) {
      if (t < g.te && tdt_cell(g, rg, s + ds, t + d)) v = tdt_operand(g, rg, pxu, pyu, plane, Dx, m, s, t);
      if (t == g.te && m == Dx) v = 0.0f;
    } else {
      if (t - d < g.te && tdt_cell(g, rg, s - ds, t - d)) v = tdt_operand(g, rg, pxu, pyu, plane, Dx, m, s - ds, t - d);
      if (s == g.sb && t == g.tb && m == Dx) v = 0.0f;
    }
    O[slot + m * LANES] = v;
  }
}

}  // namespace ftr
