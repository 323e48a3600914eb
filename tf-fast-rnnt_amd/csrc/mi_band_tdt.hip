// csrc/mi_band_tdt.hip -- the TDT recursion (mi_tdt.hip) on the pruned band itself: a fourth schedule over
// mi_band_common.h (gfx950; regular type).  No lattice exists: work and memory per utterance are (S+T) * LANES * (N+Ny).
//
//   p[s,t] = logadd( (+)_i p[s-1,t-e_i] + px_i[s-1,t-e_i],  (+)_j p[s,t-d_j] + py_j[s,t-d_j] ),   p[s_begin,t_begin] = 0
//
// Cells.  The walk visits the band cells (lo[t] + k, t) of the frames t_begin <= t < t_end that lie in the boundary
// rectangle, and the end cell (s_end, t_end), which is a destination without being a band cell.  A move exists iff its
// source and its destination are such cells; the frames it skips need not be in the band.  A destination that is no
// cell has no way on and would contribute nothing, so the move is dropped.
//
// Geometry (BandGeom, regular type): chain A puts cell (s,t) at walk step (s-sb)+(t-tb), lane (s-sb) mod LANES, with
// the transitions INTO the cell as its operands; chain B at step (se-s)+(te-t), lane (se-s) mod LANES, with the
// transitions OUT of it.  In either order a blank of duration d reads the lane's own value d steps back and a token of
// duration e the cyclically previous lane's value e + 1 steps back: one list of M = N + Ny moves with a step offset
// and a lane offset each.  The values of the last DEP steps stay in an LDS ring, hist[step & (DEP-1)][lane], DEP a
// launch parameter (a power of two > the largest offset).  The operands are scattered into wavefront order
// O[step][move][lane] first, -inf where a transition does not exist, so the chain has no predicate at all: the origin
// (chain B: the end cell) starts through its first blank operand = 0 and a 0 seeded in the ring one blank step before
// the walk.  A slot without a cell has -inf operands only and holds -inf.
//
// Schedule.  band_tdt_chain_kernel, grid (B, 2): one workgroup per utterance and direction scatters its operands (256
// threads), then its first LANES threads walk all S_n + T_n - 1 steps in float64 -- the maximum in double, the bounded
// remainder through the float32 exp2 / log2 units, as mi_tdt.hip -- fetching the operands one chunk of TCH steps ahead,
// and leave p (chain A) / q (chain B) of every slot in the workspace.  band_tdt_occupancy_kernel, one thread per band
// row, then writes exp(p(src) + operand + q(dst) - ans) for every move of every band cell, 0 where the move does not
// exist: every element of gx_band / gy_band is written, nothing is cleared beforehand.  Two launches, no atomics: the
// results are the same bits on every run.
//
// A band whose start decreases inside the rectangle puts two cells into one slot: ans = NaN, zero occupancies, as
// mi_band.hip answers it.
//
// Domain.  The kernels take any list of up to kTdtMaxMoves moves whose step offsets fit the ring; which lists an entry
// point admits is a BandMoveDomain (ftr_common.h) that the host functions take as a parameter: (5, 5, 16) for TDT, and
// (1, 8, 32) for the multi-blank recursion (include/ftr_band_multiblank.h), which is the same chain with one token move
// of duration 0 and D <= 8 blank moves of durations up to 32: M = D + 1 <= 9, DEP = 64 at duration 32.
#include "mi_band_tdt_common.h"
#include "mi_rowlane.h"   // exp_of

namespace ftr {
namespace {

// the workspace: doubles first -- head [B][2] = (ans, flat: 1 when the utterance is answered without occupancies) and
// P [B][2][steps * LANES] (p of chain A's slots, q of chain B's) -- then the floats O [B][2][(steps + TCH) * M * LANES]
struct TdtLayout { size_t steps, p_per, o_per, p_off, o_off_floats, total_floats; };
inline TdtLayout tdt_layout(int B, int T, int S, int lanes, int M) {
  TdtLayout L;
  L.steps = ((size_t)S + T + 1 + TCH - 1) / TCH * TCH;
  L.p_per = L.steps * lanes;
  L.o_per = (L.steps + TCH) * M * lanes;
  L.p_off = (size_t)B * 2;
  L.o_off_floats = 2 * (L.p_off + (size_t)B * 2 * L.p_per);
  L.total_floats = L.o_off_floats + (size_t)B * 2 * L.o_per;
  return L;
}

template <int LANES, int M>
__global__ void __launch_bounds__(kTdtThreads) band_tdt_chain_kernel(
    const float* __restrict__ pxb, const float* __restrict__ pyb, const int32_t* __restrict__ ranges,
    const int32_t* __restrict__ boundary, const BandMoves mv, double* __restrict__ wsd, float* __restrict__ wsf,
    float* __restrict__ ans, size_t p_per, size_t o_per, int B, int T, int S, int r, int DEP) {
  __shared__ double hist[kTdtMaxDep * LANES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool isB = blockIdx.y != 0;
  const int Dx = mv.Dx;
  const BandUtt u = band_utt<false>(boundary, b, S, T);
  double* head = wsd + (size_t)b * 2;
  if (u.degenerate) {
    if (!isB && tid == 0) { const float a = band_degenerate_ans(u); ans[b] = a; head[0] = (double)a; head[1] = 1.0; }
    return;
  }
  const int32_t* rg = ranges + (size_t)b * T * r;
  const int sb = u.bd.sb, tb = u.bd.tb, se = u.bd.se, te = u.bd.te, D = u.D;
  if (tdt_band_start_decreases(rg, tb, te, r, tid)) {
    if (!isB && tid == 0) { ans[b] = __builtin_nanf(""); head[0] = __builtin_nan(""); head[1] = 1.0; }
    return;
  }
  const BandGeom<false, LANES> g(r, u.bd, 0, 0, 0);
  const size_t plane = (size_t)T * r;
  const float* pxu = pxb + (size_t)b * Dx * plane;
  const float* pyu = pyb + (size_t)b * (M - Dx) * plane;
  double* P = wsd + (size_t)B * 2 + ((size_t)b * 2 + (isB ? 1 : 0)) * p_per;
  float* O = wsf + ((size_t)b * 2 + (isB ? 1 : 0)) * o_per;
  const int nch = (D + 1 + TCH - 1) / TCH;
  const float NEGF = -__builtin_inff();
  const double NEG = -__builtin_inf();

  // ---- the operands in wavefront order: every slot of the steps the chain computes is -inf, then the cells' moves
  for (int i = tid; i < nch * TCH * M * LANES; i += kTdtThreads) O[i] = NEGF;
  for (int i = tid; i < DEP * LANES; i += kTdtThreads) hist[i] = NEG;
  __syncthreads();
  if (tid == 0) hist[((0 - mv.dur[Dx]) & (DEP - 1)) * LANES] = 0.0;   // what the first cell's blank operand 0 leads from
  const int ncell = (te - tb) * r + 1;                                // the frames' band rows, and the end cell
  for (int i = tid; i < ncell; i += kTdtThreads) {
    int s, t;
    if (!tdt_nth_cell(rg, sb, tb, se, te, r, i, s, t)) continue;
    tdt_scatter_cell<LANES, M>(g, rg, pxu, pyu, plane, mv, isB, O, s, t);
  }
  __syncthreads();
  if (tid >= LANES) return;

  // ---- the chain: LANES threads of wave 0
  const int lane = tid;
  int roff[M];   // ring offset of move m's source, less the step
#pragma unroll
  for (int m = 0; m < M; ++m) roff[m] = m < Dx ? ((lane - 1) & (LANES - 1)) - (mv.dur[m] + 1) * LANES : lane - mv.dur[m] * LANES;
  const int rmask = DEP * LANES - 1;
  const int endlane = isB ? g.laneB(sb) : g.laneA(se);
  float cur[TCH][M], nxt[TCH][M];
  auto fetch = [&](float (&o)[TCH][M], int c) {
#pragma unroll
    for (int q = 0; q < TCH; ++q)
#pragma unroll
      for (int m = 0; m < M; ++m) o[q][m] = O[((size_t)(c * TCH + q) * M + m) * LANES + lane];
  };
  fetch(cur, 0);
  double vend = NEG;
  for (int c = 0; c < nch; ++c) {
    fetch(nxt, c + 1);                                  // the array is one chunk longer than the walk
#pragma unroll
    for (int q = 0; q < TCH; ++q) {
      const int w = c * TCH + q;
      double term[M];
      double m0 = NEG, plain = NEG;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        term[m] = hist[(w * LANES + roff[m]) & rmask] + (double)cur[q][m];
        m0 = fmax(m0, term[m]);
        plain += term[m];
      }
      float sum = 0.0f;
#pragma unroll
      for (int m = 0; m < M; ++m) sum += rowlane::exp_of(term[m] - m0);
      double v = m0 + (double)(__builtin_amdgcn_logf(sum) * kLn2);
      if (m0 == NEG) v = plain;                         // all -inf (or a NaN among them, which the sum keeps)
      hist[(w * LANES + lane) & rmask] = v;
      P[(size_t)w * LANES + lane] = v;
      if (w == D) vend = v;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the next lane reads it in a later step
    }
#pragma unroll
    for (int q = 0; q < TCH; ++q)
#pragma unroll
      for (int m = 0; m < M; ++m) cur[q][m] = nxt[q][m];
  }
  if (!isB && lane == endlane) { ans[b] = (float)vend; head[0] = vend; head[1] = 0.0; }
}

// one thread per band row (b,t,k): the occupancies of the M moves out of its cell
template <int LANES>
__global__ void __launch_bounds__(256) band_tdt_occupancy_kernel(
    const float* __restrict__ pxb, const float* __restrict__ pyb, const int32_t* __restrict__ ranges,
    const int32_t* __restrict__ boundary, const BandMoves mv, const double* __restrict__ wsd, float* __restrict__ gxb,
    float* __restrict__ gyb, size_t p_per, size_t rows, int B, int T, int S, int r) {
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const size_t bt = row / r;
  const int k = (int)(row - bt * r);
  const int b = (int)(bt / T), t = (int)(bt - (size_t)b * T);
  const int Dx = mv.Dx, M = mv.M;
  const size_t plane = (size_t)T * r;
  const size_t cell = (size_t)t * r + k;
  float* gxu = gxb + (size_t)b * Dx * plane;
  float* gyu = gyb + (size_t)b * (M - Dx) * plane;
  const BandUtt u = band_utt<false>(boundary, b, S, T);
  const double A = wsd[(size_t)b * 2], flat = wsd[(size_t)b * 2 + 1];
  const int32_t* rg = ranges + (size_t)b * T * r;
  const BandGeom<false, LANES> g(r, u.bd, 0, 0, 0);
  const int s = rg[(size_t)t * r] + k;
  const bool live = !u.degenerate && flat == 0.0 && A != -__builtin_inf() && t >= g.tb && t < g.te && s >= g.sb && s <= g.se;
  const double* PA = wsd + (size_t)B * 2 + ((size_t)b * 2) * p_per;
  const double* PB = PA + p_per;
  double base = 0.0;
  if (live) base = PA[(size_t)g.dgA(s, t) * LANES + g.laneA(s)] - A;
  for (int m = 0; m < M; ++m) {
    const int ds = m < Dx ? 1 : 0, d = mv.dur[m];
    float occ = 0.0f;
    if (live && tdt_cell(g, rg, s + ds, t + d)) {
      const float* src = m < Dx ? pxb + ((size_t)b * Dx + m) * plane : pyb + ((size_t)b * (M - Dx) + (m - Dx)) * plane;
      occ = rowlane::exp_of(base + (double)src[cell] + PB[(size_t)g.dgB(s + ds, t + d) * LANES + g.laneB(s + ds)]);
    }
    (m < Dx ? gxu + (size_t)m * plane : gyu + (size_t)(m - Dx) * plane)[cell] = occ;
  }
}

}  // namespace

// r within the band kernels' lanes, the move counts of the entry point's domain, and slot indices that stay 32-bit
int mi_band_tdt_supported(int T, int S, int r, int N, int Ny, BandMoveDomain dom) {
  static_assert(kBandTdtDomain.max_tok + kBandTdtDomain.max_blk <= kTdtMaxMoves &&
                kBandMultiblankDomain.max_tok + kBandMultiblankDomain.max_blk <= kTdtMaxMoves, "the chain is instantiated for 2..kTdtMaxMoves moves");
  const int lanes = band_lanes_for(r);
  if (!lanes || T < 1 || S < 0 || N < 1 || N > dom.max_tok || Ny < 1 || Ny > dom.max_blk) return 0;
  return ((uint64_t)S + T + 1 + 2 * TCH) * (uint64_t)(lanes * (N + Ny)) < (1ull << 31) ? 1 : 0;
}

size_t mi_band_tdt_workspace_floats(int B, int T, int S, int r, int N, int Ny, BandMoveDomain dom) {
  if (B < 0 || !mi_band_tdt_supported(T, S, r, N, Ny, dom)) return 0;
  return tdt_layout(B, T, S, band_lanes_for(r), N + Ny).total_floats;
}

int mi_band_tdt(const float* pxb, const float* pyb, const int32_t* ranges, const int32_t* boundary, const int32_t* tok, int N,
                const int32_t* blk, int Ny, float* ws, size_t ws_floats, float* ans, float* gxb, float* gyb, int B, int T,
                int S, int r, BandMoveDomain dom, const char* what, hipStream_t st) {
  if (B == 0) return FTR_OK;
  if (!mi_band_tdt_supported(T, S, r, N, Ny, dom)) {
    set_error("%s: T=%d S=%d r=%d N=%d Ny=%d is outside the kernel's domain (r <= 15, 1..%d token and 1..%d blank moves)", what, T, S,
              r, N, Ny, dom.max_tok, dom.max_blk);
    return FTR_ERR_UNSUPPORTED;
  }
  if (B > 65535) { set_error("%s: B = %d exceeds the 65535 utterances of one launch", what, B); return FTR_ERR_UNSUPPORTED; }
  const size_t rows = (size_t)B * T * r;
  { const int rc32 = require_rows_32bit(what, rows); if (rc32 != FTR_OK) return rc32; }
  const int lanes = band_lanes_for(r), M = N + Ny;
  const int DEP = band_tdt_ring_depth(tok, N, blk, Ny);
  static_assert(kBandTdtDomain.max_dur < kTdtMaxDep && kBandMultiblankDomain.max_dur < kTdtMaxDep, "the ring must hold the longest move");
  if (DEP > ring_depth_for(dom.max_dur)) {
    set_error("%s: a ring of %d steps exceeds the %d of durations up to %d", what, DEP, ring_depth_for(dom.max_dur), dom.max_dur);
    return FTR_ERR_UNSUPPORTED;
  }
  const TdtLayout L = tdt_layout(B, T, S, lanes, M);
  if (ws_floats < L.total_floats) {
    set_error("%s: workspace of %zu floats is too small, %zu needed", what, ws_floats, L.total_floats);
    return FTR_ERR_INVALID_ARG;
  }
  const BandMoves mv = make_band_moves(tok, N, blk, Ny);
  double* wsd = reinterpret_cast<double*>(ws);
  float* wsf = ws + L.o_off_floats;
  const bool grads = gxb != nullptr;
  dispatch_among<8, 16>(lanes, [&](auto ln) {
    dispatch_range<2, kTdtMaxMoves>(M, [&](auto m) {
      hipLaunchKernelGGL((band_tdt_chain_kernel<decltype(ln)::value, decltype(m)::value>), dim3(B, grads ? 2 : 1), dim3(kTdtThreads), 0,
                         st, pxb, pyb, ranges, boundary, mv, wsd, wsf, ans, L.p_per, L.o_per, B, T, S, r, DEP);
    }, [] {});   // supported() admits no other count
  });
  int rc = check_launch("band_tdt_chain");
  if (rc != FTR_OK || !grads) return rc;
  dispatch_among<8, 16>(lanes, [&](auto ln) {
    hipLaunchKernelGGL((band_tdt_occupancy_kernel<decltype(ln)::value>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, pxb, pyb,
                       ranges, boundary, mv, wsd, gxb, gyb, L.p_per, rows, B, T, S, r);
  });
  return check_launch("band_tdt_occupancy");
}

// the multi-blank recursion: the same chain with one token move of duration 0 (px_band [B,T,r] is its one plane) and the
// D blank moves of `durations`
int mi_band_multiblank(const float* pxb, const float* pyb, const int32_t* ranges, const int32_t* boundary, const int32_t* durations,
                       int D, float* ws, size_t ws_floats, float* ans, float* gxb, float* gyb, int B, int T, int S, int r,
                       hipStream_t st) {
  const int32_t tok[1] = {0};
  return mi_band_tdt(pxb, pyb, ranges, boundary, tok, 1, durations, D, ws, ws_floats, ans, gxb, gyb, B, T, S, r,
                     kBandMultiblankDomain, "mutual_information_band_multiblank", st);
}

}  // namespace ftr
