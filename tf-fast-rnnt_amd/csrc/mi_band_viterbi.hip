// csrc/mi_band_viterbi.hip -- best-path (Viterbi) alignment on the pruned band itself (gfx950): the select rule and the
// backtrace of mi_viterbi_tdt.hip on the chain of mi_band_tdt.hip.  No lattice exists: work and memory per utterance are
// (S+T) * LANES * (N+Ny).  include/ftr_band_viterbi.h states the definition; in short
//
//   cells: the band cells of the frames t_begin <= t < t_end inside the boundary rectangle, and the end cell; a move
//          exists iff its source and its destination are such cells (mi_band_tdt_common.h, as the band TDT loss)
//   cand[m] = p[src_m] + op_m[src_m]  (one float32 add; the operand of a move that does not exist is -inf)
//   best = cand[M-1]; move = M-1;  for m = M-2 .. 0: take = isnan(cand[m]) || cand[m] >= best; if take: best, move = cand[m], m
//   p[s_begin,t_begin] = 0, score = p[s_end,t_end]
//
// band_viterbi_kernel<LANES, M>, one workgroup of 256 threads per utterance, one launch:
//   1. scatter: the band-start check and chain A's operands O[step][move][lane] (tdt_scatter_cell, the function the band
//      TDT chain calls for each cell), the ring seeded for the origin through its first blank operand; and one flag per slot, C[step][lane]
//      = 1 where the slot holds a cell.  A slot without a cell is held at -inf, so that a move whose source is no cell
//      reads -inf + -inf: a NaN travels along moves that exist and along no other (on the lattice it also crosses cells
//      outside the band, NaN + -inf: the one stated deviation from the lattice route, which is otherwise equal bit for bit).
//   2. chain: the first LANES threads of wave 0 walk the S_n + T_n - 1 steps in float32: M ring reads, M adds, the
//      ordered select, one ring write per step; operands fetched one chunk of TCH steps ahead.  The ring is 64 steps
//      deep, whatever the moves: it serves a blank of 32 frames and a token of 16.
//   3. decisions: 4 bits per slot, one word per step: bit plane pl of the move index is a ballot over the chain's lanes
//      and sits at bits [pl * LANES, (pl + 1) * LANES) -- 64 bits at 16 lanes, 32 at 8.  The TCH words of a chunk are
//      stored by TCH lanes side by side, contiguous along the step, in the workspace (not LDS: S + T is unbounded, and one
//      home is simpler than two).  Every word the backtrace reads is written by the same launch.
//   4. backtrace, after a barrier: all threads write the -1 / 0 fills, then wave 0 walks back from the end slot: a token
//      of duration e goes back e + 1 steps and one lane, a blank of duration d goes back d steps on its lane.  The wave
//      holds the words of 64 consecutive steps in its lanes, the next lower window in flight (a stride is at most 33),
//      and reads a step by readlane: no dependent global load per move.  Bounded by S_n + T_n moves.
// Workgroup-scope barriers only, no atomics, no memset: capturable, and the same bits on every run.
#include "mi_band_tdt_common.h"
#include "launch.h"   // dispatch_among, dispatch_range

namespace ftr {
namespace {

typedef unsigned long long u64;
constexpr int kVitDep = 64;        // ring steps
constexpr int kVitMaxMoves = 9;    // N + Ny of the entry point (the alignment's limit on the lattice, too)
constexpr int kVitMaxTok = 16, kVitMaxBlk = 32;
static_assert(kVitMaxBlk < kVitDep && kVitMaxTok + 1 < kVitDep && (kVitDep & (kVitDep - 1)) == 0, "the ring must hold the longest move");
static_assert(kVitMaxBlk + 1 <= 64 && kVitMaxTok + 1 <= 64, "a backtrace stride must stay inside the prefetched window");
static_assert(kVitMaxMoves <= 16 && kVitMaxMoves <= kTdtMaxMoves, "a move index has 4 bits");

template <int LANES> struct DecWord;
template <> struct DecWord<16> { typedef u64 type; };
template <> struct DecWord<8> { typedef unsigned type; };

// the workspace: the floats O [B][(steps + TCH) * M * LANES] and C [B][(steps + TCH) * LANES], then the decision words [B][steps]
struct VitLayout { size_t steps, o_per, c_per, c_off, dec_off, total; };
inline VitLayout vit_layout(int B, int T, int S, int lanes, int M) {
  VitLayout L;
  L.steps = ((size_t)S + T + 1 + TCH - 1) / TCH * TCH;
  L.o_per = (L.steps + TCH) * M * lanes;                       // a multiple of 32 floats: the words stay 8-byte aligned
  L.c_per = (L.steps + TCH) * lanes;
  L.c_off = (size_t)B * L.o_per;                               // in floats
  L.dec_off = (L.c_off + (size_t)B * L.c_per) * sizeof(float);
  L.total = L.dec_off + (size_t)B * L.steps * (lanes == 16 ? sizeof(u64) : sizeof(unsigned));
  return L;
}

template <int LANES, int M>
__global__ void __launch_bounds__(kTdtThreads) band_viterbi_kernel(
    const float* __restrict__ pxb, const float* __restrict__ pyb, const int32_t* __restrict__ ranges,
    const int32_t* __restrict__ boundary, const BandMoves mv, float* __restrict__ wsf, typename DecWord<LANES>::type* __restrict__ wsd,
    float* __restrict__ score, int32_t* __restrict__ frames, int32_t* __restrict__ durations, int32_t* __restrict__ blank_steps,
    size_t o_per, size_t c_per, size_t c_off, size_t d_per, int T, int S, int r) {
  typedef typename DecWord<LANES>::type word_t;
  __shared__ float hist[kVitDep * LANES];
  __shared__ float sh_score;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Dx = mv.Dx;
  const BandUtt u = band_utt<false>(boundary, b, S, T);
  int32_t* fr_b = frames + (size_t)b * S;
  int32_t* du_b = durations + (size_t)b * S;
  int32_t* bs_b = blank_steps + (size_t)b * T;
  auto answer_flat = [&](float a) {   // no path to report: everything -1
    if (tid == 0) score[b] = a;
    for (int s = tid; s < S; s += kTdtThreads) { fr_b[s] = -1; du_b[s] = -1; }
    for (int t = tid; t < T; t += kTdtThreads) bs_b[t] = -1;
  };
  // an inverted rectangle: 0; a single column has no frame: only the one-cell rectangle has a path, the empty one
  if (u.degenerate) { answer_flat(band_degenerate_ans(u)); return; }
  const int32_t* rg = ranges + (size_t)b * T * r;
  const int sb = u.bd.sb, tb = u.bd.tb, se = u.bd.se, te = u.bd.te, D = u.D;
  if (tdt_band_start_decreases(rg, tb, te, r, tid)) { answer_flat(__builtin_nanf("")); return; }
  const BandGeom<false, LANES> g(r, u.bd, 0, 0, 0);
  const size_t plane = (size_t)T * r;
  const float* pxu = pxb + (size_t)b * Dx * plane;
  const float* pyu = pyb + (size_t)b * (M - Dx) * plane;
  float* O = wsf + (size_t)b * o_per;
  float* C = wsf + c_off + (size_t)b * c_per;
  word_t* dec = wsd + (size_t)b * d_per;
  const int nch = (D + 1 + TCH - 1) / TCH;
  const float NEG = -__builtin_inff();

  // ---- the operands in wavefront order: every slot of the steps the chain computes is -inf and holds no cell, then the
  // cells' moves (tdt_scatter_cell, as the band TDT chain) and their flags; the ring is -inf but for the 0 that the
  // origin's first blank operand, itself 0, leads from
  for (int i = tid; i < nch * TCH * M * LANES; i += kTdtThreads) O[i] = NEG;
  for (int i = tid; i < nch * TCH * LANES; i += kTdtThreads) C[i] = 0.0f;
  for (int i = tid; i < kVitDep * LANES; i += kTdtThreads) hist[i] = NEG;
  __syncthreads();
  if (tid == 0) hist[((0 - mv.dur[Dx]) & (kVitDep - 1)) * LANES] = 0.0f;
  const int ncell = (te - tb) * r + 1;                                // the frames' band rows, and the end cell
  for (int i = tid; i < ncell; i += kTdtThreads) {
    int s, t;
    if (!tdt_nth_cell(rg, sb, tb, se, te, r, i, s, t)) continue;
    tdt_scatter_cell<LANES, M>(g, rg, pxu, pyu, plane, mv, false, O, s, t);
    C[g.dgA(s, t) * LANES + g.laneA(s)] = 1.0f;
  }
  __syncthreads();

  // ---- the chain: LANES threads of wave 0
  if (tid < LANES) {
    const int lane = tid;
    int roff[M];   // ring offset of move m's source, less the step
#pragma unroll
    for (int m = 0; m < M; ++m) roff[m] = m < Dx ? ((lane - 1) & (LANES - 1)) - (mv.dur[m] + 1) * LANES : lane - mv.dur[m] * LANES;
    constexpr int rmask = kVitDep * LANES - 1;
    const int endlane = g.laneA(se);
    float cur[TCH][M], nxt[TCH][M], ccur[TCH], cnxt[TCH];
    auto fetch = [&](float (&o)[TCH][M], int c) {
#pragma unroll
      for (int q = 0; q < TCH; ++q)
#pragma unroll
        for (int m = 0; m < M; ++m) o[q][m] = O[((size_t)(c * TCH + q) * M + m) * LANES + lane];
    };
    auto fetch_cell = [&](float (&f)[TCH], int c) {
#pragma unroll
      for (int q = 0; q < TCH; ++q) f[q] = C[(size_t)(c * TCH + q) * LANES + lane];
    };
    fetch(cur, 0); fetch_cell(ccur, 0);
    float vend = NEG;
    for (int c = 0; c < nch; ++c) {
      fetch(nxt, c + 1); fetch_cell(cnxt, c + 1);         // the arrays are one chunk longer than the walk
      word_t mine = 0;                                    // lane q keeps the word of the chunk's step q
#pragma unroll
      for (int q = 0; q < TCH; ++q) {
        const int w = c * TCH + q;
        float cand[M];
#pragma unroll
        for (int m = 0; m < M; ++m) cand[m] = hist[(w * LANES + roff[m]) & rmask] + cur[q][m];
        float v = cand[M - 1];
        int sel = M - 1;
#pragma unroll
        for (int m = M - 2; m >= 0; --m) {
          const bool take = (cand[m] != cand[m]) || (cand[m] >= v);
          v = take ? cand[m] : v;
          sel = take ? m : sel;
        }
        v = ccur[q] != 0.0f ? v : NEG;                    // a slot without a cell
        hist[(w * LANES + lane) & rmask] = v;
        if (w == D) vend = v;
        u64 word = 0;
#pragma unroll
        for (int pl = 0; pl < 4; ++pl)
          word |= (__builtin_amdgcn_ballot_w64(((sel >> pl) & 1) != 0) & ((1ull << LANES) - 1)) << (pl * LANES);
        mine = lane == q ? (word_t)word : mine;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the next lane reads the ring in a later step
      }
      if (lane < TCH) dec[c * TCH + lane] = mine;         // the chunk's words, side by side
#pragma unroll
      for (int q = 0; q < TCH; ++q)
#pragma unroll
        for (int m = 0; m < M; ++m) cur[q][m] = nxt[q][m];
#pragma unroll
      for (int q = 0; q < TCH; ++q) ccur[q] = cnxt[q];
    }
    if (lane == endlane) sh_score = vend;
  }
  __syncthreads();                                        // the score, and the decision words for wave 0

  // ---- outputs outside the path: -1 outside the rectangle or without a path, blank_steps 0 inside
  const float sc = sh_score;
  const bool ok = !(sc != sc) && sc != NEG;
  if (tid == 0) score[b] = sc;
  for (int s = tid; s < S; s += kTdtThreads)
    if (!ok || s < sb || s >= se) { fr_b[s] = -1; du_b[s] = -1; }
  for (int t = tid; t < T; t += kTdtThreads) bs_b[t] = (ok && t >= tb && t < te) ? 0 : -1;
  __syncthreads();                                        // the walk overwrites blank_steps entries written above
  if (!ok || tid >= 64) return;

  // ---- backtrace by wave 0 from the end slot to the origin (relative coordinates)
  const int lane = tid;
  const int nsteps = nch * TCH;                           // the words this launch wrote
  int rr = u.Sn - 1, t = u.Tn - 1;
  int k = D, l = rr & (LANES - 1);
  auto ld = [&](int idx) -> u64 {                         // the word of step idx + lane (0 outside the walk)
    const int i = idx + lane;
    const bool in = i >= 0 && i < nsteps;
    const word_t wv = dec[in ? i : 0];
    return in ? (u64)wv : 0ull;
  };
  int k0 = k - 63;
  u64 curw = ld(k0), nxtw = ld(k0 - 64);
  for (int guard = u.Sn + u.Tn; (rr > 0 || t > 0) && guard > 0; --guard) {
    if (k < k0) {
      curw = nxtw;
      k0 -= 64;
      nxtw = ld(k0 - 64);
    }
    const int idx = k - k0;
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)curw, idx);
    const unsigned hi = LANES == 16 ? (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(curw >> 32), idx) : 0u;
    const u64 word = ((u64)hi << 32) | lo;
    int sel = 0;
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) sel |= (int)((word >> (pl * LANES + l)) & 1ull) << pl;
    int dur = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) dur = sel == m ? mv.dur[m] : dur;
    if (sel >= M || t < dur || (sel < Dx && rr == 0)) break;   // not a move of this walk: see below
    if (sel < Dx) {                                       // token move out of row rr - 1 at frame t - dur
      rr -= 1; t -= dur; k -= 1 + dur; l = (l - 1) & (LANES - 1);
      if (lane == 0) { fr_b[sb + rr] = tb + t; du_b[sb + rr] = dur; }
    } else {                                              // blank move out of frame t - dur
      t -= dur; k -= dur;
      if (lane == 0) bs_b[tb + t] = dur;
    }
  }
  if (rr > 0 || t > 0) {   // the walk did not arrive (decision words that are no moves of this walk; believed unreachable with
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // a finite score): no partly filled alignment leaves the kernel
    for (int s = lane; s < S; s += 64) { fr_b[s] = -1; du_b[s] = -1; }
    for (int tt = lane; tt < T; tt += 64) bs_b[tt] = -1;
  }
}

}  // namespace

// r within the band kernels' lanes, the move counts of the entry point, and slot indices that stay 32-bit
int mi_band_viterbi_supported(int T, int S, int r, int N, int Ny) {
  const int lanes = band_lanes_for(r);
  if (!lanes || T < 1 || S < 0 || N < 1 || Ny < 1 || N + Ny > kVitMaxMoves) return 0;
  return ((uint64_t)S + T + 1 + 2 * TCH) * (uint64_t)(lanes * (N + Ny)) < (1ull << 31) ? 1 : 0;
}

size_t mi_band_viterbi_workspace_bytes(int B, int T, int S, int r, int N, int Ny) {
  if (B < 0 || !mi_band_viterbi_supported(T, S, r, N, Ny)) return 0;
  return vit_layout(B, T, S, band_lanes_for(r), N + Ny).total;
}

int mi_band_viterbi(const float* pxb, const float* pyb, const int32_t* ranges, const int32_t* boundary, const int32_t* tok, int N,
                    const int32_t* blk, int Ny, void* ws, size_t ws_bytes, float* score, int32_t* frames, int32_t* durations,
                    int32_t* blank_steps, int B, int T, int S, int r, hipStream_t st) {
  const char* what = "mutual_information_band_viterbi";
  if (B == 0) return FTR_OK;
  if (!mi_band_viterbi_supported(T, S, r, N, Ny)) {
    set_error("%s: T=%d S=%d r=%d N=%d Ny=%d is outside the kernel's domain (r <= 15, N + Ny <= %d)", what, T, S, r, N, Ny, kVitMaxMoves);
    return FTR_ERR_UNSUPPORTED;
  }
  if (tok[N - 1] > kVitMaxTok || blk[Ny - 1] > kVitMaxBlk) {
    set_error("%s: a token duration above %d or a blank duration above %d exceeds the ring of %d steps", what, kVitMaxTok, kVitMaxBlk, kVitDep);
    return FTR_ERR_UNSUPPORTED;
  }
  const int lanes = band_lanes_for(r), M = N + Ny;
  const VitLayout L = vit_layout(B, T, S, lanes, M);
  if (ws_bytes < L.total) {
    set_error("%s: workspace of %zu bytes is too small, %zu needed", what, ws_bytes, L.total);
    return FTR_ERR_INVALID_ARG;
  }
  const BandMoves mv = make_band_moves(tok, N, blk, Ny);
  float* wsf = static_cast<float*>(ws);
  void* wsd = static_cast<char*>(ws) + L.dec_off;
  dispatch_among<8, 16>(lanes, [&](auto ln) {
    constexpr int LN = decltype(ln)::value;
    dispatch_range<2, kVitMaxMoves>(M, [&](auto m) {
      hipLaunchKernelGGL((band_viterbi_kernel<LN, decltype(m)::value>), dim3(B), dim3(kTdtThreads), 0, st, pxb, pyb, ranges, boundary, mv,
                         wsf, static_cast<typename DecWord<LN>::type*>(wsd), score, frames, durations, blank_steps, L.o_per, L.c_per, L.c_off, L.steps, T, S, r);
    }, [] {});   // supported() admits no other count
  });
  return check_launch("band_viterbi");
}

}  // namespace ftr
