// csrc/mi_band_common.h -- the band geometry and the chain step of the pruned loss's recursion, stated once (gfx950).
//
// Three implementations run the recursion on the band itself: mi_band_kernel (LDS resident) and mi_band_stream_kernel
// (global workspace) of mi_band.hip, and the band_seg_* kernels of mi_band_seg.hip.  They differ in where the wavefront-ordered
// arrays live and in how the walk is scheduled; what a band cell is, which of its transitions exist, where its operands go
// and what one step of a float32 chain computes is the same for all of them and is defined HERE only:
//
//   band cell (t,k)  <->  lattice cell (s,t), s = l + k,  l = ranges[b,t,0] the band start of column t   (monotone along t)
//   chain A's slot of a cell: walk step dgA = (s-sb)+(t-tb) [modified: t-tb], lane (s-sb) mod LANES, operands = the
//                             transitions INTO the cell:   OX = px(s-1, t [t-1 if modified]), OY = py(s, t-1)
//   chain B's slot:           walk step dgB = (se-s)+(te-t) [te-t],          lane (se-s) mod LANES, operands = the
//                             transitions OUT of the cell: OX = px(s,t), OY = py(s,t)
//   a transition that does not exist, leaves the rectangle or leaves the band is kNeg; the origin (chain A) and the end
//   cell (chain B) start their chain through OY = 0 (the lane starts from 0).
// The band start of a column is passed in by the caller (lo[] in LDS in the chain kernels, global reads in the segments):
// l0 / lm / lp are the band starts of columns t, t - 1 (t > tb) and t + 1 (t < te).
#pragma once
#include "ftr_common.h"

namespace ftr {

// ---------------------------------------------------------------------------------------- host: lanes, LDS ceiling
// 8-lane chains while the band is at most 7 rows wide, 16-lane chains up to 15 rows (r + 1 lanes: the modified type may have
// r + 1 cells on its last walk step, see BandGeom::end_above); 0: outside the band kernels' domain
inline int band_lanes_for(int r) { return r < 1 ? 0 : (r <= 7 ? 8 : (r <= 15 ? 16 : 0)); }
// the dynamic-LDS limit of the band kernels: 156 KB, not 160 -- they also have a few bytes of static LDS (__syncthreads_or)
constexpr size_t kBandLdsCeiling = 156 * 1024;

// ---------------------------------------------------------------------------------------- 16-lane DPP rows
template <int N>
__device__ __forceinline__ float row16_ror(float v) {   // lane i of each 16-lane row receives lane (i-N) mod 16
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xf, 0xf, false));
}
template <int N>
__device__ __forceinline__ double row16_ror(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x120 + N, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x120 + N, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float row16_max(float v) {      // all-reduce over the 16 lanes of a DPP row
  v = fmaxf(v, row16_ror<8>(v)); v = fmaxf(v, row16_ror<4>(v));
  v = fmaxf(v, row16_ror<2>(v)); v = fmaxf(v, row16_ror<1>(v));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
  v += row16_ror<8>(v); v += row16_ror<4>(v); v += row16_ror<2>(v); v += row16_ror<1>(v);
  return v;
}

// ---------------------------------------------------------------------------------------- the utterance
struct BandUtt { Bound bd; int Sn, Tn, D; bool degenerate; };   // D: walk steps after the first cell
template <bool MOD>
__device__ __forceinline__ BandUtt band_utt(const int32_t* boundary, int b, int S, int T) {
  BandUtt u;
  u.bd = load_boundary(boundary, b, S, T);
  u.Sn = u.bd.se - u.bd.sb + 1; u.Tn = u.bd.te - u.bd.tb + 1;
  u.degenerate = u.Sn <= 0 || u.Tn <= 0 || u.Tn == 1;
  u.D = (MOD ? 0 : (u.Sn - 1)) + (u.Tn - 1);
  return u;
}
// ans of a degenerate rectangle (zero occupancies): empty: 0 (mi_wave_bidir.hip); a single column has no frame inside the
// rectangle: only the one-cell lattice has a path (no transitions at all)
__device__ __forceinline__ float band_degenerate_ans(const BandUtt& u) {
  return (u.Sn <= 0 || u.Tn <= 0) ? 0.0f : ((u.Sn == 1) ? 0.0f : -INFINITY);
}

// ---------------------------------------------------------------------------------------- geometry and transition rule
// rowA / rowB: the rows at which chain A's and chain B's parts of the caller's wavefront-ordered arrays begin (the three
// layouts differ in nothing else).  lo_te: the band start of column t_end.
template <bool MOD, int LANES>
struct BandGeom {
  int r, sb, tb, se, te, rowA, rowB;
  // Column t_end has no frame: its cells are where the last frame's transitions lead.  For the regular type that is the
  // last frame's band again (py moves along a row; px inside column t_end is masked by fix_for_boundary); for the modified
  // type px moves up one row AND one column, so the END CELL may sit one row above that band (s_end = lo + r) and still be
  // reached -- by the last frame's top px.  (Any other cell of column t_end is a dead end and needs no slot.)
  bool end_above;
  __device__ BandGeom(int r_, const Bound& bd, int lo_te, int rowA_, int rowB_)
      : r(r_), sb(bd.sb), tb(bd.tb), se(bd.se), te(bd.te), rowA(rowA_), rowB(rowB_), end_above(MOD && bd.se == lo_te + r_) {}
  __device__ bool in_band(int s, int t, int l) const { return (s >= l && s <= l + r - 1) || (end_above && t == te && s == se); }
  __device__ int dgA(int s, int t) const { return MOD ? (t - tb) : (s - sb) + (t - tb); }
  __device__ int dgB(int s, int t) const { return MOD ? (te - t) : (se - s) + (te - t); }
  __device__ int laneA(int s) const { return (s - sb) & (LANES - 1); }
  __device__ int laneB(int s) const { return (se - s) & (LANES - 1); }
  __device__ int slotA(int s, int t) const { return (rowA + dgA(s, t)) * LANES + laneA(s); }
  __device__ int slotB(int s, int t) const { return (rowB + dgB(s, t)) * LANES + laneB(s); }
  // which of the four transitions of cell (s, t) exist: into it by px / py, and (for t < te) out of it by px / py
  __device__ bool x_in(int s, int t, int l0, int lm) const {
    const int tx = MOD ? t - 1 : t;
    return s - 1 >= sb && tx >= tb && tx <= te - 1 && in_band(s - 1, tx, MOD ? lm : l0);
  }
  __device__ bool y_in(int s, int t, int lm) const { return t - 1 >= tb && in_band(s, t - 1, lm); }
  __device__ bool x_out(int s, int t, int l0, int lp) const {
    const int tnx = MOD ? t + 1 : t;
    return s + 1 <= se && tnx <= te && in_band(s + 1, tnx, MOD ? lp : l0);
  }
  __device__ bool y_out(int s, int t, int lp) const { return in_band(s, t + 1, lp); }
};

// band value at lattice cell (s, t), frame t < te, band start l: log2 domain, shifted
__device__ __forceinline__ float band_at(const float* __restrict__ src, float c2, int r, int s, int t, int l) {
  return __builtin_fmaf(src[(size_t)t * r + (s - l)], kLog2e, -c2);
}
// operands of band cell (s, t): (ax, ay) = the transitions INTO it (chain A's slot), (bx, by) = the transitions OUT of it
// (chain B's slot); pxu / pyu: the utterance's band arrays
template <bool MOD, int LANES>
__device__ __forceinline__ void band_operands_in(const BandGeom<MOD, LANES>& g, const float* __restrict__ pxu, const float* __restrict__ pyu,
                                                 float cx2, float cy2, int s, int t, int l0, int lm, float& ax, float& ay) {
  ax = kNeg; ay = kNeg;
  if (g.x_in(s, t, l0, lm)) ax = band_at(pxu, cx2, g.r, s - 1, MOD ? t - 1 : t, MOD ? lm : l0);
  if (g.y_in(s, t, lm)) ay = band_at(pyu, cy2, g.r, s, t - 1, lm);
  if (s == g.sb && t == g.tb) ay = 0.0f;                             // origin trick
}
template <bool MOD, int LANES>
__device__ __forceinline__ void band_operands_out(const BandGeom<MOD, LANES>& g, const float* __restrict__ pxu, const float* __restrict__ pyu,
                                                  float cx2, float cy2, int s, int t, int l0, int lp, float& bx, float& by) {
  bx = kNeg; by = kNeg;
  if (t <= g.te - 1) {
    if (g.x_out(s, t, l0, lp)) bx = band_at(pxu, cx2, g.r, s, t, l0);
    if (g.y_out(s, t, lp)) by = band_at(pyu, cy2, g.r, s, t, l0);
  }
  if (s == g.se && t == g.te) by = 0.0f;                             // chain B's origin is the end cell
}

// an operand on its way into a slot: NaN accounting (nan_acc collects the largest |bits| seen) and the clamp to kNeg
__device__ __forceinline__ float band_clamp(float v, unsigned& nan_acc) {
  nan_acc = max(nan_acc, __float_as_uint(v) & 0x7fffffffu);
  return fmaxf(v, kNeg);
}
__device__ __forceinline__ void band_put(float2* O, int slot, float x, float y, unsigned& nan_acc) {
  O[slot] = make_float2(band_clamp(x, nan_acc), band_clamp(y, nan_acc));
}
__device__ __forceinline__ bool band_saw_nan(unsigned nan_acc) { return nan_acc > 0x7f800000u; }

// the occupancies of the two transitions out of cell (s, t), t < te, from the flow arrays the chain kernels leave behind:
// a transition whose source cell lies in front of the cut (chain A's step jm) was handled by chain B (flow kept at the source
// cell), one whose source lies on or behind the cut by chain A (flow kept at the destination cell)
template <bool MOD, int LANES>
__device__ __forceinline__ void band_cell_flows(const BandGeom<MOD, LANES>& g, const float2* O2, int jm, int s, int t, int l0, int lp,
                                                float& fx, float& fy) {
  if (g.dgA(s, t) < jm) { const float2 f = O2[g.slotA(s, t)]; fx = f.x; fy = f.y; }
  else {
    if (g.x_out(s, t, l0, lp)) fx = O2[g.slotB(s + 1, MOD ? t + 1 : t)].x;
    if (g.y_out(s, t, lp)) fy = O2[g.slotB(s, t + 1)].y;
  }
}

// ---------------------------------------------------------------------------------------- shift sample, prologue
// This thread's part of the fixed sample behind the utterance's shift constants (ftr_common.h, Shift): 2048 entries of each
// band array, N per thread of THREADS; the sums and counts of the finite ones come back summed over the wave.
template <int THREADS, int N>
__device__ __forceinline__ void band_shift_sample(const float* __restrict__ pxu, const float* __restrict__ pyu, int tb, int te, int r, int tid,
                                                  float& sx, float& nx, float& sy, float& ny) {
  static_assert(THREADS * N == 2048, "the sample is 2048 entries whatever the workgroup");
  const unsigned nfr = (unsigned)(te - tb) * (unsigned)r;
  sx = 0.0f; nx = 0.0f; sy = 0.0f; ny = 0.0f;
  float vx[N], vy[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const unsigned i = (unsigned)tb * (unsigned)r + __umulhi((unsigned)(tid + THREADS * u) * 0x9E3779B1u, nfr);
    vx[u] = pxu[i]; vy[u] = pyu[i];
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    if (shift_sample_ok(vx[u])) { sx += vx[u]; nx += 1.0f; }
    if (shift_sample_ok(vy[u])) { sy += vy[u]; ny += 1.0f; }
  }
  sx = wave_sum_dpp(sx); nx = wave_sum_dpp(nx); sy = wave_sum_dpp(sy); ny = wave_sum_dpp(ny);
}

// an utterance that is answered without a recursion: zero occupancies, ans = a (workgroup of THREADS, all of it leaves)
template <int THREADS>
__device__ __forceinline__ void band_answer_flat(float* gx_g, float* gy_g, size_t cells_g, int tid, float* ans_b, float a) {
  for (size_t i = tid; i < cells_g; i += THREADS) { gx_g[i] = 0.0f; gy_g[i] = 0.0f; }
  if (tid == 0) *ans_b = a;
}
// lo[t], 0 <= t <= T: band start per lattice column; the column t_end has no frame of its own, it continues the last frame's band
template <int THREADS>
__device__ __forceinline__ void band_load_lo(int* lo, const int32_t* __restrict__ rg, int T, int te, int r, int tid) {
  for (int t0 = 0; t0 <= T; t0 += 4 * THREADS) {               // four independent loads in flight per lane
    int v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int t = t0 + u * THREADS + tid; v[u] = (t <= T) ? rg[(size_t)min(t, te - 1) * r] : 0; }
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int t = t0 + u * THREADS + tid; if (t <= T) lo[t] = v[u]; }
  }
}
// the one precondition the wavefront order rests on: the band start never decreases along t (two cells of one walk step
// would otherwise share a slot).  Workgroup-wide (a barrier); the caller answers a violation loudly: ans = NaN, zero occupancies.
template <int THREADS>
__device__ __forceinline__ bool band_lo_decreases(const int* lo, int tb, int te, int tid) {
  int bad = 0;
  for (int t = tb + 1 + tid; t < te; t += THREADS) bad |= (lo[t] < lo[t - 1]);
  return __syncthreads_or(bad) != 0;
}

// ---------------------------------------------------------------------------------------- the float32 chain (mi_band.hip)
// One forward step: val <- logadd(dpp(val) + OX, val + OY); returns the split ratio G of the cell (the share of the px side).
__device__ __forceinline__ float chain_fwd(float& val, float2 o) {
  const float up = row16_ror<1>(val);
  const float a_ = up + o.x, b_ = val + o.y;
  const float d = a_ - b_;
  const float ex = __builtin_amdgcn_exp2f(-__builtin_fabsf(d));
  val = fmaxf(a_, b_) + __builtin_amdgcn_logf(1.0f + ex);
  const float rc = __builtin_amdgcn_rcpf(1.0f + ex);
  return (d >= 0.0f) ? rc : ex * rc;
}
// Renormalisation ("frames", as in mi_wave_bidir.hip): the chain's values are brought back to the neighbourhood of zero by an
// integer shift, the same for all lanes of the chain (a uniform shift of an anti-diagonal changes no split ratio), so that
// float32 keeps its resolution whatever the magnitude of the log-probabilities -- the static shift only removes what the
// band's MEAN transition predicts.  snap: this lane's value some steps ago (no shift in between: the same frame), so that
// the four dependent DPP maxima are off the chain; frame = what has been subtracted so far, added back on the cut.
__device__ __forceinline__ void chain_renorm(float& val, float& frame, float snap) {
  const float mx = row16_max(snap);
  const float st = (mx > kNegThresh) ? __builtin_rintf(mx) : 0.0f;
  val -= st; frame += st;
}
// The cut, wave 0 after the forward walk: p + q per cut cell (keyed by s mod 16: at most one cut cell per residue), ans, and
// the occupancy this lane injects at its cut cell (the return value).  LDS, 16 entries each: cutSA / cutSB (lattice row of each
// lane's cut cell, -1: none), cutA / cutB / occ (adjacent).  The five pointers are passed as the kernels hold them: deriving
// cutSB, cutB and occ in here costs mi_band_stream_kernel 10 VGPRs.
__device__ __forceinline__ float chain_cut(float val, float frame, int lane, int l16, int lg, bool isB, const int* cutSA, const int* cutSB,
                                           float* cutA, float* cutB, float* occ, bool poisoned, double shift_back, float* ans_b) {
  if (lane < 48) cutA[lane] = kNeg;                         // cutA, cutB, occ
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const int scut = (isB ? cutSB : cutSA)[lg];               // lattice row of this lane's cut cell
  if (scut >= 0) (isB ? cutB : cutA)[scut & 15] = val;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  {
    // both chains' frames: chain A's lanes hold theirs in DPP rows 0 / 2, chain B's in rows 1 / 3
    const float frA = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, frame), 0));
    const float frB = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, frame), 16));
    const float v = cutA[l16] + cutB[l16];
    const float m = row16_max(v);
    const float e = exp2f(v - m);
    const float sum = row16_sum(e);
    const float total = m + log2f(sum);
    const bool dead = !(total > kNegThresh);
    if (lane < 16) occ[lane] = (dead || poisoned) ? 0.0f : e / sum;
    if (lane == 0) *ans_b = poisoned ? __builtin_nanf("") : (dead ? -INFINITY : (float)(((double)total + (double)frA + (double)frB + shift_back) * 0.6931471805599453));
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  return (scut >= 0) ? occ[scut & 15] : 0.0f;
}
// One flow step: what enters the cell (from the cyclically previous lane's x and this lane's y, plus inj on the chain's FIRST
// step) is returned for the cell's slot and pushed on with the other chain's ratio g.
template <bool FIRST>
__device__ __forceinline__ float2 chain_flow(float& xo, float& yo, float g, float inj) {
  const float xin = row16_ror<1>(xo), yin = yo;
  float pg = xin + yin;
  if (FIRST) pg += inj;
  xo = pg * g; yo = pg - xo;
  return make_float2(xin, yin);
}

}  // namespace ftr
