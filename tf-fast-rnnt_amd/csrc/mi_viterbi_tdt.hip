// csrc/mi_viterbi_tdt.hip -- best-path (Viterbi) alignment over the lattice of mi_tdt.hip (token-and-duration transducer;
// token_durations = (0,) is the multi-blank lattice of mi_multiblank.hip, (0,) / (1,) the ordinary one of mi_viterbi.hip),
// and its backtrace.  MI355X addition, no reference counterpart.
//
// Moves m = 0 .. M-1: the Dx token moves in list order, then the Dy blank moves in list order.  For every cell but
// (s_begin,t_begin)
//   cand[m] = p[src_m] + op_m[src_m]     one float32 add; src_m = (s-1, t-e_i) for a token move, (s, t-d_j) for a blank
//                                        move; -inf when src_m lies outside the boundary rectangle, whatever op holds
//   best = cand[M-1]; move = M-1
//   for m = M-2 .. 0:  take = (cand[m] != cand[m]) || (cand[m] >= best);  if (take) best = cand[m], move = m
//   p[s,t] = best
// p[s_begin,t_begin] = 0, score = p[s_end,t_end].  A NaN propagates, a tie goes to the lowest-index move.  Every value
// is one add per move and ordered selects, so any dependency-respecting order gives the same bits; with (0,) / (1,) the
// rule is mi_viterbi.hip's.
//
// Forward sweep: the row-per-lane sweep and the history ring of mi_rowlane.h, as mi_tdt.hip, every predecessor a ring
// read of thread tid - ds (ds = 1 token, 0 blank).  The chain is float32, so DEP = 32 with four waves is the 32 KB that
// mi_tdt.hip spends on two, and 32 meets every depth requirement stated there for blanks up to 32 and tokens up to 16.
//
// Decisions: the move index has 4 bits; one ballot per bit plane per wave and step = four 64-bit words per (block of 64
// rows, local step kl = t + lane), staged in LDS and stored once per chunk by 32 lanes (256 contiguous bytes).  Every
// word the backtrace uses is written by the same launch, so the workspace needs no initialisation.
//
// Backtrace, by wave 0 after a barrier: a token move of duration e lowers kl by 1 + e inside a block, a blank move of
// duration d by d, so the wave holds a window of 64 consecutive steps of its block (4 planes per lane, the next lower
// window in flight: a stride is at most 33) and walks it with readlane.  frames / durations are collected per block in
// registers (lane = row) and stored 64 at a time; blank_steps is first set to 0 on [t_begin,t_end) by the whole
// workgroup, then the walk overwrites the frames it leaves by a blank move.
#include "mi_rowlane.h"

namespace ftr {
namespace {
using namespace rowlane;

constexpr int QMAXBLK = 32;            // largest blank duration
constexpr int QDEP = 32;               // ring depth
typedef unsigned long long u64;

static_assert(QDEP >= QMAXBLK && QDEP > MAXTOK && QDEP > 2 * CH - 1 + MAXTOK && (QDEP & (QDEP - 1)) == 0, "ring depth");
static_assert(QMAXBLK + 1 <= 64, "a backtrace stride must stay inside the prefetched window");

__host__ __device__ inline int vt_blocks(int S) { return (S + 1 + 63) / 64; }
// local steps kl = t + lane of a block: 0 .. T + 63, plus the tail of the last chunk that touches them
__host__ __device__ inline size_t vt_steps_per_block(int T) { return (size_t)T + 1 + 63 + CH; }
inline int vt_waves(int S) { return vt_blocks(S) < MAXW ? vt_blocks(S) : MAXW; }

struct VtLayout { size_t dec_bytes, carry_off, total; };
inline VtLayout vt_layout(int B, int S, int T) {
  VtLayout L;
  L.dec_bytes = (size_t)B * vt_blocks(S) * vt_steps_per_block(T) * 4 * sizeof(u64);
  L.carry_off = L.dec_bytes;
  L.total = L.dec_bytes + (size_t)B * 2 * (T + 1) * sizeof(float);
  return L;
}

template <int M>
__global__ void __launch_bounds__(64 * MAXW) mi_viterbi_tdt_kernel(
    const float* __restrict__ px, const float* __restrict__ py, const int32_t* __restrict__ boundary, const Moves mv,
    u64* __restrict__ dec, float* __restrict__ carry, float* __restrict__ score, int32_t* __restrict__ frames,
    int32_t* __restrict__ durations, int32_t* __restrict__ blank_steps, int S, int T, int NW) {
  extern __shared__ float hist[];                     // [QDEP][blockDim.x]: every thread's values of the last QDEP steps
  __shared__ float cwin[CW];                         // wave 0: the strip below's top row around this chunk
  __shared__ u64 words[MAXW][CH][4];                // the decision bit planes of the current chunk
  __shared__ float sh_score;

  const int b = blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, w = tid >> 6;
  const Bound bd = load_boundary(boundary, b, S, T);
  const int Sn = bd.se - bd.sb + 1, Tn = bd.te - bd.tb + 1;
  const int T1 = T + 1;
  const int Dx = mv.Dx, Dy = M - mv.Dx;
  const float NEG = -__builtin_inff();
  int32_t* fr_b = frames + (size_t)b * S;
  int32_t* du_b = durations + (size_t)b * S;
  int32_t* bs_b = blank_steps + (size_t)b * T;

  if (Sn <= 0 || Tn <= 0) {                           // inverted rectangle: score 0 as the recursion's ans, no path
    if (tid == 0) score[b] = 0.0f;
    for (int s = tid; s < S; s += nthr) { fr_b[s] = -1; du_b[s] = -1; }
    for (int t = tid; t < T; t += nthr) bs_b[t] = -1;
    return;
  }

  const size_t xplane = (size_t)S * T1, yplane = (size_t)(S + 1) * T;
  const float* px_b = px + (size_t)b * Dx * xplane;
  const float* py_b = py + (size_t)b * Dy * yplane;
  const size_t KW = vt_steps_per_block(T);
  const int NG = vt_blocks(S);
  u64* dec_b = dec + (size_t)b * NG * KW * 4;
  const float* safe_f = reinterpret_cast<const float*>(dec_b);   // where a masked lane loads from: always mapped
  if (tid == 0) sh_score = __builtin_nanf("");                    // always overwritten: the loop covers (Sn-1, Tn-1)
  __syncthreads();

  const int nst = strips(Sn, NW);
  const int below = tid > 0 ? tid - 1 : 0;            // the thread that holds the row below
  const int sback = lane == 0 ? CH : 1;              // ... and how many steps ago it was on this column
  for (int j = 0; j < nst; ++j) {
    const Strip<float> s(bd, j, NW, w, lane, b, carry, T1, false);
    const int r = s.r, skew = s.skew, s_act = s.s_act;
    const bool rowok = s.rowok, want_cin = s.want_cin, give_carry = s.give_carry && lane == 63;
    u64* dec_g = dec_b + (size_t)(j * NW + w) * KW * 4;

    // move m's operand at the predecessor of this lane's cell at relative column t
    auto operand = [&](int m, int t) -> const float* {
      const int t_act = bd.tb + t - mv.dur[m];
      return m < Dx ? px_b + m * xplane + (size_t)(s_act - 1) * T1 + t_act
                    : py_b + (m - Dx) * yplane + (size_t)s_act * T + t_act;
    };

    // every load is unconditional (a masked lane reads the workspace instead), so chunk c + 1's stay in flight while
    // chunk c computes; every unmasked index lies inside the boundary rectangle, which load_boundary clamps to the lattice
    auto load = [&](Ops<M, float>& o, int c) {
      {
        const int t = CH * c - MAXTOK + lane;
        const bool ok = want_cin && lane < CW && t >= 0 && t < Tn;
        o.cin = *(ok ? s.carry_in + t : safe_f);
        o.cin = ok ? o.cin : NEG;
      }
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int t = CH * c + q - skew;
        const bool valid = rowok && t >= 0 && t < Tn;
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const bool ok = valid && t >= mv.dur[m] && (m >= Dx || r >= 1);
          o.w[m][q] = *(ok ? operand(m, t) : safe_f);
        }
      }
    };

    auto chunk = [&](const Ops<M, float>& o, int c) {
      if (want_cin) {
        if (lane < CW) cwin[lane] = o.cin;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int k = CH * c + q;
        const int t = k - skew;
        const bool valid = rowok && t >= 0 && t < Tn;
        float cand[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const int e = mv.dur[m];
          const bool sym = m < Dx;
          const bool ok = valid && t >= e && (!sym || r >= 1);
          float src = hist[(size_t)((k - e - (sym ? sback : 0)) & (QDEP - 1)) * nthr + (sym ? below : tid)];
          if (want_cin && sym) {                      // uniform per wave; wave 0's lane 0 is on column t = k
            const float cv = cwin[MAXTOK + q - e];
            src = tid == 0 ? cv : src;
          }
          cand[m] = ok ? src + o.w[m][q] : NEG;
        }
        float v = cand[M - 1];
        int sel = M - 1;
#pragma unroll
        for (int m = M - 2; m >= 0; --m) {
          const bool take = (cand[m] != cand[m]) || (cand[m] >= v);
          v = take ? cand[m] : v;
          sel = take ? m : sel;
        }
        if (r == 0 && t == 0) v = 0.0f;
        if (valid) {
          if (r == Sn - 1 && t == Tn - 1) sh_score = v;
          if (give_carry) s.carry_out[t] = v;           // the strip's top row, for the strip above
        }
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) {
          const u64 word = __builtin_amdgcn_ballot_w64(((sel >> pl) & 1) != 0);
          if (lane == 0) words[w][q][pl] = word;
        }
        hist[(size_t)(k & (QDEP - 1)) * nthr + tid] = v;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the upper lane reads it in a later step
      }
      if (lane < 4 * CH) {                           // the chunk's 32 words, contiguous in the workspace
        const int kl = CH * c - E * w + (lane >> 2);
        if (kl >= 0 && kl < (int)KW) dec_g[(size_t)kl * 4 + (lane & 3)] = words[w][lane >> 2][lane & 3];
      }
    };

    run_chunks<Ops<M, float>>(s.nch, s.active, load, chunk);
  }

  // ---- outputs outside the path: -1 outside the rectangle or without a path, blank_steps 0 inside
  const float sc = sh_score;
  const bool ok = !(sc != sc) && sc != NEG;
  if (tid == 0) score[b] = sc;
  for (int s = tid; s < S; s += nthr)
    if (!ok || s < bd.sb || s >= bd.se) { fr_b[s] = -1; du_b[s] = -1; }
  for (int t = tid; t < T; t += nthr) bs_b[t] = (ok && t >= bd.tb && t < bd.te) ? 0 : -1;
  __syncthreads();                                    // the walk overwrites blank_steps entries written above
  if (!ok || w != 0) return;

  // ---- backtrace by wave 0 from (Sn-1, Tn-1) to the origin (relative coordinates)
  int r = Sn - 1, t = Tn - 1;
  int g = r >> 6, l = r & 63;
  u64 cur[4], nxt[4];
  auto ld = [&](u64* dst, int gg, int idx) {          // planes of step idx + lane of block gg (0 outside the block)
    const int i = idx + lane;
    const bool in = i >= 0 && i < (int)KW;
    const u64* src = dec_b + ((size_t)gg * KW + (in ? i : 0)) * 4;
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) dst[pl] = in ? src[pl] : 0ull;
  };
  int kl = t + l;
  int k0 = kl - 63;
  ld(cur, g, k0); ld(nxt, g, k0 - 64);
  int frv = -1, duv = -1;                             // lane i: frame and duration of row 64 g + i
  for (int guard = Sn + Tn; (r > 0 || t > 0) && guard > 0; --guard) {
    if (kl < k0) {
#pragma unroll
      for (int pl = 0; pl < 4; ++pl) cur[pl] = nxt[pl];
      k0 -= 64;
      ld(nxt, g, k0 - 64);
    }
    const int idx = kl - k0;
    int sel = 0;
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) {
      const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)cur[pl], idx);
      const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(cur[pl] >> 32), idx);
      const u64 word = ((u64)hi << 32) | lo;
      sel |= (int)((word >> l) & 1ull) << pl;
    }
    int dur = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) dur = sel == m ? mv.dur[m] : dur;
    if (sel >= M || t < dur || (sel < Dx && r == 0)) break;   // not a move of this lattice: unreachable on a finite path
    if (sel < Dx) {                                   // token move out of row r - 1 at frame t - dur
      const int tp = t - dur;
      if (l > 0 && lane == l - 1) { frv = tp + bd.tb; duv = dur; }
      r -= 1; t = tp; kl -= 1 + dur; l -= 1;
      if (l < 0) {                                    // into the block below: flush this block's rows, then row r there
        if (64 * g + lane < Sn - 1) { fr_b[bd.sb + 64 * g + lane] = frv; du_b[bd.sb + 64 * g + lane] = duv; }
        frv = lane == 63 ? tp + bd.tb : -1;
        duv = lane == 63 ? dur : -1;
        g -= 1; l = 63;
        kl = t + l; k0 = kl - 63;
        ld(cur, g, k0); ld(nxt, g, k0 - 64);
      }
    } else {                                          // blank move out of frame t - dur
      t -= dur; kl -= dur;
      if (lane == 0) bs_b[bd.tb + t] = dur;
    }
  }
  if (64 * g + lane < Sn - 1) { fr_b[bd.sb + 64 * g + lane] = frv; du_b[bd.sb + 64 * g + lane] = duv; }
}

}  // namespace

size_t mi_viterbi_tdt_workspace_bytes(int B, int S, int T) {
  if (B < 0 || S < 0 || T < 0) return 0;
  return vt_layout(B, S, T).total;
}

int mi_viterbi_tdt(const float* px, const float* py, const int32_t* boundary, const int32_t* token_durations, int Dx,
                   const int32_t* blank_durations, int Dy, void* ws, size_t ws_bytes, float* score, int32_t* frames,
                   int32_t* durations, int32_t* blank_steps, int B, int S, int T, hipStream_t st) {
  const char* what = "mutual_information_viterbi_tdt";
  const VtLayout L = vt_layout(B, S, T);
  int rc;
  if (launch_done(what, B, S, T, ws_bytes, L.total, "bytes", &rc)) return rc;
  const Moves mv = make_moves(token_durations, Dx, blank_durations, Dy);
  const int NW = vt_waves(S);
  u64* dec = static_cast<u64*>(ws);
  float* carry = reinterpret_cast<float*>(static_cast<char*>(ws) + L.carry_off);
  const size_t lds = (size_t)QDEP * 64 * NW * sizeof(float);
  dispatch_range<2, MAXM_ALIGN>(Dx + Dy, [&](auto m) {
    hipLaunchKernelGGL((mi_viterbi_tdt_kernel<decltype(m)::value>), dim3(B), dim3(64 * NW), lds, st, px, py, boundary, mv,
                       dec, carry, score, frames, durations, blank_steps, S, T, NW);
  }, [] {});   // the entry points admit no other arity
  return check_launch(what);
}

}  // namespace ftr
