// csrc/mi_rowlane.h -- the row-per-lane sweep that the duration-lattice kernels share: mi_multiblank.hip, mi_tdt.hip and
// mi_viterbi_tdt.hip.  Everything below is stated here once; the kernel files hold what a cell computes and stores.
//
// Layout.  One workgroup per utterance, NW waves.  Relative row r (backward: counted down from s_end) lives in wave
// (r / 64) % NW, lane r % 64 of strip r / (64 NW).  Wave w at step k handles column t = k - lane - E w, E = 64 + CH - 1,
// so the row below a lane is one step ahead of it and the wave below one chunk of CH steps.  Chunks run between
// barriers; the operands of chunk c + 1 are loaded (unconditionally: a masked lane reads the workspace instead) while
// chunk c computes.  The top row of a strip goes to the next strip through `carry` in the workspace.
//
// The history ring.  Every lane keeps its last DEP values (DEP a power of two) in LDS, hist[step & (DEP-1)][thread],
// writes step k after it has read for step k, and fences the wave after the write.  A predecessor is a ring read:
//   * own lane, blank move d: step k - d of the thread itself.  The slot is next written at step k - d + DEP >= k, after
//     the read:                                                                                     DEP >= d_max.
//   * lane >= 1, token move e: the row below is thread tid - 1 of the same wave, which was on column t - e at step
//     k - 1 - e.  The wave wrote that step earlier in program order (LDS is in order per wave) and overwrites it at
//     step k - 1 - e + DEP > k - 1:                                                                 DEP > e_max.
//   * lane 0 of wave w > 0, token move e: the row below is lane 63 of wave w - 1, thread tid - 1 all the same; with the
//     skew E it was on column t - e at step k - CH - e.  Both waves run chunk c between the same two barriers, so that
//     step lies in a chunk that is complete, and wave w - 1 writes up to step CH c + CH - 1 meanwhile without reaching
//     its slot:                                                                                     DEP > 2 CH - 1 + e_max.
//   * lane 0 of wave 0 in a strip above the first: the row below is the strip below's top row, complete in `carry`.  The
//     CH + MAXTOK values a chunk can ask for (columns CH c - MAXTOK .. CH c + CH - 1) are loaded with the operands by
//     lanes 0 .. CW - 1 and staged in LDS (`cwin`); thread 0 takes its token predecessors from there.
// mi_tdt.hip picks DEP at launch from the move list (ring_depth), mi_viterbi_tdt.hip fixes it (static_assert there).
// The ring reads and writes, the masked chunk load and the log-add stay written out in the kernels: moved behind
// functions here they changed the register allocation of these register-bound kernels (profiles/
// rowlane_refactor_resources.md); for the same reason mi_tdt.hip writes the fields of Strip out.
// mi_multiblank.hip reads only its blank predecessors from the ring (first rule); its symbol predecessor travels by a
// DPP shift and one LDS slot per wave and chunk, see there.
#pragma once
#include <type_traits>
#include "ftr_common.h"
#include "launch.h"

namespace ftr {
namespace rowlane {

constexpr int CH = 8;                  // steps per chunk
constexpr int E = 64 + CH - 1;         // skew between consecutive waves
constexpr int MAXW = 4;                // waves per workgroup
constexpr int MAXM = 10;               // moves (Dx + Dy) of the recursion (mi_tdt.hip: five of each kind, as the band's)
constexpr int MAXM_ALIGN = 9;          // ... and of the alignment (mi_viterbi_tdt.hip)
constexpr int MAXTOK = 16;             // largest token duration
constexpr int CW = CH + MAXTOK;        // carry window of a chunk

// moves 0 .. Dx-1 are the token moves (px planes), Dx .. Dx+Dy-1 the blank moves (py planes); unused slots hold 1
struct Moves { int dur[MAXM]; int Dx; };
inline Moves make_moves(const int32_t* token_durations, int Dx, const int32_t* blank_durations, int Dy) {
  Moves mv;
  for (int m = 0; m < MAXM; ++m) mv.dur[m] = m < Dx ? token_durations[m] : (m < Dx + Dy ? blank_durations[m - Dx] : 1);
  mv.Dx = Dx;
  return mv;
}

// smallest ring the rules above allow for a recursion whose blank durations stay <= 16: the power of two > 2 CH - 1 + e_max
inline int ring_depth(int emax) { return emax == 0 ? 16 : 32; }
// waves of a float64 ring of that depth: 32 KB of LDS either way
inline int ring_waves_f64(int S, int depth) {
  const int cap = depth > 16 ? MAXW / 2 : MAXW;
  const int blocks = (S + 1 + 63) / 64;
  return blocks < cap ? blocks : cap;
}

// workspace of a float64 recursion, in doubles: p [B,S+1,T+1], ans [B], carry [B,2,T+1]
struct F64Layout { size_t p_off, ans_off, carry_off, total; };
inline F64Layout f64_layout(int B, int S, int T) {
  F64Layout L;
  L.p_off = 0;
  L.ans_off = (size_t)B * (S + 1) * (T + 1);
  L.carry_off = L.ans_off + (size_t)B;
  L.total = L.carry_off + (size_t)B * 2 * (T + 1);
  return L;
}
inline size_t f64_workspace_floats(int B, int S, int T) {
  if (B < 0 || S < 0 || T < 0) return 0;
  return 2 * f64_layout(B, S, T).total;
}

// What every launcher checks first.  True: nothing to launch, return *rc.  `have` / `need` in `unit` ("floats", "bytes").
inline bool launch_done(const char* what, int B, int S, int T, size_t have, size_t need, const char* unit, int* rc) {
  *rc = FTR_OK;
  if (B == 0) return true;
  if (have < need) {
    set_error("%s: workspace of %zu %s is too small, %zu needed", what, have, unit, need);
    *rc = FTR_ERR_INVALID_ARG;
    return true;
  }
  if ((size_t)(S + 1) * (size_t)(T + 1) >= (1ull << 31)) {
    set_error("%s: one utterance's lattice (S=%d, T=%d) exceeds 2^31 cells", what, S, T);
    *rc = FTR_ERR_UNSUPPORTED;
    return true;
  }
  return false;
}

// exp(v) for v a float64 log-quantity that is <= ~0 where it matters: the float32 exp2 unit
__device__ __forceinline__ float exp_of(double v) { return __builtin_amdgcn_exp2f((float)v * kLog2e); }

inline __device__ int strips(int Sn, int NW) { return (Sn + 64 * NW - 1) / (64 * NW); }   // of 64 NW rows

// The geometry of strip j for this thread.  V: the type of the carried values.
template <typename V>
struct Strip {
  int Sn, Tn, nst;       // rows and columns of the boundary rectangle, strips
  int nwact, nch;        // waves that hold rows of this strip, chunks of its sweep
  bool active;           // this wave is one of them
  int r;                 // relative row
  bool rowok;
  int skew;              // t = k - skew
  int s_act;             // the row in the lattice
  const V* carry_in;     // the top row of strip j - 1
  V* carry_out;
  bool want_cin;         // wave 0 of a strip above the first
  bool give_carry;       // the top wave of a strip below the last

  __device__ __forceinline__ Strip(const Bound& bd, int j, int NW, int w, int lane, int b, V* carry, int T1, bool BWD) {
    Sn = bd.se - bd.sb + 1; Tn = bd.te - bd.tb + 1;
    const int R = 64 * NW;                              // rows per strip
    nst = strips(Sn, NW);
    const int rows = min(R, Sn - j * R);
    nwact = (rows + 63) >> 6;
    const int nk = Tn + 63 + E * (nwact - 1);
    nch = (nk + CH - 1) / CH;
    active = w < nwact;
    r = j * R + 64 * w + lane;
    rowok = r < Sn;
    skew = lane + E * w;
    s_act = BWD ? bd.se - r : bd.sb + r;
    carry_in = carry + ((size_t)b * 2 + ((j + 1) & 1)) * T1;
    carry_out = carry + ((size_t)b * 2 + (j & 1)) * T1;
    want_cin = active && w == 0 && j > 0;
    give_carry = active && w == NW - 1 && j + 1 < nst;
  }
  __device__ __forceinline__ bool valid(int t) const { return rowok && t >= 0 && t < Tn; }
};

// load(ops, c) fills one operand set for chunk c, chunk(ops, c) computes it: two sets, the next chunk's loads in flight
template <typename Ops, typename Load, typename Chunk>
__device__ __forceinline__ void run_chunks(int nch, bool active, Load load, Chunk chunk) {
  Ops A0, B0;
  load(A0, 0);
  for (int c = 0; c < nch; c += 2) {
    load(B0, c + 1);
    if (active) chunk(A0, c);
    __syncthreads();
    if (c + 1 >= nch) break;
    load(A0, c + 2);
    if (active) chunk(B0, c + 1);
    __syncthreads();
  }
}

// operands of one chunk of the two kernels whose predecessors all come from the ring (mi_tdt.hip, mi_viterbi_tdt.hip)
template <int M, typename V>
struct Ops {
  float w[M][CH];
  V pc[CH];    // backward: p of the cell
  V cin;       // wave 0 of a strip above the first: lane l < CW holds the strip below's top row at t = CH c - MAXTOK + l
};

}  // namespace rowlane
}  // namespace ftr
