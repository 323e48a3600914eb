// csrc/mi_tdt.hip -- the lattice recursion of the token-and-duration transducer (TDT; Xu et al., "Efficient Sequence
// Transduction by Jointly Predicting Tokens and Durations", ICML 2023; MI355X addition, no reference counterpart): every
// move, symbol or blank, also says how many frames it advances.
//
//   p[s,t] = logadd( (+)_i p[s-1,t-e_i] + px[i,s-1,t-e_i],  (+)_j p[s,t-d_j] + py[j,s,t-d_j] ),   p[s_begin,t_begin] = 0
//   ans    = p[s_end,t_end]
//   px_grad[i,s,t] = exp(p[s,t] + px[i,s,t] + q[s+1,t+e_i] - ans)     (occupancy of symbol move i out of (s,t))
//   py_grad[j,s,t] = exp(p[s,t] + py[j,s,t] + q[s,t+d_j]   - ans)     (occupancy of blank move j out of (s,t))
// with e_i the Dx token durations (0..16), d_j the Dy blank durations (1..16), Dx + Dy <= 10, a term whose source lies
// outside the boundary rectangle absent, and q the same recursion run from (s_end,t_end) backwards.  token_durations =
// (0,) is the multi-blank recursion of mi_multiblank.hip, and this file follows it: one kernel for both directions (the
// backward pass is the forward pass in mirrored coordinates r = s_end - s, t = t_end - t with the operands read at the
// cell itself), float64 p / q / ans with the bounded remainder of a logadd through the float32 exp2 / log2 units, the
// row-per-lane sweep of mi_rowlane.h.
//
// What differs is the symbol predecessor p[s-1,t-e]: the value of the row below at step k - 1 - e.  ALL moves are reads
// of the history ring of mi_rowlane.h, of thread tid - ds (ds = 1 for a symbol move, 0 for a blank) -- a single move list
// of M = Dx + Dy entries, the kernel templated on M.  The layout, the ring and why its depth is safe are stated there;
// the depth is ring_depth(e_max): 16 for e_max = 0, 32 otherwise (32 KB of ring: 4 waves at depth 16, 2 at depth 32).
#include "mi_rowlane.h"

namespace ftr {
namespace {
using namespace rowlane;

template <int M, bool BWD>
__global__ void __launch_bounds__(64 * MAXW) mi_tdt_kernel(
    const float* __restrict__ px, const float* __restrict__ py, const int32_t* __restrict__ boundary, const Moves mv,
    double* __restrict__ p, double* __restrict__ ansd, double* __restrict__ carry, float* __restrict__ ans,
    const float* __restrict__ ans_grad, float* __restrict__ px_grad, float* __restrict__ py_grad, int S, int T, int NW,
    int DEP) {
  extern __shared__ double hist[];                    // [DEP][blockDim.x]: every thread's values of the last DEP steps
  __shared__ double cwin[CW];                        // wave 0: the strip below's top row around this chunk
  __shared__ double sh_ans;

  const int b = blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, w = tid >> 6;
  const Bound bd = load_boundary(boundary, b, S, T);
  const int Sn = bd.se - bd.sb + 1, Tn = bd.te - bd.tb + 1;
  const int T1 = T + 1;
  const int Dx = mv.Dx, Dy = M - mv.Dx;
  const double NEG = -__builtin_inf();

  if (Sn <= 0 || Tn <= 0) {                           // inverted rectangle: ans = 0 as the ordinary recursion's, no path
    if (!BWD && tid == 0) { ans[b] = 0.0f; ansd[b] = 0.0; }
    return;                                           // (backward: the gradients were cleared by the launcher)
  }
  double A = 0.0;
  float ag = 1.0f;
  if (BWD) {
    A = ansd[b];
    if (A == NEG) return;                             // no path: every occupancy is zero
    if (ans_grad) ag = ans_grad[b];
  }

  const size_t xplane = (size_t)S * T1, yplane = (size_t)(S + 1) * T;
  const float* px_b = px + (size_t)b * Dx * xplane;
  const float* py_b = py + (size_t)b * Dy * yplane;
  double* p_b = p + (size_t)b * (S + 1) * T1;
  float* gx_b = px_grad + (size_t)b * Dx * xplane;
  float* gy_b = py_grad + (size_t)b * Dy * yplane;
  const float* safe_f = reinterpret_cast<const float*>(p_b);   // where a masked lane loads from: always mapped
  if (!BWD && tid == 0) sh_ans = __builtin_nan("");             // always overwritten: the loop covers (Sn-1, Tn-1)
  __syncthreads();

  const int nst = strips(Sn, NW);
  const int below = tid > 0 ? tid - 1 : 0;            // the thread that holds the row below
  const int sback = lane == 0 ? CH : 1;              // ... and how many steps ago it was on this column
  for (int j = 0; j < nst; ++j) {
    // the geometry of Strip (mi_rowlane.h), written out: through the struct mi_tdt_kernel<3,true> gains a VGPR
    const int R = 64 * NW;                              // rows per strip
    const int rows = min(R, Sn - j * R);
    const int nwact = (rows + 63) >> 6;
    const int nk = Tn + 63 + E * (nwact - 1);
    const int nch = (nk + CH - 1) / CH;
    const bool active = w < nwact;
    const int r = j * R + 64 * w + lane;              // relative row (backward: counted down from s_end)
    const bool rowok = r < Sn;
    const int skew = lane + E * w;                    // t = k - skew
    const int s_act = BWD ? bd.se - r : bd.sb + r;
    const double* carry_in = carry + ((size_t)b * 2 + ((j + 1) & 1)) * T1;   // written by strip j - 1
    double* carry_out = carry + ((size_t)b * 2 + (j & 1)) * T1;
    const bool want_cin = active && w == 0 && j > 0;
    const bool give_carry = active && w == NW - 1 && lane == 63 && j + 1 < nst;

    // element offset of move m's operand for this lane's cell at relative column t (forward: at the predecessor)
    auto operand = [&](int m, int t) -> const float* {
      const int e = mv.dur[m];
      const int t_act = BWD ? bd.te - t : bd.tb + t - e;
      return m < Dx ? px_b + m * xplane + (size_t)(BWD ? s_act : s_act - 1) * T1 + t_act
                    : py_b + (m - Dx) * yplane + (size_t)s_act * T + t_act;
    };

    // every load is unconditional (a masked lane reads the workspace instead), so chunk c + 1's stay in flight while
    // chunk c computes; every unmasked index lies inside the boundary rectangle, which load_boundary clamps to the lattice
    auto load = [&](Ops<M, double>& o, int c) {
      {
        const int t = CH * c - MAXTOK + lane;
        const bool ok = want_cin && lane < CW && t >= 0 && t < Tn;
        o.cin = *(ok ? carry_in + t : p_b);
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
        if (BWD) o.pc[q] = *(valid ? p_b + (size_t)s_act * T1 + (bd.te - t) : p_b);
      }
    };

    auto chunk = [&](const Ops<M, double>& o, int c) {
      if (want_cin) {
        if (lane < CW) cwin[lane] = o.cin;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int k = CH * c + q;
        const int t = k - skew;
        const bool valid = rowok && t >= 0 && t < Tn;
        double src[M], term[M];
        double m0 = NEG, plain = NEG;
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const int e = mv.dur[m];
          const bool sym = m < Dx;
          const bool ok = valid && t >= e && (!sym || r >= 1);
          src[m] = hist[(size_t)((k - e - (sym ? sback : 0)) & (DEP - 1)) * nthr + (sym ? below : tid)];
          if (want_cin && sym) {                      // uniform per wave; wave 0's lane 0 is on column t = k
            const double cv = cwin[MAXTOK + q - e];
            src[m] = tid == 0 ? cv : src[m];
          }
          term[m] = ok ? src[m] + (double)o.w[m][q] : NEG;
          m0 = fmax(m0, term[m]);
          plain += term[m];
        }
        float sum = 0.0f;
#pragma unroll
        for (int m = 0; m < M; ++m) sum += exp_of(term[m] - m0);
        double v = m0 + (double)(__builtin_amdgcn_logf(sum) * kLn2);
        if (m0 == NEG) v = plain;                     // all -inf (or a NaN among them, which the sum keeps)
        if (r == 0 && t == 0) v = 0.0;
        if (valid) {
          const int t_act = BWD ? bd.te - t : bd.tb + t;
          if (!BWD) {
            p_b[(size_t)s_act * T1 + t_act] = v;
            if (r == Sn - 1 && t == Tn - 1) sh_ans = v;
          } else {
            const double base = o.pc[q] - A;          // p of the cell, relative to ans
#pragma unroll
            for (int m = 0; m < M; ++m) {
              const bool sym = m < Dx;
              if (t >= mv.dur[m] && (!sym || r >= 1)) {
                float* g = sym ? gx_b + m * xplane + (size_t)s_act * T1 + t_act
                               : gy_b + (m - Dx) * yplane + (size_t)s_act * T + t_act;
                *g = ag * exp_of(base + (double)o.w[m][q] + src[m]);
              }
            }
          }
          if (give_carry) carry_out[t] = v;           // the strip's top row, for the strip above
        }
        hist[(size_t)(k & (DEP - 1)) * nthr + tid] = v;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the upper lane reads it in a later step
      }
    };

    run_chunks<Ops<M, double>>(nch, active, load, chunk);
  }
  if (!BWD && tid == 0) {
    const double a = sh_ans;
    ansd[b] = a;
    ans[b] = (float)a;
  }
}

template <bool BWD>
int tdt_launch(const float* px, const float* py, const int32_t* boundary, const int32_t* token_durations, int Dx,
               const int32_t* blank_durations, int Dy, float* ws, size_t ws_floats, float* ans, const float* ans_grad,
               float* px_grad, float* py_grad, int B, int S, int T, hipStream_t st) {
  const char* what = BWD ? "mutual_information_tdt_bwd" : "mutual_information_tdt_fwd";
  int rc;
  if (launch_done(what, B, S, T, ws_floats, f64_workspace_floats(B, S, T), "floats", &rc)) return rc;
  if (BWD) {   // the kernel writes the moves that stay inside the boundary rectangle only
    rc = zero_words(px_grad, (size_t)B * Dx * S * (T + 1), st, what);
    if (rc != FTR_OK) return rc;
    rc = zero_words(py_grad, (size_t)B * Dy * (S + 1) * T, st, what);
    if (rc != FTR_OK) return rc;
  }
  const Moves mv = make_moves(token_durations, Dx, blank_durations, Dy);
  const int DEP = ring_depth(token_durations[Dx - 1]), NW = ring_waves_f64(S, DEP);
  const F64Layout L = f64_layout(B, S, T);
  double* wsd = reinterpret_cast<double*>(ws);
  double *p = wsd + L.p_off, *ansd = wsd + L.ans_off, *carry = wsd + L.carry_off;
  const size_t lds = (size_t)DEP * 64 * NW * sizeof(double);
  dispatch_range<2, MAXM>(Dx + Dy, [&](auto m) {
    hipLaunchKernelGGL((mi_tdt_kernel<decltype(m)::value, BWD>), dim3(B), dim3(64 * NW), lds, st, px, py, boundary, mv, p,
                       ansd, carry, ans, ans_grad, px_grad, py_grad, S, T, NW, DEP);
  }, [] {});   // the entry points admit no other arity
  return check_launch(what);
}

}  // namespace

size_t mi_tdt_workspace_floats(int B, int S, int T) { return rowlane::f64_workspace_floats(B, S, T); }

int mi_tdt_fwd(const float* px, const float* py, const int32_t* boundary, const int32_t* token_durations, int Dx,
               const int32_t* blank_durations, int Dy, float* ws, size_t ws_floats, float* ans, int B, int S, int T,
               hipStream_t st) {
  return tdt_launch<false>(px, py, boundary, token_durations, Dx, blank_durations, Dy, ws, ws_floats, ans, nullptr, nullptr,
                           nullptr, B, S, T, st);
}

int mi_tdt_bwd(const float* px, const float* py, const int32_t* boundary, const int32_t* token_durations, int Dx,
               const int32_t* blank_durations, int Dy, float* ws, size_t ws_floats, const float* ans_grad, float* px_grad,
               float* py_grad, int B, int S, int T, hipStream_t st) {
  return tdt_launch<true>(px, py, boundary, token_durations, Dx, blank_durations, Dy, ws, ws_floats, nullptr, ans_grad,
                          px_grad, py_grad, B, S, T, st);
}

}  // namespace ftr
