// csrc/mi_multiblank.hip -- the lattice recursion with big blanks (multi-blank transducer, MI355X addition, no reference
// counterpart): blank j of D advances durations[j] frames, a symbol advances one row.
//
//   p[s,t] = logadd( p[s-1,t] + px[s-1,t],  (+)_j  p[s,t-d_j] + py[j,s,t-d_j] ),   p[s_begin,t_begin] = 0
//   ans    = p[s_end,t_end]
//   px_grad[s,t]   = exp(p[s,t] + px[s,t]   + q[s+1,t]   - ans)       (occupancy of the symbol move out of (s,t))
//   py_grad[j,s,t] = exp(p[s,t] + py[j,s,t] + q[s,t+d_j] - ans)       (occupancy of blank j out of (s,t))
// where q is the same recursion run from (s_end,t_end) backwards.  One kernel serves both: the backward pass is the
// forward pass in mirrored coordinates (row r = s_end - s, column t = t_end - t) with the operands read at the cell
// itself instead of at its predecessors.  The forward launch stores p, the backward launch keeps q in flight only.
//
// Arithmetic: p and q are float64.  A logadd takes the maximum in float64 and sends only the bounded remainder
// log(sum exp(v_i - max)), which lies in [0, log(D+1)], through the float32 exp2 / log2 units (as mi_band_seg.hip does),
// so a cell adds ~1e-7 of absolute error instead of one float32 ulp of a p of magnitude 1e2..1e3; the occupancies are
// exp of a float64 sum p + w + q - ans.  Float32 p-differences miss the project's 1e-4 at T = 200.
//
// Layout: the row-per-lane sweep of mi_rowlane.h.  The symbol predecessor is the lower lane's value of the previous step
// (DPP shift), lane 0's comes from the wave below as computed one chunk of CH steps earlier (one LDS slot and one barrier
// per chunk), the top row of a strip goes to the next strip through the workspace.  The blank predecessors p[s,t-d_j] are
// the lane's own values of d_j steps earlier: the history ring of mi_rowlane.h (own-lane rule only), of depth
// 2^ceil(log2(max d)) per lane, which is what limits a workgroup to 256 rows (128 with a duration above 16).
#include "mi_rowlane.h"
#include "mi_wave_common.h"

namespace ftr {
namespace {
using namespace rowlane;

constexpr int MBMAXD = 8;              // blanks (D)

struct MbDur { int d[MBMAXD]; };

inline int mb_depth(int maxd) { int n = 1; while (n < maxd) n *= 2; return n; }

__device__ __forceinline__ double dpp_shr1_f64(double old_for_lane0, double src) {
  const long long o = __builtin_bit_cast(long long, old_for_lane0), s = __builtin_bit_cast(long long, src);
  const int lo = __builtin_amdgcn_update_dpp((int)o, (int)s, 0x138, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(s >> 32), 0x138, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}

template <int D>
struct MbOps {
  float x[CH], y[D][CH];
  double pc[CH];   // backward: p of the cell
  double cin;       // wave 0 of a strip above the first: lane q < CH holds the strip below's top row for step q
};

template <int D, bool BWD>
__global__ void __launch_bounds__(64 * MAXW) mi_multiblank_kernel(
    const float* __restrict__ px, const float* __restrict__ py, const int32_t* __restrict__ boundary, const MbDur dur,
    double* __restrict__ p, double* __restrict__ ansd, double* __restrict__ carry, float* __restrict__ ans,
    const float* __restrict__ ans_grad, float* __restrict__ px_grad, float* __restrict__ py_grad, int S, int T, int NW,
    int DEP) {
  extern __shared__ double hist[];                    // [DEP][blockDim.x]: the lane's own values of the last DEP steps
  __shared__ double ring[MAXW + 1][2][CH];         // ring[w]: the row below wave w's lane 0, per step of a chunk
  __shared__ double sh_ans;

  const int b = blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, w = tid >> 6;
  const Bound bd = load_boundary(boundary, b, S, T);
  const int Sn = bd.se - bd.sb + 1, Tn = bd.te - bd.tb + 1;
  const int T1 = T + 1;
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

  const size_t plane = (size_t)(S + 1) * T;
  const float* px_b = px + (size_t)b * S * T1;
  const float* py_b = py + (size_t)b * D * plane;
  double* p_b = p + (size_t)b * (S + 1) * T1;
  float* gx_b = px_grad + (size_t)b * S * T1;
  float* gy_b = py_grad + (size_t)b * D * plane;
  const float* safe_f = reinterpret_cast<const float*>(p_b);   // where a masked lane loads from: always mapped
  if (!BWD && tid == 0) sh_ans = __builtin_nan("");             // always overwritten: the loop covers (Sn-1, Tn-1)
  __syncthreads();

  const int nst = strips(Sn, NW);
  for (int j = 0; j < nst; ++j) {
    const Strip<double> s(bd, j, NW, w, lane, b, carry, T1, BWD);
    const int r = s.r, skew = s.skew, s_act = s.s_act;
    const bool rowok = s.rowok, want_cin = s.want_cin, give_carry = s.give_carry;

    // every load is unconditional (a masked lane reads the workspace instead), so chunk c + 1's stay in flight while
    // chunk c computes; every unmasked index lies inside the boundary rectangle, which load_boundary clamps to the lattice
    auto load = [&](MbOps<D>& o, int c) {
      {
        const int t = CH * c + (lane & (CH - 1));
        const bool ok = want_cin && t < Tn;
        o.cin = *(ok ? s.carry_in + t : p_b);
        o.cin = ok ? o.cin : NEG;
      }
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int t = CH * c + q - skew;
        const bool valid = rowok && t >= 0 && t < Tn;
        const int t_act = BWD ? bd.te - t : bd.tb + t;
        const bool xok = valid && r >= 1;
        const float* xp = xok ? px_b + (size_t)(BWD ? s_act : s_act - 1) * T1 + t_act : safe_f;
        o.x[q] = *xp;
#pragma unroll
        for (int jj = 0; jj < D; ++jj) {
          const bool yok = valid && t >= dur.d[jj];
          const float* yp = yok ? py_b + jj * plane + (size_t)s_act * T + (BWD ? t_act : t_act - dur.d[jj]) : safe_f;
          o.y[jj][q] = *yp;
        }
        if (BWD) o.pc[q] = *(valid ? p_b + (size_t)s_act * T1 + t_act : p_b);
      }
    };

    double pv = NEG;
    auto chunk = [&](const MbOps<D>& o, int c) {
      if (w == 0 && lane < CH) ring[0][c & 1][lane] = o.cin;   // the strip below's top row (-inf for the first strip)
      double up0[CH];
#pragma unroll
      for (int q = 0; q < CH; ++q) up0[q] = (w > 0 && c == 0) ? NEG : ring[w][(w > 0 ? c - 1 : c) & 1][q];
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int k = CH * c + q;
        const int t = k - skew;
        const bool valid = rowok && t >= 0 && t < Tn;
        const int t_act = BWD ? bd.te - t : bd.tb + t;
        const double up = dpp_shr1_f64(up0[q], pv);
        const bool xok = valid && r >= 1;
        const double a = xok ? up + (double)o.x[q] : NEG;
        double term[D], own[D];
        double m = a, plain = a;
#pragma unroll
        for (int jj = 0; jj < D; ++jj) {
          own[jj] = hist[(size_t)((k - dur.d[jj]) & (DEP - 1)) * nthr + tid];
          term[jj] = (valid && t >= dur.d[jj]) ? own[jj] + (double)o.y[jj][q] : NEG;
          m = fmax(m, term[jj]);
          plain += term[jj];
        }
        float sum = exp_of(a - m);
#pragma unroll
        for (int jj = 0; jj < D; ++jj) sum += exp_of(term[jj] - m);
        double v = m + (double)(__builtin_amdgcn_logf(sum) * kLn2);
        if (m == NEG) v = plain;                      // all -inf (or a NaN among them, which the sum keeps)
        if (r == 0 && t == 0) v = 0.0;
        if (valid) {
          if (!BWD) {
            p_b[(size_t)s_act * T1 + t_act] = v;
            if (r == Sn - 1 && t == Tn - 1) sh_ans = v;
          } else {
            const double base = o.pc[q] - A;          // p of the cell, relative to ans
            if (xok) gx_b[(size_t)s_act * T1 + t_act] = ag * exp_of(base + (double)o.x[q] + up);
            if (t >= 1) {                             // column t_end holds no blank move
#pragma unroll
              for (int jj = 0; jj < D; ++jj)
                gy_b[jj * plane + (size_t)s_act * T + t_act] =
                    t >= dur.d[jj] ? ag * exp_of(base + (double)o.y[jj][q] + own[jj]) : 0.0f;
            }
          }
        }
        hist[(size_t)(k & (DEP - 1)) * nthr + tid] = v;
        pv = v;
        if (lane == 63) ring[w + 1][c & 1][q] = v;    // for wave w + 1 in the next chunk
      }
      if (give_carry && lane < CH) {
        const int t = CH * c + lane - 63 - E * w;
        if (t >= 0 && t < Tn) s.carry_out[t] = ring[w + 1][c & 1][lane];
      }
    };

    run_chunks<MbOps<D>>(s.nch, s.active, load, chunk);
  }
  if (!BWD && tid == 0) {
    const double a = sh_ans;
    ansd[b] = a;
    ans[b] = (float)a;
  }
}

template <bool BWD>
int mb_launch(const float* px, const float* py, const int32_t* boundary, const int32_t* durations, int D, float* ws,
              size_t ws_floats, float* ans, const float* ans_grad, float* px_grad, float* py_grad, int B, int S, int T,
              hipStream_t st) {
  const char* what = BWD ? "mutual_information_multiblank_bwd" : "mutual_information_multiblank_fwd";
  int rc;
  if (launch_done(what, B, S, T, ws_floats, f64_workspace_floats(B, S, T), "floats", &rc)) return rc;
  if (BWD) {   // the kernel writes the cells of the boundary rectangle only
    rc = zero_words(px_grad, (size_t)B * S * (T + 1), st, what);
    if (rc != FTR_OK) return rc;
    rc = zero_words(py_grad, (size_t)B * D * (S + 1) * T, st, what);
    if (rc != FTR_OK) return rc;
  }
  MbDur dur;
  for (int j = 0; j < MBMAXD; ++j) dur.d[j] = j < D ? durations[j] : 1;
  const int maxd = durations[D - 1];
  const int DEP = mb_depth(maxd), NW = ring_waves_f64(S, DEP);
  const F64Layout L = f64_layout(B, S, T);
  double* wsd = reinterpret_cast<double*>(ws);
  double *p = wsd + L.p_off, *ansd = wsd + L.ans_off, *carry = wsd + L.carry_off;
  const size_t lds = (size_t)DEP * 64 * NW * sizeof(double);
  dispatch_range<1, MBMAXD>(D, [&](auto d) {
    hipLaunchKernelGGL((mi_multiblank_kernel<decltype(d)::value, BWD>), dim3(B), dim3(64 * NW), lds, st, px, py, boundary,
                       dur, p, ansd, carry, ans, ans_grad, px_grad, py_grad, S, T, NW, DEP);
  }, [] {});   // the entry points admit no other arity
  return check_launch(what);
}

}  // namespace

size_t mi_multiblank_workspace_floats(int B, int S, int T) { return rowlane::f64_workspace_floats(B, S, T); }

int mi_multiblank_fwd(const float* px, const float* py, const int32_t* boundary, const int32_t* durations, int D, float* ws,
                      size_t ws_floats, float* ans, int B, int S, int T, hipStream_t st) {
  return mb_launch<false>(px, py, boundary, durations, D, ws, ws_floats, ans, nullptr, nullptr, nullptr, B, S, T, st);
}

int mi_multiblank_bwd(const float* px, const float* py, const int32_t* boundary, const int32_t* durations, int D, float* ws,
                      size_t ws_floats, const float* ans_grad, float* px_grad, float* py_grad, int B, int S, int T,
                      hipStream_t st) {
  return mb_launch<true>(px, py, boundary, durations, D, ws, ws_floats, nullptr, ans_grad, px_grad, py_grad, B, S, T, st);
}

}  // namespace ftr
