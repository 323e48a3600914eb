// csrc/pruned_kd.hip -- knowledge distillation on the pruned band (include/ftr_kd.h, include/ftr_kd_fact.h, include/ftr_kd_loss.h; MI355X addition,
// no reference counterpart), gfx950.
// Student and teacher joiner logits x, y [B,T,r,W] on the same `ranges`; per valid node (b,t,k) the loss is KL(p || q) with
// p = softmax(y / tau), q = softmax(x / tau) over the columns ("full"), or over three classes -- blank, the correct next
// symbol, everything else -- ("collapsed", Panchapagesan et al., ICASSP 2021).  No tau^2 factor.  A row is one of three forms,
// a compile-time parameter of every kernel:
//   KD_PLAIN one softmax over all W columns, no node weights, no duration columns: all three known at compile time, so
//            neither the weight, nor the column mask, nor a tail is in its code
//   KD_HAT   the blank column Bk is a sigmoid of its own, the other columns a softmax over c != Bk:
//            full       KL(Bern(pb) || Bern(qb)) + (1 - pb) sum_{c != Bk} v_c (log v_c - log u_c)
//            collapsed  the same with the non-blank softmax collapsed to {symbol, rest}
//   KD_TDT   a row of width W = Ct + N: a token softmax over the first Ct columns (the plain loss on them, either mode) and a
//            duration softmax over the last N <= 5, whose full KL is added with the multiplier dur_weight.  N is a run-time
//            argument, and N = 0 is how one softmax with node weights runs
// and, in the last two, optional per-node weights w [B,T,r] (a run-time pointer): node loss and gradient row times w, and
// w == 0 makes the node invalid.
//   kd_fwd_reg_kernel  one wave per row, both rows held in registers (W % 4 == 0, W <= 256 * NQ), every load issued
//                      before the first use, one pass, last rows first: as lse_rows_reg_kernel of pruned_logprobs.hip,
//                      twice the registers
//   kd_fwd_kernel      any W: two passes over the row (the second hits L1/L2), four elements at a time or one by one
//   kd_utt_sum_kernel  node losses -> per-utterance loss, one block per utterance, fixed summation tree
//   kd_bwd_kernel      one streaming pass: d loss / d x from x, y and the normalisers the forward saved (no reduction); it
//                      writes all W columns of the gradient row
// The three row kernels also have loss-carrying instantiations (LOSS; include/ftr_kd_loss.h the plain form,
// include/ftr_kd_loss_fact.h the HAT form and the weighted softmax, which is KD_TDT with N = 0): the forward writes the
// normaliser of the transducer loss on the band as well, the backward adds that loss's gradient row; see KdLossOut and
// KdLossIn below.
// The three forms share the column -> lane mapping and the order of every sum.  The columns that are not part of the main
// sums (HAT: the blank; TDT: the duration columns; collapsed: the class columns) are masked to -inf in registers, as
// tdt_lse_kernel of tdt_logprobs.hip masks 4 * i + e >= C.  What is left at the end of a row: HAT, the Bernoulli term from
// the two blank logits (the softplus / hat_sigmoids arithmetic of ftr_common.h, as the HAT builder forms its log-sigmoids),
// student and teacher on two lanes at once; TDT, the duration head from at most five columns of each row, one per lane.
// A node is valid iff t_begin <= t < t_end and s_begin <= ranges[b,t,k] <= s_end and its weight is not 0; validity is
// decided from ranges, boundary and the weight BEFORE any logits load, an invalid row is never read (padding frames of a
// joiner hold garbage), its node loss and normalisers are 0 and its gradient row is written as zeros.
// Saved normalisers, float32 planes of [B,T,r]: 0, 1 = the logsumexps of the main softmax (student, teacher); collapsed:
// 2, 3 = the same over the "rest" columns only (a masked logsumexp with its own maximum, never log(1 - ...)); TDT with
// N > 0: the last two = those of the duration head (written as 0 and never read when dur_weight == 0).
// Element types of x and y are independent (float, bf16_t, fp16_t); a row is read four elements at a time only when BOTH
// tensors pass rows_vec4.  All arithmetic is float32; the gradient row is rounded once when it is stored in x's type.
#include "kd_common.h"

namespace ftr {
namespace {

constexpr int KD_PLAIN = 0, KD_HAT = 1, KD_TDT = 2;
constexpr int KF_MAXN = FTR_KD_FACT_MAX_DUR;

__device__ __forceinline__ float wave_max(float v) { return wave_max_dpp(v); }
__device__ __forceinline__ float wave_sum(float v) { return wave_sum_dpp(v); }

// what a wave knows about its row before it touches the logits: is the node valid, whose utterance is it, its weight (1
// without weights), the blank column k0 and (collapsed) the symbol column k1 (-1: the node has no symbol class)
// (lrow, s: for the loss-carrying instantiations only -- does the band recursion look at this row's px / py at all, i.e. is
// t inside the frames of the rectangle and s inside the lattice; the node's lattice row; and `geo`, valid but for its
// weight: a node of weight 0 is out of the distillation only, the transducer loss still owns its gradient row)
struct KdRow { bool valid, lrow, geo; int b, s, k0, k1; float w; };

template <bool COLL>
__device__ __forceinline__ KdRow kd_row(size_t row, const int32_t* __restrict__ symbols, const int32_t* __restrict__ ranges,
                                        const int32_t* __restrict__ boundary, const float* __restrict__ weights, int blank,
                                        int T, int S, int Ct, int r) {
  const KdNode n = kd_node(row, ranges, boundary, weights, T, S, r);
  KdRow g;
  g.valid = n.valid; g.geo = n.geo; g.b = n.b; g.s = n.s; g.w = n.w;
  g.lrow = n.t >= n.bd.tb && n.t < n.bd.te && n.s >= 0 && n.s <= S;
  g.k0 = blank;
  g.k1 = -1;
  if (COLL && g.valid && n.s < n.bd.se) {
    const int c = min(max(symbols[(size_t)g.b * S + n.s], 0), Ct - 1);   // symbol kept among the token columns, as the pruned builders do
    if (c != blank) g.k1 = c;
  }
  return g;
}

__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));   // a NaN among a, b, c comes out of the sum
}

// the number of saved planes: 2, + 2 collapsed, + 2 with a duration head
template <bool COLL>
__device__ __forceinline__ int kd_planes(int N) { return (COLL ? 4 : 2) + (N > 0 ? 2 : 0); }

template <bool COLL>
__device__ __forceinline__ void kd_store_invalid(float* __restrict__ node, float* __restrict__ saved, size_t rows, size_t row, int N) {
  node[row] = 0.0f;
  for (int p = 0; p < kd_planes<COLL>(N); ++p) saved[(size_t)p * rows + row] = 0.0f;
}

// ---- the duration head (TDT), one column per lane: lane j < 8 takes column W - 8 + j of both rows if that is a duration
// column (N <= 5 < 8), one load per tensor issued with the class logits before the first use of the row; the head's maxima
// and sums are then three DPP steps over lanes 0..7 (the first three of wave_max_dpp / wave_sum_dpp), read from lane 7.
// A serial loop over the N columns on lane 0 was built first: with its 2 N loads and its chain of N exponentials behind the
// row's own reductions, the forward kernel took 150 - 190 us at c3 where the plain kd_fwd_reg_kernel takes 112 - 135.
static_assert(KF_MAXN <= 8, "the duration head is reduced over lanes 0..7");
__device__ __forceinline__ float oct_max(float v) {
  constexpr float ninf = -__builtin_inff();
  v = fmaxf(v, dpp_take<0x111, 0xf, 0xf>(ninf, v));   // row_shr:1
  v = fmaxf(v, dpp_take<0x112, 0xf, 0xf>(ninf, v));   // row_shr:2
  v = fmaxf(v, dpp_take<0x114, 0xf, 0xf>(ninf, v));   // row_shr:4 -> lane 7 holds the maximum of lanes 0..7
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 7));
}
__device__ __forceinline__ float oct_sum(float v) {
  v += dpp_take<0x111, 0xf, 0xf>(0.0f, v);
  v += dpp_take<0x112, 0xf, 0xf>(0.0f, v);
  v += dpp_take<0x114, 0xf, 0xf>(0.0f, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 7));
}

// this lane's duration column of both rows (scaled), -inf on the lanes that have none
struct KfDurLane { float x, y; };
template <typename ES, typename ET>
__device__ __forceinline__ KfDurLane kf_load_dur(const ES* xr, const ET* yr, int lane, int W, int Ct, bool on, float inv_tau) {
  KfDurLane d = {-INFINITY, -INFINITY};
  const int c = W - 8 + lane;
  if (on && lane < 8 && c >= Ct) {   // Ct >= 1: c is inside the row
    d.x = elem_to_float(xr[c]) * inv_tau;
    d.y = elem_to_float(yr[c]) * inv_tau;
  }
  return d;
}
// the head's full KL, by every lane of the wave: *Ds, *Dt = the two logsumexps, the return value KL(teacher || student)
__device__ __forceinline__ float kf_dur_kl(const KfDurLane d, float* Ds, float* Dt) {
  const float md = kd_safe_max(oct_max(d.x)), me = kd_safe_max(oct_max(d.y));
  const float p = __expf(d.y - me);
  const float sd = oct_sum(__expf(d.x - md)), se = oct_sum(p), kl = oct_sum(kd_term(p, d.y - d.x));
  *Ds = md + __logf(sd);
  *Dt = me + __logf(se);
  return kl / se - (*Dt - *Ds);
}

// softplus(v) and softplus(-v) of ftr_common.h from one exponential and one log1pf (the two calls share
// log1pf(expf(-|v|)): the values are theirs bit for bit), and, if asked for, hat_sigmoids(v) from the same exponential
__device__ __forceinline__ void hat_softplus_pair(float v, float* pos, float* neg, float* sp = nullptr, float* sn = nullptr) {
  const float e = expf(-fabsf(v)), t = log1pf(e);
  *pos = fmaxf(v, 0.0f) + t;
  *neg = fmaxf(-v, 0.0f) + t;
  if (sp) {
    const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
    *sp = v >= 0.0f ? big : small;
    *sn = v >= 0.0f ? small : big;
  }
}

// HAT: KL(Bern(pb) || Bern(qb)) from the two blank logits, and pn = 1 - pb = sigmoid(-yb), the mass the KL of the non-blank
// softmaxes carries.  By every lane of the wave: the even lanes evaluate the student's logit and the odd lanes the teacher's,
// so the library expf / log1pf and the divisions are issued once for both, and lanes 0 and 1 hand the results to all.  The
// forward kernels are bound by the instructions they issue, not by this tail's latency: with both logits evaluated one after
// the other the HAT forms took 149 - 187 us at c3 where the TDT forms took 125 - 165, whether the term stood after the
// row's reductions on lane 0 or ahead of them in the shadow of the row loads.
struct KfBern { float kl, pn; };
__device__ __forceinline__ float lane_value(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }
__device__ __forceinline__ KfBern kf_hat_bern(float xb, float yb, int lane) {
  float pos, neg, sp, sn;   // pos = softplus(z) = -log sigmoid(-z), neg = softplus(-z) = -log sigmoid(z), sp / sn = sigmoid(+-z)
  hat_softplus_pair((lane & 1) ? yb : xb, &pos, &neg, &sp, &sn);
  const float spx = lane_value(pos, 0), snx = lane_value(neg, 0), spy = lane_value(pos, 1), sny = lane_value(neg, 1);
  const float pb = lane_value(sp, 1), pn = lane_value(sn, 1);
  return KfBern{kd_term(pb, snx - sny) + kd_term(pn, spx - spy), pn};
}

// The end of a forward row (lane 0), from the wave-reduced sums over the columns of the main softmax that are not masked.
// ms, mt: the maxima the sums were taken against; ss, st: sums of exp(. - max); full: over all columns, kl = sum exp(y - mt)
// (y - x); collapsed: over the rest columns, and xb, yb are the blank logits, xs, ys the symbol logits (-inf without a symbol
// class).  Everything is already divided by tau.  bern: the HAT tail; dur_kl, Ds, Dt: the TDT tail; w: the node's weight.
template <int FORM, bool COLL>
__device__ __forceinline__ void kd_finish(float* __restrict__ node, float* __restrict__ saved, size_t rows, size_t row,
                                          float ms, float ss, float mt, float st, float kl, float xb, float xs, float yb,
                                          float ys, const KfBern bern, float dur_kl, float Ds, float Dt, int N, float dw, float w) {
  constexpr bool HAT = FORM == KD_HAT;
  float loss, Ls, Lt, Rs = 0.0f, Rt = 0.0f;
  if (!COLL) {
    Ls = ms + __logf(ss);
    Lt = mt + __logf(st);
    loss = kl / st - (Lt - Ls);
  } else {
    Rs = ms + __logf(ss);   // no rest column at all: -inf + log 0 = -inf
    Rt = mt + __logf(st);
    // HAT: the blank is no class of this softmax
    const float cb_s = HAT ? -INFINITY : xb, cb_t = HAT ? -INFINITY : yb;
    Ls = lse3(Rs, cb_s, xs);
    Lt = lse3(Rt, cb_t, ys);
    const float lpb = cb_t - Lt, lps = ys - Lt, lpr = Rt - Lt;
    // the hardware exp / log, as in the sums: this tail runs once per row, and with the library forms it took longer than the row
    loss = kd_term(__expf(lpb), lpb - (cb_s - Ls)) + kd_term(__expf(lps), lps - (xs - Ls)) + kd_term(__expf(lpr), lpr - (Rs - Ls));
  }
  // HAT: loss so far is the KL of the non-blank softmaxes; it carries the teacher's non-blank mass 1 - pb (mass 0 adds
  // nothing, but a NaN row stays NaN)
  if (HAT) loss = bern.kl + ((bern.pn == 0.0f && loss == loss) ? 0.0f : bern.pn * loss);
  saved[row] = Ls;
  saved[rows + row] = Lt;
  if (COLL) {
    saved[2 * rows + row] = Rs;
    saved[3 * rows + row] = Rt;
  }
  if (FORM == KD_TDT && N > 0) {   // dur_weight == 0: the head was not looked at, dur_kl = Ds = Dt = 0
    if (dw != 0.0f) loss += dw * dur_kl;
    const int p0 = COLL ? 4 : 2;
    saved[(size_t)p0 * rows + row] = Ds;
    saved[(size_t)(p0 + 1) * rows + row] = Dt;
  }
  node[row] = FORM == KD_PLAIN ? loss : loss * w;
}

// is column c outside the sums of the main softmax?
template <int FORM, bool COLL>
__device__ __forceinline__ bool kd_masked(int c, int Ct, int k0, int k1) {
  return (FORM == KD_TDT && c >= Ct) || ((FORM == KD_HAT || COLL) && c == k0) || (COLL && c == k1);
}

// ---- the loss-carrying instantiations (include/ftr_kd_loss.h; LOSS, plain form only): the forward kernels also write lse1,
// the temperature-1 logsumexp of the student row over all W columns, which is the normaliser of the transducer loss
// (band_gather_kernel and band_grad_banded_kernel of mi_band.hip read it).  What they take on top is a trailing parameter
// pack, empty for every other instantiation, as tdt_logprobs.hip does for MIX.
// lse1 restates lse_rows_reg_kernel / lse_rows_kernel of pruned_logprobs.hip operation for operation -- the raw maximum (no
// kd_safe_max: a row of -inf gives NaN there too), the exponentials of a quad added left to right and then to the lane's
// sum, the lanes' sums through the same DPP ladder -- so that the loss is the loss of rnnt_loss_pruned bit for bit.
// Which rows carry it: every node the band recursion looks at, and that is more than the valid nodes -- its shift constants
// (ftr_common.h, Shift) are means over ALL band entries of the frames [t_begin, t_end), the rows past s_end included.  Such a
// row (KdRow::lrow and not valid) has its student row read for lse1 alone; the teacher's is not.  Outside those frames
// nothing is read and lse1 = 0: the recursion never looks there.
// HAT (include/ftr_kd_loss_fact.h): the normaliser is Z, the logsumexp over c != blank, and what is restated is
// lse_rows_*<., ., HAT = true>: the blank column set to -inf before the maximum and the sum, nothing else changed.  At
// temperature 1 in full mode that is the very masking of the KD_HAT sums, so the sharing below holds for it as it stands.
// A node of weight 0 is a row that only the loss needs, like the rows past s_end.
struct KdLossOut { float* lse; };
template <typename A> __device__ __forceinline__ const A& kd_loss_arg(const A& a) { return a; }

template <int NQ>
__device__ __forceinline__ float lse1_lane_max(const f4 (&v)[NQ]) {
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) m = fmaxf(fmaxf(m, fmaxf(v[q][0], v[q][1])), fmaxf(v[q][2], v[q][3]));
  return m;
}
template <int NQ>
__device__ __forceinline__ float lse1_lane_sum(const f4 (&v)[NQ], float m, int lane, int n4) {
  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (lane + 64 * q < n4)
      sum += __expf(v[q][0] - m) + __expf(v[q][1] - m) + __expf(v[q][2] - m) + __expf(v[q][3] - m);
  }
  return sum;
}
// a row that only the loss needs, register resident (W % 4 == 0, W <= 256 * NQ)
template <int NQ>
__device__ __forceinline__ void lse1_mask_blank(f4 (&v)[NQ], int lane, int blank) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[q][e] = (4 * (lane + 64 * q) + e == blank) ? -INFINITY : v[q][e];
  }
}
template <typename ES, int NQ, bool HAT = false>
__device__ __forceinline__ float lse1_reg(const ES* xr, int lane, int n4, int blank = -1) {
  const f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  f4 v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    v[q] = (i < n4) ? load4(xr, i) : ninf;
  }
  if (HAT) lse1_mask_blank<NQ>(v, lane, blank);
  const float m = wave_max(lse1_lane_max<NQ>(v));
  return m + __logf(wave_sum(lse1_lane_sum<NQ>(v, m, lane, n4)));
}
// any W, two passes: lse_rows_kernel
template <typename ES, bool VEC, bool HAT = false>
__device__ __forceinline__ float lse1_two_pass(const ES* xr, int lane, int W, int blank = -1) {
  float m = -INFINITY, s = 0.0f;
  if (VEC) {
    const int n4 = W >> 2;
    for (int i = lane; i < n4; i += 64) {
      f4 v = load4(xr, i);
      if (HAT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (4 * i + e == blank) ? -INFINITY : v[e];
      }
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    m = wave_max(m);
    for (int i = lane; i < n4; i += 64) {
      f4 v = load4(xr, i);
      if (HAT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (4 * i + e == blank) ? -INFINITY : v[e];
      }
      s += __expf(v[0] - m) + __expf(v[1] - m) + __expf(v[2] - m) + __expf(v[3] - m);
    }
  } else {
    for (int i = lane; i < W; i += 64) m = fmaxf(m, (HAT && i == blank) ? -INFINITY : elem_to_float(xr[i]));
    m = wave_max(m);
    for (int i = lane; i < W; i += 64) s += __expf(((HAT && i == blank) ? -INFINITY : elem_to_float(xr[i])) - m);
  }
  return m + __logf(wave_sum(s));
}

template <typename ES, typename ET, int NQ, int FORM, bool COLL, bool LOSS = false, typename... L>
__global__ __launch_bounds__(256) void kd_fwd_reg_kernel(const ES* __restrict__ x, const ET* __restrict__ y,
                                                         const int32_t* __restrict__ symbols, const int32_t* __restrict__ ranges,
                                                         const int32_t* __restrict__ boundary, const float* __restrict__ weights,
                                                         int blank, float inv_tau, float dw, float* __restrict__ node,
                                                         float* __restrict__ saved, size_t rows, int T, int S, int W, int N, int r,
                                                         const L... lo) {
  static_assert(sizeof...(L) == (LOSS ? 1 : 0), "one KdLossOut when LOSS, else nothing");   // LOSS with KD_TDT: N = 0 only (the hosts)
  constexpr bool HAT = FORM == KD_HAT;
  if (FORM == KD_PLAIN) { weights = nullptr; N = 0; }   // known at compile time: what hangs on them is not in the plain form's code
  const int lane = threadIdx.x & 63;
  const size_t rowi = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (rowi >= rows) return;
  const size_t row = rows - 1 - rowi;   // last rows first: the tail of a tensor that was just written is what the cache still holds
  const int Ct = W - N;
  const KdRow g = kd_row<COLL>(row, symbols, ranges, boundary, weights, blank, T, S, Ct, r);
  const int n4 = W >> 2;
  const ES* xr = x + row * W;
  if (!g.valid) {
    if constexpr (LOSS) {   // a row of the rectangle's frames past s_end / before s_begin: the student row, for lse1 alone
      float l1 = 0.0f;
      if (g.lrow) l1 = lse1_reg<ES, NQ, HAT>(xr, lane, n4, blank);
      if (lane == 0) kd_loss_arg(lo...).lse[row] = l1;
    }
    if (lane == 0) kd_store_invalid<COLL>(node, saved, rows, row, N);
    return;
  }
  const f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const ET* yr = y + row * W;
  float xb = -INFINITY, xs = -INFINITY, yb = -INFINITY, ys = -INFINITY;
  if (HAT) {   // the two logits of the Bernoulli term
    xb = elem_to_float(xr[g.k0]) * inv_tau;
    yb = elem_to_float(yr[g.k0]) * inv_tau;
  }
  f4 v[NQ], w[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    v[q] = (i < n4) ? load4(xr, i) : ninf;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    w[q] = (i < n4) ? load4(yr, i) : ninf;
  }
  if (!HAT && COLL) {   // the class logits, by every lane from the same address: lines this wave is fetching anyway
    xb = elem_to_float(xr[g.k0]) * inv_tau;
    yb = elem_to_float(yr[g.k0]) * inv_tau;
  }
  if (COLL && g.k1 >= 0) {
    xs = elem_to_float(xr[g.k1]) * inv_tau;
    ys = elem_to_float(yr[g.k1]) * inv_tau;
  }
  const bool dur_on = FORM == KD_TDT && N > 0 && dw != 0.0f;   // the same for every wave of the launch
  const KfDurLane dur = kf_load_dur(xr, yr, lane, W, Ct, dur_on, inv_tau);
  // LOSS: lse1 from the registers that hold the student row, before they are scaled and masked.  `share`: full mode at
  // temperature 1 -- no column is masked, v * 1 is v and ms below is m1, so the exponentials of the student's sum ARE those
  // of lse1; they are added up a second time in lse1's order instead of being evaluated twice.
  float m1 = 0.0f, s1 = 0.0f;
  bool share = false;
  if constexpr (LOSS) {
    if (HAT) lse1_mask_blank<NQ>(v, lane, blank);   // Z; the column is masked in the sums below anyway
    m1 = wave_max(lse1_lane_max<NQ>(v));
    share = !COLL && inv_tau == 1.0f && m1 > -INFINITY;   // -inf: ms is kd_safe_max's 0, not m1; NaN compares false
    if (!share) s1 = lse1_lane_sum<NQ>(v, m1, lane, n4);
  }
  float ms = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool out = kd_masked<FORM, COLL>(4 * (lane + 64 * q) + e, Ct, g.k0, g.k1);
      v[q][e] = out ? -INFINITY : v[q][e] * inv_tau;
      w[q][e] = out ? -INFINITY : w[q][e] * inv_tau;
    }
    ms = fmaxf(fmaxf(ms, fmaxf(v[q][0], v[q][1])), fmaxf(v[q][2], v[q][3]));
    mt = fmaxf(fmaxf(mt, fmaxf(w[q][0], w[q][1])), fmaxf(w[q][2], w[q][3]));
  }
  ms = kd_safe_max(wave_max(ms));
  mt = kd_safe_max(wave_max(mt));
  float ss = 0.0f, st = 0.0f, kl = 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    float ex[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // masked columns and lanes past the row hold -inf: exp gives 0 and the kl term is skipped
      ex[e] = __expf(v[q][e] - ms);
      ss += ex[e];
      const float p = __expf(w[q][e] - mt);
      st += p;
      if (!COLL) kl += kd_term(p, w[q][e] - v[q][e]);
    }
    if constexpr (LOSS) {
      if (share && lane + 64 * q < n4) s1 += ex[0] + ex[1] + ex[2] + ex[3];
    }
  }
  ss = wave_sum(ss);
  st = wave_sum(st);
  if (!COLL) kl = wave_sum(kl);
  if constexpr (LOSS) {
    s1 = wave_sum(s1);
    if (lane == 0) kd_loss_arg(lo...).lse[row] = m1 + __logf(s1);
  }
  KfBern bern = {0.0f, 1.0f};
  if (HAT) bern = kf_hat_bern(xb, yb, lane);   // after the row: its registers are free by now
  float dur_kl = 0.0f, Ds = 0.0f, Dt = 0.0f;
  if (dur_on) dur_kl = kf_dur_kl(dur, &Ds, &Dt);
  if (lane == 0) kd_finish<FORM, COLL>(node, saved, rows, row, ms, ss, mt, st, kl, xb, xs, yb, ys, bern, dur_kl, Ds, Dt, N, dw, g.w);
}

// any W, one wave per row, two passes (the second hits L1/L2: a row is a few KB)
template <typename ES, typename ET, bool VEC, int FORM, bool COLL, bool LOSS = false, typename... L>
__global__ void kd_fwd_kernel(const ES* __restrict__ x, const ET* __restrict__ y, const int32_t* __restrict__ symbols,
                              const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                              const float* __restrict__ weights, int blank, float inv_tau, float dw, float* __restrict__ node,
                              float* __restrict__ saved, size_t rows, int T, int S, int W, int N, int r, const L... lo) {
  static_assert(sizeof...(L) == (LOSS ? 1 : 0), "one KdLossOut when LOSS, else nothing");   // LOSS with KD_TDT: N = 0 only (the hosts)
  constexpr bool HAT = FORM == KD_HAT;
  if (FORM == KD_PLAIN) { weights = nullptr; N = 0; }
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int Ct = W - N;
  const KdRow g = kd_row<COLL>(row, symbols, ranges, boundary, weights, blank, T, S, Ct, r);
  const ES* xr = x + row * W;
  if constexpr (LOSS) {   // lse1 by two passes of its own, in lse_rows_kernel's order: this kernel is the slow path, and the row stays in L1
    float l1 = 0.0f;
    if (g.lrow) l1 = lse1_two_pass<ES, VEC, HAT>(xr, lane, W, blank);
    if (lane == 0) kd_loss_arg(lo...).lse[row] = l1;
  }
  if (!g.valid) {
    if (lane == 0) kd_store_invalid<COLL>(node, saved, rows, row, N);
    return;
  }
  const ET* yr = y + row * W;
  float xb = -INFINITY, xs = -INFINITY, yb = -INFINITY, ys = -INFINITY;
  if (HAT || COLL) {
    xb = elem_to_float(xr[g.k0]) * inv_tau;
    yb = elem_to_float(yr[g.k0]) * inv_tau;
  }
  if (COLL && g.k1 >= 0) {
    xs = elem_to_float(xr[g.k1]) * inv_tau;
    ys = elem_to_float(yr[g.k1]) * inv_tau;
  }
  const bool dur_on = FORM == KD_TDT && N > 0 && dw != 0.0f;   // the same for every wave of the launch
  const KfDurLane dur = kf_load_dur(xr, yr, lane, W, Ct, dur_on, inv_tau);
  float ms = -INFINITY, mt = -INFINITY, ss = 0.0f, st = 0.0f, kl = 0.0f;
  if (VEC) {
    const int n4 = W >> 2;
    for (int i = lane; i < n4; i += 64) {
      const f4 v = load4(xr, i), w = load4(yr, i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool out = kd_masked<FORM, COLL>(4 * i + e, Ct, g.k0, g.k1);
        ms = fmaxf(ms, out ? -INFINITY : v[e] * inv_tau);
        mt = fmaxf(mt, out ? -INFINITY : w[e] * inv_tau);
      }
    }
    ms = kd_safe_max(wave_max(ms));
    mt = kd_safe_max(wave_max(mt));
    for (int i = lane; i < n4; i += 64) {
      const f4 v = load4(xr, i), w = load4(yr, i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool out = kd_masked<FORM, COLL>(4 * i + e, Ct, g.k0, g.k1);
        const float a = out ? -INFINITY : v[e] * inv_tau, b = out ? -INFINITY : w[e] * inv_tau;
        ss += __expf(a - ms);
        const float p = __expf(b - mt);
        st += p;
        if (!COLL) kl += kd_term(p, b - a);
      }
    }
  } else {
    for (int c = lane; c < Ct; c += 64) {   // the duration columns lie past Ct: not visited at all
      const bool out = kd_masked<FORM, COLL>(c, Ct, g.k0, g.k1);
      ms = fmaxf(ms, out ? -INFINITY : elem_to_float(xr[c]) * inv_tau);
      mt = fmaxf(mt, out ? -INFINITY : elem_to_float(yr[c]) * inv_tau);
    }
    ms = kd_safe_max(wave_max(ms));
    mt = kd_safe_max(wave_max(mt));
    for (int c = lane; c < Ct; c += 64) {
      const bool out = kd_masked<FORM, COLL>(c, Ct, g.k0, g.k1);
      const float a = out ? -INFINITY : elem_to_float(xr[c]) * inv_tau, b = out ? -INFINITY : elem_to_float(yr[c]) * inv_tau;
      ss += __expf(a - ms);
      const float p = __expf(b - mt);
      st += p;
      if (!COLL) kl += kd_term(p, b - a);
    }
  }
  ss = wave_sum(ss);
  st = wave_sum(st);
  if (!COLL) kl = wave_sum(kl);
  KfBern bern = {0.0f, 1.0f};
  if (HAT) bern = kf_hat_bern(xb, yb, lane);   // after the row: its registers are free by now
  float dur_kl = 0.0f, Ds = 0.0f, Dt = 0.0f;
  if (dur_on) dur_kl = kf_dur_kl(dur, &Ds, &Dt);
  if (lane == 0) kd_finish<FORM, COLL>(node, saved, rows, row, ms, ss, mt, st, kl, xb, xs, yb, ys, bern, dur_kl, Ds, Dt, N, dw, g.w);
}

// utt[b] = sum of the T * r node losses of utterance b: one block per utterance, a fixed summation tree (deterministic)
__global__ __launch_bounds__(256) void kd_utt_sum_kernel(const float* __restrict__ node, float* __restrict__ utt, int per) {
  __shared__ float red[4];
  const float* p = node + (size_t)blockIdx.x * per;
  float s = 0.0f;
  for (int i = threadIdx.x; i < per; i += 256) s += p[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) utt[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the same tree over w * node (include/ftr_kd_loss_fact.h): what kd_utt_sum_kernel adds up when the row kernel itself
// multiplied by w as its last step.  w == 0: the node is out, whatever its loss (an infinite one included)
__global__ __launch_bounds__(256) void kd_utt_sum_weighted_kernel(const float* __restrict__ node, const float* __restrict__ wts,
                                                                  float* __restrict__ utt, int per) {
  __shared__ float red[4];
  const float* p = node + (size_t)blockIdx.x * per;
  const float* w = wts + (size_t)blockIdx.x * per;
  float s = 0.0f;
  for (int i = threadIdx.x; i < per; i += 256) {
    const float wi = w[i];
    s += wi == 0.0f ? 0.0f : p[i] * wi;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) utt[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// occ[b,t,k] = gx + gy, the occupancies of the two arcs that leave lattice node (ranges[b,t,k], t), under the masks of
// band_grad_banded_kernel (mi_band.hip): gx only where s < S (its other mask, t == t_end of the regular type, lies outside
// the rectangle).  Exact zeros for a node outside the boundary rectangle or outside the lattice, whatever the two arrays
// hold there.  One thread per node.
__global__ void band_node_occupancy_kernel(const float* __restrict__ gxb, const float* __restrict__ gyb,
                                           const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                                           float* __restrict__ occ, size_t rows, int T, int S, int r) {
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const size_t bt = row / r;
  const int b = (int)(bt / T);
  const int t = (int)(bt - (size_t)b * T);
  const int s = ranges[row];
  const Bound bd = load_boundary(boundary, b, S, T);
  float v = 0.0f;
  if (t >= bd.tb && t < bd.te && s >= bd.sb && s <= bd.se) {
    const float gx = s < S ? gxb[row] : 0.0f;
    v = gx + gyb[row];
  }
  occ[row] = v;
}

// d loss / d x[c] of one element, a = x[c] / tau, b = y[c] / tau.  k = upstream gradient * weight / tau.
//   main softmax, full:       kk (q_c - p_c)
//                 collapsed:  kk (Q_j - P_j) w_c for c in class j, Q / P the student's / teacher's class masses and w_c the
//                             share of column c in its class: 1 for the blank and the symbol, exp(a - Rs) for a rest column
//                             (q_c = Q_rest exp(a - Rs))
//                 kk = k, or k (1 - pb) for HAT, whose blank column gets k (qb - pb) instead
//   duration column (TDT):    k dur_weight (qd_n - pd_n); exact zeros when dur_weight == 0
// A student that equals the teacher gets exact zeros: both sides of every difference are computed alike.
struct KdGrad {
  float k, kk, kdur, Ls, Lt, Rs, Ds, Dt, db, ds, dr;
  int k0, k1, Ct;
  bool dur_on;
  template <int FORM, bool COLL>
  __device__ __forceinline__ float at(int c, float a, float b) const {
    if (FORM == KD_TDT && c >= Ct) return dur_on ? kdur * (__expf(a - Ds) - __expf(b - Dt)) : 0.0f;
    if (FORM == KD_HAT && c == k0) return k * db;
    if (!COLL) return kk * (__expf(a - Ls) - __expf(b - Lt));
    return kk * (c == k0 ? db : c == k1 ? ds : (dr == 0.0f ? 0.0f : dr * __expf(a - Rs)));
  }
};

// LOSS (include/ftr_kd_loss.h; plain form only): the same pass also adds the gradient of the transducer loss on the band,
//   g[c] = a_b (-(gx + gy) exp(x[c] - lse1) + 1[c == sym] gx + 1[c == blank] gy) + k_b (d kd_node / d x[c]),
// the first term being the row of band_grad_banded_kernel (mi_band.hip) operation for operation: gx / gy are the band-shaped
// occupancies of the row itself times a_b = scale.at(b), gx only where s < S.  (That kernel also drops gx at t == t_end of the
// regular type; a valid node has t < t_end.)  Its other masks cost nothing here: an invalid node has zero occupancies -- the
// band recursion stores flows only for t_begin <= t < t_end and s_begin <= s <= s_end (band_cell_flows under exactly that
// test in both kernels of mi_band.hip, the flow store of mi_band_seg.hip likewise, zeros elsewhere) -- so the zero row it
// gets without a look at its logits is its loss gradient too.  `loss` / `kd`: is the part there at all; a part with a zero
// multiplier is never read (its planes, and for kd the teacher rows), the rule of TdtMixIn::tdt / rnnt in tdt_logprobs.hip.
// With one part absent the row is the other kernel's row bit for bit.  Last rows first, as band_grad_banded_kernel and for
// its reason.
// The other forms (include/ftr_kd_loss_fact.h).  KD_HAT: the first term is the row of band_grad_banded_kernel<., ., HAT>,
//   gx (1[c == sym] - exp(x[c] - Z)) for c != blank, gy sigmoid(-x[blank]) - gx sigmoid(x[blank]) at the blank, gx = 0 where
// the symbol is the blank.  Node weights (KD_HAT, or KD_TDT with N = 0): a weight of 0 drops the distillation part of the
// row -- its planes and the teacher's row are not read -- and leaves the transducer part, which the weights never touch.
struct KdLossIn { const float* lse; const float* gxb; const float* gyb; Scale scale; bool loss, kd; };

template <typename ES, typename ET, bool VEC, int FORM, bool COLL, bool LOSS = false, typename... L>
__global__ void kd_bwd_kernel(const ES* __restrict__ x, const ET* __restrict__ y, const int32_t* __restrict__ symbols,
                              const int32_t* __restrict__ ranges, const int32_t* __restrict__ boundary,
                              const float* __restrict__ weights, int blank, float inv_tau, float dw,
                              const float* __restrict__ saved, const Scale scale, ES* __restrict__ gx, size_t rows, int T,
                              int S, int W, int N, int r, const L... li) {
  static_assert(sizeof...(L) == (LOSS ? 1 : 0), "one KdLossIn when LOSS, else nothing");   // LOSS with KD_TDT: N = 0 only (the hosts)
  constexpr bool HAT = FORM == KD_HAT;
  if (FORM == KD_PLAIN) { weights = nullptr; N = 0; }
  const int lane = threadIdx.x & 63;
  size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (LOSS) row = rows - 1 - row;
  const int Ct = W - N;
  const KdRow g = kd_row<COLL>(row, symbols, ranges, boundary, weights, blank, T, S, Ct, r);
  ES* gr = gx + row * W;
  bool zero_row = !g.valid;
  if constexpr (LOSS && FORM != KD_PLAIN) {   // a weight of 0 takes the node out of the distillation part only
    const KdLossIn& in = kd_loss_arg(li...);
    zero_row = !g.geo || !(in.loss || (in.kd && g.valid));
  }
  if (zero_row) {   // zeros, without a look at the logits
    kd_zero_row<ES, VEC>(gr, lane, W);
    return;
  }
  const ES* xr = x + row * W;
  const ET* yr = y + row * W;
  bool kd_on = true;                       // LOSS: is there a distillation part at all?
  float tgx = 0.0f, tgy = 0.0f, ttot = 0.0f, l1 = 0.0f;   // LOSS: the transducer term of this row
  int sym = -1;
  bool loss_on = false;
  if constexpr (LOSS) {
    const KdLossIn& in = kd_loss_arg(li...);
    kd_on = in.kd;
    if constexpr (FORM != KD_PLAIN) kd_on = kd_on && g.valid;
    loss_on = in.loss;
    if (loss_on) {
      const float sc = in.scale.at(g.b);
      if (g.s < S) {
        sym = symbols[(size_t)g.b * S + g.s];
        tgx = in.gxb[row] * sc;
        if (HAT) {   // band_grad_banded_kernel<., ., HAT>: the column the forward read; px is -inf where it is the blank
          sym = min(max(sym, 0), W - 1);
          if (sym == blank) tgx = 0.0f;
        }
      }
      tgy = in.gyb[row] * sc;
      ttot = HAT ? tgx : tgx + tgy;
      l1 = in.lse[row];
    }
  }
  // one column of the row: v = x[c], a = v / tau, b = y[c] / tau
  auto column = [&](const KdGrad& d, int c, float v, float a, float b) -> float {
    if constexpr (!LOSS) return d.template at<FORM, COLL>(c, a, b);
    else {
      float val = 0.0f;
      if (loss_on) {
        val = -ttot * __expf(v - l1);
        if (c == sym) val += tgx;
        if (c == blank) {
          if (HAT) {   // gy sigmoid(-x_b) - gx sigmoid(x_b), by the lane that holds the blank column
            float sp, sn;
            hat_sigmoids(v, &sp, &sn);
            val = tgy * sn - tgx * sp;
          } else {
            val += tgy;
          }
        }
      }
      if (kd_on) {
        const float kv = d.template at<FORM, COLL>(c, a, b);
        val = loss_on ? val + kv : kv;
      }
      return val;
    }
  };
  KdGrad d;
  d.k = 0.0f; d.Ls = 0.0f; d.Lt = 0.0f;
  if (kd_on) {
    d.k = scale.at(g.b) * inv_tau;
    if (weights) d.k *= g.w;
    d.Ls = saved[row];
    d.Lt = saved[rows + row];
  }
  d.kk = d.k;
  d.Rs = 0.0f; d.Ds = 0.0f; d.Dt = 0.0f; d.db = 0.0f; d.ds = 0.0f; d.dr = 0.0f; d.kdur = 0.0f;
  d.k0 = g.k0; d.k1 = g.k1; d.Ct = Ct;
  d.dur_on = FORM == KD_TDT && N > 0 && dw != 0.0f;
  if (d.dur_on) {
    const int p0 = COLL ? 4 : 2;
    d.Ds = saved[(size_t)p0 * rows + row];
    d.Dt = saved[(size_t)(p0 + 1) * rows + row];
    d.kdur = d.k * dw;
  }
  if (HAT && kd_on) {
    float qb, qn, pb, pn;
    hat_sigmoids(elem_to_float(xr[g.k0]) * inv_tau, &qb, &qn);
    hat_sigmoids(elem_to_float(yr[g.k0]) * inv_tau, &pb, &pn);
    d.db = qb - pb;
    d.kk = d.k * pn;
  }
  if (COLL && kd_on) {   // the teacher enters through its class masses only: its class logits and Rt, not its row
    d.Rs = saved[2 * rows + row];
    if (!HAT) d.db = __expf(elem_to_float(xr[g.k0]) * inv_tau - d.Ls) - __expf(elem_to_float(yr[g.k0]) * inv_tau - d.Lt);
    if (g.k1 >= 0) d.ds = __expf(elem_to_float(xr[g.k1]) * inv_tau - d.Ls) - __expf(elem_to_float(yr[g.k1]) * inv_tau - d.Lt);
    d.dr = __expf(d.Rs - d.Ls) - __expf(saved[3 * rows + row] - d.Lt);
  }
  if (VEC) {
    const int n4 = W >> 2;
    for (int i = lane; i < n4; i += 64) {
      const f4 v = load4(xr, i);
      f4 w = {0.0f, 0.0f, 0.0f, 0.0f};
      if (kd_on && (!COLL || (d.dur_on && 4 * i + 3 >= Ct))) w = load4(yr, i);   // collapsed: only the quads with a duration column
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = column(d, 4 * i + e, v[e], v[e] * inv_tau, w[e] * inv_tau);
      store4(gr, i, o);
    }
  } else {
    for (int c = lane; c < W; c += 64) {
      const float b = (kd_on && (!COLL || (d.dur_on && c >= Ct))) ? elem_to_float(yr[c]) * inv_tau : 0.0f;
      const float v = elem_to_float(xr[c]);
      gr[c] = elem_from_float<ES>(column(d, c, v, v * inv_tau, b));
    }
  }
}

// the row form of a call: one softmax without weights is the plain form; with weights it runs as TDT with n_dur = 0
inline int kd_form(int hat, int n_dur, const float* weights) { return hat ? KD_HAT : (n_dur > 0 || weights) ? KD_TDT : KD_PLAIN; }

// The forward row kernel of a call.  lo: the loss-carrying instantiation with this output (n_dur must be 0), nullptr: the
// kernel as it is without it.
int kd_fwd_rows(const char* name, int form, const void* logits, int dtype, const void* teacher, int teacher_dtype,
                const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, int collapsed, int n_dur,
                float dur_weight, const float* weights, float* node, float* saved, const KdLossOut* lo, const KdLaunch& kl, int T,
                int S, int W, int r, hipStream_t st) {
  const size_t rows = kl.rows;
  const float inv_tau = kl.inv_tau;
  dispatch_dtype2(dtype, teacher_dtype, [&](auto stag, auto ttag) {
    using ES = typename decltype(stag)::type;
    using ET = typename decltype(ttag)::type;
    const ES* x = static_cast<const ES*>(logits);
    const ET* y = static_cast<const ET*>(teacher);
    const bool vec4 = rows_vec4<ES>(W, x) && rows_vec4<ET>(W, y);
    dispatch_among<KD_PLAIN, KD_HAT, KD_TDT>(form, [&](auto f) {
      dispatch(collapsed != 0, [&](auto coll) {
        constexpr int FORM = decltype(f)::value;
        constexpr bool COLL = decltype(coll)::value;
        if (vec4 && W <= 2048)   // both rows fit the registers of a wave: 1, 2, 4 or 8 quads of elements per lane and tensor
          dispatch_among<1, 2, 4, 8>(W <= 256 ? 1 : W <= 512 ? 2 : W <= 1024 ? 4 : 8, [&](auto n) {
            if (lo) {
              hipLaunchKernelGGL((kd_fwd_reg_kernel<ES, ET, decltype(n)::value, FORM, COLL, true, KdLossOut>), dim3(kl.blocks), dim3(64 * KD_WPB),
                                 0, st, x, y, symbols, ranges, boundary, weights, blank, inv_tau, dur_weight, node, saved, rows, T, S, W,
                                 n_dur, r, *lo);
              return;
            }
            hipLaunchKernelGGL((kd_fwd_reg_kernel<ES, ET, decltype(n)::value, FORM, COLL>), dim3(kl.blocks), dim3(64 * KD_WPB), 0, st, x, y,
                               symbols, ranges, boundary, weights, blank, inv_tau, dur_weight, node, saved, rows, T, S, W, n_dur, r);
          });
        else
          dispatch(vec4, [&](auto vec) {
            if (lo) {
              hipLaunchKernelGGL((kd_fwd_kernel<ES, ET, decltype(vec)::value, FORM, COLL, true, KdLossOut>), dim3(kl.blocks), dim3(64 * KD_WPB),
                                 0, st, x, y, symbols, ranges, boundary, weights, blank, inv_tau, dur_weight, node, saved, rows, T, S, W,
                                 n_dur, r, *lo);
              return;
            }
            hipLaunchKernelGGL((kd_fwd_kernel<ES, ET, decltype(vec)::value, FORM, COLL>), dim3(kl.blocks), dim3(64 * KD_WPB), 0, st, x, y,
                               symbols, ranges, boundary, weights, blank, inv_tau, dur_weight, node, saved, rows, T, S, W, n_dur, r);
          });
      });
    });
  });
  return check_launch(name);
}

// The backward kernel of a call.  li: the loss-carrying instantiation (n_dur must be 0), nullptr: the kernel as it is without it.
int kd_bwd_rows(const char* name, int form, const void* logits, int dtype, const void* teacher, int teacher_dtype,
                const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int blank, int collapsed, int n_dur,
                float dur_weight, const float* weights, const float* saved, Scale scale, const KdLossIn* li, void* glogits,
                const KdLaunch& kl, int T, int S, int W, int r, hipStream_t st) {
  const size_t rows = kl.rows;
  const float inv_tau = kl.inv_tau;
  dispatch_dtype2(dtype, teacher_dtype, [&](auto stag, auto ttag) {
    using ES = typename decltype(stag)::type;
    using ET = typename decltype(ttag)::type;
    const ES* x = static_cast<const ES*>(logits);
    const ET* y = static_cast<const ET*>(teacher);
    dispatch(rows_vec4<ES>(W, x, glogits) && rows_vec4<ET>(W, y), [&](auto vec) {
      dispatch_among<KD_PLAIN, KD_HAT, KD_TDT>(form, [&](auto f) {
        dispatch(collapsed != 0, [&](auto coll) {
          constexpr bool V = decltype(vec)::value, COLL = decltype(coll)::value;
          constexpr int FORM = decltype(f)::value;
          if (li) {
            hipLaunchKernelGGL((kd_bwd_kernel<ES, ET, V, FORM, COLL, true, KdLossIn>), dim3(kl.blocks), dim3(64 * KD_WPB), 0, st, x, y, symbols,
                               ranges, boundary, weights, blank, inv_tau, dur_weight, saved, scale, static_cast<ES*>(glogits), rows, T, S,
                               W, n_dur, r, *li);
            return;
          }
          hipLaunchKernelGGL((kd_bwd_kernel<ES, ET, V, FORM, COLL>), dim3(kl.blocks), dim3(64 * KD_WPB), 0, st, x, y, symbols, ranges, boundary,
                             weights, blank, inv_tau, dur_weight, saved, scale, static_cast<ES*>(glogits), rows, T, S, W, n_dur, r);
        });
      });
    });
  });
  return check_launch(name);
}

}  // namespace

// shared with csrc/pruned_kd_topk.hip
int kd_utt_sum(const float* node, float* utt, int B, int per, hipStream_t st) {
  hipLaunchKernelGGL(kd_utt_sum_kernel, dim3(B), dim3(256), 0, st, node, utt, per);
  return check_launch("pruned_kd_utt_sum");
}

int pruned_kd_fwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols,
                  const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed, int hat,
                  int n_dur, float dur_weight, const float* weights, float* node, float* saved, float* utt, int B, int T,
                  int S, int W, int r, hipStream_t st) {
  const int form = kd_form(hat, n_dur, weights);
  const char* name = form == KD_PLAIN ? "pruned_kd_fwd" : "pruned_kd_fact_fwd";   // the names the messages have always carried
  const KdLaunch kl = kd_launch(name, B, T, r, temperature);
  if (kl.done) return kl.rc;
  { const int rc = kd_fwd_rows(name, form, logits, dtype, teacher, teacher_dtype, symbols, ranges, boundary, blank, collapsed, n_dur,
                               dur_weight, weights, node, saved, nullptr, kl, T, S, W, r, st);
    if (rc != FTR_OK) return rc; }
  return kd_utt_sum(node, utt, B, T * r, st);
}

// include/ftr_kd_loss.h: the row kernel that also writes lse1, the band gather of the transducer loss, the utterance sums.
// Where the student alone may be read four elements at a time and the teacher may not, the row kernel would sum lse1 in
// another order than lse_rows does for that student; the logsumexp then runs as lse_rows' own launch, in front of the
// ordinary row kernel.
// include/ftr_kd_loss_fact.h: `hat` (lse is Z, the gather is the HAT one) and / or node weights; utt == nullptr: no utterance
// sums (the caller weights the node losses afterwards, pruned_kd_weighted_utt_sum).  Without either, ftr_kd_loss.h's call.
int pruned_band_kd_fact_fwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols,
                            const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed,
                            double delay_penalty, int modified, float* lse, float* pxb, float* pyb, float* node, float* saved,
                            float* utt, int B, int T, int S, int W, int r, int hat, const float* weights, hipStream_t st) {
  const int form = kd_form(hat, 0, weights);
  const char* name = form == KD_PLAIN ? "pruned_band_kd_fwd" : "pruned_band_kd_fact_fwd";
  const KdLaunch kl = kd_launch(name, B, T, r, temperature);
  if (kl.done) return kl.rc;
  const bool svec = dispatch_dtype(dtype, [&](auto tag) { return rows_vec4<typename decltype(tag)::type>(W, logits); });
  const bool tvec = dispatch_dtype(teacher_dtype, [&](auto tag) { return rows_vec4<typename decltype(tag)::type>(W, teacher); });
  const KdLossOut lo{lse};
  const bool fused = !svec || tvec;
  if (!fused) { const int rc = lse_rows_dtype(logits, dtype, lse, kl.rows, W, blank, hat, st); if (rc != FTR_OK) return rc; }
  { const int rc = kd_fwd_rows(name, form, logits, dtype, teacher, teacher_dtype, symbols, ranges, boundary, blank, collapsed, 0,
                               0.0f, weights, node, saved, fused ? &lo : nullptr, kl, T, S, W, r, st);
    if (rc != FTR_OK) return rc; }
  { const int rc = band_gather(logits, dtype, symbols, ranges, boundary, lse, blank, delay_penalty, pxb, pyb, B, T, S, W, r, modified, hat, st);
    if (rc != FTR_OK) return rc; }
  return utt ? kd_utt_sum(node, utt, B, T * r, st) : FTR_OK;
}

int pruned_kd_weighted_utt_sum(const float* node, const float* weights, float* utt, int B, int per, hipStream_t st) {
  hipLaunchKernelGGL(kd_utt_sum_weighted_kernel, dim3(B), dim3(256), 0, st, node, weights, utt, per);
  return check_launch("pruned_kd_weighted_utt_sum");
}

int band_node_occupancy(const float* gxb, const float* gyb, const int32_t* ranges, const int32_t* boundary, float* occ, int B,
                        int T, int S, int r, hipStream_t st) {
  const size_t rows = (size_t)B * T * r;
  if (rows == 0) return FTR_OK;
  { const int rc32 = require_rows_32bit("band_node_occupancy", rows); if (rc32 != FTR_OK) return rc32; }
  hipLaunchKernelGGL(band_node_occupancy_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, gxb, gyb, ranges, boundary,
                     occ, rows, T, S, r);
  return check_launch("band_node_occupancy");
}

int pruned_kd_bwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols,
                  const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed, int hat,
                  int n_dur, float dur_weight, const float* weights, const float* saved, Scale scale, void* glogits, int B,
                  int T, int S, int W, int r, hipStream_t st) {
  const int form = kd_form(hat, n_dur, weights);
  const char* name = form == KD_PLAIN ? "pruned_kd_bwd" : "pruned_kd_fact_bwd";
  const KdLaunch kl = kd_launch(name, B, T, r, temperature);
  if (kl.done) return kl.rc;
  return kd_bwd_rows(name, form, logits, dtype, teacher, teacher_dtype, symbols, ranges, boundary, blank, collapsed, n_dur,
                     dur_weight, weights, saved, scale, nullptr, glogits, kl, T, S, W, r, st);
}

// scale: a_b of the transducer term, kd_scale: k_b of the distillation term; a multiplier of zero: that part is not read
// (hat, weights: as in the forward)
int pruned_band_kd_fact_bwd(const void* logits, int dtype, const void* teacher, int teacher_dtype, const int32_t* symbols,
                            const int32_t* ranges, const int32_t* boundary, int blank, float temperature, int collapsed,
                            const float* lse, const float* gxb, const float* gyb, Scale scale, const float* saved, Scale kd_scale,
                            void* glogits, int B, int T, int S, int W, int r, int hat, const float* weights, hipStream_t st) {
  const int form = kd_form(hat, 0, weights);
  const char* name = form == KD_PLAIN ? "pruned_band_kd_bwd" : "pruned_band_kd_fact_bwd";
  const KdLaunch kl = kd_launch(name, B, T, r, temperature);
  if (kl.done) return kl.rc;
  const KdLossIn li{lse, gxb, gyb, scale, scale.mul != 0.0f, kd_scale.mul != 0.0f};
  // without a distillation part the teacher is not read: its alignment must not cost the student the 4-element path
  if (!li.kd) { teacher = logits; teacher_dtype = dtype; }
  return kd_bwd_rows(name, form, logits, dtype, teacher, teacher_dtype, symbols, ranges, boundary, blank, collapsed, 0, 0.0f,
                     weights, saved, kd_scale, &li, glogits, kl, T, S, W, r, st);
}

}  // namespace ftr
