// csrc/pruned_kd_topk.hip -- knowledge distillation on the pruned band from a stored top-K teacher (include/ftr_kd_topk.h;
// MI355X addition, no reference counterpart), gfx950.
// The student's joiner logits x [B,T,r,C] lie on `ranges`; the teacher is a cache on the teacher's OWN band of rt rows per
// frame: K raw logits per row, their columns (int32, clamped into [0,C) here), and optionally the logsumexp R of everything
// that was not stored ("rest", at the temperature of the call; absent = -inf = the renormalised top-K form).  Node (b,t,k),
// s = ranges[b,t,k], is distilled iff it is valid as in pruned_kd.hip, its weight is not 0, and k' = s - tranges[b,t,0] lies
// in [0,rt); its teacher row is (b,t,k').  With a = x / tau, v = values / tau, I = the row's set of columns:
//   L  = logaddexp(logsumexp_k v_k, R)          p_k = exp(v_k - L), p_R = exp(R - L): no 1 - sum anywhere
//   Ls = logsumexp_c a_c, Rs = logsumexp_{c not in I} a_c   (a masked logsumexp with its own maximum)
//   loss = w (sum_k xlogy(p_k, p_k / q_k) + xlogy(p_R, p_R / q_R)),  log q_k = a[idx_k] - Ls, log q_R = Rs - Ls
//   d loss / d x_c = (w / tau) (exp(a_c - Ls) - pt_c),  pt_c = p_k at c = idx_k, p_R exp(a_c - Rs) for c not in I
//   kt_fwd_reg_kernel  one wave per row, the student row held in registers (C % 4 == 0, C <= 256 * NQ), every load issued
//                      before the first use, one pass, last rows first: kd_fwd_reg_kernel of pruned_kd.hip with half its
//                      registers -- there is no teacher row, only one entry per lane
//   kt_fwd_kernel      any C: two passes over the row (the second hits L1/L2), four elements at a time or one by one
//   kt_bwd_kernel      one streaming pass: the gradient row from x, the K entries and the three normalisers the forward
//                      saved; it writes all C columns
// Both directions spend ONE exponential per column.  Forward: only the columns outside I are summed over the row (against
// their own maximum: Rs); the columns of I are K at most, each has one owner lane that holds a[idx_k] anyway, and Ls is Rs's
// sum moved to the full maximum plus the owners' terms.  Backward: see `folded` there.  The first build of these kernels
// summed both logsumexps over the row and took both exponentials of a column in the backward: as many as the dense kernels,
// and in bfloat16 no faster than they (0.91 - 1.03 of their time at c3 - c5), the byte count notwithstanding.
// Which columns are in I is what both masked sums and the gradient ask of every column.  Each wave keeps a slot table in
// LDS, one BYTE per column of a stretch of KT_CH = 2048 columns: 0 = not stored, k + 1 = entry k.  Lane k < K writes its
// byte; the four columns of a quad are one 32-bit word, so a quad costs one LDS read next to its global load, and the byte
// says which lane's p_k the gradient takes (read from 64 floats of LDS beside the table).  A row longer than KT_CH is swept
// stretch by stretch, the table rebuilt for each.  Entries that share a column: the contract allows that only for padding
// (value -inf, p = 0), so the byte is written a second time by the lanes whose p_k > 0 -- LDS operations of one wave
// complete in order, the second write stands.  All traffic inside one wave: no block barrier, rows of a block are independent.
// A node that is not distilled is decided from ranges, tranges, boundary and the weight BEFORE any logits load; nothing of it
// is read, its node loss and normalisers are 0 and its gradient row is written as zeros.
// Saved normalisers, float32 planes of [B,T,r]: 0 = Ls, 1 = Rs, 2 = L.
// The element types of x and of the values are independent (float, bf16_t, fp16_t); the student row is read four elements
// at a time under rows_vec4, the K values always one per lane.  All arithmetic is float32; the gradient row is rounded once
// when it is stored in x's type.
#include "kd_common.h"

namespace ftr {
namespace {

constexpr int KT_CH = 2048;   // columns per slot table: the longest register-resident row
constexpr int KT_WPB = KD_WPB;   // waves (rows) per block
static_assert(FTR_KD_TOPK_MAX_K == 64, "one teacher entry per lane of a wave; the slot byte holds k + 1 <= 64");

__device__ __forceinline__ float wave_max(float v) { return wave_max_dpp(v); }
__device__ __forceinline__ float wave_sum(float v) { return wave_sum_dpp(v); }
// orders the LDS traffic of one wave in the program's order (the hardware completes it in order; this holds the compiler to it)
__device__ __forceinline__ void kt_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// what a wave knows about its row before it touches the logits: is the node distilled, its utterance, its weight (1 without
// weights) and its row of the teacher cache
struct KtRow { bool on; int b; size_t trow; float w; };
__device__ __forceinline__ KtRow kt_row(size_t row, const int32_t* __restrict__ ranges, const int32_t* __restrict__ tranges,
                                        const int32_t* __restrict__ boundary, const float* __restrict__ weights, int T, int S,
                                        int r, int rt) {
  const KdNode n = kd_node(row, ranges, boundary, weights, T, S, r);
  KtRow g;
  g.b = n.b; g.w = n.w;
  const unsigned bt = (unsigned)row / (unsigned)r;   // the frame, as kd_node splits the row index
  // the teacher's band at this frame starts at its first element, rows consecutive (as every kernel here derives s)
  const long long kp = (long long)n.s - (long long)(tranges ? tranges[(size_t)bt * rt] : ranges[(size_t)bt * r]);
  g.on = n.valid && kp >= 0 && kp < (long long)rt;
  g.trow = (size_t)bt * rt + (size_t)(g.on ? kp : 0);
  return g;
}

// this lane's entry of the teacher row: the scaled value (-inf on the lanes past K) and the clamped column
struct KtEntry { float v; int idx; bool has; };
template <typename ET>
__device__ __forceinline__ KtEntry kt_entry(const ET* __restrict__ tv, const int32_t* __restrict__ ti, size_t trow, int lane,
                                            int K, int C, float inv_tau) {
  KtEntry e = {-INFINITY, 0, lane < K};
  if (e.has) {
    e.v = elem_to_float(tv[trow * K + lane]) * inv_tau;
    e.idx = min(max(ti[trow * K + lane], 0), C - 1);   // kept inside the row, as the builders keep `symbols`
  }
  return e;
}

// The slot table of the columns [base, base + KT_CH) of a row.  strong: this lane's entry has mass (backward only).
// Returns whether this lane OWNS its column: it lies in the stretch and the byte that stands there is this lane's -- exactly
// one owner per column of I, however often the column is repeated.
__device__ __forceinline__ bool kt_build(uint32_t* tab, int lane, int base, int C, const KtEntry e, bool strong) {
  kt_wave_sync();   // the reads of the previous stretch are done
  const int nw = (min(C - base, KT_CH) + 3) >> 2;
  for (int i = lane; i < nw; i += 64) tab[i] = 0u;
  kt_wave_sync();
  unsigned char* bytes = reinterpret_cast<unsigned char*>(tab);
  const unsigned off = (unsigned)(e.idx - base);   // idx < C: inside the cleared words whenever it is inside the stretch
  const bool here = e.has && off < (unsigned)KT_CH;
  if (here) bytes[off] = (unsigned char)(lane + 1);
  kt_wave_sync();
  if (here && strong) bytes[off] = (unsigned char)(lane + 1);
  kt_wave_sync();
  return here && bytes[off] == (unsigned char)(lane + 1);
}

// every column of a row, stretch by stretch: f(a = x[c] / tau, slot byte of c); returns kt_build's ownership
template <typename ES, bool VEC, typename F>
__device__ __forceinline__ bool kt_sweep(const ES* __restrict__ xr, uint32_t* tab, int lane, int C, const KtEntry e,
                                         float inv_tau, F&& f) {
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(tab);
  bool own = false;
  for (int base = 0; base < C; base += KT_CH) {
    own = kt_build(tab, lane, base, C, e, false) || own;
    const int cols = min(C - base, KT_CH);
    if (VEC) {
      for (int i = lane; i < (cols >> 2); i += 64) {
        const f4 v = load4(xr, (base >> 2) + i);
        const uint32_t m = tab[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) f(v[k] * inv_tau, (m >> (8 * k)) & 0xffu);
      }
    } else {
      for (int c = lane; c < cols; c += 64) f(elem_to_float(xr[base + c]) * inv_tau, (uint32_t)bytes[c]);
    }
  }
  return own;
}

__device__ __forceinline__ void kt_store_off(float* __restrict__ node, float* __restrict__ saved, size_t rows, size_t row) {
  node[row] = 0.0f;
  saved[row] = 0.0f;
  saved[rows + row] = 0.0f;
  saved[2 * rows + row] = 0.0f;
}

// The end of a forward row, by every lane of the wave.  mr_raw: the maximum of the columns NOT in I (-inf: there is none);
// sr: their sum of exp(. - kd_safe_max(mr_raw)) -- the one exponential a column costs.  The columns of I are K at most and
// each has one owner lane (own; xk = a[idx_k] on lane k), so the full logsumexp takes the rest's sum as it is, moved to the
// full maximum (mr <= ms: the factor is at most 1), and adds the owners' terms.
__device__ __forceinline__ void kt_finish(float* __restrict__ node, float* __restrict__ saved, size_t rows, size_t row, int lane,
                                          float mr_raw, float sr, bool own, const KtEntry e, float xk, float R, bool weighted,
                                          float w) {
  const float mr = kd_safe_max(mr_raw);
  const float ms = kd_safe_max(fmaxf(mr_raw, wave_max(own ? xk : -INFINITY)));
  const float ss = (sr == 0.0f ? 0.0f : sr * __expf(mr - ms)) + wave_sum(own ? __expf(xk - ms) : 0.0f);
  const float Ls = ms + __logf(ss);
  const float Rs = mr + __logf(sr);   // every column stored: 0 + log 0 = -inf
  const float mt = kd_safe_max(fmaxf(wave_max(e.v), R));
  const float L = mt + __logf(wave_sum(__expf(e.v - mt)) + __expf(R - mt));
  const float lp = e.v - L;           // the lanes past K: -inf, mass 0
  float kl = wave_sum(kd_term(__expf(lp), lp - (xk - Ls)));
  const float lpr = R - L;
  kl += kd_term(__expf(lpr), lpr - (Rs - Ls));
  if (lane == 0) {
    node[row] = weighted ? kl * w : kl;
    saved[row] = Ls;
    saved[rows + row] = Rs;
    saved[2 * rows + row] = L;
  }
}

template <typename ES, typename ET, int NQ>
__global__ __launch_bounds__(64 * KT_WPB) void kt_fwd_reg_kernel(const ES* __restrict__ x, const ET* __restrict__ tv,
                                                                 const int32_t* __restrict__ ti, const int32_t* __restrict__ ranges,
                                                                 const int32_t* __restrict__ tranges, const int32_t* __restrict__ boundary,
                                                                 const float* __restrict__ rest, const float* __restrict__ weights,
                                                                 float inv_tau, float* __restrict__ node, float* __restrict__ saved,
                                                                 size_t rows, int T, int S, int C, int r, int rt, int K) {
  __shared__ uint32_t slots[KT_WPB][KT_CH / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t rowi = (size_t)blockIdx.x * KT_WPB + wave;
  if (rowi >= rows) return;
  const size_t row = rows - 1 - rowi;   // last rows first: the tail of a tensor that was just written is what the cache still holds
  const KtRow g = kt_row(row, ranges, tranges, boundary, weights, T, S, r, rt);
  if (!g.on) {
    if (lane == 0) kt_store_off(node, saved, rows, row);
    return;
  }
  const int n4 = C >> 2;
  const ES* xr = x + row * C;
  const f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  f4 v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    v[q] = (i < n4) ? load4(xr, i) : ninf;
  }
  const KtEntry e = kt_entry(tv, ti, g.trow, lane, K, C, inv_tau);
  const float xk = e.has ? elem_to_float(xr[e.idx]) * inv_tau : 0.0f;   // a line this wave is fetching anyway
  const float R = rest ? rest[g.trow] : -INFINITY;
  uint32_t* tab = slots[wave];
  const bool own = kt_build(tab, lane, 0, C, e, false);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {   // the columns of I leave the row: masked to -inf in registers, as the lanes past the row are
    const int i = lane + 64 * q;
    const uint32_t m = (i < n4) ? tab[i] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[q][k] = ((m >> (8 * k)) & 0xffu) ? -INFINITY : v[q][k] * inv_tau;
  }
  float mr = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) mr = fmaxf(fmaxf(mr, fmaxf(v[q][0], v[q][1])), fmaxf(v[q][2], v[q][3]));
  const float mr_raw = wave_max(mr);
  mr = kd_safe_max(mr_raw);
  float sr = 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sr += __expf(v[q][k] - mr);
  }
  sr = wave_sum(sr);
  kt_finish(node, saved, rows, row, lane, mr_raw, sr, own, e, xk, R, weights != nullptr, g.w);
}

// any C, one wave per row, two passes (the second hits L1/L2: a row is a few KB)
template <typename ES, typename ET, bool VEC>
__global__ __launch_bounds__(64 * KT_WPB) void kt_fwd_kernel(const ES* __restrict__ x, const ET* __restrict__ tv,
                                                             const int32_t* __restrict__ ti, const int32_t* __restrict__ ranges,
                                                             const int32_t* __restrict__ tranges, const int32_t* __restrict__ boundary,
                                                             const float* __restrict__ rest, const float* __restrict__ weights,
                                                             float inv_tau, float* __restrict__ node, float* __restrict__ saved,
                                                             size_t rows, int T, int S, int C, int r, int rt, int K) {
  __shared__ uint32_t slots[KT_WPB][KT_CH / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * KT_WPB + wave;
  if (row >= rows) return;
  const KtRow g = kt_row(row, ranges, tranges, boundary, weights, T, S, r, rt);
  if (!g.on) {
    if (lane == 0) kt_store_off(node, saved, rows, row);
    return;
  }
  const ES* xr = x + row * C;
  const KtEntry e = kt_entry(tv, ti, g.trow, lane, K, C, inv_tau);
  const float xk = e.has ? elem_to_float(xr[e.idx]) * inv_tau : 0.0f;
  const float R = rest ? rest[g.trow] : -INFINITY;
  uint32_t* tab = slots[wave];
  float mr = -INFINITY;
  const bool own = kt_sweep<ES, VEC>(xr, tab, lane, C, e, inv_tau, [&](float a, uint32_t slot) { mr = fmaxf(mr, slot ? -INFINITY : a); });
  const float mr_raw = wave_max(mr);
  mr = kd_safe_max(mr_raw);
  float sr = 0.0f;
  kt_sweep<ES, VEC>(xr, tab, lane, C, e, inv_tau, [&](float a, uint32_t slot) { sr += slot ? 0.0f : __expf(a - mr); });
  sr = wave_sum(sr);
  kt_finish(node, saved, rows, row, lane, mr_raw, sr, own, e, xk, R, weights != nullptr, g.w);
}

// d loss / d x of a row in one streaming pass; kk = upstream gradient * weight / tau
template <typename ES, typename ET, bool VEC>
__global__ __launch_bounds__(64 * KT_WPB) void kt_bwd_kernel(const ES* __restrict__ x, const ET* __restrict__ tv,
                                                             const int32_t* __restrict__ ti, const int32_t* __restrict__ ranges,
                                                             const int32_t* __restrict__ tranges, const int32_t* __restrict__ boundary,
                                                             const float* __restrict__ rest, const float* __restrict__ weights,
                                                             float inv_tau, const float* __restrict__ saved, const Scale scale,
                                                             ES* __restrict__ gx, size_t rows, int T, int S, int C, int r, int rt,
                                                             int K) {
  __shared__ uint32_t slots[KT_WPB][KT_CH / 4];
  __shared__ float mass[KT_WPB][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * KT_WPB + wave;
  if (row >= rows) return;
  const KtRow g = kt_row(row, ranges, tranges, boundary, weights, T, S, r, rt);
  ES* gr = gx + row * C;
  if (!g.on) {   // zeros, without a look at the logits or the cache
    kd_zero_row<ES, VEC>(gr, lane, C);
    return;
  }
  const ES* xr = x + row * C;
  float kk = scale.at(g.b) * inv_tau;
  if (weights) kk *= g.w;
  const float Ls = saved[row], Rs = saved[rows + row], L = saved[2 * rows + row];
  const KtEntry e = kt_entry(tv, ti, g.trow, lane, K, C, inv_tau);
  const float pk = __expf(e.v - L);                              // 0 on the lanes past K
  const float pR = rest ? __expf(rest[g.trow] - L) : 0.0f;
  uint32_t* tab = slots[wave];
  const float* pm = mass[wave];
  mass[wave][lane] = pk;   // kt_build orders it before the first read
  // A column outside I: kk (exp(a - Ls) - pR exp(a - Rs)).  The second exponential is the first times exp(Ls - Rs), the
  // same for the whole row, so the column costs one: exp(a - Ls) kc, kc = kk (1 - pR exp(Ls - Rs)) -- as long as that factor
  // is an ordinary number.  A student whose rest class has (almost) no mass (Ls - Rs >= 60, or -inf, or NaN) keeps the two.
  const bool folded = __builtin_amdgcn_readfirstlane((int)(pR == 0.0f || Ls - Rs < 60.0f)) != 0;
  const float kc = pR == 0.0f ? kk : kk * (1.0f - pR * __expf(Ls - Rs));
  auto column = [&](float a, uint32_t slot) -> float {
    const float q = __expf(a - Ls);
    if (slot) return kk * (q - pm[(slot - 1u) & 63u]);
    if (folded) return q * kc;
    return kk * (q - pR * __expf(a - Rs));
  };
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(tab);
  for (int base = 0; base < C; base += KT_CH) {
    kt_build(tab, lane, base, C, e, pk > 0.0f);
    const int cols = min(C - base, KT_CH);
    if (VEC) {
      for (int i = lane; i < (cols >> 2); i += 64) {
        const f4 v = load4(xr, (base >> 2) + i);
        const uint32_t m = tab[i];
        f4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = column(v[k] * inv_tau, (m >> (8 * k)) & 0xffu);
        store4(gr, (base >> 2) + i, o);
      }
    } else {
      for (int c = lane; c < cols; c += 64)
        gr[base + c] = elem_from_float<ES>(column(elem_to_float(xr[base + c]) * inv_tau, (uint32_t)bytes[c]));
    }
  }
}

}  // namespace

int pruned_kd_topk_fwd(const void* logits, int dtype, const void* tvalues, int teacher_dtype, const int32_t* tindices,
                       const int32_t* ranges, const int32_t* tranges, const int32_t* boundary, const float* rest,
                       const float* weights, float temperature, float* node, float* saved, float* utt, int B, int T, int S,
                       int C, int r, int rt, int K, hipStream_t st) {
  const char* name = "pruned_kd_topk_fwd";
  const KdLaunch kl = kd_launch(name, B, T, r, temperature);
  if (kl.done) return kl.rc;
  dispatch_dtype2(dtype, teacher_dtype, [&](auto stag, auto ttag) {
    using ES = typename decltype(stag)::type;
    using ET = typename decltype(ttag)::type;
    const ES* x = static_cast<const ES*>(logits);
    const ET* tv = static_cast<const ET*>(tvalues);
    const bool vec4 = rows_vec4<ES>(C, x);
    if (vec4 && C <= KT_CH)   // the row fits the registers of a wave: 1, 2, 4 or 8 quads of elements per lane
      dispatch_among<1, 2, 4, 8>(C <= 256 ? 1 : C <= 512 ? 2 : C <= 1024 ? 4 : 8, [&](auto n) {
        hipLaunchKernelGGL((kt_fwd_reg_kernel<ES, ET, decltype(n)::value>), dim3(kl.blocks), dim3(64 * KT_WPB), 0, st, x, tv, tindices,
                           ranges, tranges, boundary, rest, weights, kl.inv_tau, node, saved, kl.rows, T, S, C, r, rt, K);
      });
    else
      dispatch(vec4, [&](auto vec) {
        hipLaunchKernelGGL((kt_fwd_kernel<ES, ET, decltype(vec)::value>), dim3(kl.blocks), dim3(64 * KT_WPB), 0, st, x, tv, tindices,
                           ranges, tranges, boundary, rest, weights, kl.inv_tau, node, saved, kl.rows, T, S, C, r, rt, K);
      });
  });
  { const int rc = check_launch(name); if (rc != FTR_OK) return rc; }
  return kd_utt_sum(node, utt, B, T * r, st);
}

int pruned_kd_topk_bwd(const void* logits, int dtype, const void* tvalues, int teacher_dtype, const int32_t* tindices,
                       const int32_t* ranges, const int32_t* tranges, const int32_t* boundary, const float* rest,
                       const float* weights, float temperature, const float* saved, Scale scale, void* glogits, int B, int T,
                       int S, int C, int r, int rt, int K, hipStream_t st) {
  const char* name = "pruned_kd_topk_bwd";
  const KdLaunch kl = kd_launch(name, B, T, r, temperature);
  if (kl.done) return kl.rc;
  dispatch_dtype2(dtype, teacher_dtype, [&](auto stag, auto ttag) {
    using ES = typename decltype(stag)::type;
    using ET = typename decltype(ttag)::type;
    const ES* x = static_cast<const ES*>(logits);
    dispatch(rows_vec4<ES>(C, x, glogits), [&](auto vec) {
      hipLaunchKernelGGL((kt_bwd_kernel<ES, ET, decltype(vec)::value>), dim3(kl.blocks), dim3(64 * KT_WPB), 0, st, x,
                         static_cast<const ET*>(tvalues), tindices, ranges, tranges, boundary, rest, weights, kl.inv_tau, saved, scale,
                         static_cast<ES*>(glogits), kl.rows, T, S, C, r, rt, K);
    });
  });
  return check_launch(name);
}

}  // namespace ftr
