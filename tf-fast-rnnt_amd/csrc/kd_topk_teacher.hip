// csrc/kd_topk_teacher.hip -- the top-K teacher cache in one pass (include/ftr_kd_topk_teacher.h; MI355X addition, no
// reference counterpart), gfx950.  What pruned_kd_topk.hip READS is written here: of every row x [C] of the teacher's joiner
// logits the K <= 64 largest elements (bit for bit), their columns, and optionally `rest`, the logsumexp of everything
// else at the temperature of the call.
// The order is total, so the cache is the same bits from run to run: descending by value compared as float32, -0 = +0, every
// NaN above +inf and equal to every other NaN, and among equal values the lower column first.  Slot j holds element j of it.
//   tt_reg_kernel  one wave per row, the row in registers (C % 4 == 0, C <= 256 * NQ, NQ = 1, 2, 4, 8 quads per lane), read
//                  once with load4, every load issued before the first use
//   tt_gen_kernel  any C, any alignment: the same rounds, each re-reading the row element by element (L1/L2 after the first)
// Selection keeps no per-element state.  Every element has an ORDER WORD, a uint32 that grows with its place in the value
// order (sign-flipped float bits, -0 and NaN canonical); round j looks for the largest element strictly below round j-1's
// winner and nothing is ever overwritten or masked.
//   float32: the threshold is (word, column).  A lane keeps the best open element of its registers -- open: word below the
//            threshold's, or equal with a higher column -- walking its columns upwards and replacing on a strictly larger
//            word, so the lowest column stands; then two wave reductions: the largest word, and the lowest column among the
//            lanes that hold it.
//   16 bit:  word (16 bits) and column (< 2048: 11 bits) fit ONE key, word << 16 | (0xffff - column), unique within the row,
//            so there are no ties: one reduction per round, and the lane's scan is max(key - P) in wrapping arithmetic -- the
//            keys below P wrap to the top of the range in their own order, those at or above P fall to the bottom -- one
//            subtraction and one maximum per element.  The winner's column is read off the key.
// After K rounds winner j's column is held by lane j: lanes 0 .. K-1 store the two output rows, consecutive lanes consecutive
// elements (one coalesced store each); the value is the element itself, re-read by its lane from the line the wave just had.
// The elements that were NOT selected are exactly those still open under the last winner, so `rest` needs no mask: one wave
// maximum and one wave sum of __expf over that set, m / tau + log(sum) in float32 (a maximum of -inf or +inf is taken as 0:
// all -inf gives exactly -inf, a +inf gives +inf, an unselected NaN gives NaN through the sum).
// A frame outside `boundary` is decided from the row index before any logits load: the filler (0, j, 0) is written instead.
// No LDS, no workspace, no barrier: rows are independent.
#include "ftr_common.h"
#include "launch.h"

namespace ftr {
namespace {

constexpr int TT_WPB = 4;       // waves (rows) per block, as the sibling row kernels
constexpr int TT_REG_C = 2048;  // the longest register-resident row: 8 quads per lane
static_assert(FTR_KD_TOPK_MAX_K == 64, "winner j is held by lane j of a wave");
static_assert(TT_REG_C <= 0x10000, "the 16-bit key keeps the column in its low half");

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  return (uint32_t)wave_max_int_dpp((int)(v ^ 0x80000000u)) ^ 0x80000000u;
}
__device__ __forceinline__ int wave_min_int(int v) { return ~wave_max_int_dpp(~v); }

// the order word of a float: larger word = earlier in the order.  Real elements lie in [0x007fffff (-inf), 0xffffffff (NaN)];
// 0 is free for "no element"
__device__ __forceinline__ uint32_t order_word(float v) {
  if (v != v) return 0xffffffffu;
  if (v == 0.0f) return 0x80000000u;   // both zeros
  const uint32_t b = __builtin_bit_cast(uint32_t, v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the same on the 16 bits of the element's own format (v is its exact up-conversion): [0x007f / 0x03ff (-inf), 0xffff (NaN)]
template <typename E>
__device__ __forceinline__ uint32_t order_half(float v) {
  if (v != v) return 0xffffu;
  if (v == 0.0f) return 0x8000u;
  const uint32_t b = elem_from_float<E>(v).bits;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

// float32 rounds: an element (word, column) is OPEN under the last winner t if it comes after it in the order
struct Pick { uint32_t word; int col; };
__device__ __forceinline__ bool open_under(uint32_t word, int col, const Pick t) {
  return word < t.word || (word == t.word && col > t.col);
}
// a lane walks its columns upwards; a strictly larger word replaces, so the lowest column of equal words stands
__device__ __forceinline__ void consider(Pick& best, uint32_t word, int col, const Pick t) {
  const bool up = open_under(word, col, t) && word > best.word;
  best.word = up ? word : best.word;
  best.col = up ? col : best.col;
}
__device__ __forceinline__ Pick wave_pick(const Pick best) {
  Pick w;
  w.word = wave_max_u32(best.word);
  w.col = wave_min_int(best.word == w.word ? best.col : 0x7fffffff);
  return w;
}
constexpr Pick kAboveAll = {0xffffffffu, -1};   // every element is open under it, the NaNs too

// is row's frame outside its utterance's [t_begin, t_end)?  (rows < 2^31: 32-bit divisions)
__device__ __forceinline__ bool frame_outside(const int32_t* __restrict__ boundary, size_t row, int T, int r) {
  const unsigned bt = (unsigned)row / (unsigned)r;
  const unsigned b = bt / (unsigned)T;
  const int t = (int)(bt - b * (unsigned)T);
  return t < max(boundary[4 * b + 1], 0) || t >= min(boundary[4 * b + 3], T);
}
template <typename E>
__device__ __forceinline__ void store_filler(E* __restrict__ vr, int32_t* __restrict__ ir, float* __restrict__ rest, size_t row,
                                             int lane, int K) {
  if (lane < K) {
    vr[lane] = elem_from_float<E>(0.0f);
    ir[lane] = lane;
  }
  if (rest && lane == 0) rest[row] = 0.0f;
}
// lanes 0 .. K-1 hold the winners' columns: the two output rows
template <typename E>
__device__ __forceinline__ void store_winners(const E* __restrict__ xr, E* __restrict__ vr, int32_t* __restrict__ ir, int lane, int K,
                                              int C, int col) {
  if (lane < K) {
    col = min(max(col, 0), C - 1);   // K <= C real elements precede every other key; this only keeps the re-read in the row
    vr[lane] = xr[col];
    ir[lane] = col;
  }
}
// rest from the wave's maximum m of the open elements and their sum of exp((x - safe(m)) / tau)
__device__ __forceinline__ float safe_max(float m) { return (m == -INFINITY || m == INFINITY) ? 0.0f : m; }
__device__ __forceinline__ float open_term(bool open, float v, float m, float inv_tau) { return open ? __expf((v - m) * inv_tau) : 0.0f; }

template <typename E, int NQ>
__global__ __launch_bounds__(64 * TT_WPB) void tt_reg_kernel(const E* __restrict__ x, const int32_t* __restrict__ boundary,
                                                             E* __restrict__ values, int32_t* __restrict__ indices,
                                                             float* __restrict__ rest, float inv_tau, size_t rows, int T, int r,
                                                             int C, int K) {
  constexpr bool UNIQ = sizeof(E) == 2;   // one key per element, unique within the row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * TT_WPB + wave;
  if (row >= rows) return;
  E* vr = values + row * K;
  int32_t* ir = indices + row * K;
  if (boundary && frame_outside(boundary, row, T, r)) {
    store_filler(vr, ir, rest, row, lane, K);
    return;
  }
  const int n4 = C >> 2;
  const E* xr = x + row * C;
  const f4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  f4 v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
    v[q] = (i < n4) ? load4(xr, i) : ninf;
  }
  uint32_t key[NQ][4];   // the quads past the row: key 0 (below every element) and value -inf (nothing in `rest`)
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = lane + 64 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (UNIQ) key[q][e] = (i < n4) ? (order_half<E>(v[q][e]) << 16) | (uint32_t)(0xffff - (4 * i + e)) : 0u;
      else key[q][e] = (i < n4) ? order_word(v[q][e]) : 0u;
    }
  }
  int mine = 0;             // lane j: the column of winner j
  uint32_t P = 0u;          // UNIQ: the last winner's key (0: none yet -- nothing wraps, the plain maximum)
  Pick last = kAboveAll;    // float32: the last winner
  for (int j = 0; j < K; ++j) {
    int col;
    if constexpr (UNIQ) {
      uint32_t best = 0u;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) best = max(best, key[q][e] - P);
      }
      P += wave_max_u32(best);
      col = 0xffff - (int)(P & 0xffffu);
    } else {
      Pick best = {0u, 0};
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) consider(best, key[q][e], 4 * (lane + 64 * q) + e, last);
      }
      last = wave_pick(best);
      col = last.col;
    }
    if (lane == j) mine = col;
  }
  store_winners(xr, vr, ir, lane, K, C, mine);
  if (!rest) return;
  bool open[NQ][4];
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      open[q][e] = UNIQ ? key[q][e] < P : open_under(key[q][e], 4 * (lane + 64 * q) + e, last);
      m = fmaxf(m, open[q][e] ? v[q][e] : -INFINITY);   // a NaN does not enter the maximum; it enters the sum
    }
  }
  m = safe_max(wave_max_dpp(m));
  float s = 0.0f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s += open_term(open[q][e], v[q][e], m, inv_tau);
  }
  s = wave_sum_dpp(s);
  if (lane == 0) rest[row] = m * inv_tau + logf(s);
}

// any C and any alignment, one wave per row: K + 2 sweeps of the row, element by element
template <typename E>
__global__ __launch_bounds__(64 * TT_WPB) void tt_gen_kernel(const E* __restrict__ x, const int32_t* __restrict__ boundary,
                                                             E* __restrict__ values, int32_t* __restrict__ indices,
                                                             float* __restrict__ rest, float inv_tau, size_t rows, int T, int r,
                                                             int C, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * TT_WPB + wave;
  if (row >= rows) return;
  E* vr = values + row * K;
  int32_t* ir = indices + row * K;
  if (boundary && frame_outside(boundary, row, T, r)) {
    store_filler(vr, ir, rest, row, lane, K);
    return;
  }
  const E* xr = x + row * C;
  int mine = 0;
  Pick last = kAboveAll;
  for (int j = 0; j < K; ++j) {
    Pick best = {0u, 0};
    for (int c = lane; c < C; c += 64) consider(best, order_word(elem_to_float(xr[c])), c, last);
    last = wave_pick(best);
    if (lane == j) mine = last.col;
  }
  store_winners(xr, vr, ir, lane, K, C, mine);
  if (!rest) return;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) {
    const float v = elem_to_float(xr[c]);
    m = fmaxf(m, open_under(order_word(v), c, last) ? v : -INFINITY);
  }
  m = safe_max(wave_max_dpp(m));
  float s = 0.0f;
  for (int c0 = 4 * lane; c0 < C; c0 += 256) {   // a lane sums the columns tt_reg_kernel gives it, in its order: the same bits
    for (int c = c0; c < min(c0 + 4, C); ++c) {
      const float v = elem_to_float(xr[c]);
      s += open_term(open_under(order_word(v), c, last), v, m, inv_tau);
    }
  }
  s = wave_sum_dpp(s);
  if (lane == 0) rest[row] = m * inv_tau + logf(s);
}

}  // namespace

int kd_teacher_topk(const void* logits, int dtype, const int32_t* boundary, void* values, int32_t* indices, float* rest,
                    float temperature, int T, int r, size_t rows, int C, int K, hipStream_t st) {
  const char* name = "kd_topk_teacher";
  if (rows == 0) return FTR_OK;
  { const int rc = require_rows_32bit(name, rows); if (rc != FTR_OK) return rc; }
  const unsigned blocks = (unsigned)((rows + TT_WPB - 1) / TT_WPB);
  const float inv_tau = 1.0f / temperature;
  dispatch_dtype(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    const E* x = static_cast<const E*>(logits);
    E* out = static_cast<E*>(values);
    if (rows_vec4<E>(C, x) && C <= TT_REG_C)   // the row fits the registers of a wave: 1, 2, 4 or 8 quads of elements per lane
      dispatch_among<1, 2, 4, 8>(C <= 256 ? 1 : C <= 512 ? 2 : C <= 1024 ? 4 : 8, [&](auto n) {
        hipLaunchKernelGGL((tt_reg_kernel<E, decltype(n)::value>), dim3(blocks), dim3(64 * TT_WPB), 0, st, x, boundary, out, indices,
                           rest, inv_tau, rows, T, r, C, K);
      });
    else
      hipLaunchKernelGGL((tt_gen_kernel<E>), dim3(blocks), dim3(64 * TT_WPB), 0, st, x, boundary, out, indices, rest, inv_tau, rows,
                         T, r, C, K);
  });
  return check_launch(name);
}

}  // namespace ftr
