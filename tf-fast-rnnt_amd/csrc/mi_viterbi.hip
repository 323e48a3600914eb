// csrc/mi_viterbi.hip -- best-path (Viterbi) alignment over the RNN-T lattice (MI355X addition, no reference
// counterpart): the recursion of mutual_information_recursion with LogAdd replaced by a select, and its backtrace.
//
//   a = p[s-1, t+off] + px[s-1, t+off]     (off = 0 regular / -1 modified; -inf where the recursion's guards say so)
//   c = p[s,   t-1]   + py[s,   t-1]
//   take_px = (a != a) || (a >= c)         (NaN propagates, ties go to the px / symbol move)
//   p[s,t]  = take_px ? a : c
//
// Every value is one float32 add and one select, so any dependency-respecting order gives the same bits.
//
// One workgroup per utterance, NW <= 16 waves.  Relative row r = s - s_begin lives in wave w = (r / 64) % NW, lane
// l = r % 64 of row strip r / (64 NW); strips run one after the other.  Wave w at step k handles the relative column
//   t = k - l - E w   (regular, E = 64 + CH - 1)        t = k - E w   (modified, E = CH - 1).
// With that skew every dependency of step k was computed at step k - 1 (lane l-1's value, through a DPP shift) except
// lane 0's: it needs lane 63 of the wave below (or the top row of the strip below) as computed at step k - CH, i.e.
// in the previous chunk of CH steps.  So the waves exchange one LDS slot of CH values per chunk and meet at one
// barrier per chunk.  The top row of a strip is carried to the next strip through the workspace.
//
// Decisions: one ballot of take_px per wave per step = one 64-bit word per (block of 64 rows, step k); the words of a
// chunk are stored together (lanes 0..CH-1, one coalesced store).  Every move of the backtrace inside a block lowers k
// by exactly one (py: t-1; px: l-1 and, regular, t / modified, t-1), so the backtrace wave holds a window of 64
// consecutive words of its block in its 64 lanes (the next lower window in flight) and walks with readlane.
#include "ftr_common.h"
#include "launch.h"
#include "mi_wave_common.h"

namespace ftr {
namespace {

constexpr int VCH = 8;               // steps per chunk (one barrier each); 16 spills under the 128-VGPR budget of 16 waves
constexpr int VMAXW = 16;            // waves per workgroup
typedef unsigned long long u64;
constexpr int kRsrcWord3 = 0x00020000;   // buffer descriptor word 3 of gfx9 (raw dword access, no swizzle)

__host__ __device__ constexpr int vit_skew(bool mod) { return mod ? VCH - 1 : 64 + VCH - 1; }

// words per block of 64 rows: the step count of the longest strip, rounded up to whole chunks
__host__ __device__ inline size_t vit_words_per_block(int T) {
  const size_t nk = (size_t)T + 1 + 63 + (size_t)vit_skew(false) * (VMAXW - 1);
  return (nk + VCH - 1) / VCH * VCH;
}
__host__ __device__ inline int vit_blocks(int S) { return (S + 1 + 63) / 64; }
inline int vit_waves(int S) { return vit_blocks(S) < VMAXW ? vit_blocks(S) : VMAXW; }

struct VitLayout {
  size_t dec_bytes, carry_off, total;
};
inline VitLayout vit_layout(int B, int S, int T) {
  VitLayout L;
  L.dec_bytes = (size_t)B * vit_blocks(S) * vit_words_per_block(T) * sizeof(u64);
  L.carry_off = L.dec_bytes;
  const bool strips = vit_blocks(S) > VMAXW;
  L.total = L.dec_bytes + (strips ? (size_t)B * 2 * (T + 1) * sizeof(float) : 0);
  return L;
}

// A raw buffer load whose whole offset is in the VGPR: a negative offset (lanes outside the rectangle) reads as
// 0xffffffff.. and is out of range.  The register copy keeps the compiler from moving a constant part of the offset into
// the instruction's immediate field, which the range check adds without wrapping (a VGPR part of -4 plus an immediate 4
// would be out of range instead of offset 0).
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t rsrc, int off) {
  asm volatile("" : "+v"(off));
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
}

struct VitOps {
  float x[VCH], y[VCH];
  float cin;   // wave 0 of a strip above the first: lane j < CH holds the strip below's top row for step j
};

template <bool MOD>
__global__ void __launch_bounds__(1024) mi_viterbi_kernel(const float* __restrict__ px, const float* __restrict__ py,
                                                          const int32_t* __restrict__ boundary, u64* __restrict__ dec,
                                                          float* __restrict__ carry, float* __restrict__ score,
                                                          int32_t* __restrict__ frames, int S, int T, int NW) {
  constexpr int E = vit_skew(MOD);
  constexpr int OFF = MOD ? -1 : 0;
  __shared__ float ring[VMAXW + 1][2][VCH];   // ring[w]: the row below wave w's lane 0, per step of a chunk
  __shared__ u64 words[VMAXW][VCH];             // the decision words of the current chunk, one per step
  __shared__ float sh_score;

  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const Bound bd = load_boundary(boundary, b, S, T);
  const int Sn = bd.se - bd.sb + 1, Tn = bd.te - bd.tb + 1;
  int32_t* fr_b = frames + (size_t)b * S;

  if (Sn <= 0 || Tn <= 0) {                     // inverted rectangle: ans = 0 as the recursion's, no path
    if (threadIdx.x == 0) score[b] = 0.0f;
    for (int s = threadIdx.x; s < S; s += blockDim.x) fr_b[s] = -1;
    return;
  }

  const int T1 = MOD ? T : T + 1;
  const size_t KW = vit_words_per_block(T);
  const int NG = vit_blocks(S);
  const int R = 64 * NW;                        // rows per strip
  const int nst = (Sn + R - 1) / R;
  // one buffer resource per operand slab of this utterance (num_records = 0 for an empty one: every load returns 0)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(S > 0 && T1 > 0 ? px + (size_t)b * S * T1 : py), 0, S > 0 && T1 > 0 ? S * T1 * 4 : 0, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(py + (size_t)b * (S + 1) * T), 0, (S + 1) * T * 4, kRsrcWord3);
  if (threadIdx.x == 0) sh_score = __builtin_nanf("");   // always overwritten: the loop below covers (Sn-1, Tn-1)
  __syncthreads();

  for (int j = 0; j < nst; ++j) {
    const int rows = min(R, Sn - j * R);
    const int nwact = (rows + 63) >> 6;
    const int nk = Tn + (MOD ? 0 : 63) + E * (nwact - 1);
    const int nch = (nk + VCH - 1) / VCH;
    const bool active = w < nwact;
    const int g = j * NW + w;                   // block of 64 rows
    const int r = j * R + 64 * w + lane;        // relative row
    int skew = (MOD ? 0 : lane) + E * w;        // t = k - skew
    asm volatile("" : "+v"(skew));              // a per-lane value: keeps the per-step guards out of scalar registers
    u64* dec_g = dec + ((size_t)b * NG + g) * KW;
    const float* carry_in = carry + ((size_t)b * 2 + ((j + 1) & 1)) * (T + 1);   // written by strip j - 1
    float* carry_out = carry + ((size_t)b * 2 + (j & 1)) * (T + 1);
    const bool want_cin = active && w == 0 && j > 0;
    const bool give_carry = active && w == NW - 1 && j + 1 < nst;
    // operands through buffer loads: 32-bit byte offsets, nothing to clamp -- a lane outside the rectangle may compute
    // any offset, the hardware returns 0 beyond the utterance's slab and the value is masked by the guards anyway
    const int xoff = ((bd.sb + r - 1) * T1 + bd.tb - skew + OFF) * 4;
    const int yoff = ((bd.sb + r) * T + bd.tb - skew - 1) * 4;
    const float NEG = -__builtin_inff();

    // the carry row below this strip (wave 0 of strips above the first); num_records 0 elsewhere: loads return 0
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(want_cin ? carry_in : py), 0, want_cin ? (T + 1) * 4 : 0, kRsrcWord3);
    const int coff = ((lane & (VCH - 1)) + OFF) * 4;

    // Unconditional, and the carry word first: the loads of chunk c + 1 stay in flight while chunk c computes (a load
    // behind a branch, or one consumed early, makes the wait counts cover the next chunk's loads too).
    auto load = [&](VitOps& o, int c) {
      o.cin = bload(rc, coff + 4 * VCH * c);
#pragma unroll
      for (int q = 0; q < VCH; ++q) {
        o.x[q] = bload(rx, xoff + 4 * (VCH * c + q));
        o.y[q] = bload(ry, yoff + 4 * (VCH * c + q));
      }
    };

    float p = NEG;
    auto chunk = [&](const VitOps& o, int c) {
      if (w == 0 && lane < VCH) ring[0][c & 1][lane] = want_cin ? o.cin : NEG;   // the strip below's top row
      float up0[VCH];
#pragma unroll
      for (int q = 0; q < VCH; ++q) up0[q] = (w > 0 && c == 0) ? NEG : ring[w][(w > 0 ? c - 1 : c) & 1][q];   // broadcast reads
#pragma unroll
      for (int q = 0; q < VCH; ++q) {
        const int t = VCH * c + q - skew;
        const float up = wavecfg::dpp_wave_shr1(up0[q], p);
        const float a = (r >= 1 && t + OFF >= 0) ? up + o.x[q] : NEG;
        const float cc = (t >= 1) ? p + o.y[q] : NEG;
        const bool take_px = (a != a) || (a >= cc);
        float v = take_px ? a : cc;
        if (r == 0 && t == 0) v = 0.0f;
        if (r == Sn - 1 && t == Tn - 1) sh_score = v;
        p = v;
        const u64 m = __builtin_amdgcn_ballot_w64(take_px);
        if (lane == 0) words[w][q] = m;
        if (lane == 63) ring[w + 1][c & 1][q] = v;               // for wave w + 1 in the next chunk
      }
      if (lane < VCH) {
        const int k = VCH * c + lane;
        dec_g[k] = words[w][lane];
        if (give_carry) {
          const float o63 = ring[w + 1][c & 1][lane];
          const int t = k - 63 * (MOD ? 0 : 1) - E * w;
          if (t >= 0 && t < Tn) carry_out[t] = o63;
        }
      }
    };

    VitOps A, Bq;
    load(A, 0);
    for (int c = 0; c < nch; c += 2) {
      load(Bq, c + 1);
      if (active) chunk(A, c);
      __syncthreads();
      if (c + 1 >= nch) break;
      load(A, c + 2);
      if (active) chunk(Bq, c + 1);
      __syncthreads();
    }
  }

  // ---- frames: -1 outside [s_begin, s_end); the backtrace writes the rows inside
  const float sc = sh_score;
  const bool ok = !(sc != sc) && sc != -__builtin_inff();
  if (threadIdx.x == 0) score[b] = sc;
  for (int s = threadIdx.x; s < S; s += blockDim.x)
    if (!ok || s < bd.sb || s >= bd.se) fr_b[s] = -1;
  if (!ok || w != 0 || Sn == 1) return;

  // ---- backtrace by wave 0 from (Sn-1, Tn-1) to the origin (relative coordinates)
  int r = Sn - 1, t = Tn - 1;
  int g = r >> 6, l = r & 63;
  auto kof = [&](int gg, int ll, int tt) { return tt + (MOD ? 0 : ll) + E * (gg % NW); };
  auto ld = [&](int gg, int idx) -> u64 {       // word idx of block gg in lane `lane` (0 below the block's start)
    const int i = idx + lane;
    return i >= 0 ? dec[((size_t)b * NG + gg) * KW + i] : 0ull;
  };
  int k = kof(g, l, t);
  int k0 = k - 63;
  u64 cur = ld(g, k0), nxt = ld(g, k0 - 64);
  int frv = -1;                                 // lane i: frame of row 64 g + i
  while (r > 0) {
    if (!MOD && t == 0) {                       // regular column 0: px moves only
      if (lane < l) frv = bd.tb;
      if (64 * g + lane < Sn - 1) fr_b[bd.sb + 64 * g + lane] = frv;
      for (int s = lane; s < 64 * g; s += 64) fr_b[bd.sb + s] = bd.tb;
      return;
    }
    if (MOD && t == 0) break;                   // unreachable on a finite path (p = -inf there)
    if (k < k0) { cur = nxt; k0 -= 64; nxt = ld(g, k0 - 64); }
    const int idx = k - k0;
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)cur, idx);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(cur >> 32), idx);
    const u64 word = ((u64)hi << 32) | lo;
    if ((word >> l) & 1ull) {                   // px move out of row r - 1
      const int tp = t + OFF;
      if (l > 0) frv = lane == l - 1 ? tp + bd.tb : frv;
      r -= 1; t = tp; k -= 1; l -= 1;
      if (l < 0) {                              // into the block below: flush this block's rows, then row r there
        if (64 * g + lane < Sn - 1) fr_b[bd.sb + 64 * g + lane] = frv;
        frv = lane == 63 ? tp + bd.tb : -1;
        g -= 1; l = 63;
        k = kof(g, l, t); k0 = k - 63;
        cur = ld(g, k0); nxt = ld(g, k0 - 64);
      }
    } else {
      t -= 1; k -= 1;
    }
  }
  if (r == 0 && 64 * g + lane < Sn - 1) fr_b[bd.sb + 64 * g + lane] = frv;
}

}  // namespace

size_t mi_viterbi_workspace_bytes(int B, int S, int T) {
  if (B < 0 || S < 0 || T < 0) return 0;
  return vit_layout(B, S, T).total;
}

int mi_viterbi(const float* px, const float* py, const int32_t* boundary, void* ws, size_t ws_bytes, float* score,
               int32_t* frames, int B, int S, int T, int modified, hipStream_t st) {
  if (B == 0) return FTR_OK;
  const VitLayout L = vit_layout(B, S, T);
  if (ws_bytes < L.total) {
    set_error("mutual_information_viterbi: workspace of %zu bytes is too small, %zu needed", ws_bytes, L.total);
    return FTR_ERR_INVALID_ARG;
  }
  if ((size_t)(S + 1 + 64) * (size_t)(T + 1 + 64 + VCH) * 4 >= (1ull << 31)) {   // 32-bit buffer offsets
    set_error("mutual_information_viterbi: one utterance's lattice (S=%d, T=%d) exceeds 2 GiB", S, T);
    return FTR_ERR_UNSUPPORTED;
  }
  u64* dec = static_cast<u64*>(ws);
  float* carry = reinterpret_cast<float*>(static_cast<char*>(ws) + L.carry_off);
  const int NW = vit_waves(S);
  dispatch(modified != 0, [&](auto mod) {
    hipLaunchKernelGGL(mi_viterbi_kernel<decltype(mod)::value>, dim3(B), dim3(64 * NW), 0, st, px, py, boundary, dec, carry, score, frames, S, T, NW);
  });
  return check_launch("mutual_information_viterbi");
}

}  // namespace ftr
