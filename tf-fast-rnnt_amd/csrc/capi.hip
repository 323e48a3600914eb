// csrc/capi.hip -- the extern "C" surface declared in include/ftr.h, include/ftr_lowp.h, include/ftr_prune_sum.h, include/ftr_joiner_act.h, include/ftr_kd.h, include/ftr_kd_fact.h, include/ftr_kd_loss.h, include/ftr_kd_topk.h, include/ftr_fused.h and include/ftr_live.h: argument validation and error reporting.  No
// allocation, no host synchronisation, no CPU fallback.  Built twice: into libftr_hip.so (the product: the symbols of
// ftr.h and ftr_lowp.h and nothing else) and, with -DFTR_DIAG, into the test-only _build/libftr_hip_diag.so, which adds the symbols of
// include/ftr_diag.h: the "plain" kernel family (the reference's arithmetic on the device, mi_plain.hip), its
// process-global switch, and the read-out of the trace / stamp builds.
#include "ftr_common.h"
#ifdef FTR_DIAG
#include "../../include/ftr_diag.h"
#endif
#include <stdlib.h>
#include <string.h>

namespace ftr {
namespace {
thread_local char g_err[512] = {0};
#ifdef FTR_DIAG
int g_mi_impl = -1;  // -1: not yet read from the environment
#endif

int device_ok() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no usable HIP device (%s); this library has no CPU path", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    return FTR_ERR_NO_DEVICE;
  }
  return FTR_OK;
}

#ifdef FTR_DIAG
int mi_impl() {
  if (g_mi_impl < 0) {
    const char* e = getenv("FTR_MI_IMPL");
    g_mi_impl = (e && strcmp(e, "plain") == 0) ? 1 : 0;
  }
  return g_mi_impl;
}
#else
constexpr int mi_impl() { return 0; }   // the product library has one kernel family and no switch
#endif
}  // namespace

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
void clear_error() { g_err[0] = 0; }
}  // namespace ftr

using namespace ftr;

#define FTR_REQUIRE(cond, ...)                 \
  do {                                         \
    if (!(cond)) {                             \
      set_error(__VA_ARGS__);                  \
      return FTR_ERR_INVALID_ARG;              \
    }                                          \
  } while (0)
#define FTR_TRY(expr)                          \
  do {                                         \
    const int rc_ = (expr);                    \
    if (rc_ != FTR_OK) return rc_;             \
  } while (0)

// The argument checks that many entry points share.  Each returns FTR_OK or FTR_ERR_INVALID_ARG with the error text set;
// an entry runs them in its own order (the first failing check is the reply) and touches the device only after the last.
namespace {
hipStream_t stream_of(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

int check_lattice(const char* what, int B, int S, int T) {
  FTR_REQUIRE(B >= 0 && S >= 0 && T >= 0, "%s: negative size B=%d S=%d T=%d", what, B, S, T);
  return FTR_OK;
}
int check_sizes(const char* what, bool ok) {
  FTR_REQUIRE(ok, "%s: bad sizes", what);
  return FTR_OK;
}
// terse: the wording of the backward entries, which do not print the value
int check_blank(const char* what, int blank, int C, bool terse = false) {
  if (blank >= 0 && blank < C) return FTR_OK;
  if (terse) set_error("%s: bad termination_symbol", what);
  else set_error("%s: termination_symbol %d not in [0,%d)", what, blank, C);
  return FTR_ERR_INVALID_ARG;
}
// the head of a builder entry: its sizes, the HAT twins' C >= 2, the termination symbol -- in this order
int check_builder(const char* what, bool sizes_ok, int blank, int C, bool terse = false, int hat = 0) {
  FTR_TRY(check_sizes(what, sizes_ok));
  FTR_REQUIRE(!hat || C >= 2, "%s: C = %d, HAT needs a blank and at least one other symbol", what, C);
  return check_blank(what, blank, C, terse);
}
int check_s_range(const char* what, int r, int S) {
  FTR_REQUIRE(r <= S + 1, "%s: s_range %d > S+1 = %d", what, r, S + 1);
  return FTR_OK;
}
int check_scale_stride(const char* what, int scale_stride) {
  FTR_REQUIRE(scale_stride == 0 || scale_stride == 1, "%s: scale_stride must be 0 or 1", what);
  return FTR_OK;
}
// the _dt entries: the element type code and the flags word, before everything else
int check_dtype(const char* what, int dtype, int flags) {
  FTR_REQUIRE(dtype == FTR_DTYPE_F32 || dtype == FTR_DTYPE_BF16 || dtype == FTR_DTYPE_FP16,
              "%s: unknown element type code %d (FTR_DTYPE_F32 = 0, FTR_DTYPE_BF16 = 1, FTR_DTYPE_FP16 = 2)", what, dtype);
  FTR_REQUIRE((flags & ~FTR_PRUNED_HAT) == 0, "%s: unknown bits in flags %d", what, flags);
  return FTR_OK;
}
// the last step of most entries: the pointers, and only then the device
int pointers_then_device(const char* what, bool all_there) {
  FTR_REQUIRE(all_there, "%s: null pointer", what);
  return device_ok();
}
// the workspace of the duration-lattice entries (multi-blank, TDT, TDT Viterbi): its size before the entry's null
// checks, its alignment after them
int check_ws_size(const char* what, size_t have, size_t need, const char* unit) {
  FTR_REQUIRE(have >= need, "%s: workspace of %zu %s is too small, %zu needed", what, have, unit, need);
  return FTR_OK;
}
int check_ws_aligned(const char* what, const void* workspace) {
  FTR_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", what);
  return FTR_OK;
}
}  // namespace


extern "C" {

int ftr_abi_version(void) { return 133; }
const char* ftr_package_version(void) { return "1.2"; }
const char* ftr_last_error(void) { return g_err; }

#ifdef FTR_DIAG
int ftr_set_mi_impl(int impl) {
  const int prev = mi_impl();
  g_mi_impl = (impl == 1) ? 1 : 0;
  return prev;
}
int ftr_get_mi_impl(void) { return mi_impl(); }
#endif

size_t ftr_mutual_information_workspace_floats(int B, int S, int T) {
  if (B < 0 || S < 0 || T < 0) return 0;
  // the bidirectional wavefront kernels: two ratio lattices, the cut vectors and the hand-off region
  // (mi_wave_bidir.hip); the plain family's p lattice fits in the same buffer
  return mi_bidir_workspace_floats(B, S, T);
}

size_t ftr_mutual_information_handoff_floats(int B, int S, int T) {
  if (B < 0 || S < 0 || T < 0) return 0;
  return mi_bidir_handoff_floats(B, S, T);
}

namespace {
int mi_fwd_common(const char* what, const float* px, const float* py, const int32_t* boundary, float* p, size_t p_floats,
                  int flags, float* ans, int B, int S, int T, int modified, void* stream) {
  clear_error();
  FTR_TRY(check_lattice(what, B, S, T));
  FTR_REQUIRE((flags & ~FTR_MI_WS_CLEAN) == 0, "%s: unknown flag bits 0x%x", what, flags);
  if (B == 0) return FTR_OK;
  FTR_REQUIRE(py && p && ans, "%s: null py/p/ans", what);
  FTR_REQUIRE(px || S == 0 || (modified ? T == 0 : false), "%s: null px", what);
  FTR_TRY(device_ok());
#ifdef FTR_DIAG
  if (mi_impl() == 1) {
    FTR_REQUIRE(p_floats >= (size_t)B * (S + 1) * (T + 1), "%s: workspace too small for the plain family", what);
    return mi_plain_fwd(px, py, boundary, p, ans, B, S, T, modified, stream_of(stream));
  }
#endif
  return mi_bidir_fwd(px, py, boundary, p, p_floats, flags, ans, B, S, T, modified, stream_of(stream));
}

int mi_bwd_common(const char* what, const float* px, const float* py, const int32_t* boundary, const float* p,
                  size_t p_floats, int flags, float* p_grad, float* px_grad, float* py_grad, float* ans_grad,
                  int overwrite_ans_grad, int B, int S, int T, int modified, void* stream) {
  clear_error();
  FTR_TRY(check_lattice(what, B, S, T));
  FTR_REQUIRE((flags & ~FTR_MI_WS_CLEAN) == 0, "%s: unknown flag bits 0x%x", what, flags);
  if (B == 0) return FTR_OK;
  FTR_REQUIRE(p && py_grad, "%s: null p/py_grad", what);
  FTR_REQUIRE(ans_grad || mi_impl() == 0, "%s: ans_grad may be NULL (= ones) only with the default kernel family", what);
  FTR_REQUIRE(px_grad || S == 0 || (modified && T == 0), "%s: null px_grad", what);
  FTR_TRY(device_ok());
#ifdef FTR_DIAG
  if (mi_impl() == 1) {
    FTR_REQUIRE((px || S == 0) && py, "%s: the plain family needs px and py", what);
    FTR_REQUIRE(p_grad, "%s: the plain family needs the p_grad scratch lattice", what);
    return mi_plain_bwd(px, py, boundary, p, p_grad, px_grad, py_grad, ans_grad, overwrite_ans_grad, B, S, T, modified, stream_of(stream));
  }
#endif
  return mi_bidir_bwd(boundary, p, p_floats, flags, px_grad, py_grad, ans_grad, overwrite_ans_grad, B, S, T, modified, stream_of(stream));
}
}  // namespace

int ftr_mutual_information_fwd_f32(const float* px, const float* py, const int32_t* boundary, float* p,
                                   float* ans, int B, int S, int T, int modified, void* stream) {
  return mi_fwd_common("mutual_information_fwd", px, py, boundary, p, (size_t)-1, 0, ans, B, S, T, modified, stream);
}

int ftr_mutual_information_bwd_f32(const float* px, const float* py, const int32_t* boundary,
                                   const float* p, float* p_grad, float* px_grad, float* py_grad,
                                   float* ans_grad, int overwrite_ans_grad, int B, int S, int T,
                                   int modified, void* stream) {
  return mi_bwd_common("mutual_information_bwd", px, py, boundary, p, (size_t)-1, 0, p_grad, px_grad, py_grad, ans_grad,
                       overwrite_ans_grad, B, S, T, modified, stream);
}

int ftr_mutual_information_fwd_ws_f32(const float* px, const float* py, const int32_t* boundary, float* p,
                                      size_t p_floats, int flags, float* ans, int B, int S, int T, int modified,
                                      void* stream) {
  return mi_fwd_common("mutual_information_fwd_ws", px, py, boundary, p, p_floats, flags, ans, B, S, T, modified, stream);
}

int ftr_mutual_information_bwd_ws_f32(const float* px, const float* py, const int32_t* boundary, const float* p,
                                      size_t p_floats, int flags, float* p_grad, float* px_grad, float* py_grad,
                                      float* ans_grad, int overwrite_ans_grad, int B, int S, int T, int modified,
                                      void* stream) {
  return mi_bwd_common("mutual_information_bwd_ws", px, py, boundary, p, p_floats, flags, p_grad, px_grad, py_grad, ans_grad,
                       overwrite_ans_grad, B, S, T, modified, stream);
}

int ftr_mutual_information_bwd_loss_ws_f32(const float* px, const float* py, const int32_t* boundary, const float* p,
                                           size_t p_floats, int flags, float* px_grad, float* py_grad, const float* ans,
                                           int reduction, float* loss_out, int B, int S, int T, int modified, void* stream) {
  const char* what = "mutual_information_bwd_loss_ws";
  clear_error();
  (void)px; (void)py;
  FTR_TRY(check_lattice(what, B, S, T));
  FTR_REQUIRE((flags & ~FTR_MI_WS_CLEAN) == 0, "%s: unknown flag bits 0x%x", what, flags);
  FTR_REQUIRE(reduction >= 0 && reduction <= 2, "%s: reduction %d is not 0 (none), 1 (mean) or 2 (sum)", what, reduction);
  if (B == 0) return FTR_OK;
  FTR_REQUIRE(p && py_grad && ans && loss_out, "%s: null p / py_grad / ans / loss_out", what);
  FTR_REQUIRE(px_grad || S == 0 || (modified && T == 0), "%s: null px_grad", what);
  FTR_REQUIRE(mi_impl() == 0, "%s: only with the default kernel family", what);
  FTR_TRY(device_ok());
  return mi_bidir_bwd(boundary, p, p_floats, flags, px_grad, py_grad, nullptr, 0, B, S, T, modified, stream_of(stream), ans, loss_out, reduction);
}

int ftr_mutual_information_workspace_init(float* p, size_t p_floats, int B, int S, int T, void* stream) {
  clear_error();
  FTR_REQUIRE(B >= 0 && S >= 0 && T >= 0, "mutual_information_workspace_init: negative size");
  FTR_REQUIRE(p, "mutual_information_workspace_init: null workspace");
  FTR_TRY(device_ok());
  return mi_bidir_ws_init(p, p_floats, B, S, T, stream_of(stream));
}

int ftr_mutual_information_status(const float* p, size_t p_floats, int B, int S, int T, int* status_host,
                                  long long* dirty_words_host, void* stream) {
  clear_error();
  FTR_REQUIRE(B >= 0 && S >= 0 && T >= 0, "mutual_information_status: negative size");
  FTR_REQUIRE(p && status_host, "mutual_information_status: null pointer");
  FTR_TRY(device_ok());
  return mi_bidir_status(p, p_floats, B, S, T, status_host, dirty_words_host, stream_of(stream));
}

// Best-path (Viterbi) alignment over the lattice of ftr_mutual_information_fwd_f32 (MI355X addition, no reference
// counterpart; csrc/mi_viterbi.hip).  Sizes, pointers and the workspace are checked before the device is touched.
size_t ftr_mutual_information_viterbi_workspace_bytes(int B, int S, int T) {
  return mi_viterbi_workspace_bytes(B, S, T);
}

int ftr_mutual_information_viterbi_f32(const float* px, const float* py, const int32_t* boundary, void* workspace,
                                       size_t workspace_bytes, float* score, int32_t* frames, int B, int S, int T,
                                       int modified, void* stream) {
  const char* what = "mutual_information_viterbi";
  clear_error();
  FTR_TRY(check_lattice(what, B, S, T));
  FTR_REQUIRE(modified == 0 || modified == 1, "%s: modified=%d must be 0 or 1", what, modified);
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_bytes, mi_viterbi_workspace_bytes(B, S, T), "bytes"));
  FTR_REQUIRE(workspace && score && (frames || S == 0), "%s: null workspace / score / frames", what);
  FTR_REQUIRE(py || T == 0, "%s: null py", what);
  FTR_REQUIRE(px || S == 0 || (modified && T == 0), "%s: null px", what);
  FTR_TRY(device_ok());
  return mi_viterbi(px, py, boundary, workspace, workspace_bytes, score, frames, B, S, T, modified, stream_of(stream));
}

int ftr_cummin_i32(const int32_t* in, int32_t* out, int rows, int cols, void* stream) {
  clear_error();
  FTR_REQUIRE(rows >= 0 && cols >= 0, "cummin: negative size");
  if (rows == 0 || cols == 0) return FTR_OK;
  FTR_TRY(pointers_then_device("cummin", in && out));
  return cummin_i32(in, out, rows, cols, stream_of(stream));
}

int ftr_prune_ranges_i32(const float* px_grad, const float* py_grad, const int32_t* boundary,
                         int32_t* ranges, int32_t* s_begin_scratch, int B, int S, int T, int T1,
                         int s_range, int* r_eff_out, void* stream) {
  clear_error();
  FTR_REQUIRE(B >= 0 && S >= 1 && T >= 1, "prune_ranges: need S >= 1 and T >= 1 (S=%d T=%d)", S, T);
  FTR_REQUIRE(T1 == T || T1 == T + 1, "prune_ranges: px_grad last dim %d must be T or T+1 (T=%d)", T1, T);
  FTR_REQUIRE(s_range >= 1, "prune_ranges: s_range=%d must be >= 1", s_range);
  const int r = (s_range > S) ? S + 1 : s_range;  // rnnt_loss.py:710-711
  if (r_eff_out) *r_eff_out = r;
  if (B == 0) return FTR_OK;
  FTR_REQUIRE(px_grad && py_grad && boundary && ranges && s_begin_scratch, "prune_ranges: null pointer (boundary is mandatory)");
  FTR_TRY(device_ok());
  return prune_ranges(px_grad, py_grad, boundary, ranges, s_begin_scratch, B, S, T, T1, r, stream_of(stream));
}

int ftr_do_pruning_f32(const float* am, const float* lm, const int32_t* ranges, float* am_pruned,
                       float* lm_pruned, int B, int T, int S1, int C, int r, void* stream) {
  clear_error();
  FTR_TRY(check_sizes("do_pruning", B >= 0 && T >= 0 && S1 >= 1 && C >= 0 && r >= 0));
  if ((size_t)B * T * r * C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device("do_pruning", am && lm && ranges && lm_pruned));   // am_pruned may be NULL: gather only
  return do_pruning(am, lm, ranges, am_pruned, lm_pruned, B, T, S1, C, r, stream_of(stream));
}

size_t ftr_do_pruning_bwd_workspace_bytes(int B, int T, int S1, int C, int r) {
  if (B < 0 || T < 0 || S1 < 1 || C < 0 || r < 0) return 0;
  return do_pruning_bwd_workspace_bytes(B, T, S1, C, r);
}

// the entry without a workspace and the one with (has_ws; a NULL or short workspace is the launcher's to judge)
static int do_pruning_bwd_entry(const char* what, const float* g_am_pruned, const float* g_lm_pruned, const int32_t* ranges,
                                float* d_am, float* d_lm, int B, int T, int S1, int C, int r, bool has_ws, void* workspace,
                                size_t workspace_bytes, void* stream) {
  clear_error();
  FTR_TRY(check_sizes(what, B >= 0 && T >= 0 && S1 >= 1 && C >= 0 && r >= 0));
  if ((size_t)B * C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, g_am_pruned && g_lm_pruned && ranges && d_am && d_lm));
  if (!has_ws) return do_pruning_bwd(g_am_pruned, g_lm_pruned, ranges, d_am, d_lm, B, T, S1, C, r, stream_of(stream));
  return do_pruning_bwd_ws(g_am_pruned, g_lm_pruned, ranges, d_am, d_lm, B, T, S1, C, r, workspace, workspace_bytes, stream_of(stream));
}

int ftr_do_pruning_bwd_f32(const float* g_am_pruned, const float* g_lm_pruned, const int32_t* ranges, float* d_am,
                           float* d_lm, int B, int T, int S1, int C, int r, void* stream) {
  return do_pruning_bwd_entry("do_pruning_bwd", g_am_pruned, g_lm_pruned, ranges, d_am, d_lm, B, T, S1, C, r, false, nullptr, 0, stream);
}

int ftr_do_pruning_bwd_ws_f32(const float* g_am_pruned, const float* g_lm_pruned, const int32_t* ranges, float* d_am,
                              float* d_lm, int B, int T, int S1, int C, int r, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return do_pruning_bwd_entry("do_pruning_bwd_ws", g_am_pruned, g_lm_pruned, ranges, d_am, d_lm, B, T, S1, C, r, true, workspace, workspace_bytes, stream);
}

// ---- include/ftr_prune_sum.h: the gather fused with the joiner's addition.  The element type code first, then the checks
// of the two entries above in their order and with their replies
int ftr_do_pruning_sum_dt(const void* am, const void* lm, int kind, const int32_t* ranges, void* out, int B, int T, int S1,
                          int C, int r, void* stream) {
  clear_error();
  FTR_TRY(check_dtype("do_pruning_sum_dt", kind, 0));
  FTR_TRY(check_sizes("do_pruning", B >= 0 && T >= 0 && S1 >= 1 && C >= 0 && r >= 0));
  if ((size_t)B * T * r * C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device("do_pruning", am && lm && ranges && out));
  return do_pruning_sum(am, lm, kind, ranges, out, B, T, S1, C, r, stream_of(stream));
}

int ftr_do_pruning_sum_bwd_ws_dt(const void* g_out, int kind, const int32_t* ranges, void* d_am, void* d_lm, int B, int T,
                                 int S1, int C, int r, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  FTR_TRY(check_dtype("do_pruning_sum_bwd_ws_dt", kind, 0));
  if (kind == FTR_DTYPE_F32) {   // one g for both inputs of the addition: the FUSE case of the float kernels, their bits
    const float* g = static_cast<const float*>(g_out);
    return do_pruning_bwd_entry("do_pruning_bwd_ws", g, g, ranges, static_cast<float*>(d_am), static_cast<float*>(d_lm), B, T, S1, C, r, true, workspace, workspace_bytes, stream);
  }
  const char* what = "do_pruning_bwd_ws";
  FTR_TRY(check_sizes(what, B >= 0 && T >= 0 && S1 >= 1 && C >= 0 && r >= 0));
  if ((size_t)B * C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, g_out && ranges && d_am && d_lm));
  return do_pruning_sum_bwd_ws(g_out, kind, ranges, d_am, d_lm, B, T, S1, C, r, workspace, workspace_bytes, stream_of(stream));
}

// ---- include/ftr_joiner_act.h: the same with an activation behind the addition.  The element type code, then the activation
// code, then the checks of ftr_do_pruning_f32 / ftr_do_pruning_bwd_ws_f32 in their order and with their replies
static int check_act(const char* what, int act) {
  FTR_REQUIRE(act == FTR_ACT_TANH || act == FTR_ACT_RELU, "%s: unknown activation code %d (FTR_ACT_TANH = 1, FTR_ACT_RELU = 2)", what, act);
  return FTR_OK;
}
int ftr_pruned_joiner_act_dt(const void* am, const void* lm, int kind, int act, const int32_t* ranges, void* out,
                             int B, int T, int S1, int C, int r, void* stream) {
  clear_error();
  FTR_TRY(check_dtype("pruned_joiner_act_dt", kind, 0));
  FTR_TRY(check_act("pruned_joiner_act_dt", act));
  FTR_TRY(check_sizes("do_pruning", B >= 0 && T >= 0 && S1 >= 1 && C >= 0 && r >= 0));
  if ((size_t)B * T * r * C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device("do_pruning", am && lm && ranges && out));
  return pruned_joiner_act(am, lm, kind, act, ranges, out, B, T, S1, C, r, stream_of(stream));
}

int ftr_pruned_joiner_act_bwd_ws_dt(const void* g_out, const void* out, int kind, int act, const int32_t* ranges,
                                    void* d_am, void* d_lm, int B, int T, int S1, int C, int r,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  FTR_TRY(check_dtype("pruned_joiner_act_bwd_ws_dt", kind, 0));
  FTR_TRY(check_act("pruned_joiner_act_bwd_ws_dt", act));
  const char* what = "do_pruning_bwd_ws";
  FTR_TRY(check_sizes(what, B >= 0 && T >= 0 && S1 >= 1 && C >= 0 && r >= 0));
  if ((size_t)B * C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, g_out && out && ranges && d_am && d_lm));
  return pruned_joiner_act_bwd_ws(g_out, out, kind, act, ranges, d_am, d_lm, B, T, S1, C, r, workspace, workspace_bytes, stream_of(stream));
}

// the ordinary entry point and its HAT twin (hat = 1: blank-excluded normaliser, which needs C >= 2)
static int pruned_logprobs_fwd_entry(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges,
                                     const int32_t* boundary, int termination_symbol, double delay_penalty,
                                     float* lse, float* px, float* py, int B, int T, int S, int C, int r,
                                     int modified, int hat, void* stream) {
  const char* what = hat ? "hat_pruned_logprobs_fwd" : "pruned_logprobs_fwd";
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 1 && C >= 1 && r >= 1, termination_symbol, C, false, hat));
  FTR_TRY(check_s_range(what, r, S));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && symbols && ranges && lse && px && py));
  return pruned_logprobs_fwd(logits, dtype, symbols, ranges, boundary, termination_symbol, delay_penalty, lse, px, py, B, T, S, C, r, modified, hat, stream_of(stream));
}

int ftr_pruned_logprobs_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                const int32_t* boundary, int termination_symbol, double delay_penalty,
                                float* lse, float* px, float* py, int B, int T, int S, int C, int r,
                                int modified, void* stream) {
  return pruned_logprobs_fwd_entry(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, delay_penalty, lse, px, py, B, T, S, C, r, modified, 0, stream);
}

int ftr_hat_pruned_logprobs_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                    const int32_t* boundary, int termination_symbol, double delay_penalty,
                                    float* lse, float* px, float* py, int B, int T, int S, int C, int r,
                                    int modified, void* stream) {
  return pruned_logprobs_fwd_entry(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, delay_penalty, lse, px, py, B, T, S, C, r, modified, 1, stream);
}

int ftr_pruned_logprobs_fwd_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                               const int32_t* boundary, int termination_symbol, double delay_penalty, float* lse,
                               float* px, float* py, int B, int T, int S, int C, int r, int modified, int flags,
                               void* stream) {
  clear_error();
  FTR_TRY(check_dtype("pruned_logprobs_fwd_dt", kind, flags));
  return pruned_logprobs_fwd_entry(logits, kind, symbols, ranges, boundary, termination_symbol, delay_penalty, lse, px, py, B, T, S, C, r, modified, flags & FTR_PRUNED_HAT, stream);
}

int ftr_pruned_logprobs_bwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                const int32_t* boundary, int termination_symbol, const float* lse,
                                const float* gpx, const float* gpy, const float* scale, float* glogits,
                                int B, int T, int S, int C, int r, int modified, void* stream) {
  const char* what = "pruned_logprobs_bwd";
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 1 && C >= 1 && r >= 1, termination_symbol, C));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && symbols && ranges && lse && gpx && gpy && glogits));
  return pruned_logprobs_bwd(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, lse, gpx, gpy, Scale{scale, 1, 1.0f}, glogits, B, T, S, C, r, modified, 0, stream_of(stream));
}

// rowmax_exp, _sum (rowsum) and _dot (dotvec, dot): one pass, the outputs the entry asks for
static int rowmax_exp_entry(const char* what, const float* x, float* probs, float* rowmax, float* rowsum, const float* dotvec,
                            float* dot, bool extras_there, long long rows, int C, void* stream) {
  clear_error();
  FTR_REQUIRE(rows >= 0 && C >= 0, "%s: negative size", what);
  if (rows == 0 || C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, x && probs && rowmax && extras_there));
  return simple_rowmax_exp(x, probs, rowmax, rowsum, dotvec, dot, (size_t)rows, C, stream_of(stream));
}

int ftr_rowmax_exp_f32(const float* x, float* probs, float* rowmax, long long rows, int C, void* stream) {
  return rowmax_exp_entry("rowmax_exp", x, probs, rowmax, nullptr, nullptr, nullptr, true, rows, C, stream);
}

int ftr_rowmax_exp_sum_f32(const float* x, float* probs, float* rowmax, float* rowsum, long long rows, int C,
                           void* stream) {
  return rowmax_exp_entry("rowmax_exp_sum", x, probs, rowmax, rowsum, nullptr, nullptr, rowsum != nullptr, rows, C, stream);
}

int ftr_rowmax_exp_dot_f32(const float* x, float* probs, float* rowmax, const float* dotvec, float* dot, long long rows,
                           int C, void* stream) {
  return rowmax_exp_entry("rowmax_exp_dot", x, probs, rowmax, nullptr, dotvec, dot, dotvec && dot, rows, C, stream);
}

int ftr_rowmax_exp_pair_f32(const float* x1, float* probs1, float* rowmax1, long long rows1, const float* x2, float* probs2,
                            float* rowmax2, long long rows2, int C, void* stream) {
  clear_error();
  FTR_REQUIRE(rows1 >= 0 && rows2 >= 0 && C >= 0, "rowmax_exp_pair: negative size");
  if (rows1 + rows2 == 0 || C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device("rowmax_exp_pair", (rows1 == 0 || (x1 && probs1 && rowmax1)) && (rows2 == 0 || (x2 && probs2 && rowmax2))));
  return simple_rowmax_exp_pair(x1, probs1, rowmax1, (size_t)rows1, x2, probs2, rowmax2, (size_t)rows2, C, stream_of(stream));
}

int ftr_rowdot_f32(const float* x, const float* v, float* dot, long long rows, int C, void* stream) {
  clear_error();
  FTR_REQUIRE(rows >= 0 && C >= 0, "rowdot: negative size");
  if (rows == 0) return FTR_OK;
  FTR_TRY(pointers_then_device("rowdot", dot && ((x && v) || C == 0)));
  return simple_rowdot(x, v, dot, (size_t)rows, C, stream_of(stream));
}

size_t ftr_colsum_weighted_workspace_floats(long long rows, int C) {
  return (rows < 0 || C < 0) ? 0 : simple_colsum_workspace_floats((size_t)rows, C);
}

int ftr_colsum_weighted_f32(const float* x, const float* w, float* out, float* workspace, size_t workspace_floats,
                            long long rows, int C, void* stream) {
  clear_error();
  FTR_REQUIRE(rows >= 0 && C >= 0, "colsum_weighted: negative size");
  if (C == 0) return FTR_OK;
  FTR_TRY(pointers_then_device("colsum_weighted", out && ((x && w && workspace) || rows == 0)));
  return simple_colsum_weighted(x, w, out, workspace, workspace_floats, (size_t)rows, C, stream_of(stream));
}

// ---- the simple / smoothed builder.  The smoothed entries are the simple ones with three more inputs and three scales:
// each pair shares a body, which takes the name, whether the smoothing inputs are required, and the constants to forward.
static int simple_fwd_entry(const char* what, bool smoothed, const float* am, const float* lm, const int32_t* symbols,
                            const float* prod, const float* am_max, const float* lm_max, const float* lmonly_norm,
                            const float* amonly_norm, const float* unigram_log, const int32_t* boundary,
                            int termination_symbol, double delay_penalty, float combined_scale, float lm_only_scale,
                            float am_only_scale, float* px, float* py, int B, int T, int S, int C, int modified, void* stream) {
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1, termination_symbol, C));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, am && lm && prod && am_max && lm_max && (!smoothed || (lmonly_norm && amonly_norm && unigram_log)) && py && (symbols || S == 0) && (px || S == 0)));
  return simple_logprobs_fwd(am, lm, symbols, prod, am_max, lm_max, boundary, termination_symbol, delay_penalty, lmonly_norm, amonly_norm, unigram_log, combined_scale, lm_only_scale, am_only_scale, px, py, B, T, S, C, modified, stream_of(stream));
}

int ftr_simple_logprobs_fwd_f32(const float* am, const float* lm, const int32_t* symbols, const float* prod,
                                const float* am_max, const float* lm_max, const int32_t* boundary,
                                int termination_symbol, double delay_penalty, float* px, float* py, int B, int T,
                                int S, int C, int modified, void* stream) {
  return simple_fwd_entry("simple_logprobs_fwd", false, am, lm, symbols, prod, am_max, lm_max, nullptr, nullptr, nullptr, boundary, termination_symbol, delay_penalty, 1.0f, 0.0f, 0.0f, px, py, B, T, S, C, modified, stream);
}

int ftr_smoothed_logprobs_fwd_f32(const float* am, const float* lm, const int32_t* symbols, const float* prod,
                                  const float* am_max, const float* lm_max, const float* lmonly_norm,
                                  const float* amonly_norm, const float* unigram_log, const int32_t* boundary,
                                  int termination_symbol, float combined_scale, float lm_only_scale,
                                  float am_only_scale, float* px, float* py, int B, int T, int S, int C,
                                  int modified, void* stream) {
  return simple_fwd_entry("smoothed_logprobs_fwd", true, am, lm, symbols, prod, am_max, lm_max, lmonly_norm, amonly_norm, unigram_log, boundary, termination_symbol, 0.0, combined_scale, lm_only_scale, am_only_scale, px, py, B, T, S, C, modified, stream);
}

int ftr_smoothed_logprobs_fwd_pen_f32(const float* am, const float* lm, const int32_t* symbols, const float* prod,
                                      const float* am_max, const float* lm_max, const float* lmonly_norm,
                                      const float* amonly_norm, const float* unigram_log, const int32_t* boundary,
                                      int termination_symbol, double delay_penalty, float combined_scale,
                                      float lm_only_scale, float am_only_scale, float* px, float* py, int B, int T,
                                      int S, int C, int modified, void* stream) {
  return simple_fwd_entry("smoothed_logprobs_fwd_pen", true, am, lm, symbols, prod, am_max, lm_max, lmonly_norm, amonly_norm, unigram_log, boundary, termination_symbol, delay_penalty, combined_scale, lm_only_scale, am_only_scale, px, py, B, T, S, C, modified, stream);
}

// the entries without a scale pass {NULL, stride 0, 1.0}, which passes the stride check and multiplies by one
static int bwd_w_entry(const char* what, const float* gpx, const float* gpy, const float* scale, int scale_stride,
                       float scale_mul, const float* prod, const int32_t* boundary, float combined_scale, float* W,
                       float* rsx, float* rsy, int B, int T, int S, int modified, void* stream, int32_t* live = nullptr,
                       bool want_live = false) {
  clear_error();
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, gpy && prod && W && rsx && rsy && (gpx || S == 0) && (live || !want_live)));
  return simple_logprobs_bwd_w(gpx, gpy, Scale{scale, scale_stride, scale_mul}, prod, boundary, W, rsx, rsy, combined_scale, B, T, S, modified, stream_of(stream), live);
}

int ftr_simple_logprobs_bwd_w_f32(const float* gpx, const float* gpy, const float* prod, const int32_t* boundary,
                                  float* W, float* rsx, float* rsy, int B, int T, int S, int modified, void* stream) {
  return bwd_w_entry("simple_logprobs_bwd_w", gpx, gpy, nullptr, 0, 1.0f, prod, boundary, 1.0f, W, rsx, rsy, B, T, S, modified, stream);
}

int ftr_smoothed_logprobs_bwd_w_f32(const float* gpx, const float* gpy, const float* prod, const int32_t* boundary,
                                    float combined_scale, float* W, float* rsx, float* rsy, int B, int T, int S,
                                    int modified, void* stream) {
  return bwd_w_entry("smoothed_logprobs_bwd_w", gpx, gpy, nullptr, 0, 1.0f, prod, boundary, combined_scale, W, rsx, rsy, B, T, S, modified, stream);
}

int ftr_simple_logprobs_bwd_w_scaled_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                         float scale_mul, const float* prod, const int32_t* boundary, float* W,
                                         float* rsx, float* rsy, int B, int T, int S, int modified, void* stream) {
  return bwd_w_entry("simple_logprobs_bwd_w_scaled", gpx, gpy, scale, scale_stride, scale_mul, prod, boundary, 1.0f, W, rsx, rsy, B, T, S, modified, stream);
}

int ftr_smoothed_logprobs_bwd_w_scaled_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                           float scale_mul, const float* prod, const int32_t* boundary,
                                           float combined_scale, float* W, float* rsx, float* rsy, int B, int T, int S,
                                           int modified, void* stream) {
  return bwd_w_entry("smoothed_logprobs_bwd_w_scaled", gpx, gpy, scale, scale_stride, scale_mul, prod, boundary, combined_scale, W, rsx, rsy, B, T, S, modified, stream);
}

static int bwd_am_entry(const char* what, bool smoothed, const float* gpx, const float* gpy, const float* scale,
                        int scale_stride, float scale_mul, const float* damp, const float* am_probs,
                        const int32_t* symbols, const int32_t* boundary, int termination_symbol, float direct_scale,
                        const float* unigram, const float* am_dot, float am_only_scale, float* R, float* d_am, int B,
                        int T, int S, int C, int modified, void* stream) {
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1, termination_symbol, C, true));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, gpy && damp && am_probs && d_am && (!smoothed || (unigram && am_dot && R)) && (gpx || S == 0) && (symbols || S == 0)));
  return simple_logprobs_bwd_am(gpx, gpy, Scale{scale, scale_stride, scale_mul}, damp, am_probs, symbols, boundary, termination_symbol, direct_scale, unigram, am_dot, am_only_scale, R, d_am, B, T, S, C, modified, stream_of(stream));
}

int ftr_simple_logprobs_bwd_am_f32(const float* gpx, const float* gpy, const float* damp, const float* am_probs,
                                   const int32_t* symbols, const int32_t* boundary, int termination_symbol,
                                   float* d_am, int B, int T, int S, int C, int modified, void* stream) {
  return bwd_am_entry("simple_logprobs_bwd_am", false, gpx, gpy, nullptr, 0, 1.0f, damp, am_probs, symbols, boundary, termination_symbol, 1.0f, nullptr, nullptr, 0.0f, nullptr, d_am, B, T, S, C, modified, stream);
}

int ftr_smoothed_logprobs_bwd_am_f32(const float* gpx, const float* gpy, const float* damp, const float* am_probs,
                                     const int32_t* symbols, const int32_t* boundary, int termination_symbol,
                                     float direct_scale, const float* unigram, const float* am_dot,
                                     float am_only_scale, float* R, float* d_am, int B, int T, int S, int C,
                                     int modified, void* stream) {
  return bwd_am_entry("smoothed_logprobs_bwd_am", true, gpx, gpy, nullptr, 0, 1.0f, damp, am_probs, symbols, boundary, termination_symbol, direct_scale, unigram, am_dot, am_only_scale, R, d_am, B, T, S, C, modified, stream);
}

int ftr_simple_logprobs_bwd_am_scaled_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                          float scale_mul, const float* damp, const float* am_probs,
                                          const int32_t* symbols, const int32_t* boundary, int termination_symbol,
                                          float* d_am, int B, int T, int S, int C, int modified, void* stream) {
  return bwd_am_entry("simple_logprobs_bwd_am_scaled", false, gpx, gpy, scale, scale_stride, scale_mul, damp, am_probs, symbols, boundary, termination_symbol, 1.0f, nullptr, nullptr, 0.0f, nullptr, d_am, B, T, S, C, modified, stream);
}

int ftr_smoothed_logprobs_bwd_am_scaled_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                            float scale_mul, const float* damp, const float* am_probs,
                                            const int32_t* symbols, const int32_t* boundary, int termination_symbol,
                                            float direct_scale, const float* unigram, const float* am_dot,
                                            float am_only_scale, float* R, float* d_am, int B, int T, int S, int C,
                                            int modified, void* stream) {
  return bwd_am_entry("smoothed_logprobs_bwd_am_scaled", true, gpx, gpy, scale, scale_stride, scale_mul, damp, am_probs, symbols, boundary, termination_symbol, direct_scale, unigram, am_dot, am_only_scale, R, d_am, B, T, S, C, modified, stream);
}

static int bwd_lm_entry(const char* what, bool smoothed, const float* dlmp, const float* lm_probs, const int32_t* symbols,
                        const float* rsx, const float* rsy, int termination_symbol, float direct_scale,
                        const float* row_term, const float* inv_rowsum, const float* unigram_grad, float* d_lm, int B,
                        int S, int C, void* stream) {
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && S >= 0 && C >= 1, termination_symbol, C, true));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, dlmp && lm_probs && rsx && rsy && d_lm && (!smoothed || (row_term && inv_rowsum && unigram_grad)) && (symbols || S == 0)));
  return simple_logprobs_bwd_lm(dlmp, lm_probs, symbols, rsx, rsy, termination_symbol, direct_scale, row_term, inv_rowsum, unigram_grad, d_lm, B, S, C, stream_of(stream));
}

int ftr_simple_logprobs_bwd_lm_f32(const float* dlmp, const float* lm_probs, const int32_t* symbols,
                                   const float* rsx, const float* rsy, int termination_symbol, float* d_lm, int B,
                                   int S, int C, void* stream) {
  return bwd_lm_entry("simple_logprobs_bwd_lm", false, dlmp, lm_probs, symbols, rsx, rsy, termination_symbol, 1.0f, nullptr, nullptr, nullptr, d_lm, B, S, C, stream);
}

int ftr_smoothed_logprobs_bwd_lm_f32(const float* dlmp, const float* lm_probs, const int32_t* symbols,
                                     const float* rsx, const float* rsy, int termination_symbol, float direct_scale,
                                     const float* row_term, const float* inv_rowsum, const float* unigram_grad,
                                     float* d_lm, int B, int S, int C, void* stream) {
  return bwd_lm_entry("smoothed_logprobs_bwd_lm", true, dlmp, lm_probs, symbols, rsx, rsy, termination_symbol, direct_scale, row_term, inv_rowsum, unigram_grad, d_lm, B, S, C, stream);
}

int ftr_negated_reduce_f32(const float* ans, int B, int reduction, float* out, void* stream) {
  clear_error();
  FTR_REQUIRE(B >= 1 && reduction >= 0 && reduction <= 2, "negated_reduce: bad arguments B=%d reduction=%d", B, reduction);
  FTR_TRY(pointers_then_device("negated_reduce", ans && out));
  return negated_reduce(ans, B, reduction, out, stream_of(stream));
}

static int pruned_logprobs_bwd_scaled_entry(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges,
                                            const int32_t* boundary, int termination_symbol, const float* lse,
                                            const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                            float scale_mul, void* glogits, int B, int T, int S, int C, int r,
                                            int modified, int hat, void* stream) {
  const char* what = hat ? "hat_pruned_logprobs_bwd_scaled" : "pruned_logprobs_bwd_scaled";
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1 && r >= 1, termination_symbol, C, true, hat));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse && gpy && glogits && (symbols || S == 0) && (gpx || S == 0)));
  return pruned_logprobs_bwd(logits, dtype, symbols, ranges, boundary, termination_symbol, lse, gpx, gpy, Scale{scale, scale_stride, scale_mul}, glogits, B, T, S, C, r, modified, hat, stream_of(stream));
}

int ftr_pruned_logprobs_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                       const int32_t* boundary, int termination_symbol, const float* lse,
                                       const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                       float scale_mul, float* glogits, int B, int T, int S, int C, int r,
                                       int modified, void* stream) {
  return pruned_logprobs_bwd_scaled_entry(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, lse, gpx, gpy, scale, scale_stride, scale_mul, glogits, B, T, S, C, r, modified, 0, stream);
}

int ftr_hat_pruned_logprobs_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                           const int32_t* boundary, int termination_symbol, const float* lse,
                                           const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                           float scale_mul, float* glogits, int B, int T, int S, int C, int r,
                                           int modified, void* stream) {
  return pruned_logprobs_bwd_scaled_entry(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, lse, gpx, gpy, scale, scale_stride, scale_mul, glogits, B, T, S, C, r, modified, 1, stream);
}

int ftr_pruned_logprobs_bwd_scaled_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                                      const int32_t* boundary, int termination_symbol, const float* lse,
                                      const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                      float scale_mul, void* glogits, int B, int T, int S, int C, int r, int modified,
                                      int flags, void* stream) {
  clear_error();
  FTR_TRY(check_dtype("pruned_logprobs_bwd_scaled_dt", kind, flags));
  return pruned_logprobs_bwd_scaled_entry(logits, kind, symbols, ranges, boundary, termination_symbol, lse, gpx, gpy, scale, scale_stride, scale_mul, glogits, B, T, S, C, r, modified, flags & FTR_PRUNED_HAT, stream);
}

int ftr_simple_logprobs_fused_supported(int C) { return simple_fused_supported(C); }
int ftr_simple_logprobs_fused_bwd_supported(int T, int C) { return simple_fused_bwd_supported(T, C); }

int ftr_normalizer_gemm_f32(int kind, const float* x, const float* y, float* out, int B, int T, int S1, int C, void* stream) {
  FTR_REQUIRE(B >= 0 && T >= 0 && S1 >= 0 && C >= 0, "normalizer_gemm: bad sizes");
  if ((size_t)B * T * S1 * C == 0) return FTR_OK;
  FTR_REQUIRE(x && y && out, "normalizer_gemm: null pointer");
  return normalizer_gemm(kind, x, y, out, B, T, S1, C, reinterpret_cast<hipStream_t>(stream));
}

int ftr_normalizer_gemm_choice(int kind, int B, int T, int S1, int C, int* solution, float* us, float* us_default, int* candidates) {
  return normalizer_gemm_choice(kind, B, T, S1, C, solution, us, us_default, candidates);
}

int ftr_normalizer_gemm_set_choice(int kind, int B, int T, int S1, int C, int solution) {
  return normalizer_gemm_set_choice(kind, B, T, S1, C, solution);
}

static int fused_fwd_entry(const char* what, bool smoothed, const float* am, const float* lm, const int32_t* symbols,
                           const float* am_probs, const float* lm_probs, const float* am_max, const float* lm_max,
                           const float* lmonly_norm, const float* amonly_norm, const float* unigram_log,
                           const int32_t* boundary, int termination_symbol, double delay_penalty, float combined_scale,
                           float lm_only_scale, float am_only_scale, float* px, float* py, float* prod, int B, int T,
                           int S, int C, int modified, void* stream) {
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1, termination_symbol, C));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, am && lm && am_probs && lm_probs && am_max && lm_max && (!smoothed || (lmonly_norm && amonly_norm && unigram_log)) && py && (symbols || S == 0) && (px || S == 0)));
  return simple_fused_fwd(am, lm, symbols, am_probs, lm_probs, am_max, lm_max, boundary, termination_symbol, delay_penalty, lmonly_norm, amonly_norm, unigram_log, combined_scale, lm_only_scale, am_only_scale, px, py, prod, B, T, S, C, modified, stream_of(stream));
}

int ftr_simple_logprobs_fused_fwd_f32(const float* am, const float* lm, const int32_t* symbols, const float* am_probs,
                                      const float* lm_probs, const float* am_max, const float* lm_max,
                                      const int32_t* boundary, int termination_symbol, double delay_penalty, float* px,
                                      float* py, float* prod, int B, int T, int S, int C, int modified, void* stream) {
  return fused_fwd_entry("simple_logprobs_fused_fwd", false, am, lm, symbols, am_probs, lm_probs, am_max, lm_max, nullptr, nullptr, nullptr, boundary, termination_symbol, delay_penalty, 1.0f, 0.0f, 0.0f, px, py, prod, B, T, S, C, modified, stream);
}

int ftr_smoothed_logprobs_fused_fwd_f32(const float* am, const float* lm, const int32_t* symbols, const float* am_probs,
                                        const float* lm_probs, const float* am_max, const float* lm_max,
                                        const float* lmonly_norm, const float* amonly_norm, const float* unigram_log,
                                        const int32_t* boundary, int termination_symbol, double delay_penalty,
                                        float combined_scale, float lm_only_scale, float am_only_scale, float* px,
                                        float* py, float* prod, int B, int T, int S, int C, int modified, void* stream) {
  return fused_fwd_entry("smoothed_logprobs_fused_fwd", true, am, lm, symbols, am_probs, lm_probs, am_max, lm_max, lmonly_norm, amonly_norm, unigram_log, boundary, termination_symbol, delay_penalty, combined_scale, lm_only_scale, am_only_scale, px, py, prod, B, T, S, C, modified, stream);
}

static int fused_bwd_am_entry(const char* what, bool smoothed, const float* gpx, const float* gpy, const float* scale,
                              int scale_stride, float scale_mul, const float* prod, const float* lm_probs,
                              const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                              int termination_symbol, float combined_scale, float direct_scale, const float* unigram,
                              const float* am_dot, float am_only_scale, float* R, float* d_am, int B, int T, int S, int C,
                              int modified, void* stream) {
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1, termination_symbol, C, true));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, gpy && prod && lm_probs && am_probs && d_am && (!smoothed || (unigram && am_dot && R)) && (gpx || S == 0) && (symbols || S == 0)));
  return simple_fused_bwd_am(gpx, gpy, Scale{scale, scale_stride, scale_mul}, prod, lm_probs, am_probs, symbols, boundary, termination_symbol, combined_scale, direct_scale, unigram, am_dot, am_only_scale, R, d_am, B, T, S, C, modified, stream_of(stream));
}

int ftr_simple_logprobs_fused_bwd_am_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                         float scale_mul, const float* prod, const float* lm_probs, const float* am_probs,
                                         const int32_t* symbols, const int32_t* boundary, int termination_symbol,
                                         float* d_am, int B, int T, int S, int C, int modified, void* stream) {
  return fused_bwd_am_entry("simple_logprobs_fused_bwd_am", false, gpx, gpy, scale, scale_stride, scale_mul, prod, lm_probs, am_probs, symbols, boundary, termination_symbol, 1.0f, 1.0f, nullptr, nullptr, 0.0f, nullptr, d_am, B, T, S, C, modified, stream);
}

int ftr_smoothed_logprobs_fused_bwd_am_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                           float scale_mul, const float* prod, const float* lm_probs,
                                           const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                                           int termination_symbol, float combined_scale, float direct_scale,
                                           const float* unigram, const float* am_dot, float am_only_scale, float* R,
                                           float* d_am, int B, int T, int S, int C, int modified, void* stream) {
  return fused_bwd_am_entry("smoothed_logprobs_fused_bwd_am", true, gpx, gpy, scale, scale_stride, scale_mul, prod, lm_probs, am_probs, symbols, boundary, termination_symbol, combined_scale, direct_scale, unigram, am_dot, am_only_scale, R, d_am, B, T, S, C, modified, stream);
}

// ---- include/ftr_fused.h: the fused d am kernel with W as an operand
static int fused_bwd_am_w_entry(const char* what, bool smoothed, const float* gpx, const float* gpy, const float* scale,
                                int scale_stride, float scale_mul, const float* W, const float* lm_probs,
                                const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                                int termination_symbol, float direct_scale, const float* unigram, const float* am_dot,
                                float am_only_scale, float* R, float* d_am, int B, int T, int S, int C, int modified,
                                void* stream, const int32_t* live = nullptr, bool want_live = false) {
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1, termination_symbol, C, true));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, gpy && W && lm_probs && am_probs && d_am && (!smoothed || (unigram && am_dot && R)) && (gpx || S == 0) && (symbols || S == 0) && (live || !want_live)));
  return simple_fused_bwd_am_w(gpx, gpy, Scale{scale, scale_stride, scale_mul}, W, lm_probs, am_probs, symbols, boundary, termination_symbol, direct_scale, unigram, am_dot, am_only_scale, R, d_am, B, T, S, C, modified, stream_of(stream), live);
}

int ftr_simple_logprobs_fused_bwd_am_w_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                           float scale_mul, const float* W, const float* lm_probs, const float* am_probs,
                                           const int32_t* symbols, const int32_t* boundary, int termination_symbol,
                                           float* d_am, int B, int T, int S, int C, int modified, void* stream) {
  return fused_bwd_am_w_entry("simple_logprobs_fused_bwd_am_w", false, gpx, gpy, scale, scale_stride, scale_mul, W, lm_probs, am_probs, symbols, boundary, termination_symbol, 1.0f, nullptr, nullptr, 0.0f, nullptr, d_am, B, T, S, C, modified, stream);
}

int ftr_smoothed_logprobs_fused_bwd_am_w_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                             float scale_mul, const float* W, const float* lm_probs,
                                             const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                                             int termination_symbol, float direct_scale, const float* unigram,
                                             const float* am_dot, float am_only_scale, float* R, float* d_am, int B, int T,
                                             int S, int C, int modified, void* stream) {
  return fused_bwd_am_w_entry("smoothed_logprobs_fused_bwd_am_w", true, gpx, gpy, scale, scale_stride, scale_mul, W, lm_probs, am_probs, symbols, boundary, termination_symbol, direct_scale, unigram, am_dot, am_only_scale, R, d_am, B, T, S, C, modified, stream);
}

int ftr_simple_logprobs_fused_bwd_am_w_columns(int B, int T, int C) { return simple_fused_bwd_columns(B, T, C); }

// ---- include/ftr_live.h: the W kernel with its table of live frame intervals, and the fused d am kernel that reads it
int ftr_simple_logprobs_bwd_w_live_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                       float scale_mul, const float* prod, const int32_t* boundary, float* W, float* rsx,
                                       float* rsy, int32_t* live, int B, int T, int S, int modified, void* stream) {
  return bwd_w_entry("simple_logprobs_bwd_w_live", gpx, gpy, scale, scale_stride, scale_mul, prod, boundary, 1.0f, W, rsx, rsy, B, T, S, modified, stream, live, true);
}

int ftr_smoothed_logprobs_bwd_w_live_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                         float scale_mul, const float* prod, const int32_t* boundary, float combined_scale,
                                         float* W, float* rsx, float* rsy, int32_t* live, int B, int T, int S, int modified,
                                         void* stream) {
  return bwd_w_entry("smoothed_logprobs_bwd_w_live", gpx, gpy, scale, scale_stride, scale_mul, prod, boundary, combined_scale, W, rsx, rsy, B, T, S, modified, stream, live, true);
}

int ftr_simple_logprobs_fused_bwd_am_live_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                              float scale_mul, const float* W, const int32_t* live, const float* lm_probs,
                                              const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                                              int termination_symbol, float* d_am, int B, int T, int S, int C, int modified,
                                              void* stream) {
  return fused_bwd_am_w_entry("simple_logprobs_fused_bwd_am_live", false, gpx, gpy, scale, scale_stride, scale_mul, W, lm_probs, am_probs, symbols, boundary, termination_symbol, 1.0f, nullptr, nullptr, 0.0f, nullptr, d_am, B, T, S, C, modified, stream, live, true);
}

int ftr_smoothed_logprobs_fused_bwd_am_live_f32(const float* gpx, const float* gpy, const float* scale, int scale_stride,
                                                float scale_mul, const float* W, const int32_t* live, const float* lm_probs,
                                                const float* am_probs, const int32_t* symbols, const int32_t* boundary,
                                                int termination_symbol, float direct_scale, const float* unigram,
                                                const float* am_dot, float am_only_scale, float* R, float* d_am, int B, int T,
                                                int S, int C, int modified, void* stream) {
  return fused_bwd_am_w_entry("smoothed_logprobs_fused_bwd_am_live", true, gpx, gpy, scale, scale_stride, scale_mul, W, lm_probs, am_probs, symbols, boundary, termination_symbol, direct_scale, unigram, am_dot, am_only_scale, R, d_am, B, T, S, C, modified, stream, live, true);
}

int ftr_mutual_information_band_supported(int T, int S, int r) { return mi_band_supported(T, S, r); }

static int pruned_band_fwd_entry(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                 int termination_symbol, double delay_penalty, float* lse, float* px_band, float* py_band,
                                 int B, int T, int S, int C, int r, int modified, int hat, void* stream) {
  const char* what = hat ? "hat_pruned_band_fwd" : "pruned_band_fwd";
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1 && r >= 1, termination_symbol, C, false, hat));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse && px_band && py_band && (symbols || S == 0)));
  // lse and the band gather are two launches: folding the gather into the lse pass (picking the blank / symbol entries out
  // of the registers that hold the row) was built and measured -- 93 - 95 us against 73 + 9 at c3: the extra per-row scalar
  // work (two divisions, the ranges -> symbols dependency) costs the streaming pass more than the second kernel does
  FTR_TRY(lse_rows_dtype(logits, dtype, lse, (size_t)B * T * r, C, termination_symbol, hat, stream_of(stream)));
  return band_gather(logits, dtype, symbols, ranges, boundary, lse, termination_symbol, delay_penalty, px_band, py_band, B, T, S, C, r, modified, hat, stream_of(stream));
}

int ftr_pruned_band_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                            int termination_symbol, double delay_penalty, float* lse, float* px_band, float* py_band,
                            int B, int T, int S, int C, int r, int modified, void* stream) {
  return pruned_band_fwd_entry(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, delay_penalty, lse, px_band, py_band, B, T, S, C, r, modified, 0, stream);
}

int ftr_hat_pruned_band_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                int termination_symbol, double delay_penalty, float* lse, float* px_band, float* py_band,
                                int B, int T, int S, int C, int r, int modified, void* stream) {
  return pruned_band_fwd_entry(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, delay_penalty, lse, px_band, py_band, B, T, S, C, r, modified, 1, stream);
}

int ftr_pruned_band_fwd_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                           const int32_t* boundary, int termination_symbol, double delay_penalty, float* lse,
                           float* px_band, float* py_band, int B, int T, int S, int C, int r, int modified, int flags,
                           void* stream) {
  clear_error();
  FTR_TRY(check_dtype("pruned_band_fwd_dt", kind, flags));
  return pruned_band_fwd_entry(logits, kind, symbols, ranges, boundary, termination_symbol, delay_penalty, lse, px_band, py_band, B, T, S, C, r, modified, flags & FTR_PRUNED_HAT, stream);
}

int ftr_band_ranges_check_i32(const int32_t* ranges, const int32_t* boundary, int32_t* flags, int B, int T, int r, void* stream) {
  clear_error();
  FTR_TRY(check_sizes("band_ranges_check", B >= 0 && T >= 0 && r >= 1));
  FTR_TRY(pointers_then_device("band_ranges_check", flags && (ranges || B == 0 || T == 0)));
  return band_ranges_check(ranges, boundary, flags, B, T, r, stream_of(stream));
}

int ftr_mutual_information_band_f32(const float* px_band, const float* py_band, const int32_t* ranges,
                                    const int32_t* boundary, float* ans, float* gx_band, float* gy_band, int B, int T,
                                    int S, int r, int modified, void* stream) {
  return ftr_mutual_information_band_ws_f32(px_band, py_band, ranges, boundary, nullptr, 0, ans, gx_band, gy_band, B, T, S, r, modified, stream);
}

size_t ftr_mutual_information_band_workspace_floats(int B, int T, int S, int r) {
  return (B < 0 || T < 1 || S < 0 || r < 1) ? 0 : mi_band_workspace_floats(B, T, S, r);
}

int ftr_mutual_information_band_ws_f32(const float* px_band, const float* py_band, const int32_t* ranges,
                                       const int32_t* boundary, float* workspace, size_t workspace_floats, float* ans,
                                       float* gx_band, float* gy_band, int B, int T, int S, int r, int modified,
                                       void* stream) {
  clear_error();
  FTR_TRY(check_sizes("mutual_information_band", B >= 0 && T >= 1 && S >= 0 && r >= 1));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device("mutual_information_band", px_band && py_band && ranges && ans && gx_band && gy_band));
  return mi_band(px_band, py_band, ranges, boundary, workspace, workspace_floats, ans, gx_band, gy_band, B, T, S, r, modified, stream_of(stream));
}

static int pruned_band_bwd_scaled_entry(const void* logits, int dtype, const int32_t* symbols, const int32_t* ranges,
                                        const int32_t* boundary, int termination_symbol, const float* lse,
                                        const float* gx_band, const float* gy_band, const float* scale, int scale_stride,
                                        float scale_mul, void* glogits, int B, int T, int S, int C, int r, int modified,
                                        int hat, void* stream) {
  const char* what = hat ? "hat_pruned_band_bwd_scaled" : "pruned_band_bwd_scaled";
  clear_error();
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1 && r >= 1, termination_symbol, C, true, hat));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse && gx_band && gy_band && glogits && (symbols || S == 0)));
  return band_grad_banded(logits, dtype, symbols, ranges, boundary, termination_symbol, lse, gx_band, gy_band, Scale{scale, scale_stride, scale_mul}, glogits, B, T, S, C, r, modified, hat, stream_of(stream));
}

int ftr_pruned_band_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                   const int32_t* boundary, int termination_symbol, const float* lse,
                                   const float* gx_band, const float* gy_band, const float* scale, int scale_stride,
                                   float scale_mul, float* glogits, int B, int T, int S, int C, int r, int modified,
                                   void* stream) {
  return pruned_band_bwd_scaled_entry(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, lse, gx_band, gy_band, scale, scale_stride, scale_mul, glogits, B, T, S, C, r, modified, 0, stream);
}

int ftr_hat_pruned_band_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                       const int32_t* boundary, int termination_symbol, const float* lse,
                                       const float* gx_band, const float* gy_band, const float* scale, int scale_stride,
                                       float scale_mul, float* glogits, int B, int T, int S, int C, int r, int modified,
                                       void* stream) {
  return pruned_band_bwd_scaled_entry(logits, FTR_DTYPE_F32, symbols, ranges, boundary, termination_symbol, lse, gx_band, gy_band, scale, scale_stride, scale_mul, glogits, B, T, S, C, r, modified, 1, stream);
}

int ftr_pruned_band_bwd_scaled_dt(const void* logits, int kind, const int32_t* symbols, const int32_t* ranges,
                                  const int32_t* boundary, int termination_symbol, const float* lse,
                                  const float* gx_band, const float* gy_band, const float* scale, int scale_stride,
                                  float scale_mul, void* glogits, int B, int T, int S, int C, int r, int modified,
                                  int flags, void* stream) {
  clear_error();
  FTR_TRY(check_dtype("pruned_band_bwd_scaled_dt", kind, flags));
  return pruned_band_bwd_scaled_entry(logits, kind, symbols, ranges, boundary, termination_symbol, lse, gx_band, gy_band, scale, scale_stride, scale_mul, glogits, B, T, S, C, r, modified, flags & FTR_PRUNED_HAT, stream);
}

// ---- multi-blank transducer (MI355X addition; csrc/mi_multiblank.hip, the mb_* kernels of csrc/pruned_logprobs.hip).
// D, the durations and the big-blank ids are host data and are validated first, then sizes and pointers, then the device.
namespace {
int mb_check_durations(const char* what, const int32_t* durations, int D, bool first_is_one) {
  FTR_REQUIRE(D >= 1 && D <= 8, "%s: D = %d, the number of blanks must be in 1..8", what, D);
  FTR_REQUIRE(durations, "%s: null durations", what);
  for (int j = 0; j < D; ++j) {
    FTR_REQUIRE(durations[j] >= 1 && durations[j] <= 32, "%s: durations[%d] = %d is outside 1..32", what, j, durations[j]);
    FTR_REQUIRE(j == 0 || durations[j] > durations[j - 1], "%s: durations must be strictly increasing (durations[%d] = %d after %d)",
                what, j, durations[j], durations[j - 1]);
  }
  FTR_REQUIRE(!first_is_one || durations[0] == 1, "%s: durations[0] = %d, the standard blank advances one frame", what, durations[0]);
  return FTR_OK;
}
int mb_check_ids(const char* what, const int32_t* ids, int D, int blank, int C) {
  FTR_REQUIRE(C >= 1 && blank >= 0 && blank < C, "%s: termination_symbol %d not in [0,%d)", what, blank, C);
  FTR_REQUIRE(ids || D == 1, "%s: null big_blank_ids", what);
  for (int j = 0; j + 1 < D; ++j) {
    FTR_REQUIRE(ids[j] >= 0 && ids[j] < C, "%s: big_blank_ids[%d] = %d not in [0,%d)", what, j, ids[j], C);
    FTR_REQUIRE(ids[j] != blank, "%s: big_blank_ids[%d] = %d is the termination_symbol", what, j, ids[j]);
    for (int i = 0; i < j; ++i)
      FTR_REQUIRE(ids[i] != ids[j], "%s: big_blank_ids[%d] = %d is a duplicate of big_blank_ids[%d]", what, j, ids[j], i);
  }
  return FTR_OK;
}
}  // namespace

// ---- token-and-duration transducer, TDT (MI355X addition; csrc/mi_tdt.hip, csrc/tdt_logprobs.hip).  The duration lists
// are host data and are validated first, then sizes and pointers, then the device.
namespace {
int tdt_check_list(const char* what, const char* name, const int32_t* v, int n, int nmax, int lo, int hi = 16) {
  FTR_REQUIRE(n >= 1 && n <= nmax, "%s: %s holds %d values, must be 1..%d", what, name, n, nmax);
  FTR_REQUIRE(v, "%s: null %s", what, name);
  for (int j = 0; j < n; ++j) {
    FTR_REQUIRE(v[j] >= lo && v[j] <= hi, "%s: %s[%d] = %d is outside %d..%d", what, name, j, v[j], lo, hi);
    FTR_REQUIRE(j == 0 || v[j] > v[j - 1], "%s: %s must be strictly increasing (%s[%d] = %d after %d)", what, name, name, j,
                v[j], v[j - 1]);
  }
  return FTR_OK;
}
int tdt_check_moves(const char* what, const int32_t* token_durations, int Dx, const int32_t* blank_durations, int Dy,
                    int blank_hi = 16, int max_moves = 9) {
  FTR_TRY(tdt_check_list(what, "token_durations", token_durations, Dx, 8, 0));
  FTR_TRY(tdt_check_list(what, "blank_durations", blank_durations, Dy, 8, 1, blank_hi));
  FTR_REQUIRE(Dx + Dy <= max_moves, "%s: Dx + Dy = %d moves (token_durations and blank_durations together), at most %d", what,
              Dx + Dy, max_moves);
  return FTR_OK;
}
int tdt_check_head(const char* what, const int32_t* durations, int N, double sigma, int blank, int C) {
  FTR_TRY(tdt_check_list(what, "durations", durations, N, 5, 0));
  FTR_REQUIRE(durations[N - 1] >= 1, "%s: durations holds no positive value: no move advances a frame", what);
  FTR_REQUIRE(sigma >= 0.0, "%s: sigma = %g must not be negative", what, sigma);
  FTR_REQUIRE(C >= 1 && blank >= 0 && blank < C, "%s: termination_symbol %d not in [0,%d)", what, blank, C);
  return FTR_OK;
}
}  // namespace

size_t ftr_mutual_information_multiblank_workspace_floats(int B, int S, int T) {
  return mi_multiblank_workspace_floats(B, S, T);
}

int ftr_mutual_information_multiblank_fwd_f32(const float* px, const float* py, const int32_t* boundary,
                                              const int32_t* durations, int D, float* workspace, size_t workspace_floats,
                                              float* ans, int B, int S, int T, void* stream) {
  const char* what = "mutual_information_multiblank_fwd";
  clear_error();
  FTR_TRY(mb_check_durations(what, durations, D, false));
  FTR_TRY(check_lattice(what, B, S, T));
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_floats, mi_multiblank_workspace_floats(B, S, T), "floats"));
  FTR_REQUIRE(workspace && ans && (py || T == 0) && (px || S == 0), "%s: null px / py / workspace / ans", what);
  FTR_TRY(check_ws_aligned(what, workspace));
  FTR_TRY(device_ok());
  return mi_multiblank_fwd(px, py, boundary, durations, D, workspace, workspace_floats, ans, B, S, T, stream_of(stream));
}

int ftr_mutual_information_multiblank_bwd_f32(const float* px, const float* py, const int32_t* boundary,
                                              const int32_t* durations, int D, float* workspace, size_t workspace_floats,
                                              const float* ans_grad, float* px_grad, float* py_grad, int B, int S, int T,
                                              void* stream) {
  const char* what = "mutual_information_multiblank_bwd";
  clear_error();
  FTR_TRY(mb_check_durations(what, durations, D, false));
  FTR_TRY(check_lattice(what, B, S, T));
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_floats, mi_multiblank_workspace_floats(B, S, T), "floats"));
  FTR_REQUIRE(workspace && (py || T == 0) && (px || S == 0), "%s: null px / py / workspace", what);
  FTR_REQUIRE((py_grad || T == 0) && (px_grad || S == 0), "%s: null px_grad / py_grad", what);
  FTR_TRY(check_ws_aligned(what, workspace));
  FTR_TRY(device_ok());
  return mi_multiblank_bwd(px, py, boundary, durations, D, workspace, workspace_floats, ans_grad, px_grad, py_grad, B, S, T, stream_of(stream));
}

int ftr_multiblank_pruned_logprobs_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                           const int32_t* boundary, int termination_symbol, const int32_t* big_blank_ids,
                                           const int32_t* durations, int D, double sigma, double delay_penalty, float* lse,
                                           float* px, float* py, int B, int T, int S, int C, int r, void* stream) {
  const char* what = "multiblank_pruned_logprobs_fwd";
  clear_error();
  FTR_TRY(mb_check_durations(what, durations, D, true));
  FTR_TRY(mb_check_ids(what, big_blank_ids, D, termination_symbol, C));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_s_range(what, r, S));
  FTR_REQUIRE(sigma >= 0.0, "%s: sigma = %g must not be negative", what, sigma);
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse && py && (symbols || S == 0) && (px || S == 0)));
  return multiblank_logprobs_fwd(logits, symbols, ranges, boundary, termination_symbol, big_blank_ids, durations, D, sigma,
                                 delay_penalty, lse, px, py, B, T, S, C, r, stream_of(stream));
}

int ftr_multiblank_pruned_logprobs_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                                  const int32_t* boundary, int termination_symbol,
                                                  const int32_t* big_blank_ids, const int32_t* durations, int D,
                                                  const float* lse, const float* gpx, const float* gpy, const float* scale,
                                                  int scale_stride, float scale_mul, float* glogits, int B, int T, int S,
                                                  int C, int r, void* stream) {
  const char* what = "multiblank_pruned_logprobs_bwd_scaled";
  clear_error();
  FTR_TRY(mb_check_durations(what, durations, D, true));
  FTR_TRY(mb_check_ids(what, big_blank_ids, D, termination_symbol, C));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse && gpy && glogits && (symbols || S == 0) && (gpx || S == 0)));
  return multiblank_logprobs_bwd(logits, symbols, ranges, boundary, termination_symbol, big_blank_ids, durations, D, lse, gpx,
                                 gpy, Scale{scale, scale_stride, scale_mul}, glogits, B, T, S, C, r, stream_of(stream));
}

size_t ftr_mutual_information_tdt_workspace_floats(int B, int S, int T) { return mi_tdt_workspace_floats(B, S, T); }

int ftr_mutual_information_tdt_fwd_f32(const float* px, const float* py, const int32_t* boundary,
                                       const int32_t* token_durations, int Dx, const int32_t* blank_durations, int Dy,
                                       float* workspace, size_t workspace_floats, float* ans, int B, int S, int T,
                                       void* stream) {
  const char* what = "mutual_information_tdt_fwd";
  clear_error();
  FTR_TRY(tdt_check_moves(what, token_durations, Dx, blank_durations, Dy, 16, 10));   // MAXM of mi_rowlane.h
  FTR_TRY(check_lattice(what, B, S, T));
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_floats, mi_tdt_workspace_floats(B, S, T), "floats"));
  FTR_REQUIRE(workspace && ans && (py || T == 0) && (px || S == 0), "%s: null px / py / workspace / ans", what);
  FTR_TRY(check_ws_aligned(what, workspace));
  FTR_TRY(device_ok());
  return mi_tdt_fwd(px, py, boundary, token_durations, Dx, blank_durations, Dy, workspace, workspace_floats, ans, B, S, T,
                    stream_of(stream));
}

int ftr_mutual_information_tdt_bwd_f32(const float* px, const float* py, const int32_t* boundary,
                                       const int32_t* token_durations, int Dx, const int32_t* blank_durations, int Dy,
                                       float* workspace, size_t workspace_floats, const float* ans_grad, float* px_grad,
                                       float* py_grad, int B, int S, int T, void* stream) {
  const char* what = "mutual_information_tdt_bwd";
  clear_error();
  FTR_TRY(tdt_check_moves(what, token_durations, Dx, blank_durations, Dy, 16, 10));   // MAXM of mi_rowlane.h
  FTR_TRY(check_lattice(what, B, S, T));
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_floats, mi_tdt_workspace_floats(B, S, T), "floats"));
  FTR_REQUIRE(workspace && (py || T == 0) && (px || S == 0), "%s: null px / py / workspace", what);
  FTR_REQUIRE((py_grad || T == 0) && (px_grad || S == 0), "%s: null px_grad / py_grad", what);
  FTR_TRY(check_ws_aligned(what, workspace));
  FTR_TRY(device_ok());
  return mi_tdt_bwd(px, py, boundary, token_durations, Dx, blank_durations, Dy, workspace, workspace_floats, ans_grad,
                    px_grad, py_grad, B, S, T, stream_of(stream));
}

// Best-path alignment over the TDT / multi-blank lattice (csrc/mi_viterbi_tdt.hip).  A blank may advance 32 frames here,
// as a big blank of the multi-blank builder does.
size_t ftr_mutual_information_viterbi_tdt_workspace_bytes(int B, int S, int T) {
  return mi_viterbi_tdt_workspace_bytes(B, S, T);
}

int ftr_mutual_information_viterbi_tdt_f32(const float* px, const float* py, const int32_t* boundary,
                                           const int32_t* token_durations, int Dx, const int32_t* blank_durations, int Dy,
                                           void* workspace, size_t workspace_bytes, float* score, int32_t* frames,
                                           int32_t* durations, int32_t* blank_steps, int B, int S, int T, void* stream) {
  const char* what = "mutual_information_viterbi_tdt";
  clear_error();
  FTR_TRY(tdt_check_moves(what, token_durations, Dx, blank_durations, Dy, 32));
  FTR_TRY(check_lattice(what, B, S, T));
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_bytes, mi_viterbi_tdt_workspace_bytes(B, S, T), "bytes"));
  FTR_REQUIRE(workspace && score && (py || T == 0) && (px || S == 0), "%s: null px / py / workspace / score", what);
  FTR_REQUIRE((frames && durations) || S == 0, "%s: null frames / durations", what);
  FTR_REQUIRE(blank_steps || T == 0, "%s: null blank_steps", what);
  FTR_TRY(check_ws_aligned(what, workspace));
  FTR_TRY(device_ok());
  return mi_viterbi_tdt(px, py, boundary, token_durations, Dx, blank_durations, Dy, workspace, workspace_bytes, score, frames,
                        durations, blank_steps, B, S, T, stream_of(stream));
}

int ftr_tdt_pruned_logprobs_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                    const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                    double sigma, double delay_penalty, float* lse_tok, float* lse_dur, float* px,
                                    float* py, int B, int T, int S, int C, int r, void* stream) {
  const char* what = "tdt_pruned_logprobs_fwd";
  clear_error();
  FTR_TRY(tdt_check_head(what, durations, N, sigma, termination_symbol, C));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_s_range(what, r, S));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse_tok && lse_dur && py && (symbols || S == 0) && (px || S == 0)));
  return tdt_logprobs_fwd(logits, symbols, ranges, boundary, termination_symbol, durations, N, sigma, delay_penalty, lse_tok,
                          lse_dur, px, py, B, T, S, C, r, stream_of(stream));
}

int ftr_tdt_pruned_logprobs_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                           const int32_t* boundary, int termination_symbol, const int32_t* durations,
                                           int N, double sigma, double delay_penalty, const float* lse_tok,
                                           const float* lse_dur, const float* gpx, const float* gpy, const float* scale,
                                           int scale_stride, float scale_mul, float* glogits, int B, int T, int S, int C,
                                           int r, void* stream) {
  const char* what = "tdt_pruned_logprobs_bwd_scaled";
  clear_error();
  (void)delay_penalty;   // a constant added to px: no gradient
  FTR_TRY(tdt_check_head(what, durations, N, sigma, termination_symbol, C));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse_tok && lse_dur && gpy && glogits && (symbols || S == 0) && (gpx || S == 0)));
  return tdt_logprobs_bwd(logits, symbols, ranges, boundary, termination_symbol, durations, N, lse_tok, lse_dur, gpx, gpy,
                          Scale{scale, scale_stride, scale_mul}, glogits, B, T, S, C, r, stream_of(stream));
}

// ---- include/ftr_band_tdt.h: the TDT loss on the pruned band itself (csrc/mi_band_tdt.hip, csrc/tdt_logprobs.hip)
size_t ftr_mutual_information_band_tdt_workspace_floats(int B, int T, int S, int r, int N, int Ny) {
  return mi_band_tdt_workspace_floats(B, T, S, r, N, Ny, kBandTdtDomain);
}
int ftr_mutual_information_band_tdt_supported(int T, int S, int r, int N, int Ny) {
  return mi_band_tdt_supported(T, S, r, N, Ny, kBandTdtDomain);
}

int ftr_mutual_information_band_tdt_f32(const float* px_band, const float* py_band, const int32_t* ranges,
                                        const int32_t* boundary, const int32_t* token_durations, int N,
                                        const int32_t* blank_durations, int Ny, float* workspace, size_t workspace_floats,
                                        float* ans, float* gx_band, float* gy_band, int B, int T, int S, int r,
                                        void* stream) {
  const char* what = "mutual_information_band_tdt";
  clear_error();
  FTR_TRY(tdt_check_list(what, "token_durations", token_durations, N, 5, 0));
  FTR_TRY(tdt_check_list(what, "blank_durations", blank_durations, Ny, 5, 1));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  if (!mi_band_tdt_supported(T, S, r, N, Ny, kBandTdtDomain)) {
    set_error("%s: T=%d S=%d r=%d is outside the kernel's domain (r <= 15)", what, T, S, r);
    return FTR_ERR_UNSUPPORTED;
  }
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_floats, mi_band_tdt_workspace_floats(B, T, S, r, N, Ny, kBandTdtDomain), "floats"));
  FTR_REQUIRE(px_band && py_band && ranges && workspace && ans, "%s: null px_band / py_band / ranges / workspace / ans", what);
  FTR_REQUIRE((gx_band != nullptr) == (gy_band != nullptr), "%s: gx_band and gy_band must both be given or both be null", what);
  FTR_TRY(check_ws_aligned(what, workspace));
  FTR_TRY(device_ok());
  return mi_band_tdt(px_band, py_band, ranges, boundary, token_durations, N, blank_durations, Ny, workspace, workspace_floats, ans,
                     gx_band, gy_band, B, T, S, r, kBandTdtDomain, what, stream_of(stream));
}

int ftr_tdt_pruned_band_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                double sigma, double delay_penalty, float* lse_tok, float* lse_dur, float* px_band,
                                float* py_band, int B, int T, int S, int C, int r, void* stream) {
  const char* what = "tdt_pruned_band_fwd";
  clear_error();
  FTR_TRY(tdt_check_head(what, durations, N, sigma, termination_symbol, C));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_s_range(what, r, S));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse_tok && lse_dur && px_band && py_band && (symbols || S == 0)));
  return tdt_band_fwd(logits, symbols, ranges, boundary, termination_symbol, durations, N, sigma, delay_penalty, lse_tok, lse_dur,
                      px_band, py_band, B, T, S, C, r, stream_of(stream));
}

int ftr_tdt_pruned_band_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                       const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                       double sigma, double delay_penalty, const float* lse_tok, const float* lse_dur,
                                       const float* gx_band, const float* gy_band, const float* scale, int scale_stride,
                                       float scale_mul, float* glogits, int B, int T, int S, int C, int r, void* stream) {
  const char* what = "tdt_pruned_band_bwd_scaled";
  clear_error();
  (void)delay_penalty;   // a constant added to px: no gradient
  FTR_TRY(tdt_check_head(what, durations, N, sigma, termination_symbol, C));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse_tok && lse_dur && gx_band && gy_band && glogits && (symbols || S == 0)));
  return tdt_band_bwd(logits, symbols, ranges, boundary, termination_symbol, durations, N, lse_tok, lse_dur, gx_band, gy_band,
                      Scale{scale, scale_stride, scale_mul}, glogits, B, T, S, C, r, stream_of(stream));
}

// ---- include/ftr_tdt_mix.h: the TDT loss mixed with the ordinary loss on the token head (the <MIX> kernels of
// csrc/tdt_logprobs.hip).  band: the band-shaped twin.  Checked as the TDT builders are, the new arguments after sigma.
namespace {
int tdt_mix_fwd_entry(int band, const char* what, const float* logits, const int32_t* symbols, const int32_t* ranges,
                      const int32_t* boundary, int termination_symbol, const int32_t* durations, int N, double sigma, int parts,
                      double delay_penalty, float* lse_tok, float* lse_dur, float* px, float* py, float* px0, float* py0, int B,
                      int T, int S, int C, int r, void* stream) {
  clear_error();
  FTR_TRY(tdt_check_head(what, durations, N, sigma, termination_symbol, C));
  FTR_REQUIRE(parts >= 1 && parts <= 3, "%s: parts = %d, must be 1 (the TDT planes), 2 (the ordinary planes) or 3 (both)", what, parts);
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_s_range(what, r, S));
  if (B == 0) return FTR_OK;
  const bool lat0 = !band && S == 0;    // the lattices of shape [.,S,.] are empty then
  const bool tdt_there = !(parts & FTR_TDT_MIX_TDT) || (py && (px || lat0));
  const bool rnnt_there = !(parts & FTR_TDT_MIX_RNNT) || (py0 && (px0 || lat0));
  FTR_TRY(pointers_then_device(what, logits && ranges && lse_tok && lse_dur && tdt_there && rnnt_there && (symbols || S == 0)));
  return tdt_mix_fwd(band, logits, symbols, ranges, boundary, termination_symbol, durations, N, sigma, parts, delay_penalty, lse_tok,
                     lse_dur, px, py, px0, py0, B, T, S, C, r, stream_of(stream));
}

int tdt_mix_bwd_entry(int band, const char* what, const float* logits, const int32_t* symbols, const int32_t* ranges,
                      const int32_t* boundary, int termination_symbol, const int32_t* durations, int N, double sigma,
                      const float* lse_tok, const float* lse_dur, const float* gpx, const float* gpy, const float* gpx0,
                      const float* gpy0, const float* scale, int scale_stride, float mul_tdt, float mul_rnnt, float* glogits, int B,
                      int T, int S, int C, int r, void* stream) {
  clear_error();
  FTR_TRY(tdt_check_head(what, durations, N, sigma, termination_symbol, C));
  FTR_REQUIRE(mul_tdt - mul_tdt == 0.0f && mul_rnnt - mul_rnnt == 0.0f, "%s: mul_tdt = %g and mul_rnnt = %g must be finite", what,
              (double)mul_tdt, (double)mul_rnnt);
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  const bool lat0 = !band && S == 0;
  const bool tdt_there = mul_tdt == 0.0f || (gpy && (gpx || lat0));     // a part with a zero multiplier is not read
  const bool rnnt_there = mul_rnnt == 0.0f || (gpy0 && (gpx0 || lat0));
  FTR_TRY(pointers_then_device(what, logits && ranges && lse_tok && lse_dur && tdt_there && rnnt_there && glogits && (symbols || S == 0)));
  return tdt_mix_bwd(band, logits, symbols, ranges, boundary, termination_symbol, durations, N, lse_tok, lse_dur, gpx, gpy, gpx0, gpy0,
                     Scale{scale, scale_stride, mul_tdt}, Scale{scale, scale_stride, mul_rnnt}, glogits, B, T, S, C, r,
                     stream_of(stream));
}
}  // namespace

int ftr_tdt_mix_pruned_band_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                    const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                    double sigma, int parts, double delay_penalty, float* lse_tok, float* lse_dur,
                                    float* px_band, float* py_band, float* px0_band, float* py0_band, int B, int T, int S,
                                    int C, int r, void* stream) {
  return tdt_mix_fwd_entry(1, "tdt_mix_pruned_band_fwd", logits, symbols, ranges, boundary, termination_symbol, durations, N, sigma,
                           parts, delay_penalty, lse_tok, lse_dur, px_band, py_band, px0_band, py0_band, B, T, S, C, r, stream);
}

int ftr_tdt_mix_pruned_logprobs_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                        const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                        double sigma, int parts, double delay_penalty, float* lse_tok, float* lse_dur,
                                        float* px, float* py, float* px0, float* py0, int B, int T, int S, int C, int r,
                                        void* stream) {
  return tdt_mix_fwd_entry(0, "tdt_mix_pruned_logprobs_fwd", logits, symbols, ranges, boundary, termination_symbol, durations, N,
                           sigma, parts, delay_penalty, lse_tok, lse_dur, px, py, px0, py0, B, T, S, C, r, stream);
}

int ftr_tdt_mix_pruned_band_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                           const int32_t* boundary, int termination_symbol, const int32_t* durations, int N,
                                           double sigma, double delay_penalty, const float* lse_tok, const float* lse_dur,
                                           const float* gx_band, const float* gy_band, const float* gx0_band,
                                           const float* gy0_band, const float* scale, int scale_stride, float mul_tdt,
                                           float mul_rnnt, float* glogits, int B, int T, int S, int C, int r, void* stream) {
  (void)delay_penalty;   // a constant added to px and px0: no gradient
  return tdt_mix_bwd_entry(1, "tdt_mix_pruned_band_bwd_scaled", logits, symbols, ranges, boundary, termination_symbol, durations, N,
                           sigma, lse_tok, lse_dur, gx_band, gy_band, gx0_band, gy0_band, scale, scale_stride, mul_tdt, mul_rnnt,
                           glogits, B, T, S, C, r, stream);
}

int ftr_tdt_mix_pruned_logprobs_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                               const int32_t* boundary, int termination_symbol, const int32_t* durations,
                                               int N, double sigma, double delay_penalty, const float* lse_tok,
                                               const float* lse_dur, const float* gpx, const float* gpy, const float* gpx0,
                                               const float* gpy0, const float* scale, int scale_stride, float mul_tdt,
                                               float mul_rnnt, float* glogits, int B, int T, int S, int C, int r,
                                               void* stream) {
  (void)delay_penalty;
  return tdt_mix_bwd_entry(0, "tdt_mix_pruned_logprobs_bwd_scaled", logits, symbols, ranges, boundary, termination_symbol, durations,
                           N, sigma, lse_tok, lse_dur, gpx, gpy, gpx0, gpy0, scale, scale_stride, mul_tdt, mul_rnnt, glogits, B, T, S,
                           C, r, stream);
}

// ---- include/ftr_band_multiblank.h: the multi-blank loss on the pruned band itself (the multi-blank domain of
// csrc/mi_band_tdt.hip, the band-shaped mb_* kernels of csrc/pruned_logprobs.hip)
size_t ftr_mutual_information_band_multiblank_workspace_floats(int B, int T, int S, int r, int D) {
  return mi_band_tdt_workspace_floats(B, T, S, r, 1, D, kBandMultiblankDomain);
}
int ftr_mutual_information_band_multiblank_supported(int T, int S, int r, int D) {
  return mi_band_tdt_supported(T, S, r, 1, D, kBandMultiblankDomain);
}

int ftr_mutual_information_band_multiblank_f32(const float* px_band, const float* py_band, const int32_t* ranges,
                                               const int32_t* boundary, const int32_t* durations, int D, float* workspace,
                                               size_t workspace_floats, float* ans, float* gx_band, float* gy_band, int B,
                                               int T, int S, int r, void* stream) {
  const char* what = "mutual_information_band_multiblank";
  clear_error();
  if (D < 1 || D > 8) {                      // the length of the list itself: the domain, before the list is read
    set_error("%s: D = %d is outside the kernel's domain (1..8 blanks)", what, D);
    return FTR_ERR_UNSUPPORTED;
  }
  FTR_TRY(mb_check_durations(what, durations, D, false));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  if (!mi_band_tdt_supported(T, S, r, 1, D, kBandMultiblankDomain)) {
    set_error("%s: T=%d S=%d r=%d is outside the kernel's domain (r <= 15)", what, T, S, r);
    return FTR_ERR_UNSUPPORTED;
  }
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_floats, mi_band_tdt_workspace_floats(B, T, S, r, 1, D, kBandMultiblankDomain), "floats"));
  FTR_REQUIRE(px_band && py_band && ranges && workspace && ans, "%s: null px_band / py_band / ranges / workspace / ans", what);
  FTR_REQUIRE((gx_band != nullptr) == (gy_band != nullptr), "%s: gx_band and gy_band must both be given or both be null", what);
  FTR_TRY(check_ws_aligned(what, workspace));
  FTR_TRY(device_ok());
  return mi_band_multiblank(px_band, py_band, ranges, boundary, durations, D, workspace, workspace_floats, ans, gx_band, gy_band, B,
                            T, S, r, stream_of(stream));
}

// ---- include/ftr_band_viterbi.h: best-path alignment on the pruned band itself (csrc/mi_band_viterbi.hip).  The move
// lists are those of ftr_mutual_information_viterbi_tdt_f32: up to 8 of a kind, a blank may advance 32 frames.
int ftr_mutual_information_band_viterbi_supported(int T, int S, int r, int N, int Ny) {
  return mi_band_viterbi_supported(T, S, r, N, Ny);
}
size_t ftr_mutual_information_band_viterbi_workspace_bytes(int B, int T, int S, int r, int N, int Ny) {
  return mi_band_viterbi_workspace_bytes(B, T, S, r, N, Ny);
}

int ftr_mutual_information_band_viterbi_f32(const float* px_band, const float* py_band, const int32_t* ranges,
                                            const int32_t* boundary, const int32_t* token_durations, int N,
                                            const int32_t* blank_durations, int Ny, void* workspace, size_t workspace_bytes,
                                            float* score, int32_t* frames, int32_t* durations, int32_t* blank_steps, int B,
                                            int T, int S, int r, void* stream) {
  const char* what = "mutual_information_band_viterbi";
  clear_error();
  FTR_TRY(tdt_check_list(what, "token_durations", token_durations, N, 8, 0));
  FTR_TRY(tdt_check_list(what, "blank_durations", blank_durations, Ny, 8, 1, 32));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  if (!mi_band_viterbi_supported(T, S, r, N, Ny)) {
    set_error("%s: T=%d S=%d r=%d N=%d Ny=%d is outside the kernel's domain (r <= 15, N + Ny <= 9)", what, T, S, r, N, Ny);
    return FTR_ERR_UNSUPPORTED;
  }
  if (B == 0) return FTR_OK;
  FTR_TRY(check_ws_size(what, workspace_bytes, mi_band_viterbi_workspace_bytes(B, T, S, r, N, Ny), "bytes"));
  FTR_REQUIRE(px_band && py_band && ranges && workspace && score && blank_steps,
              "%s: null px_band / py_band / ranges / workspace / score / blank_steps", what);
  FTR_REQUIRE((frames && durations) || S == 0, "%s: null frames / durations", what);
  FTR_TRY(check_ws_aligned(what, workspace));
  FTR_TRY(device_ok());
  return mi_band_viterbi(px_band, py_band, ranges, boundary, token_durations, N, blank_durations, Ny, workspace, workspace_bytes,
                         score, frames, durations, blank_steps, B, T, S, r, stream_of(stream));
}

int ftr_multiblank_pruned_band_fwd_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                       const int32_t* boundary, int termination_symbol, const int32_t* big_blank_ids,
                                       const int32_t* durations, int D, double sigma, double delay_penalty, float* lse,
                                       float* px_band, float* py_band, int B, int T, int S, int C, int r, void* stream) {
  const char* what = "multiblank_pruned_band_fwd";
  clear_error();
  FTR_TRY(mb_check_durations(what, durations, D, true));
  FTR_TRY(mb_check_ids(what, big_blank_ids, D, termination_symbol, C));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_s_range(what, r, S));
  FTR_REQUIRE(sigma >= 0.0, "%s: sigma = %g must not be negative", what, sigma);
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse && px_band && py_band && (symbols || S == 0)));
  return multiblank_band_fwd(logits, symbols, ranges, boundary, termination_symbol, big_blank_ids, durations, D, sigma,
                             delay_penalty, lse, px_band, py_band, B, T, S, C, r, stream_of(stream));
}

int ftr_multiblank_pruned_band_bwd_scaled_f32(const float* logits, const int32_t* symbols, const int32_t* ranges,
                                              const int32_t* boundary, int termination_symbol, const int32_t* big_blank_ids,
                                              const int32_t* durations, int D, const float* lse, const float* gx_band,
                                              const float* gy_band, const float* scale, int scale_stride, float scale_mul,
                                              float* glogits, int B, int T, int S, int C, int r, void* stream) {
  const char* what = "multiblank_pruned_band_bwd_scaled";
  clear_error();
  FTR_TRY(mb_check_durations(what, durations, D, true));
  FTR_TRY(mb_check_ids(what, big_blank_ids, D, termination_symbol, C));
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && ranges && lse && gx_band && gy_band && glogits && (symbols || S == 0)));
  return multiblank_band_bwd(logits, symbols, ranges, boundary, termination_symbol, big_blank_ids, durations, D, lse, gx_band,
                             gy_band, Scale{scale, scale_stride, scale_mul}, glogits, B, T, S, C, r, stream_of(stream));
}

// ---- include/ftr_kd.h, include/ftr_kd_fact.h: knowledge distillation on the pruned band (csrc/pruned_kd.hip)
// element type codes, mode and temperature, then the factorization and what belongs to it: before everything else
static int kd_check_head(const char* what, int kind, int teacher_kind, int mode, float temperature, int factorization,
                         int n_dur, float dur_weight, int C) {
  FTR_TRY(check_dtype(what, kind, 0));
  FTR_TRY(check_dtype(what, teacher_kind, 0));
  FTR_REQUIRE(mode == FTR_KD_FULL || mode == FTR_KD_COLLAPSED, "%s: unknown mode %d (FTR_KD_FULL = 0, FTR_KD_COLLAPSED = 1)", what, mode);
  FTR_REQUIRE(temperature > 0.0f && temperature <= 3.0e38f, "%s: temperature %g is not a finite number > 0", what, (double)temperature);
  FTR_REQUIRE(factorization == FTR_KD_FACT_SOFTMAX || factorization == FTR_KD_FACT_HAT || factorization == FTR_KD_FACT_TDT,
              "%s: unknown factorization %d (FTR_KD_FACT_SOFTMAX = 0, FTR_KD_FACT_HAT = 1, FTR_KD_FACT_TDT = 2)", what, factorization);
  if (factorization != FTR_KD_FACT_TDT) {
    FTR_REQUIRE(n_dur == 0, "%s: n_dur = %d, only FTR_KD_FACT_TDT has duration columns", what, n_dur);
    return FTR_OK;
  }
  FTR_REQUIRE(n_dur >= 1 && n_dur <= FTR_KD_FACT_MAX_DUR, "%s: n_dur = %d not in [1,%d]", what, n_dur, FTR_KD_FACT_MAX_DUR);
  FTR_REQUIRE(n_dur < C, "%s: n_dur = %d leaves no token column in a row of C = %d", what, n_dur, C);
  FTR_REQUIRE(dur_weight >= 0.0f && dur_weight <= 3.0e38f, "%s: dur_weight %g is not a finite number >= 0", what, (double)dur_weight);
  return FTR_OK;
}

// the body of both forward entries, under the entry's own `what`; the plain entry is FTR_KD_FACT_SOFTMAX, 0, 0, NULL
static int kd_fwd(const char* what, const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                  const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int termination_symbol,
                  float temperature, int mode, float* node_loss, float* saved, float* utt_loss, int B, int T, int S, int C,
                  int r, int factorization, int n_dur, float dur_weight, const float* node_weights, void* stream) {
  clear_error();
  FTR_TRY(kd_check_head(what, kind, teacher_kind, mode, temperature, factorization, n_dur, dur_weight, C));
  const int hat = factorization == FTR_KD_FACT_HAT;
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1 && r >= 1, termination_symbol, C - n_dur, false, hat));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && teacher_logits && ranges && node_loss && saved && utt_loss && (symbols || S == 0)));
  return pruned_kd_fwd(logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary, termination_symbol, temperature,
                       mode == FTR_KD_COLLAPSED, hat, n_dur, dur_weight, node_weights, node_loss, saved, utt_loss, B, T, S, C, r,
                       stream_of(stream));
}

// and of both backward entries
static int kd_bwd(const char* what, const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                  const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int termination_symbol,
                  float temperature, int mode, const float* saved, const float* scale, int scale_stride, float scale_mul,
                  void* glogits, int B, int T, int S, int C, int r, int factorization, int n_dur, float dur_weight,
                  const float* node_weights, void* stream) {
  clear_error();
  FTR_TRY(kd_check_head(what, kind, teacher_kind, mode, temperature, factorization, n_dur, dur_weight, C));
  const int hat = factorization == FTR_KD_FACT_HAT;
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1 && r >= 1, termination_symbol, C - n_dur, true, hat));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && teacher_logits && ranges && saved && glogits && (symbols || S == 0)));
  return pruned_kd_bwd(logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary, termination_symbol, temperature,
                       mode == FTR_KD_COLLAPSED, hat, n_dur, dur_weight, node_weights, saved, Scale{scale, scale_stride, scale_mul},
                       glogits, B, T, S, C, r, stream_of(stream));
}

int ftr_pruned_kd_fwd_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                         const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int termination_symbol,
                         float temperature, int mode, float* node_loss, float* saved, float* utt_loss, int B, int T, int S,
                         int C, int r, void* stream) {
  return kd_fwd("pruned_kd_fwd_dt", logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary, termination_symbol,
                temperature, mode, node_loss, saved, utt_loss, B, T, S, C, r, FTR_KD_FACT_SOFTMAX, 0, 0.0f, NULL, stream);
}

int ftr_pruned_kd_bwd_scaled_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                int termination_symbol, float temperature, int mode, const float* saved,
                                const float* scale, int scale_stride, float scale_mul, void* glogits, int B, int T, int S,
                                int C, int r, void* stream) {
  return kd_bwd("pruned_kd_bwd_scaled_dt", logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary,
                termination_symbol, temperature, mode, saved, scale, scale_stride, scale_mul, glogits, B, T, S, C, r,
                FTR_KD_FACT_SOFTMAX, 0, 0.0f, NULL, stream);
}

int ftr_pruned_kd_reduce_f32(const float* utt_loss, int B, int reduction, float* out, void* stream) {
  clear_error();
  FTR_REQUIRE(B >= 1 && reduction >= 0 && reduction <= 2, "pruned_kd_reduce: bad arguments B=%d reduction=%d", B, reduction);
  FTR_TRY(pointers_then_device("pruned_kd_reduce", utt_loss && out));
  return negated_reduce(utt_loss, B, reduction, out, stream_of(stream), 1.0f);
}

int ftr_pruned_kd_fact_fwd_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                              const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                              int termination_symbol, float temperature, int mode, float* node_loss, float* saved,
                              float* utt_loss, int B, int T, int S, int C, int r, int factorization, int n_dur,
                              float dur_weight, const float* node_weights, void* stream) {
  return kd_fwd("pruned_kd_fact_fwd_dt", logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary,
                termination_symbol, temperature, mode, node_loss, saved, utt_loss, B, T, S, C, r, factorization, n_dur, dur_weight,
                node_weights, stream);
}

int ftr_pruned_kd_fact_bwd_scaled_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                     const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                     int termination_symbol, float temperature, int mode, const float* saved,
                                     const float* scale, int scale_stride, float scale_mul, void* glogits, int B, int T,
                                     int S, int C, int r, int factorization, int n_dur, float dur_weight,
                                     const float* node_weights, void* stream) {
  return kd_bwd("pruned_kd_fact_bwd_scaled_dt", logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary,
                termination_symbol, temperature, mode, saved, scale, scale_stride, scale_mul, glogits, B, T, S, C, r, factorization,
                n_dur, dur_weight, node_weights, stream);
}

// ---- include/ftr_kd_loss.h, include/ftr_kd_loss_fact.h: the transducer loss on the band and the distillation loss in one
// pass (csrc/pruned_kd.hip); the factored entries add a HAT row, node weights, and the student's own occupancies as weights
// element kinds, mode and temperature as above, which is all the plain entries check; then the factorization, of which TDT is
// known and refused
static int kd_loss_check_head(const char* what, int kind, int teacher_kind, int mode, float temperature, int factorization, int C,
                              bool fact_entry) {
  FTR_TRY(kd_check_head(what, kind, teacher_kind, mode, temperature, FTR_KD_FACT_SOFTMAX, 0, 0.0f, C));
  if (!fact_entry) return FTR_OK;
  FTR_REQUIRE(factorization == FTR_KD_FACT_SOFTMAX || factorization == FTR_KD_FACT_HAT || factorization == FTR_KD_FACT_TDT,
              "%s: unknown factorization %d (FTR_KD_FACT_SOFTMAX = 0, FTR_KD_FACT_HAT = 1)", what, factorization);
  FTR_REQUIRE(factorization != FTR_KD_FACT_TDT, "%s: FTR_KD_FACT_TDT is out of scope for the one-pass entries (FTR_KD_FACT_SOFTMAX = 0, FTR_KD_FACT_HAT = 1)", what);
  return FTR_OK;
}

// the body of both forward entries, under the entry's own `what`; the plain entry is FTR_KD_FACT_SOFTMAX, NULL and requires
// utt_loss, which the factored one may leave out
static int kd_loss_fwd(const char* what, const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                       const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int termination_symbol,
                       float temperature, int mode, double delay_penalty, int modified, float* lse, float* px_band,
                       float* py_band, float* node_loss, float* saved, float* utt_loss, int B, int T, int S, int C, int r,
                       int factorization, const float* node_weights, bool fact_entry, void* stream) {
  clear_error();
  FTR_TRY(kd_loss_check_head(what, kind, teacher_kind, mode, temperature, factorization, C, fact_entry));
  const int hat = factorization == FTR_KD_FACT_HAT;
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1 && r >= 1, termination_symbol, C, false, hat));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && teacher_logits && ranges && lse && px_band && py_band && node_loss && saved &&
                                         (utt_loss || fact_entry) && (symbols || S == 0)));
  return pruned_band_kd_fact_fwd(logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary, termination_symbol,
                                 temperature, mode == FTR_KD_COLLAPSED, delay_penalty, modified, lse, px_band, py_band, node_loss,
                                 saved, utt_loss, B, T, S, C, r, hat, node_weights, stream_of(stream));
}

// and of both backward entries
static int kd_loss_bwd(const char* what, const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                       const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int termination_symbol,
                       float temperature, int mode, const float* lse, const float* gx_band, const float* gy_band,
                       const float* loss_scale, int loss_scale_stride, float loss_scale_mul, const float* saved,
                       const float* kd_scale, int kd_scale_stride, float kd_scale_mul, void* glogits, int B, int T, int S, int C,
                       int r, int factorization, const float* node_weights, bool fact_entry, void* stream) {
  clear_error();
  FTR_TRY(kd_loss_check_head(what, kind, teacher_kind, mode, temperature, factorization, C, fact_entry));
  FTR_REQUIRE(loss_scale_mul >= -3.0e38f && loss_scale_mul <= 3.0e38f && kd_scale_mul >= -3.0e38f && kd_scale_mul <= 3.0e38f,
              "%s: the multipliers %g and %g must be finite", what, (double)loss_scale_mul, (double)kd_scale_mul);
  const int hat = factorization == FTR_KD_FACT_HAT;
  FTR_TRY(check_builder(what, B >= 0 && T >= 1 && S >= 0 && C >= 1 && r >= 1, termination_symbol, C, true, hat));
  FTR_TRY(check_scale_stride(what, loss_scale_stride));
  FTR_TRY(check_scale_stride(what, kd_scale_stride));
  if (B == 0) return FTR_OK;
  const bool loss_on = loss_scale_mul != 0.0f, kd_on = kd_scale_mul != 0.0f;
  FTR_TRY(pointers_then_device(what, logits && ranges && glogits && (symbols || S == 0) && (!loss_on || (lse && gx_band && gy_band)) &&
                                         (!kd_on || (teacher_logits && saved))));
  return pruned_band_kd_fact_bwd(logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary, termination_symbol,
                                 temperature, mode == FTR_KD_COLLAPSED, lse, gx_band, gy_band,
                                 Scale{loss_scale, loss_scale_stride, loss_scale_mul}, saved, Scale{kd_scale, kd_scale_stride, kd_scale_mul},
                                 glogits, B, T, S, C, r, hat, node_weights, stream_of(stream));
}

int ftr_pruned_band_kd_fwd_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                              const int32_t* symbols, const int32_t* ranges, const int32_t* boundary, int termination_symbol,
                              float temperature, int mode, double delay_penalty, int modified, float* lse, float* px_band,
                              float* py_band, float* node_loss, float* saved, float* utt_loss, int B, int T, int S, int C,
                              int r, void* stream) {
  return kd_loss_fwd("pruned_band_kd_fwd_dt", logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary,
                     termination_symbol, temperature, mode, delay_penalty, modified, lse, px_band, py_band, node_loss, saved,
                     utt_loss, B, T, S, C, r, FTR_KD_FACT_SOFTMAX, NULL, false, stream);
}

int ftr_pruned_band_kd_bwd_scaled_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                     const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                     int termination_symbol, float temperature, int mode, const float* lse,
                                     const float* gx_band, const float* gy_band, const float* loss_scale,
                                     int loss_scale_stride, float loss_scale_mul, const float* saved, const float* kd_scale,
                                     int kd_scale_stride, float kd_scale_mul, void* glogits, int B, int T, int S, int C,
                                     int r, void* stream) {
  return kd_loss_bwd("pruned_band_kd_bwd_scaled_dt", logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary,
                     termination_symbol, temperature, mode, lse, gx_band, gy_band, loss_scale, loss_scale_stride, loss_scale_mul,
                     saved, kd_scale, kd_scale_stride, kd_scale_mul, glogits, B, T, S, C, r, FTR_KD_FACT_SOFTMAX, NULL, false, stream);
}

int ftr_pruned_band_kd_fact_fwd_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                   const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                   int termination_symbol, float temperature, int mode, double delay_penalty, int modified,
                                   float* lse, float* px_band, float* py_band, float* node_loss, float* saved, float* utt_loss,
                                   int B, int T, int S, int C, int r, int factorization, const float* node_weights,
                                   void* stream) {
  return kd_loss_fwd("pruned_band_kd_fact_fwd_dt", logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary,
                     termination_symbol, temperature, mode, delay_penalty, modified, lse, px_band, py_band, node_loss, saved,
                     utt_loss, B, T, S, C, r, factorization, node_weights, true, stream);
}

int ftr_pruned_band_kd_fact_bwd_scaled_dt(const void* logits, int kind, const void* teacher_logits, int teacher_kind,
                                          const int32_t* symbols, const int32_t* ranges, const int32_t* boundary,
                                          int termination_symbol, float temperature, int mode, const float* lse,
                                          const float* gx_band, const float* gy_band, const float* loss_scale,
                                          int loss_scale_stride, float loss_scale_mul, const float* saved,
                                          const float* kd_scale, int kd_scale_stride, float kd_scale_mul, void* glogits, int B,
                                          int T, int S, int C, int r, int factorization, const float* node_weights,
                                          void* stream) {
  return kd_loss_bwd("pruned_band_kd_fact_bwd_scaled_dt", logits, kind, teacher_logits, teacher_kind, symbols, ranges, boundary,
                     termination_symbol, temperature, mode, lse, gx_band, gy_band, loss_scale, loss_scale_stride, loss_scale_mul,
                     saved, kd_scale, kd_scale_stride, kd_scale_mul, glogits, B, T, S, C, r, factorization, node_weights, true,
                     stream);
}

int ftr_band_node_occupancy_f32(const float* gx_band, const float* gy_band, const int32_t* ranges, const int32_t* boundary,
                                float* occ, int B, int T, int S, int r, void* stream) {
  const char* what = "band_node_occupancy";
  clear_error();
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && r >= 1));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, gx_band && gy_band && ranges && occ));
  return band_node_occupancy(gx_band, gy_band, ranges, boundary, occ, B, T, S, r, stream_of(stream));
}

int ftr_pruned_kd_weighted_utt_sum_f32(const float* node_loss, const float* node_weights, float* utt_loss, int B, int T,
                                       int r, void* stream) {
  const char* what = "pruned_kd_weighted_utt_sum";
  clear_error();
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && r >= 1));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, node_loss && node_weights && utt_loss));
  return pruned_kd_weighted_utt_sum(node_loss, node_weights, utt_loss, B, T * r, stream_of(stream));
}

// ---- include/ftr_kd_topk.h: distillation from a stored top-K teacher on the teacher's own band (csrc/pruned_kd_topk.hip)
// element kinds and temperature, then the sizes: the head of both entries
static int kd_topk_check_head(const char* what, int kind, int teacher_kind, float temperature, const int32_t* teacher_ranges,
                              int B, int T, int S, int C, int r, int r_t, int K) {
  FTR_TRY(check_dtype(what, kind, 0));
  FTR_TRY(check_dtype(what, teacher_kind, 0));
  FTR_REQUIRE(temperature > 0.0f && temperature <= 3.0e38f, "%s: temperature %g is not a finite number > 0", what, (double)temperature);
  FTR_TRY(check_sizes(what, B >= 0 && T >= 1 && S >= 0 && C >= 1 && r >= 1 && r_t >= 1));
  FTR_REQUIRE(K >= 1 && K <= FTR_KD_TOPK_MAX_K, "%s: K = %d not in [1,%d]", what, K, FTR_KD_TOPK_MAX_K);
  FTR_REQUIRE(teacher_ranges || r_t == r, "%s: r_t = %d, but without teacher_ranges the cache lies on the student's ranges of r = %d rows",
              what, r_t, r);
  return FTR_OK;
}

int ftr_pruned_kd_topk_fwd_dt(const void* logits, int kind, const void* teacher_values, int teacher_kind,
                              const int32_t* teacher_indices, const int32_t* ranges, const int32_t* teacher_ranges,
                              const int32_t* boundary, const float* teacher_rest, const float* node_weights,
                              float temperature, float* node_loss, float* saved, float* utt_loss, int B, int T, int S,
                              int C, int r, int r_t, int K, void* stream) {
  const char* what = "pruned_kd_topk_fwd_dt";
  clear_error();
  FTR_TRY(kd_topk_check_head(what, kind, teacher_kind, temperature, teacher_ranges, B, T, S, C, r, r_t, K));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && teacher_values && teacher_indices && ranges && node_loss && saved && utt_loss));
  return pruned_kd_topk_fwd(logits, kind, teacher_values, teacher_kind, teacher_indices, ranges, teacher_ranges, boundary,
                            teacher_rest, node_weights, temperature, node_loss, saved, utt_loss, B, T, S, C, r, r_t, K,
                            stream_of(stream));
}

int ftr_pruned_kd_topk_bwd_scaled_dt(const void* logits, int kind, const void* teacher_values, int teacher_kind,
                                     const int32_t* teacher_indices, const int32_t* ranges, const int32_t* teacher_ranges,
                                     const int32_t* boundary, const float* teacher_rest, const float* node_weights,
                                     float temperature, const float* saved, const float* scale, int scale_stride,
                                     float scale_mul, void* glogits, int B, int T, int S, int C, int r, int r_t, int K,
                                     void* stream) {
  const char* what = "pruned_kd_topk_bwd_scaled_dt";
  clear_error();
  FTR_TRY(kd_topk_check_head(what, kind, teacher_kind, temperature, teacher_ranges, B, T, S, C, r, r_t, K));
  FTR_TRY(check_scale_stride(what, scale_stride));
  if (B == 0) return FTR_OK;
  FTR_TRY(pointers_then_device(what, logits && teacher_values && teacher_indices && ranges && saved && glogits));
  return pruned_kd_topk_bwd(logits, kind, teacher_values, teacher_kind, teacher_indices, ranges, teacher_ranges, boundary,
                            teacher_rest, node_weights, temperature, saved, Scale{scale, scale_stride, scale_mul}, glogits, B, T, S,
                            C, r, r_t, K, stream_of(stream));
}

int ftr_selftest(void* scratch_dev, void* stream) {
  clear_error();
  FTR_REQUIRE(scratch_dev, "selftest: need >= 8 KiB of device scratch");
  FTR_TRY(device_ok());
  return selftest(stream_of(stream), reinterpret_cast<int*>(scratch_dev));
}

#ifdef FTR_DIAG
int ftr_debug_stamps(unsigned long long* out16) {
  clear_error();
  FTR_TRY(pointers_then_device("debug_stamps", out16));
  return debug_stamps(out16);
}

int ftr_debug_trace(unsigned long long* out, int n) {
  clear_error();
  FTR_TRY(pointers_then_device("debug_trace", out || n == 0));
  return debug_trace(out, n);
}
#endif

}  // extern "C"
