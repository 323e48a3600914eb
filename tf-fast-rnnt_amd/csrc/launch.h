// csrc/launch.h -- host-side launch plumbing shared by the kernel files: the dynamic-LDS limit of a kernel, raised once per
// device, and the step from a run-time value to the template argument of the one kernel that is launched.  Host only.
#pragma once
#include "ftr_common.h"
#include <atomic>
#include <mutex>
#include <type_traits>

namespace ftr {

constexpr int kTrackedDevices = 64;   // device ordinals with a cache slot; beyond: the runtime is asked every time

// CU count of the current device (256 where it cannot be read)
inline int current_device_cus() {
  static std::atomic<int> cus[kTrackedDevices];
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
  const bool tracked = dev >= 0 && dev < kTrackedDevices;
  if (tracked && (n = cus[dev].load(std::memory_order_relaxed)) > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); return 256; }
  if (tracked) cus[dev].store(n, std::memory_order_relaxed);
  return n;
}

// The wording of a failed reserve_lds() at its site (the texts predate this header and are kept as they were)
enum class LdsText { raise, raise_why, reserve_why, reserve_bytes_why };

// A launch with more than 64 KB of dynamic LDS needs the kernel's limit raised first, on EVERY device that launches it.
// Kernel: the instantiation about to be launched; bytes: what it is launched with (or a fixed ceiling).  The largest
// grant is remembered per instantiation and device, so the runtime is called only when a request exceeds it.
template <auto Kernel>
inline int reserve_lds(size_t bytes, const char* what, LdsText text = LdsText::raise) {
  if (bytes <= 64 * 1024) return FTR_OK;
  static std::atomic<int> granted[kTrackedDevices];
  static std::mutex raising;   // two threads raising one kernel to different sizes: the larger must be the last to land
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; }
  const bool tracked = dev >= 0 && dev < kTrackedDevices;
  if (tracked && granted[dev].load(std::memory_order_acquire) >= (int)bytes) return FTR_OK;
  std::lock_guard<std::mutex> lock(raising);
  if (tracked && granted[dev].load(std::memory_order_relaxed) >= (int)bytes) return FTR_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    switch (text) {
      case LdsText::raise: set_error("%s: cannot raise the dynamic LDS limit", what); break;
      case LdsText::raise_why: set_error("%s: cannot raise the dynamic LDS limit: %s", what, hipGetErrorString(e)); break;
      case LdsText::reserve_why: set_error("%s: cannot reserve LDS: %s", what, hipGetErrorString(e)); break;
      case LdsText::reserve_bytes_why: set_error("%s: cannot reserve %zu bytes of LDS: %s", what, bytes, hipGetErrorString(e)); break;
    }
    return FTR_ERR_LAUNCH;
  }
  if (tracked) granted[dev].store((int)bytes, std::memory_order_release);
  return FTR_OK;
}

// ---- run-time value -> compile-time value.  f is a generic lambda; it is called once, with a std::bool_constant or a
// std::integral_constant, and its result is returned.  Only the listed values are instantiated.
template <typename F>
inline auto dispatch(bool flag, F&& f) {
  if (flag) return f(std::true_type{});
  return f(std::false_type{});
}
// an FTR_DTYPE_* code -> the element type: f is called with an elem_tag<float | bf16_t | fp16_t>.  The entry points of
// capi.hip reject unknown codes (check_dtype) before a launcher sees them; here any other code is float.
template <typename E> struct elem_tag { using type = E; };
template <typename F>
inline auto dispatch_dtype(int dtype, F&& f) {
  if (dtype == FTR_DTYPE_BF16) return f(elem_tag<bf16_t>{});
  if (dtype == FTR_DTYPE_FP16) return f(elem_tag<fp16_t>{});
  return f(elem_tag<float>{});
}
// may rows of C elements starting at `a` (and at `b`, if given) be read four elements at a time?  float rows are dword
// aligned whatever C is; a 16-bit row needs its 8-byte alignment, which a view at an odd element offset does not have.
template <typename E>
inline bool rows_vec4(int C, const void* a, const void* b = nullptr) {
  if ((C & 3) != 0) return false;
  if (std::is_same<E, float>::value) return true;
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0;
}
// v among V, Rest...: that one; any other v: the last of the list
template <int V, int... Rest, typename F>
inline auto dispatch_among(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
  else {
    if (v == V) return f(std::integral_constant<int, V>{});
    return dispatch_among<Rest...>(v, f);
  }
}
// v in LO..HI: f(v as a constant); any other v: otherwise()
template <int LO, int HI, typename F, typename G>
inline auto dispatch_range(int v, F&& f, G&& otherwise) {
  if constexpr (LO > HI) return otherwise();
  else {
    if (v == LO) return f(std::integral_constant<int, LO>{});
    return dispatch_range<LO + 1, HI>(v, f, otherwise);
  }
}

}  // namespace ftr
