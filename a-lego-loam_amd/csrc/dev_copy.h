// dev_copy.h — the one definition of the host side's copies between host and device and of its waits for a stream.  Header-only; it keeps
// no state beyond the error a DevTry carries.  The rules:
//   - a copy is counted in elements: dev_copy_n() alone turns a count into bytes, from the destination's element type;
//   - the direction is the function called (dev_up: host to device, dev_down: device to host), blocking without a stream, queued with one;
//   - destination and source have the same element type, but for the two exceptions below, each behind a static_assert;
//   - a count of zero is a success that calls nothing, whatever the pointers are (an empty vector's data());
//   - a DevTry keeps the first failure of a chain: what follows it does nothing, the text is "<what>: <step> failed: <runtime's reason>".
// Exceptions to "same element type": alego_point and float4 (both 16 bytes) stand for each other, and dev_down_bytes() serves the debug
// getters alego_debug_get / lm_host_debug_get, whose destination is a void* counted in bytes.
// Not copied through this header: the hipMemcpy2D of alego_debug_get and of lm_host_map_set_keyposes (strided rows), the device-to-device copy
// of kernels_icp.hip, the launchers' reads of their __device__ tick counters by symbol (ALEGO_TIMING builds), the ALEGO_DEBUG_SYNC waits that
// only print, and guard_alloc.cpp, which lies below this layer.
#ifndef ALEGO_DEV_COPY_H_
#define ALEGO_DEV_COPY_H_
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/alego_mi355x.h"

static_assert(sizeof(alego_point) == 16 && sizeof(float4) == 16, "alego_point and float4 are copied as each other");
template <class A, class B> struct DevSameElem : std::is_same<std::remove_cv_t<A>, std::remove_cv_t<B>> {};
template <> struct DevSameElem<alego_point, float4> : std::true_type {};
template <> struct DevSameElem<float4, alego_point> : std::true_type {};

// blocking (default) or queued on a stream: a hipStream_t in a copy's last argument becomes the latter
struct DevQueue {
  bool queued = false; hipStream_t st = nullptr;
  DevQueue() = default;
  DevQueue(hipStream_t s) : queued(true), st(s) {}
};

template <class D, class S> inline hipError_t dev_copy_n(D* dst, const S* src, size_t n, hipMemcpyKind kind, DevQueue q) {
  static_assert(DevSameElem<D, S>::value && !std::is_const<D>::value, "a copy's destination and source have the same element type");
  if (n == 0) return hipSuccess;
  const size_t bytes = n * sizeof(D);
  return q.queued ? hipMemcpyAsync(dst, src, bytes, kind, q.st) : hipMemcpy(dst, src, bytes, kind);
}

// host to device: n elements, a vector, an array
template <class D, class S> inline hipError_t dev_up(D* dst, const S* src, size_t n, DevQueue q = {}) { return dev_copy_n(dst, src, n, hipMemcpyHostToDevice, q); }
template <class D, class S> inline hipError_t dev_up(D* dst, const std::vector<S>& v, DevQueue q = {}) { return dev_up(dst, v.data(), v.size(), q); }
template <class D, class S, size_t N> inline hipError_t dev_up(D* dst, const S (&a)[N], DevQueue q = {}) { return dev_up(dst, a, N, q); }
// device to host
template <class D, class S> inline hipError_t dev_down(D* dst, const S* src, size_t n, DevQueue q = {}) { return dev_copy_n(dst, src, n, hipMemcpyDeviceToHost, q); }
template <class D, class S> inline hipError_t dev_down(std::vector<D>& v, const S* src, DevQueue q = {}) { return dev_down(v.data(), src, v.size(), q); }
template <class D, class S, size_t N> inline hipError_t dev_down(D (&a)[N], const S* src, DevQueue q = {}) { return dev_down(a, src, N, q); }
static_assert(sizeof(unsigned char) == 1, "dev_down_bytes counts in bytes");
inline hipError_t dev_down_bytes(void* dst, const void* src, size_t bytes) { return dev_down(static_cast<unsigned char*>(dst), static_cast<const unsigned char*>(src), bytes); }

// every stream of a list is waited for, in order, also after one has failed; the first failure is the one returned
inline hipError_t dev_wait(hipStream_t st) { return hipStreamSynchronize(st); }
template <class List> inline hipError_t dev_wait(const List& streams) {
  hipError_t r = hipSuccess;
  for (hipStream_t s : streams) { const hipError_t e = hipStreamSynchronize(s); if (r == hipSuccess) r = e; }
  return r;
}

// The first error of a chain of copies and waits.  `step` names what the chain is doing for the message ("upload", "ray casting"); without
// one a copy is an "upload" or a "device read" and a wait "a stream".  Converts to the call's return code; *err is set where the failure is taken.
class DevTry {
 public:
  DevTry(std::string what, std::string* err, const char* step = nullptr) : what_(std::move(what)), err_(err), step_(step) {}
  template <class... A> DevTry& up(A&&... a) { return ok() ? took(dev_up(std::forward<A>(a)...), "upload") : *this; }
  template <class... A> DevTry& down(A&&... a) { return ok() ? took(dev_down(std::forward<A>(a)...), "device read") : *this; }
  template <class S> DevTry& wait(const S& streams) { return ok() ? took(dev_wait(streams), "a stream") : *this; }
  DevTry& at(const char* step) { step_ = step; return *this; }
  // an error from outside the header (DevBuf::reserve, dev_down_bytes): the step named here is used when the chain has none
  DevTry& took(hipError_t e, const char* step = "allocation") {
    if (ok() && e != hipSuccess) { e_ = e; *err_ = what_ + ": " + (step_ ? step_ : step) + " failed: " + hipGetErrorString(e); }
    return *this;
  }
  bool ok() const { return e_ == hipSuccess; }
  operator int() const { return ok() ? 0 : ALEGO_ERR_HIP; }
 private:
  std::string what_; std::string* err_; const char* step_; hipError_t e_ = hipSuccess;
};
#endif
