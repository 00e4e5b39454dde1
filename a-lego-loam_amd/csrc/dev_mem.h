// dev_mem.h — the one owner of device memory on the host side: every device block of the library, kept with a handle or taken for one call,
// belongs to a DevPool or a DevBuf and so comes from guard_alloc.h (ALEGO_DEBUG_CANARY=1).  Header-only; it names no HIP call of its own but
// hipGetErrorString, for the message of a failed request (DevGet).
#ifndef ALEGO_DEV_MEM_H_
#define ALEGO_DEV_MEM_H_
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "guard_alloc.h"

// A set of device blocks freed together: by clear(), by the destructor, or one at a time by release().  Movable, not copyable.
class DevPool {
 public:
  DevPool() = default;
  DevPool(DevPool&& o) noexcept : p_(std::move(o.p_)) { o.p_.clear(); }
  DevPool& operator=(DevPool&& o) noexcept { if (this != &o) { clear(); p_ = std::move(o.p_); o.p_.clear(); } return *this; }
  ~DevPool() { clear(); }
  // `count` elements of T, at least 16 bytes; *p is null on failure
  template <class T> hipError_t get(T** p, size_t count, bool zero) {
    *p = nullptr;
    const size_t bytes = std::max<size_t>(16, count * sizeof(T));
    void* q = nullptr; hipError_t e = guard_malloc(&q, bytes);
    if (e != hipSuccess) return e;
    if (zero && (e = guard_zero(q, bytes)) != hipSuccess) { (void)guard_free(q); return e; }
    p_.push_back(q); *p = static_cast<T*>(q);
    return hipSuccess;
  }
  void release(void* p) {   // frees one member early (a pointer the pool does not own: nothing happens)
    auto it = std::find(p_.begin(), p_.end(), p);
    if (it != p_.end()) { (void)guard_free(p); p_.erase(it); }
  }
  void clear() { for (void* p : p_) (void)guard_free(p); p_.clear(); }
  // hand-over for an owner that stays a POD (VoxCtx, a kernel argument): detach() leaves every block to the caller, adopt() takes one back (null: no-op)
  void detach() { p_.clear(); }
  void adopt(void* p) { if (p) p_.push_back(p); }
 private:
  std::vector<void*> p_;
};

// "Get from a pool or set the error": get(&p, count) is mem.get(&p, count, false); on failure *err = what + the runtime's message.
struct DevGet {
  DevPool& mem; const char* what; std::string* err;
  template <class T> bool operator()(T** p, size_t count) const {
    const hipError_t e = mem.get(p, count, false);
    if (e != hipSuccess) *err = std::string(what) + hipGetErrorString(e);
    return e == hipSuccess;
  }
};

// A grow-only device array.  Growing frees the old block before it allocates the new one (the peak stays at the larger of the two) and
// keeps no contents; a failed grow leaves {nullptr, 0}.  Movable, not copyable.
template <class T>
struct DevBuf {
  T* p = nullptr; size_t cap = 0;   // cap in elements
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { mem_ = std::move(o.mem_); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  hipError_t reserve(size_t count) {
    if (count <= cap) return hipSuccess;
    clear();
    const hipError_t e = mem_.get(&p, count, false);
    if (e == hipSuccess) cap = count;
    return e;
  }
  void clear() { mem_.clear(); p = nullptr; cap = 0; }
 private:
  DevPool mem_;
};
#endif
