// Stand-alone check of csrc/dev_mem.h on the host heap (tests/test_dev_mem.py builds it with -fsanitize=address,undefined and runs it).
// The functions of guard_alloc.h are stubs here: they count live blocks, fill a new block with a non-zero byte and fail the k-th request on demand.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "dev_mem.h"

namespace {
constexpr unsigned char FILL = 0x5A;
std::set<void*> live;        // blocks handed out and not yet freed
std::vector<size_t> sizes;   // bytes of every request, in order
int n_malloc = 0, n_free = 0, foreign_free = 0;
int fail_at = -1;            // the request with this index fails (counted from the last arm())
int request = 0;
std::vector<char> order;     // 'm' / 'f' per successful call, to check that a grow frees first
void arm(int k) { fail_at = k; request = 0; }
int checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
}  // namespace

hipError_t guard_malloc(void** p, size_t bytes) {
  if (request++ == fail_at) return hipErrorOutOfMemory;
  *p = std::malloc(bytes);
  std::memset(*p, FILL, bytes);
  live.insert(*p); sizes.push_back(bytes); order.push_back('m'); ++n_malloc;
  return hipSuccess;
}
hipError_t guard_free(void* p) {
  if (!live.erase(p)) { ++foreign_free; return hipErrorInvalidValue; }   // (a double free or a foreign pointer: counted, not passed to free())
  std::free(p); order.push_back('f'); ++n_free;
  return hipSuccess;
}
hipError_t guard_zero(void* p, size_t bytes) { std::memset(p, 0, bytes); return hipSuccess; }
int guard_check(std::string*) { return -1; }

static bool all_bytes(const void* p, size_t n, unsigned char v) {
  for (size_t i = 0; i < n; ++i) if (static_cast<const unsigned char*>(p)[i] != v) return false;
  return true;
}

int main() {
  // (a) N blocks, the failure injected at every k in 0 .. N (k = N: none fails); freed by clear() and by scope exit
  constexpr int N = 5;
  for (int by_scope = 0; by_scope < 2; ++by_scope)
    for (int k = 0; k <= N; ++k) {
      const int m0 = n_malloc, f0 = n_free;
      {
        DevPool pool;
        double* p[N];
        arm(k);
        for (int i = 0; i < N; ++i) {
          p[i] = reinterpret_cast<double*>(&pool);   // (anything but null)
          const hipError_t e = pool.get(&p[i], (size_t)(i + 1) * 3, (i & 1) != 0);
          CHECK((e == hipSuccess) == (i != k));
          CHECK((p[i] != nullptr) == (i != k));
          if (p[i]) p[i][(i + 1) * 3 - 1] = 1.0;   // the last element is inside the block (ASan)
        }
        arm(-1);
        const int got = N - (k < N ? 1 : 0);
        CHECK(n_malloc - m0 == got && (int)live.size() == got);
        if (!by_scope) {
          pool.clear();
          CHECK(live.empty() && n_free - f0 == got && foreign_free == 0);
          pool.clear();   // nothing left to free
          CHECK(n_free - f0 == got && foreign_free == 0);
          int* again = nullptr;   // the pool is usable afterwards
          CHECK(pool.get(&again, 4, true) == hipSuccess && again && live.size() == 1);
          pool.clear();
          CHECK(live.empty());
        }
      }
      CHECK(live.empty() && n_free == n_malloc && foreign_free == 0);   // every block exactly once
    }
  {
    DevPool pool;
    // (b) count == 0: a non-null block of at least 16 bytes
    char* z = nullptr;
    CHECK(pool.get(&z, 0, false) == hipSuccess && z && sizes.back() >= 16);
    z[15] = 1;
    short* s = nullptr;   // 3 * 2 bytes: the minimum again
    CHECK(pool.get(&s, 3, false) == hipSuccess && s && sizes.back() == 16);
    float* f = nullptr;   // above the minimum: count * sizeof(T)
    CHECK(pool.get(&f, 5, false) == hipSuccess && f && sizes.back() == 20);
    // (c) zero = true yields zeros, zero = false leaves the stub's fill
    CHECK(all_bytes(f, 20, FILL) && all_bytes(s, 16, FILL));
    int* zi = nullptr;
    CHECK(pool.get(&zi, 7, true) == hipSuccess && all_bytes(zi, 28, 0));
    char* z0 = nullptr;
    CHECK(pool.get(&z0, 0, true) == hipSuccess && all_bytes(z0, 16, 0));
    // (d) release of a member frees it once; of a foreign pointer (or null, or the same member again) nothing
    const int f0 = n_free;
    const size_t l0 = live.size();
    pool.release(s);
    CHECK(n_free == f0 + 1 && live.size() == l0 - 1 && !live.count(s));
    int on_stack = 0;
    void* other = std::malloc(16);
    pool.release(s); pool.release(&on_stack); pool.release(other); pool.release(nullptr);
    CHECK(n_free == f0 + 1 && foreign_free == 0 && live.size() == l0 - 1);
    std::free(other);
    {
      DevPool second;
      int* q = nullptr;
      CHECK(second.get(&q, 1, false) == hipSuccess);
      pool.release(q);   // a member of another pool
      CHECK(n_free == f0 + 1 && live.count(q));
    }
    CHECK(n_free == f0 + 2);
    // hand-over: detach() leaves the blocks to the caller, adopt() takes them back
    DevPool a;
    long* h1 = nullptr; long* h2 = nullptr;
    CHECK(a.get(&h1, 2, false) == hipSuccess && a.get(&h2, 2, false) == hipSuccess);
    const int f1 = n_free;
    a.detach(); a.clear();
    CHECK(n_free == f1 && live.count(h1) && live.count(h2));
    { DevPool b; b.adopt(h1); b.adopt(nullptr); b.adopt(h2); }
    CHECK(n_free == f1 + 2 && !live.count(h1) && !live.count(h2) && foreign_free == 0);
  }
  CHECK(live.empty() && n_free == n_malloc && foreign_free == 0);
  {
    // (e) DevBuf::reserve
    DevBuf<float> b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.reserve(0) == hipSuccess && b.p == nullptr && live.empty());   // nothing asked for, nothing taken
    CHECK(b.reserve(10) == hipSuccess && b.p && b.cap == 10 && live.size() == 1 && sizes.back() == 40);
    float* first = b.p;
    b.p[9] = 1.f;
    CHECK(b.reserve(10) == hipSuccess && b.reserve(3) == hipSuccess && b.reserve(0) == hipSuccess && b.p == first && b.cap == 10 && live.size() == 1);
    order.clear();
    CHECK(b.reserve(11) == hipSuccess && b.cap == 11 && live.size() == 1 && !live.count(first) && sizes.back() == 44);
    CHECK(order.size() == 2 && order[0] == 'f' && order[1] == 'm');   // frees before it allocates
    b.p[10] = 1.f;
    arm(0);
    CHECK(b.reserve(100) != hipSuccess && b.p == nullptr && b.cap == 0 && live.empty());   // a failed grow leaves {nullptr, 0}
    arm(-1);
    CHECK(b.reserve(2) == hipSuccess && b.p && b.cap == 2 && live.size() == 1);            // and the buffer is usable afterwards
    // (f) a moved-from pool or buffer owns nothing
    DevBuf<float> c(std::move(b));
    CHECK(b.p == nullptr && b.cap == 0 && c.p && c.cap == 2 && live.size() == 1);
    b.clear();
    CHECK(live.size() == 1);
    DevBuf<float> d;
    CHECK(d.reserve(4) == hipSuccess && live.size() == 2);
    d = std::move(c);   // the target's block is freed, the source's block moves
    CHECK(c.p == nullptr && c.cap == 0 && d.cap == 2 && live.size() == 1 && live.count(d.p));
    DevPool p1;
    int *x = nullptr, *y = nullptr;
    CHECK(p1.get(&x, 1, false) == hipSuccess && p1.get(&y, 1, false) == hipSuccess && live.size() == 3);
    DevPool p2(std::move(p1));
    const int f0 = n_free;
    p1.clear(); p1.release(x);
    CHECK(n_free == f0 && live.size() == 3);
    DevPool p3;
    int* w = nullptr;
    CHECK(p3.get(&w, 1, false) == hipSuccess && live.size() == 4);
    p3 = std::move(p2);   // frees w, takes x and y
    CHECK(n_free == f0 + 1 && !live.count(w) && live.count(x) && live.count(y));
    p2.clear();
    CHECK(n_free == f0 + 1);
    p3.release(x);
    CHECK(n_free == f0 + 2 && !live.count(x));
    static_assert(!std::is_copy_constructible<DevPool>::value && !std::is_copy_assignable<DevPool>::value, "a pool is not copyable");
    static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "a buffer is not copyable");
  }
  // (g) nothing is live at exit, nothing was freed twice or freed without being owned
  CHECK(live.empty() && n_free == n_malloc && foreign_free == 0);
  std::printf("dev_mem ok: %d checks, %d blocks\n", checks, n_malloc);
  return 0;
}
