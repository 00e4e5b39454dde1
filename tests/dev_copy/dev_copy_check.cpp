// Stand-alone check of csrc/dev_copy.h on the host heap (tests/test_dev_copy.py builds it with -fsanitize=address,undefined and runs it).
// hipMemcpy, hipMemcpyAsync, hipStreamSynchronize and hipGetErrorString are stubs here: the copies memcpy, every call is recorded with its byte
// count, kind and stream, and the k-th call fails on demand.  Every buffer is sized exactly, so a copy that is too long is ASan's finding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dev_copy.h"

namespace {
struct Call { char op; size_t bytes; int kind; hipStream_t st; };   // op: 'c' blocking copy, 'a' queued copy, 'w' wait
std::vector<Call> calls;
int fail_at = -1;        // the call with this index fails (counted from the last arm()) ...
bool fail_after = false; // ... and with fail_after every later one too
int request = 0;
void arm(int k, bool after = false) { fail_at = k; fail_after = after; request = 0; calls.clear(); }
hipError_t verdict() {
  const int i = request++;
  return fail_at >= 0 && (i == fail_at || (fail_after && i > fail_at)) ? hipErrorInvalidValue : hipSuccess;
}
const char* const kInvalid = "stub: invalid value";
const char* const kNoMem = "stub: out of memory";
int checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
hipStream_t fake_stream(uintptr_t v) { return reinterpret_cast<hipStream_t>(v); }   // never dereferenced
bool ends_with(const std::string& s, const char* tail) { const size_t n = std::strlen(tail); return s.size() >= n && s.compare(s.size() - n, n, tail) == 0; }
}  // namespace

extern "C" {
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  calls.push_back(Call{'c', bytes, (int)kind, nullptr});
  const hipError_t e = verdict();
  if (e == hipSuccess) std::memcpy(dst, src, bytes);
  return e;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  calls.push_back(Call{'a', bytes, (int)kind, st});
  const hipError_t e = verdict();
  if (e == hipSuccess) std::memcpy(dst, src, bytes);
  return e;
}
hipError_t hipStreamSynchronize(hipStream_t st) {
  calls.push_back(Call{'w', 0, -1, st});
  return verdict();
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorInvalidValue ? kInvalid : e == hipErrorOutOfMemory ? kNoMem : "stub: other"; }
}

namespace {
struct E16 { float v[4]; };
struct E48 { double v[6]; };
static_assert(sizeof(E16) == 16 && sizeof(E48) == 48, "element sizes of the byte-count cases");

template <class T> T* exact(size_t n) { return n ? static_cast<T*>(std::malloc(n * sizeof(T))) : nullptr; }   // n elements and not a byte more
template <class T> void fill(T* p, size_t n, unsigned char seed) { for (size_t i = 0; i < n * sizeof(T); ++i) reinterpret_cast<unsigned char*>(p)[i] = (unsigned char)(seed + i); }
bool last_is(char op, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  return !calls.empty() && calls.back().op == op && calls.back().bytes == bytes && calls.back().kind == (int)kind && calls.back().st == st;
}

// upload and download of n elements of T, blocking and queued, by pointer and by vector: one stub call of n * sizeof(T) bytes each, none for n == 0
template <class T> void byte_counts(size_t n) {
  const hipStream_t S = fake_stream(0x40);
  const size_t bytes = n * sizeof(T);
  const size_t want = n ? 1 : 0;
  T* dev = exact<T>(n);
  std::vector<T> host(n), back(n);
  if (n) fill(host.data(), n, 3);
  arm(-1);
  CHECK(dev_up(dev, host.data(), n) == hipSuccess && calls.size() == want && (!n || last_is('c', bytes, hipMemcpyHostToDevice, nullptr)));
  CHECK(!n || std::memcmp(dev, host.data(), bytes) == 0);
  CHECK(dev_down(back.data(), dev, n) == hipSuccess && calls.size() == 2 * want && (!n || last_is('c', bytes, hipMemcpyDeviceToHost, nullptr)));
  CHECK(!n || std::memcmp(back.data(), host.data(), bytes) == 0);
  arm(-1);
  CHECK(dev_up(dev, host.data(), n, S) == hipSuccess && calls.size() == want && (!n || last_is('a', bytes, hipMemcpyHostToDevice, S)));
  CHECK(dev_down(back.data(), dev, n, S) == hipSuccess && calls.size() == 2 * want && (!n || last_is('a', bytes, hipMemcpyDeviceToHost, S)));
  arm(-1);
  CHECK(dev_up(dev, host) == hipSuccess && calls.size() == want && (!n || last_is('c', bytes, hipMemcpyHostToDevice, nullptr)));
  CHECK(dev_down(back, dev) == hipSuccess && calls.size() == 2 * want && (!n || last_is('c', bytes, hipMemcpyDeviceToHost, nullptr)));
  CHECK(dev_up(dev, host, S) == hipSuccess && calls.size() == 3 * want && (!n || last_is('a', bytes, hipMemcpyHostToDevice, S)));
  CHECK(dev_down(back, dev, S) == hipSuccess && calls.size() == 4 * want && (!n || last_is('a', bytes, hipMemcpyDeviceToHost, S)));
  CHECK(!n || std::memcmp(back.data(), host.data(), bytes) == 0);
  // a null stream is still a queued copy: hipStream_t decides, not its value
  arm(-1);
  const hipStream_t null_stream = nullptr;
  CHECK(dev_up(dev, host.data(), n, null_stream) == hipSuccess && calls.size() == want && (!n || last_is('a', bytes, hipMemcpyHostToDevice, nullptr)));
  // the same through a chain
  arm(-1);
  std::string err = "untouched";
  DevTry c("counts", &err);
  CHECK(c.up(dev, host).down(back, dev, S).up(dev, host.data(), n, S).down(back.data(), dev, n) == 0 && c.ok() && err == "untouched" && calls.size() == 4 * want);
  std::free(dev);
}
// the array overloads: N elements, from the array's type
template <class T, size_t N> void array_counts() {
  const hipStream_t S = fake_stream(0x48);
  T a[N], b[N];
  fill(a, N, 9);
  T* dev = exact<T>(N);
  arm(-1);
  CHECK(dev_up(dev, a) == hipSuccess && last_is('c', N * sizeof(T), hipMemcpyHostToDevice, nullptr));
  CHECK(dev_down(b, dev) == hipSuccess && last_is('c', N * sizeof(T), hipMemcpyDeviceToHost, nullptr) && std::memcmp(a, b, sizeof(a)) == 0);
  CHECK(dev_up(dev, a, S) == hipSuccess && last_is('a', N * sizeof(T), hipMemcpyHostToDevice, S));
  CHECK(dev_down(b, dev, S) == hipSuccess && last_is('a', N * sizeof(T), hipMemcpyDeviceToHost, S) && calls.size() == 4);
  const T(&ca)[N] = a;   // a const array uploads too
  CHECK(dev_up(dev, ca) == hipSuccess && calls.size() == 5);
  std::free(dev);
}
template <class T> void counts_of() {
  for (size_t n : {(size_t)0, (size_t)1, (size_t)5}) byte_counts<T>(n);
  array_counts<T, 1>();
  array_counts<T, 5>();
}

// a chain of N = 5 operations, one stub call each: upload, queued upload, wait, queued download, download
constexpr int N = 5;
const char* const kStep[N] = {"upload", "upload", "a stream", "device read", "device read"};
int chain(DevTry& c, int* dev, const std::vector<int>& host, std::vector<int>& back, hipStream_t S) {
  return c.up(dev, host).up(dev, host, S).wait(S).down(back, dev, S).down(back, dev);
}
}  // namespace

int main() {
  // (a) byte counts and kinds: element types of 1, 2, 4, 8, 16 and 48 bytes, n in {0, 1, 5}, every overload
  counts_of<uint8_t>(); counts_of<uint16_t>(); counts_of<float>(); counts_of<double>(); counts_of<E16>(); counts_of<E48>();
  {
    // (b) the 16-byte pair alego_point <-> float4, both ways round
    alego_point host[5], back[5];
    fill(host, 5, 1);
    float4* dev = exact<float4>(5);
    arm(-1);
    CHECK(dev_up(dev, host, 5) == hipSuccess && last_is('c', 80, hipMemcpyHostToDevice, nullptr));
    CHECK(dev_down(back, dev, 5) == hipSuccess && last_is('c', 80, hipMemcpyDeviceToHost, nullptr) && std::memcmp(host, back, 80) == 0);
    CHECK(dev_up(dev, host) == hipSuccess && last_is('c', 80, hipMemcpyHostToDevice, nullptr));
    std::vector<float4> hv(5);
    alego_point* dev_pt = exact<alego_point>(5);
    CHECK(dev_up(dev_pt, hv) == hipSuccess && last_is('c', 80, hipMemcpyHostToDevice, nullptr) && calls.size() == 4);
    std::free(dev); std::free(dev_pt);
    // the byte-wise download of the debug getters
    unsigned char src7[7] = {1, 2, 3, 4, 5, 6, 7};
    void* out = std::malloc(7);
    arm(-1);
    CHECK(dev_down_bytes(out, src7, 7) == hipSuccess && last_is('c', 7, hipMemcpyDeviceToHost, nullptr) && std::memcmp(out, src7, 7) == 0);
    CHECK(dev_down_bytes(nullptr, nullptr, 0) == hipSuccess && calls.size() == 1);
    std::free(out);
  }
  {
    // (c) a count of zero with null pointers on both sides: success, and no stub call; an armed failure is not consumed either
    const hipStream_t S = fake_stream(0x50);
    arm(0);
    CHECK(dev_up((int*)nullptr, (const int*)nullptr, 0) == hipSuccess && dev_down((int*)nullptr, (const int*)nullptr, 0) == hipSuccess);
    CHECK(dev_up((E48*)nullptr, (const E48*)nullptr, 0, S) == hipSuccess && dev_down((float4*)nullptr, (const alego_point*)nullptr, 0, S) == hipSuccess);
    std::vector<double> none;
    CHECK(none.data() == nullptr || none.empty());
    CHECK(dev_up((double*)nullptr, none) == hipSuccess && dev_down(none, (const double*)nullptr, S) == hipSuccess);
    std::string err = "untouched";
    CHECK(DevTry("zero", &err).up((int*)nullptr, (const int*)nullptr, 0).down(none, (const double*)nullptr) == 0 && err == "untouched");
    CHECK(calls.empty() && request == 0);
  }
  {
    // (d) injected failures: the k-th of N operations fails, k = N: none
    const hipStream_t S = fake_stream(0x60);
    const std::vector<int> host = {1, 2, 3};
    std::vector<int> back(3);
    int* dev = exact<int>(3);
    for (int after = 0; after < 2; ++after)   // after: every call from the k-th on would fail; the first failure is the one kept
      for (int k = 0; k <= N; ++k) {
        arm(k, after != 0);
        std::string err = "untouched";
        DevTry c("chain_test", &err);
        const int rc = chain(c, dev, host, back, S);
        CHECK((int)calls.size() == (k < N ? k + 1 : N));
        CHECK(rc == (k < N ? ALEGO_ERR_HIP : 0) && c.ok() == (k == N) && (int)c == rc);
        if (k == N) { CHECK(err == "untouched" && back == host); continue; }
        CHECK(err == std::string("chain_test: ") + kStep[k] + " failed: " + kInvalid);
        CHECK(err.rfind("chain_test", 0) == 0 && err.find(kStep[k]) != std::string::npos && ends_with(err, kInvalid));
        // what follows a failure does nothing, whatever it is, and leaves the text alone
        const std::string first = err;
        const size_t made = calls.size();
        CHECK(c.at("later").up(dev, host).wait(S).took(hipErrorOutOfMemory, "allocation").down(back, dev) == ALEGO_ERR_HIP && err == first && calls.size() == made);
      }
    // the step a site names replaces the default noun, until the next one
    arm(1);
    std::string err;
    DevTry c(std::string("occ_") + "integrate", &err, "ray casting");
    CHECK(c.wait(S).down(back, dev) == ALEGO_ERR_HIP && err == std::string("occ_integrate: ray casting failed: ") + kInvalid && calls.size() == 2);
    arm(1);
    DevTry d("map_merge", &err, "upload");
    CHECK(d.up(dev, host).at("append").wait(S) == ALEGO_ERR_HIP && err == std::string("map_merge: append failed: ") + kInvalid);
    // (e) an error from outside (DevBuf::reserve) stops the chain the same way; hipSuccess from outside does not
    arm(-1);
    err = "untouched";
    DevTry e("thin", &err);
    CHECK(e.took(hipSuccess).up(dev, host).took(hipErrorOutOfMemory).up(dev, host).wait(S).down(back, dev) == ALEGO_ERR_HIP && !e.ok());
    CHECK(calls.size() == 1 && err == std::string("thin: allocation failed: ") + kNoMem);
    DevTry f("thin", &err, "upload");   // (the chain's own step wins over the one named with the error)
    CHECK(f.took(hipErrorOutOfMemory, "allocation").up(dev, host) == ALEGO_ERR_HIP && err == std::string("thin: upload failed: ") + kNoMem && calls.size() == 1);
    std::free(dev);
  }
  {
    // (f) a wait on a list visits every stream once, in order, also after one has failed; the first failure is reported
    const std::vector<hipStream_t> list = {fake_stream(0x70), fake_stream(0x78), fake_stream(0x80), fake_stream(0x88)};
    for (int k = -1; k < (int)list.size(); ++k) {
      arm(k, false);
      std::string err = "untouched";
      const int rc = DevTry("sync", &err).wait(list);
      CHECK(calls.size() == list.size());
      for (size_t i = 0; i < list.size(); ++i) CHECK(calls[i].op == 'w' && calls[i].st == list[i]);
      CHECK(rc == (k < 0 ? 0 : ALEGO_ERR_HIP) && (k < 0 ? err == "untouched" : err == std::string("sync: a stream failed: ") + kInvalid));
    }
    arm(1, true);   // the second and every later stream fail: all are still visited
    CHECK(dev_wait(list) == hipErrorInvalidValue && calls.size() == list.size());
    arm(0);
    CHECK(dev_wait(std::vector<hipStream_t>()) == hipSuccess && calls.empty());
    CHECK(dev_wait(list[2]) == hipErrorInvalidValue && calls.size() == 1 && calls[0].st == list[2]);
  }
  std::printf("dev_copy ok: %d checks\n", checks);
  return 0;
}
