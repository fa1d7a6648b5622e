// kh_buf.h — the one owning buffer type of the library, and the accounting every allocation goes through.
// Host-only and free of HIP: what allocates is a policy, so the type is tested on the CPU with a malloc-backed one
// (tests/cpp/test_buf.cpp).  The device and pinned-host policies live in kh_model_internal.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>

namespace khm {

constexpr int KH_BUF_OK = 0;
constexpr int KH_BUF_OOM = 2;  // hipErrorOutOfMemory (kh_model_internal.h asserts the value)

// Process-wide: what the buffers of every model hold, and the hook KH_ALLOC_FAIL=k (kh_debug.cpp) - the k-th
// allocation after the hook was last set or cleared fails without reaching the policy.
struct KhAllocStats {
  std::atomic<int64_t> live{0}, live_bytes{0};
  std::atomic<int64_t> allocs{0}, injected{0};  // since the hook was last set or cleared
  std::atomic<int64_t> fail_at{0};              // 0: hook unset
};
inline KhAllocStats& alloc_stats() {
  static KhAllocStats s;
  return s;
}
inline void alloc_fail_set(const char* value) {  // nullptr: unset
  KhAllocStats& s = alloc_stats();
  const long long k = value ? atoll(value) : 0;
  s.fail_at.store(k > 0 ? k : 0, std::memory_order_relaxed);
  s.allocs.store(0, std::memory_order_relaxed);
  s.injected.store(0, std::memory_order_relaxed);
}

template <class Mem>
int counted_alloc(void** p, size_t bytes) {
  KhAllocStats& s = alloc_stats();
  const int64_t k = s.fail_at.load(std::memory_order_relaxed);
  const int64_t ordinal = s.allocs.fetch_add(1, std::memory_order_relaxed) + 1;
  *p = nullptr;
  if (k > 0 && ordinal == k) {
    s.injected.fetch_add(1, std::memory_order_relaxed);
    return KH_BUF_OOM;
  }
  const int rc = Mem::alloc(p, bytes);
  if (rc != KH_BUF_OK) {
    *p = nullptr;
    return rc;
  }
  s.live.fetch_add(1, std::memory_order_relaxed);
  s.live_bytes.fetch_add((int64_t)bytes, std::memory_order_relaxed);
  return KH_BUF_OK;
}
template <class Mem>
void counted_free(void* p, size_t bytes) {
  KhAllocStats& s = alloc_stats();
  Mem::free(p);
  s.live.fetch_sub(1, std::memory_order_relaxed);
  s.live_bytes.fetch_sub((int64_t)bytes, std::memory_order_relaxed);
}

// n elements of T from Mem.  Move-only; the destructor frees, and so does whatever replaces the contents.  Converts
// to T* so that the sites that read a buffer (kernel-argument fills, pointer arithmetic) look as they would with a
// raw pointer; a site that reinterprets the pointer takes get().
template <class T, class Mem>
class KhBuf {
 public:
  KhBuf() = default;
  KhBuf(const KhBuf&) = delete;
  KhBuf& operator=(const KhBuf&) = delete;
  KhBuf(KhBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) {
    o.p_ = nullptr;
    o.bytes_ = 0;
  }
  KhBuf& operator=(KhBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      bytes_ = o.bytes_;
      o.p_ = nullptr;
      o.bytes_ = 0;
    }
    return *this;
  }
  ~KhBuf() { reset(); }

  // frees what the buffer held, then allocates; empty on failure
  int alloc(size_t n) {
    reset();
    void* q = nullptr;
    const int rc = counted_alloc<Mem>(&q, n * sizeof(T));
    if (rc != KH_BUF_OK) return rc;
    p_ = static_cast<T*>(q);
    bytes_ = n * sizeof(T);
    return KH_BUF_OK;
  }
  int ensure(size_t n) { return p_ && size() >= n ? KH_BUF_OK : alloc(n); }
  void reset() {
    if (p_) counted_free<Mem>(p_, bytes_);  // (bytes, not elements: T may be incomplete where a holder is destroyed)
    p_ = nullptr;
    bytes_ = 0;
  }
  T* get() const { return p_; }
  size_t size() const { return bytes_ / sizeof(T); }
  explicit operator bool() const { return p_ != nullptr; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace khm
