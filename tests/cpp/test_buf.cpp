// test_buf.cpp — KhBuf (kuiperllama_amd/csrc/kh_buf.h) over a malloc-backed policy: ownership, moves, the failure
// paths, the process-wide counters and the KH_ALLOC_FAIL ordinal.  Host only; built with the address and
// undefined-behaviour sanitizers by tests/test_buf.py, so a double free, a leak or a use after free ends the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>

#include "../../kuiperllama_amd/csrc/kh_buf.h"

namespace {
int g_fail = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                      \
    }                                                                \
  } while (0)

// the policy's own books: what reached it, whatever the library's counters say
struct Heap {
  static long allocs, frees, refuse_in;  // refuse_in: > 0 counts down, the call that reaches 0 is refused
  static int alloc(void** p, size_t bytes) {
    if (refuse_in > 0 && --refuse_in == 0) return 7;
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return khm::KH_BUF_OOM;
    memset(*p, 0xA5, bytes);
    ++allocs;
    return khm::KH_BUF_OK;
  }
  static void free(void* p) {
    ++frees;
    ::free(p);
  }
};
long Heap::allocs = 0, Heap::frees = 0, Heap::refuse_in = 0;

using Buf = khm::KhBuf<int32_t, Heap>;
struct Words;  // never completed: a holder of KhBuf<Words, .> can still be destroyed
struct Holder {
  khm::KhBuf<Words, Heap> b;
};

int64_t live() { return khm::alloc_stats().live.load(); }
int64_t live_bytes() { return khm::alloc_stats().live_bytes.load(); }
int64_t made() { return khm::alloc_stats().allocs.load(); }
int64_t injected() { return khm::alloc_stats().injected.load(); }

void test_alloc_ensure_reset() {
  Buf b;
  CHECK(!b && b.get() == nullptr && b.size() == 0);
  CHECK(b.alloc(10) == khm::KH_BUF_OK);
  CHECK(b && b.size() == 10 && live() == 1 && live_bytes() == 40);
  int32_t* p = b;  // the implicit conversion use sites rely on
  CHECK(p == b.get());
  p[9] = 3;
  CHECK((b + 9)[0] == 3);
  CHECK(b.ensure(10) == khm::KH_BUF_OK && b.get() == p);  // enough: untouched
  CHECK(b.ensure(4) == khm::KH_BUF_OK && b.get() == p && b.size() == 10);
  const long frees = Heap::frees;
  CHECK(b.ensure(11) == khm::KH_BUF_OK && b.size() == 11 && Heap::frees == frees + 1);
  CHECK(live() == 1 && live_bytes() == 44);
  CHECK(b.alloc(2) == khm::KH_BUF_OK && b.size() == 2 && live() == 1 && live_bytes() == 8);  // alloc always replaces
  b.reset();
  CHECK(!b && b.size() == 0 && live() == 0 && live_bytes() == 0);
  b.reset();  // idempotent
  CHECK(Heap::allocs == Heap::frees);
}

void test_moves() {
  Buf a, b;
  CHECK(a.alloc(3) == khm::KH_BUF_OK && b.alloc(5) == khm::KH_BUF_OK);
  int32_t* pa = a;
  Buf c(std::move(a));  // move construction: the source is empty, nothing is freed
  CHECK(!a && a.size() == 0 && c.get() == pa && c.size() == 3 && live() == 2);
  const long frees = Heap::frees;
  b = std::move(c);  // onto a full buffer: its old contents are freed, once
  CHECK(Heap::frees == frees + 1 && !c && b.get() == pa && b.size() == 3 && live() == 1 && live_bytes() == 12);
  Buf& self = b;
  b = std::move(self);  // self-assignment keeps the contents
  CHECK(b.get() == pa && b.size() == 3 && live() == 1);
  a = Buf();  // an empty one onto an empty one
  CHECK(!a && live() == 1);
  {
    Buf scoped(std::move(b));
    CHECK(live() == 1);
  }  // the destructor frees
  CHECK(live() == 0 && live_bytes() == 0 && Heap::allocs == Heap::frees);
}

void test_failing_policy() {
  Buf b;
  CHECK(b.alloc(6) == khm::KH_BUF_OK);
  const long frees = Heap::frees, allocs = Heap::allocs;
  Heap::refuse_in = 1;
  CHECK(b.alloc(8) == 7);  // the policy's code comes back as it is
  CHECK(!b && b.get() == nullptr && b.size() == 0);                // empty
  CHECK(Heap::frees == frees + 1 && Heap::allocs == allocs);       // the old contents went, exactly once
  CHECK(live() == 0 && live_bytes() == 0);
  Heap::refuse_in = 1;
  CHECK(b.ensure(1) == 7 && !b && Heap::frees == frees + 1);       // nothing to free the second time
  CHECK(b.alloc(1) == khm::KH_BUF_OK && live() == 1);
}  // ... and the destructor frees what the retry got

void test_hook_ordinal() {
  khm::alloc_fail_set(nullptr);
  CHECK(made() == 0 && injected() == 0);
  Buf a, b, c;
  CHECK(a.alloc(1) == khm::KH_BUF_OK && made() == 1);
  khm::alloc_fail_set("2");  // setting restarts the ordinal
  CHECK(made() == 0 && injected() == 0);
  const long reached = Heap::allocs;
  CHECK(a.alloc(1) == khm::KH_BUF_OK);            // 1st
  CHECK(b.alloc(4) == khm::KH_BUF_OOM && !b);     // 2nd: injected, the policy is not reached
  CHECK(Heap::allocs == reached + 1 && injected() == 1 && made() == 2);
  CHECK(b.alloc(4) == khm::KH_BUF_OK && c.alloc(4) == khm::KH_BUF_OK);  // 3rd, 4th: only the k-th fails
  CHECK(injected() == 1 && made() == 4 && live() == 3);
  khm::alloc_fail_set("1");  // resetting restarts it again; a full buffer loses its contents to the failed call
  CHECK(c.alloc(9) == khm::KH_BUF_OOM && !c && live() == 2 && injected() == 1 && made() == 1);
  khm::alloc_fail_set(nullptr);  // cleared: nothing fails, the count starts over
  CHECK(made() == 0 && injected() == 0);
  CHECK(c.alloc(9) == khm::KH_BUF_OK && made() == 1 && injected() == 0);
  khm::alloc_fail_set("0");  // not an ordinal: off
  CHECK(c.alloc(9) == khm::KH_BUF_OK && injected() == 0);
  khm::alloc_fail_set(nullptr);
}

void test_incomplete_element_type() {
  Holder h;
  CHECK(!h.b);
  Holder g(std::move(h));
  CHECK(!g.b && live() == 0);
}
}  // namespace

int main() {
  test_alloc_ensure_reset();
  test_moves();
  test_failing_policy();
  test_hook_ordinal();
  test_incomplete_element_type();
  CHECK(live() == 0 && live_bytes() == 0 && Heap::allocs == Heap::frees);
  if (g_fail) {
    fprintf(stderr, "test_buf: %d check(s) failed\n", g_fail);
    return 1;
  }
  printf("test_buf: ok (%ld allocations reached the policy)\n", Heap::allocs);
  return 0;
}
