// Stand-alone check of the buffer owner (csrc/mfgp_own.h) over a counting fake instead of
// the HIP allocator: compiled and run by tests/test_own.py with the host compiler and
// -fsanitize=address,undefined (a double free or a leak of the fake's malloc'd blocks ends
// the program with the sanitizer's report). Prints "ok" and exits 0, or the failed check.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "mfgp_own.h"

namespace {

mfgp_own::Live live;
int frees = 0;
bool refuse = false;   // the fake allocator's answer

void fake_free(void* p, size_t bytes) {
  std::free(p);
  live.sub(bytes);
  ++frees;
}
int fake_raw(void** p, size_t bytes) {
  if (refuse) return 2;   // (an error code, *p untouched)
  *p = std::malloc(bytes);
  return *p ? 0 : 2;
}
int last_refused = 0;
int fake_failed(size_t bytes) {
  last_refused = (int)bytes;
  return 3;   // (stands for MFGP_ERR_DEVICE)
}
using Buf = mfgp_own::Owner<double, fake_free>;
using Raw = mfgp_own::Owner<void, fake_free>;   // the untyped instance (V, Vc)

int alloc(Buf& b, size_t bytes) { return mfgp_own::fill(b, bytes, live, fake_raw, fake_failed); }

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

bool held(int64_t count, int64_t bytes) { return live.count.load() == count && live.bytes.load() == bytes; }

}  // namespace

int main() {
  {   // allocation, the implicit pointer, reset
    Buf a;
    CHECK(!a && a.get() == nullptr && a.bytes() == 0);
    CHECK(alloc(a, 80) == 0 && a && a.bytes() == 80 && held(1, 80));
    double* p = a;   // reads as a T*
    p[9] = 1.0;
    CHECK(a[9] == 1.0 && a + 1 == p + 1);
    a.reset();
    CHECK(!a && a.bytes() == 0 && frees == 1 && held(0, 0));
    a.reset();   // an empty owner: nothing to free
    CHECK(frees == 1);
  }
  CHECK(frees == 1 && held(0, 0));   // the destructor of an empty owner frees nothing
  frees = 0;
  {   // move construction frees exactly once, at the end of the new owner
    Buf a;
    CHECK(alloc(a, 16) == 0);
    double* p = a;
    Buf b(std::move(a));
    CHECK(!a && a.bytes() == 0 && b.get() == p && b.bytes() == 16 && frees == 0 && held(1, 16));
  }
  CHECK(frees == 1 && held(0, 0));
  frees = 0;
  {   // move assignment frees the target's old buffer once, and the moved one once at the end
    Buf a, b;
    CHECK(alloc(a, 16) == 0 && alloc(b, 32) == 0 && held(2, 48));
    double* p = a;
    b = std::move(a);
    CHECK(frees == 1 && !a && b.get() == p && b.bytes() == 16 && held(1, 16));
    Buf& self = b;
    b = std::move(self);   // self-move: harmless
    CHECK(frees == 1 && b.get() == p && b.bytes() == 16 && held(1, 16));
  }
  CHECK(frees == 2 && held(0, 0));
  frees = 0;
  {   // release does not free; adoption takes the buffer back, counted all along
    Buf a;
    CHECK(alloc(a, 24) == 0);
    double* p = a.release();
    CHECK(p && !a && a.bytes() == 0 && frees == 0 && held(1, 24));
    Buf b(p, 24);
    CHECK(b.get() == p && b.bytes() == 24 && frees == 0 && held(1, 24));
  }
  CHECK(frees == 1 && held(0, 0));
  frees = 0;
  {   // swap frees nothing and exchanges pointer and size; with an empty owner too
    Buf a, b, e;
    CHECK(alloc(a, 8) == 0 && alloc(b, 40) == 0);
    double *pa = a, *pb = b;
    a.swap(b);
    CHECK(frees == 0 && a.get() == pb && a.bytes() == 40 && b.get() == pa && b.bytes() == 8 && held(2, 48));
    a.swap(e);
    CHECK(frees == 0 && !a && a.bytes() == 0 && e.get() == pb && e.bytes() == 40);
    a.swap(a);
    CHECK(frees == 0 && !a);
  }
  CHECK(frees == 2 && held(0, 0));
  frees = 0;
  {   // a failed allocation: the old buffer freed first, then pointer null and size 0
    Buf a;
    CHECK(alloc(a, 64) == 0);
    refuse = true;
    CHECK(alloc(a, 1000) == 3 && last_refused == 1000);
    CHECK(!a && a.get() == nullptr && a.bytes() == 0 && frees == 1 && held(0, 0));
    CHECK(alloc(a, 1000) == 3 && !a && a.bytes() == 0 && frees == 1);   // again, from empty
    refuse = false;
    CHECK(alloc(a, 48) == 0 && a && a.bytes() == 48 && held(1, 48));   // and the owner still serves
    CHECK(alloc(a, 0) == 0 && !a && a.bytes() == 0 && held(0, 0));     // no bytes: empty, no error
  }
  CHECK(frees == 2 && held(0, 0));
  frees = 0;
  {   // the untyped instance
    Raw v;
    CHECK(mfgp_own::fill(v, 128, live, fake_raw, fake_failed) == 0 && v && v.bytes() == 128);
    void* p = v;
    CHECK(static_cast<char*>(v.get()) == static_cast<char*>(p) && held(1, 128));
  }
  CHECK(frees == 1);
  CHECK(held(0, 0));   // the counts return to zero
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
