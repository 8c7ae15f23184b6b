// The one owner of a buffer the library allocates (plain C++, no HIP: the host files
// instantiate it over hipFree / hipHostFree in mfgp_host.h, tests/own_main.cpp over a
// counting fake).
//
//   Owner<T, Free>   a pointer and its size in bytes; move-only; frees in its destructor
//   Live             the count and the bytes of one kind of buffer held (mfgp_debug_live)
//   fill             the one allocation path: whoever calls it gets a buffer and its
//                    extent together, or an empty owner
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace mfgp_own __attribute__((visibility("hidden"))) {

struct Live {
  std::atomic<int64_t> count{0}, bytes{0};
  void add(size_t b) {
    count.fetch_add(1, std::memory_order_relaxed);
    bytes.fetch_add((int64_t)b, std::memory_order_relaxed);
  }
  void sub(size_t b) {
    count.fetch_sub(1, std::memory_order_relaxed);
    bytes.fetch_sub((int64_t)b, std::memory_order_relaxed);
  }
};

// Free(p, bytes) gives the buffer back (and takes it off its Live). Reads as a T*
// wherever one is expected (d.A = m->A, m->X + 2 * at, if (m->V)); casts and
// dereferences of the whole owner go through get().
template <class T, void (*Free)(void*, size_t)>
class Owner {
  T* p_ = nullptr;
  size_t bytes_ = 0;

 public:
  Owner() = default;
  Owner(T* p, size_t bytes) : p_(p), bytes_(p ? bytes : 0) {}   // adopts p (bytes: what its allocation counted)
  Owner(Owner&& o) noexcept : p_(o.p_), bytes_(o.bytes_) {
    o.p_ = nullptr;
    o.bytes_ = 0;
  }
  Owner& operator=(Owner&& o) noexcept {
    if (this != &o) {
      reset();
      swap(o);
    }
    return *this;
  }
  Owner(const Owner&) = delete;
  Owner& operator=(const Owner&) = delete;
  ~Owner() { reset(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t bytes() const { return bytes_; }
  void reset() {
    if (p_) Free(const_cast<void*>(static_cast<const void*>(p_)), bytes_);
    p_ = nullptr;
    bytes_ = 0;
  }
  // the caller's from here on (still counted live until someone adopts and frees it)
  T* release() {
    T* p = p_;
    p_ = nullptr;
    bytes_ = 0;
    return p;
  }
  void swap(Owner& o) noexcept {
    T* p = p_;
    const size_t b = bytes_;
    p_ = o.p_;
    bytes_ = o.bytes_;
    o.p_ = p;
    o.bytes_ = b;
  }
};

// o's buffer replaced by a fresh one of `bytes`: the old one freed FIRST (a large buffer
// never exists twice), then raw(&p, bytes) (0: success). On failure o stays empty with
// size 0 and failed(bytes) is the return code.
template <class T, void (*Free)(void*, size_t), class Raw, class Failed>
int fill(Owner<T, Free>& o, size_t bytes, Live& live, Raw raw, Failed failed) {
  o.reset();
  if (bytes == 0) return 0;   // (nothing asked for: the empty owner)
  void* p = nullptr;
  if (raw(&p, bytes) != 0 || !p) return failed(bytes);
  live.add(bytes);
  o = Owner<T, Free>(static_cast<T*>(p), bytes);
  return 0;
}

}  // namespace mfgp_own
