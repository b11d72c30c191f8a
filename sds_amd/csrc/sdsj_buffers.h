// sdsj_buffers.h -- owners for the engine's and the service's device / pinned arrays, streams and
// events, and the layout of a staged batch of the host paths.
//
// The templates and stage_layout use the standard library only (tests/asan/buffers_driver.cpp builds
// them with a counting allocator); the HIP policies at the end exist only under hipcc.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sdsj {

// Move-only owner of `size()` elements of T.  Alloc: `static void* alloc(size_t bytes)` (null on
// failure) and `static void free(void*)`.
template <class T, class Alloc>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }
  // Replaces the allocation (the old contents are gone) by one of `count` elements; on failure the
  // buffer is empty.
  bool reserve(size_t count) {
    reset();
    p_ = static_cast<T*>(Alloc::alloc(sizeof(T) * count));
    n_ = p_ ? count : 0;
    return p_ != nullptr;
  }
  void reset() {
    if (p_) Alloc::free(p_);
    p_ = nullptr, n_ = 0;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// Move-only owner of a pointer-like handle (stream, event, engine); Destroy: `static void destroy(H)`.
template <class H, class Destroy>
class Handle {
 public:
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = H(); }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = H();
    }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() {
    if (h_) Destroy::destroy(h_);
    h_ = H();
  }
  H get() const { return h_; }
  H* put() {  // for a create call; the handle must be empty
    reset();
    return &h_;
  }
  explicit operator bool() const { return h_ != H(); }

 private:
  H h_ = H();
};

// A staged batch of the host paths, one region sent with one H2D copy: m samples at 16-byte-aligned
// offsets from 0 (sample_bytes: the sum of their lengths, each rounded up to 16), then their offsets
// (int64), lengths (int32) and flip bytes, each array 16-byte aligned.  The sample region ends at
// `offsets`: that, not `total`, is the blob size k_parse checks the samples against.
struct StageLayout {
  int64_t offsets = 0, lengths = 0, flip = 0, total = 0;
};

inline StageLayout stage_layout(int m, int64_t sample_bytes) {
  const auto up16 = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
  StageLayout l;
  l.offsets = up16(sample_bytes);
  l.lengths = l.offsets + up16((int64_t)m * 8);
  l.flip = l.lengths + up16((int64_t)m * 4);
  l.total = l.flip + up16(m);
  return l;
}

}  // namespace sdsj

#ifdef __HIP__
#include <hip/hip_runtime.h>

namespace sdsj {

struct DeviceAlloc {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
  }
  static void free(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes) == hipSuccess ? p : nullptr;
  }
  static void free(void* p) { (void)hipHostFree(p); }
};
template <class T>
using DeviceBuf = Buf<T, DeviceAlloc>;
template <class T>
using PinnedBuf = Buf<T, PinnedAlloc>;

struct StreamDestroy {
  static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};
struct EventDestroy {
  static void destroy(hipEvent_t ev) { (void)hipEventDestroy(ev); }
};
using Stream = Handle<hipStream_t, StreamDestroy>;
using Event = Handle<hipEvent_t, EventDestroy>;

}  // namespace sdsj
#endif
