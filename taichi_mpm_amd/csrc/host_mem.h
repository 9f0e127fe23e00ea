// taichi_mpm_amd/csrc/host_mem.h — owners of the host layer's device and pinned arrays (host only; no kernel sees these types)
// DevBuf<T> owns one hipMalloc'ed array, PinnedBuf<T> one hipHostMalloc'ed array.  Both hold the pointer alone (capacities stay
// with the code that sizes the array), convert to T* wherever a pointer is read, move but do not copy, and release on destruction
// ON THE CURRENT DEVICE: whoever deletes an object that holds them sets the device first.
// What a kernel takes by value or what is copied to the device (Params, LevelSetDev, CdfDev, ...) keeps raw pointers: views, set
// where the owner is allocated.
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <utility>

namespace hostmem {

// live buffers of both kinds in this process (buffers, not bytes): mpmhip_debug_live_buffers
inline std::atomic<int64_t> g_live_buffers{0};

struct DeviceAlloc {
  static constexpr hipMemcpyKind copy_kind = hipMemcpyDeviceToDevice;
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void *p) { (void)hipFree(p); }
};
struct PinnedAlloc {
  static constexpr hipMemcpyKind copy_kind = hipMemcpyHostToHost;
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void *p) { (void)hipHostFree(p); }
};

template <typename T, typename A>
class Buf {
 public:
  Buf() = default;
  Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
    return *this;
  }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  ~Buf() { reset(); }

  // a new array of `count` elements, contents undefined; what was held is released first.  On failure the buffer holds nothing.
  hipError_t alloc(size_t count) {
    reset();
    return take(&p_, count);
  }
  // a new array of `count` elements holding the first `keep` elements of the old one (the rest zero-filled when `zero`); the old
  // array is released.  On failure the old array and its contents stay.
  hipError_t regrow(size_t keep, size_t count, bool zero) {
    T *q = nullptr;
    hipError_t e = take(&q, count);
    if (e != hipSuccess) return e;
    if (zero) e = hipMemset(q, 0, count * sizeof(T));
    if (e == hipSuccess && keep && p_) e = hipMemcpy(q, p_, keep * sizeof(T), A::copy_kind);
    if (e != hipSuccess) { drop(q); return e; }
    reset();
    p_ = q;
    return hipSuccess;
  }
  void reset() { drop(std::exchange(p_, nullptr)); }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  T *operator->() const { return p_; }

 private:
  static hipError_t take(T **p, size_t count) {
    void *q = nullptr;
    const hipError_t e = A::alloc(&q, count * sizeof(T));
    if (e != hipSuccess) return e;
    if (q) g_live_buffers.fetch_add(1, std::memory_order_relaxed);
    *p = static_cast<T *>(q);
    return hipSuccess;
  }
  static void drop(T *p) {
    if (!p) return;
    A::release(p);
    g_live_buffers.fetch_sub(1, std::memory_order_relaxed);
  }
  T *p_ = nullptr;
};

}  // namespace hostmem

template <typename T> using DevBuf = hostmem::Buf<T, hostmem::DeviceAlloc>;
template <typename T> using PinnedBuf = hostmem::Buf<T, hostmem::PinnedAlloc>;
