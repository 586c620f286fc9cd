// mashmap_amd/csrc/mm_devbuf.h -- DevBuf: every byte of device memory the library owns.  Needs the HIP runtime's host API only (no
// device code), so that a host program can include it with hipMalloc / hipFree of its own (tests/hostlogic/devbuf_check.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <chrono>
#include <stdint.h>
#include <utility>

// both atomic: prefetch, upload and the gather thread run ensure() concurrently
inline std::atomic<uint64_t> g_mmAllocNanos{0};  // nanoseconds of wall time inside hipMalloc / hipFree of DevBuf::ensure (MASHMAP_HIP_TIMING reports them per sized pass)
inline std::atomic<size_t> g_mmDeviceBytes{0};   // bytes all DevBufs of the process hold (mm_device_bytes)

// owns its allocation: freed by the destructor, moved but never copied
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t need) {          // grow-only; contents are NOT preserved
    if (need <= bytes) return hipSuccess;
    const auto t0 = std::chrono::steady_clock::now();
    // the new buffer first, with an eighth of head room; the old one is given up only once the new one is there -- or, when the device
    // cannot hold both, before a second attempt at the exact size (a failed growth leaves the buffer as it was whenever it can)
    void* q = nullptr;
    size_t cap = need + need / 8 + 256;
    hipError_t e = hipMalloc(&q, cap);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      release();
      e = hipMalloc(&q, cap);
      if (e != hipSuccess) { (void)hipGetLastError(); cap = need + 256; e = hipMalloc(&q, cap); }
    } else release();
    if (e == hipSuccess) { p = q; bytes = cap; g_mmDeviceBytes += cap; }
    g_mmAllocNanos.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(), std::memory_order_relaxed);
    return e;
  }
  void release() {
    if (p) { (void)hipFree(p); g_mmDeviceBytes -= bytes; }
    p = nullptr; bytes = 0;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
