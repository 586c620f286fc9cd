// mashmap_amd/csrc/mm_devbuf.h -- what the library owns of the runtime's: DevBuf, every byte of device memory; DevStream and DevEvent,
// every stream and event; PinnedBuf, every page-locked block but the public allocator's (mm_host_alloc).  Needs the HIP runtime's host
// API only (no device code), so that a host program can include it with a runtime of its own (tests/hostlogic/devbuf_check.cpp).
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

// A runtime handle that is created on request, once, and destroyed with its owner; moved but never copied.  Converts to the raw handle,
// so a launch or a copy names the member as it would name the handle (`h` itself where a macro or a template will not convert).
template <class H, hipError_t (*Destroy)(H)>
struct DevHandle {
  H h = nullptr;
  DevHandle() = default;
  DevHandle(const DevHandle&) = delete;
  DevHandle& operator=(const DevHandle&) = delete;
  DevHandle(DevHandle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  DevHandle& operator=(DevHandle&& o) noexcept {
    if (this != &o) { release(); h = std::exchange(o.h, nullptr); }
    return *this;
  }
  ~DevHandle() { release(); }
  void release() { if (h) (void)Destroy(h); h = nullptr; }
  operator H() const { return h; }
};
struct DevStream : DevHandle<hipStream_t, hipStreamDestroy> {   // non-blocking
  hipError_t ensure() {
    if (h) return hipSuccess;
    const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
    if (e != hipSuccess) h = nullptr;
    return e;
  }
};
struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy> {
  hipError_t ensure(unsigned flags = hipEventDefault) {
    if (h) return hipSuccess;
    const hipError_t e = hipEventCreateWithFlags(&h, flags);
    if (e != hipSuccess) h = nullptr;
    return e;
  }
};

// page-locked host memory.  ensure(need) keeps a block that fits; otherwise the old block goes first and exactly `need` bytes are asked
// for (the caller adds its own head room); a failure leaves it empty, with the runtime's sticky error cleared
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) { release(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); }
    return *this;
  }
  ~PinnedBuf() { release(); }
  hipError_t ensure(size_t need) {
    if (need <= bytes) return hipSuccess;
    release();
    const hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
    if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return e; }
    bytes = need;
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr; bytes = 0;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
