// tests/hostlogic/devbuf_check.cpp -- DevBuf (mashmap_amd/csrc/mm_devbuf.h) on the host: ownership, the growth policy of ensure() with
// each of its failure paths, and the live-byte counter behind mm_device_bytes.  hipMalloc / hipFree / hipGetLastError are defined HERE,
// as counting fakes over malloc / free that can be told which of the next allocations fail; the HIP runtime is not linked.  Built with
// -fsanitize=address,undefined (a double free or a leak of the fake's memory ends the program) and run by tests/test_devbuf.py.
//
//   devbuf_check         prints "ok <case>" per case that passed, "FAIL ..." for a check that did not, then the summary lines
//                        "cases <n>", "mismatches <n>", "allocations <n> frees <n>"; the status is non-zero on any mismatch
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include "../../mashmap_amd/csrc/mm_devbuf.h"

static int failures = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the fake runtime --------------------------------------------------------------------------------------------------------------
static std::map<void*, size_t> live;          // what the fake has handed out and not taken back
static size_t liveBytes = 0, nAlloc = 0, nFree = 0, nStrayFree = 0;
static unsigned failMask = 0;                 // bit i: the i-th allocation from now fails
static std::string events;                    // 'M' allocation, 'x' failed allocation, 'F' free, 'e' hipGetLastError
static size_t lastAllocSize = 0;

extern "C" hipError_t hipMalloc(void** ptr, size_t size) {
  const bool fail = failMask & 1u; failMask >>= 1;
  if (fail) { events += 'x'; *ptr = nullptr; return hipErrorOutOfMemory; }
  void* q = malloc(size ? size : 1);
  if (!q) abort();
  live[q] = size; liveBytes += size; nAlloc++; lastAllocSize = size; events += 'M';
  *ptr = q;
  return hipSuccess;
}
extern "C" hipError_t hipFree(void* ptr) {
  events += 'F';
  auto it = live.find(ptr);
  if (it == live.end()) { nStrayFree++; return hipErrorInvalidValue; }   // never handed out, or freed before
  liveBytes -= it->second; live.erase(it); nFree++;
  free(ptr);
  return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { events += 'e'; return hipSuccess; }

static size_t head(size_t need) { return need + need / 8 + 256; }        // what ensure(need) allocates when it grows

// after every step: the counter is the sum of `bytes` of the buffers under test, and what the fake has outstanding
template <class... B> static void settled(const char* where, const B&... b) {
  const size_t sum = (size_t(0) + ... + b.bytes);
  CHECK(g_mmDeviceBytes.load() == sum, "%s: counter %zu, sum of bytes %zu", where, g_mmDeviceBytes.load(), sum);
  CHECK(liveBytes == sum && live.size() == (size_t(0) + ... + (b.p ? 1u : 0u)), "%s: the fake holds %zu bytes in %zu blocks, the buffers %zu", where, liveBytes, live.size(), sum);
  CHECK((((b.p == nullptr) == (b.bytes == 0)) && ...), "%s: a pointer without bytes or bytes without a pointer", where);
  CHECK(nStrayFree == 0, "%s: %zu frees of a pointer the fake does not hold", where, nStrayFree);
}
static void done(const char* name, int before) { cases++; if (failures == before) printf("ok %s\n", name); }

// ---- the cases ---------------------------------------------------------------------------------------------------------------------
static void fits_and_grows() {
  const int f0 = failures;
  {
    DevBuf b;
    settled("empty", b);
    CHECK(b.ensure(0) == hipSuccess && !b.p && events.empty(), "ensure(0) of an empty buffer allocates nothing");
    CHECK(b.ensure(1000) == hipSuccess && b.p && b.bytes == head(1000) && b.bytes == 1381, "first ensure: bytes %zu", b.bytes);
    CHECK(events == "M", "events %s", events.c_str());
    settled("first", b);
    void* p0 = b.p; events.clear();
    CHECK(b.ensure(1) == hipSuccess && b.ensure(1000) == hipSuccess && b.ensure(1381) == hipSuccess && b.p == p0 && b.bytes == 1381 && events.empty(),
          "a size that fits keeps the pointer (events %s)", events.c_str());
    settled("fits", b);
    CHECK(b.ensure(1382) == hipSuccess && b.bytes == head(1382) && live.count(b.p) && !live.count(p0), "growth: bytes %zu", b.bytes);
    CHECK(events == "MF", "growth is new-before-old: events %s", events.c_str());
    CHECK(b.as<char>() == (char*)b.p, "as<T>");
    settled("grown", b);
    events.clear();
  }
  CHECK(events == "F", "the destructor frees: events %s", events.c_str());
  events.clear();
  DevBuf none;
  settled("after the scope", none);
  done("fits_and_grows", f0);
}

static void failure_paths() {
  const int f0 = failures;
  {                                           // the first allocation fails, the second succeeds: the old buffer is given up in between
    DevBuf b;
    CHECK(b.ensure(4096) == hipSuccess, "setup");
    void* p0 = b.p; events.clear(); failMask = 1u;
    CHECK(b.ensure(10000) == hipSuccess && b.bytes == head(10000) && lastAllocSize == head(10000) && !live.count(p0), "bytes %zu", b.bytes);
    CHECK(events == "xeFM", "events %s", events.c_str());
    settled("one failure", b);
    events.clear();
  }
  events.clear();
  {                                           // the first two fail, the exact size succeeds
    DevBuf b;
    CHECK(b.ensure(4096) == hipSuccess, "setup");
    events.clear(); failMask = 3u;
    CHECK(b.ensure(10000) == hipSuccess && b.bytes == 10000 + 256 && lastAllocSize == 10000 + 256, "bytes %zu", b.bytes);
    CHECK(events == "xeFxeM", "events %s", events.c_str());
    settled("two failures", b);
  }
  events.clear();
  {                                           // all three fail: the buffer is empty, the error comes back
    DevBuf b, other;
    CHECK(b.ensure(4096) == hipSuccess && other.ensure(100) == hipSuccess, "setup");
    events.clear(); failMask = 7u;
    CHECK(b.ensure(10000) == hipErrorOutOfMemory && !b.p && b.bytes == 0, "p %p bytes %zu", b.p, b.bytes);
    CHECK(events == "xeFxex", "events %s", events.c_str());
    settled("three failures", b, other);
    CHECK(g_mmDeviceBytes.load() == head(100), "the counter fell by the buffer that was given up: %zu", g_mmDeviceBytes.load());
    events.clear(); failMask = 7u;            // ... and from empty: nothing to give up
    CHECK(b.ensure(10000) == hipErrorOutOfMemory && !b.p && b.bytes == 0 && events == "xexex", "events %s", events.c_str());
    settled("three failures from empty", b, other);
    CHECK(b.ensure(10000) == hipSuccess && b.bytes == head(10000), "the buffer is usable again");
    settled("after the failures", b, other);
  }
  events.clear();
  CHECK(failMask == 0, "every planned failure was taken");
  done("failure_paths", f0);
}

static void moves() {
  const int f0 = failures;
  {
    DevBuf a;
    CHECK(a.ensure(500) == hipSuccess, "setup");
    void* pa = a.p; const size_t na = a.bytes;
    events.clear();
    DevBuf b(std::move(a));                   // move construction
    CHECK(!a.p && !a.bytes && b.p == pa && b.bytes == na && events.empty(), "move construction (events %s)", events.c_str());
    settled("move constructed", a, b);
    DevBuf c;
    CHECK(c.ensure(700) == hipSuccess, "setup");
    void* pc = c.p; events.clear();
    c = std::move(b);                         // move assignment onto a full buffer
    CHECK(!b.p && !b.bytes && c.p == pa && c.bytes == na && !live.count(pc) && events == "F", "move assignment (events %s)", events.c_str());
    settled("move assigned", a, b, c);
    events.clear();
    DevBuf& self = c;
    c = std::move(self);                      // self-move
    CHECK(c.p == pa && c.bytes == na && events.empty(), "self-move (events %s)", events.c_str());
    settled("self-moved", a, b, c);
    CHECK(b.ensure(64) == hipSuccess, "setup");
    void* pb = b.p; const size_t nb = b.bytes; events.clear();
    std::swap(b, c);
    CHECK(b.p == pa && b.bytes == na && c.p == pb && c.bytes == nb && events.empty(), "std::swap (events %s)", events.c_str());
    settled("swapped", a, b, c);
    std::swap(a, b);                          // ... with an empty one
    CHECK(a.p == pa && !b.p && events.empty(), "std::swap with an empty buffer");
    settled("swapped with empty", a, b, c);
    events.clear();
    a.release(); a.release();                 // release twice
    CHECK(!a.p && !a.bytes && events == "F", "release twice frees once (events %s)", events.c_str());
    settled("released", a, b, c);
    b.release();                              // ... and of an empty buffer
    CHECK(events == "F", "release of an empty buffer (events %s)", events.c_str());
    settled("released empty", a, b, c);
  }
  events.clear();
  done("moves", f0);
}

struct Batch {                                // a struct of buffers beside plain fields, as the library's resident read batch
  size_t n = 0;
  DevBuf x, y;
  int tag = 0;
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf is not copyable");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "DevBuf moves without throwing");
static_assert(!std::is_copy_constructible<Batch>::value && std::is_nothrow_move_constructible<Batch>::value && std::is_nothrow_move_assignable<Batch>::value,
              "a struct of DevBufs is movable and not copyable");

static void structs() {
  const int f0 = failures;
  {
    Batch r, parked[2];
    r.n = 14; r.tag = 1;
    CHECK(r.x.ensure(300) == hipSuccess && r.y.ensure(40) == hipSuccess && parked[1].x.ensure(9) == hipSuccess, "setup");
    void* px = r.x.p; void* py = r.y.p; void* qx = parked[1].x.p;
    events.clear();
    std::swap(r, parked[1]);
    CHECK(r.n == 0 && r.tag == 0 && r.x.p == qx && !r.y.p && parked[1].n == 14 && parked[1].tag == 1 && parked[1].x.p == px && parked[1].y.p == py && events.empty(),
          "swap of two structs (events %s)", events.c_str());
    settled("structs swapped", r.x, r.y, parked[0].x, parked[0].y, parked[1].x, parked[1].y);
    std::swap(r, parked[0]);                  // with an empty one
    CHECK(!r.x.p && parked[0].x.p == qx && events.empty(), "swap with an empty struct");
    settled("struct swapped with empty", r.x, r.y, parked[0].x, parked[0].y, parked[1].x, parked[1].y);
    r = std::move(parked[1]);
    CHECK(r.x.p == px && r.y.p == py && r.n == 14 && !parked[1].x.p && !parked[1].y.p, "move assignment of a struct");
    settled("struct moved", r.x, r.y, parked[0].x, parked[0].y, parked[1].x, parked[1].y);
    events.clear();
  }
  CHECK(events == "FFF", "the structs' destructors free their three buffers: events %s", events.c_str());
  events.clear();
  done("structs", f0);
}

int main() {
  fits_and_grows();
  failure_paths();
  moves();
  structs();
  // at exit: the counter is back at zero and every pointer the fake handed out came back exactly once
  CHECK(g_mmDeviceBytes.load() == 0, "counter at exit %zu", g_mmDeviceBytes.load());
  CHECK(live.empty() && liveBytes == 0 && nAlloc == nFree && nStrayFree == 0, "at exit: %zu blocks outstanding, %zu allocations, %zu frees, %zu stray frees", live.size(), nAlloc, nFree, nStrayFree);
  CHECK(g_mmAllocNanos.load() > 0, "time inside ensure: %llu ns over %zu allocations", (unsigned long long)g_mmAllocNanos.load(), nAlloc);
  printf("cases %d\nmismatches %d\nallocations %zu frees %zu\n", cases, failures, nAlloc, nFree);
  return failures ? 1 : 0;
}
