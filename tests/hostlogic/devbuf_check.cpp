// tests/hostlogic/devbuf_check.cpp -- DevBuf (mashmap_amd/csrc/mm_devbuf.h) on the host: ownership, the growth policy of ensure() with
// each of its failure paths, and the live-byte counter behind mm_device_bytes; DevStream, DevEvent and PinnedBuf of the same header:
// created once, given back once.  hipMalloc / hipFree / hipGetLastError, the stream and event creation and destruction and
// hipHostMalloc / hipHostFree are defined HERE, as counting fakes over malloc / free that can be told which of the next allocations or
// creations fail; the HIP runtime is not linked.  Built with -fsanitize=address,undefined (a double free or a leak of the fake's memory
// ends the program) and run by tests/test_devbuf.py.
//
//   devbuf_check         prints "ok <case>" per case that passed, "FAIL ..." for a check that did not, then the summary lines
//                        "cases <n>", "mismatches <n>", "allocations <n> frees <n>", "streams <n> destroyed <n>", "events <n> destroyed <n>",
//                        "pinned <n> freed <n>"; the status is non-zero on any mismatch
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

// streams, events and page-locked blocks: one kind each, counted apart.  A handle is a byte of the fake's own memory, so that a handle
// that is never given back is a leak the sanitizer reports.  handleFailMask bit i: the i-th creation (of any kind) from now fails
struct Kind { std::map<void*, size_t> live; size_t made = 0, gone = 0, stray = 0; };
static Kind streams, evts, pinned;
static unsigned handleFailMask = 0, lastFlags = 0;
static size_t lastPinnedSize = 0;
static hipError_t make(Kind& k, void** out, size_t size, char ok, char bad) {   // events: ok on success, bad on a planned failure
  const bool fail = handleFailMask & 1u; handleFailMask >>= 1;
  if (fail) { events += bad; *out = (void*)0x1; return hipErrorOutOfMemory; }    // (a failed creation may leave rubbish behind: the owner must not keep it)
  void* q = malloc(size ? size : 1);
  if (!q) abort();
  k.live[q] = size; k.made++; events += ok;
  *out = q;
  return hipSuccess;
}
static hipError_t unmake(Kind& k, void* h, char ev) {
  events += ev;
  auto it = k.live.find(h);
  if (it == k.live.end()) { k.stray++; return hipErrorInvalidValue; }
  k.live.erase(it); k.gone++;
  free(h);
  return hipSuccess;
}
extern "C" hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { lastFlags = flags; return make(streams, (void**)s, 1, 'S', 'x'); }
extern "C" hipError_t hipStreamDestroy(hipStream_t s) { return unmake(streams, (void*)s, 's'); }
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { lastFlags = flags; return make(evts, (void**)e, 1, 'V', 'x'); }
extern "C" hipError_t hipEventDestroy(hipEvent_t e) { return unmake(evts, (void*)e, 'v'); }
extern "C" hipError_t hipHostMalloc(void** p, size_t size, unsigned flags) { lastFlags = flags; lastPinnedSize = size; return make(pinned, p, size, 'H', 'x'); }
extern "C" hipError_t hipHostFree(void* p) { return unmake(pinned, p, 'f'); }
static bool quiet(const Kind& k) { return k.live.empty() && k.made == k.gone && k.stray == 0; }

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

static_assert(!std::is_copy_constructible<DevStream>::value && !std::is_copy_assignable<DevStream>::value && !std::is_copy_constructible<DevEvent>::value &&
              !std::is_copy_assignable<DevEvent>::value && !std::is_copy_constructible<PinnedBuf>::value && !std::is_copy_assignable<PinnedBuf>::value, "the handles are not copyable");
static_assert(std::is_nothrow_move_constructible<DevStream>::value && std::is_nothrow_move_assignable<DevStream>::value && std::is_nothrow_move_constructible<DevEvent>::value &&
              std::is_nothrow_move_assignable<DevEvent>::value && std::is_nothrow_move_constructible<PinnedBuf>::value && std::is_nothrow_move_assignable<PinnedBuf>::value,
              "the handles move without throwing");

// ensure(), a failed creation, the moves and the destructor, the same for a stream and an event (H), whose fake is k
template <class H> static void handle_life(const char* what, Kind& k, char made, char gone) {
  const std::string M(1, made), G(1, gone);
  events.clear();
  {
    H a;
    CHECK(!a.h && events.empty(), "%s: a new handle is null and creates nothing", what);
    CHECK(a.ensure() == hipSuccess && a.h && k.live.count((void*)a.h) && events == M, "%s: first ensure (events %s)", what, events.c_str());
    auto raw = a.h;
    CHECK(a.ensure() == hipSuccess && a.h == raw && events == M, "%s: ensure twice creates once (events %s)", what, events.c_str());
    decltype(a.h) viaConversion = a;
    CHECK(viaConversion == raw, "%s: converts to the raw handle", what);
    events.clear();
    H f;
    handleFailMask = 1u;
    CHECK(f.ensure() == hipErrorOutOfMemory && !f.h && events == "x", "%s: a failed creation leaves the handle null and returns the error (events %s)", what, events.c_str());
    CHECK(f.ensure() == hipSuccess && f.h && events == "x" + M, "%s: ... and a later ensure succeeds (events %s)", what, events.c_str());
    events.clear();
    H b(std::move(a));                        // move construction
    CHECK(!a.h && b.h == raw && events.empty(), "%s: move construction (events %s)", what, events.c_str());
    auto old = f.h;
    f = std::move(b);                         // move assignment onto a live handle
    CHECK(!b.h && f.h == raw && !k.live.count((void*)old) && events == G, "%s: move assignment destroys what it replaces (events %s)", what, events.c_str());
    events.clear();
    H& self = f;
    f = std::move(self);                      // self-move
    CHECK(f.h == raw && k.live.count((void*)raw) && events.empty(), "%s: self-move (events %s)", what, events.c_str());
    CHECK(k.live.size() == 1, "%s: %zu handles live, one owner", what, k.live.size());
  }
  CHECK(events == G && quiet(k), "%s: the scope's end destroys the one live handle once (events %s, %zu made, %zu destroyed, %zu stray)", what, events.c_str(), k.made, k.gone, k.stray);
  events.clear();
}

struct Created { DevStream stream; DevEvent evA, evB; };   // what mm_create makes before it hands a context out

static void handles() {
  const int f0 = failures;
  handle_life<DevStream>("stream", streams, 'S', 's');
  CHECK(lastFlags == hipStreamNonBlocking, "a stream is non-blocking: flags %u", lastFlags);
  handle_life<DevEvent>("event", evts, 'V', 'v');
  {
    DevEvent timed, untimed;
    CHECK(timed.ensure() == hipSuccess && lastFlags == hipEventDefault, "an event's default flags: %u", lastFlags);
    CHECK(untimed.ensure(hipEventDisableTiming) == hipSuccess && lastFlags == hipEventDisableTiming, "an event's own flags: %u", lastFlags);
  }
  events.clear();
  {                                           // the second event's creation fails: the scope gives the stream and the first event back
    Created* c = new Created();
    handleFailMask = 4u;
    hipError_t e = hipSuccess;
    const bool ok = (e = c->stream.ensure()) == hipSuccess && (e = c->evA.ensure()) == hipSuccess && (e = c->evB.ensure()) == hipSuccess;
    CHECK(!ok && e == hipErrorOutOfMemory && c->stream.h && c->evA.h && !c->evB.h && events == "SVx", "events %s", events.c_str());
    delete c;
    CHECK(events == "SVxvs" && quiet(streams) && quiet(evts), "a context that failed half-made leaves nothing behind (events %s)", events.c_str());
  }
  events.clear();
  CHECK(handleFailMask == 0, "every planned failure was taken");
  done("handles", f0);
}

static void pinned_blocks() {
  const int f0 = failures;
  events.clear();
  {
    PinnedBuf b;
    CHECK(b.ensure(0) == hipSuccess && !b.p && events.empty(), "ensure(0) of an empty block allocates nothing");
    CHECK(b.ensure(1000) == hipSuccess && b.p && b.bytes == 1000 && lastPinnedSize == 1000 && lastFlags == hipHostMallocDefault && events == "H",
          "first ensure: exactly the size asked for (bytes %zu, events %s)", b.bytes, events.c_str());
    void* p0 = b.p; events.clear();
    CHECK(b.ensure(1) == hipSuccess && b.ensure(1000) == hipSuccess && b.p == p0 && b.bytes == 1000 && events.empty(), "a size that fits keeps the pointer (events %s)", events.c_str());
    CHECK(b.ensure(1001) == hipSuccess && b.bytes == 1001 && lastPinnedSize == 1001 && !pinned.live.count(p0) && pinned.live.count(b.p) && events == "fH",
          "growth is free-then-allocate at exactly the size (bytes %zu, events %s)", b.bytes, events.c_str());
    CHECK(b.as<char>() == (char*)b.p, "as<T>");
    events.clear(); handleFailMask = 1u;
    CHECK(b.ensure(5000) == hipErrorOutOfMemory && !b.p && b.bytes == 0 && events == "fxe" && pinned.live.empty(),
          "a failed growth leaves it empty with the sticky error cleared (p %p, bytes %zu, events %s)", b.p, b.bytes, events.c_str());
    events.clear(); handleFailMask = 1u;
    CHECK(b.ensure(5000) == hipErrorOutOfMemory && !b.p && b.bytes == 0 && events == "xe", "... and from empty (events %s)", events.c_str());
    CHECK(b.ensure(5000) == hipSuccess && b.bytes == 5000, "the block is usable again");
    void* p1 = b.p; events.clear();
    PinnedBuf c(std::move(b));                // the moves, as DevBuf's
    CHECK(!b.p && !b.bytes && c.p == p1 && c.bytes == 5000 && events.empty(), "move construction (events %s)", events.c_str());
    CHECK(b.ensure(64) == hipSuccess, "setup");
    void* p2 = b.p; events.clear();
    b = std::move(c);
    CHECK(!c.p && !c.bytes && b.p == p1 && !pinned.live.count(p2) && events == "f", "move assignment frees what it replaces (events %s)", events.c_str());
    events.clear();
    PinnedBuf& self = b;
    b = std::move(self);
    CHECK(b.p == p1 && b.bytes == 5000 && events.empty(), "self-move (events %s)", events.c_str());
    PinnedBuf turns[2];                       // an array of two, as the index build's landing areas
    CHECK(turns[0].ensure(10) == hipSuccess && turns[1].ensure(20) == hipSuccess && pinned.live.size() == 3, "setup");
    events.clear();
  }
  CHECK(events == "fff" && quiet(pinned), "every block is freed once (events %s, %zu allocated, %zu freed, %zu stray)", events.c_str(), pinned.made, pinned.gone, pinned.stray);
  events.clear();
  CHECK(handleFailMask == 0, "every planned failure was taken");
  done("pinned", f0);
}

int main() {
  fits_and_grows();
  failure_paths();
  moves();
  structs();
  handles();
  pinned_blocks();
  CHECK(quiet(streams) && quiet(evts) && quiet(pinned), "at exit: %zu streams, %zu events, %zu page-locked blocks outstanding", streams.live.size(), evts.live.size(), pinned.live.size());
  // at exit: the counter is back at zero and every pointer the fake handed out came back exactly once
  CHECK(g_mmDeviceBytes.load() == 0, "counter at exit %zu", g_mmDeviceBytes.load());
  CHECK(live.empty() && liveBytes == 0 && nAlloc == nFree && nStrayFree == 0, "at exit: %zu blocks outstanding, %zu allocations, %zu frees, %zu stray frees", live.size(), nAlloc, nFree, nStrayFree);
  CHECK(g_mmAllocNanos.load() > 0, "time inside ensure: %llu ns over %zu allocations", (unsigned long long)g_mmAllocNanos.load(), nAlloc);
  printf("cases %d\nmismatches %d\nallocations %zu frees %zu\n", cases, failures, nAlloc, nFree);
  printf("streams %zu destroyed %zu\nevents %zu destroyed %zu\npinned %zu freed %zu\n", streams.made, streams.gone, evts.made, evts.gone, pinned.made, pinned.gone);
  return failures ? 1 : 0;
}
