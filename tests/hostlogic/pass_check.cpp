// tests/hostlogic/pass_check.cpp -- TEST HARNESS for mashmap_amd/host/pass_plan.hpp (no GPU): a producer thread and a consumer thread around
// a BatchChannel, the consumer taking device passes greedily as skch::Map does (getGroup: what is queued, at most maxGroup items), under
// randomised timing.  Prints one line per scenario:
//   "ok <scenario> items <n> passes <p> sizes <s1,s2,...>"   or   "FAIL ..." (and exits 1)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include "../../mashmap_amd/host/pass_plan.hpp"

struct Item { size_t id; };

// queuedFirst: the whole input is queued (and the producer done) before the consumer takes its first pass
static int scenario(const char* name, size_t items, size_t maxGroup, size_t cap, int producerUs, int consumerUs, unsigned seed, bool queuedFirst = false) {
  mmhost::BatchChannel<Item> ch(cap);
  std::thread prod([&] {
    std::mt19937 r2(seed * 7 + 1);
    for (size_t i = 0; i < items; i++) {
      if (producerUs) std::this_thread::sleep_for(std::chrono::microseconds(r2() % (2 * producerUs + 1)));
      ch.waitSpace();
      ch.put(Item{i});
    }
    ch.close();
  });
  if (queuedFirst) prod.join();
  std::vector<Item> g; std::vector<size_t> passSizes;
  size_t next = 0; bool bad = false; std::string why;
  std::mt19937 r3(seed * 13 + 5);
  while (true) {
    g.clear();
    if (!ch.getGroup(g, maxGroup)) break;
    if (g.empty() || g.size() > maxGroup) { bad = true; why = "group size"; break; }
    for (const auto& it : g) if (it.id != next++) { bad = true; why = "order"; }
    if (bad) break;
    passSizes.push_back(g.size());
    if (consumerUs) std::this_thread::sleep_for(std::chrono::microseconds(r3() % (2 * consumerUs * g.size() + 1)));
  }
  if (!queuedFirst) prod.join();
  if (!bad && next != items) { bad = true; why = "items lost"; }
  printf("%s %s items %zu passes %zu sizes", bad ? "FAIL" : "ok", name, items, passSizes.size());
  for (size_t i = 0; i < passSizes.size(); i++) printf("%c%zu", i ? ',' : ' ', passSizes[i]);
  if (bad) printf(" (%s)", why.c_str());
  printf("\n");
  return bad ? 1 : 0;
}

int main() {
  int rc = 0;
  // a fast producer (the device is the bottleneck): passes of several batches, never more than maxGroup
  rc |= scenario("fast-producer", 20, 4, 4, 0, 300, 1);
  // a slow producer (the reader is the bottleneck): passes of what is there, nothing is lost, nothing deadlocks
  rc |= scenario("slow-producer", 23, 4, 4, 400, 50, 3);
  // one batch per pass (several contexts, ASCII uploads, MASHMAP_HIP_COALESCE_MBP=0)
  rc |= scenario("no-coalescing", 9, 1, 2, 100, 100, 4);
  // tiny batches, many per pass (the small-batch PAF tests: MASHMAP_HIP_BATCH_MBP=0.05)
  rc |= scenario("tiny-batches", 300, 64, 64, 20, 20, 5);
  rc |= scenario("single-item", 1, 4, 4, 0, 0, 6);
  rc |= scenario("queue-smaller-than-pass", 40, 8, 3, 10, 10, 7);
  // everything queued before the first pass: maxGroup-sized passes, then the remainder
  rc |= scenario("queued-first", 10, 4, 10, 0, 0, 8, true);
  for (unsigned s = 10; s < 30; s++) rc |= scenario("random-timing", 37, 4, 4, (s * 37) % 200, (s * 53) % 200, s);
  return rc;
}
