// mashmap_amd/host/pass_plan.hpp -- how skch::Map groups the reader's batches into device passes: the hand-over queue between two stages
// of its pipeline, from which a pass takes what is queued.  Kept apart from skch_map.hpp so that it can be exercised without a GPU
// (tests/hostlogic/pass_check.cpp).
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <mutex>
#include <utility>
#include <vector>

namespace mmhost {

// Hand-over between two stages: at most `cap` items waiting.
template <class T>
class BatchChannel {
  std::deque<T> q; std::mutex mu; std::condition_variable cvFull, cvEmpty; bool done = false; size_t cap;

 public:
  explicit BatchChannel(size_t c) : cap(c) {}
  void put(T&& b) { std::unique_lock<std::mutex> lk(mu); cvFull.wait(lk, [&] { return q.size() < cap; }); q.emplace_back(std::move(b)); lk.unlock(); cvEmpty.notify_one(); }
  // blocks until there is room; with a single producer the put() that follows does not wait
  void waitSpace() { std::unique_lock<std::mutex> lk(mu); cvFull.wait(lk, [&] { return q.size() < cap; }); }
  bool get(T& b) {
    std::unique_lock<std::mutex> lk(mu);
    cvEmpty.wait(lk, [&] { return !q.empty() || done; });
    if (q.empty()) return false;
    b = std::move(q.front()); q.pop_front();
    lk.unlock(); cvFull.notify_one();
    return true;
  }
  void close() { { std::lock_guard<std::mutex> lk(mu); done = true; } cvEmpty.notify_all(); }
  // The items of one device pass, greedily: waits until something is queued or the producer is done, then takes everything that is
  // queued, at most `maxItems` -- a pass never waits for input that is not there yet and never leaves input behind that is.  false: the
  // producer is done and nothing is left.
  bool getGroup(std::vector<T>& g, size_t maxItems) {
    std::unique_lock<std::mutex> lk(mu);
    cvEmpty.wait(lk, [&] { return !q.empty() || done; });
    if (q.empty()) return false;
    while (!q.empty() && g.size() < maxItems) { g.emplace_back(std::move(q.front())); q.pop_front(); }
    lk.unlock(); cvFull.notify_all();
    return true;
  }
  // every queued item in order (only the consumer removes items: what fn sees stays put until the consumer's next get)
  template <class F> void forEach(F fn) { std::lock_guard<std::mutex> lk(mu); for (auto& b : q) fn(b); }
};

}  // namespace mmhost
