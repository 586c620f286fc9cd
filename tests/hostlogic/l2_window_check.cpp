// tests/hostlogic/l2_window_check.cpp -- mm_l2_window_core.h (the windowLen != 0 L2 stage of k_l2_window_wave) on the host, over a file of
// cases that tests/test_l2_window_core.py writes and whose loci it compares with the oracle's computeL2MappedRegions.  Built with
// -fsanitize=address,undefined: cells, heap and locus slots have exactly the sizes the case states, so an index out of range ends the
// program with a non-zero status.
//
//   l2_window_check <cases> <out>
//
// cases, 64-bit words:  nCases, then per case
//                       S segLength W heapCap locap nRec nCand   hash[S] strand[S]   nRec x (hash wpos wpos_end seqId strand)   nCand x (seqId rangeStart rangeEnd)
//                       (records: the whole index, in index order)
// out, 32-bit words per candidate:  done (0: the heap outgrew heapCap)  overflow (more loci than locap + 1)  walked entering skipped re-entered
//                                   largestHeap  n, then n x (optimalStart optimalEnd sharedSketchSize strand)
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>
#include "../../mashmap_amd/csrc/mm_l2_window_core.h"

static std::vector<int64_t> readWords(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
  std::vector<int64_t> w((size_t)n / 8);
  if (fread(w.data(), 8, w.size(), f) != w.size()) { fprintf(stderr, "short read\n"); exit(2); }
  fclose(f);
  return w;
}

struct HostPresence {
  std::unordered_map<uint64_t, int> m;
  bool find(uint64_t h, int& end) const { const auto it = m.find(h); if (it == m.end()) return false; end = it->second; return true; }
  void set(uint64_t h, int end) { m[h] = end; }
};

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: l2_window_check <cases> <out>\n"); return 2; }
  const std::vector<int64_t> w = readWords(argv[1]);
  size_t at = 0;
  auto next = [&]() { if (at >= w.size()) { fprintf(stderr, "cases file ends early\n"); exit(2); } return w[at++]; };
  const int nCases = (int)next();
  std::vector<int32_t> out;
  for (int ci = 0; ci < nCases; ci++) {
    const int S = (int)next(), segLength = (int)next(), W = (int)next(), heapCap = (int)next(), locap = (int)next();
    const long long nRec = next(); const int nCand = (int)next();
    std::vector<uint64_t> q(S); std::vector<int8_t> qs(S);
    for (auto& h : q) h = (uint64_t)next();
    for (auto& s : qs) s = (int8_t)next();
    std::vector<WinRecord> rec((size_t)nRec); std::vector<int32_t> seq((size_t)nRec);
    for (long long i = 0; i < nRec; i++) {
      rec[i].hash = (uint64_t)next(); rec[i].wpos = (int32_t)next(); rec[i].wend = (int32_t)next(); seq[i] = (int32_t)next(); rec[i].rev = next() < 0;
    }
    for (int k = 0; k < nCand; k++) {
      const int seqId = (int)next(), rangeStart = (int)next(), rangeEnd = (int)next();
      // std::lower_bound(minmerIndex, (seqId, rangeStart - segLength - 1))  (computeMap.hpp:1290-1293), then to the contig's end
      const long long target = (long long)rangeStart - segLength - 1;
      long long b = 0;
      while (b < nRec && (seq[b] < seqId || (seq[b] == seqId && rec[b].wpos < target))) b++;
      long long e = b;
      while (e < nRec && seq[e] == seqId) e++;
      const std::vector<WinRecord> mine(rec.begin() + b, rec.begin() + e);      // a copy of exactly that size: reading past it is an error
      std::vector<WinCell> cells((size_t)S + 1); std::vector<uint64_t> heap((size_t)heapCap); std::vector<WinLocus> slots((size_t)locap);
      HostPresence present; WinRuns rn; long long counts[5] = {0, 0, 0, 0, 0};
      const bool done = mm_win_candidate(mine.data(), (long long)mine.size(), q.data(), qs.data(), S, rangeStart, rangeEnd, segLength, W, cells.data(), heap.data(),
                                         heapCap, present, rn, slots.data(), locap, counts);
      out.push_back(done); out.push_back(done && rn.overflow);
      for (long long v : counts) out.push_back((int32_t)v);
      const int n = done && !rn.overflow ? rn.total() : 0;
      out.push_back(n);
      for (int i = 0; i < n; i++) { const WinLocus l = rn.locus(i); out.push_back(l.start); out.push_back(l.end); out.push_back(l.shared); out.push_back(l.strand); }
    }
  }
  if (at != w.size()) { fprintf(stderr, "cases file has %zu words left over\n", w.size() - at); return 2; }
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) { perror(argv[2]); return 2; }
  return 0;
}
