// tests/hostlogic/l1_check.cpp -- mm_l1_core.h (the literal L1 of k_l1_sweep / k_l1_window) on the host, over a file of cases that
// tests/test_l1_literal_core.py writes and whose results it compares with the oracle's computeL1CandidateRegions.  Built with
// -fsanitize=address,undefined: every array has exactly the size its case states (points, ids, the nFreq counters, the nOut claimed
// candidates at the end of a buffer of cap), so an index out of range ends the program with a non-zero status.
//
//   l1_check <windowed: 0|1> <cases> <out>
//
// cases, 64-bit words:  nCases cap sParam nCutoffs cutoffs[nCutoffs]
//                       then per case  nPts W nFreq sketchSizeQ minHits segLength hg skipPrefix nRef refGroup[nRef] key[nPts] id[nPts]
// out, 32-bit words per case:  n, then n x (seqId, rangeStartPos, rangeEndPos, intersectionSize); n == -1: more than cap candidates
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../mashmap_amd/csrc/mm_l1_core.h"

static std::vector<int64_t> readWords(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
  std::vector<int64_t> w((size_t)n / 8);
  if (fread(w.data(), 8, w.size(), f) != w.size()) { fprintf(stderr, "short read\n"); exit(2); }
  fclose(f);
  return w;
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: l1_check <windowed: 0|1> <cases> <out>\n"); return 2; }
  const bool windowed = atoi(argv[1]) != 0;
  const std::vector<int64_t> w = readWords(argv[2]);
  size_t at = 0;
  auto next = [&]() { if (at >= w.size()) { fprintf(stderr, "cases file ends early\n"); exit(2); } return w[at++]; };
  const int nCases = (int)next(); const int64_t cap = next(); const int sParam = (int)next(); const int nCutoffs = (int)next();
  std::vector<int32_t> cutoffs(nCutoffs);
  for (auto& c : cutoffs) c = (int32_t)next();
  std::vector<int32_t> out;
  for (int ci = 0; ci < nCases; ci++) {
    L1Frag q{};
    q.nPts = (int)next(); q.W = (int)next(); q.nFreq = (int)next(); q.sketchSizeQ = (int)next(); q.minHits = (int)next();
    q.segLength = (int)next(); q.hg = (int)next(); q.skipPrefix = (int)next();
    const int nRef = (int)next();
    std::vector<int32_t> refGroup(nRef);
    for (auto& g : refGroup) g = (int32_t)next();
    std::vector<uint64_t> p(q.nPts); std::vector<uint16_t> ids(q.nPts); std::vector<int32_t> freq(q.nFreq, -1);
    for (auto& k : p) k = (uint64_t)next();
    for (auto& i : ids) i = (uint16_t)next();
    q.p = p.data(); q.cutoffs = cutoffs.data(); q.nCutoffs = nCutoffs; q.sParam = sParam; q.refGroup = refGroup.data();
    if (windowed) { q.ids = ids.data(); q.freq = freq.data(); }   // the split form must not look at them

    // the device's cursor and capacity: cap slots, claimed from the END of the buffer so that one candidate too many is out of bounds
    std::vector<mm_l1_candidate> l1((size_t)cap);
    bool fit = true;
    auto claim = [&](int nOut, long long& base) { base = cap - nOut; return fit = nOut <= cap; };
    const L1Stored r = windowed ? mm_l1_literal_store<true>(q, ci, l1.data(), claim) : mm_l1_literal_store<false>(q, ci, l1.data(), claim);
    out.push_back(fit ? r.nOut : -1);
    for (int i = 0; i < r.nOut; i++) {
      const mm_l1_candidate& c = l1[(size_t)r.base + i];
      if (c.frag != ci) { fprintf(stderr, "case %d: candidate %d belongs to fragment %d\n", ci, i, c.frag); return 3; }
      out.push_back(c.seqId); out.push_back(c.rangeStartPos); out.push_back(c.rangeEndPos); out.push_back(c.intersectionSize);
    }
  }
  if (at != w.size()) { fprintf(stderr, "cases file has %zu words left over\n", w.size() - at); return 2; }
  FILE* f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) { perror(argv[3]); return 2; }
  return 0;
}
