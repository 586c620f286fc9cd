// mashmap_amd/csrc/mm_l1_core.h -- computeL1CandidateRegions over ONE fragment's sorted interval points, literally, in integers.
//
//   Map::doL1Mapping                 one call per reference group (skip_prefix)      src/map/include/computeMap.hpp:1130-1166
//   Map::computeL1CandidateRegions   windowLen, hash_to_freq, the trailing test      src/map/include/computeMap.hpp:916-954
//                                    pass 1: the best overlap count                  :948-983
//                                    the HG cut-off raises minimumHits               :984-998      mm_hg_min_hits
//                                    pass 2: runs of positions >= minimumHits        :1001-1098    mm_l1_literal_fragment
//                                    runs closer than segLength are joined           :1102-1115    L1Emit
//
// Shared by the one-thread-per-fragment kernels (k_l1_sweep: windowLen == 0; k_l1_window: --noSplit, windowLen != 0; mm_map.hip),
// which every faster L1 path is compared against, and by the CPU check (tests/hostlogic/l1_check.cpp), which runs it beside the
// oracle under a host sanitizer.  A point is the packed key  seqId << 33 | pos << 1 | OPEN  (ascending == (seqId, pos, CLOSE first)).
// Compiles for the host (g++) and for the device (hipcc).
#pragma once
#include "mm_heap.h"
#include "../../include/mashmap_hip.h"

// computeMap.hpp:984-998: a group whose best overlap count misses minHits yields nothing (false); otherwise minHits is raised to the
// cut-off of that count (Map::sketchCutoffs, one entry per sParam / 1000 counts).
MM_HD bool mm_hg_min_hits(int best, int sketchSizeQ, int& minHits, const int32_t* cutoffs, int nCutoffs, int sParam) {
  if (best < minHits) return false;
  const double div = (double)sParam / 1000.0 > 1.0 ? (double)sParam / 1000.0 : 1.0;
  int ci = (int)((double)(best < sketchSizeQ ? best : sketchSizeQ) / div);
  if (ci >= nCutoffs) ci = nCutoffs - 1;
  const int cut = cutoffs[ci];
  minHits = cut > minHits ? cut : minHits;
  return true;
}

struct L1Emit {
  mm_l1_candidate* out; int frag; int count; bool write;
  bool have; mm_l1_candidate pend;
  MM_HD void run(int seqId, int start, int end, int isize, int clusterLen, bool& firstOfGroup) {
    // join with the previous candidate of the same computeL1CandidateRegions call when close (computeMap.hpp:1102-1115)
    if (have && !firstOfGroup && seqId == pend.seqId && !(start > pend.rangeEndPos + clusterLen)) {
      pend.rangeEndPos = end; pend.intersectionSize = isize > pend.intersectionSize ? isize : pend.intersectionSize;
    } else {
      flush();
      pend.frag = frag; pend.seqId = seqId; pend.rangeStartPos = start; pend.rangeEndPos = end; pend.intersectionSize = isize; have = true;
    }
    firstOfGroup = false;
  }
  mm_l1_candidate b0, b1;                             // the first two candidates of a counting pass: most fragments need no second pass
  MM_HD void flush() {
    if (have) {
      if (write) out[count] = pend;
      else if (count == 0) b0 = pend;
      else if (count == 1) b1 = pend;
      count++; have = false;
    }
  }
};

// What the sweep of one fragment reads.  ids, W, freq, nFreq exist for windowLen != 0 only (WINDOWED): ids numbers the seeds of the
// fragment's points, freq is nFreq counters of open windows per seed (hash_to_freq, :948) -- a seed adds to the overlap only while its
// count goes 0 -> 1 and leaves it only when it returns to 0.
struct L1Frag {
  const uint64_t* p; int nPts;                        // the points, sorted
  const uint16_t* ids; int W; int32_t* freq; int nFreq;
  int sketchSizeQ, minHits;                           // Q.sketchSize and its minimumHits
  const int32_t* cutoffs; int nCutoffs, sParam, segLength, hg, skipPrefix;
  const int32_t* refGroup;
};

// WINDOWED == false states windowLen == 0: key >> 1 == (seqId << 32 | pos), so "trail <= lead in (seqId, pos)" is one 64-bit compare.
// WINDOWED == true keeps the trailing pointer W behind the leading one and handles W == 0 as well (a batch may mix short and long
// reads).  Either way the leading pointer groups points by `pos` ALONE (:967, :1047-1051), across a contig boundary too.
// Emits the joined candidates of each reference group in the reference's order.
template <bool WINDOWED>
MM_HD void mm_l1_literal_fragment(const L1Frag& q, L1Emit& em) {
  const uint64_t* p = q.p;
  const int W = WINDOWED ? q.W : 0;
  auto seqOf = [&](int i) { return (int)(p[i] >> 33); };
  auto posOf = [&](int i) { return (int)(uint32_t)(p[i] >> 1); };
  auto clearFreq = [&]() { if constexpr (WINDOWED) for (int i = 0; i < q.nFreq; i++) q.freq[i] = 0; };
  // what differs with a window: the trailing pointer stays W behind (:952-954), and a seed's CLOSE / OPEN counts only when it is
  // the seed's last open window that leaves / its first that enters
  auto behind = [&](int t, int l) {
    if constexpr (WINDOWED) { const int st = seqOf(t), sl = seqOf(l); return (st == sl && posOf(t) <= posOf(l) - W) || st < sl; }
    else return (p[t] >> 1) <= (p[l] >> 1);
  };
  auto leaves = [&](int t) { if constexpr (WINDOWED) { if (W != 0) return --q.freq[q.ids[t]] == 0; } return true; };
  auto enters = [&](int l) { if constexpr (WINDOWED) { if (W != 0) return q.freq[q.ids[l]]++ == 0; } return true; };
  // one step of either pass: the trailing pointer retires what lies behind the leading one (:950-965), which then takes in the
  // position group `cur` (:967-981)
  auto advance = [&](int& trail, int& lead, int e, int cur, int& overlap) {
    while (trail < e && behind(trail, lead)) { if (!(p[trail] & 1ull) && leaves(trail)) overlap--; trail++; }
    while (lead < e && posOf(lead) == cur) { if ((p[lead] & 1ull) && enters(lead)) overlap++; lead++; }
  };
  int b = 0;
  while (b < q.nPts) {
    int e = q.nPts;
    if (q.skipPrefix) {
      const int g = q.refGroup[seqOf(b)];
      e = b; while (e < q.nPts && q.refGroup[seqOf(e)] == g) e++;
    }
    int minHits = q.minHits;
    bool go = true;
    if (q.hg) {                                                  // pass 1: best overlap (:948-999)
      clearFreq();
      int overlap = 0, best = 0, trail = b, lead = b;
      while (lead < e) {
        advance(trail, lead, e, posOf(lead), overlap);
        best = overlap > best ? overlap : best;
      }
      go = mm_hg_min_hits(best, q.sketchSizeQ, minHits, q.cutoffs, q.nCutoffs, q.sParam);
    }
    if (go) {                                                    // pass 2: runs (:1001-1098); hash_to_freq.clear() first (:1001-1003)
      clearFreq();
      bool firstOfGroup = true, inRun = false;
      int rSeq = 0, rStart = 0, rEnd = 0, rSize = 0;
      int overlap = 0, trail = b, lead = b;
      int prevSeq = 0, prevPos = 0;
      int curSeq = seqOf(b), curPos = posOf(b);
      while (lead < e) {
        const int prevOverlap = overlap;
        if (posOf(lead) != curPos) { prevSeq = curSeq; prevPos = curPos; curSeq = seqOf(lead); curPos = posOf(lead); }
        advance(trail, lead, e, curPos, overlap);
        if (prevOverlap >= minHits) {
          if (inRun && rSeq != prevSeq) { em.run(rSeq, rStart, rEnd, rSize, q.segLength, firstOfGroup); inRun = false; }
          if (!inRun) { rStart = prevPos - W; rEnd = prevPos - W; rSeq = prevSeq; rSize = prevOverlap; inRun = true; }
          else { rSize = prevOverlap > rSize ? prevOverlap : rSize; rEnd = prevPos - W; }
        } else {
          if (inRun) em.run(rSeq, rStart, rEnd, rSize, q.segLength, firstOfGroup);
          inRun = false;
        }
      }
      if (inRun) em.run(rSeq, rStart, rEnd, rSize, q.segLength, firstOfGroup);
    }
    em.flush();
    b = e;
  }
}

// One fragment from points to stored candidates: a counting pass, then claim(nOut, base) reserves nOut slots of l1 -- false: they did
// not fit, and the fragment reports none --, then the candidates go to l1[base ..): the (at most two) the counting pass kept, or a
// second, writing pass.
struct L1Stored { int nOut; long long base; };
template <bool WINDOWED, class Claim>
MM_HD L1Stored mm_l1_literal_store(const L1Frag& q, int frag, mm_l1_candidate* l1, Claim claim) {
  L1Stored r{0, 0};
  L1Emit em; em.out = nullptr; em.frag = frag; em.count = 0; em.write = false; em.have = false;
  mm_l1_literal_fragment<WINDOWED>(q, em);
  r.nOut = em.count;
  if (r.nOut > 0) {
    if (!claim(r.nOut, r.base)) r.nOut = 0;
    else if (r.nOut <= 2) { l1[r.base] = em.b0; if (r.nOut == 2) l1[r.base + 1] = em.b1; }
    else {
      L1Emit ew; ew.out = l1 + r.base; ew.frag = frag; ew.count = 0; ew.write = true; ew.have = false;
      mm_l1_literal_fragment<WINDOWED>(q, ew);
    }
  }
  return r;
}
