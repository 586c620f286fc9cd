// mashmap_amd/csrc/mm_chain_core.h -- the tail of Map::mapModule for ONE read, from its candidate mappings, literally.
//
//   Map::mapSingleQueryFrag    kmerComplexity gate, sort by (refSeqId, refStartPos)     src/map/include/computeMap.hpp:799-800, :830-831, :1137
//   Map::mapModule             coordinates of a split read                              :632-636
//   Map::mergeMappingsInRange  sort, pair loop, union-find, extents, the two averages   :1580-1702   (src/common/dset64.hpp:93-125)
//   Map::filterWeakMappings                                                             :423-432
//   Map::filterByGroup         both sorts, the runs of one reference group under -Y,    :504-561, src/map/include/filter.hpp:36-160
//                              the query-axis plane sweep of every run
//
// i.e. MapPost::finishRead (mashmap_amd/host/skch_map_post.hpp) up to and including filterByGroup, on the integers of mm_mapping.
// Shared by the kernels (k_chain_reads, k_chain_reads_long, mm_chain.hip) and by the CPU checks (tests/hostlogic/chain_check.cpp,
// chain_long_check.cpp), which run it beside MapPost on generated reads and compare every field bit for bit.  Compiles for the host (g++)
// and for the device (hipcc).
//
// Two entry points over one body (mm_chain_read_t, a template over the working set): mm_chain_read takes a read of at most
// MM_CHAIN_MAX_RECORDS (16) records with its working set on the stack and 8-bit ids; mm_chain_read_long takes one of at most
// MM_CHAIN_LONG_MAX_RECORDS (512) with a working set the caller provides (the kernel's is in LDS) and 16-bit ids.  The body is made of the
// steps the wave-per-read kernel calls one by one: mm_chain_prepare (one record), mm_chain_partner (the best partner of member i),
// mm_chain_unite, mm_chain_finish_chain, mm_chain_keep, mm_chain_filter -- itself the sort by the reference key, mm_chain_run_end and
// mm_chain_filter_run (with mm_chain_sweep) for every run, mm_chain_filter_compact --, mm_chain_emit (one row).
//
// Why the result is the host's, bit for bit:
//   sorts     All five order-sensitive sorts of the tail -- per fragment, before the pair loop, by splitMappingId, the two of
//             filterByGroup -- go through mm_std_sort (mm_stdsort.h): libstdc++'s std::sort restated comparison for comparison and move
//             for move, from the same input order with the same key.  Up to 16 elements that is __insertion_sort alone, which is stable;
//             beyond it is introsort, whose order among equal keys is neither the input's nor any stable sort's, and it decides the chain's
//             representative: every member of a chain ties in the sort by splitMappingId, and the first of them afterwards gives
//             conservedSketches, sketchSize and approxMatches of the PAF line.  tests/hostlogic/stdsort_check.cpp compares the restated
//             sort with std::sort call for call.  The 2n events of the sweep and the (dist + score, id) pairs are totally ordered tuples:
//             any sort does (the events are heap-sorted, the pair's minimum is taken in passing).
//   status    The sweep's std::set finds two mappings equivalent when identity, queryStartPos and refSeqId agree: insert is then a
//             no-op and erase(id) removes whichever element is equivalent.  A sorted array of at most m ids (m <= 512) with the same two
//             rules.
//   identity  a function of (sketchSize, conservedSketches): the host's own floats arrive as a table.
//   chaining  chainGap <= 1 << 25 (mm_chain_params_ok).  A pair that passes dist < max_dist has |query_dist|, |ref_dist| < 2^25, their
//             squares and the sum are integers below 2^53, (query_dist - ref_dist)^2 one below 2^52: exact in a double, with or without
//             a contracted multiply-add.  Only sqrt and dist + score round, both correctly (IEEE; the library is not built with
//             fast-math).  For a pair that fails the test nothing computed is used.
//   averages  accumulated in double from 0.0 in member order, as std::accumulate does.  The identity's sum is double + float on the host
//             too.  The complexity's is not: the host's lambda adds the long double member kmerComplexity in 80 bits and rounds the sum
//             to double at every step, this function adds in double.  The two agree whenever the 80-bit sum is exact, for then the host
//             rounds once, to double, as this function does.  ASSUMPTION, not enforced: the complexities of one chain's members lie
//             within a factor 2^24 of each other.  They are floats (24 bits), at most 2^9 of them, so every exact partial sum spans at
//             most 24 + 24 + 9 + 1 = 58 bits, at most the 64 of the 80-bit format: the host's additions are exact, its conversion to
//             double is the one rounding of the step -- and the double the next step starts from is the same on both sides, by
//             induction from 0.0.  (With at most 16 members the span is 24 + 24 + 4 = 52 bits and nothing rounds before the division.)
//             Beyond the factor a sum rounds once here and twice on the host, and the two can differ in the last bit.  Complexity is
//             rawSketchSize / (maxHash / 2^64) / (2 (len - k + 1)): a factor 2^24 between two fragments of a read needs a bottom-s sketch
//             whose LARGEST hash lies below 2^40 -- s hashes out of 2^64 all that small -- which no sequence a sketch is taken of yields.
//             tests/hostlogic/chain_check.cpp draws maxHash over the whole assumed range (2^40 .. 2^64).
//   kmerComplexity  (double)((long double)maxHash / UINT64_MAX) without an 80-bit type: mm_chain_hash01.
//   runs      Under -Y (mm_chain_env::refGroup set) filterByGroup filters reference group by reference group.  Behind its sort by
//             (refSeqId, refStartPos) it walks RUNS: a run is a maximal stretch of consecutive members of that sorted order with equal
//             refGroup[refSeqId] -- std::find_if_not from the run's first member (:524) --, so a group whose contigs are not consecutive
//             in a refGroup array that is not non-decreasing (the C ABI takes one) forms two runs, here as there.  The host copies a
//             run into a vector of its own, sorts the copy by the query key and sweeps it; here the run v[b, e) is sorted in place: the
//             same elements in the same input order under the same comparator, so mm_std_sort makes the same moves.  The sweep's ids
//             are absolute positions in v (b .. e - 1, below 512: the event word's 10 bits) where the host's count from 0 inside the
//             copy: a constant offset, the same order of events and of the status set.  A run's events are ev[2b, 2e), its status set
//             status[b, e), and it writes `discard` of its own members only: two runs touch disjoint scratch and disjoint members, in
//             whatever order they are swept.  A run of one member is kept untouched
//             (filterQueryAxis returns at size <= 1).  The survivors are appended run by run, i.e. compacted in order, and the final
//             sort by the query key sees them in the order the host's `filtered` vector has.  secondaryToKeep is the same for every
//             run.  Without refGroup the single run is [0, m): the code of before.
//   noSplit   mm_chain_env::noSplit (MM_FLAG_NO_SPLIT): split_mapping is false for every read (:587), so a read longer than a segment
//             keeps its fragment's coordinates (0 .. fragLen), is not merged, and queryLen is its one fragment's length.
#pragma once
#include <math.h>
#include "mm_heap.h"
#include "mm_stdsort.h"
#include "../../include/mashmap_hip.h"

// what the function needs beside the caller's parameter block
struct mm_chain_env {
  mm_chain_params p;
  int32_t kmerSize, segLength, stride;       // stride of `identity` (sketchSize + 1)
  const float* identity;                     // identity[Qs * stride + shared]
  const int32_t* refGroup = nullptr;         // -Y (param.skip_prefix): refIdGroup[refSeqId], nContigs entries; nullptr: no groups, one run
  int32_t nContigs = 0;
  int32_t noSplit = 0;                       // --noSplit (!param.split): no read is split
};

// secondaryShort / secondarySegment are numMappingsFor... - 1 of an unsigned count: -1 (a count of 0) is what the reference and MapPost
// turn into 65535 by their cast to uint16_t (filterByGroup: filterQueryAxis(tmp, (uint16_t)n_mappings)), and so does mm_chain_read;
// anything below -1 is no count at all
MM_HD bool mm_chain_params_ok(const mm_chain_params& p) {
  return p.chainGap >= 0 && p.chainGap <= MM_CHAIN_MAX_GAP && (p.filter == MM_CHAIN_FILTER_NONE || p.filter == MM_CHAIN_FILTER_QUERY) &&
         p.secondaryShort >= -1 && p.secondarySegment >= -1 && p.minMerged >= 0;
}
#define MM_CHAIN_BAD_RECORD (-2)             // mm_chain_read: a record outside the identity table or, with refGroup, the contigs (an error, not a hand-over)

// (double)((long double)maxHash / UINT64_MAX), getSeedHits' max_hash_01 (:830), in integers.  With D = 2^64 - 1 and m' = maxHash << clz
// in [2^63, 2^64): m' * 2^64 = m' * D + m', so the quotient's 64-bit mantissa is m' with remainder m' -- more than D / 2, never a tie (D
// is odd) --: the x87 division rounds it up to m' + 1.  (maxHash == D is the quotient 1.)  Then 64 -> 53 bits, to nearest even.
MM_HD double mm_chain_hash01(uint64_t maxHash) {
  if (maxHash == 0) return 0.0;
  if (maxHash == ~0ull) return 1.0;
  int s = 0;
  while (!((maxHash << s) >> 63)) s++;
  const uint64_t M = (maxHash << s) + 1;     // m' <= 2^64 - 2 here (m' == 2^64 - 1 only for maxHash == D): no wrap
  uint64_t M53 = M >> 11;
  const uint64_t rem = M & 0x7FFull;
  if (rem > 0x400ull || (rem == 0x400ull && (M53 & 1))) M53++;
  return ldexp((double)M53, 11 - 64 - s);    // M53 <= 2^53: exact
}

// getSeedHits (:830-831): the ratio above -> double -> float
MM_HD float mm_chain_kmer_complexity(uint64_t maxHash, int rawSketchSize, int Qlen, int k) {
  const double max_hash_01 = mm_chain_hash01(maxHash);
  return (float)(((double)rawSketchSize / max_hash_01) / (double)((Qlen - k + 1) * 2));
}

MM_HD double mm_chain_sqrt(double x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dsqrt_rn(x);
#else
  return sqrt(x);
#endif
}

// One read's working set: the MappingResult fields the tail reads and writes, per record, the order v, and the scratch of the two
// phases that need any -- the union-find and the partners of mergeMappingsInRange, then the events and the status set of the sweep,
// which share their bytes.  CAP 16 with int8_t ids: 1.2 KB; CAP 512 with int16_t ids: 78 bytes a record, 39 KB.
template <int CAP_, class ID_>
struct mm_chain_work_t {
  enum : int { CAP = CAP_ };
  typedef ID_ ID;
  int32_t qs[CAP_], qe[CAP_], rs[CAP_], re[CAP_];
  int32_t sid[CAP_], cons[CAP_], sk[CAP_], blk[CAP_], approx[CAP_];
  int32_t nm[CAP_], smid[CAP_];
  float ident[CAP_];
  double kc[CAP_];
  int8_t strand[CAP_], discard[CAP_];
  ID_ v[CAP_];
  union {
    struct { ID_ parent[CAP_], best[CAP_]; int8_t rnk[CAP_]; } uf;         // rank <= lg CAP
    struct { uint64_t ev[2 * CAP_]; ID_ status[CAP_]; } sw;
  };
};
typedef mm_chain_work_t<MM_CHAIN_MAX_RECORDS, int8_t> mm_chain_work;
typedef mm_chain_work_t<MM_CHAIN_LONG_MAX_RECORDS, int16_t> mm_chain_work_long;

// res.approxMatches = std::round(res.nucIdentity * res.blockLength / 100.0): a float product, a double quotient (:1247, :1661)
MM_HD int32_t mm_chain_approx(float ident, int32_t blk) { return (int32_t)round((double)(ident * (float)blk) / 100.0); }

// the three keys the tail sorts by, as less(x, y) over ids
template <class W> MM_HD bool mm_chain_less_ref(const W& w, int x, int y) { return w.sid[x] != w.sid[y] ? w.sid[x] < w.sid[y] : w.rs[x] < w.rs[y]; }   // :799-800, filterByGroup's first
template <class W> MM_HD bool mm_chain_less_merge(const W& w, int x, int y) {
  if (w.sid[x] != w.sid[y]) return w.sid[x] < w.sid[y];
  if (w.rs[x] != w.rs[y]) return w.rs[x] < w.rs[y];
  return w.qs[x] < w.qs[y];
}
template <class W> MM_HD bool mm_chain_less_query(const W& w, int x, int y) {
  if (w.qs[x] != w.qs[y]) return w.qs[x] < w.qs[y];
  if (w.sid[x] != w.sid[y]) return w.sid[x] < w.sid[y];
  return w.rs[x] < w.rs[y];
}
// a working set of at most 16 records never leaves __insertion_sort: its kernel does not carry introsort's range stack
template <class W, class Less>
MM_HD void mm_chain_sort(W& w, int b, int e, Less less) {
  if constexpr (W::CAP <= MM_STDSORT_THRESHOLD) mm_std_insertion_sort(w.v, b, e, less);
  else mm_std_sort(w.v + b, e - b, less);
}
template <class W> MM_HD void mm_chain_sort_ref(W& w, int b, int e) { mm_chain_sort(w, b, e, [&w](int x, int y) { return mm_chain_less_ref(w, x, y); }); }
template <class W> MM_HD void mm_chain_sort_merge(W& w, int m) { mm_chain_sort(w, 0, m, [&w](int x, int y) { return mm_chain_less_merge(w, x, y); }); }
template <class W> MM_HD void mm_chain_sort_smid(W& w, int m) { mm_chain_sort(w, 0, m, [&w](int x, int y) { return w.smid[x] < w.smid[y]; }); }
template <class W> MM_HD void mm_chain_sort_query(W& w, int b, int e) { mm_chain_sort(w, b, e, [&w](int x, int y) { return mm_chain_less_query(w, x, y); }); }

// ---- prepare one record: record r of a fragment of length Qlen and complexity kc that passed the gate becomes member x (v[x] = x).
// qs / qe are the read's coordinates at once (:632-636 sets them behind the fragment's sort, to the same values for every record of the
// fragment).  false: the record names an entry outside the identity table or, with refGroup set, a contig outside [0, nContigs) -- not a
// hand-over cause but an error (k_l2_select writes shared <= Qs <= sketchSize and the index's own contig ids): nothing is read outside
// either array, and the caller reports it (mm_chain_reads: MM_ERR_STATE, "corrupt record")
template <class W>
MM_HD bool mm_chain_prepare(const mm_chain_env& E, W& w, int x, const mm_mapping& r, bool split, float kc) {
  if ((uint32_t)r.sketchSize >= (uint32_t)E.stride || (uint32_t)r.conservedSketches >= (uint32_t)E.stride) return false;
  if (E.refGroup && (uint32_t)r.refSeqId >= (uint32_t)E.nContigs) return false;
  const int32_t Qlen = r.fragLen;
  w.v[x] = (typename W::ID)x;
  w.ident[x] = E.identity[(size_t)r.sketchSize * (size_t)E.stride + (size_t)r.conservedSketches];
  w.rs[x] = r.refStartPos; w.re[x] = r.refStartPos + Qlen;
  w.qs[x] = split ? r.fragStart : 0; w.qe[x] = w.qs[x] + Qlen;
  w.sid[x] = r.refSeqId; w.sk[x] = r.sketchSize; w.cons[x] = r.conservedSketches;
  w.blk[x] = Qlen;                                                 // max(refEnd - refStart, queryEnd - queryStart)
  w.approx[x] = mm_chain_approx(w.ident[x], Qlen);
  w.strand[x] = (int8_t)r.strand; w.kc[x] = (double)kc;
  w.nm[x] = 0; w.smid[x] = 0; w.discard[x] = 0;
  return true;
}

// ---- the pair loop's inner part for member i of the sorted order: the position j > i of the partner with the least (dist + score, j), -1
// when no pair passes dist < max_dist.  Reads the working set only: the m calls are independent of each other.
template <class W>
MM_HD int mm_chain_partner(const W& w, int m, int i, int max_dist) {
  const int a = w.v[i];
  bool have = false; double bestKey = 0; int bestJ = -1;
  for (int j = i + 1; j < m; j++) {
    const int b = w.v[j];
    if (w.sid[b] != w.sid[a] || w.rs[b] > w.re[a] + max_dist) break;
    if (w.strand[b] != w.strand[a]) continue;
    const int ref_dist = w.rs[b] - w.re[a];
    int query_dist;
    if (w.strand[a] == 1 && w.qs[a] <= w.qs[b]) query_dist = w.qs[b] - w.qe[a];
    else if (w.strand[a] != 1 && w.qe[a] >= w.qe[b]) query_dist = w.qs[a] - w.qe[b];
    else continue;                                                 // dist stays at the double's maximum
    const double qd = (double)query_dist, rd = (double)ref_dist, df = (double)(query_dist - ref_dist);
    const double dist = mm_chain_sqrt(qd * qd + rd * rd);
    const double score = df * df;
    if (dist < (double)max_dist) {
      const double key = dist + score;
      if (!have || key < bestKey) { have = true; bestKey = key; bestJ = j; }     // the front of the sorted (key, id) pairs: ids ascend with j
    }
  }
  return bestJ;
}

template <class W>
MM_HD int mm_chain_find(W& w, int x) {
  while (w.uf.parent[x] != x) { w.uf.parent[x] = w.uf.parent[w.uf.parent[x]]; x = w.uf.parent[x]; }
  return x;
}

// ---- DisjointSets::unite (dset64.hpp:93-125) of positions i and j
template <class W>
MM_HD void mm_chain_unite(W& w, int i, int j) {
  int x = mm_chain_find(w, i), y = mm_chain_find(w, j);
  if (x == y) return;
  if (w.uf.rnk[x] > w.uf.rnk[y] || (w.uf.rnk[x] == w.uf.rnk[y] && x < y)) { const int t = x; x = y; y = t; }     // x goes under y
  w.uf.parent[x] = (typename W::ID)y;
  if (w.uf.rnk[x] == w.uf.rnk[y]) w.uf.rnk[y]++;
}

// ---- finish one chain: v[it, end) are its members in the order the sort by splitMappingId left them, v[it] its representative.
// Extents, the two averages in member order, block length, approxMatches (from the representative's own identity), n_merged.  Writes the
// representative's entries only, and no other chain reads them.
template <class W>
MM_HD void mm_chain_finish_chain(W& w, int it, int end) {
  const int rep = w.v[it];
  const float repIdent = w.ident[rep];
  int32_t qs = w.qs[rep], qe = w.qe[rep], rs = w.rs[rep], re = w.re[rep];
  double sumI = 0.0, sumK = 0.0;
  for (int j = it; j < end; j++) {
    const int x = w.v[j];
    qs = w.qs[x] < qs ? w.qs[x] : qs;
    rs = w.rs[x] < rs ? w.rs[x] : rs;
    qe = w.qe[x] > qe ? w.qe[x] : qe;
    re = w.re[x] > re ? w.re[x] : re;
    sumI = sumI + (double)w.ident[x];
    sumK = sumK + w.kc[x];
  }
  w.qs[rep] = qs; w.qe[rep] = qe; w.rs[rep] = rs; w.re[rep] = re;
  const int32_t dr = re - rs, dq = qe - qs;
  w.blk[rep] = dr > dq ? dr : dq;
  w.approx[rep] = mm_chain_approx(repIdent, w.blk[rep]);
  w.nm[rep] = end - it;
  w.ident[rep] = (float)(sumI / (double)w.nm[rep]);
  w.kc[rep] = sumK / (double)w.nm[rep];
}

// ---- the sweep: filterQueryAxis over the run v[b, e) (e - b > 1), sorted by (queryStartPos, refSeqId, refStartPos); ids of the sweep are
// positions in v (absolute: b .. e - 1).  An event is (pos, BEGIN = 1 / END = 2, id) in one word; marks the survivors with discard == 0.
// Scratch: ev[2b, 2e) and status[b, e) -- two runs share nothing.
template <class W>
MM_HD void mm_chain_sweep(W& w, int b, int e, int secondaryToKeep) {
  uint64_t* ev = w.sw.ev + 2 * b;
  const int m = e - b;
  for (int i = 0; i < m; i++) {
    const int x = w.v[b + i];
    w.discard[x] = 1;
    ev[2 * i] = ((uint64_t)((uint32_t)w.qs[x] ^ 0x80000000u) << 12) | (1u << 10) | (uint64_t)(b + i);
    ev[2 * i + 1] = ((uint64_t)((uint32_t)w.qe[x] ^ 0x80000000u) << 12) | (2u << 10) | (uint64_t)(b + i);
  }
  const int nE = 2 * m;
  mm_std_heap_sort(ev, 0, nE, [](uint64_t x, uint64_t y) { return x < y; });     // distinct words: any sort does
  // better(x, y): std::tie(identity as double, queryStartPos, refSeqId) of x > that of y
  auto better = [&w](int x, int y) {
    const int a = w.v[x], b = w.v[y];
    if (w.ident[a] != w.ident[b]) return w.ident[a] > w.ident[b];
    if (w.qs[a] != w.qs[b]) return w.qs[a] > w.qs[b];
    return w.sid[a] > w.sid[b]; };
  typename W::ID* status = w.sw.status + b;
  int nS = 0;
  for (int i = 0; i < nE;) {
    int j = i;
    while (j < nE && (ev[j] >> 12) == (ev[i] >> 12)) j++;
    for (int e = i; e < j; e++) {
      const int id = (int)(ev[e] & 1023u);
      int at = 0;
      while (at < nS && better(status[at], id)) at++;              // lower bound
      const bool equivalent = at < nS && !better(id, status[at]);
      if (((ev[e] >> 10) & 3u) == 1u) {
        if (!equivalent) { for (int t = nS; t > at; t--) status[t] = status[t - 1]; status[at] = (typename W::ID)id; nS++; }
      } else if (equivalent) {
        for (int t = at; t + 1 < nS; t++) status[t] = status[t + 1];
        nS--;
      }
    }
    if (nS > 0) {                                                  // markGood (filter.hpp:77-95)
      const float best = w.ident[w.v[status[0]]];
      int kept = 0;
      for (int t = 0; t < nS; t++) {
        const int x = w.v[status[t]];
        const bool worseOrSeen = best > w.ident[x] || w.discard[x] == 0;
        if (worseOrSeen && kept > secondaryToKeep) break;
        w.discard[x] = 0;
        ++kept;
      }
    }
    i = j;
  }
}

// ---- behind the chains' extents: the representatives (the first of every run of equal splitMappingId in v[0, m)) in order, then
// filterWeakMappings over them; -> new m
template <class W>
MM_HD int mm_chain_keep(const mm_chain_env& E, W& w, int m, int32_t queryLen, bool merged) {
  int k = 0;
  if (merged) {
    int32_t last = 0;
    for (int it = 0; it < m; it++) {
      const int x = w.v[it];
      const int32_t id = w.smid[x];
      if (it == 0 || id != last) w.v[k++] = (typename W::ID)x;
      last = id;
    }
    m = k; k = 0;
  }
  for (int i = 0; i < m; i++) if (!(queryLen > w.blk[w.v[i]] && w.nm[w.v[i]] < E.p.minMerged)) w.v[k++] = w.v[i];     // filterWeakMappings
  return k;
}

// ---- filterByGroup, query axis, over v[0, m), step by step
// secondaryToKeep of a read (:675-677 and the cast of :544)
MM_HD int mm_chain_secondary(const mm_chain_env& E, int32_t readLen) { return (int)(uint16_t)(readLen < E.segLength ? E.p.secondaryShort : E.p.secondarySegment); }
// the end of the run that starts at b < m: std::find_if_not over the members of the first one's group (:523-526); without groups, m
template <class W>
MM_HD int mm_chain_run_end(const mm_chain_env& E, const W& w, int m, int b) {
  if (!E.refGroup) return m;
  const int32_t g = E.refGroup[w.sid[w.v[b]]];
  int e = b + 1;
  while (e < m && E.refGroup[w.sid[w.v[e]]] == g) e++;
  return e;
}
// one run: the sort by the query key, the sweep of more than one member; its survivors have discard == 0
template <class W>
MM_HD void mm_chain_filter_run(const mm_chain_env& E, W& w, int b, int e, int secondaryToKeep) {
  (void)E;
  mm_chain_sort_query(w, b, e);
  if (e - b > 1) mm_chain_sweep(w, b, e, secondaryToKeep);
  else w.discard[w.v[b]] = 0;
}
// behind the runs: the survivors in order, then the final sort; -> new m
template <class W>
MM_HD int mm_chain_filter_compact(W& w, int m) {
  int k = 0;
  for (int i = 0; i < m; i++) if (w.discard[w.v[i]] == 0) w.v[k++] = w.v[i];
  mm_chain_sort_query(w, 0, k);
  return k;
}
// all of it on one thread; -> new m.  *runs (when non-null) receives the number of runs swept or passed through
template <class W>
MM_HD int mm_chain_filter(const mm_chain_env& E, W& w, int m, int32_t readLen, int* runs = nullptr) {
  if (runs) *runs = 0;
  if (E.p.filter != MM_CHAIN_FILTER_QUERY) return m;
  const int secondaryToKeep = mm_chain_secondary(E, readLen);
  mm_chain_sort_ref(w, 0, m);
  int nRuns = 0;
  for (int b = 0; b < m;) {
    const int e = mm_chain_run_end(E, w, m, b);
    mm_chain_filter_run(E, w, b, e, secondaryToKeep);
    nRuns++;
    b = e;
  }
  if (runs) *runs = nRuns;
  return mm_chain_filter_compact(w, m);
}

// ---- emit one row: member x
template <class W>
MM_HD mm_chain_row mm_chain_emit(const W& w, int x, int32_t querySeqId, int32_t queryLen) {
  mm_chain_row r;
  r.querySeqId = querySeqId; r.queryLen = queryLen; r.queryStartPos = w.qs[x]; r.queryEndPos = w.qe[x];
  r.refSeqId = w.sid[x]; r.refStartPos = w.rs[x]; r.refEndPos = w.re[x]; r.strand = w.strand[x];
  r.conservedSketches = w.cons[x]; r.sketchSize = w.sk[x]; r.blockLength = w.blk[x]; r.approxMatches = w.approx[x];
  r.n_merged = w.nm[x]; r.splitMappingId = w.smid[x];
  r.nucIdentity = w.ident[x]; r.pad_ = 0; r.kmerComplexity = w.kc[x];
  return r;
}

// the whole tail on one thread, 1 <= n <= W::CAP
template <class W>
MM_HD int mm_chain_read_t(const mm_chain_env& E, W& w, const mm_mapping* recs, int n, int32_t readLen, mm_chain_row* out, int* runs = nullptr) {
  int m = 0;
  if (runs) *runs = 0;
  const bool split = !E.noSplit && readLen > E.segLength;         // :587
  const int32_t querySeqId = recs[0].querySeqId;

  // ---- per fragment: mapSingleQueryFrag's gate and sort, then the read's coordinates
  for (int p = 0; p < n;) {
    int q = p;
    while (q < n && recs[q].fragStart == recs[p].fragStart) q++;
    const float kc = mm_chain_kmer_complexity(recs[p].maxHash, recs[p].rawSketchSize, recs[p].fragLen, E.kmerSize);
    if (!(kc < E.p.kmerComplexityThreshold)) {                    // :1137
      const int b = m;
      for (int i = p; i < q; i++) if (!mm_chain_prepare(E, w, m++, recs[i], split, kc)) return MM_CHAIN_BAD_RECORD;
      mm_chain_sort_ref(w, b, m);                                  // :799-800
    }
    p = q;
  }
  const int32_t queryLen = split ? readLen : recs[0].fragLen;     // (a read that is one fragment: Qlen == len)

  // ---- mergeMappingsInRange + filterWeakMappings
  if (split && E.p.merge) {
    if (m >= 2) {
      mm_chain_sort_merge(w, m);
      for (int i = 0; i < m; i++) { w.uf.parent[i] = (typename W::ID)i; w.uf.rnk[i] = 0; w.smid[w.v[i]] = i; }
      for (int i = 0; i < m; i++) {
        const int j = mm_chain_partner(w, m, i, E.p.chainGap);
        if (j >= 0) mm_chain_unite(w, i, j);
      }
      for (int i = 0; i < m; i++) w.smid[w.v[i]] = mm_chain_find(w, w.smid[w.v[i]]);
      mm_chain_sort_smid(w, m);
      for (int it = 0; it < m;) {
        int end = it;
        while (end < m && w.smid[w.v[end]] == w.smid[w.v[it]]) end++;
        mm_chain_finish_chain(w, it, end);
        it = end;
      }
    }
    m = mm_chain_keep(E, w, m, queryLen, m >= 2);
  }

  m = mm_chain_filter(E, w, m, readLen, runs);

  if (out) for (int i = 0; i < m; i++) out[i] = mm_chain_emit(w, w.v[i], querySeqId, queryLen);
  return m;
}

// Finishes the read of length readLen whose records are recs[0, n), in mm_mappings_download's order.  Writes the surviving mappings to
// out (when non-null; up to n of them), in the order filterByGroup leaves them, and returns their number; -1 for n above
// MM_CHAIN_MAX_RECORDS (the read is not taken), MM_CHAIN_BAD_RECORD for a record outside the identity table.
// *runs (when non-null): the runs filterByGroup walked for this read -- 0 with MM_CHAIN_FILTER_NONE or when nothing reached the filter,
// 1 without refGroup, the read's stretches of equal reference group with it; 0 for a read that is not taken or in error.
MM_HD int mm_chain_read(const mm_chain_env& E, const mm_mapping* recs, int n, int32_t readLen, mm_chain_row* out, int* runs = nullptr) {
  if (runs) *runs = 0;
  if (n > MM_CHAIN_MAX_RECORDS) return -1;
  if (n <= 0) return 0;
  mm_chain_work W;
  const int rows = mm_chain_read_t(E, W, recs, n, readLen, out, runs);
  if (rows < 0 && runs) *runs = 0;
  return rows;
}

// The same for a read of up to MM_CHAIN_LONG_MAX_RECORDS (512) records in the working set W the caller provides (39 KB: not for a
// device stack); -1 above that.  For n <= 16 the rows are mm_chain_read's.
MM_HD int mm_chain_read_long(const mm_chain_env& E, mm_chain_work_long& W, const mm_mapping* recs, int n, int32_t readLen, mm_chain_row* out, int* runs = nullptr) {
  if (runs) *runs = 0;
  if (n > MM_CHAIN_LONG_MAX_RECORDS) return -1;
  if (n <= 0) return 0;
  const int rows = mm_chain_read_t(E, W, recs, n, readLen, out, runs);
  if (rows < 0 && runs) *runs = 0;
  return rows;
}
